"""Host-only tests of the LOBPCG certificate path
(certify_solution(method="lobpcg"), docs/DESIGN.md §20).

Cases and the dense reference are those of test_certify.py. The whole
method runs through ops/cpu_ref.py here; the HIP ops are compared with
these in test_certify_lobpcg_gpu.py.
"""
import math

import numpy as np
import pytest
import torch

from test_certify import dense_S, grid_case, grid_reference, ring_case

from dpo_amd.certify import (BasisBudgetError, CertificateStatus,
                             certify_solution, default_block_size)

EPS = np.finfo(np.float64).eps


def s_inf(S):
    return float(np.abs(S).sum(axis=1).max())


def residual_bound(S, v, theta, resid):
    """Rounding bound on | ||S v - theta v|| computed in fp64 - the exact
    value |, for two computations (the code's and the dense one): each
    entry of S v - theta v is a sum of at most K = N + 1 products, so its
    error is below K eps (|S| |v| + |theta| |v|); the norm of that error
    vector bounds the change of the norm, and the norm itself (N squares)
    adds N eps relative."""
    N = len(v)
    a = np.abs(S) @ np.abs(v) + abs(theta) * np.abs(v)
    return 2 * (N + 1) * EPS * float(np.linalg.norm(a)) + 2 * N * EPS * resid


def check_direction(res, S, N):
    v = res.direction.cpu().numpy()
    assert v.shape == (N,)
    assert np.isfinite(v).all()
    assert abs(np.linalg.norm(v) - 1.0) < 1e-12
    return v


# --------------------------------------------------------------------
# solved grid
# --------------------------------------------------------------------
@pytest.mark.parametrize("block_size", [None, 3, 8])
@pytest.mark.parametrize("seed", [0, 1])
def test_grid_certified_exact(block_size, seed):
    meas, n, Q, _, X = grid_case()
    ev = grid_reference()
    S = dense_S(Q, X, 3)
    res = certify_solution(meas, n, 3, X, method="lobpcg",
                           block_size=block_size, precond="exact", seed=seed)
    print(f"grid m={block_size} seed={seed}: {res.status} "
          f"lambda_min={res.lambda_min!r} ref={ev[0]!r} "
          f"residual={res.residual!r} iters={res.iterations} "
          f"applications={res.applications} drops={res.basis_drops}")
    assert res.status == CertificateStatus.CERTIFIED
    assert res.method == "lobpcg" and res.precond == "exact"
    assert res.block_size == (6 if block_size is None else block_size)
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, 1e-8 * ev[-1])
    assert abs(res.lambda_max - ev[-1]) <= 1e-6 * ev[-1]
    assert 1 <= res.iterations <= 10
    # S was applied to at least the start block and one W block
    assert res.applications >= 2 * res.block_size
    v = check_direction(res, S, Q.N)
    true_resid = float(np.linalg.norm(S @ v - res.lambda_min * v))
    tol = residual_bound(S, v, res.lambda_min, true_resid)
    print(f"  residual {res.residual!r} dense {true_resid!r} tol {tol!r}")
    assert abs(res.residual - true_resid) <= tol
    d = res.as_dict()
    assert d["certificate_method"] == "lobpcg"
    assert d["certificate_block"] == res.block_size
    assert d["certificate_precond"] == "exact"
    assert d["certificate_applications"] == res.applications


def test_grid_certified_jacobi():
    """The preconditioner every large problem gets: more iterations, the
    same verdict."""
    meas, n, Q, _, X = grid_case()
    ev = grid_reference()
    res = certify_solution(meas, n, 3, X, method="lobpcg", precond="jacobi")
    print(f"grid jacobi: {res.status} lambda_min={res.lambda_min!r} "
          f"residual={res.residual!r} iters={res.iterations}")
    assert res.status == CertificateStatus.CERTIFIED
    assert res.precond == "jacobi"
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, 1e-8 * ev[-1])


def test_problem_handed_over(monkeypatch):
    """problem= is used as it is: nothing builds a second preconditioner."""
    from dpo_amd.quadratic import QuadraticProblem
    import dpo_amd.refine as R
    meas, n, Q, _, X = grid_case()
    problem = QuadraticProblem(n, 3, 5)
    problem.set_q(Q)

    def no_build(*a, **k):
        raise AssertionError("built a preconditioner although one was given")
    monkeypatch.setattr(R, "_preconditioner", no_build)
    a = certify_solution(meas, n, 3, X, method="lobpcg", problem=problem)
    assert a.status == CertificateStatus.CERTIFIED and a.precond == "exact"
    pair = ("exact", problem._lu)
    b = certify_solution(meas, n, 3, X, method="lobpcg", problem=pair)
    assert (b.status, b.lambda_min, b.iterations) == (
        a.status, a.lambda_min, a.iterations)


def test_certified_solve_builds_one_preconditioner(monkeypatch):
    """certified_solve(certify_kw={"method": "lobpcg"}) builds the
    preconditioner of Q once, for the refinement and the certificate."""
    import dpo_amd.refine as R
    meas, n, Q, _, X = grid_case()
    built = []
    real = R._preconditioner

    def counting(*a, **k):
        if not isinstance(a[4], tuple):
            built.append(a[4])
        return real(*a, **k)
    monkeypatch.setattr(R, "_preconditioner", counting)
    stair = R.certified_solve(meas, n, 3, X,
                              certify_kw={"method": "lobpcg"})
    assert stair.status == CertificateStatus.CERTIFIED
    assert stair.certificate.method == "lobpcg"
    assert stair.certificate.precond == "exact"
    assert built == ["auto"]
    assert stair.as_dict()["certificate_method"] == "lobpcg"


# --------------------------------------------------------------------
# twisted ring
# --------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 67])
@pytest.mark.parametrize("block_size", [3, 6])
@pytest.mark.parametrize("lmax_iters", [64, 4])
def test_ring_not_optimal(n, block_size, lmax_iters):
    """lmax_iters = 64: the lambda_max phase meets the witness itself;
    lmax_iters = 4: it cannot converge, eta comes from ||S||_inf and, on
    the 67 ring, LOBPCG has to find the witness."""
    meas, n, Q, X, lam_true = ring_case(n)
    S = dense_S(Q, X, 2)
    res = certify_solution(meas, n, 2, X, method="lobpcg",
                           block_size=block_size, lmax_iters=lmax_iters)
    print(f"ring n={n} m={block_size} lmax_iters={lmax_iters}: "
          f"{res.status} lambda_min={res.lambda_min!r} true={lam_true!r} "
          f"residual={res.residual!r} iters={res.iterations} "
          f"applications={res.applications}")
    assert res.status == CertificateStatus.NOT_OPTIMAL
    v = check_direction(res, S, 3 * n)
    # the largest eta the run can have used: 1e-6 ||S||_inf
    assert v @ S @ v < -1e-6 * s_inf(S)
    assert lam_true - 1e-9 <= res.lambda_min < 0.0
    for x in (res.lambda_min, res.lambda_max, res.residual, res.grad_norm):
        assert math.isfinite(x)
    if n == 67 and lmax_iters == 4:
        assert res.iterations >= 1      # LOBPCG, not Lanczos, decided


# --------------------------------------------------------------------
# gate, errors, budget, default method
# --------------------------------------------------------------------
def test_chordal_iterate_not_critical():
    meas, n, Q, X0, _ = grid_case()
    res = certify_solution(meas, n, 3, X0, method="lobpcg")
    assert res.status == CertificateStatus.NOT_CRITICAL
    assert res.iterations == 0 and res.applications == 0
    assert res.direction is None
    assert res.as_dict()["lambda_min"] is None


def test_argument_errors():
    meas, n, Q, X, _ = ring_case(8)            # d = 2, N = 24
    kw = dict(method="lobpcg")
    with pytest.raises(ValueError, match="block_size"):
        certify_solution(meas, n, 2, X, block_size=7, **kw)   # not compiled
    with pytest.raises(ValueError, match="block_size"):
        certify_solution(meas, n, 2, X, block_size=1, **kw)
    meas5, n5, _, X5, _ = ring_case(5)         # N = 15 < 3 * 6
    with pytest.raises(ValueError, match="3 m <= N"):
        certify_solution(meas5, n5, 2, X5, block_size=6, **kw)
    with pytest.raises(ValueError, match="method"):
        certify_solution(meas, n, 2, X, method="arnoldi")
    with pytest.raises(ValueError, match="basis_size"):
        certify_solution(meas, n, 2, X, basis_size=8, **kw)
    with pytest.raises(ValueError, match="keep"):
        certify_solution(meas, n, 2, X, keep=(2, 1), **kw)
    with pytest.raises(ValueError, match="precond"):
        certify_solution(meas, n, 2, X, precond="ilu", lmax_iters=2, **kw)
    with pytest.raises(ValueError, match="lobpcg"):
        certify_solution(meas, n, 2, X, block_size=3)   # Lanczos run


def test_default_block_size():
    assert default_block_size(3, 5, 108) == 6
    assert default_block_size(3, 8, 30000) == 8     # capped by the table
    assert default_block_size(2, 2, 24) == 3
    assert default_block_size(2, 5, 15) == 5        # 3 m <= N


def test_basis_budget_refused(monkeypatch):
    meas, n, Q, X, _ = ring_case(8)
    import dpo_amd.certify as C

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the budget check")
    monkeypatch.setattr(C, "assemble_connection_laplacian", no_alloc)
    monkeypatch.setattr(C.torch, "zeros", no_alloc)
    # N = 24, 25 Lanczos vectors and 7 blocks of 3 columns
    need = 8 * 24 * 25 + 8 * 7 * 24 * 3
    with pytest.raises(BasisBudgetError, match="basis_budget_bytes"):
        certify_solution(meas, n, 2, X, method="lobpcg",
                         basis_budget_bytes=need - 1)


def test_default_method_unchanged():
    meas, n, Q, _, X = grid_case()
    old = certify_solution(meas, n, 3, X)
    new = certify_solution(meas, n, 3, X, method="lanczos", precond="auto",
                           lmax_iters=64)
    assert old.as_dict() == new.as_dict()
    assert sorted(old.as_dict()) == [
        "certificate", "certificate_grad_norm", "certificate_iterations",
        "certificate_residual", "lambda_max", "lambda_min"]
    assert old.method == "lanczos" and old.basis_drops == 0
    assert torch.equal(old.direction, new.direction)


# --------------------------------------------------------------------
# degenerate basis
# --------------------------------------------------------------------
def test_exact_eigenvectors_in_the_start_block():
    """Two columns of the start block are exact eigenvectors (of the two
    largest eigenvalues): their residual, hence their column of W = T R,
    is zero to rounding and linearly dependent on X. Those columns are
    kept out of the Rayleigh-Ritz basis, the drop is counted, and the
    other columns still carry the run to its verdict."""
    meas, n, Q, _, X = grid_case()
    S = dense_S(Q, X, 3)
    ev, U = np.linalg.eigh(S)
    m = 6
    g = torch.Generator().manual_seed(4)
    start = torch.randn(Q.N, m, dtype=torch.float64, generator=g)
    start[:, 0] = torch.from_numpy(U[:, -1].copy())
    start[:, 1] = torch.from_numpy(U[:, -2].copy())
    res = certify_solution(meas, n, 3, X, method="lobpcg", block_size=m,
                           start_block=start)
    print(f"degenerate: {res.status} lambda_min={res.lambda_min!r} "
          f"residual={res.residual!r} iters={res.iterations} "
          f"drops={res.basis_drops}")
    assert res.status == CertificateStatus.CERTIFIED
    assert res.basis_drops >= 1
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, 1e-8 * ev[-1])
    for x in (res.lambda_min, res.lambda_max, res.residual):
        assert math.isfinite(x)
    assert torch.isfinite(res.direction).all()


def test_rank_deficient_start_block_refused():
    meas, n, Q, _, X = grid_case()
    start = torch.ones(Q.N, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="rank deficient"):
        certify_solution(meas, n, 3, X, method="lobpcg", start_block=start)
