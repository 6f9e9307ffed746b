"""Host-only tests of the optimality certificate (dpo_amd.certify).

Reference: a dense numpy.linalg.eigvalsh of Q.to_scipy() - blockdiag(Lambda)
with Lambda built here from its formula, not through the code under test.
"""
import functools
import math

import numpy as np
import pytest
import torch

from dpo_amd.certify import (BasisBudgetError, CertificateStatus,
                             certificate_operator, certify_solution,
                             escape_direction)
from dpo_amd.quadratic import QuadraticProblem, assemble_connection_laplacian
from dpo_amd.types import RelativeSEMeasurement


# --------------------------------------------------------------------
# shared cases (also used by test_certify_gpu.py); cached, never mutated
# --------------------------------------------------------------------
def dense_lambda(Q, Xt, d):
    """blockdiag(Lambda) (N, N) from the formula: per pose the top-left
    d x d block 0.5 sum_k (QX[a,k] X[b,k] + QX[b,k] X[a,k])."""
    X = Xt.numpy()
    QX = Q.to_scipy() @ X
    dh = d + 1
    n = X.shape[0] // dh
    L = np.zeros((n * dh, n * dh))
    for i in range(n):
        for a in range(d):
            for b in range(d):
                L[i * dh + a, i * dh + b] = 0.5 * sum(
                    QX[i * dh + a, k] * X[i * dh + b, k]
                    + QX[i * dh + b, k] * X[i * dh + a, k]
                    for k in range(X.shape[1]))
    return L


def dense_S(Q, Xt, d):
    return Q.to_scipy().toarray() - dense_lambda(Q, Xt, d)


@functools.lru_cache(maxsize=None)
def ring_case(n):
    """Twisted SE(2) ring: identity edges k -> k+1 mod n, X_k = Rot(2 pi
    k / n). Exactly critical, lambda_min(S) = 2 cos(2 pi / n) - 2."""
    meas = [RelativeSEMeasurement(0, 0, k, (k + 1) % n, np.eye(2),
                                  np.zeros(2), 1.0, 1.0)
            for k in range(n)]
    X = torch.zeros(3 * n, 2, dtype=torch.float64)
    for k in range(n):
        a = 2 * math.pi * k / n
        # row c of the pose block is column c of Rot(a)
        X[3 * k, 0], X[3 * k, 1] = math.cos(a), math.sin(a)
        X[3 * k + 1, 0], X[3 * k + 1, 1] = -math.sin(a), math.cos(a)
    Q = assemble_connection_laplacian(meas, n, 2)
    return meas, n, Q, X, 2 * math.cos(2 * math.pi / n) - 2


@functools.lru_cache(maxsize=None)
def grid_case():
    """grid3d(side=3, seed=0) lifted to r = 5: (meas, n, Q, X_chordal,
    X_solved), solved from the chordal initialisation on the host."""
    from dpo_amd.chordal import chordal_initialization
    from dpo_amd.manifold import lifting_matrix
    from dpo_amd.solver import QuadraticOptimizer, TRParams
    from dpo_amd.synthetic import grid3d
    from dpo_amd.types import OptAlgorithm
    meas, n = grid3d(side=3, seed=0)
    d, r = 3, 5
    T = chordal_initialization(d, n, meas)
    X0 = torch.from_numpy(
        np.ascontiguousarray((lifting_matrix(d, r) @ T).T))
    Q = assemble_connection_laplacian(meas, n, d)
    problem = QuadraticProblem(n, d, r)
    problem.set_q(Q)
    opt = QuadraticOptimizer(
        problem, OptAlgorithm.RTR,
        TRParams(tolerance=1e-7, max_iterations=50,
                 max_inner_iterations=200))
    X = opt.optimize(X0.clone())
    return meas, n, Q, X0, X


@functools.lru_cache(maxsize=None)
def grid_reference():
    """Dense eigenvalues of S at the solved grid iterate."""
    meas, n, Q, _, X = grid_case()
    return np.linalg.eigvalsh(dense_S(Q, X, 3))


# --------------------------------------------------------------------
# 1. operator
# --------------------------------------------------------------------
def test_operator_matches_dense_construction():
    from dpo_amd.manifold import LiftedSEManifold
    meas, n, Q, _, _ = grid_case()
    d, r = 3, 5
    g = torch.Generator().manual_seed(3)
    X = LiftedSEManifold(r, d, n).random_point(generator=g)
    lam, gn = certificate_operator(Q, X)
    L = dense_lambda(Q, X, d)
    dh = d + 1
    ref = np.stack([L[i * dh:i * dh + d, i * dh:i * dh + d]
                    for i in range(n)])
    assert lam.shape == (n, d, d)
    assert np.allclose(lam.numpy(), ref, atol=1e-10, rtol=1e-12)
    SX = (Q.to_scipy().toarray() - L) @ X.numpy()
    assert np.isclose(gn, np.linalg.norm(SX), atol=1e-10, rtol=1e-12)
    problem = QuadraticProblem(n, d, r)
    problem.Q = Q
    assert np.allclose(SX, problem.rie_grad(X).numpy(),
                       atol=1e-10, rtol=1e-12)


# --------------------------------------------------------------------
# 2. twisted ring
# --------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 67])
def test_ring_not_optimal(n):
    meas, n, Q, X, lam_true = ring_case(n)
    res = certify_solution(meas, n, 2, X)
    S = dense_S(Q, X, 2)
    lmax = np.linalg.eigvalsh(S)[-1]
    print(f"ring n={n}: {res.status} lambda_min={res.lambda_min!r} "
          f"true={lam_true!r} residual={res.residual!r} "
          f"lambda_max={res.lambda_max!r} iters={res.iterations}")
    assert res.status == CertificateStatus.NOT_OPTIMAL
    assert abs(res.lambda_min - lam_true) <= max(res.residual, 1e-8 * lmax)
    v = res.direction.numpy()
    assert v.shape == (3 * n,)
    assert abs(np.linalg.norm(v) - 1.0) < 1e-12
    assert v @ S @ v < 0.0
    # n = 8: N = 24 < max_iters drives the breakdown guard
    assert res.iterations <= 3 * n
    for x in (res.lambda_min, res.lambda_max, res.residual, res.grad_norm):
        assert math.isfinite(x)
    assert np.isfinite(v).all()


# --------------------------------------------------------------------
# 3. escape
# --------------------------------------------------------------------
def test_escape_direction_descends_from_ring():
    meas, n, Q, X, _ = ring_case(8)
    res = certify_solution(meas, n, 2, X)
    X1 = escape_direction(Q, X, res.direction)
    assert X1.shape == (24, 3)
    Y = X1.view(n, 3, 3)[:, :2, :]
    eye = torch.eye(2, dtype=torch.float64).expand(n, 2, 2)
    assert torch.allclose(torch.bmm(Y, Y.transpose(1, 2)), eye, atol=1e-10)
    problem = QuadraticProblem(n, 2, 3)
    problem.Q = Q
    f0 = 16 - 8 * math.sqrt(2)          # 4.686291501015...
    f1 = problem.f(X1)
    print(f"escape: f {f0!r} -> {f1!r}")
    assert f1 < f0


def test_escape_direction_rejects_uncompiled_rank():
    meas, n, Q, X, _ = ring_case(8)
    X6 = torch.zeros(24, 6, dtype=torch.float64)
    X6[:, :2] = X
    with pytest.raises(ValueError):
        escape_direction(Q, X6, torch.ones(24, dtype=torch.float64))


# --------------------------------------------------------------------
# 4. solved grid, 5. not critical
# --------------------------------------------------------------------
def test_solved_grid_certified():
    meas, n, Q, _, X = grid_case()
    ev = grid_reference()
    res = certify_solution(meas, n, 3, X)
    print(f"grid: {res.status} lambda_min={res.lambda_min!r} "
          f"ref={ev[0]!r} residual={res.residual!r} "
          f"lambda_max={res.lambda_max!r} ref={ev[-1]!r} "
          f"grad={res.grad_norm!r} iters={res.iterations}")
    assert res.status == CertificateStatus.CERTIFIED
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, 1e-8 * ev[-1])
    assert abs(res.lambda_max - ev[-1]) <= 1e-6 * ev[-1]


def test_unsolved_grid_not_critical():
    meas, n, Q, X0, _ = grid_case()
    res = certify_solution(meas, n, 3, X0)
    print(f"chordal init: grad={res.grad_norm!r}")
    assert res.status == CertificateStatus.NOT_CRITICAL
    assert res.iterations == 0
    assert res.direction is None


# --------------------------------------------------------------------
# 6. weights, 7. budget
# --------------------------------------------------------------------
def test_zero_weight_equals_edge_removed():
    meas, n, Q, _, X = grid_case()
    lc = next(k for k, m in enumerate(meas) if m.p1 + 1 != m.p2)
    w = [1.0] * len(meas)
    w[lc] = 0.0
    Qw = assemble_connection_laplacian(meas, n, 3, w)
    Qr = assemble_connection_laplacian(meas[:lc] + meas[lc + 1:], n, 3)
    lam_w, gn_w = certificate_operator(Qw, X)
    lam_r, gn_r = certificate_operator(Qr, X)
    assert torch.allclose(lam_w, lam_r, atol=1e-10, rtol=1e-12)
    assert np.isclose(gn_w, gn_r, atol=1e-10, rtol=1e-12)
    assert np.allclose(dense_S(Qw, X, 3), dense_S(Qr, X, 3),
                       atol=1e-10, rtol=1e-12)
    # and through the public entry point: same verdict and numbers
    kw = dict(grad_tol=float("inf"), max_iters=48)
    a = certify_solution(meas, n, 3, X, weights=w, **kw)
    b = certify_solution(meas[:lc] + meas[lc + 1:], n, 3, X, **kw)
    assert a.status == b.status and a.iterations == b.iterations
    assert abs(a.lambda_min - b.lambda_min) <= 1e-8 * abs(a.lambda_max)
    full = certificate_operator(Q, X)[0]
    assert not torch.allclose(full, lam_w, atol=1e-10, rtol=1e-12)


def test_basis_budget_refused(monkeypatch):
    meas, n, Q, X, _ = ring_case(8)
    import dpo_amd.certify as C

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the budget check")
    monkeypatch.setattr(C, "assemble_connection_laplacian", no_alloc)
    monkeypatch.setattr(C.torch, "zeros", no_alloc)
    with pytest.raises(BasisBudgetError, match="basis_budget_bytes"):
        certify_solution(meas, n, 2, X, basis_budget_bytes=1)
