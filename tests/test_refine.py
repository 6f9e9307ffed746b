"""Host-only tests of the global refinement and the staircase
(dpo_amd.refine) through the cpu_ref ops.

References: solver.truncated_cg for the tCG, vectors recomputed from
their definitions for the model decrease, and a dense
numpy.linalg.eigvalsh of S for the certificate verdicts.
"""
import functools
import math

import numpy as np
import pytest
import torch

from dpo_amd.certify import (CertificateStatus, certificate_operator,
                             certify_solution)
from dpo_amd.ops import cpu_ref as cr
from dpo_amd.quadratic import QuadraticProblem, assemble_connection_laplacian
from dpo_amd.refine import (certified_solve, default_grad_tol,
                            refine_to_critical)
from dpo_amd.solver import TRParams, truncated_cg
from dpo_amd.types import RelativeSEMeasurement

EPS = np.finfo(np.float64).eps


# --------------------------------------------------------------------
# shared cases (also used by test_refine_gpu.py); cached, never mutated
# --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case():
    """grid3d(side=3, seed=0) at r = 5: (meas, n, Q, X_chordal)."""
    from dpo_amd.chordal import chordal_initialization
    from dpo_amd.manifold import lifting_matrix
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=3, seed=0)
    d, r = 3, 5
    T = chordal_initialization(d, n, meas)
    X0 = torch.from_numpy(
        np.ascontiguousarray((lifting_matrix(d, r) @ T).T))
    return meas, n, assemble_connection_laplacian(meas, n, d), X0


@functools.lru_cache(maxsize=None)
def ring_case(n):
    """Twisted SE(2) ring as in test_certify.py: identity edges k -> k+1
    mod n, X_k = Rot(2 pi k / n); exactly critical, not optimal (all
    poses identity has cost 0)."""
    meas = [RelativeSEMeasurement(0, 0, k, (k + 1) % n, np.eye(2),
                                  np.zeros(2), 1.0, 1.0)
            for k in range(n)]
    X = torch.zeros(3 * n, 2, dtype=torch.float64)
    for k in range(n):
        a = 2 * math.pi * k / n
        X[3 * k, 0], X[3 * k, 1] = math.cos(a), math.sin(a)
        X[3 * k + 1, 0], X[3 * k + 1, 1] = -math.sin(a), math.cos(a)
    return meas, n, assemble_connection_laplacian(meas, n, 2), X


def dense_S(Q, Xt, d):
    """Q - blockdiag(Lambda), Lambda from its formula."""
    X = Xt.numpy()
    QX = Q.to_scipy() @ X
    dh = d + 1
    S = Q.to_scipy().toarray()
    for i in range(X.shape[0] // dh):
        A = QX[i * dh:i * dh + d] @ X[i * dh:i * dh + d].T
        S[i * dh:i * dh + d, i * dh:i * dh + d] -= 0.5 * (A + A.T)
    return S


def jacobi_problem(Q, n, d, r):
    problem = QuadraticProblem(n, d, r, precond="jacobi")
    problem.set_q(Q)
    return problem, ("jacobi", problem._Lpre.contiguous())


def run_tcg(Q, X, d, pre, radius, max_inner=1000, chunk=3):
    """Head, then refine_tcg_steps in chunks of `chunk` until the tCG
    ends. Returns (workspace, control as a list)."""
    ws = cr.RefineWorkspace(X)
    ctl = cr.refine_control(0.0, radius, max_inner)
    cr.refine_head(Q, ws, ctl, d, pre)
    assert ctl[cr.RF_STATUS] == cr.RS_RUN
    for _ in range(max_inner):
        cr.refine_tcg_steps(Q, ws, ctl, d, pre, chunk)
        if ctl[cr.RF_STATUS] != cr.RS_RUN:
            break
    assert ctl[cr.RF_STATUS] == cr.RS_TCG_DONE
    return ws, ctl.tolist()


@functools.lru_cache(maxsize=None)
def boundary_radii():
    """Radii at which the grid's tCG leaves the trust region in iteration
    0 and in iteration 2: from the preconditioned step lengths sqrt(e_Pe)
    after each iteration of an unconstrained run."""
    meas, n, Q, X0 = grid_case()
    _, pre = jacobi_problem(Q, n, 3, 5)
    ws = cr.RefineWorkspace(X0)
    ctl = cr.refine_control(0.0, 1e6, 1000)
    cr.refine_head(Q, ws, ctl, 3, pre)
    lengths = []
    for _ in range(3):
        cr.refine_tcg_steps(Q, ws, ctl, 3, pre, 1)
        assert ctl[cr.RF_STATUS] == cr.RS_RUN
        lengths.append(math.sqrt(float(ctl[cr.RF_EPE])))
    assert lengths[0] < lengths[1] < lengths[2]
    return 0.5 * lengths[0], 0.5 * (lengths[1] + lengths[2])


# --------------------------------------------------------------------
# 1. tCG against solver.truncated_cg
# --------------------------------------------------------------------
@pytest.mark.parametrize("which", ["converge", "boundary0", "boundary2"])
def test_tcg_matches_host_solver(which):
    meas, n, Q, X0 = grid_case()
    d, r = 3, 5
    problem, pre = jacobi_problem(Q, n, d, r)
    radius = {"converge": 10.0, "boundary0": boundary_radii()[0],
              "boundary2": boundary_radii()[1]}[which]
    grad = problem.rie_grad(X0)
    p = TRParams(max_inner_iterations=1000)
    eta_ref, Heta_ref, status = truncated_cg(problem, X0, grad, radius, p)
    ws, c = run_tcg(Q, X0, d, pre, radius)
    assert cr.REFINE_TCG_NAMES[int(c[cr.RF_TCG])] == status
    iters = int(c[cr.RF_ITER])
    if which == "converge":
        assert status == "converged" and c[cr.RF_HIT] == 0.0
    else:
        assert status == "exceeded_tr" and c[cr.RF_HIT] == 1.0
        assert iters == (1 if which == "boundary0" else 3)
    # Propagated bound: both runs evaluate the same
    # recurrence; each of the `iters` iterations adds, relative to the
    # scale of its vectors, the rounding of one Hessian row sum (K <= 7
    # blocks * 4 terms), two projections and the dots behind alpha and
    # beta (K = N r terms): 2 K eps each.
    K = ws.eta.numel()
    bound = iters * 2 * K * EPS * float(eta_ref.abs().max())
    print(f"{which}: iters {iters}, max err "
          f"{float((ws.eta - eta_ref).abs().max()):.3e}, bound {bound:.3e}")
    assert float((ws.eta - eta_ref).abs().max()) <= bound


# --------------------------------------------------------------------
# 2. scalar model decrease
# --------------------------------------------------------------------
@pytest.mark.parametrize("which", ["converge", "boundary0", "boundary2"])
def test_model_decrease_matches_vectors(which):
    meas, n, Q, X0 = grid_case()
    d, r = 3, 5
    problem, pre = jacobi_problem(Q, n, d, r)
    radius = {"converge": 10.0, "boundary0": boundary_radii()[0],
              "boundary2": boundary_radii()[1]}[which]
    ws, c = run_tcg(Q, X0, d, pre, radius)
    Heta = problem.manifold.project_tangent(X0, problem.hess_vec(ws.eta))
    g_eta = float((ws.grad * ws.eta).sum())
    e_He = float((ws.eta * Heta).sum())
    dm = -g_eta - 0.5 * e_He
    # the two sums as computed, plus the CG identities behind the
    # recurrence (r_j orthogonal to delta_{j-1}), which hold to the same
    # propagated rounding as the tCG parity above
    K = ws.eta.numel()
    scale = float((ws.grad.abs() * ws.eta.abs()).sum()
                  + 0.5 * (ws.eta.abs() * Heta.abs()).sum())
    bound = int(c[cr.RF_ITER]) * 2 * K * EPS * scale
    print(f"{which}: dm {dm:.12e} scalar {c[cr.RF_DM]:.12e} "
          f"bound {bound:.3e}")
    assert dm > 0
    assert abs(c[cr.RF_DM] - dm) <= bound


# --------------------------------------------------------------------
# 3. refine from the chordal initialisation, then certify
# --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_refined():
    meas, n, Q, X0 = grid_case()
    return refine_to_critical(Q, X0, precond="jacobi")


def test_refine_from_chordal_reaches_gate_and_certifies():
    meas, n, Q, X0 = grid_case()
    res = grid_refined()
    assert res.status == "CONVERGED"
    assert res.grad_tol == default_grad_tol(Q, X0)
    _, gn = certificate_operator(Q, res.Xt)
    assert gn <= res.grad_tol
    assert res.f_final <= res.f_init
    assert res.outer_steps >= 1 and res.inner_iterations >= 1
    assert res.as_dict()["refine_status"] == "CONVERGED"
    cert = certify_solution(meas, n, 3, res.Xt)
    assert cert.status == CertificateStatus.CERTIFIED


# --------------------------------------------------------------------
# 4. staircase on the twisted ring
# --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring_staircase(max_rank=None):
    meas, n, Q, X = ring_case(67)
    return certified_solve(meas, n, 2, X, max_rank=max_rank)


def test_staircase_ring67_certifies_at_rank_4():
    meas, n, Q, X = ring_case(67)
    res = ring_staircase()
    ranks = [lv.rank for lv in res.levels]
    verdicts = [lv.certificate.status for lv in res.levels]
    fs = [lv.refine.f_final for lv in res.levels]
    print(ranks, verdicts, fs)
    assert ranks == [2, 3, 4]
    assert verdicts == [CertificateStatus.NOT_OPTIMAL,
                        CertificateStatus.NOT_OPTIMAL,
                        CertificateStatus.CERTIFIED]
    assert fs[0] > fs[1] > fs[2]
    assert res.status == CertificateStatus.CERTIFIED and res.rank == 4
    assert res.Xt.shape == (3 * n, 4)
    # level 0 is already critical: refine is a no-op
    assert res.levels[0].refine.inner_iterations == 0
    assert torch.equal(res.levels[0].refine.Xt, X)
    eta = 1e-6 * res.certificate.lambda_max
    evals = np.linalg.eigvalsh(dense_S(Q, res.Xt, 2))
    assert evals[0] >= -eta
    # the optimum is exactly 0 (all poses identity)
    assert fs[2] <= 1e-12 * fs[0]
    d = res.as_dict()
    assert d["staircase_levels"] == 3 and d["final_rank"] == 4
    assert d["certificate"] == "certified"


def test_staircase_max_rank_stops_not_optimal():
    res = ring_staircase(3)
    assert res.status == CertificateStatus.NOT_OPTIMAL and res.rank == 3
    assert [lv.rank for lv in res.levels] == [2, 3]


# --------------------------------------------------------------------
# 5. error cases
# --------------------------------------------------------------------
def test_uncompiled_shape_raises():
    meas, n, Q, X = ring_case(67)
    X7 = torch.zeros(3 * n, 7, dtype=torch.float64)
    X7[:, :2] = X
    with pytest.raises(ValueError):
        refine_to_critical(Q, X7)
    with pytest.raises(ValueError):
        certified_solve(meas, n, 2, X7)


def test_max_outer_zero_returns_input():
    meas, n, Q, X0 = grid_case()
    res = refine_to_critical(Q, X0, max_outer=0)
    assert res.status == "MAX_OUTER"
    assert torch.equal(res.Xt, X0)
    assert res.outer_steps == 0 and res.inner_iterations == 0
    assert res.f_final == res.f_init
    assert res.grad_norm_final == res.grad_norm_init > res.grad_tol


def test_critical_input_converges_without_tcg():
    meas, n, Q, X = ring_case(67)
    res = refine_to_critical(Q, X, precond="jacobi")
    assert res.status == "CONVERGED"
    assert res.inner_iterations == 0 and res.outer_steps == 0
    assert torch.equal(res.Xt, X)
