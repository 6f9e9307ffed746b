"""Host-only tests of the thick-restart certificate path
(certify_solution(basis_size=b)). Cases and dense references are shared
with test_certify.py."""
import math

import numpy as np
import pytest
import torch

from dpo_amd.certify import (BREAKDOWN_TOL, BasisBudgetError,
                             CertificateStatus, _thick_restart,
                             certificate_operator, certify_solution,
                             default_keep)
from dpo_amd.ops import cpu_ref
from dpo_amd.ops.cpu_ref import CERT_HDR, CERT_KEEP_MAX, CERT_TOL

from test_certify import dense_S, grid_case, grid_reference, ring_case

EPS = np.finfo(np.float64).eps


def _show(tag, res):
    print(f"{tag}: {res.status} lambda_min={res.lambda_min!r} "
          f"residual={res.residual!r} lambda_max={res.lambda_max!r} "
          f"steps={res.iterations} restarts={res.restarts}")


# --------------------------------------------------------------------
# 1. ring67 in a window of 16
# --------------------------------------------------------------------
def test_ring67_restarted_not_optimal():
    meas, n, Q, X, lam_true = ring_case(67)
    b = 16
    res = certify_solution(meas, n, 2, X, basis_size=b, keep=(6, 2),
                           max_iters=1000)
    S = dense_S(Q, X, 2)
    lmax = np.linalg.eigvalsh(S)[-1]
    _show("ring67 b=16", res)
    assert res.status == CertificateStatus.NOT_OPTIMAL
    assert abs(res.lambda_min - lam_true) <= max(res.residual, 1e-8 * lmax)
    assert res.restarts >= 1
    assert res.iterations > b
    v = res.direction.numpy()
    assert v.shape == (3 * n,)
    assert np.isfinite(v).all()
    assert abs(np.linalg.norm(v) - 1.0) < 1e-12
    assert v @ S @ v < 0.0


# --------------------------------------------------------------------
# 2. solved grid in a window of 12
# --------------------------------------------------------------------
def test_grid_restarted_certified():
    meas, n, Q, _, X = grid_case()
    ev = grid_reference()
    res = certify_solution(meas, n, 3, X, basis_size=12, keep=(4, 2),
                           max_iters=1000)
    _show("grid b=12", res)
    assert res.status == CertificateStatus.CERTIFIED
    assert res.restarts >= 1
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, 1e-8 * ev[-1])
    assert abs(res.lambda_max - ev[-1]) <= 1e-6 * ev[-1]


# --------------------------------------------------------------------
# 3. window wider than the problem: breakdown before any restart
# --------------------------------------------------------------------
def test_ring8_window_wider_than_problem():
    meas, n, Q, X, _ = ring_case(8)
    ref = certify_solution(meas, n, 2, X)
    res = certify_solution(meas, n, 2, X, basis_size=16)
    _show("ring8 b=16", res)
    assert res.status == ref.status == CertificateStatus.NOT_OPTIMAL
    assert res.lambda_min == ref.lambda_min
    assert res.iterations == ref.iterations
    assert res.restarts == 0


# --------------------------------------------------------------------
# 4. budget
# --------------------------------------------------------------------
def test_budget_counts_window_not_max_iters():
    meas, n, Q, X, _ = ring_case(67)
    kw = dict(basis_budget_bytes=64 << 10, max_iters=1000)
    assert 8 * 201 * 202 > 64 << 10 >= 8 * 201 * 17
    with pytest.raises(BasisBudgetError, match="basis_budget_bytes"):
        certify_solution(meas, n, 2, X, **kw)
    res = certify_solution(meas, n, 2, X, basis_size=16, **kw)
    assert res.status == CertificateStatus.NOT_OPTIMAL
    with pytest.raises(BasisBudgetError, match="basis_budget_bytes"):
        certify_solution(meas, n, 2, X, basis_size=16,
                         basis_budget_bytes=8 * 201 * 17 - 1)


# --------------------------------------------------------------------
# 5. keep validation
# --------------------------------------------------------------------
@pytest.mark.parametrize("b, keep", [
    (16, (0, 2)),                # k_lo >= 1
    (16, (6, 0)),                # k_hi >= 1
    (16, (12, 3)),               # k_lo + k_hi + 2 <= b
    (16, (13, 2)),
    (64, (CERT_KEEP_MAX, 1)),    # k_lo + k_hi <= CERT_KEEP_MAX
    (64, (8, 9)),
    (3, None),                   # no window below 4 vectors
])
def test_keep_validation(b, keep):
    meas, n, Q, X, _ = ring_case(8)
    with pytest.raises(ValueError):
        certify_solution(meas, n, 2, X, basis_size=b, keep=keep)


def test_keep_without_basis_size_rejected():
    meas, n, Q, X, _ = ring_case(8)
    with pytest.raises(ValueError):
        certify_solution(meas, n, 2, X, keep=(2, 1))


def test_default_keep_is_valid_for_every_window():
    assert default_keep(16) == (6, 2) and default_keep(12) == (4, 2)
    assert default_keep(64) == (14, 2)
    for b in range(4, 200):
        k_lo, k_hi = default_keep(b)
        assert k_lo >= 1 and k_hi >= 1 and k_lo + k_hi + 2 <= b
        assert k_lo + k_hi <= CERT_KEEP_MAX


def test_largest_accepted_keep_runs():
    meas, n, Q, X, _ = ring_case(67)
    res = certify_solution(meas, n, 2, X, basis_size=18, keep=(14, 2),
                           max_iters=1000)
    _show("ring67 b=18 keep=(14,2)", res)
    assert res.status == CertificateStatus.NOT_OPTIMAL
    assert res.restarts >= 1


# --------------------------------------------------------------------
# 6. restart algebra on its own
# --------------------------------------------------------------------
def test_restart_algebra_matches_dense_projection():
    meas, n, Q, X, _ = ring_case(67)
    S = dense_S(Q, X, 2)
    N, b, keep = 3 * n, 16, (6, 2)
    k = sum(keep)
    lam, _ = certificate_operator(Q, X)
    g = torch.Generator().manual_seed(0)
    V = torch.zeros(b + 1, N, dtype=torch.float64)
    V[0] = torch.randn(N, dtype=torch.float64, generator=g)
    V[0] /= torch.linalg.norm(V[0])
    ctl = torch.zeros(CERT_HDR + 2 * b, dtype=torch.float64)
    ctl[CERT_TOL] = BREAKDOWN_TOL * np.abs(S).sum(axis=1).max()
    cpu_ref.cert_lanczos_window(Q, lam, V, ctl, 0, b)
    assert ctl[cpu_ref.CERT_COUNT] == b and ctl[cpu_ref.CERT_FLAG] == 0
    h = ctl.numpy()
    alpha, beta = h[CERT_HDR:CERT_HDR + b], h[CERT_HDR + b:]
    T = np.diag(alpha) + np.diag(beta[:b - 1], 1) + np.diag(beta[:b - 1], -1)
    C, Tn = _thick_restart(T, beta[b - 1], keep)
    assert C.shape == (b, k)
    cpu_ref.cert_contract(V, torch.from_numpy(C))
    # one step after the restart, with nothing but the two host resets
    ctl[cpu_ref.CERT_COUNT] = k
    ctl[CERT_HDR + b + k - 1] = 0.0
    cpu_ref.cert_lanczos_window(Q, lam, V, ctl, k, 1)
    Tn[k, k] = h[CERT_HDR + k]
    Tn[k, k + 1] = Tn[k + 1, k] = h[CERT_HDR + b + k]

    Vh = V[:k + 2].numpy()
    orth = np.abs(Vh @ Vh.T - np.eye(k + 2)).max()
    diff = np.abs(Vh @ S @ Vh.T - Tn[:k + 2, :k + 2])
    diff[k + 1, k + 1] = 0.0        # alpha of a step not taken yet
    proj = diff.max()
    tol = 2 * N * EPS * np.abs(S).sum(axis=1).max()
    print(f"restart algebra: orth {orth!r} (cap {64 * EPS * b!r}) "
          f"proj {proj!r} (cap {tol!r})")
    assert orth <= 64 * EPS * b
    assert proj <= tol
    # the kept set: 6 smallest and 2 largest Ritz values of the window
    ev = np.linalg.eigvalsh(T)
    assert np.allclose(np.diag(Tn)[:k], np.concatenate([ev[:6], ev[-2:]]),
                       rtol=0, atol=64 * EPS * ev[-1])
    # the arrowhead is not negligible, so a dropped s_i would be seen
    assert np.abs(Tn[:k, k]).max() > 1e3 * tol


# --------------------------------------------------------------------
# 7. as_dict
# --------------------------------------------------------------------
def test_as_dict_restarts_key_only_with_basis_size():
    meas, n, Q, X, _ = ring_case(8)
    base = certify_solution(meas, n, 2, X).as_dict()
    assert list(base) == ["certificate", "lambda_min", "lambda_max",
                          "certificate_residual", "certificate_grad_norm",
                          "certificate_iterations"]
    res = certify_solution(meas, n, 2, X, basis_size=16)
    out = res.as_dict()
    assert out.pop("certificate_restarts") == res.restarts == 0
    assert out == base
    # not critical: still reported as a basis_size run
    meas, n, Q, X0, _ = grid_case()
    nc = certify_solution(meas, n, 3, X0, basis_size=12)
    assert nc.status == CertificateStatus.NOT_CRITICAL
    assert nc.as_dict()["certificate_restarts"] == 0
    assert math.isnan(nc.lambda_min)
