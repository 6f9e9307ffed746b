"""GPU tests of the optimality certificate: the HIP kernels against the
fp64 torch reference of the same operations, and certify_solution on GPU
tensors against the CPU run. Cases are shared with test_certify.py."""
import math

import numpy as np
import pytest
import torch

from test_certify import grid_case, grid_reference, ring_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=1e-10, rtol=1e-12)


def _backends():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import cpu_ref, hip_backend
    return cpu_ref, hip_backend


def _kernel_case(name):
    """(Q, X, d) — grid at r = 3 and 5 (random manifold points), and the
    n = 67 ring whose N = 201 is a multiple of neither 64 nor 256."""
    from dpo_amd.manifold import LiftedSEManifold
    if name == "ring67":
        meas, n, Q, X, _ = ring_case(67)
        return Q, X, 2
    r = {"grid_r3": 3, "grid_r5": 5}[name]
    meas, n, Q, _, _ = grid_case()
    g = torch.Generator().manual_seed(11)
    return Q, LiftedSEManifold(r, 3, n).random_point(generator=g), 3


def _unit(N, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(N, dtype=torch.float64, generator=g)
    return v / torch.linalg.norm(v)


def _lanczos_state(Q, lam, m, seed=5):
    from dpo_amd.ops.cpu_ref import CERT_HDR, CERT_TOL
    N = Q.N
    V = torch.zeros(m + 1, N, dtype=torch.float64)
    V[0] = _unit(N, seed)
    ctl = torch.zeros(CERT_HDR + 2 * m, dtype=torch.float64)
    ctl[CERT_TOL] = 1e-10
    return V, ctl


# --------------------------------------------------------------------
# 1. k_cert_lambda / k_cert_apply against cpu_ref
# --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid_r3", "grid_r5", "ring67"])
def test_cert_lambda_and_apply_match_cpu(name):
    cpu_ref, hip = _backends()
    Q, X, d = _kernel_case(name)
    Qd = Q.to(DEV)
    lam_ref, res_ref = cpu_ref.cert_lambda(Q, X, d)
    lam, res = hip.cert_lambda(Qd, X.to(DEV), d)
    assert torch.allclose(lam.cpu(), lam_ref, **TOL)
    assert torch.allclose(res.cpu(), res_ref, **TOL)

    v, vp, beta = _unit(Q.N, 1), _unit(Q.N, 2), 0.37
    w_ref, a_ref = cpu_ref.cert_apply(Q, lam_ref, v, vp, beta)
    w, a = hip.cert_apply(Qd, lam, v.to(DEV), vp.to(DEV), beta)
    assert torch.allclose(w.cpu(), w_ref, **TOL)
    assert torch.allclose(a.cpu(), a_ref, **TOL)
    # first step: no previous vector
    w_ref, a_ref = cpu_ref.cert_apply(Q, lam_ref, v)
    w, a = hip.cert_apply(Qd, lam, v.to(DEV))
    assert torch.allclose(w.cpu(), w_ref, **TOL)
    assert torch.allclose(a.cpu(), a_ref, **TOL)


# --------------------------------------------------------------------
# 2. one full step
# --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid_r5", "ring67"])
def test_full_step_orthonormal_and_matches_cpu(name):
    cpu_ref, hip = _backends()
    from dpo_amd.ops.cpu_ref import CERT_COUNT, CERT_FLAG, CERT_HDR
    Q, X, d = _kernel_case(name)
    lam_ref, _ = cpu_ref.cert_lambda(Q, X, d)
    m, k = 12, 6
    Vc, cc = _lanczos_state(Q, lam_ref, m)
    Qd = Q.to(DEV)
    lam = lam_ref.to(DEV)
    Vg, cg = Vc.to(DEV), cc.to(DEV)
    # k steps in one batch, then ONE more step on its own
    for first, nsteps in ((0, k), (k, 1)):
        cpu_ref.cert_lanczos_steps(Q, lam_ref, Vc, cc, first, nsteps)
        hip.cert_lanczos_steps(Qd, lam, Vg, cg, first, nsteps)
    h = cg.cpu()
    assert h[CERT_FLAG] == 0 and h[CERT_COUNT] == k + 1
    B = Vg[:k + 2].cpu()
    new = B[k + 1]
    assert abs(float(torch.linalg.norm(new)) - 1.0) <= 1e-12
    assert float((B[:k + 1] @ new).abs().max()) <= 1e-12
    assert not Vg[k + 2:].cpu().any()      # nothing written past col k+1
    # scale: lambda_max <= ||S||_inf; use the dense value
    from test_certify import dense_S
    lmax = np.linalg.eigvalsh(dense_S(Q, X, d))[-1]
    sl_a = slice(CERT_HDR, CERT_HDR + k + 1)
    sl_b = slice(CERT_HDR + m, CERT_HDR + m + k + 1)
    assert float((h[sl_a] - cc[sl_a]).abs().max()) <= 1e-10 * lmax
    assert float((h[sl_b] - cc[sl_b]).abs().max()) <= 1e-10 * lmax


# --------------------------------------------------------------------
# 3. certify_solution on GPU tensors
# --------------------------------------------------------------------
def _certify_case(name):
    if name == "grid":
        meas, n, Q, _, X = grid_case()
        return meas, n, 3, X, grid_reference()[-1]
    meas, n, Q, X, _ = ring_case({"ring8": 8, "ring67": 67}[name])
    return meas, n, 2, X, 4.0


@pytest.mark.parametrize("name", ["ring8", "ring67", "grid"])
def test_certify_solution_gpu_matches_cpu(name):
    _backends()
    from dpo_amd.certify import certify_solution
    meas, n, d, X, lmax = _certify_case(name)
    ref = certify_solution(meas, n, d, X)
    a = certify_solution(meas, n, d, X.to(DEV))
    b = certify_solution(meas, n, d, X.to(DEV))
    print(f"{name}: cpu {ref.status} {ref.lambda_min!r} res {ref.residual!r} "
          f"it {ref.iterations}; gpu {a.status} {a.lambda_min!r} "
          f"res {a.residual!r} it {a.iterations}")
    assert a.status == ref.status
    assert abs(a.lambda_min - ref.lambda_min) <= max(
        a.residual, ref.residual, 1e-8 * lmax)
    assert a.direction.device.type == "cuda"
    assert abs(float(torch.linalg.norm(a.direction)) - 1.0) <= 1e-12
    # run-to-run determinism (docs/DESIGN.md §8): bit-identical
    assert a.lambda_min == b.lambda_min and a.iterations == b.iterations


# --------------------------------------------------------------------
# 4. breakdown on device
# --------------------------------------------------------------------
def test_breakdown_guard_within_one_batch():
    _backends()
    from dpo_amd.certify import CertificateStatus, certify_solution
    meas, n, Q, X, lam_true = ring_case(8)
    # eta = 10 > |lambda_min|: no early NOT_OPTIMAL exit, so the single
    # 32-step batch runs past the exhaustion of the N = 24 Krylov space
    for eta in (None, 10.0):
        res = certify_solution(meas, n, 2, X.to(DEV), check_every=32,
                               eta=eta)
        print(f"breakdown eta={eta}: {res.status} {res.lambda_min!r} "
              f"it {res.iterations}")
        assert 0 < res.iterations <= 24
        for x in (res.lambda_min, res.lambda_max, res.residual,
                  res.grad_norm):
            assert math.isfinite(x)
        assert torch.isfinite(res.direction).all()
        assert abs(res.lambda_min - lam_true) <= 1e-8 * 4.0
        assert res.status == (CertificateStatus.NOT_OPTIMAL if eta is None
                              else CertificateStatus.CERTIFIED)


# --------------------------------------------------------------------
# 5. driver accessor
# --------------------------------------------------------------------
def test_driver_gather_lifted_iterate():
    _backends()
    from dpo_amd.certify import CertificateStatus, certify_solution
    from dpo_amd.comm import Comm
    from dpo_amd.dist_driver import DistributedRBCDDriver
    from dpo_amd.liegroups import project_to_rotation_group
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=3, seed=0)
    d, r = 3, 5
    drv = DistributedRBCDDriver(meas, n, 2, Comm(), r=r,
                                partition="contiguous", device=DEV,
                                acceleration=True)
    res = drv.run(max_iters=250, gradnorm_tol=3e-3)
    assert res.converged, f"gradnorm {res.final_gradnorm}"
    Xt = drv.gather_lifted_iterate()
    assert Xt.shape == (n * (d + 1), r)
    # rounding: T_i = X_0^{-1} X_i with the anchor pose 0 (rotation
    # Y_0^T Y_i projected to SO(d), translation Y_0^T (p_i - p_0))
    T = drv.gather_final_trajectory()
    Xb = Xt.numpy().reshape(n, d + 1, r)
    Y0 = Xb[0, :d, :]
    for i in range(n):
        Ri = project_to_rotation_group(Y0 @ Xb[i, :d, :].T)
        ti = Y0 @ (Xb[i, d, :] - Xb[0, d, :])
        Ti = T[:, i * (d + 1):(i + 1) * (d + 1)]
        assert np.allclose(Ti[:, :d], Ri, atol=1e-8)
        assert np.allclose(Ti[:, d], ti, atol=1e-8)
    cert = certify_solution(meas, n, d, Xt.to(DEV))
    print(f"driver: {cert.status} grad {cert.grad_norm!r} "
          f"lambda_min {cert.lambda_min!r} it {cert.iterations}")
    assert abs(cert.grad_norm - res.final_gradnorm) <= 1e-6
    assert cert.status != CertificateStatus.NOT_CRITICAL
