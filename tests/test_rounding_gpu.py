"""Rounding kernels on the GPU (dpo_ops.hip, section "rounding") against
the CPU reference, every compiled (d, r).

Tolerances: tests/rounding_refs.py. The distance of a rounded rotation
from the reference's is bounded by c eps ||B||_F / (sigma_{d-1} + s
sigma_d) on well-conditioned blocks, with c = 8 x the largest
NumPy-vs-torch SVD projection discrepancy on this test's own blocks
(measured on the CPU at test time: 2.0 to 6.0 for d = 2 and 7.9 to 8.0
for d = 3 on the hosts tried, hence c = 16 to 48 and about 64; the
kernels measured 8.8 and 42.6 in the same units; the factor 8 allows
for the device's different operation order). c is never taken from the
kernel's output."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as kr
import rounding_refs as rr
from test_refine import grid_case, grid_refined, ring_case

from dpo_amd.ops import cpu_ref, hip_backend as hb
from dpo_amd.rounding import round_solution

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = rr.EPS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def block_case(d, n):
    """Blocks, their kinds and both CPU projections, shared by every r."""
    B, kind = rr.make_blocks(n, d, n)
    return B, kind, rr.project_ref(B)


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_projection_invariants_and_distance(d, r):
    c, measured = rr.measured_c(d)
    print(f"d={d}: measured c {measured:.2f}, bound constant {c:.2f}")
    assert measured > 0.0
    for n in rr.pose_counts(d, r):
        B, kind, R_ref = block_case(d, n)
        U = rr.signed_permutation_basis(d, r, n)
        Xt = rr.lift_blocks(B, U, n)
        # the signed permutation makes U^T Y_i exact: same blocks
        Bc = np.einsum("kc,nak->nca", U, Xt.reshape(n, d + 1, r)[:, :d])
        assert np.array_equal(Bc, B)
        traj, Xr = hb.round_poses(dev(Xt), d, dev(U),
                                  torch.zeros(d, dtype=torch.float64), False)
        R = Xr.cpu().numpy().reshape(n, d + 1, d)[:, :d].transpose(0, 2, 1)
        nb, gap, exempt = rr.block_stats(B)
        # invariants on every block
        orth = np.linalg.norm(R.transpose(0, 2, 1) @ R - np.eye(d),
                              axis=(1, 2))
        assert orth.max() <= 64 * EPS, (n, orth.max() / EPS)
        assert (np.linalg.det(R) > 0).all()
        m = np.abs(B).max(axis=(1, 2))
        Bn = B / np.where(m > 0, m, 1.0)[:, None, None]
        obj = np.einsum("nij,nij->n", R, Bn)
        obj_ref = np.einsum("nij,nij->n", R_ref, Bn)
        slack = 64 * EPS * np.linalg.norm(Bn, axis=(1, 2)) * np.sqrt(d)
        assert (obj >= obj_ref - slack).all(), \
            (n, ((obj_ref - obj) / np.maximum(slack, 1e-300)).max())
        # exemptions: no random block, at most the singular kinds
        assert not exempt[kind == "random"].any()
        assert set(kind[exempt]) <= set(rr.EXEMPT_KINDS)
        assert exempt.sum() <= (kind != "random").sum() * 2 / 7 + 1
        # distance on the rest
        dist = np.linalg.norm(R - R_ref, axis=(1, 2))
        bound = rr.distance_bound(B, c)
        worst = rr.normalised_distance(R, R_ref, B).max()
        print(f"  n={n}: orth {orth.max() / EPS:.1f} eps, "
              f"normalised distance {worst:.2f} (bound {c:.2f})")
        assert (dist <= bound).all(), (n, worst, c)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_translations_layouts_and_gauge(d, r, flip):
    n = 257
    c = rr.measured_c(d)[0]
    B, _ = rr.make_blocks(n, d, 7, kinds=("neg", "cI", "rot"))
    U = rr.stiefel_basis(d, r, 3)
    Xt = torch.from_numpy(rr.lift_blocks(B, U, 11))
    Ut = torch.from_numpy(U)
    t0 = kr.randn(kr.gen(19, d, r), d)
    traj, Xr = hb.round_poses(Xt.to(DEV), d, Ut.to(DEV), t0.to(DEV), flip)
    traj_c, Xr_c = cpu_ref.round_poses(Xt, d, Ut, t0, flip)
    assert traj.shape == (d, n * (d + 1)) and Xr.shape == (n * (d + 1), d)
    assert torch.equal(traj, Xr.T)                  # the two layouts
    got = Xr.cpu().view(n, d + 1, d)
    ref = Xr_c.view(n, d + 1, d)
    # translations: r-term products and the subtraction of t0
    bP = kr.matmul_bound(Xt, Ut, r + 1).view(n, d + 1, d)
    tb = bP[:, d] + 2 * EPS * t0.abs()
    assert ((got[:, d] - ref[:, d]).abs() <= tb).all()
    # rotations: the blocks the two sides project differ by bP
    Uf = U.copy()
    if flip:
        Uf[:, -1] *= -1.0
    Bc = np.einsum("kc,nak->nca", Uf, Xt.numpy().reshape(n, d + 1, r)[:, :d])
    dB = bP[:, :d].flatten(1).norm(dim=1).numpy()
    _, _, exempt = rr.block_stats(Bc)
    # a flipped c I or rotation has sigma_{d-1} = sigma_d and det < 0:
    # every rotation maximises, distance_bound is inf there
    assert flip or not exempt.any()
    dist = (got[:, :d] - ref[:, :d]).flatten(1).norm(dim=1).numpy()
    assert (dist <= rr.distance_bound(Bc, c, dB)).all()
    # gauge: both sides start from the same rounded iterate
    a = 5
    Xg, Tg = Xr_c.clone().to(DEV), traj_c.clone().to(DEV)
    hb.round_gauge(Xg, Tg, d, a)
    Xh, Th = Xr_c.clone(), traj_c.clone()
    cpu_ref.round_gauge(Xh, Th, d, a)
    assert torch.equal(Tg, Xg.T)
    A = Xr_c.view(n, d + 1, d)[a]
    shifted = Xr_c.view(n, d + 1, d).abs().clone()
    shifted[:, d] += A[d].abs()
    bG = kr.matmul_bound(shifted.reshape(-1, d), A[:d].T.contiguous(),
                         d + 1)
    assert ((Xg.cpu() - Xh).abs() <= bG).all()
    # the anchor pose becomes the identity at the origin
    Ia = Xg.cpu().view(n, d + 1, d)[a]
    assert (Ia[:d] - torch.eye(d, dtype=torch.float64)).abs().max() \
        <= 64 * EPS
    assert (Ia[d].abs() <= bG.view(n, d + 1, d)[a, d]).all()


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_gram_and_reflection_count(d, r):
    for n in (1, 257, 2 * 256 + 1):
        B, _ = rr.make_blocks(n, d, n + 1,
                              kinds=("neg", "cI", "rot", "tiny", "huge"))
        U = rr.signed_permutation_basis(d, r, n)
        Xt = torch.from_numpy(rr.lift_blocks(B, U, n + 2))
        Xd = Xt.to(DEV)
        S1 = hb.round_gram(Xd, d)
        S2 = hb.round_gram(Xd, d)
        assert torch.equal(S1, S2)                  # bitwise reproducible
        assert torch.equal(S1, S1.T)
        Yt = Xt.view(n, d + 1, r)[:, :d].reshape(n * d, r)
        S_ref = cpu_ref.round_gram(Xt, d)
        bound = kr.sop_bound(Yt.abs().T @ Yt.abs(), n * d)
        assert ((S1.cpu() - S_ref).abs() <= bound).all()
        want = int((np.linalg.slogdet(B)[0] < 0).sum())
        got = hb.round_reflections(Xd, d, torch.from_numpy(U))
        assert got.dtype == torch.int32 and int(got) == want
        assert int(cpu_ref.round_reflections(
            Xt, d, torch.from_numpy(U))) == want


@functools.lru_cache(maxsize=None)
def ring_certified():
    from dpo_amd.refine import certified_solve
    meas, n, Q, X = ring_case(67)
    return certified_solve(meas, n, 2, X).Xt


@pytest.mark.parametrize("case", ["grid", "ring"])
def test_round_solution_matches_cpu(case):
    if case == "grid":
        meas, n, Q, _ = grid_case()
        Xt, d = grid_refined().Xt, 3
    else:
        meas, n, Q, _ = ring_case(67)
        Xt, d = ring_certified(), 2
    r = Xt.shape[1]
    cpu = round_solution(Q, Xt, d)
    gpu = round_solution(Q.to(DEV), Xt.to(DEV), d)
    assert gpu.Xt_rounded.is_cuda
    assert gpu.flipped == cpu.flipped and gpu.reflected == cpu.reflected
    _, _, _, _, B = rr.round_ref(Xt.numpy(), d)
    tmax = float(Xt.view(n, d + 1, r)[:, d].norm(dim=1).max())
    rot, trans = rr.pipeline_tol(n, d, r, B, rr.measured_c(d)[0], tmax)
    T, Tc = gpu.trajectory(), cpu.trajectory()
    dh = d + 1
    Tb, Cb = T.reshape(d, n, dh), Tc.reshape(d, n, dh)
    assert np.linalg.norm(Tb[:, :, :d] - Cb[:, :, :d], axis=(0, 2)).max() \
        <= 2 * rot
    assert np.abs(Tb[:, :, d] - Cb[:, :, d]).max() <= 2 * trans
    f_tol = 0.5 * kr.central_eval_ref(meas, n, d, cpu.Xt_rounded)[2]
    assert abs(gpu.f_rounded - cpu.f_rounded) <= 2 * f_tol
    assert abs(gpu.f_relaxed - cpu.f_relaxed) <= \
        kr.central_eval_ref(meas, n, d, Xt)[2]
    assert gpu.gap == gpu.f_rounded - gpu.f_relaxed
    np.testing.assert_allclose(gpu.spectrum, cpu.spectrum, rtol=0,
                               atol=8 * n * d * EPS)


def test_packed_driver_gather_device_matches_host():
    from dpo_amd.comm import Comm
    from dpo_amd.dist_driver import DistributedRBCDDriver
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=3, seed=0)
    drv = DistributedRBCDDriver(meas, n, 3, Comm(), r=5,
                                partition="contiguous", device=DEV)
    drv.run(max_iters=3)
    assert drv._packed is not None
    host = drv.gather_final_trajectory()
    devT = drv.gather_final_trajectory(device=True)
    assert devT.shape == host.shape == (3, 4 * n)
    c = rr.measured_c(3)[0]
    Hb, Db = host.reshape(3, n, 4), devT.reshape(3, n, 4)
    for rb, a in drv.local_agents.items():
        X = a.X.cpu()
        Ya = torch.from_numpy(np.ascontiguousarray(a.global_anchor[:, :3]))
        Xb = X.view(-1, 4, 5)
        B = (Xb[:, :3, :] @ Ya).transpose(1, 2).numpy()
        bP = kr.matmul_bound(Xb.reshape(-1, 5), Ya, 6).view(-1, 4, 3)
        dB = bP[:, :3].flatten(1).norm(dim=1).numpy()
        assert not rr.block_stats(B)[2].any()
        idx = [drv.pose_to_index[(rb, i)] for i in range(a.n)]
        dist = np.linalg.norm(Hb[:, idx, :3] - Db[:, idx, :3], axis=(0, 2))
        assert (dist <= rr.distance_bound(B, c, dB)).all()
        tb = 2.0 * (float(bP[:, 3].max()) + float(kr.matmul_bound(
            torch.from_numpy(a.global_anchor[:, 3:].T.copy()), Ya, 6).max()))
        assert np.abs(Hb[:, idx, 3] - Db[:, idx, 3]).max() <= tb


def test_uncompiled_shape_raises():
    Xt = torch.zeros(3 * 4, 7, dtype=torch.float64, device=DEV)
    U = torch.zeros(7, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        hb.round_gram(Xt, 2)
    with pytest.raises(ValueError):
        hb.round_poses(Xt, 2, U, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError):
        hb.round_reflections(Xt, 2, U)
    with pytest.raises(ValueError):
        hb.round_gauge(torch.zeros(4 * 3, 4, dtype=torch.float64, device=DEV),
                       torch.zeros(4, 4 * 3, dtype=torch.float64, device=DEV),
                       4, 0)
    meas, n, Q, X = ring_case(67)
    X7 = torch.zeros(3 * n, 7, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        round_solution(Q.to(DEV), X7, 2)
