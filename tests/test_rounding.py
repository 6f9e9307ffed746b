"""Rounding of a lifted iterate to SE(d) (dpo_amd.rounding), CPU path:
exact recovery, the reflected component, anchor parity with the host
loop, the suboptimality gap and the unchanged defaults.

Tolerances: tests/rounding_refs.py. The rounded rotations are compared
under c eps ||B||_F / (sigma_{d-1} + s sigma_d) with c = 8 x the largest
NumPy-vs-torch SVD projection discrepancy on the projection test's own
blocks (measured at test time; 2.0 to 6.0 for d = 2 and 7.9 to 8.0 for
d = 3 on the hosts tried, so c is 16 to 48 and about 64)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import kernel_refs as kr
import rounding_refs as rr
from test_refine import grid_case, grid_refined, ring_case

from dpo_amd.certify import CertificateStatus
from dpo_amd.quadratic import QuadraticProblem
from dpo_amd.refine import certified_solve
from dpo_amd.rounding import RoundingResult, round_solution

EPS = rr.EPS
N_GT = 40
SHAPES = [(2, 2), (2, 4), (2, 6), (3, 3), (3, 5), (3, 8)]


def lift(T, d, L):
    """Xt (n (d+1), r) = (L T)^T."""
    return torch.from_numpy(np.ascontiguousarray((L @ T).T))


def chain_q(n, d):
    """Connection Laplacian of an identity-measurement chain: any Q of
    the right size serves the trajectory tests."""
    from dpo_amd.quadratic import assemble_connection_laplacian
    from dpo_amd.types import RelativeSEMeasurement
    meas = [RelativeSEMeasurement(0, 0, k, k + 1, np.eye(d), np.zeros(d),
                                  1.0, 1.0) for k in range(n - 1)]
    return assemble_connection_laplacian(meas, n, d)


def assert_trajectory(T, T_ref, d, rot_tol, trans_tol):
    dh = d + 1
    n = T.shape[1] // dh
    Tb, Rb = T.reshape(d, n, dh), T_ref.reshape(d, n, dh)
    rot = np.linalg.norm(Tb[:, :, :d] - Rb[:, :, :d], axis=(0, 2))
    trans = np.abs(Tb[:, :, d] - Rb[:, :, d]).max()
    print(f"rot err {rot.max():.3e} (tol {rot_tol:.3e}), "
          f"trans err {trans:.3e} (tol {trans_tol:.3e})")
    assert rot.max() <= rot_tol
    assert trans <= trans_tol


def recovery_tol(T, d, r):
    n = T.shape[1] // (d + 1)
    B = T.reshape(d, n, d + 1)[:, :, :d].transpose(1, 0, 2)
    return rr.pipeline_tol(n, d, r, B, rr.measured_c(d)[0],
                           float(np.abs(T).max()) * math.sqrt(r))


@pytest.mark.parametrize("d,r", SHAPES)
def test_exact_recovery(d, r):
    T = rr.ground_truth(N_GT, d, seed=r)
    L = rr.stiefel_basis(d, r, 0)
    res = round_solution(chain_q(N_GT, d), lift(T, d, L), d)
    assert isinstance(res, RoundingResult)
    assert res.Xt_rounded.shape == (N_GT * (d + 1), d)
    assert np.array_equal(res.trajectory(), res.Xt_rounded.numpy().T)
    assert_trajectory(res.trajectory(), T, d, *recovery_tol(T, d, r))
    assert res.reflected in (0, N_GT)
    assert res.flipped == (res.reflected == N_GT)
    # rank d: nothing outside the top d eigenvalues, which are all 1
    assert abs(res.rank_energy) <= 8 * N_GT * d * EPS
    assert np.allclose(res.spectrum[:d], 1.0, atol=8 * N_GT * d * EPS)


@pytest.mark.parametrize("d", [2, 3])
def test_reflected_component_is_flipped(d):
    T = rr.ground_truth(N_GT, d, seed=d)
    L = rr.stiefel_basis(d, d, 1)               # d x d orthogonal
    if np.linalg.det(L) > 0:
        L[:, 0] *= -1.0                         # its action has det = -1
    Q = chain_q(N_GT, d)
    res = round_solution(Q, lift(T, d, L), d)
    assert res.flipped is True
    assert res.reflected == N_GT
    assert_trajectory(res.trajectory(), T, d, *recovery_tol(T, d, d))
    # the mirror image of L: same trajectory, no flip
    L[:, 0] *= -1.0
    res2 = round_solution(Q, lift(T, d, L), d)
    assert res2.flipped is False and res2.reflected == 0
    rot, trans = recovery_tol(T, d, d)
    assert_trajectory(res.trajectory(), res2.trajectory(), d, 2 * rot,
                      2 * trans)


def anchor_tol(X, anchor, d):
    """Per-pose rotation tolerance and the translation tolerance of the
    anchor rounding: both paths project fp64 evaluations of Ya^T Y_i that
    differ by the r-term products' rounding."""
    r = X.shape[1]
    Ya = torch.from_numpy(np.ascontiguousarray(anchor[:, :d]))
    Xb = X.view(-1, d + 1, r)
    B = (Xb[:, :d, :] @ Ya).transpose(1, 2).numpy()
    dB = float(kr.matmul_bound(Xb.reshape(-1, r), Ya, r).view(
        -1, d + 1, d)[:, :d].flatten(1).norm(dim=1).max())
    _, _, exempt = rr.block_stats(B)
    assert not exempt.any()
    rot = rr.distance_bound(B, rr.measured_c(d)[0], dB).max()
    trans = 2.0 * float(kr.matmul_bound(Xb.reshape(-1, r), Ya, r + 1).max()) \
        + 2.0 * float(kr.matmul_bound(torch.from_numpy(anchor[:, d:].T.copy()),
                                      Ya, r + 1).max())
    return rot, trans


def test_agent_anchor_parity():
    from dpo_amd.driver import MultiRobotDriver
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=3, seed=0)
    drv = MultiRobotDriver(meas, n, 2, r=5, partition="contiguous")
    drv.run(max_iters=3)
    for a in drv.agents:
        a.set_global_anchor(drv.agents[0].X[:a.dh].cpu().numpy().T.copy())
        host = a.get_trajectory_in_global_frame()
        dev = a.get_trajectory_in_global_frame(device=True)
        assert dev.shape == host.shape
        assert_trajectory(dev, host, a.d,
                          *anchor_tol(a.X.cpu(), a.global_anchor, a.d))
        host = a.get_trajectory_in_local_frame()
        dev = a.get_trajectory_in_local_frame(device=True)
        anchor = a.X[:a.dh].cpu().numpy().T.copy()
        assert_trajectory(dev, host, a.d,
                          *anchor_tol(a.X.cpu(), anchor, a.d))


def test_driver_gather_parity():
    from dpo_amd.comm import Comm
    from dpo_amd.dist_driver import DistributedRBCDDriver
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=3, seed=0)
    drv = DistributedRBCDDriver(meas, n, 3, Comm(), r=5,
                                partition="contiguous")
    drv.run(max_iters=3)
    host = drv.gather_final_trajectory()
    dev = drv.gather_final_trajectory(device=True)
    assert dev.shape == host.shape == (3, 4 * n)
    rot = trans = 0.0
    for a in drv.local_agents.values():
        ra, ta = anchor_tol(a.X.cpu(), a.global_anchor, 3)
        rot, trans = max(rot, ra), max(trans, ta)
    assert_trajectory(dev, host, 3, rot, trans)


def f_tol(meas, n, d, *Xs):
    """Roundoff bound of the cost evaluations at the given iterates:
    half the <QX, X> bound of central_eval_ref each (f = 0.5 <QX, X>)."""
    return sum(0.5 * kr.central_eval_ref(meas, n, d, X)[2] for X in Xs)


def check_against_reference(res, Xt, d):
    T, reflected, flipped, spectrum, B = rr.round_ref(Xt.numpy(), d)
    n, r = Xt.shape[0] // (d + 1), Xt.shape[1]
    _, _, exempt = rr.block_stats(B)
    assert not exempt.any()
    tmax = float(Xt.view(n, d + 1, r)[:, d].norm(dim=1).max())
    rot, trans = rr.pipeline_tol(n, d, r, B, rr.measured_c(d)[0], tmax)
    assert res.reflected == reflected and res.flipped == flipped
    assert_trajectory(res.trajectory(), T, d, rot, trans)
    return spectrum


def test_gap_noise_free_ring():
    meas, n, Q, X = ring_case(67)
    stair = certified_solve(meas, n, 2, X, round=True)
    assert stair.status == CertificateStatus.CERTIFIED and stair.rank == 4
    res = stair.rounding
    check_against_reference(res, stair.Xt, 2)
    problem = QuadraticProblem(n, 2, 2, precond="jacobi")
    problem.set_q(Q)
    f_oracle = problem.f(res.Xt_rounded)
    assert abs(res.f_rounded - f_oracle) <= f_tol(meas, n, 2, res.Xt_rounded)
    assert res.gap == res.f_rounded - res.f_relaxed
    out = stair.as_dict()
    assert out["rounded_cost"] == res.f_rounded
    assert out["relaxation_cost"] == res.f_relaxed
    assert out["suboptimality_gap"] == res.gap
    assert out["rounding_flipped"] == res.flipped
    assert out["rounding_reflected"] == res.reflected
    assert out["rank_energy"] == res.rank_energy
    assert out["relative_gap"] == res.relative_gap


def test_gap_noisy_grid():
    meas, n, Q, X0 = grid_case()
    Xt = grid_refined().Xt
    res = round_solution(Q, Xt, 3)
    spectrum = check_against_reference(res, Xt, 3)
    tol = f_tol(meas, n, 3, Xt, res.Xt_rounded)
    print(f"gap {res.gap:.3e} tol {tol:.3e}")
    assert res.gap >= -tol
    assert abs(res.f_relaxed - 0.5 * kr.central_eval_ref(
        meas, n, 3, Xt)[0]) <= f_tol(meas, n, 3, Xt)
    ref_energy = spectrum[3:].sum() / spectrum.sum()
    # the share itself is a difference of O(1) eigenvalues of S / n:
    # 1e-12 relative to the spectrum's scale
    assert abs(res.rank_energy - ref_energy) <= 1e-12 * max(
        abs(ref_energy), 1.0)
    np.testing.assert_allclose(res.spectrum, spectrum, rtol=0,
                               atol=1e-12 * spectrum[0])


def test_anchor_mode_matches_host_loop():
    meas, n, Q, X0 = grid_case()
    Xt = grid_refined().Xt
    anchor = Xt[:4].numpy().T.copy()
    res = round_solution(Q, Xt, 3, mode="anchor", anchor=anchor)
    Ya, pa = anchor[:, :3], anchor[:, 3]
    X = Xt.numpy().T
    from dpo_amd.liegroups import project_to_rotation_group
    host = Ya.T @ X
    for i in range(n):
        host[:, 4 * i:4 * i + 3] = project_to_rotation_group(
            host[:, 4 * i:4 * i + 3])
        host[:, 4 * i + 3] -= Ya.T @ pa
    assert res.flipped is False
    assert_trajectory(res.trajectory(), host, 3, *anchor_tol(Xt, anchor, 3))
    with pytest.raises(ValueError):
        round_solution(Q, Xt, 3, mode="anchor")
    with pytest.raises(ValueError):
        round_solution(Q, Xt, 3, mode="nearest")


def test_uncompiled_shape_raises():
    meas, n, Q, X = ring_case(67)
    X7 = torch.zeros(3 * n, 7, dtype=torch.float64)
    X7[:, :2] = X
    with pytest.raises(ValueError):
        round_solution(Q, X7, 2)


# ---------------------------------------------------------------------
# defaults unchanged
# ---------------------------------------------------------------------
STAIR_KEYS = {
    "refine_status", "refine_f_init", "refine_f_final",
    "refine_grad_norm_init", "refine_grad_norm_final", "refine_grad_tol",
    "refine_outer", "refine_inner", "refine_rejected", "refine_tcg_status",
    "refine_precond", "refine_seconds", "staircase_levels", "final_rank",
    "levels"}
ROUND_KEYS = {"rounded_cost", "relaxation_cost", "suboptimality_gap",
              "relative_gap", "rounding_reflected", "rounding_flipped",
              "rank_energy"}


def test_certified_solve_default_keys_unchanged():
    meas, n, Q, X0 = grid_case()
    plain = certified_solve(meas, n, 3, X0)
    assert plain.rounding is None
    cert_keys = set(plain.certificate.as_dict())
    assert set(plain.as_dict()) == STAIR_KEYS | cert_keys
    assert not ROUND_KEYS & set(plain.as_dict())
    rounded = certified_solve(meas, n, 3, X0, round=True)
    assert set(rounded.as_dict()) == STAIR_KEYS | cert_keys | ROUND_KEYS


def _script(name):
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


@pytest.mark.parametrize("name,argv", [
    ("single_robot", ["--dataset", "x"]),
    ("headline", ["--dataset", "x"]),
    ("million", []),
])
def test_script_round_flag_is_opt_in(name, argv):
    mod = _script(name)
    args = mod.build_parser().parse_args(argv)
    assert args.round is False
    assert mod.build_parser().parse_args(argv + ["--round"]).round is True
    # without the flag the scripts add nothing to their JSON line
    assert mod.rounding_fields(args, None) == {}
