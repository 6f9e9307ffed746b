"""CPU side of the packed-round parity tests (docs/DESIGN.md, "Packed
round tests"): the dict path's round schedule against the reference's
cadence, the GNC fixture's distance from the TLS thresholds, and the
references of tests/kernel_refs.py that tests/test_packed_rounds_gpu.py
holds the packed path to."""
import numpy as np
import pytest
import torch

import kernel_refs as kr
from dpo_amd.comm import Comm
from dpo_amd.dist_driver import DistributedRBCDDriver, _DictBackend
from dpo_amd.synthetic import city2d, grid3d
from dpo_amd.types import RobustCostType


def _gnc_dict_driver(acceleration, device="cpu"):
    ma, n, Xg = kr.gnc_fixture()
    drv = DistributedRBCDDriver(ma.to_list(), n, 4, Comm(), r=5,
                                partition="contiguous",
                                robust=RobustCostType.GNC_TLS,
                                acceleration=acceleration,
                                selection="colored", device=device)
    kr.set_global_iterate(drv, Xg)
    return drv


@pytest.mark.parametrize("robust", [False, True], ids=["l2", "gnc"])
@pytest.mark.parametrize("acceleration", [False, True],
                         ids=["plain", "accel"])
def test_dict_schedule_matches_reference_cadence(acceleration, robust):
    """PGOAgent.iterate() restarts in rounds 4, 9, ... and re-weights in
    rounds 3, 7, 11, ... (restart_interval 5, inner iterations 4), keeps
    counting over a second run() and starts over after
    restore_initial_state(). Integers and gamma are exact."""
    if robust:
        drv = _gnc_dict_driver(acceleration)
    else:
        meas, n = grid3d(side=4, seed=0)
        drv = DistributedRBCDDriver(meas, n, 4, Comm(), r=5,
                                    partition=kr.interleaved_partition(n, 4),
                                    acceleration=acceleration,
                                    selection="colored")
    first, again = kr.run_schedule(drv)
    kr.check_schedule(first, sum(kr.SCHED_RUNS), 4, acceleration, robust)
    kr.check_schedule(again, kr.SCHED_RUNS[1], 4, acceleration, robust)
    if acceleration:
        assert first[0][0] == [4, 9]
    if robust:
        assert first[0][1] == [3, 7, 11]


def test_gnc_fixture_has_no_edge_at_a_threshold():
    """The GPU test may leave out edges whose residual is within its
    rounding bound of a GNC-TLS threshold. On this fixture and seed the
    host code has none, at the first re-weighting's mu; and the fixture
    has weights in the transition band, outliers and both co-owner
    orders, so the comparison is not vacuous."""
    ma, n, Xg = kr.gnc_fixture()
    drv = _gnc_dict_driver(False)
    a0 = drv.local_agents[0]
    mu, barc = a0.robust_cost.mu, a0.robust_cost.params.gnc_barc
    r_sq, bound = kr.gnc_edge_residuals(ma, Xg)
    lc = ma.p1 + 1 != ma.p2
    assert not kr.gnc_near_threshold(r_sq, bound, mu, barc)[lc].any()
    assert ma.outlier_mask.sum() >= 10
    w = kr.gnc_weight_ref(r_sq[lc], mu, barc)
    assert ((w > 0) & (w < 1)).sum() >= 10
    assert drv._n_cross >= 10
    # the host weights are this reference, edge for edge
    _DictBackend(drv).begin()
    part = np.repeat(np.arange(4), n // 4)
    for rb, a in drv.local_agents.items():
        a.update_loop_closures_weights()
        _, priv, shared = kr.agent_edge_index(ma.p1, ma.p2, part, rb)
        got = np.array([m.weight for m in a.private_lc])
        want = kr.gnc_weight_ref(r_sq[priv], mu, barc)
        assert np.abs(got - want).max(initial=0.0) <= kr.gnc_tol(mu)
        own = drv._cross_owned[rb]
        got = np.array([m.weight for m in a.shared_lc])
        want = kr.gnc_weight_ref(r_sq[shared], mu, barc)
        assert np.abs(got - want)[own].max(initial=0.0) <= kr.gnc_tol(mu)
        assert (got[~own] == 1.0).all()


@pytest.mark.parametrize("d", [2, 3])
def test_eval_references_agree_on_the_dict_path(d):
    """sum_rb 2 (f_rb - 0.5 <X, G>_rb) = <Q X, X> and sum_rb
    ||rgrad_rb||^2 = ||rgrad||^2 hold between kernel_refs' per-agent and
    centralized references (interleaved partition, X on the manifold but
    no solver output), within their own bounds, and the per-agent rows
    are what the dict path evaluates."""
    meas, n = grid3d(side=4, seed=0) if d == 3 else city2d(side=6, seed=0)
    drv = DistributedRBCDDriver(meas, n, 4, Comm(), r=5,
                                partition=kr.interleaved_partition(n, 4),
                                selection="colored")
    for rb, a in drv.local_agents.items():
        a.X = kr.manifold_point(a.n, d, 5, kr.gen(40, d, rb))
    _DictBackend(drv).begin()
    rows, bounds = [], []
    for rb, a in drv.local_agents.items():
        w = torch.ones(len(a._all_meas), dtype=torch.float64)
        ref, b = kr.agent_eval_ref(a, kr.nbr_from_dict(a), w)
        got = drv._eval_scalars(a)
        assert (np.abs(got - ref) <= b).all(), (rb, got, ref, b)
        rows.append(ref)
        bounds.append(b)
    rows, bounds = np.array(rows), np.array(bounds)
    cost, gn2, b_cost, b_gn2 = kr.central_eval_ref(
        meas, n, d, drv.gather_lifted_iterate())
    assert abs(2.0 * (rows[:, 0] - rows[:, 1]).sum() - cost) \
        <= 2.0 * bounds[:, :2].sum() + b_cost
    assert abs(rows[:, 2].sum() - gn2) <= bounds[:, 2].sum() + b_gn2
    assert cost > 1.0 and gn2 > 1.0
