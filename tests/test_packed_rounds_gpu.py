"""State-level parity of the packed round loop (dpo_amd/packed.py, the
_packed_* methods of PGOAgent) with the dict path and with plain fp64
references: exchange index maps, per-round evaluation, Nesterov
bookkeeping, round schedule, GNC re-weighting and whole rounds. Bounds
are exact, derived by the rules of docs/DESIGN.md "Kernel test matrix",
or the whole-solve tolerances the suite already uses; see "Packed round
tests" there."""
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr
from dpo_amd.comm import Comm
from dpo_amd.dist_driver import DistributedRBCDDriver, _DictBackend
from dpo_amd.ops import cpu_ref
from dpo_amd.synthetic import city2d, grid3d
from dpo_amd.types import RobustCostType

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = kr.EPS
R = 5


def _part(kind, n, k):
    return "contiguous" if kind == "contiguous" \
        else kr.interleaved_partition(n, k)


def _l2_driver(d=3, robots=4, part="interleaved", accel=False, comm=None,
               selection="colored"):
    meas, n = grid3d(side=4, seed=0) if d == 3 else city2d(side=6, seed=0)
    drv = DistributedRBCDDriver(meas, n, robots, comm or Comm(), r=R,
                                partition=_part(part, n, robots),
                                acceleration=accel, selection=selection,
                                device=DEV)
    return drv, meas, n


def _gnc_driver(accel=False, part="interleaved", soa=True):
    ma, n, Xg = kr.gnc_fixture()
    drv = DistributedRBCDDriver(ma if soa else ma.to_list(), n, 4, Comm(),
                                r=R, partition=_part(part, n, 4),
                                robust=RobustCostType.GNC_TLS,
                                acceleration=accel, selection="colored",
                                device=DEV)
    kr.set_global_iterate(drv, Xg)
    return drv, ma, n


def _packed(drv):
    from dpo_amd.packed import PackedBackend
    b = drv._backend()
    assert isinstance(b, PackedBackend)
    return b


def _fill(t, *key):
    """Distinct random values in place (views stay views)."""
    t.copy_(kr.randn(kr.gen(*key), *t.shape).to(t.device))


def _fill_manifold(t, d, *key):
    n = t.shape[0] // (d + 1)
    t.copy_(kr.manifold_point(n, d, t.shape[1], kr.gen(*key)).to(t.device))


def _blocks(t, dh):
    return t.view(-1, dh, t.shape[1])


# ---------------------------------------------------------------------
# 1. exchange index maps
# ---------------------------------------------------------------------
def _assert_nbr_buffers(backends, drvs, accel):
    """Every neighbour slot of every local agent of every rank holds the
    owner's X (aux: Y) block, bit for bit; NaN marks a slot never
    written."""
    seen = 0
    for b, drv in zip(backends, drvs):
        dh = drv.dh
        for rb, a in drv.local_agents.items():
            assert len(a._nbr_slot_order) > 0
            for slot, (nb, p) in enumerate(a._nbr_slot_order):
                own = drvs[drv.owner[nb] if len(drvs) > 1 else 0] \
                    .local_agents[nb]
                assert torch.equal(a._nbr_buffer[slot],
                                   _blocks(own.X, dh)[p]), (rb, slot, nb, p)
                if accel:
                    assert torch.equal(a._nbr_buffer_aux[slot],
                                       _blocks(own.Y, dh)[p]), (rb, slot)
                seen += 1
    assert seen > 0


def _assert_aliases(b, drv):
    """a.X and the neighbour buffers are views into the rank buffers, in
    rank_agents order."""
    dh, off, soff = drv.dh, 0, 0
    for rb in drv.rank_agents[drv.comm.rank]:
        a = drv.local_agents[rb]
        assert a.X.data_ptr() == b.rank_X.data_ptr() + off * dh * R * 8
        assert a.X.shape == (a.n * dh, R) and a.X.is_contiguous()
        ns = max(len(a._nbr_slot_order), 1)
        assert a._nbr_buffer.data_ptr() == \
            b.rank_nbr.data_ptr() + soff * dh * R * 8
        assert a._nbr_buffer_aux.data_ptr() == \
            b.rank_nbr_aux.data_ptr() + soff * dh * R * 8
        assert a._nbr_buffer.shape == (ns, dh, R)
        off += a.n
        soff += ns
    assert b.rank_X.shape[0] == off * dh and b.rank_nbr.shape[0] == soff


@pytest.mark.parametrize("accel", [False, True], ids=["plain", "accel"])
@pytest.mark.parametrize("part", ["contiguous", "interleaved"])
@pytest.mark.parametrize("d", [2, 3])
def test_exchange_maps_world1(d, part, accel):
    drv, _, _ = _l2_driver(d, 4, part, accel)
    b = _packed(drv)
    for rb, a in drv.local_agents.items():
        _fill(a.X, 50, d, rb)
        if accel:
            _fill(a.V, 51, d, rb)   # alpha = 1 in round 0: Y = polar(V)
    b.rank_nbr.fill_(math.nan)
    b.rank_nbr_aux.fill_(math.nan)
    b.begin()
    _assert_aliases(b, drv)
    _assert_nbr_buffers([b], [drv], accel)
    if accel:
        for a in drv.local_agents.values():
            assert not torch.equal(a.Y, a.X)


def test_exchange_maps_world2():
    """Two ranks built one after the other in this process (no
    collective): 5 agents, ranks own {0, 2, 4} and {1, 3}, payload sizes
    differ and glob_off is non-zero. The gathered [X | Y] payloads are
    handed to both ranks' _scatter by hand."""
    from dpo_amd.packed import PackedBackend
    drvs = [_l2_driver(3, 5, "interleaved", True, kr.StubComm(rk, 2))[0]
            for rk in (0, 1)]
    assert [sorted(d.local_agents) for d in drvs] == [[0, 2, 4], [1, 3]]
    bs = [PackedBackend(d) for d in drvs]
    for drv in drvs:
        for rb, a in drv.local_agents.items():
            _fill(a.X, 52, rb)
            _fill(a.Y, 53, rb)
    assert bs[0].sizes == bs[1].sizes and bs[0].sizes[0] != bs[0].sizes[1]
    payload = [torch.cat([b._pack(), b._pack(aux=True)]) for b in bs]
    assert [p.numel() for p in payload] == [2 * s for s in bs[0].sizes]
    for b, drv in zip(bs, drvs):
        assert set(b.scatter_rank) == {0, 1}
        b.rank_nbr.fill_(math.nan)
        b.rank_nbr_aux.fill_(math.nan)
        b._scatter([f[:s] for f, s in zip(payload, b.sizes)])
        b._scatter([f[s:] for f, s in zip(payload, b.sizes)], aux=True)
        _assert_aliases(b, drv)
    _assert_nbr_buffers(bs, drvs, True)


# ---------------------------------------------------------------------
# 2. per-round evaluation against the centralized problem
# ---------------------------------------------------------------------
def _check_eval(drv, b, meas, n, d, weights_global=None):
    row = b.eval_buffer(1)[0]
    b.evaluate(row)
    torch.cuda.synchronize()
    got = row.cpu().numpy()
    refs, bounds = [], []
    for rb, a in drv.local_agents.items():
        ref, bd = kr.agent_eval_ref(a, a._nbr_buffer, a._all_weights_dev)
        print(f"agent {rb}: err/bound {np.abs(got[rb] - ref) / bd}")
        assert (np.abs(got[rb] - ref) <= bd).all(), (rb, got[rb], ref, bd)
        refs.append(ref)
        bounds.append(bd)
    bounds = np.array(bounds)
    cost, gn2, b_cost, b_gn2 = kr.central_eval_ref(
        meas, n, d, drv.gather_lifted_iterate(), weights_global)
    assert cost > 1.0 and gn2 > 1.0
    assert abs(2.0 * (got[:, 0] - got[:, 1]).sum() - cost) \
        <= 2.0 * bounds[:, :2].sum() + b_cost
    assert abs(got[:, 2].sum() - gn2) <= bounds[:, 2].sum() + b_gn2


@pytest.mark.parametrize("route", ["group", "no_group", "stream"])
@pytest.mark.parametrize("d", [2, 3])
def test_evaluate_matches_centralized(d, route, monkeypatch):
    if route == "no_group":
        monkeypatch.setenv("DPO_NO_GROUP", "1")
    else:
        monkeypatch.delenv("DPO_NO_GROUP", raising=False)
    drv, meas, n = _l2_driver(
        d, 4, "interleaved",
        selection="greedy" if route == "stream" else "colored")
    b = _packed(drv)
    assert b.fanout_eval == (route != "stream")
    assert (b.group is None) == (route == "no_group")
    for rb, a in drv.local_agents.items():
        _fill_manifold(a.X, d, 54, d, rb)
    b.begin()
    _check_eval(drv, b, meas, n, d)


def _global_weights(drv, ma, part):
    """Global per-measurement weights from the agents' device weights;
    the two co-owners of a shared edge must hold the same bits."""
    w = np.full(len(ma), np.nan)
    for rb, a in drv.local_agents.items():
        wa = a._all_weights_dev.cpu().numpy()
        idx = np.concatenate(kr.agent_edge_index(ma.p1, ma.p2, part, rb))
        assert len(idx) == len(wa)
        old = w[idx]
        assert (np.isnan(old) | (old == wa)).all(), rb
        w[idx] = wa
    assert not np.isnan(w).any()
    return w


def test_evaluate_after_reweight_matches_centralized():
    drv, ma, n = _gnc_driver()
    b = _packed(drv)
    b.begin()
    b.reweight()
    w = _global_weights(drv, ma, kr.interleaved_partition(n, 4))
    assert ((w > 0) & (w < 1)).sum() >= 10
    _check_eval(drv, b, ma, n, 3, w)


# ---------------------------------------------------------------------
# 3. Nesterov bookkeeping
# ---------------------------------------------------------------------
def _check_polar(out, M, d, label):
    """out against the SVD polar factor of M, per pose within
    8 eps cond(M)^2 + 16 eps; translation rows within 4 eps |terms|."""
    err, orth = kr.polar_errors(out, M, d)
    tol = kr.polar_tol(kr.block_conds(M, d))
    print(f"{label}: max err/tol {np.max(err / tol):.3f}")
    assert (err <= tol).all() and (orth <= tol).all(), label


def test_nesterov_pre_and_post():
    drv, _, _ = _l2_driver(3, 4, "interleaved", True)
    b = _packed(drv)
    K, d = 4, 3
    for rb, a in drv.local_agents.items():
        _fill_manifold(a.X, d, 55, rb)
        _fill_manifold(a.V, d, 56, rb)
        a.gamma = 0.37
        X, V = a.X.cpu(), a.V.cpu()
        a._packed_nesterov_pre()
        gamma = (1 + math.sqrt(1 + 4 * K * K * 0.37 * 0.37)) / (2 * K)
        alpha = 1.0 / (gamma * K)
        assert a.gamma == gamma and a.alpha == alpha
        assert torch.equal(a._XPrev_packed, a.X)
        M = (1 - alpha) * X + alpha * V
        Y = a.Y.cpu()
        _check_polar(Y, M, d, f"Y agent {rb}")
        tr = slice(d, None, d + 1)
        assert ((Y[tr] - M[tr]).abs() <= 4 * EPS * (
            (1 - alpha) * X[tr].abs() + alpha * V[tr].abs())).all()
        # the solve's result stands in as another manifold point
        _fill_manifold(a.X, d, 57, rb)
        X1 = a.X.cpu()
        a.iteration_number = 1      # (1 + 1) % 30: no restart
        a._packed_nesterov_post(True)
        M = V + gamma * (X1 - Y)
        V1 = a.V.cpu()
        _check_polar(V1, M, d, f"V agent {rb}")
        assert ((V1[tr] - M[tr]).abs() <= 4 * EPS * (
            V[tr].abs() + gamma * (X1[tr].abs() + Y[tr].abs()))).all()
        assert a.gamma == gamma and torch.equal(a.X.cpu(), X1)


def test_restart_round_state_and_who_solves():
    """At a restart (PGOAgent.cpp:1040-1052) V = Y = X bitwise and
    gamma = alpha = 0 on every agent; X leaves XPrev exactly on the
    agents that optimize this round, the others are put back on it."""
    drv, _, _ = _l2_driver(3, 4, "interleaved", True)
    b = _packed(drv)
    b.begin()
    interval = next(iter(drv.local_agents.values())).params.restart_interval
    for a in drv.local_agents.values():
        a.iteration_number = interval - 2
    active = drv._color_active[0]
    assert 0 < len(active) < 4
    prev = {rb: a.X.clone() for rb, a in drv.local_agents.items()}
    b.select(active)
    b.solve()
    for rb, a in drv.local_agents.items():
        assert a.iteration_number == interval - 1
        a._packed_nesterov_post(rb in active)
    moved = set()
    for rb, a in drv.local_agents.items():
        assert torch.equal(a.V, a.X) and torch.equal(a.Y, a.X), rb
        assert a.gamma == 0.0 and a.alpha == 0.0
        assert torch.equal(a._XPrev_packed, prev[rb])
        if not torch.equal(a.X, prev[rb]):
            moved.add(rb)
    assert moved == set(active)


# ---------------------------------------------------------------------
# 4. round schedule
# ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["l2-accel", "gnc-plain", "gnc-accel"])
def test_packed_schedule_matches_reference_cadence(case):
    """Same lists as tests/test_packed_rounds.py pins for the dict path:
    kr.schedule_model is the reference's cadence."""
    accel, robust = case != "gnc-plain", case != "l2-accel"
    drv = _gnc_driver(accel)[0] if robust else \
        _l2_driver(3, 4, "interleaved", True)[0]
    from dpo_amd.packed import PackedBackend
    first, again = kr.run_schedule(drv)
    assert isinstance(drv._packed, PackedBackend)
    kr.check_schedule(first, sum(kr.SCHED_RUNS), 4, accel, robust)
    kr.check_schedule(again, kr.SCHED_RUNS[1], 4, accel, robust)
    for a in drv.local_agents.values():
        assert a.iteration_number == kr.SCHED_RUNS[1]


# ---------------------------------------------------------------------
# 5. GNC re-weighting against the host code
# ---------------------------------------------------------------------
def test_gnc_reweight_matches_host():
    pk, ma, n = _gnc_driver()
    part = kr.interleaved_partition(n, 4)
    b = _packed(pk)
    b.begin()
    a0 = pk.local_agents[0]
    mu, barc = a0.robust_cost.mu, a0.robust_cost.params.gnc_barc
    tol = kr.gnc_tol(mu)

    # the kernel alone: odometry and edges the other robot owns untouched
    before = {rb: a._all_weights_dev.clone()
              for rb, a in pk.local_agents.items()}
    for rb, a in pk.local_agents.items():
        a._packed_update_weights()
        upd = a._gnc["upd"].bool().cpu()
        widx = a._gnc["widx"].cpu()
        keep = torch.ones(before[rb].numel(), dtype=torch.bool)
        keep[widx[upd]] = False
        assert keep[:len(a._odo_ma)].all() and (~keep).sum() > 0
        assert torch.equal(a._all_weights_dev.cpu()[keep],
                           before[rb].cpu()[keep]), rb
    b.reweight()
    assert a0.robust_cost.mu == mu * a0.robust_cost.params.gnc_mu_step

    host, _, _ = _gnc_driver(soa=False)
    hb_ = host._backend()
    assert isinstance(hb_, _DictBackend)
    hb_.begin()
    for a in host.local_agents.values():
        assert a.robust_cost.mu == mu
        a.update_loop_closures_weights()
    host._dict_sync_weights()

    r_sq, bound = kr.gnc_edge_residuals(ma, kr.gnc_fixture()[2])
    near = kr.gnc_near_threshold(r_sq, bound, mu, barc)
    n_lc = n_out = 0
    for rb, a in pk.local_agents.items():
        h = host.local_agents[rb]
        want = np.array([m.weight for m in h.private_lc + h.shared_lc])
        n_odo = len(a._odo_ma)
        got = a._all_weights_dev.cpu().numpy()
        assert (got[:n_odo] == 1.0).all()
        _, priv, shared = kr.agent_edge_index(ma.p1, ma.p2, part, rb)
        idx = np.concatenate([priv, shared])
        assert len(idx) == len(want) == len(got) - n_odo
        ok = ~near[idx]
        n_lc += len(idx)
        n_out += int((~ok).sum())
        err = np.abs(got[n_odo:] - want)
        print(f"agent {rb}: max err/tol {err[ok].max() / tol:.3f}")
        assert (err[ok] <= tol).all(), rb
        assert ((want > 0) & (want < 1)).sum() >= 3
        # Q values rebuilt on the device against the host assembler
        qa = a._q_assembler
        w = torch.from_numpy(got)
        ref = qa.assemble(w.clone()).vals.clone()
        mag = torch.zeros_like(ref)
        mag.index_add_(0, qa._slots,
                       qa._blocks.abs() * w[qa._edge_of].abs()[:, None, None])
        terms = int(torch.bincount(qa._slots).max()) + 1
        assert ((a.problem.Q.vals.cpu() - ref).abs()
                <= kr.sop_bound(mag, terms)).all(), rb
    assert n_out <= 0.02 * n_lc
    # co-owners hold the same bits (asserted while merging)
    _global_weights(pk, ma, part)


# ---------------------------------------------------------------------
# 6. whole rounds, packed against dict on the same device
# ---------------------------------------------------------------------
def _round_pair(accel):
    pk, _, _ = _l2_driver(3, 4, "interleaved", accel)
    dc, _, _ = _l2_driver(3, 4, "interleaved", accel)
    dc._backend = lambda: _DictBackend(dc)
    for rb in pk.local_agents:
        assert torch.equal(pk.local_agents[rb].X, dc.local_agents[rb].X)
    return pk, dc


def _state(drv):
    return {rb: a.X.detach().cpu().clone()
            for rb, a in drv.local_agents.items()}


def _compare_rounds(pk, dc, rounds, accel=False):
    """Run `rounds` rounds on both and compare. An agent has moved when
    X is no longer bit-identical; in the first accelerated round an agent
    that does not optimize lands on polar(X), so there X is compared with
    the CPU polar factor under the polar bound at cond 1."""
    sp0, sd0 = _state(pk), _state(dc)
    thresh = 0.0
    if accel:
        thresh = float(kr.polar_tol(1.0))
        sp0 = {rb: cpu_ref.stiefel_project(X, 3) for rb, X in sp0.items()}
        sd0 = {rb: cpu_ref.stiefel_project(X, 3) for rb, X in sd0.items()}
    rp = pk.run(max_iters=rounds, gradnorm_tol=0.0)
    rd = dc.run(max_iters=rounds, gradnorm_tol=0.0)
    assert pk._packed is not None and dc._packed is None
    sp, sd = _state(pk), _state(dc)
    moved_p = {rb for rb in sp if (sp[rb] - sp0[rb]).abs().max() > thresh}
    moved_d = {rb for rb in sd if (sd[rb] - sd0[rb]).abs().max() > thresh}
    assert moved_p == moved_d
    for rb in sp:
        err = float((sp[rb] - sd[rb]).abs().max())
        print(f"agent {rb}: max |X packed - X dict| {err:.3e}")
        assert err <= 1e-6, rb
    assert len(rp.trace) == len(rd.trace) == rounds
    for (ca, ga), (cb, gb) in zip(rp.trace, rd.trace):
        assert abs(ca - cb) < 1e-6 * max(1.0, abs(cb))
        assert abs(ga - gb) < 1e-4 * max(1.0, gb)
    return moved_p


def test_plain_rounds_match_dict_path():
    pk, dc = _round_pair(False)
    moved = _compare_rounds(pk, dc, 1)
    assert moved == set(pk._color_active[0])
    # rounds 2 and 3; the colour cycle starts over with every run()
    moved = _compare_rounds(pk, dc, 2)
    assert moved and moved <= set(pk._color_active[0]) | set(
        pk._color_active[1 % pk._num_colors])
    for rb, a in pk.local_agents.items():
        assert a.iteration_number == dc.local_agents[rb].iteration_number == 3


def test_accelerated_first_round_matches_dict_path():
    """Round 1 is the one accelerated round both paths define alike
    (alpha = 1, Y = X, aux poses = poses). From round 2 on the packed
    path solves against the neighbours' aux poses of this round, the
    dict path against those published a round earlier, so
    after three rounds only the bookkeeping is compared. An agent that
    does not optimize moves to polar(X)."""
    pk, dc = _round_pair(True)
    moved = _compare_rounds(pk, dc, 1, accel=True)
    assert moved == set(pk._color_active[0])
    pk.run(max_iters=2, gradnorm_tol=0.0)
    dc.run(max_iters=2, gradnorm_tol=0.0)
    K = 4
    for rb, a in pk.local_agents.items():
        h = dc.local_agents[rb]
        assert a.iteration_number == h.iteration_number == 3
        # the packed path has prepared the next round's gamma already
        g = (1 + math.sqrt(1 + 4 * K * K * h.gamma * h.gamma)) / (2 * K)
        assert a.gamma == g and a.alpha == 1.0 / (g * K)
