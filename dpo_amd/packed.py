"""Packed GPU backend of the distributed RBCD round loop.

DistributedRBCDDriver.run() owns the round policy (active set, readback
ring, trace, stop test); this object owns the device mechanism for one
rank: consolidated X / neighbor buffers, the single pack and scatter
index ops around the boundary-pose all-gather, the native solve and eval
fan-out, GNC re-weighting and the Nesterov bookkeeping. Payloads are
device tensors end to end and nothing here syncs with the host.

Built once per driver, on the first run() that takes the packed path;
the buffers (and therefore the hipGraph cache keys of every agent) stay
fixed across run() calls, so repeated bench episodes replay hot graphs.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .ops.hip_backend import DeviceGroup

Tensor = torch.Tensor


class PackedBackend:
    def __init__(self, drv):
        self.drv = drv
        self.comm = drv.comm
        self.dev = dev = torch.device(drv.device)
        self.dh, self.r = drv.dh, drv.r
        self.accel = drv.acceleration
        self.agents = drv.local_agents
        blk = self.dh * self.r
        pub_idx = drv.pub_idx
        # debug knobs, fixed per driver
        self.time_phases = os.environ.get("DPO_TIME_PHASES", "0") == "1"
        no_group = os.environ.get("DPO_NO_GROUP", "0") == "1"

        # per-rank payload lengths and each agent's offset inside its
        # owner's payload
        self.sizes = [sum(len(pub_idx[rb]) * blk for rb in agents)
                      for agents in drv.rank_agents]
        glob_off = {}
        for agents in drv.rank_agents:
            o = 0
            for rb in agents:
                glob_off[rb] = o
                o += len(pub_idx[rb]) * blk

        # ---- consolidated per-rank buffers --------------------------
        # One X buffer and one neighbor buffer for all local agents:
        # pack/scatter become single index ops, and each agent's tensors
        # are stable contiguous views (the hipGraph keys stay valid).
        my = drv.rank_agents[self.comm.rank]
        for rb in my:
            self.agents[rb]._ensure_packed(dev)
        pose_off = {}
        off = 0
        for rb in my:
            pose_off[rb] = off
            off += self.agents[rb].n
        self.rank_X = torch.zeros(off * self.dh, self.r,
                                  dtype=torch.float64, device=dev)
        for rb in my:
            a = self.agents[rb]
            o = pose_off[rb] * self.dh
            self.rank_X[o:o + a.n * self.dh].copy_(a.X)
            a.X = self.rank_X[o:o + a.n * self.dh]
            if a.params.acceleration:
                a.Y = a.X.clone()
                a.V = a.X.clone()
        slot_off = {}
        soff = 0
        for rb in my:
            slot_off[rb] = soff
            soff += max(len(self.agents[rb]._nbr_slot_order), 1)
        self.rank_nbr = torch.zeros(max(soff, 1), self.dh, self.r,
                                    dtype=torch.float64, device=dev)
        self.rank_nbr_aux = torch.zeros_like(self.rank_nbr)
        for rb in my:
            a = self.agents[rb]
            ns = max(len(a._nbr_slot_order), 1)
            a._nbr_buffer = self.rank_nbr[slot_off[rb]:slot_off[rb] + ns]
            a._nbr_buffer_aux = \
                self.rank_nbr_aux[slot_off[rb]:slot_off[rb] + ns]

        # single pack index: global pose-block rows of every public pose
        self.pack_rows = torch.tensor(
            [pose_off[rb] + p for rb in my for p in pub_idx[rb]],
            dtype=torch.int64, device=dev)
        self.pub_rows = {
            rb: torch.tensor(pub_idx[rb], dtype=torch.int64, device=dev)
            for rb in my}
        # scatter: one (src positions -> nbr slots) pair per SOURCE rank
        pub_payload_pos = {}  # (nb agent, pose) -> index in owner payload
        for rb in range(drv.num_robots):
            base = glob_off[rb] // blk
            for k, p in enumerate(pub_idx[rb]):
                pub_payload_pos[(rb, p)] = base + k
        per_src = {}
        for rb in my:
            for slot, (nb, p) in enumerate(self.agents[rb]._nbr_slot_order):
                src, dst = per_src.setdefault(drv.owner[nb], ([], []))
                src.append(pub_payload_pos[(nb, p)])
                dst.append(slot_off[rb] + slot)
        self.scatter_rank = {
            rk: (torch.tensor(src, dtype=torch.int64, device=dev),
                 torch.tensor(dst, dtype=torch.int64, device=dev))
            for rk, (src, dst) in per_src.items()}

        # persistent eval buffers: stable pointers keep the native
        # gather/eval graph caches hot across repeated run() calls
        self.evalmat = torch.zeros(1, drv.num_robots, 3,
                                   dtype=torch.float64, device=dev)
        self.evalring = torch.zeros(0, drv.num_robots, 3,
                                    dtype=torch.float64, device=dev)

        # ---- robust (GNC) state --------------------------------------
        self.robust = not drv._robust_is_l2()
        self.w_exch = torch.zeros(drv._n_cross if self.robust else 0,
                                  dtype=torch.float64, device=dev)
        self.cross_map = {}
        self.cross_owned = {}
        if self.robust:
            for rb, a in self.agents.items():
                a._packed_gnc_setup(dev)
                self.cross_map[rb] = torch.from_numpy(
                    drv._cross_map[rb]).to(dev)
                self.cross_owned[rb] = torch.from_numpy(
                    np.nonzero(drv._cross_owned[rb])[0]).to(dev)
        params = next(iter(self.agents.values())).params \
            if self.agents else None
        self.gnc_period = params.robust_opt_inner_iters if params else 30
        self.inner_tol = params.inner_tol if params else 1e-2
        self.tr_steps = params.tr_max_iterations if params else 1

        # ---- dispatch --------------------------------------------------
        # native multi-agent fan-out (one C call per phase, fixed
        # pointers keep the per-agent hipGraph caches hot)
        self.group = None
        self.group_lidx = {}
        self.group_all = False
        if self.agents and not no_group:
            rbs = sorted(self.agents)
            self.group = DeviceGroup(
                [self.agents[rb]._dev_solver for rb in rbs],
                [self.agents[rb].X for rb in rbs],
                [self.agents[rb]._nbr_buffer for rb in rbs], rbs)
            self.group_lidx = {rb: i for i, rb in enumerate(rbs)}
            self.group_all = len(rbs) == drv.num_robots
        # accelerated solves read the aux neighbor buffer: per-agent path
        self.group_solve = self.group is not None and not self.accel
        # schedules that decide on the host every round evaluate on the
        # torch stream; the colored ones fan out on the agents' streams
        self.fanout_eval = drv.selection in ("colored", "colored_greedy")
        self._gids = {}        # active set -> ctypes id array (group solve)
        self._active = []      # this round's local active agents
        self._active_rbs = set()
        self._active_ids = None

    # -- boundary-pose exchange ------------------------------------------
    def _pack(self, aux: bool = False) -> Tensor:
        if not self.drv.rank_agents[self.comm.rank]:
            return torch.zeros(0, dtype=torch.float64, device=self.dev)
        if aux:
            parts = []
            for rb, idx in self.pub_rows.items():
                a = self.agents[rb]
                src = a.Y if a.Y is not None else a.X
                parts.append(src.view(a.n, self.dh, self.r)
                             .index_select(0, idx).reshape(-1))
            return torch.cat(parts)
        Xb = self.rank_X.view(-1, self.dh, self.r)
        return Xb.index_select(0, self.pack_rows).reshape(-1)

    def _scatter(self, flats, aux: bool = False) -> None:
        target = self.rank_nbr_aux if aux else self.rank_nbr
        for rk, (src_idx, dst_slots) in self.scatter_rank.items():
            blkv = flats[rk].view(-1, self.dh, self.r)
            target.index_copy_(0, dst_slots, blkv.index_select(0, src_idx))

    def _exchange(self, prepare: bool = True) -> None:
        """One all-gather per round. Accelerated mode computes the next
        Nesterov aux poses Y first and sends [X | Y] halves per rank in
        that same collective: nothing updates X or V between here and
        the next solve, so Y is the value the solve needs."""
        if not self.accel:
            self._scatter(self.comm.all_gather_flat(self._pack(),
                                                    self.sizes))
            return
        if prepare:
            for a in self.agents.values():
                a._packed_nesterov_pre()
        payload = torch.cat([self._pack(), self._pack(aux=True)])
        flats = self.comm.all_gather_flat(payload,
                                          [2 * s for s in self.sizes])
        self._scatter([f[:s] for f, s in zip(flats, self.sizes)])
        self._scatter([f[s:] for f, s in zip(flats, self.sizes)], aux=True)

    # -- operations of the round loop ------------------------------------
    def eval_buffer(self, rounds: int) -> Tensor:
        """Zeroed (rounds, num_robots, 3) device buffer."""
        if rounds == 1:
            buf = self.evalmat
        else:
            if self.evalring.shape[0] != rounds:
                self.evalring = torch.zeros(
                    rounds, self.drv.num_robots, 3, dtype=torch.float64,
                    device=self.dev)
            buf = self.evalring
        buf.zero_()
        return buf

    def begin(self) -> None:
        """Round-0 pre-exchange so G terms exist before the first solve.
        A fresh or restored accelerated state (gamma == 0) gets its first
        gamma, alpha and Y here; after an earlier run() the last exchange
        has prepared them already and the momentum carries on, as
        iterate() carries it on the dict path."""
        self._exchange(prepare=all(a.gamma == 0.0
                                   for a in self.agents.values()))

    def reweight_due(self, round_counter: int) -> bool:
        """shouldUpdateLoopClosureWeights (PGOAgent.cpp:1174-1179) with
        the already advanced round number: rounds P-1, 2P-1, ..."""
        return self.robust and (round_counter + 1) % self.gnc_period == 0

    def reweight(self) -> None:
        """GNC re-weighting round (reference iterate():
        shouldUpdateLoopClosureWeights -> update -> mu step). Owners
        compute the weights of inter-robot loop closures; one all-reduce
        hands them to the co-owners."""
        for a in self.agents.values():
            a._packed_update_weights()
        self.w_exch.zero_()
        for rb, a in self.agents.items():
            own = self.cross_owned[rb]
            if own.numel():
                pos = self.cross_map[rb].index_select(0, own)
                self.w_exch.index_copy_(
                    0, pos, a._w_shared_dev.index_select(0, own))
        self.comm.all_reduce_sum_(self.w_exch)
        for rb, a in self.agents.items():
            if self.cross_map[rb].numel():
                a._w_shared_dev.copy_(
                    self.w_exch.index_select(0, self.cross_map[rb]))
        for a in self.agents.values():
            a._packed_rebuild_q()
            a.robust_cost.update()
        if self.accel:
            # initializeAcceleration (PGOAgent.cpp:663-666): momentum
            # starts over on the re-weighted problem. The aux poses sent
            # last round belong to the old momentum, so they are sent
            # again (gamma = 0 gives alpha = 1 and Y = X).
            for a in self.agents.values():
                a.V.copy_(a.X)
                a.gamma = 0.0
                a.alpha = 0.0
            self._exchange()

    def select(self, active) -> None:
        """Fix this round's active agents. Accelerated mode moves every
        other agent to its aux point here, before the solves. Called
        once per round: it advances every agent's iteration_number, the
        count iterate() keeps on the dict path (restart cadence)."""
        for a in self.agents.values():
            a.iteration_number += 1
        self._active_rbs = set(active)
        if self.group_solve:
            key = tuple(active)
            ids = self._gids.get(key)
            if ids is None:
                ids = self._gids[key] = self.group.ids(
                    [self.group_lidx[rb] for rb in active
                     if rb in self.agents])
            self._active_ids = ids
            return
        self._active = [self.agents[rb] for rb in active
                        if rb in self.agents]
        if self.accel:
            for rb, a in self.agents.items():
                if rb not in active:
                    a.X.copy_(a.Y)

    def solve(self) -> None:
        """Concurrent active agents' solves overlap on per-agent HIP
        streams (data-flow fences in dpo_ops.hip order the cached
        solve/eval graphs against this stream's pack/scatter)."""
        if self.group_solve:
            ids = self._active_ids
            if len(ids):
                for _ in range(self.tr_steps):
                    self.group.solve_start(ids, tol=self.inner_tol)
                    self.group.solve_finish(ids)
            return
        for k in range(self.tr_steps):
            for a in self._active:
                a._packed_solve_async(self.accel, first=(k == 0))
            for a in self._active:
                a._packed_solve_finish()

    def exchange(self, it: int) -> None:
        if self.accel:
            for rb, a in self.agents.items():
                a._packed_nesterov_post(rb in self._active_rbs)
        self._exchange()

    def evaluate(self, row: Tensor) -> None:
        """Enqueue every local agent's [f, 0.5<X,G>, ||rgrad||^2] (fresh
        neighbor data) into its row of the (num_robots, 3) device matrix
        `row`; rows of other ranks' agents are left zero."""
        if not self.fanout_eval:
            row.zero_()
            for rb, a in self.agents.items():
                row[rb] = a._packed_eval()
        elif self.group is not None:
            # native fan-out: one C call + one gather kernel
            if not self.group_all:
                row.zero_()
            self.group.eval_all(row)
        else:
            row.zero_()
            for a in self.agents.values():
                a._packed_eval_async()
            for rb, a in self.agents.items():
                row[rb] = a._packed_eval_join()

    def finish(self) -> None:
        # dict-path state (global anchor for rounding)
        self.drv._sync_anchor()
