"""Distributed multi-robot RBCD driver: one process per GPU over RCCL.

Maps agents to ranks (agent a -> rank a % world_size); each round:
  1. the active agent(s) run the device-resident local solve,
  2. one packed all-gather moves every agent's public poses + status
     (payload is tens of KB — latency-bound over xGMI, so one fused
     collective beats per-neighbor p2p),
  3. each agent rebuilds G from fresh neighbor poses and evaluates its
     LOCAL Riemannian gradient norm — which equals the block of the
     CENTRALIZED gradient (the local Q carries the shared-edge diagonal
     corrections and G carries the cross terms, so local grad == central
     block grad when neighbor data is fresh), and the centralized cost is
     sum_agents(f_local - 0.5 <X, G>). One small all-reduce therefore
     reproduces the reference driver's centralized evaluation
     (MultiRobotExample.cpp:279-325) without gathering trajectories.
  4. greedy argmax selection / colored schedule, termination check.

Works identically under gloo (CPU, CI) and RCCL (MI355X); also usable
with world_size == 1 (all agents on one device).
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .agent import PGOAgent
from .chordal import chordal_initialization
from .comm import Comm
from .driver import RBCDResult
from .io_g2o import adjacency_from_measurements
from .partition import (contiguous_partition, multilevel_partition,
                        partition_measurements)
from .types import PGOAgentParams, PGOAgentState, PGOAgentStatus, \
    RelativeSEMeasurement, RobustCostType

Tensor = torch.Tensor
STATUS_LEN = 6


def _adjacency_from_ma(ma, num_poses):
    nbr = [set() for _ in range(num_poses)]
    for a, b in zip(ma.p1, ma.p2):
        if a != b:
            nbr[a].add(int(b))
            nbr[b].add(int(a))
    return [sorted(x) for x in nbr]


class _PhaseClock:
    """DPO_TIME_PHASES=1: host time spent in each phase call of a round
    (perf_counter reads only; nothing is synchronized)."""

    def __init__(self, on: bool):
        self.on = on
        self.t = dict.fromkeys(
            ("solve_enq", "finish", "pack", "eval", "flush"), 0.0)

    def __call__(self, phase: str, fn, *args):
        if not self.on:
            return fn(*args)
        t = time.perf_counter()
        out = fn(*args)
        self.t[phase] += time.perf_counter() - t
        return out


class _DictBackend:
    """Round mechanism over the agents' host-side neighbor dicts: runs
    on CPU, over gloo, and with agents that are not yet initialized. The
    operations mirror dpo_amd.packed.PackedBackend."""

    time_phases = False

    def __init__(self, drv: "DistributedRBCDDriver"):
        self.drv = drv
        self.sync_weights = (drv.robust != RobustCostType.L2
                             and not drv._soa and drv._n_cross > 0)
        self.active: List[int] = []

    def eval_buffer(self, rounds: int) -> Tensor:
        return torch.zeros(rounds, self.drv.num_robots, 3,
                           dtype=torch.float64)

    def begin(self) -> None:
        """Round-0 pre-exchange so G terms exist before the first solve."""
        self.exchange(0)

    def reweight_due(self, round_counter: int) -> bool:
        return False    # GNC runs inside PGOAgent.iterate on this path

    def reweight(self) -> None:
        pass

    def select(self, active: List[int]) -> None:
        self.active = active

    def solve(self) -> None:
        for rb, a in self.drv.local_agents.items():
            a.iterate(rb in self.active)
        if self.sync_weights:
            self.drv._dict_sync_weights()

    def exchange(self, it: int) -> None:
        drv = self.drv
        flats = drv.comm.all_gather_flat(drv._pack_rank_payload(),
                                         drv.rank_sizes)
        drv._unpack_and_update(flats)

    def evaluate(self, row: Tensor) -> None:
        row.zero_()
        for rb, a in self.drv.local_agents.items():
            row[rb] = torch.from_numpy(self.drv._eval_scalars(a))

    def finish(self) -> None:
        pass


class DistributedRBCDDriver:
    def __init__(self,
                 measurements: Sequence[RelativeSEMeasurement],
                 num_poses: int,
                 num_robots: int,
                 comm: Comm,
                 r: int = 5,
                 partition: str | Sequence[int] = "multilevel",
                 acceleration: bool = False,
                 robust: RobustCostType = RobustCostType.L2,
                 device: str = "cpu",
                 verbose: bool = False,
                 selection: str = "greedy",
                 inner_tol: float = 1e-2,
                 tr_max_iterations: int = 1):
        self.comm = comm
        self.num_robots = num_robots
        self.verbose = verbose
        self.selection = selection
        self.device = device
        from .measurements import MeasurementArray
        self._soa = isinstance(measurements, MeasurementArray)
        if (self._soa and robust != RobustCostType.L2
                and not str(device).startswith("cuda")):
            raise ValueError(
                "robust (non-L2) SoA driver needs a cuda device: GNC "
                "weight updates run in the packed GPU path "
                "(_packed_update_weights); on CPU pass object-mode "
                "measurements (list of RelativeSEMeasurement)")
        d = measurements.d if self._soa else measurements[0].d
        self.d, self.r, self.n_global = d, r, num_poses
        self.dh = d + 1
        self.acceleration = acceleration
        self.robust = robust

        # ---- identical partition on every rank (deterministic) ---------
        if isinstance(partition, str):
            if partition == "contiguous":
                part = contiguous_partition(num_poses, num_robots)
            else:
                if self._soa:
                    adj = _adjacency_from_ma(measurements, num_poses)
                else:
                    adj = adjacency_from_measurements(measurements,
                                                      num_poses)
                part = multilevel_partition(adj, num_robots)
        else:
            part = list(partition)
        if self._soa:
            from .measurements import partition_measurement_array
            (odometry, private_lc, shared_lc, local_idx, global_of,
             self.pose_counts) = partition_measurement_array(
                measurements, num_poses, part, num_robots)
            self.pose_to_index = {}
            for rb in range(num_robots):
                for i, g in enumerate(global_of[rb]):
                    self.pose_to_index[(rb, int(i))] = int(g)
            # global cross-edge exchange maps (GNC weight sync)
            partv = np.asarray(part, dtype=np.int64)
            src_r = partv[measurements.p1]
            dst_r = partv[measurements.p2]
            cross = np.nonzero(src_r != dst_r)[0]
            self._n_cross = len(cross)
            cross_rank = {int(g): i for i, g in enumerate(cross)}
            self._cross_map = []     # per agent: global positions
            self._cross_owned = []   # per agent: owned mask
            for rb in range(num_robots):
                sel = np.nonzero((src_r != dst_r)
                                 & ((src_r == rb) | (dst_r == rb)))[0]
                self._cross_map.append(
                    np.array([cross_rank[int(g)] for g in sel],
                             dtype=np.int64))
                other = np.where(src_r[sel] == rb, dst_r[sel], src_r[sel])
                self._cross_owned.append(other > rb)
        else:
            (odometry, private_lc, shared_lc, self.pose_map,
             self.pose_to_index, self.pose_counts) = partition_measurements(
                measurements, num_poses, part, num_robots)
            # global cross-edge enumeration (GNC weight sync on the dict
            # path; owner-computes rule — PGOAgent.cpp:1201-1244): each
            # inter-robot loop closure gets one global slot, keyed by its
            # (global src, global dst) pose pair in input order.
            partv = np.asarray(part, dtype=np.int64)
            cross_fifo: Dict[Tuple[int, int], List[int]] = {}
            n_cross = 0
            for m in measurements:
                if partv[m.p1] != partv[m.p2]:
                    cross_fifo.setdefault((m.p1, m.p2), []).append(n_cross)
                    n_cross += 1
            self._n_cross = n_cross
            # per-robot: shared_lc edge k -> global cross slot, owned mask
            self._cross_map = []
            self._cross_owned = []
            taken: Dict[Tuple[int, int], int] = {}
            for rb in range(num_robots):
                idxs = []
                owned = []
                seen: Dict[Tuple[int, int], int] = {}
                for m in shared_lc[rb]:
                    g1 = self.pose_to_index[(m.r1, m.p1)]
                    g2 = self.pose_to_index[(m.r2, m.p2)]
                    k = seen.get((g1, g2), 0)
                    seen[(g1, g2)] = k + 1
                    idxs.append(cross_fifo[(g1, g2)][k])
                    other = m.r2 if m.r1 == rb else m.r1
                    owned.append(other > rb)
                self._cross_map.append(np.asarray(idxs, dtype=np.int64))
                self._cross_owned.append(np.asarray(owned, dtype=bool))

        # ---- agents owned by this rank ---------------------------------
        self.owner = [a % comm.world_size for a in range(num_robots)]
        self.local_agents: Dict[int, PGOAgent] = {}
        from .manifold import lifting_matrix
        YL = lifting_matrix(d, r)
        if self._soa:
            # global-frame initialization: an externally provided warm
            # start (ma.warm_start) wins; else L2 mode runs the SoA/GPU
            # chordal init (vectorized assembly + BSR-kernel PCG —
            # reference MultiRobotExample.cpp:185-202 semantics at SoA
            # scale); robust mode keeps the odometry dead-reckoning
            # prefix scan (reference PGOAgent.cpp:952-957 does not trust
            # loop closures before GNC).
            if getattr(measurements, "warm_start", None) is not None:
                T_chordal_pre = measurements.warm_start
            elif robust == RobustCostType.L2:
                from .chordal import chordal_initialization_soa
                T_chordal_pre = chordal_initialization_soa(
                    measurements, num_poses, device=device,
                    tol=1e-6, max_iters=500)
            else:
                from .measurements import odometry_initialization_array
                odo_mask = (measurements.p1 + 1 == measurements.p2)
                T_chordal_pre = odometry_initialization_array(
                    d, num_poses, measurements.select(odo_mask))
        else:
            T_chordal_pre = chordal_initialization(
                d, num_poses, measurements) \
                if robust == RobustCostType.L2 else None
        Tg3 = None
        if T_chordal_pre is not None:
            Tg3 = np.ascontiguousarray(
                T_chordal_pre.reshape(d, num_poses, self.dh).transpose(
                    1, 0, 2))  # (n, d, dh) for fast slicing
        for rb in range(num_robots):
            if self.owner[rb] != comm.rank:
                continue
            p = PGOAgentParams(d=d, r=r, num_robots=num_robots,
                               acceleration=acceleration,
                               robust_cost_type=robust,
                               verbose=verbose, device=device,
                               inner_tol=inner_tol,
                               tr_max_iterations=tr_max_iterations)
            a = PGOAgent(rb, p)
            a.set_lifting_matrix(YL)
            T_init = None
            if Tg3 is not None:
                gidx = np.array([self.pose_to_index[(rb, i)]
                                 for i in range(self.pose_counts[rb])],
                                dtype=np.int64)
                T_init = np.ascontiguousarray(
                    Tg3[gidx].transpose(1, 0, 2).reshape(
                        d, self.pose_counts[rb] * self.dh))
            if self._soa:
                a.set_pose_graph_arrays(odometry[rb], private_lc[rb],
                                        shared_lc[rb], T_init=T_init)
            else:
                a.set_pose_graph(odometry[rb], private_lc[rb],
                                 shared_lc[rb], T_init=T_init)
            self.local_agents[rb] = a

        # ---- public-pose packing layout (global, same on all ranks) ----
        # For each agent: sorted local public pose indices. An agent's
        # packed payload = [status(6) | anchor(dh*r if agent 0) |
        #                   pub poses (dh*r each) | aux poses if accel].
        self.pub_idx: List[List[int]] = []
        pub_sets = self._public_pose_sets(shared_lc, num_robots)
        for rb in range(num_robots):
            self.pub_idx.append(sorted(pub_sets[rb]))
        blk = self.dh * self.r
        self.payload_sizes = []
        for rb in range(num_robots):
            sz = STATUS_LEN + len(self.pub_idx[rb]) * blk
            if rb == 0:
                sz += blk  # anchor = agent 0 pose 0
            if acceleration:
                sz += len(self.pub_idx[rb]) * blk
            self.payload_sizes.append(sz)
        self.rank_agents = [
            [rb for rb in range(num_robots) if self.owner[rb] == rk]
            for rk in range(comm.world_size)]
        self.rank_sizes = [
            sum(self.payload_sizes[rb] for rb in agents)
            for agents in self.rank_agents]

        # ---- centralized chordal init (identical on all ranks) ---------
        T_chordal = T_chordal_pre
        if T_chordal is not None:
            X_chordal = YL @ T_chordal
            for rb, a in self.local_agents.items():
                Xr = np.zeros((r, self.pose_counts[rb] * self.dh))
                for i in range(self.pose_counts[rb]):
                    g = self.pose_to_index[(rb, i)]
                    Xr[:, i * self.dh:(i + 1) * self.dh] = \
                        X_chordal[:, g * self.dh:(g + 1) * self.dh]
                a.set_x(Xr)

        # coloring for the colored schedule
        from .measurements import MeasurementArray as _MA
        nbrs = [set() for _ in range(num_robots)]
        for rb in range(num_robots):
            sl = shared_lc[rb]
            if isinstance(sl, _MA):
                if len(sl):
                    o = np.where(sl.r1 == rb, sl.r2, sl.r1)
                    nbrs[rb] = {int(x) for x in np.unique(o)}
            else:
                for m in sl:
                    o = m.r2 if m.r1 == rb else m.r1
                    nbrs[rb].add(o)
        colors = [-1] * num_robots
        for rb in range(num_robots):
            used = {colors[o] for o in nbrs[rb] if colors[o] >= 0}
            c = 0
            while c in used:
                c += 1
            colors[rb] = c
        self._colors = colors
        self._num_colors = max(colors) + 1 if colors else 1
        self._color_active = [
            [rb for rb in range(num_robots) if colors[rb] == c]
            for c in range(self._num_colors)]

        self._packed = None      # PackedBackend, built by the first GPU run
        self._round_counter = 0  # GNC cadence, counted across run() calls

    def _robust_is_l2(self) -> bool:
        return all(a.params.robust_cost_type == RobustCostType.L2
                   for a in self.local_agents.values())

    @staticmethod
    def _public_pose_sets(shared_lc, num_robots):
        from .measurements import MeasurementArray
        pub = [set() for _ in range(num_robots)]
        for rb in range(num_robots):
            sl = shared_lc[rb]
            if isinstance(sl, MeasurementArray):
                if len(sl):
                    local = np.where(sl.r1 == rb, sl.p1, sl.p2)
                    pub[rb] = {int(x) for x in np.unique(local)}
            else:
                for m in sl:
                    if m.r1 == rb:
                        pub[rb].add(m.p1)
                    else:
                        pub[rb].add(m.p2)
        return pub

    # -------------------------------------------------------------------
    def _pack_rank_payload(self) -> Tensor:
        blk = self.dh * self.r
        parts = []
        for rb in self.rank_agents[self.comm.rank]:
            a = self.local_agents[rb]
            st = a.get_status()
            parts.append(torch.from_numpy(st.as_vector()))
            if a.state == PGOAgentState.INITIALIZED:
                Xb = a.X.view(a.n, self.dh, self.r)
                idx = torch.tensor(self.pub_idx[rb], dtype=torch.int64,
                                   device=a.X.device)
                pubs = Xb.index_select(0, idx).reshape(-1).cpu()
                anchor = Xb[0].reshape(-1).cpu() if rb == 0 else None
                aux = None
                if self.acceleration and a.Y is not None:
                    Yb = a.Y.view(a.n, self.dh, self.r)
                    aux = Yb.index_select(0, idx).reshape(-1).cpu()
            else:
                pubs = torch.zeros(len(self.pub_idx[rb]) * blk,
                                   dtype=torch.float64)
                anchor = torch.zeros(blk, dtype=torch.float64) \
                    if rb == 0 else None
                aux = torch.zeros_like(pubs) if self.acceleration else None
            if anchor is not None:
                parts.append(anchor)
            parts.append(pubs)
            if self.acceleration:
                parts.append(aux)
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64)

    def _eval_scalars(self, a: PGOAgent) -> np.ndarray:
        if a.state != PGOAgentState.INITIALIZED or a.problem is None:
            return np.zeros(3)
        ok = True
        if a.has_shared_lc():
            ok = a._construct_g(a.neighbor_pose_dict)
        if not ok:
            return np.zeros(3)
        f = a.problem.f(a.X)
        half_xg = 0.5 * float((a.X * a.problem._g()).sum())
        gn2 = float(torch.linalg.norm(a.problem.rie_grad(a.X))) ** 2
        return np.array([f, half_xg, gn2])

    def _unpack_and_update(self, flats: List[Tensor]):
        """Distribute gathered public poses/statuses to local agents."""
        blk = self.dh * self.r
        statuses: Dict[int, PGOAgentStatus] = {}
        anchor = None
        pose_payloads: Dict[int, Tuple[np.ndarray, Optional[np.ndarray]]] = {}
        for rk, flat in enumerate(flats):
            f = flat.cpu().numpy()
            off = 0
            for rb in self.rank_agents[rk]:
                st = PGOAgentStatus.from_vector(f[off:off + STATUS_LEN])
                off += STATUS_LEN
                statuses[rb] = st
                if rb == 0:
                    anchor = f[off:off + blk].reshape(self.dh, self.r)
                    off += blk
                npub = len(self.pub_idx[rb])
                pubs = f[off:off + npub * blk].reshape(npub, self.dh, self.r)
                off += npub * blk
                aux = None
                if self.acceleration:
                    aux = f[off:off + npub * blk].reshape(npub, self.dh,
                                                          self.r)
                    off += npub * blk
                pose_payloads[rb] = (pubs, aux)
        # update local agents' neighbor caches
        for rb, a in self.local_agents.items():
            for nb in a.get_neighbors():
                st = statuses[nb]
                a.set_neighbor_status(st)
                pubs, aux = pose_payloads[nb]
                pd = {(nb, p): pubs[k].T.copy()
                      for k, p in enumerate(self.pub_idx[nb])}
                a.update_neighbor_poses(nb, pd)
                if self.acceleration and aux is not None \
                        and st.state == PGOAgentState.INITIALIZED:
                    ad = {(nb, p): aux[k].T.copy()
                          for k, p in enumerate(self.pub_idx[nb])}
                    a.update_aux_neighbor_poses(nb, ad)
            if anchor is not None and np.any(anchor):
                a.set_global_anchor(np.ascontiguousarray(anchor.T))
        return statuses

    def _dict_sync_weights(self) -> None:
        """All ranks: collect owner-computed GNC weights of inter-robot
        loop closures and apply them on both co-owners (one all-reduce of
        n_cross doubles; mirrors the packed path's _w_exch)."""
        w = torch.zeros(self._n_cross, dtype=torch.float64)
        for rb, a in self.local_agents.items():
            cm, own = self._cross_map[rb], self._cross_owned[rb]
            if not len(cm):
                continue
            ws = np.array([m.weight for m in a.shared_lc])
            sel = np.nonzero(own)[0]
            if len(sel):
                w[torch.from_numpy(cm[sel])] = torch.from_numpy(ws[sel])
        self.comm.all_reduce_sum_(w)
        wn = w.numpy()
        for rb, a in self.local_agents.items():
            cm = self._cross_map[rb]
            for k, m in enumerate(a.shared_lc):
                m.weight = float(wn[cm[k]])
            a.publish_weights_requested = False

    # -------------------------------------------------------------------
    # The round loop. Policy lives here; the mechanism of a round is a
    # backend: _DictBackend below (host dicts; CPU, gloo, uninitialized
    # agents) or dpo_amd.packed.PackedBackend (device tensors end to end).
    # -------------------------------------------------------------------
    def _backend(self):
        if (str(self.device).startswith("cuda")
                and (self._robust_is_l2() or self._soa)
                and all(a.state == PGOAgentState.INITIALIZED
                        for a in self.local_agents.values())):
            if self._packed is None:
                from .packed import PackedBackend
                self._packed = PackedBackend(self)
            return self._packed
        return _DictBackend(self)

    def _readback_chunk(self, gradnorm_tol: float) -> int:
        """Rounds between readbacks of the eval scalars. Evaluations land
        in a ring and are read every `chunk` rounds, so a device backend
        overlaps the eval of round t with the solves of round t+1 instead
        of draining at a host sync every round. tol <= 0 and no argmax
        selection: nothing to decide per round -> deep ring. colored with
        tol > 0: the stop test runs on ring flushes — the crossing
        iteration is read exactly from the per-round entries, only the
        break comes up to chunk-1 (monotone) rounds later. Every other
        case decides on the host each round."""
        if gradnorm_tol <= 0.0 and self.selection not in (
                "greedy", "colored_greedy"):
            return 16
        if self.selection == "colored":
            return 8
        return 1

    def _active_set(self, it: int, selected: int) -> List[int]:
        if self.selection == "colored":
            return self._color_active[it % self._num_colors]
        if self.selection == "colored_greedy":
            # the whole independent set (color) that contains the
            # max-gradient agent: greedy's targeting with colored's
            # concurrent block updates
            return self._color_active[self._colors[selected]]
        if self.selection == "round_robin":
            return [it % self.num_robots]
        return [selected]

    def run(self, max_iters: int = 1000, gradnorm_tol: float = 0.1,
            trace_file: Optional[str] = None,
            time_limit_s: Optional[float] = None) -> RBCDResult:
        backend = self._backend()
        clock = _PhaseClock(backend.time_phases)
        res = RBCDResult()
        t0 = time.perf_counter()
        chunk = self._readback_chunk(gradnorm_tol)
        # (rounds, num_robots, 3) rows of [f, 0.5<X,G>, ||rgrad||^2]
        first = backend.eval_buffer(1)
        ring = first if chunk == 1 else backend.eval_buffer(chunk)
        backend.begin()
        fout = open(trace_file, "w") if (trace_file and
                                         self.comm.rank == 0) else None
        queued: List[Tuple[int, List[int]]] = []  # evaluated, not read back

        def flush() -> Optional[int]:
            """Read the queued rounds back (the host sync), record them,
            and return the last round's max-gradient agent."""
            if not queued:
                return None
            slab = ring[:len(queued)]
            self.comm.all_reduce_sum_(slab)
            ev = slab.cpu().numpy()
            for (it, active), row in zip(queued, ev):
                cost = 2.0 * float((row[:, 0] - row[:, 1]).sum())
                gradnorm = float(np.sqrt(row[:, 2].sum()))
                res.trace.append((cost, gradnorm))
                if fout:
                    fout.write(f"{cost:.10g},{gradnorm:.10g}\n")
                if self.verbose and self.comm.rank == 0:
                    print(f"iter {it} active {active} cost {cost:.5g} "
                          f"gn {gradnorm:.5g}")
            top = int(np.argmax(ev[-1, :, 2]))
            if chunk > 1:
                slab.zero_()
            queued.clear()
            return top

        # the reference checks convergence BEFORE the first iteration
        # (MultiRobotExample.cpp:302-305): an already-converged start
        # reports 0 iterations (e.g. kitti_08)
        if gradnorm_tol > 0.0:
            backend.evaluate(first[0])
            self.comm.all_reduce_sum_(first)
            ev0 = first.cpu().numpy()[0]
            gradnorm0 = float(np.sqrt(ev0[:, 2].sum()))
            if gradnorm0 < gradnorm_tol:
                res.converged = True
                res.final_cost = 2.0 * float((ev0[:, 0] - ev0[:, 1]).sum())
                res.final_gradnorm = gradnorm0
                max_iters = 0   # no rounds: straight to the common exit
        selected = 0
        for it in range(max_iters):
            self._round_counter += 1
            if backend.reweight_due(self._round_counter):
                # weights change the cost: read back what was evaluated
                # under the old ones first (recorded, not stop-tested)
                flush()
                backend.reweight()
            active = self._active_set(it, selected)
            clock("solve_enq", backend.select, active)
            clock("finish", backend.solve)
            clock("pack", backend.exchange, it)
            clock("eval", backend.evaluate, ring[len(queued)])
            queued.append((it, active))
            res.iterations = it + 1
            if len(queued) < chunk and it + 1 < max_iters:
                continue
            scanned = len(res.trace)
            selected = clock("flush", flush)
            hit = next((k for k in range(scanned, len(res.trace))
                        if res.trace[k][1] < gradnorm_tol), None)
            if hit is not None:
                # rounds run past the crossing are dropped from the result
                res.converged = True
                res.iterations = hit + 1
                del res.trace[hit + 1:]
                break
            if time_limit_s and time.perf_counter() - t0 > time_limit_s:
                break
        if clock.on and self.comm.rank == 0 and res.iterations:
            print("phase ms/round: solve_enq %.3f finish %.3f pack %.3f "
                  "eval %.3f flush %.3f" % tuple(
                      t / res.iterations * 1e3 for t in clock.t.values()))
        if res.trace:
            res.final_cost, res.final_gradnorm = res.trace[-1]
        if fout:
            fout.close()
        res.elapsed_s = time.perf_counter() - t0
        backend.finish()
        return res

    def snapshot_initial_state(self) -> None:
        """Record every local agent's current iterate so repeated
        benchmark episodes can re-run the identical solve-to-target
        problem (bench.py). Call once after construction."""
        self._X0 = {rb: a.X.detach().clone()
                    for rb, a in self.local_agents.items()}

    def restore_initial_state(self) -> None:
        """Reset iterates (and Nesterov state) to the snapshot; the next
        run() starts from the same cold optimization state. Packed-path
        buffers are updated in place, so cached hipGraphs stay valid."""
        for rb, a in self.local_agents.items():
            a.X.copy_(self._X0[rb])
            if a.params.acceleration and a.Y is not None:
                a.Y.copy_(a.X)
                a.V.copy_(a.X)
                a.gamma = 0.0
                a.alpha = 0.0
            a.iteration_number = 0
        self._round_counter = 0

    def gather_final_trajectory(self, device: bool = False):
        """Rounded global trajectory (d, (d+1) n) on rank 0 (reference
        PartitionInitial.cpp:329-335 output). Returns None on other
        ranks. `device=True` rounds every agent on its own device
        (`dpo_amd.rounding.round_anchor`) and scatters with one
        index_copy_ per agent; the default host path is unchanged."""
        if device:
            return self._gather_final_trajectory_device()
        self._sync_anchor()
        dh = self.dh
        buf = torch.zeros(self.n_global, self.d, dh, dtype=torch.float64)
        for rb, a in self.local_agents.items():
            T = a.get_trajectory_in_global_frame()
            if T is None:
                continue
            Tb = T.reshape(self.d, a.n, dh).transpose(1, 0, 2)
            for i in range(a.n):
                buf[self.pose_to_index[(rb, i)]] = torch.from_numpy(
                    np.ascontiguousarray(Tb[i]))
        self.comm.all_reduce_sum_(buf.view(-1))
        if self.comm.rank != 0:
            return None
        return np.ascontiguousarray(
            buf.numpy().transpose(1, 0, 2).reshape(self.d,
                                                   self.n_global * dh))

    def _gather_final_trajectory_device(self):
        from .rounding import round_anchor
        self._sync_anchor()
        dh, d = self.dh, self.d
        dev = self._packed.dev if self._packed is not None else "cpu"
        buf = torch.zeros(self.n_global, dh, d, dtype=torch.float64,
                          device=dev)
        for rb, a in self.local_agents.items():
            if a.global_anchor is None or \
                    a.state != PGOAgentState.INITIALIZED:
                continue
            _, Xr = round_anchor(a.X, d, a.global_anchor)
            idx = torch.tensor([self.pose_to_index[(rb, i)]
                                for i in range(a.n)], dtype=torch.int64,
                               device=Xr.device)
            buf.index_copy_(0, idx.to(buf.device),
                            Xr.view(a.n, dh, d).to(buf.device))
        self.comm.all_reduce_sum_(buf.view(-1))
        if self.comm.rank != 0:
            return None
        return np.ascontiguousarray(
            buf.view(self.n_global * dh, d).T.cpu().numpy())

    def gather_lifted_iterate(self):
        """Global lifted iterate Xt (n_global (d+1), r) on rank 0, pose
        blocks in the `pose_to_index` order — the unrounded input of
        `dpo_amd.certify.certify_solution`. Returns None on other
        ranks."""
        dh = self.dh
        buf = torch.zeros(self.n_global, dh, self.r, dtype=torch.float64)
        for rb, a in self.local_agents.items():
            Xa = a.X.detach().cpu().view(a.n, dh, self.r)
            idx = torch.tensor([self.pose_to_index[(rb, i)]
                                for i in range(a.n)], dtype=torch.int64)
            buf.index_copy_(0, idx, Xa)
        self.comm.all_reduce_sum_(buf.view(-1))
        if self.comm.rank != 0:
            return None
        return buf.view(self.n_global * dh, self.r)

    def _sync_anchor(self):
        blk = self.dh * self.r
        dev = self._packed.dev if self._packed is not None else "cpu"
        buf = torch.zeros(blk, dtype=torch.float64, device=dev)
        if 0 in self.local_agents:
            a0 = self.local_agents[0]
            buf.copy_(a0.X.view(a0.n, self.dh, self.r)[0].reshape(-1))
        self.comm.all_reduce_sum_(buf)
        M = buf.cpu().numpy().reshape(self.dh, self.r).T
        for a in self.local_agents.values():
            a.set_global_anchor(np.ascontiguousarray(M))
