"""Batched agents (DPO_BATCH, docs/DESIGN.md section 5): one launch per
stage for a list of agents must compute, for every agent, what its
single-agent launch computes.

Per-kernel parity runs a batch of three agents with n = 7, 256 and 257
poses: the pose-per-thread kernels get 1, 1 and 2 blocks, the dense apply
(N = 28, 1024, 1028 rows for d = 3) a different extent for every agent,
and the first agent is finished inside the first block of every launch.
Whole rounds compare the driver with the batched path against
DPO_BATCH=0; the knob is read once per process, so those run in child
processes, each started once and shared by the tests below.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NS = (7, 256, 257)
SHAPES = [(3, 5), (2, 4)]
ST_RUN, ST_TCG_STOP = 0.0, 1.0
# control-block slots used below (enum CtrlSlot of dpo_ops.hip)
C_STATUS, C_ZR, C_EPE, C_EPD, C_DPD, C_COEF, C_BETA, C_ITER = \
    0, 4, 5, 6, 7, 8, 9, 10
C_RADIUS, C_HLEN, C_DOT0, C_TICKET, C_HIST, MAX_TCG = 12, 22, 24, 27, 32, 16
C_FX, C_DM, C_STOP_PENDING, C_DOT1, C_DOT2 = 1, 14, 18, 25, 26
F_SOLVE_OUT, F_EVAL_OUT = 1, 3
SENTINEL = -7.25
PADDED = ("X", "eta", "delta", "delta1", "rvec", "z", "Hd", "step", "Xprop",
          "grad", "eta_snap", "delta_snap", "ctrl", "G_buf", "eval3",
          "ctrl_host")


class BatchDesc(ctypes.Structure):
    """Mirror of struct BatchDesc (dpo_ops.hip); the size is asserted."""
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "q_rp", "q_ci", "q_vals", "Minv", "g_E0", "g_local_pose",
        "g_nbr_slot", "g_w", "X", "nbr", "Gt", "G_buf", "grad", "eta",
        "delta", "delta1", "rvec", "z", "Hd", "step", "Xprop", "eta_snap",
        "delta_snap", "ctrl", "prezero_z", "ctrl_host_dev", "eval3",
        "fences")] + [("total", ctypes.c_long), ("gtotal", ctypes.c_long)] \
        + [(k, ctypes.c_int) for k in (
            "n", "N", "g_ne", "nb_pose", "nb_upd", "nb_dense", "jsplit",
            "nb_gasm", "nb_zero", "nb_zero2", "nb_copy")]


def _lib():
    from dpo_amd.ops import hip_backend
    return hip_backend._lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _agent(n, d, r, seed):
    """Random buffers of one agent, padded: every vector has 64 spare
    elements behind its own extent, filled with the sentinel."""
    g = torch.Generator().manual_seed(seed)
    dh = d + 1
    total = n * dh * r
    N = n * dh

    def vec(scale=1.0, rows=1):
        v = torch.full((rows * total + 64,), SENTINEL, dtype=torch.float64)
        v[:rows * total] = scale * torch.randn(rows * total,
                                               dtype=torch.float64,
                                               generator=g)
        return v.to(DEV)

    # chain graph: pose i couples to i-1, i, i+1
    rp, ci = [0], []
    for i in range(n):
        ci += [j for j in (i - 1, i, i + 1) if 0 <= j < n]
        rp.append(len(ci))
    a = {"n": n, "N": N, "total": total,
         "rp": torch.tensor(rp, dtype=torch.int32, device=DEV),
         "ci": torch.tensor(ci, dtype=torch.int32, device=DEV),
         "vals": torch.randn(len(ci) * dh * dh, dtype=torch.float64,
                             generator=g).to(DEV),
         "Minv": torch.randn(N * N, dtype=torch.float32,
                             generator=g).to(DEV)}
    for k in ("X", "eta", "delta", "delta1", "rvec", "z", "Hd", "step",
              "Xprop", "grad"):
        a[k] = vec()
    a["eta_snap"] = vec(rows=2)
    a["delta_snap"] = vec(rows=2)
    # behind the control block: a spare one and 64 more slots of sentinel
    cs = _lib().dpo_ctrl_size()
    for k in ("ctrl", "ctrl_host"):
        ctrl = torch.zeros(2 * cs + 64, dtype=torch.float64)
        ctrl[cs:] = SENTINEL
        a[k] = ctrl.to(DEV)
    # linear term: ne shared edges into random local poses
    ne, nslots = 2 * n + 3, 5
    a["ne"] = ne
    a["G_buf"] = vec()
    a["E0"] = torch.randn(ne * dh * dh, dtype=torch.float64,
                          generator=g).to(DEV)
    a["local_pose"] = torch.randint(0, n, (ne,), generator=g).to(DEV)
    a["nbr_slot"] = torch.randint(0, nslots, (ne,), generator=g).to(DEV)
    a["nbr"] = torch.randn(nslots * dh * r, dtype=torch.float64,
                           generator=g).to(DEV)
    a["w"] = torch.rand(ne, dtype=torch.float64, generator=g).to(DEV)
    ev = torch.full((3 + 64,), SENTINEL, dtype=torch.float64)
    a["eval3"] = ev.to(DEV)
    a["fences"] = torch.zeros(4, dtype=torch.int32, device=DEV)
    return a


def _clone(a):
    return {k: (v.clone() if torch.is_tensor(v) else v)
            for k, v in a.items()}


def _descs(agents):
    assert _lib().dpo_batch_desc_size() == ctypes.sizeof(BatchDesc)
    arr = (BatchDesc * len(agents))()
    for b, a in zip(arr, agents):
        b.q_rp, b.q_ci, b.q_vals = (a["rp"].data_ptr(), a["ci"].data_ptr(),
                                    a["vals"].data_ptr())
        b.Minv = a["Minv"].data_ptr()
        for k in ("X", "grad", "eta", "delta", "delta1", "rvec", "z", "Hd",
                  "step", "Xprop", "eta_snap", "delta_snap", "ctrl"):
            setattr(b, k, a[k].data_ptr())
        b.prezero_z = a["z"].data_ptr()
        b.g_E0, b.g_local_pose = a["E0"].data_ptr(), a["local_pose"].data_ptr()
        b.g_nbr_slot, b.g_w = a["nbr_slot"].data_ptr(), a["w"].data_ptr()
        b.nbr = a["nbr"].data_ptr()
        b.G_buf = b.Gt = a["G_buf"].data_ptr()
        b.ctrl_host_dev = a["ctrl_host"].data_ptr()
        b.eval3 = a["eval3"].data_ptr()
        b.fences = a["fences"].data_ptr()
        b.total = b.gtotal = a["total"]
        b.n, b.N, b.g_ne = a["n"], a["N"], a["ne"]
    return arr


def _batch_op(op, agents, d, r, a=0.0, b=0.0):
    arr = _descs(agents)
    rc = _lib().dpo_batch_op(op, ctypes.cast(arr, ctypes.c_void_p),
                             len(agents), d, r, a, b, None)
    assert rc == 0
    torch.cuda.synchronize()


def _maxdiff(x, y):
    return float((x - y).abs().max())


def _check(single1, single2, batched, keys, exact_keys, n,
           one_block=(7, 256)):
    """exact_keys bit-identical; keys within ten times the single-agent
    launch's own run-to-run difference (floor 1e-12 relative). one_block:
    the agent sizes at which one block alone adds to the kernel's dots."""
    for k in exact_keys:
        assert torch.equal(single1[k], batched[k]), (n, k)
    for k in keys:
        scale = max(1.0, float(single1[k][single1[k] != SENTINEL]
                                .abs().max()))
        bound = max(10.0 * _maxdiff(single1[k], single2[k]), 1e-12 * scale)
        diff = _maxdiff(single1[k], batched[k])
        print("n", n, k, "single-vs-single", _maxdiff(single1[k],
                                                      single2[k]),
              "batched-vs-single", diff, "bound", bound)
        if n in one_block and k == "ctrl":
            # one block contributes to the dot: bit-identical
            assert torch.equal(single1[k], batched[k]), (n, k)
        assert diff <= bound, (n, k, diff, bound)
    # every ticket is back at zero, nothing behind the extents touched
    assert float(batched["ctrl"][C_TICKET]) == 0.0
    for k in PADDED:
        assert bool((batched[k][-64:] == SENTINEL).all()), (n, k)


def _setup_hd(a):
    c = a["ctrl"]
    c[C_STATUS], c[C_ITER], c[C_BETA] = ST_RUN, 0.0, 0.5
    c[C_ZR], c[C_DPD], c[C_RADIUS] = 1.0, 1.0, 1e3


@pytest.mark.parametrize("d,r", SHAPES)
def test_hd_stage_parity(d, r):
    lib = _lib()
    base = [_agent(n, d, r, 10 + i) for i, n in enumerate(NS)]
    for a in base:
        _setup_hd(a)
    singles = []
    for _ in range(2):
        run = [_clone(a) for a in base]
        for a in run:
            lib.dpo_hd_stage(_p(a["rp"]), _p(a["ci"]), _p(a["vals"]),
                             _p(a["delta"]), _p(a["delta1"]), _p(a["z"]),
                             _p(a["X"]), _p(a["Hd"]), _p(a["ctrl"]), a["n"],
                             d, r, 1, None)
        torch.cuda.synchronize()
        singles.append(run)
    bat = [_clone(a) for a in base]
    _batch_op(4, bat, d, r)
    for s1, s2, b in zip(singles[0], singles[1], bat):
        _check(s1, s2, b, ["ctrl"], ["Hd", "delta", "delta1", "z"], b["n"])


@pytest.mark.parametrize("d,r", SHAPES)
def test_candidate_parity(d, r):
    lib = _lib()
    base = [_agent(n, d, r, 20 + i) for i, n in enumerate(NS)]
    for a in base:
        c = a["ctrl"]
        c[C_STATUS], c[C_RADIUS], c[C_HLEN] = ST_TCG_STOP, 0.5, 1.0
        # one history entry that truncates at this radius
        c[C_HIST + 0] = 1.0                # z_r
        c[C_HIST + MAX_TCG] = 2.0          # d_Hd
        c[C_HIST + 2 * MAX_TCG] = 0.0      # e_Pe
        c[C_HIST + 3 * MAX_TCG] = 0.0      # e_Pd
        c[C_HIST + 4 * MAX_TCG] = 1.0      # d_Pd
        a["eta"].mul_(0.01), a["eta_snap"].mul_(0.01)
        a["delta_snap"].mul_(0.01)
        for k in ("eta", "eta_snap", "delta_snap"):
            a[k][-64:] = SENTINEL
    single = [_clone(a) for a in base]
    for a in single:
        lib.dpo_candidate(_p(a["ctrl"]), _p(a["step"]), _p(a["eta"]),
                          _p(a["eta_snap"]), _p(a["delta_snap"]), _p(a["X"]),
                          _p(a["Xprop"]), a["n"], d, r, None)
    torch.cuda.synchronize()
    bat = [_clone(a) for a in base]
    _batch_op(12, bat, d, r)
    for s, b in zip(single, bat):
        _check(s, s, b, [], ["step", "Xprop", "ctrl"], b["n"])


@pytest.mark.parametrize("d,r", SHAPES)
def test_precond_dense_parity(d, r):
    lib = _lib()
    base = [_agent(n, d, r, 30 + i) for i, n in enumerate(NS)]
    for a in base:
        a["ctrl"][C_STATUS] = ST_RUN
        a["z"][:a["total"]] = 0.0   # the stage in front cleared it
    singles = []
    for _ in range(2):
        run = [_clone(a) for a in base]
        for a in run:
            lib.dpo_precond_dense(_p(a["Minv"]), _p(a["rvec"]), _p(a["z"]),
                                  a["N"], r, _p(a["ctrl"]), 0, None)
        torch.cuda.synchronize()
        singles.append(run)
    bat = [_clone(a) for a in base]
    _batch_op(8, bat, d, r)
    for s1, s2, b in zip(singles[0], singles[1], bat):
        # z accumulates the j-split partial sums atomically
        _check(s1, s2, b, ["z"], ["rvec", "ctrl"], b["n"])


def _runs(base, single_fn, op, d, r, a=0.0, b=0.0):
    """Two rounds of single-agent launches and one batched launch, each
    on its own copy of base."""
    singles = []
    for _ in range(2):
        run = [_clone(x) for x in base]
        for x in run:
            single_fn(x)
        torch.cuda.synchronize()
        singles.append(run)
    bat = [_clone(x) for x in base]
    _batch_op(op, bat, d, r, a, b)
    return singles[0], singles[1], bat


@pytest.mark.parametrize("d,r", SHAPES)
def test_zero_and_assemble_parity(d, r):
    lib = _lib()
    cs = lib.dpo_ctrl_size()
    base = [_agent(n, d, r, 50 + i) for i, n in enumerate(NS)]
    for x in base:
        x["ctrl"][:cs] = 3.0
    # kb_dzero: G_buf cleared over its own extent, nothing else
    bat = [_clone(x) for x in base]
    _batch_op(0, bat, d, r)
    for x, b in zip(base, bat):
        assert bool((b["G_buf"][:b["total"]] == 0).all())
        for k in PADDED:
            assert bool((b[k][-64:] == SENTINEL).all()), (b["n"], k)
            if k != "G_buf":
                assert torch.equal(x[k], b[k]), (b["n"], k)
    # kb_dzero2: G_buf and the control block, not the spare block behind
    bat = [_clone(x) for x in base]
    _batch_op(1, bat, d, r)
    for x, b in zip(base, bat):
        assert bool((b["G_buf"][:b["total"]] == 0).all())
        assert bool((b["ctrl"][:cs] == 0).all())
        assert bool((b["ctrl"][cs:] == SENTINEL).all())
        for k in PADDED:
            assert bool((b[k][-64:] == SENTINEL).all()), (b["n"], k)
            if k not in ("G_buf", "ctrl"):
                assert torch.equal(x[k], b[k]), (b["n"], k)
    # kb_g_assemble against dpo_g_assemble (which clears first)
    for x in base:
        x["G_buf"][:x["total"]] = 0.0
        x["ctrl"][:cs] = 0.0

    def single(x):
        lib.dpo_g_assemble(_p(x["G_buf"]), _p(x["E0"]), _p(x["local_pose"]),
                           _p(x["nbr_slot"]), _p(x["nbr"]), _p(x["w"]),
                           x["ne"], d + 1, r, x["N"], None)
    s1, s2, bat = _runs(base, single, 2, d, r)
    for a1, a2, b in zip(s1, s2, bat):
        # several edges add into one pose atomically
        _check(a1, a2, b, ["G_buf"], ["ctrl", "X"], b["n"])


def _hess_tail(x, d, r, kind, a=0.0, b=0.0):
    V = x["Xprop"] if kind == 2 else x["X"]
    _lib().dpo_hess_tail(_p(x["rp"]), _p(x["ci"]), _p(x["vals"]), _p(V),
                         _p(x["G_buf"]), _p(x["grad"]), _p(x["rvec"]),
                         _p(x["ctrl"]), x["n"], d, r, kind, 1, a, b,
                         _p(x["eval3"]), None)


@pytest.mark.parametrize("d,r", SHAPES)
def test_gradient_init_parity(d, r):
    base = [_agent(n, d, r, 60 + i) for i, n in enumerate(NS)]
    s1, s2, bat = _runs(base, lambda x: _hess_tail(x, d, r, 1, 1e-2, 100.0),
                        3, d, r, 1e-2, 100.0)
    for a1, a2, b in zip(s1, s2, bat):
        # the batched launch also clears z for the dense apply behind it
        assert bool((b["z"][:b["total"]] == 0).all())
        b["z"][:b["total"]] = a1["z"][:b["total"]]
        _check(a1, a2, b, ["ctrl"], ["grad", "rvec", "G_buf", "X"], b["n"])


@pytest.mark.parametrize("d,r", SHAPES)
def test_candidate_eval_parity(d, r):
    cs = _lib().dpo_ctrl_size()
    base = [_agent(n, d, r, 70 + i) for i, n in enumerate(NS)]
    for x in base:
        c = x["ctrl"]
        c[C_STATUS], c[C_FX], c[C_DM] = ST_TCG_STOP, 5.0, 1.0
    # CF_ACCEPT
    s1, s2, bat = _runs(base, lambda x: _hess_tail(x, d, r, 2, 0.1), 6, d, r,
                        0.1)
    for a1, a2, b in zip(s1, s2, bat):
        _check(a1, a2, b, ["ctrl"], ["Xprop", "G_buf", "ctrl_host"], b["n"])
        assert int(b["fences"].abs().sum()) == 0
    # CF_ACCEPT_OUT: the same control block, published to the agent's own
    # host copy, and its own F_SOLVE_OUT released
    _, _, out = _runs(base, lambda x: None, 5, d, r, 0.1)
    for a1, a2, b in zip(s1, s2, out):
        _check(a1, a2, b, ["ctrl"], ["Xprop", "G_buf"], b["n"])
        assert torch.equal(b["ctrl_host"][:cs], b["ctrl"][:cs])
        assert bool((b["ctrl_host"][cs:] == SENTINEL).all())
        want = [0, 0, 0, 0]
        want[F_SOLVE_OUT] = 1
        assert b["fences"].tolist() == want


@pytest.mark.parametrize("d,r", SHAPES)
def test_evaluation_parity(d, r):
    base = [_agent(n, d, r, 80 + i) for i, n in enumerate(NS)]
    s1, s2, bat = _runs(base, lambda x: _hess_tail(x, d, r, 3), 7, d, r)
    for a1, a2, b in zip(s1, s2, bat):
        _check(a1, a2, b, ["ctrl", "eval3"], ["grad", "G_buf", "X"], b["n"])
        if b["n"] in (7, 256):
            assert torch.equal(a1["eval3"], b["eval3"])
        want = [0, 0, 0, 0]
        want[F_EVAL_OUT] = 1
        assert b["fences"].tolist() == want
        assert a1["fences"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("tail", ["z0", "beta"])
@pytest.mark.parametrize("d,r", SHAPES)
def test_proj_dots_parity(d, r, tail):
    """kb_proj_dots with its fused tail against k_proj_dots followed by
    the tail's standalone launch (what DPO_NO_CF=1 runs)."""
    lib = _lib()
    base = [_agent(n, d, r, 90 + i) for i, n in enumerate(NS)]
    for x in base:
        c = x["ctrl"]
        c[C_STATUS], c[C_ZR], c[C_COEF], c[C_ITER] = ST_RUN, 2.0, 0.5, 1.0
        c[C_EPD], c[C_DPD] = 0.25, 1.5

    def single(x):
        lib.dpo_proj_dots(_p(x["X"]), _p(x["z"]), None, _p(x["z"]),
                          _p(x["rvec"]), _p(x["ctrl"]), x["n"], d, r, C_DOT0,
                          -1, 0, 0, None)
        (lib.dpo_ctrl_z0 if tail == "z0" else lib.dpo_ctrl_beta)(
            _p(x["ctrl"]), None)
    s1, s2, bat = _runs(base, single, 9 if tail == "z0" else 10, d, r)
    for a1, a2, b in zip(s1, s2, bat):
        _check(a1, a2, b, ["ctrl"], ["z", "rvec", "X"], b["n"])


@pytest.mark.parametrize("d,r", SHAPES)
def test_tcg_update_parity(d, r):
    """kb_tcg_update + CF_RR in iteration 1, whose direction lives in the
    second buffer, against k_tcg_update on that buffer + the standalone
    tail. total / 1024 blocks: a different extent for every agent."""
    lib = _lib()
    base = [_agent(n, d, r, 100 + i) for i, n in enumerate(NS)]
    for x in base:
        c = x["ctrl"]
        c[C_STATUS], c[C_ITER], c[C_COEF] = ST_RUN, 1.0, 0.75
        c[C_STOP_PENDING] = 0.0

    def single(x):
        lib.dpo_tcg_update(_p(x["eta"]), _p(x["rvec"]), _p(x["delta1"]),
                           _p(x["Hd"]), _p(x["eta_snap"]),
                           _p(x["delta_snap"]), _p(x["ctrl"]), x["total"],
                           None)
        lib.dpo_ctrl_rr(_p(x["ctrl"]), None)
    s1, s2, bat = _runs(base, single, 11, d, r)
    for a1, a2, b in zip(s1, s2, bat):
        # the batched launch also clears z for the dense apply behind it
        assert bool((b["z"][:b["total"]] == 0).all())
        b["z"][:b["total"]] = a1["z"][:b["total"]]
        _check(a1, a2, b, ["ctrl"],
               ["eta", "rvec", "eta_snap", "delta_snap", "delta", "delta1",
                "Hd"], b["n"], one_block=(7,))


def test_tcg_end_and_commit():
    d, r = 3, 5
    lib = _lib()
    base = [_agent(n, d, r, 110 + i) for i, n in enumerate(NS)]
    for x in base:
        x["ctrl"][C_ITER] = 4.0
    base[1]["ctrl"][C_STATUS] = 2.0   # accepted: the cap leaves it alone
    s1, s2, bat = _runs(base, lambda x: lib.dpo_ctrl_tcg_end(_p(x["ctrl"]),
                                                             None), 13, d, r)
    for a1, a2, b in zip(s1, s2, bat):
        _check(a1, a2, b, [], list(PADDED), b["n"])
    assert float(bat[0]["ctrl"][C_STATUS]) == ST_TCG_STOP
    assert float(bat[1]["ctrl"][C_STATUS]) == 2.0
    # kb_commit: X <- Xprop for members 0 and 2 only
    bat = [_clone(x) for x in base]
    _batch_op(14, bat, d, r, a=5.0)
    for i, (x, b) in enumerate(zip(base, bat)):
        want = x["Xprop"] if i != 1 else x["X"]
        assert torch.equal(b["X"][:b["total"]], want[:b["total"]]), i
        for k in PADDED:
            assert bool((b[k][-64:] == SENTINEL).all()), (i, k)
            if k != "X":
                assert torch.equal(x[k], b[k]), (i, k)


def test_guard_per_agent():
    """A member at ST_TCG_STOP is a no-op inside an ST_RUN-guarded
    launch; the others match their single launches."""
    d, r = 3, 5
    lib = _lib()
    base = [_agent(n, d, r, 40 + i) for i, n in enumerate(NS)]
    for a in base:
        _setup_hd(a)
    base[1]["ctrl"][C_STATUS] = ST_TCG_STOP
    single = [_clone(a) for a in base]
    for a in (single[0], single[2]):
        lib.dpo_hd_stage(_p(a["rp"]), _p(a["ci"]), _p(a["vals"]),
                         _p(a["delta"]), _p(a["delta1"]), _p(a["z"]),
                         _p(a["X"]), _p(a["Hd"]), _p(a["ctrl"]), a["n"], d, r,
                         1, None)
    torch.cuda.synchronize()
    bat = [_clone(a) for a in base]
    _batch_op(4, bat, d, r)
    for k, v in base[1].items():
        if torch.is_tensor(v):
            assert torch.equal(v, bat[1][k]), k
    for k in ("Hd", "delta", "delta1", "ctrl"):
        assert torch.equal(single[0][k], bat[0][k]), k
    # two blocks add into the third agent's dot: measured bound for ctrl
    again = _clone(base[2])
    lib.dpo_hd_stage(_p(again["rp"]), _p(again["ci"]), _p(again["vals"]),
                     _p(again["delta"]), _p(again["delta1"]), _p(again["z"]),
                     _p(again["X"]), _p(again["Hd"]), _p(again["ctrl"]),
                     again["n"], d, r, 1, None)
    torch.cuda.synchronize()
    _check(single[2], again, bat[2], ["ctrl"], ["Hd", "delta", "delta1"],
           NS[2])


# ---------------------------------------------------------------------
# whole rounds in child processes
# ---------------------------------------------------------------------
_CHILD = """
import json, sys
import torch
from dpo_amd.comm import Comm
from dpo_amd.dist_driver import DistributedRBCDDriver
from dpo_amd.synthetic import grid3d

def run(sizes, selection, inner_tol, iters, seed=3):
    meas, n = grid3d(side=8, seed=seed)
    part = []
    for rb, sz in enumerate(sizes):
        part += [rb] * sz
    assert len(part) == n
    drv = DistributedRBCDDriver(meas, n, len(sizes), Comm(), r=5,
        partition=part, selection=selection, device='cuda:0',
        inner_tol=inner_tol)
    res = drv.run(max_iters=iters, gradnorm_tol=0.0)
    torch.cuda.synchronize()
    ags = [drv.local_agents[k] for k in sorted(drv.local_agents)]
    ctrl = [a._dev_solver.ctrl_block() for a in ags]
    cnt = [a._dev_solver.counters() for a in ags]
    grp = drv._packed.group.counters() if drv._packed.group else {}
    return {'iters': res.iterations, 'trace': [list(map(float, t))
                                               for t in res.trace],
            'X': [a.X.cpu().flatten().tolist() for a in ags],
            'status': [c[0] for c in ctrl], 'hlen': [c[22] for c in ctrl],
            'rho': [c[21] for c in ctrl],
            'dense': [getattr(a.problem, '_Minv', None) is not None for a in ags],
            'solves': [c['solves'] for c in cnt],
            'conts': [c['continuations'] for c in cnt],
            'hist': [c['hlen_hist'] for c in cnt], 'group': grp}

def make(sizes=(40, 100, 150, 222), seed=3):
    meas, n = grid3d(side=8, seed=seed)
    part = []
    for rb, sz in enumerate(sizes):
        part += [rb] * sz
    drv = DistributedRBCDDriver(meas, n, len(sizes), Comm(), r=5,
        partition=part, selection='colored', device='cuda:0')
    drv.run(max_iters=2, gradnorm_tol=0.0)
    torch.cuda.synchronize()
    return drv

def agents(drv):
    return [drv.local_agents[k] for k in sorted(drv.local_agents)]

def members(drv, color):
    return [rb for rb in sorted(drv._packed.agents)
            if drv._colors[rb] == color]

def manual_round(drv, color, accept_rho=0.1, max_shrink=10):
    # one round by hand: the colour's solves, exchange, evaluation
    pk = drv._packed
    g = pk.group
    ids = g.ids([pk.group_lidx[rb] for rb in members(drv, color)])
    g.solve_start(ids, tol=1e-2, Delta0=100.0, accept_rho=accept_rho)
    g.solve_finish(ids, max_shrink)
    pk._exchange()
    row = torch.zeros(drv.num_robots, 3, dtype=torch.float64,
                      device='cuda:0')
    g.eval_all(row)
    torch.cuda.synchronize()
    return row.cpu().flatten().tolist()

def snap(drv, row):
    ags = agents(drv)
    ctrl = [a._dev_solver.ctrl_block() for a in ags]
    return {'X': [a.X.cpu().flatten().tolist() for a in ags], 'row': row,
            'status': [c[0] for c in ctrl], 'hlen': [c[22] for c in ctrl],
            'rho': [c[21] for c in ctrl], 'shrinks': [c[23] for c in ctrl],
            'group': drv._packed.group.counters()}

def restore(drv, X0):
    for a, x in zip(agents(drv), X0):
        a.X.copy_(x)
    drv._packed._exchange()
    torch.cuda.synchronize()

def manual_cases():
    res = {}
    drv = make()
    X0 = [a.X.clone() for a in agents(drv)]
    # rejected first candidates: the construction of the shrink tests
    # (accept_rho = 2 rejects every candidate), then a threshold between
    # the two members' own rho, so that one accepts at once and the other
    # shrinks first
    res['reject_all'] = snap(drv, manual_round(drv, 0, 2.0, 2))
    res['reject_all']['members'] = members(drv, 0)
    restore(drv, X0)
    probe = snap(drv, manual_round(drv, 0))
    rho = [probe['rho'][rb] for rb in members(drv, 0)]
    thr = round(0.5 * (rho[0] + rho[1]), 4) if abs(rho[0] - rho[1]) > 1e-3 \
        else 2.0
    restore(drv, X0)
    res['reject_mix'] = snap(drv, manual_round(drv, 0, thr, 3))
    res['reject_mix']['thr'] = thr
    res['reject_mix']['probe_rho'] = rho
    restore(drv, X0)
    # descriptor refresh: new buffers for one member's G structure and Q
    # values; the old ones are cleared, so a stale descriptor would show
    a = drv.local_agents[members(drv, 0)[0]]
    s = a._dev_solver
    E0, lp, ns, w = s._grefs
    E0n, wn = E0.clone(), w.clone()
    s.set_gdata(E0n, lp, ns, wn)
    E0.zero_(); w.zero_()
    Q = a.problem.Q
    old = Q.vals
    Q.vals = old.clone()
    Q.invalidate()
    s.bind_problem_static(a.problem)
    old.zero_()
    torch.cuda.synchronize()
    before = drv._packed.group.counters()
    res['refresh'] = snap(drv, manual_round(drv, 0))
    res['refresh']['before'] = before
    # re-binding the same buffers (what a re-weighting in place does)
    before = drv._packed.group.counters()
    s.set_gdata(E0n, lp, ns, wn)
    s.bind_problem_static(a.problem)
    res['inplace'] = snap(drv, manual_round(drv, 0))
    res['inplace']['before'] = before
    # a preconditioner refresh allocates a new Minv of the same size: new
    # descriptors, the same graphs
    before = drv._packed.group.counters()
    keep = a.problem._Minv
    a.problem.refresh_preconditioner()
    s.bind_problem_static(a.problem)
    res['minv'] = snap(drv, manual_round(drv, 0))
    res['minv']['before'] = before
    res['minv']['moved'] = keep.data_ptr() != a.problem._Minv.data_ptr()
    # one block-Jacobi member: its list and the evaluation of all agents
    # take the per-agent path
    j = drv.local_agents[members(drv, 1)[0]]
    j.problem.precond_mode = 'jacobi'
    j.problem._Minv = None
    j.problem.set_q(j.problem.Q)
    j._dev_solver.bind_problem_static(j.problem)
    before = drv._packed.group.counters()
    row = manual_round(drv, 1)
    res['jacobi'] = snap(drv, manual_round(drv, 0))
    res['jacobi']['row1'] = row
    res['jacobi']['before'] = before
    return res

out = {}
if sys.argv[1] == 'seg':
    out['tol0'] = run([40, 100, 150, 222], 'colored', 0.0, 6, seed=5)
    # a rejection inside a continued list: after three rounds of this
    # fixture the next solve of colour 1 has one member still running
    # behind the one-iteration primary graph, while the other has stopped
    # and (accept_rho = 2) had its first candidate rejected
    drv = make(seed=5)
    manual_round(drv, 0)
    cnt0 = [a._dev_solver.counters()['continuations'] for a in agents(drv)]
    before = drv._packed.group.counters()
    out['reject_cont'] = snap(drv, manual_round(drv, 1, 2.0, 2))
    out['reject_cont']['before'] = before
    out['reject_cont']['members'] = members(drv, 1)
    out['reject_cont']['conts'] = [
        a._dev_solver.counters()['continuations'] - c
        for a, c in zip(agents(drv), cnt0)]
else:
    out['default'] = run([40, 100, 150, 222], 'colored', 1e-2, 6)
    out['greedy'] = run([40, 100, 150, 222], 'greedy', 1e-2, 4)
    out['manual'] = manual_cases()
print(json.dumps(out))
"""

_children = {}


def _child(tag, batch, seg=False):
    """Child output; tag tells repeated per-agent runs apart. seg: the
    inner_tol = 0 case, run with DPO_TCG_SEG=1 (on this fixture tCG stops
    after one or two iterations, so a primary graph of one iteration
    makes the two-iteration solves continue). Its seed 5 was chosen on
    the per-agent path: rounds 1 and 3 each have one member of the active
    pair continuing while the other has stopped (with seed 3 both members
    continue in the same round)."""
    key = (tag, batch, seg)
    if key not in _children:
        env = dict(os.environ)
        env.pop("DPO_BATCH", None)
        env.pop("DPO_TCG_SEG", None)
        if not batch:
            env["DPO_BATCH"] = "0"
        if seg:
            env["DPO_TCG_SEG"] = "1"
        p = subprocess.run([sys.executable, "-c", _CHILD,
                            "seg" if seg else "main"],
                           capture_output=True, text=True, env=env, cwd=HERE,
                           timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        _children[key] = json.loads(p.stdout.strip().splitlines()[-1])
    return _children[key]


def _flat(run):
    out = {"trace": torch.tensor(run["trace"], dtype=torch.float64).flatten(),
           "rho": torch.tensor(run["rho"], dtype=torch.float64)}
    for i, x in enumerate(run["X"]):
        out[f"X{i}"] = torch.tensor(x, dtype=torch.float64)
    return out


@pytest.mark.parametrize("case", ["default", "tol0"])
def test_rounds_match_per_agent_path(case):
    seg = case == "tol0"
    ref1 = _child("a", False, seg)[case]
    ref2 = _child("b", False, seg)[case]
    got = _child("a", True, seg)[case]
    print(case, "group counters", got["group"], "per-agent", ref1["group"])
    print(case, "hlen", got["hlen"], "conts", got["conts"], "hist",
          got["hist"])
    assert all(got["dense"])
    # the paths are what they should be
    assert ref1["group"]["batched_solves"] == 0
    assert ref1["group"]["batched_evals"] == 0
    assert got["group"]["batched_solves"] > 0
    assert got["group"]["batched_solves"] + got["group"]["agent_solves"] == 6
    assert got["group"]["batched_evals"] > 0
    assert got["group"]["agent_evals"] == 0
    assert got["iters"] == ref1["iters"] == 6
    assert got["status"] == ref1["status"]
    assert got["hlen"] == ref1["hlen"]
    assert got["solves"] == ref1["solves"]
    assert got["conts"] == ref1["conts"]
    assert got["hist"] == ref1["hist"]
    if case == "tol0":
        # a continuation ran for a list in which another member had
        # already stopped inside the primary graph
        assert sum(ref1["conts"]) > 0
        assert got["group"]["batched_conts"] > 0
        # lists have two members: fewer continuing members than two per
        # continued list means one of a list had stopped
        assert sum(got["conts"]) < 2 * got["group"]["batched_conts"]
    a, b, g = _flat(ref1), _flat(ref2), _flat(got)
    for k in a:
        scale = max(1.0, float(a[k].abs().max()))
        bound = max(10.0 * _maxdiff(a[k], b[k]), 1e-12 * scale)
        diff = _maxdiff(a[k], g[k])
        print(case, k, "per-agent run-to-run", _maxdiff(a[k], b[k]),
              "batched-vs-per-agent", diff, "bound", bound)
        assert diff <= bound, (case, k, diff, bound)


def test_single_active_agent_takes_per_agent_path():
    ref = _child("a", False)["greedy"]
    ref2 = _child("b", False)["greedy"]
    got = _child("a", True)["greedy"]
    print("greedy group counters", got["group"])
    assert got["group"]["batched_solves"] == 0
    assert got["group"]["batched_evals"] == 0
    assert got["status"] == ref["status"] and got["hlen"] == ref["hlen"]
    a, b, g = _flat(ref), _flat(ref2), _flat(got)
    for k in a:
        scale = max(1.0, float(a[k].abs().max()))
        bound = max(10.0 * _maxdiff(a[k], b[k]), 1e-12 * scale)
        assert _maxdiff(a[k], g[k]) <= bound, (k, bound)


def _flat_manual(run):
    out = {"row": torch.tensor(run["row"], dtype=torch.float64),
           "rho": torch.tensor(run["rho"], dtype=torch.float64)}
    for i, x in enumerate(run["X"]):
        out[f"X{i}"] = torch.tensor(x, dtype=torch.float64)
    return out


def _rho_run_to_run():
    """The per-agent path's run-to-run difference of C_RHO, pooled over
    every case of the two per-agent children. rho = (f - f_prop) / dm
    cancels ten digits on this fixture, so its difference between two
    runs is either about 1e-8 or, when the dot atomics happened to arrive
    in the same order, about 1e-14; two runs of one case sample that at
    random, all cases together give the size of the noise. This departs
    from the letter of the rule (ten times the run-to-run difference of
    the case itself), for C_RHO of the hand-driven cases only: X, the
    evaluation rows, statuses, history lengths and shrink counts keep
    the per-case bound or exact equality."""
    a, b = _child("a", False), _child("b", False)
    pairs = [(a["default"], b["default"]), (a["greedy"], b["greedy"])]
    pairs += [(a["manual"][c], b["manual"][c]) for c in a["manual"]]
    return max(_maxdiff(torch.tensor(x["rho"], dtype=torch.float64),
                        torch.tensor(y["rho"], dtype=torch.float64))
               for x, y in pairs)


def _compare_manual(case, seg=False):
    """The batched child's state after a hand-driven round against the
    per-agent children's, with the measured bound."""
    pick = (lambda c: c[case]) if seg else (lambda c: c["manual"][case])
    ref1 = pick(_child("a", False, seg))
    ref2 = pick(_child("b", False, seg))
    got = pick(_child("a", True, seg))
    assert got["status"] == ref1["status"], case
    assert got["hlen"] == ref1["hlen"], case
    assert got["shrinks"] == ref1["shrinks"], case
    a, b, g = _flat_manual(ref1), _flat_manual(ref2), _flat_manual(got)
    for k in a:
        assert bool(torch.isfinite(g[k]).all()), (case, k)
        scale = max(1.0, float(a[k].abs().max()))
        noise = _rho_run_to_run() if k == "rho" else _maxdiff(a[k], b[k])
        bound = max(10.0 * noise, 1e-12 * scale)
        diff = _maxdiff(a[k], g[k])
        print(case, k, "per-agent run-to-run", _maxdiff(a[k], b[k]),
              "batched-vs-per-agent", diff, "bound", bound)
        assert diff <= bound, (case, k, diff, bound)
    return ref1, got


def _delta(run, key):
    return run["group"][key] - run["before"][key]


def test_rejected_first_candidate():
    ref, got = _compare_manual("reject_all")
    print("reject_all shrinks", ref["shrinks"], "status", ref["status"])
    # on the per-agent path first: every member of the list shrank
    assert len(ref["members"]) == 2
    assert all(ref["shrinks"][m] == 2 for m in ref["members"])
    ref, got = _compare_manual("reject_mix")
    print("reject_mix thr", ref["thr"], "probe rho", ref["probe_rho"],
          "shrinks", ref["shrinks"], "status", ref["status"])
    assert got["thr"] == ref["thr"]
    assert sum(ref["shrinks"]) > 0
    assert got["group"]["batched_solves"] > 0


def test_rejected_candidate_inside_continuation():
    """DPO_TCG_SEG=1: one member of the list needs the continuation, the
    other has stopped with its first candidate rejected and is re-run by
    the list's continuation before it shrinks."""
    ref, got = _compare_manual("reject_cont", seg=True)
    print("reject_cont members", ref["members"], "conts", ref["conts"],
          "shrinks", ref["shrinks"], "status", ref["status"], "group",
          got["before"], got["group"])
    # the mix, on the per-agent path first
    assert len(ref["members"]) == 2
    assert sum(ref["conts"][m] for m in ref["members"]) == 1
    assert all(ref["shrinks"][m] == 2 for m in ref["members"])
    assert got["conts"] == ref["conts"]
    assert _delta(got, "batched_solves") == 1
    assert _delta(got, "batched_conts") == 1


def test_descriptor_refresh():
    ref, got = _compare_manual("refresh")
    print("refresh", got["before"], got["group"])
    # the solve list and the evaluation rebuilt their descriptors
    assert _delta(got, "desc_builds") == 2
    assert _delta(got, "batched_solves") == 1
    assert _delta(got, "batched_evals") == 1
    ref, got = _compare_manual("inplace")
    print("inplace", got["before"], got["group"])
    assert _delta(got, "desc_builds") == 0
    assert _delta(got, "captures") == 0
    assert _delta(got, "batched_solves") == 1
    ref, got = _compare_manual("minv")
    print("minv", got["before"], got["group"], "moved", got["moved"])
    assert got["moved"]
    assert _delta(got, "desc_builds") == 2
    assert _delta(got, "captures") == 0
    assert _delta(got, "batched_solves") == 1


def test_jacobi_member_takes_per_agent_path():
    ref, got = _compare_manual("jacobi")
    print("jacobi", got["before"], got["group"])
    # two rounds: the list with the block-Jacobi member went per agent,
    # the all-dense list stayed batched, both evaluations went per agent
    assert _delta(got, "batched_solves") == 1
    assert _delta(got, "agent_solves") == 1
    assert _delta(got, "batched_evals") == 0
    assert _delta(got, "agent_evals") == 2
    r1 = torch.tensor(ref["row1"], dtype=torch.float64)
    g1 = torch.tensor(got["row1"], dtype=torch.float64)
    r2 = torch.tensor(_child("b", False)["manual"]["jacobi"]["row1"],
                      dtype=torch.float64)
    bound = max(10.0 * _maxdiff(r1, r2),
                1e-12 * max(1.0, float(r1.abs().max())))
    assert _maxdiff(r1, g1) <= bound
