"""Fused solve / evaluation stages against the unfused sequence.

The default solve runs its scalar steps (control init, acceptance test,
evaluation scalars, publishing the control block) in the last block of
the Hessian kernel in front of them, and the candidate selection, the
step and the retraction in one kernel; DPO_NO_CF=1 runs the same
`__device__` bodies as launches of their own. The stand-alone ops take
both routes in one process and are compared bit for bit: each fused
step performs the same operations in the same order, and with at most
two blocks the atomic partial sums commute. Whole solves take the knob
from the environment, which is read once per process, so each setting
runs in a child process that is started once and shared.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25e77
SHAPES = [(2, 2), (3, 5), (3, 8)]
N_POSE = (1, 65, 256, 257)


def _hb():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import hip_backend
    assert hip_backend.CTRL_SIZE == kr.CTRL_SIZE
    return hip_backend


def _dev(t):
    return t.contiguous().to(DEV)


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _history_ctrl(hlen, radius, status=kr.ST_TCG_STOP):
    """A stopped control block with a plausible Krylov history: positive
    curvature, |eta|^2 growing with j."""
    c = np.zeros(kr.CTRL_SIZE)
    c[kr.C_STATUS] = status
    c[kr.C_RADIUS] = radius
    c[kr.C_HLEN] = hlen
    c[kr.C_FX] = 10.0
    for j in range(kr.MAX_TCG):
        c[kr.H_ZR(j)] = 1.0 / (j + 1.0)
        c[kr.H_DHD(j)] = 2.0 + 0.37 * j
        c[kr.H_EPE(j)] = 0.11 * j * j
        c[kr.H_EPD(j)] = 0.07 * j
        c[kr.H_DPD(j)] = 1.3 + 0.21 * j
    # slots the candidate must overwrite or clear
    c[kr.C_DOT0], c[kr.C_DOT2] = 7.0, 8.0
    c[kr.C_JSTAR], c[kr.C_TAUSTAR], c[kr.C_USE_CURRENT] = 9.0, 0.3, 1.0
    return c


def _candidate_inputs(d, r, n, rows):
    g = kr.gen(41, d, r, n)
    total = (d + 1) * n * r
    X = kr.manifold_point(n, d, r, g)
    eta = 0.1 * kr.randn(g, total)
    es = 0.1 * kr.randn(g, rows * total)
    dsn = 0.1 * kr.randn(g, rows * total)
    return X, eta, es, dsn


def _run_candidate(hb, fused, c0, X, eta, es, dsn, d):
    ctrl = _dev(torch.from_numpy(c0.copy()))
    Xd, etad, esd, dsd = _dev(X), _dev(eta), _dev(es), _dev(dsn)
    step = torch.full_like(etad, SENTINEL)
    Xp = torch.full_like(Xd, SENTINEL)
    if fused:
        hb.candidate(ctrl, step, etad, esd, dsd, Xd, Xp, d)
    else:
        hb._lib.dpo_ctrl_candidate(hb._p(ctrl), _stream())
        hb.form_step(step, etad, esd, dsd, ctrl)
        r = X.shape[-1]
        n = X.numel() // ((d + 1) * r)
        hb._lib.dpo_polar_affine(hb._p(Xd), hb._p(step), hb._p(None), 1.0,
                                 1.0, 0.0, hb._p(Xp), n, d, r, hb._p(ctrl),
                                 hb.GUARD_STOP, _stream())
    torch.cuda.synchronize()
    return ctrl.cpu().numpy(), step.cpu(), Xp.cpu()


@pytest.mark.parametrize("d,r", SHAPES)
def test_candidate_matches_unfused(d, r):
    """k_candidate against dpo_ctrl_candidate + form_step + polar_affine:
    a truncated step (jstar = 3, where the history's |eta|^2 = 0.99
    first exceeds radius^2 = 0.81: snapshot rows), a full step (current
    eta), and a guard mismatch that must leave everything untouched."""
    hb = _hb()
    rows = 4
    for n in N_POSE:
        X, eta, es, dsn = _candidate_inputs(d, r, n, rows)
        for label, c0 in (("truncate", _history_ctrl(4, 0.9)),
                          ("full", _history_ctrl(3, 1e6))):
            a = _run_candidate(hb, True, c0, X, eta, es, dsn, d)
            b = _run_candidate(hb, False, c0, X, eta, es, dsn, d)
            tag = f"candidate d={d} r={r} n={n} {label}"
            assert b[0][kr.C_USE_CURRENT] == (label == "full"), tag
            if label == "truncate":
                assert b[0][kr.C_JSTAR] == 3.0, tag
            assert np.array_equal(a[0], b[0]), tag
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), tag
            assert not (a[2] == SENTINEL).any(), tag
        c0 = _history_ctrl(4, 0.9, status=kr.ST_RUN)
        got = _run_candidate(hb, True, c0, X, eta, es, dsn, d)
        assert np.array_equal(got[0], c0)
        assert (got[1] == SENTINEL).all() and (got[2] == SENTINEL).all()


def _run_hess_tail(hb, kind, fused, p, X, c0, a=0.0, b=0.0):
    Q = p.Q.to(DEV)
    Xd, G = _dev(X), _dev(p._g())
    ctrl = _dev(torch.from_numpy(c0.copy()))
    out = torch.full_like(Xd, SENTINEL)
    out2 = torch.full_like(Xd, SENTINEL)
    out3 = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    hb.hess_tail(Q, Xd, G, ctrl, p.d, kind, fused, a, b, out, out2, out3)
    torch.cuda.synchronize()
    return ctrl.cpu().numpy(), out.cpu(), out2.cpu(), out3.cpu()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(
        torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("d,r", SHAPES)
def test_hess_tails_match_unfused(d, r):
    """CF_INIT, CF_ACCEPT and CF_EVAL in the Hessian kernel's last block
    against the kernel followed by k_ctrl_init / k_ctrl_accept /
    k_eval_combine: outputs and every control slot bit-identical."""
    hb = _hb()
    for n in N_POSE:
        p, X = kr.small_problem(d, r, n, kr.gen(43, d, r, n), with_g=True)
        tag = f"d={d} r={r} n={n}"
        zero = np.zeros(kr.CTRL_SIZE)
        # tol below and above the gradient norm: ST_RUN and ST_NO_UPDATE
        for tol in (1e-2, 1e30):
            fa = _run_hess_tail(hb, hb.HESS_TAIL_INIT, True, p, X, zero,
                                tol, 100.0)
            un = _run_hess_tail(hb, hb.HESS_TAIL_INIT, False, p, X, zero,
                                tol, 100.0)
            assert _same(fa, un), f"init {tag} tol={tol}"
            want = kr.ST_RUN if tol < 1 else kr.ST_NO_UPDATE
            assert fa[0][kr.C_STATUS] == want and fa[0][kr.C_RADIUS] == 100.0
            assert torch.equal(fa[1], fa[2]) and not (
                fa[1] == SENTINEL).any()
            assert (fa[0][kr.C_DOT0:kr.C_DOT3 + 1] == 0.0).all()
        ref, bound, _, _ = kr.eval_terms_ref(p, X)
        assert abs(fa[0][kr.C_FX] - ref[0]) <= bound[0], f"init f {tag}"
        # acceptance: f(X) against a stored C_FX just above / far below it
        for fx, rho in ((ref[0] + 1.0, 0.1), (ref[0] - 1e3, 0.1),
                        (ref[0] + 1.0, 1e9)):
            c0 = _history_ctrl(3, 1.0)
            c0[kr.C_DOT0] = c0[kr.C_DOT2] = 0.0
            c0[kr.C_FX], c0[kr.C_DM] = fx, 0.5
            fa = _run_hess_tail(hb, hb.HESS_TAIL_ACCEPT, True, p, X, c0, rho)
            un = _run_hess_tail(hb, hb.HESS_TAIL_ACCEPT, False, p, X, c0,
                                rho)
            assert _same(fa, un), f"accept {tag} fx={fx} rho={rho}"
            accepted = fx > ref[0] and rho < 1
            assert fa[0][kr.C_STATUS] == (
                kr.ST_ACCEPTED if accepted else kr.ST_TCG_STOP), tag
            assert abs(fa[0][kr.C_FPROP] - ref[0]) <= bound[0], tag
        fa = _run_hess_tail(hb, hb.HESS_TAIL_EVAL, True, p, X, zero)
        un = _run_hess_tail(hb, hb.HESS_TAIL_EVAL, False, p, X, zero)
        assert _same(fa, un), f"eval {tag}"
        assert (np.abs(fa[3].numpy() - ref) <= bound).all(), f"eval {tag}"
        assert (fa[0] == 0.0).all(), f"eval leaves dot slots dirty {tag}"


def test_accept_guard_mismatch_touches_nothing():
    """The candidate evaluation with its CF_ACCEPT tail is guarded by
    ST_TCG_STOP: in any other status the control block comes back as it
    was, sentinel dot slots included."""
    hb = _hb()
    d, r, n = 3, 5, 257
    p, X = kr.small_problem(d, r, n, kr.gen(43, d, r, n), with_g=True)
    for status in (kr.ST_RUN, kr.ST_ACCEPTED, kr.ST_NO_UPDATE):
        c0 = _history_ctrl(3, 1.0, status=status)
        c0[kr.C_DOT0] = c0[kr.C_DOT2] = SENTINEL
        got = _run_hess_tail(hb, hb.HESS_TAIL_ACCEPT, True, p, X, c0, 0.1)
        assert np.array_equal(got[0], c0), status


# ---------------------------------------------------------------------
# whole solves, default against DPO_NO_CF=1
# ---------------------------------------------------------------------
# (label, Delta0, accept_rho, max_shrink) on kr.solve_problem(d, r):
# 324 poses for d = 2, 343 for d = 3, two blocks per kernel.
SOLVE_CASES = [("interior", 1e4, 0.1, 10), ("boundary", 1.0, 0.1, 10),
               ("reject", 640.0, kr.SHRINK_ACCEPT_RHO, 2)]
SOLVE_SHAPES = [(2, 2), (3, 5)]

_CHILD = """
import json, sys
sys.path.insert(0, 'tests')
import torch
import kernel_refs as kr
from dpo_amd.ops.hip_backend import DeviceSolver
from dpo_amd.quadratic import QuadraticProblem
cases = json.loads(sys.argv[1])
shapes = json.loads(sys.argv[2])
out = {}
for d, r in shapes:
    p, X = kr.solve_problem(d, r)
    for pre in ('jacobi', 'dense'):
        pd = QuadraticProblem(p.n, d, r, precond=pre)
        pd.set_q(p.Q.to('cuda:0'))
        if pre == 'jacobi':
            pd._Lpre = pd._Lpre.contiguous()
        for label, Delta0, rho, max_shrink in cases:
            ds = DeviceSolver(p.n, d, r, 'cuda:0', max_inner=10)
            Xd = X.clone().to('cuda:0')
            st = ds.solve(pd, Xd, tol=1e-2, Delta0=Delta0,
                          max_shrink=max_shrink, accept_rho=rho,
                          compute_final_gradnorm=False)
            out['%d,%d,%s,%s' % (d, r, pre, label)] = {
                'n': p.n, 'status': st['status'], 'shrinks': st['shrinks'],
                'hlen': int(ds._stats[7]), 'seg': ds.tcg_segment(),
                'conts': ds.counters()['continuations'],
                'ctrl': [float.hex(v) for v in ds.ctrl_block()],
                'X': [float.hex(v) for v in Xd.cpu().flatten().tolist()]}
print(json.dumps(out))
"""

_children = {}


def _child(no_cf, seg):
    key = (no_cf, seg)
    if key not in _children:
        env = dict(os.environ)
        for k in ("DPO_NO_CF", "DPO_TCG_SEG"):
            env.pop(k, None)
        if no_cf:
            env["DPO_NO_CF"] = "1"
        if seg is not None:
            env["DPO_TCG_SEG"] = seg
        cases = SOLVE_CASES if seg is None else SOLVE_CASES[:1]
        p = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(cases),
                            json.dumps(SOLVE_SHAPES)], capture_output=True,
                           text=True, env=env, cwd=HERE, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        _children[key] = json.loads(p.stdout.strip().splitlines()[-1])
    return _children[key]


def _unhex(v):
    return np.array([float.fromhex(x) for x in v])


def _compare_solves(fused, unfused, seg):
    assert fused.keys() == unfused.keys() and fused
    for key, a in fused.items():
        b = unfused[key]
        d, r, pre, label = key.split(",")
        Xa, Xb = _unhex(a["X"]), _unhex(b["X"])
        ca, cb = _unhex(a["ctrl"]), _unhex(b["ctrl"])
        print(key, "seg", seg, "status", a["status"], "hlen", a["hlen"],
              "shrinks", a["shrinks"], "conts", a["conts"], "max|dX|",
              float(np.abs(Xa - Xb).max()), "max|dctrl|",
              float(np.abs(ca - cb).max()), "ctrl slots that differ",
              [(int(i), ca[i], cb[i]) for i in np.flatnonzero(ca != cb)])
        assert a["n"] in (324, 343)
        for k in ("status", "hlen", "shrinks", "seg", "conts"):
            assert a[k] == b[k], (key, k)
        if label == "reject":
            # first candidate rejected; with block-Jacobi every radius is
            # (kr.SHRINK_CASES), the dense path may accept a shrunk one
            assert 1 <= a["shrinks"] <= 2, key
            if pre == "jacobi":
                assert a["status"] == kr.ST_GIVE_UP, key
                assert a["shrinks"] == 2, key
        else:
            assert a["status"] == kr.ST_ACCEPTED and a["shrinks"] == 0, key
        if label == "boundary":
            assert a["hlen"] == 1, key
        if label == "interior":
            assert a["hlen"] > 1, key
            if seg == "1":
                assert a["conts"] == 1, key   # continuation graph ran
        if pre == "jacobi":
            # same operations, same order, two blocks per reduction
            assert np.array_equal(Xa, Xb), key
            # C_RR is the last ||r||^2 of k_tcg_update, which runs one
            # block per 1024 elements: with more than two blocks its
            # atomic partial sums do not commute, in either build, so
            # there it is held to the dot-product rule instead (K
            # partials of non-negative terms: 2 K eps ||r||^2).
            blocks = -(-Xa.size // 1024)
            if blocks > 2:
                rr = kr.C_RR
                assert abs(ca[rr] - cb[rr]) <= 2 * blocks * kr.EPS * cb[rr]
                ca[rr] = cb[rr]
            assert np.array_equal(ca, cb), key
        else:
            # The j-split dense apply adds its partial sums in arbitrary
            # atomic order in both runs, so z differs in its last bits
            # from run to run and the difference grows through the tCG
            # recurrence; 1e-6 absolute on O(1) pose entries is the bound
            # the suite already uses for one dense solve run through two
            # launch structures (test_tcg_segments, test_gpu_kernels).
            assert np.abs(Xa - Xb).max() <= 1e-6, key


def test_whole_solves_match_no_cf():
    _compare_solves(_child(False, None), _child(True, None), None)


def test_continued_solves_match_no_cf():
    """DPO_TCG_SEG=1: the interior solve needs the continuation graph, so
    its tail (candidate, acceptance, publish) runs from the second graph."""
    _compare_solves(_child(False, "1"), _child(True, "1"), "1")


# ---------------------------------------------------------------------
# group evaluation: CF_EVAL releases the fence k_gather3_fenced waits on
# ---------------------------------------------------------------------
def test_group_eval_two_agents():
    """Two agents through dpo_group_eval. The inter-agent term G is
    assembled from small-integer edge data, so every product and sum in
    it is exact in fp64 whatever the atomic order, and the CPU reference
    with the same G keeps the bounds of kr.eval_terms_ref. The second
    evaluation returns the same values only if the first cleaned its dot
    slots."""
    hb = _hb()
    d, r = 3, 5
    dh = d + 1
    solvers, Xs, nbrs, refs, keep = [], [], [], [], []
    for agent, n in enumerate((65, 257)):
        g = kr.gen(47, agent)
        p, X = kr.small_problem(d, r, n, g, with_g=False)
        ne, m = 40, 9
        E0 = torch.randint(-3, 4, (ne, dh, dh), generator=g).double()
        nbr = torch.randint(-3, 4, (m, dh, r), generator=g).double()
        w = torch.randint(1, 3, (ne,), generator=g).double()
        lp = torch.randint(0, n, (ne,), generator=g)
        slot = torch.randint(0, m, (ne,), generator=g)
        G = torch.zeros(n, dh, r, dtype=torch.float64)
        G.index_add_(0, lp, -w[:, None, None] * (E0 @ nbr[slot]))
        p.set_g(G.reshape(dh * n, r))
        refs.append(kr.eval_terms_ref(p, X)[:2])
        # dense preconditioner: the path on which the evaluation is fused
        pd = type(p)(n, d, r, precond="dense")
        pd.set_q(p.Q.to(DEV))
        ds = hb.DeviceSolver(n, d, r, DEV, max_inner=10)
        ds.bind_problem_static(pd)
        gd = [_dev(E0), _dev(lp), _dev(slot), _dev(w)]
        ds.set_gdata(*gd)
        keep.append((pd, gd))
        solvers.append(ds)
        Xs.append(_dev(X))
        nbrs.append(_dev(nbr))
    grp = hb.DeviceGroup(solvers, Xs, nbrs, [0, 1])
    out = torch.full((2, 3), SENTINEL, dtype=torch.float64, device=DEV)
    got = []
    for rep in range(2):
        out.fill_(SENTINEL)
        grp.eval_all(out)
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
        for agent, (ref, bound) in enumerate(refs):
            err = np.abs(got[rep][agent] - ref)
            print("agent", agent, "call", rep, "err", err, "bound", bound)
            assert (err <= bound).all(), (agent, rep)
    assert np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------
# Hd stage with the direction update folded in
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", SHAPES)
def test_hd_stage_folded_delta_matches_unfused(d, r):
    """k_hess_fused AUX = 2 (delta formed per neighbour from the old
    buffer and z, own tile written to the other buffer) against
    k_tcg_delta in place + the Hessian kernel: Hd, the new delta and every
    control slot bit for bit, for both parities of C_ITER and for
    C_BETA = 0 (the head's first delta) and a loop value. The buffer a
    parity only reads must come back unchanged. A status other than
    ST_RUN leaves everything untouched."""
    hb = _hb()
    for n in N_POSE:
        p, X = kr.small_problem(d, r, n, kr.gen(53, d, r, n), with_g=False)
        g = kr.gen(59, d, r, n)
        Q = p.Q.to(DEV)
        dold, z = kr.randn(g, *X.shape), kr.randn(g, *X.shape)
        for it, beta in ((0, 0.0), (1, 0.37), (2, 1.9)):
            c0 = np.zeros(kr.CTRL_SIZE)
            c0[kr.C_STATUS] = kr.ST_RUN
            c0[kr.C_ITER], c0[kr.C_BETA] = it, beta
            c0[kr.C_ZR], c0[kr.C_DPD], c0[kr.C_RADIUS] = 0.8, 1.1, 1e3
            tag = f"hd stage d={d} r={r} n={n} iter={it}"
            # unfused twin
            cu = _dev(torch.from_numpy(c0.copy()))
            du, Hu = _dev(dold), torch.full_like(_dev(X), SENTINEL)
            hb.hd_stage(Q, du, None, _dev(z), _dev(X), Hu, cu, d, False)
            # fused: old direction in buffer 1 - parity
            cf = _dev(torch.from_numpy(c0.copy()))
            bufs = [torch.full_like(du, SENTINEL) for _ in range(2)]
            bufs[1 - (it & 1)] = _dev(dold)
            Hf = torch.full_like(Hu, SENTINEL)
            hb.hd_stage(Q, bufs[0], bufs[1], _dev(z), _dev(X), Hf, cf, d,
                        True)
            torch.cuda.synchronize()
            assert torch.equal(bufs[it & 1].cpu(), du.cpu()), tag
            assert torch.equal(bufs[1 - (it & 1)].cpu(), dold), tag
            assert torch.equal(Hf.cpu(), Hu.cpu()), tag
            assert not (Hf == SENTINEL).any(), tag
            assert np.array_equal(cf.cpu().numpy(), cu.cpu().numpy()), tag
            assert cf[kr.H_DHD(it)].item() != 0.0, tag   # the tail ran
        c0[kr.C_STATUS] = kr.ST_TCG_STOP
        cf = _dev(torch.from_numpy(c0.copy()))
        bufs = [torch.full_like(du, SENTINEL) for _ in range(2)]
        Hf = torch.full_like(Hu, SENTINEL)
        hb.hd_stage(Q, bufs[0], bufs[1], _dev(z), _dev(X), Hf, cf, d, True)
        torch.cuda.synchronize()
        assert np.array_equal(cf.cpu().numpy(), c0)
        assert all((t == SENTINEL).all() for t in (bufs[0], bufs[1], Hf))


# ---------------------------------------------------------------------
# dense fp32 preconditioner apply (exported op, fixed contract)
# ---------------------------------------------------------------------
DENSE_N = (1, 255, 256, 257, 1029, 1372)


@pytest.mark.parametrize("r", (2, 5, 8))
def test_precond_dense_matrix(r):
    """dpo_precond_dense against the fp64 CPU product of the same fp32
    matrix, bound 2 K eps sum |m| |v| with K = N terms per entry."""
    hb = _hb()
    for N in DENSE_N:
        gd = torch.Generator(device=DEV).manual_seed(1000 * N + r)
        Md = torch.randn(N, N, dtype=torch.float32, device=DEV,
                         generator=gd)
        Md = (0.5 * (Md + Md.T)).contiguous()
        V = kr.randn(kr.gen(61, N, r), N, r)
        M64 = Md.cpu().double()
        ref = M64 @ V
        bound = 2.0 * N * kr.EPS * (M64.abs() @ V.abs())
        out = torch.full_like(_dev(V), float("nan"))
        hb.precond_dense(Md, _dev(V), out=out)
        torch.cuda.synchronize()
        err = (out.cpu() - ref).abs()
        print("precond_dense N", N, "r", r, "max err/bound",
              float((err / bound).max()))
        assert bool((err <= bound).all()), (N, r)
