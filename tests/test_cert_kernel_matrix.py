"""Kernel test matrix of the Lanczos certificate path: k_cert_lambda,
k_cert_apply, k_cert_gram, k_cert_sub, k_cert_norm and k_cert_reduce at
every compiled shape, the block edges, a grid-stride wrap, with
sentinel-padded buffers, the breakdown branches, the cert_off guard and
the fixed summation order (docs/DESIGN.md, "Kernel test matrix").

The entry points are called through ctypes, so every buffer a kernel
touches (w, cvec, part, gpart) belongs to the test. References come from
ops/cpu_ref.py (scalar-CSR sparse product, never a dense matrix), bounds
from the same functions on abs() copies; tests/kernel_refs.py derives
them and tests/test_kernel_refs.py checks them on the CPU.
"""
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr
from dpo_amd.ops import cpu_ref
from test_kernel_matrix import _assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = kr.CERT_SENTINEL
PAD = kr.CERT_PAD
M = kr.CERT_M
HDR, FLAG, COUNT, TOL = (cpu_ref.CERT_HDR, cpu_ref.CERT_FLAG,
                         cpu_ref.CERT_COUNT, cpu_ref.CERT_TOL)
NAN = float("nan")


def _hb():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import hip_backend
    assert hip_backend._CERT_PART == cpu_ref.CERT_BLOCK == 256
    return hip_backend


class Buf:
    """Device buffer with PAD sentinel slots on either side of the data:
    .t is the data view handed to the kernel."""

    def __init__(self, data=None, shape=None, fill=SENT):
        if data is None:
            data = torch.full(shape, fill, dtype=torch.float64)
        flat = data.reshape(-1).to(torch.float64)
        k = flat.numel()
        host = torch.full((k + 2 * PAD,), SENT, dtype=torch.float64)
        host[PAD:PAD + k] = flat
        self.buf = host.to(DEV)
        self.t = self.buf[PAD:PAD + k].view(data.shape)

    def host(self, label):
        """The data on the host, after checking that both pads survive."""
        h = self.buf.cpu()
        k = h.numel() - 2 * PAD
        assert bool((h[:PAD] == SENT).all()), f"{label}: wrote before start"
        assert bool((h[PAD + k:] == SENT).all()), f"{label}: wrote past end"
        return h[PAD:PAD + k].view(self.t.shape)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b, label):
    assert torch.equal(_bits(a), _bits(b)), f"{label}: not bit-identical"


def _qdev(Q):
    return Q.row_ptr.to(DEV), Q.col_idx.to(DEV), Q.vals.to(DEV)


def _is_sentinel(t):
    return bool((t == SENT).all())


# ---------------------------------------------------------------------
# A. k_cert_lambda + k_cert_reduce
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_lambda_and_residual(d, r):
    """Lambda blocks and ||QX - Lambda X||^2 from X and a random QX handed
    in directly, at every compiled shape; at (2, 6) and (3, 8) also one
    pose past 256 full blocks (second grid-stride trip, 256 partials)."""
    hb = _hb()
    for n in kr.cert_lambda_poses(d, r):
        label = f"cert_lambda d={d} r={r} n={n}"
        g = kr.gen(41, d, r, n)
        X = kr.manifold_point(n, d, r, g)
        QX = kr.randn(g, (d + 1) * n, r)
        lam_ref, res_ref, b_lam, b_res = kr.cert_lambda_ref(X, QX, d)
        lam = Buf(shape=(n, d, d), fill=NAN)
        res = Buf(shape=(1,), fill=NAN)
        part = Buf(shape=(256,))
        Xd, QXd = X.to(DEV), QX.to(DEV)
        hb._lib.dpo_cert_lambda(hb._p(Xd), hb._p(QXd), hb._p(lam.t),
                                hb._p(res.t), hb._p(part.t), n, d, r,
                                hb._stream(Xd))
        torch.cuda.synchronize()
        _assert_close(lam.host(label), lam_ref, b_lam, label + " lam")
        _assert_close(res.host(label), [res_ref], [b_res], label + " res")
        ph = part.host(label)
        npart = cpu_ref.cert_partials(n)
        assert _is_sentinel(ph[npart:]), label
        assert bool(torch.isfinite(ph[:npart]).all()) and not bool(
            (ph[:npart] == SENT).any()), label
        # the residual is the fixed-order sum of exactly these partials
        assert float(res.host(label)[0]) == kr.cert_fixed_order_sum(
            ph[:npart].numpy()), label


# ---------------------------------------------------------------------
# B. k_cert_apply
# ---------------------------------------------------------------------
def _apply_raw(hb, Qd, lam, v, vprev, beta, w, alpha, part, n, d):
    hb._lib.dpo_cert_apply(hb._p(Qd[0]), hb._p(Qd[1]), hb._p(Qd[2]),
                           hb._p(lam), hb._p(v), hb._p(vprev), hb._p(beta),
                           hb._p(w), hb._p(alpha), hb._p(part), n, d,
                           hb._stream(v))
    torch.cuda.synchronize()


ROW_CASES = [(d, n) for d in (2, 3) for n in kr.CERT_ROW_POSES[d]]


@pytest.mark.parametrize("d,n", ROW_CASES)
def test_apply_three_forms(d, n):
    """w = S v - beta vprev and alpha = <v, w>: without vprev, with
    vprev and beta = 0.37, and with vprev but a null beta_prev (beta = 0
    by definition)."""
    hb = _hb()
    N = n * (d + 1)
    Q, Qa = kr.cert_matrix(n, d)
    Qd = _qdev(Q)
    g = kr.gen(42, d, n)
    lam = kr.cert_lam_blocks(n, d, g)
    v, vprev = kr.randn(g, N), kr.randn(g, N)
    lamd = Buf(lam)
    vd, vpd = v.to(DEV), vprev.to(DEV)
    betad = torch.tensor([kr.CERT_BETA_PREV], dtype=torch.float64,
                         device=DEV)
    forms = {"no-vprev": (None, None, None, 0.0),
             "beta": (vpd, betad, vprev, kr.CERT_BETA_PREV),
             "null-beta": (vpd, None, None, 0.0)}
    for form, (vp_dev, b_dev, vp_ref, beta) in forms.items():
        label = f"cert_apply d={d} n={n} {form}"
        w_ref, a_ref, b_w, b_a = kr.cert_apply_ref(Q, Qa, lam, v, vp_ref,
                                                   beta)
        w = Buf(shape=(N,), fill=NAN)
        alpha = Buf(shape=(1,))
        part = Buf(shape=(256,))
        _apply_raw(hb, Qd, lamd.t, vd, vp_dev, b_dev, w.t, alpha.t, part.t,
                   n, d)
        _assert_close(w.host(label), w_ref, b_w, label + " w")
        _assert_close(alpha.host(label), [a_ref], [b_a], label + " alpha")
        ph = part.host(label)
        npart = cpu_ref.cert_partials(N)
        assert _is_sentinel(ph[npart:]), label
        assert float(alpha.host(label)[0]) == kr.cert_fixed_order_sum(
            ph[:npart].numpy()), label
        lamd.host(label)


@pytest.mark.parametrize("d,n", ROW_CASES)
def test_apply_translation_rows_get_no_lambda(d, n):
    """With Lambda blocks of 1e6 the translation rows (c == d) must still
    equal the plain Q v reference within its own bound."""
    hb = _hb()
    N = n * (d + 1)
    label = f"cert_apply translation rows d={d} n={n}"
    Q, Qa = kr.cert_matrix(n, d)
    v = kr.randn(kr.gen(45, d, n), N)
    zero = torch.zeros(n, d, d, dtype=torch.float64)
    w_ref, _, b_w, _ = kr.cert_apply_ref(Q, Qa, zero, v)
    # the Lambda buffer is padded: a row index one too far stays inside it
    big = Buf(torch.full((n, d, d), 1e6, dtype=torch.float64))
    w = Buf(shape=(N,), fill=NAN)
    alpha, part = Buf(shape=(1,)), Buf(shape=(256,))
    _apply_raw(hb, _qdev(Q), big.t, v.to(DEV), None, None, w.t, alpha.t,
               part.t, n, d)
    wt = w.host(label).view(n, d + 1)
    _assert_close(wt[:, d], w_ref.view(n, d + 1)[:, d],
                  b_w.view(n, d + 1)[:, d], label)
    # and the rotation rows did get it
    assert float((wt[:, :d] - w_ref.view(n, d + 1)[:, :d]).abs().max()) > 1.0


# ---------------------------------------------------------------------
# C. one Lanczos step, dissected
# ---------------------------------------------------------------------
class StepRun:
    """One call of dpo_cert_lanczos (path "column") or
    dpo_cert_lanczos_split (path "split") on test-owned buffers."""

    def __init__(self, hb, Q, lam, V, ctl, path, first, nsteps):
        n, d = lam.shape[0], lam.shape[1]
        m = V.shape[0] - 1
        N = V.shape[1]
        self.V, self.ctl = Buf(V), Buf(ctl)
        self.w = Buf(shape=(N,), fill=NAN)
        self.cvec = Buf(shape=(m + 1,))
        self.part = Buf(shape=(256,))
        self.gpart = Buf(shape=((m + 1) * 256,))
        Qd = _qdev(Q)
        lamd = lam.to(DEV)
        head = [hb._p(Qd[0]), hb._p(Qd[1]), hb._p(Qd[2]), hb._p(lamd),
                hb._p(self.V.t), hb._p(self.w.t), hb._p(self.cvec.t),
                hb._p(self.part.t)]
        tail = [hb._p(self.ctl.t), n, d, m, first, nsteps,
                hb._stream(lamd)]
        if path == "split":
            hb._lib.dpo_cert_lanczos_split(*head, hb._p(self.gpart.t), *tail)
        else:
            assert path == "column"
            hb._lib.dpo_cert_lanczos(*head, *tail)
        torch.cuda.synchronize()

    def host(self, label):
        return {k: getattr(self, k).host(f"{label} {k}")
                for k in ("V", "ctl", "w", "cvec", "part", "gpart")}


def _ctl_others_unchanged(ctl_after, ctl_before, touched, label):
    keep = torch.ones(ctl_before.numel(), dtype=torch.bool)
    keep[list(touched)] = False
    same = _bits(ctl_after) == _bits(ctl_before)
    assert bool(same[keep].all()), (
        f"{label}: ctl slots {(~same & keep).nonzero()[:, 0].tolist()} "
        "changed")


STEP_CASES = [(3, n) for n in kr.CERT_ROW_POSES[3]] + [
    (2, n) for n in kr.CERT_ROW_POSES[2]]


@pytest.mark.parametrize("d,n", STEP_CASES)
def test_one_lanczos_step_dissected(d, n):
    """alpha_j, beta_j, v_{j+1}, the post-CGS2 w, the second-pass cvec and
    the beta^2 partials of one step against cpu_ref, by both Gram paths;
    two runs of a path are bit-identical; nothing else is written."""
    hb = _hb()
    N = n * (d + 1)
    npart = cpu_ref.cert_partials(N)
    for j in kr.cert_steps_for(N):
        Q, Qa, lam, V, ctl = kr.cert_step_state(n, d, j)
        st = kr.cert_step_ref(Q, Qa, lam, V, ctl, j)
        Vc, cc = V.clone(), ctl.clone()
        cpu_ref.cert_lanczos_steps(Q, lam, Vc, cc, j, 1)
        # alpha_j, beta_j and v_{j+1} are compared with cpu_ref's own
        # outputs; st supplies their bounds and the intermediates
        a_ref, beta_ref = float(cc[HDR + j]), float(cc[HDR + M + j])
        assert float(cc[FLAG]) == 0.0 and float(cc[COUNT]) == j + 1
        for path in ("column", "split"):
            label = f"cert step d={d} n={n} j={j} {path}"
            out = StepRun(hb, Q, lam, V, ctl, path, j, 1).host(label)
            c = out["ctl"]
            _assert_close(c[HDR + j:HDR + j + 1], [a_ref], [st.b_alpha],
                          label + " alpha")
            _assert_close(c[HDR + M + j:HDR + M + j + 1], [beta_ref],
                          [st.b_beta], label + " beta")
            assert float(c[COUNT]) == j + 1 and float(c[FLAG]) == 0.0
            _ctl_others_unchanged(c, ctl, (COUNT, HDR + j, HDR + M + j),
                                  label)
            _assert_close(out["V"][j + 1], Vc[j + 1], st.b_v, label + " v")
            _assert_close(out["w"], st.w2, st.b_w2, label + " w")
            _assert_close(out["cvec"][:j + 1], st.c2, st.b_c2,
                          label + " cvec")
            beta2 = math.fsum(out["part"][:npart].tolist())
            _assert_close([beta2], [st.beta2], [st.b_beta2],
                          label + " sum(part)")
            _same_bits(out["V"][:j + 1], V[:j + 1], label + " V[0..j]")
            assert _is_sentinel(out["V"][j + 2:]), label
            assert _is_sentinel(out["cvec"][j + 1:]), label
            assert _is_sentinel(out["part"][npart:]), label
            used = (j + 1) * npart if path == "split" else 0
            assert _is_sentinel(out["gpart"][used:]), label
            again = StepRun(hb, Q, lam, V, ctl, path, j, 1).host(label)
            for k in out:
                _same_bits(again[k], out[k], f"{label} rerun {k}")


# ---------------------------------------------------------------------
# D. k_cert_norm branches and the cert_off guard
# ---------------------------------------------------------------------
NORM_CASES = [(3, 65), (3, 16385)]      # N = 260 (two blocks), 65 540
NORM_J = 1


def _breakdown_state(kind, d, n):
    """(Q, lam, V, ctl) whose step NORM_J breaks down in the given way."""
    j = NORM_J
    if kind == "threshold":
        Q, _, lam, V, ctl = kr.cert_step_state(n, d, j, tol=1e300)
    elif kind == "zero":
        _, _, lam, V, ctl = kr.cert_step_state(n, d, j, beta_prev=0.0)
        Q = kr.cert_zero_matrix(n, d)
        lam = torch.zeros_like(lam)
    else:
        assert kind == "nan"
        Q, _, lam, V, ctl = kr.cert_step_state(n, d, j)
        V[j, V.shape[1] - 3] = NAN         # a row of the last block
    return Q, lam, V, ctl


def _assert_breakdown(V_after, c_after, V, ctl, label):
    """flag = 1, beta_j = +0.0, COUNT = j + 1, the whole row j + 1 and
    everything after it untouched, alpha_{j+1} and beta_{j+1} untouched."""
    j = NORM_J
    assert float(c_after[FLAG]) == 1.0, label
    assert _bits(c_after[HDR + M + j:HDR + M + j + 1]).item() == 0, label
    assert float(c_after[COUNT]) == j + 1, label
    _ctl_others_unchanged(c_after, ctl, (FLAG, COUNT, HDR + j, HDR + M + j),
                          label)
    _same_bits(V_after[:j + 1], V[:j + 1], label + " V[0..j]")
    assert _is_sentinel(V_after[j + 1:]), label + ": row j + 1 written"


@pytest.mark.parametrize("kind", ["threshold", "zero", "nan"])
@pytest.mark.parametrize("d,n", NORM_CASES)
def test_norm_breakdown_branches(d, n, kind):
    """beta below the threshold, beta exactly 0 and beta NaN, with three
    steps enqueued in one call: step j raises the flag in every block's
    view and the two later steps of the batch are no-ops."""
    hb = _hb()
    j = NORM_J
    Q, lam, V, ctl = _breakdown_state(kind, d, n)
    # the CPU reference takes the same branch
    Vc, cc = V.clone(), ctl.clone()
    cpu_ref.cert_lanczos_steps(Q, lam, Vc, cc, j, 3)
    _assert_breakdown(Vc, cc, V, ctl, f"cpu_ref {kind}")
    for path in ("column", "split"):
        label = f"cert_norm {kind} d={d} n={n} {path}"
        out = StepRun(hb, Q, lam, V, ctl, path, j, 3).host(label)
        _assert_breakdown(out["V"], out["ctl"], V, ctl, label)
        a_dev, a_ref = out["ctl"][HDR + j], cc[HDR + j]
        if kind == "nan":
            assert math.isnan(float(a_dev)) and math.isnan(float(a_ref))
        else:
            assert bool(torch.isfinite(out["ctl"]).all()), label
            assert bool(torch.isfinite(out["V"][:j + 1]).all()), label
        if kind == "zero":
            assert float(a_dev) == 0.0 == float(a_ref)
            assert not bool(out["w"].any()), label
        # the later steps of the batch touched nothing: same bits as a
        # call that enqueues step j alone
        one = StepRun(hb, Q, lam, V, ctl, path, j, 1).host(label)
        for k in out:
            _same_bits(out[k], one[k], f"{label} nsteps 3 vs 1: {k}")


@pytest.mark.parametrize("d,n", NORM_CASES)
def test_raised_flag_makes_every_step_a_no_op(d, n):
    """With the flag raised beforehand both Lanczos entry points leave
    V, w, cvec, part, gpart and ctl bit-identical. dpo_cert_apply takes
    no control array: it must run regardless."""
    hb = _hb()
    j = NORM_J
    N = n * (d + 1)
    Q, Qa, lam, V, ctl = kr.cert_step_state(n, d, j)
    ctl[FLAG] = 1.0
    Vc, cc = V.clone(), ctl.clone()
    cpu_ref.cert_lanczos_steps(Q, lam, Vc, cc, j, 3)
    _same_bits(Vc, V, "cpu_ref V")
    _same_bits(cc, ctl, "cpu_ref ctl")
    for path in ("column", "split"):
        label = f"cert_off d={d} n={n} {path}"
        run = StepRun(hb, Q, lam, V, ctl, path, j, 3)
        out = run.host(label)
        _same_bits(out["V"], V, label + " V")
        _same_bits(out["ctl"], ctl, label + " ctl")
        assert bool(torch.isnan(out["w"]).all()), label + " w"
        for k in ("cvec", "part", "gpart"):
            assert _is_sentinel(out[k]), f"{label} {k}"
    label = f"cert_apply ignores the flag d={d} n={n}"
    w_ref, a_ref, b_w, b_a = kr.cert_apply_ref(Q, Qa, lam, V[j])
    w, alpha, part = Buf(shape=(N,), fill=NAN), Buf(shape=(1,)), Buf(
        shape=(256,))
    _apply_raw(hb, _qdev(Q), lam.to(DEV), V[j].to(DEV), None, None, w.t,
               alpha.t, part.t, n, d)
    _assert_close(w.host(label), w_ref, b_w, label + " w")
    _assert_close(alpha.host(label), [a_ref], [b_a], label + " alpha")


# ---------------------------------------------------------------------
# E. full 256-partial fan-in of cert_sum_partials, bit for bit
# ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sparse", "dense"])
def test_full_fan_in_is_the_documented_order(case):
    """N = 65 536 makes all 256 partial slots live. The device sum must
    equal the emulation of its order bit for bit: a 64-lane xor-shuffle
    tree per wave, then waves 0..3 in sequence."""
    hb = _hb()
    N = 65536
    assert cpu_ref.cert_partials(N) == 256
    p = kr.cert_fanin_cases()[case]
    want = kr.cert_fixed_order_sum(p)
    g = kr.gen(46)
    V, w = kr.randn(g, 1, N), kr.randn(g, N)
    part = Buf(torch.from_numpy(p.copy()))
    alpha, c, gpart = Buf(shape=(1,)), Buf(shape=(1,)), Buf(shape=(256,))
    Vd, wd = V.to(DEV), w.to(DEV)
    hb._lib.dpo_cert_gram_split(hb._p(Vd), hb._p(wd), hb._p(c.t),
                                hb._p(gpart.t), hb._p(None), hb._p(part.t),
                                hb._p(alpha.t), 1, N, hb._stream(Vd))
    torch.cuda.synchronize()
    label = f"fan-in {case}"
    got = float(alpha.host(label)[0])
    print(f"{label}: device {got!r}, emulation {want!r}, "
          f"exact {math.fsum(p)!r}")
    assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64)
    _same_bits(part.host(label), torch.from_numpy(p), label + " part")
    _assert_close(c.host(label), [float(V[0] @ w)], [kr.dot_bound(V[0], w)],
                  label + " c")
    assert float(c.host(label)[0]) == kr.cert_fixed_order_sum(
        gpart.host(label).numpy()), label
