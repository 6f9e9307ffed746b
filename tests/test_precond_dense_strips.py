"""Dense preconditioner apply by column strips (docs/DESIGN.md section 3).

A block owns 32 output rows and the whole j range, so Z is written with
plain stores in a fixed summation order. The 16-byte-load instantiation
runs when N % 4 == 0 and Minv is 16-byte aligned, the 4-byte-load one
otherwise; both use the same strip, reduction and stores.

Vector-path sizes: one lane group (4), the strip edge 32 +- 4, the edge of
the 32-row block pass 128 +- 4 (and with it several strips), 1024 / 1028
(32 strips, 33 with a 4-row tail) and the benchmark's 1252. Scalar-path
sizes: 3, 33, 195, 771, 1251 (odd N), and 1028 with Minv a view offset by
one float, which fails the alignment test.
"""
import functools

import pytest
import torch

import kernel_refs as kr
import test_batched_rounds_gpu as tb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.25e77
VEC_N = (4, 28, 32, 36, 124, 128, 132, 1024, 1028, 1252)
SCALAR_N = (3, 33, 195, 771, 1251)
OFFSET_N = 1028


def _hb():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import hip_backend
    return hip_backend


@functools.lru_cache(maxsize=None)
def _matrix(N):
    """Symmetric fp32 matrix on the device behind one spare float (so a
    view offset by one float exists), and its fp64 copy on the host."""
    g = kr.gen(71, N)
    A = torch.randn(N, N, dtype=torch.float32, generator=g)
    M = (0.5 * (A + A.T)).contiguous()
    buf = torch.zeros(N * N + 1, dtype=torch.float32, device=DEV)
    return buf, M, M.double()


def _aligned(N):
    buf, M, M64 = _matrix(N)
    Md = buf[:N * N].view(N, N)
    Md.copy_(M)
    assert Md.data_ptr() % 16 == 0
    return Md, M64


def _offset(N):
    buf, M, M64 = _matrix(N)
    Md = buf[1:].view(N, N)
    Md.copy_(M)
    assert Md.data_ptr() % 16 == 4
    return Md, M64


def _apply(hb, Md, V):
    """One launch into a NaN-filled output with 64 sentinels behind it;
    every row must be written and nothing beyond."""
    N, r = V.shape
    buf = torch.full((N * r + 64,), SENTINEL, dtype=torch.float64,
                     device=DEV)
    out = buf[:N * r].view(N, r)
    out.fill_(float("nan"))
    hb.precond_dense(Md, V, out=out)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), ("row not written", N, r)
    assert bool((buf[N * r:] == SENTINEL).all()), ("wrote past Z", N, r)
    return out.clone()


def _check(hb, Md, M64, N, r, label):
    V = kr.randn(kr.gen(72, N, r), N, r)
    Vd = V.to(DEV)
    out = _apply(hb, Md, Vd)
    ref = M64 @ V
    bound = kr.matmul_bound(M64, V, N)
    err = (out.cpu() - ref).abs()
    print(label, "N", N, "r", r, "max err/bound",
          float((err / bound).max()))
    assert bool((err <= bound).all()), (label, N, r)
    # determinism: a second launch on the same inputs, bit for bit
    assert torch.equal(out, _apply(hb, Md, Vd)), (label, N, r)
    return out


@pytest.mark.parametrize("r", kr.RS)
def test_vector_path(r):
    hb = _hb()
    for N in VEC_N:
        Md, M64 = _aligned(N)
        _check(hb, Md, M64, N, r, "vector")


@pytest.mark.parametrize("r", kr.RS)
def test_scalar_path(r):
    hb = _hb()
    for N in SCALAR_N:
        Md, M64 = _aligned(N)
        _check(hb, Md, M64, N, r, "scalar")
    # an offset view must take the 4-byte loads, and gives the bits of
    # the 16-byte loads: same strip, same summation order
    Md, M64 = _offset(OFFSET_N)
    off = _check(hb, Md, M64, OFFSET_N, r, "scalar-offset")
    Md, M64 = _aligned(OFFSET_N)
    V = kr.randn(kr.gen(72, OFFSET_N, r), OFFSET_N, r).to(DEV)
    assert torch.equal(off, _apply(hb, Md, V)), r


def test_guarded_off_is_zero():
    """The exported stand-alone entry returns exactly zero when guarded
    off, on both paths."""
    hb = _hb()
    for N in (36, 33):
        Md, _ = _aligned(N)
        V = kr.randn(kr.gen(73, N), N, 5).to(DEV)
        ctrl = torch.zeros(kr.CTRL_SIZE, dtype=torch.float64, device=DEV)
        ctrl[kr.C_STATUS] = kr.ST_TCG_STOP
        out = torch.full_like(V, float("nan"))
        hb.precond_dense(Md, V, out=out, ctrl=ctrl, guard=hb.GUARD_RUN)
        torch.cuda.synchronize()
        assert bool((out == 0.0).all()), N


@pytest.mark.parametrize("d,r", tb.SHAPES)
def test_batched_parity(d, r):
    """kb_precond_dense (dpo_batch_op 8): every agent's z is bit-identical
    to its single-agent launch. z starts as garbage: the apply overwrites
    it and needs no cleared output. (3, 5): N = 28, 1024, 1028, all on
    the vector path; (2, 4): N = 21, 768, 771, a mixed batch that runs
    the scalar instantiation against single launches on either path."""
    lib = tb._lib()
    base = [tb._agent(n, d, r, 30 + i) for i, n in enumerate(tb.NS)]
    for a in base:
        a["ctrl"][tb.C_STATUS] = tb.ST_RUN
    single = [tb._clone(a) for a in base]
    for a in single:
        lib.dpo_precond_dense(tb._p(a["Minv"]), tb._p(a["rvec"]),
                              tb._p(a["z"]), a["N"], r, tb._p(a["ctrl"]), 0,
                              None)
    torch.cuda.synchronize()
    bat = [tb._clone(a) for a in base]
    tb._batch_op(8, bat, d, r)
    for s, b in zip(single, bat):
        tb._check(s, s, b, [], ["z", "rvec", "ctrl"], b["n"])
        assert not bool((b["z"][:b["total"]] == tb.SENTINEL).any())
