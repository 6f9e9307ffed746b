"""GPU tests of the LOBPCG certificate path (docs/DESIGN.md §20): every
new HIP op against its fp64 counterpart in ops/cpu_ref.py from common
inputs, the status guards, run-to-run determinism, and
certify_solution(method="lobpcg") on GPU tensors against the CPU run.

Tolerances are forward rounding bounds 2 K eps sum |a| |b| (K terms per
sum, the factor 2 for the two computations compared), evaluated with the
reference itself on abs() copies of the inputs.
"""
import functools

import numpy as np
import pytest
import torch

from test_certify import dense_S, grid_case, grid_reference, ring_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
POSES = (1, 65, 256, 257)
# one row past 256 blocks x 256 threads: one thread takes a second trip
N_WRAP = 65537
DM = [(d, m) for d, ms in ((2, range(2, 7)), (3, range(3, 9))) for m in ms]


def _backends():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import cpu_ref, hip_backend
    return cpu_ref, hip_backend


@functools.lru_cache(maxsize=None)
def _bsr(n, d):
    """A random BSR matrix with up to four blocks per row (the apply does
    not need symmetry) and random Lambda blocks."""
    from dpo_amd.quadratic import BSRMatrix
    dh = d + 1
    cols = [sorted({(i - 1) % n, i, (i + 1) % n, (7 * i + 3) % n})
            for i in range(n)]
    row_ptr = np.cumsum([0] + [len(c) for c in cols]).astype(np.int32)
    col_idx = np.concatenate(cols).astype(np.int32)
    g = torch.Generator().manual_seed(100 * n + d)
    vals = torch.randn(len(col_idx), dh, dh, dtype=torch.float64,
                       generator=g)
    lam = torch.randn(n, d, d, dtype=torch.float64, generator=g)
    Q = BSRMatrix(n, dh, torch.from_numpy(row_ptr),
                  torch.from_numpy(col_idx), vals)
    return Q, lam


def _workspaces(N, m, seed):
    """A CPU and a GPU workspace with the same random contents, theta and
    coefficients."""
    cpu_ref, _ = _backends()
    g = torch.Generator().manual_seed(seed)
    wc = cpu_ref.LobWorkspace(N, m)
    for t in (wc.B, wc.SB, wc.R):
        t.copy_(torch.randn(t.shape, dtype=torch.float64, generator=g))
    theta = torch.randn(m, dtype=torch.float64, generator=g)
    C = torch.randn(3 * m, 2 * m, dtype=torch.float64, generator=g)
    cpu_ref.lob_set_coefficients(wc.ctl, theta, C, m)
    return wc, _to_gpu(wc)


def _to_gpu(wc):
    cpu_ref, _ = _backends()
    wg = cpu_ref.LobWorkspace(wc.N, wc.m, DEV)
    for name in ("B", "SB", "R", "ctl", "part", "out"):
        getattr(wg, name).copy_(getattr(wc, name))
    return wg


def _abs_copy(wc):
    cpu_ref, _ = _backends()
    wa = cpu_ref.LobWorkspace(wc.N, wc.m)
    for name in ("B", "SB", "R", "ctl"):
        getattr(wa, name).copy_(getattr(wc, name).abs())
    wa.ctl[cpu_ref.LOB_STATUS] = 0.0
    return wa


def _close(got, ref, bound, what):
    err = (got.cpu() - ref).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max())!r} max bound "
          f"{float(bound.max())!r}")
    assert worst <= 0.0, what


# --------------------------------------------------------------------
# 1. ops against cpu_ref
# --------------------------------------------------------------------
@pytest.mark.parametrize("d,m", DM)
def test_apply_matches_cpu(d, m):
    cpu_ref, hip = _backends()
    for n in POSES:
        Q, lam = _bsr(n, d)
        N = n * (d + 1)
        wc, wg = _workspaces(N, m, 3)
        blk = cpu_ref.LOB_W
        cpu_ref.cert_lob_apply(Q, lam, wc, blk)
        hip.cert_lob_apply(Q.to(DEV), lam.to(DEV), wg, blk)
        # |Q| |W| + |Lambda| |W|: at most 4 (d + 1) + d terms per entry
        from dpo_amd.quadratic import BSRMatrix
        Qa = BSRMatrix(Q.n, Q.dh, Q.row_ptr, Q.col_idx, Q.vals.abs())
        wa = _abs_copy(wc)
        cpu_ref.cert_lob_apply(Qa, -lam.abs(), wa, blk)
        K = 4 * (d + 1) + d
        _close(wg.SB[blk], wc.SB[blk], 2 * K * EPS * wa.SB[blk],
               f"apply d={d} m={m} n={n}")
        # nothing but SB[blk] was written
        for other in (0, 2):
            assert torch.equal(wg.SB[other].cpu(), wc.SB[other])
        assert torch.equal(wg.B.cpu(), wc.B)


@pytest.mark.parametrize("m", range(2, 9))
def test_resid_and_gram_match_cpu(m):
    cpu_ref, hip = _backends()
    for N in (3, 195, 768, 1028, N_WRAP):
        wc, wg = _workspaces(N, m, 5)
        wa = _abs_copy(wc)
        cpu_ref.cert_lob_resid(wc, zero=True)
        hip.cert_lob_resid(wg, zero=True)
        cpu_ref.cert_lob_resid(wa)
        # R = SX - theta X: two terms
        _close(wg.R, wc.R, 2 * 2 * EPS * (wa.SB[0] + wa.B[0] * wa.ctl[
            cpu_ref.LOB_THETA:cpu_ref.LOB_THETA + m]), f"resid m={m} N={N}")
        assert not wg.B[cpu_ref.LOB_W].cpu().any()      # W cleared
        assert torch.equal(wg.B[0].cpu(), wc.B[0])
        assert torch.equal(wg.B[2].cpu(), wc.B[2])
        cpu_ref.cert_lob_gram(wc)
        hip.cert_lob_gram(wg)
        # abs() Gram matrices: N terms per entry; the squared norms are
        # sums of N squares of R, whose own error enters twice
        wa.R.copy_(wc.R.abs())
        wa.B.copy_(wc.B.abs())
        k = 3 * m
        Bf = wa.B.permute(1, 0, 2).reshape(N, k)
        SBf = wa.SB.permute(1, 0, 2).reshape(N, k)
        bounds = (2 * N * EPS * (Bf.T @ Bf), 2 * N * EPS * (Bf.T @ SBf))
        hg, hc = wg.out.cpu(), wc.out
        iu = torch.triu(torch.ones(k, k, dtype=torch.bool))
        for a, name in enumerate(("G_B", "G_A")):
            got = hg[a * k * k:(a + 1) * k * k].view(k, k)
            ref = hc[a * k * k:(a + 1) * k * k].view(k, k)
            _close(got[iu], ref[iu], bounds[a][iu],
                   f"{name} m={m} N={N}")
        r_abs = wa.SB[0] + wa.B[0] * wa.ctl[
            cpu_ref.LOB_THETA:cpu_ref.LOB_THETA + m]
        rn_bound = (2 * (N + 2) * EPS * (wc.R * wc.R).sum(dim=0)
                    + 2 * 2 * 2 * EPS * (wc.R.abs() * r_abs).sum(dim=0))
        _close(hg[2 * k * k:], hc[2 * k * k:], rn_bound,
               f"rn2 m={m} N={N}")
        GBg, GAg, _ = wg.unpack()
        assert np.array_equal(GBg, GBg.T) and np.array_equal(GAg, GAg.T)


@pytest.mark.parametrize("m", range(2, 9))
def test_update_in_place_matches_out_of_place(m):
    cpu_ref, hip = _backends()
    for N in (3, 195, 768, 1028, N_WRAP):
        wc, wg = _workspaces(N, m, 9)
        wa = _abs_copy(wc)
        cpu_ref.cert_lob_update(wc)          # out of place, then stored
        hip.cert_lob_update(wg)              # in place
        cpu_ref.cert_lob_update(wa)
        for T, Tc, Ta, name in ((wg.B, wc.B, wa.B, "B"),
                                (wg.SB, wc.SB, wa.SB, "SB")):
            for blk in (0, 2):
                _close(T[blk], Tc[blk], 2 * 3 * m * EPS * Ta[blk],
                       f"update {name}[{blk}] m={m} N={N}")
            assert torch.equal(T[1].cpu(), Tc[1])        # W, SW untouched


# --------------------------------------------------------------------
# 2. guards
# --------------------------------------------------------------------
@pytest.mark.parametrize("pre_mode", ["jacobi", "dense"])
def test_non_run_status_is_a_no_op(pre_mode):
    cpu_ref, hip = _backends()
    d, m, n = 3, 5, 65
    Q, lam = _bsr(n, d)
    N = n * (d + 1)
    _, wg = _workspaces(N, m, 13)
    wg.ctl[cpu_ref.LOB_STATUS] = 1.0
    wg.part.fill_(-7.0)
    wg.out.fill_(-7.0)
    before = {k: getattr(wg, k).clone()
              for k in ("B", "SB", "R", "ctl", "part", "out")}
    if pre_mode == "jacobi":
        pre = ("jacobi", torch.eye(d + 1, dtype=torch.float64, device=DEV)
               .repeat(n, 1, 1).contiguous())
    else:
        pre = ("dense", torch.eye(N, dtype=torch.float32, device=DEV))
    Qd, lamd = Q.to(DEV), lam.to(DEV)
    hip.cert_lob_resid(wg)
    hip.cert_lob_apply(Qd, lamd, wg, 1)
    hip.cert_lob_gram(wg)
    hip.cert_lob_update(wg)
    hip.cert_lob_iter(Qd, lamd, wg, pre)
    torch.cuda.synchronize()
    for k, ref in before.items():
        assert torch.equal(getattr(wg, k), ref), k


# --------------------------------------------------------------------
# 3. certify_solution on GPU tensors
# --------------------------------------------------------------------
def test_jacobi_run_is_bit_reproducible():
    _backends()
    from dpo_amd.certify import certify_solution
    meas, n, Q, _, X = grid_case()
    kw = dict(method="lobpcg", precond="jacobi")
    a = certify_solution(meas, n, 3, X.to(DEV), **kw)
    b = certify_solution(meas, n, 3, X.to(DEV), **kw)
    assert a.status == b.status and a.iterations == b.iterations
    assert a.lambda_min == b.lambda_min and a.residual == b.residual
    assert torch.equal(a.direction, b.direction)


def _case(name):
    if name == "grid":
        meas, n, Q, _, X = grid_case()
        return meas, n, 3, Q, X, {}
    meas, n, Q, X, _ = ring_case(67)
    # ring67: the lambda_max phase meets the witness; ring67_lob: it
    # cannot, and LOBPCG has to
    return meas, n, 2, Q, X, ({} if name == "ring67" else {"lmax_iters": 4})


@pytest.mark.parametrize("precond", ["dense", "jacobi"])
@pytest.mark.parametrize("name", ["grid", "ring67", "ring67_lob"])
def test_certify_lobpcg_gpu_matches_cpu(name, precond):
    _backends()
    from dpo_amd.certify import CertificateStatus, certify_solution
    meas, n, d, Q, X, extra = _case(name)
    S = dense_S(Q, X, d)
    ev = np.linalg.eigvalsh(S)
    kw = dict(method="lobpcg", precond=precond, **extra)
    ref = certify_solution(meas, n, d, X, **kw)
    res = certify_solution(meas, n, d, X.to(DEV), **kw)
    print(f"{name} {precond}: cpu {ref.status} {ref.lambda_min!r} res "
          f"{ref.residual!r} it {ref.iterations}; gpu {res.status} "
          f"{res.lambda_min!r} res {res.residual!r} it {res.iterations} "
          f"apps {res.applications} drops {res.basis_drops}")
    assert res.status == ref.status
    assert res.precond == precond or res.iterations == 0
    assert abs(res.lambda_min - ev[0]) <= max(res.residual, ref.residual)
    v = res.direction.cpu().numpy()
    assert res.direction.device.type == "cuda"
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-12
    if name == "grid":
        assert res.status == CertificateStatus.CERTIFIED
        assert 1 <= res.iterations <= 40
    else:
        assert res.status == CertificateStatus.NOT_OPTIMAL
        # the largest eta the run can have used: 1e-6 ||S||_inf
        assert v @ S @ v < -1e-6 * float(np.abs(S).sum(axis=1).max())
        if name == "ring67_lob":
            assert res.iterations >= 1
