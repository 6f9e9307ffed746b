"""Kernel test matrix: every compiled (d, r) shape, block edges, guards,
the tCG vector ops and the scalar control kernels, each against a plain
fp64 CPU reference under a derived bound (tests/kernel_refs.py; the
rule is written down in docs/DESIGN.md, "Kernel test matrix").

Pose counts: thread-per-pose kernels run n in {1, 65, 256, 257};
tile-per-pose kernels run n in {1, PB, PB + 1, 3 PB + 1, 257} with
PB = 256 // ((d + 1) r), which for r = 6 and r = 7 (d = 3) leaves a dead
thread tail inside every block.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_refs as kr
from dpo_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = kr.EPS
SENTINEL = -7.25e77
TOTALS = (1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 2 + 1)


def _hb():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import hip_backend
    assert hip_backend.CTRL_SIZE == kr.CTRL_SIZE
    assert hip_backend.MAX_TCG == kr.MAX_TCG
    for name in ("C_STATUS", "C_RR", "C_ZR", "C_EPE", "C_EPD", "C_DPD",
                 "C_COEF", "C_BETA", "C_ITER", "C_J", "C_RADIUS", "C_DM",
                 "C_JSTAR", "C_TAUSTAR", "C_USE_CURRENT", "C_STOP_PENDING",
                 "C_BOUND", "C_HLEN", "C_SHRINKS", "C_DOT0", "C_DOT1",
                 "C_DOT2", "C_DOT3", "C_HIST"):
        assert getattr(hip_backend, name) == getattr(kr, name), name
    return hip_backend


def _dev(t):
    return t.contiguous().to(DEV)


def _nan_like(t):
    return torch.full_like(t, float("nan"), device=DEV)


def _assert_close(out, ref, bound, label):
    """|out - ref| <= bound entry-wise (NaN fails); prints the margin."""
    out = torch.as_tensor(out, dtype=torch.float64)
    ref = torch.as_tensor(ref, dtype=torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    diff = (out - ref).abs()
    ok = diff <= bound
    if not bool(ok.all()):
        bad = (~ok).flatten().nonzero()[:, 0]
        i = int(bad[0])
        raise AssertionError(
            f"{label}: {bad.numel()} of {ref.numel()} entries outside the "
            f"bound; first flat index {i}: got {out.flatten()[i]!r}, "
            f"ref {ref.flatten()[i]!r}, bound {bound.flatten()[i]!r}")
    worst = float((diff / bound.clamp_min(1e-300)).max()) if ref.numel() else 0
    print(f"{label}: max |err| {float(diff.max()):.3e}, "
          f"max bound {float(bound.max()):.3e}, worst err/bound {worst:.3f}")


def _marker_ctrl():
    """Host ctrl block with a distinct finite value in every slot."""
    return np.arange(kr.CTRL_SIZE, dtype=np.float64) * 0.375 + 11.0


def _ctrl_dev(c):
    return torch.from_numpy(np.asarray(c, dtype=np.float64).copy()).to(DEV)


def _assert_ctrl_unchanged(ctrl_dev, before, except_slots=(), label=""):
    after = ctrl_dev.cpu().numpy()
    keep = np.ones(kr.CTRL_SIZE, dtype=bool)
    keep[list(except_slots)] = False
    same = after.view(np.int64) == np.asarray(before).view(np.int64)
    assert same[keep].all(), (
        f"{label}: ctrl slots {np.nonzero(~same & keep)[0].tolist()} changed")
    return after


# ---------------------------------------------------------------------
# A.1 BSR SpMM
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", kr.SHAPES + [(3, 9)])
def test_bsr_spmm(d, r):
    """Q @ V against the dense fp64 product. (3, 9) is not a compiled
    shape: it takes the generic kernel (tile 36, 7 poses per block)."""
    hb = _hb()
    dh = d + 1
    ns = kr.n_tile(d, r) if (d, r) in kr.SHAPES else (1, 8, 50)
    for n in ns:
        g = kr.gen(11, d, r, n)
        Q = kr.random_bsr(n, dh, g)
        V = kr.randn(g, dh * n, r)
        Qd = Q.to_dense()
        ref = Qd @ V
        bound = kr.matmul_bound(Qd, V, kr.bsr_max_row_terms(Q))
        assert float(bound.max()) < 1e-10     # a whole term is ~1
        out = _nan_like(V)
        hb.bsr_spmm(_dev(Q.row_ptr), _dev(Q.col_idx), _dev(Q.vals), n, dh,
                    _dev(V), out=out)
        _assert_close(out.cpu(), ref, bound, f"bsr_spmm d={d} r={r} n={n}")


# ---------------------------------------------------------------------
# A.2 fused projection + dots, called directly
# ---------------------------------------------------------------------
def _proj_dots_raw(hb, X, V, G, out, dotWith, ctrl, n, d, r, slot, slot2,
                   guard=-1):
    hb._lib.dpo_proj_dots(hb._p(X), hb._p(V), hb._p(G), hb._p(out),
                          hb._p(dotWith), hb._p(ctrl), n, d, r, slot, slot2,
                          0, guard, hb._stream(X))


def check_proj_dots(hb, d, r, n):
    """dpo_proj_dots with G, both dot slots, dotWith given and null."""
    g = kr.gen(12, d, r, n)
    N = (d + 1) * n
    X = kr.manifold_point(n, d, r, g)
    V, G, W = kr.randn(g, N, r), kr.randn(g, N, r), kr.randn(g, N, r)
    A = V + G
    P = cpu_ref.tangent_project(X, A, d)
    bP = kr.tangent_project_bound(X, A, d)
    T = A.numel()
    dot2 = float((A * X).sum())
    b2 = kr.dot_bound(A, X)
    for with_w in (True, False):
        label = f"proj_dots d={d} r={r} n={n} dotWith={with_w}"
        other = W if with_w else P
        dot1 = float((P * other).sum())
        b1 = float(kr.sop_bound((P.abs() * other.abs()).sum(), T))
        b1 += float((bP * other.abs()).sum())
        if not with_w:
            b1 += float((bP * (P.abs() + bP)).sum())
        before = _marker_ctrl()
        before[kr.C_DOT0] = 0.0
        before[kr.C_DOT2] = 0.0
        ctrl = _ctrl_dev(before)
        out = _nan_like(V)
        _proj_dots_raw(hb, _dev(X), _dev(V), _dev(G), out,
                       _dev(W) if with_w else None, ctrl, n, d, r,
                       kr.C_DOT0, kr.C_DOT2)
        _assert_close(out.cpu(), P, bP, label + " out")
        after = _assert_ctrl_unchanged(ctrl, before,
                                       (kr.C_DOT0, kr.C_DOT2), label)
        _assert_close(after[kr.C_DOT0], dot1, b1, label + " <P,W>")
        _assert_close(after[kr.C_DOT2], dot2, b2, label + " <V+G,X>")


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_proj_dots(d, r):
    hb = _hb()
    for n in kr.N_POSE:
        check_proj_dots(hb, d, r, n)


# ---------------------------------------------------------------------
# A.3 polar projection of an affine combination
# ---------------------------------------------------------------------
def _check_polar(out, A, B, C, ca, cb, cc, d, label):
    M = kr.affine(A, B, C, ca, cb, cc)
    r = M.shape[1]
    err, orth = kr.polar_errors(out, M, d)
    tol = kr.polar_tol(kr.block_conds(M, d))
    print(f"{label}: max err/tol {np.max(err / tol):.3f}, "
          f"max orth/tol {np.max(orth / tol):.3f}, max tol {tol.max():.2e}")
    assert not np.isnan(err).any() and not np.isnan(orth).any(), label
    assert (err <= tol).all(), (label, float(np.max(err / tol)))
    assert (orth <= tol).all(), (label, float(np.max(orth / tol)))
    # translation rows: the affine combination itself. 4 eps relative to
    # |ca A| + |cb B| + |cc C| covers its three roundings in any order,
    # fused or not.
    mag = kr.affine(A.abs(), None if B is None else B.abs(),
                    None if C is None else C.abs(),
                    abs(ca), abs(cb), abs(cc))
    ot = out.view(-1, d + 1, r)[:, d, :]
    _assert_close(ot, M.view(-1, d + 1, r)[:, d, :],
                  4.0 * EPS * mag.view(-1, d + 1, r)[:, d, :],
                  label + " translation")


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_polar_affine_forms(d, r):
    """1-operand (stiefel_project), 2-operand (retract) and 3-operand
    (1.7 A - 0.7 B + 0.3 C) forms against the SVD polar factor."""
    hb = _hb()
    for n in kr.N_POSE:
        forms = kr.polar_form_inputs(d, r, n)
        A, B, C, ca, cb, cc = forms["one"]
        out = hb.stiefel_project(_dev(A), d).cpu()
        _check_polar(out, A, B, C, ca, cb, cc, d, f"polar one {d},{r} n={n}")
        A, B, C, ca, cb, cc = forms["two"]
        out = hb.retract(_dev(A), _dev(B), d).cpu()
        _check_polar(out, A, B, C, ca, cb, cc, d, f"polar two {d},{r} n={n}")
        A, B, C, ca, cb, cc = forms["three"]
        out = hb.polar_affine(_dev(A), _dev(B), _dev(C), ca, cb, cc, d).cpu()
        _check_polar(out, A, B, C, ca, cb, cc, d,
                     f"polar three {d},{r} n={n}")


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_polar_conditioning(d, r):
    """Blocks with cond(M) in {1, 1e2, 1e4} at scales {1e-3, 1, 1e3}:
    inside the stated domain, so within 8 eps cond^2 + 16 eps."""
    hb = _hb()
    for label, cond, M in kr.polar_cond_cases(d, r):
        out = hb.stiefel_project(_dev(M), d).cpu()
        _check_polar(out, M, None, None, 1.0, 0.0, 0.0, d,
                     f"polar {d},{r} {label}")


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_polar_retraction_step_lengths(d, r):
    """X + eta with tangent eta, ||eta|| from 1e-8 to 1e2 per pose."""
    hb = _hb()
    for label, cbound, X, eta in kr.polar_retract_cases(d, r):
        out = hb.retract(_dev(X), _dev(eta), d).cpu()
        _check_polar(out, X, eta, None, 1.0, 1.0, 0.0, d,
                     f"retract {d},{r} {label}")


# ---------------------------------------------------------------------
# A.4 block-Jacobi apply
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_precond_jacobi(d, r):
    """Per-pose (L L^T) z = v against torch.cholesky_solve, blocks with
    condition numbers 1, 1e3 and 1e6."""
    hb = _hb()
    dh = d + 1
    for n in kr.N_POSE:
        g = kr.gen(14, d, r, n)
        A = kr.spd_blocks(n, dh, g)
        V = kr.randn(g, n * dh, r)
        L = torch.linalg.cholesky(A).contiguous()
        ref = torch.cholesky_solve(V.view(n, dh, r), L).reshape(-1, r)
        out = _nan_like(V)
        hb.precond_jacobi(_dev(L), _dev(V), dh, out=out)
        _assert_close(out.cpu(), ref, kr.jacobi_tol(A, V),
                      f"jacobi dh={dh} r={r} n={n}")


# ---------------------------------------------------------------------
# A.5 dense fp32 preconditioner apply
# ---------------------------------------------------------------------
# N = (d + 1) n for d in {2, 3} and the pose list, plus N = 2400, where
# the 32-way j split has jchunk = 75: one full 64-row tile and one of 11.
# Not covered: the jsplit == 1 store path (no atomics) needs
# ceil(N / 256) >= 512, i.e. N >= 130 817 — a 68 GB fp32 matrix.
DENSE_N = (3, 4, 195, 260, 768, 771, 1024, 1028, 2400)


def check_precond_dense(hb, N, r, label):
    gd = torch.Generator(device=DEV).manual_seed(1000 * N + r)
    Md = torch.randn(N, N, dtype=torch.float32, device=DEV, generator=gd)
    Md = (0.5 * (Md + Md.T)).contiguous()
    V = kr.randn(kr.gen(15, N, r), N, r)
    M64 = Md.cpu().double()
    ref = M64 @ V
    out = _nan_like(V)
    hb.precond_dense(Md, _dev(V), out=out)
    _assert_close(out.cpu(), ref, kr.matmul_bound(M64, V, N), label)


@pytest.mark.parametrize("r", kr.RS)
def test_precond_dense(r):
    hb = _hb()
    for N in DENSE_N:
        check_precond_dense(hb, N, r, f"precond_dense r={r} N={N}")


# ---------------------------------------------------------------------
# A.6 scatter-add assembly
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_g_assemble(d, r):
    """Gt[pose] += -w E0 @ nbr[slot] with at least 40 edges into one
    pose, exact-zero weights and one pose that receives nothing."""
    hb = _hb()
    dh = d + 1
    n0, nslots, heavy, empty = 8, 6, 2, 5
    for ne in (1, 255, 257):
        g = kr.gen(16, d, r, ne)
        pose = torch.randint(0, n0 - 1, (ne,), generator=g)
        pose[pose >= empty] += 1                 # never the empty pose
        pose[:min(ne, 48)] = heavy
        slot = torch.randint(0, nslots, (ne,), generator=g)
        E0 = kr.randn(g, ne, dh, dh)
        nbr = kr.randn(g, nslots, dh, r)
        w = torch.rand(ne, dtype=torch.float64, generator=g)
        w[3::4] = 0.0
        contrib = -torch.bmm(E0 * w[:, None, None], nbr[slot])
        mag = torch.bmm(E0.abs() * w[:, None, None], nbr[slot].abs())
        ref = torch.zeros(n0, dh, r, dtype=torch.float64)
        ref.index_add_(0, pose, contrib)
        S = torch.zeros(n0, dh, r, dtype=torch.float64)
        S.index_add_(0, pose, mag)
        K = (dh + 1) * int(torch.bincount(pose, minlength=n0).max())
        Gt = torch.full((n0 * dh, r), SENTINEL, dtype=torch.float64,
                        device=DEV)
        hb.g_assemble(Gt, _dev(E0), _dev(pose), _dev(slot), _dev(nbr),
                      _dev(w), dh, r)
        out = Gt.cpu().view(n0, dh, r)
        _assert_close(out, ref, kr.sop_bound(S, K),
                      f"g_assemble d={d} r={r} ne={ne}")
        assert torch.equal(out[empty], torch.zeros(dh, r,
                                                   dtype=torch.float64))


@pytest.mark.parametrize("dh", [3, 4])
def test_q_assemble(dh):
    """vals[slot] += w[edge] * block with at least 40 contributions into
    one slot, exact-zero weights and one slot that receives nothing."""
    hb = _hb()
    nnzb, new, heavy, empty = 7, 50, 3, 5
    for nc in (1, 255, 257):
        g = kr.gen(17, dh, nc)
        slot = torch.randint(0, nnzb - 1, (nc,), generator=g)
        slot[slot >= empty] += 1
        slot[:min(nc, 48)] = heavy
        edge = torch.randint(0, new, (nc,), generator=g)
        blocks = kr.randn(g, nc, dh, dh)
        w = torch.rand(new, dtype=torch.float64, generator=g)
        w[::3] = 0.0
        ref = torch.zeros(nnzb, dh, dh, dtype=torch.float64)
        ref.index_add_(0, slot, blocks * w[edge][:, None, None])
        S = torch.zeros(nnzb, dh, dh, dtype=torch.float64)
        S.index_add_(0, slot, blocks.abs() * w[edge][:, None, None])
        K = 2 * int(torch.bincount(slot, minlength=nnzb).max())
        vals = torch.full((nnzb, dh, dh), SENTINEL, dtype=torch.float64,
                          device=DEV)
        hb.q_assemble(vals, _dev(blocks), _dev(slot), _dev(edge), _dev(w),
                      dh)
        out = vals.cpu()
        _assert_close(out, ref, kr.sop_bound(S, K),
                      f"q_assemble dh={dh} ncontrib={nc}")
        assert torch.equal(out[empty], torch.zeros(dh, dh,
                                                   dtype=torch.float64))


# ---------------------------------------------------------------------
# A.7 GNC-TLS weights
# ---------------------------------------------------------------------
@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_gnc_weights(d, r):
    """Residual from the kernel's header formula in NumPy, weight from
    robust.py. Residuals planted at 0.5 lower, sqrt(lower upper) and
    2 upper; endpoints mix local poses and the neighbour buffer; widx is
    a non-identity permutation into a larger weight array; masked-out and
    unnamed weights must stay bit-identical."""
    hb = _hb()
    dh = d + 1
    nloc, nnbr, barc = 9, 7, 10.0
    for ne in (1, 256, 257):
        for mi, mu in enumerate((1e-2, 1.0, 1e4)):
            g = kr.gen(18, d, r, ne, mi)
            X = kr.manifold_point(nloc, d, r, g)
            NB = kr.manifold_point(nnbr, d, r, g)
            e1n = torch.randint(0, 2, (ne,), generator=g).to(torch.uint8)
            e2n = torch.randint(0, 2, (ne,), generator=g).to(torch.uint8)
            e1 = torch.where(e1n.bool(),
                             torch.randint(0, nnbr, (ne,), generator=g),
                             torch.randint(0, nloc, (ne,), generator=g))
            e2 = torch.where(e2n.bool(),
                             torch.randint(0, nnbr, (ne,), generator=g),
                             torch.randint(0, nloc, (ne,), generator=g))
            R = torch.linalg.qr(kr.randn(g, ne, d, d))[0].contiguous()
            t = kr.randn(g, ne, d)
            Xb, Nb = X.view(nloc, dh, r), NB.view(nnbr, dh, r)
            P1 = torch.where(e1n.bool()[:, None, None], Nb[e1 % nnbr],
                             Xb[e1 % nloc]).numpy()
            P2 = torch.where(e2n.bool()[:, None, None], Nb[e2 % nnbr],
                             Xb[e2 % nloc]).numpy()
            one = np.ones(ne)
            base = kr.gnc_residual_sq(P1, P2, R.numpy(), t.numpy(), one,
                                      one, d)
            assert base.min() > 1e-3
            lower = mu / (mu + 1.0) * barc ** 2
            upper = (mu + 1.0) / mu * barc ** 2
            target = np.array([0.5 * lower, math.sqrt(lower * upper),
                               2.0 * upper])[np.arange(ne) % 3]
            kappa = target / base
            r_sq = kr.gnc_residual_sq(P1, P2, R.numpy(), t.numpy(), kappa,
                                      kappa, d)
            ref = kr.gnc_weight_ref(r_sq, mu, barc)
            nw = ne + 5
            widx = torch.randperm(nw, generator=g)[:ne]
            if ne == 1:
                widx[0] = 3
            assert not torch.equal(widx, torch.arange(ne))
            upd = (torch.rand(ne, generator=g) > 1.0 / 3.0).to(torch.uint8)
            upd[0] = 1
            w0 = 0.25 + 0.5 * torch.rand(nw, dtype=torch.float64,
                                         generator=g)
            wd = _dev(w0)
            gd = {"e1_idx": _dev(e1), "e1_nbr": _dev(e1n),
                  "e2_idx": _dev(e2), "e2_nbr": _dev(e2n), "R": _dev(R),
                  "t": _dev(t), "kappa": _dev(torch.from_numpy(kappa)),
                  "tau": _dev(torch.from_numpy(kappa)), "upd": _dev(upd),
                  "widx": _dev(widx), "ne": ne}
            hb.gnc_weights(_dev(X), _dev(NB), gd, wd, d, r, mu, barc ** 2)
            w1 = wd.cpu()
            label = f"gnc d={d} r={r} ne={ne} mu={mu:g}"
            m = upd.bool()
            _assert_close(w1[widx[m]], torch.from_numpy(ref)[m],
                          kr.gnc_tol(mu), label)
            keep = torch.ones(nw, dtype=torch.bool)
            keep[widx[m]] = False
            assert torch.equal(w1[keep], w0[keep]), label
            # the planted regimes really are the three branches
            assert (ref[np.arange(ne) % 3 == 0] == 1.0).all()
            assert (ref[np.arange(ne) % 3 == 2] == 0.0).all()
            mid = ref[np.arange(ne) % 3 == 1]
            assert ((mid > 0.0) & (mid < 1.0)).all()


# ---------------------------------------------------------------------
# B. fused kernels through DeviceSolver
# ---------------------------------------------------------------------
def _device_problem(p):
    from dpo_amd.quadratic import QuadraticProblem
    pd = QuadraticProblem(p.n, p.d, p.r, precond="jacobi")
    pd.set_q(p.Q.to(DEV))
    pd._Lpre = pd._Lpre.contiguous()
    if p.Gt is not None:
        pd.set_g(_dev(p.Gt))
    return pd


def check_eval_terms(hb, d, r, n):
    """[f, 0.5 <X, G>, ||rgrad||^2] from the fused Hessian kernel (MODE 0,
    three dot slots, multi-block fan-in) against the CPU problem."""
    p, X = kr.small_problem(d, r, n, kr.gen(19, d, r, n), with_g=True)
    ref, bound, _, _ = kr.eval_terms_ref(p, X)
    pd = _device_problem(p)
    ds = hb.DeviceSolver(n, d, r, DEV, max_inner=10)
    Xd = _dev(X)
    for rep in range(2):     # the second call checks the slots self-clean
        out = ds.eval_terms(pd, Xd).cpu().numpy()
        _assert_close(out, ref, bound,
                      f"eval_terms d={d} r={r} n={n} call {rep}")


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_eval_terms(d, r):
    hb = _hb()
    for n in (1, 65, 257):
        check_eval_terms(hb, d, r, n)


INTERIOR_RADII = (1e4, 1e5, 1e6)
BOUNDARY_RADII = (1.0, 0.1, 10.0)


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_local_solve_matches_host(d, r):
    """One device local solve per tCG outcome against the host optimizer
    (Jacobi preconditioner, max_inner = 10) on a two-block problem: one
    radius at which the host's tCG converges in the interior and one at
    which it is truncated at the boundary, each classified on the host
    first."""
    hb = _hb()
    p, X = kr.solve_problem(d, r)
    assert 257 <= p.n <= 350
    pd = _device_problem(p)
    hosts = {}
    for want, radii in (("converged", INTERIOR_RADII),
                        ("exceeded_tr", BOUNDARY_RADII)):
        for Delta0 in radii:
            Xh, res, runs, iters = kr.host_solve(p, X, 1e-2, Delta0, 10)
            if res.tcg_status == want and runs == 1:
                hosts[want] = (Delta0, Xh, res, iters)
                break
        assert want in hosts, f"no radius gives a host {want} solve"
    for want, (Delta0, Xh, res, iters) in hosts.items():
        label = f"solve d={d} r={r} {want} Delta0={Delta0:g}"
        ds = hb.DeviceSolver(p.n, d, r, DEV, max_inner=10)
        Xd = _dev(X.clone())
        st = ds.solve(pd, Xd, tol=1e-2, Delta0=Delta0)
        hlen = int(ds._stats[7])
        print(label, st, "hlen", hlen, "host iters", iters,
              "host f_opt", res.f_opt, "gn_opt", res.grad_norm_opt,
              "max|dX|", float((Xd.cpu() - Xh).abs().max()))
        assert st["status"] == hb.ST_ACCEPTED, label
        assert st["shrinks"] == 0 and hlen == iters, label
        assert abs(st["f_init"] - res.f_init) < 1e-6 * max(
            1, abs(res.f_init)), label
        assert abs(st["grad_norm_init"] - res.grad_norm_init) < 1e-6, label
        assert abs(st["f_opt"] - res.f_opt) < 1e-5 * max(
            1, abs(res.f_opt)), label
        assert abs(st["grad_norm_opt"] - res.grad_norm_opt) < 1e-6, label
        assert torch.allclose(Xd.cpu(), Xh, atol=1e-6, rtol=0), label


@pytest.mark.parametrize("d,r,Delta0,max_shrink", kr.SHRINK_CASES)
def test_shrink_loop_matches_model(d, r, Delta0, max_shrink):
    """The batched device shrink loop against kr.model_solve on a solve
    that rejects every candidate (accept_rho = 2): all max_shrink attempts
    run, the host reads the last one. The status, the shrink count and
    the history length are exact, X is untouched, and rho — which differs
    from attempt to attempt by far more than its bound (checked on the
    CPU in test_kernel_refs) — is the last attempt's."""
    hb = _hb()
    p, X, c, status, attempts, b_rho = kr.shrink_case_ref(d, r, Delta0,
                                                          max_shrink)
    assert status == kr.ST_GIVE_UP and len(attempts) == max_shrink + 1
    ds = hb.DeviceSolver(p.n, d, r, DEV, max_inner=10)
    Xd = _dev(X.clone())
    st = ds.solve(_device_problem(p), Xd, tol=1e-2, Delta0=Delta0,
                  max_shrink=max_shrink, accept_rho=kr.SHRINK_ACCEPT_RHO,
                  compute_final_gradnorm=False)
    label = f"shrink d={d} r={r} Delta0={Delta0:g} max_shrink={max_shrink}"
    print(label, st, "hlen", ds._stats[7], "model rho", c[kr.C_RHO],
          "|drho|", abs(st["rho"] - c[kr.C_RHO]), "bound", b_rho)
    assert st["status"] == hb.ST_GIVE_UP, label
    assert st["shrinks"] == max_shrink, label
    assert ds._stats[7] == c[kr.C_HLEN], label
    assert torch.equal(Xd.cpu(), X), label
    assert abs(st["rho"] - c[kr.C_RHO]) <= b_rho, label


def run_wide_child():
    """Body of the DPO_HESS_WIDE=1 child process: eval_terms and
    proj_dots through the element-per-thread kernels, each against the
    CPU reference; exits non-zero on the first mismatch, naming it."""
    hb = _hb()
    done = 0
    case = None
    try:
        for d, r in kr.SHAPES:
            pb = kr.poses_per_block(d, r)
            for n in sorted({1, pb, pb + 1, 3 * pb + 1}):
                case = f"eval_terms d={d} r={r} n={n}"
                check_eval_terms(hb, d, r, n)
                case = f"proj_dots d={d} r={r} n={n}"
                check_proj_dots(hb, d, r, n)
                done += 2
    except AssertionError as e:
        print(json.dumps({"ok": False, "case": case, "error": str(e)}))
        sys.exit(1)
    print(json.dumps({"ok": True, "cases": done}))


def test_wide_kernels_match_cpu():
    """k_hess_wide / k_proj_wide for every shape at n in {1, PB, PB + 1,
    3 PB + 1}. A child process, because the path choice is read from the
    environment once per process."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            f"sys.path.insert(0, {here!r})\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r})\n"
            "import test_kernel_matrix as t\n"
            "t.run_wide_child()\n")
    env = dict(os.environ, DPO_HESS_WIDE="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, env=env, cwd=os.path.dirname(here),
                       timeout=300)
    lines = p.stdout.strip().splitlines()
    assert lines, p.stderr[-2000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res["ok"], (res, p.stderr[-2000:])
    assert res["cases"] == 2 * sum(
        len({1, pb, pb + 1, 3 * pb + 1})
        for pb in (kr.poses_per_block(d, r) for d, r in kr.SHAPES))


# ---------------------------------------------------------------------
# C. tCG vector ops
# ---------------------------------------------------------------------
def _base_ctrl(status):
    c = _marker_ctrl()
    c[kr.C_STATUS] = status
    return c


@pytest.mark.parametrize("total", TOTALS)
def test_tcg_update(total):
    """Four elements per thread: totals around the unroll and the block
    size. C_ITER = 0 must not read the old eta (pre-filled with NaN)."""
    hb = _hb()
    rows, coef, dot1_0 = 4, 0.37, 0.5
    for j in (0, 2):
        for stop in (0, 1):
            label = f"tcg_update total={total} iter={j} stop={stop}"
            g = kr.gen(20, total, j, stop)
            eta = kr.randn(g, total)
            rv, dl, Hd = (kr.randn(g, total), kr.randn(g, total),
                          kr.randn(g, total))
            if j == 0:
                eta = torch.full((total,), float("nan"),
                                 dtype=torch.float64)
            before = _base_ctrl(kr.ST_RUN)
            before[kr.C_COEF] = coef
            before[kr.C_ITER] = j
            before[kr.C_STOP_PENDING] = stop
            before[kr.C_DOT1] = dot1_0
            ctrl = _ctrl_dev(before)
            snap0 = torch.full((rows, total), SENTINEL, dtype=torch.float64)
            eta_d, rv_d = _dev(eta), _dev(rv)
            es, dsn = _dev(snap0), _dev(snap0)
            hb.tcg_update(eta_d, rv_d, _dev(dl), _dev(Hd), es, dsn, ctrl)
            e_old = torch.zeros(total, dtype=torch.float64) if j == 0 \
                else eta
            _assert_close(eta_d.cpu(), e_old + coef * dl,
                          2 * EPS * (e_old.abs() + coef * dl.abs()),
                          label + " eta")
            es, dsn = es.cpu(), dsn.cpu()
            assert torch.equal(es[j], e_old), label + " eta snapshot"
            assert torch.equal(dsn[j], dl), label + " delta snapshot"
            others = [k for k in range(rows) if k != j]
            assert torch.equal(es[others], snap0[others]), label
            assert torch.equal(dsn[others], snap0[others]), label
            if stop:
                assert torch.equal(rv_d.cpu(), rv), label + " r touched"
                _assert_ctrl_unchanged(ctrl, before, (), label)
            else:
                rn = rv + coef * Hd
                brn = 2 * EPS * (rv.abs() + coef * Hd.abs())
                _assert_close(rv_d.cpu(), rn, brn, label + " r")
                after = _assert_ctrl_unchanged(ctrl, before, (kr.C_DOT1,),
                                               label)
                rr = float((rn * rn).sum())
                b = float((2 * rn.abs() * brn + brn * brn).sum()) \
                    + kr.dot_bound(rn, rn) + 2 * EPS * (dot1_0 + rr)
                _assert_close(after[kr.C_DOT1], dot1_0 + rr, b,
                              label + " C_DOT1")


@pytest.mark.parametrize("total", TOTALS)
def test_tcg_delta_form_step_axpby_dots(total):
    hb = _hb()
    g = kr.gen(21, total)
    # delta = -z + beta * delta
    dl, z = kr.randn(g, total), kr.randn(g, total)
    before = _base_ctrl(kr.ST_RUN)
    before[kr.C_BETA] = beta = 0.625
    ctrl = _ctrl_dev(before)
    dd = _dev(dl)
    hb.tcg_delta(dd, _dev(z), ctrl)
    _assert_close(dd.cpu(), beta * dl - z,
                  2 * EPS * (beta * dl.abs() + z.abs()),
                  f"tcg_delta total={total}")
    _assert_ctrl_unchanged(ctrl, before, (), "tcg_delta")
    # step = eta, or snapshot row jstar of eta + tau * that row of delta
    rows, tau = 5, -1.75
    eta = kr.randn(g, total)
    es, dsn = kr.randn(g, rows, total), kr.randn(g, rows, total)
    for use_current in (0, 1):
        for jstar in (0, 3):
            label = f"form_step total={total} cur={use_current} j={jstar}"
            before = _base_ctrl(kr.ST_TCG_STOP)
            before[kr.C_USE_CURRENT] = use_current
            before[kr.C_JSTAR] = jstar
            before[kr.C_TAUSTAR] = tau
            ctrl = _ctrl_dev(before)
            step = torch.full((total,), SENTINEL, dtype=torch.float64,
                              device=DEV)
            hb.form_step(step, _dev(eta), _dev(es), _dev(dsn), ctrl)
            if use_current:
                assert torch.equal(step.cpu(), eta), label
            else:
                _assert_close(step.cpu(), es[jstar] + tau * dsn[jstar],
                              2 * EPS * (es[jstar].abs()
                                         + abs(tau) * dsn[jstar].abs()),
                              label)
            _assert_ctrl_unchanged(ctrl, before, (), label)
    # out = a A + b B
    A, B = kr.randn(g, total), kr.randn(g, total)
    a, b = 1.3, -0.45
    out = hb.axpby(_dev(A), _dev(B), a, b, out=_nan_like(A))
    _assert_close(out.cpu(), a * A + b * B,
                  2 * EPS * (abs(a) * A.abs() + abs(b) * B.abs()),
                  f"axpby total={total}")
    out = hb.axpby(_dev(A), None, a, b, out=_nan_like(A))
    assert torch.equal(out.cpu(), a * A), f"axpby no B total={total}"
    # dots
    C = kr.randn(g, total)
    s0, s2 = 0.75, -1.5
    for two in (False, True):
        label = f"dots total={total} two={two}"
        before = _marker_ctrl()
        before[kr.C_DOT0], before[kr.C_DOT2] = s0, s2
        ctrl = _ctrl_dev(before)
        hb.dots(_dev(A), _dev(B), _dev(C) if two else None, ctrl,
                kr.C_DOT0, kr.C_DOT2 if two else -1)
        touched = (kr.C_DOT0, kr.C_DOT2) if two else (kr.C_DOT0,)
        after = _assert_ctrl_unchanged(ctrl, before, touched, label)
        ab = float((A * B).sum())
        _assert_close(after[kr.C_DOT0], s0 + ab,
                      kr.dot_bound(A, B) + 2 * EPS * (abs(s0) + abs(ab)),
                      label + " <A,B>")
        if two:
            ac = float((A * C).sum())
            _assert_close(after[kr.C_DOT2], s2 + ac,
                          kr.dot_bound(A, C) + 2 * EPS * (abs(s2) + abs(ac)),
                          label + " <A,C>")


def test_guard_mismatch_touches_nothing():
    """Every guarded kernel launched with a guard that does not match
    ctrl[C_STATUS]: sentinel-filled outputs and the whole control block
    must come back bit-identical."""
    hb = _hb()
    d, r, n = 3, 5, 257
    dh = d + 1
    N = dh * n
    total = N * r
    g = kr.gen(22)
    X = _dev(kr.manifold_point(n, d, r, g))
    V = _dev(kr.randn(g, N, r))
    Q = kr.random_bsr(n, dh, g)
    L = _dev(torch.linalg.cholesky(kr.spd_blocks(n, dh, g)))
    Minv = torch.randn(N, N, dtype=torch.float32, device=DEV)

    def sentinel(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float64, device=DEV)

    def run(name, status, launch, outs):
        before = _base_ctrl(status)
        ctrl = _ctrl_dev(before)
        snaps = [o.clone() for o in outs]
        launch(ctrl)
        torch.cuda.synchronize()
        for k, (o, s) in enumerate(zip(outs, snaps)):
            assert torch.equal(o.cpu().view(torch.int64),
                               s.cpu().view(torch.int64)), (name, k)
        _assert_ctrl_unchanged(ctrl, before, (), name)

    out = sentinel(N, r)
    run("bsr_spmm", kr.ST_TCG_STOP, lambda c: hb.bsr_spmm(
        _dev(Q.row_ptr), _dev(Q.col_idx), _dev(Q.vals), n, dh, V, out=out,
        ctrl=c, guard=hb.GUARD_RUN), [out])
    out = sentinel(N, r)
    run("proj_dots", kr.ST_TCG_STOP, lambda c: _proj_dots_raw(
        hb, X, V, None, out, None, c, n, d, r, kr.C_DOT0, kr.C_DOT2,
        guard=hb.GUARD_RUN), [out])
    out = sentinel(N, r)
    run("polar_affine", kr.ST_RUN, lambda c: hb._lib.dpo_polar_affine(
        hb._p(X), hb._p(V), None, 1.0, 1.0, 0.0, hb._p(out), n, d, r,
        hb._p(c), hb.GUARD_STOP, hb._stream(X)), [out])
    out = sentinel(N, r)
    run("precond_jacobi", kr.ST_TCG_STOP, lambda c: hb.precond_jacobi(
        L, V, dh, out=out, ctrl=c, guard=hb.GUARD_RUN), [out])
    # the dense apply clears its output for the j-split partial sums in
    # an unguarded helper launch before the guarded kernel: the contract
    # is that the guarded kernel adds nothing, so the output is all zero
    before = _base_ctrl(kr.ST_TCG_STOP)
    ctrl = _ctrl_dev(before)
    out = sentinel(N, r)
    hb.precond_dense(Minv, V, out=out, ctrl=ctrl, guard=hb.GUARD_RUN)
    assert torch.equal(out.cpu(), torch.zeros(N, r, dtype=torch.float64))
    _assert_ctrl_unchanged(ctrl, before, (), "precond_dense")

    vecs = [sentinel(total) for _ in range(4)]
    es, dsn = sentinel(3, total), sentinel(3, total)
    run("tcg_update", kr.ST_ACCEPTED, lambda c: hb.tcg_update(
        vecs[0], vecs[1], vecs[2], vecs[3], es, dsn, c),
        vecs + [es, dsn])
    dl = sentinel(total)
    run("tcg_delta", kr.ST_TCG_STOP, lambda c: hb.tcg_delta(
        dl, vecs[0], c), [dl])
    step = sentinel(total)
    run("form_step", kr.ST_RUN, lambda c: hb.form_step(
        step, vecs[0], es, dsn, c), [step])
    a, b = _dev(kr.randn(g, total)), _dev(kr.randn(g, total))
    run("dots", kr.ST_TCG_STOP, lambda c: hb.dots(
        a, b, b, c, kr.C_DOT0, kr.C_DOT2, guard=hb.GUARD_RUN), [])


# ---------------------------------------------------------------------
# D. scalar control kernels against the Python model
# ---------------------------------------------------------------------
def _run_ctrl(hb, name, c0, *args):
    """Launch dpo_ctrl_<name> on a copy of c0; return (device, model)."""
    ctrl = _ctrl_dev(c0)
    getattr(hb._lib, "dpo_ctrl_" + name)(hb._p(ctrl), *args,
                                         hb._stream(ctrl))
    m = kr.CtrlModel(c0)
    getattr(m, name)(*args)
    return ctrl.cpu().numpy(), m.c


def _check_ctrl(hb, name, c0, *args, label=""):
    got, want = _run_ctrl(hb, name, c0, *args)
    label = f"ctrl_{name} {label}"
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert (nan_g == nan_w).all(), (label, np.nonzero(nan_g != nan_w)[0])
    ok = nan_w | (np.abs(got - want) <= kr.ctrl_tol(want)) | (got == want)
    assert ok.all(), (label, [(int(i), got[i], want[i])
                              for i in np.nonzero(~ok)[0]])
    return got


def _tcg_state(radius=1e3, iters=0):
    """A consistent mid-tCG block: `iters` interior iterations of the
    model on made-up (positive-curvature) dot products."""
    m = kr.CtrlModel(_base_ctrl(kr.ST_RUN))
    c = m.c
    c[kr.C_DOT0], c[kr.C_DOT1], c[kr.C_DOT2] = 3.5, 16.0, 0.25
    m.init(1e-2, radius, 1.0, 0.1)
    c[kr.C_DOT0] = 2.0
    m.z0()
    for j in range(iters):
        c[kr.C_DOT0] = 40.0 + 3.0 * j          # <delta, H delta>
        m.alpha()
        assert c[kr.C_STOP_PENDING] == 0.0
        c[kr.C_DOT1] = 9.0 / (j + 1)           # ||r||^2, above the bound
        m.rr()
        assert c[kr.C_STATUS] == kr.ST_RUN
        if j + 1 < kr.MAX_TCG:
            c[kr.C_DOT0] = 1.5 / (j + 1)       # <z, r>
            m.beta()
    return c.copy()


def test_ctrl_init_z0():
    hb = _hb()
    c0 = _marker_ctrl()
    c0[kr.C_DOT0], c0[kr.C_DOT1], c0[kr.C_DOT2] = 3.5, 16.0, 0.25
    for tol, st in ((1e-2, kr.ST_RUN), (4.0 + 1e-9, kr.ST_NO_UPDATE),
                    (4.0, kr.ST_RUN)):
        got = _check_ctrl(hb, "init", c0, tol, 100.0, 1.0, 0.1,
                          label=f"tol={tol}")
        assert got[kr.C_STATUS] == st
        assert got[kr.C_BOUND] == 4.0 * 0.1 and got[kr.C_FX] == 1.875
    c0[kr.C_DOT1] = 1e-4           # ||r0|| = 0.01 < kappa: bound = r0^2
    got = _check_ctrl(hb, "init", c0, 1e-3, 10.0, 1.0, 0.1, label="theta")
    assert abs(got[kr.C_BOUND] - 1e-4) < 1e-18
    c = _base_ctrl(kr.ST_RUN)
    c[kr.C_DOT0] = 2.5
    got = _check_ctrl(hb, "z0", c, label="run")
    assert got[kr.C_ZR] == 2.5 and got[kr.C_DPD] == 2.5
    for st in (kr.ST_TCG_STOP, kr.ST_ACCEPTED, kr.ST_NO_UPDATE):
        c = _base_ctrl(st)
        got = _check_ctrl(hb, "z0", c, label=f"status {st}")
        assert (got == c).all()


def test_ctrl_alpha():
    hb = _hb()
    base = _tcg_state(radius=2.0, iters=3)
    e_Pe, e_Pd, d_Pd = base[kr.C_EPE], base[kr.C_EPD], base[kr.C_DPD]
    assert e_Pd > 0 and d_Pd > 0 and e_Pe < 4.0
    cases = {"interior": (1e4, None), "boundary": (1e-3, None),
             "negative curvature": (-0.5, None), "zero curvature": (0.0, None),
             "d_Pd zero": (1e-3, 0.0)}
    for label, (d_Hd, dpd) in cases.items():
        c = base.copy()
        c[kr.C_DOT0] = d_Hd
        if dpd is not None:
            c[kr.C_DPD] = dpd
        got = _check_ctrl(hb, "alpha", c, label=label)
        j = int(c[kr.C_ITER])
        assert got[kr.H_DHD(j)] == d_Hd and got[kr.H_ZR(j)] == c[kr.C_ZR]
        if label == "interior":
            assert got[kr.C_STOP_PENDING] == 0.0
            assert got[kr.C_EPE] > e_Pe
        else:
            assert got[kr.C_STOP_PENDING] == 1.0
            assert got[kr.C_EPE] == e_Pe
            tau = got[kr.C_COEF]
            if dpd == 0.0:
                assert tau == 0.0
            else:
                # tau lands on the trust-region boundary
                lhs = e_Pe + 2 * tau * e_Pd + tau * tau * d_Pd
                assert tau > 0 and abs(lhs - 4.0) <= 1e-12 * 4.0, label
    for st in (kr.ST_TCG_STOP, kr.ST_GIVE_UP):
        c = base.copy()
        c[kr.C_STATUS] = st
        c[kr.C_DOT0] = 5.0
        got = _check_ctrl(hb, "alpha", c, label=f"status {st}")
        assert (got == c).all()


def test_ctrl_rr_beta_tcg_end():
    hb = _hb()
    base = _tcg_state(radius=1e3, iters=2)
    bound = base[kr.C_BOUND]
    for label, rr, stop, st, cur in (
            ("under bound", (0.5 * bound) ** 2, 0.0, kr.ST_TCG_STOP, 1.0),
            ("over bound", (2.0 * bound) ** 2, 0.0, kr.ST_RUN, None),
            ("stop pending", 123.0, 1.0, kr.ST_TCG_STOP, 0.0)):
        c = base.copy()
        c[kr.C_DOT1] = rr
        c[kr.C_STOP_PENDING] = stop
        got = _check_ctrl(hb, "rr", c, label=label)
        assert got[kr.C_STATUS] == st
        if cur is not None:
            assert got[kr.C_USE_CURRENT] == cur
            assert got[kr.C_HLEN] == c[kr.C_ITER] + 1
        if stop:
            assert got[kr.C_DOT1] == rr and got[kr.C_RR] == c[kr.C_RR]
    c = base.copy()
    c[kr.C_DOT0] = 0.8
    got = _check_ctrl(hb, "beta", c, label="run")
    assert got[kr.C_ITER] == c[kr.C_ITER] + 1 and got[kr.C_ZR] == 0.8
    got = _check_ctrl(hb, "tcg_end", base, label="run")
    assert got[kr.C_STATUS] == kr.ST_TCG_STOP
    assert got[kr.C_HLEN] == base[kr.C_ITER] and got[kr.C_USE_CURRENT] == 1.0
    for name in ("rr", "beta", "tcg_end"):
        c = base.copy()
        c[kr.C_STATUS] = kr.ST_TCG_STOP
        got = _check_ctrl(hb, name, c, label="not running")
        assert (got == c).all(), name


def _stopped_history(hlen, radius):
    c = _tcg_state(radius=1e6, iters=kr.MAX_TCG)
    c[kr.C_STATUS] = kr.ST_TCG_STOP
    c[kr.C_HLEN] = hlen
    c[kr.C_RADIUS] = radius
    return c


def test_ctrl_candidate():
    hb = _hb()
    full = _stopped_history(kr.MAX_TCG, 1e6)
    epe = [full[kr.H_EPE(j)] for j in range(kr.MAX_TCG)]
    assert all(b > a for a, b in zip(epe, epe[1:]))
    mid_radius = math.sqrt(0.5 * (epe[5] + epe[6]))
    cases = [("hlen 0", 0, 1e6, None), ("hlen 1 full", 1, 1e6, None),
             ("hlen max full", kr.MAX_TCG, 1e6, None),
             ("truncate j=0", kr.MAX_TCG, 1e-3, 0),
             ("hlen 1 truncate", 1, 1e-3, 0),
             ("truncate j=5", kr.MAX_TCG, mid_radius, 5),
             ("truncate before hlen", 4, mid_radius, None)]
    for label, hlen, radius, jstar in cases:
        c = _stopped_history(hlen, radius)
        c[kr.C_DOT0], c[kr.C_DOT2] = 7.0, 8.0
        got = _check_ctrl(hb, "candidate", c, label=label)
        assert got[kr.C_DOT0] == 0.0 and got[kr.C_DOT2] == 0.0
        if jstar is None:
            assert got[kr.C_USE_CURRENT] == 1.0, label
        else:
            assert got[kr.C_USE_CURRENT] == 0.0, label
            assert got[kr.C_JSTAR] == jstar, label
            j, tau = jstar, got[kr.C_TAUSTAR]
            lhs = (got[kr.H_EPE(j)] + 2 * tau * got[kr.H_EPD(j)]
                   + tau * tau * got[kr.H_DPD(j)])
            assert abs(lhs - radius ** 2) <= 1e-12 * radius ** 2, label
        dm = kr.model_decrease_from_history(got)
        assert abs(got[kr.C_DM] - dm) <= 1e-12 * max(abs(dm), 1e-300), label
    # negative and zero curvature stored in the history; d_Pd == 0
    for label, edits, jstar in (
            ("negative curvature", {kr.H_DHD(3): -0.5}, 3),
            ("zero curvature", {kr.H_DHD(2): 0.0}, 2),
            ("d_Pd zero", {kr.H_DPD(0): 0.0, kr.H_DHD(0): -1.0}, 0)):
        c = _stopped_history(kr.MAX_TCG, 1e6)
        for slot, val in edits.items():
            c[slot] = val
        got = _check_ctrl(hb, "candidate", c, label=label)
        assert got[kr.C_JSTAR] == jstar and got[kr.C_USE_CURRENT] == 0.0
        if "d_Pd" in label:
            assert got[kr.C_TAUSTAR] == 0.0 and got[kr.C_DM] == 0.0
    c = _stopped_history(kr.MAX_TCG, 1.0)
    c[kr.C_STATUS] = kr.ST_RUN
    got = _check_ctrl(hb, "candidate", c, label="running")
    assert (got == c).all()


def test_ctrl_accept_shrink():
    hb = _hb()
    base = _stopped_history(3, 10.0)
    base[kr.C_FX] = 100.0
    for label, dm, qxx, gx, rho_min, st in (
            ("rho above", 4.0, 2 * 97.0, 0.0, 0.1, kr.ST_ACCEPTED),
            ("rho below", 4.0, 2 * 99.8, 0.0, 0.1, kr.ST_TCG_STOP),
            ("rho on the threshold side", 4.0, 2 * 99.0, 0.0, 0.25,
             kr.ST_TCG_STOP),
            ("fprop above fX", 4.0, 2 * 100.5, 0.5, 0.1, kr.ST_TCG_STOP),
            ("dm negative, f down", -1.0, 2 * 99.0, 0.0, 0.1,
             kr.ST_ACCEPTED),
            ("dm zero, f up", 0.0, 2 * 101.0, 0.0, 0.1, kr.ST_TCG_STOP)):
        c = base.copy()
        c[kr.C_DM], c[kr.C_DOT0], c[kr.C_DOT2] = dm, qxx, gx
        got = _check_ctrl(hb, "accept", c, rho_min, label=label)
        assert got[kr.C_STATUS] == st, label
        assert got[kr.C_FPROP] == 0.5 * qxx + gx
    got = _check_ctrl(hb, "shrink", base, label="stopped")
    assert got[kr.C_RADIUS] == 2.5 and got[kr.C_SHRINKS] == \
        base[kr.C_SHRINKS] + 1
    for name, args in (("accept", (0.1,)), ("shrink", ())):
        for st in (kr.ST_RUN, kr.ST_ACCEPTED):
            c = base.copy()
            c[kr.C_STATUS] = st
            got = _check_ctrl(hb, name, c, *args, label=f"status {st}")
            assert (got == c).all(), name


# ---------------------------------------------------------------------
# shape validation: ValueError before any native call
# ---------------------------------------------------------------------
class _NoNative:
    """Stands in for the loaded library: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native entry point {name} reached")


@pytest.mark.parametrize("d,r", [(3, 9), (2, 7), (4, 5)])
def test_unsupported_shape_raises_before_native_call(d, r, monkeypatch):
    hb = _hb()
    with pytest.raises(ValueError):
        hb._check_shape(d, r)
    # the wrappers: with the library handle replaced, reaching a launcher
    # (which would abort the process) is impossible
    monkeypatch.setattr(hb, "_lib", _NoNative())
    n = 4
    X = torch.zeros((d + 1) * n, r, dtype=torch.float64, device=DEV)
    w = torch.zeros(4, dtype=torch.float64, device=DEV)
    calls = [lambda: hb.tangent_project(X, X, d),
             lambda: hb.stiefel_project(X, d),
             lambda: hb.retract(X, X, d),
             lambda: hb.polar_affine(X, X, None, 1.0, 1.0, 0.0, d),
             lambda: hb.gnc_weights(X, X, {}, w, d, r, 1.0, 1.0),
             lambda: hb.DeviceSolver(n, d, r, DEV)]
    if r > 8:
        M = torch.zeros(4, 4, dtype=torch.float32, device=DEV)
        calls.append(lambda: hb.precond_dense(
            M, torch.zeros(4, r, dtype=torch.float64, device=DEV)))
    if d + 1 not in (3, 4):
        L = torch.zeros(n, d + 1, d + 1, dtype=torch.float64, device=DEV)
        calls.append(lambda: hb.precond_jacobi(L, X, d + 1))
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
    wide = torch.zeros(4 * n, 65, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        hb.bsr_spmm(w, w, w, n, 4, wide)
