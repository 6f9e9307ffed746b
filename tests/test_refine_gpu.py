"""GPU tests of the refine kernels (dpo_ops.hip section "refine") stage by
stage against cpu_ref from a common state, their guards and batching, and
refine_to_critical / certified_solve end to end against the CPU run.

Bounds are the derived ones of docs/DESIGN.md §15 (tests/kernel_refs.py):
2 K eps sum |a||b| for sums of K products, propagated through the tangent
projection; cond 64 eps ||A^-1|| ||v|| for the block-Jacobi solve; 8 eps
cond^2 + 16 eps for the polar factor; every control slot 64 eps relative.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as kr
from test_refine import (boundary_radii, grid_case, grid_refined,
                         jacobi_problem, ring_case, ring_staircase)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = kr.EPS
CTL_RTOL = 64.0 * EPS


def _backends():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import cpu_ref, hip_backend
    return cpu_ref, hip_backend


# --------------------------------------------------------------------
# cases and state transfer
# --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(d, n_kind):
    """Q for the stage tests: "two_blocks" is city2d(side=18) (324 poses)
    or grid3d(side=7) (343 poses); 1 and 257 are a chain of that many
    poses with unit-noise-free random edges (one pose: the zero Q)."""
    from dpo_amd.quadratic import BSRMatrix, assemble_connection_laplacian
    from dpo_amd.synthetic import city2d, grid3d
    from dpo_amd.types import RelativeSEMeasurement
    if n_kind == "two_blocks":
        meas, n = city2d(side=18) if d == 2 else grid3d(side=7)
        return assemble_connection_laplacian(meas, n, d), n
    n = int(n_kind)
    if n == 1:
        dh = d + 1
        return BSRMatrix(1, dh, torch.tensor([0, 1], dtype=torch.int32),
                         torch.tensor([0], dtype=torch.int32),
                         torch.zeros(1, dh, dh, dtype=torch.float64)), 1
    g = kr.gen(17, d, n)
    meas = []
    for k in range(n - 1):
        R = kr.manifold_point(1, d, d, g)[:d].numpy().T
        meas.append(RelativeSEMeasurement(
            0, 0, k, k + 1, R, kr.randn(g, d).numpy(), 2.0, 1.5))
    return assemble_connection_laplacian(meas, n, d), n


def precond_of(Q, n, d, r, mode):
    from dpo_amd.quadratic import QuadraticProblem
    problem = QuadraticProblem(n, d, r, precond=mode)
    # the dense mode is built on whatever device Q is on; keep it on the
    # CPU here and move the fp32 inverse
    if mode == "dense":
        A = Q.to_dense() + 0.1 * torch.eye(Q.N, dtype=torch.float64)
        return ("dense", torch.linalg.inv(A).to(torch.float32).contiguous())
    problem.set_q(Q)
    return ("jacobi", problem._Lpre.contiguous())


def to_dev(ws, ctl, pre):
    cr, _ = _backends()
    g = cr.RefineWorkspace(ws.X.to(DEV))
    for name in cr.REFINE_BUFS[1:]:
        getattr(g, name).copy_(getattr(ws, name))
    return g, ctl.to(DEV), (pre[0], pre[1].to(DEV))


def abs_q(Q):
    from dpo_amd.quadratic import BSRMatrix
    return BSRMatrix(Q.n, Q.dh, Q.row_ptr, Q.col_idx, Q.vals.abs())


def spmm_bound(Q, V):
    """Entry-wise bound of Q @ V (any order, FMA)."""
    return kr.sop_bound(abs_q(Q).spmm(V.abs()), kr.bsr_max_row_terms(Q))


def proj_bound(Q, X, V, d):
    """Bound of P_X(Q V) entry-wise."""
    QV = Q.spmm(V)
    return kr.tangent_project_bound(X, QV, d, spmm_bound(Q, V))


def precond_bound(pre, X, V, d):
    """Bound of z = P_X(M^-1 V)."""
    cr, _ = _backends()
    mode, data = pre
    N, r = V.shape
    if mode == "dense":
        M = data.to(torch.float64)
        Z, bZ = M @ V, kr.matmul_bound(M, V, N)
    else:
        dh = d + 1
        A = torch.bmm(data, data.transpose(1, 2))
        ev = torch.linalg.eigvalsh(A)
        vn = V.view(-1, dh, r).norm(dim=1)
        tol = 64.0 * EPS * (ev[:, -1] / ev[:, 0] / ev[:, 0])[:, None] * vn
        bZ = tol[:, None, :].expand(-1, dh, r).reshape(N, r)
        Z = torch.cholesky_solve(V.view(-1, dh, r), data).reshape(N, r)
    return kr.tangent_project_bound(X, Z, d, bZ.contiguous())


def check_vec(name, gpu, ref, bound):
    err = (gpu.cpu() - ref).abs()
    worst = float((err - bound).max())
    print(f"  {name}: max err {float(err.max()):.3e}, "
          f"max bound {float(torch.as_tensor(bound).max()):.3e}")
    assert worst <= 0.0, f"{name}: {worst:.3e} over its bound"


def check_ctl(gpu, ref, skip=()):
    cr, _ = _backends()
    g, c = gpu.cpu().numpy(), ref.numpy()
    for slot in range(cr.RF_SIZE):
        if slot in skip:
            continue
        err, tol = abs(g[slot] - c[slot]), CTL_RTOL * abs(c[slot])
        if err > 0:
            print(f"  ctl[{slot}]: gpu {g[slot]!r} ref {c[slot]!r} "
                  f"err/|ref| {err / max(abs(c[slot]), 1e-300) / EPS:.1f} eps")
        assert err <= tol, f"control slot {slot}: {g[slot]!r} vs {c[slot]!r}"


STAGE_CASES = [(d, r, "two_blocks", "jacobi") for d, r in kr.SHAPES] \
    + [(d, r, nk, "jacobi") for d, r in kr.SHAPES for nk in ("1", "257")] \
    + [(2, 3, "two_blocks", "dense"), (3, 5, "two_blocks", "dense")]


# --------------------------------------------------------------------
# 1. head, one tCG iteration, candidate: each from a common state
# --------------------------------------------------------------------
@pytest.mark.parametrize("d,r,n_kind,mode", STAGE_CASES)
def test_stages_match_cpu_ref(d, r, n_kind, mode):
    cr, hip = _backends()
    Q, n = graph(d, n_kind)
    X = kr.manifold_point(n, d, r, kr.gen(23, d, r, n))
    pre = precond_of(Q, n, d, r, mode)
    Qd = Q.to(DEV)

    # ---- head ----
    # from a random point the first step is long: a radius of 1e6 keeps
    # the first tCG iteration inside the trust region, so it continues
    ws = cr.RefineWorkspace(X)
    ctl = cr.refine_control(1e-9, 1e6, 1000)
    gws, gctl, gpre = to_dev(ws, ctl, pre)
    cr.refine_head(Q, ws, ctl, d, pre)
    hip.refine_head(Qd, gws, gctl, d, gpre)
    print("head")
    b_grad = proj_bound(Q, X, X, d)
    check_vec("grad", gws.grad, ws.grad, b_grad)
    check_vec("r", gws.r, ws.r, b_grad)
    assert torch.equal(gws.eta.cpu(), ws.eta)
    if n_kind == "1":
        # one pose, Q = 0: the gradient is zero and the head converges
        assert ctl[cr.RF_STATUS] == cr.RS_CONVERGED
        check_ctl(gctl, ctl)
        return
    assert ctl[cr.RF_STATUS] == cr.RS_RUN
    # z0 is computed from each side's own r: |M^-1| applied to the
    # difference of the two r adds to the preconditioner's own bound
    b_z = precond_bound(pre, X, ws.r, d) \
        + precond_apply_abs(pre, X, b_grad, d)
    check_vec("z", gws.z, ws.z, b_z)
    check_vec("delta", gws.delta, ws.delta, b_z)
    check_ctl(gctl, ctl)

    # ---- one tCG iteration from the CPU's post-head state ----
    gws, gctl, _ = to_dev(ws, ctl, pre)
    before = {k: getattr(ws, k).clone() for k in ("eta", "r", "delta")}
    cr.refine_tcg_steps(Q, ws, ctl, d, pre, 1)
    hip.refine_tcg_steps(Qd, gws, gctl, d, gpre, 1)
    print("tcg iteration")
    assert ctl[cr.RF_STATUS] == cr.RS_RUN, "pick a state that continues"
    b_Hd = proj_bound(Q, X, before["delta"], d)
    check_vec("Hd", gws.Hd, ws.Hd, b_Hd)
    coef, beta = float(ctl[cr.RF_COEF]), float(ctl[cr.RF_BETA])
    # fma: one rounding of the result; coef within 64 eps
    b_eta = 66.0 * EPS * (before["eta"].abs()
                          + abs(coef) * before["delta"].abs())
    check_vec("eta", gws.eta, ws.eta, b_eta)
    b_r = abs(coef) * b_Hd + 66.0 * EPS * (before["r"].abs()
                                           + abs(coef) * ws.Hd.abs())
    check_vec("r", gws.r, ws.r, b_r)
    b_z = precond_bound(pre, X, ws.r, d) + precond_apply_abs(pre, X, b_r, d)
    check_vec("z", gws.z, ws.z, b_z)
    b_delta = b_z + 66.0 * EPS * (abs(beta) * before["delta"].abs()
                                  + ws.z.abs())
    check_vec("delta", gws.delta, ws.delta, b_delta)
    check_ctl(gctl, ctl)

    # ---- candidate from the CPU's state, its one-step eta as the step
    ctl[cr.RF_STATUS] = cr.RS_TCG_DONE
    gws, gctl, _ = to_dev(ws, ctl, pre)
    cr.refine_candidate(Q, ws, ctl, d)
    hip.refine_candidate(Qd, gws, gctl, d)
    print("candidate")
    conds = kr.block_conds(X + ws.eta, d)
    tol = torch.from_numpy(kr.polar_tol(conds))[:, None, None].expand(
        n, d + 1, r).reshape(-1, r)
    check_vec("Xp", gws.Xp, ws.Xp, tol)
    assert ctl[cr.RF_STATUS] == cr.RS_HEAD
    check_ctl(gctl, ctl)
    if ctl[cr.RF_ACCEPTED] != 0.0:
        assert torch.equal(gws.X, gws.Xp)
    else:
        assert torch.equal(gws.X.cpu(), X)


def precond_apply_abs(pre, X, bV, d):
    """Entry-wise bound of P_X(M^-1 e) for |e| <= bV."""
    mode, data = pre
    N, r = bV.shape
    if mode == "dense":
        bZ = data.to(torch.float64).abs() @ bV
    else:
        dh = d + 1
        Ainv = torch.cholesky_inverse(data).abs()
        bZ = torch.bmm(Ainv, bV.view(-1, dh, r)).reshape(N, r)
    zero = torch.zeros_like(bV)
    return kr.tangent_project_bound(X, zero, d, bZ.contiguous())


# --------------------------------------------------------------------
# 2. grid cap: one pose past 256 blocks of 256 threads
# --------------------------------------------------------------------
def test_hd_stage_past_grid_cap():
    cr, hip = _backends()
    from dpo_amd.quadratic import assemble_connection_laplacian
    from dpo_amd.synthetic import grid3d_soa
    side = 41                      # 68921 poses >= 256 * 256 + 1
    ma, n_all = grid3d_soa(side)
    n = cr.CERT_BLOCK * cr.CERT_BLOCK + 1
    assert n_all >= n
    d, r = 3, 3
    Q = assemble_connection_laplacian(ma, n_all, d)
    g = kr.gen(29)
    X = kr.manifold_point(n_all, d, r, g)
    ws = cr.RefineWorkspace(X)
    ws.delta.copy_(kr.randn(g, *X.shape))
    ctl = cr.refine_control(0.0, 10.0, 10)
    ctl[cr.RF_STATUS] = cr.RS_RUN
    assert cr.cert_partials(n_all) == cr.CERT_BLOCK
    gws, gctl, _ = to_dev(ws, ctl, ("jacobi", torch.zeros(1)))
    cr.refine_hd_stage(Q, ws, ctl, d)
    hip.refine_hd_stage(Q.to(DEV), gws, gctl, d)
    check_vec("Hd", gws.Hd, ws.Hd, proj_bound(Q, X, ws.delta, d))
    dot = float(gws.part[:cr.CERT_BLOCK].sum())
    ref = float(ws.part[0])
    bound = kr.dot_bound(ws.delta, ws.Hd) + float(
        (ws.delta.abs() * proj_bound(Q, X, ws.delta, d)).sum())
    print(f"<delta, Hd>: gpu {dot!r} ref {ref!r} bound {bound:.3e}")
    assert abs(dot - ref) <= bound


# --------------------------------------------------------------------
# 3. guards
# --------------------------------------------------------------------
@pytest.mark.parametrize("d,r,mode", [(2, 3, "jacobi"), (3, 5, "jacobi"),
                                      (3, 5, "dense")])
def test_guards_leave_everything_untouched(d, r, mode):
    cr, hip = _backends()
    Q, n = graph(d, "257")
    pre = precond_of(Q, n, d, r, mode)
    Qd = Q.to(DEV)
    g = kr.gen(31, d, r)
    ws = cr.RefineWorkspace(kr.manifold_point(n, d, r, g))
    for name in cr.REFINE_BUFS[1:]:
        getattr(ws, name).copy_(kr.randn(g, *ws.X.shape))
    ws.part.copy_(kr.randn(g, ws.part.numel()))
    ctl0 = cr.refine_control(1e-3, 10.0, 100)
    ctl0[cr.RF_FX:cr.RF_DHD + 1] = kr.randn(g, cr.RF_DHD).abs() + 0.5
    ctl0[cr.RF_ACCEPTED] = 0.0
    ctl0[cr.RF_STOP] = 0.0
    stages = {
        # the head's z0 kernels are the tCG's, guarded on RS_RUN like them
        "head": (lambda w, c, p: hip.refine_head(Qd, w, c, d, p),
                 (cr.RS_TCG_DONE, cr.RS_CONVERGED)),
        "tcg": (lambda w, c, p: hip.refine_tcg_steps(Qd, w, c, d, p, 2),
                (cr.RS_TCG_DONE, cr.RS_CONVERGED, cr.RS_HEAD)),
        "hd": (lambda w, c, p: hip.refine_hd_stage(Qd, w, c, d),
               (cr.RS_TCG_DONE, cr.RS_CONVERGED, cr.RS_HEAD)),
        # RS_HEAD with RF_ACCEPTED = 0 is the guard of the copy kernel
        "candidate": (lambda w, c, p: hip.refine_candidate(Qd, w, c, d),
                      (cr.RS_RUN, cr.RS_CONVERGED, cr.RS_HEAD)),
    }
    for name, (run, statuses) in stages.items():
        for st in statuses:
            ctl = ctl0.clone()
            ctl[cr.RF_STATUS] = st
            gws, gctl, gpre = to_dev(ws, ctl, pre)
            gws.part.copy_(ws.part)
            run(gws, gctl, gpre)
            torch.cuda.synchronize()
            assert torch.equal(gctl.cpu(), ctl), (name, st)
            assert torch.equal(gws.part.cpu(), ws.part), (name, st)
            for buf in cr.REFINE_BUFS:
                assert torch.equal(getattr(gws, buf).cpu(),
                                   getattr(ws, buf)), (name, st, buf)


# --------------------------------------------------------------------
# 4. batch over-enqueue
# --------------------------------------------------------------------
def test_over_enqueued_batch_is_noops():
    cr, hip = _backends()
    meas, n, Q, X0 = grid_case()
    d = 3
    _, pre = jacobi_problem(Q, n, d, 5)
    Qd = Q.to(DEV)
    out = []
    for nsteps in (16, 3):
        ws = cr.RefineWorkspace(X0)
        ctl = cr.refine_control(0.0, boundary_radii()[1], 1000)
        gws, gctl, gpre = to_dev(ws, ctl, pre)
        hip.refine_head(Qd, gws, gctl, d, gpre)
        hip.refine_tcg_steps(Qd, gws, gctl, d, gpre, nsteps)
        out.append((gws.eta.cpu(), gctl.cpu()))
    (eta16, ctl16), (eta3, ctl3) = out
    assert ctl3[cr.RF_STATUS] == cr.RS_TCG_DONE
    assert ctl3[cr.RF_ITER] == 3 and ctl3[cr.RF_TCG] == cr.RT_EXCEEDED_TR
    assert torch.equal(eta16, eta3) and torch.equal(ctl16, ctl3)


# --------------------------------------------------------------------
# 5. end to end
# --------------------------------------------------------------------
def test_grid_refine_and_certify_on_gpu():
    from dpo_amd.certify import (CertificateStatus, certificate_operator,
                                 certify_solution)
    from dpo_amd.refine import refine_to_critical
    meas, n, Q, X0 = grid_case()
    cpu = grid_refined()
    Qd = Q.to(DEV)
    runs = [refine_to_critical(Qd, X0.to(DEV), precond="jacobi")
            for _ in range(2)]
    res = runs[0]
    assert res.status == cpu.status == "CONVERGED"
    assert res.Xt.is_cuda and res.precond == "jacobi"
    _, gn = certificate_operator(Qd, res.Xt)
    print(f"grad norm {gn:.3e} (refine {res.grad_norm_final:.3e}), tol "
          f"{res.grad_tol:.3e}; outer {res.outer_steps}/{cpu.outer_steps} "
          f"inner {res.inner_iterations}/{cpu.inner_iterations}")
    assert gn <= res.grad_tol and res.grad_norm_final <= res.grad_tol
    assert res.f_final <= res.f_init
    assert torch.equal(runs[0].Xt, runs[1].Xt)
    cert = certify_solution(meas, n, 3, res.Xt)
    assert cert.status == CertificateStatus.CERTIFIED


def test_ring67_staircase_on_gpu():
    from dpo_amd.certify import CertificateStatus
    from dpo_amd.refine import certified_solve
    meas, n, Q, X = ring_case(67)
    cpu = ring_staircase()
    runs = [certified_solve(meas, n, 2, X.to(DEV),
                            refine_kw={"precond": "jacobi"})
            for _ in range(2)]
    res = runs[0]
    print([(lv.rank, lv.certificate.status.value, lv.refine.outer_steps,
            lv.refine.inner_iterations, lv.refine.f_final)
           for lv in res.levels])
    assert len(res.levels) == len(cpu.levels) == 3
    assert [lv.rank for lv in res.levels] == [lv.rank for lv in cpu.levels]
    assert [lv.certificate.status for lv in res.levels] \
        == [lv.certificate.status for lv in cpu.levels]
    assert res.status == CertificateStatus.CERTIFIED and res.rank == 4
    for lv in res.levels:
        assert lv.refine.status == "CONVERGED"
        assert lv.refine.grad_norm_final <= lv.refine.grad_tol
    assert torch.equal(runs[0].Xt, runs[1].Xt)
    # precond="auto" on the GPU is the dense inverse at this size
    auto = certified_solve(meas, n, 2, X.to(DEV))
    assert auto.levels[-1].refine.precond == "dense"
    assert auto.status == CertificateStatus.CERTIFIED and auto.rank == 4


# --------------------------------------------------------------------
# 6. more than 16 tCG iterations in one solve
# --------------------------------------------------------------------
def test_tcg_runs_past_16_iterations():
    """The RBCD device solver stops at MAX_TCG = 16. On the 343-pose grid
    with block-Jacobi, from the iterate refined to the default gate (a
    small gradient, hence a tight relative tCG bound), the CPU reference
    needs more; the GPU must finish with the same count and status."""
    cr, hip = _backends()
    from dpo_amd.chordal import chordal_initialization
    from dpo_amd.manifold import lifting_matrix
    from dpo_amd.refine import refine_to_critical
    from dpo_amd.synthetic import grid3d
    d, r = 3, 5
    Q, n = graph(d, "two_blocks")
    meas, _ = grid3d(side=7)
    T = chordal_initialization(d, n, meas)
    X0 = torch.from_numpy(
        np.ascontiguousarray((lifting_matrix(d, r) @ T).T))
    pre = precond_of(Q, n, d, r, "jacobi")
    X1 = refine_to_critical(Q, X0, precond="jacobi").Xt
    ws = cr.RefineWorkspace(X1)
    ctl = cr.refine_control(0.0, 10.0, 1000)
    gws, gctl, gpre = to_dev(ws, ctl, pre)
    cr.refine_head(Q, ws, ctl, d, pre)
    cr.refine_tcg_steps(Q, ws, ctl, d, pre, 1000)
    iters = int(ctl[cr.RF_ITER])
    print(f"CPU tCG iterations: {iters}, "
          f"status {cr.REFINE_TCG_NAMES[int(ctl[cr.RF_TCG])]}")
    assert ctl[cr.RF_STATUS] == cr.RS_TCG_DONE and iters > 16
    Qd = Q.to(DEV)
    hip.refine_head(Qd, gws, gctl, d, gpre)
    hip.refine_tcg_steps(Qd, gws, gctl, d, gpre, iters + 8)
    h = gctl.cpu()
    assert h[cr.RF_STATUS] == cr.RS_TCG_DONE
    assert int(h[cr.RF_ITER]) == iters
    assert h[cr.RF_TCG] == ctl[cr.RF_TCG]
