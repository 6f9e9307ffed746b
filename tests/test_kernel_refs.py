"""CPU checks of tests/kernel_refs.py: the references, bounds and input
builders the GPU kernel matrix relies on must themselves be right, and
every polar-projection input used on the GPU must lie inside the stated
domain of the Gram-matrix iteration."""
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr
from dpo_amd.ops import cpu_ref


def test_shape_and_n_lists():
    assert len(kr.SHAPES) == 11
    assert (2, 2) in kr.SHAPES and (3, 8) in kr.SHAPES
    assert (3, 9) not in kr.SHAPES and (2, 7) not in kr.SHAPES
    # r = 6 and r = 7 (d = 3) leave a dead thread tail in each block
    assert kr.poses_per_block(3, 6) == 10 and kr.poses_per_block(3, 7) == 9
    assert kr.n_tile(3, 7) == (1, 9, 10, 28, 257)
    for d, r in kr.SHAPES:
        assert max(kr.n_tile(d, r)) <= 600


def test_sop_bound_holds_for_any_order_and_sees_a_dropped_term():
    g = kr.gen(1)
    a, b = kr.randn(g, 4000), kr.randn(g, 4000)
    bound = kr.dot_bound(a, b)
    exact = float(np.dot(a.numpy().astype(np.longdouble),
                         b.numpy().astype(np.longdouble)))
    perm = torch.randperm(4000, generator=g)
    for s in (float((a * b).sum()), float((a[perm] * b[perm]).sum()),
              float(sum((a * b).tolist()))):
        assert abs(s - exact) <= bound
    assert bound < 1e-8
    drop = float((a[1:] * b[1:]).sum())
    assert abs(drop - exact) > 1e3 * bound


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_random_bsr_is_symmetric_with_uneven_rows(n):
    Q = kr.random_bsr(n, 4, kr.gen(2, n))
    D = Q.to_dense()
    assert D.shape == (4 * n, 4 * n)
    assert torch.equal(D, D.T)
    lens = np.diff(Q.row_ptr.numpy())
    assert lens.min() >= 1
    if n >= 65:
        assert lens.max() >= 40 and lens.min() <= 4
    ci = Q.col_idx.numpy()
    assert ci.min() >= 0 and ci.max() < n


def test_tangent_project_bound_covers_reordered_evaluation():
    d, r, n = 3, 5, 65
    g = kr.gen(3)
    X = kr.manifold_point(n, d, r, g)
    A = kr.randn(g, 4 * n, r)
    ref = cpu_ref.tangent_project(X, A, d)
    Xl = X.numpy().astype(np.longdouble).reshape(n, 4, r)
    Al = A.numpy().astype(np.longdouble).reshape(n, 4, r)
    Y = Xl[:, :3]
    S = np.einsum("nak,nbk->nab", Y, Al[:, :3])
    S = 0.5 * (S + S.transpose(0, 2, 1))
    P = Al.copy()
    P[:, :3] -= np.einsum("nab,nbk->nak", S, Y)
    err = np.abs(ref.numpy().reshape(n, 4, r) - P).astype(np.float64)
    b = kr.tangent_project_bound(X, A, d).numpy().reshape(n, 4, r)
    assert (err <= b).all()
    assert b.max() < 1e-13
    assert (b[:, 3] == 0).all()      # translation rows are copies


# ---------------------------------------------------------------- polar
def _emulation_margin(M, d):
    out = kr.polar_emulation(M, d)
    err, orth = kr.polar_errors(out, M, d)
    tol = kr.polar_tol(kr.block_conds(M, d))
    return np.maximum(err, orth) / tol


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_polar_inputs_are_inside_the_domain(d, r):
    """Under the CPU emulation of the Gram-matrix iteration, every input
    the GPU polar tests use stays under 8 eps cond^2 + 16 eps."""
    for n in kr.N_POSE:
        for form, (A, B, C, ca, cb, cc) in kr.polar_form_inputs(
                d, r, n).items():
            M = kr.affine(A, B, C, ca, cb, cc)
            assert kr.block_conds(M, d).max() < 1e6, (form, n)
            assert _emulation_margin(M, d).max() <= 1.0, (form, n)
    for label, cond, M in kr.polar_cond_cases(d, r):
        c = kr.block_conds(M, d)
        assert np.allclose(c, cond, rtol=1e-6), label
        assert _emulation_margin(M, d).max() <= 1.0, label
    for label, cbound, X, eta in kr.polar_retract_cases(d, r):
        M = X + eta
        assert kr.block_conds(M, d).max() <= cbound * (1 + 1e-9), label
        assert _emulation_margin(M, d).max() <= 1.0, label


@pytest.mark.parametrize("d,r", [(2, 2), (3, 3), (3, 5), (3, 8)])
def test_polar_bound_is_not_vacuous(d, r):
    """At cond(M) = 1e7 the iteration is outside its domain: the
    emulation is off the SVD polar by about 0.15 and its Y Y^T - I
    exceeds the bound on every block, so the GPU assertions (closeness
    and orthonormality under one bound) would fail there."""
    M = kr.cond_blocks(200, d, r, 1e7, 1.0, kr.gen(6, d, r))
    out = kr.polar_emulation(M, d)
    err, orth = kr.polar_errors(out, M, d)
    tol = kr.polar_tol(1e7)
    assert orth.min() > tol      # every block fails the orthonormality check
    assert err.max() > 0.05


def test_polar_emulation_zero_block_when_gram_trace_underflows():
    M = torch.full((4, 5), 1e-160, dtype=torch.float64)
    out = kr.polar_emulation(M, 3)
    assert torch.equal(out[:3], torch.zeros(3, 5, dtype=torch.float64))
    assert torch.equal(out[3], M[3])


# --------------------------------------------------------------- jacobi
@pytest.mark.parametrize("dh", [3, 4])
def test_jacobi_blocks_and_tolerance(dh):
    n, r = 65, 5
    g = kr.gen(8, dh)
    A = kr.spd_blocks(n, dh, g)
    ev = torch.linalg.eigvalsh(A)
    assert float(ev.min()) > 0.999
    conds = (ev[:, -1] / ev[:, 0]).numpy()
    assert conds.max() > 0.9e6 and conds.min() < 1.1
    V = kr.randn(g, n * dh, r)
    L = torch.linalg.cholesky(A)
    ref = torch.cholesky_solve(V.view(n, dh, r), L).reshape(-1, r)
    Al = A.numpy().astype(np.longdouble)
    xl = np.stack([np.linalg.solve(A[i].numpy(), V.view(n, dh, r)[i].numpy())
                   for i in range(n)])
    # one step of refinement in extended precision
    res = V.view(n, dh, r).numpy().astype(np.longdouble) - Al @ xl
    xl = xl + np.stack([np.linalg.solve(A[i].numpy(),
                                        res[i].astype(np.float64))
                        for i in range(n)])
    err = np.abs(ref.numpy().reshape(n, dh, r) - xl).astype(np.float64)
    tol = kr.jacobi_tol(A, V).numpy().reshape(n, dh, r)
    assert (err <= tol).all()
    # a swapped pair of factor entries is far outside it
    assert tol.max() < 1e-6 * float(V.abs().max())


# ------------------------------------------------------------------ gnc
def test_gnc_reference_regimes():
    barc = 10.0
    for mu in (1e-2, 1.0, 1e4):
        lower = mu / (mu + 1) * barc ** 2
        upper = (mu + 1) / mu * barc ** 2
        w = kr.gnc_weight_ref(
            np.array([0.5 * lower, math.sqrt(lower * upper), 2 * upper]),
            mu, barc)
        assert w[0] == 1.0 and w[2] == 0.0
        # at the geometric mean r^2 = barc^2 exactly: w = sqrt(mu(mu+1)) - mu
        assert abs(w[1] - (math.sqrt(mu * (mu + 1)) - mu)) <= kr.gnc_tol(mu)
        assert 0.0 < w[1] < 1.0


def test_gnc_residual_zero_for_consistent_edge():
    d, r = 3, 5
    g = kr.gen(9)
    P1 = kr.manifold_point(1, d, r, g).view(1, d + 1, r).numpy()
    R = torch.linalg.qr(kr.randn(g, d, d))[0].numpy()[None]
    t = kr.randn(g, 1, d).numpy()
    P2 = np.zeros_like(P1)
    P2[:, :d] = np.einsum("eab,eak->ebk", R, P1[:, :d])
    P2[:, d] = P1[:, d] + np.einsum("ea,eak->ek", t, P1[:, :d])
    rsq = kr.gnc_residual_sq(P1, P2, R, t, np.array([3.0]),
                             np.array([2.0]), d)
    assert rsq[0] < 1e-28
    P2[:, d, 0] += 2.0
    rsq = kr.gnc_residual_sq(P1, P2, R, t, np.array([3.0]),
                             np.array([2.0]), d)
    assert abs(rsq[0] - 8.0) < 1e-12


# ---------------------------------------------------- tCG control model
@pytest.fixture(scope="module")
def tcg_problem():
    from dpo_amd.quadratic import (QuadraticProblem,
                                   assemble_connection_laplacian)
    from dpo_amd.synthetic import grid3d
    meas, n = grid3d(side=4, seed=0)
    d, r = 3, 5
    p = QuadraticProblem(n, d, r, precond="jacobi")
    p.set_q(assemble_connection_laplacian(meas, n, d))
    return p, kr.manifold_point(n, d, r, kr.gen(10))


@pytest.mark.parametrize("Delta0,status,use_current", [
    (1e4, "converged", 1.0), (1.0, "exceeded_tr", 0.0),
    (100.0, "exceeded_tr", 0.0)])
def test_ctrl_model_reproduces_host_tcg(tcg_problem, Delta0, status,
                                        use_current):
    """The control model, driven through a whole solve, takes the host
    optimizer's step and ends in its status."""
    p, X0 = tcg_problem
    Xh, res, runs, iters = kr.host_solve(p, X0, 1e-2, Delta0, 10)
    Xm, c, st = kr.model_solve(p, X0, 1e-2, Delta0, 10)
    assert res.tcg_status == status and runs == 1
    assert st == kr.ST_ACCEPTED and c[kr.C_SHRINKS] == 0
    assert c[kr.C_USE_CURRENT] == use_current
    assert int(c[kr.C_HLEN]) == iters
    assert torch.allclose(Xm, Xh, atol=1e-9, rtol=0)
    assert abs(c[kr.C_FPROP] - res.f_opt) <= 1e-9 * abs(res.f_opt)
    # model decrease recomputed from the stored history
    dm = kr.model_decrease_from_history(c)
    assert abs(dm - c[kr.C_DM]) <= 1e-12 * abs(dm)


def test_ctrl_model_max_inner_cap(tcg_problem):
    p, X0 = tcg_problem
    Xh, res, runs, iters = kr.host_solve(p, X0, 1e-2, 1e4, 2)
    Xm, c, st = kr.model_solve(p, X0, 1e-2, 1e4, 2)
    assert res.tcg_status == "max_inner" and iters == 2
    assert int(c[kr.C_HLEN]) == 2 and c[kr.C_USE_CURRENT] == 1.0
    assert torch.allclose(Xm, Xh, atol=1e-9, rtol=0)


def test_ctrl_model_no_update_below_tolerance(tcg_problem):
    p, X0 = tcg_problem
    Xm, c, st = kr.model_solve(p, X0, 1e9, 100.0, 10)
    assert st == kr.ST_NO_UPDATE and Xm is X0


def test_boundary_tau_lands_on_the_radius():
    m = kr.CtrlModel()
    c = m.c
    c[kr.C_STATUS] = kr.ST_RUN
    c[kr.C_ZR], c[kr.C_EPE], c[kr.C_EPD], c[kr.C_DPD] = 2.0, 1.5, 0.3, 0.8
    c[kr.C_RADIUS] = 2.0
    c[kr.C_DOT0] = 0.1          # alpha = 20: far past the boundary
    m.alpha()
    assert c[kr.C_STOP_PENDING] == 1.0
    tau = c[kr.C_COEF]
    lhs = 1.5 + 2 * tau * 0.3 + tau * tau * 0.8
    assert abs(lhs - 4.0) <= 1e-12 * 4.0 and tau > 0


@pytest.mark.parametrize("d,r,Delta0,max_shrink", kr.SHRINK_CASES)
def test_shrink_cases_tell_the_attempts_apart(d, r, Delta0, max_shrink):
    """What keeps the device shrink test honest: every case gives up
    after exactly max_shrink shrinks, and the rho the host must read (the
    last attempt's) is at least 100 rho bounds away from the rho of every
    earlier attempt, so a replay that stopped early, skipped a shrink or
    formed the step of another attempt cannot pass. Attempts that take
    the same full step share one rho by construction (the (3, 8) case
    has three); they are told apart from the last one, which is what the
    device reports."""
    p, X0, c, status, attempts, b_rho = kr.shrink_case_ref(d, r, Delta0,
                                                           max_shrink)
    assert status == kr.ST_GIVE_UP
    assert c[kr.C_SHRINKS] == max_shrink == len(attempts) - 1
    assert c[kr.C_RHO] == attempts[-1]["rho"] < kr.SHRINK_ACCEPT_RHO
    assert c[kr.C_RADIUS] == Delta0 * 0.25 ** max_shrink
    assert 0.0 < b_rho < 1e-6
    for a in attempts[:-1]:
        assert abs(a["rho"] - attempts[-1]["rho"]) >= 100.0 * b_rho
    # successive attempts with different steps differ as clearly
    for a, b in zip(attempts, attempts[1:]):
        same_step = a["use_current"] and b["use_current"]
        assert same_step or abs(a["rho"] - b["rho"]) >= 100.0 * b_rho


def test_shrink_case_switches_from_full_step_to_replay():
    """The (3, 8) case: the full step (C_USE_CURRENT = 1) survives three
    radii, the fourth truncates the stored path at snapshot jstar = 1."""
    _, _, c, _, attempts, _ = kr.shrink_case_ref(3, 8, 1e5, 3)
    assert [a["use_current"] for a in attempts] == [True, True, True, False]
    assert attempts[-1]["jstar"] == 1 and c[kr.C_JSTAR] == 1
    assert c[kr.C_USE_CURRENT] == 0.0 and c[kr.C_HLEN] > 2
    assert abs(attempts[0]["rho"] - 1.416412642) < 1e-8
    assert abs(attempts[-1]["rho"] - 1.286575622) < 1e-8
    assert attempts[-1]["radius"] == 1562.5


# ------------------------------------------- certificate kernel matrix
# Every bound of the certificate matrix is checked twice here: the fp64
# reference lies within HALF its bound of a numpy.longdouble evaluation
# of the same operation (the device gets the other half), and the
# bound's maximum is below 1e-3 of the median magnitude of what it
# guards, so a dropped term or a wrong Lambda entry cannot hide.
LD = np.longdouble


def _ld(t):
    return t.numpy().astype(LD)


def _within_half(ref, exact, bound, what):
    err = np.abs(np.asarray(ref, dtype=np.float64).astype(LD) - exact)
    half = 0.5 * np.asarray(bound, dtype=np.float64).astype(LD)
    assert (err <= half).all(), (what, float(err.max()))


def _sees_fault(bound, guarded, what):
    b = float(np.max(np.asarray(bound, dtype=np.float64)))
    med = float(np.median(np.abs(np.asarray(guarded, dtype=np.float64))))
    assert 0.0 <= b < 1e-3 * med, (what, b, med)


def _s_apply_ld(Q, lam, v):
    """(Q - Lambda) v in longdouble on the scalar CSR (every row has its
    diagonal block, so reduceat sees no empty row)."""
    csr = Q.to_scalar_csr()
    crow = csr.crow_indices().numpy()
    assert (np.diff(crow) > 0).all()
    prod = csr.values().numpy().astype(LD) * v[csr.col_indices().numpy()]
    w = np.add.reduceat(prod, crow[:-1])
    n, d = lam.shape[0], lam.shape[1]
    wb = w.reshape(n, d + 1)
    wb[:, :d] -= np.einsum("nab,nb->na", _ld(lam),
                           v.reshape(n, d + 1)[:, :d])
    return w


def test_cert_sizes_reach_the_wrap():
    assert np.finfo(LD).eps < 1e-18
    for d, ns in kr.CERT_ROW_POSES.items():
        N = [(d + 1) * n for n in ns]
        assert cpu_ref.cert_partials(N[-1]) == 256
        assert 0 < N[-1] - 65536 <= 4          # rows on a second trip
    assert 4 * kr.CERT_ROW_POSES[3][-2] == 65536
    assert kr.cert_lambda_poses(3, 8)[-1] == 65537
    assert kr.cert_lambda_poses(2, 6)[-1] == 65537
    assert kr.cert_lambda_poses(3, 5) == kr.N_POSE
    assert kr.cert_steps_for(3) == (0, 1) and kr.cert_steps_for(4) == (0, 1)
    assert kr.cert_steps_for(192) == kr.CERT_STEPS
    Q, Qa = kr.cert_matrix(65, 3)
    assert kr.cert_matrix(65, 3)[0] is Q
    assert torch.equal(Qa.vals, Q.vals.abs())


@pytest.mark.parametrize("d,r", kr.SHAPES)
def test_cert_lambda_ref_and_bounds(d, r):
    for n in kr.cert_lambda_poses(d, r):
        g = kr.gen(41, d, r, n)
        X = kr.manifold_point(n, d, r, g)
        QX = kr.randn(g, (d + 1) * n, r)
        lam, res, b_lam, b_res = kr.cert_lambda_ref(X, QX, d)
        Xl = _ld(X).reshape(n, d + 1, r)
        Gl = _ld(QX).reshape(n, d + 1, r)
        A = np.einsum("nak,nbk->nab", Gl[:, :d], Xl[:, :d])
        L = 0.5 * (A + A.transpose(0, 2, 1))
        gl = Gl.copy()
        gl[:, :d] -= np.einsum("nab,nbk->nak", L, Xl[:, :d])
        _within_half(lam.numpy(), L, b_lam.numpy(), ("lam", d, r, n))
        _within_half(res, (gl * gl).sum(), b_res, ("res", d, r, n))
        _sees_fault(b_lam, lam, ("lam", d, r, n))
        _sees_fault(b_res, res, ("res", d, r, n))
    # with QX = Q X it is cpu_ref.cert_lambda
    Q, _ = kr.cert_matrix(65, d)
    X = kr.manifold_point(65, d, r, kr.gen(47, d, r))
    lam_c, res_c = cpu_ref.cert_lambda(Q, X, d)
    lam, res, b_lam, b_res = kr.cert_lambda_ref(X, Q.spmm(X), d)
    assert bool(((lam - lam_c).abs() <= b_lam).all())
    assert abs(res - float(res_c)) <= b_res


@pytest.mark.parametrize("d,n", [(2, 1), (2, 65), (2, 21846), (3, 1),
                                 (3, 64), (3, 65), (3, 16385)])
def test_cert_apply_ref_and_bounds(d, n):
    N = n * (d + 1)
    Q, Qa = kr.cert_matrix(n, d)
    g = kr.gen(42, d, n)
    lam = kr.cert_lam_blocks(n, d, g)
    v, vprev = kr.randn(g, N), kr.randn(g, N)
    for vp, beta in ((None, 0.0), (vprev, kr.CERT_BETA_PREV)):
        w, alpha, b_w, b_a = kr.cert_apply_ref(Q, Qa, lam, v, vp, beta)
        wl = _s_apply_ld(Q, lam, _ld(v))
        if vp is not None:
            wl -= LD(beta) * _ld(vp)
        _within_half(w.numpy(), wl, b_w.numpy(), ("w", d, n))
        _within_half(alpha, np.dot(_ld(v), wl), b_a, ("alpha", d, n))
        _sees_fault(b_w, w, ("w", d, n))
        _sees_fault(b_a, alpha, ("alpha", d, n))
    assert kr.cert_apply_terms(Q, d) == \
        int(np.diff(Q.row_ptr.numpy()).max()) * (d + 1) + d + 1


@pytest.mark.parametrize("d,n", [(2, 1), (2, 65), (2, 21846), (3, 1),
                                 (3, 64), (3, 65), (3, 16385)])
def test_cert_step_ref_and_bounds(d, n):
    """cert_step_ref against a longdouble run of the same step, and
    cpu_ref.cert_lanczos_steps (the reference of alpha, beta and v_{j+1}
    on the device) against the same run under the same bounds."""
    N = n * (d + 1)
    M, H = kr.CERT_M, cpu_ref.CERT_HDR
    for j in kr.cert_steps_for(N):
        Q, Qa, lam, V, ctl = kr.cert_step_state(n, d, j)
        assert bool((V[j + 1:] == kr.CERT_SENTINEL).all())
        G = V[:j + 1] @ V[:j + 1].T
        assert float((G - torch.eye(j + 1, dtype=torch.float64)).abs()
                     .max()) < 1e-13
        st = kr.cert_step_ref(Q, Qa, lam, V, ctl, j)
        Vc, cc = V.clone(), ctl.clone()
        cpu_ref.cert_lanczos_steps(Q, lam, Vc, cc, j, 1)
        assert float(cc[cpu_ref.CERT_COUNT]) == j + 1
        assert bool((Vc[j + 2:] == kr.CERT_SENTINEL).all())
        # the same step in longdouble
        Bl = _ld(V[:j + 1])
        wl = _s_apply_ld(Q, lam, Bl[j])
        if j > 0:
            wl -= LD(float(ctl[H + M + j - 1])) * Bl[j - 1]
        what = (d, n, j)
        _within_half(st.w0.numpy(), wl, st.b_w0.numpy(), ("w0",) + what)
        al = np.dot(Bl[j], wl)
        _within_half(st.alpha, al, st.b_alpha, ("alpha",) + what)
        _within_half(float(cc[H + j]), al, st.b_alpha, ("alpha c",) + what)
        for p in (1, 2):
            cl = Bl @ wl
            _within_half(getattr(st, f"c{p}").numpy(), cl,
                         getattr(st, f"b_c{p}").numpy(), (f"c{p}",) + what)
            wl = wl - Bl.T @ cl
            _within_half(getattr(st, f"w{p}").numpy(), wl,
                         getattr(st, f"b_w{p}").numpy(), (f"w{p}",) + what)
        b2 = (wl * wl).sum()
        bl = np.sqrt(b2)
        _within_half(st.beta2, b2, st.b_beta2, ("beta2",) + what)
        _within_half(st.beta, bl, st.b_beta, ("beta",) + what)
        _within_half(float(cc[H + M + j]), bl, st.b_beta, ("beta c",) + what)
        _within_half(st.vnext.numpy(), wl / bl, st.b_v.numpy(),
                     ("v",) + what)
        _within_half(Vc[j + 1].numpy(), wl / bl, st.b_v.numpy(),
                     ("v c",) + what)
        _sees_fault(st.b_w2, st.w2, ("w2",) + what)
        _sees_fault(st.b_v, st.vnext, ("v",) + what)
        _sees_fault(st.b_alpha, st.alpha, ("alpha",) + what)
        _sees_fault(st.b_beta, st.beta, ("beta",) + what)
        _sees_fault(st.b_beta2, st.beta2, ("beta2",) + what)
        _sees_fault(st.b_c1, st.c1, ("c1",) + what)
        # the second-pass coefficients are rounding noise themselves
        # (about eps ||w||): what their bound must see is one dropped
        # product of the Gram sum
        assert float(st.c2.abs().max()) < 64 * N * kr.EPS * st.beta
        terms = (V[:j + 1].abs() * st.w1.abs()[None, :])
        _sees_fault(st.b_c2, terms, ("c2",) + what)


@pytest.mark.parametrize("kind,tol,beta_prev", [
    ("threshold", 1e300, kr.CERT_BETA_PREV), ("zero", 0.0, 0.0),
    ("nan", 0.0, kr.CERT_BETA_PREV), ("flag", 0.0, kr.CERT_BETA_PREV)])
def test_cert_breakdown_outcomes_of_the_cpu_reference(kind, tol, beta_prev):
    """What the device tests expect of each k_cert_norm branch and of a
    raised flag is what cpu_ref.cert_lanczos_steps does."""
    d, n, j = 3, 65, 1
    M, H = kr.CERT_M, cpu_ref.CERT_HDR
    Q, _, lam, V, ctl = kr.cert_step_state(n, d, j, tol=tol,
                                           beta_prev=beta_prev)
    if kind == "zero":
        Q, lam = kr.cert_zero_matrix(n, d), torch.zeros_like(lam)
    elif kind == "nan":
        V[j, V.shape[1] - 3] = float("nan")
    elif kind == "flag":
        ctl[cpu_ref.CERT_FLAG] = 1.0
    Vc, cc = V.clone(), ctl.clone()
    cpu_ref.cert_lanczos_steps(Q, lam, Vc, cc, j, 3)
    assert bool((Vc[j + 1:] == kr.CERT_SENTINEL).all())
    assert float(cc[cpu_ref.CERT_FLAG]) == 1.0
    if kind == "flag":
        assert torch.equal(cc, ctl)
        return
    assert float(cc[H + M + j]) == 0.0
    assert float(cc[cpu_ref.CERT_COUNT]) == j + 1
    assert float(cc[H + j + 1]) == float(ctl[H + j + 1])
    assert float(cc[H + M + j + 1]) == float(ctl[H + M + j + 1])
    assert math.isnan(float(cc[H + j])) == (kind == "nan")
    if kind == "zero":
        assert float(cc[H + j]) == 0.0


def test_cert_fixed_order_sum_is_not_a_plain_sum():
    cases = kr.cert_fanin_cases()
    for p in cases.values():
        assert p.shape == (256,)
        assert (p[0], p[1], p[255]) == (1e16, 1.0, -1e16)
    s = cases["sparse"]
    assert math.fsum(s) == 1.0 and kr.cert_fixed_order_sum(s) == 0.0
    assert kr.cert_fixed_order_sum(s[:255]) == 1e16     # a dropped slot
    p = cases["dense"]
    dev = kr.cert_fixed_order_sum(p)
    naive = 0.0
    for x in p.tolist():
        naive += x
    assert dev != math.fsum(p) and dev != naive
    # another wave order is another number
    assert dev != kr.cert_fixed_order_sum(p, (3, 2, 1, 0))
    assert dev != kr.cert_fixed_order_sum(p[:255])
    # exact on exactly representable data, and a short list is padded
    q = np.arange(1.0, 201.0)
    assert kr.cert_fixed_order_sum(q) == 200 * 201 / 2
