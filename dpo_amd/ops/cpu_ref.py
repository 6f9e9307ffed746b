"""PyTorch fp64 reference implementations of the dpo_amd hot ops.

Layout convention ("Xt layout", used framework-wide):
  X is a torch tensor of shape (N, r), N = (d+1) * n, fp64, where for pose
  i the rows [i*(d+1), i*(d+1)+d) hold Y_i^T (the transposed Stiefel
  component, d x r) and row i*(d+1)+d holds p_i^T (the translation, r).
  This is the transpose of the reference's r x (d+1)n matrices
  (QuadraticProblem.h:26-30); chosen so the BSR SpMM Q @ X reads/writes
  coalesced rows on the GPU.

The math mirrors:
  * tangent projection P_Y(V) = V - Y sym(Y^T V) per Stiefel block
    (ROPTLIB Stiefel projection, used at QuadraticProblem.cpp:82,95)
  * polar projection to St(d, r) = UV^T from the thin SVD
    (reference DPGO_utils.cpp:479-485)
  * Hessian-vec / gradient SpMM X*Q (QuadraticProblem.cpp:62-73), here
    Q @ Xt in the transposed layout (Q symmetric).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

Tensor = torch.Tensor


def _pose_view(X: Tensor, d: int) -> Tensor:
    """(N, r) -> (n, d+1, r) view."""
    N, r = X.shape
    dh = d + 1
    return X.view(N // dh, dh, r)


def tangent_project(X: Tensor, V: Tensor, d: int) -> Tensor:
    """Project ambient V onto the tangent space of (St(d,r) x R^r)^n at X.

    Stiefel part: P = V - Y sym(Y^T V); Euclidean rows pass through.
    In Xt layout with Yt = X-rows (d x r): S = sym(Yt @ Vt^T) (d x d),
    P_t = Vt - S @ Yt.
    """
    Xb = _pose_view(X, d)
    Vb = _pose_view(V, d).clone()
    Yt = Xb[:, :d, :]                      # (n, d, r)
    Vt = Vb[:, :d, :]
    A = torch.bmm(Yt, Vt.transpose(1, 2))  # (n, d, d) = Y^T V
    S = 0.5 * (A + A.transpose(1, 2))
    Vb[:, :d, :] = Vt - torch.bmm(S, Yt)
    return Vb.view_as(V)


def stiefel_project(M: Tensor, d: int) -> Tensor:
    """Map ambient M to the manifold: per-pose polar (= UV^T) of the Stiefel
    block; Euclidean rows unchanged. Equals the reference's per-pose
    projectToStiefelManifold (DPGO_utils.cpp:479-485,
    LiftedSEManifold.cpp:34-45)."""
    Mb = _pose_view(M, d).clone()
    Yt = Mb[:, :d, :]                      # (n, d, r), wide (d <= r)
    U, _, Vh = torch.linalg.svd(Yt, full_matrices=False)
    Mb[:, :d, :] = torch.bmm(U, Vh)
    return Mb.view_as(M)


def retract(X: Tensor, eta: Tensor, d: int) -> Tensor:
    """Polar retraction R_X(eta) = proj_manifold(X + eta)."""
    return stiefel_project(X + eta, d)


def spmm_q(Q: Tensor, X: Tensor) -> Tensor:
    """Q @ X with Q sparse CSR/COO (N, N) fp64, X (N, r)."""
    return torch.sparse.mm(Q, X)


def precond_factor(Qdiag_blocks: Tensor) -> Tensor:
    """Cholesky factors of the (regularized) diagonal blocks, (n, dh, dh)."""
    return torch.linalg.cholesky(Qdiag_blocks)


def precond_apply(L: Tensor, X: Tensor, V: Tensor, d: int) -> Tensor:
    """Block-Jacobi preconditioner: per-pose solve (LL^T) z = v followed by
    tangent projection at X (the reference applies Cholmod LDL^T of
    Q + 0.1 I then projects, QuadraticProblem.cpp:75-87; block-Jacobi is
    our GPU-friendly substitute — it only needs to precondition)."""
    dh = d + 1
    N, r = V.shape
    Vb = V.view(N // dh, dh, r)
    Z = torch.cholesky_solve(Vb, L)
    return tangent_project(X, Z.reshape(N, r), d)


def sym_block_diag(Q: Tensor, d: int, reg: float = 0.1) -> Tensor:
    """Extract (d+1)x(d+1) diagonal blocks of sparse Q, plus reg * I."""
    dh = d + 1
    N = Q.shape[0]
    n = N // dh
    Qc = Q.coalesce() if Q.layout == torch.sparse_coo else Q.to_sparse_coo().coalesce()
    idx = Qc.indices()
    val = Qc.values()
    rows, cols = idx[0], idx[1]
    bi = rows // dh
    bj = cols // dh
    mask = bi == bj
    br = rows[mask] % dh
    bc = cols[mask] % dh
    blocks = torch.zeros(n, dh, dh, dtype=Q.dtype, device=Q.device)
    blocks.index_put_((bi[mask], br, bc), val[mask], accumulate=True)
    blocks += reg * torch.eye(dh, dtype=Q.dtype, device=Q.device)
    return blocks


# ---------------------------------------------------------------------
# Optimality certificate: S = Q - Lambda(X), Lanczos with full
# reorthogonalisation (docs/DESIGN.md §14). Q is a BSRMatrix; the CPU
# path multiplies with its scalar CSR mirror.
# ---------------------------------------------------------------------
# control array: [flag, completed steps, breakdown threshold, -,
#                 alpha[0..m), beta[0..m)]
CERT_FLAG, CERT_COUNT, CERT_TOL, CERT_HDR = 0, 1, 2, 4

# (d, r) shapes the HIP extension compiles (DPO_FOREACH_DR)
CERT_SHAPES = {2: range(2, 7), 3: range(3, 9)}


def cert_check_shape(d: int, r: Optional[int]) -> None:
    """Raise ValueError for a (d, r) outside the compiled shape table
    (r = None checks d alone)."""
    if d not in CERT_SHAPES or (r is not None and r not in CERT_SHAPES[d]):
        raise ValueError(
            f"unsupported (d={d}, r={r}): compiled shapes are d=2 with "
            "r in 2..6 and d=3 with r in 3..8")


def cert_lambda(Q, Xt: Tensor, d: int) -> Tuple[Tensor, Tensor]:
    """Lambda blocks (n, d, d), Lambda_i = sym(QX_i X_i^T) on the rotation
    rows, and the 1-element tensor ||Q Xt - Lambda Xt||_F^2."""
    QX = torch.sparse.mm(Q.to_scalar_csr(), Xt)
    Xb = _pose_view(Xt, d)
    Gb = _pose_view(QX, d).clone()
    Yt = Xb[:, :d, :]
    A = torch.bmm(Gb[:, :d, :], Yt.transpose(1, 2))
    lam = 0.5 * (A + A.transpose(1, 2))
    Gb[:, :d, :] -= torch.bmm(lam, Yt)
    return lam.contiguous(), (Gb * Gb).sum().reshape(1)


def _cert_s_apply(csr: Tensor, lam: Tensor, v: Tensor) -> Tensor:
    n, d = lam.shape[0], lam.shape[1]
    w = torch.sparse.mm(csr, v[:, None])[:, 0]
    wb = w.view(n, d + 1)
    wb[:, :d] -= torch.bmm(lam, v.view(n, d + 1)[:, :d, None])[:, :, 0]
    return w


def cert_apply(Q, lam: Tensor, v: Tensor, v_prev: Optional[Tensor] = None,
               beta_prev: float = 0.0) -> Tuple[Tensor, Tensor]:
    """w = (Q - Lambda) v - beta_prev * v_prev and alpha = <v, w>."""
    w = _cert_s_apply(Q.to_scalar_csr(), lam, v)
    if v_prev is not None:
        w -= beta_prev * v_prev
    return w, torch.dot(v, w).reshape(1)


def cert_lanczos_steps(Q, lam: Tensor, V: Tensor, ctl: Tensor,
                       first_step: int, nsteps: int) -> None:
    """Lanczos steps first_step .. first_step + nsteps - 1 in place.

    V is the (m + 1, N) basis (row j = v_j, row 0 set by the caller).
    Step j forms w = S v_j - beta_{j-1} v_{j-1}, alpha_j = <v_j, w>,
    orthogonalises w against v_0..v_j twice (CGS2), then beta_j = ||w||
    and v_{j+1} = w / beta_j. When beta_j falls below ctl[CERT_TOL] the
    flag is set, beta_j is recorded as 0 and every later step is a
    no-op, so nothing divides by a vanished beta."""
    m = V.shape[0] - 1
    assert ctl.numel() == CERT_HDR + 2 * m
    assert 0 <= first_step and first_step + nsteps <= m
    csr = Q.to_scalar_csr()
    tol = float(ctl[CERT_TOL])
    for j in range(first_step, first_step + nsteps):
        if float(ctl[CERT_FLAG]) != 0.0:
            return
        w = _cert_s_apply(csr, lam, V[j])
        if j > 0:
            w -= ctl[CERT_HDR + m + j - 1] * V[j - 1]
        ctl[CERT_HDR + j] = torch.dot(V[j], w)
        B = V[:j + 1]
        for _ in range(2):
            w -= B.T @ (B @ w)
        beta = float(torch.linalg.norm(w))
        ok = beta >= tol and beta > 0.0
        ctl[CERT_HDR + m + j] = beta if ok else 0.0
        ctl[CERT_COUNT] = j + 1
        if not ok:
            ctl[CERT_FLAG] = 1.0
            return
        V[j + 1] = w / beta


# Thick-restart window (certify_solution(basis_size=b)): the same step
# inside a basis of b + 1 rows. After a restart that kept k Ritz vectors
# the caller sets ctl[CERT_COUNT] = k and zeroes beta[k - 1]; step k then
# needs no special case, because CGS2 removes the arrowhead component.
# `gram` selects the HIP Gram kernel and has no meaning on the CPU.
CERT_KEEP_MAX = 16      # k_cert_contract's compile-time column bound
CERT_BLOCK = 256        # threads per block, and most partials per sum


def cert_partials(N: int) -> int:
    """Blocks (= per-block partial slots) the certificate kernels use
    for a length-N vector."""
    return min(-(-N // CERT_BLOCK), CERT_BLOCK)


def cert_lanczos_window(Q, lam: Tensor, V: Tensor, ctl: Tensor,
                        first_step: int, nsteps: int,
                        gram: Optional[str] = None) -> None:
    """cert_lanczos_steps on the (b + 1, N) window basis V."""
    cert_lanczos_steps(Q, lam, V, ctl, first_step, nsteps)


def cert_gram_split(V: Tensor, w: Tensor, c: Tensor,
                    ctl: Optional[Tensor] = None,
                    alpha_part: Optional[Tensor] = None,
                    alpha: Optional[Tensor] = None) -> None:
    """c[:] = V[:len(c)] @ w and, with `alpha`, alpha[0] = the sum of the
    cert_partials(N) partials in alpha_part. A raised ctl[CERT_FLAG]
    leaves both untouched."""
    if ctl is not None and float(ctl[CERT_FLAG]) != 0.0:
        return
    c.copy_(V[:c.numel()] @ w)
    if alpha is not None:
        alpha[0] = alpha_part[:cert_partials(w.numel())].sum()


def cert_contract(V: Tensor, C: Tensor) -> None:
    """Thick-restart contraction of the (b + 1, N) basis with the (b, k)
    Ritz coefficients C: V[:k] = C^T @ V[:b] (out of place, then stored)
    and V[k] = V[b]. Rows past k keep stale data."""
    b, k = C.shape
    assert V.shape[0] == b + 1 and 1 <= k <= min(b, CERT_KEEP_MAX)
    new = C.T.to(V.dtype) @ V[:b]
    carry = V[b].clone()
    V[:k] = new
    V[k] = carry


# ---------------------------------------------------------------------
# refine: global Riemannian trust region on f(X) = 0.5 <Q, X^T X>
# (docs/DESIGN.md §17). The control array mirrors RefSlot in dpo_ops.hip;
# the functions below are the fp64 reference of the HIP stages, with the
# scalar steps in the order of k_ref_ctl.
# ---------------------------------------------------------------------
(RF_STATUS, RF_FX, RF_GN2, RF_RR, RF_ZR, RF_EPE, RF_EPD, RF_DPD, RF_COEF,
 RF_BETA, RF_ITER, RF_RADIUS, RF_BOUND, RF_DM, RF_STOP, RF_TCG, RF_FPROP,
 RF_RHO, RF_ACCEPTED, RF_GRAD_TOL, RF_MAX_INNER, RF_MAX_RADIUS, RF_OUTER,
 RF_INNER, RF_REJECTED, RF_STREAK, RF_HIT, RF_DHD) = range(28)
RF_SIZE = 32
RS_RUN, RS_TCG_DONE, RS_CONVERGED, RS_HEAD = range(4)
RT_NONE, RT_CONVERGED, RT_EXCEEDED_TR, RT_NEG_CURV, RT_MAX_INNER = range(5)
REFINE_TCG_NAMES = ("none", "converged", "exceeded_tr", "negative_curvature",
                    "max_inner")
# workspace vectors, in the order the HIP entry point takes them
REFINE_BUFS = ("X", "Xp", "QV", "grad", "eta", "r", "z", "delta", "Hd")


class RefineWorkspace:
    """Caller-owned buffers of one refinement: the nine (N, r) vectors of
    REFINE_BUFS (X is the iterate, a copy of the Xt given) and the
    per-block partial slots of the HIP kernels."""

    def __init__(self, Xt: Tensor):
        assert Xt.dim() == 2 and Xt.dtype == torch.float64
        self.X = Xt.detach().clone().contiguous()
        for name in REFINE_BUFS[1:]:
            setattr(self, name, torch.zeros_like(self.X))
        self.part = torch.zeros(2 * CERT_BLOCK, dtype=torch.float64,
                                device=Xt.device)

    def bufs(self):
        return [getattr(self, name) for name in REFINE_BUFS]


def refine_control(grad_tol: float, Delta0: float, max_inner: int,
                   device="cpu") -> Tensor:
    """A fresh control array: status RS_HEAD, radius Delta0 (capped at
    5 Delta0 when it grows), everything else zero."""
    if max_inner < 1:
        raise ValueError("max_inner must be at least 1")
    h = torch.zeros(RF_SIZE, dtype=torch.float64)
    h[RF_STATUS] = RS_HEAD
    h[RF_GRAD_TOL] = grad_tol
    h[RF_RADIUS] = Delta0
    h[RF_MAX_RADIUS] = 5.0 * Delta0
    h[RF_MAX_INNER] = max_inner
    return h.to(device)


def _refine_precond(pre, X: Tensor, V: Tensor, d: int) -> Tensor:
    """z = P_X(M^-1 V); pre = (mode, data): ("jacobi", L (n, dh, dh)),
    ("dense", Minv (N, N) fp32) or, CPU only, ("exact", scipy splu)."""
    mode, data = pre
    if mode == "jacobi":
        return precond_apply(data, X, V, d)
    if mode == "dense":
        # fp32 storage, fp64 accumulation, as k_precond_dense
        Z = data.to(torch.float64) @ V
    elif mode == "exact":
        Z = torch.from_numpy(data.solve(V.numpy()))
    else:
        raise ValueError(f"unknown preconditioner mode {mode!r}")
    return tangent_project(X, Z, d)


def _dot(a: Tensor, b: Tensor) -> float:
    return float((a * b).sum())


def refine_hd_stage(Q, ws: RefineWorkspace, ctl: Tensor, d: int) -> None:
    """Hd = P_X(Q delta) and part[0] = <delta, Hd> (status RS_RUN only;
    the HIP version leaves per-block partials in ws.part instead)."""
    if float(ctl[RF_STATUS]) != RS_RUN:
        return
    ws.QV.copy_(torch.sparse.mm(Q.to_scalar_csr(), ws.delta))
    ws.Hd.copy_(tangent_project(ws.X, ws.QV, d))
    ws.part[0] = _dot(ws.delta, ws.Hd)


def refine_head(Q, ws: RefineWorkspace, ctl: Tensor, d: int, pre) -> None:
    """Head of an outer step (status RS_HEAD only): grad = P_X(Q X), f,
    ||grad||^2, the tCG bound; status RS_CONVERGED when ||grad|| <=
    grad_tol, else RS_RUN with r = grad, eta = 0, z0 and delta0 = -z0."""
    if float(ctl[RF_STATUS]) != RS_HEAD:
        return
    ws.QV.copy_(torch.sparse.mm(Q.to_scalar_csr(), ws.X))
    s0 = _dot(ws.QV, ws.X)
    ws.grad.copy_(tangent_project(ws.X, ws.QV, d))
    ws.r.copy_(ws.grad)
    ws.eta.zero_()
    s1 = _dot(ws.grad, ws.grad)
    nr0 = s1 ** 0.5
    ctl[RF_FX] = 0.5 * s0
    ctl[RF_GN2] = s1
    ctl[RF_RR] = s1
    ctl[RF_BOUND] = nr0 * min(nr0, 0.1)
    # RF_TCG keeps how the last tCG ended until the next one ends
    for slot in (RF_EPE, RF_EPD, RF_COEF, RF_BETA, RF_ITER, RF_DM, RF_STOP,
                 RF_HIT):
        ctl[slot] = 0.0
    if nr0 <= float(ctl[RF_GRAD_TOL]):
        ctl[RF_STATUS] = RS_CONVERGED
        return
    ctl[RF_STATUS] = RS_RUN
    ws.z.copy_(_refine_precond(pre, ws.X, ws.r, d))
    zr = _dot(ws.z, ws.r)
    ctl[RF_ZR] = zr
    ctl[RF_DPD] = zr
    ws.delta.copy_(-ws.z)


def refine_tcg_steps(Q, ws: RefineWorkspace, ctl: Tensor, d: int, pre,
                     nsteps: int) -> None:
    """nsteps tCG iterations, each a no-op unless the status is RS_RUN.
    An iteration that meets the boundary or negative curvature, converges
    or reaches max_inner sets RS_TCG_DONE and RF_TCG."""
    for _ in range(nsteps):
        if float(ctl[RF_STATUS]) != RS_RUN:
            return
        refine_hd_stage(Q, ws, ctl, d)
        c = ctl.tolist()
        d_Hd, z_r = float(ws.part[0]), c[RF_ZR]
        e_Pe, e_Pd, d_Pd = c[RF_EPE], c[RF_EPD], c[RF_DPD]
        rad2 = c[RF_RADIUS] * c[RF_RADIUS]
        if d_Hd != 0.0:
            alpha = z_r / d_Hd
        else:   # IEEE division, as on the device
            alpha = float("nan") if z_r == 0.0 or z_r != z_r else \
                float("inf") * (1.0 if z_r > 0 else -1.0)
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        ctl[RF_DHD] = d_Hd
        ctl[RF_ITER] = c[RF_ITER] + 1.0
        ctl[RF_INNER] = c[RF_INNER] + 1.0
        if d_Hd <= 0.0 or e_Pe_new >= rad2:
            disc = e_Pd * e_Pd + d_Pd * (rad2 - e_Pe)
            tau = (-e_Pd + max(disc, 0.0) ** 0.5) / d_Pd if d_Pd > 0.0 \
                else 0.0
            ctl[RF_COEF] = tau
            ctl[RF_DM] = c[RF_DM] + (tau * z_r - 0.5 * tau * tau * d_Hd)
            ctl[RF_STOP] = 1.0
            ctl[RF_TCG] = RT_NEG_CURV if d_Hd <= 0.0 else RT_EXCEEDED_TR
            ws.eta.add_(ws.delta, alpha=tau)
            ctl[RF_HIT] = 1.0
            ctl[RF_STATUS] = RS_TCG_DONE
            return
        ctl[RF_COEF] = alpha
        ctl[RF_EPE] = e_Pe_new
        ctl[RF_DM] = c[RF_DM] + 0.5 * alpha * z_r
        ws.eta.add_(ws.delta, alpha=alpha)
        ws.r.add_(ws.Hd, alpha=alpha)
        rr = _dot(ws.r, ws.r)
        ctl[RF_RR] = rr
        if rr ** 0.5 <= c[RF_BOUND]:
            ctl[RF_TCG] = RT_CONVERGED
            ctl[RF_STATUS] = RS_TCG_DONE
            return
        if c[RF_ITER] + 1.0 >= c[RF_MAX_INNER]:
            ctl[RF_TCG] = RT_MAX_INNER
            ctl[RF_STATUS] = RS_TCG_DONE
            return
        ws.z.copy_(_refine_precond(pre, ws.X, ws.r, d))
        zr_new = _dot(ws.z, ws.r)
        beta = zr_new / z_r
        ctl[RF_BETA] = beta
        ctl[RF_EPD] = beta * (e_Pd + alpha * d_Pd)
        ctl[RF_DPD] = zr_new + beta * beta * d_Pd
        ctl[RF_ZR] = zr_new
        ws.delta.mul_(beta).sub_(ws.z)


def refine_candidate(Q, ws: RefineWorkspace, ctl: Tensor, d: int) -> None:
    """Candidate stage (status RS_TCG_DONE only): Xp = retract(X, eta),
    f(Xp), rho, the radius update and the acceptance test; an accepted Xp
    is copied into X. Leaves status RS_HEAD."""
    if float(ctl[RF_STATUS]) != RS_TCG_DONE:
        return
    ws.Xp.copy_(retract(ws.X, ws.eta, d))
    ws.QV.copy_(torch.sparse.mm(Q.to_scalar_csr(), ws.Xp))
    c = ctl.tolist()
    fprop, fX = 0.5 * _dot(ws.QV, ws.Xp), c[RF_FX]
    rho = (fX - fprop) / max(c[RF_DM], 1e-300)
    ctl[RF_FPROP] = fprop
    ctl[RF_RHO] = rho
    if rho < 0.25:
        ctl[RF_RADIUS] = c[RF_RADIUS] * 0.25
    elif rho > 0.75 and c[RF_HIT] != 0.0:
        ctl[RF_RADIUS] = min(2.0 * c[RF_RADIUS], c[RF_MAX_RADIUS])
    acc = rho > 0.1 and fprop <= fX
    ctl[RF_ACCEPTED] = 1.0 if acc else 0.0
    ctl[RF_STREAK] = 0.0 if acc else c[RF_STREAK] + 1.0
    if not acc:
        ctl[RF_REJECTED] = c[RF_REJECTED] + 1.0
    ctl[RF_OUTER] = c[RF_OUTER] + 1.0
    ctl[RF_STATUS] = RS_HEAD
    if acc:
        ws.X.copy_(ws.Xp)


# ---------------------------------------------------------------------
# rounding: the lifted iterate to SE(d) (docs/DESIGN.md §19). Batched
# torch, no loop over poses; the HIP kernels use another algorithm
# (closed form / Jacobi on the Davenport matrix) for the same maximiser.
# ---------------------------------------------------------------------
def project_to_rotations(B: Tensor) -> Tensor:
    """argmax_{R in SO(d)} tr(R^T B) for every block of B (n, d, d):
    U V^T of the SVD with the determinant fix on U's last column."""
    U, _, Vh = torch.linalg.svd(B)
    neg = torch.linalg.det(U) * torch.linalg.det(Vh) < 0
    U = U.clone()
    U[neg, :, -1] *= -1.0
    return torch.bmm(U, Vh)


def _round_blocks(Xt: Tensor, d: int, U: Tensor):
    """U^T Y_i (n, d, d) and U^T p_i (n, d)."""
    r = Xt.shape[1]
    cert_check_shape(d, r)
    assert U.shape == (r, d)
    Xb = _pose_view(Xt, d)
    P = Xb @ U.to(Xt.dtype)                 # (n, d+1, d), row a = (U^T y_a)^T
    return P[:, :d, :].transpose(1, 2), P[:, d, :]


def round_gram(Xt: Tensor, d: int) -> Tensor:
    """S = sum_i Y_i Y_i^T (r, r) over the rotation rows."""
    cert_check_shape(d, Xt.shape[1])
    Yt = _pose_view(Xt, d)[:, :d, :].reshape(-1, Xt.shape[1])
    return Yt.T @ Yt


def round_poses(Xt: Tensor, d: int, U: Tensor, t0: Tensor,
                flip: bool = False):
    """(traj (d, n (d+1)), Xr (n (d+1), d)): R_i = the SO(d) projection of
    U^T Y_i, t_i = U^T p_i - t0; `flip` negates U's last column."""
    if flip:
        U = U.clone()
        U[:, -1] *= -1.0
    B, t = _round_blocks(Xt, d, U)
    n = B.shape[0]
    out = torch.empty(n, d + 1, d, dtype=Xt.dtype)
    out[:, :d, :] = project_to_rotations(B).transpose(1, 2)
    out[:, d, :] = t - t0.to(Xt.dtype)
    Xr = out.view(n * (d + 1), d)
    return Xr.T.contiguous(), Xr


def round_reflections(Xt: Tensor, d: int, U: Tensor) -> Tensor:
    """1-element int32 tensor: poses with det(U^T Y_i) < 0."""
    B, _ = _round_blocks(Xt, d, U)
    neg = torch.linalg.slogdet(B)[0] < 0
    return neg.sum().to(torch.int32).reshape(1)


def round_gauge(Xr: Tensor, traj: Tensor, d: int, anchor_pose: int) -> None:
    """In place on both layouts: R_i <- R_a^T R_i, t_i <- R_a^T (t_i -
    t_a) for a = anchor_pose."""
    cert_check_shape(d, d)
    dh = d + 1
    Xb = Xr.view(-1, dh, d)
    A = Xb[anchor_pose].clone()
    Xb[:, d, :] -= A[d]
    Ra = A[:d].T                            # Xt layout holds R_a^T
    Xb.copy_(Xb @ Ra)                       # rows v^T -> (R_a^T v)^T
    traj.copy_(Xr.T)


def round_cost(Q, X: Tensor, G: Optional[Tensor] = None) -> Tensor:
    """1-element tensor f(X) = 0.5 <Q X, X> + <X, G>."""
    f = 0.5 * (torch.sparse.mm(Q.to_scalar_csr(), X) * X).sum()
    if G is not None:
        f = f + (X * G).sum()
    return f.reshape(1)


# ---------------------------------------------------------------------
# Certificate, second eigensolver: LOBPCG with a Gram-based
# Rayleigh-Ritz step (docs/DESIGN.md §20). The control array mirrors
# LobSlot in dpo_ops.hip; the functions below are the fp64 reference of
# the HIP ops. Blocks are row-major (N, m); B = [X W P] and SB = [SX SW
# SP] are (3, N, m) tensors.
# ---------------------------------------------------------------------
LOB_STATUS, LOB_THETA, LOB_COEF = 0, 4, 12
LOB_MAX_M = 8
LOB_SIZE = LOB_COEF + (3 * LOB_MAX_M) * (2 * LOB_MAX_M)
LOB_X, LOB_W, LOB_P = 0, 1, 2           # block numbers inside B and SB
# partial slots of the HIP kernels: Gram tiles, then residual columns
LOB_GPART = 24 * LOB_MAX_M * 4 * CERT_BLOCK
LOB_RPART = LOB_MAX_M * CERT_BLOCK


class LobWorkspace:
    """Caller-owned buffers of one LOBPCG run with block size m: B and SB
    (3, N, m), the residual block R (N, m) (seven blocks in all), the
    control array, the partial slots and `out` = [G_B (3m, 3m), G_A
    (3m, 3m), squared residual norms (m)], which the host reads once per
    iteration."""

    def __init__(self, N: int, m: int, device="cpu"):
        if not 1 <= m <= LOB_MAX_M:
            raise ValueError(f"block size {m} outside 1..{LOB_MAX_M}")
        kw = dict(dtype=torch.float64, device=device)
        self.N, self.m = N, m
        self.B = torch.zeros(3, N, m, **kw)
        self.SB = torch.zeros(3, N, m, **kw)
        self.R = torch.zeros(N, m, **kw)
        self.ctl = torch.zeros(LOB_SIZE, **kw)
        self.part = torch.zeros(LOB_GPART + LOB_RPART, **kw)
        self.out = torch.zeros(2 * 9 * m * m + m, **kw)

    def unpack(self, h=None):
        """(G_B, G_A, rn2) as numpy arrays from `out` (or a host copy h),
        G_B and G_A symmetrised from their upper triangles."""
        import numpy as np
        if h is None:
            h = self.out.cpu().numpy()
        k = 3 * self.m
        mats = []
        for a in range(2):
            U = np.triu(h[a * k * k:(a + 1) * k * k].reshape(k, k))
            mats.append(U + np.triu(U, 1).T)
        return mats[0], mats[1], h[2 * k * k:].copy()


def lob_set_coefficients(ctl_host: Tensor, theta, C, m: int) -> None:
    """Fill a host copy of the control array: theta (m) and C (3m, 2m)."""
    ctl_host[LOB_THETA:LOB_THETA + m] = torch.as_tensor(
        theta, dtype=torch.float64)
    ctl_host[LOB_COEF:LOB_COEF + 6 * m * m] = torch.as_tensor(
        C, dtype=torch.float64).reshape(-1)


def _lob_run(ws: LobWorkspace) -> bool:
    return float(ws.ctl[LOB_STATUS]) == 0.0


def cert_lob_resid(ws: LobWorkspace, zero: bool = False) -> None:
    """R = SX - X diag(theta) and the squared column norms, left in the
    residual slots of ws.part (slot 0 of each column here; per-block
    partials on the device). `zero` clears W."""
    if not _lob_run(ws):
        return
    m = ws.m
    theta = ws.ctl[LOB_THETA:LOB_THETA + m]
    torch.sub(ws.SB[LOB_X], ws.B[LOB_X] * theta, out=ws.R)
    npart = cert_partials(ws.N)
    rp = ws.part[LOB_GPART:LOB_GPART + m * npart].view(m, npart)
    rp.zero_()
    rp[:, 0] = (ws.R * ws.R).sum(dim=0)
    if zero:
        ws.B[LOB_W].zero_()


def lob_precond(pre, V: Tensor, d: int) -> Tensor:
    """T V for pre = (mode, data) as in `_refine_precond`, without the
    tangent projection: the eigenproblem lives in R^N."""
    mode, data = pre
    N, m = V.shape
    if mode == "jacobi":
        Z = torch.cholesky_solve(V.view(N // (d + 1), d + 1, m), data)
        return Z.reshape(N, m)
    if mode == "dense":
        return data.to(torch.float64) @ V
    if mode == "exact":
        return torch.from_numpy(data.solve(V.numpy()))
    raise ValueError(f"unknown preconditioner mode {mode!r}")


def cert_lob_precond(ws: LobWorkspace, pre, d: int) -> None:
    """W = T R."""
    if _lob_run(ws):
        ws.B[LOB_W].copy_(lob_precond(pre, ws.R, d))


def cert_lob_apply(Q, lam: Tensor, ws: LobWorkspace, blk: int) -> None:
    """SB[blk] = (Q - Lambda) B[blk]."""
    if not _lob_run(ws):
        return
    n, d = lam.shape[0], lam.shape[1]
    V = ws.B[blk]
    out = torch.sparse.mm(Q.to_scalar_csr(), V)
    ob = out.view(n, d + 1, ws.m)
    ob[:, :d, :] -= torch.bmm(lam, V.view(n, d + 1, ws.m)[:, :d, :])
    ws.SB[blk].copy_(out)


def cert_lob_gram(ws: LobWorkspace) -> None:
    """out = [B^T B, B^T SB, squared residual norms]."""
    if not _lob_run(ws):
        return
    m, k = ws.m, 3 * ws.m
    Bf = ws.B.permute(1, 0, 2).reshape(ws.N, k)
    SBf = ws.SB.permute(1, 0, 2).reshape(ws.N, k)
    ws.out[:k * k] = (Bf.T @ Bf).reshape(-1)
    ws.out[k * k:2 * k * k] = (Bf.T @ SBf).reshape(-1)
    npart = cert_partials(ws.N)
    rp = ws.part[LOB_GPART:LOB_GPART + m * npart].view(m, npart)
    ws.out[2 * k * k:] = rp.sum(dim=1)


def cert_lob_update(ws: LobWorkspace) -> None:
    """X <- [X W P] C[:, :m], P <- [W P] C[m:, m:], and SX, SP from SB
    with the same coefficients (out of place, then stored)."""
    if not _lob_run(ws):
        return
    m, k = ws.m, 3 * ws.m
    C = ws.ctl[LOB_COEF:LOB_COEF + k * 2 * m].view(k, 2 * m)
    for T in (ws.B, ws.SB):
        Tf = T.permute(1, 0, 2).reshape(ws.N, k)
        newx = Tf @ C[:, :m]
        newp = Tf[:, m:] @ C[m:, m:]
        T[LOB_X].copy_(newx)
        T[LOB_P].copy_(newp)


def cert_lob_iter(Q, lam: Tensor, ws: LobWorkspace, pre) -> None:
    """The device half of one iteration: residual, W = T R, SW = S W and
    the Gram matrices."""
    d = lam.shape[1]
    cert_lob_resid(ws, zero=pre[0] == "dense")
    cert_lob_precond(ws, pre, d)
    cert_lob_apply(Q, lam, ws, LOB_W)
    cert_lob_gram(ws)
