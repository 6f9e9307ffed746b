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
