"""References, input builders and tolerance helpers of the kernel test
matrix (tests/test_kernel_matrix.py). Plain fp64 NumPy / torch on the
CPU, importable without a GPU; tests/test_kernel_refs.py checks the
helpers themselves.

Tolerance rule (docs/DESIGN.md, "Kernel test matrix"):
  * anything that is a sum of K products sum_i a_i b_i is compared under
    the classical bound |gpu - ref| <= 2 K eps sum_i |a_i||b_i|, which
    holds for every summation order and with or without FMA contraction
    (each side is within K (eps / 2) sum|a||b| of the exact value, the
    factor 2 is head room). sop_bound() computes it from abs() copies of
    the operands.
  * the tangent projection propagates that bound through its two small
    products (tangent_project_bound()).
  * the block-Jacobi solve uses the forward error bound of a backward
    stable solve, cond(block) 64 eps ||v|| (jacobi_tol()).
  * the polar projection uses the error model of the Newton-Schulz
    iteration on the Gram matrix, 8 eps cond(M)^2 + 16 eps (polar_tol()).
None of these is fitted to what the kernels return.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from dpo_amd.ops import cpu_ref
from dpo_amd.quadratic import BSRMatrix

Tensor = torch.Tensor

EPS = float(np.finfo(np.float64).eps)

# the (d, r) pairs the HIP extension compiles, read from the one table
SHAPES = [(d, r) for d in sorted(cpu_ref.CERT_SHAPES)
          for r in cpu_ref.CERT_SHAPES[d]]
RS = sorted({r for _, r in SHAPES})

# thread-per-pose kernels: one thread, a partly filled block, one full
# 256-thread block, and one thread in a second block
N_POSE = (1, 65, 256, 257)


def poses_per_block(d: int, r: int) -> int:
    """Poses per 256-thread block of the tile-per-pose kernels."""
    return 256 // ((d + 1) * r)


def n_tile(d: int, r: int):
    """Pose counts for tile-per-pose kernels: one pose, one full block,
    one pose in a second block, a fourth block with one pose, 257."""
    pb = poses_per_block(d, r)
    return tuple(sorted({1, pb, pb + 1, 3 * pb + 1, 257}))


def gen(*key) -> torch.Generator:
    """Fixed per-case generator."""
    seed = 1469598103
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def randn(g, *shape) -> Tensor:
    return torch.randn(*shape, dtype=torch.float64, generator=g)


# ---------------------------------------------------------------------
# sum-of-products bound
# ---------------------------------------------------------------------
def sop_bound(abs_sum, K: int):
    """2 K eps S for S = sum |a_i||b_i| (tensor or float), K terms."""
    return 2.0 * K * EPS * abs_sum


def matmul_bound(A: Tensor, B: Tensor, K: int) -> Tensor:
    """Entry-wise bound for A @ B with at most K accumulated terms."""
    return sop_bound(A.abs() @ B.abs(), K)


def dot_bound(a: Tensor, b: Tensor) -> float:
    return float(sop_bound((a.abs() * b.abs()).sum(), a.numel()))


def tangent_project_bound(X: Tensor, A: Tensor, d: int,
                          bA: Optional[Tensor] = None) -> Tensor:
    """Entry-wise bound for P = A - sym(Y A^T) Y at X (Y = Stiefel rows),
    given an entry-wise bound bA on the error already in A. Propagates
    the sum-of-products bound through S = sym(Y A^T) (r terms) and S Y
    (d terms); the final subtraction adds one rounding of the result."""
    N, r = A.shape
    dh = d + 1
    if bA is None:
        bA = torch.zeros_like(A)
    Yb = X.view(-1, dh, r)[:, :d, :].abs()
    Ab = A.view(-1, dh, r)[:, :d, :].abs()
    bAb = bA.view(-1, dh, r)[:, :d, :]
    # |delta S| <= sym(|Y| bA^T) + 2 r eps sym(|Y||A|^T)
    YA = torch.bmm(Yb, Ab.transpose(1, 2))
    Sabs = 0.5 * (YA + YA.transpose(1, 2))
    YbA = torch.bmm(Yb, bAb.transpose(1, 2))
    dS = 0.5 * (YbA + YbA.transpose(1, 2)) + sop_bound(Sabs, r + 1)
    SY = torch.bmm(Sabs, Yb)
    out = bA.clone().view(-1, dh, r)
    out[:, :d, :] += torch.bmm(dS, Yb) + sop_bound(SY, d + 1) \
        + EPS * (Ab + SY)
    return out.view(N, r)


# ---------------------------------------------------------------------
# block-sparse test matrices
# ---------------------------------------------------------------------
def random_bsr(n: int, dh: int, g: torch.Generator, hub_degree: int = 40):
    """Symmetric BSRMatrix with random fp64 blocks (B_ji = B_ij^T; not
    PSD): every diagonal block, a chain, about n random extra pairs and
    one hub pose with about hub_degree neighbours, so that row lengths
    vary from 2 to more than 40."""
    pairs = {(i, i) for i in range(n)}
    pairs |= {(i, i + 1) for i in range(n - 1)}
    if n > 2:
        ij = torch.randint(0, n, (n, 2), generator=g).tolist()
        pairs |= {(min(i, j), max(i, j)) for i, j in ij if i != j}
        hub = n // 3
        nb = torch.randperm(n, generator=g)[:min(hub_degree, n - 1) + 1]
        pairs |= {(min(hub, j), max(hub, j)) for j in nb.tolist() if j != hub}
    upper = sorted(pairs)
    blocks = randn(g, len(upper), dh, dh)
    rows = {}
    for (i, j), B in zip(upper, blocks):
        if i == j:
            rows.setdefault(i, {})[i] = 0.5 * (B + B.T)
        else:
            rows.setdefault(i, {})[j] = B
            rows.setdefault(j, {})[i] = B.T
    row_ptr = [0]
    col_idx = []
    vals = []
    for i in range(n):
        for j in sorted(rows[i]):
            col_idx.append(j)
            vals.append(rows[i][j])
        row_ptr.append(len(col_idx))
    return BSRMatrix(n, dh,
                     torch.tensor(row_ptr, dtype=torch.int32),
                     torch.tensor(col_idx, dtype=torch.int32),
                     torch.stack(vals).contiguous())


def bsr_max_row_terms(Q: BSRMatrix) -> int:
    """Most products accumulated into one output entry of Q @ V."""
    rp = Q.row_ptr.cpu().numpy()
    return int(np.diff(rp).max()) * Q.dh


def manifold_point(n: int, d: int, r: int, g: torch.Generator) -> Tensor:
    return cpu_ref.stiefel_project(randn(g, (d + 1) * n, r), d)


# ---------------------------------------------------------------------
# polar projection: error model, emulation, inputs
# ---------------------------------------------------------------------
POLAR_CONDS = (1.0, 1e2, 1e4)
POLAR_SCALES = (1e-3, 1.0, 1e3)
RETRACT_ETA_NORMS = (1e-8, 1e-2, 1.0, 1e2)


def polar_tol(cond):
    """Error model of the GPU polar projection: it forms the Gram matrix
    M M^T, whose condition number is cond(M)^2, and iterates on it in
    fp64, so the factor is accurate to a multiple of eps cond(M)^2."""
    return 8.0 * EPS * np.asarray(cond, dtype=np.float64) ** 2 + 16.0 * EPS


def block_conds(M: Tensor, d: int) -> np.ndarray:
    """cond of the d x r Stiefel block of every pose."""
    s = torch.linalg.svdvals(M.view(-1, d + 1, M.shape[1])[:, :d, :])
    return (s[:, 0] / s[:, -1]).numpy()


def polar_emulation(M: Tensor, d: int) -> Tensor:
    """NumPy emulation of the algorithm the GPU polar projection uses:
    coupled Newton-Schulz iteration for Gram^{-1/2} on the trace-scaled
    d x d Gram matrix, at most 40 iterations, stopped when the update
    factor is the identity to 1e-15; result Gram^{-1/2} M. A vanishing
    Gram trace gives a zero block. Translation rows pass through."""
    r = M.shape[1]
    Mb = M.view(-1, d + 1, r).numpy().copy()
    Y = Mb[:, :d, :]
    S = Y @ Y.transpose(0, 2, 1)
    tr = np.trace(S, axis1=1, axis2=2)
    ok = tr > 1e-300
    I = np.broadcast_to(np.eye(d), S.shape)
    with np.errstate(all="ignore"):
        Yk = S / np.where(ok, tr, 1.0)[:, None, None]
        Zk = I.copy()
        active = ok.copy()
        for _ in range(40):
            if not active.any():
                break
            T = 0.5 * (3.0 * I - Zk @ Yk)
            Yn, Zn = Yk @ T, T @ Zk
            Yk = np.where(active[:, None, None], Yn, Yk)
            Zk = np.where(active[:, None, None], Zn, Zk)
            active &= ~(((T - I) ** 2).sum(axis=(1, 2)) < 1e-30)
        out = (Zk / np.sqrt(np.where(ok, tr, 1.0))[:, None, None]) @ Y
    out[~ok] = 0.0
    Mb[:, :d, :] = out
    return torch.from_numpy(Mb).view_as(M)


def polar_errors(out: Tensor, M: Tensor, d: int):
    """Per pose: max |out - SVD polar| and ||Y Y^T - I||_inf on the
    Stiefel rows; max relative deviation of the translation rows."""
    r = M.shape[1]
    ref = cpu_ref.stiefel_project(M, d).view(-1, d + 1, r)
    ob = out.view(-1, d + 1, r)
    err = (ob[:, :d] - ref[:, :d]).abs().amax(dim=(1, 2)).numpy()
    G = torch.bmm(ob[:, :d], ob[:, :d].transpose(1, 2)) - torch.eye(
        d, dtype=torch.float64)
    orth = G.abs().sum(dim=2).amax(dim=1).numpy()
    return err, orth


def cond_blocks(n: int, d: int, r: int, cond: float, scale: float,
                g: torch.Generator) -> Tensor:
    """(N, r) input whose Stiefel blocks are U diag(s) V^T with singular
    values log-spaced in [scale / cond, scale]; Gaussian translations."""
    U = torch.linalg.qr(randn(g, n, d, d))[0]
    V = torch.linalg.qr(randn(g, n, r, d))[0]
    s = scale * torch.logspace(0.0, -math.log10(cond), d,
                               dtype=torch.float64)
    M = randn(g, n, d + 1, r)
    M[:, :d, :] = torch.bmm(U * s[None, None, :], V.transpose(1, 2))
    return M.reshape(n * (d + 1), r).contiguous()


def retraction_inputs(n: int, d: int, r: int, eta_norm: float,
                      g: torch.Generator):
    """X on the manifold and a tangent eta with per-pose Stiefel-block
    Frobenius norm eta_norm. Tangency makes Y eta^T skew, so the Gram
    matrix of Y + eta is I + eta eta^T and cond(Y + eta) <=
    sqrt(1 + eta_norm^2): the retraction stays inside the domain of the
    Gram-matrix iteration for every step length."""
    X = manifold_point(n, d, r, g)
    eta = cpu_ref.tangent_project(X, randn(g, (d + 1) * n, r), d)
    eb = eta.view(n, d + 1, r)
    nrm = eb[:, :d, :].flatten(1).norm(dim=1)
    eb[:, :d, :] *= (eta_norm / nrm)[:, None, None]
    return X, eta.contiguous()


POLAR_N = 257  # conditioning cases: two blocks of the per-pose kernel
POLAR_ABC = (1.7, -0.7, 0.3)


def polar_form_inputs(d: int, r: int, n: int):
    """Operands of the three polar_affine forms at one (shape, n):
    {form: (A, B, C, ca, cb, cc)}. 1-operand: a Gaussian matrix;
    2-operand: the retraction X + eta; 3-operand: the Nesterov-style
    combination 1.7 A - 0.7 B + 0.3 C of a manifold point and two
    Gaussian matrices."""
    g = gen(3, d, r, n)
    N = (d + 1) * n
    X = manifold_point(n, d, r, g)
    eta = 0.3 * cpu_ref.tangent_project(X, randn(g, N, r), d)
    ca, cb, cc = POLAR_ABC
    return {
        "one": (randn(g, N, r), None, None, 1.0, 0.0, 0.0),
        "two": (X, eta, None, 1.0, 1.0, 0.0),
        "three": (X, randn(g, N, r), randn(g, N, r), ca, cb, cc),
    }


def affine(A, B, C, ca, cb, cc) -> Tensor:
    M = ca * A
    if B is not None:
        M = M + cb * B
    if C is not None:
        M = M + cc * C
    return M


def polar_cond_cases(d: int, r: int):
    """[(label, M)]: constructed-spectrum blocks, every cond x scale."""
    out = []
    for ci, cond in enumerate(POLAR_CONDS):
        for si, scale in enumerate(POLAR_SCALES):
            g = gen(4, d, r, ci, si)
            out.append((f"cond{cond:g}-scale{scale:g}", cond,
                        cond_blocks(POLAR_N, d, r, cond, scale, g)))
    return out


def polar_retract_cases(d: int, r: int):
    """[(label, cond bound, X, eta)] for every step length."""
    out = []
    for ei, en in enumerate(RETRACT_ETA_NORMS):
        X, eta = retraction_inputs(POLAR_N, d, r, en, gen(5, d, r, ei))
        out.append((f"eta{en:g}", math.sqrt(1.0 + en * en), X, eta))
    return out


# ---------------------------------------------------------------------
# block-Jacobi
# ---------------------------------------------------------------------
JACOBI_CONDS = (1.0, 1e3, 1e6)


def spd_blocks(n: int, dh: int, g: torch.Generator) -> Tensor:
    """(n, dh, dh) SPD blocks W diag(lam) W^T with lam log-spaced in
    [1, cond], cond cycling through JACOBI_CONDS over the poses. The
    smallest eigenvalue is 1, so ||A^-1|| = 1 and ||x|| <= ||v||."""
    W = torch.linalg.qr(randn(g, n, dh, dh))[0]
    conds = torch.tensor([JACOBI_CONDS[i % len(JACOBI_CONDS)]
                          for i in range(n)], dtype=torch.float64)
    t = torch.linspace(0.0, 1.0, dh, dtype=torch.float64)
    lam = conds[:, None] ** t[None, :]
    A = torch.bmm(W * lam[:, None, :], W.transpose(1, 2))
    return 0.5 * (A + A.transpose(1, 2))


def jacobi_tol(blocks: Tensor, V: Tensor) -> Tensor:
    """(N, r) tolerance cond(block) 64 eps ||v||, ||v|| the 2-norm of the
    pose's right-hand-side column: the forward error cond eps ||x|| of a
    backward-stable solve, with ||x|| <= ||A^-1|| ||v|| = ||v|| for the
    blocks of spd_blocks()."""
    n, dh, _ = blocks.shape
    r = V.shape[1]
    ev = torch.linalg.eigvalsh(blocks)
    cond = ev[:, -1] / ev[:, 0]
    vn = V.view(n, dh, r).norm(dim=1)                    # (n, r)
    tol = 64.0 * EPS * cond[:, None] * vn
    return tol[:, None, :].expand(n, dh, r).reshape(n * dh, r)


# ---------------------------------------------------------------------
# GNC-TLS weights
# ---------------------------------------------------------------------
def gnc_residual_sq(P1, P2, R, t, kappa, tau, d):
    """r^2 = kappa ||R^T Y1t - Y2t||_F^2 + tau ||p2 - p1 - t^T Y1t||^2 on
    the lifted poses P1, P2 (ne, d+1, r) (NumPy)."""
    Y1, p1 = P1[:, :d, :], P1[:, d, :]
    Y2, p2 = P2[:, :d, :], P2[:, d, :]
    rot = np.einsum("eab,eak->ebk", R, Y1) - Y2
    tran = p2 - p1 - np.einsum("ea,eak->ek", t, Y1)
    return kappa * (rot ** 2).sum(axis=(1, 2)) + tau * (tran ** 2).sum(axis=1)


def gnc_weight_ref(r_sq, mu: float, barc: float) -> np.ndarray:
    """The project's own GNC-TLS weight function (robust.py), per edge."""
    from dpo_amd.robust import RobustCost
    from dpo_amd.types import RobustCostParams, RobustCostType
    rc = RobustCost(RobustCostType.GNC_TLS, RobustCostParams(gnc_barc=barc))
    rc.mu = mu
    return np.array([rc.weight(math.sqrt(v)) for v in r_sq])


def gnc_tol(mu: float) -> float:
    """sqrt(barc^2 mu (mu + 1) / r^2) - mu cancels at large mu."""
    return 64.0 * EPS * (1.0 + mu)


# ---------------------------------------------------------------------
# tCG control block: layout and a Python model of the control steps
# ---------------------------------------------------------------------
(C_STATUS, C_FX, C_GN0SQ, C_RR, C_ZR, C_EPE, C_EPD, C_DPD, C_COEF, C_BETA,
 C_ITER, C_J, C_RADIUS, C_FPROP, C_DM, C_JSTAR, C_TAUSTAR, C_USE_CURRENT,
 C_STOP_PENDING, C_BOUND, C_GN1SQ, C_RHO, C_HLEN, C_SHRINKS, C_DOT0, C_DOT1,
 C_DOT2, C_DOT3) = range(28)
C_HIST = 32
MAX_TCG = 16
CTRL_SIZE = C_HIST + 5 * MAX_TCG
ST_RUN, ST_TCG_STOP, ST_ACCEPTED, ST_GIVE_UP, ST_NO_UPDATE = range(5)


def H_ZR(j): return C_HIST + j
def H_DHD(j): return C_HIST + MAX_TCG + j
def H_EPE(j): return C_HIST + 2 * MAX_TCG + j
def H_EPD(j): return C_HIST + 3 * MAX_TCG + j
def H_DPD(j): return C_HIST + 4 * MAX_TCG + j


def _steihaug_step(z_r, d_Hd, e_Pe, e_Pd, d_Pd, radius):
    """One Steihaug-Toint decision (solver.truncated_cg): returns
    (hit, coef, e_Pe_new); hit = negative curvature or boundary, coef =
    tau to the boundary, else the CG step length alpha."""
    with np.errstate(all="ignore"):
        alpha = np.float64(z_r) / np.float64(d_Hd) if d_Hd != 0 else math.inf
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
    if d_Hd <= 0 or e_Pe_new >= radius * radius:
        disc = e_Pd * e_Pd + d_Pd * (radius * radius - e_Pe)
        tau = ((-e_Pd + math.sqrt(max(disc, 0.0))) / d_Pd
               if d_Pd > 0 else 0.0)
        return True, tau, e_Pe_new
    return False, float(alpha), float(e_Pe_new)


class CtrlModel:
    """Python model of the scalar tCG / trust-region control steps on a
    CTRL_SIZE fp64 block. Each method is one control kernel: it consumes
    the dot products the vector kernels left in the C_DOT* slots and
    clears them, as the device contract requires."""

    def __init__(self, ctrl=None):
        self.c = (np.zeros(CTRL_SIZE) if ctrl is None
                  else np.array(ctrl, dtype=np.float64))
        assert self.c.shape == (CTRL_SIZE,)

    def init(self, tol, Delta0, theta, kappa):
        c = self.c
        # C_DOT0 = <QX + G, X>, C_DOT2 = <G, X>, C_DOT1 = ||grad||^2
        c[C_FX] = 0.5 * (c[C_DOT0] + c[C_DOT2])
        gn0sq = c[C_DOT1]
        c[C_GN0SQ] = gn0sq
        c[C_RR] = gn0sq
        nr0 = math.sqrt(gn0sq)
        c[C_BOUND] = nr0 * min(nr0 ** theta, kappa)
        c[C_RADIUS] = Delta0
        for s in (C_EPE, C_EPD, C_ITER, C_J, C_USE_CURRENT, C_STOP_PENDING,
                  C_BETA, C_DOT0, C_DOT1, C_DOT2, C_DOT3):
            c[s] = 0.0
        c[C_STATUS] = ST_NO_UPDATE if nr0 < tol else ST_RUN

    def z0(self):
        c = self.c
        if c[C_STATUS] != ST_RUN:
            return
        c[C_ZR] = c[C_DOT0]
        c[C_DPD] = c[C_DOT0]
        c[C_DOT0] = 0.0

    def alpha(self):
        c = self.c
        if c[C_STATUS] != ST_RUN:
            return
        j = int(c[C_ITER])
        d_Hd = c[C_DOT0]
        c[C_DOT0] = 0.0
        c[H_ZR(j)], c[H_DHD(j)] = c[C_ZR], d_Hd
        c[H_EPE(j)], c[H_EPD(j)], c[H_DPD(j)] = c[C_EPE], c[C_EPD], c[C_DPD]
        hit, coef, e_Pe_new = _steihaug_step(
            c[C_ZR], d_Hd, c[C_EPE], c[C_EPD], c[C_DPD], c[C_RADIUS])
        c[C_COEF] = coef
        c[C_STOP_PENDING] = 1.0 if hit else 0.0
        if not hit:
            c[C_EPE] = e_Pe_new

    def rr(self):
        c = self.c
        if c[C_STATUS] != ST_RUN:
            return
        j = int(c[C_ITER])
        if c[C_STOP_PENDING] != 0.0:
            c[C_STATUS] = ST_TCG_STOP
            c[C_J] = j
            c[C_HLEN] = j + 1
            c[C_USE_CURRENT] = 0.0
            return
        rr = c[C_DOT1]
        c[C_DOT1] = 0.0
        c[C_RR] = rr
        if math.sqrt(rr) <= c[C_BOUND]:
            c[C_STATUS] = ST_TCG_STOP
            c[C_J] = j + 1
            c[C_HLEN] = j + 1
            c[C_USE_CURRENT] = 1.0

    def beta(self):
        c = self.c
        if c[C_STATUS] != ST_RUN:
            return
        z_r_new = c[C_DOT0]
        c[C_DOT0] = 0.0
        with np.errstate(all="ignore"):
            beta = z_r_new / c[C_ZR]
        c[C_BETA] = beta
        c[C_EPD] = beta * (c[C_EPD] + c[C_COEF] * c[C_DPD])
        c[C_DPD] = z_r_new + beta * beta * c[C_DPD]
        c[C_ZR] = z_r_new
        c[C_ITER] += 1.0

    def tcg_end(self):
        c = self.c
        if c[C_STATUS] != ST_RUN:
            return
        c[C_STATUS] = ST_TCG_STOP
        c[C_J] = c[C_ITER]
        c[C_HLEN] = c[C_ITER]
        c[C_USE_CURRENT] = 1.0

    def candidate(self):
        """Replay the stored Krylov scalars at the current radius."""
        c = self.c
        if c[C_STATUS] != ST_TCG_STOP:
            return
        dm = 0.0
        jstar = -1
        for j in range(min(int(c[C_HLEN]), MAX_TCG)):
            z_r, d_Hd = c[H_ZR(j)], c[H_DHD(j)]
            hit, coef, _ = _steihaug_step(z_r, d_Hd, c[H_EPE(j)],
                                          c[H_EPD(j)], c[H_DPD(j)],
                                          c[C_RADIUS])
            if hit:
                dm += coef * z_r - 0.5 * coef * coef * d_Hd
                jstar = j
                c[C_JSTAR] = j
                c[C_TAUSTAR] = coef
                break
            dm += 0.5 * coef * z_r
        c[C_USE_CURRENT] = 1.0 if jstar < 0 else 0.0
        c[C_DM] = dm
        c[C_DOT0] = 0.0
        c[C_DOT2] = 0.0

    def accept(self, accept_rho):
        c = self.c
        if c[C_STATUS] != ST_TCG_STOP:
            return
        # C_DOT0 = <Q Xp, Xp>, C_DOT2 = <G, Xp>
        fprop = 0.5 * c[C_DOT0] + c[C_DOT2]
        c[C_DOT0] = 0.0
        c[C_DOT2] = 0.0
        c[C_FPROP] = fprop
        rho = (c[C_FX] - fprop) / max(c[C_DM], 1e-300)
        c[C_RHO] = rho
        if rho > accept_rho and fprop <= c[C_FX]:
            c[C_STATUS] = ST_ACCEPTED

    def shrink(self):
        c = self.c
        if c[C_STATUS] != ST_TCG_STOP:
            return
        c[C_RADIUS] *= 0.25
        c[C_SHRINKS] += 1.0


def model_decrease_from_history(c) -> float:
    """-<g, s> - 0.5 <s, H s> of the step the stored history describes
    at radius c[C_RADIUS], from the CG identities: a full step j lowers
    the model by 0.5 alpha_j <z_j, r_j>, a step tau along delta_j by
    tau <z_j, r_j> - 0.5 tau^2 <delta_j, H delta_j>. tau is re-derived
    as the positive root of ||eta_j + tau delta_j||_P = radius."""
    R2 = c[C_RADIUS] ** 2
    dm = 0.0
    for j in range(min(int(c[C_HLEN]), MAX_TCG)):
        z_r, d_Hd = c[H_ZR(j)], c[H_DHD(j)]
        e_Pe, e_Pd, d_Pd = c[H_EPE(j)], c[H_EPD(j)], c[H_DPD(j)]
        full = None
        if d_Hd > 0:
            a = z_r / d_Hd
            if e_Pe + 2 * a * e_Pd + a * a * d_Pd < R2:
                full = a
        if full is None:
            if d_Pd > 0:
                roots = np.roots([d_Pd, 2 * e_Pd, e_Pe - R2])
                tau = float(max(roots.real)) if R2 >= e_Pe else 0.0
            else:
                tau = 0.0
            return dm + tau * z_r - 0.5 * tau * tau * d_Hd
        dm += 0.5 * full * z_r
    return dm


def ctrl_tol(model: np.ndarray) -> np.ndarray:
    """Per-slot tolerance for comparing a device control block with the
    model: the steps are a handful of fp64 operations that the compiler
    may contract into FMAs, so 64 eps relative to the slot's magnitude
    (floor 1) — not bit equality. Flags, counters and untouched slots
    are integers or copies and compare equal under it as well."""
    return 64.0 * EPS * np.maximum(1.0, np.abs(model))


def model_solve(problem, X0: Tensor, tol: float, Delta0: float,
                max_inner: int, accept_rho: float = 0.1,
                max_shrink: int = 10, theta: float = 1.0,
                kappa: float = 0.1, attempts: Optional[list] = None):
    """One RBCD local solve with the vector work in torch on the CPU and
    every scalar decision taken by CtrlModel, in the order the device
    solve enqueues them. Returns (X, ctrl block, final status). A list
    passed as `attempts` receives one record per candidate: radius,
    use_current, jstar, rho, dm and the candidate point Xp."""
    assert max_inner <= MAX_TCG
    man = problem.manifold
    m = CtrlModel()
    c = m.c
    G = problem._g()
    A = problem.Q.spmm(X0) + G
    grad = man.project_tangent(X0, A)
    c[C_DOT1] = float((grad * grad).sum())
    c[C_DOT0] = float((A * X0).sum())
    c[C_DOT2] = float((G * X0).sum())
    m.init(tol, Delta0, theta, kappa)
    if c[C_STATUS] != ST_RUN:
        return X0, c, int(c[C_STATUS])
    r = grad.clone()
    z = problem.precondition(X0, r)
    c[C_DOT0] = float((z * r).sum())
    m.z0()
    delta = -z
    eta = torch.zeros_like(grad)
    eta_snap, delta_snap = [], []
    for _ in range(max_inner):
        if c[C_STATUS] != ST_RUN:
            break
        Hd = man.project_tangent(X0, problem.hess_vec(delta))
        c[C_DOT0] = float((delta * Hd).sum())
        m.alpha()
        eta_snap.append(eta.clone())
        delta_snap.append(delta.clone())
        eta = eta + c[C_COEF] * delta
        if c[C_STOP_PENDING] == 0.0:
            r = r + c[C_COEF] * Hd
            c[C_DOT1] = float((r * r).sum())
        m.rr()
        if c[C_STATUS] != ST_RUN:
            break
        z = problem.precondition(X0, r)
        c[C_DOT0] = float((z * r).sum())
        m.beta()
        delta = -z + c[C_BETA] * delta
    m.tcg_end()
    for attempt in range(max_shrink + 1):
        if attempt:
            m.shrink()
        m.candidate()
        if c[C_USE_CURRENT] != 0.0:
            step = eta
        else:
            j = int(c[C_JSTAR])
            step = eta_snap[j] + c[C_TAUSTAR] * delta_snap[j]
        Xp = man.retract(X0, step)
        c[C_DOT0] = float((problem.Q.spmm(Xp) * Xp).sum())
        c[C_DOT2] = float((G * Xp).sum())
        m.accept(accept_rho)
        if attempts is not None:
            attempts.append({
                "radius": float(c[C_RADIUS]),
                "use_current": c[C_USE_CURRENT] != 0.0,
                "jstar": int(c[C_JSTAR]), "rho": float(c[C_RHO]),
                "dm": float(c[C_DM]), "Xp": Xp})
        if c[C_STATUS] == ST_ACCEPTED:
            return Xp, c, ST_ACCEPTED
    return X0, c, ST_GIVE_UP


def host_solve(problem, X0: Tensor, tol: float, Delta0: float,
               max_inner: int):
    """The host QuadraticOptimizer's RBCD solve, instrumented: returns
    (X, OptResult, tCG runs, Hessian products of the last run). The last
    count is the tCG iteration count, the device's history length."""
    from dpo_amd.solver import QuadraticOptimizer, TRParams
    from dpo_amd.types import OptAlgorithm
    runs = []
    hess_vec, precondition = problem.hess_vec, problem.precondition
    state = {"fresh": True}

    def counted_hess_vec(V):
        if state["fresh"]:
            runs.append(0)
            state["fresh"] = False
        runs[-1] += 1
        return hess_vec(V)

    def retract(X, eta, _orig=problem.manifold.retract):
        state["fresh"] = True
        return _orig(X, eta)

    problem.hess_vec = counted_hess_vec
    problem.manifold.retract = retract
    try:
        tr = TRParams(tolerance=tol, initial_radius=Delta0, max_iterations=1,
                      max_inner_iterations=max_inner)
        opt = QuadraticOptimizer(problem, OptAlgorithm.RTR, tr)
        X = opt.optimize(X0.clone())
    finally:
        del problem.hess_vec
        del problem.manifold.retract
    return X, opt.result, len(runs), (runs[-1] if runs else 0)


def solve_problem(d: int, r: int, with_g: bool = False):
    """Measurement-built PSD problem with 257 <= n <= 350 poses (two
    blocks of every thread-per-pose kernel), Jacobi preconditioner, and
    a manifold start point. d = 3: grid3d(side=7), n = 343; d = 2:
    city2d(side=18), n = 324."""
    from dpo_amd.quadratic import (QuadraticProblem,
                                   assemble_connection_laplacian)
    from dpo_amd.synthetic import city2d, grid3d
    meas, n = grid3d(side=7, seed=2) if d == 3 else city2d(side=18, seed=2)
    Q = assemble_connection_laplacian(meas, n, d)
    g = gen(7, d, r)
    X = manifold_point(n, d, r, g)
    p = QuadraticProblem(n, d, r, precond="jacobi")
    p.set_q(Q)
    if with_g:
        p.set_g(randn(g, (d + 1) * n, r))
    return p, X


# Device shrink loop: solves on solve_problem(d, r) that reject every
# candidate (accept_rho = 2 is above any rho these problems produce), so
# the whole batched loop runs and the last attempt's scalars reach the
# host. (d, r, Delta0, max_shrink); tol = 1e-2, max_inner = 10.
SHRINK_ACCEPT_RHO = 2.0
SHRINK_CASES = (
    (3, 8, 1e5, 3),     # attempts 0-2 full step, attempt 3 replays jstar = 1
    (3, 5, 640.0, 1), (3, 5, 640.0, 2), (3, 5, 640.0, 3),
    (2, 2, 640.0, 1), (2, 2, 640.0, 2), (2, 2, 640.0, 3),
)


def f_bound(problem, X: Tensor) -> float:
    """Bound on the error of f(X) = 0.5 <QX, X> + <G, X> as the fused
    Hessian kernel's dot slots give it (eval_terms_ref's rule)."""
    return float(eval_terms_ref(problem, X)[1][0])


_shrink_refs = {}


def shrink_case_ref(d: int, r: int, Delta0: float, max_shrink: int):
    """model_solve of one SHRINK_CASES entry, computed once: (problem, X0,
    ctrl block, status, attempts, rho bound). rho = (fX - fprop) / dm: the
    error of fX - fprop is at most the sum of the two f bounds (at X0 and
    at the last candidate), and dm is the model's C_DM."""
    key = (d, r, Delta0, max_shrink)
    if key not in _shrink_refs:
        p, X0 = solve_problem(d, r)
        attempts = []
        _, c, status = model_solve(p, X0, 1e-2, Delta0, 10,
                                   accept_rho=SHRINK_ACCEPT_RHO,
                                   max_shrink=max_shrink, attempts=attempts)
        b_rho = (f_bound(p, X0) + f_bound(p, attempts[-1]["Xp"])) / c[C_DM]
        _shrink_refs[key] = (p, X0, c, status, attempts, b_rho)
    return _shrink_refs[key]


def small_problem(d: int, r: int, n: int, g: torch.Generator,
                  with_g: bool = True):
    """PSD problem on exactly n poses: a measurement-built graph cut to
    its first n poses (the odometry chain keeps it connected)."""
    from dpo_amd.quadratic import (QuadraticProblem,
                                   assemble_connection_laplacian)
    from dpo_amd.synthetic import city2d, grid3d
    if d == 3:
        side = max(2, math.ceil(n ** (1.0 / 3.0) - 1e-9))
        meas, n_all = grid3d(side=side, seed=1)
    else:
        side = max(2, math.ceil(math.sqrt(n) - 1e-9))
        meas, n_all = city2d(side=side, seed=1)
    assert n_all >= n
    meas = [m for m in meas if m.p1 < n and m.p2 < n]
    p = QuadraticProblem(n, d, r, precond="jacobi")
    if meas:
        p.set_q(assemble_connection_laplacian(meas, n, d))
    else:
        # a single pose has no edges: one PSD diagonal block
        assert n == 1
        B = randn(g, d + 1, d + 1)
        p.set_q(BSRMatrix(1, d + 1, torch.tensor([0, 1], dtype=torch.int32),
                          torch.tensor([0], dtype=torch.int32),
                          (B @ B.T)[None].contiguous()))
    if with_g:
        p.set_g(randn(g, (d + 1) * n, r))
    return p, manifold_point(n, d, r, g)


def eval_terms_ref(problem, X: Tensor, bG: Optional[Tensor] = None):
    """[f, 0.5 <X, G>, ||rgrad||^2] in fp64 on the CPU, with a bound for
    each from the sum-of-products rule: the spmm entries carry
    matmul_bound, the projection propagates it, and each scalar adds the
    bound of its own final dot product. bG is an entry-wise bound on the
    error already in the device's G (one assembled by a kernel)."""
    Q, d = problem.Q, problem.d
    G = problem._g()
    Qd = Q.to_dense()
    K = bsr_max_row_terms(Q) + 1
    A = Qd @ X + G
    bA = sop_bound(Qd.abs() @ X.abs() + G.abs(), K)
    if bG is not None:
        bA = bA + bG
    f = 0.5 * float(((Qd @ X) * X).sum()) + float((G * X).sum())
    xg = 0.5 * float((X * G).sum())
    P = cpu_ref.tangent_project(X, A, d)
    bP = tangent_project_bound(X, A, d, bA)
    gn2 = float((P * P).sum())
    T = X.numel()
    b_f = float((bA * X.abs()).sum()) + float(sop_bound(
        (A.abs() * X.abs()).sum() + (G.abs() * X.abs()).sum(), T))
    b_xg = float(sop_bound((G.abs() * X.abs()).sum(), T))
    if bG is not None:     # b_f has it through bA
        b_xg += 0.5 * float((bG * X.abs()).sum())
    b_gn2 = float((2.0 * P.abs() * bP + bP * bP).sum()) + float(
        sop_bound((P * P).sum(), T))
    return (np.array([f, xg, gn2]), np.array([b_f, b_xg, b_gn2]), P, bP)


# ---------------------------------------------------------------------
# packed round loop (tests/test_packed_rounds*.py)
# ---------------------------------------------------------------------
class StubComm:
    """rank `rank` of `world_size` with no process group behind it. The
    driver and PackedBackend constructors only read the two numbers; the
    tests hand the gathered payloads to _scatter themselves, so a
    collective reached by accident is an error, not a hang."""

    def __init__(self, rank: int, world_size: int):
        self.rank, self.world_size = rank, world_size

    def all_gather_flat(self, local, sizes):
        raise AssertionError("collective on a stub communicator")

    all_reduce_sum_ = barrier = all_gather_flat


def interleaved_partition(num_poses: int, num_robots: int, run: int = 3):
    """pose g -> robot (g // run) % num_robots: every robot owns many
    short runs of the trajectory, so local order, public-pose indices and
    neighbour slot order all differ from the contiguous split."""
    return [(g // run) % num_robots for g in range(num_poses)]


def agent_edge_index(p1, p2, part, rb: int):
    """Global measurement indices of agent rb's (odometry, private,
    shared) edges, in the order the agent stores them: input order within
    each class; odometry is a same-robot edge between consecutive global
    poses."""
    part = np.asarray(part)
    p1, p2 = np.asarray(p1), np.asarray(p2)
    r1, r2 = part[p1], part[p2]
    same = r1 == r2
    odo = same & (p1 + 1 == p2)
    return (np.nonzero(odo & (r1 == rb))[0],
            np.nonzero(same & ~odo & (r1 == rb))[0],
            np.nonzero(~same & ((r1 == rb) | (r2 == rb)))[0])


def central_eval_ref(meas, n: int, d: int, Xg: Tensor, weights=None):
    """(<QX, X>, ||rgrad||^2) of the centralized problem at the global
    iterate Xg, fp64 on the CPU, each with the sum-of-products bound of
    this reference's own arithmetic."""
    from dpo_amd.quadratic import assemble_connection_laplacian
    Q = assemble_connection_laplacian(meas, n, d, weights)
    Qd = Q.to_dense()
    K = bsr_max_row_terms(Q) + 1
    A = Qd @ Xg
    bA = sop_bound(Qd.abs() @ Xg.abs(), K)
    T = Xg.numel()
    cost = float((A * Xg).sum())
    b_cost = float((bA * Xg.abs()).sum()) + float(
        sop_bound((A.abs() * Xg.abs()).sum(), T))
    P = cpu_ref.tangent_project(Xg, A, d)
    bP = tangent_project_bound(Xg, A, d, bA)
    gn2 = float((P * P).sum())
    b_gn2 = float((2.0 * P.abs() * bP + bP * bP).sum()) + float(
        sop_bound((P * P).sum(), T))
    return cost, gn2, b_cost, b_gn2


def agent_eval_ref(agent, nbr: Tensor, weights: Tensor):
    """[f, 0.5 <X, G>, ||rgrad||^2] of one agent and their bounds
    (eval_terms_ref), on the agent's own Q assembled on the CPU from
    `weights` (odometry | private | shared) and the G assembled on the
    CPU from the neighbour buffer `nbr` (n_slots, dh, r). G is a
    scatter-add of dh-term products, so it carries its own bound from the
    abs() copies of E0 and nbr."""
    from types import SimpleNamespace
    from dpo_amd.quadratic import GAssembler
    X = agent.X.detach().cpu()
    weights = weights.detach().cpu()
    Q = agent._q_assembler.assemble(weights.clone())
    Q = BSRMatrix(Q.n, Q.dh, Q.row_ptr.clone(), Q.col_idx.clone(),
                  Q.vals.clone())
    ga = agent._g_assembler
    nsh = ga.E0.shape[0]
    wsh = weights[weights.numel() - nsh:]
    if nsh:
        G = ga.assemble(nbr.cpu(), wsh, agent.r)
        gabs = GAssembler.__new__(GAssembler)
        gabs.n, gabs.d = ga.n, ga.d
        gabs.E0, gabs.local_pose, gabs.nbr_slot = \
            ga.E0.abs(), ga.local_pose, ga.nbr_slot
        deg = int(torch.bincount(ga.local_pose).max())
        bG = sop_bound(gabs.assemble(nbr.cpu().abs(), wsh.abs(),
                                     agent.r).abs(), deg * ga.E0.shape[1] + 1)
    else:
        G = torch.zeros_like(X)
        bG = torch.zeros_like(X)
    prob = SimpleNamespace(Q=Q, d=agent.d, _g=lambda: G)
    return eval_terms_ref(prob, X, bG)[:2]


def schedule_probe(drv):
    """Instrument a DistributedRBCDDriver (either backend) and return the
    log its later run() calls fill: per agent the 1-based round numbers,
    counted over the driver's life, of every Nesterov restart and every
    GNC re-weighting, and gamma as each solve phase sees it. The round
    number is counted by wrapping reweight_due(), the first call of every
    round on whichever backend run() picks."""
    log = {"round": 0, "restart": {}, "reweight": {}, "gamma": {}}
    for rb, a in drv.local_agents.items():
        for k in ("restart", "reweight", "gamma"):
            log[k][rb] = []

        def wrap(name, key, a=a, rb=rb):
            inner = getattr(a, name)

            def f(*args, **kw):
                log[key][rb].append(log["round"])
                return inner(*args, **kw)
            setattr(a, name, f)
        wrap("_restart_nesterov", "restart")          # dict path
        wrap("_packed_restart", "restart")            # packed path
        wrap("update_loop_closures_weights", "reweight")
        wrap("_packed_update_weights", "reweight")
    make = drv._backend

    def backend():
        b = make()
        if getattr(b, "_probed", False):
            return b
        b._probed = True
        due, solve = b.reweight_due, b.solve

        def due_(round_counter):
            log["round"] += 1
            return due(round_counter)

        def solve_():
            # the dict path updates gamma inside iterate(): record what
            # _update_x sees; the packed path has it ready before solve()
            if drv.acceleration and hasattr(b, "rank_X"):
                for rb, a in drv.local_agents.items():
                    log["gamma"][rb].append(a.gamma)
            return solve()
        b.reweight_due, b.solve = due_, solve_
        return b
    drv._backend = backend
    if drv.acceleration:
        for rb, a in drv.local_agents.items():
            def ux(do_opt, acceleration, a=a, rb=rb, inner=a._update_x):
                if acceleration:
                    log["gamma"][rb].append(a.gamma)
                return inner(do_opt, acceleration)
            a._update_x = ux
    return log


SCHED_RESTART, SCHED_GNC = 5, 4      # restart_interval, inner iters
SCHED_RUNS = (7, 6)                  # two run() calls, then a restored one


def schedule_model(rounds: int, num_robots: int, accel: bool, robust: bool):
    """The reference's cadence (PGOAgent.cpp iterate(), shouldRestart(),
    shouldUpdateLoopClosureWeights()): round k = 1, 2, ... re-weights at
    its start when (k + 1) % SCHED_GNC == 0, which also resets gamma, and
    restarts at its end when (k + 1) % SCHED_RESTART == 0. Returns
    (restart rounds, re-weighting rounds, gamma seen by each solve)."""
    restart, reweight, gammas = [], [], []
    gamma, K = 0.0, num_robots
    for k in range(1, rounds + 1):
        if robust and (k + 1) % SCHED_GNC == 0:
            reweight.append(k)
            gamma = 0.0
        if accel:
            gamma = (1 + math.sqrt(1 + 4 * K * K * gamma * gamma)) / (2 * K)
            gammas.append(gamma)
            if (k + 1) % SCHED_RESTART == 0:
                restart.append(k)
                gamma = 0.0
    return restart, reweight, gammas


def run_schedule(drv):
    """Two consecutive run() calls and one after restore_initial_state()
    on a probed driver: [(restart, reweight, gamma) per agent] for the
    first two together and for the restored one."""
    for a in drv.local_agents.values():
        a.params.restart_interval = SCHED_RESTART
        a.params.robust_opt_inner_iters = SCHED_GNC
    log = schedule_probe(drv)
    drv.snapshot_initial_state()

    def take():
        out = {rb: (log["restart"][rb][:], log["reweight"][rb][:],
                    log["gamma"][rb][:]) for rb in drv.local_agents}
        for k in ("restart", "reweight", "gamma"):
            for v in log[k].values():
                v.clear()
        log["round"] = 0
        return out
    for n in SCHED_RUNS:
        res = drv.run(max_iters=n, gradnorm_tol=0.0)
        assert res.iterations == n
    first = take()
    drv.restore_initial_state()
    drv.run(max_iters=SCHED_RUNS[1], gradnorm_tol=0.0)
    return first, take()


def check_schedule(got, rounds: int, num_robots: int, accel: bool,
                   robust: bool):
    want = schedule_model(rounds, num_robots, accel, robust)
    assert sorted(got) == list(range(num_robots))
    for rb, lists in got.items():
        assert lists == want, (rb, lists, want)


# GNC fixture: grid3d_soa side 4, 30 % planted outliers, odometry
# dead-reckoning iterate (what the robust drivers start from)
GNC_SIDE, GNC_OUTLIERS, GNC_SEED = 4, 0.3, 5


def gnc_fixture():
    """(MeasurementArray, n, global lifted iterate (r, dh n) at r = 5)."""
    from dpo_amd.manifold import lifting_matrix
    from dpo_amd.measurements import odometry_initialization_array
    from dpo_amd.synthetic import grid3d_soa
    ma, n = grid3d_soa(side=GNC_SIDE, outlier_prob=GNC_OUTLIERS,
                       seed=GNC_SEED)
    T = odometry_initialization_array(3, n, ma.select(ma.p1 + 1 == ma.p2))
    return ma, n, lifting_matrix(3, 5) @ T


def set_global_iterate(drv, Xg: np.ndarray) -> None:
    """set_x every local agent to its poses of the global iterate."""
    dh = drv.dh
    for rb, a in drv.local_agents.items():
        cols = np.concatenate([
            np.arange(dh) + dh * drv.pose_to_index[(rb, i)]
            for i in range(drv.pose_counts[rb])])
        a.set_x(np.ascontiguousarray(Xg[:, cols]))


def gnc_edge_residuals(ma, Xg: np.ndarray, d: int = 3):
    """r^2 of every measurement at the global iterate and the
    sum-of-products bound of that number: each of the dh r residual
    entries is a (d + 1)-term sum, squared and added up."""
    dh = d + 1
    r = Xg.shape[0]
    P = np.ascontiguousarray(Xg.T).reshape(-1, dh, r)
    P1, P2 = P[ma.p1], P[ma.p2]
    r_sq = gnc_residual_sq(P1, P2, ma.R, ma.t, ma.kappa, ma.tau, d)
    A1, A2 = np.abs(P1), np.abs(P2)
    A1[:, d, :] *= -1.0     # p2 - p1 - t^T Y1 -> |p2| + |p1| + |t|^T |Y1|
    A2[:, :d, :] *= -1.0    # R^T Y1 - Y2      -> |R|^T |Y1| + |Y2|
    r_abs = gnc_residual_sq(A1, A2, np.abs(ma.R), -np.abs(ma.t), ma.kappa,
                            ma.tau, d)
    return r_sq, sop_bound(r_abs, 2 * (d + 1) + dh * r)


def gnc_near_threshold(r_sq, bound, mu: float, barc: float) -> np.ndarray:
    """Edges whose r^2 is within its bound of a GNC-TLS threshold."""
    lower = mu / (mu + 1.0) * barc ** 2
    upper = (mu + 1.0) / mu * barc ** 2
    return (np.abs(r_sq - lower) <= bound) | (np.abs(r_sq - upper) <= bound)


def nbr_from_dict(agent) -> Tensor:
    """The neighbour buffer (n_slots, dh, r) the dict path would build."""
    return torch.from_numpy(np.stack(
        [agent.neighbor_pose_dict[pid].T
         for pid in agent._nbr_slot_order]))


# ---------------------------------------------------------------------
# certificate kernel matrix (tests/test_cert_kernel_matrix.py): the six
# Lanczos-path kernels k_cert_lambda, k_cert_apply, k_cert_gram,
# k_cert_sub, k_cert_norm, k_cert_reduce
# ---------------------------------------------------------------------
CERT_M = 8                      # basis size of the dissected step
CERT_STEPS = (0, 1, 5)
CERT_PAD = 64                   # sentinel slots on either side of a buffer
CERT_SENTINEL = -7.25e77
CERT_BETA_PREV = 0.37
# one pose past 256 blocks x 256 threads, at the two largest register tiles
CERT_LAMBDA_WRAP = {(2, 6): 65537, (3, 8): 65537}
# thread-per-row kernels, N = (d + 1) n: 3 / 192 / 195 and 65 538 (two
# rows on a second grid-stride trip) for d = 2; 4 / 256 / 260, 65 536
# (256 full blocks, no second trip) and 65 540 (four rows on one) for d = 3
CERT_ROW_POSES = {2: (1, 64, 65, 21846), 3: (1, 64, 65, 16384, 16385)}


def cert_lambda_poses(d: int, r: int):
    wrap = CERT_LAMBDA_WRAP.get((d, r))
    return N_POSE + ((wrap,) if wrap else ())


def cert_steps_for(N: int):
    """Step j needs j + 1 orthonormal basis rows and a direction left for
    v_{j+1}: j + 2 <= N (N = 3 and 4 cannot hold step 5)."""
    return tuple(j for j in CERT_STEPS if j + 2 <= N)


@functools.lru_cache(maxsize=None)
def cert_matrix(n: int, d: int):
    """(Q, |Q|) of random_bsr(n, d + 1), built once per (n, d) with the
    scalar-CSR mirrors the CPU reference multiplies with."""
    Q = random_bsr(n, d + 1, gen(40, n, d))
    Qa = BSRMatrix(Q.n, Q.dh, Q.row_ptr, Q.col_idx, Q.vals.abs())
    Q.to_scalar_csr()
    Qa.to_scalar_csr()
    return Q, Qa


def cert_zero_matrix(n: int, d: int):
    """The pattern of cert_matrix(n, d) with every stored value zero."""
    Q, _ = cert_matrix(n, d)
    return BSRMatrix(Q.n, Q.dh, Q.row_ptr, Q.col_idx,
                     torch.zeros_like(Q.vals))


def cert_lam_blocks(n: int, d: int, g: torch.Generator) -> Tensor:
    """Random symmetric (n, d, d) blocks, independent of Q."""
    A = randn(g, n, d, d)
    return (0.5 * (A + A.transpose(1, 2))).contiguous()


def cert_basis(N: int, j: int, m: int, g: torch.Generator) -> Tensor:
    """(m + 1, N) basis: rows 0..j are the Q factor of a random
    N x (j + 1) matrix, every later row is CERT_SENTINEL."""
    assert j + 1 <= N
    V = torch.full((m + 1, N), CERT_SENTINEL, dtype=torch.float64)
    V[:j + 1] = torch.linalg.qr(randn(g, N, j + 1))[0].T
    return V


def cert_ctl(m: int, j: int, tol: float = 0.0,
             beta_prev: float = CERT_BETA_PREV) -> Tensor:
    """Control array with a distinct finite marker in every slot but the
    flag (0), the threshold and beta_{j-1}."""
    ctl = 100.0 + 0.375 * torch.arange(cpu_ref.CERT_HDR + 2 * m,
                                       dtype=torch.float64)
    ctl[cpu_ref.CERT_FLAG] = 0.0
    ctl[cpu_ref.CERT_TOL] = tol
    if j > 0:
        ctl[cpu_ref.CERT_HDR + m + j - 1] = beta_prev
    return ctl


def cert_step_state(n: int, d: int, j: int, m: int = CERT_M,
                    tol: float = 0.0, beta_prev: float = CERT_BETA_PREV):
    """(Q, |Q|, lam, V, ctl) of one Lanczos step j at (n, d)."""
    g = gen(43, n, d, j)
    Q, Qa = cert_matrix(n, d)
    lam = cert_lam_blocks(n, d, g)
    V = cert_basis(n * (d + 1), j, m, g)
    return Q, Qa, lam, V, cert_ctl(m, j, tol, beta_prev)


# ---- k_cert_lambda ---------------------------------------------------
def cert_lambda_ref(X: Tensor, QX: Tensor, d: int):
    """Lambda_i = sym(QX_i Y_i^T) and res = ||QX - Lambda X||_F^2 from X and
    a given QX (the arithmetic of cpu_ref.cert_lambda without its sparse
    product), with their bounds.

    lam: each entry is half a sum of 2 r products plus the halving:
    sop_bound(sym(|QX||Y|^T), 2 r + 1). g = QX - Lambda Y on the rotation
    rows: the lam error enters through |Y|, and the d products subtracted
    from QX add sop_bound(|QX| + |Lambda||Y|, d + 1); translation rows are
    copies. res = sum g^2 over T = n (d + 1) r non-negative terms:
    sum (2 |g| b_g + b_g^2) + sop_bound(sum g^2, T).
    Returns (lam, res, b_lam, b_res)."""
    r = X.shape[1]
    Xb, Gb = _pose(X, d), _pose(QX, d)
    Y, G = Xb[:, :d, :], Gb[:, :d, :]
    A = torch.bmm(G, Y.transpose(1, 2))
    lam = 0.5 * (A + A.transpose(1, 2))
    Aa = torch.bmm(G.abs(), Y.abs().transpose(1, 2))
    b_lam = sop_bound(0.5 * (Aa + Aa.transpose(1, 2)), 2 * r + 1)
    g = Gb.clone()
    g[:, :d, :] -= torch.bmm(lam, Y)
    b_g = torch.zeros_like(g)
    b_g[:, :d, :] = torch.bmm(b_lam, Y.abs()) + sop_bound(
        G.abs() + torch.bmm(lam.abs(), Y.abs()), d + 1)
    res = float((g * g).sum())
    b_res = float((2.0 * g.abs() * b_g + b_g * b_g).sum()) + float(
        sop_bound(res, g.numel()))
    return lam.contiguous(), res, b_lam, b_res


def _pose(X: Tensor, d: int) -> Tensor:
    return X.view(-1, d + 1, X.shape[1])


# ---- k_cert_apply ----------------------------------------------------
def cert_apply_terms(Q: BSRMatrix, d: int) -> int:
    """Most products accumulated into one entry of w: the longest BSR
    row, the d Lambda products and the beta term."""
    return bsr_max_row_terms(Q) + d + 1


def cert_apply_ref(Q: BSRMatrix, Qa: BSRMatrix, lam: Tensor, v: Tensor,
                   vprev: Optional[Tensor] = None, beta: float = 0.0):
    """w = (Q - Lambda) v - beta vprev and alpha = <v, w> by
    cpu_ref.cert_apply, with bounds from the same function on abs()
    copies: b_w = 2 K eps (|Q||v| + |Lambda||v| + |beta||vprev|) entry-wise,
    b_alpha = dot_bound(v, w) + sum |v| b_w. Returns (w, alpha, b_w,
    b_alpha)."""
    d = lam.shape[1]
    w, alpha = cpu_ref.cert_apply(Q, lam, v, vprev, beta)
    w_abs, _ = cpu_ref.cert_apply(
        Qa, -lam.abs(), v.abs(), None if vprev is None else vprev.abs(),
        -abs(beta))
    b_w = sop_bound(w_abs, cert_apply_terms(Q, d))
    b_alpha = dot_bound(v, w) + float((v.abs() * b_w).sum())
    return w, float(alpha), b_w, b_alpha


# ---- one Lanczos step ------------------------------------------------
def cert_step_ref(Q: BSRMatrix, Qa: BSRMatrix, lam: Tensor, V: Tensor,
                  ctl: Tensor, j: int) -> SimpleNamespace:
    """Step j of cpu_ref.cert_lanczos_steps, operation for operation, with
    the intermediates the device leaves in w, cvec and part and a bound
    for each (tests/test_kernel_refs.py shows that these and cpu_ref's own
    alpha, beta and v_{j+1} lie within half the bound of a longdouble run
    of the step).

    Derivation, every bound entry-wise and valid for any summation order:
      apply   b_w = 2 K eps (|Q||v_j| + |Lambda||v_j| + |beta||v_{j-1}|),
              K = cert_apply_terms; b_alpha = dot_bound + sum |v_j| b_w.
      CGS pass (twice), B = V[0..j]:
        c = B w is j + 1 sums of N products of an inexact w:
              b_c = 2 N eps |B||w| + |B| b_w
        w' = w - B^T c adds j + 1 products to w, per row:
              b_w' = b_w + |B|^T b_c + 2 (j + 2) eps (|w| + |B|^T |c|)
        The second pass's c is about eps ||w||: it is compared under the
        absolute b_c, never relatively.
      beta^2 = sum w^2 (what the part slots add up to), N terms:
              b_beta2 = sum (2 |w| b_w + b_w^2) + 2 N eps sum w^2
      beta:   | ||w + e|| - ||w|| | <= ||e||_2, and the two norm
              evaluations round by at most N eps beta between them:
              b_beta = ||b_w||_2 + N eps beta
      v_{j+1} = w / beta: |dv| <= (b_w + |w| b_beta / beta) / beta. The
              roundings of the division (1.5 eps |v| between w / beta and
              w * (1 / beta)) sit inside the head room of b_w, which is
              at least (j + 2) eps |w|.
    """
    m = V.shape[0] - 1
    N = V.shape[1]
    d = lam.shape[1]
    hdr = cpu_ref.CERT_HDR
    vj = V[j]
    w = cpu_ref._cert_s_apply(Q.to_scalar_csr(), lam, vj)
    w_abs = cpu_ref._cert_s_apply(Qa.to_scalar_csr(), -lam.abs(), vj.abs())
    if j > 0:
        w -= ctl[hdr + m + j - 1] * V[j - 1]
        w_abs += ctl[hdr + m + j - 1].abs() * V[j - 1].abs()
    out = SimpleNamespace(j=j, N=N)
    b_w = sop_bound(w_abs, cert_apply_terms(Q, d))
    out.w0, out.b_w0 = w.clone(), b_w
    out.alpha = float(torch.dot(vj, w))
    out.b_alpha = dot_bound(vj, w) + float((vj.abs() * b_w).sum())
    B = V[:j + 1]
    Ba = B.abs()
    for p in (1, 2):
        c = B @ w
        b_c = sop_bound(Ba @ w.abs(), N) + Ba @ b_w
        b_w = b_w + Ba.T @ b_c + sop_bound(w.abs() + Ba.T @ c.abs(), j + 2)
        w = w - B.T @ c
        setattr(out, f"c{p}", c)
        setattr(out, f"b_c{p}", b_c)
        setattr(out, f"w{p}", w.clone())
        setattr(out, f"b_w{p}", b_w)
    out.beta = float(torch.linalg.norm(w))
    out.beta2 = float((w * w).sum())
    out.b_beta2 = float((2.0 * w.abs() * b_w + b_w * b_w).sum()) + float(
        sop_bound(out.beta2, N))
    out.b_beta = float(torch.linalg.norm(b_w)) + N * EPS * out.beta
    if out.beta > 0.0:
        out.vnext = w / out.beta
        out.b_v = (b_w + w.abs() * (out.b_beta / out.beta)) / out.beta
    return out


# ---- fixed-order fan-in -----------------------------------
def cert_fixed_order_sum(part, wave_order=(0, 1, 2, 3)) -> float:
    """cert_sum_partials in NumPy fp64, in the device's order: slot t of
    <= 256 goes to thread t (the rest add 0.0), each 64-lane wave runs
    the xor-shuffle tree v += v[lane ^ off] for off = 32, 16, 8, 4, 2, 1,
    then the four wave sums are added in sequence, wave 0 first.
    wave_order exists so that the CPU check can show that another order
    gives another result."""
    p = np.zeros(256, dtype=np.float64)
    part = np.asarray(part, dtype=np.float64)
    assert part.ndim == 1 and part.size <= 256
    p[:part.size] = part
    lanes = np.arange(64)
    sh = []
    for wv in range(4):
        v = p[64 * wv:64 * wv + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ off]
        assert (v == v[0]).all() or np.isnan(v).any()
        sh.append(v[0])
    s = sh[wave_order[0]]
    for wv in wave_order[1:]:
        s = s + sh[wv]
    return float(s)


def cert_fanin_cases():
    """{label: 256 partials} with 1e16, 1, -1e16 in slots 0, 1 and 255.
    "sparse": zeros elsewhere; there 1e16 + 1 rounds to 1e16 in every
    order, so it pins the result (0.0, not the exact 1.0) but not the
    order. "dense": the other slots hold Gaussians scaled over
    1e-3..1e17. The two 1e16 have the same ulp, and rounding is
    symmetric, so only values with other ulps make the wave order, a
    plain left-to-right sum and the exact sum all differ from the device
    order (tests/test_kernel_refs.py asserts that they do)."""
    g = gen(44)
    sparse = np.zeros(256)
    dense = (randn(g, 256) * 10.0 ** (20.0 * torch.rand(
        256, dtype=torch.float64, generator=g) - 3.0)).numpy()
    for p in (sparse, dense):
        p[0], p[1], p[255] = 1e16, 1.0, -1e16
    return {"sparse": sparse, "dense": dense}
