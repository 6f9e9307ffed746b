"""A-posteriori global-optimality certificate for the rank-relaxed
pose-graph problem.

For a lifted iterate Xt (N, r) of f(X) = 0.5 <Q, X^T X> let QX = Q @ Xt
and let Lambda be block-diagonal with one (d+1) x (d+1) block per pose:
top-left d x d block sym(QX_i X_i^T), zero translation row and column.
With S = Q - Lambda, S @ Xt is the Riemannian gradient, and Xt is a
global minimiser of the relaxation iff it is critical and S is positive
semidefinite. `certify_solution` estimates lambda_min(S) with Lanczos
(full reorthogonalisation, basis resident on Xt's device);
`escape_direction` turns a negative-curvature Ritz vector into the one
saddle-escape step at rank r + 1.

Limitations: CERTIFIED rests on the Lanczos residual bound
|beta_m u_m| for the smallest Ritz pair, not on a factorisation-based
interval proof; and graphs with a tiny spectral gap can need more steps
than `max_iters` and then return INCONCLUSIVE. With `basis_size` the
basis is a fixed window (thick-restart Lanczos), so `max_iters` is a time
budget and no longer a memory one. `method="lobpcg"` runs a
preconditioned block eigensolver for the small end under the same
decision rule (docs/DESIGN.md §20).
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .ops.cpu_ref import (CERT_COUNT, CERT_FLAG, CERT_HDR, CERT_KEEP_MAX,
                          CERT_SHAPES, CERT_TOL, cert_check_shape)
from .quadratic import (BSRMatrix, QuadraticProblem,
                        assemble_connection_laplacian)

Tensor = torch.Tensor

# beta_j below BREAKDOWN_TOL * ||S||_inf ends the recurrence: the Krylov
# space is exhausted and the Ritz values are exact to that accuracy.
BREAKDOWN_TOL = 1e-10
# the largest Ritz pair counts as converged (lambda_max known to this
# relative accuracy) once its residual bound is below this
LMAX_RTOL = 1e-7


class CertificateStatus(Enum):
    CERTIFIED = "certified"
    NOT_OPTIMAL = "not_optimal"
    NOT_CRITICAL = "not_critical"
    INCONCLUSIVE = "inconclusive"


@dataclass
class CertificateResult:
    status: CertificateStatus
    lambda_min: float      # smallest Ritz value of S (nan if not run)
    residual: float        # Lanczos residual bound of that Ritz pair
    lambda_max: float      # largest Ritz value (the problem's scale)
    grad_norm: float       # ||S @ Xt||_F
    iterations: int        # Lanczos steps taken
    direction: Optional[Tensor]  # (N,) unit Ritz vector of lambda_min
    restarts: int = 0      # thick restarts taken (basis_size path)
    restarted: bool = False  # basis_size was given
    # method="lobpcg": `iterations` counts LOBPCG iterations and
    # `residual` is the true ||S x - theta x|| of the returned direction
    method: str = "lanczos"
    block_size: int = 0          # LOBPCG block size m
    precond: Optional[str] = None  # preconditioner LOBPCG ran with
    applications: int = 0        # columns S was applied to (LOBPCG runs:
    #                              lambda_max phase included)
    basis_drops: int = 0         # Rayleigh-Ritz solves on a reduced basis

    def as_dict(self) -> dict:
        """JSON-safe summary (no direction; values not computed are None).
        `certificate_restarts` appears only for a basis_size run, the
        `certificate_method`, `_block`, `_precond`, `_applications` and
        `_basis_drops` keys only for a LOBPCG run."""
        def num(x):
            return None if x != x else x
        out = {"certificate": self.status.value,
               "lambda_min": num(self.lambda_min),
               "lambda_max": num(self.lambda_max),
               "certificate_residual": num(self.residual),
               "certificate_grad_norm": self.grad_norm,
               "certificate_iterations": self.iterations}
        if self.restarted:
            out["certificate_restarts"] = self.restarts
        if self.method == "lobpcg":
            out["certificate_method"] = self.method
            out["certificate_block"] = self.block_size
            out["certificate_precond"] = self.precond
            out["certificate_applications"] = self.applications
            out["certificate_basis_drops"] = self.basis_drops
        return out


class BasisBudgetError(MemoryError):
    """The Lanczos basis would exceed `basis_budget_bytes`."""


def _d_of(Q: BSRMatrix) -> int:
    return Q.dh - 1


def certificate_operator(Q: BSRMatrix, Xt: Tensor) -> Tuple[Tensor, float]:
    """Lambda blocks (n, d, d) of S = Q - Lambda(Xt) and the gradient norm
    ||S @ Xt||_F. Q and Xt live on the same device; GPU tensors run the
    HIP kernels (one host read, of the norm)."""
    d = _d_of(Q)
    assert Xt.dtype == torch.float64 and Xt.shape[0] == Q.N
    be = ops.backend_for(Xt)
    lam, res = be.cert_lambda(Q, Xt.contiguous(), d)
    return lam, float(torch.sqrt(res)[0])


def _inf_norm_bound(Q: BSRMatrix, lam: Tensor) -> float:
    """||S||_inf >= every |eigenvalue| of S, from the BSR values."""
    n, dh = Q.n, Q.dh
    d = dh - 1
    rows = torch.repeat_interleave(
        torch.arange(n, device=Q.vals.device),
        (Q.row_ptr[1:] - Q.row_ptr[:-1]).long())
    rs = torch.zeros(n, dh, dtype=torch.float64, device=Q.vals.device)
    rs.index_add_(0, rows, Q.vals.abs().sum(dim=2))
    rs[:, :d] += lam.abs().sum(dim=2)
    return float(rs.max())


def _ritz(alpha: np.ndarray, beta: np.ndarray):
    """Extreme Ritz pairs of the k x k Lanczos tridiagonal: (theta_min,
    u_min, resid_min, theta_max, resid_max); beta[k-1] couples to the
    next (unseen) basis vector."""
    k = len(alpha)
    T = np.diag(alpha)
    if k > 1:
        off = beta[:k - 1]
        T += np.diag(off, 1) + np.diag(off, -1)
    evals, evecs = np.linalg.eigh(T)
    bk = abs(beta[k - 1])
    return (float(evals[0]), evecs[:, 0], float(bk * abs(evecs[-1, 0])),
            float(evals[-1]), float(bk * abs(evecs[-1, -1])))


def _ritz_dense(T: np.ndarray, beta_last: float):
    """`_ritz` for the dense projected matrix T (k x k) of a thick-restart
    window; beta_last couples its last basis vector to the next one."""
    evals, evecs = np.linalg.eigh(T)
    bk = abs(beta_last)
    return (float(evals[0]), evecs[:, 0], float(bk * abs(evecs[-1, 0])),
            float(evals[-1]), float(bk * abs(evecs[-1, -1])))


def default_keep(basis_size: int) -> Tuple[int, int]:
    """Ritz pairs kept at a restart of a window of b vectors: the two
    largest (one for b < 6) and the b // 2 - k_hi smallest, at least one
    and at most what the contraction kernel's CERT_KEEP_MAX columns
    leave. Half the window is the usual thick-restart compromise between
    progress per restart and steps between restarts."""
    k_hi = 2 if basis_size >= 6 else 1
    k_lo = min(max(1, basis_size // 2 - k_hi), CERT_KEEP_MAX - k_hi)
    return k_lo, k_hi


def _check_keep(basis_size: int,
                keep: Optional[Tuple[int, int]]) -> Tuple[int, int]:
    if basis_size < 4:
        raise ValueError(f"basis_size={basis_size}: a restart window needs "
                         "at least 4 vectors")
    k_lo, k_hi = default_keep(basis_size) if keep is None else keep
    if (k_lo < 1 or k_hi < 1 or k_lo + k_hi + 2 > basis_size
            or k_lo + k_hi > CERT_KEEP_MAX):
        raise ValueError(
            f"keep=({k_lo}, {k_hi}) with basis_size={basis_size}: need "
            "k_lo >= 1, k_hi >= 1, k_lo + k_hi + 2 <= basis_size and "
            f"k_lo + k_hi <= {CERT_KEEP_MAX}")
    return int(k_lo), int(k_hi)


def _thick_restart(T: np.ndarray, beta_last: float,
                   keep: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray]:
    """Restart of a full window with projected matrix T (b x b): the
    (b, k) coefficients C of the kept Ritz vectors (k_lo smallest, k_hi
    largest) and the new projected matrix, diag(theta_1..theta_k) with
    the arrowhead s_i = beta_last * Y[b - 1, i] in row and column k and
    zero (to be filled by the next steps) below."""
    b = T.shape[0]
    k_lo, k_hi = keep
    evals, Y = np.linalg.eigh(T)
    idx = list(range(k_lo)) + list(range(b - k_hi, b))
    k = len(idx)
    Tn = np.zeros_like(T)
    Tn[np.arange(k), np.arange(k)] = evals[idx]
    Tn[:k, k] = Tn[k, :k] = beta_last * Y[b - 1, idx]
    return np.ascontiguousarray(Y[:, idx]), Tn


def certify_solution(measurements, n: int, d: int, Xt: Tensor, *,
                     weights: Optional[Sequence[float]] = None,
                     eta: Optional[float] = None,
                     grad_tol: Optional[float] = None,
                     max_iters: int = 512, check_every: int = 16,
                     seed: int = 0,
                     basis_budget_bytes: int = 2 << 30,
                     basis_size: Optional[int] = None,
                     keep: Optional[Tuple[int, int]] = None,
                     method: str = "lanczos",
                     block_size: Optional[int] = None,
                     precond="auto", problem=None, lmax_iters: int = 64,
                     start_block: Optional[Tensor] = None
                     ) -> CertificateResult:
    """Certify that the lifted iterate Xt (N, r), N = n (d+1), is a global
    minimiser of the rank-relaxed problem of `measurements`.

    Q is assembled with `weights` (per-edge, e.g. final GNC weights;
    default: the measurements' stored weights) on Xt's device. Lanczos
    runs from a seeded random start in batches of `check_every` steps,
    with one device-to-host read of the alpha/beta arrays per batch, and
    keeps all basis vectors for full reorthogonalisation.

    eta       curvature tolerance: S counts as PSD when lambda_min >=
              -eta. Default 1e-6 * lambda_max(S).
    grad_tol  criticality tolerance on ||S Xt||_F. Default
              1e-4 * sqrt(lambda_max(S)); lambda_max is not known before
              Lanczos runs, so the default uses the bound ||S||_inf >=
              lambda_max in its place.
    basis_budget_bytes
              the basis costs N * (m + 1) doubles, m = min(max_iters, N);
              BasisBudgetError is raised before anything is allocated
              when that exceeds the budget.
    basis_size
              None: the path above. b >= 4: thick-restart Lanczos in a
              window of b vectors. The basis costs N * (b + 1) doubles
              whatever max_iters is; max_iters counts operator
              applications across restarts and may exceed b and N. Full
              reorthogonalisation stays, inside the window. When the
              window is full it is contracted to the kept Ritz vectors
              plus the residual vector and the recurrence carries on.
    keep      (k_lo, k_hi): the k_lo smallest and k_hi largest Ritz pairs
              survive a restart; the large end is kept because CERTIFIED
              waits for lambda_max to converge. Default `default_keep(b)`.
              ValueError unless k_lo, k_hi >= 1, k_lo + k_hi + 2 <= b and
              k_lo + k_hi <= 16 (the contraction kernel's column bound).

    Decision, in this order: NOT_CRITICAL when the gradient norm exceeds
    grad_tol (Lanczos is skipped); NOT_OPTIMAL as soon as the smallest
    Ritz value theta < -eta (a Rayleigh quotient, hence a rigorous
    witness; `direction` is its Ritz vector); CERTIFIED when the residual
    bound of theta is <= eta and theta >= -eta, or on breakdown (Krylov
    space exhausted, Ritz values exact); INCONCLUSIVE at max_iters.
    Until the largest Ritz pair has converged the default eta is taken
    from ||S||_inf, so a NOT_OPTIMAL verdict never rests on an
    underestimated scale, and CERTIFIED waits for that convergence.

    method    "lanczos" (default): everything above. "lobpcg": the same
              gate, scale and decision rule, with a preconditioned block
              eigensolver for the small end (docs/DESIGN.md §20): an
              unrestarted Lanczos phase of at most `lmax_iters` steps
              fixes lambda_max (and returns at once on a NOT_OPTIMAL
              witness or a breakdown), then LOBPCG runs from a seeded
              random (N, m) block that is deliberately not seeded with
              Xt. `max_iters` then counts LOBPCG iterations, the result's
              `residual` is the true ||S x - theta x|| of `direction`,
              and `basis_size` / `keep` are refused.
    block_size
              m, in the compiled shape table of d with 3 m <= N. Default
              min(r + 1, largest compiled): one vector more than the
              zero cluster of S at a solved rank-r iterate.
    precond   "auto" | "dense" | "jacobi" | "exact", as in
              `QuadraticProblem` (of Q + 0.1 I). Under "auto" a failed
              dense build falls back to block-Jacobi with a warning.
    problem   a `QuadraticProblem` whose `set_q` ran on this Q, or a
              `(mode, data)` pair of `refine.build_preconditioner`: used
              instead of building a preconditioner.
    start_block
              (N, m) start block in place of the seeded random one, for
              diagnostics; never pass Xt (see above).
    Memory: the lambda_max basis plus seven (N, m) blocks, checked against
    `basis_budget_bytes` before anything is allocated.
    """
    assert Xt.dim() == 2 and Xt.shape[0] == n * (d + 1)
    N, r = Xt.shape
    cert_check_shape(d, r)
    if method not in ("lanczos", "lobpcg"):
        raise ValueError(f"unknown method {method!r}: 'lanczos' or 'lobpcg'")
    if method == "lobpcg":
        return _certify_lobpcg(
            measurements, n, d, Xt, weights=weights, eta=eta,
            grad_tol=grad_tol, max_iters=max_iters, check_every=check_every,
            seed=seed, basis_budget_bytes=basis_budget_bytes,
            basis_size=basis_size, keep=keep, block_size=block_size,
            precond=precond, problem=problem, lmax_iters=lmax_iters,
            start_block=start_block)
    if block_size is not None or problem is not None \
            or start_block is not None:
        raise ValueError("block_size, problem and start_block are only "
                         "meaningful with method='lobpcg'")
    if basis_size is None:
        if keep is not None:
            raise ValueError("keep is only meaningful with basis_size")
        m = int(min(max_iters, N))
    else:
        m = int(basis_size)
        keep = _check_keep(m, keep)
    need = 8 * N * (m + 1)
    if need > basis_budget_bytes:
        raise BasisBudgetError(
            f"Lanczos basis needs {need} bytes (N={N}, {m + 1} vectors) "
            f"but basis_budget_bytes={basis_budget_bytes}; raise the "
            "budget or " + ("lower max_iters or pass basis_size"
                            if basis_size is None else "lower basis_size"))
    dev = Xt.device
    Xt = Xt.to(torch.float64).contiguous()
    if isinstance(weights, Tensor):
        weights = weights.detach().cpu().tolist()
    Q = assemble_connection_laplacian(measurements, n, d, weights)
    if dev.type != "cpu":
        Q = Q.to(dev)
    lam, grad_norm = certificate_operator(Q, Xt)
    bound = _inf_norm_bound(Q, lam)
    nan = float("nan")
    if grad_tol is None:
        grad_tol = 1e-4 * float(np.sqrt(bound))
    if not grad_norm <= grad_tol:
        return CertificateResult(CertificateStatus.NOT_CRITICAL, nan, nan,
                                 nan, grad_norm, 0, None, 0,
                                 basis_size is not None)

    be = ops.backend_for(Xt)
    g = torch.Generator().manual_seed(seed)
    v0 = torch.randn(N, dtype=torch.float64, generator=g)
    v0 /= torch.linalg.norm(v0)
    V = torch.zeros(m + 1, N, dtype=torch.float64, device=dev)
    V[0] = v0.to(dev)
    ctl_host = torch.zeros(CERT_HDR + 2 * m, dtype=torch.float64)
    ctl_host[CERT_TOL] = BREAKDOWN_TOL * bound
    ctl = ctl_host.to(dev)

    def finish(status, k, theta, u, resid, lmax, steps=None, restarts=0):
        y = (torch.from_numpy(u.copy()).to(dev) @ V[:k])
        y /= torch.linalg.norm(y)
        return CertificateResult(status, theta, resid, lmax, grad_norm,
                                 k if steps is None else steps, y,
                                 restarts, basis_size is not None)

    def decide(theta, resid, lmax, resid_max, exact):
        lmax_ok = exact or resid_max <= LMAX_RTOL * abs(lmax)
        eta_now = eta if eta is not None else 1e-6 * (
            lmax if lmax_ok else bound)
        if theta < -eta_now:
            return CertificateStatus.NOT_OPTIMAL
        if exact or (lmax_ok and resid <= eta_now):
            return CertificateStatus.CERTIFIED
        return CertificateStatus.INCONCLUSIVE

    if basis_size is not None:
        # Thick restart: a window of m = basis_size vectors whose first
        # `pos` columns are filled; T is its dense projected matrix.
        T = np.zeros((m, m))
        pos = total = restarts = 0
        while True:
            nsteps = min(check_every, m - pos, max_iters - total)
            be.cert_lanczos_window(Q, lam, V, ctl, pos, nsteps)
            h = ctl.cpu().numpy()  # the one device-to-host read per batch
            k = int(h[CERT_COUNT])
            broke = h[CERT_FLAG] != 0.0
            alpha, beta = h[CERT_HDR:CERT_HDR + m], h[CERT_HDR + m:]
            for j in range(pos, k):
                T[j, j] = alpha[j]
                if j + 1 < m:
                    T[j, j + 1] = T[j + 1, j] = beta[j]
            total += k - pos
            pos = k
            theta, u, resid, lmax, resid_max = _ritz_dense(
                T[:k, :k], beta[k - 1])
            status = decide(theta, resid, lmax, resid_max, bool(broke))
            if (status != CertificateStatus.INCONCLUSIVE or broke
                    or total >= max_iters):
                return finish(status, k, theta, u, resid, lmax, total,
                              restarts)
            if k == m:
                C, T = _thick_restart(T, beta[m - 1], keep)
                be.cert_contract(V, torch.from_numpy(C))
                restarts += 1
                pos = C.shape[1]
                # the step count, and the beta slot the next k_cert_apply
                # reads: CGS2 removes the arrowhead component by itself
                h = h.copy()
                h[CERT_COUNT] = pos
                h[CERT_HDR + m + pos - 1] = 0.0
                ctl.copy_(torch.from_numpy(h))

    done = 0
    while True:
        nsteps = min(check_every, m - done)
        be.cert_lanczos_steps(Q, lam, V, ctl, done, nsteps)
        h = ctl.cpu().numpy()      # the one device-to-host read per batch
        k = int(h[CERT_COUNT])
        broke = h[CERT_FLAG] != 0.0
        done += nsteps
        theta, u, resid, lmax, resid_max = _ritz(
            h[CERT_HDR:CERT_HDR + k], h[CERT_HDR + m:CERT_HDR + m + k])
        # broke: beta_k = 0, the Ritz values are exact
        status = decide(theta, resid, lmax, resid_max, bool(broke))
        if status != CertificateStatus.INCONCLUSIVE or broke or done >= m:
            return finish(status, k, theta, u, resid, lmax)


# LOBPCG (docs/DESIGN.md §20). A Gram matrix scaled to unit diagonal
# whose smallest eigenvalue is below LOB_SINGULAR_TOL counts as
# numerically singular: the Cholesky-based reduction of the pencil loses
# about eps / lambda_min(G_B) in the Ritz values, 2e-6 relative at this
# threshold, which is the size of the default eta. The verdict never
# rests on those values (it is re-evaluated on a fresh S x), so the
# threshold trades iterations, not correctness.
LOB_SINGULAR_TOL = 1e-10


def default_block_size(d: int, r: int, N: int) -> int:
    """min(r + 1, largest compiled block size), lowered to the largest
    compiled m with 3 m <= N on a tiny graph."""
    m = min(r + 1, max(CERT_SHAPES[d]))
    while 3 * m > N and m - 1 in CERT_SHAPES[d]:
        m -= 1
    return m


def _lob_rayleigh_ritz(GB: np.ndarray, GA: np.ndarray, m: int, idx):
    """Rayleigh-Ritz on the columns `idx` of B = [X W P] from the Gram
    matrices G_B = B^T B and G_A = B^T S B (3m x 3m): theta (m, ascending)
    and the (3m, 2m) coefficients of the new X (columns [0, m)) and of the
    new P (columns [m, 2m): the same combination without its X part).
    None when G_B, scaled to unit diagonal, is not numerically positive
    definite or the factorisation fails."""
    import scipy.linalg as sla
    idx = np.asarray(idx, dtype=np.int64)
    gb = GB[np.ix_(idx, idx)]
    ga = GA[np.ix_(idx, idx)]
    dg = np.diag(gb)
    if not (np.isfinite(gb).all() and np.isfinite(ga).all()
            and (dg > 0.0).all()):
        return None
    s = 1.0 / np.sqrt(dg)
    gbs = gb * s[:, None] * s[None, :]
    gas = ga * s[:, None] * s[None, :]
    try:
        if np.linalg.eigvalsh(gbs)[0] < LOB_SINGULAR_TOL:
            return None
        w, Y = sla.eigh(gas, gbs)
    except (np.linalg.LinAlgError, sla.LinAlgError, ValueError):
        return None
    if not (np.isfinite(w).all() and np.isfinite(Y).all()):
        return None
    c = s[:, None] * Y[:, :m]
    C = np.zeros((3 * m, 2 * m))
    C[idx, :m] = c
    tail = idx >= m
    C[idx[tail], m:] = c[tail]
    return w[:m].copy(), C


def _lob_preconditioner(Q: BSRMatrix, n: int, d: int, r: int, precond,
                        problem):
    if problem is not None:
        if isinstance(problem, tuple):
            return problem
        assert problem.Q is not None and problem.N == Q.N, \
            "problem= needs a QuadraticProblem after set_q on the same Q"
        mode = problem._active_precond
        data = {"jacobi": problem._Lpre, "dense": problem._Minv,
                "exact": problem._lu}[mode]
        return mode, data.contiguous() if mode == "jacobi" else data
    from .refine import _preconditioner   # (refine imports this module)
    return _preconditioner(Q, n, d, r, precond)


def _certify_lobpcg(measurements, n, d, Xt, *, weights, eta, grad_tol,
                    max_iters, check_every, seed, basis_budget_bytes,
                    basis_size, keep, block_size, precond, problem,
                    lmax_iters, start_block) -> CertificateResult:
    """certify_solution(method="lobpcg"); see there."""
    from .ops.cpu_ref import (LOB_P, LOB_W, LOB_X, LobWorkspace,
                              lob_set_coefficients)
    N, r = Xt.shape
    if basis_size is not None or keep is not None:
        raise ValueError("basis_size and keep belong to method='lanczos'")
    if block_size is None:
        m = default_block_size(d, r, N)
    else:
        m = int(block_size)
    if m not in CERT_SHAPES[d] or 3 * m > N:
        raise ValueError(
            f"block_size={m}: needs a compiled block size of d={d} "
            f"({CERT_SHAPES[d][0]}..{CERT_SHAPES[d][-1]}) with 3 m <= N={N}")
    if lmax_iters < 1 or max_iters < 1:
        raise ValueError("lmax_iters and max_iters must be at least 1")
    if problem is None and precond not in ("auto", "dense", "jacobi",
                                           "exact"):
        raise ValueError(f"unknown precond {precond!r}: 'auto', 'dense', "
                         "'jacobi' or 'exact'")
    ml = int(min(lmax_iters, N))
    need = 8 * N * (ml + 1) + 8 * 7 * N * m
    if need > basis_budget_bytes:
        raise BasisBudgetError(
            f"LOBPCG needs {need} bytes (N={N}: {ml + 1} Lanczos vectors "
            f"and 7 blocks of {m} columns) but basis_budget_bytes="
            f"{basis_budget_bytes}; raise the budget or lower lmax_iters "
            "or block_size")
    dev = Xt.device
    Xt = Xt.to(torch.float64).contiguous()
    if isinstance(weights, Tensor):
        weights = weights.detach().cpu().tolist()
    Q = assemble_connection_laplacian(measurements, n, d, weights)
    if dev.type != "cpu":
        Q = Q.to(dev)
    lam, grad_norm = certificate_operator(Q, Xt)
    bound = _inf_norm_bound(Q, lam)
    nan = float("nan")
    if grad_tol is None:
        grad_tol = 1e-4 * float(np.sqrt(bound))
    apps = 0

    def result(status, theta, resid, lmax, its, y, mode=None, drops=0):
        return CertificateResult(status, theta, resid, lmax, grad_norm, its,
                                 y, method="lobpcg", block_size=m,
                                 precond=mode, applications=apps,
                                 basis_drops=drops)

    if not grad_norm <= grad_tol:
        return result(CertificateStatus.NOT_CRITICAL, nan, nan, nan, 0, None)

    def decide(theta, resid, lmax, lmax_ok, exact=False):
        eta_now = eta if eta is not None else 1e-6 * (
            lmax if lmax_ok else bound)
        if theta < -eta_now:
            return CertificateStatus.NOT_OPTIMAL
        if exact or (lmax_ok and resid <= eta_now):
            return CertificateStatus.CERTIFIED
        return CertificateStatus.INCONCLUSIVE

    # ---- lambda_max phase: the unrestarted Lanczos kernels, untouched
    be = ops.backend_for(Xt)
    g = torch.Generator().manual_seed(seed)
    v0 = torch.randn(N, dtype=torch.float64, generator=g)
    v0 /= torch.linalg.norm(v0)
    V = torch.zeros(ml + 1, N, dtype=torch.float64, device=dev)
    V[0] = v0.to(dev)
    ctl_host = torch.zeros(CERT_HDR + 2 * ml, dtype=torch.float64)
    ctl_host[CERT_TOL] = BREAKDOWN_TOL * bound
    ctl = ctl_host.to(dev)
    done = 0
    while True:
        nsteps = min(check_every, ml - done)
        be.cert_lanczos_steps(Q, lam, V, ctl, done, nsteps)
        h = ctl.cpu().numpy()
        k = int(h[CERT_COUNT])
        broke = bool(h[CERT_FLAG] != 0.0)
        done += nsteps
        theta, u, resid, lmax, resid_max = _ritz(
            h[CERT_HDR:CERT_HDR + k], h[CERT_HDR + ml:CERT_HDR + ml + k])
        lmax_ok = broke or resid_max <= LMAX_RTOL * abs(lmax)
        status = decide(theta, resid, lmax, lmax_ok, broke)
        if broke or status == CertificateStatus.NOT_OPTIMAL:
            apps = k
            y = torch.from_numpy(u.copy()).to(dev) @ V[:k]
            y /= torch.linalg.norm(y)
            return result(status, theta, resid, lmax, 0, y)
        if lmax_ok or done >= ml:
            break
    apps = k
    del V

    # ---- LOBPCG
    pre = _lob_preconditioner(Q, n, d, r, precond, problem)
    mode = pre[0]
    ws = LobWorkspace(N, m, dev)
    if start_block is None:
        g = torch.Generator().manual_seed(seed + 1)
        X0 = torch.randn(N, m, dtype=torch.float64, generator=g)
    else:
        X0 = start_block.detach().to("cpu", torch.float64)
        if X0.shape != (N, m):
            raise ValueError(f"start_block must be ({N}, {m})")
    ws.B[LOB_X].copy_(X0)
    ctl_host = torch.zeros_like(ws.ctl, device="cpu")
    drops = 0

    def upload(theta_new, C):
        lob_set_coefficients(ctl_host, theta_new, C, m)
        ws.ctl.copy_(ctl_host)
        be.cert_lob_update(ws)

    def fresh(j):
        """theta, the true residual norm and the unit vector of column j
        from a new application of S (no recurrence)."""
        nonlocal apps
        v = ws.B[LOB_X][:, j].contiguous()
        v = v / torch.linalg.norm(v)
        w, alpha = be.cert_apply(Q, lam, v)
        apps += 1
        th = float(alpha[0])
        return th, float(torch.linalg.norm(w - th * v)), v

    be.cert_lob_apply(Q, lam, ws, LOB_X)
    be.cert_lob_gram(ws)
    apps += m
    GB, GA, _ = ws.unpack()
    rr = _lob_rayleigh_ritz(GB, GA, m, range(m))
    if rr is None:
        raise ValueError("LOBPCG start block is rank deficient")
    upload(*rr)
    have_p = False
    tiny2 = (BREAKDOWN_TOL * bound) ** 2
    it = 0
    while True:
        it += 1
        be.cert_lob_iter(Q, lam, ws, pre)
        apps += m
        # the one device-to-host read of the iteration
        GB, GA, rn2 = ws.unpack()
        xn2 = np.diag(GB)[:m]
        with np.errstate(all="ignore"):
            rq = np.diag(GA)[:m] / xn2
            res = np.sqrt(rn2 / xn2)
        ok = np.isfinite(rq) & np.isfinite(res)
        j = int(np.argmin(np.where(ok, rq, np.inf)))
        status = (decide(rq[j], res[j], lmax, lmax_ok) if ok[j]
                  else CertificateStatus.INCONCLUSIVE)
        # lambda_max did not converge, so CERTIFIED is not available, and
        # the smallest pair has converged at the scale of the Ritz value
        # of lambda_max (a lower bound): more iterations cannot change
        # the verdict
        stuck = bool(not lmax_ok and ok[j] and res[j] <= (
            eta if eta is not None else 1e-6 * abs(lmax)))
        if (status != CertificateStatus.INCONCLUSIVE or it >= max_iters
                or stuck or not ok.all()):
            th, rs, v = fresh(j)
            status = decide(th, rs, lmax, lmax_ok)
            if (status != CertificateStatus.INCONCLUSIVE or it >= max_iters
                    or stuck or not ok.all()):
                return result(status, th, rs, lmax, it, v, mode, drops)
            # the recurrences of SX and SP have drifted from S X and S P:
            # rebuild both and take the next iteration from there
            be.cert_lob_apply(Q, lam, ws, LOB_X)
            be.cert_lob_apply(Q, lam, ws, LOB_P)
            apps += 2 * m
            continue
        # columns of W whose residual has vanished (an exact eigenvector
        # in the block) are rounding noise and stay out of the basis
        w_ok = (rn2 > tiny2 * xn2) & (np.diag(GB)[m:2 * m] > 0.0)
        p_ok = (np.diag(GB)[2 * m:] > 0.0) & have_p
        if not w_ok.all():
            drops += 1
        xs = list(range(m))
        wsel = [m + c for c in range(m) if w_ok[c]]
        psel = [2 * m + c for c in range(m) if p_ok[c]]
        rr = _lob_rayleigh_ritz(GB, GA, m, xs + wsel + psel)
        if rr is None and psel:
            drops += 1              # drop P, retry on [X W]
            psel = []
            rr = _lob_rayleigh_ritz(GB, GA, m, xs + wsel)
        if rr is None and wsel:
            drops += 1              # drop W too: re-orthonormalise X
            wsel = []
            rr = _lob_rayleigh_ritz(GB, GA, m, xs)
        if rr is None:
            th, rs, v = fresh(j)
            return result(decide(th, rs, lmax, lmax_ok), th, rs, lmax, it, v,
                          mode, drops)
        upload(*rr)
        have_p = bool(wsel or psel)


def escape_direction(Q: BSRMatrix, Xt: Tensor, direction: Tensor, *,
                     max_backtracks: int = 20) -> Tensor:
    """One saddle-escape (staircase) step: the rank-(r+1) iterate
    retract([Xt, 0] + a * [0, direction]), a halved from 1 until the cost
    strictly decreases. `direction` is a negative-curvature vector of S
    (CertificateResult.direction of a NOT_OPTIMAL result): the step is
    tangent at [Xt, 0] and the cost changes by a^2/2 * v^T S v + O(a^3).

    Raises ValueError if rank r + 1 is outside the compiled shape table
    and RuntimeError if no decrease is found within max_backtracks."""
    d = _d_of(Q)
    N, r = Xt.shape
    cert_check_shape(d, r + 1)
    assert direction.shape == (N,)
    problem = QuadraticProblem(Q.n, d, r + 1)
    problem.Q = Q           # cost oracle only: no preconditioner needed
    X0 = torch.zeros(N, r + 1, dtype=torch.float64, device=Xt.device)
    X0[:, :r] = Xt
    step = torch.zeros_like(X0)
    step[:, r] = direction.to(Xt.device)
    f0 = problem.f(X0)
    a = 1.0
    for _ in range(max_backtracks + 1):
        X1 = problem.manifold.retract(X0, a * step)
        if problem.f(X1) < f0:
            return X1
        a *= 0.5
    raise RuntimeError(
        f"escape_direction: no cost decrease within {max_backtracks} "
        "backtracks; is `direction` a negative-curvature direction of S?")
