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
budget and no longer a memory one.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .ops.cpu_ref import (CERT_COUNT, CERT_FLAG, CERT_HDR, CERT_KEEP_MAX,
                          CERT_TOL, cert_check_shape)
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

    def as_dict(self) -> dict:
        """JSON-safe summary (no direction; values not computed are None).
        `certificate_restarts` appears only for a basis_size run."""
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
                     keep: Optional[Tuple[int, int]] = None
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
    """
    assert Xt.dim() == 2 and Xt.shape[0] == n * (d + 1)
    N, r = Xt.shape
    cert_check_shape(d, r)
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
