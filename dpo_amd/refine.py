"""Certified solve: global second-order refinement of a gathered RBCD
iterate and the Riemannian staircase around the optimality certificate.

`refine_to_critical` runs a Riemannian trust region (Steihaug-Toint
preconditioned tCG, the scalar logic of `solver.trust_region` batch mode)
on f(X) = 0.5 <Q, X^T X> over the whole graph until the gradient norm is
below the certificate's criticality gate. On a GPU tensor every stage is
a HIP kernel and the control array stays on the device: the host reads it
once per batch of `check_every` tCG iterations (docs/DESIGN.md §17).
There is no cap on inner iterations and no Krylov history.

`certified_solve` alternates refine -> `certify_solution` and, on a
NOT_OPTIMAL verdict, lifts the iterate to rank r + 1 along the negative
curvature direction (`escape_direction`) and repeats.
"""
from __future__ import annotations

import time
import warnings
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .certify import (CertificateResult, CertificateStatus, _d_of,
                      _inf_norm_bound, certificate_operator,
                      certify_solution, escape_direction)
from .ops.cpu_ref import (CERT_SHAPES, REFINE_TCG_NAMES, RF_FX, RF_GN2,
                          RF_INNER, RF_OUTER, RF_REJECTED, RF_STATUS,
                          RF_STREAK, RF_TCG, RS_CONVERGED, RS_RUN,
                          RS_TCG_DONE, RefineWorkspace, cert_check_shape,
                          refine_control)
from .quadratic import (BSRMatrix, QuadraticProblem,
                        assemble_connection_laplacian)
from .rounding import RoundingResult

Tensor = torch.Tensor

# rejected candidates in a row after which the radius has shrunk by
# 4^-10 and the refinement gives up
STALL_REJECTIONS = 10


@dataclass
class RefineResult:
    Xt: Tensor
    status: str             # CONVERGED | MAX_OUTER | TIME_LIMIT | STALLED
    f_init: float
    f_final: float
    grad_norm_init: float
    grad_norm_final: float
    grad_tol: float
    outer_steps: int        # candidates evaluated
    inner_iterations: int   # tCG iterations over all outer steps
    rejected: int           # candidates rejected
    tcg_status: str         # how the last tCG ended
    precond: str
    elapsed_s: float

    def as_dict(self) -> dict:
        """JSON-safe summary (no Xt)."""
        return {"refine_status": self.status,
                "refine_f_init": self.f_init,
                "refine_f_final": self.f_final,
                "refine_grad_norm_init": self.grad_norm_init,
                "refine_grad_norm_final": self.grad_norm_final,
                "refine_grad_tol": self.grad_tol,
                "refine_outer": self.outer_steps,
                "refine_inner": self.inner_iterations,
                "refine_rejected": self.rejected,
                "refine_tcg_status": self.tcg_status,
                "refine_precond": self.precond,
                "refine_seconds": self.elapsed_s}


def default_grad_tol(Q: BSRMatrix, Xt: Tensor) -> float:
    """Half of `certify_solution`'s default criticality gate
    1e-4 sqrt(||S||_inf) at Xt. Half, because the certificate evaluates
    the gate again at the refined iterate, where Lambda differs a little."""
    lam, _ = certificate_operator(Q, Xt)
    return 0.5 * 1e-4 * float(np.sqrt(_inf_norm_bound(Q, lam)))


def _preconditioner(Q: BSRMatrix, n: int, d: int, r: int, precond):
    if isinstance(precond, tuple):      # built by the caller, (mode, data)
        return precond
    problem = QuadraticProblem(n, d, r, precond=precond)
    try:
        problem.set_q(Q)
    except RuntimeError as e:
        # the dense N x N factorisation can fail inside the solver
        # library well below the size cap (seen at N = 20000); under
        # "auto" take the other preconditioner and say so
        if precond != "auto":
            raise
        warnings.warn(f"dense preconditioner failed ({e}); using "
                      "block-Jacobi", RuntimeWarning)
        problem = QuadraticProblem(n, d, r, precond="jacobi")
        problem.set_q(Q)
    mode = problem._active_precond
    data = {"jacobi": problem._Lpre, "dense": problem._Minv,
            "exact": problem._lu}[mode]
    if mode == "jacobi":
        data = data.contiguous()
    return mode, data


def build_preconditioner(Q: BSRMatrix, r: int, precond: str = "auto"):
    """The `(mode, data)` pair `refine_to_critical` builds for Q at rank
    r, for callers that refine more than once with one Q."""
    return _preconditioner(Q, Q.n, _d_of(Q), r, precond)


def refine_to_critical(Q: BSRMatrix, Xt: Tensor, *,
                       grad_tol: Optional[float] = None,
                       precond="auto", Delta0: float = 10.0,
                       max_outer: int = 100, max_inner: int = 1000,
                       check_every: int = 16,
                       time_limit_s: Optional[float] = None) -> RefineResult:
    """Riemannian trust region from Xt (N, r) on Q's device until
    ||grad f|| <= grad_tol (default: `default_grad_tol`).

    precond   "auto" takes what `QuadraticProblem.set_q` chooses: on a GPU
              the dense fp32 inverse up to N = 24576 and block-Jacobi
              above, on the CPU the exact sparse factorisation. "jacobi"
              and "dense" force one; only block-Jacobi is bit-reproducible
              on the GPU. A `(mode, data)` pair from `build_preconditioner`
              is used as it is (one build for several refinements).
    max_inner tCG iteration budget per outer step (no cap of 16).
    check_every
              tCG iterations enqueued between two reads of the control
              array.
    Status STALLED means ten candidates in a row were rejected. Raises
    ValueError for a (d, r) outside the compiled shape table."""
    d = _d_of(Q)
    assert Xt.dim() == 2 and Xt.shape[0] == Q.N
    N, r = Xt.shape
    cert_check_shape(d, r)
    if check_every < 1:
        raise ValueError("check_every must be at least 1")
    t0 = time.perf_counter()
    Xt = Xt.to(torch.float64).contiguous()
    if grad_tol is None:
        grad_tol = default_grad_tol(Q, Xt)
    be = ops.backend_for(Xt)
    ws = RefineWorkspace(Xt)
    ctl = refine_control(grad_tol, Delta0, max_inner, Xt.device)
    # max_outer = 0 runs the head alone (f and the gradient norm of the
    # input): block-Jacobi then, the cheapest to build
    pre = _preconditioner(Q, Q.n, d, r,
                          precond if max_outer > 0 else "jacobi")
    mode = pre[0]

    def read():
        return ctl.cpu().tolist()   # the one device-to-host read

    be.refine_head(Q, ws, ctl, d, pre)
    if max_outer > 0:
        be.refine_tcg_steps(Q, ws, ctl, d, pre, check_every)
    h = read()
    f_init, gn_init = h[RF_FX], float(np.sqrt(h[RF_GN2]))
    status = None
    while status is None:
        st = int(h[RF_STATUS])
        if st == RS_CONVERGED:
            status = "CONVERGED"
        elif int(h[RF_OUTER]) >= max_outer:
            status = "MAX_OUTER"
        elif int(h[RF_STREAK]) >= STALL_REJECTIONS:
            status = "STALLED"
        elif (time_limit_s is not None
              and time.perf_counter() - t0 > time_limit_s):
            status = "TIME_LIMIT"
        else:
            assert st in (RS_RUN, RS_TCG_DONE), f"refine status {st}"
            if st == RS_TCG_DONE:
                # candidate, then the next step's head and first batch:
                # the guards turn whatever does not apply into no-ops
                be.refine_candidate(Q, ws, ctl, d)
                be.refine_head(Q, ws, ctl, d, pre)
            be.refine_tcg_steps(Q, ws, ctl, d, pre, check_every)
            h = read()
    return RefineResult(
        ws.X, status, f_init, h[RF_FX], gn_init,
        float(np.sqrt(h[RF_GN2])), float(grad_tol), int(h[RF_OUTER]),
        int(h[RF_INNER]), int(h[RF_REJECTED]),
        REFINE_TCG_NAMES[int(h[RF_TCG])], mode,
        time.perf_counter() - t0)


@dataclass
class StaircaseLevel:
    rank: int
    refine: RefineResult
    certificate: CertificateResult

    def as_dict(self) -> dict:
        out = {"rank": self.rank}
        out.update(self.refine.as_dict())
        out.update(self.certificate.as_dict())
        return out


@dataclass
class StaircaseResult:
    Xt: Tensor
    rank: int
    certificate: CertificateResult
    levels: List[StaircaseLevel] = field(default_factory=list)
    # certified_solve(round=True): the SE(d) rounding of Xt
    rounding: Optional["RoundingResult"] = None

    @property
    def status(self) -> CertificateStatus:
        return self.certificate.status

    def as_dict(self) -> dict:
        """The last level's refine and certificate fields, the level
        records, `staircase_levels` and `final_rank`; with a rounding,
        its `RoundingResult.as_dict()` fields as well."""
        out = self.levels[-1].refine.as_dict()
        out.update(self.certificate.as_dict())
        out["staircase_levels"] = len(self.levels)
        out["final_rank"] = self.rank
        out["levels"] = [lv.as_dict() for lv in self.levels]
        if self.rounding is not None:
            out.update(self.rounding.as_dict())
        return out


def certified_solve(measurements, n: int, d: int, Xt: Tensor, *,
                    weights: Optional[Sequence[float]] = None,
                    max_rank: Optional[int] = None,
                    refine_kw: Optional[dict] = None,
                    certify_kw: Optional[dict] = None,
                    round: bool = False) -> StaircaseResult:
    """Riemannian staircase from the lifted iterate Xt (N, r): refine to
    criticality, certify, and on NOT_OPTIMAL escape to rank r + 1 and
    repeat. Stops on any other verdict, or with NOT_OPTIMAL when r + 1 is
    outside the compiled shapes or above `max_rank`. Q is assembled once;
    `refine_kw` / `certify_kw` go to `refine_to_critical` /
    `certify_solution`; with `certify_kw["method"] == "lobpcg"` the
    preconditioner of Q is built once and handed to both (`precond=` and
    `problem=`). With `round=True` the final level's iterate is
    rounded to SE(d) on its device (`rounding.round_solution`,
    mode="svd") and the result carries it as `rounding`: the trajectory,
    its cost and the suboptimality gap, which bounds the distance to the
    global optimum when the verdict is CERTIFIED."""
    assert Xt.dim() == 2 and Xt.shape[0] == n * (d + 1)
    cert_check_shape(d, Xt.shape[1])
    top = max(CERT_SHAPES[d])
    max_rank = top if max_rank is None else min(int(max_rank), top)
    refine_kw = dict(refine_kw or {})
    certify_kw = dict(certify_kw or {})
    if isinstance(weights, Tensor):
        weights = weights.detach().cpu().tolist()
    Q = assemble_connection_laplacian(measurements, n, d, weights)
    if Xt.device.type != "cpu":
        Q = Q.to(Xt.device)
    X = Xt.to(torch.float64).contiguous()
    if (certify_kw.get("method") == "lobpcg"
            and certify_kw.get("problem") is None):
        # one preconditioner of Q (it does not depend on the rank) for
        # the refinement and the LOBPCG certificate of every level
        pre = refine_kw.get("precond", "auto")
        if not isinstance(pre, tuple):
            pre = _preconditioner(Q, n, d, X.shape[1], pre)
        refine_kw["precond"] = certify_kw["problem"] = pre
    levels: List[StaircaseLevel] = []
    while True:
        r = X.shape[1]
        ref = refine_to_critical(Q, X, **refine_kw)
        cert = certify_solution(measurements, n, d, ref.Xt, weights=weights,
                                **certify_kw)
        levels.append(StaircaseLevel(r, ref, cert))
        if (cert.status != CertificateStatus.NOT_OPTIMAL
                or r + 1 > max_rank):
            rounding = None
            if round:
                from .rounding import round_solution
                rounding = round_solution(Q, ref.Xt, d, mode="svd")
            return StaircaseResult(ref.Xt, r, cert, levels, rounding)
        X = escape_direction(Q, ref.Xt, cert.direction)
