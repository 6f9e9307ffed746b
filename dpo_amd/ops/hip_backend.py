"""ctypes bindings for the dpo_amd HIP extension + GPU op implementations.

Mirrors the cpu_ref op interface for CUDA (ROCm) tensors, and provides
DeviceSolver — the device-resident RBCD trust-region local solve with
on-GPU tCG control (one host sync per solve in the common case).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

Tensor = torch.Tensor

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "hip", "libdpo_hip_ops.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(f"HIP extension not built: {_LIB_PATH}")

_lib = ctypes.CDLL(_LIB_PATH)

_c = ctypes.c_void_p
_i = ctypes.c_int
_l = ctypes.c_long
_d = ctypes.c_double

_lib.dpo_bsr_spmm.argtypes = [_c, _c, _c, _i, _i, _c, _c, _i, _c, _i, _c]
_lib.dpo_bsr_spmm_mfma.argtypes = [_c, _c, _c, _c, _c, _c, _i, _i, _i, _c]
_lib.dpo_proj_dots.argtypes = [_c, _c, _c, _c, _c, _c, _i, _i, _i, _i, _i,
                               _i, _i, _c]
_lib.dpo_polar_affine.argtypes = [_c, _c, _c, _d, _d, _d, _c, _i, _i, _i,
                                  _c, _i, _c]
_lib.dpo_precond_dense.argtypes = [_c, _c, _c, _i, _i, _c, _i, _c]
_lib.dpo_precond_jacobi.argtypes = [_c, _c, _c, _i, _i, _i, _c, _i, _c]
_lib.dpo_tcg_update.argtypes = [_c, _c, _c, _c, _c, _c, _c, _l, _c]
_lib.dpo_tcg_delta.argtypes = [_c, _c, _c, _l, _c]
_lib.dpo_form_step.argtypes = [_c, _c, _c, _c, _c, _l, _c]
_lib.dpo_axpby.argtypes = [_c, _c, _d, _d, _c, _l, _c]
_lib.dpo_dots.argtypes = [_c, _c, _c, _c, _i, _i, _l, _i, _c]
_lib.dpo_ctrl_init.argtypes = [_c, _d, _d, _d, _d, _c]
for name in ("dpo_ctrl_z0", "dpo_ctrl_alpha", "dpo_ctrl_rr", "dpo_ctrl_beta",
             "dpo_ctrl_tcg_end", "dpo_ctrl_candidate", "dpo_ctrl_shrink"):
    getattr(_lib, name).argtypes = [_c, _c]
_lib.dpo_ctrl_accept.argtypes = [_c, _d, _c]
_lib.dpo_q_assemble.argtypes = [_c, _c, _c, _c, _c, _i, _i, _l, _c]
_lib.dpo_g_assemble.argtypes = [_c, _c, _c, _c, _c, _c, _i, _i, _i, _l, _c]
_lib.dpo_ctrl_size.restype = _i
_lib.dpo_ctx_create.restype = _c
_lib.dpo_ctx_create.argtypes = [_i, _i, _i, _i]
_lib.dpo_ctx_destroy.argtypes = [_c]
_lib.dpo_ctx_set_problem.argtypes = [_c, _c, _c, _c, _c, _c, _c]
_lib.dpo_rbcd_solve.restype = _i
_lib.dpo_rbcd_solve.argtypes = [_c, _c, _d, _d, _i, _d, _i,
                                ctypes.POINTER(ctypes.c_double), _c]
_lib.dpo_eval_terms.argtypes = [_c, _c, _c, _c]
_lib.dpo_ctx_set_gdata.argtypes = [_c, _c, _c, _c, _c, _i]
_lib.dpo_round_solve.restype = _i
_lib.dpo_round_solve.argtypes = [_c, _c, _c, _d, _d, _i, _d,
                                 ctypes.POINTER(ctypes.c_double), _c]
_lib.dpo_round_eval.argtypes = [_c, _c, _c, _c, _c]
_lib.dpo_round_solve_async.argtypes = [_c, _c, _c, _d, _d, _d, _c]
_lib.dpo_round_solve_finish.restype = _i
_lib.dpo_round_solve_finish.argtypes = [
    _c, _i, ctypes.POINTER(ctypes.c_double), _c]
_lib.dpo_tcg_segment.restype = _i
_lib.dpo_tcg_segment.argtypes = [_c]
_lib.dpo_ctx_counters.restype = _i
_lib.dpo_ctx_counters.argtypes = [_c, ctypes.POINTER(ctypes.c_long), _i]
_lib.dpo_round_eval_async.argtypes = [_c, _c, _c, _c, _c]
_lib.dpo_eval_join.argtypes = [_c, _c]
_lib.dpo_gnc_weights.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c, _c,
                                 _c, _c, _c, _i, _i, _i, _d, _d, _c]
_lib.dpo_group_create.restype = _c
_lib.dpo_group_create.argtypes = [
    ctypes.POINTER(ctypes.c_void_p), _i, ctypes.POINTER(ctypes.c_void_p),
    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)]
_lib.dpo_group_destroy.argtypes = [_c]
_lib.dpo_group_solve_start.argtypes = [
    _c, ctypes.POINTER(ctypes.c_int), _i, _d, _d, _d, _c]
_lib.dpo_group_solve_finish.argtypes = [
    _c, ctypes.POINTER(ctypes.c_int), _i, _i, _c]
_lib.dpo_group_eval.argtypes = [_c, _c, _l, _c]
_lib.dpo_group_counters.restype = _i
_lib.dpo_group_counters.argtypes = [_c, ctypes.POINTER(ctypes.c_long), _i]
_lib.dpo_batch_desc_size.restype = _i
_lib.dpo_batch_op.restype = _i
_lib.dpo_batch_op.argtypes = [_i, _c, _i, _i, _i, _d, _d, _c]
_lib.dpo_ctx_ctrl.restype = _i
_lib.dpo_ctx_ctrl.argtypes = [_c, ctypes.POINTER(ctypes.c_double), _i]
_lib.dpo_hd_stage.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c, _i, _i,
                              _i, _i, _c]
_lib.dpo_candidate.argtypes = [_c, _c, _c, _c, _c, _c, _c, _i, _i, _i, _c]
_lib.dpo_hess_tail.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _i, _i, _i,
                               _i, _i, _d, _d, _c, _c]

CTRL_SIZE = _lib.dpo_ctrl_size()

# ctrl slots mirrored from dpo_ops.hip
C_STATUS, C_FX, C_GN0SQ = 0, 1, 2
C_RR, C_ZR, C_EPE, C_EPD, C_DPD, C_COEF, C_BETA, C_ITER, C_J = range(3, 12)
C_RADIUS, C_FPROP, C_DM = 12, 13, 14
C_JSTAR, C_TAUSTAR, C_USE_CURRENT, C_STOP_PENDING, C_BOUND = range(15, 20)
C_GN1SQ, C_RHO, C_HLEN, C_SHRINKS = 20, 21, 22, 23
C_DOT0, C_DOT1, C_DOT2, C_DOT3 = 24, 25, 26, 27
C_HIST = 32  # z_r, d_Hd, e_Pe, e_Pd, d_Pd histories, MAX_TCG entries each
ST_RUN, ST_TCG_STOP, ST_ACCEPTED, ST_GIVE_UP, ST_NO_UPDATE = range(5)
MAX_TCG = 16
GUARD_NONE, GUARD_RUN, GUARD_STOP = -1, ST_RUN, ST_TCG_STOP


def _p(t: Optional[Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(t: Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(t: Tensor, dtype=torch.float64):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous()


def _check_shape(d: Optional[int], r: Optional[int]) -> None:
    """Raise ValueError unless (d, r) is a compiled kernel shape; the
    native launchers abort the process on anything else. d = None
    checks r alone (ops templated on r only)."""
    from .cpu_ref import CERT_SHAPES, cert_check_shape
    if d is not None:
        cert_check_shape(d, r)
    elif not any(r in rs for rs in CERT_SHAPES.values()):
        raise ValueError(
            f"unsupported r={r}: compiled shapes have r in 2..8")


# ---------------------------------------------------------------------
# op interface (mirrors cpu_ref)
# ---------------------------------------------------------------------
def tangent_project(X: Tensor, V: Tensor, d: int) -> Tensor:
    _chk(X); _chk(V)
    n = X.shape[0] // (d + 1)
    r = X.shape[1]
    _check_shape(d, r)
    out = torch.empty_like(V)
    _lib.dpo_proj_dots(_p(X), _p(V), None, _p(out), None, None,
                       n, d, r, -1, -1, 0, GUARD_NONE, _stream(X))
    return out


def stiefel_project(M: Tensor, d: int) -> Tensor:
    """Per-pose polar factor of the d x r Stiefel block; translation
    rows pass through.

    Domain: the kernel iterates (Newton-Schulz, at most 40 steps) on the
    d x d Gram matrix M M^T, so its error against the SVD polar factor
    is about eps * cond(M)^2: 1e-12 at cond 1e2, 1e-8 at 1e4, 1e-4 at
    1e6. Beyond cond(M) ~ 1e6 the result is silently not orthonormal. A
    block whose Gram trace underflows (<= 1e-300) gives a zero block.
    Retractions stay inside the domain: for X on the manifold and a
    tangent eta the Gram matrix is I + eta eta^T, cond <= sqrt(1 +
    ||eta||^2)."""
    _chk(M)
    n = M.shape[0] // (d + 1)
    r = M.shape[1]
    _check_shape(d, r)
    out = torch.empty_like(M)
    _lib.dpo_polar_affine(_p(M), None, None, 1.0, 0.0, 0.0, _p(out),
                          n, d, r, None, GUARD_NONE, _stream(M))
    return out


def retract(X: Tensor, eta: Tensor, d: int) -> Tensor:
    _chk(X); _chk(eta)
    n = X.shape[0] // (d + 1)
    r = X.shape[1]
    _check_shape(d, r)
    out = torch.empty_like(X)
    _lib.dpo_polar_affine(_p(X), _p(eta), None, 1.0, 1.0, 0.0, _p(out),
                          n, d, r, None, GUARD_NONE, _stream(X))
    return out


def polar_affine(A: Tensor, B: Optional[Tensor], C: Optional[Tensor],
                 ca: float, cb: float, cc: float, d: int) -> Tensor:
    _chk(A)
    n = A.shape[0] // (d + 1)
    r = A.shape[1]
    _check_shape(d, r)
    out = torch.empty_like(A)
    _lib.dpo_polar_affine(_p(A), _p(B), _p(C), ca, cb, cc, _p(out),
                          n, d, r, None, GUARD_NONE, _stream(A))
    return out


def bsr_spmm(row_ptr: Tensor, col_idx: Tensor, vals: Tensor, n: int,
             dh: int, X: Tensor, out: Optional[Tensor] = None,
             ctrl: Optional[Tensor] = None, guard: int = GUARD_NONE) -> Tensor:
    _chk(vals); _chk(X)
    r = X.shape[1]
    # shapes outside the compiled table take the generic kernel, which
    # needs at least one dh x r tile per 256-thread block
    if dh < 1 or r < 1 or dh * r > 256:
        raise ValueError(f"unsupported (dh={dh}, r={r}): needs dh*r <= 256")
    if out is None:
        out = torch.empty_like(X)
    _lib.dpo_bsr_spmm(_p(row_ptr), _p(col_idx), _p(vals), n, dh,
                      _p(X), _p(out), r, _p(ctrl), guard, _stream(X))
    return out


def build_spmm_mfma_groups(row_ptr, col_idx, n: int):
    """Host-side grouped-ELL structure for the fp64-MFMA SpMM A/B
    kernel (d = 3): 4-pose row groups with per-group column unions.
    Returns (grp_ptr, grp_cols, grp_blk) numpy int32 arrays; grp_blk has
    4 entries per (group, union-column) = the Q block index of each pose
    in the group for that column, or -1."""
    import numpy as np
    rp = row_ptr.cpu().numpy() if isinstance(row_ptr, Tensor) else row_ptr
    ci = col_idx.cpu().numpy() if isinstance(col_idx, Tensor) else col_idx
    ngroups = (n + 3) // 4
    grp_ptr = [0]
    grp_cols = []
    grp_blk = []
    for g in range(ngroups):
        rows = range(g * 4, min(g * 4 + 4, n))
        union = {}
        for pi, i in enumerate(rows):
            for p in range(rp[i], rp[i + 1]):
                union.setdefault(int(ci[p]), [-1, -1, -1, -1])[pi] = p
        for j in sorted(union):
            grp_cols.append(j)
            grp_blk.extend(union[j])
        grp_ptr.append(len(grp_cols))
    return (np.asarray(grp_ptr, dtype=np.int32),
            np.asarray(grp_cols, dtype=np.int32),
            np.asarray(grp_blk, dtype=np.int32))


def bsr_spmm_mfma(grp_ptr: Tensor, grp_cols: Tensor, grp_blk: Tensor,
                  vals: Tensor, X: Tensor,
                  out: Optional[Tensor] = None) -> Tensor:
    """fp64-MFMA SpMM (d=3 / dh=4 only); A/B study kernel."""
    _chk(vals); _chk(X)
    r = X.shape[1]
    n = X.shape[0] // 4
    if out is None:
        out = torch.empty_like(X)
    _lib.dpo_bsr_spmm_mfma(_p(grp_ptr), _p(grp_cols), _p(grp_blk),
                           _p(vals), _p(X), _p(out),
                           int(grp_ptr.numel() - 1), n, r, _stream(X))
    return out


def precond_dense(Minv: Tensor, V: Tensor,
                  out: Optional[Tensor] = None,
                  ctrl: Optional[Tensor] = None,
                  guard: int = GUARD_NONE) -> Tensor:
    _chk(Minv, torch.float32); _chk(V)
    N, r = V.shape
    _check_shape(None, r)
    if out is None:
        out = torch.empty_like(V)
    _lib.dpo_precond_dense(_p(Minv), _p(V), _p(out), N, r, _p(ctrl), guard,
                           _stream(V))
    return out


def precond_jacobi(L: Tensor, V: Tensor, dh: int,
                   out: Optional[Tensor] = None,
                   ctrl: Optional[Tensor] = None,
                   guard: int = GUARD_NONE) -> Tensor:
    _chk(L); _chk(V)
    N, r = V.shape
    if dh not in (3, 4):
        raise ValueError(f"unsupported dh={dh}: compiled for dh in (3, 4)")
    n = N // dh
    if out is None:
        out = torch.empty_like(V)
    _lib.dpo_precond_jacobi(_p(L), _p(V), _p(out), n, dh, r, _p(ctrl),
                            guard, _stream(V))
    return out


def g_assemble(Gt: Tensor, E0: Tensor, local_pose: Tensor, nbr_slot: Tensor,
               nbr: Tensor, w: Tensor, dh: int, r: int) -> Tensor:
    _chk(Gt)
    ne = E0.shape[0]
    N = Gt.shape[0]
    _lib.dpo_g_assemble(_p(Gt), _p(E0), _p(local_pose), _p(nbr_slot),
                        _p(nbr), _p(w), ne, dh, r, N, _stream(Gt))
    return Gt


def q_assemble(vals: Tensor, blocks: Tensor, slots: Tensor, edge_of: Tensor,
               w: Tensor, dh: int) -> Tensor:
    _chk(vals)
    ncontrib = blocks.shape[0]
    nnzb = vals.shape[0]
    _lib.dpo_q_assemble(_p(vals), _p(blocks), _p(slots), _p(edge_of), _p(w),
                        ncontrib, dh * dh, nnzb, _stream(vals))
    return vals


# ---------------------------------------------------------------------
# tCG vector ops. Coefficients, the iteration index and the guard status
# are read from the ctrl block (CTRL_SIZE fp64 slots on the device).
# ---------------------------------------------------------------------
def tcg_update(eta: Tensor, rvec: Tensor, delta: Tensor, Hd: Tensor,
               eta_snap: Tensor, delta_snap: Tensor, ctrl: Tensor) -> None:
    """Snapshot row j = C_ITER, eta += coef * delta, and unless a stop is
    pending r += coef * Hd with ||r||^2 added to C_DOT1. Runs only in
    status ST_RUN."""
    for t in (eta, rvec, delta, Hd, eta_snap, delta_snap, ctrl):
        _chk(t)
    total = eta.numel()
    assert rvec.numel() == delta.numel() == Hd.numel() == total
    assert eta_snap.numel() == delta_snap.numel()
    assert eta_snap.numel() % total == 0 and ctrl.numel() >= CTRL_SIZE
    _lib.dpo_tcg_update(_p(eta), _p(rvec), _p(delta), _p(Hd), _p(eta_snap),
                        _p(delta_snap), _p(ctrl), total, _stream(eta))


def tcg_delta(delta: Tensor, z: Tensor, ctrl: Tensor) -> None:
    """delta = -z + C_BETA * delta in place (status ST_RUN only)."""
    _chk(delta); _chk(z); _chk(ctrl)
    assert z.numel() == delta.numel() and ctrl.numel() >= CTRL_SIZE
    _lib.dpo_tcg_delta(_p(delta), _p(z), _p(ctrl), delta.numel(),
                       _stream(delta))


def form_step(step: Tensor, eta: Tensor, eta_snap: Tensor,
              delta_snap: Tensor, ctrl: Tensor) -> None:
    """step = eta when C_USE_CURRENT, else snapshot row C_JSTAR of eta
    plus C_TAUSTAR times that row of delta (status ST_TCG_STOP only)."""
    for t in (step, eta, eta_snap, delta_snap, ctrl):
        _chk(t)
    total = step.numel()
    assert eta.numel() == total and eta_snap.numel() == delta_snap.numel()
    assert eta_snap.numel() % total == 0 and ctrl.numel() >= CTRL_SIZE
    _lib.dpo_form_step(_p(step), _p(eta), _p(eta_snap), _p(delta_snap),
                       _p(ctrl), total, _stream(step))


def axpby(A: Tensor, B: Optional[Tensor], a: float, b: float,
          out: Optional[Tensor] = None) -> Tensor:
    """out = a * A + b * B (B optional)."""
    _chk(A)
    if B is not None:
        _chk(B)
        assert B.numel() == A.numel()
    if out is None:
        out = torch.empty_like(A)
    _chk(out)
    assert out.numel() == A.numel()
    _lib.dpo_axpby(_p(A), _p(B), a, b, _p(out), A.numel(), _stream(A))
    return out


def dots(A: Tensor, B: Tensor, C: Optional[Tensor], ctrl: Tensor,
         slot: int, slot2: int = -1, guard: int = GUARD_NONE) -> None:
    """ctrl[slot] += <A, B>; with C and slot2 >= 0 also ctrl[slot2] +=
    <A, C>."""
    _chk(A); _chk(B); _chk(ctrl)
    assert B.numel() == A.numel() and ctrl.numel() >= CTRL_SIZE
    assert 0 <= slot < CTRL_SIZE and -1 <= slot2 < CTRL_SIZE
    if C is not None:
        _chk(C)
        assert C.numel() == A.numel()
    _lib.dpo_dots(_p(A), _p(B), _p(C), _p(ctrl), slot, slot2, A.numel(),
                  guard, _stream(A))


def candidate(ctrl: Tensor, step: Tensor, eta: Tensor, eta_snap: Tensor,
              delta_snap: Tensor, X: Tensor, Xprop: Tensor, d: int) -> None:
    """One trust-region candidate in one launch (status ST_TCG_STOP
    only): the selection of dpo_ctrl_candidate, the step of form_step
    and Xprop = polar(X + step)."""
    for t in (ctrl, step, eta, eta_snap, delta_snap, X, Xprop):
        _chk(t)
    r = X.shape[-1]
    _check_shape(d, r)
    total = X.numel()
    n = total // ((d + 1) * r)
    assert step.numel() == eta.numel() == Xprop.numel() == total
    assert eta_snap.numel() == delta_snap.numel()
    assert eta_snap.numel() % total == 0 and ctrl.numel() >= CTRL_SIZE
    _lib.dpo_candidate(_p(ctrl), _p(step), _p(eta), _p(eta_snap),
                       _p(delta_snap), _p(X), _p(Xprop), n, d, r, _stream(X))


def hd_stage(Q, d0: Tensor, d1: Optional[Tensor], z: Tensor, X: Tensor,
             Hd: Tensor, ctrl: Tensor, d: int, fused: bool) -> None:
    """The tCG Hd stage (status ST_RUN only): delta = C_BETA * delta_old
    - z, Hd = P_X(Q delta), <delta, Hd> and the alpha step. fused: one
    kernel that reads delta_old from buffer 1 - (C_ITER & 1) of (d0, d1)
    and writes delta into the other; else tcg_delta in place on d0
    followed by the Hessian kernel."""
    for t in (d0, z, X, Hd, ctrl):
        _chk(t)
    r = X.shape[-1]
    _check_shape(d, r)
    n = X.numel() // ((d + 1) * r)
    assert Q.n == n and ctrl.numel() >= CTRL_SIZE
    assert d0.numel() == z.numel() == Hd.numel() == X.numel()
    if fused:
        _chk(d1)
        assert d1.numel() == X.numel()
    _lib.dpo_hd_stage(_p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals), _p(d0),
                      _p(d1), _p(z), _p(X), _p(Hd), _p(ctrl), n, d, r,
                      1 if fused else 0, _stream(X))


HESS_TAIL_INIT, HESS_TAIL_ACCEPT, HESS_TAIL_EVAL = 1, 2, 3


def hess_tail(Q, V: Tensor, G: Optional[Tensor], ctrl: Tensor, d: int,
              kind: int, fused: bool, a: float = 0.0, b: float = 0.0,
              out: Optional[Tensor] = None, out2: Optional[Tensor] = None,
              out3: Optional[Tensor] = None) -> None:
    """One Hessian stage of the solve or the evaluation together with the
    scalar step behind it: run by the kernel's last block (fused) or as
    the separate launch of the unfused sequence.
      HESS_TAIL_INIT    out = grad f(V), out2 = copy; control init with
                        tol = a, Delta0 = b
      HESS_TAIL_ACCEPT  f(V) dots (status ST_TCG_STOP only); acceptance
                        test with accept_rho = a
      HESS_TAIL_EVAL    out = grad f(V); out3 = [f, 0.5 <V, G>, gn^2]"""
    _chk(V); _chk(ctrl)
    r = V.shape[-1]
    _check_shape(d, r)
    n = V.numel() // ((d + 1) * r)
    assert Q.n == n and ctrl.numel() >= CTRL_SIZE
    assert kind in (HESS_TAIL_INIT, HESS_TAIL_ACCEPT, HESS_TAIL_EVAL)
    for t in (G, out, out2):
        if t is not None:
            _chk(t)
            assert t.numel() == V.numel()
    if kind != HESS_TAIL_ACCEPT:
        assert out is not None
    if kind == HESS_TAIL_INIT:
        assert out2 is not None
    if kind == HESS_TAIL_EVAL:
        assert out3 is not None and out3.numel() >= 3
        _chk(out3)
    _lib.dpo_hess_tail(_p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals), _p(V),
                       _p(G), _p(out), _p(out2), _p(ctrl), n, d, r, kind,
                       1 if fused else 0, a, b, _p(out3), _stream(V))


# ---------------------------------------------------------------------
# Device-resident RBCD local solve
# ---------------------------------------------------------------------
class DeviceSolver:
    """Native (C++) RBCD trust-region local solve with device-resident
    tCG control. Semantics mirror reference QuadraticOptimizer::
    trustRegion with Max_Iteration == 1 (QuadraticOptimizer.cpp:92-110):
    one Steihaug-tCG TR step, radius shrunk /4 until accepted (<= 10
    shrinks). The Krylov path is radius-independent, so rejections replay
    stored snapshots instead of re-running tCG. One host sync per solve
    in the accepted-first-try case; ~1 enqueue call from Python."""

    def __init__(self, n: int, d: int, r: int, device, max_inner: int = 10):
        assert max_inner <= MAX_TCG
        _check_shape(d, r)
        self.n, self.d, self.r = n, d, r
        self.dh = d + 1
        self.N = self.dh * n
        self.max_inner = max_inner
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.handle = _lib.dpo_ctx_create(n, d, r, max_inner)
        self._stats = (ctypes.c_double * 8)()
        self._eval_out = torch.zeros(3, dtype=torch.float64,
                                     device=self.device)
        self._refs = None  # keep problem tensors alive across the call

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.dpo_ctx_destroy(self.handle)
        except Exception:
            pass

    def _bind(self, problem):
        Q = problem.Q
        G = problem.Gt
        Minv = getattr(problem, "_Minv", None)
        Ljac = getattr(problem, "_Lpre", None)
        if Minv is None and Ljac is not None:
            Ljac = Ljac.contiguous()
        self._refs = (Q.row_ptr, Q.col_idx, Q.vals, G, Minv, Ljac)
        _lib.dpo_ctx_set_problem(self.handle, _p(Q.row_ptr), _p(Q.col_idx),
                                 _p(Q.vals), _p(G), _p(Minv), _p(Ljac))

    def solve(self, problem, X: Tensor, tol: float = 1e-2,
              Delta0: float = 100.0, max_shrink: int = 10,
              accept_rho: float = 0.1, compute_final_gradnorm: bool = True):
        """One RBCD local solve in place on X. Returns a stats dict."""
        self._bind(problem)
        status = _lib.dpo_rbcd_solve(
            self.handle, _p(X), tol, Delta0, max_shrink, accept_rho,
            1 if compute_final_gradnorm else 0, self._stats, _stream(X))
        st = self._stats
        return {
            "status": int(st[0]),
            "f_init": st[1],
            "grad_norm_init": st[2],
            "f_opt": st[3],
            "grad_norm_opt": st[4],
            "rho": st[5],
            "shrinks": int(st[6]),
        }

    def tcg_segment(self) -> int:
        """tCG iterations held by the primary solve graph for the problem
        currently bound (DPO_TCG_SEG resolved); == max_inner means one
        graph."""
        return int(_lib.dpo_tcg_segment(self.handle))

    def counters(self) -> dict:
        """Host-side solve statistics of this context: solves finished,
        continuation-graph launches (DPO_TCG_SEG), and the histogram of
        tCG iterations per solve (index = Krylov history length)."""
        buf = (ctypes.c_long * (MAX_TCG + 3))()
        n = _lib.dpo_ctx_counters(self.handle, buf, len(buf))
        assert n == len(buf)
        return {"solves": int(buf[0]), "continuations": int(buf[1]),
                "hlen_hist": [int(v) for v in buf[2:]]}

    def ctrl_block(self) -> list:
        """The device control block, all CTRL_SIZE slots (synchronises)."""
        buf = (ctypes.c_double * CTRL_SIZE)()
        assert _lib.dpo_ctx_ctrl(self.handle, buf, CTRL_SIZE) \
            == CTRL_SIZE
        return list(buf)

    def eval_terms(self, problem, X: Tensor) -> Tensor:
        """Device 3-vector [f(X), 0.5<X,G>, ||rgrad||^2]; no host sync."""
        self._bind(problem)
        _lib.dpo_eval_terms(self.handle, _p(X), _p(self._eval_out),
                            _stream(X))
        return self._eval_out

    # --- fused per-round entry points (G assembled in C++) -----------
    def set_gdata(self, E0: Tensor, local_pose: Tensor, nbr_slot: Tensor,
                  w: Tensor) -> None:
        self._grefs = (E0, local_pose, nbr_slot, w)
        _lib.dpo_ctx_set_gdata(self.handle, _p(E0), _p(local_pose),
                               _p(nbr_slot), _p(w), E0.shape[0])

    def bind_problem_static(self, problem) -> None:
        """Bind the Q/preconditioner pointers once (re-call after a Q
        rebuild). The G term is produced in-C++ by the round calls."""
        Q = problem.Q
        Minv = getattr(problem, "_Minv", None)
        Ljac = getattr(problem, "_Lpre", None)
        if Minv is None and Ljac is not None:
            Ljac = Ljac.contiguous()
        self._refs = (Q.row_ptr, Q.col_idx, Q.vals, None, Minv, Ljac)
        _lib.dpo_ctx_set_problem(self.handle, _p(Q.row_ptr), _p(Q.col_idx),
                                 _p(Q.vals), None, _p(Minv), _p(Ljac))

    def round_solve(self, X: Tensor, nbr: Tensor, tol: float = 1e-2,
                    Delta0: float = 100.0) -> int:
        return _lib.dpo_round_solve(self.handle, _p(X), _p(nbr), tol,
                                    Delta0, 10, 0.1, self._stats,
                                    _stream(X))

    def round_eval(self, X: Tensor, nbr: Tensor,
                   out: Optional[Tensor] = None) -> Tensor:
        dst = self._eval_out if out is None else out
        _lib.dpo_round_eval(self.handle, _p(X), _p(nbr), _p(dst),
                            _stream(X))
        return dst

    # --- async multi-stream variants (overlap concurrent agents) -----
    def round_solve_async(self, X: Tensor, nbr: Tensor, tol: float = 1e-2,
                          Delta0: float = 100.0) -> None:
        _lib.dpo_round_solve_async(self.handle, _p(X), _p(nbr), tol,
                                   Delta0, 0.1, _stream(X))

    def round_solve_finish(self, X: Tensor) -> int:
        return _lib.dpo_round_solve_finish(self.handle, 10, self._stats,
                                           _stream(X))

    def round_eval_async(self, X: Tensor, nbr: Tensor,
                         out: Optional[Tensor] = None) -> Tensor:
        dst = self._eval_out if out is None else out
        _lib.dpo_round_eval_async(self.handle, _p(X), _p(nbr), _p(dst),
                                  _stream(X))
        return dst

    def eval_join(self, X: Tensor) -> Tensor:
        _lib.dpo_eval_join(self.handle, _stream(X))
        return self._eval_out


class DeviceGroup:
    """Multi-agent round fan-out: one C call per phase instead of a
    Python loop over agents (solve fan-out for the active set, eval
    fan-out + single-gather-kernel for every agent). Pointers (X,
    neighbor buffer, eval scratch) are fixed at construction; the
    per-ctx hipGraph caches stay hot."""

    def __init__(self, solvers, Xs, nbrs, rows):
        n = len(solvers)
        assert n == len(Xs) == len(nbrs) == len(rows)
        self._keep = (solvers, Xs, nbrs)
        handles = (ctypes.c_void_p * n)(
            *[ctypes.c_void_p(s.handle) for s in solvers])
        xp = (ctypes.c_void_p * n)(*[ctypes.c_void_p(x.data_ptr())
                                     for x in Xs])
        np_ = (ctypes.c_void_p * n)(*[ctypes.c_void_p(b.data_ptr())
                                      for b in nbrs])
        rw = (ctypes.c_int * n)(*rows)
        self.n = n
        self.handle = _lib.dpo_group_create(handles, n, xp, np_, rw)
        assert self.handle, "dpo_group_create failed"
        self._js_of = Xs[0]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.dpo_group_destroy(self.handle)
        except Exception:
            pass

    def ids(self, idx_list):
        return (ctypes.c_int * len(idx_list))(*idx_list)

    def solve_start(self, ids, tol: float = 1e-2, Delta0: float = 100.0,
                    accept_rho: float = 0.1) -> None:
        _lib.dpo_group_solve_start(self.handle, ids, len(ids), tol,
                                   Delta0, accept_rho,
                                   _stream(self._js_of))

    def solve_finish(self, ids, max_shrink: int = 10) -> None:
        _lib.dpo_group_solve_finish(self.handle, ids, len(ids),
                                    max_shrink, _stream(self._js_of))

    def counters(self) -> dict:
        """Which path the group's rounds took: batched / per-agent solve
        rounds and evaluations, batched continuations, graph captures of
        the batched sequences and descriptor builds."""
        buf = (ctypes.c_long * 7)()
        assert _lib.dpo_group_counters(self.handle, buf, 7) == 7
        keys = ("batched_solves", "batched_conts", "batched_evals",
                "agent_solves", "agent_evals", "captures", "desc_builds")
        return {k: int(v) for k, v in zip(keys, buf)}

    def eval_all(self, out: Tensor) -> None:
        """Evaluate every agent; out is a (num_robots, 3) fp64 device
        matrix — only this group's rows are written."""
        _lib.dpo_group_eval(self.handle, _p(out), out.stride(0),
                            _stream(self._js_of))


def gnc_weights(X: Tensor, nbr: Tensor, g: dict, weights: Tensor,
                d: int, r: int, mu: float, barc_sq: float) -> None:
    """Launch the GNC-TLS weight-update kernel over g['ne'] edges."""
    _check_shape(d, r)
    _lib.dpo_gnc_weights(
        _p(X), _p(nbr), _p(g["e1_idx"]), _p(g["e1_nbr"]), _p(g["e2_idx"]),
        _p(g["e2_nbr"]), _p(g["R"]), _p(g["t"]), _p(g["kappa"]),
        _p(g["tau"]), _p(g["upd"]), _p(g["widx"]), _p(weights),
        g["ne"], d, r, mu, barc_sq, _stream(X))


# ---------------------------------------------------------------------
# Optimality certificate (S = Q - Lambda(X), Lanczos with full
# reorthogonalisation) — interface mirrors cpu_ref.cert_*
# ---------------------------------------------------------------------
_lib.dpo_cert_lambda.argtypes = [_c, _c, _c, _c, _c, _i, _i, _i, _c]
_lib.dpo_cert_apply.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c, _c,
                                _i, _i, _c]
_lib.dpo_cert_lanczos.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c,
                                  _i, _i, _i, _i, _i, _c]
_lib.dpo_cert_ctrl_header.restype = _i
_lib.dpo_cert_max_part.restype = _i

from .cpu_ref import CERT_HDR, cert_check_shape  # noqa: E402

assert _lib.dpo_cert_ctrl_header() == CERT_HDR
_CERT_PART = _lib.dpo_cert_max_part()


def _chk_q(Q, like: Tensor):
    _chk(Q.vals)
    _chk(Q.row_ptr, torch.int32)
    _chk(Q.col_idx, torch.int32)
    assert Q.vals.device == like.device


def cert_lambda(Q, Xt: Tensor, d: int):
    """Lambda blocks (n, d, d) of the certificate operator at Xt and the
    1-element device tensor ||Q Xt - Lambda Xt||_F^2. No host sync."""
    _chk(Xt); _chk_q(Q, Xt)
    N, r = Xt.shape
    n = N // (d + 1)
    assert Q.n == n and Q.dh == d + 1 and N == n * (d + 1)
    cert_check_shape(d, r)
    QX = bsr_spmm(Q.row_ptr, Q.col_idx, Q.vals, n, d + 1, Xt)
    lam = torch.empty(n, d, d, dtype=torch.float64, device=Xt.device)
    res = torch.empty(1, dtype=torch.float64, device=Xt.device)
    part = torch.empty(_CERT_PART, dtype=torch.float64, device=Xt.device)
    _lib.dpo_cert_lambda(_p(Xt), _p(QX), _p(lam), _p(res), _p(part),
                         n, d, r, _stream(Xt))
    return lam, res


def cert_apply(Q, lam: Tensor, v: Tensor, v_prev: Optional[Tensor] = None,
               beta_prev: float = 0.0):
    """w = (Q - Lambda) v - beta_prev * v_prev and the 1-element device
    tensor alpha = <v, w> (one fused Lanczos operator application)."""
    _chk(lam); _chk(v); _chk_q(Q, v)
    n, d = lam.shape[0], lam.shape[1]
    cert_check_shape(d, None)
    assert Q.n == n and Q.dh == d + 1 and v.shape == (n * (d + 1),)
    dev = v.device
    beta = None
    if v_prev is not None:
        _chk(v_prev)
        assert v_prev.shape == v.shape
        beta = torch.tensor([beta_prev], dtype=torch.float64, device=dev)
    w = torch.empty_like(v)
    alpha = torch.empty(1, dtype=torch.float64, device=dev)
    part = torch.empty(_CERT_PART, dtype=torch.float64, device=dev)
    _lib.dpo_cert_apply(_p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals), _p(lam),
                        _p(v), _p(v_prev), _p(beta), _p(w), _p(alpha),
                        _p(part), n, d, _stream(v))
    return w, alpha


def cert_lanczos_steps(Q, lam: Tensor, V: Tensor, ctl: Tensor,
                       first_step: int, nsteps: int) -> None:
    """Enqueue Lanczos steps first_step .. first_step + nsteps - 1 with
    no host synchronisation. V: (m + 1, N) basis, row j = v_j; ctl: the
    (CERT_HDR + 2 m) control array (see cpu_ref.cert_lanczos_steps)."""
    _chk(lam); _chk(V); _chk(ctl); _chk_q(Q, V)
    n, d = lam.shape[0], lam.shape[1]
    cert_check_shape(d, None)
    m = V.shape[0] - 1
    N = V.shape[1]
    assert Q.n == n and Q.dh == d + 1 and N == n * (d + 1)
    assert ctl.numel() == CERT_HDR + 2 * m
    assert 0 <= first_step and nsteps >= 0 and first_step + nsteps <= m
    dev = V.device
    w = torch.empty(N, dtype=torch.float64, device=dev)
    cvec = torch.empty(m + 1, dtype=torch.float64, device=dev)
    part = torch.empty(_CERT_PART, dtype=torch.float64, device=dev)
    _lib.dpo_cert_lanczos(_p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals),
                          _p(lam), _p(V), _p(w), _p(cvec), _p(part),
                          _p(ctl), n, d, m, first_step, nsteps, _stream(V))


# ---- thick-restart window (interface mirrors cpu_ref) ----------------
_lib.dpo_cert_lanczos_split.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c,
                                        _c, _i, _i, _i, _i, _i, _c]
_lib.dpo_cert_gram_split.argtypes = [_c, _c, _c, _c, _c, _c, _c, _i, _l,
                                     _c]
_lib.dpo_cert_contract.argtypes = [_c, _c, _i, _i, _l, _c]
_lib.dpo_cert_keep_max.restype = _i

from .cpu_ref import CERT_KEEP_MAX, cert_partials  # noqa: E402

assert _lib.dpo_cert_keep_max() == CERT_KEEP_MAX

# Below this N the window path keeps k_cert_gram (one workgroup per
# column). Measured step time with 64 stored vectors, column / split in
# us (profiles/cert_gram_ab.json, docs/DESIGN.md §14): N = 864 30 / 82,
# 10 976 50 / 84, 42 592 133 / 89, 4e6 16 130 / 4 389. The split step is
# flat near 85 us up to N ~ 4e4 (few blocks, each with 8 serial block
# sums per column tile, and two more launches); the column step grows
# with N and crosses it near 2.5e4 by linear interpolation. N is fixed
# per problem, so the choice is too.
CERT_SPLIT_MIN_N = 24576


def cert_lanczos_window(Q, lam: Tensor, V: Tensor, ctl: Tensor,
                        first_step: int, nsteps: int,
                        gram: Optional[str] = None) -> None:
    """cert_lanczos_steps on the (b + 1, N) window basis of the restarted
    path. gram: "split" (row-split Gram), "column" (k_cert_gram), or
    None to choose by N (CERT_SPLIT_MIN_N)."""
    n, d = lam.shape[0], lam.shape[1]
    N = V.shape[1]
    if gram is None:
        gram = "split" if N >= CERT_SPLIT_MIN_N else "column"
    assert gram in ("split", "column")
    if gram == "column":
        return cert_lanczos_steps(Q, lam, V, ctl, first_step, nsteps)
    _chk(lam); _chk(V); _chk(ctl); _chk_q(Q, V)
    cert_check_shape(d, None)
    m = V.shape[0] - 1
    assert Q.n == n and Q.dh == d + 1 and N == n * (d + 1)
    assert ctl.numel() == CERT_HDR + 2 * m
    assert 0 <= first_step and nsteps >= 0 and first_step + nsteps <= m
    dev = V.device
    w = torch.empty(N, dtype=torch.float64, device=dev)
    cvec = torch.empty(m + 1, dtype=torch.float64, device=dev)
    part = torch.empty(_CERT_PART, dtype=torch.float64, device=dev)
    gpart = torch.empty((m + 1) * _CERT_PART, dtype=torch.float64,
                        device=dev)
    _lib.dpo_cert_lanczos_split(
        _p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals), _p(lam), _p(V), _p(w),
        _p(cvec), _p(part), _p(gpart), _p(ctl), n, d, m, first_step,
        nsteps, _stream(V))


def cert_gram_split(V: Tensor, w: Tensor, c: Tensor,
                    ctl: Optional[Tensor] = None,
                    alpha_part: Optional[Tensor] = None,
                    alpha: Optional[Tensor] = None) -> None:
    """c[:] = V[:len(c)] @ w by the row-split Gram kernels and, with
    `alpha`, alpha[0] = the fixed-order sum of the cert_partials(N)
    partials in alpha_part. A raised ctl flag leaves both untouched."""
    _chk(V); _chk(w); _chk(c)
    ncols, N = c.numel(), w.numel()
    assert V.dim() == 2 and V.shape[1] == N and 1 <= ncols <= V.shape[0]
    if ctl is not None:
        _chk(ctl)
        assert ctl.numel() >= CERT_HDR
    if alpha is not None:
        _chk(alpha); _chk(alpha_part)
        assert alpha.numel() == 1
        assert alpha_part.numel() >= cert_partials(N)
    gpart = torch.empty(ncols * _CERT_PART, dtype=torch.float64,
                        device=V.device)
    _lib.dpo_cert_gram_split(_p(V), _p(w), _p(c), _p(gpart), _p(ctl),
                             _p(alpha_part), _p(alpha), ncols, N,
                             _stream(V))


def cert_contract(V: Tensor, C: Tensor) -> None:
    """Thick-restart contraction of the (b + 1, N) device basis with the
    (b, k) Ritz coefficients C (host or device), in place:
    V[:k] = C^T @ V[:b], V[k] = V[b]. Rows past k keep stale data."""
    _chk(V)
    b, k = C.shape
    assert V.shape[0] == b + 1 and 1 <= k <= min(b, CERT_KEEP_MAX)
    Cp = torch.zeros(b, CERT_KEEP_MAX, dtype=torch.float64)
    Cp[:, :k] = C.detach().to("cpu", torch.float64)
    Cd = Cp.to(V.device)
    _lib.dpo_cert_contract(_p(V), _p(Cd), b, k, V.shape[1], _stream(V))


# ---------------------------------------------------------------------
# refine: device-resident global trust region (docs/DESIGN.md §17) —
# interface mirrors cpu_ref.refine_*
# ---------------------------------------------------------------------
_lib.dpo_refine_stage.argtypes = [_i, _c, _c, _c,
                                  ctypes.POINTER(ctypes.c_void_p), _c, _c,
                                  _c, _c, _i, _i, _i, _i, _c]
_lib.dpo_refine_ctrl_size.restype = _i

from .cpu_ref import (CERT_BLOCK, RF_SIZE, RefineWorkspace,  # noqa: E402,F401
                      refine_control)

assert _lib.dpo_refine_ctrl_size() == RF_SIZE
assert _CERT_PART == CERT_BLOCK


def _refine_stage(stage: int, Q, ws, ctl: Tensor, d: int, pre,
                  nsteps: int = 0) -> None:
    bufs = ws.bufs()
    X = bufs[0]
    N, r = X.shape
    n = N // (d + 1)
    cert_check_shape(d, r)
    _chk_q(Q, X); _chk(ctl); _chk(ws.part)
    assert Q.n == n and Q.dh == d + 1 and N == n * (d + 1)
    assert ctl.numel() == RF_SIZE and ws.part.numel() >= 2 * _CERT_PART
    for t in bufs:
        _chk(t)
        assert t.shape == X.shape and t.device == X.device
    L = Minv = None
    if pre is not None:
        mode, data = pre
        if mode == "jacobi":
            L = data
            _chk(L)
            assert L.shape == (n, d + 1, d + 1)
        elif mode == "dense":
            Minv = data
            _chk(Minv, torch.float32)
            assert Minv.shape == (N, N)
        else:
            raise ValueError(
                f"preconditioner mode {mode!r} has no HIP kernel: use "
                "'jacobi' or 'dense'")
    ptrs = (ctypes.c_void_p * len(bufs))(*[t.data_ptr() for t in bufs])
    _lib.dpo_refine_stage(stage, _p(Q.row_ptr), _p(Q.col_idx), _p(Q.vals),
                          ptrs, _p(L), _p(Minv), _p(ws.part), _p(ctl), n, d,
                          r, nsteps, _stream(X))


def refine_head(Q, ws, ctl: Tensor, d: int, pre) -> None:
    """cpu_ref.refine_head on the device; no host synchronisation."""
    assert pre is not None
    _refine_stage(0, Q, ws, ctl, d, pre)


def refine_tcg_steps(Q, ws, ctl: Tensor, d: int, pre, nsteps: int) -> None:
    """Enqueue nsteps tCG iterations; those past the stopping point are
    runs of guarded no-ops."""
    assert pre is not None and nsteps >= 0
    _refine_stage(1, Q, ws, ctl, d, pre, nsteps)


def refine_candidate(Q, ws, ctl: Tensor, d: int) -> None:
    _refine_stage(2, Q, ws, ctl, d, None)


def refine_hd_stage(Q, ws, ctl: Tensor, d: int) -> None:
    """Hd = P_X(Q delta) with the per-block partials of <delta, Hd> in
    ws.part[:cert_partials(n)] (status RS_RUN only)."""
    _refine_stage(3, Q, ws, ctl, d, None)


# ---------------------------------------------------------------------
# Rounding to SE(d) (docs/DESIGN.md §19) — interface mirrors
# cpu_ref.round_*. Nothing here synchronises with the host.
# ---------------------------------------------------------------------
_lib.dpo_round_gram.argtypes = [_c, _c, _c, _i, _i, _i, _c]
_lib.dpo_round_gram_part.restype = _i
_lib.dpo_round_poses.argtypes = [_c, _c, _c, _i, _c, _c, _i, _i, _i, _c]
_lib.dpo_round_reflections.argtypes = [_c, _c, _c, _c, _i, _i, _i, _c]
_lib.dpo_round_gauge.argtypes = [_c, _c, _c, _i, _i, _c]

_ROUND_GRAM_PART = _lib.dpo_round_gram_part()


def _round_dims(Xt: Tensor, d: int):
    _chk(Xt)
    assert Xt.dim() == 2 and Xt.shape[0] % (d + 1) == 0
    N, r = Xt.shape
    _check_shape(d, r)
    return N // (d + 1), r


def _round_basis(U: Tensor, like: Tensor, r: int, d: int) -> Tensor:
    U = U.to(device=like.device, dtype=torch.float64).contiguous()
    assert U.shape == (r, d)
    return U


def round_gram(Xt: Tensor, d: int) -> Tensor:
    """S = sum_i Y_i Y_i^T (r, r) over the rotation rows of every pose
    block, on Xt's device; bitwise run-to-run reproducible."""
    n, r = _round_dims(Xt, d)
    S = torch.empty(r, r, dtype=torch.float64, device=Xt.device)
    part = torch.empty(_ROUND_GRAM_PART, dtype=torch.float64,
                       device=Xt.device)
    _lib.dpo_round_gram(_p(Xt), _p(S), _p(part), n, d, r, _stream(Xt))
    return S


def round_poses(Xt: Tensor, d: int, U: Tensor, t0: Tensor,
                flip: bool = False):
    """R_i = argmax_{SO(d)} tr(R^T U^T Y_i), t_i = U^T p_i - t0, with U's
    last column negated under `flip`: the (d, n (d+1)) trajectory layout
    and the Xt layout (n (d+1), d)."""
    n, r = _round_dims(Xt, d)
    U = _round_basis(U, Xt, r, d)
    t0 = t0.to(device=Xt.device, dtype=torch.float64).contiguous()
    assert t0.shape == (d,)
    traj = torch.empty(d, n * (d + 1), dtype=torch.float64, device=Xt.device)
    Xr = torch.empty(n * (d + 1), d, dtype=torch.float64, device=Xt.device)
    _lib.dpo_round_poses(_p(Xt), _p(U), _p(t0), int(bool(flip)), _p(traj),
                         _p(Xr), n, d, r, _stream(Xt))
    return traj, Xr


def round_reflections(Xt: Tensor, d: int, U: Tensor) -> Tensor:
    """1-element int32 device tensor: poses with det(U^T Y_i) < 0."""
    n, r = _round_dims(Xt, d)
    U = _round_basis(U, Xt, r, d)
    count = torch.empty(1, dtype=torch.int32, device=Xt.device)
    ipart = torch.empty(_CERT_PART, dtype=torch.int32, device=Xt.device)
    _lib.dpo_round_reflections(_p(Xt), _p(U), _p(count), _p(ipart), n, d, r,
                               _stream(Xt))
    return count


def round_gauge(Xr: Tensor, traj: Tensor, d: int, anchor_pose: int) -> None:
    """In place on both layouts: R_i <- R_a^T R_i, t_i <- R_a^T (t_i -
    t_a) for a = anchor_pose, which is copied device to device first."""
    _chk(Xr); _chk(traj)
    dh = d + 1
    n = Xr.shape[0] // dh
    _check_shape(d, d)
    assert Xr.shape == (n * dh, d) and traj.shape == (d, n * dh)
    assert 0 <= anchor_pose < n
    anchor = Xr[anchor_pose * dh:(anchor_pose + 1) * dh].clone()
    _lib.dpo_round_gauge(_p(Xr), _p(traj), _p(anchor), n, d, _stream(Xr))


def round_cost(Q, X: Tensor, G: Optional[Tensor] = None) -> Tensor:
    """1-element device tensor f(X) = 0.5 <Q X, X> + <X, G> from the
    BSR SpMM and dot kernels."""
    _chk(X); _chk_q(Q, X)
    assert X.shape[0] == Q.N
    QX = bsr_spmm(Q.row_ptr, Q.col_idx, Q.vals, Q.n, Q.dh, X)
    acc = torch.zeros(CTRL_SIZE, dtype=torch.float64, device=X.device)
    dots(QX, X, None, acc, C_DOT0)
    if G is not None:
        dots(X, G.contiguous(), None, acc, C_DOT1)
    return (0.5 * acc[C_DOT0] + acc[C_DOT1]).reshape(1)


# ---------------------------------------------------------------------
# Certificate, LOBPCG (docs/DESIGN.md §20) — interface mirrors
# cpu_ref.cert_lob_*. Nothing here synchronises with the host.
# ---------------------------------------------------------------------
_lib.dpo_cert_lobpcg_ctrl_size.restype = _i
_lib.dpo_cert_lobpcg_part_size.restype = _i
_lib.dpo_cert_lobpcg_resid.argtypes = [_c, _c, _c, _c, _c, _c, _l, _i, _c]
_lib.dpo_cert_lobpcg_apply.argtypes = [_c, _c, _c, _c, _c, _c, _c, _i, _i,
                                       _i, _c]
_lib.dpo_cert_lobpcg_gram.argtypes = [_c, _c, _c, _c, _c, _l, _i, _c]
_lib.dpo_cert_lobpcg_update.argtypes = [_c, _c, _c, _l, _i, _c]
_lib.dpo_cert_lobpcg_iter.argtypes = [_c, _c, _c, _c, _c, _c, _c, _c, _c,
                                      _c, _c, _c, _i, _i, _i, _c]

from .cpu_ref import (LOB_GPART, LOB_RPART, LOB_SIZE, LOB_W,  # noqa: E402
                      LobWorkspace)

assert _lib.dpo_cert_lobpcg_ctrl_size() == LOB_SIZE
assert _lib.dpo_cert_lobpcg_part_size() == LOB_GPART + LOB_RPART


def _chk_lob(ws, d: Optional[int] = None) -> None:
    N, m = ws.N, ws.m
    _check_shape(d, m)
    for t in (ws.B, ws.SB, ws.R, ws.ctl, ws.part, ws.out):
        _chk(t)
        assert t.device == ws.B.device
    assert ws.B.shape == (3, N, m) and ws.SB.shape == (3, N, m)
    assert ws.R.shape == (N, m) and ws.ctl.numel() == LOB_SIZE
    assert ws.part.numel() == LOB_GPART + LOB_RPART
    assert ws.out.numel() == 18 * m * m + m


def _lob_pre(ws, pre, d: int):
    """(L, Minv) pointers' tensors of a (mode, data) preconditioner."""
    mode, data = pre
    n = ws.N // (d + 1)
    if mode == "jacobi":
        _chk(data)
        assert data.shape == (n, d + 1, d + 1)
        return data, None
    if mode == "dense":
        _chk(data, torch.float32)
        assert data.shape == (ws.N, ws.N)
        return None, data
    raise ValueError(f"preconditioner mode {mode!r} has no HIP kernel: use "
                     "'jacobi' or 'dense'")


def cert_lob_resid(ws, zero: bool = False) -> None:
    """R = SX - X diag(theta), per-block partials of the squared column
    norms in ws.part's residual slots; `zero` clears W."""
    _chk_lob(ws)
    _lib.dpo_cert_lobpcg_resid(_p(ws.ctl), _p(ws.B[0]), _p(ws.SB[0]),
                               _p(ws.R), _p(ws.B[LOB_W]) if zero else None,
                               _p(ws.part), ws.N, ws.m, _stream(ws.B))


def cert_lob_precond(ws, pre, d: int) -> None:
    """W = T R with the guarded solve kernels (stand-alone: the dense
    apply clears W by a launch of its own; cert_lob_iter does not)."""
    _chk_lob(ws, d)
    L, Minv = _lob_pre(ws, pre, d)
    if Minv is not None:
        precond_dense(Minv, ws.R, ws.B[LOB_W], ws.ctl, 0)
    else:
        precond_jacobi(L, ws.R, d + 1, ws.B[LOB_W], ws.ctl, 0)


def cert_lob_apply(Q, lam: Tensor, ws, blk: int) -> None:
    """SB[blk] = (Q - Lambda) B[blk]."""
    n, d = lam.shape[0], lam.shape[1]
    _chk_lob(ws, d); _chk(lam); _chk_q(Q, ws.B)
    assert Q.n == n and Q.dh == d + 1 and ws.N == n * (d + 1)
    assert 0 <= blk < 3
    _lib.dpo_cert_lobpcg_apply(_p(ws.ctl), _p(Q.row_ptr), _p(Q.col_idx),
                               _p(Q.vals), _p(lam), _p(ws.B[blk]),
                               _p(ws.SB[blk]), n, d, ws.m, _stream(ws.B))


def cert_lob_gram(ws) -> None:
    """ws.out = [G_B, G_A (upper block triangles), squared residual
    norms]; bitwise run-to-run reproducible."""
    _chk_lob(ws)
    _lib.dpo_cert_lobpcg_gram(_p(ws.ctl), _p(ws.B), _p(ws.SB), _p(ws.part),
                              _p(ws.out), ws.N, ws.m, _stream(ws.B))


def cert_lob_update(ws) -> None:
    """X, P, SX, SP from the coefficients in ws.ctl, in place."""
    _chk_lob(ws)
    _lib.dpo_cert_lobpcg_update(_p(ws.ctl), _p(ws.B), _p(ws.SB), ws.N, ws.m,
                                _stream(ws.B))


def cert_lob_iter(Q, lam: Tensor, ws, pre) -> None:
    """Residual, W = T R, SW = S W and both Gram matrices, enqueued with
    no host synchronisation."""
    n, d = lam.shape[0], lam.shape[1]
    _chk_lob(ws, d); _chk(lam); _chk_q(Q, ws.B)
    assert Q.n == n and Q.dh == d + 1 and ws.N == n * (d + 1)
    L, Minv = _lob_pre(ws, pre, d)
    _lib.dpo_cert_lobpcg_iter(_p(ws.ctl), _p(Q.row_ptr), _p(Q.col_idx),
                              _p(Q.vals), _p(lam), _p(ws.B), _p(ws.SB),
                              _p(ws.R), _p(L), _p(Minv), _p(ws.part),
                              _p(ws.out), n, d, ws.m, _stream(ws.B))
