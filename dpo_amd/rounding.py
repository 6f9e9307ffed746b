"""Rounding of a lifted iterate to an SE(d) trajectory, on the iterate's
device, with the cost of the result and the suboptimality gap
(docs/DESIGN.md §19).

The lifted iterate Xt (n (d+1), r) holds, per pose, a d-frame Y_i in R^r
and a translation p_i in R^r. Rounding picks an r x d basis U, projects
every U^T Y_i onto SO(d) and maps the translations with U^T:

  mode="svd"     U = the top-d eigenvectors of S = sum_i Y_i Y_i^T
                 (SE-Sync's rounding; equal to the top left singular
                 vectors of the rotation columns). When more than half of
                 the blocks U^T Y_i have a negative determinant the lifted
                 solution sits in the reflected component and U's last
                 column is negated. The result is expressed in the frame
                 of pose `anchor_pose`.
  mode="anchor"  U = Y_a, t0 = Y_a^T p_a from a given (r, d+1) anchor pose:
                 what `PGOAgent._round_trajectory` computes (the
                 reference's first-pose rounding). No gauge step.

On a GPU tensor the Gram matrix, the per-pose projection, the reflection
count and the gauge change are HIP kernels and nothing loops over poses
on the host. The host reads back the r x r Gram matrix (its
eigendecomposition is at most 8 x 8), the reflection count and the final
scalars: three synchronisations for any n.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .ops.cpu_ref import cert_check_shape

Tensor = torch.Tensor


@dataclass
class RoundingResult:
    """Outcome of `round_solution`.

    `gap = f_rounded - f_relaxed` bounds `f_rounded - f*`, the distance of
    the rounded trajectory's cost from the global optimum f* of the
    pose-graph problem, ONLY when the relaxed iterate is the global
    minimiser of the rank-r relaxation: then f_relaxed <= f* <= f_rounded.
    That is the case when `certify_solution` returned CERTIFIED for the
    iterate, and the README's caveat applies unchanged: CERTIFIED is a
    numerical verdict, not an interval-arithmetic proof. For any other
    iterate `gap` is just the cost the rounding added and may be
    negative.

    Both costs follow `QuadraticProblem.f`: f(X) = 0.5 <Q X, X> + <X, G>.
    """
    Xt_rounded: Tensor      # (n (d+1), d), on the input's device
    trajectory_dev: Tensor  # (d, n (d+1)), on the input's device
    f_rounded: float
    f_relaxed: float
    gap: float
    relative_gap: float     # gap / max(|f_rounded|, |f_relaxed|), 0 if both 0
    reflected: int          # blocks with det(U^T Y_i) < 0 before any flip
    flipped: bool           # U's last column was negated
    spectrum: np.ndarray    # the r eigenvalues of S / n, descending
    rank_energy: float      # share of `spectrum` outside the top d
    mode: str

    def trajectory(self) -> np.ndarray:
        """(d, n (d+1)) numpy array, the layout of
        `PGOAgent.get_trajectory_in_global_frame`."""
        return np.ascontiguousarray(self.trajectory_dev.cpu().numpy())

    def as_dict(self) -> dict:
        """JSON-safe summary (no trajectory)."""
        return {"rounded_cost": self.f_rounded,
                "relaxation_cost": self.f_relaxed,
                "suboptimality_gap": self.gap,
                "relative_gap": self.relative_gap,
                "rounding_reflected": self.reflected,
                "rounding_flipped": self.flipped,
                "rank_energy": self.rank_energy}


def round_anchor(Xt: Tensor, d: int, anchor):
    """First-pose rounding against an (r, d+1) anchor (numpy or tensor):
    (trajectory (d, n (d+1)), Xt_rounded (n (d+1), d)) on Xt's device.
    Xt stays where it is; the anchor's r (d+1) numbers are all that
    cross to the device."""
    Xt = Xt.detach().to(torch.float64).contiguous()
    r = Xt.shape[1]
    cert_check_shape(d, r)
    A = torch.as_tensor(np.asarray(anchor) if not isinstance(anchor, Tensor)
                        else anchor, dtype=torch.float64).cpu()
    assert A.shape == (r, d + 1)
    U = A[:, :d].contiguous()
    t0 = U.T @ A[:, d]
    return ops.backend_for(Xt).round_poses(Xt, d, U, t0, False)


def gram_spectrum(Xt: Tensor, d: int):
    """(U (r, d), spectrum (r,)): the top-d eigenvectors of S = sum_i Y_i
    Y_i^T and the eigenvalues of S / n in descending order. One host
    read of the r x r matrix.

    At a rank-d solution the top d eigenvalues coincide, so eigh returns
    an arbitrary orthonormal basis of the dominant subspace, reflections
    included, and the last bits of S decide which. The basis is therefore
    re-derived from the subspace alone: Gram-Schmidt (QR with a positive
    diagonal) of the projections of e_1 .. e_d onto it. For r = d this
    is the identity, so a pose counts as reflected exactly when det Y_i <
    0. If those projections are numerically dependent (below 1e-8) the
    eigh basis is kept."""
    n = Xt.shape[0] // (d + 1)
    S = ops.backend_for(Xt).round_gram(Xt, d).cpu()
    w, V = torch.linalg.eigh(S)
    w, V = w.flip(0), V.flip(1)
    U = V[:, :d]
    Qm, Rm = torch.linalg.qr((U @ U.T)[:, :d])
    diag = torch.diagonal(Rm)
    if float(diag.abs().min()) > 1e-8:
        U = Qm * torch.sign(diag)
    return U.contiguous(), (w / n).numpy()


def round_solution(Q, Xt: Tensor, d: int, *, mode: str = "svd",
                   anchor=None, anchor_pose: int = 0,
                   G: Optional[Tensor] = None) -> RoundingResult:
    """Round the lifted iterate Xt (n (d+1), r) of the problem with data
    matrix Q (a `BSRMatrix` on Xt's device) to SE(d).

    mode         "svd" or "anchor" (module docstring).
    anchor       (r, d+1) lifted anchor pose, required by mode="anchor".
    anchor_pose  mode="svd": the pose whose frame the result is in.
    G            optional linear term (n (d+1), r) of f (an agent's
                 coupling to fixed neighbours), mode="svd" only: the
                 rounded cost then uses G U and both costs are taken
                 before the gauge step, which <X, G> is not invariant
                 under.
    Raises ValueError for a (d, r) outside the compiled shapes. See
    `RoundingResult` for what `gap` does and does not bound."""
    assert Xt.dim() == 2 and Xt.shape[0] % (d + 1) == 0
    Xt = Xt.detach().to(torch.float64).contiguous()
    n, r = Xt.shape[0] // (d + 1), Xt.shape[1]
    cert_check_shape(d, r)
    assert Q.N == Xt.shape[0]
    be = ops.backend_for(Xt)
    f_relaxed = be.round_cost(Q, Xt, G)
    U, spectrum = gram_spectrum(Xt, d)                      # host read 1
    if mode == "svd":
        if not 0 <= anchor_pose < n:
            raise ValueError(f"anchor_pose {anchor_pose} outside 0..{n - 1}")
        reflected = int(be.round_reflections(Xt, d, U))     # host read 2
        flipped = 2 * reflected > n
        traj, Xr = be.round_poses(Xt, d, U, torch.zeros(d, dtype=Xt.dtype),
                                  flipped)
        f_rounded = None
        if G is not None:
            Ud = U.clone()
            if flipped:
                Ud[:, -1] *= -1.0
            f_rounded = be.round_cost(Q, Xr, (G @ Ud.to(G.device)))
        be.round_gauge(Xr, traj, d, anchor_pose)
        if f_rounded is None:
            f_rounded = be.round_cost(Q, Xr)
    elif mode == "anchor":
        if anchor is None:
            raise ValueError('mode="anchor" needs the (r, d+1) anchor pose')
        if G is not None:
            raise ValueError('G is supported by mode="svd" only')
        traj, Xr = round_anchor(Xt, d, anchor)
        Ua = torch.as_tensor(np.asarray(anchor.cpu() if isinstance(
            anchor, Tensor) else anchor), dtype=torch.float64)[:, :d]
        reflected = int(be.round_reflections(Xt, d, Ua.contiguous()))
        flipped = False
        f_rounded = be.round_cost(Q, Xr)
    else:
        raise ValueError(f"unknown rounding mode {mode!r}")
    f_rounded, f_relaxed = torch.cat([f_rounded, f_relaxed]).tolist()  # 3
    gap = f_rounded - f_relaxed
    scale = max(abs(f_rounded), abs(f_relaxed))
    total = float(spectrum.sum())
    return RoundingResult(
        Xr, traj, f_rounded, f_relaxed, gap,
        gap / scale if scale > 0.0 else 0.0, reflected, flipped, spectrum,
        float(spectrum[d:].sum()) / total if total > 0.0 else 0.0, mode)
