"""Reference, input builders and tolerances of the rounding tests
(tests/test_rounding.py, tests/test_rounding_gpu.py). NumPy on the CPU,
written out independently of dpo_amd.rounding.

Tolerances (docs/DESIGN.md §19):
  * sums of K products use kernel_refs.sop_bound / matmul_bound;
  * the invariants of a projected block (orthogonality 64 eps, det > 0,
    objective within 64 eps ||B||_F sqrt(d) of the reference's) need no
    condition number;
  * the distance of a rounded rotation from the reference's is compared
    with  c eps ||B||_F / (sigma_{d-1} + s sigma_d),  s = sign det B: the
    polar-factor perturbation bound. c is 8 x the largest discrepancy,
    normalised the same way, between two fp64 SVD projections on the CPU
    (NumPy's and torch's) over the blocks of the test itself
    (`measured_c`); it is never derived from the code under test. Blocks
    with (sigma_{d-1} + s sigma_d) / sigma_1 < 1e-6 are exempt from this
    check alone.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from dpo_amd.liegroups import project_to_rotation_group

EPS = float(np.finfo(np.float64).eps)
C_MARGIN = 8.0
EXEMPT_BELOW = 1e-6
ADVERSARIAL = ("neg", "cI", "rot", "tiny", "huge", "rank", "zero")
EXEMPT_KINDS = ("rank", "zero")


# ---------------------------------------------------------------------
# the reference rounding: np.linalg.eigh for the basis, a plain loop
# ---------------------------------------------------------------------
def round_ref(Xt, d, anchor_pose=0):
    """SE-Sync rounding of Xt (n (d+1), r): (T (d, n (d+1)) in the frame
    of pose anchor_pose, reflected, flipped, spectrum of S / n, the blocks
    U^T Y_i before the flip)."""
    X = np.asarray(Xt, dtype=np.float64)
    dh, r = d + 1, X.shape[1]
    Xb = X.reshape(-1, dh, r)
    n = Xb.shape[0]
    Yt = Xb[:, :d, :].reshape(n * d, r)
    w, V = np.linalg.eigh(Yt.T @ Yt)
    U = V[:, ::-1][:, :d]
    # orientation from the subspace alone (eigh's is arbitrary when the
    # top d eigenvalues coincide): Gram-Schmidt of P e_1 .. P e_d
    Qm, Rm = np.linalg.qr((U @ U.T)[:, :d])
    if np.abs(np.diag(Rm)).min() > 1e-8:
        U = Qm * np.sign(np.diag(Rm))
    B = np.stack([U.T @ Xb[i, :d, :].T for i in range(n)])
    reflected = int(sum(np.linalg.slogdet(B[i])[0] < 0 for i in range(n)))
    flipped = 2 * reflected > n
    if flipped:
        U = U.copy()
        U[:, -1] *= -1.0
    R = [project_to_rotation_group(U.T @ Xb[i, :d, :].T) for i in range(n)]
    t = [U.T @ Xb[i, d, :] for i in range(n)]
    T = np.zeros((d, n * dh))
    for i in range(n):
        T[:, i * dh:i * dh + d] = R[anchor_pose].T @ R[i]
        T[:, i * dh + d] = R[anchor_pose].T @ (t[i] - t[anchor_pose])
    return T, reflected, flipped, w[::-1] / n, B


def project_ref(B):
    """Per-block SO(d) projection, NumPy SVD (n, d, d)."""
    return np.stack([project_to_rotation_group(b) for b in B])


def project_ref_torch(B):
    """The second reference: torch.linalg.svd with the determinant fix."""
    Bt = torch.from_numpy(np.ascontiguousarray(B))
    U, _, Vh = torch.linalg.svd(Bt)
    neg = torch.linalg.det(U) * torch.linalg.det(Vh) < 0
    U = U.clone()
    U[neg, :, -1] *= -1.0
    return torch.bmm(U, Vh).numpy()


# ---------------------------------------------------------------------
# conditioning of a block and the distance bound
# ---------------------------------------------------------------------
def block_stats(B):
    """(||B||_F, gap = sigma_{d-1} + s sigma_d, exempt mask), computed on
    max-normalised blocks so that 1e+-150 scales neither overflow nor
    underflow."""
    B = np.asarray(B, dtype=np.float64)
    m = np.abs(B).max(axis=(1, 2))
    safe = np.where(m > 0, m, 1.0)
    Bn = B / safe[:, None, None]
    s = np.linalg.svd(Bn, compute_uv=False)
    sg = np.sign(np.linalg.slogdet(Bn)[0])
    gap = s[:, -2] + sg * s[:, -1]
    exempt = (m == 0) | (gap < EXEMPT_BELOW * np.maximum(s[:, 0], 1e-300))
    return np.linalg.norm(Bn, axis=(1, 2)) * m, gap * m, exempt


def normalised_distance(Ra, Rb, B):
    """||Ra - Rb||_F (sigma_{d-1} + s sigma_d) / (eps ||B||_F) per block,
    0 on exempt blocks."""
    nb, gap, exempt = block_stats(B)
    dist = np.linalg.norm(Ra - Rb, axis=(1, 2))
    with np.errstate(all="ignore"):
        ratio = np.where(exempt, 1.0, gap / np.where(nb > 0, nb, 1.0))
    return np.where(exempt, 0.0, dist * ratio / EPS)


def distance_bound(B, c, dB=0.0):
    """Per-block bound on ||R - R_ref||_F: (c eps ||B||_F + 2 dB) / gap,
    dB a bound on the Frobenius error already in the block the code under
    test projects (2 / gap is the polar factor's Lipschitz constant).
    inf on exempt blocks."""
    nb, gap, exempt = block_stats(B)
    with np.errstate(all="ignore"):
        out = (c * EPS * nb + 2.0 * dB) / np.where(exempt, 1.0, gap)
    return np.where(exempt, np.inf, out)


# ---------------------------------------------------------------------
# blocks: rotation + 0.3 randn, a fixed share adversarial
# ---------------------------------------------------------------------
def _rotations(n, d, rng):
    Q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def make_blocks(n, d, seed, kinds=ADVERSARIAL):
    """(B (n, d, d), kind (n,) of str): block i is adversarial when
    i % 4 == 3, cycling through `kinds`; every other block is a rotation
    plus 0.3 randn ("random")."""
    rng = np.random.default_rng(1000 * d + seed)
    B = _rotations(n, d, rng) + 0.3 * rng.standard_normal((n, d, d))
    kind = np.array(["random"] * n, dtype=object)
    for i in range(3, n, 4):
        k = kinds[(i // 4) % len(kinds)]
        kind[i] = k
        if k == "neg":
            B[i][:, 0] *= -1.0 if np.linalg.det(B[i]) > 0 else 1.0
        elif k == "cI":
            B[i] = 2.5 * np.eye(d)
        elif k == "rot":
            B[i] = _rotations(1, d, rng)[0]
        elif k == "tiny":
            B[i] *= 1e-150
        elif k == "huge":
            B[i] *= 1e150
        elif k == "rank":
            U, s, Vt = np.linalg.svd(B[i])
            s[-1] = 0.0
            B[i] = (U * s) @ Vt
        elif k == "zero":
            B[i] = 0.0
    return B, kind


def signed_permutation_basis(d, r, seed):
    """(r, d) basis with one +-1 per column in distinct rows: U^T Y is
    then exact in floating point, so the block the kernel projects is the
    block the test built."""
    rng = np.random.default_rng(77 + 10 * r + d + seed)
    rows = rng.permutation(r)[:d]
    U = np.zeros((r, d))
    U[rows, np.arange(d)] = rng.choice([-1.0, 1.0], size=d)
    return U


def stiefel_basis(d, r, seed):
    rng = np.random.default_rng(99 + 10 * r + d + seed)
    return np.linalg.qr(rng.standard_normal((r, d)))[0]


def lift_blocks(B, U, seed):
    """Xt (n (d+1), r) with Y_i = U B_i (so U^T Y_i = B_i for an
    orthonormal U) and Gaussian lifted translations."""
    n, d, _ = B.shape
    r = U.shape[0]
    rng = np.random.default_rng(5 + seed)
    Xb = np.empty((n, d + 1, r))
    Xb[:, :d, :] = np.einsum("kc,nca->nak", U, B)
    Xb[:, d, :] = rng.standard_normal((n, r))
    return Xb.reshape(n * (d + 1), r)


def pose_counts(d, r):
    """1; one fewer than, exactly and one more than the poses of one
    256-thread block; three Gram partial blocks plus one pose. Every
    rounding kernel is thread-per-pose, so a block covers 256 poses for
    every (d, r)."""
    return (1, 255, 256, 257, 2 * 256 + 1)


@functools.lru_cache(maxsize=None)
def measured_c(d):
    """C_MARGIN x the largest normalised discrepancy between the NumPy
    and the torch SVD projection over every block of the projection test
    for this d (all pose counts)."""
    worst = 0.0
    for n in pose_counts(d, d):
        B, _ = make_blocks(n, d, n)
        worst = max(worst, float(normalised_distance(
            project_ref(B), project_ref_torch(B), B).max()))
    return C_MARGIN * worst, worst


# ---------------------------------------------------------------------
# ground-truth trajectories for the exact-recovery tests
# ---------------------------------------------------------------------
def ground_truth(n, d, seed=0):
    """Random SE(d) trajectory with pose 0 the identity: T (d, n (d+1))."""
    rng = np.random.default_rng(seed)
    R = _rotations(n, d, rng)
    t = rng.standard_normal((n, d)) * 3.0
    R[0], t[0] = np.eye(d), 0.0
    T = np.zeros((d, n * (d + 1)))
    for i in range(n):
        T[:, i * (d + 1):i * (d + 1) + d] = R[i]
        T[:, i * (d + 1) + d] = t[i]
    return T


def pipeline_tol(n, d, r, B, c, tmax):
    """(rot_tol, trans_tol) for a whole svd-mode rounding against another
    fp64 evaluation of it, from the blocks B = U^T Y_i of the reference.
      sub   2 n d eps / relgap: the dominant subspace of S, whose entries
            are sums of n d products and whose gap to the rest of the
            spectrum is relgap = 1 for the rank-d iterates used here;
      dB    the error that and the r-term products leave in a block;
      proj  the projection bound with that dB (worst block);
    the gauge multiplies two projected rotations (2 proj + d-term
    products); translations of size <= tmax see sub, the r- and d-term
    products and the anchor rotation's error."""
    sub = 2.0 * n * d * EPS
    dB = (sub + 2.0 * r * EPS) * np.sqrt(d)
    proj = float(distance_bound(B, c, dB).max())
    rot = 2.0 * proj + 2.0 * d * EPS * np.sqrt(d)
    trans = 2.0 * tmax * (sub + 2.0 * (r + d) * EPS + proj)
    return rot, trans
