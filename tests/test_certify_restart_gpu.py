"""GPU tests of the thick-restart certificate path: k_cert_contract and
the row-split Gram against the fp64 CPU reference, and
certify_solution(basis_size=b) on GPU tensors against the CPU run. Cases
are shared with test_certify.py."""
import numpy as np
import pytest
import torch

from test_certify import grid_case, grid_reference, ring_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
# 1 thread; a partly filled, a full and a just-overfull block; and one
# row past 256 blocks x 256 threads, so one thread takes a second
# grid-stride trip
SIZES = [1, 255, 256, 257, 65537]


def _backends():
    from dpo_amd import ops
    assert ops.hip_available(), "HIP extension must load on a GPU box"
    from dpo_amd.ops import cpu_ref, hip_backend
    return cpu_ref, hip_backend


def _randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.float64, generator=g)


# --------------------------------------------------------------------
# 1. k_cert_contract, in place, against the out-of-place CPU product
# --------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("k", [1, 3, 6])
def test_cert_contract_matches_cpu(N, k):
    cpu_ref, hip = _backends()
    b = 8
    assert k <= min(cpu_ref.CERT_KEEP_MAX, b - 2)
    V = _randn(b + 1, N, seed=N + k)
    C = _randn(b, k, seed=7 * k)
    ref = V.clone()
    cpu_ref.cert_contract(ref, C)
    Vd = V.to(DEV)
    hip.cert_contract(Vd, C)
    out = Vd.cpu()
    # sum of b products per entry: |gpu - ref| <= 2 b eps sum |C||V|
    bound = 2 * b * EPS * (C.abs().T @ V[:b].abs())
    err = (out[:k] - ref[:k]).abs()
    print(f"contract N={N} k={k}: max err {float(err.max())!r}, "
          f"min slack {float((bound - err).min())!r}")
    assert bool((err <= bound).all())
    assert torch.equal(out[k], V[b])       # the carried vector, exactly
    # rows past k may hold anything; the CPU reference got the same V[k]
    assert torch.equal(ref[k], V[b])


def test_cert_contract_widest_column_count():
    """k at the compile-time bound, in a window wide enough to hold it."""
    cpu_ref, hip = _backends()
    k = cpu_ref.CERT_KEEP_MAX
    b, N = k + 2, 257
    V = _randn(b + 1, N, seed=3)
    C = _randn(b, k, seed=4)
    ref = V.clone()
    cpu_ref.cert_contract(ref, C)
    Vd = V.to(DEV)
    hip.cert_contract(Vd, C)
    out = Vd.cpu()
    bound = 2 * b * EPS * (C.abs().T @ V[:b].abs())
    assert bool(((out[:k] - ref[:k]).abs() <= bound).all())
    assert torch.equal(out[k], V[b])


# --------------------------------------------------------------------
# 2. row-split Gram
# --------------------------------------------------------------------
def _gram_case(N, ncols):
    from dpo_amd.ops.cpu_ref import cert_partials
    V = _randn(ncols, N, seed=N + ncols)
    w = _randn(N, seed=N)
    # alpha partials as k_cert_apply leaves them: block partials of
    # <V[ncols - 1], w>
    npart = cert_partials(N)
    prod = V[ncols - 1] * w
    part = torch.stack([c.sum() for c in torch.chunk(prod, npart)])
    assert part.numel() == npart
    return V, w, part


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("ncols", [1, 2, 9])
def test_gram_split_matches_cpu(N, ncols):
    cpu_ref, hip = _backends()
    V, w, part = _gram_case(N, ncols)
    c_ref = torch.empty(ncols, dtype=torch.float64)
    a_ref = torch.empty(1, dtype=torch.float64)
    cpu_ref.cert_gram_split(V, w, c_ref, None, part, a_ref)
    Vd, wd, pd = V.to(DEV), w.to(DEV), part.to(DEV)
    runs = []
    for _ in range(2):
        c = torch.full((ncols,), -7.0, dtype=torch.float64, device=DEV)
        a = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
        hip.cert_gram_split(Vd, wd, c, None, pd, a)
        runs.append((c.cpu(), a.cpu()))
    (c, a), (c2, a2) = runs
    # a sum of N products, any order: 2 N eps sum |V||w|
    bound = 2 * N * EPS * (V.abs() @ w.abs())
    err = (c - c_ref).abs()
    print(f"gram N={N} ncols={ncols}: max err {float(err.max())!r} "
          f"min bound {float(bound.min())!r}; alpha err "
          f"{float((a - a_ref).abs()[0])!r}")
    assert bool((err <= bound).all())
    assert float((a - a_ref).abs()[0]) <= float(bound[ncols - 1])
    assert torch.equal(c, c2) and torch.equal(a, a2)    # §8: bit-identical
    # without alpha: c alone, same bits
    c3 = torch.empty(ncols, dtype=torch.float64, device=DEV)
    hip.cert_gram_split(Vd, wd, c3)
    assert torch.equal(c3.cpu(), c)


@pytest.mark.parametrize("N", [257, 65537])
def test_gram_split_guard(N):
    """Breakdown flag raised beforehand: sentinel outputs untouched."""
    cpu_ref, hip = _backends()
    from dpo_amd.ops.cpu_ref import CERT_FLAG, CERT_HDR
    ncols = 9
    V, w, part = _gram_case(N, ncols)
    ctl = torch.zeros(CERT_HDR, dtype=torch.float64)
    ctl[CERT_FLAG] = 1.0
    sent = torch.full((ncols + 1,), 12345.678, dtype=torch.float64)
    for be, dev in ((cpu_ref, "cpu"), (hip, DEV)):
        c, a = sent[:ncols].to(dev), sent[ncols:].to(dev)
        ctl_d = ctl.to(dev)
        be.cert_gram_split(V.to(dev), w.to(dev), c, ctl_d, part.to(dev), a)
        assert torch.equal(c.cpu(), sent[:ncols])
        assert torch.equal(a.cpu(), sent[ncols:])
        assert torch.equal(ctl_d.cpu(), ctl)


# --------------------------------------------------------------------
# 3. certify_solution(basis_size=b) on GPU tensors
# --------------------------------------------------------------------
def _certify_case(name):
    if name == "grid":
        meas, n, Q, _, X = grid_case()
        return meas, n, 3, X, grid_reference()[-1], dict(
            basis_size=12, keep=(4, 2), max_iters=1000)
    meas, n, Q, X, _ = ring_case(67)
    return meas, n, 2, X, 4.0, dict(basis_size=16, keep=(6, 2),
                                    max_iters=1000)


@pytest.mark.parametrize("name", ["ring67", "grid"])
def test_certify_restarted_gpu_matches_cpu(name):
    _backends()
    from dpo_amd.certify import certify_solution
    meas, n, d, X, lmax, kw = _certify_case(name)
    ref = certify_solution(meas, n, d, X, **kw)
    a = certify_solution(meas, n, d, X.to(DEV), **kw)
    b = certify_solution(meas, n, d, X.to(DEV), **kw)
    print(f"{name}: cpu {ref.status} {ref.lambda_min!r} res {ref.residual!r} "
          f"it {ref.iterations} rs {ref.restarts}; gpu {a.status} "
          f"{a.lambda_min!r} res {a.residual!r} it {a.iterations} "
          f"rs {a.restarts}")
    assert a.status == ref.status
    assert abs(a.lambda_min - ref.lambda_min) <= (
        a.residual + ref.residual + 1e-8 * lmax)
    assert a.restarts >= 1
    assert a.direction.device.type == "cuda"
    assert abs(float(torch.linalg.norm(a.direction)) - 1.0) <= 1e-12
    assert (a.lambda_min, a.residual, a.iterations, a.restarts) == (
        b.lambda_min, b.residual, b.iterations, b.restarts)


@pytest.mark.parametrize("gram", ["split", "column"])
def test_window_steps_match_cpu_with_either_gram(gram):
    """The window op with each Gram kernel, across one restart, against
    the CPU window: alpha and beta to 1e-10 lambda_max as in the
    unrestarted step test."""
    cpu_ref, hip = _backends()
    from dpo_amd.certify import _thick_restart, certificate_operator
    from dpo_amd.ops.cpu_ref import CERT_COUNT, CERT_FLAG, CERT_HDR, CERT_TOL
    meas, n, Q, X, _ = ring_case(67)
    lam, _ = certificate_operator(Q, X)
    N, b, keep = Q.N, 16, (6, 2)
    k = sum(keep)
    Vc = torch.zeros(b + 1, N, dtype=torch.float64)
    Vc[0] = _randn(N, seed=5)
    Vc[0] /= torch.linalg.norm(Vc[0])
    cc = torch.zeros(CERT_HDR + 2 * b, dtype=torch.float64)
    cc[CERT_TOL] = 1e-10
    Qd, lamd, Vg, cg = Q.to(DEV), lam.to(DEV), Vc.to(DEV), cc.to(DEV)
    cpu_ref.cert_lanczos_window(Q, lam, Vc, cc, 0, b)
    hip.cert_lanczos_window(Qd, lamd, Vg, cg, 0, b, gram=gram)
    h = cc.numpy()
    alpha, beta = h[CERT_HDR:CERT_HDR + b], h[CERT_HDR + b:]
    T = np.diag(alpha) + np.diag(beta[:b - 1], 1) + np.diag(beta[:b - 1], -1)
    C, _ = _thick_restart(T, beta[b - 1], keep)
    C = torch.from_numpy(C)
    assert float((cg.cpu() - cc).abs().max()) <= 1e-10 * 4.0
    cpu_ref.cert_contract(Vc, C)
    hip.cert_contract(Vg, C)
    for ctl in (cc, cg):
        ctl[CERT_COUNT] = k
        ctl[CERT_HDR + b + k - 1] = 0.0
    cpu_ref.cert_lanczos_window(Q, lam, Vc, cc, k, 3)
    hip.cert_lanczos_window(Qd, lamd, Vg, cg, k, 3, gram=gram)
    g = cg.cpu()
    assert g[CERT_FLAG] == 0 and g[CERT_COUNT] == k + 3
    assert float((g - cc).abs().max()) <= 1e-10 * 4.0
    B = Vg[:k + 4].cpu()
    assert float((B @ B.T - torch.eye(k + 4, dtype=torch.float64))
                 .abs().max()) <= 1e-12


# --------------------------------------------------------------------
# 4. the allocation really is (b + 1) N
# --------------------------------------------------------------------
def test_restarted_gpu_run_inside_small_budget():
    _backends()
    from dpo_amd.certify import (BasisBudgetError, CertificateStatus,
                                 certify_solution)
    meas, n, Q, X, _ = ring_case(67)
    kw = dict(basis_budget_bytes=64 << 10, max_iters=1000)
    with pytest.raises(BasisBudgetError):
        certify_solution(meas, n, 2, X.to(DEV), **kw)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = certify_solution(meas, n, 2, X.to(DEV), basis_size=16, **kw)
    peak = torch.cuda.max_memory_allocated() - before
    print(f"budget: {res.status} it {res.iterations} rs {res.restarts} "
          f"peak {peak} B")
    assert res.status == CertificateStatus.NOT_OPTIMAL
    # the unrestarted basis alone would be 8 * 201 * 202 = 324 816 bytes
    assert peak < 8 * 201 * 202
