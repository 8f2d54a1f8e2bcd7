"""The three kernels of the Chebyshev low-rank product (csrc/rpgp_lowrank.hip) at the edges of what each does between its first
load and its last store: the projection's float64 recurrence, the combine's batched block sum (kCombineBatch = 8 partials per
thread in flight, then a loop) with its coefficient chunks, and the output pass that requests its coordinates, its V element
and its share of U (as float4) before the first wait.  Reference: oracle/cmvm.py in float64; bound: TOL of
test_lowrank_fused_gpu.py.  One reference per (N, J), computed for three columns and shared by every case of that shape."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-7          # the low-rank product against the float64 oracle (test_lowrank_fused_gpu.py)
KAPPA = 0.84932180028801907     # (2 ln 2)^-1/2: a = (z - mid) KAPPA in rpgp_prepare
SCALE = 0.05
N_BATCHES = 2048 * 49 + 1       # 50 row blocks: more than kCombineBatch * G = 48 at PB = 40

_problems = {}


def _pad8(p):
    return (p + 7) & ~7


def _select(h):
    from rpgp_amd import _lib
    lib = _lib.load()
    p, tail = ctypes.c_int(-1), ctypes.c_double(-1.0)
    _lib.check(lib.rpgp_lowrank_select(float(h), 64, ctypes.byref(p), ctypes.byref(tail), None), "rpgp_lowrank_select")
    return p.value


def _width_for(pb):
    """Half-width w of Z whose plan has rank pb - 3 (the middle of the bucket of padded rank pb), by bisection on the host's
    rank selection, which is monotone in h = KAPPA w."""
    lo, hi = 0.0, 9.0 / KAPPA
    assert _select(KAPPA * hi) == 0 or _select(KAPPA * hi) > pb - 3
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        p = _select(KAPPA * mid)
        if p == pb - 3:
            return mid
        if p == 0 or p > pb - 3:
            hi = mid
        else:
            lo = mid
    raise AssertionError("no width gives rank %d" % (pb - 3))


def _rows(N, J):
    """Every row where the float64 reference is cheap, else a stride plus both ends and the rows around the row-block edges."""
    if N * N * J <= 3e8:
        return np.arange(N)
    edges = [np.arange(max(b - 3, 0), min(b + 3, N)) for b in range(2048, N, 2048)]
    return np.unique(np.concatenate([np.arange(0, N, 97), np.arange(70), np.arange(N - 130, N)] + edges))


def _problem(N, J, dev, width=None):
    """(Z, V [N x 3], prep, rows, K v on rows in float64) of one shape; Z normal, or uniform on [-width, width] with both ends
    present in every column."""
    key = (N, J, width)
    if key not in _problems:
        from oracle import cmvm
        from rpgp_amd import ops
        g = torch.Generator().manual_seed(1000 * J + N % 997)
        if width is None:
            Z = torch.randn(N, J, generator=g)
        else:
            Z = (torch.rand(N, J, generator=g) * 2.0 - 1.0) * width
            Z[0, :], Z[1, :] = -width, width
        V = torch.randn(N, 3, generator=g)
        Z, V = Z.to(dev), V.to(dev)
        prep = ops.Prepared(Z)
        assert prep.rank > 0
        rows = _rows(N, J)
        Zh, Vh = Z.double().cpu().numpy(), V.double().cpu().numpy()
        ref = cmvm.mvm(np.ascontiguousarray(Zh[rows]), Zh, Vh, SCALE)
        _problems[key] = (Z, V, prep, rows, Zh, Vh, ref)
    return _problems[key]


def _err(out, ref):
    return np.linalg.norm(out - ref) / np.linalg.norm(ref)


def _check(prob, T, noise, what):
    from rpgp_amd import ops
    Z, V, prep, rows, Zh, Vh, ref = prob
    out = ops.mvm_sym_prepared(prep, V[:, :T].contiguous(), SCALE, noise).double().cpu().numpy()
    e = _err(out[rows], ref[:, :T] + noise * Vh[rows, :T])
    print("%s T=%d noise=%g rank %d rel err %.3g" % (what, T, noise, prep.rank, e))
    assert e <= TOL, (what, T, noise, e)


@pytest.mark.parametrize("noise", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("J", [1, 3, 4, 5, 20, 64])
@pytest.mark.parametrize("N", [1, 63, 65, 2047, 2049, 6145])
def test_shapes_at_the_edges(gpu_device, N, J, T, noise):
    _check(_problem(N, J, gpu_device), T, noise, "N=%d J=%d" % (N, J))


@pytest.mark.parametrize("noise", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 3])
def test_block_sum_longer_than_one_batch(gpu_device, T, noise):
    """50 row blocks at PB = 40 (G = 6 groups of 8 partials in flight): the combine's loop runs a second, partly empty batch."""
    prob = _problem(N_BATCHES, 2, gpu_device, width=_width_for(40))
    assert _pad8(prob[2].rank) == 40
    _check(prob, T, noise, "N=%d J=2" % N_BATCHES)


def test_projection_range(gpu_device):
    from rpgp_amd import ops
    Z, V, prep, rows, Zh, Vh, _ = _problem(2049, 5, gpu_device)
    from oracle import cmvm
    Zs = np.ascontiguousarray(Zh[:, 1:3])
    ref = cmvm.mvm(Zs, Zs, Vh, SCALE) + 0.1 * Vh
    out = ops.mvm_sym_prepared(prep, V, SCALE, 0.1, j0=1, j1=3).double().cpu().numpy()
    e = _err(out, ref)
    print("j=[1,3) of 5 rel err %.3g" % e)
    assert e <= TOL, e


def test_row_shard_leaves_exact_zeros(gpu_device):
    from rpgp_amd import ops
    N = 2049
    Z, V, prep, rows, Zh, Vh, ref = _problem(N, 5, gpu_device)
    out = ops.mvm_sym_prepared(prep, V, SCALE, 0.0, shard=(3, 1)).double().cpu().numpy()
    r0, r1 = N * 1 // 3, N * 2 // 3
    e = _err(out[r0:r1], ref[r0:r1])
    print("shard (3, 1) rel err %.3g" % e)
    assert e <= TOL, e
    assert np.abs(out[:r0]).max() == 0.0 and np.abs(out[r1:]).max() == 0.0


@pytest.mark.parametrize("pb", [8, 16, 24, 32, 40, 48, 56, 64])
def test_every_padded_rank(gpu_device, pb):
    """Z uniform on [-w, w], w chosen on the host so that the plan's rank falls in the bucket of each padded rank."""
    prob = _problem(4097, 3, gpu_device, width=_width_for(pb))
    prep = prob[2]
    assert prep.rank == _select(prep.max_abs * (1.0 + 2.0 ** -20)) and _pad8(prep.rank) == pb, (prep.rank, pb)
    for T in (1, 3):
        _check(prob, T, 0.1, "PB=%d" % pb)


@pytest.mark.parametrize("N,J", [(65, 5), (6145, 20)])
def test_repeatable_and_column_independent(gpu_device, N, J):
    from rpgp_amd import ops
    Z, V, prep = _problem(N, J, gpu_device)[:3]
    a = ops.mvm_sym_prepared(prep, V, SCALE, 0.1)
    assert torch.equal(ops.mvm_sym_prepared(prep, V, SCALE, 0.1), a)
    one = ops.mvm_sym_prepared(prep, V[:, :1].contiguous(), SCALE, 0.1)
    assert torch.equal(one, a[:, :1])


@pytest.mark.parametrize("N,J,T", [(65, 5, 1), (6145, 20, 3)])
def test_in_place(gpu_device, N, J, T):
    """out = V element for element: each element of V is read by the thread that writes it, before it writes."""
    from rpgp_amd import ops
    Z, V, prep = _problem(N, J, gpu_device)[:3]
    Vt = V[:, :T].contiguous()
    ref = ops.mvm_sym_prepared(prep, Vt, SCALE, 0.1)
    buf = Vt.clone()
    res = ops.mvm_sym_prepared(prep, buf, SCALE, 0.1, out=buf)
    assert res.data_ptr() == buf.data_ptr()
    assert torch.equal(buf, ref)
