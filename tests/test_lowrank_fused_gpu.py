"""The projection pass of the Chebyshev low-rank product (csrc/rpgp_lowrank.hip: a transposed wave reduction whose layout
depends on the padded rank, block partials that the combine adds in block order) beyond test_lowrank_gpu.py: one plan through
many calls of changing shape against the float64 oracle with the first call repeated bit for bit, the C4 product under a busy
chip with every value compared bit for bit (a partial read before it was written is a silent wrong sum), ragged sizes at
1, 2 and 3 row blocks, and a product of 210 columns.  An in-launch combine by the last-arriving workgroup was built against
these tests and measured slower than the separate launch; they stay as the checks any such hand-off must pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-7          # the low-rank product against the float64 oracle (test_lowrank_gpu.py)


def _inputs(N, J, T, dev, seed):
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(N, J, generator=g).to(dev)
    V = torch.randn(N, T, generator=g).to(dev)
    return Z, V


def _oracle(Zh, Vh, rows, scale, noise, a, b):
    from oracle import cmvm
    Zs = np.ascontiguousarray(Zh[:, a:b])
    return cmvm.mvm(np.ascontiguousarray(Zs[rows]), Zs, Vh, scale) + noise * Vh[rows]


def _err(out, ref):
    return np.linalg.norm(out - ref) / np.linalg.norm(ref)


def test_one_plan_through_changing_shapes(gpu_device):
    from rpgp_amd import ops
    N, J = 20011, 20
    Z, _ = _inputs(N, J, 1, gpu_device, 21)
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    Zh = Z.double().cpu().numpy()
    rows = np.arange(0, N, 23)
    g = torch.Generator().manual_seed(22)
    Vs = {T: torch.randn(N, T, generator=g).to(gpu_device) for T in (1, 4, 11, 12, 17)}
    first = None
    for T, V in Vs.items():
        Vh = V.double().cpu().numpy()
        for a, b in [(0, 3), (3, 11), (19, 20), (0, 20)]:
            out = ops.mvm_sym_prepared(prep, V, 0.05, 0.1, j0=a, j1=b)
            if first is None:
                first = (T, a, b, out.clone())
            e = _err(out.double().cpu().numpy()[rows], _oracle(Zh, Vh, rows, 0.05, 0.1, a, b))
            print("T=%d j=[%d,%d) rel err %.3g" % (T, a, b, e))
            assert e <= TOL, (T, a, b, e)
        for world, r in [(3, 1), (8, 7)]:
            out = ops.mvm_sym_prepared(prep, V, 0.05, 0.0, shard=(world, r)).double().cpu().numpy()
            r0, r1 = N * r // world, N * (r + 1) // world
            mine = rows[(rows >= r0) & (rows < r1)]
            e = _err(out[mine], _oracle(Zh, Vh, mine, 0.05, 0.0, 0, J))
            print("T=%d shard (%d, %d) rel err %.3g" % (T, world, r, e))
            assert e <= TOL, (T, world, r, e)
            assert np.abs(out[:r0]).max(initial=0.0) == 0.0 and np.abs(out[r1:]).max(initial=0.0) == 0.0
    T, a, b, ref = first
    assert torch.equal(ops.mvm_sym_prepared(prep, Vs[T], 0.05, 0.1, j0=a, j1=b), ref)


def test_c4_product_under_load_is_bit_identical(gpu_device):
    """Uneven load, caches warm from the previous call, every word checked: the benchmark's product 300 times while a second
    stream copies 64 MB device to device per product."""
    import bench
    from rpgp_amd import ops
    N, d, J, reps = 50000, 20, 20, 300
    X, P, ls, V = bench.make_inputs(N, d, J, 1, gpu_device)
    Z = ops.project(X, (P / ls[:, None]).contiguous())
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    quiet = ops.mvm_sym_prepared(prep, V, 1.0 / J, 0.1).clone()
    torch.cuda.synchronize()
    src = torch.ones(16 << 20, device=gpu_device)
    dst = torch.empty_like(src)
    outs = torch.empty(reps, N, 1, device=gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    for k in range(reps):
        with torch.cuda.stream(side):
            dst.copy_(src)
        ops.mvm_sym_prepared(prep, V, 1.0 / J, 0.1, out=outs[k])
    torch.cuda.synchronize()
    same = (outs == quiet.unsqueeze(0)).flatten(1).all(dim=1)
    assert bool(same.all()), "products that differ from the quiet one: %s" % torch.nonzero(~same).flatten().tolist()[:20]


@pytest.mark.parametrize("T", [1, 11])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2048, 2049, 4097])
def test_ragged_sizes(gpu_device, N, T):
    from rpgp_amd import ops
    Z, V = _inputs(N, 7, T, gpu_device, 100 + N + T)
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    out = ops.mvm_sym_prepared(prep, V, 0.2, 0.1).double().cpu().numpy()
    e = _err(out, _oracle(Z.double().cpu().numpy(), V.double().cpu().numpy(), np.arange(N), 0.2, 0.1, 0, 7))
    print("N=%d T=%d rel err %.3g" % (N, T, e))
    assert e <= TOL, e


def test_many_columns(gpu_device):
    """J T = 4 200 (projection, column) pairs in one call, then a narrow call on the same plan: a column's sums do not depend
    on how many columns travel with it."""
    from rpgp_amd import ops
    N, J, T = 3001, 20, 210
    Z, V = _inputs(N, J, T, gpu_device, 31)
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    Zh, Vh = Z.double().cpu().numpy(), V.double().cpu().numpy()
    rows = np.arange(0, N, 10)
    a = ops.mvm_sym_prepared(prep, V, 0.05, 0.1)
    e = _err(a.double().cpu().numpy()[rows], _oracle(Zh, Vh, rows, 0.05, 0.1, 0, J))
    print("T=%d rel err %.3g" % (T, e))
    assert e <= TOL, e
    small = ops.mvm_sym_prepared(prep, V[:, :3].contiguous(), 0.05, 0.1)
    e = _err(small.double().cpu().numpy()[rows], _oracle(Zh, Vh[:, :3], rows, 0.05, 0.1, 0, J))
    assert e <= TOL, e
    assert torch.equal(ops.mvm_sym_prepared(prep, V, 0.05, 0.1), a)
    assert torch.equal(small, a[:, :3])
