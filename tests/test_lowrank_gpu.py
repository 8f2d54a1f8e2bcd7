"""The Chebyshev low-rank form of the prepared product (csrc/rpgp_lowrank.hip) through ops.mvm_sym_prepared: the benchmark's
C4 launch on every row against the float64 C oracle at the exact kernel's own accuracy, against the exact sweep
(RPGP_LOWRANK=0) for several right-hand-side counts, j-ranges, pair shards, ragged sizes, a constant Z, the fall-back to the
sweep for a range too wide for the largest rank, run-to-run bit identity and the profiling hook."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sweep(fn):
    old = os.environ.get("RPGP_LOWRANK")
    os.environ["RPGP_LOWRANK"] = "0"
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("RPGP_LOWRANK", None)
        else:
            os.environ["RPGP_LOWRANK"] = old


def _rel(a, b):
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _inputs(N, J, T, dev, seed):
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(N, J, generator=g).to(dev)
    V = torch.randn(N, T, generator=g).to(dev)
    return Z, V


def test_bench_launch_every_row_against_the_c_oracle(gpu_device):
    import bench
    from oracle import cmvm
    from rpgp_amd import ops
    N, d, J = 50000, 20, 20
    X, P, ls, V = bench.make_inputs(N, d, J, 1, gpu_device)
    Z = ops.project(X, (P / ls[:, None]).contiguous())
    prep = ops.Prepared(Z)
    assert prep.fast_ok and 30 <= prep.rank <= 48
    out = ops.mvm_sym_prepared(prep, V, 1.0 / J, 0.1).double().cpu().numpy()
    Zh = Z.double().cpu().numpy()
    ref = cmvm.mvm(Zh, Zh, V.double().cpu().numpy(), 1.0 / J, 0.1)
    assert np.linalg.norm(out - ref) / np.linalg.norm(ref) <= 5e-7
    assert np.abs(out - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("T", [1, 4, 11])
def test_matches_the_oracle_and_the_sweep(gpu_device, T):
    """On a range wider than C4's the sweep itself is further from float64 (its per-entry error grows with a'^2): the
    low-rank product is held to 5e-7 against the oracle, and to the sweep's own tolerance against the sweep."""
    from oracle import cmvm
    from rpgp_amd import ops
    Z, V = _inputs(20011, 20, T, gpu_device, 7 + T)
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    lr = ops.mvm_sym_prepared(prep, V, 0.05, 0.1)
    sw = _sweep(lambda: ops.mvm_sym_prepared(prep, V, 0.05, 0.1))
    assert not torch.equal(lr, sw)                       # really the other path
    assert _rel(lr, sw) <= 2e-6
    rows = np.arange(0, 20011, 7)
    Zh, Vh = Z.double().cpu().numpy(), V.double().cpu().numpy()
    ref = cmvm.mvm(Zh[rows], Zh, Vh, 0.05) + 0.1 * Vh[rows]
    o = lr.double().cpu().numpy()[rows]
    assert np.linalg.norm(o - ref) / np.linalg.norm(ref) <= 5e-7


def test_j_ranges_and_pair_shards(gpu_device):
    from rpgp_amd import ops
    Z, V = _inputs(15013, 20, 2, gpu_device, 3)
    prep = ops.Prepared(Z)
    full = _sweep(lambda: ops.mvm_sym_prepared(prep, V, 0.05, 0.3))
    for a, b in [(0, 3), (3, 11), (19, 20), (0, 20)]:
        lr = ops.mvm_sym_prepared(prep, V, 0.05, 0.0, j0=a, j1=b)
        assert _rel(lr, _sweep(lambda: ops.mvm_sym_prepared(prep, V, 0.05, 0.0, j0=a, j1=b))) <= 2e-6, (a, b)
    for world in (3, 8):
        parts = [ops.mvm_sym_prepared(prep, V, 0.05, 0.3 if r == 0 else 0.0, shard=(world, r)) for r in range(world)]
        assert _rel(sum(parts), full) <= 2e-6, world
        # a rank writes its own rows of K v; the noise-free ranks write zeros elsewhere
        r0, r1 = 15013 * 1 // world, 15013 * 2 // world
        assert float(parts[1][:r0].abs().max()) == 0.0 and float(parts[1][r1:].abs().max()) == 0.0


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_ragged_sizes(gpu_device, N):
    from oracle import cmvm
    from rpgp_amd import ops
    Z, V = _inputs(N, 7, 3, gpu_device, N)
    prep = ops.Prepared(Z)
    assert prep.rank > 0
    out = ops.mvm_sym_prepared(prep, V, 0.2, 0.1)
    ref = cmvm.mvm(Z.double().cpu().numpy(), Z.double().cpu().numpy(), V.double().cpu().numpy(), 0.2, 0.1)
    assert np.linalg.norm(out.double().cpu().numpy() - ref) / np.linalg.norm(ref) <= 5e-7


def test_constant_z_is_rank_one(gpu_device):
    from rpgp_amd import ops
    rng = np.random.default_rng(0)
    Z = torch.from_numpy(np.repeat(rng.standard_normal((1, 5)).astype(np.float32), 300, axis=0)).to(gpu_device)
    V = torch.from_numpy(rng.standard_normal((300, 1)).astype(np.float32)).to(gpu_device)
    prep = ops.Prepared(Z)
    assert prep.rank == 1
    out = ops.mvm_sym_prepared(prep, V, 0.2, 0.0).cpu().numpy().ravel()
    np.testing.assert_allclose(out, np.full(300, 0.2 * 5 * float(V.sum())), rtol=2e-5, atol=2e-4)


def test_wide_range_falls_back_to_the_sweep(gpu_device):
    from rpgp_amd import ops
    rng = np.random.default_rng(11)
    Zh = rng.uniform(-11.2, 11.2, (3001, 6)).astype(np.float32)
    Zh[0], Zh[1] = -11.2, 11.2                            # max|a| = 11.2 * 0.849 = 9.5: rank 69 > 64, a^2 < 100
    Z = torch.from_numpy(Zh).to(gpu_device)
    V = torch.from_numpy(rng.standard_normal((3001, 1)).astype(np.float32)).to(gpu_device)
    prep = ops.Prepared(Z)
    assert prep.fast_ok and prep.rank == 0
    assert torch.equal(ops.mvm_sym_prepared(prep, V, 0.3, 0.1), _sweep(lambda: ops.mvm_sym_prepared(prep, V, 0.3, 0.1)))


def test_repeated_calls_are_bit_identical_and_profiled(gpu_device):
    from rpgp_amd import ops, _lib
    lib = _lib.load()
    Z, V = _inputs(50000, 20, 1, gpu_device, 5)
    prep = ops.Prepared(Z)
    a = ops.mvm_sym_prepared(prep, V, 0.05, 0.1)
    _lib.check(lib.rpgp_profile_begin(), "rpgp_profile_begin")
    b = ops.mvm_sym_prepared(prep, V, 0.05, 0.1)
    c = ops.mvm_sym_prepared(prep, V, 0.05, 0.1)
    torch.cuda.synchronize()
    ms, cnt = ctypes.c_float(0), ctypes.c_int(0)
    _lib.check(lib.rpgp_profile_end(ctypes.byref(ms), ctypes.byref(cnt)), "rpgp_profile_end")
    assert torch.equal(a, b) and torch.equal(a, c)
    assert cnt.value == 2 and ms.value > 0
