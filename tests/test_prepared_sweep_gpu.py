"""The exact prepared sweep (rpgp_mvm_sym_prepared_range: mvm_fact_kernel<JT, TT, R> of csrc/rpgp_kernels.hip, the hand-scheduled
kernels of csrc/rpgp_fact_asm.hip, the float64 slab reducer) against float64, ENTRY BY ENTRY, in every piece it compiles.
ops.mvm_sym_prepared serves the Chebyshev low-rank form whenever the plan has a rank, so everything here runs inside
prepared_sweep_reference.sweep(): RPGP_LOWRANK=0, and RPGP_FACT_ASM where a case is there for one of the two kernel families.

(a) Unit right-hand sides: V[:, t] = e_c for the probe columns c of edge_columns(N) (both sides of every kind of chunk, stage,
subtile and row-block boundary, the ragged tail), so out[:, t] = scale K[:, c] + noise e_c with nothing summed over columns.
Every output is held to  2 scale entry_bound + u |ref|  (tests/prepared_sweep_reference.py: the derived float32 bound of the
factorised form, margin 2 because the 1 ULP of the hardware exponential is documented, not measured; u |ref| the final cast).
One probe column reads a column of K through the row-side accumulators for the rows up to its block and through the rotating
transposed accumulators and slabT behind it, so every row edge (ragged last block, second row of a lane, masked rows >= N) meets
every column edge.  Each case prints its worst error / un-margined bound (measured: 0.71 on the wide range, 0.23 - 0.57 on
the others; the float32 numpy emulation of the host module gives 0.73 and 0.35 - 0.51).
(b) All of K at N = 300 and 257 through identity blocks, and its symmetry.
(c) Dense right-hand sides against oracle/cmvm.c for the column sums and the reducer, and run-to-run bit identity."""
import functools

import numpy as np
import pytest
import torch

from tests import prepared_sweep_reference as psr

pytestmark = pytest.mark.gpu

U = psr.U
SCALE, NOISE = np.float32(0.07), np.float32(0.3)          # float32 values: what the C-ABI receives is what the reference uses


def _id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=4)
def _reference(N, J, T, j0, j1, kind, limit):
    """(Z, probe columns, float64 reference N x C with the noise on the diagonal entries, un-margined bound of scale K)."""
    Z = psr.wide_inputs(N, J) if kind == "wide" else psr.normal_inputs(N, J, N + J + T)
    cols = psr.edge_columns(N, limit)
    K, terms = psr.kernel_columns(Z, cols, j0, j1)
    bound = float(SCALE) * psr.entry_bound(Z, cols, j0, j1, terms=terms)
    ref = float(SCALE) * K
    ref[cols, np.arange(len(cols))] += float(NOISE)
    for a in (Z, ref, bound):
        a.setflags(write=False)
    return Z, cols, ref, bound


def _prepared(Z, dev):
    from rpgp_amd import ops
    prep = ops.Prepared(torch.tensor(Z).to(dev))           # (a copy: the cached reference arrays are read-only)
    assert prep.fast_ok
    return prep


def _probe(prep, N, cols, T, dev, j0, j1, env_asm, world=1, lowrank_env=True):
    """float64 N x len(cols): the probes' outputs (pair shards summed in float64 on the host, noise on rank 0)."""
    from rpgp_amd import ops
    import contextlib
    out = np.full((N, len(cols)), np.nan)
    where = {c: q for q, c in enumerate(cols)}
    with (psr.sweep(env_asm) if lowrank_env else contextlib.nullcontext()):
        for Vh, blk in psr.unit_blocks(N, cols, T):
            V = torch.from_numpy(Vh).to(dev)
            if world == 1:
                got = ops.mvm_sym_prepared(prep, V, SCALE, NOISE, j0=j0, j1=j1).cpu().numpy().astype(np.float64)
            else:
                got = sum(ops.mvm_sym_prepared(prep, V, SCALE, NOISE if r == 0 else 0.0, j0=j0, j1=j1,
                                               shard=(world, r)).cpu().numpy().astype(np.float64) for r in range(world))
            assert got.shape == (N, T)
            for t, c in enumerate(blk):
                out[:, where[c]] = got[:, t]
    return out


def _hold(got, ref, bound, what, casts=1):
    """Every entry within 2 bound + casts u |ref|; prints and returns the worst error / (bound + casts u |ref|)."""
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), what
    cast = casts * U * np.abs(ref)
    ratio = err / (bound + cast)
    i, q = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("sweep-ratio %s worst %.3f at row %d probe %d" % (what, ratio[i, q], i, q))
    bad = err > 2.0 * bound + cast
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s: %d entries beyond the bound; first at row %d, probe %d: got %.9g ref %.9g err %.3g allowed %.3g"
                             % (what, int(bad.sum()), r, c, got[r, c], ref[r, c], err[r, c], (2.0 * bound + cast)[r, c]))
    return float(ratio[i, q])


def _unit_case(dev, N, J, T, j0=0, j1=None, env=(None,), kind="normal", limit=48, world=1):
    j1 = J if j1 is None else j1
    Z, cols, ref, bound = _reference(N, J, T, j0, j1, kind, limit)
    prep = _prepared(Z, dev)
    outs = {}
    for env_asm in env:
        outs[env_asm] = _probe(prep, N, cols, T, dev, j0, j1, env_asm, world)
        _hold(outs[env_asm], ref, bound, "N%d J%d T%d j%d:%d asm=%s world=%d" % (N, J, T, j0, j1, env_asm, world),
              casts=3 if world > 1 else 1)
    return prep, Z, cols, outs


# ---- (a) unit vectors ------------------------------------------------------------------------------------------------------------
ONE_ROW = [(300, 19, 12),        # J pieces 10 + 8 + 1 (accumulate twice), T piece 12
           (257, 17, 4),         # 10 + 5 + 2, T piece 4, one row past a 256-row block
           (700, 13, 1),         # 10 + 3 (the padded half slot), T piece 1
           (63, 14, 5),          # 10 + 4, 5 columns of the 12 piece
           (65, 1, 3),           # JT = 1, 3 columns of the 4 piece
           (1, 3, 2),            # a single point
           (2049, 20, 13),       # JT = 20, T pieces 12 + 1
           (4095, 7, 16)]        # 5 + 2, T pieces 12 + 4, the last N of the one-row plan at T > 4


@pytest.mark.parametrize("case", ONE_ROW, ids=_id)
def test_one_row_per_lane_every_piece(gpu_device, case):
    """mvm_fact_kernel<JT, TT, 1>: every JT piece, first and accumulating; every T piece, full and with tcnt < TT."""
    _unit_case(gpu_device, *case)


TWO_ROWS = [(4096, 20, 12),      # the first N of the two-row plan
            (4161, 19, 5),       # 10 + 8 + 1, 5 of 12, a ragged subtile of one column behind 8 row blocks and 65 chunks
            (4161, 6, 13),       # 5 + 1 at T pieces 12 + 1: the odd piece and JT = 1 at t0 = 12
            (10240, 17, 4),      # the T <= 4 threshold of the two-row plan: 10 + 5 + 2, T piece 4
            (10303, 20, 2)]      # 2 of the 4 piece


@pytest.mark.parametrize("case", TWO_ROWS, ids=_id)
def test_two_rows_per_lane_compiler_kernels(gpu_device, case):
    """mvm_fact_kernel<JT, TT, 2> (RPGP_FACT_ASM=0 keeps the hand-scheduled kernels out of the T = 1 pieces)."""
    _unit_case(gpu_device, *case, env=("0",))


ASM_TAIL = [(4161, 20, 13, 0, 20),     # the J = 20 loop with ldv = 13, t0 = 12 on the non-tapered plan
            (4161, 18, 13, 0, 18),     # thin 10, then thin 8 with accumulate
            (4225, 12, 13, 0, 12),     # thin 10 + thin 2
            (4161, 7, 25, 0, 7),       # T pieces 12 + 12 + 1: thin 5 + thin 2 at t0 = 24
            (5000, 20, 13, 3, 6),      # thin 3
            (5000, 20, 13, 2, 6)]      # thin 4


@pytest.mark.parametrize("case", ASM_TAIL, ids=_id)
def test_asm_kernels_serve_the_tail_column_of_a_block(gpu_device, case):
    """T = 13 (25) splits into 12 (+ 12) + 1 and the last column goes to the hand-scheduled kernels with ldv = T, t0 = T - 1,
    on the plan made for T right-hand sides (two rows per lane from N = 4096, no taper).  Probes under RPGP_FACT_ASM=1 and =0
    against the bound; with a dense right-hand side the tail column differs bitwise between the settings (another summation
    order: the hand-scheduled kernel ran) while the other columns are equal (it served nothing else)."""
    from rpgp_amd import ops
    N, J, T, j0, j1 = case
    prep, Z, cols, outs = _unit_case(gpu_device, N, J, T, j0, j1, env=("1", "0"))
    V = torch.from_numpy(psr.dense_rhs(N, T, N + J + T + 1)).to(gpu_device)
    dense = {}
    for env_asm in ("1", "0"):
        with psr.sweep(env_asm):
            dense[env_asm] = ops.mvm_sym_prepared(prep, V, SCALE, NOISE, j0=j0, j1=j1)
    assert torch.equal(dense["1"][:, :T - 1], dense["0"][:, :T - 1])
    assert not torch.equal(dense["1"][:, T - 1], dense["0"][:, T - 1])


@pytest.mark.parametrize("case", [(10240, 20, 1), (16449, 20, 1), (16449, 3, 1)], ids=_id)
def test_asm_kernels_t1_probes(gpu_device, case):
    """The hand-scheduled J = 20 and 3-projection kernels on their own plan (tapered for J = 20), one probe per call; 16 449 is
    the first size with chunks of 128 columns (two subtiles per stage).  The 16 probes nearest the ends."""
    _unit_case(gpu_device, *case, env=("1",), limit=16)


@pytest.mark.parametrize("case", [(4161, 20, 13), (10303, 20, 1)], ids=_id)
def test_pair_shards_sum_to_the_entries(gpu_device, case):
    """Three workgroup ranges (partial row blocks, zero-initialised slabs): the partial products, summed in float64."""
    _unit_case(gpu_device, *case, world=3)


def test_wide_range_entries_from_one_to_underflow(gpu_device):
    """max|a| = 9.5: beyond rank 64, so the sweep is what ops.mvm_sym_prepared runs by default; entries from 1 down to
    underflow; the default call and the forced sweep are the same launches."""
    N, J, T = 3001, 6, 12
    prep, Z, cols, outs = _unit_case(gpu_device, N, J, T, kind="wide")
    assert prep.rank == 0 and abs(prep.max_abs - 9.5) < 0.05
    Zr, colsr, ref, bound = _reference(N, J, T, 0, J, "wide", 48)
    assert ref.min() < 1e-30 and ref.max() > float(SCALE) * J
    default = _probe(prep, N, cols, T, gpu_device, 0, J, None, lowrank_env=False)
    assert np.array_equal(default, outs[None])


# ---- (b) the whole matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", [(300, 19), (257, 17)])
def test_whole_matrix_and_its_symmetry(gpu_device, N, J):
    from rpgp_amd import ops
    Z = psr.normal_inputs(N, J, N + J + 12)
    cols = list(range(N))
    K, terms = psr.kernel_columns(Z, cols)
    bound = float(SCALE) * psr.entry_bound(Z, cols, terms=terms)
    ref = float(SCALE) * K + float(NOISE) * np.eye(N)
    prep = _prepared(Z, gpu_device)
    got = _probe(prep, N, cols, 12, gpu_device, 0, J, None)
    _hold(got, ref, bound, "whole N%d J%d" % (N, J))
    sym = np.abs(got - got.T)
    assert (sym <= 2.0 * (np.minimum(bound, bound.T) + U * np.abs(ref))).all(), float(sym.max())


# ---- (c) dense right-hand sides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2049, 20, 13), (4161, 18, 13), (4161, 19, 5), (10303, 20, 2), (16449, 20, 1)], ids=_id)
def test_dense_rhs_matches_the_c_oracle_and_repeats(gpu_device, case):
    from oracle import cmvm
    from rpgp_amd import ops
    N, J, T = case
    Z = psr.normal_inputs(N, J, N + J + T)
    Vh = psr.dense_rhs(N, T, N + J + T + 1)
    prep = _prepared(Z, gpu_device)
    V = torch.from_numpy(Vh).to(gpu_device)
    with psr.sweep():
        out = ops.mvm_sym_prepared(prep, V, SCALE, NOISE)
        again = ops.mvm_sym_prepared(prep, V, SCALE, NOISE)
    assert torch.equal(out, again)
    Zd = Z.astype(np.float64)
    ref = cmvm.mvm(Zd, Zd, Vh.astype(np.float64), float(SCALE), float(NOISE))
    got = out.cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)
    print("sweep-dense N%d J%d T%d worst column %.3g worst entry %.3g of max|ref|" % (N, J, T, rel.max(), np.abs(got - ref).max() / np.abs(ref).max()))
    assert rel.max() < 2e-6
    assert np.abs(got - ref).max() < 1e-5 * np.abs(ref).max()
