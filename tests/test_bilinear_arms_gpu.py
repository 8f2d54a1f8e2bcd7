"""Every piece, slice and size regime of the derivative kernels against float64 (tests/bilinear_reference.py).

The bilinear derivative is a dispatch tree; each case below names the arm it walks.  Every result is held by
`bilinear_reference.check` to the 2-norm gates of the project (2e-5 / 1e-11, whole slice and per column), to
|got - ref| <= c u B entrywise (B: the sum of the absolute values of what the kernel adds up) and |gs - ref| <= c u Bs,
and to untouched columns outside [j0, j1); float32 cases run twice and must agree bit for bit (the float64 path adds
atomically).  All inputs are seeded: Z ~ 0.8 N(0, 1), L, R ~ 0.1 N(0, 1), scale = 0.05.

  float32, ops.bilinear_grad(Z, L, R, scale, j0, j1) on a J = 20 matrix; slice sets S1 = 0:7 7:14 14:20 (J-sharding on 3
  ranks: pieces 5+2, 5+2, 5+1), S2 = 0:3 3:7 7:17 17:20 (3, 4, 10, 3), S3 = 2:10 (8: register staging), S4 = 0:20, S5 = 5:6 6:8
    N = 300     T = 1, 3, 12     plain sweep, bilinear_kernel<JT, 1 / 4 / 12>                              S1 S2 S5
    N = 2047    T = 4            last N of the plain sweep                                                 S1 S4
    N = 2048    T = 1, 4, 5, 12  first N of the symmetric sweep, four exact row blocks, TT = 4 and 12      S1 .. S5
    N = 2300    T = 1, 4, 11     ragged (4 * 512 + 252, last subtile 60 columns), 4-unrolled slab loops    S1 .. S5
    N = 2300    T = 13, 24       the 12-column accumulation of ops.bilinear_grad with a slice              S1
    N = 16500   T = 3, 11        chunks of two subtiles, ragged tail; 3 x 22 rows; gscale by checksum      7:14 S4
    N = 192000  T = 1            plain sweep above the symmetric sweep's limit; J = 4, 3 x 22 rows         1:3
    (S4 with 4 < T <= 12 at N >= 2048: RPGP_BIL_ASM=1 and =0; the S1 slices summed are S4 to 2e-6)
  C-ABI with ldz = 10 (NaN padding) and ldg = 12 (sentinel-filled): N = 2300 and 300, J = 7, T = 4, slices 0:7 and 2:7
  dense-weight form, float32 and float64: N = 1100, J = 20, S1 and S4
  float64 derivative: J = 35 (pieces 20 + 8 + 4 + 2 + 1) whole and 3:11 (piece 8), N = 300, T = 1, 4, 5, 13, 16 (TT = 4 / 12,
    T in passes); N = 4200, J = 7, T = 5 (column splits of two 64-column tiles with a ragged end)
  related arms at the per-column gates 1e-5 / 1e-12: ops.mvm_rect / ops.dense on S1 at (M, N) = (97, 2300), (1, 50) in both
    precisions; the float64 product with J = 35, N = 4200, T = 3, 13, 16 (square on 150 rows, rectangular with M = 1)

The constant of the entrywise gate: c_ref = 3.64 (tests/test_bilinear_reference_host.py: the largest ratio of the
sequential float32 restatement over the cases above with N <= 2300; by group N300 2.89, N2047 2.00, N2048 3.13, N2300 3.05,
strided 1.80, dense 3.64), hence c = 16 c_ref rounded up to a power of two = 64 = the cap, in both precisions.

Largest |got - ref| / (u B) an MI355X reached (c = 64), per arm over its slices; each case prints its own as an `ARM` line
under `pytest -s`.  Columns: cases, largest entrywise ratio and its slice, largest |gs - ref| / (u Bs), largest per-column
relative 2-norm.  The largest of all is 2.24: the kernels sum in tiles, slabs and (symmetric sweep) float64, so they stay
below the sequential restatement's 3.64.
    N300-T1                 9     2.24 at 7:14     0.009   1.0e-06
    N300-T3                 9     0.91 at 0:7      0.019   4.0e-07
    N300-T12                9     0.50 at 7:14     0.005   3.0e-07
    N2047-T4                4     0.41 at 14:20    0.001   5.2e-07
    N2048-T1               11     0.46 at 14:20    0.002   2.4e-07
    N2048-T4               11     0.28 at 0:7      0.001   2.3e-07
    N2048-T5               10     0.26 at 0:7      0.003   2.5e-07
    N2048-T5-asm1           1     0.21 at 0:20     0.001   2.5e-07
    N2048-T5-asm0           1     0.26 at 0:20     0.001   2.5e-07
    N2048-T12              10     0.21 at 0:7      0.002   2.0e-07
    N2048-T12-asm1          1     0.15 at 0:20     0.000   1.9e-07
    N2048-T12-asm0          1     0.21 at 0:20     0.000   2.0e-07
    N2300-T1               11     0.40 at 7:14     0.002   6.5e-07
    N2300-T4               11     0.24 at 14:20    0.002   2.2e-07
    N2300-T11              10     0.12 at 14:20    0.001   2.4e-07
    N2300-T11-asm1          1     0.15 at 0:20     0.001   2.3e-07
    N2300-T11-asm0          1     0.12 at 0:20     0.001   2.4e-07
    N2300-T13               3     0.11 at 0:7      0.001   2.4e-07
    N2300-T24               3     0.09 at 7:14     0.001   2.4e-07
    N16500-T3               2     0.07 at 7:14       -     3.5e-07      (66 rows; gscale against the checksum: see the test)
    N16500-T11              1     0.03 at 7:14       -     3.0e-07
    N16500-T11-asm1         1     0.04 at 0:20       -     3.5e-07
    N16500-T11-asm0         1     0.04 at 0:20       -     3.6e-07
    N192000-T1              1     0.60 at 1:3        -     5.7e-06
    strided-N2300           2     0.20 at 0:7      0.001   2.2e-07
    strided-N300            2     0.70 at 0:7      0.005   2.9e-07
    dense-f32-N1100         4     1.03 at 0:7      0.007   3.1e-07
    dense-f64-N1100         4     0.75 at 0:20     0.002   3.5e-16
    f64-N300-T1             2     0.83 at 0:35     0.020   9.0e-16
    f64-N300-T4             2     0.54 at 0:35     0.013   4.8e-16
    f64-N300-T5             2     0.58 at 0:35     0.002   4.9e-16
    f64-N300-T13            2     0.33 at 0:35     0.003   4.5e-16
    f64-N300-T16            2     0.29 at 0:35     0.005   4.1e-16
    f64-N4200-T5            1     0.17 at 0:7      0.001   4.9e-16
  S1 slices summed against S4: bit-equal under RPGP_BIL_ASM=0 at all seven (N, T); 1.5e-7, 1.6e-7, 1.8e-7 from the hand-scheduled
  loop at (2048, 5), (2048, 12), (2300, 11).  Related arms: float32 products <= 5.3e-7, blocks <= 1.6e-7; float64 <= 2.0e-14.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc
from tests import bilinear_reference as br
from tests.test_bil_asm_gpu import _with_asm

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e9


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _report(case, st):
    print("ARM %-34s ratio %8.3f  gscale %s  rel %.2e  column %.2e"
          % (case, st["ratio"], "   -    " if st["gs_ratio"] is None else "%8.3f" % st["gs_ratio"], st["rel"], st["col_rel"]))


def _three_row_sets(N):
    mid = N // 2 - 69 if N == 16500 else N // 2 - 11          # 16500: rows 8181 .. 8202
    return np.concatenate([np.arange(0, 22), np.arange(mid, mid + 22), np.arange(N - 22, N)])


# ---- float32 slices through ops.bilinear_grad on a J = 20 matrix, full-matrix references --------------------------------
@functools.lru_cache(maxsize=None)
def _bank(N):
    Z, LR = br.inputs(N, 20, list(br.F32_TABLE[N]))
    return Z, LR, br.Bank(Z, dict(LR), br.SCALE)


def _asm_modes(N, T, sl):
    """The whole-J launches with T > 4 of the symmetric sweep exist twice: hand-scheduled loop and compiler's kernel."""
    return (1, 0) if (N >= 2048 and sl == (0, 20) and 4 < T <= 12) else (None,)


F32_CASES = [pytest.param(N, T, sl, asm, id="N%d-T%d-%d:%d%s" % (N, T, sl[0], sl[1], "" if asm is None else "-asm%d" % asm))
             for N, table in br.F32_TABLE.items() for T, slices in table.items() for sl in slices
             for asm in _asm_modes(N, T, sl)]


def _run(fn, asm):
    return fn() if asm is None else _with_asm(bool(asm), fn)


@pytest.mark.parametrize("N,T,sl,asm", F32_CASES)
def test_f32_slice_against_float64(gpu_device, request, N, T, sl, asm):
    from rpgp_amd import ops
    Z, LR, bank = _bank(N)
    Zd, Ld, Rd = _dev(Z, gpu_device), _dev(LR[T][0], gpu_device), _dev(LR[T][1], gpu_device)
    gZ, gs = _run(lambda: ops.bilinear_grad(Zd, Ld, Rd, br.SCALE, sl[0], sl[1]), asm)
    gZ2, gs2 = _run(lambda: ops.bilinear_grad(Zd, Ld, Rd, br.SCALE, sl[0], sl[1]), asm)
    assert torch.equal(gZ, gZ2) and torch.equal(gs, gs2)                         # run-to-run bit identity
    case = request.node.callspec.id
    st = br.check(gZ.cpu().numpy(), float(gs), bank.ref(T, sl[0], sl[1]), br.C, br.U32, case,
                  outside=None if sl == (0, 20) else 0.0)
    _report(case, st)


@pytest.mark.parametrize("N,T", [(N, T) for N in (2048, 2300) for T, s in br.F32_TABLE[N].items() if (0, 20) in s])
def test_s1_slices_sum_to_the_whole(gpu_device, N, T):
    """The 7 / 7 / 6 slices of J-sharded training on 3 ranks, summed, are the whole-J derivative to 2e-6 (as
    test_kernels_gpu.py::test_pair_sharded_mvm_sums_to_full holds the product).  Like for like — the slices and the whole both
    from the compiler's `bilinear_sym_kernel` (RPGP_BIL_ASM=0) — the two are bit-equal: 0 at every (N, T).  For 4 < T <= 12 the
    whole-J call takes the hand-scheduled loop by default, which forms S and sums in another order: 1.5e-7 .. 1.9e-7 from
    the slices on an MI355X, held to the same 2e-6."""
    from rpgp_amd import ops
    Z, LR, bank = _bank(N)
    Zd, Ld, Rd = _dev(Z, gpu_device), _dev(LR[T][0], gpu_device), _dev(LR[T][1], gpu_device)
    parts = [ops.bilinear_grad(Zd, Ld, Rd, br.SCALE, j0, j1) for j0, j1 in br.S1]
    acc = sum(p[0] for p in parts)
    gs_acc = sum(float(p[1]) for p in parts)
    for asm in (0, 1) if 4 < T <= 12 else (0,):
        whole, gs_whole = _with_asm(bool(asm), lambda: ops.bilinear_grad(Zd, Ld, Rd, br.SCALE))
        rel = float((acc.double() - whole.double()).norm() / whole.double().norm())
        print("ARM sum-of-S1 N%d T%d asm%d rel %.2e gscale %.2e" % (N, T, asm, rel, abs(gs_acc - float(gs_whole)) / abs(float(gs_whole))))
        if asm == 0:
            assert torch.equal(acc, whole)
        assert rel < 2e-6
        # (each of the two float32 figures lies within c u Bs of the float64 value)
        assert abs(gs_acc - float(gs_whole)) <= 2 * br.C * br.U32 * bank.ref(T, 0, 20).Bs


# ---- chunks of two subtiles (N = 16500) and the plain sweep above the symmetric sweep's limit (N = 192000) -------------
LARGE = {16500: dict(J=20, Ts=[3, 11], slices=[(7, 14), (0, 20)]), 192000: dict(J=4, Ts=[1], slices=[(1, 3)])}


@functools.lru_cache(maxsize=None)
def _bank_rows(N):
    spec = LARGE[N]
    Z, LR = br.inputs(N, spec["J"], spec["Ts"])
    return Z, LR, br.Bank(Z, dict(LR), br.SCALE, rows=_three_row_sets(N))


LARGE_CASES = [pytest.param(N, T, sl, asm, id="N%d-T%d-%d:%d%s" % (N, T, sl[0], sl[1], "" if asm is None else "-asm%d" % asm))
               for N, spec in LARGE.items() for T in spec["Ts"] for sl in spec["slices"] for asm in _asm_modes(N, T, sl)]


@pytest.mark.parametrize("N,T,sl,asm", LARGE_CASES)
def test_f32_large_rows_against_float64(gpu_device, request, N, T, sl, asm):
    """3 x 22 rows of gZ (first, middle, the ragged tail) against float64; gscale against the checksum
    sum(L * (K_slice R)) / scale with K_slice R from ops.mvm_sym on the same slice (oracle-checked in test_kernels_gpu.py),
    as test_headline_oracle_gpu.py::test_bilinear_derivative_rows does."""
    from rpgp_amd import ops
    Z, LR, bank = _bank_rows(N)
    J = Z.shape[1]
    Zd, Ld, Rd = _dev(Z, gpu_device), _dev(LR[T][0], gpu_device), _dev(LR[T][1], gpu_device)
    gZ, gs = _run(lambda: ops.bilinear_grad(Zd, Ld, Rd, br.SCALE, sl[0], sl[1]), asm)
    gZ2, gs2 = _run(lambda: ops.bilinear_grad(Zd, Ld, Rd, br.SCALE, sl[0], sl[1]), asm)
    assert torch.equal(gZ, gZ2) and torch.equal(gs, gs2)
    case = request.node.callspec.id
    st = br.check(gZ.cpu().numpy(), None, bank.ref(T, sl[0], sl[1]), br.C, br.U32, case,
                  outside=None if sl == (0, J) else 0.0)
    _report(case, st)
    KR = ops.mvm_sym(Zd, Rd, br.SCALE, 0.0, sl[0], sl[1])
    gs_chk = float((Ld.double() * KR.double()).sum()) / br.SCALE
    # gscale = 1/2 sum_i rowS_i with rowS_i = sum_t L_it (K R)_it + R_it (K L)_it, itself a float32 sum of N terms of random sign
    # (at N = 192000: gscale = 44 out of rows of +-7).  A sequential float32 sum of N such terms carries a rounding error of
    # about u |sum| sqrt(N / 2) (partial sums grow like sqrt(k), one rounding of relative size u each); over the rows these add
    # in quadrature: 1/2 u sqrt(N / 2) |rowS|_2 for the kernel, as much for the checksum's product.  That stands where the C4
    # test has its absolute 1e-4: tolerances of 0.06 at N = 192000 and 0.03 .. 0.1 at N = 16500 in all, against differences of 0.007 and <= 0.0009 measured
    # on an MI355X (the kernels sum in splits and slabs, hence better) — and 38, what a dropped 512-row block moves gscale by.
    KL = ops.mvm_sym(Zd, Ld, br.SCALE, 0.0, sl[0], sl[1])
    rowS = ((Ld.double() * KR.double()).sum(1) + (Rd.double() * KL.double()).sum(1)) / br.SCALE
    tol = 2e-5 * abs(gs_chk) + br.U32 * math.sqrt(N / 2.0) * float(rowS.norm())
    print("ARM %s gscale %.9g checksum %.9g difference %.3g tolerance %.3g" % (case, float(gs), gs_chk, abs(float(gs) - gs_chk), tol))
    assert abs(float(gs) - gs_chk) < tol


# ---- row strides of the C-ABI: ldz = 10 (NaN in the padding), ldg = 12 (sentinel-filled) ---------------------------------
@functools.lru_cache(maxsize=None)
def _bank_strided(N):
    Z, LR = br.inputs(N, br.STRIDED_J, [br.STRIDED_T], seed=N + 7)
    return Z, LR, br.Bank(Z, dict(LR), br.SCALE)


@pytest.mark.parametrize("sl", br.STRIDED_SLICES, ids=lambda s: "%d:%d" % s)
@pytest.mark.parametrize("N", br.STRIDED_N)
def test_f32_strided_c_abi(gpu_device, request, N, sl):
    from rpgp_amd import ops, _lib
    lib = _lib.load()
    Z, LR, bank = _bank_strided(N)
    J, T, ldz, ldg = br.STRIDED_J, br.STRIDED_T, 10, 12
    Zbuf = torch.full((N, ldz), float("nan"), device=gpu_device)
    Zbuf[:, :J] = _dev(Z, gpu_device)
    Ld, Rd = _dev(LR[T][0], gpu_device), _dev(LR[T][1], gpu_device)
    ws = ops._workspace(gpu_device, lib.rpgp_bilinear_grad_workspace_bytes(N, sl[1] - sl[0]))
    outs = []
    for _ in range(2):
        gbuf = torch.full((N, ldg), SENTINEL, device=gpu_device)
        gs = torch.full((), SENTINEL, device=gpu_device)
        _lib.check(lib.rpgp_bilinear_grad(Zbuf.data_ptr(), Ld.data_ptr(), Rd.data_ptr(), gbuf.data_ptr(), gs.data_ptr(), N,
                                          ldz, ldg, T, sl[0], sl[1], br.SCALE, ws.data_ptr(), ws.numel(), ops._stream()),
                   "rpgp_bilinear_grad")
        outs.append((gbuf, gs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    got = outs[0][0].cpu().numpy()
    assert not np.isnan(got).any() and not np.isnan(float(outs[0][1]))
    case = "strided-N%d-%d:%d" % (N, sl[0], sl[1])
    st = br.check(got, float(outs[0][1]), bank.ref(T, sl[0], sl[1]), br.C, br.U32, case, outside=np.float32(SENTINEL))
    _report(case, st)


# ---- dense-weight form, both precisions -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bank_dense(f64):
    dt = np.float64 if f64 else np.float32
    Z, _ = br.inputs(br.DENSE_N, 20, [], dtype=dt)
    S = br.symmetric_weights(br.DENSE_N, br.DENSE_N, dtype=dt)
    return Z, S, br.Bank(Z, {"S": S}, br.SCALE, precise=f64)


@pytest.mark.parametrize("sl", br.S1 + br.S4, ids=lambda s: "%d:%d" % s)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_dense_weight_form(gpu_device, f64, sl):
    from rpgp_amd import ops
    Z, S, bank = _bank_dense(f64)
    Zd, Sd = _dev(Z, gpu_device), _dev(S, gpu_device)
    gZ, gs = ops.bilinear_grad_dense(Zd, Sd, br.SCALE, sl[0], sl[1])
    if not f64:                                                    # (the float64 path adds atomically)
        gZ2, gs2 = ops.bilinear_grad_dense(Zd, Sd, br.SCALE, sl[0], sl[1])
        assert torch.equal(gZ, gZ2) and torch.equal(gs, gs2)
    case = "dense-%s-N%d-%d:%d" % ("f64" if f64 else "f32", br.DENSE_N, sl[0], sl[1])
    st = br.check(gZ.cpu().numpy(), float(gs), bank.ref("S", sl[0], sl[1]), br.C, br.U64 if f64 else br.U32, case,
                  outside=None if sl == (0, 20) else 0.0)
    _report(case, st)


# ---- the float64 derivative: J = 35 = pieces 20 + 8 + 4 + 2 + 1, TT = 4 and 12, T in passes, column splits of two tiles --
F64 = {300: dict(J=35, Ts=[1, 4, 5, 13, 16], slices=[(0, 35), (3, 11)]), 4200: dict(J=7, Ts=[5], slices=[(0, 7)])}


@functools.lru_cache(maxsize=None)
def _bank_f64(N):
    spec = F64[N]
    Z, LR = br.inputs(N, spec["J"], spec["Ts"], dtype=np.float64)
    return Z, LR, br.Bank(Z, dict(LR), br.SCALE, precise=True)     # sums in extended precision: the kernels' peer otherwise


@pytest.mark.parametrize("N,T,sl", [pytest.param(N, T, sl, id="f64-N%d-T%d-%d:%d" % (N, T, sl[0], sl[1]))
                                    for N, spec in F64.items() for T in spec["Ts"] for sl in spec["slices"]])
def test_f64_derivative(gpu_device, request, N, T, sl):
    from rpgp_amd import ops
    Z, LR, bank = _bank_f64(N)
    gZ, gs = ops.bilinear_grad(_dev(Z, gpu_device), _dev(LR[T][0], gpu_device), _dev(LR[T][1], gpu_device), br.SCALE,
                               sl[0], sl[1])
    assert gZ.dtype == torch.float64
    case = request.node.callspec.id
    st = br.check(gZ.cpu().numpy(), float(gs), bank.ref(T, sl[0], sl[1]), br.C, br.U64, case,
                  outside=None if sl == (0, Z.shape[1]) else 0.0)
    _report(case, st)


# ---- related arms of the same files at the project's per-column 2-norm gates --------------------------------------------
def _col_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)).max())


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("M,N", [(97, 2300), (1, 50)])
def test_rect_product_and_dense_block_slices(gpu_device, M, N, f64):
    """ops.mvm_rect and ops.dense on the slices S1 of a J = 20 pair against oracle.dense_gp.mvm / additive_rbf on the sliced
    columns."""
    from rpgp_amd import ops
    dt = np.float64 if f64 else np.float32
    gate = 1e-12 if f64 else 1e-5
    rng = np.random.default_rng(M + N)
    Z1 = (0.8 * rng.standard_normal((M, 20))).astype(dt)
    Z2 = (0.8 * rng.standard_normal((N, 20))).astype(dt)
    V = rng.standard_normal((N, 3)).astype(dt)
    Z1d, Z2d, Vd = _dev(Z1, gpu_device), _dev(Z2, gpu_device), _dev(V, gpu_device)
    for j0, j1 in br.S1:
        out = ops.mvm_rect(Z1d, Z2d, Vd, br.SCALE, j0, j1).cpu().numpy()
        e1 = _col_err(out, orc.mvm(Z1[:, j0:j1], Z2[:, j0:j1], V, br.SCALE))
        Kd = ops.dense(Z1d, Z2d, br.SCALE, j0, j1).cpu().numpy()
        e2 = _col_err(Kd, br.SCALE * orc.additive_rbf(Z1[:, j0:j1], Z2[:, j0:j1]))
        print("ARM rect M%d N%d %s %d:%d product %.2e block %.2e" % (M, N, "f64" if f64 else "f32", j0, j1, e1, e2))
        assert e1 < gate and e2 < gate, (j0, j1, e1, e2)


@functools.lru_cache(maxsize=None)
def _f64_product_problem():
    N, J = 4200, 35
    rng = np.random.default_rng(N + J)
    Z = 0.8 * rng.standard_normal((N, J))
    V = rng.standard_normal((N, 16))
    # rows in every 256-row block class: first, around the block boundary 2048, the ragged tail, a seeded spread
    rows = np.unique(np.concatenate([np.arange(0, 22), np.arange(2037, 2059), np.arange(N - 22, N),
                                     rng.choice(N, size=64, replace=False)]))
    return Z, V, rows, orc.additive_rbf(Z[rows], Z), orc.additive_rbf(Z[:1] + 0.25, Z)


@pytest.mark.parametrize("T", [3, 13, 16])
def test_f64_product_t_pieces_and_column_splits(gpu_device, T):
    """rpgp_mvm_f64 with J = 35 (pieces 20 + 8 + 4 + 2 + 1), T in pieces 12 / 4 / 1 and column splits of two 64-column tiles
    (N = 4200): the square operator with noise on 150 rows, the rectangular one with M = 1."""
    from rpgp_amd import ops
    Z, V, rows, K, K1 = _f64_product_problem()
    V = np.ascontiguousarray(V[:, :T])
    Zd, Vd = _dev(Z, gpu_device), _dev(V, gpu_device)
    out = ops.mvm_sym(Zd, Vd, 0.3, 0.2).cpu().numpy()
    e1 = _col_err(out[rows], 0.3 * (K @ V) + 0.2 * V[rows])
    outr = ops.mvm_rect(_dev(Z[:1] + 0.25, gpu_device), Zd, Vd, 0.3).cpu().numpy()
    e2 = _col_err(outr, 0.3 * (K1 @ V))
    print("ARM f64 product T%d square %.2e rectangular %.2e" % (T, e1, e2))
    assert e1 < 1e-12 and e2 < 1e-12
