"""Host checks of tests/bilinear_reference.py (no GPU): the float32 restatement of the bilinear derivative passes the
checker at every case of tests/test_bilinear_arms_gpu.py with N <= 2300, which is where the constant of the entrywise
gate is measured (c_ref = the restatement's largest |restate - ref| / (u B); the GPU tests use 16 c_ref rounded up to a
power of two, at most 64); the row-subset reference is the full one; and the checker's mutation self-test: six defects
a kernel arm could have, each of which must make `check` fail — with the gates that fire asserted, so that what only the
entrywise gate sees is visible."""
import functools

import numpy as np
import pytest

from oracle import dense_gp as orc
from tests import bilinear_reference as br

GROUPS = ["N300", "N2047", "N2048", "N2300", "strided", "dense"]


@functools.lru_cache(maxsize=None)
def _group(name):
    """[(case id, Ref, restated gZ, restated gscale)] of one group of cases."""
    out = []
    if name.startswith("N"):
        N = int(name[1:])
        table = br.F32_TABLE[N]
        Z, LR = br.inputs(N, 20, list(table))
        bank = br.Bank(Z, dict(LR), br.SCALE)
        rb = br.RestateBank(Z, dict(LR), br.SCALE)
        for T, slices in table.items():
            for j0, j1 in slices:
                out.append((("N%d-T%d-%d:%d" % (N, T, j0, j1)), bank.ref(T, j0, j1)) + rb.get(T, j0, j1))
    elif name == "strided":
        for N in br.STRIDED_N:
            Z, LR = br.inputs(N, br.STRIDED_J, [br.STRIDED_T], seed=N + 7)
            bank = br.Bank(Z, dict(LR), br.SCALE)
            rb = br.RestateBank(Z, dict(LR), br.SCALE)
            for j0, j1 in br.STRIDED_SLICES:
                out.append((("strided-N%d-%d:%d" % (N, j0, j1)), bank.ref(br.STRIDED_T, j0, j1)) + rb.get(br.STRIDED_T, j0, j1))
    else:
        Z, _ = br.inputs(br.DENSE_N, 20, [])
        S = br.symmetric_weights(br.DENSE_N, br.DENSE_N)
        bank = br.Bank(Z, {"S": S}, br.SCALE)
        rb = br.RestateBank(Z, {"S": S}, br.SCALE)
        for j0, j1 in br.S1 + br.S4:
            out.append((("dense-N%d-%d:%d" % (br.DENSE_N, j0, j1)), bank.ref("S", j0, j1)) + rb.get("S", j0, j1))
    return out


@pytest.mark.parametrize("name", GROUPS)
def test_restatement_passes_the_checker(name):
    """restate_f32 passes `check` at the constant in use (c = 16 c_ref rounded up to a power of two, at most 64); its own
    largest ratio stays within the 4 that c_ref may reach."""
    assert br.C <= br.C_CAP
    worst = 0.0
    for case, ref, g, gs in _group(name):
        st = br.check(g, gs, ref, br.C, br.U32, case)
        worst = max(worst, st["ratio"], st["gs_ratio"])
    print("%s: largest ratio of the restatement %.3f" % (name, worst))
    assert worst <= br.C_REF_CAP, (name, worst)


def test_c_ref_gives_the_constant_in_use():
    """c_ref over ALL the cases (3.64 where this was written; it moves in the second digit with the CPU's exp2 and sgemm):
    at most 4, and 16 c_ref rounded up to a power of two is the constant the GPU tests use."""
    c_ref = max(max(br.ratios(g, ref, br.U32).max(), abs(float(gs) - ref.gs) / (br.U32 * ref.Bs))
                for name in GROUPS for _, ref, g, gs in _group(name))
    print("c_ref = %.4f" % c_ref)
    assert c_ref <= br.C_REF_CAP
    assert br.c_from(c_ref) == br.C <= br.C_CAP


def test_plain_float64_sums_are_within_one_unit_of_the_extended_ones():
    """The reference of the float32 cases sums in plain float64 (einsum); against sums in extended precision that is a
    ratio below 2 u64 B even at the largest full-matrix size, N = 4200 (u64 = 2^-29 u32)."""
    Z, LR = br.inputs(4200, 7, [5], dtype=np.float64)
    rows = np.concatenate([np.arange(0, 22), np.arange(2089, 2111), np.arange(4178, 4200)])
    plain = br.reference(Z, LR[5][0], LR[5][1], br.SCALE, 0, 7, rows=rows)
    exact = br.reference(Z, LR[5][0], LR[5][1], br.SCALE, 0, 7, rows=rows, precise=True)
    r = br.ratios(plain.gZ, exact, br.U64).max()
    print("plain against extended sums: %.3f u64 B" % r)
    assert r <= 2.0


def test_reference_is_the_oracle_and_the_bank_is_the_reference():
    N, T = 700, 5
    Z, LR = br.inputs(N, 20, [T])
    L, R = LR[T]
    bank = br.Bank(Z, {T: (L, R)}, br.SCALE)
    for j0, j1 in [(0, 20), (7, 14), (5, 6)]:
        ref = br.reference(Z, L, R, br.SCALE, j0, j1)
        gZ, gs = orc.bilinear_grad(Z[:, j0:j1].astype(np.float64), L, R, br.SCALE)
        assert np.array_equal(ref.gZ, gZ) and ref.gs == gs
        b = bank.ref(T, j0, j1)
        assert np.abs(b.gZ - ref.gZ).max() <= 1e-13 * ref.B.max() and abs(b.gs - ref.gs) <= 1e-13 * ref.Bs
        assert np.array_equal(b.B, ref.B) and b.Bs == ref.Bs
        # the bound bounds: |value| <= B, and it is the sum of |terms| formed independently here for one column
        assert (np.abs(ref.gZ) <= ref.B).all() and abs(ref.gs) <= ref.Bs
        p = br.reference(Z, L, R, br.SCALE, j0, j1, precise=True)
        assert np.abs(p.gZ - ref.gZ).max() <= 1e-13 * ref.B.max() and abs(p.gs - ref.gs) <= 1e-13 * ref.Bs
    Zd, Ld, Rd = Z.astype(np.float64), L.astype(np.float64), R.astype(np.float64)
    j = 9
    d = Zd[:, j][:, None] - Zd[:, j][None, :]
    terms = sum(np.abs(Ld[:, t][:, None] * Rd[:, t][None, :]) + np.abs(Rd[:, t][:, None] * Ld[:, t][None, :]) for t in range(T))
    Bj = br.SCALE * (terms * np.exp(-0.5 * d * d) * np.abs(d)).sum(axis=1)
    assert np.abs(bank.ref(T, j, j + 1).B[:, 0] - Bj).max() <= 1e-13 * Bj.max()
    # the explicit-S form with S = L R^T + R L^T is the factor form
    S = Ld @ Rd.T + Rd @ Ld.T
    rd = br.reference_dense(Z, S, br.SCALE, 7, 14)
    ref = br.reference(Z, L, R, br.SCALE, 7, 14)
    assert np.abs(rd.gZ - ref.gZ).max() <= 1e-13 * ref.B.max() and abs(rd.gs - ref.gs) <= 1e-13 * ref.Bs
    assert (rd.B <= ref.B * (1 + 1e-13)).all()                     # |S| <= the factor form's bound of it


def test_row_subset_reference_equals_the_full_one():
    N, T = 2300, 11
    Z, LR = br.inputs(N, 20, [T])
    full = _group("N2300")
    rows = np.concatenate([np.arange(0, 22), np.arange(1139, 1161), np.arange(N - 22, N)])
    for j0, j1 in [(7, 14), (0, 20)]:
        ref = next(r for case, r, _, _ in full if case == "N2300-T11-%d:%d" % (j0, j1))
        sub = br.reference(Z, LR[T][0], LR[T][1], br.SCALE, j0, j1, rows=rows)
        assert sub.gs is None and sub.gZ.shape == (66, j1 - j0)
        assert np.abs(sub.gZ - ref.gZ[rows]).max() <= 1e-12 * np.abs(ref.gZ).max()
        assert np.abs(sub.B - ref.B[rows]).max() <= 1e-12 * ref.B.max()
        # `check` with a row-subset reference picks the rows out of a whole result
        g = next(g for case, _, g, _ in full if case == "N2300-T11-%d:%d" % (j0, j1))
        br.check(g, None, sub, br.C, br.U32, "rows")


# ---- the checker's mutation self-test: N = 2300, slice (7, 14), T = 11 -----------------------------------------------
MUT_T, MUT_J0, MUT_J1 = 11, 7, 14


@pytest.fixture(scope="module")
def mut():
    full = {case: (ref, g, gs) for case, ref, g, gs in _group("N2300")}
    ref, g, gs = full["N2300-T%d-%d:%d" % (MUT_T, MUT_J0, MUT_J1)]
    prev = full["N2300-T%d-0:7" % MUT_T][1]
    whole = np.zeros((2300, 20), dtype=np.float32)                # as `ops` hands it back: zero outside the slice
    whole[:, MUT_J0:MUT_J1] = g
    br.check(whole, gs, ref, br.C, br.U32, "unmutated", outside=0.0)
    Z, LR = br.inputs(2300, 20, [MUT_T])
    return {"ref": ref, "whole": whole, "gs": gs, "prev": prev, "Z": Z.astype(np.float64),
            "L": LR[MUT_T][0].astype(np.float64), "R": LR[MUT_T][1].astype(np.float64)}


def _fired(mut, whole, gs):
    with pytest.raises(br.CheckFailure) as ei:
        br.check(whole, gs, mut["ref"], br.C, br.U32, "mutation", outside=0.0)
    print(ei.value)
    assert str(ei.value).startswith("mutation: ")                  # the message names the case
    return set(ei.value.gates)


@pytest.mark.parametrize("target,gates", [(None, {"norm", "column", "entry"}), (110.0, {"entry"})])
def test_mutation_one_dropped_pair(mut, target, gates):
    """The contribution of one column c to one row is missing.  A term of median size in that row is about B / N = 1400 u B
    here: at this size the 2-norm gates see it too (the row's value is about B / 200, so the one entry moves by 2 %).  The
    term of that row whose largest |term| / (u B) over the seven columns is nearest 110 — about its 2 % quantile — passes
    both 2-norm gates (the per-column one fires from about 180): only the entrywise gate, at 64, fires."""
    i = 1000
    Z, L, R = mut["Z"], mut["L"], mut["R"]
    S = L[i] @ R.T + R[i] @ L.T
    d = Z[i, MUT_J0:MUT_J1][None, :] - Z[:, MUT_J0:MUT_J1]
    terms = -br.SCALE * S[:, None] * np.exp(-0.5 * d * d) * d                       # N x 7
    if target is None:
        c = int(np.argsort(np.abs(terms[:, 0]))[len(terms) // 2])
    else:
        size = (np.abs(terms) / (br.U32 * mut["ref"].B[i])).max(axis=1)
        c = int(np.argmin(np.abs(size - target)))
        assert abs(size[c] - target) < 5.0
    whole = mut["whole"].copy()
    whole[i, MUT_J0:MUT_J1] -= terms[c].astype(np.float32)
    assert _fired(mut, whole, mut["gs"]) == gates


def test_mutation_stale_ragged_rows(mut):
    """The last 60 rows (the ragged last subtile: 2300 = 35 * 64 + 60) keep the previous slice's values."""
    whole = mut["whole"].copy()
    whole[-60:, MUT_J0:MUT_J1] = mut["prev"][-60:]
    assert _fired(mut, whole, mut["gs"]) == {"norm", "column", "entry"}


def test_mutation_adjacent_columns_exchanged(mut):
    whole = mut["whole"].copy()
    whole[:, [9, 10]] = whole[:, [10, 9]]
    assert _fired(mut, whole, mut["gs"]) == {"norm", "column", "entry"}


def test_mutation_one_column_scaled(mut):
    """One column times 1 + 2^-12: 2.4e-4 of that column, 9e-5 of the slice."""
    whole = mut["whole"].copy()
    whole[:, 11] *= np.float32(1.0 + 2.0 ** -12)
    assert _fired(mut, whole, mut["gs"]) == {"norm", "column", "entry"}


def test_mutation_gscale_without_the_last_row_block(mut):
    """gscale summed over the four whole 512-row blocks only."""
    Z, L, R = mut["Z"], mut["L"], mut["R"]
    gs = orc.bilinear_grad(Z[:, MUT_J0:MUT_J1], L, R, br.SCALE)[1]
    W = L[2048:] @ R.T
    k = sum(np.exp(-0.5 * (Z[2048:, j][:, None] - Z[:, j][None, :]) ** 2) for j in range(MUT_J0, MUT_J1))
    assert _fired(mut, mut["whole"], np.float32(gs - (W * k).sum())) == {"gscale"}


def test_mutation_slice_written_one_column_to_the_right(mut):
    """j0 ignored by one column: column 7 stays empty, column 14 is written."""
    whole = np.zeros_like(mut["whole"])
    whole[:, MUT_J0 + 1:MUT_J1 + 1] = mut["whole"][:, MUT_J0:MUT_J1]
    assert _fired(mut, whole, mut["gs"]) == {"norm", "column", "entry", "outside"}
