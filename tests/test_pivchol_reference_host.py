"""Host checks of tests/pivchol_reference.py (no GPU): the column providers are the oracle's matrices; the float32
restatement of the greedy loop passes the step-by-step checker on the inputs of every case of
tests/test_pivchol_steps_gpu.py (cases above 70 000 rows: the same generator at 4 099 rows), which is where the constants of
the entrywise gate are measured, per operator kind (c_ref = the restatement's largest |l - ref| / (u B) over the main
cases; the GPU tests use 16 c_ref rounded up to a power of two, at most 256); every main case is resolved from the
reference side alone (smallest d_p / d0 >= 1e-2, no skipped step); the checker's mutation self-test: six defects a
factorisation kernel could have, each of which must fire its gate with a figure above 4 C; and the float64 oracle factor
and the generic float32 greedy loop of the product (`precond.pivoted_cholesky`, CPU tensors) pass the same checker."""
import functools

import numpy as np
import pytest

from oracle import dense_gp as orc
from oracle import family as fam_oracle
from oracle import ski as sko
from tests import pivchol_reference as pr

CASES = pr.cases()
KINDS = ("rbf", "family", "grid")


@functools.lru_cache(maxsize=None)
def _restated(case_id):
    """(case, provider, scale, restated L, records) of one case at its host size."""
    case = next(c for c in CASES if c["id"] == case_id)
    Z, scale = pr.inputs(case["N"], case["J"], host=True)
    prov = pr.provider_of(case, Z)
    L = pr.restate_f32(prov, scale, case["rank"])
    return case, prov, scale, L, pr.check(L, prov, scale, case=case_id)


@pytest.mark.parametrize("case_id", [c["id"] for c in CASES])
def test_restatement_passes_the_checker_and_main_cases_are_resolved(case_id):
    """restate_f32 passes `check` at the constant in use; a main case has no step below d_p / d0 = 1e-2 and none skipped."""
    case, prov, scale, L, records = _restated(case_id)
    assert pr.C[prov.name] <= pr.C_CAP
    worst, dmin, skipped = pr.summary(records)
    print("%s: largest ratio %.3f, smallest d_p/d0 %.3e, skipped %.2f" % (case_id, worst, dmin, skipped))
    pr.assert_resolved(case, records)        # (2305, 1, 16): eight resolved steps, then the single 1-D RBF is used up
    assert case["main"] == (case["live"] == min(case["rank"], prov.N))
    if prov.N < case["rank"]:
        assert all(r["exhausted"] for r in records[prov.N:]) and not L[:, prov.N:].any()


def test_c_ref_gives_the_constants_in_use():
    """c_ref per operator kind over the main cases (7.28 / 4.92 / 1.84 where this was written; they move in the second
    digit with the CPU's exp2 and cos): 16 c_ref rounded up to a power of two is the constant the GPU tests use, at most 256."""
    c_ref = dict.fromkeys(KINDS, 0.0)
    for c in CASES:
        case, prov, scale, L, records = _restated(c["id"])
        if case["main"]:
            c_ref[prov.name] = max(c_ref[prov.name], pr.summary(records)[0])
    print("c_ref = %r" % (c_ref,))
    for kind in KINDS:
        assert pr.c_from(c_ref[kind]) == pr.C[kind] <= pr.C_CAP, (kind, c_ref[kind])


# ---- the providers are the oracle's matrices ---------------------------------------------------------------------------
def test_exact_and_family_providers_are_the_oracle():
    rng = np.random.default_rng(3)
    Z = (0.8 * rng.standard_normal((90, 8))).astype(np.float32)
    K = orc.additive_rbf(Z.astype(np.float64), Z.astype(np.float64))
    prov = pr.FamilyProvider(Z)
    assert prov.name == "rbf" and np.array_equal(prov.diag()[0], np.full(90, 8.0))
    for p in (0, 41, 89):
        k, s = prov.column(p)
        assert np.abs(k - K[:, p]).max() <= 1e-14 * 8 and (s >= np.abs(k)).all()
    for kind, group in [("Matern", 1), ("InverseMQ", 1), ("Cosine", 1), ("RBF", 2), ("RBF", 4)]:
        w = pr.family_weights(8 // group, 5)
        prov = pr.FamilyProvider(Z, kind, group, w)
        K = fam_oracle.kernel_matrix(Z, Z, kind, group, w)
        assert prov.name == "family" and np.abs(prov.diag()[0] - np.diag(K)).max() <= 1e-14
        for p in (0, 41, 89):
            k, s = prov.column(p)
            assert np.abs(k - K[:, p]).max() <= 1e-14 * 8 and (s >= np.abs(k) * (1 - 1e-15)).all()
    # |t phi'(t)| of every kind against a central difference of the oracle's phi
    t = np.linspace(0.05, 3.0, 60)
    for kind in fam_oracle.KINDS:
        num = t * (fam_oracle._phi(kind, (t + 1e-6) ** 2) - fam_oracle._phi(kind, (t - 1e-6) ** 2)) / 2e-6
        assert np.abs(pr._phi_sens(kind, t) - np.abs(fam_oracle._phi(kind, t * t)) - np.abs(num)).max() < 1e-7


@pytest.mark.parametrize("kind,rule,weighted", [("RBF", "shared", False), ("Matern", "shared", True), ("RBF", "reference", True),
                                                ("Cosine", "reference", False)])
def test_grid_provider_is_the_dense_ski_oracle(kind, rule, weighted):
    rng = np.random.default_rng(11)
    N, J, G = 120, 3, 64
    Z = (rng.standard_normal((N, J)) * np.linspace(0.5, 1.5, J)).astype(np.float32)
    grid = pr.host_grid_block(Z, G, rule)
    w = pr.grid_weights(J) if weighted else None
    prov = pr.GridProvider(Z, grid, G, kind, w)
    g64 = (grid[0].astype(np.float64), grid[1].astype(np.float64))
    # the oracle's dense pieces, put together as the kernels define the operator: taps at (z - g0) * (1/h) with the grid
    # block's own 1/h, Toeplitz lags lag * h
    K = np.zeros((N, N))
    for j in range(J):
        Wj = sko.interp_matrix(Z[:, j], g64[0][j], 1.0 / float(grid[2][j]), G)
        K += (1.0 if w is None else float(w[j])) * (Wj @ sko.toeplitz(g64[1][j], G, kind) @ Wj.T)
    d, ds = prov.diag()
    assert np.abs(d - np.diag(K)).max() <= 1e-13 * J
    # oracle.ski.dense_kernel / diag_sparse divide by h instead: the same operator up to the rounding of the block's 1/h, one
    # relative u on every tap position — which the sensitivity covers (it allows two)
    Kh = sko.dense_kernel(Z, Z, 1.0, G, g64, w, kind)
    assert (np.abs(d - sko.diag_sparse(Z, 1.0, G, g64, w, kind)) <= pr.U32 * ds).all()
    assert (np.abs(d - np.diag(Kh)) <= pr.U32 * ds).all()
    for p in (0, 57, N - 1):
        k, s = prov.column(p)
        assert np.abs(k - K[:, p]).max() <= 1e-13 * J and (np.abs(k - Kh[:, p]) <= pr.U32 * s).all()
        assert (s >= np.abs(k)).all() and abs(s[p] - ds[p]) <= 1e-10 * ds[p]      # the diagonal's sensitivity is the column's
    # the float32 restatement of the entries and of the diagonal is the same operator
    assert np.abs(prov.diag_f32(0.5) - 0.5 * d).max() <= pr.U32 * 0.5 * ds.max()
    assert np.abs(prov.column_f32(57, 0.5) - 0.5 * K[:, 57]).max() <= pr.U32 * 0.5 * prov.column(57)[1].max()


# ---- other factorisations of the same matrices pass the same checker -----------------------------------------------------
def test_float64_oracle_factor_passes_with_nothing_to_spare():
    """oracle.dense_gp.pivoted_cholesky of the float64 matrix: every ratio is float64 rounding (below 1e-6 of a unit)."""
    for case_id in ("one_workgroup-N1024-J20-r15", "family-Matern-g1-c6-N300-r17", "grid_row_major-N3000-J3-r15-G256-RBF-shared"):
        case, prov, scale, _, _ = _restated(case_id)
        if prov.N > 1100:
            Z = prov.Z32[:700]
            prov = pr.provider_of(case, Z, None if case["op"] != "grid" else (prov.g0, prov.h, prov.inv_h))
        K = float(np.float32(scale)) * np.stack([prov.column(p)[0] for p in range(prov.N)], axis=1)
        L, piv = orc.pivoted_cholesky(K, case["rank"])
        records = pr.check(L, prov, scale, case=case_id)
        assert [r["pivot"] for r in records] == piv
        assert pr.summary(records)[0] < 1e-6


def test_generic_greedy_loop_of_the_product_passes(oracle_backend):
    """precond.pivoted_cholesky on CPU tensors (rows from the CPU test double): float32, and float64 (whose only error is
    the scale, which `check` rounds to float32 as the C entry points take it: below one unit)."""
    import torch
    from rpgp_amd.operators import AdditiveRPOperator
    from rpgp_amd.precond import pivoted_cholesky
    Z, scale = pr.inputs(1024, 20)
    prov = pr.FamilyProvider(Z)
    for dtype, limit in [(torch.float32, pr.C["rbf"]), (torch.float64, 1.0)]:
        op = AdditiveRPOperator(torch.from_numpy(Z).to(dtype), None, torch.tensor(0.8, dtype=dtype), weight=1.0 / 20)
        L = pivoted_cholesky(op._diagonal(), op._get_rows, 15)
        assert L.dtype == dtype
        records = pr.check(L.numpy(), prov, scale, case="generic-%s" % dtype)
        print("generic loop, %s: largest ratio %.3g" % (dtype, pr.summary(records)[0]))
        assert pr.summary(records)[0] <= limit


# ---- the checker's mutation self-test ------------------------------------------------------------------------------------
MUT_CASE = "fast_step-N2049-J20-r15"


def _fired(L, prov, scale, c=None):
    with pytest.raises(pr.CheckFailure) as ei:
        pr.check(L, prov, scale, c=c, case="mutation")
    print(ei.value)
    assert str(ei.value).startswith("mutation: ")
    return set(ei.value.gates), ei.value.ratios


def test_mutation_one_stale_row():
    """One row of the last column holds its neighbour's value."""
    _, prov, scale, L, _ = _restated(MUT_CASE)
    L = L.copy()
    L[1000, -1] = L[1001, -1]
    gates, ratios = _fired(L, prov, scale)
    assert gates == {"entry"} and ratios["entry"] > 4 * pr.C["rbf"]


def test_mutation_last_term_of_the_correction_sum_dropped():
    _, prov, scale, _, _ = _restated(MUT_CASE)
    L = pr.restate_f32(prov, scale, 15, mutate={"drop_last_corr": 14})
    gates, ratios = _fired(L, prov, scale)
    assert "entry" in gates and ratios["entry"] > 4 * pr.C["rbf"]


def test_mutation_two_columns_swapped():
    """Columns 6 and 9 exchanged: step 6 then takes a pivot that is not the largest residual, from a column that holds
    three corrections too many."""
    _, prov, scale, L, _ = _restated(MUT_CASE)
    L = L.copy()
    L[:, [6, 9]] = L[:, [9, 6]]
    gates, ratios = _fired(L, prov, scale)
    assert {"greedy", "entry"} <= gates and ratios["entry"] > 4 * pr.C["rbf"] and ratios["greedy"] > 4 * pr.C["rbf"]


def test_mutation_kernel_row_taken_one_row_off():
    """Step 7 evaluates K(i, pivot + 1): the largest entry of the column is then not the square root of its row's residual."""
    _, prov, scale, _, _ = _restated(MUT_CASE)
    L = pr.restate_f32(prov, scale, 15, mutate={"row_off": 7})
    gates, ratios = _fired(L, prov, scale)
    assert {"pivot", "entry"} <= gates and ratios["entry"] > 4 * pr.C["rbf"]


@pytest.mark.parametrize("kind", ["Matern", "Cosine"])
def test_mutation_family_kind_with_the_rbf_prescale(kind):
    """pivchol_pre returning the RBF's sqrt(log2(e) / 2) for another kind."""
    case_id = next(c["id"] for c in CASES if c["op"] == "family" and c["kind"] == kind and c["N"] == 300)
    case, prov, scale, _, _ = _restated(case_id)
    bad = pr.FamilyProvider(prov.Z32, case["kind"], case["group"], prov.w32, pre=pr.PRE["RBF"])
    L = pr.restate_f32(bad, scale, case["rank"])
    gates, ratios = _fired(L, prov, scale)
    assert "entry" in gates and ratios["entry"] > 4 * pr.C["family"]


def test_mutation_second_best_pivot():
    """Step 5 takes the second-largest residual diagonal entry and everything else is done right: the column is the right
    one for that pivot, so only the greedy gate can see it (the gap there is 1e-2 d0, the bound 1e-6 d0)."""
    _, prov, scale, _, _ = _restated(MUT_CASE)
    L = pr.restate_f32(prov, scale, 15, mutate={"second_best": 5})
    gates, ratios = _fired(L, prov, scale)
    assert gates == {"greedy"} and ratios["greedy"] > 4 * pr.C["rbf"]


@pytest.mark.parametrize("case_id", ["grid_row_major-N3000-J3-r15-G256-RBF-shared", "grid_row_major-N3000-J5-r17-G256-RBF-shared",
                                     "grid_fast-N65536-J3-r16-G512-RBF-shared", "grid_column_major-N65537-J3-r17-G512-RBF-shared"])
def test_mutations_of_the_grid_operator(case_id):
    """The grid operator's entry bound is the widest (float32 tap positions, widest at G = 512); the dropped last correction
    term and the kernel row one row off still fire the entry gate with figures above 4 C, and a second-best pivot fires the
    greedy gate — the same derived bound as for the exact operator — at an early, a middle and the last step."""
    case, prov, scale, _, _ = _restated(case_id)
    rank = case["rank"]
    gates, ratios = _fired(pr.restate_f32(prov, scale, rank, mutate={"drop_last_corr": rank - 1}), prov, scale)
    assert "entry" in gates and ratios["entry"] > 4 * pr.C["grid"]
    gates, ratios = _fired(pr.restate_f32(prov, scale, rank, mutate={"row_off": 7}), prov, scale)
    assert {"pivot", "entry"} <= gates and ratios["entry"] > 4 * pr.C["grid"]
    for m in (2, rank // 2, rank - 1):
        gates, ratios = _fired(pr.restate_f32(prov, scale, rank, mutate={"second_best": m}), prov, scale)
        assert gates == {"greedy"} and ratios["greedy"] > 4 * pr.C["grid"], m


def test_mutations_of_the_contract():
    """A repeated pivot, a non-zero column after the last row has been a pivot, and a NaN each fire their own gate."""
    _, prov, scale, L, _ = _restated(MUT_CASE)
    rep = L.copy()
    rep[:, 9] = rep[:, 4]
    assert "repeat" in _fired(rep, prov, scale)[0]
    bad = L.copy()
    bad[77, 3] = np.nan
    assert _fired(bad, prov, scale)[0] == {"nan"}
    case, sp, sscale, Ls, _ = _restated("one_workgroup-N5-J3-r8")
    Ls = Ls.copy()
    Ls[2, 6] = 1e-30
    assert _fired(Ls, sp, sscale)[0] == {"zero"}
    with pytest.raises(ValueError):
        pr.check(L, prov, scale, c=512.0)
