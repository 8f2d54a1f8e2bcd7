"""Host checks of tests/f64_reference.py (no GPU): the geometry of every case of tests/test_f64_kernels_gpu.py, the constants of
its gates, the mutation table, and the analytic SKI derivative of the test double against central differences.

Constants (`test_constants`, run with -s to see them).  c_ref = largest |restatement - long double| / (u A) over the cases of
the entry point, n_ref = the same for the oracle's numpy float64 form; C = smallest power of two >= 4 max(c_ref, n_ref).
Measured where this was written (they move in the last digit with the CPU's exp and BLAS):

    entry point        c_ref   n_ref   4 x max    C
    mvm                 1.06    2.37      9.47   16
    dense               3.14    4.53     18.11   32
    bilinear            0.21    0.16      0.84    1
    bilinear_dense      0.92    0.56      3.66    4
    project             2.79    2.60     11.16   16
    project_grad        0.36    1.76      7.04    8
    ski                 0.55      -       2.19    4
    ski_scatter         0.31    0.27      1.24    2
    ski_gather          0.35    0.35      1.41    2
    ski_grid_product    0.95    0.77      3.80    4

The ski row has no long-double form: its two sides are the float64 restatement with the kernel's tap rule (position times
1/h) and the dense float64 oracle (position over h), over every form of every case of the GPU module (fr.SKI_SWEEP: the
starred shape with both grid rules, weighted and not, every radial kind; T = 70 at G = 128; N = 1 and (257, 5, 1, 2) at G = 8;
the clamped rows); the largest ratio is the dense block of (257, 5, 1, 2) at G = 8.  Its magnitudes carry the tap position
(tests/f64_reference.py).  The staged entries are measured one by one against long double with the magnitudes their GPU
tests use: the Toeplitz stage (no tap position in it: the kernel's in-order fma chain and numpy's product, per projection and
column), the scatter (kernel tap rule and the oracle's against long-double weights at the long-double position) and the
gather."""
import functools

import numpy as np
import pytest
import torch

from oracle import ski as sko
from tests import f64_reference as fr
from tests.oracle_backend import OracleBackend


# ---- geometry -------------------------------------------------------------------------------------------------------------
def test_geometry_of_the_named_cases():
    g = fr.geometry(4161, 4161, 17, 0, 5)
    print("(4161, 4161, 5, 17):", g)
    assert (g["splits"], g["cps"], g["last_split"], g["last_tile"]) == (33, 128, 65, 1) and g["tiles"] == [2] * 33
    assert g["pieces"] == [4, 1] and g["chunks"] == [12, 5]
    g = fr.geometry(4097, 4097, 1, 0, 2)
    print("(4097, 4097, 2, 1):", g)
    assert g["last_split"] == 1 and g["tiles"][-1] == 1 and g["tiles"][0] == 2 and g["chunks"] == [1]
    g = fr.geometry(2305, 7361, 16, 0, 3)
    print("(2305, 7361, 3, 16):", g)
    assert g["splits"] > 1 and min(g["tiles"][:-1]) >= 2 and g["chunks"] == [12, 4] and g["pieces"] == [2, 1]
    g = fr.geometry(321, 321, 14, 0, 35)
    assert g["pieces"] == [20, 8, 4, 2, 1] and g["chunks"] == [12, 2] and g["last_tile"] == 1
    g = fr.geometry(4161, 130, 1, 0, 3)
    assert g["splits"] == 3 and g["last_split"] == 2
    g = fr.geometry(7, 4500, 13, 0, 8)
    assert g["pieces"] == [8] and g["chunks"] == [12, 1] and g["last_tile"] == 4500 - 70 * 64
    assert fr.geometry(4161, 4161, 17, 0, 5, derivative=True)["chunks"] == [12, 5]
    assert fr.geometry(4097, 4097, 16, 0, 3, derivative=True)["chunks"] == [12, 4]
    assert fr.geometry(65, 65, 13, 0, 2, derivative=True)["chunks"] == [12, 1]
    assert fr.geometry(300, 200, 5, *fr.SLICE)["pieces"] == [4, 2, 1]
    for M, N, J, T in fr.MVM_CASES:
        print((M, N, J, T), fr.geometry(M, N, T, 0, J))
    # the projection's grid-stride loop: more than one element per thread only above 8192 * 256 elements
    assert fr.project_blocks(110000, 20) == (8192, 2) and fr.project_blocks(257, 7)[1] == 1


# ---- the constants ----------------------------------------------------------------------------------------------------------
def _ratio_ld(got, ld, A):
    """|got - ld| / (u A) with the difference taken in long double."""
    err = np.abs(np.asarray(got).astype(fr.LD) - ld).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / (fr.U * np.asarray(A)))
    return float(np.max(r))


@functools.lru_cache(maxsize=None)
def _measure(entry):
    c_ref = n_ref = 0.0
    if entry == "mvm":
        jobs = [fr.mvm_inputs(*c) + (0, None) for c in fr.MVM_CASES]
        jobs.append(fr.mvm_slice_inputs() + (0.0,) + fr.SLICE)
        Zl, Vl = fr.large_coordinate_inputs()
        jobs.append((Zl, Zl, Vl, fr.NOISE, 0, None))
        for Z1, Z2, V, noise, j0, j1 in jobs:
            z1, z2 = Z1[:, j0:j1], Z2[:, j0:j1]
            A, ld = fr.mvm_mag(z1, z2, V, fr.SCALE, noise, long_double=True)
            c_ref = max(c_ref, _ratio_ld(fr.restate_mvm(Z1, Z2, V, fr.SCALE, noise, j0, j1), ld, A))
            n_ref = max(n_ref, _ratio_ld(fr.mvm_ref(z1, z2, V, fr.SCALE, noise), ld, A))
    elif entry == "dense":
        jobs = [fr.dense_inputs(*c) + (0, None) for c in fr.DENSE_CASES] + [fr.mvm_slice_inputs()[:2] + fr.SLICE]
        for Z1, Z2, j0, j1 in jobs:
            A, ld = fr.dense_mag(Z1[:, j0:j1], Z2[:, j0:j1], fr.SCALE, long_double=True)
            c_ref = max(c_ref, _ratio_ld(fr.restate_dense(Z1, Z2, fr.SCALE, j0, j1), ld, A))
            n_ref = max(n_ref, _ratio_ld(fr.dense_ref(Z1[:, j0:j1], Z2[:, j0:j1], fr.SCALE), ld, A))
    elif entry == "bilinear":
        for N, J, T in fr.BILINEAR_CASES:
            Z, L, R = fr.bilinear_inputs(N, J, T)
            A, Ags, g, gs = fr.bilinear_mag(Z, L, R, fr.SCALE, long_double=True)
            rg, rs = fr.restate_bilinear(Z, L, R, fr.SCALE)
            ng, nsc = fr.bilinear_ref(Z, L, R, fr.SCALE)
            c_ref = max(c_ref, _ratio_ld(rg, g, A), _ratio_ld(rs, gs, Ags))
            n_ref = max(n_ref, _ratio_ld(ng, g, A), _ratio_ld(nsc, gs, Ags))
    elif entry == "bilinear_dense":
        for N, J in fr.BILINEAR_DENSE_CASES:
            Z, S = fr.bilinear_dense_inputs(N, J)
            A, Ags, g, gs = fr.bilinear_mag(Z, None, None, fr.SCALE, S=S, long_double=True)
            rg, rs = fr.restate_bilinear_dense(Z, S, fr.SCALE)
            ng, nsc = fr.bilinear_dense_ref(Z, S, fr.SCALE)
            c_ref = max(c_ref, _ratio_ld(rg, g, A), _ratio_ld(rs, gs, Ags))
            n_ref = max(n_ref, _ratio_ld(ng, g, A), _ratio_ld(nsc, gs, Ags))
    elif entry in ("project", "project_grad"):
        for c in fr.PROJECT_CASES:
            X, P, G = fr.project_inputs(*c)
            if entry == "project":
                A, ld = fr.project_mag(X, P, long_double=True)
                c_ref, n_ref = max(c_ref, _ratio_ld(fr.restate_project(X, P), ld, A)), max(n_ref, _ratio_ld(X @ P, ld, A))
            else:
                A, ld = fr.project_grad_mag(X, G, long_double=True)
                c_ref = max(c_ref, _ratio_ld(fr.restate_project_grad(X, G), ld, A))
                n_ref = max(n_ref, _ratio_ld(X.T @ G, ld, A))
    elif entry == "ski_grid_product":
        ob = OracleBackend()
        G, (N, M, J, T) = 16, (130, 33, 3, 3)
        Z, Zs, V, L, R, w = fr.ski_inputs(N, M, J, T)
        for rule in ("shared", "reference"):
            for wt in (None, torch.from_numpy(w)):
                gpn = ob.ski_grid(torch.from_numpy(Z), torch.from_numpy(Zs), G, wt, rule).double().numpy()
                hist = fr.ski_hist_mag(Z, gpn, V, G, True)
                for weighted in (True, False):
                    ref, A, seq, ld = fr.ski_grid_product_forms(hist, gpn, G, weighted, long_double=True)
                    col = lambda got: max(float((np.abs(got[j].astype(fr.LD) - ld[j]).astype(np.float64).max(axis=0)
                                                 / (fr.U * A[j].max(axis=0))).max()) for j in range(J))
                    c_ref, n_ref = max(c_ref, col(seq)), max(n_ref, col(ref))
    elif entry in ("ski_scatter", "ski_gather"):
        ob = OracleBackend()
        G, (N, M, J, T) = 16, (130, 33, 3, 3)
        host, _ = fr.ski_case_inputs("starred", N, M, J, T)
        Zt, Zst = torch.from_numpy(host["Z"]), torch.from_numpy(host["Zs"])
        colr = lambda got, ld, A: float((np.abs(np.asarray(got).astype(fr.LD) - ld).astype(np.float64).max(axis=0)
                                         / (fr.U * A.max(axis=0))).max())
        for rule, weighted in fr.SKI_STAGED:
            gp = ob.ski_grid(Zt, Zst, G, torch.from_numpy(host["w"]) if weighted else None, rule).double()
            gpn = gp.numpy()
            if entry == "ski_scatter":
                for src in ("L", "R", "V"):
                    got, A, ld = fr.ski_scatter_forms(host["Z"], gpn, host[src], G)
                    num = ob.ski_scatter(Zt, gp, torch.from_numpy(host[src]), G).numpy()
                    c_ref = max(c_ref, colr(got.reshape(J * G, -1), ld.reshape(J * G, -1), A.reshape(J * G, -1)))
                    n_ref = max(n_ref, colr(num.reshape(J * G, -1), ld.reshape(J * G, -1), A.reshape(J * G, -1)))
            else:
                H = ob.ski_grid_product(torch.from_numpy(fr.ski_hist_mag(host["Z"], gpn, host["V"], G, True)), gp, G)
                for noise in (0.0, fr.NOISE):
                    got, A, ld = fr.ski_gather_forms(host["Z"], gpn, H.numpy(), host["V"], noise, G)
                    num = ob.ski_gather(Zt, gp, H, torch.from_numpy(host["V"]), fr.SCALE, noise, G).numpy()
                    c_ref, n_ref = max(c_ref, colr(got, ld, A)), max(n_ref, colr(num, ld, A))
    else:
        ob = OracleBackend()
        for case in fr.SKI_SWEEP:
            name, N, M, J, T, G, rule, weighted, kind, forms = case
            host, both = fr.ski_case_inputs(name, N, M, J, T)
            gpn = ob.ski_grid(torch.from_numpy(host["Z"]), torch.from_numpy(host["Zs"]) if both else None, G,
                              torch.from_numpy(host["w"]) if weighted else None, rule, kind).double().numpy()
            oracle, restated = fr.ski_oracle(host, gpn, G, forms), fr.ski_restated(host, gpn, G, forms)
            for label, (ref, A) in oracle.items():
                r = fr.column_ratio(restated[label], ref, A)
                if r > c_ref:
                    c_ref = r
                    print("  ski c_ref %.3f at %s %s" % (r, fr.ski_case_id(case), label))
    return c_ref, n_ref


@pytest.mark.parametrize("entry", sorted(fr.C))
def test_constants(entry):
    """The unmutated restatement (and the oracle's numpy form) pass every gate of every case, and the constant in force is
    the smallest power of two >= 4 x the larger measured ratio."""
    c_ref, n_ref = _measure(entry)
    print("%s: c_ref %.3f, numpy-vs-long-double %.3f, C = %g" % (entry, c_ref, n_ref, fr.C[entry]))
    worst = max(c_ref, n_ref)
    assert 4.0 * worst <= fr.C[entry]
    # the smallest such power of two -- for a figure that may sit a quarter lower on another CPU's exp and BLAS
    assert fr.c_from(worst) == fr.C[entry] or fr.c_from(1.25 * worst) == fr.C[entry]


# ---- the mutation table -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mvm_case(case):
    """(Z1, Z2, V, noise, j0, j1, reference, A) of a product case, computed once."""
    if case == "slice":
        Z1, Z2, V = fr.mvm_slice_inputs()
        noise, (j0, j1) = 0.0, fr.SLICE
    else:
        Z1, Z2, V, noise = fr.mvm_inputs(*case)
        j0, j1 = 0, Z1.shape[1]
    z1, z2 = Z1[:, j0:j1], Z2[:, j0:j1]
    return Z1, Z2, V, noise, j0, j1, fr.mvm_ref(z1, z2, V, fr.SCALE, noise), fr.mvm_mag(z1, z2, V, fr.SCALE, noise)


def _mvm_gate(case, mutate):
    Z1, Z2, V, noise, j0, j1, ref, A = _mvm_case(case)
    return fr.ratio(fr.restate_mvm(Z1, Z2, V, fr.SCALE, noise, j0, j1, mutate=mutate), ref, A) / fr.C["mvm"]


def _dense_gate(case, mutate):
    if case == "slice":
        Z1, Z2, _ = fr.mvm_slice_inputs()
        j0, j1 = fr.SLICE
    else:
        Z1, Z2 = fr.dense_inputs(*case)
        j0, j1 = 0, Z1.shape[1]
    got = fr.restate_dense(Z1, Z2, fr.SCALE, j0, j1, mutate=mutate)
    z1, z2 = Z1[:, j0:j1], Z2[:, j0:j1]
    return fr.ratio(got, fr.dense_ref(z1, z2, fr.SCALE), fr.dense_mag(z1, z2, fr.SCALE)) / fr.C["dense"]


def _bilinear_gate(case, mutate):
    """Worst of gZ, gscale and the guard columns (slice case: (N, J, T, j0, j1, ldg))."""
    N, J, T = case[:3]
    j0, j1, ldg = (case[3:] if len(case) > 3 else (0, J, J))
    Z, L, R = fr.bilinear_inputs(N, J, T)
    gZ, gs = fr.restate_bilinear(Z, L, R, fr.SCALE, j0, j1, ldg, mutate=mutate)
    ref, gs_ref = fr.bilinear_ref(Z[:, j0:j1], L, R, fr.SCALE)
    A, Ags = fr.bilinear_mag(Z[:, j0:j1], L, R, fr.SCALE)
    guard = np.delete(gZ, np.s_[j0:j1], axis=1)
    return max(fr.ratio(gZ[:, j0:j1], ref, A), fr.ratio(gs, gs_ref, Ags), 0.0 if np.isnan(guard).all() else np.inf) \
        / fr.C["bilinear"]


def _bilinear_dense_gate(case, mutate):
    N, J, lds = case
    Z, S = fr.bilinear_dense_inputs(N, J, lds)
    gZ, gs = fr.restate_bilinear_dense(Z, S, fr.SCALE, mutate=mutate)
    ref, gs_ref = fr.bilinear_dense_ref(Z, S[:, :N], fr.SCALE)
    A, Ags = fr.bilinear_mag(Z, None, None, fr.SCALE, S=S[:, :N])
    return max(fr.ratio(gZ, ref, A), fr.ratio(gs, gs_ref, Ags)) / fr.C["bilinear_dense"]


BIL_SLICE = (130, 12, 3) + fr.SLICE + (14,)
# per mutation: the cases that are meant to catch it (all of them cases of the GPU module), cheapest first
TABLE = {
    "tile_reread": [(_mvm_gate, (4097, 4097, 2, 1)), (_bilinear_gate, (4097, 3, 16))],
    "drop_ragged": [(_mvm_gate, (65, 65, 3, 2)), (_mvm_gate, (4097, 4097, 2, 1)), (_bilinear_gate, (65, 2, 13))],
    "cend_unclamped": [(_mvm_gate, (65, 65, 3, 2)), (_bilinear_gate, (65, 2, 13))],
    "chunk_t0": [(_mvm_gate, (321, 321, 35, 14)), (_bilinear_gate, (65, 2, 13))],
    "tcnt_mask": [(_mvm_gate, (321, 321, 35, 14)), (_bilinear_gate, (65, 2, 13))],
    "piece_j0": [(_mvm_gate, (321, 321, 35, 14)), (_dense_gate, (33, 300, 11)), (_bilinear_gate, (321, 35, 14))],
    "noise_per_piece": [(_mvm_gate, (321, 321, 35, 14))],
    "dense_no_accumulate": [(_dense_gate, (33, 300, 11)), (_dense_gate, "slice")],
    "ldz_swap": [(_mvm_gate, "slice"), (_dense_gate, "slice")],
    "rowS_overwrite": [(_bilinear_gate, (65, 2, 13))],
    "rowS_multicount": [(_bilinear_gate, (65, 2, 13)), (_bilinear_dense_gate, (321, 35, None))],
    "gz_outside_slice": [(_bilinear_gate, BIL_SLICE)],
    "lds_as_n": [(_bilinear_dense_gate, (64, 3, 69))],
}


def test_the_table_names_every_mutation():
    assert set(TABLE) == set(fr.MUTATIONS)


@pytest.mark.parametrize("mutate", fr.MUTATIONS)
def test_every_mutation_breaks_a_gate(mutate):
    """Each listed case passes unmutated and fails, by its own gate, with the mutation."""
    for gate, case in TABLE[mutate]:
        clean, broken = gate(case, None), gate(case, mutate)
        print("%-20s %-22s %-24s clean %.3f C, mutated %.3g C" % (mutate, gate.__name__, case, clean, broken))
        assert clean <= 1.0 < broken, (mutate, case, clean, broken)


def test_the_tile_loop_mutations_reach_the_named_cases():
    """The reachability evidence at the cases the issue names: the multi-tile product case (4161, 4161, 5, 17) -- 33 splits of
    two tiles, the last a full tile and a one-column one, chunks 12 + 5 -- passes as restated and fails when the second tile
    is not re-filled and when the later chunk loses t0; (4097, 4097, 2, 1), the one-column last split, fails when that ragged
    tile is dropped; pieces 8 + 2 + 1 of the dense block fail when it stops accumulating."""
    big = (4161, 4161, 5, 17)
    clean = _mvm_gate(big, None)
    figures = {m: _mvm_gate(big, m) for m in ("tile_reread", "chunk_t0")}
    print("(4161, 4161, 5, 17): clean %.3f C, %s" % (clean, ", ".join("%s %.3g C" % kv for kv in figures.items())))
    assert clean <= 1.0 and min(figures.values()) > 1.0
    assert _mvm_gate((4097, 4097, 2, 1), "drop_ragged") > 1.0 and _dense_gate((33, 300, 11), "dense_no_accumulate") > 1.0


# ---- the analytic SKI derivative of the test double -----------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["shared", "reference"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", fr.SKI_KINDS)
def test_oracle_ski_derivative_matches_central_differences(rule, weighted, kind):
    """OracleBackend.ski_bilinear_grad against central differences of oracle.ski.bilinear_objective at EVERY entry of
    N = 40, J = 3, G = 16, T = 3.  Step s = 2e-5.  Between knots the objective is a polynomial of degree <= 6 in z_ij (W is
    piecewise cubic, the grid fixed), so the central difference errs by at most s^2 / 6 max|f'''| plus the rounding
    8 u F / (2 s), F the objective with every term in absolute value (8: the roundings of one term and of the pairwise sums).
    With |w| <= 1, |w'| <= 1.5, |w''| <= 5, |w'''| <= 9 per tap in position units:
    |f'''| <= scale w_j / h^3 (9 P_i + 1008 |c_i|), P_i the sum over the row's 4 taps of sum_t |L_it| |HR| + |R_it| |HL| with
    absolute-value histograms (the other rows, linear in w) and c_i = L_i . R_i times the 16 Toeplitz entries <= 1 of the
    row's own pair (quadratic in w: 2 w''' T w + 6 w'' T w').  Where a knot lies within 2 s of z_ij (the shared rule puts
    its two extreme points on knots) W is only C^1 and the bound is the first-order one: s / 2 max|f''| with
    |f''| <= scale w_j / h^2 (5 P_i + 232 |c_i|)  (2 w'' T w + 2 w' T w')."""
    s = 2e-5
    ob = OracleBackend()
    N, M, J, T, G = 40, 10, 3, 3, 16
    Z, Zs, V, L, R, w = fr.ski_inputs(N, M, J, T, seed=1)
    Zt = torch.from_numpy(Z)
    gp = ob.ski_grid(Zt, None, G, torch.from_numpy(w) if weighted else None, rule, kind).double()
    grid, wts = ob._grid(gp), ob._w(gp)
    gZ = ob.ski_bilinear_grad(Zt, gp, torch.from_numpy(L), torch.from_numpy(R), fr.SCALE, G)[0].numpy()
    g0, h, inv_h, _, _ = fr.ski_block(gp.numpy(), J)
    pos = (Z - g0[None, :]) / h[None, :]
    assert pos.min() >= 1.0 and pos.max() <= G - 2.0                    # (no row clamps: the convention there is not at issue)
    knot = np.abs(pos - np.round(pos)) * h[None, :] <= 2 * s
    assert knot.sum() <= 2 * J                                          # (the shared rule puts its two extreme points on knots)
    La, Ra = np.abs(L), np.abs(R)
    F, bound = 0.0, np.zeros((N, J))
    for j in range(J):
        Wa = np.abs(sko.interp_matrix(Z[:, j], g0[j], h[j], G))
        Ta = np.abs(sko.toeplitz(h[j], G, kind))
        wj = 1.0 if wts is None else abs(wts[j])
        HLa, HRa = Ta @ (Wa.T @ La), Ta @ (Wa.T @ Ra)
        F += fr.SCALE * wj * float((La * (Wa @ HRa)).sum())
        P = 4.0 * (La[:, None, :] * HRa[None, :, :] + Ra[:, None, :] * HLa[None, :, :]).sum(axis=2).max(axis=1)
        c = np.abs((L * R).sum(axis=1))
        bound[:, j] = np.where(knot[:, j], s / 2.0 * fr.SCALE * wj / h[j] ** 2 * (5.0 * P + 232.0 * c),
                               s * s / 6.0 * fr.SCALE * wj / h[j] ** 3 * (9.0 * P + 1008.0 * c))
    bound += 8.0 * fr.U * F / (2.0 * s)
    worst = 0.0
    for i in range(N):
        for j in range(J):
            Zp, Zm = Z.copy(), Z.copy()
            Zp[i, j] += s
            Zm[i, j] -= s
            fd = (sko.bilinear_objective(Zp, L, R, fr.SCALE, G, grid, wts, kind)
                  - sko.bilinear_objective(Zm, L, R, fr.SCALE, G, grid, wts, kind)) / (2 * s)
            worst = max(worst, abs(gZ[i, j] - fd) / bound[i, j])
    print("%s %s %s: worst |analytic - central difference| / bound = %.3f (bounds %.1e .. %.1e, |gZ| up to %.2f)"
          % (rule, weighted, kind, worst, bound.min(), bound.max(), np.abs(gZ).max()))
    assert worst <= 1.0
