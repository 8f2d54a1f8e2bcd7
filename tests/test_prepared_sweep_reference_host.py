"""tests/prepared_sweep_reference.py on the CPU: the float64 columns against the oracle, the derived bound against a float32
numpy emulation of the factorised formula on every input distribution tests/test_prepared_sweep_gpu.py uses, the probe columns."""
import os

import numpy as np
import pytest

from tests import prepared_sweep_reference as psr

# (name, Z, j0, j1): the distributions of the GPU module (0.9 x standard normal at its projection counts, a j-slice, the wide
# uniform range) at sizes a CPU sums in a second
DISTRIBUTIONS = [
    ("normal-J20", lambda: psr.normal_inputs(1500, 20, 1520), 0, 20),
    ("normal-J19", lambda: psr.normal_inputs(900, 19, 919), 0, 19),
    ("normal-J13", lambda: psr.normal_inputs(700, 13, 714), 0, 13),
    ("normal-J7", lambda: psr.normal_inputs(1300, 7, 1332), 0, 7),
    ("normal-J1", lambda: psr.normal_inputs(65, 1, 69), 0, 1),
    ("normal-slice", lambda: psr.normal_inputs(1000, 20, 5033), 2, 6),
    ("wide", lambda: psr.wide_inputs(3001, 6), 0, 6),
    ("wide-small", lambda: psr.wide_inputs(500, 3, seed=3), 0, 3),
]


def test_kernel_columns_agree_with_the_oracle():
    from oracle import dense_gp as orc
    Z = psr.normal_inputs(331, 7, 1)
    cols = psr.edge_columns(331)
    K, terms = psr.kernel_columns(Z, cols)
    ref = orc.additive_rbf(Z.astype(np.float64), Z.astype(np.float64))[:, cols]
    assert np.abs(K - ref).max() < 1e-13 * 7
    assert terms.shape == (331, len(cols), 7) and np.abs(terms.sum(axis=2) - K).max() == 0.0
    Ks, _ = psr.kernel_columns(Z, cols, 2, 5)
    refs = orc.additive_rbf(Z[:, 2:5].astype(np.float64), Z[:, 2:5].astype(np.float64))[:, cols]
    assert np.abs(Ks - refs).max() < 1e-13 * 3


@pytest.mark.parametrize("name,make,j0,j1", DISTRIBUTIONS, ids=[d[0] for d in DISTRIBUTIONS])
def test_float32_emulation_stays_inside_the_unmargined_bound(name, make, j0, j1):
    """Per term (e * Ea against k_j, bound rel_j k_j + 2^-120) and per entry with the J sum in the compiler kernel's order
    (against `entry_bound`): worst ratio error / bound < 1, mean ratio > 0.02 (an inflated bound would push the mean down).
    Measured here: per term worst 0.46 - 0.75, mean 0.10 - 0.12 (max|a| 1.7 ... 9.5); per entry worst 0.35 - 0.73, mean 0.07 - 0.12."""
    Z = make()
    N = Z.shape[0]
    cols = psr.edge_columns(N)
    K, terms = psr.kernel_columns(Z, cols, j0, j1)
    a = psr.scaled_coordinates(Z, j0, j1)
    e, Ea = psr.emulate_terms(Z, cols, j0, j1)
    with np.errstate(under="ignore"):
        got_t = (e * Ea[:, None, :]).astype(np.float64)
    bound_t = psr.term_rel(a[:, None, :], a[cols][None, :, :]) * terms + psr.FLUSH
    r_t = np.abs(got_t - terms) / bound_t
    live = terms > 2.0 ** -100                                   # (the mean over terms that are not all flush allowance)
    bound = psr.entry_bound(Z, cols, j0, j1, terms=terms)
    r_e = np.abs(psr.emulate_entries(Z, cols, j0, j1).astype(np.float64) - K) / bound
    print("%s: max|a| %.2f  per term worst %.3f mean %.3f  per entry worst %.3f mean %.3f"
          % (name, np.abs(a).max(), r_t.max(), r_t[live].mean(), r_e.max(), r_e.mean()))
    assert r_t.max() < 1.0 and r_e.max() < 1.0
    assert r_t[live].mean() > 0.02 and r_e.mean() > 0.02


def test_bound_is_the_stated_formula():
    """One term by hand: the formula of the module docstring, not a constant that drifted."""
    a, b = 1.25, -0.5
    want = 2.0 ** -24 * (np.log(2.0) * (6 * 1.75 * 1.75 + 1.5625 + 0.25 + abs(2 * a * b - 0.25)) + 5)
    assert abs(psr.term_rel(np.float64(a), np.float64(b)) - want) < 1e-20
    Z = np.array([[0.0], [1.0], [3.0]], dtype=np.float32)              # mid 1.5
    bd = psr.entry_bound(Z, [1])
    aa = (Z[:, 0].astype(np.float64) - 1.5) * psr.C_EXP2
    k = np.exp(-0.5 * (Z[:, 0].astype(np.float64) - 1.0) ** 2)
    assert np.allclose(bd[:, 0], psr.term_rel(aa, aa[1]) * k + 2.0 ** -120, rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 300, 700, 2049, 4095, 4096, 4161, 4225, 5000, 10240, 10303, 16449])
def test_edge_columns(N):
    cols = psr.edge_columns(N)
    assert len(cols) <= 48 and len(set(cols)) == len(cols) and all(0 <= c < N for c in cols)
    assert 0 in cols and N - 1 in cols
    for q in (64, 256, 512):
        if N > q:                                                   # both sides of a q boundary, and of the LAST one below N
            b = (N - 1) // q * q
            assert b - 1 in cols and b in cols
            assert any(c % q == q - 1 and c + 1 in cols for c in cols)
    if N > 64:
        assert 63 in cols and 64 in cols
    tail0 = (N - 1) // 64 * 64
    assert any(tail0 <= c < N for c in cols)
    few = psr.edge_columns(N, 16)
    assert few == cols[:16]


def test_unit_blocks_cover_the_probes():
    cols = psr.edge_columns(4161)
    for T in (1, 5, 13, 25):
        blocks = psr.unit_blocks(4161, cols, T)
        assert len(blocks) == -(-len(cols) // T)
        seen = []
        for V, blk in blocks:
            assert V.shape == (4161, T) and V.dtype == np.float32 and V.sum() == T
            assert all(V[c, t] == 1.0 for t, c in enumerate(blk))
            seen += blk
        assert set(seen) == set(cols)


def test_dense_rhs_rule_looks_at_v_alone():
    """Standard-normal float32 columns, none with a sum in the lowest decile of |1^T v| / sqrt(N); the first seed that has none."""
    for (N, T, seed) in [(2049, 13, 2083), (4161, 5, 4186), (10303, 2, 10326), (16449, 1, 16471)]:
        V = psr.dense_rhs(N, T, seed)
        assert V.shape == (N, T) and V.dtype == np.float32
        assert (np.abs(V.astype(np.float64).sum(axis=0)) >= np.sqrt(N) / 8).all()
        assert abs(V.std() - 1.0) < 0.05 and abs(V.mean()) < 0.05
        first = np.random.default_rng(seed).standard_normal((N, T)).astype(np.float32)
        if (np.abs(first.astype(np.float64).sum(axis=0)) >= np.sqrt(N) / 8).all():
            assert np.array_equal(V, first)
        assert np.array_equal(V, psr.dense_rhs(N, T, seed))


def test_sweep_sets_and_restores_the_environment():
    keep = {k: os.environ.get(k) for k in ("RPGP_LOWRANK", "RPGP_FACT_ASM")}
    try:
        os.environ.pop("RPGP_LOWRANK", None)
        os.environ["RPGP_FACT_ASM"] = "7"
        with psr.sweep():
            assert os.environ["RPGP_LOWRANK"] == "0" and os.environ["RPGP_FACT_ASM"] == "7"
            with psr.sweep("0"):
                assert os.environ["RPGP_FACT_ASM"] == "0"
            assert os.environ["RPGP_FACT_ASM"] == "7"
        assert "RPGP_LOWRANK" not in os.environ and os.environ["RPGP_FACT_ASM"] == "7"
        os.environ.pop("RPGP_FACT_ASM")
        with pytest.raises(RuntimeError):
            with psr.sweep("1"):
                assert os.environ["RPGP_FACT_ASM"] == "1"
                raise RuntimeError("x")
        assert "RPGP_FACT_ASM" not in os.environ and "RPGP_LOWRANK" not in os.environ
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_pieces_restate_the_dispatch():
    assert [jt for _, jt in psr.j_pieces(0, 19)] == [10, 8, 1]
    assert [jt for _, jt in psr.j_pieces(0, 17)] == [10, 5, 2]
    assert [jt for _, jt in psr.j_pieces(0, 13)] == [10, 3]
    assert [jt for _, jt in psr.j_pieces(0, 14)] == [10, 4]
    assert [jt for _, jt in psr.j_pieces(0, 6)] == [5, 1]
    assert [jt for _, jt in psr.j_pieces(2, 6)] == [4] and [jt for _, jt in psr.j_pieces(3, 6)] == [3]
    assert psr.t_pieces(13) == [(0, 12, 12), (12, 1, 1)] and psr.t_pieces(16) == [(0, 12, 12), (12, 4, 4)]
    assert psr.t_pieces(25) == [(0, 12, 12), (12, 12, 12), (24, 1, 1)]
    assert psr.t_pieces(5) == [(0, 12, 5)] and psr.t_pieces(3) == [(0, 4, 3)] and psr.t_pieces(2) == [(0, 4, 2)]
