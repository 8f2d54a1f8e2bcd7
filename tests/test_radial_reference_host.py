"""The checks of the full radial kernels, tried on the CPU (no GPU): the float32 emulation of the Gram form
(tests/radial_reference.py) passes the entry bound, the row bound and the norm-wise gates that tests/test_radial_kernels_gpu.py
applies to the HIP kernels, and every defect of the mutation table misses at least one of them."""
import numpy as np
import pytest

from tests import radial_reference as rr


def _battery(emu, kind, d, N, M, T, seed, scale=0.7, noise=0.13, shift=3.0):
    """Every check of the GPU tests on `emu`, with raw inputs X = Z + shift and the centre mu = shift."""
    rng = np.random.default_rng(seed + 1000)
    mu = np.full(d, shift, dtype=np.float32)
    X1, X2 = (rr.inputs(N, d, seed) + mu).astype(np.float32), (rr.inputs(M, d, seed + 1) + mu).astype(np.float32)
    Z1, Z2 = (X1 - mu).astype(np.float32), (X2 - mu).astype(np.float32)        # what a correct kernel receives
    V = rng.standard_normal((N, T)).astype(np.float32)
    rr.check_dense(emu.dense(X2, X1, mu, scale), Z2, Z1, kind, scale)
    rr.check_dense(emu.dense(X1, None, mu, scale), Z1, Z1, kind, scale)
    rr.check_product(emu.product(X1, None, mu, V, scale, noise), Z1, None, V, kind, scale, noise)
    rr.check_product(emu.product(X2, X1, mu, V, scale), Z2, Z1, V, kind, scale)
    eye = np.eye(N, dtype=np.float32)[:, :min(N, 16)]
    diag = emu.product(X1, None, mu, eye, scale, noise)
    want = np.float32(scale) + np.float32(noise)
    assert all(diag[i, i] == want for i in range(eye.shape[1])), "the diagonal contribution is not exactly scale + noise"
    n = rr.grad_rows(d, N)
    L, R = rng.standard_normal((n, T)).astype(np.float32), rng.standard_normal((n, T)).astype(np.float32)
    gZ, gs = emu.grad(X1[:n], mu, scale, L=L, R=R)
    rr.check_grad(gZ, gs, *rr.grad_factors(Z1[:n], L, R, kind, scale))
    S = rng.standard_normal((n, n)).astype(np.float32)
    S = ((S + S.T) / 2).astype(np.float32)
    gZ, gs = emu.grad(X1[:n], mu, scale, S=S)
    rr.check_grad(gZ, gs, *rr.grad_dense(Z1[:n], S, kind, scale))


def test_cases_cover_every_axis_for_every_kind():
    cs = rr.cases()
    for kind in rr.KINDS:
        mine = [c for c in cs if c[0] == kind]
        assert {c[1] for c in mine} == set(rr.DIMS)
        assert {(c[2], c[3]) for c in mine} == set(rr.SIZES)
        assert {c[4] for c in mine} == set(rr.WIDTHS)


@pytest.mark.parametrize("kind,d,N,M,T", [c for c in rr.cases() if c[1] * c[2] <= 40000])
def test_emulation_passes_bounds_and_gates(kind, d, N, M, T):
    _battery(rr.Emulation(kind), kind, d, N, M, T, seed=d + N)


def test_emulation_figures_of_the_stated_inputs():
    """The figures the issue quotes for the centred inputs Z = N(0,1) min(1, 2 / sqrt(d)): product rel a few 1e-7, K max-abs
    <= 1e-5, gZ rel <= 2.2e-6 — an order of magnitude inside the gates."""
    for kind, d in (("RBF", 90), ("Matern", 21), ("Cosine", 5), ("InverseMQ", 385)):
        N, T = 257, 11
        Z = rr.inputs(N, d, 7)
        rng = np.random.default_rng(8)
        V, L, R = (rng.standard_normal((N, T)).astype(np.float32) for _ in range(3))
        emu = rr.Emulation(kind)
        r, _ = rr.check_product(emu.product(Z, None, None, V, 0.7, 0.13), Z, None, V, kind, 0.7, 0.13)
        e, _ = rr.check_dense(emu.dense(Z, None, None, 1.0), Z, Z, kind, 1.0)
        gZ, gs = emu.grad(Z, None, 1.0, L=L, R=R)
        rz, _ = rr.check_grad(gZ, gs, *rr.grad_factors(Z, L, R, kind, 1.0))
        assert r < 2e-6 and e < 1e-5 and rz < 5e-6, (kind, d, r, e, rz)


# (defect, kind, d, N, M, T): a shape at which the defect exists (d % 4 != 0, more than one tile, duplicates, ...)
MUTATIONS = [
    ("drop_last_chunk", "RBF", 5, 65, 31, 11),
    ("drop_tile", "InverseMQ", 4, 257, 129, 1),
    ("drop_noise", "RBF", 20, 63, 64, 16),
    ("diagonal_not_forced", "Cosine", 90, 65, 31, 11),
    ("no_clamp", "Matern", 33, 257, 129, 1),
    ("no_clamp", "Cosine", 33, 257, 129, 1),
    ("centre_one_operand", "RBF", 21, 65, 31, 11),
    ("grad_factor_2", "Matern", 3, 65, 31, 16),
    ("drop_RLt", "InverseMQ", 21, 63, 64, 11),
]


@pytest.mark.parametrize("defect,kind,d,N,M,T", MUTATIONS)
def test_every_mutation_misses_a_check(defect, kind, d, N, M, T):
    _battery(rr.Emulation(kind), kind, d, N, M, T, seed=5)                      # the sound emulation passes at this shape ...
    with pytest.raises(AssertionError):                                        # ... and the defective one does not
        _battery(rr.Emulation(kind, defect), kind, d, N, M, T, seed=5)
    assert set(m[0] for m in MUTATIONS) == set(rr.Emulation.DEFECTS)


def test_uncentred_inputs_are_why_centring_is_required():
    """Un-centred z-scored inputs at lengthscale 1, d = 90: entries near K ~ 1 (near-duplicates) are off by ~1e-4 in the Gram form,
    against ~1e-6 once the same inputs are centred and scaled by sqrt(d) — the bound says so too (it grows with the norms)."""
    rng = np.random.default_rng(0)
    d, N = 90, 200
    X = (rng.standard_normal((N, d)) + 1.0).astype(np.float32)
    X[1::2] = X[0::2] * np.float32(1.0 + 1e-3)                                  # near-duplicate pairs: K ~ 1
    emu = rr.Emulation("RBF")
    bad = np.abs(emu.dense(X, None, None, 1.0).astype(np.float64) - rr.kernel(X, X, "RBF"))
    Zc = ((X - X.mean(0)) / np.float32(np.sqrt(d))).astype(np.float32)
    good = np.abs(emu.dense(Zc, None, None, 1.0).astype(np.float64) - rr.kernel(Zc, Zc, "RBF"))
    assert bad.max() > 2e-5 and good.max() < 2e-6
    assert (bad <= rr.entry_bound(X, X, "RBF")).all() and (good <= rr.entry_bound(Zc, Zc, "RBF")).all()
