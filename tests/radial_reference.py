"""Reference, error bounds and a float32 emulation for the full radial kernels (csrc/rpgp_radial.hip) — test helpers.

The float64 reference of every check is oracle/family.py with ONE component of group = d and weights [1]:
    K[i,i'] = scale * phi_kind(|a_i - b_i'|^2)
evaluated on the float32 inputs exactly as the kernel receives them.

The kernel takes the squared distance in the Gram form d2 = max(|a|^2 + |b|^2 - 2 a.b, 0) in float32.  With u = 2^-24

    |delta d2_ij| <= (d + 4) u (|a_i| + |b_j|)^2                          (any summation order)
    entry bound   =  scale (C_phi (d + 4) u (|a_i| + |b_j|)^2 + c u (1 + d2 |phi'(d2)|))
    row bound     =  sum_j entry_ij |V_jt|  +  (N - 1) u sum_j |K_ij| |V_jt|

C_phi = max |phi'| (0.5 RBF, 1.5 Matern, 0.5 InverseMQ, pi^2 / 2 Cosine).  c = 8 would cover a handful of roundings on the
argument path plus the hardware transcendental.  It is NOT taken from the radial kernels: it was measured on the MI355X on the
existing direct-difference family kernels (ops.family_dense, one component, group = d in {1, 3, 4, 5, 20}, the inputs of
`inputs()` at (N, M) = (257, 129) and (1237, 301), scale 1.3), whose largest error in the unit scale u (1 + d2 |phi'|) is
recorded in C_MEASURED_FAMILY below (tools/radial_bench.py --constant prints it).  Twice their maximum, 2 x 6.553 = 13.11 (the
Cosine member, through the library cosine of the runtime-(kind, group) kernels), exceeds 8, so c = 13.11.  The
radial kernels themselves stay below 0.25 of the entry bound at c = 8 on every case of `cases()`.

`Emulation` is a numpy float32 restatement of the same Gram form (derivative included) with switchable defects: the host test
(tests/test_radial_reference_host.py) holds it to the bounds and gates below and shows that every defect of the mutation table
misses at least one of them — so the checks the GPU tests apply can see those defects.
"""
import numpy as np

from oracle import family as fmo

U = 2.0 ** -24
C_PHI = {"RBF": 0.5, "Matern": 1.5, "InverseMQ": 0.5, "Cosine": 0.5 * np.pi ** 2}
# largest |family_dense - float64| / (scale u (1 + d2 |phi'|)) of the direct-difference family kernels on the MI355X (see the
# module docstring; tools/radial_bench.py --constant prints it): RBF, Matern, InverseMQ, Cosine
C_MEASURED_FAMILY = {"RBF": 3.190, "Matern": 3.408, "InverseMQ": 2.757, "Cosine": 6.553}
C_CONST = max(8.0, 2.0 * max(C_MEASURED_FAMILY.values()))

# gates of tests/test_family_gpu.py for the same quantities
GATE_PRODUCT_REL = 5e-6
GATE_DENSE_ABS = 2e-5
GATE_GRAD_REL = 2e-5

KINDS = ("RBF", "Matern", "InverseMQ", "Cosine")
DIMS = (1, 3, 4, 5, 20, 21, 33, 90, 385)
SIZES = ((1, 1), (5, 3), (63, 64), (65, 31), (257, 129), (1237, 301))          # (N, M)
WIDTHS = (1, 11, 16)


def cases():
    """(kind, d, N, M, T): the cross product thinned so that every value of every axis meets every kind at least once."""
    out = []
    for k, kind in enumerate(KINDS):
        for j, d in enumerate(DIMS):
            N, M = SIZES[(j + k) % len(SIZES)]
            out.append((kind, d, N, M, WIDTHS[(j + k) % len(WIDTHS)]))
    return out


def grad_rows(d, n):
    """Rows the derivative checks use at (d, n): n, or 257 where the float64 reference (d matrices of n x n) would not fit a
    test of a few seconds."""
    return n if d * n * n <= 6e7 else min(n, 257)


def inputs(n, d, seed, duplicates=True):
    """Z = N(0,1) min(1, 2 / sqrt(d)), seeded, float32, centred; with n >= 4 one pair of exact duplicate rows (0, 1) and one pair
    at a factor 1 + 1e-4 (2, 3)."""
    rng = np.random.default_rng(seed)
    Z = (rng.standard_normal((n, d)) * min(1.0, 2.0 / np.sqrt(d))).astype(np.float32)
    if duplicates and n >= 4:
        Z[1] = Z[0]
        Z[3] = Z[2] * np.float32(1.0 + 1e-4)
    Z = (Z - Z.mean(axis=0, dtype=np.float64).astype(np.float32)).astype(np.float32)
    if duplicates and n >= 4:
        Z[1] = Z[0]
    return Z


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def sqdist(Z1, Z2):
    Z1, Z2 = np.asarray(Z1, dtype=np.float64), np.asarray(Z2, dtype=np.float64)
    d2 = np.zeros((Z1.shape[0], Z2.shape[0]))
    for m in range(Z1.shape[1]):
        df = Z1[:, m:m + 1] - Z2[:, m:m + 1].T
        d2 += df * df
    return d2


def kernel(Z1, Z2, kind, scale=1.0):
    return fmo.kernel_matrix(Z1, Z2, kind, np.asarray(Z1).shape[1], [1.0], scale)


def product(Z1, Z2, V, kind, scale=1.0, noise=0.0):
    return fmo.mvm(Z1, Z2, V, kind, np.asarray(Z1).shape[1], [1.0], scale, noise)


def grad_factors(Z, L, R, kind, scale=1.0):
    gZ, gc = fmo.bilinear_grad(np.asarray(Z, dtype=np.float64), L, R, kind, np.asarray(Z).shape[1], [1.0], scale)
    return gZ, float(gc[0])


def grad_dense(Z, S, kind, scale=1.0):
    gZ, gc = fmo.bilinear_grad_dense(np.asarray(Z, dtype=np.float64), S, kind, np.asarray(Z).shape[1], [1.0], scale)
    return gZ, float(gc[0])


# ---- the two bounds -------------------------------------------------------------------------------------------------------
def entry_bound(Z1, Z2, kind, scale=1.0, c=C_CONST):
    Z1, Z2 = np.asarray(Z1, dtype=np.float64), np.asarray(Z2, dtype=np.float64)
    d = Z1.shape[1]
    n1, n2 = np.sqrt((Z1 * Z1).sum(1)), np.sqrt((Z2 * Z2).sum(1))
    d2 = sqdist(Z1, Z2)
    dphi = np.abs(fmo._dphi(kind, d2, fmo._phi(kind, d2)))
    return abs(scale) * (C_PHI[kind] * (d + 4) * U * (n1[:, None] + n2[None, :]) ** 2 + c * U * (1.0 + d2 * dphi))


def row_bound(Z1, Z2, V, kind, scale=1.0, c=C_CONST):
    V = np.abs(np.asarray(V, dtype=np.float64)).reshape(np.asarray(Z2).shape[0], -1)
    n = V.shape[0]
    return entry_bound(Z1, Z2, kind, scale, c) @ V + (n - 1) * U * (np.abs(kernel(Z1, Z2, kind, scale)) @ V)


def check_dense(got, Z1, Z2, kind, scale, c=C_CONST):
    """Entry bound and max-abs gate of a dense block; returns (max error, largest error / bound)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - kernel(Z1, Z2, kind, scale))
    ratio = float((err / entry_bound(Z1, Z2, kind, scale, c)).max())
    assert np.isfinite(err).all(), "non-finite entries"
    assert ratio <= 1.0, "entry bound exceeded: %.3g of it (max error %.3g)" % (ratio, err.max())
    assert err.max() <= GATE_DENSE_ABS, "max-abs %.3g" % err.max()
    return float(err.max()), ratio


def check_product(got, Z1, Z2, V, kind, scale, noise=0.0, c=C_CONST):
    """Row bound and norm-wise gate of a product (Z2 None: the symmetric operator with noise); returns (rel, error / bound)."""
    sym = Z2 is None
    Zb = Z1 if sym else Z2
    V2 = np.asarray(V, dtype=np.float64).reshape(np.asarray(Zb).shape[0], -1)
    ref = product(Z1, Zb, V2, kind, scale, noise if sym else 0.0)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "non-finite entries"
    err = np.abs(got - ref)
    ratio = float((err / row_bound(Z1, Zb, V2, kind, scale, c)).max())
    r = rel(got, ref)
    assert ratio <= 1.0, "row bound exceeded: %.3g of it" % ratio
    assert r <= GATE_PRODUCT_REL, "product rel %.3g" % r
    return r, ratio


def check_grad(gZ, gscale, ref_gZ, ref_gscale):
    """Norm-wise gates of the derivative; returns (rel gZ, rel gscale)."""
    gZ = np.asarray(gZ, dtype=np.float64)
    assert np.isfinite(gZ).all() and np.isfinite(gscale), "non-finite entries"
    rz = rel(gZ, ref_gZ) if np.linalg.norm(ref_gZ) > 0 else float(np.abs(gZ).max())
    rs = abs(float(gscale) - ref_gscale) / max(abs(ref_gscale), 1e-300)
    assert rz <= GATE_GRAD_REL, "gZ rel %.3g" % rz
    assert rs <= GATE_GRAD_REL, "gscale rel %.3g" % rs
    return rz, rs


# ---- float32 emulation of the Gram form -----------------------------------------------------------------------------------
_F = np.float32


def _phi32(kind, d2):
    d2 = d2.astype(_F)
    with np.errstate(invalid="ignore"):
        if kind == "RBF":
            p = np.exp(_F(-0.5) * d2)
            return p, _F(-0.5) * p
        if kind == "InverseMQ":
            p = _F(1.0) / np.sqrt(_F(1.0) + d2)
            return p, _F(-0.5) * p * p * p
        r = np.sqrt(d2)
        if kind == "Matern":
            e = np.exp(_F(-np.sqrt(3.0)) * r)
            return (_F(1.0) + _F(np.sqrt(3.0)) * r) * e, _F(-1.5) * e
        x2 = _F(np.pi ** 2) * d2
        series = _F(1.0) + x2 * (_F(-1.0 / 6) + x2 * (_F(1.0 / 120) + x2 * (_F(-1.0 / 5040) + x2 * _F(1.0 / 362880))))
        with np.errstate(divide="ignore"):
            direct = np.sin(_F(np.pi) * r) / (_F(np.pi) * r)
        sinc = np.where(x2 < _F(0.25), series, direct).astype(_F)
        sinc = np.where(np.isnan(d2), _F(np.nan), sinc)
        return np.cos(_F(np.pi) * r).astype(_F), _F(-0.5 * np.pi ** 2) * sinc


class Emulation:
    """The radial kernels in numpy float32: inputs X (raw) and the centre mu, Z = X - mu, row norms, Gram product over
    features four at a time, d2 = max(na + nb - 2 G, 0) with a forced diagonal in the symmetric form, phi, the product over
    64-column tiles, the derivative as a_i r_i - (M A)_i.  `defect` switches ONE of the mutation table's defects on."""

    DEFECTS = ("drop_last_chunk", "drop_tile", "drop_noise", "diagonal_not_forced", "no_clamp", "centre_one_operand",
               "grad_factor_2", "drop_RLt")

    def __init__(self, kind, defect=None):
        assert defect is None or defect in self.DEFECTS
        self.kind, self.defect = kind, defect

    def _centre(self, X, mu, second=False):
        X = np.asarray(X, dtype=_F)
        if mu is None or (second and self.defect == "centre_one_operand"):
            return X
        return (X - np.asarray(mu, dtype=_F)).astype(_F)

    def _d2(self, A, B, sym):
        d = A.shape[1]
        # (norms by numpy's pairwise float32 sum, the Gram product feature by feature: two different summation orders, as any
        #  pair of orders is covered by the bound)
        na, nb = (A * A).sum(1, dtype=_F), (B * B).sum(1, dtype=_F)
        G = np.zeros((A.shape[0], B.shape[0]), dtype=_F)
        dd = (d // 4) * 4 if (self.defect == "drop_last_chunk" and d % 4) else d
        for m in range(dd):
            G += A[:, m:m + 1] * B[:, m:m + 1].T
        d2 = (na[:, None] + nb[None, :]) - _F(2.0) * G
        if self.defect != "no_clamp":
            d2 = np.maximum(d2, _F(0.0))
        if sym and self.defect != "diagonal_not_forced":
            np.fill_diagonal(d2, _F(0.0))
        return d2.astype(_F)

    def dense(self, X1, X2, mu, scale):
        sym = X2 is None
        A = self._centre(X1, mu)
        B = A if sym else self._centre(X2, mu, second=True)
        return _F(scale) * _phi32(self.kind, self._d2(A, B, sym))[0]

    def product(self, X1, X2, mu, V, scale, noise=0.0):
        sym = X2 is None
        A = self._centre(X1, mu)
        B = A if sym else self._centre(X2, mu, second=True)
        K = _phi32(self.kind, self._d2(A, B, sym))[0]
        V = np.asarray(V, dtype=_F).reshape(B.shape[0], -1)
        out = np.zeros((A.shape[0], V.shape[1]), dtype=_F)
        tiles = list(range(0, B.shape[0], 64))
        if self.defect == "drop_tile" and len(tiles) > 1:
            tiles = tiles[:1] + tiles[2:]
        for c0 in tiles:
            out += K[:, c0:c0 + 64] @ V[c0:c0 + 64]
        out = _F(scale) * out
        if sym and self.defect != "drop_noise":
            out = out + _F(noise) * V
        return out.astype(_F)

    def grad(self, X, mu, scale, L=None, R=None, S=None):
        A = self._centre(X, mu)
        if S is None:
            L, R = np.asarray(L, dtype=_F).reshape(A.shape[0], -1), np.asarray(R, dtype=_F).reshape(A.shape[0], -1)
            S = L @ R.T
            if self.defect != "drop_RLt":
                S = S + R @ L.T
        S = np.asarray(S, dtype=_F)
        p, dp = _phi32(self.kind, self._d2(A, A, True))
        Mm = (S * dp).astype(_F)
        np.fill_diagonal(Mm, _F(0.0))
        r = Mm.sum(1, dtype=_F)
        gZ = _F(2.0 * scale) * (A * r[:, None] - Mm @ A)
        if self.defect == "grad_factor_2":
            gZ = _F(0.5) * gZ
        return gZ.astype(_F), float(0.5 * (S.astype(np.float64) * p).sum())
