"""Float64 reference, condition bound and checker of the bilinear derivative (rpgp_bilinear_grad, its dense-weight and
float64 twins; include/rpgp.h) — plain numpy, no device code, in the spirit of tests/cg_reference.py.

    gZ[i, j] = -scale * sum_c S[i, c] e_j(i, c) (z_ij - z_cj)        e_j(i, c) = exp(-(z_ij - z_cj)^2 / 2)
    gscale   = 1/2 sum_i sum_c S[i, c] sum_j e_j(i, c)               S = L R^T + R L^T (or an explicit symmetric S)

An entry of gZ is a sum of N terms of both signs that cancel to 1/40 .. 1/200 of their absolute sum, so a relative 2-norm
over the whole of gZ cannot see one stale row or one mis-staged column.  The forward error of a floating-point sum is
bounded by (a small multiple of) u times the sum of the ABSOLUTE values of what is added up, so next to every reference
value this module returns that sum — the condition bound

    B[i, j] = scale * sum_c (sum_t |L_it R_ct| + |R_it L_ct|) e_j(i, c) |z_ij - z_cj|          (|S[i, c]| for an explicit S)
    Bs      = 1/2 sum_i sum_c (the same bound of |S|) sum_j e_j(i, c)

and `check` holds a result to  |got - ref| <= c u B  entrywise (and to the project's 2-norm gates, whole and per column).
The constant c is MEASURED on the host (tests/test_bilinear_reference_host.py): `restate_f32` is the same sum in float32
with the kernels' arithmetic (inputs pre-scaled by sqrt(log2(e) / 2), exp2(-d^2), S formed in float32) and a sequential
running sum; its largest entrywise ratio is c_ref and the GPU tests use 16 c_ref rounded up to a power of two, never
more than C_CAP: a dropped term moves an entry by about B / N = 2^24 u B / N, which a larger constant would let pass.

`reference` takes gZ and gscale from oracle.dense_gp.bilinear_grad on the sliced columns.  `Bank` is the same numbers
column by column for SEVERAL weight sets over one Z — every exponential once, shared by all the slices and right-hand-side
widths of a test module (the host module holds the two to 1e-13 of each other)."""
import numpy as np

from oracle import dense_gp as orc

U32 = 2.0 ** -24
U64 = 2.0 ** -53
GATES = {U32: 2e-5, U64: 1e-11}       # relative 2-norm gates of test_kernels_gpu.py / test_double_gpu.py
C_CAP = 64.0
C_REF_CAP = 4.0
# the constant of the entrywise gate in use: 16 c_ref rounded up to a power of two.  The host module measures c_ref = 3.64 on
# its CPU and asserts that whatever it measures still gives this constant (any c_ref in (2, 4] does)
C = 64.0
KEXP2 = 0.8493218002880191            # sqrt(0.5 * log2(e)):  exp(-d^2 / 2) = exp2(-(KEXP2 d)^2)


class Ref:
    """gZ, B: [rows x (j1 - j0)] float64; gs, Bs: floats (None with a row subset); rows: None or the row indices."""

    def __init__(self, gZ, gs, B, Bs, j0, j1, rows=None):
        self.gZ, self.gs, self.B, self.Bs, self.j0, self.j1, self.rows = gZ, gs, B, Bs, j0, j1, rows


class CheckFailure(AssertionError):
    """`gates`: the names of every gate that fired ("norm", "column", "entry", "gscale", "outside", "nan")."""

    def __init__(self, message, gates):
        super().__init__(message)
        self.gates = tuple(gates)


def c_from(c_ref):
    """The constant of the GPU tests: 16 c_ref rounded up to a power of two (see the module docstring)."""
    return float(2.0 ** np.ceil(np.log2(16.0 * c_ref)))


def _weights64(L, R, S, rows):
    """(S, bound of |S|) restricted to `rows`, float64."""
    sel = slice(None) if rows is None else rows
    if S is not None:
        Sr = np.asarray(S, dtype=np.float64)[sel]
        return Sr, np.abs(Sr)
    L = np.asarray(L, dtype=np.float64).reshape(L.shape[0], -1)
    R = np.asarray(R, dtype=np.float64).reshape(R.shape[0], -1)
    Sr = L[sel] @ R.T + R[sel] @ L.T
    Sa = np.abs(L[sel]) @ np.abs(R).T + np.abs(R[sel]) @ np.abs(L).T
    return Sr, Sa


def _rowsum(A, Bm, precise):
    if precise:                       # products rounded once in float64, the sum in extended precision
        return np.asarray((A * Bm).sum(axis=1, dtype=np.longdouble), dtype=np.float64)
    return np.einsum("ic,ic->i", A, Bm)


def _columns64(Z, weights, scale, cols, rows, precise):
    """Per weight set (S, Sa): gZ, B [m x len(cols)] and the per-column parts gs_j, Bs_j [len(cols)] — row-block-wise
    (m = len(rows)) as test_headline_oracle_gpu.py::test_bilinear_derivative_rows forms them: O(m N J)."""
    Z = np.asarray(Z, dtype=np.float64)
    m = Z.shape[0] if rows is None else len(rows)
    out = [dict(gZ=np.zeros((m, len(cols))), B=np.zeros((m, len(cols))), gs=np.zeros(len(cols)), Bs=np.zeros(len(cols)))
           for _ in weights]
    d, e, g = (np.empty((m, Z.shape[0])) for _ in range(3))        # reused by every column
    for k, j in enumerate(cols):
        zc = Z[:, j]
        zr = zc if rows is None else zc[rows]
        np.subtract(zr[:, None], zc[None, :], out=d)
        np.multiply(d, d, out=e)
        e *= -0.5
        np.exp(e, out=e)
        np.multiply(e, d, out=g)
        np.abs(g, out=d)                                          # |e d|
        for o, (S, Sa) in zip(out, weights):
            o["gZ"][:, k] = -scale * _rowsum(S, g, precise)
            o["B"][:, k] = scale * _rowsum(Sa, d, precise)
            o["gs"][k] = 0.5 * _rowsum(S, e, precise).sum()
            o["Bs"][k] = 0.5 * _rowsum(Sa, e, precise).sum()
    return out


def reference(Z, L, R, scale, j0, j1, rows=None, precise=False):
    """float64 gZ[:, j0:j1] and gscale of oracle.dense_gp.bilinear_grad on Z[:, j0:j1], with their condition bounds.
    `rows`: only those rows of gZ, at O(len(rows) N J); no gscale then.  `precise`: extended-precision sums (the
    reference of the float64 kernels, whose own rounding is the reference's otherwise)."""
    Z = np.asarray(Z, dtype=np.float64)
    w = _weights64(L, R, None, rows)
    o = _columns64(Z, [w], scale, list(range(j0, j1)), rows, precise)[0]
    if rows is not None:
        return Ref(o["gZ"], None, o["B"], None, j0, j1, np.asarray(rows))
    if precise:
        return Ref(o["gZ"], float(o["gs"].sum()), o["B"], float(o["Bs"].sum()), j0, j1)
    gZ, gs = orc.bilinear_grad(Z[:, j0:j1], L, R, scale)
    return Ref(gZ, float(gs), o["B"], float(o["Bs"].sum()), j0, j1)


def reference_dense(Z, S, scale, j0, j1, precise=False):
    """The same pair for an explicit symmetric weight matrix S: d/dZ, d/dscale of 1/2 sum(S * K); the bound uses |S|."""
    o = _columns64(Z, [_weights64(None, None, S, None)], scale, list(range(j0, j1)), None, precise)[0]
    return Ref(o["gZ"], float(o["gs"].sum()), o["B"], float(o["Bs"].sum()), j0, j1)


class Bank:
    """Every column of the reference for several weight sets over ONE Z, computed once: `weights` maps a key to (L, R) or
    to an explicit S; `ref(key, j0, j1)` is `reference(...)` / `reference_dense(...)` for that key."""

    def __init__(self, Z, weights, scale, rows=None, precise=False):
        self.Z = np.asarray(Z, dtype=np.float64)
        self.rows = None if rows is None else np.asarray(rows)
        self.keys = list(weights)
        ws = [_weights64(w[0], w[1], None, self.rows) if isinstance(w, tuple) else _weights64(None, None, w, self.rows)
              for w in weights.values()]
        self.out = dict(zip(self.keys, _columns64(self.Z, ws, scale, list(range(self.Z.shape[1])), self.rows, precise)))

    def ref(self, key, j0, j1):
        o = self.out[key]
        if self.rows is not None:
            return Ref(o["gZ"][:, j0:j1], None, o["B"][:, j0:j1], None, j0, j1, self.rows)
        return Ref(o["gZ"][:, j0:j1], float(o["gs"][j0:j1].sum()), o["B"][:, j0:j1], float(o["Bs"][j0:j1].sum()), j0, j1)


class RestateBank:
    """`restate_f32` column by column for several weight sets over one Z (see `Bank`): `weights` maps a key to (L, R) or
    to an explicit S; `get(key, j0, j1)` is `restate_f32(...)` for that key, bit for bit."""

    def __init__(self, Z, weights, scale):
        f = np.float32
        k = f(KEXP2)
        Zs = np.asarray(Z, dtype=f) * k
        N, J = Zs.shape
        Ss = {}
        for key, w in weights.items():
            if isinstance(w, tuple):
                L = np.asarray(w[0], dtype=f).reshape(N, -1)
                R = np.asarray(w[1], dtype=f).reshape(N, -1)
                Ss[key] = L @ R.T + R @ L.T
            else:
                Ss[key] = np.asarray(w, dtype=f)
        self.gZ = {key: np.zeros((N, J), dtype=f) for key in Ss}
        self.rowS = {key: np.zeros((J, N), dtype=f) for key in Ss}
        mul = f(-scale) / k
        for j in range(J):
            d = Zs[:, j][:, None] - Zs[:, j][None, :]
            e = np.exp2(-(d * d))
            d *= e
            for key, S in Ss.items():
                self.gZ[key][:, j] = np.cumsum(S * d, axis=1, dtype=f)[:, -1] * mul
                self.rowS[key][j] = np.cumsum(S * e, axis=1, dtype=f)[:, -1]

    def get(self, key, j0, j1):
        f = np.float32
        rowS = np.zeros(self.gZ[key].shape[0], dtype=f)
        for j in range(j0, j1):
            rowS += self.rowS[key][j]
        return self.gZ[key][:, j0:j1].copy(), f(0.5) * np.cumsum(rowS, dtype=f)[-1]


def restate_f32(Z, L, R, scale, j0, j1, S=None):
    """The same sum in float32 on the CPU with the kernels' arithmetic: Z pre-scaled by sqrt(log2(e) / 2), exp2(-d^2), S
    formed in float32 (or given), a sequential float32 running sum over the columns (np.cumsum(..., dtype=float32)[:, -1]).
    Returns (gZ [N x (j1 - j0)], gscale)."""
    Z = np.asarray(Z)[:, j0:j1]
    return RestateBank(Z, {0: (L, R) if S is None else S}, scale).get(0, 0, j1 - j0)


def ratios(got_gZ, ref, u):
    """Entrywise |got - ref| / (u B) over the slice (0 where both the error and the bound vanish)."""
    got = _slice_of(np.asarray(got_gZ, dtype=np.float64), ref)
    err = np.abs(got - ref.gZ)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / (u * ref.B)
    r[(err == 0) & (ref.B == 0)] = 0.0
    return r


def _slice_of(got, ref):
    if ref.rows is not None and got.shape[0] != len(ref.rows):
        got = got[ref.rows]
    if got.shape[1] != ref.j1 - ref.j0:
        got = got[:, ref.j0:ref.j1]
    return got


def check(got_gZ, got_gs, ref, c, u, case="", outside=None):
    """Every gate of the module docstring; raises CheckFailure naming the case, the first offending (row, column) and
    the ratio, with `.gates` listing every gate that fired.  `got_gZ`: the slice itself or the full-width array (then
    `outside`, when given, is the value every column outside [j0, j1) must still hold exactly: the caller's sentinel, or
    0 where `ops` allocates).  `got_gs=None` skips gscale (row-subset references carry none).  Returns the figures."""
    if not c <= C_CAP:
        raise ValueError("c = %g exceeds the cap %g" % (c, C_CAP))
    gate = GATES[u]
    full = np.asarray(got_gZ, dtype=np.float64)
    got = _slice_of(full, ref)
    rowid = (lambda i: int(i)) if ref.rows is None else (lambda i: int(ref.rows[i]))
    fails, gates = [], []

    def fail(name, msg):
        gates.append(name)
        fails.append("[%s] %s" % (name, msg))

    if not np.isfinite(got).all():
        i, j = np.argwhere(~np.isfinite(got))[0]
        fail("nan", "non-finite entry at (%d, %d)" % (rowid(i), ref.j0 + j))
    rel = np.linalg.norm(got - ref.gZ) / np.linalg.norm(ref.gZ)
    if not rel < gate:
        fail("norm", "relative 2-norm of the slice %.3e >= %.1e" % (rel, gate))
    col = np.linalg.norm(got - ref.gZ, axis=0) / np.linalg.norm(ref.gZ, axis=0)
    if not (col < gate).all():
        j = int(np.argmax(~(col < gate)))
        fail("column", "relative 2-norm of column %d is %.3e >= %.1e" % (ref.j0 + j, col[j], gate))
    r = ratios(got, ref, u)
    bad = ~(r <= c)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        fail("entry", "first entry beyond c u B at (row %d, column %d): |got - ref| / (u B) = %.4g > c = %g (largest %.4g, "
             "%d entries)" % (rowid(i), ref.j0 + j, r[i, j], c, np.nanmax(r), int(bad.sum())))
    gs_ratio = None
    if got_gs is not None:
        gs_ratio = abs(float(got_gs) - ref.gs) / (u * ref.Bs)
        if not gs_ratio <= c:
            fail("gscale", "|gs - ref| / (u Bs) = %.4g > c = %g (got %.9g, reference %.9g)" % (gs_ratio, c, float(got_gs), ref.gs))
    if outside is not None and full.shape[1] != ref.j1 - ref.j0:
        keep = np.ones(full.shape[1], dtype=bool)
        keep[ref.j0:ref.j1] = False
        out = full[:, keep]
        wrong = ~(out == outside)
        if wrong.any():
            i, j = np.argwhere(wrong)[0]
            fail("outside", "column %d outside [%d, %d) changed at row %d: %r instead of %r"
                 % (int(np.flatnonzero(keep)[j]), ref.j0, ref.j1, int(i), out[i, j], outside))
    if fails:
        raise CheckFailure("%s: %s" % (case, "; ".join(fails)), gates)
    return {"ratio": float(r.max()), "gs_ratio": gs_ratio, "rel": float(rel), "col_rel": float(col.max())}


# ---- the cases of tests/test_bilinear_arms_gpu.py (the host module restates those with N <= 2300) ----------------
SCALE = 0.05
S1 = [(0, 7), (7, 14), (14, 20)]
S2 = [(0, 3), (3, 7), (7, 17), (17, 20)]
S3 = [(2, 10)]
S4 = [(0, 20)]
S5 = [(5, 6), (6, 8)]
ALL_SETS = S1 + S2 + S3 + S4 + S5
# N -> {T: slices}: the size regimes of the float32 derivative on a J = 20 matrix (full-matrix references)
F32_TABLE = {
    300: {1: S1 + S2 + S5, 3: S1 + S2 + S5, 12: S1 + S2 + S5},             # plain sweep, bilinear_kernel<JT, 1 / 4 / 12>
    2047: {4: S1 + S4},                                                   # last N of the plain sweep
    2048: {1: ALL_SETS, 4: ALL_SETS, 5: ALL_SETS, 12: ALL_SETS},          # first N of the symmetric sweep, TT = 4 and 12
    2300: {1: ALL_SETS, 4: ALL_SETS, 11: ALL_SETS, 13: S1, 24: S1},       # ragged; 13 / 24: 12-column accumulation in ops
}


def inputs(N, J, Ts, seed=None, dtype=np.float32):
    """Seeded Z ~ 0.8 N(0, 1) [N x J] and, per T in Ts, L, R ~ 0.1 N(0, 1) [N x T] (the distributions of
    test_bil_asm_gpu.py)."""
    rng = np.random.default_rng(N if seed is None else seed)
    Z = (0.8 * rng.standard_normal((N, J))).astype(dtype)
    LR = {}
    for T in Ts:
        r = np.random.default_rng(1000 * T + N)
        LR[T] = ((0.1 * r.standard_normal((N, T))).astype(dtype), (0.1 * r.standard_normal((N, T))).astype(dtype))
    return Z, LR


def symmetric_weights(N, seed, dtype=np.float32):
    A = 0.01 * np.random.default_rng(seed).standard_normal((N, N))
    return (A + A.T).astype(dtype)


STRIDED_N, STRIDED_J, STRIDED_T, STRIDED_SLICES = (2300, 300), 7, 4, [(0, 7), (2, 7)]       # the C-ABI with ldz = 10, ldg = 12
DENSE_N = 1100
