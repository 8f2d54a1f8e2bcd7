"""Float64 step-by-step reference, condition bound and checker of the pivoted-Cholesky factor (rpgp_pivoted_cholesky,
rpgp_family_pivoted_cholesky, rpgp_ski_pivoted_cholesky; include/rpgp.h) — plain numpy (scipy.sparse through
oracle/ski.py for the grid operator), no device code, in the spirit of tests/cg_reference.py and tests/bilinear_reference.py.

A float64 factor with its own pivots cannot be compared entry by entry: the exact kernel's residual diagonal starts
constant, near-ties are legitimate, and once a pivot differs every later column does.  So `check` holds ONE STEP AT A TIME
to float64, on the factor's own earlier columns: with L the result cast to float64, K the float64 kernel of the float32
inputs (only its diagonal and the column K[:, p] are ever formed: O(N (J + m)) per step) and, for step m,

    S_i = sum_{q<m} L[i,q]^2        R_i = K_ii - S_i   (0 where i has been a pivot: the kernels set that entry to 0)

  pivot   p = argmax_i |L[i,m]| (smallest index on ties; the residual is PSD, so |l_i| <= l_p): L[p,m] must be positive
          and must be the square root of R_p to the entry bound below                                      [gate "pivot"]
  repeat  p must not be an earlier pivot                                                                    [gate "repeat"]
  greedy  max_i R_i - R_p <= (2m + 2) u [(K_aa + S_a) + (K_pp + S_p)], a = the argmax, u = 2^-24: a running diagonal
          entry is m rounded squares subtracted (rounded) from a start rounded twice (scale * weight sum)   [gate "greedy"]
          The grid operator is held to the same bound: its start is a computed entry (rpgp_ski_diag), but the diagonal of
          W T W^T depends on the tap fraction only through the interpolation ripple, so the float32 tap position that widens
          the off-diagonal entries does not reach it (restatement: gap / bound <= 0.3 on every grid case).
  column  d_p = R_p,  ref_i = (K[i,p] - sum_{q<m} L[i,q] L[p,q]) / sqrt(d_p)
          B_i = (Ksens[i,p] + sum_{q<m} |L[i,q]| |L[p,q]|) / sqrt(d_p) + |ref_i| (K_pp + S_p) / d_p
          |L[i,m] - ref_i| <= C u B_i for every i                                                           [gate "entry"]
          (the last term of B: the kernel divides by its float32 RUNNING d_p, the reference by the recomputed one)
  exhaustion  where max_i R_i <= 1e-10 d0 + the greedy bound, the kernel's `ok` flag may have fallen either way: a zero
          column and a non-zero one are both accepted and the step is not checked further.  Where max_i R_i is exactly 0
          (every row has been a pivot: N < rank) the column must be exactly zero                            [gate "zero"]
  non-finite entries                                                                                        [gate "nan"]

A step whose d_p / d0 is below RESOLVED_FLOOR = 1e-2 is recorded as skipped (its column is only held to the pivot, repeat
and greedy rules): the one-step bound is first order in u (K_pp + S_p) / d_p, and the running d_p has by then taken up m
roundings of size u d0.  Main cases are RESOLVED — the host module asserts from the reference side alone that the float32
restatement's smallest d_p / d0 is at least RESOLVED_FLOOR — so no GPU case passes by skipping.  One listed case cannot be:
(N, J, rank) = (2305, 1, 16), a single 1-D RBF, whose residual diagonal falls to 3e-2 d0 at step 7, 9e-3 at step 8 and
5e-5 at step 12 (restatement; steps 13 - 15 are exhausted).  It runs as listed with its first eight steps held to every
gate (`main` false), next to (2305, 1, 8): the same eight steps, resolved, with the factor's other row stride.

Ksens[i,p] is the entry's sensitivity to a relative u perturbation of each term and of each term's argument:
  RBF (groups: r^2 over the group's columns)   sum_c |w_c| e_c (1 + r_c^2 / 2)
  other kinds, phi(t) of t = |z_ic - z_pc|       sum_c |w_c| (|phi| + |t phi'(t)|)
  grid interpolation                             sum_j |w_j| sum_{q,q'} [ Tsens[lag] |w_q w'_q'|
                                                          + 2 |T[lag]| (u_i |w'_q' dw_q| + u_p |w_q dw'_q'|) ]
    with Tsens = |T| + |t T'(t)| at t = lag h (the Toeplitz entry is the sub-kernel of a rounded product lag * h), dw = d w / d fr
    the derivative of a tap weight with respect to the tap fraction, and u_i = (z_i - g0) (1/h) the tap position of row i, a
    float32 number of size up to G.  The kernels form it from a rounded difference and a rounded product, each wrong by up
    to u u_i, so the fraction fr = u - floor(u) carries an ABSOLUTE error of up to 2 u u_i <= 2 u G however small fr is: in
    units of u that is 2 u_i, taken per row here instead of the 2 G that bounds it.  The 1/h the kernels multiply by is the
    grid block's own float32 entry, an INPUT: the float64 side interpolates at (z - g0) * (1/h) with that very number
    (oracle.ski.interp_sparse with spacing 1 / (1/h)), not at (z - g0) / h, which would add a third, systematic, u u_i that
    is no rounding of the kernel's.  The Toeplitz lags use h, as the kernels do.  This term dominates the bound (several
    hundred against 1): float32 tap positions on a grid of 512 points resolve an entry to about 3e-5 of its size, and no
    check of these kernels can be sharper than that.

The constant C is MEASURED on the host (tests/test_pivchol_reference_host.py), per operator kind: `restate_f32` is the same
greedy loop in float32 with the kernels' arithmetic (inputs pre-scaled by sqrt(log2(e) / 2), exp2(-d^2), an fma correction
sum in column order, (row - corr) * (1 / sqrt(d_p)), clamp at 0, the pivot's entry zeroed); its largest entrywise ratio over
the inputs of every GPU case is c_ref and C = 16 c_ref rounded up to a power of two, never more than C_CAP = 256: a stale
row moves the ratio to 1e5 and more."""
import numpy as np

from oracle import family as fam_oracle
from oracle import ski as sko

U32 = 2.0 ** -24
KEXP2 = 0.8493218002880191            # sqrt(0.5 * log2(e)):  exp(-d^2 / 2) = exp2(-(KEXP2 d)^2)
C_CAP = 256.0
RESOLVED_FLOOR = 1e-2                 # smallest d_p / d0 of a main case (asserted on the restatement by the host module);
                                      # a step below it is recorded as skipped
# the constants of the entrywise gate in use, per operator kind: 16 c_ref rounded up to a power of two.  The host module
# measures c_ref on its CPU (written beside each) and asserts that whatever it measures still gives these constants.
C = {"rbf": 128.0,                    # c_ref = 7.28 (N = 1025, J = 64, rank 64)
     "family": 128.0,                 # c_ref = 4.92 (Cosine, N = 2049)
     "grid": 32.0}                    # c_ref = 1.84 (N = 65536, J = 3, rank 16)
PRE = {"RBF": KEXP2, "Matern": 1.7320508075688772, "InverseMQ": 1.0, "Cosine": 0.5}       # Phi<>::pre of the kernels


def c_from(c_ref):
    """The constant of the GPU tests: 16 c_ref rounded up to a power of two (see the module docstring)."""
    return float(2.0 ** np.ceil(np.log2(16.0 * c_ref)))


class CheckFailure(AssertionError):
    """`gates`: the names of every gate that fired ("pivot", "repeat", "greedy", "entry", "zero", "nan"); `ratios`: per
    fired gate its largest figure — entry / pivot: |l - ref| / (u B); greedy: gap / (u [(K_aa + S_a) + (K_pp + S_p)])."""

    def __init__(self, message, gates, ratios, records=()):
        super().__init__(message)
        self.gates = tuple(gates)
        self.ratios = dict(ratios)
        self.records = list(records)                   # the per-step records up to the last step looked at


def _fma32(a, b, c):
    """float32 fma: the product of two float32 numbers is exact in float64."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


# ---- sub-kernels: value and |t phi'(t)| in float64, the kernels' arithmetic in float32 ---------------------------------
def _phi_sens(kind, r):
    """|phi(r)| + |r phi'(r)| of a non-RBF 1-D sub-kernel (oracle.family._phi is the value)."""
    r = np.abs(r)
    if kind == "Matern":
        s = np.sqrt(3.0) * r
        return (1.0 + s) * np.exp(-s) + s * s * np.exp(-s)
    if kind == "InverseMQ":
        return (1.0 + r * r) ** -0.5 + r * r * (1.0 + r * r) ** -1.5
    if kind == "Cosine":
        return np.abs(np.cos(np.pi * r)) + np.abs(np.pi * r * np.sin(np.pi * r))
    if kind == "RBF":
        return np.exp(-0.5 * r * r) * (1.0 + r * r)
    raise ValueError("Unknown kernel type")


def _phi_f32(kind, dd):
    """Phi<kind>::val of the pre-scaled float32 difference dd (csrc/rpgp_tile.h)."""
    f = np.float32
    if kind == "RBF":
        return np.exp2(-(dd * dd))
    if kind == "Matern":
        a = np.abs(dd)
        return (f(1.0) + a) * np.exp2(f(-1.4426950408889634) * a)
    if kind == "InverseMQ":
        return f(1.0) / np.sqrt(_fma32(dd, dd, f(1.0)))
    if kind == "Cosine":                                # the hardware cosine takes revolutions
        return np.cos(f(2.0 * np.pi) * (dd - np.floor(dd))).astype(f)
    raise ValueError("Unknown kernel type")


def _radial_f32(kind, lag, h):
    """ski_radial_f32 (csrc/rpgp_ski_common.h): the sub-kernel between grid points `lag` spacings apart."""
    f = np.float32
    lag = lag.astype(f)
    if kind == "RBF":
        return _phi_f32("RBF", lag * (f(h) * f(KEXP2)))
    d = lag * f(h)
    if kind == "Matern":
        s = f(1.7320508075688772) * d
        return (f(1.0) + s) * np.exp2(f(-1.4426950408889634) * s)
    if kind == "InverseMQ":
        return f(1.0) / np.sqrt(_fma32(d, d, f(1.0)))
    return _phi_f32("Cosine", f(0.5) * d)


# ---- column providers (unscaled: `check` and `restate_f32` multiply by scale) ------------------------------------------
class FamilyProvider:
    """K = sum_c w_c phi_kind(group c of the columns of Z) (oracle/family.py); kind "RBF", group 1, no weights: the exact
    operator.  `pre`: the pre-scale of the float32 restatement (the mutation self-test swaps it)."""

    def __init__(self, Z, kind="RBF", group=1, weights=None, pre=None):
        self.Z32 = np.ascontiguousarray(Z, dtype=np.float32)
        self.Z = self.Z32.astype(np.float64)
        self.N, cols = self.Z.shape
        self.kind, self.group, self.ncomp = kind, int(group), cols // int(group)
        if kind != "RBF" and self.group != 1:
            raise ValueError("the pivoted-Cholesky kernels take groups of the RBF only")
        self.w32 = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        self.w = np.ones(self.ncomp) if weights is None else self.w32.astype(np.float64)
        self.name = "rbf" if (kind == "RBF" and self.group == 1 and weights is None) else "family"
        self.d0 = float(self.w.sum())                  # phi(0) = 1 for every kind
        self.pre = np.float32(PRE[kind] if pre is None else pre)
        self.grid_like = False

    def diag(self):
        return np.full(self.N, self.d0), None

    def column(self, p):
        Z, g = self.Z, self.group
        k, s = np.zeros(self.N), np.zeros(self.N)
        for c in range(self.ncomp):
            d = Z[:, c * g:(c + 1) * g] - Z[p, c * g:(c + 1) * g]
            r2 = (d * d).sum(axis=1)
            if self.kind == "RBF":
                e = np.exp(-0.5 * r2)
                k += self.w[c] * e
                s += abs(self.w[c]) * e * (1.0 + 0.5 * r2)
            else:
                k += self.w[c] * fam_oracle._phi(self.kind, r2)
                s += abs(self.w[c]) * _phi_sens(self.kind, np.sqrt(r2))
        return k, s

    def diag_f32(self, scale):
        return np.full(self.N, np.float32(scale) * np.float32(self.d0), dtype=np.float32)

    def column_f32(self, p, scale):
        f = np.float32
        Zs, g = self.Z32 * self.pre, self.group
        acc = np.zeros(self.N, dtype=f)
        for c in range(self.ncomp):
            if g == 1:
                phi = _phi_f32(self.kind, Zs[:, c] - Zs[p, c])
            else:
                r2 = np.zeros(self.N, dtype=f)
                for q in range(g):
                    dd = Zs[:, c * g + q] - Zs[p, c * g + q]
                    r2 = _fma32(dd, dd, r2)
                phi = np.exp2(-r2)
            acc = acc + phi if self.w32 is None else _fma32(self.w32[c], phi, acc)
        return f(scale) * acc


def _cubic_d(U):
    """|d/dU| of oracle.ski._cubic."""
    U = np.abs(U)
    return np.abs(np.where(U < 1.0, (4.5 * U - 5.0) * U, (-1.5 * U + 5.0) * U - 4.0))


def host_grid_block(Z, G, rule="shared"):
    """(g0 [J], h [J], 1/h [J]) in float32 of a coordinate matrix: the rules of oracle/ski.py rounded the way the device's
    grid block holds them (the GPU tests read the device's own block instead)."""
    Z = np.asarray(Z, dtype=np.float64)
    J = Z.shape[1]
    g0, h = sko.grid_params_reference(Z, None, G) if rule == "reference" else sko.grid_params(Z, None, G)
    g0 = np.broadcast_to(np.asarray(g0, dtype=np.float32), (J,)).copy()
    h = np.broadcast_to(np.asarray(h, dtype=np.float32), (J,)).copy()
    return g0, h, (np.float32(1.0) / h).astype(np.float32)


class GridProvider:
    """K = sum_j w_j W_j T_j W_j^T: W_j from oracle.ski.interp_sparse, T_j from oracle.ski.toeplitz, on the float32 grid
    block `grid` = (g0 [J], h [J], 1/h [J]): tap positions (z - g0) * (1/h), Toeplitz lags lag * h, on both sides (see the
    module docstring)."""

    name = "grid"

    def __init__(self, Z, grid, G, kind="RBF", weights=None):
        self.Z32 = np.ascontiguousarray(Z, dtype=np.float32)
        self.Z = self.Z32.astype(np.float64)
        self.N, self.J = self.Z.shape
        self.G, self.kind = int(G), kind
        self.g0, self.h, self.inv_h = (np.asarray(a, dtype=np.float32).reshape(-1) for a in grid)
        self.w32 = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        self.w = np.ones(self.J) if weights is None else self.w32.astype(np.float64)
        self.d0 = float(self.J)                        # what the kernels measure exhaustion against
        self.grid_like = True
        self._T = {}
        self.W, self.Wa, self.dW, self.idx0, self.vals, self.dvals = [], [], [], [], [], []
        import scipy.sparse as sp
        for j in range(self.J):
            g0, hpos = float(self.g0[j]), 1.0 / float(self.inv_h[j])
            W = sko.interp_sparse(self.Z[:, j], g0, hpos, self.G)
            u = np.clip((self.Z[:, j] - g0) / hpos, 1.0, self.G - 2.0)
            fr = u - np.floor(u)
            # |d w / d fr| times the tap position: the weight's sensitivity to the float32 position, in units of u / 2
            dv = u[:, None] * np.stack([_cubic_d(fr + 1.0), _cubic_d(fr), _cubic_d(1.0 - fr), _cubic_d(2.0 - fr)], axis=1)
            self.W.append(W)
            self.Wa.append(abs(W))
            self.dW.append(sp.csr_matrix((dv.ravel(), W.indices, W.indptr), shape=W.shape))
            self.idx0.append(W.indices[::4].astype(np.int64))
            self.vals.append(W.data.reshape(-1, 4))
            self.dvals.append(dv)

    def _toep(self, j):
        """(T, |T|, Tsens) of projection j (cached per spacing)."""
        h = float(self.h[j])
        if h not in self._T:
            T = sko.toeplitz(h, self.G, self.kind)
            m = np.arange(self.G)
            r = np.abs(m[:, None] - m[None, :]) * h
            self._T[h] = (T, np.abs(T), _phi_sens(self.kind, r))
        return self._T[h]

    def diag(self):
        """(K_ii, Dsens_ii): the 4 x 4 quadratic form of a row's own taps."""
        k, s = np.zeros(self.N), np.zeros(self.N)
        for j in range(self.J):
            h = float(self.h[j])
            lag = np.arange(4) * h
            t = fam_oracle._phi(self.kind, lag * lag)
            ts = _phi_sens(self.kind, lag)
            v, a, dv = self.vals[j], np.abs(self.vals[j]), self.dvals[j]
            for q in range(4):
                for qq in range(4):
                    k += self.w[j] * v[:, q] * v[:, qq] * t[abs(q - qq)]
                    s += abs(self.w[j]) * (a[:, q] * a[:, qq] * ts[abs(q - qq)]
                                           + 4.0 * abs(t[abs(q - qq)]) * a[:, qq] * dv[:, q])
        return k, s

    def column(self, p):
        k, s = np.zeros(self.N), np.zeros(self.N)
        for j in range(self.J):
            T, Ta, Ts = self._toep(j)
            cols = slice(self.idx0[j][p], self.idx0[j][p] + 4)
            vp, ap, dp = self.vals[j][p], np.abs(self.vals[j][p]), self.dvals[j][p]
            k += self.w[j] * (self.W[j] @ (T[:, cols] @ vp))
            s += abs(self.w[j]) * (self.Wa[j] @ (Ts[:, cols] @ ap)
                                   + 2.0 * (self.dW[j] @ (Ta[:, cols] @ ap) + self.Wa[j] @ (Ta[:, cols] @ dp)))
        return k, s

    def _taps_f32(self, j):
        f = np.float32
        u = (self.Z32[:, j] - self.g0[j]) * self.inv_h[j]
        u = np.minimum(np.maximum(u, f(1.0)), f(self.G - 2))
        fl = np.floor(u)
        fr = u - fl
        idx0 = np.clip(fl.astype(np.int64) - 1, 0, self.G - 4)

        def cub(U):
            return np.where(U < f(1.0), ((f(1.5) * U - f(2.5)) * U) * U + f(1.0), ((f(-0.5) * U + f(2.5)) * U - f(4.0)) * U + f(2.0))
        return idx0, np.stack([cub(fr + f(1.0)), cub(fr), cub(f(1.0) - fr), cub(f(2.0) - fr)], axis=1).astype(f)

    def _f32(self):
        if not hasattr(self, "_taps"):
            self._taps = [self._taps_f32(j) for j in range(self.J)]
        return self._taps

    def diag_f32(self, scale):
        f = np.float32
        acc = np.zeros(self.N, dtype=f)
        for j, (idx0, w) in enumerate(self._f32()):
            c = _radial_f32(self.kind, np.arange(4), self.h[j])
            aj = np.zeros(self.N, dtype=f)
            for q in range(4):
                for qq in range(4):
                    aj = _fma32(w[:, q] * w[:, qq], c[abs(q - qq)], aj)
            acc = _fma32(f(1.0) if self.w32 is None else self.w32[j], aj, acc)
        return f(scale) * acc

    def column_f32(self, p, scale):
        f = np.float32
        acc = np.zeros(self.N, dtype=f)
        for j, (idx0, w) in enumerate(self._f32()):
            delta = idx0 - idx0[p]
            tl = [_radial_f32(self.kind, np.abs(delta + t - 3), self.h[j]) for t in range(7)]
            aj = np.zeros(self.N, dtype=f)
            for q in range(4):
                for qq in range(4):
                    aj = _fma32(w[:, q] * w[p, qq], tl[q - qq + 3], aj)
            acc = _fma32(f(1.0) if self.w32 is None else self.w32[j], aj, acc)
        return f(scale) * acc


# ---- the float32 restatement of the greedy loop --------------------------------------------------------------------------
def restate_f32(provider, scale, rank, mutate=None):
    """The greedy loop of the kernels in float32 (see the module docstring): L [N x rank] float32.  `mutate` (the host
    module's self-test): {"drop_last_corr": m} leaves the last term out of step m's correction sum, {"row_off": m} takes
    step m's kernel column from the row after the pivot, {"second_best": m} forces the second-largest diagonal entry."""
    f = np.float32
    mutate = mutate or {}
    N = provider.N
    d = provider.diag_f32(scale).astype(f)
    d0 = f(scale) * f(provider.d0)
    L = np.zeros((N, rank), dtype=f)
    for m in range(rank):
        p = int(np.argmax(d))
        if mutate.get("second_best") == m:
            p = int(np.argsort(-d, kind="stable")[1])
        dp = d[p]
        if dp > f(1e-10) * d0:
            src = p + 1 if mutate.get("row_off") == m else p
            row = provider.column_f32(src % N, scale)
            corr = np.zeros(N, dtype=f)
            last = m - 1 if mutate.get("drop_last_corr") == m else m
            for q in range(last):
                corr = _fma32(L[:, q], L[p, q], corr)
            l = (row - corr) * (f(1.0) / np.sqrt(dp))
        else:
            l = np.zeros(N, dtype=f)
        L[:, m] = l
        nd = d - l * l
        nd[nd < 0] = f(0.0)
        nd[p] = f(0.0)
        d = nd
    return L


# ---- the checker ---------------------------------------------------------------------------------------------------------
def check(L, provider, scale, c=None, case=""):
    """Every gate of the module docstring on the factor L [N x rank] of scale * K(provider); `c`: the constant of the
    entrywise gate (default: the provider kind's).  Returns the per-step records {"step", "pivot", "dp_d0", "ratio", "gap",
    "bound", "skipped", "exhausted"}; raises CheckFailure naming the case, the step and the first offending row."""
    c = C[provider.name] if c is None else float(c)
    if not c <= C_CAP:
        raise ValueError("c = %g exceeds the cap %g" % (c, C_CAP))
    L = np.asarray(L, dtype=np.float64)
    N, rank = L.shape
    assert N == provider.N
    scale = float(np.float32(scale))
    Kd = scale * provider.diag()[0]
    d0 = scale * provider.d0
    S = np.zeros(N)
    is_piv = np.zeros(N, dtype=bool)
    pivots, records, fails, gates, ratios = [], [], [], [], {}

    def fail(name, msg, ratio=None):
        if name not in gates:
            gates.append(name)
        if ratio is not None:
            ratios[name] = max(ratios.get(name, 0.0), float(ratio))
        if len(fails) < 8:
            fails.append("[%s] %s" % (name, msg))

    for m in range(rank):
        col = L[:, m]
        rec = {"step": m, "pivot": None, "dp_d0": None, "ratio": None, "gap": None, "bound": None, "skipped": False,
               "exhausted": False}
        records.append(rec)
        if not np.isfinite(col).all():
            fail("nan", "step %d: non-finite entry at row %d" % (m, int(np.argmax(~np.isfinite(col)))))
            break
        R = np.where(is_piv, 0.0, Kd - S)
        a = int(np.argmax(R))
        if is_piv.all():                                           # every row has been a pivot: nothing is left
            rec["exhausted"] = True
            if (col != 0.0).any():
                fail("zero", "step %d: every row has been a pivot, yet row %d holds %r" % (m, int(np.argmax(col != 0.0)),
                                                                                       col[np.argmax(col != 0.0)]))
            continue
        p = int(np.argmax(np.abs(col)))
        gsum = (Kd[a] + S[a]) + (Kd[p] + S[p])
        bound = (2 * m + 2) * U32 * gsum
        if R[a] <= 1e-10 * d0 + bound:                             # exhausted: the `ok` flag may have fallen either way
            rec["exhausted"] = True
            if (col != 0.0).any():
                is_piv[p] = True
                pivots.append(p)
                S += col * col
            continue
        rec.update(pivot=p, dp_d0=R[p] / d0, gap=R[a] - R[p], bound=bound)
        if p in pivots:
            fail("repeat", "step %d: row %d was the pivot of step %d already" % (m, p, pivots.index(p)))
        if R[a] - R[p] > bound:
            fail("greedy", "step %d: pivot %d leaves R = %.9g while row %d holds %.9g: gap %.3e > bound %.3e"
                 % (m, p, R[p], a, R[a], R[a] - R[p], bound), (R[a] - R[p]) / (U32 * gsum))
        dp = R[p]
        if not col[p] > 0.0:
            fail("pivot", "step %d: L[%d, %d] = %r with R_p = %r" % (m, p, m, col[p], dp))
        elif dp / d0 < RESOLVED_FLOOR:
            rec["skipped"] = True
        else:
            k, ks = provider.column(p)
            Lp = L[p, :m]
            ref = (scale * k - L[:, :m] @ Lp) / np.sqrt(dp)
            B = (scale * ks + np.abs(L[:, :m]) @ np.abs(Lp)) / np.sqrt(dp) + np.abs(ref) * (Kd[p] + S[p]) / dp
            err = np.abs(col - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = err / (U32 * B)
            r[(err == 0.0) & (B == 0.0)] = 0.0
            rec["ratio"] = float(np.nanmax(r))
            if not r[p] <= c:
                fail("pivot", "step %d: L[%d, %d] = %.9g is not sqrt(R_p) = %.9g: ratio %.4g > c = %g"
                     % (m, p, m, col[p], np.sqrt(dp), r[p], c), r[p])
            bad = ~(r <= c)
            if bad.any():
                i = int(np.argmax(bad))
                fail("entry", "step %d (pivot %d, d_p/d0 = %.3e): first entry beyond c u B at row %d: got %.9g, reference %.9g, "
                     "|got - ref| / (u B) = %.4g > c = %g (largest %.4g, %d rows)"
                     % (m, p, dp / d0, i, col[i], ref[i], r[i], c, np.nanmax(r), int(bad.sum())), np.nanmax(r))
        is_piv[p] = True
        pivots.append(p)
        S += col * col
    if fails:
        raise CheckFailure("%s: %s" % (case, "; ".join(fails)), gates, ratios, records)
    return records


def summary(records):
    """(worst ratio, smallest d_p / d0, share of skipped steps among those not exhausted) of one case's records."""
    live = [r for r in records if not r["exhausted"]]
    rat = [r["ratio"] for r in live if r["ratio"] is not None]
    dp = [r["dp_d0"] for r in live if r["dp_d0"] is not None]
    return (max(rat) if rat else 0.0, min(dp) if dp else float("inf"),
            sum(r["skipped"] for r in live) / max(len(live), 1))


def assert_resolved(case, records):
    """The first `live` steps of a case (all of them in a main case with N >= rank) are neither skipped nor exhausted and
    keep d_p / d0 >= RESOLVED_FLOOR.  What follows them in the one unresolved case is held to whatever gates `check` applied
    (a step near the floor may fall on either side of it); with N < rank the steps from N on are exhausted."""
    lead = records[:case["live"]]
    assert not any(r["skipped"] or r["exhausted"] for r in lead), case["id"]
    assert min(r["dp_d0"] for r in lead) >= RESOLVED_FLOOR, case["id"]
    assert all(r["exhausted"] for r in records[case["N"]:]), case["id"]


def show(case, records):
    """One line per step, printed by the GPU module before it asserts."""
    for r in records:
        if r["exhausted"] or r["pivot"] is None:
            print("%s step %2d: %s" % (case, r["step"], "exhausted" if r["exhausted"] else "not looked at"))
        else:
            print("%s step %2d: pivot %7d  d_p/d0 %.3e  ratio %s  gap %.2e (bound %.2e)%s"
                  % (case, r["step"], r["pivot"], r["dp_d0"], "   -   " if r["ratio"] is None else "%7.3f" % r["ratio"],
                     r["gap"], r["bound"], "  SKIPPED" if r["skipped"] else ""))


# ---- the cases of tests/test_pivchol_steps_gpu.py (the host module restates them; N above HOST_FULL_N at HOST_N) ----
HOST_FULL_N, HOST_N = 70000, 4099
# path -> [(N, J, rank)]: the exact operator
EXACT = {
    "one_workgroup": [(1, 1, 1), (2, 3, 2), (63, 20, 15), (64, 64, 16), (65, 32, 16), (1024, 20, 15), (1025, 64, 64),
                      (2048, 20, 64)],
    "fast_step": [(2049, 20, 15), (2304, 32, 16), (2305, 1, 16), (2305, 1, 8)],
    "general_step": [(2049, 33, 17), (2304, 20, 64), (9000, 64, 33), (131073, 3, 8), (524289, 2, 3), (524800, 2, 3)],
}
UNRESOLVED = (2305, 1, 16)            # see the module docstring
SMALL_N = (5, 3, 8)                   # one workgroup, N < rank: columns 5 .. 7 exactly zero
LDZ_CASE = (2049, 20, 15, 23)         # fast step through the C entry with ldz = 23
# (kind, group, columns, ranks): the general step kernel's (kind, group, weights) switch, at N = 2049 and N = 300
FAMILY = [("Matern", 1, 6, (12, 17)), ("InverseMQ", 1, 20, (12, 17)), ("Cosine", 1, 3, (4,)), ("RBF", 2, 8, (12, 17))]
FAMILY_N = (2049, 300)
# (N, J, rank, G, sub-kernel, grid rule, weighted)
GRID = {
    "grid_row_major": [(3000, 3, 15, 256, "RBF", "shared", False), (3000, 5, 17, 256, "RBF", "shared", False)],
    "grid_column_major": [(65536, 5, 15, 512, "RBF", "shared", False), (65537, 3, 17, 512, "RBF", "shared", False)],
    "grid_fast": [(65536, 3, 16, 512, "RBF", "shared", False), (65537, 4, 15, 512, "RBF", "reference", False),
                  (70001, 1, 16, 512, "Matern", "shared", False), (65536, 3, 16, 512, "RBF", "shared", True)],
}


def spread_of(N, J):
    """The standard deviation of a case's coordinates: 0.7, 0.8, 0.9 or 1.0."""
    return 0.7 + 0.1 * ((N + J) % 4)


def inputs(N, J, seed=None, host=False):
    """Seeded Z ~ spread N(0, 1) [N x J] float32 and scale = 0.8 / J.  `host`: the host module's size — the same generator
    (seed and spread of the case) at HOST_N rows where the case has more than HOST_FULL_N."""
    rng = np.random.default_rng(1000 * J + N if seed is None else seed)
    n = HOST_N if (host and N > HOST_FULL_N) else N
    return (spread_of(N, J) * rng.standard_normal((n, J))).astype(np.float32), 0.8 / J


def family_weights(ncomp, seed):
    """Weights in [0.3, 1] with one weight 0 (the second component) where there are more than two."""
    w = np.random.default_rng(seed).uniform(0.3, 1.0, size=ncomp).astype(np.float32)
    if ncomp > 2:
        w[1] = 0.0
    return w


def grid_weights(J):
    return np.linspace(0.5, 1.5, J).astype(np.float32) if J > 1 else np.ones(1, dtype=np.float32)


def weight_sum32(w):
    """The weight sum a caller hands to rpgp_family_pivoted_cholesky: summed in float64, rounded once."""
    return float(np.float32(np.asarray(w, dtype=np.float64).sum()))


def cases():
    """Every case of the GPU module as a dict: id, path, op ("exact" | "family" | "grid"), N, J, rank and the operator's
    own fields; `main`: held to RESOLVED_FLOOR and to zero skipped steps."""
    out = []
    for path, lst in EXACT.items():
        for N, J, rank in lst:
            out.append(dict(id="%s-N%d-J%d-r%d" % (path, N, J, rank), path=path, op="exact", N=N, J=J, rank=rank,
                            main=(N, J, rank) != UNRESOLVED))
    N, J, rank = SMALL_N
    out.append(dict(id="one_workgroup-N%d-J%d-r%d" % SMALL_N, path="one_workgroup", op="exact", N=N, J=J, rank=rank, main=True))
    for kind, group, cols, ranks in FAMILY:
        for N in FAMILY_N:
            for rank in ranks:
                out.append(dict(id="family-%s-g%d-c%d-N%d-r%d" % (kind, group, cols, N, rank), path="family", op="family",
                                N=N, J=cols, rank=rank, kind=kind, group=group, main=True))
    for path, lst in GRID.items():
        for N, J, rank, G, kind, rule, weighted in lst:
            out.append(dict(id="%s-N%d-J%d-r%d-G%d-%s-%s%s" % (path, N, J, rank, G, kind, rule, "-weighted" if weighted else ""),
                            path=path, op="grid", N=N, J=J, rank=rank, G=G, kind=kind, rule=rule, weighted=weighted, main=True))
    # N < rank through the general step kernel (the family and the grid operator take it at any N): its `ok == false` branch
    N, J, rank = SMALL_N
    out.append(dict(id="family-Matern-g1-c%d-N%d-r%d" % (J, N, rank), path="family", op="family", N=N, J=J, rank=rank,
                    kind="Matern", group=1, main=True))
    out.append(dict(id="grid_row_major-N%d-J%d-r%d-G64-RBF-shared" % SMALL_N, path="grid_row_major", op="grid", N=N, J=J,
                    rank=rank, G=64, kind="RBF", rule="shared", weighted=False, main=True))
    for c in out:       # `live`: the leading steps that must be resolved; the rest must be skipped or exhausted
        c["live"] = 8 if not c["main"] else min(c["rank"], c["N"])
    return out


def provider_of(case, Z, grid=None):
    """The float64 / float32 column provider of a case on coordinates Z; `grid`: the device's grid block as (g0, h, 1/h)
    arrays (default: `host_grid_block`)."""
    if case["op"] == "exact":
        return FamilyProvider(Z)
    if case["op"] == "family":
        return FamilyProvider(Z, case["kind"], case["group"], family_weights(case["J"] // case["group"], case["J"]))
    grid = host_grid_block(Z, case["G"], case["rule"]) if grid is None else grid
    return GridProvider(Z, grid, case["G"], case["kind"], grid_weights(case["J"]) if case["weighted"] else None)
