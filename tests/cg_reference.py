"""Plain numpy reference for the native mBCG executor (csrc/rpgp_cg.hip), step for step: a float64 preconditioned CG that
returns every alpha, every beta and the iterate after a fixed number of iterations, a kernel operator whose float64 product
is cheap at any N, the case table of tests/test_native_cg_steps_gpu.py, and the bound those tests hold the executor to.
Nothing here touches the GPU: tests/test_cg_reference_host.py checks this file against dense algebra on the CPU.

Why few iterations: CG coefficients of two correct implementations drift apart chaotically after a handful of iterations;
at m = 4 float32 and float64 agree to a few 1e-6, while an error in one column of the preconditioner moves alpha by
percents.  The bound is 8 x the largest float32-to-float64 distance of a plain CPU emulation over the whole case table
(the 8 covers the executor's summation order — float32 per workgroup, float64 across slabs — against numpy's pairwise sums);
it is computed here, from CPU numbers only."""
import functools
import math

import numpy as np

M_ITERS = 4                 # iterations of every step-for-step case
G_LEVELS = 64               # levels per coordinate of the quantised inputs
NOISE = 0.5                 # noise of the system = sigma^2 of the preconditioner
OUTPUTSCALE = 0.9           # kernel scale = OUTPUTSCALE / J
T_MAX = 16                  # a reference is computed for 16 columns; a case with T columns takes the leading T
MARGIN = 8.0
TAME = 1e-4                 # condition 1: every case's own float32-to-float64 distance is below this
SEED = 0                    # of every input
SENSITIVITY = 50.0          # condition 2: dropping the last column of L moves alpha by >= this many alpha bounds


# ---- inputs ----------------------------------------------------------------------------------------------------------------
class QuantisedKernel:
    """s * sum_j exp(-(z_ij - z_kj)^2 / 2) + noise I for coordinates that take G float32 levels per column:
    Z[i, j] = levels[idx[i, j], j].  With S_j the N x G selection matrix of column j the matrix is exactly
    s * sum_j S_j E_j S_j^T + noise I, E_j the G x G float64 Gram matrix of the levels, so a product with an N x T block costs
    O(N T + G^2 T) per column: a histogram, a G x G product, a gather."""

    def __init__(self, N, J, seed):
        rng = np.random.default_rng([seed, N, J])
        self.N, self.J = N, J
        self.scale, self.noise = OUTPUTSCALE / J, NOISE
        self.levels = np.sort(rng.standard_normal((G_LEVELS, J)), axis=0).astype(np.float32)
        self.idx = rng.integers(0, G_LEVELS, size=(N, J))
        self.Z = np.take_along_axis(self.levels, self.idx, axis=0)             # float32 [N, J]
        lv = self.levels.astype(np.float64)
        d = lv[:, None, :] - lv[None, :, :]
        self.E = np.exp(-0.5 * d * d).transpose(2, 0, 1).copy()                # float64 [J, G, G]
        self.E32 = self.E.astype(np.float32)

    def matvec(self, V):
        """float64 product with an N x T block."""
        V = np.asarray(V, dtype=np.float64)
        out = self.noise * V
        H = np.empty((G_LEVELS, V.shape[1]))
        for j in range(self.J):
            ij = self.idx[:, j]
            for t in range(V.shape[1]):
                H[:, t] = np.bincount(ij, weights=V[:, t], minlength=G_LEVELS)
            out += self.scale * (self.E[j] @ H)[ij]
        return out

    def matvec32(self, V):
        """The float32 emulation's product: float32 kernel values, float32 products and sums of the level histogram (which
        numpy only accumulates in float64; it is rounded to float32 before use)."""
        V = np.asarray(V, dtype=np.float32)
        out = np.float32(self.noise) * V
        H = np.empty((G_LEVELS, V.shape[1]), dtype=np.float32)
        for j in range(self.J):
            ij = self.idx[:, j]
            for t in range(V.shape[1]):
                H[:, t] = np.bincount(ij, weights=V[:, t], minlength=G_LEVELS)
            out += np.float32(self.scale) * (self.E32[j] @ H)[ij]
        return out

    def dense(self, noise=True):
        """The dense float64 matrix (small N only), straight from the coordinates."""
        Z = self.Z.astype(np.float64)
        K = np.zeros((self.N, self.N))
        for j in range(self.J):
            d = Z[:, j:j + 1] - Z[:, j:j + 1].T
            K += np.exp(-0.5 * d * d)
        K *= self.scale
        if noise:
            K[np.diag_indices(self.N)] += self.noise
        return K


class DenseKernel:
    """Kd + noise I for a float32 matrix Kd as RPGP_OP_DENSE stores it: the reference runs on Kd.double()."""

    def __init__(self, Kd32, noise):
        self.Kd32, self.Kd, self.noise = Kd32, Kd32.astype(np.float64), noise

    def matvec(self, V):
        V = np.asarray(V, dtype=np.float64)
        return self.Kd @ V + self.noise * V

    def matvec32(self, V):
        V = np.asarray(V, dtype=np.float32)
        return self.Kd32 @ V + np.float32(self.noise) * V


def make_L(N, K, sigma2, seed):
    """Random N x K float32 factor with entries N(0, 2 sigma2 / N): deliberately NOT a pivoted-Cholesky factor.  Any L gives a
    valid SPD M = L L^T + sigma2 I; with this one CG does not converge in three iterations, the betas stay O(1) and every
    column of L matters."""
    if K == 0:
        return None
    rng = np.random.default_rng([seed, N, K, 7])
    return (rng.standard_normal((N, K)) * math.sqrt(2.0 * sigma2 / N)).astype(np.float32)


def make_rhs(N, seed, L=None):
    """N x 16 float32 right-hand sides: Gaussian, plus (with a preconditioner) a Gaussian combination of the columns of L of
    the same norm.  About half of every right-hand side then lies in the range of L, each column of L carries 1 / (2 K) of
    it, and leaving one column out of the preconditioner moves alpha by percents at every N (condition 2); a purely random
    right-hand side has only K / N of itself in that range, and at N = 300 001 one column moved alpha by as little as 4e-4, seed depending."""
    rng = np.random.default_rng([seed, N, 11])
    b = rng.standard_normal((N, T_MAX))
    if L is not None:
        K = L.shape[1]
        b = b + math.sqrt(N / (2.0 * NOISE * K)) * (L.astype(np.float64) @ rng.standard_normal((K, T_MAX)))
    return b.astype(np.float32)


def capacitance_inverse(L, sigma2):
    """Cinv = (sigma2 I + L^T L)^-1 in float64 (what the executor is handed)."""
    Ld = L.astype(np.float64)
    return np.linalg.inv(float(sigma2) * np.eye(L.shape[1]) + Ld.T @ Ld)


# ---- the algorithm ---------------------------------------------------------------------------------------------------------
class PcgResult:
    def __init__(self, x, alpha, beta, resid):
        self.x, self.alpha, self.beta, self.resid = x, alpha, beta, resid
        for a in (x, alpha, beta, resid):
            a.setflags(write=False)                       # shared between tests: nobody edits a reference


def pcg(matvec, B, L, sigma2, m, dtype=np.float64):
    """Preconditioned batched CG exactly as the header of csrc/rpgp_cg.hip states it, `min(m, N)` iterations, no stopping rule:
      columns of B normalised by their float64 norm (norm < 1e-10: a zero column, left unscaled), x0 = 0, r0 = b;
      z = M^-1 r = (r - L Cinv L^T r) / sigma2, Cinv = (sigma2 I + L^T L)^-1 in float64 (L None: z = r);  p0 = z0;
      alpha = r.z / p.Ap;  x += alpha p;  r -= alpha Ap;  z = M^-1 r;  beta = r'.z' / r.z;  p = z + beta p;
      a zero column keeps alpha = 0 (and so x = 0).
    dtype=float64: the reference.  dtype=float32: a plain emulation — float32 vectors, products and sums (numpy's), the
    Woodbury correction L (Cinv (L^T r)) and the subtraction from r in float64 as in pass B — used only to size the bound.
    Returns PcgResult(x un-normalised [N x T] float64, alpha [n_iter x T], beta [n_iter x T], residual norms [T])."""
    f32 = np.dtype(dtype) == np.float32
    B = np.asarray(B)
    N, T = B.shape
    n_iter = min(m, N)
    nrm = np.linalg.norm(B.astype(np.float64), axis=0)
    zero = nrm < 1e-10
    nrm = np.where(zero, 1.0, nrm)
    eps = 1e-30
    if L is not None:
        Ld = L.astype(np.float64)
        Cinv = capacitance_inverse(L, sigma2)

    def precond(r):
        if L is None:
            return r.copy()
        w = (L.T @ r).astype(np.float64) if f32 else Ld.T @ r          # float32 L^T r sums in the emulation
        z = (r.astype(np.float64) - Ld @ (Cinv @ w)) / float(sigma2)
        return z.astype(dtype)

    def coldot(a, b):
        # (summed along contiguous memory: numpy's pairwise summation; a sum over axis 0 of a row-major block is sequential)
        return np.ascontiguousarray((a * b).T).sum(axis=1, dtype=dtype)

    r = (B.astype(dtype) / nrm.astype(dtype)).astype(dtype)
    x = np.zeros((N, T), dtype=dtype)
    z = precond(r)
    p = z.copy()
    rz = coldot(r, z)
    alpha = np.zeros((n_iter, T), dtype=dtype)
    beta = np.zeros((n_iter, T), dtype=dtype)
    for k in range(n_iter):
        Ap = np.asarray(matvec(p), dtype=dtype)
        pAp = coldot(p, Ap)
        ok = (np.abs(pAp) > eps) & ~zero
        a = np.where(ok, rz / np.where(ok, pAp, 1), 0).astype(dtype)
        x = x + a * p
        r = r - a * Ap
        z = precond(r)
        rz_new = coldot(r, z)
        ok = np.abs(rz) > eps
        b = np.where(ok, rz_new / np.where(ok, rz, 1), 0).astype(dtype)
        p = z + b * p
        rz = rz_new
        alpha[k], beta[k] = a, b
    resid = np.where(zero, 0.0, np.sqrt(coldot(r, r).astype(np.float64)))
    return PcgResult(x.astype(np.float64) * nrm, alpha.astype(np.float64), beta.astype(np.float64), resid)


def tridiagonals(alpha, beta):
    """Lanczos tridiagonals [T x m x m] of the coefficient histories [m x T]:
    T[k][k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1},  T[k][k+1] = T[k+1][k] = sqrt(beta_k) / alpha_k."""
    m, T = alpha.shape
    t = np.zeros((T, m, m))
    for c in range(T):
        for k in range(m):
            t[c, k, k] = 1.0 / alpha[k, c] + (beta[k - 1, c] / alpha[k - 1, c] if k else 0.0)
            if k + 1 < m:
                t[c, k, k + 1] = t[c, k + 1, k] = math.sqrt(beta[k, c]) / alpha[k, c]
    return t


# ---- distances -------------------------------------------------------------------------------------------------------------
def coefficient_error(got, ref, skip_last=False):
    """Largest error of a coefficient history [n_iter x T], relative to the largest magnitude of that coefficient in its
    column of the reference.  Columns whose reference is all zero (a zero right-hand side) are the caller's to check exactly.
    skip_last: leave the last row out (see `distance`)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if skip_last:
        got, ref = got[:-1], ref[:-1]
    if ref.shape[0] == 0:
        return 0.0
    scale = np.abs(ref).max(axis=0)
    live = scale > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref)[:, live] / scale[live]).max())


def iterate_error(got, ref):
    """Largest relative 2-norm error of a column of x (columns with a zero reference excluded)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nr = np.linalg.norm(ref, axis=0)
    live = nr > 0
    if not live.any():
        return 0.0
    return float((np.linalg.norm(got - ref, axis=0)[live] / nr[live]).max())


def krylov_exhausted(n_iter, N):
    """N iterations on N rows (N <= m): the last residual is mathematically zero, and the last beta = r'.z' / r.z is what
    rounding left of it over an r.z that may itself be tiny — 0 or 1e-31 in float64, anything up to 1e-1 in float32 (N = 2,
    a right-hand side close to an eigenvector).  It says nothing about the implementation and is left out of the distances;
    the GPU tests only ask that it is finite."""
    return n_iter >= N


def distance(got, ref, N, T=None):
    """(alpha, beta, x) distances of two PcgResults over the leading T columns."""
    s = slice(0, T)
    return (coefficient_error(got.alpha[:, s], ref.alpha[:, s]),
            coefficient_error(got.beta[:, s], ref.beta[:, s], krylov_exhausted(ref.alpha.shape[0], N)),
            iterate_error(got.x[:, s], ref.x[:, s]))


# ---- systems and references, one per (N, K, J, kind, seed) --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(N, J=3, seed=SEED):
    return QuantisedKernel(N, J, seed)


@functools.lru_cache(maxsize=None)
def dense_system(N, J=3, seed=SEED):
    """The same kernel as a float32 matrix without the noise (RPGP_OP_DENSE's Kd) and the operator on its float64 copy."""
    return DenseKernel(system(N, J, seed).dense(noise=False).astype(np.float32), NOISE)


def _operator(N, J, seed, kind):
    return dense_system(N, J, seed) if kind == "dense" else system(N, J, seed)


@functools.lru_cache(maxsize=None)
def preconditioner(N, K, seed=SEED):
    return make_L(N, K, NOISE, seed)


@functools.lru_cache(maxsize=None)
def rhs(N, K=0, seed=SEED):
    b = make_rhs(N, seed, preconditioner(N, K, seed))
    b.setflags(write=False)
    return b


def reference(N, K, J=3, seed=SEED, kind="quantised", dtype="float64", drop_last=False):
    return _reference(N, K, J, seed, kind, dtype, drop_last)


@functools.lru_cache(maxsize=None)
def _reference(N, K, J, seed, kind, dtype, drop_last):
    """pcg of the system (N, K, J, seed) for 16 right-hand sides, M_ITERS iterations.  kind: "quantised" (the float64 kernel
    of the float32 coordinates: what the fused and the prepared operator compute) or "dense" (Kd.double() of the float32
    matrix).  drop_last: the preconditioner without its last column (condition 2)."""
    op = _operator(N, J, seed, kind)
    L = preconditioner(N, K, seed)
    if drop_last:
        L = L[:, :-1] if K > 1 else None
    mv = op.matvec32 if dtype == "float32" else op.matvec
    return pcg(mv, rhs(N, K, seed), L, NOISE, M_ITERS, np.dtype(dtype))


# ---- the case table ----------------------------------------------------------------------------------------------------------
# (group, N, T, K, J, direct): direct False = the k_reduce launches (RPGP_CG_DIRECT=0)
RANKS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16)
ROWS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 512)
SLAB_TILES = (16, 17, 32, 33, 48, 64)


def _cases():
    c = []
    c += [("every_tt", 777, T, K, 3, True) for T in range(1, 17) for K in (0, 15)]
    c += [("rank_ladder", 777, T, K, 3, True) for K in RANKS for T in (1, 11, 16)]
    c += [("row_ladder", N, T, K, 3, True) for N in ROWS for (T, K) in ((1, 1), (11, 15), (16, 16))]
    c += [("slabs", 256 * t - 100, 11, 15, 3, True) for t in SLAB_TILES]
    c += [("slabs", 16385, 11, 15, 3, True)]                          # 65 slabs: past kDirectParts, the k_reduce launches
    c += [("two_tiles", 300001, T, 15, 1, True) for T in (1, 16)]      # 1 172 tiles > kMaxBlocks: two tiles per workgroup
    c += [("reduce_launches", 777, T, 15, 3, False) for T in range(1, 17)]
    c += [("reduce_launches", 777, 11, K, 3, False) for K in RANKS]
    return c


CASES = _cases()
# the N = 777 cases of the first two groups once more through the prepared and the cached-matrix operator
OPERATOR_CASES = [(g, N, T, K, J, kind) for (g, N, T, K, J, d) in CASES if g in ("every_tt", "rank_ladder")
                  for kind in ("prepared", "dense")]


def case_id(case):
    g, N, T, K, J, last = case
    tail = ("" if last else "-reduce") if isinstance(last, bool) else "-" + last
    return "%s-N%d-T%d-K%d%s" % (g, N, T, K, tail)


def reference_keys():
    """Every (N, K, J, kind) a reference is needed for."""
    keys = {(N, K, J, "quantised") for (_, N, _, K, J, _) in CASES}
    keys |= {(N, K, J, "dense") for (_, N, _, K, J, kind) in OPERATOR_CASES if kind == "dense"}
    return sorted(keys)


@functools.lru_cache(maxsize=None)
def case_distances():
    """{(N, K, J, kind): (alpha, beta, x) distance of pcg(float32) from pcg(float64)} over the whole case table (16 columns:
    every case's columns are among them)."""
    return {k: distance(reference(k[0], k[1], k[2], SEED, k[3], "float32"), reference(k[0], k[1], k[2], SEED, k[3]), k[0])
            for k in reference_keys()}


@functools.lru_cache(maxsize=None)
def bounds():
    """(alpha, beta, x): MARGIN x the largest float32-to-float64 distance over the case table.  CPU numbers only."""
    d = np.array(list(case_distances().values()))
    return tuple(float(v) for v in MARGIN * d.max(axis=0))


@functools.lru_cache(maxsize=None)
def sensitivities():
    """{(N, K, J, kind): alpha distance of the float64 reference without the last column of L from the true one}, for the
    cases with N >= 17 and K >= 1 (below that a column of L is a large part of the space and the question is moot)."""
    out = {}
    for (N, K, J, kind) in reference_keys():
        if N >= 17 and K >= 1:
            full, less = reference(N, K, J, SEED, kind), reference(N, K, J, SEED, kind, "float64", True)
            out[(N, K, J, kind)] = coefficient_error(less.alpha, full.alpha)
    return out
