"""References, error magnitudes and a numpy restatement of the tiling of the float64 parity kernels (csrc/rpgp_f64.hip,
csrc/rpgp_ski_f64.hip).  Importable without a GPU; tests/test_f64_reference_host.py checks this module on the CPU and measures
the constants, tests/test_f64_kernels_gpu.py holds the kernels to it.

Every gate is entry-wise, |got - ref| <= C u A with u = 2^-53.  `ref` is the oracle (oracle.dense_gp, oracle.ski through
tests.oracle_backend.OracleBackend).  A is the reference's own sum with every term in absolute value, each exponential term
e = exp(-x), x = (z - z')^2 / 2, carrying the factor (1 + x): the relative error of e from a relative error eps of its argument
is x eps, so the one gate serves coordinates of any size.  C (per entry point, `C` below) comes from the CPU alone: 4 times the
larger of |restatement - long double| / (u A) and |numpy float64 - long double| / (u A) over all cases, rounded up to a power of
two (the factor 4: the device's software exp and its own, fixed-length, summation order, neither of which numpy reproduces).

The restatement (`restate_*`) walks the loops of the host code and of the kernels of rpgp_f64.hip: the j-pieces 20 / 8 / 4 / 2 /
1, the T chunks (12 / 4 / 1 for the product, 12 / 4 for the derivative), the column splits of mvm64_splits with the split
width rounded up to 64, the 64-column tiles with the `cend` and `tcnt` masks, the base value noise V and the accumulate flag of
the dense block.  Buffers are addressed flat with their leading dimensions, as the kernels do.  `mutate=` selects one
deliberate error (MUTATIONS); an index a mutation pushes past an array wraps around (modulo the array's size), a stand-in for
whatever lies behind the array on the device.  Rows are independent in every kernel, so the row blocks of 256 are not walked.

The grid-interpolation (SKI) kernels take their tap position as (z - g0) * (1 / h), the oracle as (z - g0) / h: one relative u
on a position of up to G.  Their magnitudes therefore use |W| + pos |dW/dpos| for the interpolation weights (and |dW| + pos
|d2W| for the derivative's), |phi| + |r phi'| for the Toeplitz entries, and |V|, |L|, |R|; the SKI gate is per output column:
the column's largest error against C u times the column's largest magnitude.  The staged entries (scatter, Toeplitz product,
gather) carry constants of their own, each measured against long double with the magnitude its test uses."""
import functools
import math

import numpy as np

from oracle import dense_gp as orc

U = 2.0 ** -53
LD = np.longdouble
PIECES = (20, 8, 4, 2, 1)
SCALE, NOISE = 0.3, 0.2

# constants of the gates, per entry point: measured by tests/test_f64_reference_host.py::test_constants (c_ref in its docstring)
C = {"mvm": 16, "dense": 32, "bilinear": 1, "bilinear_dense": 4, "project": 16, "project_grad": 8, "ski": 4, "ski_grid_product": 4,
     "ski_scatter": 2, "ski_gather": 2}

MUTATIONS = ("tile_reread", "drop_ragged", "cend_unclamped", "chunk_t0", "tcnt_mask", "piece_j0", "noise_per_piece",
             "dense_no_accumulate", "ldz_swap", "rowS_overwrite", "rowS_multicount", "gz_outside_slice", "lds_as_n")


def c_from(c_ref):
    """The smallest power of two >= 4 c_ref (it may lie below one)."""
    return 2.0 ** math.ceil(math.log2(4.0 * c_ref)) if c_ref > 0.0 else 0.0


def ratio(got, ref, A):
    """Largest |got - ref| / (u A); an entry with A = 0 must be exact."""
    got, ref, A = (np.asarray(a, dtype=np.float64) for a in (got, ref, A))
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / (U * A))
    return float(r.max()) if r.size else 0.0


def column_ratio(got, ref, A):
    """SKI gate: per column, largest |got - ref| / (u largest A); the worst column."""
    got, ref, A = (np.asarray(a, dtype=np.float64).reshape(np.shape(ref)[0] if np.ndim(ref) else 1, -1) for a in (got, ref, A))
    err = np.abs(got - ref).max(axis=0)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / (U * A.max(axis=0)))
    return float(r.max())


# ---- the loops of the host code -------------------------------------------------------------------------------------------
def pieces(j0, j1):
    out, j = [], j0
    while j < j1:
        jt = next(p for p in PIECES if p <= j1 - j)
        out.append((j, jt))
        j += jt
    return out


def chunks_mvm(T):
    out, t0 = [], 0
    while t0 < T:
        tt = 12 if T - t0 > 4 else (4 if T - t0 > 1 else 1)
        tcnt = min(T - t0, tt)
        out.append((t0, tt, tcnt))
        t0 += tcnt
    return out


def chunks_bilinear(T):
    out, t0 = [], 0
    while t0 < T:
        tt = 12 if T - t0 > 4 else 4
        tcnt = min(T - t0, tt)
        out.append((t0, tt, tcnt))
        t0 += tcnt
    return out


def splits(M, N):
    """(number of column splits, columns per split) of launch_mvm64 / launch_bil64."""
    nrb = (M + 255) // 256
    ns = (1024 + nrb - 1) // nrb
    ns = max(min(ns, (N + 63) // 64), 1)
    cps = ((N + ns - 1) // ns + 63) // 64 * 64
    return (N + cps - 1) // cps, cps


def geometry(M, N, T, j0, j1, derivative=False):
    ns, cps = splits(M, N)
    last = N - (ns - 1) * cps
    return {"splits": ns, "cps": cps, "tiles": [(min(cps, N - s * cps) + 63) // 64 for s in range(ns)], "last_split": last,
            "last_tile": last - (last - 1) // 64 * 64, "pieces": [jt for _, jt in pieces(j0, j1)],
            "chunks": [c[2] for c in (chunks_bilinear(T) if derivative else chunks_mvm(T))]}


def _flat(buf, idx):
    return buf[idx % buf.size]


def _tiles(N, cps, s, ns, mutate):
    """(first column read, first column owned, width) of the tiles of split s."""
    cbeg = s * cps
    cend = cbeg + cps if (cbeg + cps < N or mutate == "cend_unclamped") else N
    for k, c0 in enumerate(range(cbeg, cend, 64)):
        nc = min(64, cend - c0)
        if mutate == "drop_ragged" and s == ns - 1 and nc < 64:
            continue
        yield (cbeg if (mutate == "tile_reread" and k >= 1) else c0), c0, nc


def _ksum(a, zc):
    d = a[:, None, :] - zc[None, :, :]
    return np.exp(-0.5 * d * d), d


def restate_mvm(Z1, Z2, V, scale, noise=0.0, j0=0, j1=None, mutate=None):
    """rpgp_mvm_f64 on Z1 (M x ldz1), Z2 (N x ldz2), V (N x T): out (M x T)."""
    M, ldz1 = Z1.shape
    N, ldz2 = Z2.shape
    T = V.shape[1]
    j1 = ldz1 if j1 is None else j1
    z1, z2, v = Z1.ravel(), Z2.ravel(), V.ravel()
    if mutate == "ldz_swap":
        ldz1 = ldz2
    rows = np.arange(M)
    out = (noise * V[:M] if noise != 0.0 else np.zeros((M, T))).ravel().copy()
    ns, cps = splits(M, N)
    for pi, (j, jt) in enumerate(pieces(j0, j1)):
        if mutate == "noise_per_piece" and pi > 0 and noise != 0.0:
            out += (noise * V[:M]).ravel()
        jr = j0 if mutate == "piece_j0" else j
        a = _flat(z1, rows[:, None] * ldz1 + jr + np.arange(jt))
        for (t0, tt, tcnt) in chunks_mvm(T):
            tr = 0 if mutate == "chunk_t0" else t0
            tmask = np.ones(tt, bool) if mutate == "tcnt_mask" else np.arange(tt) < tcnt
            for s in range(ns):
                acc = np.zeros((M, tt))
                for src, c0, nc in _tiles(N, cps, s, ns, mutate):
                    cols = (src + np.arange(nc)) % N if mutate == "cend_unclamped" else src + np.arange(nc)
                    zc = _flat(z2, cols[:, None] * ldz2 + jr + np.arange(jt))
                    sv = np.where(tmask[None, :], _flat(v, cols[:, None] * T + tr + np.arange(tt)), 0.0)
                    e, _ = _ksum(a, zc)
                    acc += e.sum(axis=2) @ sv
                tw = np.nonzero(tmask)[0]
                np.add.at(out, (rows[:, None] * T + t0 + tw[None, :]) % out.size, scale * acc[:, tw])
    return out.reshape(M, T)


def restate_dense(Z1, Z2, scale, j0=0, j1=None, ldo=None, mutate=None):
    """rpgp_dense_f64 into a NaN-filled M x ldo buffer (ldo defaults to N)."""
    M, ldz1 = Z1.shape
    N, ldz2 = Z2.shape
    j1 = ldz1 if j1 is None else j1
    ldo = N if ldo is None else ldo
    z1, z2 = Z1.ravel(), Z2.ravel()
    if mutate == "ldz_swap":
        ldz1 = ldz2
    out = np.full((M, ldo), np.nan)
    for pi, (j, jt) in enumerate(pieces(j0, j1)):
        jr = j0 if mutate == "piece_j0" else j
        a = _flat(z1, np.arange(M)[:, None] * ldz1 + jr + np.arange(jt))
        b = _flat(z2, np.arange(N)[:, None] * ldz2 + jr + np.arange(jt))
        acc = np.zeros((M, N))
        for q in range(jt):
            d = a[:, q:q + 1] - b[:, q:q + 1].T
            acc += np.exp(-0.5 * d * d)
        accumulate = pi > 0 and mutate != "dense_no_accumulate"
        out[:, :N] = scale * acc + out[:, :N] if accumulate else scale * acc
    return out


def _tree_sum(x, width):
    """sum_f64_kernel / project_grad_f64_kernel: `width` strided partial sums, then the halving tree."""
    n = x.shape[0]
    pad = np.zeros(((n + width - 1) // width * width,) + x.shape[1:])
    pad[:n] = x
    sh = np.add.reduce(pad.reshape((-1, width) + x.shape[1:]), axis=0)
    w = width // 2
    while w > 0:
        sh[:w] = sh[:w] + sh[w:2 * w]
        w //= 2
    return sh[0]


def _restate_bilinear(Z, L, R, S, scale, j0, j1, ldg, lds, mutate):
    N, ldz = Z.shape
    dense = S is not None
    j1 = ldz if j1 is None else j1
    ldg = ldz if ldg is None else ldg
    z = Z.ravel()
    rows = np.arange(N)
    T = 1 if dense else L.shape[1]
    rowS = np.zeros(N)
    gZ = np.full((N, ldg), np.nan)
    if mutate == "gz_outside_slice":
        gZ[:] = 0.0
    gZ[:, j0:j1] = 0.0
    ns, cps = splits(N, N)
    if dense:
        s_flat = S.ravel()
        lds = S.shape[1] if lds is None else lds
        if mutate == "lds_as_n":
            lds = N
    else:
        lf, rf = L.ravel(), R.ravel()
    kfull = None
    if mutate == "rowS_multicount":
        kfull = sum(np.exp(-0.5 * (Z[:, q:q + 1] - Z[:, q:q + 1].T) ** 2) for q in range(j0, j1))
        sfull = S[:, :N] if dense else L @ R.T + R @ L.T
    for (j, jt) in pieces(j0, j1):
        jr = j0 if mutate == "piece_j0" else j
        a = _flat(z, rows[:, None] * ldz + jr + np.arange(jt))
        for (t0, tt, tcnt) in ([(0, 4, 0)] if dense else chunks_bilinear(T)):
            if mutate == "rowS_overwrite":
                rowS[:] = 0.0
            tr = 0 if mutate == "chunk_t0" else t0
            tmask = np.ones(tt, bool) if mutate == "tcnt_mask" else np.arange(tt) < tcnt
            if not dense:
                li = np.where(tmask[None, :], _flat(lf, rows[:, None] * T + tr + np.arange(tt)), 0.0)
                ri = np.where(tmask[None, :], _flat(rf, rows[:, None] * T + tr + np.arange(tt)), 0.0)
            for s in range(ns):
                accG, accS = np.zeros((N, jt)), np.zeros(N)
                for src, c0, nc in _tiles(N, cps, s, ns, mutate):
                    cols = (src + np.arange(nc)) % N if mutate == "cend_unclamped" else src + np.arange(nc)
                    zc = _flat(z, cols[:, None] * ldz + jr + np.arange(jt))
                    if dense:
                        Sv = _flat(s_flat, ((c0 + np.arange(nc)) % N)[None, :] * lds + rows[:, None])
                    else:
                        lc = np.where(tmask[None, :], _flat(lf, cols[:, None] * T + tr + np.arange(tt)), 0.0)
                        rc = np.where(tmask[None, :], _flat(rf, cols[:, None] * T + tr + np.arange(tt)), 0.0)
                        Sv = li @ rc.T + ri @ lc.T
                    e, d = _ksum(a, zc)
                    accG += np.einsum("ic,icj->ij", Sv, e * d)
                    accS += (Sv * e.sum(axis=2)).sum(axis=1)
                gZ[:, j:j + jt] += -scale * accG
                if mutate != "rowS_multicount":
                    rowS += accS
            if mutate == "rowS_multicount":
                rowS += (sfull * kfull).sum(axis=1)
    return gZ, 0.5 * _tree_sum(rowS, 1024)


def restate_bilinear(Z, L, R, scale, j0=0, j1=None, ldg=None, mutate=None):
    """rpgp_bilinear_grad_f64: (gZ in a NaN-filled N x ldg buffer, gscale)."""
    return _restate_bilinear(Z, L, R, None, scale, j0, j1, ldg, None, mutate)


def restate_bilinear_dense(Z, S, scale, j0=0, j1=None, ldg=None, mutate=None):
    """rpgp_bilinear_grad_dense_f64 with S an N x lds buffer (the kernel reads S[c][i])."""
    return _restate_bilinear(Z, None, None, S, scale, j0, j1, ldg, None, mutate)


def restate_project(X, P):
    """project_f64_kernel (the grid-stride loop changes no element's arithmetic): fma chain over k."""
    acc = np.zeros((X.shape[0], P.shape[1]))
    for k in range(X.shape[1]):
        acc += X[:, k:k + 1] * P[k:k + 1, :]
    return acc


def project_blocks(N, J):
    """(workgroups launched, elements per thread at most) of rpgp_project_f64."""
    total = N * J
    blocks = min((total + 255) // 256, 8192)
    return blocks, (total + blocks * 256 - 1) // (blocks * 256)


def restate_project_grad(X, G):
    N, d = X.shape
    return _tree_sum((X[:, :, None] * G[:, None, :]).reshape(N, -1), 256).reshape(d, G.shape[1])


# ---- references (oracle), magnitudes and the long-double forms, in row blocks -----------------------------------------------
def _blocks(M, step=512):
    return [(r, min(r + step, M)) for r in range(0, M, step)]


def _pair_terms(Z1b, Z2, dtype):
    """(K, Kabs) of a row block: sum_j e_j and sum_j (1 + x) e_j (Kabs always float64)."""
    K = np.zeros((Z1b.shape[0], Z2.shape[0]), dtype=dtype)
    Ka = np.zeros((Z1b.shape[0], Z2.shape[0]))
    for j in range(Z1b.shape[1]):
        d = Z1b[:, j:j + 1].astype(dtype) - Z2[:, j:j + 1].astype(dtype).T
        x = 0.5 * d * d
        e = np.exp(-x)
        K += e
        Ka += ((1.0 + x) * e).astype(np.float64)
    return K, Ka


def mvm_ref(Z1, Z2, V, scale, noise=0.0):
    return orc.mvm(Z1, Z2, V, scale, noise)


def mvm_mag(Z1, Z2, V, scale, noise=0.0, long_double=False):
    """A of the product; with long_double also the long-double reference: (A, ref_ld)."""
    M, T = Z1.shape[0], V.shape[1]
    A = np.zeros((M, T))
    ref = np.zeros((M, T), dtype=LD) if long_double else None
    Va = np.abs(V)
    for r0, r1 in _blocks(M):
        K, Ka = _pair_terms(Z1[r0:r1], Z2, LD if long_double else np.float64)
        A[r0:r1] = scale * (Ka @ Va)
        if long_double:
            ref[r0:r1] = LD(scale) * (K @ V.astype(LD))
    if noise != 0.0:
        A += np.abs(noise * V[:M])
        if long_double:
            ref += LD(noise) * V[:M].astype(LD)
    return (A, ref) if long_double else A


def dense_ref(Z1, Z2, scale):
    return scale * orc.additive_rbf(Z1, Z2)


def dense_mag(Z1, Z2, scale, long_double=False):
    A = np.zeros((Z1.shape[0], Z2.shape[0]))
    ref = np.zeros(A.shape, dtype=LD) if long_double else None
    for r0, r1 in _blocks(Z1.shape[0]):
        K, Ka = _pair_terms(Z1[r0:r1], Z2, LD if long_double else np.float64)
        A[r0:r1] = scale * Ka
        if long_double:
            ref[r0:r1] = LD(scale) * K
    return (A, ref) if long_double else A


def bilinear_ref(Z, L, R, scale):
    return orc.bilinear_grad(Z, L, R, scale)


def bilinear_dense_ref(Z, S, scale):
    """The float64 twin of what tests/test_kernels_gpu.py::test_bilinear_grad_dense_matches_oracle computes."""
    N, J = Z.shape
    g, ks = np.zeros((N, J)), np.zeros((N, N))
    for j in range(J):
        d = Z[:, j:j + 1] - Z[:, j:j + 1].T
        e = np.exp(-0.5 * d * d)
        ks += e
        g[:, j] = -scale * (S * e * d).sum(axis=1)
    return g, 0.5 * (S * ks).sum()


def bilinear_mag(Z, L, R, scale, S=None, long_double=False):
    """(A_gZ, A_gscale) for S = L R^T + R L^T or a given dense symmetric S; with long_double also (gZ_ld, gscale_ld)."""
    N, J = Z.shape
    dt = LD if long_double else np.float64
    A, Ags = np.zeros((N, J)), 0.0
    g = np.zeros((N, J), dtype=LD) if long_double else None
    gs = LD(0.0)
    for r0, r1 in _blocks(N, 256):
        if S is None:
            Sa = np.abs(L[r0:r1]) @ np.abs(R).T + np.abs(R[r0:r1]) @ np.abs(L).T
            Sb = (L[r0:r1].astype(dt) @ R.astype(dt).T + R[r0:r1].astype(dt) @ L.astype(dt).T) if long_double else None
        else:
            Sa = np.abs(S[r0:r1])
            Sb = S[r0:r1].astype(dt) if long_double else None
        ksa = np.zeros((r1 - r0, N))
        ks = np.zeros((r1 - r0, N), dtype=dt)
        for j in range(J):
            d = Z[r0:r1, j:j + 1].astype(dt) - Z[:, j:j + 1].astype(dt).T
            x = 0.5 * d * d
            e = np.exp(-x)
            ea = ((1.0 + x) * e).astype(np.float64)
            ksa += ea
            A[r0:r1, j] = scale * (Sa * ea * np.abs(d).astype(np.float64)).sum(axis=1)
            if long_double:
                ks += e
                g[r0:r1, j] = -LD(scale) * (Sb * e * d).sum(axis=1)
        Ags += 0.5 * float((Sa * ksa).sum())
        if long_double:
            gs += LD(0.5) * (Sb * ks).sum()
    return (A, Ags, g, gs) if long_double else (A, Ags)


def project_mag(X, P, long_double=False):
    A = np.abs(X) @ np.abs(P)
    return (A, X.astype(LD) @ P.astype(LD)) if long_double else A


def project_grad_mag(X, G, long_double=False):
    A = np.abs(X).T @ np.abs(G)
    return (A, X.astype(LD).T @ G.astype(LD)) if long_double else A


# ---- the cases ------------------------------------------------------------------------------------------------------------
MVM_CASES = [(4161, 4161, 5, 17), (4097, 4097, 2, 1), (321, 321, 35, 14), (2305, 7361, 3, 16), (4161, 130, 3, 1),
             (7, 4500, 8, 13), (1, 1, 1, 1), (64, 64, 3, 4), (65, 65, 3, 2), (257, 256, 1, 5)]
DENSE_CASES = [(1, 1, 1), (17, 257, 35), (33, 300, 11)]
BILINEAR_CASES = [(4161, 5, 17), (4097, 3, 16), (321, 35, 14), (1, 1, 1), (65, 2, 13)]
BILINEAR_DENSE_CASES = [(4161, 3), (321, 35), (64, 3)]
PROJECT_CASES = [(110000, 3, 20), (1, 1, 1), (255, 5, 7), (257, 5, 7)]
SLICE = (3, 10)              # (j0, j1) of the slice cases; Z1 is 12 wide, Z2 14 wide
SLICE_LD = (12, 14)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=None)
def mvm_inputs(M, N, J, T):
    """(Z1, Z2, V, noise): symmetric cases share Z and carry the noise term."""
    rng = _rng(1, M, N, J, T)
    Z2 = rng.standard_normal((N, J))
    Z1 = Z2 if M == N else rng.standard_normal((M, J))
    return Z1, Z2, rng.standard_normal((N, T)), (NOISE if M == N else 0.0)


@functools.lru_cache(maxsize=None)
def mvm_slice_inputs(M=300, N=200, T=5):
    rng = _rng(2, M, N, T)
    return rng.standard_normal((M, SLICE_LD[0])), rng.standard_normal((N, SLICE_LD[1])), rng.standard_normal((N, T))


@functools.lru_cache(maxsize=None)
def large_coordinate_inputs(N=300, J=4, T=3, dup=10):
    """Z = 30 x standard normal with `dup` duplicated rows (row N - 1 - k repeats row k): most e underflow, a duplicated pair
    contributes exactly J."""
    rng = _rng(3, N, J, T)
    Z = 30.0 * rng.standard_normal((N, J))
    Z[N - dup:] = Z[:dup][::-1]
    return Z, rng.standard_normal((N, T))


@functools.lru_cache(maxsize=None)
def dense_inputs(M, N, J):
    rng = _rng(4, M, N, J)
    return rng.standard_normal((M, J)), rng.standard_normal((N, J))


@functools.lru_cache(maxsize=None)
def bilinear_inputs(N, J, T):
    rng = _rng(5, N, J, T)
    return rng.standard_normal((N, J)), rng.standard_normal((N, T)), rng.standard_normal((N, T))


@functools.lru_cache(maxsize=None)
def bilinear_dense_inputs(N, J, lds=None):
    """(Z, S buffer N x lds with S = A + A^T in its first N columns, NaN behind)."""
    rng = _rng(6, N, J)
    Z = rng.standard_normal((N, J))
    Am = rng.standard_normal((N, N))
    S = np.full((N, N if lds is None else lds), np.nan)
    S[:, :N] = Am + Am.T
    return Z, S


@functools.lru_cache(maxsize=None)
def project_inputs(N, d, J):
    rng = _rng(7, N, d, J)
    return rng.standard_normal((N, d)), rng.standard_normal((d, J)), rng.standard_normal((N, J))


# ---- grid interpolation (SKI) -----------------------------------------------------------------------------------------------
SKI_KINDS = ("RBF", "Matern", "InverseMQ", "Cosine")


def ski_block(gp, J):
    """(g0 [J], h [J], 1/h [J], w [J] or None, kind) of a float64 grid block (numpy)."""
    gp = np.asarray(gp, dtype=np.float64)
    flags = int(gp[3])
    kind = SKI_KINDS[(flags >> 2) & 3]
    w = gp[4:4 + J].copy() if flags & 1 else None
    if flags & 2:
        arr = gp[4 + J:4 + 4 * J].reshape(J, 3)
        return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), w, kind
    return np.full(J, gp[0]), np.full(J, gp[1]), np.full(J, gp[2]), w, kind


def _phi_sens(kind, r):
    """|phi(r)| + |r phi'(r)| of the 1-D sub-kernels (oracle.family._phi is the value)."""
    r = np.abs(r)
    if kind == "RBF":
        return np.exp(-0.5 * r * r) * (1.0 + r * r)
    if kind == "Matern":
        s = np.sqrt(3.0) * r
        return (1.0 + s) * np.exp(-s) + s * s * np.exp(-s)
    if kind == "InverseMQ":
        return (1.0 + r * r) ** -0.5 + r * r * (1.0 + r * r) ** -1.5
    return np.abs(np.cos(np.pi * r)) + np.abs(np.pi * r * np.sin(np.pi * r))


def _cubic_all(Uv):
    """(w, dw/dU, d2w/dU2) of the Keys kernel at U >= 0."""
    inner = Uv < 1.0
    w = np.where(inner, ((1.5 * Uv - 2.5) * Uv) * Uv + 1.0, ((-0.5 * Uv + 2.5) * Uv - 4.0) * Uv + 2.0)
    dw = np.where(inner, (4.5 * Uv - 5.0) * Uv, (-1.5 * Uv + 5.0) * Uv - 4.0)
    return w, dw, np.where(inner, 9.0 * Uv - 5.0, -3.0 * Uv + 5.0)


def ski_taps(z, g0, inv_h, G):
    """The rule of `taps` in rpgp_ski_f64.hip (position by multiplication with 1/h): first tap, 4 weights, their derivatives
    in z, the 4 second derivatives in position units, the clipped position, and whether the row clamps."""
    u0 = (z - g0) * inv_h
    u = np.clip(u0, 1.0, G - 2.0)
    fl = np.floor(u)
    fr = u - fl
    idx0 = np.clip(fl.astype(np.int64) - 1, 0, G - 4)
    s = np.stack([fr + 1.0, fr, 1.0 - fr, 2.0 - fr], axis=1)
    w, dw, d2 = _cubic_all(s)
    sign = np.array([1.0, 1.0, -1.0, -1.0])
    return idx0, w, dw * sign * inv_h, d2, u, (u0 < 1.0) | (u0 > G - 2.0)


def _dense_rows(idx0, vals, G):
    W = np.zeros((idx0.shape[0], G))
    for q in range(4):
        np.add.at(W, (np.arange(idx0.shape[0]), idx0 + q), vals[:, q])
    return W


def ski_parts(Z, gp, G, sens=False):
    """Per projection (W, dW, Tm, w_j) as dense matrices from the kernel's tap rule; with sens the magnitudes
    (|W| + pos |dW/dpos|, (|dW/dpos| + pos |d2W/dpos2|) / h, |phi| + |r phi'|, |w_j|)."""
    J = Z.shape[1]
    g0, h, inv_h, w, kind = ski_block(gp, J)
    from oracle.family import _phi
    out = []
    lag = np.arange(G)[:, None] - np.arange(G)[None, :]
    for j in range(J):
        idx0, wv, dwv, d2, u, _ = ski_taps(Z[:, j], g0[j], inv_h[j], G)
        wj = 1.0 if w is None else w[j]
        if sens:
            dpos = np.abs(dwv) / inv_h[j]
            out.append((_dense_rows(idx0, np.abs(wv) + u[:, None] * dpos, G),
                        _dense_rows(idx0, (dpos + u[:, None] * np.abs(d2)) * inv_h[j], G),
                        _phi_sens(kind, lag * h[j]), abs(wj)))
        else:
            d = lag * h[j]
            out.append((_dense_rows(idx0, wv, G), _dense_rows(idx0, dwv, G), _phi(kind, d * d), wj))
    return out


def ski_mvm_mag(Z1, Z2, gp, V, scale, noise, G, restate=False):
    """A of the SKI product (restate: the staged product itself, scatter -> Toeplitz -> gather, from the kernel's tap rule)."""
    out = np.zeros((Z1.shape[0], V.shape[1]))
    Vv = V if restate else np.abs(V)
    for (W1, _, Tm, wj), (W2, _, _, _) in zip(ski_parts(Z1, gp, G, not restate), ski_parts(Z2, gp, G, not restate)):
        out += W1 @ (wj * (Tm @ (W2.T @ Vv)))
    out *= scale
    if noise != 0.0:
        out += noise * V if restate else np.abs(noise * V)
    return out


def ski_dense_mag(Z1, Z2, gp, scale, G, restate=False):
    out = np.zeros((Z1.shape[0], Z2.shape[0]))
    for (W1, _, Tm, wj), (W2, _, _, _) in zip(ski_parts(Z1, gp, G, not restate), ski_parts(Z2, gp, G, not restate)):
        out += wj * (W1 @ Tm @ W2.T)
    return scale * out


def ski_bilinear_mag(Z, gp, L, R, scale, G, restate=False):
    """(A_gZ, A_gscale, A_gcomp) (restate: the values themselves from the kernel's formulas and tap rule)."""
    N, J = Z.shape
    La, Ra = (L, R) if restate else (np.abs(L), np.abs(R))
    gZ, gc = np.zeros((N, J)), np.zeros(J)
    for j, (W, dW, Tm, wj) in enumerate(ski_parts(Z, gp, G, not restate)):
        HL, HR = Tm @ (W.T @ La), Tm @ (W.T @ Ra)
        gZ[:, j] = scale * wj * ((La * (dW @ HR)).sum(axis=1) + (Ra * (dW @ HL)).sum(axis=1))
        gc[j] = wj * (La * (W @ HR)).sum()
    return gZ, gc.sum(), gc


def ski_hist_mag(Z, gp, V, G, restate=False):
    """J x G x T: W_j^T V (restate) or its magnitude."""
    Vv = V if restate else np.abs(V)
    return np.stack([W.T @ Vv for (W, _, _, _) in ski_parts(Z, gp, G, not restate)])


def ski_inputs(N, M, J, T, seed=0):
    rng = _rng(8, N, M, J, T, seed)
    Z = rng.standard_normal((N, J)) * np.linspace(1.0, 1.6, J)
    Zs = 0.8 * rng.standard_normal((M, J))
    return Z, Zs, rng.standard_normal((N, T)), rng.standard_normal((N, T)), rng.standard_normal((N, T)), \
        rng.uniform(0.3, 1.4, size=J)


def ski_grid_product_forms(hist, gp, G, weighted, long_double=False):
    """rpgp_ski_f64_grid_product of a J x G x T histogram: (reference w_j Tm_j hist_j by numpy, A = |w_j| (|phi| + |r phi'|) |hist_j|);
    with long_double also the kernel's own sum (one fma chain over the G grid points, in order) and the long-double form with
    the Toeplitz entries evaluated in long double (RBF blocks only).  This stage has no tap position in it, so its magnitude
    has no position term and it carries a constant of its own."""
    from oracle.family import _phi
    J, _, T = hist.shape
    g0, h, inv_h, w, kind = ski_block(gp, J)
    lag = np.arange(G)[:, None] - np.arange(G)[None, :]
    ref, A, seq, ld = [], [], [], []
    for j in range(J):
        wj = w[j] if (weighted and w is not None) else 1.0
        d = lag * h[j]
        Tm = _phi(kind, d * d)
        ref.append(wj * (Tm @ hist[j]))
        A.append(abs(wj) * (_phi_sens(kind, d) @ np.abs(hist[j])))
        if long_double:
            assert kind == "RBF"
            acc = np.zeros((G, T))
            for gg in range(G):
                acc += Tm[:, gg:gg + 1] * hist[j][gg:gg + 1, :]
            seq.append(wj * acc)
            dl = lag.astype(LD) * LD(h[j])
            ld.append(LD(wj) * (np.exp(-LD(0.5) * dl * dl) @ hist[j].astype(LD)))
    return (np.stack(ref), np.stack(A), np.stack(seq), np.stack(ld)) if long_double else (np.stack(ref), np.stack(A))


# ---- the SKI cases, shared by the host measurement and the GPU module ----------------------------------------------------------
ALL_FORMS = ("product", "rect", "diag", "dense", "deriv")
_RW = [("shared", False), ("shared", True), ("reference", False), ("reference", True)]
# (name, N, M, J, T, G, rule, weighted, kind, forms)
SKI_SWEEP = [("starred", 130, 33, 3, 3, 16, r, w, k, ALL_FORMS) for (r, w) in _RW for k in SKI_KINDS] + \
    [("T70", 900, 300, 4, 70, 128, r, True, "RBF", ("product", "rect", "deriv")) for r in ("shared", "reference")] + \
    [("single", 1, 1, 1, 1, 8, r, False, "RBF", ALL_FORMS) for r in ("shared", "reference")] + \
    [("G8", 257, 5, 1, 2, 8, r, False, "RBF", ALL_FORMS) for r in ("shared", "reference")] + \
    [("clamp", 130, 33, 3, 3, 16, r, True, "RBF", ("rect", "dense")) for r in ("shared", "reference")]
SKI_STAGED = [("shared", True), ("reference", True), ("shared", False)]      # at (130, 33, 3, 3), G = 16


def ski_case_id(case):
    name, N, M, J, T, G, rule, weighted, kind, _ = case
    return "%s-%s-%s-%s" % (name, rule[:3], "w" if weighted else "u", kind)


def ski_case_inputs(name, N, M, J, T):
    """Host arrays of a case and whether the grid block also covers Zs.  "single": one point, Zs = Z, so the range is zero and
    the rule's clamp_min decides the grid.  "clamp": the block is built from Z alone and every entry of Zs lies more than a
    spacing outside its range (a spacing is at most range / (G - 5): a quarter of the range clears it)."""
    Z, Zs, V, L, R, w = ski_inputs(N, M, J, T)
    both = True
    if name == "single":
        Z, V, L, R = np.array([[0.75]]), np.array([[1.25]]), np.array([[0.8]]), np.array([[-1.1]])
        Zs, both = Z.copy(), False
    elif name == "clamp":
        Zs, both = np.sign(Zs) * (np.abs(Z).max() + 0.25 * (Z.max() - Z.min()) + np.abs(Zs)), False
    return dict(Z=Z, Zs=Zs, V=V, L=L, R=R, w=w), both


def ski_oracle(host, gp, G, forms):
    """label -> (oracle value, A), 2-D arrays, for the forms of a case with the float64 grid block gp (numpy)."""
    import torch
    from tests.oracle_backend import OracleBackend
    ob = OracleBackend()
    c = {k: torch.from_numpy(np.ascontiguousarray(host[k])) for k in ("Z", "Zs", "V", "L", "R")}
    gpc = torch.from_numpy(np.ascontiguousarray(gp))
    Z, Zs, V, L, R = (host[k] for k in ("Z", "Zs", "V", "L", "R"))
    out = {}
    if "product" in forms:
        out["product"] = (ob.ski_mvm(c["Z"], c["Z"], gpc, c["V"], SCALE, NOISE, G).numpy(), ski_mvm_mag(Z, Z, gp, V, SCALE, NOISE, G))
    if "rect" in forms:
        out["rect"] = (ob.ski_mvm(c["Zs"], c["Z"], gpc, c["V"], SCALE, 0.0, G).numpy(), ski_mvm_mag(Zs, Z, gp, V, SCALE, 0.0, G))
    if "diag" in forms:
        out["diag"] = (ob.ski_diag(c["Z"], gpc, SCALE, G).numpy()[:, None], np.diag(ski_dense_mag(Z, Z, gp, SCALE, G))[:, None])
    if "dense" in forms:
        out["dense"] = (ob.ski_dense(c["Zs"], c["Z"], gpc, SCALE, G).numpy(), ski_dense_mag(Zs, Z, gp, SCALE, G))
    if "deriv" in forms:
        g, gs, gc = ob.ski_bilinear_grad_comp(c["Z"], gpc, c["L"], c["R"], SCALE, G)
        Ag, As, Ac = ski_bilinear_mag(Z, gp, L, R, SCALE, G)
        out["gZ"], out["gscale"] = (g.numpy(), Ag), (gs.numpy().reshape(1, 1), np.array([[As]]))
        out["gcomp"] = (gc.numpy().reshape(1, -1), Ac.reshape(1, -1))
    return out


def ski_restated(host, gp, G, forms):
    """label -> the same forms from the kernels' own formulas and tap rule (float64 numpy)."""
    Z, Zs, V, L, R = (host[k] for k in ("Z", "Zs", "V", "L", "R"))
    out = {}
    if "product" in forms:
        out["product"] = ski_mvm_mag(Z, Z, gp, V, SCALE, NOISE, G, True)
    if "rect" in forms:
        out["rect"] = ski_mvm_mag(Zs, Z, gp, V, SCALE, 0.0, G, True)
    if "diag" in forms:
        out["diag"] = np.diag(ski_dense_mag(Z, Z, gp, SCALE, G, True))[:, None]
    if "dense" in forms:
        out["dense"] = ski_dense_mag(Zs, Z, gp, SCALE, G, True)
    if "deriv" in forms:
        g, gs, gc = ski_bilinear_mag(Z, gp, L, R, SCALE, G, True)
        out["gZ"], out["gscale"], out["gcomp"] = g, np.array([[gs]]), gc.reshape(1, -1)
    return out


def _weights_ld(z, g0, h, G):
    """Dense N x G interpolation matrix in long double, the position taken as (z - g0) / h in long double."""
    u = np.clip((z.astype(LD) - LD(g0)) / LD(h), LD(1.0), LD(G - 2.0))
    fl = np.floor(u)
    fr = u - fl
    idx0 = np.clip(fl.astype(np.int64) - 1, 0, G - 4)
    W = np.zeros((z.shape[0], G), dtype=LD)
    for q, sq in enumerate([fr + 1, fr, 1 - fr, 2 - fr]):
        wq = np.where(sq < 1, ((LD(1.5) * sq - LD(2.5)) * sq) * sq + 1, ((LD(-0.5) * sq + LD(2.5)) * sq - 4) * sq + 2)
        np.add.at(W, (np.arange(z.shape[0]), idx0 + q), wq)
    return W


def ski_scatter_forms(Z, gp, V, G):
    """rpgp_ski_f64_scatter: (kernel-rule float64 histogram, A, long-double histogram), J x G x T."""
    J = Z.shape[1]
    g0, h, _, _, _ = ski_block(gp, J)
    ld = np.stack([_weights_ld(Z[:, j], g0[j], h[j], G).T @ V.astype(LD) for j in range(J)])
    return ski_hist_mag(Z, gp, V, G, True), ski_hist_mag(Z, gp, V, G), ld


def ski_gather_forms(Z, gp, H, V, noise, G):
    """rpgp_ski_f64_gather of a given J x G x T float64 H: (kernel-rule float64 result, A, long-double result)."""
    J = Z.shape[1]
    g0, h, _, _, _ = ski_block(gp, J)
    val, sens = ski_parts(Z, gp, G), ski_parts(Z, gp, G, True)
    got = SCALE * sum(val[j][0] @ H[j] for j in range(J)) + (noise * V if noise else 0.0)
    A = SCALE * sum(sens[j][0] @ np.abs(H[j]) for j in range(J)) + abs(noise) * np.abs(V)
    ld = LD(SCALE) * sum(_weights_ld(Z[:, j], g0[j], h[j], G) @ H[j].astype(LD) for j in range(J)) + LD(noise) * V.astype(LD)
    return got, A, ld
