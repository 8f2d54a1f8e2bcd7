"""Float64 reference, probe columns and a derived float32 error bound for the exact prepared sweep
(rpgp_mvm_sym_prepared_range: csrc/rpgp_kernels.hip mvm_fact_kernel<JT, TT, R>, csrc/rpgp_fact_asm.hip).  numpy only, importable
without a GPU: tests/test_prepared_sweep_reference_host.py checks this module on the CPU, tests/test_prepared_sweep_gpu.py holds
the kernels to it.

What the sweep computes.  rpgp_prepare centres projection j at mid_j = 0.5f * (min_j + max_j) (prep_finish_kernel, float32) and
stores a = (z - mid_j) * c with c = float32(sqrt(0.5 log2 e)), Ea = exp2(-a^2) on the row side and {2a, -a^2} on the column
side.  One term of K(i, c) is

    t = fma(a, 2b, -b^2);   e = exp2(t);   term = e * Ea            exp2(-a^2) * exp2(2ab - b^2) = exp2(-(a - b)^2)

and the reference's entry (memory_efficient_gam_kernel.py:20-30, as oracle/dense_gp.py restates it) is k = exp(-0.5 (z_i - z_c)^2)
= exp2(-(a - b)^2) with a, b the UNROUNDED centred and scaled coordinates: the midpoint cancels in the difference.

The bound (`entry_bound`).  u = 2^-24, a and b in float64 from the float32 Z and the float32 midpoint.  The computed a differs
from a by at most 3u|a|: the subtraction z - mid, the product with c, and c itself (a float32 constant) are one relative u
each.  The roundings of a and of b are independent, so the computed difference is off by up to 3u (|a| + |b|) ABSOLUTE (not
relative to |a - b|), and the exponent -(a - b)^2 by 2 |a - b| 3u (|a| + |b|) = 6u |a - b| (|a| + |b|).  The two squares are
rounded once each, u a^2 (inside Ea's argument) and u b^2 (the stored -b^2), and the FMA rounds its result, u |2ab - b^2|.
An error d of the exponent is a relative error ln2 d of the power.  The two hardware exponentials are documented to 1 ULP,
which is at most 2u relative each, and their product is rounded once: 5u.  To first order in u

    rel_j = u (ln2 (6 |a - b| (|a| + |b|) + a^2 + b^2 + |2ab - b^2|) + 5)
    bound(i, c) = sum_j rel_j k_j + J 2^-120

the last term for products below the normal range, which the device flushes to zero (every exp2 argument of a fast_ok Z lies in
[-300, 100], Ea >= 2^-100: only a term whose value is below 2^-126 can be flushed).

What the bound leaves out on purpose: the J terms are ADDED in float32 (packed even / odd partial sums and one horizontal add
in the compiler kernels, a chain over the projections in the hand-scheduled ones, one more addition per later J piece into
the slab).  In the FMA form K = fma(e, Ea, K) the product is not rounded on its own, so the "product" u of a term is really
the rounding of that addition.  Those roundings are at most (JT - 1) u K per piece in the worst case and random in sign; they
are carried by the distance between the documented 1 ULP and what the exponential delivers.  The host module measures the
ratio error / bound with the sum done in the compiler kernel's order, and the GPU module prints it per case.

Unit right-hand sides make the statement per entry: with V[:, t] = e_c the product is scale K[:, c] with nothing summed over
columns, the reducer adds zeros in float64, and the only further rounding is the cast of scale * K to float32 (u |ref|)."""
import contextlib
import math
import os

import numpy as np

U = 2.0 ** -24
C_EXP2 = math.sqrt(0.5 * math.log2(math.e))
C_EXP2_F32 = np.float32(0.8493218002880191)          # kExp2Scale
J_PIECES = (20, 10, 8, 5, 4, 3, 2, 1)                 # kJPieces
FLUSH = 2.0 ** -120
MAX_PROBES = 48


@contextlib.contextmanager
def sweep(env_asm=None):
    """Force the exact sweep for ops.mvm_sym_prepared (RPGP_LOWRANK=0; ops.lowrank_enabled reads it per call) and, with env_asm
    "0" / "1", choose between the compiler-scheduled and the hand-scheduled kernels (RPGP_FACT_ASM, read per launch)."""
    assert env_asm in (None, "0", "1")
    new = {"RPGP_LOWRANK": "0"}
    if env_asm is not None:
        new["RPGP_FACT_ASM"] = env_asm
    old = {k: os.environ.get(k) for k in new}
    os.environ.update(new)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def j_pieces(j0, j1):
    """(first projection, count) of the compiled pieces a j-range is served by (next_j_piece)."""
    out, j = [], j0
    while j < j1:
        jt = next(p for p in J_PIECES if p <= j1 - j)
        out.append((j, jt))
        j += jt
    return out


def t_pieces(T):
    """(t0, compiled width, columns used) of the right-hand-side blocks (next_t_piece)."""
    out, t0 = [], 0
    while t0 < T:
        tt = 12 if T - t0 > 4 else (4 if T - t0 > 1 else 1)
        tcnt = min(T - t0, tt)
        out.append((t0, tt, tcnt))
        t0 += tcnt
    return out


def midpoint(Z):
    """mid_j of prep_finish_kernel: 0.5f * (min + max) in float32 (min and max are exact in any order)."""
    Z = np.asarray(Z)
    assert Z.dtype == np.float32
    return np.float32(0.5) * (Z.min(axis=0) + Z.max(axis=0))


def _cols(cols):
    return np.asarray(cols, dtype=np.int64).reshape(-1)


def kernel_columns(Z, cols, j0=0, j1=None):
    """(K, terms): K[:, q] = sum_{j0 <= j < j1} exp(-0.5 (z_ij - z_cj)^2) for c = cols[q], float64 from the float32 Z widened
    to float64; terms is the N x len(cols) x (j1 - j0) array of the summands."""
    Z = np.asarray(Z)
    assert Z.dtype == np.float32 and Z.ndim == 2
    j1 = Z.shape[1] if j1 is None else j1
    Zd = Z[:, j0:j1].astype(np.float64)
    d = Zd[:, None, :] - Zd[_cols(cols)][None, :, :]
    terms = np.exp(-0.5 * d * d)
    return terms.sum(axis=2), terms


def scaled_coordinates(Z, j0=0, j1=None):
    """a = (z - mid) sqrt(0.5 log2 e) in float64, mid the float32 midpoint of ALL rows of Z."""
    Z = np.asarray(Z)
    j1 = Z.shape[1] if j1 is None else j1
    return (Z[:, j0:j1].astype(np.float64) - midpoint(Z)[j0:j1].astype(np.float64)) * C_EXP2


def term_rel(a, b):
    """rel of the module docstring for row coordinates a and column coordinates b (broadcast)."""
    return U * (math.log(2.0) * (6.0 * np.abs(a - b) * (np.abs(a) + np.abs(b)) + a * a + b * b + np.abs(2.0 * a * b - b * b)) + 5.0)


def entry_bound(Z, cols, j0=0, j1=None, terms=None):
    """N x len(cols): sum_j rel_j k_j + J 2^-120 (no margin)."""
    a = scaled_coordinates(Z, j0, j1)
    if terms is None:
        terms = kernel_columns(Z, cols, j0, j1)[1]
    rel = term_rel(a[:, None, :], a[_cols(cols)][None, :, :])
    return (rel * terms).sum(axis=2) + a.shape[1] * FLUSH


def edge_columns(N, limit=MAX_PROBES):
    """Probe columns, most important first: the two ends, both sides of the last multiple of 64, of 256 and of 512 below N, the
    middle of the ragged tail, both sides of 64 m for m = 1, 4, 5, 8, 9 (every chunk, stage and subtile boundary of the plan is
    a multiple of 64, every row-block boundary a multiple of 256, whatever chunk width the plan chooses).  Distinct, inside
    [0, N), at most `limit` (<= 48) of them."""
    cand = [0, N - 1]
    last64 = (N - 1) // 64 * 64
    for q in (64, 256, 512):
        b = (N - 1) // q * q
        cand += [b - 1, b]
    cand.append((last64 + N) // 2)
    for m in (1, 4, 5, 8, 9):
        cand += [64 * m - 1, 64 * m]
    out = []
    for c in cand:
        if 0 <= c < N and c not in out:
            out.append(c)
    return out[:min(limit, MAX_PROBES)]


def unit_blocks(N, cols, T):
    """Right-hand sides of T unit vectors each that cover `cols`: a list of (V float32 N x T, columns of that block); the last
    block wraps around to the first columns so that every block is full."""
    cols = list(cols)
    out = []
    for s in range(0, len(cols), T):
        blk = [cols[(s + t) % len(cols)] for t in range(T)]
        V = np.zeros((N, T), dtype=np.float32)
        V[blk, np.arange(T)] = 1.0
        out.append((V, blk))
    return out


# ---- float32 emulation of the compiler kernel's arithmetic (host test only) --------------------------------------------------
def _fma32(x, y, z):
    """One rounding: the float32 product is exact in float64 (48 bits)."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def emulate_terms(Z, cols, j0=0, j1=None):
    """(e, Ea) in float32 with the operations of prep_build_kernel and fact_pair_sum in their order: e is N x C x J', Ea N x J'."""
    Z = np.asarray(Z)
    assert Z.dtype == np.float32
    j1 = Z.shape[1] if j1 is None else j1
    a = ((Z - midpoint(Z)) * C_EXP2_F32)[:, j0:j1]
    assert a.dtype == np.float32
    na2 = -(a * a)
    Ea = np.exp2(na2)
    c = _cols(cols)
    t = _fma32(a[:, None, :], (np.float32(2.0) * a[c])[None, :, :], np.broadcast_to(na2[c][None, :, :], (a.shape[0], c.size, a.shape[1])))
    with np.errstate(under="ignore"):
        e = np.exp2(t)
    assert e.dtype == np.float32 and Ea.dtype == np.float32
    return e, Ea


def emulate_entries(Z, cols, j0=0, j1=None):
    """float32 K[:, cols] as mvm_fact_kernel sums it: per J piece the even and the odd projections in two FMA chains and one
    addition (JT = 1: one product), later pieces added to the slab entry."""
    Z = np.asarray(Z)
    j1 = Z.shape[1] if j1 is None else j1
    e, Ea = emulate_terms(Z, cols, j0, j1)
    slab = None
    with np.errstate(under="ignore"):
        for (j, jt) in j_pieces(j0, j1):
            q = j - j0
            if jt == 1:
                ks = e[:, :, q] * Ea[:, None, q]
            else:
                acc = [np.zeros(e.shape[:2], dtype=np.float32) for _ in range(2)]
                for p in range(jt):
                    acc[p % 2] = _fma32(e[:, :, q + p], np.broadcast_to(Ea[:, None, q + p], e.shape[:2]), acc[p % 2])
                ks = acc[0] + acc[1]
            slab = ks if slab is None else slab + ks
    assert slab.dtype == np.float32
    return slab


# ---- inputs of the GPU cases ---------------------------------------------------------------------------------------------------
def normal_inputs(N, J, seed):
    """Z = 0.9 x standard normal (the distribution of tests/test_fact_asm_gpu.py), float32."""
    return (np.random.default_rng(seed).standard_normal((N, J)) * 0.9).astype(np.float32)


def dense_rhs(N, T, seed):
    """A standard-normal float32 V for the relative 2-norm gate of the dense products (2e-6 per column, from
    tests/test_fact_asm_gpu.py).  That gate divides by the norm of the product.  The entries of K for Z = 0.9 x standard normal
    have mean J / sqrt(1 + 2 * 0.81) = 0.62 J and a standard deviation of about 0.28 sqrt(J), so the product is dominated by
    0.62 J (1^T v) 1 and its norm by |1^T v|, while the float32 accumulation error of a 64-column chunk depends on |v| alone: a
    column whose sum happens to be near zero has the same absolute error over a several times smaller norm (at N = 10303, J =
    20: |1^T v| = 2.7 against 38.6 gives norms of 740 against 3392, and float32 sums of the EXACT entries in chunks of 64
    columns are then already 1.8e-6 from float64 in the first column and 4.0e-7 in the second).  The gate was set on draws
    without such a column, so a draw is taken only if every column has |1^T v| >= sqrt(N) / 8 (which nine in ten standard-normal
    columns have): seeds seed, seed + 1000, ... in turn.  The rule looks at V alone."""
    for k in range(64):
        V = np.random.default_rng(seed + 1000 * k).standard_normal((N, T)).astype(np.float32)
        if (np.abs(V.sum(axis=0, dtype=np.float64)) >= math.sqrt(N) / 8.0).all():
            return V
    raise RuntimeError("no draw passed")


def wide_inputs(N=3001, J=6, seed=11):
    """Z uniform in +-11.2 with the two extreme rows pinned: max|a| = 11.2 * 0.849 = 9.5 (a^2 < 100: fast_ok; beyond rank 64)."""
    Z = np.random.default_rng(seed).uniform(-11.2, 11.2, (N, J)).astype(np.float32)
    if N >= 2:
        Z[0], Z[1] = -11.2, 11.2
    return Z
