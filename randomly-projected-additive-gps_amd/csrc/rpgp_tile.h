// rpgp_tile.h — what the tile-sweep translation units (rpgp_kernels.hip, rpgp_symcache.hip, rpgp_bilinear.hip,
// rpgp_dense_mvm.hip, rpgp_pivchol.hip) share: constants and vector types, the device helpers every sweep inlines, the
// kernel-function policies, the tile plan and the piece dispatch.  Not part of the C-ABI.  Everything here is file-local
// (anonymous namespace) in each of them, as it was when they were one file; the process state they share (g_rotdir,
// g_num_cus) is NOT here: it has one definition in rpgp_kernels.hip (rpgp_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"

using namespace rpgp_internal;   // as_stream, launch_status, g_rotdir, g_num_cus, Taper, ... unqualified in those files

namespace {

constexpr float kExp2Scale = 0.8493218002880191f;  // sqrt(0.5 * log2(e)):  exp(-d^2/2) = exp2(-(c d)^2)
constexpr int kSC = 256;                           // columns staged in LDS per sub-chunk (T <= 4)
// wide right-hand sides stage fewer columns so that LDS (sT = 4*SC*TT floats) still admits several workgroups per CU
template <int TT> struct StageCols { static constexpr int v = (TT > 4) ? 64 : 256; };

typedef float float2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float floatx4m __attribute__((ext_vector_type(4)));

// LDS row stride (floats) for a column's JT coordinates: (stride/4) odd keeps the per-lane
// ds_read_b128 of 16 consecutive columns on 16 distinct 4-bank slots (MI355X_MICROARCH.md §LDS).
template <int JT> struct ColStride { static constexpr int v = (JT % 8 == 0) ? JT + 4 : JT; };

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// DPP wave rotate by one lane (gfx9: wave_rol:1 = 0x134).  Direction is probed once on the host
// (rpgp_init) and passed to kernels as `rotdir`, so correctness does not rest on the mnemonic.
__device__ __forceinline__ float wave_rotate1(float x) {
  int xi = __builtin_bit_cast(int, x);
  // bound_ctrl = true: every lane of a wave rotate has a valid source, and the compiler no longer has to materialise the
  // `old` operand with an extra v_mov_b32 per rotation (24 per two steps in the T = 12 kernel)
  int r = __builtin_amdgcn_update_dpp(0, xi, 0x134, 0xf, 0xf, true);
  return __builtin_bit_cast(float, r);
}

// sum_j exp2(-(a_j - b_j)^2), written on float2 so hipcc emits v_pk_add_f32 / v_pk_mul_f32.
template <int JT>
__device__ __forceinline__ float pair_kernel_sum(const float (&a)[JT], const float (&b)[JT]) {
  if constexpr (JT % 2 == 0) {
    float2v acc = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < JT; j += 2) {
      float2v av = {a[j], a[j + 1]};
      float2v bv = {b[j], b[j + 1]};
      float2v d = av - bv;
      float2v m = -(d * d);
      float2v e = {fast_exp2(m.x), fast_exp2(m.y)};
      acc += e;
    }
    float s;                      // one v_add_f32 (asm): keeps the SLP vectoriser from packing neighbouring rows' adds behind moves
    asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(acc.x), "v"(acc.y));
    return s;
  } else {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      float d = a[j] - b[j];
      acc += fast_exp2(-(d * d));
    }
    return acc;
  }
}

// ---------------------------------------------------------------------------------------------
// Kernel-function policies.  The hot path is KfBase (unweighted sum of 1-D RBFs).  The other members of the
// reference's additive family (`kernel_type` of training_routines.py:47-88, k > 1 sub-kernels of
// :172-174, per-component weights of polynomial_projection_kernels.py:88-98) run through the SAME tile / dense kernels
// with a different policy:
//     K[i,i'] = scale * sum_c w[c] * phi(columns [c*G, (c+1)*G) of Z)
// `pre` is the factor applied to Z when it is loaded (so the inner loop works on prescaled differences dd), `val` the
// 1-D function of dd, `val_grad` additionally returns g with  d phi / d z_i = mulG * g.
// ---------------------------------------------------------------------------------------------
template <int KIND> struct Phi;
template <> struct Phi<RPGP_KIND_RBF> {                 // exp(-d^2 / 2) = exp2(-(c d)^2)
  static constexpr float pre = kExp2Scale;
  static constexpr float mulG = -1.0f / kExp2Scale;
  static __device__ __forceinline__ float val(float dd) { return fast_exp2(-(dd * dd)); }
  static __device__ __forceinline__ void val_grad(float dd, float &phi, float &g) {
    phi = fast_exp2(-(dd * dd));
    g = phi * dd;
  }
};
template <> struct Phi<RPGP_KIND_MATERN15> {            // (1 + sqrt3 r) exp(-sqrt3 r), dd = sqrt3 (z - z')
  static constexpr float pre = 1.7320508075688772f;
  static constexpr float mulG = -1.7320508075688772f;
  static __device__ __forceinline__ float val(float dd) {
    const float u = __builtin_fabsf(dd);
    return (1.0f + u) * fast_exp2(-1.4426950408889634f * u);
  }
  static __device__ __forceinline__ void val_grad(float dd, float &phi, float &g) {
    const float u = __builtin_fabsf(dd);
    const float e = fast_exp2(-1.4426950408889634f * u);
    phi = (1.0f + u) * e;
    g = dd * e;                                         // d phi / d dd = -dd e
  }
};
template <> struct Phi<RPGP_KIND_IMQ> {                 // (1 + r^2)^(-1/2)   (imq_kernel.py:8-9)
  static constexpr float pre = 1.0f;
  static constexpr float mulG = -1.0f;
  static __device__ __forceinline__ float val(float dd) { return __builtin_amdgcn_rsqf(__builtin_fmaf(dd, dd, 1.0f)); }
  static __device__ __forceinline__ void val_grad(float dd, float &phi, float &g) {
    phi = __builtin_amdgcn_rsqf(__builtin_fmaf(dd, dd, 1.0f));
    g = dd * phi * phi * phi;
  }
};
template <> struct Phi<RPGP_KIND_COSINE> {              // cos(pi r) (period 1); v_cos/v_sin take revolutions: dd = (z - z') / 2
  static constexpr float pre = 0.5f;
  static constexpr float mulG = -3.14159265358979323846f;
  static __device__ __forceinline__ float val(float dd) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(dd)); }
  static __device__ __forceinline__ void val_grad(float dd, float &phi, float &g) {
    const float f = __builtin_amdgcn_fractf(dd);
    phi = __builtin_amdgcn_cosf(f);
    g = __builtin_amdgcn_sinf(f);
  }
};

struct KfBase {                                         // the hot path: sum_j exp2(-(a_j - b_j)^2), weights folded in `scale`
  static constexpr float pre = kExp2Scale;
  static constexpr int group = 1;
  static constexpr bool weighted = false;
  template <int JT>
  static __device__ __forceinline__ float pair_sum(const float (&a)[JT], const float (&b)[JT], const float *) {
    return pair_kernel_sum<JT>(a, b);
  }
};

template <int KIND>
struct KfPhi {                                          // weighted sum of 1-D functions
  static constexpr float pre = Phi<KIND>::pre;
  static constexpr float mulG = Phi<KIND>::mulG;
  static constexpr int group = 1;
  static constexpr bool weighted = true;
  template <int JT>
  static __device__ __forceinline__ float pair_sum(const float (&a)[JT], const float (&b)[JT], const float *w) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < JT; ++j) acc = __builtin_fmaf(w[j], Phi<KIND>::val(a[j] - b[j]), acc);
    return acc;
  }
  // per-column gradient factors and per-component values for the bilinear derivative
  template <int JT>
  static __device__ __forceinline__ void pair_grad(const float (&a)[JT], const float *b, const float *w, float S,
                                                   float (&accG)[JT], float (&accC)[JT]) {
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      float phi, g;
      Phi<KIND>::val_grad(a[j] - b[j], phi, g);
      accG[j] = __builtin_fmaf(S * w[j], g, accG[j]);
      accC[j] = __builtin_fmaf(S, phi, accC[j]);
    }
  }
};

template <int G>
struct KfGroupRbf {                                     // weighted sum of G-dimensional RBFs (products of G 1-D RBFs)
  static constexpr float pre = kExp2Scale;
  static constexpr float mulG = -1.0f / kExp2Scale;
  static constexpr int group = G;
  static constexpr bool weighted = true;
  template <int JT>
  static __device__ __forceinline__ float pair_sum(const float (&a)[JT], const float (&b)[JT], const float *w) {
    static_assert(JT % G == 0, "column pieces must hold whole groups");
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < JT / G; ++c) {
      float r2 = 0.f;
#pragma unroll
      for (int m = 0; m < G; ++m) {
        const float dd = a[c * G + m] - b[c * G + m];
        r2 = __builtin_fmaf(dd, dd, r2);
      }
      acc = __builtin_fmaf(w[c], fast_exp2(-r2), acc);
    }
    return acc;
  }
  template <int JT>
  static __device__ __forceinline__ void pair_grad(const float (&a)[JT], const float *b, const float *w, float S,
                                                   float (&accG)[JT], float (&accC)[JT / G]) {
#pragma unroll
    for (int c = 0; c < JT / G; ++c) {
      float dd[G];
      float r2 = 0.f;
#pragma unroll
      for (int m = 0; m < G; ++m) {
        dd[m] = a[c * G + m] - b[c * G + m];
        r2 = __builtin_fmaf(dd[m], dd[m], r2);
      }
      const float phi = fast_exp2(-r2);
      const float sw = S * w[c] * phi;
#pragma unroll
      for (int m = 0; m < G; ++m) accG[c * G + m] = __builtin_fmaf(sw, dd[m], accG[c * G + m]);
      accC[c] = __builtin_fmaf(S, phi, accC[c]);
    }
  }
};

template <int JT>
__device__ __forceinline__ void lds_load_cols(const float *sB, int idx, float (&b)[JT]) {
  constexpr int STR = ColStride<JT>::v;
  const float *p = sB + idx * STR;
  if constexpr (JT % 4 == 0) {
#pragma unroll
    for (int j = 0; j < JT; j += 4) {
      float4v q = *reinterpret_cast<const float4v *>(p + j);
      b[j] = q.x; b[j + 1] = q.y; b[j + 2] = q.z; b[j + 3] = q.w;
    }
  } else if constexpr (JT % 2 == 0) {
#pragma unroll
    for (int j = 0; j < JT; j += 2) {
      float2v q = *reinterpret_cast<const float2v *>(p + j);
      b[j] = q.x; b[j + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < JT; ++j) b[j] = p[j];
  }
}

template <int TT>
__device__ __forceinline__ void lds_load_vec(const float *sV, int idx, float (&v)[TT]) {
  const float *p = sV + idx * TT;
  if constexpr (TT % 4 == 0) {
#pragma unroll
    for (int t = 0; t < TT; t += 4) {
      float4v q = *reinterpret_cast<const float4v *>(p + t);
      v[t] = q.x; v[t + 1] = q.y; v[t + 2] = q.z; v[t + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < TT; ++t) v[t] = p[t];
  }
}

// Linear workgroup index -> (row block, column chunk).  Row block b owns ceil((N - cbase(b)) / chunk) chunks (cbase = its
// own first row for the symmetric sweep, 0 otherwise); workgroups are numbered row block by row block.  A rank's
// launch covers the contiguous range [w0, w0 + gridDim.x) of that numbering (pair-sharding at workgroup granularity).
// `used`: a translation unit whose callers all pass ONE block size (rpgp_bilinear.hip: BR = 512, sym) would otherwise have that
// constant propagated into this function before it is inlined; the sweeps were tuned and measured as one file, where the
// callers differ and no such specialisation happens, and bilinear_sym_kernel allocates its scalar registers differently
// after it.  With the attribute every kernel's code equals the single-file build's (tools/kernel_code_diff.py).
__attribute__((used)) __device__ __forceinline__ void wg_to_tile(int lin, int N, int BR, int chunk, bool sym, int &rb, int &kchunk) {
  int b = 0, acc = 0;
  for (;;) {
    const int cbase = sym ? b * BR : 0;
    const int cb = (N - cbase + chunk - 1) / chunk;
    if (lin < acc + cb) break;
    acc += cb;
    ++b;
  }
  rb = b;
  kchunk = lin - acc;
}

// ------------------------------- host side: pieces, tile plan, family dispatch ----------------------------

// decomposition of a j-range into the compiled JT pieces
// 10 / 5 / 3 make the J-shards of 2 / 4 / 8 ranks (J = 20) a single sweep per MVM
const int kJPieces[] = {20, 10, 8, 5, 4, 3, 2, 1};
inline int next_j_piece(int remaining) {
  for (int p : kJPieces)
    if (p <= remaining) return p;
  return 1;
}
const int kTPieces[] = {12, 4, 1};
inline int next_t_piece(int remaining) {
  // prefer the smallest compiled piece that covers the remainder, else the largest
  if (remaining >= 12) return 12;
  if (remaining > 4) return 12;
  if (remaining > 1) return 4;
  return 1;
}

struct TilePlan {
  int R;           // rows per lane
  int BR;          // rows per workgroup
  int nrb;         // row blocks
  int chunk_cols;  // columns per workgroup (multiple of 64)
  int total_wg;    // workgroups of the whole problem (row block by row block)
  int w0, w1;      // workgroup range of this call (pair-sharding); default = all
  int rb0, rb1;    // row blocks touched by that range
  int row0, rows;  // first row / number of rows of those row blocks (slab addressing)
  int maxchunks;   // chunk slabs per row (the most chunks any touched row block has)
  bool partial;    // the range is a strict subset: slabs are zero-initialised before the sweep
  rpgp_internal::Taper taper;   // first row blocks of the half / quarter / eighth-size chunks (nrb = none; rpgp_internal.h)
};

inline int plan_chunk(double pairs, int BR, bool big, double target_wgs = 4608.0) {
  // aim for ~4600 workgroups (6 rounds of 3 workgroups per CU) so the dispatcher can balance the triangular sweep;
  // chunks are multiples of 64 columns (one rotation subtile), at least 128 (64 for small problems)
  double cc = pairs / ((double)BR * target_wgs);
  int chunk = (int)((cc + 63.0) / 64.0) * 64;
  const int min_chunk = big ? 128 : 64;
  if (chunk < min_chunk) chunk = min_chunk;
  if (chunk > 8192) chunk = 8192;
  return chunk;
}

inline int chunks_of(const TilePlan &p, int64_t N, bool sym, int b) {
  const long long cbase = sym ? (long long)b * p.BR : 0;
  const int cb = rpgp_internal::taper_chunk(b, p.chunk_cols, p.taper.tb1, p.taper.tb2, p.taper.tb3);
  return (int)((N - cbase + cb - 1) / cb);
}

// `world`-way split: the chunk size is chosen for the per-rank share of the pairs so that every rank still launches
// a few thousand workgroups; rank r gets workgroups [total*r/world, total*(r+1)/world).
inline TilePlan make_plan(int64_t M, int64_t N, bool sym, int T, int world = 1, int rank = 0, bool r1 = false,
                          int br_override = 0, double target_wgs = 4608.0, bool taper = false, int chunk_override = 0) {
  TilePlan p;
  // two rows per lane halve the LDS traffic per pair (measured: one row per lane is 20 % slower even at T = 11)
  // measured (tools/time_small.py): with T > 4 right-hand sides two rows per lane win from N ~ 4k up (362 vs 429 us at
  // N = 14939, T = 11); with T <= 4 only once there are enough 512-row workgroups to fill the chip (N >~ 10k)
  const long long r2_min = T > 4 ? 4096 : 10240;
  p.R = (M >= r2_min && !r1) ? 2 : 1;   // r1: the family policies are instantiated with one row per lane only
  p.BR = 256 * p.R;
  if (br_override > 0) {                // matrix-core kernels (rpgp_mfma.hip): 4 waves x one 32-row MFMA tile
    p.R = 0;
    p.BR = br_override;
  }
  p.nrb = (int)((M + p.BR - 1) / p.BR);
  const double pairs = (sym ? 0.5 * (double)M * (double)N : (double)M * (double)N) / (double)(world > 0 ? world : 1);
  p.chunk_cols = chunk_override > 0 ? chunk_override : plan_chunk(pairs, p.BR, M >= 16384, target_wgs);
  p.taper = rpgp_internal::Taper{p.nrb, p.nrb, p.nrb};
  if (taper && sym && world <= 1 && M == N && p.chunk_cols >= 256) {
    // remaining share of the pairs after row block b is ((N - b BR) / N)^2: half-size chunks for the last 20 % of the work,
    // quarter-size for the last 6 %, eighth-size for the last 1.5 % (single GPU only: pair-sharding splits by workgroup COUNT)
    const double fr[3] = {0.20, 0.06, 0.015};
    int tb[3];
    for (int l = 0; l < 3; ++l) {
      const double cols = std::sqrt(fr[l]) * (double)N;
      int b = (int)(((double)N - cols) / (double)p.BR);
      if (b < 0) b = 0;
      if (b > p.nrb) b = p.nrb;
      tb[l] = b;
    }
    p.taper = rpgp_internal::Taper{tb[0], tb[1], tb[2]};
  }
  long long total = 0;
  for (int b = 0; b < p.nrb; ++b) total += chunks_of(p, N, sym, b);
  p.total_wg = (int)total;
  if (world <= 1) {
    p.w0 = 0;
    p.w1 = p.total_wg;
  } else {
    p.w0 = (int)(total * rank / world);
    p.w1 = (int)(total * (rank + 1) / world);
  }
  p.partial = !(p.w0 == 0 && p.w1 == p.total_wg);
  // row blocks touched by [w0, w1)
  p.rb0 = 0;
  p.rb1 = 0;
  long long acc = 0;
  bool started = false;
  for (int b = 0; b < p.nrb; ++b) {
    const int cb = chunks_of(p, N, sym, b);
    if (!started && p.w0 < acc + cb) { p.rb0 = b; started = true; }
    if (p.w1 > acc) p.rb1 = b + 1;
    acc += cb;
  }
  if (p.w1 <= p.w0) { p.rb0 = 0; p.rb1 = 0; }
  p.row0 = p.rb0 * p.BR;
  const long long rend = (long long)p.rb1 * p.BR < M ? (long long)p.rb1 * p.BR : M;
  p.rows = (int)(rend - p.row0 > 0 ? rend - p.row0 : 0);
  p.maxchunks = 1;
  for (int b = p.rb0; b < p.rb1; ++b) {
    const int cb = chunks_of(p, N, sym, sym ? b : 0);
    if (cb > p.maxchunks) p.maxchunks = cb;
  }
  return p;
}

inline size_t plan_workspace_floats(const TilePlan &p, int64_t N, int T, bool sym) {
  size_t f = (size_t)p.maxchunks * p.rows * T;
  if (sym) f += (size_t)(p.rb1 - p.rb0) * N * T;
  return f;
}

inline size_t mvm_workspace_floats(int64_t M, int64_t N, int T, bool sym, int world = 1, int rank = 0, bool r1 = false) {
  size_t f = plan_workspace_floats(make_plan(M, N, sym, T, world, rank, r1), N, T, sym);
  if (sym && !r1 && M == N && world <= 1) {       // the tapered plan of the single-GPU T = 1 prepared path (more chunk slabs)
    const size_t g = plan_workspace_floats(make_plan(M, N, sym, T, world, rank, false, 0, 4608.0, true), N, T, sym);
    if (g > f) f = g;
  }
  return f;
}

// ---- generalised family dispatch ---------------------------------------------------------------
template <int V> using IntC = std::integral_constant<int, V>;

// calls f(IntC<piece>{}) for the compiled column piece `jt` (next_j_piece) / right-hand-side piece `tt` (next_t_piece)
template <class F>
int with_j_piece(int jt, F &&f) {
  switch (jt) {
    case 20: return f(IntC<20>{});
    case 10: return f(IntC<10>{});
    case 8: return f(IntC<8>{});
    case 5: return f(IntC<5>{});
    case 4: return f(IntC<4>{});
    case 3: return f(IntC<3>{});
    case 2: return f(IntC<2>{});
    default: return f(IntC<1>{});
  }
}
template <class F>
int with_t_piece(int tt, F &&f) {
  switch (tt) {
    case 1: return f(IntC<1>{});
    case 4: return f(IntC<4>{});
    default: return f(IntC<12>{});
  }
}

// calls f(policy object) for the (kind, group) pair; RPGP_EINVAL for combinations that are not instantiated
template <class F>
int with_family_policy(int kind, int group, F &&f) {
  switch (kind) {
    case RPGP_KIND_RBF:
      switch (group) {
        case 1: return f(KfGroupRbf<1>{});
        case 2: return f(KfGroupRbf<2>{});
        case 3: return f(KfGroupRbf<3>{});
        case 4: return f(KfGroupRbf<4>{});
        case 5: return f(KfGroupRbf<5>{});
        case 8: return f(KfGroupRbf<8>{});
        case 10: return f(KfGroupRbf<10>{});
        case 20: return f(KfGroupRbf<20>{});
        default: return RPGP_EINVAL;
      }
    case RPGP_KIND_MATERN15: return group == 1 ? f(KfPhi<RPGP_KIND_MATERN15>{}) : RPGP_EINVAL;
    case RPGP_KIND_IMQ: return group == 1 ? f(KfPhi<RPGP_KIND_IMQ>{}) : RPGP_EINVAL;
    case RPGP_KIND_COSINE: return group == 1 ? f(KfPhi<RPGP_KIND_COSINE>{}) : RPGP_EINVAL;
    default: return RPGP_EINVAL;
  }
}

// column pieces: {10, 4, 2, 1} columns for 1-D sub-kernels; for G-dimensional groups as many whole groups as fit in
// ~10 columns (fewer passes over the pair space), then single groups
template <int G> struct GroupBig { static constexpr int v = (G <= 5) ? G * (10 / G) : G; };
template <class KF>
inline int family_piece(int remaining) {
  if (KF::group > 1) return remaining >= GroupBig<KF::group>::v ? GroupBig<KF::group>::v : KF::group;
  return remaining >= 10 ? 10 : (remaining >= 4 ? 4 : (remaining >= 2 ? 2 : 1));
}
template <class KF, class F>
int with_family_piece(int jt, F &&f) {
  if constexpr (KF::group > 1) {
    if (jt == GroupBig<KF::group>::v) return f(IntC<GroupBig<KF::group>::v>{});
    return f(IntC<KF::group>{});
  } else {
    switch (jt) {
      case 10: return f(IntC<10>{});
      case 4: return f(IntC<4>{});
      case 2: return f(IntC<2>{});
      default: return f(IntC<1>{});
    }
  }
}

inline int family_check(const rpgp_family *fam, int ld_a, int ld_b) {
  if (!fam || !fam->weights || fam->ncomp <= 0 || fam->group <= 0) return RPGP_EINVAL;
  const long long cols = (long long)fam->ncomp * fam->group;
  if (cols > ld_a || cols > ld_b) return RPGP_EINVAL;
  return with_family_policy(fam->kind, fam->group, [](auto) { return 0; });
}

}  // namespace
