// rpgp_kernels.hip — the fused tile MVM (direct and prepared / factorised forms, additive and generalised family), its slab
// reduce, the dense block, the projection, space_equally, and the library's init / version / error / profile hooks with their
// entries of the C-ABI of include/rpgp.h.  What the tile sweeps share is rpgp_tile.h; the other users of it are one file per
// concern: rpgp_symcache.hip (packed symmetric cache), rpgp_bilinear.hip (derivative), rpgp_dense_mvm.hip (cached-K GEMM / GEMV),
// rpgp_pivchol.hip (pivoted Cholesky).  The process state (g_rotdir, g_num_cus) is defined here, once.
//
// Hot path: the additive randomly-projected RBF kernel
//     K[i,i'] = scale * sum_j exp(-0.5 (Z[i,j]-Z[i',j])^2)
// applied to a block of vectors without ever storing K.  gfx950 only: wave64, DPP wave rotates,
// packed fp32 VALU, 160 KB LDS.  No CUDA/compat paths.
//
// Tiling of the fused MVM (mvm_tile_kernel):
//   * a 256-thread workgroup owns BR = 256*R rows; each lane keeps R rows' JT projected coordinates
//     (pre-multiplied by sqrt(0.5*log2 e) so the inner loop is sub, mul, v_exp_f32, add) and its
//     R*TT row accumulators in VGPRs;
//   * the workgroup sweeps one chunk of columns, staged 256 at a time in LDS with coalesced loads;
//   * inside a 64-column subtile, lane l visits column (l + s) mod 64 at step s (a per-lane LDS read,
//     bank-conflict free for the padded strides used).  Because every lane holds a DIFFERENT column,
//     the transposed product  out[i'] += K[i,i'] v[i]  needs no cross-lane reduction: its accumulator
//     is rotated one lane per step with a DPP wave rotate, so after 64 steps lane l holds column l.
//     Each unordered pair is therefore evaluated once (SYM=true), halving the exp count;
//   * partial results go to per-(row-block / chunk) slabs in a caller-provided workspace and a small
//     reduce kernel sums them in a fixed order: deterministic, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stddef.h>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"
#include "rpgp_tile.h"

namespace {

__global__ void probe_rotate_kernel(int *out) {
  float x = (float)threadIdx.x;
  float y = wave_rotate1(x);
  out[threadIdx.x] = (int)y;
}

// ---------------------------------------------------------------------------------------------
// Fused MVM tile kernel.  grid = (max chunks per row block, row blocks); block = 256.
//   SYM : Z1 == Z2 (N x N), columns of row block rb start at its own first row (upper triangle incl.
//         the diagonal block); the transposed product is produced for columns beyond the diagonal block.
//   !SYM: rectangular M x N, every row block sweeps all columns.
// slabR[k][row][T]  : partial row products of chunk k           (k < chunks of that row block)
// slabT[rb][col][T] : partial transposed products of row block rb (only col >= (rb+1)*BR written)
// ---------------------------------------------------------------------------------------------
template <int JT, int TT, int R, bool SYM, class KF = KfBase>
__global__ __launch_bounds__(256) void mvm_tile_kernel(
    const float *__restrict__ Z1, const float *__restrict__ Z2, const float *__restrict__ V,
    float *__restrict__ slabR, float *__restrict__ slabT, int M, int N, int ldz1, int ldz2, int ldv,
    int j0, int t0, int tcnt, int chunk_cols, int rotdir, int accumulate, int w0, int rb_first, int slab_row0,
    int slab_rows, const float *__restrict__ wts) {
  constexpr int BR = 256 * R;
  constexpr int SC = StageCols<TT>::v;
  constexpr int STR = ColStride<JT>::v;
  __shared__ __attribute__((aligned(16))) float sB[SC * STR];
  __shared__ __attribute__((aligned(16))) float sV[SC * TT];
  __shared__ __attribute__((aligned(16))) float sT[SYM ? 4 * SC * TT : 4];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, SYM ? N : N, BR, chunk_cols, SYM, rb, kchunk);
  const int r0 = rb * BR;
  const int cbase = SYM ? r0 : 0;
  const long long cb = (long long)cbase + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;

  // component weights of this column piece (uniform; unused by the hot-path policy)
  float wreg[KF::weighted ? JT / KF::group : 1];
  if constexpr (KF::weighted) {
#pragma unroll
    for (int c = 0; c < JT / KF::group; ++c) wreg[c] = wts[j0 / KF::group + c];
  } else {
    wreg[0] = 0.f;
  }

  float a[R][JT];
  float vrow[R][TT];
  float accR[R][TT];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    const bool valid = row < M;
    // unconditional loads from a clamped row (a load under a condition compiles to a branch + s_waitcnt vmcnt(0) per
    // element: 40 serial round trips here); rows beyond M carry a valid row's coordinates, are never stored, and their
    // right-hand side is masked to zero, so they contribute nothing
    const int rowc = valid ? row : M - 1;
#pragma unroll
    for (int j = 0; j < JT; ++j) a[r][j] = Z1[(size_t)rowc * ldz1 + j0 + j] * KF::pre;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if constexpr (SYM) vrow[r][t] = V[(size_t)rowc * ldv + t0 + (t < tcnt ? t : 0)] * ((valid && t < tcnt) ? 1.f : 0.f);
      else vrow[r][t] = 0.f;
      accR[r][t] = 0.f;
    }
  }

  for (int c0 = c_begin; c0 < c_end; c0 += SC) {
    __syncthreads();
    if (tid < SC) {
      const int col = c0 + tid;
      const bool cv = col < c_end;
      const int colc = cv ? col : N - 1;            // (same: clamped column, its right-hand side masked to zero)
      float zc[JT], vc[TT];
#pragma unroll
      for (int j = 0; j < JT; ++j) zc[j] = Z2[(size_t)colc * ldz2 + j0 + j];
#pragma unroll
      for (int t = 0; t < TT; ++t) vc[t] = V[(size_t)colc * ldv + t0 + (t < tcnt ? t : 0)];
#pragma unroll
      for (int j = 0; j < JT; ++j) sB[tid * STR + j] = zc[j] * KF::pre;
#pragma unroll
      for (int t = 0; t < TT; ++t) sV[tid * TT + t] = vc[t] * ((cv && t < tcnt) ? 1.f : 0.f);
    }
    __syncthreads();
    const int ncol = c_end - c0;
    const int nsub = ncol >= SC ? SC / 64 : (ncol + 63) / 64;
    for (int sub = 0; sub < nsub; ++sub) {
      const bool doT = SYM && (c0 + sub * 64 >= r0 + BR);
      float accT[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) accT[t] = 0.f;
      if (doT) {
#pragma unroll 2
        for (int s = 0; s < 64; ++s) {
          const int idx = sub * 64 + ((lane + rotdir * s) & 63);
          float b[JT], v[TT];
          lds_load_cols<JT>(sB, idx, b);
          lds_load_vec<TT>(sV, idx, v);
          float tsum[TT];
#pragma unroll
          for (int t = 0; t < TT; ++t) tsum[t] = accT[t];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float ks = KF::template pair_sum<JT>(a[r], b, wreg);
#pragma unroll
            for (int t = 0; t < TT; ++t) {
              accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
              tsum[t] = __builtin_fmaf(ks, vrow[r][t], tsum[t]);
            }
          }
#pragma unroll
          for (int t = 0; t < TT; ++t) accT[t] = wave_rotate1(tsum[t]);
        }
      } else {
#pragma unroll 2
        for (int s = 0; s < 64; ++s) {
          const int idx = sub * 64 + ((lane + s) & 63);
          float b[JT], v[TT];
          lds_load_cols<JT>(sB, idx, b);
          lds_load_vec<TT>(sV, idx, v);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float ks = KF::template pair_sum<JT>(a[r], b, wreg);
#pragma unroll
            for (int t = 0; t < TT; ++t) accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
          }
        }
      }
      if constexpr (SYM) {
#pragma unroll
        for (int t = 0; t < TT; ++t) sT[(wave * SC + sub * 64 + lane) * TT + t] = accT[t];
      }
    }
    if constexpr (SYM) {
      __syncthreads();
      const int col = c0 + tid;
      if (tid < SC && col < c_end && col >= r0 + BR) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          if (t < tcnt) {
            float sum = sT[(0 * SC + tid) * TT + t] + sT[(1 * SC + tid) * TT + t] +
                        sT[(2 * SC + tid) * TT + t] + sT[(3 * SC + tid) * TT + t];
            float *dst = slabT + ((size_t)(rb - rb_first) * N + col) * ldv + t0 + t;
            *dst = accumulate ? *dst + sum : sum;
          }
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    if (row < M) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (t < tcnt) {
          float *dst = slabR + ((size_t)kchunk * slab_rows + (row - slab_row0)) * ldv + t0 + t;
          *dst = accumulate ? *dst + accR[r][t] : accR[r][t];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Factorised fast path ("prepared" MVM).
//   exp2(-(a-b)^2) = exp2(-a^2) * exp2(2ab - b^2)
// so per pair-term the loop is  t = fma(a, 2b, -b^2);  e = v_exp_f32(t);  K = fma(e, exp2(-a^2), K)
// (3 VALU issues instead of 4: the subtract disappears).  2ab - b^2 <= a^2 must stay below the fp32 exponent range,
// so rpgp_prepare centres every projection at the midpoint of its range and records max|a|; the host only takes this
// path when max a^2 < kFactMaxSq, otherwise the exact direct kernel above is used.
// prep buffer: [header 256 B][mid J floats, padded to 256 B][rowdat N*J float2 {a, Ea}][coldat N*J float2 {2a, -a^2}]
// ---------------------------------------------------------------------------------------------
constexpr float kFactMaxSq = 100.0f;   // a^2 bound (|z - mid| < 11.8): exp2(100) is far inside fp32 range
constexpr int kPrepHeaderFloats = 64;
constexpr int kPrepMidFloats = 64;     // J <= 64 projections per prepared buffer

struct PrepLayout {
  float *header;
  float *mid;
  float2v *rowdat;
  float2v *coldat;
};

__host__ __device__ inline PrepLayout prep_layout(void *prep, long long N, int J) {
  PrepLayout L;
  L.header = reinterpret_cast<float *>(prep);
  L.mid = L.header + kPrepHeaderFloats;
  L.rowdat = reinterpret_cast<float2v *>(L.mid + kPrepMidFloats);
  L.coldat = L.rowdat + (size_t)N * J;
  return L;
}

// NaN-propagating min / max so that non-finite inputs are caught by the range guard
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }

// per-block partial min/max of every projection.  Thread t handles projection t % J of rows n0 + t / J, n0 + t / J + 256 / J, ...;
// eight rows' loads are requested together (clamped to a valid row, masked afterwards: a loop of one load per trip is a chain of
// dependent round trips — 60 us at C4 in its first form, VERDICT r5 #6a)
__global__ __launch_bounds__(256) void prep_minmax_kernel(const float *__restrict__ Z, float *__restrict__ part,
                                                          long long N, int ldz, int J, long long rows_per_block) {
  __shared__ float smin[256], smax[256];
  const long long n0 = (long long)blockIdx.x * rows_per_block;
  const long long n1 = (n0 + rows_per_block < N) ? n0 + rows_per_block : N;
  const int j = threadIdx.x % J;
  const int rstep = 256 / J;
  float mn = 3.4e38f, mx = -3.4e38f;
  if ((int)threadIdx.x < rstep * J && n0 < n1) {
    for (long long n = n0 + threadIdx.x / J; n < n1; n += 8LL * rstep) {
      float z[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long long r = n + (long long)u * rstep;
        z[u] = Z[(r < n1 ? r : n1 - 1) * ldz + j];            // (a clamped row repeats a value of this thread's own column)
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        mn = min_nan(mn, z[u]);
        mx = max_nan(mx, z[u]);
      }
    }
  }
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  __syncthreads();
  if ((int)threadIdx.x < J) {
    for (int t = threadIdx.x + J; t < rstep * J; t += J) {
      mn = min_nan(mn, smin[t]);
      mx = max_nan(mx, smax[t]);
    }
    part[((size_t)blockIdx.x * J + threadIdx.x) * 2 + 0] = mn;
    part[((size_t)blockIdx.x * J + threadIdx.x) * 2 + 1] = mx;
  }
}

__global__ __launch_bounds__(256) void prep_finish_kernel(const float *__restrict__ part, int nparts, int J,
                                                          float *__restrict__ header, float *__restrict__ mid) {
  __shared__ float smin[256], smax[256], shalf[64];
  // thread t folds the partials p = t / J, t / J + 256 / J, ... of projection t % J (min / max are exact: any order), eight
  // records in flight at a time
  const int j = threadIdx.x % J, pstep = 256 / J;
  float mn = 3.4e38f, mx = -3.4e38f;
  if ((int)threadIdx.x < pstep * J) {
    const float2v *pr = reinterpret_cast<const float2v *>(part);
    for (int p = threadIdx.x / J; p < nparts; p += 8 * pstep) {
      float2v v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = p + u * pstep;
        v[u] = pr[(size_t)(q < nparts ? q : nparts - 1) * J + j];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        mn = min_nan(mn, v[u].x);
        mx = max_nan(mx, v[u].y);
      }
    }
  }
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  __syncthreads();
  if ((int)threadIdx.x < J) {
    for (int t = threadIdx.x + J; t < pstep * J; t += J) {
      mn = min_nan(mn, smin[t]);
      mx = max_nan(mx, smax[t]);
    }
    mid[j] = 0.5f * (mn + mx);
    shalf[j] = 0.5f * (mx - mn) * kExp2Scale;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.f;
    bool finite = true;
    for (int q = 0; q < J; ++q) {
      finite = finite && (shalf[q] == shalf[q]) && (shalf[q] < 3.0e38f);
      m = shalf[q] > m ? shalf[q] : m;
    }
    header[1] = m;                                             // max |a|
    reinterpret_cast<int *>(header)[0] = (finite && m * m < kFactMaxSq) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void prep_build_kernel(const float *__restrict__ Z, const float *__restrict__ mid,
                                                         float2v *__restrict__ rowdat, float2v *__restrict__ coldat,
                                                         long long N, int ldz, int J) {
  const long long total = N * J;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long n = g / J;
    const int j = (int)(g % J);
    const float a = (Z[n * ldz + j] - mid[j]) * kExp2Scale;
    const float na2 = -(a * a);
    rowdat[g] = float2v{a, fast_exp2(na2)};
    coldat[g] = float2v{2.0f * a, na2};
  }
}

// LDS record of one column: NP = ceil(JT/2) float4 {b2_even, b2_odd, nb2_even, nb2_odd}; stride padded so that
// (stride/4) is odd (conflict-free per-lane ds_read_b128)
template <int JT> struct FactStride {
  static constexpr int np = (JT + 1) / 2;
  static constexpr int v = (np % 2 == 0) ? 4 * np + 4 : 4 * np;
};

// K(i, c) partial sum over JT projections in factorised form; q points at this column's packed LDS record
// [pair p: b2_{2p}, b2_{2p+1}, nb2_{2p}, nb2_{2p+1}] (JT even) or [b2, nb2] (JT == 1)
// ASMADD: the horizontal add of the packed sum as ONE v_add_f32 written in asm.  Left to the compiler, the SLP vectoriser
// packs the two rows' adds of the T = 1 loop into a v_pk_add_f32 behind three v_mov_b32 each (6 moves + 2 packed adds per two
// steps); the asm form measured 2.352 against 2.365-2.388 ms alternating in one process on one box (4 of 4 pairs).
template <int JT, bool ASMADD = false>
__device__ __forceinline__ float fact_pair_sum(const float2v (&ap)[(JT + 1) / 2], const float2v (&ea)[(JT + 1) / 2],
                                               const float *q) {
  if constexpr (JT != 1) {
    // odd JT: the last record's second slot is padding (b2 = 0, nb2 = -1e30 -> e = 0, and Ea = 0 on the row side)
    float2v acc = {0.f, 0.f};
#pragma unroll
    for (int p = 0; p < (JT + 1) / 2; ++p) {
      const float4v c = *reinterpret_cast<const float4v *>(q + 4 * p);
      const float2v b2 = {c.x, c.y};
      const float2v nb2 = {c.z, c.w};
      const float2v t = __builtin_elementwise_fma(ap[p], b2, nb2);
      const float2v e = {fast_exp2(t.x), fast_exp2(t.y)};
      acc = __builtin_elementwise_fma(e, ea[p], acc);
    }
    if constexpr (ASMADD) {
      float s;
      asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(acc.x), "v"(acc.y));
      return s;
    } else {
      return acc.x + acc.y;
    }
  } else {
    const float t = __builtin_fmaf(ap[0].x, q[0], q[1]);
    return fast_exp2(t) * ea[0].x;
  }
}

template <int JT, int TT, int R>
__global__ __launch_bounds__(256) void mvm_fact_kernel(const float2v *__restrict__ rowdat,
                                                       const float2v *__restrict__ coldat,
                                                       const float *__restrict__ V, float *__restrict__ slabR,
                                                       float *__restrict__ slabT, int N, int J, int ldv, int j0, int t0,
                                                       int tcnt, int chunk_cols, int rotdir, int accumulate,
                                                       int w0, int rb_first, int slab_row0, int slab_rows) {
  constexpr int BR = 256 * R;
  constexpr int SC = StageCols<TT>::v;
  constexpr int NP = (JT + 1) / 2;
  constexpr int STR = (JT == 1) ? 2 : FactStride<JT>::v;
  __shared__ __attribute__((aligned(16))) float sB[SC * STR];
  __shared__ __attribute__((aligned(16))) float sV[SC * TT];
  __shared__ __attribute__((aligned(16))) float sT[4 * SC * TT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, N, BR, chunk_cols, true, rb, kchunk);
  const int r0 = rb * BR;
  const long long cb = (long long)r0 + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;

  float2v ap[R][NP], ea[R][NP];
  float vrow[R][TT], accR[R][TT];
  // Unconditional loads from clamped addresses, masked by a multiply: a load under a condition — or a select next to the
  // load — compiles to a branch with its own s_waitcnt vmcnt(0), i.e. 20+ SERIAL round trips in this prologue and 10 per
  // stage below (round 3, same-box A/B: T = 1 2.314 -> 2.278 ms, T = 11 block 3.26 -> 3.19 ms, N = 7372 T = 11 125 -> 117 us).
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    const bool valid = row < N;
    const int rowc = valid ? row : N - 1;
    const float vm = valid ? 1.f : 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float2v x0 = rowdat[(size_t)rowc * J + j0 + 2 * p];
      float2v x1 = {0.f, 0.f};
      if (2 * p + 1 < JT) x1 = rowdat[(size_t)rowc * J + j0 + 2 * p + 1];
      ap[r][p] = float2v{x0.x, x1.x};
      ea[r][p] = float2v{x0.y * vm, x1.y * vm};     // invalid rows: Ea = 0 -> K = 0
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int tc = t < tcnt ? t : 0;
      vrow[r][t] = V[(size_t)rowc * ldv + t0 + tc] * ((valid && t < tcnt) ? 1.f : 0.f);
      accR[r][t] = 0.f;
    }
  }

  for (int c0 = c_begin; c0 < c_end; c0 += SC) {
    __syncthreads();
    if (tid < SC) {
      const int col = c0 + tid;
      const bool cv = col < c_end;
      if constexpr (JT == 1) {
        float2v x = {0.f, -1.0e30f};
        if (cv) x = coldat[(size_t)col * J + j0];
        sB[tid * STR + 0] = x.x;
        sB[tid * STR + 1] = x.y;
      } else {
        const int colc = cv ? col : N - 1;
        const float cm = cv ? 1.f : 0.f, padv = cv ? 0.f : -1.0e30f;     // padded columns: b2 = 0, nb2 = -1e30 -> exp2 = 0
        float2v y0[NP], y1[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          y0[p] = coldat[(size_t)colc * J + j0 + 2 * p];
          y1[p] = float2v{0.f, -1.0e30f};
          if (2 * p + 1 < JT) y1[p] = coldat[(size_t)colc * J + j0 + 2 * p + 1];
        }
        float vv[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) vv[t] = V[(size_t)colc * ldv + t0 + (t < tcnt ? t : 0)];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const bool has1 = 2 * p + 1 < JT;
          *reinterpret_cast<float4v *>(&sB[tid * STR + 4 * p]) =
              float4v{y0[p].x * cm, has1 ? y1[p].x * cm : 0.f, __builtin_fmaf(y0[p].y, cm, padv),
                      has1 ? __builtin_fmaf(y1[p].y, cm, padv) : -1.0e30f};
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) sV[tid * TT + t] = vv[t] * ((cv && t < tcnt) ? 1.f : 0.f);
      }
      if constexpr (JT == 1) {
#pragma unroll
        for (int t = 0; t < TT; ++t)
          sV[tid * TT + t] = (cv && t < tcnt) ? V[(size_t)col * ldv + t0 + t] : 0.f;
      }
    }
    __syncthreads();
    const int ncol = c_end - c0;
    const int nsub = ncol >= SC ? SC / 64 : (ncol + 63) / 64;
    for (int sub = 0; sub < nsub; ++sub) {
      const bool doT = (c0 + sub * 64 >= r0 + BR);
      float accT[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) accT[t] = 0.f;
      if (doT) {
#pragma unroll 2
        for (int s = 0; s < 64; ++s) {
          const int idx = sub * 64 + ((lane + rotdir * s) & 63);
          float v[TT];
          lds_load_vec<TT>(sV, idx, v);
          float tsum[TT];
#pragma unroll
          for (int t = 0; t < TT; ++t) tsum[t] = accT[t];
          // (24-bit multiply: v_mul_lo_u32 is a quarter-rate instruction, one per step in this loop)
          const float *colrec = sB + __mul24(idx, STR);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float ks = fact_pair_sum<JT, true>(ap[r], ea[r], colrec);     // (T = 11 block: 3.32 -> 3.29 ms as well)
#pragma unroll
            for (int t = 0; t < TT; ++t) {
              accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
              tsum[t] = __builtin_fmaf(ks, vrow[r][t], tsum[t]);
            }
          }
#pragma unroll
          for (int t = 0; t < TT; ++t) accT[t] = wave_rotate1(tsum[t]);
        }
      } else {
#pragma unroll 2
        for (int s = 0; s < 64; ++s) {
          const int idx = sub * 64 + ((lane + s) & 63);
          float v[TT];
          lds_load_vec<TT>(sV, idx, v);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float ks = fact_pair_sum<JT>(ap[r], ea[r], sB + idx * STR);
#pragma unroll
            for (int t = 0; t < TT; ++t) accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < TT; ++t) sT[(wave * SC + sub * 64 + lane) * TT + t] = accT[t];
    }
    __syncthreads();
    {
      const int col = c0 + tid;
      if (tid < SC && col < c_end && col >= r0 + BR) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          if (t < tcnt) {
            float sum = sT[(0 * SC + tid) * TT + t] + sT[(1 * SC + tid) * TT + t] +
                        sT[(2 * SC + tid) * TT + t] + sT[(3 * SC + tid) * TT + t];
            float *dst = slabT + ((size_t)(rb - rb_first) * N + col) * ldv + t0 + t;
            *dst = accumulate ? *dst + sum : sum;
          }
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    if (row < N) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (t < tcnt) {
          float *dst = slabR + ((size_t)kchunk * slab_rows + (row - slab_row0)) * ldv + t0 + t;
          *dst = accumulate ? *dst + accR[r][t] : accR[r][t];
        }
      }
    }
  }
}

// out[row][t] = scale * (sum_k slabR[k][row][t] + sum_{rb < row/BR} slabT[rb][row][t]) + noise * V[row][t]
// A workgroup owns 32 consecutive outputs; its 8 half-waves split the slab entries (entry k goes to group k % 8, each
// read is a 128-byte contiguous segment) and the 8 group sums are added in a fixed order: deterministic, and short
// enough for the small problems (N < 10k) where a one-thread-per-output loop over ~150 slabs was latency-bound.
template <int kRedOutputs>
__global__ __launch_bounds__(256) void mvm_reduce_kernel(const float *__restrict__ slabR, const float *__restrict__ slabT,
                                  const float *__restrict__ V, float *__restrict__ out, int M, int N, int T,
                                  int BR, int chunk_cols, int sym, float scale, float noise,
                                  const int *__restrict__ guard, int rb0, int rb1, int slab_row0, int slab_rows,
                                  rpgp_internal::Taper taper = rpgp_internal::Taper{0x7fffffff, 0x7fffffff, 0x7fffffff}) {
  constexpr int kRedGroups = 256 / kRedOutputs;
  __shared__ double sacc[kRedGroups][kRedOutputs];   // float64: ~150 slab entries per output, free at this size
  const int o = threadIdx.x & (kRedOutputs - 1), g = threadIdx.x / kRedOutputs;
  const size_t gid = (size_t)blockIdx.x * kRedOutputs + o;
  const bool valid = gid < (size_t)M * T;
  double acc = 0.0;
  if (valid) {
    const int row = (int)(gid / T);
    const int rb = row / BR;
    const int cbase = sym ? rb * BR : 0;
    const int chunk_b = rpgp_internal::taper_chunk(rb, chunk_cols, taper.tb1, taper.tb2, taper.tb3);
    const int nk = (N - cbase + chunk_b - 1) / chunk_b;
    if (rb >= rb0 && rb < rb1) {                    // row products exist only for this call's row blocks
      const size_t lid = gid - (size_t)slab_row0 * T;
      for (int k = g; k < nk; k += kRedGroups) acc += (double)slabR[(size_t)k * slab_rows * T + lid];
    }
    if (sym) {
      const int bend = rb < rb1 ? rb : rb1;         // transposed products written by row blocks rb0 <= b < min(rb, rb1)
      int b = rb0 + g;                              // four entries in flight, added in the same order as the plain loop
      for (; b + 3 * kRedGroups < bend; b += 4 * kRedGroups) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = slabT[(size_t)(b + u * kRedGroups - rb0) * N * T + gid];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += (double)v[u];
      }
      for (; b < bend; b += kRedGroups) acc += (double)slabT[(size_t)(b - rb0) * N * T + gid];
    }
  }
  sacc[g][o] = acc;
  __syncthreads();
  if (g != 0 || !valid) return;
  if (guard && *guard == 0) {   // prepared (factorised) path used although rpgp_prepare flagged the range as unsafe
    out[gid] = __builtin_nanf("");
    return;
  }
  double tot = sacc[0][o];
#pragma unroll
  for (int q = 1; q < kRedGroups; ++q) tot += sacc[q][o];
  float r = (float)((double)scale * tot);
  if (noise != 0.f) r = __builtin_fmaf(noise, V[gid], r);
  out[gid] = r;
}

// Outputs per workgroup of the slab reduce: 32 (eight groups share the slab entries: the latency-bound small problems) up to
// 256 (one group, 1 KB contiguous per slab entry: the large ones, where 128-byte pieces 2 MB apart waste the HBM rate).
inline int red_outputs(size_t total) {
  // measured (tools/r5_symk_red_prof.sh, T = 11 packed-cache product): 64 outputs beat 32 at every size measured (N = 7k,
  // 81k outputs: 7.2 -> 6.5 us; 15k: 10.4 -> 9.4; 50k: 36.6 -> 29.6); 128 only from N ~ 15k (8.3 us) and lose at 7k (10.0 us);
  // below the measured range the round-2 width stays
  return total >= (size_t)65536 ? 64 : 32;
}
#define RPGP_LAUNCH_MVM_REDUCE(total_, st_, ...)                                                                          \
  do {                                                                                                                    \
    const size_t tot__ = (total_);                                                                                        \
    switch (red_outputs(tot__)) {                                                                                         \
      case 64: hipLaunchKernelGGL(mvm_reduce_kernel<64>, dim3((unsigned)((tot__ + 63) / 64)), dim3(256), 0, st_, __VA_ARGS__); break;    \
      default: hipLaunchKernelGGL(mvm_reduce_kernel<32>, dim3((unsigned)((tot__ + 31) / 32)), dim3(256), 0, st_, __VA_ARGS__); break;    \
    }                                                                                                                     \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Dense block: out[m][n] = scale * sum_j exp(-0.5 (Z1[m,j]-Z2[n,j])^2).  One thread per output column
// (coalesced stores), RT rows per workgroup held in LDS.
// ---------------------------------------------------------------------------------------------
template <int JT, class KF = KfBase>
__global__ __launch_bounds__(256) void dense_kernel(const float *__restrict__ Z1, const float *__restrict__ Z2,
                                                    float *__restrict__ out, int M, int N, int ldz1, int ldz2,
                                                    long long ldo, int j0, float scale, int accumulate,
                                                    const float *__restrict__ wts) {
  constexpr int RT = 16;
  __shared__ float sA[RT][JT];
  float wreg[KF::weighted ? JT / KF::group : 1];
  if constexpr (KF::weighted) {
#pragma unroll
    for (int c = 0; c < JT / KF::group; ++c) wreg[c] = wts[j0 / KF::group + c];
  } else {
    wreg[0] = 0.f;
  }
  const int tid = threadIdx.x;
  const int col = blockIdx.x * 256 + tid;
  const int m0 = blockIdx.y * RT;
  for (int e = tid; e < RT * JT; e += 256) {
    const int r = e / JT, j = e % JT;
    sA[r][j] = (m0 + r < M) ? Z1[(size_t)(m0 + r) * ldz1 + j0 + j] * KF::pre : 0.f;
  }
  __syncthreads();
  if (col >= N) return;
  float b[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) b[j] = Z2[(size_t)col * ldz2 + j0 + j] * KF::pre;
#pragma unroll 4
  for (int r = 0; r < RT; ++r) {
    if (m0 + r >= M) break;
    const float acc = KF::template pair_sum<JT>(sA[r], b, wreg);
    float *dst = out + (size_t)(m0 + r) * ldo + col;
    *dst = accumulate ? __builtin_fmaf(scale, acc, *dst) : scale * acc;
  }
}

// ---------------------------------------------------------------------------------------------
// Projection Z = X @ Peff and its backward dPeff = X^T @ G (thin GEMMs; plain VALU version).
// ---------------------------------------------------------------------------------------------
// Z = X @ Peff on the matrix cores: v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain, MI355X_MICROARCH.md "FP32-input
// MFMA").  One wave64 owns a 16-row stripe of Z and walks the column tiles; the K dimension (d) advances 4 per MFMA.
//   A (16x4): lane l holds X[row0 + l%16][k0 + l/16]        B (4x16): lane l holds Peff[k0 + l/16][col0 + l%16]
//   D (16x16): lane l holds Z[row0 + 4*(l/16) + r][col0 + l%16], r = 0..3
__global__ __launch_bounds__(256) void project_kernel(const float *__restrict__ X, const float *__restrict__ Peff,
                                                      float *__restrict__ Z, long long N, int d, int J) {
  extern __shared__ float sP[];  // d4 x J16 zero-padded copy of Peff (d4 = d rounded up to 4, J16 = J rounded up to 16)
  const int d4 = (d + 3) & ~3, J16 = (J + 15) & ~15;
  for (int e = threadIdx.x; e < d4 * J16; e += 256) {
    const int k = e / J16, j = e % J16;
    sP[e] = (k < d && j < J) ? Peff[k * J + j] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const long long stripes = (N + 15) / 16;
  for (long long sidx = (long long)blockIdx.x * 4 + wave; sidx < stripes; sidx += (long long)gridDim.x * 4) {
    const long long row = sidx * 16 + m;
    const bool rv = row < N;
    for (int col0 = 0; col0 < J16; col0 += 16) {
      floatx4m acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < d4; k0 += 4) {
        const int k = k0 + q;
        const float a = (rv && k < d) ? X[row * d + k] : 0.f;
        const float b = sP[k * J16 + col0 + m];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long orow = sidx * 16 + 4 * q + r;
        const int ocol = col0 + m;
        if (orow < N && ocol < J) Z[orow * J + ocol] = acc[r];
      }
    }
  }
}

// dPeff[k][j] = sum_n X[n][k] G[n][j]; one workgroup per (k, j-tile) would be overkill: d*J <= ~1024 outputs,
// each workgroup reduces a slice of n for all (k,j) handled by its threads, then atomics-free two-pass.
__global__ __launch_bounds__(256) void project_grad_partial_kernel(const float *__restrict__ X,
                                                                   const float *__restrict__ G,
                                                                   float *__restrict__ part, long long N, int d,
                                                                   int J, long long rows_per_block) {
  // thread e handles output element (k,j) = (e / J, e % J) for e < d*J (loop if d*J > 256)
  const long long n0 = (long long)blockIdx.x * rows_per_block;
  const long long n1 = (n0 + rows_per_block < N) ? n0 + rows_per_block : N;
  for (int e = threadIdx.x; e < d * J; e += 256) {
    const int k = e / J, j = e % J;
    float acc = 0.f;
    for (long long n = n0; n < n1; ++n) acc = __builtin_fmaf(X[n * d + k], G[n * J + j], acc);
    part[(size_t)blockIdx.x * d * J + e] = acc;
  }
}

__global__ void sum_partials_kernel(const float *__restrict__ part, float *__restrict__ out, int count, int nparts,
                                    float mul) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int p = 0; p < nparts; ++p) acc += part[(size_t)p * count + e];
  out[e] = acc * mul;
}

// ---------------------------------------------------------------------------------------------
// DPA-GP diversification (rp.space_equally, rp.py:241-266) as ONE single-workgroup launch:
// `niter` plain gradient steps of size lr on  L(P) = sum_{a != b} cos^4(angle(P_a, P_b)),  then row normalisation.
//   c_ab = P_a.P_b / (n_a n_b);   dL/dP_a = sum_{b != a} 8 c_ab^3 ( P_b / (n_a n_b) - c_ab P_a / n_a^2 )
// J x d <= 64 x 64 lives in LDS for the whole optimisation (5000 steps ~ 10 ms instead of seconds of autograd steps on
// the host, which dominated the wall time of a DPA-GP experiment on the GPU box).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void space_equally_kernel(float *__restrict__ P, int J, int d, float lr, int niter,
                                                            float *__restrict__ final_loss) {
  __shared__ float sA[64 * 65];
  __shared__ float sB[64 * 65];      // ping-pong copies of P
  __shared__ float sC[64 * 65];      // cos_ab (diagonal zeroed)
  __shared__ float sN[64];
  __shared__ float sred[256];
  const int tid = threadIdx.x;
  float *cur = sA, *nxt = sB;
  for (int e = tid; e < J * d; e += 256) cur[(e / d) * 65 + e % d] = P[e];
  __syncthreads();
  for (int it = 0; it <= niter; ++it) {
    if (tid < J) {
      float s2 = 0.f;
      for (int q = 0; q < d; ++q) s2 = __builtin_fmaf(cur[tid * 65 + q], cur[tid * 65 + q], s2);
      sN[tid] = sqrtf(s2);
    }
    __syncthreads();
    for (int e = tid; e < J * J; e += 256) {
      const int a = e / J, b = e % J;
      float dot = 0.f;
      for (int q = 0; q < d; ++q) dot = __builtin_fmaf(cur[a * 65 + q], cur[b * 65 + q], dot);
      sC[a * 65 + b] = a == b ? 0.f : dot / (sN[a] * sN[b]);
    }
    __syncthreads();
    if (it == niter) break;          // the last pass only refreshes norms and cosines for the loss / normalisation
    for (int e = tid; e < J * d; e += 256) {
      const int a = e / d, q = e % d;
      const float na = sN[a], pa = cur[a * 65 + q];
      float g = 0.f;
      for (int b = 0; b < J; ++b) {
        const float c = sC[a * 65 + b];
        const float c3 = c * c * c;
        g = __builtin_fmaf(8.0f * c3, cur[b * 65 + q] / (na * sN[b]) - c * pa / (na * na), g);
      }
      nxt[a * 65 + q] = pa - lr * g;
    }
    __syncthreads();
    float *tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  float part = 0.f;
  for (int e = tid; e < J * J; e += 256) {
    const float c = sC[(e / J) * 65 + e % J];
    part += c * c * c * c;
  }
  sred[tid] = part;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sred[tid] += sred[tid + w];
    __syncthreads();
  }
  if (tid == 0 && final_loss) final_loss[0] = sred[0];
  for (int e = tid; e < J * d; e += 256) P[e] = cur[(e / d) * 65 + e % d] / sN[e / d];
}

// ------------------------------- host-side helpers -------------------------------------------

// Optional measurement hook (bench.py): HIP-event pairs around the dominant (tile) kernel launches.
constexpr int kProfMax = 4096;
bool g_prof_on = false;
int g_prof_n = 0;
hipEvent_t g_prof_ev[2 * kProfMax];

template <int JT, int TT, bool SYM>
int launch_mvm_tile(const TilePlan &p, const float *Z1, const float *Z2, const float *V, float *slabR, float *slabT,
                    int M, int N, int ldz1, int ldz2, int ldv, int j0, int t0, int tcnt, int accumulate,
                    hipStream_t st) {
  dim3 grid(p.w1 - p.w0), block(256);
  if (p.R == 2)
    hipLaunchKernelGGL((mvm_tile_kernel<JT, TT, 2, SYM>), grid, block, 0, st, Z1, Z2, V, slabR, slabT, M, N, ldz1,
                       ldz2, ldv, j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows,
                       (const float *)nullptr);
  else
    hipLaunchKernelGGL((mvm_tile_kernel<JT, TT, 1, SYM>), grid, block, 0, st, Z1, Z2, V, slabR, slabT, M, N, ldz1,
                       ldz2, ldv, j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows,
                       (const float *)nullptr);
  return launch_status();
}

template <bool SYM>
int mvm_common(const float *Z1, const float *Z2, const float *V, float *out, int64_t M, int64_t N, int ldz1,
               int ldz2, int T, int j0, int j1, float scale, float noise, void *ws, size_t ws_bytes, void *stream,
               int world = 1, int rank = 0) {
  if (!Z1 || !Z2 || !V || !out || M <= 0 || N <= 0 || T <= 0 || j0 < 0 || j1 <= j0 || ldz1 < j1 || ldz2 < j1)
    return RPGP_EINVAL;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return RPGP_EINVAL;
  int rc = rpgp_init();
  if (rc) return rc;
  if (world < 1 || rank < 0 || rank >= world) return RPGP_EINVAL;
  const size_t need = mvm_workspace_floats(M, N, T, SYM, world, rank) * sizeof(float);
  if (!ws || ws_bytes < need) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const TilePlan p = make_plan(M, N, SYM, T, world, rank);
  float *slabR = reinterpret_cast<float *>(ws);
  float *slabT = slabR + (size_t)p.maxchunks * p.rows * T;
  if (p.partial && need) RPGP_CHECK(hipMemsetAsync(ws, 0, need, st));   // row blocks shared with a neighbour rank
  int first = 1;
  const bool prof = g_prof_on && g_prof_n < kProfMax;
  if (prof) RPGP_CHECK(hipEventRecord(g_prof_ev[2 * g_prof_n], st));
  for (int j = j0; j < j1 && p.w1 > p.w0;) {
    const int jt = next_j_piece(j1 - j);
    for (int t0 = 0; t0 < T;) {
      const int tt = next_t_piece(T - t0);
      const int tcnt = (T - t0 < tt) ? T - t0 : tt;
      rc = with_j_piece(jt, [&](auto jc) {
        return with_t_piece(tt, [&](auto tc) {
          return launch_mvm_tile<decltype(jc)::value, decltype(tc)::value, SYM>(p, Z1, Z2, V, slabR, slabT, (int)M, (int)N, ldz1,
                                                                              ldz2, T, j, t0, tcnt, first ? 0 : 1, st);
        });
      });
      if (rc) return rc;
      t0 += tcnt;
    }
    first = 0;
    j += jt;
  }
  if (prof) {
    RPGP_CHECK(hipEventRecord(g_prof_ev[2 * g_prof_n + 1], st));
    ++g_prof_n;
  }
  const size_t total = (size_t)M * T;
  RPGP_LAUNCH_MVM_REDUCE(total, st, slabR, slabT, V,
                     out, (int)M, (int)N, T, p.BR, p.chunk_cols, SYM ? 1 : 0, scale, noise, (const int *)nullptr, p.rb0,
                     p.rb1, p.row0, p.rows);
  return launch_status();
}

// Does the hand-scheduled kernel (rpgp_fact_asm.hip) serve this call?  The whole J = 20 operator, ONE right-hand side, two
// rows per lane, and the rotation direction its LDS image assumes; RPGP_FACT_ASM=0 keeps the compiler-scheduled kernel
// (read per launch: A/B pairs alternate inside one process).
inline bool fact_asm_enabled() {
  const char *env_asm = getenv("RPGP_FACT_ASM");
  return !(env_asm && atoi(env_asm) == 0);
}
inline bool fact_asm_applies(const TilePlan &p, int T, int J, int j0, int j1) {
  return fact_asm_enabled() && p.R == 2 && T == 1 && J == 20 && j0 == 0 && j1 == 20 && g_rotdir == 1;
}

// ---- prepared (factorised) path -----------------------------------------------------------------
template <int JT, int TT>
int launch_mvm_fact(const TilePlan &p, const float2v *rowdat, const float2v *coldat, const float *V, float *slabR,
                    float *slabT, int N, int J, int ldv, int j0, int t0, int tcnt, int accumulate, hipStream_t st) {
  dim3 grid(p.w1 - p.w0), block(256);
  if constexpr (TT == 1 && JT == 20) {
    if (tcnt == 1 && fact_asm_applies(p, 1, J, j0, j0 + 20))
      return rpgp_internal::launch_mvm_fact_asm(rowdat, coldat, V, slabR, slabT, N, ldv, t0, p.chunk_cols, p.taper, accumulate,
                                                p.w0, p.w1 - p.w0, p.rb0, p.row0, p.rows, st);
  }
  if constexpr (TT == 1 && JT >= 2 && JT <= 10) {
    // J-slices (the ranks of north_star's J-split; J = d models): the same generated loop with fewer quads per record
    if (tcnt == 1 && fact_asm_enabled() && p.R == 2 && g_rotdir == 1 && rpgp_internal::fact_asm_thin_supported(JT))
      return rpgp_internal::launch_mvm_fact_asm_thin(JT, rowdat, coldat, V, slabR, slabT, N, J, j0, ldv, t0, p.chunk_cols,
                                                     p.taper, accumulate, p.w0, p.w1 - p.w0, p.rb0, p.row0, p.rows, st);
  }
  if (p.R == 2)
    hipLaunchKernelGGL((mvm_fact_kernel<JT, TT, 2>), grid, block, 0, st, rowdat, coldat, V, slabR, slabT, N, J, ldv,
                       j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows);
  else
    hipLaunchKernelGGL((mvm_fact_kernel<JT, TT, 1>), grid, block, 0, st, rowdat, coldat, V, slabR, slabT, N, J, ldv,
                       j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows);
  return launch_status();
}

template <int JT>
int launch_dense(const float *Z1, const float *Z2, float *out, int M, int N, int ldz1, int ldz2, long long ldo,
                 int j0, float scale, int accumulate, hipStream_t st) {
  dim3 grid((N + 255) / 256, (M + 15) / 16);
  hipLaunchKernelGGL((dense_kernel<JT>), grid, dim3(256), 0, st, Z1, Z2, out, M, N, ldz1, ldz2, ldo, j0, scale,
                     accumulate, (const float *)nullptr);
  return launch_status();
}

template <class KF, int JT, bool SYM>
int launch_family_tile(int tt, const TilePlan &p, const float *Z1, const float *Z2, const float *V, float *slabR,
                       float *slabT, int M, int N, int ldz1, int ldz2, int ldv, int j0, int t0, int tcnt,
                       int accumulate, const float *wts, hipStream_t st) {
  dim3 grid(p.w1 - p.w0), block(256);
  switch (tt) {
    case 1:
      hipLaunchKernelGGL((mvm_tile_kernel<JT, 1, 1, SYM, KF>), grid, block, 0, st, Z1, Z2, V, slabR, slabT, M, N, ldz1,
                         ldz2, ldv, j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows, wts);
      break;
    case 4:
      hipLaunchKernelGGL((mvm_tile_kernel<JT, 4, 1, SYM, KF>), grid, block, 0, st, Z1, Z2, V, slabR, slabT, M, N, ldz1,
                         ldz2, ldv, j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows, wts);
      break;
    default:
      hipLaunchKernelGGL((mvm_tile_kernel<JT, 12, 1, SYM, KF>), grid, block, 0, st, Z1, Z2, V, slabR, slabT, M, N, ldz1,
                         ldz2, ldv, j0, t0, tcnt, p.chunk_cols, g_rotdir, accumulate, p.w0, p.rb0, p.row0, p.rows, wts);
      break;
  }
  return launch_status();
}

template <bool SYM>
int family_mvm_common(const rpgp_family *fam, const float *Z1, const float *Z2, const float *V, float *out, int64_t M,
                      int64_t N, int ldz1, int ldz2, int T, float scale, float noise, void *ws, size_t ws_bytes,
                      void *stream) {
  if (!Z1 || !Z2 || !V || !out || M <= 0 || N <= 0 || T <= 0) return RPGP_EINVAL;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return RPGP_EINVAL;
  int rc = family_check(fam, ldz1, ldz2);
  if (rc) return rc;
  rc = rpgp_init();
  if (rc) return rc;
  const size_t need = mvm_workspace_floats(M, N, T, SYM, 1, 0, true) * sizeof(float);
  if (!ws || ws_bytes < need) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const TilePlan p = make_plan(M, N, SYM, T, 1, 0, true);
  float *slabR = reinterpret_cast<float *>(ws);
  float *slabT = slabR + (size_t)p.maxchunks * p.rows * T;
  const int J = fam->ncomp * fam->group;
  const float *wts = fam->weights;
  rc = with_family_policy(fam->kind, fam->group, [&](auto kf) -> int {
    using KF = decltype(kf);
    int first = 1;
    for (int j = 0; j < J;) {
      const int jt = family_piece<KF>(J - j);
      for (int t0 = 0; t0 < T;) {
        const int tt = next_t_piece(T - t0);
        const int tcnt = (T - t0 < tt) ? T - t0 : tt;
        const int r2 = with_family_piece<KF>(jt, [&](auto jc) -> int {
          return launch_family_tile<KF, decltype(jc)::value, SYM>(tt, p, Z1, Z2, V, slabR, slabT, (int)M, (int)N, ldz1,
                                                                  ldz2, T, j, t0, tcnt, first ? 0 : 1, wts, st);
        });
        if (r2) return r2;
        t0 += tcnt;
      }
      first = 0;
      j += jt;
    }
    return 0;
  });
  if (rc) return rc;
  const size_t total = (size_t)M * T;
  RPGP_LAUNCH_MVM_REDUCE(total, st, slabR, slabT, V, out, (int)M, (int)N, T, p.BR, p.chunk_cols, SYM ? 1 : 0, scale, noise,
                     (const int *)nullptr, p.rb0, p.rb1, p.row0, p.rows);
  return launch_status();
}

}  // namespace

namespace rpgp_internal {
// the process state every translation unit shares (declared in rpgp_internal.h): this is its ONE definition
int g_num_cus = 256;       // compute units of the current device (set by rpgp_init)
int g_rotdir = 0;  // +1: wave_rotate1 delivers lane l+1's value to lane l; -1: lane l-1's.  0 = not probed.

// the slab reduce for the sweeps of other translation units (rpgp_symcache.hip): same arguments, same 32 / 64 choice
int mvm_reduce_launch(size_t total, hipStream_t st, const float *slabR, const float *slabT, const float *V, float *out, int M,
                      int N, int T, int BR, int chunk_cols, int sym, float scale, float noise, const int *guard, int rb0,
                      int rb1, int slab_row0, int slab_rows, Taper taper) {
  RPGP_LAUNCH_MVM_REDUCE(total, st, slabR, slabT, V, out, M, N, T, BR, chunk_cols, sym, scale, noise, guard, rb0, rb1,
                         slab_row0, slab_rows, taper);
  return launch_status();
}
// the rpgp_profile_* hook for products launched from other translation units (rpgp_lowrank.hip)
bool prof_open(hipStream_t st) {
  if (!g_prof_on || g_prof_n >= kProfMax) return false;
  return hipEventRecord(g_prof_ev[2 * g_prof_n], st) == hipSuccess;
}
int prof_close(hipStream_t st) {
  RPGP_CHECK(hipEventRecord(g_prof_ev[2 * g_prof_n + 1], st));
  ++g_prof_n;
  return 0;
}
}  // namespace rpgp_internal

// ------------------------------------ C ABI ---------------------------------------------------

extern "C" {

int rpgp_version(void) { return RPGP_ABI_VERSION; }

const char *rpgp_error_string(int code) {
  switch (code) {
    case 0: return "success";
    case RPGP_EINVAL: return "rpgp: invalid argument";
    case RPGP_EWORKSPACE: return "rpgp: workspace too small";
    case RPGP_ENODEVICE: return "rpgp: no usable gfx950 device";
    case RPGP_ENUMERIC: return "rpgp: NaNs encountered in an iterative solve";
    default: return hipGetErrorString((hipError_t)code);
  }
}

int rpgp_init(void) {
  if (g_rotdir != 0) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RPGP_ENODEVICE;
  {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
      g_num_cus = ncu;
  }
  int *d = nullptr;
  RPGP_CHECK(hipMalloc(&d, 64 * sizeof(int)));
  hipLaunchKernelGGL(probe_rotate_kernel, dim3(1), dim3(64), 0, 0, d);
  int h[64];
  hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return (int)e;
  if (h[0] == 1 && h[63] == 0) g_rotdir = 1;
  else if (h[0] == 63 && h[1] == 0) g_rotdir = -1;
  else return RPGP_ENODEVICE;
  return 0;
}

int rpgp_prepared_kernel_id(int64_t N, int J, int T) {
  if (N <= 0 || J <= 0 || T <= 0) return -RPGP_EINVAL;
  if (rpgp_init()) return -RPGP_EINVAL;
  const TilePlan p = make_plan(N, N, true, T);
  if (fact_asm_applies(p, T, J, 0, J)) return 1;
  // a sweep over J projections that is one compiled piece (a rank's J-slice, or a model with that many projections)
  if (T == 1 && fact_asm_enabled() && p.R == 2 && g_rotdir == 1 && rpgp_internal::fact_asm_thin_supported(J)) return 2;
  return 0;
}

int rpgp_profile_begin(void) {
  if (!g_prof_on) {
    for (int i = 0; i < 2 * kProfMax; ++i)
      if (!g_prof_ev[i]) RPGP_CHECK(hipEventCreate(&g_prof_ev[i]));
  }
  g_prof_on = true;
  g_prof_n = 0;
  return 0;
}

int rpgp_profile_end(float *avg_ms_host, int *count_host) {
  g_prof_on = false;
  double sum = 0.0;
  for (int i = 0; i < g_prof_n; ++i) {
    RPGP_CHECK(hipEventSynchronize(g_prof_ev[2 * i + 1]));
    float ms = 0.f;
    RPGP_CHECK(hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]));
    sum += ms;
  }
  if (avg_ms_host) *avg_ms_host = g_prof_n ? (float)(sum / g_prof_n) : 0.f;
  if (count_host) *count_host = g_prof_n;
  g_prof_n = 0;
  return 0;
}

int rpgp_space_equally(float *P, int J, int d, float lr, int niter, float *final_loss, void *stream) {
  if (!P || J <= 0 || d <= 0 || J > 64 || d > 64 || niter < 0) return RPGP_EINVAL;
  hipLaunchKernelGGL(space_equally_kernel, dim3(1), dim3(256), 0, as_stream(stream), P, J, d, lr, niter, final_loss);
  return launch_status();
}

int rpgp_project(const float *X, const float *Peff, float *Z, int64_t N, int d, int J, void *stream) {
  if (!X || !Peff || !Z || N <= 0 || d <= 0 || J <= 0 || (size_t)(d + 3) * (J + 15) * 4 > 64 * 1024) return RPGP_EINVAL;
  const long long stripes = (N + 15) / 16;
  int blocks = (int)((stripes + 3) / 4 < 4096 ? (stripes + 3) / 4 : 4096);
  const size_t lds = (size_t)((d + 3) & ~3) * ((J + 15) & ~15) * sizeof(float);
  hipLaunchKernelGGL(project_kernel, dim3(blocks), dim3(256), lds, as_stream(stream), X, Peff, Z, (long long)N, d, J);
  return launch_status();
}

int rpgp_project_grad(const float *X, const float *G, float *dPeff, int64_t N, int d, int J, void *stream) {
  if (!X || !G || !dPeff || N <= 0 || d <= 0 || J <= 0) return RPGP_EINVAL;
  // two-pass deterministic reduction; partials live in a small static-size device buffer per call
  // (allocated by the caller-visible workspace would be cleaner, but d*J*nblk is tiny) -> use hipMallocAsync.
  hipStream_t st = as_stream(stream);
  if (d <= 64 && J <= 64) {
    // thin X^T G on the matrix cores with float64 accumulation (rpgp_precond.hip; the slab kernel below walked 512 rows
    // serially per thread on N / 512 workgroups: 88 us at N = 7372, d = 8, J = 20)
    double *gpart = nullptr;
    RPGP_CHECK(hipMallocAsync((void **)&gpart, rpgp_internal::gram_part_bytes(d, J), st));
    const int grc = rpgp_internal::gram_launch(X, d, G, J, (long long)N, d, J, nullptr, dPeff, gpart, st);
    (void)hipFreeAsync(gpart, st);
    return grc;
  }
  const int nblk = (int)((N + 511) / 512 < 1024 ? (N + 511) / 512 : 1024);
  const long long rows_per_block = (N + nblk - 1) / nblk;
  float *part = nullptr;
  RPGP_CHECK(hipMallocAsync((void **)&part, (size_t)nblk * d * J * sizeof(float), st));
  hipLaunchKernelGGL(project_grad_partial_kernel, dim3(nblk), dim3(256), 0, st, X, G, part, (long long)N, d, J,
                     rows_per_block);
  hipLaunchKernelGGL(sum_partials_kernel, dim3((d * J + 255) / 256), dim3(256), 0, st, part, dPeff, d * J, nblk, 1.0f);
  int rc = launch_status();
  (void)hipFreeAsync(part, st);
  return rc;
}

size_t rpgp_mvm_sym_workspace_bytes(int64_t N, int T) {
  if (N <= 0 || T <= 0) return 0;
  return mvm_workspace_floats(N, N, T, true) * sizeof(float);
}

int rpgp_mvm_sym(const float *Z, const float *V, float *out, int64_t N, int ldz, int T, int j0, int j1, float scale,
                 float noise, void *workspace, size_t workspace_bytes, void *stream) {
  return mvm_common<true>(Z, Z, V, out, N, N, ldz, ldz, T, j0, j1, scale, noise, workspace, workspace_bytes, stream);
}

// workgroups of the range pass: 256 rows each (a thread walks ~256 J / 256 coordinates; the round-5 form gave a thread of
// its 25 workgroups 2 000 serial rows and took 60 us at C4 — VERDICT r5 #6a), at most 1 024 partial records
inline int prep_minmax_blocks(int64_t N) { return (int)((N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024); }

size_t rpgp_prepare_bytes(int64_t N, int J) {
  if (N <= 0 || J <= 0 || J > kPrepMidFloats) return 0;
  // header + mid + rowdat + coldat + min/max partials (tail)
  const size_t nblk = (size_t)prep_minmax_blocks(N);
  return (kPrepHeaderFloats + kPrepMidFloats) * sizeof(float) + 2 * (size_t)N * J * sizeof(float2v) +
         nblk * J * 2 * sizeof(float);
}

int rpgp_prepare(const float *Z, int64_t N, int ldz, int J, void *prep, size_t prep_bytes, void *stream) {
  if (!Z || !prep || N <= 0 || J <= 0 || J > kPrepMidFloats || ldz < J) return RPGP_EINVAL;
  if (prep_bytes < rpgp_prepare_bytes(N, J)) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  PrepLayout L = prep_layout(prep, N, J);
  float *part = reinterpret_cast<float *>(L.coldat + (size_t)N * J);
  const int nblk = prep_minmax_blocks(N);
  const long long rows_per_block = (N + nblk - 1) / nblk;
  hipLaunchKernelGGL(prep_minmax_kernel, dim3(nblk), dim3(256), 0, st, Z, part, (long long)N, ldz, J, rows_per_block);
  hipLaunchKernelGGL(prep_finish_kernel, dim3(1), dim3(256), 0, st, part, nblk, J, L.header, L.mid);
  const long long total = N * J;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(prep_build_kernel, dim3(blocks), dim3(256), 0, st, Z, L.mid, L.rowdat, L.coldat, (long long)N, ldz, J);
  return launch_status();
}

int rpgp_prepare_status(const void *prep, int *fast_ok_host, float *max_abs_host, void *stream) {
  if (!prep) return RPGP_EINVAL;
  float h[2];
  hipStream_t st = as_stream(stream);
  RPGP_CHECK(hipMemcpyAsync(h, prep, sizeof(h), hipMemcpyDeviceToHost, st));
  RPGP_CHECK(hipStreamSynchronize(st));
  if (fast_ok_host) *fast_ok_host = *reinterpret_cast<int *>(&h[0]);
  if (max_abs_host) *max_abs_host = h[1];
  return 0;
}

int rpgp_mvm_sym_prepared(const void *prep, const float *V, float *out, int64_t N, int J, int T, int j0, int j1,
                          float scale, float noise, void *workspace, size_t workspace_bytes, void *stream) {
  return rpgp_mvm_sym_prepared_range(prep, V, out, N, J, T, j0, j1, 1, 0, scale, noise, workspace, workspace_bytes,
                                     stream);
}

size_t rpgp_mvm_sym_range_workspace_bytes(int64_t N, int T, int world, int rank) {
  if (N <= 0 || T <= 0 || world < 1 || rank < 0 || rank >= world) return 0;
  return mvm_workspace_floats(N, N, T, true, world, rank) * sizeof(float);
}

int rpgp_mvm_sym_range(const float *Z, const float *V, float *out, int64_t N, int ldz, int T, int j0, int j1, int world,
                       int rank, float scale, float noise, void *workspace, size_t workspace_bytes, void *stream) {
  return mvm_common<true>(Z, Z, V, out, N, N, ldz, ldz, T, j0, j1, scale, noise, workspace, workspace_bytes, stream,
                          world, rank);
}

int rpgp_mvm_sym_prepared_range(const void *prep, const float *V, float *out, int64_t N, int J, int T, int j0, int j1,
                                int world, int rank, float scale, float noise, void *workspace, size_t workspace_bytes,
                                void *stream) {
  if (!prep || !V || !out || N <= 0 || T <= 0 || J <= 0 || J > kPrepMidFloats || j0 < 0 || j1 <= j0 || j1 > J)
    return RPGP_EINVAL;
  if (N > 0x7fffffffLL) return RPGP_EINVAL;
  int rc = rpgp_init();
  if (rc) return rc;
  if (world < 1 || rank < 0 || rank >= world) return RPGP_EINVAL;
  const size_t need = mvm_workspace_floats(N, N, T, true, world, rank) * sizeof(float);
  if (!workspace || workspace_bytes < need) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  TilePlan p = make_plan(N, N, true, T, world, rank);
  // the hand-scheduled kernel (rpgp_fact_asm.hip) understands tapered chunks: smaller workgroups at the end of the sweep
  if (fact_asm_applies(p, T, J, j0, j1)) p = make_plan(N, N, true, T, world, rank, false, 0, 4608.0, true);
  PrepLayout L = prep_layout(const_cast<void *>(prep), N, J);
  float *slabR = reinterpret_cast<float *>(workspace);
  float *slabT = slabR + (size_t)p.maxchunks * p.rows * T;
  if (p.partial && need) RPGP_CHECK(hipMemsetAsync(workspace, 0, need, st));
  int first = 1;
  const bool prof = g_prof_on && g_prof_n < kProfMax;
  if (prof) RPGP_CHECK(hipEventRecord(g_prof_ev[2 * g_prof_n], st));
  for (int j = j0; j < j1 && p.w1 > p.w0;) {
    const int jt = next_j_piece(j1 - j);
    for (int t0 = 0; t0 < T;) {
      const int tt = next_t_piece(T - t0);
      const int tcnt = (T - t0 < tt) ? T - t0 : tt;
      rc = with_j_piece(jt, [&](auto jc) {
        return with_t_piece(tt, [&](auto tc) {
          return launch_mvm_fact<decltype(jc)::value, decltype(tc)::value>(p, L.rowdat, L.coldat, V, slabR, slabT, (int)N, J, T, j,
                                                                         t0, tcnt, first ? 0 : 1, st);
        });
      });
      if (rc) return rc;
      t0 += tcnt;
    }
    first = 0;
    j += jt;
  }
  if (prof) {
    RPGP_CHECK(hipEventRecord(g_prof_ev[2 * g_prof_n + 1], st));
    ++g_prof_n;
  }
  const size_t total = (size_t)N * T;
  RPGP_LAUNCH_MVM_REDUCE(total, st, slabR, slabT, V, out,
                     (int)N, (int)N, T, p.BR, p.chunk_cols, 1, scale, noise,
                     reinterpret_cast<const int *>(L.header), p.rb0, p.rb1, p.row0, p.rows, p.taper);
  return launch_status();
}

size_t rpgp_mvm_rect_workspace_bytes(int64_t M, int64_t N, int T) {
  if (M <= 0 || N <= 0 || T <= 0) return 0;
  return mvm_workspace_floats(M, N, T, false) * sizeof(float);
}

int rpgp_mvm_rect(const float *Z1, const float *Z2, const float *V, float *out, int64_t M, int64_t N, int ldz1,
                  int ldz2, int T, int j0, int j1, float scale, void *workspace, size_t workspace_bytes,
                  void *stream) {
  return mvm_common<false>(Z1, Z2, V, out, M, N, ldz1, ldz2, T, j0, j1, scale, 0.f, workspace, workspace_bytes,
                           stream);
}

int rpgp_dense(const float *Z1, const float *Z2, float *out, int64_t M, int64_t N, int ldz1, int ldz2, int64_t ldo,
               int j0, int j1, float scale, void *stream) {
  if (!Z1 || !Z2 || !out || M <= 0 || N <= 0 || j0 < 0 || j1 <= j0 || ldz1 < j1 || ldz2 < j1 || ldo < N)
    return RPGP_EINVAL;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return RPGP_EINVAL;
  hipStream_t st = as_stream(stream);
  int first = 1;
  for (int j = j0; j < j1;) {
    const int jt = next_j_piece(j1 - j);
    int rc;
    switch (jt) {
      case 20: rc = launch_dense<20>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 10: rc = launch_dense<10>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 8: rc = launch_dense<8>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 5: rc = launch_dense<5>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 3: rc = launch_dense<3>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 4: rc = launch_dense<4>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      case 2: rc = launch_dense<2>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
      default: rc = launch_dense<1>(Z1, Z2, out, (int)M, (int)N, ldz1, ldz2, ldo, j, scale, !first, st); break;
    }
    if (rc) return rc;
    first = 0;
    j += jt;
  }
  return 0;
}

// ---- generalised family: C-ABI -------------------------------------------------------------------
size_t rpgp_family_mvm_workspace_bytes(int64_t M, int64_t N, int T, int sym) {
  if (M <= 0 || N <= 0 || T <= 0) return 0;
  return mvm_workspace_floats(M, N, T, sym != 0, 1, 0, true) * sizeof(float);
}

int rpgp_family_mvm_sym(const rpgp_family *fam, const float *Z, const float *V, float *out, int64_t N, int ldz, int T,
                        float scale, float noise, void *workspace, size_t workspace_bytes, void *stream) {
  return family_mvm_common<true>(fam, Z, Z, V, out, N, N, ldz, ldz, T, scale, noise, workspace, workspace_bytes,
                                 stream);
}

int rpgp_family_mvm_rect(const rpgp_family *fam, const float *Z1, const float *Z2, const float *V, float *out,
                         int64_t M, int64_t N, int ldz1, int ldz2, int T, float scale, void *workspace,
                         size_t workspace_bytes, void *stream) {
  return family_mvm_common<false>(fam, Z1, Z2, V, out, M, N, ldz1, ldz2, T, scale, 0.f, workspace, workspace_bytes,
                                  stream);
}

int rpgp_family_dense(const rpgp_family *fam, const float *Z1, const float *Z2, float *out, int64_t M, int64_t N,
                      int ldz1, int ldz2, int64_t ldo, float scale, void *stream) {
  if (!Z1 || !Z2 || !out || M <= 0 || N <= 0 || ldo < N || M > 0x7fffffffLL || N > 0x7fffffffLL) return RPGP_EINVAL;
  int rc = family_check(fam, ldz1, ldz2);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int J = fam->ncomp * fam->group;
  const float *wts = fam->weights;
  return with_family_policy(fam->kind, fam->group, [&](auto kf) -> int {
    using KF = decltype(kf);
    int first = 1;
    for (int j = 0; j < J;) {
      const int jt = family_piece<KF>(J - j);
      const int r2 = with_family_piece<KF>(jt, [&](auto jc) -> int {
        constexpr int JT = decltype(jc)::value;
        dim3 grid((unsigned)((N + 255) / 256), (unsigned)((M + 15) / 16));
        hipLaunchKernelGGL((dense_kernel<JT, KF>), grid, dim3(256), 0, st, Z1, Z2, out, (int)M, (int)N, ldz1, ldz2,
                           (long long)ldo, j, scale, first ? 0 : 1, wts);
        return launch_status();
      });
      if (r2) return r2;
      first = 0;
      j += jt;
    }
    return 0;
  });
}

}  // extern "C"
