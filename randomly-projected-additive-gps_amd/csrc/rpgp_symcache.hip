// rpgp_symcache.hip — the packed symmetric cache: the fused symmetric sweep's kernel values stored once, in the order the
// sweep consumes them (thin layout: rotating accumulators on the VALU; wide layout: 16 x 16 tiles for the matrix cores), its
// build and product kernels, their plans and the rpgp_symcache_* entries of the C-ABI.  The slab reduce of the product is
// mvm_reduce_kernel of rpgp_kernels.hip (rpgp_internal::mvm_reduce_launch).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stddef.h>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"
#include "rpgp_tile.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Packed symmetric cache ("symcache"): the cached-K mode without the lower triangle.
//   The fused symmetric sweep evaluates every unordered pair once and uses the value twice (row product and, through
//   the rotating accumulators, the transposed product).  The cache stores exactly the values that sweep consumes, in
//   the order it consumes them, so that the cached product is the same sweep with a 16-byte load in place of the J
//   exponentials: HALF the bytes of the N x N matrix per product (and half the HBM footprint).
//   Unit of storage: one 64-column subtile of one row block = BR x 64 floats, laid out
//       [wave 0..3][s4 0..15][r 0..R-1][lane 0..63][u 0..3]      (float4 per lane: rotation steps s = 4 s4 + u)
//   value (wave, s4, r, lane, u) = sum_j exp2(-(a - b)^2) for row r0 + wave*64R + r*64 + lane and column
//   csub + ((lane + rotdir*s) & 63).  Subtiles are numbered row block by row block, left to right from the diagonal
//   block's first column (subtile g of row block rb: columns rb*BR + 64 g ...), so the layout depends on (N, R) only.
//   A wave's loads are 1 KB contiguous; it streams 16 R KB per subtile.  Pairs outside the matrix hold 0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ long long symk_first_subtile(int rb, int N, int BR) {
  const long long nsN = (N + 63) / 64, q = BR / 64;
  return (long long)rb * nsN - q * ((long long)rb * (rb - 1) / 2);
}

// JT scaled coordinates of point `n` (clamped to a valid row), or `pad` in every slot when !ok — ALWAYS loaded: a load under a
// condition (or a select next to it) compiles to a branch with its own s_waitcnt vmcnt(0), one serial round trip per element.
// The masking is arithmetic (z * m + padv) so that the optimiser cannot turn it back into a branch.
template <int JT>
__device__ __forceinline__ void load_coords_masked(const float *__restrict__ Z, int n, int N, int ldz, int j0, bool ok,
                                                   float pad, float (&out)[JT]) {
  const int nc = (ok && n < N) ? n : N - 1;
  const float m = ok ? kExp2Scale : 0.f, padv = ok ? 0.f : pad;
  float z[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) z[j] = Z[(size_t)nc * ldz + j0 + j];
#pragma unroll
  for (int j = 0; j < JT; ++j) out[j] = __builtin_fmaf(z[j], m, padv);
}

template <int JT, int R>
__global__ __launch_bounds__(256) void symk_build_kernel(const float *__restrict__ Z, float4v *__restrict__ cache, int N,
                                                         int ldz, int j0, int chunk_cols, int rotdir, int accumulate,
                                                         int w0, long long sub0) {
  constexpr int BR = 256 * R;
  constexpr int STR = ColStride<JT>::v;
  __shared__ __attribute__((aligned(16))) float sB[64 * STR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, N, BR, chunk_cols, true, rb, kchunk);
  const int r0 = rb * BR;
  const long long cb = (long long)r0 + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;
  // rows / columns outside the matrix sit at +3e18 / +1e18: every pair with one of them is exp2(-huge) = 0
  float a[R][JT];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    load_coords_masked<JT>(Z, row, N, ldz, j0, row < N, 3.0e18f, a[r]);
  }
  const long long g0 = symk_first_subtile(rb, N, BR) + (long long)kchunk * (chunk_cols / 64) - sub0;
  int sub = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += 64, ++sub) {
    __syncthreads();
    if (tid < 64) {
      const int col = c0 + tid;
      float bc[JT];
      load_coords_masked<JT>(Z, col, N, ldz, j0, col < c_end, 1.0e18f, bc);
#pragma unroll
      for (int j = 0; j < JT; ++j) sB[tid * STR + j] = bc[j];
    }
    __syncthreads();
    float4v *dst = cache + ((size_t)((g0 + sub) * 4 + wave) * 16) * R * 64 + lane;
    for (int s4 = 0; s4 < 16; ++s4) {
      float4v kq[R];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = (lane + rotdir * (4 * s4 + u)) & 63;
        float b[JT];
        lds_load_cols<JT>(sB, idx, b);
#pragma unroll
        for (int r = 0; r < R; ++r) kq[r][u] = pair_kernel_sum<JT>(a[r], b);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float4v *q = dst + (size_t)(s4 * R + r) * 64;
        if (accumulate) {
          const float4v old = *q;
          kq[r] += old;
        }
        *q = kq[r];
      }
    }
  }
}

// Cached symmetric product: the loop nest of mvm_fact_kernel with the kernel value taken from the cache.  The wave's
// stream is requested D steps (of 4 rotation steps x R rows = R KB) ahead through a register ring, across subtile and
// LDS-stage boundaries.
// Loads of the packed cache: nontemporal for a cache that is streamed once per product; DEFAULT policy for one that fits the
// 256 MB Infinity Cache, where the products of one solve re-read it back to back (symk_nt_loads below; measured
// tools/r5_symk_nt_ab.py, T = 11: 39 MB 24.6 -> 21.9 us, 118 MB 37.7 -> 35.4, 234 MB 59.9 -> 52.4, thin T = 1 46.1 -> 41.4; the other
// way from ~300 MB: 464 MB 106 -> 113 us, 5 GB 947 -> 1039).
template <bool NT>
__device__ __forceinline__ float4v symk_tile_load(const float4v *p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

template <int TT, int R, bool NTL = true>
__global__ __launch_bounds__(256) void symk_mvm_kernel(const float4v *__restrict__ cache, const float *__restrict__ V,
                                                       float *__restrict__ slabR, float *__restrict__ slabT, int N, int ldv,
                                                       int t0, int tcnt, int chunk_cols, int rotdir, int accumulate, int w0,
                                                       int rb_first, int slab_row0, int slab_rows, long long sub0) {
  constexpr int BR = 256 * R;
  constexpr int SC = StageCols<TT>::v;
  constexpr int D = (TT > 4) ? 8 : 4;               // ring depth (steps): the wide blocks run 2 waves per SIMD and need the distance
  __shared__ __attribute__((aligned(16))) float sV[SC * TT];
  __shared__ __attribute__((aligned(16))) float sT[4 * SC * TT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, N, BR, chunk_cols, true, rb, kchunk);
  const int r0 = rb * BR;
  const long long cb = (long long)r0 + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;

  float vrow[R][TT], accR[R][TT];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      vrow[r][t] = (row < N && t < tcnt) ? V[(size_t)row * ldv + t0 + t] : 0.f;
      accR[r][t] = 0.f;
    }
  }
  const long long g0 = symk_first_subtile(rb, N, BR) + (long long)kchunk * (chunk_cols / 64) - sub0;
  const int total = ((c_end - c_begin + 63) / 64) * 16;                 // steps of this workgroup
  const float4v *wp = cache + ((size_t)(g0 * 4 + wave) * 16) * R * 64 + lane;
  // step n = 16 * subtile + s4  ->  wp + subtile * (4 waves * 16 * R * 64) + s4 * R * 64
  auto step_ptr = [&](int n) {
    n = n < total ? n : total - 1;                                      // tail: re-request the last step (no branch)
    return wp + (size_t)(n >> 4) * (size_t)(4 * 16 * R * 64) + (size_t)(n & 15) * (R * 64);
  };
  float4v ring[D][R];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float4v *q = step_ptr(d);
#pragma unroll
    for (int r = 0; r < R; ++r) ring[d][r] = symk_tile_load<NTL>(q + r * 64);
  }
  int n = 0;
  // the stage's right-hand sides are requested one stage ahead, from clamped addresses (a load under a condition compiles to
  // a branch with `s_waitcnt vmcnt(0)` behind it, which drains the ring at the head of every stage)
  float vpre[TT];
  auto v_request = [&](int c0n) {
    const int col = c0n + (tid < SC ? tid : 0);
    const int colc = col < N ? col : N - 1;
#pragma unroll
    for (int t = 0; t < TT; ++t) vpre[t] = V[(size_t)colc * ldv + t0 + (t < tcnt ? t : 0)];
  };
  v_request(c_begin);
  for (int c0 = c_begin; c0 < c_end; c0 += SC) {
    __syncthreads();
    if (tid < SC) {
#pragma unroll
      for (int t = 0; t < TT; ++t) sV[tid * TT + t] = (c0 + tid < c_end && t < tcnt) ? vpre[t] : 0.f;
    }
    v_request(c0 + SC < c_end ? c0 + SC : c0);
    __syncthreads();
    const int ncol = c_end - c0;
    const int nsub = ncol >= SC ? SC / 64 : (ncol + 63) / 64;
    for (int sub = 0; sub < nsub; ++sub) {
      const bool doT = (c0 + sub * 64 >= r0 + BR);
      float accT[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) accT[t] = 0.f;
#pragma nounroll
      for (int g = 0; g < 16 / D; ++g) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          float4v cur[R];
#pragma unroll
          for (int r = 0; r < R; ++r) cur[r] = ring[k][r];
          {
            const float4v *q = step_ptr(n + D);
#pragma unroll
            for (int r = 0; r < R; ++r) ring[k][r] = symk_tile_load<NTL>(q + r * 64);
          }
          ++n;
          if (doT) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int idx = sub * 64 + ((lane + rotdir * (4 * (g * D + k) + u)) & 63);
              float v[TT];
              lds_load_vec<TT>(sV, idx, v);
              if constexpr (TT % 2 == 0) {
                // both products on float2 so that hipcc emits v_pk_fma_f32 for the transposed sums as well (left to
                // the SLP vectoriser, the chains through the DPP rotation stayed scalar: 96 of 192 FMAs per step)
                float2v ts2[TT / 2];
#pragma unroll
                for (int q = 0; q < TT / 2; ++q) ts2[q] = float2v{accT[2 * q], accT[2 * q + 1]};
#pragma unroll
                for (int r = 0; r < R; ++r) {
                  const float2v ks2 = {cur[r][u], cur[r][u]};
#pragma unroll
                  for (int q = 0; q < TT / 2; ++q) {
                    const float2v a2 = __builtin_elementwise_fma(ks2, float2v{v[2 * q], v[2 * q + 1]},
                                                                 float2v{accR[r][2 * q], accR[r][2 * q + 1]});
                    accR[r][2 * q] = a2.x;
                    accR[r][2 * q + 1] = a2.y;
                    ts2[q] = __builtin_elementwise_fma(ks2, float2v{vrow[r][2 * q], vrow[r][2 * q + 1]}, ts2[q]);
                  }
                }
#pragma unroll
                for (int q = 0; q < TT / 2; ++q) {
                  accT[2 * q] = wave_rotate1(ts2[q].x);
                  accT[2 * q + 1] = wave_rotate1(ts2[q].y);
                }
              } else {
                float tsum[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) tsum[t] = accT[t];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                  const float ks = cur[r][u];
#pragma unroll
                  for (int t = 0; t < TT; ++t) {
                    accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
                    tsum[t] = __builtin_fmaf(ks, vrow[r][t], tsum[t]);
                  }
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) accT[t] = wave_rotate1(tsum[t]);
              }
            }
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int idx = sub * 64 + ((lane + rotdir * (4 * (g * D + k) + u)) & 63);
              float v[TT];
              lds_load_vec<TT>(sV, idx, v);
#pragma unroll
              for (int r = 0; r < R; ++r) {
                const float ks = cur[r][u];
#pragma unroll
                for (int t = 0; t < TT; ++t) accR[r][t] = __builtin_fmaf(ks, v[t], accR[r][t]);
              }
            }
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
            const float sum = sT[(0 * SC + tid) * TT + t] + sT[(1 * SC + tid) * TT + t] +
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

// ---- wide layout of the packed cache (blocks of 5..16 right-hand sides on the matrix cores) -----------------------------
// Same subtiles, same size; inside a wave's 16 R KB the values are stored as 16 x 16 tiles in the A/B operand order of
// v_mfma_f32_16x16x4_f32:  [wave][slot(rt 0..4R-1, ct 0..3)][lane]  float4 = K[row0 + 16 rt + (l % 16)][csub + 16 ct + 4 (l / 16) + i]
// (slots in the pair order the product consumes: (2m, p), (2m + 1, (p + 1) % 4), p = 0..3).
// One tile feeds two groups of four exact-fp32 MFMAs:
//   row product        D[t][rho]   += sum_i  A = V[csub + 16 ct + 4k + i][t]   x  B = tile_i             (contracts the columns)
//   transposed product D'[t][gam]  += sum_j  A = V[row0 + 16 rt + 4k + j][t]   x  B = L2_j               (contracts the rows)
// where L2_j[lane] = K[16 rt + 4 (l/16) + j][16 ct + l % 16] is the tile transposed through a per-wave LDS scratch (one
// 16-byte store, four 4-byte loads per lane, conflict-free at row stride 20; a wave's DS operations execute in order, so no
// barrier).  (First version: transposed in registers by four more MFMAs against identity slices — exact, but 12 instead
// of 8 matrix-pipe issues per tile: 1.14 ms against 1.00 ms for the T = 11 block at N = 50k.)
// The rotating accumulators of the thin layout cost T DPP moves per 64 pairs; here the transposed sums of a column tile
// stay in one accumulator across the wave's 4 R row tiles.
template <int JT, int R>
__global__ __launch_bounds__(256) void symk_build_tile_kernel(const float *__restrict__ Z, float4v *__restrict__ cache,
                                                              int N, int ldz, int j0, int chunk_cols, int accumulate,
                                                              int w0, long long sub0) {
  constexpr int BR = 256 * R;
  constexpr int STR = ColStride<JT>::v;
  __shared__ __attribute__((aligned(16))) float sB[64 * STR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rho = lane & 15, kap = lane >> 4;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, N, BR, chunk_cols, true, rb, kchunk);
  const int r0 = rb * BR;
  const long long cb = (long long)r0 + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;
  const long long g0 = symk_first_subtile(rb, N, BR) + (long long)kchunk * (chunk_cols / 64) - sub0;
  int sub = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += 64, ++sub) {
    __syncthreads();
    if (tid < 64) {
      const int col = c0 + tid;
      float bc[JT];
      load_coords_masked<JT>(Z, col, N, ldz, j0, col < c_end, 1.0e18f, bc);
#pragma unroll
      for (int j = 0; j < JT; ++j) sB[tid * STR + j] = bc[j];
    }
    __syncthreads();
    float4v *dst = cache + ((size_t)((g0 + sub) * 4 + wave) * 16) * R * 64 + lane;
#pragma nounroll
    for (int rt = 0; rt < 4 * R; ++rt) {
      const int row = r0 + wave * (64 * R) + 16 * rt + rho;
      float a[JT];
      load_coords_masked<JT>(Z, row, N, ldz, j0, row < N, 3.0e18f, a);
#pragma nounroll
      for (int ct = 0; ct < 4; ++ct) {
        float4v kq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float b[JT];
          lds_load_cols<JT>(sB, 16 * ct + 4 * kap + i, b);
          kq[i] = pair_kernel_sum<JT>(a, b);
        }
        // slot of tile (rt, ct) in the product's pair order: pairs A = (2 m, p), B = (2 m + 1, (p + 1) % 4)
        const int slot = (rt >> 1) * 8 + (((rt & 1) ? ((ct + 3) & 3) : ct) << 1) + (rt & 1);
        float4v *q = dst + (size_t)slot * 64;
        if (accumulate) {
          const float4v old = *q;
          kq += old;
        }
        *q = kq;
      }
    }
  }
}

// One pair of row tiles (2 RT2, 2 RT2 + 1) of a subtile, then the next pair (compile-time recursion: a `#pragma unroll`
// loop over the pairs was kept rolled by hipcc, which then rotated the accumulator arrays through registers with ~1000
// v_mov per subtile).
template <int R, bool DOT, int RT2, bool NT = true>
__device__ __forceinline__ void symk_tile_rows(const float4v *wp, float4v (&ring)[8], const float (&acol)[4][4],
                                               const float (&arow)[4 * R][4], float *scr, int woff, int roff,
                                               floatx4m (&accR)[4 * R], floatx4m (&accT)[4]) {
  constexpr int NRT = 4 * R, NTL = 4 * NRT, D = 8;
  constexpr size_t SUB = (size_t)4 * NTL * 64;
  if constexpr (RT2 < NRT / 2) {
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int rtA = 2 * RT2, ctA = pp, rtB = 2 * RT2 + 1, ctB = (pp + 1) & 3;
      const float4v kA = ring[2 * pp], kB = ring[2 * pp + 1];
      {
        const int m0 = RT2 * 8 + 2 * pp + D, m1 = m0 + 1;            // slots requested now (>= NT: next subtile)
        ring[2 * pp] = symk_tile_load<NT>(wp + (m0 < NTL ? (size_t)m0 * 64 : SUB + (size_t)(m0 - NTL) * 64));
        ring[2 * pp + 1] = symk_tile_load<NT>(wp + (m1 < NTL ? (size_t)m1 * 64 : SUB + (size_t)(m1 - NTL) * 64));
      }
      __builtin_amdgcn_sched_barrier(0);       // keep the requests D tiles ahead (hipcc sinks them to their first use)
      if constexpr (DOT) {
        // transpose of the two tiles through the wave's LDS scratch: row-major 16 x 20 (16-byte stores and the 4-byte
        // loads below are conflict-free at that stride); a wave's DS operations execute in order, so neither a barrier nor
        // a second buffer is needed; the eight row-product MFMAs cover the round trip
        *reinterpret_cast<float4v *>(scr + woff) = kA;
        *reinterpret_cast<float4v *>(scr + 320 + woff) = kB;
        floatx4m lA, lB;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lA[j] = scr[roff + 20 * j];
          lB[j] = scr[320 + roff + 20 * j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          accR[rtA] = __builtin_amdgcn_mfma_f32_16x16x4f32(acol[ctA][i], kA[i], accR[rtA], 0, 0, 0);
          accR[rtB] = __builtin_amdgcn_mfma_f32_16x16x4f32(acol[ctB][i], kB[i], accR[rtB], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          accT[ctA] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[rtA][j], lA[j], accT[ctA], 0, 0, 0);
          accT[ctB] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[rtB][j], lB[j], accT[ctB], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          accR[rtA] = __builtin_amdgcn_mfma_f32_16x16x4f32(acol[ctA][i], kA[i], accR[rtA], 0, 0, 0);
          accR[rtB] = __builtin_amdgcn_mfma_f32_16x16x4f32(acol[ctB][i], kB[i], accR[rtB], 0, 0, 0);
        }
      }
    }
    symk_tile_rows<R, DOT, RT2 + 1, NT>(wp, ring, acol, arow, scr, woff, roff, accR, accT);
  }
}

// The wide-layout product: ONE workgroup barrier per 64-column subtile (round 5; the three-barrier first form it replaced is
// tools/experiments/r6_removed_forms.patch).
//  * The staged right-hand sides and the four waves' transposed sums live in DOUBLE-BUFFERED LDS images.  Subtile s reads its
//    A operands from sV[s & 1], requests the block of subtile s + 1 at its head (four registers per thread) and writes it to
//    sV[(s + 1) & 1] at its end; the waves' transposed sums go to sT[s & 1]; ONE barrier; then the fixed-order cross-wave
//    sum and the slab store (bit-identical results to the three-barrier form).
//  * Why one barrier is enough: an image written in subtile s was last read in subtile s - 1 (sV) or s - 2 (sT), and every
//    reader of those passed the barrier of subtile s - 1 only after its reads — which the writer has passed too.
//  (A first form without any staging — every wave requesting its own sixteen A operands from global memory one subtile
//  ahead — needs 16 more registers than the 256 there are: the reloads put an `s_waitcnt vmcnt(0)` at the head of every
//  subtile, which drains the tile ring.)
template <int R, bool NTLOAD = true>
__global__ __launch_bounds__(256, 2) void symk_mvm_tile2_kernel(const float4v *__restrict__ cache, const float *__restrict__ V,
                                                             float *__restrict__ slabR, float *__restrict__ slabT, int N,
                                                             int ldv, int t0, int tcnt, int chunk_cols, int w0, int rb_first,
                                                             int slab_row0, int slab_rows, long long sub0) {
  constexpr int BR = 256 * R;
  constexpr int NRT = 4 * R;
  constexpr int NT = 4 * NRT;
  constexpr int D = 8;
  constexpr int SVS = 17;
  __shared__ __attribute__((aligned(16))) float sV[2][64 * SVS];
  __shared__ __attribute__((aligned(16))) float sT[2][4 * 64 * 16];
  __shared__ __attribute__((aligned(16))) float sX[4 * 640];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tn = lane & 15, kap = lane >> 4;
  int rb, kchunk;
  wg_to_tile(blockIdx.x + w0, N, BR, chunk_cols, true, rb, kchunk);
  const int r0 = rb * BR;
  const long long cb = (long long)r0 + (long long)kchunk * chunk_cols;
  if (cb >= N) return;
  const int c_begin = (int)cb;
  const int c_end = (c_begin + chunk_cols < N) ? c_begin + chunk_cols : N;
  const int rw0 = r0 + wave * (64 * R);

  float arow[NRT][4];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rw0 + 16 * rt + 4 * kap + j;
      arow[rt][j] = (row < N && tn < tcnt) ? V[(size_t)row * ldv + t0 + tn] : 0.f;
    }
  float *scr = sX + wave * 640;
  const int woff = tn * 20 + 4 * kap;
  const int roff = 4 * kap * 20 + tn;
  floatx4m accR[NRT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) accR[rt] = floatx4m{0.f, 0.f, 0.f, 0.f};

  const long long g0 = symk_first_subtile(rb, N, BR) + (long long)kchunk * (chunk_cols / 64) - sub0;
  const float4v *wp = cache + ((size_t)(g0 * 4 + wave) * 16) * R * 64 + lane;
  constexpr size_t SUB = (size_t)4 * NT * 64;
  float4v ring[D];
#pragma unroll
  for (int d = 0; d < D; ++d) ring[d] = symk_tile_load<NTLOAD>(wp + (size_t)d * 64);
  float vpre[4];
  auto v_request = [&](int c0n) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + 256 * it;
      const int c = e >> 4, t = e & 15;
      const int col = c0n + c;
      const int colc = col < N ? col : N - 1;
      const int tc = t < tcnt ? t : 0;
      vpre[it] = V[(size_t)colc * ldv + t0 + tc];
    }
  };
  auto v_stage = [&](float *dst, int c0n) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + 256 * it;
      const int c = e >> 4, t = e & 15;
      dst[c * SVS + t] = (c0n + c < c_end && t < tcnt) ? vpre[it] : 0.f;
    }
  };
  // contiguous slab stores: element e = c * tcnt + t of a subtile's block (when the block is one run: t0 == 0, tcnt == ldv)
  const bool dense_slab = (t0 == 0 && tcnt == ldv);
  int lidx[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = tid + 256 * it;
    const int c = e / tcnt, t = e - c * tcnt;
    lidx[it] = (e < 64 * tcnt) ? c * 16 + t : -1;
  }
  v_request(c_begin);
  v_stage(sV[0], c_begin);
  __syncthreads();
  int par = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += 64, wp += SUB, par ^= 1) {
    float acol[4][4];
    {
      const float *sv = sV[par];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) acol[ct][i] = sv[(16 * ct + 4 * kap + i) * SVS + tn];
    }
    // The next subtile's block is requested here and written to LDS at the END of this subtile: in straight-line code hipcc
    // counts the 16 R tile requests issued in between and waits with `vmcnt(8)` — the ring stays in flight.  (Consumed at the
    // head of the next iteration the wait becomes `vmcnt(3..0)`: across the back edge the counter model is conservative, and
    // that drains the ring once per subtile — the three-barrier form above does exactly that.)
    v_request(c0 + 64 < c_end ? c0 + 64 : c0);
    const bool doT = (c0 >= r0 + BR);
    floatx4m accT[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) accT[ct] = floatx4m{0.f, 0.f, 0.f, 0.f};
    float *st = sT[par];
    // ONE instruction stream for every subtile: the diagonal block's subtiles (no transposed product: the block is stored
    // whole) run the transposed MFMAs too and drop their sums — BR / N of the matrix work (1 % at N = 50k, 7 % at 7k) on a
    // pipe that is not the bound, against two copies of the tile code whose register maps hipcc reconciles with moves of the
    // whole ring (and an `s_waitcnt vmcnt(0)`) on the loop's back edge.
    symk_tile_rows<R, true, 0, NTLOAD>(wp, ring, acol, arow, scr, woff, roff, accR, accT);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[(wave * 64 + 16 * ct + tn) * 16 + 4 * kap + r] = accT[ct][r];
    v_stage(sV[par ^ 1], c0 + 64);                       // (past the chunk: zeros, never read)
    __syncthreads();
    if (doT) {
      if (dense_slab) {
        // the subtile's 64 x tcnt sums are one contiguous run of the slab: thread e writes element e (whole 256-byte
        // wave stores instead of 176-byte fragments with five idle lanes in sixteen)
        float *dstT = slabT + ((size_t)(rb - rb_first) * N + c0) * ldv;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int e = tid + 256 * it;
          const int li = lidx[it];
          if (li >= 0 && c0 + (li >> 4) < c_end) {
            const float sum = st[0 * 1024 + li] + st[1 * 1024 + li] + st[2 * 1024 + li] + st[3 * 1024 + li];
            dstT[e] = sum;
          }
        }
      } else {
      for (int e = tid; e < 64 * 16; e += 256) {
        const int c = e >> 4, t = e & 15;
        const int col = c0 + c;
        if (col < c_end && t < tcnt) {
          const float sum = st[(0 * 64 + c) * 16 + t] + st[(1 * 64 + c) * 16 + t] + st[(2 * 64 + c) * 16 + t] +
                            st[(3 * 64 + c) * 16 + t];
          slabT[((size_t)(rb - rb_first) * N + col) * ldv + t0 + t] = sum;
        }
      }
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    const int row = rw0 + 16 * rt + tn;
    if (row < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = 4 * kap + r;
        if (t < tcnt) slabR[((size_t)kchunk * slab_rows + (row - slab_row0)) * ldv + t0 + t] = accR[rt][r];
      }
    }
  }
}

// ---- packed symmetric cache: host side ------------------------------------------------------------------------------
struct SymkPlan {
  TilePlan p;
  long long sub0, sub1;        // subtile range [sub0, sub1) of this rank's workgroups
};
inline long long symk_host_first_subtile(int rb, int64_t N, int BR) {
  const long long nsN = (N + 63) / 64, q = BR / 64;
  return (long long)rb * nsN - q * ((long long)rb * (rb - 1) / 2);
}
// first subtile of workgroup `lin` of the plan's numbering (lin == total_wg: one past the last subtile)
inline long long symk_wg_subtile(const TilePlan &p, int64_t N, int lin) {
  long long acc = 0;
  for (int b = 0; b < p.nrb; ++b) {
    const int cb = chunks_of(p, N, true, b);
    if (lin < acc + cb) return symk_host_first_subtile(b, N, p.BR) + (lin - acc) * (long long)(p.chunk_cols / 64);
    acc += cb;
  }
  return symk_host_first_subtile(p.nrb, N, p.BR);
}
// One row-tile set per wave (R = 1: 256-row blocks) for a whole cache up to this size — squarer workgroup tiles and twice the
// workgroups to spread over the chip (tools/experiments/r5_symk_r1_sweep.py, profiles/r5b_symk_r1_sweep.jsonl: wide T = 11
// N = 4k 22.6 -> 20.5 us, 5.5k 25.6 -> 22.0, 7.4k 35.0 -> 32.2, 11k 56.8 -> 53.8, 15k 107.6 -> 100.6; thin T = 1 15k 86.1 -> 77.1).
// The LAYOUT of the cache follows R, so every entry point asks this one function.
constexpr int64_t kSymkR1Max = 16384;
inline bool symk_r1(int64_t N, int world) { return world <= 1 && N <= kSymkR1Max; }

// Smallest chunk (multiple of 64 columns) whose workgroups all fit ONE resident round of `slots`: with every workgroup
// running at once the product's time is the longest workgroup's, and a handful of workgroups beyond the slots wait for a
// whole workgroup time (N = 14939: 523 workgroups of 896 columns 123 us, 465 of 1024 columns 101 us).
inline int symk_one_round_chunk(int64_t N, int BR, int slots) {
  const int nrb = (int)((N + BR - 1) / BR);
  for (int c = 64; c <= 8192; c += 64) {
    long long total = 0;
    for (int b = 0; b < nrb; ++b) total += (N - (long long)b * BR + c - 1) / c;
    if (total <= slots) return c;
  }
  return 8192;
}

inline SymkPlan symk_plan(int64_t N, int world, int rank, bool wide = false) {
  SymkPlan sp;
  // A cached workgroup has no exponentials to hide its prologue (row block of V, ring start-up) and epilogue (slabs)
  // behind, so it wants longer column chunks than the fused sweep: measured optimum ~N / 14 workgroups per rank
  // (N = 15k: 1000, T = 11 product 0.152 ms against 0.199 ms with the fused sweep's 4600; N = 50k: 3600, 1.31 ms).
  double wgs = (double)N / 14.0;
  wgs = wgs < 512.0 ? 512.0 : (wgs > 4608.0 ? 4608.0 : wgs);
  const bool r1 = symk_r1(N, world);
  int chunk = 0;
  if (wide && world <= 1) {
    // The matrix-core (wide) product keeps two workgroups per CU resident and a workgroup's prologue / slabs cost more than
    // in the thin form: few, long workgroups.  The subtile layout of the cache depends on (N, R) only, so the build and the
    // product of a whole (unsharded) cache may be chunked differently; sharded caches keep one rule for both (their byte
    // ranges follow it).
    // EXACTLY filled rounds of the 2-per-CU resident workgroups: one round up to N = 36 000, three above
    // (tools/experiments/r5_symk_rounds.py: 28 001: 342 -> 307 us, 33 000: 426 -> 397, 40 000: 613 -> 592, 50 000: 957 -> 934
    // against the N / 28 rule, whose workgroup count lands between two rounds)
    // (two per CU also for the 256-row kernel, whose 154 registers would admit three: sized for three it is 0 - 9 % slower)
    chunk = symk_one_round_chunk(N, r1 ? 256 : 512, (N <= 36000 ? 1 : 3) * 2 * (g_num_cus > 0 ? g_num_cus : 256));
  }
  sp.p = make_plan(N, N, true, 12, world, rank, r1, 0, wgs, false, chunk);      // R = 2 above kSymkR1Max, whatever T is later
  sp.sub0 = symk_wg_subtile(sp.p, N, sp.p.w0);
  sp.sub1 = symk_wg_subtile(sp.p, N, sp.p.w1);
  return sp;
}
// (+ one subtile of padding: the wide product's requests run a few tiles past a workgroup's last subtile)
inline size_t symk_bytes(const SymkPlan &sp) { return (size_t)(sp.sub1 - sp.sub0 + 1) * sp.p.BR * 64 * sizeof(float); }
// nontemporal loads unless the (rank's share of the) cache fits the Infinity Cache
inline bool symk_nt_loads(const SymkPlan &sp) {
  return symk_bytes(sp) > (size_t)300000000;      // (277 MB: default policy 60.9 us against 64.6; 464 MB: 113 against 106)
}
inline int symk_t_piece(int remaining) {
  if (remaining > 4) return 12;                        // (an exact T = 11 instantiation measured slower than the padded 12)
  if (remaining > 1) return 4;
  return 1;
}
template <int JT>
int symk_launch_build(const SymkPlan &sp, const float *Z, float4v *cache, int N, int ldz, int j0, int accumulate,
                      hipStream_t st) {
  dim3 grid(sp.p.w1 - sp.p.w0), block(256);
  if (sp.p.R == 2)
    hipLaunchKernelGGL((symk_build_kernel<JT, 2>), grid, block, 0, st, Z, cache, N, ldz, j0, sp.p.chunk_cols, g_rotdir,
                       accumulate, sp.p.w0, sp.sub0);
  else
    hipLaunchKernelGGL((symk_build_kernel<JT, 1>), grid, block, 0, st, Z, cache, N, ldz, j0, sp.p.chunk_cols, g_rotdir,
                       accumulate, sp.p.w0, sp.sub0);
  return launch_status();
}
template <int JT>
int symk_launch_build_tile(const SymkPlan &sp, const float *Z, float4v *cache, int N, int ldz, int j0, int accumulate,
                           hipStream_t st) {
  dim3 grid(sp.p.w1 - sp.p.w0), block(256);
  if (sp.p.R == 2)
    hipLaunchKernelGGL((symk_build_tile_kernel<JT, 2>), grid, block, 0, st, Z, cache, N, ldz, j0, sp.p.chunk_cols,
                       accumulate, sp.p.w0, sp.sub0);
  else
    hipLaunchKernelGGL((symk_build_tile_kernel<JT, 1>), grid, block, 0, st, Z, cache, N, ldz, j0, sp.p.chunk_cols,
                       accumulate, sp.p.w0, sp.sub0);
  return launch_status();
}
inline int symk_launch_mvm_tile(const SymkPlan &sp, const float4v *cache, const float *V, float *slabR, float *slabT,
                                int N, int T, int t0, int tcnt, hipStream_t st) {
  dim3 grid(sp.p.w1 - sp.p.w0), block(256);
  const bool nt = symk_nt_loads(sp);
#define RPGP_SYMK_T2(RR, NTF)                                                                                        \
  hipLaunchKernelGGL((symk_mvm_tile2_kernel<RR, NTF>), grid, block, 0, st, cache, V, slabR, slabT, N, T, t0, tcnt,   \
                     sp.p.chunk_cols, sp.p.w0, sp.p.rb0, sp.p.row0, sp.p.rows, sp.sub0)
  if (sp.p.R == 2) {
    if (nt) RPGP_SYMK_T2(2, true); else RPGP_SYMK_T2(2, false);
  } else {
    if (nt) RPGP_SYMK_T2(1, true); else RPGP_SYMK_T2(1, false);
  }
#undef RPGP_SYMK_T2
  return launch_status();
}
template <int TT>
int symk_launch_mvm(const SymkPlan &sp, const float4v *cache, const float *V, float *slabR, float *slabT, int N, int T,
                    int t0, int tcnt, hipStream_t st) {
  dim3 grid(sp.p.w1 - sp.p.w0), block(256);
  const bool nt = symk_nt_loads(sp);
#define RPGP_SYMK_THIN(RR, NTF)                                                                                      \
  hipLaunchKernelGGL((symk_mvm_kernel<TT, RR, NTF>), grid, block, 0, st, cache, V, slabR, slabT, N, T, t0, tcnt,     \
                     sp.p.chunk_cols, g_rotdir, 0, sp.p.w0, sp.p.rb0, sp.p.row0, sp.p.rows, sp.sub0)
  if (sp.p.R == 2) {
    if (nt) RPGP_SYMK_THIN(2, true); else RPGP_SYMK_THIN(2, false);
  } else {
    if (nt) RPGP_SYMK_THIN(1, true); else RPGP_SYMK_THIN(1, false);
  }
#undef RPGP_SYMK_THIN
  return launch_status();
}
}  // namespace

extern "C" {

size_t rpgp_symcache_bytes(int64_t N, int world, int rank) {
  if (N <= 0 || N > 0x7fffffffLL || world < 1 || rank < 0 || rank >= world) return 0;
  return symk_bytes(symk_plan(N, world, rank));          // (the layout's R depends on (N, world) only: one size for both layouts)
}

size_t rpgp_symcache_workspace_bytes(int64_t N, int T, int world, int rank) {
  if (N <= 0 || N > 0x7fffffffLL || T <= 0 || world < 1 || rank < 0 || rank >= world) return 0;
  (void)rpgp_init();                               // (the wide plan counts the device's CUs; harmless without a device)
  const size_t a = plan_workspace_floats(symk_plan(N, world, rank, false).p, N, T, true);
  const size_t b = plan_workspace_floats(symk_plan(N, world, rank, true).p, N, T, true);        // (chunked differently)
  return (a > b ? a : b) * sizeof(float);
}

int rpgp_symcache_build(const float *Z, void *cache, size_t cache_bytes, int64_t N, int ldz, int j0, int j1, int layout,
                        int world, int rank, void *stream) {
  if (!Z || !cache || N <= 0 || N > 0x7fffffffLL || j0 < 0 || j1 <= j0 || ldz < j1 || world < 1 || rank < 0 ||
      rank >= world || (layout != RPGP_SYMCACHE_THIN && layout != RPGP_SYMCACHE_WIDE))
    return RPGP_EINVAL;
  const int irc = rpgp_init();
  if (irc) return irc;
  SymkPlan sp = symk_plan(N, world, rank);
  if (cache_bytes < symk_bytes(sp)) return RPGP_EWORKSPACE;
  if (world <= 1) {
    // The build of a whole cache is chunked on its own (the layout depends on (N, R) only): a compute-bound sweep of equal
    // workgroups at eight per CU wants MANY of them — ~6000 instead of the product's N / 14 (tools/experiments/
    // r5_symk_build_wgs.py, profiles/r5b_symk_build_wgs.jsonl: N = 7k 93.6 -> 72.8 us, 15k 267 -> 245, 28k 930 -> 834, 50k 2796 -> 2739)
    sp.p = make_plan(N, N, true, 12, world, rank, symk_r1(N, world), 0, 6144.0);
    sp.sub0 = symk_wg_subtile(sp.p, N, sp.p.w0);
    sp.sub1 = symk_wg_subtile(sp.p, N, sp.p.w1);
  }
  if (sp.p.w1 <= sp.p.w0) return 0;
  hipStream_t st = as_stream(stream);
  float4v *c = reinterpret_cast<float4v *>(cache);
  int first = 1;
  for (int j = j0; j < j1;) {
    const int jt = next_j_piece(j1 - j);
    int rc = 0;
    if (layout == RPGP_SYMCACHE_WIDE) {
      switch (jt) {
        case 20: rc = symk_launch_build_tile<20>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 10: rc = symk_launch_build_tile<10>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 8: rc = symk_launch_build_tile<8>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 5: rc = symk_launch_build_tile<5>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 4: rc = symk_launch_build_tile<4>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 3: rc = symk_launch_build_tile<3>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        case 2: rc = symk_launch_build_tile<2>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
        default: rc = symk_launch_build_tile<1>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      }
    } else
    switch (jt) {
      case 20: rc = symk_launch_build<20>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 10: rc = symk_launch_build<10>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 8: rc = symk_launch_build<8>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 5: rc = symk_launch_build<5>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 4: rc = symk_launch_build<4>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 3: rc = symk_launch_build<3>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      case 2: rc = symk_launch_build<2>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
      default: rc = symk_launch_build<1>(sp, Z, c, (int)N, ldz, j, first ? 0 : 1, st); break;
    }
    if (rc) return rc;
    first = 0;
    j += jt;
  }
  return 0;
}

int rpgp_symcache_mvm(const void *cache, size_t cache_bytes, int layout, const float *V, float *out, int64_t N, int T,
                      float scale, float noise, int world, int rank, void *ws, size_t ws_bytes, void *stream) {
  if (!cache || !V || !out || N <= 0 || N > 0x7fffffffLL || T <= 0 || world < 1 || rank < 0 || rank >= world ||
      (layout != RPGP_SYMCACHE_THIN && layout != RPGP_SYMCACHE_WIDE))
    return RPGP_EINVAL;
  const int irc = rpgp_init();
  if (irc) return irc;
  const SymkPlan sp = symk_plan(N, world, rank, layout == RPGP_SYMCACHE_WIDE);
  if (cache_bytes < symk_bytes(sp)) return RPGP_EINVAL;
  const TilePlan &p = sp.p;
  const size_t need = plan_workspace_floats(p, N, T, true) * sizeof(float);
  if (need && (!ws || ws_bytes < need)) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  float *slabR = reinterpret_cast<float *>(ws);
  float *slabT = slabR + (size_t)p.maxchunks * p.rows * T;
  if (p.partial && need) RPGP_CHECK(hipMemsetAsync(ws, 0, need, st));   // row blocks shared with a neighbour rank
  const float4v *c = reinterpret_cast<const float4v *>(cache);
  for (int t0 = 0; layout == RPGP_SYMCACHE_WIDE && t0 < T && p.w1 > p.w0; t0 += 16) {
    const int tcnt = (T - t0 < 16) ? T - t0 : 16;
    const int rc = symk_launch_mvm_tile(sp, c, V, slabR, slabT, (int)N, T, t0, tcnt, st);
    if (rc) return rc;
  }
  for (int t0 = 0; layout == RPGP_SYMCACHE_THIN && t0 < T && p.w1 > p.w0;) {
    const int tt = symk_t_piece(T - t0);
    const int tcnt = (T - t0 < tt) ? T - t0 : tt;
    int rc = 0;
    switch (tt) {
      case 1: rc = symk_launch_mvm<1>(sp, c, V, slabR, slabT, (int)N, T, t0, tcnt, st); break;
      case 4: rc = symk_launch_mvm<4>(sp, c, V, slabR, slabT, (int)N, T, t0, tcnt, st); break;
      default: rc = symk_launch_mvm<12>(sp, c, V, slabR, slabT, (int)N, T, t0, tcnt, st); break;
    }
    if (rc) return rc;
    t0 += tcnt;
  }
  const size_t total = (size_t)N * T;
  return mvm_reduce_launch(total, st, slabR, slabT, V, out, (int)N, (int)N, T, p.BR, p.chunk_cols, 1, scale, noise,
                           (const int *)nullptr, p.rb0, p.rb1, p.row0, p.rows);
}

}  // extern "C"
