// rpgp_bilinear.hip — the bilinear derivative of the additive kernel: the full and the symmetric sweep, the
// form with an explicit S, the generalised-family forms, their slab reduces and fixed-order column / vector sums, and the
// rpgp_bilinear_grad* / rpgp_family_bilinear_grad* entries of the C-ABI.  The hand-scheduled form of
// bilinear_sym_kernel<20, 12, true> is rpgp_bil_asm.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stddef.h>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"
#include "rpgp_tile.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Bilinear derivative.  Lane owns a row; columns broadcast from LDS.
//   S = sum_t L[i,t] R[i',t] + R[i,t] L[i',t]
//   gz[i][j] += S * e_j * d_j   (d in exp2-scaled units; caller multiplies by -scale/kExp2Scale... see host)
//   gs[i]    += S * sum_j e_j
// grid = (column splits, row blocks of 256); partial slabs reduced by bilinear_reduce_kernel.
// ---------------------------------------------------------------------------------------------
template <int JT, int TT>
__global__ __launch_bounds__(256) void bilinear_kernel(const float *__restrict__ Z, const float *__restrict__ L,
                                                       const float *__restrict__ Rm, float *__restrict__ slabG,
                                                       float *__restrict__ slabS, int N, int ldz, int T, int j0,
                                                       int cols_per_split) {
  constexpr int STR = JT + 2 * TT;
  __shared__ __attribute__((aligned(16))) float sC[64 * STR];
  const int tid = threadIdx.x;
  const int row = blockIdx.y * 256 + tid;
  const bool valid = row < N;
  const int c_begin = blockIdx.x * cols_per_split;
  if (c_begin >= N) return;
  const int c_end = (c_begin + cols_per_split < N) ? c_begin + cols_per_split : N;

  float a[JT], li[TT], ri[TT], accG[JT];
  float accS = 0.f;
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    a[j] = valid ? Z[(size_t)row * ldz + j0 + j] * kExp2Scale : 0.f;
    accG[j] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    li[t] = (valid && t < T) ? L[(size_t)row * T + t] : 0.f;
    ri[t] = (valid && t < T) ? Rm[(size_t)row * T + t] : 0.f;
  }
  for (int c0 = c_begin; c0 < c_end; c0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * STR; e += 256) {
      const int c = e / STR, q = e % STR;
      const int col = c0 + c;
      float val = 0.f;
      if (col < c_end) {
        if (q < JT) val = Z[(size_t)col * ldz + j0 + q] * kExp2Scale;
        else if (q < JT + TT) { const int t = q - JT; val = t < T ? L[(size_t)col * T + t] : 0.f; }
        else { const int t = q - JT - TT; val = t < T ? Rm[(size_t)col * T + t] : 0.f; }
      }
      sC[e] = val;
    }
    __syncthreads();
    const int nc = (c_end - c0 < 64) ? c_end - c0 : 64;
    for (int c = 0; c < nc; ++c) {
      const float *p = sC + c * STR;
      float S = 0.f;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        S = __builtin_fmaf(li[t], p[JT + TT + t], S);
        S = __builtin_fmaf(ri[t], p[JT + t], S);
      }
      float ks = 0.f;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const float dd = a[j] - p[j];
        const float e = fast_exp2(-(dd * dd));
        ks += e;
        accG[j] = __builtin_fmaf(S * e, dd, accG[j]);
      }
      accS = __builtin_fmaf(S, ks, accS);
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < JT; ++j) slabG[((size_t)blockIdx.x * N + row) * JT + j] = accG[j];
    slabS[(size_t)blockIdx.x * N + row] = accS;
  }
}

// ---------------------------------------------------------------------------------------------
// Symmetric form of the bilinear derivative (what training runs at N >= 2048): S_ii' = S_i'i, so every unordered pair
// is evaluated ONCE and feeds both rows,
//     gz[i][j] += S e_j d_j      gz[i'][j] -= S e_j d_j      gs[i] += S sum_j e_j      gs[i'] += S sum_j e_j
// — half the exponentials of the full sweep above.  Same tile decomposition as the fused MVM (a workgroup owns BR = 512
// rows and a chunk of columns starting at its diagonal block; lane l visits column (l + s) mod 64 at step s; the JT + 1
// transposed accumulators travel with their column by a DPP wave rotate per step); two rows per lane halve the LDS
// traffic per pair (the one-row full sweep spends 11 ds_read_b128 per pair: 93 % of the LDS issue rate).
// slabR[kchunk][row][JT + 1] : row sums of a column chunk         slabT[rb][col][JT + 1] : transposed sums of row block rb
// ---------------------------------------------------------------------------------------------
// LDS-DMA of one dword per lane (wave-instruction: 64 consecutive floats at `lds_dst`); hipcc does not count it: the caller
// waits with an explicit s_waitcnt vmcnt.  M0 (the DMA's LDS base) is written in the statement that uses it.
__device__ __forceinline__ void glds_dword(const void *gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

// Zs[n][q] = Z[n][j0 + q] * kExp2Scale (the derivative's DMA staging cannot scale on the way into LDS)
__global__ __launch_bounds__(256) void scale_columns_kernel(const float *__restrict__ Z, float *__restrict__ Zs, long long N,
                                                            int ldz, int j0, int JT) {
  const long long total = N * JT;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long n = g / JT;
    const int q = (int)(g - n * JT);
    Zs[g] = Z[n * ldz + j0 + q] * kExp2Scale;
  }
}

// DMA = true (JT + 2 TT a multiple of 4 with an odd quarter, so that the LDS records are unpadded and the subtile image is
// linear, and 64 records a whole number of 256-element pieces): Z is the pre-scaled copy Zs (row stride JT, j0 = 0) and the
// subtile's 64 column records are written by LDS-DMA — the register staging loop compiles to global_load; s_waitcnt vmcnt(0);
// ds_write per element (eleven serial round trips per subtile with all four waves idle), and unrolling it into registers
// spills (the kernel already holds 252 VGPRs: 106 spills, 7.0 ms).
template <int JT, int TT, bool DMA = false>
__global__ __launch_bounds__(256, 2) void bilinear_sym_kernel(const float *__restrict__ Z, const float *__restrict__ L,
                                                              const float *__restrict__ Rm, float *__restrict__ slabR,
                                                              float *__restrict__ slabT, int N, int ldz, int T, int j0,
                                                              int chunk_cols, int rotdir, int w0, int rb_first,
                                                              int slab_row0, int slab_rows) {
  constexpr int R = 2;
  constexpr int BR = 256 * R;
  constexpr int W = JT + 1;                        // slab width: JT gradient columns + the scale column
  constexpr int STRQ = JT + 2 * TT;
  constexpr int STR = (STRQ % 4 == 0) ? (((STRQ / 4) % 2 == 1) ? STRQ : STRQ + 4) : STRQ;   // (STR/4) odd: conflict-free b128
  __shared__ __attribute__((aligned(16))) float sC[64 * STR];
  __shared__ __attribute__((aligned(16))) float sT[4 * 64 * W];
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

  float a[R][JT], li[R][TT], ri[R][TT], accG[R][JT], accS[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    const bool valid = row < N;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      if constexpr (DMA) a[r][j] = valid ? Z[(size_t)row * JT + j] : 0.f;
      else a[r][j] = valid ? Z[(size_t)row * ldz + j0 + j] * kExp2Scale : 0.f;
      accG[r][j] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {               // rows beyond N: L = R = 0 -> S = 0 -> no contribution
      li[r][t] = (valid && t < T) ? L[(size_t)row * T + t] : 0.f;
      ri[r][t] = (valid && t < T) ? Rm[(size_t)row * T + t] : 0.f;
    }
    accS[r] = 0.f;
  }

  for (int c0 = c_begin; c0 < c_end; c0 += 64) {
    __syncthreads();
    if constexpr (DMA) {
      static_assert(STR == STRQ, "linear (unpadded) subtile image");
      constexpr int NST = (64 * STRQ + 255) / 256;             // (the last piece may be partial: its tail lanes are masked off)
      const unsigned sc_bytes = (unsigned)(size_t)sC;
      const unsigned uw = __builtin_amdgcn_readfirstlane((unsigned)wave);
#pragma unroll 1                                                 // (rolled: unrolled, the eleven address computations are hoisted
      for (int it = 0; it < NST; ++it) {                         //  together and spill; the DMAs need no wait between them)
        const int e = tid + 256 * it;
        if (e >= 64 * STRQ) break;                              // (EXEC-masked lanes of a DMA do not write)
        const int c = e / STRQ, q = e % STRQ;
        const int col = c0 + c;
        const int colc = col < N ? col : N - 1;                 // clamped: every lane of the DMA reads a valid address
        const bool isz = q < JT, isl = q < JT + TT;
        int t = isz ? 0 : (isl ? q - JT : q - JT - TT);
        t = t < T ? t : T - 1;                                  // (slot t >= T: the row side's L / R are zero there)
        const float *src = isz ? Z : (isl ? L : Rm);
        const size_t off = isz ? (size_t)colc * JT + q : (size_t)colc * T + t;
        glds_dword(src + off, __builtin_amdgcn_readfirstlane(sc_bytes + (unsigned)(it * 256 + (int)uw * 64) * 4u));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (c0 + 64 > c_end) {                                    // ragged last subtile: columns beyond the end get L = R = 0
#pragma unroll 1
        for (int it = 0; it < NST; ++it) {
          const int e = tid + 256 * it;
          const int c = e / STRQ, q = e % STRQ;
          if (e < 64 * STRQ && c0 + c >= c_end && q >= JT) sC[e] = 0.f;
        }
      }
    } else {
      for (int e = tid; e < 64 * STRQ; e += 256) {
        const int c = e / STRQ, q = e % STRQ;
        const int col = c0 + c;
        float val = 0.f;                            // columns beyond the chunk: L = R = 0 -> S = 0
        if (col < c_end) {
          if (q < JT) val = Z[(size_t)col * ldz + j0 + q] * kExp2Scale;
          else if (q < JT + TT) { const int t = q - JT; val = t < T ? L[(size_t)col * T + t] : 0.f; }
          else { const int t = q - JT - TT; val = t < T ? Rm[(size_t)col * T + t] : 0.f; }
        }
        sC[c * STR + q] = val;
      }
    }
    __syncthreads();
    const bool doT = (c0 >= r0 + BR);
    float accT[W];
#pragma unroll
    for (int q = 0; q < W; ++q) accT[q] = 0.f;
#pragma unroll 1
    for (int s = 0; s < 64; ++s) {
      const float *p = sC + __mul24((lane + rotdir * s) & 63, STR);       // (24-bit multiply: v_mul_lo_u32 is quarter rate)
      float pz[JT], pl[TT], pr[TT];
#pragma unroll
      for (int j = 0; j < JT; ++j) pz[j] = p[j];
#pragma unroll
      for (int t = 0; t < TT; ++t) { pl[t] = p[JT + t]; pr[t] = p[JT + TT + t]; }
      float tg[W];
#pragma unroll
      for (int q = 0; q < W; ++q) tg[q] = accT[q];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float S = 0.f;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          S = __builtin_fmaf(li[r][t], pr[t], S);
          S = __builtin_fmaf(ri[r][t], pl[t], S);
        }
        float ks = 0.f;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
          const float dd = a[r][j] - pz[j];
          const float e = fast_exp2(-(dd * dd));
          ks += e;
          const float se = S * e;                       // g = (S e) d feeds both sides as an FMA (was mul + add + sub)
          accG[r][j] = __builtin_fmaf(se, dd, accG[r][j]);
          tg[j] = __builtin_fmaf(-se, dd, tg[j]);
        }
        const float sk = S * ks;
        accS[r] += sk;
        tg[JT] += sk;
      }
      if (doT) {
#pragma unroll
        for (int q = 0; q < W; ++q) accT[q] = wave_rotate1(tg[q]);
      }
    }
    if (doT) {
#pragma unroll
      for (int q = 0; q < W; ++q) sT[(wave * 64 + lane) * W + q] = accT[q];
    }
    __syncthreads();
    if (doT) {
      for (int e = tid; e < 64 * W; e += 256) {
        const int c = e / W, q = e % W;
        const int col = c0 + c;
        if (col < c_end) {
          const float sum = sT[(0 * 64 + c) * W + q] + sT[(1 * 64 + c) * W + q] + sT[(2 * 64 + c) * W + q] +
                            sT[(3 * 64 + c) * W + q];
          slabT[((size_t)(rb - rb_first) * N + col) * W + q] = sum;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + wave * (64 * R) + r * 64 + lane;
    if (row < N) {
      float *dst = slabR + ((size_t)kchunk * slab_rows + (row - slab_row0)) * W;
#pragma unroll
      for (int j = 0; j < JT; ++j) dst[j] = accG[r][j];
      dst[JT] = accS[r];
    }
  }
}

// gZ[row][j0 + q] = mulG * (sum_k slabR[k][row][q] + sum_{b < row / BR} slabT[b][row][q]),  q < JT;   column JT -> rowS
__global__ __launch_bounds__(256) void bilinear_sym_reduce_kernel(const float *__restrict__ slabR,
                                                                  const float *__restrict__ slabT,
                                                                  float *__restrict__ gZ, float *__restrict__ rowS, int N,
                                                                  int JT, int ldg, int j0, int BR, int chunk_cols,
                                                                  int slab_rows, float mulG, int accumulate) {
  const int W = JT + 1;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)N * W) return;
  const int row = (int)(gid / W), q = (int)(gid % W);
  const int rb = row / BR;
  const int nk = (N - rb * BR + chunk_cols - 1) / chunk_cols;
  double acc = 0.0;
  // four slab entries requested together, added in slab order (a rolled `acc += load` loop waits for every load: up to
  // ~110 serial round trips per output at N = 50k)
  int k = 0;
  for (; k + 3 < nk; k += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = slabR[(size_t)(k + u) * slab_rows * W + gid];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += (double)v[u];
  }
  for (; k < nk; ++k) acc += (double)slabR[(size_t)k * slab_rows * W + gid];
  int b = 0;
  for (; b + 3 < rb; b += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = slabT[(size_t)(b + u) * N * W + gid];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += (double)v[u];
  }
  for (; b < rb; ++b) acc += (double)slabT[(size_t)b * N * W + gid];
  if (q < JT) gZ[(size_t)row * ldg + j0 + q] = mulG * (float)acc;
  else rowS[row] = accumulate ? rowS[row] + (float)acc : (float)acc;
}

// Dense-weight variant for the Cholesky regime (N <= max_cholesky_size): S is an explicit symmetric N x N matrix
// (e.g. Khat^-1 - alpha alpha^T).  Lane owns row i and reads S[c][i] (coalesced thanks to symmetry).
template <int JT>
__global__ __launch_bounds__(256) void bilinear_dense_kernel(const float *__restrict__ Z, const float *__restrict__ S,
                                                             float *__restrict__ slabG, float *__restrict__ slabS,
                                                             int N, int ldz, long long lds_, int j0,
                                                             int cols_per_split) {
  __shared__ __attribute__((aligned(16))) float sC[64 * JT];
  const int tid = threadIdx.x;
  const int row = blockIdx.y * 256 + tid;
  const bool valid = row < N;
  const int c_begin = blockIdx.x * cols_per_split;
  if (c_begin >= N) return;
  const int c_end = (c_begin + cols_per_split < N) ? c_begin + cols_per_split : N;
  float a[JT], accG[JT];
  float accS = 0.f;
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    a[j] = valid ? Z[(size_t)row * ldz + j0 + j] * kExp2Scale : 0.f;
    accG[j] = 0.f;
  }
  for (int c0 = c_begin; c0 < c_end; c0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * JT; e += 256) {
      const int c = e / JT, q = e % JT;
      const int col = c0 + c;
      sC[e] = (col < c_end) ? Z[(size_t)col * ldz + j0 + q] * kExp2Scale : 0.f;
    }
    __syncthreads();
    const int nc = (c_end - c0 < 64) ? c_end - c0 : 64;
    for (int c = 0; c < nc; ++c) {
      const float *p = sC + c * JT;
      const float Sv = valid ? S[(size_t)(c0 + c) * lds_ + row] : 0.f;
      float ks = 0.f;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const float dd = a[j] - p[j];
        const float e = fast_exp2(-(dd * dd));
        ks += e;
        accG[j] = __builtin_fmaf(Sv * e, dd, accG[j]);
      }
      accS = __builtin_fmaf(Sv, ks, accS);
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < JT; ++j) slabG[((size_t)blockIdx.x * N + row) * JT + j] = accG[j];
    slabS[(size_t)blockIdx.x * N + row] = accS;
  }
}

// gZ[row][j0+j] = mulG * sum_split slabG ; rowS[row] = sum_split slabS  (+= if accumulate)
__global__ void bilinear_reduce_kernel(const float *__restrict__ slabG, const float *__restrict__ slabS,
                                       float *__restrict__ gZ, float *__restrict__ rowS, int N, int JT, int ldg,
                                       int j0, int nsplit, float mulG, int accumulate) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)N * (JT + 1)) return;
  const int row = (int)(gid / (JT + 1));
  const int q = (int)(gid % (JT + 1));
  float acc = 0.f;
  if (q < JT) {
    for (int s = 0; s < nsplit; ++s) acc += slabG[((size_t)s * N + row) * JT + q];
    gZ[(size_t)row * ldg + j0 + q] = mulG * acc;
  } else {
    for (int s = 0; s < nsplit; ++s) acc += slabS[(size_t)s * N + row];
    rowS[row] = accumulate ? rowS[row] + acc : acc;
  }
}

// ---------------------------------------------------------------------------------------------
// Bilinear derivative for the generalised family (weighted policies): same sweep as bilinear_kernel, but the
// per-row by-products are the UNWEIGHTED per-component sums  rowC[i][c] = sum_i' S_ii' phi_c(i,i')  (the gradients of
// the component weights and of the outer scale follow from them on the host).
// ---------------------------------------------------------------------------------------------
template <int JT, int TT, class KF>
__global__ __launch_bounds__(256) void family_bilinear_kernel(const float *__restrict__ Z, const float *__restrict__ L,
                                                              const float *__restrict__ Rm, float *__restrict__ slabG,
                                                              float *__restrict__ slabC, int N, int ldz, int T, int j0,
                                                              int cols_per_split, const float *__restrict__ wts) {
  constexpr int STR = JT + 2 * TT;
  constexpr int NC = JT / KF::group;
  __shared__ __attribute__((aligned(16))) float sC[64 * STR];
  const int tid = threadIdx.x;
  const int row = blockIdx.y * 256 + tid;
  const bool valid = row < N;
  const int c_begin = blockIdx.x * cols_per_split;
  if (c_begin >= N) return;
  const int c_end = (c_begin + cols_per_split < N) ? c_begin + cols_per_split : N;

  float wreg[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) wreg[c] = wts[j0 / KF::group + c];
  float a[JT], li[TT], ri[TT], accG[JT], accC[NC];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    a[j] = valid ? Z[(size_t)row * ldz + j0 + j] * KF::pre : 0.f;
    accG[j] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) accC[c] = 0.f;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    li[t] = (valid && t < T) ? L[(size_t)row * T + t] : 0.f;
    ri[t] = (valid && t < T) ? Rm[(size_t)row * T + t] : 0.f;
  }
  for (int c0 = c_begin; c0 < c_end; c0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * STR; e += 256) {
      const int c = e / STR, q = e % STR;
      const int col = c0 + c;
      float val = 0.f;
      if (col < c_end) {
        if (q < JT) val = Z[(size_t)col * ldz + j0 + q] * KF::pre;
        else if (q < JT + TT) { const int t = q - JT; val = t < T ? L[(size_t)col * T + t] : 0.f; }
        else { const int t = q - JT - TT; val = t < T ? Rm[(size_t)col * T + t] : 0.f; }
      }
      sC[e] = val;
    }
    __syncthreads();
    const int nc = (c_end - c0 < 64) ? c_end - c0 : 64;
    for (int c = 0; c < nc; ++c) {
      const float *p = sC + c * STR;
      float S = 0.f;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        S = __builtin_fmaf(li[t], p[JT + TT + t], S);
        S = __builtin_fmaf(ri[t], p[JT + t], S);
      }
      KF::template pair_grad<JT>(a, p, wreg, S, accG, accC);
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < JT; ++j) slabG[((size_t)blockIdx.x * N + row) * JT + j] = accG[j];
#pragma unroll
    for (int c = 0; c < NC; ++c) slabC[((size_t)blockIdx.x * N + row) * NC + c] = accC[c];
  }
}

// explicit symmetric weight matrix S (Cholesky regime), cf. bilinear_dense_kernel
template <int JT, class KF>
__global__ __launch_bounds__(256) void family_bilinear_dense_kernel(const float *__restrict__ Z,
                                                                    const float *__restrict__ S,
                                                                    float *__restrict__ slabG, float *__restrict__ slabC,
                                                                    int N, int ldz, long long lds_, int j0,
                                                                    int cols_per_split, const float *__restrict__ wts) {
  constexpr int NC = JT / KF::group;
  __shared__ __attribute__((aligned(16))) float sC[64 * JT];
  const int tid = threadIdx.x;
  const int row = blockIdx.y * 256 + tid;
  const bool valid = row < N;
  const int c_begin = blockIdx.x * cols_per_split;
  if (c_begin >= N) return;
  const int c_end = (c_begin + cols_per_split < N) ? c_begin + cols_per_split : N;
  float wreg[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) wreg[c] = wts[j0 / KF::group + c];
  float a[JT], accG[JT], accC[NC];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    a[j] = valid ? Z[(size_t)row * ldz + j0 + j] * KF::pre : 0.f;
    accG[j] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) accC[c] = 0.f;
  for (int c0 = c_begin; c0 < c_end; c0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * JT; e += 256) {
      const int c = e / JT, q = e % JT;
      const int col = c0 + c;
      sC[e] = (col < c_end) ? Z[(size_t)col * ldz + j0 + q] * KF::pre : 0.f;
    }
    __syncthreads();
    const int nc = (c_end - c0 < 64) ? c_end - c0 : 64;
    for (int c = 0; c < nc; ++c) {
      const float Sv = valid ? S[(size_t)(c0 + c) * lds_ + row] : 0.f;
      KF::template pair_grad<JT>(a, sC + c * JT, wreg, Sv, accG, accC);
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < JT; ++j) slabG[((size_t)blockIdx.x * N + row) * JT + j] = accG[j];
#pragma unroll
    for (int c = 0; c < NC; ++c) slabC[((size_t)blockIdx.x * N + row) * NC + c] = accC[c];
  }
}

// gZ[row][j0+j] = mulG * sum_split slabG ; rowC[row][c0 + c] = sum_split slabC
__global__ void family_bilinear_reduce_kernel(const float *__restrict__ slabG, const float *__restrict__ slabC,
                                              float *__restrict__ gZ, float *__restrict__ rowC, int N, int JT, int NC,
                                              int ldg, int j0, int c0, int ncomp, int nsplit, float mulG) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)N * (JT + NC)) return;
  const int row = (int)(gid / (JT + NC));
  const int q = (int)(gid % (JT + NC));
  float acc = 0.f;
  if (q < JT) {
    for (int s = 0; s < nsplit; ++s) acc += slabG[((size_t)s * N + row) * JT + q];
    gZ[(size_t)row * ldg + j0 + q] = mulG * acc;
  } else {
    const int c = q - JT;
    for (int s = 0; s < nsplit; ++s) acc += slabC[((size_t)s * N + row) * NC + c];
    rowC[(size_t)row * ncomp + c0 + c] = acc;
  }
}

// out[c] = mul * sum_row x[row][c]  (one workgroup per column, fixed order)
__global__ __launch_bounds__(1024) void sum_columns_kernel(const float *__restrict__ x, float *__restrict__ out, int n,
                                                           int ncols, float mul) {
  __shared__ float sh[1024];
  const int c = blockIdx.x;
  float a4[4] = {0.f, 0.f, 0.f, 0.f}, tail = 0.f;        // independent chains: the loads of four strides are in flight together
  int i = threadIdx.x;
  for (; i + 3 * 1024 < n; i += 4 * 1024) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = x[(size_t)(i + u * 1024) * ncols + c];
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] += v[u];
  }
  for (; i < n; i += 1024) tail += x[(size_t)i * ncols + c];
  const float acc = ((a4[0] + a4[1]) + (a4[2] + a4[3])) + tail;
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = sh[0] * mul;
}

// deterministic single-block sum: out[0] = mul * sum_i x[i]
__global__ __launch_bounds__(1024) void sum_vector_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                          int n, float mul) {
  __shared__ float sh[1024];
  // eight independent partial sums per thread (a single dependent chain of n / 1024 loads took 98 us at n = 391k); fixed order
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int i = threadIdx.x;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = x[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) a8[u] += v[u];
  }
  float tail = 0.f;
  for (; i < n; i += 1024) tail += x[i];
  const float acc = (((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]))) + tail;
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0] * mul;
}

template <int JT>
int launch_bilinear(int tt, const float *Z, const float *L, const float *R, float *slabG, float *slabS, int N,
                    int ldz, int T, int j0, int cols_per_split, int nsplit, hipStream_t st) {
  dim3 grid(nsplit, (N + 255) / 256);
  if (tt <= 1)
    hipLaunchKernelGGL((bilinear_kernel<JT, 1>), grid, dim3(256), 0, st, Z, L, R, slabG, slabS, N, ldz, T, j0, cols_per_split);
  else if (tt <= 4)
    hipLaunchKernelGGL((bilinear_kernel<JT, 4>), grid, dim3(256), 0, st, Z, L, R, slabG, slabS, N, ldz, T, j0, cols_per_split);
  else
    hipLaunchKernelGGL((bilinear_kernel<JT, 12>), grid, dim3(256), 0, st, Z, L, R, slabG, slabS, N, ldz, T, j0, cols_per_split);
  return launch_status();
}

template <int JT>
int launch_bilinear_dense(const float *Z, const float *S, float *slabG, float *slabS, int N, int ldz, long long lds_,
                          int j0, int cols_per_split, int nsplit, hipStream_t st) {
  dim3 grid(nsplit, (N + 255) / 256);
  hipLaunchKernelGGL((bilinear_dense_kernel<JT>), grid, dim3(256), 0, st, Z, S, slabG, slabS, N, ldz, lds_, j0,
                     cols_per_split);
  return launch_status();
}

// symmetric-sweep plan of the bilinear derivative (BR = 512): slabR [maxchunks][N][21] + slabT [row blocks][N][21] + rowS
inline bool bilinear_use_sym(int64_t N) {
  if (N < 2048) return false;
  const double slabT_bytes = (double)((N + 511) / 512) * (double)N * 21.0 * 4.0;
  return slabT_bytes <= 6.0e9;                     // beyond ~190k rows the full sweep's 46 MB workspace is kept
}
// (Chunk sizes from 448 to 896 columns at C4, 64 to 192 at C3 / C2 are within 2 % of each other for this sweep: its nine
//  rounds of unequal workgroups leave the dispatcher enough to smooth — profiles/r5b_bilinear_chunk_sweep.jsonl.)
inline TilePlan bilinear_plan(int64_t N) { return make_plan(N, N, true, 12, 1, 0, false, 512); }
inline size_t bilinear_sym_floats(int64_t N) {
  const TilePlan p = bilinear_plan(N);
  return ((size_t)p.maxchunks * N + (size_t)p.nrb * N) * 21 + (size_t)N + (size_t)N * 20;     // slabs, rowS, scaled copy of Z
}

template <int JT>
int launch_bilinear_sym(int tt, const TilePlan &p, const float *Z, const float *L, const float *R, float *slabR,
                               float *slabT, int N, int ldz, int T, int j0, hipStream_t st, float *Zs) {
  dim3 grid(p.total_wg), block(256);
  // (JT + 8 or JT + 24 a multiple of 8 would pad the LDS records: JT = 8 keeps the register staging)
  constexpr bool dma4 = !((JT + 8) % 4 == 0 && ((JT + 8) / 4) % 2 == 0), dma12 = !((JT + 24) % 4 == 0 && ((JT + 24) / 4) % 2 == 0);
  if constexpr (dma4 && dma12) {
    // the column records are staged by LDS-DMA from a pre-scaled copy of Z (20-column piece at C4: 6.26 -> 5.87 ms alternating
    // in one process, bit-identical results)
    if (Zs) {
      const long long total = (long long)N * JT;
      hipLaunchKernelGGL(scale_columns_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256),
                         0, st, Z, Zs, (long long)N, ldz, j0, JT);
      if constexpr (JT == 20) {
        // the hand-scheduled loop (rpgp_bil_asm.hip) for the training block (5 .. 12 right-hand-side slots) of the whole
        // J = 20 operator; RPGP_BIL_ASM=0 keeps the compiler-scheduled kernel (A/B runs, tests)
        const char *ea = getenv("RPGP_BIL_ASM");
        if (tt > 4 && T <= 12 && g_rotdir == 1 && !(ea && ea[0] == '0'))
          return rpgp_internal::launch_bilinear_sym_asm(Zs, L, R, slabR, slabT, N, T, p.chunk_cols, p.total_wg, st);
      }
      if (tt <= 4)
        hipLaunchKernelGGL((bilinear_sym_kernel<JT, 4, true>), grid, block, 0, st, Zs, L, R, slabR, slabT, N, JT, T, 0,
                           p.chunk_cols, g_rotdir, 0, 0, 0, N);
      else
        hipLaunchKernelGGL((bilinear_sym_kernel<JT, 12, true>), grid, block, 0, st, Zs, L, R, slabR, slabT, N, JT, T, 0,
                           p.chunk_cols, g_rotdir, 0, 0, 0, N);
      return launch_status();
    }
  }
  if (tt <= 4)
    hipLaunchKernelGGL((bilinear_sym_kernel<JT, 4>), grid, block, 0, st, Z, L, R, slabR, slabT, N, ldz, T, j0,
                       p.chunk_cols, g_rotdir, 0, 0, 0, N);
  else
    hipLaunchKernelGGL((bilinear_sym_kernel<JT, 12>), grid, block, 0, st, Z, L, R, slabR, slabT, N, ldz, T, j0,
                       p.chunk_cols, g_rotdir, 0, 0, 0, N);
  return launch_status();
}

inline int bilinear_nsplit(int64_t N) {
  const int64_t nrb = (N + 255) / 256;
  int64_t ns = (2048 + nrb - 1) / nrb;
  const int64_t maxs = (N + 255) / 256;
  if (ns > maxs) ns = maxs;
  if (ns < 1) ns = 1;
  return (int)ns;
}

}  // namespace

namespace rpgp_internal {
// fixed-order sums of a row vector / of the columns of an N x C block (the by-products of the derivative kernels), for the
// translation units that produce such blocks (rpgp_ski_base.hip)
int sum_vector_launch(const float *x, float *out, int n, float mul, hipStream_t st) {
  hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(1024), 0, st, x, out, n, mul);
  return (int)hipGetLastError();
}
int sum_columns_launch(const float *x, float *out, int n, int C, float mul, hipStream_t st) {
  hipLaunchKernelGGL(sum_columns_kernel, dim3(C), dim3(1024), 0, st, x, out, n, C, mul);
  return (int)hipGetLastError();
}
}  // namespace rpgp_internal

extern "C" {

size_t rpgp_bilinear_grad_workspace_bytes(int64_t N, int J) {
  if (N <= 0 || J <= 0) return 0;
  const int ns = bilinear_nsplit(N);
  // slabG [ns][N][<=20] + slabS [ns][N] + rowS [N]
  size_t f = (size_t)ns * N * 21 + (size_t)N;
  if (bilinear_use_sym(N)) {
    const size_t g = bilinear_sym_floats(N);
    if (g > f) f = g;
  }
  return f * sizeof(float);
}

int rpgp_bilinear_grad(const float *Z, const float *L, const float *R, float *gZ, float *gscale, int64_t N, int ldz,
                       int ldg, int T, int j0, int j1, float scale, void *workspace, size_t workspace_bytes,
                       void *stream) {
  if (!Z || !L || !R || !gZ || !gscale || N <= 0 || T <= 0 || T > 12 || j0 < 0 || j1 <= j0 || ldz < j1 || ldg < j1)
    return RPGP_EINVAL;
  if (N > 0x7fffffffLL) return RPGP_EINVAL;
  if (!workspace || workspace_bytes < rpgp_bilinear_grad_workspace_bytes(N, j1 - j0)) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  if (bilinear_use_sym(N)) {
    // symmetric sweep: every unordered pair once (half the exponentials), tile plan of the fused MVM with BR = 512
    int rc = rpgp_init();
    if (rc) return rc;
    const TilePlan p = bilinear_plan(N);
    float *slabR = reinterpret_cast<float *>(workspace);
    float *slabT = slabR + (size_t)p.maxchunks * N * 21;
    float *rowS = slabT + (size_t)p.nrb * N * 21;
    float *Zs = rowS + (size_t)N;
    int first = 1;
    for (int j = j0; j < j1;) {
      const int jt = next_j_piece(j1 - j);
      switch (jt) {
        case 20: rc = launch_bilinear_sym<20>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 10: rc = launch_bilinear_sym<10>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 8: rc = launch_bilinear_sym<8>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 5: rc = launch_bilinear_sym<5>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 3: rc = launch_bilinear_sym<3>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 4: rc = launch_bilinear_sym<4>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        case 2: rc = launch_bilinear_sym<2>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
        default: rc = launch_bilinear_sym<1>(T, p, Z, L, R, slabR, slabT, (int)N, ldz, T, j, st, Zs); break;
      }
      if (rc) return rc;
      const size_t total = (size_t)N * (jt + 1);
      hipLaunchKernelGGL(bilinear_sym_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slabR,
                         slabT, gZ, rowS, (int)N, jt, ldg, j, p.BR, p.chunk_cols, (int)N, -scale / kExp2Scale,
                         first ? 0 : 1);
      rc = launch_status();
      if (rc) return rc;
      first = 0;
      j += jt;
    }
    hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(1024), 0, st, rowS, gscale, (int)N, 0.5f);
    return launch_status();
  }
  const int ns_max = bilinear_nsplit(N);          // the slab layout (and the workspace size) uses the upper bound
  int cps = (int)((N + ns_max - 1) / ns_max);
  cps = (cps + 63) / 64 * 64;
  // splits that actually own columns: rounding cps up to 64 can leave trailing splits empty, and an empty split's
  // workgroups return without writing their slab — the reduce must not read them
  const int ns = (int)((N + cps - 1) / cps);
  float *slabG = reinterpret_cast<float *>(workspace);
  float *slabS = slabG + (size_t)ns_max * N * 20;
  float *rowS = slabS + (size_t)ns_max * N;
  int first = 1;
  for (int j = j0; j < j1;) {
    const int jt = next_j_piece(j1 - j);
    int rc;
    switch (jt) {
      case 20: rc = launch_bilinear<20>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 10: rc = launch_bilinear<10>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 8: rc = launch_bilinear<8>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 5: rc = launch_bilinear<5>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 3: rc = launch_bilinear<3>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 4: rc = launch_bilinear<4>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      case 2: rc = launch_bilinear<2>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
      default: rc = launch_bilinear<1>(T, Z, L, R, slabG, slabS, (int)N, ldz, T, j, cps, ns, st); break;
    }
    if (rc) return rc;
    // d/dZ = -scale * S e (z_i - z_i') ; kernel accumulated S e (c z_i - c z_i')  ->  multiply by -scale / c
    const size_t total = (size_t)N * (jt + 1);
    hipLaunchKernelGGL(bilinear_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slabG, slabS,
                       gZ, rowS, (int)N, jt, ldg, j, ns, -scale / kExp2Scale, first ? 0 : 1);
    rc = launch_status();
    if (rc) return rc;
    first = 0;
    j += jt;
  }
  hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(1024), 0, st, rowS, gscale, (int)N, 0.5f);
  return launch_status();
}

int rpgp_bilinear_grad_dense(const float *Z, const float *S, float *gZ, float *gscale, int64_t N, int ldz, int ldg,
                             int64_t lds_, int j0, int j1, float scale, void *workspace, size_t workspace_bytes,
                             void *stream) {
  if (!Z || !S || !gZ || !gscale || N <= 0 || j0 < 0 || j1 <= j0 || ldz < j1 || ldg < j1 || lds_ < N)
    return RPGP_EINVAL;
  if (N > 0x7fffffffLL) return RPGP_EINVAL;
  if (!workspace || workspace_bytes < rpgp_bilinear_grad_workspace_bytes(N, j1 - j0)) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int ns_max = bilinear_nsplit(N);          // the slab layout (and the workspace size) uses the upper bound
  int cps = (int)((N + ns_max - 1) / ns_max);
  cps = (cps + 63) / 64 * 64;
  // splits that actually own columns: rounding cps up to 64 can leave trailing splits empty, and an empty split's
  // workgroups return without writing their slab — the reduce must not read them
  const int ns = (int)((N + cps - 1) / cps);
  float *slabG = reinterpret_cast<float *>(workspace);
  float *slabS = slabG + (size_t)ns_max * N * 20;
  float *rowS = slabS + (size_t)ns_max * N;
  int first = 1;
  for (int j = j0; j < j1;) {
    const int jt = next_j_piece(j1 - j);
    int rc;
    switch (jt) {
      case 20: rc = launch_bilinear_dense<20>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 10: rc = launch_bilinear_dense<10>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 8: rc = launch_bilinear_dense<8>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 5: rc = launch_bilinear_dense<5>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 3: rc = launch_bilinear_dense<3>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 4: rc = launch_bilinear_dense<4>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      case 2: rc = launch_bilinear_dense<2>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
      default: rc = launch_bilinear_dense<1>(Z, S, slabG, slabS, (int)N, ldz, lds_, j, cps, ns, st); break;
    }
    if (rc) return rc;
    const size_t total = (size_t)N * (jt + 1);
    hipLaunchKernelGGL(bilinear_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slabG, slabS,
                       gZ, rowS, (int)N, jt, ldg, j, ns, -scale / kExp2Scale, first ? 0 : 1);
    rc = launch_status();
    if (rc) return rc;
    first = 0;
    j += jt;
  }
  hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(1024), 0, st, rowS, gscale, (int)N, 0.5f);
  return launch_status();
}

size_t rpgp_family_bilinear_grad_workspace_bytes(int64_t N, int ncols, int ncomp) {
  if (N <= 0 || ncols <= 0 || ncomp <= 0) return 0;
  const int ns = bilinear_nsplit(N);
  // slabG [ns][N][<=20] + slabC [ns][N][<=10] + rowC [N][ncomp]
  return ((size_t)ns * N * 30 + (size_t)N * ncomp) * sizeof(float);
}

// mode 0: S = L R^T + R L^T from N x T factors; mode 1: explicit symmetric S (N x N, row stride lds)
static int family_bilinear_common(const rpgp_family *fam, const float *Z, const float *L, const float *R,
                                  const float *S, int64_t lds_, float *gZ, float *gcomp, int64_t N, int ldz, int ldg,
                                  int T, float scale, void *workspace, size_t workspace_bytes, void *stream) {
  if (!Z || !gZ || !gcomp || N <= 0 || N > 0x7fffffffLL) return RPGP_EINVAL;
  int rc = family_check(fam, ldz, ldg);
  if (rc) return rc;
  const int J = fam->ncomp * fam->group, C = fam->ncomp;
  if (!workspace || workspace_bytes < rpgp_family_bilinear_grad_workspace_bytes(N, J, C)) return RPGP_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int ns_max = bilinear_nsplit(N);          // the slab layout (and the workspace size) uses the upper bound
  int cps = (int)((N + ns_max - 1) / ns_max);
  cps = (cps + 63) / 64 * 64;
  // splits that actually own columns: rounding cps up to 64 can leave trailing splits empty, and an empty split's
  // workgroups return without writing their slab — the reduce must not read them
  const int ns = (int)((N + cps - 1) / cps);
  float *slabG = reinterpret_cast<float *>(workspace);
  float *slabC = slabG + (size_t)ns_max * N * 20;
  float *rowC = slabC + (size_t)ns_max * N * 10;
  const float *wts = fam->weights;
  rc = with_family_policy(fam->kind, fam->group, [&](auto kf) -> int {
    using KF = decltype(kf);
    for (int j = 0; j < J;) {
      const int jt = family_piece<KF>(J - j);
      const int r2 = with_family_piece<KF>(jt, [&](auto jc) -> int {
        constexpr int JT = decltype(jc)::value;
        constexpr int NC = JT / KF::group;
        dim3 grid(ns, (unsigned)((N + 255) / 256));
        if (S) {
          hipLaunchKernelGGL((family_bilinear_dense_kernel<JT, KF>), grid, dim3(256), 0, st, Z, S, slabG, slabC, (int)N,
                             ldz, (long long)lds_, j, cps, wts);
        } else if (T <= 1) {
          hipLaunchKernelGGL((family_bilinear_kernel<JT, 1, KF>), grid, dim3(256), 0, st, Z, L, R, slabG, slabC, (int)N,
                             ldz, T, j, cps, wts);
        } else if (T <= 4) {
          hipLaunchKernelGGL((family_bilinear_kernel<JT, 4, KF>), grid, dim3(256), 0, st, Z, L, R, slabG, slabC, (int)N,
                             ldz, T, j, cps, wts);
        } else {
          hipLaunchKernelGGL((family_bilinear_kernel<JT, 12, KF>), grid, dim3(256), 0, st, Z, L, R, slabG, slabC, (int)N,
                             ldz, T, j, cps, wts);
        }
        int r3 = launch_status();
        if (r3) return r3;
        const size_t total = (size_t)N * (JT + NC);
        hipLaunchKernelGGL(family_bilinear_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slabG,
                           slabC, gZ, rowC, (int)N, JT, NC, ldg, j, j / KF::group, C, ns, scale * KF::mulG);
        return launch_status();
      });
      if (r2) return r2;
      j += jt;
    }
    return 0;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(sum_columns_kernel, dim3(C), dim3(1024), 0, st, rowC, gcomp, (int)N, C, 0.5f);
  return launch_status();
}

int rpgp_family_bilinear_grad(const rpgp_family *fam, const float *Z, const float *L, const float *R, float *gZ,
                              float *gcomp, int64_t N, int ldz, int ldg, int T, float scale, void *workspace,
                              size_t workspace_bytes, void *stream) {
  if (!L || !R || T <= 0 || T > 12) return RPGP_EINVAL;
  return family_bilinear_common(fam, Z, L, R, nullptr, 0, gZ, gcomp, N, ldz, ldg, T, scale, workspace, workspace_bytes,
                                stream);
}

int rpgp_family_bilinear_grad_dense(const rpgp_family *fam, const float *Z, const float *S, float *gZ, float *gcomp,
                                    int64_t N, int ldz, int ldg, int64_t lds_, float scale, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  if (!S || lds_ < N) return RPGP_EINVAL;
  return family_bilinear_common(fam, Z, nullptr, nullptr, S, lds_, gZ, gcomp, N, ldz, ldg, 0, scale, workspace,
                                workspace_bytes, stream);
}

}  // extern "C"
