// rpgp_pivchol.hip — the rank-k pivoted Cholesky preconditioner factor: the one-workgroup kernel, the per-step kernels
// (general, flagship fast, SKI fast), their dispatch (pivchol_common) and the rpgp_*pivoted_cholesky* entries of the C-ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stddef.h>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"
#include "rpgp_tile.h"

#include "rpgp_ski_common.h"   // ski_grid_of, ski_taps, ski_wj: the grid-interpolation rows of pivchol_step_kernel

namespace {

// ---------------------------------------------------------------------------------------------
// Rank-k pivoted Cholesky of K = scale * sum_j exp(-0.5 (z_ij - z_i'j)^2) (preconditioner) as ONE
// single-workgroup launch: k greedy steps of {argmax of the residual diagonal, one kernel row, rank-1 downdate}.
// L is N x k row-major (what the native mBCG executor consumes).  Work per step is O(N (J + k)): negligible next to
// one MVM, so a single CU is enough and no host round-trips are needed (the torch version costs ~10 launches/step).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pivchol_kernel(const float *__restrict__ Z, float *__restrict__ L,
                                                       float *__restrict__ dwork, int N, int ldz, int J, int k,
                                                       float scale) {
  __shared__ float sval[16];
  __shared__ int sidx[16];
  __shared__ float szp[64];
  __shared__ float slp[64];
  __shared__ float sdp;
  __shared__ int spiv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float d0 = scale * (float)J;
  for (int i = tid; i < N; i += 1024) dwork[i] = d0;
  __syncthreads();
  for (int m = 0; m < k; ++m) {
    // argmax of the residual diagonal (ties -> smallest index: deterministic)
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < N; i += 1024) {
      const float v = dwork[i];
      if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sval[wave] = bv; sidx[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      float v = sval[0];
      int ix = sidx[0];
      for (int w = 1; w < 16; ++w)
        if (sval[w] > v || (sval[w] == v && sidx[w] < ix)) { v = sval[w]; ix = sidx[w]; }
      sdp = v;
      spiv = ix;
    }
    __syncthreads();
    const int piv = spiv;
    const float dp = sdp;
    const bool ok = dp > 1e-10f * d0;
    if (tid < J) szp[tid] = Z[(size_t)piv * ldz + tid] * kExp2Scale;
    if (tid < m) slp[tid] = L[(size_t)piv * k + tid];
    __syncthreads();
    const float inv_sq = ok ? 1.0f / sqrtf(dp) : 0.f;
    for (int i = tid; i < N; i += 1024) {
      float l = 0.f;
      if (ok) {
        float row = 0.f;
        for (int j = 0; j < J; ++j) {
          const float dd = Z[(size_t)i * ldz + j] * kExp2Scale - szp[j];
          row += fast_exp2(-(dd * dd));
        }
        row *= scale;
        float corr = 0.f;
        for (int q = 0; q < m; ++q) corr = __builtin_fmaf(L[(size_t)i * k + q], slp[q], corr);
        l = (row - corr) * inv_sq;
      }
      L[(size_t)i * k + m] = l;
      float nd = dwork[i] - l * l;
      nd = nd < 0.f ? 0.f : nd;
      dwork[i] = (i == piv) ? 0.f : nd;
    }
    __syncthreads();
  }
}

// Multi-workgroup form for N > 2048: one launch per greedy step.  The launch of step m first reduces the per-workgroup
// argmax partials left by step m-1 (every workgroup redundantly, same fixed order -> same pivot everywhere), then
// evaluates the pivot's kernel row on its own rows, writes column m of L, downdates the residual diagonal and leaves
// its argmax partial for step m+1 (ping-pong buffers).  k + 1 launches spread over the whole chip instead of one CU:
// 6.5 ms -> ~0.3 ms at N = 50k.  The entry K(i, piv) is evaluated by a runtime-shaped routine that also covers the other
// family members (kind / group / per-component weights; the hot path is kind RBF, group 1, unit weights).
__device__ __forceinline__ float pivchol_entry(const float *__restrict__ zi, const float *__restrict__ szp, int kind,
                                               int group, int ncomp, const float *__restrict__ wts) {
  float acc = 0.f;
  for (int c = 0; c < ncomp; ++c) {
    float phi;
    if (kind == RPGP_KIND_RBF) {
      float r2 = 0.f;
      for (int q = 0; q < group; ++q) {
        const float dd = zi[c * group + q] * kExp2Scale - szp[c * group + q];
        r2 = __builtin_fmaf(dd, dd, r2);
      }
      phi = fast_exp2(-r2);
    } else if (kind == RPGP_KIND_MATERN15) {
      phi = Phi<RPGP_KIND_MATERN15>::val(zi[c] * Phi<RPGP_KIND_MATERN15>::pre - szp[c]);
    } else if (kind == RPGP_KIND_IMQ) {
      phi = Phi<RPGP_KIND_IMQ>::val(zi[c] * Phi<RPGP_KIND_IMQ>::pre - szp[c]);
    } else {
      phi = Phi<RPGP_KIND_COSINE>::val(zi[c] * Phi<RPGP_KIND_COSINE>::pre - szp[c]);
    }
    acc = wts ? __builtin_fmaf(wts[c], phi, acc) : acc + phi;
  }
  return acc;
}

__device__ __forceinline__ float pivchol_pre(int kind) {
  return kind == RPGP_KIND_RBF ? kExp2Scale
                               : (kind == RPGP_KIND_MATERN15 ? Phi<RPGP_KIND_MATERN15>::pre
                                                             : (kind == RPGP_KIND_IMQ ? Phi<RPGP_KIND_IMQ>::pre
                                                                                      : Phi<RPGP_KIND_COSINE>::pre));
}

// block-wide argmax (ties -> smallest index); result valid in thread 0
__device__ __forceinline__ void block_argmax(float &bv, int &bi, float *sval, int *sidx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sval[wave] = bv; sidx[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
      if (sval[w] > bv || (sval[w] == bv && sidx[w] < bi)) { bv = sval[w]; bi = sidx[w]; }
  }
}

// argmax partials of an already filled residual diagonal (SKI: the diagonal is not constant)
__global__ __launch_bounds__(256) void pivchol_init_from_diag_kernel(const float *__restrict__ dwork,
                                                                     float *__restrict__ pval, int *__restrict__ pidx,
                                                                     int N) {
  __shared__ float sval[4];
  __shared__ int sidx[4];
  float bv = -1.f;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    const float v = dwork[i];
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
  }
  block_argmax(bv, bi, sval, sidx);
  if (threadIdx.x == 0) {
    pval[blockIdx.x] = bv;
    pidx[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(256) void pivchol_step_kernel(const float *__restrict__ Z, float *__restrict__ L,
                                                           float *__restrict__ dwork, const float *__restrict__ pval_in,
                                                           const int *__restrict__ pidx_in, float *__restrict__ pval_out,
                                                           int *__restrict__ pidx_out, int nparts, int N, int ldz,
                                                           int ncols, int k, int m, float scale, float d0, int kind,
                                                           int group, int ncomp, const float *__restrict__ wts,
                                                           const float *__restrict__ gp, int G, int const_diag = 0,
                                                           float *__restrict__ Lt = nullptr) {
  // Lt (rank x N, optional): the factor is kept COLUMN-major while it is built — a row of the N x k factor is 4 k bytes, so
  // the correction sum below reads every 64-byte line of it whatever m is and the new column is one 4-byte store per line;
  // column-major, step m reads m coalesced vectors and writes one.  L is then written once at the end (pivchol_untranspose).
  __shared__ float sval[4];
  __shared__ int sidx[4];
  __shared__ float szp[64];
  __shared__ float slp[64];
  __shared__ float spw[64][4];     // SKI mode (gp != nullptr): the pivot's interpolation weights / first tap per column
  __shared__ int spidx[64];
  __shared__ float sdp;
  __shared__ int spiv;
  // pivot of this step from the previous launch's partials; const_diag (step 0 of a stationary kernel): the residual diagonal
  // is d0 everywhere and the first pivot is row 0 (ties -> smallest index) — no initialisation launch, no partials to read
  float bv = -1.f;
  int bi = 0x7fffffff;
  if (const_diag) {
    if (threadIdx.x == 0) { sdp = d0; spiv = 0; }
  } else {
    for (int q = threadIdx.x; q < nparts; q += 256) {
      const float v = pval_in[q];
      const int ix = pidx_in[q];
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    block_argmax(bv, bi, sval, sidx);
    if (threadIdx.x == 0) { sdp = bv; spiv = bi; }
  }
  __syncthreads();
  const int piv = spiv;
  const float dp = sdp;
  const bool ok = dp > 1e-10f * d0;
  const float pre = pivchol_pre(kind);
  if ((int)threadIdx.x < ncols) {
    const float zp = Z[(size_t)piv * ldz + threadIdx.x];
    szp[threadIdx.x] = zp * pre;
    if (gp) {
      float w[4], dw[4];
      const float *gj = ski_grid_of(gp, ncols, threadIdx.x);
      spidx[threadIdx.x] = ski_taps<false>(zp, gj[0], gj[2], G, w, dw);
#pragma unroll
      for (int q = 0; q < 4; ++q) spw[threadIdx.x][q] = w[q];
    }
  }
  if ((int)threadIdx.x < m)
    slp[threadIdx.x] = Lt ? Lt[(size_t)threadIdx.x * N + piv] : L[(size_t)piv * k + threadIdx.x];
  __syncthreads();
  const float inv_sq = ok ? 1.0f / sqrtf(dp) : 0.f;
  bv = -1.f;
  bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    float l = 0.f;
    if (ok) {
      float row;
      if (gp) {
        // K_ski(i, piv) = sum_j sum_{q,q'} w_q(z_ij) w_q'(z_pj) Toep[(idx_i + q) - (idx_p + q')]: 7 distinct lags per column
        float acc = 0.f;
        for (int j = 0; j < ncols; ++j) {
          float w[4], dw[4];
          const float *gj = ski_grid_of(gp, ncols, j);
          const int idx = ski_taps<false>(Z[(size_t)i * ldz + j], gj[0], gj[2], G, w, dw);
          const int delta = idx - spidx[j];
          float tl[7];
#pragma unroll
          for (int u = 0; u < 7; ++u) {
            const int lag = delta + u - 3;            // (the sub-kernel of the grid block: RBF unless flags say otherwise)
            tl[u] = ski_radial_f32(ski_kind(gp), lag < 0 ? -lag : lag, gj[1]);
          }
          float aj = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) aj = __builtin_fmaf(w[q] * spw[j][qq], tl[q - qq + 3], aj);
          acc = __builtin_fmaf(ski_wj(gp, j), aj, acc);
        }
        row = scale * acc;
      } else {
        row = scale * pivchol_entry(Z + (size_t)i * ldz, szp, kind, group, ncomp, wts);
      }
      float corr = 0.f;
      if (Lt) {
        for (int q = 0; q < m; ++q) corr = __builtin_fmaf(Lt[(size_t)q * N + i], slp[q], corr);
      } else {
        for (int q = 0; q < m; ++q) corr = __builtin_fmaf(L[(size_t)i * k + q], slp[q], corr);
      }
      l = (row - corr) * inv_sq;
    }
    if (Lt) Lt[(size_t)m * N + i] = l;
    else L[(size_t)i * k + m] = l;
    float nd = (const_diag ? d0 : dwork[i]) - l * l;
    nd = nd < 0.f ? 0.f : nd;
    nd = (i == piv) ? 0.f : nd;
    dwork[i] = nd;
    if (nd > bv || (nd == bv && i < bi)) { bv = nd; bi = i; }
  }
  __syncthreads();
  block_argmax(bv, bi, sval, sidx);
  if (threadIdx.x == 0) {
    pval_out[blockIdx.x] = bv;
    pidx_out[blockIdx.x] = bi;
  }
}

// The grid-interpolation operator's step with few projections (the C5 shape: J = 3), one row per thread, the factor column-major:
// as in pivchol_step_fast_kernel below, what does not depend on the pivot — the thread's coordinates and with them its taps
// and weights, its residual diagonal entry, its entries of the factor's first m columns — is requested at the head of the kernel
// and lands while the pivot is being found.  Same arithmetic in the same order as pivchol_step_kernel.
__global__ __launch_bounds__(256) void pivchol_step_ski_fast_kernel(const float *__restrict__ Z, float *__restrict__ dwork,
                                                                    const float *__restrict__ pval_in,
                                                                    const int *__restrict__ pidx_in,
                                                                    float *__restrict__ pval_out, int *__restrict__ pidx_out,
                                                                    int nparts, int N, int ldz, int ncols, int m, float scale,
                                                                    float d0, const float *__restrict__ gp, int G,
                                                                    float *__restrict__ Lt) {
  __shared__ float sval[4];
  __shared__ int sidx[4];
  __shared__ float slp[16];
  __shared__ float spw[4][4];
  __shared__ int spidx[4];
  __shared__ float sdp;
  __shared__ int spiv;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const bool own = i < N;
  const int ic = own ? i : N - 1;
  // the partials of the previous step (nparts <= 2 048: eight per thread, clamped, always loaded)
  float pv[8];
  int pi[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int q = tid + 256 * u;
    const int qc = q < nparts ? q : nparts - 1;
    pv[u] = pval_in[qc];
    pi[u] = pidx_in[qc];
  }
  // own-row operands
  float zr[4], lr[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) zr[j] = Z[(size_t)ic * ldz + (j < ncols ? j : ncols - 1)];
#pragma unroll
  for (int q = 0; q < 16; ++q) lr[q] = Lt[(size_t)(q < m ? q : 0) * N + ic];
  const float dprev = dwork[ic];
  const int kind = ski_kind(gp);
  float ow[4][4], ohs[4], owj[4];
  int oidx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float dw[4];
    const float *gj = ski_grid_of(gp, ncols, j < ncols ? j : ncols - 1);
    oidx[j] = ski_taps<false>(zr[j], gj[0], gj[2], G, ow[j], dw);
    ohs[j] = gj[1];
    owj[j] = ski_wj(gp, j < ncols ? j : ncols - 1);
  }
  float bv = -1.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int q = tid + 256 * u;
    if (q < nparts && (pv[u] > bv || (pv[u] == bv && pi[u] < bi))) { bv = pv[u]; bi = pi[u]; }
  }
  block_argmax(bv, bi, sval, sidx);
  if (tid == 0) { sdp = bv; spiv = bi; }
  __syncthreads();
  const int piv = spiv;
  const float dp = sdp;
  const bool ok = dp > 1e-10f * d0;
  if (tid < ncols) {
    const float zp = Z[(size_t)piv * ldz + tid];
    float w[4], dw[4];
    const float *gj = ski_grid_of(gp, ncols, tid);
    spidx[tid] = ski_taps<false>(zp, gj[0], gj[2], G, w, dw);
#pragma unroll
    for (int q = 0; q < 4; ++q) spw[tid][q] = w[q];
  }
  if (tid < m) slp[tid] = Lt[(size_t)tid * N + piv];
  __syncthreads();
  const float inv_sq = ok ? 1.0f / sqrtf(dp) : 0.f;
  bv = -1.f;
  bi = 0x7fffffff;
  if (own) {
    float l = 0.f;
    if (ok) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < ncols) {
          const int delta = oidx[j] - spidx[j];
          float tl[7];
#pragma unroll
          for (int u = 0; u < 7; ++u) {
            const int lag = delta + u - 3;
            tl[u] = ski_radial_f32(kind, lag < 0 ? -lag : lag, ohs[j]);
          }
          float aj = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) aj = __builtin_fmaf(ow[j][q] * spw[j][qq], tl[q - qq + 3], aj);
          acc = __builtin_fmaf(owj[j], aj, acc);
        }
      }
      const float row = scale * acc;
      float corr = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < m) corr = __builtin_fmaf(lr[q], slp[q], corr);
      l = (row - corr) * inv_sq;
    }
    Lt[(size_t)m * N + i] = l;
    float nd = dprev - l * l;
    nd = nd < 0.f ? 0.f : nd;
    nd = (i == piv) ? 0.f : nd;
    dwork[i] = nd;
    bv = nd;
    bi = i;
  }
  __syncthreads();
  block_argmax(bv, bi, sval, sidx);
  if (tid == 0) {
    pval_out[blockIdx.x] = bv;
    pidx_out[blockIdx.x] = bi;
  }
}

// L (N x k, row-major) from the column-major scratch the steps filled: a workgroup owns 256 consecutive rows, reads 16
// coalesced vectors at a time into LDS and writes them as 64-byte runs of its rows.
__global__ __launch_bounds__(256) void pivchol_untranspose_kernel(const float *__restrict__ Lt, float *__restrict__ L, int N,
                                                                  int k) {
  __shared__ float tile[16 * 257];
  const int r0 = blockIdx.x * 256;
  const int rows = (N - r0 < 256) ? N - r0 : 256;
  const int i = r0 + threadIdx.x;
  const int ic = i < N ? i : N - 1;
  for (int q0 = 0; q0 < k; q0 += 16) {
    const int cw = (k - q0 < 16) ? k - q0 : 16;
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = Lt[(size_t)(q0 + (q < cw ? q : cw - 1)) * N + ic];       // 16 loads in flight
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) tile[q * 257 + threadIdx.x] = v[q];
    __syncthreads();
    for (int e = threadIdx.x; e < rows * cw; e += 256) {
      const int r = e / cw, q = e - r * cw;
      L[(size_t)(r0 + r) * k + q0 + q] = tile[q * 257 + r];
    }
  }
}

// Fast path of the per-step form for the flagship operator (plain RBF projections, <= 32 columns, rank <= 16, one row per
// thread: N <= 131072).  A greedy step is a chain of dependent round trips — argmax partials -> pivot -> the pivot's row ->
// this thread's own row -> entry — of which the LAST operands do not depend on the pivot at all: the thread's coordinates,
// its row of L and its residual diagonal entry are requested at the head of the kernel, behind the partials, and land while
// the pivot is being found.  Same arithmetic in the same order as pivchol_step_kernel (padded terms add exact zeros).
__global__ __launch_bounds__(256) void pivchol_step_fast_kernel(const float *__restrict__ Z, float *__restrict__ L,
                                                                float *__restrict__ dwork,
                                                                const float *__restrict__ pval_in,
                                                                const int *__restrict__ pidx_in,
                                                                float *__restrict__ pval_out, int *__restrict__ pidx_out,
                                                                int nparts, int N, int ldz, int ncols, int k, int m,
                                                                float scale, float d0, int const_diag) {
  __shared__ float sval[4];
  __shared__ int sidx[4];
  __shared__ float szp[32];
  __shared__ float slp[16];
  __shared__ float sdp;
  __shared__ int spiv;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const bool own = i < N;
  const size_t ic = (size_t)(own ? i : N - 1);
  float pv[2];
  int pi[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {                     // (nparts <= 512; clamped, always loaded)
    const int q = tid + 256 * u;
    const int qc = q < nparts ? q : nparts - 1;
    pv[u] = const_diag ? -1.f : pval_in[qc];
    pi[u] = const_diag ? 0x7fffffff : pidx_in[qc];
  }
  float zr[32], lr[16];
#pragma unroll
  for (int j = 0; j < 32; ++j) zr[j] = Z[ic * ldz + (j < ncols ? j : ncols - 1)];
#pragma unroll
  for (int q = 0; q < 16; ++q) lr[q] = L[ic * k + (q < k ? q : k - 1)];
  const float dprev = const_diag ? d0 : dwork[ic];
  float bv = -1.f;
  int bi = 0x7fffffff;
  if (const_diag) {
    if (tid == 0) { sdp = d0; spiv = 0; }
  } else {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = tid + 256 * u;
      if (q < nparts && (pv[u] > bv || (pv[u] == bv && pi[u] < bi))) { bv = pv[u]; bi = pi[u]; }
    }
    block_argmax(bv, bi, sval, sidx);
    if (tid == 0) { sdp = bv; spiv = bi; }
  }
  __syncthreads();
  const int piv = spiv;
  const float dp = sdp;
  const bool ok = dp > 1e-10f * d0;
  if (tid < ncols) szp[tid] = Z[(size_t)piv * ldz + tid] * kExp2Scale;
  if (tid < m) slp[tid] = L[(size_t)piv * k + tid];
  __syncthreads();
  const float inv_sq = ok ? 1.0f / sqrtf(dp) : 0.f;
  bv = -1.f;
  bi = 0x7fffffff;
  if (own) {
    float l = 0.f;
    if (ok) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        if (j < ncols) {
          const float dd = zr[j] * kExp2Scale - szp[j];
          float r2 = 0.f;
          r2 = __builtin_fmaf(dd, dd, r2);
          acc = acc + fast_exp2(-r2);
        }
      }
      const float row = scale * acc;
      float corr = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < m) corr = __builtin_fmaf(lr[q], slp[q], corr);
      l = (row - corr) * inv_sq;
    }
    L[(size_t)i * k + m] = l;
    float nd = dprev - l * l;
    nd = nd < 0.f ? 0.f : nd;
    nd = (i == piv) ? 0.f : nd;
    dwork[i] = nd;
    bv = nd;
    bi = i;
  }
  __syncthreads();
  block_argmax(bv, bi, sval, sidx);
  if (tid == 0) {
    pval_out[blockIdx.x] = bv;
    pidx_out[blockIdx.x] = bi;
  }
}

}  // namespace

extern "C" {

// diag_work: N + kPivcholScratch floats (residual diagonal + argmax partials of the multi-workgroup form)
static int pivchol_common(const float *Z, float *L, float *diag_work, int64_t N, int ldz, int ncols, int rank,
                          float scale, float d0, int kind, int group, int ncomp, const float *wts, void *stream,
                          const float *gp = nullptr, int G = 0, float *Lt = nullptr) {
  hipStream_t st = as_stream(stream);
  if (N <= 2048 && kind == RPGP_KIND_RBF && group == 1 && !wts && !gp) {      // launch-latency regime: one workgroup
    hipLaunchKernelGGL(pivchol_kernel, dim3(1), dim3(1024), 0, st, Z, L, diag_work, (int)N, ldz, ncols, rank, scale);
    return launch_status();
  }
  // (all greedy steps as ONE cooperative launch with grid barriers was built in round 5 and measured no faster than the
  //  per-step launches — a grid barrier ~8 us against a 1.5 - 2 us launch boundary: tools/experiments/r6_removed_forms.patch)
  int nb = (int)((N + 255) / 256);
  // up to 2 048 workgroups: one row per thread up to N = 524 288.  (A cap of 512 made a thread of the C5 operator walk three
  // rows one after the other at two waves per SIMD — a chain of dependent global round trips per row, 14 us per step with
  // nothing to read from the factor yet.)
  constexpr int kMaxParts = RPGP_PIVCHOL_SCRATCH / 4;
  if (nb > kMaxParts) nb = kMaxParts;
  float *pval[2] = {diag_work + N, diag_work + N + kMaxParts};
  int *pidx[2] = {reinterpret_cast<int *>(diag_work + N + 2 * kMaxParts), reinterpret_cast<int *>(diag_work + N + 3 * kMaxParts)};
  if (gp) {    // SKI: the residual diagonal starts at diag(K_ski), which depends on the point
    const int drc = rpgp_ski_diag(Z, gp, diag_work, N, ldz, ncols, G, scale, stream);       // (rpgp_ski_base.hip)
    if (drc) return drc;
    hipLaunchKernelGGL(pivchol_init_from_diag_kernel, dim3(nb), dim3(256), 0, st, diag_work, pval[0], pidx[0], (int)N);
  }
  // (a stationary kernel's residual diagonal starts at d0 everywhere: step 0 knows that itself — no initialisation launch)
  // the flagship operator's fast per-step kernel (own-row operands requested before the pivot is known); every other operator,
  // wide coordinate rows and ranks beyond 16 take the general per-step kernel
  const bool fast = kind == RPGP_KIND_RBF && group == 1 && !wts && !gp && ncols <= 32 &&
                    rank <= 16 && N <= 131072;
  for (int m = 0; fast && m < rank; ++m)
    hipLaunchKernelGGL(pivchol_step_fast_kernel, dim3(nb), dim3(256), 0, st, Z, L, diag_work, pval[m & 1], pidx[m & 1],
                       pval[(m + 1) & 1], pidx[(m + 1) & 1], nb, (int)N, ldz, ncols, rank, m, scale, d0, m == 0 ? 1 : 0);
  if (fast) return launch_status();
  // grid interpolation with few projections, one row per thread, column-major factor: own-row operands requested up front
  const bool ski_fast = gp && Lt && ncols <= 4 && rank <= 16 && (long long)nb * 256 >= N && !wts;
  for (int m = 0; ski_fast && m < rank; ++m)
    hipLaunchKernelGGL(pivchol_step_ski_fast_kernel, dim3(nb), dim3(256), 0, st, Z, diag_work, pval[m & 1], pidx[m & 1],
                       pval[(m + 1) & 1], pidx[(m + 1) & 1], nb, (int)N, ldz, ncols, m, scale, d0, gp, G, Lt);
  for (int m = ski_fast ? rank : 0; m < rank; ++m) {
    hipLaunchKernelGGL(pivchol_step_kernel, dim3(nb), dim3(256), 0, st, Z, L, diag_work, pval[m & 1], pidx[m & 1],
                       pval[(m + 1) & 1], pidx[(m + 1) & 1], nb, (int)N, ldz, ncols, rank, m, scale, d0, kind, group,
                       ncomp, wts, gp, G, (m == 0 && !gp) ? 1 : 0, Lt);
  }
  if (Lt)
    hipLaunchKernelGGL(pivchol_untranspose_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, Lt, L, (int)N, rank);
  return launch_status();
}

int rpgp_pivoted_cholesky(const float *Z, float *L, float *diag_work, int64_t N, int ldz, int J, int rank, float scale,
                          void *stream) {
  if (!Z || !L || !diag_work || N <= 0 || J <= 0 || J > 64 || rank <= 0 || rank > 64 || ldz < J || N > 0x7fffffffLL)
    return RPGP_EINVAL;
  return pivchol_common(Z, L, diag_work, N, ldz, J, rank, scale, scale * (float)J, RPGP_KIND_RBF, 1, J, nullptr, stream);
}

// the SKI factor is built column-major from this size on (below it the factor sits in L2 and the row-major form is as fast)
static const int64_t kPivcholColumnMajorMin = 65536;

size_t rpgp_ski_pivoted_cholesky_work_floats(int64_t N, int rank) {
  if (N <= 0 || rank <= 0) return 0;
  return (size_t)N + RPGP_PIVCHOL_SCRATCH + (N >= kPivcholColumnMajorMin ? (size_t)N * (size_t)rank : 0);
}

int rpgp_ski_pivoted_cholesky(const float *Z, const float *grid_params, float *L, float *diag_work, size_t diag_work_floats,
                              int64_t N, int ldz, int J, int G, int rank, float scale, void *stream) {
  if (!Z || !grid_params || !L || !diag_work || N <= 0 || J <= 0 || J > 64 || G < 8 || rank <= 0 || rank > 64 ||
      ldz < J || N > 0x7fffffffLL)
    return RPGP_EINVAL;
  if (diag_work_floats < rpgp_ski_pivoted_cholesky_work_floats(N, rank)) return RPGP_EWORKSPACE;
  float *Lt = N >= kPivcholColumnMajorMin ? diag_work + N + RPGP_PIVCHOL_SCRATCH : nullptr;
  return pivchol_common(Z, L, diag_work, N, ldz, J, rank, scale, scale * (float)J, RPGP_KIND_RBF, 1, J, nullptr, stream,
                        grid_params, G, Lt);
}

int rpgp_family_pivoted_cholesky(const rpgp_family *fam, const float *Z, float *L, float *diag_work, int64_t N,
                                 int ldz, int rank, float scale, float weight_sum, void *stream) {
  if (!Z || !L || !diag_work || N <= 0 || rank <= 0 || rank > 64 || N > 0x7fffffffLL) return RPGP_EINVAL;
  const int rc = family_check(fam, ldz, ldz);
  if (rc) return rc;
  const int ncols = fam->ncomp * fam->group;
  if (ncols > 64) return RPGP_EINVAL;
  return pivchol_common(Z, L, diag_work, N, ldz, ncols, rank, scale, scale * weight_sum, fam->kind, fam->group,
                        fam->ncomp, fam->weights, stream);
}

}  // extern "C"
