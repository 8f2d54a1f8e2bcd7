// rpgp_dense_mvm.hip — the cached-K mode: out = Kd V + noise V for a dense N x N fp32 matrix in HBM (MFMA GEMM for wide
// blocks, VALU GEMV for T <= 12), their slab reduces and rpgp_dense_mvm of the C-ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stddef.h>
#include <atomic>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"
#include "rpgp_tile.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Cached-K mode: out = Kd @ V + noise V for a dense N x N fp32 matrix in HBM and a thin block V (T <= 16 columns per
// pass).  HBM-bound stream of Kd; the multiply-accumulate runs on the matrix cores (v_mfma_f32_16x16x4_f32, exact
// fp32) so the VALU only issues loads.  A 256-thread workgroup owns 128 rows (32 per wave = two 16-row MFMA tiles);
// V is staged 256 rows at a time in LDS and shared by the four waves.
//   A tile: lane (m = l%16, q = l/16) loads float4 Kd[row0+m][c + 4q .. 4q+3]; MFMA i uses component i with
//   B_i[q][n] = V[c + 4q + i][n]  (any consistent ordering of the K dimension is valid);
//   D: lane holds out[row0 + 4*(l/16) + r][l%16], r = 0..3.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_gemm_kernel(const float *__restrict__ Kd, const float *__restrict__ V,
                                                         float *__restrict__ slab, int N, long long ldk, int T, int t0,
                                                         int tcnt, int rows_per_split) {
  // Kd is symmetric, so out[c][t] = sum_r Kd[r][c] V[r][t]: every wave owns 64 consecutive OUTPUT indices c and
  // streams down the rows r of Kd, 4 rows per step.  Lane (k = l/16, n = l%16) loads float4 Kd[r+k][c0 + 4n .. 4n+3]
  // (256 contiguous bytes per row per wave-instruction) and feeds its 4 components to 4 MFMAs:
  //   D_i[t][n] += sum_k V[r+k][t] * Kd[r+k][c0 + 4n + i]        (A: lane (t = l%16, k = l/16) holds V[r+k][t])
  constexpr int VC = 256;                        // V rows staged per step
  __shared__ float sV[VC * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, k = lane >> 4;
  const int c0 = blockIdx.x * 256 + wave * 64;   // first output index of this wave
  const int cl = c0 + 4 * n;                     // this lane's 4 columns
  // (padded rows: the last column group's 16-byte load may reach into the row's own padding — those values only feed
  // output columns >= N, which are not stored)
  const bool vec_ok = ((ldk & 3) == 0) && ((((uintptr_t)Kd) & 15) == 0) && cl < N && (cl + 3 < ldk);
  floatx4m acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = floatx4m{0.f, 0.f, 0.f, 0.f};
  const int rs = blockIdx.y * rows_per_split;
  const int re = (rs + rows_per_split < N) ? rs + rows_per_split : N;
  for (int rb = rs; rb < re; rb += VC) {
    __syncthreads();
    for (int e = tid; e < VC * 16; e += 256) {
      const int rr = e >> 4, t = e & 15;
      const int row = rb + rr;
      sV[e] = (row < re && t < tcnt) ? V[(size_t)row * T + t0 + t] : 0.f;
    }
    __syncthreads();
    const int rend = (rb + VC < re) ? VC : re - rb;
#pragma unroll 4
    for (int rr = 0; rr < rend; rr += 4) {
      const int row = rb + rr + k;
      float4v a = {0.f, 0.f, 0.f, 0.f};
      if (row < re) {
        const float *kp = Kd + (size_t)row * ldk + cl;
        if (vec_ok) {
          a = __builtin_nontemporal_load(reinterpret_cast<const float4v *>(kp));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cl + i < N) a[i] = kp[i];
        }
      }
      const float v = sV[(rr + k) * 16 + n];     // A operand: V[row][t = n] for k = l/16 (zero beyond the split)
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, a.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, a.y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, a.z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, a.w, acc[3], 0, 0, 0);
    }
  }
  // D_i: lane holds out^T[t = 4k + r][c = c0 + 4n + i]
  float *sl = slab + (size_t)blockIdx.y * N * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = cl + i;
    if (c < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sl[(size_t)c * 16 + 4 * k + r] = acc[i][r];
    }
  }
}

// VALU form for T <= 12: the padded 16-column MFMA above spends 128 matrix-pipe cycles per KB of Kd per SIMD — as much
// as HBM allows a SIMD to receive (1 KB / 132 clk at 8 TB/s), so it cannot overlap its way to the HBM roofline.  Here a
// wave owns 256 output columns (lane = 4 consecutive columns) and streams down the rows of the symmetric Kd: every
// wave-instruction loads ONE contiguous KB of a row (perfectly coalesced), V[row][0..T) is wave-uniform (scalar loads,
// SGPR multiplier), and the update is 4 T v_fma_f32 per lane (8.8 T cycles per KB).  Split-K slabs + the same
// fixed-order reduce as the MFMA form.
// The workgroup owns 256 columns and its four waves take alternate 8-row batches of the split's rows; their accumulators
// are added through LDS in a fixed order ((w0 + w2) + (w1 + w3)) before ONE slab record is written.  (Four waves side by
// side on 1024 columns, each writing its own slab record, needed 4x the slabs for the same number of resident waves: at
// N = 15k, T = 11 the slab write burst and its re-read by the reduce were a quarter of the product's time; the split form
// is faster at every size measured, 4k <= N <= 50k — profiles/r2_gemv_wave_split_sweep.txt.)
template <int TT>
__global__ __launch_bounds__(256) void dense_gemv_valu_kernel(const float *__restrict__ Kd, const float *__restrict__ V,
                                                              float *__restrict__ slab, int N, long long ldk,
                                                              int rows_per_split) {
  // TT is the EXACT number of right-hand sides (V is N x TT, row-major): the V loads are unconditional wave-uniform
  // scalar loads that hipcc merges into s_load_dwordx4/x8, and the row loop is branch-free.  (The first version
  // guarded every load with `t < T` / per-lane alignment tests: one branch per load, 2.4 TB/s at N = 15k.)
  __shared__ float4v sRed[2 * TT * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // SGPR: keeps the V row pointer scalar
  const int cl = blockIdx.x * 256 + 4 * lane;                      // this lane's 4 output columns
  const bool base_ok = ((ldk & 3) == 0) && ((((uintptr_t)Kd) & 15) == 0);
  float acc[4][TT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;
  const int rs = blockIdx.y * rows_per_split;
  const int re = (rs + rows_per_split < N) ? rs + rows_per_split : N;
  constexpr int RB = 8;
  constexpr int WSTEP = 4;                        // batches between two of a wave's own
  const int wfirst = wave;
  // The 16-byte path also serves the ragged right edge when the rows are padded (cl + 3 < ldk: the pad belongs to the
  // row's own allocation; what it holds only reaches accumulators of columns >= N, which are never stored).  Sending
  // those lanes down the element-wise path made one wave per split walk its rows one dependent load at a time — at
  // N = 14 939 (N % 4 = 3) that straggler set the whole kernel's time: 208 us against 143 us for T = 11.
  if (base_ok && cl < N && cl + 3 < ldk) {
    // batches of 8 rows: 8 x 16 B per lane in flight before the first FMA (the bytes in flight per CU come from the depth
    // of each thread's own load queue).  A rolling form that re-requests row q of the next batch right after row q's FMAs
    // (sched_barrier-pinned) measured no better at any size and cost 28 VGPRs.
    int row = rs + wfirst * RB;
    const float *kp = Kd + (size_t)row * ldk + cl;
    const float *vp = V + (size_t)row * TT;
    for (; row + RB <= re; row += WSTEP * RB) {
      float4v a[RB];
#pragma unroll
      for (int q = 0; q < RB; ++q) a[q] = __builtin_nontemporal_load(reinterpret_cast<const float4v *>(kp + (size_t)q * ldk));
#pragma unroll
      for (int q = 0; q < RB; ++q) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const float v = vp[q * TT + t];                         // wave-uniform address: scalar load
          acc[0][t] = __builtin_fmaf(a[q].x, v, acc[0][t]);
          acc[1][t] = __builtin_fmaf(a[q].y, v, acc[1][t]);
          acc[2][t] = __builtin_fmaf(a[q].z, v, acc[2][t]);
          acc[3][t] = __builtin_fmaf(a[q].w, v, acc[3][t]);
        }
      }
      kp += (size_t)WSTEP * RB * ldk;
      vp += WSTEP * RB * TT;
    }
    // the ragged last rows of the last split (fewer than 8): the wave whose batch they would have started
    if (row < re) {
      for (; row < re; ++row) {
        const float4v a = __builtin_nontemporal_load(reinterpret_cast<const float4v *>(kp));
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const float v = vp[t];
          acc[0][t] = __builtin_fmaf(a.x, v, acc[0][t]);
          acc[1][t] = __builtin_fmaf(a.y, v, acc[1][t]);
          acc[2][t] = __builtin_fmaf(a.z, v, acc[2][t]);
          acc[3][t] = __builtin_fmaf(a.w, v, acc[3][t]);
        }
        kp += ldk;
        vp += TT;
      }
    }
  } else if (cl < N) {
    // unaligned matrix (or an unpadded ragged right edge): element-wise loads
    for (int row = rs + wfirst; row < re; row += WSTEP) {
      const float *kp = Kd + (size_t)row * ldk + cl;
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = (cl + i < N) ? kp[i] : 0.f;
      const float *vp = V + (size_t)row * TT;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float v = vp[t];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][t] = __builtin_fmaf(a[i], v, acc[i][t]);
      }
    }
  }
  {
    if (wave >= 2) {
#pragma unroll
      for (int t = 0; t < TT; ++t) sRed[((wave - 2) * TT + t) * 64 + lane] = float4v{acc[0][t], acc[1][t], acc[2][t], acc[3][t]};
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float4v x = sRed[(wave * TT + t) * 64 + lane];
        acc[0][t] += x.x; acc[1][t] += x.y; acc[2][t] += x.z; acc[3][t] += x.w;
      }
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
      for (int t = 0; t < TT; ++t) sRed[t * 64 + lane] = float4v{acc[0][t], acc[1][t], acc[2][t], acc[3][t]};
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float4v x = sRed[t * 64 + lane];
      acc[0][t] += x.x; acc[1][t] += x.y; acc[2][t] += x.z; acc[3][t] += x.w;
    }
  }
  // compact slab, column-fastest: [split][t][Npad] — a lane's 4 columns are one 16-byte store per t and a wave's store
  // is one contiguous KB (the [column][t] layout scattered 44 dword stores per lane: 14 M partial-line writes per
  // product at N = 15k)
  const size_t npad = ((size_t)N + 3) & ~(size_t)3;
  float *sl = slab + (size_t)blockIdx.y * npad * TT;
  if (cl + 3 < N) {
#pragma unroll
    for (int t = 0; t < TT; ++t)
      *reinterpret_cast<float4v *>(sl + (size_t)t * npad + cl) = float4v{acc[0][t], acc[1][t], acc[2][t], acc[3][t]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = cl + i;
      if (c < N) {
#pragma unroll
        for (int t = 0; t < TT; ++t) sl[(size_t)t * npad + c] = acc[i][t];
      }
    }
  }
}

// out[row][t0+n] = sum_split slab[split][row][n] + noise * V[row][t0+n]   (fixed order: deterministic)
// `sw` = slab width (floats per (split, row)): 16 for the MFMA form, the exact T for the VALU form.
// A workgroup owns 32 consecutive slab entries; its 8 thread groups split the row-split slabs (slab s goes to group
// s % 8, 4 loads in flight per thread) and the 8 partial sums are added in a fixed order — deterministic.  (One thread
// per entry looping over ~100 slabs took 18-33 us: a third of the whole cached-K product at N = 7k.)
__global__ __launch_bounds__(256) void dense_gemm_reduce_kernel(const float *__restrict__ slab,
                                                                const float *__restrict__ V, float *__restrict__ out,
                                                                int N, int T, int t0, int tcnt, int nsplit, float noise,
                                                                int sw) {
  __shared__ float part[8][32];
  const int o = threadIdx.x & 31, g = threadIdx.x >> 5;
  const size_t per = (size_t)N * sw;
  const size_t gid = (size_t)blockIdx.x * 32 + o;
  float acc = 0.f;
  if (gid < per) {
    int sidx = g;
    for (; sidx + 24 < nsplit; sidx += 32) {
      const float x0 = slab[(size_t)sidx * per + gid], x1 = slab[(size_t)(sidx + 8) * per + gid];
      const float x2 = slab[(size_t)(sidx + 16) * per + gid], x3 = slab[(size_t)(sidx + 24) * per + gid];
      acc += x0;
      acc += x1;
      acc += x2;
      acc += x3;
    }
    for (; sidx < nsplit; sidx += 8) acc += slab[(size_t)sidx * per + gid];
  }
  part[g][o] = acc;
  __syncthreads();
  if (g != 0 || gid >= per) return;
  const int row = (int)(gid / sw), n = (int)(gid % sw);
  if (n >= tcnt) return;
  float tot = part[0][o];
#pragma unroll
  for (int q = 1; q < 8; ++q) tot += part[q][o];
  const size_t oidx = (size_t)row * T + t0 + n;
  out[oidx] = __builtin_fmaf(noise, V[oidx], tot);
}

// Reduce of the VALU form's column-fastest slabs [split][t][npad]: out[col][t] = sum_split slab + noise * V[col][t].
// Same 8-group fixed-order scheme as above; a workgroup owns 32 consecutive columns of one t.
__global__ __launch_bounds__(256) void dense_gemv_reduce_kernel(const float *__restrict__ slab,
                                                                const float *__restrict__ V, float *__restrict__ out,
                                                                int N, int T, int nsplit, float noise) {
  __shared__ float part[8][32];
  const int o = threadIdx.x & 31, g = threadIdx.x >> 5;
  const size_t npad = ((size_t)N + 3) & ~(size_t)3;
  const int t = blockIdx.y;
  const int col = blockIdx.x * 32 + o;
  const size_t per = npad * T;
  const size_t e = (size_t)t * npad + col;
  float acc = 0.f;
  if (col < N) {
    int sidx = g;
    for (; sidx + 24 < nsplit; sidx += 32) {
      const float x0 = slab[(size_t)sidx * per + e], x1 = slab[(size_t)(sidx + 8) * per + e];
      const float x2 = slab[(size_t)(sidx + 16) * per + e], x3 = slab[(size_t)(sidx + 24) * per + e];
      acc += x0;
      acc += x1;
      acc += x2;
      acc += x3;
    }
    for (; sidx < nsplit; sidx += 8) acc += slab[(size_t)sidx * per + e];
  }
  part[g][o] = acc;
  __syncthreads();
  if (g != 0 || col >= N) return;
  float tot = part[0][o];
#pragma unroll
  for (int q = 1; q < 8; ++q) tot += part[q][o];
  const size_t oidx = (size_t)col * T + t;
  out[oidx] = __builtin_fmaf(noise, V[oidx], tot);
}

}  // namespace

extern "C" {

namespace {
// resident workgroups per CU of dense_gemv_valu_kernel<T>, asked of the runtime once per T (register and LDS budget of
// the instantiation hipcc actually produced), capped at 8
int gemv_blocks_per_cu(int T) {
  static std::atomic<int> cache[13];
  const int tt = T < 1 ? 1 : (T > 12 ? 12 : T);
  int v = cache[tt].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int nb = 0;
  hipError_t e = hipSuccess;
#define RPGP_OCC_CASE(TT_)                                                                                             \
  case TT_:                                                                                                            \
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dense_gemv_valu_kernel<TT_>, 256, 0);                         \
    break
  switch (tt) {
    RPGP_OCC_CASE(1); RPGP_OCC_CASE(2); RPGP_OCC_CASE(3); RPGP_OCC_CASE(4); RPGP_OCC_CASE(5); RPGP_OCC_CASE(6);
    RPGP_OCC_CASE(7); RPGP_OCC_CASE(8); RPGP_OCC_CASE(9); RPGP_OCC_CASE(10); RPGP_OCC_CASE(11);
    default: RPGP_OCC_CASE(12);
  }
#undef RPGP_OCC_CASE
  if (e != hipSuccess || nb < 1) nb = 4;
  if (nb > 8) nb = 8;
  cache[tt].store(nb, std::memory_order_relaxed);
  return nb;
}
}  // namespace

int rpgp_dense_mvm(const float *Kd, const float *V, float *out, int64_t N, int64_t ldk, int T, float noise,
                   void *stream) {
  if (!Kd || !V || !out || N <= 0 || T <= 0 || ldk < N || N > 0x7fffffffLL) return RPGP_EINVAL;
  {
    const int irc = rpgp_init();
    if (irc) return irc;
  }
  hipStream_t st = as_stream(stream);
  float *slab = nullptr;
  int rc = 0;
  if (T <= 12) {
    // VALU form: 256 output columns per workgroup, the rows split over blockIdx.y (and over the four waves inside).
    // Every workgroup streams the same amount of data and they all start together, so the launch must be ONE resident
    // round: a grid a few percent over the resident capacity runs two rounds and doubles the time (N = 14 939, T = 11: 1560
    // workgroups on 1536 slots).  Capacity per CU from the register budget of the instantiation: <= 64 VGPRs (T <= 2) 8
    // workgroups, T <= 8 six, wider five (a conservative count of what hipcc allocates for them).
    const unsigned ncb = (unsigned)((N + 255) / 256);
    const int per_cu = gemv_blocks_per_cu(T);
    const long long resident = (long long)g_num_cus * per_cu;
    long long nsplit = resident / ncb;
    const long long cap_bytes = (long long)(0.15 * (double)N / T);      // slab bytes <= 15 % of the matrix bytes
    if (nsplit > cap_bytes) nsplit = cap_bytes;
    if (nsplit > (N + 63) / 64) nsplit = (N + 63) / 64;
    if (nsplit > 160) nsplit = 160;
    if (nsplit < 1) nsplit = 1;
    int cps = (int)((N + nsplit - 1) / nsplit);
    cps = (cps + 31) / 32 * 32;                        // whole 8-row batches for each of the four waves
    nsplit = (N + cps - 1) / cps;
    const size_t npad = ((size_t)N + 3) & ~(size_t)3;
    RPGP_CHECK(hipMallocAsync((void **)&slab, (size_t)nsplit * npad * T * sizeof(float), st));
    dim3 vgrid(ncb, (unsigned)nsplit), block(256);
#define RPGP_GEMV_CASE(TT_)                                                                                            \
  case TT_:                                                                                                            \
    hipLaunchKernelGGL((dense_gemv_valu_kernel<TT_>), vgrid, block, 0, st, Kd, V, slab, (int)N, (long long)ldk, cps);   \
    break
    switch (T) {
      RPGP_GEMV_CASE(1); RPGP_GEMV_CASE(2); RPGP_GEMV_CASE(3); RPGP_GEMV_CASE(4); RPGP_GEMV_CASE(5); RPGP_GEMV_CASE(6);
      RPGP_GEMV_CASE(7); RPGP_GEMV_CASE(8); RPGP_GEMV_CASE(9); RPGP_GEMV_CASE(10); RPGP_GEMV_CASE(11);
      default: RPGP_GEMV_CASE(12);
    }
#undef RPGP_GEMV_CASE
    hipLaunchKernelGGL(dense_gemv_reduce_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)T), dim3(256), 0, st, slab, V,
                       out, (int)N, T, (int)nsplit, noise);
    rc = launch_status();
    (void)hipFreeAsync(slab, st);
    return rc;
  }
  const int nrb = (int)((N + 255) / 256);
  const int ncb_ = (int)((N + 255) / 256);
  int nsplit = (3072 + ncb_ - 1) / ncb_;          // ~3000 workgroups keep enough loads in flight to stream HBM
  const int max_split = (int)((N + 255) / 256);
  if (nsplit > max_split) nsplit = max_split;
  if (nsplit > 32) nsplit = 32;
  if (nsplit < 1) nsplit = 1;
  int cps = (int)((N + nsplit - 1) / nsplit);
  cps = (cps + 255) / 256 * 256;
  nsplit = (int)((N + cps - 1) / cps);
  RPGP_CHECK(hipMallocAsync((void **)&slab, (size_t)nsplit * N * 16 * sizeof(float), st));
  dim3 grid((unsigned)nrb, (unsigned)nsplit), block(256);
  for (int t0 = 0; t0 < T && rc == 0; t0 += 16) {
    const int tcnt = (T - t0 < 16) ? T - t0 : 16;
    hipLaunchKernelGGL(dense_gemm_kernel, grid, block, 0, st, Kd, V, slab, (int)N, (long long)ldk, T, t0, tcnt, cps);
    const size_t total = (size_t)N * 16;
    hipLaunchKernelGGL(dense_gemm_reduce_kernel, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, slab, V, out,
                       (int)N, T, t0, tcnt, nsplit, noise, 16);
    rc = launch_status();
  }
  (void)hipFreeAsync(slab, st);
  return rc;
}

}  // extern "C"
