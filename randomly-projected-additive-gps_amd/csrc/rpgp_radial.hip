// rpgp_radial.hip — the full (non-additive) radial kernels, matrix-free, on the matrix cores:
//     K[i,i'] = scale * phi_kind(|a_i - b_i'|^2),  a, b = rows of Z1, Z2 (N x d, already centred and divided by the lengthscales)
// with phi the four functions of the family (RBF, Matern-1.5, InverseMQ, Cosine) — the family's single component of
// group = d, for any 1 <= d <= 1024.  The squared distance is taken in the Gram form
//     d2 = max(|a|^2 + |b|^2 - 2 a.b, 0)
// whose a.b is an exact-fp32 FMA chain on v_mfma_f32_16x16x4_f32, so that the VALU is left with phi alone.
//
// Error model (u = 2^-24): |delta d2| <= (d + 4) u (|a| + |b|)^2 for any summation order, hence
// |delta K| <= scale (C_phi delta d2 + c u (1 + d2 |phi'|)) with C_phi = max |phi'| (0.5 / 1.5 / 0.5 / pi^2 / 2).  The error
// grows with the NORMS, not with the distance: callers centre the inputs.
//
// Tiling.  A 256-thread workgroup owns 64 rows (16 per wave) and walks 64-column tiles; the operands of a tile are staged
// through LDS in chunks of 32 features ([feature][row] with stride 81).  The Gram block is computed TRANSPOSED
// (A operand = the columns, B operand = the rows), so that lane l = (m = l % 16, q = l / 16) of a wave holds
// G[row = m][col = 16 ct + 4 q + r], r = 0..3, ct = 0..3 — which is the B-operand layout of the products that follow:
//     product      out^T[t][row]      += sum_col V[col][t]      K[row][col]      (A = V, 4 MFMAs per 16 x 16 block)
//     derivative   (M A)^T[f][row]    += sum_col a[col][f]      M[row][col]      (A = the staged column coordinates)
//     S from factors  S[row][col]      = sum_t [L|R][col][t] [R|L][row][t]       (A = the staged column factors)
// One writer per output element, fixed summation order, no atomics: repeated calls are bit-identical.
//
// Known redundancy (correct, not tuned).  The derivative runs one workgroup column per 128-feature slice (gridDim.y), and EVERY
// slice recomputes the whole Gram block, phi' and S of its tiles: about 4x the Gram work at d = 385.  Its explicit-S form
// (Cholesky regime only, small N) reads S[row][col .. col + 3] with the 16 rows of a wave strided by lds, 16 bytes per lane,
// and repeats that read per slice.  The dense block stores 16 bytes per lane with the same row stride.  A block of fewer than
// 64 rows (the single rows the pivoted-Cholesky loop asks for through _get_rows) still computes 64-row tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/rpgp.h"

namespace {

#include "rpgp_radial_tile.h"

constexpr int kLdV = 20;         // LDS stride of a column's 16 right-hand-side slots
constexpr int kMaxT = 16;
constexpr int kFS = 128;         // features per slice of the derivative's accumulator (8 accumulators of 16 features)
constexpr int kMaxSplit = 32;    // column splits of the product at small M

// ---- product --------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void radial_mvm_kernel(const float *__restrict__ Z1, const float *__restrict__ Z2,
                                                         const float *__restrict__ na, const float *__restrict__ nb,
                                                         const float *__restrict__ V, float *__restrict__ out,
                                                         float *__restrict__ slab, long long M, long long N, int d, int ldz1,
                                                         int ldz2, int T, float scale, float noise, int sym,
                                                         int tiles_per_split) {
  __shared__ float sA[kKC * kLd];
  __shared__ float sB[kKC * kLd];
  __shared__ float sV[kCT * kLdV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const long long row0 = (long long)blockIdx.x * kRB;
  const long long grow = row0 + wave * 16 + m;
  const long long ntiles = (N + kCT - 1) / kCT;
  const long long t_begin = (long long)blockIdx.y * tiles_per_split;
  const long long t_end = t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles;
  const float na_r = na[grow];                                            // (padded to a multiple of 64: in range)
  floatx4 accO[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
  for (long long tile = t_begin; tile < t_end; ++tile) {
    const long long col0 = tile * kCT;
    floatx4 acc[4];
    gram_tile(sA, sB, Z1, M, ldz1, row0, Z2, N, ldz2, col0, d, tile == t_begin, acc, [&]() {
      for (int idx = threadIdx.x; idx < kCT * 16; idx += 256) {
        const int c = idx >> 4, t = idx & 15;
        const long long gc = col0 + c;
        sV[c * kLdV + t] = (gc < N && t < T) ? V[(size_t)gc * T + t] : 0.f;
      }
    });
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const long long cbase = col0 + ct * 16 + 4 * q;
      const floatx4 nbv = *reinterpret_cast<const floatx4 *>(nb + cbase);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float d2 = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[ct][r], na_r + nbv[r]), 0.f);
        if (sym && grow == cbase + r) d2 = 0.f;
        const float kv = phi_val<KIND>(d2);
        const float vop = sV[(ct * 16 + 4 * q + r) * kLdV + m];
        accO[ct & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vop, kv, accO[ct & 1], 0, 0, 0);
      }
    }
  }
  const floatx4 o = accO[0] + accO[1];                                    // out^T[t = 4 q + r][row = m]
  if (gridDim.y == 1) {
    if (grow < M) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = 4 * q + r;
        if (t < T) {
          float val = scale * o[r];
          if (sym) val = __builtin_fmaf(noise, V[(size_t)grow * T + t], val);
          out[(size_t)grow * T + t] = val;
        }
      }
    }
  } else {
    const long long mpad = (long long)gridDim.x * kRB;
    *reinterpret_cast<floatx4 *>(slab + ((size_t)blockIdx.y * mpad + grow) * 16 + 4 * q) = o;
  }
}

// out = scale * (the splits' partial sums, in split order) + noise V
__global__ __launch_bounds__(256) void radial_mvm_finish_kernel(const float *__restrict__ slab, int nsplit, long long mpad,
                                                                const float *__restrict__ V, float *__restrict__ out,
                                                                long long M, int T, float scale, float noise, int sym) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * T) return;
  const long long row = idx / T;
  const int t = (int)(idx - row * T);
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += slab[((size_t)sp * mpad + row) * 16 + t];
  float val = scale * s;
  if (sym) val = __builtin_fmaf(noise, V[idx], val);
  out[idx] = val;
}

// ---- dense block ----------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void radial_dense_kernel(const float *__restrict__ Z1, const float *__restrict__ Z2,
                                                           const float *__restrict__ na, const float *__restrict__ nb,
                                                           float *__restrict__ out, long long M, long long N, int d, int ldz1,
                                                           int ldz2, long long ldo, float scale, int sym, int tiles_per_group) {
  __shared__ float sA[kKC * kLd];
  __shared__ float sB[kKC * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const long long row0 = (long long)blockIdx.x * kRB;
  const long long grow = row0 + wave * 16 + m;
  const long long ntiles = (N + kCT - 1) / kCT;
  const long long t_begin = (long long)blockIdx.y * tiles_per_group;
  const long long t_end = t_begin + tiles_per_group < ntiles ? t_begin + tiles_per_group : ntiles;
  const float na_r = na[grow];
  for (long long tile = t_begin; tile < t_end; ++tile) {
    const long long col0 = tile * kCT;
    floatx4 acc[4];
    gram_tile(sA, sB, Z1, M, ldz1, row0, Z2, N, ldz2, col0, d, tile == t_begin, acc, []() {});
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const long long cbase = col0 + ct * 16 + 4 * q;
      const floatx4 nbv = *reinterpret_cast<const floatx4 *>(nb + cbase);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float d2 = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[ct][r], na_r + nbv[r]), 0.f);
        if (sym && grow == cbase + r) d2 = 0.f;
        const float kv = scale * phi_val<KIND>(d2);
        if (grow < M && cbase + r < N) out[(size_t)grow * ldo + cbase + r] = kv;
      }
    }
  }
}

// ---- derivative -----------------------------------------------------------------------------------------------------------
// gZ[i][f] = 2 scale sum_j S_ij phi'(d2_ij) (a_if - a_jf) = 2 scale (a_if r_i - (M A)_if),  M = S o phi' (zero diagonal),
// r_i = sum_j M_ij; gpart[row block] = sum S o phi over the block's rows (slice 0 only).  grid = (row blocks, feature slices).
template <int KIND, bool EXPLICIT>
__global__ __launch_bounds__(256) void radial_bilinear_kernel(const float *__restrict__ Z, const float *__restrict__ nz,
                                                              const float *__restrict__ L, const float *__restrict__ R,
                                                              const float *__restrict__ S, long long lds,
                                                              float *__restrict__ gZ, float *__restrict__ gpart, long long N,
                                                              int d, int ldz, int ldg, int T, float scale) {
  __shared__ float sA[kKC * kLd];
  __shared__ float sB[kKC * kLd];
  __shared__ float sLR[kKC * kLd];
  __shared__ float sred[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const long long row0 = (long long)blockIdx.x * kRB;
  const long long grow = row0 + wave * 16 + m;
  const int fs0 = blockIdx.y * kFS;
  const int T4 = (T + 3) & ~3, KK = 2 * T4;                               // contraction length of S = [L|R] [R|L]^T, <= 32
  float rowop[8];                                                         // [R | L] of the wave's rows, B-operand layout
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    float v = 0.f;
    if constexpr (!EXPLICIT) {
      const int kk = 4 * s + q;
      if (kk < KK && grow < N) {
        const int t = kk < T4 ? kk : kk - T4;
        if (t < T) v = kk < T4 ? R[(size_t)grow * T + t] : L[(size_t)grow * T + t];
      }
    }
    rowop[s] = v;
  }
  const float na_r = nz[grow];
  floatx4 accG[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) accG[s] = floatx4{0.f, 0.f, 0.f, 0.f};
  float rsum = 0.f, gs = 0.f;
  const long long ntiles = (N + kCT - 1) / kCT;
  for (long long tile = 0; tile < ntiles; ++tile) {
    const long long col0 = tile * kCT;
    floatx4 acc[4];
    gram_tile(sA, sB, Z, N, ldz, row0, Z, N, ldz, col0, d, tile == 0, acc, [&]() {
      if constexpr (!EXPLICIT) {
        for (int idx = threadIdx.x; idx < kCT * kKC; idx += 256) {
          const int kk = idx & (kKC - 1), c = idx >> 5;
          const long long gc = col0 + c;
          float v = 0.f;
          if (kk < KK && gc < N) {
            const int t = kk < T4 ? kk : kk - T4;
            if (t < T) v = kk < T4 ? L[(size_t)gc * T + t] : R[(size_t)gc * T + t];
          }
          sLR[kk * kLd + c] = v;
        }
      }
    });
    floatx4 sacc[4];
    if constexpr (!EXPLICIT) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) sacc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (4 * s < KK) {
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const float aop = sLR[(4 * s + q) * kLd + ct * 16 + m];
            sacc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(aop, rowop[s], sacc[ct], 0, 0, 0);
          }
        }
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long col = col0 + ct * 16 + 4 * q + r;
          sacc[ct][r] = (grow < N && col < N) ? S[(size_t)grow * lds + col] : 0.f;
        }
    }
    floatx4 Mv[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const long long cbase = col0 + ct * 16 + 4 * q;
      const floatx4 nbv = *reinterpret_cast<const floatx4 *>(nz + cbase);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool diag = grow == cbase + r;
        float d2 = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[ct][r], na_r + nbv[r]), 0.f);
        if (diag) d2 = 0.f;
        float p, dp;
        phi_both<KIND>(d2, p, dp);
        const float sv = sacc[ct][r];                                     // (zero outside the matrix: the factors are padded)
        gs = __builtin_fmaf(sv, p, gs);
        const float mv = diag ? 0.f : sv * dp;
        rsum += mv;
        Mv[ct][r] = mv;
      }
    }
#pragma unroll
    for (int ci = 0; ci < kFS / kKC; ++ci) {
      const int c0 = fs0 + ci * kKC;
      if (c0 < d) {
        if (d > kKC) {                                                    // (one chunk: the Gram's staging is this chunk)
          __syncthreads();
          stage_chunk(sB, Z, N, ldz, col0, c0, d);
          __syncthreads();
        }
        const bool second = c0 + 16 < d;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + 4 * q + r;
            accG[2 * ci] = __builtin_amdgcn_mfma_f32_16x16x4f32(sB[m * kLd + c], Mv[ct][r], accG[2 * ci], 0, 0, 0);
            if (second)
              accG[2 * ci + 1] =
                  __builtin_amdgcn_mfma_f32_16x16x4f32(sB[(16 + m) * kLd + c], Mv[ct][r], accG[2 * ci + 1], 0, 0, 0);
          }
      }
    }
  }
  rsum += __shfl_xor(rsum, 16);
  rsum += __shfl_xor(rsum, 32);
  if (grow < N) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = fs0 + s * 16 + 4 * q + r;                           // (M A)^T[f][row = m]
        if (f < d) gZ[(size_t)grow * ldg + f] = 2.0f * scale * __builtin_fmaf(Z[(size_t)grow * ldz + f], rsum, -accG[s][r]);
      }
  }
  if (blockIdx.y == 0) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) gs += __shfl_xor(gs, o);
    if (lane == 0) sred[wave] = gs;
    __syncthreads();
    if (threadIdx.x == 0) gpart[blockIdx.x] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
  }
}

// gscale = 0.5 * sum of the row blocks' partial sums (float64, fixed order)
__global__ __launch_bounds__(256) void radial_gscale_kernel(const float *__restrict__ gpart, long long n,
                                                            float *__restrict__ gscale) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += (double)gpart[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gscale[0] = (float)(0.5 * sh[0]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool bad_dims(int kind, long long M, long long N, int d) {
  return kind < RPGP_KIND_RBF || kind > RPGP_KIND_COSINE || d < 1 || d > kMaxD || M < 1 || N < 1 || M >= (1LL << 31) - 64 ||
         N >= (1LL << 31) - 64;
}

// column splits of the product: enough workgroups for the chip at small M, each split a fixed range of column tiles
inline void mvm_split(long long M, long long N, int &nsplit, int &tiles_per) {
  const long long nrb = (M + kRB - 1) / kRB, ntiles = (N + kCT - 1) / kCT;
  long long want = nrb >= 512 ? 1 : (1024 + nrb - 1) / nrb;
  if (want > kMaxSplit) want = kMaxSplit;
  if (want > ntiles) want = ntiles;
  tiles_per = (int)((ntiles + want - 1) / want);
  nsplit = (int)((ntiles + tiles_per - 1) / tiles_per);
}

}  // namespace

extern "C" {

size_t rpgp_radial_workspace_bytes(int64_t M, int64_t N, int T) {
  if (M < 1 || N < 1 || T < 0 || T > kMaxT) return 0;
  int nsplit = 1, tiles_per = 1;
  mvm_split(M, N, nsplit, tiles_per);
  const long long big = M > N ? M : N;
  size_t total = align256(sizeof(float) * (size_t)pad64(M)) + align256(sizeof(float) * (size_t)pad64(N));
  total += align256(sizeof(float) * 16 * (size_t)pad64(M) * (size_t)(nsplit > 1 ? nsplit : 0));
  total += align256(sizeof(float) * (size_t)((big + kRB - 1) / kRB));
  return total;
}

int rpgp_radial_mvm(int kind, const float *Z1, const float *Z2, const float *V, float *out, int64_t M, int64_t N, int d,
                    int ldz1, int ldz2, int T, float scale, float noise, void *workspace, size_t workspace_bytes,
                    void *stream) {
  const bool sym = Z2 == nullptr;
  if (bad_dims(kind, M, N, d) || !Z1 || !V || !out || !workspace || T < 1 || T > kMaxT || ldz1 < d || (!sym && ldz2 < d) ||
      (sym && M != N) || !aligned4(Z1) || !aligned4(Z2) || !aligned4(V) || !aligned4(out) || !aligned16(workspace))
    return RPGP_EINVAL;
  if (workspace_bytes < rpgp_radial_workspace_bytes(M, N, T)) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char *w = reinterpret_cast<char *>(workspace);
  float *na = reinterpret_cast<float *>(w); w += align256(sizeof(float) * (size_t)pad64(M));
  float *nb = reinterpret_cast<float *>(w); w += align256(sizeof(float) * (size_t)pad64(N));
  float *slab = reinterpret_cast<float *>(w);
  int rc = launch_norms(Z1, M, d, ldz1, na, st);
  if (rc) return rc;
  if (sym) {
    nb = na;
    Z2 = Z1;
    ldz2 = ldz1;
  } else {
    rc = launch_norms(Z2, N, d, ldz2, nb, st);
    if (rc) return rc;
  }
  int nsplit = 1, tiles_per = 1;
  mvm_split(M, N, nsplit, tiles_per);
  const long long nrb = (M + kRB - 1) / kRB;
  RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL(radial_mvm_kernel<KK_>, dim3((unsigned)nrb, (unsigned)nsplit), dim3(256), 0, st,
                                                Z1, Z2, na, nb, V, out, slab, (long long)M, (long long)N, d, ldz1, ldz2, T,
                                                scale, noise, sym ? 1 : 0, tiles_per));
  rc = (int)hipGetLastError();
  if (rc || nsplit == 1) return rc;
  const long long n = (long long)M * T;
  hipLaunchKernelGGL(radial_mvm_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slab, nsplit, nrb * kRB, V,
                     out, (long long)M, T, scale, noise, sym ? 1 : 0);
  return (int)hipGetLastError();
}

int rpgp_radial_dense(int kind, const float *Z1, const float *Z2, float *out, int64_t M, int64_t N, int d, int ldz1, int ldz2,
                      int64_t ldo, float scale, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(kind, M, N, d) || !Z1 || !Z2 || !out || !workspace || ldz1 < d || ldz2 < d || ldo < N || !aligned4(Z1) ||
      !aligned4(Z2) || !aligned4(out) || !aligned16(workspace))
    return RPGP_EINVAL;
  if (workspace_bytes < rpgp_radial_workspace_bytes(M, N, 0)) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char *w = reinterpret_cast<char *>(workspace);
  float *na = reinterpret_cast<float *>(w); w += align256(sizeof(float) * (size_t)pad64(M));
  float *nb = reinterpret_cast<float *>(w);
  int rc = launch_norms(Z1, M, d, ldz1, na, st);
  if (rc) return rc;
  rc = launch_norms(Z2, N, d, ldz2, nb, st);
  if (rc) return rc;
  const bool sym = Z1 == Z2 && M == N && ldz1 == ldz2;                    // the square block of one Z: exact diagonal
  const long long nrb = (M + kRB - 1) / kRB, ntiles = (N + kCT - 1) / kCT;
  long long groups = (2048 + nrb - 1) / nrb;
  if (groups > ntiles) groups = ntiles;
  if (groups > 65535) groups = 65535;
  const int tiles_per = (int)((ntiles + groups - 1) / groups);
  groups = (ntiles + tiles_per - 1) / tiles_per;
  RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL(radial_dense_kernel<KK_>, dim3((unsigned)nrb, (unsigned)groups), dim3(256), 0, st,
                                                Z1, Z2, na, nb, out, (long long)M, (long long)N, d, ldz1, ldz2, (long long)ldo,
                                                scale, sym ? 1 : 0, tiles_per));
  return (int)hipGetLastError();
}

int rpgp_radial_bilinear_grad(int kind, const float *Z, const float *L, const float *R, const float *S, float *gZ,
                              float *gscale, int64_t N, int d, int ldz, int ldg, int T, int64_t lds, float scale,
                              void *workspace, size_t workspace_bytes, void *stream) {
  const bool expl = S != nullptr;
  if (bad_dims(kind, N, N, d) || !Z || !gZ || !gscale || !workspace || ldz < d || ldg < d || !aligned4(Z) || !aligned4(gZ) ||
      !aligned4(gscale) || !aligned16(workspace))
    return RPGP_EINVAL;
  if (expl ? (lds < N || !aligned4(S)) : (!L || !R || T < 1 || T > kMaxT || !aligned4(L) || !aligned4(R))) return RPGP_EINVAL;
  if (workspace_bytes < rpgp_radial_workspace_bytes(N, N, 0)) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char *w = reinterpret_cast<char *>(workspace);
  float *nz = reinterpret_cast<float *>(w); w += 2 * align256(sizeof(float) * (size_t)pad64(N));
  float *gpart = reinterpret_cast<float *>(w);
  int rc = launch_norms(Z, N, d, ldz, nz, st);
  if (rc) return rc;
  const long long nrb = (N + kRB - 1) / kRB;
  const int nslices = (d + kFS - 1) / kFS;
  const dim3 grid((unsigned)nrb, (unsigned)nslices);
  if (expl) {
    RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL((radial_bilinear_kernel<KK_, true>), grid, dim3(256), 0, st, Z, nz, L, R, S,
                                                  (long long)lds, gZ, gpart, (long long)N, d, ldz, ldg, 0, scale));
  } else {
    RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL((radial_bilinear_kernel<KK_, false>), grid, dim3(256), 0, st, Z, nz, L, R, S,
                                                  (long long)0, gZ, gpart, (long long)N, d, ldz, ldg, T, scale));
  }
  rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(radial_gscale_kernel, dim3(1), dim3(256), 0, st, gpart, nrb, gscale);
  return (int)hipGetLastError();
}

}  // extern "C"
