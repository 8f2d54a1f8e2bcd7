// rpgp_radial_tile.h — the tile body of the full radial kernels, shared by rpgp_radial.hip (product, dense block, symmetric
// derivative) and rpgp_inducing.hip (the cross-kernel slab and its derivative): phi / phi', the row norms, the LDS staging and
// the 16 x 64 Gram block of a wave on v_mfma_f32_16x16x4_f32.  Include inside the translation unit's anonymous namespace.
#pragma once

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kRB = 64;          // rows per workgroup (16 per wave)
constexpr int kCT = 64;          // columns per tile
constexpr int kKC = 32;          // features staged per chunk
constexpr int kLd = 81;          // LDS stride of one feature's 64 rows / columns (17 mod 64: the 4 x 16 operand reads spread)
constexpr int kMaxD = 1024;

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline long long pad64(long long n) { return (n + 63) & ~63LL; }

// ---- phi(d2) and phi'(d2) = d phi / d(d2) ---------------------------------------------------------------------------------
template <int KIND> __device__ __forceinline__ void phi_both(float d2, float &phi, float &dphi) {
  if constexpr (KIND == RPGP_KIND_RBF) {
    constexpr float kHalfLog2e = (float)(0.5 * 1.4426950408889634);
    phi = __builtin_amdgcn_exp2f(-kHalfLog2e * d2);                       // exp(-d2 / 2)
    dphi = -0.5f * phi;
  } else if constexpr (KIND == RPGP_KIND_MATERN15) {
    const float r = __builtin_sqrtf(d2);
    constexpr float kSqrt3Log2e = (float)(1.7320508075688772 * 1.4426950408889634);
    const float e = __builtin_amdgcn_exp2f(-kSqrt3Log2e * r);             // exp(-sqrt3 r)
    phi = __builtin_fmaf(1.7320508075688772f, r, 1.0f) * e;
    dphi = -1.5f * e;
  } else if constexpr (KIND == RPGP_KIND_IMQ) {
    const float p = __builtin_amdgcn_rsqf(1.0f + d2);
    phi = p;
    dphi = -0.5f * p * p * p;
  } else {                                                                // cos(pi r); phi' = -(pi^2 / 2) sinc(r)
    const float r = __builtin_sqrtf(d2);
    phi = cospif(r);
    const float x2 = 9.8696044010893586f * d2;
    float sinc;
    if (x2 < 0.25f) {       // the series in d2: no square root, no division near the duplicates (next term < 3e-11)
      sinc = __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, 2.7557319e-6f, -1.9841270e-4f),
                                                                  8.3333333e-3f), -0.16666667f), 1.0f);
    } else {
      sinc = sinpif(r) / (3.14159265358979323846f * r);
    }
    dphi = -4.9348022005446793f * sinc;
  }
}
template <int KIND> __device__ __forceinline__ float phi_val(float d2) {
  if constexpr (KIND == RPGP_KIND_COSINE) {
    return cospif(__builtin_sqrtf(d2));
  } else {
    float p, dp;
    phi_both<KIND>(d2, p, dp);
    return p;
  }
}

// ---- row norms, once per launch -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void radial_norms_kernel(const float *__restrict__ Z, long long n, int d, int ldz,
                                                           float *__restrict__ out, long long npad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  float s = 0.f;
  if (i < n) {
    const float *z = Z + (size_t)i * ldz;
    for (int m = 0; m < d; ++m) s = __builtin_fmaf(z[m], z[m], s);
  }
  out[i] = s;                                                             // (zero in the padding up to a multiple of 64)
}

// 64 rows x 32 features of Z from row0 / feature f0 into dst[feature][row], zero outside the matrix
__device__ __forceinline__ void stage_chunk(float *__restrict__ dst, const float *__restrict__ Z, long long nrows, int ldz,
                                            long long row0, int f0, int d) {
  for (int idx = threadIdx.x; idx < kRB * kKC; idx += 256) {
    const int f = idx & (kKC - 1), r = idx >> 5;
    const long long gr = row0 + r;
    const int gf = f0 + f;
    dst[f * kLd + r] = (gr < nrows && gf < d) ? Z[(size_t)gr * ldz + gf] : 0.f;
  }
}

// The wave's 16 x 64 block of Z1 Z2^T, transposed layout (lane l = (m = l % 16, q = l / 16) holds
// G[row = m][col = 16 ct + 4 q + r]).  `stage_a`: the first tile of this workgroup (with one chunk the rows stay staged).
// `extra()` runs with the staging of chunk 0, between the same two barriers.
template <class Extra>
__device__ __forceinline__ void gram_tile(float *__restrict__ sA, float *__restrict__ sB, const float *__restrict__ Z1,
                                          long long M, int ldz1, long long row0, const float *__restrict__ Z2, long long N,
                                          int ldz2, long long col0, int d, bool stage_a, floatx4 (&acc)[4], Extra extra) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int f0 = 0; f0 < d; f0 += kKC) {
    __syncthreads();
    if (stage_a || d > kKC) stage_chunk(sA, Z1, M, ldz1, row0, f0, d);
    stage_chunk(sB, Z2, N, ldz2, col0, f0, d);
    if (f0 == 0) extra();
    __syncthreads();
    const int left = d - f0;
    const int ksteps = ((left < kKC ? left : kKC) + 3) >> 2;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int k = 4 * ks + q;
      const float a = sA[k * kLd + wave * 16 + m];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float b = sB[k * kLd + ct * 16 + m];
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc[ct], 0, 0, 0);
      }
    }
  }
}

inline int launch_norms(const float *Z, long long n, int d, int ldz, float *out, hipStream_t st) {
  const long long npad = pad64(n);
  hipLaunchKernelGGL(radial_norms_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, Z, n, d, ldz, out, npad);
  return (int)hipGetLastError();
}

#define RADIAL_DISPATCH_KIND(kind_, CALL)                 \
  switch (kind_) {                                        \
    case RPGP_KIND_RBF: { constexpr int KK_ = RPGP_KIND_RBF; CALL; } break;           \
    case RPGP_KIND_MATERN15: { constexpr int KK_ = RPGP_KIND_MATERN15; CALL; } break; \
    case RPGP_KIND_IMQ: { constexpr int KK_ = RPGP_KIND_IMQ; CALL; } break;           \
    default: { constexpr int KK_ = RPGP_KIND_COSINE; CALL; } break;                   \
  }
