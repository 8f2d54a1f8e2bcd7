// rpgp_inducing.hip — what an inducing-point (SGPR) objective needs from the N training rows, with no N x M object held:
//     rpgp_inducing_gram   G[M x M] = sum_i k_i k_i^T,  g[M x T] = sum_i k_i Y_i^T,   k_i = phi_kind(|z_i - u_.|^2)
//     rpgp_inducing_grad   the adjoint of both with respect to the inducing points U and the per-feature squared differences
// k_i is the float32 entry of the radial tile body (rpgp_radial_tile.h: Gram-form distance on v_mfma_f32_16x16x4_f32); every
// product of two float32 values is exact in float64 and every sum over the rows is float64 on v_mfma_f64_16x16x4_f64.
//
// Why float64 (measured on the host): with G accumulated in float32, A = K_uu + (s / sigma^2) G lost positive
// definiteness at cond(K_uu) = 2e5; with C = dL/dG rounded to float32 the gradient with respect to U was off by 5e-4 there.
//
// The rows are walked in slabs whose length comes from the workspace the caller hands in.  Per slab:
//   1. inducing_slab_kernel    phi (and phi') of the slab, rows x Mp float32 (Mp = M padded to 64, zero in the padding)
//   2. inducing_s_kernel       (derivative only) S = (2 K C + Y v^T) o phi', K C on the float64 matrix cores with C as given
//   3. wide_gram_kernel        part (+)= A^T [B1 | B2 (squared) | 1] in float64: A = phi, B = [phi | Y] for the Gram entries;
//                              A = S, B = [Z | Z o Z | 1] for the derivative (P = S^T Z, Q = S^T Z^2, cs = S^T 1)
// and once at the end the row splits of `part` are summed in split order.  One writer per element everywhere, fixed order, no
// atomics: repeated calls are bit-identical (for one slab length).
//
// f64 MFMA lane map (lane l: c = l % 16, q = l / 16): A operand = A[i = c][k = q], B operand = B[k = q][j = c], result register
// r = D[i = q + 4 r][j = c].
//
// Not tuned: the wide Gram reads its operands straight from memory (L2 serves the reuse), and the derivative recomputes the slab
// the Gram entry already made.  tools/sgpr_bench.py times the whole step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/rpgp.h"

namespace {

#include "rpgp_radial_tile.h"

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int kMaxM = 1024;
constexpr int kMaxT = 16;
constexpr int kMaxSplits = 8;
constexpr long long kMaxSlab = 1LL << 20;

// ---- 1. the slab: phi and phi' of rows [0, nrows) of Zs against U --------------------------------------------------------------
// grid = (row blocks of the slab, column tiles); every element of the rpad x Mp buffers is written (zero outside nrows x M).
template <int KIND, bool DERIV>
__global__ __launch_bounds__(256) void inducing_slab_kernel(const float *__restrict__ Zs, const float *__restrict__ U,
                                                            const float *__restrict__ nz, const float *__restrict__ nu,
                                                            float *__restrict__ phi, float *__restrict__ dphi, long long nrows,
                                                            int M, int Mp, int d, int ldz, int ldu) {
  __shared__ float sA[kKC * kLd];
  __shared__ float sB[kKC * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const long long row0 = (long long)blockIdx.x * kRB;
  const long long grow = row0 + wave * 16 + m;
  const long long col0 = (long long)blockIdx.y * kCT;
  const float na_r = nz[grow];
  floatx4 acc[4];
  gram_tile(sA, sB, Zs, nrows, ldz, row0, U, (long long)M, ldu, col0, d, true, acc, []() {});
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const long long cbase = col0 + ct * 16 + 4 * q;
    const floatx4 nbv = *reinterpret_cast<const floatx4 *>(nu + cbase);
    floatx4 pv, dv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d2 = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[ct][r], na_r + nbv[r]), 0.f);
      float p, dp;
      phi_both<KIND>(d2, p, dp);
      const bool in = grow < nrows && cbase + r < M;
      pv[r] = in ? p : 0.f;
      dv[r] = in ? dp : 0.f;
    }
    *reinterpret_cast<floatx4 *>(phi + (size_t)grow * Mp + cbase) = pv;
    if constexpr (DERIV) *reinterpret_cast<floatx4 *>(dphi + (size_t)grow * Mp + cbase) = dv;
  }
}

// ---- 2. S = (2 K C + Y v^T) o phi', in place over phi' --------------------------------------------------------------------------
// grid = (row blocks of the slab, column tiles); a wave owns 16 rows x 64 columns.  The contraction index of step e of a
// 16-wide chunk is k0 + 4 q + e on both operands (each lane reads its four K values as one 16-byte load).
__global__ __launch_bounds__(256) void inducing_s_kernel(const float *__restrict__ phi, float *__restrict__ dphi_s,
                                                         const double *__restrict__ C, const float *__restrict__ Ys,
                                                         const double *__restrict__ v, long long nrows, int M, int Mp, int T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const long long r0 = (long long)blockIdx.x * kRB + wave * 16;
  const int j0 = blockIdx.y * kCT;
  doublex4 acc[4], acy[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    acc[nb] = doublex4{0.0, 0.0, 0.0, 0.0};
    acy[nb] = doublex4{0.0, 0.0, 0.0, 0.0};
  }
  const float *arow = phi + (size_t)(r0 + c) * Mp;
  const int kend = (M + 15) & ~15;
  for (int k0 = 0; k0 < kend; k0 += 16) {
    const floatx4 a4 = *reinterpret_cast<const floatx4 *>(arow + k0 + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = k0 + 4 * q + e;
      const int kc = kk < M ? kk : M - 1;
      const double a = (double)a4[e];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const int col = j0 + 16 * nb + c;
        const double b = C[(size_t)kc * M + (col < M ? col : M - 1)];
        acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (kk < M && col < M) ? b : 0.0, acc[nb], 0, 0, 0);
      }
    }
  }
  if (T > 0) {
    const long long yr = r0 + c;
    const long long yrc = yr < nrows ? yr : nrows - 1;
    for (int t0 = 0; t0 < T; t0 += 4) {
      const int t = t0 + q;
      const int tc = t < T ? t : T - 1;
      const float yv = Ys[(size_t)yrc * T + tc];
      const double a = (yr < nrows && t < T) ? (double)yv : 0.0;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const int col = j0 + 16 * nb + c;
        const double b = v[(size_t)(col < M ? col : M - 1) * T + tc];
        acy[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (t < T && col < M) ? b : 0.0, acy[nb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t at = (size_t)(r0 + q + 4 * r) * Mp + j0 + 16 * nb + c;   // (inside the rpad x Mp buffer; phi' is zero outside)
      const double w = 2.0 * acc[nb][r] + acy[nb][r];
      dphi_s[at] = (float)(w * (double)dphi_s[at]);
    }
}

// ---- 3. part[split] (+)= A^T [B1 | B2 | 1] ---------------------------------------------------------------------------------------
// A: rows x KA float32 (lda); the right operand has KB = n1 + n2 + ones virtual columns: B1 (n1, ld1), then B2 (n2, ld2; squared
// in float64 when sq2), then a column of ones.  grid = (KA tiles of 64, KB tiles of 64, row splits); a wave owns 16 x 64 of the
// output; split z walks a contiguous range of 4-row steps.  part[z][i * KB + j].  `sym` (B1 == A, the Gram matrix): the 64 x 64
// tiles strictly below the diagonal are left out and never read; sum_parts_kernel takes them from their mirror tiles.
struct WideB {
  const float *B1;
  long long ld1;
  int n1;
  const float *B2;
  long long ld2;
  int n2;
  int sq2;
  int ones;
};

__global__ __launch_bounds__(256) void wide_gram_kernel(const float *__restrict__ A, long long lda, int KA, WideB b, int KB,
                                                        long long rows, double *__restrict__ part, int accumulate,
                                                        int sym) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int a0 = blockIdx.x * 64 + wave * 16;
  const int b0 = blockIdx.y * 64;
  if (a0 >= KA) return;                                                   // (wave-uniform; no barrier below)
  if (sym && blockIdx.y < blockIdx.x) return;                             // (the mirror tile is summed in its place)
  doublex4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = doublex4{0.0, 0.0, 0.0, 0.0};
  const long long nsteps = (rows + 3) / 4;
  const long long per = (nsteps + gridDim.z - 1) / gridDim.z;
  const long long s0 = (long long)blockIdx.z * per;
  const long long s1 = s0 + per < nsteps ? s0 + per : nsteps;
  const int acol = a0 + c;
  const int acolc = acol < KA ? acol : KA - 1;
  // the lane's four right-operand columns do not change over the rows: where they live (a valid address for the column of
  // ones and for the padding too, so that every load is unconditional) and what becomes of the value loaded
  const float *bp[4];
  long long bl[4];
  int bm[4];                                                              // 0 as loaded, 1 squared, 2 one, 3 zero
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int col = b0 + 16 * nb + c;
    if (col < b.n1) {
      bp[nb] = b.B1 + col, bl[nb] = b.ld1, bm[nb] = 0;
    } else if (col < b.n1 + b.n2) {
      bp[nb] = b.B2 + (col - b.n1), bl[nb] = b.ld2, bm[nb] = b.sq2 ? 1 : 0;
    } else {
      bp[nb] = A + acolc, bl[nb] = lda, bm[nb] = col < KB ? 2 : 3;
    }
  }
  constexpr int kU = 4;                                                   // steps in flight: their loads issue together
  for (long long s = s0; s < s1; s += kU) {
    float av[kU], xv[kU][4];
    bool rv[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long n = 4 * (s + u) + q;
      rv[u] = s + u < s1 && n < rows;
      const long long nc = rv[u] ? n : rows - 1;                          // (clamped row + select: no load under a condition)
      av[u] = A[(size_t)nc * lda + acolc];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) xv[u][nb] = bp[nb][(size_t)nc * bl[nb]];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const double a = (rv[u] && acol < KA) ? (double)av[u] : 0.0;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        if (b0 + 16 * nb < KB) {
          const double x = (double)xv[u][nb];
          const double bv = bm[nb] == 0 ? x : bm[nb] == 1 ? x * x : bm[nb] == 2 ? 1.0 : 0.0;
          acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rv[u] ? bv : 0.0, acc[nb], 0, 0, 0);
        }
      }
    }
  }
  double *dst = part + (size_t)blockIdx.z * KA * KB;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = a0 + q + 4 * r, j = b0 + 16 * nb + c;
      if (i < KA && j < KB) {
        const size_t at = (size_t)i * KB + j;
        dst[at] = accumulate ? dst[at] + acc[nb][r] : acc[nb][r];
      }
    }
}

// out[i][j - c0] (leading dimension ldo) = the splits' sums of columns [c0, c1), in split order.  `out` may be split 0 of
// `part` itself (c0 = 0, ldo = KB, no mirror): a thread reads only the element it writes.  `mirror`: an element of a tile
// strictly below the diagonal is the sum of its transposed element (see wide_gram_kernel; both triangles are written).
__global__ __launch_bounds__(256) void sum_parts_kernel(const double *part, int splits, int KA, int KB, int c0, int c1,
                                                        double *out, int ldo, int mirror) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int w = c1 - c0;
  if (idx >= (long long)KA * w) return;
  const int i = (int)(idx / w), j = c0 + (int)(idx - (long long)i * w);
  const bool flip = mirror && (j >> 6) < (i >> 6);
  const size_t at = flip ? (size_t)j * KB + i : (size_t)i * KB + j;
  double s = 0.0;
  for (int z = 0; z < splits; ++z) s += part[(size_t)z * KA * KB + at];
  out[(size_t)i * ldo + (j - c0)] = s;
}

// red = [P | Q | cs] (M x (2 d + 1), summed over the splits):  gU[j][m] = 2 (cs_j u_jm - P_jm)
__global__ __launch_bounds__(256) void inducing_gu_kernel(const double *__restrict__ red, const float *__restrict__ U, int ldu,
                                                          int M, int d, double *__restrict__ gU) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)M * d) return;
  const int j = (int)(idx / d), m = (int)(idx - (long long)j * d);
  const int KB = 2 * d + 1;
  const double u = (double)U[(size_t)j * ldu + m];
  gU[idx] = 2.0 * (red[(size_t)j * KB + 2 * d] * u - red[(size_t)j * KB + m]);
}

// q[m] = sum_j (Q_jm - 2 u_jm P_jm + cs_j u_jm^2), j in order
__global__ __launch_bounds__(256) void inducing_q_kernel(const double *__restrict__ red, const float *__restrict__ U, int ldu,
                                                         int M, int d, double *__restrict__ qout) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= d) return;
  const int KB = 2 * d + 1;
  double s = 0.0;
  for (int j = 0; j < M; ++j) {
    const double u = (double)U[(size_t)j * ldu + m];
    const double *row = red + (size_t)j * KB;
    s += row[d + m] - 2.0 * u * row[m] + row[2 * d] * u * u;
  }
  qout[m] = s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int splits_for(int KA, int KB, bool sym) {
  const int ta = (KA + 63) / 64, tb = (KB + 63) / 64;
  const int tiles = sym ? ta * (ta + 1) / 2 + ta * (tb - ta) : ta * tb;      // (the tiles that run: see wide_gram_kernel)
  int s = 512 / tiles;
  if (s < 1) s = 1;
  if (s > kMaxSplits) s = kMaxSplits;
  return s;
}

inline size_t part_bytes(int M, int d, int T) {
  const size_t gram = (size_t)splits_for(M, M + T, true) * M * (size_t)(M + T);
  const size_t grad = (size_t)splits_for(M, 2 * d + 1, false) * M * (size_t)(2 * d + 1);
  return align256(sizeof(double) * (gram > grad ? gram : grad));
}
inline size_t fixed_bytes(int M, int d, int T) { return align256(sizeof(float) * (size_t)pad64(M)) + part_bytes(M, d, T); }
inline size_t row_bytes(int M) { return sizeof(float) * (1 + 2 * (size_t)pad64(M)); }

inline bool bad_shape(int64_t M, int d, int T) { return M < 1 || M > kMaxM || d < 1 || d > kMaxD || T < 0 || T > kMaxT; }

struct Layout {
  float *nu, *nz, *phi, *dphi;
  double *part;
  long long slab;
};

// the slab length the workspace allows (a multiple of 64, no longer than the padded N); 0: too small
inline long long carve(void *workspace, size_t bytes, int64_t N, int M, int d, int T, Layout &lay) {
  const size_t fixed = fixed_bytes(M, d, T);
  if (bytes < fixed + 64 * row_bytes(M)) return 0;
  long long slab = (long long)((bytes - fixed) / row_bytes(M)) & ~63LL;
  if (slab > pad64(N)) slab = pad64(N);
  if (slab > kMaxSlab) slab = kMaxSlab;
  char *w = reinterpret_cast<char *>(workspace);
  lay.nu = reinterpret_cast<float *>(w); w += align256(sizeof(float) * (size_t)pad64(M));
  lay.part = reinterpret_cast<double *>(w); w += part_bytes(M, d, T);
  lay.nz = reinterpret_cast<float *>(w); w += sizeof(float) * (size_t)slab;
  lay.phi = reinterpret_cast<float *>(w); w += sizeof(float) * (size_t)slab * (size_t)pad64(M);
  lay.dphi = reinterpret_cast<float *>(w);
  lay.slab = slab;
  return slab;
}

inline int launch_wide(const float *A, long long lda, int KA, const WideB &b, long long rows, double *part, bool accumulate,
                       bool sym, hipStream_t st) {
  const int KB = b.n1 + b.n2 + b.ones;
  const dim3 grid((unsigned)((KA + 63) / 64), (unsigned)((KB + 63) / 64), (unsigned)splits_for(KA, KB, sym));
  hipLaunchKernelGGL(wide_gram_kernel, grid, dim3(256), 0, st, A, lda, KA, b, KB, rows, part, accumulate ? 1 : 0,
                     sym ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t rpgp_inducing_workspace_bytes(int64_t M, int d, int T, int64_t rows) {
  if (bad_shape(M, d, T) || rows < 1) return 0;
  long long r = pad64(rows);
  if (r > kMaxSlab) r = kMaxSlab;
  return fixed_bytes((int)M, d, T) + (size_t)r * row_bytes((int)M);
}

int rpgp_inducing_gram(int kind, const float *Z, const float *U, const float *Y, double *G, double *g, int64_t N, int64_t M,
                       int d, int ldz, int ldu, int T, void *workspace, size_t workspace_bytes, void *stream) {
  if (kind < RPGP_KIND_RBF || kind > RPGP_KIND_COSINE || bad_shape(M, d, T) || N < 1 || N >= (1LL << 31) - 64 || !Z || !U ||
      !G || !workspace || ldz < d || ldu < d || (T > 0 && (!Y || !g)) || !aligned(Z, 4) || !aligned(U, 4) || !aligned(Y, 4) ||
      !aligned(G, 8) || !aligned(g, 8) || !aligned(workspace, 16))
    return RPGP_EINVAL;
  Layout lay;
  if (!carve(workspace, workspace_bytes, N, (int)M, d, T, lay)) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Mi = (int)M, Mp = (int)pad64(M);
  int rc = launch_norms(U, M, d, ldu, lay.nu, st);
  if (rc) return rc;
  for (long long r0 = 0; r0 < N; r0 += lay.slab) {
    const long long nr = N - r0 < lay.slab ? N - r0 : lay.slab;
    const float *Zs = Z + (size_t)r0 * ldz;
    rc = launch_norms(Zs, nr, d, ldz, lay.nz, st);
    if (rc) return rc;
    const dim3 grid((unsigned)(pad64(nr) / kRB), (unsigned)(Mp / kCT));
    RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL((inducing_slab_kernel<KK_, false>), grid, dim3(256), 0, st, Zs, U, lay.nz,
                                                  lay.nu, lay.phi, lay.dphi, nr, Mi, Mp, d, ldz, ldu));
    rc = (int)hipGetLastError();
    if (rc) return rc;
    const WideB b{lay.phi, Mp, Mi, T > 0 ? Y + (size_t)r0 * T : nullptr, T, T, 0, 0};
    rc = launch_wide(lay.phi, Mp, Mi, b, nr, lay.part, r0 > 0, true, st);
    if (rc) return rc;
  }
  const int KB = Mi + T, splits = splits_for(Mi, KB, true);
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)(((long long)Mi * Mi + 255) / 256)), dim3(256), 0, st, lay.part, splits,
                     Mi, KB, 0, Mi, G, Mi, 1);
  rc = (int)hipGetLastError();
  if (rc || T == 0) return rc;
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)(((long long)Mi * T + 255) / 256)), dim3(256), 0, st, lay.part, splits, Mi,
                     KB, Mi, KB, g, T, 0);
  return (int)hipGetLastError();
}

int rpgp_inducing_grad(int kind, const float *Z, const float *U, const float *Y, const double *C, const double *v, double *gU,
                       double *q, int64_t N, int64_t M, int d, int ldz, int ldu, int T, void *workspace,
                       size_t workspace_bytes, void *stream) {
  if (kind < RPGP_KIND_RBF || kind > RPGP_KIND_COSINE || bad_shape(M, d, T) || N < 1 || N >= (1LL << 31) - 64 || !Z || !U ||
      !C || !gU || !q || !workspace || ldz < d || ldu < d || (T > 0 && (!Y || !v)) || !aligned(Z, 4) || !aligned(U, 4) ||
      !aligned(Y, 4) || !aligned(C, 8) || !aligned(v, 8) || !aligned(gU, 8) || !aligned(q, 8) || !aligned(workspace, 16))
    return RPGP_EINVAL;
  Layout lay;
  if (!carve(workspace, workspace_bytes, N, (int)M, d, T, lay)) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Mi = (int)M, Mp = (int)pad64(M);
  int rc = launch_norms(U, M, d, ldu, lay.nu, st);
  if (rc) return rc;
  for (long long r0 = 0; r0 < N; r0 += lay.slab) {
    const long long nr = N - r0 < lay.slab ? N - r0 : lay.slab;
    const float *Zs = Z + (size_t)r0 * ldz;
    rc = launch_norms(Zs, nr, d, ldz, lay.nz, st);
    if (rc) return rc;
    const dim3 grid((unsigned)(pad64(nr) / kRB), (unsigned)(Mp / kCT));
    RADIAL_DISPATCH_KIND(kind, hipLaunchKernelGGL((inducing_slab_kernel<KK_, true>), grid, dim3(256), 0, st, Zs, U, lay.nz,
                                                  lay.nu, lay.phi, lay.dphi, nr, Mi, Mp, d, ldz, ldu));
    rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(inducing_s_kernel, grid, dim3(256), 0, st, lay.phi, lay.dphi, C, T > 0 ? Y + (size_t)r0 * T : nullptr, v,
                       nr, Mi, Mp, T);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    const WideB b{Zs, ldz, d, Zs, ldz, d, 1, 1};
    rc = launch_wide(lay.dphi, Mp, Mi, b, nr, lay.part, r0 > 0, false, st);
    if (rc) return rc;
  }
  const int KB = 2 * d + 1, splits = splits_for(Mi, KB, false);
  // the splits summed in place into split 0 (each thread reads and writes its own element), then gU and q from it
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)(((long long)Mi * KB + 255) / 256)), dim3(256), 0, st, lay.part, splits,
                     Mi, KB, 0, KB, lay.part, KB, 0);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(inducing_gu_kernel, dim3((unsigned)(((long long)Mi * d + 255) / 256)), dim3(256), 0, st, lay.part, U, ldu,
                     Mi, d, gU);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(inducing_q_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, lay.part, U, ldu, Mi, d, q);
  return (int)hipGetLastError();
}

}  // extern "C"
