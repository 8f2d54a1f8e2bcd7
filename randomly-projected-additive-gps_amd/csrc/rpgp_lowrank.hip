// rpgp_lowrank.hip — Chebyshev low-rank form of the prepared symmetric MVM (gfx950).
//
// On the centred, exp2-scaled coordinates of rpgp_prepare every 1-D term is exp2(-(a - b)^2) with |a|, |b| <= h
// (h = max_abs of the prep header).  With x = a / h on [-1, 1]:
//   exp2(-h^2 (x - y)^2) = sum_{m,n < p} c_mn T_m(x) T_n(y) + tail,   |tail| <= sum_{max(m,n) >= p} |c_mn|  (|T_m| <= 1)
// so   K_j v = T(x_j) (C (T(x_j)^T v))   costs ~4 N p FMAs per projection and no transcendentals.  The rank p is chosen on
// the host (double precision) so that the discarded tail is <= 2^-26 per kernel entry, below fp32 rounding of the entries.
//
// Plan (once per Z, after rpgp_prepare): the p x p coefficients in fp32 (zero-padded to PB = p rounded up to 8) and the
// coordinates x = a / h transposed to [J][N] (one coalesced row per projection), both in a caller-owned device buffer.
// Product: three launches, no float atomics (repeated calls are bit-identical):
//   (a) project  W_j[n][t]  = sum_i T_n(x_ij) v_it           per (row block, projection, t): block partials
//   (b) combine  U_j[m][t]  = scale * sum_n c_mn W_j[n][t]   per (projection, t): partials summed in a fixed order
//   (c) output   out_it     = sum_j sum_m T_m(x_ij) U_j[m][t] (Clenshaw) + noise * v_it
// The product moves ~4 MB and does ~40 M FMAs at the headline shape, so each kernel is a latency chain rather than a stream,
// and each requests every global load it needs before its first wait: (a) its 8 rows' x and v, then the recurrence and the sums
// in float64; (b) a batch of block partials and the thread's chunk of a coefficient row; (c) the lane's coordinates, its element
// of V and the thread's share of U, which goes through LDS.  DESIGN.md 7.4 and 7.4a have the measurements.
//
// Bilinear derivative (rpgp_bilinear_grad's contract, S = L R^T + R L^T).  With g(x, y) = d f / dx, the factor of that
// contract is  -(z_i - z_i') e(i, i') = (kappa / h) g(x_i, x_i')  (kappa = (2 ln 2)^-1/2: a = (z - mid) kappa), and
//   G(x, y) = (kappa / h) g(x, y) = -2 ln2 kappa h (x - y) f(x, y) = sum_{m,n < q} d_mn T_m(x) T_n(y) + tail  (D antisymmetric)
// in z units (|G| <= e^-1/2), chosen like C: the smallest q whose tail is <= the tolerance.  Four launches:
//   (a) project  W^L_j, W^R_j as for the product (T(x)^T L, T(x)^T R, float64 block partials and, here, a float64
//                Chebyshev recurrence), to rank max(p, q)
//   (b) combine  U^R_j = scale D W^R_j, U^L_j = scale D W^L_j (float64), and gscale_jt = W^L_j[:,t]^T C W^R_j[:,t]
//   (c) output   gZ_ij = sum_m T_m(x_ij) q_m,  q_m = sum_t L_it U^R_j[m][t] + R_it U^L_j[m][t]  (float64, one Clenshaw sum);
//                the first workgroup also sums the gscale_jt in a fixed order
//
// Explicit features (rpgp_lowrank_post_select, rpgp_lowrank_features_f64, rpgp_lowrank_features_grad_f64): C = G G^T on the
// host, then B = sqrt(scale) [T(x_1) G | ... | T(x_J) G] and its adjoint in float64 on v_mfma_f64_16x16x4_f64.  Both kernels are
// one body (lr_features_body) with an epilogue each, for every padded rank 8 ... 128: G in static LDS up to 64, in dynamic LDS
// above.
//
// Ranks above 64 (plans of rpgp_lowrank_create_cap, up to 128): the kernels above keep one float64 value per rank and lane, which
// stops fitting the register file at 64, so padded ranks 72 ... 128 run forms of their own — the projection in two rank slices
// per row block (lrx_project_kernel), the product's output pass with a float64 Clenshaw sum (lrx_output_kernel), the
// derivative's with its sum split at 64 (lrgx_output_kernel) and its combine with the ranks as arguments (lrgx_combine_kernel).
// DESIGN.md 7.8.
//
// Panels (plans of rpgp_lowrank_create_panels): beyond the ranks the interval is cut into P equal panels instead, points of one
// panel and of neighbouring panels interact through forms of rank <= 64 and points further apart are dropped; the rows of every
// column are sorted by panel once per plan and the product and the derivative run kernels of their own (lrp_* / lrpg_*) over
// the sorted blocks, per panel, and in natural order.  DESIGN.md 7.9.
//
// Every kernel is templated on the padded rank; dispatch_pb turns the runtime value into the template argument.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"

namespace {

typedef float float2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

// rpgp_prepare's buffer (rpgp_kernels.hip): [header 64 floats][mid 64 floats][rowdat N*J float2 {a, exp2(-a^2)}][...]
constexpr int kPrepRowdatOffsetFloats = 128;
constexpr int kPrepMaxJ = 64;

constexpr int kRefDegree = 128;          // reference degree of the 2-D Chebyshev interpolant (rank selection)
constexpr int kMaxRank = 64;             // largest rank of a plan of rpgp_lowrank_create[_tol] (PB <= 64 accumulators per lane)
constexpr int kCapRank = 128;            // largest rank of a plan of rpgp_lowrank_create_cap (the lrx / lrgx kernels above 64)
constexpr double kTailTol = 1.0 / (1 << 26);
constexpr double kKappa = 0.84932180028801907;   // (2 ln 2)^-1/2
constexpr int kProjRowsPerThread = 8;    // pass (a): 2 048 rows per workgroup
constexpr int kProjRows = 256 * kProjRowsPerThread;
constexpr int kCombineBatch = 8;         // pass (b): block partials a thread requests before it adds the first
constexpr int kOutRows = 64;             // pass (c): 64 rows x 4 projection groups per workgroup

struct LowrankPlan {
  int p, pb;                             // rank and padded rank (multiple of 8)
  int64_t N;
  int J;
  double h, tail;
  const float *coef;                     // pb x pb, fp32, zero outside p x p
  const float *xt;                       // J x N coordinates x = a / h
  int q = 0, qb = 0;                     // derivative rank and padded rank (0: no derivative, see rpgp_lowrank_grad_prepare)
  const double *dcoef = nullptr;         // qb x qb, fp64 (in z units), zero outside q x q
  const double *ccoef = nullptr;         // pb x pb, fp64: the coefficients whose fp32 rounding is `coef` (gscale)
  double tol = 0.0;                      // the plan's tail tolerance
  int cap = kMaxRank;                    // largest rank the plan selects (rpgp_lowrank_create_cap: up to kCapRank)
  int ld = kMaxRank;                     // its buffers hold ld x ld coefficients: 64, or the padded cap above 64
  // a panel plan (rpgp_lowrank_create_panels; 0 panels: the single-interval plan above).  coef / dcoef / ccoef are then C0 / D0
  // / C0 in float64 at half-width hp, xt the LOCAL coordinates [J][N] in natural order
  int panels = 0;
  double hp = 0.0;                       // panel half-width h / panels
  int nbmax = 0;                         // projection blocks reserved per column: N / 2048 + panels
  const float *coef1 = nullptr;          // pb x pb, fp32: the neighbour form C1 (x in the lower panel, y in the upper)
  const uint8_t *pidx = nullptr;         // [J][N] panel of every (column, row), natural order
  const int *perm = nullptr;             // [J][nbmax 2048] rows in panel order, every (column, panel) padded to whole blocks: -1
  const float *xs = nullptr;             // [J][nbmax 2048] local coordinates in that order (0 in a padded slot)
  const int *bstart = nullptr;           // [J][panels + 1] first block of every panel; [panels]: the column's block count
  const double *dcoef1 = nullptr;        // qb x qb, fp64: D1
  const double *ccoef1 = nullptr;        // pb x pb, fp64: C1
  double bounds[3] = {0.0, 0.0, 0.0};    // per-entry bounds of the product: tail of C0, tail of C1, largest dropped value
  int q_sel = 0;                         // the derivative rank of the selection, and its float64 blocks (leading dimension
  std::vector<double> hd0, hd1, hc0, hc1;  // pad8(q_sel) / pb) kept on the host for rpgp_lowrank_grad_prepare
};

// side of the coefficient blocks of a plan with the rank cap `cap`: rpgp_lowrank_create's 64 up to there, the padded cap above
inline int cap_ld(int cap) { return cap <= kMaxRank ? kMaxRank : (cap + 7) & ~7; }

inline int pad8(int p) { return (p + 7) & ~7; }
inline int proj_blocks(int64_t N) { return (int)((N + kProjRows - 1) / kProjRows); }

// ---- rank selection (host, double) ------------------------------------------------------------------------------
// coefficients of the degree-(M-1) interpolant of f(x, y) = exp2(-h^2 (x - y)^2) at the M x M Chebyshev points of the
// first kind (a separable DCT-II), c[m * M + n]; deriv: of G(x, y) = -2 ln2 kappa h (x - y) f(x, y) instead, made exactly
// antisymmetric
void cheb2d_coefficients(double h, std::vector<double> &c, bool deriv = false) {
  const int M = kRefDegree;
  std::vector<double> xs(M), cs((size_t)M * M), f((size_t)M * M), g((size_t)M * M);
  for (int k = 0; k < M; ++k) xs[k] = cos(M_PI * (k + 0.5) / M);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < M; ++k) cs[(size_t)m * M + k] = cos(M_PI * m * (k + 0.5) / M);
  const double h2 = h * h;
  for (int k = 0; k < M; ++k)
    for (int l = 0; l <= k; ++l) {
      const double d = xs[k] - xs[l];
      if (!deriv) {
        f[(size_t)k * M + l] = f[(size_t)l * M + k] = exp2(-h2 * d * d);
      } else {
        const double v = -2.0 * M_LN2 * kKappa * h * d * exp2(-h2 * d * d);
        f[(size_t)k * M + l] = v;
        f[(size_t)l * M + k] = -v;
      }
    }
  // g[k][n] = sum_l f[k][l] cos_n(l);  c[m][n] = sum_k cos_m(k) g[k][n]
  for (int k = 0; k < M; ++k)
    for (int n = 0; n < M; ++n) {
      double s = 0.0;
      for (int l = 0; l < M; ++l) s += f[(size_t)k * M + l] * cs[(size_t)n * M + l];
      g[(size_t)k * M + n] = s;
    }
  c.assign((size_t)M * M, 0.0);
  for (int m = 0; m < M; ++m) {
    for (int k = 0; k < M; ++k) {
      const double w = cs[(size_t)m * M + k];
      for (int n = 0; n < M; ++n) c[(size_t)m * M + n] += w * g[(size_t)k * M + n];
    }
    const double wm = (m == 0 ? 1.0 : 2.0) / M;
    for (int n = 0; n < M; ++n) c[(size_t)m * M + n] *= wm * (n == 0 ? 1.0 : 2.0) / M;
  }
  if (deriv)
    for (int m = 0; m < M; ++m) {
      c[(size_t)m * M + m] = 0.0;
      for (int n = 0; n < m; ++n) {
        const double a = 0.5 * (c[(size_t)m * M + n] - c[(size_t)n * M + m]);
        c[(size_t)m * M + n] = a;
        c[(size_t)n * M + m] = -a;
      }
    }
}

// smallest p with sum_{max(m,n) >= p} |c_mn| <= tol; 0 when the reference degree does not resolve f or p > p_max.
// `tail` receives the bound of the chosen p (plus a rounding allowance of the fp64 transform).
int select_rank(double h, int p_max, double tol, double *tail, std::vector<double> &c, bool deriv = false) {
  const int M = kRefDegree;
  if (!(h >= 0.0) || !isfinite(h)) return 0;
  cheb2d_coefficients(h, c, deriv);
  // shell sums: s[q] = sum_{max(m,n) == q} |c_mn|
  std::vector<double> shell(M, 0.0);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < M; ++n) shell[m > n ? m : n] += fabs(c[(size_t)m * M + n]);
  double unresolved = 0.0;                 // the last 8 shells: must be at the rounding level of the transform
  for (int q = M - 8; q < M; ++q) unresolved += shell[q];
  if (unresolved > 1e-11) return 0;
  const double allowance = 1e-13 + unresolved;
  double t = 0.0;
  int p = M;
  for (int q = M - 1; q >= 1; --q) {       // tail of p = q is the sum of the shells q .. M-1
    if (t + shell[q] + allowance > tol) break;
    t += shell[q];
    p = q;
  }
  if (p > p_max) return 0;
  if (tail) *tail = t + allowance;
  return p;
}

// ---- device -----------------------------------------------------------------------------------------------------
// one DPP move of a float64 (two 32-bit halves)
template <int CTRL> __device__ __forceinline__ double dpp_d(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// sum over the 64 lanes of a wave, the same value in every lane: quad / half-row / row by DPP, then the four rows
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_d<0xb1>(v);    // quad_perm [1,0,3,2]
  v += dpp_d<0x4e>(v);    // quad_perm [2,3,0,1]
  v += dpp_d<0x141>(v);   // row_half_mirror
  v += dpp_d<0x140>(v);   // row_mirror
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}

// plan: xt[j][n] = a_nj * inv_h
__global__ __launch_bounds__(256) void lr_coords_kernel(const float2v *__restrict__ rowdat, float *__restrict__ xt,
                                                        long long N, int J, float inv_h) {
  const long long total = N * J;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const int j = (int)(g / N);
    const long long n = g - (long long)j * N;
    xt[g] = rowdat[n * J + j].x * inv_h;
  }
}

// One level of a transposed wave reduction: a + b after the exchange is, in the lanes that keep `a`, the sum of a over the lane
// and its partner, in the other lanes that of b.  HALF = 32: lanes 0-31 keep a, partner l ^ 32 (v_permlane32_swap: lanes 32-63
// of the first operand change places with lanes 0-31 of the second); HALF = 16: the even rows of 16 keep a, partner l ^ 16
// (v_permlane16_swap: odd rows of the first with even rows of the second).  3 instructions for two values where two butterflies
// take 6, and half as many values are live afterwards.
template <int HALF> __device__ __forceinline__ double swap_add(double a, double b) {
  const unsigned long long ab = __builtin_bit_cast(unsigned long long, a), bb = __builtin_bit_cast(unsigned long long, b);
  unsigned alo, blo, ahi, bhi;
  if constexpr (HALF == 32) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ab, (unsigned)bb, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ab >> 32), (unsigned)(bb >> 32), false, false);
    alo = lo[0], blo = lo[1], ahi = hi[0], bhi = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)ab, (unsigned)bb, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(ab >> 32), (unsigned)(bb >> 32), false, false);
    alo = lo[0], blo = lo[1], ahi = hi[0], bhi = hi[1];
  }
  return __builtin_bit_cast(double, ((unsigned long long)ahi << 32) | alo) +
         __builtin_bit_cast(double, ((unsigned long long)bhi << 32) | blo);
}

// (a) block partials part[b][jj][t][0..PB) = sum over the block's rows of T_m(x_ij) v_it.  grid (row blocks, jn, T)
// The sums are float64 (T_m v exact, then added): W is a sum of N terms of both signs that C turns into a much smaller
// product — in float32 its rounding alone is ~1e-6 of the result (measured in an emulation at N = 20 011), in float64 ~3e-8.
// The recurrence runs in float64 too: x and v are widened once per row, then each m is two v_fma_f64 (T_m, then the sum) and no
// conversion; a float32 recurrence cost a v_fma_f32 and a v_cvt_f64_f32 per m beside the float64 accumulate.
// The 64 lanes' PB accumulators are summed transposed: two exchange levels (lane ^ 32, lane ^ 16) halve the live values each,
// leaving PB / 4 per lane (row r of 16 lanes holds m = r PB / 4 + i), which four DPP steps sum inside the row: ~5 PB
// instructions per wave where PB butterflies took ~23 PB.  The order of the additions is a function of PB alone.
// PB = 40: 108 VGPR, PB = 48: 123, PB = 64: 155 (two more than with the float32 recurrence, the same waves per SIMD); no scratch.
template <int PB>
__global__ __launch_bounds__(256) void lr_project_kernel(const float *__restrict__ xt, const float *__restrict__ V,
                                                         double *__restrict__ part, int N, int T, int j0, int jn) {
  __shared__ double red[4 * PB];
  const int b = blockIdx.x, jj = blockIdx.y, t = blockIdx.z;
  const float *x = xt + (size_t)(j0 + jj) * N;
  const int r0 = b * kProjRows + (int)threadIdx.x;
  float xv[kProjRowsPerThread], vv[kProjRowsPerThread];
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {          // every load requested before the first use: no branch around a
    const int i = r0 + u * 256, ic = i < N ? i : N - 1;   // load (a row past N reads row N - 1 and counts with v = 0)
    xv[u] = x[ic];
    vv[u] = V[(size_t)ic * T + t];
  }
  __builtin_amdgcn_sched_barrier(0);                      // (the scheduler would sink each load to one row ahead of its use)
  double acc[PB];
#pragma unroll
  for (int m = 0; m < PB; ++m) acc[m] = 0.0;
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    const double xi = (double)xv[u], v = r0 + u * 256 < N ? (double)vv[u] : 0.0, x2 = 2.0 * xi;
    double tm2 = 1.0, tm1 = xi;
    acc[0] += v;
    acc[1] = __builtin_fma(xi, v, acc[1]);
#pragma unroll
    for (int m = 2; m < PB; ++m) {
      const double tm = __builtin_fma(x2, tm1, -tm2);     // T_m = 2x T_{m-1} - T_{m-2}
      acc[m] = __builtin_fma(tm, v, acc[m]);
      tm2 = tm1;
      tm1 = tm;
    }
  }
  constexpr int QB = PB / 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < PB / 2; ++i) acc[i] = swap_add<32>(acc[i], acc[i + PB / 2]);
#pragma unroll
  for (int i = 0; i < QB; ++i) {
    double s = swap_add<16>(acc[i], acc[i + QB]);
    s += dpp_d<0xb1>(s);    // quad_perm [1,0,3,2]
    s += dpp_d<0x4e>(s);    // quad_perm [2,3,0,1]
    s += dpp_d<0x141>(s);   // row_half_mirror
    s += dpp_d<0x140>(s);   // row_mirror
    if ((lane & 15) == i) red[w * PB + QB * (lane >> 4) + i] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    const int m = threadIdx.x;
    part[(((size_t)b * jn + jj) * T + t) * PB + m] = (red[m] + red[PB + m]) + (red[2 * PB + m] + red[3 * PB + m]);
  }
}

// (b) U[jj][t][m] = scale * sum_n c_mn W[n],  W[n] = sum_b part[b][jj][t][n] (float64, U rounded to float32 at the end).
// grid (jn, T).  Thread (g, n) of the G = 256 / PB groups adds the blocks b = g, g + G, ... in that order and the groups' sums
// are added in the order g = 0 ... G - 1.  The product with C is split the same way: thread (g, m) takes the CH columns
// n = g CH ... of row m in ascending order (CH = PB / G rounded up to a multiple of 4), and the NCH chunk sums are added in the
// order g = 0 ... NCH - 1.  The order of every addition is fixed by (nblk, PB) alone.
// One round trip: a thread requests a batch of kCombineBatch partials (a block past nblk re-reads block nblk - 1 and counts
// as 0) and its CH coefficients (CH / 4 dwordx4 loads, a chunk past the row's end re-reads the row's last four and is not
// used) before the first add; nblk <= kCombineBatch G needs no further load, a longer sum loops over batches.  A whole
// coefficient row per thread would be one chunk less in LDS, but its PB registers cost occupancy from PB = 24 on.
template <int PB>
__global__ __launch_bounds__(256) void lr_combine_kernel(const double *__restrict__ part, const float *__restrict__ coef,
                                                         float *__restrict__ U, int nblk, int T, int jn, float scale) {
  constexpr int G = 256 / PB;
  constexpr int CH = ((PB + G - 1) / G + 3) & ~3, NCH = (PB + CH - 1) / CH;
  static_assert(NCH <= G, "a chunk of the coefficient row per group");
  __shared__ double sw[G][PB];
  __shared__ double w[PB];
  const int jj = blockIdx.x, t = blockIdx.y;
  const int n = threadIdx.x % PB, g = threadIdx.x / PB;
  const size_t bstride = (size_t)jn * T * PB;
  const double *p = part + ((size_t)jj * T + t) * PB + n;
  double pv[kCombineBatch];
#pragma unroll
  for (int k = 0; k < kCombineBatch; ++k) {
    const int b = g + k * G;
    pv[k] = p[(size_t)(b < nblk ? b : nblk - 1) * bstride];
  }
  float4v c[CH / 4];
#pragma unroll
  for (int k = 0; k < CH / 4; ++k) {
    const int col = g * CH + 4 * k;
    c[k] = *reinterpret_cast<const float4v *>(coef + n * PB + (col < PB ? col : PB - 4));
  }
  __builtin_amdgcn_sched_barrier(0);                      // (every load above is in flight before the first add)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kCombineBatch; ++k) s += g + k * G < nblk ? pv[k] : 0.0;
  for (int b0 = g + kCombineBatch * G; b0 < nblk; b0 += kCombineBatch * G) {
#pragma unroll
    for (int k = 0; k < kCombineBatch; ++k) {
      const int b = b0 + k * G;
      pv[k] = p[(size_t)(b < nblk ? b : nblk - 1) * bstride];
    }
#pragma unroll
    for (int k = 0; k < kCombineBatch; ++k) s += b0 + k * G < nblk ? pv[k] : 0.0;
  }
  if (g < G) sw[g][n] = s;
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    double a = sw[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < G; ++q) a += sw[q][threadIdx.x];
    w[threadIdx.x] = a;
  }
  __syncthreads();
  if (g < NCH) {                                          // (sw is free again: its readers are past the barrier)
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int col = g * CH + k;
      if (col < PB) a = __builtin_fma((double)c[k >> 2][k & 3], w[col], a);
    }
    sw[g][n] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    const int m = threadIdx.x;
    double a = sw[0][m];
#pragma unroll
    for (int q = 1; q < NCH; ++q) a += sw[q][m];
    U[((size_t)jj * T + t) * PB + m] = (float)((double)scale * a);
  }
}

// (c) out_it = sum_j sum_m T_m(x_ij) U[j][t][m] + noise v_it on this rank's rows [r0, r1); noise v_it (or 0) elsewhere.
// A workgroup: 64 rows x 4 groups of projections (wave g takes jj = g, g + 4, ...), the groups' sums added in order.
// Every global load is requested before the first wait, in this order: the lane's coordinates (unconditional, on a row clamped
// into this rank's slice and into [0, N - 1], behind the wave-uniform jj < jn only), wave 0's V[o] for the noise term, then the
// thread's share of U as dwordx4 loads (at most kTrips, a wave whose share lies past jn PB skips the trip).  Then U goes to
// LDS, one barrier, and the Clenshaw sums.  A row outside the slice computes on a clamped coordinate and is replaced by 0
// at the end; V[o] is read by the thread that later writes out[o], so out may alias V.
// (The dwordx4 loads of U are 16-byte aligned when the caller's workspace is, as hipMalloc's and torch's are: U lies a
// multiple of 64 bytes behind it.  Behind an 8-byte aligned workspace they are unaligned loads, which gfx950 serves.)
// grid (row blocks of 64, T)
template <int PB>
__global__ __launch_bounds__(256) void lr_output_kernel(const float *__restrict__ xt, const float *__restrict__ U,
                                                        const float *__restrict__ V, float *__restrict__ out, int N, int T,
                                                        int j0, int jn, int r0, int r1, float noise) {
  __shared__ __attribute__((aligned(16))) float su[kPrepMaxJ * PB];
  __shared__ float sacc[4][kOutRows];
  const int t = blockIdx.y;
  const int r = threadIdx.x & (kOutRows - 1), g = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int i = blockIdx.x * kOutRows + r;
  const bool mine = i >= r0 && i < r1;
  int ic = i > r0 ? i : r0;
  ic = ic < r1 ? ic : r1 - 1;
  ic = ic < N ? ic : N - 1;
  ic = ic > 0 ? ic : 0;
  constexpr int kMaxPer = kPrepMaxJ / 4;
  float xv[kMaxPer];
#pragma unroll
  for (int q = 0; q < kMaxPer; ++q) {
    const int jj = g + 4 * q;
    xv[q] = jj < jn ? xt[(size_t)(j0 + jj) * N + ic] : 0.f;
  }
  float vn = 0.f;
  if (g == 0 && noise != 0.f) vn = V[(size_t)(i < N ? i : N - 1) * T + t];
  constexpr int kTrips = (kPrepMaxJ * PB / 4 + 255) / 256;
  const int nu4 = jn * (PB / 4);                          // U[.][t][.] of the jn projections as float4
  float4v uv[kTrips];
#pragma unroll
  for (int k = 0; k < kTrips; ++k)
    if (g * kOutRows + 256 * k < nu4) {
      const int e = (int)threadIdx.x + 256 * k, ec = e < nu4 ? e : nu4 - 1;
      uv[k] = *reinterpret_cast<const float4v *>(U + ((size_t)(ec / (PB / 4)) * T + t) * PB + 4 * (ec % (PB / 4)));
    }
  __builtin_amdgcn_sched_barrier(0);                      // (every load above is in flight before the first wait)
#pragma unroll
  for (int k = 0; k < kTrips; ++k)
    if (g * kOutRows + 256 * k < nu4) {
      const int e = (int)threadIdx.x + 256 * k;
      if (e < nu4) *reinterpret_cast<float4v *>(su + 4 * e) = uv[k];
    }
  __syncthreads();
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < kMaxPer; ++q) {
    const int jj = g + 4 * q;
    if (jj >= jn) break;
    const float *u = su + jj * PB;
    const float x = xv[q], x2 = 2.f * x;
    float b1 = 0.f, b2 = 0.f;                             // Clenshaw: b_k = U_k + 2x b_{k+1} - b_{k+2}
#pragma unroll
    for (int k = PB - 1; k >= 1; --k) {
      const float bk = __builtin_fmaf(x2, b1, u[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    acc += __builtin_fmaf(x, b1, u[0] - b2);
  }
  sacc[g][r] = acc;
  __syncthreads();
  if (g != 0 || i >= N) return;
  float res = mine ? (sacc[0][r] + sacc[1][r]) + (sacc[2][r] + sacc[3][r]) : 0.f;
  if (noise != 0.f) res = __builtin_fmaf(noise, vn, res);
  out[(size_t)i * T + t] = res;
}

// ---- per-component weights (rpgp_mvm_sym_lowrank_weighted: the RBF, group-1 members of rpgp_family) ---------------------------
// K = scale sum_j w_j K_j is linear in the weights and every K_j shares the plan's one form, so w_j enters the product in
// exactly one place: pass (b) of projection j.  The kernels below are lr_combine_kernel, lrg_combine_kernel and
// lrg_output_kernel with that factor (and, for the derivative, one sum per component in place of the single gscale); they are
// kernels of their own, not a template argument of the unweighted ones, so that those keep their names and their code.
// Every launcher takes the weights as a nullable pointer and launches these kernels when it is given one.
//
// (b) U[jj][t][m] = (scale w[j0 + jj]) * sum_n c_mn W[n]: lr_combine_kernel's loads, block-partial order, chunking and single
// round trip, with the weight requested beside the partials and the factor scale * w formed in float64 (w = 1: the same bits).
// `w` points at the weight of projection j0.
template <int PB>
__global__ __launch_bounds__(256) void lrw_combine_kernel(const double *__restrict__ part, const float *__restrict__ coef,
                                                          const float *__restrict__ w, float *__restrict__ U, int nblk, int T,
                                                          int jn, float scale) {
  constexpr int G = 256 / PB;
  constexpr int CH = ((PB + G - 1) / G + 3) & ~3, NCH = (PB + CH - 1) / CH;
  static_assert(NCH <= G, "a chunk of the coefficient row per group");
  __shared__ double sw[G][PB];
  __shared__ double ws[PB];
  const int jj = blockIdx.x, t = blockIdx.y;
  const int n = threadIdx.x % PB, g = threadIdx.x / PB;
  const size_t bstride = (size_t)jn * T * PB;
  const double *p = part + ((size_t)jj * T + t) * PB + n;
  double pv[kCombineBatch];
#pragma unroll
  for (int k = 0; k < kCombineBatch; ++k) {
    const int b = g + k * G;
    pv[k] = p[(size_t)(b < nblk ? b : nblk - 1) * bstride];
  }
  float4v c[CH / 4];
#pragma unroll
  for (int k = 0; k < CH / 4; ++k) {
    const int col = g * CH + 4 * k;
    c[k] = *reinterpret_cast<const float4v *>(coef + n * PB + (col < PB ? col : PB - 4));
  }
  const float wj = w[jj];
  __builtin_amdgcn_sched_barrier(0);                      // (every load above is in flight before the first add)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kCombineBatch; ++k) s += g + k * G < nblk ? pv[k] : 0.0;
  for (int b0 = g + kCombineBatch * G; b0 < nblk; b0 += kCombineBatch * G) {
#pragma unroll
    for (int k = 0; k < kCombineBatch; ++k) {
      const int b = b0 + k * G;
      pv[k] = p[(size_t)(b < nblk ? b : nblk - 1) * bstride];
    }
#pragma unroll
    for (int k = 0; k < kCombineBatch; ++k) s += b0 + k * G < nblk ? pv[k] : 0.0;
  }
  if (g < G) sw[g][n] = s;
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    double a = sw[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < G; ++q) a += sw[q][threadIdx.x];
    ws[threadIdx.x] = a;
  }
  __syncthreads();
  if (g < NCH) {                                          // (sw is free again: its readers are past the barrier)
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int col = g * CH + k;
      if (col < PB) a = __builtin_fma((double)c[k >> 2][k & 3], ws[col], a);
    }
    sw[g][n] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    const int m = threadIdx.x;
    double a = sw[0][m];
#pragma unroll
    for (int q = 1; q < NCH; ++q) a += sw[q][m];
    U[((size_t)jj * T + t) * PB + m] = (float)(((double)scale * (double)wj) * a);
  }
}

// the product at a padded rank up to 64.  w: the weights (rpgp_mvm_sym_lowrank_weighted) or null; [r0, r1): the rows written
template <int PB>
int launch_lowrank(const LowrankPlan &P, const float *w, const float *V, float *out, int N, int T, int j0, int jn, int r0,
                   int r1, float scale, float noise, double *part, float *U, hipStream_t st) {
  const int nblk = proj_blocks(N);
  hipLaunchKernelGGL(lr_project_kernel<PB>, dim3(nblk, jn, T), dim3(256), 0, st, P.xt, V, part, N, T, j0, jn);
  if (w)
    hipLaunchKernelGGL(lrw_combine_kernel<PB>, dim3(jn, T), dim3(256), 0, st, part, P.coef, w + j0, U, nblk, T, jn, scale);
  else
    hipLaunchKernelGGL(lr_combine_kernel<PB>, dim3(jn, T), dim3(256), 0, st, part, P.coef, U, nblk, T, jn, scale);
  hipLaunchKernelGGL(lr_output_kernel<PB>, dim3((N + kOutRows - 1) / kOutRows, T), dim3(256), 0, st, P.xt, U, V, out, N, T,
                     j0, jn, r0, r1, noise);
  return (int)hipGetLastError();
}


// ---- bilinear derivative ----------------------------------------------------------------------------------------
// (a) lr_project_kernel with the Chebyshev recurrence in float64: near |x| = 1 the fp32 recurrence's error grows with m, which
// the derivative (ranks up to 64, a bilinear gscale without the product's noise term) does not absorb.  Same layout and order.
template <int PB>
__global__ __launch_bounds__(256) void lrg_project_kernel(const float *__restrict__ xt, const float *__restrict__ V,
                                                          double *__restrict__ part, int N, int T, int j0, int jn) {
  __shared__ double red[4][PB];
  const int b = blockIdx.x, jj = blockIdx.y, t = blockIdx.z;
  const float *x = xt + (size_t)(j0 + jj) * N;
  const int r0 = b * kProjRows + (int)threadIdx.x;
  float xv[kProjRowsPerThread], vv[kProjRowsPerThread];
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    const int i = r0 + u * 256;
    const bool ok = i < N;
    xv[u] = ok ? x[i] : 0.f;
    vv[u] = ok ? V[(size_t)i * T + t] : 0.f;
  }
  double acc[PB];
#pragma unroll
  for (int m = 0; m < PB; ++m) acc[m] = 0.0;
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    const double xi = xv[u], v = vv[u], x2 = 2.0 * xi;
    double tm2 = 1.0, tm1 = xi;
    acc[0] += v;
    acc[1] = __builtin_fma(xi, v, acc[1]);
#pragma unroll
    for (int m = 2; m < PB; ++m) {
      const double tm = __builtin_fma(x2, tm1, -tm2);
      acc[m] = __builtin_fma(tm, v, acc[m]);
      tm2 = tm1;
      tm1 = tm;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < PB; ++m) {
    const double s = wave_sum(acc[m]);
    if (lane == 0) red[w][m] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    const int m = threadIdx.x;
    part[(((size_t)b * jn + jj) * T + t) * PB + m] = (red[0][m] + red[1][m]) + (red[2][m] + red[3][m]);
  }
}

// (b) per (projection, t): W^L, W^R summed over the row blocks in a fixed order (float64, as lr_combine_kernel), then
//   U[jj][t][0][m] = scale sum_n d_mn W^R[n],  U[jj][t][1][m] = scale sum_n d_mn W^L[n]   (float64, m < QB)
//   gsp[jj][t]     = sum_{m,n < p} W^L[m] c_mn W^R[n]   (the product's coefficients in float64, leading dimension pc)
// partL / partR: [b][jj][t][PB] (PB >= QB and >= p).  grid (jn, T)
template <int PB, int QB>
__global__ __launch_bounds__(256) void lrg_combine_kernel(const double *__restrict__ partL, const double *__restrict__ partR,
                                                          const double *__restrict__ dcoef, const double *__restrict__ ccoef,
                                                          double *__restrict__ U, double *__restrict__ gsp, int nblk, int T,
                                                          int jn, int p, int pc, double scale) {
  constexpr int G = 256 / PB;
  __shared__ double sw[2][G][PB];
  __shared__ double w[2][PB];
  __shared__ double cw[PB];
  const int jj = blockIdx.x, t = blockIdx.y;
  const int n = threadIdx.x % PB, g = threadIdx.x / PB;
  if (g < G) {
    double sl = 0.0, sr = 0.0;
    for (int b = g; b < nblk; b += G) {
      const size_t o = (((size_t)b * jn + jj) * T + t) * PB + n;
      sl += partL[o];
      sr += partR[o];
    }
    sw[0][g][n] = sl;
    sw[1][g][n] = sr;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    double sl = sw[0][0][threadIdx.x], sr = sw[1][0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < G; ++k) {
      sl += sw[0][k][threadIdx.x];
      sr += sw[1][k][threadIdx.x];
    }
    w[0][threadIdx.x] = sl;
    w[1][threadIdx.x] = sr;
  }
  __syncthreads();
  const int m = threadIdx.x;
  if (m < QB) {
    double ur = 0.0, ul = 0.0;
#pragma unroll 8
    for (int k = 0; k < QB; ++k) {
      const double d = dcoef[m * QB + k];
      ur = __builtin_fma(d, w[1][k], ur);
      ul = __builtin_fma(d, w[0][k], ul);
    }
    double *u = U + ((size_t)jj * T + t) * 2 * QB;
    u[m] = scale * ur;
    u[QB + m] = scale * ul;
  }
  if (m < PB) {                                           // (C W^R)[m], zero beyond p
    double s = 0.0;
    if (m < p)
      for (int k = 0; k < p; ++k) s = __builtin_fma(ccoef[m * pc + k], w[1][k], s);
    cw[m] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < p; ++k) s = __builtin_fma(w[0][k], cw[k], s);
    gsp[(size_t)jj * T + t] = s;
  }
}

// (c) gZ[i][j0 + jj] = sum_m T_m(x_ij) q_m,  q_m = sum_t L_it U[jj][t][0][m] + R_it U[jj][t][1][m]  (float64 fold, Clenshaw).
// A workgroup: 64 rows x 4 waves, wave w takes jj = w, w + 4, ...; the results are staged in LDS and written row by row.
// Workgroup (0, 0) also writes gscale = sum_jj sum_t gsp[jj][t] (fixed order).  grid (row blocks of 64)
template <int QB>
__global__ __launch_bounds__(256) void lrg_output_kernel(const float *__restrict__ xt, const double *__restrict__ U,
                                                         const double *__restrict__ gsp, const float *__restrict__ L,
                                                         const float *__restrict__ R, float *__restrict__ gZ,
                                                         float *__restrict__ gscale, int N, int T, int j0, int jn, int ldg) {
  __shared__ float sres[kOutRows][kPrepMaxJ + 1];
  const int r = threadIdx.x & (kOutRows - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int row0 = blockIdx.x * kOutRows;
  const int i = row0 + r;
  const bool ok = i < N;
  for (int jj = wv; jj < jn; jj += 4) {
    const double *u = U + (size_t)jj * T * 2 * QB;
    double q[QB];
#pragma unroll
    for (int m = 0; m < QB; ++m) q[m] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double l = ok ? (double)L[(size_t)i * T + t] : 0.0;
      const double rr = ok ? (double)R[(size_t)i * T + t] : 0.0;
      const double *ut = u + (size_t)t * 2 * QB;
#pragma unroll
      for (int m = 0; m < QB; ++m) q[m] = __builtin_fma(l, ut[m], __builtin_fma(rr, ut[QB + m], q[m]));
    }
    const double x = ok ? (double)xt[(size_t)(j0 + jj) * N + i] : 0.0, x2 = 2.0 * x;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = QB - 1; k >= 1; --k) {
      const double bk = __builtin_fma(x2, b1, q[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    sres[r][jj] = (float)__builtin_fma(x, b1, q[0] - b2);
  }
  __syncthreads();
  const int rows = N - row0 < kOutRows ? N - row0 : kOutRows;
  for (int e = threadIdx.x; e < rows * jn; e += 256) {
    const int rr = e / jn, c = e - rr * jn;
    gZ[(size_t)(row0 + rr) * ldg + j0 + c] = sres[rr][c];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < jn * T; ++k) s += gsp[k];
    *gscale = (float)s;
  }
}

inline int grad_pb(const LowrankPlan &P) { return pad8(P.q > P.p ? P.q : P.p); }

// workspace of the derivative: partL, partR (nblk x jn x T x PB doubles each), U (jn x T x 2 x QB doubles), gsp (jn x T)
inline size_t grad_ws_bytes(const LowrankPlan &P, int64_t N, int jn, int T) {
  return ((size_t)proj_blocks(N) * jn * T * grad_pb(P) * 2 + (size_t)jn * T * 2 * P.qb + (size_t)jn * T) * sizeof(double);
}

// The weighted derivative (rpgp_bilinear_grad_lowrank_weighted).  (b) is lrg_combine_kernel with U^R, U^L carrying
// scale * w[j0 + jj] (float64; w = 1: the same bits) and gsp left as it is, the UNWEIGHTED W^L^T C W^R of the component.
// `w` points at the weight of projection j0.
template <int PB, int QB>
__global__ __launch_bounds__(256) void lrgw_combine_kernel(const double *__restrict__ partL, const double *__restrict__ partR,
                                                           const double *__restrict__ dcoef, const double *__restrict__ ccoef,
                                                           const float *__restrict__ wt, double *__restrict__ U,
                                                           double *__restrict__ gsp, int nblk, int T, int jn, int p, int pc,
                                                           double scale) {
  constexpr int G = 256 / PB;
  __shared__ double sw[2][G][PB];
  __shared__ double w[2][PB];
  __shared__ double cw[PB];
  const int jj = blockIdx.x, t = blockIdx.y;
  const int n = threadIdx.x % PB, g = threadIdx.x / PB;
  const double sj = scale * (double)wt[jj];
  if (g < G) {
    double sl = 0.0, sr = 0.0;
    for (int b = g; b < nblk; b += G) {
      const size_t o = (((size_t)b * jn + jj) * T + t) * PB + n;
      sl += partL[o];
      sr += partR[o];
    }
    sw[0][g][n] = sl;
    sw[1][g][n] = sr;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    double sl = sw[0][0][threadIdx.x], sr = sw[1][0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < G; ++k) {
      sl += sw[0][k][threadIdx.x];
      sr += sw[1][k][threadIdx.x];
    }
    w[0][threadIdx.x] = sl;
    w[1][threadIdx.x] = sr;
  }
  __syncthreads();
  const int m = threadIdx.x;
  if (m < QB) {
    double ur = 0.0, ul = 0.0;
#pragma unroll 8
    for (int k = 0; k < QB; ++k) {
      const double d = dcoef[m * QB + k];
      ur = __builtin_fma(d, w[1][k], ur);
      ul = __builtin_fma(d, w[0][k], ul);
    }
    double *u = U + ((size_t)jj * T + t) * 2 * QB;
    u[m] = sj * ur;
    u[QB + m] = sj * ul;
  }
  if (m < PB) {                                           // (C W^R)[m], zero beyond p
    double s = 0.0;
    if (m < p)
      for (int k = 0; k < p; ++k) s = __builtin_fma(ccoef[m * pc + k], w[1][k], s);
    cw[m] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < p; ++k) s = __builtin_fma(w[0][k], cw[k], s);
    gsp[(size_t)jj * T + t] = s;
  }
}

// (c) is lrg_output_kernel with one sum per component in place of the single gscale: thread jj < jn of workgroup 0 writes
// gcomp[j0 + jj] = sum_t gsp[jj][t] (float64, t ascending; jn <= 64 < 256 threads), rpgp_family_bilinear_grad's unweighted sums.
// gZ has the leading dimension J of the plan.  grid (row blocks of 64)
template <int QB>
__global__ __launch_bounds__(256) void lrgw_output_kernel(const float *__restrict__ xt, const double *__restrict__ U,
                                                          const double *__restrict__ gsp, const float *__restrict__ L,
                                                          const float *__restrict__ R, float *__restrict__ gZ,
                                                          float *__restrict__ gcomp, int N, int T, int j0, int jn, int ldg) {
  __shared__ float sres[kOutRows][kPrepMaxJ + 1];
  const int r = threadIdx.x & (kOutRows - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int row0 = blockIdx.x * kOutRows;
  const int i = row0 + r;
  const bool ok = i < N;
  for (int jj = wv; jj < jn; jj += 4) {
    const double *u = U + (size_t)jj * T * 2 * QB;
    double q[QB];
#pragma unroll
    for (int m = 0; m < QB; ++m) q[m] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double l = ok ? (double)L[(size_t)i * T + t] : 0.0;
      const double rr = ok ? (double)R[(size_t)i * T + t] : 0.0;
      const double *ut = u + (size_t)t * 2 * QB;
#pragma unroll
      for (int m = 0; m < QB; ++m) q[m] = __builtin_fma(l, ut[m], __builtin_fma(rr, ut[QB + m], q[m]));
    }
    const double x = ok ? (double)xt[(size_t)(j0 + jj) * N + i] : 0.0, x2 = 2.0 * x;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = QB - 1; k >= 1; --k) {
      const double bk = __builtin_fma(x2, b1, q[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    sres[r][jj] = (float)__builtin_fma(x, b1, q[0] - b2);
  }
  __syncthreads();
  const int rows = N - row0 < kOutRows ? N - row0 : kOutRows;
  for (int e = threadIdx.x; e < rows * jn; e += 256) {
    const int rr = e / jn, c = e - rr * jn;
    gZ[(size_t)(row0 + rr) * ldg + j0 + c] = sres[rr][c];
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < jn) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += gsp[(size_t)threadIdx.x * T + t];
    gcomp[j0 + threadIdx.x] = (float)s;
  }
}

// the derivative at padded ranks up to 64.  w: the weights (gout = gcomp) or null (gout = gscale)
template <int PB, int QB>
int launch_grad(const LowrankPlan &P, const float *w, const float *L, const float *R, float *gZ, float *gout, int N, int ldg,
                int T, int j0, int jn, float scale, void *ws, hipStream_t st) {
  const int nblk = proj_blocks(N);
  const size_t np = (size_t)nblk * jn * T * PB;
  double *partL = reinterpret_cast<double *>(ws), *partR = partL + np;
  double *U = partR + np, *gsp = U + (size_t)jn * T * 2 * QB;
  const dim3 rows((N + kOutRows - 1) / kOutRows);
  hipLaunchKernelGGL(lrg_project_kernel<PB>, dim3(nblk, jn, T), dim3(256), 0, st, P.xt, L, partL, N, T, j0, jn);
  hipLaunchKernelGGL(lrg_project_kernel<PB>, dim3(nblk, jn, T), dim3(256), 0, st, P.xt, R, partR, N, T, j0, jn);
  if (w) {
    hipLaunchKernelGGL((lrgw_combine_kernel<PB, QB>), dim3(jn, T), dim3(256), 0, st, partL, partR, P.dcoef, P.ccoef, w + j0, U,
                       gsp, nblk, T, jn, P.p, P.pb, (double)scale);
    hipLaunchKernelGGL(lrgw_output_kernel<QB>, rows, dim3(256), 0, st, P.xt, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg);
  } else {
    hipLaunchKernelGGL((lrg_combine_kernel<PB, QB>), dim3(jn, T), dim3(256), 0, st, partL, partR, P.dcoef, P.ccoef, U, gsp, nblk,
                       T, jn, P.p, P.pb, (double)scale);
    hipLaunchKernelGGL(lrg_output_kernel<QB>, rows, dim3(256), 0, st, P.xt, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg);
  }
  return (int)hipGetLastError();
}

// ---- padded ranks 72 ... 128 of the product and the derivative (plans of rpgp_lowrank_create_cap) ---------------------------
// The kernels above keep PB (or QB) float64 values per lane, two VGPRs each: 155 VGPRs at 64, more than the register file at
// 128.  The kernels below are their forms for 64 < PB <= 128, kernels of their own so that every kernel above keeps its code.
//
// (a) One kernel for the product and the derivative.  A workgroup owns a rank slice of a row block: slice 0 the ranks
// [0, 64), slice 1 the ranks [64, PB) (8 ... 64 of them).  It runs the float64 recurrence up to its slice's upper end — one
// v_fma_f64 per rank below the slice — and accumulates its own slice only, so a lane holds at most 64 accumulators, and then
// reduces them with lr_project_kernel's transposed exchange at the slice's offset.  The order of every addition is a function
// of PB alone; part[b][jj][t][PB] as above.  The slice is the low bit of blockIdx.x (the z dimension is T, up to 65 535).
template <int LO, int CNT, int PB>
__device__ __forceinline__ void lrx_project_slice(const float (&xv)[kProjRowsPerThread], const float (&vv)[kProjRowsPerThread],
                                                  int r0, int N, double *__restrict__ red, double *__restrict__ dst) {
  static_assert(CNT >= 8 && CNT <= 64 && CNT % 8 == 0 && LO + CNT == (LO ? PB : 64), "a slice of at most 64 ranks");
  double acc[CNT];
#pragma unroll
  for (int m = 0; m < CNT; ++m) acc[m] = 0.0;
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    const double xi = (double)xv[u], v = r0 + u * 256 < N ? (double)vv[u] : 0.0, x2 = 2.0 * xi;
    double tm2 = 1.0, tm1 = xi;
    if constexpr (LO == 0) {
      acc[0] += v;
      acc[1] = __builtin_fma(xi, v, acc[1]);
    }
#pragma unroll
    for (int m = 2; m < LO + CNT; ++m) {
      const double tm = __builtin_fma(x2, tm1, -tm2);     // T_m = 2x T_{m-1} - T_{m-2}
      if (m >= LO) acc[m - LO] = __builtin_fma(tm, v, acc[m - LO]);
      tm2 = tm1;
      tm1 = tm;
    }
  }
  constexpr int QB = CNT / 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CNT / 2; ++i) acc[i] = swap_add<32>(acc[i], acc[i + CNT / 2]);
#pragma unroll
  for (int i = 0; i < QB; ++i) {
    double s = swap_add<16>(acc[i], acc[i + QB]);
    s += dpp_d<0xb1>(s);    // quad_perm [1,0,3,2]
    s += dpp_d<0x4e>(s);    // quad_perm [2,3,0,1]
    s += dpp_d<0x141>(s);   // row_half_mirror
    s += dpp_d<0x140>(s);   // row_mirror
    if ((lane & 15) == i) red[w * CNT + QB * (lane >> 4) + i] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < CNT) {
    const int m = threadIdx.x;
    dst[LO + m] = (red[m] + red[CNT + m]) + (red[2 * CNT + m] + red[3 * CNT + m]);
  }
}

// grid (2 row blocks, jn, T): blockIdx.x = 2 b + slice
template <int PB>
__global__ __launch_bounds__(256) void lrx_project_kernel(const float *__restrict__ xt, const float *__restrict__ V,
                                                          double *__restrict__ part, int N, int T, int j0, int jn) {
  static_assert(PB > 64 && PB <= 128 && PB % 8 == 0, "the ranks above lr_project_kernel's");
  __shared__ double red[4 * 64];
  const int b = blockIdx.x >> 1, slice = blockIdx.x & 1, jj = blockIdx.y, t = blockIdx.z;
  const float *x = xt + (size_t)(j0 + jj) * N;
  const int r0 = b * kProjRows + (int)threadIdx.x;
  float xv[kProjRowsPerThread], vv[kProjRowsPerThread];
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {          // every load requested before the first use, as lr_project_kernel
    const int i = r0 + u * 256, ic = i < N ? i : N - 1;
    xv[u] = x[ic];
    vv[u] = V[(size_t)ic * T + t];
  }
  __builtin_amdgcn_sched_barrier(0);
  double *dst = part + (((size_t)b * jn + jj) * T + t) * PB;
  if (slice == 0)
    lrx_project_slice<0, 64, PB>(xv, vv, r0, N, red, dst);
  else
    lrx_project_slice<64, PB - 64, PB>(xv, vv, r0, N, red, dst);
}

// (c) of the product: lr_output_kernel's loads, LDS staging and group order with the Clenshaw recurrence in float64.  The
// rounding of a float32 recurrence grows with the degree (and with its square near |x| = 1), which ranks above 64 — half-widths
// above 7, where the float32 coordinate itself is already coarse — do not leave room for; U stays float32 in LDS (32 KB at PB
// 128) and is widened as it is read.  grid (row blocks of 64, T)
template <int PB>
__global__ __launch_bounds__(256) void lrx_output_kernel(const float *__restrict__ xt, const float *__restrict__ U,
                                                         const float *__restrict__ V, float *__restrict__ out, int N, int T,
                                                         int j0, int jn, int r0, int r1, float noise) {
  static_assert(PB > 64 && PB <= 128 && PB % 8 == 0, "the ranks above lr_output_kernel's");
  __shared__ __attribute__((aligned(16))) float su[kPrepMaxJ * PB];
  __shared__ double sacc[4][kOutRows];
  const int t = blockIdx.y;
  const int r = threadIdx.x & (kOutRows - 1), g = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int i = blockIdx.x * kOutRows + r;
  const bool mine = i >= r0 && i < r1;
  int ic = i > r0 ? i : r0;
  ic = ic < r1 ? ic : r1 - 1;
  ic = ic < N ? ic : N - 1;
  ic = ic > 0 ? ic : 0;
  constexpr int kMaxPer = kPrepMaxJ / 4;
  float xv[kMaxPer];
#pragma unroll
  for (int q = 0; q < kMaxPer; ++q) {
    const int jj = g + 4 * q;
    xv[q] = jj < jn ? xt[(size_t)(j0 + jj) * N + ic] : 0.f;
  }
  float vn = 0.f;
  if (g == 0 && noise != 0.f) vn = V[(size_t)(i < N ? i : N - 1) * T + t];
  constexpr int kTrips = (kPrepMaxJ * PB / 4 + 255) / 256;
  const int nu4 = jn * (PB / 4);                          // U[.][t][.] of the jn projections as float4
  float4v uv[kTrips];
#pragma unroll
  for (int k = 0; k < kTrips; ++k)
    if (g * kOutRows + 256 * k < nu4) {
      const int e = (int)threadIdx.x + 256 * k, ec = e < nu4 ? e : nu4 - 1;
      uv[k] = *reinterpret_cast<const float4v *>(U + ((size_t)(ec / (PB / 4)) * T + t) * PB + 4 * (ec % (PB / 4)));
    }
  __builtin_amdgcn_sched_barrier(0);                      // (every load above is in flight before the first wait)
#pragma unroll
  for (int k = 0; k < kTrips; ++k)
    if (g * kOutRows + 256 * k < nu4) {
      const int e = (int)threadIdx.x + 256 * k;
      if (e < nu4) *reinterpret_cast<float4v *>(su + 4 * e) = uv[k];
    }
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < kMaxPer; q += 2) {                  // two projections at a time: two independent float64 chains
    const int jj = g + 4 * q;
    if (jj >= jn) break;
    const bool two = jj + 4 < jn;                         // (wave-uniform; a missing second one re-reads the first's U)
    const float *u = su + jj * PB, *w = su + (two ? jj + 4 : jj) * PB;
    const double x = (double)xv[q], x2 = 2.0 * x, y = (double)xv[q + 1], y2 = 2.0 * y;
    double b1 = 0.0, b2 = 0.0, c1 = 0.0, c2 = 0.0;        // Clenshaw: b_k = U_k + 2x b_{k+1} - b_{k+2}
#pragma unroll 8
    for (int k = PB - 1; k >= 1; --k) {
      const double bk = __builtin_fma(x2, b1, (double)u[k] - b2), ck = __builtin_fma(y2, c1, (double)w[k] - c2);
      b2 = b1;
      b1 = bk;
      c2 = c1;
      c1 = ck;
    }
    acc += __builtin_fma(x, b1, (double)u[0] - b2);
    if (two) acc += __builtin_fma(y, c1, (double)w[0] - c2);
  }
  sacc[g][r] = acc;
  __syncthreads();
  if (g != 0 || i >= N) return;
  double res = mine ? (sacc[0][r] + sacc[1][r]) + (sacc[2][r] + sacc[3][r]) : 0.0;
  if (noise != 0.f) res = __builtin_fma((double)noise, (double)vn, res);
  out[(size_t)i * T + t] = (float)res;
}

template <int PB>
int launch_lowrank_wide(const LowrankPlan &P, const float *w, const float *V, float *out, int N, int T, int j0, int jn,
                        int r0, int r1, float scale, float noise, double *part, float *U, hipStream_t st) {
  const int nblk = proj_blocks(N);
  hipLaunchKernelGGL(lrx_project_kernel<PB>, dim3(2 * nblk, jn, T), dim3(256), 0, st, P.xt, V, part, N, T, j0, jn);
  if (w)
    hipLaunchKernelGGL(lrw_combine_kernel<PB>, dim3(jn, T), dim3(256), 0, st, part, P.coef, w + j0, U, nblk, T, jn, scale);
  else
    hipLaunchKernelGGL(lr_combine_kernel<PB>, dim3(jn, T), dim3(256), 0, st, part, P.coef, U, nblk, T, jn, scale);
  hipLaunchKernelGGL(lrx_output_kernel<PB>, dim3((N + kOutRows - 1) / kOutRows, T), dim3(256), 0, st, P.xt, U, V, out, N, T,
                     j0, jn, r0, r1, noise);
  return (int)hipGetLastError();
}

// (b) of the derivative for PB > 64: lrg_combine_kernel / lrgw_combine_kernel (wt: the weight of projection j0, or null) with
// the padded ranks as arguments — a latency chain of one workgroup per (projection, t), which 136 (PB, QB) pairs of each
// kernel would compile for nothing.  Same order of every addition as the templated kernels: G = 256 / pb groups over the row
// blocks, then the groups in ascending order.  D is exactly antisymmetric, so thread m reads d_km (consecutive in m) and
// subtracts where lrg_combine_kernel reads row m and adds: the same products, signs and order.
__global__ __launch_bounds__(256) void lrgx_combine_kernel(const double *__restrict__ partL, const double *__restrict__ partR,
                                                           const double *__restrict__ dcoef, const double *__restrict__ ccoef,
                                                           const float *__restrict__ wt, double *__restrict__ U,
                                                           double *__restrict__ gsp, int nblk, int T, int jn, int p, int pc,
                                                           int pb, int qb, double scale) {
  __shared__ double sw[2][256];
  __shared__ double w[2][128];
  __shared__ double cw[128];
  const int G = 256 / pb;
  const int jj = blockIdx.x, t = blockIdx.y;
  const int n = threadIdx.x % pb, g = threadIdx.x / pb;
  const double sj = wt ? scale * (double)wt[jj] : scale;
  if (g < G) {
    double sl = 0.0, sr = 0.0;
    for (int b = g; b < nblk; b += G) {
      const size_t o = (((size_t)b * jn + jj) * T + t) * pb + n;
      sl += partL[o];
      sr += partR[o];
    }
    sw[0][g * pb + n] = sl;
    sw[1][g * pb + n] = sr;
  }
  __syncthreads();
  const int m = threadIdx.x;
  if (m < pb) {
    double sl = sw[0][m], sr = sw[1][m];
    for (int k = 1; k < G; ++k) {
      sl += sw[0][k * pb + m];
      sr += sw[1][k * pb + m];
    }
    w[0][m] = sl;
    w[1][m] = sr;
  }
  __syncthreads();
  if (m < qb) {
    double ur = 0.0, ul = 0.0;
#pragma unroll 8
    for (int k = 0; k < qb; ++k) {
      const double d = -dcoef[k * qb + m];                // = d_mk
      ur = __builtin_fma(d, w[1][k], ur);
      ul = __builtin_fma(d, w[0][k], ul);
    }
    double *u = U + ((size_t)jj * T + t) * 2 * qb;
    u[m] = sj * ur;
    u[qb + m] = sj * ul;
  }
  if (m < pb) {                                           // (C W^R)[m], zero beyond p
    double s = 0.0;
    if (m < p)
      for (int k = 0; k < p; ++k) s = __builtin_fma(ccoef[m * pc + k], w[1][k], s);
    cw[m] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < p; ++k) s = __builtin_fma(w[0][k], cw[k], s);
    gsp[(size_t)jj * T + t] = s;
  }
}

// (c) of the derivative for QB > 64: lrg_output_kernel / lrgw_output_kernel (per_comp) with the Clenshaw sum split at 64.
// Clenshaw consumes q_k in descending k, so L and R are folded into the upper QB - 64 values first, the recurrence runs down to
// k = 64, the lower 64 values are folded into the same registers, and the recurrence continues with its (b1, b2): at most 64
// q per lane, lrg_output_kernel<64>'s footprint, for one more read of the lane's T values of L and R.  grid (row blocks of 64)
template <int QB>
__global__ __launch_bounds__(256) void lrgx_output_kernel(const float *__restrict__ xt, const double *__restrict__ U,
                                                          const double *__restrict__ gsp, const float *__restrict__ L,
                                                          const float *__restrict__ R, float *__restrict__ gZ,
                                                          float *__restrict__ gout, int N, int T, int j0, int jn, int ldg,
                                                          int per_comp) {
  static_assert(QB > 64 && QB <= 128 && QB % 8 == 0, "the ranks above lrg_output_kernel's");
  constexpr int HI = QB - 64;
  __shared__ float sres[kOutRows][kPrepMaxJ + 1];
  const int r = threadIdx.x & (kOutRows - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int row0 = blockIdx.x * kOutRows;
  const int i = row0 + r;
  const bool ok = i < N;
  for (int jj = wv; jj < jn; jj += 4) {
    const double *u = U + (size_t)jj * T * 2 * QB;
    const double x = ok ? (double)xt[(size_t)(j0 + jj) * N + i] : 0.0, x2 = 2.0 * x;
    double q[64];
#pragma unroll
    for (int m = 0; m < HI; ++m) q[m] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double l = ok ? (double)L[(size_t)i * T + t] : 0.0;
      const double rr = ok ? (double)R[(size_t)i * T + t] : 0.0;
      const double *ut = u + (size_t)t * 2 * QB + 64;
#pragma unroll
      for (int m = 0; m < HI; ++m) q[m] = __builtin_fma(l, ut[m], __builtin_fma(rr, ut[QB + m], q[m]));
    }
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = HI - 1; k >= 0; --k) {                   // ranks QB - 1 ... 64
      const double bk = __builtin_fma(x2, b1, q[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    asm volatile("" : "+v"(b1), "+v"(b2));                // (the upper sum ends here: its q are dead before the lower fold)
#pragma unroll
    for (int m = 0; m < 64; ++m) q[m] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double l = ok ? (double)L[(size_t)i * T + t] : 0.0;
      const double rr = ok ? (double)R[(size_t)i * T + t] : 0.0;
      const double *ut = u + (size_t)t * 2 * QB;
#pragma unroll
      for (int m = 0; m < 64; ++m) q[m] = __builtin_fma(l, ut[m], __builtin_fma(rr, ut[QB + m], q[m]));
    }
#pragma unroll
    for (int k = 63; k >= 1; --k) {
      const double bk = __builtin_fma(x2, b1, q[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    sres[r][jj] = (float)__builtin_fma(x, b1, q[0] - b2);
  }
  __syncthreads();
  const int rows = N - row0 < kOutRows ? N - row0 : kOutRows;
  for (int e = threadIdx.x; e < rows * jn; e += 256) {
    const int rr = e / jn, c = e - rr * jn;
    gZ[(size_t)(row0 + rr) * ldg + j0 + c] = sres[rr][c];
  }
  if (blockIdx.x != 0) return;
  if (per_comp) {                                         // gcomp[j0 + jj] = sum_t gsp[jj][t], as lrgw_output_kernel
    if ((int)threadIdx.x < jn) {
      double s = 0.0;
      for (int t = 0; t < T; ++t) s += gsp[(size_t)threadIdx.x * T + t];
      gout[j0 + threadIdx.x] = (float)s;
    }
  } else if (threadIdx.x == 0) {                          // gscale, as lrg_output_kernel
    double s = 0.0;
    for (int k = 0; k < jn * T; ++k) s += gsp[k];
    *gout = (float)s;
  }
}

// the derivative with PB = pad8(max(p, q)) > 64; w: the weights (gout = gcomp, ldg = J) or null (gout = gscale).  QB <= 64
// (p > 64 >= q) runs the output kernels above.
template <int PB>
void launch_grad_wide_project(const LowrankPlan &P, const float *L, const float *R, double *partL, double *partR, int N, int T,
                              int j0, int jn, hipStream_t st) {
  const int nblk = proj_blocks(N);
  hipLaunchKernelGGL(lrx_project_kernel<PB>, dim3(2 * nblk, jn, T), dim3(256), 0, st, P.xt, L, partL, N, T, j0, jn);
  hipLaunchKernelGGL(lrx_project_kernel<PB>, dim3(2 * nblk, jn, T), dim3(256), 0, st, P.xt, R, partR, N, T, j0, jn);
}

template <int QB>
void launch_grad_wide_output(const LowrankPlan &P, const float *w, const double *U, const double *gsp, const float *L,
                             const float *R, float *gZ, float *gout, int N, int T, int j0, int jn, int ldg, hipStream_t st) {
  const dim3 grid((N + kOutRows - 1) / kOutRows);
  if constexpr (QB > 64)
    hipLaunchKernelGGL(lrgx_output_kernel<QB>, grid, dim3(256), 0, st, P.xt, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg,
                       w ? 1 : 0);
  else if (w)
    hipLaunchKernelGGL(lrgw_output_kernel<QB>, grid, dim3(256), 0, st, P.xt, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg);
  else
    hipLaunchKernelGGL(lrg_output_kernel<QB>, grid, dim3(256), 0, st, P.xt, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg);
}

// ---- explicit features of the posterior (rpgp_lowrank_post_select / rpgp_lowrank_features_f64) --------------------------
// C (p x p, symmetric PSD up to rounding: a congruence of the kernel's Gram matrix at the Chebyshev points) = Q diag(l) Q^T by
// cyclic Jacobi rotations in double (a fixed sweep order: deterministic).  a: p x p row-major, overwritten; q: eigenvectors as
// columns (p x p row-major); l: eigenvalues.
void jacobi_eigh(std::vector<double> &a, int p, std::vector<double> &q, std::vector<double> &l) {
  q.assign((size_t)p * p, 0.0);
  for (int i = 0; i < p; ++i) q[(size_t)i * p + i] = 1.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < p; ++i) {
      diag += a[(size_t)i * p + i] * a[(size_t)i * p + i];
      for (int j = i + 1; j < p; ++j) off += a[(size_t)i * p + j] * a[(size_t)i * p + j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int i = 0; i < p - 1; ++i)
      for (int j = i + 1; j < p; ++j) {
        const double aij = a[(size_t)i * p + j];
        if (aij == 0.0) continue;
        const double aii = a[(size_t)i * p + i], ajj = a[(size_t)j * p + j];
        const double theta = (ajj - aii) / (2.0 * aij);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < p; ++k) {                     // A <- A R (columns i, j), then A <- R^T A (rows i, j)
          const double aki = a[(size_t)k * p + i], akj = a[(size_t)k * p + j];
          a[(size_t)k * p + i] = c * aki - s * akj;
          a[(size_t)k * p + j] = s * aki + c * akj;
        }
        for (int k = 0; k < p; ++k) {
          const double aik = a[(size_t)i * p + k], ajk = a[(size_t)j * p + k];
          a[(size_t)i * p + k] = c * aik - s * ajk;
          a[(size_t)j * p + k] = s * aik + c * ajk;
        }
        for (int k = 0; k < p; ++k) {
          const double qki = q[(size_t)k * p + i], qkj = q[(size_t)k * p + j];
          q[(size_t)k * p + i] = c * qki - s * qkj;
          q[(size_t)k * p + j] = s * qki + c * qkj;
        }
      }
  }
  l.resize(p);
  for (int i = 0; i < p; ++i) l[i] = a[(size_t)i * p + i];
}

// The same decomposition for p > 64, where Jacobi's O(p^3) sweeps with strided column updates take 37 ms (p = 113) to 142 ms
// (p = 128) on the host: Householder reduction to tridiagonal form, then the implicit QL iteration with the rotations
// accumulated into q (the textbook tred2 / tql2 pair).  Deterministic: no pivoting, a fixed order.  a: p x p row-major
// (read only); q: eigenvectors as columns; l: eigenvalues (ascending up to ties).  The caller's tail bound is taken from
// C - G G^T itself, so it covers this solver's rounding as it covers Jacobi's.
void tridiagonal_ql_eigh(const std::vector<double> &a, int p, std::vector<double> &q, std::vector<double> &l) {
  q = a;
  l.assign(p, 0.0);
  std::vector<double> e(p, 0.0);
  double *d = l.data();
  auto V = [&](int i, int j) -> double & { return q[(size_t)i * p + j]; };
  for (int j = 0; j < p; ++j) d[j] = V(p - 1, j);
  for (int i = p - 1; i > 0; --i) {                       // Householder reduction of row i
    double scale = 0.0, h = 0.0;
    for (int k = 0; k < i; ++k) scale += fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (int j = 0; j < i; ++j) {
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
        V(j, i) = 0.0;
      }
    } else {
      for (int k = 0; k < i; ++k) {
        d[k] /= scale;
        h += d[k] * d[k];
      }
      double f = d[i - 1], g = sqrt(h);
      if (f > 0.0) g = -g;
      e[i] = scale * g;
      h -= f * g;
      d[i - 1] = f - g;
      for (int j = 0; j < i; ++j) e[j] = 0.0;
      for (int j = 0; j < i; ++j) {                       // e = A u (the lower triangle only)
        f = d[j];
        V(j, i) = f;
        g = e[j] + V(j, j) * f;
        for (int k = j + 1; k < i; ++k) {
          g += V(k, j) * d[k];
          e[k] += V(k, j) * f;
        }
        e[j] = g;
      }
      f = 0.0;
      for (int j = 0; j < i; ++j) {
        e[j] /= h;
        f += e[j] * d[j];
      }
      const double hh = f / (h + h);
      for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (int j = 0; j < i; ++j) {                       // A <- A - u e^T - e u^T
        f = d[j];
        g = e[j];
        for (int k = j; k < i; ++k) V(k, j) -= f * e[k] + g * d[k];
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  for (int i = 0; i < p - 1; ++i) {                       // accumulate the reflections
    V(p - 1, i) = V(i, i);
    V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (int k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (int j = 0; j <= i; ++j) {
        double g = 0.0;
        for (int k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (int k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (int k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
  }
  for (int j = 0; j < p; ++j) {
    d[j] = V(p - 1, j);
    V(p - 1, j) = 0.0;
  }
  V(p - 1, p - 1) = 1.0;
  for (int i = 1; i < p; ++i) e[i - 1] = e[i];            // implicit QL on (d, e)
  e[p - 1] = 0.0;
  const double eps = 2.220446049250313e-16;
  double f = 0.0, tst1 = 0.0;
  for (int lo = 0; lo < p; ++lo) {
    tst1 = fmax(tst1, fabs(d[lo]) + fabs(e[lo]));
    int m = lo;
    while (m < p - 1 && fabs(e[m]) > eps * tst1) ++m;
    if (m > lo) {
      for (int iter = 0; iter < 200; ++iter) {            // (converges in a few; the bound only ends a pathological input)
        double g = d[lo];
        double pp = (d[lo + 1] - g) / (2.0 * e[lo]);
        double r = hypot(pp, 1.0);
        if (pp < 0.0) r = -r;
        d[lo] = e[lo] / (pp + r);
        d[lo + 1] = e[lo] * (pp + r);
        const double dl1 = d[lo + 1];
        double h = g - d[lo];
        for (int i = lo + 2; i < p; ++i) d[i] -= h;
        f += h;
        pp = d[m];
        double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
        const double el1 = e[lo + 1];
        for (int i = m - 1; i >= lo; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * pp;
          r = hypot(pp, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = pp / r;
          pp = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < p; ++k) {
            h = V(k, i + 1);
            V(k, i + 1) = s * V(k, i) + c * h;
            V(k, i) = c * V(k, i) - s * h;
          }
        }
        pp = -s * s2 * c3 * el1 * e[lo] / dl1;
        e[lo] = s * pp;
        d[lo] = c * pp;
        if (fabs(e[lo]) <= eps * tst1) break;
      }
    }
    d[lo] += f;
    e[lo] = 0.0;
  }
}

constexpr int kFeatRows = 64;            // rows per workgroup (4 waves x 16 rows, all projections)
constexpr int kFeatLd = 80;              // LDS row stride of G in doubles (PB <= 64): rows 4s + kq of one read land 32 banks apart

typedef double double4v __attribute__((ext_vector_type(4)));

// ---- padded ranks 72 ... 128 (r up to p: up to 8 column tiles) --------------------------------------------------------------
// G no longer fits the 64 KB of static LDS, so it is staged in dynamic LDS sized from the column tiles in use: PB rows of
// wide_ld(nct) doubles.  The stride stays = 16 mod 32 doubles: ds_read_b64 serves a 32-lane half per cycle, lanes 0-15 read 16
// consecutive doubles (banks 0-31) of row 4s + kq and lanes 16-31 those of the next row, 2 * stride = 32 mod 64 banks further
// on: no conflict.  LDS per workgroup: PB * wide_ld * 8 bytes, from 27 KB (PB 72, one tile) to 144 KB (PB 128, eight tiles) of
// the CU's 160 KB, so 5 ... 1 workgroups per CU (DESIGN.md §7.5 has the table).
// Registers (hipcc 7.2, -O3, gfx950; unified VGPRs, of which 8 are AGPRs), lr_features_kernel | lr_features_grad_kernel, no
// scratch and no spill in any of them:
//   PB  64:  76 | 108
//   PB  72:  80 | 112      PB  80:  84 | 116      PB  88:  88 | 120      PB  96:  92 | 124
//   PB 104:  96 | 128      PB 112: 100 | 132      PB 120: 104 | 136      PB 128: 108 | 140
// so registers allow 3 waves per SIMD at worst and above PB 64 LDS is what bounds the occupancy.
constexpr int kFeatMaxRank = 128;        // largest p (and r) of the feature kernels
constexpr int wide_ld(int nct) { return ((nct * 16 + 31) & ~31) + 16; }           // 48, 48, 80, 80, 112, 112, 144, 144
constexpr size_t wide_lds_bytes(int pb, int nct) { return (size_t)pb * wide_ld(nct) * sizeof(double); }

// G (p x r) -> LDS rows of `ld` doubles, zero-padded to PB x 16 nct
template <int PB>
__device__ __forceinline__ void stage_wide(double *gs, const double *__restrict__ G, int p, int r, int nct, int ld) {
  const int nc = nct * 16;
  for (int e = threadIdx.x; e < PB * nc; e += 256) {
    const int m = e / nc, k = e - m * nc;
    gs[m * ld + k] = (m < p && k < r) ? G[m * r + k] : 0.0;
  }
  __syncthreads();
}

// the lane's part of the (16 x PB) Chebyshev tile: a[s] = T_{4s + kq}(x)
template <int PB>
__device__ __forceinline__ void chebyshev_tile(double x, int kq, double (&a)[PB / 4]) {
  const double x2 = 2.0 * x;
  double tm2 = 1.0, tm1 = x;
  a[0] = kq == 0 ? 1.0 : (kq == 1 ? x : 0.0);
#pragma unroll
  for (int m = 2; m < PB; ++m) {                          // T_m = 2x T_{m-1} - T_{m-2}; lane keeps m = 4s + kq
    const double tm = __builtin_fma(x2, tm1, -tm2);
    if ((m & 3) == kq) a[m >> 2] = tm;
    tm2 = tm1;
    tm1 = tm;
  }
}

// what a lane of the feature body knows about its place: its wave's first row, the rows N, the features per projection r, and
// lane l's column l & 15 and quarter l >> 4 (the product tile's rows kq + 4 i, i < 4)
struct FeatLane {
  long long rbase, N;
  int r, c16, kq;
};

// The body of both feature kernels.  G (zero-padded to PB rows) is staged in LDS once per workgroup; a wave takes 16 rows and,
// for each projection, forms the (16 x PB) Chebyshev tile in registers (lane l: row l & 15, T_m for m = 4s + (l >> 4)) and
// multiplies it by G's column tiles of 16 on v_mfma_f64_16x16x4_f64 (A[row l&15][k l>>4], B[k l>>4][col l&15]; D col l&15,
// row (l>>4) + 4 reg).  Each product tile whose column is below r goes to the epilogue: init once, then per projection begin,
// tile per column tile, end.  PB <= 64: G in static LDS, PB x kFeatLd doubles, all 64 columns staged; above: stage_wide.
// which column of Z projection j reads: j itself, or the entry j of a list (the *_cols kernels)
struct ColsAll {
  __device__ __forceinline__ int operator()(int j) const { return j; }
};
struct ColsList {
  const int *__restrict__ cols;
  __device__ __forceinline__ int operator()(int j) const { return cols[j]; }
};

template <int PB, typename Epilogue, typename Cols = ColsAll>
__device__ __forceinline__ void lr_features_body(const double *__restrict__ Z, long long N, int J, int ldz,
                                                 const double *__restrict__ mid, double inv_w, const double *__restrict__ G,
                                                 int p, int r, Epilogue ep, Cols zcol = {}) {
  const int nct = (r + 15) >> 4;
  double *gs;
  int ld;
  if constexpr (PB <= 64) {
    __shared__ double gn[PB * kFeatLd];
    gs = gn;
    ld = kFeatLd;
    for (int e = threadIdx.x; e < PB * 64; e += 256) {
      const int m = e >> 6, k = e & 63;
      gs[m * kFeatLd + k] = (m < p && k < r) ? G[m * r + k] : 0.0;
    }
    __syncthreads();
  } else {
    extern __shared__ double gw[];
    gs = gw;
    ld = wide_ld(nct);
    stage_wide<PB>(gs, G, p, r, nct, ld);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const FeatLane L = {(long long)blockIdx.x * kFeatRows + wv * 16, N, r, lane & 15, lane >> 4};
  const long long row = L.rbase + L.c16;
  const bool ok = row < N;
  const double *gl = gs + L.kq * ld + L.c16;
  ep.init(L);
  for (int j = 0; j < J; ++j) {
    const double x = ok ? (Z[row * ldz + zcol(j)] - mid[j]) * inv_w : 0.0;
    double a[PB / 4];
    chebyshev_tile<PB>(x, L.kq, a);
    ep.begin(j);
    for (int ct = 0; ct < nct; ++ct) {
      double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < PB / 4; ++s)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], gl[4 * s * ld + ct * 16], acc, 0, 0, 0);
      const int col = ct * 16 + L.c16;
      if (col < r) ep.tile(L, j, col, acc);
    }
    ep.end(L, j);
  }
}

// B[i ldb + j r + k] = sqrt_scale * (product tile).  Every store: 4 rows x 16 consecutive doubles.
struct FeatStore {
  double sqrt_scale;
  double *__restrict__ B;
  long long ldb;
  __device__ __forceinline__ void init(const FeatLane &) {}
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void tile(const FeatLane &L, int j, int col, const double4v &acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long ro = L.rbase + L.kq + 4 * i;
      if (ro < L.N) B[ro * ldb + (long long)j * L.r + col] = sqrt_scale * acc[i];
    }
  }
  __device__ __forceinline__ void end(const FeatLane &, int) {}
};

// FeatStore with the factor of projection j read from col_scale[j]
struct FeatStoreCols {
  const double *__restrict__ col_scale;
  FeatStore s;
  __device__ __forceinline__ void init(const FeatLane &L) { s.init(L); }
  __device__ __forceinline__ void begin(int j) { s.sqrt_scale = col_scale[j]; }
  __device__ __forceinline__ void tile(const FeatLane &L, int j, int col, const double4v &acc) { s.tile(L, j, col, acc); }
  __device__ __forceinline__ void end(const FeatLane &, int) {}
};

// The adjoint: each product tile is multiplied element-wise by W = ca alpha v^T + cy Y read as 4 rows x 16 consecutive doubles
// of Y, summed over the column tiles in the lane, then over the 16 lanes of a row by xor-shuffles 8, 4, 2, 1 (a fixed order);
// lane l & 15 == 0 writes each (i, j) once.
struct FeatAdjoint {
  double fac;
  const double *__restrict__ Y;
  long long ldy;
  const double *__restrict__ alpha, *__restrict__ v;
  double ca, cy;
  double *__restrict__ gZ;
  long long ldg;
  double al[4], part[4];                                  // ca alpha of the lane's output rows kq + 4 i; their sums
  __device__ __forceinline__ void init(const FeatLane &L) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long ro = L.rbase + L.kq + 4 * i;
      al[i] = ro < L.N ? ca * alpha[ro] : 0.0;
    }
  }
  __device__ __forceinline__ void begin(int) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i] = 0.0;
  }
  __device__ __forceinline__ void tile(const FeatLane &L, int j, int col, const double4v &acc) {
    const long long f = (long long)j * L.r + col;
    const double vc = v[f];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long ro = L.rbase + L.kq + 4 * i;
      if (ro < L.N) part[i] = __builtin_fma(acc[i], __builtin_fma(cy, Y[ro * ldy + f], al[i] * vc), part[i]);
    }
  }
  __device__ __forceinline__ void end(const FeatLane &L, int j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      part[i] += __shfl_xor(part[i], 8);
      part[i] += __shfl_xor(part[i], 4);
      part[i] += __shfl_xor(part[i], 2);
      part[i] += __shfl_xor(part[i], 1);
    }
    if (L.c16 == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long ro = L.rbase + L.kq + 4 * i;
        if (ro < L.N) gZ[ro * ldg + j] = fac * part[i];
      }
    }
  }
};

// FeatAdjoint with the factor col_scale[j] * inv_w per projection, written to column cols[j] of gZ (W's columns stay j r + k)
struct FeatAdjointCols {
  const double *__restrict__ col_scale;
  const int *__restrict__ cols;
  double inv_w;
  FeatAdjoint a;
  __device__ __forceinline__ void init(const FeatLane &L) { a.init(L); }
  __device__ __forceinline__ void begin(int j) {
    a.fac = col_scale[j] * inv_w;
    a.begin(j);
  }
  __device__ __forceinline__ void tile(const FeatLane &L, int j, int col, const double4v &acc) { a.tile(L, j, col, acc); }
  __device__ __forceinline__ void end(const FeatLane &L, int j) { a.end(L, cols[j]); }
};

// B[i ldb + j r + k] = sqrt_scale * sum_{m < p} T_m(x_ij) G[m r + k],  x_ij = (Z[i ldz + j] - mid[j]) inv_w.
// grid (ceil(N / 64)); PB > 64: dynamic LDS wide_lds_bytes(PB, ceil(r / 16))
template <int PB>
__global__ __launch_bounds__(256) void lr_features_kernel(const double *__restrict__ Z, long long N, int J, int ldz,
                                                          const double *__restrict__ mid, double inv_w,
                                                          const double *__restrict__ G, int p, int r, double sqrt_scale,
                                                          double *__restrict__ B, long long ldb) {
  lr_features_body<PB>(Z, N, J, ldz, mid, inv_w, G, p, r, FeatStore{sqrt_scale, B, ldb});
}

// The adjoint of lr_features_kernel (rpgp_lowrank_features_grad_f64): with W = ca alpha v^T + cy Y (N x J r, never stored),
//   gZ[i ldg + j] = fac * sum_{k < r} (sum_{m < p} T_m(x_ij) Gd[m r + k]) W[i, j r + k],   fac = sqrt_scale inv_w,
// Gd the derivative coefficients of G (sum_m T'_m G[m, k] = sum_m T_m Gd[m, k]).  Same grid and LDS.
template <int PB>
__global__ __launch_bounds__(256) void lr_features_grad_kernel(const double *__restrict__ Z, long long N, int J, int ldz,
                                                               const double *__restrict__ mid, double inv_w,
                                                               const double *__restrict__ Gd, int p, int r, double fac,
                                                               const double *__restrict__ Y, long long ldy,
                                                               const double *__restrict__ alpha, const double *__restrict__ v,
                                                               double ca, double cy, double *__restrict__ gZ, long long ldg) {
  lr_features_body<PB>(Z, N, J, ldz, mid, inv_w, Gd, p, r, FeatAdjoint{fac, Y, ldy, alpha, v, ca, cy, gZ, ldg});
}

// The two kernels on a list of columns under one form, with a factor per column (rpgp_lowrank_features_cols_f64 /
// rpgp_lowrank_features_grad_cols_f64): the same body; projection c reads column cols[c] of Z, B / Y / v are the form's dense
// nc r block, gZ is written at column cols[c].  Same grid and LDS as the kernels above.
template <int PB>
__global__ __launch_bounds__(256) void lr_features_cols_kernel(const double *__restrict__ Z, long long N, int nc, int ldz,
                                                               const int *__restrict__ cols, const double *__restrict__ mid,
                                                               double inv_w, const double *__restrict__ G, int p, int r,
                                                               const double *__restrict__ col_scale, double *__restrict__ B,
                                                               long long ldb) {
  lr_features_body<PB>(Z, N, nc, ldz, mid, inv_w, G, p, r, FeatStoreCols{col_scale, FeatStore{0.0, B, ldb}}, ColsList{cols});
}

template <int PB>
__global__ __launch_bounds__(256) void lr_features_grad_cols_kernel(
    const double *__restrict__ Z, long long N, int nc, int ldz, const int *__restrict__ cols, const double *__restrict__ mid,
    double inv_w, const double *__restrict__ Gd, int p, int r, const double *__restrict__ col_scale,
    const double *__restrict__ Y, long long ldy, const double *__restrict__ alpha, const double *__restrict__ v, double ca,
    double cy, double *__restrict__ gZ, long long ldg) {
  lr_features_body<PB>(Z, N, nc, ldz, mid, inv_w, Gd, p, r,
                       FeatAdjointCols{col_scale, cols, inv_w, FeatAdjoint{0.0, Y, ldy, alpha, v, ca, cy, gZ, ldg}},
                       ColsList{cols});
}

// launch of either feature kernel: no dynamic LDS up to PB 64; above 64 KB it needs the function attribute (set per call: it
// belongs to the current device's copy of the kernel)
template <typename K, typename... A>
int launch_features(K kernel, int pb, int r, dim3 grid, hipStream_t st, A... args) {
  const size_t bytes = pb > 64 ? wide_lds_bytes(pb, (r + 15) >> 4) : 0;
  if (bytes > 65536) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)wide_lds_bytes(pb, kFeatMaxRank / 16));
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), bytes, st, args...);
  return (int)hipGetLastError();
}

// f(std::integral_constant<int, PB>) for the padded rank pb, a multiple of 8 in [8, MAX]; RPGP_EINVAL for any other pb
template <int MAX, int PB = 8, typename F>
int dispatch_pb(int pb, F &&f) {
  if constexpr (PB > MAX)
    return RPGP_EINVAL;
  else
    return pb == PB ? f(std::integral_constant<int, PB>{}) : dispatch_pb<MAX, PB + 8>(pb, f);
}

// dst[m ld + n] = c_mn for m, n < p, c the kRefDegree-strided coefficients of cheb2d_coefficients
template <typename T>
void copy_leading_block(const std::vector<double> &c, int p, T *dst, size_t ld) {
  for (int m = 0; m < p; ++m)
    for (int n = 0; n < p; ++n) dst[m * ld + n] = (T)c[(size_t)m * kRefDegree + n];
}

// rpgp_lowrank_select / rpgp_lowrank_grad_select (deriv): rank, tail and the leading block (leading dimension p_max)
int select_to_host(double h, int p_max, double tol, bool deriv, int *p_host, double *tail_host, double *coef_host) {
  if (!p_host || p_max < 1 || p_max > kRefDegree || !(tol > 0.0)) return RPGP_EINVAL;
  std::vector<double> c;
  double tail = 0.0;
  const int p = select_rank(h, p_max, tol < kTailTol ? tol : kTailTol, &tail, c, deriv);
  *p_host = p;
  if (tail_host) *tail_host = p ? tail : 0.0;
  if (coef_host) copy_leading_block(c, p, coef_host, p_max);
  return 0;
}


// the plan of rpgp_lowrank_create and of rpgp_lowrank_create_cap (rpgp_lowrank_create_tol: that entry at the cap 64)
int create_plan(const void *prep, int64_t N, int J, float max_abs, double tol, void *plan, size_t plan_bytes, int *p_host,
                void **handle_host, void *stream, int cap = kMaxRank) {
  if (!prep || !plan || !p_host || !handle_host || N <= 0 || N > 0x7fffffffLL || J <= 0 || J > kPrepMaxJ)
    return RPGP_EINVAL;
  if (plan_bytes < rpgp_lowrank_plan_bytes_cap(N, J, cap)) return RPGP_EWORKSPACE;
  *p_host = 0;
  *handle_host = nullptr;
  // a slightly wider interval than max|a| absorbs the rounding of a = (z - mid) * c at the ends of the range
  const double h = (double)max_abs * (1.0 + 1.0 / (1 << 20));
  std::vector<double> c;
  double tail = 0.0;
  const int p = select_rank(h, cap, tol, &tail, c);
  if (p == 0) return 0;                                   // not served: the sweep runs
  const int pb = pad8(p);
  std::vector<float> cf((size_t)pb * pb, 0.f);
  copy_leading_block(c, p, cf.data(), pb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float *coef = reinterpret_cast<float *>(plan);
  const int ld = cap_ld(cap);
  float *xt = coef + (size_t)ld * ld;
  hipError_t e = hipMemcpyAsync(coef, cf.data(), cf.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  // (rank 1: T_0 = 1 whatever x is; h = 0 would divide by zero)
  const float inv_h = (p == 1 || !(h > 0.0)) ? 0.f : (float)(1.0 / h);
  const long long total = N * J;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  const float2v *rowdat = reinterpret_cast<const float2v *>(reinterpret_cast<const float *>(prep) + kPrepRowdatOffsetFloats);
  hipLaunchKernelGGL(lr_coords_kernel, dim3(blocks), dim3(256), 0, st, rowdat, xt, (long long)N, J, inv_h);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  e = hipStreamSynchronize(st);                           // (the host copy of the coefficients goes out of scope)
  if (e != hipSuccess) return (int)e;
  LowrankPlan *P = new (std::nothrow) LowrankPlan{p, pb, N, J, h, tail, coef, xt};
  if (!P) return RPGP_EINVAL;
  P->tol = tol;
  P->cap = cap;
  P->ld = ld;
  *p_host = p;
  *handle_host = P;
  return 0;
}

// the derivative of a plan with pad8(max(p, q)) > 64: the projections by padded rank, the combine with the ranks as arguments,
// the output by QB.  w: the weights (gout = gcomp) or null (gout = gscale).  Same workspace layout as launch_grad.
int launch_grad_wide(const LowrankPlan &P, const float *w, const float *L, const float *R, float *gZ, float *gout, int N,
                     int ldg, int T, int j0, int jn, float scale, void *ws, hipStream_t st) {
  const int nblk = proj_blocks(N), pb = grad_pb(P), qb = P.qb;
  const size_t np = (size_t)nblk * jn * T * pb;
  double *partL = reinterpret_cast<double *>(ws), *partR = partL + np;
  double *U = partR + np, *gsp = U + (size_t)jn * T * 2 * qb;
  int rc = dispatch_pb<kCapRank, kMaxRank + 8>(pb, [&](auto b) {
    launch_grad_wide_project<decltype(b)::value>(P, L, R, partL, partR, N, T, j0, jn, st);
    return (int)hipGetLastError();
  });
  if (rc) return rc;
  hipLaunchKernelGGL(lrgx_combine_kernel, dim3(jn, T), dim3(256), 0, st, partL, partR, P.dcoef, P.ccoef, w ? w + j0 : nullptr, U,
                     gsp, nblk, T, jn, P.p, P.pb, pb, qb, (double)scale);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  return dispatch_pb<kCapRank>(qb, [&](auto b) {
    launch_grad_wide_output<decltype(b)::value>(P, w, U, gsp, L, R, gZ, gout, N, T, j0, jn, ldg, st);
    return (int)hipGetLastError();
  });
}

// ---- panels: any half-width at the per-row work of a rank <= 64 plan (rpgp_lowrank_create_panels) -----------------------------
// [-h, h] is cut into P equal panels of half-width hp = h / P; panel k has the centre c_k = -h + (2k + 1) hp and the local
// coordinate x = (a - c_k) / hp.  Two points of one panel interact through C0 (the single-interval form at hp), a point of panel
// k with one of panel k + 1 through C1, the coefficients of exp2(-hp^2 (x - y - 2)^2) (the opposite order: C1^T), and points two
// or more panels apart, at least 2 hp apart, are dropped: exp2(-4 hp^2).  D0, D1 and -D1^T are the same for the derivative.
// Every kernel below is new; none of the kernels above serves a panel plan.  DESIGN.md 7.9.
constexpr int kMaxPanels = 16;           // hp <= 6.4 at p, q <= 64: half-widths up to about 100
constexpr int kPanelLdsBytes = 32768;    // U of one column chunk in the output pass

// the coefficients of cheb2d_coefficients for the shifted argument: F(hp (x - y - shift)), F(d) = exp2(-d^2), or
// -(d / kappa) exp2(-d^2) for the derivative.  No symmetry is imposed (shift 2 has none).
void cheb2d_shifted(double hp, double shift, bool deriv, std::vector<double> &c) {
  const int M = kRefDegree;
  std::vector<double> xs(M), cs((size_t)M * M), f((size_t)M * M), g((size_t)M * M);
  for (int k = 0; k < M; ++k) xs[k] = cos(M_PI * (k + 0.5) / M);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < M; ++k) cs[(size_t)m * M + k] = cos(M_PI * m * (k + 0.5) / M);
  for (int k = 0; k < M; ++k)
    for (int l = 0; l < M; ++l) {
      const double d = hp * (xs[k] - xs[l] - shift), e = exp2(-d * d);
      f[(size_t)k * M + l] = deriv ? -(d / kKappa) * e : e;
    }
  for (int k = 0; k < M; ++k)
    for (int n = 0; n < M; ++n) {
      double s = 0.0;
      for (int l = 0; l < M; ++l) s += f[(size_t)k * M + l] * cs[(size_t)n * M + l];
      g[(size_t)k * M + n] = s;
    }
  c.assign((size_t)M * M, 0.0);
  for (int m = 0; m < M; ++m) {
    for (int k = 0; k < M; ++k) {
      const double w = cs[(size_t)m * M + k];
      for (int n = 0; n < M; ++n) c[(size_t)m * M + n] += w * g[(size_t)k * M + n];
    }
    const double wm = (m == 0 ? 1.0 : 2.0) / M;
    for (int n = 0; n < M; ++n) c[(size_t)m * M + n] *= wm * (n == 0 ? 1.0 : 2.0) / M;
  }
}

// select_rank's rule on given coefficients: the smallest p <= p_max whose tail (shells p ... plus the rounding allowance) is
// <= tol, 0 when there is none or the last 8 shells are not at rounding level; tail_of: that bound for a given p
struct Shells {
  double s[kRefDegree], allowance;
  bool resolved;
  explicit Shells(const std::vector<double> &c) {
    const int M = kRefDegree;
    for (int q = 0; q < M; ++q) s[q] = 0.0;
    for (int m = 0; m < M; ++m)
      for (int n = 0; n < M; ++n) s[m > n ? m : n] += fabs(c[(size_t)m * M + n]);
    double unresolved = 0.0;
    for (int q = M - 8; q < M; ++q) unresolved += s[q];
    resolved = unresolved <= 1e-11;
    allowance = 1e-13 + unresolved;
  }
  double tail_of(int p) const {
    double t = 0.0;
    for (int q = kRefDegree - 1; q >= p; --q) t += s[q];
    return t + allowance;
  }
  int rank(int p_max, double tol) const {
    if (!resolved) return 0;
    for (int p = 1; p <= p_max; ++p)
      if (tail_of(p) <= tol) return p;
    return 0;
  }
};

struct PanelForms {
  int P = 0, p = 0, q = 0;
  double hp = 0.0, b[3] = {0, 0, 0}, d[3] = {0, 0, 0};
  std::vector<double> c0, c1, d0, d1;    // kRefDegree-strided coefficients
};

// the forms of P panels at the tolerance, or false: a rank above 64, an unresolved form or a dropped value above the tolerance
bool panel_forms(double h, double tol, int P, PanelForms &F) {
  if (!(h > 0.0) || !isfinite(h) || P < 2 || P > kMaxPanels) return false;
  const double hp = h / P;
  // two or more panels apart: d >= 2 hp, where exp2(-d^2) and, from d = kappa on, (d / kappa) exp2(-d^2) fall (P = 2 drops nothing)
  const double drop = P > 2 ? exp2(-4.0 * hp * hp) : 0.0;
  const double ddrop = P > 2 ? (2.0 * hp < kKappa ? 1.0 : (2.0 * hp / kKappa) * exp2(-4.0 * hp * hp)) : 0.0;
  if (drop > tol || ddrop > tol) return false;
  cheb2d_coefficients(hp, F.d0, true);                    // (the largest rank of the four first: a count too small ends here)
  const Shells t0(F.d0);
  const int q0 = t0.rank(kMaxRank, tol);
  if (!q0) return false;
  cheb2d_coefficients(hp, F.c0);
  cheb2d_shifted(hp, 2.0, false, F.c1);
  cheb2d_shifted(hp, 2.0, true, F.d1);
  const Shells s0(F.c0), s1(F.c1), t1(F.d1);
  const int p0 = s0.rank(kMaxRank, tol), p1 = s1.rank(kMaxRank, tol), q1 = t1.rank(kMaxRank, tol);
  if (!p0 || !p1 || !q1) return false;
  F.P = P;
  F.hp = hp;
  F.p = p0 > p1 ? p0 : p1;
  F.q = q0 > q1 ? q0 : q1;
  F.b[0] = s0.tail_of(F.p), F.b[1] = s1.tail_of(F.p), F.b[2] = drop;
  F.d[0] = t0.tail_of(F.q), F.d[1] = t1.tail_of(F.q), F.d[2] = ddrop;
  return true;
}

// the smallest served panel count (panels 0), or that count alone
bool panel_select(double h, double tol, int panels, PanelForms &F) {
  if (panels) return panel_forms(h, tol, panels, F);
  if (!(h > 0.0) || !isfinite(h)) return false;
  int P = (int)ceil(h / 9.0);            // (hp >= 9 has no derivative rank <= 64 at any tolerance <= 2^-26: 61 at 7.86)
  for (P = P < 2 ? 2 : P; P <= kMaxPanels; ++P)
    if (panel_forms(h, tol, P, F)) return true;
  return false;
}

inline int panel_nbmax(int64_t N, int P) { return (int)(N / kProjRows) + P; }

// offsets (bytes) of the parts of a panel plan's buffer, each a multiple of 16
struct PanelLayout {
  size_t coef0, coef1, xl, xs, perm, bstart, pidx, total;
  PanelLayout(int64_t N, int J, int P) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t S = (size_t)panel_nbmax(N, P) * kProjRows;
    coef0 = 0;
    coef1 = coef0 + (size_t)kMaxRank * kMaxRank * sizeof(float);
    xl = coef1 + (size_t)kMaxRank * kMaxRank * sizeof(float);
    xs = up(xl + (size_t)N * J * sizeof(float));
    perm = up(xs + S * J * sizeof(float));
    bstart = up(perm + S * J * sizeof(int));
    pidx = up(bstart + (size_t)J * (P + 1) * sizeof(int));
    total = up(pidx + (size_t)N * J);
  }
};

// THE assignment of a prepared coordinate to (panel, local coordinate), for both orders: the panel is floor((a + h) / (2 hp))
// clamped to [0, P - 1] (a = +h: the last panel; an inner edge: the upper panel; a NaN: panel 0), evaluated in float64 from the
// float32 a, so it is a function of Z alone.  (A division, not a product with 1 / (2 hp): correctly rounded, it returns the
// integer for a coordinate exactly on an edge.)
__device__ __forceinline__ void panel_of(float a, double h, double hp, double inv_hp, int P, int &k, float &x) {
  const double kk = fmin(fmax(floor(((double)a + h) / (2.0 * hp)), 0.0), (double)(P - 1));
  k = (int)kk;
  x = (float)(((double)a - (-h + (2.0 * kk + 1.0) * hp)) * inv_hp);
}

// plan: xl[j][n], pidx[j][n] in natural order
__global__ __launch_bounds__(256) void lrp_coords_kernel(const float2v *__restrict__ rowdat, float *__restrict__ xl,
                                                         uint8_t *__restrict__ pidx, long long N, int J, double h, double hp,
                                                         double inv_hp, int P) {
  const long long total = N * J;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const int j = (int)(g / N);
    const long long n = g - (long long)j * N;
    int k;
    float x;
    panel_of(rowdat[n * J + j].x, h, hp, inv_hp, P, k, x);
    xl[g] = x;
    pidx[g] = (uint8_t)k;
  }
}

// plan: the stable counting sort of one column by panel, one workgroup per column, no atomics.  Thread t owns the rows
// [t chunk, (t + 1) chunk): it counts them by panel, the counts are prefix-summed over the threads (per panel) and over the panels
// (whole projection blocks each), and the thread then places its rows in ascending order.  Every position is a prefix sum, so the
// result is a function of Z alone.  Slots between a panel's last row and its last block's end keep perm = -1, x = 0.
__global__ __launch_bounds__(256) void lrp_sort_kernel(const uint8_t *__restrict__ pidx, const float *__restrict__ xl,
                                                       int *__restrict__ perm, float *__restrict__ xs, int *__restrict__ bstart,
                                                       int N, int P, int nbmax) {
  __shared__ int cnt[kMaxPanels][257];
  __shared__ int base[kMaxPanels];
  const int j = blockIdx.x, t = threadIdx.x;
  const size_t S = (size_t)nbmax * kProjRows;
  const uint8_t *pk = pidx + (size_t)j * N;
  const int chunk = (N + 255) / 256;
  const int i0 = t * chunk < N ? t * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
  for (int k = 0; k < P; ++k) cnt[k][t] = 0;
  for (int i = i0; i < i1; ++i) {
    const int k = pk[i] < P ? pk[i] : P - 1;
    cnt[k][t] += 1;
  }
  for (size_t s = t; s < S; s += 256) {
    perm[j * S + s] = -1;
    xs[j * S + s] = 0.f;
  }
  __syncthreads();
  if (t < P) {
    int run = 0;
    for (int u = 0; u < 256; ++u) {
      const int v = cnt[t][u];
      cnt[t][u] = run;
      run += v;
    }
    cnt[t][256] = run;
  }
  __syncthreads();
  if (t == 0) {
    int b = 0;
    for (int k = 0; k < P; ++k) {
      bstart[j * (P + 1) + k] = b;
      base[k] = b * kProjRows;
      b += (cnt[k][256] + kProjRows - 1) / kProjRows;
    }
    bstart[j * (P + 1) + P] = b;
  }
  __syncthreads();
  for (int i = i0; i < i1; ++i) {
    const int k = pk[i] < P ? pk[i] : P - 1;
    const int pos = base[k] + cnt[k][t];
    cnt[k][t] += 1;
    perm[j * S + pos] = i;
    xs[j * S + pos] = xl[(size_t)j * N + i];
  }
}

// (a) lr_project_kernel's body over the sorted slots of a column: block b covers the slots [2048 b, 2048 (b + 1)), all of one
// panel; V is read through the permutation (a padded slot: row 0, counted with v = 0).  A block past the column's count leaves.
// The derivative's projections of L and R are this kernel too.  grid (nbmax, jn, T)
template <int PB>
__global__ __launch_bounds__(256) void lrp_project_kernel(const float *__restrict__ xs, const int *__restrict__ perm,
                                                          const int *__restrict__ bstart, const float *__restrict__ V,
                                                          double *__restrict__ part, int T, int j0, int jn, int P, int nbmax) {
  __shared__ double red[4 * PB];
  const int b = blockIdx.x, jj = blockIdx.y, t = blockIdx.z;
  if (b >= bstart[(j0 + jj) * (P + 1) + P]) return;
  const size_t s0 = ((size_t)(j0 + jj) * nbmax + b) * kProjRows + threadIdx.x;
  float xv[kProjRowsPerThread], vv[kProjRowsPerThread];
  int pr[kProjRowsPerThread];
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    xv[u] = xs[s0 + u * 256];
    pr[u] = perm[s0 + u * 256];
  }
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) vv[u] = V[(size_t)(pr[u] < 0 ? 0 : pr[u]) * T + t];
  __builtin_amdgcn_sched_barrier(0);
  double acc[PB];
#pragma unroll
  for (int m = 0; m < PB; ++m) acc[m] = 0.0;
#pragma unroll
  for (int u = 0; u < kProjRowsPerThread; ++u) {
    const double xi = (double)xv[u], v = pr[u] < 0 ? 0.0 : (double)vv[u], x2 = 2.0 * xi;
    double tm2 = 1.0, tm1 = xi;
    acc[0] += v;
    acc[1] = __builtin_fma(xi, v, acc[1]);
#pragma unroll
    for (int m = 2; m < PB; ++m) {
      const double tm = __builtin_fma(x2, tm1, -tm2);     // T_m = 2x T_{m-1} - T_{m-2}
      acc[m] = __builtin_fma(tm, v, acc[m]);
      tm2 = tm1;
      tm1 = tm;
    }
  }
  constexpr int QB = PB / 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < PB / 2; ++i) acc[i] = swap_add<32>(acc[i], acc[i + PB / 2]);
#pragma unroll
  for (int i = 0; i < QB; ++i) {
    double s = swap_add<16>(acc[i], acc[i + QB]);
    s += dpp_d<0xb1>(s);    // quad_perm [1,0,3,2]
    s += dpp_d<0x4e>(s);    // quad_perm [2,3,0,1]
    s += dpp_d<0x141>(s);   // row_half_mirror
    s += dpp_d<0x140>(s);   // row_mirror
    if ((lane & 15) == i) red[w * PB + QB * (lane >> 4) + i] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < PB) {
    const int m = threadIdx.x;
    part[(((size_t)b * jn + jj) * T + t) * PB + m] = (red[m] + red[PB + m]) + (red[2 * PB + m] + red[3 * PB + m]);
  }
}

// W of the panels k - 1, k, k + 1 of (projection jj, t) into ws[3][pb]: thread (which, n) adds that panel's blocks in ascending
// order; a panel outside [0, P) is zero
__device__ __forceinline__ void panel_sums(const double *__restrict__ part, const int *__restrict__ bs, double *ws, int k, int P,
                                           int jn, int jj, int T, int t, int pb) {
  for (int e = threadIdx.x; e < 3 * pb; e += 256) {
    const int which = e / pb, n = e - which * pb, kk = k - 1 + which;
    double s = 0.0;
    if (kk >= 0 && kk < P)
      for (int b = bs[kk]; b < bs[kk + 1]; ++b) s += part[(((size_t)b * jn + jj) * T + t) * pb + n];
    ws[e] = s;
  }
}

// (b) U[jj][t][k][m] = (scale w_j) (C0 W_k + C1 W_{k+1} + C1^T W_{k-1})[m] in float64, the three products in that order, each
// over n ascending.  `w`: the weight of projection j0, or null; null and a weight of 1 give the same bits (scale * 1.0 is scale).
// grid (jn P, T)
template <int PB>
__global__ __launch_bounds__(256) void lrp_combine_kernel(const double *__restrict__ part, const float *__restrict__ coef0,
                                                          const float *__restrict__ coef1, const float *__restrict__ w,
                                                          const int *__restrict__ bstart, float *__restrict__ U, int T, int j0,
                                                          int jn, int P, float scale) {
  __shared__ double ws[3 * PB];
  const int jj = blockIdx.x / P, k = blockIdx.x - jj * P, t = blockIdx.y;
  panel_sums(part, bstart + (j0 + jj) * (P + 1), ws, k, P, jn, jj, T, t, PB);
  __syncthreads();
  const int m = threadIdx.x;
  if (m >= PB) return;
  const double sj = w ? (double)scale * (double)w[jj] : (double)scale;
  double a = 0.0;
  for (int n = 0; n < PB; ++n) a = __builtin_fma((double)coef0[m * PB + n], ws[PB + n], a);
  for (int n = 0; n < PB; ++n) a = __builtin_fma((double)coef1[m * PB + n], ws[2 * PB + n], a);
  for (int n = 0; n < PB; ++n) a = __builtin_fma((double)coef1[n * PB + m], ws[n], a);
  U[(((size_t)jj * T + t) * P + k) * PB + m] = (float)(sj * a);
}

// (c) lr_output_kernel in natural row order, each lane on its own panel's U.  LDS holds U[.][t] of a chunk of jc projections,
// P rows of PB + 1 floats each: lanes of a wave read the same m of different panels' rows, and the odd stride puts those rows
// PB + 1 banks apart (lanes of one panel read one address, a broadcast) where a stride of PB, a multiple of 8, would send every
// panel to the same few banks.  jc = 32 KB / (P (PB + 1) 4 B): 31 projections at P = 4, PB = 64, 7 at P = 16; 32 KB per
// workgroup leaves five workgroups (20 waves) per CU.  Wave g takes the projections jj = g (mod 4) of every chunk in ascending
// order, so the order of the additions does not depend on the chunking.  grid (row blocks of 64, T), dynamic LDS
template <int PB>
__global__ __launch_bounds__(256) void lrp_output_kernel(const float *__restrict__ xl, const uint8_t *__restrict__ pidx,
                                                         const float *__restrict__ U, const float *__restrict__ V,
                                                         float *__restrict__ out, int N, int T, int j0, int jn, int r0, int r1,
                                                         float noise, int P, int jc) {
  extern __shared__ float su[];
  __shared__ float sacc[4][kOutRows];
  constexpr int LD = PB + 1;
  const int t = blockIdx.y;
  const int r = threadIdx.x & (kOutRows - 1), g = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int i = blockIdx.x * kOutRows + r;
  const bool mine = i >= r0 && i < r1;
  int ic = i > r0 ? i : r0;
  ic = ic < r1 ? ic : r1 - 1;
  ic = ic < N ? ic : N - 1;
  ic = ic > 0 ? ic : 0;
  float vn = 0.f;
  if (g == 0 && noise != 0.f) vn = V[(size_t)(i < N ? i : N - 1) * T + t];
  float acc = 0.f;
  for (int c0 = 0; c0 < jn; c0 += jc) {
    const int cn = jn - c0 < jc ? jn - c0 : jc;
    if (c0) __syncthreads();                              // (the previous chunk's readers are done)
    for (int e = threadIdx.x; e < cn * P * PB; e += 256) {
      const int c = e / (P * PB), rem = e - c * (P * PB), row = rem / PB, m = rem - row * PB;
      su[(c * P + row) * LD + m] = U[((size_t)(c0 + c) * T + t) * P * PB + rem];
    }
    __syncthreads();
    for (int jj = c0 + ((g - c0) & 3); jj < c0 + cn; jj += 4) {
      const size_t o = (size_t)(j0 + jj) * N + ic;
      const float x = xl[o], x2 = 2.f * x;
      int pk = pidx[o];
      pk = pk < P ? pk : P - 1;
      const float *u = su + ((jj - c0) * P + pk) * LD;
      float b1 = 0.f, b2 = 0.f;                           // Clenshaw: b_k = U_k + 2x b_{k+1} - b_{k+2}
#pragma unroll
      for (int k = PB - 1; k >= 1; --k) {
        const float bk = __builtin_fmaf(x2, b1, u[k] - b2);
        b2 = b1;
        b1 = bk;
      }
      acc += __builtin_fmaf(x, b1, u[0] - b2);
    }
  }
  sacc[g][r] = acc;
  __syncthreads();
  if (g != 0 || i >= N) return;
  float res = mine ? (sacc[0][r] + sacc[1][r]) + (sacc[2][r] + sacc[3][r]) : 0.f;
  if (noise != 0.f) res = __builtin_fmaf(noise, vn, res);
  out[(size_t)i * T + t] = res;
}

inline int panel_chunk(const LowrankPlan &P, int jn) {
  const int jc = kPanelLdsBytes / (P.panels * (P.pb + 1) * (int)sizeof(float));
  return jc < 1 ? 1 : (jc < jn ? jc : jn);
}

// workspace of the product of a panel plan: part (nbmax x jn x T x PB doubles), U (jn x T x P x PB floats)
inline size_t panel_ws_bytes(const LowrankPlan &P, int jn, int T) {
  return (size_t)jn * T * P.pb * ((size_t)P.nbmax * sizeof(double) + (size_t)P.panels * sizeof(float));
}

// w: the weights (all of them; the launches offset by j0) or null
int launch_panels(const LowrankPlan &P, const float *w, const float *V, float *out, int N, int T, int j0, int jn, int r0,
                  int r1, float scale, float noise, void *ws, hipStream_t st) {
  double *part = reinterpret_cast<double *>(ws);
  float *U = reinterpret_cast<float *>(part + (size_t)P.nbmax * jn * T * P.pb);
  const int jc = panel_chunk(P, jn);
  const size_t lds = (size_t)jc * P.panels * (P.pb + 1) * sizeof(float);
  return dispatch_pb<kMaxRank>(P.pb, [&](auto pbc) {
    constexpr int PB = decltype(pbc)::value;
    hipLaunchKernelGGL(lrp_project_kernel<PB>, dim3(P.nbmax, jn, T), dim3(256), 0, st, P.xs, P.perm, P.bstart, V, part, T, j0,
                       jn, P.panels, P.nbmax);
    hipLaunchKernelGGL(lrp_combine_kernel<PB>, dim3(jn * P.panels, T), dim3(256), 0, st, part, P.coef, P.coef1,
                       w ? w + j0 : nullptr, P.bstart, U, T, j0, jn, P.panels, scale);
    hipLaunchKernelGGL(lrp_output_kernel<PB>, dim3((N + kOutRows - 1) / kOutRows, T), dim3(256), lds, st, P.xt, P.pidx, U, V,
                       out, N, T, j0, jn, r0, r1, noise, P.panels, jc);
    return (int)hipGetLastError();
  });
}

// (b) of the derivative, per (projection, panel, t), in float64, with the padded ranks as arguments (a latency chain of one
// workgroup, as lrgx_combine_kernel):
//   U[jj][k][t][0][m] = (scale w_j) (D0 W^R_k + D1 W^R_{k+1} - D1^T W^R_{k-1})[m],  [1][m]: the same of W^L
//   gsp[jj][k][t]     = W^L_k^T (C0 W^R_k + C1 W^R_{k+1} + C1^T W^R_{k-1})   (unweighted; leading dimension pc)
// grid (jn P, T)
__global__ __launch_bounds__(256) void lrpg_combine_kernel(const double *__restrict__ partL, const double *__restrict__ partR,
                                                           const double *__restrict__ d0, const double *__restrict__ d1,
                                                           const double *__restrict__ c0, const double *__restrict__ c1,
                                                           const float *__restrict__ wt, const int *__restrict__ bstart,
                                                           double *__restrict__ U, double *__restrict__ gsp, int T, int j0,
                                                           int jn, int P, int p, int pc, int pb, int qb, double scale) {
  __shared__ double wl[3 * kMaxRank], wr[3 * kMaxRank], cw[kMaxRank];
  const int jj = blockIdx.x / P, k = blockIdx.x - jj * P, t = blockIdx.y;
  const int *bs = bstart + (j0 + jj) * (P + 1);
  panel_sums(partL, bs, wl, k, P, jn, jj, T, t, pb);
  panel_sums(partR, bs, wr, k, P, jn, jj, T, t, pb);
  __syncthreads();
  const double sj = wt ? scale * (double)wt[jj] : scale;
  const int m = threadIdx.x;
  if (m < qb) {
    double ur = 0.0, ul = 0.0;
    for (int n = 0; n < qb; ++n) {
      const double d = d0[m * qb + n];
      ur = __builtin_fma(d, wr[pb + n], ur);
      ul = __builtin_fma(d, wl[pb + n], ul);
    }
    for (int n = 0; n < qb; ++n) {
      const double d = d1[m * qb + n];
      ur = __builtin_fma(d, wr[2 * pb + n], ur);
      ul = __builtin_fma(d, wl[2 * pb + n], ul);
    }
    for (int n = 0; n < qb; ++n) {
      const double d = -d1[n * qb + m];
      ur = __builtin_fma(d, wr[n], ur);
      ul = __builtin_fma(d, wl[n], ul);
    }
    double *u = U + (((size_t)jj * P + k) * T + t) * 2 * qb;
    u[m] = sj * ur;
    u[qb + m] = sj * ul;
  }
  if (m < pb) {
    double s = 0.0;
    if (m < p) {
      for (int n = 0; n < p; ++n) s = __builtin_fma(c0[m * pc + n], wr[pb + n], s);
      for (int n = 0; n < p; ++n) s = __builtin_fma(c1[m * pc + n], wr[2 * pb + n], s);
      for (int n = 0; n < p; ++n) s = __builtin_fma(c1[n * pc + m], wr[n], s);
    }
    cw[m] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int n = 0; n < p; ++n) s = __builtin_fma(wl[pb + n], cw[n], s);
    gsp[((size_t)jj * P + k) * T + t] = s;
  }
}

// (c) of the derivative: lrg_output_kernel with each lane on its own panel's U (read from global memory: P T 2 QB doubles per
// projection do not fit LDS).  Workgroup 0 sums gsp in a fixed order: per component (comp: gout = gcomp, thread jj adds panels,
// then t, ascending) or all of it (gout = gscale: jj, panel, t ascending).  grid (row blocks of 64)
template <int QB>
__global__ __launch_bounds__(256) void lrpg_output_kernel(const float *__restrict__ xl, const uint8_t *__restrict__ pidx,
                                                          const double *__restrict__ U, const double *__restrict__ gsp,
                                                          const float *__restrict__ L, const float *__restrict__ R,
                                                          float *__restrict__ gZ, float *__restrict__ gout, int N, int T, int j0,
                                                          int jn, int ldg, int P, int comp) {
  __shared__ float sres[kOutRows][kPrepMaxJ + 1];
  const int r = threadIdx.x & (kOutRows - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kOutRows);
  const int row0 = blockIdx.x * kOutRows;
  const int i = row0 + r;
  const bool ok = i < N;
  const int ic = ok ? i : N - 1;
  for (int jj = wv; jj < jn; jj += 4) {
    const size_t o = (size_t)(j0 + jj) * N + ic;
    int pk = pidx[o];
    pk = pk < P ? pk : P - 1;
    const double *u = U + ((size_t)jj * P + pk) * T * 2 * QB;
    double q[QB];
#pragma unroll
    for (int m = 0; m < QB; ++m) q[m] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double l = ok ? (double)L[(size_t)i * T + t] : 0.0;
      const double rr = ok ? (double)R[(size_t)i * T + t] : 0.0;
      const double *ut = u + (size_t)t * 2 * QB;
#pragma unroll
      for (int m = 0; m < QB; ++m) q[m] = __builtin_fma(l, ut[m], __builtin_fma(rr, ut[QB + m], q[m]));
    }
    const double x = (double)xl[o], x2 = 2.0 * x;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = QB - 1; k >= 1; --k) {
      const double bk = __builtin_fma(x2, b1, q[k] - b2);
      b2 = b1;
      b1 = bk;
    }
    sres[r][jj] = (float)__builtin_fma(x, b1, q[0] - b2);
  }
  __syncthreads();
  const int rows = N - row0 < kOutRows ? N - row0 : kOutRows;
  for (int e = threadIdx.x; e < rows * jn; e += 256) {
    const int rr = e / jn, c = e - rr * jn;
    gZ[(size_t)(row0 + rr) * ldg + j0 + c] = sres[rr][c];
  }
  if (blockIdx.x != 0) return;
  if (comp) {
    if ((int)threadIdx.x < jn) {
      double s = 0.0;
      for (int k = 0; k < P * T; ++k) s += gsp[(size_t)threadIdx.x * P * T + k];
      gout[j0 + threadIdx.x] = (float)s;
    }
  } else if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < jn * P * T; ++k) s += gsp[k];
    *gout = (float)s;
  }
}

// workspace of the derivative of a panel plan: partL, partR (nbmax x jn x T x PB doubles each), U (jn x P x T x 2 x QB doubles),
// gsp (jn x P x T)
inline size_t panel_grad_ws_bytes(const LowrankPlan &P, int jn, int T) {
  return ((size_t)P.nbmax * jn * T * grad_pb(P) * 2 + (size_t)jn * P.panels * T * (2 * P.qb + 1)) * sizeof(double);
}

// w: the weights (gout = gcomp) or null (gout = gscale)
int launch_panels_grad(const LowrankPlan &P, const float *w, const float *L, const float *R, float *gZ, float *gout, int N,
                       int ldg, int T, int j0, int jn, float scale, void *ws, hipStream_t st) {
  const int pb = grad_pb(P), qb = P.qb;
  const size_t np = (size_t)P.nbmax * jn * T * pb;
  double *partL = reinterpret_cast<double *>(ws), *partR = partL + np;
  double *U = partR + np, *gsp = U + (size_t)jn * P.panels * T * 2 * qb;
  int rc = dispatch_pb<kMaxRank>(pb, [&](auto pbc) {
    constexpr int PB = decltype(pbc)::value;
    hipLaunchKernelGGL(lrp_project_kernel<PB>, dim3(P.nbmax, jn, T), dim3(256), 0, st, P.xs, P.perm, P.bstart, L, partL, T, j0,
                       jn, P.panels, P.nbmax);
    hipLaunchKernelGGL(lrp_project_kernel<PB>, dim3(P.nbmax, jn, T), dim3(256), 0, st, P.xs, P.perm, P.bstart, R, partR, T, j0,
                       jn, P.panels, P.nbmax);
    return (int)hipGetLastError();
  });
  if (rc) return rc;
  hipLaunchKernelGGL(lrpg_combine_kernel, dim3(jn * P.panels, T), dim3(256), 0, st, partL, partR, P.dcoef, P.dcoef1, P.ccoef,
                     P.ccoef1, w ? w + j0 : nullptr, P.bstart, U, gsp, T, j0, jn, P.panels, P.p, P.pb, pb, qb, (double)scale);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  return dispatch_pb<kMaxRank>(qb, [&](auto qbc) {
    constexpr int QB = decltype(qbc)::value;
    hipLaunchKernelGGL(lrpg_output_kernel<QB>, dim3((N + kOutRows - 1) / kOutRows), dim3(256), 0, st, P.xt, P.pidx, U, gsp, L, R,
                       gZ, gout, N, T, j0, jn, ldg, P.panels, w ? 1 : 0);
    return (int)hipGetLastError();
  });
}

// rpgp_lowrank_grad_prepare of a panel plan: [D0][D1][C0][C1], 64 x 64 doubles each, from the blocks the plan's selection
// kept on the host.  The derivative was selected with the plan, at the plan's tolerance: a smaller `tol` is not served.
int panel_grad_prepare(LowrankPlan &P, double tol, void *dcoef, int *q_host, hipStream_t st) {
  if ((tol < kTailTol ? tol : kTailTol) < P.tol || !P.q_sel) return 0;
  double *dd = reinterpret_cast<double *>(dcoef);
  const size_t blk = (size_t)kMaxRank * kMaxRank;
  const std::vector<double> *src[4] = {&P.hd0, &P.hd1, &P.hc0, &P.hc1};
  for (int k = 0; k < 4; ++k) {
    hipError_t e = hipMemcpyAsync(dd + k * blk, src[k]->data(), src[k]->size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  P.q = P.q_sel;
  P.qb = pad8(P.q);
  P.dcoef = dd;
  P.dcoef1 = dd + blk;
  P.ccoef = dd + 2 * blk;
  P.ccoef1 = dd + 3 * blk;
  *q_host = P.q;
  return 0;
}

int create_panel_plan(const void *prep, int64_t N, int J, float max_abs, double tol, int panels, void *plan, size_t plan_bytes,
                      int *panels_host, int *p_host, void **handle_host, hipStream_t st) {
  *panels_host = *p_host = 0;
  *handle_host = nullptr;
  const double h = (double)max_abs * (1.0 + 1.0 / (1 << 20));     // (create_plan's allowance for the rounding at the ends)
  PanelForms F;
  if (!panel_select(h, tol, panels, F)) return 0;         // not served
  const PanelLayout lay(N, J, F.P);
  if (plan_bytes < lay.total) return RPGP_EWORKSPACE;
  LowrankPlan *P = new (std::nothrow) LowrankPlan{};
  if (!P) return RPGP_EINVAL;
  const int pb = pad8(F.p), qb = pad8(F.q);
  char *base = reinterpret_cast<char *>(plan);
  P->p = F.p, P->pb = pb, P->N = N, P->J = J, P->h = h, P->tail = F.b[0] > F.b[1] ? F.b[0] : F.b[1];
  P->tol = tol;
  P->panels = F.P, P->hp = F.hp, P->nbmax = panel_nbmax(N, F.P);
  for (int k = 0; k < 3; ++k) P->bounds[k] = F.b[k];
  float *coef0 = reinterpret_cast<float *>(base + lay.coef0), *coef1 = reinterpret_cast<float *>(base + lay.coef1);
  float *xl = reinterpret_cast<float *>(base + lay.xl), *xs = reinterpret_cast<float *>(base + lay.xs);
  int *perm = reinterpret_cast<int *>(base + lay.perm), *bstart = reinterpret_cast<int *>(base + lay.bstart);
  uint8_t *pidx = reinterpret_cast<uint8_t *>(base + lay.pidx);
  P->coef = coef0, P->coef1 = coef1, P->xt = xl, P->xs = xs, P->perm = perm, P->bstart = bstart, P->pidx = pidx;
  std::vector<float> cf0((size_t)pb * pb, 0.f), cf1((size_t)pb * pb, 0.f);
  copy_leading_block(F.c0, F.p, cf0.data(), pb);
  copy_leading_block(F.c1, F.p, cf1.data(), pb);
  P->q_sel = F.q;
  P->hd0.assign((size_t)qb * qb, 0.0), P->hd1.assign((size_t)qb * qb, 0.0);
  P->hc0.assign((size_t)pb * pb, 0.0), P->hc1.assign((size_t)pb * pb, 0.0);
  copy_leading_block(F.d0, F.q, P->hd0.data(), qb);
  copy_leading_block(F.d1, F.q, P->hd1.data(), qb);
  copy_leading_block(F.c0, F.p, P->hc0.data(), pb);
  copy_leading_block(F.c1, F.p, P->hc1.data(), pb);
  int rc = (int)hipMemcpyAsync(coef0, cf0.data(), cf0.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (!rc) rc = (int)hipMemcpyAsync(coef1, cf1.data(), cf1.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (!rc) {
    const long long total = N * J;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    const float2v *rowdat = reinterpret_cast<const float2v *>(reinterpret_cast<const float *>(prep) + kPrepRowdatOffsetFloats);
    hipLaunchKernelGGL(lrp_coords_kernel, dim3(blocks), dim3(256), 0, st, rowdat, xl, pidx, (long long)N, J, h, F.hp, 1.0 / F.hp,
                       F.P);
    hipLaunchKernelGGL(lrp_sort_kernel, dim3(J), dim3(256), 0, st, pidx, xl, perm, xs, bstart, (int)N, F.P, P->nbmax);
    rc = (int)hipGetLastError();
  }
  if (!rc) rc = (int)hipStreamSynchronize(st);            // (the host copies of the coefficients go out of scope)
  if (rc) {
    delete P;
    return rc;
  }
  *panels_host = F.P;
  *p_host = F.p;
  *handle_host = P;
  return 0;
}

// ---- the launch of a plan of any kind: panels, a padded rank above 64, a padded rank up to 64 -----------------------------------
// The extern "C" entries check their own arguments and workspace size and then call these two.  w: the weights or null.

// rows [r0, r1) of the product (all of them unless the call is pair-sharded); the workspace holds J columns
int product(const LowrankPlan &P, const float *w, const float *V, float *out, int N, int T, int j0, int jn, int r0, int r1,
            float scale, float noise, void *workspace, hipStream_t st) {
  const bool prof = rpgp_internal::prof_open(st);
  int rc;
  if (P.panels) {
    rc = launch_panels(P, w, V, out, N, T, j0, jn, r0, r1, scale, noise, workspace, st);
  } else {
    double *part = reinterpret_cast<double *>(workspace);
    float *U = reinterpret_cast<float *>(part + (size_t)proj_blocks(N) * jn * T * P.pb);
    rc = dispatch_pb<kCapRank>(P.pb, [&](auto pb) {
      constexpr int PB = decltype(pb)::value;
      if constexpr (PB <= kMaxRank)
        return launch_lowrank<PB>(P, w, V, out, N, T, j0, jn, r0, r1, scale, noise, part, U, st);
      else
        return launch_lowrank_wide<PB>(P, w, V, out, N, T, j0, jn, r0, r1, scale, noise, part, U, st);
    });
  }
  if (prof) {
    const int pc = rpgp_internal::prof_close(st);
    if (!rc) rc = pc;
  }
  return rc;
}

// workspace of the derivative of jn columns
inline size_t derivative_ws_bytes(const LowrankPlan &P, int64_t N, int jn, int T) {
  return P.panels ? panel_grad_ws_bytes(P, jn, T) : grad_ws_bytes(P, N, jn, T);
}

// gout: gcomp with weights, gscale without
int derivative(const LowrankPlan &P, const float *w, const float *L, const float *R, float *gZ, float *gout, int N, int ldg,
               int T, int j0, int jn, float scale, void *workspace, hipStream_t st) {
  if (P.panels) return launch_panels_grad(P, w, L, R, gZ, gout, N, ldg, T, j0, jn, scale, workspace, st);
  if (grad_pb(P) > kMaxRank) return launch_grad_wide(P, w, L, R, gZ, gout, N, ldg, T, j0, jn, scale, workspace, st);
  // (PB < QB never occurs: PB = pad8(max(p, q)) >= QB, so no such kernel is instantiated)
  return dispatch_pb<kMaxRank>(P.qb, [&](auto qb) {
    return dispatch_pb<kMaxRank>(grad_pb(P), [&](auto pb) -> int {
      constexpr int QB = decltype(qb)::value, PB = decltype(pb)::value;
      if constexpr (PB >= QB)
        return launch_grad<PB, QB>(P, w, L, R, gZ, gout, N, ldg, T, j0, jn, scale, workspace, st);
      else
        return RPGP_EINVAL;
    });
  });
}

}  // namespace

extern "C" {

int rpgp_lowrank_panels_select(double h, double tol, int panels, int *panels_host, double *hp_host, int *p_host, int *q_host,
                               double *bounds_host, double *dbounds_host, double *coef_host) {
  if (!panels_host || !(tol > 0.0) || panels < 0 || panels == 1 || panels > kMaxPanels) return RPGP_EINVAL;
  *panels_host = 0;
  PanelForms F;
  if (!panel_select(h, tol < kTailTol ? tol : kTailTol, panels, F)) return 0;
  *panels_host = F.P;
  if (hp_host) *hp_host = F.hp;
  if (p_host) *p_host = F.p;
  if (q_host) *q_host = F.q;
  for (int k = 0; k < 3; ++k) {
    if (bounds_host) bounds_host[k] = F.b[k];
    if (dbounds_host) dbounds_host[k] = F.d[k];
  }
  if (coef_host) {                                        // [C0][C1][D0][D1], 64 x 64 doubles each, zero outside p x p / q x q
    const size_t blk = (size_t)kMaxRank * kMaxRank;
    for (size_t e = 0; e < 4 * blk; ++e) coef_host[e] = 0.0;
    copy_leading_block(F.c0, F.p, coef_host, kMaxRank);
    copy_leading_block(F.c1, F.p, coef_host + blk, kMaxRank);
    copy_leading_block(F.d0, F.q, coef_host + 2 * blk, kMaxRank);
    copy_leading_block(F.d1, F.q, coef_host + 3 * blk, kMaxRank);
  }
  return 0;
}

int rpgp_lowrank_panels_max(void) { return kMaxPanels; }

size_t rpgp_lowrank_panels_plan_bytes(int64_t N, int J) {
  if (N <= 0 || N > 0x7fffffffLL || J <= 0 || J > kPrepMaxJ) return 0;
  return PanelLayout(N, J, kMaxPanels).total;
}

int rpgp_lowrank_create_panels(const void *prep, int64_t N, int J, float max_abs, double tol, int panels, void *plan,
                               size_t plan_bytes, int *panels_host, int *p_host, void **handle_host, void *stream) {
  if (!prep || !plan || !panels_host || !p_host || !handle_host || N <= 0 || N > 0x7fffffffLL || J <= 0 || J > kPrepMaxJ)
    return RPGP_EINVAL;
  if (!(tol > 0.0) || panels < 0 || panels == 1 || panels > kMaxPanels) return RPGP_EINVAL;
  // (the sorted slots of a column are indexed by int: N / 2048 + 16 blocks of 2048 stay below 2^31 for every N up to 2^31 - 2^16)
  if (N > 0x7fffffffLL - 65536) return RPGP_EINVAL;
  return create_panel_plan(prep, N, J, max_abs, tol < kTailTol ? tol : kTailTol, panels, plan, plan_bytes, panels_host, p_host,
                           handle_host, reinterpret_cast<hipStream_t>(stream));
}

int rpgp_lowrank_panels_info(const void *handle, int *panels_host, double *hp_host, int *p_host, int *q_host,
                             double *bounds_host) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P) return RPGP_EINVAL;
  if (panels_host) *panels_host = P->panels;
  if (hp_host) *hp_host = P->panels ? P->hp : P->h;
  if (p_host) *p_host = P->p;
  if (q_host) *q_host = P->panels ? P->q_sel : P->q;
  if (bounds_host)
    for (int k = 0; k < 3; ++k) bounds_host[k] = P->bounds[k];
  return 0;
}

int rpgp_lowrank_select(double h, int p_max, int *p_host, double *tail_host, double *coef_host) {
  return select_to_host(h, p_max, kTailTol, false, p_host, tail_host, coef_host);
}

size_t rpgp_lowrank_plan_bytes(int64_t N, int J) { return rpgp_lowrank_plan_bytes_cap(N, J, kMaxRank); }

size_t rpgp_lowrank_plan_bytes_cap(int64_t N, int J, int p_max) {
  if (N <= 0 || J <= 0 || J > kPrepMaxJ || p_max < 1 || p_max > kCapRank) return 0;
  const size_t ld = cap_ld(p_max);
  return (ld * ld + (size_t)N * J) * sizeof(float);
}

int rpgp_lowrank_create_cap(const void *prep, int64_t N, int J, float max_abs, double tol, int p_max, void *plan,
                            size_t plan_bytes, int *p_host, void **handle_host, void *stream) {
  if (!(tol > 0.0) || p_max < 1 || p_max > kCapRank) return RPGP_EINVAL;
  return create_plan(prep, N, J, max_abs, tol < kTailTol ? tol : kTailTol, plan, plan_bytes, p_host, handle_host, stream, p_max);
}

size_t rpgp_lowrank_grad_bytes(const void *handle) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P) return 0;
  if (P->panels) return (size_t)4 * kMaxRank * kMaxRank * sizeof(double);      // D0, D1, C0, C1
  return (size_t)2 * P->ld * P->ld * sizeof(double);      // D and C (64: RPGP_LOWRANK_GRAD_BYTES)
}

int rpgp_lowrank_create(const void *prep, int64_t N, int J, float max_abs, void *plan, size_t plan_bytes, int *p_host,
                        void **handle_host, void *stream) {
  return create_plan(prep, N, J, max_abs, kTailTol, plan, plan_bytes, p_host, handle_host, stream);
}

int rpgp_lowrank_create_tol(const void *prep, int64_t N, int J, float max_abs, double tol, void *plan, size_t plan_bytes,
                            int *p_host, void **handle_host, void *stream) {
  return rpgp_lowrank_create_cap(prep, N, J, max_abs, tol, kMaxRank, plan, plan_bytes, p_host, handle_host, stream);
}

int rpgp_lowrank_destroy(void *handle) {
  delete reinterpret_cast<LowrankPlan *>(handle);
  return 0;
}

size_t rpgp_mvm_sym_lowrank_workspace_bytes(const void *handle, int64_t N, int T) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || N <= 0 || N > 0x7fffffffLL || T <= 0) return 0;
  if (P->panels) return panel_ws_bytes(*P, P->J, T);
  return (size_t)P->J * T * P->pb * ((size_t)proj_blocks(N) * sizeof(double) + sizeof(float));
}

int rpgp_mvm_sym_lowrank_range(const void *handle, const void *prep, const float *V, float *out, int64_t N, int J, int T,
                               int j0, int j1, int world, int rank, float scale, float noise, void *workspace,
                               size_t workspace_bytes, void *stream) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || !prep || !V || !out || N <= 0 || T <= 0 || J <= 0 || J > kPrepMaxJ || j0 < 0 || j1 <= j0 || j1 > J)
    return RPGP_EINVAL;
  if (N != P->N || J != P->J || T > 65535) return RPGP_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return RPGP_EINVAL;
  const size_t need = rpgp_mvm_sym_lowrank_workspace_bytes(handle, N, T);
  if (!workspace || workspace_bytes < need) return RPGP_EWORKSPACE;
  const int n = (int)N;
  // a rank of a pair-sharded call writes its row slice of K v (and the noise term, if it was given one, on every row)
  const int r0 = (int)((int64_t)n * rank / world), r1 = (int)((int64_t)n * (rank + 1) / world);
  return product(*P, nullptr, V, out, n, T, j0, j1 - j0, r0, r1, scale, noise, workspace, reinterpret_cast<hipStream_t>(stream));
}

int rpgp_lowrank_grad_select(double h, int q_max, double tol, int *q_host, double *tail_host, double *coef_host) {
  return select_to_host(h, q_max, tol, true, q_host, tail_host, coef_host);
}

int rpgp_lowrank_grad_prepare(void *handle, double tol, void *dcoef, size_t dcoef_bytes, int *q_host, void *stream) {
  LowrankPlan *P = reinterpret_cast<LowrankPlan *>(handle);
  if (!P || !dcoef || !q_host || !(tol > 0.0)) return RPGP_EINVAL;
  if (dcoef_bytes < rpgp_lowrank_grad_bytes(handle)) return RPGP_EWORKSPACE;
  *q_host = 0;
  P->q = P->qb = 0;
  P->dcoef = nullptr;
  if (P->panels) return panel_grad_prepare(*P, tol, dcoef, q_host, reinterpret_cast<hipStream_t>(stream));
  std::vector<double> c;
  double tail = 0.0;
  const int q = select_rank(P->h, P->cap, tol < kTailTol ? tol : kTailTol, &tail, c, true);
  // (a rank-1 plan stores x = 0: it cannot evaluate a derivative of rank > 1)
  if (q == 0 || (P->p == 1 && q > 1)) return 0;
  const int qb = pad8(q);
  // [D: qb x qb][C: pb x pb at ld x ld doubles: 32 KiB for ld = 64], both float64; C is the plan's own selection again (same h,
  // tolerance and cap: same p)
  std::vector<double> d((size_t)qb * qb, 0.0), cc((size_t)P->pb * P->pb, 0.0), cf;
  copy_leading_block(c, q, d.data(), qb);
  if (select_rank(P->h, P->cap, P->tol, nullptr, cf) != P->p) return RPGP_EINVAL;
  copy_leading_block(cf, P->p, cc.data(), P->pb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double *dd = reinterpret_cast<double *>(dcoef), *dc = dd + (size_t)P->ld * P->ld;
  hipError_t e = hipMemcpyAsync(dd, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(dc, cc.data(), cc.size() * sizeof(double), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  P->q = q;
  P->qb = qb;
  P->dcoef = dd;
  P->ccoef = dc;
  *q_host = q;
  return 0;
}

size_t rpgp_bilinear_grad_lowrank_workspace_bytes(const void *handle, int64_t N, int T) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || !P->q || N <= 0 || N > 0x7fffffffLL || T <= 0) return 0;
  return derivative_ws_bytes(*P, N, P->J, T);
}

int rpgp_bilinear_grad_lowrank(const void *handle, const float *L, const float *R, float *gZ, float *gscale, int64_t N,
                               int ldg, int T, int j0, int j1, float scale, void *workspace, size_t workspace_bytes,
                               void *stream) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || !L || !R || !gZ || !gscale || N <= 0 || T <= 0 || T > 65535) return RPGP_EINVAL;
  if (N != P->N || j0 < 0 || j1 <= j0 || j1 > P->J || ldg < P->J) return RPGP_EINVAL;
  if (!P->q) return RPGP_EINVAL;                          // no derivative rank: the caller runs rpgp_bilinear_grad
  if (!workspace || workspace_bytes < derivative_ws_bytes(*P, N, j1 - j0, T)) return RPGP_EWORKSPACE;
  return derivative(*P, nullptr, L, R, gZ, gscale, (int)N, ldg, T, j0, j1 - j0, scale, workspace,
                    reinterpret_cast<hipStream_t>(stream));
}

int rpgp_mvm_sym_lowrank_weighted(const void *handle, const void *prep, const float *weights, const float *V, float *out,
                                  int64_t N, int J, int T, int j0, int j1, float scale, float noise, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || !prep || !weights || !V || !out || N <= 0 || T <= 0 || J <= 0 || J > kPrepMaxJ || j0 < 0 || j1 <= j0 || j1 > J)
    return RPGP_EINVAL;
  if (N != P->N || J != P->J || T > 65535) return RPGP_EINVAL;
  const size_t need = rpgp_mvm_sym_lowrank_workspace_bytes(handle, N, T);
  if (!workspace || workspace_bytes < need) return RPGP_EWORKSPACE;
  const int n = (int)N;
  return product(*P, weights, V, out, n, T, j0, j1 - j0, 0, n, scale, noise, workspace, reinterpret_cast<hipStream_t>(stream));
}

int rpgp_bilinear_grad_lowrank_weighted(const void *handle, const float *weights, const float *L, const float *R, float *gZ,
                                        float *gcomp, int64_t N, int J, int T, int j0, int j1, float scale, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  const LowrankPlan *P = reinterpret_cast<const LowrankPlan *>(handle);
  if (!P || !weights || !L || !R || !gZ || !gcomp || N <= 0 || T <= 0 || T > 65535) return RPGP_EINVAL;
  if (N != P->N || J != P->J || j0 < 0 || j1 <= j0 || j1 > J) return RPGP_EINVAL;
  if (!P->q) return RPGP_EINVAL;                          // no derivative rank: the caller runs rpgp_family_bilinear_grad
  if (!workspace || workspace_bytes < derivative_ws_bytes(*P, N, j1 - j0, T)) return RPGP_EWORKSPACE;
  return derivative(*P, weights, L, R, gZ, gcomp, (int)N, P->J, T, j0, j1 - j0, scale, workspace,
                    reinterpret_cast<hipStream_t>(stream));
}

int rpgp_lowrank_post_select(double h, double tol, int p_max, int *p_host, int *r_host, double *tail_host, double *G_host) {
  if (!p_host || !r_host || p_max < 1 || p_max > kRefDegree || !(tol > 0.0)) return RPGP_EINVAL;
  *p_host = *r_host = 0;
  if (tail_host) *tail_host = 0.0;
  std::vector<double> c;
  double tail = 0.0;
  const int p = select_rank(h, p_max, tol, &tail, c);
  if (p == 0) return 0;
  std::vector<double> a((size_t)p * p), q, l;
  for (int m = 0; m < p; ++m)
    for (int n = 0; n < p; ++n)
      a[(size_t)m * p + n] = 0.5 * (c[(size_t)m * kRefDegree + n] + c[(size_t)n * kRefDegree + m]);
  if (p <= kMaxRank)
    jacobi_eigh(a, p, q, l);
  else
    tridiagonal_ql_eigh(a, p, q, l);
  // eigenpairs in descending order (ties: the lower index first); negative eigenvalues are always dropped, then the smallest
  // while p * sum |dropped l| <= tol: |T(x)^T (C - G G^T) T(y)| <= sum_dropped |l| (q^T T(x)) (q^T T(y)) <= p sum |l|
  std::vector<int> ord(p);
  for (int i = 0; i < p; ++i) ord[i] = i;
  for (int i = 1; i < p; ++i)                             // insertion sort: stable, deterministic
    for (int k = i; k > 0 && l[ord[k]] > l[ord[k - 1]]; --k) {
      const int t = ord[k];
      ord[k] = ord[k - 1];
      ord[k - 1] = t;
    }
  int r = p;
  double dropped = 0.0;
  while (r > 0 && l[ord[r - 1]] < 0.0) dropped += fabs(l[ord[--r]]);
  while (r > 1 && p * (dropped + l[ord[r - 1]]) <= tol) dropped += l[ord[--r]];
  if (r < 1) return 0;
  std::vector<double> g((size_t)p * r);
  for (int m = 0; m < p; ++m)
    for (int k = 0; k < r; ++k) g[(size_t)m * r + k] = q[(size_t)m * p + ord[k]] * sqrt(l[ord[k]]);
  // the bound also covers the factorisation's own rounding: the entrywise sum of |C - G G^T| bounds |T(x)^T (C - G G^T) T(y)|
  double resid = 0.0;
  for (int m = 0; m < p; ++m)
    for (int n = 0; n < p; ++n) {
      double s = 0.0;
      for (int k = 0; k < r; ++k) s += g[(size_t)m * r + k] * g[(size_t)n * r + k];
      resid += fabs(c[(size_t)m * kRefDegree + n] - s);
    }
  const double bound = (p * dropped > resid ? p * dropped : resid) * (1.0 + 1e-12) + 1e-15;
  *p_host = p;
  *r_host = r;
  if (tail_host) *tail_host = tail + bound;
  if (G_host)
    for (int m = 0; m < p; ++m)
      for (int k = 0; k < r; ++k) G_host[(size_t)m * p_max + k] = g[(size_t)m * r + k];
  return 0;
}

int rpgp_lowrank_features_f64(const double *Z, int64_t N, int J, int ldz, const double *mid, double inv_w, const double *G,
                              int p, int r, double sqrt_scale, double *B, int64_t ldb, void *stream) {
  if (!Z || !mid || !G || !B || N < 1 || J < 1 || J > kPrepMaxJ || ldz < J || p < 1 || p > kFeatMaxRank || r < 1 || r > p ||
      ldb < (int64_t)J * r || N > ((int64_t)1 << 36))
    return RPGP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + kFeatRows - 1) / kFeatRows));
  return dispatch_pb<kFeatMaxRank>(pad8(p), [&](auto pb) {
    return launch_features(lr_features_kernel<decltype(pb)::value>, pb, r, grid, st, Z, (long long)N, J, ldz, mid, inv_w, G, p,
                           r, sqrt_scale, B, (long long)ldb);
  });
}

int rpgp_lowrank_features_grad_f64(const double *Z, int64_t N, int J, int ldz, const double *mid, double inv_w,
                                   const double *Gd, int p, int r, double sqrt_scale, const double *Y, int64_t ldy,
                                   const double *alpha, const double *v, double ca, double cy, double *gZ, int64_t ldg,
                                   void *stream) {
  if (!Z || !mid || !Gd || !Y || !alpha || !v || !gZ || N < 1 || J < 1 || J > kPrepMaxJ || ldz < J || p < 1 ||
      p > kFeatMaxRank || r < 1 || r > p || ldy < (int64_t)J * r || ldg < J || N > ((int64_t)1 << 36))
    return RPGP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + kFeatRows - 1) / kFeatRows));
  const double fac = sqrt_scale * inv_w;
  return dispatch_pb<kFeatMaxRank>(pad8(p), [&](auto pb) {
    return launch_features(lr_features_grad_kernel<decltype(pb)::value>, pb, r, grid, st, Z, (long long)N, J, ldz, mid, inv_w,
                           Gd, p, r, fac, Y, (long long)ldy, alpha, v, ca, cy, gZ, (long long)ldg);
  });
}

int rpgp_lowrank_features_cols_f64(const double *Z, int64_t N, int nc, int ldz, const int32_t *cols, const double *mid,
                                   double inv_w, const double *G, int p, int r, const double *col_scale, double *B, int64_t ldb,
                                   void *stream) {
  if (!Z || !cols || !mid || !G || !col_scale || !B || N < 1 || nc < 1 || nc > kPrepMaxJ || ldz < nc || p < 1 ||
      p > kFeatMaxRank || r < 1 || r > p || ldb < (int64_t)nc * r || N > ((int64_t)1 << 36))
    return RPGP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + kFeatRows - 1) / kFeatRows));
  return dispatch_pb<kFeatMaxRank>(pad8(p), [&](auto pb) {
    return launch_features(lr_features_cols_kernel<decltype(pb)::value>, pb, r, grid, st, Z, (long long)N, nc, ldz,
                           (const int *)cols, mid, inv_w, G, p, r, col_scale, B, (long long)ldb);
  });
}

int rpgp_lowrank_features_grad_cols_f64(const double *Z, int64_t N, int nc, int ldz, const int32_t *cols, const double *mid,
                                        double inv_w, const double *Gd, int p, int r, const double *col_scale, const double *Y,
                                        int64_t ldy, const double *alpha, const double *v, double ca, double cy, double *gZ,
                                        int64_t ldg, void *stream) {
  if (!Z || !cols || !mid || !Gd || !col_scale || !Y || !alpha || !v || !gZ || N < 1 || nc < 1 || nc > kPrepMaxJ ||
      ldz < nc || p < 1 || p > kFeatMaxRank || r < 1 || r > p || ldy < (int64_t)nc * r || ldg < nc || N > ((int64_t)1 << 36))
    return RPGP_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + kFeatRows - 1) / kFeatRows));
  return dispatch_pb<kFeatMaxRank>(pad8(p), [&](auto pb) {
    return launch_features(lr_features_grad_cols_kernel<decltype(pb)::value>, pb, r, grid, st, Z, (long long)N, nc, ldz,
                           (const int *)cols, mid, inv_w, Gd, p, r, col_scale, Y, (long long)ldy, alpha, v, ca, cy, gZ,
                           (long long)ldg);
  });
}

}  // extern "C"
