// rpgp_ski_post.hip — the two passes over the rows that the closed-form posterior of the grid-interpolation (SKI) models needs
// (ski_posterior.py).  With w_i the row of 4 J cubic-convolution weights of point i placed in a vector of J G
// entries (the stencil rule of every SKI kernel here: rpgp_ski_f64.hip `taps`):
//     rpgp_ski_gram_f64       A = sum_i w_i w_i^T (J G x J G),   g = sum_i w_i Y_i^T (J G x T)
//     rpgp_ski_quadform_f64   out[i] = w_i^T C w_i
// float64 throughout, no float atomics, every sum in a fixed order: a repeated call is bit-identical.
//
// The Gram pass keeps the OUTPUT stationary.  Plan (k_cell_rank, k_cell_scan, k_cell_start, k_place): every projection's rows
// in a STABLE counting sort by first-tap cell — chunks of 256 rows, a row's position = start of its cell + rows of that cell
// in earlier chunks + its rank among the rows of that cell in its own chunk, all prefix sums — so the sorted order is
// ascending row index inside a cell, whatever the launch does.  Product (k_gram): a workgroup owns a strip of S rows of A
// (S nodes of projection j) against a chunk of Jc projections j' >= j, S x Jc x G doubles in LDS.  It walks the contiguous
// segment of sorted rows whose stencil can reach the strip (cells a0 - 3 .. a0 + S - 1), one row per step; thread (s, j', r)
// adds w_j[a0 + s] w_j'[n] for the one tap n = r (mod 4) of that row's stencil in j' — the 4 S Jc targets of a step are distinct,
// and an LDS address is only ever touched by the same thread (n mod 4 is the thread's), so the loop needs no barrier.  The
// block rows j' > j are computed once and mirrored (k_mirror); inside a diagonal block (j' = j) entry (a, b) and entry (b, a)
// see the same rows in the same order and the same two factors, so A == A^T bitwise.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/rpgp.h"
#include "rpgp_internal.h"

namespace {

using rpgp_internal::launch_status;
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int kChunk = 256;         // rows per chunk of the counting sort
constexpr int kMaxG = 8192;         // one G-wide strip row of doubles within kLdsBytes
constexpr int kLdsBytes = 65536;    // dynamic LDS of k_gram
constexpr int kMaxT = 16;

__device__ __forceinline__ double cubic_w(double U) {
  return (U < 1.0) ? ((1.5 * U - 2.5) * U) * U + 1.0 : ((-0.5 * U + 2.5) * U - 4.0) * U + 2.0;
}
__device__ __forceinline__ int gp_flags(const double *__restrict__ gp) { return (int)gp[3]; }
__device__ __forceinline__ const double *gp_grid(const double *__restrict__ gp, int J, int j) {
  return (gp_flags(gp) & 2) ? gp + 4 + J + 3 * j : gp;
}
// first tap (in [0, G - 4]) and tap fraction of z: the rule of `taps` (rpgp_ski_f64.hip), same arithmetic
__device__ __forceinline__ int cell_of(double z, double g0, double inv_h, int G, double &fr) {
  double u = (z - g0) * inv_h;
  u = u < 1.0 ? 1.0 : (u > (double)(G - 2) ? (double)(G - 2) : u);
  const double fl = floor(u);
  fr = u - fl;
  const int idx0 = (int)fl - 1;
  return idx0 < 0 ? 0 : (idx0 > G - 4 ? G - 4 : idx0);
}
// weight of tap q = 0 .. 3 for the tap fraction fr
__device__ __forceinline__ double tap_w(double fr, int q) {
  return cubic_w(q == 0 ? fr + 1.0 : (q == 1 ? fr : (q == 2 ? 1.0 - fr : 2.0 - fr)));
}

// ---- plan: stable counting sort of every projection's rows by cell ------------------------------------------------------------
// cellrank[j][i] = (cell, rank of row i among the rows of that cell in its chunk); counts[j][cell][chunk] = rows of the cell in
// the chunk (written by the last such row; zero-filled before)
__global__ __launch_bounds__(kChunk) void k_cell_rank(const double *__restrict__ Z, const double *__restrict__ gp,
                                                       int2 *__restrict__ cellrank, int *__restrict__ counts, long long N,
                                                       int ldz, int J, int G, int nchunk) {
  __shared__ int cells[kChunk];
  const int j = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
  const long long i = (long long)chunk * kChunk + t;
  int cell = -1;
  if (i < N) {
    const double *gj = gp_grid(gp, J, j);
    double fr;
    cell = cell_of(Z[i * ldz + j], gj[0], gj[2], G, fr);
  }
  cells[t] = cell;
  __syncthreads();
  if (i >= N) return;
  int rank = 0, later = 0;
  for (int u = 0; u < kChunk; ++u) {
    const int same = cells[u] == cell;
    rank += same & (u < t);
    later |= same & (u > t);
  }
  cellrank[(size_t)j * N + i] = make_int2(cell, rank);
  if (!later) counts[((size_t)j * (G - 3) + cell) * nchunk + chunk] = rank + 1;
}

// a wave per (j, cell): counts[j][cell][.] -> its exclusive prefix over the chunks, cellsum[j][cell] = its total
__global__ __launch_bounds__(256) void k_cell_scan(int *__restrict__ counts, int *__restrict__ cellsum, int ncell, int nchunk) {
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6), j = blockIdx.y, lane = threadIdx.x & 63;
  if (cell >= ncell) return;
  int *c = counts + ((size_t)j * ncell + cell) * nchunk;
  int run = 0;
  for (int base = 0; base < nchunk; base += 64) {
    const int k = base + lane;
    const int v = k < nchunk ? c[k] : 0;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (k < nchunk) c[k] = run + x - v;
    run += __shfl(x, 63);
  }
  if (lane == 0) cellsum[(size_t)j * ncell + cell] = run;
}

// a workgroup per j: start[j][cell] = rows in the cells before it, start[j][ncell] = N
__global__ __launch_bounds__(1024) void k_cell_start(const int *__restrict__ cellsum, int *__restrict__ start, int ncell, int N) {
  __shared__ int part[1024];
  const int j = blockIdx.x, t = threadIdx.x;
  const int *cs = cellsum + (size_t)j * ncell;
  int *st = start + (size_t)j * (ncell + 1);
  const int per = (ncell + 1023) / 1024;
  const int b = t * per < ncell ? t * per : ncell, e = b + per < ncell ? b + per : ncell;
  int s = 0;
  for (int k = b; k < e; ++k) s += cs[k];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int k = b; k < e; ++k) {
    st[k] = run;
    run += cs[k];
  }
  if (t == 0) st[ncell] = N;
}

__global__ __launch_bounds__(256) void k_place(const int2 *__restrict__ cellrank, const int *__restrict__ counts,
                                               const int *__restrict__ start, int *__restrict__ perm, long long N, int ncell,
                                               int nchunk) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= N) return;
  const int2 cr = cellrank[(size_t)j * N + i];
  const long long p = (long long)start[(size_t)j * (ncell + 1) + cr.x] +
                      counts[((size_t)j * ncell + cr.x) * nchunk + (int)(i / kChunk)] + cr.y;
  if (p >= 0 && p < N) perm[(size_t)j * N + p] = (int)i;
}

// ---- the product ---------------------------------------------------------------------------------------------------------------
// grid (strips of S nodes, j, chunks of Jc projections from j on); 4 S Jc threads rounded up to waves; acc: S Jc rows of GP doubles
template <int S>
__global__ __launch_bounds__(256) void k_gram(const double *__restrict__ Z, const double *__restrict__ gp,
                                              const int *__restrict__ perm, const int *__restrict__ start, double *__restrict__ A,
                                              long long N, int ldz, int J, int G, int Jc, int GP) {
  extern __shared__ double acc[];
  const int a0 = blockIdx.x * S, j = blockIdx.y, jp0 = j + blockIdx.z * Jc;
  if (jp0 >= J) return;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int jn = J - jp0 < Jc ? J - jp0 : Jc;
  for (int e = tid; e < S * Jc * GP; e += nt) acc[e] = 0.0;
  __syncthreads();
  const int r = tid & 3, s = (tid >> 2) % S, jl = tid / (4 * S);
  const int a = a0 + s;
  if (jl < jn && a < G) {
    const int jp = jp0 + jl;
    const double *gj = gp_grid(gp, J, j), *gjp = gp_grid(gp, J, jp);
    const double g0 = gj[0], ih = gj[2], g0p = gjp[0], ihp = gjp[2];
    const int c_lo = a0 - 3 > 0 ? a0 - 3 : 0, c_hi = a0 + S - 1 < G - 4 ? a0 + S - 1 : G - 4;
    const int *pj = perm + (size_t)j * N, *sj = start + (size_t)j * (G - 2);
    const int k0 = sj[c_lo] > 0 ? sj[c_lo] : 0, k1 = sj[c_hi + 1] < N ? sj[c_hi + 1] : (int)N;
    double *row = acc + (size_t)(s * Jc + jl) * GP;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
      const long long i = pj[k];
      if ((unsigned long long)i >= (unsigned long long)N) continue;   // (never with a sound plan: no read outside Z either way)
      double fr, frp;
      const int q = a - cell_of(Z[i * ldz + j], g0, ih, G, fr);
      const int cp = cell_of(Z[i * ldz + jp], g0p, ihp, G, frp);
      if (q >= 0 && q <= 3) {
        const int qp = (r - cp) & 3;                       // the tap of this row's stencil on a node = r (mod 4)
        row[cp + qp] = fma(tap_w(fr, q), tap_w(frp, qp), row[cp + qp]);
      }
    }
  }
  __syncthreads();
  const size_t ldA = (size_t)J * G;
  for (int e = tid; e < S * jn * G; e += nt) {
    const int n = e % G, rj = e / G, l = rj % jn, ss = rj / jn;
    if (a0 + ss < G) A[((size_t)j * G + a0 + ss) * ldA + (size_t)(jp0 + l) * G + n] = acc[(size_t)(ss * Jc + l) * GP + n];
  }
}

// A[(j', b)][(j, a)] = A[(j, a)][(j', b)] for j < j': 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void k_mirror(double *__restrict__ A, int G, long long n) {
  __shared__ double tile[32][33];
  const long long r0 = (long long)blockIdx.y * 32, c0 = (long long)blockIdx.x * 32;
  if ((c0 + 31) / G <= r0 / G) return;                    // no entry of the tile lies in a block row above its block column
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int y = ty; y < 32; y += 8) {
    const long long rr = r0 + y, cc = c0 + tx;
    if (rr < n && cc < n && rr / G < cc / G) tile[y][tx] = A[rr * n + cc];
  }
  __syncthreads();
  for (int y = ty; y < 32; y += 8) {
    const long long cc = c0 + y, rr = r0 + tx;
    if (rr < n && cc < n && rr / G < cc / G) A[cc * n + rr] = tile[tx][y];
  }
}

// g[(j, a)][t] = sum_i w_j(i)[a] Y[i][t]: thread (s, t) of a strip of 4 nodes, the sum in a register
__global__ __launch_bounds__(64) void k_gram_rhs(const double *__restrict__ Z, const double *__restrict__ gp,
                                                 const int *__restrict__ perm, const int *__restrict__ start,
                                                 const double *__restrict__ Y, double *__restrict__ g, long long N, int ldz, int J,
                                                 int G, int T) {
  const int a0 = blockIdx.x * 4, j = blockIdx.y, t = threadIdx.x & 15, a = a0 + (threadIdx.x >> 4);
  if (t >= T || a >= G) return;
  const double *gj = gp_grid(gp, J, j);
  const double g0 = gj[0], ih = gj[2];
  const int c_lo = a0 - 3 > 0 ? a0 - 3 : 0, c_hi = a0 + 3 < G - 4 ? a0 + 3 : G - 4;
  const int *pj = perm + (size_t)j * N, *sj = start + (size_t)j * (G - 2);
  const int k0 = sj[c_lo] > 0 ? sj[c_lo] : 0, k1 = sj[c_hi + 1] < N ? sj[c_hi + 1] : (int)N;
  double acc = 0.0;
#pragma unroll 4
  for (int k = k0; k < k1; ++k) {
    const long long i = pj[k];
    if ((unsigned long long)i >= (unsigned long long)N) continue;
    double fr;
    const int q = a - cell_of(Z[i * ldz + j], g0, ih, G, fr);
    if (q >= 0 && q <= 3) acc = fma(tap_w(fr, q), Y[i * T + t], acc);
  }
  g[((size_t)j * G + a) * T + t] = acc;
}

// out[i] = sum_c w_c (sum_r w_r C[r][c]) over the 4 J taps r and c of row i: a wave per row, lane l takes the columns
// c = l, l + 64, ..; the lanes' sums meet in a butterfly (every lane ends with the same bits)
__global__ __launch_bounds__(256) void k_quadform(const double *__restrict__ Z, const double *__restrict__ gp,
                                                  const double *__restrict__ C, double *__restrict__ out, long long M, int ldz,
                                                  int J, int G, long long ldc) {
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= M) return;
  double acc = 0.0;
  for (int c = lane; c < 4 * J; c += 64) {
    const int jp = c >> 2, qp = c & 3;
    const double *gjp = gp_grid(gp, J, jp);
    double frp;
    const int cp = cell_of(Z[i * ldz + jp], gjp[0], gjp[2], G, frp);
    const double *col = C + (size_t)jp * G + cp + qp;
    double part = 0.0;
    for (int j = 0; j < J; ++j) {
      const double *gj = gp_grid(gp, J, j);
      double fr;
      const int cj = cell_of(Z[i * ldz + j], gj[0], gj[2], G, fr);
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fma(tap_w(fr, q), col[((size_t)j * G + cj + q) * ldc], part);
    }
    acc = fma(tap_w(frp, qp), part, acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) out[i] = acc;
}

struct GramLayout {
  int2 *cellrank;
  int *counts, *cellsum, *start, *perm;
  size_t counts_bytes, total;
};
inline GramLayout gram_layout(void *ws, int64_t N, int J, int G) {
  const size_t nchunk = (size_t)((N + kChunk - 1) / kChunk), ncell = (size_t)G - 3;
  GramLayout l;
  char *w = reinterpret_cast<char *>(ws);
  size_t off = 0;
  l.cellrank = reinterpret_cast<int2 *>(w + off); off += align256(sizeof(int2) * (size_t)J * (size_t)N);
  l.counts_bytes = sizeof(int) * (size_t)J * ncell * nchunk;
  l.counts = reinterpret_cast<int *>(w + off); off += align256(l.counts_bytes);
  l.cellsum = reinterpret_cast<int *>(w + off); off += align256(sizeof(int) * (size_t)J * ncell);
  l.start = reinterpret_cast<int *>(w + off); off += align256(sizeof(int) * (size_t)J * (ncell + 1));
  l.perm = reinterpret_cast<int *>(w + off); off += align256(sizeof(int) * (size_t)J * (size_t)N);
  l.total = off;
  return l;
}
inline bool gram_shape_ok(int64_t N, int J, int G, int T) {
  return N >= 1 && N <= INT_MAX && J >= 1 && J <= 65535 && G >= 8 && G <= kMaxG && T >= 0 && T <= kMaxT;
}

}  // namespace

extern "C" {

size_t rpgp_ski_gram_f64_workspace_bytes(int64_t N, int J, int G, int T) {
  if (!gram_shape_ok(N, J, G, T)) return 0;
  return gram_layout(nullptr, N, J, G).total;
}

int rpgp_ski_gram_f64(const double *Z, const double *grid_params, const double *Y, double *A, double *g, int64_t N, int ldz, int J,
                      int G, int T, void *workspace, size_t workspace_bytes, void *stream) {
  if (!gram_shape_ok(N, J, G, T) || !Z || !grid_params || !A || ldz < J || (T > 0 && (!Y || !g)) || !aligned(Z, 8) ||
      !aligned(grid_params, 8) || !aligned(Y, 8) || !aligned(A, 8) || !aligned(g, 8) || !aligned(workspace, 16))
    return RPGP_EINVAL;
  const GramLayout l = gram_layout(workspace, N, J, G);
  if (!workspace || workspace_bytes < l.total) return RPGP_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nchunk = (int)((N + kChunk - 1) / kChunk), ncell = G - 3;
  RPGP_CHECK(hipMemsetAsync(l.counts, 0, l.counts_bytes, st));
  hipLaunchKernelGGL(k_cell_rank, dim3(nchunk, J), dim3(kChunk), 0, st, Z, grid_params, l.cellrank, l.counts, (long long)N, ldz, J,
                     G, nchunk);
  hipLaunchKernelGGL(k_cell_scan, dim3((ncell + 3) / 4, J), dim3(256), 0, st, l.counts, l.cellsum, ncell, nchunk);
  hipLaunchKernelGGL(k_cell_start, dim3(J), dim3(1024), 0, st, l.cellsum, l.start, ncell, (int)N);
  hipLaunchKernelGGL(k_place, dim3(nchunk, J), dim3(256), 0, st, l.cellrank, l.counts, l.start, l.perm, (long long)N, ncell,
                     nchunk);
  // strip height S and projections per chunk Jc from the LDS budget: S Jc rows of GP doubles (padded by 4 when there is more
  // than one row, so that rows of one column start 4 doubles apart in the banks), at most 256 threads
  const int S = G <= 2044 ? 4 : (G <= 4092 ? 2 : 1);
  int GP = G + 4;
  int Jc = kLdsBytes / (S * GP * (int)sizeof(double));
  if (Jc < 1) Jc = 1, GP = G;                             // (S = 1 and G above 8188: one unpadded row)
  if (Jc > 64 / S) Jc = 64 / S;
  if (Jc > J) Jc = J;
  const int threads = ((4 * S * Jc + 63) / 64) * 64;
  const size_t lds = sizeof(double) * (size_t)S * Jc * GP;
  const dim3 grid((G + S - 1) / S, J, (J + Jc - 1) / Jc);
  if (S == 4)
    hipLaunchKernelGGL(k_gram<4>, grid, dim3(threads), lds, st, Z, grid_params, l.perm, l.start, A, (long long)N, ldz, J, G, Jc, GP);
  else if (S == 2)
    hipLaunchKernelGGL(k_gram<2>, grid, dim3(threads), lds, st, Z, grid_params, l.perm, l.start, A, (long long)N, ldz, J, G, Jc, GP);
  else
    hipLaunchKernelGGL(k_gram<1>, grid, dim3(threads), lds, st, Z, grid_params, l.perm, l.start, A, (long long)N, ldz, J, G, Jc, GP);
  if (J > 1) {
    const long long n = (long long)J * G;
    const unsigned nt = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_mirror, dim3(nt, nt), dim3(256), 0, st, A, G, n);
  }
  if (T > 0)
    hipLaunchKernelGGL(k_gram_rhs, dim3((G + 3) / 4, J), dim3(64), 0, st, Z, grid_params, l.perm, l.start, Y, g, (long long)N, ldz,
                       J, G, T);
  return launch_status();
}

int rpgp_ski_quadform_f64(const double *Z, const double *grid_params, const double *C, double *out, int64_t M, int ldz, int J,
                          int G, int64_t ldc, void *stream) {
  if (!Z || !grid_params || !C || !out || M < 1 || M > 4 * (int64_t)INT_MAX || J < 1 || J > 65535 || G < 8 || ldz < J ||
      ldc < (int64_t)J * G ||
      !aligned(Z, 8) || !aligned(grid_params, 8) || !aligned(C, 8) || !aligned(out, 8))
    return RPGP_EINVAL;
  hipLaunchKernelGGL(k_quadform, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), Z, grid_params,
                     C, out, (long long)M, ldz, J, G, (long long)ldc);
  return launch_status();
}

}  // extern "C"
