/*
 * rpgp.h — C-ABI of the MI355X-native additive randomly-projected GP kernel path.
 *
 * Drop-in boundary.  The reference (idelbrid/Randomly-Projected-Additive-GPs) is pure
 * Python on GPyTorch; it has no FFI of its own.  The entry points below are what a GPyTorch
 * `Kernel.forward` -> `LazyTensor` binding for this path would call; each one names the reference
 * interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM) unless a name ends in `_host`;
 *   - row-major, contiguous unless a leading dimension (`ld*`) is given;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *     allocates nothing, and is re-entrant (no global mutable state besides a one-time device probe);
 *   - return value: 0 on success, otherwise a hipError_t value or one of the RPGP_E* codes below;
 *     `rpgp_error_string` turns either into text.  Python callers raise RuntimeError / ValueError.
 *
 * Kernel definition:
 *   K[i,i'] = scale * sum_{j in [j0,j1)} exp(-0.5 * (Z1[i,j] - Z2[i',j])^2)
 *   with Z = (X / lengthscale) P  (prescale)  or  (X P) / lengthscale  (postscale);
 *   for the J20 specs scale = outputscale * (1/J).
 */
#ifndef RPGP_H
#define RPGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPGP_ABI_VERSION 4

#define RPGP_EINVAL     10001 /* bad argument (shape, range, null pointer) */
#define RPGP_EWORKSPACE 10002 /* workspace too small: call the matching *_workspace_bytes */
#define RPGP_ENODEVICE  10003 /* no gfx950 device visible */
#define RPGP_ENUMERIC   10004 /* NaNs encountered in an iterative solve */

/* ABI version of the loaded library. */
int rpgp_version(void);

/* Text for a return code of any function below (static storage). */
const char *rpgp_error_string(int code);

/* One-time probe of the current device (checks gfx9 wave64, finds the DPP rotate direction used by the
 * symmetric kernel).  Called lazily by the compute entry points; exposed so hosts can fail early. */
int rpgp_init(void);

/*
 * DPA-GP diversification of the projection directions (replaces the gradient loop of rp.space_equally, rp.py:241-266, for
 * d < J): `niter` plain gradient steps of size `lr` on sum_{a != b} cos^4(angle(P_a, P_b)), then row normalisation, in
 * ONE single-workgroup launch.  P: J x d row-major DEVICE array, updated in place (J, d <= 64); final_loss (DEVICE, 1
 * float, may be NULL) receives the energy before the normalisation, as the reference returns it.
 */
int rpgp_space_equally(float *P, int J, int d, float lr, int niter, float *final_loss, void *stream);

/*
 * Projection  Z = X @ Peff   (X: N x d, Peff: d x J, Z: N x J).
 * Replaces gp_models/kernels/scaled_projection_kernel.py:21-27 (`x1.div(lengthscale)` + `projection_module(x1)`);
 * the caller folds the ARD lengthscale into Peff (prescale: diag(1/l) P; postscale: P diag(1/l)).
 */
int rpgp_project(const float *X, const float *Peff, float *Z, int64_t N, int d, int J, void *stream);

/*
 * Backward of the projection w.r.t. Peff:  dPeff = X^T @ G  (G: N x J, dPeff: d x J).
 * Replaces autograd through scaled_projection_kernel.py:21-27 for the lengthscale / learn_proj gradients.
 */
int rpgp_project_grad(const float *X, const float *G, float *dPeff, int64_t N, int d, int J, void *stream);

/*
 * Symmetric fused MVM:  out = scale * sum_{j in [j0,j1)} K_j(Z,Z) @ V  +  noise * V      (V, out: N x T)
 * K is never stored; each unordered pair (i,i') is evaluated once.
 * Replaces the dense `K @ V` inside gpytorch.utils.linear_cg reached from fitting/optimizing.py:67-71
 * (kernel built at training_routines.py:148-159,169-171,406 and evaluated by scaled_projection_kernel.py:37).
 * `ldz` = row stride of Z in floats (>= j1).  Results are deterministic (no float atomics).
 */
size_t rpgp_mvm_sym_workspace_bytes(int64_t N, int T);
int rpgp_mvm_sym(const float *Z, const float *V, float *out, int64_t N, int ldz, int T,
                 int j0, int j1, float scale, float noise,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Prepared (factorised) fast path for repeated symmetric MVMs with the same Z (every CG iteration of one
 * hyper-parameter step).  exp(-(a-b)^2/2) is evaluated as exp2(-a'^2) * exp2(2a'b' - b'^2) on centred, pre-scaled
 * coordinates: 3 VALU issues per pair-term instead of 4.  `rpgp_prepare` centres each projection at the midpoint of its
 * range, writes the packed row/column tables into `prep` and records whether the exponent range is safe
 * (max a'^2 < 100); `rpgp_prepare_status` copies that verdict to the host (synchronises the stream once).  Only call
 * `rpgp_mvm_sym_prepared` when fast_ok == 1 — otherwise it fills `out` with NaN — and use rpgp_mvm_sym (exact direct
 * form, any range) instead.  Same result contract, workspace and determinism as rpgp_mvm_sym; relative error per
 * kernel entry <= ~1e-7 * (1 + a'^2).   J <= 64.
 */
size_t rpgp_prepare_bytes(int64_t N, int J);
int rpgp_prepare(const float *Z, int64_t N, int ldz, int J, void *prep, size_t prep_bytes, void *stream);
int rpgp_prepare_status(const void *prep, int *fast_ok_host, float *max_abs_host, void *stream);
int rpgp_mvm_sym_prepared(const void *prep, const float *V, float *out, int64_t N, int J, int T,
                          int j0, int j1, float scale, float noise,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Pair-sharding of the symmetric MVM across ranks (multi-GPU).  The (row block, column chunk) workgroups of the tile
 * decomposition are numbered row block by row block; rank r of `world` executes the contiguous range
 * [total*r/world, total*(r+1)/world) (the chunk size is chosen for the per-rank share, so every rank still launches a
 * few thousand workgroups of equal size).  Each rank therefore evaluates ALL J projections on 1/world of the (i,i')
 * pairs at the full per-term efficiency and produces a partial N x T output (row AND transposed contributions);
 * the partials are summed with one all-reduce — the same message as J-sharding (`MultiDeviceKernel` counterpart,
 * training_routines.py:407-408) without the per-pair overhead of thin J-slices.  Pass the noise on exactly ONE rank
 * (its slab reduce adds noise*V for every row) and 0 on the others.  world = 1, rank = 0 is the plain call.  Workspace: rpgp_mvm_sym_range_workspace_bytes.
 */
size_t rpgp_mvm_sym_range_workspace_bytes(int64_t N, int T, int world, int rank);
int rpgp_mvm_sym_range(const float *Z, const float *V, float *out, int64_t N, int ldz, int T, int j0, int j1,
                       int world, int rank, float scale, float noise,
                       void *workspace, size_t workspace_bytes, void *stream);
int rpgp_mvm_sym_prepared_range(const void *prep, const float *V, float *out, int64_t N, int J, int T,
                                int j0, int j1, int world, int rank, float scale, float noise,
                                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Chebyshev low-rank form of the prepared symmetric MVM.  On the centred coordinates of rpgp_prepare every 1-D term is
 * exp2(-h^2 (x - y)^2) with x = a'/h, y = b'/h in [-1, 1] (h = max_abs of rpgp_prepare_status), which is numerically low-rank:
 * K_j ~ T(x_j) C T(x_j)^T with the p x p Chebyshev coefficients C of that function.  The product then costs ~4 N J p FMAs
 * and no exponentials.  p is the smallest rank whose discarded coefficient tail sum_{max(m,n) >= p} |c_mn| (a bound on the
 * error of every kernel entry, since |T_m| <= 1) is <= 2^-26; results differ from the sweep at the 1e-7 level, not only in
 * summation order.
 *   rpgp_lowrank_select (host only, no device): the rank for a half-width h, 0 when it exceeds p_max (<= 128) or the reference
 *     degree 128 does not resolve the function; `tail_host` (optional) receives the claimed bound, `coef_host` (optional,
 *     p_max x p_max row-major) the p x p float64 coefficients.
 *   rpgp_lowrank_create: plan of one prepared buffer (call after rpgp_prepare, once per Z) in the caller's device buffer of
 *     rpgp_lowrank_plan_bytes; *p_host = 0 and *handle_host = NULL when the range needs more than 64 (not served: use
 *     rpgp_mvm_sym_prepared_range).  Synchronises the stream.  The handle is host memory: rpgp_lowrank_destroy frees it (the
 *     device buffer stays the caller's).
 *   rpgp_mvm_sym_lowrank_range: same arguments and result contract as rpgp_mvm_sym_prepared_range plus the handle; a rank of
 *     (world, rank) writes its row slice [N r / world, N (r + 1) / world) of scale * K v and noise * V on every row; repeated
 *     calls are bit-identical.  Workspace: rpgp_mvm_sym_lowrank_workspace_bytes.
 */
int rpgp_lowrank_select(double h, int p_max, int *p_host, double *tail_host, double *coef_host);
size_t rpgp_lowrank_plan_bytes(int64_t N, int J);
int rpgp_lowrank_create(const void *prep, int64_t N, int J, float max_abs, void *plan, size_t plan_bytes, int *p_host,
                        void **handle_host, void *stream);
int rpgp_lowrank_destroy(void *handle);
size_t rpgp_mvm_sym_lowrank_workspace_bytes(const void *handle, int64_t N, int T);
int rpgp_mvm_sym_lowrank_range(const void *handle, const void *prep, const float *V, float *out, int64_t N, int J, int T,
                               int j0, int j1, int world, int rank, float scale, float noise,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Training tolerance and the low-rank bilinear derivative (same plan).
 *   rpgp_lowrank_create_tol: rpgp_lowrank_create with the per-entry tail tolerance min(tol, 2^-26) (tol > 0).  A tail eps per
 *     entry moves the operator by ||K~ - K||_2 <= N scale J eps, so a solve on scale K + sigma^2 I asks for
 *     tol = 1e-3 sigma^2 / (scale J N) as well.
 *   rpgp_lowrank_grad_select (host only, like rpgp_lowrank_select): the rank q of the antisymmetric Chebyshev coefficients D of
 *     G(x, y) = -2 ln2 kappa h (x - y) exp2(-h^2 (x - y)^2)  (kappa = (2 ln 2)^-1/2), i.e. -(z - z') e(z, z') in z units:
 *     the smallest q whose discarded tail sum_{max(m,n) >= q} |d_mn| is <= min(tol, 2^-26); 0 above q_max (<= 128).
 *     `coef_host` (optional, q_max x q_max row-major) receives D.
 *   rpgp_lowrank_grad_prepare: chooses q for the plan's h and stores D and the plan's own coefficients C (both float64) in the
 *     caller's device buffer of RPGP_LOWRANK_GRAD_BYTES (rpgp_lowrank_grad_bytes(handle) for a plan of rpgp_lowrank_create_cap,
 *     below), which must outlive the handle's derivative calls.  *q_host = 0 (no derivative rank) when q > 64 (the plan's cap)
 *     or the plan has rank 1.  Synchronises the stream.  A later call replaces the rank.
 *   rpgp_bilinear_grad_lowrank: rpgp_bilinear_grad's result contract (gZ for the columns [j0, j1) only — the others are not
 *     touched —, gscale) on the plan's Z, any T, computed from the product form in four launches with float64 reductions in a
 *     fixed order: repeated calls are bit-identical.  RPGP_EINVAL when the handle has no derivative rank.  Workspace:
 *     rpgp_bilinear_grad_lowrank_workspace_bytes (0 without a derivative rank).
 */
#define RPGP_LOWRANK_GRAD_BYTES 65536
int rpgp_lowrank_create_tol(const void *prep, int64_t N, int J, float max_abs, double tol, void *plan, size_t plan_bytes,
                            int *p_host, void **handle_host, void *stream);
int rpgp_lowrank_grad_select(double h, int q_max, double tol, int *q_host, double *tail_host, double *coef_host);
int rpgp_lowrank_grad_prepare(void *handle, double tol, void *dcoef, size_t dcoef_bytes, int *q_host, void *stream);
size_t rpgp_bilinear_grad_lowrank_workspace_bytes(const void *handle, int64_t N, int T);
int rpgp_bilinear_grad_lowrank(const void *handle, const float *L, const float *R, float *gZ, float *gscale, int64_t N,
                               int ldg, int T, int j0, int j1, float scale, void *workspace, size_t workspace_bytes,
                               void *stream);

/*
 * The same product and derivative with per-component weights: K = scale sum_j w_j K_j, the RBF, group-1 members of rpgp_family
 * (below) on the plan of rpgp_lowrank_create[_tol] for the prepared buffer of the family operator's Z.  `weights`: DEVICE,
 * J floats, of any sign (the product is linear in them); w = 1 returns the bits of the unweighted entries.  Unsharded.
 *   rpgp_mvm_sym_lowrank_weighted: out = scale sum_{j in [j0, j1)} w_j K_j V + noise V; the weight enters the combine pass
 *     (U_j = (float)((double)scale (double)w_j C W_j)), the other two passes are rpgp_mvm_sym_lowrank_range's.  Repeated calls
 *     are bit-identical.  Workspace: rpgp_mvm_sym_lowrank_workspace_bytes.
 *   rpgp_bilinear_grad_lowrank_weighted: rpgp_family_bilinear_grad's result contract (below) on the plan's Z (N x J, leading
 *     dimension J): gZ[i][j] = scale w_j sum_i' S_ii' dk_j/dz_i for j in [j0, j1) and gcomp[j] = 0.5 sum_ii' S_ii' k_j(i, i'),
 *     the UNWEIGHTED component sums (float64, fixed order, no atomics); columns and components outside [j0, j1) are not touched.
 *     RPGP_EINVAL, with the outputs untouched, when the handle has no derivative rank.  Workspace:
 *     rpgp_bilinear_grad_lowrank_workspace_bytes.
 */
int rpgp_mvm_sym_lowrank_weighted(const void *handle, const void *prep, const float *weights, const float *V, float *out,
                                  int64_t N, int J, int T, int j0, int j1, float scale, float noise,
                                  void *workspace, size_t workspace_bytes, void *stream);
int rpgp_bilinear_grad_lowrank_weighted(const void *handle, const float *weights, const float *L, const float *R, float *gZ,
                                        float *gcomp, int64_t N, int J, int T, int j0, int j1, float scale,
                                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Plans with a rank cap of the caller's, up to 128 (half-widths up to about 14, where the reference degree 128 stops resolving
 * the function).  The creators above size their buffers for rank 64 and keep doing so; a plan made here remembers its cap, and
 * every entry that takes a handle — rpgp_mvm_sym_lowrank_range, rpgp_mvm_sym_lowrank_weighted, rpgp_lowrank_grad_prepare,
 * rpgp_bilinear_grad_lowrank[_weighted], the two *_workspace_bytes, rpgp_mbcg_workspace_bytes and the executor's
 * RPGP_OP_LOWRANK / RPGP_OP_LOWRANK_FAMILY — serves its padded ranks 8 ... 128 with the contracts stated above.  Padded ranks
 * above 64 run kernels of their own (the projection in two rank slices per row block, float64 Clenshaw sums in both output
 * passes); a plan whose p and q are <= 64 runs the kernels, and returns the bits, of a plan of rpgp_lowrank_create_tol.
 *   rpgp_lowrank_plan_bytes_cap: size of the plan buffer for the cap p_max (1 ... 128; 0 outside, or for N, J outside
 *     rpgp_lowrank_plan_bytes' limits).  p_max <= 64: rpgp_lowrank_plan_bytes(N, J).
 *   rpgp_lowrank_create_cap: rpgp_lowrank_create_tol with the cap p_max: *p_host = 0 and *handle_host = NULL when the range
 *     needs more than p_max.  RPGP_EINVAL for p_max outside 1 ... 128.  Like the other creators it does not read the prepared
 *     header's fast_ok (that guards the factorised sweep's exp2 range; this form reads the centred coordinates only) and
 *     serves any finite max_abs the reference degree resolves; a non-finite max_abs is not served.  The coordinates themselves
 *     are the caller's to vouch for: rpgp_prepare's max_abs skips a NaN of Z (its fast_ok is then 0), so a caller that serves
 *     buffers that are not fast_ok checks the prepared coordinates for NaN first, as ops.LowrankTrainPlan does.
 *   rpgp_lowrank_grad_bytes: size of rpgp_lowrank_grad_prepare's buffer for this handle: RPGP_LOWRANK_GRAD_BYTES for a plan of
 *     rpgp_lowrank_create[_tol] or a cap <= 64, D and C (float64) at the padded cap above; 0 for a NULL handle.
 *     rpgp_lowrank_grad_prepare requires that many bytes and selects q up to the plan's cap.
 */
size_t rpgp_lowrank_plan_bytes_cap(int64_t N, int J, int p_max);
int rpgp_lowrank_create_cap(const void *prep, int64_t N, int J, float max_abs, double tol, int p_max, void *plan,
                            size_t plan_bytes, int *p_host, void **handle_host, void *stream);
size_t rpgp_lowrank_grad_bytes(const void *handle);

/*
 * Panel plans: any half-width at the per-row work of a rank <= 64 plan.  [-h, h] is cut into P equal panels of half-width
 * hp = h / P (centres c_k = -h + (2k + 1) hp, local coordinate x = (a - c_k) / hp).  Two points of one panel interact through
 * C0 (rpgp_lowrank_select's form at hp), a point of panel k with one of panel k + 1 through C1, the coefficients of
 * exp2(-hp^2 (x - y - 2)^2) (x in the lower panel; the opposite order is C1^T), and points two or more panels apart are dropped:
 * they are at least 2 hp apart.  D0, D1 and -D1^T are the same for the derivative.  The per-entry bound of the product is the
 * largest of the tail of C0, the tail of C1 and the largest dropped value exp2(-4 hp^2) (0 for P = 2, which drops nothing); the
 * derivative's is built the same way from D0, D1 and (2 hp / kappa) exp2(-4 hp^2).
 *   rpgp_lowrank_panels_select (host only, no device): the smallest P in 2 ... rpgp_lowrank_panels_max() (16: half-widths up to
 *     about 100) — or, for panels > 0, that count alone — for which the four ranks are <= 64 and all six bounds are <=
 *     min(tol, 2^-26).  *panels_host = 0: none.  p = the larger rank of C0 and C1, q of D0 and D1; bounds_host[3] / dbounds_host[3]
 *     (optional) = {tail of the same-panel form, tail of the neighbour form, dropped} at those ranks; coef_host (optional):
 *     [C0][C1][D0][D1], 64 x 64 doubles each, zero outside p x p / q x q.  RPGP_EINVAL for panels = 1 or outside 0 ... 16.
 *   rpgp_lowrank_panels_plan_bytes: size of the plan buffer for any panel count (0 for N, J outside the limits).
 *   rpgp_lowrank_create_panels: the plan of that selection at h = max_abs (1 + 2^-20), once per Z after rpgp_prepare, into the
 *     caller's buffer; *panels_host = *p_host = 0 and *handle_host = NULL when it is not served.  The plan holds C0, C1 (fp32), the
 *     local coordinate and the panel of every (column, row) in natural order, and for every column the rows in panel order: a
 *     stable counting sort whose positions are prefix sums (a function of Z alone), every (column, panel) segment padded to whole
 *     projection blocks of 2 048 slots (a padded slot contributes v = 0), with the first block of every panel per column.  A
 *     coordinate at +h belongs to the last panel, one exactly on an inner edge to the upper panel.  Like rpgp_lowrank_create_cap
 *     it does not read fast_ok, and the caller vouches for coordinates without a NaN.  rpgp_lowrank_destroy frees the handle.
 *   rpgp_lowrank_panels_info: P (0: a single-interval plan), hp, p, q and the product's three bounds of a handle.
 * Every entry that takes a handle serves a panel plan with the contract stated above: rpgp_mvm_sym_lowrank_range,
 * rpgp_mvm_sym_lowrank_weighted, rpgp_bilinear_grad_lowrank[_weighted], the two *_workspace_bytes, rpgp_lowrank_grad_bytes
 * (D0, D1 and the float64 C0, C1: 128 KiB), rpgp_lowrank_grad_prepare (the derivative is selected with the plan, at the plan's
 * tolerance: *q_host = 0 for a smaller `tol`), rpgp_mbcg_workspace_bytes and the executor's RPGP_OP_LOWRANK /
 * RPGP_OP_LOWRANK_FAMILY.  No float atomics; repeated calls are bit-identical; a NULL weight pointer and weights of 1 give the
 * same bits.
 */
int rpgp_lowrank_panels_select(double h, double tol, int panels, int *panels_host, double *hp_host, int *p_host, int *q_host,
                               double *bounds_host, double *dbounds_host, double *coef_host);
int rpgp_lowrank_panels_max(void);
size_t rpgp_lowrank_panels_plan_bytes(int64_t N, int J);
int rpgp_lowrank_create_panels(const void *prep, int64_t N, int J, float max_abs, double tol, int panels, void *plan,
                               size_t plan_bytes, int *panels_host, int *p_host, void **handle_host, void *stream);
int rpgp_lowrank_panels_info(const void *handle, int *panels_host, double *hp_host, int *p_host, int *q_host,
                             double *bounds_host);

/*
 * Explicit features of the truncated kernel (the closed-form posterior of the low-rank form).  Factor C ~= G G^T (G: p x r), so
 * that every 1-D term is exp2(-h^2 (x - y)^2) ~= (G^T T(x))^T (G^T T(y)) and the kernel is K_lr = B B^T with
 * B = sqrt(scale) [T(x_1) G | ... | T(x_J) G]  (N x J r).
 *   rpgp_lowrank_post_select (host only, no device): p = the rank of rpgp_lowrank_select at the per-entry tolerance `tol` (p_max
 *     <= 128), C = the p x p coefficients, factored by a symmetric eigensolver in double (cyclic Jacobi for p <= 64, Householder
 *     tridiagonalisation with implicit QL above); the smallest eigenpairs (every negative one first) are dropped while p * sum |dropped eigenvalues| <= tol.  G = Q_r Lambda_r^1/2 goes row-major into
 *     `G_host` (optional, p_max x p_max, row m at m * p_max); *tail_host (optional) = the selection's tail + the dropped bound
 *     (max of p * sum |dropped|, sum_mn |C - G G^T|_mn): it bounds |T(x)^T G G^T T(y) - exp2(-h^2 (x - y)^2)| on [-1, 1]^2.
 *     *p_host = *r_host = 0: not served (h not finite, not resolved by the reference degree, or p > p_max).  Deterministic.
 *   rpgp_lowrank_features_f64: B[i ldb + j r + k] = sqrt_scale * sum_{m < p} T_m(x_ij) G[m r + k] with
 *     x_ij = (Z[i ldz + j] - mid[j]) * inv_w; Z (N x ldz), mid (J), G (p x r, compact row-major) and B are float64 device
 *     arrays.  The recurrence and the products run in float64 in a fixed order (repeated calls are bit-identical); the
 *     columns [J r, ldb) of B are not written.  Limits: N >= 1, 1 <= J <= 64, ldz >= J, 1 <= r <= p <= 128, ldb >= J r.
 */
int rpgp_lowrank_post_select(double h, double tol, int p_max, int *p_host, int *r_host, double *tail_host, double *G_host);
int rpgp_lowrank_features_f64(const double *Z, int64_t N, int J, int ldz, const double *mid, double inv_w, const double *G,
                              int p, int r, double sqrt_scale, double *B, int64_t ldb, void *stream);

/*
 * The adjoint of rpgp_lowrank_features_f64 (the closed-form marginal likelihood's derivative through the features).  With
 * W = ca alpha v^T + cy Y (N x J r; formed row by row, never stored) and x_ij = (Z[i ldz + j] - mid[j]) * inv_w:
 *   rpgp_lowrank_features_grad_f64: gZ[i ldg + j] = sqrt_scale * inv_w * sum_{m < p} T_m(x_ij) sum_{k < r} Gd[m r + k] W[i, j r + k]
 *     Gd (p x r, compact row-major) are the derivative coefficients of the features' G: sum_m T'_m(x) G[m r + k] =
 *     sum_m T_m(x) Gd[m r + k] (the host's Chebyshev derivative recurrence), so gZ = dL/dZ for dL/dB = W.  Z (N x ldz), mid (J),
 *     Y (N x ldy), alpha (N), v (J r) and gZ are float64 device arrays.  Float64 throughout, in a fixed order, without atomics:
 *     each (i, j) is written once and repeated calls are bit-identical; the columns [J, ldg) of gZ are not written.
 *     Limits: N >= 1, 1 <= J <= 64, ldz >= J, 1 <= r <= p <= 128, ldy >= J r, ldg >= J.
 */
int rpgp_lowrank_features_grad_f64(const double *Z, int64_t N, int J, int ldz, const double *mid, double inv_w,
                                   const double *Gd, int p, int r, double sqrt_scale, const double *Y, int64_t ldy,
                                   const double *alpha, const double *v, double ca, double cy, double *gZ, int64_t ldg,
                                   void *stream);

/*
 * The same two kernels for a LIST of columns of Z under one form and with a factor per column (kernels with one lengthscale and
 * one weight per projection: the columns are served in classes, each with its own inv_w, G, p and r).  For c < nc, j = cols[c]
 * and x_ic = (Z[i ldz + j] - mid[c]) * inv_w:
 *   rpgp_lowrank_features_cols_f64: B[i ldb + c r + k] = col_scale[c] * sum_{m < p} T_m(x_ic) G[m r + k];
 *   rpgp_lowrank_features_grad_cols_f64: gZ[i ldg + cols[c]] = col_scale[c] * inv_w * sum_{m < p} T_m(x_ic) sum_{k < r}
 *     Gd[m r + k] W[i, c r + k],  W = ca alpha v^T + cy Y on the nc r columns of this form.
 * cols (int32), mid and col_scale (float64) are device arrays of length nc; cols holds distinct indices in [0, ldz) in any order
 * (the caller's contract: they are not read on the host).  B, Y and v point at the form's first feature column, so the kernels
 * see a dense nc r block: the columns of B outside [0, nc r) and the columns of gZ that are not listed are not touched.  The
 * adjoint's factor is the double product col_scale[c] * inv_w; with cols = 0 ... J - 1, ldz = J and col_scale = sqrt_scale both
 * return the bits of rpgp_lowrank_features_f64 / rpgp_lowrank_features_grad_f64.  Float64 throughout, fixed order, no atomics:
 * repeated calls are bit-identical.  Limits: N >= 1, 1 <= nc <= 64, 1 <= r <= p <= 128, ldb, ldy >= nc r, ldz, ldg >= nc (and
 * > max(cols)).
 */
int rpgp_lowrank_features_cols_f64(const double *Z, int64_t N, int nc, int ldz, const int32_t *cols, const double *mid,
                                   double inv_w, const double *G, int p, int r, const double *col_scale, double *B, int64_t ldb,
                                   void *stream);
int rpgp_lowrank_features_grad_cols_f64(const double *Z, int64_t N, int nc, int ldz, const int32_t *cols, const double *mid,
                                        double inv_w, const double *Gd, int p, int r, const double *col_scale, const double *Y,
                                        int64_t ldy, const double *alpha, const double *v, double ca, double cy, double *gZ,
                                        int64_t ldg, void *stream);

/*
 * Rectangular fused MVM:  out = scale * sum_j K_j(Z1,Z2) @ V      (Z1: M x ., Z2: N x ., V: N x T, out: M x T)
 * Replaces K(X*,X) @ alpha and K(X,X*) blocks of the prediction strategy driven from training_routines.py:551-575.
 */
size_t rpgp_mvm_rect_workspace_bytes(int64_t M, int64_t N, int T);
int rpgp_mvm_rect(const float *Z1, const float *Z2, const float *V, float *out,
                  int64_t M, int64_t N, int ldz1, int ldz2, int T,
                  int j0, int j1, float scale,
                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Dense block  out[m, n] = scale * sum_j exp(-0.5 (Z1[m,j]-Z2[n,j])^2)   (out: M x N, row stride ldo).
 * Used for pivoted-Cholesky rows, `evaluate()`/`to_dense()` at small N and the cached-K mode.
 * Replaces LazyEvaluatedKernelTensor.evaluate_kernel()/_getitem on the kernel of training_routines.py:169-171.
 */
int rpgp_dense(const float *Z1, const float *Z2, float *out, int64_t M, int64_t N,
               int ldz1, int ldz2, int64_t ldo, int j0, int j1, float scale, void *stream);

/*
 * Bilinear derivative for backward, symmetric operator:
 *   S = L R^T + R L^T            (L, R: N x T)
 *   gZ[i,j]  = -scale * sum_i' S[i,i'] e_j(i,i') (Z[i,j]-Z[i',j])     for j in [j0,j1)   (gZ: N x ldg)
 *   gscale   = 0.5 * sum_{i,i'} S[i,i'] sum_j e_j(i,i')               (1 float, device)
 * i.e. d/dZ and d/dscale of  sum_{ii'} (L R^T)[i,i'] K[i,i'].
 * Replaces LazyTensor._quad_form_derivative triggered by loss.backward() at fitting/optimizing.py:72.
 */
size_t rpgp_bilinear_grad_workspace_bytes(int64_t N, int J);
int rpgp_bilinear_grad(const float *Z, const float *L, const float *R, float *gZ, float *gscale,
                       int64_t N, int ldz, int ldg, int T, int j0, int j1, float scale,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Same derivative with an explicit symmetric weight matrix S (N x N, row stride lds):
 *   gZ[i,j] = -scale * sum_i' S[i,i'] e_j(i,i') (Z[i,j]-Z[i',j]) ;  gscale = 0.5 * sum_{ii'} S[i,i'] sum_j e_j(i,i')
 * i.e. d/dZ, d/dscale of 0.5 * sum(S * K).  Used by the dense Cholesky regime (N <= max_cholesky_size, or
 * `--use_chol`, gp_experiment_runner.py:236,326) where S = Khat^-1 - alpha alpha^T is formed exactly.
 * Workspace: rpgp_bilinear_grad_workspace_bytes.
 */
int rpgp_bilinear_grad_dense(const float *Z, const float *S, float *gZ, float *gscale,
                             int64_t N, int ldz, int ldg, int64_t lds, int j0, int j1, float scale,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Rank-`rank` pivoted Cholesky of K(Z,Z) (greedy max-diagonal pivots): L (N x rank, row-major) with K ~= L L^T, for the
 * Woodbury preconditioner M = L L^T + sigma^2 I (GPyTorch `pivoted_cholesky`, max_preconditioner_size = 15,
 * SURVEY.md Appendix B.3).  One single-workgroup launch for N <= 2048, otherwise rank + 1 chip-wide launches (one per
 * greedy step; pivots identical: ties go to the smallest index).  `diag_work` is N + RPGP_PIVCHOL_SCRATCH floats of
 * device scratch.  J, rank <= 64.  The family variant takes weight_sum = sum_c weights[c] (the kernel's diagonal is
 * scale * weight_sum).
 */
#define RPGP_PIVCHOL_SCRATCH 8192
int rpgp_pivoted_cholesky(const float *Z, float *L, float *diag_work, int64_t N, int ldz, int J, int rank,
                          float scale, void *stream);

/*
 * Dense-matrix MVM for the cached-K mode:  out = Kd @ V + noise * V   (Kd: N x N fp32 in HBM, row stride ldk).
 * HBM-bound stream of Kd with the thin GEMM on the matrix cores (v_mfma_f32_16x16x4_f32) — SURVEY.md §8(f) rank 2.
 */
int rpgp_dense_mvm(const float *Kd, const float *V, float *out, int64_t N, int64_t ldk, int T,
                   float noise, void *stream);

/*
 * Packed symmetric cache of the additive kernel (cached-K mode without the lower triangle): every unordered pair of
 * points is evaluated once (`rpgp_symcache_build`, the fused symmetric sweep with a store in place of the products) and
 * kept in the order that sweep consumes it; `rpgp_symcache_mvm` is the same sweep with a 16-byte load in place of the J
 * exponentials: out = scale * (sum_j K_j) V + noise * V from HALF the bytes of the dense N x N matrix.  Same role as
 * rpgp_dense + rpgp_dense_mvm (the matrix GPyTorch's lazily evaluated kernel materialises for `_matmul`,
 * training_routines.py:406 with fitting/optimizing.py:69-71) for blocks of up to 12 right-hand sides per pass; wider
 * blocks take ceil(T / 12) passes over the cache — use the dense matrix for those.
 * The cached values are the unscaled sums over j in [j0, j1) in fp32, so an outputscale change needs no rebuild.
 * (world, rank): pair-sharding as in rpgp_mvm_sym_range — the cache holds this rank's share of the pairs only and the
 * product is a partial result (noise on ONE rank); world = 1, rank = 0 is the whole matrix.  The layout depends on
 * (N, world, rank) only; a cache is valid for exactly the arguments it was built with.
 * `layout` (the same value for the build and every product on that cache; size and workspace do not depend on it):
 *   RPGP_SYMCACHE_THIN — rotation order of the fused sweep; products of 1..4 right-hand sides are HBM-bound on the
 *                        N^2/2 stored values (VALU passes of up to 12 columns for wider blocks);
 *   RPGP_SYMCACHE_WIDE — 16 x 16 tiles in v_mfma_f32_16x16x4_f32 operand order; blocks of up to 16 right-hand sides per
 *                        pass on the matrix cores (the training block of 10 probes + the residual).
 */
#define RPGP_SYMCACHE_THIN 0
#define RPGP_SYMCACHE_WIDE 1
size_t rpgp_symcache_bytes(int64_t N, int world, int rank);
size_t rpgp_symcache_workspace_bytes(int64_t N, int T, int world, int rank);
int rpgp_symcache_build(const float *Z, void *cache, size_t cache_bytes, int64_t N, int ldz, int j0, int j1, int layout,
                        int world, int rank, void *stream);
int rpgp_symcache_mvm(const void *cache, size_t cache_bytes, int layout, const float *V, float *out, int64_t N, int T,
                      float scale, float noise, int world, int rank, void *workspace, size_t workspace_bytes,
                      void *stream);

/*
 * SKI path (1-D grid interpolation per projection; replaces the `GridInterpolationKernel` wrap of
 * training_routines.py:157-158 used by model_specs/additive_spread_prescale_Jd_ski.json):
 *   K ~= scale * sum_j W_j Tm W_j^T,   W_j = cubic-convolution (Keys) interpolation weights of projection j onto ONE
 *   shared regular grid of G points,  Tm[m,m'] = exp(-0.5 ((m-m') h)^2)  (symmetric Toeplitz).
 * rpgp_ski_grid       : grid_params (device: g0, h, 1/h, has_weights = 0) from the min/max of Z1 (and Z2 if given) so that
 *                       all points lie in [g_2, g_{G-3}]  (h = range / (G-5)).  The block may be 4 + J floats long: a caller
 *                       that sets has_weights = 1 and appends w_0 .. w_{J-1} gets K ~= scale * sum_j w_j W_j Tm W_j^T
 *                       from every SKI entry point (the `weighted` components of polynomial_projection_kernels.py:88-98).
 * rpgp_ski_mvm        : out = scale * sum_j W1_j Tm W2_j^T V (+ noise V when Z1 == Z2)    (out: M x T, V: N x T).
 *                       scatter (per-(chunk, projection) fixed-point LDS histograms + slabs for T <= 12: bitwise
 *                       reproducible; float atomics for wider blocks), Toeplitz product (MFMA), gather.
 *                       HBM traffic ~ 4 (N (J + T) + M (J + T)) bytes.
 * rpgp_ski_diag       : diag[i] = scale * sum_j w_i^T Tm[4x4] w_i.
 * rpgp_ski_bilinear_grad : d/dZ and d/dscale of sum((L R^T) * K) for the square operator (T <= 12); `row_scratch`
 *                       is N floats of device scratch.
 * All need `rpgp_ski_workspace_bytes(J, G, T)` bytes of workspace; G*13*4 <= 64 KB (G <= 1260).
 */
size_t rpgp_ski_workspace_bytes(int J, int G, int T);
int rpgp_ski_grid(const float *Z1, int64_t N1, int ld1, const float *Z2, int64_t N2, int ld2, int J, int G,
                  float *grid_params, void *workspace, size_t workspace_bytes, void *stream);
/* The reference's grid rule (polynomial_projection_kernels.py:54-63; the `rp_poly` / `strictly_additive` / `additive` kinds
 * with `ski: true`): every projection gets ITS OWN grid — spacing_j = (max_j - min_j) / (G - 4), bounds
 * [min_j - 2.01 spacing_j, max_j + 2.01 spacing_j], G points spanning the bounds.  grid_params: 4 + 4 J floats,
 * [., ., ., flags = 2, w_0 .. w_{J-1} = 1, (g0_j, h_j, 1/h_j) x J]; set flags = 3 and fill the w_j for per-projection output
 * scales.  Every SKI entry point reads either block form.  (With fixed projections the reference's static bounds,
 * computed once from X, scale with 1/lengthscale_j exactly like the current projected coordinates do, so recomputing the
 * bounds from the current Z reproduces them.) */
int rpgp_ski_grid_per_projection(const float *Z1, int64_t N1, int ld1, const float *Z2, int64_t N2, int ld2, int J, int G,
                                 float *grid_params, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_ski_mvm(const float *Z1, const float *Z2, const float *grid_params, const float *V, float *out,
                 int64_t M, int64_t N, int ldz1, int ldz2, int J, int G, int T, float scale, float noise,
                 void *workspace, size_t workspace_bytes, void *stream);
/*
 * The three stages of rpgp_ski_mvm as separate calls (T <= 12), for the row-sharded multi-GPU SKI operator that replaces
 * `MultiDeviceKernel` around the SKI kernel (training_routines.py:407-408 with :157-158): every rank scatters ITS rows,
 * the J x G x T float64 histogram is all-reduced (RCCL), the Toeplitz product is replicated and every rank gathers ITS
 * rows.  grid_params must be built from the GLOBAL coordinate range (same block on every rank).
 *   rpgp_ski_scatter      : hist[j][g][t] (float64, J*G*T) = sum_i w(z_ij)[g] V[i][t] over the N local rows
 *   rpgp_ski_grid_product : H[j][m][t] (float32) = w_j * sum_m' Tm[m,m'] hist[j][m'][t]
 *   rpgp_ski_gather       : out[i][t] = scale * sum_j sum_k w_k(z_ij) H[j][idx0+k][t] + noise * V[i][t]  (V may be NULL if noise == 0)
 */
int rpgp_ski_scatter(const float *Z, const float *grid_params, const float *V, double *hist, int64_t N, int ldz, int J,
                     int G, int T, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_ski_grid_product(const double *hist, const float *grid_params, float *H, int J, int G, int T, void *stream);
int rpgp_ski_gather(const float *Z, const float *grid_params, const float *H, const float *V, float *out, int64_t M,
                    int ldz, int J, int G, int T, float scale, float noise, void *stream);
/*
 * Planned SKI product for the square operator (Z fixed over a whole CG solve = one hyper-parameter step): rpgp_ski_plan
 * sorts every projection's points by the grid cell of their first tap ONCE (stable radix sort: deterministic order) and
 * keeps the tap fractions in that order; the scatter of every later product is then a segmented reduction over the sorted
 * points — no atomics — and the Toeplitz stage reads its first column from the plan.
 *   rpgp_ski_mvm_planned     : same result contract as rpgp_ski_mvm(Z, Z, ...) for T <= 12 (bitwise reproducible)
 *   rpgp_ski_scatter_planned : stage 1 only (the row-sharded operator: plan built on the LOCAL rows), = rpgp_ski_scatter
 *   rpgp_ski_gather_fast     : stage 3; with J * G * T floats fitting in LDS (and >= 32 768 rows) the table H is LDS-resident,
 *                              else = rpgp_ski_gather (`plan` may be NULL: the gather reads the coordinates themselves)
 * Workspace of the products: rpgp_ski_workspace_bytes(J, G, T) (RPGP_EWORKSPACE when the per-cell tap records of J * G cells
 * exceed its scratch — more than ~340 projections: fall back to rpgp_ski_mvm).  N * J < 2^31.
 */
size_t rpgp_ski_plan_bytes(int64_t N, int J, int G);
size_t rpgp_ski_plan_workspace_bytes(int64_t N, int J, int G);
int rpgp_ski_plan(const float *Z, const float *grid_params, int64_t N, int ldz, int J, int G, void *plan, size_t plan_bytes,
                  void *workspace, size_t workspace_bytes, void *stream);
int rpgp_ski_mvm_planned(const void *plan, const float *Z, const float *grid_params, const float *V, float *out, int64_t N,
                         int ldz, int J, int G, int T, float scale, float noise, void *workspace, size_t workspace_bytes,
                         void *stream);
int rpgp_ski_scatter_planned(const void *plan, const float *V, double *hist, int64_t N, int J, int G, int T, void *workspace,
                             size_t workspace_bytes, void *stream);
int rpgp_ski_gather_fast(const void *plan, const float *Z, const float *grid_params, const float *H, const float *V, float *out,
                         int64_t M, int ldz, int J, int G, int T, float scale, float noise, void *stream);
/* Pivoted Cholesky of the SKI operator (same contract as rpgp_pivoted_cholesky).  diag_work: DEVICE scratch of
 * rpgp_ski_pivoted_cholesky_work_floats(N, rank) floats — the residual diagonal, the argmax partials and, from N = 65 536 on,
 * the factor in column-major order while it is built (step m then reads m coalesced vectors instead of every line of the
 * N x rank array); RPGP_EWORKSPACE if smaller. */
size_t rpgp_ski_pivoted_cholesky_work_floats(int64_t N, int rank);
int rpgp_ski_pivoted_cholesky(const float *Z, const float *grid_params, float *L, float *diag_work, size_t diag_work_floats,
                              int64_t N, int ldz,
                              int J, int G, int rank, float scale, void *stream);
int rpgp_ski_diag(const float *Z, const float *grid_params, float *diag, int64_t N, int ldz, int J, int G,
                  float scale, void *stream);
/* Dense block K_ski(Z1, Z2) (M x N, row stride ldo) straight from the interpolation weights and the Toeplitz lags (J <= 64). */
int rpgp_ski_dense(const float *Z1, const float *Z2, const float *grid_params, float *out, int64_t M, int64_t N,
                   int ldz1, int ldz2, int64_t ldo, int J, int G, float scale, void *stream);
int rpgp_ski_bilinear_grad(const float *Z, const float *grid_params, const float *L, const float *R, float *gZ,
                           float *gscale, int64_t N, int ldz, int ldg, int J, int G, int T, float scale,
                           void *workspace, size_t workspace_bytes, float *row_scratch, void *stream);
/* Same with per-projection output scales in the grid parameter block (see rpgp_ski_grid): additionally gcomp[j] (DEVICE,
 * J floats) = the part of gscale contributed by projection j (it carries w_j; divide by w_j for the unweighted component
 * sum); row_scratch: N * (J + 1) floats. */
int rpgp_ski_bilinear_grad_comp(const float *Z, const float *grid_params, const float *L, const float *R, float *gZ,
                                float *gscale, float *gcomp, int64_t N, int ldz, int ldg, int J, int G, int T,
                                float scale, void *workspace, size_t workspace_bytes, float *row_scratch,
                                void *stream);

/*
 * float64 parity kernels of the SKI operator (csrc/rpgp_ski_f64.hip): `--double` (/root/reference/training_routines.py:481) for
 * the `ski: true` specifications (/root/reference/training_routines.py:157-158).  Same operator and grid-parameter layout as the
 * float32 entry points above, every array float64 (grid_params included: [g0, h, 1/h, flags, w_j .., (g0_j, h_j, 1/h_j) ..]);
 * a thread per output element, the scatter with float64 hardware atomics (sums differ in the last bits between runs), the
 * Toeplitz stage a plain O(G^2) sum — written for clarity, not speed.  Any T (the host passes <= 64 columns per call).
 *   rpgp_ski_f64_mvm           out (M x T) = scale sum_j w_j W1_j Tm_j W2_j^T V (+ noise V: square operator only)
 *   rpgp_ski_f64_diag / _dense the diagonal / a dense block K_ski(Z1, Z2)
 *   rpgp_ski_f64_bilinear_grad d/dZ, d/dscale (device scalar) and (gcomp != NULL, J doubles) the per-projection parts of d/dscale
 *                              (each carries its w_j) of sum((L R^T) * K_ski(Z, Z))
 */
size_t rpgp_ski_f64_workspace_bytes(int J, int G, int T);
int rpgp_ski_f64_mvm(const double *Z1, const double *Z2, const double *grid_params, const double *V, double *out, int64_t M,
                     int64_t N, int ldz1, int ldz2, int J, int G, int T, double scale, double noise, void *workspace,
                     size_t workspace_bytes, void *stream);
int rpgp_ski_f64_diag(const double *Z, const double *grid_params, double *diag, int64_t N, int ldz, int J, int G, double scale,
                      void *stream);
int rpgp_ski_f64_dense(const double *Z1, const double *Z2, const double *grid_params, double *out, int64_t M, int64_t N, int ldz1,
                       int ldz2, int64_t ldo, int J, int G, double scale, void *stream);
int rpgp_ski_f64_bilinear_grad(const double *Z, const double *grid_params, const double *L, const double *R, double *gZ,
                               double *gscale, double *gcomp, int64_t N, int ldz, int ldg, int J, int G, int T, double scale,
                               void *workspace, size_t workspace_bytes, void *stream);
/* The stages of the float64 product and derivative as separate calls — `--double` for the row-sharded operator (one process per
 * GPU: MultiDeviceKernel around the grid-interpolation kernel, /root/reference/training_routines.py:407-408 with :157-158, under
 * :481): scatter the LOCAL rows into columns [hoff, hoff + T) of a J x G x HT float64 histogram (zero_first: clear it), all-reduce
 * it (caller), replicated grid product, gather the local rows; the derivative from the all-reduced J x G x 2T block
 * [W^T L | W^T R].  rpgp_ski_f64_bilinear_finish workspace: J * G * 2T + J doubles (+ 512 B). */
int rpgp_ski_f64_scatter(const double *Z, const double *grid_params, const double *V, double *hist, int64_t N, int ldz, int J,
                         int G, int T, int HT, int hoff, int zero_first, void *stream);
int rpgp_ski_f64_grid_product(const double *hist, const double *grid_params, double *H, int J, int G, int T, int weighted,
                              void *stream);
int rpgp_ski_f64_gather(const double *Z, const double *grid_params, const double *H, const double *V, double *out, int64_t M,
                        int ldz, int J, int G, int T, double scale, double noise, void *stream);
int rpgp_ski_f64_bilinear_finish(const double *Z, const double *grid_params, const double *hist2, const double *L, const double *R,
                                 double *gZ, double *gscale, double *gcomp, int64_t N, int ldz, int ldg, int J, int G, int T,
                                 double scale, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The two passes over the rows of the closed-form posterior of the grid-interpolation models (csrc/rpgp_ski_post.hip;
 * ski_posterior.py).  w_i: the 4 J cubic-convolution weights of row i of Z (N x J, leading dimension ldz) placed
 * in a vector of J G entries, by the stencil rule of every SKI entry point (grid coordinate clipped to [1, G - 2], first tap in
 * [0, G - 4]).  Every array float64; grid_params: the float64 grid block above (both grid rules and the weights flag parse; the
 * weights and the kind do not enter).  No float atomics, every sum in a fixed order: a repeated call is bit-identical.
 *   rpgp_ski_gram_f64      A (J G x J G, row-major, both triangles, A == A^T bitwise) = sum_i w_i w_i^T and g (J G x T, row-major)
 *                          = sum_i w_i Y_i^T for Y (N x T, row-major), 0 <= T <= 16; Y and g may be NULL when T == 0.  Workspace:
 *                          rpgp_ski_gram_f64_workspace_bytes(N, J, G, T) (0 for a shape that is not served), 16-byte aligned;
 *                          RPGP_EWORKSPACE if smaller.  RPGP_EINVAL: N outside 1 ... 2^31 - 1, J outside 1 ... 65535, G outside
 *                          8 ... 8192, T outside 0 ... 16, ldz < J, a null or misaligned pointer.
 *   rpgp_ski_quadform_f64  out[i] = w_i^T C w_i for the M rows of Z; C: J G x J G with leading dimension ldc >= J G, BOTH
 *                          triangles are read (the plain double sum over the 4 J x 4 J taps, nothing doubled).  RPGP_EINVAL:
 *                          M < 1, J outside 1 ... 65535, G < 8, ldz < J, ldc < J G, a null or misaligned pointer.
 */
size_t rpgp_ski_gram_f64_workspace_bytes(int64_t N, int J, int G, int T);
int rpgp_ski_gram_f64(const double *Z, const double *grid_params, const double *Y, double *A, double *g, int64_t N, int ldz, int J,
                      int G, int T, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_ski_quadform_f64(const double *Z, const double *grid_params, const double *C, double *out, int64_t M, int ldz, int J,
                          int G, int64_t ldc, void *stream);

/*
 * The derivative in two stages for the row-sharded SKI operator (MLL backward of a model whose rows are split over ranks):
 *   rpgp_ski_bilinear_scatter : hist2[j][g][0..T) = W_j^T L, hist2[j][g][T..2T) = W_j^T R over the N LOCAL rows (float64,
 *                               J * G * 2T) — all-reduce it over the ranks —
 *   rpgp_ski_bilinear_finish  : Toeplitz products of the 2T columns, then gZ (local rows), gscale and (gcomp != NULL:
 *                               row_scratch N * (J + 1) floats) gcomp as PARTIAL sums over the local rows (all-reduce them).
 * T <= 12; rpgp_ski_bilinear_grad[_comp] is exactly scatter + finish.
 */
int rpgp_ski_bilinear_scatter(const float *Z, const float *grid_params, const float *L, const float *R, double *hist2,
                              int64_t N, int ldz, int J, int G, int T, void *workspace, size_t workspace_bytes,
                              void *stream);
/* stage 1 with the points of Z taken from its plan (rpgp_ski_plan): two cell-sorted scatters, no atomics */
int rpgp_ski_bilinear_scatter_planned(const void *plan, const float *L, const float *R, double *hist2, int64_t N, int J, int G,
                                      int T, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_ski_bilinear_finish(const float *Z, const float *grid_params, const double *hist2, const float *L, const float *R,
                             float *gZ, float *gscale, float *gcomp, int64_t N, int ldz, int ldg, int J, int G, int T,
                             float scale, void *workspace, size_t workspace_bytes, float *row_scratch, void *stream);

/*
 * Generalised additive family — the other members behind the same operator:
 *     K[i,i'] = scale * sum_{c < ncomp} weights[c] * phi_kind( columns [c*group, (c+1)*group) of Z )
 *   kind RBF      exp(-r^2/2), r^2 summed over the group's columns   (k > 1 sub-kernels of training_routines.py:172-174,
 *                 the product groups of polynomial_projection_kernels.py:70-86; group in {1,2,3,4,5,8,10,20})
 *   kind MATERN15 (1 + sqrt3 r) exp(-sqrt3 r)     kind IMQ  (1 + r^2)^(-1/2)     kind COSINE  cos(pi r)
 *                 (`kernel_type` of training_routines.py:47-88, imq_kernel.py:8-9; group must be 1)
 * `weights` (DEVICE, ncomp floats, required) are the per-component output scales (the `weighted` ScaleKernels of
 * polynomial_projection_kernels.py:88-98; all 1/J for additive_rp).  Z holds ncomp*group columns, already divided by
 * the lengthscales.  Same tile / dense kernels as the hot path with a different kernel-function policy; no factorised
 * fast path; float64 and the combinations not instantiated here: rpgp_family_generic_* below.
 * rpgp_family_bilinear_grad*: gZ as rpgp_bilinear_grad; gcomp[c] (DEVICE, ncomp) = 0.5 sum_ii' S_ii' phi_c(i,i'), the
 * unweighted per-component sums (d/d weights[c] = scale * gcomp[c]; d/d scale = sum_c weights[c] gcomp[c]).
 */
#define RPGP_KIND_RBF 0
#define RPGP_KIND_MATERN15 1
#define RPGP_KIND_IMQ 2
#define RPGP_KIND_COSINE 3
/* OR-ed into the `kind` of the rpgp_family_generic_* calls only: a group is the PRODUCT of `group` 1-D sub-kernels
 * (the ProductKernel groups of polynomial_projection_kernels.py:70-86) instead of one radial group-dimensional sub-kernel
 * (training_routines.py:172-174).  The two are the same function for the RBF. */
#define RPGP_KIND_PRODUCT 16
typedef struct rpgp_family {
  int kind, group, ncomp;
  const float *weights;
} rpgp_family;
size_t rpgp_family_mvm_workspace_bytes(int64_t M, int64_t N, int T, int sym);
int rpgp_family_mvm_sym(const rpgp_family *fam, const float *Z, const float *V, float *out, int64_t N, int ldz, int T,
                        float scale, float noise, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_family_mvm_rect(const rpgp_family *fam, const float *Z1, const float *Z2, const float *V, float *out,
                         int64_t M, int64_t N, int ldz1, int ldz2, int T, float scale, void *workspace,
                         size_t workspace_bytes, void *stream);
int rpgp_family_dense(const rpgp_family *fam, const float *Z1, const float *Z2, float *out, int64_t M, int64_t N,
                      int ldz1, int ldz2, int64_t ldo, float scale, void *stream);
size_t rpgp_family_bilinear_grad_workspace_bytes(int64_t N, int ncols, int ncomp);
int rpgp_family_bilinear_grad(const rpgp_family *fam, const float *Z, const float *L, const float *R, float *gZ,
                              float *gcomp, int64_t N, int ldz, int ldg, int T, float scale, void *workspace,
                              size_t workspace_bytes, void *stream);
int rpgp_family_bilinear_grad_dense(const rpgp_family *fam, const float *Z, const float *S, float *gZ, float *gcomp,
                                    int64_t N, int ldz, int ldg, int64_t lds, float scale, void *workspace,
                                    size_t workspace_bytes, void *stream);
int rpgp_family_pivoted_cholesky(const rpgp_family *fam, const float *Z, float *L, float *diag_work, int64_t N,
                                 int ldz, int rank, float scale, float weight_sum, void *stream);

/* The same family with RUNTIME (kind, group) in float32 or float64 (csrc/rpgp_family_generic.hip) — what the templated
 * kernels above do not instantiate: `--double` (training_routines.py:481) for every member, k > 1 sub-kernels of the
 * non-RBF types in the RADIAL form `additive_rp` builds (training_routines.py:172-174: kernel(active_dims = a group of k
 * columns); imq_kernel.py:8-9) or, with `kind | RPGP_KIND_PRODUCT`, in the PRODUCT-of-1-D form of the rp_poly kinds
 * (polynomial_projection_kernels.py:70-86), any group size <= 32 (ncomp * group <= 64).  `dtype`: RPGP_F32 / RPGP_F64 selects the element
 * type of EVERY pointer argument (weights, Z, V, L, R, S, outputs).  Parity path: lane-owns-row, library transcendental
 * functions, one writer per output (bitwise reproducible).
 *   mvm:      out (M x T) = scale * K(Z1, Z2) V (+ noise V when Z2 == NULL: the symmetric operator on Z1, M == N); T <= 16
 *   dense:    out (M x N, leading dimension ldo) = scale * K(Z1, Z2)
 *   bilinear: gZ / gcomp exactly as rpgp_family_bilinear_grad (S == NULL: weights S = L R^T + R L^T from the N x T factors)
 *             or rpgp_family_bilinear_grad_dense (S: explicit symmetric N x N matrix, leading dimension lds).
 */
int rpgp_family_generic_mvm(int dtype, int kind, int group, int ncomp, const void *weights, const void *Z1, const void *Z2,
                            const void *V, void *out, int64_t M, int64_t N, int ldz1, int ldz2, int T, double scale,
                            double noise, void *stream);
int rpgp_family_generic_dense(int dtype, int kind, int group, int ncomp, const void *weights, const void *Z1, const void *Z2,
                              void *out, int64_t M, int64_t N, int ldz1, int ldz2, int64_t ldo, double scale, void *stream);
size_t rpgp_family_generic_bilinear_workspace_bytes(int dtype, int64_t N, int ncomp);
int rpgp_family_generic_bilinear(int dtype, int kind, int group, int ncomp, const void *weights, const void *Z, const void *L,
                                 const void *R, const void *S, void *gZ, void *gcomp, int64_t N, int ldz, int ldg, int T,
                                 int64_t lds, double scale, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Full (non-additive) radial kernels, matrix-free (csrc/rpgp_radial.hip): the family's single component of group = d,
 *     K[i,i'] = scale * phi_kind(|a_i - b_i'|^2),   a, b = rows of Z1 (M x d), Z2 (N x d), already centred and divided by the
 * lengthscales, `kind` an RPGP_KIND_* value, 1 <= d <= 1024 (the reference's UCI sets reach d = 385).  float32.  The squared
 * distance is the Gram form d2 = max(|a|^2 + |b|^2 - 2 a.b, 0) with a.b an exact-fp32 FMA chain on v_mfma_f32_16x16x4_f32
 * (operands staged through LDS in feature chunks; row norms once per launch); phi runs on the VALU.  One writer per output
 * element, fixed summation order, no atomics: repeated calls are bit-identical.
 * Numerics (u = 2^-24): |delta d2_ij| <= (d + 4) u (|a_i| + |b_j|)^2 for any summation order, so
 *     |delta K_ij| <= scale (C_phi (d + 4) u (|a_i| + |b_j|)^2 + c u (1 + d2 |phi'(d2)|)),
 * C_phi = max |phi'| = 0.5 (RBF), 1.5 (Matern), 0.5 (InverseMQ), pi^2 / 2 (Cosine).  The error grows with the NORMS of the
 * rows, not with their distance: the caller subtracts one common centre from Z1 and Z2 (the kernel is translation-invariant).
 * The derivative's a_i r_i - (M A)_i cancels for near-duplicate rows; its relative error in norm is ~3e-7 at lengthscales of
 * sqrt(d) and up to ~5e-3 where K is close to the identity and the gradient itself is negligible.
 *   rpgp_radial_mvm            out (M x T) = scale K(Z1, Z2) V; Z2 == NULL: the symmetric operator on Z1 (M == N) with
 *                              + noise V, d2 forced to 0 on the diagonal so that the diagonal entry is exactly
 *                              scale phi(0) + noise.  V is N x T, out M x T, both contiguous; T <= 16.  Few rows: the columns
 *                              are split over workgroups and summed in split order.
 *   rpgp_radial_dense          out (M x N, leading dimension ldo) = scale K(Z1, Z2); Z1 == Z2 (same pointer, M == N): exact
 *                              diagonal as above.
 *   rpgp_radial_bilinear_grad  the convention of rpgp_family_bilinear_grad for one component: gZ[i][m] (N x d, leading
 *                              dimension ldg) = 2 scale sum_j S_ij phi'(d2_ij) (a_im - a_jm), gscale[0] (DEVICE) = 0.5 sum S o phi
 *                              (no factor `scale`).  S == NULL: S = L R^T + R L^T from the N x T factors (contiguous, T <= 16);
 *                              otherwise S is an explicit symmetric N x N matrix with leading dimension lds (L, R, T ignored).
 * Workspace of all three: rpgp_radial_workspace_bytes(M, N, T) (the derivative: M = N; dense and derivative: any T), 16-byte
 * aligned; RPGP_EWORKSPACE if smaller.  RPGP_EINVAL: d outside 1 ... 1024, T outside 1 ... 16, an unknown kind, a null or
 * misaligned pointer, a leading dimension smaller than the row length.
 */
size_t rpgp_radial_workspace_bytes(int64_t M, int64_t N, int T);
int rpgp_radial_mvm(int kind, const float *Z1, const float *Z2, const float *V, float *out, int64_t M, int64_t N, int d,
                    int ldz1, int ldz2, int T, float scale, float noise, void *workspace, size_t workspace_bytes,
                    void *stream);
int rpgp_radial_dense(int kind, const float *Z1, const float *Z2, float *out, int64_t M, int64_t N, int d, int ldz1, int ldz2,
                      int64_t ldo, float scale, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_radial_bilinear_grad(int kind, const float *Z, const float *L, const float *R, const float *S, float *gZ,
                              float *gscale, int64_t N, int d, int ldz, int ldg, int T, int64_t lds, float scale,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Inducing-point (SGPR) sums over the training rows (csrc/rpgp_inducing.hip).  Z (N x d, leading dimension ldz) and U (M x d,
 * ldu) are float32, centred and divided by the lengthscales; Y is N x T float32, contiguous.  k_i = phi_kind(|z_i - u_.|^2) is
 * the float32 entry of the radial kernels above (same Gram-form distance, same entry bound, no scale).  Every output is float64,
 * row-major and contiguous.  1 <= d <= 1024, 1 <= M <= 1024, 0 <= T <= 16 (T == 0: Y, g, v may be NULL), any RPGP_KIND_*.
 *   rpgp_inducing_gram   G[M x M] = sum_i k_i k_i^T (both triangles), g[M x T] = sum_i k_i Y_i^T.  Products of two float32
 *                        values are exact in float64; the sums are float64 on v_mfma_f64_16x16x4_f64.
 *   rpgp_inducing_grad   for C (M x M float64, symmetric) and v (M x T float64), i.e. for the function
 *                        f = sum(C o G) + sum(v o g):  W = 2 K C + Y v^T,  S = W o phi'(d2)  (K C in float64 with C as given),
 *                            gU[M x d] = 2 sum_i S_ij (u_j - z_i)               = df / dU
 *                            q[d]      = sum_ij S_ij (z_im - u_jm)^2            (df / d l_m = -(2 / l_m) q_m)
 *                        S is rounded to float32 once per entry; every sum over the rows is float64.
 * The rows are walked in slabs: nothing N-sized is held or written.  The slab length is taken from the workspace handed in:
 * rpgp_inducing_workspace_bytes(M, d, T, rows) is the size for slabs of `rows` rows (rounded up to 64); any size from
 * rows = 64 up is accepted and more bytes mean longer slabs; RPGP_EWORKSPACE if smaller.  The size does not depend on N.
 * Fixed summation order for one slab length, no atomics: repeated calls are bit-identical.  RPGP_EINVAL as above.
 */
size_t rpgp_inducing_workspace_bytes(int64_t M, int d, int T, int64_t rows);
int rpgp_inducing_gram(int kind, const float *Z, const float *U, const float *Y, double *G, double *g, int64_t N, int64_t M,
                       int d, int ldz, int ldu, int T, void *workspace, size_t workspace_bytes, void *stream);
int rpgp_inducing_grad(int kind, const float *Z, const float *U, const float *Y, const double *C, const double *v, double *gU,
                       double *q, int64_t N, int64_t M, int d, int ldz, int ldu, int T, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * Native mBCG executor (replaces gpytorch.utils.linear_cg as configured at gp_experiment_runner.py:324-329; algorithm in
 * SURVEY.md Appendix B.2).  Solves (A) X = rhs for T <= 16 right-hand sides with A described by `rpgp_operator`
 * (noise included), optional Woodbury preconditioner M = L L^T + sigma2 I given as L (N x k, k <= 16) and
 * Cinv = (sigma2 I + L^T L)^-1 (k x k, FLOAT64: the capacitance system is ill-conditioned).  Right-hand-side columns are normalised internally; the loop stops when the mean
 * column residual norm < tolerance after >= min_iter iterations (tested every `check_every` iterations — the only host
 * synchronisations) or at max_iter.  The first `hist_len` (<= 64) iterations' alpha / beta coefficients are returned in
 * HOST arrays laid out [hist_len][16] for the Lanczos tridiagonals.  Returns RPGP_ENUMERIC on NaNs.
 * stagnation_window > 0: also stop (without convergence: *mean_resid_host stays >= tolerance) when the best mean
 * residual has not improved by 1 % over that many consecutive tests — the fp32 floor of a badly conditioned system.
 */
#define RPGP_OP_FUSED 0           /* rpgp_mvm_sym on Z */
#define RPGP_OP_FUSED_PREPARED 1  /* rpgp_mvm_sym_prepared on prep */
#define RPGP_OP_SKI 2             /* rpgp_ski_mvm on Z + grid_params; prep != NULL: an rpgp_ski_plan of Z (planned product) */
#define RPGP_OP_DENSE 3           /* cached-K: symmetric Kd (N x N, row stride ldk) in HBM, applied by rpgp_dense_mvm */
#define RPGP_OP_FAMILY 4          /* rpgp_family_mvm_sym on Z + family */
#define RPGP_OP_SYMCACHE 5        /* packed symmetric cache: Kd = the cache, ldk = its size in bytes, G = its layout; scale, noise */
#define RPGP_OP_SUM 6             /* sum of G unsharded operators on the same N rows: prep -> rpgp_operator[G] in HOST memory (each
                                     part with its own scale / noise; no nesting) — the additive kernels whose multiplicative
                                     groups differ in size (general_rp_poly, training_routines.py:192-207) */
#define RPGP_OP_LOWRANK 7         /* Chebyshev low-rank product (rpgp_mvm_sym_lowrank_range): prep = the plan HANDLE of
                                     rpgp_lowrank_create[_tol]; N, J, j0, j1, scale, noise as for FUSED_PREPARED; unsharded only */
#define RPGP_OP_LOWRANK_FAMILY 8  /* the same with per-component weights (rpgp_mvm_sym_lowrank_weighted): prep = the plan HANDLE,
                                     family = an RBF, group-1 family with ncomp == J (its device weights); any other family is
                                     RPGP_EINVAL; N, J, j0, j1, scale, noise as for RPGP_OP_LOWRANK; unsharded only */
#define RPGP_OP_RADIAL 9          /* rpgp_radial_mvm on Z (N x J, leading dimension ldz): J = d input columns, family->kind =
                                     the RPGP_KIND_* value (group, ncomp, weights unused); scale, noise; unsharded only */
typedef struct rpgp_operator {
  int kind;
  int64_t N;
  int J, ldz, j0, j1, G;
  float scale, noise;
  const float *Z;
  const void *prep;
  const float *grid_params;
  const float *Kd;
  int64_t ldk;
  const rpgp_family *family;
  int world, rank;              /* pair-shard of RPGP_OP_FUSED / FUSED_PREPARED / SYMCACHE (0 or 1, 0: the whole operator) */
} rpgp_operator;

/*
 * Sharded solves (one process per GPU).  `fn(ctx, buf, count, dtype, stream)` is the in-place SUM all-reduce described
 * under "Multi-GPU pieces" below; the executor calls it between its enqueue-only phases on the launch stream, so a
 * sharded solve still has no host synchronisation per iteration (the convergence flag stays on the device).
 *   RPGP_SHARD_PARTIAL  vectors are replicated; the operator (RPGP_OP_FUSED / FUSED_PREPARED with (world, rank) or a
 *                       [j0, j1) slice, RPGP_OP_SYMCACHE with (world, rank)) yields this rank's partial product, the noise
 *                       term is added on rank 0 only, ONE all-reduce of the N x T block per iteration;
 *   RPGP_SHARD_ROWS     RPGP_OP_SKI on this rank's rows (op->N local rows, T <= 12; rhs / x / L are the local rows; op->N
 *                       may be 0): the J x G x T float64 histogram and two 288-double reduction vectors per iteration are
 *                       all-reduced; global_N = total number of rows (iteration cap).  grid_params must come from the
 *                       GLOBAL coordinate range and Cinv from the all-reduced capacitance matrix.
 * reducer == NULL, mode RPGP_SHARD_NONE or fn == NULL: the single-GPU solve.
 */
#define RPGP_SHARD_NONE 0
#define RPGP_SHARD_PARTIAL 1
#define RPGP_SHARD_ROWS 2
typedef int (*rpgp_allreduce_fn)(void *ctx, void *buf, size_t count, int dtype, void *stream);
typedef struct rpgp_reducer {
  int mode, world, rank;
  int64_t global_N;
  rpgp_allreduce_fn fn;
  void *ctx;
} rpgp_reducer;
/* (The hipGraph form of the iteration loop — SURVEY.md §8(f) rank 3 — was built in round 5, measured 6 - 17 % slower than the
 *  queue-ahead executor and is parked as tools/experiments/r6_removed_forms.patch; ABI 3 no longer exports its switch.) */
size_t rpgp_mbcg_workspace_bytes(const rpgp_operator *op, int T, int precond_rank);
int rpgp_mbcg_solve(const rpgp_operator *op, const float *rhs, float *x, int T, int max_iter, int min_iter,
                    int hist_len, int check_every, int stagnation_window, float tolerance, int precond_rank,
                    const float *L,
                    const double *Cinv, float precond_sigma2, const rpgp_reducer *reducer, float *alpha_hist_host,
                    float *beta_hist_host, int *iterations_host, float *mean_resid_host, void *workspace,
                    size_t workspace_bytes, void *stream);

/*
 * Stochastic Lanczos quadrature estimate of log|A| from the CG coefficient histories rpgp_mbcg_solve returns (HOST
 * arithmetic, no device work): the first `num_probes` columns of alpha_hist / beta_hist ([iters][ld] floats) are unit-norm
 * probe columns;  log|A| ~ (n / num_probes) sum_p sum_m Q_p[0][m]^2 log lambda_pm  over the Lanczos tridiagonals
 * T[k][k] = 1/alpha_k + beta_{k-1}/alpha_{k-1}, T[k][k+1] = sqrt(beta_k)/alpha_k.  Replaces what GPyTorch's
 * `inv_quad_logdet` does with the `t_mat` of `linear_cg` (lanczos_tridiag_to_diag + the log-det sum), reached from
 * `-mll(output, train_y)` at /root/reference/fitting/optimizing.py:67-72.  RPGP_ENUMERIC: the QL iteration did not converge.
 */
int rpgp_slq_logdet(const float *alpha_hist, const float *beta_hist, int iters, int ld, int num_probes, double n,
                    double *logdet_out);

/*
 * The small kernels AROUND the solve of one optimiser step of the flagship model (csrc/rpgp_step.hip): each call is one launch
 * for a stretch the reference runs as a chain of element-wise torch launches on d + 3 scalars and a few
 * N x 11 blocks — `-mll(model(train_x), train_y)` / `loss.backward()` at /root/reference/fitting/optimizing.py:67-72 on the model
 * of /root/reference/training_routines.py:131-189, 325-410.  All enqueue on `stream`; only rpgp_step_hyper waits (for three floats).
 *
 * rpgp_step_hyper: raw parameters -> outputscale = softplus(raw_os), noise = softplus(raw_noise) + min_noise, ls = softplus(raw_ls)
 *   (n_ls = 1, or d with `prescale`, or J), Peff[d x J] = P / ls with P = W^T (W: the J x d weight of the frozen Linear
 *   projection).  dev_out (device, 8 + 2 n_ls floats): [0] outputscale [1] noise [2] mean [3] sigmoid(raw_os) [4] sigmoid(raw_noise)
 *   [8..) ls, then sigmoid(raw_ls).  The three scalars the other entry points take BY VALUE come back through pinned memory
 *   (the call spins until the kernel has published them): *outputscale_host, *noise_host, *mean_host.
 * rpgp_step_probes: z = L e1 + sqrt_noise e2 (L: N x k, e1: k x p, e2: N x p standard normal draws — GPyTorch's preconditioner-
 *   distributed probe vectors), full_rhs[N x (p + 1)] = [z | y - *mean_dev].  p <= 16, k <= 64.  The probes are not normalised:
 *   rpgp_mbcg_solve normalises every column itself and returns Khat^-1 of the columns as given.
 * rpgp_step_value: inv_quad = sum_i full_rhs[i][col] solves[i][col] (N x T blocks);  out2[0] = (inv_quad + logdet) c1 + c2,
 *   out2[1] = inv_quad.  The workspace's first 4 bytes are an arrival counter: ZERO on entry (zero the buffer once), zero
 *   again on exit; it must not be shared between streams.  `ticket_out` (optional): the kernel also POSTS out2[0] to pinned
 *   host memory and *ticket_out names the slot (-1: none); rpgp_step_value_wait(ticket, &v) returns that value on the calling
 *   thread as soon as the kernel has run — the training loop's per-step `loss.item()` (fitting/optimizing.py:76) without
 *   waiting for the derivative and the optimiser update queued behind it.  RPGP_EINVAL: the ticket is older than 16 posts, from
 *   another thread, or the value has not arrived within 2 s (read out2[0] the ordinary way then).
 * rpgp_step_lr: the two sides of the bilinear derivative from the solve of [probes | r] (solves: N x (p + 1)):
 *   left = [solves_c gq / p | -gq alpha], right = [pre_probes (row stride ldp) | alpha], gq = g[0] * gscale (g: device scalar, the
 *   incoming gradient); partials[2 b], partials[2 b + 1] = workgroup b's sum(left * right), sum(alpha); *nparts_out workgroups.
 * rpgp_step_hyper_backward: dPeff (d x J, gradient w.r.t. Peff, to be scaled by zfac) -> gradients of the raw parameters:
 *   g_raw_ls = -sum(dPeff P) / ls^2 sigmoid(raw_ls) (per row / column / overall), g_raw_os = gs_scale gs[0] sigmoid(raw_os),
 *   g_raw_noise = (sum partials[2 b] + g[0] dlp_over_n) sigmoid(raw_noise), g_mean = -2 gq sum partials[2 b + 1].
 */
int rpgp_step_hyper(const float *raw_ls, int n_ls, const float *raw_os, const float *raw_noise, const float *mean,
                    const float *W, int d, int J, int prescale, float min_noise, float *Peff, float *dev_out,
                    float *outputscale_host, float *noise_host, float *mean_host, void *stream);
int rpgp_step_probes(const float *L, int k, const float *e1, const float *e2, float sqrt_noise, const float *y,
                     const float *mean_dev, int64_t N, int p, float *full_rhs, void *stream);
size_t rpgp_step_value_workspace_bytes(void);
int rpgp_step_value(const float *full_rhs, const float *solves, int64_t N, int T, int col, double logdet, double c1, double c2,
                    float *out2, void *workspace, size_t workspace_bytes, int *ticket_out, void *stream);
int rpgp_step_value_wait(int ticket, float *value_host);
size_t rpgp_step_lr_workspace_bytes(void);
int rpgp_step_lr(const float *solves, const float *pre_probes, int64_t ldp, const float *g, float gscale, int64_t N, int p,
                 float *left, float *right, float *partials, int *nparts_out, void *stream);
int rpgp_step_hyper_backward(const float *dPeff, const float *W, int d, int J, int n_ls, int prescale, float zfac,
                             const float *hyper_dev, const float *gs, const float *partials, int nparts, const float *g,
                             float gscale, float dlp_over_n, float gs_scale, float *g_raw_ls, float *g_raw_os,
                             float *g_raw_noise, float *g_mean, void *stream);

/*
 * Multi-GPU pieces (one process per GPU; replaces `MultiDeviceKernel(kernel, devices, devices[0])`,
 * training_routines.py:407-408).
 *
 * rpgp_allreduce_fn: in-place SUM all-reduce of `count` elements (dtype RPGP_F32 / RPGP_F64) of the DEVICE buffer
 * `buf` over the ranks, ENQUEUED on `stream` (no host synchronisation); every rank must end with bit-identical
 * values.  The host binds it to its communicator: `rpgp_comm_allreduce` below (ctx = the rpgp_comm), or a callback
 * that issues the RCCL collective on the same stream (torch.distributed.all_reduce in the Python host).
 *
 * rpgp_comm: SUM all-reduce over IPC-mapped peer buffers for the small, latency-bound messages of the sharded solve
 * (N x T partial products, J x G x T grid histograms, inner products).  One kernel launch per call: every rank publishes
 * its data in a staging buffer that all peers have mapped (hipIpcGetMemHandle / hipIpcOpenMemHandle), raises a flag in
 * each peer's memory, waits for the peers' flags and adds the W contributions in rank order (one-shot), or reduces its
 * own 1/W chunk and writes it to all peers (two-shot, messages > 512 KB).  Bootstrap: every rank calls
 * rpgp_comm_create, the RPGP_COMM_HANDLE_BYTES handles are exchanged out of band in rank order (the Python host uses
 * torch.distributed.all_gather_object), then rpgp_comm_connect.  A message may hold at most `max_bytes` bytes.
 * Waits are bounded (20 s): a lost peer raises the comm's error word (rpgp_comm_error) instead of hanging the GPU.
 */
#define RPGP_F32 0
#define RPGP_F64 1
#define RPGP_COMM_HANDLE_BYTES 64
typedef struct rpgp_comm rpgp_comm;
int rpgp_comm_create(int world, int rank, size_t max_bytes, rpgp_comm **out, void *handle_out);
int rpgp_comm_connect(rpgp_comm *comm, const void *all_handles);
size_t rpgp_comm_capacity(const rpgp_comm *comm);
int rpgp_comm_allreduce(void *comm, void *buf, size_t count, int dtype, void *stream);
int rpgp_comm_error(rpgp_comm *comm, int *error_host);
int rpgp_comm_destroy(rpgp_comm *comm);

/*
 * Woodbury preconditioner M = L L^T + sigma^2 I outside the mBCG executor (GPyTorch's `_preconditioner` closure and its
 * `precond_lt` / probe-vector solves, reached from `mll()` at fitting/optimizing.py:69-72): the float64 Gram products and
 * the cancelling update.
 *   rpgp_gram_f64: out[K x T] (row-major float64) = A^T B for fp32 A (N x K, leading dimension lda) and B (N x T, ldb);
 *                  exact products, float64 sums in a fixed order.  K, T <= 64.  Workspace: rpgp_gram_f64_workspace_bytes.
 *   rpgp_woodbury_apply: out[N x T] = (float)(((double)R - L Tm) / noise), Tm: K x T float64 (row-major).
 */
size_t rpgp_gram_f64_workspace_bytes(int K, int T);
int rpgp_gram_f64(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t N, int K, int T, double *out,
                  void *workspace, size_t workspace_bytes, void *stream);
int rpgp_woodbury_apply(const float *L, int64_t ldl, const float *R, int64_t ldr, const double *Tm, double noise,
                        float *out, int64_t ldo, int64_t N, int K, int T, void *stream);
/* The same with t = Cinv gram_LR formed inside the kernel (gram_LR = L^T R from rpgp_gram_f64, Cinv from rpgp_woodbury_setup):
 * M^-1 R in two launches (Gram product, this) instead of four. */
int rpgp_woodbury_apply_cinv(const float *L, int64_t ldl, const float *R, int64_t ldr, const double *gram_LR,
                             const double *Cinv, double noise, float *out, int64_t ldo, int64_t N, int K, int T,
                             void *stream);
/* One launch for the K x K capacitance matrix C = gram + noise I (gram = L^T L, row-major float64, K <= 64): chol = its lower
 * Cholesky factor, cinv = C^-1, logdet[0] = log|C| (all float64, device).  A non-positive pivot fills the outputs with NaN. */
int rpgp_woodbury_setup(const double *gram, double noise, int K, double *chol, double *cinv, double *logdet, void *stream);
/* The same; *logdet_pinned_host (may be NULL) is PINNED host memory (hipHostMalloc) that the kernel writes log|C| to as well:
 * readable by the host once the stream has passed the launch — no device-to-host copy. */
int rpgp_woodbury_setup_pinned(const double *gram, double noise, int K, double *chol, double *cinv, double *logdet,
                               double *logdet_pinned_host, void *stream);

/*
 * Float64 variants for `--double` (training_routines.py:481).  Same contracts as the fp32 entry points of the same
 * name; parity path (software exp, no symmetry exploitation, no workspace).  rpgp_mvm_f64 covers both the square
 * (Z1 == Z2, optional noise) and the rectangular product; `row_scratch` is N doubles of device scratch.
 */
int rpgp_project_f64(const double *X, const double *Peff, double *Z, int64_t N, int d, int J, void *stream);
int rpgp_project_grad_f64(const double *X, const double *G, double *dPeff, int64_t N, int d, int J, void *stream);
int rpgp_mvm_f64(const double *Z1, const double *Z2, const double *V, double *out, int64_t M, int64_t N,
                 int ldz1, int ldz2, int T, int j0, int j1, double scale, double noise, void *stream);
int rpgp_dense_f64(const double *Z1, const double *Z2, double *out, int64_t M, int64_t N, int ldz1, int ldz2,
                   int64_t ldo, int j0, int j1, double scale, void *stream);
int rpgp_bilinear_grad_f64(const double *Z, const double *L, const double *R, double *gZ, double *gscale,
                           int64_t N, int ldz, int ldg, int T, int j0, int j1, double scale,
                           double *row_scratch, void *stream);
int rpgp_bilinear_grad_dense_f64(const double *Z, const double *S, double *gZ, double *gscale, int64_t N,
                                 int ldz, int ldg, int64_t lds, int j0, int j1, double scale,
                                 double *row_scratch, void *stream);

/*
 * Measurement hook used by bench.py (roofline.achieved): between begin/end every rpgp_mvm_sym / rpgp_mvm_rect call
 * records a HIP-event pair on its stream around the dominant fused tile kernel launch(es) (the small slab-reduce
 * launch is outside the pair).  `rpgp_profile_end` synchronises those events and returns the mean duration (ms)
 * and the number of calls in HOST memory.  Not thread-safe; off by default.
 */
int rpgp_profile_begin(void);
int rpgp_profile_end(float *avg_ms_host, int *count_host);

/* Which kernel `rpgp_mvm_sym_prepared` launches for a single-GPU N x N operator with J projections and T right-hand sides on
 * THIS process' settings (benchmark / profile labelling only; no reference counterpart — GPyTorch has one `_matmul`):
 *   0 = mvm_fact_kernel (compiler-scheduled), 1 = mvm_fact_asm_kernel (hand-scheduled loop, rpgp_fact_asm.hip),
 *   2 = mvm_fact_asm_thin_kernel<J> (the same schedule generated for a sweep of exactly J = 2 / 3 / 4 / 5 / 8 / 10 projections:
 *   a rank's slice under the J-split, or a model with that many projections).  Negative: RPGP_EINVAL. */
int rpgp_prepared_kernel_id(int64_t N, int J, int T);

/*
 * Phase markers (SURVEY.md §5 "Tracing / profiling"; the loop they annotate is fitting/optimizing.py:65-76): roctx ranges
 * pushed / popped on the calling thread, recorded by `rocprofv3 --marker-trace`.  The library marks its own phases (one mBCG
 * solve, every 8th CG iteration, all-reduce hook calls); the host stack marks projection + tables, the preconditioner, the
 * derivative and the optimiser update through these two calls.  ROCm's librocprofiler-sdk-roctx is bound at first use ONLY if
 * it is already loaded in the process (rocprofv3 --marker-trace preloads it): otherwise rpgp_range_available() == 0 and the
 * calls do nothing.
 */
int rpgp_range_push(const char *name);
int rpgp_range_pop(void);
int rpgp_range_available(void);

#ifdef __cplusplus
}
#endif
#endif /* RPGP_H */
