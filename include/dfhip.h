/*
 * dfhip.h -- C-ABI of libdfhip.so, the MI355X (gfx950) GP-surrogate + acquisition engine
 * that sits under Dragonfly's GP hot path.
 *
 * The reference (dragonfly 0.1.7, /root/reference) is pure Python/NumPy/SciPy and has no
 * FFI of its own; the seams are Python class boundaries.  Every entry
 * point below names the reference function(s) it replaces (paths relative to the
 * reference root).  The Python host side in dragonfly_amd/ binds these with ctypes
 * (dragonfly_amd/_lib.py); INTEGRATION.md shows the stub a Dragonfly maintainer would add.
 *
 * Conventions
 *   - All matrices are row-major (NumPy C order) float64; indices are int64.
 *   - Every `const double*` / `double*` data argument may be a HOST pointer or a DEVICE
 *     pointer obtained from dfh_malloc(); the library detects which (hipPointerGetAttributes)
 *     and stages host buffers itself.  Scalars returned through pointers are host memory.
 *   - Return value: DFH_OK, or an error code; dfh_last_error() gives the text (thread local).
 *   - Calls on one dfh_ctx are serialised by the caller (the reference is single threaded).
 *   - No callbacks into the host language.  Not fork-safe after the first dfh_ctx_create().
 */
#ifndef DFHIP_H
#define DFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFH_ABI_VERSION 2   /* 2: dfh_kernel_desc grew the additive-factor fields at its end */

/* ---- status codes --------------------------------------------------------------------- */
#define DFH_OK            0
#define DFH_ERR_NOT_PD    1  /* Cholesky met a non-positive pivot (numpy LinAlgError analogue;
                                dragonfly/utils/general_utils.py:178,190)                    */
#define DFH_ERR_BAD_ARG   2  /* ValueError analogue                                          */
#define DFH_ERR_HIP       3  /* HIP runtime error, see dfh_last_error()                      */
#define DFH_ERR_JITTER    4  /* jitter ladder exhausted (ValueError at general_utils.py:200) */

/* ---- kernel description ---------------------------------------------------------------- */
#define DFH_KERNEL_SE       0 /* dragonfly/gp/kernel.py:132 SEKernel                         */
#define DFH_KERNEL_MATERN   1 /* dragonfly/gp/kernel.py:225 MaternKernel, nu in {.5,1.5,2.5} */
#define DFH_KERNEL_ADDITIVE 2 /* dragonfly/gp/kernel.py:461 AdditiveKernel over SE/Matern    */
#define DFH_KERNEL_PRODUCT  3 /* dragonfly/gp/kernel.py:541 CoordinateProductKernel over SE/Matern
                               * (scale * prod_g k_g(X[:, coords_g]); same group fields as ADDITIVE) */
#define DFH_KERNEL_POLY     4 /* dragonfly/gp/kernel.py:331 PolyKernel: scale * ((x*s).(y*s) + 1)^order;
                               * `nu` = order (a non-negative integer), `bw` = dim_scalings s   */
#define DFH_KERNEL_EXPDECAY 5 /* dragonfly/gp/kernel.py:398 ExpDecayKernel (the multi-fidelity
                               * kernel of euclidean_gp.py:881-887): scale * prod_d (1 + x_d +
                               * y_d)^-powers_d + offset; `nu` = offset, `bw` = powers, dim <= 8.
                               * POLY and EXPDECAY are not stationary: k(x,x) depends on x.  They
                               * are accepted alone and as factors of a PRODUCT (sub_kind, with
                               * sub_nu = order / offset and sub_bw = scalings / powers); POLY also
                               * as a group of an ADDITIVE kernel (gp/euclidean_gp.py:870-879).    */
#define DFH_KERNEL_ESP      6 /* dragonfly/gp/kernel.py:671-744 ESPKernel (ESPKernelSE / ESPKernelMatern):
                               * scale * e_order(k_0, .., k_{dim-1}), the elementary symmetric
                               * polynomial of the dim 1-D kernels k_c(x_c, y_c), by Newton-Girard
                               * from the power sums as the reference computes it.  `scale` = ESP
                               * scale, `nu` = order (an integer in 1..dim, at most 32 here),
                               * n_groups = dim with group_off = 0..dim and group_dims[g] = g (one
                               * column per group, in column order); sub_kind[g] SE | MATERN with
                               * sub_scale / sub_nu / sub_bw that 1-D kernel's scale, nu, bandwidth;
                               * group_factor / factor_is_sum / factor_scale NULL.               */
#define DFH_KERNEL_HAMMING  7 /* dragonfly/gp/kernel.py:436-457 HammingKernel (utils/general_utils.py:113-145):
                               * k(x, y) = sum_c w_c [x_c == y_c] over the dim columns, which hold category
                               * codes stored as doubles and are compared for exact equality; the terms are
                               * added in the order of NumPy's (eq * wts).sum(axis=1).  `bw` = dim_weights,
                               * `scale` must be 1 and `nu` 0, dim <= 32.  k(x, x) = sum_c w_c for every x.
                               * Accepted alone and as a factor of a PRODUCT (sub_kind, with sub_bw = the
                               * weights, sub_scale = 1, sub_nu = 0): with SE / Matern / EXPDECAY factors over
                               * other column groups that is the reference's CartesianProductKernel
                               * (kernel.py:504-538).  Not a group of an ADDITIVE kernel or additive factor,
                               * not an ESP member, not in the add-UCB entry points: DFH_ERR_BAD_ARG.       */

/* One Euclidean kernel.  For SE / MATERN: `dim`, `scale`, `nu`, `bw[dim]` (dim_bandwidths); POLY /
 * EXPDECAY reuse `nu` and `bw` as described above.
 * For ADDITIVE: `scale` is the outer scale, and the n_groups sub-kernels are described by the
 * flattened arrays: group g covers input columns group_dims[group_off[g] .. group_off[g+1])
 * with bandwidths sub_bw[group_off[g] .. group_off[g+1]) , kind sub_kind[g], scale
 * sub_scale[g], smoothness sub_nu[g].  All pointers are HOST pointers, read during the call. */
typedef struct dfh_kernel_desc {
  int32_t kind;
  int32_t dim;            /* input dimension d (number of columns of X)                      */
  double  scale;
  double  nu;             /* MATERN: nu ; POLY: order ; EXPDECAY: offset                     */
  const double*  bw;      /* [dim]   SE / MATERN: bandwidths ; POLY: scalings ; EXPDECAY: powers */
  int32_t n_groups;       /* ADDITIVE only                                                   */
  const int32_t* group_off;   /* [n_groups+1]                                                */
  const int32_t* group_dims;  /* [group_off[n_groups]] column indices                        */
  const int32_t* sub_kind;    /* [n_groups] SE | MATERN (| POLY | EXPDECAY | HAMMING in a PRODUCT) */
  const double*  sub_scale;   /* [n_groups]                                                  */
  const double*  sub_nu;      /* [n_groups]                                                  */
  const double*  sub_bw;      /* [group_off[n_groups]]                                       */
  /* PRODUCT only, all three NULL when every group is a factor of its own.  Otherwise an
   * AdditiveKernel may stand among the product's kernels (the multi-fidelity GP with an additive
   * domain model, gp/euclidean_gp.py:696-707; kernel.py:461-501 inside kernel.py:578-589): its
   * groups are listed like any others, group_factor[g] (non-decreasing, 0 .. n_factors-1) says
   * which factor group g belongs to, and a factor f with factor_is_sum[f] != 0 is
   * factor_scale[f] * (k_g + k_g' + ...) over its groups (sub_scale[g] = the group kernels' own
   * scales); a factor with factor_is_sum[f] == 0 has exactly one group and is that kernel.
   * factor_is_sum[f] == DFH_FACTOR_PRODUCT: the factor is itself a product, a CartesianProductKernel
   * among the kernels of a CartesianProductKernel (the fidelity-space and the domain kernel of a
   * multi-fidelity GP on a Cartesian-product domain, gp/cartesian_product_gp.py:310-319).  It is
   * (factor_scale[f] * 1.0) * k_g * k_g' * ... over its groups, left to right, and the value
   * multiplies the running result where its last group ends -- the reference's scale * np.ones,
   * K *= k per part, then K_outer *= K (kernel.py:525-533), rounding for rounding.  Its groups are
   * SE, MATERN, EXPDECAY or HAMMING; a POLY group, an additive factor inside it or a further
   * level of nesting is DFH_ERR_BAD_ARG.  The add-UCB entry points do not take such a kernel.      */
#define DFH_FACTOR_PRODUCT 2
  const int32_t* group_factor;   /* [n_groups]                                               */
  const int32_t* factor_is_sum;  /* [n_factors]                                              */
  const double*  factor_scale;   /* [n_factors]                                              */
} dfh_kernel_desc;

/* ---- acquisitions ---------------------------------------------------------------------- */
#define DFH_ACQ_MEAN  0 /* mu                                                                */
#define DFH_ACQ_UCB   1 /* mu + p0*sd            p0 = beta_th   (gpb_acquisitions.py:211-223)*/
#define DFH_ACQ_EI    2 /* sd*(z*Phi(z)+phi(z)), z=(mu-p0)/sd, p0 = curr_best   (:247-261)   */
#define DFH_ACQ_PI    3 /* Phi((mu-p0)/sd)                                      (:230-239)   */
#define DFH_ACQ_TTEI  4 /* c*(z*Phi(z)+phi(z)), c=sqrt(p1^2+sd^2), z=(mu-p0)/c  (:269-280)   */
#define DFH_ACQ_STD   5 /* sd                                                                */

typedef struct dfh_ctx dfh_ctx;   /* one per device: stream, workspaces                      */
typedef struct dfh_gp  dfh_gp;    /* a fitted GP resident in HBM                              */

/* ---- context / memory ------------------------------------------------------------------ */
int  dfh_abi_version(void);
int  dfh_device_count(int* count);
int  dfh_ctx_create(int device, dfh_ctx** out);
void dfh_ctx_destroy(dfh_ctx* ctx);
int  dfh_sync(dfh_ctx* ctx);
const char* dfh_last_error(void);
int  dfh_device_name(dfh_ctx* ctx, char* buf, size_t buflen);
/* Free / total HBM of the context's device in bytes (hipMemGetInfo); plumbing for leak checks. */
int  dfh_mem_info(dfh_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

int  dfh_malloc(dfh_ctx* ctx, size_t bytes, void** dptr);
int  dfh_free(dfh_ctx* ctx, void* dptr);
int  dfh_memcpy_h2d(dfh_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  dfh_memcpy_d2h(dfh_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* HIP-event timing on the context's stream (the stream every kernel is launched on).
 * dfh_timer_begin records an event; dfh_timer_end records a second one, waits for it and
 * returns the elapsed milliseconds.  Used by bench.py for the roofline numbers.            */
int  dfh_timer_begin(dfh_ctx* ctx);
int  dfh_timer_end(dfh_ctx* ctx, double* ms);

/* ---- linear-algebra building blocks (exposed for tests and for the drop-in utils) ------- */

/* K_out[n1 x n2] = kernel(X1[n1 x d], X2[n2 x d]).  X2 == NULL means X2 = X1.
 * Replaces Kernel.evaluate -> _child_evaluate (dragonfly/gp/kernel.py:76-89,171-181,292-299,
 * 484-494) including dist_squared's clip at 0 (dragonfly/utils/general_utils.py:58-70).
 * diag_add is added to K_out[i][i] (only meaningful when X2 == NULL; fuses
 * `K + noise_var*np.eye(n)`, dragonfly/gp/gp_core.py:843).                                  */
int dfh_kernel_matrix(dfh_ctx* ctx, const dfh_kernel_desc* k,
                      const double* X1, int64_t n1, const double* X2, int64_t n2,
                      double diag_add, double* K_out);

/* Squared Euclidean distances, dragonfly/utils/general_utils.py:58-70 (dist_squared).      */
int dfh_dist_squared(dfh_ctx* ctx, const double* X1, int64_t n1, const double* X2,
                     int64_t n2, int64_t d, double* D_out);

/* C[M x N] = beta*C + alpha * A[M x K] * op(B), op(B) = B^T with B[N x K] (transb = 0) or
 * B[K x N] (transb = 1); fp64 MFMA tiles.  The dense contraction np.dot / dgemm stands for
 * at general_utils.py:68, gp_core.py:174,181.  lower_only != 0 computes only tiles that
 * intersect the lower triangle (SYRK use).                                                   */
int dfh_gemm(dfh_ctx* ctx, int transb, int64_t M, int64_t N, int64_t K, double alpha,
             const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
             double* C, int64_t ldc, int lower_only);

/* In-place lower Cholesky of the row-major n x n matrix A (lda = n); the strict upper
 * triangle is zeroed (numpy.linalg.cholesky semantics, general_utils.py:178).
 * Returns DFH_ERR_NOT_PD if a pivot is <= 0 or NaN; *info_pivot = 1-based index (0 if ok).   */
int dfh_cholesky(dfh_ctx* ctx, double* A, int64_t n, int64_t* info_pivot);

/* stable_cholesky (general_utils.py:166-204): factor M; on failure retry M + 10^p*max(diag M)
 * for p = -11..4.  M_in is preserved, L_out (n x n) receives the factor.
 * *jitter_power = INT32_MIN when no jitter was needed.  DFH_ERR_JITTER if p reaches 5.       */
int dfh_stable_cholesky(dfh_ctx* ctx, const double* M_in, int64_t n, double* L_out,
                        int32_t* jitter_power);

/* project_symmetric_to_psd_cone (utils/general_utils.py:150-163): out = V max(Lambda, epsilon) V^T
 * for the symmetric M = V Lambda V^T (n x n; out may equal M).  Used on the Gram matrix of kernels
 * that are not guaranteed PSD (gp_core.py:838-841, epsilon = 0) and on their posterior covariances
 * (get_post_covar_from_raw_covar, gp_core.py:849-857, epsilon = 0.05 noise_var).  No eigenvectors
 * are formed: epsilon I + (B + B sign(B)) / 2 with B = M - epsilon I and the matrix sign function
 * from 96 Newton-Schulz steps on the fp64 MFMA GEMM (csrc/psdproj.hip); agrees with the eigh route
 * to ~1e-13 |M|.                                                                                */
int dfh_project_psd(dfh_ctx* ctx, const double* M, int64_t n, double epsilon, double* out);

/* Solve L x = b (upper = 0) or L^T x = b (upper = 1) with L lower-triangular n x n row major;
 * b is n x nrhs row-major (nrhs >= 1).  Replaces solve_lower_triangular /
 * solve_upper_triangular (general_utils.py:208-221) as used at gp_core.py:162-163,180.       */
int dfh_solve_triangular(dfh_ctx* ctx, const double* L, int64_t n, int upper,
                         const double* b, int64_t nrhs, double* x_out);

/* ---- GP fit / posterior ----------------------------------------------------------------- */
#define DFH_FIT_NO_JITTER 1  /* report DFH_ERR_NOT_PD instead of running the jitter ladder    */
/* Kernels that are not guaranteed PSD (Cartesian-product / neural-network GPs), _get_cholesky_decomp's
 * other branches (gp/gp_core.py:827-840).  Honoured by dfh_gp_fit_gram, and by dfh_gp_fit and
 * dfh_gp_lml_batch, which build the Gram matrix on the device from the descriptor first.  A handle
 * that dfh_gp_fit made with one of them keeps its kernel and inputs: predictions, acquisitions and
 * dfh_gp_get work on it (DFH_GET_K is the kernel matrix itself, not its projection); its hallucinated
 * posteriors and dfh_gp_append rebuild the extended matrix from scratch under the same flag, because
 * a projection is not a block-row update.  In dfh_gp_lml_batch every candidate of a call with one
 * of them is fitted on its own.                                                                 */
#define DFH_FIT_PROJECT_FIRST      2  /* 'project_first': K -> its projection onto the PSD cone
                                         (dfh_project_psd), then K + noise I and the ladder     */
#define DFH_FIT_TRY_BEFORE_PROJECT 4  /* 'try_before_project': plain Cholesky of K + noise I; only
                                         if that is not positive definite, as project_first    */

/* GP.build_posterior (gp_core.py:155-163) + _get_cholesky_decomp 'guaranteed_psd'
 * (gp_core.py:841-844) + compute_log_marginal_likelihood (gp_core.py:222-227):
 *   K = kernel(X,X); L = stable_cholesky(K + noise_var I); alpha = L^T \ (L \ y_centred);
 *   lml = -1/2 y^T alpha - sum log L_ii - n/2 log 2 pi.
 * X[n x d], y_centred[n] = Y - mean_func(X) (the mean function is a host callable in the
 * reference, gp_core.py:161, so it is evaluated by the caller).                             */
int dfh_gp_fit(dfh_ctx* ctx, const dfh_kernel_desc* k, const double* X, int64_t n, int64_t d,
               const double* y_centred, double noise_var, int flags, dfh_gp** out,
               double* lml, int32_t* jitter_power);
int dfh_gp_free(dfh_gp* gp);

#define DFH_GET_L        0   /* n x n lower factor (GP.L)                                     */
#define DFH_GET_ALPHA    1   /* n (GP.alpha)                                                  */
#define DFH_GET_K        2   /* n x n kernel matrix without noise (GP.K_trtr_wo_noise),
                                recomputed on demand: the fit factors the Gram matrix in place  */
/* Copies one of the fitted quantities above into the caller's buffer `out` (host or device
 * memory, sized as the table says).  These are the attributes the reference reads off a GP from outside
 * (opt/gpb_acquisitions.py:169,171,367,369; gp/gp_core.py:203).  Handles from dfh_gp_fit_gram
 * keep no kernel: DFH_GET_K returns DFH_ERR_BAD_ARG for them.                                 */
int dfh_gp_get(dfh_gp* gp, int what, double* out);
int64_t dfh_gp_n(dfh_gp* gp);

/* Posterior for ANY positive semi-definite kernel the caller evaluates itself: GP.build_posterior
 * (gp/gp_core.py:155-163) with the Gram matrix from the documented override hook
 * GP._get_training_kernel_matrix (:149-153), and GP.eval (:165-190) with the caller's cross matrix.
 * K is n x n (kernel(X, X), without noise); the handle keeps L, alpha and the block inverses, no
 * kernel: it works with dfh_gp_predict_gram / dfh_gp_predict_covar_gram, dfh_gp_get (L, alpha),
 * dfh_gp_n, dfh_gp_free; the kernel-based entry points return DFH_ERR_BAD_ARG for it.            */
int dfh_gp_fit_gram(dfh_ctx* ctx, const double* K, int64_t n, const double* y_centred, double noise_var,
                    int flags, dfh_gp** out, double* lml, int32_t* jitter_power);
/* mu = Kcross alpha + mean, sd = sqrt(kss - rowsumsq(Kcross L^-T)) (no clipping: NaN as NumPy).
 * Kcross [m x n], row i = kernel(x*_i, X); kss [m] = kernel(x*_i, x*_i) (NULL with sd_out NULL).  */
int dfh_gp_predict_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* kss, double mean_const,
                        const double* mean_vals, double* mu_out, double* sd_out);
/* mu_out = Kcross alpha (no mean added), cov_out [m x m] = Ktete - V^T V  (gp_core.py:179-181).   */
int dfh_gp_predict_covar_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* Ktete,
                              double* mu_out, double* cov_out);

/* Incremental posterior update: the posterior of `gp` extended by q new observations, as a NEW
 * handle (`gp` stays valid and unchanged).  Replaces the rebuild of GP.add_data_multiple
 * (gp/gp_core.py:139-146: X.extend, Y.extend, build_posterior) with a block-row append of the
 * Cholesky factor, O(n^2 q) instead of O((n+q)^3); same kernel, noise variance and data order,
 * so L, alpha and lml equal the rebuilt ones up to rounding.  y_centred holds all n+q centred
 * labels (old ones first).  If the existing fit used the stable_cholesky ladder or the appended
 * block is not positive definite, the extended matrix is rebuilt and factored from scratch with
 * the ladder (utils/general_utils.py:166-204), as the reference's rebuild would.               */
int dfh_gp_append(dfh_gp* gp, const double* Xnew, int64_t q, const double* y_centred, int flags,
                  dfh_gp** out, double* lml, int32_t* jitter_power);

/* Hyper-parameter tuning inner loop: log marginal likelihoods of `nb` candidate settings on the
 * same data.  Replaces a loop of GPFitter._tuning_objective calls (gp/gp_core.py:551-564: build_gp
 * -> GP.build_posterior :155-163 -> compute_log_marginal_likelihood :222-227), as issued by
 * random_maximise / random_sample_cts_dscr for the 'rand' and 'rand_exp_sampling' tuners
 * (utils/oper_utils.py:70-80, 100-112; gp_core.py:435-445).  descs[c], mean_consts[c] (NULL = 0),
 * noise_vars[c] describe candidate c; y holds the raw labels (the constant mean is subtracted on
 * the device).  Gram matrices of a group of candidates are factored in lock-step; a candidate that
 * needs the stable_cholesky ladder gets it individually (jitter_powers[c], INT32_MIN = none).
 * Errors as dfh_gp_fit (DFH_ERR_NOT_PD with DFH_FIT_NO_JITTER, DFH_ERR_JITTER when the ladder is
 * exhausted, utils/general_utils.py:200).
 * A call with a handful of candidates -- what the slice sampler (sampling/slice.py:45-68) and the tree search
 * (utils/doo.py:112-121) issue a hundred thousand times per run -- is ONE kernel launch up to n = 128 with nothing
 * copied: descriptors are read from, and results written to, the context's mapped pinned buffer while the host polls
 * a status word (bounded; the call is still synchronous: lml_out is valid on return).                           */
/* Optional hints in `flags` of dfh_gp_lml_batch (a caller that knows where its buffers live saves the library one
 * pointer query each -- microseconds that matter when a slice sampler calls with one candidate at n = 50):          */
#define DFH_LML_X_IS_DEVICE 0x100   /* X is device memory (a dfh_alloc buffer)                                   */
#define DFH_LML_Y_IS_HOST   0x200   /* y is ordinary host memory                                                 */
int dfh_gp_lml_batch(dfh_ctx* ctx, const dfh_kernel_desc* descs, int32_t nb, const double* X, int64_t n,
                     int64_t d, const double* y, const double* mean_consts, const double* noise_vars,
                     int flags, double* lml_out /* [nb] */, int32_t* jitter_powers /* [nb] or NULL */);

/* Triangular solves with the factor (solve_lower/upper_triangular, utils/general_utils.py:208-221,
 * as used at gp_core.py:162-163,180) multiply by explicit inverses of the 512 x 512 diagonal
 * blocks of L; where such an inverse M is not good enough -- max|I - M L_bb| above 1e-13
 * (DFH_REFINE_TOL), i.e. an ill-conditioned block -- the solves add steps of iterative refinement
 * against L_bb so that their residual is that of a substitution (dtrtrs).  steps_out
 * [ceil(n/512)] receives the number of steps per block (0 everywhere for well-conditioned fits). */
int dfh_gp_refine_steps(dfh_gp* gp, int32_t* steps_out);

/* Gradient of the log marginal likelihood of a fit (GP.compute_grad_log_marginal_likelihood,
 * gp/gp_core.py:229-240) in the tuner's coordinates, every component from one inverse of the
 * factored matrix and one pass over it:
 *   grad_out[0]        d lml / d log scale
 *   grad_out[1 + c]    d lml / d log bw_c, c < dim
 *   grad_out[dim + 1]  d lml / d log noise_var
 *   grad_out[dim + 2]  d lml / d (constant mean) = sum alpha
 * It is the gradient of the matrix as factored, K + (noise_var + the jitter the fit added) I.  A
 * pair of points at squared distance 0 (the diagonal, duplicated rows) adds exactly 0 to every
 * bandwidth component.  lml_out (or NULL) receives the value dfh_gp_fit reported.
 * For a handle of dfh_gp_fit / dfh_gp_append with a single SE or MATERN kernel, nu 0.5, 1.5 or
 * 2.5; every other kernel kind, a handle of dfh_gp_fit_gram and a fit under DFH_FIT_PROJECT_FIRST /
 * DFH_FIT_TRY_BEFORE_PROJECT return DFH_ERR_BAD_ARG, dfh_last_error() naming the case.
 * Deterministic: the same bits on every call.                                                   */
int dfh_gp_lml_grad(dfh_gp* gp, double* grad_out /* [dim + 3], host */, double* lml_out /* or NULL */);

/* The same gradient with one entry per bandwidth of every group, so that additive and product
 * kernels have one too (the reference's AdditiveKernel / CoordinateProductKernel have no gradient).
 * Q = dim for a single SE / MATERN kernel; Q = group_off[n_groups] for ADDITIVE / PRODUCT.
 *   grad_out[0]       d lml / d log scale            (the outer scale)
 *   grad_out[1 + q]   d lml / d log bandwidth q      (q < Q: position in the flattened sub_bw /
 *                                                    group_dims arrays; for a single kernel, column q)
 *   grad_out[Q + 1]   d lml / d log noise_var
 *   grad_out[Q + 2]   d lml / d (constant mean) = sum alpha
 * sub_scale[g] enters the value and is not differentiated (the fitters hold it at 1).
 * With S_c = ((x_ic - x_jc) / bw_c)^2 for a column c of group g and dsq_g the group's squared scaled
 * distance, dK / d log bw_c = scale * s_g k_g'(dsq_g) * (-2 S_c) for an ADDITIVE kernel and
 * scale * (prod_{h != g} s_h k_h) * s_g k_g'(dsq_g) * (-2 S_c) for a PRODUCT; a pair of points at
 * squared distance 0 IN GROUP g's COLUMNS adds exactly 0 to group g's bandwidths.
 * For a handle of dfh_gp_fit / dfh_gp_append whose kernel is a single SE / MATERN kernel, or an
 * ADDITIVE or PRODUCT kernel whose groups are all SE / MATERN, nu 0.5, 1.5 or 2.5 throughout.
 * DFH_ERR_BAD_ARG, dfh_last_error() naming the case: a handle of dfh_gp_fit_gram; a fit under
 * DFH_FIT_PROJECT_FIRST / DFH_FIT_TRY_BEFORE_PROJECT; a POLY / EXPDECAY / HAMMING kernel or part; an
 * ESP kernel; a nested factor (group_factor != NULL); len other than Q + 3.
 * For a single kernel the result is dfh_gp_lml_grad's, bit for bit.  The device workspace is that
 * of dfh_gp_lml_grad plus n doubles per group: one pass over the matrix per group.
 * Deterministic: the same bits on every call.                                                   */
int dfh_gp_lml_grad_groups(dfh_gp* gp, double* grad_out /* [len], host */, int64_t len /* must be Q + 3 */,
                           double* lml_out /* or NULL */);

/* GP.eval(X_test, 'std') without the mean function (gp_core.py:165-190):
 *   mu_out[m]  = K(Xs, X) alpha           (caller adds mean_func(Xs))
 *   sd_out[m]  = sqrt(k(x,x) - ||L \ k(X,x)||^2), no clipping -> NaN for negative variance
 * sd_out may be NULL (uncert_form='none').  Only the diagonal of the posterior covariance
 * is formed (the reference forms the m x m matrix and takes its diagonal).
 * If Xh != NULL (q rows) the variance is that of the GP augmented with q hallucinated
 * observations at Xh (eval_with_hallucinated_observations, gp_core.py:192-220); the mean
 * is unchanged.                                                                             */
int dfh_gp_predict(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                   double* mu_out, double* sd_out);

/* Full posterior covariance GP.eval(X_test,'covar') (gp_core.py:179-184): cov_out[m x m].  */
int dfh_gp_predict_covar(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                         double* mu_out, double* cov_out);

/* Fused posterior + acquisition + arg-max over m candidates (gpb_acquisitions.py:215-280
 * closures + oper_utils.random_maximise's `obj_vals.argmax()`, oper_utils.py:73).
 *   mean_const : constant prior mean added to mu (fitter GPs use a constant mean,
 *                gp_core.py:527-530); if mean_vals (optional, [m]) is given it is used instead
 *                (arbitrary mean functions are host callables evaluated by the caller).
 *   params     : acquisition parameters p0, p1 (see DFH_ACQ_*).
 *   vals_out   : optional [m] acquisition values.
 *   best_val / best_idx : numpy argmax semantics -- first NaN wins, else first maximum.     */
int dfh_gp_acq_argmax(dfh_gp* gp, int acq, const double* params, const double* Xs, int64_t m,
                      const double* Xh, int64_t q, double mean_const, const double* mean_vals,
                      double* vals_out, double* best_val, int64_t* best_idx);

/* Blocked-joint Thompson sampling (asy_ts -> GP.draw_samples -> draw_gaussian_samples,
 * gpb_acquisitions.py:119-127, gp_core.py:250-254, general_utils.py:224-232).
 * Candidates are processed in blocks of `block` rows; inside a block the draw is the exact
 * joint draw  s = mu + stable_cholesky(Sigma_block) u ; blocks are independent.  With
 * block >= m this is literally gp.draw_samples(1, Xs).  U[m] are the standard normals
 * (np.random.normal in the reference) supplied by the caller.
 * samples_out optional [m]; jitter_powers_out optional [ceil(m/block)].                     */
int dfh_gp_ts(dfh_gp* gp, const double* Xs, int64_t m, int64_t block, const double* U,
              double mean_const, const double* mean_vals, double* samples_out,
              double* best_val, int64_t* best_idx, int32_t* jitter_powers_out);

/* The joint draw with evaluations in progress and S samples: block by block as dfh_gp_ts, one covariance
 * and one stable_cholesky (jitter ladder included) per block, shared by all S draws; draw s is
 * mu + L_b U_b[:, s].  U is [m x S] row-major -- np.random.normal(size=(m, S)), what
 * draw_gaussian_samples (utils/general_utils.py:224-232) draws.  With block >= m and q == 0 the call is
 * gp.draw_samples(S, Xs) (gp/gp_core.py:250-254); with q > 0 it is
 * gp.draw_samples_with_hallucinated_observations(S, Xs, Xh) (gp_core.py:256-261): the mean from the real
 * data, the covariance from the GP augmented with Xh [q x d] (block form, or the augmented GP factored
 * from scratch where that is not positive definite, as in dfh_mo_ts_argmax).  The product L_b U_b is one
 * launch for all S draws, in the single draw's summation order: row s of an S-draw equals, bit for bit,
 * the S = 1 call with column s of U (an aligned, contiguous vector), and S = 1, q = 0 is dfh_gp_ts.
 * samples_out: optional [S x m], sample-major; best_vals / best_idx: optional [S], np.argmax's winner of
 * each draw (first NaN, else first maximum); jitter_powers_out: optional [ceil(m/block)], INT32_MIN =
 * none.  Xs, U and mean_vals may be host or device pointers.  DFH_ERR_BAD_ARG, before any launch, for
 * S < 1, q < 0, q > 0 without Xh, and a posterior built from a Gram matrix.                            */
int dfh_gp_draw(dfh_gp* gp, const double* Xs, int64_t m, int64_t block,
                const double* Xh, int64_t q,            /* in-progress points, NULL / 0 = none */
                const double* U, int32_t S,             /* [m x S] row-major */
                double mean_const, const double* mean_vals /* [m] or NULL */,
                double* samples_out /* [S x m] or NULL */, double* best_vals /* [S] or NULL */,
                int64_t* best_idx /* [S] or NULL */, int32_t* jitter_powers_out /* [ceil(m/block)] or NULL */);

/* Point-wise Thompson sampling: for every row i the ONE-point draw gp.draw_samples(1, [x_i]) -- with q > 0
 * gp.draw_samples_with_hallucinated_observations(1, [x_i], Xh) -- which is what the reference's maximisers on
 * Cartesian-product domains make of a sampler (opt/gpb_acquisitions.py:35-37 wraps it as acq_fn([x]),
 * exd/exd_utils.py:265 calls it per candidate).  No joint draw: s_i = mu_i + sqrt(v_i) u_i with v_i the posterior
 * variance of row i alone, unclipped; the product and the sum round separately, as L.dot(U).T + mu does
 * (utils/general_utils.py:224-232).  A 1 x 1 stable_cholesky succeeds only for v > 0 and its ladder, which adds
 * 10^p v, rescues neither v <= 0 nor NaN: if any row has such a variance the call returns DFH_ERR_JITTER (and the
 * outputs are unspecified).  The posterior is the chunked one of dfh_gp_acq_argmax (the points in progress in block
 * form, or the augmented GP where that is not positive definite -- always for fits with a projection flag), followed
 * by one kernel per chunk for variance, sample and arg-max: no m x m or per-candidate matrix, no per-candidate launch.
 * U: [m] standard normals; Xs, U, mean_vals and samples_out may be host or device pointers.  samples_out: optional [m];
 * best_val / best_idx: optional, np.argmax's rule (first NaN, else first maximum).  DFH_ERR_BAD_ARG, before any
 * launch, for m < 1, q < 0, q > 0 without Xh, and a posterior built from a Gram matrix.                             */
int dfh_gp_ts_pointwise(dfh_gp* gp, const double* Xs, int64_t m,
                        const double* Xh, int64_t q,            /* in-progress points, NULL / 0 = none */
                        const double* U,                        /* [m] */
                        double mean_const, const double* mean_vals /* [m] or NULL */,
                        double* samples_out /* [m] or NULL */, double* best_val, int64_t* best_idx);

/* add-UCB per-group posterior (gpb_acquisitions.py:139-189): for additive-kernel GPs,
 * group g's acquisition over its own candidate set Xg[m x |g|]:
 *   mu_g = scale*k_g(Xg, X[:,g]) alpha ; sd_g from the shared L ; val = mu_g + beta*sd_g.   */
int dfh_gp_add_ucb_group(dfh_gp* gp, int32_t group, double beta, const double* Xg, int64_t m,
                         double* vals_out, double* best_val, int64_t* best_idx);
/* All groups of the additive model in one call: group g's candidates Xg_all + sum_{h<g} m_h*|group h|
 * ([m_g x |group g|]), betas[g], results best_vals[g] / best_idx[g] (index within the group's
 * candidates), vals_out [sum m_g] or NULL.  The G triangular solves of the reference
 * (opt/gpb_acquisitions.py:161-176) become one solve with sum(m_g) right-hand sides.            */
int dfh_gp_add_ucb_all(dfh_gp* gp, const double* betas, const double* Xg_all, const int64_t* m_per_group,
                       double* vals_out, double* best_vals, int64_t* best_idx);

/* ---- BOCA's decision step on a multi-fidelity GP (opt/gpb_acquisitions.py:313-439) --------------------
 * add-UCB at a fixed fidelity (_add_ucb_for_boca, :334-388).  The GP's kernel must be a PRODUCT of exactly two
 * factors, the first a plain fidelity factor (SE | MATERN | EXPDECAY | POLY over the fidelity columns), the second a
 * sum of SE / MATERN groups (factor_is_sum; the additive domain model, gp/euclidean_gp.py:696-707), and the GP must
 * have been fitted without DFH_FIT_PROJECT_FIRST / DFH_FIT_TRY_BEFORE_PROJECT: DFH_ERR_BAD_ARG otherwise.  z_opt is
 * fidel_to_opt ([number of fidelity columns], host or device).  `group` counts the groups of the additive factor,
 * Xg holds that group's columns only.  With w_i = k_fid(z_opt, Z_i) and k_ff = k_fid(z_opt, z_opt) (:353-354):
 *   K_tetr_j[a][i] = (kern_scale w_i) k_j(x_a, X_i[group j])                                   (:364-366)
 *   mu_j = K_tetr_j alpha ; var_j = (kern_scale k_ff) k_j(x, x) - |L^-1 K_tetr_j^T|^2, not clipped (:367-373)
 *   val = mu_j + beta sqrt(var_j)                                                              (:374)
 * The additive factor's own scale does not enter (the reference uses the group kernels directly).  The weight
 * multiplies the cross matrix where it is stored, so mean and solve read it weighted; the arg-max is np.argmax's
 * (first NaN, else first maximum).  Outputs as dfh_gp_add_ucb_group / _all.                             */
int dfh_mf_add_ucb_group(dfh_gp* gp, const double* z_opt, int32_t group, double beta,
                         const double* Xg, int64_t m, double* vals_out, double* best_val, int64_t* best_idx);
/* Every group of the additive factor in one call, one triangular solve with sum(m_g) right-hand sides (the loop
 * of :357-381): layout of betas / Xg_all / m_per_group / vals_out / best_vals / best_idx as dfh_gp_add_ucb_all. */
int dfh_mf_add_ucb_all(dfh_gp* gp, const double* z_opt, const double* betas, const double* Xg_all,
                       const int64_t* m_per_group, double* vals_out, double* best_vals, int64_t* best_idx);
/* The joint candidates of a fixed fidelity, mfgp.get_ZX_from_ZZ_XX([fidel_to_opt] * m, x) of _get_fidel_to_opt_gp
 * (:314-332; gp/mf_gp.py get_ZX_from_ZZ_XX): out[a] = [z, Xd[a]], m x (p + d), written in HBM.  Xd [m x d] and out
 * are DEVICE buffers, z [p] is a HOST buffer.  With it UCB / EI / PI / TTEI / TS at fidel_to_opt are
 * dfh_gp_acq_argmax / dfh_gp_ts on joint points, with the joint in-progress pairs as Xh.                 */
int dfh_join_fixed_columns(dfh_ctx* ctx, const double* z, int64_t p, const double* Xd, int64_t m, int64_t d,
                           double* out);

/* ---- multi-objective acquisitions (opt/multiobjective_gpb_acquisitions.py:19-107) -----------------
 * K fitted GPs -- one per objective: the same candidates, independent kernels and factors -- in ONE call:
 * candidates -> K posteriors (or K joint draws) -> scalarisation -> arg-max (np.argmax's: first NaN, else
 * first maximum).  The reference's closures call gp.eval / gp.draw_samples once per objective and scalarise
 * K vectors of m values in NumPy.  All K handles must belong to one context and have the same input
 * dimension, 1 <= k <= DFH_MO_MAX_OBJECTIVES; otherwise, and for a zero weight or refs == NULL under
 * DFH_MO_TCH: DFH_ERR_BAD_ARG.  weights [k] / refs [k] (anc_data.obj_weights / .reference_point) are
 * host arrays; mean_consts [k] are the objectives' constant prior means, mean_vals ([k x m], objective-
 * major, host or device) replaces them when given (one of the two must be); vals_out: optional [m].
 * The formulas are the reference's in its order of operations, sums over i = 0 .. k-1:
 *   LIN UCB (:76-90)   (0.0 + sum mu_i w_i) + beta sqrt(0.0 + sum (sd_i sd_i)(w_i w_i))
 *   TCH UCB (:93-106)  min_i ((mu_i + beta sqrt(sd_i) - ref_i) / w_i) from +inf -- the reference takes
 *                      np.sqrt of what gp.eval(.., 'std') returns, the standard deviation; kept
 *   LIN TS  (:19-41)   0.0 + sum s_i w_i
 *   TCH TS  (:44-67)   min_i ((s_i - ref_i) / w_i) from +inf
 * min is np.minimum: NaN when either operand is NaN.                                                  */
#define DFH_MO_LIN 0      /* linear scalarisation      */
#define DFH_MO_TCH 1      /* Tchebychev scalarisation  */
#define DFH_MO_MAX_OBJECTIVES 8

/* mo_lin_asy_ucb / mo_tch_asy_ucb (:76-106) + random_maximise's arg-max (utils/oper_utils.py:73).  beta is
 * the caller's sqrt(0.2 dim log(2 dim t + 1)) (:71-73).  The closures call gp.eval, not the hallucinating
 * wrapper: no Xh here.                                                                                */
int dfh_mo_ucb_argmax(dfh_gp* const* gps, int32_t k, int scal, double beta,
                      const double* weights /*[k]*/, const double* refs /*[k], TCH only*/,
                      const double* Xs, int64_t m,
                      const double* mean_consts /*[k]*/, const double* mean_vals /*[k x m] or NULL*/,
                      double* vals_out /*[m] or NULL*/, double* best_val, int64_t* best_idx);

/* mo_lin_asy_ts / mo_tch_asy_ts (:19-67): s_i is objective i's blocked-joint draw exactly as dfh_gp_ts
 * defines it, from row i of U [k x m] (the reference draws objective 0's m normals, then objective 1's,
 * ...).  With Xh (q in-progress points; get_gp_sampler_for_parallel_strategy, opt/gpb_acquisitions.py:67-87)
 * the block covariance is that of the GP augmented with them (gp/gp_core.py:192-220, 256-261; the mean is
 * unchanged): block >= m is gp.draw_samples_with_hallucinated_observations(1, Xs, Xh).
 * jitter_powers_out: optional [k x ceil(m/block)], INT32_MIN = none.                                   */
int dfh_mo_ts_argmax(dfh_gp* const* gps, int32_t k, int scal,
                     const double* weights, const double* refs,
                     const double* Xs, int64_t m, int64_t block,
                     const double* Xh, int64_t q,            /* hallucinated points, may be NULL / 0 */
                     const double* U /*[k x m], objective-major*/,
                     const double* mean_consts, const double* mean_vals,
                     double* vals_out, double* best_val, int64_t* best_idx,
                     int32_t* jitter_powers_out /*[k x ceil(m/block)] or NULL*/);

/* mo_lin_asy_ts / mo_tch_asy_ts on a Cartesian-product domain, where the reference's maximiser calls the closure one
 * point at a time (opt/gpb_acquisitions.py:35-37, exd/exd_utils.py:265) and the closure draws once per objective:
 * s_ij, candidate i and objective j, is the ONE-point draw that dfh_gp_ts_pointwise(gps[j], ...) makes from the
 * normal U[i*k + j] -- sqrt(v) u + mu with v the unclipped posterior variance of row i alone, product and sum rounded
 * apart; Xh hallucinated exactly as there (block form, or the augmented GP, always for fits with a projection flag).
 * The k draws of a candidate are scalarised by the LIN TS / TCH TS formulas above, sums over j = 0 .. k-1, then the
 * arg-max (first NaN, else first maximum).
 * ORDER OF THE NORMALS: U is [m x k], POINT-major -- the reference's loop over points runs the loop over objectives
 * inside it, each draw taking one np.random.normal(size=(1, 1)).  dfh_mo_ts_argmax above is OBJECTIVE-major ([k x m]):
 * the two layouts are not interchangeable.
 * samples_out: optional [k x m], objective-major (row j: objective j's draws); vals_out: optional [m].  Xs, U,
 * mean_vals, samples_out and vals_out may be host or device pointers.  DFH_ERR_BAD_ARG, before any launch, for the
 * conditions of the section's head, Gram-fitted handles, m < 1, q < 0, q > 0 without Xh, U == NULL, and neither
 * mean_consts nor mean_vals.  DFH_ERR_JITTER (dfh_gp_ts_pointwise's message; outputs unspecified) if any objective's
 * variance at any row is not > 0, NaN included: the reference's 1 x 1 stable_cholesky fails there on every rung. */
int dfh_mo_ts_pointwise(dfh_gp* const* gps, int32_t k, int scal,
                        const double* weights, const double* refs,
                        const double* Xs, int64_t m,
                        const double* Xh, int64_t q,            /* hallucinated points, may be NULL / 0 */
                        const double* U /*[m x k], POINT-major: U[i*k + j]*/,
                        const double* mean_consts, const double* mean_vals /*[k x m] objective-major, or NULL*/,
                        double* samples_out /*[k x m] objective-major, or NULL*/,
                        double* vals_out /*[m] or NULL*/,
                        double* best_val, int64_t* best_idx);

/* ---- candidate generation on the device ---------------------------------------------------
 * The m x d block of uniform candidates every random-search acquisition draws,
 *   np.random.random((max_evals, dim))                   (dragonfly/utils/oper_utils.py:62)
 *   pts * (bounds[:,1] - bounds[:,0]) + bounds[:,0]      (dragonfly/utils/general_utils.py:25-27)
 * produced in HBM, bit for bit what NumPy produces from the same generator state, so neither the
 * host generation nor the m x d host-to-device copy remains.  `bounds` is a HOST array [d][2]
 * (lo, hi) or NULL for the unit cube; `out` [m x d] may be a dfh_malloc() pointer (the candidates
 * then stay on the device for dfh_gp_acq_argmax / dfh_gp_ts / dfh_gp_predict) or a host pointer.
 *
 * dfh_rand_mt19937_uniform continues a legacy NumPy state -- `key`[624] and `pos` of
 * np.random.get_state() -- and updates both in place to the state NumPy would be left in, so the
 * caller hands them back with np.random.set_state() and later host draws continue the stream.
 * dfh_rand_philox_uniform does the same for numpy.random.Philox (Philox4x64-10): key[2], and in/out
 * counter[4], buffer[4], buffer_pos of the bit generator's state.
 * Only rows [row_begin, row_begin + row_count) of the m x d block are written (`out` is
 * [row_count x d]) while the state advances over the whole block: every rank of a multi-GPU run
 * starts from the same state, keeps its own shard of the candidates, and ends in the same state
 * (one process draws them all in the reference).  Philox computes the shard's blocks only; for
 * MT19937 the words before and after the shard are jumped over (polynomial jump-ahead on the host,
 * a few ms whatever the distance) once there are more than 2^23 of them, walked otherwise.
 *
 * dfh_mt19937_advance (host only, no device needed): key / pos after n_words further 32-bit words
 * of the stream, i.e. what np.random.get_state() shows after random_sample(n_words / 2).         */
int dfh_rand_mt19937_uniform(dfh_ctx* ctx, uint32_t* key, int32_t* pos, int64_t m, int64_t d,
                             int64_t row_begin, int64_t row_count, const double* bounds, double* out);
int dfh_mt19937_advance(uint32_t* key, int32_t* pos, int64_t n_words);
/* np.random.normal(size=m) from the same legacy state -- the standard normals draw_gaussian_samples
 * takes (dragonfly/utils/general_utils.py:230; Thompson sampling, gp_core.py:250-254) -- produced in
 * HBM bit for bit: NumPy's legacy_gauss (polar method with rejection on the MT19937 double stream).
 * has_gauss / gauss: in/out, the cached second normal of np.random.get_state()[3:5]; key / pos are
 * updated as by the uniform entry point.  `out` [m] may be a host or a device pointer.  log() is
 * evaluated in double-double on the device; the ~4 % of pairs whose log lies within 0.025 ulp of a
 * rounding boundary are decided by the host C library's log() (what NumPy itself calls).        */
int dfh_rand_mt19937_normal(dfh_ctx* ctx, uint32_t* key, int32_t* pos, int32_t* has_gauss, double* gauss,
                            int64_t m, double* out);
int dfh_rand_philox_uniform(dfh_ctx* ctx, const uint64_t* key, uint64_t* counter, uint64_t* buffer,
                            int32_t* buffer_pos, int64_t m, int64_t d, int64_t row_begin,
                            int64_t row_count, const double* bounds, double* out);

/* ---- multi-GPU: candidate shards across the GPUs of a node ------------
 * The reference has no collective: every candidate of a random-search acquisition sits in ONE
 * array in ONE process and the winner is obj_vals.argmax() (dragonfly/utils/oper_utils.py:59-80,
 * line 73).  Candidates are independent given the fitted GP, so they shard contiguously over the
 * devices; the fit is replicated (identical on every device; one n = 16384 factorisation does not
 * shard profitably over xGMI) and the ONLY exchange is an RCCL all-gather of one 16-byte
 * (value:f64, global row index:i64) pair per rank, followed by the same deterministic reduce on
 * every rank -- first NaN wins, else the largest value, ties to the lowest global index: exactly
 * np.argmax over the whole set (RCCL has no MAXLOC; all-reduce(max) alone would lose the index).
 * RCCL is dlopen'ed on first use; no PyTorch anywhere.                                         */

/* Host-only pieces of the contract (no GPU needed).
 * dfh_shard_bounds: rows [*lo, *hi) of rank's contiguous shard of m candidates, shard edges on
 * multiples of `align` (the Thompson block size, so the blocks -- hence the joint draws -- are
 * those of a single device doing it all).
 * dfh_reduce_argmax: the reduce above over `count` (value, global index) pairs; pairs with
 * idx < 0 (empty shards) are skipped; no pair at all gives (NaN, -1).                          */
int dfh_shard_bounds(int64_t m, int rank, int world, int64_t align, int64_t* lo, int64_t* hi);
int dfh_reduce_argmax(const double* vals, const int64_t* idxs, int count, double* best_val,
                      int64_t* best_idx);

/* (1) One process per GPU.  Rank 0 calls dfh_comm_unique_id (ncclGetUniqueId) and hands the
 * DFH_UNIQUE_ID_BYTES to the other processes by whatever means the host side has; every process
 * then calls dfh_comm_create on its own context (ncclCommInitRank: blocks until all arrived).  */
#define DFH_UNIQUE_ID_BYTES 128
typedef struct dfh_comm dfh_comm;
int  dfh_comm_unique_id(void* id_out /* [DFH_UNIQUE_ID_BYTES] */);
int  dfh_comm_create(dfh_ctx* ctx, int nranks, int rank, const void* id, dfh_comm** out);
void dfh_comm_destroy(dfh_comm* comm);
int  dfh_comm_rank(dfh_comm* comm);
int  dfh_comm_size(dfh_comm* comm);
/* The communicator as RCCL reports it: ranks it formed (ncclCommCount; 0 for the host-exchange test mode), this
 * rank (ncclCommUserRank), library version (ncclGetVersion, e.g. 22707).  No reference counterpart: the reference
 * is one process (dragonfly/utils/oper_utils.py:59-80 finds its arg-max in one array).                          */
int  dfh_comm_info(dfh_comm* comm, int32_t* ranks_formed, int32_t* rank, int32_t* rccl_version);
/* all-gather of (local_val, local_idx) on the context's stream + the reduce; identical result on
 * every rank.  local_idx is the GLOBAL row index (or < 0 for an empty shard).                   */
int  dfh_comm_allgather_argmax(dfh_comm* comm, double local_val, int64_t local_idx,
                               double* best_val, int64_t* best_idx);
/* recv[r*count + j] = rank r's send[j] (host buffers, count <= 4096): the winning candidate's
 * coordinates travelling from its owner to every rank.                                          */
int  dfh_comm_allgather_f64(dfh_comm* comm, const double* send, int count, double* recv);
/* plumbing for benchmarks: element-wise max of inout[count <= 64] over the ranks; barrier.      */
int  dfh_comm_allreduce_max(dfh_comm* comm, double* inout, int count);
int  dfh_comm_barrier(dfh_comm* comm);

/* (2) One process, N devices: a context per device, a host thread per device for the blocking
 * per-device work, one communicator clique (ncclCommInitAll).  device_ids NULL = devices 0..N-1.
 * Fails with DFH_ERR_BAD_ARG when fewer than n_devices are visible.                             */
typedef struct dfh_mgpu dfh_mgpu;
int      dfh_mgpu_create(int n_devices, const int* device_ids, dfh_mgpu** out);
void     dfh_mgpu_destroy(dfh_mgpu* mg);
int      dfh_mgpu_size(dfh_mgpu* mg);
dfh_ctx* dfh_mgpu_ctx(dfh_mgpu* mg, int rank);    /* rank's context (for dfh_malloc / uploads)  */
dfh_gp*  dfh_mgpu_gp(dfh_mgpu* mg, int rank);     /* rank's replica of the current fit, or NULL */
dfh_comm* dfh_mgpu_comm(dfh_mgpu* mg, int rank);
int      dfh_mgpu_sync(dfh_mgpu* mg);
/* Replicated dfh_gp_fit on every device (GP.build_posterior, gp/gp_core.py:155-163).  X[r],
 * y_centred[r]: rank r's copy -- a host pointer (the same one may be given for all ranks) or a
 * pointer into rank r's HBM.  lml, jitter_power: [n_devices] or NULL.  Replaces the previous fit. */
int dfh_mgpu_fit(dfh_mgpu* mg, const dfh_kernel_desc* k, const double* const* X, int64_t n, int64_t d,
                 const double* const* y_centred, double noise_var, int flags, double* lml,
                 int32_t* jitter_power);
int dfh_mgpu_free_fit(dfh_mgpu* mg);
/* The tuning inner loop over the devices: dfh_gp_lml_batch with the candidates cut into contiguous shards, rank r
 * evaluating candidates [shard_lo[r], shard_lo[r + 1]) on its own context from its own host thread.  X[r], y[r]: rank
 * r's copies, as for dfh_mgpu_fit (a host pointer -- the same one may be given for every rank -- or a pointer into
 * rank r's HBM); descs, mean_consts, noise_vars, flags, lml_out, jitter_powers as for dfh_gp_lml_batch, indexed by the
 * global candidate number.  The candidates are independent given (X, y): no communicator is involved.
 * The cut is derived (dfh_lml_shard_plan, host only): up to n = 2047 a candidate is one workgroup and a device runs
 * DFH_MGPU_LML_FILL of them at a time, so used = min(n_devices, ceil(nb / DFH_MGPU_LML_FILL)) ranks take part -- a
 * second device gets work only once the first is full; beyond n = 2047 a candidate is a full fit and
 * used = min(n_devices, nb).  DFH_MGPU_LML_SPREAD in `flags` forces used = n_devices.  Rank r < used takes
 * dfh_shard_bounds(nb, r, used, 1); the others get an empty shard, no thread and no launch.
 * Rank r's slice of the result is bit for bit what dfh_gp_lml_batch returns for those candidates alone on that device
 * (the whole result need not equal ONE single-device call bit for bit: the schedule of a group depends on its size).
 * Every rank has finished when the call returns, also when a shard failed; the status and message are those of the
 * lowest failing rank, which holds the lowest-numbered failing candidate's shard.  nb == 0: DFH_OK, no argument is
 * looked at.  Any other bad argument: DFH_ERR_BAD_ARG before a thread starts.  shard_lo [n_devices + 1] or NULL.      */
#define DFH_MGPU_LML_FILL   256      /* candidates that fill one device: one workgroup per CU                      */
#define DFH_MGPU_LML_SPREAD 0x1000   /* cut the batch over every device, however small it is                        */
int dfh_lml_shard_plan(int32_t nb, int64_t n, int world, int flags, int64_t* shard_lo /* [world + 1] */);
int dfh_mgpu_lml_batch(dfh_mgpu* mg, const dfh_kernel_desc* descs, int32_t nb, const double* const* X, int64_t n,
                       int64_t d, const double* const* y, const double* mean_consts, const double* noise_vars,
                       int flags, double* lml_out /* [nb] */, int32_t* jitter_powers /* [nb] or NULL */,
                       int64_t* shard_lo /* [n_devices + 1] or NULL */);
/* dfh_gp_ts / dfh_gp_acq_argmax over contiguous shards: rank r holds rows [off_r, off_r + m[r]) of
 * the global candidate set, off_r = m[0] + ... + m[r-1]; Xs[r] (and U[r], the shard's standard
 * normals) are host pointers or pointers into rank r's HBM; m[r] == 0 is an empty shard.
 * best_idx is the GLOBAL row index, identical to the single-device call on the concatenated set
 * (for dfh_mgpu_ts when the shards are cut on multiples of `block`).  local_vals / local_idx:
 * optional [n_devices], each rank's own winner (global index) before the exchange.              */
int dfh_mgpu_ts(dfh_mgpu* mg, const double* const* Xs, const int64_t* m, int64_t block,
                const double* const* U, double mean_const, double* best_val, int64_t* best_idx,
                double* local_vals, int64_t* local_idx);
int dfh_mgpu_acq_argmax(dfh_mgpu* mg, int acq, const double* params, const double* const* Xs,
                        const int64_t* m, double mean_const, double* best_val, int64_t* best_idx,
                        double* local_vals, int64_t* local_idx);
/* The same two calls with evaluations in progress.  Xh[r] is rank r's copy of the q in-progress points
 * [q x d] -- a host pointer (the same one for every rank will do) or a pointer into rank r's HBM; NULL /
 * q == 0 = none.  Each rank builds the augmentation on its own replica (block form, or the augmented GP
 * factored from scratch where that is not positive definite).  mean_vals: NULL, or [n_devices] pointers
 * (entries may be NULL) to the prior mean over rank r's shard, which then replaces mean_const there.
 * jitter_powers_out (Thompson): NULL or [sum_r ceil(m[r] / block)], rank after rank, INT32_MIN = none.
 * The contract is the one above: the global winner is that of the single-device call -- dfh_gp_draw with
 * S = 1, or dfh_gp_acq_argmax with Xh -- on the concatenated candidates (Thompson: shards cut on
 * multiples of `block`).                                                                            */
int dfh_mgpu_ts_halluc(dfh_mgpu* mg, const double* const* Xs, const int64_t* m, int64_t block,
                       const double* const* Xh, int64_t q, const double* const* U, double mean_const,
                       const double* const* mean_vals, double* best_val, int64_t* best_idx,
                       double* local_vals, int64_t* local_idx, int32_t* jitter_powers_out);
int dfh_mgpu_acq_argmax_halluc(dfh_mgpu* mg, int acq, const double* params, const double* const* Xs,
                               const int64_t* m, const double* const* Xh, int64_t q, double mean_const,
                               const double* const* mean_vals, double* best_val, int64_t* best_idx,
                               double* local_vals, int64_t* local_idx);
/* the exchange alone: vals / idxs [n_devices] in, the reduced pair out                          */
int dfh_mgpu_allgather_argmax(dfh_mgpu* mg, const double* vals, const int64_t* idxs,
                              double* best_val, int64_t* best_idx);

/* ---- timing of the last call's dominant kernels (HIP events, ms) ------------------------- */
#define DFH_T_KERNMAT  0   /* training kernel-matrix build                                   */
#define DFH_T_CHOL     1   /* blocked Cholesky (all launches)                                */
#define DFH_T_SOLVE    2   /* alpha solves + lml                                             */
#define DFH_T_CROSS    3   /* cross kernel matrices                                          */
#define DFH_T_TRSM     4   /* posterior triangular solves                                    */
#define DFH_T_ACQ      5   /* variance + acquisition + arg-max                               */
#define DFH_T_TS       6   /* TS block covariance + cholesky + sample                        */
#define DFH_T_COUNT    8
int dfh_ctx_timings(dfh_ctx* ctx, int enable, double* ms_out /* [DFH_T_COUNT] or NULL */);

/* Counters of the context since it was created (diagnostics; nothing in the reference corresponds):
 * out[0] = factorisations repeated on the schedule without inter-workgroup hand-offs because a bounded
 * wait expired or a resident panel's block inverse was too poor (the result is the same, the call slower);
 * out[1] = how many of the next factorisations go straight to that schedule (set after two such repeats in
 * a row, e.g. on a device shared with other work); out[2] = the route the most recent kernel-matrix build
 * took (0 none yet, 1 symmetric single-part, 2 cross matrix through LDS, 3 strip, 4 strip with the posterior
 * mean riding along, 5 symmetric multi-part, 6 generic, 7 ESP, 8 column-weighted); out[3] = how many such
 * builds there were.  Both are kept on the host.                                                    */
int dfh_ctx_counters(dfh_ctx* ctx, int64_t* out /* [4] */);

/* Per-launch HIP-event timing of the fp64 MFMA GEMM kernel (the dominant kernel of the path),
 * recorded on the stream each launch goes to.  Returns the totals since the last call in
 * stats_out[8][5] = per kernel variant {launches, sum of launch durations in ms, algorithmic
 * flop, busy ms = length of the union of the launch intervals (launches of different streams
 * overlap), algorithmic bytes = each operand once + the output tile written (and read when it
 * is updated)}; variant index = 4*(B is [K x N]) + 2*(edge path) + (64x64 tiles), so variant 0 is
 * the 128x128 NT throughput configuration.  stats_out may be NULL.  Then enables (1) / disables
 * (0) further recording.                                                                        */
int dfh_ctx_gemm_profile(dfh_ctx* ctx, int enable, double* stats_out /* [40] or NULL */);

/* Launches of the one-workgroup-per-CU ("solo") form of the 128x128 NT GEMM kernel since the context was
 * created (diagnostics; long-K products take it, see DFH_GEMM_SOLO in INTEGRATION.md section 6).  Kept on the host. */
int dfh_ctx_gemm_solo_launches(dfh_ctx* ctx, int64_t* out);

/* What the triangular solves launched since the context was created (diagnostics; kept on the host, counted where the
 * kernel is launched).  out[16]:
 *   [0] k_trsv_blk_fwd   [1] k_trsv_upd_fwd<8>   [2] k_trsv_upd_fwd<2>
 *   [3] k_trsv_blk_bwd   [4] k_trsv_upd_bwd<16>  [5] k_trsv_upd_bwd<64>
 *   [6] 512-blocks solved by the general single-vector route (odd leading dimension, or a block that is refined)
 *   [7] refinement steps run: one per step, block and solve, single-vector and many-right-hand-side solves alike
 *   [8 .. 15] launches of the few-row GEMM gemm_skinny_kernel<MT, SPLIT>: <1>, <2>, <4>, <4, split>, <8>, <8, split>,
 *             <16>, <16, split>.
 * The tests hold every triangular-solve case to the kernels it was written for with them.                          */
int dfh_ctx_solve_launches(dfh_ctx* ctx, int64_t* out /* [16] */);

#ifdef __cplusplus
}
#endif
#endif /* DFHIP_H */
