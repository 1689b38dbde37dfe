// Internal declarations shared by the libdfhip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <math.h>
#include <string>
#include <vector>
#include <unordered_map>
#include <functional>
#include "../../include/dfhip.h"

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double double4_t __attribute__((ext_vector_type(4)));

void dfh_set_error(const char* fmt, ...);

#define DFH_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e__ = (call);                                                            \
    if (e__ != hipSuccess) {                                                            \
      dfh_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
      return DFH_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)

#define DFH_TRY(call)                 \
  do {                                \
    int rc__ = (call);                \
    if (rc__ != DFH_OK) return rc__;  \
  } while (0)

#define DFH_ARG(cond)                                                         \
  do {                                                                        \
    if (!(cond)) {                                                            \
      dfh_set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond);    \
      return DFH_ERR_BAD_ARG;                                                 \
    }                                                                         \
  } while (0)

#define DFH_LAUNCH_CHECK() DFH_HIP(hipGetLastError())

// Run-time switches: the value of an environment variable, or dflt when it is not set.  A site keeps
// the result in a `static const` (one read per process) and writes its own clamp, if it has one, next to the call.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
static_assert(sizeof(long) == sizeof(int64_t), "env_long also reads the 64-bit switches");
inline double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
inline bool env_flag(const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; }

// A device allocation that is kept for the life of its owner (ctx scratch or gp state).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// matrices factored in lock-step by one batched cholesky_device call (one pivot flag each)
constexpr int CHOL_MAX_BATCH = 64;
// function attributes (dynamic LDS limits) are per device: the "already set" flags are indexed by it
constexpr int DFH_MAX_DEVICES = 64;

// The labels of the last tuning call, kept on the device between calls: the host copy a call's labels are compared with,
// the device copy (scratch slot SCR_YCACHE), sum y and sum y^2
struct LabelCache {
  std::vector<double> host;
  const double* dev = nullptr;
  double sum = 0.0, sum2 = 0.0;
};

struct dfh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;      // every kernel is launched on this stream ...
  hipStream_t main_stream = nullptr; // (== stream except inside StreamSwap scopes)
  hipStream_t side = nullptr;        // high-priority panel stream of the look-ahead Cholesky
  hipStream_t bulk = nullptr;        // low-priority stream: next chunk's cross kernel + TRSM (TS)
  hipStream_t aux = nullptr;         // off-critical-path work of the factorisation (block inverses)
  std::vector<hipEvent_t> evpool;    // untimed events for cross-stream ordering
  // factorisations that were repeated on the schedule without inter-workgroup hand-offs (a bounded wait
  // expired, or a block inverse was too poor for the resident panels) -- dfh_ctx_counters; after two in a row
  // the next calls go straight to that schedule (chol_cooldown of them), so that a crowded device does not pay
  // the time-out of ~1 s on every fit
  int64_t chol_fallbacks = 0;
  int chol_fallback_streak = 0, chol_cooldown = 0;
  // the kernel-matrix builder's booking (kernmat.h: KmRoute): the route the most recent call took and how many calls
  // there were -- dfh_ctx_counters; the tests hold every case to the kernel it was written for with them
  int64_t km_route = 0, km_dispatches = 0;
  LabelCache labels;               // labels of the last tuning call, resident (lml.hip: resident_labels)
  int lml_team_cooldown = 0;       // tuning batches that take one workgroup per candidate after a team's hand-off timed out
  hipEvent_t ev0 = nullptr, ev1 = nullptr;         // dfh_timer_begin / end
  // scratch pool: grow-only named slots reused across calls (no hipMalloc in hot loops)
  std::vector<DevBuf> scratch;
  int64_t* d_info = nullptr;                         // device int64[CHOL_MAX_BATCH + 16]: pivot flag per batch matrix, 8 debug words, hand-off status
  int64_t* h_info = nullptr;                         // pinned mirror
  void* h_stage = nullptr; size_t h_stage_bytes = 0; // pinned, grow-only: small per-call blobs and results
  // section timing
  bool timing = false;
  double t_ms[DFH_T_COUNT] = {0};
  hipEvent_t tev0[DFH_T_COUNT] = {nullptr}, tev1[DFH_T_COUNT] = {nullptr};   // one pair per section (nestable)
  char name[256] = {0};
  int n_cu = 256;
  double chunk_cap_gib = 0.0;        // posterior chunk cap of this context (gp_posterior.hip: pick_chunk), set on first use
  // Extended GEMM launches of the factorisation (gemm_f64.hip, chol.hip), consumed by the next
  // gemm_f64 call(s) while set: a device-side skip condition (the launch exits unless *gemm_cond >
  // gemm_cond_thr) and the look-ahead tile order with its completion counters.
  const double* gemm_cond = nullptr; double gemm_cond_thr = 0.0;
  int* gemm_la_cnt = nullptr;
  int64_t gemm_solo_launches = 0;   // launches of gemm_f64_solo_kernel since the context was created
  int64_t solve_launches[16] = {0}; // the solve layer's booking since the context was created (SolveCounter; dfh_ctx_solve_launches)
  // per-launch HIP-event profile of the GEMM kernel (bench.py roofline numbers)
  bool gemm_prof = false;
  struct GemmRec { hipEvent_t e0, e1; double flops, bytes; int variant; };
  std::vector<GemmRec> gemm_recs;
  size_t gemm_used = 0;
  hipEvent_t gemm_base = nullptr;   // time origin of the per-launch intervals
  // Block cache behind dev_alloc / dev_release: hipMalloc + hipFree of anything beyond the
  // runtime's small-block arena costs ~0.3 ms (2 MiB), which is most of a GP fit at n < 1000 --
  // the hyper-parameter searches of the reference fit and drop thousands of those in a row.
  struct PoolBlock { void* p; size_t cap; };
  std::vector<PoolBlock> pool_idle;                 // released blocks, ready for reuse
  std::unordered_map<void*, size_t> pool_caps;      // capacity of every block handed out or idle
  size_t pool_idle_bytes = 0;
  size_t pool_idle_limit = size_t(2) << 30;         // DFH_POOL_MAX_MIB (0 disables the cache)
};

enum ScratchSlot {
  SCR_STAGE_A = 0,  // host->device staging of inputs
  SCR_STAGE_B,
  SCR_STAGE_C,
  SCR_STAGE_D,
  SCR_XS,           // scaled / gathered copies
  SCR_KCT,          // candidate-by-train cross kernel / V^T chunk
  SCR_XS2,          // second parity of SCR_XS / SCR_KCT / SCR_VEC (pipelined Thompson sampling)
  SCR_KCT2,
  SCR_VECB,
  SCR_STAGE_A2,
  SCR_TMP,          // TRSM block temp
  SCR_TMP2,
  SCR_VEC,          // small vectors
  SCR_VEC2,
  SCR_VEC3,
  SCR_RED,          // reduction partials
  SCR_CHOLW,        // cholesky panel workspace
  SCR_CHOLINV,      // cholesky diag-block inverses (transient use)
  SCR_CHOLT,        // inverse-assembly temporaries
  SCR_TSK,          // TS block covariance
  SCR_TSL,          // TS block factor
  SCR_AUG,          // hallucination: augmented rows
  SCR_AUG2,
  SCR_OUT,          // device result staging for host outputs
  SCR_OUT2,
  SCR_DELTA,        // quality of the kept block inverses (one double per diagonal block)
  SCR_CHOLSYNC,     // resident look-ahead Cholesky: per-panel counters
  SCR_CHOLX,        // ... its inverse-based panel solve: solution
  SCR_CHOLR,        // ... and residual
  SCR_REFINE,       // residual of the refined row solves (trsm_rows*)
  SCR_CHOLKEEP,     // ... block inverses when the caller keeps none
  SCR_MUPART,       // cross matrix with the posterior mean fused in: per-block partial sums
  SCR_RED2,         // two-stage log-determinant: per-workgroup partial sums
  SCR_YCACHE,       // labels of the last tuning call (kept across calls: a fitter asks thousands of times with the same y)
  SCR_LMLCTL,       // tuning group: results | failed pivots | status | team flags, one block (one memset, one copy back)
  SCR_AUG2B,        // second parity of SCR_AUG2 (hallucinated Thompson sampling: the pipelined chunks)
  SCR_COUNT
};

// Device memory that outlives a call (GP state, caller-visible buffers): cached by size on release.
// The context's stream is idle whenever a block is released (callers synchronise first), so a
// reused block is never still being written by an earlier launch.
int dev_alloc(dfh_ctx* ctx, size_t bytes, void** out);
void dev_release(dfh_ctx* ctx, void* p);      // ctx may be null / already destroyed: plain hipFree

// pinned host staging memory of at least `bytes` (contents undefined; valid until the next call)
int pinned_get(dfh_ctx* ctx, size_t bytes, void** out);

// returns a device pointer with at least `bytes` capacity (contents undefined)
int scratch_get(dfh_ctx* ctx, int slot, size_t bytes, void** out);
bool ctx_is_live(const dfh_ctx* ctx);    // false once dfh_ctx_destroy ran (or for a foreign pointer)

// Resolve a user pointer: if it is a host pointer, copy `bytes` to scratch slot `slot` and
// return the device copy; if it is a device pointer return it unchanged.
int to_device(dfh_ctx* ctx, const void* p, size_t bytes, int slot, const double** out);
bool is_device_ptr(const void* p);
// MT19937 state n_words further down the stream, by jump-ahead on the host (mtjump.hip)
int mt19937_advance_host(uint32_t* key, int32_t* pos, int64_t n_words);
// Copy a device result to a user pointer that may be host or device.
int from_device(dfh_ctx* ctx, void* user_dst, const void* dev_src, size_t bytes);

// Temporarily route launches to another stream of the same context.
struct StreamSwap {
  dfh_ctx* c; hipStream_t old;
  StreamSwap(dfh_ctx* ctx, hipStream_t s) : c(ctx), old(ctx->stream) { c->stream = s; }
  ~StreamSwap() { c->stream = old; }
};
int ctx_event(dfh_ctx* ctx, size_t idx, hipEvent_t* out);   // lazily created, untimed
// index ranges of the context's event pool: the Thompson pipeline's five events come first, the
// factorisation's 2 + 5 per panel follow without an upper limit (the pool grows on demand), so the
// largest factorisation is set by memory, not by the pool
constexpr size_t EV_TS_BASE = 0;
constexpr size_t EV_CHOL_BASE = 8;

struct SectionTimer {
  dfh_ctx* ctx; int which; bool on;
  SectionTimer(dfh_ctx* c, int w);
  ~SectionTimer();
};

// ---------------------------------------------------------------------------------------
// device-level building blocks (all asynchronous on ctx->stream, device pointers only)
// ---------------------------------------------------------------------------------------
#define GEMM_LOWER   1   // compute only tiles intersecting the lower triangle (row >= col)
#define GEMM_KTRI_B  2   // B is [N x K] lower triangular (B[j][k]=0 for k>j): clip k-range
#define GEMM_TRANSB  4   // B is [K x N]

// Two-level batch: blockIdx.z = b2 * count + b1 ; operand offset = b1 * s? + b2 * s?2
struct GemmBatch {
  int count = 1; int64_t sA = 0, sB = 0, sCin = 0, sCout = 0;
  int count2 = 1; int64_t sA2 = 0, sB2 = 0, sCin2 = 0, sCout2 = 0;
};

// Cout = beta*Cin + alpha * A * op(B).  Cin may equal Cout.  Cin may be null iff beta == 0.
int gemm_f64(dfh_ctx* ctx, int flags, int64_t M, int64_t N, int64_t K, double alpha,
             const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
             const double* Cin, int64_t ldcin, double* Cout, int64_t ldc,
             const GemmBatch* batch = nullptr);

// What ran inside the triangular solves (dfh_ctx::solve_launches, in the order dfh_ctx_solve_launches reports): counted on
// the host where the kernel is launched, so that a test can hold a case to the kernel it was written for.
enum SolveCounter {
  SOLVE_TRSV_BLK_FWD = 0,       // k_trsv_blk_fwd
  SOLVE_TRSV_UPD_FWD8,          // k_trsv_upd_fwd<8>
  SOLVE_TRSV_UPD_FWD2,          // k_trsv_upd_fwd<2>
  SOLVE_TRSV_BLK_BWD,           // k_trsv_blk_bwd
  SOLVE_TRSV_UPD_BWD16,         // k_trsv_upd_bwd<16>
  SOLVE_TRSV_UPD_BWD64,         // k_trsv_upd_bwd<64>
  SOLVE_TRSV_GENERAL_BLOCKS,    // 512-blocks solved by the general single-vector route (gemv_rows / gemv_cols)
  SOLVE_REFINE_STEPS,           // refinement steps, one per step, block and solve (single-vector and row solves alike)
  SOLVE_SKINNY_BASE,            // gemm_skinny_kernel<MT, SPLIT>, eight slots: <1>, <2>, then <4>, <8>, <16> each unsplit, split
  SOLVE_COUNTERS = 16
};

// Few-row variant (m <= 256, K a multiple of 64, NT only): streams B once, see gemm_f64.hip.
// Acopy (optional, 16-byte aligned rows, even ld): A is also copied there -- it must not overlap
// anything the call reads or writes.
bool gemm_skinny_applies(int64_t m, int64_t N, int64_t K, const double* A, int64_t lda, const double* B,
                         int64_t ldb);
int gemm_skinny_nt(dfh_ctx* ctx, int64_t m, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                   const double* B, int64_t ldb, double beta, const double* Cin, int64_t ldcin, double* Cout,
                   int64_t ldc, double* Acopy = nullptr, int64_t ldacopy = 0);

// Flattened kernel description.  A "part" is one SE / Matern kernel over a subset of the input
// columns: SE and Matern kernels have one part, an additive kernel one part per group
// (dragonfly/gp/kernel.py:484-494).  Inputs are pre-scaled once into a packed layout
//   Xp[n][P],  P = sum_parts pad4(|cols_part|),  Xp[i][poff+c] = X[i][cols[c]] / bw[c]
// (get_scaled_repr, kernel.py:179-181,255-257) with zero padding, plus the per-part squared
// row norms Np[n][n_parts] ((X**2).sum(axis=1), general_utils.py:66-67).
#define DFH_KERNEL_DIST 3   // internal: clip(dist_sq) itself (dfh_dist_squared)
struct PartDev {
  int kind;        // DFH_KERNEL_SE | DFH_KERNEL_MATERN | DFH_KERNEL_DIST | DFH_KERNEL_POLY | DFH_KERNEL_EXPDECAY | DFH_KERNEL_HAMMING
  int poff;        // first packed column
  int kc;          // packed (padded to 4) column count
  int p;           // Matern: int(nu) ; Poly: order ; ExpDecay / Hamming: number of (real) columns
  double scale_c;  // SE / Poly / ExpDecay: scale ; Matern: scale * norm_constant (kernel.py:298)
  double s8, s2;   // Matern: sqrt(8 nu), sqrt(2 nu)
  double gfac;     // Matern: Gamma(p+1)/Gamma(2p+1) ; ExpDecay: offset
  double coeff[8]; // Matern: (p+i)!/(i!(p-i)!) ; ExpDecay: powers
  double k0;       // SE / Matern: k_part(x, x) (distance 0); Hamming: the sum of the weights (k(x, x) for every x);
                   // unused for Poly / ExpDecay
  // A part of an ADDITIVE FACTOR of a product kernel (an AdditiveKernel among the kernels of a
  // CoordinateProductKernel: the multi-fidelity GP with an additive domain model, gp/euclidean_gp.py:696-707):
  // the factor's parts are adjacent; they are summed (0 + k_1 + k_2 ..., kernel.py:490-493), the sum is
  // scaled (kernel.py:494) and only then multiplied into the product (kernel.py:588).
  // A part of a PRODUCT FACTOR (FM_PROD: a CartesianProductKernel among the kernels of a CartesianProductKernel, the
  // fidelity-space and domain kernels of a CPMFGP, gp/cartesian_product_gp.py:310-319): the factor's parts are
  // adjacent; the factor starts at fscale * 1.0 (scale * np.ones, kernel.py:526), is multiplied by each part in turn
  // (kernel.py:532) and multiplies the product at its last part.
  int fmode;       // 0: a factor of its own ; FM_IN / FM_PROD (| FM_BEGIN | FM_END): inside an additive / a product factor
  int fpad;
  double fscale;   // the additive / product factor's scale (every part of the factor carries it)
};
constexpr int FM_IN = 4, FM_BEGIN = 1, FM_END = 2, FM_PROD = 8;
constexpr int EXPDECAY_MAX_DIM = 8;
constexpr int HAMMING_MAX_DIM = 32;    // one operand chunk of the kernel-matrix kernel (KM_KC); one level of NumPy's pairwise sum
// where the weights of the Hamming columns sit in a kernel's device image (kerndev.hip: blob_layout), from its start
__host__ __device__ inline size_t blob_hw_offset(int n_parts, int P) {
  const size_t p = P ? P : 1;
  const size_t a16 = 15;
  return ((sizeof(PartDev) * (size_t)n_parts + a16) & ~a16) + ((8 * p + a16) & ~a16) + 2 * ((4 * p + a16) & ~a16);
}
struct KernDev {
  int kind = 0, dim = 0, n_parts = 0, P = 0;
  bool multi = false;          // additive: sum over parts then outer scale; product: scale * prod over parts
  bool product = false;        // (multi only) combine the parts by multiplication (kernel.py:584-588)
  bool nested = false;         // (product only) some factor is a sum or a product of parts (PartDev::fmode)
  double outer_scale = 1.0;
  std::vector<PartDev> parts;
  std::vector<int> cols;       // [P] source column per packed column (-1 = padding)
  std::vector<int> lcols;      // [P] column index local to the part (for pre-gathered inputs)
  std::vector<double> bw;      // [P]
  std::vector<double> hw;      // [P] Hamming parts: the column's weight (0 for every other column)
  PartDev* d_parts = nullptr;
  int* d_cols = nullptr;
  int* d_lcols = nullptr;
  double* d_bw = nullptr;
  void* d_blob = nullptr;      // the one device allocation behind the four pointers (owned if set)
  double kxx = 0.0;            // prior variance k(x,x) of a stationary kernel
  bool stationary = true;      // false with a Poly / ExpDecay / Hamming part: the SE / Matern-only kernels do not apply, and
                               // k(x,x) comes from prior_diag (it depends on x for Poly / ExpDecay; a Hamming part's is its k0)
  bool hamming = false;        // some part is a Hamming kernel: the kernel-matrix instances that know the compare (km_generic.hip)
  // ESP kernel (DFH_KERNEL_ESP): one SE / Matern part per column, combined by Newton-Girard into the
  // elementary symmetric polynomial of order esp_order, times outer_scale.  multi is set (several parts)
  // and product is not: every consumer of multi / product must test esp first.
  bool esp = false;
  int esp_order = 0;
};
constexpr int ESP_MAX_ORDER = 32;      // register bucket of the ESP kernel-matrix kernel (km_esp.hip)
constexpr int ESP_MAX_DIM = 256;       // one tile's columns of both operands in LDS
// SE and Matern: k(x, x) does not depend on x (every other kind's prior variance comes from prior_diag)
inline bool kind_is_stationary(int kind) { return kind == DFH_KERNEL_SE || kind == DFH_KERNEL_MATERN; }
inline bool part_is_stationary(const KernDev& kd, int part) { return kind_is_stationary(kd.parts[part].kind); }
int kerndev_build(dfh_ctx* ctx, const dfh_kernel_desc* k, KernDev* out);
// host-only part of kerndev_build, and the upload of several descriptors with one copy into a
// caller-provided device blob (kerndev_blob_bytes each, in order); such KernDevs own no memory
int kerndev_build_host(const dfh_kernel_desc* k, KernDev* out);
int kerndev_stage_many(KernDev* kds, int count, char* host, void* d_blob, size_t blob_bytes);
size_t kerndev_blob_bytes(const KernDev& kd);
void kerndev_blob_fill(const KernDev& kd, char* host);     // the image itself, kerndev_blob_bytes(kd) bytes at host
int kerndev_upload_many(dfh_ctx* ctx, KernDev* kds, int count, void* d_blob, size_t blob_bytes);
int kerndev_build_dist(dfh_ctx* ctx, int dim, KernDev* out);
int kerndev_clone(dfh_ctx* ctx, const KernDev& src, KernDev* out);   // deep copy with its own device image
void kerndev_free(KernDev* kd);
double kerndev_part_kxx(const KernDev& kd, int part);
// out[i] = k(x_i, x_i) from the packed inputs of m points (any kernel; needed when !kd.stationary)
// (an ESP kernel: kd.kxx for every point; the posterior paths use kd.kxx directly for every stationary kernel)
// part_lo / part_hi (default: all parts): the prior variance of those groups of an additive kernel only
int prior_diag(dfh_ctx* ctx, const KernDev& kd, const double* Xp, const double* Np, int64_t m, double* out, int part_lo = 0,
               int part_hi = -1);

// Xp[n][P] / Np[n][n_parts] for parts [part_lo, part_hi) (other parts' columns untouched).
// pre_gathered: X holds only the columns of part_lo (ldx >= |cols|), as in add-UCB group
// candidates (gpb_acquisitions.py:164-166).
// count > 1: a lock-step batch -- kernel images sBlob bytes apart (kd is the first), outputs sXp /
// sNp doubles apart.
int pack_scaled(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool pre_gathered,
                const double* X, int64_t n, int64_t ldx, double* Xp, double* Np, int count = 1,
                int64_t sBlob = 0, int64_t sXp = 0, int64_t sNp = 0);
int kernmat_sym_batch(dfh_ctx* ctx, const KernDev& kd, int count, int64_t sBlob, const double* Xp,
                      int64_t sXp, const double* Np, int64_t sNp, int64_t n, const double* d_diag_adds,
                      double* K, int64_t sK, int64_t ldk);

// K (ldk) = sum over parts [part_lo, part_hi) of k_part (times outer scale if multi) between packed points
// (pack_scaled: Xp[n][P], Np[n][n_parts]).
struct KmPts { const double* Xp; const double* Np; int64_t n; };
// kernmat_gram: K(pts, pts) + diag_add I.  lower_only: the tiles on and below the diagonal suffice (the fit, whose
// factorisation reads nothing above it); the kernels that can then leave the rest of the buffer as it is.
int kernmat_gram(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool apply_outer, KmPts pts, double diag_add,
                 double* K, int64_t ldk, bool lower_only = false);
// kernmat_cross: K(pts1, pts2).  mean: out[pts1.n] = K alpha is wanted from the same pass; done tells whether the kernel
// that ran could do it -- the caller multiplies itself otherwise.
// col_w (device, [pts2.n]; one SE / Matern part only): K[a][i] = col_w[i] * k_part(pts1_a, pts2_i) -- the part on its
// own, without the kernel's outer scale or its other factors (apply_outer is not read); the weight is in before the store,
// so whatever is formed from K afterwards (the mean, the solve) is weighted.  No kernel with col_w fuses the mean.
struct KmMean { const double* alpha; double* out; bool done; };
int kernmat_cross(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool apply_outer, KmPts pts1, KmPts pts2,
                  double* K, int64_t ldk, KmMean* mean = nullptr, const double* col_w = nullptr);

// Blocked Cholesky, in place on the lower triangle of the row-major matrix A (upper part of the
// off-diagonal blocks is left untouched; the upper part of the 64x64 diagonal blocks is zeroed).
// keep_inv (optional): receives the inverses of the CHOL_NB x CHOL_NB diagonal blocks of L,
// block b at keep_inv + b*CHOL_NB*CHOL_NB, row-major with ld = CHOL_NB, zero upper part.
// *info_pivot = 0 on success, else the 1-based index of the first non-positive pivot.
constexpr int64_t CHOL_NB = 512;
// nbatch > 1: nbatch independent matrices of the same size at A + b*strideA are factored in lock
// step (one launch sequence, every kernel batched): the latency-bound pivot chain is paid once.
// info_pivot has nbatch entries.
// keep_inv buffers hold inv_buffer_doubles(n) doubles per matrix: the block inverses, then clean
// copies of the diagonal blocks themselves (lower triangle, zero elsewhere, row stride CHOL_NB).
// refine_out (host, [nbatch][nblk], optional): iterative-refinement steps a solve should take with
// each block, from the measured quality max|I - inv L_bb| of its inverse (chol.hip: refine_steps).
inline int64_t inv_buffer_doubles(int64_t n) { return 2 * ((n + CHOL_NB - 1) / CHOL_NB) * CHOL_NB * CHOL_NB; }
// inv64_only: keep_inv receives only the inverses of the 64 x 64 diagonal blocks (on the diagonal of
// each 512-block slot, zero elsewhere) -- no 512-block assembly, no quality measurement, refine_out
// all zero: for callers that substitute with 64-blocks themselves (the small tuning objective).
// rebuild (optional): restores the input in A; enables the schedules that may need a second attempt
// (chol.hip: resident look-ahead, hand-off timeouts) -- without it those failures are DFH_ERR_HIP.
int cholesky_device(dfh_ctx* ctx, double* A, int64_t n, int64_t lda, double* keep_inv,
                    int64_t* info_pivot, int nbatch = 1, int64_t strideA = 0, int64_t strideKeep = 0,
                    int* refine_out = nullptr, bool inv64_only = false,
                    const std::function<int()>* rebuild = nullptr);
// A in place -> its factor under the stable_cholesky ladder (general_utils.py:166-203): plain Cholesky first; if that
// fails and allow_jitter, 10^-11 .. 10^4 times the largest diagonal entry is added until it factors.  `rebuild`
// re-creates the matrix in A (a failed factorisation destroys it).  *jitter_power: the power that was needed
// (INT32_MIN: none), *jitter_added: what went onto the diagonal.  ld = 0: n.
int stable_cholesky_device(dfh_ctx* ctx, double* A, int64_t n, double* keep_inv, bool allow_jitter,
                           const std::function<int()>& rebuild, int32_t* jitter_power, double* jitter_added,
                           int64_t ld = 0, int* refine_out = nullptr);
constexpr int DFH_INTERNAL_RETRY = 1000;   // chol.hip internal: never crosses the C-ABI (a hand-off wait expired)
constexpr int DFH_INTERNAL_RETRY_COND = 1001;   // ... a block inverse too poor for the inverse-based panel solve (deterministic)

// the largest n the tuning objective runs with one workgroup (or a team) per candidate (lml.h; mgpu.hip shards by it)
constexpr int64_t LMLWG_MAX_N = 2047;

// alpha-solves with the factor and its diagonal-block inverses (in place on x[n]):
//   forward : x <- L^{-1} x          backward : x <- L^{-T} x
// refine (host, one entry per diagonal block, or null): refinement steps per block, see above
int trsv_both(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv, double* x, const int* refine);
int trsv_forward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                 double* x, const int* refine = nullptr);
int trsv_backward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                  double* x, const int* refine = nullptr);
// Rows-as-RHS solve used by the posterior:  Vt[m x n] <- Kct[m x n] * L^{-T}  (in place),
// i.e. each row v of Vt satisfies L v = k  (solve_lower_triangular(L, K_tetr.T), gp_core.py:180)
// diag_override: where the clean copies of L's diagonal blocks are, when not right behind its inverses
int trsm_rows(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
              double* Kct, int64_t m, int64_t ldk, const int* refine = nullptr, const double* diag_override = nullptr);
// Xt[m x n] <- Bt[m x n] * L^{-1} (in place): each row x satisfies L^T x = b
int trsm_rows_backward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                       double* Bt, int64_t m, int64_t ldb, const int* refine = nullptr);
// inverses of the CHOL_NB diagonal blocks of an existing lower factor L (layout as keep_inv)
// diag (optional): where the clean diagonal-block copies go (default: right behind the inverses)
int tri_block_inverses(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, double* inv,
                       int* refine_out = nullptr, double* diag = nullptr);

// projection of a symmetric matrix onto {eigenvalues >= eps} (psdproj.hip); out may alias M
int psd_project_device(dfh_ctx* ctx, const double* M, int64_t n, int64_t ldm, double eps, double* out, int64_t ldo);

// small helpers (elementwise / reductions)
int fill_f64(dfh_ctx* ctx, double* p, int64_t n, double v);
int zero_upper(dfh_ctx* ctx, double* A, int64_t n, int64_t lda);
int diag_max(dfh_ctx* ctx, const double* A, int64_t n, int64_t lda, double* host_out);
int add_diag(dfh_ctx* ctx, double* A, int64_t n, int64_t lda, double v);
int copy_matrix(dfh_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd,
                int64_t rows, int64_t cols);
int transpose_matrix(dfh_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd,
                     int64_t rows, int64_t cols);
// yout[m] = beta*yin + alpha * A[m x n] x[n]   (yin may equal yout; may be null iff beta == 0)
// tri_lower: row i only uses columns j <= i (lower-triangular A)
int gemv_rows(dfh_ctx* ctx, const double* A, int64_t m, int64_t n, int64_t lda, const double* x,
              double alpha, const double* yin, double beta, double* yout, bool tri_lower = false);
// yout[n] = beta*yin + alpha * A[m x n]^T x[m]
int gemv_cols(dfh_ctx* ctx, const double* A, int64_t m, int64_t n, int64_t lda, const double* x,
              double alpha, const double* yin, double beta, double* yout);
// out[m] = sum_j A[i][j]^2
int row_sumsq(dfh_ctx* ctx, const double* A, int64_t m, int64_t n, int64_t lda, double* out);
// host result: sum(log(diag(L))) and dot(a,b)
int logdet_and_dot_device(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* a,
                          const double* b, double* d_out2);
int logdet_and_dot(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* a,
                   const double* b, double* host_logdet, double* host_dot);
// log marginal likelihood from logdet = sum(log L_ii) and dot = (y - m)^T alpha      (gp_core.py:224-226)
inline double lml_value(double logdet, double dot, int64_t n) {
  return -0.5 * dot - logdet - 0.5 * (double)n * log(2.0 * M_PI);
}
// the projection branches of _get_cholesky_decomp (gp_core.py:827-841) among the fit flags
constexpr int DFH_FIT_PSD_FLAGS = DFH_FIT_PROJECT_FIRST | DFH_FIT_TRY_BEFORE_PROJECT;
