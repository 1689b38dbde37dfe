// The GP object that lives in HBM and what its six units share: gp_fit.hip (fits, append, Gram-matrix posteriors),
// gp_posterior.hip (chunk sizing, the chunked posterior and its driver, the acquisition epilogues), gp_halluc.hip (points
// in progress), gp_argmax.hip (arg-max reductions), gp_adducb.hip (the add-UCB stack) and gp_draw.hip (Thompson sampling,
// joint draws, multi-objective calls).  Internal: include/dfhip.h is the contract.
#pragma once
#include "common.h"

struct dfh_gp {
  dfh_ctx* ctx = nullptr;
  KernDev kd;
  int64_t n = 0, d = 0, nblk = 0;
  double noise_var = 0.0;
  double diag_jitter = 0.0;      // what the ladder added on top of noise_var (0 if none)
  double* Xp = nullptr;          // [n][P] packed scaled training inputs
  double* Np = nullptr;          // [n][n_parts]
  double* L = nullptr;           // [n][n] lower factor (strict upper part unspecified)
  double* inv = nullptr;         // [2][nblk][NB][NB]: inverses of the diagonal blocks of L, then clean copies of the blocks
  std::vector<int> refine;       // [nblk] refinement steps the solves take with each block (chol.hip: refine_steps)
  double* alpha = nullptr;       // [n]
  double lml = 0.0;              // log marginal likelihood of the fit (gp_core.py:224-226)
  bool upper_zeroed = false;
  bool gram = false;             // built from a host-evaluated Gram matrix: no kernel, no packed inputs
  int psd_flags = 0;             // DFH_FIT_PROJECT_FIRST / DFH_FIT_TRY_BEFORE_PROJECT the fit ran under (L is not chol(K + noise I) of the kernel's K)
};

// state of the hallucinated augmentation (gp_core.py:192-220)
struct Halluc {
  int64_t q = 0;
  double* Xhp = nullptr; double* Nhp = nullptr;   // packed Xh
  double* Wt = nullptr;                           // [q][n] = K(Xh,X) L^-T
  double* Lh = nullptr;                           // [q][q] chol(K_hh + noise I - Wt Wt^T)
};

#pragma GCC visibility push(hidden)      // what the units share: none of it joins the library's exported symbols

// The points in progress of one call, resolved (halluc_resolve): the block form `h` on gp's own factor, or -- where
// that is not positive definite, or gp's fit needed the ladder -- the augmented GP `aug` factored from scratch, which
// this scope owns and frees.  With q == 0 neither: h.q == 0 and aug == nullptr.
struct HallucScope {
  Halluc h;
  dfh_gp* gp = nullptr;
  dfh_gp* aug = nullptr;
  HallucScope() = default;
  HallucScope(const HallucScope&) = delete;
  HallucScope& operator=(const HallucScope&) = delete;
  ~HallucScope() { if (aug) dfh_gp_free(aug); }
  dfh_gp* cov_gp() const { return aug ? aug : gp; }          // whose factor the variances and covariances come from
  int64_t block_q() const { return aug ? 0 : h.q; }          // rows of the second block row (0: there is none)
  const Halluc* block() const { return block_q() > 0 ? &h : nullptr; }
};

// One chunk of the posterior (posterior_chunk): which parts of the kernel, and what besides the mean.
struct ChunkReq {
  int part_lo = 0, part_hi = -1;        // part range (-1: all of the kernel's)
  bool pre_gathered = false;            // Xs holds only the columns of part_lo (the add-UCB group path)
  bool want_var = true;                 // solve the cross matrix into V^T (and fill ss / ss2)
  const Halluc* h = nullptr;            // block form of the points in progress: the second block row as well
  int parity = 0;                       // which set of chunk buffers (the pipelined Thompson sampling alternates)
  const double* col_w = nullptr;        // one weight per training row on the cross matrix (kernmat_cross: col_w; gp_mf.hip)
};
struct ChunkOut {                       // where posterior_chunk left things (scratch of the request's parity)
  double* Xsp = nullptr; double* Nsp = nullptr;   // the packed candidates
  double* Kct = nullptr;                // cross matrix, V^T once solved
  double* T = nullptr;                  // V2^T: the rows solved against Lh (block form only)
};

// Packed candidates in one scratch block: Xsp [rows][P] at its start, Nsp [rows][n_parts] behind it on a 256-byte boundary
struct PackedXs { size_t nsp_off, bytes; };
inline PackedXs packed_xs_layout(const KernDev& kd, int64_t rows) {
  const size_t b_xsp = ((size_t)rows * kd.P * 8 + 255) / 256 * 256;
  return PackedXs{b_xsp, b_xsp + (size_t)rows * kd.n_parts * 8};
}

// What gp_eval_driver is asked for (predict, acquisition arg-max, add-UCB of one group, point-wise Thompson sampling)
struct EvalReq {
  int acq = DFH_ACQ_MEAN;
  const double* params = nullptr;                 // the acquisition's two parameters (null: zeros)
  const double* Xs = nullptr;                     // candidates [m][ldxs], host or device
  int64_t m = 0, ldxs = 0;
  int part_lo = 0, part_hi = -1;                  // as ChunkReq
  bool pre_gathered = false;
  const double* col_w = nullptr;                  // as ChunkReq (device, [n])
  double kxx = 0.0;                               // prior variance of a stationary part range
  const double* Xh = nullptr; int64_t q = 0;      // points in progress
  const double* U = nullptr;                      // [m] standard normals (host or device): the epilogue is the point-wise
                                                  // Thompson draw, vals_out its samples; acq and params are not read
  double mean_const = 0.0;
  const double* mean_vals = nullptr;              // per candidate (host or device), instead of mean_const
  bool want_var = true;
  double* mu_out = nullptr; double* sd_out = nullptr; double* vals_out = nullptr;     // [m] each, optional
  double* best_val = nullptr; int64_t* best_idx = nullptr;                            // the winner, optional
};

// Running winner of an arg-max over chunks (argmax.h's ordering)
struct Winner {
  bool have = false; double v = 0.0; int64_t i = -1;
  void merge(double ov, int64_t oi);
  int update(dfh_ctx* ctx, const double* vals, int64_t mc, int64_t i0);    // arg-max of vals[0..mc) (device), indices from i0; synchronises
  void store(double* best_val, int64_t* best_idx) const {
    if (best_val) *best_val = v;
    if (best_idx) *best_idx = i;
  }
};

// The candidates and their prior means chunk by chunk, wherever the caller keeps them: a device pointer is offset, a host
// pointer staged (Xs through `slot`, which the pipelined Thompson sampling alternates; the means through SCR_STAGE_D).
struct ChunkStager {
  dfh_ctx* ctx = nullptr; const double* Xs = nullptr; int64_t ldxs = 0; const double* mean_vals = nullptr;
  bool xs_dev = true, mv_dev = true;
  ChunkStager() = default;
  ChunkStager(dfh_ctx* c, const double* Xs_, int64_t ldxs_, const double* mean_vals_)
      : ctx(c), Xs(Xs_), ldxs(ldxs_), mean_vals(mean_vals_), xs_dev(Xs_ ? is_device_ptr(Xs_) : true),
        mv_dev(mean_vals_ ? is_device_ptr(mean_vals_) : true) {}
  int xs(int64_t i0, int64_t mc, int slot, const double** out) const {
    if (xs_dev) { *out = Xs + i0 * ldxs; return DFH_OK; }
    return to_device(ctx, Xs + i0 * ldxs, (size_t)mc * ldxs * 8, slot, out);
  }
  int mean(int64_t i0, int64_t mc, const double** out) const {             // *out = nullptr without mean_vals
    *out = nullptr;
    if (!mean_vals) return DFH_OK;
    if (mv_dev) { *out = mean_vals + i0; return DFH_OK; }
    return to_device(ctx, mean_vals + i0, (size_t)mc * 8, SCR_STAGE_D, out);
  }
};

// What the stacked add-UCB calls differ in (add_ucb_stacked): the additive kernel's groups, or the groups of a
// multi-fidelity GP's additive domain factor at a fixed fidelity (gp_mf.hip)
struct StackedGroups {
  int part0 = 0, G = 0;                 // the groups are the kernel's parts [part0, part0 + G)
  const double* col_w = nullptr;        // weights of the training rows (ChunkReq::col_w), or null
  double prior_scale = 1.0;             // prior variance of group g = prior_scale * k_g(x, x)
  // the per-group route, taken when the stack does not fit one posterior chunk
  std::function<int(int g, double beta, const double* Xg, int64_t m, double* vals, double* best_val, int64_t* best_idx)> one_group;
};

struct DevBlock {           // dev_alloc'ed memory of one call
  dfh_ctx* ctx; void* p = nullptr;
  explicit DevBlock(dfh_ctx* c) : ctx(c) {}
  ~DevBlock() {             // (a block goes back to the cache only once nothing in flight can touch it)
    if (!p) return;
    (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->bulk);
    dev_release(ctx, p);
  }
};

// One launch of the acquisition epilogue (posterior_acq): mean, standard deviation and value of m candidates, each where asked
struct AcqArgs {
  int acq = DFH_ACQ_MEAN; double p0 = 0.0, p1 = 0.0;                  // the acquisition and its two parameters
  double kxx = 0.0; const double* kss = nullptr;                       // prior variance: one for all, or per candidate
  double mean_const = 0.0; const double* mean_vals = nullptr;          // prior mean: one for all, or per candidate
  const double* mu_raw = nullptr; const double* ss = nullptr; const double* ss2 = nullptr;   // (ss null: sd = 0; ss2 optional)
  int64_t m = 0;
  double* mu_out = nullptr; double* sd_out = nullptr; double* val_out = nullptr;
};

// Partial winners of a two-stage arg-max in SCR_RED (argmax_parts): room for cap pairs, behind them the final pair and a flag
struct ArgmaxParts { int cap = 0; double* pv = nullptr; long* pi = nullptr; int* flag = nullptr; };

// gp_posterior.hip
bool free_plus_own_scratch(dfh_ctx* ctx, size_t* bytes);     // free device memory + the context's own scratch; false: unknown
int64_t pick_chunk(dfh_ctx* ctx, int64_t n, int64_t m);      // candidate rows per posterior chunk
int gp_eval_driver(dfh_gp* gp, const EvalReq& rq);          // predict / acquisitions / point-wise TS, chunk by chunk
// One chunk of candidates (device pointer Xs_dev, mc rows): fills mu_raw, ss (and ss2 with rq.h)
int posterior_chunk(dfh_gp* gp, const double* Xs_dev, int64_t mc, int64_t ldxs, const ChunkReq& rq, double* mu_raw,
                    double* ss, double* ss2, ChunkOut* out = nullptr);
int posterior_acq(dfh_ctx* ctx, const AcqArgs& a);
int pointwise_variance_error();                              // sets the point-wise draw's message, returns DFH_ERR_JITTER
// gp_halluc.hip
int halluc_resolve(dfh_gp* gp, const double* Xh, int64_t q, HallucScope* s);
// posterior_chunk with the scope's points in progress; *out is what hs.cov_gp()'s call left, `spare` takes hs.aug's own mean
int halluc_chunk(const HallucScope& hs, const double* Xs_dev, int64_t mc, int64_t ldxs, ChunkReq rq, double* mu_raw, double* ss,
                 double* ss2, double* spare, ChunkOut* out);
int halluc_second_row(dfh_gp* gp, const Halluc& h, const double* Xsp, const double* Nsp, const double* Kct, int64_t rows,
                      int slot, double* ss2, double** T_out);
// gp_argmax.hip (np.argmax's rule throughout: argmax.h)
int argmax_parts(dfh_ctx* ctx, int cap, ArgmaxParts* p);
// stage 2 over p's first nparts partial winners and the pair (with `flag`, p.flag too) copied back; synchronises ctx->stream
int argmax_finish(dfh_ctx* ctx, const ArgmaxParts& p, int nparts, double* best_val, int64_t* best_idx, int* flag = nullptr);
// per row of v [rows x ld] over its first m elements / per segment [off[g], off[g+1]) of v; indices local
int argmax_rows(dfh_ctx* ctx, hipStream_t stream, const double* v, int64_t rows, int64_t ld, int64_t m, double* out_v, long* out_i);
int argmax_segments(dfh_ctx* ctx, const double* v, const long* off, int G, double* out_v, long* out_i);
// gp_adducb.hip
int add_ucb_stacked(dfh_gp* gp, const StackedGroups& sg, const double* betas, const double* Xg_all, const int64_t* m_per_group,
                    double* vals_out, double* best_vals, int64_t* best_idx);
// gp_draw.hip
int add_vec(dfh_ctx* ctx, double* y, const double* a, double c, int64_t n);     // y[i] = (a ? a[i] : 0) + c + y[i]
#pragma GCC visibility pop
