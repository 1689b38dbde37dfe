// The tuning objective, extern "C" dfh_gp_lml_batch: its route chooser, the workgroup-per-candidate and lock-step schedules,
// and the kernels of the lock-step schedule's solve stage (the one-launch forms live in lml_tiny.hip and lml_wg.h).
#include "lml.h"
#include <cstring>
#include <math.h>
#include <algorithm>

// Hyper-parameter tuning inner loop: the log marginal likelihoods of `nb`
// candidate hyper-parameter settings on the same data, i.e. GPFitter._tuning_objective
// (gp_core.py:551-564 -> build_gp -> build_posterior -> compute_log_marginal_likelihood, :222-227)
// for the list of candidates random_maximise / random_sample_cts_dscr evaluate one by one
// (oper_utils.py:70-80, 100-112).  Candidates are processed in groups whose Gram matrices are
// factored in lock-step by one batched launch sequence; a candidate whose matrix is not positive
// definite falls back to the stable_cholesky ladder on its own, exactly as a single fit would.
__global__ void k_centre(const double* __restrict__ y, double c, double* __restrict__ out,
                         double* __restrict__ out2, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const double v = y[i] - c; out[i] = v; out2[i] = v; }
}

// ---- the solve stage of a lock-step group, all candidates per launch (n > CHOL_NB) --------------------
// The log marginal likelihood needs sum(log L_ii) and (y - m)^T alpha = ||L^-1 (y - m)||^2: one FORWARD
// solve per candidate, no backward solve (what k_lml_tiny does in LDS).  Right-looking block
// substitution as in trsv_forward, but every launch carries all candidates (blockIdx.y): 3 launches
// per 512-block for the whole group instead of ~50 per candidate.
__global__ void k_centre_batch(const double* __restrict__ y, const double* __restrict__ means, double* __restrict__ vecs,
                               long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vecs[(long)blockIdx.y * 2 * n + i] = y[i] - means[blockIdx.y];     // r = y - m  (z is written block by block)
}

// yout[c][row] = beta * yin[c][row] + alpha * A[c][row, 0:n] . x[c][0:n]; one wave per row (n <= 1024), four rows per
// workgroup, blockIdx.y = candidate c; operands sA / sx / sy doubles apart between candidates
__global__ void k_gemv_rows_wave_batch(const double* __restrict__ A, long sA, long m, long n, long lda,
                                       const double* __restrict__ x, long sx, double alpha, const double* yin, double beta,
                                       double* yout, long sy) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const int lane = threadIdx.x & 63;
  const double* a = A + (long)blockIdx.y * sA + row * lda;
  const double* xv = x + (long)blockIdx.y * sx;
  double s0 = 0.0, s1 = 0.0;
  const bool vec = ((lda & 1) == 0) && ((sA & 1) == 0) && ((sx & 1) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  if (vec) {
    const long n2 = n >> 1;
    for (long j = lane; j < n2; j += 64) {
      const double2_t av = reinterpret_cast<const double2_t*>(a)[j];
      const double2_t xx = reinterpret_cast<const double2_t*>(xv)[j];
      s0 = fma(av.x, xx.x, s0);
      s1 = fma(av.y, xx.y, s1);
    }
    if ((n & 1) && lane == 0) s0 = fma(a[n - 1], xv[n - 1], s0);
  } else {
    for (long j = lane; j < n; j += 64) s0 = fma(a[j], xv[j], s0);
  }
  double sum = s0 + s1;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) {
    double v = alpha * sum;
    if (beta != 0.0) v += beta * yin[(long)blockIdx.y * sy + row];
    yout[(long)blockIdx.y * sy + row] = v;
  }
}

// out[2c] = sum(log L_c[i][i]), out[2c+1] = z_c . z_c      (fixed summation order: deterministic)
__global__ __launch_bounds__(256) void k_logdet_sumsq_batch(const double* __restrict__ L, long sL, long n, long ldl,
                                                            const double* __restrict__ z, long sz, double* __restrict__ out) {
  __shared__ double s1[256], s2[256];
  const double* Lc = L + (long)blockIdx.x * sL;
  const double* zc = z + (long)blockIdx.x * sz;
  double ld = 0.0, dt = 0.0;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    ld += log(Lc[i * ldl + i]);
    dt = fma(zc[i], zc[i], dt);
  }
  s1[threadIdx.x] = ld;
  s2[threadIdx.x] = dt;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) { s1[threadIdx.x] += s1[threadIdx.x + st]; s2[threadIdx.x] += s2[threadIdx.x + st]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = s1[0]; out[2 * blockIdx.x + 1] = s2[0]; }
}

// n <= CHOL_NB (one diagonal block): the whole solve stage of a candidate in one workgroup, without the 512-block
// inverse -- r = y - m, forward substitution over 64-blocks with the factor itself and the inverses of its 64 x 64
// diagonal blocks (what trtri64_kernel leaves on the diagonal of the inverse buffer), z_b = Linv_bb (r_b - sum_{i<b} L_bi z_i),
// then out = {sum log L_ii, z . z}  (= yc . alpha: the backward solve is not needed).  blockIdx.x = candidate.  Saves the
// inverse assembly (six GEMM launches) and its quality measurement per call; a 64-block inverse needs no refinement.
__global__ __launch_bounds__(256) void k_lml_finish_small64(const double* __restrict__ L, long sL, long ldl,
                                                            const double* __restrict__ inv, long sInv,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ means, int n,
                                                            double* __restrict__ out2) {
  __shared__ double r[CHOL_NB], z[CHOL_NB], t[64], red[8];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  L += (long)c * sL;
  inv += (long)c * sInv;
  const double mean = means[c];
  for (int i = tid; i < n; i += 256) r[i] = y[i] - mean;
  __syncthreads();
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int w = min(64, n - b0);
    // t = r_b - L[b, 0:b0] z[0:b0], a wave per row
    for (int i = wave; i < w; i += 4) {
      const double* row = L + (long)(b0 + i) * ldl;
      double s = 0.0;
      for (int j = lane; j < b0; j += 64) s = fma(row[j], z[j], s);
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) t[i] = r[b0 + i] - s;
    }
    __syncthreads();
    // z_b = Linv_bb t (lower triangular 64 x 64, row stride CHOL_NB)
    for (int i = wave; i < w; i += 4) {
      const double* row = inv + (long)(b0 + i) * CHOL_NB + b0;
      double s = (lane <= i) ? row[lane] * t[lane] : 0.0;
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) z[b0 + i] = s;
    }
    __syncthreads();
  }
  double ld = 0.0, dt = 0.0;
  for (int j = tid; j < n; j += 256) {
    dt = fma(z[j], z[j], dt);
    ld += log(L[(long)j * ldl + j]);
  }
  for (int off = 32; off > 0; off >>= 1) { ld += __shfl_down(ld, off, 64); dt += __shfl_down(dt, off, 64); }
  if (lane == 0) { red[wave] = ld; red[4 + wave] = dt; }
  __syncthreads();
  if (tid == 0) {
    out2[2 * c] = (red[0] + red[1]) + (red[2] + red[3]);
    out2[2 * c + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

namespace {

// The DFH_LML_* switches of the route chooser and the two schedules, read once per process at the
// first call.  A launcher's own switches stay beside it: DFH_LML_DIRECT, DFH_LML_TINY64 (lml_tiny.hip), DFH_LML_FUSED,
// DFH_LML_FUSED_MAX_N (lml_wg.h: lml_fused_limits).
struct LmlSwitches {
  bool tiny = env_flag("DFH_LML_TINY", true);                 // the one-launch forms
  bool wg = env_flag("DFH_LML_WG", true);                     // one workgroup (or team) per candidate; 0: lock-step for every n
  int wg_min_batch = env_int("DFH_LML_WG_MIN_BATCH", 1);      // ... for calls of at least this many candidates
  int wg_group = env_int("DFH_LML_WG_GROUP", 0);              // > 0: candidates per group of that route (default: one per CU)
  int team = env_int("DFH_LML_TEAM", -1);                     // 0 = never a team, N = teams of up to N workgroups (default: up to 8)
  double group_gib = env_double("DFH_LML_GROUP_GIB", 8.0);    // Gram matrices of one group of candidates (<= 0: the default)
  bool batch_solve = env_flag("DFH_LML_BATCH_SOLVE", true);   // lock-step solve stage at n > 512: all candidates per launch
};
const LmlSwitches& lml_switches() {
  static const LmlSwitches sw;
  return sw;
}

// how many matrices of `doubles` elements a group may hold (DFH_LML_GROUP_GIB)
int64_t group_cap_by_memory(int64_t doubles) {
  const double gib = lml_switches().group_gib > 0.0 ? lml_switches().group_gib : 8.0;
  return std::max<int64_t>(1, (int64_t)(gib * 1073741824.0 / ((double)doubles * 8.0)));
}

// The one place that knows a threshold: which way a call goes.
//   PsdEach  a PSD flag: a projection is per matrix, every candidate is a fit of its own
//   Fused    a handful of mid-sized candidates (a slice sampler's call at 64 <= n <= 128): Gram matrix, factorisation and
//            forward solve of each in ONE launch by one workgroup, nothing copied (lml_wg.h: lml_wgf_kernel)
//   Tiny     small problems: pack, Gram matrix, stable_cholesky and the solve of every candidate in ONE launch (lml_tiny.hip)
//   Wg       one workgroup or a team per candidate up to n = LMLWG_MAX_N
//   Lockstep groups through the batched cholesky_device, any n
enum class LmlRoute { PsdEach, Fused, Tiny, Wg, Lockstep };

LmlRoute lml_route(const LmlCall& a) {
  const LmlSwitches& sw = lml_switches();
  if (a.flags & DFH_FIT_PSD_FLAGS) return LmlRoute::PsdEach;
  if (sw.tiny && a.n <= std::max(TINY_MAX_N, LMLF_KERNEL_MAX_N) && lml_one_launch_kernels(a.kds, a.nb)) {
    const LmlFusedLimits fused = lml_fused_limits();          // (DFH_LML_FUSED_MAX_N is capped at what the kernel takes)
    if (a.n > TINY64_MAX_N && a.n <= std::min(fused.max_n, LMLF_KERNEL_MAX_N) && a.nb <= fused.max_count &&
        lml_fused_fits_lds(a.kds, a.nb, a.n))
      return LmlRoute::Fused;
    if (a.n <= TINY_MAX_N) return LmlRoute::Tiny;
  }
  if (sw.wg && a.n <= LMLWG_MAX_N && a.nb >= sw.wg_min_batch) return LmlRoute::Wg;
  return LmlRoute::Lockstep;
}

// *y_host <- y where the host can read it: y itself, or a copy in `hold` when the labels are resident on the device
int labels_on_host(dfh_ctx* ctx, const double* y, int64_t n, int flags, std::vector<double>& hold, const double** y_host) {
  *y_host = y;
  if ((flags & DFH_LML_Y_IS_HOST) || !is_device_ptr(y)) return DFH_OK;
  hold.resize((size_t)n);
  DFH_HIP(hipMemcpyAsync(hold.data(), y, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *y_host = hold.data();
  return DFH_OK;
}

// what a group's packed inputs (pad-to-4 columns per kernel part) and kernel images need
struct GroupShape {
  int64_t Pmax = 0, parts_max = 0;
  size_t blob_bytes = 0;
  bool uniform = true;                       // structurally identical single-part kernels
};

// of the g candidates kds[0..g), a slice of the call's descriptors
GroupShape group_shape(const KernDev* kds, int g) {
  GroupShape gs;
  for (int c = 0; c < g; ++c) {
    gs.Pmax = std::max<int64_t>(gs.Pmax, kds[c].P);
    gs.parts_max = std::max<int64_t>(gs.parts_max, kds[c].n_parts);
    gs.blob_bytes += kerndev_blob_bytes(kds[c]);
    gs.uniform = gs.uniform && !kds[c].multi && kds[c].n_parts == 1 && kds[c].P == kds[0].P &&
                 kerndev_blob_bytes(kds[c]) == kerndev_blob_bytes(kds[0]);
  }
  return gs;
}

// K + noise_var * I (gp_core.py:843) of the g staged candidates, candidate c at K + c * sK with row stride ldK: a uniform
// group in one pack and one Gram launch (noise d_noise[c], on the device), otherwise candidate by candidate (h_noise[c])
int build_group_grams(dfh_ctx* ctx, const KernDev* kds, int g, const GroupShape& gs, const double* dX,
                      int64_t n, int64_t d, double* Xpb, double* Npb, const double* d_noise, const double* h_noise,
                      double* K, int64_t sK, int64_t ldK) {
  const int64_t sXp = n * gs.Pmax, sNp = n * gs.parts_max;
  if (gs.uniform) {
    const int64_t sBlob = (int64_t)kerndev_blob_bytes(kds[0]);
    DFH_TRY(pack_scaled(ctx, kds[0], 0, 1, false, dX, n, d, Xpb, Npb, g, sBlob, sXp, sNp));
    return kernmat_sym_batch(ctx, kds[0], g, sBlob, Xpb, sXp, Npb, sNp, n, d_noise, K, sK, ldK);
  }
  for (int c = 0; c < g; ++c) {
    double* Xp = Xpb + c * sXp; double* Np = Npb + c * sNp;
    DFH_TRY(pack_scaled(ctx, kds[c], 0, kds[c].n_parts, false, dX, n, d, Xp, Np));
    DFH_TRY(kernmat_gram(ctx, kds[c], 0, kds[c].n_parts, true, KmPts{Xp, Np, n}, h_noise[c], K + c * sK, ldK));
  }
  return DFH_OK;
}

// ---- the lock-step schedule: groups of up to CHOL_MAX_BATCH candidates through the batched cholesky_device (any n) ----

// the buffers of a call's groups (scratch slots of the context: nothing to free) and their host mirrors, for G candidates
struct LockstepBufs {
  int64_t n, nblk, ldK, strideK, strideInv;
  const double* dy = nullptr;
  double *Kb = nullptr, *invb = nullptr, *vecs = nullptr, *red = nullptr, *dpar = nullptr;   // dpar: [g] noise, then [g] mean
  std::vector<double> hred, hpar;
  std::vector<int> refine;                   // refinement steps per candidate and diagonal block
  explicit LockstepBufs(int64_t n_)
      : n(n_), nblk((n_ + CHOL_NB - 1) / CHOL_NB), ldK((n_ + 1) & ~(int64_t)1),     // even leading dimension: 16-byte row starts
        strideK(n_ * ldK), strideInv(inv_buffer_doubles(n_)) {}
};
// candidates c0 .. c0 + g of the call, their descriptors uploaded and their inputs packed at Xpb / Npb
struct LockstepGroup { int c0, g; const KernDev* kds; GroupShape gs; double *Xpb, *Npb; };

int lockstep_buffers(const LmlCall& a, int G, LockstepBufs& b) {
  dfh_ctx* ctx = a.ctx;
  DFH_TRY(to_device(ctx, a.y, (size_t)b.n * 8, SCR_STAGE_B, &b.dy));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)G * b.strideK * 8, (void**)&b.Kb));
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)G * b.strideInv * 8, (void**)&b.invb));
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)G * b.n * 8 * 2, (void**)&b.vecs));
  DFH_TRY(scratch_get(ctx, SCR_OUT2, (size_t)std::max(256, G * 16), (void**)&b.red));   // SCR_RED belongs to the gemv partials
  DFH_TRY(scratch_get(ctx, SCR_OUT, (size_t)std::max(256, G * 16), (void**)&b.dpar));
  b.hred.resize((size_t)G * 2); b.hpar.resize((size_t)G * 2);
  b.refine.assign((size_t)G * b.nblk, 0);
  return DFH_OK;
}

// descriptors (device images in one scratch blob: nothing to free), room for the packed inputs, {noise, mean} of the group
int lockstep_stage_group(const LmlCall& a, LockstepBufs& b, int c0, int g, LockstepGroup& grp) {
  dfh_ctx* ctx = a.ctx;
  grp = LockstepGroup{c0, g, a.kds + c0, group_shape(a.kds + c0, g), nullptr, nullptr};
  void* blob = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_AUG2, grp.gs.blob_bytes, &blob));
  DFH_TRY(kerndev_upload_many(ctx, a.kds + c0, g, blob, grp.gs.blob_bytes));
  DFH_TRY(scratch_get(ctx, SCR_XS, (size_t)g * b.n * grp.gs.Pmax * 8, (void**)&grp.Xpb));
  DFH_TRY(scratch_get(ctx, SCR_XS2, (size_t)g * b.n * grp.gs.parts_max * 8, (void**)&grp.Npb));
  for (int c = 0; c < g; ++c) {
    b.hpar[c] = a.noise_vars[c0 + c];
    b.hpar[g + c] = a.mean_consts ? a.mean_consts[c0 + c] : 0.0;
  }
  DFH_HIP(hipMemcpyAsync(b.dpar, b.hpar.data(), (size_t)g * 16, hipMemcpyHostToDevice, ctx->stream));
  return DFH_OK;
}

// K + noise_var * I of candidate c again, from the packed inputs (a failed factorisation destroys it)
int lockstep_rebuild(const LmlCall& a, const LockstepBufs& b, const LockstepGroup& grp, int c) {
  const int64_t n = b.n;
  double* Xp = grp.Xpb + c * n * grp.gs.Pmax; double* Np = grp.Npb + c * n * grp.gs.parts_max;
  return kernmat_gram(a.ctx, grp.kds[c], 0, grp.kds[c].n_parts, true, KmPts{Xp, Np, n}, a.noise_vars[grp.c0 + c],
                      b.Kb + c * b.strideK, b.ldK);
}

// the batched factorisation; a candidate whose matrix is not positive definite then takes the stable_cholesky ladder on
// its own, exactly as a single fit would
int lockstep_factor_group(const LmlCall& a, LockstepBufs& b, const LockstepGroup& grp) {
  dfh_ctx* ctx = a.ctx;
  const int64_t n = b.n;
  int64_t piv[CHOL_MAX_BATCH] = {0};
  // n <= 512: the finish kernel substitutes with 64-blocks, so the 512-block inverse is not built
  const bool inv64_only = n <= CHOL_NB;
  const std::function<int()> rebuild_all = [&]() -> int {
    for (int c = 0; c < grp.g; ++c) DFH_TRY(lockstep_rebuild(a, b, grp, c));
    return DFH_OK;
  };
  int rc = cholesky_device(ctx, b.Kb, n, b.ldK, b.invb, piv, grp.g, b.strideK, b.strideInv, b.refine.data(), inv64_only,
                           &rebuild_all);
  if (rc != DFH_OK && rc != DFH_ERR_NOT_PD) return rc;
  for (int c = 0; c < grp.g; ++c) {
    const int cand = grp.c0 + c;
    if (a.jitter_powers) a.jitter_powers[cand] = INT32_MIN;
    if (piv[c] == 0) continue;
    if (a.flags & DFH_FIT_NO_JITTER) {
      dfh_set_error("Matrix is not positive definite (candidate %d, pivot %lld)", a.cand_base + cand, (long long)piv[c]);
      return DFH_ERR_NOT_PD;
    }
    auto rebuild = [&]() -> int { return lockstep_rebuild(a, b, grp, c); };
    DFH_TRY(rebuild());
    int32_t jp = INT32_MIN;
    DFH_TRY(stable_cholesky_device(ctx, b.Kb + c * b.strideK, n, b.invb + c * b.strideInv, true, rebuild, &jp, nullptr, b.ldK,
                                   b.refine.data() + (size_t)c * b.nblk));
    if (a.jitter_powers) a.jitter_powers[cand] = jp;
  }
  return DFH_OK;
}

// n <= 512, one workgroup per candidate: substitution with 64-blocks
// (a candidate that went through the jitter ladder has the full inverse in its slot: its diagonal
//  64-blocks are the inverses of the factor's diagonal blocks all the same)
int lockstep_solve_small64(dfh_ctx* ctx, const LockstepBufs& b, int g) {
  hipLaunchKernelGGL(k_lml_finish_small64, dim3((unsigned)g), dim3(256), 0, ctx->stream, b.Kb, (long)b.strideK, (long)b.ldK,
                     b.invb, (long)b.strideInv, b.dy, b.dpar + g, (int)b.n, b.red);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// all candidates per launch: r = y - m; for each 512-block z_b = M_b r_b, r_below -= L[below, b] z_b
int lockstep_solve_batched(dfh_ctx* ctx, const LockstepBufs& b, int g) {
  const int64_t n = b.n, NB = CHOL_NB;
  const long sv = 2 * (long)n;                 // candidate c: r at vecs + c*sv, z behind it
  double* vecs = b.vecs;
  hipLaunchKernelGGL(k_centre_batch, dim3((unsigned)((n + 255) / 256), (unsigned)g), dim3(256), 0, ctx->stream, b.dy,
                     b.dpar + g, vecs, (long)n);
  DFH_LAUNCH_CHECK();
  for (int64_t b0 = 0; b0 < n; b0 += NB) {
    const int64_t w = std::min<int64_t>(NB, n - b0), below = n - b0 - w;
    hipLaunchKernelGGL(k_gemv_rows_wave_batch, dim3((unsigned)((w + 3) / 4), (unsigned)g), dim3(256), 0, ctx->stream,
                       b.invb + (b0 / NB) * NB * NB, (long)b.strideInv, (long)w, (long)w, (long)NB, vecs + b0, sv, 1.0,
                       (const double*)nullptr, 0.0, vecs + n + b0, sv);
    DFH_LAUNCH_CHECK();
    if (below > 0) {
      hipLaunchKernelGGL(k_gemv_rows_wave_batch, dim3((unsigned)((below + 3) / 4), (unsigned)g), dim3(256), 0,
                         ctx->stream, b.Kb + (b0 + w) * b.ldK + b0, (long)b.strideK, (long)below, (long)w, (long)b.ldK,
                         vecs + n + b0, sv, -1.0, vecs + b0 + w, 1.0, vecs + b0 + w, sv);
      DFH_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(k_logdet_sumsq_batch, dim3((unsigned)g), dim3(256), 0, ctx->stream, b.Kb, (long)b.strideK, (long)n,
                     (long)b.ldK, vecs + n, sv, b.red);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// candidate by candidate (some block's inverse wants refinement, or DFH_LML_BATCH_SOLVE=0)
int lockstep_solve_each(dfh_ctx* ctx, const LockstepBufs& b, int g) {
  const int64_t n = b.n;
  for (int c = 0; c < g; ++c) {
    double* yc = b.vecs + (int64_t)c * 2 * n;
    double* alpha = yc + n;
    hipLaunchKernelGGL(k_centre, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, b.dy, b.hpar[g + c], yc, alpha, (long)n);
    DFH_LAUNCH_CHECK();
    // alpha = L^T \ (L \ (y - m))      (gp_core.py:161-163)
    DFH_TRY(trsv_both(ctx, b.Kb + c * b.strideK, n, b.ldK, b.invb + c * b.strideInv, alpha, b.refine.data() + (size_t)c * b.nblk));
    DFH_TRY(logdet_and_dot_device(ctx, b.Kb + c * b.strideK, n, b.ldK, yc, alpha, b.red + 2 * c));
  }
  return DFH_OK;
}

// the solve stage in the form the size and the inverses' quality allow, and the group's results
int lockstep_solve_group(const LmlCall& a, LockstepBufs& b, const LockstepGroup& grp) {
  dfh_ctx* ctx = a.ctx;
  const int g = grp.g;
  bool any_refine = false;
  for (size_t i = 0; i < (size_t)g * b.nblk; ++i) any_refine = any_refine || b.refine[i] > 0;
  if (b.n <= CHOL_NB) DFH_TRY(lockstep_solve_small64(ctx, b, g));
  else if (!any_refine && lml_switches().batch_solve) DFH_TRY(lockstep_solve_batched(ctx, b, g));
  else DFH_TRY(lockstep_solve_each(ctx, b, g));
  DFH_HIP(hipMemcpyAsync(b.hred.data(), b.red, (size_t)g * 16, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < g; ++c) a.lml_out[grp.c0 + c] = lml_value(b.hred[2 * c], b.hred[2 * c + 1], b.n);
  return DFH_OK;
}

int lml_batch_lockstep(const LmlCall& a) {
  dfh_ctx* ctx = a.ctx;
  LockstepBufs b(a.n);
  // group size: up to CHOL_MAX_BATCH matrices and (DFH_LML_GROUP_GIB, default 8) GiB of Gram
  // matrices at a time.  Measured ms per candidate at 2 / 8 GiB: n=4096 1.55 / 1.07, n=16384
  // 42.6 (one at a time) / 30.0 (four in lock-step: the panel chains of the four interleave).
  const int G = (int)std::min<int64_t>(std::min<int64_t>(a.nb, CHOL_MAX_BATCH), group_cap_by_memory(b.strideK));
  DFH_TRY(lockstep_buffers(a, G, b));
  for (int c0 = 0; c0 < a.nb; c0 += G) {
    LockstepGroup grp;
    DFH_TRY(lockstep_stage_group(a, b, c0, std::min(G, a.nb - c0), grp));
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_TRY(build_group_grams(ctx, grp.kds, grp.g, grp.gs, a.dX, a.n, a.d, grp.Xpb, grp.Npb, b.dpar, a.noise_vars + c0, b.Kb,
                                b.strideK, b.ldK));
    }
    {
      SectionTimer t(ctx, DFH_T_CHOL);
      DFH_TRY(lockstep_factor_group(a, b, grp));
    }
    SectionTimer t(ctx, DFH_T_SOLVE);
    DFH_TRY(lockstep_solve_group(a, b, grp));
  }
  return DFH_OK;
}

// candidate c of the call takes the lock-step schedule by itself (which runs the stable_cholesky ladder as a single fit would)
int redo_alone(const LmlCall& a, int c) {
  LmlCall one = a;
  one.descs += c; one.kds += c; one.nb = 1; one.noise_vars += c; one.lml_out += c; one.cand_base += c;
  if (one.mean_consts) one.mean_consts += c;
  if (one.jitter_powers) one.jitter_powers += c;
  return lml_batch_lockstep(one);
}

// ---- one workgroup (or a team) per candidate (lml_wg.h), n <= LMLWG_MAX_N: per group of up to one candidate per CU three
// launches -- pack, Gram matrices, factor + forward solve + reductions -- and one copy back.  A candidate whose matrix
// does not factor as it stands (or whose augmented pivot fails) is handed to the lock-step schedule on its own. ----

// The labels stay resident between calls (round 6): a fitter asks thousands of times with the same y, and staging
// 16 KB of pageable memory per call -- copy, synchronise -- was a sixth of a small group's call.  Host labels are
// compared with the copy of the last call (memcmp: exact); device labels are used where they are.
struct Labels { const double* dy; double sum_y, sum_y2; };

int resident_labels(dfh_ctx* ctx, const double* y, int64_t n, int flags, Labels* out) {
  std::vector<double> y_hold;
  const double* y_host = nullptr;
  DFH_TRY(labels_on_host(ctx, y, n, flags, y_hold, &y_host));
  if (!y_hold.empty()) {                       // device labels, downloaded for their sums
    *out = Labels{y, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i) { out->sum_y += y_host[i]; out->sum_y2 = fma(y_host[i], y_host[i], out->sum_y2); }
    return DFH_OK;
  }
  LabelCache& cache = ctx->labels;
  double* ybuf = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_YCACHE, (size_t)std::max<int64_t>(2048, n) * 8, (void**)&ybuf));
  if (ybuf != cache.dev || cache.host.size() != (size_t)n || std::memcmp(cache.host.data(), y, (size_t)n * 8) != 0) {
    cache.host.assign(y, y + n);
    DFH_HIP(hipMemcpyAsync(ybuf, cache.host.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    DFH_HIP(hipStreamSynchronize(ctx->stream));
    cache.dev = ybuf;
    cache.sum = cache.sum2 = 0.0;
    for (int64_t i = 0; i < n; ++i) { cache.sum += y[i]; cache.sum2 = fma(y[i], y[i], cache.sum2); }
  }
  *out = Labels{ybuf, cache.sum, cache.sum2};
  return DFH_OK;
}

// Where a group of g candidates keeps what.  One control block per group on the device, zeroed by ONE memset and copied
// back by ONE copy into the pinned buffer; descriptors and {aug. diagonal, mean, noise} go up from the pinned buffer in
// ONE copy.  (Round 5: three pageable copies up, three memsets, three pageable copies back and three synchronisations
// per group -- 160 of a small group's 210 us, profiles/r06_small_calls.txt.)
//   pinned:  descriptors | (16-byte aligned) {aug. diagonal, mean, noise} [3 g] | (64-byte aligned) what comes back [3 g + 1]
//   control: results [2 g] | failed pivots [g] | status [1] | team flags [g][LMLT_SYNC_INTS]
struct WgGroupLayout {
  int g;
  size_t up_par, up_bytes, back_off, back_bytes;
  WgGroupLayout(int g_, size_t blob_bytes)
      : g(g_), up_par((blob_bytes + 15) & ~size_t(15)), up_bytes(up_par + (size_t)g_ * 24),
        back_off((up_bytes + 63) & ~size_t(63)), back_bytes((size_t)(3 * g_ + 1) * 8) {}
  size_t pinned_bytes() const { return back_off + back_bytes; }
  static size_t control_bytes(int G) { return (size_t)(3 * G + 8) * 8 + (size_t)G * LMLT_SYNC_INTS * sizeof(int); }
  // failed pivots, status and a team's flags: one memset (the results in front of them are always written)
  size_t zeroed_bytes(int team) const { return (size_t)(g + 1) * 8 + (team > 1 ? (size_t)g * LMLT_SYNC_INTS * sizeof(int) : 0); }
  double* hpar(char* pinned) const { return reinterpret_cast<double*>(pinned + up_par); }
  const double* hred(const char* pinned) const { return reinterpret_cast<const double*>(pinned + back_off); }
  const long long* hinfo(const char* pinned) const { return reinterpret_cast<const long long*>(pinned + back_off) + 2 * g; }
  unsigned long long hstatus(const char* pinned) const { return reinterpret_cast<const unsigned long long*>(pinned + back_off)[3 * g]; }
  double* dpar(void* blob) const { return reinterpret_cast<double*>(static_cast<char*>(blob) + up_par); }
  long long* dinfo(double* ctl) const { return reinterpret_cast<long long*>(ctl + 2 * g); }
  unsigned long long* dstatus(double* ctl) const { return reinterpret_cast<unsigned long long*>(ctl + 3 * g); }
  int* dsync(double* ctl) const { return reinterpret_cast<int*>(ctl + 3 * g + 1); }
};

// a call's buffers and the group in hand: candidates c0 .. c0 + g
struct WgGroup {
  int64_t nbt, NP, sK;                         // tile rows of the augmented system, padded order, doubles per matrix
  Labels labels;
  double *Kb = nullptr, *ctl = nullptr;
  int c0 = 0, g = 0;
  const KernDev* kds = nullptr;
  GroupShape gs;
  WgGroupLayout lay{0, 0};
  char* pinned = nullptr;
  void* blob = nullptr;
  double *Xpb = nullptr, *Npb = nullptr;
  std::vector<char> skip;                      // candidates that go to the lock-step schedule without being tried
};

// hpar <- {aug. diagonal, mean, noise} of the group; skip[c]: nothing bounds candidate c's augmented pivot
void wg_fill_params(const LmlCall& a, WgGroup& w) {
  const int g = w.g;
  double* hpar = w.lay.hpar(w.pinned);
  const double sum_y = w.labels.sum_y, sum_y2 = w.labels.sum_y2;
  for (int c = 0; c < g; ++c) {
    // the augmented row's diagonal entry: c = 1 + |y - m|^2 / s2 > z.z (the eigenvalues of K + s2 I are >= s2)
    // (|y - m|^2 = sum y^2 - 2 m sum y + n m^2: a bound needs no more than that, with a hair of slack for its rounding)
    const double m = a.mean_consts ? a.mean_consts[w.c0 + c] : 0.0, s2 = a.noise_vars[w.c0 + c];
    const double r2 = std::max(0.0, (sum_y2 - 2.0 * m * sum_y + (double)a.n * m * m)) * (1.0 + 1e-6) + 1e-6 * sum_y2;
    hpar[c] = 1.0 + r2 / s2;
    hpar[g + c] = m;
    hpar[2 * g + c] = s2;
    // (no noise, or a ratio beyond the double range: nothing bounds z.z -- such a candidate takes the lock-step schedule)
    w.skip[c] = !(s2 > 0.0) || !std::isfinite(hpar[c]);
    if (w.skip[c]) hpar[c] = 1.0;
  }
}

// a group that leaves most of the device idle gets a TEAM of workgroups per candidate (lml_wg.h: lml_team_kernel)
// (a timed-out hand-off costs ~0.1 s of polling plus the rebuilt group, and a slice sampler calls a hundred thousand
//  times: after one, the context's next 32 groups take one workgroup per candidate -- a shared device does not pay
//  the stall on every call; advisor, round 5)
int wg_pick_team(dfh_ctx* ctx, int g, int64_t nbt) {
  const int team_env = lml_switches().team;
  const bool team_cooling = ctx->lml_team_cooldown > 0;
  if (team_cooling) --ctx->lml_team_cooldown;
  int team = 1;
  if (team_env != 0 && !team_cooling) {
    const int cap = team_env > 0 ? team_env : 8;
    while (team * 2 <= cap && (int64_t)team * 2 * g <= ctx->n_cu && team * 2 <= nbt) team *= 2;
  }
  return team;
}

// Gram matrices, the launch with `team` workgroups per candidate, and the control block back in the pinned buffer
int wg_run_group(const LmlCall& a, const WgGroup& w, int team) {
  dfh_ctx* ctx = a.ctx;
  const int g = w.g;
  double* dpar = w.lay.dpar(w.blob);
  {
    SectionTimer t(ctx, DFH_T_KERNMAT);
    DFH_TRY(build_group_grams(ctx, w.kds, g, w.gs, a.dX, a.n, a.d, w.Xpb, w.Npb, dpar + 2 * g, a.noise_vars + w.c0, w.Kb, w.sK, w.NP));
  }
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    DFH_HIP(hipMemsetAsync(w.lay.dinfo(w.ctl), 0, w.lay.zeroed_bytes(team), ctx->stream));
    DFH_TRY(lml_wg_batch(ctx, w.Kb, w.sK, w.NP, a.n, g, w.labels.dy, dpar, w.ctl, w.lay.dinfo(w.ctl), team, w.lay.dstatus(w.ctl),
                         w.lay.dsync(w.ctl)));
  }
  DFH_HIP(hipMemcpyAsync(w.pinned + w.lay.back_off, w.ctl, w.lay.back_bytes, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// the group's results out; `redo` <- the candidates for the lock-step schedule
void wg_collect(const LmlCall& a, const WgGroup& w, std::vector<int>& redo) {
  const double* hred = w.lay.hred(w.pinned);
  const long long* hinfo = w.lay.hinfo(w.pinned);
  for (int c = 0; c < w.g; ++c) {
    if (w.skip[c] || hinfo[c] != 0 || !std::isfinite(hred[2 * c]) || !std::isfinite(hred[2 * c + 1])) { redo.push_back(w.c0 + c); continue; }
    if (a.jitter_powers) a.jitter_powers[w.c0 + c] = INT32_MIN;
    a.lml_out[w.c0 + c] = lml_value(hred[2 * c], hred[2 * c + 1], a.n);
  }
}

// descriptors and parameters of candidates c0 .. c0 + g staged in the pinned buffer and on their way up
int wg_stage_group(const LmlCall& a, WgGroup& w, int c0, int g) {
  dfh_ctx* ctx = a.ctx;
  w.c0 = c0; w.g = g; w.kds = a.kds + c0;
  w.gs = group_shape(w.kds, g);
  w.lay = WgGroupLayout(g, w.gs.blob_bytes);
  void* pinned = nullptr;
  DFH_TRY(pinned_get(ctx, w.lay.pinned_bytes(), &pinned));
  w.pinned = static_cast<char*>(pinned);
  DFH_TRY(scratch_get(ctx, SCR_AUG2, w.lay.up_bytes, &w.blob));
  DFH_TRY(kerndev_stage_many(a.kds + c0, g, w.pinned, w.blob, w.gs.blob_bytes));
  DFH_TRY(scratch_get(ctx, SCR_XS, (size_t)g * a.n * w.gs.Pmax * 8, (void**)&w.Xpb));
  DFH_TRY(scratch_get(ctx, SCR_XS2, (size_t)g * a.n * w.gs.parts_max * 8, (void**)&w.Npb));
  wg_fill_params(a, w);
  DFH_HIP(hipMemcpyAsync(w.blob, w.pinned, w.lay.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  return DFH_OK;
}

int lml_batch_wg(const LmlCall& a) {
  dfh_ctx* ctx = a.ctx;
  WgGroup w;
  w.nbt = (a.n + 1 + 63) / 64; w.NP = 64 * w.nbt; w.sK = w.NP * w.NP;
  const int wg_group = lml_switches().wg_group;
  const int64_t by_cu = wg_group > 0 ? wg_group : std::max(1, ctx->n_cu);
  const int G = (int)std::min<int64_t>(std::min<int64_t>(a.nb, by_cu), group_cap_by_memory(w.sK));
  DFH_TRY(resident_labels(ctx, a.y, a.n, a.flags, &w.labels));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)G * w.sK * 8, (void**)&w.Kb));
  DFH_TRY(scratch_get(ctx, SCR_LMLCTL, WgGroupLayout::control_bytes(G), (void**)&w.ctl));
  w.skip.assign((size_t)G, 0);
  std::vector<int> redo;                       // candidates for the lock-step schedule
  for (int c0 = 0; c0 < a.nb; c0 += G) {
    DFH_TRY(wg_stage_group(a, w, c0, std::min(G, a.nb - c0)));
    const int team = wg_pick_team(ctx, w.g, w.nbt);
    DFH_TRY(wg_run_group(a, w, team));
    if (team > 1 && w.lay.hstatus(w.pinned) != 0) {
      // a hand-off between the members of a team timed out (the device is shared, or not all of them were
      // resident): the matrices are rebuilt and every candidate gets ONE workgroup, which waits for nobody
      ++ctx->chol_fallbacks;
      ctx->lml_team_cooldown = 32;
      DFH_TRY(wg_run_group(a, w, 1));
    }
    wg_collect(a, w, redo);
  }
  for (int c : redo) DFH_TRY(redo_alone(a, c));
  return DFH_OK;
}

// ---- the routes that need no schedule ----

// a projection is per matrix (96 GEMM steps each, psdproj.hip): every candidate is a fit of its own, as the candidates
// that need the ladder are
int lml_each_psd(const LmlCall& a) {
  dfh_ctx* ctx = a.ctx;
  const int64_t n = a.n, d = a.d;
  std::vector<double> y_hold, yc((size_t)n);
  const double* y_host = nullptr;
  DFH_TRY(labels_on_host(ctx, a.y, n, a.flags, y_hold, &y_host));
  double* dXown = nullptr;       // (the fit stages y through the workspaces; X must not sit in one of them)
  DFH_TRY(dev_alloc(ctx, (size_t)n * d * 8, (void**)&dXown));
  int rc = DFH_OK;
  if (hipMemcpyAsync(dXown, a.dX, (size_t)n * d * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = DFH_ERR_HIP;
  for (int c = 0; c < a.nb && rc == DFH_OK; ++c) {
    const double mc = a.mean_consts ? a.mean_consts[c] : 0.0;
    for (int64_t i = 0; i < n; ++i) yc[(size_t)i] = y_host[i] - mc;
    dfh_gp* g = nullptr;
    rc = dfh_gp_fit(ctx, &a.descs[c], dXown, n, d, yc.data(), a.noise_vars[c], a.flags & (DFH_FIT_PSD_FLAGS | DFH_FIT_NO_JITTER), &g,
                    a.lml_out + c, a.jitter_powers ? a.jitter_powers + c : nullptr);
    if (g) dfh_gp_free(g);
  }
  dev_release(ctx, dXown);
  return rc;
}

// Fused or Tiny: every candidate in one launch; a fused candidate whose pivot failed (the ladder), or whose augmented
// pivot nothing bounds, is handed to the lock-step schedule on its own (the tiny kernels run the ladder themselves)
int lml_one_launch(const LmlCall& a, LmlRoute route) {
  dfh_ctx* ctx = a.ctx;
  std::vector<double> ld_dot((size_t)a.nb * 2), y_hold;
  std::vector<long long> info((size_t)a.nb, 0);
  const double* y_host = nullptr;
  DFH_TRY(labels_on_host(ctx, a.y, a.n, a.flags, y_hold, &y_host));
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    if (route == LmlRoute::Fused)
      DFH_TRY(lml_wg_fused_batch(ctx, a.kds, a.nb, a.dX, a.n, a.d, y_host, a.noise_vars, a.mean_consts, ld_dot.data(), info.data()));
    else
      DFH_TRY(lml_tiny_batch(ctx, a.kds, a.nb, a.dX, a.n, a.d, y_host, a.noise_vars, a.mean_consts, !(a.flags & DFH_FIT_NO_JITTER),
                             ld_dot.data(), a.jitter_powers));
  }
  for (int c = 0; c < a.nb; ++c) {
    if (info[c] != 0) { DFH_TRY(redo_alone(a, c)); continue; }
    if (route == LmlRoute::Fused && a.jitter_powers) a.jitter_powers[c] = INT32_MIN;
    a.lml_out[c] = lml_value(ld_dot[2 * c], ld_dot[2 * c + 1], a.n);
  }
  return DFH_OK;
}

}  // namespace

extern "C" int dfh_gp_lml_batch(dfh_ctx* ctx, const dfh_kernel_desc* descs, int32_t nb, const double* X,
                                int64_t n, int64_t d, const double* y, const double* mean_consts,
                                const double* noise_vars, int flags, double* lml_out,
                                int32_t* jitter_powers) {
  DFH_ARG(ctx && descs && nb >= 0 && X && y && noise_vars && lml_out && n >= 1 && d >= 1);
  if (nb == 0) return DFH_OK;
  for (int c = 0; c < nb; ++c) DFH_ARG(descs[c].dim == d);
  DFH_HIP(hipSetDevice(ctx->device));
  const double* dX = nullptr;
  if (flags & DFH_LML_X_IS_DEVICE) dX = X;
  else DFH_TRY(to_device(ctx, X, (size_t)n * d * 8, SCR_STAGE_A, &dX));
  std::vector<KernDev> kds((size_t)nb);        // host descriptors, built once: every route and a candidate's second try take slices
  for (int c = 0; c < nb; ++c) DFH_TRY(kerndev_build_host(&descs[c], &kds[c]));
  const LmlCall call = {ctx, descs, kds.data(), nb, dX, n, d, y, mean_consts, noise_vars, flags, lml_out, jitter_powers, 0};
  const LmlRoute route = lml_route(call);
  switch (route) {
    case LmlRoute::PsdEach: return lml_each_psd(call);
    case LmlRoute::Fused:
    case LmlRoute::Tiny: return lml_one_launch(call, route);
    case LmlRoute::Wg: return lml_batch_wg(call);
    case LmlRoute::Lockstep: break;
  }
  return lml_batch_lockstep(call);
}
