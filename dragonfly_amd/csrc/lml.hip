// The tuning objective, extern "C" dfh_gp_lml_batch: its dispatcher, the workgroup-per-candidate and lock-step schedules,
// and the kernels of the lock-step schedule's solve stage (the one-launch forms live in lml_tiny.hip and lml_wg.h).
#include "common.h"
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

// n <= CHOL_NB (one diagonal block): the whole solve stage of a candidate in one workgroup --
// yc = y - m, z = L^-1 yc through the explicit block inverse M (followed by steps[c] steps of
// iterative refinement against the clean copy Ld of the block, chol.hip: refine_steps), then
// out = {sum log L_ii, z . z}  (= yc . alpha: the backward solve is not needed).  blockIdx.x = candidate.
__global__ __launch_bounds__(256) void k_lml_finish_small(const double* __restrict__ inv, long sInv,
                                                          const double* __restrict__ y,
                                                          const double* __restrict__ means, int n,
                                                          const int* __restrict__ steps,
                                                          double* __restrict__ out2) {
  __shared__ double yc[CHOL_NB], z[CHOL_NB], r[CHOL_NB], red[8];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  inv += (long)c * sInv;
  const double* Ld = inv + CHOL_NB * CHOL_NB;                // clean copy of the factor (one block: nblk = 1)
  const double mean = means[c];
  const int nsteps = steps[c];
  for (int i = tid; i < n; i += 256) yc[i] = y[i] - mean;
  __syncthreads();
  // dst_i (+)= sum_{j <= i} A[i][j] src[j], a wave per row
  auto lower_mv = [&](const double* A, const double* src, double* dst, double sign, const double* base) {
    for (int i = wave; i < n; i += 4) {
      const double* row = A + (long)i * CHOL_NB;
      double s = 0.0;
      for (int j = lane; j <= i; j += 64) s = fma(row[j], src[j], s);
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) dst[i] = (base ? base[i] : 0.0) + sign * s;
    }
    __syncthreads();
  };
  lower_mv(inv, yc, z, 1.0, nullptr);                       // z = M yc
  for (int s = 0; s < nsteps; ++s) {
    lower_mv(Ld, z, r, -1.0, yc);                           // r = yc - L z
    lower_mv(inv, r, z, 1.0, z);                            // z += M r
  }
  // (y - m)^T alpha = ||L^-1 (y - m)||^2 = z . z: the backward solve is not needed for the likelihood
  double ld = 0.0, dt = 0.0;
  for (int j = tid; j < n; j += 256) {
    dt = fma(z[j], z[j], dt);
    ld += log(Ld[(long)j * CHOL_NB + j]);
  }
  for (int off = 32; off > 0; off >>= 1) { ld += __shfl_down(ld, off, 64); dt += __shfl_down(dt, off, 64); }
  if (lane == 0) { red[wave] = ld; red[4 + wave] = dt; }
  __syncthreads();
  if (tid == 0) {
    out2[2 * c] = (red[0] + red[1]) + (red[2] + red[3]);
    out2[2 * c + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// The same stage without the 512-block inverse: forward substitution over 64-blocks with the factor
// itself and the inverses of its 64 x 64 diagonal blocks (what trtri64_kernel leaves on the diagonal
// of the inverse buffer) -- z_b = Linv_bb (r_b - sum_{i<b} L_bi z_i).  Saves the inverse assembly
// (six GEMM launches) and its quality measurement per call; a 64-block inverse needs no refinement.
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

// the switches that more than one place consults, read when the library is loaded
const bool small64_on = env_flag("DFH_LML_SMALL64", true);     // n <= 512: substitution with 64-block inverses, no 512-block inverse
const double group_gib_env = env_double("DFH_LML_GROUP_GIB", 8.0);
const double group_gib = group_gib_env > 0.0 ? group_gib_env : 8.0;   // Gram matrices of one group of candidates

// the arguments of dfh_gp_lml_batch, X resolved to the device; cand_base: index of descs[0] in the caller's list (error messages)
struct LmlCall {
  dfh_ctx* ctx; const dfh_kernel_desc* descs; int32_t nb; const double* dX; int64_t n, d; const double* y;
  const double* mean_consts; const double* noise_vars; int flags; double* lml_out; int32_t* jitter_powers;
  int cand_base;
};

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

// kds[0..g) <- the host descriptors of descs[c0..c0+g)
int stage_group(const dfh_kernel_desc* descs, int c0, int g, std::vector<KernDev>& kds, GroupShape& gs) {
  gs = GroupShape();
  for (int c = 0; c < g; ++c) {
    kds[c] = KernDev();
    DFH_TRY(kerndev_build_host(&descs[c0 + c], &kds[c]));
    gs.Pmax = std::max<int64_t>(gs.Pmax, kds[c].P);
    gs.parts_max = std::max<int64_t>(gs.parts_max, kds[c].n_parts);
    gs.blob_bytes += kerndev_blob_bytes(kds[c]);
    gs.uniform = gs.uniform && !kds[c].multi && kds[c].n_parts == 1 && kds[c].P == kds[0].P &&
                 kerndev_blob_bytes(kds[c]) == kerndev_blob_bytes(kds[0]);
  }
  return DFH_OK;
}

// K + noise_var * I (gp_core.py:843) of the g staged candidates, candidate c at K + c * sK with row stride ldK: a uniform
// group in one pack and one Gram launch (noise d_noise[c], on the device), otherwise candidate by candidate (h_noise[c])
int build_group_grams(dfh_ctx* ctx, const std::vector<KernDev>& kds, int g, const GroupShape& gs, const double* dX,
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

// The lock-step schedule: groups of up to CHOL_MAX_BATCH candidates through the batched cholesky_device (any n)
int lml_batch_lockstep(const LmlCall& a) {
  dfh_ctx* ctx = a.ctx;
  const int32_t nb = a.nb;
  const int64_t n = a.n, NB = CHOL_NB;
  const int64_t nblk = (n + NB - 1) / NB;
  const int64_t ldK = (n + 1) & ~(int64_t)1;                 // even leading dimension: 16-byte row starts
  const int64_t strideK = n * ldK, strideInv = inv_buffer_doubles(n);
  // group size: up to CHOL_MAX_BATCH matrices and (DFH_LML_GROUP_GIB, default 8) GiB of Gram
  // matrices at a time.  Measured ms per candidate at 2 / 8 GiB: n=4096 1.55 / 1.07, n=16384
  // 42.6 (one at a time) / 30.0 (four in lock-step: the panel chains of the four interleave).
  const int64_t by_mem = std::max<int64_t>(1, (int64_t)(group_gib * 1073741824.0 / ((double)strideK * 8.0)));
  const int G = (int)std::min<int64_t>(std::min<int64_t>(nb, CHOL_MAX_BATCH), by_mem);
  std::vector<KernDev> kds((size_t)G);       // device images live in one scratch blob: nothing to free
  const double* dy = nullptr;
  DFH_TRY(to_device(ctx, a.y, (size_t)n * 8, SCR_STAGE_B, &dy));
  double *Kb = nullptr, *invb = nullptr, *vecs = nullptr, *red = nullptr, *dpar = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)G * strideK * 8, (void**)&Kb));
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)G * strideInv * 8, (void**)&invb));
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)G * n * 8 * 2, (void**)&vecs));
  DFH_TRY(scratch_get(ctx, SCR_OUT2, (size_t)std::max(256, G * 16), (void**)&red));   // SCR_RED belongs to the gemv partials
  DFH_TRY(scratch_get(ctx, SCR_OUT, (size_t)std::max(256, G * 24), (void**)&dpar));   // per candidate {noise, mean}, then int steps
  std::vector<double> hred((size_t)G * 2), hpar((size_t)G * 2);
  std::vector<int> refine((size_t)G * nblk, 0);           // refinement steps per candidate and diagonal block
  for (int c0 = 0; c0 < nb; c0 += G) {
    const int g = std::min(G, nb - c0);
    GroupShape gs;
    DFH_TRY(stage_group(a.descs, c0, g, kds, gs));
    void* blob = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_AUG2, gs.blob_bytes, &blob));
    DFH_TRY(kerndev_upload_many(ctx, kds.data(), g, blob, gs.blob_bytes));
    double *Xpb = nullptr, *Npb = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_XS, (size_t)g * n * gs.Pmax * 8, (void**)&Xpb));
    DFH_TRY(scratch_get(ctx, SCR_XS2, (size_t)g * n * gs.parts_max * 8, (void**)&Npb));
    const int64_t sXp = n * gs.Pmax, sNp = n * gs.parts_max;
    for (int c = 0; c < g; ++c) {
      hpar[c] = a.noise_vars[c0 + c];
      hpar[g + c] = a.mean_consts ? a.mean_consts[c0 + c] : 0.0;
    }
    DFH_HIP(hipMemcpyAsync(dpar, hpar.data(), (size_t)g * 16, hipMemcpyHostToDevice, ctx->stream));
    auto build_M = [&](int c) -> int {           // K + noise_var * I again, from the packed inputs (a failed factorisation destroys it)
      double* Xp = Xpb + c * sXp; double* Np = Npb + c * sNp;
      return kernmat_gram(ctx, kds[c], 0, kds[c].n_parts, true, KmPts{Xp, Np, n}, a.noise_vars[c0 + c], Kb + c * strideK,
                          ldK);
    };
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_TRY(build_group_grams(ctx, kds, g, gs, a.dX, n, a.d, Xpb, Npb, dpar, a.noise_vars + c0, Kb, strideK, ldK));
    }
    {
      SectionTimer t(ctx, DFH_T_CHOL);
      int64_t piv[CHOL_MAX_BATCH] = {0};
      // n <= 512: the finish kernel substitutes with 64-blocks, so the 512-block inverse is not built
      const bool inv64_only = small64_on && n <= NB;
      const std::function<int()> rebuild_all = [&]() -> int {
        for (int c = 0; c < g; ++c) DFH_TRY(build_M(c));
        return DFH_OK;
      };
      int rc = cholesky_device(ctx, Kb, n, ldK, invb, piv, g, strideK, strideInv, refine.data(), inv64_only, &rebuild_all);
      if (rc != DFH_OK && rc != DFH_ERR_NOT_PD) return rc;
      for (int c = 0; c < g; ++c) {
        if (a.jitter_powers) a.jitter_powers[c0 + c] = INT32_MIN;
        if (piv[c] == 0) continue;
        if (a.flags & DFH_FIT_NO_JITTER) {
          dfh_set_error("Matrix is not positive definite (candidate %d, pivot %lld)", a.cand_base + c0 + c, (long long)piv[c]);
          return DFH_ERR_NOT_PD;
        }
        auto rebuild = [&]() -> int { return build_M(c); };
        DFH_TRY(rebuild());
        int32_t jp = INT32_MIN;
        DFH_TRY(stable_cholesky_device(ctx, Kb + c * strideK, n, invb + c * strideInv, true, rebuild, &jp, nullptr, ldK,
                                       refine.data() + (size_t)c * nblk));
        if (a.jitter_powers) a.jitter_powers[c0 + c] = jp;
      }
    }
    {
      SectionTimer t(ctx, DFH_T_SOLVE);
      if (n <= NB && small64_on) {
        // (a candidate that went through the jitter ladder has the full inverse in its slot: its diagonal
        //  64-blocks are the inverses of the factor's diagonal blocks all the same)
        hipLaunchKernelGGL(k_lml_finish_small64, dim3((unsigned)g), dim3(256), 0, ctx->stream, Kb, (long)strideK, (long)ldK,
                           invb, (long)strideInv, dy, dpar + g, (int)n, red);
        DFH_LAUNCH_CHECK();
      } else if (n <= NB) {
        // one block per candidate (nblk = 1): its refinement steps ride behind {noise, mean} in dpar
        int* dsteps = reinterpret_cast<int*>(dpar + 2 * g);
        DFH_HIP(hipMemcpyAsync(dsteps, refine.data(), (size_t)g * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_lml_finish_small, dim3((unsigned)g), dim3(256), 0, ctx->stream, invb, (long)strideInv,
                           dy, dpar + g, (int)n, dsteps, red);
        DFH_LAUNCH_CHECK();
      } else {
        bool any_refine = false;
        for (size_t i = 0; i < (size_t)g * nblk; ++i) any_refine = any_refine || refine[i] > 0;
        static const bool batch_solve = env_flag("DFH_LML_BATCH_SOLVE", true);
        if (!any_refine && batch_solve) {
          // all candidates per launch: r = y - m; for each 512-block z_b = M_b r_b, r_below -= L[below, b] z_b
          const long sv = 2 * (long)n;                 // candidate c: r at vecs + c*sv, z behind it
          hipLaunchKernelGGL(k_centre_batch, dim3((unsigned)((n + 255) / 256), (unsigned)g), dim3(256), 0, ctx->stream, dy,
                             dpar + g, vecs, (long)n);
          DFH_LAUNCH_CHECK();
          for (int64_t b0 = 0; b0 < n; b0 += NB) {
            const int64_t w = std::min<int64_t>(NB, n - b0), below = n - b0 - w;
            hipLaunchKernelGGL(k_gemv_rows_wave_batch, dim3((unsigned)((w + 3) / 4), (unsigned)g), dim3(256), 0, ctx->stream,
                               invb + (b0 / NB) * NB * NB, (long)strideInv, (long)w, (long)w, (long)NB, vecs + b0, sv, 1.0,
                               (const double*)nullptr, 0.0, vecs + n + b0, sv);
            DFH_LAUNCH_CHECK();
            if (below > 0) {
              hipLaunchKernelGGL(k_gemv_rows_wave_batch, dim3((unsigned)((below + 3) / 4), (unsigned)g), dim3(256), 0,
                                 ctx->stream, Kb + (b0 + w) * ldK + b0, (long)strideK, (long)below, (long)w, (long)ldK,
                                 vecs + n + b0, sv, -1.0, vecs + b0 + w, 1.0, vecs + b0 + w, sv);
              DFH_LAUNCH_CHECK();
            }
          }
          hipLaunchKernelGGL(k_logdet_sumsq_batch, dim3((unsigned)g), dim3(256), 0, ctx->stream, Kb, (long)strideK, (long)n,
                             (long)ldK, vecs + n, sv, red);
          DFH_LAUNCH_CHECK();
        } else {
          for (int c = 0; c < g; ++c) {
            double* yc = vecs + (int64_t)c * 2 * n;
            double* alpha = yc + n;
            hipLaunchKernelGGL(k_centre, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dy, hpar[g + c], yc, alpha, (long)n);
            DFH_LAUNCH_CHECK();
            // alpha = L^T \ (L \ (y - m))      (gp_core.py:161-163)
            DFH_TRY(trsv_both(ctx, Kb + c * strideK, n, ldK, invb + c * strideInv, alpha, refine.data() + (size_t)c * nblk));
            DFH_TRY(logdet_and_dot_device(ctx, Kb + c * strideK, n, ldK, yc, alpha, red + 2 * c));
          }
        }
      }
      DFH_HIP(hipMemcpyAsync(hred.data(), red, (size_t)g * 16, hipMemcpyDeviceToHost, ctx->stream));
      DFH_HIP(hipStreamSynchronize(ctx->stream));
      for (int c = 0; c < g; ++c) a.lml_out[c0 + c] = lml_value(hred[2 * c], hred[2 * c + 1], n);
    }
  }
  return DFH_OK;
}

// candidate c of the call takes the lock-step schedule by itself (which runs the stable_cholesky ladder as a single fit would)
int redo_alone(const LmlCall& a, int c) {
  LmlCall one = a;
  one.descs += c; one.nb = 1; one.noise_vars += c; one.lml_out += c; one.cand_base += c;
  if (one.mean_consts) one.mean_consts += c;
  if (one.jitter_powers) one.jitter_powers += c;
  return lml_batch_lockstep(one);
}

// One workgroup per candidate (lml_wg.h: lml_wg_kernel), 128 < n <= LMLWG_MAX_N: per group of up to one candidate
// per CU three launches -- pack, Gram matrices, factor + forward solve + reductions -- and one copy back.  A
// candidate whose matrix does not factor as it stands (or whose augmented pivot fails) is handed to the
// lock-step schedule on its own, which runs the stable_cholesky ladder exactly as before.
int lml_batch_wg(const LmlCall& a) {
  dfh_ctx* ctx = a.ctx;
  const int32_t nb = a.nb;
  const int64_t n = a.n;
  const double* y = a.y;
  const int64_t nbt = (n + 1 + 63) / 64, NP = 64 * nbt, sK = NP * NP;
  static const int group_env = env_int("DFH_LML_WG_GROUP", 0), group_max = group_env > 0 ? group_env : 0;
  const int64_t by_mem = std::max<int64_t>(1, (int64_t)(group_gib * 1073741824.0 / ((double)sK * 8.0)));
  const int64_t by_cu = group_max > 0 ? group_max : std::max(1, ctx->n_cu);
  const int G = (int)std::min<int64_t>(std::min<int64_t>(nb, by_cu), by_mem);
  // The labels stay resident between calls (round 6): a fitter asks thousands of times with the same y, and staging
  // 16 KB of pageable memory per call -- copy, synchronise -- was a sixth of a small group's call.  Host labels are
  // compared with the copy of the last call (memcmp: exact); device labels are used where they are.
  const double* dy = nullptr;
  double sum_y = 0.0, sum_y2 = 0.0;
  std::vector<double> y_hold;
  const double* y_host = nullptr;
  DFH_TRY(labels_on_host(ctx, y, n, a.flags, y_hold, &y_host));
  if (!y_hold.empty()) {                       // device labels, downloaded for their sums
    dy = y;
    for (int64_t i = 0; i < n; ++i) { sum_y += y_host[i]; sum_y2 = fma(y_host[i], y_host[i], sum_y2); }
  } else {
    double* ybuf = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_YCACHE, (size_t)std::max<int64_t>(2048, n) * 8, (void**)&ybuf));
    if (ybuf != ctx->ycache_dev || ctx->ycache_host.size() != (size_t)n ||
        std::memcmp(ctx->ycache_host.data(), y, (size_t)n * 8) != 0) {
      ctx->ycache_host.assign(y, y + n);
      DFH_HIP(hipMemcpyAsync(ybuf, ctx->ycache_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
      DFH_HIP(hipStreamSynchronize(ctx->stream));
      ctx->ycache_dev = ybuf;
      double s1 = 0.0, s2 = 0.0;
      for (int64_t i = 0; i < n; ++i) { s1 += y[i]; s2 = fma(y[i], y[i], s2); }
      ctx->ycache_sum = s1; ctx->ycache_sum2 = s2;
    }
    dy = ybuf;
    sum_y = ctx->ycache_sum; sum_y2 = ctx->ycache_sum2;
  }
  // One control block per group on the device -- results [2 g] | failed pivots [g] | status [1] | team flags -- zeroed by
  // ONE memset and copied back by ONE copy into the pinned buffer; descriptors and {aug. diagonal, mean, noise} go up
  // from the pinned buffer in ONE copy.  (Round 5: three pageable copies up, three memsets, three pageable copies
  // back and three synchronisations per group -- 160 of a small group's 210 us, profiles/r06_small_calls.txt.)
  double *Kb = nullptr, *ctl = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)G * sK * 8, (void**)&Kb));
  const size_t ctl_bytes = (size_t)(3 * G + 8) * 8 + (size_t)G * LMLT_SYNC_INTS * sizeof(int);
  DFH_TRY(scratch_get(ctx, SCR_LMLCTL, ctl_bytes, (void**)&ctl));
  std::vector<KernDev> kds((size_t)G);
  std::vector<char> skip((size_t)G, 0);
  // DFH_LML_TEAM: 0 = never a team, N = teams of up to N workgroups (default: up to 8)
  static const int team_env = env_int("DFH_LML_TEAM", -1);
  std::vector<int> redo;                       // candidates for the lock-step schedule
  for (int c0 = 0; c0 < nb; c0 += G) {
    const int g = std::min(G, nb - c0);
    GroupShape gs;
    DFH_TRY(stage_group(a.descs, c0, g, kds, gs));
    // pinned: descriptors | {aug. diagonal, mean, noise} [3 g] | (64-byte aligned) what comes back [3 g + 1]
    const size_t up_par = (gs.blob_bytes + 15) & ~size_t(15), up_bytes = up_par + (size_t)g * 24;
    const size_t back_off = (up_bytes + 63) & ~size_t(63), back_bytes = (size_t)(3 * g + 1) * 8;
    void* pinned = nullptr;
    DFH_TRY(pinned_get(ctx, back_off + back_bytes, &pinned));
    char* hup = static_cast<char*>(pinned);
    double* hpar = reinterpret_cast<double*>(hup + up_par);
    const double* hred = reinterpret_cast<const double*>(hup + back_off);
    const long long* hinfo = reinterpret_cast<const long long*>(hup + back_off) + 2 * g;
    const unsigned long long* hstatus_p = reinterpret_cast<const unsigned long long*>(hup + back_off) + 3 * g;
    void* blob = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_AUG2, up_bytes, &blob));
    DFH_TRY(kerndev_stage_many(kds.data(), g, hup, blob, gs.blob_bytes));
    double* dpar = reinterpret_cast<double*>(static_cast<char*>(blob) + up_par);
    double* red = ctl;
    long long* dinfo = reinterpret_cast<long long*>(ctl + 2 * g);
    unsigned long long* d_status = reinterpret_cast<unsigned long long*>(ctl + 3 * g);
    int* d_sync = reinterpret_cast<int*>(ctl + 3 * g + 1);
    double *Xpb = nullptr, *Npb = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_XS, (size_t)g * n * gs.Pmax * 8, (void**)&Xpb));
    DFH_TRY(scratch_get(ctx, SCR_XS2, (size_t)g * n * gs.parts_max * 8, (void**)&Npb));
    for (int c = 0; c < g; ++c) {
      // the augmented row's diagonal entry: c = 1 + |y - m|^2 / s2 > z.z (the eigenvalues of K + s2 I are >= s2)
      // (|y - m|^2 = sum y^2 - 2 m sum y + n m^2: a bound needs no more than that, with a hair of slack for its rounding)
      const double m = a.mean_consts ? a.mean_consts[c0 + c] : 0.0, s2 = a.noise_vars[c0 + c];
      const double r2 = std::max(0.0, (sum_y2 - 2.0 * m * sum_y + (double)n * m * m)) * (1.0 + 1e-6) + 1e-6 * sum_y2;
      hpar[c] = 1.0 + r2 / s2;
      hpar[g + c] = m;
      hpar[2 * g + c] = s2;
      // (no noise, or a ratio beyond the double range: nothing bounds z.z -- such a candidate takes the lock-step schedule)
      skip[c] = !(s2 > 0.0) || !std::isfinite(hpar[c]);
      if (skip[c]) hpar[c] = 1.0;
    }
    DFH_HIP(hipMemcpyAsync(blob, hup, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    // a group that leaves most of the device idle gets a TEAM of workgroups per candidate (lml_wg.h: lml_team_kernel)
    int team = 1;
    // (a timed-out hand-off costs ~0.1 s of polling plus the rebuilt group, and a slice sampler calls a hundred thousand
    //  times: after one, the context's next 32 groups take one workgroup per candidate -- a shared device does not pay
    //  the stall on every call; advisor, round 5)
    const bool team_cooling = ctx->lml_team_cooldown > 0;
    if (team_cooling) --ctx->lml_team_cooldown;
    if (team_env != 0 && !team_cooling) {
      const int cap = team_env > 0 ? team_env : 8;
      while (team * 2 <= cap && (int64_t)team * 2 * g <= ctx->n_cu && team * 2 <= nbt) team *= 2;
    }
    auto run_group = [&](int tm) -> int {
      {
        SectionTimer t(ctx, DFH_T_KERNMAT);
        DFH_TRY(build_group_grams(ctx, kds, g, gs, a.dX, n, a.d, Xpb, Npb, dpar + 2 * g, a.noise_vars + c0, Kb, sK, NP));
      }
      {
        SectionTimer t(ctx, DFH_T_CHOL);
        // failed pivots, status and the team's flags: one memset (the results in front of them are always written)
        DFH_HIP(hipMemsetAsync(dinfo, 0, (size_t)(g + 1) * 8 + (tm > 1 ? (size_t)g * LMLT_SYNC_INTS * sizeof(int) : 0),
                               ctx->stream));
        DFH_TRY(lml_wg_batch(ctx, Kb, sK, NP, n, g, dy, dpar, red, dinfo, tm, d_status, d_sync));
      }
      DFH_HIP(hipMemcpyAsync(hup + back_off, ctl, back_bytes, hipMemcpyDeviceToHost, ctx->stream));
      DFH_HIP(hipStreamSynchronize(ctx->stream));
      return DFH_OK;
    };
    DFH_TRY(run_group(team));
    if (team > 1 && *hstatus_p != 0) {
      // a hand-off between the members of a team timed out (the device is shared, or not all of them were
      // resident): the matrices are rebuilt and every candidate gets ONE workgroup, which waits for nobody
      ++ctx->chol_fallbacks;
      ctx->lml_team_cooldown = 32;
      DFH_TRY(run_group(1));
    }
    for (int c = 0; c < g; ++c) {
      if (skip[c] || hinfo[c] != 0 || !std::isfinite(hred[2 * c]) || !std::isfinite(hred[2 * c + 1])) { redo.push_back(c0 + c); continue; }
      if (a.jitter_powers) a.jitter_powers[c0 + c] = INT32_MIN;
      a.lml_out[c0 + c] = lml_value(hred[2 * c], hred[2 * c + 1], n);
    }
  }
  for (int c : redo) DFH_TRY(redo_alone(a, c));
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
  std::vector<double> y_hold;                  // the labels, when a route wants them on the host and they are not
  const double* y_host = nullptr;
  if (flags & DFH_FIT_PSD_FLAGS) {
    // a projection is per matrix (96 GEMM steps each, psdproj.hip): every candidate is a fit of its own, as the
    // candidates that need the ladder are
    DFH_TRY(labels_on_host(ctx, y, n, flags, y_hold, &y_host));
    std::vector<double> yc((size_t)n);
    double* dXown = nullptr;       // (the fit stages y through the workspaces; X must not sit in one of them)
    DFH_TRY(dev_alloc(ctx, (size_t)n * d * 8, (void**)&dXown));
    int rc = DFH_OK;
    if (hipMemcpyAsync(dXown, dX, (size_t)n * d * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = DFH_ERR_HIP;
    for (int c = 0; c < nb && rc == DFH_OK; ++c) {
      const double mc = mean_consts ? mean_consts[c] : 0.0;
      for (int64_t i = 0; i < n; ++i) yc[(size_t)i] = y_host[i] - mc;
      dfh_gp* g = nullptr;
      rc = dfh_gp_fit(ctx, &descs[c], dXown, n, d, yc.data(), noise_vars[c], flags & (DFH_FIT_PSD_FLAGS | DFH_FIT_NO_JITTER), &g,
                      lml_out + c, jitter_powers ? jitter_powers + c : nullptr);
      if (g) dfh_gp_free(g);
    }
    dev_release(ctx, dXown);
    return rc;
  }
  const LmlCall call = {ctx, descs, nb, dX, n, d, y, mean_consts, noise_vars, flags, lml_out, jitter_powers, 0};
  static const bool tiny_enabled = env_flag("DFH_LML_TINY", true);
  const bool fused_range = tiny_enabled && n > TINY64_MAX_N && n <= 255 && nb <= 64;
  const bool tiny_range = tiny_enabled && n <= TINY_MAX_N;
  if (fused_range || tiny_range) {
    // host descriptors of every candidate, for the one-launch forms (gone again before the other schedules stage theirs)
    std::vector<KernDev> all((size_t)nb);
    for (int c = 0; c < nb; ++c) DFH_TRY(kerndev_build_host(&descs[c], &all[c]));
    if (fused_range && lml_wg_fused_applies(all.data(), nb, n)) {
      // a handful of mid-sized candidates (a slice sampler's call at 64 <= n <= 128): Gram matrix, factorisation and
      // forward solve of each in ONE launch by one workgroup, nothing copied (lml_wg.h: lml_wgf_kernel)
      std::vector<double> ld_dot((size_t)nb * 2);
      std::vector<long long> info((size_t)nb);
      DFH_TRY(labels_on_host(ctx, y, n, flags, y_hold, &y_host));
      {
        SectionTimer t(ctx, DFH_T_CHOL);
        DFH_TRY(lml_wg_fused_batch(ctx, all.data(), nb, dX, n, d, y_host, noise_vars, mean_consts, ld_dot.data(), info.data()));
      }
      for (int c = 0; c < nb; ++c) {
        if (info[c] != 0) {        // a failed pivot (the ladder) or no bound on the augmented pivot
          DFH_TRY(redo_alone(call, c));
          continue;
        }
        if (jitter_powers) jitter_powers[c] = INT32_MIN;
        lml_out[c] = lml_value(ld_dot[2 * c], ld_dot[2 * c + 1], n);
      }
      return DFH_OK;
    }
    if (tiny_range && lml_tiny_applies(all.data(), nb, n)) {
      // small problems: pack, Gram matrix, stable_cholesky and the solve of every candidate in ONE
      // launch (lml_tiny.hip: k_lml_tiny)
      std::vector<double> ld_dot((size_t)nb * 2);
      DFH_TRY(labels_on_host(ctx, y, n, flags, y_hold, &y_host));
      SectionTimer t(ctx, DFH_T_CHOL);
      DFH_TRY(lml_tiny_batch(ctx, all.data(), nb, dX, n, d, y_host, noise_vars, mean_consts,
                             !(flags & DFH_FIT_NO_JITTER), ld_dot.data(), jitter_powers));
      for (int c = 0; c < nb; ++c) lml_out[c] = lml_value(ld_dot[2 * c], ld_dot[2 * c + 1], n);
      return DFH_OK;
    }
  }
  // one workgroup per candidate up to n = 2047 (DFH_LML_WG=0: the lock-step schedule for every n)
  static const int wg_min_batch = env_int("DFH_LML_WG_MIN_BATCH", 1);
  static const bool wg_enabled = env_flag("DFH_LML_WG", true);
  if (wg_enabled && n <= LMLWG_MAX_N && nb >= wg_min_batch) return lml_batch_wg(call);
  return lml_batch_lockstep(call);
}
