// extern "C" entry points of libdfhip.so (see include/dfhip.h for the contract and the
// reference functions each one replaces) and the GP object that lives in HBM.
#include "common.h"
#include <cstring>
#include <math.h>
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <stdlib.h>

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
  bool upper_zeroed = false;
  bool gram = false;             // built from a host-evaluated Gram matrix: no kernel, no packed inputs
  int psd_flags = 0;             // DFH_FIT_PROJECT_FIRST / DFH_FIT_TRY_BEFORE_PROJECT the fit ran under (L is not chol(K + noise I) of the kernel's K)
};

namespace {

int64_t pick_chunk(dfh_ctx* ctx, int64_t n, int64_t m) {
  // candidate rows per posterior chunk: the m_c x n cross matrix (solved in place into V^T) is sized
  // for a 288 GB part -- DFH_CHUNK_GIB (32) GiB, two of them alive in the pipelined Thompson
  // sampling.  Measured on the bench step (n = 16384, 262144 candidates, TS blocks factored in
  // lock-step batches of DFH_TS_BATCH): 4 GiB / 8 blocks 1434 ms, 8 GiB / 16 1403-1412, 16 GiB / 32
  // 1397, 32 GiB / 64 1389 -- bigger chunks mean taller TRSM products (1048 -> 1021 ms) and more
  // Thompson blocks per latency-bound factorisation chain (332 -> 310 ms).
  // The cap is per CONTEXT (its device, and whoever else is on it): an eighth of what was free on the
  // context's device when the context first asked, plus what the context's own scratch pool already
  // held then -- not an eighth of the first device's total memory for the whole process.
  static const double chunk_env = env_double("DFH_CHUNK_GIB", 32.0), chunk_gib = chunk_env > 0.0 ? chunk_env : 32.0;
  if (ctx->chunk_cap_gib <= 0.0) {
    size_t f = 0, t = 0;
    double cap = 36.0;
    if (hipMemGetInfo(&f, &t) == hipSuccess) {
      size_t own = 0;
      for (const DevBuf& b : ctx->scratch) own += b.bytes;
      cap = (double)(f + own) / 8.0 / 1073741824.0;
    } else {
      (void)hipGetLastError();
    }
    ctx->chunk_cap_gib = cap > 0.25 ? cap : 0.25;
  }
  const double gib = chunk_gib < ctx->chunk_cap_gib ? chunk_gib : ctx->chunk_cap_gib;
  int64_t mc = (int64_t)(gib * (double)(1LL << 27)) / (n > 0 ? n : 1);
  mc = std::max<int64_t>(512, std::min<int64_t>(mc, 262144));
  mc = (mc / 512) * 512;
  if (mc > m) mc = m;
  return mc;
}

// numpy argmax ordering: a NaN beats everything, earlier index wins ties
__device__ __forceinline__ bool better(double va, long ia, double vb, long ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) {
    if (na && nb) return ia < ib;
    return na;
  }
  if (va > vb) return true;
  if (va < vb) return false;
  return ia < ib;
}

__global__ void k_argmax_stage1(const double* __restrict__ v, long m, long idx_base,
                                double* __restrict__ pv, long* __restrict__ pi) {
  __shared__ double sv[256];
  __shared__ long si[256];
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long)gridDim.x * blockDim.x) {
    const double x = v[i];
    if (bi == LONG_MAX || better(x, idx_base + i, bv, bi)) { bv = x; bi = idx_base + i; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { pv[blockIdx.x] = sv[0]; pi[blockIdx.x] = si[0]; }
}

__global__ void k_argmax_stage2(const double* pv, const long* pi, int nparts, double* out_v, long* out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  double bv = -INFINITY; long bi = LONG_MAX;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    if (pi[i] != LONG_MAX && (bi == LONG_MAX || better(pv[i], pi[i], bv, bi))) { bv = pv[i]; bi = pi[i]; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[0] = sv[0]; out_i[0] = si[0]; }
}

// One workgroup per segment [off[g], off[g+1]) of v: its arg-max (np.argmax rule, index local to the segment)
__global__ void k_argmax_segments(const double* __restrict__ v, const long* __restrict__ off,
                                  double* __restrict__ out_v, long* __restrict__ out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const long lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double x = v[i];
    if (bi == LONG_MAX || better(x, i - lo, bv, bi)) { bv = x; bi = i - lo; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[blockIdx.x] = sv[0]; out_i[blockIdx.x] = si[0]; }
}

bool host_better(double va, int64_t ia, double vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) { if (na && nb) return ia < ib; return na; }
  if (va > vb) return true;
  if (va < vb) return false;
  return ia < ib;
}

// arg-max of v[0..m) (device), indices offset by idx_base; merges into host running best
int argmax_update(dfh_ctx* ctx, const double* v, int64_t m, int64_t idx_base, bool* have,
                  double* best_v, int64_t* best_i) {
  if (m <= 0) return DFH_OK;
  const int nblocks = (int)std::min<int64_t>(1024, (m + 255) / 256);
  char* buf = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)(nblocks + 1) * 16 + 64, (void**)&buf));
  double* pv = reinterpret_cast<double*>(buf);
  long* pi = reinterpret_cast<long*>(buf + (size_t)(nblocks + 1) * 8);
  hipLaunchKernelGGL(k_argmax_stage1, dim3(nblocks), dim3(256), 0, ctx->stream, v, (long)m, (long)idx_base, pv, pi);
  DFH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_argmax_stage2, dim3(1), dim3(256), 0, ctx->stream, pv, pi, nblocks, pv + nblocks, pi + nblocks);
  DFH_LAUNCH_CHECK();
  double hv; long hi;
  DFH_HIP(hipMemcpyAsync(&hv, pv + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipMemcpyAsync(&hi, pi + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  if (!*have || host_better(hv, (int64_t)hi, *best_v, *best_i)) { *best_v = hv; *best_i = (int64_t)hi; *have = true; }
  return DFH_OK;
}

// arg-max of every row of v [rows x ld] (np.argmax rule, index local to the row): one workgroup per row
__global__ void k_argmax_rows(const double* __restrict__ v, long ld, long m, double* __restrict__ out_v,
                              long* __restrict__ out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const double* r = v + (long)blockIdx.x * ld;
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = threadIdx.x; i < m; i += blockDim.x) {
    const double x = r[i];
    if (bi == LONG_MAX || better(x, i, bv, bi)) { bv = x; bi = i; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[blockIdx.x] = sv[0]; out_i[blockIdx.x] = si[0]; }
}

// S joint draws of one Thompson block in one launch: out[s][i] = mu[i] + sum_{j <= i} L[i][j] Ut[s][j], L the B x B lower
// factor (row-major; its strict upper triangle holds stale covariance and is never read), Ut the block's normals
// sample-major (row s at s * ldu).  One 256-thread workgroup per (tile of DRAW_TILE draws, row of L): the row is read
// once per tile, each element multiplied into the tile's DRAW_TILE accumulator pairs, and the tiles of a row are
// neighbours in the grid, so all but the first find the row in L2.  Per draw the arithmetic is k_gemv_rows' with
// tri_lower (runtime.hip) operation for operation -- the thread's strided fma chain (even / odd elements apart when
// `vec`, the condition under which that kernel takes its double2 path), the wave's shuffle tree, the four wave sums as
// (w0 + w1) + (w2 + w3), then + mu -- so draw s is bit for bit the single draw with column s of the normals.
#define DRAW_TILE 8
__global__ __launch_bounds__(256) void k_tri_draw(const double* __restrict__ L, long B, const double* __restrict__ Ut,
                                                  long ldu, int S, const double* __restrict__ mu,
                                                  double* __restrict__ out, long ldo, int vec) {
  __shared__ double sm[DRAW_TILE][4];
  const long row = blockIdx.y;
  const int s_lo = (int)blockIdx.x * DRAW_TILE;
  const int nt = S - s_lo < DRAW_TILE ? S - s_lo : DRAW_TILE;
  const double* a = L + row * B;
  const long n = row + 1;                                   // only columns j <= row
  const double* x[DRAW_TILE];                               // a short tile repeats its last draw: no branch in the loop
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) x[t] = Ut + (long)(s_lo + (t < nt ? t : nt - 1)) * ldu;
  double s0[DRAW_TILE], s1[DRAW_TILE];
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) { s0[t] = 0.0; s1[t] = 0.0; }
  if (vec) {
    const bool x2 = ((reinterpret_cast<uintptr_t>(Ut) & 15) == 0) && ((ldu & 1) == 0);
    const long n2 = n >> 1;
    for (long j = threadIdx.x; j < n2; j += 256) {
      const double2_t av = reinterpret_cast<const double2_t*>(a)[j];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) {
        double2_t xv;
        if (x2) xv = reinterpret_cast<const double2_t*>(x[t])[j];
        else { xv.x = x[t][2 * j]; xv.y = x[t][2 * j + 1]; }
        s0[t] = fma(av.x, xv.x, s0[t]);
        s1[t] = fma(av.y, xv.y, s1[t]);
      }
    }
    if ((n & 1) && threadIdx.x == 0) {
      const double al = a[n - 1];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) s0[t] = fma(al, x[t][n - 1], s0[t]);
    }
  } else {
    for (long j = threadIdx.x; j < n; j += 256) {
      const double aj = a[j];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) s0[t] = fma(aj, x[t][j], s0[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) {
    double s = s0[t] + s1[t];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sm[t][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < nt) {
    const int t = threadIdx.x;
    const double v = (sm[t][0] + sm[t][1]) + (sm[t][2] + sm[t][3]);
    out[(long)(s_lo + t) * ldo + row] = v + mu[row];
  }
}

// Phi(x): scipy.special.ndtr structure (xsf/cephes/ndtr.h) on the device erf/erfc
__device__ __forceinline__ double ndtr_dev(double a) {
  if (a != a) return a;
  const double x = a * 0.70710678118654752440;   // M_SQRT1_2
  const double z = fabs(x);
  double y;
  if (z < 1.0) {
    y = 0.5 + 0.5 * erf(x);
  } else {
    y = 0.5 * erfc(z);
    if (x > 0) y = 1.0 - y;
  }
  return y;
}
__device__ __forceinline__ double norm_pdf_dev(double x) {
  return exp(-(x * x) / 2.0) / 2.5066282746310002;   // scipy _norm_pdf: exp(-x**2/2.0)/sqrt(2*pi)
}
__device__ __forceinline__ double ei_norm_diff(double nd) {
  return nd * ndtr_dev(nd) + norm_pdf_dev(nd);       // gpb_acquisitions.py:247-249
}

// mu/sd/acquisition for one chunk.
//   mu_raw = K(Xs,X) alpha ; ss = ||L^-1 k||^2 ; ss2 = extra hallucination term (or null)
//   kss = prior variances k(x_i, x_i) of a kernel that is not stationary (else null: kxx)
__global__ void k_posterior_acq(int acq, double p0, double p1, double kxx, const double* __restrict__ kss,
                                double mean_const, const double* __restrict__ mean_vals, const double* __restrict__ mu_raw,
                                const double* __restrict__ ss, const double* __restrict__ ss2, long m,
                                double* __restrict__ mu_out, double* __restrict__ sd_out,
                                double* __restrict__ val_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double mu = (mean_vals ? mean_vals[i] : mean_const) + mu_raw[i];   // gp_core.py:173-175
  double sd = 0.0;
  if (ss) {
    if (kss) kxx = kss[i];
    double var = kxx - ss[i];                               // diag(K_tete - V^T V), gp_core.py:181
    if (ss2) var = kxx - (ss[i] + ss2[i]);
    sd = sqrt(var);                                         // gp_core.py:187 (NaN if var < 0)
  }
  if (mu_out) mu_out[i] = mu;
  if (sd_out) sd_out[i] = sd;
  if (!val_out) return;
  double v;
  switch (acq) {
    case DFH_ACQ_MEAN: v = mu; break;
    case DFH_ACQ_STD: v = sd; break;
    case DFH_ACQ_UCB: v = mu + p0 * sd; break;              // gpb_acquisitions.py:222
    case DFH_ACQ_EI: {                                      // :256-260
      const double nd = (mu - p0) / sd;
      v = sd * ei_norm_diff(nd);
      break;
    }
    case DFH_ACQ_PI: v = ndtr_dev((mu - p0) / sd); break;   // :238
    case DFH_ACQ_TTEI: {                                    // :275-279
      const double comb = sqrt(p1 * p1 + sd * sd);
      const double nd = (mu - p0) / comb;
      v = comb * ei_norm_diff(nd);
      break;
    }
    default: v = mu;
  }
  val_out[i] = v;
}

// hallucination tail: T[m x q] holds k(x, Xh) - V1 W^T ; solve rows with Lh (q x q lower) and
// return the squared norms.
__global__ void k_halluc_rows(double* __restrict__ T, long m, int q, const double* __restrict__ Lh,
                              double* __restrict__ ss2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double* t = T + i * q;
  double acc = 0.0;
  for (int c = 0; c < q; ++c) {
    double s = t[c];
    for (int k = 0; k < c; ++k) s = fma(-Lh[c * q + k], t[k], s);
    s = s / Lh[c * q + c];
    t[c] = s;
    acc = fma(s, s, acc);
  }
  ss2[i] = acc;
}

__global__ void k_add_vec(double* __restrict__ y, const double* __restrict__ a, double c, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (a ? a[i] : 0.0) + c + y[i];
}

// state of the hallucinated augmentation (gp_core.py:192-220)
struct Halluc {
  int64_t q = 0;
  double* Xhp = nullptr; double* Nhp = nullptr;   // packed Xh
  double* Wt = nullptr;                           // [q][n] = K(Xh,X) L^-T
  double* Lh = nullptr;                           // [q][q] chol(K_hh + noise I - Wt Wt^T)
};

// The reference factors the whole augmented matrix with stable_cholesky (gp_core.py:199-206).  The
// block form below gives the same factor as long as that factorisation needs no jitter; when the
// Schur complement is not positive definite, or the base fit itself needed the ladder (its jitter
// was chosen for the n x n matrix, the reference would re-run the ladder on the (n+q) x (n+q) one),
// DFH_ERR_NOT_PD is returned and the callers fall back to halluc_augmented_gp.
int halluc_prepare(dfh_gp* gp, const double* Xh_user, int64_t q, Halluc* h) {
  dfh_ctx* ctx = gp->ctx;
  h->q = q;
  if (q <= 0) return DFH_OK;
  DFH_ARG(q <= 4096);
  if (gp->diag_jitter != 0.0) return DFH_ERR_NOT_PD;
  if (gp->psd_flags) return DFH_ERR_NOT_PD;      // the reference projects the whole augmented matrix (gp_core.py:199-206)
  const KernDev& kd = gp->kd;
  const double* Xh = nullptr;
  DFH_TRY(to_device(ctx, Xh_user, (size_t)q * gp->d * 8, SCR_STAGE_C, &Xh));
  char* buf = nullptr;
  const size_t b_xhp = (size_t)q * kd.P * 8, b_nhp = (size_t)q * kd.n_parts * 8;
  const size_t b_wt = (size_t)q * gp->n * 8, b_lh = (size_t)q * q * 8;
  DFH_TRY(scratch_get(ctx, SCR_AUG, b_xhp + b_nhp + b_wt + b_lh + 1024, (void**)&buf));
  h->Xhp = reinterpret_cast<double*>(buf);
  h->Nhp = reinterpret_cast<double*>(buf + ((b_xhp + 255) / 256) * 256);
  h->Wt = reinterpret_cast<double*>(reinterpret_cast<char*>(h->Nhp) + ((b_nhp + 255) / 256) * 256);
  h->Lh = reinterpret_cast<double*>(reinterpret_cast<char*>(h->Wt) + ((b_wt + 255) / 256) * 256);
  DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, Xh, q, gp->d, h->Xhp, h->Nhp));
  // Wt = K(Xh, X) L^-T
  DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, h->Xhp, h->Nhp, q, gp->Xp, gp->Np, gp->n, false, 0.0, h->Wt, gp->n));
  DFH_TRY(trsm_rows(ctx, gp->L, gp->n, gp->n, gp->inv, h->Wt, q, gp->n, gp->refine.data()));
  // S = K(Xh,Xh) + (noise + jitter) I - Wt Wt^T ; Lh = chol(S)
  const std::function<int()> build_S = [&]() -> int {
    DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, h->Xhp, h->Nhp, q, h->Xhp, h->Nhp, q, true, gp->noise_var, h->Lh, q));
    return gemm_f64(ctx, 0, q, q, gp->n, -1.0, h->Wt, gp->n, h->Wt, gp->n, 1.0, h->Lh, q, h->Lh, q);
  };
  DFH_TRY(build_S());
  int64_t piv = 0;
  int rc = cholesky_device(ctx, h->Lh, q, q, nullptr, &piv, 1, 0, 0, nullptr, false, &build_S);
  if (rc == DFH_ERR_NOT_PD)
    dfh_set_error("augmented (hallucinated) kernel matrix is not positive definite at pivot %lld",
                  (long long)(gp->n + piv));
  return rc;
}

// One chunk of candidates (device pointer Xs_dev, mc rows): fills mu_raw, ss (and ss2).
// pre_gathered/part range select the add-UCB group path.
int posterior_chunk(dfh_gp* gp, const double* Xs_dev, int64_t mc, int64_t ldxs, int part_lo, int part_hi,
                    bool pre_gathered, bool want_var, const Halluc* h, double** Kct_out,
                    double* mu_raw, double* ss, double* ss2, int parity = 0, double** Xsp_out = nullptr,
                    double** Nsp_out = nullptr, double** T_out = nullptr) {
  dfh_ctx* ctx = gp->ctx;
  const KernDev& kd = gp->kd;
  double* Xsp = nullptr; double* Nsp = nullptr; double* Kct = nullptr;
  char* xs = nullptr;
  const size_t b_xsp = ((size_t)mc * kd.P * 8 + 255) / 256 * 256;
  DFH_TRY(scratch_get(ctx, parity ? SCR_XS2 : SCR_XS, b_xsp + (size_t)mc * kd.n_parts * 8, (void**)&xs));
  Xsp = reinterpret_cast<double*>(xs);
  Nsp = reinterpret_cast<double*>(xs + b_xsp);
  DFH_TRY(scratch_get(ctx, parity ? SCR_KCT2 : SCR_KCT, (size_t)mc * gp->n * 8, (void**)&Kct));
  if (Xsp_out) *Xsp_out = Xsp;
  if (Nsp_out) *Nsp_out = Nsp;
  {
    SectionTimer t(ctx, DFH_T_CROSS);
    DFH_TRY(pack_scaled(ctx, kd, part_lo, part_hi, pre_gathered, Xs_dev, mc, ldxs, Xsp, Nsp));
    bool mu_done = false;      // gp_core.py:174, from the same pass where the kernel can
    DFH_TRY(kernmat_packed(ctx, kd, part_lo, part_hi, true, Xsp, Nsp, mc, gp->Xp, gp->Np, gp->n, false, 0.0, Kct, gp->n,
                           gp->alpha, mu_raw, &mu_done));
    if (!mu_done) DFH_TRY(gemv_rows(ctx, Kct, mc, gp->n, gp->n, gp->alpha, 1.0, nullptr, 0.0, mu_raw));
  }
  if (want_var) {
    {
      SectionTimer t(ctx, DFH_T_TRSM);
      DFH_TRY(trsm_rows(ctx, gp->L, gp->n, gp->n, gp->inv, Kct, mc, gp->n, gp->refine.data()));                // gp_core.py:180
    }
    SectionTimer t(ctx, DFH_T_ACQ);
    if (ss) DFH_TRY(row_sumsq(ctx, Kct, mc, gp->n, gp->n, ss));
    if (h && h->q > 0) {
      const int64_t q = h->q;
      double* T = nullptr;
      DFH_TRY(scratch_get(ctx, parity ? SCR_AUG2B : SCR_AUG2, (size_t)mc * q * 8, (void**)&T));
      // T = k(Xs, Xh) - V1t Wt^T
      DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, Xsp, Nsp, mc, h->Xhp, h->Nhp, q, false, 0.0, T, q));
      DFH_TRY(gemm_f64(ctx, 0, mc, q, gp->n, -1.0, Kct, gp->n, h->Wt, gp->n, 1.0, T, q, T, q));
      hipLaunchKernelGGL(k_halluc_rows, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, T, (long)mc, (int)q, h->Lh, ss2);
      DFH_LAUNCH_CHECK();
      if (T_out) *T_out = T;        // V2^T: the rows solved against Lh
    }
  }
  if (Kct_out) *Kct_out = Kct;
  return DFH_OK;
}

// Fallback of the hallucinated posterior: the GP over (X, Xh) factored from scratch with the
// stable_cholesky ladder -- literally gp_core.py:196-206; only its variance is used (the labels
// are irrelevant: zeros).  The caller frees *aug.
int halluc_augmented_gp(dfh_gp* gp, const double* Xh, int64_t q, dfh_gp** aug) {
  std::vector<double> y0((size_t)(gp->n + q), 0.0);
  return dfh_gp_append(gp, Xh, q, y0.data(), 0, aug, nullptr, nullptr);
}

// Multi-objective scalarisations (opt/multiobjective_gpb_acquisitions.py:19-107), one value per candidate from the k
// rows of A (posterior means, or joint draws) and S (posterior standard deviations; UCB only), row i at i * ld.
// The reference's order of operations, quirks included: the Tchebychev UCB takes the square root of the standard
// deviation (:102-103); np.minimum gives NaN when either operand is NaN.
struct MoParams { double w[DFH_MO_MAX_OBJECTIVES]; double ref[DFH_MO_MAX_OBJECTIVES]; };
__device__ __forceinline__ double np_minimum(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? a : b;
}
__global__ void k_mo_scalarise(int scal, int ucb, int k, double beta, MoParams par, const double* __restrict__ A,
                               const double* __restrict__ S, long ld, long m, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double v;
  if (scal == DFH_MO_LIN) {
    double tot = 0.0, s2 = 0.0;
    for (int j = 0; j < k; ++j) {
      const double w = par.w[j];
      tot = tot + A[j * ld + i] * w;                         // :38 (s += sample * weight), :86 (mu_tot += mu * weight)
      if (ucb) { const double sd = S[j * ld + i]; s2 = s2 + (sd * sd) * (w * w); }   // :87
    }
    v = ucb ? tot + beta * sqrt(s2) : tot;                   // :88
  } else {
    v = INFINITY;                                            // :61, :99
    for (int j = 0; j < k; ++j) {
      double t = A[j * ld + i];
      if (ucb) t = t + beta * sqrt(S[j * ld + i]);           // :103, the square root of 'std' as there
      v = np_minimum(v, (t - par.ref[j]) / par.w[j]);        // :64, :103-104
    }
  }
  out[i] = v;
}

// What both multi-objective entry points demand of their arguments (include/dfhip.h)
int mo_check(dfh_gp* const* gps, int32_t k, int scal, const double* weights, const double* refs, MoParams* par) {
  DFH_ARG(gps && k >= 1 && k <= DFH_MO_MAX_OBJECTIVES && weights);
  DFH_ARG(scal == DFH_MO_LIN || scal == DFH_MO_TCH);
  DFH_ARG(scal == DFH_MO_LIN || refs);
  for (int i = 0; i < k; ++i) {
    DFH_ARG(gps[i] && !gps[i]->gram);            // needs the kernels
    DFH_ARG(gps[i]->ctx == gps[0]->ctx && gps[i]->d == gps[0]->d);
    DFH_ARG(scal == DFH_MO_LIN || weights[i] != 0.0);
    par->w[i] = weights[i];
    par->ref[i] = (scal == DFH_MO_TCH) ? refs[i] : 0.0;
  }
  for (int i = k; i < DFH_MO_MAX_OBJECTIVES; ++i) { par->w[i] = 0.0; par->ref[i] = 0.0; }
  return DFH_OK;
}

// Rows per posterior chunk with K fitted GPs resident: pick_chunk's figure, and never more than an eighth of what
// is free NOW -- with the K factors (K x n^2 x 8 bytes), their block inverses and everything else the caller keeps in
// HBM already taken out -- plus the context's own scratch, which the chunk reuses.
int64_t mo_pick_chunk(dfh_ctx* ctx, int64_t n_max, int64_t m) {
  int64_t mc = pick_chunk(ctx, n_max, m);
  size_t f = 0, t = 0;
  if (hipMemGetInfo(&f, &t) == hipSuccess) {
    size_t own = 0;
    for (const DevBuf& b : ctx->scratch) own += b.bytes;
    int64_t cap = (int64_t)((f + own) / 8 / ((size_t)(n_max > 0 ? n_max : 1) * 8));
    cap = std::max<int64_t>(512, (cap / 512) * 512);
    if (mc > cap) mc = cap;
  } else {
    (void)hipGetLastError();
  }
  return mc;
}

struct DevBlock {           // dev_alloc'ed memory of one call
  dfh_ctx* ctx; void* p = nullptr;
  explicit DevBlock(dfh_ctx* c) : ctx(c) {}
  ~DevBlock() {             // (a block goes back to the cache only once nothing in flight can touch it)
    if (!p) return;
    (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->bulk);
    dev_release(ctx, p);
  }
};

}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" int dfh_kernel_matrix(dfh_ctx* ctx, const dfh_kernel_desc* k, const double* X1, int64_t n1,
                                 const double* X2, int64_t n2, double diag_add, double* K_out) {
  DFH_ARG(ctx && k && K_out);
  DFH_ARG(n1 >= 0 && (X2 == nullptr || n2 >= 0));
  const bool sym = (X2 == nullptr);
  if (sym) n2 = n1;
  if (n1 == 0 || n2 == 0) return DFH_OK;     // kernel.py:81-82: empty result
  DFH_ARG(X1 != nullptr);
  DFH_HIP(hipSetDevice(ctx->device));
  KernDev kd;
  int rc = kerndev_build(ctx, k, &kd);
  if (rc != DFH_OK) { kerndev_free(&kd); return rc; }
  auto body = [&]() -> int {
    const int64_t d = k->dim;
    const double *dX1 = nullptr, *dX2 = nullptr;
    DFH_TRY(to_device(ctx, X1, (size_t)n1 * d * 8, SCR_STAGE_A, &dX1));
    if (!sym) DFH_TRY(to_device(ctx, X2, (size_t)n2 * d * 8, SCR_STAGE_B, &dX2));
    char* buf = nullptr;
    const size_t b1 = ((size_t)n1 * kd.P * 8 + 255) / 256 * 256, bn1 = ((size_t)n1 * kd.n_parts * 8 + 255) / 256 * 256;
    const size_t b2 = sym ? 0 : ((size_t)n2 * kd.P * 8 + 255) / 256 * 256, bn2 = sym ? 0 : (size_t)n2 * kd.n_parts * 8;
    DFH_TRY(scratch_get(ctx, SCR_XS, b1 + bn1 + b2 + bn2 + 256, (void**)&buf));
    double* Xp1 = reinterpret_cast<double*>(buf);
    double* Np1 = reinterpret_cast<double*>(buf + b1);
    double* Xp2 = sym ? Xp1 : reinterpret_cast<double*>(buf + b1 + bn1);
    double* Np2 = sym ? Np1 : reinterpret_cast<double*>(buf + b1 + bn1 + b2);
    DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX1, n1, d, Xp1, Np1));
    if (!sym) DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX2, n2, d, Xp2, Np2));
    const bool dev_out = is_device_ptr(K_out);
    double* Kd = K_out;
    if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n1 * n2 * 8, (void**)&Kd));
    {
      SectionTimer t(ctx, sym ? DFH_T_KERNMAT : DFH_T_CROSS);
      DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, Xp1, Np1, n1, Xp2, Np2, n2, sym, diag_add, Kd, n2));
    }
    if (!dev_out) DFH_TRY(from_device(ctx, K_out, Kd, (size_t)n1 * n2 * 8));
    return DFH_OK;
  };
  rc = body();
  (void)hipStreamSynchronize(ctx->stream);
  kerndev_free(&kd);
  return rc;
}

extern "C" int dfh_dist_squared(dfh_ctx* ctx, const double* X1, int64_t n1, const double* X2, int64_t n2,
                                int64_t d, double* D_out) {
  DFH_ARG(ctx && D_out && d >= 1 && n1 >= 0 && n2 >= 0);
  if (n1 == 0 || n2 == 0) return DFH_OK;
  DFH_ARG(X1 && X2);
  DFH_HIP(hipSetDevice(ctx->device));
  KernDev kd;
  int rc = kerndev_build_dist(ctx, (int)d, &kd);
  if (rc != DFH_OK) { kerndev_free(&kd); return rc; }
  auto body = [&]() -> int {
    const double *dX1 = nullptr, *dX2 = nullptr;
    DFH_TRY(to_device(ctx, X1, (size_t)n1 * d * 8, SCR_STAGE_A, &dX1));
    DFH_TRY(to_device(ctx, X2, (size_t)n2 * d * 8, SCR_STAGE_B, &dX2));
    char* buf = nullptr;
    const size_t b1 = ((size_t)n1 * kd.P * 8 + 255) / 256 * 256, bn1 = ((size_t)n1 * 8 + 255) / 256 * 256;
    const size_t b2 = ((size_t)n2 * kd.P * 8 + 255) / 256 * 256, bn2 = (size_t)n2 * 8;
    DFH_TRY(scratch_get(ctx, SCR_XS, b1 + bn1 + b2 + bn2 + 256, (void**)&buf));
    double* Xp1 = reinterpret_cast<double*>(buf);
    double* Np1 = reinterpret_cast<double*>(buf + b1);
    double* Xp2 = reinterpret_cast<double*>(buf + b1 + bn1);
    double* Np2 = reinterpret_cast<double*>(buf + b1 + bn1 + b2);
    DFH_TRY(pack_scaled(ctx, kd, 0, 1, false, dX1, n1, d, Xp1, Np1));
    DFH_TRY(pack_scaled(ctx, kd, 0, 1, false, dX2, n2, d, Xp2, Np2));
    const bool dev_out = is_device_ptr(D_out);
    double* Kd = D_out;
    if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n1 * n2 * 8, (void**)&Kd));
    DFH_TRY(kernmat_packed(ctx, kd, 0, 1, false, Xp1, Np1, n1, Xp2, Np2, n2, false, 0.0, Kd, n2));
    if (!dev_out) DFH_TRY(from_device(ctx, D_out, Kd, (size_t)n1 * n2 * 8));
    return DFH_OK;
  };
  rc = body();
  (void)hipStreamSynchronize(ctx->stream);
  kerndev_free(&kd);
  return rc;
}

extern "C" int dfh_gemm(dfh_ctx* ctx, int transb, int64_t M, int64_t N, int64_t K, double alpha,
                        const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                        double* C, int64_t ldc, int lower_only) {
  DFH_ARG(ctx && C && M >= 0 && N >= 0 && K >= 0);
  if (M == 0 || N == 0) return DFH_OK;
  DFH_ARG((K == 0 || (A && B)) && lda >= K && ldc >= N && ldb >= (transb ? N : K));
  DFH_HIP(hipSetDevice(ctx->device));
  const double *dA = nullptr, *dB = nullptr, *dCin = nullptr;
  DFH_TRY(to_device(ctx, A, (size_t)M * lda * 8, SCR_STAGE_A, &dA));
  DFH_TRY(to_device(ctx, B, (size_t)(transb ? K : N) * ldb * 8, SCR_STAGE_B, &dB));
  const bool dev_out = is_device_ptr(C);
  double* dC = C;
  if (!dev_out) {
    DFH_TRY(scratch_get(ctx, SCR_STAGE_C, (size_t)M * ldc * 8, (void**)&dC));
    DFH_HIP(hipMemcpyAsync(dC, C, (size_t)M * ldc * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  dCin = dC;
  int flags = (transb ? GEMM_TRANSB : 0) | (lower_only ? GEMM_LOWER : 0);
  DFH_TRY(gemm_f64(ctx, flags, M, N, K, alpha, dA, lda, dB, ldb, beta, dCin, ldc, dC, ldc));
  if (!dev_out) DFH_TRY(from_device(ctx, C, dC, (size_t)M * ldc * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_cholesky(dfh_ctx* ctx, double* A, int64_t n, int64_t* info_pivot) {
  DFH_ARG(ctx && n >= 0);
  if (info_pivot) *info_pivot = 0;
  if (n == 0) return DFH_OK;
  DFH_ARG(A != nullptr);
  DFH_HIP(hipSetDevice(ctx->device));
  const bool dev = is_device_ptr(A);
  double* dA = A;
  if (!dev) {
    DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)n * n * 8, (void**)&dA));
    DFH_HIP(hipMemcpyAsync(dA, A, (size_t)n * n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  int rc;
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    // a host matrix can be uploaded again: the schedules that may need a second attempt are open to it
    const std::function<int()> reupload = [&]() -> int {
      DFH_HIP(hipMemcpyAsync(dA, A, (size_t)n * n * 8, hipMemcpyHostToDevice, ctx->stream));
      return DFH_OK;
    };
    rc = cholesky_device(ctx, dA, n, n, nullptr, info_pivot, 1, 0, 0, nullptr, false, dev ? nullptr : &reupload);
  }
  if (rc != DFH_OK) return rc;
  DFH_TRY(zero_upper(ctx, dA, n, n));
  if (!dev) DFH_TRY(from_device(ctx, A, dA, (size_t)n * n * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_stable_cholesky(dfh_ctx* ctx, const double* M_in, int64_t n, double* L_out,
                                   int32_t* jitter_power) {
  DFH_ARG(ctx && n >= 0);
  if (jitter_power) *jitter_power = INT32_MIN;
  if (n == 0) return DFH_OK;                         // general_utils.py:174-175
  DFH_ARG(M_in && L_out);
  DFH_HIP(hipSetDevice(ctx->device));
  const double* dM = nullptr;
  DFH_TRY(to_device(ctx, M_in, (size_t)n * n * 8, SCR_TSK, &dM));
  const bool dev_out = is_device_ptr(L_out);
  double* dL = L_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)n * n * 8, (void**)&dL));
  auto rebuild = [&]() -> int { return copy_matrix(ctx, dM, n, dL, n, n, n); };
  DFH_TRY(rebuild());
  int rc;
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    rc = stable_cholesky_device(ctx, dL, n, nullptr, true, rebuild, jitter_power, nullptr);
  }
  if (rc != DFH_OK) return rc;
  DFH_TRY(zero_upper(ctx, dL, n, n));
  if (!dev_out) DFH_TRY(from_device(ctx, L_out, dL, (size_t)n * n * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_solve_triangular(dfh_ctx* ctx, const double* L, int64_t n, int upper, const double* b,
                                    int64_t nrhs, double* x_out) {
  DFH_ARG(ctx && n >= 0 && nrhs >= 1);
  if (n == 0) return DFH_OK;
  DFH_ARG(L && b && x_out);
  DFH_HIP(hipSetDevice(ctx->device));
  const double *dL = nullptr, *dB = nullptr;
  DFH_TRY(to_device(ctx, L, (size_t)n * n * 8, SCR_TSL, &dL));
  DFH_TRY(to_device(ctx, b, (size_t)n * nrhs * 8, SCR_STAGE_B, &dB));
  const int64_t nblk = (n + CHOL_NB - 1) / CHOL_NB;
  double* inv = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_CHOLINV, (size_t)inv_buffer_doubles(n) * 8, (void**)&inv));
  std::vector<int> refine((size_t)nblk, 0);
  DFH_TRY(tri_block_inverses(ctx, dL, n, n, inv, refine.data()));
  double* dX = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_OUT, (size_t)n * nrhs * 8, (void**)&dX));
  if (nrhs == 1) {
    DFH_HIP(hipMemcpyAsync(dX, dB, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (!upper) DFH_TRY(trsv_forward(ctx, dL, n, n, inv, dX, refine.data()));
    else DFH_TRY(trsv_backward(ctx, dL, n, n, inv, dX, refine.data()));
  } else {
    double* Bt = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * nrhs * 8, (void**)&Bt));
    DFH_TRY(transpose_matrix(ctx, dB, nrhs, Bt, n, n, nrhs));       // Bt[nrhs][n]
    {
      SectionTimer t(ctx, DFH_T_TRSM);
      if (!upper) DFH_TRY(trsm_rows(ctx, dL, n, n, inv, Bt, nrhs, n, refine.data()));
      else DFH_TRY(trsm_rows_backward(ctx, dL, n, n, inv, Bt, nrhs, n, refine.data()));
    }
    DFH_TRY(transpose_matrix(ctx, Bt, n, dX, nrhs, nrhs, n));
  }
  DFH_TRY(from_device(ctx, x_out, dX, (size_t)n * nrhs * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" int dfh_gp_free(dfh_gp* gp) {
  if (!gp) return DFH_OK;
  if (gp->ctx && ctx_is_live(gp->ctx)) {      // the context may already be gone (teardown order)
    (void)hipSetDevice(gp->ctx->device);
    (void)hipStreamSynchronize(gp->ctx->stream);
  }
  kerndev_free(&gp->kd);
  dev_release(gp->ctx, gp->Xp);
  dev_release(gp->ctx, gp->Np);
  dev_release(gp->ctx, gp->L);
  dev_release(gp->ctx, gp->inv);
  dev_release(gp->ctx, gp->alpha);
  delete gp;
  return DFH_OK;
}

extern "C" int64_t dfh_gp_n(dfh_gp* gp) { return gp ? gp->n : -1; }

extern "C" int dfh_gp_refine_steps(dfh_gp* gp, int32_t* steps_out) {
  DFH_ARG(gp && steps_out);
  for (int64_t b = 0; b < gp->nblk; ++b) steps_out[b] = b < (int64_t)gp->refine.size() ? gp->refine[b] : 0;
  return DFH_OK;
}

// alpha = L^T \ (L \ y_centred) (gp_core.py:161-163) and the log marginal likelihood (:224-226)
static int gp_alpha_and_lml(dfh_gp* gp, const double* dy, double* lml) {
  dfh_ctx* ctx = gp->ctx;
  const int64_t n = gp->n;
  SectionTimer t(ctx, DFH_T_SOLVE);
  DFH_HIP(hipMemcpyAsync(gp->alpha, dy, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
  DFH_TRY(trsv_both(ctx, gp->L, n, n, gp->inv, gp->alpha, gp->refine.data()));
  double logdet = 0.0, dot = 0.0;
  DFH_TRY(logdet_and_dot(ctx, gp->L, n, n, dy, gp->alpha, &logdet, &dot));
  if (lml) *lml = lml_value(logdet, dot, n);
  return DFH_OK;
}

// gp->L <- the factor of K + noise_var I for the n x n kernel matrix dK (device, without noise, left as it is) under
// _get_cholesky_decomp's three branches (gp_core.py:827-847); shared by dfh_gp_fit_gram and the flagged dfh_gp_fit / dfh_gp_append
static int factor_gram_psd(dfh_gp* gp, const double* dK, int flags, int32_t* jitter_power) {
  dfh_ctx* ctx = gp->ctx;
  const int64_t n = gp->n;
  const double noise_var = gp->noise_var;
  auto build_M = [&]() -> int {     // K + noise_var * I     (gp_core.py:843)
    DFH_TRY(copy_matrix(ctx, dK, n, gp->L, n, n, n));
    return add_diag(ctx, gp->L, n, n, noise_var);
  };
  bool project = (flags & DFH_FIT_PROJECT_FIRST) != 0;
  if (flags & DFH_FIT_TRY_BEFORE_PROJECT) {
    // gp_core.py:829-837: plain Cholesky of K + noise I (no ladder); only if that fails, project
    DFH_TRY(build_M());
    SectionTimer t(ctx, DFH_T_CHOL);
    int64_t piv = 0;
    const std::function<int()> rebuild_M = build_M;      // (a hand-off time-out repeats on the safe schedule)
    const int rc = cholesky_device(ctx, gp->L, n, n, gp->inv, &piv, 1, 0, 0, gp->refine.data(), false, &rebuild_M);
    if (rc == DFH_OK) return DFH_OK;
    if (rc != DFH_ERR_NOT_PD) return rc;
    project = true;
  }
  if (project) {
    // gp_core.py:838-841: the kernel matrix (without noise) goes to the PSD cone first
    double* Kp = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)n * n * 8, (void**)&Kp));
    DFH_TRY(psd_project_device(ctx, dK, n, n, 0.0, Kp, n));
    dK = Kp;
  }
  DFH_TRY(build_M());
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    DFH_TRY(stable_cholesky_device(ctx, gp->L, n, gp->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                   jitter_power, &gp->diag_jitter, 0, gp->refine.data()));
  }
  return DFH_OK;
}

extern "C" int dfh_gp_fit(dfh_ctx* ctx, const dfh_kernel_desc* k, const double* X, int64_t n, int64_t d,
                          const double* y_centred, double noise_var, int flags, dfh_gp** out,
                          double* lml, int32_t* jitter_power) {
  DFH_ARG(ctx && k && out && n >= 1 && d >= 1 && X && y_centred);
  DFH_ARG(k->dim == d);
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  DFH_HIP(hipSetDevice(ctx->device));
  dfh_gp* gp = new dfh_gp();
  gp->ctx = ctx; gp->n = n; gp->d = d; gp->noise_var = noise_var;
  gp->nblk = (n + CHOL_NB - 1) / CHOL_NB;
  auto body = [&]() -> int {
    DFH_TRY(kerndev_build(ctx, k, &gp->kd));
    const KernDev& kd = gp->kd;
    DFH_TRY(dev_alloc(ctx, (size_t)n * kd.P * 8, (void**)&gp->Xp));
    DFH_TRY(dev_alloc(ctx, (size_t)n * kd.n_parts * 8, (void**)&gp->Np));
    DFH_TRY(dev_alloc(ctx, (size_t)n * n * 8, (void**)&gp->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n) * 8, (void**)&gp->inv));
    gp->refine.assign((size_t)gp->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n * 8, (void**)&gp->alpha));
    const double *dX = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, X, (size_t)n * d * 8, SCR_STAGE_A, &dX));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n * 8, SCR_STAGE_B, &dy));
    // From n = 2048 on only the lower triangle of the Gram matrix is written (the factorisation, in place in this buffer,
    // reads nothing else; whoever asks for GP.L gets a zeroed upper part, dfh_gp_get): half the bytes of the
    // HBM-write-bound build.  DFH_KM_LOWER_ONLY=0: the full symmetric matrix as before.
    static const bool lower_env = env_flag("DFH_KM_LOWER_ONLY", true);
    static const bool poison_l = env_flag("DFH_TEST_POISON_L", false);
    auto build_M = [&]() -> int {     // K + noise_var * I     (gp_core.py:843)
      SectionTimer t(ctx, DFH_T_KERNMAT);
      ctx->km_lower_only = lower_env && n >= 2048;
      // test hook (tests/test_gpu_upper_triangle_unread.py): the buffer comes recycled from the pool, and with the
      // lower-triangle-only build the tiles above the diagonal keep whatever it held -- correctness rests on no schedule
      // of the factorisation or the solves ever reading them.  DFH_TEST_POISON_L=1 fills the buffer with NaN first.
      if (poison_l) DFH_HIP(hipMemsetAsync(gp->L, 0xFF, (size_t)n * n * 8, ctx->stream));
      const int rc = kernmat_packed(ctx, kd, 0, kd.n_parts, true, gp->Xp, gp->Np, n, gp->Xp, gp->Np, n, true, noise_var, gp->L, n);
      ctx->km_lower_only = false;
      return rc;
    };
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX, n, d, gp->Xp, gp->Np));
    }
    if (flags & DFH_FIT_PSD_FLAGS) {
      // gp_core.py:827-841 from the descriptor: the whole kernel matrix (no noise, both triangles: the projection
      // multiplies with it) is built in a workspace, and the factor comes from it as dfh_gp_fit_gram's does
      gp->psd_flags = flags & DFH_FIT_PSD_FLAGS;
      double* Kw = nullptr;
      DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * n * 8, (void**)&Kw));
      {
        SectionTimer t(ctx, DFH_T_KERNMAT);
        DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, gp->Xp, gp->Np, n, gp->Xp, gp->Np, n, true, 0.0, Kw, n));
      }
      DFH_TRY(factor_gram_psd(gp, Kw, flags, jitter_power));
      return gp_alpha_and_lml(gp, dy, lml);
    }
    DFH_TRY(build_M());
    {
      SectionTimer t(ctx, DFH_T_CHOL);
      DFH_TRY(stable_cholesky_device(ctx, gp->L, n, gp->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                     jitter_power, &gp->diag_jitter, 0, gp->refine.data()));
    }
    return gp_alpha_and_lml(gp, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(gp); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = gp;
  return DFH_OK;
}

// ---------------------------------------------------------------------------------------------
// Posterior for an arbitrary positive semi-definite kernel evaluated by the caller:
// GP.build_posterior with the Gram matrix coming from the documented override hook
// GP._get_training_kernel_matrix (gp_core.py:149-163), and GP.eval with the caller's K(X*, X)
// (gp_core.py:165-190).  The O(n^3) / O(n^2 m) linear algebra is the same device path as for the
// built-in kernels; only the kernel evaluations stay with the caller.
__global__ void k_sd_from_prior(const double* __restrict__ kss, const double* __restrict__ ss,
                                double* __restrict__ sd, long m) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) sd[i] = sqrt(kss[i] - ss[i]);        // no clipping: NaN as in np.sqrt(np.diag(.)), gp_core.py:187
}

extern "C" int dfh_gp_fit_gram(dfh_ctx* ctx, const double* K, int64_t n, const double* y_centred,
                               double noise_var, int flags, dfh_gp** out, double* lml, int32_t* jitter_power) {
  DFH_ARG(ctx && K && out && n >= 1 && y_centred);
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  DFH_HIP(hipSetDevice(ctx->device));
  dfh_gp* gp = new dfh_gp();
  gp->ctx = ctx; gp->n = n; gp->d = 0; gp->noise_var = noise_var; gp->gram = true;
  gp->nblk = (n + CHOL_NB - 1) / CHOL_NB;
  auto body = [&]() -> int {
    DFH_TRY(dev_alloc(ctx, (size_t)n * n * 8, (void**)&gp->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n) * 8, (void**)&gp->inv));
    gp->refine.assign((size_t)gp->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n * 8, (void**)&gp->alpha));
    const double *dK = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, K, (size_t)n * n * 8, SCR_KCT, &dK));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n * 8, SCR_STAGE_B, &dy));
    DFH_TRY(factor_gram_psd(gp, dK, flags, jitter_power));
    return gp_alpha_and_lml(gp, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(gp); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = gp;
  return DFH_OK;
}

// mu = Kcross alpha (+ mean), sd = sqrt(kss - rowsumsq(Kcross L^-T)); Kcross is m x n, row i = k(x*_i, X)
extern "C" int dfh_gp_predict_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* kss,
                                   double mean_const, const double* mean_vals, double* mu_out, double* sd_out) {
  DFH_ARG(gp && m >= 0 && (sd_out == nullptr || kss != nullptr));
  if (m == 0) return DFH_OK;
  DFH_ARG(Kcross && mu_out);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  const int64_t mc_max = pick_chunk(ctx, n, m);
  const bool k_dev = is_device_ptr(Kcross), s_dev = kss ? is_device_ptr(kss) : true;
  const bool mv_dev = mean_vals ? is_device_ptr(mean_vals) : true;
  double *vec = nullptr, *Kct = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 4, (void**)&vec));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)mc_max * n * 8, (void**)&Kct));
  double* mu = vec; double* ss = vec + mc_max; double* sd = vec + 2 * mc_max; double* ks = vec + 3 * mc_max;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    // the chunk of K(X*, X) is solved in place, so it always goes through the workspace
    DFH_HIP(hipMemcpyAsync(Kct, Kcross + i0 * n, (size_t)mc * n * 8,
                           k_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    {
      SectionTimer t(ctx, DFH_T_CROSS);
      DFH_TRY(gemv_rows(ctx, Kct, mc, n, n, gp->alpha, 1.0, nullptr, 0.0, mu));     // gp_core.py:174
    }
    const double* mv_c = nullptr;
    if (mean_vals) {
      if (mv_dev) mv_c = mean_vals + i0;
      else DFH_TRY(to_device(ctx, mean_vals + i0, (size_t)mc * 8, SCR_STAGE_D, &mv_c));
    }
    hipLaunchKernelGGL(k_add_vec, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, mu, mv_c,
                       mv_c ? 0.0 : mean_const, (long)mc);
    DFH_LAUNCH_CHECK();
    DFH_TRY(from_device(ctx, mu_out + i0, mu, (size_t)mc * 8));
    if (sd_out) {
      {
        SectionTimer t(ctx, DFH_T_TRSM);
        DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, mc, n, gp->refine.data()));                  // gp_core.py:180
      }
      SectionTimer t(ctx, DFH_T_ACQ);
      DFH_TRY(row_sumsq(ctx, Kct, mc, n, n, ss));
      const double* ks_c = kss + i0;
      if (!s_dev) {
        DFH_HIP(hipMemcpyAsync(ks, kss + i0, (size_t)mc * 8, hipMemcpyHostToDevice, ctx->stream));
        ks_c = ks;
      }
      hipLaunchKernelGGL(k_sd_from_prior, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, ks_c, ss, sd, (long)mc);
      DFH_LAUNCH_CHECK();
      DFH_TRY(from_device(ctx, sd_out + i0, sd, (size_t)mc * 8));
    }
    DFH_HIP(hipStreamSynchronize(ctx->stream));      // host source buffers may be reused by the caller
  }
  return DFH_OK;
}

// mu_out = Kcross alpha (raw, no mean), cov_out = Ktete - V^T V with V^T = Kcross L^-T  (gp_core.py:179-181)
extern "C" int dfh_gp_predict_covar_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* Ktete,
                                         double* mu_out, double* cov_out) {
  DFH_ARG(gp && m >= 0);
  if (m == 0) return DFH_OK;
  DFH_ARG(Kcross && Ktete && mu_out && cov_out);
  DFH_ARG((double)m * (double)gp->n * 8.0 < 64e9 && (double)m * (double)m * 8.0 < 64e9);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  double *vec = nullptr, *Kct = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)m * 8, (void**)&vec));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)m * n * 8, (void**)&Kct));
  DFH_HIP(hipMemcpyAsync(Kct, Kcross, (size_t)m * n * 8,
                         is_device_ptr(Kcross) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  DFH_TRY(gemv_rows(ctx, Kct, m, n, n, gp->alpha, 1.0, nullptr, 0.0, vec));
  DFH_TRY(from_device(ctx, mu_out, vec, (size_t)m * 8));
  DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, m, n, gp->refine.data()));
  const bool dev_out = is_device_ptr(cov_out);
  double* C = cov_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)m * m * 8, (void**)&C));
  DFH_HIP(hipMemcpyAsync(C, Ktete, (size_t)m * m * 8,
                         is_device_ptr(Ktete) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  DFH_TRY(gemm_f64(ctx, 0, m, m, n, -1.0, Kct, n, Kct, n, 1.0, C, m, C, m));
  if (!dev_out) DFH_TRY(from_device(ctx, cov_out, C, (size_t)m * m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// ---------------------------------------------------------------------------------------------
// Incremental posterior update.  GP.add_data_multiple (gp_core.py:139-146)
// extends X, Y and rebuilds the posterior from scratch -- O((n+q)^3).  With the same kernel,
// noise and data order the factor of the extended matrix is
//     L' = [ L  0 ; B  Ls ],  B = K(Xnew, X) L^-T,  Ls = chol(K(Xnew,Xnew) + noise I - B B^T)
// (the Cholesky factor is unique), which costs O(n^2 q).  A NEW handle is returned; `gp` is left
// untouched (shallow copies of a GP share the handle).  When the reference's rebuild would leave
// the plain-Cholesky branch -- the existing fit needed the stable_cholesky ladder, or the Schur
// complement is not positive definite -- the extended matrix is rebuilt and factored from
// scratch with the ladder, exactly what build_posterior would do.
extern "C" int dfh_gp_append(dfh_gp* gp, const double* Xnew, int64_t q, const double* y_centred, int flags,
                             dfh_gp** out, double* lml, int32_t* jitter_power) {
  DFH_ARG(gp && out && q >= 1 && Xnew && y_centred);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n, n2 = gp->n + q, d = gp->d, NB = CHOL_NB;
  dfh_gp* g2 = new dfh_gp();
  g2->ctx = ctx; g2->n = n2; g2->d = d; g2->noise_var = gp->noise_var;
  g2->nblk = (n2 + NB - 1) / NB;
  auto body = [&]() -> int {
    DFH_TRY(kerndev_clone(ctx, gp->kd, &g2->kd));
    const KernDev& kd = g2->kd;
    const int64_t P = kd.P, parts = kd.n_parts;
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * P * 8, (void**)&g2->Xp));
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * parts * 8, (void**)&g2->Np));
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * n2 * 8, (void**)&g2->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n2) * 8, (void**)&g2->inv));
    g2->refine.assign((size_t)g2->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * 8, (void**)&g2->alpha));
    const double *dXn = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, Xnew, (size_t)q * d * 8, SCR_STAGE_A, &dXn));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n2 * 8, SCR_STAGE_B, &dy));
    double* Xpn = g2->Xp + n * P; double* Npn = g2->Np + n * parts;
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_HIP(hipMemcpyAsync(g2->Xp, gp->Xp, (size_t)n * P * 8, hipMemcpyDeviceToDevice, ctx->stream));
      DFH_HIP(hipMemcpyAsync(g2->Np, gp->Np, (size_t)n * parts * 8, hipMemcpyDeviceToDevice, ctx->stream));
      DFH_TRY(pack_scaled(ctx, kd, 0, parts, false, dXn, q, d, Xpn, Npn));
    }
    auto full_refit = [&]() -> int {             // what build_posterior does: K' + noise I, ladder
      if (gp->psd_flags) {                       // ... or the projection branches, as the fit this handle came from
        g2->psd_flags = gp->psd_flags;
        double* Kw = nullptr;
        DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n2 * n2 * 8, (void**)&Kw));
        {
          SectionTimer t(ctx, DFH_T_KERNMAT);
          DFH_TRY(kernmat_packed(ctx, kd, 0, parts, true, g2->Xp, g2->Np, n2, g2->Xp, g2->Np, n2, true, 0.0, Kw, n2));
        }
        return factor_gram_psd(g2, Kw, gp->psd_flags | (flags & DFH_FIT_NO_JITTER), jitter_power);
      }
      auto build_M = [&]() -> int {
        SectionTimer t(ctx, DFH_T_KERNMAT);
        return kernmat_packed(ctx, kd, 0, parts, true, g2->Xp, g2->Np, n2, g2->Xp, g2->Np, n2, true,
                              g2->noise_var, g2->L, n2);
      };
      DFH_TRY(build_M());
      SectionTimer t(ctx, DFH_T_CHOL);
      return stable_cholesky_device(ctx, g2->L, n2, g2->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                    jitter_power, &g2->diag_jitter, 0, g2->refine.data());
    };
    bool appended = false;
    if (gp->diag_jitter == 0.0 && !gp->psd_flags) {       // (a projection is not a block-row update)
      double* Bm = g2->L + n * n2;               // rows n.., columns 0..n-1
      double* S = g2->L + n * n2 + n;            // the new diagonal block (ld n2)
      DFH_TRY(copy_matrix(ctx, gp->L, n, g2->L, n2, n, n));
      {
        SectionTimer t(ctx, DFH_T_CROSS);
        DFH_TRY(kernmat_packed(ctx, kd, 0, parts, true, Xpn, Npn, q, g2->Xp, g2->Np, n, false, 0.0, Bm, n2));
      }
      {
        SectionTimer t(ctx, DFH_T_TRSM);
        DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Bm, q, n2, gp->refine.data()));
      }
      {
        SectionTimer t(ctx, DFH_T_CHOL);
        const std::function<int()> build_S = [&]() -> int {
          DFH_TRY(kernmat_packed(ctx, kd, 0, parts, true, Xpn, Npn, q, Xpn, Npn, q, true, g2->noise_var, S, n2));
          return gemm_f64(ctx, GEMM_LOWER, q, q, n, -1.0, Bm, n2, Bm, n2, 1.0, S, n2, S, n2);
        };
        DFH_TRY(build_S());
        int64_t piv = 0;
        const int rc = cholesky_device(ctx, S, q, n2, nullptr, &piv, 1, 0, 0, nullptr, false, &build_S);
        if (rc == DFH_OK) {
          // inverses of the 512-blocks: untouched blocks are copied, the rest recomputed from L'
          const int64_t kb0 = n / NB;            // first diagonal block that contains a new row
          double* diag2 = g2->inv + g2->nblk * NB * NB;
          if (kb0 > 0) {
            DFH_HIP(hipMemcpyAsync(g2->inv, gp->inv, (size_t)kb0 * NB * NB * 8, hipMemcpyDeviceToDevice, ctx->stream));
            DFH_HIP(hipMemcpyAsync(diag2, gp->inv + gp->nblk * NB * NB, (size_t)kb0 * NB * NB * 8,
                                   hipMemcpyDeviceToDevice, ctx->stream));
            std::copy(gp->refine.begin(), gp->refine.begin() + kb0, g2->refine.begin());
          }
          DFH_TRY(tri_block_inverses(ctx, g2->L + kb0 * NB * (n2 + 1), n2 - kb0 * NB, n2, g2->inv + kb0 * NB * NB,
                                     g2->refine.data() + kb0, diag2 + kb0 * NB * NB));
          appended = true;
        } else if (rc != DFH_ERR_NOT_PD) {
          return rc;
        }
      }
    }
    if (!appended) DFH_TRY(full_refit());
    return gp_alpha_and_lml(g2, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(g2); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = g2;
  return DFH_OK;
}

extern "C" int dfh_gp_get(dfh_gp* gp, int what, double* out) {
  DFH_ARG(gp && out);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  if (what == DFH_GET_ALPHA) return from_device(ctx, out, gp->alpha, (size_t)n * 8);
  if (what == DFH_GET_L) {
    if (!gp->upper_zeroed) { DFH_TRY(zero_upper(ctx, gp->L, n, n)); gp->upper_zeroed = true; }
    return from_device(ctx, out, gp->L, (size_t)n * n * 8);
  }
  if (what == DFH_GET_K) {
    DFH_ARG(!gp->gram);      // the caller evaluated the Gram matrix and still has it
    const bool dev_out = is_device_ptr(out);
    double* Kd = out;
    if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * n * 8, (void**)&Kd));
    DFH_TRY(kernmat_packed(ctx, gp->kd, 0, gp->kd.n_parts, true, gp->Xp, gp->Np, n, gp->Xp, gp->Np, n, true, 0.0, Kd, n));
    if (!dev_out) DFH_TRY(from_device(ctx, out, Kd, (size_t)n * n * 8));
    return DFH_OK;
  }
  dfh_set_error("dfh_gp_get: unknown selector %d", what);
  return DFH_ERR_BAD_ARG;
}

// shared driver for predict / acquisition arg-max
static int gp_eval_driver(dfh_gp* gp, int acq, const double* params, const double* Xs, int64_t m, int64_t ldxs,
                          int part_lo, int part_hi, bool pre_gathered, double kxx, const double* Xh, int64_t q,
                          double mean_const, const double* mean_vals, bool want_var, double* mu_out,
                          double* sd_out, double* vals_out, double* best_val, int64_t* best_idx) {
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  Halluc h;
  dfh_gp* aug = nullptr;                    // set when the variance comes from the re-factored augmented GP
  if (q > 0 && want_var) {
    int rc = halluc_prepare(gp, Xh, q, &h);
    if (rc == DFH_ERR_NOT_PD) {
      h.q = 0;
      rc = halluc_augmented_gp(gp, Xh, q, &aug);
    }
    DFH_TRY(rc);
  }
  struct AugGuard { dfh_gp* g; ~AugGuard() { if (g) dfh_gp_free(g); } } aug_guard{nullptr};
  aug_guard.g = aug;
  const int64_t mc_max = pick_chunk(gp->ctx, gp->n + (aug ? q : 0), m);
  const bool xs_dev = is_device_ptr(Xs);
  const bool mv_dev = mean_vals ? is_device_ptr(mean_vals) : true;
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 8, (void**)&vec));
  // a kernel with a polynomial / exponential-decay factor: k(x, x) per candidate; on the add-UCB group path
  // (pre_gathered: one group of an additive kernel) the group's own prior variance, if it is such a group
  bool range_stationary = gp->kd.stationary;
  if (pre_gathered) {
    range_stationary = true;
    for (int g = part_lo; g < part_hi; ++g)
      range_stationary = range_stationary && (gp->kd.parts[g].kind == DFH_KERNEL_SE || gp->kd.parts[g].kind == DFH_KERNEL_MATERN);
  }
  double* kss = (want_var && !range_stationary) ? vec + 7 * mc_max : nullptr;
  double* mu_raw = vec; double* ss = vec + mc_max; double* ss2 = vec + 2 * mc_max;
  double* mu_c = vec + 3 * mc_max; double* sd_c = vec + 4 * mc_max; double* val_c = vec + 5 * mc_max;
  bool have = false; double bv = 0.0; int64_t bi = -1;
  const double p0 = params ? params[0] : 0.0, p1 = params ? params[1] : 0.0;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    const double* xs_c = nullptr;
    if (xs_dev) xs_c = Xs + i0 * ldxs;
    else DFH_TRY(to_device(ctx, Xs + i0 * ldxs, (size_t)mc * ldxs * 8, SCR_STAGE_A, &xs_c));
    const double* mv_c = nullptr;
    if (mean_vals) {
      if (mv_dev) mv_c = mean_vals + i0;
      else DFH_TRY(to_device(ctx, mean_vals + i0, (size_t)mc * 8, SCR_STAGE_D, &mv_c));
    }
    double* xsp = nullptr; double* nsp = nullptr;
    if (aug) {
      // mean from the real data, variance from the augmented factor (gp_core.py:195, 207-213)
      DFH_TRY(posterior_chunk(aug, xs_c, mc, ldxs, part_lo, part_hi, pre_gathered, true, nullptr, nullptr, vec + 6 * mc_max, ss, ss2));
      DFH_TRY(posterior_chunk(gp, xs_c, mc, ldxs, part_lo, part_hi, pre_gathered, false, nullptr, nullptr, mu_raw, nullptr, nullptr,
                              0, &xsp, &nsp));
    } else {
      DFH_TRY(posterior_chunk(gp, xs_c, mc, ldxs, part_lo, part_hi, pre_gathered, want_var, &h, nullptr, mu_raw, ss, ss2,
                              0, &xsp, &nsp));
    }
    if (kss) DFH_TRY(pre_gathered ? prior_diag(ctx, gp->kd, xsp, nsp, mc, kss, part_lo, part_hi) : prior_diag(ctx, gp->kd, xsp, nsp, mc, kss));
    {
      SectionTimer t(ctx, DFH_T_ACQ);
      const bool need_val = vals_out || best_val || best_idx;
      hipLaunchKernelGGL(k_posterior_acq, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, acq, p0, p1,
                         kxx, kss, mean_const, mv_c, mu_raw, want_var ? ss : nullptr,
                         (want_var && h.q > 0) ? ss2 : nullptr, (long)mc, mu_out ? mu_c : nullptr,
                         sd_out ? sd_c : nullptr, need_val ? val_c : nullptr);
      DFH_LAUNCH_CHECK();
      if (need_val && (best_val || best_idx)) DFH_TRY(argmax_update(ctx, val_c, mc, i0, &have, &bv, &bi));
    }
    if (mu_out) DFH_TRY(from_device(ctx, mu_out + i0, mu_c, (size_t)mc * 8));
    if (sd_out) DFH_TRY(from_device(ctx, sd_out + i0, sd_c, (size_t)mc * 8));
    if (vals_out) DFH_TRY(from_device(ctx, vals_out + i0, val_c, (size_t)mc * 8));
  }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

extern "C" int dfh_gp_predict(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                              double* mu_out, double* sd_out) {
  DFH_ARG(gp && m >= 0 && q >= 0);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  if (m == 0) return DFH_OK;
  DFH_ARG(Xs && mu_out && (q == 0 || Xh));
  return gp_eval_driver(gp, DFH_ACQ_MEAN, nullptr, Xs, m, gp->d, 0, gp->kd.n_parts, false, gp->kd.kxx, Xh, q,
                        0.0, nullptr, sd_out != nullptr, mu_out, sd_out, nullptr, nullptr, nullptr);
}

extern "C" int dfh_gp_acq_argmax(dfh_gp* gp, int acq, const double* params, const double* Xs, int64_t m,
                                 const double* Xh, int64_t q, double mean_const, const double* mean_vals,
                                 double* vals_out, double* best_val, int64_t* best_idx) {
  DFH_ARG(gp && m >= 1 && Xs && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_ARG(acq >= DFH_ACQ_MEAN && acq <= DFH_ACQ_STD);
  DFH_ARG(params || acq == DFH_ACQ_MEAN || acq == DFH_ACQ_STD);
  const bool want_var = acq != DFH_ACQ_MEAN;
  return gp_eval_driver(gp, acq, params, Xs, m, gp->d, 0, gp->kd.n_parts, false, gp->kd.kxx, Xh, q, mean_const,
                        mean_vals, want_var, nullptr, nullptr, vals_out, best_val, best_idx);
}

extern "C" int dfh_gp_add_ucb_group(dfh_gp* gp, int32_t group, double beta, const double* Xg, int64_t m,
                                    double* vals_out, double* best_val, int64_t* best_idx) {
  DFH_ARG(gp && Xg && m >= 1);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_ARG(gp->kd.multi && !gp->kd.product && !gp->kd.esp && group >= 0 && group < gp->kd.n_parts);   // additive kernels only
  const PartDev& pd = gp->kd.parts[group];
  int gdim = 0;
  for (int c = 0; c < pd.kc; ++c) gdim += gp->kd.cols[pd.poff + c] >= 0;
  const double kxx = gp->kd.outer_scale * kerndev_part_kxx(gp->kd, group);   // kern_scale * kernel_j(x,x)
  const double params[2] = {beta, 0.0};
  return gp_eval_driver(gp, DFH_ACQ_UCB, params, Xg, m, gdim, group, group + 1, true, kxx, nullptr, 0, 0.0,
                        nullptr, true, nullptr, nullptr, vals_out, best_val, best_idx);
}

// All additive groups at once: the per-group cross matrices are stacked into one (sum m_g) x n
// matrix so that the posterior solve is ONE triangular solve with sum(m_g) right-hand sides instead
// of G small ones (the reference issues G solve_lower_triangular calls, gpb_acquisitions.py:161-176).
// Xg_all: group g's candidates [m_g x |group g|], back to back.  Falls back to the per-group
// route when the stack does not fit one posterior chunk.
extern "C" int dfh_gp_add_ucb_all(dfh_gp* gp, const double* betas, const double* Xg_all, const int64_t* m_per_group,
                                  double* vals_out, double* best_vals, int64_t* best_idx) {
  DFH_ARG(gp && betas && Xg_all && m_per_group && best_vals && best_idx);
  DFH_ARG(!gp->gram);
  DFH_ARG(gp->kd.multi && !gp->kd.product && !gp->kd.esp);     // additive kernels only
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = gp->kd;
  const int G = kd.n_parts;
  const int64_t n = gp->n;
  std::vector<int64_t> off(G + 1, 0), xoff(G + 1, 0);
  std::vector<int> gdim(G, 0);
  for (int g = 0; g < G; ++g) {
    DFH_ARG(m_per_group[g] >= 1);
    for (int c = 0; c < kd.parts[g].kc; ++c) gdim[g] += kd.cols[kd.parts[g].poff + c] >= 0;
    off[g + 1] = off[g] + m_per_group[g];
    xoff[g + 1] = xoff[g] + m_per_group[g] * gdim[g];
  }
  const int64_t M = off[G];
  if (M > pick_chunk(ctx, n, M)) {
    for (int g = 0; g < G; ++g)
      DFH_TRY(dfh_gp_add_ucb_group(gp, g, betas[g], Xg_all + xoff[g], m_per_group[g],
                                   vals_out ? vals_out + off[g] : nullptr, &best_vals[g], &best_idx[g]));
    return DFH_OK;
  }
  const double* dXg = nullptr;
  DFH_TRY(to_device(ctx, Xg_all, (size_t)xoff[G] * 8, SCR_STAGE_A, &dXg));
  static_assert(sizeof(long) == sizeof(int64_t), "offsets travel as int64");
  const double* d_off = nullptr;                     // segment offsets for the per-group arg-max
  DFH_TRY(to_device(ctx, reinterpret_cast<const double*>(off.data()), (size_t)(G + 1) * 8, SCR_STAGE_B, &d_off));
  char* xs = nullptr;
  const size_t b_xsp = ((size_t)M * kd.P * 8 + 255) / 256 * 256;
  DFH_TRY(scratch_get(ctx, SCR_XS, b_xsp + (size_t)M * kd.n_parts * 8, (void**)&xs));
  double* Xsp = reinterpret_cast<double*>(xs);
  double* Nsp = reinterpret_cast<double*>(xs + b_xsp);
  double *Kct = nullptr, *vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)M * n * 8, (void**)&Kct));
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)M * 8 * 4, (void**)&vec));
  double* mu_raw = vec; double* ss = vec + M; double* val = vec + 2 * M; double* kss_w = vec + 3 * M;
  {
    SectionTimer t(ctx, DFH_T_CROSS);
    bool mu_all = true;          // posterior means from the cross-matrix pass itself where the kernel can
    for (int g = 0; g < G; ++g) {
      double* Xsp_g = Xsp + off[g] * kd.P; double* Nsp_g = Nsp + off[g] * kd.n_parts;
      DFH_TRY(pack_scaled(ctx, kd, g, g + 1, true, dXg + xoff[g], m_per_group[g], gdim[g], Xsp_g, Nsp_g));
      // K_j(X*_j, X[:, group j]) with the outer scale        (gpb_acquisitions.py:166-168)
      bool mu_done = false;
      DFH_TRY(kernmat_packed(ctx, kd, g, g + 1, true, Xsp_g, Nsp_g, m_per_group[g], gp->Xp, gp->Np, n, false,
                             0.0, Kct + off[g] * n, n, gp->alpha, mu_raw + off[g], &mu_done));
      mu_all = mu_all && mu_done;
    }
    if (!mu_all) DFH_TRY(gemv_rows(ctx, Kct, M, n, n, gp->alpha, 1.0, nullptr, 0.0, mu_raw));
  }
  {
    SectionTimer t(ctx, DFH_T_TRSM);
    DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, M, n, gp->refine.data()));
  }
  SectionTimer t(ctx, DFH_T_ACQ);
  DFH_TRY(row_sumsq(ctx, Kct, M, n, n, ss));
  for (int g = 0; g < G; ++g) {
    const double kxx = kd.outer_scale * kerndev_part_kxx(kd, g);        // kern_scale * kernel_j(x, x)
    const int64_t mg = m_per_group[g];
    const double* kss_g = nullptr;
    if (kd.parts[g].kind != DFH_KERNEL_SE && kd.parts[g].kind != DFH_KERNEL_MATERN) {
      // a polynomial group: its prior variance depends on the point
      DFH_TRY(prior_diag(ctx, kd, Xsp + off[g] * kd.P, Nsp + off[g] * kd.n_parts, mg, kss_w + off[g], g, g + 1));
      kss_g = kss_w + off[g];
    }
    hipLaunchKernelGGL(k_posterior_acq, dim3((unsigned)((mg + 255) / 256)), dim3(256), 0, ctx->stream, (int)DFH_ACQ_UCB,
                       betas[g], 0.0, kxx, kss_g, 0.0, (const double*)nullptr, mu_raw + off[g], ss + off[g],
                       (const double*)nullptr, (long)mg, (double*)nullptr, (double*)nullptr, val + off[g]);
    DFH_LAUNCH_CHECK();
  }
  {   // the G arg-maxes in one launch and one copy back (each used to cost a stream synchronisation)
    char* red = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)G * 16, (void**)&red));
    double* d_bv = reinterpret_cast<double*>(red);
    long* d_bi = reinterpret_cast<long*>(red + (size_t)G * 8);
    hipLaunchKernelGGL(k_argmax_segments, dim3((unsigned)G), dim3(256), 0, ctx->stream, val,
                       reinterpret_cast<const long*>(d_off), d_bv, d_bi);
    DFH_LAUNCH_CHECK();
    DFH_HIP(hipMemcpyAsync(best_vals, d_bv, (size_t)G * 8, hipMemcpyDeviceToHost, ctx->stream));
    DFH_HIP(hipMemcpyAsync(best_idx, d_bi, (size_t)G * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (vals_out) DFH_TRY(from_device(ctx, vals_out, val, (size_t)M * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_gp_predict_covar(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                                    double* mu_out, double* cov_out) {
  DFH_ARG(gp && m >= 0 && q >= 0);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  if (m == 0) return DFH_OK;
  DFH_ARG(Xs && mu_out && cov_out && (q == 0 || Xh));
  DFH_ARG((double)m * (double)gp->n * 8.0 < 64e9);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = gp->kd;
  Halluc h;
  if (q > 0) {
    const int rc = halluc_prepare(gp, Xh, q, &h);
    if (rc == DFH_ERR_NOT_PD) {
      // covariance from the augmented GP factored from scratch, mean from the real data
      dfh_gp* aug = nullptr;
      DFH_TRY(halluc_augmented_gp(gp, Xh, q, &aug));
      int rc2 = dfh_gp_predict_covar(aug, Xs, m, nullptr, 0, mu_out, cov_out);
      dfh_gp_free(aug);
      DFH_TRY(rc2);
      return dfh_gp_predict(gp, Xs, m, nullptr, 0, mu_out, nullptr);
    }
    DFH_TRY(rc);
  }
  const double* dXs = nullptr;
  DFH_TRY(to_device(ctx, Xs, (size_t)m * gp->d * 8, SCR_STAGE_A, &dXs));
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)m * 8 * 3, (void**)&vec));
  double* Kct = nullptr;
  DFH_TRY(posterior_chunk(gp, dXs, m, gp->d, 0, kd.n_parts, false, true, nullptr, &Kct, vec, vec + m, vec + 2 * m));
  DFH_TRY(from_device(ctx, mu_out, vec, (size_t)m * 8));
  // cov = K(Xs,Xs) - V^T V     (gp_core.py:179-181)
  const bool dev_out = is_device_ptr(cov_out);
  double* C = cov_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)m * m * 8, (void**)&C));
  char* xs = reinterpret_cast<char*>(ctx->scratch[SCR_XS].p);      // packed Xs left by posterior_chunk
  double* Xsp = reinterpret_cast<double*>(xs);
  double* Nsp = reinterpret_cast<double*>(xs + ((size_t)m * kd.P * 8 + 255) / 256 * 256);
  DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, Xsp, Nsp, m, Xsp, Nsp, m, true, 0.0, C, m));
  DFH_TRY(gemm_f64(ctx, 0, m, m, gp->n, -1.0, Kct, gp->n, Kct, gp->n, 1.0, C, m, C, m));
  if (q > 0) {
    // second block row of the augmented solve: V2t = (k(Xs,Xh) - V1t Wt^T) Lh^-T ; cov -= V2t V2t^T
    double* T = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_AUG2, (size_t)m * q * 8, (void**)&T));
    DFH_TRY(kernmat_packed(ctx, kd, 0, kd.n_parts, true, Xsp, Nsp, m, h.Xhp, h.Nhp, q, false, 0.0, T, q));
    DFH_TRY(gemm_f64(ctx, 0, m, q, gp->n, -1.0, Kct, gp->n, h.Wt, gp->n, 1.0, T, q, T, q));
    hipLaunchKernelGGL(k_halluc_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, T, (long)m, (int)q, h.Lh, vec + 2 * m);
    DFH_LAUNCH_CHECK();
    DFH_TRY(gemm_f64(ctx, 0, m, m, q, -1.0, T, q, T, q, 1.0, C, m, C, m));
  }
  if (!dev_out) DFH_TRY(from_device(ctx, cov_out, C, (size_t)m * m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// The blocked-joint draw of dfh_gp_ts (include/dfhip.h) for one GP.  `gp` gives the mean; the block covariances come from
// `cov_gp`'s factor -- gp itself, or the augmented GP of the hallucination's fall-back (halluc_augmented_gp) -- and, with
// `h` (halluc_prepare's block form of the q in-progress points, gp_core.py:192-220), lose the rank-q term V2^T V2 as well.
// samples_dev (optional, device [m]) receives the draw without a trip to the host; the arg-max is skipped when neither
// best_val nor best_idx is wanted (the multi-objective call scalarises K draws first).
// S > 1 (dfh_gp_draw): U is [m x S] row-major, np.random.normal(size=(m, S)), and every block's factor serves all S draws
// in one launch of k_tri_draw; samples_dev / samples_out are then [S x m] and best_val / best_idx [S].  S == 1 runs the
// code, kernels and synchronisation points it always ran.
static int ts_run(dfh_gp* gp, dfh_gp* cov_gp, const Halluc* h, const double* Xs, int64_t m, int64_t block, const double* U,
                  double mean_const, const double* mean_vals, double* samples_dev, double* samples_out, double* best_val,
                  int64_t* best_idx, int32_t* jitter_powers_out, int32_t S = 1) {
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = cov_gp->kd;
  const int64_t n = cov_gp->n;
  const int64_t hq = (h && cov_gp == gp) ? h->q : 0;
  if (block > m) block = m;
  DFH_ARG((double)block * (double)block * 8.0 < 32e9);
  // several TS blocks share one posterior chunk so the TRSM runs on big GEMMs
  int64_t bpc = std::max<int64_t>(1, pick_chunk(ctx, n, m) / block);
  const int64_t mc_max = std::min(m, bpc * block);
  const int64_t nchunks = (m + mc_max - 1) / mc_max;
  const bool xs_dev = is_device_ptr(Xs), u_dev = is_device_ptr(U);
  const bool mv_dev = mean_vals ? is_device_ptr(mean_vals) : true;
  double* vec[2] = {nullptr, nullptr};
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 3, (void**)&vec[0]));      // mu | draw | spare (ss2 / unused mean)
  DFH_TRY(scratch_get(ctx, SCR_VECB, (size_t)mc_max * 8 * 3, (void**)&vec[1]));
  // up to DFH_TS_BATCH (64) blocks of a chunk are factored as one lock-step batch
  static const int ts_batch = std::min(std::max(env_int("DFH_TS_BATCH", 64), 1), CHOL_MAX_BATCH);
  const int64_t lb_slots = std::max<int64_t>(1, std::min<int64_t>(ts_batch, mc_max / block));
  double* Lb = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)lb_slots * block * block * 8, (void**)&Lb));
  // S > 1: the chunk's normals sample-major (even leading dimension: a block's offset alone decides the 16-byte
  // alignment, as it does for the single draw's vector) | its S draws, rows tight | the per-draw winners
  DevBlock multi(ctx);
  const int64_t ldu = (mc_max + 1) & ~(int64_t)1;
  double* Ut = nullptr; double* sampS = nullptr; double* win_v = nullptr; long* win_i = nullptr;
  std::vector<double> hv, bvS; std::vector<long> hi; std::vector<int64_t> biS; std::vector<char> haveS;
  if (S > 1) {
    DFH_TRY(dev_alloc(ctx, ((size_t)S * ldu + (size_t)S * mc_max + 2 * (size_t)S) * 8, &multi.p));
    Ut = static_cast<double*>(multi.p);
    sampS = Ut + (int64_t)S * ldu;
    win_v = sampS + (int64_t)S * mc_max;
    win_i = reinterpret_cast<long*>(win_v + S);
    hv.resize(S); hi.resize(S); haveS.assign(S, 0); bvS.assign(S, 0.0); biS.assign(S, -1);
  }
  // Two-stage software pipeline over chunks.  Stage 1 (low-priority `bulk` stream): cross kernel
  // matrix, mu, and the posterior TRSM of chunk c+1 -- large MFMA GEMMs.  Stage 2 (main + panel
  // streams): per TS block of chunk c the covariance SYRK, its stable_cholesky (latency-bound
  // look-ahead factorisation, host-synchronous because of the jitter ladder) and the draw.
  // The factorisations hide behind the next chunk's TRSM instead of idling the GPU.
  hipStream_t mainS = ctx->stream, bulkS = ctx->bulk;
  struct Stage1 { double* Kct; double* Xsp; double* Nsp; double* mu; double* T; };
  Stage1 st[2];
  hipEvent_t ev_in, ev_ready[2], ev_free[2];
  DFH_TRY(ctx_event(ctx, EV_TS_BASE, &ev_in));
  for (int p = 0; p < 2; ++p) {
    DFH_TRY(ctx_event(ctx, EV_TS_BASE + 1 + p, &ev_ready[p]));
    DFH_TRY(ctx_event(ctx, EV_TS_BASE + 3 + p, &ev_free[p]));
  }
  DFH_HIP(hipEventRecord(ev_in, mainS));
  DFH_HIP(hipStreamWaitEvent(bulkS, ev_in, 0));        // inputs produced on the main stream are ready

  auto stage1 = [&](int64_t c) -> int {
    const int p = (int)(c & 1);
    const int64_t i0 = c * mc_max;
    const int64_t mc = std::min(mc_max, m - i0);
    StreamSwap on_bulk(ctx, bulkS);
    if (c >= 2) DFH_HIP(hipStreamWaitEvent(bulkS, ev_free[p], 0));   // parity buffers released by stage 2
    const double* xs_c = nullptr;
    if (xs_dev) xs_c = Xs + i0 * gp->d;
    else DFH_TRY(to_device(ctx, Xs + i0 * gp->d, (size_t)mc * gp->d * 8, p ? SCR_STAGE_A2 : SCR_STAGE_A, &xs_c));
    st[p].mu = vec[p];
    st[p].T = nullptr;
    if (cov_gp != gp) {
      // mean from the real data, V^T from the augmented factor (gp_core.py:195, 207-213); same parity buffers, in this order
      DFH_TRY(posterior_chunk(gp, xs_c, mc, gp->d, 0, kd.n_parts, false, false, nullptr, nullptr, st[p].mu, nullptr, nullptr, p));
      DFH_TRY(posterior_chunk(cov_gp, xs_c, mc, gp->d, 0, kd.n_parts, false, true, nullptr, &st[p].Kct, vec[p] + 2 * mc_max,
                              nullptr, nullptr, p, &st[p].Xsp, &st[p].Nsp));
    } else {
      DFH_TRY(posterior_chunk(gp, xs_c, mc, gp->d, 0, kd.n_parts, false, true, hq > 0 ? h : nullptr, &st[p].Kct, st[p].mu,
                              nullptr, vec[p] + 2 * mc_max, p, &st[p].Xsp, &st[p].Nsp, &st[p].T));
    }
    DFH_HIP(hipEventRecord(ev_ready[p], bulkS));
    return DFH_OK;
  };

  bool have = false; double bv = 0.0; int64_t bi = -1;
  int64_t blk_idx = 0;
  DFH_TRY(stage1(0));
  for (int64_t c = 0; c < nchunks; ++c) {
    const int p = (int)(c & 1);
    const int64_t i0 = c * mc_max;
    const int64_t mc = std::min(mc_max, m - i0);
    if (c + 1 < nchunks) DFH_TRY(stage1(c + 1));        // enqueue ahead: overlaps with the blocks below
    DFH_HIP(hipStreamWaitEvent(mainS, ev_ready[p], 0));
    const double* u_c = nullptr;
    if (u_dev) u_c = U + i0 * S;
    else DFH_TRY(to_device(ctx, U + i0 * S, (size_t)mc * S * 8, SCR_STAGE_C, &u_c));
    if (S > 1) DFH_TRY(transpose_matrix(ctx, u_c, S, Ut, ldu, mc, S));
    const double* mv_c = nullptr;
    if (mean_vals) {
      if (mv_dev) mv_c = mean_vals + i0;
      else DFH_TRY(to_device(ctx, mean_vals + i0, (size_t)mc * 8, SCR_STAGE_D, &mv_c));
    }
    double* mu_raw = st[p].mu;
    double* samp = vec[p] + mc_max;
    double* Kct = st[p].Kct;
    // mean_vals = test_mean + K_tetr alpha
    hipLaunchKernelGGL(k_add_vec, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, mu_raw, mv_c,
                       mv_c ? 0.0 : mean_const, (long)mc);
    DFH_LAUNCH_CHECK();
    // one TS block: Sigma = K(Xb,Xb) - V^T V (gp_core.py:179-181; chol reads the lower triangle),
    // stable_cholesky (general_utils.py:229), s = L u + mu (general_utils.py:231)
    auto sigma_kernel = [&](int64_t b0, int64_t B, double* dst) -> int {
      const double* Xbp = st[p].Xsp + b0 * kd.P;
      const double* Nbp = st[p].Nsp + b0 * kd.n_parts;
      return kernmat_packed(ctx, kd, 0, kd.n_parts, true, Xbp, Nbp, B, Xbp, Nbp, B, true, 0.0, dst, B);
    };
    auto single_block = [&](int64_t b0, int64_t B, double* dst, int64_t bidx) -> int {
      const double* Vt = Kct + b0 * n;
      auto build_sigma = [&]() -> int {
        DFH_TRY(sigma_kernel(b0, B, dst));
        DFH_TRY(gemm_f64(ctx, GEMM_LOWER, B, B, n, -1.0, Vt, n, Vt, n, 1.0, dst, B, dst, B));
        if (hq == 0) return DFH_OK;
        const double* V2t = st[p].T + b0 * hq;           // second block row of the augmented solve: Sigma -= V2^T V2
        return gemm_f64(ctx, GEMM_LOWER, B, B, hq, -1.0, V2t, hq, V2t, hq, 1.0, dst, B, dst, B);
      };
      DFH_TRY(build_sigma());
      int32_t jp = INT32_MIN;
      DFH_TRY(stable_cholesky_device(ctx, dst, B, nullptr, true, build_sigma, &jp, nullptr));
      if (jitter_powers_out) jitter_powers_out[bidx] = jp;
      return DFH_OK;
    };
    // s = L u + mu of one factored block: the single draw's kernel, or all S draws in one launch.  `vec` is the single
    // draw's choice of summation order for this block (gemv_rows: even leading dimension, factor and normals 16-byte
    // aligned -- the caller's U taken to be aligned as a whole), so that draw s is that call's with column s.
    auto draw_block = [&](const double* Lf, int64_t b0, int64_t B) -> int {
      if (S == 1) return gemv_rows(ctx, Lf, B, B, B, u_c + b0, 1.0, mu_raw + b0, 1.0, samp + b0, true);
      const int vec = ((B & 1) == 0) && ((reinterpret_cast<uintptr_t>(Lf) & 15) == 0) && ((((u_dev ? i0 : 0) + b0) & 1) == 0);
      hipLaunchKernelGGL(k_tri_draw, dim3((unsigned)((S + DRAW_TILE - 1) / DRAW_TILE), (unsigned)B), dim3(256), 0, ctx->stream,
                         Lf, (long)B, (const double*)(Ut + b0), (long)ldu, (int)S, (const double*)(mu_raw + b0), sampS + b0,
                         (long)mc, vec);
      DFH_LAUNCH_CHECK();
      return DFH_OK;
    };
    const int64_t nfull = mc / block;
    for (int64_t g0 = 0; g0 < nfull; g0 += lb_slots) {
      // the equal-sized blocks of the chunk are factored in lock-step: one batched launch sequence
      // instead of `nb` latency-bound ones
      const int nb = (int)std::min<int64_t>(lb_slots, nfull - g0);
      const int64_t B = block;
      SectionTimer t(ctx, DFH_T_TS);
      if (nb == 1) {
        DFH_TRY(single_block(g0 * B, B, Lb, blk_idx + g0));
      } else {
        // (also the rebuild closure of the factorisation: small groups take the one-launch panels, whose
        //  hand-offs are bounded waits -- on expiry, e.g. with other contexts crowding the device, the group
        //  is rebuilt and factored on the schedule without inter-workgroup waits)
        const std::function<int()> build_group = [&]() -> int {
          for (int b = 0; b < nb; ++b) DFH_TRY(sigma_kernel((g0 + b) * B, B, Lb + b * B * B));
          GemmBatch bs;
          bs.count = nb; bs.sA = bs.sB = B * n; bs.sCin = bs.sCout = B * B;
          const double* Vt = Kct + g0 * B * n;
          DFH_TRY(gemm_f64(ctx, GEMM_LOWER, B, B, n, -1.0, Vt, n, Vt, n, 1.0, Lb, B, Lb, B, &bs));
          if (hq == 0) return DFH_OK;
          GemmBatch bh;
          bh.count = nb; bh.sA = bh.sB = B * hq; bh.sCin = bh.sCout = B * B;
          const double* V2t = st[p].T + g0 * B * hq;
          return gemm_f64(ctx, GEMM_LOWER, B, B, hq, -1.0, V2t, hq, V2t, hq, 1.0, Lb, B, Lb, B, &bh);
        };
        DFH_TRY(build_group());
        int64_t piv[CHOL_MAX_BATCH] = {0};
        int rc = cholesky_device(ctx, Lb, B, B, nullptr, piv, nb, B * B, 0, nullptr, false, &build_group);
        if (rc != DFH_OK && rc != DFH_ERR_NOT_PD) return rc;
        for (int b = 0; b < nb; ++b) {
          if (piv[b] == 0) { if (jitter_powers_out) jitter_powers_out[blk_idx + g0 + b] = INT32_MIN; continue; }
          // this block needs the jitter ladder: redo it alone (rebuilds Sigma first)
          DFH_TRY(single_block((g0 + b) * B, B, Lb + b * B * B, blk_idx + g0 + b));
        }
      }
      for (int b = 0; b < nb; ++b) {
        const int64_t b0 = (g0 + b) * B;
        DFH_TRY(draw_block(Lb + b * B * B, b0, B));
      }
    }
    if (nfull * block < mc) {           // ragged last block
      const int64_t b0 = nfull * block, B = mc - b0;
      SectionTimer t(ctx, DFH_T_TS);
      DFH_TRY(single_block(b0, B, Lb, blk_idx + nfull));
      DFH_TRY(draw_block(Lb, b0, B));
    }
    blk_idx += (mc + block - 1) / block;
    if (S > 1) {
      if (best_val || best_idx) {
        hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned)S), dim3(256), 0, mainS, (const double*)sampS, (long)mc, (long)mc,
                           win_v, win_i);
        DFH_LAUNCH_CHECK();
        DFH_HIP(hipMemcpyAsync(hv.data(), win_v, (size_t)S * 8, hipMemcpyDeviceToHost, mainS));
        DFH_HIP(hipMemcpyAsync(hi.data(), win_i, (size_t)S * 8, hipMemcpyDeviceToHost, mainS));
        DFH_HIP(hipStreamSynchronize(mainS));
        for (int32_t si = 0; si < S; ++si) {
          const int64_t gi = i0 + (int64_t)hi[si];
          if (!haveS[si] || host_better(hv[si], gi, bvS[si], biS[si])) { bvS[si] = hv[si]; biS[si] = gi; haveS[si] = 1; }
        }
      }
      if (samples_dev)
        DFH_HIP(hipMemcpy2DAsync(samples_dev + i0, (size_t)m * 8, sampS, (size_t)mc * 8, (size_t)mc * 8, (size_t)S,
                                 hipMemcpyDeviceToDevice, mainS));
      if (samples_out) {
        const bool out_dev = is_device_ptr(samples_out);
        DFH_HIP(hipMemcpy2DAsync(samples_out + i0, (size_t)m * 8, sampS, (size_t)mc * 8, (size_t)mc * 8, (size_t)S,
                                 out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, mainS));
        if (!out_dev) DFH_HIP(hipStreamSynchronize(mainS));
      }
    } else {
      if (best_val || best_idx) DFH_TRY(argmax_update(ctx, samp, mc, i0, &have, &bv, &bi));
      if (samples_dev) DFH_HIP(hipMemcpyAsync(samples_dev + i0, samp, (size_t)mc * 8, hipMemcpyDeviceToDevice, mainS));
      if (samples_out) DFH_TRY(from_device(ctx, samples_out + i0, samp, (size_t)mc * 8));
    }
    DFH_HIP(hipEventRecord(ev_free[p], mainS));
  }
  DFH_HIP(hipStreamSynchronize(mainS));
  DFH_HIP(hipStreamSynchronize(bulkS));
  if (S > 1) {
    for (int32_t si = 0; si < S; ++si) {
      if (best_val) best_val[si] = bvS[si];
      if (best_idx) best_idx[si] = biS[si];
    }
    return DFH_OK;
  }
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

extern "C" int dfh_gp_ts(dfh_gp* gp, const double* Xs, int64_t m, int64_t block, const double* U,
                         double mean_const, const double* mean_vals, double* samples_out, double* best_val,
                         int64_t* best_idx, int32_t* jitter_powers_out) {
  DFH_ARG(gp && Xs && U && m >= 1 && block >= 1);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  // (the arg-max always ran here, whatever the caller asked for: keep its synchronisation points)
  double bv = 0.0; int64_t bi = -1;
  DFH_TRY(ts_run(gp, gp, nullptr, Xs, m, block, U, mean_const, mean_vals, nullptr, samples_out, &bv, &bi, jitter_powers_out));
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

// The joint draw of one GP with points in progress and S samples (include/dfhip.h): gp.draw_samples(S, Xs) and
// gp.draw_samples_with_hallucinated_observations(S, Xs, Xh) (gp_core.py:250-261) block by block.  One covariance and one
// stable_cholesky per block, shared by the S draws.
extern "C" int dfh_gp_draw(dfh_gp* gp, const double* Xs, int64_t m, int64_t block, const double* Xh, int64_t q,
                           const double* U, int32_t S, double mean_const, const double* mean_vals, double* samples_out,
                           double* best_vals, int64_t* best_idx, int32_t* jitter_powers_out) {
  DFH_ARG(gp && Xs && U && m >= 1 && block >= 1);
  DFH_ARG(S >= 1 && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_HIP(hipSetDevice(gp->ctx->device));
  // the augmentation as dfh_mo_ts_argmax takes it: block form, or the augmented GP factored from scratch with the ladder
  Halluc h;
  dfh_gp* aug = nullptr;
  if (q > 0) {
    int rc = halluc_prepare(gp, Xh, q, &h);
    if (rc == DFH_ERR_NOT_PD) {
      h.q = 0;
      rc = halluc_augmented_gp(gp, Xh, q, &aug);
    }
    DFH_TRY(rc);
  }
  const int rc = ts_run(gp, aug ? aug : gp, q > 0 ? &h : nullptr, Xs, m, block, U, mean_const, mean_vals, nullptr, samples_out,
                        best_vals, best_idx, jitter_powers_out, S);
  if (aug) dfh_gp_free(aug);
  return rc;
}

// ---- multi-objective acquisitions: K fitted GPs, one call -------------------------------------------------------
extern "C" int dfh_mo_ucb_argmax(dfh_gp* const* gps, int32_t k, int scal, double beta, const double* weights,
                                 const double* refs, const double* Xs, int64_t m, const double* mean_consts,
                                 const double* mean_vals, double* vals_out, double* best_val, int64_t* best_idx) {
  MoParams par;
  DFH_TRY(mo_check(gps, k, scal, weights, refs, &par));
  DFH_ARG(Xs && m >= 1 && (mean_consts || mean_vals));
  dfh_ctx* ctx = gps[0]->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t d = gps[0]->d;
  int64_t n_max = 0;
  for (int i = 0; i < k; ++i) n_max = std::max(n_max, gps[i]->n);
  const int64_t mc_max = mo_pick_chunk(ctx, n_max, m);
  // the candidates (and per-candidate prior means) go to HBM once, not once per objective
  DevBlock stage(ctx);
  const bool xs_dev = is_device_ptr(Xs), mv_dev = mean_vals ? is_device_ptr(mean_vals) : true;
  const size_t b_xs = xs_dev ? 0 : (size_t)m * d * 8, b_mv = mv_dev ? 0 : (size_t)k * m * 8;
  if (b_xs + b_mv) {
    DFH_TRY(dev_alloc(ctx, b_xs + b_mv, &stage.p));
    char* sp = static_cast<char*>(stage.p);
    if (b_xs) { DFH_HIP(hipMemcpyAsync(sp, Xs, b_xs, hipMemcpyHostToDevice, ctx->stream)); Xs = reinterpret_cast<const double*>(sp); }
    if (b_mv) { DFH_HIP(hipMemcpyAsync(sp + b_xs, mean_vals, b_mv, hipMemcpyHostToDevice, ctx->stream)); mean_vals = reinterpret_cast<const double*>(sp + b_xs); }
    DFH_HIP(hipStreamSynchronize(ctx->stream));      // pageable sources: staged before the caller's buffers may change
  }
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * (4 + 2 * (size_t)k), (void**)&vec));
  double* mu_raw = vec; double* ss = vec + mc_max; double* kss_w = vec + 2 * mc_max; double* val_c = vec + 3 * mc_max;
  double* MU = vec + 4 * mc_max; double* SD = MU + (int64_t)k * mc_max;       // [k][mc_max] each
  bool have = false; double bv = 0.0; int64_t bi = -1;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    const unsigned grid = (unsigned)((mc + 255) / 256);
    for (int i = 0; i < k; ++i) {
      dfh_gp* gp = gps[i];
      double* xsp = nullptr; double* nsp = nullptr;
      // gp.eval(x, 'std'), :85 / :102 -- each objective packs the shared candidates with its own bandwidths
      DFH_TRY(posterior_chunk(gp, Xs + i0 * d, mc, d, 0, gp->kd.n_parts, false, true, nullptr, nullptr, mu_raw, ss, nullptr,
                              0, &xsp, &nsp));
      double* kss = gp->kd.stationary ? nullptr : kss_w;
      if (kss) DFH_TRY(prior_diag(ctx, gp->kd, xsp, nsp, mc, kss));
      SectionTimer t(ctx, DFH_T_ACQ);
      hipLaunchKernelGGL(k_posterior_acq, dim3(grid), dim3(256), 0, ctx->stream, (int)DFH_ACQ_MEAN, 0.0, 0.0, gp->kd.kxx,
                         (const double*)kss, mean_consts ? mean_consts[i] : 0.0,
                         mean_vals ? mean_vals + (int64_t)i * m + i0 : (const double*)nullptr, (const double*)mu_raw,
                         (const double*)ss, (const double*)nullptr, (long)mc, MU + (int64_t)i * mc_max,
                         SD + (int64_t)i * mc_max, (double*)nullptr);
      DFH_LAUNCH_CHECK();
    }
    SectionTimer t(ctx, DFH_T_ACQ);
    hipLaunchKernelGGL(k_mo_scalarise, dim3(grid), dim3(256), 0, ctx->stream, scal, 1, (int)k, beta, par, (const double*)MU,
                       (const double*)SD, (long)mc_max, (long)mc, val_c);
    DFH_LAUNCH_CHECK();
    if (best_val || best_idx) DFH_TRY(argmax_update(ctx, val_c, mc, i0, &have, &bv, &bi));
    if (vals_out) DFH_TRY(from_device(ctx, vals_out + i0, val_c, (size_t)mc * 8));
  }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

extern "C" int dfh_mo_ts_argmax(dfh_gp* const* gps, int32_t k, int scal, const double* weights, const double* refs,
                                const double* Xs, int64_t m, int64_t block, const double* Xh, int64_t q, const double* U,
                                const double* mean_consts, const double* mean_vals, double* vals_out, double* best_val,
                                int64_t* best_idx, int32_t* jitter_powers_out) {
  MoParams par;
  DFH_TRY(mo_check(gps, k, scal, weights, refs, &par));
  DFH_ARG(Xs && U && m >= 1 && block >= 1 && q >= 0 && (q == 0 || Xh) && (mean_consts || mean_vals));
  dfh_ctx* ctx = gps[0]->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t d = gps[0]->d;
  if (block > m) block = m;
  const int64_t nblk = (m + block - 1) / block;
  // candidates (if they come from the host) | the K draws, objective-major | the scalarised values.  Memory of this
  // call's own, not scratch: the hallucination's fall-back re-fits a GP between two objectives.
  DevBlock hold(ctx);
  const bool xs_dev = is_device_ptr(Xs);
  const size_t b_xs = xs_dev ? 0 : (size_t)m * d * 8;
  DFH_TRY(dev_alloc(ctx, b_xs + (size_t)(k + 1) * m * 8, &hold.p));
  char* hp = static_cast<char*>(hold.p);
  if (b_xs) { DFH_HIP(hipMemcpyAsync(hp, Xs, b_xs, hipMemcpyHostToDevice, ctx->stream)); Xs = reinterpret_cast<const double*>(hp); DFH_HIP(hipStreamSynchronize(ctx->stream)); }
  double* S = reinterpret_cast<double*>(hp + b_xs);
  double* vals = S + (int64_t)k * m;
  for (int i = 0; i < k; ++i) {
    dfh_gp* gp = gps[i];
    // get_gp_sampler_for_parallel_strategy (:29, :54): the draw of the GP augmented with the points in progress
    // (gp_core.py:256-261) -- block form, or the augmented GP factored from scratch where that is not positive definite
    Halluc h;
    dfh_gp* aug = nullptr;
    if (q > 0) {
      int rc = halluc_prepare(gp, Xh, q, &h);
      if (rc == DFH_ERR_NOT_PD) {
        h.q = 0;
        rc = halluc_augmented_gp(gp, Xh, q, &aug);
      }
      DFH_TRY(rc);
    }
    const int rc = ts_run(gp, aug ? aug : gp, &h, Xs, m, block, U + (int64_t)i * m, mean_consts ? mean_consts[i] : 0.0,
                          mean_vals ? mean_vals + (int64_t)i * m : nullptr, S + (int64_t)i * m, nullptr, nullptr, nullptr,
                          jitter_powers_out ? jitter_powers_out + (int64_t)i * nblk : nullptr);
    if (aug) dfh_gp_free(aug);
    DFH_TRY(rc);
  }
  SectionTimer t(ctx, DFH_T_ACQ);
  hipLaunchKernelGGL(k_mo_scalarise, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, scal, 0, (int)k, 0.0, par,
                     (const double*)S, (const double*)nullptr, (long)m, (long)m, vals);
  DFH_LAUNCH_CHECK();
  bool have = false; double bv = 0.0; int64_t bi = -1;
  if (best_val || best_idx) DFH_TRY(argmax_update(ctx, vals, m, 0, &have, &bv, &bi));
  if (vals_out) DFH_TRY(from_device(ctx, vals_out, vals, (size_t)m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

#ifdef DFH_DEBUG_HOOKS      // diagnostics: built only with `python -m dragonfly_amd.build --debug-hooks` (include/dfhip_debug.h)
// Diagnostics hook (not part of the product path): do kernels on the bulk stream and on the main /
// panel streams actually run concurrently?  Enqueues `n_big` large GEMMs on stream A and `n_small`
// tiny kernels on stream B and reports the time of each alone and together.
// which: 0 = A is bulk, B is main; 1 = A is main, B is side; 2 = A is bulk, B is side
extern "C" int dfh_debug_overlap(dfh_ctx* ctx, int which, int n_big, int n_small, double* out_ms /*[4]*/) {
  DFH_ARG(ctx && out_ms);
  hipStream_t A = (which == 1) ? ctx->main_stream : ctx->bulk;
  hipStream_t B = (which == 0) ? ctx->main_stream : ctx->side;
  const int64_t M = 16384, N = 512, K = 4096;
  double *a = nullptr, *b = nullptr, *c = nullptr, *v = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)M * K * 8, (void**)&a));
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)N * K * 8, (void**)&b));
  DFH_TRY(scratch_get(ctx, SCR_TMP, (size_t)M * N * 8, (void**)&c));
  DFH_TRY(scratch_get(ctx, SCR_VEC, 1 << 20, (void**)&v));
  DFH_TRY(fill_f64(ctx, a, M * K, 0.5));
  DFH_TRY(fill_f64(ctx, b, N * K, 0.25));
  DFH_HIP(hipDeviceSynchronize());
  int least = 0, greatest = 0;
  DFH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  out_ms[3] = least * 100.0 + greatest;
  auto run = [&](bool big, bool small, double* ms) -> int {
    DFH_HIP(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    if (big) {
      StreamSwap sw(ctx, A);
      for (int i = 0; i < n_big; ++i) DFH_TRY(gemm_f64(ctx, 0, M, N, K, 1.0, a, K, b, K, 0.0, nullptr, 0, c, N));
    }
    if (small) {
      StreamSwap sw(ctx, B);
      for (int i = 0; i < n_small; ++i) {
        if (which >= 10) DFH_TRY(fill_f64(ctx, v, 4096, 1.0));
        else DFH_TRY(gemm_f64(ctx, 0, 64, 64, 64, 1.0, a, K, b, K, 0.0, nullptr, 0, v, 64));   // 38 KB LDS, 1 workgroup
      }
    }
    DFH_HIP(hipStreamSynchronize(B));
    auto t1 = std::chrono::steady_clock::now();
    DFH_HIP(hipDeviceSynchronize());
    auto t2 = std::chrono::steady_clock::now();
    ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return DFH_OK;
  };
  double m[2];
  DFH_TRY(run(true, false, m));  out_ms[0] = m[1];            // big alone
  DFH_TRY(run(false, true, m));  out_ms[1] = m[1];            // small alone
  DFH_TRY(run(true, true, m));   out_ms[2] = m[0];            // small-stream completion time when both run
  out_ms[3] += m[1] * 1e6;                                    // total together (packed: ms*1e6 + prio)
  return DFH_OK;
}

// Diagnostics hook: achievable pure-write HBM bandwidth (the kernel-matrix build is write-only).
__global__ void k_dbg_fill16(double2_t* p, long n2, double v) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const double2_t vv = (double2_t){v, v};
  for (; i < n2; i += stride) p[i] = vv;
}
__global__ void k_dbg_copy16(const double2_t* __restrict__ s, double2_t* __restrict__ d, long n2) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n2; i += stride) d[i] = s[i];
}
extern "C" int dfh_debug_write_bw(dfh_ctx* ctx, double gbytes, double* out /*[3]: fill16 TB/s, memset TB/s, copy TB/s (r+w)*/) {
  DFH_ARG(ctx && out && gbytes > 0.01 && gbytes < 16);
  const long n2 = (long)(gbytes * 1e9 / 16);
  double2_t *a = nullptr, *b = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n2 * 16, (void**)&a));
  DFH_TRY(scratch_get(ctx, SCR_KCT2, (size_t)n2 * 16, (void**)&b));
  hipEvent_t e0, e1;
  DFH_HIP(hipEventCreate(&e0)); DFH_HIP(hipEventCreate(&e1));
  float ms;
  for (int grid : {2048, 8192}) {
    hipLaunchKernelGGL(k_dbg_fill16, dim3(grid), dim3(256), 0, ctx->stream, a, n2, 1.0);
  }
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(k_dbg_fill16, dim3(4096), dim3(256), 0, ctx->stream, a, n2, 2.0);
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[0] = 5.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) DFH_HIP(hipMemsetAsync(a, 0, (size_t)n2 * 16, ctx->stream));
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[1] = 5.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(k_dbg_copy16, dim3(4096), dim3(256), 0, ctx->stream, a, b, n2);
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[2] = 5.0 * 2.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return DFH_OK;
}
#endif  // DFH_DEBUG_HOOKS
