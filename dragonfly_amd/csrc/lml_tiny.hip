// The whole tuning objective of a SMALL problem in one launch (k_lml_tiny, n <= TINY_MAX_N; k_lml_tiny64, n <= 63, on
// the 64 x 64 machinery of factor64.h), the pinned staging blob both share with the fused one-workgroup form of
// lml_wg.h (tiny_blob_build, tiny_arm_results, tiny_poll_results) and the host launcher.  The route chooser is lml.hip.
#include "lml.h"
#include <atomic>
#include <chrono>
#include <cstring>
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace {

#include "kerneval.h"   // ExpConsts, exp_fast, kern_eval, combine_nested, np_sumsq, TinyCand

// ---------------------------------------------------------------------------------------
// The whole tuning objective of SMALL problems in one launch (n <= TINY_MAX_N): workgroup c packs
// the inputs for candidate c's kernel, builds K + noise I, factors it (stable_cholesky's jitter
// ladder included) and solves for the log marginal likelihood -- all in LDS, nothing but the two
// result numbers goes back to HBM.  Sequential hyper-parameter searches (the reference's slice
// sampler, its PDOO) ask for a handful of such values per call thousands of times; with one
// launch per stage a call costs ~0.3 ms of launches and synchronisations, far more than the
// arithmetic of a 50 x 50 Cholesky.
// ---------------------------------------------------------------------------------------
struct TinyArgs {
  ExpConsts ec;
  const double* X; long ldx;       // [n x d] raw inputs (device)
  const char* blob;                // TinyCand[count] | kernel images | y[n] | pow10[16]
  long y_off, pow_off;
  int n, count, allow_jitter;
  int direct;                      // blob and out are host memory mapped into the device (small groups: no copies)
#ifdef DFH_DEBUG_HOOKS
  long long* stamps;               // diagnostics (DFH_TINY_STAMPS=1): [count][16] s_memrealtime (100 MHz) of k_lml_tiny64's phases
#endif
  double* out;                     // [count][4] = {sum log L_ii, |L^-1 (y - m)|^2, jitter power or -100, status}
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower, j <= i

__global__ __launch_bounds__(256) void k_lml_tiny(TinyArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int c = blockIdx.x, tid = threadIdx.x, n = a.n;
  const TinyCand cand = reinterpret_cast<const TinyCand*>(a.blob)[c];
  const char* image = a.blob + cand.image;
  const int P = cand.P, n_parts = cand.n_parts;
  // kernel image sections (blob_layout): parts | bw | cols | lcols
  const size_t off_bw = (sizeof(PartDev) * n_parts + 15) & ~size_t(15);
  const size_t off_cols = off_bw + ((sizeof(double) * (P ? P : 1) + 15) & ~size_t(15));
  const PartDev* parts_g = reinterpret_cast<const PartDev*>(image);
  __shared__ PartDev parts[TINY_MAX_PARTS];          // the Gram loop reads them per entry: keep them off the global-load path
  for (int q = tid; q < n_parts * (int)(sizeof(PartDev) / sizeof(int)); q += 256)
    reinterpret_cast<int*>(parts)[q] = reinterpret_cast<const int*>(parts_g)[q];
  const double* bw = reinterpret_cast<const double*>(image + off_bw);
  const int* cols = reinterpret_cast<const int*>(image + off_cols);
  const double* y = reinterpret_cast<const double*>(a.blob + a.y_off);
  const double* pow10 = reinterpret_cast<const double*>(a.blob + a.pow_off);

  double* A = lds;                                   // packed lower triangle of the (n+1) x (n+1) system
  double* Xp = A + (n + 1) * (n + 2) / 2;            // [n][P]
  double* Np = Xp + n * P;                           // [n][n_parts]
  __shared__ int s_fail;
  __shared__ double s_pivot;

  // get_scaled_repr (kernel.py:179-181) and the squared row norms (general_utils.py:66-67)
  for (int idx = tid; idx < n * P; idx += 256) {
    const int row = idx / P, pc = idx - row * P;
    const int col = cols[pc];
    Xp[idx] = col >= 0 ? a.X[(long)row * a.ldx + col] / bw[pc] : 0.0;
  }
  __syncthreads();
  for (int idx = tid; idx < n * n_parts; idx += 256) {
    const int row = idx / n_parts, part = idx - row * n_parts;
    const PartDev& pd = parts[part];
    int nreal = 0;
    for (int q = 0; q < pd.kc; ++q) nreal += cols[pd.poff + q] >= 0;
    Np[idx] = np_sumsq(Xp + row * P + pd.poff, nreal);
  }
  __syncthreads();

  const int tx = tid & 15, ty = tid >> 4;
  double max_diag = 0.0;                             // max(diag(K + noise I)), for the ladder
  int power = -100;                                  // -100: no jitter needed
  for (int attempt = 0; attempt < 17; ++attempt) {
    double jitter = 0.0;
    if (attempt > 0) {
      power = attempt - 12;                          // -11 ... 4 (general_utils.py:183-203)
      jitter = pow10[attempt - 1] * max_diag;
    }
    // K + noise I (+ jitter I), lower triangle; row n of the system is y - m
    for (int i = ty; i < n; i += 16) {
      for (int j = tx; j <= i; j += 16) {
        double res = cand.multi ? (cand.product ? cand.outer : 0.0) : 0.0;
        double fsum = 0.0;
        for (int part = 0; part < n_parts; ++part) {
          const PartDev& pd = parts[part];
          const double* xi = Xp + i * P + pd.poff;
          const double* xj = Xp + j * P + pd.poff;
          double dot = 0.0;
          for (int q = 0; q < pd.kc; ++q) dot = fma(xi[q], xj[q], dot);
          double dsq = (Np[j * n_parts + part] + Np[i * n_parts + part]) - 2.0 * dot;   // general_utils.py:66-68
          dsq = dsq < 0.0 ? 0.0 : dsq;
          const double kv = kern_eval(pd, dsq, a.ec);
          if (!cand.multi) res = kv;
          else if (!cand.product) res = res + kv;
          else combine_nested(pd, kv, res, fsum);          // (a plain factor: res * kv)
        }
        if (cand.multi && !cand.product) res = cand.outer * res;
        if (i == j) {
          res += cand.noise;                         // gp_core.py:843
          if (attempt > 0) res += jitter;            // M + diag_noise * np.eye(n)
        }
        A[tri(i, j)] = res;
      }
    }
    for (int j = tid; j < n; j += 256) A[tri(n, j)] = y[j] - cand.mean;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    if (attempt == 0) {                              // np.diag(M).max() of the un-jittered matrix
      double m = -INFINITY;
      bool any_nan = false;
      for (int i = 0; i < n; ++i) { const double v = A[tri(i, i)]; any_nan |= (v != v); m = v > m ? v : m; }
      max_diag = any_nan ? NAN : m;
    }
    // Left-looking Cholesky in panels of four columns; the extra row turns into z = L^-1 (y - m)
    // along the way.  Two threads per row.  For a panel starting at k0 the bulk of the work --
    // b[c] = sum_{j<k0} L[i][j] L[k0+c][j], c = 0..3 -- is one pass over the row: each L[i][j]
    // (a per-lane LDS load) feeds four FMAs, the four panel rows are broadcasts; nothing is stored
    // inside the pass.  The four columns are then finished one after the other from registers:
    // v = A[i][k] - b[c] - sum_{c'<c} L[i][k0+c'] L[k][k0+c'], pivot, scale -- two barriers each.
    const int half = tid & 1, slot = tid >> 1;
    bool failed = false;
    for (int k0 = 0; k0 < n && !failed; k0 += 4) {
      const int width = n - k0 < 4 ? n - k0 : 4;
      const int j0 = half ? (k0 + 1) / 2 : 0, j1 = half ? k0 : (k0 + 1) / 2;
      const double* prow[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) prow[c] = A + tri(k0 + (c < width ? c : 0), 0);
      // this thread's rows: i0 = k0 + slot and, only while more than 128 rows are left, i0 + 128
      double bulk[2][4], mine[2][4];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int i = k0 + slot + 128 * r;
#pragma unroll
        for (int c = 0; c < 4; ++c) { bulk[r][c] = 0.0; mine[r][c] = 0.0; }
        if (i > n) continue;
        const double* rowi = A + tri(i, 0);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        int j = j0;
        for (; j + 2 <= j1; j += 2) {
          const double x = rowi[j], y2 = rowi[j + 1];
          s0 = fma(x, prow[0][j], s0); s1 = fma(x, prow[1][j], s1);
          s2 = fma(x, prow[2][j], s2); s3 = fma(x, prow[3][j], s3);
          t0 = fma(y2, prow[0][j + 1], t0); t1 = fma(y2, prow[1][j + 1], t1);
          t2 = fma(y2, prow[2][j + 1], t2); t3 = fma(y2, prow[3][j + 1], t3);
        }
        if (j < j1) {
          const double x = rowi[j];
          s0 = fma(x, prow[0][j], s0); s1 = fma(x, prow[1][j], s1);
          s2 = fma(x, prow[2][j], s2); s3 = fma(x, prow[3][j], s3);
        }
        s0 += t0; s1 += t1; s2 += t2; s3 += t3;
        bulk[r][0] = s0 + __shfl_xor(s0, 1, 64); bulk[r][1] = s1 + __shfl_xor(s1, 1, 64);
        bulk[r][2] = s2 + __shfl_xor(s2, 1, 64); bulk[r][3] = s3 + __shfl_xor(s3, 1, 64);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= width || failed) continue;            // uniform
        const int k = k0 + c;
        const double* rowk = A + tri(k, 0);
        double v[2] = {0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int i = k0 + slot + 128 * r;
          if (i < k || i > n) continue;                // rows above this column's diagonal are done
          double acc = A[tri(i, k)] - bulk[r][c];
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            if (cc < c) acc -= mine[r][cc] * rowk[k0 + cc];
          v[r] = acc;
          if (i == k && half == 0) s_pivot = acc;
        }
        __syncthreads();                               // the pivot is published; row k has been read
        const double pivot = s_pivot;
        if (!(pivot > 0.0)) {                          // not positive definite (or NaN): uniform
          if (tid == 0) s_fail = 1;
          failed = true;
          continue;
        }
        const double lkk = sqrt(pivot);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int i = k0 + slot + 128 * r;
          if (i < k || i > n) continue;
          const double lik = (i == k) ? lkk : v[r] / lkk;
          mine[r][c] = lik;
          if (half == 0) A[tri(i, k)] = lik;
        }
        __syncthreads();
      }
    }
    __syncthreads();
    if (!s_fail) break;
    __syncthreads();
    if (!a.allow_jitter || attempt == 16) { power = attempt == 16 ? 99 : 98; break; }   // status below
  }

  double* out = a.out + 4 * (long)c;
  if (s_fail) {
    if (tid == 0) tiny_publish(out, a.direct != 0, NAN, NAN, (double)power, power == 98 ? 1.0 : 2.0);
    return;
  }
  double ld = 0.0, zz = 0.0;
  for (int i = tid; i < n; i += 256) {
    ld += log(A[tri(i, i)]);
    const double z = A[tri(n, i)];
    zz = fma(z, z, zz);
  }
  for (int o = 32; o > 0; o >>= 1) { ld += __shfl_down(ld, o, 64); zz += __shfl_down(zz, o, 64); }
  __shared__ double s_ld[4], s_zz[4];
  if ((tid & 63) == 0) { s_ld[tid >> 6] = ld; s_zz[tid >> 6] = zz; }
  __syncthreads();
  if (tid == 0)
    tiny_publish(out, a.direct != 0, (s_ld[0] + s_ld[1]) + (s_ld[2] + s_ld[3]), (s_zz[0] + s_zz[1]) + (s_zz[2] + s_zz[3]),
                 (double)power, 0.0);
}


#include "factor64.h"   // factor64's owner / consumer steps (shared with chol.hip and lml_wg.h)

// ---------------------------------------------------------------------------------------
// The same objective for n <= 63 with the factorisation on the 64 x 64 machinery of chol.hip (round 6).
// k_lml_tiny's column loop costs two workgroup barriers, an LDS round trip, a square root and a division per
// column, ~1100 cycles each: 39 us for n = 50 on an otherwise idle device (profiles/r06_small_calls_before.txt), most
// of a slice sampler's call.  Here the system [[K + s2 I, .], [(y - m)^T, 1]] is staged as ONE 64 x 64 tile (identity
// below row n) and factored by the four waves without barriers -- the owner chain of f64_owner_step is ~225 cycles
// per column -- and only as far as column n - 1: row n of the factor, z = L^-1 (y - m), is final in column k as soon as
// column k is, so the augmented row never has to be a pivot, and the waves whose sixteen columns lie beyond n - 1 sit
// the factorisation out.  Everything else -- packing, Gram entries, the jitter ladder, the results -- is k_lml_tiny's.
// ---------------------------------------------------------------------------------------
#ifdef DFH_DEBUG_HOOKS
#define TSTAMP(a, e) do { if ((a).stamps && threadIdx.x == 0) (a).stamps[(long)blockIdx.x * 16 + (e)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TSTAMP(a, e) do {} while (0)
#endif
constexpr size_t TINY64_FIXED_LDS = sizeof(double) * (PB * SPP + PB * PB + 3 * PB * 17);

__global__ __launch_bounds__(256, 1) void k_lml_tiny64(TinyArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int c = blockIdx.x, tid = threadIdx.x, n = a.n;
  const int lane = tid & 63, w = tid >> 6;
  TSTAMP(a, 0);
  const TinyCand cand = reinterpret_cast<const TinyCand*>(a.blob)[c];
  const char* image = a.blob + cand.image;
  const int P = cand.P, n_parts = cand.n_parts;
  const size_t off_bw = (sizeof(PartDev) * n_parts + 15) & ~size_t(15);
  const size_t off_cols = off_bw + ((sizeof(double) * (P ? P : 1) + 15) & ~size_t(15));
  const PartDev* parts_g = reinterpret_cast<const PartDev*>(image);
  __shared__ PartDev parts[TINY_MAX_PARTS];
  for (int q = tid; q < n_parts * (int)(sizeof(PartDev) / sizeof(int)); q += 256)
    reinterpret_cast<int*>(parts)[q] = reinterpret_cast<const int*>(parts_g)[q];
  const double* bw = reinterpret_cast<const double*>(image + off_bw);
  const int* cols = reinterpret_cast<const int*>(image + off_cols);
  const double* y = reinterpret_cast<const double*>(a.blob + a.y_off);
  const double* pow10 = reinterpret_cast<const double*>(a.blob + a.pow_off);

  double* stage = lds;                               // [64][SPP] the system, lower triangle
  double* ring = stage + PB * SPP;             // [64][64] published columns
  double* tbuf0 = ring + PB * PB;                    // 3 x [64][17] layout buffers of waves 1..3
  double* Xp = tbuf0 + 3 * PB * 17;                  // [n][P]
  double* Np = Xp + n * P;                           // [n][n_parts]
  __shared__ int s_badv[4];
  __shared__ int s_ring_timeout;
  __shared__ double s_ld[4], s_zz[4];

  TSTAMP(a, 1);
  // identity below row n, zero above the diagonal; row n = y - m with a unit diagonal
  for (int idx = tid; idx < PB * PB; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    stage[i * SPP + j] = (i == j && i >= n) ? 1.0 : 0.0;
  }
  for (int idx = tid; idx < n * P; idx += 256) {
    const int row = idx / P, pc = idx - row * P;
    const int col = cols[pc];
    Xp[idx] = col >= 0 ? a.X[(long)row * a.ldx + col] / bw[pc] : 0.0;
  }
  __syncthreads();
  for (int idx = tid; idx < n * n_parts; idx += 256) {
    const int row = idx / n_parts, part = idx - row * n_parts;
    const PartDev& pd = parts[part];
    int nreal = 0;
    for (int q = 0; q < pd.kc; ++q) nreal += cols[pd.poff + q] >= 0;
    Np[idx] = np_sumsq(Xp + row * P + pd.poff, nreal);
  }
  for (int j = tid; j < n; j += 256) stage[n * SPP + j] = y[j] - cand.mean;
  __syncthreads();

  TSTAMP(a, 2);
  double max_diag = 0.0;
  int power = -100;
  bool failed = false;
  double av[16];
  for (int attempt = 0; attempt < 17; ++attempt) {
    double jitter = 0.0;
    if (attempt > 0) {
      if (attempt == 1) {                            // np.diag(M).max() of the un-jittered matrix, still staged
        double m = -INFINITY;
        bool any_nan = false;
        for (int i = 0; i < n; ++i) { const double v = stage[i * SPP + i]; any_nan |= (v != v); m = v > m ? v : m; }
        max_diag = any_nan ? NAN : m;
        __syncthreads();                             // every thread has read the old diagonal
      }
      power = attempt - 12;                          // -11 ... 4 (general_utils.py:183-203)
      jitter = pow10[attempt - 1] * max_diag;
    }
    // K + noise I (+ jitter I: M + diag_noise * np.eye(n), general_utils.py:190), lower triangle   (gp_core.py:843)
    tiny_gram_lower(cand, parts, n_parts, Xp, P, Np, n, a.ec, [&](int i, int j, double v) {
      if (i == j) {
        v += cand.noise;                             // gp_core.py:843
        if (attempt > 0) v += jitter;                // M + diag_noise * np.eye(n)
      }
      stage[i * SPP + j] = v;
    });
    if (tid < PB) ring[tid * PB] = 0.0;              // row-0 entries double as the "published" flags
    if (tid == 0) s_ring_timeout = 0;
    __syncthreads();
    TSTAMP(a, 3);
    double* tbuf = tbuf0 + (w > 0 ? (w - 1) : 0) * PB * 17;
    const int bad = tiny64_factor(av, lane, w, stage, tbuf, ring, n - 1, &s_ring_timeout);
    if (lane == 0) s_badv[w] = (bad >= 0 && bad < n) ? bad : -1;
    __syncthreads();
    TSTAMP(a, 4);
    failed = s_badv[0] >= 0 || s_badv[1] >= 0 || s_badv[2] >= 0 || s_badv[3] >= 0 || s_ring_timeout != 0;
    if (!failed) break;
    if (!a.allow_jitter || attempt == 16) { power = attempt == 16 ? 99 : 98; break; }
    __syncthreads();                                 // the verdict is read before the next attempt rewrites it
  }

  double* out = a.out + 4 * (long)c;
  if (failed) {
    if (tid == 0) tiny_publish(out, a.direct != 0, NAN, NAN, (double)power, power == 98 ? 1.0 : 2.0);
    return;
  }
  // sum log L_kk (lane k of the wave that owns column k) and z.z (row n = lane n)
  double lkk = 1.0, zz = 0.0;                        // (one logarithm per lane: log(1) = 0 in the lanes that own no column)
  if (16 * w <= n - 1) {
#pragma unroll
    for (int kl = 0; kl < 16; ++kl) {
      const int k = 16 * w + kl;
      if (k < n) {
        lkk = (lane == k) ? av[kl] : lkk;
        if (lane == n) zz = fma(av[kl], av[kl], zz);
      }
    }
  }
  double ldv = log(lkk);
  for (int o = 32; o > 0; o >>= 1) { ldv += __shfl_down(ldv, o, 64); zz += __shfl_down(zz, o, 64); }
  if (lane == 0) { s_ld[w] = ldv; s_zz[w] = zz; }
  __syncthreads();
  TSTAMP(a, 5);
  if (tid == 0)
    tiny_publish(out, a.direct != 0, (s_ld[0] + s_ld[1]) + (s_ld[2] + s_ld[3]), (s_zz[0] + s_zz[1]) + (s_zz[2] + s_zz[3]),
                 (double)power, 0.0);
  TSTAMP(a, 6);
}


}  // namespace


int tiny_blob_build(dfh_ctx* ctx, const KernDev* kds, int count, int64_t n, const double* y_host,
                    const double* noise_vars, const double* mean_consts, TinyBlob* tb) {
  std::vector<size_t> image_off((size_t)count);
  size_t at = ((sizeof(TinyCand) * (size_t)count) + 15) & ~size_t(15);
  int Pmax = 1, parts_max = 1;
  for (int c = 0; c < count; ++c) {
    image_off[c] = at;
    at += kerndev_blob_bytes(kds[c]);
    Pmax = std::max(Pmax, kds[c].P);
    parts_max = std::max(parts_max, kds[c].n_parts);
  }
  const size_t y_off = at;
  at += sizeof(double) * (size_t)n;
  const size_t pow_off = at;
  at += sizeof(double) * 16;
  // blob and results go through pinned staging memory: two asynchronous copies and one
  // synchronisation per call instead of two staged, blocking ones
  const size_t res_off = (at + 63) & ~size_t(63);
  void* pinned = nullptr;
  DFH_TRY(pinned_get(ctx, res_off + sizeof(double) * 4 * (size_t)count, &pinned));
  char* host_blob = static_cast<char*>(pinned);
  std::memset(host_blob, 0, at);
  TinyCand* cands = reinterpret_cast<TinyCand*>(host_blob);
  for (int c = 0; c < count; ++c) {
    cands[c].image = (long)image_off[c];
    cands[c].P = kds[c].P; cands[c].n_parts = kds[c].n_parts;
    cands[c].multi = kds[c].multi ? 1 : 0; cands[c].product = kds[c].product ? 1 : 0;
    cands[c].outer = kds[c].outer_scale;
    cands[c].noise = noise_vars[c];
    cands[c].mean = mean_consts ? mean_consts[c] : 0.0;
    kerndev_blob_fill(kds[c], host_blob + image_off[c]);
  }
  std::memcpy(host_blob + y_off, y_host, sizeof(double) * (size_t)n);
  double* pw = reinterpret_cast<double*>(host_blob + pow_off);
  static const std::vector<double> pow10_table = []() {                 // 10 ** diag_noise_power, once per process
    std::vector<double> t(16);
    for (int p = -11; p < 5; ++p) t[(size_t)(p + 11)] = pow(10.0, (double)p);
    return t;
  }();
  std::memcpy(pw, pow10_table.data(), sizeof(double) * 16);
  tb->host = host_blob; tb->bytes = at; tb->y_off = y_off; tb->pow_off = pow_off;
  tb->res = reinterpret_cast<double*>(host_blob + res_off);
  tb->Pmax = Pmax; tb->parts_max = parts_max;
  return DFH_OK;
}

// Host side of a direct call's results: the kernel's status words (res[4 c + 3]; the kernel's status is 0, 1 or 2) set
// to -1.0, "not there yet", before the launch and polled in the pinned buffer after it; past the budget the stream is
// synchronised like any other call and a kernel that never wrote is an error.
void tiny_arm_results(volatile double* vres, int count) {
  for (int c = 0; c < count; ++c) vres[4 * c + 3] = -1.0;
}

int tiny_poll_results(dfh_ctx* ctx, volatile double* vres, int count, const char* what) {
  bool all_in = false;
  const auto t_start = std::chrono::steady_clock::now();
  for (long spin = 0; !all_in; ++spin) {
    all_in = true;
    for (int c = 0; c < count; ++c) all_in = all_in && vres[4 * c + 3] != -1.0;
    if (all_in) break;
    if ((spin & 1023) == 1023 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > 0.25) break;
  }
  if (!all_in) {
    DFH_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < count; ++c)
      if (vres[4 * c + 3] == -1.0) { dfh_set_error("%s: no result for candidate %d", what, c); return DFH_ERR_HIP; }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return DFH_OK;
}

// Returns DFH_ERR_NOT_PD / DFH_ERR_JITTER as the one-fit path would.
int lml_tiny_batch(dfh_ctx* ctx, const KernDev* kds, int count, const double* dX, int64_t n, int64_t ldx,
                   const double* y_host, const double* noise_vars, const double* mean_consts,
                   bool allow_jitter, double* logdet_dot, int32_t* powers) {
  TinyBlob tb;
  DFH_TRY(tiny_blob_build(ctx, kds, count, n, y_host, noise_vars, mean_consts, &tb));
  char* host_blob = tb.host;
  const size_t at = tb.bytes, y_off = tb.y_off, pow_off = tb.pow_off;
  const int Pmax = tb.Pmax, parts_max = tb.parts_max;
  double* res = tb.res;
  // A handful of candidates (a slice sampler's or a tree search's call: gp_core.py:551-574 under sampling/slice.py,
  // utils/doo.py) is latency, not work: the kernel reads the descriptors straight from the pinned buffer (mapped into
  // the device: a few hundred bytes over PCIe) and writes its four numbers per candidate straight back into it, status
  // word last, while the host polls that word -- one launch, no copy, no stream synchronisation.  DFH_LML_DIRECT=0: off;
  // =N: groups of up to N candidates (default 16).
  static const int direct_max = env_int("DFH_LML_DIRECT", 16);
  const bool direct = count <= direct_max && at <= (size_t)32768 && !ctx->timing;
  void* d_blob = nullptr;
  double* d_out = nullptr;
  if (!direct) {
    DFH_TRY(scratch_get(ctx, SCR_AUG2, at, &d_blob));
    DFH_TRY(scratch_get(ctx, SCR_OUT2, sizeof(double) * 4 * (size_t)count, (void**)&d_out));
    DFH_HIP(hipMemcpyAsync(d_blob, host_blob, at, hipMemcpyHostToDevice, ctx->stream));
  }
  TinyArgs a;
  a.ec = kExpConsts;
  a.X = dX; a.ldx = ldx;
  a.blob = direct ? host_blob : static_cast<const char*>(d_blob);
  a.y_off = (long)y_off; a.pow_off = (long)pow_off;
  a.n = (int)n; a.count = count; a.allow_jitter = allow_jitter ? 1 : 0;
  a.direct = direct ? 1 : 0;
  a.out = direct ? res : d_out;
#ifdef DFH_DEBUG_HOOKS
  static long long* d_stamps = nullptr;
  static const bool want_stamps = getenv("DFH_TINY_STAMPS") != nullptr;
  if (want_stamps && !d_stamps) DFH_HIP(hipMalloc((void**)&d_stamps, 64 * 16 * 8));
  a.stamps = (want_stamps && count <= 64) ? d_stamps : nullptr;
#endif
  volatile double* vres = res;
  if (direct) tiny_arm_results(vres, count);
  static bool attr_set[DFH_MAX_DEVICES] = {false};
  if (!attr_set[ctx->device]) {
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lml_tiny), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 4096));      // static LDS (kernel parts, flags) takes ~2 KB
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lml_tiny64), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 4096));
    attr_set[ctx->device] = true;
  }
  // n <= 63: the system is one 64 x 64 tile for the barrier-free factorisation (k_lml_tiny64); DFH_LML_TINY64=0: k_lml_tiny
  static const bool tiny64 = env_flag("DFH_LML_TINY64", true);
  if (tiny64 && n <= TINY64_MAX_N) {
    const size_t lds_bytes = TINY64_FIXED_LDS + sizeof(double) * ((size_t)n * Pmax + (size_t)n * parts_max);
    hipLaunchKernelGGL(k_lml_tiny64, dim3((unsigned)count), dim3(256), lds_bytes, ctx->stream, a);
  } else {
    const size_t lds_bytes = sizeof(double) * ((size_t)(n + 1) * (n + 2) / 2 + (size_t)n * Pmax + (size_t)n * parts_max);
    hipLaunchKernelGGL(k_lml_tiny, dim3((unsigned)count), dim3(256), lds_bytes, ctx->stream, a);
  }
  DFH_LAUNCH_CHECK();
  if (direct) {
    // (a kernel of this size runs tens of microseconds; a ladder over seventeen attempts a millisecond)
    DFH_TRY(tiny_poll_results(ctx, vres, count, "k_lml_tiny"));
  } else {
    DFH_HIP(hipMemcpyAsync(res, d_out, sizeof(double) * 4 * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    DFH_HIP(hipStreamSynchronize(ctx->stream));
  }
#ifdef DFH_DEBUG_HOOKS
  if (a.stamps) {
    static long long acc[8] = {0}; static long calls = 0;
    long long hs[16];
    DFH_HIP(hipMemcpy(hs, d_stamps, sizeof(hs), hipMemcpyDeviceToHost));
    for (int e = 0; e < 6; ++e) acc[e] += hs[e + 1] - hs[e];
    if (++calls % 1000 == 0) {
      fprintf(stderr, "[tiny64 stamps, mean of 1000, us] cand %.2f | descr+fill %.2f | pack+norms %.2f | gram %.2f | factor %.2f | reduce %.2f | publish %.2f\n",
              0.0, acc[0] / 1e5, acc[1] / 1e5, acc[2] / 1e5, acc[3] / 1e5, acc[4] / 1e5, acc[5] / 1e5);
      for (int e = 0; e < 8; ++e) acc[e] = 0;
    }
  }
#endif
  for (int c = 0; c < count; ++c) {
    const int status = (int)res[4 * c + 3];
    if (status == 1) {
      dfh_set_error("Matrix is not positive definite (candidate %d)", c);
      return DFH_ERR_NOT_PD;
    }
    if (status == 2) {
      dfh_set_error("Could not compute Cholesky decomposition despite adding jitter to the diagonal (candidate %d). "
                    "This is likely because the M is not positive semi-definite or has infinities/nans.", c);
      return DFH_ERR_JITTER;
    }
    logdet_dot[2 * c] = res[4 * c];
    logdet_dot[2 * c + 1] = res[4 * c + 1];
    const int pwr = (int)res[4 * c + 2];
    if (powers) powers[c] = pwr == -100 ? INT32_MIN : pwr;
  }
  return DFH_OK;
}
