// Gradient of the log marginal likelihood of a fitted GP (gp_core.py:229-240) in the tuner's coordinates: log scale,
// log bandwidths, log noise variance, constant mean.  With A = K + (noise_var + jitter) I as factored, alpha as stored
// and W = alpha alpha^T - A^-1, every component is half a trace of W times a derivative of K.  The reference forms one
// n x n derivative matrix and two triangular solves per parameter; here all parameters share one inverse and one pass:
//   A^-1          Z = L^-T by trsm_rows on identity rows (a row block at a time, on the trailing factor: the rows of
//                 L^-T are zero before their own column), then Z Z^T by the NT GEMM, lower tiles only
//   tr(A^-1 K)    for the scale component, NOT as sum_ij (A^-1)_ij K_ij: on a fit that took jitter the entries of A^-1
//                 reach 1 / jitter, and their rounding alone is 1e-6 of a sum that is below n.  Instead V = K L^-T (the
//                 Gram matrix as the fit built it, trsm_rows on its rows) and sum_ij V_ij Z_ij = tr(L^-1 K L^-T): the
//                 entries of V are O(sqrt(scale)), and the factor's backward error cancels against the K it came from
//   k_lml_grad_F  one pass over the lower triangle in 64 x 64 tiles: dsq as the Gram kernels form it, K, dK/d(dsq), W;
//                 F = -2 W dK/d(dsq) written to both triangles; per-workgroup partial sums of alpha_i alpha_j K_ij and
//                 of W's diagonal
//   k_lml_grad_FX r = F 1 and G = F Xp, a wave per row (k_lml_grad_rowdot, the same way, for the rows of V o Z)
//   k_lml_grad_finish   the bandwidth components sum_i xs_ic (xs_ic r_i - G_ic) = 1/2 sum_ij F_ij s_c,ij (F is
//                 symmetric), the scale and noise components from the partial sums, sum alpha
// Additive and product kernels of SE / Matern parts (dfh_gp_lml_grad_groups): K = scale sum_g k_g or scale prod_g k_g, each
// part on its own packed columns.  k_lml_grad_F_parts is the same tile pass with every part's dsq_h formed as the
// multi-part Gram kernels form it (the part's columns, the part's own norms) and
//   F_g = -2 W scale dk_g/d(dsq_g)                         (additive)
//   F_g = -2 W scale (prod_{h != g} k_h) dk_g/d(dsq_g)     (product: the other parts' values multiplied, never K / k_g)
// one pass per group g into the one F buffer, each followed by k_lml_grad_FX on the group's packed columns alone; the
// row sums of the groups sit side by side ([n_parts][n]) for k_lml_grad_finish.  The scale component takes the whole K.
// Every sum runs in a fixed order: no floating-point atomics, the same bits on every call.
#include "gp.h"
#include <algorithm>

namespace {

#include "kerneval.h"   // ExpConsts, exp_fast, sqrt_fast, kern_eval

constexpr int GT = 64;             // tile edge
constexpr int GKC = 16;            // packed columns per LDS chunk
constexpr int GKP = GKC + 2;       // operand row stride (doubles)
constexpr int GSR = 32;            // rows per staging pass
constexpr int GSP = GT + 2;        // staging row stride: 16-byte aligned rows
constexpr int GOPER = 2 * GT * GKP;
constexpr int GSTAGE = GSR * GSP;
constexpr int GBODY = GOPER > GSTAGE ? GOPER : GSTAGE;

struct GradArgs {
  ExpConsts ec;
  const double* Xp; const double* Np;    // packed scaled inputs [n][P], squared row norms per part [n][n_parts]
  const double* alpha;                   // [n]
  const double* Ainv; long lda;          // A^-1, tiles on and below the diagonal
  double* F; long ldf;                   // out: both triangles (ldf even, F 16-byte aligned)
  const PartDev* parts;                  // the kernel's parts (k_lml_grad_F: its one part)
  int n, P;
  int n_parts, product, group;           // (k_lml_grad_F_parts) parts summed or multiplied; the part F is the derivative in
  double outer;                          // (k_lml_grad_F_parts) the outer scale
  double zero_tol;                       // (k_lml_grad_F) dsq <= zero_tol * (na + nb) is the rounding of its own formula: counts as 0
  double* part;                          // out: [tiles][2] partial sums of alpha_i alpha_j K_ij (both triangles) and of W's diagonal
};

// F = -2 W dK/d(dsq) of one entry from its kernel value's pieces.  SE: dK/d(dsq) = -K/2.  Matern (kernel.py:259-270)
// with dist = sqrt(dsq), m = s8 dist, K = C u(m) exp(-s2 dist), s8 = 2 s2: dK/d(dist) = C exp(-s2 dist) s2 (2 u' - u),
// and 2 u' - u is -c0, -c0 m, -m (c0 m + c1 - 4 c0) for nu = 1/2, 3/2, 5/2 (the constant terms cancel exactly, so they
// are never formed); dK/d(dsq) = dK/d(dist) / (2 dist).
__device__ __forceinline__ void grad_entry(const PartDev& pd, double dsq, const ExpConsts& ec, double& kv, double& dk2) {
  // kv = K, dk2 = -2 dK/d(dsq) (for dsq > 0)
  if (pd.kind == DFH_KERNEL_SE) {
    kv = pd.scale_c * exp_fast(-dsq / 2, ec);
    dk2 = kv;
    return;
  }
  const double dist = sqrt_fast(dsq);
  const double mult = pd.s8 * dist;
  const double e = pd.scale_c * (pd.gfac * exp_fast_neg(-pd.s2 * dist, ec));
  if (pd.p == 0) {
    kv = e * pd.coeff[0];
    dk2 = dsq > 0.0 ? e * pd.s2 * pd.coeff[0] / dist : 0.0;
  } else if (pd.p == 1) {
    kv = e * fma(pd.coeff[0], mult, pd.coeff[1]);
    dk2 = e * pd.s2 * pd.s8 * pd.coeff[0];
  } else {
    kv = e * fma(fma(pd.coeff[0], mult, pd.coeff[1]), mult, pd.coeff[2]);
    dk2 = e * pd.s2 * pd.s8 * fma(pd.coeff[0], mult, pd.coeff[1] - 4.0 * pd.coeff[0]);
  }
}

// tile (ti, tj), tj <= ti, of the lower-triangular enumeration
__device__ __forceinline__ void lower_tile(unsigned lin, unsigned& ti, unsigned& tj) {
  ti = (unsigned)((sqrt(8.0 * (double)lin + 1.0) - 1.0) * 0.5);
  while ((unsigned long long)ti * (ti + 1) / 2 > lin) --ti;
  while ((unsigned long long)(ti + 1) * (ti + 2) / 2 <= lin) ++ti;
  tj = lin - (unsigned)((unsigned long long)ti * (ti + 1) / 2);
}

// What ends a tile of either F kernel: the workgroup's two partial sums (each thread's share in s_wk, s_tr) to
// part[2 lin], and the tile in the accumulator registers to F -- staged stores as kernmat_sym_kernel's: passes [0, NH)
// the tile itself, [NH, 2 NH) its mirror image
__device__ __forceinline__ void finish_tile(const GradArgs& p, double4_t (&acc)[2][2], double s_wk, double s_tr, double* St,
                                            double* red, unsigned lin, long m0, long n0, bool diag_tile) {
  constexpr int WT = 2, WS = 32, NH = GT / GSR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  if (!diag_tile) s_wk *= 2.0;                           // the mirror tile's entries
  for (int off = 32; off > 0; off >>= 1) {
    s_wk += __shfl_down(s_wk, off, 64);
    s_tr += __shfl_down(s_tr, off, 64);
  }
  if (lane == 0) { red[wave] = s_wk; red[4 + wave] = s_tr; }
  const int npass = diag_tile ? NH : 2 * NH;
  for (int pass = 0; pass < npass; ++pass) {
    const bool mirror = pass >= NH;
    const int h = mirror ? pass - NH : pass;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
          const int irow = mirror ? (wn * WS + j * 16 + l15) : (wm * WS + i * 16 + l4 + 4 * r);
          const int icol = mirror ? (wm * WS + i * 16 + l4 + 4 * r) : (wn * WS + j * 16 + l15);
          if (irow / GSR == h) St[(irow - h * GSR) * GSP + icol] = acc[i][j][r];
        }
    __syncthreads();
    const long row_base = (mirror ? n0 : m0) + h * GSR;
    const long col_base = mirror ? m0 : n0;
    constexpr int RP = GT / 2;
#pragma unroll
    for (int q = 0; q < (GSR * RP) / 256; ++q) {
      const int idx = tid + 256 * q;
      const int r = idx / RP, c2 = (idx % RP) * 2;
      const long row = row_base + r, col = col_base + c2;
      if (row < p.n && col + 1 < p.n) {
        *reinterpret_cast<double2_t*>(p.F + row * p.ldf + col) = *reinterpret_cast<const double2_t*>(St + r * GSP + c2);
      } else if (row < p.n && col < p.n) {
        p.F[row * p.ldf + col] = St[r * GSP + c2];
      }
    }
  }
  if (tid == 0) {                                        // (red was written before the first barrier of the passes)
    p.part[2 * (long)lin] = (red[0] + red[1]) + (red[2] + red[3]);
    p.part[2 * (long)lin + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// the dot products of part `h` of the tile's rows with its columns (chunks of GKC packed columns through As / Bs), and
// the part's squared norms of both in na / nb; with h = 0 alpha of both in al_r / al_c as well
__device__ __forceinline__ void part_dots(const GradArgs& p, const PartDev& pd, int h, long m0, long n0, double* As, double* Bs,
                                          double* na, double* nb, double* al_r, double* al_c, double4_t (&acc)[2][2]) {
  constexpr int WT = 2, WS = 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const double* __restrict__ Xp = p.Xp;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < pd.kc; k0 += GKC) {
    const int kc = min(GKC, pd.kc - k0);
    const int kh = kc >> 1;
    __syncthreads();
    for (int idx = tid; idx < GT * kh; idx += 256) {
      const int r = idx / kh, c2 = (idx - r * kh) * 2;
      const long rowa = m0 + r, rowb = n0 + r;
      double2_t va = (double2_t){0.0, 0.0}, vb = (double2_t){0.0, 0.0};
      if (rowa < p.n) va = *reinterpret_cast<const double2_t*>(Xp + rowa * p.P + pd.poff + k0 + c2);
      if (rowb < p.n) vb = *reinterpret_cast<const double2_t*>(Xp + rowb * p.P + pd.poff + k0 + c2);
      *reinterpret_cast<double2_t*>(As + r * GKP + c2) = va;
      *reinterpret_cast<double2_t*>(Bs + r * GKP + c2) = vb;
    }
    if (k0 == 0) {
      if (tid < GT) {
        const long row = m0 + tid;
        na[tid] = row < p.n ? p.Np[row * p.n_parts + h] : 0.0;
        if (h == 0) al_r[tid] = row < p.n ? p.alpha[row] : 0.0;
      } else if (tid < 2 * GT) {
        const long row = n0 + tid - GT;
        nb[tid - GT] = row < p.n ? p.Np[row * p.n_parts + h] : 0.0;
        if (h == 0) al_c[tid - GT] = row < p.n ? p.alpha[row] : 0.0;
      }
    }
    __syncthreads();
    const double* as = As + (wm * WS + l15) * GKP + l4;
    const double* bs = Bs + (wn * WS + l15) * GKP + l4;
    for (int kk = 0; kk < kc; kk += 4) {
      double a[WT], b[WT];
#pragma unroll
      for (int t = 0; t < WT; ++t) a[t] = as[t * 16 * GKP + kk];
#pragma unroll
      for (int t = 0; t < WT; ++t) b[t] = bs[t * 16 * GKP + kk];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
}

// A^-1 of one entry of the matrix: an entry above the diagonal takes it from its mirror position (the product that made
// A^-1 wrote the lower tiles only); W = alpha_i alpha_j - A^-1, 0 outside the matrix
__device__ __forceinline__ double w_entry(const GradArgs& p, long grow, long gcol, double aa) {
  if (grow >= p.n || gcol >= p.n) return 0.0;
  const double ainv = (gcol > grow) ? p.Ainv[gcol * p.lda + grow] : p.Ainv[grow * p.lda + gcol];
  return aa - ainv;
}

#define GRAD_TILE_PROLOGUE()                                                                                \
  constexpr int WT = 2, WS = 32;                                                                            \
  __shared__ __attribute__((aligned(16))) double smem[GBODY + 4 * GT + 8];                                  \
  double* As = smem;                     /* [GT][GKP] */                                                    \
  double* Bs = As + GT * GKP;            /* [GT][GKP] */                                                    \
  double* na = smem + GBODY;             /* [GT] squared norms of the tile's rows / columns (of one part) */\
  double* nb = na + GT;                                                                                     \
  double* al_r = nb + GT;                /* [GT] alpha of the tile's rows / columns */                      \
  double* al_c = al_r + GT;                                                                                 \
  double* red = al_c + GT;               /* [8] */                                                          \
  double* St = smem;                     /* [GSR][GSP] staging, reuses the operand tiles */                 \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                               \
  const int wm = wave >> 1, wn = wave & 1;                                                                  \
  const int l15 = lane & 15, l4 = lane >> 4;                                                                \
  const unsigned lin = blockIdx.x;                                                                          \
  unsigned ti, tj;                                                                                          \
  lower_tile(lin, ti, tj);                                                                                  \
  const long m0 = (long)ti * GT, n0 = (long)tj * GT;                                                        \
  const ExpConsts& ec = p.ec

// A single SE / Matern kernel.  A kernel of its own beside k_lml_grad_F_parts: one part needs neither the running K nor
// the factor in front of the derivative in registers, and dfh_gp_lml_grad's arithmetic stays what it was.
__global__ __launch_bounds__(256) void k_lml_grad_F(GradArgs p) {
  GRAD_TILE_PROLOGUE();
  const PartDev& pd = p.parts[0];
  double4_t acc[WT][WT];
  part_dots(p, pd, 0, m0, n0, As, Bs, na, nb, al_r, al_c, acc);

  // distances -> F (in the accumulator registers) and this thread's share of the two sums
  double s_wk = 0.0, s_tr = 0.0;
#pragma unroll
  for (int i = 0; i < WT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = wm * WS + i * 16 + l4 + 4 * r;
      const long grow = m0 + lr;
      const double nai = na[lr], ali = al_r[lr];
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int lc = wn * WS + j * 16 + l15;
        const long gcol = n0 + lc;
        const double nbj = nb[lc];
        double dsq = (nbj + nai) - 2.0 * acc[i][j][r];
        dsq = dsq < 0.0 ? 0.0 : dsq;
        double kv, dk2;
        grad_entry(pd, dsq, ec, kv, dk2);
        const double aa = ali * al_c[lc];                // (0 outside the matrix: alpha is staged as 0 there)
        const double w = w_entry(p, grow, gcol, aa);
        s_wk += aa * kv;
        if (grow == gcol) s_tr += w;
        const bool zero = grow == gcol || dsq <= p.zero_tol * (nbj + nai);
        acc[i][j][r] = zero ? 0.0 : w * dk2;
      }
    }
  }
  finish_tile(p, acc, s_wk, s_tr, St, red, lin, m0, n0, ti == tj);
}

// An additive or product kernel of SE / Matern parts, F of part p.group.  res: K as kernmat_symmulti_kernel combines it
// (0 + k_1 + k_2 ..., the outer scale last; scale * k_1 * k_2 ...).  fac: -2 dK/d(dsq_g) -- additive scale * dk2_g;
// product scale * k_1 .. dk2_g .. k_P in the same order, so a factor that underflowed to 0 gives 0 and never 0 / 0.
// The zero-distance rule is part g's: (kc_g + 2) ulps of its own two norms (a kc_g-term dot product and the norms), and
// the diagonal.  Every pass forms the same K, so every pass writes the same two partial sums.
__global__ __launch_bounds__(256) void k_lml_grad_F_parts(GradArgs p) {
  GRAD_TILE_PROLOGUE();
  const bool product = p.product != 0;
  double4_t res[WT][WT], fac[WT][WT];
  {
    const double r0 = product ? p.outer : 0.0;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) { res[i][j] = (double4_t){r0, r0, r0, r0}; fac[i][j] = res[i][j]; }
  }
  for (int h = 0; h < p.n_parts; ++h) {
    const PartDev& pd = p.parts[h];
    double4_t acc[WT][WT];
    part_dots(p, pd, h, m0, n0, As, Bs, na, nb, al_r, al_c, acc);
    const bool mine = (h == p.group);
    const double zero_tol = (double)(pd.kc + 2) * 0x1p-52;
#pragma unroll
    for (int i = 0; i < WT; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm * WS + i * 16 + l4 + 4 * r;
        const double nai = na[lr];
#pragma unroll
        for (int j = 0; j < WT; ++j) {
          const int lc = wn * WS + j * 16 + l15;
          const double nbj = nb[lc];
          double dsq = (nbj + nai) - 2.0 * acc[i][j][r];
          dsq = dsq < 0.0 ? 0.0 : dsq;
          double kv, dk2;
          grad_entry(pd, dsq, ec, kv, dk2);
          if (m0 + lr == n0 + lc || dsq <= zero_tol * (nbj + nai)) dk2 = 0.0;
          if (product) {
            res[i][j][r] *= kv;
            fac[i][j][r] *= mine ? dk2 : kv;
          } else {
            res[i][j][r] += kv;
            if (mine) fac[i][j][r] = dk2;
          }
        }
      }
    }
  }

  double s_wk = 0.0, s_tr = 0.0;
#pragma unroll
  for (int i = 0; i < WT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = wm * WS + i * 16 + l4 + 4 * r;
      const long grow = m0 + lr;
      const double ali = al_r[lr];
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int lc = wn * WS + j * 16 + l15;
        const long gcol = n0 + lc;
        const double kv = product ? res[i][j][r] : p.outer * res[i][j][r];
        const double dk2 = product ? fac[i][j][r] : p.outer * fac[i][j][r];
        const double aa = ali * al_c[lc];
        const double w = w_entry(p, grow, gcol, aa);
        s_wk += aa * kv;
        if (grow == gcol) s_tr += w;
        fac[i][j][r] = dk2 == 0.0 ? 0.0 : w * dk2;       // (as k_lml_grad_F: a zero-distance pair adds exactly 0)
      }
    }
  }
  finish_tile(p, fac, s_wk, s_tr, St, red, lin, m0, n0, ti == tj);
}
#undef GRAD_TILE_PROLOGUE

// r[i] = sum_j F[i][j], G[i][c] = sum_j F[i][j] Xp[j][c] for the packed columns [c_lo, c_hi) (one part's; every column of
// a single kernel): a wave per row, four packed columns per pass over the row (parts are multiples of 4 wide; the row
// stays in the caches between the passes)
__global__ __launch_bounds__(256) void k_lml_grad_FX(const double* __restrict__ F, long ldf, const double* __restrict__ Xp,
                                                     int P, int c_lo, int c_hi, int n, double* __restrict__ r,
                                                     double* __restrict__ G) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const double* f = F + row * ldf;
  for (int c0 = c_lo; c0 < c_hi; c0 += 4) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, rs = 0.0;
    for (int j = lane; j < n; j += 64) {
      const double fv = f[j];
      const double2_t x01 = *reinterpret_cast<const double2_t*>(Xp + (long)j * P + c0);
      const double2_t x23 = *reinterpret_cast<const double2_t*>(Xp + (long)j * P + c0 + 2);
      s0 = fma(fv, x01.x, s0); s1 = fma(fv, x01.y, s1);
      s2 = fma(fv, x23.x, s2); s3 = fma(fv, x23.y, s3);
      rs += fv;
    }
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64);
      s2 += __shfl_down(s2, off, 64); s3 += __shfl_down(s3, off, 64);
      rs += __shfl_down(rs, off, 64);
    }
    if (lane == 0) {
      double* g = G + row * P + c0;
      g[0] = s0; g[1] = s1; g[2] = s2; g[3] = s3;
      if (c0 == c_lo) r[row] = rs;
    }
  }
}

// t[i] = sum_j V[i][j] Z[i][j]: a wave per row
__global__ __launch_bounds__(256) void k_lml_grad_rowdot(const double* __restrict__ V, const double* __restrict__ Z, long ld, int n,
                                                         double* __restrict__ t) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const double* v = V + row * ld;
  const double* z = Z + row * ld;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s = fma(v[j], z[j], s);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) t[row] = s;
}

// sum over the workgroup's 256 threads in a fixed order; the result in every thread
__device__ __forceinline__ double block_sum256(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}

// out[0] = 1/2 (sum alpha_i alpha_j K_ij - sum t), out[1 + c] = sum_i xs_ic (xs_ic r_i - G_ic) (workgroup c; r [n_parts][n]:
// the row sums of the F of column c's part), out[P + 1] = 1/2 noise_var tr W, out[P + 2] = sum alpha (workgroup P)
__global__ __launch_bounds__(256) void k_lml_grad_finish(const double* __restrict__ Xp, int P, int n, const PartDev* __restrict__ parts,
                                                         const double* __restrict__ r,
                                                         const double* __restrict__ G, const double* __restrict__ part,
                                                         long tiles, const double* __restrict__ alpha,
                                                         const double* __restrict__ t, double noise_var,
                                                         double* __restrict__ out) {
  __shared__ double s[256];
  const int tid = threadIdx.x, c = blockIdx.x;
  if (c < P) {
    int h = 0;
    while (c >= parts[h].poff + parts[h].kc) ++h;         // (the parts tile [0, P) in order)
    const double* rh = r + (long)h * n;
    double v = 0.0;
    for (long i = tid; i < n; i += 256) {
      const double x = Xp[i * P + c];
      v += x * (x * rh[i] - G[i * P + c]);
    }
    v = block_sum256(v, s);
    if (tid == 0) out[1 + c] = v;
    return;
  }
  double wk = 0.0, tr = 0.0, sa = 0.0, ak = 0.0;
  for (long q = tid; q < tiles; q += 256) { wk += part[2 * q]; tr += part[2 * q + 1]; }
  for (long i = tid; i < n; i += 256) { sa += alpha[i]; ak += t[i]; }
  wk = block_sum256(wk, s);
  tr = block_sum256(tr, s);
  sa = block_sum256(sa, s);
  ak = block_sum256(ak, s);
  if (tid == 0) { out[0] = 0.5 * (wk - ak); out[P + 1] = 0.5 * noise_var * tr; out[P + 2] = sa; }
}

// which fit this is, for the message of a rejected call (nullptr: a single SE / Matern kernel, nu <= 2.5)
const char* unsupported_kernel(const KernDev& kd) {
  switch (kd.kind) {
    case DFH_KERNEL_ADDITIVE: return "an ADDITIVE kernel";
    case DFH_KERNEL_PRODUCT: return "a PRODUCT kernel";
    case DFH_KERNEL_POLY: return "a POLY kernel";
    case DFH_KERNEL_EXPDECAY: return "an EXPDECAY kernel";
    case DFH_KERNEL_ESP: return "an ESP kernel";
    case DFH_KERNEL_HAMMING: return "a HAMMING kernel";
    default: break;
  }
  if (kd.kind != DFH_KERNEL_SE && kd.kind != DFH_KERNEL_MATERN) return "a kernel of unknown kind";
  if (kd.multi || kd.n_parts != 1) return "a kernel of several parts";
  if (kd.kind == DFH_KERNEL_MATERN && kd.parts[0].p > 2) return "a MATERN kernel with nu above 2.5";
  return nullptr;
}

// the same for dfh_gp_lml_grad_groups: nullptr for an ADDITIVE / PRODUCT kernel of plain SE / Matern parts (nu <= 2.5) as well
const char* unsupported_groups(const KernDev& kd) {
  if (kd.kind != DFH_KERNEL_ADDITIVE && kd.kind != DFH_KERNEL_PRODUCT) return unsupported_kernel(kd);
  if (kd.esp) return "an ESP kernel";
  if (kd.nested) return "a nested factor (an additive or product factor inside a PRODUCT kernel, group_factor)";
  for (const PartDev& pd : kd.parts) {
    if (pd.kind == DFH_KERNEL_POLY) return "a POLY part";
    if (pd.kind == DFH_KERNEL_EXPDECAY) return "an EXPDECAY part";
    if (pd.kind == DFH_KERNEL_HAMMING) return "a HAMMING part";
    if (pd.kind != DFH_KERNEL_SE && pd.kind != DFH_KERNEL_MATERN) return "a part of unknown kind";
    if (pd.kind == DFH_KERNEL_MATERN && pd.p > 2) return "a MATERN part with nu above 2.5";
  }
  return nullptr;
}

// what both entry points reject, under the caller's name
int reject_fit(const dfh_gp* gp, const char* fn) {
  if (gp->gram) {
    dfh_set_error("%s: a Gram-mode fit (dfh_gp_fit_gram) keeps no kernel to differentiate", fn);
    return DFH_ERR_BAD_ARG;
  }
  if (gp->psd_flags) {
    dfh_set_error("%s: a %s fit factors a projection, not K + noise I of the kernel", fn,
                  (gp->psd_flags & DFH_FIT_PROJECT_FIRST) ? "project_first" : "try_before_project");
    return DFH_ERR_BAD_ARG;
  }
  return DFH_OK;
}

// Z = L^-T from the factor, then t[i] = sum_j (K L^-T)_ij Z_ij (sum t = tr(A^-1 K)), then A^-1 = Z Z^T (tiles on and below
// the diagonal) into B, which held K L^-T until then.  Z and B are n x ldw.
int inverse_from_factor(dfh_gp* gp, double* Z, double* B, int64_t ldw, double* t) {
  dfh_ctx* ctx = gp->ctx;
  const int64_t n = gp->n, NB = CHOL_NB;
  DFH_HIP(hipMemsetAsync(Z, 0, (size_t)n * ldw * 8, ctx->stream));
  DFH_TRY(add_diag(ctx, Z, n, ldw, 1.0));
  // row r of L^-T is zero before column r: the rows of block b are a solve with the trailing factor L[b.., b..] alone
  const double* diag = gp->inv + gp->nblk * NB * NB;
  for (int64_t b = 0; b < gp->nblk; ++b) {
    const int64_t r0 = b * NB, w = std::min(NB, n - r0);
    DFH_TRY(trsm_rows(ctx, gp->L + r0 * (n + 1), n - r0, n, gp->inv + b * NB * NB, Z + r0 * (ldw + 1), w, ldw,
                      gp->refine.data() + b, diag + b * NB * NB));
  }
  DFH_TRY(kernmat_gram(ctx, gp->kd, 0, gp->kd.n_parts, true, KmPts{gp->Xp, gp->Np, n}, 0.0, B, ldw));
  DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, B, n, ldw, gp->refine.data()));
  hipLaunchKernelGGL(k_lml_grad_rowdot, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, B, Z, (long)ldw, (int)n, t);
  DFH_LAUNCH_CHECK();
  return gemm_f64(ctx, GEMM_LOWER, n, n, n, 1.0, Z, ldw, Z, ldw, 0.0, nullptr, 0, B, ldw);
}

// The gradient by packed column: host[0] log scale, host[1 + q] log bandwidth of packed column q (padding columns: 0),
// host[P + 1] log noise_var, host[P + 2] the constant mean.  A single kernel takes k_lml_grad_F, once; a kernel of
// several parts k_lml_grad_F_parts, once per part into the same F.
int lml_grad_packed(dfh_gp* gp, std::vector<double>* host) {
  dfh_ctx* ctx = gp->ctx;
  const KernDev& kd = gp->kd;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  const int P = kd.P, n_parts = kd.n_parts;
  DFH_ARG(n < (1LL << 30) && (P % 4) == 0 && n_parts >= 1 && kd.parts[0].poff == 0);
  for (int h = 0; h < n_parts; ++h)     // the parts tile [0, P) in order, each a multiple of 4 wide
    DFH_ARG(kd.parts[h].kc % 4 == 0 && kd.parts[h].poff + kd.parts[h].kc == (h + 1 < n_parts ? kd.parts[h + 1].poff : P));
  const int64_t ldw = (n + 7) / 8 * 8;
  const int64_t tiles_1d = (n + GT - 1) / GT, tiles = tiles_1d * (tiles_1d + 1) / 2;
  DFH_ARG(tiles < (1LL << 31));
  double *Z = nullptr, *Ainv = nullptr, *vec = nullptr, *part = nullptr, *out = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * ldw * 8, (void**)&Z));
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)n * ldw * 8, (void**)&Ainv));
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)n * (P + n_parts + 1) * 8, (void**)&vec));
  DFH_TRY(scratch_get(ctx, SCR_RED2, (size_t)tiles * 16, (void**)&part));
  DFH_TRY(scratch_get(ctx, SCR_OUT, (size_t)(P + 3) * 8, (void**)&out));
  double* r = vec; double* G = vec + n * n_parts; double* trow = G + n * P;      // r [n_parts][n], G [n][P], trow [n]
  {
    SectionTimer t(ctx, DFH_T_TRSM);
    DFH_TRY(inverse_from_factor(gp, Z, Ainv, ldw, trow));
  }
  double* F = Z;                                         // (Z is dead once the product has read it)
  {
    SectionTimer t(ctx, DFH_T_KERNMAT);
    GradArgs a;
    a.ec = kExpConsts;
    a.Xp = gp->Xp; a.Np = gp->Np; a.alpha = gp->alpha;
    a.Ainv = Ainv; a.lda = ldw; a.F = F; a.ldf = ldw;
    a.parts = kd.d_parts; a.n = (int)n; a.P = P;
    a.n_parts = n_parts; a.product = kd.product ? 1 : 0; a.outer = kd.outer_scale; a.group = 0;
    // (nb + na) - 2 acc carries the rounding of a P-term dot product and of the two norms: (P + 2) ulps of na + nb
    a.zero_tol = (double)(P + 2) * 0x1p-52;
    a.part = part;
    for (int g = 0; g < n_parts; ++g) {
      const PartDev& pd = kd.parts[g];
      a.group = g;
      if (kd.multi) hipLaunchKernelGGL(k_lml_grad_F_parts, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL(k_lml_grad_F, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, a);
      DFH_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_lml_grad_FX, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, F, (long)ldw, gp->Xp, P, pd.poff,
                         pd.poff + pd.kc, (int)n, r + (int64_t)g * n, G);
      DFH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_lml_grad_finish, dim3((unsigned)(P + 1)), dim3(256), 0, ctx->stream, gp->Xp, P, (int)n, kd.d_parts, r, G,
                       part, (long)tiles, gp->alpha, trow, gp->noise_var, out);
    DFH_LAUNCH_CHECK();
  }
  host->resize((size_t)P + 3);
  DFH_TRY(from_device(ctx, host->data(), out, host->size() * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

}  // namespace

extern "C" int dfh_gp_lml_grad(dfh_gp* gp, double* grad_out, double* lml_out) {
  DFH_ARG(gp && grad_out);
  DFH_TRY(reject_fit(gp, "dfh_gp_lml_grad"));
  const KernDev& kd = gp->kd;
  if (const char* what = unsupported_kernel(kd)) {
    dfh_set_error("dfh_gp_lml_grad: %s is not supported (a single SE or MATERN kernel with nu 0.5, 1.5 or 2.5 is)", what);
    return DFH_ERR_BAD_ARG;
  }
  std::vector<double> host;
  DFH_TRY(lml_grad_packed(gp, &host));
  const int64_t d = gp->d;
  const int P = kd.P;
  grad_out[0] = host[0];
  for (int64_t c = 0; c < d; ++c) grad_out[1 + c] = 0.0;
  for (int q = 0; q < P; ++q)
    if (kd.cols[q] >= 0) grad_out[1 + kd.cols[q]] = host[1 + q];
  grad_out[d + 1] = host[P + 1];
  grad_out[d + 2] = host[P + 2];
  if (lml_out) *lml_out = gp->lml;
  return DFH_OK;
}

extern "C" int dfh_gp_lml_grad_groups(dfh_gp* gp, double* grad_out, int64_t len, double* lml_out) {
  DFH_ARG(gp && grad_out);
  DFH_TRY(reject_fit(gp, "dfh_gp_lml_grad_groups"));
  const KernDev& kd = gp->kd;
  if (const char* what = unsupported_groups(kd)) {
    dfh_set_error("dfh_gp_lml_grad_groups: %s is not supported (a single SE or MATERN kernel, or an ADDITIVE / PRODUCT kernel "
                  "of plain SE / MATERN parts, nu 0.5, 1.5 or 2.5, is)", what);
    return DFH_ERR_BAD_ARG;
  }
  // the packed columns that are not padding, in order: the parts' columns as sub_bw / group_dims list them (a single
  // kernel: its columns)
  const int P = kd.P;
  int64_t Q = 0;
  for (int q = 0; q < P; ++q) Q += kd.cols[q] >= 0;
  if (len != Q + 3) {
    dfh_set_error("dfh_gp_lml_grad_groups: len is %lld, this kernel's gradient has %lld bandwidths + 3 = %lld entries",
                  (long long)len, (long long)Q, (long long)(Q + 3));
    return DFH_ERR_BAD_ARG;
  }
  std::vector<double> host;
  DFH_TRY(lml_grad_packed(gp, &host));
  grad_out[0] = host[0];
  int64_t at = 1;
  for (int q = 0; q < P; ++q)
    if (kd.cols[q] >= 0) grad_out[at++] = host[1 + q];
  grad_out[Q + 1] = host[P + 1];
  grad_out[Q + 2] = host[P + 2];
  if (lml_out) *lml_out = gp->lml;
  return DFH_OK;
}
