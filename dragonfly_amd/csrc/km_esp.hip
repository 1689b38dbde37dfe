// Kernel matrices of the ESP kernel: one VALU kernel, five register buckets by order.
#include "kernmat.h"

namespace {

// ---------------------------------------------------------------------------------------
// ESP kernel matrix (DFH_KERNEL_ESP; ESPKernel._child_evaluate, dragonfly/gp/kernel.py:693-726):
//   k_c      = the 1-D SE / Matern kernel of column c on X1[:, c], X2[:, c]   (kern_eval, dist_squared's expansion)
//   p_i      = ((0 + k_0**i) + k_1**i) + ...                                    i = 1..order
//   e_m      = (sum_{i=1..m} (-1)**(i-1) e_{m-i} p_i) / m                       e_0 = 1
//   K[i][j]  = scale * e_order
// No MFMA: every dot product is 1-D, the element is ~d (exp + order) + order^2 fp64 VALU operations with
// nothing to share, so this is a VALU kernel.  A 32 x 32 tile: both operands' scaled columns in LDS
// (x * x is recomputed -- it is the one product the reference's row norm of a single column is), each
// thread 4 elements of one output column; the power sums p_1..p_KB (KB >= order, a register bucket) and,
// in the epilogue, e_0..e_KB live in registers.  k_c**i is a running product (NumPy: pow for i >= 3, so
// ~1 ulp per term apart); the recursion is separate multiply / add / true division, rounding where NumPy
// rounds (the library builds with -ffp-contract=off).
// ---------------------------------------------------------------------------------------
constexpr int ESP_TILE = 32;

struct EspArgs {
  ExpConsts ec;
  const double* Xp1; const double* Xp2;    // packed scaled inputs: one part per column, column c at c * 4
  int n1, n2, P, dim, order;
  const PartDev* parts;                    // [dim] the columns' 1-D kernels
  double scale, diag_add;
  int symmetric, lower_only;
  double* K; long ldk;
};

template <int KB, bool ALL_SE>
__global__ __launch_bounds__(256) void kernmat_esp_kernel(EspArgs p) {
  constexpr int U = KB <= 4 ? 4 : (KB <= 8 ? 2 : 1);   // elements in flight per thread (registers: ~2 KB doubles each)
  extern __shared__ __attribute__((aligned(16))) double esm[];
  double* xa = esm;                                      // [dim][32] the tile's rows of X1
  double* xb = esm + (size_t)p.dim * ESP_TILE;           // [dim][32] the tile's rows of X2
  unsigned ti, tj;
  if (p.symmetric) {                                     // lower-triangular tile enumeration
    const unsigned lin = blockIdx.x;
    ti = (unsigned)((sqrt(8.0 * (double)lin + 1.0) - 1.0) * 0.5);
    while ((unsigned long long)ti * (ti + 1) / 2 > lin) --ti;
    while ((unsigned long long)(ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    tj = lin - (unsigned)((unsigned long long)ti * (ti + 1) / 2);
  } else {
    ti = blockIdx.y; tj = blockIdx.x;
  }
  const long r0 = (long)ti * ESP_TILE, c0 = (long)tj * ESP_TILE;
  for (int idx = threadIdx.x; idx < p.dim * ESP_TILE; idx += 256) {
    const int c = idx >> 5, r = idx & (ESP_TILE - 1);
    const long ra = r0 + r, rb = c0 + r;
    xa[idx] = ra < p.n1 ? p.Xp1[ra * p.P + 4 * c] : 0.0;
    xb[idx] = rb < p.n2 ? p.Xp2[rb * p.P + 4 * c] : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x & (ESP_TILE - 1), ty = threadIdx.x >> 5;    // output column; rows ty + 8 a
  const long col = c0 + tx;
  const int order = p.order;
  for (int a0 = 0; a0 < 4; a0 += U) {
    double ps[U][KB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < KB; ++i) ps[u][i] = 0.0;
    for (int c = 0; c < p.dim; ++c) {
      const double y = xb[c * ESP_TILE + tx];
      const double ny = y * y;
      const PartDev& pd = p.parts[c];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double x = xa[c * ESP_TILE + ty + 8 * (a0 + u)];
        double dsq = (ny + x * x) - 2.0 * (x * y);                          // general_utils.py:66-68
        dsq = dsq < 0.0 ? 0.0 : dsq;
        const double kv = ALL_SE ? pd.scale_c * exp_fast(-dsq / 2, p.ec) : kern_eval(pd, dsq, p.ec);
        double kp = kv;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          if (i < order) {                                                   // power_sum[i + 1] += k_c ** (i + 1)
            ps[u][i] = ps[u][i] + kp;
            kp = kp * kv;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double e[KB + 1];
      e[0] = 1.0;
      double last = 1.0;
#pragma unroll
      for (int m = 1; m <= KB; ++m) {
        if (m <= order) {                                                    // kernel.py:718-722
          double acc = 0.0;
#pragma unroll
          for (int i = 1; i <= m; ++i) {
            const double t = e[m - i] * ps[u][i - 1];
            acc = (i & 1) ? acc + t : acc - t;
          }
          e[m] = acc / (double)m;
          last = e[m];
        }
      }
      const long row = r0 + ty + 8 * (a0 + u);
      if (row >= p.n1 || col >= p.n2) continue;
      double res = p.scale * last;                                           // kernel.py:726
      if (p.symmetric) {
        if (row < col) continue;                                             // (diagonal tile: its lower half)
        if (row == col) res = res + p.diag_add;
        p.K[row * p.ldk + col] = res;
        if (!p.lower_only && row != col) p.K[col * p.ldk + row] = res;
      } else {
        p.K[row * p.ldk + col] = res;
      }
    }
  }
}

template <int KB>
int launch_esp(dfh_ctx* ctx, const EspArgs& a, bool all_se, dim3 grid, size_t smem) {
  auto fn = all_se ? reinterpret_cast<const void*>(kernmat_esp_kernel<KB, true>)
                   : reinterpret_cast<const void*>(kernmat_esp_kernel<KB, false>);
  static bool attr_set[DFH_MAX_DEVICES][2] = {};
  if (smem > 64 * 1024 && !attr_set[ctx->device][all_se]) {
    DFH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(2 * sizeof(double) * ESP_MAX_DIM * ESP_TILE)));
    attr_set[ctx->device][all_se] = true;
  }
  if (all_se) hipLaunchKernelGGL((kernmat_esp_kernel<KB, true>), grid, dim3(256), smem, ctx->stream, a);
  else hipLaunchKernelGGL((kernmat_esp_kernel<KB, false>), grid, dim3(256), smem, ctx->stream, a);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

}  // namespace

// K (ldk) = the ESP kernel between two packed inputs; symmetric: Xp1 == Xp2, n1 == n2, diag_add on the
// diagonal, and lower-triangle tiles only (mirrored unless the call wants the lower triangle only).
int km_launch_esp(dfh_ctx* ctx, const KmCall& c) {
  const KernDev& kd = *c.kd;
  const double *Xp1 = c.a.Xp, *Xp2 = c.b.Xp;
  const int64_t n1 = c.a.n, n2 = c.b.n, ldk = c.ldk;
  const bool symmetric = c.symmetric;
  double* K = c.K;
  DFH_ARG(kd.esp && kd.n_parts == kd.dim && kd.dim <= ESP_MAX_DIM && kd.P == 4 * kd.dim);
  DFH_ARG(kd.esp_order >= 1 && kd.esp_order <= ESP_MAX_ORDER && kd.esp_order <= kd.dim);
  DFH_ARG(!symmetric || n1 == n2);
  bool all_se = true;
  for (int g = 0; g < kd.n_parts; ++g) all_se = all_se && kd.parts[g].kind == DFH_KERNEL_SE;
  EspArgs a;
  a.ec = kExpConsts;
  a.Xp1 = Xp1; a.Xp2 = Xp2; a.n2 = (int)n2; a.P = kd.P; a.dim = kd.dim; a.order = kd.esp_order;
  a.parts = kd.d_parts; a.scale = kd.outer_scale; a.diag_add = c.diag_add;
  a.symmetric = symmetric ? 1 : 0;
  a.lower_only = (symmetric && c.lower_only) ? 1 : 0;
  a.ldk = ldk;
  const size_t smem = 2 * sizeof(double) * (size_t)kd.dim * ESP_TILE;
  const int ord = kd.esp_order;
  auto launch = [&](const EspArgs& b, dim3 grid) -> int {
    if (ord <= 2) return launch_esp<2>(ctx, b, all_se, grid, smem);
    if (ord <= 4) return launch_esp<4>(ctx, b, all_se, grid, smem);
    if (ord <= 8) return launch_esp<8>(ctx, b, all_se, grid, smem);
    if (ord <= 16) return launch_esp<16>(ctx, b, all_se, grid, smem);
    return launch_esp<32>(ctx, b, all_se, grid, smem);
  };
  if (symmetric) {
    const int64_t T = (n1 + ESP_TILE - 1) / ESP_TILE;
    DFH_ARG(T * (T + 1) / 2 < (1LL << 31));
    a.n1 = (int)n1; a.K = K;
    return launch(a, dim3((unsigned)(T * (T + 1) / 2)));
  }
  const int64_t rows_per_launch = 65535LL * ESP_TILE;
  for (int64_t r0 = 0; r0 < n1; r0 += rows_per_launch) {
    const int64_t rr = n1 - r0 < rows_per_launch ? n1 - r0 : rows_per_launch;
    EspArgs b = a;
    b.Xp1 = Xp1 + r0 * kd.P; b.n1 = (int)rr; b.K = K + r0 * ldk;
    DFH_TRY(launch(b, dim3((unsigned)((n2 + ESP_TILE - 1) / ESP_TILE), (unsigned)((rr + ESP_TILE - 1) / ESP_TILE))));
  }
  return DFH_OK;
}
