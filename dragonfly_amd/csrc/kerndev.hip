// The flattened kernel description (KernDev, common.h) on the host: one part from its parameters, a descriptor from a
// dfh_kernel_desc, the device image ("blob") of a descriptor -- layout, upload, clone, free.  No kernel in here.
#include "common.h"
#include <cstring>
#include <math.h>
#include <stdlib.h>

namespace {

double factorial_d(int n) {
  double r = 1.0;
  for (int i = 2; i <= n; ++i) r *= (double)i;
  return r;
}

double part_value_at_zero(const PartDev& pd);

int fill_part(PartDev& pd, int kind, double scale, double nu) {
  pd.kind = kind;
  pd.p = 0; pd.s8 = pd.s2 = pd.gfac = 0.0; pd.k0 = 0.0;
  for (int i = 0; i < 8; ++i) pd.coeff[i] = 0.0;
  if (kind == DFH_KERNEL_SE || kind == DFH_KERNEL_DIST) {
    pd.scale_c = scale;
    pd.k0 = part_value_at_zero(pd);
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_POLY) {               // nu carries the order
    if (!(nu >= 0.0 && nu <= 64.0 && nu == floor(nu))) {
      dfh_set_error("polynomial kernel: the order has to be an integer in [0, 64] (got %g)", nu);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = (int)nu; pd.scale_c = scale;
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_EXPDECAY) {           // nu carries the offset; powers are set by the caller
    pd.scale_c = scale; pd.gfac = nu;
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_HAMMING) {            // the weights go to the image's hw section, their sum to k0 (make_part)
    pd.scale_c = 1.0;
    return DFH_OK;
  }
  // Matern: kernel.py:242-253, 259-270
  double frac = fmod(nu, 1.0);
  if (!(frac == 0.5) || nu < 0.5) {
    dfh_set_error("Matern kernel: nu has to be p + 0.5 where p is an integer (got %g)", nu);
    return DFH_ERR_BAD_ARG;
  }
  const int p = (int)nu;
  if (p > 7) {
    dfh_set_error("Matern kernel: nu = %g not supported (p <= 7)", nu);
    return DFH_ERR_BAD_ARG;
  }
  pd.p = p;
  for (int i = 0; i <= p; ++i)
    pd.coeff[i] = factorial_d(p + i) / (factorial_d(i) * factorial_d(p - i));
  pd.s8 = sqrt(8.0 * nu);
  pd.s2 = sqrt(2.0 * nu);
  pd.gfac = tgamma((double)p + 1.0) / tgamma(2.0 * p + 1.0);
  // norm_constant = 1 / _eval_kernel_values_unnormalised(0)   (kernel.py:253)
  double u0 = 0.0;
  const double mult0 = pd.s8 * 0.0;
  for (int i = 0; i <= p; ++i) u0 += pd.coeff[i] * pow(mult0, (double)(p - i));
  u0 *= (pd.gfac * exp(-pd.s2 * 0.0));
  const double norm_constant = 1.0 / u0;
  pd.scale_c = scale * norm_constant;
  pd.k0 = part_value_at_zero(pd);
  return DFH_OK;
}

double part_value_at_zero(const PartDev& pd) {
  // k_part(x, x): distance 0
  if (pd.kind == DFH_KERNEL_SE) return pd.scale_c * exp(-0.0 / 2);
  if (pd.kind == DFH_KERNEL_MATERN) {
    double u = 0.0;
    for (int i = 0; i <= pd.p; ++i) u += pd.coeff[i] * pow(0.0, (double)(pd.p - i));
    u *= (pd.gfac * exp(-pd.s2 * 0.0));
    return pd.scale_c * u;
  }
  return 0.0;
}

// device image of a KernDev: [parts | bw | cols | lcols | hw], each section 16-byte aligned (hw: the weight of
// every packed column of a Hamming part, 0 elsewhere; the kernels find it with blob_hw_offset)
static size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }
static void blob_layout(const KernDev& kd, size_t off[5], size_t* total) {
  const size_t P = kd.P ? kd.P : 1;
  off[0] = 0;
  off[1] = off[0] + pad16(sizeof(PartDev) * kd.parts.size());
  off[2] = off[1] + pad16(sizeof(double) * P);
  off[3] = off[2] + pad16(sizeof(int) * P);
  off[4] = blob_hw_offset((int)kd.parts.size(), kd.P);
  *total = off[4] + pad16(sizeof(double) * P);
}
static void blob_fill(const KernDev& kd, char* host) {
  size_t off[5], total;
  blob_layout(kd, off, &total);
  std::memcpy(host + off[0], kd.parts.data(), sizeof(PartDev) * kd.parts.size());
  std::memcpy(host + off[1], kd.bw.data(), sizeof(double) * kd.P);
  std::memcpy(host + off[2], kd.cols.data(), sizeof(int) * kd.P);
  std::memcpy(host + off[3], kd.lcols.data(), sizeof(int) * kd.P);
  std::memcpy(host + off[4], kd.hw.data(), sizeof(double) * kd.P);
}
static void blob_point(KernDev* kd, char* dev) {
  size_t off[5], total;
  blob_layout(*kd, off, &total);
  kd->d_parts = reinterpret_cast<PartDev*>(dev + off[0]);
  kd->d_bw = reinterpret_cast<double*>(dev + off[1]);
  kd->d_cols = reinterpret_cast<int*>(dev + off[2]);
  kd->d_lcols = reinterpret_cast<int*>(dev + off[3]);
}

int upload(dfh_ctx* ctx, KernDev* kd) {
  size_t off[5], total;
  blob_layout(*kd, off, &total);
  std::vector<char> host(total, 0);
  blob_fill(*kd, host.data());
  DFH_HIP(hipMalloc(&kd->d_blob, total));
  blob_point(kd, static_cast<char*>(kd->d_blob));
  DFH_HIP(hipMemcpyAsync(kd->d_blob, host.data(), total, hipMemcpyHostToDevice, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

void add_part_cols(KernDev* kd, PartDev& pd, const int* cols, const double* bw, int ncols) {
  pd.poff = kd->P;
  pd.kc = (ncols + 3) & ~3;
  for (int c = 0; c < pd.kc; ++c) {
    kd->cols.push_back(c < ncols ? cols[c] : -1);
    kd->lcols.push_back(c < ncols ? c : -1);
    kd->bw.push_back(c < ncols ? bw[c] : 1.0);
    kd->hw.push_back(0.0);
  }
  kd->P += pd.kc;
}

}  // namespace

// (eq * wts).sum(axis=1) of a row whose entries all compare equal: NumPy's pairwise order (hamming_eval on the device)
static double np_sum_host(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// One part from (kind, scale, nu, per-column parameters): SE / Matern bandwidths divide the inputs,
// polynomial scalings multiply them (stored negated, see k_pack_cols), exponential-decay powers go
// into the part and its inputs stay as they are.
static int make_part(KernDev* kd, int kind, double scale, double nu, const int* cols, const double* par, int ncols) {
  PartDev pd;
  DFH_TRY(fill_part(pd, kind, scale, nu));
  pd.fmode = 0; pd.fpad = 0; pd.fscale = 1.0;
  std::vector<double> bw((size_t)ncols);
  if (kind == DFH_KERNEL_POLY) {
    for (int c = 0; c < ncols; ++c) {
      if (!(par[c] > 0.0)) { dfh_set_error("polynomial kernel: dim_scalings must be positive"); return DFH_ERR_BAD_ARG; }
      bw[c] = -par[c];
    }
  } else if (kind == DFH_KERNEL_EXPDECAY) {
    if (ncols > EXPDECAY_MAX_DIM) {
      dfh_set_error("exponential-decay kernel: at most %d dimensions (got %d)", EXPDECAY_MAX_DIM, ncols);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = ncols;
    for (int c = 0; c < ncols; ++c) { pd.coeff[c] = par[c]; bw[c] = 1.0; }
  } else if (kind == DFH_KERNEL_HAMMING) {
    if (ncols > HAMMING_MAX_DIM) {
      dfh_set_error("Hamming kernel: at most %d dimensions (got %d)", HAMMING_MAX_DIM, ncols);
      return DFH_ERR_BAD_ARG;
    }
    if (scale != 1.0 || nu != 0.0) {
      dfh_set_error("Hamming kernel: scale must be 1 and nu 0 (got %g, %g)", scale, nu);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = ncols;
    for (int c = 0; c < ncols; ++c) bw[c] = 1.0;         // the category codes stay as they are (x / 1.0)
    pd.k0 = np_sum_host(par, ncols);                      // k(x, x) = sum_c w_c whatever x
  } else {
    for (int c = 0; c < ncols; ++c) bw[c] = par[c];
  }
  add_part_cols(kd, pd, cols, bw.data(), ncols);
  if (kind == DFH_KERNEL_HAMMING)
    for (int c = 0; c < ncols; ++c) kd->hw[(size_t)pd.poff + c] = par[c];
  kd->parts.push_back(pd);
  return DFH_OK;
}

// what every kerndev_build_host starts from
static void kerndev_reset(const dfh_kernel_desc* k, KernDev* kd) {
  kd->kind = k->kind; kd->dim = k->dim; kd->P = 0;
  kd->parts.clear(); kd->cols.clear(); kd->lcols.clear(); kd->bw.clear(); kd->hw.clear();
  kd->stationary = true; kd->kxx = 0.0;
  kd->esp = false; kd->esp_order = 0; kd->hamming = false;
}

static int make_whole_part(const dfh_kernel_desc* k, KernDev* kd) {      // one part over every column
  DFH_ARG(k->bw != nullptr);
  std::vector<int> ident(k->dim);
  for (int i = 0; i < k->dim; ++i) ident[i] = i;
  return make_part(kd, k->kind, k->scale, k->nu, ident.data(), k->bw, k->dim);
}

// SE / Matern
static int build_single_stationary(const dfh_kernel_desc* k, KernDev* kd) {
  DFH_TRY(make_whole_part(k, kd));
  kd->multi = false; kd->product = false; kd->outer_scale = 1.0; kd->nested = false;
  kd->kxx = kd->parts[0].k0;
  return DFH_OK;
}

// polynomial / exponential-decay / Hamming: a product with one factor and outer scale 1 (1.0 * k is exact): the generic
// multi-part kernel-matrix kernel is the only one that knows these kinds
static int build_single_nonstationary(const dfh_kernel_desc* k, KernDev* kd) {
  kd->hamming = k->kind == DFH_KERNEL_HAMMING;
  DFH_TRY(make_whole_part(k, kd));
  kd->multi = true; kd->product = true; kd->outer_scale = 1.0; kd->nested = false;
  kd->stationary = false;
  return DFH_OK;
}

// additive / product kernels, a product's factors possibly additive or products themselves (nested)
static int build_groups(const dfh_kernel_desc* k, KernDev* kd) {
  DFH_ARG(k->n_groups >= 1 && k->group_off && k->group_dims && k->sub_kind && k->sub_scale && k->sub_bw);
  const bool product = (k->kind == DFH_KERNEL_PRODUCT);
  const bool nested = product && k->group_factor != nullptr;
  if (k->group_factor || k->factor_is_sum || k->factor_scale)
    DFH_ARG(product && k->group_factor && k->factor_is_sum && k->factor_scale);
  double acc = product ? k->scale : 0.0;
  double facc = 0.0;                              // k(x, x) of the additive / product factor under way
  for (int g = 0; g < k->n_groups; ++g) {
    const int lo = k->group_off[g], hi = k->group_off[g + 1];
    DFH_ARG(hi > lo);
    for (int c = lo; c < hi; ++c) DFH_ARG(k->group_dims[c] >= 0 && k->group_dims[c] < k->dim);
    const int sk = k->sub_kind[g];
    // polynomial groups also in an additive kernel (the reference's factory builds them: euclidean_gp.py:870-879)
    DFH_ARG(kind_is_stationary(sk) || sk == DFH_KERNEL_POLY || (product && (sk == DFH_KERNEL_EXPDECAY || sk == DFH_KERNEL_HAMMING)));
    if (sk == DFH_KERNEL_HAMMING) kd->hamming = true;
    DFH_TRY(make_part(kd, sk, k->sub_scale[g], k->sub_nu ? k->sub_nu[g] : 0.0, k->group_dims + lo,
                      k->sub_bw + lo, hi - lo));
    if (!kind_is_stationary(sk)) kd->stationary = false;
    const double k0 = kd->parts.back().k0;
    PartDev& pd = kd->parts.back();
    pd.fmode = 0; pd.fpad = 0; pd.fscale = 1.0;
    if (nested) {
      const int f = k->group_factor[g];
      DFH_ARG(f >= 0 && f <= g && (g == 0 ? f == 0 : (f == k->group_factor[g - 1] || f == k->group_factor[g - 1] + 1)));
      const bool first = g == 0 || k->group_factor[g - 1] != f;
      const bool last = g + 1 == k->n_groups || k->group_factor[g + 1] != f;
      if (k->factor_is_sum[f] == DFH_FACTOR_PRODUCT) {
        // the groups of a Cartesian-product kernel: SE / Matern / exponential decay / Hamming (no polynomial, no factor inside)
        DFH_ARG(kind_is_stationary(sk) || sk == DFH_KERNEL_EXPDECAY || sk == DFH_KERNEL_HAMMING);
        pd.fmode = FM_PROD | (first ? FM_BEGIN : 0) | (last ? FM_END : 0);
        pd.fscale = k->factor_scale[f];
        facc = (first ? pd.fscale * 1.0 : facc) * k0;         // combine_nested's order
        if (last) acc *= facc;
      } else if (k->factor_is_sum[f]) {
        DFH_ARG(sk != DFH_KERNEL_EXPDECAY && sk != DFH_KERNEL_HAMMING);       // an additive kernel's groups: SE / Matern / polynomial
        pd.fmode = FM_IN | (first ? FM_BEGIN : 0) | (last ? FM_END : 0);
        pd.fscale = k->factor_scale[f];
        facc = first ? 0.0 + k0 : facc + k0;
        if (last) acc *= pd.fscale * facc;
      } else {
        DFH_ARG(first && last);                   // a plain factor is one group
        acc *= k0;
      }
    } else if (product) {
      acc *= k0;                                    // K *= kernel(...)        kernel.py:588
    } else {
      acc += k0;                                    // result += kernel(...)   kernel.py:493
    }
  }
  kd->multi = true; kd->product = product; kd->outer_scale = k->scale; kd->nested = nested;
  kd->kxx = !kd->stationary ? 0.0 : (product ? acc : k->scale * acc);        // kernel.py:494
  return DFH_OK;
}

// k(x, x) of an ESP kernel: the device's power sums and Newton-Girard steps on the parts' values at distance 0
// (a Matern part's k0 is norm_constant * unnorm(0), not necessarily exactly 1)
static double esp_kxx(const KernDev& kd, int order, double scale) {
  double ps[ESP_MAX_ORDER] = {0.0};
  for (int g = 0; g < kd.dim; ++g) {
    const double kv = kd.parts[g].k0;
    double kp = kv;
    for (int i = 0; i < order; ++i) { ps[i] = ps[i] + kp; kp = kp * kv; }
  }
  double e[ESP_MAX_ORDER + 1];
  e[0] = 1.0;
  for (int m = 1; m <= order; ++m) {
    double acc = 0.0;
    for (int i = 1; i <= m; ++i) {
      const double t = e[m - i] * ps[i - 1];
      acc = (i & 1) ? acc + t : acc - t;
    }
    e[m] = acc / (double)m;
  }
  return scale * e[order];
}

// kernel.py:671-744: one 1-D SE / Matern kernel per column, kernel_list[i] on column i
static int build_esp(const dfh_kernel_desc* k, KernDev* kd) {
  if (!(k->n_groups == k->dim && k->group_off && k->group_dims && k->sub_kind && k->sub_scale && k->sub_bw)) {
    dfh_set_error("ESP kernel: needs n_groups == dim (%d) with group_off, group_dims, sub_kind, sub_scale, sub_bw",
                  k->dim);
    return DFH_ERR_BAD_ARG;
  }
  if (k->group_factor || k->factor_is_sum || k->factor_scale) {
    dfh_set_error("ESP kernel: group_factor / factor_is_sum / factor_scale must be NULL");
    return DFH_ERR_BAD_ARG;
  }
  if (k->dim > ESP_MAX_DIM) {
    dfh_set_error("ESP kernel: at most %d dimensions on the device (got %d)", ESP_MAX_DIM, k->dim);
    return DFH_ERR_BAD_ARG;
  }
  if (!(k->nu >= 1.0 && k->nu <= (double)k->dim && k->nu == floor(k->nu))) {
    dfh_set_error("ESP kernel: order must be an integer between 1 and dim = %d (got %g)", k->dim, k->nu);
    return DFH_ERR_BAD_ARG;
  }
  const int order = (int)k->nu;
  if (order > ESP_MAX_ORDER) {
    dfh_set_error("ESP kernel: order %d is above the device's %d", order, ESP_MAX_ORDER);
    return DFH_ERR_BAD_ARG;
  }
  if (k->group_off[0] != 0) {
    dfh_set_error("ESP kernel: group_off[0] must be 0");
    return DFH_ERR_BAD_ARG;
  }
  for (int g = 0; g < k->dim; ++g) {
    if (k->group_off[g + 1] != g + 1 || k->group_dims[g] != g) {
      dfh_set_error("ESP kernel: group %d must be column %d alone (group_off = 0..dim, group_dims[g] = g)", g, g);
      return DFH_ERR_BAD_ARG;
    }
    if (!kind_is_stationary(k->sub_kind[g])) {
      dfh_set_error("ESP kernel: the kernel of column %d must be SE or Matern (kind %d)", g, k->sub_kind[g]);
      return DFH_ERR_BAD_ARG;
    }
    DFH_TRY(make_part(kd, k->sub_kind[g], k->sub_scale[g], k->sub_nu ? k->sub_nu[g] : 0.0, &g, k->sub_bw + g, 1));
  }
  kd->multi = true; kd->product = false; kd->outer_scale = k->scale; kd->nested = false;
  kd->esp = true; kd->esp_order = order;
  kd->kxx = esp_kxx(*kd, order, k->scale);
  return DFH_OK;
}

int kerndev_build_host(const dfh_kernel_desc* k, KernDev* kd) {
  DFH_ARG(k != nullptr && kd != nullptr);
  DFH_ARG(k->dim >= 1);
  kerndev_reset(k, kd);
  if (k->kind == DFH_KERNEL_SE || k->kind == DFH_KERNEL_MATERN) {
    DFH_TRY(build_single_stationary(k, kd));
  } else if (k->kind == DFH_KERNEL_POLY || k->kind == DFH_KERNEL_EXPDECAY || k->kind == DFH_KERNEL_HAMMING) {
    DFH_TRY(build_single_nonstationary(k, kd));
  } else if (k->kind == DFH_KERNEL_ADDITIVE || k->kind == DFH_KERNEL_PRODUCT) {
    DFH_TRY(build_groups(k, kd));
  } else if (k->kind == DFH_KERNEL_ESP) {
    DFH_TRY(build_esp(k, kd));
  } else {
    dfh_set_error("unknown kernel kind %d", k->kind);
    return DFH_ERR_BAD_ARG;
  }
  kd->n_parts = (int)kd->parts.size();
  return DFH_OK;
}

int kerndev_build(dfh_ctx* ctx, const dfh_kernel_desc* k, KernDev* kd) {
  DFH_TRY(kerndev_build_host(k, kd));
  return upload(ctx, kd);
}

size_t kerndev_blob_bytes(const KernDev& kd) {
  size_t off[5], total;
  blob_layout(kd, off, &total);
  return total;
}
void kerndev_blob_fill(const KernDev& kd, char* host) { blob_fill(kd, host); }

// The images of kds[0 .. count) laid out in `host` one behind the other, and the descriptors pointed at where they
// WILL be on the device (d_blob, which they do not own); *used = the bytes laid out.
static int stage_images(KernDev* kds, int count, char* host, void* d_blob, size_t blob_bytes, size_t* used) {
  size_t at = 0;
  for (int c = 0; c < count; ++c) {
    const size_t sz = kerndev_blob_bytes(kds[c]);
    DFH_ARG(at + sz <= blob_bytes);
    blob_fill(kds[c], host + at);
    kds[c].d_blob = nullptr;                    // not owned
    blob_point(&kds[c], static_cast<char*>(d_blob) + at);
    at += sz;
  }
  *used = at;
  return DFH_OK;
}

// Without the copy: `host` is the caller's pinned staging memory, copied up by the caller together with whatever else
// the launch needs.
int kerndev_stage_many(KernDev* kds, int count, char* host, void* d_blob, size_t blob_bytes) {
  std::memset(host, 0, blob_bytes);
  size_t used = 0;
  return stage_images(kds, count, host, d_blob, blob_bytes, &used);
}

int kerndev_upload_many(dfh_ctx* ctx, KernDev* kds, int count, void* d_blob, size_t blob_bytes) {
  std::vector<char> host(blob_bytes, 0);
  size_t used = 0;
  DFH_TRY(stage_images(kds, count, host.data(), d_blob, blob_bytes, &used));
  DFH_HIP(hipMemcpyAsync(d_blob, host.data(), used, hipMemcpyHostToDevice, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}


int kerndev_build_dist(dfh_ctx* ctx, int dim, KernDev* kd) {
  DFH_ARG(dim >= 1);
  kd->kind = DFH_KERNEL_DIST; kd->dim = dim; kd->P = 0;
  kd->parts.clear(); kd->cols.clear(); kd->lcols.clear(); kd->bw.clear(); kd->hw.clear();
  PartDev pd;
  DFH_TRY(fill_part(pd, DFH_KERNEL_DIST, 1.0, 0.0));
  std::vector<int> ident(dim);
  std::vector<double> ones(dim, 1.0);
  for (int i = 0; i < dim; ++i) ident[i] = i;
  add_part_cols(kd, pd, ident.data(), ones.data(), dim);
  kd->parts.push_back(pd);
  kd->multi = false; kd->outer_scale = 1.0; kd->kxx = 0.0;
  kd->esp = false; kd->esp_order = 0; kd->hamming = false;
  kd->n_parts = 1;
  return upload(ctx, kd);
}

int kerndev_clone(dfh_ctx* ctx, const KernDev& src, KernDev* out) {
  *out = src;
  out->d_blob = nullptr; out->d_parts = nullptr; out->d_cols = nullptr; out->d_lcols = nullptr; out->d_bw = nullptr;
  return upload(ctx, out);
}

void kerndev_free(KernDev* kd) {
  if (!kd) return;
  if (kd->d_blob) (void)hipFree(kd->d_blob);
  kd->d_blob = nullptr;
  kd->d_parts = nullptr; kd->d_cols = nullptr; kd->d_lcols = nullptr; kd->d_bw = nullptr;
}

double kerndev_part_kxx(const KernDev& kd, int part) { return part_value_at_zero(kd.parts[part]); }
