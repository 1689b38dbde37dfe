// The arg-max reductions of the acquisitions: kernels over argmax.h, the running winner, host calls with the launch geometry.
#include "gp.h"
#include "argmax.h"
#include <algorithm>

namespace {

// Stage 1 of a long vector: one partial winner per workgroup, indices offset by idx_base
__global__ void k_argmax_stage1(const double* __restrict__ v, long m, long idx_base, double* __restrict__ pv,
                                long* __restrict__ pi) {
  const long lo = (long)blockIdx.x * blockDim.x;
  double bv; long bi;
  argmax_scan(v, lo, m, (long)gridDim.x * blockDim.x, idx_base + lo, bv, bi);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// Stage 2: the best of the partial winners (their own indices; an empty partial has ARGMAX_NONE)
__global__ void k_argmax_stage2(const double* pv, const long* pi, int nparts, double* out_v, long* out_i) {
  double bv = -INFINITY; long bi = ARGMAX_NONE;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    if (pi[i] != ARGMAX_NONE && (bi == ARGMAX_NONE || argmax_better(pv[i], pi[i], bv, bi))) { bv = pv[i]; bi = pi[i]; }
  }
  block_argmax(bv, bi);
  if (threadIdx.x == 0) { out_v[0] = bv; out_i[0] = bi; }
}

// One workgroup per span of v, indices local: segment [off[g], off[g+1]), or without `off` the first m of row g of v [rows x ld]
__global__ void k_argmax_spans(const double* __restrict__ v, const long* __restrict__ off, long ld, long m,
                               double* __restrict__ out_v, long* __restrict__ out_i) {
  const long lo = off ? off[blockIdx.x] : (long)blockIdx.x * ld, hi = off ? off[blockIdx.x + 1] : lo + m;
  double bv; long bi;
  argmax_scan(v, lo, hi, blockDim.x, 0, bv, bi);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) { out_v[blockIdx.x] = bv; out_i[blockIdx.x] = bi; }
}

}  // namespace

int argmax_parts(dfh_ctx* ctx, int cap, ArgmaxParts* p) {
  char* buf = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)(cap + 1) * 16 + 64, (void**)&buf));
  p->cap = cap;
  p->pv = reinterpret_cast<double*>(buf);
  p->pi = reinterpret_cast<long*>(buf + (size_t)(cap + 1) * 8);
  p->flag = reinterpret_cast<int*>(buf + (size_t)(cap + 1) * 16);
  return DFH_OK;
}

int argmax_finish(dfh_ctx* ctx, const ArgmaxParts& p, int nparts, double* best_val, int64_t* best_idx, int* flag) {
  hipLaunchKernelGGL(k_argmax_stage2, dim3(1), dim3(256), 0, ctx->stream, (const double*)p.pv, (const long*)p.pi, nparts,
                     p.pv + p.cap, p.pi + p.cap);
  DFH_LAUNCH_CHECK();
  DFH_HIP(hipMemcpyAsync(best_val, p.pv + p.cap, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipMemcpyAsync(best_idx, p.pi + p.cap, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (flag) DFH_HIP(hipMemcpyAsync(flag, p.flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

int argmax_rows(dfh_ctx* ctx, hipStream_t stream, const double* v, int64_t rows, int64_t ld, int64_t m, double* out_v,
                long* out_i) {
  hipLaunchKernelGGL(k_argmax_spans, dim3((unsigned)rows), dim3(256), 0, stream, v, (const long*)nullptr, (long)ld, (long)m,
                     out_v, out_i);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

int argmax_segments(dfh_ctx* ctx, const double* v, const long* off, int G, double* out_v, long* out_i) {
  hipLaunchKernelGGL(k_argmax_spans, dim3((unsigned)G), dim3(256), 0, ctx->stream, v, off, 0L, 0L, out_v, out_i);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

void Winner::merge(double ov, int64_t oi) {
  if (!have || argmax_better(ov, oi, v, i)) { v = ov; i = oi; have = true; }
}

int Winner::update(dfh_ctx* ctx, const double* vals, int64_t m, int64_t idx_base) {
  if (m <= 0) return DFH_OK;
  ArgmaxParts p;
  DFH_TRY(argmax_parts(ctx, (int)std::min<int64_t>(1024, (m + 255) / 256), &p));
  hipLaunchKernelGGL(k_argmax_stage1, dim3(p.cap), dim3(256), 0, ctx->stream, vals, (long)m, (long)idx_base, p.pv, p.pi);
  DFH_LAUNCH_CHECK();
  double hv; int64_t hi;
  DFH_TRY(argmax_finish(ctx, p, p.cap, &hv, &hi));
  merge(hv, hi);
  return DFH_OK;
}
