// The arg-max rule of the library (np.argmax: the first NaN, else the first maximum) and the workgroup reduction applying it.
// Every arg-max in csrc/ -- gp_argmax.hip's kernels, k_ts_pointwise, Winner::merge, mgpu.hip's reduce across ranks -- uses it.
#pragma once
#include "common.h"
#include <limits.h>

#pragma GCC visibility push(hidden)      // shared by the units, none of it exported

static_assert(sizeof(long) == sizeof(int64_t), "device indices (long) and host indices (int64_t) are one type");

// Does (va, ia) come before (vb, ib)?  A NaN beats everything, the earlier index wins ties.
__host__ __device__ __forceinline__ bool argmax_better(double va, long ia, double vb, long ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return (na && nb) ? ia < ib : na;
  if (va != vb) return va > vb;
  return ia < ib;
}

#define ARGMAX_NONE LONG_MAX             // index of "no element yet": a thread without elements, an empty partial

// One thread's share of a scan: the best of v[lo + t], v[lo + t + step], ... below v[hi], t = threadIdx.x; v[lo + j] has index base + j
__device__ __forceinline__ void argmax_scan(const double* __restrict__ v, long lo, long hi, long step, long base, double& bv, long& bi) {
  bv = -INFINITY; bi = ARGMAX_NONE;
  for (long i = lo + threadIdx.x; i < hi; i += step) {
    const double x = v[i];
    if (bi == ARGMAX_NONE || argmax_better(x, base + (i - lo), bv, bi)) { bv = x; bi = base + (i - lo); }
  }
}

// The best of the 256 threads' pairs (bi == ARGMAX_NONE: the thread has none), by an LDS tree; the workgroup's winner is
// left in thread 0's bv / bi.  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_argmax(double& bv, long& bi) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const int t = threadIdx.x;
  sv[t] = bv; si[t] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const double ov = sv[t + s]; const long oi = si[t + s];
      if (oi != ARGMAX_NONE && (si[t] == ARGMAX_NONE || argmax_better(ov, oi, sv[t], si[t]))) { sv[t] = ov; si[t] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { bv = sv[0]; bi = si[0]; }
}

#pragma GCC visibility pop
