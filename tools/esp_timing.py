"""Times the ESP kernel (DFH_KERNEL_ESP, csrc/km_esp.hip kernmat_esp_kernel) on the device and prints one JSON object:
the symmetric Gram matrix at three (n, d, order) against the fp64 VALU roofline, a cross matrix, a fit plus an EI
arg-max over 65536 candidates, and a 64-candidate tuning batch.

    python tools/esp_timing.py [--reps R]

Roofline: an element costs ~ d (22 SE) + 2 d order + order^2 + 10 order fp64 VALU operations;
FP64_VALU_PEAK_TOPS is bench.py's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_VALU_PEAK_TOPS = 39.3


def _spec(dim, order, rs, kind='se'):
  from dragonfly_amd.engine import KernelSpec
  return KernelSpec('esp', dim, 1.0, nu=order, sub_kinds=[kind] * dim, sub_scales=[1.0] * dim,
                    sub_nus=[2.5 if kind == 'matern' else 0.0] * dim,
                    sub_bandwidths=[[b] for b in rs.uniform(0.3, 1.5, dim)])


def _ops(dim, order):
  return dim * 22 + 2 * dim * order + order * order + 10 * order


def _time(eng, fn, reps):
  fn()
  eng.sync()
  best = float('inf')
  for _ in range(reps):
    eng.timer_begin()
    fn()
    best = min(best, eng.timer_end())
  return best


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  args = ap.parse_args()
  from dragonfly_amd.engine import get_engine
  eng = get_engine()
  rs = np.random.RandomState(0)
  out = {'gram': []}
  for n, d, order in ((4096, 10, 3), (16384, 32, 4), (4096, 20, 10)):
    X = eng.to_device(rs.rand(n, d))
    K = eng.empty((n, n))
    spec = _spec(d, order, rs)
    ms = _time(eng, lambda: eng.kernel_matrix(spec, X, None, out=K), args.reps)
    elems = n * n               # the full symmetric build: lower tiles computed once, mirrored
    tops = elems / 2.0 * _ops(d, order) / (ms * 1e-3) / 1e12
    out['gram'].append(dict(n=n, d=d, order=order, ms=ms, est_ops_per_elem=_ops(d, order),
                            frac_fp64_valu_peak=tops / FP64_VALU_PEAK_TOPS))
    del K
  n, m, d, order = 4096, 65536, 10, 3
  spec = _spec(d, order, rs)
  X, Xs = eng.to_device(rs.rand(n, d)), eng.to_device(rs.rand(m, d))
  Kc = eng.empty((m, n))
  out['cross'] = dict(m=m, n=n, d=d, order=order, ms=_time(eng, lambda: eng.kernel_matrix(spec, Xs, X, out=Kc), args.reps))
  del Kc
  Xh = rs.rand(n, d)
  Y = np.sin(3 * Xh.sum(axis=1))
  Xc = rs.rand(m, d)
  t0 = time.perf_counter()
  gp = eng.gp_fit(spec, Xh, Y - Y.mean(), 0.01)
  gp.acq_argmax('ei', Xc, params=(float(Y.max()), 0.0), mean_const=float(Y.mean()))
  out['fit_plus_ei_argmax'] = dict(n=n, m=m, wall_ms=(time.perf_counter() - t0) * 1e3)
  n = 1000
  Xh = rs.rand(n, 6)
  Y = np.sin(3 * Xh.sum(axis=1))
  specs = [_spec(6, 1 + c % 6, rs, 'se' if c % 2 else 'matern') for c in range(64)]
  eng.gp_lml_batch(specs, Xh, Y, [0.0] * 64, [0.01] * 64)
  t0 = time.perf_counter()
  eng.gp_lml_batch(specs, Xh, Y, [0.0] * 64, [0.01] * 64)
  out['lml_batch_64'] = dict(n=n, wall_ms=(time.perf_counter() - t0) * 1e3)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
