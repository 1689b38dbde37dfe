"""Times the fused multi-objective calls against the per-objective route on the same library and writes
profiles/moo_timing.json.

    python tools/moo_timing.py [--out profiles/moo_timing.json]

Per size, K = 3 objectives (SE, Matern-2.5, SE with other bandwidths; d = 6): medians of 7 wall-clock samples after 2
warm-up calls, every sample ending with the results on the host (both routes synchronise before they return).
  fused      one Engine.mo_ucb_argmax / mo_thompson call
  per_obj    what the reference's closures cost on this library: K x predict (or K x thompson with
             return_samples=True), the K vectors downloaded and scalarised in NumPy, np.argmax
  download   (Thompson sampling with q = 3 points in progress, m = 4096 only) K x predict_covar with the hallucinated
             points -- the m x m covariance downloaded -- and the draw through the library's stable_cholesky
Sizes: (n, m) = (200, 1000), (4096, 65536), and 32-point tree-search frontiers at n = 4096 (UCB with return_vals).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, K = 6, 3
REPS, WARM = 7, 2


def median_ms(fn):
  for _ in range(WARM):
    fn()
  ts = []
  for _ in range(REPS):
    t0 = time.perf_counter()
    fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fit_objectives(engine, n, rs):
  from dragonfly_amd.engine import KernelSpec
  X = rs.random_sample((n, D))
  specs = [KernelSpec('se', D, 1.0, np.full(D, 0.6)), KernelSpec('matern', D, 1.2, np.full(D, 0.8), nu=2.5),
           KernelSpec('se', D, 0.8, np.linspace(0.4, 0.9, D))]
  gps = []
  for j, spec in enumerate(specs):
    y = np.sin(3 * X[:, j]) - np.sum((X - 0.3 * (j + 1)) ** 2, axis=1) + 0.05 * rs.standard_normal(n)
    gps.append(engine.gp_fit(spec, X, y - np.median(y), 0.01 * float(np.var(y))))
  return gps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moo_timing.json'))
  args = ap.parse_args()
  from dragonfly_amd.engine import get_engine
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  from oracle_engine_moo import scalarise_ts, scalarise_ucb        # the reference's NumPy scalarisations
  engine = get_engine()
  rs = np.random.RandomState(0)
  w, ref, beta, means = [0.5, 0.3, 0.2], [-3.0, -3.0, -3.0], 1.7, [0.0] * K
  rows = []
  for n, m, what in ((200, 1000, 'rand'), (4096, 65536, 'rand'), (4096, 32, 'pdoo frontier')):
    gps = fit_objectives(engine, n, rs)
    Xs = rs.random_sample((m, D))
    U = rs.standard_normal((K, m))
    block = min(m, 4096)
    for scal in ('lin', 'tch'):
      def ucb_fused():
        return engine.mo_ucb_argmax(gps, scal, beta, w, ref, Xs, mean_consts=means, return_vals=(m == 32))
      def ucb_per_obj():
        evals = [gp.predict(Xs) for gp in gps]
        return np.argmax(scalarise_ucb(scal, beta, w, ref, [e[0] for e in evals], [e[1] for e in evals]))
      f, p = median_ms(ucb_fused), median_ms(ucb_per_obj)
      rows.append(dict(acq='ucb', scal=scal, n=n, m=m, what=what, fused_ms=f[0], per_obj_ms=p[0], fused_min_max=f[1:], per_obj_min_max=p[1:],
                       per_obj_over_fused=p[0] / f[0]))
      print(rows[-1], flush=True)
      if m == 32:
        continue
      def ts_fused():
        return engine.mo_thompson(gps, scal, w, ref, Xs, U, block=block, mean_consts=means)
      def ts_per_obj():
        draws = [gp.thompson(Xs, U[i], block=block, return_samples=True)[2] for i, gp in enumerate(gps)]
        return np.argmax(scalarise_ts(scal, w, ref, draws))
      f, p = median_ms(ts_fused), median_ms(ts_per_obj)
      rows.append(dict(acq='ts', scal=scal, n=n, m=m, block=block, what=what, fused_ms=f[0], per_obj_ms=p[0], fused_min_max=f[1:],
                       per_obj_min_max=p[1:], per_obj_over_fused=p[0] / f[0]))
      print(rows[-1], flush=True)
    if n == 4096 and m == 65536:
      # points in progress: the fused hallucinated draw against the m x m download route, one joint block of 4096
      mq = 4096
      Xq, Uq, Xh = Xs[:mq], U[:, :mq].copy(), rs.random_sample((3, D))
      def halluc_fused():
        return engine.mo_thompson(gps, 'lin', w, ref, Xq, Uq, block=mq, X_halluc=Xh, mean_consts=means)
      def halluc_download():
        draws = []
        for i, gp in enumerate(gps):
          mu, cov = gp.predict_covar(Xq, X_halluc=Xh)
          draws.append(mu + engine.stable_cholesky(cov).dot(Uq[i]))
        return np.argmax(scalarise_ts('lin', w, ref, draws))
      f, p = median_ms(halluc_fused), median_ms(halluc_download)
      rows.append(dict(acq='ts', scal='lin', n=n, m=mq, block=mq, q=3, what='points in progress', fused_ms=f[0], download_ms=p[0],
                       fused_min_max=f[1:], download_min_max=p[1:], download_over_fused=p[0] / f[0]))
      print(rows[-1], flush=True)
    for gp in gps:
      gp.free()
  out = dict(device=engine.name(), objectives=K, dim=D, repetitions=REPS, warmup=WARM, statistic='median wall-clock ms per call', rows=rows)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
