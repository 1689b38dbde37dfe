"""Times what the multi-GPU tuning route costs when it buys nothing -- one device -- and writes
profiles/mgpu_tuning_timing.json.

    python tools/mgpu_tuning_timing.py [--out profiles/mgpu_tuning_timing.json] [--parent-json FILE]
    python tools/mgpu_tuning_timing.py --engine-only --root /path/to/parent/checkout --out FILE     # the yardstick

Batches (SE-ARD, d = 5): 10 000 candidates at n = 1000, 64 at n = 1000, 8 at n = 200.  Per batch and route three
rounds, each the median of 7 wall-clock samples after 2 warm-up calls (every call ends with the values on the host);
reported: the median of the round medians and their spread (max - min), the run-to-run figure a difference has to
exceed to mean anything.
  engine     Engine.gp_lml_batch, inputs resident                      (the route of tuning_gpus=None)
  fitter     EuclideanGPFitter.lml_batch of the stand-alone fitter, 8 candidates at n = 200, tuning_gpus=None
  multi1     MultiEngine(1).gp_lml_batch                                -- the fan-out with nobody to fan out to
  multi2     MultiEngine(2, device_ids=[0, 0]).gp_lml_batch(spread=True) -- two contexts and two host threads on ONE
             device (library test switch): overhead and contention, NOT a speed-up; a second device is what it needs
--engine-only times `engine` and `fitter` alone, from the package under --root: run on a checkout of the parent commit
in the same session it is the yardstick (--parent-json merges it and says whether the unchanged routes sit within the
spread).  No speed-up from N > 1 devices can be measured on one device and none is claimed.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 5
REPS, WARM, ROUNDS = 7, 2, 3
BATCHES = ((10000, 1000), (64, 1000), (8, 200))


def median_ms(fn):
  for _ in range(WARM):
    fn()
  ts = []
  for _ in range(REPS):
    t0 = time.perf_counter()
    fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts))


def rounds_ms(fn):
  meds = [median_ms(fn) for _ in range(ROUNDS)]
  return dict(ms=float(np.median(meds)), spread_ms=float(max(meds) - min(meds)), rounds_ms=meds)


def problem(nb, n):
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(nb + n)
  X = rs.random_sample((n, D))
  y = np.sin(3 * X.sum(axis=1)) + 0.1 * rs.standard_normal(n)
  yv = float(y.var())
  specs = [KernelSpec('se', D, yv * (0.5 + rs.random_sample()), 0.3 + 0.6 * rs.random_sample(D)) for _ in range(nb)]
  return X, y, specs, list(0.2 * rs.standard_normal(nb)), list(yv * np.exp(rs.uniform(np.log(0.005), np.log(0.2), nb)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mgpu_tuning_timing.json'))
  ap.add_argument('--root', default=ROOT, help='the checkout whose dragonfly_amd is timed')
  ap.add_argument('--engine-only', action='store_true')
  ap.add_argument('--parent-json', default=None)
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  os.environ['DFH_MGPU_ALLOW_DUPLICATE_DEVICES'] = '1'
  from dragonfly_amd import parallel
  from dragonfly_amd.engine import get_engine
  from dragonfly_amd.euclidean_gp import EuclideanGPFitter
  engine = get_engine()
  multi1 = multi2 = None
  if not args.engine_only:
    multi1, multi2 = parallel.MultiEngine(1), parallel.MultiEngine(2, device_ids=[0, 0])
  rows = []
  for nb, n in BATCHES:
    X, y, specs, means, noises = problem(nb, n)
    Xd = engine.to_device(X)
    row = dict(candidates=nb, n=n, engine=rounds_ms(lambda: engine.gp_lml_batch(specs, Xd, y, means, noises)))
    if (nb, n) == (8, 200):
      fitter = EuclideanGPFitter(list(X), list(y), options=Namespace(kernel_type='se', hp_tune_criterion='ml'))
      lo, hi = fitter.cts_hp_bounds[:, 0], fitter.cts_hp_bounds[:, 1]
      cts = [lo + (hi - lo) * (0.3 + 0.05 * k) for k in range(nb)]
      row['fitter'] = rounds_ms(lambda: fitter.lml_batch(cts, [[]] * nb))
    if not args.engine_only:
      X1, X2 = multi1.to_devices(X), multi2.to_devices(X)
      row['multi1'] = rounds_ms(lambda: multi1.gp_lml_batch(specs, X1, y, means, noises))
      row['multi2_one_device'] = rounds_ms(lambda: multi2.gp_lml_batch(specs, X2, y, means, noises, spread=True))
      row['multi1_overhead_ms'] = row['multi1']['ms'] - row['engine']['ms']
      row['multi2_one_device_over_engine'] = row['multi2_one_device']['ms'] / row['engine']['ms']
      for a in X1 + X2:
        a.free()
    Xd.free()
    rows.append(row)
    print(row, flush=True)
  out = dict(device=engine.name(), dim=D, repetitions=REPS, warmup=WARM, rounds=ROUNDS,
             statistic='median over rounds of the median wall-clock ms per call; spread_ms = max - min of the round medians',
             note='multi2_one_device: two contexts sharing ONE device -- overhead on one device, not a multi-GPU speed-up',
             rows=rows)
  if args.parent_json:
    parent = json.load(open(args.parent_json))
    out['parent_rows'] = parent['rows']
    for row, prow in zip(rows, parent['rows']):
      for key in ('engine', 'fitter'):
        if key in row and key in prow:
          diff = row[key]['ms'] - prow[key]['ms']
          spread = max(row[key]['spread_ms'], prow[key]['spread_ms'])
          row[key + '_vs_parent'] = dict(parent_ms=prow[key]['ms'], diff_ms=diff, spread_ms=spread, within_spread=bool(abs(diff) <= spread))
  if multi1 is not None:
    multi1.close()
    multi2.close()
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
