"""Times dfh_gp_lml_grad next to dfh_gp_fit of the same GP (SE, d = 8) and writes profiles/lml_grad_timing.json:
device-event times, 3 warm-ups then the median of 10, the ratio to the fit, and the share of the gradient spent in its
'trsm' section -- L^-T by trsm_rows on n identity rows, K and K L^-T (a second trsm_rows on n rows) for tr(A^-1 K), and the
n^3 product A^-1 = Z Z^T -- against the tile pass and the small kernels after it.
  python tools/time_lml_grad.py [out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dragonfly_amd.engine import get_engine, KernelSpec

WARMUP, REPS = 3, 10


def median_ms(eng, fn):
  for _ in range(WARMUP):
    fn()
  ts = []
  for _ in range(REPS):
    eng.sync()
    eng.timer_begin()
    fn()
    ts.append(eng.timer_end())
  return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'lml_grad_timing.json')
  eng = get_engine()
  d = 8
  rows = []
  for n in (1000, 4096):
    rs = np.random.RandomState(n)
    X = rs.random_sample((n, d))
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + 0.05 * rs.standard_normal(n)
    spec = KernelSpec('se', d, 1.3, 0.35 + 0.4 * rs.random_sample(d))
    Xd = eng.to_device(X)
    fit_ms = median_ms(eng, lambda: eng.gp_fit(spec, Xd, y - y.mean(), 1e-2))
    fit = eng.gp_fit(spec, Xd, y - y.mean(), 1e-2)
    grad_ms = median_ms(eng, fit.lml_grad)
    eng.timings(True)
    for _ in range(REPS):
      fit.lml_grad()
    sec = eng.timings(False)
    total = sum(sec.values())
    rows.append({'n': n, 'd': d, 'kernel': 'se',
                 'fit_ms': {'median': fit_ms[0], 'min': fit_ms[1], 'max': fit_ms[2]},
                 'lml_grad_ms': {'median': grad_ms[0], 'min': grad_ms[1], 'max': grad_ms[2]},
                 'lml_grad_over_fit': grad_ms[0] / fit_ms[0],
                 'sections_ms_per_call': {k: v / REPS for k, v in sec.items() if v > 0},
                 'inverse_and_trace_share': sec['trsm'] / total if total > 0 else None})
    print(json.dumps(rows[-1]), flush=True)
    Xd.free()
  record = {'what': 'dfh_gp_lml_grad against dfh_gp_fit of the same GP, device events, %d warm-ups, median of %d' % (WARMUP, REPS),
            'device': 'MI355X (gfx950), one GPU', 'rows': rows}
  with open(out, 'w') as f:
    json.dump(record, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
