"""Times dfh_gp_lml_grad_groups on additive kernels of 1, 5 and 20 two-column SE groups and on a two-factor product
(SE x Matern 2.5, four columns each), n = 1000 and 4096, and writes profiles/lml_grad_groups_timing.json.  Beside each:
dfh_gp_fit of the same handle, and dfh_gp_lml_grad on a single SE kernel of the same n and the same packed width P (a
group is padded to a multiple of 4 packed columns, so the single kernel has d = P) -- the function as it was before the
groups.  Device-event times bracketed as tools/time_lml_grad.py brackets them: 3 warm-ups, then the median of 10 with
the smallest and the largest; the grouped and the single gradient are timed alternately, twice, so that a drift of the
machine shows as a spread between the two rounds and not as a difference between the two functions.
  python tools/time_lml_grad_groups.py [out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dragonfly_amd.engine import get_engine, KernelSpec
from time_lml_grad import median_ms, WARMUP, REPS


def stats(t):
  return {'median': t[0], 'min': t[1], 'max': t[2]}


def grouped_spec(family, groups, kinds, rs, d):
  bw = (0.35 + 0.4 * rs.random_sample(d)) * np.sqrt(max(d, 3) / 3.0)
  return KernelSpec(family, d, 1.3, groups=groups, sub_kinds=[k for k, _ in kinds], sub_scales=[1.0] * len(groups),
                    sub_nus=[nu for _, nu in kinds], sub_bandwidths=[bw[g] for g in groups])


def main():
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'lml_grad_groups_timing.json')
  eng = get_engine()
  shapes = [('additive', [[2 * g, 2 * g + 1] for g in range(G)], [('se', 0.0)] * G) for G in (1, 5, 20)]
  shapes.append(('product', [[0, 1, 2, 3], [4, 5, 6, 7]], [('se', 0.0), ('matern', 2.5)]))
  rows = []
  for n in (1000, 4096):
    for family, groups, kinds in shapes:
      d = sum(len(g) for g in groups)
      P = sum((len(g) + 3) // 4 * 4 for g in groups)
      rs = np.random.RandomState(n + d)
      X = rs.random_sample((n, max(d, P)))
      y = np.sin(3.0 * X[:, :2].sum(axis=1)) + 0.05 * rs.standard_normal(n)
      yc = y - y.mean()
      spec = grouped_spec(family, groups, kinds, rs, d)
      single = KernelSpec('se', P, 1.3, (0.35 + 0.4 * rs.random_sample(P)) * np.sqrt(max(P, 3) / 3.0))
      Xg, Xs = eng.to_device(np.ascontiguousarray(X[:, :d])), eng.to_device(np.ascontiguousarray(X[:, :P]))
      fit_ms = median_ms(eng, lambda: eng.gp_fit(spec, Xg, yc, 1e-2))
      fit, fit_single = eng.gp_fit(spec, Xg, yc, 1e-2), eng.gp_fit(single, Xs, yc, 1e-2)
      rounds = [(median_ms(eng, fit.lml_grad_groups), median_ms(eng, fit_single.lml_grad)) for _ in range(2)]
      eng.timings(True)
      for _ in range(REPS):
        fit.lml_grad_groups()
      sec = eng.timings(False)
      grouped_ms, single_ms = min(r[0][0] for r in rounds), min(r[1][0] for r in rounds)
      rows.append({'n': n, 'family': family, 'groups': len(groups), 'd': d, 'P': P,
                   'fit_ms': stats(fit_ms),
                   'lml_grad_groups_ms': [stats(r[0]) for r in rounds],
                   'single_kernel_same_P_lml_grad_ms': [stats(r[1]) for r in rounds],
                   'lml_grad_groups_over_fit': grouped_ms / fit_ms[0],
                   'lml_grad_groups_over_single': grouped_ms / single_ms,
                   'ms_per_group_beyond_single': (grouped_ms - single_ms) / len(groups),
                   'sections_ms_per_call': {k: v / REPS for k, v in sec.items() if v > 0}})
      print(json.dumps(rows[-1]), flush=True)
      Xg.free(); Xs.free()
  record = {'what': 'dfh_gp_lml_grad_groups against dfh_gp_fit of the same handle and dfh_gp_lml_grad on a single SE kernel of '
                    'the same n and packed width P; device events, %d warm-ups, median of %d, two alternating rounds (the '
                    'ratios use the smaller median of each); the cost per group carries no target: this is the baseline'
                    % (WARMUP, REPS),
            'device': 'MI355X (gfx950), one GPU', 'rows': rows}
  with open(out, 'w') as f:
    json.dump(record, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
