"""Times one decision of BOCA's point choice on the device against the routes it replaces and writes
profiles/boca_decision.json.

    python tools/boca_bench.py [--out profiles/boca_decision.json] [--sizes 200,1000,4000]

Per n in {200, 1000, 4000}, p = 1 fidelity column, d = 6, m = 10 000 candidates: medians of 5 wall-clock samples after 2
warm-up calls, every sample ending with the winner on the host (every route synchronises before it returns).
  add_ucb  fused     gpb_acquisitions.asy_add_ucb_for_boca: candidates in HBM, one dfh_mf_add_ucb_all call
           host      what the parent commit does for the same decision, restated (the reference is not on the GPU
                     machine): L and alpha fetched to the host, then per group the reference's arithmetic
                     (opt/gpb_acquisitions.py:353-374) in NumPy / SciPy -- kernels of oracle/ref_numpy.py, one
                     solve_triangular of n x m_j
  ucb, ts  fused     the acquisition on BOCA's view (FidelToOptGP): candidates joined with the fidelity in HBM, one fused call
           closure   the closure route of the same commit: view -> batched eval_at_fidel / draw_samples on host
                     candidates -> host formula and np.argmax
  cross    the cross-matrix section (dfh_ctx_timings 'cross': packing, the kernel, the mean product) of one add-UCB
           group call, m = 10 000, the 3-column Matern group: the weighted instance (kernmat_colw_kernel, through
           dfh_mf_add_ucb_group) beside the unweighted one on the same shape (kernmat_kernel<2, true>, through
           dfh_gp_add_ucb_group of the additive GP of the domain columns); min / median / max of 7 calls each.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, D, M = 1, 6, 10000
GROUPS = [[0], [1, 2], [3, 4, 5]]
REPS, WARM = 5, 2


def stats_ms(fn, reps=REPS):
  for _ in range(WARM):
    fn()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


class Box(object):
  def __init__(self, bounds):
    self.bounds = bounds

  def get_type(self):
    return 'euclidean'


def host_add_ucb(gp, z_opt, anc, dbw, kern_scale):
  """ the parent commit's route for BOCA's add-UCB: the factor and alpha on the host, the reference's loop in NumPy """
  from scipy.linalg import solve_triangular
  from oracle import ref_numpy as O
  from dragonfly_amd.general_utils import map_to_bounds
  L, alpha = gp.device_gp.get_L(), gp.device_gp.get_alpha()
  ZZ, XX = np.asarray(gp.ZZ), np.asarray(gp.XX)
  fid = O.KernelSpec('se', P, 1.0, np.array([0.6]))
  w = fid(ZZ, z_opt.reshape(1, -1))
  kff = float(fid(z_opt.reshape(1, -1), z_opt.reshape(1, -1)))
  point = np.zeros(D)
  m_j = anc.max_evals // len(GROUPS)
  for grp in GROUPS:
    kern_j = O.KernelSpec('matern', len(grp), 1.0, dbw[grp], nu=2.5)
    X_j = map_to_bounds(np.random.random((m_j, len(grp))), anc.domain_bounds[grp])
    K_tetr = kern_scale * np.repeat(w.T, m_j, axis=0) * kern_j(X_j, XX[:, grp])
    mu = K_tetr.dot(alpha)
    V = solve_triangular(L, K_tetr.T, lower=True)
    var = kern_scale * kff * 1.0 - (V * V).sum(axis=0)          # diag(k_j(x, x)) = 1 for a Matern kernel of scale 1
    beta = np.sqrt(0.2 * len(grp) * np.log(2 * len(grp) * anc.t + 1))
    point[grp] = X_j[int(np.argmax(mu + beta * np.sqrt(var)))]
  return point


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'boca_decision.json'))
  ap.add_argument('--sizes', default='200,1000,4000')
  args = ap.parse_args()
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, mf_gp
  from dragonfly_amd.engine import get_engine, KernelSpec
  engine = get_engine()
  rs = np.random.RandomState(0)
  bounds = np.array([[0.0, 1.0]] * D)
  z_opt = np.ones(P)
  dbw = 0.4 + 0.1 * np.arange(D)
  kern_scale, noise = 0.9, 0.02
  rows = []
  for n in [int(s) for s in args.sizes.split(',')]:
    ZZ, XX = rs.random_sample((n, P)), rs.random_sample((n, D))
    YY = np.sin(3 * XX.sum(axis=1)) * (0.5 + ZZ[:, 0]) + 0.05 * rs.standard_normal(n)
    mean_c = float(np.median(YY))
    mean = lambda x, _c=mean_c: np.array([_c] * len(x))
    add_kernel = K.AdditiveKernel(1.0, [K.MaternKernel(len(g), 2.5, 1.0, dbw[g]) for g in GROUPS], GROUPS)
    add_gp = mf_gp.EuclideanMFGP(list(ZZ), list(XX), list(YY), None, kern_scale, K.SEKernel(P, 1.0, np.array([0.6])), add_kernel, mean, noise)
    gp = mf_gp.EuclideanMFGP(list(ZZ), list(XX), list(YY), None, kern_scale, K.SEKernel(P, 1.0, np.array([0.6])),
                             K.MaternKernel(D, 2.5, 1.0, dbw), mean, noise)
    anc = Namespace(curr_acq='ucb', max_evals=M, t=n, domain=Box(bounds), domain_bounds=bounds, curr_max_val=float(YY.max()),
                    acq_opt_method='rand', eval_points_in_progress=[], eval_fidels_in_progress=[], handle_parallel='halluc',
                    is_mf=True, eval_fidel_points_in_progress=[])
    view = A.FidelToOptGP(gp, z_opt)
    beta = A._get_ucb_beta_th(D, n)        # pylint: disable=protected-access
    runs = {
      ('add_ucb', 'fused'): lambda: A.asy_add_ucb_for_boca(add_gp, z_opt, anc),
      ('add_ucb', 'host'): lambda: host_add_ucb(add_gp, z_opt, anc, dbw, kern_scale),
      ('ucb', 'fused'): lambda: A.asy_ucb(view, anc),
      ('ucb', 'closure'): lambda: A._host_acquisition(view, anc, lambda mu, sd: mu + beta * sd),      # pylint: disable=protected-access
      ('ts', 'fused'): lambda: A.asy_ts(view, anc),
      ('ts', 'closure'): lambda: A.maximise_acquisition(A.get_gp_sampler_for_parallel_strategy(view, anc), anc, vectorised=True),
    }
    # both routes of a pair draw the same candidates from the same seed: they must choose the same point
    for acq in ('add_ucb', 'ucb', 'ts'):
      other = 'host' if acq == 'add_ucb' else 'closure'
      picks = []
      for route in ('fused', other):
        np.random.seed(1)
        picks.append(np.asarray(runs[(acq, route)]()))
      row = dict(acq=acq, n=n, m=M, same_point=bool(np.array_equal(picks[0], picks[1])))
      for route in ('fused', other):
        row[route] = stats_ms(runs[(acq, route)])
      row['%s_over_fused' % other] = row[other]['median_ms'] / row['fused']['median_ms']
      rows.append(row)
      print(row, flush=True)
    # the weighted cross-matrix instance beside the unweighted one: the 3-column group, m = 10 000
    add_only = engine.gp_fit(KernelSpec('additive', D, kern_scale, groups=GROUPS, sub_kinds=['matern'] * 3, sub_scales=[1.0] * 3,
                                        sub_nus=[2.5] * 3, sub_bandwidths=[dbw[g] for g in GROUPS]), XX, YY - mean_c, noise)
    Xg = engine.to_device(rs.random_sample((M, 3)))
    cross = {}
    for name, call in (('weighted', lambda: add_gp.device_gp.mf_add_ucb_group(z_opt, 2, 1.5, Xg)),
                       ('unweighted', lambda: add_only.add_ucb_group(2, 1.5, Xg))):
      for _ in range(WARM):
        call()
      ts = []
      for _ in range(7):
        engine.timings(True)
        call()
        ts.append(engine.timings(True)['cross'])
      cross[name] = dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))
    engine.timings(False)
    cross['weighted_minus_unweighted_ms'] = cross['weighted']['median_ms'] - cross['unweighted']['median_ms']
    cross['spread_ms'] = max(cross['weighted']['max_ms'] - cross['weighted']['min_ms'], cross['unweighted']['max_ms'] - cross['unweighted']['min_ms'])
    rows.append(dict(acq='cross section of one add-UCB group call', n=n, m=M, group_columns=3, **cross))
    print(rows[-1], flush=True)
    Xg.free(); add_only.free()
  out = dict(device=engine.name(), fidelity_dim=P, dim=D, candidates=M, repetitions=REPS, warmup=WARM,
             statistic='median wall-clock ms per decision (cross: ms of the section per call)', rows=rows)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
