"""Writes tests/golden/cpmf_A_n70.npz and cpmf_B_n70.npz: what the unmodified reference computes for a multi-fidelity GP
on a Cartesian-product domain -- CPMFGP (gp/cartesian_product_gp.py:251-319) over
kernel_scale * (s_f * k_f1 * k_f2 ..) * (s_d * k_d1 * k_d2 ..) -- and for BOCA's decision step on it
(opt/gpb_acquisitions.py:314-332, 399-439), for tests/test_gpu_cpmf.py and tests/test_cpmf_cpu.py.  Runs the real
reference on the CPU; nothing under oracle/ is changed.

    python tools/record_cpmf_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

Fixture A: fidelity space = a Euclidean part (dim 1, SE) and a discrete part of 2 columns (Hamming); domain = a Euclidean
part (dim 3, Matern 2.5), an integral part (dim 1, SE) and a discrete part of 9 columns (Hamming: nine columns enter the
eight accumulators of NumPy's pairwise sum, two stay below it).  Fixture B: one SE part in the fidelity space and one
Matern-2.5 part in the domain -- product factors of a single part.  n = 70 training pairs, M = 257 candidates at
fidel_to_opt, a 37 x 70 cross matrix at random fidelities, Q = 2 (fidelity, point) pairs in progress, F = 12 candidate
fidelities of BOCA's fidelity choice.

Recorded, numbers only: the packed pairs [z | x] (categories are small integers, used as their own codes), Y and every
hyper-parameter; the Gram matrix, the cross matrix and the log marginal likelihood; mu and sigma of the candidates at
fidel_to_opt with q = 0 and q = 2 pairs in progress; the per-point values of the reference's OWN asy_ucb / asy_ei /
asy_pi / asy_ttei closures, called one point per call as its maximiser calls them on these domains; the one-point
Thompson draws for the recorded normals (the stream of M calls of np.random.normal(size=(1, 1))); and the
(fidelity, point) the reference's boca() returns for each acquisition, the maximiser's samples pinned to the
candidates, the function caller's candidate fidelities, cost ratios and information gaps pinned to recorded ones.

The tool refuses to write a fixture in which a recorded decision -- an arg-max, a cand_fidel_stds > std_thresholds
comparison, the cost-ratio arg-min -- has a relative margin below MIN_GAP, or in which a per-point variance is not
positive.  The noise variance is Var(Y) / 20.
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
N, M, Q, F, N_CROSS = 70, 257, 2, 12, 37
MIN_GAP = 1e-8
ACQS = ('ucb', 'ei', 'pi', 'ttei', 'ts')

# per fixture: the parts of the fidelity space and of the domain, (kind, columns, per-column parameters[, nu])
FIXTURES = {
  'A': dict(seed=20260311, thresh_coeff=2.5, kernel_scale=1.6, fidel_scale=0.9, domain_scale=1.25,
            fidel=[('se', 1, [0.6]), ('hamming', 2, [0.7, 0.3])],
            domain=[('matern', 3, [0.5, 0.8, 0.65], 2.5), ('se', 1, [2.5]),
                    ('hamming', 9, [0.16, 0.08, 0.12, 0.1, 0.14, 0.06, 0.09, 0.11, 0.14])]),
  'B': dict(seed=20260312, thresh_coeff=0.5, kernel_scale=1.3, fidel_scale=1.0, domain_scale=1.0,
            fidel=[('se', 1, [0.5])], domain=[('matern', 3, [0.6, 0.45, 0.9], 2.5)]),
}


def _part_points(rng, part, n, integral):
  kind, dim = part[0], part[1]
  if kind == 'hamming':
    return rng.randint(0, 3, size=(n, dim)).astype(float)
  if integral:
    return rng.randint(1, 8, size=(n, dim)).astype(float)
  return rng.random_sample((n, dim))


def space_points(rng, parts, n):
  """ the packed [n x width] block of a space and the same as lists of per-part lists; the Euclidean part after the first
      one of fixture A's domain is the integral one """
  blocks = [_part_points(rng, part, n, integral=(part[0] == 'se' and j > 0)) for j, part in enumerate(parts)]
  packed = np.hstack(blocks)
  def item(kind, row):
    return [int(v) for v in row] if kind == 'hamming' else row.copy()
  pts = [[item(part[0], blk[i]) for part, blk in zip(parts, blocks)] for i in range(n)]
  return pts, packed


def objective(Zp, Xp):
  z0 = Zp[:, 0]
  out = np.sin(3 * Xp[:, 0]) + Xp[:, 1] ** 2 - (Xp[:, 2] - 0.4) ** 2 - 0.4 * (1 - z0) ** 2
  if Zp.shape[1] > 1:
    out = out + 0.2 * (Zp[:, 1] == Zp[:, 2]) - 0.05 * (Xp[:, 3] - 4) ** 2 + 0.3 * (Xp[:, 4] == Xp[:, 5]) - 0.1 * (Xp[:, 12] == 2)
  return out


def top2(vals):
  vals = np.asarray(vals, dtype=float)
  order = np.sort(vals)
  return int(np.argmax(vals)), float((order[-1] - order[-2]) / np.max(np.abs(vals)))


def build_kernel(ref_kernel, scale, parts):
  kernels = []
  for part in parts:
    if part[0] == 'se':
      kernels.append(ref_kernel.SEKernel(part[1], 1.0, part[2]))
    elif part[0] == 'matern':
      kernels.append(ref_kernel.MaternKernel(part[1], part[3], 1.0, part[2]))
    else:
      kernels.append(ref_kernel.HammingKernel(part[2]))
  return ref_kernel.CartesianProductKernel(scale, kernels)


class _Domain(object):
  def get_type(self):
    return 'cartesian_product'


class _Caller(object):
  """ what boca() reads of the function caller, with recorded candidate fidelities """

  def __init__(self, fidel_to_opt, fidels, cost_ratios, gaps):
    self.fidel_to_opt, self.fidels, self.cost_ratios, self.gaps = fidel_to_opt, fidels, cost_ratios, gaps

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):     # pylint: disable=unused-argument
    return list(self.fidels), list(self.cost_ratios)

  def get_information_gap(self, fidels):
    assert len(fidels) == len(self.gaps)
    return list(self.gaps)


def record(name, fx, ref_kernel, CPMFGP, ref_acq):
  rng = np.random.RandomState(fx['seed'])
  ZZ, Zp = space_points(rng, fx['fidel'], N)
  XX, Xp = space_points(rng, fx['domain'], N)
  Y = objective(Zp, Xp) + 0.05 * rng.standard_normal(N)
  noise = float(np.var(Y) / 20)
  mean_c = float(np.mean(Y))
  C, Cp = space_points(rng, fx['domain'], M)
  f2o, f2o_p = space_points(rng, fx['fidel'], 1)
  f2o, f2o_p = f2o[0], f2o_p[0]
  f2o[0][0] = f2o_p[0] = 0.95
  HZ, HZp = space_points(rng, fx['fidel'], Q)
  HX, HXp = space_points(rng, fx['domain'], Q)
  TZ, TZp = space_points(rng, fx['fidel'], N_CROSS)
  TX, TXp = space_points(rng, fx['domain'], N_CROSS)
  FZ, FZp = space_points(rng, fx['fidel'], F)
  cost_ratios = np.sort(0.05 + 0.9 * rng.random_sample(F))
  gaps = 0.1 + rng.random_sample(F)
  fidel_kernel = build_kernel(ref_kernel, fx['fidel_scale'], fx['fidel'])
  domain_kernel = build_kernel(ref_kernel, fx['domain_scale'], fx['domain'])
  mean_func = lambda x: np.array([mean_c] * len(x))
  gp = CPMFGP(ZZ, XX, list(Y), None, mean_func, noise, fx['kernel_scale'], fidel_kernel, domain_kernel,
              [None] * len(fx['fidel']), [None] * len(fx['domain']))
  assert gp.kernel.is_guaranteed_psd() and gp.handle_non_psd_kernels == 'project_first'
  out = dict(Xp=np.hstack([Zp, Xp]), Y=Y, noise=noise, mean_const=mean_c, kernel_scale=fx['kernel_scale'],
             fidel_scale=fx['fidel_scale'], domain_scale=fx['domain_scale'], Cp=Cp, f2o=f2o_p, Hp=np.hstack([HZp, HXp]),
             Tp=np.hstack([TZp, TXp]), Fp=FZp, cost_ratios=cost_ratios, info_gaps=gaps, min_gap=MIN_GAP)
  for space in ('fidel', 'domain'):
    for j, part in enumerate(fx[space]):
      out['%s_par_%d' % (space, j)] = np.array(part[2], dtype=float)
  out['K'] = gp._get_training_kernel_matrix()                       # pylint: disable=protected-access
  out['K_cross'] = gp.kernel(list(zip(TZ, TX)), gp.X)
  out['lml'] = float(gp.compute_log_marginal_likelihood())
  out['alpha'] = np.ravel(gp.alpha)
  pairs = list(zip(HZ, HX))
  t = N + 1
  y_range = float(np.max(Y) - np.min(Y))
  np.random.seed(fx['seed'] + 1)
  out['U'] = U = np.array([np.random.normal(size=(1, 1))[0, 0] for _ in range(M)])

  # the maximiser's samples pinned to the candidates; the closures are called one point per call, as on these domains
  captured = []
  def pinned(acq_fn, anc_data, *args, **kwargs):                     # pylint: disable=unused-argument
    cands = C[:anc_data.max_evals]
    vals = np.array([float(np.ravel(acq_fn([x]))[0]) for x in cands])
    captured.append(vals)
    return cands[int(np.argmax(vals))]
  saved = ref_acq.maximise_acquisition
  ref_acq.maximise_acquisition = pinned
  try:
    for q in (0, Q):
      tag = 'q%d' % q
      anc = Namespace(domain=_Domain(), acq_opt_method='rand', max_evals=M, t=t, is_mf=True, handle_parallel='halluc',
                      eval_points_in_progress=HX if q else [], eval_fidel_points_in_progress=pairs if q else [],
                      curr_max_val=float(np.max(Y)), boca_thresh_coeff=fx['thresh_coeff'], y_range=y_range,
                      boca_max_low_fidel_cost_ratio=0.9)
      joint = list(zip([f2o] * M, C))
      if q:
        post = [gp.eval_with_hallucinated_observations([p], pairs, uncert_form='std') for p in joint]
      else:
        post = [gp.eval([p], uncert_form='std') for p in joint]
      mu = np.array([float(p[0][0]) for p in post])
      sd = np.array([float(p[1][0]) for p in post])
      assert np.all(sd * sd > 0), 'a variance is not positive (%s %s): choose another seed' % (name, tag)
      out['mu_' + tag], out['sd_' + tag] = mu, sd
      caller = _Caller(f2o, FZ, cost_ratios, gaps)
      for acq in ACQS:
        anc.curr_acq = acq
        seed = fx['seed'] + 1
        while True:                                                    # (TTEI: a seed whose coin takes the two-step branch)
          np.random.seed(seed)
          if acq != 'ttei' or np.random.random() >= 0.5:
            break
          seed += 1
        np.random.seed(seed)
        del captured[:]
        fidel, point = ref_acq.boca(getattr(ref_acq.asy, acq), gp, anc, caller)
        vals = captured[-1]
        if acq == 'ts':
          assert np.max(np.abs(vals - (sd * U + mu))) < 1e-12
        if acq == 'ttei':
          assert len(captured) == 2 and len(vals) == M // 2
          ref_pt = C[int(np.argmax(captured[0]))]
          _, gap0 = top2(captured[0])
          assert gap0 > MIN_GAP, 'top-two gap of TTEI\'s first step (%s %s)' % (name, tag)
          rp = [(f2o, ref_pt)]
          rm, rs = gp.eval_with_hallucinated_observations(rp, pairs, uncert_form='std') if q else gp.eval(rp, uncert_form='std')
          out['ttei_ei_%s' % tag], out['ttei_params_%s' % tag] = captured[0], np.array([float(rm[0]), float(rs[0])])
        win, gap = top2(vals)
        assert np.all(np.isfinite(vals)) and C[win] is point
        assert gap > MIN_GAP, 'top-two gap %.2e of %s (%s %s): choose another seed' % (gap, acq, name, tag)
        # the fidelity choice at that point, with its margins
        _, stds = gp.eval_at_fidel(FZ, [point] * F, uncert_form='std')
        stds = stds / np.sqrt(gp.kernel.hyperparams['scale'])
        thresholds = anc.boca_thresh_coeff * y_range * np.sqrt(cost_ratios) * gaps
        margin = float(np.min(np.abs(stds - thresholds) / np.maximum(stds, thresholds)))
        assert margin > MIN_GAP, 'a std-threshold comparison of %s (%s %s) has margin %.2e' % (acq, name, tag, margin)
        qualifying = np.where(stds > thresholds)[0]
        fid_idx = -1
        if len(qualifying) > 0:
          roots = np.sort(np.sqrt(cost_ratios)[qualifying])
          assert len(roots) == 1 or (roots[1] - roots[0]) / roots[1] > MIN_GAP
          best = qualifying[int(np.argmin(np.sqrt(cost_ratios)[qualifying]))]
          assert abs(cost_ratios[best] - anc.boca_max_low_fidel_cost_ratio) / anc.boca_max_low_fidel_cost_ratio > MIN_GAP
          if cost_ratios[best] <= anc.boca_max_low_fidel_cost_ratio:
            fid_idx = int(best)
        assert (fidel is f2o) if fid_idx < 0 else (fidel is FZ[fid_idx])
        key = '%s_%s' % (acq, tag)
        out[key], out[key + '_win'], out[key + '_gap'], out[key + '_fidel'] = vals, win, gap, fid_idx
        out[key + '_fidel_stds'], out[key + '_margin'] = stds, margin
        print('%s %-5s %s winner %3d gap %.2e fidelity %2d (%d qualify, margin %.2e)' % (name, acq, tag, win, gap, fid_idx,
                                                                                      len(qualifying), margin))
      out['beta_' + tag] = float(ref_acq._get_ucb_beta_th(ref_acq._get_gp_ucb_dim(Namespace(kernel=domain_kernel)), t))   # pylint: disable=protected-access
      print('%s %s smallest variance %.3e' % (name, tag, float(np.min(sd * sd))))
  finally:
    ref_acq.maximise_acquisition = saved
  out['thresholds'] = fx['thresh_coeff'] * y_range * np.sqrt(cost_ratios) * gaps
  out['y_range'], out['t'], out['thresh_coeff'] = y_range, t, fx['thresh_coeff']
  path = os.path.join(OUT, 'cpmf_%s_n70.npz' % name)
  np.savez_compressed(path, **out)
  check = np.load(path, allow_pickle=False)
  assert sorted(check.files) == sorted(out)
  print('wrote', path, os.path.getsize(path), 'bytes; noise %.4g = Var(Y) / 20' % noise)


def main():
  sys.path.insert(0, ROOT)
  from oracle.make_golden import import_reference
  if len(sys.argv) > 1:
    os.environ['DRAGONFLY_REFERENCE'] = sys.argv[1]
  import_reference()
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.cartesian_product_gp import CPMFGP
  import dragonfly.opt.gpb_acquisitions as ref_acq
  for name in sorted(FIXTURES):
    record(name, FIXTURES[name], ref_kernel, CPMFGP, ref_acq)


if __name__ == '__main__':
  main()
