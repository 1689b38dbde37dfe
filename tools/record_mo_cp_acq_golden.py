"""Writes tests/golden/mo_cp_acq_n70.npz: what the reference computes, ONE POINT PER CALL, when it maximises a
multi-objective acquisition over random samples of a Cartesian-product domain (opt/gpb_acquisitions.py:35-37,
exd/exd_utils.py:265; opt/multiobjective_gpb_acquisitions.py:19-106) -- per candidate and objective the posterior and the
one-point Thompson draw, and the scalarised values of the reference's OWN mo_lin_asy_ts / mo_tch_asy_ts / mo_lin_asy_ucb /
mo_tch_asy_ucb closures, called one point at a time -- for tests/test_gpu_mo_cp.py.  Runs the real reference on the CPU;
nothing under oracle/ is changed.

    python tools/record_mo_cp_acq_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

The data: the mixed domain of tools/record_cp_acq_golden.py -- a 2-D SE part, an integer Matern part, a Hamming part of
two columns -- 70 training points, 257 candidates (candidate DUP_CAND equal to training point DUP_TRAIN), K = 3 GPs on the
same points with different scales, bandwidths, Matern nu (2.5 / 1.5 / 0.5), Hamming weights, noise and constant means,
fitted with 'project_first' as every CPGP is, and Q = 2 points in progress.  U holds the m K normals POINT-major, U[i, j]
for candidate i and objective j: the order in which the reference's loop over points, with the closure's loop over
objectives inside, takes them from the global stream, one np.random.normal(size=(1, 1)) each.  The file holds numbers
only.  Every arg-max is checked here to be decided by more than MIN_GAP of the largest value and every variance to be
positive; a seed that fails a check is replaced, never tolerated.
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
N, M, Q, K = 70, 257, 2, 3
DUP_CAND, DUP_TRAIN = 100, 17
SEED = 20250317
MIN_GAP = 1e-8
SCALES = [1.7, 0.9, 2.4]
SE_BWS = [[0.45, 0.8], [0.3, 0.55], [0.9, 0.6]]
MATERN_NUS = [2.5, 1.5, 0.5]
MATERN_BWS = [[2.5], [1.6], [3.2]]
HAMMING_WS = [[0.6, 0.4], [0.5, 0.5], [0.25, 0.75]]
NOISES = [0.02, 0.05, 0.01]
WEIGHTS = [0.5, 0.3, 0.2]
REFERENCE_POINT = [-1.5, -2.0, -1.0]
DIM = 5


def points(rng, n):
  """ list-of-lists points and the same packed: [x0, x1 | k | c0, c1] """
  x = rng.random_sample((n, 2))
  k = rng.randint(1, 8, size=(n, 1))
  c = rng.randint(0, 3, size=(n, 2))
  packed = np.hstack([x, k.astype(float), c.astype(float)])
  return [[x[i].copy(), [int(k[i, 0])], [int(c[i, 0]), int(c[i, 1])]] for i in range(n)], packed


def objectives(packed):
  """ the K objectives on packed points, [K x n] """
  x0, x1, k, c0, c1 = packed.T
  return np.array([np.sin(3 * x0) + x1 ** 2 - 0.05 * (k - 4) ** 2 + 0.3 * (c0 == c1),
                   np.cos(4 * x1) - (x0 - 0.6) ** 2 + 0.1 * k - 0.2 * (c0 == 2),
                   x0 * x1 - 0.03 * (k - 2) ** 2 + 0.25 * (c1 == 0) - 0.1 * (c0 == 1)])


def top2(vals):
  """ (winner by np.argmax, gap between the two largest values relative to the largest magnitude) """
  vals = np.asarray(vals, dtype=float)
  order = np.sort(vals)
  return int(np.argmax(vals)), float((order[-1] - order[-2]) / np.max(np.abs(vals)))


class _Domain(object):
  """ what the reference's closures read of a CartesianProductDomain: its type and its dimension (:79, :96) """
  dim = DIM

  def get_type(self):
    return 'cartesian_product'


def main():
  sys.path.insert(0, ROOT)
  from oracle.make_golden import import_reference
  if len(sys.argv) > 1:
    os.environ['DRAGONFLY_REFERENCE'] = sys.argv[1]
  import_reference()
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.cartesian_product_gp import CPGP
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  rng = np.random.RandomState(SEED)
  X, Xp = points(rng, N)
  Y = objectives(Xp) + 0.05 * rng.standard_normal((K, N))
  C, Cp = points(rng, M)
  C[DUP_CAND], Cp[DUP_CAND] = X[DUP_TRAIN], Xp[DUP_TRAIN]
  H, Hp = points(rng, Q)
  mean_consts = [float(np.mean(Y[j])) for j in range(K)]
  gps = []
  for j in range(K):
    kern = ref_kernel.CartesianProductKernel(SCALES[j], [ref_kernel.SEKernel(2, 1.0, SE_BWS[j]),
                                                         ref_kernel.MaternKernel(1, MATERN_NUS[j], 1.0, MATERN_BWS[j]),
                                                         ref_kernel.HammingKernel(HAMMING_WS[j])])
    assert kern.is_guaranteed_psd()
    gps.append(CPGP(X, list(Y[j]), kern, lambda x, _c=mean_consts[j]: np.array([_c] * len(x)), NOISES[j],
                    handle_non_psd_kernels='project_first'))
  t = N + 1
  beta = float(ref_moo._get_ucb_beta_th(DIM, t))       # pylint: disable=protected-access
  out = dict(Xp=Xp, Y=Y, Cp=Cp, Hp=Hp, mean_consts=np.array(mean_consts), noises=np.array(NOISES), scales=np.array(SCALES),
             se_bws=np.array(SE_BWS), matern_nus=np.array(MATERN_NUS), matern_bws=np.array(MATERN_BWS),
             hamming_ws=np.array(HAMMING_WS), weights=np.array(WEIGHTS), reference_point=np.array(REFERENCE_POINT),
             beta=beta, t=t, dim=DIM, dup_cand=DUP_CAND, dup_train=DUP_TRAIN, min_gap=MIN_GAP)
  np.random.seed(SEED + 1)
  out['U'] = U = np.random.normal(size=(M, K))         # POINT-major: U[i, j]

  # the reference's closures as its maximiser sees them on these domains: acq_fn([x]), one point per call
  captured = {}
  def capture(acq_fn, anc_data, *args, **kwargs):       # pylint: disable=unused-argument
    captured['values'] = np.array([float(np.ravel(acq_fn([x]))[0]) for x in C])
  saved = ref_moo.maximise_acquisition
  ref_moo.maximise_acquisition = capture
  try:
    for q in (0, Q):
      tag = 'q%d' % q
      anc = Namespace(domain=_Domain(), acq_opt_method='rand', max_evals=M, t=t, is_mf=False, handle_parallel='halluc',
                      eval_points_in_progress=H if q else [], obj_weights=WEIGHTS, reference_point=REFERENCE_POINT)
      if q:
        one = lambda gp, x: gp.eval_with_hallucinated_observations([x], H, uncert_form='std')
        draw = lambda gp, x: gp.draw_samples_with_hallucinated_observations(1, [x], H)
      else:
        one = lambda gp, x: gp.eval([x], uncert_form='std')
        draw = lambda gp, x: gp.draw_samples(1, [x])
      post = [[one(gp, x) for x in C] for gp in gps]
      mu = np.array([[float(p[0][0]) for p in row] for row in post])
      sd = np.array([[float(p[1][0]) for p in row] for row in post])
      assert np.all(sd * sd > 0), 'a variance is not positive (%s): choose another seed' % tag
      # the m K one-point draws in the reference's order: the point loop outside, the objective loop inside
      np.random.seed(SEED + 1)
      draws = np.array([[float(np.ravel(draw(gp, x))[0]) for gp in gps] for x in C]).T        # [K x M]
      assert np.max(np.abs(draws - (sd * U.T + mu))) < 1e-12
      out['mu_' + tag], out['sd_' + tag], out['draws_' + tag] = mu, sd, draws
      vals = {}
      for scal, fn in (('lin', ref_moo.mo_lin_asy_ts), ('tch', ref_moo.mo_tch_asy_ts)):
        np.random.seed(SEED + 1)
        fn(gps, anc)
        vals[scal + '_ts'] = captured.pop('values')
      # the closures' values are the scalarised draws, in this order of the normals, bit for bit
      lin = 0.0
      for j in range(K):
        lin = lin + draws[j] * WEIGHTS[j]
      assert np.array_equal(vals['lin_ts'], lin)
      if q == 0:                                         # (UCB ignores the points in progress: the closures call gp.eval)
        for scal, fn in (('lin', ref_moo.mo_lin_asy_ucb), ('tch', ref_moo.mo_tch_asy_ucb)):
          fn(gps, anc)
          vals[scal + '_ucb'] = captured.pop('values')
      for name, v in vals.items():
        win, gap = top2(v)
        assert np.all(np.isfinite(v)), (name, tag)
        assert gap > MIN_GAP, 'top-two gap %.2e of %s (%s): choose another seed' % (gap, name, tag)
        out['%s_%s' % (name, tag)], out['%s_win_%s' % (name, tag)], out['%s_gap_%s' % (name, tag)] = v, win, gap
        print('%-8s %s winner %3d gap %.3e' % (name, tag, win, gap))
      print('smallest variance (%s) %.3e' % (tag, float(np.min(sd * sd))))
  finally:
    ref_moo.maximise_acquisition = saved
  path = os.path.join(OUT, 'mo_cp_acq_n70.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
