"""Child of tests/test_gpu_trsolve.py: the triangular solves with DFH_REFINE_FORCE_STEPS = 1, 2 or 3 in the environment (the
switch is read once per process), so that every copy of the refinement step -- few-row, wide and backward row solves,
the two single-vector routes -- runs on purpose, once, twice and three times.

Easy factors (tests/trsolve_cases.py): refining a good solution must leave it good -- a stale residual or an aliased
buffer leaves an error of order one -- under the same two assertions as without steps, and the step counter must equal
steps x blocks for every solve.  With three steps the hard factor at n = 1088 as well, every form held to the backward
error of the naturally refined solve: there a later step that reuses an earlier residual shows.  Then the call sites at the GP level, one well-conditioned SE fit at n = 1100 against
oracle.ref_numpy.GPOracle at the project's 1e-10: alpha and lml, predict with m = 5, 256 and 300, predict with three
points in progress, predict_covar, append of 7 rows (odd leading dimension of the appended block) and of 8, and
add_ucb_all on a two-group additive fit.  Prints OK."""
import os
import sys

import numpy as np

import trsolve_cases as T
from oracle import ref_numpy as O

GP_TOL = 1e-10


def easy_cases(eng, steps):
  for n, k, upper in T.FORCED_CASES:
    L, B, X = T.easy_problem(n, upper, k)
    Bk = T.columns(B, k)
    Xd, got = T.booked(eng, lambda: eng.solve_triangular(L, Bk, upper=upper))     # pylint: disable=cell-var-from-loop
    what = 'forced %d: n %d nrhs %d upper %d' % (steps, n, k, upper)
    assert T.families(got) == T.expected_launches(n, k, upper, steps=steps), (what, got)
    T.check_easy(L, Xd, Bk, T.columns(X, k), upper, what)


def hard_cases(eng, steps):
  """ Three steps are what the worst block of a hard factor asks for (delta up to 2e-5), one more than most need: every
      form must reach the backward error of the naturally refined solve with them -- a second or third step that works
      from an earlier residual stays at the error of the first. """
  n = 1088
  for upper in (False, True):
    L, B, Xref, formula = T.hard_problem(n, upper)
    assert max(formula) <= steps
    A = L.T if upper else L
    for k in T.HARD_NRHS:
      Bk = T.columns(B, k)
      Xd, got = T.booked(eng, lambda: eng.solve_triangular(L, Bk, upper=upper))   # pylint: disable=cell-var-from-loop
      assert T.families(got) == T.expected_launches(n, k, upper, steps=steps), (n, k, upper, got)
      r_dev, r_ref = T.ratio(A, Xd, Bk), T.ratio(A, T.columns(Xref, k), Bk)
      print('forced %d, hard: n %d nrhs %d upper %d  device / scipy %.2f' % (steps, n, k, upper, r_dev / r_ref))
      assert r_dev <= T.BACKWARD_ERROR_FACTOR * r_ref, (k, upper, r_dev / r_ref)


def _close(a, b, what):
  e = T.relerr(a, b)
  print('%-34s %.2e' % (what, e))
  assert e < GP_TOL, (what, e)


def gp_call_sites(eng, steps):
  from dragonfly_amd.engine import KernelSpec
  n, d = 1100, 6
  nblk = T.nblocks(n)
  rs = np.random.RandomState(1100)
  X = rs.rand(n + 8, d)
  Y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.randn(n + 8)
  bw = np.full(d, 0.5)
  scale, noise = float(Y.var()), float(Y.var() / 20)
  spec, ospec = KernelSpec('se', d, scale, bw), O.KernelSpec('se', d, scale, bw)
  before = eng.solve_launches()['refine_steps']
  gp = eng.gp_fit(spec, X[:n], Y[:n], noise)
  assert list(gp.refine_steps()) == [steps] * nblk
  assert eng.solve_launches()['refine_steps'] - before == 2 * steps * nblk      # alpha: a forward and a backward solve
  og = O.GPOracle(X[:n], Y[:n], ospec, 0.0, noise)
  _close(gp.get_alpha(), og.alpha, 'alpha')
  assert abs(gp.lml - og.lml()) <= GP_TOL * abs(og.lml()), (gp.lml, og.lml())
  for m in (5, 256, 300):                                                        # few-row, its last size, wide
    Xs = rs.rand(m, d)
    (mu, sd), got = T.booked(eng, lambda: gp.predict(Xs))                        # pylint: disable=cell-var-from-loop
    assert got['refine_steps'] == steps * nblk, (m, got)
    mur, sdr = og.eval(Xs, 'std')
    _close(mu, mur, 'predict m = %d: mu' % m)
    _close(sd, sdr, 'predict m = %d: sd' % m)
  Xs, Xh = rs.rand(40, d), rs.rand(3, d)
  mu, sd = gp.predict(Xs, X_halluc=Xh)
  mur, sdr = og.eval_with_hallucinated_observations(Xs, Xh)
  _close(mu, mur, 'three points in progress: mu')
  _close(sd, sdr, 'three points in progress: sd')
  mu, cov = gp.predict_covar(Xs)
  mur, covr = og.eval(Xs, 'covar')
  _close(mu, mur, 'predict_covar m = 40: mu')
  _close(cov, covr, 'predict_covar m = 40: covariance')
  for q in (7, 8):                                                               # n + q odd, even
    g2 = gp.append(X[n:n + q], Y[:n + q])
    o2 = O.GPOracle(X[:n + q], Y[:n + q], ospec, 0.0, noise)
    _close(g2.get_alpha(), o2.alpha, 'append of %d rows: alpha' % q)
    _close(g2.get_L(), o2.L, 'append of %d rows: L' % q)
    assert abs(g2.lml - o2.lml()) <= GP_TOL * abs(o2.lml()), (q, g2.lml, o2.lml())
    g2.free()
  gp.free()
  # add-UCB of an additive GP: every group's cross matrix stacked into one row solve
  d, groups = 4, [[0, 1], [2, 3]]
  Xa = rs.rand(n, d)
  Ya = np.sin(3 * Xa[:, :2].sum(axis=1)) + np.cos(2 * Xa[:, 2:].sum(axis=1)) + 0.05 * rs.randn(n)
  bws = [np.full(2, 0.4), np.full(2, 0.6)]
  scale, noise = float(Ya.var()), float(Ya.var() / 20)
  aspec = KernelSpec('additive', d, scale, groups=groups, sub_kinds=['se'] * 2, sub_scales=[1.0] * 2, sub_nus=[0.0] * 2,
                     sub_bandwidths=bws)
  oa = O.GPOracle(Xa, Ya, O.KernelSpec('additive', d, scale, groups=groups, subs=[O.KernelSpec('se', 2, 1.0, b) for b in bws]),
                  0.0, noise)
  ga = eng.gp_fit(aspec, Xa, Ya, noise)
  _close(ga.get_alpha(), oa.alpha, 'additive fit: alpha')
  cands = [rs.rand(40, 2), rs.rand(37, 2)]
  betas = [O.add_ucb_beta_th(2, n)] * 2
  (bvs, bis, vals), got = T.booked(eng, lambda: ga.add_ucb_all(betas, cands, return_vals=True))
  assert got['refine_steps'] == steps * nblk, got
  for j in range(2):
    vr = O.add_ucb_group_values(oa, j, cands[j], n)
    _close(vals[j], vr, 'add_ucb_all: group %d' % j)
    assert bis[j] == int(np.argmax(vr)) and bvs[j] == vals[j][bis[j]]
  ga.free()


def main():
  from dragonfly_amd.engine import get_engine
  steps = int(os.environ.get('DFH_REFINE_FORCE_STEPS', '-1'))
  assert steps in (1, 2, 3), 'run with DFH_REFINE_FORCE_STEPS = 1, 2 or 3'
  eng = get_engine()
  easy_cases(eng, steps)
  if steps == 3:
    hard_cases(eng, steps)
  gp_call_sites(eng, steps)
  print('OK')


if __name__ == '__main__':
  sys.exit(main())
