"""Writes tests/golden/boca_*.npz from the real reference (a Dragonfly checkout, DRAGONFLY_REFERENCE or /root/reference):
the inputs and the reference's outputs of BOCA's decision step (opt/gpb_acquisitions.py:313-439) that
tests/test_gpu_boca.py holds the device to.  Data only (allow_pickle=False on the reading side).

    python tools/make_boca_golden.py

  boca_adducb_<fidelity kernel>_n<n>.npz   _add_ucb_for_boca's per-group values (the closure _mf_add_ucb_acq_j itself,
                                           reached through the name maximise_acquisition) at recorded candidates
  boca_view_n70.npz                        ucb / ei / pi / ttei values and a Thompson draw of the Namespace view
                                           (_get_fidel_to_opt_gp) at 300 recorded candidates, q = 0 and 2 pairs in progress
  boca_sequence.npz                        eight decisions of boca() itself with the GP's data growing

For every recorded arg-max the tool asserts that the best and the second-best value differ by more than 1e-8 of the
largest magnitude and that no posterior variance is within 1e-12 * scale of zero, and takes the next seed otherwise: an
arg-max decided by rounding is no test vector."""
import os
import sys
import warnings
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SIZE_LIMIT = os.path.getsize(os.path.join(GOLDEN, 'mfgp_f1_d3_n70.npz'))

GROUPS = [[0], [1, 2], [3, 4, 5]]
GROUP_KINDS = ['se', 'matern', 'matern']          # Matern: nu = 2.5
GAP, VAR_FLOOR = 1e-8, 1e-12


class Retry(Exception):
  """ this seed gives an arg-max too close to call, or a variance at zero """


def check_gap(vals):
  vals = np.asarray(vals, dtype=float)
  if not np.all(np.isfinite(vals)):
    raise Retry('non-finite value')
  if len(vals) > 1:
    top = np.sort(vals)[-2:]
    if not top[1] - top[0] > GAP * np.max(np.abs(vals)):
      raise Retry('arg-max gap')


def check_var(var, scale):
  if not np.all(np.asarray(var) > VAR_FLOOR * scale):
    raise Retry('variance at zero')


def fidel_kernel(rk, kind, p):
  if kind == 'se':
    return rk.SEKernel(p, 1.0, np.array([0.6, 0.9][:p])), dict(fid_kind=0, fid_bw=np.array([0.6, 0.9][:p]), fid_nu=0.0)
  powers = np.array([1.7, 0.8][:p])
  return rk.ExpDecayKernel(p, 1.0, 0.3, powers), dict(fid_kind=5, fid_bw=powers, fid_nu=0.3)


def data(rs, n, p, d):
  ZZ, XX = rs.random_sample((n, p)), rs.random_sample((n, d))
  ZZ[::4] = 1.0                                   # evaluations at fidel_to_opt itself, as a real run has
  YY = np.sin(3 * XX.sum(axis=1)) * (0.5 + ZZ.mean(axis=1)) + 0.05 * rs.randn(n)
  return ZZ, XX, YY


def adducb_fixture(fid_kind, p, n, seed):
  """ the reference's own closure at recorded candidates, two stackings of m_g in {1, 33, 257} """
  from dragonfly.gp import kernel as rk
  from dragonfly.gp.euclidean_gp import EuclideanMFGP
  from dragonfly.exd.domains import EuclideanDomain
  import dragonfly.opt.gpb_acquisitions as ref_acq
  rs = np.random.RandomState(seed)
  d = 6
  ZZ, XX, YY = data(rs, n, p, d)
  dbw = 0.3 + 0.12 * np.arange(d)
  subs = [rk.SEKernel(len(g), 1.0, dbw[g]) if k == 'se' else rk.MaternKernel(len(g), 2.5, 1.0, dbw[g])
          for g, k in zip(GROUPS, GROUP_KINDS)]
  add_scale, kern_scale, noise, mean_c = 1.4, 0.7, 0.02, float(np.median(YY))
  fk, fid = fidel_kernel(rk, fid_kind, p)
  gp = EuclideanMFGP(list(ZZ), list(XX), list(YY), None, kern_scale, fk, rk.AdditiveKernel(add_scale, subs, GROUPS),
                     lambda x: np.array([mean_c] * len(x)), noise)
  z_opt = np.ones(p)
  out = dict(ZZ=ZZ, XX=XX, YY=YY, kern_scale=kern_scale, add_scale=add_scale, noise=noise, mean_c=mean_c, z_opt=z_opt,
             group_off=np.cumsum([0] + [len(g) for g in GROUPS]), group_dims=np.concatenate(GROUPS),
             sub_kinds=np.array([0 if k == 'se' else 1 for k in GROUP_KINDS]), sub_bw=np.concatenate([dbw[g] for g in GROUPS]),
             t=n, **fid)
  bounds = np.array([[0.0, 1.0]] * d)
  for tag, sizes in (('a', [1, 33, 257]), ('b', [257, 33, 1])):
    cands = [rs.random_sample((m, len(g))) for m, g in zip(sizes, GROUPS)]
    vals = []
    def recorder(acq_fn, anc_j, *args, **kwargs):          # stands where random_maximise would draw its own candidates
      j = len(vals)
      v = np.asarray(acq_fn(cands[j]), dtype=float)
      check_gap(v)
      # the variance behind v, restated only to see that none is at zero: (:364-370)
      w = kern_scale * fk(gp.ZZ, [z_opt])
      K = w.T * subs[j](cands[j], XX[:, GROUPS[j]])
      V = np.linalg.solve(gp.L, K.T)
      prior = kern_scale * float(fk([z_opt], [z_opt])) * np.diag(subs[j](cands[j], cands[j]))
      check_var(prior - (V * V).sum(axis=0), kern_scale)
      vals.append(v)
      return cands[j][int(np.argmax(v))]
    anc = Namespace(max_evals=300, t=n, domain=EuclideanDomain(bounds), domain_bounds=bounds, acq_opt_method='rand',
                    curr_acq='add_ucb')
    saved = ref_acq.maximise_acquisition
    ref_acq.maximise_acquisition = recorder
    try:
      point = ref_acq.asy_add_ucb_for_boca(gp, z_opt, anc)
    finally:
      ref_acq.maximise_acquisition = saved
    out['sizes_' + tag] = np.array(sizes)
    out['cands_' + tag] = np.concatenate([c.ravel() for c in cands])
    out['vals_' + tag] = np.concatenate(vals)
    out['argmax_' + tag] = np.array([int(np.argmax(v)) for v in vals])
    out['point_' + tag] = np.asarray(point, dtype=float)
  return out


def view_gp(rk, EuclideanMFGP, ZZ, XX, YY, hp):
  fk = rk.SEKernel(1, 1.0, hp['fid_bw'])
  dk = rk.MaternKernel(XX.shape[1], 2.5, 1.0, hp['dom_bw'])
  mean_c = hp['mean_c']
  return EuclideanMFGP(list(ZZ), list(XX), list(YY), None, hp['kern_scale'], fk, dk,
                       lambda x: np.array([mean_c] * len(x)), hp['noise'])


def view_fixture(seed):
  """ the reference's acquisitions on its Namespace view at 300 recorded candidates """
  from dragonfly.gp import kernel as rk
  from dragonfly.gp.euclidean_gp import EuclideanMFGP
  from dragonfly.exd.domains import EuclideanDomain
  import dragonfly.opt.gpb_acquisitions as ref_acq
  rs = np.random.RandomState(seed)
  n, p, d, m = 70, 1, 3, 300
  ZZ, XX, YY = data(rs, n, p, d)
  hp = dict(fid_bw=np.array([0.6]), dom_bw=np.array([0.35, 0.5, 0.8]), kern_scale=0.9, noise=0.02, mean_c=float(np.median(YY)))
  gp = view_gp(rk, EuclideanMFGP, ZZ, XX, YY, hp)
  z_opt = np.ones(p)
  view = ref_acq._get_fidel_to_opt_gp(gp, z_opt)       # pylint: disable=protected-access
  cands = rs.random_sample((m, d))
  Zh, Xh = rs.random_sample((2, p)), rs.random_sample((2, d))
  bounds = np.array([[0.0, 1.0]] * d)
  out = dict(ZZ=ZZ, XX=XX, YY=YY, z_opt=z_opt, cands=cands, Zh=Zh, Xh=Xh, t=n, curr_max_val=float(YY.max()), **hp)
  for q in (0, 2):
    fidels, points = list(Zh[:q]), list(Xh[:q])
    anc = Namespace(max_evals=m, t=n, domain=EuclideanDomain(bounds), curr_max_val=float(YY.max()), acq_opt_method='rand',
                    eval_points_in_progress=points, eval_fidels_in_progress=fidels, handle_parallel='halluc', is_mf=True,
                    eval_fidel_points_in_progress=gp.get_ZX_from_ZZ_XX(fidels, points))
    got = {}
    def recorder(acq_fn, anc_data, *args, **kwargs):
      v = np.asarray(acq_fn(cands[:anc_data.max_evals]), dtype=float).ravel()
      check_gap(v)
      got['vals'] = v
      return cands[int(np.argmax(v))]
    gp_eval = ref_acq._get_gp_eval_for_parallel_strategy(view, anc, 'std')      # pylint: disable=protected-access
    check_var(gp_eval(list(cands))[1] ** 2, hp['kern_scale'])
    saved = ref_acq.maximise_acquisition
    ref_acq.maximise_acquisition = recorder
    try:
      for acq in ('ucb', 'ei', 'pi'):
        getattr(ref_acq, 'asy_' + acq)(view, anc)
        out['%s_q%d' % (acq, q)] = got['vals']
      ref_point = cands[int(np.argmax(out['ei_q%d' % q]))]
      ref_mean, ref_std = [float(np.ravel(v)[0]) for v in gp_eval([ref_point])]
      ref_acq._ttei(gp_eval, anc, ref_point)             # pylint: disable=protected-access
      out['ttei_q%d' % q] = got['vals']
      out['ttei_ref_q%d' % q] = np.array([ref_mean, ref_std])
      np.random.seed(seed + 17 + q)
      state = np.random.get_state()
      ref_acq.asy_ts(view, anc)
      out['ts_q%d' % q] = got['vals']
      np.random.set_state(state)
      out['ts_normals_q%d' % q] = np.random.normal(size=(m, 1)).ravel()      # what draw_gaussian_samples drew (general_utils.py:230)
    finally:
      ref_acq.maximise_acquisition = saved
  return out


class StubCaller(object):
  """ what boca() reads of the function caller, from recorded arrays """

  def __init__(self, fidel_to_opt, cand_fidels, cost_ratios, info_gaps):
    self.fidel_to_opt = fidel_to_opt
    self.cand_fidels, self.cost_ratios, self.info_gaps = cand_fidels, cost_ratios, info_gaps

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):
    del point, filter_by_cost
    return [np.array(z) for z in self.cand_fidels], list(self.cost_ratios)

  def get_information_gap(self, fidels):
    assert len(fidels) == len(self.info_gaps)
    return list(self.info_gaps)


SEQ_ACQS = ['ucb', 'ei', 'ts', 'pi', 'ttei', 'ucb', 'ts', 'ei']


def sequence_fixture(seed):
  """ eight decisions of the reference's boca(), the GP's data growing by five evaluations each """
  from dragonfly.gp import kernel as rk
  from dragonfly.gp.euclidean_gp import EuclideanMFGP
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.utils.general_utils import map_to_bounds
  import dragonfly.opt.gpb_acquisitions as ref_acq
  rs = np.random.RandomState(seed)
  p, d, n0, step, C = 1, 3, 30, 5, 24
  ZZ, XX, YY = data(rs, n0 + step * len(SEQ_ACQS), p, d)
  hp = dict(fid_bw=np.array([0.5]), dom_bw=np.array([0.4, 0.55, 0.7]), kern_scale=0.9, noise=0.02, mean_c=float(np.median(YY)))
  z_opt = np.ones(p)
  bounds = np.array([[0.0, 1.0]] * d)
  cand_fidels = rs.random_sample((len(SEQ_ACQS), C, p)) * 0.95
  cost_ratios = 0.2 + 0.8 * cand_fidels.mean(axis=2)
  info_gaps = np.abs(1.0 - cand_fidels).sum(axis=2)
  Zh, Xh = rs.random_sample((2, p)), rs.random_sample((2, d))
  out = dict(ZZ=ZZ, XX=XX, YY=YY, z_opt=z_opt, cand_fidels=cand_fidels, cost_ratios=cost_ratios, info_gaps=info_gaps, Zh=Zh,
             Xh=Xh, n0=n0, step=step, max_evals=200, boca_thresh_coeff=0.05, boca_max_low_fidel_cost_ratio=0.9,
             acq_ids=np.array([['ucb', 'ei', 'pi', 'ttei', 'ts'].index(a) for a in SEQ_ACQS]), seeds=seed + 100 + np.arange(len(SEQ_ACQS)),
             **hp)
  fidels_out, points_out, stds_out = [], [], []
  original = ref_acq.maximise_acquisition
  def spy(acq_fn, anc_data, *args, **kwargs):
    """ the reference's maximiser, then its candidates and values once more (same state, same draws) for the gap """
    state0 = np.random.get_state()
    point = original(acq_fn, anc_data, *args, **kwargs)
    state1 = np.random.get_state()
    np.random.set_state(state0)
    cands = map_to_bounds(np.random.random((anc_data.max_evals, d)), bounds)          # oper_utils.py:61-62
    vals = np.asarray(acq_fn(cands), dtype=float).ravel()
    assert np.array_equal(cands[int(np.argmax(vals))], point)
    check_gap(vals)
    np.random.set_state(state1)
    return point
  ref_acq.maximise_acquisition = spy
  try:
    for k, acq in enumerate(SEQ_ACQS):
      n = n0 + step * k
      gp = view_gp(rk, EuclideanMFGP, ZZ[:n], XX[:n], YY[:n], hp)
      q = 2 if k % 2 else 0
      fidels, points = list(Zh[:q]), list(Xh[:q])
      y_range = float(YY[:n].max() - YY[:n].min())
      anc = Namespace(curr_acq=acq, max_evals=200, t=n, domain=EuclideanDomain(bounds), curr_max_val=float(YY[:n].max()),
                      acq_opt_method='rand', eval_points_in_progress=points, eval_fidels_in_progress=fidels,
                      handle_parallel='halluc', is_mf=True, mf_strategy='boca', boca_thresh_coeff=0.05,
                      boca_max_low_fidel_cost_ratio=0.9, y_range=y_range,
                      eval_fidel_points_in_progress=gp.get_ZX_from_ZZ_XX(fidels, points))
      caller = StubCaller(z_opt, cand_fidels[k], cost_ratios[k], info_gaps[k])
      np.random.seed(int(out['seeds'][k]))
      fidel, point = ref_acq.boca(getattr(ref_acq.asy, acq), gp, anc, caller)
      # the fidelity rule must not sit on its threshold either
      _, stds = gp.eval_at_fidel(list(cand_fidels[k]), [point] * C, uncert_form='std')
      check_var(gp.eval_at_fidel([z_opt] * 1, [point], uncert_form='std')[1] ** 2, hp['kern_scale'])
      stds = stds / np.sqrt(hp['kern_scale'])
      thr = 0.05 * y_range * np.sqrt(cost_ratios[k]) * info_gaps[k]
      if np.min(np.abs(stds - thr) / thr) < 1e-6:
        raise Retry('threshold')
      fidels_out.append(np.asarray(fidel, dtype=float)); points_out.append(np.asarray(point, dtype=float)); stds_out.append(stds)
  finally:
    ref_acq.maximise_acquisition = original
  out.update(fidels=np.array(fidels_out), points=np.array(points_out), cand_stds=np.array(stds_out))
  if len(set(map(tuple, out['fidels']))) < 2:
    raise Retry('every decision chose the same fidelity')
  return out


def with_retries(make, seed):
  for attempt in range(50):
    try:
      return make(seed + 1000 * attempt)
    except Retry as e:
      print('  seed %d: %s -- next seed' % (seed + 1000 * attempt, e))
  raise RuntimeError('no seed passed the checks')


def save(name, arrays):
  path = os.path.join(GOLDEN, name + '.npz')
  np.savez(path, **{k: np.asarray(v) for k, v in arrays.items()})
  size = os.path.getsize(path)
  assert size <= SIZE_LIMIT, (name, size, SIZE_LIMIT)
  assert all(v.dtype != object for v in np.load(path, allow_pickle=False).values())
  print('wrote %s (%d bytes)' % (os.path.relpath(path, ROOT), size))


def main():
  from oracle.make_golden import import_reference
  import_reference()
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    for fid_kind, p in (('se', 2), ('expdecay', 1)):
      for n in (70, 131):
        save('boca_adducb_%s_n%d' % (fid_kind, n), with_retries(lambda seed, _f=fid_kind, _p=p, _n=n: adducb_fixture(_f, _p, _n, seed), 11 + n))
    save('boca_view_n70', with_retries(view_fixture, 23))
    save('boca_sequence', with_retries(sequence_fixture, 37))


if __name__ == '__main__':
  main()
