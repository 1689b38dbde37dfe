"""GPU: BOCA's decision step on the device (csrc/gp_mf.hip, the weighted cross-matrix kernel of csrc/km_generic.hip)
against what the real reference recorded (tests/golden/boca_*.npz, tools/make_boca_golden.py): dfh_join_fixed_columns,
dfh_mf_add_ucb_group / _all, the fused calls on joint points that BOCA's view takes, eight decisions of boca() with the
GP's data growing, and the bad-argument cases.  Bounds: values 1e-10 relative (the project's parity bar, SURVEY.md
section 8d; max|a - b| / max|b| as conftest.relerr), arg-max indices and decisions equal."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest

from conftest import load_golden, relerr
from dragonfly_amd import _lib
from dragonfly_amd.engine import KernelSpec, _ptr
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

GROUPS = [[0], [1, 2], [3, 4, 5]]
KIND_NAMES = {0: 'se', 1: 'matern', 5: 'expdecay'}


def _mf_additive_spec(p, kern_scale, fid_kind, fid_nu, fid_bw, add_scale, sub_kinds, sub_bws):
  """ kern_scale * k_fid(z) * (add_scale * sum_j k_j(x_j)) over joint points [z, x], groups of sizes (1, 2, 3) """
  groups = [list(range(p))] + [[p + c for c in g] for g in GROUPS]
  return KernelSpec('product', p + 6, kern_scale, groups=groups, sub_kinds=[fid_kind] + list(sub_kinds),
                    sub_scales=[1.0] * 4, sub_nus=[fid_nu] + [2.5 if k == 'matern' else 0.0 for k in sub_kinds],
                    sub_bandwidths=[fid_bw] + list(sub_bws), group_factors=[0, 1, 1, 1], factor_sums=[False, True],
                    factor_scales=[1.0, add_scale])


def _adducb_gp(engine, g):
  p = g['ZZ'].shape[1]
  off = g['group_off']
  sub_kinds = [KIND_NAMES[int(k)] for k in g['sub_kinds']]
  sub_bws = [g['sub_bw'][off[j]:off[j + 1]] for j in range(3)]
  spec = _mf_additive_spec(p, float(g['kern_scale']), KIND_NAMES[int(g['fid_kind'])], float(g['fid_nu']), g['fid_bw'],
                           float(g['add_scale']), sub_kinds, sub_bws)
  return engine.gp_fit(spec, np.hstack((g['ZZ'], g['XX'])), g['YY'] - float(g['mean_c']), float(g['noise']))


def _split(flat, sizes, widths):
  out, at = [], 0
  for m, w in zip(sizes, widths):
    out.append(flat[at:at + m * w].reshape(m, w))
    at += m * w
  return out


@pytest.mark.parametrize('m,p,d', [(1, 1, 1), (37, 2, 3), (300, 1, 6)])
def test_join_fixed_columns_is_hstack(engine, m, p, d):
  rs = np.random.RandomState(m)
  z, X = rs.random_sample(p), rs.random_sample((m, d))
  got = engine.join_fixed(z, engine.to_device(X)).download()
  assert got.shape == (m, p + d) and np.array_equal(got, np.hstack((np.tile(z, (m, 1)), X)))


@pytest.mark.parametrize('n', [70, 131])
@pytest.mark.parametrize('fid', ['se', 'expdecay'])
def test_mf_add_ucb_matches_the_reference(engine, fid, n):
  """ SE fidelity kernel with p = 2 / exponential-decay with p = 1; n = 70 (a ragged tile) and 131 (the first size past a
      128 tile); groups of sizes (1, 2, 3), SE and Matern-2.5; m_g = (1, 33, 257) and (257, 33, 1).  Values within
      1e-10, arg-max equal, _all equal to _group bit for bit. """
  g = load_golden('boca_adducb_%s_n%d' % (fid, n))
  gp = _adducb_gp(engine, g)
  betas = [O.add_ucb_beta_th(len(grp), int(g['t'])) for grp in GROUPS]
  for tag in ('a', 'b'):
    sizes = [int(s) for s in g['sizes_' + tag]]
    cands = _split(g['cands_' + tag], sizes, [1, 2, 3])
    want = np.split(g['vals_' + tag], np.cumsum(sizes)[:-1])
    bvs, bis, vals = gp.mf_add_ucb_all(g['z_opt'], betas, cands, return_vals=True)
    for j in range(3):
      err = relerr(vals[j], want[j])
      print('mf_add_ucb_all %s n=%d %s group %d m=%d: rel. err %.2e' % (fid, n, tag, j, sizes[j], err))
      assert err < 1e-10
      assert int(bis[j]) == int(g['argmax_' + tag][j]) and bvs[j] == vals[j][int(bis[j])]
      bv, bi, v = gp.mf_add_ucb_group(g['z_opt'], j, betas[j], cands[j], return_vals=True)
      assert np.array_equal(v, vals[j]) and bi == bis[j] and bv == bvs[j]
    point = np.zeros(6)
    for grp, c, i in zip(GROUPS, cands, bis):
      point[grp] = c[int(i)]
    assert np.array_equal(point, g['point_' + tag])
  gp.free()


def test_unit_weights_give_the_additive_add_ucb(engine):
  """ Where the weight sits: a constant fidelity kernel (exponential decay with power 0, offset 0: k_fid = 1 exactly) and
      an additive factor of scale 1 make the multi-fidelity GP the additive GP of the domain columns, and its weighted
      add-UCB the existing dfh_gp_add_ucb_all of that GP.  1e-13: the two Gram matrices come from different kernels and
      agree to an ulp (1.1e-16), alpha and the factor to that times the condition number -- n * scale / noise, about 200
      with the noise variance chosen here -- and the values are sums of products of the two. """
  rs = np.random.RandomState(5)
  n, scale, noise = 70, 0.7, 0.5
  Z, X = rs.random_sample((n, 1)), rs.random_sample((n, 6))
  y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.randn(n)
  kinds, bws = ['se', 'matern', 'matern'], [np.array([0.4]), np.array([0.5, 0.6]), np.array([0.45, 0.7, 0.8])]
  mf = engine.gp_fit(_mf_additive_spec(1, scale, 'expdecay', 0.0, np.array([0.0]), 1.0, kinds, bws), np.hstack((Z, X)), y, noise)
  add = engine.gp_fit(KernelSpec('additive', 6, scale, groups=GROUPS, sub_kinds=kinds, sub_scales=[1.0] * 3,
                                 sub_nus=[0.0, 2.5, 2.5], sub_bandwidths=bws), X, y, noise)
  cands = [rs.random_sample((m, len(grp))) for m, grp in zip((33, 257, 1), GROUPS)]
  betas = [1.3, 0.7, 2.1]
  bv1, bi1, v1 = mf.mf_add_ucb_all(np.array([0.8]), betas, cands, return_vals=True)
  bv2, bi2, v2 = add.add_ucb_all(betas, cands, return_vals=True)
  for j in range(3):
    err = relerr(v1[j], v2[j])
    print('unit weights, group %d: rel. difference %.2e' % (j, err))
    assert err < 1e-13
  assert np.array_equal(bi1, bi2)
  mf.free(); add.free()


def _view_gp(engine, g, n=None):
  n = len(g['YY']) if n is None else n
  spec = KernelSpec('product', 4, float(g['kern_scale']), groups=[[0], [1, 2, 3]], sub_kinds=['se', 'matern'], sub_scales=[1.0, 1.0],
                    sub_nus=[0.0, 2.5], sub_bandwidths=[g['fid_bw'], g['dom_bw']])
  return engine.gp_fit(spec, np.hstack((g['ZZ'], g['XX']))[:n], g['YY'][:n] - float(g['mean_c']), float(g['noise']))


@pytest.fixture(scope='module')
def view_case(engine):
  g = load_golden('boca_view_n70')
  gp = _view_gp(engine, g)
  joint = engine.join_fixed(g['z_opt'], engine.to_device(g['cands']))
  return g, gp, joint


@pytest.mark.parametrize('q', [0, 2])
@pytest.mark.parametrize('acq', ['ucb', 'ei', 'pi', 'ttei', 'ts'])
def test_fused_view_route_matches_the_reference(view_case, acq, q):
  """ What FidelToOptGP's fused route calls: the joint GP's fused acquisition / Thompson draw on [z*, x] rows joined in
      HBM, the joint pairs in progress as X_halluc -- against the reference's acquisitions on its Namespace view at the
      same 300 candidates (n = 70). """
  g, gp, joint = view_case
  mean_c, m = float(g['mean_c']), len(g['cands'])
  Xh = np.hstack((g['Zh'], g['Xh']))[:q] if q else None
  want = g['%s_q%d' % (acq, q)]
  if acq == 'ts':
    _, bi, vals, _ = gp.thompson(joint, g['ts_normals_q%d' % q], block=m, mean_const=mean_c, return_samples=True, X_halluc=Xh)
  else:
    params = {'ucb': (O.ucb_beta_th(3, int(g['t'])), 0.0), 'ei': (float(g['curr_max_val']), 0.0), 'pi': (float(g['curr_max_val']), 0.0),
              'ttei': tuple(g['ttei_ref_q%d' % q]) if acq == 'ttei' else None}[acq]
    _, bi, vals = gp.acq_argmax(acq, joint, params=params, mean_const=mean_c, X_halluc=Xh, return_vals=True)
  err = relerr(vals, want)
  print('view %s q=%d: rel. err %.2e' % (acq, q, err))
  assert err < 1e-10 and bi == int(np.argmax(want))


class _StubCaller(object):
  """ what boca() reads of the function caller, from the recorded arrays """

  def __init__(self, fidel_to_opt, cand_fidels, cost_ratios, info_gaps):
    self.fidel_to_opt, self.cand_fidels, self.cost_ratios, self.info_gaps = fidel_to_opt, cand_fidels, cost_ratios, info_gaps

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):
    del point, filter_by_cost
    return [np.array(z) for z in self.cand_fidels], list(self.cost_ratios)

  def get_information_gap(self, fidels):
    assert len(fidels) == len(self.info_gaps)
    return list(self.info_gaps)


class _Box(object):
  def __init__(self, bounds):
    self.bounds = bounds

  def get_type(self):
    return 'euclidean'


def test_recorded_decision_sequence(engine):
  """ Eight decisions of dragonfly_amd.gpb_acquisitions.boca on the device -- ucb, ei, ts, pi, ttei, ucb, ts, ei, every
      other one with two (fidelity, point) pairs in progress, the GP's data growing from 30 by 5 -- choose the
      (fidelity, point) the reference's boca chose from the same seeds. """
  del engine
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, mf_gp
  g = load_golden('boca_sequence')
  acqs = [['ucb', 'ei', 'pi', 'ttei', 'ts'][i] for i in g['acq_ids']]
  bounds = np.array([[0.0, 1.0]] * 3)
  mean_c = float(g['mean_c'])
  for k, acq in enumerate(acqs):
    n = int(g['n0']) + int(g['step']) * k
    ZZ, XX, YY = g['ZZ'][:n], g['XX'][:n], g['YY'][:n]
    gp = mf_gp.EuclideanMFGP(list(ZZ), list(XX), list(YY), None, float(g['kern_scale']), K.SEKernel(1, 1.0, g['fid_bw']),
                             K.MaternKernel(3, 2.5, 1.0, g['dom_bw']), lambda x: np.array([mean_c] * len(x)), float(g['noise']))
    q = 2 if k % 2 else 0
    fidels, points = list(g['Zh'][:q]), list(g['Xh'][:q])
    anc = Namespace(curr_acq=acq, max_evals=int(g['max_evals']), t=n, domain=_Box(bounds), curr_max_val=float(YY.max()),
                    acq_opt_method='rand', eval_points_in_progress=points, eval_fidels_in_progress=fidels, handle_parallel='halluc',
                    is_mf=True, mf_strategy='boca', boca_thresh_coeff=float(g['boca_thresh_coeff']),
                    boca_max_low_fidel_cost_ratio=float(g['boca_max_low_fidel_cost_ratio']), y_range=float(YY.max() - YY.min()),
                    eval_fidel_points_in_progress=gp.get_ZX_from_ZZ_XX(fidels, points))
    caller = _StubCaller(g['z_opt'], g['cand_fidels'][k], g['cost_ratios'][k], g['info_gaps'][k])
    np.random.seed(int(g['seeds'][k]))
    fidel, point = A.boca(getattr(A.asy, acq), gp, anc, caller)
    assert np.array_equal(np.asarray(point), g['points'][k]), (k, acq)
    assert np.array_equal(np.asarray(fidel, dtype=float), g['fidels'][k]), (k, acq)


def test_bad_arguments(engine):
  """ a non-product GP, a product without an additive second factor, a projected fit, a group out of range: DFH_ERR_BAD_ARG """
  rs = np.random.RandomState(3)
  n = 40
  J = rs.random_sample((n, 7))
  y = np.sin(J.sum(axis=1))
  z, Xg = np.array([1.0]), rs.random_sample((5, 1))
  kinds, bws = ['se', 'matern', 'matern'], [np.array([0.4]), np.array([0.5, 0.6]), np.array([0.45, 0.7, 0.8])]
  good = _mf_additive_spec(1, 0.7, 'se', 0.0, np.array([0.6]), 1.2, kinds, bws)
  plain = KernelSpec('product', 7, 0.7, groups=[[0], [1, 2, 3, 4, 5, 6]], sub_kinds=['se', 'matern'], sub_scales=[1.0, 1.0],
                     sub_nus=[0.0, 2.5], sub_bandwidths=[np.array([0.6]), np.full(6, 0.5)])
  cases = [('se', engine.gp_fit(KernelSpec('se', 7, 1.0, np.full(7, 0.5)), J, y, 0.05), 0),
           ('plain product', engine.gp_fit(plain, J, y, 0.05), 0),
           ('projected fit', engine.gp_fit(good, J, y, 0.05, handle_non_psd_kernels='project_first'), 0),
           ('group out of range', engine.gp_fit(good, J, y, 0.05), 3),
           ('negative group', engine.gp_fit(good, J, y, 0.05), -1)]
  bv, bi = C.c_double(0), C.c_int64(-1)
  for name, gp, group in cases:
    rc = engine.lib.dfh_mf_add_ucb_group(gp.handle, _ptr(z), group, 1.0, _ptr(Xg), 5, None, C.byref(bv), C.byref(bi))
    assert rc == _lib.DFH_ERR_BAD_ARG, (name, rc)
    if group == 0:
      ms, out_v, out_i = np.array([5, 5, 5], dtype=np.int64), np.empty(3), np.empty(3, dtype=np.int64)
      betas, flat = np.ones(3), rs.random_sample(5 * 6)
      rc = engine.lib.dfh_mf_add_ucb_all(gp.handle, _ptr(z), _ptr(betas), _ptr(flat), _ptr(ms), None, _ptr(out_v), _ptr(out_i))
      assert rc == _lib.DFH_ERR_BAD_ARG, (name, rc)
    gp.free()
  # and the good GP with a good group still answers
  gp = engine.gp_fit(good, J, y, 0.05)
  assert np.isfinite(gp.mf_add_ucb_group(z, 0, 1.0, Xg)[0])
  gp.free()
