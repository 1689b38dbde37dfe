"""CPU: dragonfly_amd.multiobjective_gpb_acquisitions over the NumPy stand-in engine (tests/oracle_engine_moo.py)
against the REAL reference's recorded outputs (tests/golden/moo_*.npz, tools/make_moo_golden.py) -- values, index,
point, final generator state -- its fall-back routes, and install(multi_objective=True) under the reference."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

from conftest import load_golden, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
MOO_NAMES = ['dragonfly.opt.multiobjective_gpb_acquisitions.%s.%s' % (ns, acq) for ns in ('asy', 'seq')
             for acq in ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb')]


def _gen():
  spec = importlib.util.spec_from_file_location('make_moo_golden', os.path.join(ROOT, 'tools', 'make_moo_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


G = _gen()


class _Box(object):
  """ what the acquisitions ask of a Euclidean domain """
  def __init__(self, dim, kind='euclidean'):
    self.bounds, self.dim, self.kind = np.array([[0.0, 1.0]] * dim), dim, kind

  def get_type(self):
    return self.kind

  def get_dim(self):
    return self.dim


def _mirror_gps(idx):
  from dragonfly_amd import kernel as K
  from dragonfly_amd.gp_core import GP
  X, objs, weights, ref_point, Xh, t = G.case_data(idx)
  return G.build_gps(K, GP, X, objs), weights, ref_point, Xh, t


@pytest.mark.parametrize('idx', range(len(G.CASES)))
def test_mirror_reproduces_the_reference_fixture(idx, monkeypatch):
  from oracle_engine_moo import patch_engine_moo
  eng = patch_engine_moo(monkeypatch)
  from dragonfly_amd import multiobjective_gpb_acquisitions as moo
  name, scal, acq, kinds, q = G.CASES[idx]
  gold = load_golden('moo_' + name)
  gps, weights, ref_point, Xh, t = _mirror_gps(idx)
  seen = {}
  for method in ('mo_ucb_argmax', 'mo_thompson'):
    def recording(*args, _orig=getattr(eng, method), **kwargs):
      kwargs['return_vals'] = True
      out = _orig(*args, **kwargs)
      seen['vals'] = out[2]
      return out[0], out[1]
    monkeypatch.setattr(eng, method, recording)
  np.random.set_state(G.unpack_state(gold['state_key'], gold['state_pos'], gold['state_gauss']))
  point = getattr(moo.asy, '%s_%s' % (scal, acq))(gps, G.anc_data_for(_Box(G.DIM), scal, weights, ref_point, Xh, t))
  after = np.random.get_state()
  assert eng.calls == [('mo_ucb_argmax' if acq == 'ucb' else 'mo_thompson', G.M)]      # one fused call
  err = relerr(seen['vals'], gold['vals'])
  print(name, 'relerr', err)
  assert err <= TOL
  assert int(np.argmax(seen['vals'])) == int(gold['best_idx']) and np.array_equal(point, gold['point'])
  want = G.unpack_state(gold['after_key'], gold['after_pos'], gold['after_gauss'])
  assert np.array_equal(after[1], want[1]) and after[2:] == want[2:]


def test_thompson_multiplies_the_budget_for_other_maximisers(monkeypatch):
  from oracle_engine_moo import patch_engine_moo
  eng = patch_engine_moo(monkeypatch)
  from dragonfly_amd import multiobjective_gpb_acquisitions as moo
  gps, weights, ref_point, Xh, t = _mirror_gps(3)
  anc = G.anc_data_for(_Box(G.DIM), 'tch', weights, ref_point, Xh, t, method='direct', max_evals=50)
  np.random.seed(1)
  moo.mo_tch_asy_ts(gps, anc)
  assert eng.calls == [('mo_thompson', 200)] and anc.max_evals == 50 and anc.acq_opt_method == 'direct'


def test_ucb_under_the_tree_search_asks_a_frontier_per_call(monkeypatch):
  from oracle_engine_moo import patch_engine_moo, scalarise_ucb
  eng = patch_engine_moo(monkeypatch)
  from dragonfly_amd import multiobjective_gpb_acquisitions as moo
  from dragonfly_amd.doo import pdoo_maximise_batched
  gps, weights, ref_point, Xh, t = _mirror_gps(1)
  anc = G.anc_data_for(_Box(G.DIM), 'tch', weights, ref_point, Xh, t, method='pdoo', max_evals=120)
  point = moo.mo_tch_asy_ucb(gps, anc)
  assert len(eng.calls) > 1 and all(c[0] == 'mo_ucb_argmax' for c in eng.calls) and max(c[1] for c in eng.calls) > 1
  # the same search over the reference's closure (K gp.eval calls per frontier)
  beta = np.sqrt(0.2 * G.DIM * np.log(2 * G.DIM * t + 1))
  def closure(x):
    evals = [gp.eval(x, uncert_form='std') for gp in gps]
    return scalarise_ucb('tch', beta, weights, ref_point, [e[0] for e in evals], [e[1] for e in evals])
  _, want, _ = pdoo_maximise_batched(closure, anc.domain.bounds, 120, frontier=32, depth=2)
  assert np.array_equal(point, want)


class _HostGP(object):
  """ anything with eval / draw_samples that is not a mirror GP with a device kernel """
  def __init__(self, gp):
    self.gp, self.evals, self.draws = gp, 0, 0

  def eval(self, x, uncert_form='none'):
    self.evals += 1
    return self.gp.eval(x, uncert_form=uncert_form)

  def draw_samples(self, num, x):
    self.draws += 1
    return self.gp.draw_samples(num, x)


@pytest.mark.parametrize('why', ['host_gp', 'is_mf'])
def test_fall_back_to_the_closure_route(why, monkeypatch):
  from oracle_engine_moo import patch_engine_moo
  eng = patch_engine_moo(monkeypatch)
  from dragonfly_amd import multiobjective_gpb_acquisitions as moo
  gps, weights, ref_point, Xh, t = _mirror_gps(0)
  wrapped = [_HostGP(gp) for gp in gps]
  anc = G.anc_data_for(_Box(G.DIM), 'lin', weights, ref_point, Xh, t, max_evals=64)
  if why == 'is_mf':
    anc.is_mf = True
    anc.eval_fidel_points_in_progress = []
  given = wrapped if why == 'host_gp' else [wrapped[0], gps[1]]
  np.random.seed(2)
  p_ucb = moo.mo_lin_asy_ucb(given, anc)
  p_ts = moo.mo_lin_asy_ts(given, anc)
  assert eng.calls == [] and wrapped[0].evals == 1 and wrapped[0].draws == 1
  assert p_ucb.shape == (G.DIM,) and p_ts.shape == (G.DIM,)
  with pytest.raises(NotImplementedError):          # other domains are the reference's business (install dispatches them)
    moo.mo_lin_asy_ucb(gps, G.anc_data_for(_Box(G.DIM, 'cartesian_product'), 'lin', weights, ref_point, Xh, t))


def test_namespaces_mirror_the_reference():
  from dragonfly_amd import multiobjective_gpb_acquisitions as moo
  for ns in (moo.asy, moo.seq):
    assert sorted(vars(ns)) == ['lin_ts', 'lin_ucb', 'tch_ts', 'tch_ucb']
  assert vars(moo.syn) == {}
  assert moo.asy.lin_ts is moo.mo_lin_asy_ts and moo.seq.tch_ucb is moo.mo_tch_asy_ucb


# ---- under the reference ------------------------------------------------------------------------------------------
def _reference():
  from oracle.make_golden import import_reference, REF
  if not os.path.isdir(REF):
    pytest.skip('no reference checkout at %s' % REF)
  import_reference()


def _moo_run(scal, acq, method, workers):
  """ a short multi-objective run of the reference's public API (opt/multiobjective_gp_bandit.py): two objectives on
      [0,1]^3; with two synthetic workers an evaluation is in progress whenever a point is chosen """
  from dragonfly.opt.multiobjective_gp_bandit import multiobjective_gpb_from_multi_func_caller, get_all_euc_moo_gp_bandit_args
  from dragonfly.exd.experiment_caller import EuclideanMultiFunctionCaller
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.exd.worker_manager import SyntheticWorkerManager
  from dragonfly.utils.option_handler import load_options
  f1 = lambda x: -float(np.sum((np.asarray(x) - 0.2) ** 2))
  f2 = lambda x: -float(np.sum((np.asarray(x) - 0.8) ** 2))
  caller = EuclideanMultiFunctionCaller([f1, f2], EuclideanDomain([[0, 1]] * 3), vectorised=False)
  opts = load_options(get_all_euc_moo_gp_bandit_args())
  opts.gpb_hp_tune_criterion = 'ml'
  opts.gpb_ml_hp_tune_opt = 'rand'
  opts.hp_tune_max_evals = 30
  opts.acq_opt_max_evals = 60
  opts.acq_opt_method = method
  opts.acq = acq
  opts.moors_scalarisation = 'tchebychev' if scal == 'tch' else 'linear'
  np.random.seed(11)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    _, _, history = multiobjective_gpb_from_multi_func_caller(
        caller, SyntheticWorkerManager(workers, time_distro='const'), 12, is_mf=False, options=opts, reporter='silent')
  return np.array(history.query_points)


@pytest.mark.parametrize('scal', ['lin', 'tch'])
@pytest.mark.parametrize('acq,method,workers', [('ucb', 'rand', 1), ('ucb', 'direct', 1), ('ts', 'rand', 2), ('ts', 'direct', 2)])
def test_install_with_the_flag_returns_the_reference_runs_points(scal, acq, method, workers, monkeypatch):
  _reference()
  from oracle_engine_moo import patch_engine_moo
  from dragonfly_amd import install
  want = _moo_run(scal, acq, method, workers)
  eng = patch_engine_moo(monkeypatch)
  install.install(multi_objective=True)
  try:
    got = _moo_run(scal, acq, method, workers)
  finally:
    install.uninstall()
  assert len(eng.calls) > 0 and {c[0] for c in eng.calls} == {'mo_ucb_argmax' if acq == 'ucb' else 'mo_thompson'}
  assert got.shape == want.shape and np.array_equal(got, want)


def test_install_flag_patches_the_four_names_and_uninstall_restores_them():
  _reference()
  from dragonfly_amd import install
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  before = {(ns, acq): getattr(getattr(ref_moo, ns), acq) for ns in ('asy', 'seq') for acq in ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb')}
  plain = install.install()
  try:
    assert all(getattr(getattr(ref_moo, ns), acq) is fn for (ns, acq), fn in before.items())
  finally:
    install.uninstall()
  flagged = install.install(multi_objective=True)
  try:
    # without the flag: the same list of names as before the flag existed; with it: those and the eight entries
    assert [n for n in flagged if n not in MOO_NAMES] == plain and sorted(n for n in flagged if n in MOO_NAMES) == sorted(MOO_NAMES)
    assert not any(n in MOO_NAMES for n in plain)
    from dragonfly_amd import multiobjective_gpb_acquisitions as moo
    for (ns, acq), fn in before.items():
      now = getattr(getattr(ref_moo, ns), acq)
      assert now is not fn and now.__wrapped__ is getattr(moo.asy, acq) and now.reference_callable is fn
  finally:
    install.uninstall()
  assert all(getattr(getattr(ref_moo, ns), acq) is fn for (ns, acq), fn in before.items())
