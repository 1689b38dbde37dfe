"""CPU plumbing of the fused multi-objective acquisitions on Cartesian-product domains, install(multi_objective=True,
cartesian_product=True, cp_acquisitions=True), on the engine's CPU stand-in (tests/oracle_engine_mo_cp.py) with the real
reference present (skipped otherwise, like tests/test_cp_acq_cpu.py):
 - the reference's CPMultiObjectiveGPBandit asks for the same points as it is and installed (tests/mo_cp_cases.py): both
   scalarisations; 'ucb', 'ts' and the default 'ucb-ts'; 'rand' and the default GA on a mixed domain; three workers with
   hallucinated evaluations in progress; 'pdoo' on an all-float product;
 - an installed Thompson step is ONE mo_thompson_pointwise, an installed 'rand' UCB step ONE mo_ucb_argmax, and under the
   GA one mo_ucb_argmax per evaluated point, with no per-objective posterior call;
 - a host-kernel GP among the objectives, a kernel not guaranteed PSD, nine objectives, GPs on two engines keep the
   reference's callable, and objectives whose packed candidates differ take the per-point closures: the same points;
 - without one of the three flags install() rebinds what it rebound and a product-domain call reaches the reference's
   callable; uninstall() restores everything; the module's own maximise_acquisition forwards product domains."""
import os
from argparse import Namespace
from copy import deepcopy

import numpy as np
import pytest

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')), reason='the reference checkout is not present')
FLAGS = dict(multi_objective=True, cartesian_product=True, cp_acquisitions=True)
ACQS = ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb')


def _reference():
  from oracle.make_golden import import_reference
  import_reference()


def _installed(monkeypatch, **flags):
  from oracle_engine_mo_cp import patch_engine_mo_cp
  from dragonfly_amd import install
  eng = patch_engine_mo_cp(monkeypatch)
  return eng, install.install(**flags)


_WANT = {}


def _reference_points(case):
  """ the unmodified reference's run of a case: computed once, shared """
  import mo_cp_cases as cases
  if case['id'] not in _WANT:
    _WANT[case['id']] = cases.run_case(case)
  return _WANT[case['id']]


def _case_ids():
  import mo_cp_cases as cases
  return [c['id'] for c in cases.CASES]


@pytest.mark.parametrize('case_id', _case_ids())
def test_reference_bandit_asks_for_the_same_points_installed(case_id, monkeypatch):
  _reference()
  import mo_cp_cases as cases
  from dragonfly_amd import install
  case = [c for c in cases.CASES if c['id'] == case_id][0]
  want = _reference_points(case)
  assert len(want) >= 15 + cases.NUM_STEPS
  eng, _ = _installed(monkeypatch, **FLAGS)
  try:
    got = cases.run_case(case)
  finally:
    install.uninstall()
  assert got == want
  calls = eng.calls
  fused = calls.get('mo_thompson_pointwise', 0) + calls.get('mo_ucb_argmax', 0)
  assert fused >= cases.NUM_STEPS - 1                    # every step after the initial points went through a fused call
  assert 'thompson_pointwise' not in calls and 'thompson' not in calls and 'predict_covar' not in calls
  if case['acq'] == 'ts':
    assert 'mo_ucb_argmax' not in calls and 'predict' not in calls
  if case['acq'] == 'ucb':
    assert 'mo_thompson_pointwise' not in calls
  if case['acq'] == 'default':
    assert calls.get('mo_thompson_pointwise', 0) > 0 and calls.get('mo_ucb_argmax', 0) > 0      # 'ucb-ts'
  if case['workers'] > 1:
    assert calls.get('with_points_in_progress', 0) > 0


def _fitted(cases, case=None):
  """ (the GPs the reference's bandit fitted last, through whatever is installed; the processed domain) """
  opt = cases.fitted_bandit(case or cases.CASES[0])
  return list(opt.gps), opt.domain


def _anc(domain, method, k=2, **extra):
  anc = Namespace(domain=domain, acq_opt_method=method, max_evals=40, t=20, is_mf=False, handle_parallel='halluc',
                  eval_points_in_progress=[], obj_weights=list(np.linspace(0.6, 0.4, k) / k * 2), reference_point=[-3.0] * k)
  for key, val in extra.items():
    setattr(anc, key, val)
  return anc


@pytest.mark.parametrize('acq', ACQS)
@pytest.mark.parametrize('method', ['rand', 'ga'])
def test_installed_step_call_counts(acq, method, monkeypatch):
  """ counted by the stand-in's spy: the reference makes one posterior or draw per objective and candidate here """
  _reference()
  import mo_cp_cases as cases
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  from dragonfly_amd import install
  eng, _ = _installed(monkeypatch, **FLAGS)
  try:
    gps, domain = _fitted(cases)
    eng.calls.clear()
    np.random.seed(3)
    point = getattr(ref_moo.asy, acq)(gps, _anc(domain, method))
    fused = dict(eng.calls)
    assert domain.is_a_member(point)
    # the same step as two of the flags leave it: the reference's callable, one call per objective and point
    install.uninstall()
    install.install(multi_objective=True, cartesian_product=True)
    eng.calls.clear()
    np.random.seed(3)
    want = getattr(ref_moo.asy, acq)(gps, _anc(domain, method))
    plain = dict(eng.calls)
  finally:
    install.uninstall()
  assert repr(point) == repr(want)
  assert not any(name.startswith('mo_') for name in plain)
  if acq.endswith('_ts'):
    assert fused == {'mo_thompson_pointwise': 1}
    assert sum(plain.values()) >= 2 * (40 if method == 'rand' else 160)       # (the GA: four times the candidates)
  elif method == 'rand':
    assert fused == {'mo_ucb_argmax': 1}
    assert plain.get('predict', 0) >= 2 * 40
  else:
    # the GA asks point by point: one device call per point instead of one gp.eval per objective and point
    assert set(fused) == {'mo_ucb_argmax'} and 2 * fused['mo_ucb_argmax'] == plain['predict']


def _swap_targets(dispatcher):
  """ the dispatcher's two targets replaced by markers; returns the function that puts them back """
  closure = dict(zip(dispatcher.__code__.co_freevars, dispatcher.__closure__))
  theirs, ours = closure['theirs'].cell_contents, closure['ours'].cell_contents
  closure['theirs'].cell_contents = lambda *a, **k: 'theirs'
  closure['ours'].cell_contents = lambda *a, **k: 'ours'
  def restore():
    closure['theirs'].cell_contents, closure['ours'].cell_contents = theirs, ours
  return restore


def test_fallbacks_take_the_reference_callable(monkeypatch):
  _reference()
  import mo_cp_cases as cases
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  from dragonfly_amd import install, multiobjective_gpb_acquisitions as MO
  eng, _ = _installed(monkeypatch, **FLAGS)
  try:
    gps, domain = _fitted(cases)
    for acq in ACQS:
      dispatcher = getattr(ref_moo.asy, acq)
      restore = _swap_targets(dispatcher)
      try:
        for method in ('rand', 'ga', 'pdoo'):              # (a mixed domain has no tree search: Dragonfly's own maximiser)
          assert dispatcher(gps, _anc(domain, method)) == 'ours'
        assert dispatcher(gps, _anc(domain, 'rand', is_mf=True)) == 'theirs'
        # a host-kernel GP among the objectives
        with monkeypatch.context() as mp:
          mp.setattr(gps[1].kernel, 'has_device_spec', lambda: False, raising=False)
          assert gps[1]._generic and not gps[0]._generic                              # pylint: disable=protected-access
          assert dispatcher(gps, _anc(domain, 'rand')) == 'theirs'
        # a kernel not guaranteed PSD
        with monkeypatch.context() as mp:
          mp.setattr(gps[0].kernel.kernel_list[-1], 'is_guaranteed_psd', lambda: False, raising=False)
          assert not gps[0].kernel.is_guaranteed_psd() and gps[1].kernel.is_guaranteed_psd()
          assert dispatcher(gps, _anc(domain, 'rand')) == 'theirs'
        # nine objectives
        assert dispatcher((gps * 5)[:8], _anc(domain, 'rand', k=8)) == 'ours'
        assert dispatcher((gps * 5)[:9], _anc(domain, 'rand', k=9)) == 'theirs'
        # GPs on two engines
        with monkeypatch.context() as mp:
          mp.setattr(gps[1].device_gp, 'engine', object(), raising=False)
          assert dispatcher(gps, _anc(domain, 'rand')) == 'theirs'
        assert dispatcher(gps, _anc(domain, 'rand')) == 'ours'
      finally:
        restore()
    # nine objectives for real: the reference's callable, no fused call, the point it returns by itself
    nine = (gps * 5)[:9]
    eng.calls.clear()
    np.random.seed(5)
    got = ref_moo.asy.lin_ts(nine, _anc(domain, 'rand', k=9))
    assert not any(name.startswith('mo_') for name in eng.calls)
    np.random.seed(5)
    assert repr(got) == repr(ref_moo.asy.lin_ts.reference_callable(nine, _anc(domain, 'rand', k=9)))
    assert not MO.mo_cp_acquisition_applies('lin_ts', nine, _anc(domain, 'rand', k=9))
    assert not MO.mo_cp_acquisition_applies('lin_ei', gps, _anc(domain, 'rand'))
  finally:
    install.uninstall()


@pytest.mark.parametrize('acq', ACQS)
def test_objectives_packed_differently_take_the_per_point_closures(acq, monkeypatch):
  """ two GPs built from differently ordered training lists give a category different codes: no objective is handed rows
      coded by the other's dictionary, and the step returns the reference callable's point """
  _reference()
  import mo_cp_cases as cases
  import dragonfly.gp.cartesian_product_gp as ref_cpgp
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  from dragonfly_amd import install, kernel as K, multiobjective_gpb_acquisitions as MO
  eng, _ = _installed(monkeypatch, **FLAGS)
  try:
    gps, domain = _fitted(cases)
    kern = deepcopy(gps[1].kernel)
    for part in kern.kernel_list:
      if isinstance(part, K.HammingKernel):
        part.coder = K.CategoryCoder()
    order = sorted(range(len(gps[1].X)), key=lambda i: repr(gps[1].X[i][-1]), reverse=True)
    other = ref_cpgp.CPGP([gps[1].X[i] for i in order], [gps[1].Y[i] for i in order], kern, gps[1].mean_func, gps[1].noise_var,
                          handle_non_psd_kernels='project_first')
    pair = [gps[0], other]
    probe = [gps[0].X[i] for i in range(len(gps[0].X))]
    assert not np.array_equal(gps[0].kernel.pack_many(probe), other.kernel.pack_many(probe))
    anc = _anc(domain, 'rand')
    assert MO.mo_cp_acquisition_applies(acq, pair, anc)
    eng.calls.clear()
    np.random.seed(5)
    got = getattr(ref_moo.asy, acq)(pair, anc)
    assert not any(name.startswith('mo_') for name in eng.calls) and sum(eng.calls.values()) >= 2 * 40
    np.random.seed(5)
    want = getattr(ref_moo.asy, acq).reference_callable(pair, _anc(domain, 'rand'))
    assert repr(got) == repr(want)
  finally:
    install.uninstall()


def test_rebound_names_and_uninstall(monkeypatch):
  _reference()
  import mo_cp_cases as cases
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo
  from dragonfly_amd import install
  before = {ns: {acq: getattr(getattr(ref_moo, ns), acq) for acq in ACQS} for ns in ('asy', 'seq')}
  before_maximise = ref_moo.maximise_acquisition
  _, flagged = _installed(monkeypatch, **FLAGS)
  install.uninstall()
  eng, two = _installed(monkeypatch, multi_objective=True, cartesian_product=True)
  try:
    assert two == flagged
    gps, domain = _fitted(cases)
    for acq in ACQS:
      restore = _swap_targets(getattr(ref_moo.asy, acq))
      try:
        assert getattr(ref_moo.asy, acq)(gps, _anc(domain, 'rand')) == 'theirs'
      finally:
        restore()
  finally:
    install.uninstall()
  # without multi_objective the four names are not rebound at all, with or without the other two
  _, no_mo_flagged = _installed(monkeypatch, cartesian_product=True, cp_acquisitions=True)
  try:
    assert all(getattr(getattr(ref_moo, ns), acq) is before[ns][acq] for ns in before for acq in ACQS)
  finally:
    install.uninstall()
  _, no_mo = _installed(monkeypatch, cartesian_product=True)
  install.uninstall()
  assert no_mo_flagged == no_mo and not any('multiobjective_gpb_acquisitions.asy' in name for name in no_mo)
  with pytest.raises(ValueError):
    install.install(multi_objective=True, cp_acquisitions=True)
  assert install._saved == []                                # pylint: disable=protected-access
  assert all(getattr(getattr(ref_moo, ns), acq) is before[ns][acq] for ns in before for acq in ACQS)
  assert ref_moo.maximise_acquisition is before_maximise


def test_module_maximise_acquisition_forwards_product_domains(monkeypatch):
  from dragonfly_amd import multiobjective_gpb_acquisitions as MO
  monkeypatch.setattr(MO, '_maximise_acquisition', lambda acq_fn, anc_data, *a, **k: ('forwarded', anc_data.domain.get_type(), k))
  domain = lambda kind: Namespace(get_type=lambda: kind)
  assert MO.maximise_acquisition(None, Namespace(domain=domain('cartesian_product')), vectorised=True) == \
         ('forwarded', 'cartesian_product', {'vectorised': True})
  assert MO.maximise_acquisition(None, Namespace(domain=domain('euclidean')))[1] == 'euclidean'
  for kind in ('neural_network', 'integral'):
    with pytest.raises(NotImplementedError):
      MO.maximise_acquisition(None, Namespace(domain=domain(kind)))
