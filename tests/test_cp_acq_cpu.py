"""CPU plumbing of the fused acquisitions on Cartesian-product domains, install(cartesian_product=True,
cp_acquisitions=True), on the engine's CPU stand-in (tests/oracle_engine_cp_acq.py) with the real reference present
(skipped otherwise, like tests/test_cp_fitter_cpu.py):
 - the reference's CPGPBandit asks for the same points as it is and installed (tests/cp_acq_cases.py): 'rand' with UCB,
   EI, TTEI and Thompson sampling on a mixed domain, Thompson sampling with three workers (asynchronous with hallucinated
   evaluations in progress, and synchronous batches), and the tree search on an all-float product (the default 'direct', and 'pdoo');
 - an installed 'rand' step is ONE acq_argmax or ONE thompson_pointwise, with no posterior call per candidate;
 - the GA, kernels with an undescribed part, kernels not guaranteed PSD and multi-fidelity runs keep the reference's
   callable; without the flag install() rebinds what it always rebound; the flag alone is a ValueError;
 - the vectorised packing is kernel.pack row for row."""
import os
import warnings

from argparse import Namespace

import numpy as np
import pytest

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')), reason='the reference checkout is not present')


def _reference():
  from oracle.make_golden import import_reference
  import_reference()


def _installed(monkeypatch, **flags):
  from oracle_engine_cp_acq import patch_engine_cp_acq
  from dragonfly_amd import install
  eng = patch_engine_cp_acq(monkeypatch)
  return eng, install.install(cartesian_product=True, **flags)


_WANT = {}


def _reference_points(case):
  """ the unmodified reference's run of a case: computed once, shared """
  import cp_acq_cases as cases
  if case['id'] not in _WANT:
    _WANT[case['id']] = cases.run_case(case)
  return _WANT[case['id']]


def _case_ids():
  import cp_acq_cases as cases
  return [c['id'] for c in cases.CASES]


@pytest.mark.parametrize('case_id', _case_ids())
def test_reference_bandit_asks_for_the_same_points_installed(case_id, monkeypatch):
  _reference()
  import cp_acq_cases as cases
  from dragonfly_amd import install
  case = [c for c in cases.CASES if c['id'] == case_id][0]
  want = _reference_points(case)
  # (several workers: the 15 points of the initial design, then at least NUM_EVALS model-based evaluations)
  assert len(want) == cases.NUM_EVALS if case['workers'] == 1 else len(want) >= 15 + cases.NUM_EVALS
  eng, _ = _installed(monkeypatch, cp_acquisitions=True)
  try:
    got = cases.run_case(case)
  finally:
    install.uninstall()
  assert got == want
  calls = eng.calls
  if case['domain'] is cases.MIXED:
    fused = 'thompson_pointwise' if case['acq'] == 'ts' else 'acq_argmax'
    assert calls.get(fused, 0) >= cases.NUM_EVALS // 2 - 1       # every step after the initial points went through the fused call
    assert 'thompson' not in calls and 'predict_covar' not in calls
    assert calls.get('predict', 0) <= calls[fused]               # (TTEI's reference point: at most one per step)
    assert (calls.get('with_points_in_progress', 0) > 0) == (case['workers'] > 1)
  else:
    # the tree search asked for its centres a frontier at a time: far fewer posterior calls than boxes
    steps = cases.NUM_EVALS // 2
    assert 0 < calls.get('predict', 0) < steps * 60 / 4


def _fitted_bandit_gp(cases, case):
  """ the GP the reference's bandit fitted for its eighth ask on the mixed domain, through whatever is installed:
      (gp, processed domain, the labels so far) """
  opt = cases.fitted_bandit(case)
  return opt.gp, opt.domain, None, list(opt.gp.Y)


def _anc(domain, method, Y, **extra):
  anc = Namespace(domain=domain, acq_opt_method=method, max_evals=80, t=15, curr_max_val=max(Y), is_mf=False,
                  handle_parallel='halluc', eval_points_in_progress=[])
  for key, val in extra.items():
    setattr(anc, key, val)
  return anc


@pytest.mark.parametrize('acq', ['ucb', 'ei', 'pi', 'ts'])
def test_installed_rand_step_is_one_engine_call(acq, monkeypatch):
  """ counted by the stand-in's spy: the reference evaluates max_evals posteriors here, one per candidate """
  _reference()
  import cp_acq_cases as cases
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly_amd import install
  eng, _ = _installed(monkeypatch, cp_acquisitions=True)
  try:
    gp, domain, _, Y = _fitted_bandit_gp(cases, cases.CASES[0])
    eng.calls.clear()
    point = getattr(ref_acq.asy, acq)(gp, _anc(domain, 'rand', Y))
    fused = 'thompson_pointwise' if acq == 'ts' else 'acq_argmax'
    assert eng.calls == {fused: 1}
    assert domain.is_a_member(point)
    # the same step as the flag leaves it: one posterior call per candidate
    install.uninstall()
    install.install(cartesian_product=True)
    eng.calls.clear()
    getattr(ref_acq.asy, acq)(gp, _anc(domain, 'rand', Y))
    assert 'acq_argmax' not in eng.calls and 'thompson_pointwise' not in eng.calls
    assert sum(eng.calls.values()) >= 80
  finally:
    install.uninstall()


def test_fallbacks_take_the_reference_callable(monkeypatch):
  _reference()
  import cp_acq_cases as cases
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly_amd import install, gpb_acquisitions as A
  _installed(monkeypatch, cp_acquisitions=True)
  try:
    gp, domain, _, Y = _fitted_bandit_gp(cases, cases.CASES[0])
    dispatcher = ref_acq.asy.ucb
    # the dispatcher's two targets, replaced by markers for the length of the test
    closure = dict(zip(dispatcher.__code__.co_freevars, dispatcher.__closure__))
    theirs, ours = closure['theirs'].cell_contents, closure['ours'].cell_contents
    closure['theirs'].cell_contents = lambda *a, **k: 'theirs'
    closure['ours'].cell_contents = lambda *a, **k: 'ours'
    try:
      assert dispatcher(gp, _anc(domain, 'rand', Y)) == 'ours'
      assert dispatcher(gp, _anc(domain, 'pdoo', Y)) == 'theirs'                     # a mixed domain has no tree search
      # the GA, the default for mixed domains
      assert dispatcher(gp, _anc(domain, 'ga', Y)) == 'theirs'
      assert A.cp_acquisition_applies('ts', gp, _anc(domain, 'ga', Y))               # (TS always draws random candidates)
      # a multi-fidelity anc_data
      assert dispatcher(gp, _anc(domain, 'rand', Y, is_mf=True)) == 'theirs'
      # a kernel with a part the device does not describe: the GP runs in host-kernel mode
      with monkeypatch.context() as mp:
        mp.setattr(type(gp.kernel), 'has_device_spec', lambda self: False)
        assert gp._generic and dispatcher(gp, _anc(domain, 'rand', Y)) == 'theirs'   # pylint: disable=protected-access
      assert dispatcher(gp, _anc(domain, 'rand', Y)) == 'ours'
    finally:
      closure['theirs'].cell_contents, closure['ours'].cell_contents = theirs, ours
  finally:
    install.uninstall()


def test_kernel_not_guaranteed_psd_takes_the_reference_callable(monkeypatch):
  _reference()
  import cp_acq_cases as cases
  from dragonfly_amd import install, gpb_acquisitions as A
  _installed(monkeypatch, cp_acquisitions=True)
  try:
    gp, domain, _, Y = _fitted_bandit_gp(cases, cases.CASES[0])
    anc = _anc(domain, 'rand', Y)
    assert A.cp_acquisition_applies('ucb', gp, anc)
    monkeypatch.setattr(type(gp.kernel.kernel_list[-1]), 'is_guaranteed_psd', lambda self: False)
    assert not gp.kernel.is_guaranteed_psd()
    assert not A.cp_acquisition_applies('ucb', gp, anc) and not A.cp_acquisition_applies('ts', gp, anc)
    assert not A.cp_acquisition_applies('add_ucb', gp, anc)
  finally:
    install.uninstall()


def test_flag_off_rebinds_what_it_always_rebound(monkeypatch):
  _reference()
  import cp_acq_cases as cases
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly_amd import install
  eng, plain = _installed(monkeypatch)
  try:
    gp, domain, _, Y = _fitted_bandit_gp(cases, cases.CASES[0])
    eng.calls.clear()
    ref_acq.asy.ucb(gp, _anc(domain, 'rand', Y))
    assert 'acq_argmax' not in eng.calls and eng.calls.get('predict', 0) >= 80
  finally:
    install.uninstall()
  _, flagged = _installed(monkeypatch, cp_acquisitions=True)
  install.uninstall()
  assert flagged == plain


def test_flag_needs_cartesian_product():
  _reference()
  from dragonfly_amd import install
  with pytest.raises(ValueError):
    install.install(cp_acquisitions=True)
  assert install._saved == []                                # pylint: disable=protected-access


def test_vectorised_packing_is_pack_row_for_row(monkeypatch):
  from oracle_engine_cp_acq import patch_engine_cp_acq
  from dragonfly_amd import kernel as K
  patch_engine_cp_acq(monkeypatch)                            # (the kernels ask the engine which kinds it describes)
  rs = np.random.RandomState(12)
  def kern():
    return K.CartesianProductKernel(1.3, [K.SEKernel(2, 1.0, [0.4, 0.6]), K.MaternKernel(1, 2.5, 1.0, [2.0]),
                                          K.HammingKernel([0.5, 0.3, 0.2])])
  items = [['a', 'b', 'c', 'zz'], [0, 1, 2, 5], [1, 1.0, '1', 'b']]        # 1 == 1.0 share a code, '1' has its own
  def pts(n):
    return [[rs.random_sample(2), [int(rs.randint(1, 6))], [col[rs.randint(0, len(col))] for col in items]] for _ in range(n)]
  seen, X = pts(7), pts(50)
  one, many = kern(), kern()
  assert np.array_equal(one.pack(seen), many.pack(seen))     # (both coders have met some categories already)
  want = np.vstack([one.pack([x]) for x in X])               # a point at a time
  got = many.pack_many(X)
  assert got.shape == (50, 6) and np.array_equal(got, want)
  assert np.array_equal(many.pack_many(X), one.pack(X))      # and again, with every category known
  assert one.kernel_list[2].coder.columns == many.kernel_list[2].coder.columns
  with pytest.raises(ValueError):
    many.pack_many([[np.zeros(2), [1], ['a', 0, float('nan')]]])
  with pytest.raises(ValueError):
    many.pack_many([[np.zeros(2), [1], ['a', 0, ['unhashable']]]])
