"""CPU: BOCA's decision step (opt/gpb_acquisitions.py:313-439) through the mirror -- dragonfly_amd.gpb_acquisitions.boca,
FidelToOptGP, _add_ucb_for_boca and install(multi_fidelity=True, boca=True) -- against the unmodified reference, on the
NumPy stand-in of the engine (tests/oracle_engine_boca.py; there is no GPU here and no reference on the GPU machine).
What this pins is everything above the C-ABI: the decisions (fidelity, point), the random-number call order, the call
stream of the fused route.  The C-ABI side is pinned on the MI355X by tests/test_gpu_boca.py."""
import os
import warnings

from argparse import Namespace

import numpy as np
import pytest

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')),
                                reason='needs the reference tree (build container only)')

N, FD = 40, 1
GROUPS = [[0, 3], [1], [2, 4, 5]]


def _data(dd):
  rs = np.random.RandomState(40 + dd)
  ZZ, XX = rs.random_sample((N, FD)), rs.random_sample((N, dd))
  ZZ[::3] = 1.0                          # a third of the evaluations at fidel_to_opt itself, as in a real run
  YY = np.sin(3 * XX.sum(axis=1)) * (0.5 + ZZ[:, 0]) + 0.05 * rs.randn(N)
  return ZZ, XX, YY


def _mfgp(kmod, gp_cls, dd, additive):
  """ scale * SE(z) * Matern-2.5(x) (additive: a sum of Matern-2.5 groups over d = 6) with the classes of `kmod` """
  ZZ, XX, YY = _data(dd)
  dbw = 0.35 + 0.1 * np.arange(dd)
  fidel_kernel = kmod.SEKernel(FD, 1.0, np.array([0.6]))
  if additive:
    subs = [kmod.MaternKernel(len(g), 2.5, 1.0, dbw[g]) for g in GROUPS]
    domain_kernel = kmod.AdditiveKernel(1.3, subs, GROUPS)
  else:
    domain_kernel = kmod.MaternKernel(dd, 2.5, 1.0, dbw)
  mean_c = float(np.median(YY))
  return gp_cls(list(ZZ), list(XX), list(YY), None, 0.8, fidel_kernel, domain_kernel,
                lambda x, _c=mean_c: np.array([_c] * len(x)), 0.01)


def _caller(dd):
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.exd.experiment_caller import EuclideanFunctionCaller
  return EuclideanFunctionCaller(lambda z, x: 0.0, EuclideanDomain([[0, 1]] * dd), vectorised=False,
                                 raw_fidel_space=EuclideanDomain([[0, 1]] * FD),
                                 fidel_cost_func=lambda z: 0.2 + 0.8 * float(np.ravel(z)[0]),
                                 raw_fidel_to_opt=np.array([1.0] * FD))


def _anc(gp, acq, method, dd, in_progress):
  from dragonfly.exd.domains import EuclideanDomain
  bounds = np.array([[0.0, 1.0]] * dd)
  rs = np.random.RandomState(7)
  fidels = [rs.random_sample(FD) for _ in range(2)] if in_progress else []
  points = [rs.random_sample(dd) for _ in range(2)] if in_progress else []
  YY = _data(dd)[2]
  return Namespace(curr_acq=acq, max_evals=120, t=N, domain=EuclideanDomain(bounds), curr_max_val=float(YY.max()),
                   eval_points_in_progress=points, acq_opt_method=method, handle_parallel='halluc', mf_strategy='boca',
                   is_mf=True, domain_bounds=bounds, boca_thresh_coeff=0.01, boca_max_low_fidel_cost_ratio=0.9,
                   y_range=float(YY.max() - YY.min()), eval_fidels_in_progress=fidels,
                   eval_fidel_points_in_progress=gp.get_ZX_from_ZZ_XX(fidels, points))


def _decide(boca, asy, gp, acq, method, dd, in_progress, seed):
  np.random.seed(seed)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    fidel, point = boca(getattr(asy, acq), gp, _anc(gp, acq, method, dd, in_progress), _caller(dd))
  return np.asarray(fidel, dtype=float), np.asarray(point, dtype=float), np.random.get_state()


@pytest.mark.parametrize('method', ['rand', 'pdoo'])
@pytest.mark.parametrize('in_progress', [False, True], ids=['q0', 'q2'])
@pytest.mark.parametrize('acq', ['ucb', 'ei', 'pi', 'ttei', 'ts', 'add_ucb'])
def test_boca_decides_as_the_reference(acq, in_progress, method, monkeypatch):
  """ (a) one MF GP, n = 40, p = 1, d = 3 (add_ucb: d = 6, additive domain model), SE x Matern-2.5: the reference's boca
      and ours return the same (fidelity, point) and leave the global random state where the reference leaves it """
  from oracle.make_golden import import_reference
  import_reference()
  import dragonfly.gp.kernel as ref_kernel
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly.gp.euclidean_gp import EuclideanMFGP as RefMFGP
  from oracle_engine_boca import patch_engine_boca
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, mf_gp
  additive = acq == 'add_ucb'
  dd = 6 if additive else 3
  seed = 300 + 7 * ['ucb', 'ei', 'pi', 'ttei', 'ts', 'add_ucb'].index(acq)
  want = _decide(ref_acq.boca, ref_acq.asy, _mfgp(ref_kernel, RefMFGP, dd, additive), acq, method, dd, in_progress, seed)
  eng = patch_engine_boca(monkeypatch)
  ours = _mfgp(K, mf_gp.EuclideanMFGP, dd, additive)
  assert not ours._generic                      # pylint: disable=protected-access
  got = _decide(A.boca, A.asy, ours, acq, method, dd, in_progress, seed)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
  assert got[2][0] == want[2][0] and np.array_equal(got[2][1], want[2][1]) and got[2][2:] == want[2][2:]
  names = [c[0] for c in eng.calls]
  if additive:
    assert ('mf_add_ucb_all' if method == 'rand' else 'mf_add_ucb_group') in names
  elif method == 'rand' and not (acq == 'ts' and in_progress):
    # the fused route: candidates joined with the fidelity, the joint pairs in progress hallucinated by the fused call
    assert 'join_fixed' in names
    fused = [c for c in eng.calls if c[0] in ('acq_argmax', 'thompson')]
    assert fused and all(c[2][1] == FD + dd for c in fused if c[0] == 'acq_argmax')
    if acq != 'ts':
      assert all(c[3] == (2 if in_progress else 0) for c in fused)


def test_view_has_the_reference_namespace_attributes(monkeypatch):
  from oracle.make_golden import import_reference
  import_reference()
  from oracle_engine_boca import patch_engine_boca
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, mf_gp
  patch_engine_boca(monkeypatch)
  gp = _mfgp(K, mf_gp.EuclideanMFGP, 3, False)
  view = A._get_fidel_to_opt_gp(gp, np.array([1.0]))      # pylint: disable=protected-access
  for name in ('eval', 'eval_with_hallucinated_observations', 'draw_samples', 'draw_samples_with_hallucinated_observations'):
    assert callable(getattr(view, name))
  assert view.kernel is gp.get_domain_kernel() and view.mfgp is gp and view.is_fusable()
  x = list(np.random.RandomState(1).random_sample((5, 3)))
  mu, sd = view.eval(x, uncert_form='std')
  mu2, sd2 = gp.eval_at_fidel([np.array([1.0])] * 5, x, uncert_form='std')
  assert np.array_equal(mu, mu2) and np.array_equal(sd, sd2)
  with pytest.raises(NotImplementedError):
    A.syn_add_ucb_for_boca(2, [gp], np.array([1.0]), None)


def _mf_run(num_workers, acq, extra):
  """ tests/test_install_end_to_end.py's _mf_run with options: a short BOCA run of the reference, 1-D fidelity space """
  from dragonfly.opt import gp_bandit
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.exd.experiment_caller import EuclideanFunctionCaller
  from dragonfly.exd.worker_manager import SyntheticWorkerManager
  from dragonfly.utils.option_handler import load_options
  dd = extra.get('dim', 2)
  f = lambda z, x: -float(np.sum((np.asarray(x) - 0.3) ** 2)) - \
                   0.3 * (1 - float(np.ravel(z)[0])) * float(np.sin(5 * np.sum(x)))
  cost = lambda z: 0.2 + 0.8 * float(np.ravel(z)[0])
  caller = EuclideanFunctionCaller(f, EuclideanDomain([[0, 1]] * dd), vectorised=False,
                                   raw_fidel_space=EuclideanDomain([[0, 1]]), fidel_cost_func=cost,
                                   raw_fidel_to_opt=np.array([1.0]))
  opts = load_options(gp_bandit.get_all_mf_euc_gp_bandit_args())
  opts.gpb_hp_tune_criterion = 'ml'
  opts.gpb_ml_hp_tune_opt = 'rand'
  opts.hp_tune_max_evals = 30
  opts.acq_opt_max_evals = 100
  opts.acq_opt_method = 'rand'
  if acq is not None:
    opts.acq = acq
  for k, v in extra.items():
    if k != 'dim':
      assert hasattr(opts, k), k
      setattr(opts, k, v)
  np.random.seed(9)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    opt = gp_bandit.EuclideanGPBandit(caller, SyntheticWorkerManager(num_workers, time_distro='const'), is_mf=True,
                                      options=opts, reporter='silent')
    _, _, history = opt.optimise(8)
  return np.array(history.query_points), np.array(history.query_fidels), type(opt.gp).__module__


# The unmodified reference cannot run 'add_ucb' together with domain_use_additive_gp=True: its bandit then builds no
# add_gp_processor and _determine_next_query reads it (opt/gp_bandit.py:595-596, 653: AttributeError), so there is nothing
# to compare with.  'add_ucb-ucb' runs without the flag -- the bandit fits the additive multi-fidelity model itself
# (:603-609) and BOCA's add-UCB runs on it -- and the flag runs with 'ucb', where the additive GP goes through the view.
RUNS = [(1, None, {}), (3, 'ucb-ts', {}), (2, 'add_ucb-ucb', dict(dim=4)), (2, 'ucb', dict(domain_use_additive_gp=True, dim=4))]


@pytest.mark.parametrize('num_workers,acq,extra', RUNS,
                         ids=['w1-default', 'w3-ucb-ts', 'w2-add_ucb-ucb', 'w2-ucb-domain_use_additive_gp'])
def test_reference_multifidelity_runs_with_boca_installed(num_workers, acq, extra, monkeypatch):
  """ (b) the unmodified reference against install(multi_fidelity=True, boca=True) on the stand-in: the same query
      points and query fidelities, and the decisions did go through our boca """
  from oracle.make_golden import import_reference
  import_reference()
  from oracle_engine_boca import patch_engine_boca
  from dragonfly_amd import install
  want_pts, want_fidels, want_mod = _mf_run(num_workers, acq, extra)
  assert want_mod.startswith('dragonfly.')
  eng = patch_engine_boca(monkeypatch)
  install.install(multi_fidelity=True, boca=True)
  try:
    got_pts, got_fidels, got_mod = _mf_run(num_workers, acq, extra)
  finally:
    install.uninstall()
  assert got_mod.startswith('dragonfly_amd.')
  assert np.array_equal(got_pts, want_pts) and np.array_equal(got_fidels, want_fidels)
  names = set(c[0] for c in eng.calls)
  assert 'join_fixed' in names or 'mf_add_ucb_all' in names
  if acq is not None and 'add_ucb' in acq:
    assert 'mf_add_ucb_all' in names


def test_boca_flag_handling(monkeypatch):
  """ (c) boca=True only with multi_fidelity=True; without the flag the name stays the reference's; uninstall restores """
  from oracle.make_golden import import_reference
  import_reference()
  from oracle_engine_boca import patch_engine_boca
  from dragonfly_amd import install, gpb_acquisitions as A
  import dragonfly.opt.gpb_acquisitions as ref_acq
  patch_engine_boca(monkeypatch)
  ref_boca = ref_acq.boca
  with pytest.raises(ValueError):
    install.install(boca=True)
  assert ref_acq.boca is ref_boca and install._saved == []      # pylint: disable=protected-access
  install.install(multi_fidelity=True)
  try:
    assert ref_acq.boca is ref_boca
  finally:
    install.uninstall()
  patched = install.install(multi_fidelity=True, boca=True)
  try:
    assert 'dragonfly.opt.gpb_acquisitions.boca' in patched
    assert ref_acq.boca is not ref_boca and ref_acq.boca.__wrapped__ is A.boca and ref_acq.boca.reference_callable is ref_boca
  finally:
    install.uninstall()
  assert ref_acq.boca is ref_boca
