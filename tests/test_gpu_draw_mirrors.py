"""MI355X: the mirrors' joint draws on the fused route (dfh_gp_draw) -- GP.draw_samples with several samples,
GP.draw_samples_with_hallucinated_observations, and asy_ts with evaluations in progress -- against the reference's
arithmetic under the same seed, and against today's host route (the capability attribute masked)."""
from argparse import Namespace

import numpy as np
import pytest

from conftest import relerr

import draw_cases as D
import truth_bounds as tb

pytestmark = pytest.mark.gpu
M = 160


def _mirror(kind):
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean
  from dragonfly_amd.kernel import MaternKernel, SEKernel
  p = D.problem(kind)
  kernel = SEKernel(D.DIM, p['scale'], p['bw']) if kind == 'se' else MaternKernel(D.DIM, 2.5, p['scale'], p['bw'])
  return EuclideanGP(p['X'], p['Y'], kernel, ConstantMean(p['mean']), p['noise'])


def _state(state):
  return (state[0], state[1].tolist(), state[2], state[3], state[4])


@pytest.fixture
def no_covariance_on_the_host(monkeypatch):
  """ spy: the fused route never asks for the m x m covariance """
  from dragonfly_amd.engine import FittedGP
  calls = []
  original = FittedGP.predict_covar
  def spy(self, *args, **kwargs):
    calls.append(args[0].shape)
    return original(self, *args, **kwargs)
  monkeypatch.setattr(FittedGP, 'predict_covar', spy)
  return calls


@pytest.mark.parametrize('kind,S,q,seed', [('se', 3, 0, 11), ('m25', 2, 2, 12), ('se', 1, 2, 13)])
@pytest.mark.parametrize('device_normals', [True, False])
def test_draws_under_a_seed_equal_the_reference(kind, S, q, seed, device_normals, no_covariance_on_the_host, monkeypatch):
  from dragonfly_amd import gp_core
  monkeypatch.setattr(gp_core, 'DEVICE_NORMALS', device_normals)
  gp = _mirror(kind)
  rs = np.random.RandomState(200 + seed)
  Xs, Xh = rs.random_sample((M, D.DIM)), rs.random_sample((q, D.DIM))
  host = np.random.RandomState(seed)
  U = host.normal(size=(M, S))
  ref, _, truth = D.reference_draw(kind, Xs, Xh, U, M)
  np.random.seed(seed)
  got = gp.draw_samples_with_hallucinated_observations(S, list(Xs), list(Xh)) if q else gp.draw_samples(S, list(Xs))
  after = np.random.get_state()
  bound = tb.bound(ref, truth)
  print(kind, S, q, 'relerr', relerr(got, ref), 'bound', bound)
  assert got.shape == (S, M) and relerr(got, ref) <= bound
  assert _state(after) == _state(host.get_state())
  assert no_covariance_on_the_host == []
  if S > 1 or q:      # today's route, for the same seed: the covariance comes to the host, the draw is the same
    monkeypatch.setattr(type(gp.device_gp), 'fused_draws', False)
    np.random.seed(seed)
    old = gp.draw_samples_with_hallucinated_observations(S, list(Xs), list(Xh)) if q else gp.draw_samples(S, list(Xs))
    print('the host route: relerr', relerr(old, ref))
    assert no_covariance_on_the_host == [(M, D.DIM)] and old.shape == got.shape
    assert _state(np.random.get_state()) == _state(after)


@pytest.mark.parametrize('device_candidates', [True, False])
def test_asy_ts_with_points_in_progress_returns_todays_point(device_candidates, no_covariance_on_the_host, monkeypatch):
  from dragonfly_amd import gpb_acquisitions as A
  from dragonfly_amd.oper_utils import EuclideanDomain
  monkeypatch.setattr(A, 'DEVICE_CANDIDATES', device_candidates)
  gp = _mirror('se')
  domain = EuclideanDomain([[0, 1]] * D.DIM)
  pending = [np.array([0.3, 0.6, 0.2]), np.array([0.8, 0.1, 0.5])]
  mk_anc = lambda: Namespace(max_evals=300, t=D.N, domain=domain, domain_bounds=domain.bounds, acq_opt_method='rand',
                             curr_max_val=float(D.problem('se')['Y'].max()), handle_parallel='halluc',
                             eval_points_in_progress=list(pending), is_mf=False)
  np.random.seed(77)
  fused = np.asarray(A.asy_ts(gp, mk_anc()), dtype=float)
  fused_state = np.random.get_state()
  assert no_covariance_on_the_host == []
  monkeypatch.setattr(type(gp.device_gp), 'fused_draws', False)
  np.random.seed(77)
  today = np.asarray(A.asy_ts(gp, mk_anc()), dtype=float)
  assert no_covariance_on_the_host == [(300, D.DIM)]
  assert np.array_equal(fused, today)
  assert _state(fused_state) == _state(np.random.get_state())
  # the synchronous batch is the asynchronous rule worker by worker: the second worker sees the first one's point
  monkeypatch.setattr(type(gp.device_gp), 'fused_draws', True)
  del no_covariance_on_the_host[:]
  np.random.seed(78)
  batch = A.syn_ts(2, gp, mk_anc())
  assert len(batch) == 2 and no_covariance_on_the_host == []
