"""CPU: the joint-draw exports (dfh_gp_draw, dfh_mgpu_ts_halluc, dfh_mgpu_acq_argmax_halluc) are in the header, the built
library and the ctypes table, argument for argument; and the mirrors choose the fused route by the fitted handle's
capability attribute alone -- shown with a recording handle over the NumPy stand-in engine (tests/oracle_engine.py),
which has no such attribute and keeps today's route."""
import os
import re
import shutil
import subprocess
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT
from oracle import ref_numpy as O

import draw_cases as D

NEW_EXPORTS = ('dfh_gp_draw', 'dfh_mgpu_ts_halluc', 'dfh_mgpu_acq_argmax_halluc')


def _declaration(name):
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfhip.h')).read(), flags=re.S)
  found = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, text)
  assert found, '%s is not declared in include/dfhip.h' % name
  return [a for a in found.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', NEW_EXPORTS)
def test_export_is_in_header_library_and_table(name):
  from dragonfly_amd import _lib
  args = _declaration(name)
  nm = shutil.which('nm') or '/opt/rocm/lib/llvm/bin/llvm-nm'
  out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
  assert re.search(r'\bT %s\b' % name, out), '%s is not exported by the built library' % name
  restype, argtypes = _lib.SIGNATURES[name]
  assert len(argtypes) == len(args), (name, len(argtypes), len(args))
  assert _lib.load().dfh_abi_version() == 2


def test_the_capability_is_an_attribute_of_the_handle_class():
  from dragonfly_amd.engine import FittedGP
  from oracle_engine import OracleFittedGP
  assert FittedGP.fused_draws is True and not hasattr(OracleFittedGP, 'fused_draws')


class Recording(object):
  """ a fitted handle that records what it is asked and answers with the stand-in's arithmetic """

  def __init__(self, inner, capable):
    self.inner, self.engine, self.calls = inner, inner.engine, []
    if capable:
      self.fused_draws = True

  def __getattr__(self, name):
    target = getattr(self.inner, name)
    if not callable(target):
      return target
    def recorded(*args, **kwargs):
      self.calls.append((name, args, kwargs))
      return target(*args, **kwargs)
    return recorded

  def _joint(self, Xs, U, X_halluc, shift):
    og = self.inner.oracle
    mu, cov = og.eval_with_hallucinated_observations(Xs, X_halluc, 'covar') if X_halluc is not None and len(X_halluc) else og.eval(Xs, 'covar')
    return O.draw_gaussian_samples_with_normals(mu + shift, cov, U)

  def thompson(self, Xs, U, block=4096, mean_const=0.0, mean_vals=None, return_samples=False, X_halluc=None):
    self.calls.append(('thompson', (Xs, U), dict(block=block, X_halluc=X_halluc)))
    samples = self._joint(Xs, np.asarray(U).reshape(-1, 1), X_halluc, mean_const if mean_vals is None else np.asarray(mean_vals))[0]
    best_val, best_idx = O.argmax_first(samples)
    return (best_val, best_idx, samples, [None]) if return_samples else (best_val, best_idx)

  def draw(self, Xs, U, num_samples=1, block=None, X_halluc=None, mean_const=0.0, mean_vals=None, return_samples=True):
    self.calls.append(('draw', (Xs, U), dict(num_samples=num_samples, block=block, X_halluc=X_halluc)))
    samples = self._joint(Xs, np.asarray(U).reshape(len(Xs), num_samples), X_halluc, mean_const if mean_vals is None else np.asarray(mean_vals))
    return samples, samples.max(axis=1), samples.argmax(axis=1), [None]


def _mirror(monkeypatch, capable):
  from oracle_engine import patch_engine
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean
  from dragonfly_amd.kernel import SEKernel
  patch_engine(monkeypatch)
  p = D.problem('se')
  gp = EuclideanGP(p['X'], p['Y'], SEKernel(D.DIM, p['scale'], p['bw']), ConstantMean(p['mean']), p['noise'])
  gp._fitted = Recording(gp._fitted, capable)      # pylint: disable=protected-access
  return gp, gp._fitted                            # pylint: disable=protected-access


PENDING = [np.array([0.3, 0.6, 0.2]), np.array([0.8, 0.1, 0.5])]
EVALS = 300


def _anc():
  from dragonfly_amd.oper_utils import EuclideanDomain
  domain = EuclideanDomain([[0, 1]] * D.DIM)
  return Namespace(max_evals=EVALS, t=D.N, domain=domain, domain_bounds=domain.bounds, acq_opt_method='rand', curr_max_val=1.0,
                   handle_parallel='halluc', eval_points_in_progress=list(PENDING), is_mf=False)


def _state(state):
  return (state[0], state[1].tolist(), state[2], state[3], state[4])


def _reference_sequence(seed, m, S):
  """ the reference's np.random calls: the candidates (oper_utils.py:61-62), then the normals (general_utils.py:230) """
  host = np.random.RandomState(seed)
  cands = host.random_sample((m, D.DIM))
  return host, cands, host.normal(size=(m, S))


def test_asy_ts_hands_the_points_in_progress_to_a_capable_handle(monkeypatch):
  from dragonfly_amd import gpb_acquisitions as A
  gp, rec = _mirror(monkeypatch, capable=True)
  host, cands, normals = _reference_sequence(5, EVALS, 1)
  np.random.seed(5)
  point = A.asy_ts(gp, _anc())
  assert [c[0] for c in rec.calls] == ['thompson']          # one fused call, no posterior covariance on the host
  _, (Xs, U), kw = rec.calls[0]
  assert np.array_equal(kw['X_halluc'], np.array(PENDING)) and kw['block'] == EVALS
  assert np.array_equal(Xs, cands)                          # candidates first ...
  assert U.shape == (EVALS,) and np.array_equal(U, normals.ravel())      # ... then the normals
  assert _state(np.random.get_state()) == _state(host.get_state())
  # today's route from the same seed picks the same point
  plain_gp, plain = _mirror(monkeypatch, capable=False)
  np.random.seed(5)
  assert np.array_equal(point, A.asy_ts(plain_gp, _anc()))
  assert _state(np.random.get_state()) == _state(host.get_state())
  assert [c[0] for c in plain.calls] == ['predict', 'predict_covar']


def test_without_the_capability_nothing_but_todays_calls_is_made(monkeypatch):
  from dragonfly_amd import gpb_acquisitions as A
  gp, rec = _mirror(monkeypatch, capable=False)
  rs = np.random.RandomState(2)
  Xs = list(rs.random_sample((40, D.DIM)))
  np.random.seed(6)
  A.asy_ts(gp, _anc())
  gp.draw_samples_with_hallucinated_observations(2, Xs, PENDING)
  gp.draw_samples(3, Xs)
  gp.draw_samples(1, Xs)
  assert [c[0] for c in rec.calls] == ['predict', 'predict_covar', 'predict', 'predict_covar', 'predict_covar', 'thompson']
  assert rec.calls[-1][2] == dict(block=40, X_halluc=None)      # the single draw's call, without the new keyword
  # no points in progress: the fused Thompson step of today, called without the new keyword
  anc = _anc()
  anc.eval_points_in_progress = []
  del rec.calls[:]
  A.asy_ts(gp, anc)
  assert [c[0] for c in rec.calls] == ['thompson'] and rec.calls[0][2]['X_halluc'] is None


@pytest.mark.parametrize('S,q', [(3, 0), (2, 2), (1, 2)])
def test_gp_draws_go_through_one_call_of_a_capable_handle(S, q, monkeypatch):
  gp, rec = _mirror(monkeypatch, capable=True)
  rs = np.random.RandomState(3)
  m = 40
  Xs = rs.random_sample((m, D.DIM))
  host = np.random.RandomState(9)
  normals = host.normal(size=(m, S))
  np.random.seed(9)
  got = gp.draw_samples_with_hallucinated_observations(S, list(Xs), PENDING[:q]) if q else gp.draw_samples(S, list(Xs))
  assert [c[0] for c in rec.calls] == ['draw']
  _, (Xt, U), kw = rec.calls[0]
  assert kw['num_samples'] == S and kw['block'] is None and np.array_equal(Xt, Xs)
  assert (kw['X_halluc'] is None) if not q else np.array_equal(kw['X_halluc'], np.array(PENDING[:q]))
  assert np.shape(U) == (m, S) and np.array_equal(U, normals)
  assert _state(np.random.get_state()) == _state(host.get_state())
  # the values are the reference's (gp_core.py:250-261) for those normals
  og = D.oracle_gp('se')
  mu, cov = og.eval_with_hallucinated_observations(Xs, np.array(PENDING[:q]), 'covar') if q else og.eval(Xs, 'covar')
  want = O.draw_gaussian_samples_with_normals(mu, cov, normals)
  assert got.shape == (S, m) and np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
