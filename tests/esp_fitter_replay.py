"""The stand-alone EuclideanGPFitter with kernel_type='esp' on the cases of tests/golden/esp_fitter_d4_n30.npz
(tools/make_esp_golden.py: the reference's fitter, same options, same seed), and the comparison with what the
reference chose.  Shared by tests/test_esp_fitter_cpu.py (CPU stand-in of the engine) and tests/test_gpu_esp.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tools'))
from make_esp_golden import FITTER_CASES, FITTER_SEED, fitter_options, fitter_record   # noqa: E402

CASE_NAMES = [name for name, _ in FITTER_CASES]


def run_case(name, X, Y):
  from dragonfly_amd.euclidean_gp import EuclideanGPFitter
  opts = dict(FITTER_CASES)[name]
  np.random.seed(FITTER_SEED)
  fitter = EuclideanGPFitter(list(X), list(Y), options=fitter_options(opts))
  kind, gp, hps = fitter.fit_gp()
  return fitter_record(kind, gp, hps)


def check_case(name, g, lml_tol):
  got = run_case(name, g['X'], g['Y'])
  want = {k.split('__', 1)[1]: v for k, v in g.items() if k.startswith(name + '__')}
  assert str(got['kind']) == str(want['kind']), (name, got['kind'], want['kind'])
  assert got['order'] == int(want['order']) and got['nu'] == float(want['nu']), (name, got['order'], got['nu'])
  assert np.array_equal(got['dscr'], want['dscr']), (name, got['dscr'], want['dscr'])
  assert np.array_equal(got['cts'], want['cts']), (name, got['cts'], want['cts'])
  assert got['scale'] == float(want['scale']) and got['noise'] == float(want['noise'])
  assert np.array_equal(got['bws'], want['bws'])
  assert abs(got['lml'] - float(want['lml'])) <= lml_tol * abs(float(want['lml'])), (name, got['lml'], want['lml'])
