"""MI355X: the block-inverse triangular solves of csrc/trsolve.hip, element by element through Engine.solve_triangular,
each case held by Engine.solve_launches() to the kernels it was written for (tests/trsolve_cases.py has the tables, the
references and the reasons for every size; tests/test_trsolve_cases_cpu.py the conditions these assertions rest on).

  few-row form    2 <= nrhs <= 256 forward: gemm_skinny_kernel<MT, SPLIT> for the block solve and the update, with its
                  fall-backs (odd n, n % 4 == 2, a last block that is no multiple of 64); all eight instantiations over
                  the table; a column's bits do not depend on the batch it is solved in
  wide form       nrhs > 256 forward
  backward        L^T X = B for any nrhs >= 2
  single vector   the four kernels of their own with both update variants each at even sizes, the general route at odd
  refinement      hard factors, whose 512-block inverses need 2 or 3 steps: the backward error of the device against
                  scipy's on the same problem, at most BACKWARD_ERROR_FACTOR times as large (an unrefined solve is at
                  least ten times further out: the CPU test); the measured table is written beside the
                  conditioning sweep's, as trsolve_backward_error.txt (committed copy: profiles/)
  forced steps    DFH_REFINE_FORCE_STEPS = 1, 2, 3 in a child process each (tests/trsolve_forced_check.py): every copy of
                  the refinement step on good factors, and the call sites at the GP level against the oracle

Easy factors are held to 1e-11 (conftest.relerr) against scipy.linalg.solve_triangular and to
|fl(A X) - B| <= 2 gamma_n (|A||X| + |B|)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import trsolve_cases as T
from conftest import ROOT
from test_gpu_conditioning import REPORT as SWEEP_REPORT

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(SWEEP_REPORT), 'trsolve_backward_error.txt')


def _run(engine, L, B, upper):
  X, got = T.booked(engine, lambda: engine.solve_triangular(L, B, upper=upper))
  return X, got


def _easy_case(engine, n, nrhs, upper, ncols):
  """ one easy case: the counters it was written for, then the two assertions; returns (X, the counters' difference) """
  L, B, Xref = T.easy_problem(n, upper, ncols)
  Bk = T.columns(B, nrhs)
  X, got = _run(engine, L, Bk, upper)
  what = 'n %d nrhs %d upper %d' % (n, nrhs, upper)
  assert T.families(got) == T.expected_launches(n, nrhs, upper), (what, got)
  T.check_easy(L, X, Bk, T.columns(Xref, nrhs), upper, what)
  return X, got


@pytest.fixture(scope='module')
def few_row(engine):
  """ run(n, nrhs): a few-row case solved and checked once, whichever test asks first """
  done = {}

  def run(n, nrhs):
    if (n, nrhs) not in done:
      done[(n, nrhs)] = _easy_case(engine, n, nrhs, False, T.FEW_ROWS)
    return done[(n, nrhs)]
  return run


@pytest.mark.parametrize('n,nrhs', T.FEW_ROW_CASES)
def test_few_row_forward(few_row, n, nrhs):
  few_row(n, nrhs)


def test_few_row_table_books_all_eight_instantiations(engine, few_row):
  """ which of the split and unsplit kernels a product takes depends on the device's CU count, so the per-case
      expectation is the MT; over the table every instantiation must have run """
  seen = dict.fromkeys(T.SKINNY, 0)
  for n, nrhs in T.FEW_ROW_CASES:
    got = few_row(n, nrhs)[1]
    for k in T.SKINNY:
      seen[k] += got[k]
  print(seen)
  assert all(seen.values()), seen


def test_few_row_column_bits_do_not_depend_on_the_batch(few_row):
  """ the few-row kernel's documented property (gemm_f64.hip): a row's result depends on K and on nothing else, whichever
      MT it is computed by -- column j of the solution is the same for 2, 17 and 256 right-hand sides """
  n = T.BITS_N
  big = few_row(n, max(T.BITS_NRHS))[0]
  for k in T.BITS_NRHS:
    X = few_row(n, k)[0]
    same = X.view(np.int64) == np.ascontiguousarray(big[:, :k]).view(np.int64)
    assert same.all(), (k, tuple(int(v) for v in np.argwhere(~same)[0]))


@pytest.mark.parametrize('n,nrhs', T.WIDE_CASES)
def test_wide_forward(engine, n, nrhs):
  _easy_case(engine, n, nrhs, False, 640)


@pytest.mark.parametrize('n,nrhs', T.BACKWARD_CASES)
def test_backward(engine, n, nrhs):
  _easy_case(engine, n, nrhs, True, 300)


@pytest.mark.parametrize('n', T.VECTOR_CASES)
def test_single_vector(engine, n):
  """ even sizes: the kernels of their own, and exactly the update variants the size was chosen for; odd: the general
      route and none of them """
  for upper in (False, True):
    _, got = _easy_case(engine, n, 1, upper, 1)
    if n % 2:
      assert got['trsv_general_blocks'] == T.nblocks(n) and not any(got[k] for k in T.FAST_VECTOR), got
    else:
      assert got['trsv_general_blocks'] == 0


@pytest.fixture(scope='module')
def report():
  os.makedirs(os.path.dirname(REPORT), exist_ok=True)
  with open(REPORT, 'w') as f:
    f.write('Backward error of the refined block-inverse solves on hard factors (tests/test_gpu_trsolve.py):\n'
            'ratio = max(|A X - B| / (|A||X| + |B|)), device and scipy.linalg.solve_triangular on the same problem;\n'
            'the test allows device / scipy <= %.1f.\n'
            '    n upper nrhs  steps run         scipy / gamma_n  device / gamma_n  device / scipy\n' % T.BACKWARD_ERROR_FACTOR)

    def line(text):
      print(text)
      f.write(text + '\n')
      f.flush()
    yield line


@pytest.mark.parametrize('n,upper,nrhs', T.HARD_CASES)
def test_natural_refinement_backward_error(engine, report, n, upper, nrhs):
  """ BACKWARD_ERROR_FACTOR (trsolve_cases.py) was set once from the measured table with headroom; its cap, a tenth of
      the smallest unrefined / scipy ratio, is asserted by tests/test_trsolve_cases_cpu.py """
  L, B, Xref, _ = T.hard_problem(n, upper)
  A = L.T if upper else L
  Bk, Xk = T.columns(B, nrhs), T.columns(Xref, nrhs)
  X, got = _run(engine, L, Bk, upper)
  nblk = T.nblocks(n)
  r_dev, r_ref = T.ratio(A, X, Bk), T.ratio(A, Xk, Bk)
  report('%5d %5d %4d  %-16s  %15.5f  %16.5f  %14.2f' % (n, upper, nrhs, got['refine_steps'], r_ref / T.gamma(n),
                                                       r_dev / T.gamma(n), r_dev / r_ref))
  assert np.all(np.isfinite(X))
  assert got['refine_steps'] >= nblk, got                       # at least one step in every block
  assert not any(got[k] for k in T.FAST_VECTOR), got             # a refined single vector takes the general route
  assert got['trsv_general_blocks'] == (nblk if nrhs == 1 else 0), got
  assert r_dev <= T.BACKWARD_ERROR_FACTOR * r_ref, (r_dev / r_ref, r_dev / T.gamma(n))


@pytest.mark.parametrize('steps', [1, 2, 3])
def test_forced_refinement_steps(steps):
  env = dict(os.environ)
  env['DFH_REFINE_FORCE_STEPS'] = str(steps)
  env.pop('DFH_REFINE_TOL', None)
  res = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'tests', 'trsolve_forced_check.py')],
                       env=env, capture_output=True, text=True, timeout=300)
  print(res.stdout[-6000:])
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-3000:], res.stderr[-4000:])
