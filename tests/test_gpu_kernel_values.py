"""MI355X: the VALUES of every kernel-matrix route, element by element in ulps against a long-double truth, on
exact-argument inputs (tests/kernel_value_check.py holds the case table, the truth and the checks), and the acquisition
epilogue over a z sweep into the subnormal tail of Phi (tests/acq_tail_check.py).

Every case names the route it was written for and fails when kernmat_dispatch books another
(Engine.counters()['km_route']), so a case cannot silently test another kernel; the test ids carry variant and route.
The variants whose switches are read once per process (DFH_KM_CFG, DFH_KM_STRIP, DFH_KM_SYMMULTI) run their cases in a
child process each, one at a time, with a time limit of its own.  The column-weighted route is reachable only through
the multi-fidelity calls and stays with test_gpu_boca.py; the strip kernel with the mean riding along is reached here
through a fit's predict and held to the strip kernel's own matrix."""
import numpy as np
import pytest

import acq_tail_check as A
import kernel_value_check as V

pytestmark = pytest.mark.gpu
IN_PROCESS = [c for c in V.CASES if c.variant == 'default']


def test_route_table_reaches_every_route_but_colw(engine):
  reached = set()
  for case in V.EDGE_CASES:
    if case.variant == 'default':
      ref = V.reference_of(case)
      V.km(engine, case.route, ref.spec, ref.X1, ref.X2)
      reached.add(engine.counters()['km_route'])
  # strip + mean: a prediction of at least 8 packed columns books the mean riding along, and its bits are those of
  # K(X*, X) alpha with the strip kernel's own K within the rounding of the sum
  case = next(c for c in V.CASES if c.route == 'strip' and c.kernel == 'se')
  ref = V.reference_of(case)
  gp = engine.gp_fit(ref.spec, ref.X2, np.cos(ref.X2[:, 0]), 0.01)
  try:
    before = engine.counters()['km_dispatches']
    mu = gp.predict(ref.X1, want_std=False)[0]
    assert engine.counters()['km_route'] == 'strip_mean' and engine.counters()['km_dispatches'] == before + 1
    reached.add('strip_mean')
    K = V.km(engine, 'strip', ref.spec, ref.X1, ref.X2)
    alpha = gp.get_alpha()
    assert np.all(np.abs(mu - K.dot(alpha)) <= 4 * len(alpha) * 2.0 ** -53 * np.abs(K).dot(np.abs(alpha)))
  finally:
    gp.free()
  assert reached == set(V.ROUTES) - {'colw'}, reached


@pytest.mark.parametrize('case', IN_PROCESS, ids=V.case_id)
def test_values_in_ulps(engine, case):
  V.check_values(engine, case)


@pytest.mark.parametrize('case', [c for c in V.EDGE_CASES if c.variant == 'default'], ids=V.case_id)
def test_edges(engine, case):
  V.check_edges(engine, case)


@pytest.mark.parametrize('variant', [v for v in V.VARIANTS if v != 'default'])
def test_variant_in_child_process(engine, variant):
  res = V.run_child(variant)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-3000:], res.stderr[-4000:])


@pytest.mark.parametrize('acq', ['pi', 'ei', 'ttei'])
def test_acquisition_tails(engine, acq):
  A.check(engine, acq)


@pytest.mark.parametrize('acq', ['pi', 'ei', 'ttei'])
def test_acquisition_nan_sigma(engine, acq):
  A.check_nan(engine, acq)
