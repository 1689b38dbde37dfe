"""MI355X: one acquisition step per case of tests/acq_step_cases.py through the mirrors -- Euclidean GPs, BOCA's view, the
Cartesian-product device GP, the multi-objective acquisitions; candidates and normals drawn in HBM and on the host -- held
bit for bit to tests/golden/acq_step_parent.npz: the point returned, where the global np.random state was left, and the
calls made on the fitted handles and the engine, as the package made them before gpb_acquisitions was folded into one
fused step (recorded twice on the device; a key that did not reproduce is stored empty and fails as such).  Nothing is
tolerated: the library is the same, so a step that returns other bits or calls the engine differently has changed.

Independently of the file, the two sides of a case -- candidates in HBM / on the host -- return the same point and leave
the same state: the device generators continue the global stream bit for bit."""
import numpy as np
import pytest

import acq_step_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def records(engine):
  del engine
  return S.run_all()


@pytest.fixture(scope='module')
def parent():
  return S.load(S.GOLDEN)


def test_the_record_holds_exactly_these_cases(parent):
  want = set('%s|%s|%s' % (name, side, what) for name in S.CASES for side in S.SIDES for what in ('point', 'tail', 'stream'))
  assert set(parent) == want


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_step_is_the_recorded_step(records, parent, name):
  for side in S.SIDES:
    for what in ('point', 'tail', 'stream'):
      key = '%s|%s|%s' % (name, side, what)
      got, want = records[key], parent[key]
      print(key, str(got) if what == 'stream' else got.tolist())
      assert want.size > 0, '%s did not reproduce when the file was recorded (stored empty)' % key
      assert S.same(got, want), '%s: %s, recorded %s' % (key, got, want)


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_candidates_in_hbm_and_on_the_host_give_the_same_step(records, name):
  for what in ('point', 'tail'):
    dev, host = records['%s|dev|%s' % (name, what)], records['%s|host|%s' % (name, what)]
    assert S.same(dev, host), '%s %s: in HBM %s, on the host %s' % (name, what, dev.tolist(), host.tolist())
  assert np.all(np.isfinite(records['%s|dev|point' % name]))
