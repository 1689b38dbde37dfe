"""MI355X: dfh_gp_lml_batch (csrc/lml.hip) returns, bit for bit, what the commit before the tuning objective moved into
its own translation unit returned -- one small input per route of the dispatcher (the 64 x 64 tile, the one-launch small
group, the one-launch small problem, the workgroup route with and without teams, its ladder fall-back and its
non-uniform branch with resident labels, the lock-step schedule's batched solve, the per-candidate PSD fits).
tests/golden/lml_batch_parent_bits.npz was written by tools/record_lml_bits.py at that commit, twice: a case whose
result was not bit-reproducible there carries its run-to-run relative spread and is held to twice that (two runs
bound the spread from below only); every other case to equality of the uint64 views.

The shapes are the smallest that reach each route by the thresholds of csrc/lml.hip as they stand; the test does not
observe the route taken (only the ladder case shows it, through its jitter power), so whoever moves a threshold
checks tools/record_lml_bits.py's CASES against it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import record_lml_bits as R     # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
  return dict(np.load(R.GOLDEN, allow_pickle=False))


def test_fixture_holds_every_case(golden):
  assert list(golden['names']) == [c[0] for c in R.CASES]
  assert list(golden['seeds']) == [c[1] for c in R.CASES]


@pytest.mark.parametrize('name', [c[0] for c in R.CASES])
def test_bits_of_the_parent(engine, golden, name):
  lml, powers, digest = R.run_case(engine, name)
  assert np.array_equal(digest, golden['digest_' + name]), 'the inputs rebuilt from the seed are not the recorded ones'
  want, spread = golden['lml_' + name], float(golden['spread_' + name])
  print(name, 'spread', spread, 'lml', lml.tolist(), 'recorded', want.tolist())
  assert np.array_equal(powers, golden['powers_' + name]), (name, powers, golden['powers_' + name])
  if spread == 0.0:
    assert np.array_equal(lml.view(np.uint64), want.view(np.uint64)), (name, lml, want)
  else:
    assert np.max(np.abs(lml - want) / np.abs(want)) <= 2.0 * spread, (name, lml, want, spread)
