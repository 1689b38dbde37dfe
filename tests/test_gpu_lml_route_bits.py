"""MI355X: every branch of dfh_gp_lml_batch's route chooser and of its two schedules -- the in-kernel ladder, a one-launch
candidate handed on alone, resident labels, a kernel the one-launch forms refuse, the tile edges and both ends of the
workgroup route, the label cache, the PSD route, section timing, the failures with their texts, and twelve switch variants --
held to the bits the library returned before its host side was taken apart: tests/golden/lml_route_bits.npz
(tests/lml_route_bits_check.py, which states the comparison rule).  One subprocess per variant: the DFH_LML_* switches are
read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lml_route_bits_check import GOLDEN, VARIANTS

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fixture_was_recorded_twice_and_reproduced():
  """ every variant recorded twice; at most two calls carry a run-to-run spread, none above 1e-13 """
  known = dict(np.load(GOLDEN, allow_pickle=False))
  for variant in VARIANTS:
    assert int(known[variant + '__runs']) >= 2, variant
  spreads = {k: float(v) for k, v in known.items() if k.endswith('__spread')}
  assert len(spreads) >= sum(len(cases) for _, cases in VARIANTS.values())
  carried = {k: v for k, v in spreads.items() if v != 0.0}
  assert len(carried) <= 2 and all(v <= 1e-13 for v in carried.values()), carried


@pytest.mark.gpu
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_routes_bit_for_bit(engine, variant):
  env = dict(os.environ, **VARIANTS[variant][0])
  res = subprocess.run([sys.executable, os.path.join(HERE, 'lml_route_bits_check.py'), '--variant', variant], env=env,
                       capture_output=True, text=True, timeout=300)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-3000:], res.stderr[-4000:])
