"""MI355X: the outputs of the GP entry points -- fit, append, posterior, acquisitions, add-UCB (the multi-fidelity one
included), covariance, Thompson sampling (blocked and point-wise), joint draws, the multi-objective calls -- held bit for bit to the digests recorded in
tests/golden/api_output_digests.npz (tests/api_digest_check.py), in a subprocess whose posterior chunks are the 512-row
floor (DFH_CHUNK_GIB is read once per process), so that 1100 candidates run as three chunks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_outputs_bit_for_bit(engine):
  env = dict(os.environ, DFH_CHUNK_GIB='0.0001')
  res = subprocess.run([sys.executable, os.path.join(HERE, 'api_digest_check.py')], env=env, capture_output=True, text=True,
                       timeout=600)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-2000:], res.stderr[-4000:])
