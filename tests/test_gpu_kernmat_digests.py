"""MI355X: every route of the kernel-matrix builder -- single-part symmetric / cross, the odd-leading-dimension
fall-through, the strip kernel with and without the fused mean, the symmetric multi-part kernel, the generic instances,
ESP, dist_squared, the prior diagonal, both pack routes, the lower-triangle build of a fit -- held bit for bit to the
digests recorded in tests/golden/kernmat_digests.npz (tests/kernmat_digest_check.py).  One subprocess per switch variant:
the DFH_KM_* / DFH_PACK_FUSED switches are read once per process."""
import os
import subprocess
import sys

import pytest

from kernmat_digest_check import VARIANTS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_kernel_matrices_bit_for_bit(engine, variant):
  env = dict(os.environ, **VARIANTS[variant][0])
  res = subprocess.run([sys.executable, os.path.join(HERE, 'kernmat_digest_check.py'), '--variant', variant], env=env,
                       capture_output=True, text=True, timeout=600)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-2000:], res.stderr[-4000:])
