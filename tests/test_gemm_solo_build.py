"""CPU: what the solo form of the 128-tile fp64 GEMM (gemm_f64_solo_kernel) must be by design, read from the built
library's code-object metadata (tools/isa_audit.py --resources): no scratch, no spilled register, and a static LDS
image of two stages of 256 rows x 34 doubles = 139264 B -- more than half a CU's 160 KB, which is what keeps a
second workgroup off the CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import isa_audit  # noqa: E402  pylint: disable=wrong-import-position

LIB = os.path.join(ROOT, 'dragonfly_amd', 'libdfhip.so')


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_audit.LLVM, 'llvm-readelf')), reason='ROCm LLVM tools not found')
def test_solo_kernel_resources():
  assert os.path.exists(LIB), 'libdfhip.so is not built (python -m dragonfly_amd.build)'
  usage = {k: v for k, v in isa_audit.resource_usage(LIB).items() if 'gemm_f64_solo_kernel' in k}
  assert len(usage) == 1, sorted(usage)
  (name, r), = usage.items()
  assert r['scratch'] == 0, '%s: %d B/lane of scratch' % (name, r['scratch'])
  assert r['vgpr_spill'] == 0, '%s: %d spilled VGPRs' % (name, r['vgpr_spill'])
  assert r['lds'] == 2 * 256 * 34 * 8 == 139264, '%s: %d B of LDS' % (name, r['lds'])
