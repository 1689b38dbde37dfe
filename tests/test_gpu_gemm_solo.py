"""MI355X: the solo form of the 128 x 128-tile fp64 NT GEMM (gemm_f64_solo_kernel: one workgroup per CU, K in chunks
of 32 through a double-buffered LDS image, one barrier per chunk, the last chunk peeled).

By default only long-K products with a full wave of tiles take it.  DFH_GEMM_SOLO (read once per process) = 2 sends
every product that is eligible but for K and the tile count through it, so the checks run in a child process with
that setting, on 1792 x 1792 x K (196 tiles) with the two references of tests/gemm_check.py:
  K = 32 one chunk (nothing staged), 64 one hand-over, 96 both LDS buffers written twice, 128 and 160 the steady
  state of either buffer parity; each with alpha = -1 (beta * C enters through the accumulators) and alpha = 0.5
  (added in the epilogue); K = 64, 96 with LOWER as well.
The K-clipped product with a triangular B (inside the blocked triangular solve) is the launch whose tile columns run
different chunk counts -- 4, 8, 12 and 16 -- and is held to the residual bound of test_k_clipped_triangular_b.
K = 48 is no multiple of the chunk and stays on the two-workgroup kernel.  Engine.gemm_solo_launches() must have
counted exactly the eligible launches: the kernel under test is what ran.

The solo loop sums the same products in the same order as the chunk-of-16 loop: a second child with
DFH_GEMM_SOLO=0 computes the same randn products and the parent compares the arrays bit for bit.

Run as a program:  test_gpu_gemm_solo.py OUTDIR   (DFH_GEMM_SOLO = 0 or 2 in the environment)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_check as G

pytestmark = pytest.mark.gpu

SCALARS = [(-1, 1), (0.5, -1)]
SOLO_EXACT = ([G._case('solo', 1792, 1792, K, False, a, b, G.NT128) for K in (32, 64, 96, 128, 160) for a, b in SCALARS] +
              [G._case('solo', 1792, 1792, K, False, a, b, G.NT128, lower=True) for K in (64, 96) for a, b in SCALARS])
SOLO_ROUNDED = G._case('solo', 1792, 1792, 96, False, -1, 1, G.NT128)
NOT_A_CHUNK_MULTIPLE = G._case('solo', 1792, 1792, 48, False, -1, 1, G.NT128)
BITS_K = (64, 96, 160)


def bits_products(eng):
  """ {name: result} of the randn products whose bits the two kernels must share: C - A B^T, plain and LOWER """
  out = {}
  for K in BITS_K:
    rs = np.random.RandomState(1792 + K)
    A, B, C = rs.randn(1792, K), rs.randn(1792, K), rs.randn(1792, 1792)
    for lower in (False, True):
      out['k%d_%s' % (K, 'lower' if lower else 'plain')] = eng.gemm(A, B, C, alpha=-1.0, beta=1.0, lower_only=lower)
  return out


def triangular_b(eng):
  """ as test_gpu_gemm_pipeline.test_k_clipped_triangular_b; returns the NT128 launches the solve booked """
  n, nrhs = 1024, 6144
  rs = np.random.RandomState(1024 + 6144)
  L = np.tril((rs.rand(n, n) - 0.5) / np.sqrt(n), -1) + 4.0 * np.eye(n)
  B = rs.randn(n, nrhs)
  X, booked = G.profiled(eng, lambda: eng.solve_triangular(L, B))
  assert booked.get(G.NT128, 0) >= 2, booked             # the K-clipped multiplies of the two 512-blocks
  kappa = float(np.linalg.cond(L))
  res = np.abs(L.dot(X) - B)
  bound = G.gamma(n) * kappa * (np.abs(L).dot(np.abs(X)) + np.abs(B))
  print('kappa(L) = %.3f, largest residual / bound = %.4f, slots booked %r' % (kappa, float(np.max(res / bound)), booked))
  assert np.all(np.isfinite(X))
  assert not (res > bound).any(), G.first_bad(res > bound)
  return booked[G.NT128]


def main(outdir):
  from dragonfly_amd.engine import get_engine
  mode = os.environ.get('DFH_GEMM_SOLO')
  assert mode in ('0', '2')
  eng = get_engine()
  assert eng.gemm_solo_launches() == 0
  expected = 0
  if mode == '2':
    for c in SOLO_EXACT:
      G.check_exact(eng, c)
      expected += 1
      assert eng.gemm_solo_launches() == expected, (G.case_id(c), eng.gemm_solo_launches(), expected)
      print('ok', G.case_id(c))
    G.check_rounded(eng, SOLO_ROUNDED)
    expected += 1
    assert eng.gemm_solo_launches() == expected
    # the solve's NT128 launches: per 512-block the update by the blocks before it and the K-clipped multiply; the
    # first block's update has K = 0 (a copy through the tile prologue and epilogue) and no chunk for the solo loop
    booked = triangular_b(eng)
    assert booked == 4, booked
    expected += 3
    assert eng.gemm_solo_launches() == expected, (eng.gemm_solo_launches(), expected)
    G.check_exact(eng, NOT_A_CHUNK_MULTIPLE)
    assert eng.gemm_solo_launches() == expected, 'K = 48 took the solo kernel'
  for name, arr in bits_products(eng).items():
    np.save(os.path.join(outdir, name + '.npy'), arr)
  expected += 2 * len(BITS_K) if mode == '2' else 0
  assert eng.gemm_solo_launches() == expected, (eng.gemm_solo_launches(), expected)
  print('OK')


def _child(mode, outdir):
  env = dict(os.environ)
  env['DFH_GEMM_SOLO'] = mode
  os.makedirs(outdir)
  res = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), outdir], env=env,
                       capture_output=True, text=True, timeout=300)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-3000:], res.stderr[-4000:])


def test_forced_solo_cases_and_bits(tmp_path):
  """ the child with DFH_GEMM_SOLO=2 runs every case above; then the same randn products from either kernel,
      bit for bit """
  solo, plain = str(tmp_path / 'solo'), str(tmp_path / 'plain')
  _child('2', solo)
  _child('0', plain)
  names = sorted(os.listdir(solo))
  assert names == sorted(os.listdir(plain)) and len(names) == 2 * len(BITS_K)
  for name in names:
    a, b = np.load(os.path.join(solo, name)), np.load(os.path.join(plain, name))
    assert np.array_equal(a, b), (name, G.first_bad(a != b))


def test_default_dispatch_keeps_short_k_on_the_two_workgroup_kernel(engine):
  """ K = 64 is below any K floor the dispatch may have (never under 1024): the counter does not move """
  before = engine.gemm_solo_launches()
  G.check_exact(engine, G._case('solo', 1792, 1792, 64, False, -1, 1, G.NT128))
  assert engine.gemm_solo_launches() == before


if __name__ == '__main__':
  main(sys.argv[1])
