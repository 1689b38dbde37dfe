"""MI355X: the K-loop pipeline of the 128 x 128-tile fp64 GEMM where its schedule can go wrong -- few chunks, a
chunk count that differs between the tiles of one launch, a guard off by one.

The 128-tile loop keeps chunk c+1 in registers while it multiplies chunk c, writes it into the other LDS buffer
between the two MFMA groups and reads the first fragments of chunk c+1 behind the barrier, all of it guarded by
"is there a chunk c+1", so the interesting chunk counts are 0, 1 (no staging at all), 2 (one hand-over), 3 (both LDS
buffers written twice) and a few more of either parity.  tests/gemm_check.py covers K = 16, 17 and 48 on these
tiles; the cases here add K = 32 ... 96 on whole tiles and K = 1 ... 81 through the bounds-checked kernel, with the
same two references (integer inputs: the int64 product bit for bit; randn inputs: gamma_{K+2} against long double)
and the same booking check -- each case states the gemm_profile slot it was written for.

The K-clipped product with a triangular B (GEMM_KTRI_B, inside the blocked triangular solve) is the one launch whose
tiles have different chunk counts -- 8, 16, 24 and 32 for the four tile columns of a 512-block: a 1024 x 6144 solve
runs it on 48 x 4 = 192 128-tiles and is held to the componentwise residual bound of a backward-stable solve.

Run as a program with DFH_GEMM_FORCE_LA=1 (read once per process) the LOWER cases LA_PIPE go through the look-ahead
kernel, which shares the tile body."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_check as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# both epilogues: alpha = -1 takes beta * C in through the accumulators in the tile prologue, alpha = 0.5 adds it at
# the end
SCALARS = [(-1, 1), (0.5, -1)]

NT128_PIPE = [G._case('pipe', 1792, 1792, K, False, a, b, G.NT128) for K in (32, 64, 80, 96) for a, b in SCALARS]
# ragged M and N (14 x 15 tiles) and every K the edge kernel's k predicate can clip a chunk at; the scalars alternate
NT128E_PIPE = [G._case('pipe', 1791, 1793, K, False, *SCALARS[i % 2], G.NT128E)
               for i, K in enumerate((1, 15, 31, 33, 49, 65, 81))]
NN128_PIPE = [G._case('pipe', 1792, 1792, K, True, -1, 1, G.NN128) for K in (32, 64)]
LOWER_PIPE = [G._case('pipe', 1792, 1792, K, False, a, b, G.NT128, lower=True)
              for K in (32, 64) for a, b in ((-1, 1), (0.5, 0))]
EXACT = NT128_PIPE + NT128E_PIPE + NN128_PIPE + LOWER_PIPE
ROUNDED = [NT128_PIPE[2], NT128E_PIPE[3], NN128_PIPE[0]]          # K = 64 (-1, 1); K = 33; NN K = 32
SAME_BITS = [NT128_PIPE[2], NT128E_PIPE[5]]

# look-ahead order (child process): 5 and 8 tile rows, two and three chunks
LA_PIPE = [G._case('la', M, M, K, False, -1, 1, G.LA, lower=True) for M in (640, 1024) for K in (32, 48)]


@pytest.mark.parametrize('case', EXACT, ids=G.case_id)
def test_exact(engine, case):
  G.check_exact(engine, case)


@pytest.mark.parametrize('case', ROUNDED, ids=G.case_id)
def test_rounded(engine, case):
  G.check_rounded(engine, case)


@pytest.mark.parametrize('case', SAME_BITS, ids=G.case_id)
def test_same_call_same_bits(engine, case):
  G.check_deterministic(engine, case)


@pytest.mark.parametrize('alpha', [1, 2])
@pytest.mark.parametrize('beta', [0, 0.5, 1])
def test_k_zero_on_128_tiles(engine, alpha, beta):
  """ no chunk at all: out = beta * C straight from the prologue (alpha = 1) or the epilogue (alpha = 2) """
  G.check_k0(engine, 1792, 1792, False, G.NT128, alpha, beta)


def test_lookahead_tile_order():
  env = dict(os.environ)
  env['DFH_GEMM_FORCE_LA'] = '1'
  res = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=300)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-2000:], res.stderr[-4000:])


def test_k_clipped_triangular_b(engine):
  """ L X = B with n = 1024 and 6144 right-hand sides: per 512-block of L one K-clipped product of 48 x 4 128-tiles
      whose tile columns run 8, 16, 24 and 32 chunks.  L has diagonal 4 and off-diagonal entries in (-0.5, 0.5) /
      sqrt(n); the residual of a backward-stable solve obeys |L X - B| <= gamma_n (|L| |X| + |B|), the bound
      asserted carries the condition number of L on top:  |L X - B| <= gamma_n kappa(L) (|L| |X| + |B|). """
  n, nrhs = 1024, 6144
  rs = np.random.RandomState(1024 + 6144)
  L = np.tril((rs.rand(n, n) - 0.5) / np.sqrt(n), -1) + 4.0 * np.eye(n)
  B = rs.randn(n, nrhs)
  X, booked = G.profiled(engine, lambda: engine.solve_triangular(L, B))
  assert booked.get(G.NT128, 0) >= 2, booked             # the K-clipped multiplies of the two 512-blocks
  kappa = float(np.linalg.cond(L))
  res = np.abs(L.dot(X) - B)
  bound = G.gamma(n) * kappa * (np.abs(L).dot(np.abs(X)) + np.abs(B))
  ratio = float(np.max(res / bound))
  print('kappa(L) = %.3f, largest residual / bound = %.4f, slots booked %r' % (kappa, ratio, booked))
  assert np.all(np.isfinite(X))
  assert not (res > bound).any(), G.first_bad(res > bound)


def main():
  from dragonfly_amd.engine import get_engine
  assert os.environ.get('DFH_GEMM_FORCE_LA') == '1'
  eng = get_engine()
  for c in LA_PIPE:
    G.check_exact(eng, c)
    print('ok', G.case_id(c))
  G.check_deterministic(eng, LA_PIPE[-1])
  print('OK')


if __name__ == '__main__':
  main()
