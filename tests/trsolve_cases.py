"""Inputs, references and checks of the block-inverse triangular solves (csrc/trsolve.hip: trsv_*, trsm_rows,
trsm_rows_backward; under them the few-row MFMA kernel gemm_skinny_kernel<MT, SPLIT> of csrc/gemm_f64.hip), shared by
tests/test_gpu_trsolve.py, its child tests/trsolve_forced_check.py and the CPU test tests/test_trsolve_cases_cpu.py.

Two kinds of factor, both built without a Cholesky of the whole matrix:
  easy   tril((rand - 0.5) / sqrt(n), -1) + 4 I: kappa ~ 1, every 512-block inverse is good and no solve is refined.
         A solution is held to the project's 1e-11 against scipy.linalg.solve_triangular (dtrtrs) and to
             |fl(A X) - B| <= 2 gamma_n (|A| |X| + |B|),   gamma_n = n u / (1 - n u),   u = 2^-53
         -- one gamma_n is the residual of a backward-stable solve, the other the evaluation of A X in float64.
  hard   the same strict lower part, with each 512-block of the diagonal replaced by the Cholesky factor of a squared-
         exponential Gram matrix (bandwidth 0.15, points rand(w), + 1e-12 I): the explicit inverse M of such a block has
         max|I - M L_bb| between 2e-7 and 2e-5, which refine_steps' formula (csrc/chol.hip) answers with 2 or 3 steps.
         Right-hand sides are B = A Xtrue (Xtrue = randn; the product in numpy.longdouble, rounded): a random B does not
         excite the inverse's error, this one does.  The yardstick is the backward error
             ratio(A, X, B) = max(|A X - B| / (|A| |X| + |B|))
         of the device against scipy's on the same problem.  blocked_mirror is the device's algorithm in NumPy: with the
         formula's steps its ratio stays within a small factor of scipy's, without them it is at least 100 times larger
         (tests/test_trsolve_cases_cpu.py asserts both), so a solve that skips its refinement cannot pass.

Every case also states what it expects of Engine.solve_launches(), from the dispatch predicates of trsolve.hip and
gemm_f64.hip restated here as functions of n, nrhs and the direction: a case cannot silently test another kernel."""
import functools
import math
import os
import sys

import numpy as np
from scipy.linalg import solve_triangular

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

U = 2.0 ** -53
NB = 512                        # CHOL_NB: the block of the kept inverses
FEW_ROWS = 256                  # TRSM_FEW_ROWS: at most this many right-hand sides take the few-row form
REFINE_TOL = 1e-13              # DFH_REFINE_TOL's default
TOL = 1e-11                     # the project's bound on a triangular solve against scipy (test_gpu_trsv.py)

# -- the tables -------------------------------------------------------------------------------------------------------
# few-row form, forward: (n, nrhs).  n = 1088 = 512 + 512 + 64: every product is eligible for the few-row GEMM, K = 512 and
# a single 64-slab.  512: one block, no update.  576: the last block's K is a single slab.  704: three slabs.  1000: the
# last block (488 rows: no multiple of 64) falls back, the update's column tile is clamped at rest = 488.  1001 (odd
# leading dimension): nothing is eligible.  1002 (n % 4 == 2): the block solve is eligible, the update is not.  65, 1: one
# short block.  2624 = 5 * 512 + 64: the first update has rest = 2112 > 2048 columns, more 64-column workgroups than an
# eighth of the CUs, so the unsplit MT = 4, 8, 16 kernels run.
FEW_NRHS = (2, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256)
FEW_ROW_CASES = [(1088, k) for k in FEW_NRHS] + \
                [(512, 2), (512, 17), (512, 64), (512, 256),
                 (576, 16), (576, 33), (576, 129),
                 (704, 2), (704, 65), (704, 255),
                 (1000, 17), (1000, 128), (1000, 256),
                 (1001, 2), (1001, 33), (1001, 256),
                 (1002, 16), (1002, 65), (1002, 255),
                 (65, 2), (65, 129), (1, 2), (1, 256),
                 (2624, 33), (2624, 100), (2624, 256)]
BITS_N, BITS_NRHS = 1088, (2, 17, 256)                    # batch invariance, bit for bit
WIDE_CASES = [(n, k) for n in (513, 1000, 1536) for k in (257, 300, 640)]
BACKWARD_CASES = [(n, k) for n in (1, 65, 512, 513, 1000, 1536) for k in (2, 19, 256, 257, 300)]
# single vector: even sizes take the four kernels of their own.  4162 = 8 * 512 + 66: upd_fwd<8> over 3650, 3138, 2626 and
# 2114 rows (none a multiple of the 32 rows of a workgroup), upd_bwd<64> from a last block of 66 rows; 4608: upd_bwd<64>
# from a whole block.  An odd size (odd leading dimension) takes the general route.
VECTOR_CASES = [2, 1000, 1536, 4162, 4608, 1001]
# natural refinement: hard factors, both directions
HARD_N, HARD_NRHS = (1000, 1088, 1600), (1, 24, 300)
HARD_CASES = [(n, upper, k) for n in HARD_N for upper in (False, True) for k in HARD_NRHS]
# The device's backward error may be this many times scipy's on a hard case.  Measured on the MI355X
# (profiles/trsolve_backward_error.txt): 0.46 .. 6.1, the largest where scipy's own ratio happens to be small (0.0025
# gamma_n; the NumPy mirror with the formula's steps is at 4.3 there) -- every device ratio is below 0.02 gamma_n.  Set
# once, at twice the largest measured value for run-to-run differences.  The cap is a tenth of the smallest (unrefined
# mirror / scipy) ratio among HARD_CASES, which tests/test_trsolve_cases_cpu.py computes (203, so the cap is 20.3) and
# holds this number to: a solve that skips its refinement is at least seventeen times over the bound.
BACKWARD_ERROR_FACTOR = 12.0
# forced steps (the child): the forms at the two sizes, (n, nrhs, upper)
FORCED_CASES = [(n, k, up) for n in (1000, 1088) for (k, up) in ((1, False), (1, True), (17, False), (256, False),
                                                                  (300, False), (19, True), (300, True))]

COUNTERS = ('trsv_blk_fwd', 'trsv_upd_fwd8', 'trsv_upd_fwd2', 'trsv_blk_bwd', 'trsv_upd_bwd16', 'trsv_upd_bwd64',
            'trsv_general_blocks', 'refine_steps')
SKINNY = ('skinny_1', 'skinny_2', 'skinny_4', 'skinny_4_split', 'skinny_8', 'skinny_8_split', 'skinny_16',
          'skinny_16_split')
SKINNY_FAMILIES = ('skinny_1', 'skinny_2', 'skinny_4', 'skinny_8', 'skinny_16')
FAST_VECTOR = COUNTERS[:6]


def gamma(n):
  return n * U / (1.0 - n * U)


def relerr(a, b):
  from conftest import relerr as conftest_relerr
  return conftest_relerr(a, b)


# -- factors and right-hand sides ---------------------------------------------------------------------------------------
def _strict_lower(n, seed):
  rs = np.random.RandomState(seed)
  return np.tril((rs.rand(n, n) - 0.5) / np.sqrt(n), -1)


@functools.lru_cache(maxsize=2)
def easy_factor(n, seed=0):
  L = _strict_lower(n, 7919 * n + seed) + 4.0 * np.eye(n)
  L.setflags(write=False)
  return L


@functools.lru_cache(maxsize=4)
def hard_factor(n, seed=0):
  L = _strict_lower(n, 7919 * n + seed)
  for b, c0 in enumerate(range(0, n, NB)):
    w = min(NB, n - c0)
    x = np.random.RandomState(104729 * (seed + 1) + 31 * n + b).rand(w)
    K = np.exp(-(x[:, None] - x[None, :]) ** 2 / (2 * 0.15 ** 2)) + 1e-12 * np.eye(w)
    L[c0:c0 + w, c0:c0 + w] = np.linalg.cholesky(K)
  L.setflags(write=False)
  return L


@functools.lru_cache(maxsize=8)
def easy_problem(n, upper, ncols):
  """ (L, B [n x ncols], scipy's X); a case with fewer right-hand sides takes the first columns """
  L = easy_factor(n)
  B = np.random.RandomState(13 * n + ncols + (1 if upper else 0)).randn(n, ncols)
  X = solve_triangular(L, B, lower=True, trans='T' if upper else 'N')
  for a in (B, X):
    a.setflags(write=False)
  return L, B, X


def longdouble_product(A, X):
  """ fl_64(A X) with the sum in numpy.longdouble, row block by row block over the columns where the triangular A
      (n x n, lower or upper) is not zero; X is n x k """
  n = A.shape[0]
  A = np.ascontiguousarray(A)
  lower = not np.any(np.triu(A, 1))
  Xl = X.astype(np.longdouble)
  out = np.empty((n, X.shape[1]))
  for i0 in range(0, n, 128):
    i1 = min(n, i0 + 128)
    j0, j1 = (0, i1) if lower else (i0, n)
    out[i0:i1] = A[i0:i1, j0:j1].astype(np.longdouble).dot(Xl[j0:j1]).astype(np.float64)
  return out


@functools.lru_cache(maxsize=None)
def hard_problem(n, upper):
  """ (L, B = A Xtrue [n x max(HARD_NRHS)], scipy's X, the step count of refine_steps' formula per block) """
  L = hard_factor(n)
  A = L.T if upper else L
  Xtrue = np.random.RandomState(17 * n + (1 if upper else 0)).randn(n, max(HARD_NRHS))
  B = longdouble_product(A, Xtrue)
  X = solve_triangular(L, B, lower=True, trans='T' if upper else 'N')
  for a in (B, X):
    a.setflags(write=False)
  return L, B, X, formula_steps(L)


def columns(B, nrhs):
  """ the first nrhs columns as the engine wants them: a vector for one right-hand side """
  return np.ascontiguousarray(B[:, 0]) if nrhs == 1 else np.ascontiguousarray(B[:, :nrhs])


# -- the measures ---------------------------------------------------------------------------------------------------------
def ratio(A, X, B):
  """ componentwise backward error max(|A X - B| / (|A| |X| + |B|)), the residual evaluated in float64 """
  X2, B2 = X.reshape(X.shape[0], -1), B.reshape(B.shape[0], -1)
  den = np.abs(A).dot(np.abs(X2)) + np.abs(B2)
  res = np.abs(A.dot(X2) - B2)
  ok = den > 0
  assert not (res[~ok] > 0).any()
  return float(np.max(res[ok] / den[ok])) if ok.any() else 0.0


def check_easy(L, X, B, Xref, upper, what=''):
  """ the two assertions of an easy case: the project's bound against scipy, and the residual of a backward-stable
      solve evaluated in float64 """
  n = L.shape[0]
  A = L.T if upper else L
  X2, B2 = X.reshape(n, -1), B.reshape(n, -1)
  assert X.shape == B.shape and np.all(np.isfinite(X)), what
  err = relerr(X2, Xref.reshape(n, -1))
  res = np.abs(A.dot(X2) - B2)
  bound = 2 * gamma(n) * (np.abs(A).dot(np.abs(X2)) + np.abs(B2))
  bad = res > bound
  worst = float(np.max(res / np.where(bound > 0, bound, 1.0)))
  print('%s relerr %.2e  residual / bound %.4f' % (what, err, worst))
  assert err < TOL, (what, err)
  assert not bad.any(), (what, worst, tuple(int(v) for v in np.argwhere(bad)[0]))


# -- the device's algorithm in NumPy --------------------------------------------------------------------------------------
def refine_steps_formula(delta, tol=REFINE_TOL):
  """ refine_steps of csrc/chol.hip """
  if not delta > tol:
    return 0
  if not delta < 0.25:
    return 8
  return min(8, max(1, int(math.ceil(math.log(1e-15) / math.log(delta))) - 1))


def _block_inverses(L):
  n = L.shape[0]
  out = []
  for c0 in range(0, n, NB):
    Lbb = np.tril(L[c0:c0 + NB, c0:c0 + NB])
    M = solve_triangular(Lbb, np.eye(Lbb.shape[0]), lower=True)
    out.append((Lbb, M, float(np.max(np.abs(np.eye(Lbb.shape[0]) - M.dot(Lbb))))))
  return out


def block_deltas(L):
  return [d for _, _, d in _block_inverses(L)]


def formula_steps(L):
  return tuple(refine_steps_formula(d) for d in block_deltas(L))


def blocked_mirror(L, B, upper, steps):
  """ The block substitution by explicit 512-block inverses, x_b = M_b t_b with t_b the right-hand side less the
      blocks already solved, then `steps` rounds of x_b += M_b (t_b - L_bb x_b) -- an integer, or 'formula' for
      refine_steps' count per block. """
  n = L.shape[0]
  B2 = B.reshape(n, -1)
  X = np.zeros_like(B2)
  blocks = _block_inverses(L)
  order = range(len(blocks) - 1, -1, -1) if upper else range(len(blocks))
  for b in order:
    Lbb, M, delta = blocks[b]
    c0, c1 = b * NB, min(n, (b + 1) * NB)
    if upper:
      t = B2[c0:c1] - L[c1:, c0:c1].T.dot(X[c1:])
      Ab, Mb = Lbb.T, M.T
    else:
      t = B2[c0:c1] - L[c0:c1, :c0].dot(X[:c0])
      Ab, Mb = Lbb, M
    x = Mb.dot(t)
    for _ in range(refine_steps_formula(delta) if steps == 'formula' else steps):
      x = x + Mb.dot(t - Ab.dot(x))
    X[c0:c1] = x
  return X.reshape(B.shape)


# -- what a case must book ------------------------------------------------------------------------------------------------
def nblocks(n):
  return (n + NB - 1) // NB


def skinny_family(nrhs):
  tiles = (nrhs + 15) // 16
  return 'skinny_1' if tiles <= 1 else 'skinny_2' if tiles <= 2 else 'skinny_4' if tiles <= 4 else \
      'skinny_8' if tiles <= 8 else 'skinny_16'


def skinny_products(n, nrhs):
  """ the column counts N of the few-row GEMM launches of trsm_rows(n, nrhs) with ldl = ldk = n, in launch order
      (gemm_skinny_applies: K = w a multiple of 64; A = Kct + c0 with an even ldk; B = the panel of L with ldl a
      multiple of 4 and a 32-byte aligned start, or the inverse block, stride 512) """
  if not 1 <= nrhs <= FEW_ROWS:
    return []
  out = []
  for c0 in range(0, n, NB):
    w = min(NB, n - c0)
    rest = n - c0 - w
    if n % 2 == 0 and w % 64 == 0:
      out.append(w)
    if rest > 0 and n % 4 == 0:
      out.append(rest)
  return out


def skinny_variants(n, nrhs, n_cu=256):
  """ the instantiations by name, split resolved for a device of n_cu compute units (gemm_skinny_nt) """
  fam = skinny_family(nrhs)
  out = {}
  for N in skinny_products(n, nrhs):
    split = (nrhs + 15) // 16 > 2 and (N + 63) // 64 <= n_cu // 8
    name = fam + ('_split' if split else '')
    out[name] = out.get(name, 0) + 1
  return out


def expected_launches(n, nrhs, upper, steps=0):
  """ What dfh_solve_triangular(n, nrhs, upper) books in Engine.solve_launches(), the split and unsplit few-row kernels
      of one MT added up (families()): `steps` refinement steps in every block (0: an easy factor, nothing forced). """
  exp = dict.fromkeys(COUNTERS + SKINNY_FAMILIES, 0)
  nblk = nblocks(n)
  exp['refine_steps'] = steps * nblk
  if nrhs == 1:
    if n % 2 or steps > 0:                               # trsv_fast_applies: even ldl, no block refined
      exp['trsv_general_blocks'] = nblk
    elif not upper:
      exp['trsv_blk_fwd'] = nblk
      for c0 in range(0, n, NB):
        below = n - c0 - min(NB, n - c0)
        if below > 4 * NB:
          exp['trsv_upd_fwd8'] += 1
        elif below > 0:
          exp['trsv_upd_fwd2'] += 1
    else:
      exp['trsv_blk_bwd'] = nblk
      for c0 in range(NB, n, NB):
        exp['trsv_upd_bwd16' if c0 < 8 * NB else 'trsv_upd_bwd64'] += 1
  elif not upper and nrhs <= FEW_ROWS:
    exp[skinny_family(nrhs)] = len(skinny_products(n, nrhs))
  return exp


def families(counts):
  """ solve_launches() (or a difference of two) with the split and unsplit few-row kernels of one MT added up """
  out = {k: counts[k] for k in COUNTERS}
  for fam in SKINNY_FAMILIES:
    out[fam] = counts[fam] + counts.get(fam + '_split', 0)
  return out


def booked(engine, fn):
  """ (fn(), what it added to engine.solve_launches()) """
  before = engine.solve_launches()
  out = fn()
  after = engine.solve_launches()
  return out, {k: after[k] - before[k] for k in after}
