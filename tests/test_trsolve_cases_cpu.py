"""CPU: the conditions the assertions of tests/test_gpu_trsolve.py rest on, and the launch counts its cases expect.

The hard cases (tests/trsolve_cases.py: hard_factor, B = A Xtrue) separate a refined block-inverse solve from an
unrefined one by two orders of magnitude of backward error, with scipy's dtrtrs as the yardstick: that is what lets the
GPU test hold the device to a small multiple of scipy's error and still fail a solve that skipped its refinement.  The
launch counts are stated here once by hand, per size, and the predicates of trsolve_cases.py -- which the GPU test asserts
against Engine.solve_launches() -- must reproduce them, so that the case tables and the predicates cannot drift apart."""
import numpy as np
import pytest

import trsolve_cases as T


@pytest.fixture(scope='module')
def hard_ratios():
  """ {(n, upper, nrhs): (scipy's ratio, the unrefined mirror's, the formula-step mirror's)} """
  out = {}
  for n in T.HARD_N:
    for upper in (False, True):
      L, B, X, _ = T.hard_problem(n, upper)
      A = L.T if upper else L
      X0, XF = T.blocked_mirror(L, B, upper, 0), T.blocked_mirror(L, B, upper, 'formula')
      for k in T.HARD_NRHS:
        out[(n, upper, k)] = tuple(T.ratio(A, Z[:, :k], B[:, :k]) for Z in (X, X0, XF))
  return out


def test_hard_cases_tell_a_refined_solve_from_an_unrefined_one(hard_ratios):
  assert sorted(hard_ratios) == sorted(T.HARD_CASES)
  for (n, upper, k), (r_scipy, r_plain, r_formula) in sorted(hard_ratios.items()):
    print('n %4d upper %d nrhs %3d  scipy / gamma_n %.4f  unrefined / scipy %8.1f  formula steps / scipy %.2f'
          % (n, upper, k, r_scipy / T.gamma(n), r_plain / r_scipy, r_formula / r_scipy))
    assert 0 < r_scipy <= T.gamma(n)
    assert r_plain >= 100 * r_scipy
    assert r_formula <= 10 * r_scipy


def test_backward_error_factor_is_under_its_cap(hard_ratios):
  """ a tenth of the smallest unrefined / scipy ratio: a device solve without refinement is at least ten times over """
  cap = min(r_plain / r_scipy for r_scipy, r_plain, _ in hard_ratios.values()) / 10
  print('cap %.1f, factor %.1f' % (cap, T.BACKWARD_ERROR_FACTOR))
  assert 1.0 < T.BACKWARD_ERROR_FACTOR <= cap


@pytest.mark.parametrize('n', T.HARD_N)
def test_every_block_of_a_hard_factor_takes_a_step(n):
  deltas = T.block_deltas(T.hard_factor(n))
  steps = T.formula_steps(T.hard_factor(n))
  print(n, ['%.1e' % d for d in deltas], steps)
  assert len(steps) == T.nblocks(n) and min(steps) >= 1
  assert all(1e-8 < d < 1e-4 for d in deltas)


def test_easy_factor_takes_no_step_and_the_mirror_solves_it():
  n = 1088
  L, B, X = T.easy_problem(n, False, 8)
  assert T.formula_steps(L) == (0, 0, 0)
  T.check_easy(L, T.blocked_mirror(L, B, False, 0), B, X, False, 'mirror forward')
  Lu, Bu, Xu = T.easy_problem(n, True, 8)
  T.check_easy(Lu, T.blocked_mirror(Lu, Bu, True, 2), Bu, Xu, True, 'mirror backward, two steps')


def test_refine_steps_formula():
  assert [T.refine_steps_formula(d) for d in (0.0, 1e-13, 2e-13, 1e-8, 2e-7, 2e-5, 1e-2, 0.2, 0.25, float('nan'))] == \
      [0, 0, 1, 1, 2, 3, 7, 8, 8, 0]


# few-row GEMM launches of a forward solve with 2 <= nrhs <= 256, by hand from trsm_rows and gemm_skinny_applies:
#   1088  blocks 512 | 512 | 64: three block solves, two updates
#   512   one block solve
#   576   512 | 64: two block solves (K = 512, K = 64), one update
#   704   512 | 192: the same with K = 192
#   1000  512 | 488: the first block's solve and update; 488 is no multiple of 64
#   1001  odd leading dimension: none
#   1002  the first block's solve; ldl % 4 == 2 keeps the update out, 490 the last block
#   65, 1 none
#   2624  512 x 5 | 64: six block solves, five updates
FEW_ROW_LAUNCHES = {1088: 5, 512: 1, 576: 3, 704: 3, 1000: 2, 1001: 0, 1002: 1, 65: 0, 1: 0, 2624: 11}


def test_few_row_cases_expect_the_launches_stated_by_hand():
  assert {n for n, _ in T.FEW_ROW_CASES} == set(FEW_ROW_LAUNCHES)
  for n, k in T.FEW_ROW_CASES:
    exp = T.expected_launches(n, k, False)
    fam = T.skinny_family(k)
    assert exp[fam] == FEW_ROW_LAUNCHES[n], (n, k)
    assert sum(exp.values()) == exp[fam], (n, k, exp)          # nothing else: no refinement, no single-vector kernel
  assert [T.skinny_family(k) for k in T.FEW_NRHS] == ['skinny_1', 'skinny_1', 'skinny_2', 'skinny_2', 'skinny_4', 'skinny_4',
                                                     'skinny_8', 'skinny_8', 'skinny_16', 'skinny_16', 'skinny_16']
  assert {k for n, k in T.FEW_ROW_CASES if n == T.BITS_N} >= set(T.BITS_NRHS)


def test_few_row_table_reaches_all_eight_instantiations_on_256_compute_units():
  seen = {}
  for n, k in T.FEW_ROW_CASES:
    for name, c in T.skinny_variants(n, k, n_cu=256).items():
      seen[name] = seen.get(name, 0) + c
  assert sorted(seen) == sorted(T.SKINNY), seen
  # the unsplit MT >= 4 kernels come from the one update with more than 2048 columns
  assert T.skinny_variants(2624, 33) == {'skinny_4': 1, 'skinny_4_split': 10}
  assert T.skinny_variants(2624, 100) == {'skinny_8': 1, 'skinny_8_split': 10}
  assert T.skinny_variants(2624, 256) == {'skinny_16': 1, 'skinny_16_split': 10}
  assert T.skinny_products(1000, 17) == [512, 488] and T.skinny_products(704, 2) == [512, 192, 192]


def test_wide_and_backward_cases_expect_no_counted_launch():
  for n, k in T.WIDE_CASES:
    assert k > T.FEW_ROWS and not any(T.expected_launches(n, k, False).values())
  for n, k in T.BACKWARD_CASES:
    assert k >= 2 and not any(T.expected_launches(n, k, True).values())
  assert T.expected_launches(1000, 300, False, steps=2)['refine_steps'] == 4
  assert T.expected_launches(1088, 19, True, steps=3)['refine_steps'] == 9


# single vector: {n: (blk_fwd, upd_fwd<8>, upd_fwd<2>, blk_bwd, upd_bwd<16>, upd_bwd<64>, general blocks per direction)}
#   4162 = 8 * 512 + 66: nine blocks; 3650, 3138, 2626, 2114 rows below the first four take eight rows per wave, the four
#   shorter panels two; backward, the last block (c0 = 4096) takes 64 columns per workgroup, the seven before it 16
VECTOR_LAUNCHES = {2: (1, 0, 0, 1, 0, 0, 0), 1000: (2, 0, 1, 2, 1, 0, 0), 1536: (3, 0, 2, 3, 2, 0, 0),
                   4162: (9, 4, 4, 9, 7, 1, 0), 4608: (9, 4, 4, 9, 7, 1, 0), 1001: (0, 0, 0, 0, 0, 0, 2)}


def test_single_vector_cases_expect_the_launches_stated_by_hand():
  assert sorted(T.VECTOR_CASES) == sorted(VECTOR_LAUNCHES)
  hit = dict.fromkeys(T.FAST_VECTOR, 0)
  for n in T.VECTOR_CASES:
    fwd, bwd = T.expected_launches(n, 1, False), T.expected_launches(n, 1, True)
    want = VECTOR_LAUNCHES[n]
    assert (fwd['trsv_blk_fwd'], fwd['trsv_upd_fwd8'], fwd['trsv_upd_fwd2']) == want[:3], n
    assert (bwd['trsv_blk_bwd'], bwd['trsv_upd_bwd16'], bwd['trsv_upd_bwd64']) == want[3:6], n
    assert fwd['trsv_general_blocks'] == bwd['trsv_general_blocks'] == want[6], n
    assert sum(fwd.values()) == sum(want[:3]) + want[6] and sum(bwd.values()) == sum(want[3:6]) + want[6]
    for k in hit:
      hit[k] += fwd[k] + bwd[k]
  assert all(hit.values()), hit                                # every kernel of the fast route, both update variants
  # a block that is refined sends the whole solve down the general route
  assert T.expected_launches(1088, 1, False, steps=2) == dict(T.expected_launches(1089, 1, False), refine_steps=6)


def test_forced_cases_cover_the_four_forms():
  forms = {(k == 1, 1 < k <= T.FEW_ROWS and not up, k > T.FEW_ROWS and not up, k > 1 and up) for _, k, up in T.FORCED_CASES}
  assert len(forms) == 4 and {n for n, _, _ in T.FORCED_CASES} == {1000, 1088}


def test_ratio_and_mirror_on_a_tiny_system():
  L = np.array([[2.0, 0.0], [1.0, 4.0]])
  B = np.array([[2.0], [9.0]])
  X = np.array([[1.0], [2.0]])
  assert T.ratio(L, X, B) == 0.0
  assert T.ratio(L, X + np.array([[0.0], [0.5]]), B) == 2.0 / (1.0 + 10.0 + 9.0)
  assert np.array_equal(T.blocked_mirror(L, B, False, 0), X)
  assert np.allclose(T.blocked_mirror(L, np.array([[4.0], [8.0]]), True, 1), [[1.0], [2.0]])
