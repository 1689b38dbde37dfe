"""MI355X: every variant of the fp64 MFMA GEMM behind the public dfh_gemm against references of the same product
(tests/gemm_check.py holds the case table, the two references and the checks).

Each case states the kernel variant it was written for -- slot = (NN ? 4 : 0) | (edge ? 2 : 0) | (64-tile ? 1 : 0),
as gemm_profile books it -- and fails if the dispatch books anything else, so a case cannot silently test another
kernel.  The test ids carry the slot: `-v` prints the table.

Slots 6 and 7 have two tenants each.  A plain NN product through the bounds-checked kernel books 6 (128-tiles) or 7
(64-tiles) by the formula above, and those are the launches booked here in-process.  The factorisation's
conditional launch, also booked as 6, is only reachable from inside the factorisation and stays with
test_gpu_chol_paths.py.  The look-ahead kernel, also booked as 7, is NT and LOWER only; DFH_GEMM_FORCE_LA=1 sends
public LOWER products of five or more tile rows through it, and because the switch is read once per process those
cases run in a child process (test_lookahead_tile_order)."""
import os
import subprocess
import sys

import pytest

import gemm_check as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_case_table_reaches_every_variant():
  booked = G.slots_in_table()
  assert all(booked[s] >= 1 for s in range(8)), dict(booked)
  assert [next(iter(c.slots)) for c in G.one_case_per_slot()] == list(range(8))
  assert all(c.slots == {G.LA: 1} and c.lower and not c.transb and c.M >= 640 for c in G.LA_CASES)


@pytest.mark.parametrize('case', G.EXACT_CASES, ids=G.case_id)
def test_exact(engine, case):
  G.check_exact(engine, case)


@pytest.mark.parametrize('case', G.ROUNDED_CASES, ids=G.case_id)
def test_rounded(engine, case):
  G.check_rounded(engine, case)


@pytest.mark.parametrize('alpha,beta', G.K0_SCALARS)
@pytest.mark.parametrize('M,N,transb,slot', G.K0_SHAPES)
def test_k_zero_null_operands(engine, M, N, transb, slot, alpha, beta):
  G.check_k0(engine, M, N, transb, slot, alpha, beta)


@pytest.mark.parametrize('M,N,K,transb,slot', G.NAN_SHAPES)
def test_nan_containment(engine, M, N, K, transb, slot):
  G.check_nan(engine, M, N, K, transb, slot)


@pytest.mark.parametrize('case', G.one_case_per_slot(), ids=G.case_id)
def test_same_call_same_bits(engine, case):
  G.check_deterministic(engine, case)


@pytest.mark.parametrize('case', G.ROWSPLIT, ids=G.case_id)
def test_row_split_rows_are_the_parts_rows(engine, case):
  G.check_row_split_bits(engine, case)


def test_row_subrange_is_tile_size_invariant(engine):
  G.check_subrange_bits(engine)


def test_lookahead_tile_order(engine):
  env = dict(os.environ)
  env['DFH_GEMM_FORCE_LA'] = '1'
  res = subprocess.run([sys.executable, os.path.join(HERE, 'gemm_check.py')], env=env, capture_output=True, text=True,
                       timeout=300)
  assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-2000:], res.stderr[-4000:])
