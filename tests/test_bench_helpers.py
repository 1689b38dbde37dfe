"""CPU: the measurement code's own arithmetic (bench.py) -- the error norms it reports, the fp64-pipe bound, and the
two CPU legs stage by stage: the oracle's port against the reference's stored outputs and, where a Dragonfly checkout
exists, against the reference's own functions bit for bit."""
import os

import numpy as np
import pytest

import bench
from conftest import load_golden, relerr
from oracle import make_golden as MG


def test_error_norms():
  b = np.array([1.0, 1e-6, -2.0, 0.0])
  a = b + np.array([1e-12, 1e-12, 0.0, 1e-12])
  assert bench.rel(a, b) == pytest.approx(1e-12 / 2.0)
  # element-wise: only entries with |b| >= 1e-3 max|b| count (1e-6 and 0 are masked)
  assert bench.rel_elem(a, b) == pytest.approx(1e-12)
  assert bench.both(a, b) == [bench.rel(a, b), bench.rel_elem(a, b)]
  assert bench.rel_elem([], []) == 0.0 and bench.rel_elem([0.0], [0.0]) == 0.0


def test_fp64_pipe_bound():
  r = bench.fp64_pipe_frac('se', 32, 1e9, 1, 1.0)
  # 2 * 32 flop per element on the matrix cores, 28 vector instructions per element
  assert r['min_ms_mfma'] == pytest.approx(2 * 32 * 1e9 / 78.6e12 * 1e3, rel=1e-3)
  assert r['min_ms_valu'] == pytest.approx(28 * 1e9 / 39.3e12 * 1e3, rel=1e-3)
  assert r['frac_of_fp64_pipe_peak'] == pytest.approx((r['min_ms_mfma'] + r['min_ms_valu']) / 1.0, rel=1e-3)


# (n = 2048 with 1100 candidates: OpenBLAS / LAPACK take their blocked, multi-threaded code paths there -- dpotrf's
#  recursive panels, dtrsm / dgemm blocking -- which n = 384 does not reach: `kind: port` is pinned to the reference's
#  own functions at a size where the library's blocking matters)
#  Without a Dragonfly checkout the port is held to the reference's outputs stored by `python oracle/make_golden.py cpu_legs`
#  (tests/golden/cpu_legs_reference.npz): to 1e-12, as BLAS results move in the last bits with the host's thread count;
#  with a checkout, the two legs are also run side by side and must agree bit for bit.
@pytest.mark.parametrize('n,m', MG.CPU_LEGS_CASES)
def test_cpu_legs_agree_stage_by_stage(monkeypatch, n, m):
  prob, X, Y, cands, U = MG.cpu_legs_inputs(n, m)
  monkeypatch.setenv('DRAGONFLY_REFERENCE', '')
  fp, kp, kind_p, _ = bench.cpu_functions(prob)
  assert kind_p == 'port'
  _, b = bench.oracle_stages(fp, kp, X, Y, prob['mean_c'], prob['noise'], [cands], [U], posterior_chunks=[cands])
  g = load_golden('cpu_legs_reference')
  want = lambda k: g['n%d_%s' % (n, k)]
  assert relerr(b['alpha'], want('alpha')) < 1e-12 and abs(b['lml'] - float(want('lml'))) < 1e-12 * abs(float(want('lml')))
  for k in ('mu', 'sd', 'draw'):
    assert relerr(b['blocks'][0][k], want(k)) < 1e-12, k
  assert b['blocks'][0]['argmax'] == int(want('argmax'))
  assert relerr(b['posterior'][0]['sd'], want('posterior_sd')) < 1e-12
  if not os.path.isdir(os.path.join(MG.REF, 'dragonfly')):
    return
  monkeypatch.setenv('DRAGONFLY_REFERENCE', MG.REF)
  fr, kr, kind_r, _ = bench.cpu_functions(prob)
  assert kind_r == 'reference'
  _, a = bench.oracle_stages(fr, kr, X, Y, prob['mean_c'], prob['noise'], [cands], [U], posterior_chunks=[cands])
  assert np.array_equal(a['alpha'], b['alpha']) and a['lml'] == b['lml']
  for key in ('mu', 'sd', 'draw'):
    assert np.array_equal(a['blocks'][0][key], b['blocks'][0][key])
  assert a['blocks'][0]['argmax'] == b['blocks'][0]['argmax']
  assert np.array_equal(a['posterior'][0]['sd'], b['posterior'][0]['sd'])


def test_contract_line_carries_the_side_targets_inside_roofline():
  """ The last stdout line of bench.py is the contract's JSON line cut from the full record: short enough to survive a
      tail, every side target a scalar INSIDE `roofline` (a record that keeps roofline's scalars keeps them). """
  import json
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  full = None
  for ln in open(os.path.join(root, 'profiles', 'r05_bench.json')):
    if ln.startswith('{"metric'):
      full = json.loads(ln)
  line = bench.contract_line(full)
  text = json.dumps(line)
  assert len(text) < 4000
  for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
    assert key in line
  r = line['roofline']
  assert all(not isinstance(v, (dict, list)) for v in r.values())
  assert r['cholesky_frac_of_fp64_mfma_peak'] == full['roofline']['side_targets']['cholesky_frac_of_fp64_mfma_peak']
  assert r['kernel_matrix_frac_by_section8d_bytes'] == full['roofline']['side_targets']['kernel_matrix_frac_by_section8d_bytes']
  assert r['chol_ms'] == full['chol_ms'] and r['solve_ms'] == full['solve_ms'] and r['comm_ranks_formed'] == 1
  assert r['C2_chol_ms'] == full['configs']['C2']['sections_ms']['chol']
  assert set(line['cpu_baseline']) == {'value', 'unit', 'cores', 'kind', 'sample'}
  assert 'workload' in line['config'] and 'model' not in line['config']


def test_dump_outputs_writes_the_last_step_as_float64(tmp_path):
  """ --dump-outputs: one float64 .npy per value the timed path returns; an index survives the cast exactly. """
  result = {'lml': -8983.546226064143, 'best': 10.538616786596952, 'idx': 2097151}
  bench.dump_outputs(str(tmp_path / 'out'), result)
  assert sorted(os.listdir(str(tmp_path / 'out'))) == ['lml.npy', 'ts_argmax.npy', 'ts_best.npy']
  for name, key in bench.DUMP_KEYS:
    a = np.load(str(tmp_path / 'out' / (name + '.npy')))
    assert a.dtype == np.float64 and a.shape == (1,) and a[0] == result[key]
