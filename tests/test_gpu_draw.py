"""MI355X: dfh_gp_draw through the C-ABI -- the joint draw of one GP with evaluations in progress and S samples
(gp/gp_core.py:250-261, utils/general_utils.py:224-232) -- against the reference block by block (oracle/ref_numpy.py),
and bit for bit against the single-draw entry points it generalises.  One tolerance, the project's: 1e-10 norm-wise, or
max(1e-10, 2 err(reference, extended-precision truth)) where the reference's own draw is further than that from the
truth (tests/truth_bounds.py); the truth is built as tests/test_gpu_moo.py::_truth_draw builds it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import relerr
from oracle import ref_numpy as O

import draw_cases as D
import truth_bounds as tb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gps(engine):
  fitted = {kind: D.device_gp(engine, kind) for kind in D.KINDS}
  yield fitted
  for gp in fitted.values():
    gp.free()


def _draw(gp, kind, Xs, U, S, block, Xh, **kw):
  return gp.draw(Xs, U, num_samples=S, block=block, X_halluc=Xh if len(Xh) else None, mean_const=D.problem(kind)['mean'], **kw)


@pytest.mark.parametrize('name', sorted(D.CASES))
def test_parity_with_the_oracle(gps, name):
  """ ragged last block (300 = 2 * 128 + 44), one block, a block that needs the ladder, block = 1, block > m, q = 0 """
  c = D.case(name)
  S = c['U'].shape[1]
  samples, bvs, bis, powers = _draw(gps[c['kind']], c['kind'], c['Xs'], c['U'], S, c['block'], c['Xh'])
  bound = tb.bound(c['ref'], c['truth'])
  err = relerr(samples, c['ref'])
  print(name, 'relerr', err, 'bound', bound, 'reference vs truth', relerr(c['ref'], c['truth']), 'jitter powers', powers,
        'reference arithmetic', c['powers'], 'winners', list(bis), 'reference', c['winners'])
  assert samples.shape == c['ref'].shape
  assert err <= bound, (name, err, bound)
  assert powers == c['powers']
  for s in range(S):
    assert int(bis[s]) == c['winners'][s] and bvs[s] == samples[s, bis[s]], s


@pytest.mark.parametrize('kind', sorted(D.KINDS))
def test_one_draw_without_points_in_progress_is_dfh_gp_ts(gps, kind):
  rs = np.random.RandomState(21)
  m, block = 300, 128
  Xs, U = rs.random_sample((m, D.DIM)), rs.standard_normal(m)
  mean = D.problem(kind)['mean']
  bv, bi, want, want_powers = gps[kind].thompson(Xs, U, block=block, mean_const=mean, return_samples=True)
  samples, bvs, bis, powers = gps[kind].draw(Xs, U, num_samples=1, block=block, mean_const=mean)
  assert np.array_equal(samples[0], want) and (bvs[0], int(bis[0])) == (bv, bi) and powers == want_powers


@pytest.mark.parametrize('kind', sorted(D.KINDS))
def test_one_draw_with_points_in_progress_is_the_one_objective_mo_thompson(engine, gps, kind):
  """ dfh_mo_ts_argmax with k = 1, DFH_MO_LIN and weight 1.0 scalarises s to 0.0 + s * 1.0 """
  rs = np.random.RandomState(22)
  m, block = 300, 128
  Xs, Xh, U = rs.random_sample((m, D.DIM)), rs.random_sample((3, D.DIM)), rs.standard_normal(m)
  mean = D.problem(kind)['mean']
  bv, bi, want, want_powers = engine.mo_thompson([gps[kind]], 'lin', [1.0], None, Xs, U, block=block, X_halluc=Xh,
                                                 mean_consts=[mean], return_vals=True)
  samples, bvs, bis, powers = gps[kind].draw(Xs, U, num_samples=1, block=block, X_halluc=Xh, mean_const=mean)
  assert np.array_equal(samples[0], want) and (bvs[0], int(bis[0])) == (bv, bi) and [powers] == want_powers
  # FittedGP.thompson's keyword takes the same route
  got = gps[kind].thompson(Xs, U, block=block, mean_const=mean, return_samples=True, X_halluc=Xh)
  assert got[:2] == (bv, bi) and np.array_equal(got[2], want) and got[3] == powers
  # and the points in progress matter
  assert relerr(gps[kind].draw(Xs, U, num_samples=1, block=block, mean_const=mean)[0][0], want) > 1e-6


@pytest.mark.parametrize('B', [1, 63, 64, 65, 128, 257])
def test_row_s_of_a_multi_draw_is_the_single_draw_with_column_s(gps, B):
  """ the new kernel's summation order is the single draw's: odd and even blocks (scalar / two-element loads), blocks of
      less than one wave, exactly 64, one more, more than 256 columns (several strides per thread), a ragged last block,
      full and partial tiles of 8 draws """
  kind = 'se' if B % 2 else 'm25'
  rs = np.random.RandomState(30 + B)
  m = 3 if B == 1 else 2 * B + (B + 1) // 2
  Xs, Xh, U9 = rs.random_sample((m, D.DIM)), rs.random_sample((2, D.DIM)), rs.standard_normal((m, 9))
  gp = gps[kind]
  singles = [_draw(gp, kind, Xs, np.ascontiguousarray(U9[:, s]), 1, B, Xh) for s in range(9)]
  for S in (2, 3, 5, 8, 9):
    samples, bvs, bis, powers = _draw(gp, kind, Xs, np.ascontiguousarray(U9[:, :S]), S, B, Xh)
    for s in range(S):
      one, bv1, bi1, pw1 = singles[s]
      assert np.array_equal(samples[s], one[0]), (B, S, s, relerr(samples[s], one[0]))
      assert (bvs[s], bis[s]) == (bv1[0], bi1[0]) and powers == pw1, (B, S, s)


def test_host_inputs_equal_device_inputs(engine, gps):
  c = D.case('se_ragged_q3')
  S, mean = c['U'].shape[1], D.problem('se')['mean']
  mv = np.full(len(c['Xs']), mean)
  want = gps['se'].draw(c['Xs'], c['U'], num_samples=S, block=c['block'], X_halluc=c['Xh'], mean_vals=mv)
  dXs, dU, dmv = engine.to_device(c['Xs']), engine.to_device(c['U']), engine.to_device(mv)
  got = gps['se'].draw(dXs, dU, num_samples=S, block=c['block'], X_halluc=c['Xh'], mean_vals=dmv)
  for buf in (dXs, dU, dmv):
    buf.free()
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
  assert got[3] == want[3]
  # a constant prior mean as a value per candidate is the same draw
  assert np.array_equal(want[0], _draw(gps['se'], 'se', c['Xs'], c['U'], S, c['block'], c['Xh'])[0])


CHUNK_M, CHUNK_BLOCK, CHUNK_Q, CHUNK_S = 1300, 128, 2, 3
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_draw as M
from dragonfly_amd.engine import get_engine
np.savez(%(out)r, **M.chunk_case(get_engine()))
'''


def chunk_inputs():
  rs = np.random.RandomState(41)
  return rs.random_sample((CHUNK_M, D.DIM)), rs.random_sample((CHUNK_Q, D.DIM)), rs.standard_normal((CHUNK_M, CHUNK_S))


def chunk_case(engine):
  """ (run in the child) the S-draw and the S single draws over more candidates than one small chunk holds """
  Xs, Xh, U = chunk_inputs()
  gp = D.device_gp(engine, 'm25')
  samples, bvs, bis, powers = _draw(gp, 'm25', Xs, U, CHUNK_S, CHUNK_BLOCK, Xh)
  singles = [_draw(gp, 'm25', Xs, np.ascontiguousarray(U[:, s]), 1, CHUNK_BLOCK, Xh) for s in range(CHUNK_S)]
  return dict(samples=samples, bvs=bvs, bis=bis, powers=np.array([-99 if p is None else p for p in powers]),
              singles=np.array([one[0][0] for one in singles]), single_bis=np.array([one[2][0] for one in singles]))


def test_several_chunks(tmp_path):
  """ DFH_CHUNK_GIB is read once per process: the small-chunk run (512-row chunks, three of them) is one child """
  out = str(tmp_path / 'child.npz')
  env = dict(os.environ, DFH_CHUNK_GIB='0.0001')
  res = subprocess.run(['timeout', '-k', '10', '240', sys.executable, '-c',
                        CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)], env=env, capture_output=True,
                       text=True, timeout=300)
  assert res.returncode == 0, res.stderr[-2000:]
  child = np.load(out)
  Xs, Xh, U = chunk_inputs()
  ref, powers, truth = D.reference_draw('m25', Xs, Xh, U, CHUNK_BLOCK)
  bound = tb.bound(ref, truth)
  err = relerr(child['samples'], ref)
  print('three chunks: relerr', err, 'bound', bound, 'reference vs truth', relerr(ref, truth))
  assert err <= bound
  assert list(child['powers']) == [-99 if p is None else p for p in powers]
  assert np.array_equal(child['samples'], child['singles']) and np.array_equal(child['bis'], child['single_bis'])
  for s in range(CHUNK_S):
    assert int(child['bis'][s]) == O.argmax_first(ref[s])[1] and child['bvs'][s] == child['samples'][s, child['bis'][s]]


def test_fall_back_when_the_base_fit_needed_the_ladder(engine):
  """ The block form of the augmentation stands on a base factor without jitter.  The ladder case of
      tests/test_gpu_oracle_parity.py (SE, bandwidth 0.3 on 2-D points, a point in progress that duplicates a training
      point) with a noise variance far below the rounding of the Gram matrix: at n = 200 that matrix has a hundred
      eigenvalues of either sign around 1e-15, its factorisation fails and the ladder's first step, 1e-11 max(diag), mends
      it -- for the n x n fit and, as the reference re-runs the ladder on the whole augmented matrix
      (gp_core.py:199-206), for the (n + q) x (n + q) one.  The device factors the augmented GP from scratch too. """
  from dragonfly_amd.engine import KernelSpec
  from oracle import ref_longdouble as T
  rs = np.random.RandomState(5)
  n, d, m, S = 200, 2, 40, 2
  X = rs.rand(n, d)
  Y = np.sin(3 * X.sum(axis=1))
  scale, bw = float(Y.var()), np.full(d, 0.3)
  noise = 1e-17 * scale
  ks = O.KernelSpec('se', d, scale, bw)
  og = O.GPOracle(X, Y, ks, 0.0, noise)
  gp = engine.gp_fit(KernelSpec('se', d, scale, bw), X, Y, noise)
  assert og.jitter_power == -11 and gp.jitter_power == og.jitter_power
  Xh = np.vstack([X[7], rs.rand(d)])
  Xs, U = rs.rand(m, d), rs.standard_normal((m, S))
  mu, cov = og.eval_with_hallucinated_observations(Xs, Xh, 'covar')
  ref = O.draw_gaussian_samples_with_normals(mu, cov, U)
  _, pw = O.stable_cholesky(cov, return_power=True)
  # the truth from the kernel, as _truth_draw builds it, with the jitter each of the reference's three ladders settled on
  Xa = np.vstack([X, Xh])
  _, pa = O.stable_cholesky(ks(Xa, Xa) + noise * np.eye(n + 2), return_power=True)
  assert pa == -11
  jit_of = lambda power, M: 0.0 if power is None else (10.0 ** power) * float(np.diag(M).max())
  jit_b = jit_of(og.jitter_power, ks(X, X) + noise * np.eye(n))
  jit_a = jit_of(pa, ks(Xa, Xa) + noise * np.eye(n + 2))
  mean = T.gp_truth('se', bw, scale, X, Y, noise + jit_b, Xs, 0.0, 0.0)['mu']
  truth = np.array([mean + T.gp_truth('se', bw, scale, Xa, np.zeros(n + 2), noise + jit_a, Xs, 0.0, 0.0,
                                      ts_normals=np.ascontiguousarray(U[:, s]), ts_jitter=jit_of(pw, cov))['draw'] for s in range(S)])
  samples, bvs, bis, powers = gp.draw(Xs, U, num_samples=S, X_halluc=Xh)
  gp.free()
  bound = tb.bound(ref, truth)
  err = relerr(samples, ref)
  print('fall-back: relerr', err, 'bound', bound, 'reference vs truth', relerr(ref, truth), 'draw power', powers, pw)
  assert err <= bound and powers == [pw]
  for s in range(S):
    assert int(bis[s]) == O.argmax_first(ref[s])[1] and bvs[s] == samples[s, bis[s]]


def test_argument_errors(engine, gps):
  from dragonfly_amd import _lib
  lib, gp = engine.lib, gps['se']
  rs = np.random.RandomState(3)
  m = 10
  Xs, Xh, U = rs.random_sample((m, D.DIM)), rs.random_sample((1, D.DIM)), rs.standard_normal((m, 2))
  out = np.empty((2, m))
  ptr = lambda a: C.c_void_p(a.ctypes.data)
  call = lambda handle, xh, q, S: lib.dfh_gp_draw(handle, ptr(Xs), m, m, xh, q, ptr(U), S, 0.0, None, ptr(out), None, None, None)
  assert call(gp.handle, ptr(Xh), 1, 2) == _lib.DFH_OK
  assert call(gp.handle, None, 0, 0) == _lib.DFH_ERR_BAD_ARG             # S < 1
  assert call(gp.handle, None, 1, 1) == _lib.DFH_ERR_BAD_ARG             # points in progress without their array
  assert call(gp.handle, ptr(Xh), -1, 1) == _lib.DFH_ERR_BAD_ARG         # q < 0
  p = D.problem('se')
  gram = engine.gp_fit_gram(D.oracle_gp('se').K_trtr_wo_noise, p['Y'] - p['mean'], p['noise'])
  assert call(gram.handle, None, 0, 1) == _lib.DFH_ERR_BAD_ARG           # a posterior without a kernel
  gram.free()
  with pytest.raises(ValueError):
    gp.draw(Xs, U, num_samples=3)                                         # normals for two draws only
