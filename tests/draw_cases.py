"""Shared data of the joint-draw tests (dfh_gp_draw; tests/test_gpu_draw*.py, tests/test_gpu_mgpu_halluc.py): one small
GP per kernel, the cases, and per case the reference's draw block by block (oracle/ref_numpy.py) with its
extended-precision truth (built as tests/test_gpu_moo.py::_truth_draw builds it).  Everything here runs on the CPU;
each case is computed once per process and handed out unchanged."""
import functools

import numpy as np

from oracle import ref_numpy as O

N, DIM = 150, 3
KINDS = {'se': ('se', 0.3, 0.0), 'm25': ('matern', 0.5, 2.5)}      # kind -> (kernel, base bandwidth, nu)

# name -> (kernel, candidates, block, points in progress, draws, candidate rows set equal to row 3)
CASES = {
  'se_ragged_q3': ('se', 300, 128, 3, 3, ()),            # 300 = 2 * 128 + 44
  'm25_ragged_q3': ('m25', 300, 128, 3, 3, ()),
  'se_one_block_q1': ('se', 300, 300, 1, 3, ()),
  'm25_jitter_q2': ('m25', 160, 160, 2, 2, (7, 100)),    # a singular block: the ladder adds 1e-11 max(diag)
  'se_block1_q3': ('se', 9, 1, 3, 2, ()),
  'm25_block_over_m_q0': ('m25', 37, 64, 0, 3, ()),
}


@functools.lru_cache(maxsize=None)
def problem(kind):
  """ RandomState(7): X uniform (150, 3), Y = sin(3 sum x) + 0.05 N(0, 1); scale Var(Y), mean median(Y), noise Var(Y) / 20,
      bandwidths bw (1 + 0.2 j).  Returns the objective as tests/test_gpu_moo.py describes one. """
  rs = np.random.RandomState(7)
  X = rs.random_sample((N, DIM))
  Y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.standard_normal(N)
  _, bw, _ = KINDS[kind]
  return dict(kind=kind, X=X, Y=Y, scale=float(Y.var()), mean=float(np.median(Y)), noise=float(Y.var() / 20),
              bw=bw * (1 + 0.2 * np.arange(DIM)))


def oracle_gp(kind):
  p = problem(kind)
  kernel, _, nu = KINDS[kind]
  spec = O.KernelSpec('se', DIM, p['scale'], p['bw']) if kernel == 'se' else O.KernelSpec('matern', DIM, p['scale'], p['bw'], nu=nu)
  return O.GPOracle(p['X'], p['Y'], spec, p['mean'], p['noise'])


def device_gp(engine, kind):
  """ the same GP fitted on the device (labels centred by the constant mean, which the draw adds back) """
  from dragonfly_amd.engine import KernelSpec
  p = problem(kind)
  kernel, _, nu = KINDS[kind]
  spec = KernelSpec('se', DIM, p['scale'], p['bw']) if kernel == 'se' else KernelSpec('matern', DIM, p['scale'], p['bw'], nu=nu)
  return engine.gp_fit(spec, p['X'], p['Y'] - p['mean'], p['noise'])


def inputs(name):
  """ candidates, points in progress and normals [m x S] of a case """
  kind, m, block, q, S, dup = CASES[name]
  rs = np.random.RandomState(1000 + sorted(CASES).index(name))
  Xs = rs.random_sample((m, DIM))
  for row in dup:
    Xs[row] = Xs[3]
  Xh = rs.random_sample((q, DIM))
  U = rs.standard_normal((m, S))
  return kind, Xs, Xh, U, block


def reference_draw(kind, Xs, Xh, U, block, want_truth=True):
  """ The reference block by block: gp.draw_samples_with_hallucinated_observations(S, x_b, Xh) (gp.draw_samples for no
      points in progress) with the normals U_b.  Returns (draws [S x m], jitter powers per block, truth [S x m]). """
  from test_gpu_moo import _truth_draw
  p, og = problem(kind), oracle_gp(kind)
  m, S = U.shape
  ref, truth, powers = np.empty((S, m)), np.empty((S, m)), []
  for b0 in range(0, m, block):
    xb, Ub = Xs[b0:b0 + block], U[b0:b0 + block]
    mu, cov = og.eval_with_hallucinated_observations(xb, Xh, 'covar') if len(Xh) else og.eval(xb, 'covar')
    ref[:, b0:b0 + len(xb)] = O.draw_gaussian_samples_with_normals(mu, cov, Ub)
    powers.append(O.stable_cholesky(cov, return_power=True)[1])
    for s in range(S if want_truth else 0):
      truth[s, b0:b0 + len(xb)], pw = _truth_draw(p['X'], p, xb, Xh, np.ascontiguousarray(Ub[:, s]))
      assert pw == powers[-1]
  return ref, powers, (truth if want_truth else None)


@functools.lru_cache(maxsize=None)
def case(name):
  kind, Xs, Xh, U, block = inputs(name)
  ref, powers, truth = reference_draw(kind, Xs, Xh, U, block)
  for a in (Xs, Xh, U, ref, truth):
    a.setflags(write=False)
  return dict(kind=kind, Xs=Xs, Xh=Xh, U=U, block=block, ref=ref, powers=powers, truth=truth,
              winners=[O.argmax_first(row)[1] for row in ref])
