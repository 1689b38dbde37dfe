"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

One acquisition step of dragonfly_amd.gpb_acquisitions / multiobjective_gpb_acquisitions per case, on the device, through
the mirrors: Euclidean GPs, BOCA's view of a multi-fidelity GP (through A.boca), the Cartesian-product device GP and the
multi-objective acquisitions -- each with candidates (and normals) drawn in HBM and drawn on the host, with and without
points in progress, with the fitter's constant mean and with a callable one.  Per case three things are kept:

    <case>|point    the returned point (BOCA: fidelity, then point), float64 bits
    <case>|tail     np.random.random(4) drawn right after the step: where the global state was left
    <case>|stream   the calls the mirrors made on the fitted handles and the engine, in order: the method, per array
                    argument D (DeviceArray) or H (host array) and its shape, and the sorted keyword names

tests/test_gpu_acq_steps.py holds them bit for bit to tests/golden/acq_step_parent.npz, which the package recorded before
the acquisition modules were folded into one fused step.  The spy wraps methods of the handle and engine objects of the
case and records only what the mirrors call on them (calls an engine method makes itself are not recorded); it does not
look into the library.

    acq_step_cases.py --record FILE    write the records into FILE (created or updated).  Record twice into the same file:
                                       a key whose second record differs from its first is stored empty -- it did not
                                       reproduce and is not checked; such keys are findings to report.

The inputs are built by + - * / only from RandomState(seed).random_sample, so their bytes do not depend on the host's
libm.  Shapes: n = 40, d = 3, 200 candidates (Thompson sampling under 'pdoo': 800, past a 256-thread block); the product
domain is the recorded mixed case of tests/golden/cp_acq_n70.npz (n = 70, 257 candidates).
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'acq_step_parent.npz')
N, DIM, MAX_EVALS, SEED = 40, 3, 200, 4322
GROUPS = [[0, 2], [1]]
MEAN_C = 0.125
HANDLE_METHODS = ('acq_argmax', 'thompson', 'thompson_pointwise', 'draw', 'predict', 'predict_covar', 'add_ucb_group',
                  'add_ucb_all', 'mf_add_ucb_group', 'mf_add_ucb_all')
ENGINE_METHODS = ('random_candidates', 'random_normals', 'join_fixed', 'empty', 'to_device', 'mo_ucb_argmax', 'mo_thompson')


def uniforms(seed, shape):
  return np.random.RandomState(seed).random_sample(shape)


def poly_labels(X):
  return 4.0 * (X[:, 0] - 0.5) * (X[:, 0] - 0.5) * (X[:, 1] - 0.2) - 3.0 * (X[:, 1] - 0.6) * (X[:, 1] - 0.6) + \
         2.0 * (X[:, 2] - 0.4) * (X[:, 0] - 0.7)


def _rows_mean(x):
  """ a prior mean that is no constant: a polynomial of the first two coordinates of each row """
  x = np.asarray([np.asarray(r, dtype=np.float64) for r in x]).reshape(len(x), -1)
  return MEAN_C + 0.5 * x[:, 0] - 0.4 * x[:, 0] * x[:, 1]


def _cp_mean(pts):
  """ the same on the points of the mixed product domain: a polynomial of the float part """
  return np.array([MEAN_C + 0.5 * p[0][0] - 0.4 * p[0][0] * p[0][1] for p in pts])


# the spy ------------------------------------------------------------------------------------------------------------------
def _describe(arg):
  from dragonfly_amd.engine import DeviceArray
  if isinstance(arg, DeviceArray):
    return 'D%s' % (tuple(int(s) for s in arg.shape),)
  if isinstance(arg, np.ndarray):
    return 'H%s' % (arg.shape,)
  if isinstance(arg, (list, tuple)) and len(arg) > 0 and all(isinstance(a, (np.ndarray, DeviceArray)) for a in arg):
    return '[%s]' % ','.join(_describe(a) for a in arg)
  if isinstance(arg, str):
    return arg
  return '-'


class Spy(object):
  """ Records the calls made from outside on the wrapped objects while it is active; the objects are as before afterwards """

  def __init__(self, handles, engine):
    self.targets = [(h, HANDLE_METHODS) for h in handles] + [(engine, ENGINE_METHODS)]
    self.calls, self.depth, self.wrapped = [], 0, []

  def _wrap(self, name, fn):
    def call(*args, **kwargs):
      if self.depth == 0:
        kws = [k if _describe(kwargs[k]) == '-' else '%s=%s' % (k, _describe(kwargs[k])) for k in sorted(kwargs)]
        self.calls.append('%s(%s;%s)' % (name, ','.join(_describe(a) for a in args), ','.join(kws)))
      self.depth += 1
      try:
        return fn(*args, **kwargs)
      finally:
        self.depth -= 1
    return call

  def __enter__(self):
    for obj, names in self.targets:
      for name in names:
        if hasattr(obj, name) and name not in vars(obj):
          setattr(obj, name, self._wrap(name, getattr(obj, name)))
          self.wrapped.append((obj, name))
    return self

  def __exit__(self, *exc):
    for obj, name in self.wrapped:
      delattr(obj, name)
    self.wrapped = []

  def stream(self):
    return ' '.join(self.calls)


# what the acquisitions read of a domain and of BOCA's function caller --------------------------------------------------------
class Box(object):
  def __init__(self, bounds):
    self.bounds = np.asarray(bounds, dtype=np.float64)
    self.dim = len(self.bounds)

  def get_type(self):
    return 'euclidean'

  def get_dim(self):
    return self.dim


class CPDomain(object):
  list_of_domains = ()

  def get_type(self):
    return 'cartesian_product'

  def has_constraints(self):
    return False


class StubCaller(object):
  """ what boca() reads of the function caller (as in tests/test_gpu_boca.py) """
  fidel_to_opt = np.array([1.0])

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):
    del point, filter_by_cost
    return [np.array([0.25]), np.array([0.5])], [0.25, 0.5]

  def get_information_gap(self, fidels):
    return [0.75, 0.5][:len(fidels)]


BOUNDS = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5]])


def _data():
  U = uniforms(1, (N, DIM))
  X = BOUNDS[:, 0] + U * (BOUNDS[:, 1] - BOUNDS[:, 0])
  return X, poly_labels(U)


def _in_progress(q):
  """ two points in the corner where the posterior of these labels peaks, so that hallucinating them moves the winners """
  return list(np.array([[0.0625, 0.875, 0.53125], [0.09375, 0.9375, 0.5]])[:q])


def _mean(kind):
  from dragonfly_amd.gp_core import ConstantMean
  return ConstantMean(MEAN_C) if kind == 'const' else _rows_mean


def _bandwidths(dim=DIM):
  return 0.6 * (1 + 0.2 * np.arange(dim))


# the four families: each returns (handles to spy on, step() -> point as a flat float64 array) --------------------------------
def euclidean_case(acq, q, mean, method='rand', max_evals=MAX_EVALS, mask_fused_draws=False):
  from dragonfly_amd import gpb_acquisitions as A, kernel as K
  from dragonfly_amd.euclidean_gp import EuclideanGP
  X, Y = _data()
  if acq == 'add_ucb':
    bw = _bandwidths()
    kern = K.AdditiveKernel(1.5, [K.SEKernel(2, 1.0, bw[GROUPS[0]]), K.MaternKernel(1, 2.5, 1.0, bw[GROUPS[1]])], GROUPS)
  else:
    kern = K.SEKernel(DIM, 0.5, _bandwidths())
  gp = EuclideanGP(list(X), list(Y), kern, _mean(mean), 0.01)
  anc = Namespace(domain=Box(BOUNDS), domain_bounds=BOUNDS, acq_opt_method=method, max_evals=max_evals, t=N + 1,
                  curr_max_val=float(Y.max()), is_mf=False, handle_parallel='halluc', eval_points_in_progress=_in_progress(q))
  if mask_fused_draws:
    gp.device_gp.fused_draws = False                 # on this handle alone: the sampler route of asy_ts
  return [gp.device_gp], lambda: np.asarray(getattr(A.asy, acq)(gp, anc), dtype=np.float64).ravel()


def boca_case(acq, q, mean):
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, mf_gp
  X, Y = _data()
  Z = uniforms(2, (N, 1))
  Z[::3] = 1.0                                       # a third of the evaluations at fidel_to_opt itself
  Y = Y * (0.5 + Z[:, 0])
  bw = _bandwidths()
  if acq == 'add_ucb':
    dom = K.AdditiveKernel(1.25, [K.MaternKernel(2, 2.5, 1.0, bw[GROUPS[0]]), K.SEKernel(1, 1.0, bw[GROUPS[1]])], GROUPS)
  else:
    dom = K.MaternKernel(DIM, 2.5, 1.0, bw)
  gp = mf_gp.EuclideanMFGP(list(Z), list(X), list(Y), None, 0.75, K.SEKernel(1, 1.0, np.array([0.6])), dom, _mean(mean), 0.01)
  fidels, points = [np.array([0.75]), np.array([0.5])][:q], _in_progress(q)
  anc = Namespace(curr_acq=acq, domain=Box(BOUNDS), domain_bounds=BOUNDS, acq_opt_method='rand', max_evals=MAX_EVALS, t=N + 1,
                  curr_max_val=float(Y.max()), is_mf=True, mf_strategy='boca', handle_parallel='halluc',
                  eval_points_in_progress=points, eval_fidels_in_progress=fidels,
                  eval_fidel_points_in_progress=gp.get_ZX_from_ZZ_XX(fidels, points), boca_thresh_coeff=0.01,
                  boca_max_low_fidel_cost_ratio=0.9, y_range=float(Y.max() - Y.min()))

  def step():
    fidel, point = A.boca(getattr(A.asy, acq), gp, anc, StubCaller())
    return np.concatenate([np.asarray(fidel, dtype=np.float64).ravel(), np.asarray(point, dtype=np.float64).ravel()])
  return [gp.device_gp], step


def _cp_unpack(P):
  return [[row[0:2].copy(), [int(row[2])], [int(row[3]), int(row[4])]] for row in P]


def cp_case(acq, q, mean):
  """ the mixed domain as recorded from the reference (tests/golden/cp_acq_n70.npz): the candidates are the recorded ones
      (there is no reference on the GPU machine to sample the domain with) """
  from dragonfly_amd import gpb_acquisitions as A, kernel as K
  from dragonfly_amd.gp_core import ConstantMean, GP
  g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'cp_acq_n70.npz'), allow_pickle=False))

  class PackedCPGP(GP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  kern = K.CartesianProductKernel(float(g['scale']), [K.SEKernel(2, 1.0, g['se_bw']), K.MaternKernel(1, 2.5, 1.0, g['matern_bw']),
                                                       K.HammingKernel(g['hamming_w'])])
  mean_func = ConstantMean(float(g['mean_const'])) if mean == 'const' else _cp_mean
  gp = PackedCPGP(_cp_unpack(g['Xp']), list(g['Y']), kern, mean_func, float(g['noise']), handle_non_psd_kernels='project_first')
  anc = Namespace(domain=CPDomain(), acq_opt_method='rand', max_evals=257, t=71, curr_max_val=float(np.max(g['Y'])), is_mf=False,
                  handle_parallel='halluc', eval_points_in_progress=_cp_unpack(g['Hp'])[:q])
  cands = _cp_unpack(g['Cp'])
  assert A.cp_acquisition_applies(acq, gp, anc)

  def step():
    saved = A._cp_candidates                         # pylint: disable=protected-access
    A._cp_candidates = lambda anc_data: cands[:int(anc_data.max_evals)]
    try:
      point = getattr(A.asy, acq)(gp, anc)
    finally:
      A._cp_candidates = saved
    return np.concatenate([np.asarray(part, dtype=np.float64).ravel() for part in point])
  return [gp.device_gp], step


def mo_case(scal, acq, q, mean, method='rand'):
  from dragonfly_amd import kernel as K, multiobjective_gpb_acquisitions as M
  from dragonfly_amd.gp_core import GP
  X, Y = _data()
  Y2 = 0.5 - (X[:, 0] - 0.6) * (X[:, 0] - 0.6) - 0.3 * X[:, 1] * X[:, 2]
  gps = [GP(list(X), list(Y), K.SEKernel(DIM, 0.5, _bandwidths()), _mean(mean), 0.01),
         GP(list(X), list(Y2), K.MaternKernel(DIM, 2.5, 0.75, 1.5 * _bandwidths()), _mean(mean), 0.02)]
  anc = Namespace(domain=Box(BOUNDS), acq_opt_method=method, max_evals=MAX_EVALS, obj_weights=[0.6, 0.4],
                  reference_point=[-0.5, -0.75], t=N + 1, handle_parallel='halluc', is_mf=False,
                  eval_points_in_progress=_in_progress(q), curr_max_val=None)
  return [gp.device_gp for gp in gps], lambda: np.asarray(getattr(M.asy, '%s_%s' % (scal, acq))(gps, anc), dtype=np.float64).ravel()


def _cases():
  """ name (without the candidates' side) -> builder """
  out = {}
  for mean in ('const', 'call'):
    for q in (0, 2):
      tag = 'q%d|%s' % (q, mean)
      for acq in ('ucb', 'ei', 'pi', 'ttei', 'ts'):
        out['euc|%s|%s' % (acq, tag)] = lambda acq=acq, q=q, mean=mean: euclidean_case(acq, q, mean)
        out['boca|%s|%s' % (acq, tag)] = lambda acq=acq, q=q, mean=mean: boca_case(acq, q, mean)
      for acq in ('ucb', 'ei', 'ttei', 'ts'):
        out['cp|%s|%s' % (acq, tag)] = lambda acq=acq, q=q, mean=mean: cp_case(acq, q, mean)
      for scal in ('lin', 'tch'):
        out['mo|%s_ts|%s' % (scal, tag)] = lambda scal=scal, q=q, mean=mean: mo_case(scal, 'ts', q, mean)
    for scal in ('lin', 'tch'):
      out['mo|%s_ucb|q0|%s' % (scal, mean)] = lambda scal=scal, mean=mean: mo_case(scal, 'ucb', 0, mean)
  for q in (0, 2):                                   # add-UCB reads no prior mean of the GP
    out['euc|add_ucb|q%d|const' % q] = lambda q=q: euclidean_case('add_ucb', q, 'const')
    out['boca|add_ucb|q%d|const' % q] = lambda q=q: boca_case('add_ucb', q, 'const')
  out['euc|ts-pdoo|q0|const'] = lambda: euclidean_case('ts', 0, 'const', method='pdoo')
  out['euc|ts-sampler|q2|const'] = lambda: euclidean_case('ts', 2, 'const', mask_fused_draws=True)
  out['euc|add_ucb-pdoo|q0|const'] = lambda: euclidean_case('add_ucb', 0, 'const', method='pdoo', max_evals=60)
  out['mo|lin_ucb-pdoo|q0|const'] = lambda: mo_case('lin', 'ucb', 0, 'const', method='pdoo')
  return out


CASES = _cases()
SIDES = ('dev', 'host')                              # candidates (and normals) drawn in HBM / on the host


def run_case(name, side):
  """ {'point', 'tail', 'stream'} of one step """
  from dragonfly_amd import gpb_acquisitions as A
  from dragonfly_amd.engine import get_engine
  handles, step = CASES[name]()
  saved = A.DEVICE_CANDIDATES
  A.DEVICE_CANDIDATES = side == 'dev'
  try:
    np.random.seed(SEED)
    with Spy(handles, get_engine()) as spy:
      point = step()
    tail = np.random.random(4)
  finally:
    A.DEVICE_CANDIDATES = saved
  return dict(point=point, tail=tail, stream=np.array(spy.stream()))


def run_all():
  out = {}
  for name in sorted(CASES):
    for side in SIDES:
      for what, val in run_case(name, side).items():
        out['%s|%s|%s' % (name, side, what)] = val
  return out


def same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def load(path):
  if not os.path.exists(path):
    return {}
  with np.load(path, allow_pickle=False) as z:
    return {k: z[k] for k in z.files}


def main():
  assert len(sys.argv) == 3 and sys.argv[1] == '--record', __doc__
  path = sys.argv[2]
  np.random.seed(SEED)
  assert np.random.random() >= 0.5                   # TTEI's coin takes the two-step branch
  known = load(path)
  got = run_all()
  for key, val in got.items():
    print(key, val.tolist() if val.dtype.kind == 'f' else str(val))
    known[key] = val if key not in known or same(known[key], val) else np.zeros(0)
  np.savez_compressed(path, **known)
  print('empty: %s' % sorted(k for k in known if known[k].size == 0))
  print('OK')


if __name__ == '__main__':
  main()
