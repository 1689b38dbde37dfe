"""MI355X: the tuning inner loop cut over several devices (dfh_mgpu_lml_batch, parallel.MultiEngine.gp_lml_batch).
A test box has one device, so the ranks are contexts of device 0 driven concurrently from their own host threads
(library test switch DFH_MGPU_ALLOW_DUPLICATE_DEVICES, as tests/test_gpu_mgpu.py) and `spread=True` cuts batches
that would not fill one device.  The contract: rank r's slice of the result is, bit for bit, what Engine.gp_lml_batch
returns for those candidates alone; the whole result stays within the tolerance tests/test_gpu_hp_tuning.py applies
to the same quantity (1e-10 relative to the oracle)."""
import functools
import importlib.util
import os
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu
TOL = 1e-10          # tests/test_gpu_hp_tuning.py: TOL


@pytest.fixture(scope='module')
def multis():
  """ MultiEngine(nranks) on nranks contexts of device 0, made on first use, shared by the tests of this module """
  from dragonfly_amd import parallel
  made = {}
  saved = os.environ.get('DFH_MGPU_ALLOW_DUPLICATE_DEVICES')
  os.environ['DFH_MGPU_ALLOW_DUPLICATE_DEVICES'] = '1'

  def get(nranks):
    if nranks not in made:
      made[nranks] = parallel.MultiEngine(nranks, device_ids=[0] * nranks)
    return made[nranks]
  yield get
  for mg in made.values():
    mg.close()
  if saved is None:
    del os.environ['DFH_MGPU_ALLOW_DUPLICATE_DEVICES']
  else:
    os.environ['DFH_MGPU_ALLOW_DUPLICATE_DEVICES'] = saved


@functools.lru_cache(maxsize=None)
def _se_problem(n, nb=65, d=3):
  """ (X, Y, specs, oracle specs, means, noises): SE-ARD candidates on n points; a smaller batch is a prefix """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(1000 + n)
  X = rs.rand(n, d)
  Y = np.sin(4 * X.sum(axis=1)) + 0.1 * rs.randn(n)
  yv = float(Y.var())
  specs, ospecs = [], []
  for _ in range(nb):
    scale, bw = yv * (0.5 + rs.rand()), 0.3 + 0.6 * rs.rand(d)
    specs.append(KernelSpec('se', d, scale, bw))
    ospecs.append(O.KernelSpec('se', d, scale, bw))
  means = list(0.2 * rs.randn(nb))
  noises = list(yv * np.exp(rs.uniform(np.log(0.005), np.log(0.2), nb)))
  return X, Y, specs, ospecs, means, noises


def _assert_slices_equal_single_device(engine, mg, specs, X, Y, means, noises, spread=True, **kwargs):
  """ the first row of the table: every rank's slice, values and jitter powers, equals the single-device call on
      those candidates bit for bit; the cut the library reports is lml_shard_plan's.  Returns (lml, powers, cut). """
  from dragonfly_amd import parallel
  nb = len(specs)
  plan = parallel.lml_shard_plan(nb, len(X), mg.size, spread=spread)
  # (the single-device calls first: they are the reference, computed once, with the device to themselves)
  want = [engine.gp_lml_batch(specs[lo:hi], X, Y, means[lo:hi], noises[lo:hi], return_powers=True, **kwargs) if hi > lo else None
          for lo, hi in plan]
  lml, powers, cut = mg.gp_lml_batch(specs, X, Y, means, noises, return_powers=True, return_shards=True, spread=spread, **kwargs)
  assert cut == plan
  assert lml.shape == (nb,) and len(powers) == nb
  for (lo, hi), w in zip(plan, want):
    if w is not None:
      assert np.array_equal(lml[lo:hi], w[0]), (lo, hi, lml[lo:hi], w[0])
      assert powers[lo:hi] == w[1], (lo, hi)
  return lml, powers, cut


@pytest.mark.parametrize('nranks', [2, 3])
@pytest.mark.parametrize('nb', [1, 2, 7, 65])
@pytest.mark.parametrize('n', [50, 100, 200])        # the tiny, the workgroup-Gram and the workgroup schedule
def test_slice_equals_the_single_device_call(engine, multis, n, nb, nranks):
  X, Y, specs, _, means, noises = _se_problem(n)
  _assert_slices_equal_single_device(engine, multis(nranks), specs[:nb], X, Y, means[:nb], noises[:nb])


@pytest.mark.parametrize('n', [50, 100, 200])
def test_whole_result_against_the_oracle(engine, multis, n):
  X, Y, specs, ospecs, means, noises = _se_problem(n)
  nb = 7
  lml = multis(3).gp_lml_batch(specs[:nb], X, Y, means[:nb], noises[:nb], spread=True)
  for c in range(nb):
    ref = O.GPOracle(X, Y, ospecs[c], means[c], noises[c]).lml()
    print(n, c, 'relerr', abs(lml[c] - ref) / abs(ref))
    assert abs(lml[c] - ref) <= TOL * abs(ref), (n, c, lml[c], ref)


def test_inputs_resident_on_every_rank(engine, multis):
  """ to_devices: one upload per rank, the list handed to the call -- same bits as host inputs """
  X, Y, specs, _, means, noises = _se_problem(200)
  mg = multis(2)
  Xs = mg.to_devices(X)
  got = mg.gp_lml_batch(specs[:7], Xs, Y, means[:7], noises[:7], spread=True)
  assert np.array_equal(got, mg.gp_lml_batch(specs[:7], X, Y, means[:7], noises[:7], spread=True))
  for a in Xs:
    a.free()


def test_fewer_candidates_than_ranks(engine, multis):
  X, Y, specs, _, means, noises = _se_problem(100)
  mg = multis(3)
  _, _, cut = _assert_slices_equal_single_device(engine, mg, specs[:2], X, Y, means[:2], noises[:2])
  assert cut == [(0, 1), (1, 2), (2, 2)]             # rank 2: the empty shard -- the library starts no thread for it


def test_per_candidate_fits_use_a_rank_each(engine, multis):
  """ n > 2047: a candidate is a full fit, so three candidates spread over two ranks without being asked to """
  from dragonfly_amd import parallel
  X, Y, specs, _, means, noises = _se_problem(2100, nb=3)
  assert parallel.lml_shard_plan(3, 2100, 2) == [(0, 2), (2, 3)]
  assert parallel.lml_shard_plan(3, 2047, 2) == [(0, 3), (3, 3)]
  _assert_slices_equal_single_device(engine, multis(2), specs, X, Y, means, noises, spread=False)


def _load_tool(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_additive_and_matern_descriptors(engine, multis):
  from dragonfly_amd.engine import KernelSpec
  g = load_golden('gp_additive_d10_n80')
  X, Y = g['X'], g['Y']
  rs = np.random.RandomState(12)
  groups = [[2 * i, 2 * i + 1] for i in range(5)]
  specs, means, noises = [], [], []
  for c in range(7):
    if c % 2 == 0:
      specs.append(KernelSpec('additive', 10, float(0.5 + rs.rand()), groups=groups, sub_kinds=['se'] * 5, sub_scales=[1.0] * 5,
                              sub_nus=[0.0] * 5, sub_bandwidths=[0.3 + 0.6 * rs.rand(2) for _ in range(5)]))
    else:
      specs.append(KernelSpec('matern', 10, float(0.5 + rs.rand()), 0.5 + rs.rand(10), nu=2.5))
    means.append(float(0.1 * rs.randn()))
    noises.append(float(Y.var() * np.exp(rs.uniform(np.log(0.01), np.log(0.2)))))
  _assert_slices_equal_single_device(engine, multis(3), specs, X, Y, means, noises)


def test_cp_product_descriptor_with_project_first(engine, multis):
  """ the candidates the reference's 'rand' tuner asked for on the mixed domain (tests/golden/cp_fitter_mixed_n60.npz):
      every candidate is a projected fit of its own, on whichever rank holds it """
  from dragonfly_amd import kernel as K
  gold = load_golden('cp_fitter_mixed_n60')
  X, Y = _load_tool('make_cp_golden').fitter_data()
  cands = gold['rand_cands'][:7]

  def kernel_of(c):
    w = c[8:11]
    return K.CartesianProductKernel(np.exp(c[2]), [K.MaternKernel(3, 2.5, 1.0, np.exp(c[3:6])), K.MaternKernel(2, 2.5, 1.0, np.exp(c[6:8])),
                                                   K.HammingKernel(w / w.sum())])
  kerns = [kernel_of(c) for c in cands]
  P = kerns[0].pack(X)
  lml, _, _ = _assert_slices_equal_single_device(engine, multis(3), [k.to_spec() for k in kerns], P, np.asarray(Y), list(cands[:, 0]),
                                                 list(np.exp(cands[:, 1])), handle_non_psd_kernels='project_first')
  assert np.max(np.abs(lml - gold['rand_lmls'][:7])) <= TOL * np.max(np.abs(gold['rand_lmls'][:7]))


def _singular_problem():
  """ duplicated rows and, for ONE candidate, no noise: only that candidate's matrix is numerically singular """
  from dragonfly_amd.engine import KernelSpec
  n, d = 200, 2
  rs = np.random.RandomState(31)
  X = rs.rand(n, d)
  X[100:] = X[:100]
  Y = np.cos(3 * X[:, 0]) + X[:, 1]
  good = [KernelSpec('se', d, 1.0, np.full(d, b)) for b in (0.3, 0.5, 0.4, 0.6, 0.35, 0.45)]
  bad = KernelSpec('se', d, 1.0, np.full(d, 2.0))
  return X, Y, good, bad


def test_jitter_ladder_in_a_later_shard(engine, multis):
  X, Y, good, bad = _singular_problem()
  specs, noises = good + [bad], [1e-3] * 6 + [0.0]            # 7 candidates on 3 ranks: [0, 3) [3, 6) [6, 7)
  _, powers, cut = _assert_slices_equal_single_device(engine, multis(3), specs, X, Y, [0.0] * 7, noises)
  assert cut[2] == (6, 7)
  assert powers[6] is not None and powers[:6] == [None] * 6
  assert powers[6] == O.GPOracle(X, Y, O.KernelSpec('se', 2, 1.0, np.full(2, 2.0)), 0.0, 0.0).jitter_power


def test_failure_in_the_middle_shard_leaves_nothing_behind(engine, multis):
  """ a clean non-PD status from the middle one of three shards: the exception is the single-device call's, every rank
      has finished, and the same MultiEngine goes on giving the right values """
  X, Y, good, bad = _singular_problem()
  specs, noises = good[:4] + [bad] + good[4:], [1e-3] * 4 + [0.0] + [1e-3] * 2       # candidate 4 lies in [3, 6)
  mg = multis(3)
  with pytest.raises(np.linalg.LinAlgError):
    engine.gp_lml_batch(specs[3:6], X, Y, [0.0] * 3, noises[3:6], allow_jitter=False)
  with pytest.raises(np.linalg.LinAlgError):
    mg.gp_lml_batch(specs, X, Y, [0.0] * 7, noises, allow_jitter=False, spread=True)
  mg.sync()                                              # nothing in flight on any rank
  _assert_slices_equal_single_device(engine, mg, good, X, Y, [0.0] * 6, [1e-3] * 6)
  _assert_slices_equal_single_device(engine, mg, specs, X, Y, [0.0] * 7, noises)        # with the ladder: fine again


def test_process_per_gpu_form_is_the_identity_without_a_communicator(engine):
  from dragonfly_amd import parallel
  X, Y, specs, _, means, noises = _se_problem(100)
  got = parallel.sharded_gp_lml_batch(engine, specs[:7], X, Y, means[:7], noises[:7])
  assert np.array_equal(got, engine.gp_lml_batch(specs[:7], X, Y, means[:7], noises[:7]))


def test_fitter_end_to_end(engine, multis):
  """ the stand-alone fitter's 'rand' tuner, 600 candidates (more than fill one device: the plan cuts them over the
      two ranks): the same hyper-parameters win as with tuning_gpus=None, on the same seed """
  from dragonfly_amd import parallel
  from dragonfly_amd.euclidean_gp import EuclideanGPFitter
  g = load_golden('fitter_d3_n45')
  mg = multis(2)
  calls = []
  real = mg.gp_lml_batch
  mg.gp_lml_batch = lambda specs, *a, **k: (calls.append(len(specs)), real(specs, *a, **k))[1]
  parallel.set_tuning_engine(mg)
  out = []
  try:
    for gpus in (2, None):
      opts = Namespace(kernel_type='se', ml_hp_tune_opt='rand', hp_tune_max_evals=600, hp_tune_criterion='ml')
      np.random.seed(4242)
      fitter = EuclideanGPFitter(list(g['X']), list(g['Y']), options=opts, tuning_gpus=gpus)
      _, gp, hps = fitter.fit_gp()
      out.append((np.array(hps[0], dtype=float), list(hps[1]), gp.compute_log_marginal_likelihood()))
      assert calls == [600]                              # the multi route ran for tuning_gpus=2, and only then
  finally:
    parallel.set_tuning_engine(None, size=2)
    del mg.gp_lml_batch
  assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
  assert abs(out[0][2] - out[1][2]) <= 1e-12 * abs(out[1][2])
