"""CPU: the host side of the multi-GPU tuning batch (second half): the shard plan
(parallel.lml_shard_plan against a hand-written table and against the library's dfh_lml_shard_plan), the routing of the
fitters' batch objective with tuning_gpus (a stand-in MultiEngine over the stand-in engine of tests/oracle_engine.py),
the process-per-GPU form over a stand-in communicator, and uninstall()."""
import os
import threading
import warnings
from argparse import Namespace

import numpy as np
import pytest

from conftest import load_golden
from dragonfly_amd import _lib, parallel
from oracle_engine import OracleEngine, patch_engine

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')),
                                     reason='needs the reference tree (build container only)')

# (nb, n, world, spread) -> the cut, written out by hand from the rule: up to n = 2047 a device takes 256 candidates
# before the next one gets any; beyond, a candidate each; the ranks taking part share the batch in equal contiguous parts
PLAN_TABLE = [
  ((0, 1000, 1, False), [(0, 0)]),
  ((0, 1000, 3, False), [(0, 0), (0, 0), (0, 0)]),
  ((1, 1000, 1, False), [(0, 1)]),
  ((1, 1000, 3, False), [(0, 1), (1, 1), (1, 1)]),
  ((255, 1000, 1, False), [(0, 255)]),
  ((255, 1000, 2, False), [(0, 255), (255, 255)]),
  ((255, 1000, 3, False), [(0, 255), (255, 255), (255, 255)]),
  ((256, 1000, 1, False), [(0, 256)]),
  ((256, 1000, 2, False), [(0, 256), (256, 256)]),
  ((256, 1000, 3, False), [(0, 256), (256, 256), (256, 256)]),
  ((257, 1000, 1, False), [(0, 257)]),
  ((257, 1000, 2, False), [(0, 129), (129, 257)]),
  ((257, 1000, 3, False), [(0, 129), (129, 257), (257, 257)]),
  ((600, 1000, 2, False), [(0, 300), (300, 600)]),
  ((600, 1000, 3, False), [(0, 200), (200, 400), (400, 600)]),
  ((10000, 1000, 8, False), [(1250 * r, 1250 * (r + 1)) for r in range(8)]),
  ((3, 2047, 3, False), [(0, 3), (3, 3), (3, 3)]),
  ((3, 2048, 3, False), [(0, 1), (1, 2), (2, 3)]),
  ((3, 2048, 2, False), [(0, 2), (2, 3)]),
  ((2, 2048, 3, False), [(0, 1), (1, 2), (2, 2)]),           # nb < world
  ((2, 50, 3, True), [(0, 1), (1, 2), (2, 2)]),
  ((7, 100, 3, True), [(0, 3), (3, 6), (6, 7)]),
  ((65, 200, 2, True), [(0, 33), (33, 65)]),
  ((4, 200, 3, True), [(0, 2), (2, 4), (4, 4)]),
  ((1, 200, 3, True), [(0, 1), (1, 1), (1, 1)]),
]


@pytest.mark.parametrize('args,want', PLAN_TABLE, ids=['nb%d-n%d-w%d%s' % (a[0], a[1], a[2], '-spread' if a[3] else '') for a, _ in PLAN_TABLE])
def test_lml_shard_plan_table(args, want):
  nb, n, world, spread = args
  assert parallel.lml_shard_plan(nb, n, world, spread=spread) == want


def _library_plan(nb, n, world, spread):
  cut = np.zeros(world + 1, dtype=np.int64)
  rc = _lib.load().dfh_lml_shard_plan(nb, n, world, _lib.MGPU_LML_SPREAD if spread else 0, cut.ctypes.data_as(_lib.c_int64_p))
  assert rc == _lib.DFH_OK
  assert cut[world] == nb
  return [(int(cut[r]), int(cut[r + 1])) for r in range(world)]


def test_lml_shard_plan_is_the_librarys_and_well_formed():
  for nb in list(range(0, 12)) + [255, 256, 257, 511, 512, 513, 600, 769, 2049, 10000]:
    for n in (1, 63, 2047, 2048, 5000):
      for world in (1, 2, 3, 4, 8):
        for spread in (False, True):
          plan = parallel.lml_shard_plan(nb, n, world, spread=spread)
          assert plan == _library_plan(nb, n, world, spread), (nb, n, world, spread)
          # contiguous, covering [0, nb), non-overlapping; empty shards only at the tail
          assert len(plan) == world and plan[0][0] == 0 and plan[-1][1] == nb
          assert all(lo <= hi for lo, hi in plan) and all(plan[r][1] == plan[r + 1][0] for r in range(world - 1))
          sizes = [hi - lo for lo, hi in plan]
          used = parallel.lml_ranks_used(plan)
          assert all(s > 0 for s in sizes[:used]) and all(s == 0 for s in sizes[used:])
          if n <= 2047 and not spread and nb > 0:
            assert used == min(world, -(-nb // 256))


def test_lml_shard_plan_rejects_bad_arguments():
  for args in ((-1, 10, 2), (5, 0, 2), (5, 10, 0)):
    with pytest.raises(ValueError):
      parallel.lml_shard_plan(*args)
    cut = np.zeros(8, dtype=np.int64)
    assert _lib.load().dfh_lml_shard_plan(args[0], args[1], args[2], 0, cut.ctypes.data_as(_lib.c_int64_p)) == _lib.DFH_ERR_BAD_ARG


class StandInMultiEngine(object):
  """ parallel.MultiEngine's tuning interface over the NumPy engine: every shard of the plan is one call of it """
  made = []

  def __init__(self, n_devices, device_ids=None):
    del device_ids
    self.size, self.engine, self.calls, self.uploads, self.closed = int(n_devices), OracleEngine(), [], 0, False
    StandInMultiEngine.made.append(self)

  def to_devices(self, host):
    self.uploads += 1
    return [np.array(host, dtype=np.float64) for _ in range(self.size)]

  def gp_lml_batch(self, specs, X, y, mean_consts, noise_vars, allow_jitter=True, return_powers=False,
                   handle_non_psd_kernels='guaranteed_psd', spread=False):
    assert isinstance(X, list) and len(X) == self.size and not return_powers and handle_non_psd_kernels == 'guaranteed_psd'
    plan = parallel.lml_shard_plan(len(specs), len(X[0]), self.size, spread=spread)
    self.calls.append(plan)
    return np.concatenate([self.engine.gp_lml_batch(specs[lo:hi], X[r], y, mean_consts[lo:hi], noise_vars[lo:hi], allow_jitter)
                           for r, (lo, hi) in enumerate(plan) if hi > lo])

  def close(self):
    self.closed = True


@pytest.fixture
def stand_in_multi(monkeypatch):
  StandInMultiEngine.made = []
  monkeypatch.setattr(parallel, 'MultiEngine', StandInMultiEngine)
  yield StandInMultiEngine
  parallel.close_tuning_engines()


def _standalone_fit(tuning_gpus, evals=600):
  from dragonfly_amd.euclidean_gp import EuclideanGPFitter
  g = load_golden('fitter_d3_n45')
  opts = Namespace(kernel_type='se', ml_hp_tune_opt='rand', hp_tune_max_evals=evals, hp_tune_criterion='ml')
  np.random.seed(4242)
  fitter = EuclideanGPFitter(list(g['X']), list(g['Y']), options=opts, tuning_gpus=tuning_gpus)
  _, gp, hps = fitter.fit_gp()
  return fitter, np.array(hps[0], dtype=float), list(hps[1]), gp.compute_log_marginal_likelihood()


def test_standalone_fitter_routes_large_batches_only(monkeypatch, stand_in_multi):
  eng = patch_engine(monkeypatch)
  eng.lml_batch_sizes = []
  _, want_cts, want_dscr, want_lml = _standalone_fit(None)
  assert eng.lml_batch_sizes == [600] and stand_in_multi.made == []
  eng.lml_batch_sizes = []
  fitter, got_cts, got_dscr, got_lml = _standalone_fit(2)
  assert len(stand_in_multi.made) == 1 and stand_in_multi.made[0].size == 2
  assert stand_in_multi.made[0].calls == [[(0, 300), (300, 600)]] and stand_in_multi.made[0].uploads == 1
  assert eng.lml_batch_sizes == []                           # the 600 went nowhere else
  assert np.array_equal(got_cts, want_cts) and got_dscr == want_dscr and got_lml == want_lml
  # a handful of candidates (a slice sampler's or a tree search's call) stays on the process's engine
  cts = [np.array([b[0] + 0.3 * (b[1] - b[0]) * (k + 1) / 4 for b in fitter.cts_hp_bounds]) for k in range(4)]
  fitter.lml_batch(cts, [[]] * 4)
  assert eng.lml_batch_sizes == [4] and len(stand_in_multi.made[0].calls) == 1
  # ... and with 256 candidates, which one device holds at once, nothing is created at all
  stand_in_multi.made = []
  parallel.close_tuning_engines()
  _standalone_fit(2, evals=256)
  assert stand_in_multi.made == []


def test_sampler_keyword_reaches_the_fitter(monkeypatch):
  from dragonfly_amd.euclidean_gp import EuclideanGPFitter
  from dragonfly_amd.hp_sampling import PosteriorHPSampler
  patch_engine(monkeypatch)
  g = load_golden('fitter_d3_n45')
  fitter = EuclideanGPFitter(list(g['X']), list(g['Y']), options=Namespace(kernel_type='se', hp_tune_criterion='post_sampling'))
  assert fitter.tuning_gpus is None
  PosteriorHPSampler(fitter)
  assert fitter.tuning_gpus is None
  PosteriorHPSampler(fitter, tuning_gpus=4)
  assert fitter.tuning_gpus == 4


def _installed_fitter(monkeypatch, tuning_gpus, evals=600):
  from oracle.make_golden import import_reference
  import_reference()
  eng = patch_engine(monkeypatch)
  eng.lml_batch_sizes = []
  from dragonfly_amd import install
  install.install(tuning_gpus=tuning_gpus)
  import dragonfly.opt.gp_bandit as GB
  from dragonfly.gp.euclidean_gp import euclidean_gp_args
  from dragonfly.utils.option_handler import load_options
  rs = np.random.RandomState(3)
  X = [rs.rand(3) for _ in range(30)]
  Y = [float(np.sin(3 * x).sum() + 0.1 * rs.randn()) for x in X]
  opts = load_options(euclidean_gp_args, partial_options=dict(kernel_type='se', ml_hp_tune_opt='rand', hp_tune_max_evals=evals,
                                                              hp_tune_criterion='ml'))
  np.random.seed(99)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    fitter = GB.EuclideanGPFitter(X, Y, options=opts)
    _, gp, hps = fitter.fit_gp()
  return eng, install, fitter, (gp.kernel.hyperparams['scale'], np.asarray(gp.kernel.hyperparams['dim_bandwidths'], dtype=float),
                                gp.noise_var, np.array(hps[0], dtype=float))


@needs_reference
def test_installed_fitter_routes_a_rand_batch_through_the_multi_engine(monkeypatch, stand_in_multi):
  eng, install, _, want = _installed_fitter(monkeypatch, None)
  install.uninstall()
  assert eng.lml_batch_sizes == [600] and stand_in_multi.made == []
  eng, install, fitter, got = _installed_fitter(monkeypatch, 2)
  try:
    assert len(stand_in_multi.made) == 1                          # one MultiEngine(2), made on the first batch that needs it
    multi = stand_in_multi.made[0]
    assert multi.size == 2 and multi.calls == [[(0, 300), (300, 600)]] and eng.lml_batch_sizes == []
    # the winning hyper-parameters are those of tuning_gpus=None on the same seed
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and np.array_equal(got[3], want[3])
    # a slice sampler's batch of four never goes there
    cts = [np.array([b[0] + 0.3 * (b[1] - b[0]) * (k + 1) / 4 for b in fitter.cts_hp_bounds]) for k in range(4)]
    lmls = fitter._lml_batch(cts, [[]] * 4)      # pylint: disable=protected-access
    assert len(lmls) == 4 and eng.lml_batch_sizes == [4] and len(multi.calls) == 1
  finally:
    install.uninstall()


@needs_reference
def test_uninstall_restores_everything(monkeypatch, stand_in_multi):
  from oracle.make_golden import import_reference
  import_reference()
  import dragonfly.gp.euclidean_gp as ref_egp
  import dragonfly.opt.gp_bandit as ref_gp_bandit
  import dragonfly.opt.multiobjective_gp_bandit as ref_moo_bandit
  before = (ref_gp_bandit.EuclideanGPFitter, ref_moo_bandit.EuclideanGPFitter, ref_egp.EuclideanGP)
  _, install, _, _ = _installed_fitter(monkeypatch, 2)
  assert ref_gp_bandit.EuclideanGPFitter is not before[0] and len(stand_in_multi.made) == 1
  install.uninstall()
  assert (ref_gp_bandit.EuclideanGPFitter, ref_moo_bandit.EuclideanGPFitter, ref_egp.EuclideanGP) == before
  assert stand_in_multi.made[0].closed and parallel._tuning_engines == {}      # pylint: disable=protected-access
  # a later install without the keyword makes fitters that never ask for several GPUs
  eng, install, _, _ = _installed_fitter(monkeypatch, None)
  install.uninstall()
  assert eng.lml_batch_sizes == [600] and len(stand_in_multi.made) == 1


class ThreadComm(object):
  """ the communicator interface of parallel.RcclComm between the threads of this process """

  def __init__(self, rank, size, shared):
    self.rank, self.size, self.shared = rank, size, shared

  def allgather_rows(self, row, is_owner):
    barrier, slot = self.shared
    if is_owner:
      slot[0] = np.array(row, dtype=np.float64)
    barrier.wait()
    out = slot[0].copy()
    barrier.wait()
    return out


@pytest.mark.parametrize('world,nb,spread', [(2, 7, True), (3, 2, True), (3, 600, False), (2, 5, False)])
def test_process_per_gpu_form_gathers_every_shard_on_every_rank(world, nb, spread):
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(nb)
  X = rs.rand(12, 2)
  y = np.sin(3 * X.sum(axis=1))
  specs = [KernelSpec('se', 2, 1.0 + 0.01 * c, np.array([0.4, 0.6])) for c in range(nb)]
  means, noises = list(0.1 * rs.randn(nb)), list(0.01 + 0.05 * rs.rand(nb))
  want = OracleEngine().gp_lml_batch(specs, X, y, means, noises)
  assert np.array_equal(parallel.sharded_gp_lml_batch(OracleEngine(), specs, X, y, means, noises), want)     # comm=None
  shared = (threading.Barrier(world), [None])
  got, sizes = [None] * world, [None] * world

  def run(r):
    eng = OracleEngine()
    eng.lml_batch_sizes = []
    got[r] = parallel.sharded_gp_lml_batch(eng, specs, X, y, means, noises, comm=ThreadComm(r, world, shared), spread=spread)
    sizes[r] = sum(eng.lml_batch_sizes)
  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(60)
  assert sizes == [hi - lo for lo, hi in parallel.lml_shard_plan(nb, 12, world, spread=spread)]
  for r in range(world):
    assert np.array_equal(got[r], want), r
