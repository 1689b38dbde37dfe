"""MI355X: dfh_mgpu_ts_halluc / dfh_mgpu_acq_argmax_halluc -- the multi-GPU Thompson step and fused acquisitions with
evaluations in progress -- on the one device of a test box (the library's duplicate-device test mode, as
tests/test_gpu_mgpu.py sets it up): N contexts and host threads, results equal to the single-context calls
(dfh_gp_draw with S = 1, dfh_gp_acq_argmax with Xh) on the concatenated candidates, bit for bit."""
import numpy as np
import pytest

from dragonfly_amd import parallel
from dragonfly_amd.engine import KernelSpec

import draw_cases as D

pytestmark = pytest.mark.gpu
BLOCK = 128


@pytest.mark.parametrize('nranks,m', [(2, 3 * BLOCK + 44), (4, 3 * BLOCK - 40)])      # (4 ranks, 3 blocks: one shard is empty)
@pytest.mark.parametrize('q', [0, 3])
def test_sharded_calls_with_points_in_progress_equal_the_single_context_calls(engine, nranks, m, q, monkeypatch):
  monkeypatch.setenv('DFH_MGPU_ALLOW_DUPLICATE_DEVICES', '1')
  p = D.problem('m25')
  spec = KernelSpec('matern', D.DIM, p['scale'], p['bw'], nu=2.5)
  yc, mean, noise = p['Y'] - p['mean'], p['mean'], p['noise']
  rs = np.random.RandomState(500 + 10 * nranks + q)
  cands, Xh, U = rs.random_sample((m, D.DIM)), rs.random_sample((q, D.DIM)), rs.standard_normal(m)
  cands[7], cands[150] = cands[3], cands[140]      # duplicates inside the first two blocks: singular covariances
  gp = engine.gp_fit(spec, p['X'], yc, noise)
  halluc = Xh if q else None
  _, bvs, bis, want_powers = gp.draw(cands, U, num_samples=1, block=BLOCK, X_halluc=halluc, mean_const=mean, return_samples=False)
  want_ts = (float(bvs[0]), int(bis[0]))
  print('jitter powers', want_powers)
  best = float(p['Y'].max())
  want_acq = {'ucb': gp.acq_argmax('ucb', cands, params=(2.0, 0.0), mean_const=mean, X_halluc=halluc),
              'ei': gp.acq_argmax('ei', cands, params=(best, 0.0), mean_const=mean, X_halluc=halluc)}
  bounds = [parallel.shard_bounds(m, r, nranks, align=BLOCK) for r in range(nranks)]
  assert (min(hi - lo for lo, hi in bounds) == 0) == (nranks == 4)
  cs, us = [cands[lo:hi] for lo, hi in bounds], [U[lo:hi] for lo, hi in bounds]
  mg = parallel.MultiEngine(nranks, device_ids=[0] * nranks)
  try:
    assert mg.fit(spec, p['X'], yc, noise) == [gp.lml] * nranks
    bv, bi, local, powers = mg.thompson(cs, us, block=BLOCK, mean_const=mean, return_local=True, X_halluc=Xh)
    assert (bv, bi) == want_ts
    assert [pw for rank in powers for pw in rank] == want_powers
    for r, (lo, hi) in enumerate(bounds):
      if hi > lo:
        _, v, i, _ = gp.draw(cands[lo:hi], U[lo:hi], num_samples=1, block=BLOCK, X_halluc=halluc, mean_const=mean, return_samples=False)
        assert local[r] == (float(v[0]), int(i[0]) + lo), r
      else:
        assert local[r][1] == -1 and powers[r] == []
    for acq, params in (('ucb', (2.0, 0.0)), ('ei', (best, 0.0))):
      assert mg.acq_argmax(acq, cs, params=params, mean_const=mean, X_halluc=Xh) == want_acq[acq], acq
    # the prior mean as values per candidate, the points in progress resident in each rank's memory
    mvs = [np.full(hi - lo, mean) for lo, hi in bounds]
    xh_dev = [e.to_device(Xh) for e in mg.engines] if q else Xh
    assert mg.thompson(cs, us, block=BLOCK, X_halluc=xh_dev, mean_vals=mvs) == want_ts
    assert mg.acq_argmax('ei', cs, params=(best, 0.0), X_halluc=xh_dev, mean_vals=mvs) == want_acq['ei']
    if q:
      for buf in xh_dev:
        buf.free()
      # without the keyword: today's exports, which know nothing of the points in progress
      plain = gp.thompson(cands, U, block=BLOCK, mean_const=mean)
      assert mg.thompson(cs, us, block=BLOCK, mean_const=mean) == plain and plain != want_ts
  finally:
    mg.close()
    gp.free()
