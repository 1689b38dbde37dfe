"""CPU plumbing of the ESP kernel above the C-ABI, on the engine's CPU stand-in (tests/oracle_engine_esp.py):
 - the stand-alone EuclideanGPFitter with kernel_type='esp' chooses what the reference's fitter chose
   (tests/golden/esp_fitter_d4_n30.npz: se / matern members, tuned and fixed order, ML by 'rand' and 'pdoo',
   posterior sampling), hyper-parameters, order and nu alike;
 - the reference's ask/tell bandit with kernel_type='esp' recommends the same points with dragonfly_amd.install()
   as without it (needs the reference tree)."""
import os
import warnings

import numpy as np
import pytest

from conftest import load_golden
from esp_fitter_replay import CASE_NAMES, check_case

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
HAVE_REF = os.path.isdir(os.path.join(REF, 'dragonfly'))


@pytest.mark.parametrize('name', CASE_NAMES)
def test_standalone_fitter_reproduces_the_reference_choice(name, monkeypatch):
  from oracle_engine_esp import patch_engine_esp
  patch_engine_esp(monkeypatch)
  check_case(name, load_golden('esp_fitter_d4_n30'), 1e-12)


def _ask(options_update, num_asks=2):
  """ tell 40 evaluations of a 4-D function, then ask; the recommended points and the GP's hyper-parameters """
  from dragonfly.opt import gp_bandit
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.exd.experiment_caller import EuclideanFunctionCaller
  from dragonfly.utils.option_handler import load_options
  opts = load_options(gp_bandit.get_all_euc_gp_bandit_args())
  opts.gpb_hp_tune_criterion = 'ml'
  opts.hp_tune_max_evals = 20
  opts.kernel_type = 'esp'
  for k, v in options_update.items():
    setattr(opts, k, v)
  np.random.seed(2016)
  caller = EuclideanFunctionCaller(None, EuclideanDomain([[0, 1]] * 4))
  opt = gp_bandit.EuclideanGPBandit(caller, ask_tell_mode=True, options=opts, reporter='silent')
  opt.initialise()
  rs = np.random.RandomState(7)
  X = rs.random_sample((40, 4))
  opt.tell([(x, float(np.sin(3 * x.sum()))) for x in X])
  opt.first_qinfos = []
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    points = [np.array(opt.ask()) for _ in range(num_asks)]
  kern = opt.gp.kernel
  hps = (kern.hyperparams['scale'], int(kern.hyperparams['order']), opt.gp.noise_var,
         [float(np.ravel(k.hyperparams['dim_bandwidths'])[0]) for k in kern.kernel_list],
         [k.hyperparams.get('nu') for k in kern.kernel_list], type(opt.gp).__module__, type(kern).__module__)
  return points, hps


BANDIT_CONFIGS = [
  dict(acq='ucb', acq_opt_method='rand', acq_opt_max_evals=200, gpb_ml_hp_tune_opt='rand'),
  dict(acq='ei', acq_opt_method='rand', acq_opt_max_evals=200, gpb_ml_hp_tune_opt='rand'),
  dict(acq='ei', esp_kernel_type='matern', acq_opt_method='rand', acq_opt_max_evals=200, gpb_ml_hp_tune_opt='rand'),
  dict(acq='ucb', acq_opt_method='pdoo', acq_opt_max_evals=100, gpb_ml_hp_tune_opt='pdoo'),
  dict(acq='add_ucb', acq_opt_method='rand', acq_opt_max_evals=200, gpb_ml_hp_tune_opt='rand'),
  dict(acq='ucb', acq_opt_method='rand', acq_opt_max_evals=200, gpb_hp_tune_criterion='ml-post_sampling',
       gpb_ml_hp_tune_opt='rand', gpb_post_hp_tune_burn=8),
]


@pytest.mark.skipif(not HAVE_REF, reason='needs the reference tree (build container only)')
@pytest.mark.parametrize('cfg', BANDIT_CONFIGS, ids=['%s-%s-%d' % (c['acq'], c.get('esp_kernel_type', 'se'), i)
                                                     for i, c in enumerate(BANDIT_CONFIGS)])
def test_reference_bandit_with_esp_recommends_the_same_points_installed(cfg, monkeypatch):
  from oracle.make_golden import import_reference
  import_reference()
  from oracle_engine_esp import patch_engine_esp
  from dragonfly_amd import install
  want_points, want_hps = _ask(cfg)
  assert want_hps[5].startswith('dragonfly.') and want_hps[6].startswith('dragonfly.')
  eng = patch_engine_esp(monkeypatch)
  eng.lml_batch_sizes = []
  install.install()
  try:
    got_points, got_hps = _ask(cfg)
  finally:
    install.uninstall()
  # the bandit's GP and its ESP kernel are the mirrors, and the fitter tuned in batches
  assert got_hps[5].startswith('dragonfly_amd.') and got_hps[6].startswith('dragonfly_amd.')
  assert len(eng.lml_batch_sizes) > 0 and max(eng.lml_batch_sizes) >= 3
  assert got_hps[:5] == want_hps[:5], (got_hps[:5], want_hps[:5])
  for got, want in zip(got_points, want_points):
    assert np.array_equal(got, want)
