"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

The runs of the reference's CPGPBandit that tests/test_cp_acq_cpu.py makes twice -- as it is, and with
dragonfly_amd.install(cartesian_product=True, cp_acquisitions=True) on the engine's stand-in -- and compares point for
point.  Needs the reference importable (oracle.make_golden.import_reference)."""
import warnings

import numpy as np

MIXED = [{'name': 'x', 'type': 'float', 'min': 0, 'max': 1, 'dim': 2},
         {'name': 'k', 'type': 'int', 'min': 1, 'max': 5},
         {'name': 'c', 'type': 'discrete', 'items': ['a', 'b', 'c']},
         {'name': 'e', 'type': 'discrete', 'items': ['u', 'v']}]
# two Euclidean parts (dimensions 2 and 1): variables of one type and kernel are grouped into one part, so the second
# part gets a kernel of its own
FLOATS = [{'name': 'x', 'type': 'float', 'min': 0, 'max': 1, 'dim': 2},
          {'name': 'z', 'type': 'float', 'min': -1, 'max': 2, 'kernel': 'matern'}]


def mixed_objective(p):
  x, k, c, e = p
  return -float(np.sum((np.asarray(x) - 0.4) ** 2)) - 0.1 * (k - 3) ** 2 + {'a': 0.0, 'b': 0.3, 'c': -0.2}[c] + 0.1 * (e == 'u')


def floats_objective(p):
  x, z = p
  return -float(np.sum((np.asarray(x) - 0.3) ** 2)) - 0.5 * (float(np.ravel(z)[0]) - 0.7) ** 2


CASES = [
  dict(id='mixed-rand-ucb', domain=MIXED, acq='ucb', acq_opt_method='rand', workers=1),
  dict(id='mixed-rand-ei', domain=MIXED, acq='ei', acq_opt_method='rand', workers=1),
  dict(id='mixed-rand-ttei', domain=MIXED, acq='ttei', acq_opt_method='rand', workers=1),
  dict(id='mixed-rand-ts', domain=MIXED, acq='ts', acq_opt_method='rand', workers=1),
  dict(id='mixed-ts-halluc-3-workers', domain=MIXED, acq='ts', acq_opt_method='rand', workers=3, capital=9),
  dict(id='mixed-syn-ts-3-workers', domain=MIXED, acq='ts', acq_opt_method='rand', workers=3, capital=9, mode='syn'),
  dict(id='floats-default', domain=FLOATS, acq='ucb', acq_opt_method='default', workers=1),
  dict(id='floats-pdoo', domain=FLOATS, acq='ei', acq_opt_method='pdoo', workers=1),
]
NUM_EVALS = 12


def load(domain_vars):
  from dragonfly import load_config
  return load_config({'domain': domain_vars})


def bandit_options(case, seed=11):
  from dragonfly.opt.gp_bandit import get_all_cp_gp_bandit_args
  from dragonfly.utils.option_handler import load_options
  from dragonfly.utils.reporters import get_reporter
  np.random.seed(seed)
  options = load_options(get_all_cp_gp_bandit_args(), reporter=get_reporter('silent'))
  options.acq = case['acq']
  options.acq_opt_method = case['acq_opt_method']
  options.acq_opt_max_evals = 60
  options.gpb_hp_tune_criterion = 'ml'
  options.gpb_ml_hp_tune_opt = 'rand'
  options.gpb_hp_tune_max_evals = 20
  options.handle_parallel = 'halluc'
  options.mode = case.get('mode', 'asy')
  return options


def ask_tell_bandit(case, seed=11):
  from dragonfly.exd.experiment_caller import CPFunctionCaller
  from dragonfly.opt.gp_bandit import CPGPBandit
  from dragonfly.utils.reporters import get_reporter
  config = load(case['domain'])
  options = bandit_options(case, seed)
  caller = CPFunctionCaller(None, config.domain, domain_orderings=config.domain_orderings)
  opt = CPGPBandit(caller, ask_tell_mode=True, options=options, reporter=get_reporter('silent'))
  opt.initialise()
  return opt


def fitted_bandit(case, num_evals=8, seed=11):
  """ the bandit after num_evals ask / tell rounds: opt.gp is the GP its fitter built for the last ask """
  objective = mixed_objective if case['domain'] is MIXED else floats_objective
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    opt = ask_tell_bandit(case, seed)
    for _ in range(num_evals):
      pt = opt.ask()
      opt.tell([(pt, objective(pt))])
  return opt


def run_case(case, seed=11):
  """ NUM_EVALS evaluations of the reference's CPGPBandit from a fixed seed; returns the queried points as text (the
      points are lists of arrays, numbers and strings).  One worker: ask / tell.  Several: the bandit's own loop over a
      synthetic worker manager, which is where evaluations are in progress while the next point is chosen.  Its capital
      is spent per worker and its initial design is 15 points, so case['capital'] = 9 gives 28 evaluations: NUM_EVALS
      model-based ones (and the one in flight at the end) after the design. """
  from dragonfly import maximise_function
  from dragonfly.utils.reporters import get_reporter
  objective = mixed_objective if case['domain'] is MIXED else floats_objective
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    if case['workers'] > 1:
      config = load(case['domain'])
      options = bandit_options(case, seed)
      _, _, hist = maximise_function(objective, config.domain, case['capital'], num_workers=case['workers'], config=config,
                                     options=options, reporter=get_reporter('silent'))
      return [repr(pt) for pt in hist.query_points]
    opt = ask_tell_bandit(case, seed)
    points = []
    for _ in range(NUM_EVALS):
      pt = opt.ask()
      points.append(repr(pt))
      opt.tell([(pt, objective(pt))])
  return points
