"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

What tests/test_cpmf_cpu.py and tests/test_gpu_cpmf.py share: the structure of the fixtures tools/record_cpmf_golden.py
records (read from the tool itself), the nested product descriptor and the mirror kernel of a fixture, its packed rows
as the reference's list-of-lists points, BOCA's fidelity rule on recorded numbers, and the multi-fidelity bandit runs on
a Cartesian-product domain that the CPU test makes twice."""
import importlib.util
import os
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TOOL = []


def tool():
  if not _TOOL:
    spec = importlib.util.spec_from_file_location('record_cpmf_golden', os.path.join(ROOT, 'tools', 'record_cpmf_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _TOOL.append(mod)
  return _TOOL[0]


def parts_of(name, g):
  """ [(space index, kind, columns of the packed pair, parameters, nu)] of a fixture, fidelity space first """
  fx = tool().FIXTURES[name]
  out, at = [], 0
  for f, space in enumerate(('fidel', 'domain')):
    for j, part in enumerate(fx[space]):
      out.append((f, part[0], list(range(at, at + part[1])), np.asarray(g['%s_par_%d' % (space, j)], dtype=float),
                  part[3] if part[0] == 'matern' else 0.0))
      at += part[1]
  return out


def fidel_width(name):
  return sum(part[1] for part in tool().FIXTURES[name]['fidel'])


def spec_of(name, g):
  """ the fixture's kernel as ONE product descriptor with two product factors """
  from dragonfly_amd.engine import KernelSpec
  parts = parts_of(name, g)
  dim = parts[-1][2][-1] + 1
  return KernelSpec('product', dim, float(g['kernel_scale']), groups=[p[2] for p in parts], sub_kinds=[p[1] for p in parts],
                    sub_scales=[1.0] * len(parts), sub_nus=[p[4] for p in parts], sub_bandwidths=[p[3] for p in parts],
                    group_factors=[p[0] for p in parts], factor_sums=[2, 2],
                    factor_scales=[float(g['fidel_scale']), float(g['domain_scale'])])


def mirror_kernels(name, g):
  """ (fidelity-space kernel, domain kernel) of the fixture as dragonfly_amd.kernel mirrors """
  from dragonfly_amd import kernel as K
  out = []
  for f, scale in enumerate((float(g['fidel_scale']), float(g['domain_scale']))):
    members = []
    for pf, kind, cols, par, nu in parts_of(name, g):
      if pf != f:
        continue
      members.append(K.SEKernel(len(cols), 1.0, par) if kind == 'se' else
                     K.MaternKernel(len(cols), nu, 1.0, par) if kind == 'matern' else K.HammingKernel(par))
    out.append(K.CartesianProductKernel(scale, members))
  return out


def unpack(name, P, space):
  """ packed rows of one space ('fidel' | 'domain') as lists of per-part lists, categories as ints """
  fx = tool().FIXTURES[name]
  pts = []
  for row in np.atleast_2d(P):
    at, pt = 0, []
    for part in fx[space]:
      block = row[at:at + part[1]]
      pt.append([int(v) for v in block] if part[0] == 'hamming' else block.copy())
      at += part[1]
    pts.append(pt)
  return pts


def unpack_pairs(name, P):
  w = fidel_width(name)
  P = np.atleast_2d(P)
  return list(zip(unpack(name, P[:, :w], 'fidel'), unpack(name, P[:, w:], 'domain')))


def boca_fidelity(g, stds_over_root_scale, max_ratio=0.9):
  """ opt/gpb_acquisitions.py:419-438 on the recorded cost ratios and thresholds: the index of the chosen candidate
      fidelity, -1 for fidel_to_opt """
  cost_ratios = np.asarray(g['cost_ratios'])
  qualifying = np.where(np.asarray(stds_over_root_scale) > np.asarray(g['thresholds']))[0]
  if len(qualifying) == 0:
    return -1
  best = qualifying[int(np.sqrt(cost_ratios)[qualifying].argmin())]
  return -1 if cost_ratios[best] > max_ratio else int(best)


# ---- the reference's multi-fidelity bandit on a product domain, for the run made twice ---------------------------------
CONFIG = {'domain': [{'name': 'x', 'type': 'float', 'min': 0, 'max': 1, 'dim': 2},
                     {'name': 'k', 'type': 'int', 'min': 1, 'max': 5},
                     {'name': 'c', 'type': 'discrete', 'items': ['a', 'b', 'c']}],
          'fidel_space': [{'name': 'f', 'type': 'float', 'min': 0, 'max': 1},
                          {'name': 'g', 'type': 'discrete', 'items': ['lo', 'hi']}],
          'fidel_to_opt': [0.9, 'hi']}


def mf_objective(z, p):
  x, k, c = p
  fz, grade = z
  return -float(np.sum((np.asarray(x) - 0.4) ** 2)) - 0.1 * (k - 3) ** 2 + {'a': 0.0, 'b': 0.3, 'c': -0.2}[c] \
         - 0.3 * (1 - float(np.ravel(fz)[0])) ** 2 - 0.05 * (grade == 'lo')


def mf_cost(z):
  fz, grade = z
  return 0.2 + float(np.ravel(fz)[0]) ** 2 + 0.3 * (grade == 'hi')


def mf_options(acq):
  from dragonfly.opt.gp_bandit import get_all_mf_cp_gp_bandit_args
  from dragonfly.utils.option_handler import load_options
  from dragonfly.utils.reporters import get_reporter
  options = load_options(get_all_mf_cp_gp_bandit_args(), reporter=get_reporter('silent'))
  options.acq = acq
  options.acq_opt_method = 'rand'
  options.acq_opt_max_evals = 60
  options.gpb_hp_tune_criterion = 'ml'
  options.gpb_ml_hp_tune_opt = 'rand'
  options.gpb_hp_tune_max_evals = 20
  return options


def run_mf_bandit(acq, capital=12, seed=5):
  """ the reference's CPGPBandit(is_mf=True) through maximise_multifidelity_function; returns the queried
      (fidelity, point) sequence and the optimum as text """
  from dragonfly import load_config, maximise_multifidelity_function
  from dragonfly.utils.reporters import get_reporter
  np.random.seed(seed)
  config = load_config(CONFIG)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    val, pt, hist = maximise_multifidelity_function(mf_objective, None, None, None, mf_cost, capital, config=config,
                                                    options=mf_options(acq), reporter=get_reporter('silent'))
  return repr(val), repr(pt), [repr(z) for z in hist.query_fidels], [repr(x) for x in hist.query_points]
