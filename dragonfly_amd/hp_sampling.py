"""Posterior sampling of GP hyper-parameters: the 'post_sampling' tuning criterion stand-alone.

Host-side mirror of dragonfly/gp/gp_core.py:476-487 (set-up: uniform priors over the continuous
hyper-parameter boxes, equal-weight categorical priors over the discrete ones) and :592-726 (the
sampler: every hyper-parameter in turn, in a random order -- continuous ones by univariate slice
sampling, discrete ones by a Metropolis walk on the category index, the additive grouping by a
Metropolis walk on a permutation seed).  The target density is the reference's `_logp`: the log
priors of ALL hyper-parameters summed in index order plus the log marginal likelihood of the GP
(dragonfly/gp/gp_core.py:597-622); priors as in dragonfly/distributions/continuous.py:108-153 and
discrete.py:107-160; the Metropolis step as in dragonfly/sampling/metropolis.py:79-215, 218-299
(normal proposal of unit scale rounded to an integer step, scale tuned every 100 steps).

What is different is where the time goes: every density value is a GP fit, and here the fits go to
the device in batches -- the slice sampler through dragonfly_amd.slice_sampler (the points its
loops will visit, evaluated a few at a time), a Metropolis step's two densities (proposal and
current point: the reference evaluates both, every step) in one call.  The random numbers are
drawn by the same calls in the same order, so a seeded run yields the reference's samples
(tests/test_post_sampling_cpu.py against fixtures from the real fitter).
"""
from argparse import Namespace

import numpy as np
import numpy.random as nr

from .slice_sampler import SpeculativeSlice


class UniformPrior(object):
  """ continuous.py:108-153 -- what the sampler uses of it """

  def __init__(self, lower, upper):
    self.lower, self.upper = float(lower), float(upper)

  def logp(self, x):
    if x < self.lower or x > self.upper:
      return -np.inf
    return -np.log(self.upper - self.lower)

  def get_mean(self):
    return (self.lower + self.upper) / 2


class CategoricalPrior(object):
  """ discrete.py:107-160 -- what the sampler uses of it """

  def __init__(self, categories, p):
    self.cat = list(categories)
    self.k = len(self.cat)
    self.p = np.array(p)

  def draw_random(self, size=None):
    samples = nr.multinomial(1, self.p, size)
    return np.argmax(samples, len(samples.shape) - 1)

  def get_category(self, i):
    if i < 0 or i >= self.k:
      return None
    return self.cat[int(i)]

  def get_id(self, category):
    if category is None or np.isnan(category):
      return -1
    return self.cat.index(category)

  def logp(self, value):
    if value < 0 or value >= self.k:
      return -np.inf
    return np.log(self.p[value])


def _tune_scale(scale, acc_rate):
  """ metropolis.py:243-281 """
  if acc_rate < 0.001:
    return scale * 0.1
  if acc_rate < 0.05:
    return scale * 0.5
  if acc_rate < 0.2:
    return scale * 0.9
  if acc_rate > 0.95:
    return scale * 10.0
  if acc_rate > 0.75:
    return scale * 2.0
  if acc_rate > 0.5:
    return scale * 1.1
  return scale


def metropolis_integer_walk(logp_pair, q0, num_samples, tune_interval=100):
  """ Metropolis(model, discrete=True) of metropolis.py for a one-dimensional integer state:
      `logp_pair(q, q0) -> (log p(q), log p(q0))` -- the reference evaluates both densities at every
      step; here they come from one call.  Returns [num_samples x 1] like the reference. """
  if num_samples is None:
    num_samples = 1
  q0 = np.array([q0]) if not hasattr(q0, '__len__') else np.asarray(q0)
  scaling = np.atleast_1d(1.).astype('d')
  unit = np.ones(1)
  steps_until_tune, accepted = tune_interval, 0
  samples = np.zeros([num_samples, len(q0)])
  for i in range(num_samples):
    if not steps_until_tune:
      scaling = _tune_scale(scaling, accepted / float(tune_interval))
      steps_until_tune, accepted = tune_interval, 0
    delta = np.round(nr.normal(scale=unit) * scaling, 0).astype('int64')
    q0 = q0.astype('int64')
    q = (q0 + delta).astype('int64')
    lq, lq0 = logp_pair(q, q0)
    rate = min(1, np.exp(lq - lq0))
    if np.isfinite(rate) and nr.uniform() < rate:        # (the uniform is drawn only for a finite rate)
      q0 = q
      accepted += 1
    steps_until_tune -= 1
    samples[i] = q0
    q0 = samples[i]
  return samples


class PosteriorHPSampler(object):
  """ The state machine of gp_core.py:592-726 over a fitter that offers
        cts_hp_bounds, dscr_hp_vals, param_order, num_hps, options (post_hp_tune_*),
        lml_batch(cts_list, dscr_list, other_gp_params) -> log marginal likelihoods,
      and, for additive models, add_dim / add_max_group_size.  `sample(num_samples)` returns
      (cts_hps [num x n_cts], dscr_hps [num x n_dscr], other_gp_params [num]).
      tuning_gpus (not None): handed to the fitter, whose lml_batch decides per batch where it runs
      (parallel.tuning_route); a sampler's batches of a few candidates stay on the fitter's one engine. """

  def __init__(self, fitter, add_dim=None, add_max_group_size=None, tuning_gpus=None):
    self.f = fitter
    if tuning_gpus is not None:
      fitter.tuning_gpus = tuning_gpus
    self.num_cts = len(fitter.cts_hp_bounds)
    self.priors = [UniformPrior(b[0], b[-1]) for b in fitter.cts_hp_bounds] + \
                  [CategoricalPrior(v, np.repeat(1.0 / len(v), len(v))) for v in fitter.dscr_hp_vals]
    self.num_hps = len(self.priors)
    self.add_dim, self.add_max_group_size = add_dim, add_max_group_size
    self.hps = None
    self.other_gp_params = None
    self.curr_hp = None
    self.parameter = None
    self.group_size = None

  # -- the density ---------------------------------------------------------------------------------
  def _log_prior(self, hps):
    lp = 0
    for i, prior in enumerate(self.priors):
      if isinstance(prior, CategoricalPrior):
        lp += prior.logp(prior.get_id(hps[i]))
      else:
        lp += prior.logp(hps[i])
    return lp

  def _with_value(self, x):
    """ The hyper-parameter vector (and grouping) `_logp` evaluates at value x of the current
        coordinate; None when the value lies outside the prior's support before any fit. """
    hps = np.array(self.hps, dtype=np.float64)
    other = self.other_gp_params
    if self.parameter == 'additive_grp':
      if x < 0:
        return None, None
      order = list(np.random.RandomState(seed=int(np.ravel(x)[0])).permutation(self.add_dim))
      other = Namespace(add_gp_groupings=[order[i:i + self.group_size] for i in range(0, self.add_dim, self.group_size)])
    elif isinstance(self.priors[self.curr_hp], CategoricalPrior):
      cat = self.priors[self.curr_hp].get_category(np.asarray(x).item())
      hps[self.curr_hp] = np.nan if cat is None else cat
    else:
      hps[self.curr_hp] = x
    return hps, other

  def logp_batch(self, xs):
    """ log density at every value in xs of the current coordinate, the others as they are: the
        fits of all values with a finite prior go to the device in one call. """
    out = np.empty(len(xs))
    pending = []
    for k, x in enumerate(xs):
      hps, other = self._with_value(x)
      lp = -np.inf if hps is None else self._log_prior(hps)
      if not np.isfinite(lp):
        out[k] = lp
      else:
        pending.append((k, lp, hps, other))
    if pending:
      if self.parameter == 'additive_grp':          # one grouping per value: one call each
        lmls = [self.f.lml_batch([h[:self.num_cts]], [list(h[self.num_cts:self.num_hps])], o)[0] for _, _, h, o in pending]
      else:
        lmls = self.f.lml_batch([h[:self.num_cts] for _, _, h, _ in pending],
                                [list(h[self.num_cts:self.num_hps]) for _, _, h, _ in pending], self.other_gp_params)
      for (k, lp, _, _), lml in zip(pending, lmls):
        out[k] = lp + lml
    return out

  def _logp_pair(self, q, q0):
    vals = self.logp_batch([q, q0])
    return vals[0], vals[1]

  # -- the sampler ---------------------------------------------------------------------------------
  def sample(self, num_samples):
    opts = self.f.options
    if opts.post_hp_tune_method != 'slice':
      raise NotImplementedError('post_hp_tune_method=%s: only the slice sampler runs stand-alone.  The gradient of '
                                'the marginal likelihood exists (GP.compute_grad_log_marginal_likelihood); a NUTS sampler '
                                'does not: use dragonfly_amd.install with a real Dragonfly.' % (opts.post_hp_tune_method))
    offset = opts.post_hp_tune_offset
    num_dscr = self.num_hps - self.num_cts
    total = (num_samples - 1) * offset + 1
    cts = np.zeros([total, self.num_cts])
    dscr = np.zeros([total, num_dscr])
    others = [None] * total
    burn = int(np.sqrt(self.num_hps) * 100) if opts.post_hp_tune_burn == -1 else opts.post_hp_tune_burn
    # starting point: prior means, one random category each (gp_core.py:661-667)
    self.hps = np.ones((self.num_hps,))
    for i in range(self.num_cts):
      self.hps[i] = self.priors[i].get_mean()
    for i in range(self.num_cts, self.num_hps):
      self.hps[i] = self.priors[i].get_category(int(np.ravel(self.priors[i].draw_random(1))[0]))
    additive = self.add_dim is not None
    if additive:
      order = list(nr.permutation(self.add_dim))
      size0 = int(self.hps[-1])
      self.other_gp_params = Namespace(add_gp_groupings=[order[i:i + size0] for i in range(0, self.add_dim, size0)])
    else:
      self.other_gp_params = Namespace(add_gp_groupings=None)
    visit = list(range(self.num_hps))
    nr.shuffle(visit)
    for i in visit:
      self.curr_hp = i
      self.parameter = self.f.param_order[i][0]
      j = i - self.num_cts
      if self.f.param_order[i][-1] == 'cts':
        chain = SpeculativeSlice(self.logp_batch).sample(self.hps[i], total, burn)
        cts[:, i] = np.squeeze(chain, axis=1)
        self.hps[i] = cts[0, i]
      elif self.parameter != 'additive_grp':
        prior = self.priors[i]
        walk = np.squeeze(metropolis_integer_walk(self._logp_pair, prior.get_id(self.hps[i]), total), axis=1)
        for t, val in enumerate(walk):
          dscr[t, j] = prior.get_category(int(val))
        self.hps[i] = dscr[0, j]
      else:
        dscr[:, j] = nr.randint(1, self.add_max_group_size + 1, total)
        seed = int(nr.randint(self.add_dim))
        for t in range(total):
          self.group_size = int(dscr[t, j])
          seed = int(np.ravel(metropolis_integer_walk(self._logp_pair, seed, 1))[0])
          order = list(np.random.RandomState(seed=seed).permutation(self.add_dim))
          others[t] = Namespace(add_gp_groupings=[order[k:k + self.group_size]
                                                  for k in range(0, self.add_dim, self.group_size)])
        self.other_gp_params = others[0]
    pick = [t * offset for t in range(num_samples)]
    return cts[pick, :], dscr[pick, :], [others[t] for t in pick]
