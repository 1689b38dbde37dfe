"""The fitters install(batched_tuning=True) puts under the reference's bandits (seam S3 of INTEGRATION.md): subclasses
OF THE REFERENCE'S fitters that change one thing -- the maximum-likelihood tuners and the slice sampler see their
objective as a batch, candidates in, log marginal likelihoods out, one dfh_gp_lml_batch call.

A candidate becomes (kernel description, constant mean, noise variance) through the reference's own build_gp.  That
method ends in a call of the GP class by a module global looked up at call time (gp/euclidean_gp.py:338,
gp/cartesian_product_gp.py); all that is wanted of the object are three of its arguments, so for the length of the walk
the name is bound to a stand-in that keeps them and does nothing else (a GP object per candidate -- data lists copied and
checked -- was a fifth of a small run's time).  Candidates that cannot run from a description -- a user mean function, a
kernel the host evaluates -- take one fit each through the reference's _tuning_objective.
"""
import contextlib
import os

import numpy as np

from . import gaplog
from .cartesian_product_gp import runs_from_descriptor
from .kernel import CartesianProductKernel


# DFH_SLICE_MERGE=0: the speculative slice sampler's stepping-out and shrinking candidates in separate density calls again
_SLICE_MERGE_FIRST = os.environ.get('DFH_SLICE_MERGE', '1') != '0'


@contextlib.contextmanager
def bound_stand_in(ref_module, name, stand_in):
  """ The reference module's global `name` is `stand_in` inside the block, and what it was afterwards. """
  saved = getattr(ref_module, name)
  setattr(ref_module, name, stand_in)
  try:
    yield
  finally:
    setattr(ref_module, name, saved)


class _StandIn(object):
  """ What a batch needs of the GP the reference's build_gp constructs: kernel, mean function, noise variance, and
      whether the host would have to evaluate the kernel.  A subclass is one GP class's constructor signature. """
  __slots__ = ('kernel', 'mean_func', 'noise_var', 'host_kernel')

  def __init__(self, kernel, mean_func, noise_var, host_kernel, build_posterior):
    if build_posterior:
      raise RuntimeError('dragonfly_amd.install: the candidate stand-in was asked for a real GP')
    self.kernel, self.mean_func, self.noise_var, self.host_kernel = kernel, mean_func, noise_var, host_kernel


class _KernelMeanNoise(_StandIn):
  """ EuclideanGP's constructor (gp/euclidean_gp.py:151-152). """
  __slots__ = ()

  def __init__(self, X, Y, kernel, mean_func, noise_var, kernel_hyperparams=None, build_posterior=True, reporter=None):
    # pylint: disable=unused-argument
    # (gp_core.GP._generic for a plain EuclideanGP: a kernel without a device description is evaluated by the host)
    _StandIn.__init__(self, kernel, mean_func, noise_var,
                      not (hasattr(kernel, 'to_spec') and getattr(kernel, 'has_device_spec', lambda: True)()),
                      build_posterior or isinstance(kernel, str))


class _CPKernelMeanNoise(_StandIn):
  """ CPGP's constructor (gp/cartesian_product_gp.py:211-213). """
  __slots__ = ('handle_non_psd_kernels',)

  def __init__(self, X, Y, kernel, mean_func, noise_var, domain_lists_of_dists=None, build_posterior=True, reporter=None,
               handle_non_psd_kernels='project_first'):
    # pylint: disable=unused-argument
    _StandIn.__init__(self, kernel, mean_func, noise_var, not runs_from_descriptor(kernel, domain_lists_of_dists),
                      build_posterior)
    self.handle_non_psd_kernels = handle_non_psd_kernels


class _CPMFKernelMeanNoise(_StandIn):
  """ CPMFGP's constructor (gp/cartesian_product_gp.py:254-258): the joint kernel is composed as that constructor
      composes it, from our mirror. """
  __slots__ = ('handle_non_psd_kernels',)

  def __init__(self, ZZ, XX, YY, mf_kernel, mean_func, noise_var, kernel_scale=None, fidel_space_kernel=None,
               domain_kernel=None, fidel_space_lists_of_dists=None, domain_lists_of_dists=None, build_posterior=True,
               reporter=None, handle_non_psd_kernels='project_first'):
    # pylint: disable=unused-argument
    described = mf_kernel is None and isinstance(fidel_space_kernel, CartesianProductKernel) and \
                isinstance(domain_kernel, CartesianProductKernel)
    if described:
      mf_kernel = CartesianProductKernel(kernel_scale, [fidel_space_kernel, domain_kernel])
    _StandIn.__init__(self, mf_kernel, mean_func, noise_var,
                      not (described and runs_from_descriptor(mf_kernel, fidel_space_lists_of_dists, domain_lists_of_dists)),
                      build_posterior)
    self.handle_non_psd_kernels = handle_non_psd_kernels


def _per_candidate(dscr_hps):
  """ The tuners hand over the discrete hyper-parameters as one row per candidate, or as one row for all of them. """
  return len(dscr_hps) > 0 and isinstance(dscr_hps[0], (list, tuple, np.ndarray))


def _dscr_row(dscr_hps, per_cand, i):
  """ The discrete row of candidate i, a list of its own (build_gp consumes it). """
  return list(dscr_hps[i]) if per_cand else list(dscr_hps)


def _logged(lmls):
  if gaplog.ENABLED and len(lmls) >= 16:       # (a random-search batch: its arg-max is the fitter's choice)
    gaplog.top2('hp_batch', lmls)
  return lmls


def make_batched_fitter(ref_fitter_cls, tuning_gpus=None):
  """ A subclass of the reference's EuclideanGPFitter whose maximum-likelihood tuners evaluate the
      tuning objective (gp_core.py:551-564) in batches on the device.  tuning_gpus: see install(). """
  import dragonfly.gp.euclidean_gp as ref_egp
  from . import parallel
  from .doo import pdoo_maximise_batched
  from .engine import get_engine, KernelSpec
  from .gpb_acquisitions import _fortran_direct_available
  from .kernel import _as_2d_array
  from .oper_utils import random_maximise, random_sample_cts_dscr

  class BatchedEuclideanGPFitter(ref_fitter_cls):
    """ dragonfly.gp.euclidean_gp.EuclideanGPFitter with batched ML tuning (dragonfly_amd.install). """
    pdoo_frontier = 32
    # the module global build_gp constructs its GP by, and what is bound to it while candidates are walked
    gp_global = (ref_egp, 'EuclideanGP')
    stand_in = _KernelMeanNoise

    # -- what differs between the fitters: the Cartesian-product fitter overrides these -----------------
    def _kernel_spec(self, kernel):
      return kernel.to_spec(self.dim)

    def _mean_probe(self):
      """ a point at which the candidates' constant mean functions are read """
      return [np.zeros(self.dim)]

    def _joins_batch(self, gp, extra):
      """ whether the candidate build_gp made `gp` of can be fitted in the batch's one device call; `extra` is the
          batch's own state, handed on to _engine_lml_batch """
      # (a fitter subclass that builds its GP through its own import gets a real GP here, not the stand-in: it has
      #  no `host_kernel`; what the mirror's GP calls `_generic` says the same, and anything else takes the safe route)
      return not getattr(gp, 'host_kernel', getattr(gp, '_generic', True))

    def _host_points(self, extra):
      return _as_2d_array(self.X)

    def _device_points(self, extra):
      if getattr(self, '_X_dev', None) is None:
        self._X_dev = get_engine().to_device(self._host_points(extra))
      return self._X_dev

    def _lml_keywords(self, extra):
      return {}

    # -- the batch objective -------------------------------------------------------------------------------
    def _engine_lml_batch(self, specs, means, noises, extra=None):
      """ one device call for the candidates: the process's engine, or -- install(tuning_gpus=N), a batch that fills
          more than one GPU -- the candidates cut over N of them """
      multi = parallel.tuning_route(tuning_gpus, len(specs), len(self.X))
      if multi is None:
        engine, points = get_engine(), self._device_points(extra)
      else:
        engine, points = multi, parallel.per_rank_inputs(self, multi, lambda: self._host_points(extra), self.X)
      return engine.gp_lml_batch(specs, points, self._labels_array(), means, noises, **self._lml_keywords(extra))

    def _candidates_by_build_gp(self, cts_hps_list, dscr_hps, other_gp_params):
      """ (specs, means, noises, extra) of the candidates, each through the reference's own build_gp (gp_core.py:
          501-543) without a posterior -- that gives the kernel, the constant mean and the noise variance it would be
          fitted with -- or None when any of them must take a fit of its own. """
      if getattr(self.options, 'mean_func', None) is not None:
        return None
      per_cand, probe, extra = _per_candidate(dscr_hps), self._mean_probe(), {}
      specs, means, noises = [], [], []
      with bound_stand_in(self.gp_global[0], self.gp_global[1], self.stand_in):
        for i, cts in enumerate(cts_hps_list):
          gp = self.build_gp(cts, _dscr_row(dscr_hps, per_cand, i), other_gp_params=other_gp_params, build_posterior=False)
          if not self._joins_batch(gp, extra):
            return None
          specs.append(self._kernel_spec(gp.kernel))
          means.append(float(gp.mean_func(probe)[0]))
          noises.append(float(gp.noise_var))
      return specs, means, noises, extra

    def _fit_each(self, cts_hps_list, dscr_hps, other_gp_params):
      """ an arbitrary mean function, or a kernel the host evaluates: one fit per candidate """
      per_cand = _per_candidate(dscr_hps)
      return np.array([self._tuning_objective(cts, _dscr_row(dscr_hps, per_cand, i), other_gp_params=other_gp_params)
                       for i, cts in enumerate(cts_hps_list)])

    def _lml_batch(self, cts_hps_list, dscr_hps, other_gp_params=None):
      """ Log marginal likelihoods of a list of candidates, the whole list fitted in one device call. """
      if len(cts_hps_list) == 0:
        return np.zeros((0,))
      decoded = self._decode_candidates(cts_hps_list, dscr_hps, _per_candidate(dscr_hps), other_gp_params)
      if decoded is not None:
        return _logged(self._engine_lml_batch(*decoded))
      batch = self._candidates_by_build_gp(cts_hps_list, dscr_hps, other_gp_params)
      if batch is None:
        return self._fit_each(cts_hps_list, dscr_hps, other_gp_params)
      return self._engine_lml_batch(*batch)

    def _build_one(self, cts, dscr, other_gp_params=None):
      """ (kernel signature, mean, noise) of one candidate by the general route: the reference's build_gp. """
      batch = self._candidates_by_build_gp([cts], dscr, other_gp_params)
      return None if batch is None else (batch[0][0].signature(), batch[1][0], batch[2][0])

    def _set_up_ml_hp_tune(self):
      """ gp_core.py:423-474, then the optimisers are swapped for their batch-objective forms
          (same random draws / same boxes, so the same hyper-parameters win). """
      ref_fitter_cls._set_up_ml_hp_tune(self)
      self._X_dev = None
      method = self.ml_hp_tune_opt_method
      def _rand(obj, max_evals):
        val, pt, _ = random_maximise(obj, self.cts_hp_bounds, max_evals, vectorised=True)
        return val, pt, None
      def _tree(obj, max_evals):
        val, pt, _ = pdoo_maximise_batched(obj, self.cts_hp_bounds, max_evals, frontier=self.pdoo_frontier,
                                           depth=2 if self.pdoo_frontier > 0 else 0)
        return val, pt, None
      def _rand_exp(obj, max_evals):
        cts, dscr, lml_vals = random_sample_cts_dscr(obj, self.cts_hp_bounds, self.dscr_hp_vals, max_evals,
                                                     vectorised=True)
        probs = np.exp(lml_vals - max(lml_vals))
        return cts, dscr, probs / probs.sum()
      self._batched_ml = True
      if method == 'rand':
        self.cts_hp_optimise = _rand
      elif method == 'pdoo' or (method == 'direct' and not _fortran_direct_available()):
        self.cts_hp_optimise = _tree
      elif method == 'rand_exp_sampling':
        self.hp_sampler = _rand_exp
      else:
        self._batched_ml = False          # a compiled DIRECT drives the search one point at a time

    def _decode_candidates(self, cts_hps_list, dscr_hps, per_cand, other_gp_params):
      """ (specs, means, noises) of the candidates WITHOUT a call of the reference's build_gp per candidate, for the
          usual cases -- an SE or Matern kernel over all dimensions or an additive model of such kernels, no user mean
          function, the fitter's own build_gp / _child_build_gp -- or None (then _lml_batch takes the general route above).
          The arithmetic is the reference's, operation for operation and on operands of the same shape (gp_core.py:
          501-543: the tuned mean is the first entry, exp of the next is the noise variance; gp/euclidean_gp.py:796-866:
          exp of the next is the scale, np.exp of the next `dim` entries -- one call on the slice -- the bandwidths, or
          exp of one entry repeated; a tuned Matern nu is the first discrete entry), so the numbers are the same bits.
          What it skips are the objects: per candidate a kernel, a mean closure, a stand-in GP and a second
          description of the kernel, ~50 us of Python that a real run pays some 300 000 times per 60 evaluations.
          The first calls of every fitter check candidate 0 against the general route and switch this one off for
          good on any difference. """
      state = getattr(self, '_amd_decode', None)
      if state is None:
        state = self._amd_decode = {'ok': self._decode_applies(), 'checks': 0}
      if not state['ok']:
        return None
      try:
        dim = self.dim
        # what does not depend on the candidate is worked out once per fitter (and set of labels): the option fields,
        # the kernel's fixed hyper-parameters, the constant means gp_core.py:516-523 computes from the labels
        plan = state.get('plan')
        if plan is None or plan[0] is not self.Y or plan[1] != len(self.Y):
          o = self.options
          kh = self._prep_init_kernel_hyperparams(self.kernel_type)
          if kh['dim'] != dim:
            return None
          mean_type, noise_type = o.mean_func_type, o.noise_var_type
          if mean_type == 'mean':
            mean_c = np.mean(self.Y)
          elif mean_type == 'median':
            mean_c = np.median(self.Y)
          elif mean_type == 'upper_bound':
            mean_c = np.mean(self.Y) + 3 * np.std(self.Y)
          elif mean_type == 'const':
            mean_c = o.mean_func_const
          else:
            mean_c = 0
          noise_c = None
          if noise_type == 'label':
            noise_c = o.noise_var_label * (self.Y.std() ** 2)
          elif noise_type != 'tune':
            noise_c = o.noise_var_value
          matern = self.kernel_type == 'matern'
          nu_fixed = kh['nu'] if matern and 'nu' in kh and not kh['nu'] < 0 else None
          plan = state['plan'] = (self.Y, len(self.Y), mean_type, noise_type, mean_c, noise_c, matern, nu_fixed,
                                  o.use_same_bandwidth, bool(o.use_additive_gp))
        _, _, mean_type, noise_type, mean_c, noise_c, matern, nu_fixed, same_bw, additive = plan
        if additive:
          # an additive model (gp/euclidean_gp.py:329-337, 820-826, 893-897): the groups come with the call, every
          # group's kernel has scale 1 and its columns' bandwidths, the sum carries the scale
          groupings = other_gp_params.add_gp_groupings
          groups = [[int(c) for c in grp] for grp in groupings]
          n_groups = len(groups)
        specs, means, noises = [], [], []
        for i, cts in enumerate(cts_hps_list):
          dscr = _dscr_row(dscr_hps, per_cand, i)
          if self.num_hps != len(cts) + len(dscr):
            return None                                 # (the general route raises the reference's error)
          if additive:
            dscr = dscr[:-1]                            # the group size's index
          if mean_type == 'tune':
            mean = cts[0].item()
            cts = cts[1:]
          else:
            mean = mean_c
          if noise_type == 'tune':
            noise = np.exp(cts[0])
            cts = cts[1:]
          else:
            noise = noise_c
          scale = np.exp(cts[0])
          cts = cts[1:]
          if same_bw:
            bws = [np.exp(cts[0])] * dim
            cts = cts[1:]
          else:
            bws = np.exp(cts[0:dim])
            cts = cts[dim:]
          if len(cts) != 0:
            return None
          if matern:
            if nu_fixed is None:
              nu = dscr[0]
              dscr = dscr[1:]
            else:
              nu = nu_fixed
            if nu % 1 != 0.5:
              return None
          if len(dscr) != 0 or len(bws) != dim:
            return None
          if additive:
            specs.append(KernelSpec('additive', dim, scale, groups=groups, sub_kinds=['matern' if matern else 'se'] * n_groups,
                                    sub_scales=[1.0] * n_groups, sub_nus=[nu if matern else 0.0] * n_groups,
                                    sub_bandwidths=[np.ravel(np.asarray([bws[idx] for idx in grp], dtype=float))
                                                    for grp in groupings]))
          else:
            specs.append(KernelSpec('matern', dim, scale, bws, nu=nu) if matern else KernelSpec('se', dim, scale, bws))
          means.append(float(mean))
          noises.append(float(noise))
      except Exception:             # pylint: disable=broad-except
        return None                 # whatever it was, the general route meets it the way the reference does
      if state['checks'] < 3:
        state['checks'] += 1
        want = self._build_one(cts_hps_list[0], _dscr_row(dscr_hps, per_cand, 0), other_gp_params)
        got = (specs[0].signature(), means[0], noises[0])
        if want is None or want != got:
          state['ok'] = False
          return None
      return specs, means, noises

    def _decode_applies(self):
      import dragonfly.gp.kernel as _ref_kernel
      from . import kernel as _kernel
      o = self.options
      return (type(self)._child_build_gp is ref_fitter_cls._child_build_gp and type(self).build_gp is ref_fitter_cls.build_gp
              and self.kernel_type in ('se', 'matern') and getattr(o, 'mean_func', None) is None
              and _ref_kernel.SEKernel is _kernel.SEKernel and _ref_kernel.MaternKernel is _kernel.MaternKernel
              and _ref_kernel.AdditiveKernel is _kernel.AdditiveKernel)

    def _labels_array(self):
      """ self.Y as the float64 array every batch call hands to the engine (converted once per list of labels) """
      cached = getattr(self, '_amd_labels', None)
      if cached is None or cached[0] is not self.Y or cached[1] != len(self.Y):
        cached = self._amd_labels = (self.Y, len(self.Y), np.asarray(self.Y, dtype=np.float64))
      return cached[2]

    # -- posterior sampling (gp_core.py:476-487, 592-726) -------------------------------------------
    def _set_up_post_sampling_hp_tune(self):
      """ The continuous hyper-parameters are slice-sampled one coordinate at a time
          (gp_core.py:687-697); the sampler is swapped for the speculative one, which follows the
          same chain with its density evaluations batched. """
      ref_fitter_cls._set_up_post_sampling_hp_tune(self)
      if self.options.post_hp_tune_method == 'slice':
        self.hp_sampler_cts = self._speculative_slice

    def _speculative_slice(self, model, init_sample, num_samples, burn):
      # pylint: disable=unused-argument
      from .slice_sampler import SpeculativeSlice
      return SpeculativeSlice(self._post_logp_batch, merge_first=_SLICE_MERGE_FIRST).sample(init_sample, num_samples, burn)

    def _post_logp_batch(self, xs):
      """ The log density `_logp` of gp_core.py:597-622 -- log priors of all hyper-parameters, summed
          in index order, plus the log marginal likelihood -- at each value in xs of the
          coordinate being sampled (self.curr_hp), the others as they currently are. """
      num_cts = len(self.cts_hp_bounds)
      out = np.empty(len(xs))
      pending = []
      base = np.array(self.hps, dtype=np.float64)

      def prior_term(i, value):
        prior = self.hp_priors[i]
        if type(prior).__name__ == 'Categorical':
          return prior.logp(prior.get_id(value))
        return prior.logp(value)
      # only the coordinate being sampled changes between the xs: the other priors' terms are evaluated once, and
      # added in index order per x exactly as the reference's loop adds them (same partial sums, same bits)
      # (and the sampler asks several times per step of a coordinate -- stepping out, shrinking -- with the others unchanged)
      cur = self.curr_hp
      key = (cur, base.tobytes())
      cached = getattr(self, '_amd_prior_terms', None)
      if cached is not None and cached[0] == key and cached[1] is self.hp_priors:
        terms = cached[2]
      else:
        terms = [None if i == cur else prior_term(i, base[i]) for i in range(len(self.hp_priors))]
        self._amd_prior_terms = (key, self.hp_priors, terms)
      for k, x in enumerate(xs):
        hps = base.copy()
        hps[cur] = x
        lp = 0
        for i, t in enumerate(terms):
          lp += prior_term(i, hps[i]) if t is None else t
        if not np.isfinite(lp):
          out[k] = lp
        else:
          pending.append((k, lp, hps))
      if pending:
        lmls = self._lml_batch([h[:num_cts] for _, _, h in pending],
                               [h[num_cts:self.num_hps] for _, _, h in pending], self.other_gp_params)
        for (k, lp, _), lml in zip(pending, lmls):
          out[k] = lp + lml
      return out

    def _optimise_cts_hps_for_given_dscr_hps(self, given_dscr_hps):
      """ gp_core.py:576-583 / euclidean_gp.py:303-313 with the batch objective. """
      if not getattr(self, '_batched_ml', False):
        return ref_fitter_cls._optimise_cts_hps_for_given_dscr_hps(self, given_dscr_hps)
      # (an option of the Euclidean fitter: the Cartesian-product fitters' option lists do not carry it)
      if getattr(self.options, 'use_additive_gp', False):
        from dragonfly.gp.euclidean_gp import optimise_cts_hps_for_given_dscr_hps_in_add_model
        return optimise_cts_hps_for_given_dscr_hps_in_add_model(
            given_dscr_hps, self.options.num_groups_per_group_size, self.dim, self.hp_tune_max_evals,
            self.cts_hp_optimise, self._lml_batch)
      objective = lambda arg: self._lml_batch(arg, list(given_dscr_hps))
      val, cts_hps, _ = self.cts_hp_optimise(objective, self.hp_tune_max_evals)
      return val, cts_hps, None

    def _sample_cts_dscr_hps_for_rand_exp_sampling(self):
      """ gp_core.py:585-590 (non-additive models) with the batch objective. """
      if not getattr(self, '_batched_ml', False) or getattr(self.options, 'use_additive_gp', False):
        return ref_fitter_cls._sample_cts_dscr_hps_for_rand_exp_sampling(self)
      cts, dscr, probs = self.hp_sampler(self._lml_batch, self.hp_tune_max_evals)
      return cts, dscr, [None] * len(cts), probs

  return BatchedEuclideanGPFitter


def make_batched_cp_fitter(ref_fitter_cls, tuning_gpus=None, gp_name='CPGP', stand_in=_CPKernelMeanNoise):
  """ A subclass of the reference's CPGPFitter (gp/cartesian_product_gp.py:322-377) whose maximum-likelihood tuners see
      their objective as a batch: the machinery of make_batched_fitter -- the vectorised random search for 'rand' and
      'rand_exp_sampling', the batched tree search for 'pdoo' and the 'direct' fall-back, the speculative slice sampler
      -- over a batch objective that takes (kernel, mean, noise) of every candidate from the reference's own build_gp
      through a stand-in for the GP constructor and evaluates the list in ONE dfh_gp_lml_batch call with the
      projection flag.  The points are packed once per data set (the category codes do not depend on the
      hyper-parameters).  Candidates whose kernel has no device description take one fit each.
      gp_name, stand_in: the module global the fitter constructs its GP by and the stand-in bound to it while the
      candidates are decoded -- ('CPMFGP', _CPMFKernelMeanNoise) for the reference's CPMFGPFitter (:394-497). """
  import dragonfly.gp.cartesian_product_gp as ref_cpgp
  from .engine import get_engine
  base = make_batched_fitter(ref_fitter_cls, tuning_gpus=tuning_gpus)
  cp_stand_in = stand_in

  class BatchedCPGPFitter(base):
    """ dragonfly.gp.cartesian_product_gp.CPGPFitter with batched ML tuning (dragonfly_amd.install). """
    gp_global = (ref_cpgp, gp_name)
    stand_in = cp_stand_in

    def _decode_candidates(self, cts_hps_list, dscr_hps, per_cand, other_gp_params):
      return None                    # (the short cut of the Euclidean fitter's own factory does not apply)

    def _kernel_spec(self, kernel):
      return kernel.to_spec()

    def _mean_probe(self):
      return [self.X[0]]

    def _joins_batch(self, gp, extra):
      """ a kernel on the descriptor route, and one handle_non_psd_kernels for the whole batch: `extra` keeps it, and
          the first candidate's kernel, by which the points are packed """
      if getattr(gp, 'host_kernel', True) or extra.setdefault('mode', gp.handle_non_psd_kernels) != gp.handle_non_psd_kernels:
        return False
      extra.setdefault('kernel', gp.kernel)
      return True

    def _host_points(self, extra):
      return extra['kernel'].pack(self.X)

    def _device_points(self, extra):
      cached = getattr(self, '_amd_packed', None)
      if cached is None or cached[0] is not self.X or cached[1] != len(self.X):
        cached = self._amd_packed = (self.X, len(self.X), get_engine().to_device(self._host_points(extra)))
      return cached[2]

    def _lml_keywords(self, extra):
      return {'handle_non_psd_kernels': extra['mode']}

    def _lml_batch(self, cts_hps_list, dscr_hps, other_gp_params=None):
      if len(cts_hps_list) == 0:
        return np.zeros((0,))
      batch = self._candidates_by_build_gp(cts_hps_list, dscr_hps, other_gp_params)
      if batch is None:
        return self._fit_each(cts_hps_list, dscr_hps, other_gp_params)
      return _logged(self._engine_lml_batch(*batch))

  return BatchedCPGPFitter
