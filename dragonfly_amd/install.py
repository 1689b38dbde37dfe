"""Install the MI355X engine under a real Dragonfly (the drop-in of SURVEY.md section 8b).

    import dragonfly_amd.install as dfi
    dfi.install()          # before building optimisers / calling maximise_function
    ...
    dfi.uninstall()

What is rebound (each is a *name looked up at call time* in the reference, so no reference file is
edited):
  S1 kernels   dragonfly.gp.kernel.SEKernel / MaternKernel / AdditiveKernel / ESPKernelSE /
               ESPKernelMatern -> dragonfly_amd.kernel
               (the Euclidean kernel factory resolves `gp_kernel.SEKernel` etc. at call time:
               dragonfly/gp/euclidean_gp.py:17,850,859,882,890,896); an ESP kernel then is one
               kernel-matrix launch instead of one per dimension and a host recursion
  S2/S3 GP     dragonfly.gp.euclidean_gp.EuclideanGP -> dragonfly_amd.euclidean_gp.EuclideanGP
               (every Euclidean fitter constructs its GP through this module global,
               dragonfly/gp/euclidean_gp.py:338)
  S2' MF GP    (only with install(multi_fidelity=True)) dragonfly.gp.euclidean_gp.EuclideanMFGP ->
               dragonfly_amd.mf_gp.EuclideanMFGP.  SE / Matern fidelity and domain kernels give the
               coordinate-product kernel on the device; any other factor (the reference's poly /
               expdecay kernels) puts the GP into host-kernel mode -- kernel evaluated by its own
               class on the host, factorisation and posterior on the device.  The MF fitter
               constructs its GP through this module global (dragonfly/gp/euclidean_gp.py:707).
               Opt-in because the reference class cannot be reached once the name is rebound (its
               __init__ calls super(EuclideanMFGP, self)).
  S2'' CP GP   (only with install(cartesian_product=True)) dragonfly.gp.cartesian_product_gp.CPGP ->
               dragonfly_amd.cartesian_product_gp.device_cpgp_class(...): the reference's own class body over the
               device GP, and HammingKernel / CartesianProductKernel in dragonfly.gp.kernel and
               dragonfly.gp.cartesian_product_gp -> our mirrors.  A CP kernel whose parts are SE, Matern,
               exponential-decay or Hamming kernels is evaluated on the device from one product descriptor
               (categories packed as codes), projected ('project_first', gp_core.py:838-841), factored and
               evaluated there; with any other part (neural-network kernels, pre-computed distances) the
               kernel stays on the host and only the projection, the factorisation and the posterior run
               on the device.  The CP fitter constructs its GP through this module global.  Opt-in for
               the same reason as the MF GP.  With batched_tuning, dragonfly.opt.gp_bandit.CPGPFitter and
               dragonfly.opt.multiobjective_gp_bandit.CPGPFitter -> make_batched_cp_fitter(...): the S3 fitter's
               batch objective for CP candidates, one dfh_gp_lml_batch call with the projection flag.
  S2''' CP MF GP  (only with install(multi_fidelity=True, cartesian_product=True, cp_multi_fidelity=True))
               dragonfly.gp.cartesian_product_gp.CPMFGP -> dragonfly_amd.cartesian_product_gp.device_cpmfgp_class(...):
               the reference's own class body over dragonfly_amd.mf_gp.MFGP.  The joint kernel
               kernel_scale * (1.0 * k_f1 * ..) * (1.0 * k_d1 * ..) is ONE product descriptor whose two factors are
               products themselves (factor_is_sum = DFH_FACTOR_PRODUCT), multiplied on the device in the reference's
               order; the (z, x) pairs are packed side by side.  Distance lists or a part the device does not know:
               host-kernel mode, as for CPGP.  With batched_tuning dragonfly.opt.gp_bandit.CPMFGPFitter -> the batched
               CP fitter (one dfh_gp_lml_batch call with the projection flag per batch of candidates).
  S4 acquisitions  dispatchers are written into the namespaces
               dragonfly.opt.gpb_acquisitions.asy / syn / seq (looked up with getattr at
               dragonfly/opt/gp_bandit.py:490,510,651,681): the fused callables on Euclidean
               domains, the reference's own callables on every other domain
  S3 fitter    dragonfly.opt.gp_bandit.EuclideanGPFitter and
               dragonfly.opt.multiobjective_gp_bandit.EuclideanGPFitter (the names the bandits
               construct their fitters by, gp_bandit.py:22,584; multiobjective_gp_bandit.py:27,481)
               -> a subclass OF THE REFERENCE'S fitter that only changes how the maximum-likelihood
               tuners see their objective: as a batch (candidates in, log marginal likelihoods
               out, one dfh_gp_lml_batch call) instead of one fit per callback.  'rand' and
               'rand_exp_sampling' evaluate their whole sample in one call, 'pdoo' -- and 'direct'
               without the Fortran library, the reference's own fall-back and its default -- run
               the tree search of dragonfly_amd.doo a frontier per call, and the slice sampler of
               the posterior-sampling criterion evaluates its loops' next candidates a batch at
               a time (dragonfly_amd.slice_sampler: the same chain, draw for draw).  Everything
               else of the fitter (options, bounds, priors, the bandit bookkeeping) is the
               reference's code.  install(batched_tuning=False) leaves the fitter alone.
               install(tuning_gpus=N): a random-search batch that fills more than one GPU is cut over N
               GPUs of this process (parallel.MultiEngine.gp_lml_batch); smaller batches go where they went.
  S4' MOO      dragonfly.opt.multiobjective_gpb_acquisitions.maximise_acquisition -> ours for
               Euclidean domains: the multi-objective closures are maximised by the batched tree
               search / the vectorised random search too.
  S4'' MOO acquisitions  (only with install(multi_objective=True)) the four callables of the namespaces
               dragonfly.opt.multiobjective_gpb_acquisitions.asy / seq (lin_ts, tch_ts, lin_ucb, tch_ucb) ->
               dispatchers as in S4: dragonfly_amd.multiobjective_gpb_acquisitions on Euclidean domains -- the
               K objectives' posteriors (or joint draws, points in progress hallucinated on the device), the
               scalarisation and the arg-max in one device call -- the reference's own callables elsewhere.
               Opt-in: without the flag the per-objective call stream of S4' stays exactly as it was.
               With cartesian_product=True and cp_acquisitions=True as well, the four dispatchers call ours on
               Cartesian-product domains too, when multiobjective_gpb_acquisitions.mo_cp_acquisition_applies holds: K
               device CP GPs on the descriptor route on one engine, kernels guaranteed PSD, no multi-fidelity.  A
               Thompson step is the reference's samples in ONE mo_thompson_pointwise call (dfh_mo_ts_pointwise, normals
               point-major), a UCB step ONE mo_ucb_argmax on 'rand', a frontier per call under the tree search, one call
               per point under Dragonfly's own maximisers (the GA, a compiled DIRECT).  The names rebound are the same.
  S4''' BOCA   (only with install(multi_fidelity=True, boca=True)) dragonfly.opt.gpb_acquisitions.boca (looked up
               at call time, opt/gp_bandit.py:495,660,663) -> a dispatcher: dragonfly_amd.gpb_acquisitions.boca when
               the GP is the mirror EuclideanMFGP with a device kernel on a Euclidean domain -- the point chosen by
               the fused call on [fidel_to_opt, candidate] rows joined in HBM (add-UCB: dfh_mf_add_ucb_all on the
               joint GP's factor), the fidelity by the reference's rule over one eval_at_fidel call -- the
               reference's own boca otherwise.  Opt-in: without the flag the call stream of S2' stays as it was.
  S4-CP-BOCA   (only with install(multi_fidelity=True, cartesian_product=True, boca=True, cp_acquisitions=True,
               cp_multi_fidelity=True)) the BOCA dispatcher calls ours on Cartesian-product domains too, where
               gpb_acquisitions.cp_boca_applies holds.  The point: the reference's samples packed by the domain kernel,
               joined in HBM with the packed fidel_to_opt, the (fidelity, point) pairs in progress packed jointly, in
               ONE acq_argmax / thompson_pointwise call; the tree search of an all-Euclidean domain a frontier per call
               through the view; the GA, a compiled DIRECT and add-UCB the reference's callables, point by point on the
               device posterior.  The fidelity: one eval_at_fidel call and the reference's rule.
  S4-CP        (only with install(cartesian_product=True, cp_acquisitions=True)) the S4 dispatchers of ucb / ei / pi / ttei / ts
               call ours on Cartesian-product domains as well, when gpb_acquisitions.cp_acquisition_applies holds: the device
               CP GP on the descriptor route, a kernel guaranteed PSD, no multi-fidelity, and 'rand' -- the reference's own
               samples packed in one pass into ONE acq_argmax / thompson_pointwise call -- or the tree search on an
               all-Euclidean product without constraints, a frontier per call.  The GA, a compiled DIRECT, add_ucb and
               everything else keep the reference's callable.  Opt-in: the names rebound are the same either way.
A compiled Fortran DIRECT, when present, keeps working: it calls gp.eval per point, which now
runs on the device, through `external_maximise_with_method`.
"""
import os

import numpy as np

from . import gaplog


_saved = []     # (object, attribute name, original value)


def install(multi_fidelity=False, batched_tuning=True, cartesian_product=False, multi_objective=False, tuning_gpus=None,
            boca=False, cp_acquisitions=False, cp_multi_fidelity=False):
  """ Rebinds the names listed above; returns the list of patched attributes.
      boca=True (only together with multi_fidelity=True; ValueError otherwise): BOCA's decision step runs on the device.
      cp_acquisitions=True (only together with cartesian_product=True; ValueError otherwise): the S4 dispatchers call
      ours on Cartesian-product domains too, where gpb_acquisitions.cp_acquisition_applies says so -- and, together
      with multi_objective=True, the multi-objective dispatchers where
      multiobjective_gpb_acquisitions.mo_cp_acquisition_applies does.  The names rebound are the same with and without it.
      cp_multi_fidelity=True (only together with cartesian_product=True and multi_fidelity=True; ValueError otherwise):
      dragonfly.gp.cartesian_product_gp.CPMFGP -> cartesian_product_gp.device_cpmfgp_class(...), the multi-fidelity GP
      of Cartesian-product domains on the device GP, and with batched_tuning dragonfly.opt.gp_bandit.CPMFGPFitter ->
      the batched CP fitter over it.  Without the flag neither name is touched.
      tuning_gpus=N > 1 (with batched_tuning): a tuning batch large enough to fill more than one GPU
      (parallel.lml_shard_plan: more than 256 candidates up to n = 2047) is cut over N GPUs of this process
      (dfh_mgpu_lml_batch); every other batch, and everything with None or 1, goes exactly where it went before. """
  if boca and not multi_fidelity:
    raise ValueError('install(boca=True) needs multi_fidelity=True: BOCA runs on the device through the mirror MF GP.')
  if cp_acquisitions and not cartesian_product:
    raise ValueError('install(cp_acquisitions=True) needs cartesian_product=True: the fused calls run on the device CP GP.')
  if cp_multi_fidelity and not (cartesian_product and multi_fidelity):
    raise ValueError('install(cp_multi_fidelity=True) needs cartesian_product=True and multi_fidelity=True: the '
                     'multi-fidelity GP of product domains runs on the device CP kernel mirrors.')
  import dragonfly.gp.kernel as ref_kernel
  import dragonfly.gp.euclidean_gp as ref_egp
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly.exd.exd_utils import maximise_with_method
  from . import kernel, euclidean_gp, gpb_acquisitions, mf_gp
  patched = []
  def _set(mod, name, new):
    _saved.append((mod, name, getattr(mod, name)))
    setattr(mod, name, new)
    patched.append('%s.%s' % (mod.__name__, name))
  for name in ('SEKernel', 'MaternKernel', 'AdditiveKernel', 'ESPKernelSE', 'ESPKernelMatern'):
    _set(ref_kernel, name, getattr(kernel, name))
  _set(ref_egp, 'EuclideanGP', euclidean_gp.EuclideanGP)

  if multi_fidelity:
    _set(ref_egp, 'EuclideanMFGP', mf_gp.EuclideanMFGP)
  if cartesian_product:
    import dragonfly.gp.cartesian_product_gp as ref_cpgp
    from . import cartesian_product_gp
    _set(ref_cpgp, 'CPGP', cartesian_product_gp.device_cpgp_class(ref_cpgp))
    # the CP kernel factory builds its Hamming parts and the product itself by these two names, looked up at call time
    # in both modules (cartesian_product_gp.py:19); the Euclidean parts already arrive as our mirrors
    for name in ('HammingKernel', 'CartesianProductKernel'):
      _set(ref_kernel, name, getattr(kernel, name))
      _set(ref_cpgp, name, getattr(kernel, name))
    if cp_multi_fidelity:
      _set(ref_cpgp, 'CPMFGP', cartesian_product_gp.device_cpmfgp_class(ref_cpgp))
  for ns_name in ('asy', 'syn', 'seq'):
    ref_ns = getattr(ref_acq, ns_name)
    our_ns = getattr(gpb_acquisitions, ns_name)
    for acq in ('ucb', 'ei', 'pi', 'ttei', 'ts', 'add_ucb'):
      _saved.append((ref_ns, acq, getattr(ref_ns, acq)))
      setattr(ref_ns, acq, _euclidean_dispatch(getattr(our_ns, acq), getattr(ref_ns, acq),
                                               cp_acq=acq if cp_acquisitions else None))
      patched.append('dragonfly.opt.gpb_acquisitions.%s.%s' % (ns_name, acq))
  gpb_acquisitions.external_maximise_with_method = maximise_with_method
  if boca:
    _set(ref_acq, 'boca', _boca_dispatch(gpb_acquisitions.boca, ref_acq.boca,
                                         cp_boca=cp_acquisitions and cp_multi_fidelity))
  # the multi-objective acquisitions (opt/multiobjective_gpb_acquisitions.py:19-107) are closures
  # over rows of points handed to maximise_acquisition, a name they import at module level: with
  # ours they get the batched tree search / vectorised random search on Euclidean domains
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo_acq
  ref_maximise = ref_moo_acq.maximise_acquisition
  def _moo_maximise_acquisition(acq_fn, anc_data, *args, **kwargs):
    if anc_data.domain.get_type() == 'euclidean':
      return gpb_acquisitions.maximise_acquisition(acq_fn, anc_data, *args, **kwargs)
    return ref_maximise(acq_fn, anc_data, *args, **kwargs)
  _set(ref_moo_acq, 'maximise_acquisition', _moo_maximise_acquisition)
  if multi_objective:
    # the four acquisitions themselves, looked up with getattr in the namespaces asy / seq
    # (opt/multiobjective_gp_bandit.py): K posteriors or draws, scalarisation and arg-max in one device call
    from . import multiobjective_gpb_acquisitions as our_moo_acq
    for ns_name in ('asy', 'seq'):
      ref_ns, our_ns = getattr(ref_moo_acq, ns_name), getattr(our_moo_acq, ns_name)
      for acq in ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb'):
        _saved.append((ref_ns, acq, getattr(ref_ns, acq)))
        setattr(ref_ns, acq, _euclidean_dispatch(getattr(our_ns, acq), getattr(ref_ns, acq),
                                                 mo_cp_acq=acq if cp_acquisitions else None))
        patched.append('dragonfly.opt.multiobjective_gpb_acquisitions.%s.%s' % (ns_name, acq))
  if batched_tuning:
    import dragonfly.opt.gp_bandit as ref_gp_bandit
    import dragonfly.opt.multiobjective_gp_bandit as ref_moo_bandit
    batched = make_batched_fitter(ref_egp.EuclideanGPFitter, tuning_gpus=tuning_gpus)
    _set(ref_gp_bandit, 'EuclideanGPFitter', batched)
    _set(ref_moo_bandit, 'EuclideanGPFitter', batched)
    if cartesian_product:
      # the names the CP bandits construct their fitter by (gp_bandit.py, multiobjective_gp_bandit.py)
      import dragonfly.gp.cartesian_product_gp as ref_cpgp
      batched_cp = make_batched_cp_fitter(ref_cpgp.CPGPFitter, tuning_gpus=tuning_gpus)
      _set(ref_gp_bandit, 'CPGPFitter', batched_cp)
      _set(ref_moo_bandit, 'CPGPFitter', batched_cp)
      if cp_multi_fidelity:
        _set(ref_gp_bandit, 'CPMFGPFitter', make_batched_cp_fitter(ref_cpgp.CPMFGPFitter, tuning_gpus=tuning_gpus,
                                                                   gp_name='CPMFGP', stand_in=_CPMFKernelMeanNoise))
  return patched


def _euclidean_dispatch(ours, theirs, cp_acq=None, mo_cp_acq=None):
  """ The acquisition entry installed in the reference's namespaces: ours on Euclidean domains,
      the reference's own callable on every other domain (Cartesian-product, neural-network, ...
      domains keep running exactly as before).  Works for asy (gp, anc_data) and syn
      (num_workers, gps, anc_datas) signatures: the ancillary data is the last argument.
      cp_acq (install(cp_acquisitions=True): the acquisition's name): ours on a Cartesian-product domain as well,
      when gpb_acquisitions.cp_acquisition_applies holds for every GP of the call -- the device CP GP on the
      descriptor route with a kernel guaranteed PSD, no multi-fidelity, 'rand' or the tree search; the GA, a compiled
      DIRECT, host-kernel GPs and add-UCB stay with the reference's callable.
      mo_cp_acq (install(multi_objective=True, cartesian_product=True, cp_acquisitions=True): the multi-objective
      acquisition's name): ours on a Cartesian-product domain when
      multiobjective_gpb_acquisitions.mo_cp_acquisition_applies holds for the call's list of GPs. """
  def acquisition(*args, **kwargs):
    anc_data = args[-1]
    if isinstance(anc_data, (list, tuple)):
      anc_data = anc_data[0]
    if anc_data.domain.get_type() == 'euclidean':
      return ours(*args, **kwargs)
    if cp_acq is not None and anc_data.domain.get_type() == 'cartesian_product':
      from .gpb_acquisitions import cp_acquisition_applies, cp_boca_view_applies
      gps = args[-2]
      gps = list(gps) if isinstance(gps, (list, tuple)) else [gps]
      # (BOCA's view of a product-domain GP exists only where _boca_dispatch let our boca() make it)
      if all(cp_acquisition_applies(cp_acq, gp, anc_data) or cp_boca_view_applies(cp_acq, gp, anc_data) for gp in gps):
        return ours(*args, **kwargs)
    if mo_cp_acq is not None and anc_data.domain.get_type() == 'cartesian_product':
      from .multiobjective_gpb_acquisitions import mo_cp_acquisition_applies
      if mo_cp_acquisition_applies(mo_cp_acq, args[-2], anc_data):
        return ours(*args, **kwargs)
    return theirs(*args, **kwargs)
  acquisition.__wrapped__ = ours
  acquisition.reference_callable = theirs
  return acquisition


def _boca_dispatch(ours, theirs, cp_boca=False):
  """ dragonfly.opt.gpb_acquisitions.boca under install(boca=True): ours for the mirror EuclideanMFGP with a device
      kernel on a Euclidean domain, the reference's own boca for everything else.
      cp_boca (install(boca=True, cp_acquisitions=True, cp_multi_fidelity=True)): ours on a Cartesian-product domain as
      well, where gpb_acquisitions.cp_boca_applies holds -- the device CPMFGP on the descriptor route, a kernel
      guaranteed PSD, not add-UCB. """
  def boca(select_pt_func, mfgp, anc_data, func_caller):
    from . import gpb_acquisitions, mf_gp
    if anc_data.domain.get_type() == 'euclidean' and isinstance(mfgp, mf_gp.EuclideanMFGP) and \
       gpb_acquisitions._is_device_gp(mfgp):     # pylint: disable=protected-access
      return ours(select_pt_func, mfgp, anc_data, func_caller)
    if cp_boca and gpb_acquisitions.cp_boca_applies(mfgp, anc_data):
      return ours(select_pt_func, mfgp, anc_data, func_caller)
    return theirs(select_pt_func, mfgp, anc_data, func_caller)
  boca.__wrapped__ = ours
  boca.reference_callable = theirs
  return boca


# DFH_SLICE_MERGE=0: the speculative slice sampler's stepping-out and shrinking candidates in separate density calls again
_SLICE_MERGE_FIRST = os.environ.get('DFH_SLICE_MERGE', '1') != '0'


class _KernelMeanNoise(object):
  """ What BatchedEuclideanGPFitter._lml_batch needs of the GP the reference's build_gp constructs -- kernel, mean
      function, noise variance -- with EuclideanGP's constructor signature (gp/euclidean_gp.py:151-152). """
  __slots__ = ('kernel', 'mean_func', 'noise_var', 'host_kernel')

  def __init__(self, X, Y, kernel, mean_func, noise_var, kernel_hyperparams=None, build_posterior=True, reporter=None):
    # pylint: disable=unused-argument
    if isinstance(kernel, str) or build_posterior:
      raise RuntimeError('dragonfly_amd.install: the candidate stand-in was asked for a real GP')
    self.kernel, self.mean_func, self.noise_var = kernel, mean_func, noise_var
    # (gp_core.GP._generic for a plain EuclideanGP: a kernel without a device description is evaluated by the host)
    self.host_kernel = not (hasattr(kernel, 'to_spec') and getattr(kernel, 'has_device_spec', lambda: True)())


def make_batched_fitter(ref_fitter_cls, tuning_gpus=None):
  """ A subclass of the reference's EuclideanGPFitter whose maximum-likelihood tuners evaluate the
      tuning objective (gp_core.py:551-564) in batches on the device.  tuning_gpus: see install(). """
  from . import parallel
  from .doo import pdoo_maximise_batched
  from .engine import get_engine, KernelSpec
  from .gpb_acquisitions import _fortran_direct_available
  from .kernel import _as_2d_array
  from .oper_utils import random_maximise, random_sample_cts_dscr

  class BatchedEuclideanGPFitter(ref_fitter_cls):
    """ dragonfly.gp.euclidean_gp.EuclideanGPFitter with batched ML tuning (dragonfly_amd.install). """
    pdoo_frontier = 32

    def _engine_lml_batch(self, specs, means, noises):
      """ one device call for the candidates: the process's engine, or -- install(tuning_gpus=N), a batch that fills
          more than one GPU -- the candidates cut over N of them """
      multi = parallel.tuning_route(tuning_gpus, len(specs), len(self.X))
      if multi is not None:
        Xs = parallel.per_rank_inputs(self, multi, lambda: _as_2d_array(self.X), self.X)
        return multi.gp_lml_batch(specs, Xs, self._labels_array(), means, noises)
      if getattr(self, '_X_dev', None) is None:
        self._X_dev = get_engine().to_device(_as_2d_array(self.X))
      return get_engine().gp_lml_batch(specs, self._X_dev, self._labels_array(), means, noises)

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
          function, the fitter's own build_gp / _child_build_gp -- or None (then _lml_batch takes the general route below).
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
          dscr = list(dscr_hps[i]) if per_cand else list(dscr_hps)
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
        want = self._build_one(cts_hps_list[0], list(dscr_hps[0]) if per_cand else list(dscr_hps), other_gp_params)
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

    def _build_one(self, cts, dscr, other_gp_params=None):
      """ (kernel signature, mean, noise) of one candidate by the general route: the reference's build_gp. """
      import dragonfly.gp.euclidean_gp as _ref_egp
      saved_cls = _ref_egp.EuclideanGP
      _ref_egp.EuclideanGP = _KernelMeanNoise
      try:
        gp = self.build_gp(cts, dscr, other_gp_params=other_gp_params, build_posterior=False)
      finally:
        _ref_egp.EuclideanGP = saved_cls
      if getattr(gp, 'host_kernel', getattr(gp, '_generic', True)):
        return None
      return (gp.kernel.to_spec(self.dim).signature(), float(gp.mean_func([np.zeros(self.dim)])[0]), float(gp.noise_var))

    def _lml_batch(self, cts_hps_list, dscr_hps, other_gp_params=None):
      """ Log marginal likelihoods of a list of candidates.  Each candidate goes through the
          reference's own build_gp (gp_core.py:501-543) without building a posterior -- that gives
          the kernel, the constant mean and the noise variance it would be fitted with -- and the
          whole list is fitted in one device call. """
      per_cand = len(dscr_hps) > 0 and isinstance(dscr_hps[0], (list, tuple, np.ndarray))
      if len(cts_hps_list) == 0:
        return np.zeros((0,))
      user_mean = getattr(self.options, 'mean_func', None) is not None
      decoded = self._decode_candidates(cts_hps_list, dscr_hps, per_cand, other_gp_params)
      if decoded is not None:
        specs, means, noises = decoded
        lmls = self._engine_lml_batch(specs, means, noises)
        if gaplog.ENABLED and len(lmls) >= 16:       # (a random-search batch: its arg-max is the fitter's choice)
          gaplog.top2('hp_batch', lmls)
        return lmls
      specs, means, noises = [], [], []
      probe = [np.zeros(self.dim)]
      # build_gp ends in `EuclideanGP(self.X, self.Y, kernel, mean_func, noise_var, build_posterior=False)`, a module
      # global of the reference looked up at call time (gp/euclidean_gp.py:338).  All that is wanted of that object here
      # are its three arguments: for the length of this loop the name is bound to a stand-in that keeps them and does
      # nothing else (a GP object per candidate -- data lists copied and checked -- was a fifth of a small run's time).
      import dragonfly.gp.euclidean_gp as _ref_egp
      saved_cls = _ref_egp.EuclideanGP
      _ref_egp.EuclideanGP = _KernelMeanNoise
      try:
        for i, cts in enumerate(cts_hps_list):
          dscr = list(dscr_hps[i]) if per_cand else list(dscr_hps)
          gp = self.build_gp(cts, dscr, other_gp_params=other_gp_params, build_posterior=False)
          # (a fitter subclass that builds its GP through its own import gets a real GP here, not the stand-in: it has
          #  no `host_kernel`; what the mirror's GP calls `_generic` says the same, and anything else takes the safe route)
          if user_mean or getattr(gp, 'host_kernel', getattr(gp, '_generic', True)):
            specs = None
            break
          specs.append(gp.kernel.to_spec(self.dim))
          means.append(float(gp.mean_func(probe)[0]))
          noises.append(float(gp.noise_var))
      finally:
        _ref_egp.EuclideanGP = saved_cls
      if specs is None:
        # an arbitrary mean function, or a kernel the host evaluates: one fit per candidate
        return np.array([self._tuning_objective(c, list(dscr_hps[j]) if per_cand else list(dscr_hps),
                                                other_gp_params=other_gp_params)
                         for j, c in enumerate(cts_hps_list)])
      return self._engine_lml_batch(specs, means, noises)

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
      if self.options.use_additive_gp:
        from dragonfly.gp.euclidean_gp import optimise_cts_hps_for_given_dscr_hps_in_add_model
        return optimise_cts_hps_for_given_dscr_hps_in_add_model(
            given_dscr_hps, self.options.num_groups_per_group_size, self.dim, self.hp_tune_max_evals,
            self.cts_hp_optimise, self._lml_batch)
      objective = lambda arg: self._lml_batch(arg, list(given_dscr_hps))
      val, cts_hps, _ = self.cts_hp_optimise(objective, self.hp_tune_max_evals)
      return val, cts_hps, None

    def _sample_cts_dscr_hps_for_rand_exp_sampling(self):
      """ gp_core.py:585-590 (non-additive models) with the batch objective. """
      if not getattr(self, '_batched_ml', False) or self.options.use_additive_gp:
        return ref_fitter_cls._sample_cts_dscr_hps_for_rand_exp_sampling(self)
      cts, dscr, probs = self.hp_sampler(self._lml_batch, self.hp_tune_max_evals)
      return cts, dscr, [None] * len(cts), probs

  return BatchedEuclideanGPFitter


class _CPKernelMeanNoise(object):
  """ _KernelMeanNoise with CPGP's constructor signature (gp/cartesian_product_gp.py:211-213): what the CP fitter's
      build_gp hands to its GP, kept and nothing else. """
  __slots__ = ('kernel', 'mean_func', 'noise_var', 'handle_non_psd_kernels', 'host_kernel')

  def __init__(self, X, Y, kernel, mean_func, noise_var, domain_lists_of_dists=None, build_posterior=True, reporter=None,
               handle_non_psd_kernels='project_first'):
    # pylint: disable=unused-argument
    if build_posterior:
      raise RuntimeError('dragonfly_amd.install: the candidate stand-in was asked for a real GP')
    self.kernel, self.mean_func, self.noise_var = kernel, mean_func, noise_var
    self.handle_non_psd_kernels = handle_non_psd_kernels
    from .kernel import CartesianProductKernel
    # (cartesian_product_gp._uses_descriptor: our mirror, every part described, no part given by distances)
    self.host_kernel = not (isinstance(kernel, CartesianProductKernel) and kernel.has_device_spec() and
                            all(dists is None for dists in domain_lists_of_dists or []))


class _CPMFKernelMeanNoise(object):
  """ The same with CPMFGP's constructor signature (gp/cartesian_product_gp.py:254-258): the joint kernel is composed
      as that constructor composes it, from our mirror. """
  __slots__ = ('kernel', 'mean_func', 'noise_var', 'handle_non_psd_kernels', 'host_kernel')

  def __init__(self, ZZ, XX, YY, mf_kernel, mean_func, noise_var, kernel_scale=None, fidel_space_kernel=None,
               domain_kernel=None, fidel_space_lists_of_dists=None, domain_lists_of_dists=None, build_posterior=True,
               reporter=None, handle_non_psd_kernels='project_first'):
    # pylint: disable=unused-argument
    if build_posterior:
      raise RuntimeError('dragonfly_amd.install: the candidate stand-in was asked for a real GP')
    from .kernel import CartesianProductKernel
    described = mf_kernel is None and isinstance(fidel_space_kernel, CartesianProductKernel) and \
                isinstance(domain_kernel, CartesianProductKernel)
    if described:
      mf_kernel = CartesianProductKernel(kernel_scale, [fidel_space_kernel, domain_kernel])
    self.kernel, self.mean_func, self.noise_var = mf_kernel, mean_func, noise_var
    self.handle_non_psd_kernels = handle_non_psd_kernels
    # (cartesian_product_gp._uses_mf_descriptor)
    self.host_kernel = not (described and mf_kernel.has_device_spec() and
                            all(dists is None for dists in fidel_space_lists_of_dists or []) and
                            all(dists is None for dists in domain_lists_of_dists or []))


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
  from . import parallel
  from .engine import get_engine
  base = make_batched_fitter(ref_fitter_cls, tuning_gpus=tuning_gpus)

  class BatchedCPGPFitter(base):
    """ dragonfly.gp.cartesian_product_gp.CPGPFitter with batched ML tuning (dragonfly_amd.install). """

    def _decode_candidates(self, cts_hps_list, dscr_hps, per_cand, other_gp_params):
      return None                    # (the short cut of the Euclidean fitter's own factory does not apply)

    def _packed_points(self, kernel):
      cached = getattr(self, '_amd_packed', None)
      if cached is None or cached[0] is not self.X or cached[1] != len(self.X):
        cached = self._amd_packed = (self.X, len(self.X), get_engine().to_device(kernel.pack(self.X)))
      return cached[2]

    def _lml_batch(self, cts_hps_list, dscr_hps, other_gp_params=None):
      per_cand = len(dscr_hps) > 0 and isinstance(dscr_hps[0], (list, tuple, np.ndarray))
      if len(cts_hps_list) == 0:
        return np.zeros((0,))
      user_mean = getattr(self.options, 'mean_func', None) is not None
      import dragonfly.gp.cartesian_product_gp as _ref_cpgp
      saved_cls = getattr(_ref_cpgp, gp_name)
      setattr(_ref_cpgp, gp_name, stand_in)
      specs, means, noises, mode, first_kernel = [], [], [], None, None
      try:
        for i, cts in enumerate(cts_hps_list):
          dscr = list(dscr_hps[i]) if per_cand else list(dscr_hps)
          gp = self.build_gp(cts, dscr, other_gp_params=other_gp_params, build_posterior=False)
          if user_mean or getattr(gp, 'host_kernel', True) or (mode is not None and gp.handle_non_psd_kernels != mode):
            specs = None
            break
          mode = gp.handle_non_psd_kernels
          first_kernel = first_kernel or gp.kernel
          specs.append(gp.kernel.to_spec())
          means.append(float(gp.mean_func([self.X[0]])[0]))
          noises.append(float(gp.noise_var))
      finally:
        setattr(_ref_cpgp, gp_name, saved_cls)
      if specs is None:
        # an arbitrary mean function, or a kernel the host evaluates: one fit per candidate
        return np.array([self._tuning_objective(c, list(dscr_hps[j]) if per_cand else list(dscr_hps),
                                                other_gp_params=other_gp_params)
                         for j, c in enumerate(cts_hps_list)])
      multi = parallel.tuning_route(tuning_gpus, len(specs), len(self.X))
      if multi is not None:
        packed = parallel.per_rank_inputs(self, multi, lambda: first_kernel.pack(self.X), self.X)
        lmls = multi.gp_lml_batch(specs, packed, self._labels_array(), means, noises, handle_non_psd_kernels=mode)
      else:
        lmls = get_engine().gp_lml_batch(specs, self._packed_points(first_kernel), self._labels_array(), means, noises,
                                         handle_non_psd_kernels=mode)
      if gaplog.ENABLED and len(lmls) >= 16:
        gaplog.top2('hp_batch', lmls)
      return lmls

    def _optimise_cts_hps_for_given_dscr_hps(self, given_dscr_hps):
      """ gp_core.py:576-583 with the batch objective. """
      if not getattr(self, '_batched_ml', False):
        return ref_fitter_cls._optimise_cts_hps_for_given_dscr_hps(self, given_dscr_hps)
      objective = lambda arg: self._lml_batch(arg, list(given_dscr_hps))
      val, cts_hps, _ = self.cts_hp_optimise(objective, self.hp_tune_max_evals)
      return val, cts_hps, None

    def _sample_cts_dscr_hps_for_rand_exp_sampling(self):
      """ gp_core.py:585-590 with the batch objective. """
      if not getattr(self, '_batched_ml', False):
        return ref_fitter_cls._sample_cts_dscr_hps_for_rand_exp_sampling(self)
      cts, dscr, probs = self.hp_sampler(self._lml_batch, self.hp_tune_max_evals)
      return cts, dscr, [None] * len(cts), probs

  return BatchedCPGPFitter


def uninstall():
  """ Restores every name install() rebound. """
  from . import gpb_acquisitions, parallel
  for obj, name, old in reversed(_saved):
    setattr(obj, name, old)
  del _saved[:]
  parallel.close_tuning_engines()
  gpb_acquisitions.external_maximise_with_method = None
