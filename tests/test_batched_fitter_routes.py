"""dragonfly_amd.batched_fitter: where the one candidate loop (_candidates_by_build_gp) sends a tuning batch, for the
Euclidean and the Cartesian-product fitter at n = 8 -- one engine call with every candidate's (spec, mean, noise), or
one fit per candidate -- and that the reference module's GP global, bound to a stand-in while the candidates are walked,
is the installed class again afterwards, whatever happened in between.  The engine is the CPU stand-in with its
gp_lml_batch recorded; the expected triples come from GPs the fitter's build_gp makes outside the walk (the real
mirror classes).  CPU, needs the reference tree."""
import contextlib
import importlib.util
import os
import warnings

import numpy as np
import pytest

from oracle_engine_cp import patch_engine_cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')),
                                reason='needs the reference tree (build container only)')

N, DIM, NUM_CANDS = 8, 3, 5


def _cp_data():
  spec = importlib.util.spec_from_file_location('make_cp_golden', os.path.join(ROOT, 'tools', 'make_cp_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _euclidean_fitter():
  import dragonfly.opt.gp_bandit as GB
  from dragonfly.gp.euclidean_gp import euclidean_gp_args
  from dragonfly.utils.option_handler import load_options
  rs = np.random.RandomState(3)
  X = [rs.rand(DIM) for _ in range(N)]
  Y = [float(np.sin(3 * x).sum() + 0.1 * rs.randn()) for x in X]
  fitter = GB.EuclideanGPFitter(X, Y, options=load_options(euclidean_gp_args, partial_options={'kernel_type': 'se'}))
  fitter._set_up()                                        # pylint: disable=protected-access
  fitter._amd_decode = {'ok': False, 'checks': 3}         # the decode short cut off: every batch takes the candidate loop
  import dragonfly.gp.euclidean_gp as ref_module
  expected = lambda gp: (gp.kernel.to_spec(DIM).signature(), float(gp.mean_func([np.zeros(DIM)])[0]), float(gp.noise_var))
  return fitter, ref_module, 'EuclideanGP', expected, {}


def _cp_fitter():
  import dragonfly.opt.gp_bandit as GB
  from dragonfly.exd import domains
  G = _cp_data()
  X, Y = G.fitter_data(N)
  fitter = GB.CPGPFitter(X, Y, G.fitter_domain(domains), domain_kernel_ordering=['', '', ''], options=G.fitter_options())
  import dragonfly.gp.cartesian_product_gp as ref_module
  expected = lambda gp: (gp.kernel.to_spec().signature(), float(gp.mean_func([X[0]])[0]), float(gp.noise_var))
  return fitter, ref_module, 'CPGP', expected, {'handle_non_psd_kernels': 'project_first'}


def _candidates(fitter):
  rs = np.random.RandomState(11)
  lo = np.array([b[0] for b in fitter.cts_hp_bounds], dtype=float)
  hi = np.array([b[1] for b in fitter.cts_hp_bounds], dtype=float)
  cts = [lo + (hi - lo) * rs.rand(len(lo)) for _ in range(NUM_CANDS)]
  dscr = [[vals[rs.randint(len(vals))] for vals in fitter.dscr_hp_vals] for _ in range(NUM_CANDS)]
  return cts, dscr


@contextlib.contextmanager
def _odd_one_out(fitter, **fields):
  """ the stand-in of the fitter's class, with `fields` set on the third object made: the candidate in the middle """
  cls = type(fitter)
  base = cls.stand_in

  class OddOneOut(base):
    __slots__ = ()
    made = 0

    def __init__(self, *args, **kwargs):
      base.__init__(self, *args, **kwargs)
      OddOneOut.made += 1
      if OddOneOut.made == 3:
        for name, value in fields.items():
          setattr(self, name, value)
  cls.stand_in = OddOneOut
  try:
    yield OddOneOut
  finally:
    cls.stand_in = base


@pytest.mark.parametrize('make', [_euclidean_fitter, _cp_fitter], ids=['euclidean', 'cartesian_product'])
def test_candidate_loop_routes(make, monkeypatch):
  from oracle.make_golden import import_reference
  import_reference()
  eng = patch_engine_cp(monkeypatch)
  engine_calls, own_fits = [], []

  def gp_lml_batch(specs, X, y, mean_consts, noise_vars, **keywords):
    engine_calls.append(([s.signature() for s in specs], list(mean_consts), list(noise_vars), np.shape(X), keywords))
    return np.arange(len(specs), dtype=float)
  monkeypatch.setattr(eng, 'gp_lml_batch', gp_lml_batch, raising=False)
  from dragonfly_amd import install
  install.install(cartesian_product=True)
  try:
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      fitter, ref_module, gp_name, expected, keywords = make()
    installed = getattr(ref_module, gp_name)
    cts, dscr = _candidates(fitter)

    def own_fit(self, cts_hps, dscr_hps, other_gp_params=None):
      own_fits.append((list(cts_hps), list(dscr_hps)))
      return float(len(own_fits))
    monkeypatch.setattr(type(fitter), '_tuning_objective', own_fit)

    def route(dscr_hps=dscr):
      """ (engine calls, own fits) of one _lml_batch over the candidates; the GP global must be back afterwards """
      del engine_calls[:], own_fits[:]
      lmls = fitter._lml_batch(cts, dscr_hps)             # pylint: disable=protected-access
      assert getattr(ref_module, gp_name) is installed and len(lmls) == NUM_CANDS
      return list(engine_calls), list(own_fits)
    each_on_its_own = ([], [(list(c), list(d)) for c, d in zip(cts, dscr)])

    # every candidate on the device: exactly one engine call, with what build_gp makes of each candidate
    want = [expected(fitter.build_gp(c, list(d), build_posterior=False)) for c, d in zip(cts, dscr)]
    calls, fits = route()
    assert fits == [] and len(calls) == 1
    specs, means, noises, shape, got_keywords = calls[0]
    assert list(zip(specs, means, noises)) == want and shape[0] == N and got_keywords == keywords
    # ... and the same with one discrete row for all candidates
    calls, fits = route(dscr[0])
    assert fits == [] and len(calls) == 1 and calls[0][0] == [expected(fitter.build_gp(c, list(dscr[0]), build_posterior=False))[0]
                                                              for c in cts]
    assert fitter._lml_batch([], dscr).shape == (0,) and engine_calls == calls     # pylint: disable=protected-access

    # a candidate in the middle whose kernel the host evaluates: one fit per candidate, no engine call
    with _odd_one_out(fitter, host_kernel=True) as odd:
      assert route() == each_on_its_own and odd.made == 3
    if gp_name == 'CPGP':
      # ... and one with another handle_non_psd_kernels than the candidates before it
      with _odd_one_out(fitter, handle_non_psd_kernels='try_before_project') as odd:
        assert route() == each_on_its_own and odd.made == 3

    # a user's mean function: one fit per candidate, no engine call
    fitter.options.mean_func = lambda x: np.zeros(len(x))
    assert route() == each_on_its_own
    fitter.options.mean_func = None

    # build_gp raises at the second candidate: the error reaches the caller and the global is still put back
    built = []

    def failing_build_gp(*args, **kwargs):
      built.append(getattr(ref_module, gp_name))
      if len(built) == 2:
        raise RuntimeError('build_gp failed')
      return type(fitter).build_gp(fitter, *args, **kwargs)
    fitter.build_gp = failing_build_gp
    del engine_calls[:], own_fits[:]
    with pytest.raises(RuntimeError, match='build_gp failed'):
      fitter._lml_batch(cts, dscr)                        # pylint: disable=protected-access
    assert built == [type(fitter).stand_in] * 2 and getattr(ref_module, gp_name) is installed
    assert engine_calls == [] and own_fits == []
  finally:
    install.uninstall()
