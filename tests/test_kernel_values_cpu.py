"""The reference side of tests/test_gpu_kernel_values.py, without a device: on the whole case table of
tests/kernel_value_check.py the inputs are on their lattice, exactly; the oracle's dist_squared equals the squared
distance computed in integers, bit for bit; the truth alone reaches every band (arg < 1, normal, subnormal, exactly
zero) with at least 50 entries; and the NumPy oracle is as close to the long-double truth as the bounds of the device
tests assume -- 2 ulp for SE, 3 (1 + arg) ulp for Matern where gfac exp(-arg) is a normal number.  In the tail the
oracle rounds gfac exp(-arg) into a subnormal before the Matern polynomial multiplies it: there it is held to
3 (1 + arg) ulp plus one unit of 2^-1074 times that multiplier, scale u(mult).

The acquisition sweep: ld_acq_truth against scipy.special.ndtr within 4 (1 + z^2) ulp where Phi is a normal double.
x = z / sqrt 2 carries 1.5 ulp (the constant, the product); through erfc's conditioning 2 x^2 = z^2 that is 1.5 z^2 ulp,
plus 2 ulp for cephes' erfc and 0.5 for the truth's rounding to double.  The worst point is the other branch, at the
seam: 0.5 + 0.5 erf(x) with x just above -1 is 0.079 from an erf of 0.84, so erf's 2 ulp and x's 0.62 ulp-of-erf come
to (2.62 / 2) 2^-53 = 10.5 ulp of the result, 11.5 with the sum's and the truth's roundings, over 1 + z^2 = 3: 3.8.
Below that range scipy's ndtr is within the same bound or exactly 0 (cephes' underflow guard at z^2 / 2 > 709.78)."""
import math

import numpy as np
import pytest
import scipy.special

import acq_tail_check as A
import kernel_value_check as V
from oracle import ref_numpy as O

LD = np.longdouble
INPUTS = list({c[2:]: c for c in V.CASES}.values())          # the variants share their inputs


def test_table_names_every_route_but_colw_and_every_variant():
  assert V.routes_in_table() == [r for r in V.ROUTES if r not in ('colw', 'strip_mean')]
  assert set(c.variant for c in V.CASES) == set(V.VARIANTS)
  assert all(any(e.variant == c.variant and e.route == c.route for e in V.EDGE_CASES) for c in V.CASES)


@pytest.mark.parametrize('case', INPUTS, ids=V.case_id)
def test_lattice_is_exact_and_the_oracle_agrees_with_the_integers(case):
  ref = V.reference_of(case)
  X1 = ref.X2 if ref.X1 is None else ref.X1
  for X in (X1, ref.X2):
    k = X * 2.0 ** case.q
    assert np.all(k == np.rint(k)) and np.abs(X).max() <= case.span
  for part in V.parts_of(ref.spec):
    dsq_int, E = V.dsq_exact(part, X1, ref.X2)               # asserts 4 max sum s^2 < 2^53
    assert dsq_int.max() < 2 ** 53
    exact = np.ldexp(dsq_int.astype(np.float64), -2 * E)
    cols, bw = part[3], part[4]
    assert np.array_equal(O.dist_squared(X1[:, cols] / bw, ref.X2[:, cols] / bw), exact)


@pytest.mark.parametrize('case', [c for c in INPUTS if c.kernel == 'se' or c.kernel[0] == 'm'], ids=V.case_id)
def test_truth_reaches_every_band(case):
  bands = V.reference_of(case).bands
  assert all(bands[b] >= V.BAND_MIN for b in V.BANDS), bands


@pytest.mark.parametrize('case', INPUTS, ids=V.case_id)
def test_oracle_is_within_the_recorded_figures(case):
  ref = V.reference_of(case)
  V.assert_clean(ref.oracle, V.case_id(case))                 # what the device is asked, the reference does
  if case.kernel == 'se':
    assert max(ref.oracle_ulp.values()) <= 2.0, ref.oracle_ulp
  elif case.kernel[0] == 'm':
    assert ref.oracle_ulp['head'] <= 3.0, ref.oracle_ulp
    kind, scale, nu, _, _ = V.parts_of(ref.spec)[0]
    p = int(nu)
    gfac = LD(math.factorial(p)) / LD(math.factorial(2 * p))
    tail = ref.regions['tail']
    arg, truth = ref.arg_max[tail], ref.truth[tail]
    unit = LD(2.0) ** -1074
    allowed = 3 * (1 + arg) * np.spacing(np.abs(truth.astype(np.float64))).astype(LD) + unit * truth / (gfac * np.exp(-arg))
    assert np.all(np.abs(ref.oracle[tail].astype(LD) - truth) <= allowed)
  elif case.kernel.startswith('esp'):
    assert ref.oracle_ulp['head'] <= V.ESP_ORACLE_ULP[int(ref.spec.nu)] and 'tail' not in ref.regions, ref.oracle_ulp
  if not case.n1:
    assert np.array_equal(ref.oracle, ref.oracle.T)


def test_acquisition_truth_agrees_with_ndtr():
  z = np.concatenate([A.z_targets(), [np.nan]])
  rs = np.random.RandomState(5)
  sd = 0.01 + rs.random_sample(z.size)                        # a fixed synthetic mu and sigma: z as the device forms it
  mu = A.BEST + z * sd
  z = (mu - A.BEST) / sd
  Phi, ei_norm = A.T.acq_truth(z)
  assert np.isnan(Phi[-1]) and np.isnan(ei_norm[-1])
  z, sd, mu, Phi, ei_norm = z[:-1], sd[:-1], mu[:-1], Phi[:-1], ei_norm[:-1]
  assert Phi.min() == 0.0 and ((Phi > 0) & (Phi < 2.0 ** -1022)).sum() >= 10 and Phi.max() <= 1.0
  assert np.all(np.diff(Phi[np.argsort(z, kind='stable')]) >= 0) and np.all(ei_norm >= 0)
  head = Phi >= 2.0 ** -1022
  for oracle in (scipy.special.ndtr(z), O.acq_values('pi', mu, sd, A.BEST)):
    err = A.ulps(oracle, Phi, z)
    assert err[head].max() <= 4.0
    assert np.all((err[~head] <= 4.0) | ((oracle[~head] == 0.0) & (z[~head] ** 2 / 2 > 709.78)))
  # EI as the reference evaluates it: phi = exp(-z^2 / 2) carries the rounding of z^2 / 2, z^2 / 4 ulp, and z Phi + phi
  # cancels to ~1 / z^2 of its terms for z << 0 -- (1 + z^2)^2 ulp in all, although the function's own conditioning is
  # 1 + z^2.  The device's limit comes from this figure of the oracle, so it is recorded here where it is large.
  ei = sd.astype(LD) * ei_norm.astype(LD)
  ei_head = ei.astype(np.float64) >= 2.0 ** -1022
  assert (A.ulps(O.acq_values('ei', mu, sd, A.BEST), ei, z) / (1 + z * z))[ei_head & head].max() <= 4.0
