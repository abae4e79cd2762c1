"""Fluxes and radiances by scattering order (recScatOrd) on the MI355X: per photon against the oracle's fates, exact
closure over the orders, the orders of an isotropic slab against the Neumann series of its integral equation, the same bits
whatever the schedule, nothing changed when the orders are off, and the rules of specifyParameters."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import expn

from tests import cases
from tests.test_analytic import RADIANCE_MUS, RADIANCE_PHIS, thermal_case

pytestmark = pytest.mark.gpu

SEED = 20240917


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integ(M, case, mu0=1.0, phi0=0.0, nsteps=10001, **params):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=nsteps, useRayTracing=True, useRussianRoulette=True, **params)
    photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
    return dom, integ, photons, new_RandomNumberSequence(SEED)


def _stats(integ, dom):
    from mcbrat3d_amd import driver
    return driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ,
                                                   integ.numIntensityDirections(), integ.numRecScatOrd))


# ---- 4. per photon against the oracle ----------------------------------------------------------------------------------
def test_step_cloud_orders_match_the_oracle_fates(M):
    """fluxUpByScatOrd is the histogram of the top exits by (column, nScatter); under a black surface the arrival is the
    photon's last event and its fate records nScatter after the reflection's increment, so fluxDownByScatOrd is the
    histogram of the surface fates by (column, nScatter - 1)."""
    from oracle import oracle as O
    n, N = 100000, 8
    case = cases.step_cloud(ssa=0.99)
    dom, integ, photons, rng = _integ(M, case, recScatOrd=True, numRecScatOrd=N)
    assert integ.computeRadiativeTransfer(dom, rng, photons, n) == n
    got = integ.reportResults()
    assert integ.badPhotons() == 0
    f = O.compute_rt(cases.oracle_problem(case), O.solar_source(1.0, 0.0), O.philox_rng(SEED, 0), n, want_fates=True)["fates"]
    nppc = n / 32.0
    tol_col = 8.0 * 32 / n  # a handful of flipped photons per column, as test_gpu_parity's batch test allows
    for fate, shift, key in ((0, 0, "fluxUpByScatOrd"), (1, 1, "fluxDownByScatOrd")):
        sel = f["fate"] == fate
        order = f["nScatter"][sel] - shift
        keep = order <= N
        want = np.zeros((32, N + 1))
        np.add.at(want, (f["ix"][sel][keep] - 1, order[keep]), f["weight"][sel][keep].astype(np.float64))
        want /= nppc
        assert got[key].shape == (32, 1, N + 1)
        assert np.max(np.abs(got[key][:, 0, :] - want)) < tol_col, key
        assert np.allclose(got["mean" + key[0].upper() + key[1:]], want.mean(axis=0), atol=8.0 / n + 2e-6), key
    assert np.all(got["fluxUpByScatOrd"][:, :, 0] == 0.0)  # nothing leaves the top unscattered under a zenith sun


# ---- 5. exact closure --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("withRadiance", [False, True])
def test_orders_sum_to_the_totals(M, withRadiance):
    """A slab in which no photon scatters more than N times: the orders add up to the totals (integer tallies: the sums
    differ by float rounding only).  On the thick step cloud the partial sums stay below the totals in every column."""
    rad = dict(minForwardTableSize=1801, intensityMus=RADIANCE_MUS, intensityPhis=RADIANCE_PHIS, computeIntensity=True) \
        if withRadiance else {}
    case = cases.plane_parallel(ssa=0.5, tau=0.5, nz=8, g=0.0, nleg=2)
    dom, integ, photons, rng = _integ(M, case, 0.6, 20.0, recScatOrd=True, numRecScatOrd=60, **rad)
    integ.computeRadiativeTransfer(dom, rng, photons, 200000)
    r = integ.reportResults()
    for k in ("fluxUp", "fluxDown"):
        s = r[k + "ByScatOrd"].astype(np.float64).sum(axis=-1)
        assert np.allclose(s, r[k], rtol=2e-5, atol=1e-7), k
        assert abs(r["mean" + k[0].upper() + k[1:] + "ByScatOrd"].astype(np.float64).sum() - r["mean" + k[0].upper() + k[1:]]) < 1e-5
    if withRadiance:
        s = r["intensityByScatOrd"].astype(np.float64).sum(axis=-1)
        assert np.allclose(s, r["intensity"], rtol=2e-5, atol=1e-7)
        assert np.allclose(r["meanIntensityByScatOrd"].astype(np.float64).sum(axis=-1), r["meanIntensity"], rtol=2e-5, atol=1e-7)
    integ.finalize()
    # thick: partial sums
    dom, integ, photons, rng = _integ(M, cases.step_cloud(ssa=0.99), recScatOrd=True, numRecScatOrd=3, **rad)
    integ.computeRadiativeTransfer(dom, rng, photons, 100000)
    r = integ.reportResults()
    for k in ("fluxUp", "fluxDown") + (("intensity",) if withRadiance else ()):
        s = r[k + "ByScatOrd"].astype(np.float64).sum(axis=-1)
        assert np.all(s <= r[k] * (1 + 2e-5) + 1e-7), k
    assert r["fluxUpByScatOrd"].sum() < 0.95 * r["fluxUp"].sum()  # (the orders above 3 carry much of the step cloud's reflection)


# ---- 6. theory ---------------------------------------------------------------------------------------------------------
def neumann_orders(b, omega, mu0, orders, mus=(), cells=1500):
    """The Neumann series of test_analytic.isotropic_slab's discretisation: S_1 = omega direct, S_{k+1} = omega K S_k.
    Returns up[k], down[k] (k = 0..orders, down[0] the direct beam) and the radiance rad[k, mu] leaving the top."""
    h = b / cells
    edges = np.arange(cells + 1) * h
    tc = edges[:-1] + 0.5 * h
    kern = 0.5 * np.abs(expn(2, np.abs(tc[:, None] - edges[None, :-1])) - expn(2, np.abs(tc[:, None] - edges[None, 1:])))
    kern[np.arange(cells), np.arange(cells)] = 1.0 - expn(2, 0.5 * h)
    direct = (np.exp(-edges[:-1] / mu0) - np.exp(-edges[1:] / mu0)) / (4.0 * np.pi * h)
    up, down = np.zeros(orders + 1), np.zeros(orders + 1)
    rad = np.zeros((orders + 1, len(mus)))
    down[0] = np.exp(-b / mu0)
    s = omega * direct
    for k in range(1, orders + 1):
        up[k] = 2.0 * np.pi * float(np.sum(s * (expn(3, edges[:-1]) - expn(3, edges[1:]))))
        down[k] = 2.0 * np.pi * float(np.sum(s * (expn(3, b - edges[1:]) - expn(3, b - edges[:-1]))))
        rad[k] = [float(np.sum(s * (np.exp(-edges[:-1] / m) - np.exp(-edges[1:] / m)))) for m in mus]
        s = omega * (kern @ s)
    return up, down, rad


def single_scatter_radiance(b, omega, mu0, mu):
    """Order 1 in closed form, per unit incident flux on the horizontal (the normalisation of test_analytic's radiances):
    omega / (4 pi (mu0 + mu)) (1 - exp(-b (1/mu0 + 1/mu))); per unit irradiance normal to the beam it carries a factor mu0."""
    return omega / (4.0 * np.pi * (mu0 + mu)) * (1.0 - np.exp(-b * (1.0 / mu0 + 1.0 / mu)))


def test_the_neumann_series_adds_up_to_the_integral_equation():
    from tests.test_analytic import isotropic_radiance, isotropic_slab
    b, omega, mu0 = 1.0, 0.9, 0.6
    up, down, rad = neumann_orders(b, omega, mu0, 200, RADIANCE_MUS)
    u, d, direct = isotropic_slab(b, omega, mu0)
    assert abs(up.sum() - u) < 1e-6 and abs(down.sum() - d - direct) < 1e-6
    assert np.allclose(rad.sum(axis=0), isotropic_radiance(b, omega, mu0, RADIANCE_MUS), rtol=1e-6)
    assert np.allclose(rad[1], [single_scatter_radiance(b, omega, mu0, m) for m in RADIANCE_MUS], rtol=2e-4)


@pytest.mark.parametrize("b,omega,mu0", [(1.0, 0.9, 0.6), (2.0, 1.0, 1.0)])
def test_isotropic_slab_orders_against_the_neumann_series(M, b, omega, mu0):
    case = cases.plane_parallel(ssa=omega, tau=b, nz=16, g=0.0, nleg=2)
    case["albedo"] = 0.0
    dom, integ, photons, rng = _integ(M, case, mu0, 33.0, nsteps=9001, minForwardTableSize=1801, intensityMus=RADIANCE_MUS,
                                      intensityPhis=RADIANCE_PHIS, computeIntensity=True, useRussianRouletteForIntensity=False,
                                      recScatOrd=True, numRecScatOrd=5)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, rng, photons, 100000, 40) == 4000000
    st = _stats(integ, dom)
    assert integ.badPhotons() == 0
    integ.finalize()
    up, down, rad = neumann_orders(b, omega, mu0, 5, RADIANCE_MUS)
    assert st["meanFluxUpByScatOrd"][0] == 0.0
    for k in range(4):
        for name, theory in (("meanFluxUpByScatOrd", up[k]), ("meanFluxDownByScatOrd", down[k])):
            mean, err = st[name][k], st[name + "_StdErr"][k]
            assert abs(mean - theory) < 5.0 * err + 2e-6, (name, k, mean, theory, err)
    for k in (1, 2):
        mean, err = st["intensityByScatOrd"][0, 0, :, k], st["intensityByScatOrd_StdErr"][0, 0, :, k]
        assert np.all(np.abs(mean - rad[k]) < 5.0 * err + 1e-6), (k, mean, rad[k], err)
    closed = np.array([single_scatter_radiance(b, omega, mu0, m) for m in RADIANCE_MUS])
    mean, err = st["intensityByScatOrd"][0, 0, :, 1], st["intensityByScatOrd_StdErr"][0, 0, :, 1]
    assert np.all(np.abs(mean - closed) < 5.0 * err + 2e-4 * closed), (mean, closed, err)


def test_thermal_radiance_without_scattering_is_all_order_zero(M):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case, _, _, _ = thermal_case(1.0, 0.0, [285.0, 270.0, 255.0, 240.0], 290.0)
    dom = cases.product_domain(case)
    w = M.new_Weights(4, 4, 4)
    M.emission_weighting(dom, w, 290.0)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=101, minForwardTableSize=181, LW_flag=1.0, intensityMus=RADIANCE_MUS,
                            intensityPhis=RADIANCE_PHIS, computeIntensity=True, recScatOrd=True, numRecScatOrd=2)
    photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 200000)
    r = integ.reportResults()
    integ.finalize()
    assert r["intensity"].max() > 0.0
    assert np.array_equal(r["intensityByScatOrd"][..., 0], r["intensity"])
    assert not np.any(r["intensityByScatOrd"][..., 1:])
    assert np.array_equal(r["meanIntensityByScatOrd"][:, 0], r["meanIntensity"].astype(np.float32)) or \
        np.allclose(r["meanIntensityByScatOrd"][:, 0], r["meanIntensity"], rtol=1e-6)
    assert np.array_equal(r["fluxUpByScatOrd"][..., 0], r["fluxUp"])


# ---- 7. the same bits whatever the schedule ----------------------------------------------------------------------------
def _run(M, case, nDirs, tuning=None, calls=1, asyncOn=False, N=6):
    rad = dict(minForwardTableSize=1801, intensityMus=RADIANCE_MUS[:nDirs], intensityPhis=RADIANCE_PHIS[:nDirs],
               computeIntensity=True) if nDirs else {}
    dom, integ, photons, rng = _integ(M, case, 0.7, 40.0, recScatOrd=True, numRecScatOrd=N, **rad)
    if tuning:
        integ.setTuning(**tuning)
    if asyncOn:
        integ.setAsync(True)
    integ.resetMoments()
    for _ in range(calls):
        integ.computeRadiativeTransfer(dom, rng, photons, 20000, 10 // calls)
    integ.synchronize()
    m = integ.moments()
    integ.finalize()
    return m


@pytest.mark.parametrize("nDirs", [0, 2])
def test_order_moments_do_not_depend_on_the_schedule(M, nDirs):
    case = cases.step_cloud(ssa=0.99)
    ref = _run(M, case, nDirs)
    assert ref[0] == 200000
    for kw in (dict(tuning=dict(layerSkip=0)), dict(tuning=dict(layerSkip=2)), dict(tuning=dict(layerSkip=1)),
               dict(tuning=dict(privateTallies=0)), dict(calls=10), dict(asyncOn=True), dict(asyncOn=True, calls=10)):
        got = _run(M, case, nDirs, **kw)
        assert np.array_equal(got, ref), kw


def test_large_domain_global_tallies_match_private_ones_on_a_cut(M):
    """128x128x64 with radiance and orders: global atomics (private tallies do not fit) in one call of 4 batches and in 4
    calls: the same bits; N = 100 fits the tally budget there."""
    case = cases.landsat_like()
    rad = dict(minForwardTableSize=1801, intensityMus=RADIANCE_MUS[:2], intensityPhis=RADIANCE_PHIS[:2], computeIntensity=True)
    out = []
    for calls in (1, 4):
        dom, integ, photons, rng = _integ(M, case, 0.5, 30.0, recScatOrd=True, numRecScatOrd=100, **rad)
        integ.resetMoments()
        for _ in range(calls):
            integ.computeRadiativeTransfer(dom, rng, photons, 25000, 4 // calls)
        mode = integ.walkMode()  # (the plan of the loaded domain)
        assert not mode["blockWalk"] and not mode["widePlan"] and not mode["privateTallies"]
        out.append(integ.moments())
        r = integ.reportResults()
        assert r["fluxUpByScatOrd"].shape == (128, 128, 101) and r["intensityByScatOrd"].shape == (128, 128, 2, 101)
        integ.finalize()
    assert np.array_equal(out[0], out[1])


# ---- 8. nothing changes when off ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nDirs", [0, 2])
def test_orders_off_after_a_round_trip_changes_nothing(M, nDirs):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = cases.step_cloud(ssa=0.99)
    rad = dict(minForwardTableSize=1801, intensityMus=RADIANCE_MUS[:nDirs], intensityPhis=RADIANCE_PHIS[:nDirs],
               computeIntensity=True) if nDirs else {}
    dom, integ, photons, _ = _integ(M, case, **rad)

    def once():
        integ.resetMoments()
        integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 20000, 5)
        return integ.moments()

    before = once()
    length, mode = integ.momentsLength(), integ._lib.mcbrat_get_walk_mode(integ._ctx)  # (with the optics loaded: the plan's bits)
    assert nDirs > 0 or integ.walkMode()["blockWalk"]
    integ.specifyParameters(numRecScatOrd=4)
    assert integ.momentsLength() > length
    if nDirs == 0:
        assert not integ.walkMode()["blockWalk"]  # (the block walk has no order tallies)
    with_orders = once()
    integ.specifyParameters(numRecScatOrd=-1)
    assert integ.momentsLength() == length and integ._lib.mcbrat_get_walk_mode(integ._ctx) == mode
    after = once()
    assert np.array_equal(before, after)
    assert "fluxUpByScatOrd" not in integ.reportResults()
    # the order-blind part of the run with orders is that of the face-by-face walk (the block walk has no ORD variant): the
    # same photons, the same integer tallies, the same bits
    integ.setTuning(blockWalk=0)
    plain = once()
    M1, M2 = (len(plain) - 8) // 2, (len(with_orders) - 8) // 2
    assert np.array_equal(with_orders[:8], plain[:8])
    assert np.array_equal(with_orders[8:8 + M1], plain[8:8 + M1])
    assert np.array_equal(with_orders[8 + M2:8 + M2 + M1], plain[8 + M1:])
    integ.finalize()


# ---- 9. the rules of specifyParameters ---------------------------------------------------------------------------------
def test_specify_parameters_rules(M):
    from mcbrat3d_amd._capi import McbratError
    case = cases.step_cloud(ssa=0.99)
    dom, integ, photons, rng = _integ(M, case)
    length = integ.momentsLength()
    with pytest.raises(McbratError, match="set recScatOrd to true, but did not provide number of orders to track"):
        integ.specifyParameters(recScatOrd=True)
    integ.specifyParameters(recScatOrd=True, numRecScatOrd=-2)  # negative: nothing recorded
    assert integ.numRecScatOrd == -1 and integ.momentsLength() == length
    integ.computeRadiativeTransfer(dom, rng, photons, 10000)
    assert not any("ScatOrd" in k for k in integ.reportResults())
    integ.specifyParameters(numRecScatOrd=2)
    assert integ.numRecScatOrd == 2 and integ.recScatOrd
    integ.specifyParameters(recScatOrd=False)
    assert integ.numRecScatOrd == -1
    integ.specifyParameters(intensityMus=RADIANCE_MUS, intensityPhis=RADIANCE_PHIS, computeIntensity=True, numRecScatOrd=3)
    with pytest.raises(McbratError, match="limitIntensityContributions"):
        integ.specifyParameters(limitIntensityContributions=True, maxIntensityContribution=5.0)
    integ.specifyParameters(numRecScatOrd=-1)
    integ.specifyParameters(limitIntensityContributions=True, maxIntensityContribution=5.0)
    with pytest.raises(McbratError, match="limitIntensityContributions"):
        integ.specifyParameters(numRecScatOrd=3)
    with pytest.raises(McbratError, match="limitIntensityContributions"):  # the library refuses it too
        integ._check(integ._lib.mcbrat_specify_scattering_orders(integ._ctx, 3))
    integ.specifyParameters(limitIntensityContributions=False, numRecScatOrd=3)
    integ.computeRadiativeTransfer(dom, rng, photons, 10000)
    r = integ.reportResults()
    assert r["fluxUpByScatOrd"].shape == r["fluxDownByScatOrd"].shape == (32, 1, 4)
    assert r["meanFluxUpByScatOrd"].shape == (4,) and r["meanIntensityByScatOrd"].shape == (3, 4)
    assert r["intensityByScatOrd"].shape == (32, 1, 3, 4)
    with pytest.raises(McbratError, match="too large"):  # the memory budget, not an allocation error
        integ.specifyParameters(numRecScatOrd=10 ** 8)
    integ.finalize()


def test_spectral_run_and_counters_refuse_orders(M):
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    case = cases.step_cloud(ssa=0.99)
    with pytest.raises(McbratError, match="scattering order"):
        broadband.SpectralRun(M, [cases.product_domain(case)], numRecScatOrd=2)
    dom, integ, photons, rng = _integ(M, case, recScatOrd=True, numRecScatOrd=2)
    integ.enableCounters(True)
    with pytest.raises(McbratError, match="scattering orders"):
        integ.computeRadiativeTransfer(dom, rng, photons, 10000)
    integ.finalize()


def test_fortran_driver_prints_the_python_means_by_order(M, tmp_path):
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from mcbrat3d_amd import flatdomain
    fdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fortran")
    if shutil.which("amdflang") is None and not os.path.exists(os.path.join(fdir, "mcbrat_driver")):
        pytest.skip("no Fortran compiler on this box and no prebuilt driver")
    if shutil.which("amdflang") is not None:
        subprocess.check_call(["make", "-C", fdir], stdout=subprocess.DEVNULL)
    ppb, nb, N = 50000, 8, 3
    case = cases.step_cloud(0.99)
    dom = cases.product_domain(case)
    flat = flatdomain.write_flat_domain(str(tmp_path / "step.flat"), dom)
    nml = tmp_path / "o.nml"
    nml.write_text("""&radiativeTransfer
  solarMu = 1.0, solarAzimuth = 0.0 /
&monteCarlo
  numPhotonsPerBatch = %d, numBatches = %d, iseed = 10, nPhaseIntervals = 10001 /
&algorithms
  useRayTracing = .true., useRussianRoulette = .true. /
&output
  recScatOrd = .true., numRecScatOrd = %d /
&fileNames
  physDomainFile = "%s" /
""" % (ppb, nb, N, flat))
    out = subprocess.check_output([os.path.join(fdir, "mcbrat_driver"), str(nml)], text=True, cwd=str(tmp_path))
    rows = re.findall(r"order\s+(\d+) mean flux up/down:\s+([-\d.]+) \+-\s*([-\d.]+)\s+([-\d.]+) \+-\s*([-\d.]+)", out)
    assert len(rows) == N + 1, out
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, useRayTracing=True, useRussianRoulette=True, recScatOrd=True, numRecScatOrd=N)
    photons = M.new_PhotonStream(1.0, 0.0, numberOfPhotons=10 ** 9)
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(10), photons, ppb, nb)
    st = driver.statistics(driver.unpack_moments(integ.moments(), 32, 1, 32, 0, N))
    integ.finalize()
    for p, u, ue, d, de in rows:
        p = int(p)
        want = [st["meanFluxUpByScatOrd"][p], st["meanFluxUpByScatOrd_StdErr"][p],
                st["meanFluxDownByScatOrd"][p], st["meanFluxDownByScatOrd_StdErr"][p]]
        assert np.allclose([float(u), float(ue), float(d), float(de)], want, atol=1.5e-6), (p, want)
