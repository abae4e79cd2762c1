"""Upward and downward flux through every level of every column (recLevelFluxes) on the GPU.

The checks of this file need no oracle: exact identities (the boundary levels are fluxUp / fluxDown bit for bit, nothing else
moves, the schedule does not show, the flux divergence of a layer is what it absorbed), closed forms (Beer-Lambert over a grey
surface) and a direct-beam ray-cast written here.  The oracle's own level tallies, and transport theory at the inner levels of
scattering media, are what tests/test_gpu_level_flux_oracle.py holds the same kernels to."""
import ctypes as C

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

SEED = 20250917
ISO = [np.zeros(2, np.float32)]  # isotropic scattering


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _medium(xe, ye, ze, ext, ssa, albedo, legendre=None):
    ext = np.asarray(ext, np.float64)
    return dict(name="levels", xe=np.asarray(xe, np.float64), ye=np.asarray(ye, np.float64), ze=np.asarray(ze, np.float64), albedo=albedo,
                components=[dict(ext=ext, ssa=np.full_like(ext, ssa), pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=legendre or [cases.hg_legendre(0.7, 24)])])


def solar_case():
    """3 x 2 x 4, unlike cells on irregular z levels, omega0 = 0.9, a Lambertian surface of unlike patches."""
    rng = np.random.default_rng(5)
    case = _medium([0.0, 0.05, 0.12, 0.15], [0.0, 0.08, 0.12], [0.0, 0.03, 0.08, 0.1, 0.16], rng.uniform(2.0, 25.0, (3, 2, 4)), 0.9, 0.0)
    return cases.patchy_surface(case, nxs=4, nys=3)


def thermal_case(nz=3, ssa=0.9):
    rng = np.random.default_rng(6)
    ze = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.15, nz))])
    case = _medium([0.0, 0.1, 0.2], [0.0, 0.1, 0.2], ze, rng.uniform(3.0, 20.0, (2, 2, nz)), ssa, 0.3)
    case.update(temps=rng.uniform(240.0, 300.0, (2, 2, nz)), sfc_temp=295.0, lambda_um=10.0)
    return case


def _integrator(M, case, rr=True, levels=True, thermal=False, tuning=None):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    surface = cases.product_surface(case)
    integ.specifyParameters(minInverseTableSize=9001, useRayTracing=True, useRussianRoulette=rr, LW_flag=1.0 if thermal else -1.0,
                            recLevelFluxes=levels, **({"surfaceBDRF": surface} if surface is not None else {}))
    integ.setTuning(**{"eventThreshold": 16, **(tuning or {})})
    if thermal:
        w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
        M.emission_weighting(dom, w, case["sfc_temp"])
        photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    else:
        photons = M.new_PhotonStream(case.get("mu0", 0.6), case.get("phi0", 30.0), numberOfPhotons=10 ** 12)
    return dom, integ, photons


def _moments(M, case, rr=True, levels=True, thermal=False, tuning=None, ppb=2000, batches=4):
    """The moment array of `batches` batches, unpacked: name -> (S1, S2); and the raw array."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, rr, levels, thermal, tuning)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, ppb, batches) == ppb * batches
    raw = integ.moments().copy()
    assert integ.badPhotons() == 0
    assert integ.momentsLength() * 2 + 8 == raw.size
    integ.finalize()
    return driver.unpack_moments(raw, dom.numX, dom.numY, dom.numZ, 0, -1, levelFluxes=levels), raw


CASES = [("solar, roulette", solar_case, True, False), ("solar, no roulette", solar_case, False, False),
         ("thermal", thermal_case, True, True)]


@pytest.fixture(scope="module")
def level_runs(M):
    """The level-flux run of every case, traced once and shared (never modified)."""
    return {name: _moments(M, make(), rr, True, thermal) for name, make, rr, thermal in CASES}


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_boundary_levels_are_fluxup_and_fluxdown_bit_for_bit(level_runs, name):
    mom, _ = level_runs[name]
    nz = mom["levelFluxUp"][0].shape[2] - 1
    assert mom["batches"] == 4 and mom["totalPhotons"] == 8000
    for m in (0, 1):  # S1 and S2
        assert np.array_equal(mom["levelFluxUp"][m][:, :, nz], mom["fluxUp"][m])
        assert np.array_equal(mom["levelFluxDown"][m][:, :, 0], mom["fluxDown"][m])
        assert mom["meanLevelFluxUp"][m][nz] == mom["meanFluxUp"][m]
        assert mom["meanLevelFluxDown"][m][0] == mom["meanFluxDown"][m]
    assert mom["fluxUp"][0].sum() > 0 and mom["fluxDown"][0].sum() > 0
    # something crosses every inner level both ways in a scattering medium
    assert np.all(mom["meanLevelFluxUp"][0][1:nz] > 0) and np.all(mom["meanLevelFluxDown"][0][1:nz] > 0)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,rr,thermal", CASES)
def test_nothing_else_moves(M, level_runs, name, make, rr, thermal):
    """Every moment that exists without level fluxes is what the same walk gives without them."""
    on, _ = level_runs[name]
    off, _ = _moments(M, make(), rr, False, thermal, tuning=dict(layerSkip=0, blockWalk=0))
    assert "levelFluxUp" not in off and set(off) == set(on) - {"levelFluxUp", "levelFluxDown", "meanLevelFluxUp", "meanLevelFluxDown"}
    for k, v in off.items():
        if k in ("totalPhotons", "batches"):
            assert on[k] == v
        else:
            assert np.array_equal(on[k][0], v[0]) and np.array_equal(on[k][1], v[1]), k


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,rr,thermal", [CASES[1], CASES[2]])
def test_the_schedule_does_not_show(M, level_runs, name, make, rr, thermal):
    base = level_runs[name][1]
    for tuning in (dict(blockSize=256), dict(blockSize=512), dict(privateTallies=0, blockSize=256), dict(privateTallies=0, blockSize=512),
                   dict(privateTallies=1, blocksPerCU=1), dict(privateTallies=2, blocksPerCU=3), dict(privateTallies=0, blocksPerCU=2),
                   dict(privateTallies=1, maxBatchesInFlight=1, eventThreshold=4)):
        _, raw = _moments(M, make(), rr, True, thermal, tuning=tuning)
        assert np.array_equal(raw, base), tuning


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _collisions_per_photon(M, case, thermal, n):
    """Counted by the instrumented kernel on the same walk (level fluxes off: the two are refused together)."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, False, False, thermal, dict(layerSkip=0, blockWalk=0))
    integ.enableCounters(True)
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, n)
    c = integ.counters()
    integ.finalize()
    return c["collisions"] / float(n)


@pytest.mark.parametrize("thermal", [False, True])
def test_flux_divergence_is_the_absorption(M, thermal):
    """Per batch and over the whole domain, the net downward flux into layer k is what absorbedProfile(k) records for it (with
    the thermal launch's -1).  Exact per photon history but for the rounding of the weight at a collision: the deposit is
    float(w (1 - omega0)), the weight goes on as float(w omega0), and the two add up to w to within one rounding of a weight
    <= 1, 2^-24.  A photon's error is therefore at most (its collisions) x 2^-24 of its unit weight, the domain-mean flux's at
    most (mean collisions per photon) x 2^-24; the tolerance is ten times that (which also covers the float results: each
    mean is one float of size <= 1, 2^-24 again, six of them in the identity)."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    if thermal:
        case = thermal_case(nz=4)
    else:
        rng = np.random.default_rng(9)
        case = _medium([0.0, 0.1, 0.2], [0.0, 0.1, 0.2], [0.0, 0.04, 0.1, 0.13, 0.2, 0.24], rng.uniform(2.0, 20.0, (2, 2, 5)), 0.8, 0.4)
    n = 20000
    tol = 10.0 * _collisions_per_photon(M, case, thermal, n) * 2.0 ** -24
    dom, integ, photons = _integrator(M, case, False, True, thermal)
    rns = new_RandomNumberSequence(SEED)
    dz = np.diff(np.asarray(case["ze"], np.float64))
    for batch in range(3):
        integ.computeRadiativeTransfer(dom, rns, photons, n)
        r = integ.reportResults()
        lv = integ.reportLevelFluxes()
        assert np.array_equal(lv["levelFluxUp"], r["levelFluxUp"])
        net = lv["meanLevelFluxDown"].astype(np.float64) - lv["meanLevelFluxUp"].astype(np.float64)
        absorbed = r["absorbedProfile"].astype(np.float64) * dz * 1000.0
        worst = np.abs(np.diff(net) - absorbed).max()
        print("flux divergence, %s, batch %d: worst %.3e, tolerance %.3e" % ("thermal" if thermal else "solar", batch, worst, tol))
        assert worst <= tol
        assert np.abs(absorbed).max() > 0.01  # (the identity is not 0 = 0)
    assert integ.badPhotons() == 0
    integ.finalize()


# 5 ---------------------------------------------------------------------------------------------------------------------------
Z_BOUND, Z_FLOOR = 4.5, 1e-6  # tests/test_analytic.py::test_product_beer_lambert: 4.5 standard errors and 1e-6


@pytest.mark.parametrize("mu0", [1.0, 0.4])
def test_beer_lambert_over_a_grey_surface_in_every_column(M, mu0):
    from scipy.special import expn
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    taus, albedo, width = np.array([0.3, 1.2, 2.5]), 0.5, 1.0e4  # columns so wide that none knows of its neighbours
    ze = np.array([0.0, 0.02, 0.09, 0.13, 0.25])
    share = np.array([0.4, 0.1, 0.3, 0.2])                       # of a column's optical depth, bottom up
    ext = taus[:, None, None] * (share / np.diff(ze))[None, None, :]
    case = _medium(width * np.arange(4), [0.0, width], ze, ext, 0.0, albedo, legendre=ISO)
    case.update(mu0=mu0, phi0=0.0)
    dom, integ, photons = _integrator(M, case, True, True)
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 50000, 40)
    st = driver.statistics(driver.unpack_moments(integ.moments(), 3, 1, 4, 0, -1, levelFluxes=True))
    assert integ.badPhotons() == 0
    integ.finalize()
    below = np.concatenate([[0.0], np.cumsum(share)])  # share of the optical depth below level k
    for i, tau in enumerate(taus):
        down = np.exp(-tau * (1.0 - below) / mu0)
        up = albedo * np.exp(-tau / mu0) * 2.0 * expn(3, tau * below)
        for name, theory in (("levelFluxDown", down), ("levelFluxUp", up)):
            got, err = st[name][i, 0, :], st[name + "_StdErr"][i, 0, :]
            print(name, "column", i, "mu0", mu0, "z-scores", np.round((got - theory) / np.maximum(err, 1e-30), 2))
            assert np.all(np.abs(got - theory) < Z_BOUND * err + Z_FLOOR), (name, i, got, theory, err)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def _direct_beam(xe, ze, ext, mu0, phi_deg, per_column):
    """levelFluxDown(x, k) of the direct beam by ray-casting: per_column entry points per column (midpoints), each followed down
    through the periodic grid; exp(-tau) goes to the column in which the ray crosses each level.  The optical depth of a layer's
    stretch is the integral of that layer's extinction over the x interval the ray covers in it, over sin(theta)."""
    nx, nz = len(xe) - 1, len(ze) - 1
    Lx = xe[-1] - xe[0]
    sin_t = np.sqrt(1.0 - mu0 * mu0) * np.cos(np.radians(phi_deg))  # signed x component of the direction (phi = 0 or 180)
    x = np.concatenate([xe[i] + (np.arange(per_column) + 0.5) * (xe[i + 1] - xe[i]) / per_column for i in range(nx)])
    tau = np.zeros_like(x)
    out = np.zeros((nx, nz + 1))

    def tally(k):
        col = np.searchsorted(xe, xe[0] + np.mod(x - xe[0], Lx), side="right") - 1
        np.add.at(out[:, k], np.clip(col, 0, nx - 1), np.exp(-tau))

    tally(nz)
    for k in range(nz - 1, -1, -1):
        cum = np.concatenate([[0.0], np.cumsum(ext[:, k] * np.diff(xe))])  # integral of the layer's extinction from xe[0]

        def integral(p):
            wraps = np.floor((p - xe[0]) / Lx)
            return wraps * cum[-1] + np.interp(p - wraps * Lx, xe, cum)

        x_new = x + (ze[k + 1] - ze[k]) / mu0 * sin_t
        tau = tau + np.abs(integral(x_new) - integral(x)) / abs(sin_t)
        x = x_new
        tally(k)
    return out / per_column


@pytest.mark.parametrize("phi0", [0.0, 180.0])
def test_columns_are_attributed_where_the_beam_crosses(M, phi0):
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    mu0 = 0.5
    xe, ze = 0.02 * np.arange(5), np.array([0.0, 0.03, 0.05, 0.09])  # the beam moves 1.7 cells per cell height: it crosses columns and wraps
    ext = np.array([[4.0, 30.0, 9.0], [25.0, 2.0, 14.0], [8.0, 18.0, 40.0], [35.0, 6.0, 3.0]])
    case = _medium(xe, [0.0, 0.05], ze, ext[:, None, :], 0.0, 0.0, legendre=ISO)
    case.update(mu0=mu0, phi0=phi0)
    dom, integ, photons = _integrator(M, case, True, True)
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 50000, 40)
    st = driver.statistics(driver.unpack_moments(integ.moments(), 4, 1, 3, 0, -1, levelFluxes=True))
    assert integ.badPhotons() == 0
    integ.finalize()
    theory = _direct_beam(xe, ze, ext, mu0, phi0, 4000)
    quadrature = np.abs(theory - _direct_beam(xe, ze, ext, mu0, phi0, 2000))  # the ray-cast's own error, by halving its entry points
    got, err = st["levelFluxDown"][:, 0, :], st["levelFluxDown_StdErr"][:, 0, :]
    print("phi0", phi0, "z-scores\n", np.round((got - theory) / np.maximum(err, 1e-30), 2), "\nquadrature", quadrature.max())
    assert np.all(np.abs(got - theory) < Z_BOUND * err + Z_FLOOR + quadrature), (got, theory, err)
    assert np.ptp(theory[:, 0]) > 20.0 * err[:, 0].max()  # (the columns differ by far more than the noise: a wrong attribution would show)
    assert np.all(st["levelFluxUp"] == 0.0) and np.all(st["meanLevelFluxUp"] == 0.0)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def _raises(integ, rc, text):
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match=text):
        integ._check(rc)


def test_refusals_in_both_orders_of_calls(M):
    """The library's own refusals (called through the C ABI: specifyParameters would refuse most of these before the library sees them)."""
    from mcbrat3d_amd._capi import McbratError, ptr
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = solar_case()
    dom, integ, photons = _integrator(M, case, True, False)
    L, ctx = integ._lib, integ._ctx
    mus, phis = np.array([0.5], np.float32), np.array([0.0], np.float32)
    f0 = C.c_float(0.3)
    inten = lambda n: L.mcbrat_specify_intensity(ctx, n, ptr(mus), ptr(phis), 0, f0, 0, 0, 0, C.c_float(1e30))  # noqa: E731
    xs, ys = np.array([0.0, 0.15]), np.array([0.0, 0.12])
    rpv = np.array([0.1, 0.8, -0.1, 0.5], np.float32)  # rho0, k, Theta, rhoC of the one patch
    brdf = lambda kind: L.mcbrat_set_surface_brdf(ctx, kind, 2, 2, ptr(xs), ptr(ys), 4 if kind else 1, ptr(rpv))  # noqa: E731
    on, off = (lambda: L.mcbrat_specify_level_fluxes(ctx, 1)), (lambda: L.mcbrat_specify_level_fluxes(ctx, 0))
    # intensity directions
    integ._check(inten(1)); _raises(integ, on(), "level fluxes.*intensity directions"); integ._check(inten(0))
    integ._check(on()); _raises(integ, inten(1), "level fluxes.*intensity directions"); integ._check(off())
    # scattering orders
    integ._check(L.mcbrat_specify_scattering_orders(ctx, 3)); _raises(integ, on(), "level fluxes.*scattering orders")
    integ._check(L.mcbrat_specify_scattering_orders(ctx, -1))
    integ._check(on()); _raises(integ, L.mcbrat_specify_scattering_orders(ctx, 3), "level fluxes.*scattering orders"); integ._check(off())
    # a BRDF surface (kind 1: RPV); a Lambertian description (kind 0) is allowed
    integ._check(brdf(1)); _raises(integ, on(), "level fluxes.*BRDF surface"); integ._check(brdf(0))
    integ._check(on()); _raises(integ, brdf(1), "level fluxes.*BRDF surface"); integ._check(brdf(0)); integ._check(off())
    # event counters and photon fates
    integ._check(L.mcbrat_enable_counters(ctx, 1)); _raises(integ, on(), "level fluxes.*event counters / photon fates")
    integ._check(L.mcbrat_enable_counters(ctx, 0))
    integ._check(on()); _raises(integ, L.mcbrat_enable_counters(ctx, 1), "level fluxes.*event counters / photon fates")
    integ.recLevelFluxes = integ._levels_token = True  # (the wrapper's view of what the library now holds)
    with pytest.raises(McbratError, match="level fluxes.*event counters / photon fates"):
        integ.traceFates(dom, new_RandomNumberSequence(SEED), photons, 100)
    integ._check(off())
    integ.finalize()


def test_level_bins_must_fit_the_tally_budget(M):
    """8192 x 8192 columns on 5 levels: 2 x 2^26 x 5 bins of 8 bytes are 5 GiB.  Refused when level fluxes are asked for on such a
    grid, and when such a grid is set with level fluxes on."""
    from mcbrat3d_amd._capi import ptr
    dom, integ, _ = _integrator(M, solar_case(), True, False)
    L, ctx = integ._lib, integ._ctx
    xe, ze = np.arange(8193, dtype=np.float64), np.arange(5, dtype=np.float64)
    integ._check(L.mcbrat_specify_level_fluxes(ctx, 1))
    _raises(integ, L.mcbrat_set_grid(ctx, 8192, 8192, 4, ptr(xe), ptr(xe), ptr(ze)), "level bins.*4 GiB tally budget")
    integ._check(L.mcbrat_specify_level_fluxes(ctx, 0))
    integ._check(L.mcbrat_set_grid(ctx, 8192, 8192, 4, ptr(xe), ptr(xe), ptr(ze)))
    _raises(integ, L.mcbrat_specify_level_fluxes(ctx, 1), "level bins.*4 GiB tally budget")
    integ.finalize()


def test_python_refusals_and_the_copy(M):
    from mcbrat3d_amd._capi import McbratError
    dom, integ, _ = _integrator(M, solar_case(), True, True)
    with pytest.raises(McbratError, match="level fluxes.*intensity directions"):
        integ.specifyParameters(intensityMus=[0.5], intensityPhis=[0.0], computeIntensity=True)
    with pytest.raises(McbratError, match="level fluxes.*scattering orders"):
        integ.specifyParameters(recScatOrd=True, numRecScatOrd=2)
    twin = integ.copy_Integrator()
    assert twin.recLevelFluxes and twin.momentsLength() == integ.momentsLength()
    twin.finalize()
    integ.finalize()


def test_the_plan_with_level_fluxes_and_back(M):
    """Level fluxes run on the face-by-face walk; switching them off restores the plan and the length of the moment array."""
    for make in (lambda: cases.step_cloud(), lambda: cases.landsat_like(n=64, nz=16)):
        case = make()
        dom, integ, photons = _integrator(M, case, True, False)
        integ.prepare(dom, photons)
        before, length = integ.walkMode(), integ.momentsLength()
        assert before["layerSkip"] and (before["blockWalk"] or before["clearAirFlight"])
        integ.specifyParameters(recLevelFluxes=True)
        during = integ.walkMode()
        assert not during["layerSkip"] and not during["clearAirFlight"] and not during["blockWalk"] and not during["widePlan"]
        ncol = dom.numX * dom.numY
        assert integ.momentsLength() == length + 2 * (dom.numZ + 1) * (1 + ncol)
        integ.specifyParameters(recLevelFluxes=False)
        assert integ.walkMode() == before and integ.momentsLength() == length
        integ.finalize()


def test_asynchronous_mode_gives_the_same_moments(M):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    raw = {}
    for mode in (False, True):
        dom, integ, photons = _integrator(M, solar_case(), False, True)
        integ.setAsync(mode)
        integ.resetMoments()
        rns = new_RandomNumberSequence(SEED)
        for batches in (2, 1, 3):
            integ.computeRadiativeTransfer(dom, rns, photons, 2000, batches)
        integ.synchronize()
        raw[mode] = integ.moments().copy()
        integ.finalize()
    assert raw[True][1] == 6 and np.array_equal(raw[True], raw[False])
