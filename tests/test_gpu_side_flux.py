"""The flux through the vertical faces of every cell (recSideFluxes) on the GPU.

What holds the tally:

4. every older part of the moments and of the last-batch results is bit for bit what it is without the setting, on the same walk
   with level fluxes on; the schedule does not show; asynchronous mode gives the same moments;
5. closed forms pin units and signs: a vacuum and a grey absorber under an oblique sun, an overhead sun;
6. photon by photon, bit for bit: black media, every float against the ray-cast helper of tests/side_cases.py (held on the CPU by
   tests/test_side_flux_host.py) pushed through the written-out epilogue;
7. the cell balance: per batch and per cell, what enters through the six faces minus what leaves is what the cell absorbed;
8. the refusals, the tally budget, the plan and the copy.

No photon is dropped in any of these runs (asserted per run, and by tests/conftest.py when an integrator is finalised)."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC
from tests import side_cases as SC

pytestmark = pytest.mark.gpu

SEED = 20251019
CALLS = SC.CALLS
Z_BOUND = 4.5
OLD = ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "fluxUp", "fluxDown", "fluxAbsorbed", "absorbedProfile", "absorbedVolume",
       "meanLevelFluxUp", "meanLevelFluxDown", "levelFluxUp", "levelFluxDown")
OLD_REPORT = ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "fluxUp", "fluxDown", "fluxAbsorbed", "absorbedProfile", "volumeAbsorption",
              "meanLevelFluxUp", "meanLevelFluxDown", "levelFluxUp", "levelFluxDown")


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integrator(M, case, source, rr=True, table=LC.TABLE, side=True, tuning=None, levels=True):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    surface = cases.product_surface(case)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=rr, LW_flag=-1.0, recLevelFluxes=levels,
                            recSideFluxes=side, **({"surfaceBDRF": surface} if surface is not None else {}))
    integ.setTuning(**(tuning or {}))
    return dom, integ, M.new_PhotonStream(numberOfPhotons=10 ** 12, **source)


def _tuning(priv, block):
    """The tuning that gives the kernels of template argument PRIV = priv: 0 global atomics and the flat form of the walk; 2 the
    library's plan (mcbrat_set_tuning: privateTallies = 1), which on these small domains keeps tallies and grid in LDS -- the
    nested form.  (privateTallies = 2 is private tallies WITHOUT the grid in LDS, which under level fluxes gives way to PRIV 0.)"""
    return dict(privateTallies=1 if priv == 2 else 0, blockSize=block, eventThreshold=16)


def _assert_form(integ, tuning):
    """Where the tuning names the form of the walk (privateTallies 0 or 1 with a block size), the plan is that form."""
    if tuning and tuning.get("privateTallies") in (0, 1) and "blockSize" in tuning and "blocksPerCU" not in tuning:
        assert integ.walkMode()["privateTallies"] == bool(tuning["privateTallies"]), tuning


def _trace(M, case, source, rr=True, tuning=None, side=True, calls=CALLS, table=LC.TABLE, asynchronous=False):
    """-> dict(reports: reportResults() after each call, raw: the moment array, mom: it unpacked, stats, len, dims)."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, source, rr, table, side, tuning)
    integ.prepare(dom, photons)  # (the plan is that of the loaded domain)
    walk = integ.walkMode()
    assert not walk["layerSkip"] and not walk["blockWalk"] and not walk["clearAirFlight"] and not walk["widePlan"]
    _assert_form(integ, tuning)
    if asynchronous:
        integ.setAsync(True)
    integ.resetMoments()
    rns = new_RandomNumberSequence(SEED)
    reports = []
    for ppb, nb in calls:
        assert integ.computeRadiativeTransfer(dom, rns, photons, ppb, nb) == ppb * nb
        if not asynchronous:
            reports.append(integ.reportResults())
    integ.synchronize()
    raw = integ.moments().copy()
    assert integ.badPhotons() == 0 and raw.size == 8 + 2 * integ.momentsLength()
    mom = driver.unpack_moments(raw, dom.numX, dom.numY, dom.numZ, 0, -1, levelFluxes=True, sideFluxes=side)
    out = dict(reports=reports, raw=raw, len=integ.momentsLength(), dims=(dom.numX, dom.numY, dom.numZ), mom=mom,
               stats=driver.statistics(mom))
    integ.finalize()
    return out


# 4 ---------------------------------------------------------------------------------------------------------------------------
SOLAR = [n for n, v in LC.EXACT.items() if v[1] is not None]
SOURCES = {"RandomAzimuth": dict(solarMu=0.6), "Flux": dict(), "Spotlight": dict(solarMu=0.6, solarAzimuth=30.0, solarX=0.3, solarY=0.7)}
MOVES = [(name, None) for name in SOLAR] + [("irregular, oblique, flat walk", kind) for kind in SOURCES]


def _exact_case(name, kind=None):
    grid, mu0, phi0, priv, block, rr = LC.EXACT[name]
    source = dict(solarMu=mu0, solarAzimuth=phi0) if kind is None else SOURCES[kind]
    return LC.medium(grid), source, rr, _tuning(priv, block)


def _assert_old_parts_equal(on, off):
    nx, ny, nz = on["dims"]
    assert on["len"] == off["len"] + 4 * nz * (1 + nx * ny)
    old = off["len"]
    # the moment array: header, then both sums of every older part at its old offset
    assert np.array_equal(on["raw"][:8], off["raw"][:8])
    assert np.array_equal(on["raw"][8:8 + old], off["raw"][8:8 + old])
    assert np.array_equal(on["raw"][8 + on["len"]:8 + on["len"] + old], off["raw"][8 + old:8 + 2 * old])
    for k in OLD:
        for m in (0, 1):
            assert np.array_equal(np.asarray(on["mom"][k][m]), np.asarray(off["mom"][k][m])), k


@pytest.mark.parametrize("name,kind", MOVES, ids=[n if k is None else k for n, k in MOVES])
def test_nothing_else_moves(M, name, kind):
    """With the setting and without it, on the same walk with level fluxes on, batches of 8000, 8000 and 4000: the header, both
    sums of every older part of the moment array and every older last-batch result have the same bits."""
    case, source, rr, tuning = _exact_case(name, kind)
    on, off = _trace(M, case, source, rr, tuning, True), _trace(M, case, source, rr, tuning, False)
    nx, ny, nz = on["dims"]
    _assert_old_parts_equal(on, off)
    for a, b in zip(on["reports"], off["reports"]):
        for k in OLD_REPORT:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        for n_, m_ in zip(SC.NAMES, SC.MEANS):
            assert a[n_].shape == (nx, ny, nz) and a[m_].shape == (nz,) and n_ not in b
    # something crosses the sides in a scattering medium, both ways on both axes (the Spotlight's one column included)
    assert all(np.asarray(on["stats"][m_]).min() > 0 for m_ in SC.MEANS)


SCHEDULES = (dict(blockSize=256), dict(blockSize=512), dict(privateTallies=0, blockSize=256), dict(privateTallies=0, blockSize=512),
             dict(privateTallies=1, blocksPerCU=1), dict(privateTallies=2, blocksPerCU=3), dict(privateTallies=0, blocksPerCU=2),
             dict(privateTallies=1, maxBatchesInFlight=1, eventThreshold=4))


def test_the_schedule_does_not_show(M):
    """The tuning list of tests/test_gpu_level_flux.py::test_the_schedule_does_not_show: identical raw moment arrays."""
    case, source = LC.medium("irregular"), dict(solarMu=0.5, solarAzimuth=30.0)
    calls = ((2000, 4),)
    base = _trace(M, case, source, False, dict(eventThreshold=16), calls=calls)["raw"]
    for tuning in SCHEDULES:
        raw = _trace(M, case, source, False, {"eventThreshold": 16, **tuning}, calls=calls)["raw"]
        assert np.array_equal(raw, base), tuning


def test_asynchronous_mode_gives_the_same_moments(M):
    case, source = LC.medium("irregular z"), dict(solarMu=0.6, solarAzimuth=210.0)
    calls = ((2000, 2), (2000, 1), (2000, 3))
    raw = {mode: _trace(M, case, source, False, dict(eventThreshold=16), calls=calls, asynchronous=mode)["raw"] for mode in (False, True)}
    assert raw[True][1] == 6 and np.array_equal(raw[True], raw[False])


# 5 ---------------------------------------------------------------------------------------------------------------------------
WALKS = {"flat walk": _tuning(0, 256), "nested walk": _tuning(2, 512)}
FORTY = ((5000, 40),)  # 2 x 10^5 photons in 40 batches


def _assert_closed_form(res, want, label):
    """want: name -> [nz] expectation or None (exactly zero in every bin and mean, both moment sums)."""
    st, mom = res["stats"], res["mom"]
    for name, mean in zip(SC.NAMES, SC.MEANS):
        if want[name] is None:
            for key in (name, mean):
                assert not np.any(mom[key][0]) and not np.any(mom[key][1]), (label, key)
            continue
        got, err = np.asarray(st[mean], np.float64), np.asarray(st[mean + "_StdErr"], np.float64)
        z = (got - want[name]) / np.where(err > 0, err, 1.0)
        print("%s: %s %s +- %s, closed form %s, z %s" % (label, mean, got, err, want[name], z))
        assert np.all(np.abs(got - want[name]) <= Z_BOUND * err + 1e-5), (label, mean)


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("phi0", [30.0, 210.0])
@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_vacuum_under_an_oblique_sun(M, grid, phi0, walk):
    """mu0 = 0.5: the layer means of XPlus - XMinus and of YPlus - YMinus are tan(theta0) cos(phi0) and tan(theta0) sin(phi0) in
    every layer; nothing travels against the beam, so at phi0 = 30 XMinus and YMinus are exactly 0, and at 210 the roles swap."""
    res = _trace(M, SC.medium_on(grid, 0.0), dict(solarMu=0.5, solarAzimuth=phi0), tuning=WALKS[walk], calls=FORTY, table=2001)
    fx, fy = SC.horizontal(0.5, phi0)
    nz = res["dims"][2]
    want = dict(sideFluxXPlus=np.full(nz, fx) if fx > 0 else None, sideFluxXMinus=np.full(nz, -fx) if fx < 0 else None,
                sideFluxYPlus=np.full(nz, fy) if fy > 0 else None, sideFluxYMinus=np.full(nz, -fy) if fy < 0 else None)
    _assert_closed_form(res, want, "vacuum, %s, phi0 %g, %s" % (grid, phi0, walk))


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_grey_absorber_under_an_oblique_sun(M, grid, walk):
    """omega0 = 0, sigma = 10 / km, mu0 = 0.5, phi0 = 30: only the direct beam travels, and the layer mean of the flux through a
    vertical face is tan(theta0) cos(phi0) mu0 / (sigma dz_k) (exp(-tau_top / mu0) - exp(-tau_bot / mu0)), the beam averaged over
    the layer's depth."""
    sigma = 10.0
    case = SC.medium_on(grid, sigma)
    res = _trace(M, case, dict(solarMu=0.5, solarAzimuth=30.0), tuning=WALKS[walk], calls=FORTY, table=2001)
    fx, fy = SC.horizontal(0.5, 30.0)
    prof = SC.absorber_profile(case["ze"], sigma, 0.5)
    want = dict(sideFluxXPlus=fx * prof, sideFluxXMinus=None, sideFluxYPlus=fy * prof, sideFluxYMinus=None)
    _assert_closed_form(res, want, "grey absorber, %s, %s" % (grid, walk))


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_overhead_sun_in_a_vacuum_crosses_no_side(M, grid, walk):
    res = _trace(M, SC.medium_on(grid, 0.0), dict(solarMu=1.0, solarAzimuth=0.0), tuning=WALKS[walk], table=2001)
    _assert_closed_form(res, dict.fromkeys(SC.NAMES), "overhead sun, %s, %s" % (grid, walk))
    assert np.all(np.asarray(res["stats"]["levelFluxDown"]) > 0)
    for rep in res["reports"]:
        assert all(not np.any(rep[k]) for k in SC.NAMES + SC.MEANS)


# 6 ---------------------------------------------------------------------------------------------------------------------------
BITS = [(grid, ext, mu0, phi0, priv, block) for grid, ext, mu0, phi0 in SC.RAY_CASES for priv in (0, 2) for block in (256, 512)]


@pytest.mark.parametrize("grid,ext,mu0,phi0,priv,block", BITS)
def test_photon_by_photon_bit_for_bit(M, grid, ext, mu0, phi0, priv, block):
    """Black media (omega0 = 0, albedo 0): every weight is exactly 1 and every raw bin a multiple of 2^32.  Every maximal run of
    photon ids the ray-cast helper leaves unflagged, in calls of at most 128 ids: every float of the four arrays and the four
    means EQUALS the helper's integer counts pushed through the written-out epilogue (side_cases.side_values).  No tolerance."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    rc = SC.ray_cast(grid, ext, mu0, phi0)
    calls = SC.split_runs(LC.clean_runs(rc["flagged"]))
    case = SC.medium_on(grid, ext)
    g = EM.Grid(case["xe"], case["ye"], case["ze"])
    dom, integ, photons = _integrator(M, case, dict(solarMu=mu0, solarAzimuth=phi0), table=2001,
                                      tuning=_tuning(priv, block))
    integ.prepare(dom, photons)
    walk = integ.walkMode()
    assert walk["privateTallies"] == (priv == 2)  # (the form of the walk asked for)
    assert not walk["layerSkip"] and not walk["blockWalk"] and not walk["clearAirFlight"]
    failures, crossings = [], 0
    for first, count in calls:
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(LC.SEED, first), photons, count) == count
        means, bins = SC.report_arrays(integ.reportSideFluxes(), g)
        raw = SC.raw_bins(rc, first, count)
        wmeans, wbins = SC.side_values(g, raw, count)
        crossings += int(raw.sum() >> 32)
        if not (np.array_equal(bins, wbins) and np.array_equal(means, wmeans)):
            bad = np.flatnonzero(bins != wbins)
            failures.append((first, count, bad[:6].tolist(), bins[bad[:6]].tolist(), wbins[bad[:6]].tolist()))
    bad = integ.badPhotons()
    integ.finalize()
    print("bit for bit: %s, ext %g, sun (%g, %g), PRIV %d, BLOCK %d: flagged %.4f of %d ids, %d calls, %d crossings, calls that differ %d"
          % (grid, ext, mu0, phi0, priv, block, rc["flagged"].mean(), rc["flagged"].size, len(calls), crossings, len(failures)))
    assert not failures, (len(failures), failures[:3])
    assert bad == 0 and crossings > 0


# 7 ---------------------------------------------------------------------------------------------------------------------------
def _events_per_batch(M, case, source, n):
    """Crossings plus collisions of a batch of n photons, counted by the instrumented kernel on the same walk (level and side
    fluxes off: they are refused together with the counters)."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, source, False, 9001, False, dict(layerSkip=0, blockWalk=0, eventThreshold=16), levels=False)
    integ.enableCounters(True)
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, n)
    c = integ.counters()
    integ.finalize()
    return float(c["crossings"] + c["collisions"])


@pytest.mark.parametrize("walk", list(WALKS))
def test_the_cell_balance(M, walk):
    """Per batch and per cell, in photon weights (each reported float multiplied back by its normaliser): the downward net through
    the cell's top face, minus that through its bottom face, plus the inward net through its four sides, equals
    absorbedVolume nppc dz 1000.  Exact per photon history -- every step of the walk leaves one cell for its neighbour through
    one face, and the deposit of that step is booked at that face, in the patch both cells share -- but for three roundings.  The
    tolerance is derived from them, not measured:

    * the weight at a collision: the deposit is float(w (1 - omega0)), the weight goes on as float(w omega0), and the two add up to
      w within one rounding of a weight <= 1, 2^-24 of w.  The weights that collided in a cell sum to A_cell / (1 - omega0), A_cell
      the absorbed weight: 2^-24 A_cell / (1 - omega0);
    * one float rounding, 2^-24 relative, of each of the thirteen floats in the identity (four level fluxes, eight side fluxes, the
      absorption): 2^-24 times the sum of their magnitudes in photon weights (the level floats are a conversion and a division,
      two roundings: the second is left to the factor below);
    * half a fixed-point unit, 2^-33, per deposit: bounded by the batch's crossings plus collisions, counted by the instrumented
      kernel on the same walk.

    At most a factor 10 over that sum is allowed, as tests/test_gpu_level_flux.py::test_flux_divergence_is_the_absorption allows.
    Roulette off; 3 x 2 x 5 irregular cells, omega0 = 0.8, albedo 0.4, mu0 = 0.6, phi0 = 30; three batches of 20 000."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from tests.test_gpu_level_flux import _medium
    rng = np.random.default_rng(9)
    omega = 0.8
    case = _medium([0.0, 0.05, 0.12, 0.15], [0.0, 0.08, 0.12], [0.0, 0.04, 0.1, 0.13, 0.2, 0.24], rng.uniform(2.0, 20.0, (3, 2, 5)), omega, 0.4)
    source = dict(solarMu=0.6, solarAzimuth=30.0)
    n = 20000
    events = _events_per_batch(M, case, source, n)
    dom, integ, photons = _integrator(M, case, source, False, 9001, True, WALKS[walk])
    integ.prepare(dom, photons)
    _assert_form(integ, WALKS[walk])
    g = EM.Grid(case["xe"], case["ye"], case["ze"])
    nx, ny, nz = g.nx, g.ny, g.nz
    nppc = g.photons_per_column(n).astype(np.float64).reshape(ny, nx).T[:, :, None]  # [ix, iy, 1]
    dx, dy, dz = np.diff(g.xe)[:, None, None], np.diff(g.ye)[None, :, None], g.dz[None, None, :]
    rns = new_RandomNumberSequence(SEED)
    for batch in range(3):
        assert integ.computeRadiativeTransfer(dom, rns, photons, n) == n
        r = integ.reportResults()
        f64 = lambda k: np.asarray(r[k], np.float64)  # noqa: E731
        down, up = f64("levelFluxDown") * nppc, f64("levelFluxUp") * nppc          # [ix, iy, level]
        xp, xm = f64("sideFluxXPlus") * nppc * dz / dx, f64("sideFluxXMinus") * nppc * dz / dx
        yp, ym = f64("sideFluxYPlus") * nppc * dz / dy, f64("sideFluxYMinus") * nppc * dz / dy
        absorbed = f64("volumeAbsorption") * nppc * dz * 1000.0
        top = down[:, :, 1:] - up[:, :, 1:]
        bottom = down[:, :, :-1] - up[:, :, :-1]
        # the low-x face of cell ix is the bin of cell ix - 1 (the periodic image for ix = 0): inward is plus there, minus at the high face
        sides = (np.roll(xp - xm, 1, axis=0) - (xp - xm)) + (np.roll(yp - ym, 1, axis=1) - (yp - ym))
        magnitudes = down[:, :, 1:] + up[:, :, 1:] + down[:, :, :-1] + up[:, :, :-1] + np.roll(xp + xm, 1, axis=0) + xp + xm + \
            np.roll(yp + ym, 1, axis=1) + yp + ym + absorbed
        tol = 10.0 * (2.0 ** -24 * absorbed / (1.0 - omega) + 2.0 ** -24 * magnitudes + 2.0 ** -33 * events)
        residual = np.abs(top - bottom + sides - absorbed)
        worst = np.unravel_index(np.argmax(residual / tol), residual.shape)
        print("cell balance, %s, batch %d: worst residual %.3e photon weights in cell %s against the tolerance %.3e (absorbed %.1f, through "
              "the top %.1f, through the sides %.1f)" % (walk, batch, residual[worst], worst, tol[worst], absorbed[worst], top[worst], sides[worst]))
        assert np.all(residual <= tol), (walk, batch, worst, residual[worst], tol[worst])
        # the identity is not 0 = 0
        through_top = down[:, :, 1:]
        assert (np.abs(sides) > 0.01 * through_top).mean() > 0.5 and (absorbed > 0.01 * through_top).mean() > 0.5
    assert integ.badPhotons() == 0
    integ.finalize()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def _raises(integ, rc, text):
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match=text):
        integ._check(rc)


def test_refusals_through_the_c_abi(M):
    from mcbrat3d_amd._capi import ptr
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = SC.medium_on("33 x 1 x 2", 0.0)
    dom, integ, photons = _integrator(M, case, dict(solarMu=0.5, solarAzimuth=0.0), side=False, levels=False)
    integ.prepare(dom, photons)
    L, ctx = integ._lib, integ._ctx
    side, levels, direct, act = (lambda on: L.mcbrat_specify_side_fluxes(ctx, on)), (lambda on: L.mcbrat_specify_level_fluxes(ctx, on)), \
        (lambda on: L.mcbrat_specify_direct_level_fluxes(ctx, on)), (lambda on: L.mcbrat_specify_actinic_flux(ctx, on))
    length, walk = integ.momentsLength(), integ.walkMode()
    lvl, sd = 2 * 3 * (1 + 33), 4 * 2 * (1 + 33)
    _raises(integ, L.mcbrat_report_side_fluxes(ctx, None, None), "side-flux information not available")
    # without level fluxes
    _raises(integ, side(1), "side fluxes.*need level fluxes")
    assert integ.momentsLength() == length and integ.walkMode() == walk
    integ._check(levels(1)); integ._check(side(1))
    assert integ.momentsLength() == length + lvl + sd
    _raises(integ, L.mcbrat_report_side_fluxes(ctx, None, None), "no batch has been traced yet")
    # the setting first: level fluxes cannot be switched off under it, and what it cannot be combined with is refused
    _raises(integ, levels(0), "side fluxes.*need level fluxes")
    _raises(integ, direct(1), "side fluxes.*direct level fluxes")
    _raises(integ, act(1), "side fluxes.*actinic flux")
    mus, phis = np.array([0.5], np.float32), np.array([0.0], np.float32)
    inten = lambda n: L.mcbrat_specify_intensity(ctx, n, ptr(mus), ptr(phis), 0, C.c_float(0.3), 0, 0, 0, C.c_float(1e30))  # noqa: E731
    xs, ys = np.array([0.0, 1.03125]), np.array([0.0, 0.5])
    rpv = np.array([0.1, 0.8, -0.1, 0.5], np.float32)
    _raises(integ, inten(1), "level fluxes.*intensity directions")
    _raises(integ, L.mcbrat_specify_scattering_orders(ctx, 3), "level fluxes.*scattering orders")
    _raises(integ, L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(ys), 4, ptr(rpv)), "level fluxes.*BRDF surface")
    _raises(integ, L.mcbrat_enable_counters(ctx, 1), "level fluxes.*event counters / photon fates")
    with pytest.raises(M.McbratError, match="level fluxes.*event counters / photon fates"):
        integ.traceFates(dom, new_RandomNumberSequence(SEED), photons, 100)
    assert integ.momentsLength() == length + lvl + sd
    # the other order of calls
    integ._check(side(0)); integ._check(direct(1))
    assert integ.momentsLength() == length + 2 * lvl
    _raises(integ, side(1), "side fluxes.*direct level fluxes")
    integ._check(direct(0)); integ._check(act(1))
    _raises(integ, side(1), "side fluxes.*actinic flux")
    assert integ.momentsLength() == length + lvl + 2 * (1 + 33)
    integ._check(act(0)); integ._check(levels(0))
    assert integ.momentsLength() == length and integ.walkMode() == walk
    for on, off, text in ((lambda: inten(1), lambda: inten(0), "intensity directions"),
                          (lambda: L.mcbrat_specify_scattering_orders(ctx, 3), lambda: L.mcbrat_specify_scattering_orders(ctx, -1), "scattering orders"),
                          (lambda: L.mcbrat_enable_counters(ctx, 1), lambda: L.mcbrat_enable_counters(ctx, 0), "event counters"),
                          (lambda: L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(ys), 4, ptr(rpv)),
                           lambda: L.mcbrat_set_surface_brdf(ctx, 1, 0, 0, None, None, 0, None), "BRDF surface")):
        integ._check(on())
        _raises(integ, levels(1), "level fluxes.*" + text)  # (and without level fluxes no side fluxes)
        _raises(integ, side(1), "side fluxes.*need level fluxes")
        integ._check(off())
    assert integ.momentsLength() == length and integ.walkMode() == walk
    # and after all that it traces
    integ._check(levels(1)); integ._check(side(1))
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000) == 1000
    mean = np.zeros(4 * 2, np.float32)
    integ._check(L.mcbrat_report_side_fluxes(ctx, ptr(mean), None))
    assert np.abs(mean[:2] - np.sqrt(3.0)).max() < 0.2 and not np.any(mean[2:])  # (phi0 = 0: all of it through the x faces, towards +x)
    integ.finalize()


def test_a_thermal_stream_is_refused_when_it_is_traced(M):
    from mcbrat3d_amd._capi import McbratError
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = cases.homog_lw(n=3)
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=2001, LW_flag=1.0, recLevelFluxes=True, recSideFluxes=True)
    w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
    M.emission_weighting(dom, w, case["sfc_temp"])
    photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    with pytest.raises(McbratError, match="side fluxes.*thermal source"):
        integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000)
    integ.specifyParameters(recSideFluxes=False)  # without the setting the stream runs, level fluxes on
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000) == 1000
    integ.finalize()


def test_the_bins_must_fit_the_tally_budget(M):
    """8192 x 8192 columns, 2 layers: the two level parts are 2 x 2^26 x 3 bins of 8 bytes, 3 GiB, and fit the 4 GiB budget; the
    four side parts are 4 x 2^26 x 2 bins, 4 GiB more, and the two together do not."""
    from mcbrat3d_amd._capi import ptr
    dom, integ, _ = _integrator(M, SC.medium_on("1 x 1 x 1", 0.0), dict(solarMu=0.5, solarAzimuth=0.0))
    L, ctx = integ._lib, integ._ctx
    xe, ze = np.arange(8193, dtype=np.float64), np.arange(3, dtype=np.float64)
    length = integ.momentsLength()
    _raises(integ, L.mcbrat_set_grid(ctx, 8192, 8192, 2, ptr(xe), ptr(xe), ptr(ze)), "side fluxes.*4 GiB tally budget")
    assert integ.momentsLength() == length
    integ._check(L.mcbrat_specify_side_fluxes(ctx, 0))
    integ._check(L.mcbrat_set_grid(ctx, 8192, 8192, 2, ptr(xe), ptr(xe), ptr(ze)))  # level fluxes alone fit
    _raises(integ, L.mcbrat_specify_side_fluxes(ctx, 1), "side fluxes.*4 GiB tally budget")
    integ.finalize()


def test_python_refusals_leave_the_integrator_as_it_was_and_the_copy_carries_the_setting(M):
    from mcbrat3d_amd._capi import McbratError
    dom, integ, photons = _integrator(M, SC.medium_on("1 x 1 x 1", 0.0), dict(solarMu=0.5, solarAzimuth=0.0), side=False, levels=False)
    length = integ.momentsLength()
    with pytest.raises(McbratError, match="side fluxes.*need level fluxes"):
        integ.specifyParameters(recSideFluxes=True, useRussianRoulette=False)
    assert not integ.recSideFluxes and integ.useRussianRoulette and integ.momentsLength() == length
    integ.specifyParameters(recLevelFluxes=True, recSideFluxes=True)
    assert integ.momentsLength() == length + 2 * 2 * 2 + 4 * 2
    with pytest.raises(McbratError, match="side fluxes.*need level fluxes"):
        integ.specifyParameters(recLevelFluxes=False)
    with pytest.raises(McbratError, match="side fluxes.*direct level fluxes"):
        integ.specifyParameters(recDirectLevelFluxes=True)
    with pytest.raises(McbratError, match="side fluxes.*actinic flux"):
        integ.specifyParameters(recActinicFlux=True)
    with pytest.raises(McbratError, match="level fluxes.*scattering orders"):
        integ.specifyParameters(recScatOrd=True, numRecScatOrd=2, useRussianRoulette=False)
    with pytest.raises(McbratError, match="level fluxes.*intensity directions"):
        integ.specifyParameters(intensityMus=[0.5], intensityPhis=[0.0], computeIntensity=True)
    assert integ.recSideFluxes and integ.recLevelFluxes and not integ.recDirectLevelFluxes and not integ.recActinicFlux
    assert integ.numRecScatOrd < 0 and integ.useRussianRoulette and integ.momentsLength() == length + 2 * 2 * 2 + 4 * 2
    twin = integ.copy_Integrator()
    assert twin.recSideFluxes and twin.recLevelFluxes and twin.momentsLength() == integ.momentsLength()
    twin.finalize()
    # from the side tally to the direct tally or the actinic flux in one call, and back
    integ.specifyParameters(recSideFluxes=False, recDirectLevelFluxes=True)
    integ.specifyParameters(recSideFluxes=True, recDirectLevelFluxes=False)
    integ.specifyParameters(recSideFluxes=False, recActinicFlux=True)
    integ.specifyParameters(recSideFluxes=True, recActinicFlux=False)
    integ.specifyParameters(recLevelFluxes=False, recSideFluxes=False)
    assert integ.momentsLength() == length
    # SpectralRun refuses it before any integrator is made
    from mcbrat3d_amd import broadband
    with pytest.raises(McbratError, match="side fluxes.*spectrally integrated"):
        broadband.SpectralRun(M, [dom], recSideFluxes=True)
    integ.finalize()


def test_the_plan_with_side_fluxes_and_back(M):
    """Side fluxes run on the face-by-face walk of level fluxes; switching both off restores the plan and the moment array."""
    for make in (lambda: cases.step_cloud(), lambda: cases.landsat_like(n=64, nz=16)):
        case = make()
        dom, integ, photons = _integrator(M, case, dict(solarMu=0.6, solarAzimuth=30.0), table=9001, side=False, levels=False)
        integ.prepare(dom, photons)
        before, length = integ.walkMode(), integ.momentsLength()
        assert before["layerSkip"] and (before["blockWalk"] or before["clearAirFlight"])
        integ.specifyParameters(recLevelFluxes=True)
        levels_walk = integ.walkMode()
        integ.specifyParameters(recSideFluxes=True)
        during = integ.walkMode()
        assert during == levels_walk  # (the side bins are no part of the LDS slab: the plan of level fluxes alone)
        assert not during["layerSkip"] and not during["clearAirFlight"] and not during["blockWalk"] and not during["widePlan"]
        ncol = dom.numX * dom.numY
        assert integ.momentsLength() == length + 2 * (dom.numZ + 1) * (1 + ncol) + 4 * dom.numZ * (1 + ncol)
        integ.specifyParameters(recLevelFluxes=False, recSideFluxes=False)
        assert integ.walkMode() == before and integ.momentsLength() == length
        integ.finalize()
