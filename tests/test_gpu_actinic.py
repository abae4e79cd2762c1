"""The actinic flux of every cell by track length (recActinicFlux) on the GPU.

What holds the tally:

1. every older part of the moments and of the last-batch results is bit for bit what it is without the setting, with level
   fluxes on and off, however the batches are split;
2. a vacuum under an overhead sun: actinicFlux = fluxDown in every cell of a column (1e-5 relative);
3. a vacuum under an oblique sun: every layer mean is 1 / mu0; 2 / mu0 over a white surface, 2 under isotropic incidence;
4. track length against collisions: absorbedVolume = sigma_abs actinicFlux / 1000 in every absorbing cell, at statistics;
5. where nothing absorbs: 4 pi J of the integral-equation solver for a two-layer slab;
6. the epilogue bit for bit against the expressions written out in tests/actinic_cases.py, from bins known by construction;
7. the refusals, through the C ABI in both orders of calls, and through Python;
8. no photon is dropped in any of these runs (asserted per run, and by tests/conftest.py when an integrator is finalised)."""
import ctypes as C

import numpy as np
import pytest

from tests import actinic_cases as AC
from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC

pytestmark = pytest.mark.gpu

SEED = 20251018
CALLS = AC.CALLS
Z_BOUND = 4.5
OLD = ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "fluxUp", "fluxDown", "fluxAbsorbed", "absorbedProfile", "absorbedVolume")
LEVEL = ("meanLevelFluxUp", "meanLevelFluxDown", "levelFluxUp", "levelFluxDown")
OLD_REPORT = ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "fluxUp", "fluxDown", "fluxAbsorbed", "absorbedProfile", "volumeAbsorption")


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integrator(M, case, source, rr=True, table=LC.TABLE, actinic=True, levels=False, tuning=None):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    surface = cases.product_surface(case)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=rr, LW_flag=-1.0, recLevelFluxes=levels,
                            recActinicFlux=actinic, **({"surfaceBDRF": surface} if surface is not None else {}))
    # the same face-by-face walk with and without the setting: no layer skipping, no block walk
    integ.setTuning(layerSkip=0, blockWalk=0, **(tuning or {}))
    return dom, integ, M.new_PhotonStream(numberOfPhotons=10 ** 12, **source)


def _trace(M, case, source, rr=True, tuning=None, actinic=True, levels=False, calls=CALLS, table=LC.TABLE):
    """-> dict(reports: reportResults() after each call, raw: the moment array, mom: it unpacked, stats, len, dims)."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, source, rr, table, actinic, levels, tuning)
    walk = integ.walkMode()
    assert not walk["layerSkip"] and not walk["blockWalk"] and not walk["clearAirFlight"]
    if actinic:
        assert not walk["widePlan"]
    integ.resetMoments()
    rns = new_RandomNumberSequence(SEED)
    reports = []
    for ppb, nb in calls:
        assert integ.computeRadiativeTransfer(dom, rns, photons, ppb, nb) == ppb * nb
        reports.append(integ.reportResults())
    raw = integ.moments().copy()
    assert integ.badPhotons() == 0 and raw.size == 8 + 2 * integ.momentsLength()
    mom = driver.unpack_moments(raw, dom.numX, dom.numY, dom.numZ, 0, -1, levelFluxes=levels, actinicFlux=actinic)
    out = dict(reports=reports, raw=raw, len=integ.momentsLength(), dims=(dom.numX, dom.numY, dom.numZ), mom=mom,
               stats=driver.statistics(mom))
    integ.finalize()
    return out


def _exact_case(name):
    grid, mu0, phi0, priv, block, rr = LC.EXACT[name]
    return LC.medium(grid), dict(solarMu=mu0, solarAzimuth=phi0), rr, dict(privateTallies=priv, blockSize=block, eventThreshold=16)


_cache = {}


def run_exact(M, name, actinic, levels, calls=CALLS):
    key = (name, actinic, levels, calls)
    if key not in _cache:
        case, source, rr, tuning = _exact_case(name)
        _cache[key] = _trace(M, case, source, rr, tuning, actinic, levels, calls)
    return _cache[key]


SOLAR = [n for n, v in LC.EXACT.items() if v[1] is not None]


# 1 ---------------------------------------------------------------------------------------------------------------------------
WHOLE = ((20000, 1),)  # the same photons in one batch


@pytest.mark.parametrize("calls", [CALLS, WHOLE], ids=["8000 + 8000 + 4000", "20000"])
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("name", SOLAR)
def test_nothing_else_moves(M, name, levels, calls):
    """With the setting and without it, on the same face-by-face walk: the header, both sums of every older part of the moment
    array and every older last-batch result have the same bits -- with level fluxes on and off, and however the photons are
    split into batches (the tallies are integers: whichever kernel and plan traced them, the bins are the same)."""
    on, off = run_exact(M, name, True, levels, calls), run_exact(M, name, False, levels, calls)
    nx, ny, nz = on["dims"]
    assert on["len"] == off["len"] + nz * (1 + nx * ny)
    old = off["len"]
    # the moment array: header, then both sums of every older part at its old offset
    assert np.array_equal(on["raw"][:8], off["raw"][:8])
    assert np.array_equal(on["raw"][8:8 + old], off["raw"][8:8 + old])
    assert np.array_equal(on["raw"][8 + on["len"]:8 + on["len"] + old], off["raw"][8 + old:8 + 2 * old])
    for k in OLD + (LEVEL if levels else ()):
        for m in (0, 1):
            assert np.array_equal(np.asarray(on["mom"][k][m]), np.asarray(off["mom"][k][m])), k
    # the last-batch results after every call
    for a, b in zip(on["reports"], off["reports"]):
        for k in OLD_REPORT + (LEVEL if levels else ()):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert a["actinicFlux"].shape == (nx, ny, nz) and a["meanActinicFlux"].shape == (nz,) and np.all(a["actinicFlux"] > 0)
    # the tally itself does not depend on the level tally beside it
    other = run_exact(M, name, True, not levels, calls)
    for k in ("actinicFlux", "meanActinicFlux"):
        for m in (0, 1):
            assert np.array_equal(on["mom"][k][m], other["mom"][k][m]), k


@pytest.mark.parametrize("name", ["regular, oblique, flat walk", "irregular, oblique back, nested walk"])
def test_the_bins_do_not_depend_on_the_split_into_batches(M, name):
    """The first moment sum of a bin is sum_b x_b n_b with x_b = raw_b / (n_b c) (c: the column's share and, for a cell, its
    depth), i.e. sum_b raw_b / c: the integer tallies of the batches add up to the one batch's tally whatever the split, so
    the sums of 8000 + 8000 + 4000 and of one batch of 20 000 differ by the rounding of the floats only -- each x_b is one
    float conversion and one division (2 x 2^-24), the photons per column one more, over three batches: 1e-6 relative bounds it,
    where a single missing or doubled deposit of the 10^5 in a bin would show at 1e-5."""
    split, whole = run_exact(M, name, True, False, CALLS), run_exact(M, name, True, False, WHOLE)
    for k in ("actinicFlux", "meanActinicFlux", "absorbedVolume", "fluxDown", "fluxUp"):
        a, b = np.asarray(split["mom"][k][0], np.float64), np.asarray(whole["mom"][k][0], np.float64)
        print("%s: %s: worst relative difference of the first moment sums %.3e" % (name, k, np.abs(a / b - 1.0).max()))
        assert np.all(b > 0) and np.abs(a / b - 1.0).max() < 1e-6, k


# 2 ---------------------------------------------------------------------------------------------------------------------------
OVERHEAD = [(grid, priv, block) for grid in LC.GRIDS for priv, block in ((0, 256), (2, 512))] + \
           [("regular", 0, 512), ("irregular", 2, 256)]


def _assert_overhead(res):
    for rep in res["reports"]:
        down = np.asarray(rep["fluxDown"], np.float64)
        act = np.asarray(rep["actinicFlux"], np.float64)
        assert np.all(down > 0)
        rel = np.abs(act / down[:, :, None] - 1.0)
        print("overhead sun: worst relative difference of actinicFlux from fluxDown %.3e" % rel.max())
        assert rel.max() < 1e-5
    st = res["stats"]
    assert np.abs(st["actinicFlux"] / st["fluxDown"][:, :, None] - 1.0).max() < 1e-5


@pytest.mark.parametrize("grid,priv,block", OVERHEAD)
def test_vacuum_under_an_overhead_sun(M, grid, priv, block):
    res = _trace(M, AC.vacuum_on(grid), dict(solarMu=1.0, solarAzimuth=0.0),
                 tuning=dict(privateTallies=priv, blockSize=block, eventThreshold=16), table=2001)
    _assert_overhead(res)


@pytest.mark.parametrize("name", list(AC.small_vacuums()))
@pytest.mark.parametrize("levels", [False, True])
def test_small_vacuums_under_an_overhead_sun(M, name, levels):
    res = _trace(M, AC.small_vacuums()[name], dict(solarMu=1.0, solarAzimuth=0.0), levels=levels, table=2001)
    _assert_overhead(res)


# 3 ---------------------------------------------------------------------------------------------------------------------------
def _area_weighted_layer_means(case, act):
    area = np.diff(case["xe"])[:, None] * np.diff(case["ye"])[None, :]
    return (np.asarray(act, np.float64) * area[:, :, None]).sum(axis=(0, 1)) / area.sum()


@pytest.mark.parametrize("priv,block", [(0, 256), (2, 512)])
def test_vacuum_under_an_oblique_sun(M, priv, block):
    """Every photon crosses every layer, whichever column it is in, with the path dz / mu0: the layer mean is 1 / mu0.

    Which mean: on irregular columns actinicFlux divides a cell's tally by the photons launched into ITS column (by area), and
    meanActinicFlux is the plain sum over the columns divided by their number, as meanLevelFluxUp is -- a photon that crosses
    into a narrower column counts for more there.  The quantity that is 1 / mu0 photon by photon is the AREA-weighted mean of
    actinicFlux over the layer (= total path in the layer / (photons dz)); that is what is held to 1e-5 here."""
    case = AC.vacuum_on("irregular")
    res = _trace(M, case, dict(solarMu=0.5, solarAzimuth=30.0), tuning=dict(privateTallies=priv, blockSize=block, eventThreshold=16), table=2001)
    for rep in res["reports"]:
        means = _area_weighted_layer_means(case, rep["actinicFlux"])
        print("oblique sun: area-weighted layer means * mu0 - 1:", means * 0.5 - 1.0)
        assert np.abs(means * 0.5 - 1.0).max() < 1e-5
        assert np.all(rep["fluxDown"] > 0)
    means = _area_weighted_layer_means(case, res["stats"]["actinicFlux"])
    assert np.abs(means * 0.5 - 1.0).max() < 1e-5


def _area_means_with_errors(M, case, source, tuning):
    """Area-weighted layer means per batch (one call per batch, from the last-batch results), their photon-weighted mean and
    the standard error of the batch spread, as driver.statistics forms it."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, source, tuning=tuning, table=2001)
    rns = new_RandomNumberSequence(SEED)
    ns, vals = [], []
    for n in (8000, 8000, 4000):
        assert integ.computeRadiativeTransfer(dom, rns, photons, n) == n
        ns.append(n)
        vals.append(_area_weighted_layer_means(case, integ.reportActinicFlux()["actinicFlux"]))
    assert integ.badPhotons() == 0
    integ.finalize()
    ns, vals = np.asarray(ns, np.float64)[:, None], np.asarray(vals)
    mean = (ns * vals).sum(axis=0) / ns.sum()
    second = (ns * vals * vals).sum(axis=0) / ns.sum()
    return mean, np.sqrt(np.maximum(0.0, second - mean ** 2) / (len(vals) - 1.0))


@pytest.mark.parametrize("what", ["white surface", "isotropic incidence"])
def test_vacuum_with_lambertian_legs(M, what):
    """Albedo 1 under the oblique sun: the reflected legs are Lambertian, <1 / mu> = 2, so 1 / mu0 + 2 = 2 / mu0 at mu0 = 0.5.
    The Flux source (isotropic incidence) over a black surface: 2.  Within 4.5 standard errors of the batch spread."""
    if what == "white surface":
        case, source, want = AC.vacuum_on("irregular", albedo=1.0), dict(solarMu=0.5, solarAzimuth=30.0), 2.0 / 0.5
    else:
        case, source, want = AC.vacuum_on("irregular"), dict(), 2.0
    mean, err = _area_means_with_errors(M, case, source, dict(privateTallies=0, blockSize=256, eventThreshold=16))
    print("%s: layer means %s, standard errors %s, z %s" % (what, mean, err, (mean - want) / err))
    assert np.all(err > 0) and np.all(np.abs(mean - want) < Z_BOUND * err)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _assert_track_length_against_collisions(case, res, label):
    st = res["stats"]
    sig = AC.sigma_abs(case)
    vol, act = np.asarray(st["absorbedVolume"], np.float64), np.asarray(st["actinicFlux"], np.float64)
    ea, ef = np.asarray(st["absorbedVolume_StdErr"], np.float64), sig * np.asarray(st["actinicFlux_StdErr"], np.float64) / 1000.0
    cells = sig > 0
    assert cells.sum() > 0 and np.all(ea[cells] > 0) and np.all(ef[cells] > 0)
    z = (vol - sig * act / 1000.0)[cells] / np.sqrt(ea ** 2 + ef ** 2)[cells]
    N = z.size
    print("%s: cells %d, max |z| %.2f (limit %.2f), mean z %.3f (limit %.3f), std z %.2f"
          % (label, N, np.abs(z).max(), max(4.0, np.sqrt(2.0 * np.log(N)) + 1.0), z.mean(), 0.2 + 3.0 / np.sqrt(N), z.std()))
    assert np.abs(z).max() < max(4.0, np.sqrt(2.0 * np.log(N)) + 1.0)
    assert abs(z.mean()) < 0.2 + 3.0 / np.sqrt(N)
    # the layer sums against absorbedProfile: profile(k) = mean over the columns of absorbedVolume, so the track-length twin is
    # the mean over the columns of sigma_abs actinicFlux / 1000.  The cells of a layer share photons, so the twin's standard
    # error is not the cells' in quadrature: it is the batch spread of the twin itself, formed per batch from the last-batch
    # results of every call (equal batches, one per call) as driver.statistics forms a standard error.
    ncol = sig.shape[0] * sig.shape[1]
    prof, ep = np.asarray(st["absorbedProfile"], np.float64), np.asarray(st["absorbedProfile_StdErr"], np.float64)
    per = np.array([(sig * np.asarray(r["actinicFlux"], np.float64) / 1000.0).sum(axis=(0, 1)) / ncol for r in res["reports"]])
    assert per.shape[0] == st["batches"]
    twin = per.mean(axis=0)
    et = np.sqrt(np.maximum(0.0, (per * per).mean(axis=0) - twin ** 2) / (per.shape[0] - 1.0))
    assert np.allclose(twin, (sig * act / 1000.0).sum(axis=(0, 1)) / ncol, rtol=1e-5)
    layers = sig.sum(axis=(0, 1)) > 0
    zl = (prof - twin)[layers] / np.sqrt(ep ** 2 + et ** 2)[layers]
    L = zl.size
    print("%s: layers %d, max |z| %.2f, mean z %.3f" % (label, L, np.abs(zl).max(), zl.mean()))
    assert np.abs(zl).max() < max(4.0, np.sqrt(2.0 * np.log(L)) + 1.0)
    assert abs(zl.mean()) < 0.2 + 3.0 / np.sqrt(L)


TRACK = [(grid, priv, block, rr) for grid, (priv, block, rr) in zip(LC.GRIDS, ((0, 256, True), (2, 512, False), (2, 256, True), (0, 512, False)))] + \
        [("regular", 2, 256, False), ("irregular", 2, 512, True), ("irregular z", 0, 256, True), ("irregular x y", 0, 256, False)]


@pytest.mark.parametrize("grid,priv,block,rr", TRACK)
def test_track_length_against_collisions(M, grid, priv, block, rr):
    case = LC.medium(grid)
    res = _trace(M, case, dict(solarMu=0.5, solarAzimuth=30.0), rr, dict(privateTallies=priv, blockSize=block, eventThreshold=16),
                 calls=((50000, 1),) * 40)
    _assert_track_length_against_collisions(case, res, "%s, PRIV %d, roulette %s" % (grid, priv, rr))


@pytest.mark.parametrize("rr", [True, False])
def test_track_length_against_collisions_on_the_stretched_cut(M, rr):
    case = LC.stretched_cut()
    res = _trace(M, case, dict(solarMu=0.5, solarAzimuth=30.0), rr, calls=((100000, 1),) * 40)
    _assert_track_length_against_collisions(case, res, "stretched cut, roulette %s" % rr)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_where_nothing_absorbs(M):
    """Two isotropically scattering layers (tau 0.5 conservative over tau 2 with omega0 = 0.9) over albedo 0.3 at mu0 = 0.6 on
    3 x 2 columns: the layer means of the actinic flux against 4 pi J of the integral-equation solver (its units are pinned
    by tests/test_actinic_host.py).  The medium is horizontally uniform, so the plain and the area-weighted mean have the same
    expectation; meanActinicFlux and its standard error are used.  4.5 standard errors plus 1e-5."""
    case, ref = AC.slab_case(), AC.layered_reference()
    res = _trace(M, case, dict(solarMu=AC.SLAB["mu0"], solarAzimuth=AC.SLAB["phi0"]), calls=((50000, 20),))
    st = res["stats"]
    got, err = np.asarray(st["meanActinicFlux"], np.float64), np.asarray(st["meanActinicFlux_StdErr"], np.float64)
    want = ref["actinic"][::-1]  # bottom up
    print("two layers: meanActinicFlux %s +- %s, 4 pi J %s, z %s" % (got, err, want, (got - want) / err))
    assert np.all(np.abs(got - want) < Z_BOUND * err + 1e-5)
    # the conservative layer: light where nothing is absorbed
    assert np.all(st["absorbedVolume"][:, :, 1] == 0) and np.all(st["actinicFlux"][:, :, 1] > 1.0)
    # and the absorbing one by both estimators
    prof = np.asarray(st["absorbedProfile"], np.float64) * np.diff(case["ze"]) * 1000.0  # flux absorbed per layer
    assert abs(prof[0] - ref["absorbed"][1]) < Z_BOUND * st["absorbedProfile_StdErr"][0] * np.diff(case["ze"])[0] * 1000.0 + 1e-5


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["regular", "irregular"])
def test_the_epilogue_bit_for_bit(M, grid):
    """The library does not hand out a batch's slab with the setting on (photon fates are refused with it), so the raw bins
    come by construction: in a vacuum under an overhead sun every photon adds ONE known integer to each cell of its column
    (tests/actinic_cases.py: overhead_deposits writes the leg's float arithmetic out), and the photons per column are
    fluxDown's whole numbers.  From these bins the expressions of the actinic parts of the finish kernels (cell_fold, batch_mean, mean_fold),
    written out in tests/actinic_cases.py, give actinicFlux, meanActinicFlux, both moment sums and the last-batch values --
    compared bit for bit."""
    case = AC.vacuum_on(grid)
    res = _trace(M, case, dict(solarMu=1.0, solarAzimuth=0.0), table=2001)
    g = EM.Grid(case["xe"], case["ye"], case["ze"])
    unit = AC.actinic_unit(case["xe"], case["ye"], case["ze"])
    per_photon = AC.overhead_deposits(case["ze"], LC.GRIDS[grid][1] == "regular", unit)
    assert np.all(per_photon > 0) and np.all(per_photon < 1 << 32)
    # photons per column of every batch: one-batch calls of the same ids give fluxDown = count / nppc
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, dict(solarMu=1.0, solarAzimuth=0.0), table=2001)
    rns = new_RandomNumberSequence(SEED)
    raws, last_reports = [], []
    for n in (8000, 8000, 4000):
        assert integ.computeRadiativeTransfer(dom, rns, photons, n) == n
        rep = integ.reportResults()
        counts = np.asarray(rep["fluxDown"], np.float64).T.reshape(-1) * g.photons_per_column(n).astype(np.float64)
        assert np.abs(counts - np.rint(counts)).max() < 1e-2 and np.rint(counts).sum() == n
        raws.append((np.rint(counts).astype(np.int64)[None, :] * per_photon[:, None]).reshape(-1))
        # a one-batch call is the mirror of one batch
        mean, cells = AC.actinic_values(g, raws[-1], n, unit)
        assert np.array_equal(rep["meanActinicFlux"], mean)
        assert np.array_equal(np.asarray(rep["actinicFlux"]).transpose(2, 1, 0).reshape(-1), cells)
    assert integ.badPhotons() == 0
    integ.finalize()
    s1, s2, last = AC.actinic_epilogue(g, np.stack(raws), CALLS, unit)
    nz, nvox = g.nz, g.nvox
    mom = res["mom"]
    assert np.array_equal(mom["meanActinicFlux"][0], s1[:nz]) and np.array_equal(mom["meanActinicFlux"][1], s2[:nz])
    assert np.array_equal(np.asarray(mom["actinicFlux"][0]).transpose(2, 1, 0).reshape(-1), s1[nz:])
    assert np.array_equal(np.asarray(mom["actinicFlux"][1]).transpose(2, 1, 0).reshape(-1), s2[nz:])
    final = res["reports"][-1]
    assert np.array_equal(final["meanActinicFlux"], last[:nz])
    assert np.array_equal(np.asarray(final["actinicFlux"]).transpose(2, 1, 0).reshape(-1), last[nz:])
    # the tail sits behind everything else in the raw array too
    M_ = res["len"]
    assert np.array_equal(res["raw"][8 + M_ - nz - nvox:8 + M_], s1) and np.array_equal(res["raw"][8 + 2 * M_ - nz - nvox:], s2)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def _raises(integ, rc, text):
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match=text):
        integ._check(rc)


def test_refusals_through_the_c_abi(M):
    from mcbrat3d_amd._capi import ptr
    case = AC.small_vacuums()["33 x 1 x 2"]
    dom, integ, photons = _integrator(M, case, dict(solarMu=0.5, solarAzimuth=0.0), actinic=False)
    L, ctx = integ._lib, integ._ctx
    act, levels, direct = (lambda on: L.mcbrat_specify_actinic_flux(ctx, on)), (lambda on: L.mcbrat_specify_level_fluxes(ctx, on)), \
        (lambda on: L.mcbrat_specify_direct_level_fluxes(ctx, on))
    length, walk = integ.momentsLength(), integ.walkMode()
    _raises(integ, L.mcbrat_report_actinic_flux(ctx, None, None), "actinic-flux information not available")
    integ._check(act(1))
    assert integ.momentsLength() == length + 2 * (1 + 33)
    _raises(integ, L.mcbrat_report_actinic_flux(ctx, None, None), "no batch has been traced yet")
    # the setting first: what it cannot be combined with is refused, and leaves the context as it was
    mus, phis = np.array([0.5], np.float32), np.array([0.0], np.float32)
    inten = lambda n: L.mcbrat_specify_intensity(ctx, n, ptr(mus), ptr(phis), 0, C.c_float(0.3), 0, 0, 0, C.c_float(1e30))  # noqa: E731
    xs, ys = np.array([0.0, 1.03125]), np.array([0.0, 0.5])
    rpv = np.array([0.1, 0.8, -0.1, 0.5], np.float32)
    _raises(integ, inten(1), "actinic flux.*intensity directions")
    _raises(integ, L.mcbrat_specify_scattering_orders(ctx, 3), "actinic flux.*scattering orders")
    _raises(integ, L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(ys), 4, ptr(rpv)), "actinic flux.*BRDF surface")
    _raises(integ, L.mcbrat_enable_counters(ctx, 1), "actinic flux.*event counters / photon fates")
    assert integ.momentsLength() == length + 2 * (1 + 33)
    # level fluxes are accepted beside it, their direct tally is not
    integ._check(levels(1))
    assert integ.momentsLength() == length + 2 * (1 + 33) + 2 * 3 * (1 + 33)
    _raises(integ, direct(1), "actinic flux.*direct level fluxes")
    assert integ.momentsLength() == length + 2 * (1 + 33) + 2 * 3 * (1 + 33)
    # the other order of calls
    integ._check(act(0)); integ._check(direct(1))
    _raises(integ, act(1), "actinic flux.*direct level fluxes")
    integ._check(direct(0)); integ._check(levels(0))
    assert integ.momentsLength() == length
    integ._check(inten(1)); _raises(integ, act(1), "actinic flux.*intensity directions"); integ._check(inten(0))
    integ._check(L.mcbrat_specify_scattering_orders(ctx, 3)); _raises(integ, act(1), "actinic flux.*scattering orders")
    integ._check(L.mcbrat_specify_scattering_orders(ctx, -1))
    integ._check(L.mcbrat_enable_counters(ctx, 1)); _raises(integ, act(1), "actinic flux.*event counters / photon fates")
    integ._check(L.mcbrat_enable_counters(ctx, 0))
    integ._check(L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(ys), 4, ptr(rpv))); _raises(integ, act(1), "actinic flux.*BRDF surface")
    integ._check(L.mcbrat_set_surface_brdf(ctx, 1, 0, 0, None, None, 0, None))  # back to the domain's albedo
    assert integ.momentsLength() == length and integ.walkMode() == walk
    # photon fates
    integ._check(act(1))
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    with pytest.raises(M.McbratError, match="actinic flux.*event counters / photon fates"):
        integ.traceFates(dom, new_RandomNumberSequence(SEED), photons, 100)
    # and after all that it traces, with level fluxes beside it
    integ._check(levels(1))
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000) == 1000
    mean = np.zeros(2, np.float32)
    integ._check(L.mcbrat_report_actinic_flux(ctx, ptr(mean), None))
    assert np.abs(mean * 0.5 - 1.0).max() < 1e-4
    integ.finalize()


def test_a_thermal_stream_is_refused_when_it_is_traced(M):
    from mcbrat3d_amd._capi import McbratError
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = cases.homog_lw(n=3)
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=2001, LW_flag=1.0, recActinicFlux=True)
    w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
    M.emission_weighting(dom, w, case["sfc_temp"])
    photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    with pytest.raises(McbratError, match="actinic flux.*thermal source"):
        integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000)
    integ.specifyParameters(recActinicFlux=False)  # without the setting the stream runs
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000) == 1000
    integ.finalize()


def test_the_bins_must_fit_the_tally_budget(M):
    """8192 x 8192 columns: 9 layers of 2^26 actinic bins of 8 bytes are 4.5 GiB and do not fit; 3 layers are 1.5 GiB and fit,
    and so do the two level parts of that grid alone (2 x 2^26 x 4 bins: 4 GiB, the budget) -- together they do not."""
    from mcbrat3d_amd._capi import ptr
    dom, integ, _ = _integrator(M, AC.small_vacuums()["1 x 1 x 1"], dict(solarMu=0.5, solarAzimuth=0.0))
    L, ctx = integ._lib, integ._ctx
    xe = np.arange(8193, dtype=np.float64)
    _raises(integ, L.mcbrat_set_grid(ctx, 8192, 8192, 9, ptr(xe), ptr(xe), ptr(np.arange(10, dtype=np.float64))), "actinic flux.*4 GiB tally budget")
    integ._check(L.mcbrat_set_grid(ctx, 8192, 8192, 3, ptr(xe), ptr(xe), ptr(np.arange(4, dtype=np.float64))))
    _raises(integ, L.mcbrat_specify_level_fluxes(ctx, 1), "actinic flux.*4 GiB tally budget")
    integ._check(L.mcbrat_specify_actinic_flux(ctx, 0)); integ._check(L.mcbrat_specify_level_fluxes(ctx, 1))
    _raises(integ, L.mcbrat_specify_actinic_flux(ctx, 1), "actinic flux.*4 GiB tally budget")
    integ.finalize()


def test_python_refusals_leave_the_integrator_as_it_was_and_the_copy_carries_the_setting(M):
    from mcbrat3d_amd._capi import McbratError
    dom, integ, photons = _integrator(M, AC.small_vacuums()["1 x 1 x 1"], dict(solarMu=0.5, solarAzimuth=0.0), actinic=False)
    length = integ.momentsLength()
    integ.specifyParameters(recActinicFlux=True)
    assert integ.momentsLength() == length + 2
    with pytest.raises(McbratError, match="actinic flux.*scattering orders"):
        integ.specifyParameters(recScatOrd=True, numRecScatOrd=2, useRussianRoulette=False)
    with pytest.raises(McbratError, match="actinic flux.*intensity directions"):
        integ.specifyParameters(intensityMus=[0.5], intensityPhis=[0.0], computeIntensity=True)
    with pytest.raises(McbratError, match="actinic flux.*direct level fluxes"):
        integ.specifyParameters(recLevelFluxes=True, recDirectLevelFluxes=True)
    assert integ.recActinicFlux and not integ.recLevelFluxes and integ.numRecScatOrd < 0 and integ.useRussianRoulette
    assert integ.momentsLength() == length + 2
    integ.specifyParameters(recLevelFluxes=True)  # accepted together
    assert integ.momentsLength() == length + 2 + 2 * 2 * 2
    twin = integ.copy_Integrator()
    assert twin.recActinicFlux and twin.recLevelFluxes and twin.momentsLength() == integ.momentsLength()
    twin.finalize()
    # from the direct tally to the actinic flux in one call, and back
    integ.specifyParameters(recActinicFlux=False, recDirectLevelFluxes=True)
    integ.specifyParameters(recActinicFlux=True, recDirectLevelFluxes=False)
    integ.specifyParameters(recLevelFluxes=False, recActinicFlux=False)
    assert integ.momentsLength() == length
    integ.finalize()
