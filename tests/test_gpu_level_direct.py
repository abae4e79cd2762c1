"""The direct beam apart from the diffuse light in the downward level flux (recDirectLevelFluxes) on the GPU.

A photon is direct from its launch to its first collision or surface arrival.  What holds the direct tally:

1. the black twin (tests/level_direct_cases.py), product against product, bit for bit;
2. the oracle's level tallies of the twin over the clean photon ids of the real medium, no statistics;
3. the totals, and every older moment, are what they are without the setting, bit for bit;
4. identities of the definition (level numZ is all direct, 0 <= direct <= down, direct + diffuse = down to the rounding of the
   two floats, the direct beam only loses photons on its way down, a vacuum has no diffuse light);
5. Beer-Lambert for the direct mean and the plane-parallel solvers minus Beer-Lambert for the diffuse mean, at statistics;
6. the library's refusals, through the C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import level_cases as LC
from tests import level_direct_cases as DC

pytestmark = pytest.mark.gpu

SEED = 20251018
CALLS = ((8000, 2), (4000, 1))  # 20 000 photons in 3 batches: two of 8000 in one call, then the rest
Z_BOUND, Z_FLOOR = 4.5, 1e-6   # the theory tier of tests/test_gpu_level_flux_oracle.py
KEYS = ("levelFluxDownDirect", "levelFluxDownDiffuse", "meanLevelFluxDownDirect", "meanLevelFluxDownDiffuse")


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integrator(M, case, source, rr=True, table=LC.TABLE, direct=True, levels=True, tuning=None):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    surface = cases.product_surface(case)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=rr, LW_flag=-1.0, recLevelFluxes=levels,
                            recDirectLevelFluxes=direct, **({"surfaceBDRF": surface} if surface is not None else {}))
    if tuning:
        integ.setTuning(**tuning)
    return dom, integ, M.new_PhotonStream(numberOfPhotons=10 ** 12, **source)


def _trace(M, case, source, rr, tuning, direct):
    """-> dict(reports: reportLevelFluxes() after each call, raw: the moment array, mom: it unpacked, len: momentsLength())."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom, integ, photons = _integrator(M, case, source, rr, direct=direct, tuning=tuning)
    integ.resetMoments()
    rns = new_RandomNumberSequence(SEED)
    reports = []
    for ppb, nb in CALLS:
        assert integ.computeRadiativeTransfer(dom, rns, photons, ppb, nb) == ppb * nb
        reports.append(integ.reportLevelFluxes())
    raw = integ.moments().copy()
    assert integ.badPhotons() == 0 and raw.size == 8 + 2 * integ.momentsLength()
    out = dict(reports=reports, raw=raw, len=integ.momentsLength(), dims=(dom.numX, dom.numY, dom.numZ),
               mom=driver.unpack_moments(raw, dom.numX, dom.numY, dom.numZ, 0, -1, levelFluxes=True, directLevelFluxes=direct))
    integ.finalize()
    return out


_cache = {}


def run(M, name, variant):
    """The run of a medium of DC.MEDIA, traced once and shared (never modified).  variant: "direct" the real medium with the
    setting on, "plain" the real medium with level fluxes only, "twin" its black twin with level fluxes only."""
    if (name, variant) not in _cache:
        make, source, priv, block, rr = DC.MEDIA[name]
        case = DC.black_twin(make()) if variant == "twin" else make()
        _cache[name, variant] = _trace(M, case, source, rr, dict(privateTallies=priv, blockSize=block, eventThreshold=16), variant == "direct")
    return _cache[name, variant]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.MEDIA))
def test_the_direct_tally_is_the_black_twin_bit_for_bit(M, name):
    real, twin = run(M, name, "direct"), run(M, name, "twin")
    deposits = 0.0
    for got, ref in zip(real["reports"], twin["reports"]):
        assert np.array_equal(got["levelFluxDownDirect"], ref["levelFluxDown"])
        assert np.array_equal(got["meanLevelFluxDownDirect"], ref["meanLevelFluxDown"])
        assert not ref["levelFluxUp"].any() and not ref["meanLevelFluxUp"].any()
        deposits += float(ref["levelFluxDown"].astype(np.float64).sum())
    for m in (0, 1):  # both sums of the moment array
        assert np.array_equal(real["mom"]["levelFluxDownDirect"][m], twin["mom"]["levelFluxDown"][m])
        assert np.array_equal(real["mom"]["meanLevelFluxDownDirect"][m], twin["mom"]["meanLevelFluxDown"][m])
        assert not twin["mom"]["levelFluxUp"][m].any()
    nx, ny, nz = real["dims"]
    assert twin["mom"]["meanLevelFluxDown"][0][nz] > 0 and deposits > 0
    if name != "one cell":  # (something of the medium shows: the twin is not the vacuum)
        assert twin["mom"]["meanLevelFluxDown"][0][0] < 0.9 * twin["mom"]["meanLevelFluxDown"][0][nz]


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, v in LC.EXACT.items() if v[1] is not None])
def test_clean_photons_direct_bins_against_the_oracle_on_the_twin(M, name):
    """The clean id runs of the REAL medium (as test_clean_photons_bin_by_bin): the product's direct bins and means lie in the
    bracket of the oracle's level sums on the black twin over the same ids.  Every weight is 1, so the bracket is the epilogue's
    rounding only.  The ids left out are the real medium's flagged ids, whose share tests/test_oracle_levels.py holds."""
    from oracle import oracle as O
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    grid, mu0, phi0, priv, block, rr = LC.EXACT[name]
    case, P, src = LC.oracle_setup(name)
    Pt = cases.oracle_problem(DC.black_twin(case), nsteps=LC.TABLE, use_russian_roulette=rr)
    near = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, 0), LC.N_IDS)["nearFace"]
    runs = LC.clean_runs(near)
    dom, integ, photons = _integrator(M, case, dict(solarMu=mu0, solarAzimuth=phi0), rr,
                                      tuning=dict(privateTallies=priv, blockSize=block, eventThreshold=16))
    compared, deposits, worst = 0, 0, -np.inf
    for first, count in runs:
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(LC.SEED, first), photons, count) == count
        got = integ.reportLevelFluxes()
        ref = O.compute_rt_levels(Pt, src, O.philox_rng(LC.SEED, first), count)
        assert not ref["nearFace"].any() and ref["counters"]["badPhotons"] == 0  # the twin flags none of the real medium's clean ids
        assert not ref["levelUpCount"].any() and np.array_equal(ref["levelDown"], ref["levelDownCount"])  # nothing upward; weights 1
        bracket = LC.product_bracket(ref, case["xe"], case["ye"], count)
        v, (lo, hi) = got["levelFluxDownDirect"].transpose(2, 1, 0), bracket["levelFluxDown"]
        assert np.all((v >= lo) & (v <= hi)), (name, first, count, np.argwhere((v < lo) | (v > hi))[:5])
        assert not np.any((v > 0) & (ref["levelDownCount"] == 0)) and not np.any((v == 0) & (lo > 0)), (name, first)
        mean, (mlo, mhi) = got["meanLevelFluxDownDirect"], bracket["meanLevelFluxDown"]
        assert np.all((mean >= mlo) & (mean <= mhi)), (name, first, mean, mlo, mhi)
        worst = max(worst, float(np.maximum(v - hi, lo - v).max()), float(np.maximum(mean - mhi, mlo - mean).max()))
        compared += count
        deposits += int(ref["levelDownCount"].sum())
    assert integ.badPhotons() == 0
    integ.finalize()
    print("direct, exact: %s: %d runs, %d of %d ids compared (left out %.4f), %d direct deposits, worst excess over the bracket %.3e"
          % (name, len(runs), compared, LC.N_IDS, near.mean(), deposits, worst))
    assert compared == LC.N_IDS - int(near.sum()) and near.mean() <= 0.05
    assert deposits > compared


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.MEDIA))
def test_the_total_is_untouched(M, name):
    on, off = run(M, name, "direct"), run(M, name, "plain")
    for a, b in zip(on["reports"], off["reports"]):
        assert set(a) == set(b) | set(KEYS)
        for k in b:
            assert np.array_equal(a[k], b[k]), k
    nx, ny, nz = on["dims"]
    n0, n1 = off["len"], on["len"]
    assert n1 == n0 + 2 * (nz + 1) * (1 + nx * ny)
    # header, S1 and S2 of every older part of the moment array
    assert np.array_equal(on["raw"][:8 + n0], off["raw"][:8 + n0])
    assert np.array_equal(on["raw"][8 + n1:8 + n1 + n0], off["raw"][8 + n0:])


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _identities(case, r, n):
    from tests import epilogue_mirror as EM
    down, direct, diffuse = (r[k].astype(np.float64) for k in ("levelFluxDown", "levelFluxDownDirect", "levelFluxDownDiffuse"))
    nz = down.shape[2] - 1
    assert np.array_equal(r["levelFluxDownDirect"][:, :, nz], r["levelFluxDown"][:, :, nz])
    assert r["meanLevelFluxDownDirect"][nz] == r["meanLevelFluxDown"][nz]
    assert np.all(direct >= 0) and np.all(direct <= down) and np.all(diffuse >= 0)
    assert np.all(np.abs(direct + diffuse - down) <= 4.0 * 2.0 ** -24 * down)
    md, mdir, mdif = (r[k].astype(np.float64) for k in ("meanLevelFluxDown", "meanLevelFluxDownDirect", "meanLevelFluxDownDiffuse"))
    assert np.all(mdir >= 0) and np.all(mdir <= md) and np.all(mdif >= 0)
    # raw direct counts: every direct weight is 1, so a bin is (count / nppc) in float, count <= n < 2^24 -- recovered exactly
    nppc = EM.Grid(case["xe"], case["ye"], [0.0, 1.0]).photons_per_column(n).astype(np.float64).reshape(down.shape[1], down.shape[0]).T
    counts = direct * nppc[:, :, None]
    assert np.all(np.abs(counts - np.rint(counts)) < 1e-3)
    per_level = np.rint(counts).sum(axis=(0, 1))
    assert per_level[nz] == n and np.all(np.diff(per_level) >= 0)  # nothing joins the direct beam on its way down
    return per_level


@pytest.mark.parametrize("name", list(DC.MEDIA))
def test_identities_of_the_definition(M, name):
    make = DC.MEDIA[name][0]
    case = make()
    for r, (ppb, _) in zip(run(M, name, "direct")["reports"], CALLS):
        per_level = _identities(case, r, ppb)
    if name != "one cell":
        assert per_level[0] < per_level[-1]


def test_a_vacuum_has_no_diffuse_light(M):
    case = DC.vacuum()
    res = _trace(M, case, dict(solarMu=0.5, solarAzimuth=30.0), True, dict(eventThreshold=16), True)
    for r, (ppb, _) in zip(res["reports"], CALLS):
        _identities(case, r, ppb)
        assert np.array_equal(r["levelFluxDownDirect"], r["levelFluxDown"]) and not r["levelFluxDownDiffuse"].any()
        assert np.array_equal(r["meanLevelFluxDownDirect"], r["meanLevelFluxDown"]) and not r["meanLevelFluxDownDiffuse"].any()
        assert np.all(r["meanLevelFluxUp"] > 0)  # (the surface reflects: the reflected photons come down nowhere)
    for m in (0, 1):
        assert np.array_equal(res["mom"]["levelFluxDownDirect"][m], res["mom"]["levelFluxDown"][m])
        assert not res["mom"]["levelFluxDownDiffuse"][m].any() and not res["mom"]["meanLevelFluxDownDiffuse"][m].any()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["isotropic layers over albedo 0.5", "HG g = 0.85, tau = 4, regular z", "homogeneous on a stretched 7 x 5 x 12 grid"])
def test_direct_and_diffuse_means_against_theory(M, name):
    """meanLevelFluxDownDirect(k) against exp(-tau_k / mu0), meanLevelFluxDownDiffuse(k) against the solver's downward flux minus
    that; 4 x 10^6 photons in 40 batches, the bound of the existing theory tier.  On the stretched grid every column's direct
    profile is the slab's too: by that bound where the batches' spread is a standard error, by the count's own Poisson
    distribution at the same probability where a bin sees a handful of photons or none (below)."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    t = LC.theory(name)
    beam = np.exp(-DC.optical_depth_above_levels(t["case"]) / t["mu0"])
    dom, integ, photons = _integrator(M, t["case"], dict(solarMu=t["mu0"], solarAzimuth=t["phi0"]), True, table=t["table"])
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 100000, 40) == 4000000
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, 0, -1, levelFluxes=True, directLevelFluxes=True))
    assert integ.badPhotons() == 0
    integ.finalize()
    for key, want in (("LevelFluxDownDirect", beam), ("LevelFluxDownDiffuse", t["down"] - beam)):
        got, err = st["mean" + key], st["mean" + key + "_StdErr"]
        print("theory: %s: mean%s z-scores %s" % (name, key, np.round((got - want) / np.maximum(err, 1e-30), 2)))
        assert np.all(np.abs(got - want) < Z_BOUND * err + Z_FLOOR), (key, got, want, err)
    assert beam[0] < 0.5 and np.all(t["down"] - beam > -1e-9)  # (the solver's own precision)
    if dom.numX * dom.numY > 1:
        # Every column's direct profile is the slab's.  A direct deposit has weight 1, so a bin is a count over the photons per
        # column: (number of photons that cross level k in the column) / nppc, the count binomial with a small probability --
        # Poisson with mean lambda = beam(k) nppc.  Where a batch expects 25 deposits or more the batch means are normal and their
        # spread over 40 batches is a standard error: the tier's bound.  Below that (down to 0.2 deposits in the whole run at the
        # bottom of tau / mu0 = 13) it is not -- a bin nobody reached has "standard error" 0 -- and the same two-sided
        # probability, that of 4.5 standard deviations of a normal variable, bounds the count in its own Poisson distribution.
        from scipy.special import erfc
        from scipy.stats import poisson
        from tests import epilogue_mirror as EM
        nppc = EM.Grid(t["case"]["xe"], t["case"]["ye"], [0.0, 1.0]).photons_per_column(4000000).astype(np.float64).reshape(dom.numY, dom.numX).T
        lam = beam[None, None, :] * nppc[:, :, None]
        normal = lam / 40.0 >= 25.0
        col, cerr = st["levelFluxDownDirect"], st["levelFluxDownDirect_StdErr"]
        z = (col - beam[None, None, :]) / np.maximum(cerr, 1e-30)
        print("theory: %s: levelFluxDownDirect per column: max |z| %.2f over %d bins of 25 deposits per batch or more" % (name, np.abs(z[normal]).max(), normal.sum()))
        assert np.all((np.abs(col - beam[None, None, :]) < Z_BOUND * cerr + Z_FLOOR)[normal]), np.abs(z[normal]).max()
        counts = col * nppc[:, :, None]
        assert np.all(np.abs(counts - np.rint(counts)) < 1e-3 * np.maximum(1.0, counts * 1e-3))  # (whole photons)
        counts = np.rint(counts)
        tail = np.minimum(poisson.cdf(counts, lam), poisson.sf(counts - 1.0, lam))
        print("theory: %s: levelFluxDownDirect per column: smallest Poisson tail %.3e over %d bins below that, %d of them empty"
              % (name, tail[~normal].min(), (~normal).sum(), (counts[~normal] == 0).sum()))
        assert np.all(tail[~normal] >= 0.5 * erfc(Z_BOUND / np.sqrt(2.0)))
        assert normal[:, :, -2:].all() and not normal[:, :, :2].any()  # (both regimes are there, in every column)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def _raises(integ, rc, text):
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match=text):
        integ._check(rc)


def test_refusals_through_the_c_abi(M):
    from mcbrat3d_amd._capi import ptr
    dom, integ, photons = _integrator(M, DC.thirty_three_columns(), dict(solarMu=0.5, solarAzimuth=0.0), direct=False, levels=False)
    L, ctx = integ._lib, integ._ctx
    levels, direct = (lambda on: L.mcbrat_specify_level_fluxes(ctx, on)), (lambda on: L.mcbrat_specify_direct_level_fluxes(ctx, on))
    length = integ.momentsLength()
    # the setting without level fluxes, and level fluxes switched off under it
    _raises(integ, direct(1), "direct level fluxes.*need level fluxes")
    assert integ.momentsLength() == length
    _raises(integ, L.mcbrat_report_direct_level_fluxes(ctx, None, None, None, None), "direct level-flux information not available")
    integ._check(levels(1)); integ._check(direct(1))
    assert integ.momentsLength() == length + 4 * 3 * (1 + 33)
    _raises(integ, L.mcbrat_report_direct_level_fluxes(ctx, None, None, None, None), "no batch has been traced yet")
    _raises(integ, levels(0), "direct level fluxes.*need level fluxes")
    # everything level fluxes are refused with, while both are on
    mus, phis = np.array([0.5], np.float32), np.array([0.0], np.float32)
    inten = lambda n: L.mcbrat_specify_intensity(ctx, n, ptr(mus), ptr(phis), 0, C.c_float(0.3), 0, 0, 0, C.c_float(1e30))  # noqa: E731
    xs, ys = np.array([0.0, 0.515625]), np.array([0.0, 0.0625])
    rpv = np.array([0.1, 0.8, -0.1, 0.5], np.float32)
    _raises(integ, inten(1), "level fluxes.*intensity directions")
    _raises(integ, L.mcbrat_specify_scattering_orders(ctx, 3), "level fluxes.*scattering orders")
    _raises(integ, L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(ys), 4, ptr(rpv)), "level fluxes.*BRDF surface")
    _raises(integ, L.mcbrat_enable_counters(ctx, 1), "level fluxes.*event counters / photon fates")
    # ... and in the other order of calls: what refuses level fluxes leaves nothing for the setting to separate
    integ._check(direct(0)); integ._check(levels(0))
    assert integ.momentsLength() == length
    integ._check(inten(1)); _raises(integ, levels(1), "level fluxes.*intensity directions"); _raises(integ, direct(1), "need level fluxes")
    integ._check(inten(0))
    integ._check(L.mcbrat_specify_scattering_orders(ctx, 3)); _raises(integ, levels(1), "level fluxes.*scattering orders")
    _raises(integ, direct(1), "need level fluxes"); integ._check(L.mcbrat_specify_scattering_orders(ctx, -1))
    integ.finalize()


def test_a_thermal_stream_is_refused_when_it_is_traced(M):
    from mcbrat3d_amd._capi import McbratError
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from tests.test_gpu_level_flux import thermal_case
    case = thermal_case()
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=9001, LW_flag=1.0, recLevelFluxes=True, recDirectLevelFluxes=True)
    w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
    M.emission_weighting(dom, w, case["sfc_temp"])
    photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    with pytest.raises(McbratError, match="direct level fluxes.*thermal source"):
        integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000)
    integ.specifyParameters(recDirectLevelFluxes=False)  # level fluxes alone run with it
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 1000) == 1000
    integ.finalize()


def test_three_level_parts_must_fit_the_tally_budget(M):
    """8192 x 8192 columns on 3 levels: two level parts of 2^26 x 3 bins of 8 bytes are 3 GiB and fit, three are 4.5 GiB."""
    from mcbrat3d_amd._capi import ptr
    dom, integ, _ = _integrator(M, DC.one_cell(), dict(solarMu=0.5, solarAzimuth=0.0), direct=True)
    L, ctx = integ._lib, integ._ctx
    xe, ze = np.arange(8193, dtype=np.float64), np.arange(3, dtype=np.float64)
    _raises(integ, L.mcbrat_set_grid(ctx, 8192, 8192, 2, ptr(xe), ptr(xe), ptr(ze)), "direct level fluxes.*level bins.*4 GiB tally budget")
    integ._check(L.mcbrat_specify_direct_level_fluxes(ctx, 0))
    integ._check(L.mcbrat_set_grid(ctx, 8192, 8192, 2, ptr(xe), ptr(xe), ptr(ze)))  # level fluxes alone fit
    _raises(integ, L.mcbrat_specify_direct_level_fluxes(ctx, 1), "direct level fluxes.*level bins.*4 GiB tally budget")
    integ.finalize()


def test_python_refusals_leave_the_integrator_as_it_was_and_the_copy_carries_the_setting(M):
    from mcbrat3d_amd._capi import McbratError
    dom, integ, photons = _integrator(M, DC.one_cell(), dict(solarMu=0.5, solarAzimuth=0.0), direct=False, levels=False)
    length = integ.momentsLength()
    with pytest.raises(McbratError, match="direct level fluxes.*need level fluxes"):
        integ.specifyParameters(recDirectLevelFluxes=True, useRussianRoulette=False)
    assert not integ.recDirectLevelFluxes and not integ.recLevelFluxes and integ.useRussianRoulette and integ.momentsLength() == length
    integ.specifyParameters(recLevelFluxes=True, recDirectLevelFluxes=True)
    assert integ.momentsLength() == length + 4 * 2 * 2
    with pytest.raises(McbratError, match="direct level fluxes.*need level fluxes"):
        integ.specifyParameters(recLevelFluxes=False)
    with pytest.raises(McbratError, match="level fluxes.*scattering orders"):
        integ.specifyParameters(recScatOrd=True, numRecScatOrd=2)
    assert integ.recDirectLevelFluxes and integ.recLevelFluxes and integ.numRecScatOrd < 0
    twin = integ.copy_Integrator()
    assert twin.recDirectLevelFluxes and twin.momentsLength() == integ.momentsLength()
    twin.finalize()
    integ.specifyParameters(recLevelFluxes=False, recDirectLevelFluxes=False)
    assert integ.momentsLength() == length
    integ.finalize()
