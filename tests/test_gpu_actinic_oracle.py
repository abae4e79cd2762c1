"""The product's actinic flux (recActinicFlux) against the oracle's track-length tally
(oracle.compute_rt_actinic, held on the CPU by tests/test_oracle_actinic.py) and against transport theory, in three tiers:

* exact -- photon ids the oracle calls clean (no stop point within delta = 64 x 2^-23 x the path length of a face, no step past an
  edge or a corner of a cell within delta), the same ids in the product on the same Philox streams in calls of at most 128 ids:
  every cell and every layer mean inside a bracket derived from the two tallies' arithmetic (actinic_cases.actinic_bracket), no
  statistics -- a piece of path that is missing, misplaced by one cell or carried at another weight stands far outside it;
* statistical -- heterogeneous 3-D media against the oracle's reference-faithful MT mode, cell by cell;
* theory -- the layer means (and on the stretched grid every cell) against the deterministic profiles of tests/test_analytic.py:
  what a layer absorbs is the difference of the net flux between its two levels."""
import numpy as np
import pytest

from tests import actinic_cases as AC
from tests import cases
from tests import level_cases as LC

pytestmark = pytest.mark.gpu

SEED = 20241005
Z_BOUND = 4.5


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integrator(M, case, mu0, phi0, rr, table, levels=False, tuning=None):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    surface = cases.product_surface(case)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=rr, LW_flag=-1.0, recLevelFluxes=levels,
                            recActinicFlux=True, **({"surfaceBDRF": surface} if surface is not None else {}))
    integ.setTuning(layerSkip=0, blockWalk=0, **(tuning or {}))
    return dom, integ, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)


# exact tier ----------------------------------------------------------------------------------------------------------
WITH_LEVELS = ("regular, oblique, flat walk", "irregular, oblique back, nested walk")  # one per form of the walk: the LVL + ACT kernels
EXACT = [(name, False) for name in AC.SOLAR_EXACT] + [(name, True) for name in WITH_LEVELS]


@pytest.mark.parametrize("name,levels", EXACT, ids=[n + (", level fluxes on" if lv else "") for n, lv in EXACT])
def test_clean_photons_cell_by_cell(M, name, levels):
    """Every maximal run of clean photon ids in calls of at most 128 ids, the oracle run on exactly those ids: each float of
    reportActinicFlux() lies in the bracket of actinic_cases.actinic_bracket (its docstring derives it), and a cell is zero in
    the product where the oracle deposited nothing.  With level fluxes on, the level bins of the same calls lie in
    level_cases.product_bracket as well."""
    from oracle import oracle as O
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    grid, mu0, phi0, priv, block, rr = LC.EXACT[name]
    case, P, src = LC.oracle_setup(name)
    near = O.compute_rt_actinic(P, src, O.philox_rng(LC.SEED, 0), LC.N_IDS)["nearFace"]
    runs = LC.clean_runs(near)
    calls = AC.split_runs(runs)
    dom, integ, photons = _integrator(M, case, mu0, phi0, rr, LC.TABLE, levels, dict(privateTallies=priv, blockSize=block, eventThreshold=16))
    walk = integ.walkMode()
    assert not walk["layerSkip"] and not walk["blockWalk"] and not walk["clearAirFlight"]
    worst, width, rel_width, live, deposits, failures, fractions = -np.inf, 0.0, 0.0, 0, 0, [], []
    lvl_worst, lvl_deposits = -np.inf, 0
    for first, count in calls:
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(LC.SEED, first), photons, count) == count
        got = integ.reportActinicFlux()
        ref = O.compute_rt_actinic(P, src, O.philox_rng(LC.SEED, first), count)
        assert not ref["nearFace"].any() and ref["counters"]["badPhotons"] == 0
        bracket = AC.actinic_bracket(ref, case["xe"], case["ye"], case["ze"], count)
        v, (lo, hi) = np.asarray(got["actinicFlux"]).transpose(2, 1, 0), bracket["actinicFlux"]  # [k, iy, ix]
        mean, (mlo, mhi) = np.asarray(got["meanActinicFlux"]), bracket["meanActinicFlux"]
        out = (v < lo) | (v > hi)
        if out.any() or np.any((mean < mlo) | (mean > mhi)) or np.any((v > 0) & (ref["actinicCount"] == 0)):
            failures.append((first, count, np.argwhere(out)[:4].tolist(), v[out][:4], lo[out][:4], hi[out][:4], mean, mlo, mhi))
        bins = ref["actinicCount"] > 0
        worst = max(worst, float(np.maximum(v - hi, lo - v)[bins | (v > 0)].max()), float(np.maximum(mean - mhi, mlo - mean).max()))
        wide = np.unravel_index(np.argmax(np.where(bins, hi - lo, -1.0)), hi.shape)
        if float(hi[wide] - lo[wide]) > width:
            width, rel_width = float(hi[wide] - lo[wide]), float((hi[wide] - lo[wide]) / hi[wide])
        fractions.append(((hi - lo)[bins] / hi[bins]).astype(np.float64))
        live += int(bins.sum())
        deposits += int(ref["actinicCount"].sum())
        if levels:
            lv, lb = integ.reportLevelFluxes(), LC.product_bracket(ref, case["xe"], case["ye"], count)
            for key, raw in (("levelFluxUp", "levelUp"), ("levelFluxDown", "levelDown")):
                u, (ulo, uhi) = lv[key].transpose(2, 1, 0), lb[key]
                um, (umlo, umhi) = lv["mean" + key[0].upper() + key[1:]], lb["mean" + key[0].upper() + key[1:]]
                assert np.all((u >= ulo) & (u <= uhi)) and np.all((um >= umlo) & (um <= umhi)), (name, key, first, count)
                assert not np.any((u > 0) & (ref[raw + "Count"] == 0)) and not np.any((u == 0) & (ulo > 0)), (name, key, first)
                lvl_worst = max(lvl_worst, float(np.maximum(u - uhi, ulo - u).max()), float(np.maximum(um - umhi, umlo - um).max()))
                lvl_deposits += int(ref[raw + "Count"].sum())
    bad = integ.badPhotons()
    integ.finalize()
    clean = LC.N_IDS - int(near.sum())
    print("exact: %s%s: %d runs, %d calls, %d clean of %d ids (flagged %.4f), %d live bins, %d deposits; worst excess over the bracket "
          "over the live bins and the means %.3e (<= 0: inside), widest bracket %.3e, as a fraction of its bin's value %.3e (median over the live bins %.3e); "
          "calls outside %d"
          % (name, ", level fluxes on" if levels else "", len(runs), len(calls), clean, LC.N_IDS, near.mean(), live, deposits, worst, width,
             rel_width, float(np.median(np.concatenate(fractions))), len(failures)))
    if levels:
        print("exact: %s: level bins beside it: %d deposits, worst excess over level_cases.product_bracket %.3e" % (name, lvl_deposits, lvl_worst))
    assert not failures, (name, len(failures), failures[:3])
    assert bad == 0 and deposits > clean and (not levels or lvl_deposits > clean)


# statistical tier ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.STATISTICAL))
def test_heterogeneous_media_agree_with_the_mt_oracle_cell_by_cell(M, name):
    """4 x 10^6 photons of the product in 100 batches against 10^6 of the oracle's MT mode in 100 batches: nothing shared but the
    physics.  Every cell and every layer mean with level_cases.assert_level_parity's bounds."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    make, mu0, phi0 = LC.STATISTICAL[name]
    case = make()
    dom, integ, photons = _integrator(M, case, mu0, phi0, True, 10001)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(77), photons, 40000, 100) == 4000000
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, 0, -1, actinicFlux=True))
    assert integ.badPhotons() == 0
    integ.finalize()
    g = {"means": (np.asarray(st["meanActinicFlux"], np.float64), np.asarray(st["meanActinicFlux_StdErr"], np.float64)),
         "bins": (np.asarray(st["actinicFlux"], np.float64).T.reshape(-1), np.asarray(st["actinicFlux_StdErr"], np.float64).T.reshape(-1))}
    c = AC.oracle_actinic_run(name, "mt", 100, 10000, seed=10, procs=16)
    LC.assert_level_parity(g, c, "actinic, " + name)


# theory tier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.SOLAR_THEORY)
def test_mean_actinic_flux_against_theory(M, name):
    """meanActinicFlux at every absorbing layer against (net flux in - net flux out) / ((1 - omega) dtau) of the deterministic
    level profiles, 4 x 10^6 photons in 40 batches; on the stretched grid every cell against its layer's value (column
    attribution on irregular x / y / z).  4.5 standard errors plus the level tier's floor of 1e-6 on each of the four fluxes,
    carried through the quotient: 4e-6 / ((1 - omega) dtau)."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    t = AC.actinic_theory(name)
    dom, integ, photons = _integrator(M, t["case"], t["mu0"], t["phi0"], True, t["table"])
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, 100000, 40) == 4000000
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, 0, -1, actinicFlux=True))
    assert integ.badPhotons() == 0
    integ.finalize()
    k, want, floor = t["layers"], t["actinic"], t["floor"]
    assert k.sum() >= 6
    got, err = np.asarray(st["meanActinicFlux"], np.float64), np.asarray(st["meanActinicFlux_StdErr"], np.float64)
    print("theory: %s: meanActinicFlux z-scores %s" % (name, np.round(((got - want) / np.maximum(err, 1e-30))[k], 2)))
    assert np.all(np.abs(got - want)[k] < (Z_BOUND * err + floor)[k]), (got, want, err)
    if name.startswith("homogeneous on a stretched"):
        cell, cerr = np.asarray(st["actinicFlux"], np.float64), np.asarray(st["actinicFlux_StdErr"], np.float64)  # [ix, iy, k]
        z = (cell - want[None, None, :]) / np.maximum(cerr, 1e-30)
        print("theory: %s: actinicFlux per cell: max |z| %.2f, mean z %.3f over %d cells" % (name, np.abs(z[:, :, k]).max(), z[:, :, k].mean(), z[:, :, k].size))
        assert np.all(cerr[:, :, k] > 0) and np.all(np.abs(cell - want[None, None, :])[:, :, k] < (Z_BOUND * cerr + floor[None, None, :])[:, :, k])
