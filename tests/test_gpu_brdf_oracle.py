"""The BRDF instantiations of trace_kernel (RPV, Ross-Li, Cox-Munk with and without its glint sampler; DESIGN.md sections 4.11 and
4.11.1) against the oracle's own statement of the four models (oracle.compute_rt_brdf, held on the CPU by
tests/test_oracle_brdf.py), in two tiers:

* exact -- photon ids the oracle calls clean (no stop point within 64 x 2^-23 x the path length of a face or of a patch edge, no
  decision of the reflection or of the roulette within the slack of its threshold), the same ids in the product on the same Philox
  streams in calls of at most 128 ids: every float of reportResults() -- fluxUp, fluxDown, the column absorption, the volume
  absorption, the profile, the three means and with orders on the order arrays -- inside a bracket derived from the two sides'
  arithmetic (brdf_cases.brdf_bracket); zero where the oracle deposited nothing.  A 3-D scattering medium over six unlike
  patches, on every plan the BRDF kernels are built for.  The product is never asked for photon fates;
* statistical -- level_cases.stretched_cut over each model's patches against the oracle's reference-faithful MT mode, fluxes and
  radiance per column: nothing shared but the physics."""
import numpy as np
import pytest

from tests import actinic_cases as AC
from tests import brdf_cases as BC
from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _integrator(M, case, mu0, phi0, rr, table, tuning, layer_skip, orders=0, views=None, glint=True, inten_rr=False):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    params = dict(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=rr, LW_flag=-1.0, surfaceBDRF=cases.product_surface(case))
    if orders:
        params.update(recScatOrd=True, numRecScatOrd=orders - 1)
    if views is not None:
        params.update(minForwardTableSize=BC.FWD_ANGLES, intensityMus=list(views[0]), intensityPhis=list(views[1]), computeIntensity=True,
                      useRussianRouletteForIntensity=inten_rr, zetaMin=BC.ZETA_MIN)
    integ.specifyParameters(**params)
    integ.setTuning(layerSkip=layer_skip, blockWalk=0, **tuning)
    if not glint:
        integ.setOption(glintSampling=0)
    return dom, integ, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)


# exact tier ----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(BC.EXACT))
def test_clean_photons_bin_by_bin(M, name):
    """Every maximal run of clean photon ids in calls of at most 128 ids, the oracle run on exactly those ids: each float of
    reportResults() lies in the bracket of brdf_cases.brdf_bracket (its docstring derives it), a bin is 0 where the oracle
    deposited nothing and positive where the bracket's lower end is.  On the rows with views the radiance of the same calls,
    summed, against the oracle's: direction means to 5e-4 relative, pixels to 1 % of the direction mean (the bounds of
    tests/test_gpu_intensity.py::test_step_cloud_radiance_matches_oracle_per_pixel, which leaves flipped histories in)."""
    from oracle import oracle as O
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    grid, mu0, phi0, model, glint, tuning, layer_skip, rr, orders, views = BC.EXACT[name]
    case, P, src, inten = BC.oracle_setup(name)
    near = BC.oracle_run(name, 0, BC.N_IDS)["nearFace"]
    runs = LC.clean_runs(near)
    calls = AC.split_runs(runs)
    dom, integ, photons = _integrator(M, case, mu0, phi0, rr, LC.TABLE, tuning, layer_skip, orders, BC.VIEWS if views else None, glint)
    integ.prepare(dom, photons)  # (the plan is made for a loaded domain: before it walkMode() echoes the walk options alone)
    walk = integ.walkMode()
    assert {k: walk[k] for k in BC.expected_walk(name)} == BC.expected_walk(name), walk
    g = EM.Grid(case["xe"], case["ye"], case["ze"])
    worst, width, rel_width, live, deposits, failures, fractions = -np.inf, 0.0, 0.0, 0, 0, [], []
    rad_got, rad_ref, traced = 0.0, 0.0, 0
    for first, count in calls:
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(LC.SEED, first), photons, count) == count
        got = BC.product_arrays(integ.reportResults(), orders)
        ref = O.compute_rt_brdf(P, src, O.philox_rng(LC.SEED, first), count, intensity=inten, orders=orders, delta=BC.DELTA)
        assert not ref["nearFace"].any() and ref["counters"]["badPhotons"] == 0
        bracket = BC.brdf_bracket(ref, case["xe"], case["ye"], case["ze"], count)
        bad = []
        for key, (lo, hi) in bracket.items():
            v = got[key]
            assert np.shape(v) == np.shape(lo), key
            out = (v < lo) | (v > hi) | ((v == 0) & (lo > 0))
            if key in BC.COUNTS:
                out |= (v != 0) & (ref[BC.COUNTS[key]] == 0)
                bins = ref[BC.COUNTS[key]] > 0
                live, deposits = live + int(bins.sum()), deposits + int(ref[BC.COUNTS[key]].sum())
                fractions.append(((hi - lo)[bins] / hi[bins]).astype(np.float64))
                wide = np.unravel_index(np.argmax(np.where(bins, hi - lo, -1.0)), hi.shape)
                if float(hi[wide] - lo[wide]) > width:
                    width, rel_width = float(hi[wide] - lo[wide]), float((hi[wide] - lo[wide]) / hi[wide])
            worst = max(worst, float(np.max(np.maximum(v - hi, lo - v))))
            if np.any(out):
                bad.append((key, np.argwhere(out)[:3].tolist(), np.asarray(v)[out][:3], np.asarray(lo)[out][:3], np.asarray(hi)[out][:3]))
        if bad:
            failures.append((first, count, bad))
        if views:
            nppc = g.photons_per_column(count).astype(np.float64).reshape(g.ny, g.nx)
            rad_got = rad_got + np.asarray(integ.reportResults()["intensity"], np.float64).transpose(2, 1, 0) * nppc[None]
            rad_ref = rad_ref + ref["intensity"].astype(np.float64).reshape(-1, g.ny, g.nx)
        traced += count
    bad_photons = integ.badPhotons()
    integ.finalize()
    clean = BC.N_IDS - int(near.sum())
    print("exact: %s: %d runs, %d calls, %d clean of %d ids (flagged %.4f), %d live bins, %d deposits; worst excess over the bracket "
          "over all floats %.3e (<= 0: inside), widest bracket %.3e, as a fraction of its bin's value %.3e (median over the live bins %.3e); "
          "calls outside %d" % (name, len(runs), len(calls), clean, BC.N_IDS, near.mean(), live, deposits, worst, width, rel_width,
                                float(np.median(np.concatenate(fractions))), len(failures)))
    assert not failures, (name, len(failures), failures[:2])
    assert bad_photons == 0 and traced == clean and deposits > clean
    if views:
        nppc = g.photons_per_column(traced).astype(np.float64).reshape(g.ny, g.nx)
        a, b = rad_got / nppc[None], rad_ref / nppc[None]
        ma, mb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
        print("exact: %s: radiance over the same calls: direction means %s against %s (relative %s), worst pixel difference over the "
              "direction mean %.3e" % (name, ma, mb, np.abs(ma / mb - 1.0), float((np.abs(a - b).max(axis=(1, 2)) / mb).max())))
        assert np.all(mb > 0) and np.allclose(ma, mb, rtol=5e-4, atol=0.0)
        assert np.all(np.abs(a - b).max(axis=(1, 2)) < 0.01 * mb)


# statistical tier ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", BC.STATISTICAL)
def test_patches_over_a_heterogeneous_medium_agree_with_the_mt_oracle(M, model):
    """4 x 10^6 photons of the product in 100 batches (a call each) against 10^6 of the oracle's MT mode in 100 batches: nothing shared but the
    physics.  Cox-Munk with the glint sampler on, two views, intensity roulette on.  The columns' fluxUp, fluxDown and absorption,
    the means, and the radiance per pixel and per direction with level_cases.assert_level_parity's bounds."""
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from oracle import oracle as O
    case = BC.statistical_case(model)
    dom, integ, photons = _integrator(M, case, BC.STAT_SUN[0], BC.STAT_SUN[1], True, 10001, {}, -1, 0, BC.STAT_VIEWS, True, inten_rr=True)
    integ.resetMoments()
    ppb, nb, per_direction = 40000, 100, []
    for b in range(nb):  # one batch per call, the moments adding up: each call's meanIntensity is that batch's mean per direction
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(77, b * ppb), photons, ppb) == ppb
        per_direction.append((ppb, np.asarray(integ.reportResults()["meanIntensity"], np.float64).copy()))
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, len(BC.STAT_VIEWS[0]), -1))
    assert st["totalPhotons"] == ppb * nb and st["batches"] == nb and integ.badPhotons() == 0
    integ.finalize()
    mi, mi_err = O.batch_statistics(per_direction)

    def cols(key):  # [ix, iy(, d)] -> x fastest, direction slowest
        v = np.asarray(st[key], np.float64)
        return (v.transpose(2, 1, 0) if v.ndim == 3 else v.T).reshape(-1)
    g = {"means": (np.concatenate([[st["meanFluxUp"], st["meanFluxDown"], st["meanFluxAbsorbed"]], mi]),
                   np.concatenate([[st["meanFluxUp_StdErr"], st["meanFluxDown_StdErr"], st["meanFluxAbsorbed_StdErr"]], mi_err])),
         "bins": tuple(np.concatenate([cols("fluxUp" + s), cols("fluxDown" + s), cols("fluxAbsorbed" + s), cols("intensity" + s)])
                       for s in ("", "_StdErr"))}
    c = BC.oracle_stat_run(model, "mt", 100, 10000, seed=10, procs=16)
    LC.assert_level_parity(g, c, "BRDF " + model)
