"""The oracle's level tallies (oracle.compute_rt_levels: upward and downward flux through every level of every column, DESIGN.md
section 4.12 restated on the CPU) held to what they must obey before the GPU tests lean on them: exact identities per batch, the
reference-faithful MT mode against the Philox mode, transport theory at every level, and -- on the very inputs of
tests/test_gpu_level_flux_oracle.py's photon-by-photon comparison -- the share of photons that comparison leaves out."""
import numpy as np
import pytest

from tests import level_cases as LC

SEED = 20241005


def _without_roulette(name):
    from oracle import oracle as O
    from tests import cases
    grid, mu0, phi0 = LC.EXACT[name][:3]
    case = LC.medium(grid, thermal=mu0 is None)
    P = cases.oracle_problem(case, nsteps=LC.TABLE, use_russian_roulette=False, lw_flag=1.0 if mu0 is None else -1.0)
    if mu0 is None:
        vw, frac, _ = O.emission_weighting(P, case["temps"].transpose(2, 1, 0).reshape(-1), case["lambda_um"], case["sfc_temp"])
        return P, O.EmissionSource(vw, frac), frac
    return P, O.solar_source(mu0, phi0), None


@pytest.mark.parametrize("name", ["regular, oblique, flat walk", "irregular, oblique back, nested walk", "thermal, irregular z"])
def test_identities_per_batch(name):
    """Level nz upward is the raw fluxUp and level 0 downward the raw fluxDown: the same deposits, summed in double here and in
    float there, so equal to within the float tally's rounding -- at most half an ulp of the running sum per addition,
    (deposits) x 2^-24 x (the sum).  Every solar photon is launched through level nz, and nothing else goes down through it: the
    launch deposits add up to the photon count exactly.  The net downward flux into layer k minus that out of it is the layer's
    volume absorption (with the thermal launch's -1), roulette off: per photon exact but for float(w (1 - omega0)) + float(w omega0)
    against w, 2^-24 per collision, and for the float volume tally's own rounding as above."""
    from oracle import oracle as O
    P, src, frac = _without_roulette(name)
    n, nz = 10000, P.nz
    for batch in range(3):
        r = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, batch * n), n)
        plain = O.compute_rt(P, src, O.philox_rng(LC.SEED, batch * n), n)
        for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption"):
            assert np.array_equal(r[k], plain[k]), k  # (the tallies of orc_compute_rt do not notice)
        assert r["counters"] == plain["counters"] and r["counters"]["badPhotons"] == 0
        for level, key, flux in ((nz, "levelUp", "fluxUp"), (0, "levelDown", "fluxDown")):
            s, c = r[key][level].reshape(-1), r[key + "Count"][level].reshape(-1)
            assert s.sum() > 0 and np.all(np.abs(s - r[flux]) <= c * 2.0 ** -24 * s)
        if frac is None:
            assert r["levelDown"][nz].sum() == n and r["levelDownCount"][nz].sum() == n and r["levelUpCount"][nz].sum() == r["counters"]["topExits"]
        else:  # thermal: nothing enters from above; every atmospheric launch leaves its -1 in the volume tally
            assert r["levelDown"][nz].sum() == 0.0
    # (the divergence in batches of 500 photons: the worst-case bound grows with the square of the batch, a deposit does not)
    n = 500
    for batch in range(6):
        r = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, 50000 + batch * n), n)
        net = (r["levelDown"] - r["levelUp"]).sum(axis=(1, 2))
        vol = r["volumeAbsorption"].reshape(nz, -1).astype(np.float64)
        tol = r["counters"]["collisions"] * 2.0 ** -24 * (1.0 + np.abs(vol).max())
        worst = np.abs(net[1:] - net[:-1] - vol.sum(axis=1)).max()
        print(name, "batch", batch, "divergence: worst %.3e, tolerance %.3e" % (worst, tol))
        assert worst <= tol and np.abs(vol).max() > 1.0 and tol < 0.02  # (far below one deposit: the lightest photon weighs 0.6^n)


def test_surface_emitted_photons_cross_level_0_upward_with_weight_1():
    """Over a black surface nothing but the surface's own emission goes up through level 0: one deposit of weight 1 per
    surface-emitted photon, whose number is binomial in the surface's share of the emitted power."""
    from oracle import oracle as O
    from tests import cases
    case = LC.medium("irregular z", thermal=True)
    case["albedo"] = 0.0
    P = cases.oracle_problem(case, nsteps=LC.TABLE, lw_flag=1.0)
    vw, frac, _ = O.emission_weighting(P, case["temps"].transpose(2, 1, 0).reshape(-1), case["lambda_um"], case["sfc_temp"])
    n = 20000
    r = O.compute_rt_levels(P, O.EmissionSource(vw, frac), O.philox_rng(LC.SEED, 0), n)
    launched = r["levelUpCount"][0].sum()
    assert r["levelUp"][0].sum() == launched and r["levelDown"][P.nz].sum() == 0.0
    assert abs(launched / n - (1.0 - frac)) < 4.5 * np.sqrt(frac * (1.0 - frac) / n)


def test_philox_mode_agrees_with_mt_mode_level_by_level():
    """tests/test_oracle_modes.py's statistic and bounds on the level bins of a heterogeneous 3-D medium over a patchy surface."""
    name = "stretched 8 x 6 x 10 over patches"
    a = LC.oracle_level_run(name, "philox", 30, 10000, seed=10)
    b = LC.oracle_level_run(name, "mt", 30, 10000, seed=10)
    LC.assert_level_parity(a, b, name)


@pytest.mark.parametrize("name", ["isotropic layers over albedo 0.5", "HG g = 0.85, tau = 4, regular z", "thermal slab"])
def test_oracle_level_fluxes_against_theory(name):
    """Upward and downward flux at every level against the deterministic profiles of tests/test_analytic.py: 4.5 standard errors
    (from the variance of 25 batches of 10^4 photons) + 10^-6."""
    from oracle import oracle as O
    from tests import cases
    t = LC.theory(name)
    case, thermal = t["case"], t["mu0"] is None
    P = cases.oracle_problem(case, nsteps=t["table"], lw_flag=1.0 if thermal else -1.0)
    if thermal:
        vw, frac, _ = O.emission_weighting(P, case["temps"].transpose(2, 1, 0).reshape(-1), case["lambda_um"], case["sfc_temp"])
        src = O.EmissionSource(vw, frac)
    else:
        src = O.solar_source(t["mu0"], t["phi0"])
    per, nb = 10000, 25
    rows = {"meanLevelFluxUp": [], "meanLevelFluxDown": []}
    for b in range(nb):
        r = O.compute_rt_levels(P, src, O.philox_rng(SEED, b * per), per)
        v = O.normalize_levels(P, r["n"], r)
        for k in rows:
            rows[k].append((per, v[k]))
    for k, want in (("meanLevelFluxUp", t["up"]), ("meanLevelFluxDown", t["down"])):
        mean, err = O.batch_statistics(rows[k])
        print(name, k, "z-scores", np.round((mean - want) / np.maximum(err, 1e-30), 2))
        assert np.all(np.abs(mean - want) < 4.5 * err + 1e-6), (k, mean, want, err)


@pytest.mark.parametrize("name", list(LC.EXACT))
def test_few_photons_are_left_out_of_the_exact_comparison(name):
    """The photon-by-photon GPU comparison leaves out the photons the oracle flags (a stop point within 64 x 2^-23 x the path
    length of a face): at most 5 % of them, in every case and for the seed it uses."""
    from oracle import oracle as O
    _, P, src = LC.oracle_setup(name)
    r = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, 0), LC.N_IDS)
    share = float(r["nearFace"].mean())
    print(name, "flagged share %.4f" % share, "runs of clean ids", len(LC.clean_runs(r["nearFace"])))
    assert r["counters"]["badPhotons"] == 0 and share <= 0.05
    assert sum(c for _, c in LC.clean_runs(r["nearFace"])) == LC.N_IDS - int(r["nearFace"].sum())
