"""The oracle's track-length tally (oracle.compute_rt_actinic: the sum of w l over every piece of path inside a cell, DESIGN.md
section 4.14 restated on the CPU) held to what it must obey before the GPU tests lean on it: closure against the legs' lengths,
the vacuum identities, its own collision estimator, the reference-faithful MT mode against the Philox mode, transport theory,
and -- on the very inputs of tests/test_gpu_actinic_oracle.py's photon-by-photon comparison -- the share of photons that
comparison leaves out."""
import numpy as np
import pytest

from tests import actinic_cases as AC
from tests import cases
from tests import level_cases as LC

SEED = 20241005


def _area_weighted_layer_means(case, act):
    """act [nz, ny, nx] -> [nz]"""
    area = np.diff(case["ye"])[:, None] * np.diff(case["xe"])[None, :]
    return (act * area[None]).sum(axis=(1, 2)) / area.sum()


# closure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["philox", "mt"])
@pytest.mark.parametrize("name", ["regular, oblique, flat walk", "irregular, oblique back, nested walk", "irregular x y, oblique back, flat walk"])
def test_the_cells_add_up_to_the_legs(name, mode):
    """Per batch the raw tally summed over all cells is the sum over photons and legs of w x (leg length), the length taken in the
    scattering loop from the positions before and after the leg (by z, which does not wrap; refined along the axis of the
    largest direction cosine) and not from the walk's steps: both are double sums of the same lengths, 1e-12 relative.  The
    other results are orc_compute_rt_levels' bit for bit, and that entry point's own flag is a subset of this one's."""
    from oracle import oracle as O
    _, P, src = LC.oracle_setup(name)
    n = 10000
    rng = O.mt_rng([SEED, 1, 0]) if mode == "mt" else None
    twin = O.mt_rng([SEED, 1, 0]) if mode == "mt" else None
    for batch in range(3):
        if mode == "philox":
            rng, twin = O.philox_rng(LC.SEED, batch * n), O.philox_rng(LC.SEED, batch * n)
        r = O.compute_rt_actinic(P, src, rng, n)
        old = O.compute_rt_levels(P, src, twin, n)
        for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption", "levelUp", "levelDown", "levelUpCount", "levelDownCount"):
            assert np.array_equal(r[k], old[k]), k
        assert r["counters"] == old["counters"] and r["counters"]["badPhotons"] == 0
        assert not np.any(old["nearFace"] & ~r["nearFace"])
        total = r["actinic"].sum()
        print(name, mode, "batch", batch, "cells / legs - 1 = %.3e" % (total / r["legSum"] - 1.0))
        assert total > 0 and abs(total / r["legSum"] - 1.0) < 1e-12
        # one deposit per full step and one per step cut short by the optical-depth target (every leg that does not leave)
        cut = r["actinicCount"].sum() - r["counters"]["crossings"]
        assert r["counters"]["collisions"] <= cut <= r["counters"]["legs"] and np.all(r["actinic"] > 0)
        assert np.all(r["actinicSlack"] > 0) and np.all(r["actinicSlack"] < 1e-3 * r["actinic"])


# vacuum ----------------------------------------------------------------------------------------------------------------------
def _top_layer_share(P, z_regular):
    """The share of the top layer's depth below a solar launch: the launch lies at the fraction 1 - 2^-23 of the domain's height
    (regular z) or of the top layer's index range (irregular z), not on the top face."""
    ze, nz = P.ze, P.nz
    frac = 1.0 - 2.0 ** -23
    if z_regular:
        z = ze[0] + frac * (ze[-1] - ze[0])
    else:
        t = frac * nz  # (the launch's unit height times the layer count, as the launch forms it)
        z = ze[nz - 1] + (t - np.floor(t)) * (ze[nz] - ze[nz - 1])
    return (z - ze[nz - 1]) / (ze[nz] - ze[nz - 1])


@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_vacuum_under_an_overhead_sun(grid):
    """Every photon crosses every cell of its column once at weight 1: actinicFlux = fluxDown in every cell to double rounding,
    the top layer by the share of its depth that lies below the launch."""
    from oracle import oracle as O
    case = AC.vacuum_on(grid)
    P = cases.oracle_problem(case, nsteps=2001)
    n = 6000
    r = O.compute_rt_actinic(P, O.solar_source(1.0, 0.0), O.philox_rng(LC.SEED, 0), n)
    act = O.normalize_actinic(P, r["n"], r)["actinicFlux"]
    down = r["levelDown"][0] / O._nppc(P, n)  # (fluxDown's deposits, summed in double)
    assert r["counters"]["badPhotons"] == 0 and np.all(down > 0) and not r["nearFace"].any()
    share = np.ones(P.nz)
    share[-1] = _top_layer_share(P, LC.GRIDS[grid][1] == "regular")
    rel = np.abs(act / (down[None] * share[:, None, None]) - 1.0)
    print(grid, "worst relative difference of actinicFlux from fluxDown %.3e (top layer: 1 - %.3e of its depth)" % (rel.max(), 1.0 - share[-1]))
    assert rel.max() < 1e-12 and 0.0 < 1.0 - share[-1] < 1e-5


def test_vacuum_under_an_oblique_sun():
    """mu0 = 0.5, phi0 = 30 degrees on the irregular grid: every photon crosses every layer with the path dz / mu0 whichever
    columns it passes, so the area-weighted layer mean of actinicFlux times mu0 is 1 to 1e-12 (the top layer: the share of its depth
    below the launch)."""
    from oracle import oracle as O
    case = AC.vacuum_on("irregular")
    P = cases.oracle_problem(case, nsteps=2001)
    for mode, rng in (("philox", O.philox_rng(LC.SEED, 0)), ("mt", O.mt_rng(SEED))):
        r = O.compute_rt_actinic(P, O.solar_source(0.5, 30.0), rng, 6000)
        assert r["counters"]["badPhotons"] == 0
        nppc_area = 6000.0 * (np.diff(P.ye)[:, None] * np.diff(P.xe)[None, :]) / ((P.xe[-1] - P.xe[0]) * (P.ye[-1] - P.ye[0]))
        act = r["actinic"] / (nppc_area[None] * np.diff(P.ze)[:, None, None])  # (photons per column by area in double, not its float)
        means = _area_weighted_layer_means(case, act)
        mu0 = float(np.float32(0.5))
        print(mode, "area-weighted layer means * mu0 - 1:", means * mu0 - 1.0)
        share = np.ones(P.nz)
        share[-1] = _top_layer_share(P, False)
        assert np.abs(means * mu0 / share - 1.0).max() < 1e-12


# track length against collisions -----------------------------------------------------------------------------------------------
def _collision_run(case, mu0, phi0, n_batches, ppb):
    """What tests.test_gpu_actinic._assert_track_length_against_collisions reads, from the oracle: statistics of
    absorbedVolume, actinicFlux and absorbedProfile over the batches and the per-batch actinicFlux, x-first as the product's."""
    from oracle import oracle as O
    P = cases.oracle_problem(case, nsteps=LC.TABLE, use_russian_roulette=True)
    rows = {"absorbedVolume": [], "actinicFlux": [], "absorbedProfile": []}
    reports = []
    for b in range(n_batches):
        r = O.compute_rt_actinic(P, O.solar_source(mu0, phi0), O.philox_rng(SEED, b * ppb), ppb)
        assert r["counters"]["badPhotons"] == 0
        vol = O.normalize(P, r["n"], r)["volumeAbsorption"].reshape(P.nz, P.ny, P.nx).astype(np.float64).transpose(2, 1, 0)
        act = O.normalize_actinic(P, r["n"], r)["actinicFlux"].transpose(2, 1, 0)
        rows["absorbedVolume"].append((ppb, vol)); rows["actinicFlux"].append((ppb, act)); rows["absorbedProfile"].append((ppb, vol.mean(axis=(0, 1))))
        reports.append(dict(actinicFlux=act))
    st = dict(batches=n_batches)
    for k, v in rows.items():
        st[k], st[k + "_StdErr"] = O.batch_statistics(v)
    return dict(stats=st, reports=reports)


@pytest.mark.parametrize("grid", list(LC.GRIDS) + ["stretched cut"])
def test_track_length_against_the_oracles_own_collisions(grid):
    """volumeAbsorption (the collision estimator the oracle restates from the reference) against sigma_abs actinicFlux / 1000 in
    every absorbing cell and layer by layer, with the bounds of tests/test_gpu_actinic.py: 4 x 10^5 photons in 40 batches."""
    from tests.test_gpu_actinic import _assert_track_length_against_collisions
    case = LC.stretched_cut() if grid == "stretched cut" else LC.medium(grid)
    _assert_track_length_against_collisions(case, _collision_run(case, 0.5, 30.0, 40, 10000), "oracle, " + grid)


# the two generator modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.STATISTICAL))
def test_philox_mode_agrees_with_mt_mode_cell_by_cell(name):
    """level_cases.assert_level_parity's bounds on every cell and every layer mean, 100 batches of 10^4 photons on either side
    (100: with fewer the z-scores of thousands of bins are Student's t with tails the bound for a normal sample does not hold)."""
    a = AC.oracle_actinic_run(name, "philox", 100, 10000, seed=10, procs=8)  # (the MT streams are per process: a fixed number)
    b = AC.oracle_actinic_run(name, "mt", 100, 10000, seed=10, procs=8)
    LC.assert_level_parity(a, b, "actinic, " + name)


# theory ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.SOLAR_THEORY)
def test_oracle_actinic_flux_against_theory(name):
    """meanActinicFlux at every absorbing layer against (net flux in - net flux out) / ((1 - omega) dtau) of the deterministic
    profiles, and on the stretched grid every cell against its layer's value: 4.5 standard errors (25 batches of 10^4 photons)
    plus the floor 4e-6 / ((1 - omega) dtau)."""
    from oracle import oracle as O
    t = AC.actinic_theory(name)
    P = cases.oracle_problem(t["case"], nsteps=t["table"])
    per, nb = 10000, 25
    means, cells = [], []
    for b in range(nb):
        r = O.compute_rt_actinic(P, O.solar_source(t["mu0"], t["phi0"]), O.philox_rng(SEED, b * per), per)
        assert r["counters"]["badPhotons"] == 0
        v = O.normalize_actinic(P, r["n"], r)
        means.append((per, v["meanActinicFlux"])); cells.append((per, v["actinicFlux"]))
    k = t["layers"]
    assert k.sum() >= 6
    mean, err = O.batch_statistics(means)
    print(name, "meanActinicFlux z-scores", np.round(((mean - t["actinic"]) / np.maximum(err, 1e-30))[k], 2))
    assert np.all(np.abs(mean - t["actinic"])[k] < (4.5 * err + t["floor"])[k]), (mean, t["actinic"], err)
    if name.startswith("homogeneous on a stretched"):
        cell, cerr = O.batch_statistics(cells)
        z = (cell - t["actinic"][:, None, None]) / np.maximum(cerr, 1e-30)
        print(name, "actinicFlux per cell: max |z| %.2f, mean z %.3f over %d cells" % (np.abs(z[k]).max(), z[k].mean(), z[k].size))
        assert np.all(cerr[k] > 0) and np.all(np.abs(cell - t["actinic"][:, None, None])[k] < (4.5 * cerr + t["floor"][:, None, None])[k])


# the share left out ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.SOLAR_EXACT)
def test_few_photons_are_left_out_of_the_exact_comparison(name):
    """The photon-by-photon GPU comparison leaves out the photons the oracle flags -- a stop point within
    delta = 64 x 2^-23 x the path length of a face, or a step whose cell has two faces within delta of each other along the leg (an
    edge or a corner) -- at most 5 % of them, in every case and for the seed it uses."""
    from oracle import oracle as O
    _, P, src = LC.oracle_setup(name)
    r = O.compute_rt_actinic(P, src, O.philox_rng(LC.SEED, 0), LC.N_IDS)
    old = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, 0), LC.N_IDS)["nearFace"]
    share, runs = float(r["nearFace"].mean()), LC.clean_runs(r["nearFace"])
    print(name, "flagged share %.4f (stop points alone %.4f)" % (share, old.mean()), "runs of clean ids", len(runs), "calls of at most",
          AC.MAX_IDS, "ids:", len(AC.split_runs(runs)))
    assert r["counters"]["badPhotons"] == 0 and share <= 0.05
    assert sum(c for _, c in runs) == LC.N_IDS - int(r["nearFace"].sum())
    calls = AC.split_runs(runs)
    assert sum(c for _, c in calls) == LC.N_IDS - int(r["nearFace"].sum()) and max(c for _, c in calls) <= AC.MAX_IDS
    assert not any(r["nearFace"][f:f + c].any() for f, c in calls)
