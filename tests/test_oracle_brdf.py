"""The oracle's surface BRDFs (oracle.compute_rt_brdf, oracle/mcbrat_oracle.c: RPV, Ross-Li and Cox-Munk with its glint sampler,
DESIGN.md sections 4.11 and 4.11.1 restated on the CPU in plain C) held to what they must obey before the GPU tests lean on them:

* R against the numpy statements of the models (tests/brdf_ref.py, tests/coxmunk_ref.py), the sampler against the library's host
  compile of its own (mcbrat_brdf_sample) -- here the oracle is the reference;
* kind 0 and the Lambertian limits of kinds 1-3 against today's surface description, array-equal; the bookkeeping of the double
  sums, the counts, the slack and the photons' energy;
* on the very rows of tests/test_gpu_brdf_oracle.py's photon-by-photon comparison: the share of photons it leaves out, that the
  rows reach what they are there for (weights above 1, photons ended by R = 0, both components of the glint mixture), and
  delta_0, from which the bracket's delta is taken;
* the reference-faithful MT mode against the Philox mode on the statistical tier's case."""
import numpy as np
import pytest

from tests import brdf_cases as BC
from tests import brdf_ref as B
from tests import cases
from tests import coxmunk_ref as CM
from tests import level_cases as LC

SEED = 20260117
N_PAIRS = 100000


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


def _pairs(n, seed):
    """n pairs (d_in, d_out): random, a share with cosines below the 0.01 clamp on either side, the hot spot's neighbourhood,
    and exact backscatter (d_out = -d_in)."""
    rng = np.random.default_rng(seed)
    mi, mr = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    pi_, pr = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, 2.0 * np.pi, n)
    k = n // 10
    mi[:k] = rng.uniform(1e-6, 0.01, k)            # below the clamp, arriving
    mr[k:2 * k] = rng.uniform(2.0 ** -16, 0.01, k)  # ... leaving
    mr[2 * k:3 * k] = mi[2 * k:3 * k] * (1.0 + rng.uniform(-1e-3, 1e-3, k))  # around the hot spot
    pr[2 * k:3 * k] = pi_[2 * k:3 * k] + np.pi + rng.uniform(-1e-3, 1e-3, k)
    d_in, d_out = B.direction(-mi, pi_), B.direction(mr, pr)
    d_out[3 * k:4 * k] = -d_in[3 * k:4 * k]         # exact backscatter
    d_in[4 * k:4 * k + 8] = B.direction(-1.0, 0.0)  # straight down, and straight back up
    d_out[4 * k:4 * k + 4] = B.direction(1.0, 0.0)
    return d_in, d_out


def _patches(model):
    return [tuple(q) for row in BC.SURFACES[model] for q in row]


@pytest.mark.parametrize("model", ["RPV", "RossLi", "CoxMunk"])
def test_reflectance_matches_the_python_statements(O, model):
    """10^5 pairs of directions per model, spread over the parameter vectors of the rows' patches: both sides are double evaluations
    of one formula, so relative 1e-10 (absolute below R = 1e-12)."""
    d_in, d_out = _pairs(N_PAIRS, SEED)
    kind = O.BRDF_KINDS[model]
    qs = _patches(model)
    worst_rel, worst_abs, zeros, above = 0.0, 0.0, 0, 0
    for i, q in enumerate(qs):
        sl = slice(i * N_PAIRS // len(qs), (i + 1) * N_PAIRS // len(qs))
        q32 = np.asarray(q, np.float32)
        want = CM.reflectance(q32, d_in[sl], d_out[sl]) if model == "CoxMunk" else B.reflectance(kind, q32.astype(np.float64), d_in[sl], d_out[sl])
        got = O.brdf_reflectance(kind, q32, d_in[sl], d_out[sl])
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        small = want < 1e-12
        if small.any():
            worst_abs = max(worst_abs, float(np.abs(got - want)[small].max()))
        if (~small).any():
            worst_rel = max(worst_rel, float((np.abs(got - want)[~small] / want[~small]).max()))
        zeros, above = zeros + int((got == 0.0).sum()), above + int((got > 1.0).sum())
    print("%s: worst relative difference %.3e, worst absolute below 1e-12 %.3e; R = 0 at %d pairs, R > 1 at %d" % (model, worst_rel, worst_abs, zeros, above))
    assert worst_rel <= 1e-10 and worst_abs <= 1e-12


def test_lambertian_limits_are_exact(O):
    """RPV (a, 1, 0, 1), Ross-Li (a, 0, 0) and Cox-Munk (U, 1, 0, a) return the float a exactly, whatever the directions."""
    d_in, d_out = _pairs(2000, SEED + 1)
    for a in (np.float32(0.3), np.float32(0.05), np.float32(0.9), np.float32(0.0)):
        for model in ("RPV", "RossLi", "CoxMunk"):
            got = O.brdf_reflectance(O.BRDF_KINDS[model], BC.LAMBERTIAN_LIMITS[model](float(a)), d_in, d_out)
            assert np.all(got == np.float64(a)), (model, a)


def test_sampler_against_the_library(O):
    """The library's host compile of its reflection (mcbrat_brdf_sample) against the oracle's on the same uniforms: directions to
    1e-12, the factor to one float ulp, and the same photons ended -- except where the oracle's own flag marks the draw as a tie
    (the component, or the end of the photon, changes when a direction component moves by delta)."""
    from mcbrat3d_amd import surface as S
    rng = np.random.default_rng(SEED + 2)
    n, glint, lambert, dead, ties = 4000, 0, 0, 0, 0
    for q in _patches("CoxMunk") + [(2.0, 1.34, 0.0, 0.0), (15.0, 1.34, 0.22, 0.0)]:
        for mu0 in (1.0, 0.6, 0.2, 0.03):
            d_in = CM.direction(-mu0, rng.uniform(0.0, 2.0 * np.pi))
            if mu0 in (0.6, 0.03):  # as the kernels hand it over: floats, a unit vector to 2^-24 only (both sides scale the mirror direction to length 1)
                d_in = d_in.astype(np.float32).astype(np.float64)
            u = rng.uniform(size=(n, 3))
            u[:8, 0] = (0.0, 1.0, 0.0, 1.0, 0.5, 0.5, 0.0, 1.0)  # the ends of the uniforms' closed interval
            u[:8, 1] = (0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.5, 0.5)
            d_lib, w_lib = S.brdf_sample(3, np.asarray(q, np.float32), d_in, u)
            r = O.brdf_reflect(3, q, d_in, u, delta=BC.DELTA)
            f32 = r["factor"].astype(np.float32)
            ok = ~r["tie"]
            assert np.array_equal((w_lib > 0)[ok], (f32 > 0)[ok]), (q, mu0)
            live = ok & (f32 > 0)
            assert np.abs(d_lib - r["d_out"])[live].max() <= 1e-12, (q, mu0)
            assert np.all(np.abs(w_lib - f32)[live] <= np.spacing(f32[live])), (q, mu0)
            assert np.all(w_lib[ok & (f32 == 0)] == 0)
            glint, lambert = glint + int((r["comp"] & 1).sum()), lambert + int(((r["comp"] & 1) == 0).sum())
            dead, ties = dead + int((r["comp"] >> 1).sum()), ties + int(r["tie"].sum())
    print("sampler: %d glint draws, %d Lambertian draws, %d ended by the sampled direction, %d ties" % (glint, lambert, dead, ties))
    assert glint > 10000 and lambert > 10000 and dead > 0
    # the land models keep the Lambertian draw and multiply by R
    for model in ("RPV", "RossLi"):
        q, d_in, u = _patches(model)[0], CM.direction(-0.4, 2.0), rng.uniform(size=(500, 3))
        d_lib, w_lib = S.brdf_sample(O.BRDF_KINDS[model], np.asarray(q, np.float32), d_in, u)
        r = O.brdf_reflect(O.BRDF_KINDS[model], q, d_in, u)
        f32 = r["factor"].astype(np.float32)
        assert np.abs(d_lib - r["d_out"]).max() <= 1e-12 and np.all(np.abs(w_lib - f32) <= np.spacing(np.maximum(f32, np.float32(1e-30))))


@pytest.mark.parametrize("model", ["Lambertian", "RPV", "RossLi", "CoxMunk"])
@pytest.mark.parametrize("mode", ["philox", "mt"])
def test_kind_0_and_the_lambertian_limits_follow_the_surface_description(O, model, mode):
    """Kind 0 through the new entry, and kinds 1-3 at their Lambertian limits, against orc_compute_rt on today's surface
    description: fates, float tallies and counters array-equal, in both generator modes; radiance too (w R / pi against
    (w a) / pi: to 1e-6, as the product's)."""
    case = cases.patchy_surface(BC.medium("irregular"), nxs=3, nys=2)  # (reflectances 0 .. 0.9, one patch black)
    refl, x, y = case["surface"]
    P0 = cases.oracle_problem(case, nsteps=LC.TABLE)
    if model == "Lambertian":
        new = dict(case, surface_brdf=("Lambertian", np.asarray(refl, np.float32)[None], x, y))
        new.pop("surface")
    else:
        new = BC.lambertian_limit(case, model, refl, x, y)
    P1 = cases.oracle_problem(new, nsteps=LC.TABLE)
    assert P1.c.surfKind == O.BRDF_KINDS[model]
    n = 6000
    rng = (lambda: O.philox_rng(LC.SEED, 123)) if mode == "philox" else (lambda: O.mt_rng([7, 1, 0]))
    src = O.solar_source(0.6, 210.0)
    a = O.compute_rt(P0, src, rng(), n, want_fates=True)
    b = O.compute_rt_brdf(P1, src, rng(), n, want_fates=True, delta=BC.DELTA)
    assert np.array_equal(a["fates"], b["fates"]) and a["counters"] == b["counters"] and a["counters"]["surfaceHits"] > n // 4
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption"):
        assert np.array_equal(a[k], b["float"][k]), k
    assert b["aboveOne"] == 0 and b["ties"] == 0 and b["endedByZero"] == a["counters"]["surfaceAbsorbed"] * (model != "Lambertian")
    inten = cases.oracle_intensity(case, BC.VIEWS[0], BC.VIEWS[1], n_angles=BC.FWD_ANGLES)
    ia = O.compute_rt_intensity(P0, src, rng(), n, inten)["intensity"]
    ib = O.compute_rt_brdf(P1, src, rng(), n, intensity=inten)["intensity"]
    assert ia.sum() > 0 and np.allclose(ia, ib, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("name", ["RPV, regular, oblique, global atomics 256, orders", "Ross-Li, irregular, overhead, wide plan",
                                  "Cox-Munk sampled, irregular, oblique back, kernel PRIV 2 at 512 lanes"])
def test_bookkeeping(O, name):
    """The double sums are the float tallies' deposits (equal to the float sum's rounding, (deposits) x 2^-24 x the sum, the line
    of tests/test_oracle_levels.py; the volume tally by that file's bound for it), the orders add up to no more than the whole,
    the float results do not notice the new tallies, every photon's energy closes, and with delta = 0 the slack is the 2^-23
    terms alone: of a single photon's exit, a whole number of them, one per reflection since the weight was last exactly 1."""
    case, P, src, _ = BC.oracle_setup(name)
    orders = BC.EXACT[name][8]
    n = 10000
    r = O.compute_rt_brdf(P, src, O.philox_rng(LC.SEED, 0), n, orders=orders, delta=BC.DELTA, want_fates=True)
    z = O.compute_rt_brdf(P, src, O.philox_rng(LC.SEED, 0), n, orders=orders, delta=0.0, want_fates=True)
    assert r["counters"]["badPhotons"] == 0 and np.array_equal(r["fates"], z["fates"])
    for k in ("fluxUp", "fluxDown"):
        s, c, f = r[k].reshape(-1), r[k + "Count"].reshape(-1), r["float"][k]
        assert s.sum() > 0 and np.all(np.abs(s - f) <= c * 2.0 ** -24 * s), k
        assert np.array_equal(r[k], z[k]) and np.all(z[k + "Slack"] <= r[k + "Slack"])
    vol, fvol = r["volumeAbsorption"].reshape(-1), r["float"]["volumeAbsorption"].astype(np.float64)
    assert np.abs(vol - fvol).max() <= r["counters"]["collisions"] * 2.0 ** -24 * (1.0 + np.abs(fvol).max())
    assert np.allclose(r["fluxAbsorbed"].reshape(-1), r["float"]["fluxAbsorbed"], rtol=1e-5)
    assert r["fluxUpCount"].sum() == r["counters"]["topExits"] and r["fluxDownCount"].sum() == r["counters"]["surfaceHits"]
    assert r["volumeAbsorptionCount"].sum() == r["counters"]["absorbEvents"]
    if orders:
        for k in ("fluxUp", "fluxDown"):
            assert np.all(r[k + "ByOrd"].sum(axis=0) <= r[k] * (1.0 + 1e-12)) and np.all(r[k + "ByOrdCount"].sum(axis=0) <= r[k + "Count"])
        assert r["fluxDownByOrdCount"][0].sum() > 0 and r["fluxUpByOrdCount"][0].sum() == 0  # (nothing leaves the top unscattered)
    ok = r["fates"]["fate"] != 3
    assert np.all(np.abs(r["closure"])[ok] <= r["closureBound"][ok]) and r["closureBound"].max() < 1e-4
    # delta = 0: the slack of every bin is at most (reflections of the longest history) x 2^-23 x the bin's sum, and positive
    most = int(r["fates"]["nScatter"].max())
    for k in ("fluxUp", "fluxDown", "volumeAbsorption"):
        assert np.all(z[k + "Slack"] <= most * 2.0 ** -23 * z[k] * (1.0 + 1e-12)) and z[k + "Slack"].sum() > 0
    whole = 0
    for first in range(40000, 40300):  # single photons
        one = O.compute_rt_brdf(P, src, O.philox_rng(LC.SEED, first), 1, delta=0.0)
        if one["fluxUp"].sum() > 0:
            m = one["fluxUpSlack"].sum() / (one["fluxUp"].sum() * 2.0 ** -23)
            assert abs(m - round(m)) < 1e-6 and 0 <= round(m) <= one["counters"]["surfaceHits"], (first, m)
            whole += round(m) > 0
    assert whole > 20


@pytest.fixture(scope="module")
def rows(O):
    """Every exact-tier row once over its N_IDS ids, with the arrivals; shared by the tests below, left unchanged."""
    return {name: BC.oracle_run(name, 0, BC.N_IDS, want_fates=True, arrivals=True) for name in BC.EXACT}


@pytest.mark.parametrize("name", list(BC.EXACT))
def test_few_photons_are_left_out_of_the_exact_comparison(rows, name):
    """At most 5 % of the ids flagged (the bound of tests/test_oracle_levels.py), none dropped; the clean runs cover the rest."""
    r = rows[name]
    share = float(r["nearFace"].mean())
    print(name, "flagged share %.4f (ties among them: %d)" % (share, r["ties"]), "runs of clean ids", len(LC.clean_runs(r["nearFace"])),
          "reflections", r["reflections"], "weights above 1:", r["aboveOne"], "ended by R = 0:", r["endedByZero"],
          "glint / Lambertian draws", r["glintTaken"], r["lambertTaken"])
    assert r["counters"]["badPhotons"] == 0 and share <= 0.05
    assert sum(c for _, c in LC.clean_runs(r["nearFace"])) == BC.N_IDS - int(r["nearFace"].sum())
    if name.startswith("Cox-Munk sampled"):
        assert r["glintTaken"] >= 500 and r["lambertTaken"] >= 500


def test_the_rows_reach_what_they_are_there_for(rows):
    """Conditions on the inputs: over the RPV rows at least 100 reflected weights above 1, over the Ross-Li rows at least 20 photons
    ended by R = 0; both grids, three suns, and every model on at least two plans."""
    above = sum(r["aboveOne"] for n, r in rows.items() if n.startswith("RPV"))
    ended = sum(r["endedByZero"] for n, r in rows.items() if n.startswith("Ross-Li"))
    print("RPV rows: %d reflected weights above 1; Ross-Li rows: %d photons ended by R = 0" % (above, ended))
    assert above >= 100 and ended >= 20
    assert {v[0] for v in BC.EXACT.values()} == {"regular", "irregular"} and len({v[1:3] for v in BC.EXACT.values()}) == 3
    for model in ("RPV", "RossLi", "CoxMunk"):
        assert len({str(sorted(v[5].items())) + str(v[6]) for v in BC.EXACT.values() if v[3] == model}) >= 2
    assert sum(1 for v in BC.EXACT.values() if v[8]) == 2 and sum(1 for v in BC.EXACT.values() if v[9]) == 2
    # every plan named for the rows is there: setTuning's values (1: kernel PRIV 2 where the grid fits the LDS; 2: kernel PRIV 1)
    plans = [(v[5], v[6]) for v in BC.EXACT.values()]

    def has(layer_skip=None, **want):
        return any(all(t.get(k) == x for k, x in want.items()) and (layer_skip is None or ls == layer_skip) for t, ls in plans)
    assert has(privateTallies=0, brickLayout=0, blockSize=256) and has(brickLayout=1) and has(privateTallies=1)
    assert has(privateTallies=1, blockSize=512) and has(privateTallies=2) and has(privateTallies=4) and has(layer_skip=1)
    assert any(t == {} for t, _ in plans)  # the library's own choice
    for name in BC.EXACT:
        assert ("kernel PRIV 2" in name) == (BC.EXACT[name][5].get("privateTallies") == 1), name
        assert ("kernel PRIV 1" in name) == (BC.EXACT[name][5].get("privateTallies") == 2), name


def test_delta_0(O, rows):
    """delta_0: the largest componentwise difference of the arriving direction at a surface arrival between the oracle's plain run
    and its run with the direction carried through scatterings in double, over the ids that are clean and have the same fate in
    both, on every exact-tier row.  The bracket's delta is max(4 delta_0, 2^-22): brdf_cases.DELTA must not be below it."""
    d0, arrivals = 0.0, 0
    for name, a in rows.items():
        b = BC.oracle_run(name, 0, BC.N_IDS, want_fates=True, arrivals=True, double_directions=True)
        fa, fb = a["fates"], b["fates"]
        same = ~a["nearFace"] & ~b["nearFace"]
        for f in ("fate", "ix", "iy", "iz", "nScatter"):
            same &= fa[f] == fb[f]
        same &= np.bincount(a["arrivalPhoton"], minlength=BC.N_IDS) == np.bincount(b["arrivalPhoton"], minlength=BC.N_IDS)
        assert same.mean() > 0.98, (name, same.mean())
        da, db = a["arrivalDir"][same[a["arrivalPhoton"]]], b["arrivalDir"][same[b["arrivalPhoton"]]]
        assert da.shape == db.shape and da.shape[0] > 5000
        d0, arrivals = max(d0, float(np.abs(da - db).max())), arrivals + da.shape[0]
    print("delta_0 = %.4e over %d surface arrivals; 4 delta_0 = %.4e, delta = %.4e" % (d0, arrivals, 4.0 * d0, BC.DELTA))
    assert 2.0 ** -24 < d0 and max(4.0 * d0, 2.0 ** -22) <= BC.DELTA


def test_bracket_of_an_oracle_run_holds_its_own_floats(O):
    """brdf_bracket on the oracle's own sums: the floats that its float tallies normalise to lie inside (the float tallies round
    every addition, the bracket's ends do not: checked to the tallies' rounding), lo <= hi everywhere, and a bin without deposits
    has the bracket [0, 0]."""
    name = "RPV, regular, oblique, global atomics 256, orders"
    case, P, src, _ = BC.oracle_setup(name)
    r = BC.oracle_run(name, 0, 128)
    br = BC.brdf_bracket(r, case["xe"], case["ye"], case["ze"], 128)
    norm = O.normalize(P, 128, r["float"])
    for k, count in BC.COUNTS.items():
        lo, hi = br[k]
        assert np.all(lo <= hi) and np.all(hi[r[count] == 0] == 0), k
    for k in ("fluxUp", "fluxDown"):
        lo, hi = br[k]
        v = norm[k].reshape(lo.shape)
        assert np.all(v >= lo * (1.0 - 2.0 ** -20)) and np.all(v <= hi * (1.0 + 2.0 ** -20)), k
    assert br["meanFluxUp"][0] > 0.1 and (br["meanFluxUp"][1] - br["meanFluxUp"][0]) < 1e-4 * br["meanFluxUp"][1]


@pytest.mark.parametrize("model", BC.STATISTICAL)
def test_philox_mode_agrees_with_mt_mode(model):
    """The oracle's reference-faithful MT mode against its Philox mode on the statistical tier's case (fluxes and radiance per
    column, intensity roulette on), with level_cases.assert_level_parity's bounds.  10^6 photons a side in 100 batches, the MT
    sample of the GPU tier: at 30 batches Cox-Munk's absorbed mean stood at 4.1 standard errors of that sample's own estimate, at
    100 batches (two seeds) at 2.1 and 2.5 -- a bias would have grown with the square root of the sample, not shrunk."""
    a = BC.oracle_stat_run(model, "philox", 100, 10000, seed=10)
    b = BC.oracle_stat_run(model, "mt", 100, 10000, seed=10)
    LC.assert_level_parity(a, b, "BRDF " + model)
