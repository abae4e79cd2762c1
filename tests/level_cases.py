"""The small media on which the level fluxes of the product are compared with the oracle's photon by photon
(tests/test_gpu_level_flux_oracle.py), shared with the CPU test that holds the share of photons left out of that comparison
(tests/test_oracle_levels.py).

ONE extinction value everywhere -- there two correct walks cannot amplify the float rounding of a leg's length (DESIGN.md
section 3) -- and everything else unlike from cell to cell: two components with different shares, omega0, the entry of a
multi-entry phase table, and a patchy Lambertian surface with one black patch.  4 x 3 x 5 cells of 0.03-0.05 km at
20 / km: a photon crosses the domain's sides several times before it leaves."""
import numpy as np

from tests import cases

SEED = 20251018
N_IDS = 20000     # photon ids traced per case
EXT = 20.0        # km^-1, everywhere
TABLE = 9001      # points of the inverse phase-function tables, both sides

# (regular spacings are exact binary fractions: the integrator's test for a regular grid compares the spacing with its float)
_AXES = dict(
    regular=(0.03125 * np.arange(5), 0.046875 * np.arange(4), 0.0390625 * np.arange(6)),
    irregular=(np.concatenate([[0.0], np.cumsum([0.03, 0.05, 0.04, 0.035])]), np.concatenate([[0.0], np.cumsum([0.05, 0.03, 0.04])]),
               np.concatenate([[0.0], np.cumsum([0.03, 0.05, 0.035, 0.045, 0.04])])))
GRIDS = {"regular": ("regular", "regular"), "irregular z": ("regular", "irregular"), "irregular x y": ("irregular", "regular"),
         "irregular": ("irregular", "irregular")}


def medium(grid, thermal=False):
    xy, z = GRIDS[grid]
    xe, ye, ze = _AXES[xy][0], _AXES[xy][1], _AXES[z][2]
    shape = (len(xe) - 1, len(ye) - 1, len(ze) - 1)
    rng = np.random.default_rng(11)
    share = rng.uniform(0.2, 0.8, shape)  # of the first component
    comps = [dict(ext=EXT * share, ssa=rng.uniform(0.6, 1.0, shape), pfIndex=rng.integers(1, 4, shape).astype(np.int32),
                  legendre=[cases.hg_legendre(g, 24) for g in (0.85, 0.6, 0.3)]),
             dict(ext=EXT * (1.0 - share), ssa=rng.uniform(0.8, 1.0, shape), pfIndex=rng.integers(1, 3, shape).astype(np.int32),
                  legendre=[np.array([0.0, 0.1], np.float32), cases.hg_legendre(-0.2, 12)])]
    # (thermal: an albedo that is a float.  The product keeps the domain's albedo as float where the reference and the oracle
    # keep real(8): with 0.3 the reflected weight float(w * albedo) differs in its last bit for some w, and the sums of this
    # comparison with it -- DESIGN.md section 3.)
    case = dict(name="levels " + grid, xe=xe, ye=ye, ze=ze, albedo=0.25 if thermal else 0.0, components=comps)
    if thermal:
        case.update(temps=rng.uniform(240.0, 300.0, shape), sfc_temp=295.0, lambda_um=10.0)
        return case
    return cases.patchy_surface(case, nxs=3, nys=2)


# name -> (grid, mu0, phi0 or None for the thermal source, privateTallies, blockSize, roulette)
EXACT = {
    "regular, oblique, flat walk": ("regular", 0.5, 30.0, 0, 256, True),
    "regular, oblique back, nested walk": ("regular", 0.6, 210.0, 2, 512, False),
    "regular, overhead sun": ("regular", 1.0, 0.0, 2, 256, True),
    "irregular z, oblique, nested walk": ("irregular z", 0.5, 30.0, 2, 256, False),
    "irregular z, oblique back, flat walk": ("irregular z", 0.6, 210.0, 0, 512, True),
    "irregular x y, oblique, nested walk": ("irregular x y", 0.5, 30.0, 2, 512, True),
    "irregular x y, oblique back, flat walk": ("irregular x y", 0.6, 210.0, 0, 256, False),
    "irregular, oblique, flat walk": ("irregular", 0.5, 30.0, 0, 512, False),
    "irregular, oblique back, nested walk": ("irregular", 0.6, 210.0, 2, 256, True),
    "irregular, overhead sun": ("irregular", 1.0, 0.0, 0, 256, True),
    "thermal, regular": ("regular", None, None, 0, 256, True),
    "thermal, irregular z": ("irregular z", None, None, 2, 512, True),
}


def oracle_setup(name):
    """(case, oracle problem, oracle source) of an exact-tier case."""
    from oracle import oracle as O
    grid, mu0, phi0, _, _, rr = EXACT[name]
    case = medium(grid, thermal=mu0 is None)
    P = cases.oracle_problem(case, nsteps=TABLE, use_russian_roulette=rr, lw_flag=1.0 if mu0 is None else -1.0)
    if mu0 is None:
        vw, frac, _ = O.emission_weighting(P, case["temps"].transpose(2, 1, 0).reshape(-1), case["lambda_um"], case["sfc_temp"])
        return case, P, O.EmissionSource(vw, frac)
    return case, P, O.solar_source(mu0, phi0)


def clean_runs(near):
    """[(first id, count)] of the maximal runs of unflagged photon ids."""
    clean = np.concatenate([[False], ~np.asarray(near, bool), [False]])
    edges = np.flatnonzero(clean[1:] != clean[:-1])
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


# ---------------------------------------------------------------------------------------------------------------------
# bracket of the product's results from the oracle's sums (the exact tier's tolerance)
# ---------------------------------------------------------------------------------------------------------------------
def tally_ends(s, c, k=0.0):
    """The two ends of what a bin's integer tally times 2^-32 may be, from the oracle's double sum s, its deposit count c and a
    slack sum k (0: none): s -+ (k + c 2^-33 + c 2^-53 s), the lower end not below 0.  product_bracket derives the terms."""
    c = np.asarray(c, np.float64)
    slack = c * 2.0 ** -53 * s
    return np.maximum(s - c * 2.0 ** -33 - slack - k, 0.0), s + c * 2.0 ** -33 + slack + k


def product_bracket(res, xe, ye, n):
    """[lo, hi] for every number reportLevelFluxes() may return for the photons whose oracle sums are `res`
    (oracle.compute_rt_levels): dict name -> (lo, hi), float32, levels [nz + 1, ny, nx] and means [nz + 1].

    The product adds the integer nearest to w 2^32 per deposit (weight_to_fixed: exact for w >= 2^-8, off by at most half a
    unit below) where the oracle adds w: after c deposits into a bin its integer tally R obeys |R 2^-32 - S| <= c 2^-33 for the
    oracle's sum S -- a bracket one 2^-32 per deposit wide.  (S itself is a double sum of c floats in (0, 1]: exact to
    c 2^-53 S, which widens the bracket by that much.)  The epilogue then forms
    (float)((double)R 2^-32) / nppc per bin and the fixed float tree of tests/epilogue_mirror.py over the columns of a level
    for the means: every step is a correctly rounded operation, monotone in its non-negative inputs, so pushing the two
    ends of the tally's bracket through the mirror brackets the floats exactly.  No measured slack."""
    from tests import epilogue_mirror as EM
    g = EM.Grid(xe, ye, [0.0, 1.0])
    nppc = g.photons_per_column(n)
    out = {}
    for name, key in (("levelFluxUp", "levelUp"), ("levelFluxDown", "levelDown")):
        s = res[key]
        nl = s.shape[0]
        ends = []
        for raw in tally_ends(s, res[key + "Count"]):
            ends.append(raw.reshape(nl, -1).astype(np.float32) / nppc[None, :])
        out[name] = tuple(e.reshape(s.shape) for e in ends)
        out["mean" + name[0].upper() + name[1:]] = tuple(EM.tree_mean(e) for e in ends)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# statistical tier: heterogeneous 3-D media, the oracle's MT mode against its Philox mode (CPU) and against the product
# ---------------------------------------------------------------------------------------------------------------------
def stretched_cut():
    """cases.stretched_grid_cloud cut to 8 x 6 x 10, over a patchy surface."""
    return cases.patchy_surface(cases.stretched_grid_cloud(nx=8, ny=6, nz=10), nxs=4, nys=3)


def small_cloud_field():
    """A regular-z cloud field (the `spaced` branch of the walk) of two components, over a grey surface: under the cloud
    layers nothing but the surface's return goes upward, and a bin with a handful of deposits has no Gaussian statistic."""
    return cases.landsat_like(n=16, nz=12, regular=True, albedo=0.3)


STATISTICAL = {"stretched 8 x 6 x 10 over patches": (stretched_cut, 0.5, 30.0), "cloud field 16 x 16 x 12, regular": (small_cloud_field, 0.5, 30.0)}


def _level_worker(args):
    name, mode, seed, proc, first_batch, n_batches, ppb = args
    from oracle import oracle as O
    make, mu0, phi0 = STATISTICAL[name]
    P = cases.oracle_problem(make(), use_russian_roulette=True)
    rng = O.mt_rng([seed, proc, 0]) if mode == "mt" else None
    out = []
    for b in range(first_batch, first_batch + n_batches):
        if mode == "philox":
            rng = O.philox_rng(seed, b * ppb)
        r = O.compute_rt_levels(P, O.solar_source(mu0, phi0), rng, ppb)
        v = O.normalize_levels(P, r["n"], r)
        out.append((ppb, np.concatenate([v["meanLevelFluxUp"], v["meanLevelFluxDown"]]),
                    np.concatenate([v["levelFluxUp"].reshape(-1), v["levelFluxDown"].reshape(-1)])))
    return out


def oracle_level_run(name, mode, n_batches, ppb, seed=10, procs=None):
    """-> {"means": (mean, stderr) of [meanLevelFluxUp | meanLevelFluxDown], "bins": the same of [levelFluxUp | levelFluxDown],
    level slowest, x fastest} from the batch variance, the oracle spread over processes as tests/stats.py does."""
    import multiprocessing as mp
    import os
    from oracle import oracle as O
    O.build()
    procs = procs or max(1, min(8, len(os.sched_getaffinity(0)), n_batches))
    base, extra = divmod(n_batches, procs)
    jobs, lo = [], 0
    for p in range(procs):
        nb = base + (1 if p < extra else 0)
        if nb:
            jobs.append((name, mode, seed, p + 1, lo, nb, ppb))
        lo += nb
    if len(jobs) == 1:
        parts = [_level_worker(jobs[0])]
    else:
        with mp.get_context("spawn").Pool(len(jobs)) as pool:
            parts = pool.map(_level_worker, jobs)
    rows = [r for part in parts for r in part]
    return {"means": O.batch_statistics([(n, m) for n, m, _ in rows]), "bins": O.batch_statistics([(n, b) for n, _, b in rows])}


def assert_level_parity(a, b, label):
    """tests/test_gpu_vs_mt.py's bounds on the N = 2 ncol (nz + 1) level bins and the 2 (nz + 1) means: the means within 4 sigma,
    max |z| < max(4, sqrt(2 ln N) + 1), |mean z| < 0.2."""
    from tests import stats
    zm, zb = stats.z_scores(a["means"], b["means"]), stats.z_scores(a["bins"], b["bins"])
    report = dict(label=label, max_z_means=float(np.abs(zm).max()), max_z_bins=float(np.abs(zb).max()), mean_z_bins=float(zb.mean()),
                  std_z_bins=float(zb.std()), n_bins=int(zb.size))
    print(report)
    assert np.abs(zm).max() < 4.0, report
    assert np.abs(zb).max() < max(4.0, np.sqrt(2.0 * np.log(zb.size)) + 1.0), report
    assert abs(zb.mean()) < 0.2, report
    return report


# ---------------------------------------------------------------------------------------------------------------------
# theory tier: plane-parallel answers at every level (tests/test_analytic.py's solvers)
# ---------------------------------------------------------------------------------------------------------------------
def theory(name):
    """-> dict(case, mu0, phi0 (None: thermal), table, up, down): the flux through every level, bottom up as the level index."""
    from tests import test_analytic as A
    if name == "isotropic layers over albedo 0.5":
        dt = np.asarray(A.LAYERED["dtaus"])
        up, down = A.layered_isotropic_profile(dt, A.LAYERED["omegas"], 0.35, np.concatenate([[0.0], np.cumsum(dt)]), albedo=0.5)
        return dict(case=A.layered_case(0.5), mu0=0.35, phi0=10.0, table=101, up=up[::-1], down=down[::-1])
    if name == "HG g = 0.85, tau = 4, regular z":
        b, omega, g, nleg, node = A.HG_SLABS[2]
        case, chi = A.hg_slab(b, omega, g, nleg, nz=8)
        mu0, up, down = A.doubling_profile(b, omega, A.sampled_moments(chi, table=9001), node, np.linspace(0.0, b, 9), streams=A.HG_STREAMS)
        return dict(case=case, mu0=mu0, phi0=20.0, table=9001, up=up[::-1], down=down[::-1])
    if name == "thermal slab":
        tau, omega, temps, sfc = A.THERMAL_SLABS[1]
        case = A.thermal_case(tau, omega, temps, sfc)[0]
        up, down = A.thermal_profile(tau, omega, A.planck(10.0, np.asarray(temps)[::-1]), float(A.planck(10.0, sfc)),
                                     np.linspace(0.0, tau, len(temps) + 1))
        return dict(case=case, mu0=None, phi0=None, table=101, up=up[::-1], down=down[::-1])
    if name == "homogeneous on a stretched 7 x 5 x 12 grid":
        case = A.homogeneous_3d(3.0, 0.9, 0.6, 48)
        chi = np.concatenate([[1.0], cases.hg_legendre(0.6, 48).astype(np.float64)])
        ze = case["ze"]
        mu0, up, down = A.doubling_profile(3.0, 0.9, A.sampled_moments(chi, table=9001), 40, 3.0 * (1.0 - ze[::-1] / ze[-1]), streams=A.HG_STREAMS)
        return dict(case=case, mu0=mu0, phi0=57.0, table=9001, up=up[::-1], down=down[::-1])
    raise KeyError(name)

