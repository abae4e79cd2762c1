"""The small medium, the surfaces and the rows on which the BRDF kernels are held to the oracle's BRDF entry photon by photon
(oracle.compute_rt_brdf, DESIGN.md sections 3 and 4.11), shared by tests/test_oracle_brdf.py (CPU: the conditions on these inputs,
delta_0) and tests/test_gpu_brdf_oracle.py.

The medium is level_cases.medium's construction, thinner and brighter so that reflections dominate: ONE extinction value
everywhere (5 / km), omega0 from 0.9-1 and 0.95-1, 4 x 3 x 5 cells, over 3 x 2 surface patches on positions of their own, every
patch with parameters of its own."""
import numpy as np

from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC

EXT = 5.0              # km^-1, everywhere
N_IDS = LC.N_IDS       # photon ids traced per row
ORDERS = 3             # scattering orders 0, 1, 2 on the rows that record them
VIEWS = ([1.0, 0.5, 0.3], [0.0, 200.0, 75.0])  # the three views of the rows with radiance: mus, phis (degrees)
FWD_ANGLES = 1801

# delta, the move of one direction component in the bracket of R: max(4 delta_0, 2^-22).  delta_0 -- the
# largest componentwise difference of the arriving direction at a surface arrival between the oracle's float run and its run with
# the direction carried in double -- is measured by tests/test_oracle_brdf.py on every row below, which asserts 4 delta_0 <= DELTA;
# as measured there it is 1.1105e-6 (DELTA_0_MEASURED).  The product is never consulted for it.
DELTA_0_MEASURED = 1.1105e-6
DELTA = 4.5e-6


def medium(grid):
    xy, z = LC.GRIDS[grid]
    xe, ye, ze = LC._AXES[xy][0], LC._AXES[xy][1], LC._AXES[z][2]
    shape = (len(xe) - 1, len(ye) - 1, len(ze) - 1)
    rng = np.random.default_rng(11)
    share = rng.uniform(0.2, 0.8, shape)  # of the first component
    comps = [dict(ext=EXT * share, ssa=rng.uniform(0.9, 1.0, shape), pfIndex=rng.integers(1, 4, shape).astype(np.int32),
                  legendre=[cases.hg_legendre(g, 24) for g in (0.85, 0.6, 0.3)]),
             dict(ext=EXT * (1.0 - share), ssa=rng.uniform(0.95, 1.0, shape), pfIndex=rng.integers(1, 3, shape).astype(np.int32),
                  legendre=[np.array([0.0, 0.1], np.float32), cases.hg_legendre(-0.2, 12)])]
    return dict(name="brdf " + grid, xe=xe, ye=ye, ze=ze, albedo=0.0, components=comps)


def patch_positions(case, nxs, nys):
    """cases.patchy_surface's positions: nxs x nys patches that span the domain, on edges of their own."""
    _, x, y = cases.patchy_surface(case, nxs=nxs, nys=nys)["surface"]
    return x, y


# parameters per patch, [ix][iy] over 3 x 2 patches
_RPV = [[(0.30, 0.70, -0.10, 0.30), (0.25, 1.30, 0.15, 0.60)],    # vegetation; k > 1 and Theta > 0
        [(0.00, 0.80, -0.05, 0.50), (0.30, 0.72, -0.12, 0.30)],   # a black patch (rho0 = 0)
        [(0.28, 0.75, -0.08, 0.35), (0.27, 0.68, -0.10, 1.00)]]
_ROSSLI = [[(0.30, 0.15, 0.05), (0.25, 0.00, 0.00)],               # ... fIso alone
           [(0.35, 0.20, 0.06), (0.28, 0.10, 0.08)],
           [(0.20, 0.25, 0.04), (0.32, 0.12, 0.07)]]
_COXMUNK = [[(1.0, 1.34, 0.00, 0.00), (5.0, 1.00, 0.00, 0.05)],    # calm; n = 1 (the Lambertian limit a_w)
            [(10.0, 1.34, 0.22, 0.02), (3.0, 1.34, 0.00, 0.05)],   # whitecaps
            [(7.0, 1.34, 0.00, 0.03), (2.0, 1.34, 0.00, 0.01)]]
SURFACES = {"RPV": _RPV, "RossLi": _ROSSLI, "CoxMunk": _COXMUNK}
LAMBERTIAN_LIMITS = {"RPV": lambda a: (a, 1.0, 0.0, 1.0), "RossLi": lambda a: (a, 0.0, 0.0), "CoxMunk": lambda a: (4.0, 1.0, 0.0, a)}


def with_surface(case, model, table=None, glint=True):
    """A copy of the case over the patches of `model` (table: parameters [nxs][nys], default SURFACES[model])."""
    q = np.asarray(SURFACES[model] if table is None else table, np.float32)  # [ix, iy, p]
    x, y = patch_positions(case, q.shape[0], q.shape[1])
    out = dict(case)
    out["surface_brdf"] = (model, np.ascontiguousarray(q.transpose(2, 0, 1)), x, y)
    out["glint_sampling"] = bool(glint)
    return out


def lambertian_limit(case, model, refl, x, y):
    """The case over the surface `model` in its Lambertian limit of the reflectances refl[ix, iy] on positions x, y."""
    refl = np.asarray(refl, np.float32)
    q = np.array([[LAMBERTIAN_LIMITS[model](float(a)) for a in row] for row in refl], np.float32)
    out = dict(case)
    out.pop("surface", None)
    out["surface_brdf"] = (model, np.ascontiguousarray(q.transpose(2, 0, 1)), x, y)
    return out


# setTuning(privateTallies=) and the kernel it selects (include/mcbrat.h, pick_trace in mcbrat_variants.h):
# 1 = tallies private to a workgroup AND, where the optical grid fits (this medium does), the grid in LDS: kernel PRIV 2;
# 2 = private tallies without the grid in LDS: kernel PRIV 1; 4 = the wide plan, one workgroup of 1024 lanes per compute unit.
# name -> (grid, mu0, phi0, model, glint sampling, tuning, layerSkip, roulette, orders, views)
GLOBAL_256 = dict(privateTallies=0, brickLayout=0, blockSize=256)
GLOBAL_512 = dict(privateTallies=0, brickLayout=0, blockSize=512)
BRICKS = dict(privateTallies=0, brickLayout=1, blockSize=256)
GRID_LDS_256 = dict(privateTallies=1, brickLayout=0, blockSize=256)      # kernel PRIV 2, 256 lanes
GRID_LDS_512 = dict(privateTallies=1, brickLayout=0, blockSize=512)      # kernel PRIV 2, 512 lanes
TALLIES_LDS_256 = dict(privateTallies=2, brickLayout=0, blockSize=256)   # kernel PRIV 1, 256 lanes
TALLIES_LDS_512 = dict(privateTallies=2, brickLayout=0, blockSize=512)   # kernel PRIV 1, 512 lanes
OWN_CHOICE = dict()                                             # the library's own plan with blockWalk = 0: the 768-lane kernel
WIDE = dict(privateTallies=4, blockSize=0, brickLayout=0)      # the wide plan: 1024 lanes
EXACT = {
    "RPV, regular, oblique, global atomics 256, orders": ("regular", 0.5, 30.0, "RPV", True, GLOBAL_256, 0, True, ORDERS, False),
    "RPV, irregular, oblique back, bricks": ("irregular", 0.6, 210.0, "RPV", True, BRICKS, 0, False, 0, False),
    "RPV, regular, overhead, kernel PRIV 1 at 256 lanes, views": ("regular", 1.0, 0.0, "RPV", True, TALLIES_LDS_256, 0, True, 0, True),
    "RPV, irregular, oblique, kernel PRIV 2 at 512 lanes, orders": ("irregular", 0.5, 30.0, "RPV", True, GRID_LDS_512, 0, True, ORDERS, False),
    "Ross-Li, regular, oblique back, own choice": ("regular", 0.6, 210.0, "RossLi", True, OWN_CHOICE, 0, True, 0, False),
    "Ross-Li, irregular, overhead, wide plan": ("irregular", 1.0, 0.0, "RossLi", True, WIDE, 0, False, 0, False),
    "Ross-Li, regular, oblique, layerSkip, global atomics 512": ("regular", 0.5, 30.0, "RossLi", True, GLOBAL_512, 1, True, 0, False),
    "Ross-Li, irregular, oblique back, kernel PRIV 1 at 512 lanes, views": ("irregular", 0.6, 210.0, "RossLi", True, TALLIES_LDS_512, 0, True, 0, True),
    "Cox-Munk sampled, regular, oblique, kernel PRIV 2 at 256 lanes": ("regular", 0.5, 30.0, "CoxMunk", True, GRID_LDS_256, 0, True, 0, False),
    "Cox-Munk sampled, irregular, oblique back, kernel PRIV 2 at 512 lanes": ("irregular", 0.6, 210.0, "CoxMunk", True, GRID_LDS_512, 0, False, 0, False),
    "Cox-Munk plain, regular, overhead, bricks": ("regular", 1.0, 0.0, "CoxMunk", False, BRICKS, 0, True, 0, False),
    "Cox-Munk sampled, irregular, oblique, own choice": ("irregular", 0.5, 30.0, "CoxMunk", True, OWN_CHOICE, 0, True, 0, False),
}


def expected_walk(name):
    """What walkMode() must say of a row's plan once the domain is loaded: the bits it can tell."""
    tuning, layer_skip = EXACT[name][5], EXACT[name][6]
    want = dict(blockWalk=False, layerSkip=bool(layer_skip))
    if "privateTallies" in tuning:
        want.update(privateTallies=tuning["privateTallies"] in (1, 2), widePlan=tuning["privateTallies"] == 4)
        if tuning["privateTallies"] == 4:
            del want["privateTallies"]  # (tests/test_gpu_epilogue.py asserts widePlan alone of the wide plan)
    else:  # the library's own choice for this medium: private tallies, not the wide plan
        want.update(privateTallies=True, widePlan=False)
    return want


def oracle_setup(name):
    """(case, oracle problem, oracle source, oracle intensity or None) of an exact-tier row."""
    from oracle import oracle as O
    grid, mu0, phi0, model, glint, _, _, rr, _, views = EXACT[name]
    case = with_surface(medium(grid), model, glint=glint)
    P = cases.oracle_problem(case, nsteps=LC.TABLE, use_russian_roulette=rr)
    inten = cases.oracle_intensity(case, VIEWS[0], VIEWS[1], n_angles=FWD_ANGLES) if views else None
    return case, P, O.solar_source(mu0, phi0), inten


def oracle_run(name, first, count, **kw):
    """oracle.compute_rt_brdf of the row's ids first .. first + count - 1 on their Philox streams, delta = DELTA."""
    from oracle import oracle as O
    case, P, src, inten = oracle_setup(name)
    kw.setdefault("delta", DELTA)
    return O.compute_rt_brdf(P, src, O.philox_rng(LC.SEED, first), count, intensity=inten, orders=EXACT[name][8], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# bracket of the product's results from the oracle's sums (the exact tier's tolerance)
# ---------------------------------------------------------------------------------------------------------------------
def brdf_bracket(res, xe, ye, ze, n):
    """[lo, hi] for every float reportResults() may return for the photons whose oracle sums are `res` (oracle.compute_rt_brdf):
    dict name -> (lo, hi), float32 -- fluxUp, fluxDown, fluxAbsorbed [ny, nx], volumeAbsorption [nz, ny, nx], absorbedProfile [nz],
    meanFluxUp / Down / Absorbed, and with orders fluxUpByScatOrd, fluxDownByScatOrd [orders, ny, nx] and their means [orders].

    level_cases.product_bracket with the slack in it.  Per bin the oracle holds S (the double sum of its deposits), c (their
    number) and K (the slack sum of w rho: what two correct evaluations of R may make of the weights since the photon's first
    BRDF reflection).  The product adds the integer nearest to w' 2^32 per deposit (weight_to_fixed_wide: its
    integer part is exact and above 1 so is its fraction, a multiple of 2^-23; below 1 it is weight_to_fixed, off by at most half
    a unit), w' within w rho of the oracle's w: its tally R obeys |R 2^-32 - S| <= K + c 2^-33 + c 2^-53 S
    (level_cases.tally_ends).  R is an integer: it lies between the floor and the ceiling of the two ends.  The epilogue's
    arithmetic (tests/epilogue_mirror.py: batch_values) is correctly rounded and monotone in its non-negative inputs -- the
    column absorption is the integer sum of the column's volume bins -- so the two ends pushed through it bracket the floats."""
    orders = res["fluxUpByOrd"].shape[0] if "fluxUpByOrd" in res else 0
    g = EM.Grid(xe, ye, ze, nDir=0, nOrd=orders)
    parts = ["fluxUp", "fluxDown", "volumeAbsorption"] + (["fluxUpByOrd", "fluxDownByOrd"] if orders else [])
    ends = []
    for e in (0, 1):
        slab = [LC.tally_ends(res[k], res[k + "Count"], res[k + "Slack"])[e].reshape(-1) * 4294967296.0 for k in parts]
        slab = np.concatenate(slab)
        ends.append((np.floor(slab) if e == 0 else np.ceil(slab)).astype(np.int64))
    out = {}
    vals = [EM.batch_values(g, slab, n) for slab in ends]
    col, cell = (g.ny, g.nx), (g.nz, g.ny, g.nx)

    def pair(f):
        return tuple(f(v) for v in vals)
    out["fluxUp"], out["fluxDown"], out["fluxAbsorbed"] = (pair(lambda v, i=i: v[0][i].reshape(col)) for i in range(3))
    out["meanFluxUp"], out["meanFluxDown"], out["meanFluxAbsorbed"] = (pair(lambda v, i=i: v[1][i]) for i in range(3))
    out["absorbedProfile"] = pair(lambda v: v[1][3:])
    out["volumeAbsorption"] = pair(lambda v: v[2].reshape(cell))
    if orders:
        ocol = (orders,) + col
        out["fluxUpByScatOrd"] = pair(lambda v: v[4][:orders * g.ncol].reshape(ocol))
        out["fluxDownByScatOrd"] = pair(lambda v: v[4][orders * g.ncol:].reshape(ocol))
        out["meanFluxUpByScatOrd"] = pair(lambda v: v[5][:orders])
        out["meanFluxDownByScatOrd"] = pair(lambda v: v[5][orders:])
    return out


# the oracle's key whose deposit count tells whether a bin of the product's may be other than 0
COUNTS = dict(fluxUp="fluxUpCount", fluxDown="fluxDownCount", fluxAbsorbed="fluxAbsorbedCount", volumeAbsorption="volumeAbsorptionCount",
              fluxUpByScatOrd="fluxUpByOrdCount", fluxDownByScatOrd="fluxDownByOrdCount")


def product_arrays(got, orders):
    """reportResults() in the bracket's layouts (x fastest): name -> float array."""
    out = {k: np.asarray(got[k]).T for k in ("fluxUp", "fluxDown", "fluxAbsorbed")}
    out["volumeAbsorption"] = np.asarray(got["volumeAbsorption"]).transpose(2, 1, 0)
    out["absorbedProfile"] = np.asarray(got["absorbedProfile"])
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        out[k] = np.float32(got[k])
    if orders:
        for k in ("fluxUpByScatOrd", "fluxDownByScatOrd"):
            out[k] = np.asarray(got[k]).transpose(2, 1, 0)
            out["mean" + k[0].upper() + k[1:]] = np.asarray(got["mean" + k[0].upper() + k[1:]])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# statistical tier: level_cases.stretched_cut over each model's patches, the oracle's MT mode against its Philox mode (CPU) and
# against the product
# ---------------------------------------------------------------------------------------------------------------------
STAT_SUN = (0.5, 30.0)
STAT_VIEWS = ([1.0, 0.5], [0.0, 120.0])
ZETA_MIN = 0.3
STATISTICAL = ("RPV", "RossLi", "CoxMunk")


def statistical_case(model):
    """level_cases.stretched_cut() with its 4 x 3 patches given that model's parameters (SURFACES[model], tiled)."""
    case = LC.stretched_cut()
    q = np.asarray(SURFACES[model], np.float32)
    table = np.array([[q[ix % q.shape[0], iy % q.shape[1]] for iy in range(3)] for ix in range(4)], np.float32)
    _, x, y = case["surface"]
    out = dict(case)
    out.pop("surface")
    out["surface_brdf"] = (model, np.ascontiguousarray(table.transpose(2, 0, 1)), x, y)
    return out


def _stat_worker(args):
    model, mode, seed, proc, first_batch, n_batches, ppb = args
    from oracle import oracle as O
    case = statistical_case(model)
    P = cases.oracle_problem(case, use_russian_roulette=True)
    inten = cases.oracle_intensity(case, STAT_VIEWS[0], STAT_VIEWS[1], n_angles=FWD_ANGLES, use_russian_roulette=True, zeta_min=ZETA_MIN)
    rng = O.mt_rng([seed, proc, 0]) if mode == "mt" else None
    out = []
    for b in range(first_batch, first_batch + n_batches):
        if mode == "philox":
            rng = O.philox_rng(seed, b * ppb)
        r = O.compute_rt_brdf(P, O.solar_source(*STAT_SUN), rng, ppb, intensity=inten)
        v = O.normalize(P, r["n"], r["float"])
        I = r["intensity"].astype(np.float64) / O._nppc(P, r["n"]).reshape(-1)[None, :]
        means = np.concatenate([[v[k].mean(dtype=np.float64) for k in ("fluxUp", "fluxDown", "fluxAbsorbed")], I.mean(axis=1)])
        bins = np.concatenate([v["fluxUp"], v["fluxDown"], v["fluxAbsorbed"], I.reshape(-1)]).astype(np.float64)
        out.append((ppb, means, bins))
    return out


def oracle_stat_run(model, mode, n_batches, ppb, seed=10, procs=None):
    """-> {"means": (mean, stderr) of [meanFluxUp, meanFluxDown, meanFluxAbsorbed | meanIntensity per view], "bins": the same of
    [fluxUp | fluxDown | fluxAbsorbed | intensity per view] per column, x fastest} from the batch variance, the oracle spread over
    processes as level_cases.oracle_level_run spreads it."""
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
            jobs.append((model, mode, seed, p + 1, lo, nb, ppb))
        lo += nb
    if len(jobs) == 1:
        parts = [_stat_worker(jobs[0])]
    else:
        with mp.get_context("spawn").Pool(len(jobs)) as pool:
            parts = pool.map(_stat_worker, jobs)
    rows = [r for part in parts for r in part]
    return {"means": O.batch_statistics([(n, m) for n, m, _ in rows]), "bins": O.batch_statistics([(n, b) for n, _, b in rows])}
