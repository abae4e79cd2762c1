"""Media, references and the host mirror for the actinic flux of every cell (recActinicFlux), shared by
tests/test_actinic_host.py (CPU) and tests/test_gpu_actinic.py.

Layouts (col = ix + nx iy, voxel v = col + ncol iz, as tests/epilogue_mirror.py):
  slab part  actinic[nvox] int64, units of 2^-32 2^e km of weighted path (e: actinic_unit)
  moments    the tail [meanActinic nz | actinic nvox] behind every other tail, in S1, S2 and the last-batch array"""
import numpy as np

from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC

F32, F64 = np.float32, np.float64
CALLS = ((8000, 2), (4000, 1))  # 20 000 photons in 3 batches: two of 8000 in one call, then the rest


# ---------------------------------------------------------------------------------------------------------------------
# the fixed point (mcbrat_api.hip: actinic_unit) and the epilogue (mcbrat_kernels.hip: the actinic parts -- cell_fold with
# actinic_value, their batch_mean and mean_fold) written out
# ---------------------------------------------------------------------------------------------------------------------
def actinic_unit(xe, ye, ze):
    """2^e km: e the smallest integer with (diagonal of the largest spacings of the three axes) (1 + 2^-10) < 2^e."""
    w = [float(np.max(np.diff(np.asarray(e, F64)))) for e in (xe, ye, ze)]
    longest = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * (1.0 + 1.0 / 1024.0)
    return float(np.ldexp(1.0, int(np.frexp(longest)[1])))


def actinic_values(g, raw, n, unit):
    """One batch's normalised values from its raw bins [nvox] int64: (layer means [nz], cells [nvox]) float32 --
    (float)((((double)raw 2^-32) unit) / ((double)nppc dz)) and the fixed float tree over the columns of a layer."""
    nppc = g.photons_per_column(n)
    raw = np.asarray(raw, np.int64).reshape(g.nz, g.ncol)
    vals = (((raw.astype(F64) * EM.TALLY_INV) * F64(unit)) / (nppc.astype(F64)[None, :] * g.dz[:, None])).astype(F32)
    return EM.tree_mean(vals), vals.reshape(-1)


def actinic_epilogue(g, raws, calls, unit):
    """The actinic tail of the moments after the calls [(photons per batch, batches), ...] (each one launch round) from the raw
    bins of every batch, raws [nBatches, nvox]: (S1 [nz + nvox], S2 [nz + nvox], last [nz + nvox])."""
    n = g.nz + g.nvox
    s1, s2, last = np.zeros(n, F64), np.zeros(n, F64), np.zeros(n, F32)
    b = 0
    for ppb, nb in calls:
        vals = []
        for _ in range(nb):
            vals.append(np.concatenate(actinic_values(g, raws[b], ppb, unit)))
            b += 1
        a1, a2 = EM._fold(np.stack(vals), [ppb] * nb)  # each call folds its batches, then adds its partial sums
        s1, s2, last = s1 + a1, s2 + a2, vals[-1]
    return s1, s2, last


# ---------------------------------------------------------------------------------------------------------------------
# vacuum: what every photon deposits is known
# ---------------------------------------------------------------------------------------------------------------------
def vacuum(xe, ye, ze, albedo=0.0):
    shape = (len(xe) - 1, len(ye) - 1, len(ze) - 1)
    return dict(name="vacuum", xe=np.asarray(xe, F64), ye=np.asarray(ye, F64), ze=np.asarray(ze, F64), albedo=albedo,
                components=[dict(ext=np.zeros(shape), ssa=np.ones(shape), pfIndex=np.ones(shape, np.int32),
                                 legendre=[cases.hg_legendre(0.5, 4)])])


def vacuum_on(grid, albedo=0.0):
    """The vacuum on one of the four grids of tests/level_cases.py (4 x 3 x 5 cells)."""
    xy, z = LC.GRIDS[grid]
    return vacuum(LC._AXES[xy][0], LC._AXES[xy][1], LC._AXES[z][2], albedo)


def small_vacuums():
    """1 x 1 x 1 and 33 x 1 x 2 cells (33 columns: more than half a wave of one-column photons, an odd count)."""
    return {"1 x 1 x 1": vacuum([0.0, 0.25], [0.0, 0.5], [0.0, 0.125]),
            "33 x 1 x 2": vacuum(0.03125 * np.arange(34), [0.0, 0.5], [0.0, 0.0625, 0.1875])}


def overhead_deposits(ze, z_regular, unit):
    """The integer every photon of an overhead sun (direction (0, 0, -1), weight 1) adds to the cells of its column in a vacuum,
    bottom up: the walk's float arithmetic for this one leg, written out.  The launch lies at the fraction 1 - 2^-23 of the
    domain's height (regular z) or of the top layer's index range (irregular z); distances along the leg are floats,
    (float)(edge - pz) * (1 / dz) with 1 / dz = -1, or on a regular z axis the previous distance plus the float spacing."""
    ze = np.asarray(ze, F64)
    nz = len(ze) - 1
    frac = F64(F32(1.0) - F32(1.1920929e-07))
    if z_regular:
        pz = ze[0] + frac * (ze[-1] - ze[0])
    else:
        t = (frac - ze[0]) * F64(nz)
        fl = np.floor(t)
        k = max(min(int(fl) + 1, nz), 1)
        pz = ze[k - 1] + (t - fl) * (ze[k] - ze[k - 1])
    dzf = F32((ze[-1] - ze[0]) / nz)
    scale = F32(1.0 / unit)
    out = np.zeros(nz, np.int64)
    tcur = F32(0.0)
    tnz = F32(ze[nz - 1] - pz) * F32(-1.0)
    for k in range(nz - 1, -1, -1):
        length = F32(tnz - tcur)
        v = F32(F32(F32(1.0) * length) * scale)
        out[k] = (1 << 32) if v >= F32(1.0) else int(np.rint(F64(F32(v * F32(4294967296.0)))))
        tcur = tnz
        if k > 0:
            tnz = F32(tnz + F32(dzf * F32(1.0))) if z_regular else F32(F32(ze[k - 1] - pz) * F32(-1.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# where nothing absorbs: a two-layer isotropically scattering slab against the integral equation
# ---------------------------------------------------------------------------------------------------------------------
SLAB = dict(dtaus=[0.5, 2.0], omegas=[1.0, 0.9], albedo=0.3, mu0=0.6, phi0=25.0)


def slab_case():
    """Top layer conservative (tau 0.5), bottom layer omega0 = 0.9 (tau 2), isotropic, on 3 x 2 columns, as
    tests.test_analytic.layered_case mixes its layers: a conservative scatterer and an absorber."""
    dt, om = np.asarray(SLAB["dtaus"]), np.asarray(SLAB["omegas"])
    xe, ye, ze = np.array([0.0, 0.3, 0.5, 0.9]), np.array([0.0, 0.45, 0.7]), np.array([0.0, 0.08, 0.13])
    shape = (3, 2, 2)
    ext = np.broadcast_to((dt[::-1] / np.diff(ze))[None, None, :], shape).copy()  # per layer, bottom up
    omb = np.broadcast_to(om[::-1][None, None, :], shape).copy()
    iso = [np.zeros(2, np.float32)]
    comps = [dict(ext=ext * omb, ssa=np.ones(shape), pfIndex=np.ones(shape, np.int32), legendre=iso),
             dict(ext=ext * (1.0 - omb), ssa=np.zeros(shape), pfIndex=np.ones(shape, np.int32), legendre=iso)]
    return dict(name="two layers", xe=xe, ye=ye, ze=ze, components=comps, albedo=SLAB["albedo"])


def layered_reference(cells_per_layer=150):
    """4 pi J per layer of SLAB from tests.test_analytic._layered_solution, the solver's mean intensity J averaged over each
    layer's cells by optical depth -- the actinic flux per unit flux through a horizontal unit area at the top -- and what
    each layer absorbs by the same J.  Top layer first, as SLAB."""
    from tests import test_analytic as A
    _, h, om, _, _, j = A._layered_solution(SLAB["dtaus"], SLAB["omegas"], SLAB["mu0"], SLAB["albedo"], cells_per_layer)
    nl = len(SLAB["dtaus"])
    jh = (4.0 * np.pi * j * h).reshape(nl, cells_per_layer)
    hh = h.reshape(nl, cells_per_layer)
    absorbed = (4.0 * np.pi * (1.0 - om) * j * h).reshape(nl, cells_per_layer).sum(axis=1)
    return dict(actinic=jh.sum(axis=1) / hh.sum(axis=1), absorbed=absorbed)


# ---------------------------------------------------------------------------------------------------------------------
# track length against collisions
# ---------------------------------------------------------------------------------------------------------------------
def sigma_abs(case):
    """sum over the components of ext_c (1 - omega0_c) per cell, km^-1, [nx, ny, nz]."""
    shape = (len(case["xe"]) - 1, len(case["ye"]) - 1, len(case["ze"]) - 1)
    s = np.zeros(shape)
    for comp in case["components"]:
        ext, ssa = np.asarray(comp["ext"], F64), np.asarray(comp["ssa"], F64)
        if ext.ndim == 1:  # a 1-D component: per layer
            ext, ssa = ext[None, None, :], ssa[None, None, :]
        s = s + np.broadcast_to(ext * (1.0 - ssa), shape)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the product against the oracle's track-length tally (oracle.compute_rt_actinic): tests/test_oracle_actinic.py (CPU) and
# tests/test_gpu_actinic_oracle.py
# ---------------------------------------------------------------------------------------------------------------------
MAX_IDS = 128  # photon ids per product call of the exact tier
SOLAR_EXACT = [n for n, v in LC.EXACT.items() if v[1] is not None]


def split_runs(runs, most=MAX_IDS):
    """[(first id, count)] of the calls that trace the runs of clean ids, none longer than `most`."""
    return [(first + lo, min(most, count - lo)) for first, count in runs for lo in range(0, count, most)]


def actinic_bracket(res, xe, ye, ze, n):
    """[lo, hi] for every float reportActinicFlux() may return for the photons whose oracle sums are `res`
    (oracle.compute_rt_actinic): dict(actinicFlux=(lo, hi) [nz, ny, nx], meanActinicFlux=(lo, hi) [nz]), float32.

    Per bin the oracle holds S = sum of w l (km, double), the deposits c and actinicSlack = sum of w 2 delta.  The product's
    integer tally R (units of 2^-32 2^e km, 2^e = actinic_unit) is the sum over the same pieces of
    rint(fl(fl(w l') 2^-e) 2^32), l' its own float length of the piece.  Term by term, |R 2^-32 2^e - S| is at most

    * sum of w |l' - l| <= sum of w 2 delta = actinicSlack: the two walks place each end of a piece (a face, a collision point)
      within delta = 64 x 2^-23 x (the path so far) of each other -- the margin by which a photon is called clean, so an end that
      could fall on the other side of a face is not among the ids compared;
    * the float roundings of l' = tmin - tcur and of w l', 2^-24 relative each (the scaling by 2^-e and by 2^32 is exact):
      (1 + 2^-24)^2 - 1 < 3 x 2^-24 of the product's own sum, itself at most S + actinicSlack;
    * half a fixed-point unit per deposit, c 2^-33 2^e (a value rounded to zero, or a negative length converted to zero, which
      only moves it towards the oracle's non-negative piece, included);
    * the rounding of the oracle's own double sum of c non-negative terms, c 2^-53 S.

    R is an integer: it lies between the floor and the ceiling of the two ends in its unit.  The epilogue then forms
    (float)(((R 2^-32) 2^e) / (nppc dz)) per cell and the fixed float tree over the columns of a layer (actinic_values): every
    step is a correctly rounded operation, monotone in its non-negative inputs, so pushing the two ends through the written-out
    epilogue brackets the floats.  No measured slack."""
    g = EM.Grid(xe, ye, ze)
    unit = actinic_unit(xe, ye, ze)
    s, c, slack = res["actinic"].reshape(-1), res["actinicCount"].reshape(-1).astype(F64), res["actinicSlack"].reshape(-1)
    half = slack + 3.0 * 2.0 ** -24 * (s + slack) + c * 2.0 ** -33 * unit + c * 2.0 ** -53 * s
    to_raw = 4294967296.0 / unit
    ends = [np.floor(np.maximum(s - half, 0.0) * to_raw).astype(np.int64), np.ceil((s + half) * to_raw).astype(np.int64)]
    (mlo, clo), (mhi, chi) = (actinic_values(g, raw, n, unit) for raw in ends)
    shape = res["actinic"].shape
    return dict(actinicFlux=(clo.reshape(shape), chi.reshape(shape)), meanActinicFlux=(mlo, mhi))


def _actinic_worker(args):
    name, mode, seed, proc, first_batch, n_batches, ppb = args
    from oracle import oracle as O
    make, mu0, phi0 = LC.STATISTICAL[name]
    P = cases.oracle_problem(make(), use_russian_roulette=True)
    rng = O.mt_rng([seed, proc, 0]) if mode == "mt" else None
    out = []
    for b in range(first_batch, first_batch + n_batches):
        if mode == "philox":
            rng = O.philox_rng(seed, b * ppb)
        r = O.compute_rt_actinic(P, O.solar_source(mu0, phi0), rng, ppb)
        v = O.normalize_actinic(P, r["n"], r)
        out.append((ppb, v["meanActinicFlux"], v["actinicFlux"].reshape(-1)))
    return out


def oracle_actinic_run(name, mode, n_batches, ppb, seed=10, procs=None):
    """-> {"means": (mean, stderr) of meanActinicFlux [nz], "bins": the same of actinicFlux [nz ny nx], layer slowest, x fastest}
    of a case of level_cases.STATISTICAL from the batch variance, the oracle spread over processes as
    level_cases.oracle_level_run spreads it."""
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
        parts = [_actinic_worker(jobs[0])]
    else:
        with mp.get_context("spawn").Pool(len(jobs)) as pool:
            parts = pool.map(_actinic_worker, jobs)
    rows = [r for part in parts for r in part]
    return {"means": O.batch_statistics([(n, m) for n, m, _ in rows]), "bins": O.batch_statistics([(n, b) for n, _, b in rows])}


SOLAR_THEORY = ("isotropic layers over albedo 0.5", "HG g = 0.85, tau = 4, regular z", "homogeneous on a stretched 7 x 5 x 12 grid")


def actinic_theory(name):
    """level_cases.theory(name) with the layer means of the actinic flux that its level fluxes imply.  In a plane-parallel medium
    what layer k absorbs is the difference of the net flux (down - up) between its two levels, and it is sigma_abs dz times the
    layer's actinic flux: actinic[k] = (net[k + 1] - net[k]) / ((1 - omega_k) dtau_k), (1 - omega_k) dtau_k = sigma_abs_k dz_k, wherever
    that is positive (`layers`).  floor[k] = 4e-6 / ((1 - omega_k) dtau_k): 1e-6 on each of the four fluxes, through the quotient."""
    t = LC.theory(name)
    sig = sigma_abs(t["case"])
    assert np.all(sig == sig[:1, :1, :])  # plane parallel
    absorbing = sig[0, 0] * np.diff(np.asarray(t["case"]["ze"], F64))
    layers = absorbing > 0
    net = np.asarray(t["down"], F64) - np.asarray(t["up"], F64)
    safe = np.where(layers, absorbing, 1.0)
    return dict(t, layers=layers, actinic=np.where(layers, (net[1:] - net[:-1]) / safe, np.nan), floor=np.where(layers, 4e-6 / safe, np.nan))
