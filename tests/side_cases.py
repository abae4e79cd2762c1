"""Media, the written-out epilogue and the ray-cast helper for the flux through the vertical faces of every cell (recSideFluxes,
DESIGN.md section 4.15), shared by tests/test_side_flux_host.py (CPU) and tests/test_gpu_side_flux.py.

Layouts (col = ix + nx iy, voxel v = col + ncol iz, as tests/epilogue_mirror.py; the four parts in the order of NAMES):
  slab part  side[4][nvox] int64, units of 2^-32 photon weights; bin (q, ix, iy, k) is the face x = xe[ix + 1] (q 0, 1) or
             y = ye[iy + 1] (q 2, 3) of the patch (row iy or column ix, layer k), crossed towards + (q 0, 2) or - (q 1, 3)
  moments    the tail [means 4 nz | bins 4 nvox] behind every other tail, in S1, S2 and the last-batch array"""
import numpy as np

from tests import cases
from tests import epilogue_mirror as EM
from tests import level_cases as LC

F32, F64 = np.float32, np.float64
NAMES = ("sideFluxXPlus", "sideFluxXMinus", "sideFluxYPlus", "sideFluxYMinus")
MEANS = tuple("mean" + n[0].upper() + n[1:] for n in NAMES)
CALLS = ((8000, 2), (4000, 1))  # 20 000 photons in 3 batches: two of 8000 in one call, then the rest
MAX_IDS = 128                   # photon ids per product call of the photon-by-photon tier
DELTA = 64.0 * 2.0 ** -23       # times the km travelled: the margin by which a photon id is called clean


# ---------------------------------------------------------------------------------------------------------------------
# the epilogue (mcbrat_kernels.hip: the side parts -- cell_fold<4> with side_value, their batch_mean and mean_fold) written out
# ---------------------------------------------------------------------------------------------------------------------
def side_extents(g):
    """[4, ncol] double: the cell's extent along the crossed axis -- dx of the column for the x parts, dy for the y parts."""
    dx, dy = np.diff(g.xe), np.diff(g.ye)
    ex = np.broadcast_to(dx[None, :], (g.ny, g.nx)).reshape(-1)
    ey = np.broadcast_to(dy[:, None], (g.ny, g.nx)).reshape(-1)
    return np.stack([ex, ex, ey, ey])


def side_values(g, raw, n):
    """One batch's normalised values from its raw bins [4, nz, ncol] int64: (layer means [4 nz], bins [4 nvox]) float32 --
    F = (float)((((double)raw 2^-32) len) / ((double)nppc dz)), len = dx of an x face and dy of a y face, nppc the photons of
    the cell's column; the means by the fixed float tree over the columns of a layer."""
    nppc = g.photons_per_column(n).astype(F64)
    raw = np.asarray(raw, np.int64).reshape(4, g.nz, g.ncol)
    vals = (((raw.astype(F64) * EM.TALLY_INV) * side_extents(g)[:, None, :]) / (nppc[None, None, :] * g.dz[None, :, None])).astype(F32)
    return EM.tree_mean(vals).reshape(-1), vals.reshape(-1)


def side_epilogue(g, raws, calls):
    """The side tail of the moments after the calls [(photons per batch, batches), ...] (each one launch round) from the raw
    bins of every batch, raws [nBatches, 4, nz, ncol]: (S1, S2, last), each [4 nz + 4 nvox]."""
    n = 4 * (g.nz + g.nvox)
    s1, s2, last = np.zeros(n, F64), np.zeros(n, F64), np.zeros(n, F32)
    b = 0
    for ppb, nb in calls:
        vals = []
        for _ in range(nb):
            vals.append(np.concatenate(side_values(g, raws[b], ppb)))
            b += 1
        a1, a2 = EM._fold(np.stack(vals), [ppb] * nb)  # each call folds its batches, then adds its partial sums
        s1, s2, last = s1 + a1, s2 + a2, vals[-1]
    return s1, s2, last


def report_arrays(rep, g):
    """reportSideFluxes()' dict -> (means [4 nz], bins [4 nvox]) in the library's order."""
    return (np.concatenate([np.asarray(rep[m], F32) for m in MEANS]),
            np.concatenate([np.asarray(rep[n], F32).transpose(2, 1, 0).reshape(-1) for n in NAMES]))


# ---------------------------------------------------------------------------------------------------------------------
# media: one extinction value (or none), omega0 = 0, albedo 0 -- every weight is exactly 1
# ---------------------------------------------------------------------------------------------------------------------
def black(xe, ye, ze, ext, albedo=0.0, ssa=0.0):
    shape = (len(xe) - 1, len(ye) - 1, len(ze) - 1)
    return dict(name="black" if ext else "vacuum", xe=np.asarray(xe, F64), ye=np.asarray(ye, F64), ze=np.asarray(ze, F64), albedo=albedo,
                components=[dict(ext=np.full(shape, float(ext)), ssa=np.full(shape, float(ssa)), pfIndex=np.ones(shape, np.int32),
                                 legendre=[cases.hg_legendre(0.5, 4)])])


def axes(grid):
    """The edges of one of the four 4 x 3 x 5 grids of tests/level_cases.py, or of the two small domains."""
    if grid == "1 x 1 x 1":
        return np.array([0.0, 0.25]), np.array([0.0, 0.5]), np.array([0.0, 0.125])
    if grid == "33 x 1 x 2":
        return 0.03125 * np.arange(34), np.array([0.0, 0.5]), np.array([0.0, 0.0625, 0.125])
    xy, z = LC.GRIDS[grid]
    return LC._AXES[xy][0], LC._AXES[xy][1], LC._AXES[z][2]


GRIDS = tuple(LC.GRIDS) + ("1 x 1 x 1", "33 x 1 x 2")
# the photon-by-photon cases: (grid, extinction, mu0, phi0)
RAY_CASES = [(grid, ext, mu0, phi0) for grid in GRIDS for ext, suns in ((LC.EXT, ((0.5, 30.0), (0.6, 210.0))),
                                                                         (0.0, ((0.5, 30.0), (0.6, 210.0), (0.2, 75.0))))
             for mu0, phi0 in suns]


def medium_on(grid, ext, albedo=0.0, ssa=0.0):
    return black(*axes(grid), ext, albedo, ssa)


# ---------------------------------------------------------------------------------------------------------------------
# the ray-cast helper: the first leg of every photon id, from the definition of DESIGN.md section 4.15 in double arithmetic
# ---------------------------------------------------------------------------------------------------------------------
_uniform_cache = {}


def launch_uniforms(seed, n):
    """[n, 3] float32: the launch fractions (event 0, block 0, slots 0 and 1) and the first leg's uniform (event 1, block 0, slot
    0) of photon ids 0 .. n-1, from the oracle's Philox generator; float(u) 2^-32 as the kernels form a uniform."""
    key = (int(seed), int(n))
    if key not in _uniform_cache:
        from oracle import oracle as O
        k = (seed & 0xFFFFFFFF, seed >> 32)
        out = np.zeros((n, 3), F32)
        scale = F32(2.3283064365386963e-10)
        for i in range(n):
            a = O.philox4x32_10((0, 0, i & 0xFFFFFFFF, i >> 32), k)
            b = O.philox4x32_10((1, 0, i & 0xFFFFFFFF, i >> 32), k)
            out[i] = (F32(a[0]) * scale, F32(a[1]) * scale, F32(b[0]) * scale)
        _uniform_cache[key] = out
    return _uniform_cache[key]


def launch_height(ze):
    """The launch height of DESIGN.md section 4.10: the fraction 1 - spacing(1.) of the domain's height on a regular z axis, of the
    layer index range on an irregular one (computeRadiativeTransfer :484-493)."""
    ze = np.asarray(ze, F64)
    nz = len(ze) - 1
    frac = F64(F32(1.0) - F32(1.1920929e-07))
    d = float(F32(ze[1] - ze[0]))
    if all(abs((ze[i + 1] - ze[i]) - d) <= 2.0 * EM.spacing(ze[i + 1]) for i in range(nz)):
        return ze[0] + frac * (ze[-1] - ze[0])
    t = (frac - ze[0]) * F64(nz)
    fl = np.floor(t)
    k = max(min(int(fl) + 1, nz), 1)
    return ze[k - 1] + (t - fl) * (ze[k] - ze[k - 1])


def direction(mu0, phi0):
    """makeDirectionCosines of the Directional source: float cosines, widened."""
    mu = -abs(F32(mu0))
    phi = F32(F32(phi0) * np.arccos(F32(-1.0))) / F32(180.0)
    st = np.sqrt(F32(1.0) - mu * mu)
    return np.array([st * np.cos(phi), st * np.sin(phi), mu], F32).astype(F64)


def _plane_hits(p0, d, length, edges, period, images=True):
    """Where the segments p0[i] + t d, 0 < t <= length[i], meet the planes {edges[j] + m period}: (t [n, K], j [K], valid
    [n, K]) over the K candidate planes.  One axis; d is shared by the photons."""
    n = p0.shape[0]
    if d == 0.0:
        return np.zeros((n, 0)), np.zeros(0, np.int64), np.zeros((n, 0), bool)
    if images:
        reach = float(np.max(length)) * abs(d)
        m = np.arange(-int(np.ceil(reach / period)) - 2, int(np.ceil(reach / period)) + 3)
        planes = (edges[None, :-1] + m[:, None] * period).reshape(-1)  # (edges[-1] + m period is edges[0] + (m + 1) period: one plane)
        j = np.tile(np.arange(len(edges) - 1), m.size)
    else:
        planes, j = np.asarray(edges, F64), np.arange(len(edges))
    t = (planes[None, :] - p0[:, None]) / d
    return t, j, (t > 0.0) & (t <= length[:, None])


def ray_cast(grid, ext, mu0, phi0, seed=LC.SEED, n=LC.N_IDS):
    """The first leg of photon ids 0 .. n-1 of the Directional source over a medium of one extinction value `ext` (0: a vacuum),
    omega0 = 0 and albedo 0 -- the whole history of such a photon.  -> dict(
      ids [C], bins [C, 4]: photon id and side bin (q, k, iy, ix) of each of the C crossings, sorted by id,
      flagged [n] bool, ncross [n, 2] (x and y crossings per id), disp [n, 2] (the leg's x and y displacement in km),
      start [n, 2], dims).

    The leg starts at (x0 + U0 Lx, y0 + U1 Ly, launch_height) and runs along direction(mu0, phi0) for
    -log(max(tiny, U)) / ext km, or to the surface if that comes first (always in a vacuum).  An x crossing is a t with
    x(t) = xe[j] + m Lx; its bin is the cell on the face's low side, ix = (j - 1) mod nx, in the patch (iy, k) that holds
    (y(t), z(t)); plus if the leg travels towards +x.  y likewise.  An id is flagged when the leg's end lies within
    delta = DELTA t of a face (the surface it ends on apart), or when an x or y crossing lies within delta of another face's
    crossing along the leg (an edge or a corner: two correct walks may attribute the patch differently)."""
    xe, ye, ze = (np.asarray(e, F64) for e in axes(grid))
    nx_, ny_, nz_ = len(xe) - 1, len(ye) - 1, len(ze) - 1
    Lx, Ly = xe[-1] - xe[0], ye[-1] - ye[0]
    u = launch_uniforms(seed, n)
    d = direction(mu0, phi0)
    z0 = launch_height(ze)
    to_surface = (ze[0] - z0) / d[2]
    px, py = xe[0] + u[:, 0].astype(F64) * Lx, ye[0] + u[:, 1].astype(F64) * Ly
    pz = np.full(n, z0)
    length = np.full(n, to_surface)
    if ext > 0.0:
        free = (-np.log(np.maximum(u[:, 2], np.finfo(F32).tiny))).astype(F64) / ext
        length = np.minimum(length, free)
    lands = length >= to_surface
    tx, jx, vx = _plane_hits(px, d[0], length, xe, Lx)
    ty, jy, vy = _plane_hits(py, d[1], length, ye, Ly)
    tz, _, vz = _plane_hits(pz, d[2], length, ze[1:], 0.0, images=False)  # (the surface, ze[0], a leg ends on is no crossing)
    # flags: the end near a face (perpendicular distance) ...
    delta = DELTA * length
    ex, ey, ez = px + length * d[0], py + length * d[1], pz + length * d[2]
    wx, wy = np.mod(ex - xe[0], Lx) + xe[0], np.mod(ey - ye[0], Ly) + ye[0]
    near = np.minimum(np.abs(wx[:, None] - xe[None, :]).min(axis=1), np.abs(wy[:, None] - ye[None, :]).min(axis=1)) < delta
    near |= ~lands & (np.abs(ez[:, None] - ze[None, :]).min(axis=1) < delta)
    # ... or an x / y crossing near another face's crossing along the leg
    big = 1e300
    for (ta, va), others in (((tx, vx), ((ty, vy), (tz, vz))), ((ty, vy), ((tx, vx), (tz, vz)))):
        for tb, vb in others:
            if ta.shape[1] and tb.shape[1]:
                gap = np.abs(np.where(va, ta, big)[:, :, None] - np.where(vb, tb, -big)[:, None, :])
                near |= (gap < DELTA * np.where(va, ta, 0.0)[:, :, None]).any(axis=(1, 2))
    ids, bins = [], []
    for a, (t, j, v) in enumerate(((tx, jx, vx), (ty, jy, vy))):
        i, c = np.nonzero(v)
        tt = t[i, c]
        k = np.clip(np.searchsorted(ze, pz[i] + tt * d[2], side="right") - 1, 0, nz_ - 1)
        if a == 0:
            iy = np.clip(np.searchsorted(ye, np.mod(py[i] + tt * d[1] - ye[0], Ly) + ye[0], side="right") - 1, 0, ny_ - 1)
            b = np.stack([np.full(i.size, 0 if d[0] > 0 else 1), k, iy, (j[c] - 1) % nx_], axis=1)
        else:
            ix = np.clip(np.searchsorted(xe, np.mod(px[i] + tt * d[0] - xe[0], Lx) + xe[0], side="right") - 1, 0, nx_ - 1)
            b = np.stack([np.full(i.size, 2 if d[1] > 0 else 3), k, (j[c] - 1) % ny_, ix], axis=1)
        ids.append(i)
        bins.append(b.astype(np.int64))
    ids, bins = np.concatenate(ids), np.concatenate(bins)
    order = np.argsort(ids, kind="stable")
    return dict(ids=ids[order], bins=bins[order], flagged=near, ncross=np.stack([vx.sum(axis=1), vy.sum(axis=1)], axis=1),
                disp=np.stack([length * d[0], length * d[1]], axis=1), start=np.stack([px, py], axis=1), length=length, lands=lands,
                dims=(nx_, ny_, nz_))


def raw_bins(rc, first, count):
    """[4, nz, ncol] int64: the raw side bins of photon ids first .. first + count - 1, every crossing a weight of exactly 1."""
    nx_, ny_, nz_ = rc["dims"]
    out = np.zeros((4, nz_, ny_, nx_), np.int64)
    lo, hi = np.searchsorted(rc["ids"], [first, first + count])
    c = rc["bins"][lo:hi]
    np.add.at(out, (c[:, 0], c[:, 1], c[:, 2], c[:, 3]), 1)
    return (out << 32).reshape(4, nz_, ny_ * nx_)


def split_runs(runs, most=MAX_IDS):
    """[(first id, count)] of the calls that trace the runs of clean ids, none longer than `most`."""
    return [(first + lo, min(most, count - lo)) for first, count in runs for lo in range(0, count, most)]


# ---------------------------------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------------------------------
def horizontal(mu0, phi0):
    """(tan theta0 cos phi0, tan theta0 sin phi0): the net flux density through a vertical face per unit flux through a horizontal
    unit area, in a vacuum."""
    t = np.sqrt(1.0 - mu0 * mu0) / mu0
    return t * np.cos(np.radians(phi0)), t * np.sin(np.radians(phi0))


def absorber_profile(ze, ext, mu0):
    """mu0 / (sigma dz_k) (exp(-tau_top / mu0) - exp(-tau_bot / mu0)) per layer, bottom up: the layer average of the direct beam."""
    ze = np.asarray(ze, F64)
    tau = ext * (ze[-1] - ze)  # optical depth from the top down to every level
    return mu0 / (ext * np.diff(ze)) * (np.exp(-tau[1:] / mu0) - np.exp(-tau[:-1] / mu0))
