"""A host mirror of the epilogue of a call (mcbrat_kernels.hip: finish_gather / finish_fold; finish_excess is not mirrored):
integer batch tallies in, the f64 moment array and the f32 `last` array out, with the kernels' float32 / float64 operations
in the kernels' order, so that the GPU's results can be compared with it bit for bit.

Plain numpy.  The operations are vectorised over output elements only: every element sees the same sequence of IEEE
operations as its owner thread on the device (the library is built with -ffp-contract=off, so no fused multiply-adds).

Layouts (DESIGN.md sections 2 and 4.9; col = ix + nx * iy, voxel v = col + ncol * iz):
  slab     [fluxUp ncol | fluxDown ncol | volume nvox | intensity ncol nDir | upByOrd ncol nOrd | downByOrd ncol nOrd |
            intensityByOrd ncol nDir nOrd]   (int64, 2^-32 photon weights; no limitIntensityContributions part)
  moments  header(8) + S1[M] + S2[M], M = moments_len
  last     [meanUp meanDown meanAbs | up ncol | down ncol | absorbed ncol | profile nz | volume nvox | intensity ncol nDir |
            meanUpByOrd nOrd | meanDownByOrd nOrd | upByOrd ncol nOrd | downByOrd ncol nOrd | meanIntensityByOrd nDir nOrd |
            intensityByOrd ncol nDir nOrd]"""
import numpy as np

F32, F64 = np.float32, np.float64
TALLY_INV = 2.0 ** -32  # kTallyInv
LANES = 256             # kFinishBlock: the lanes of the strided float tree


def spacing(x):
    """spacing_d (mcbrat_api.hip): Fortran SPACING of a double."""
    x = abs(float(x))
    return np.finfo(np.float64).tiny if x == 0.0 else np.ldexp(1.0, int(np.frexp(x)[1]) - 53)


def xy_regular(xe, ye):
    """The library's regular-spacing flag for x/y (mcbrat_set_grid; new_Integrator :163-181)."""
    def reg(e):
        e = np.asarray(e, np.float64)
        d = float(F32(e[1] - e[0]))
        return all(abs((e[i + 1] - e[i]) - d) <= 2.0 * spacing(e[i + 1]) for i in range(len(e) - 1))
    return reg(xe) and reg(ye)


def relative_areas(xe, ye):
    """relArea[col] (mcbrat_set_grid; computeRadiativeTransfer :334-340): a double expression stored to float."""
    xe, ye = np.asarray(xe, np.float64), np.asarray(ye, np.float64)
    dx, dy = np.diff(xe), np.diff(ye)
    a = (dy[:, None] * dx[None, :]) / ((xe[-1] - xe[0]) * (ye[-1] - ye[0]))  # [iy, ix]: col = ix + nx iy
    return a.reshape(-1).astype(F32)


def moments_len(ncol, nz, nDir, nOrd):
    return 3 + 3 * ncol + nz + ncol * nz + nDir * ncol + nOrd * (2 + nDir) * (1 + ncol)


def slab_len(ncol, nz, nDir, nOrd):
    return 2 * ncol + ncol * nz + nDir * ncol + nOrd * (2 + nDir) * ncol


def tree_mean(values):
    """batch_mean and its tree_sum (the flux means, the profile, every tally's means): lane t sums values[t], values[t + 256], ... in float; a fixed tree of 256 lanes
    (red[t] += red[t + o], o = 128 .. 1); red[0] / (float)ncol.  `values`: [..., ncol] float32, reduced over the last axis."""
    v = np.asarray(values, F32)
    ncol = v.shape[-1]
    rows = -(-ncol // LANES)
    pad = np.zeros(v.shape[:-1] + (rows * LANES,), F32)  # (s + 0.0f == s: the padding adds nothing)
    pad[..., :ncol] = v
    pad = pad.reshape(v.shape[:-1] + (rows, LANES))
    red = np.zeros(v.shape[:-1] + (LANES,), F32)
    for r in range(rows):
        red = red + pad[..., r, :]
    o = LANES // 2
    while o > 0:
        red[..., :o] = red[..., :o] + red[..., o:2 * o]
        o >>= 1
    return red[..., 0] / F32(ncol)


def sequential_mean(values):
    """mcbrat_report_intensity's meanIntensity: a float sum in column order over (float)ncol (reportResults :980-992)."""
    v = np.asarray(values, F32)
    s = np.zeros(v.shape[:-1], F32)
    for c in range(v.shape[-1]):
        s = s + v[..., c]
    return s / F32(v.shape[-1])


class Grid:
    """What the epilogue knows of the domain: the cell edges (and the x/y flag and column areas the library derives)."""

    def __init__(self, xe, ye, ze, nDir=0, nOrd=0):
        self.xe, self.ye, self.ze = (np.asarray(e, np.float64) for e in (xe, ye, ze))
        self.nx, self.ny, self.nz = len(self.xe) - 1, len(self.ye) - 1, len(self.ze) - 1
        self.ncol = self.nx * self.ny
        self.nvox = self.ncol * self.nz
        self.nDir, self.nOrd = int(nDir), int(nOrd)
        self.regular = xy_regular(self.xe, self.ye)
        self.relArea = relative_areas(self.xe, self.ye)
        self.dz = np.diff(self.ze)
        self.M = moments_len(self.ncol, self.nz, self.nDir, self.nOrd)
        self.S = slab_len(self.ncol, self.nz, self.nDir, self.nOrd)
        self.base = 3 + 3 * self.ncol + self.nz + self.nvox + self.nDir * self.ncol  # moments_base
        self.slabOrders = 2 * self.ncol + self.nvox + self.nDir * self.ncol       # slab_orders

    def photons_per_column(self, n):
        """[ncol] float: (float)n / (float)ncol on a regular x/y grid, relArea[col] * (float)n otherwise (:331, :342)."""
        if self.regular:
            return np.full(self.ncol, F32(n) / F32(self.ncol), F32)
        return self.relArea * F32(n)

    def empty_moments(self):
        return np.zeros(8 + 2 * self.M, np.float64)

    def empty_last(self):
        return np.zeros(self.M, F32)


def batch_values(g, slab, n):
    """The normalised values of one batch: (columns [3, ncol], scalars [3 + nz], volume [nvox], intensity [nDir ncol],
    order bins [(2 + nDir) nOrd ncol], order means [(2 + nDir) nOrd]) -- float32, formed as the finish kernels form them."""
    slab = np.asarray(slab, np.int64)
    ncol, nz = g.ncol, g.nz
    nppc = g.photons_per_column(n)

    def colv(raw):  # column_value: (float)((double)raw * 2^-32) / nppc
        return (np.asarray(raw, np.int64).astype(F64) * TALLY_INV).astype(F32) / nppc

    vol_raw = slab[2 * ncol:2 * ncol + g.nvox].reshape(nz, ncol)
    absorbed = np.zeros(ncol, np.int64)
    for k in range(nz):  # (integer: exact in any order)
        absorbed = absorbed + vol_raw[k]
    cols = np.stack([colv(slab[:ncol]), colv(slab[ncol:2 * ncol]), colv(absorbed)])
    # volume: (float)(((double)raw * 2^-32) / (((double)nppc * dz) * 1000.0))
    denom = (nppc.astype(F64)[None, :] * g.dz[:, None]) * 1000.0
    vol = ((vol_raw.astype(F64) * TALLY_INV) / denom).astype(F32)
    scal = np.concatenate([tree_mean(cols), tree_mean(vol)])
    i0 = 2 * ncol + g.nvox
    inten = colv(slab[i0:i0 + g.nDir * ncol].reshape(g.nDir, ncol)).reshape(-1) if g.nDir else np.zeros(0, F32)
    nm = (2 + g.nDir) * g.nOrd
    if nm:
        ob = colv(slab[g.slabOrders:g.slabOrders + nm * ncol].reshape(nm, ncol))
        om = tree_mean(ob)
    else:
        ob, om = np.zeros((0, ncol), F32), np.zeros(0, F32)
    return cols, scal, vol.reshape(-1), inten, ob.reshape(-1), om


def _fold(values, ns):
    """s1 += (double)x * n; s2 += n * ((double)x * (double)x) over the batches in order (values [nb, ...] float32)."""
    s1 = np.zeros(values.shape[1:], F64)
    s2 = np.zeros(values.shape[1:], F64)
    for x, n in zip(values, ns):
        xd, nd = x.astype(F64), F64(n)
        s1 = s1 + xd * nd
        s2 = s2 + nd * (xd * xd)
    return s1, s2


def epilogue(g, slabs, ppb, round_size, moments=None, last=None):
    """One mirrored call: `slabs` [nBatches, g.S] int64 are the batches of the call in order, cut into launch rounds of
    `round_size` batches (the library's batches in flight); each round folds its batches and adds its partial sums into the
    moments.  Returns (moments, last), updated in place when given (a call without resetMoments adds to what is there)."""
    slabs = np.asarray(slabs, np.int64)
    nB = slabs.shape[0]
    assert slabs.shape[1] == g.S, (slabs.shape, g.S)
    mom = g.empty_moments() if moments is None else moments
    lst = g.empty_last() if last is None else last
    M, ncol, nz, nvox = g.M, g.ncol, g.nz, g.nvox
    for b0 in range(0, nB, int(round_size)):
        nb = min(int(round_size), nB - b0)
        total = ppb * nb
        ns = [min(total - b * ppb, ppb) for b in range(nb)]  # batch_photons
        per = [batch_values(g, slabs[b0 + b], ns[b]) for b in range(nb)]
        parts = []
        # (moment offset, values [nb, len]) of every part, each folded in batch order
        parts.append((0, np.stack([p[1][:3] for p in per])))                          # domain means (mean_fold: kFoldScalars)
        parts.append((3, np.stack([p[0].reshape(-1) for p in per])))                  # column fluxes (mean_fold: kFoldColumns)
        parts.append((3 + 3 * ncol, np.stack([p[1][3:] for p in per])))               # absorption profile
        parts.append((3 + 3 * ncol + nz, np.stack([p[2] for p in per])))               # volume (cell_fold, volume_value)
        if g.nDir:
            parts.append((3 + 3 * ncol + nz + nvox, np.stack([p[3] for p in per])))   # intensity (bin_fold)
        if g.nOrd:
            no, nd = g.nOrd, g.nDir
            om = np.stack([p[5] for p in per])
            ob = np.stack([p[4] for p in per])
            parts.append((g.base, om[:, :2 * no]))                                     # meanUp/Down by order
            parts.append((g.base + 2 * no, ob[:, :2 * ncol * no]))                     # up/down by order (bin_fold)
            if nd:
                parts.append((g.base + 2 * no + 2 * ncol * no, om[:, 2 * no:]))        # meanIntensity by order
                parts.append((g.base + 2 * no + 2 * ncol * no + nd * no, ob[:, 2 * ncol * no:]))
        for off, vals in parts:
            s1, s2 = _fold(vals, ns)
            k = vals.shape[1]
            mom[8 + off:8 + off + k] = mom[8 + off:8 + off + k] + s1
            mom[8 + M + off:8 + M + off + k] = mom[8 + M + off:8 + M + off + k] + s2
            lst[off:off + k] = vals[-1]
        mom[0] = mom[0] + F64(total)  # header: photons and batches done
        mom[1] = mom[1] + F64(nb)
    return mom, lst


def fold_batch_values(g, values, ppb, round_size, moments=None):
    """The moments of a call from per-batch normalised values instead of tallies: values [nBatches, M] float32 (each batch's
    values at their moment offsets, e.g. recovered from one-batch calls as S1 / n).  Launch rounds as in epilogue()."""
    values = np.asarray(values, F32)
    mom = g.empty_moments() if moments is None else moments
    M = g.M
    for b0 in range(0, values.shape[0], int(round_size)):
        nb = min(int(round_size), values.shape[0] - b0)
        s1, s2 = _fold(values[b0:b0 + nb], [ppb] * nb)
        mom[8:8 + M] = mom[8:8 + M] + s1
        mom[8 + M:8 + 2 * M] = mom[8 + M:8 + 2 * M] + s2
        mom[0] = mom[0] + F64(ppb * nb)
        mom[1] = mom[1] + F64(nb)
    return mom
