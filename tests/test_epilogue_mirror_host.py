"""The epilogue mirror (tests/epilogue_mirror.py) against a literal restatement of the finish kernels: one Python loop per
kernel part, indexed as the kernel indexes (thread by thread, lane by lane), on hand-sized inputs.  Keeps the mirror's own
vectorised indexing honest before the GPU tests hold the kernels to it bit for bit."""
import numpy as np
import pytest

from tests import epilogue_mirror as E

F32, F64 = np.float32, np.float64


def literal_epilogue(g, slabs, ppb, round_size, mom=None, last=None):
    """finish_gather + finish_fold of mcbrat_kernels.hip, restated loop by loop with float32 / float64 scalars."""
    ncol, nz, nvox, nDir, nOrd, M = g.ncol, g.nz, g.nvox, g.nDir, g.nOrd, g.M
    mom = np.zeros(8 + 2 * M) if mom is None else mom
    last = np.zeros(M, F32) if last is None else last
    base = 3 + 3 * ncol + nz + ncol * nz + nDir * ncol
    S = 2 * ncol + ncol * nz + nDir * ncol

    def nppc_of(col, n):
        return F32(n) / F32(ncol) if g.regular else F32(g.relArea[col] * F32(n))

    def cv(raw, nppc):
        return F32(F32(F64(int(raw)) * 2.0 ** -32) / nppc)

    def volv(raw, nppc, k):
        return F32((F64(int(raw)) * 2.0 ** -32) / ((F64(nppc) * (g.ze[k + 1] - g.ze[k])) * 1000.0))

    def tree(vals):
        red = [F32(0)] * 256
        for t in range(256):
            s = F32(0)
            for c in range(t, ncol, 256):
                s = F32(s + vals(c))
            red[t] = s
        o = 128
        while o > 0:
            for t in range(o):
                red[t] = F32(red[t] + red[t + o])
            o //= 2
        return F32(red[0] / F32(ncol))

    def fold(xs, ns, off):
        s1, s2 = F64(0), F64(0)
        for x, n in zip(xs, ns):
            s1 = s1 + F64(x) * F64(n)
            s2 = s2 + F64(n) * (F64(x) * F64(x))
        mom[8 + off] += s1
        mom[8 + M + off] += s2
        last[off] = xs[-1]

    for b0 in range(0, len(slabs), round_size):
        nb = min(round_size, len(slabs) - b0)
        total = ppb * nb
        ns = [min(total - b * ppb, ppb) for b in range(nb)]
        sl = [slabs[b0 + b] for b in range(nb)]
        # the columns part, then its mean_fold
        for q in range(3):
            for col in range(ncol):
                xs = []
                for b in range(nb):
                    raw = sl[b][q * ncol + col] if q < 2 else sum(int(sl[b][2 * ncol + col + ncol * k]) for k in range(nz))
                    xs.append(cv(raw, nppc_of(col, ns[b])))
                fold(xs, ns, 3 + q * ncol + col)
        # the volume part (cell_fold, volume_value)
        for v in range(nvox):
            col, k = v % ncol, v // ncol
            fold([volv(sl[b][2 * ncol + v], nppc_of(col, ns[b]), k) for b in range(nb)], ns, 3 + 3 * ncol + nz + v)
        # the flux means and the profile (batch_mean), then the scalars' mean_fold
        for q in range(3 + nz):
            xs = []
            for b in range(nb):
                if q < 3:
                    def val(c, b=b, q=q):
                        raw = sl[b][q * ncol + c] if q < 2 else sum(int(sl[b][2 * ncol + c + ncol * k]) for k in range(nz))
                        return cv(raw, nppc_of(c, ns[b]))
                else:
                    def val(c, b=b, k=q - 3):
                        return volv(sl[b][2 * ncol + ncol * k + c], nppc_of(c, ns[b]), k)
                xs.append(tree(val))
            fold(xs, ns, q if q < 3 else 3 + 3 * ncol + (q - 3))
        # the intensity part (bin_fold)
        for v in range(ncol * nDir):
            col = v % ncol
            fold([cv(sl[b][2 * ncol + nvox + v], nppc_of(col, ns[b])) for b in range(nb)], ns, 3 + 3 * ncol + nz + nvox + v)
        # the order bins (bin_fold)
        for e in range((2 + nDir) * ncol * nOrd):
            col = e % ncol
            off = base + 2 * nOrd + (e if e < 2 * ncol * nOrd else e + nDir * nOrd)
            fold([cv(sl[b][S + e], nppc_of(col, ns[b])) for b in range(nb)], ns, off)
        # the order means (batch_mean), then their mean_fold
        for m in range((2 + nDir) * nOrd):
            xs = [tree(lambda c, b=b: cv(sl[b][S + ncol * m + c], nppc_of(c, ns[b]))) for b in range(nb)]
            fold(xs, ns, base + (m if m < 2 * nOrd else 2 * nOrd + 2 * ncol * nOrd + (m - 2 * nOrd)))
        mom[0] += F64(total)
        mom[1] += F64(nb)
    return mom, last


def _grid(nx, ny, nz, regular, nDir=0, nOrd=0, seed=0):
    rng = np.random.default_rng(seed)
    if regular:
        xe, ye = 0.125 * np.arange(nx + 1), 0.25 * np.arange(ny + 1)
    else:
        xe = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.2, nx))])
        ye = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.2, ny))])
    ze = np.concatenate([[0.0], np.cumsum(rng.uniform(0.01, 0.1, nz))])
    return E.Grid(xe, ye, ze, nDir, nOrd)


def _slabs(g, nb, ppb, seed):
    """Random tallies of the size a batch of ppb photons can leave (up to ppb weights in a bin, fractional weights)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, ppb * 2 ** 32, (nb, g.S), dtype=np.int64)
    s[rng.random(s.shape) < 0.3] = 0
    return s


@pytest.mark.parametrize("nx,ny,nz,regular,nDir,nOrd,nb,ppb,rounds", [
    (1, 1, 1, True, 0, 0, 1, 1, 1),
    (3, 2, 2, True, 1, 2, 5, 7, 2),
    (5, 1, 3, False, 0, 0, 4, 13, 3),
    (4, 3, 2, False, 2, 1, 3, 1000003, 1),
    (260, 1, 1, True, 0, 1, 2, 11, 1),     # ncol > 256: the tree's lanes take two columns
    (13, 20, 1, False, 1, 0, 3, 5, 2),
])
def test_mirror_matches_literal_restatement(nx, ny, nz, regular, nDir, nOrd, nb, ppb, rounds):
    g = _grid(nx, ny, nz, regular, nDir, nOrd, seed=nx * 7 + ny)
    assert g.regular == regular
    first, second = _slabs(g, nb, ppb, 1), _slabs(g, nb + 1, ppb, 2)
    mom, last = E.epilogue(g, first, ppb, rounds)
    ref_mom, ref_last = literal_epilogue(g, list(first), ppb, rounds)
    assert np.array_equal(mom, ref_mom) and np.array_equal(last, ref_last)
    # a second call adds to the moments and overwrites `last`
    mom, last = E.epilogue(g, second, ppb, rounds, mom, last)
    ref_mom, ref_last = literal_epilogue(g, list(second), ppb, rounds, ref_mom, ref_last)
    assert np.array_equal(mom, ref_mom) and np.array_equal(last, ref_last)


def test_mirror_by_hand():
    """One column, one layer, four photons: three out of the top, one absorbed half way up a 0.5 km layer."""
    g = E.Grid([0.0, 1.0], [0.0, 1.0], [0.0, 0.5])
    slab = np.array([[3 << 32, 0, 1 << 32]], np.int64)
    mom, last = E.epilogue(g, slab, 4, 1)
    assert last[0] == F32(0.75) and last[1] == 0 and last[2] == F32(0.25)
    assert last[6] == F32(0.25 / 0.5 / 1000.0) and last[7] == last[6]  # profile and volume: weight / (n dz 1000)
    assert mom[0] == 4 and mom[1] == 1
    assert mom[8 + 0] == 0.75 * 4 and mom[8 + g.M + 0] == 4 * 0.75 ** 2


def test_mirror_rounds_and_tree_shape():
    """The launch-round grouping and the tree are visible in the bits: a different grouping or a sequential sum gives
    different moments on inputs made to round differently."""
    g = _grid(300, 1, 2, True, seed=5)
    s = _slabs(g, 7, 3, 9)
    a = E.epilogue(g, s, 3, 7)[0]
    b = E.epilogue(g, s, 3, 3)[0]
    assert not np.array_equal(a, b)
    assert np.array_equal(a[:2], b[:2])
    v = np.random.default_rng(1).random(1000).astype(F32) * F32(1e-3) + F32(1)
    assert E.tree_mean(v) != E.sequential_mean(v)


def test_xy_regular_and_areas():
    assert E.xy_regular(0.125 * np.arange(11), [0.0, 0.5])
    assert not E.xy_regular(0.1 * np.arange(11), [0.0, 0.5])  # (0.1 is no float: its float32 spacing is off by more than 2 ulp)
    assert not E.xy_regular([0.0, 0.1, 0.25], [0.0, 1.0])
    a = E.relative_areas([0.0, 1.0, 3.0], [0.0, 2.0])
    assert a.dtype == F32 and a.tolist() == [F32(1 / 3), F32(2 / 3)]
