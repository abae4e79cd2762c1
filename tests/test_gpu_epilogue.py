"""The epilogue of a call (finish_gather / finish_fold / finish_excess) held bit for bit to the host mirror of
tests/epilogue_mirror.py, with no tolerance anywhere.

1. Exact end to end from per-photon fates.  Over a black surface, with one component and every cell's single-scattering
   albedo exactly 0 or 1, a photon keeps weight 1.0 until it collides in an ssa = 0 cell; that collision deposits
   weight_to_fixed(1) = 2^32 in the cell and kills the photon (fate 2 at (ix, iy, iz)).  A top exit (fate 0) adds 2^32 to
   fluxUp(ix, iy), a surface arrival (fate 1) to fluxDown(ix, iy); the bins by scattering order get the same 2^32 at the
   order the photon has (the fate's nScatter; a surface arrival's record is taken after the reflection's increment).  So
   traceFates of the job's photon ids gives every batch's integer slab, and the mirror gives the moment array and the
   `last` array the production computeRadiativeTransfer must have produced.
2. Fold consistency for what fates cannot rebuild (radiance, fractional albedos, reflecting and per-patch surfaces,
   limitIntensityContributions, thermal emission): one call of nb batches must equal the fold of nb one-batch calls at the
   matching firstPhotonId, launch rounds mirrored; every one-batch call's domain means are the mirror's float tree over
   that batch's column values.  The level, direct / diffuse, actinic and side tails (DESIGN.md sections 4.12 to 4.15) are held
   the same way on the face-by-face plans: each tail is [means | bins], and a batch's means are the float tree over its bins.
3. The tally capacity: 2^31 - 1 photons into one bin give exactly 1.0; 2^31 is refused."""
import numpy as np
import pytest

from tests import cases
from tests import epilogue_mirror as E

pytestmark = pytest.mark.gpu

SEED = 20261016
F32 = np.float32


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _edges(n, size, regular, rng):
    if regular:
        return (size / n) * np.arange(n + 1) if n & (n - 1) == 0 else 0.0625 * np.arange(n + 1)
    d = rng.uniform(0.5, 1.5, n)
    return np.concatenate([[0.0], np.cumsum(d * (size / d.sum()))])


def binary_case(nx, ny, nz, regular, seed, height=0.5, absorbing=0.35):
    """One component over a black surface, every cell's albedo exactly 0 or 1, column optical depths of about 0.5 to 3,
    so that every fate (top exit, surface arrival, absorption) happens in many cells."""
    rng = np.random.default_rng(seed)
    xe, ye = _edges(nx, 0.5, regular, rng), _edges(ny, 0.5, regular, rng)
    ze = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, nz))])
    ze *= height / ze[-1]
    ext = rng.uniform(0.5, 3.0, (nx, ny, 1)) / height * rng.uniform(0.2, 1.8, (nx, ny, nz))
    ext[rng.random(ext.shape) < 0.1] = 0.0  # some clear cells
    ssa = np.where(rng.random(ext.shape) < absorbing, 0.0, 1.0)
    return dict(name="binary%dx%dx%d" % (nx, ny, nz), xe=xe, ye=ye, ze=ze, albedo=0.0,
                components=[dict(ext=ext, ssa=ssa, pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=[cases.hg_legendre(0.8, 16)])])


def _grid(case, nDir=0, nOrd=0):
    return E.Grid(case["xe"], case["ye"], case["ze"], nDir, nOrd)


def _round_size(g, nb, k):
    """The library's batches in flight: its 4 GiB slab budget (never binding here), maxBatchesInFlight when > 0, nb."""
    assert g.S * 8 * nb < 4 << 30
    return min(k, nb) if k > 0 else nb


def slabs_from_fates(g, fates, ppb, nb):
    """[nb, g.S] integer tallies of consecutive batches of ppb photons from their fates (see the module's docstring)."""
    f = fates["fate"].astype(np.int64)
    assert f.size == ppb * nb
    assert np.all((f >= 0) & (f <= 2)), "fates other than top / surface / absorbed: %r" % np.unique(f)
    assert np.all(fates["weight"][f < 2] == 1.0), "a photon left with a weight other than 1"
    ncol = g.ncol
    col = (fates["ix"].astype(np.int64) - 1) + g.nx * (fates["iy"].astype(np.int64) - 1)
    idx = np.where(f == 0, col, np.where(f == 1, ncol + col, 2 * ncol + col + ncol * (fates["iz"].astype(np.int64) - 1)))
    if g.nOrd:  # order bins: [up ncol nOrd | down ncol nOrd], order slowest
        order = fates["nScatter"].astype(np.int64) - (f == 1)
        oidx = g.slabOrders + np.where(f == 0, 0, ncol * g.nOrd) + ncol * order + col
        keep = (f < 2) & (order <= g.nOrd - 1)
    batch = np.arange(f.size, dtype=np.int64) // ppb
    flat = np.bincount(batch * g.S + idx, minlength=nb * g.S)
    if g.nOrd:
        flat = flat + np.bincount((batch * g.S + oidx)[keep], minlength=nb * g.S)
    return flat.reshape(nb, g.S).astype(np.int64) << 32


def _parts(g):
    """(name, start, length) of the moment array's parts, for messages."""
    ncol, nz, nvox = g.ncol, g.nz, g.nvox
    out = [("means", 0, 3), ("fluxUp", 3, ncol), ("fluxDown", 3 + ncol, ncol), ("fluxAbsorbed", 3 + 2 * ncol, ncol),
           ("profile", 3 + 3 * ncol, nz), ("volume", 3 + 3 * ncol + nz, nvox), ("intensity", 3 + 3 * ncol + nz + nvox, g.nDir * ncol)]
    if g.nOrd:
        no = g.nOrd
        out += [("meanByOrd", g.base, 2 * no), ("upDownByOrd", g.base + 2 * no, 2 * ncol * no),
                ("intensityByOrd", g.base + 2 * no + 2 * ncol * no, g.nDir * no * (1 + ncol))]
    for name, s, rows in getattr(g, "tails", ()):
        out += [(name + " means", s, rows), (name + " bins", s + rows, rows * ncol)]
    return out


def _where_differs(g, got, want, fates=None, ppb=None):
    """A message naming the differing parts of a moment array (S1 / S2), and the photons whose fates ended in the first
    differing column (so that a photon the production and the instrumented kernels trace differently is named by id)."""
    msg = []
    for half, o in (("S1", 8), ("S2", 8 + g.M)):
        for name, s, n in _parts(g):
            bad = np.nonzero(got[o + s:o + s + n] != want[o + s:o + s + n])[0]
            if bad.size:
                msg.append("%s %s: %d of %d differ, first at %d (%r vs %r)" % (half, name, bad.size, n, bad[0],
                                                                              got[o + s + bad[0]], want[o + s + bad[0]]))
                if fates is not None and name in ("fluxUp", "fluxDown", "fluxAbsorbed", "volume") and len(msg) == 1:
                    col = int(bad[0]) % g.ncol
                    hit = (fates["ix"] - 1) + g.nx * (fates["iy"] - 1) == col
                    msg.append("photons (index in the job) that ended in column %d: %r" % (col, np.nonzero(hit)[0][:20].tolist()))
    if not np.array_equal(got[:8], want[:8]):
        msg.append("header %r vs %r" % (got[:8].tolist(), want[:8].tolist()))
    return "; ".join(msg)


def _check_report(g, res, last):
    """reportResults() is the `last` array: the last batch's normalised values."""
    nx, ny, nz, ncol = g.nx, g.ny, g.nz, g.ncol
    f2 = lambda a: a.reshape(ny, nx).T  # noqa: E731
    assert np.array_equal(np.array([res["meanFluxUp"], res["meanFluxDown"], res["meanFluxAbsorbed"]], F32), last[:3])
    for i, k in enumerate(("fluxUp", "fluxDown", "fluxAbsorbed")):
        assert np.array_equal(res[k], f2(last[3 + i * ncol:3 + (i + 1) * ncol])), k
    assert np.array_equal(res["absorbedProfile"], last[3 + 3 * ncol:3 + 3 * ncol + nz])
    assert np.array_equal(res["volumeAbsorption"], last[3 + 3 * ncol + nz:3 + 3 * ncol + nz + g.nvox].reshape(nz, ny, nx).transpose(2, 1, 0))
    if g.nOrd:
        no, b = g.nOrd, g.base
        assert np.array_equal(res["meanFluxUpByScatOrd"], last[b:b + no])
        assert np.array_equal(res["meanFluxDownByScatOrd"], last[b + no:b + 2 * no])
        o = b + 2 * no
        assert np.array_equal(res["fluxUpByScatOrd"], last[o:o + ncol * no].reshape(no, ny, nx).transpose(2, 1, 0))
        assert np.array_equal(res["fluxDownByScatOrd"], last[o + ncol * no:o + 2 * ncol * no].reshape(no, ny, nx).transpose(2, 1, 0))
    if g.nDir:
        i0 = 3 + 3 * ncol + nz + g.nvox
        inten = last[i0:i0 + g.nDir * ncol].reshape(g.nDir, ncol)
        assert np.array_equal(res["intensity"], inten.reshape(g.nDir, ny, nx).transpose(2, 1, 0))
        assert np.array_equal(res["meanIntensity"], E.sequential_mean(inten))


# ---- 1. exact, from per-photon fates -------------------------------------------------------------------------------------
# The plans (tests/test_gpu_tunings.py): face by face with tallies private to a workgroup in LDS (privateTallies=1) or in
# global memory (0: the deposit-combining path), bricked grids, layer skipping, the block walk, the wide plan (4/5/6).
FACE_PRIV = dict(layerSkip=0, blockWalk=0, privateTallies=1, brickLayout=0)
FACE_GLOBAL = dict(layerSkip=0, blockWalk=0, privateTallies=0, brickLayout=0)
FACE_BRICKS = dict(layerSkip=0, blockWalk=0, privateTallies=0, brickLayout=1)
LAYERS = dict(layerSkip=3, blockWalk=0, privateTallies=0, brickLayout=0)
BLOCK = dict(blockWalk=2)
WIDE_FACE = dict(layerSkip=0, blockWalk=0, privateTallies=4, blockSize=0, brickLayout=0)
WIDE_LAYERS = dict(layerSkip=2, blockWalk=0, privateTallies=5, brickLayout=0)
WIDE_BLOCK = dict(blockWalk=2, privateTallies=6)

# id, (nx, ny, nz, regular), ppb, nb, maxBatchesInFlight, calls, first photon id, tuning, walkMode() expected, orders
FATE_CASES = [
    ("ncol1-tall", (1, 1, 160, True), 3001, 129, 3, 1, 0, FACE_PRIV, dict(privateTallies=True, blockWalk=False), 0),
    ("ncol255-ny1-block", (255, 1, 4, True), 1537, 65, 64, 1, 0, BLOCK, dict(blockWalk=True), 0),
    ("ncol256-irregular-global", (16, 16, 3, False), 999, 64, 0, 1, 12345, FACE_GLOBAL, dict(privateTallies=False, blockWalk=False), 0),
    ("ncol257-layers", (257, 1, 3, False), 2049, 63, 1, 1, 0, LAYERS, dict(layerSkip=True, blockWalk=False), 0),
    ("ncol1000-wide", (40, 25, 5, True), 600001, 1, 64, 1, 0, WIDE_FACE, dict(widePlan=True), 0),
    ("nz1-bricks-id-beyond-2^32", (20, 13, 1, False), 333, 129, 64, 1, 3 << 32, FACE_BRICKS, dict(blockWalk=False), 0),
    ("two-calls-wide-block", (12, 12, 8, True), 1000, 65, 64, 2, 7, WIDE_BLOCK, dict(blockWalk=True, widePlan=True), 0),
    ("two-calls-wide-layers", (30, 7, 6, False), 777, 65, 3, 2, 0, WIDE_LAYERS, dict(widePlan=True, layerSkip=True), 0),
    ("orders-rounds", (24, 11, 6, False), 1501, 65, 3, 1, 0, dict(layerSkip=0, blockWalk=0), dict(blockWalk=False), 3),
    ("orders-ncol260", (260, 1, 2, True), 1003, 64, 64, 2, 1 << 33, dict(layerSkip=3, blockWalk=0), dict(layerSkip=True), 2),
]


@pytest.mark.timeout(240, method="thread")
@pytest.mark.parametrize("cid,dims,ppb,nb,k,calls,first,tuning,mode,nOrdRec", FATE_CASES, ids=[c[0] for c in FATE_CASES])
def test_moments_from_fates_bitwise(M, cid, dims, ppb, nb, k, calls, first, tuning, mode, nOrdRec):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    nx, ny, nz, regular = dims
    assert ppb * nb * calls <= 1_100_000
    case = binary_case(nx, ny, nz, regular, seed=nx * 1000 + ny * 10 + nz)
    g = _grid(case, nOrd=nOrdRec + 1 if nOrdRec else 0)
    assert g.regular == regular and g.ncol == nx * ny
    mu0, phi0 = (1.0, 0.0) if nx * ny == 1 else (0.7, 35.0)
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    try:
        integ.specifyParameters(minInverseTableSize=2001, useRayTracing=True, useRussianRoulette=True)
        integ.setTuning(**{**tuning, "maxBatchesInFlight": k})
        photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
        fates = integ.traceFates(dom, new_RandomNumberSequence(SEED, first), photons, ppb * nb * calls)
        if nOrdRec:  # (the instrumented kernels carry no order tallies: fates first, then the orders on)
            integ.specifyParameters(recScatOrd=True, numRecScatOrd=nOrdRec)
        got_mode = integ.walkMode()
        assert all(got_mode[key] == v for key, v in mode.items()), (cid, got_mode)
        rng = new_RandomNumberSequence(SEED, first)
        mom = last = None
        for c in range(calls):  # consecutive calls, no resetMoments: each adds to the moments
            done = integ.computeRadiativeTransfer(dom, rng, photons, ppb, nb)
            assert done == ppb * nb
            part = fates[c * ppb * nb:(c + 1) * ppb * nb]
            mom, last = E.epilogue(g, slabs_from_fates(g, part, ppb, nb), ppb, _round_size(g, nb, k), mom, last)
        assert rng.nextPhotonId == first + calls * ppb * nb
        got = integ.moments()
        assert got.shape == mom.shape
        assert np.array_equal(got, mom), "%s: %s" % (cid, _where_differs(g, got, mom, fates, ppb))
        _check_report(g, integ.reportResults(), last)
        # (the cases are not degenerate: every fate happens)
        assert all(np.any(fates["fate"] == q) for q in (0, 1, 2)) or nx * ny == 1
    finally:
        integ.finalize()


# ---- 2. fold consistency: what fates cannot rebuild ----------------------------------------------------------------------
# The tallies of the face-by-face plans, in the only combinations the refusal rules (mcbrat_variants.h) allow that between them reach
# every level, actinic and side part of the epilogue.
FACE_KINDS = {"levels-direct": dict(recLevelFluxes=True, recDirectLevelFluxes=True),
              "levels-side": dict(recLevelFluxes=True, recSideFluxes=True),
              "levels-actinic": dict(recLevelFluxes=True, recActinicFlux=True)}


def _tails(g, kw):
    """-> ([(name, start, rows)], end) of the moment tails behind the mirror's parts, each [means rows | bins rows ncol] in the
    order of mcbrat_layout.h: levels (up, down by level), direct (direct, diffuse by level), actinic (by layer), side (four parts
    by layer)."""
    rows = [(name, n) for name, key, n in (("levels", "recLevelFluxes", 2 * (g.nz + 1)), ("direct", "recDirectLevelFluxes", 2 * (g.nz + 1)),
                                           ("actinic", "recActinicFlux", g.nz), ("side", "recSideFluxes", 4 * g.nz)) if kw.get(key)]
    out, at = [], g.base
    for name, n in rows:
        out.append((name, at, n))
        at += n * (1 + g.ncol)
    return out, at


def _fold_case(kind):
    """(case, specifyParameters keywords, source) of a domain the fates cannot rebuild."""
    if kind == "thermal":
        case = cases.homog_lw(n=8, ext=6.0, ssa=0.6, albedo=0.2)
        return case, dict(LW_flag=1.0), "thermal"
    rng = np.random.default_rng(5)
    case = binary_case(20, 13, 6, False, seed=77)
    comp = case["components"][0]
    comp["ssa"] = rng.uniform(0.3, 0.999, comp["ext"].shape)   # fractional albedos
    comp["legendre"] = [cases.hg_legendre(0.85, 32)]
    case["albedo"] = 0.3                                        # a reflecting surface
    mus, phis = [1.0, 0.5, -0.3], [0.0, 45.0, 200.0]
    if kind in FACE_KINDS:
        return case, dict(FACE_KINDS[kind]), "solar"
    if kind == "radiance":
        return case, dict(intensityMus=mus[:2], intensityPhis=phis[:2], computeIntensity=True, minForwardTableSize=2001), "solar"
    if kind == "limit":
        return case, dict(intensityMus=mus[:2], intensityPhis=phis[:2], computeIntensity=True, minForwardTableSize=2001,
                          limitIntensityContributions=True, maxIntensityContribution=0.02), "solar"
    if kind == "orders-patches":
        case = cases.patchy_surface(case)
        return case, dict(intensityMus=mus, intensityPhis=phis, computeIntensity=True, minForwardTableSize=2001,
                          recScatOrd=True, numRecScatOrd=3), "solar"
    if kind == "orders-ncol300":
        big = binary_case(300, 1, 3, True, seed=3)
        big["components"][0]["ssa"] = np.full(big["components"][0]["ext"].shape, 0.95)
        big["albedo"] = 0.2
        return big, dict(intensityMus=mus[:1], intensityPhis=phis[:1], computeIntensity=True, minForwardTableSize=2001,
                         recScatOrd=True, numRecScatOrd=2), "solar"
    raise ValueError(kind)


def _fold_integrator(M, kind, k):
    case, kw, source = _fold_case(kind)
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    if source == "thermal":
        w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
        M.emission_weighting(dom, w, case["sfc_temp"])
        photons = M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12)
    else:
        photons = M.new_PhotonStream(0.6, 20.0, numberOfPhotons=10 ** 12)
    surf = cases.product_surface(case)
    if surf is not None:
        kw = dict(kw, surfaceBDRF=surf)
    integ.specifyParameters(minInverseTableSize=2001, useRayTracing=True, useRussianRoulette=True, **kw)
    integ.setTuning(maxBatchesInFlight=k)
    nDir = integ.numIntensityDirections()
    g = _grid(case, nDir, integ.numRecScatOrd + 1 if integ.numRecScatOrd >= 0 else 0)
    if kind in FACE_KINDS:  # the moments' length from the library: the mirror knows nothing of these tails
        integ.prepare(dom, photons)  # (the plan is that of the loaded domain)
        walk = integ.walkMode()
        assert not walk["blockWalk"] and not walk["layerSkip"] and not walk["widePlan"], walk
        g.tails, end = _tails(g, kw)
        g.M = (len(integ.moments()) - 8) // 2
        assert g.M == end and (g.ncol, g.nvox) == (260, 1560) and {t[0] for t in g.tails} == set(kind.split("-"))
    return integ, dom, photons, g


# kind, nb, maxBatchesInFlight
FOLD_CASES = [("radiance", 65, 3), ("radiance", 1, 64), ("limit", 129, 64), ("limit", 64, 1), ("orders-patches", 65, 64),
              ("orders-patches", 63, 3), ("orders-ncol300", 64, 3), ("thermal", 65, 64), ("thermal", 129, 1),
              ("levels-direct", 65, 3), ("levels-direct", 129, 64), ("levels-side", 65, 64), ("levels-side", 63, 3),
              ("levels-actinic", 129, 1), ("levels-actinic", 64, 64)]


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("kind,nb,k", FOLD_CASES, ids=["%s-nb%d-k%d" % c for c in FOLD_CASES])
def test_call_equals_fold_of_one_batch_calls(M, kind, nb, k):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    ppb, first = 1201, 5 << 32
    integ, dom, photons, g = _fold_integrator(M, kind, k)
    try:
        M_ = g.M
        vals = np.zeros((nb, M_), F32)
        for b in range(nb):
            integ.resetMoments()
            rng = new_RandomNumberSequence(SEED, first + b * ppb)
            assert integ.computeRadiativeTransfer(dom, rng, photons, ppb, 1) == ppb
            one = integ.moments()
            assert one[0] == ppb and one[1] == 1
            x = (one[8:8 + M_] / ppb).astype(F32)
            assert np.array_equal(x.astype(np.float64) * ppb, one[8:8 + M_]), "S1 / n is not a float: the recovery is not exact"
            assert np.array_equal(np.float64(ppb) * (x.astype(np.float64) * x), one[8 + M_:]), "S2 is not n x^2 of the same x"
            vals[b] = x
            # the batch's domain means and profile are the float tree over its column values
            ncol, nz = g.ncol, g.nz
            assert np.array_equal(x[:3], E.tree_mean(x[3:3 + 3 * ncol].reshape(3, ncol))), (kind, b)
            prof = x[3 + 3 * ncol:3 + 3 * ncol + nz]
            vol = x[3 + 3 * ncol + nz:3 + 3 * ncol + nz + g.nvox].reshape(nz, ncol)
            assert np.array_equal(prof, E.tree_mean(vol)), (kind, b)  # (the profile divides each voxel as the volume does)
            if g.nOrd:  # ... and so are the means by scattering order, over that batch's order bins
                no, base = g.nOrd, g.base
                bins = x[base + 2 * no:base + 2 * no + 2 * ncol * no].reshape(2 * no, ncol)
                assert np.array_equal(x[base:base + 2 * no], E.tree_mean(bins)), (kind, b)
                if g.nDir:
                    o = base + 2 * no + 2 * ncol * no
                    ibins = x[o + g.nDir * no:o + g.nDir * no + g.nDir * no * ncol].reshape(g.nDir * no, ncol)
                    assert np.array_equal(x[o:o + g.nDir * no], E.tree_mean(ibins)), (kind, b)
            for name, s, rows in getattr(g, "tails", ()):  # ... and every tail's means, over that batch's bins of the tail
                assert np.array_equal(x[s:s + rows], E.tree_mean(x[s + rows:s + rows * (1 + ncol)].reshape(rows, ncol))), (kind, b, name)
            if b == nb - 1:
                res = integ.reportResults()
                _check_report(g, res, x)
        for name, s, rows in getattr(g, "tails", ()):  # (the tails are not degenerate: most means are fed -- the diffuse light from above the top is not)
            assert np.count_nonzero(vals[:, s:s + rows].max(axis=0) > 0) >= rows - 1, (kind, name)
        integ.resetMoments()
        rng = new_RandomNumberSequence(SEED, first)
        assert integ.computeRadiativeTransfer(dom, rng, photons, ppb, nb) == ppb * nb
        got = integ.moments()
        want = E.fold_batch_values(g, vals, ppb, _round_size(g, nb, k))
        assert np.array_equal(got, want), "%s: %s" % (kind, _where_differs(g, got, want))
        _check_report(g, integ.reportResults(), vals[-1])
    finally:
        integ.finalize()


# ---- 3. the capacity of the tallies --------------------------------------------------------------------------------------
def _vacuum_column(M):
    case = dict(name="vacuum", xe=np.array([0.0, 1.0]), ye=np.array([0.0, 1.0]), ze=np.array([0.0, 1.0]), albedo=0.0,
                components=[dict(ext=np.zeros((1, 1, 1)), ssa=np.ones((1, 1, 1)), pfIndex=np.ones((1, 1, 1), np.int32),
                                 legendre=[cases.hg_legendre(0.5, 4)])])
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=2001, useRayTracing=True, useRussianRoulette=True)
    return integ, dom, M.new_PhotonStream(1.0, 0.0, numberOfPhotons=1 << 40)


def test_batch_larger_than_the_tallies_is_refused(M):
    """2^31 unit weights in one bin would be 2^63 units of 2^-32: the int64 wraps to -2^63 and the flux reads -1.0.  Refused
    before anything is traced; the context goes on working."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ, dom, photons = _vacuum_column(M)
    try:
        rng = new_RandomNumberSequence(SEED)
        with pytest.raises(M.McbratError, match="numPhotonsPerBatch is too large"):
            integ.computeRadiativeTransfer(dom, rng, photons, 1 << 31)
        assert rng.nextPhotonId == 0 and integ.moments()[0] == 0
        assert integ.computeRadiativeTransfer(dom, rng, photons, 1000, 3) == 3000
        res = integ.reportResults()
        assert res["meanFluxDown"] == 1.0 and res["meanFluxUp"] == 0.0
        assert integ.moments()[:2].tolist() == [3000.0, 3.0]
    finally:
        integ.finalize()


@pytest.mark.slow
@pytest.mark.timeout(600, method="thread")
def test_largest_batch_fills_one_bin_exactly(M):
    """2^31 - 1 one-leg photons straight down a vacuum column onto a black surface, all into one fluxDown bin: the bin holds
    2^63 - 2^32 and the flux is exactly 1.0, its standard error exactly 0."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from mcbrat3d_amd import driver
    integ, dom, photons = _vacuum_column(M)
    try:
        n = (1 << 31) - 1
        assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, n) == n
        res = integ.reportResults()
        assert res["fluxDown"][0, 0] == 1.0 and res["fluxUp"][0, 0] == 0.0 and res["meanFluxDown"] == 1.0
        assert res["meanFluxUp"] == 0.0 and res["meanFluxAbsorbed"] == 0.0
        st = driver.statistics(driver.unpack_moments(integ.moments(), 1, 1, 1))
        assert st["meanFluxDown"] == 1.0 and st["meanFluxDown_StdErr"] == 0.0 and st["fluxDown"][0, 0] == 1.0
        assert st["fluxDown_StdErr"][0, 0] == 0.0 and st["fluxUp"][0, 0] == 0.0
    finally:
        integ.finalize()
