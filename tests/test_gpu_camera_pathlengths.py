"""The backward camera's radiance by photon path length on the GPU: exact vacuum images (the whole pixel
in the one bin of its length, bit for bit the plain render's), the bins as a partition of the plain render, the equivalence
theorem against a render with a uniform absorber, bitwise determinism at the seams between pixels, the LDS share, refusals that
leave the context untouched.  `dropped` is 0 in every render here."""
import ctypes as C

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
SEED = 20261021
PI = np.pi
F32 = np.float32
DELTA = 1e-5   # sixteen times the 6.2e-7 section 4.19 measured for march()'s optical depth: L is the same float sum without the extinction
Z = 4.5        # the slab comparisons of tests/test_gpu_camera.py
# The 1-bin render against mcbrat_render_camera: float accumulation along a path against per-estimate fixed point.  Largest
# relative deviation of a pixel measured on the MI355X over the two cases of check 2 (two cameras each), the two seam cases and
# the 2 x 2 x 2 context of the refusal test: 1.19e-7 (0 / 1.06e-7, 9.4e-8 / 0, 1.19e-7, 1.06e-7, 4.6e-8) -- one unit in the last
# place of the float outputs; times 4 for other compilers (the convention of section 4.19).  1e-4 would be a bug.
PLAIN_MEASURED = 1.2e-7
PLAIN_RTOL = 4.0 * PLAIN_MEASURED


def _integrator(case, mu0, phi0, surface=None, tables=2001, fwd=1801):
    import mcbrat3d_amd as M
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=tables, minForwardTableSize=fwd, useRayTracing=True, useRussianRoulette=True, surfaceBDRF=surface)
    integ.prepare(dom, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12))
    return integ


def _plain(integ, cam, spp, batches=1, seed=SEED, first=0):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderCamera(cam, new_RandomNumberSequence(seed, first), spp, batches)
    assert out["dropped"] == 0
    return out


def _bylen(integ, cam, edges, spp, batches=1, seed=SEED, first=0):
    out = integ.renderCameraPathLengths(cam, edges, spp, numBatches=batches, seed=seed, firstSample=first)
    assert out["dropped"] == 0
    assert out["radiance"].shape == (len(edges), cam.npy, cam.npx) and out["batchMeans"].shape == (batches, len(edges), cam.npy, cam.npx)
    return out


def _ortho(npx=1, npy=1, mu=1.0, phi=0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("orthographic", npx=npx, npy=npy, mu=mu, phi=phi, footprint=footprint, height=height, **kw)


def _pinhole(npx, npy, position, look, up=(0.0, 1.0, 0.0), fov=60.0, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=npx, npy=npy, position=position, look=look, up=up, fov=fov, **kw)


def _vacuum(albedo=0.3):
    from tests.test_gpu_camera import VAC, _medium
    return _medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=albedo)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. vacuum over a Lambertian surface: exact
# ---------------------------------------------------------------------------------------------------------------------------------
H, MU0, PHI0 = 0.25, 0.5, 30.0


def _four_edges(L):
    return np.array([0.0, L * (1.0 - DELTA), L * (1.0 + DELTA), 2.0 * L], F32)


@pytest.mark.parametrize("height", [0.25, 0.11])
@pytest.mark.parametrize("mu", [1.0, 0.4, 0.05])
def test_vacuum_the_whole_pixel_lies_in_the_bin_of_its_length(mu, height):
    a = 0.3
    integ = _integrator(_vacuum(a), MU0, PHI0, tables=101, fwd=181)
    cam = _ortho(3, 2, mu, 110.0, height=height)          # jitter on; at 0.05 a ray crosses the 0.5 wide domain up to ten times
    L = height / float(F32(mu)) + H / MU0
    edges = _four_edges(L)
    assert edges[1] < L < edges[2]
    plain, out = _plain(integ, cam, 197, 2), _bylen(integ, cam, edges, 197, 2)
    integ.finalize()
    rad, err = out["radiance"], out["radiance_StdErr"]
    assert rad[1].tobytes() == plain["radiance"].tobytes()
    assert np.all(np.abs(rad[1].astype(np.float64) - a / PI) <= (a / PI) * 2.0 ** -22 + 2.0 ** -31), rad[1]
    assert np.all(err == 0.0) and np.all(plain["radiance_StdErr"] == 0.0)
    assert np.all(rad[[0, 2, 3]] == 0.0), rad


def test_vacuum_a_camera_looking_up_sees_nothing_in_any_bin():
    integ = _integrator(_vacuum(), MU0, PHI0, tables=101, fwd=181)
    out = _bylen(integ, _ortho(2, 2, -0.7, 250.0, height=0.0), _four_edges(1.0), 197, 2)
    integ.finalize()
    assert np.all(out["radiance"] == 0.0) and np.all(out["radiance_StdErr"] == 0.0) and np.all(out["batchMeans"] == 0.0)


def test_vacuum_a_pinhole_puts_every_pixel_in_the_bin_of_its_own_length():
    a, z = 0.3, 0.11
    integ = _integrator(_vacuum(a), MU0, PHI0, tables=101, fwd=181)
    cam = _pinhole(3, 2, (0.1, 0.2, z), (0.5, -0.3, -1.0), up=(0.1, 1.0, 0.0), fov=90.0, jitter=False)
    Lp = np.zeros((cam.npy, cam.npx))
    for j in range(cam.npy):
        for i in range(cam.npx):
            _, d = cam.ray(i, j)
            assert d[2] < -0.1
            Lp[j, i] = z * np.linalg.norm(d) / -d[2] + H / MU0
    assert len(set(np.round(Lp.ravel(), 6))) == Lp.size   # an asymmetric look: no two pixels share a length
    L_max = 0.79                                          # a bound on these pixels' lengths (0.61 .. 0.78), off their multiples
    assert Lp.max() < L_max
    edges = (2.0 * L_max / 64.0 * np.arange(64)).astype(F32)
    want = np.searchsorted(edges, Lp.ravel(), "right").reshape(Lp.shape) - 1
    assert len(set(want.ravel())) >= 3
    # the condition on this test's own design: no length within DELTA of an edge, so no pixel is left out below
    assert np.all(np.abs(Lp[..., None] - edges.astype(np.float64)) > DELTA * Lp[..., None])
    plain, out = _plain(integ, cam, 64, 2), _bylen(integ, cam, edges, 64, 2)
    integ.finalize()
    expected = np.zeros((64, cam.npy, cam.npx), F32)
    for j in range(cam.npy):
        for i in range(cam.npx):
            expected[want[j, i], j, i] = plain["radiance"][j, i]
    assert np.all(plain["radiance"] > 0.9 * a / PI)
    assert out["radiance"].tobytes() == expected.tobytes()
    assert np.all(out["radiance_StdErr"] == 0.0)


def test_vacuum_periodic_wraps_over_a_checkerboard_do_not_disturb_the_length():
    import mcbrat3d_amd as M
    refl = np.array([[0.1, 0.8], [0.6, 0.25]], F32)
    surface = M.new_SurfaceDescription(refl[None], np.array([0.0, 0.25, 0.5]), np.array([0.0, 0.2, 0.5]))
    integ = _integrator(_vacuum(0.0), MU0, PHI0, surface=surface, tables=101, fwd=181)
    mu, z = 0.05, 0.25
    cam = _ortho(3, 2, mu, 110.0, height=z)
    edges = _four_edges(z / float(F32(mu)) + H / MU0)
    plain, out = _plain(integ, cam, 197, 2), _bylen(integ, cam, edges, 197, 2)
    integ.finalize()
    assert out["radiance"][1].tobytes() == plain["radiance"].tobytes() and out["radiance_StdErr"][1].tobytes() == plain["radiance_StdErr"].tobytes()
    assert out["batchMeans"][:, 1].tobytes() == plain["batchMeans"].tobytes()
    assert np.all(out["radiance"][[0, 2, 3]] == 0.0)
    # the pixels meet different patches, ten domain widths away
    assert np.all(plain["radiance"] >= F32(0.1 / PI) * F32(0.999)) and len(set(plain["radiance"].ravel())) > 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the bins partition the plain render
# ---------------------------------------------------------------------------------------------------------------------------------
EDGES = {1: np.array([0.0], F32), 7: np.array([0.0, 0.3, 0.5, 0.7, 1.0, 1.5, 3.0], F32), 256: (4.0 / 256.0 * np.arange(256)).astype(F32)}


def _partition(integ, cam, spp, batches, label):
    """check 2 for one (integrator, camera, sample range) -> the largest relative deviation of the 1-bin render from the plain one"""
    plain = _plain(integ, cam, spp, batches)["radiance"].astype(np.float64)
    outs = {n: _bylen(integ, cam, e, spp, batches) for n, e in EDGES.items()}
    sums = {n: o["radiance"].astype(np.float64).sum(axis=0) for n, o in outs.items()}
    for n in (7, 256):
        # the integer tallies behind the sums are equal by construction: what differs is the float rounding of n outputs
        assert np.all(np.abs(sums[n] - sums[1]) <= n * 2.0 ** -24 * sums[1]), (label, n, sums[n], sums[1])
        assert (outs[n]["radiance"] > 0).any(axis=(1, 2)).sum() >= 3, (label, n)   # the light is spread over the bins
    one = sums[1]
    assert np.all(one[plain == 0.0] == 0.0)
    dev = float(np.max(np.abs(one - plain)[plain > 0] / plain[plain > 0])) if (plain > 0).any() else 0.0
    print("path lengths, %s: 1 bin against the plain render, largest relative deviation of a pixel %.3g" % (label, dev))
    assert dev < 1e-4, (label, dev)   # (more than that is a bug, not rounding)
    assert dev <= PLAIN_RTOL, (label, dev)
    return dev


def _step_cloud():
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    return case


def test_the_bins_partition_the_plain_render_on_the_step_cloud():
    integ = _integrator(_step_cloud(), 0.5, 30.0)
    _partition(integ, _ortho(8, 1, 0.8, 20.0), 2048, 2, "step cloud, from the top")
    _partition(integ, _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0), 2048, 2, "step cloud, sky imager inside")
    integ.finalize()


def test_the_bins_partition_the_plain_render_on_the_small_domain():
    from tests.test_gpu_camera import small_domain
    case = small_domain()
    integ = _integrator(case, 0.5, 30.0, surface=cases.product_surface(case), tables=9001)
    _partition(integ, _ortho(4, 3, 0.6, 110.0, footprint=(0.0, 0.5, 0.0, 0.3), height=0.2), 2048, 2, "small domain, from the top")
    _partition(integ, _pinhole(3, 2, (0.2, 0.15, 0.1), (0.3, 0.2, -1.0), fov=80.0), 2048, 2, "small domain, inside")
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the equivalence theorem: a render without the absorber gives the radiance with it
# ---------------------------------------------------------------------------------------------------------------------------------
# The values chosen: the small domain with its extinction times 0.3 (optical depth about 0.5 on
# average), k = 1 per km -- k H / mu0 = 0.4 --, 256 edges 4 / 255 km apart up to 4 km: k dL = 1.6 %, the open bin beyond 4 km.
K_ABS, THIN, L_OPEN = 1.0, 0.3, 4.0


def _thin_domain(absorber):
    from tests.test_gpu_camera import small_domain
    case = small_domain()
    comps = []
    for comp in case["components"]:
        comps.append(dict(comp, ext=comp["ext"] * THIN))
    if absorber:
        ext = np.full(comps[0]["ext"].shape, K_ABS)
        comps.append(dict(ext=ext, ssa=np.zeros_like(ext), pfIndex=np.ones(ext.shape, np.int32), legendre=[cases.hg_legendre(0.0, 2)]))
    case["components"] = comps
    return case


def _series(batch_values):
    """(mean, standard error of the mean) of a series of batch values [batch, ...]"""
    v = np.asarray(batch_values, np.float64)
    return v.mean(axis=0), v.std(axis=0, ddof=1) / np.sqrt(v.shape[0])


def test_the_equivalence_theorem_against_a_render_with_the_absorber():
    from mcbrat3d_amd.camera import absorbed_radiance
    h, mu0 = 0.2, 0.5
    edges = (L_OPEN / 255.0 * np.arange(256)).astype(F32)
    assert K_ABS * h / mu0 >= 0.25   # an estimator that forgot the sun ray's length would be off by more than 20 %
    cams = {"from the top": _ortho(4, 3, 1.0, 0.0, footprint=(0.0, 0.5, 0.0, 0.3), height=h),
            "inside": _pinhole(3, 2, (0.2, 0.15, 0.1), (0.3, 0.2, -1.0), fov=80.0)}
    spp, nb = 8192, 16
    results = {}
    for absorber in (False, True):
        case = _thin_domain(absorber)
        integ = _integrator(case, mu0, 30.0, surface=cases.product_surface(case), tables=9001)
        for name, cam in cams.items():
            results[name, absorber] = (_bylen(integ, cam, edges, spp, nb, seed=SEED) if not absorber else _plain(integ, cam, spp, nb, seed=SEED + 1))
        integ.finalize()
    for name in cams:
        A, B = results[name, False], results[name, True]
        means = A["batchMeans"].astype(np.float64)                       # [batch, bin, y, x]
        brackets = [absorbed_radiance(m, edges, K_ABS) for m in means]
        lower, lower_err = _series([b[0] for b in brackets])
        upper, upper_err = _series([b[1] for b in brackets])
        IB, IB_err = _series(B["batchMeans"])
        # per pixel
        s_lo, s_up = np.sqrt(lower_err ** 2 + IB_err ** 2), np.sqrt(upper_err ** 2 + IB_err ** 2)
        assert np.all(lower - Z * s_lo <= IB) and np.all(IB <= upper + Z * s_up), (name, lower, IB, upper, s_lo)
        # the image mean, its three conditions, and the power to see a missing term
        lo_m, lo_e = _series([b[0].mean() for b in brackets])
        up_m, up_e = _series([b[1].mean() for b in brackets])
        ib_m, ib_e = _series(B["batchMeans"].astype(np.float64).mean(axis=(1, 2)))
        whole = A["radiance"].astype(np.float64)
        print("equivalence, %s: I_B %.6g +- %.2g in [%.6g, %.6g] (width %.2f %%), without the absorber %.6g, open bin %.3g of it" % (
            name, ib_m, ib_e, lo_m, up_m, 100 * (up_m - lo_m) / ib_m, whole.sum(axis=0).mean(), whole[-1].mean() / whole.sum(axis=0).mean()))
        assert up_m - lo_m <= 0.03 * ib_m, (name, lo_m, up_m, ib_m)
        assert whole[-1].mean() <= 0.01 * whole.sum(axis=0).mean(), name
        assert np.hypot(up_e, ib_e) < 0.01 * ib_m, (name, up_e, ib_e)
        assert lo_m - Z * np.hypot(lo_e, ib_e) <= ib_m <= up_m + Z * np.hypot(up_e, ib_e), (name, lo_m, ib_m, up_m)
        assert whole.sum(axis=0).mean() > 1.2 * ib_m, name               # the absorber takes more than the bracket is wide


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. determinism, and the seams between pixels
# ---------------------------------------------------------------------------------------------------------------------------------
def _sky(lds=-1):
    return _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)   # a sky imager inside the cloud


@pytest.mark.parametrize("spp", [1000, 7])   # not a multiple of 64: some waves span two pixels; below 64: every wave does
def test_bitwise_determinism_at_the_seams(spp):
    integ = _integrator(_step_cloud(), 0.5, 30.0)
    e = EDGES[7]
    two = _bylen(integ, _sky(), e, spp, 2)
    again = _bylen(integ, _sky(), e, spp, 2)
    for k in ("radiance", "radiance_StdErr", "batchMeans"):
        assert again[k].tobytes() == two[k].tobytes(), k                                   # two identical calls
        assert _bylen(integ, _sky(0), e, spp, 2)[k].tobytes() == _bylen(integ, _sky(1), e, spp, 2)[k].tobytes() == two[k].tobytes(), k
    first, second = _bylen(integ, _sky(), e, spp, 1, first=0), _bylen(integ, _sky(), e, spp, 1, first=spp)
    assert first["batchMeans"].tobytes() == two["batchMeans"][:1].tobytes() and second["batchMeans"].tobytes() == two["batchMeans"][1:].tobytes()
    # every deposit straight to global memory: the same integers
    integ.setOption(cameraPathBinsInLds=0)
    assert _bylen(integ, _sky(), e, spp, 2)["batchMeans"].tobytes() == two["batchMeans"].tobytes()
    integ.setOption(cameraPathBinsInLds=1)
    assert two["batchMeans"].std() > 0 and (two["radiance"] > 0).any(axis=(1, 2)).sum() >= 3
    _partition(integ, _sky(), spp, 2, "seams, %d samples per pixel" % spp)
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the LDS share
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_lds_share_counts_the_histograms_with_the_grid():
    """32 x 32 x 17 cells: 70304 bytes of grid and edges fit the share of 79 KB alone, not with the 17408 bytes of eight
    histograms of 256 bins and their edges; with 8 bins (544 bytes) they do."""
    from mcbrat3d_amd._capi import McbratError
    nx, ny, nz = 32, 32, 17
    assert 8 * (nx + ny + nz + 3) + 4 * nx * ny * nz <= 79 * 1024 < 8 * (nx + ny + nz + 3) + 4 * nx * ny * nz + 256 * (8 * 8 + 4)
    ext = np.random.default_rng(9).uniform(1.0, 9.0, (nx, ny, nz))
    case = dict(name="lds", xe=0.5 / nx * np.arange(nx + 1), ye=0.5 / ny * np.arange(ny + 1), ze=0.25 / nz * np.arange(nz + 1), albedo=0.2,
                components=[dict(ext=ext, ssa=np.full_like(ext, 0.95), pfIndex=np.ones(ext.shape, np.int32), legendre=[cases.hg_legendre(0.6, 32)])])
    integ = _integrator(case, 0.5, 30.0)
    cam = lambda lds: _ortho(4, 2, 0.7, 40.0, gridInLds=lds)   # noqa: E731
    wide, few = EDGES[256], (0.25 * np.arange(8)).astype(F32)
    assert _plain(integ, cam(1), 256, 2)["radiance"].min() > 0                         # the grid alone fits
    auto = _bylen(integ, cam(-1), wide, 256, 2)                                        # -1: renders, from global memory
    assert auto["batchMeans"].tobytes() == _bylen(integ, cam(0), wide, 256, 2)["batchMeans"].tobytes()
    with pytest.raises(McbratError, match="renderCameraPathLengths: gridInLds = 1.*path-length histograms do not fit the LDS share together"):
        _bylen(integ, cam(1), wide, 256, 2)
    placed = {lds: _bylen(integ, cam(lds), few, 256, 2) for lds in (-1, 0, 1)}         # both placements exist: bit for bit
    assert placed[0]["batchMeans"].tobytes() == placed[1]["batchMeans"].tobytes() == placed[-1]["batchMeans"].tobytes()
    a, b = auto["radiance"].astype(np.float64).sum(axis=0), placed[1]["radiance"].astype(np.float64).sum(axis=0)
    assert np.all(np.abs(a - b) <= 256 * 2.0 ** -24 * b) and np.all(b > 0)
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals, and a context left as it was
# ---------------------------------------------------------------------------------------------------------------------------------
OK_EDGES = np.array([0.0, 0.5, 2.0], F32)


def _call(ctx, cam, edges=OK_EDGES, nbins=None, spp=64, batches=1, n=4, rad=True):
    edges = None if edges is None else np.ascontiguousarray(edges, F32)
    nbins = (0 if edges is None else len(edges)) if nbins is None else nbins
    out = np.zeros(max(n, 1) * max(nbins, 1), F32) if rad else None
    rc = ctx.L.mcbrat_render_camera_pathlengths(ctx.ctx, C.addressof(cam) if cam is not None else None, nbins, ctx.ptr(edges), SEED, 0, spp, batches,
                                                ctx.ptr(out), None, None, None)
    return rc, (ctx.L.mcbrat_last_error(ctx.ctx).decode() if rc else ""), out


def _plain_call(ctx, cam, spp=256, batches=2):
    rad = np.zeros(4, F32)
    assert ctx.L.mcbrat_render_camera(ctx.ctx, C.addressof(cam), SEED, 0, spp, batches, ctx.ptr(rad), None, None, None) == 0
    return rad


def test_refusals_in_order_leave_the_context_untouched():
    from tests.test_gpu_camera import REFUSED_CAMERAS, _struct
    from tests.test_gpu_refusal_matrix import Context
    fresh = Context()
    _, reference = fresh.trace()
    fresh.close()
    c = Context()
    before = c.state()
    plain_before = _plain_call(c, _struct())
    bad_cam, tall = _struct(mu=0.0), _struct(z=1.5)
    refused = [
        # the entry's own checks, in their order: each call also holds the fault of every later check
        (dict(cam=None, edges=None, nbins=0, spp=0, batches=0), "no camera"),
        (dict(cam=bad_cam, rad=False, nbins=0, spp=0), "no camera"),
        (dict(cam=bad_cam, edges=None, nbins=3), "no camera"),
        (dict(cam=bad_cam, nbins=0, spp=0), "mu"),
        (dict(cam=tall, nbins=0, edges=[1.0, 0.5], spp=0), "numBins must be between 1 and 256"),
        (dict(cam=tall, nbins=257, edges=np.arange(257.0), spp=0), "numBins must be between 1 and 256"),
        (dict(cam=tall, edges=[0.0, np.inf, 1.0], spp=0), "not finite"),
        (dict(cam=tall, edges=[0.0, np.nan], spp=0), "not finite"),
        (dict(cam=tall, edges=[0.5, 1.0], spp=0), "pathEdges[0] must be 0"),
        (dict(cam=tall, edges=[0.0, 1.0, 1.0], spp=0), "strictly ascending"),
        (dict(cam=tall, edges=[0.0, 2.0, 1.0], spp=0), "strictly ascending"),
        # then everything mcbrat_render_camera refuses, in its order
        (dict(cam=tall, spp=0, batches=0), "samplesPerPixel must be at least 1"),
        (dict(cam=_struct(z=1.5, npx=4096, npy=4096), batches=0, n=1, edges=EDGES[256]), "numBatches must be at least 1"),
        (dict(cam=_struct(z=1.5, npx=4096, npy=4096), n=1, edges=EDGES[256]), "tally budget"),
        (dict(cam=_struct(z=1.5, npx=32768, npy=32768), n=1, edges=[0.0], batches=2), "tally budget"),
        (dict(cam=tall), "height"),
    ]
    for kw, word in refused:
        kw = dict(kw)
        rc, text, _ = _call(c, kw.pop("cam"), **kw)
        assert rc != 0 and word in text and text.startswith("renderCameraPathLengths: "), (kw, word, rc, text)
        assert "renderCamera:" not in text
    for kw, word in REFUSED_CAMERAS:
        rc, text, _ = _call(c, _struct(**kw))
        assert rc != 0 and word in text and text.startswith("renderCameraPathLengths: "), (kw, rc, text)
    assert c.state() == before
    # a successful render: sensible numbers, the context still as a fresh one, the plain camera as before
    rc, text, rad = _call(c, _struct(), spp=256, batches=2)
    assert rc == 0 and np.all(rad.reshape(3, 4).sum(axis=0) > 0), (rc, text, rad)
    assert c.state() == before
    assert _plain_call(c, _struct()).tobytes() == plain_before.tobytes()
    dev = float(np.max(np.abs(rad.reshape(3, 4).astype(np.float64).sum(axis=0) - plain_before) / plain_before))
    print("path lengths, the 2 x 2 x 2 context: the bins' sum against the plain render, largest relative deviation %.3g" % dev)
    assert dev <= PLAIN_RTOL, dev
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    rc, text, _ = _call(c, _struct(), spp=0)                                      # ... and after a refused one
    assert rc != 0 and c.state() == before
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    assert _plain_call(c, _struct()).tobytes() == plain_before.tobytes()
    c.close()
    # a source other than the Directional one, a BRDF surface, missing pieces
    c = Context(thermal=True)
    rc, text, _ = _call(c, _struct())
    assert rc != 0 and "Directional solar source" in text and text.startswith("renderCameraPathLengths: ")
    c.close()
    c = Context()
    c.ok(c.L.mcbrat_set_source_random_azimuth(c.ctx, C.c_float(0.5)))
    assert "Directional solar source" in _call(c, _struct())[1]
    c.ok(c.L.mcbrat_set_source_solar(c.ctx, C.c_float(0.5), C.c_float(0.0)))
    c.ok(c.setters["rpv"]())
    text = _call(c, _struct())[1]
    assert "a BRDF surface is not supported by the backward camera" in text and text.startswith("renderCameraPathLengths: ")
    c.close()
    L, ptr = c.L, c.ptr
    bare = L.mcbrat_create(0)
    rad = np.zeros(12, F32)
    s = _struct()
    e, one = np.array([0.0, 0.5, 1.0]), np.ones(8)
    texts = []
    for step in range(4):  # nothing; the grid; optics and source without tables; the forward table without the inverse one
        if step == 1:
            assert L.mcbrat_set_grid(bare, 2, 2, 2, ptr(e), ptr(e), ptr(e)) == 0
        if step == 2:
            assert L.mcbrat_set_optics(bare, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(8, np.int32)), 0.2) == 0
            assert L.mcbrat_set_source_solar(bare, C.c_float(0.5), C.c_float(0.0)) == 0
        if step == 3:
            fwd = np.ones(181, F32)
            assert L.mcbrat_set_forward_table(bare, 1, 181, 1, ptr(fwd), None) == 0
        assert L.mcbrat_render_camera_pathlengths(bare, C.addressof(s), 3, ptr(OK_EDGES), SEED, 0, 64, 1, ptr(rad), None, None, None) != 0
        texts.append(L.mcbrat_last_error(bare).decode())
    L.mcbrat_destroy(bare)
    assert "not completely specified" in texts[0] and "not completely specified" in texts[1], texts
    assert "forward phase function table" in texts[2] and "inverse phase function table" in texts[3], texts
    assert all(t.startswith("renderCameraPathLengths: ") for t in texts[:3]), texts


# ---------------------------------------------------------------------------------------------------------------------------------
# the namelist driver with pathLengthEdges in its /camera/ group, end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_namelist_driver_writes_the_image_by_path_length(tmp_path):
    from mcbrat3d_amd import driver_cli, ncio
    nml, cam_nc, res_nc = tmp_path / "run.nml", tmp_path / "camera.nc", tmp_path / "out.nc"
    head = ("&radiativeTransfer solarMu = 0.5, solarAzimuth = 30. /\n&monteCarlo numPhotonsPerBatch = 2000, numBatches = 4, iseed = 7, nPhaseIntervals = 2001 /\n"
            "&fileNames physDomainFile = 'builtin:i3rcStepCloud', outputNetcdfFile = '%s' /\n" % res_nc)
    camera = ("&camera cameraKind = 'pinhole', cameraPixels = 6, 4, cameraPosition = 0.2, 0.25, 0., cameraLook = 0.2, 0., 1.,\n"
              " cameraUp = 0., 1., 0., cameraFov = 70., cameraSamplesPerPixel = 512, cameraBatches = 4, outputCameraFile = '%s'%s /\n")
    nml.write_text(head + camera % (cam_nc, ""))
    driver_cli.main([str(nml)])
    plain = ncio.readCamera_netcdf(str(cam_nc))
    nml.write_text(head + camera % (cam_nc, ",\n pathLengthEdges = 0., 0.3, 0.6, 1.2, 2.4"))
    driver_cli.main([str(nml)])
    got, res = ncio.readCamera_netcdf(str(cam_nc)), ncio.readCamera_netcdf(str(res_nc))
    assert np.array_equal(got["cameraRadiance"], plain["cameraRadiance"]) and np.array_equal(got["cameraRadiance_StdErr"], plain["cameraRadiance_StdErr"])
    assert not any(k in plain for k in ncio.CAMERA_PATH_VARIABLES) and got["cameraDroppedPaths"] == 0
    by_length = got["cameraRadianceByPathLength"].astype(np.float64)
    assert by_length.shape == (5, 4, 6) and got["cameraRadianceByPathLength_StdErr"].shape == (5, 4, 6)
    assert got["cameraPathLengthEdges"].tolist() == [F32(x) for x in (0.0, 0.3, 0.6, 1.2, 2.4)]
    # the same seed and sample range as the image: the bins sum to it, to the rounding of five float outputs and check 2's
    image = got["cameraRadiance"].astype(np.float64)
    assert np.all(image > 0) and np.all(np.abs(by_length.sum(axis=0) - image) <= (5 * 2.0 ** -24 + PLAIN_RTOL) * image)
    assert (by_length > 0).any(axis=(1, 2)).sum() >= 3
    for k in ncio.CAMERA_PATH_VARIABLES:
        assert np.array_equal(res[k], got[k]), k
