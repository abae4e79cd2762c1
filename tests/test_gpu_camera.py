"""The backward Monte Carlo camera on the GPU: mcbrat_sun_transmittance against an f64 ray-cast
written here, exact vacuum images, the periodic fold on a checkerboard surface, transport theory (absorbing and isotropically
scattering slabs, sensor on top of and inside the slab), reciprocity with the forward local estimate, bitwise determinism,
refusals that leave the context untouched.  `dropped` is 0 in every render here, and badPhotons() of every integrator (the
autouse fixture of conftest.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
SEED = 20261020
PI = np.pi


def _integrator(case, mu0, phi0, rr=True, surface=None, tables=2001, fwd=1801):
    import mcbrat3d_amd as M
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=tables, minForwardTableSize=fwd, useRayTracing=True, useRussianRoulette=rr, surfaceBDRF=surface)
    integ.prepare(dom, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12))
    return integ, dom


def _render(integ, cam, spp, batches=1, seed=SEED, first=0):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderCamera(cam, new_RandomNumberSequence(seed, first), spp, batches)
    assert out["dropped"] == 0
    return out


def _ortho(npx=1, npy=1, mu=1.0, phi=0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("orthographic", npx=npx, npy=npy, mu=mu, phi=phi, footprint=footprint, height=height, **kw)


def _pinhole(npx, npy, position, look, up=(0.0, 1.0, 0.0), fov=60.0, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=npx, npy=npy, position=position, look=look, up=up, fov=fov, **kw)


def _medium(xe, ye, ze, ext, ssa=0.9, albedo=0.0, g=0.0):
    ext = np.asarray(ext, np.float64)
    return dict(name="camera", xe=np.asarray(xe, float), ye=np.asarray(ye, float), ze=np.asarray(ze, float), albedo=albedo,
                components=[dict(ext=ext, ssa=np.where(ext > 0, ssa, 0.0), pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=[cases.hg_legendre(g, 2 if g == 0.0 else 32)])])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. sun transmittance against an f64 ray-cast
# ---------------------------------------------------------------------------------------------------------------------------------
def sun_vector(mu0, phi0):
    """unit vector toward the sun as the library holds it: minus the float32 direction cosines of mcbrat_set_source_solar"""
    mu = -np.abs(np.float32(mu0))
    phi = np.float32(phi0) * np.arccos(np.float32(-1.0)) / np.float32(180.0)
    s = np.sqrt(np.float32(1.0) - mu * mu)
    return -np.array([s * np.cos(phi), s * np.sin(phi), mu], np.float32).astype(np.float64)


def raycast(xe, ye, ze, ext, point, sun):
    """(tau, {cell: its share of tau}) from `point` toward the sun up to the top, in f64: every plane the ray meets -- each periodic
    image of each face -- cuts the ray; a piece lies in the cell of its midpoint.  Independent of the kernel's march by index.
    Along an axis the ray does not move on, a point on a face belongs to the cell above it (the kernel's find_cell)."""
    x, y, z = (float(v) for v in point)
    tTop = (ze[-1] - z) / sun[2]
    if tTop <= 0.0:
        return 0.0, {}
    cuts = [0.0, tTop]
    for e, o, d in ((xe, x, sun[0]), (ye, y, sun[1])):
        L = e[-1] - e[0]
        if d != 0.0:
            lo, hi = sorted((o, o + d * tTop))
            for m in range(int(np.floor((lo - e[0]) / L)) - 1, int(np.floor((hi - e[0]) / L)) + 2):
                for edge in e[:-1]:
                    t = (edge + m * L - o) / d
                    if 0.0 < t < tTop:
                        cuts.append(t)
    for edge in ze:
        t = (edge - z) / sun[2]
        if 0.0 < t < tTop:
            cuts.append(t)
    cuts = np.unique(cuts)
    tau, by_cell = 0.0, {}

    def cell(e, v, moving):
        L = e[-1] - e[0]
        v = e[0] + (v - e[0]) % L if moving is not None else v
        return int(np.clip(np.searchsorted(e, v, side="right") - 1, 0, len(e) - 2))

    for a, b in zip(cuts[:-1], cuts[1:]):
        m = 0.5 * (a + b)
        c = (cell(xe, x + sun[0] * m, True), cell(ye, y + sun[1] * m, True), cell(ze, z + sun[2] * m, None))
        part = ext[c] * (b - a)
        tau += part
        by_cell[c] = by_cell.get(c, 0.0) + part
    return tau, by_cell


# (edges and extinctions: unequal, eight / six distinct values, and chosen -- by a search over random candidates on the CPU, with the
# ray-cast below -- so that every cell a ray of this test walks through holds more than 1 % of the ray's optical depth)
GRIDS = {
    "1x1x1": (np.array([0.0, 0.4]), np.array([0.0, 0.3]), np.array([0.0, 0.25]), np.full((1, 1, 1), 3.0)),
    "2x2x2": (np.array([0.0, 0.192, 0.413]), np.array([-0.1, 0.157, 0.375]), np.array([0.0, 0.094, 0.157]),
              np.array([[[3.2, 0.8], [1.4, 4.4]], [[3.8, 2.0], [2.6, 5.0]]])),
    "3x1x2": (np.array([0.0, 0.106, 0.263, 0.459]), np.array([0.0, 0.423]), np.array([0.0, 0.088, 0.174]),
              np.array([[[3.3, 2.5]], [[4.2, 5.0]], [[1.6, 0.8]]])),
}
SUNS = [(1.0, 0.0), (0.5, 0.0), (0.3, 37.0), (0.05, 200.0)]
# Largest relative deviation of tau = -ln T from the f64 ray-cast measured on the MI355X over every ray below (float face
# distances, float accumulation of segment x extinction, expf, and T itself rounded to float): 6.2e-7 (1.5e-7 / 5.1e-7 / 6.2e-7 on
# the three grids); times 4 for other compilers.  (A deviation near 1e-4 would be a finding about the walk, not a tolerance.)
TAU_RTOL = 2.5e-6


def _points(xe, ye, ze):
    xc, yc, zc = (0.5 * (e[1:] + e[:-1]) for e in (xe, ye, ze))
    pts = [(x, y, z) for x in xc for y in yc for z in zc]                                  # cell centres
    pts += [(xe[i], yc[0], zc[0]) for i in range(len(xe))] + [(xc[0], ye[j], zc[-1]) for j in range(len(ye))]  # on x / y faces (both domain ends too)
    pts += [(xc[-1], yc[-1], ze[k]) for k in range(len(ze))]                               # on z faces: z0 and zMax among them
    pts += [(xe[i], ye[j], zc[0]) for i in range(len(xe)) for j in range(len(ye))]         # on vertical edges
    pts += [(xe[i], ye[j], ze[k]) for i in range(len(xe)) for j in range(len(ye)) for k in range(len(ze))]  # on corners
    Lx, Ly = xe[-1] - xe[0], ye[-1] - ye[0]
    pts += [(xc[0] - 3 * Lx, yc[0] + 2 * Ly, zc[0]), (xe[-1] + 0.25 * Lx, ye[0] - 7.5 * Ly, ze[0]), (xe[0] - Lx, ye[-1] + Ly, zc[-1])]  # outside [x0, xMax)
    return np.array(pts, np.float64)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_sun_transmittance_against_an_f64_raycast(grid):
    xe, ye, ze, ext = GRIDS[grid]
    case = _medium(xe, ye, ze, ext)
    pts = _points(xe, ye, ze)
    worst = 0.0
    for mu0, phi0 in SUNS:
        integ, _ = _integrator(case, mu0, phi0, tables=101, fwd=181)
        got = {}
        for lds in (0, 1):
            integ.setOption(cameraGridInLds=lds)
            got[lds] = integ.sunTransmittance(pts)
        integ.finalize()
        assert got[0].tobytes() == got[1].tobytes()  # the grid in LDS or in global memory: the same walk, bit for bit
        sun = sun_vector(mu0, phi0)
        for p, T in zip(pts, got[0]):
            tau, by_cell = raycast(xe, ye, ze, ext, p, sun)
            if tau == 0.0:
                assert T == 1.0, (grid, mu0, phi0, p)
                continue
            # the condition on this test's own design: a cell missed or walked twice would move tau by more than 1 %
            assert min(by_cell.values()) > 0.01 * tau, (grid, mu0, phi0, p, by_cell)
            dev = abs(-np.log(float(T)) - tau) / tau
            worst = max(worst, dev)
            assert dev < TAU_RTOL, (grid, mu0, phi0, tuple(p), float(T), tau, dev)
    print("sun transmittance %s: largest relative deviation of tau %.3g" % (grid, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. vacuum over a Lambertian surface: exact
# ---------------------------------------------------------------------------------------------------------------------------------
VAC = dict(xe=[0.0, 0.2, 0.5], ye=[0.0, 0.3, 0.5], ze=[0.0, 0.1, 0.25])


def _vacuum_cameras():
    lo, mid, hi = 0.0, 0.11, 0.25
    return {
        "orthographic nadir": (_ortho(3, 2, 1.0, 0.0, height=hi), None),
        "orthographic oblique": (_ortho(3, 2, 0.4, 110.0, height=mid), None),
        "orthographic looking up": (_ortho(2, 2, -0.7, 250.0, height=lo), None),
        # the pinhole: horizontal look, even row count -- the lower rows see the surface, the upper ones the sky (samples at the
        # pixel centres: a jittered sample next to the horizon is a path as long as the bound on a leg's crossings allows)
        "pinhole at z0": (_pinhole(5, 4, (0.1, 0.2, lo), (1.0, 0.3, 0.0), up=(0, 0, 1), fov=100.0, jitter=False), "rows"),
        "pinhole mid-height": (_pinhole(5, 4, (0.1, 0.2, mid), (-1.0, 0.3, 0.0), up=(0, 0, 1), fov=100.0, jitter=False), "rows"),
        "pinhole at zMax": (_pinhole(5, 4, (0.1, 0.2, hi), (0.2, -1.0, 0.0), up=(0, 0, 1), fov=100.0, jitter=False), "rows"),
        "pinhole looking down, jittered": (_pinhole(4, 3, (0.1, 0.2, mid), (0.1, 0.2, -1.0), fov=70.0), None),
    }


@pytest.mark.parametrize("which", ["orthographic nadir", "orthographic oblique", "orthographic looking up", "pinhole at z0",
                                   "pinhole mid-height", "pinhole at zMax", "pinhole looking down, jittered"])
def test_vacuum_over_a_lambertian_surface_is_exact(which):
    a = 0.3
    integ, _ = _integrator(_medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=a), 0.5, 30.0, tables=101, fwd=181)
    cam, rows = _vacuum_cameras()[which]
    out = _render(integ, cam, 197, 2)
    integ.finalize()
    rad, err = out["radiance"], out["radiance_StdErr"]
    down = np.zeros((cam.npy, cam.npx), bool)
    for j in range(cam.npy):
        for i in range(cam.npx):
            dz = [cam.ray(i, j, u, v)[1][2] for u in (0.0, 1.0) for v in (0.0, 1.0)] if cam.jitter else [cam.ray(i, j)[1][2]]
            assert all(d < 0 for d in dz) or all(d > 0 for d in dz)  # (no pixel of these cameras straddles the horizon)
            down[j, i] = dz[0] < 0
    if rows:
        assert down[:2].all() and not down[2:].any()
    assert np.all(err == 0.0)
    assert np.all(rad[~down] == 0.0)
    # to the fixed-point step (2^-32 or finer at these counts) and the float rounding of a T / pi and of the mean
    assert np.all(np.abs(rad[down].astype(np.float64) - a / PI) <= (a / PI) * 2.0 ** -22 + 2.0 ** -31), rad


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. geometry through the periodic fold: exact
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkerboard_surface_through_the_periodic_fold():
    import mcbrat3d_amd as M
    xe, ye, ze = np.array(VAC["xe"]), np.array(VAC["ye"]), np.array(VAC["ze"])
    refl = np.array([[0.1, 0.8], [0.6, 0.25]], np.float32)  # [x patch, y patch]
    sx, sy = np.array([0.0, 0.25, 0.5]), np.array([0.0, 0.2, 0.5])
    surface = M.new_SurfaceDescription(refl[None], sx, sy)
    integ, _ = _integrator(_medium(xe, ye, ze, np.zeros((2, 2, 2)), albedo=0.0), 0.5, 30.0, surface=surface, tables=101, fwd=181)
    cam = _pinhole(16, 12, (0.31, 0.07, 0.2), (0.5, 0.8, -0.45), up=(0.1, 0.0, 1.0), fov=110.0, jitter=False)
    out = _render(integ, cam, 1, 1)
    integ.finalize()
    expected = np.zeros((cam.npy, cam.npx))
    periods, margin = set(), np.inf
    for j in range(cam.npy):
        for i in range(cam.npx):
            o, d = cam.ray(i, j)
            if d[2] >= 0:
                assert d[2] > 1e-3
                continue
            t = (ze[0] - o[2]) / d[2]
            hx, hy = o[0] + d[0] * t, o[1] + d[1] * t
            periods.add((int(np.floor(hx / 0.5)), int(np.floor(hy / 0.5))))
            fx, fy = hx % 0.5, hy % 0.5
            margin = min(margin, min(abs(fx - e) for e in sx), min(abs(fy - e) for e in sy))
            expected[j, i] = refl[int(fx >= sx[1]), int(fy >= sy[1])] / PI
    assert len(periods) >= 6 and margin > 1e-4, (len(periods), margin)  # several domain periods; no hit on a patch boundary
    assert (expected > 0).sum() > 100 and (expected == 0).sum() >= 16
    assert np.all(np.abs(out["radiance"] - expected) <= expected * 2.0 ** -22 + 2.0 ** -31), (out["radiance"], expected)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. transport theory: slabs
# ---------------------------------------------------------------------------------------------------------------------------------
def _slab_check(out, theory):
    mean, err = float(out["radiance"].mean()), float(np.sqrt((out["radiance_StdErr"].astype(np.float64) ** 2).sum()) / out["radiance"].size)
    print("mean %.6g theory %.6g stderr %.3g (%.2f sigma)" % (mean, theory, err, (mean - theory) / err))
    assert err < 0.01 * theory, (err, theory)               # the power condition
    assert abs(mean - theory) < 4.5 * err, (mean, theory, err)


@pytest.mark.parametrize("mu_v,phi_v", [(1.0, 0.0), (0.6, 140.0)])
def test_absorbing_slab_over_a_reflecting_surface(mu_v, phi_v):
    from tests.test_analytic import slab
    tau, a, mu0 = 1.0, 0.5, 0.5
    integ, _ = _integrator(slab(tau, 0.0, albedo=a), mu0, 20.0, tables=101, fwd=181)
    out = _render(integ, _ortho(1, 1, mu_v, phi_v), 16384, 16)
    integ.finalize()
    _slab_check(out, a / PI * np.exp(-tau / mu_v - tau / mu0))


def _slab_cameras(kind, mu, phi, z, looking_down=True):
    """the camera that sees the light travelling along (+-mu, phi) at height z of the plane-parallel slab"""
    m = mu if looking_down else -mu
    if kind == "orthographic":
        return _ortho(1, 1, m, phi, height=z)
    s = np.sqrt(1.0 - m * m)
    look = (-s * np.cos(np.radians(phi)), -s * np.sin(np.radians(phi)), -m)
    return _pinhole(2, 2, (0.1, 0.2, z), look, up=(0.3, -0.2, 0.1) if abs(m) > 0.99 else (0, 0, 1), fov=1.0)


@pytest.mark.parametrize("kind", ["orthographic", "pinhole"])
@pytest.mark.parametrize("b,omega,mu0", [(1.0, 1.0, 0.6), (3.0, 0.9, 1.0)])
def test_radiance_at_the_top_of_an_isotropically_scattering_slab(b, omega, mu0, kind):
    from tests.test_analytic import RADIANCE_MUS, RADIANCE_PHIS, RADIANCE_SLABS, isotropic_radiance, slab
    assert (b, omega, mu0) in RADIANCE_SLABS
    integ, _ = _integrator(slab(b, omega, nz=16), mu0, 33.0, tables=9001)
    theory = isotropic_radiance(b, omega, mu0, RADIANCE_MUS)
    outs = [_render(integ, _slab_cameras(kind, mu, phi, 0.25), 8192 if kind == "pinhole" else 32768, 16) for mu, phi in zip(RADIANCE_MUS, RADIANCE_PHIS)]
    integ.finalize()
    for out, th in zip(outs, theory):
        _slab_check(out, float(th))


def radiance_inside(b, omega, mu0, tau0, mu, cells=1500):
    """(upwelling, downwelling diffuse) radiance along the cosine mu at optical depth tau0 (a cell edge) inside the isotropically
    scattering slab of tests/test_analytic.py, black surface: 1/mu int S(t) e^(-|t - tau0|/mu) dt over the half-line seen, S from
    the same integral equation as isotropic_radiance."""
    from scipy.special import expn
    h = b / cells
    edges = np.arange(cells + 1) * h
    tc = edges[:-1] + 0.5 * h
    kern = 0.5 * np.abs(expn(2, np.abs(tc[:, None] - edges[None, :-1])) - expn(2, np.abs(tc[:, None] - edges[None, 1:])))
    kern[np.arange(cells), np.arange(cells)] = 1.0 - expn(2, 0.5 * h)
    direct = (np.exp(-edges[:-1] / mu0) - np.exp(-edges[1:] / mu0)) / (4.0 * np.pi * h)
    src = np.linalg.solve(np.eye(cells) - omega * kern, omega * direct)
    w = np.abs(np.exp(-np.abs(edges[:-1] - tau0) / mu) - np.exp(-np.abs(edges[1:] - tau0) / mu))
    below = tc > tau0
    return float(np.sum(src[below] * w[below])), float(np.sum(src[~below] * w[~below]))


@pytest.mark.parametrize("b,omega,mu0", [(1.0, 1.0, 0.6), (3.0, 0.9, 1.0)])
def test_radiance_inside_an_isotropically_scattering_slab(b, omega, mu0):
    from tests.test_analytic import slab
    integ, _ = _integrator(slab(b, omega, nz=16), mu0, 33.0, tables=9001)
    mu, phi = 0.7, 120.0
    up, down = radiance_inside(b, omega, mu0, 0.5 * b, mu)
    for looking_down, theory in ((True, up), (False, down)):
        _slab_check(_render(integ, _slab_cameras("orthographic", mu, phi, 0.125, looking_down), 32768, 16), theory)
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. reciprocity with the forward local estimate
# ---------------------------------------------------------------------------------------------------------------------------------
def small_domain():
    """4 x 3 x 2, unequal edges (cells 0.125 x 0.1 wide -- the camera cuts its footprint into equal pixels, so pixels are columns
    only where the columns are equally wide -- and layers of 0.08 and 0.12), two components, a per-patch surface.
    Both components are Henyey-Greenstein series long enough for their inverse tables to sample what their forward tables hold
    (<mu> and <P2> of the inverse table to 5e-4).  That matters here and nowhere else in this file: the forward estimator takes the
    LAST scattering of a history from the forward table and samples the others from the inverse one, the backward estimator takes
    the FIRST (the one next to the sun), so the two agree only as far as the two tables describe one phase function.  With the
    two-term series (0, 0.1) as second component -- the reference's inverse routine samples it isotropically, <P2> = 1e-4 where
    the forward table has 0.1 -- the domain means of this test differed by 0.9 % (7.5 sigma), by 4.4 % with that component alone,
    and by less than one sigma without it (measured)."""
    xe, ye, ze = 0.125 * np.arange(5), 0.1 * np.arange(4), np.array([0.0, 0.08, 0.2])
    rng = np.random.default_rng(5)
    e1, e2 = rng.uniform(2.0, 12.0, (4, 3, 2)), rng.uniform(0.5, 3.0, (4, 3, 2))
    case = dict(name="small", xe=xe, ye=ye, ze=ze, albedo=0.0,
                components=[dict(ext=e1, ssa=np.full_like(e1, 0.95), pfIndex=np.ones(e1.shape, np.int32), legendre=[cases.hg_legendre(0.7, 64)]),
                            dict(ext=e2, ssa=np.full_like(e2, 1.0), pfIndex=np.ones(e2.shape, np.int32), legendre=[cases.hg_legendre(0.3, 32)])])
    return cases.patchy_surface(case, 3, 2)


def _reciprocity(case, mu0, phi0, views, z_of, photons, batches, spp):
    """forward INTEN run and backward render of the same pixels -> per view (forward mean, its error, backward mean, its error)"""
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    mus, phis = [v[0] for v in views], [v[1] for v in views]
    integ.specifyParameters(minInverseTableSize=9001, minForwardTableSize=1801, intensityMus=mus, intensityPhis=phis, computeIntensity=True,
                            surfaceBDRF=cases.product_surface(case))
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12), photons, batches)
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, len(views)))
    xe, ye = case["xe"], case["ye"]
    res = []
    for d, (mu, phi) in enumerate(views):
        cam = _ortho(dom.numX, dom.numY, mu, phi, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=z_of(mu))
        out = _render(integ, cam, spp, 16, seed=SEED + 1 + d)
        res.append((st["intensity"][:, :, d].T.astype(np.float64), st["intensity_StdErr"][:, :, d].T.astype(np.float64),
                    out["radiance"].astype(np.float64), out["radiance_StdErr"].astype(np.float64)))
    integ.finalize()
    return res


def _reciprocity_check(res):
    for fwd, ferr, bwd, berr in res:
        err = np.sqrt(ferr ** 2 + berr ** 2)
        z = (bwd - fwd) / err
        mean_err = np.sqrt((ferr ** 2).sum() + (berr ** 2).sum()) / fwd.size
        print("pixels: worst %.2f sigma; domain mean forward %.6g backward %.6g, combined error %.3g (%.2f %%)" % (
            np.abs(z).max(), fwd.mean(), bwd.mean(), mean_err, 100 * mean_err / fwd.mean()))
        assert np.all(np.abs(z) < 4.5), z                                   # every pixel, none left out
        assert mean_err < 0.01 * fwd.mean()                                 # the power condition on the domain mean
        assert abs(bwd.mean() - fwd.mean()) < 4.5 * mean_err


def test_reciprocity_with_the_forward_estimate_on_the_step_cloud():
    """32 x 1 pixels, nadir and (0.6, 110): forward 40 x 200000 photons, backward 16 x 8192 paths per pixel.  Measured on the
    MI355X: combined error of the domain mean 0.24 % and 0.23 % of it (below the 1 % the power condition asks for), domain means
    -1.8 and -0.3 of that error apart, worst pixel 3.5 sigma; the test runs in 0.25 s."""
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    _reciprocity_check(_reciprocity(case, 0.5, 30.0, [(1.0, 0.0), (0.6, 110.0)], lambda mu: 0.25, 200000, 40, 8192))


def test_reciprocity_with_the_forward_estimate_on_a_small_domain():
    """4 x 3 pixels over two components, unequal edges and a per-patch surface: two upward views at zMax (forward 40 x 200000
    photons, backward 16 x 16384 paths per pixel: combined error of the domain mean 0.12-0.13 %, measured)."""
    _reciprocity_check(_reciprocity(small_domain(), 0.5, 30.0, [(1.0, 0.0), (0.6, 110.0)], lambda mu: 0.2, 200000, 40, 16384))


def test_reciprocity_of_a_downward_view_on_the_small_domain():
    """The light travelling down (mu = -0.6) at z0: a camera on the ground that looks up.  Over a BLACK surface: for mu < 0 the
    forward product, like the reference, also takes a local estimate from every surface reflection -- its view ray starts below
    the surface -- so over a reflecting surface its downward `intensity` holds a term a F_down / pi that no sensor above the
    surface sees (measured on the per-patch surface: forward 0.299, backward 0.230, the pixel over the black patch equal)."""
    case = small_domain()
    case.pop("surface")
    _reciprocity_check(_reciprocity(case, 0.5, 30.0, [(-0.6, 75.0)], lambda mu: 0.0, 200000, 40, 16384))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_means_are_bitwise_reproducible():
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    integ, _ = _integrator(case, 0.5, 30.0)
    cam = lambda lds=-1: _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)  # noqa: E731  (a sky imager inside the cloud)
    spp = 1000  # (not a multiple of 64)
    two = _render(integ, cam(), spp, 2)["batchMeans"]
    assert _render(integ, cam(), spp, 2)["batchMeans"].tobytes() == two.tobytes()                      # two identical calls
    first, second = _render(integ, cam(), spp, 1, first=0)["batchMeans"], _render(integ, cam(), spp, 1, first=spp)["batchMeans"]
    assert first.tobytes() == two[:1].tobytes() and second.tobytes() == two[1:].tobytes()              # two batches = two calls
    assert _render(integ, cam(0), spp, 2)["batchMeans"].tobytes() == _render(integ, cam(1), spp, 2)["batchMeans"].tobytes() == two.tobytes()
    # the same samples as part of a longer range: 1000 alone against batch 1 of 3 from firstSample = -1000
    longer = _render(integ, cam(), spp, 3, first=2 ** 40 - spp)["batchMeans"]
    assert _render(integ, cam(), spp, 1, first=2 ** 40)["batchMeans"].tobytes() == longer[1:2].tobytes()
    assert two.std() > 0 and np.all(two > 0)
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals, and a context left as it was
# ---------------------------------------------------------------------------------------------------------------------------------
def _struct(**kw):
    from mcbrat3d_amd._capi import Camera
    s = Camera()
    s.kind, s.npx, s.npy, s.jitter, s.gridInLds, s.mu, s.phiDeg = 0, 2, 2, 1, -1, 1.0, 0.0
    s.xLo, s.xHi, s.yLo, s.yHi, s.z = 0.0, 1.0, 0.0, 1.0, 1.0
    s.position[:], s.look[:], s.up[:], s.fovXDeg = (0.5, 0.5, 0.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0
    for k, v in kw.items():
        if k in ("position", "look", "up"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def _call(ctx, cam, spp=64, batches=1, n=4):
    rad = np.zeros(max(n, 1), np.float32)
    rc = ctx.L.mcbrat_render_camera(ctx.ctx, C.addressof(cam), SEED, 0, spp, batches, ctx.ptr(rad), None, None, None)
    return rc, (ctx.L.mcbrat_last_error(ctx.ctx).decode() if rc else ""), rad


REFUSED_CAMERAS = [
    (dict(mu=0.0), "mu"), (dict(z=1.5), "height"), (dict(z=-0.1), "height"), (dict(xHi=0.0), "footprint"), (dict(yLo=2.0), "footprint"),
    (dict(kind=1, look=(0.0, 2.0, 0.0)), "parallel"), (dict(kind=1, fovXDeg=0.0), "field of view"), (dict(kind=1, fovXDeg=180.0), "field of view"),
    (dict(kind=1, position=(0.5, 0.5, 1.01)), "height"), (dict(kind=2), "kind"), (dict(npx=0), "pixel"),
]


def test_refusals_leave_the_context_untouched():
    from tests.test_gpu_refusal_matrix import Context
    fresh = Context()
    _, reference = fresh.trace()
    fresh.close()
    c = Context()
    before = c.state()
    for kw, word in REFUSED_CAMERAS:
        rc, text, _ = _call(c, _struct(**kw))
        assert rc != 0 and word in text and text.startswith("renderCamera:"), (kw, rc, text)
    rc, text, _ = _call(c, _struct(), spp=0)
    assert rc != 0 and "samplesPerPixel" in text
    rc, text, _ = _call(c, _struct(npx=32768, npy=32768), batches=2, n=1)
    assert rc != 0 and "tally budget" in text
    assert c.state() == before
    # a successful render: sensible numbers, and the context still as a fresh one
    rc, text, rad = _call(c, _struct(), spp=256, batches=2)
    assert rc == 0 and np.all(rad > 0), (rc, text, rad)
    assert c.state() == before
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    c.close()
    # a source other than the Directional one, a BRDF surface, missing pieces
    c = Context(thermal=True)
    rc, text, _ = _call(c, _struct())
    assert rc != 0 and "Directional solar source" in text
    c.close()
    c = Context()
    c.ok(c.L.mcbrat_set_source_random_azimuth(c.ctx, C.c_float(0.5)))
    assert "Directional solar source" in _call(c, _struct())[1]
    c.ok(c.L.mcbrat_set_source_solar(c.ctx, C.c_float(0.5), C.c_float(0.0)))
    c.ok(c.setters["rpv"]())
    assert "BRDF surface" in _call(c, _struct())[1]
    c.close()
    L, ptr = c.L, c.ptr
    bare = L.mcbrat_create(0)
    rad = np.zeros(4, np.float32)
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
            fwd = np.ones(181, np.float32)
            assert L.mcbrat_set_forward_table(bare, 1, 181, 1, ptr(fwd), None) == 0
        assert L.mcbrat_render_camera(bare, C.addressof(s), SEED, 0, 64, 1, ptr(rad), None, None, None) != 0
        texts.append(L.mcbrat_last_error(bare).decode())
    L.mcbrat_destroy(bare)
    assert "not completely specified" in texts[0] and "not completely specified" in texts[1], texts
    assert "forward phase function table" in texts[2] and "inverse phase function table" in texts[3], texts


# ---------------------------------------------------------------------------------------------------------------------------------
# the namelist driver with a /camera/ group, end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_namelist_driver_renders_and_writes_the_camera(tmp_path):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import driver_cli
    nml, cam_nc, res_nc = tmp_path / "run.nml", tmp_path / "camera.nc", tmp_path / "out.nc"
    text = ("&radiativeTransfer solarMu = 0.5, solarAzimuth = 30. /\n&monteCarlo numPhotonsPerBatch = 2000, numBatches = 4, iseed = 7, nPhaseIntervals = 2001 /\n"
            "&fileNames physDomainFile = 'builtin:i3rcStepCloud', outputNetcdfFile = '%s' /\n" % res_nc)
    nml.write_text(text)
    plain = driver_cli.main([str(nml)])
    nml.write_text(text + "&camera cameraKind = 'pinhole', cameraPixels = 6, 4, cameraPosition = 0.2, 0.25, 0., cameraLook = 0.2, 0., 1.,\n"
                          " cameraUp = 0., 1., 0., cameraFov = 70., cameraSamplesPerPixel = 512, cameraBatches = 4, outputCameraFile = '%s' /\n" % cam_nc)
    stats = driver_cli.main([str(nml)])
    for k in ("meanFluxUp", "meanFluxDown", "fluxUp"):  # the group changes nothing else
        assert np.array_equal(np.asarray(stats[k]), np.asarray(plain[k])), k
    a, b = netcdf_file(str(cam_nc), "r", mmap=False), netcdf_file(str(res_nc), "r", mmap=False)
    try:
        img = a.variables["cameraRadiance"][:].copy()
        assert img.shape == (4, 6) and np.all(img > 0) and np.all(a.variables["cameraRadiance_StdErr"][:] > 0)  # a sky imager under the cloud
        assert np.array_equal(b.variables["cameraRadiance"][:], img) and a.cameraKind.decode() == "pinhole" and a.cameraDroppedPaths == 0
        assert a.cameraSamplesPerPixel == 512 and a.cameraBatches == 4 and list(a.cameraPixels) == [6, 4]
    finally:
        a.close()
        b.close()
