"""The emission renders on the GPU: exact cases (a vacuum over an emitting surface, Kirchhoff, every
sample of a small render recomputed), transport theory for emitting slabs (tests/test_analytic.py), reciprocity with the forward
thermal `intensity`, bitwise invariants, refusals.  `dropped` is 0 in every render here."""
import ctypes as C

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
SEED = 20261021
PI = np.pi


def _integrator(case, source="none", rr=True, surface=None, tables=2001, mu0=0.5, phi0=30.0):
    """an integrator with the case's domain loaded and: no source at all, the Directional solar one, or the thermal one"""
    import mcbrat3d_amd as M
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=tables, useRayTracing=True, useRussianRoulette=rr, surfaceBDRF=surface,
                            LW_flag=1.0 if source == "thermal" else -1.0)
    if source == "none":
        integ.prepareDomain(dom)
    elif source == "solar":
        integ.prepare(dom, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12))
    else:
        w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
        M.emission_weighting(dom, w, case["sfc_temp"])
        integ.prepare(dom, M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12))
    return integ, dom


def _render(integ, cam, spp, batches, cell, sfc, seed=SEED, first=0):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderCameraEmission(cam, new_RandomNumberSequence(seed, first), spp, batches, cellSource=cell, surfaceSource=sfc)
    assert out["dropped"] == 0
    return out


def _sense(integ, sensors, n, batches, cell, sfc, seed=SEED, first=0, lds=-1):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderSensorsEmission(sensors, new_RandomNumberSequence(seed, first), n, batches, cellSource=cell, surfaceSource=sfc, gridInLds=lds)
    assert out["dropped"] == 0
    return out


def _ortho(npx=1, npy=1, mu=1.0, phi=0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("orthographic", npx=npx, npy=npy, mu=mu, phi=phi, footprint=footprint, height=height, **kw)


def _pinhole(npx, npy, position, look, up=(0.0, 1.0, 0.0), fov=60.0, **kw):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=npx, npy=npy, position=position, look=look, up=up, fov=fov, **kw)


def _medium(xe, ye, ze, ext, ssa=0.0, albedo=0.0):
    ext = np.asarray(ext, np.float64)
    return dict(name="emission", xe=np.asarray(xe, float), ye=np.asarray(ye, float), ze=np.asarray(ze, float), albedo=albedo,
                components=[dict(ext=ext, ssa=np.where(ext > 0, ssa, 0.0), pfIndex=np.ones(ext.shape, np.int32), legendre=[cases.hg_legendre(0.0, 2)])])


def _exact(value, expected, src_max, w0=1.0):
    """to the fixed-point step (src_max 2^-40 at these counts, times w0) and the float rounding of the deposit and of the mean"""
    return np.all(np.abs(np.asarray(value, np.float64) - expected) <= np.abs(expected) * 2.0 ** -22 + w0 * src_max * 2.0 ** -31)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a vacuum over an emitting Lambertian surface: exact
# ---------------------------------------------------------------------------------------------------------------------------------
VAC = dict(xe=[0.0, 0.2, 0.5], ye=[0.0, 0.3, 0.5], ze=[0.0, 0.1, 0.25])
CHECKER = np.array([[3.0, 11.5], [7.25, 0.5]], np.float32)  # surfaceSource[iy, ix]


def _vacuum_cameras():
    lo, mid, hi = 0.0, 0.11, 0.25
    return {
        "orthographic nadir": _ortho(3, 2, 1.0, 0.0, height=hi, jitter=False),
        "orthographic oblique": _ortho(3, 2, 0.4, 110.0, height=mid, jitter=False),
        "orthographic looking up": _ortho(2, 2, -0.7, 250.0, height=lo, jitter=False),
        "orthographic down at z0": _ortho(3, 2, 0.8, 40.0, height=lo, jitter=False),
        "pinhole at z0": _pinhole(5, 4, (0.1, 0.2, lo), (1.0, 0.3, 0.0), up=(0, 0, 1), fov=100.0, jitter=False),
        "pinhole mid-height": _pinhole(5, 4, (0.1, 0.2, mid), (-1.0, 0.3, 0.0), up=(0, 0, 1), fov=100.0, jitter=False),
        "pinhole at zMax": _pinhole(5, 4, (0.1, 0.2, hi), (0.2, -1.0, 0.0), up=(0, 0, 1), fov=100.0, jitter=False),
    }


@pytest.mark.parametrize("which", sorted(_vacuum_cameras()))
def test_vacuum_over_an_emitting_surface_is_exact(which):
    a = 0.3
    integ, _ = _integrator(_medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=a), tables=101)
    cam = _vacuum_cameras()[which]
    out = _render(integ, cam, 197, 2, np.zeros((2, 2, 2), np.float32), CHECKER)
    integ.finalize()
    xe, ye = np.array(VAC["xe"]), np.array(VAC["ye"])
    expected, margin = np.zeros((cam.npy, cam.npx)), np.inf
    for j in range(cam.npy):
        for i in range(cam.npx):
            o, d = cam.ray(i, j)
            if d[2] > 0:
                continue
            t = (0.0 - o[2]) / d[2]
            hx, hy = (o[0] + d[0] * t) % 0.5, (o[1] + d[1] * t) % 0.5
            margin = min(margin, np.abs(xe - hx).min(), np.abs(ye - hy).min())
            emitted = np.float32(np.float32(1.0) - np.float32(a)) * CHECKER[int(hy >= ye[1]), int(hx >= xe[1])]
            expected[j, i] = float(emitted)
    assert margin > 1e-4                                   # no line of sight meets the surface on a column's edge
    seen = expected > 0
    if which == "orthographic looking up":
        assert not seen.any()
    else:                                                  # more than one column of the checkerboard is seen (from z0: the one below)
        assert len(set(expected[seen])) >= (1 if which == "pinhole at z0" else 2)
    if which.startswith("pinhole"):
        assert (~seen).any()                               # ... and the rows above the horizon see none
    assert np.all(out["radiance_StdErr"] == 0.0)
    assert np.all(out["radiance"][~seen] == 0.0)           # above the horizon: exactly nothing
    assert _exact(out["radiance"][seen], expected[seen], float(CHECKER.max())), (out["radiance"], expected)


def test_point_sensors_over_a_uniform_emitting_surface_are_exact():
    from mcbrat3d_amd.sensors import new_Sensors
    a, s_sfc = 0.3, 6.5
    integ, _ = _integrator(_medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=a), tables=101)
    sensors = new_Sensors([(0.1, 0.2, 0.25), (0.1, 0.2, 0.25), (0.3, 0.4, 0.0)], tilt=[180.0, 0.0, 0.0])
    out = _sense(integ, sensors, 197, 2, np.zeros((2, 2, 2), np.float32), np.full((2, 2), s_sfc, np.float32))
    integ.finalize()
    assert set(out) >= {"irradiance", "irradiance_StdErr", "batchMeans", "dropped"} and out["batchMeans"].shape == (2, 3)
    assert np.all(out["irradiance_StdErr"] == 0.0)
    emitted = float(np.float32(np.float32(1.0) - np.float32(a)) * np.float32(s_sfc))
    assert _exact(out["irradiance"][0], PI * emitted, s_sfc, PI), out["irradiance"]   # facing down at zMax: pi (1 - a) S_sfc
    assert out["irradiance"][1] == 0.0 and out["irradiance"][2] == 0.0                # facing up: exactly nothing


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. Kirchhoff: an absorbing medium and a black surface at one temperature emit B along every line of sight
# ---------------------------------------------------------------------------------------------------------------------------------
def test_kirchhoff_bit_for_bit():
    from tests.test_gpu_camera import GRIDS
    xe, ye, ze, ext = GRIDS["2x2x2"]
    B = 7.3125
    integ, _ = _integrator(_medium(xe, ye, ze, ext, ssa=0.0, albedo=0.0), tables=101)
    fp = (xe[0], xe[-1], ye[0], ye[-1])
    cams = [_ortho(3, 2, mu, phi, footprint=fp, height=ze[-1]) for mu, phi in ((1.0, 0.0), (0.7, 120.0), (0.35, 250.0), (0.05, 33.0))]
    cams.append(_pinhole(4, 3, (0.1, 0.2, ze[-1]), (0.1, 0.2, -1.0), fov=70.0))
    for cam in cams:
        out = _render(integ, cam, 197, 2, np.full((2, 2, 2), B, np.float32), np.full((2, 2), B, np.float32))
        assert np.all(out["radiance_StdErr"] == 0.0)
        assert _exact(out["radiance"], B, B), out["radiance"]
        assert np.all(out["radiance"] == np.float32(B))    # ... and in fact to the bit: B / srcMax is 1
    integ.finalize()


def test_kirchhoff_actinic_flux_at_the_bottom_of_a_slab():
    """2 pi B from the surface below and 2 pi B (1 - E2(tau)) from the layer above (nothing comes in at the top)"""
    from scipy.special import expn
    from mcbrat3d_amd.sensors import new_Sensors
    from tests.test_analytic import slab
    tau, B = 1.0, 4.25
    case = slab(tau, 0.0)
    nz = len(case["ze"]) - 1
    integ, _ = _integrator(case, tables=101)
    out = _sense(integ, new_Sensors([(0.2, 0.3, case["ze"][0])], kind="spherical"), 16384, 16, np.full((nz, 1, 1), B, np.float32), np.full((1, 1), B, np.float32))
    integ.finalize()
    theory = 2.0 * PI * B + 2.0 * PI * B * (1.0 - float(expn(2, tau)))
    v, e = float(out["irradiance"][0]), float(out["irradiance_StdErr"][0])
    print("actinic flux %.6g theory %.6g stderr %.3g (%.2f sigma)" % (v, theory, e, (v - theory) / e))
    assert e < 0.005 * theory and abs(v - theory) < 4.5 * e


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every sample of a small render, recomputed from Philox, mcbrat_camera_ray and an f64 ray-cast
# ---------------------------------------------------------------------------------------------------------------------------------
SBS = dict(xe=np.array([0.0, 0.3, 0.5]), ye=np.array([0.0, 0.4]), ze=np.array([0.0, 0.1, 0.25]),
           ext=np.array([[[1.5, 4.0]], [[6.0, 2.5]]]),                                # [ix, iy, iz]
           cell=np.array([[[2.0, 9.5]], [[5.25, 13.0]]], np.float32),                   # cellSource[iz, iy, ix]
           sfc=np.array([[1.0, 7.5]], np.float32))                                      # surfaceSource[iy, ix]
# (the seed: the first of six candidates tried on the CPU whose smallest margin, below, is above 1e-3: 100 times the bound asked for)
SBS_SEED, SBS_N, SBS_BATCHES = 20261026, 197, 3


def _sbs_camera():
    return _pinhole(1, 1, (0.21, 0.13, 0.2), (0.35, 0.2, -1.0), up=(0.0, 1.0, 0.0), fov=120.0)


def _first_event(o, d, tau, g):
    """f64: the first event of the path from o along d with optical depth tau -> (the deposit, the smallest distance of the event's
    point to a face of its cell relative to the cell, or of tau to the optical depth at the exit relative to it)"""
    xe, ye, ze, ext = g["xe"], g["ye"], g["ze"], g["ext"]
    if d[2] == 0.0:
        return None
    tEnd = ((ze[-1] if d[2] > 0 else ze[0]) - o[2]) / d[2]
    cuts = [0.0, tEnd]
    for e, p, q in ((xe, o[0], d[0]), (ye, o[1], d[1])):
        L = e[-1] - e[0]
        if q != 0.0:
            lo, hi = sorted((p, p + q * tEnd))
            for m in range(int(np.floor((lo - e[0]) / L)) - 1, int(np.floor((hi - e[0]) / L)) + 2):
                cuts += [t for t in ((edge + m * L - p) / q for edge in e[:-1]) if 0.0 < t < tEnd]
    cuts += [t for t in ((edge - o[2]) / d[2] for edge in ze) if 0.0 < t < tEnd]
    cuts = np.unique(cuts)

    def where(t):
        x, y, z = o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t
        x, y = xe[0] + (x - xe[0]) % (xe[-1] - xe[0]), ye[0] + (y - ye[0]) % (ye[-1] - ye[0])
        idx = [int(np.clip(np.searchsorted(e, v, side="right") - 1, 0, len(e) - 2)) for e, v in ((xe, x), (ye, y), (ze, z))]
        rel = min(min(v - e[i], e[i + 1] - v) / (e[i + 1] - e[i]) for e, v, i in ((xe, x, idx[0]), (ye, y, idx[1]), (ze, z, idx[2])))
        return idx, rel

    acc = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        (ix, iy, iz), _ = where(0.5 * (a + b))
        part = ext[ix, iy, iz] * (b - a)
        if acc + part >= tau:
            (jx, jy, jz), rel = where(a + (tau - acc) / ext[ix, iy, iz])
            assert (jx, jy, jz) == (ix, iy, iz)
            return float(g["cell"][iz, iy, ix]), rel
        acc += part
    margin = (tau - acc) / acc
    if d[2] > 0:
        return 0.0, margin                                                             # the top: nothing comes in
    (ix, iy, _), _ = where(tEnd)
    x, y = o[0] + d[0] * tEnd, o[1] + d[1] * tEnd
    x, y = xe[0] + (x - xe[0]) % (xe[-1] - xe[0]), ye[0] + (y - ye[0]) % (ye[-1] - ye[0])
    rel = min(min(v - e[i], e[i + 1] - v) / (e[i + 1] - e[i]) for e, v, i in ((xe, x, ix), (ye, y, iy)))
    return float(g["sfc"][iy, ix]), min(margin, rel)


def sample_by_sample_reference(seed=SBS_SEED):
    """-> (the deposit of every sample [batch, k], the smallest margin): host arithmetic only"""
    from tests.test_gpu_sources import philox, u01
    cam = _sbs_camera()
    n = SBS_N * SBS_BATCHES
    ids = np.arange(n, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros(n, np.uint64)
    jit = philox([zero, zero, ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], key)          # event 0, pixel 0
    leg = philox([zero + np.uint64(1), zero, ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], key)  # event 1
    u, v = u01(jit[0]).astype(np.float64), u01(jit[1]).astype(np.float64)
    tiny = np.float32(np.finfo(np.float32).tiny)
    tau = np.maximum(-np.log(np.maximum(u01(leg[0]), tiny)), tiny).astype(np.float64)            # (float32 arithmetic, as the kernel's)
    deposits, margin = np.zeros(n), np.inf
    for k in range(n):
        o, d = cam.ray(0, 0, float(u[k]), float(v[k]))
        d = np.asarray(d, np.float32).astype(np.float64)                                # the kernel marches along the float direction
        deposits[k], rel = _first_event(np.asarray(o, np.float64), d, float(tau[k]), SBS)
        margin = min(margin, rel)
    return deposits.reshape(SBS_BATCHES, SBS_N), margin


def test_every_sample_is_recomputed():
    deposits, margin = sample_by_sample_reference()
    # the design of the test itself: no sample's event lies where the kernel's float march may legitimately pick the neighbour
    assert margin > 1e-5, margin
    assert len(set(deposits.reshape(-1))) == 6          # the four cells and the two columns of the surface are all met
    integ, _ = _integrator(_medium(SBS["xe"], SBS["ye"], SBS["ze"], SBS["ext"], ssa=0.0, albedo=0.0), tables=101)
    out = _render(integ, _sbs_camera(), SBS_N, SBS_BATCHES, SBS["cell"], SBS["sfc"], seed=SBS_SEED)
    integ.finalize()
    src_max = float(SBS["cell"].max())
    step = src_max * 2.0 ** -40                          # the scale at 197 samples per bin is 2^40 per unit of srcMax
    got = out["batchMeans"].reshape(SBS_BATCHES).astype(np.float64)
    want = deposits.mean(axis=1)
    print("batch means", got, "recomputed", want)
    # n fixed-point steps on the batch's sum; the mean is handed back as a float
    assert np.all(np.abs(got - want) <= SBS_N * step / SBS_N + want * 2.0 ** -23), (got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. - 6. transport theory: emitting, isotropically scattering slabs
# ---------------------------------------------------------------------------------------------------------------------------------
def _thermal(tau, omega, temps, sfc, albedo=0.0, lam=10.0):
    """the slab of tests/test_analytic.thermal_case with a surface albedo -> (case, cellSource, surfaceSource, total), sources in the
    units of tests/test_analytic.planck, total = 4 pi (1 - omega) sum B dtau + pi (1 - a) B_s: what the theory's shares are shares of"""
    from tests.test_analytic import planck, thermal_case
    case, _, _, _ = thermal_case(tau, omega, temps, sfc, lam)
    case["albedo"] = albedo
    n = len(temps)
    b_l, b_s = planck(lam, np.asarray(temps, np.float64)), float(planck(lam, sfc))
    cell = np.broadcast_to(b_l[:, None, None], (n, n, n)).astype(np.float32)
    total = 4.0 * PI * (1.0 - omega) * float(b_l.sum()) * tau / n + PI * (1.0 - albedo) * b_s
    return case, cell, np.full((n, n), b_s, np.float32), total


def _theory_check(what, value, err, theory, src_max, w0=1.0):
    print("%s: %.6g theory %.6g stderr %.3g (%s sigma)" % (what, value, theory, err, "%.2f" % ((value - theory) / err) if err > 0 else "-"))
    if err == 0.0:  # the same value in every batch (every path ends in the same deposit, or in none): exact instead
        assert _exact(value, theory, src_max, w0), (what, value, theory)
        return
    assert err < 0.005 * theory, (what, err, theory)           # the power condition
    assert abs(value - theory) < 4.5 * err, (what, value, theory, err)


@pytest.mark.parametrize("tau,omega,temps,sfc", __import__("tests.test_analytic", fromlist=["THERMAL_SLABS"]).THERMAL_SLABS)
def test_radiance_at_the_top_of_an_emitting_slab(tau, omega, temps, sfc):
    from tests.test_analytic import RADIANCE_MUS, RADIANCE_PHIS, planck, thermal_radiance
    case, cell, sfc_src, total = _thermal(tau, omega, temps, sfc)
    theory = thermal_radiance(tau, omega, planck(10.0, np.asarray(temps)[::-1]), float(planck(10.0, sfc)), RADIANCE_MUS) * total
    integ, _ = _integrator(case, tables=101)
    outs = [_render(integ, _ortho(1, 1, mu, phi, footprint=(0.0, 0.6, 0.0, 0.6), height=0.6), 16384, 16, cell, sfc_src) for mu, phi in zip(RADIANCE_MUS, RADIANCE_PHIS)]
    integ.finalize()
    for mu, out, th in zip(RADIANCE_MUS, outs, theory):
        _theory_check("mu %.2f" % mu, float(out["radiance"][0, 0]), float(out["radiance_StdErr"][0, 0]), float(th), float(max(cell.max(), sfc_src.max())))


@pytest.mark.parametrize("b,omega,temp,sfc", [(1.0, 0.5, 285.0, 300.0), (3.0, 0.9, 270.0, 305.0)])
def test_fluxes_of_an_emitting_slab_over_a_grey_surface(b, omega, temp, sfc):
    """a = 0.3, isotropic scattering: the flux through the top and onto the surface against matrix doubling with Kirchhoff's law"""
    from mcbrat3d_amd.sensors import new_Sensors
    from tests.test_analytic import planck, thermal_doubling
    a = 0.3
    case, cell, sfc_src, total = _thermal(b, omega, [temp] * 6, sfc, albedo=a)
    _, up, onto = thermal_doubling(b, omega, [1.0], float(planck(10.0, temp)), float(planck(10.0, sfc)), a)
    integ, _ = _integrator(case, tables=101)
    out = _sense(integ, new_Sensors([(0.31, 0.17, 0.6), (0.31, 0.17, 0.0)], tilt=[180.0, 0.0]), 16384, 16, cell, sfc_src)
    integ.finalize()
    for what, i, th in (("through the top", 0, up * total), ("onto the surface", 1, onto * total)):
        _theory_check(what, float(out["irradiance"][i]), float(out["irradiance_StdErr"][i]), float(th), float(max(cell.max(), sfc_src.max())), PI)


@pytest.mark.parametrize("tau,omega,temps,sfc", __import__("tests.test_analytic", fromlist=["THERMAL_SLABS"]).THERMAL_SLABS)
def test_fluxes_inside_an_emitting_slab(tau, omega, temps, sfc):
    from mcbrat3d_amd.sensors import new_Sensors
    from tests.test_analytic import planck, thermal_profile
    case, cell, sfc_src, total = _thermal(tau, omega, temps, sfc)
    taus = [0.0, 0.5 * tau, tau]
    up, down = thermal_profile(tau, omega, planck(10.0, np.asarray(temps)[::-1]), float(planck(10.0, sfc)), taus)
    zs = [0.6 * (1.0 - t / tau) for t in taus]
    # facing down measures the upward flux, facing up the downward one
    sensors = new_Sensors([(0.31, 0.17, z) for z in zs for _ in (0, 1)], tilt=[180.0, 0.0] * 3)
    integ, _ = _integrator(case, tables=101)
    out = _sense(integ, sensors, 16384, 16, cell, sfc_src)
    integ.finalize()
    for k, t in enumerate(taus):
        for side, th in ((0, up[k]), (1, down[k])):
            _theory_check("tau %.2f %s" % (t, ("up", "down")[side]), float(out["irradiance"][2 * k + side]), float(out["irradiance_StdErr"][2 * k + side]),
                          float(th * total), float(max(cell.max(), sfc_src.max())), PI)


# ---------------------------------------------------------------------------------------------------------------------------------
# reciprocity with the forward thermal `intensity`
# ---------------------------------------------------------------------------------------------------------------------------------
def _thermal_small_domain(patchy):
    """the 4 x 3 x 2 domain of the camera's reciprocity test with temperatures that differ along all three axes.  The forward
    thermal source, like the reference's, emits pi (1 - A) B_s from the surface with A the DOMAIN's albedo, whatever the surface
    description reflects: over the per-patch surface the two estimators describe one physical problem only where the surface
    does not emit, so that case has a cold (0 K) surface; the emitting surface is the uniform one, A = 0.3."""
    from tests.test_gpu_camera import small_domain
    case = small_domain()
    ix, iy, iz = np.meshgrid(np.arange(4), np.arange(3), np.arange(2), indexing="ij")
    case["temps"] = 262.0 + 7.0 * ix + 4.3 * iy + 13.7 * iz + 1.1 * ix * iy
    case["lambda_um"] = 10.0
    if patchy:
        case["sfc_temp"] = 0.0
    else:
        case.pop("surface")
        case["albedo"], case["sfc_temp"] = 0.3, 295.0
    return case


# forward 40 x 200000 photons, backward 16 x 16384 paths per pixel: the solar test's counts (DESIGN.md section 4.22 has the figures)
@pytest.mark.parametrize("patchy", [True, False])
def test_reciprocity_with_the_forward_thermal_intensity(patchy):
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = _thermal_small_domain(patchy)
    views = [(1.0, 0.0), (0.6, 110.0)]                          # upward-travelling only
    dom = cases.product_domain(case)
    w = M.new_Weights(dom.numX, dom.numY, dom.numZ)
    flux = M.emission_weighting(dom, w, case["sfc_temp"])       # dLambda = 1: intensity x flux is W m-2 sr-1 um-1
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=9001, minForwardTableSize=1801, LW_flag=1.0, intensityMus=[v[0] for v in views],
                            intensityPhis=[v[1] for v in views], computeIntensity=True, surfaceBDRF=cases.product_surface(case))
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 12), 200000, 40)
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, len(views)))
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    assert len(set(cell.reshape(-1))) == 24 and np.all(sfc == sfc[0, 0]) and (sfc[0, 0] > 0) == (not patchy)
    xe, ye = case["xe"], case["ye"]
    for d, (mu, phi) in enumerate(views):
        cam = _ortho(dom.numX, dom.numY, mu, phi, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=case["ze"][-1])
        out = _render(integ, cam, 16384, 16, cell, sfc, seed=SEED + 1 + d)
        fwd, ferr = st["intensity"][:, :, d].T.astype(np.float64) * flux, st["intensity_StdErr"][:, :, d].T.astype(np.float64) * flux
        bwd, berr = out["radiance"].astype(np.float64), out["radiance_StdErr"].astype(np.float64)
        z = (bwd - fwd) / np.sqrt(ferr ** 2 + berr ** 2)
        mean_err = np.sqrt((ferr ** 2).sum() + (berr ** 2).sum()) / fwd.size
        print("view (%.1f, %.0f): worst pixel %.2f sigma; domain mean forward %.6g backward %.6g, combined error %.3g (%.3f %%), %.2f sigma" % (
            mu, phi, np.abs(z).max(), fwd.mean(), bwd.mean(), mean_err, 100 * mean_err / fwd.mean(), (bwd.mean() - fwd.mean()) / mean_err))
        assert np.all(np.abs(z) < 4.5), z
        assert mean_err < 0.003 * fwd.mean()
        assert abs(bwd.mean() - fwd.mean()) < 4.5 * mean_err
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# invariants: bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene():
    """the thermal small domain with its uniform grey surface, and sources that differ from cell to cell"""
    import mcbrat3d_amd as M
    case = _thermal_small_domain(False)
    dom = cases.product_domain(case)
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    sfc = sfc * np.linspace(0.8, 1.2, 12, dtype=np.float32).reshape(3, 4)
    return case, cell, sfc


def _bytes(out):
    return {k: np.asarray(v).tobytes() for k, v in out.items() if k not in ("emission",)}


SCENE_SENSORS = dict(positions=[(0.1, 0.05, 0.0), (0.33, 0.21, 0.2), (0.4, 0.1, 0.11), (0.02, 0.27, 0.05)],
                     normals=[(0, 0, 1), (0.2, -0.1, -1.0), (1.0, 0.3, 0.2), (0, 0, 1)], kind=["planar", "planar", "planar", "spherical"], ids=[7, 3, 11, 5])


def _scene_sensors(which=slice(None)):
    """on the ground facing up, at the top facing down and aside, tilted inside the medium, and a spherical one"""
    from mcbrat3d_amd.sensors import new_Sensors
    k = SCENE_SENSORS
    return new_Sensors(k["positions"][which], normals=k["normals"][which], kind=k["kind"][which], ids=k["ids"][which])


def test_outputs_do_not_depend_on_where_the_grid_lies_nor_on_how_the_samples_are_split():
    case, cell, sfc = _scene()
    integ, _ = _integrator(case, tables=2001)
    cam = lambda lds=-1: _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)  # noqa: E731  (inside the medium, looking up)
    spp = 1000  # (not a multiple of 64)
    both = [_render(integ, cam(lds), spp, 2, cell, sfc) for lds in (0, 1)]
    assert _bytes(both[0]) == _bytes(both[1])
    two = both[0]["batchMeans"]
    assert two.std() > 0 and np.all(two > 0)
    first, second = (_render(integ, cam(), spp, 1, cell, sfc, first=f)["batchMeans"] for f in (0, spp))
    assert first.tobytes() == two[:1].tobytes() and second.tobytes() == two[1:].tobytes()     # one call = two calls of half the range
    s = _scene_sensors()
    a, b = (_sense(integ, s, spp, 2, cell, sfc, lds=lds) for lds in (0, 1))
    assert _bytes(a) == _bytes(b) and np.all(a["irradiance"] > 0) and np.all(a["irradiance_StdErr"] > 0)
    first, second = (_sense(integ, s, spp, 1, cell, sfc, first=f)["batchMeans"] for f in (0, spp))
    assert first.tobytes() == a["batchMeans"][:1].tobytes() and second.tobytes() == a["batchMeans"][1:].tobytes()
    integ.finalize()


def test_a_sensor_reads_the_same_alone_and_among_others():
    case, cell, sfc = _scene()
    integ, _ = _integrator(case, tables=2001)
    together = _sense(integ, _scene_sensors(), 1000, 2, cell, sfc)
    for i in range(4):
        alone = _sense(integ, _scene_sensors(slice(i, i + 1)), 1000, 2, cell, sfc)
        for k in ("irradiance", "irradiance_StdErr"):
            assert alone[k].tobytes() == together[k][i:i + 1].tobytes(), (i, k)
        assert alone["batchMeans"].tobytes() == np.ascontiguousarray(together["batchMeans"][:, i:i + 1]).tobytes()
    integ.finalize()


def test_the_source_of_the_context_is_not_consulted():
    case, cell, sfc = _scene()
    cam = _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0)
    sensors = _scene_sensors()
    got = []
    for source in ("none", "solar", "thermal"):
        integ, _ = _integrator(case, source=source, tables=2001)
        got.append((_bytes(_render(integ, cam, 500, 2, cell, sfc)), _bytes(_sense(integ, sensors, 500, 2, cell, sfc))))
        integ.finalize()
    assert got[0] == got[1] == got[2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the context is left as it was; refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _camera_struct(**kw):
    from tests.test_gpu_camera import _struct
    return _struct(**kw)


def _sensor_structs(n=1, **kw):
    from mcbrat3d_amd._capi import Sensor
    arr = (Sensor * n)()
    for s in arr:
        s.kind, s.id = 0, 1
        s.position[:], s.e1[:], s.e2[:], s.normal[:] = (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
        for k, v in kw.items():
            if k in ("position", "e1", "e2", "normal"):
                getattr(s, k)[:] = v
            else:
                setattr(s, k, v)
    return arr


CELL8, SFC4 = np.linspace(1.0, 8.0, 8, dtype=np.float32), np.linspace(2.0, 5.0, 4, dtype=np.float32)


def _call_camera(c, cam, cell=CELL8, sfc=SFC4, spp=64, batches=1, n=4):
    rad = np.zeros(max(n, 1), np.float32)
    rc = c.L.mcbrat_render_camera_emission(c.ctx, C.addressof(cam), c.ptr(cell), c.ptr(sfc), SEED, 0, spp, batches, c.ptr(rad), None, None, None)
    return rc, (c.L.mcbrat_last_error(c.ctx).decode() if rc else ""), rad


def _call_sensors(c, arr, cell=CELL8, sfc=SFC4, n=None, samples=64, batches=1, lds=-1):
    n = len(arr) if n is None else n
    irr = np.zeros(max(len(arr), 1), np.float32)
    rc = c.L.mcbrat_render_sensors_emission(c.ctx, n, C.addressof(arr), c.ptr(cell), c.ptr(sfc), SEED, 0, samples, batches, lds, c.ptr(irr), None, None, None)
    return rc, (c.L.mcbrat_last_error(c.ctx).decode() if rc else ""), irr


def _solar_image(c):
    cam = _camera_struct()
    rad, err, means = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(8, np.float32)
    assert c.L.mcbrat_render_camera(c.ctx, C.addressof(cam), SEED, 0, 256, 2, c.ptr(rad), c.ptr(err), c.ptr(means), None) == 0
    return rad.tobytes() + err.tobytes() + means.tobytes()


def test_the_context_is_left_as_it_was():
    from tests.test_gpu_refusal_matrix import Context
    fresh = Context()
    _, reference = fresh.trace()
    fresh.close()
    c = Context()
    before, image = c.state(), _solar_image(c)
    rc, text, rad = _call_camera(c, _camera_struct(), spp=256, batches=2)
    assert rc == 0 and np.all(rad > 0), (rc, text, rad)
    rc, text, irr = _call_sensors(c, _sensor_structs(2), samples=256, batches=2)
    assert rc == 0 and np.all(irr > 0), (rc, text, irr)
    assert c.state() == before and _solar_image(c) == image          # the solar camera before and after: the same bytes
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()    # ... and a trace as a fresh context's
    rc, text, _ = _call_camera(c, _camera_struct(), cell=-CELL8)     # after a refused render too
    assert rc != 0 and c.state() == before
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    c.close()


def test_refusals():
    from tests.test_gpu_camera import REFUSED_CAMERAS
    from tests.test_gpu_refusal_matrix import Context
    P, S = "renderCameraEmission:", "renderSensorsEmission:"
    c = Context()
    before = c.state()

    def refused(result, prefix, *words):
        rc, text, _ = result
        assert rc != 0 and text.startswith(prefix) and all(w in text for w in words), (rc, text, words)

    # the camera's and the sensors' own members, the counts, the budget: the solar entries' rules
    for kw, word in REFUSED_CAMERAS:
        rc, text, _ = _call_camera(c, _camera_struct(**kw))
        assert rc != 0 and word in text and text.startswith(("renderCamera:", P)), (kw, rc, text)  # (camera_refusal words its own prefix)
    refused(_call_camera(c, _camera_struct(), spp=0), P, "samplesPerPixel")
    refused(_call_camera(c, _camera_struct(), batches=0), P, "numBatches")
    refused(_call_camera(c, _camera_struct(npx=32768, npy=32768), batches=2, n=1), P, "tally budget")
    refused(_call_sensors(c, _sensor_structs(1), n=0), S, "at least one sensor")
    refused(_call_sensors(c, _sensor_structs(1), samples=0), S, "samplesPerSensor")
    refused(_call_sensors(c, _sensor_structs(1), batches=0), S, "numBatches")
    refused(_call_sensors(c, _sensor_structs(1), lds=2), S, "gridInLds")
    refused(_call_sensors(c, _sensor_structs(1), n=2 ** 30, batches=2), S, "tally budget")
    for kw, word in ((dict(kind=2), "kind"), (dict(normal=(0.0, 0.0, 0.0)), "normal"), (dict(position=(0.5, np.nan, 0.5)), "finite")):
        rc, text, _ = _call_sensors(c, _sensor_structs(1, **kw))
        assert rc != 0 and word in text, (kw, rc, text)
    refused(_call_sensors(c, _sensor_structs(1, position=(0.5, 0.5, 1.5))), S, "outside the domain")
    # the sources: a null array, a negative value, a NaN, nothing that emits -- each once, for both entries
    bad = CELL8.copy()
    bad[3] = -1.0
    nan = SFC4.copy()
    nan[2] = np.nan
    for call, arg, prefix in ((_call_camera, _camera_struct(), P), (_call_sensors, _sensor_structs(1), S)):
        refused(call(c, arg, cell=None), prefix, "null")
        refused(call(c, arg, sfc=None), prefix, "null")
        refused(call(c, arg, cell=bad), prefix, "cellSource", "negative or not finite")
        refused(call(c, arg, sfc=nan), prefix, "surfaceSource", "negative or not finite")
        refused(call(c, arg, cell=np.zeros(8, np.float32), sfc=np.zeros(4, np.float32)), prefix, "nothing emits")
    assert c.state() == before
    # a BRDF surface
    c.ok(c.setters["rpv"]())
    refused(_call_camera(c, _camera_struct()), P, "BRDF surface")
    refused(_call_sensors(c, _sensor_structs(1)), S, "BRDF surface")
    c.close()
    # a thermal context and one with another solar source are NOT refused: the source rule does not apply
    c = Context(thermal=True)
    assert _call_camera(c, _camera_struct())[0] == 0 and _call_sensors(c, _sensor_structs(1))[0] == 0
    c.close()
    c = Context()
    c.ok(c.L.mcbrat_set_source_random_azimuth(c.ctx, C.c_float(0.5)))
    assert _call_camera(c, _camera_struct())[0] == 0
    c.close()
    # missing pieces: nothing; the grid alone; optics without an inverse table (no forward table is asked for); gridInLds = 1
    # where the grid does not fit
    L, ptr = c.L, c.ptr
    bare = L.mcbrat_create(0)
    bare_ctx = type("Bare", (), dict(L=L, ptr=staticmethod(ptr), ctx=bare))
    e, one = np.array([0.0, 0.5, 1.0]), np.ones(8)
    texts = []
    for step in range(3):
        if step == 1:
            assert L.mcbrat_set_grid(bare, 2, 2, 2, ptr(e), ptr(e), ptr(e)) == 0
        if step == 2:
            assert L.mcbrat_set_optics(bare, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(8, np.int32)), 0.2) == 0
        for call, arg, prefix in ((_call_camera, _camera_struct(), P), (_call_sensors, _sensor_structs(1), S)):
            rc, text, _ = call(bare_ctx, arg)
            assert rc != 0 and (text.startswith(prefix) or step == 2), (step, text)
            texts.append(text)
    assert all("not completely specified" in t for t in texts[:4]) and all("inverse phase function table" in t for t in texts[4:]), texts
    inv = np.zeros(101, np.float32)
    coef = np.zeros(2, np.float32)
    assert L.mcbrat_inverse_table_legendre(len(coef), ptr(coef), len(inv), ptr(inv)) == 0
    assert L.mcbrat_set_inverse_table(bare, 1, len(inv), 1, ptr(inv)) == 0
    assert _call_camera(bare_ctx, _camera_struct())[0] == 0                         # now complete: no source, no forward table
    L.mcbrat_destroy(bare)
    big = L.mcbrat_create(0)
    big_ctx = type("Big", (), dict(L=L, ptr=staticmethod(ptr), ctx=big))
    n = 32
    e, one = np.linspace(0.0, 1.0, n + 1), np.ones(n ** 3)
    assert L.mcbrat_set_grid(big, n, n, n, ptr(e), ptr(e), ptr(e)) == 0
    assert L.mcbrat_set_optics(big, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(n ** 3, np.int32)), 0.2) == 0
    assert L.mcbrat_set_inverse_table(big, 1, len(inv), 1, ptr(inv)) == 0
    cell, sfc = np.ones(n ** 3, np.float32), np.ones(n * n, np.float32)
    refused(_call_camera(big_ctx, _camera_struct(gridInLds=1), cell=cell, sfc=sfc), P, "gridInLds = 1", "do not fit")
    refused(_call_sensors(big_ctx, _sensor_structs(1), cell=cell, sfc=sfc, lds=1), S, "gridInLds = 1", "do not fit")
    L.mcbrat_destroy(big)


# ---------------------------------------------------------------------------------------------------------------------------------
# the namelist driver with emission = .true., end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_namelist_driver_renders_the_emission_camera_and_sensors(tmp_path):
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver_cli, ncio
    case = _thermal_small_domain(False)
    dom = cases.product_domain(case)
    ncio.write_Domain(dom, str(tmp_path / "small.dom"))
    nml, cam_nc, sen_nc = tmp_path / "run.nml", tmp_path / "camera.nc", tmp_path / "sensors.nc"
    nml.write_text("&radiativeTransfer solarMu = 0.5, solarAzimuth = 30., surfaceTemp = 295. /\n"
                   "&monteCarlo numPhotonsPerBatch = 2000, numBatches = 2, iseed = 7, nPhaseIntervals = 2001 /\n"
                   "&fileNames physDomainFile = '%s' /\n"
                   "&camera cameraKind = 'orthographic', cameraPixels = 4, 3, cameraMu = 1., emission = .true., cameraSamplesPerPixel = 512,\n"
                   " cameraBatches = 4, outputCameraFile = '%s' /\n"
                   "&sensors sensorKind = 'planar', sensorPositions = 0.1, 0.05, 0., emission = .true., sensorSamples = 512, sensorBatches = 4,\n"
                   " outputSensorFile = '%s' /\n" % (tmp_path / "small.dom", cam_nc, sen_nc))
    driver_cli.main([str(nml)])
    image, irr = ncio.readCamera_netcdf(str(cam_nc)), ncio.readSensors_netcdf(str(sen_nc))
    cell, sfc = M.planck_sources(dom, 295.0)
    lo, hi = min(cell.min(), sfc.min()), max(cell.max(), sfc.max())
    assert image["cameraEmission"].shape == (3, 4) and np.all(image["cameraEmission"] > 0) and np.all(image["cameraEmission"] < hi)
    assert image["cameraDroppedPaths"] == 0 and irr["sensorDroppedPaths"] == 0
    assert 0 < irr["sensorEmission"][0] < PI * hi and lo > 0
