"""The emission renders with the expected-value estimator on the GPU: the exact cases of section 4.22
under the new entries, zero variance without scattering against an f64 ray-cast written here, agreement with the collision
estimator at statistics, thin air, transport theory, thick cells and the cut, bitwise invariants, the LDS fit edge, refusals, the
namelist driver.  `dropped` is 0 in every render here.  Every test fails without the entries."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_emission import (CHECKER, PI, SEED, VAC, _bytes, _camera_struct, _exact, _integrator, _medium, _ortho, _pinhole, _scene,
                                     _scene_sensors, _sensor_structs, _solar_image, _thermal, _thermal_small_domain, _theory_check, _vacuum_cameras)

pytestmark = pytest.mark.gpu

# Largest relative deviation of a render without scattering from the f64 ray-cast below, measured on the MI355X over every view of
# test_zero_variance_without_scattering and every jittered ray of test_every_jittered_ray_is_its_integral (float face distances,
# float accumulation of the optical depth, expf and expm1f, the float sum of the segments): 5.8e-7, on a jittered ray at mu 0.35
# (jittered: 3.7e-7 at mu 0.05, 1.1e-7 and 2.2e-7 for the pinholes; without jitter: 1.4e-7 at most); times 4 for other compilers,
# the rule of DESIGN.md section 4.19.
RAY_RTOL = 4.0 * 5.8e-7


def _render(integ, cam, spp, batches, cell, sfc, seed=SEED, first=0, estimator="expected"):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderCameraEmission(cam, new_RandomNumberSequence(seed, first), spp, batches, cellSource=cell, surfaceSource=sfc, estimator=estimator)
    assert out["dropped"] == 0 and out["estimator"] == estimator and out["emission"] is True
    return out


def _sense(integ, sensors, n, batches, cell, sfc, seed=SEED, first=0, lds=-1, estimator="expected"):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    out = integ.renderSensorsEmission(sensors, new_RandomNumberSequence(seed, first), n, batches, cellSource=cell, surfaceSource=sfc, gridInLds=lds,
                                      estimator=estimator)
    assert out["dropped"] == 0 and out["estimator"] == estimator
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the f64 reference: the cells a ray crosses, and the formal solution along it
# ---------------------------------------------------------------------------------------------------------------------------------
def ray_cells(o, d, g):
    """f64: the ray from o along d up to the top or the surface -> (ix, iy, iz, t_in, t_out per segment, the column it meets the
    surface in or None at the top, (x, y) there folded into the domain)"""
    xe, ye, ze = g["xe"], g["ye"], g["ze"]
    assert d[2] != 0.0
    t_end = ((ze[-1] if d[2] > 0 else ze[0]) - o[2]) / d[2]
    cuts = [0.0, t_end]
    for e, p, q in ((xe, o[0], d[0]), (ye, o[1], d[1])):
        L = e[-1] - e[0]
        if q != 0.0:
            lo, hi = sorted((p, p + q * t_end))
            for m in range(int(np.floor((lo - e[0]) / L)) - 1, int(np.floor((hi - e[0]) / L)) + 2):
                cuts += [t for t in ((edge + m * L - p) / q for edge in e[:-1]) if 0.0 < t < t_end]
    cuts += [t for t in ((edge - o[2]) / d[2] for edge in ze) if 0.0 < t < t_end]
    cuts = np.unique(cuts)

    def where(t):
        x, y, z = o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t
        x, y = xe[0] + (x - xe[0]) % (xe[-1] - xe[0]), ye[0] + (y - ye[0]) % (ye[-1] - ye[0])
        return [int(np.clip(np.searchsorted(e, v, side="right") - 1, 0, len(e) - 2)) for e, v in ((xe, x), (ye, y), (ze, z))], (x, y)

    segs = [tuple(where(0.5 * (a + b))[0]) + (a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    if d[2] > 0:
        return segs, None, None
    (ix, iy, _), xy = where(t_end)
    return segs, (ix, iy), xy


def ray_emission(o, d, g):
    """f64: sum over the segments E[v] e^(-tau_in) (1 - e^(-dtau)) + e^(-tau_sfc) (1 - a) S_sfc.  g: xe, ye, ze, ext [ix, iy, iz], E
    [iz, iy, ix] (the emission per unit extinction), sfc [iy, ix], albedo"""
    segs, column, _ = ray_cells(o, d, g)
    tau, total = 0.0, 0.0
    for ix, iy, iz, a, b in segs:
        dtau = g["ext"][ix, iy, iz] * (b - a)
        if dtau > 0.0:
            total += g["E"][iz, iy, ix] * np.exp(-tau) * -np.expm1(-dtau)
        tau += dtau
    if column is not None:
        total += np.exp(-tau) * (1.0 - g["albedo"]) * g["sfc"][column[1], column[0]]
    return total


def _float_direction(d):
    return np.asarray(d, np.float32).astype(np.float64)          # the kernel marches along the float direction


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the exact cases of section 4.22, under the new entries
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(_vacuum_cameras()))
def test_vacuum_over_an_emitting_surface_is_exact(which):
    a = 0.3
    integ, _ = _integrator(_medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=a), tables=101)
    cam = _vacuum_cameras()[which]
    out = _render(integ, cam, 197, 2, np.zeros((2, 2, 2), np.float32), CHECKER)
    integ.finalize()
    xe, ye = np.array(VAC["xe"]), np.array(VAC["ye"])
    expected = np.zeros((cam.npy, cam.npx))
    for j in range(cam.npy):
        for i in range(cam.npx):
            o, d = cam.ray(i, j)
            if d[2] > 0:
                continue
            t = (0.0 - o[2]) / d[2]
            hx, hy = (o[0] + d[0] * t) % 0.5, (o[1] + d[1] * t) % 0.5
            expected[j, i] = float(np.float32(np.float32(1.0) - np.float32(a)) * CHECKER[int(hy >= ye[1]), int(hx >= xe[1])])
    seen = expected > 0
    assert seen.any() == (which != "orthographic looking up")
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
    assert np.all(out["irradiance_StdErr"] == 0.0) and out["batchMeans"].shape == (2, 3)
    emitted = float(np.float32(np.float32(1.0) - np.float32(a)) * np.float32(s_sfc))
    assert _exact(out["irradiance"][0], PI * emitted, s_sfc, PI), out["irradiance"]   # facing down at zMax: pi (1 - a) S_sfc
    assert out["irradiance"][1] == 0.0 and out["irradiance"][2] == 0.0                # facing up: exactly nothing


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. zero variance without scattering: the defining property
# ---------------------------------------------------------------------------------------------------------------------------------
def _absorbing(albedo):
    """3 x 2 x 2, unequal edges, omega0 = 0, another extinction and another source in every cell, one vacuum cell, an emitting
    surface with another source in every column -> (the case, cellSource, surfaceSource, the reference's grid)"""
    xe, ye, ze = np.array([0.0, 0.25, 0.35, 0.6]), np.array([0.0, 0.25, 0.4]), np.array([0.0, 0.1, 0.25])
    ext = np.array([[[1.5, 4.0], [0.7, 2.2]], [[6.0, 0.0], [3.1, 5.3]], [[2.5, 0.4], [8.0, 1.1]]])     # [ix, iy, iz]; (1, 0, 1) is a vacuum
    cell = (2.0 + 1.375 * np.arange(12, dtype=np.float64).reshape(2, 2, 3) % 7.0 + 0.25 * np.arange(12).reshape(2, 2, 3)).astype(np.float32)
    sfc = np.array([[1.0, 7.5, 3.25], [9.0, 0.5, 4.75]], np.float32)
    assert len(set(ext.reshape(-1))) == 12 and len(set(cell.reshape(-1))) == 12 and len(set(sfc.reshape(-1))) == 6
    E = np.where(ext.transpose(2, 1, 0) > 0, cell.astype(np.float64), 0.0)
    return _medium(xe, ye, ze, ext, ssa=0.0, albedo=albedo), cell, sfc, dict(xe=xe, ye=ye, ze=ze, ext=ext, E=E, sfc=sfc.astype(np.float64), albedo=albedo)


def _absorbing_views():
    fp = (0.0, 0.6, 0.0, 0.4)
    return {  # name -> (albedo, camera)
        "nadir": (0.0, lambda **kw: _ortho(3, 2, 1.0, 0.0, footprint=fp, height=0.25, **kw)),
        "mu 0.35": (0.0, lambda **kw: _ortho(3, 2, 0.35, 110.0, footprint=fp, height=0.25, **kw)),
        "mu 0.05": (0.0, lambda **kw: _ortho(3, 2, 0.05, 33.0, footprint=fp, height=0.25, **kw)),       # through many periodic wraps
        "pinhole looking down": (0.0, lambda **kw: _pinhole(3, 2, (0.13, 0.21, 0.17), (0.3, -0.2, -1.0), fov=70.0, **kw)),
        "pinhole looking up": (0.3, lambda **kw: _pinhole(3, 2, (0.13, 0.21, 0.04), (0.2, 0.1, 1.0), fov=70.0, **kw)),   # never sees the surface
    }


def _deviation(got, want, src_max):
    """relative, less the fixed-point step and the rounding of the mean to a float"""
    return float(np.max(np.maximum(np.abs(np.asarray(got, np.float64) - want) - src_max * 2.0 ** -40 - np.abs(want) * 2.0 ** -24, 0.0) / np.abs(want)))


@pytest.mark.parametrize("which", sorted(_absorbing_views()))
def test_zero_variance_without_scattering(which):
    albedo, make = _absorbing_views()[which]
    case, cell, sfc, g = _absorbing(albedo)
    cam = make(jitter=False)
    integ, _ = _integrator(case, tables=101)
    out = _render(integ, cam, 3, 4, cell, sfc)
    integ.finalize()
    want = np.zeros((cam.npy, cam.npx))
    for j in range(cam.npy):
        for i in range(cam.npx):
            o, d = cam.ray(i, j)
            want[j, i] = ray_emission(np.asarray(o, np.float64), _float_direction(d), g)
    means = out["batchMeans"]
    assert np.all(out["radiance_StdErr"] == 0.0)
    assert all(means[b].tobytes() == means[0].tobytes() for b in range(4)) and out["radiance"].tobytes() == means[0].tobytes()
    dev = _deviation(out["radiance"], want, float(max(cell.max(), sfc.max())))
    print("%s: largest relative deviation from the f64 ray-cast %.3g (tolerance %.3g); image %s" % (which, dev, RAY_RTOL, out["radiance"].reshape(-1)))
    assert np.all(want > 0) and len(set(np.round(want.reshape(-1), 6))) == want.size     # every pixel another value
    assert dev <= RAY_RTOL


@pytest.mark.parametrize("which", ["mu 0.05", "mu 0.35", "pinhole looking down", "pinhole looking up"])
def test_every_jittered_ray_is_its_integral(which):
    """jitter = 1, one sample per pixel and batch, 64 batches: every batch mean is one ray, mcbrat_camera_ray at the sample's Philox jitter"""
    from tests.test_gpu_sources import philox, u01
    albedo, make = _absorbing_views()[which]
    case, cell, sfc, g = _absorbing(albedo)
    cam = make(jitter=True)
    nb = 64
    integ, _ = _integrator(case, tables=101)
    out = _render(integ, cam, 1, nb, cell, sfc)
    integ.finalize()
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    want = np.zeros((nb, cam.npy, cam.npx))
    ids = np.arange(nb, dtype=np.uint64)
    zero = np.zeros(nb, np.uint64)
    for j in range(cam.npy):
        for i in range(cam.npx):
            jit = philox([zero, zero + np.uint64(j * cam.npx + i), ids, zero], key)      # event 0, the pixel, the sample
            u, v = u01(jit[0]).astype(np.float64), u01(jit[1]).astype(np.float64)
            for b in range(nb):
                o, d = cam.ray(i, j, float(u[b]), float(v[b]))
                want[b, j, i] = ray_emission(np.asarray(o, np.float64), _float_direction(d), g)
    dev = _deviation(out["batchMeans"], want, float(max(cell.max(), sfc.max())))
    print("jittered rays, %s: largest relative deviation from the f64 ray-cast %.3g (tolerance %.3g)" % (which, dev, RAY_RTOL))
    assert np.all(out["radiance_StdErr"] > 0.0)              # the rays differ; each of them is exact
    assert dev <= RAY_RTOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every sample recomputed: the one-pixel pinhole of tests/test_gpu_emission.py::test_every_sample_is_recomputed, as it is
# ---------------------------------------------------------------------------------------------------------------------------------
def every_sample_reference(seed, truncated=False):
    """-> (the deposit of every sample [n]: the f64 integral along its whole ray -- `truncated`, a misstated rule: only up to the
    collision point --, whether an event of the sample lies within 1e-3 of a face, relative to its cell).  Host arithmetic only:
    the path is replayed from Philox as tests/test_gpu_emission.sample_by_sample_reference replays it (omega0 = 0: one leg)."""
    from tests.test_gpu_emission import SBS, SBS_BATCHES, SBS_N, _first_event, _sbs_camera
    from tests.test_gpu_sources import philox, u01
    cam = _sbs_camera()
    n = SBS_N * SBS_BATCHES
    ids = np.arange(n, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros(n, np.uint64)
    jit = philox([zero, zero, ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], key)
    leg = philox([zero + np.uint64(1), zero, ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], key)
    u, v = u01(jit[0]).astype(np.float64), u01(jit[1]).astype(np.float64)
    tiny = np.float32(np.finfo(np.float32).tiny)
    tau = np.maximum(-np.log(np.maximum(u01(leg[0]), tiny)), tiny).astype(np.float64)
    g = dict(xe=SBS["xe"], ye=SBS["ye"], ze=SBS["ze"], ext=SBS["ext"], E=SBS["cell"].astype(np.float64), sfc=SBS["sfc"].astype(np.float64), albedo=0.0)
    deposits, near = np.zeros(n), np.zeros(n, bool)
    for k in range(n):
        o, d = cam.ray(0, 0, float(u[k]), float(v[k]))
        o, d = np.asarray(o, np.float64), _float_direction(d)
        _, rel = _first_event(o, d, float(tau[k]), SBS)
        near[k] = rel < 1e-3
        if not truncated:
            deposits[k] = ray_emission(o, d, g)
            continue
        segs, column, _ = ray_cells(o, d, g)
        acc = 0.0
        for ix, iy, iz, a, b in segs:
            dtau = g["ext"][ix, iy, iz] * (b - a)
            part = min(dtau, float(tau[k]) - acc)
            deposits[k] += g["E"][iz, iy, ix] * np.exp(-acc) * -np.expm1(-part)
            acc += part
            if part < dtau:
                break
        else:
            if column is not None:
                deposits[k] += np.exp(-acc) * g["sfc"][column[1], column[0]]
    return deposits, near


def test_every_sample_is_recomputed():
    """One sample per batch: batchMeans is every path's own sum; every path is held to the f64 integral along its whole ray
    (measured on the MI355X: 1.8e-7 at most).  No
    sample of this seed has an event within 1e-3 of a face (checked on the CPU: the cap is 3 %).  The two-component variant with
    scattering is test_every_sample_of_a_scattering_path_is_recomputed."""
    from tests.test_gpu_emission import SBS, SBS_BATCHES, SBS_N, SBS_SEED, _sbs_camera
    n = SBS_N * SBS_BATCHES
    want, near = every_sample_reference(SBS_SEED)
    assert near.mean() <= 0.03, near.mean()                  # the cap on what may be left out: the reference alone stays within it
    integ, _ = _integrator(_medium(SBS["xe"], SBS["ye"], SBS["ze"], SBS["ext"], ssa=0.0, albedo=0.0), tables=101)
    per_path = _render(integ, _sbs_camera(), 1, n, SBS["cell"], SBS["sfc"], seed=SBS_SEED)["batchMeans"].reshape(n).astype(np.float64)
    batches = _render(integ, _sbs_camera(), SBS_N, SBS_BATCHES, SBS["cell"], SBS["sfc"], seed=SBS_SEED)["batchMeans"].reshape(SBS_BATCHES).astype(np.float64)
    integ.finalize()
    src_max = float(SBS["cell"].max())
    legs = 1                                                 # omega0 = 0: every path is one leg
    tol = RAY_RTOL * legs * want + src_max * 2.0 ** -40 + want * 2.0 ** -24
    dev = np.abs(per_path - want)
    print("every sample: largest relative deviation %.3g (tolerance %.3g); %d of %d samples within 1e-3 of a face, %d of them outside" % (
        (dev / want)[~near].max(), RAY_RTOL, near.sum(), n, (dev > tol)[near].sum()))
    assert np.all(dev[~near] <= tol[~near])
    # the batches of 197 are the means of these paths (the pending-bin and wave-reduction paths, which a one-sample render skips)
    assert np.all(np.abs(batches - per_path.reshape(SBS_BATCHES, SBS_N).mean(axis=1)) <= SBS_N * 2.0 ** -24 * batches)
    # a misstated rule is seen: a deposit that stops at the collision point moves more than half of the samples beyond the tolerance
    wrong, _ = every_sample_reference(SBS_SEED, truncated=True)
    assert (np.abs(per_path - wrong) > tol)[~near].mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. the same pinhole over two components (omega0 = 0.9 and 0.3) and a reflecting surface: the whole path replayed
# ---------------------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def _fma(a, b, c):
    """fmaf: the product of two floats is exact in double"""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _cos_sin_kernels(r):
    z = r * r
    c = _fma(z, _fma(z, _fma(z, _fma(z, F32(2.43904487962774090654e-5), F32(-1.38867637746099294692e-3)), F32(4.16666233237390631894e-2)),
                     F32(-0.499999997251031003120)), F32(1.0))
    s = _fma(r * z, _fma(z, _fma(z, _fma(z, F32(2.7183114939898219064e-6), F32(-1.98393348360966317347e-4)), F32(8.3333293858894631756e-3)),
                         F32(-0.166666666416265235595)), r)
    return c, s


def _cos_0_pi(x):
    """mcbrat_photon.h: cos_0_pi, in float"""
    q = np.rint(x * F32(0.636619772))
    r = _fma(q, F32(-1.57079637050628662109375), x)
    r = _fma(q, F32(4.371138828673793e-8), r)
    c, s = _cos_sin_kernels(r)
    return c if q == 0 else (-s if q == 1 else -c)


def _sincos_2pi(u):
    """mcbrat_photon.h: sincos_2pi, in float -> (cos, sin)"""
    q = np.rint(F32(4.0) * u)
    r = (u - F32(0.25) * q) * F32(6.28318548202514648)
    cc, ss = _cos_sin_kernels(r)
    qi = int(q) & 3
    return ((cc, ss), (-ss, cc), (-cc, -ss), (ss, -cc))[qi]


TWO = dict(share=np.array([[[0.3, 0.55]], [[0.6, 0.4]]]), ssa=(0.9, 0.3), albedo=0.3, table=9001)   # share: of component 0 in the extinction, [ix, iy, iz]
# (the seed: the first candidate tried on the CPU, section 4.22's; 3 of its 591 samples have an event within 1e-3 of a face, 0.5 %)
TWO_SEED = 20261026


def two_component_case():
    """-> (the case, the reference's grid): SBS's grid and extinction split between an isotropic component of omega0 = 0.9 and one of 0.3"""
    from tests.test_gpu_emission import SBS
    from oracle import oracle as O
    e0, e1 = SBS["ext"] * TWO["share"], SBS["ext"] * (1.0 - TWO["share"])
    comps = [dict(ext=e, ssa=np.full_like(e, w0), pfIndex=np.ones(e.shape, np.int32), legendre=[cases.hg_legendre(0.0, 2)]) for e, w0 in ((e0, TWO["ssa"][0]), (e1, TWO["ssa"][1]))]
    case = dict(name="two", xe=SBS["xe"], ye=SBS["ye"], ze=SBS["ze"], albedo=TWO["albedo"], components=comps)
    tot, cum, ssa, _ = O.optical_properties_by_component(2, 1, 2, comps)
    cum, ssa = cum.reshape(2, 2, 1, 2).astype(F32), ssa.reshape(2, 2, 1, 2).astype(F32)          # [c, iz, iy, ix], the floats the kernel reads
    S = SBS["cell"].astype(np.float64)
    absorb = [1.0 - ssa[c].astype(np.float64) for c in range(2)]
    f0 = cum[0].astype(np.float64)
    g = dict(xe=SBS["xe"], ye=SBS["ye"], ze=SBS["ze"], ext=tot.reshape(2, 1, 2).transpose(2, 1, 0), cum=cum, ssa=ssa, S=S,
             E=S * (f0 * absorb[0] + (1.0 - f0) * absorb[1]), Ec=[S * absorb[0], S * absorb[1]], sfc=SBS["sfc"].astype(np.float64),
             albedo=float(F32(TWO["albedo"])))
    return case, g


def replay_paths(seed, n, g, table, rule="expected"):
    """Host arithmetic only: the paths of the one-pixel pinhole, sample 0 .. n - 1, replayed from Philox with the kernel's rules (the
    weights, the roulette and the new direction in float as the kernel forms them, positions and optical depths in double).  Every
    leg deposits, with the weight it starts with, the f64 integral along its whole ray.  rule: "expected"; or one of two misstated
    rules -- "truncated": the integral stops at the collision point; "picked": (1 - omega0) of the component picked at the leg's
    collision (component 0 where there is none) instead of E[v].
    -> (the sum of every path, the number of its legs, whether one of its events lies within 1e-3 of a face)"""
    from tests.test_gpu_emission import _sbs_camera
    from tests.test_gpu_sources import philox, u01
    cam = _sbs_camera()
    key = (seed & 0xFFFFFFFF, seed >> 32)
    xe, ye, ze = g["xe"], g["ye"], g["ze"]
    tiny = F32(np.finfo(np.float32).tiny)
    nt = table.shape[-1]
    inv_n = F32(1.0) / F32(nt)
    sums, legs, near = np.zeros(n), np.zeros(n, int), np.zeros(n, bool)

    def block(event, k):
        q = philox([np.array([event], np.uint64), np.zeros(1, np.uint64), np.array([k & 0xFFFFFFFF], np.uint64), np.array([k >> 32], np.uint64)], key)
        return [u01(x)[0] for x in q]

    def rel_to_faces(point, cell, axes):
        out = 1.0
        for e, v, i in axes:
            v = e[0] + (v - e[0]) % (e[-1] - e[0]) if e is not ze else v
            out = min(out, (v - e[i]) / (e[i + 1] - e[i]), (e[i + 1] - v) / (e[i + 1] - e[i]))
        return out

    for k in range(n):
        u, v = block(0, k)[:2]
        o, d = cam.ray(0, 0, float(u), float(v))
        pos, d = np.asarray(o, np.float64), np.asarray(d, F32)
        w = F32(1.0)
        for event in range(1, 100000):
            q = block(event, k)
            tau = float(max(-np.log(max(q[0], tiny)), tiny))
            uX, uY, uZ = q[1], q[2], q[3]
            d64 = d.astype(np.float64)
            segs, column, xy = ray_cells(pos, d64, g)
            legs[k] += 1
            acc, hit = 0.0, None
            for ix, iy, iz, a, b in segs:
                e = g["ext"][ix, iy, iz]
                if e > 0.0 and acc + e * (b - a) >= tau:
                    hit = (a + (tau - acc) / e, ix, iy, iz)
                    break
                acc += e * (b - a)
            c = 0
            if hit is not None:
                t, ix, iy, iz = hit
                point = pos + d64 * t
                near[k] |= rel_to_faces(point, None, ((xe, point[0], ix), (ye, point[1], iy), (ze, point[2], iz))) < 1e-3
                for kc in range(g["cum"].shape[0] - 1):
                    if uZ >= g["cum"][kc][iz, iy, ix]:
                        c = kc + 1
            else:
                near[k] |= (tau - acc) / acc < 1e-3 if acc > 0.0 else False
                if column is not None:
                    near[k] |= rel_to_faces(None, None, ((xe, xy[0], column[0]), (ye, xy[1], column[1]))) < 1e-3
            # the leg's deposit, with the weight it starts with
            E = g["Ec"][c] if rule == "picked" else g["E"]
            tau_in, total = 0.0, 0.0
            for jx, jy, jz, a, b in segs:
                if rule == "truncated" and hit is not None and a >= hit[0]:
                    break
                if rule == "truncated" and hit is not None:
                    b = min(b, hit[0])
                dtau = g["ext"][jx, jy, jz] * (b - a)
                if dtau > 0.0:
                    total += E[jz, jy, jx] * np.exp(-tau_in) * -np.expm1(-dtau)
                tau_in += dtau
            if column is not None and not (rule == "truncated" and hit is not None):
                total += np.exp(-tau_in) * (1.0 - g["albedo"]) * g["sfc"][column[1], column[0]]
            sums[k] += float(w) * total
            if hit is None:
                if column is None:
                    break                                                        # out of the top
                w = w * F32(g["albedo"])
                if not w > 0.0:
                    break
                mu = np.sqrt(uX)
                if mu == 0.0:
                    mu = max(np.sqrt(uZ), F32(1.52587890625e-05))
                sin_t = np.sqrt(F32(1.0) - mu * mu)
                cphi, sphi = _sincos_2pi(uY)
                t_end = (ze[0] - pos[2]) / d64[2]
                pos = np.array([pos[0] + d64[0] * t_end, pos[1] + d64[1] * t_end, ze[0] + np.finfo(np.float64).tiny])
                d = np.array([sin_t * cphi, sin_t * sphi, mu], F32)
                continue
            pos = point
            w = w * g["ssa"][c][iz, iy, ix]
            if not w > 0.0:
                break
            if w < 0.5:                                                          # Russian roulette, block 1 of the event
                uR = block(event | (1 << 24), k)[1]
                if uR >= w:
                    break
                w = F32(1.0)
            tb = table[c]
            ai = int(uX * F32(nt)) + 1
            if ai < nt:
                left = uX - F32(ai - 1) * inv_n
                ang = (F32(1.0) - left) * tb[ai - 1] + left * tb[ai]
            else:
                ang = tb[nt - 1]
            cs = _cos_0_pi(ang)
            AX, AY = _sincos_2pi(uY)
            B = np.sqrt(max(F32(1.0) - cs * cs, F32(0.0)))
            AX, AY = AX * B, AY * B
            B = d[0] * AX - d[1] * AY
            D = cs - B / (F32(1.0) + abs(d[2]))
            d = np.array([d[0] * D + AX, d[1] * D - AY, d[2] * cs - np.copysign(abs(B), d[2] * B)], F32)
    return sums, legs, near


def _two_component_reference(rule="expected"):
    from tests.test_gpu_emission import SBS_BATCHES, SBS_N
    case, g = two_component_case()
    dom = cases.product_domain(case)
    table = np.stack([np.asarray(t, F32)[0] for t in dom.tabulateInversePhaseFunctions(TWO["table"])])    # the product's own tables: the kernel's input
    assert table.shape == (2, TWO["table"])
    return (case, g) + replay_paths(TWO_SEED, SBS_N * SBS_BATCHES, g, table, rule)


def test_every_sample_of_a_scattering_path_is_recomputed():
    """Two components (omega0 = 0.9 and 0.3, isotropic) over a surface of albedo 0.3; one sample per batch: batchMeans is every
    path's own sum, held to the replay within the ray-cast's tolerance times the largest number of legs of a path.  A cap, not a
    measurement: samples with an event within 1e-3 of a face are left out, at most 3 % of them.  Measured on the MI355X: up to 8
    legs, the largest relative deviation 6.2e-7 (tolerance 1.9e-5), 3 of 591 samples left out; a deposit that stops at the
    collision point moves 90.8 % of the samples beyond the tolerance, (1 - omega0) of the picked component all of them."""
    from tests.test_gpu_emission import SBS, SBS_BATCHES, SBS_N, _sbs_camera
    n = SBS_N * SBS_BATCHES
    case, g, want, legs, near = _two_component_reference()
    assert near.mean() <= 0.03, near.mean()
    assert legs.max() >= 5 and (legs > 1).mean() > 0.5       # the paths scatter and reflect: most have more than one leg
    integ, _ = _integrator(case, tables=TWO["table"])
    per_path = _render(integ, _sbs_camera(), 1, n, SBS["cell"], SBS["sfc"], seed=TWO_SEED)["batchMeans"].reshape(n).astype(np.float64)
    batches = _render(integ, _sbs_camera(), SBS_N, SBS_BATCHES, SBS["cell"], SBS["sfc"], seed=TWO_SEED)["batchMeans"].reshape(SBS_BATCHES).astype(np.float64)
    integ.finalize()
    src_max = float(max(SBS["cell"].max(), SBS["sfc"].max()))
    tol = RAY_RTOL * legs.max() * want + src_max * 2.0 ** -40 + want * 2.0 ** -24
    dev = np.abs(per_path - want)
    keep = ~near
    print("scattering paths: up to %d legs; largest relative deviation %.3g (tolerance %.3g); %d of %d samples within 1e-3 of a face, %d of them outside" % (
        legs.max(), (dev / want)[keep].max(), RAY_RTOL * legs.max(), near.sum(), n, (dev > tol)[near].sum()))
    assert np.all(dev[keep] <= tol[keep]), "%d samples outside the tolerance, the worst by %.3g" % ((dev > tol)[keep].sum(), (dev / tol)[keep].max())
    assert np.all(np.abs(batches - per_path.reshape(SBS_BATCHES, SBS_N).mean(axis=1)) <= SBS_N * 2.0 ** -24 * batches)
    # the same replay sees a misstated rule: each moves more than half of the samples beyond the tolerance
    for rule in ("truncated", "picked"):
        wrong = _two_component_reference(rule)[2]
        moved = (np.abs(per_path - wrong) > tol)[keep].mean()
        print("   rule '%s': %.1f %% of the samples beyond the tolerance" % (rule, 100.0 * moved))
        assert moved > 0.5, (rule, moved)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the two estimators agree at statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def _agree(what, a, ea, b, eb, each=4.5, mean=3.0):
    a, ea, b, eb = (np.asarray(x, np.float64) for x in (a, ea, b, eb))
    z = (a - b) / np.sqrt(ea ** 2 + eb ** 2)
    mean_err = np.sqrt((ea ** 2).sum() + (eb ** 2).sum()) / a.size
    zm = (a.mean() - b.mean()) / mean_err
    print("%s: worst %.2f sigma; mean expected %.6g collision %.6g (%.2f sigma); standard errors expected / collision %s" % (
        what, np.abs(z).max(), a.mean(), b.mean(), zm, np.round(ea / eb, 3).reshape(-1)))
    assert np.all(np.abs(z) < each), z
    assert abs(zm) < mean


def test_the_two_estimators_agree_at_statistics():
    from mcbrat3d_amd.sensors import new_Sensors
    import mcbrat3d_amd as M
    case = _thermal_small_domain(False)
    dom = cases.product_domain(case)
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    integ, _ = _integrator(case, tables=9001)
    xe, ye, ze = case["xe"], case["ye"], case["ze"]
    for d, (mu, phi) in enumerate([(1.0, 0.0), (0.6, 110.0)]):
        cam = _ortho(dom.numX, dom.numY, mu, phi, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=ze[-1])
        x, c = (_render(integ, cam, 4096, 16, cell, sfc, seed=SEED + 1 + d, estimator=e) for e in ("expected", "collision"))
        _agree("view (%.1f, %.0f)" % (mu, phi), x["radiance"], x["radiance_StdErr"], c["radiance"], c["radiance_StdErr"])
    mid = 0.5 * (ze[0] + ze[-1])
    sensors = new_Sensors([(0.1, 0.05, mid), (0.33, 0.21, mid), (0.4, 0.1, mid)], normals=[(0, 0, 1), (0.2, -0.1, -1.0), (0, 0, 1)],
                          kind=["planar", "planar", "spherical"])
    x, c = (_sense(integ, sensors, 4096, 16, cell, sfc, estimator=e) for e in ("expected", "collision"))
    integ.finalize()
    _agree("sensors", x["irradiance"], x["irradiance_StdErr"], c["irradiance"], c["irradiance_StdErr"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. thin air, where it pays
# ---------------------------------------------------------------------------------------------------------------------------------
def thin_column():
    """a 2 x 2 x 4 clear-sky column: gas of total optical depth 0.02, omega0 = 0.2, colder with height, over a cold black surface
    -> (the case, cellSource, surfaceSource)"""
    xe, ye, ze = np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    ext = np.full((2, 2, 4), 0.02)
    level = np.array([9.5, 8.0, 6.75, 5.5])
    cell = (level[:, None, None] * (1.0 + 0.02 * np.arange(4).reshape(2, 2))[None]).astype(np.float32)
    return _medium(xe, ye, ze, ext, ssa=0.2, albedo=0.0), cell, np.zeros((2, 2), np.float32)


def test_thin_air_is_where_it_pays():
    case, cell, sfc = thin_column()
    integ, _ = _integrator(case, tables=101)
    cam = _ortho(2, 2, 1.0, 0.0, footprint=(0.0, 1.0, 0.0, 1.0), height=1.0)
    x, c = (_render(integ, cam, 256, 8, cell, sfc, estimator=e) for e in ("expected", "collision"))
    integ.finalize()
    ratio = c["radiance_StdErr"].astype(np.float64) / x["radiance_StdErr"].astype(np.float64)
    print("thin column: expected %s +- %s, collision %s +- %s; standard errors collision / expected %s" % (
        x["radiance"].reshape(-1), x["radiance_StdErr"].reshape(-1), c["radiance"].reshape(-1), c["radiance_StdErr"].reshape(-1), ratio.reshape(-1)))
    z = (x["radiance"].astype(np.float64) - c["radiance"]) / np.sqrt(x["radiance_StdErr"].astype(np.float64) ** 2 + c["radiance_StdErr"].astype(np.float64) ** 2)
    assert np.all(np.abs(z) < 4.5), z
    assert np.all(x["radiance_StdErr"] < c["radiance_StdErr"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. transport theory
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_against_theory(what, value, err, theory, src_max, w0=1.0, omega=None):
    """_theory_check, the criterion of the collision estimator's tests: exact where every batch gives the same value, the power
    condition and 4.5 standard errors otherwise.  Without scattering this estimator has no statistical spread at all: where the
    jitter moves a ray across a column, the batches are the same integral summed over faces at other distances and differ in
    the float's last bit (measured on the absorbing slab at mu 0.7: a standard error of 5.8e-18 on 4.2e-8, 1.4e-10 relative, the
    value 1.7e-9 from theory).  A standard error below one unit in the last place of the value is that rounding, not a spread:
    such batches count as the same value and are held to the exact branch, which is the stricter of the two."""
    same = err <= abs(value) * 2.0 ** -23
    assert not same or omega == 0.0, (what, err, value)         # only a medium that does not scatter has no spread
    if same and err > 0.0:
        print("%s: standard error %.3g, %.3g of the value: the rounding of equal batches" % (what, err, err / abs(value)))
    _theory_check(what, value, 0.0 if same else err, theory, src_max, w0)


@pytest.mark.parametrize("tau,omega,temps,sfc", __import__("tests.test_analytic", fromlist=["THERMAL_SLABS"]).THERMAL_SLABS)
def test_radiance_at_the_top_of_an_emitting_slab(tau, omega, temps, sfc):
    from tests.test_analytic import RADIANCE_MUS, RADIANCE_PHIS, planck, thermal_radiance
    case, cell, sfc_src, total = _thermal(tau, omega, temps, sfc)
    theory = thermal_radiance(tau, omega, planck(10.0, np.asarray(temps)[::-1]), float(planck(10.0, sfc)), RADIANCE_MUS) * total
    integ, _ = _integrator(case, tables=101)
    outs = [_render(integ, _ortho(1, 1, mu, phi, footprint=(0.0, 0.6, 0.0, 0.6), height=0.6), 16384, 16, cell, sfc_src) for mu, phi in zip(RADIANCE_MUS, RADIANCE_PHIS)]
    integ.finalize()
    for mu, out, th in zip(RADIANCE_MUS, outs, theory):
        _check_against_theory("mu %.2f" % mu, float(out["radiance"][0, 0]), float(out["radiance_StdErr"][0, 0]), float(th), float(max(cell.max(), sfc_src.max())),
                              omega=omega)


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
    _check_against_theory("actinic flux", float(out["irradiance"][0]), float(out["irradiance_StdErr"][0]), theory, B, 4.0 * PI, omega=0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. thick cells and the cut
# ---------------------------------------------------------------------------------------------------------------------------------
def test_thick_cells_and_the_cut():
    xe, ye, ze = np.array([0.0, 0.5]), np.array([0.0, 0.5]), np.array([0.0, 0.5, 1.0])
    ext = np.full((1, 1, 2), 400.0)                            # an optical depth of 200 per cell
    cell, sfc = np.array([1.0, 2.0], np.float32).reshape(2, 1, 1), np.full((1, 1), 0.5, np.float32)
    down = _ortho(1, 1, 1.0, 0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=1.0)
    up = _ortho(1, 1, -1.0, 0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.0)
    integ, _ = _integrator(_medium(xe, ye, ze, ext, ssa=0.0, albedo=0.0), tables=101)
    for cam, want in ((down, 2.0), (up, 1.0)):
        out = _render(integ, cam, 64, 2, cell, sfc)
        v = out["radiance"][0, 0]
        print("thick cells: reads %r, the cell's source %r" % (v, want))
        assert np.isfinite(v) and abs(np.float64(v) - want) <= np.spacing(np.float32(want)) and out["radiance_StdErr"][0, 0] == 0.0
    integ.finalize()
    integ, _ = _integrator(_medium(xe, ye, ze, ext, ssa=0.999, albedo=0.0), tables=101)
    for cam in (down, up):
        out = _render(integ, cam, 64, 2, cell, sfc)            # (dropped == 0: _render)
        assert np.all(np.isfinite(out["radiance"])) and np.all(np.isfinite(out["radiance_StdErr"])) and 0.0 < out["radiance"][0, 0] < 4.0
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. determinism and placement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_where_the_grids_lie_nor_on_how_the_samples_are_split():
    case, cell, sfc = _scene()
    integ, _ = _integrator(case, tables=2001)
    cam = lambda lds=-1: _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)  # noqa: E731  (inside the medium, looking up)
    spp = 200  # (not a multiple of 64)
    both = [_render(integ, cam(lds), spp, 2, cell, sfc) for lds in (0, 1)]
    assert _bytes(both[0]) == _bytes(both[1])
    two = both[0]["batchMeans"]
    assert two.std() > 0 and np.all(two > 0)
    first, second = (_render(integ, cam(), spp, 1, cell, sfc, first=f)["batchMeans"] for f in (0, spp))
    assert first.tobytes() == two[:1].tobytes() and second.tobytes() == two[1:].tobytes()     # one call = two calls of half the range
    collision = _render(integ, cam(), spp, 2, cell, sfc, estimator="collision")
    assert collision["batchMeans"].tobytes() != two.tobytes()                                   # (another estimator, not another name)
    s = _scene_sensors()
    a, b = (_sense(integ, s, spp, 2, cell, sfc, lds=lds) for lds in (0, 1))
    assert _bytes(a) == _bytes(b) and np.all(a["irradiance"] > 0) and np.all(a["irradiance_StdErr"] > 0)
    first, second = (_sense(integ, s, spp, 1, cell, sfc, first=f)["batchMeans"] for f in (0, spp))
    assert first.tobytes() == a["batchMeans"][:1].tobytes() and second.tobytes() == a["batchMeans"][1:].tobytes()
    # a sensor reads the same alone and among others
    for i in range(4):
        alone = _sense(integ, _scene_sensors(slice(i, i + 1)), spp, 2, cell, sfc)
        for k in ("irradiance", "irradiance_StdErr"):
            assert alone[k].tobytes() == a[k][i:i + 1].tobytes(), (i, k)
        assert alone["batchMeans"].tobytes() == np.ascontiguousarray(a["batchMeans"][:, i:i + 1]).tobytes()
    integ.finalize()


def test_the_lds_fit_edge():
    """24 x 24 x 24: one grid of 55 KB fits the share of 79 KB, the pair of 110 KB does not"""
    import mcbrat3d_amd as M
    from mcbrat3d_amd.sensors import new_Sensors
    n = 24
    e = np.linspace(0.0, 1.0, n + 1)
    rng = np.random.default_rng(24)
    ext = rng.uniform(0.5, 3.0, (n, n, n))
    cell, sfc = rng.uniform(1.0, 9.0, (n, n, n)).astype(np.float32), rng.uniform(1.0, 9.0, (n, n)).astype(np.float32)
    integ, _ = _integrator(_medium(e, e, e, ext, ssa=0.5, albedo=0.1), tables=101)
    cam = lambda lds: _pinhole(2, 2, (0.31, 0.42, 0.55), (0.3, 0.1, -1.0), fov=60.0, gridInLds=lds)  # noqa: E731
    sensors = new_Sensors([(0.3, 0.4, 0.5)], kind="spherical")
    assert _render(integ, cam(1), 16, 1, cell, sfc, estimator="collision")["radiance"].min() > 0        # the collision entry accepts it
    _sense(integ, sensors, 16, 1, cell, sfc, lds=1, estimator="collision")
    with pytest.raises(M.McbratError, match=r"^renderCameraEmissionExpected: gridInLds = 1, but the extinction grid and the emission grid do not fit"):
        _render(integ, cam(1), 16, 1, cell, sfc)
    with pytest.raises(M.McbratError, match=r"^renderSensorsEmissionExpected: gridInLds = 1, but the extinction grid and the emission grid do not fit"):
        _sense(integ, sensors, 16, 1, cell, sfc, lds=1)
    a, b = (_render(integ, cam(lds), 16, 1, cell, sfc) for lds in (-1, 0))
    assert _bytes(a) == _bytes(b) and a["radiance"].min() > 0
    a, b = (_sense(integ, sensors, 16, 1, cell, sfc, lds=lds) for lds in (-1, 0))
    assert _bytes(a) == _bytes(b) and a["irradiance"].min() > 0
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals and the context
# ---------------------------------------------------------------------------------------------------------------------------------
CELL8, SFC4 = np.linspace(1.0, 8.0, 8, dtype=np.float32), np.linspace(2.0, 5.0, 4, dtype=np.float32)
PX, SX = "renderCameraEmissionExpected: ", "renderSensorsEmissionExpected: "


def _call_camera(c, cam, cell=CELL8, sfc=SFC4, spp=64, batches=1, n=4, entry="mcbrat_render_camera_emission_expected", rad=True):
    out, dropped = np.zeros(max(n, 1), np.float32), C.c_int64(-1)
    rc = getattr(c.L, entry)(c.ctx, C.addressof(cam) if cam is not None else None, c.ptr(cell), c.ptr(sfc), SEED, 0, spp, batches,
                             c.ptr(out) if rad else None, None, None, C.addressof(dropped))
    assert rc != 0 or dropped.value == 0
    return rc, (c.L.mcbrat_last_error(c.ctx).decode() if rc else ""), out


def _call_sensors(c, arr, cell=CELL8, sfc=SFC4, n=None, samples=64, batches=1, lds=-1, entry="mcbrat_render_sensors_emission_expected", irr=True):
    n = len(arr) if n is None else n
    out, dropped = np.zeros(max(len(arr), 1), np.float32), C.c_int64(-1)
    rc = getattr(c.L, entry)(c.ctx, n, C.addressof(arr), c.ptr(cell), c.ptr(sfc), SEED, 0, samples, batches, lds, c.ptr(out) if irr else None, None,
                             None, C.addressof(dropped))
    assert rc != 0 or dropped.value == 0
    return rc, (c.L.mcbrat_last_error(c.ctx).decode() if rc else ""), out


def _same_refusal(c, call, prefix, model, **kw):
    """the call is refused under the new entry with the sentence the emission entry refuses it with, under the entry's own name
    (of two faults at once both entries name the same one: the same order)"""
    rc, text, _ = call(c, **kw)
    rc0, text0, _ = call(c, entry=model, **kw)
    assert rc != 0 and rc0 != 0 and text.startswith(prefix), (kw, text)
    assert text[len(prefix):] == text0.split(": ", 1)[1], (text, text0)
    return text


def test_refusals_are_the_emission_entries_in_the_same_order():
    from tests.test_gpu_camera import REFUSED_CAMERAS
    from tests.test_gpu_refusal_matrix import Context
    c = Context()
    before = c.state()
    bad, nan = CELL8.copy(), SFC4.copy()
    bad[3], nan[2] = -1.0, np.nan
    zeros8, zeros4 = np.zeros(8, np.float32), np.zeros(4, np.float32)
    cam_model, sen_model = "mcbrat_render_camera_emission", "mcbrat_render_sensors_emission"
    K = lambda **kw: dict(cam=_camera_struct(), **kw)          # noqa: E731
    S = lambda **kw: dict(arr=_sensor_structs(1), **kw)        # noqa: E731
    camera_cases = [dict(cam=None), K(rad=False), K(cell=None), K(sfc=None), K(cell=None, spp=0), K(spp=0), K(batches=0), K(spp=0, batches=0),
                    dict(cam=_camera_struct(npx=32768, npy=32768), batches=2, n=1), K(cell=bad), K(sfc=nan), K(cell=bad, sfc=nan), K(cell=zeros8, sfc=zeros4),
                    K(cell=bad, spp=0), dict(cam=_camera_struct(mu=0.0), spp=0), dict(cam=_camera_struct(z=1.5), cell=bad), dict(cam=_camera_struct(z=1.5), spp=0)]
    camera_cases += [dict(cam=_camera_struct(**kw)) for kw, _ in REFUSED_CAMERAS]
    words = [_same_refusal(c, _call_camera, PX, cam_model, **kw) for kw in camera_cases]
    for word in ("no camera", "null pointer", "samplesPerPixel", "numBatches", "tally budget", "cellSource holds", "surfaceSource holds", "nothing emits",
                 "mu must be", "height lies outside", "footprint", "parallel", "field of view", "kind must be", "at least one pixel"):
        assert any(word in w for w in words), word
    sensor_cases = [S(n=0), S(irr=False), S(cell=None), S(sfc=None), S(samples=0), S(batches=0), S(lds=2), S(lds=2, samples=0), S(n=2 ** 30, batches=2),
                    S(cell=bad), S(sfc=nan), S(cell=zeros8, sfc=zeros4), S(cell=bad, samples=0), dict(arr=_sensor_structs(1, kind=2), cell=bad),
                    dict(arr=_sensor_structs(1, kind=2)), dict(arr=_sensor_structs(1, normal=(0.0, 0.0, 0.0))), dict(arr=_sensor_structs(1, position=(0.5, np.nan, 0.5))),
                    dict(arr=_sensor_structs(1, position=(0.5, 0.5, 1.5))), dict(arr=_sensor_structs(1, position=(0.5, 0.5, 1.5)), cell=bad)]
    words = [_same_refusal(c, _call_sensors, SX, sen_model, **kw) for kw in sensor_cases]
    for word in ("at least one sensor", "no sensors or no array", "null pointer", "samplesPerSensor", "numBatches", "gridInLds must be", "tally budget",
                 "cellSource holds", "surfaceSource holds", "nothing emits", "sensor kind", "non-zero normal", "not finite", "outside the domain"):
        assert any(word in w for w in words), word
    assert c.state() == before
    # a BRDF surface
    c.ok(c.setters["rpv"]())
    assert "BRDF surface" in _same_refusal(c, _call_camera, PX, cam_model, **K()) and "BRDF surface" in _same_refusal(c, _call_sensors, SX, sen_model, **S())
    assert "BRDF surface" in _same_refusal(c, _call_camera, PX, cam_model, **K(cell=bad))       # (the context before the sources)
    c.close()
    # missing pieces: nothing; the grid alone; optics without an inverse table
    L, ptr = c.L, c.ptr
    bare = L.mcbrat_create(0)
    bare_ctx = type("Bare", (), dict(L=L, ptr=staticmethod(ptr), ctx=bare))
    e, one = np.array([0.0, 0.5, 1.0]), np.ones(8)
    for step in range(3):
        if step == 1:
            assert L.mcbrat_set_grid(bare, 2, 2, 2, ptr(e), ptr(e), ptr(e)) == 0
        if step == 2:
            assert L.mcbrat_set_optics(bare, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(8, np.int32)), 0.2) == 0
        for call, kw, prefix, model in ((_call_camera, K(), PX, cam_model), (_call_sensors, S(), SX, sen_model)):
            rc, text, _ = call(bare_ctx, **kw)
            rc0, text0, _ = call(bare_ctx, entry=model, **kw)
            assert rc != 0 and rc0 != 0
            if step < 2:
                assert text.startswith(prefix) and "not completely specified" in text and text[len(prefix):] == text0.split(": ", 1)[1]
            else:
                assert "inverse phase function table" in text and text == text0      # (the context's own text)
    inv, coef = np.zeros(101, np.float32), np.zeros(2, np.float32)
    assert L.mcbrat_inverse_table_legendre(len(coef), ptr(coef), len(inv), ptr(inv)) == 0
    assert L.mcbrat_set_inverse_table(bare, 1, len(inv), 1, ptr(inv)) == 0
    rc, text, rad = _call_camera(bare_ctx, _camera_struct())                          # now complete: no source, no forward table
    assert rc == 0 and np.all(rad > 0), text
    L.mcbrat_destroy(bare)


def _emission_bytes(c):
    out = b""
    for entry in ("mcbrat_render_camera_emission",):
        rc, _, rad = _call_camera(c, _camera_struct(), spp=256, batches=2, entry=entry)
        assert rc == 0
        out += rad.tobytes()
    rc, _, irr = _call_sensors(c, _sensor_structs(2), samples=256, batches=2, entry="mcbrat_render_sensors_emission")
    assert rc == 0
    return out + irr.tobytes()


def test_the_context_is_left_as_it_was():
    from tests.test_gpu_refusal_matrix import Context
    fresh = Context()
    _, reference = fresh.trace()
    fresh.close()
    c = Context()
    before, image, emitted = c.state(), _solar_image(c), _emission_bytes(c)
    rc, text, rad = _call_camera(c, _camera_struct(), spp=256, batches=2)
    assert rc == 0 and np.all(rad > 0), (rc, text, rad)
    rc, text, irr = _call_sensors(c, _sensor_structs(2), samples=256, batches=2)
    assert rc == 0 and np.all(irr > 0), (rc, text, irr)
    assert c.state() == before and _solar_image(c) == image and _emission_bytes(c) == emitted    # the other entries: the same bytes
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()    # ... and a trace as a fresh context's
    for call, arg in ((_call_camera, _camera_struct()), (_call_sensors, _sensor_structs(1))):
        rc, text, _ = call(c, arg, cell=-CELL8)                      # after a refused render too
        assert rc != 0 and c.state() == before
    assert _solar_image(c) == image and _emission_bytes(c) == emitted
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the namelist driver
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_namelist_driver_takes_the_estimator(tmp_path):
    from mcbrat3d_amd import driver_cli, ncio
    from tests.test_gpu_camera import GRIDS
    xe, ye, ze, ext = GRIDS["2x2x2"]
    case = _medium(xe, ye, ze, ext, ssa=0.6, albedo=0.2)
    ix, iy, iz = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    case["temps"], case["lambda_um"], case["sfc_temp"] = 262.0 + 7.0 * ix + 4.3 * iy + 13.7 * iz, 10.0, 295.0
    dom = cases.product_domain(case)
    ncio.write_Domain(dom, str(tmp_path / "small.dom"))

    def run(tag, key):
        nml, cam_nc, sen_nc = tmp_path / (tag + ".nml"), tmp_path / (tag + "_camera.nc"), tmp_path / (tag + "_sensors.nc")
        nml.write_text("&radiativeTransfer solarMu = 0.5, solarAzimuth = 30., surfaceTemp = 295. /\n"
                       "&monteCarlo numPhotonsPerBatch = 500, numBatches = 2, iseed = 7, nPhaseIntervals = 501 /\n"
                       "&fileNames physDomainFile = '%s' /\n"
                       "&camera cameraKind = 'orthographic', cameraPixels = 2, 2, cameraMu = 1., emission = .true.,%s cameraSamplesPerPixel = 128,\n"
                       " cameraBatches = 4, outputCameraFile = '%s' /\n"
                       "&sensors sensorKind = 'planar', sensorPositions = 0.1, 0.05, 0., emission = .true.,%s sensorSamples = 128, sensorBatches = 4,\n"
                       " outputSensorFile = '%s' /\n" % (tmp_path / "small.dom", key, cam_nc, key, sen_nc))
        driver_cli.main([str(nml)])
        return (ncio.readCamera_netcdf(str(cam_nc)), ncio.readSensors_netcdf(str(sen_nc)), open(str(cam_nc), "rb").read(), open(str(sen_nc), "rb").read())

    plain = run("plain", "")
    named = run("named", " emissionEstimator = 'collision',")
    expected = run("expected", " emissionEstimator = 'expected',")
    assert plain[2] == named[2] and plain[3] == named[3]               # 'collision' writes what a namelist without the key writes
    assert "cameraEstimator" not in plain[0] and "sensorEstimator" not in plain[1]
    image, irr = expected[0], expected[1]
    assert image["cameraEstimator"] == "expected" and irr["sensorEstimator"] == "expected"
    assert image["cameraEmission"].shape == (2, 2) and np.all(image["cameraEmission"] > 0) and image["cameraDroppedPaths"] == 0 and irr["sensorDroppedPaths"] == 0
    # the same scene by the other estimator: within the two renders' standard errors
    z = (image["cameraEmission"].astype(np.float64) - plain[0]["cameraEmission"]) / np.hypot(image["cameraEmission_StdErr"], plain[0]["cameraEmission_StdErr"])
    assert np.all(np.abs(z) < 4.5)
    assert abs(irr["sensorEmission"][0] - plain[1]["sensorEmission"][0]) < 4.5 * np.hypot(irr["sensorEmission_StdErr"][0], plain[1]["sensorEmission_StdErr"][0])
