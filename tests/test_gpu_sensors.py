"""The backward sensors on the GPU: exact vacuum values -- every sample's direction recomputed from Philox
and the host mirror of the ray mapping --, the periodic fold on a checkerboard surface, transport theory (an absorbing slab,
isotropically scattering slabs: irradiance at three depths, actinic flux inside), the tie to the forward level fluxes face by
face, bitwise determinism, refusals that leave the context untouched, and the camera's image bit for bit as the parent commit
rendered it.  `dropped` is 0 in every render here."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_camera import TAU_RTOL, VAC, _integrator, _medium, _pinhole, small_domain, sun_vector
from tests.test_gpu_sources import philox, u01

pytestmark = pytest.mark.gpu
SEED = 20261021
PI = np.pi
W0 = {"planar": PI, "spherical": 4.0 * PI}


def _sensors(*a, **kw):
    from mcbrat3d_amd.sensors import new_Sensors
    return new_Sensors(*a, **kw)


def _render(integ, sensors, samples, batches=1, seed=SEED, first=0, lds=-1):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    rng = new_RandomNumberSequence(seed, first)
    out = integ.renderSensors(sensors, rng, samples, batches, gridInLds=lds)
    assert out["dropped"] == 0 and rng.nextPhotonId == first + samples * batches
    assert np.array_equal(out["irradiance"], out["diffuse"] + out["direct"])
    return out


def _exact(got, expected, w0):
    """the camera's vacuum tolerance scaled by w0: the fixed-point step plus float rounding"""
    got, expected = np.asarray(got, np.float64), np.asarray(expected, np.float64)
    return np.all(np.abs(got - expected) <= expected * 2.0 ** -22 + w0 * 2.0 ** -31)


def mirror_directions(sensors, i, seed, first, count):
    """(origins, directions) of the samples first .. first + count - 1 of sensor i: [u, v, a, c] = block 0 of event 0 under the
    counter (0, id, index lo, index hi), through the host mirror of the mapping"""
    idx = np.arange(first, first + count, dtype=np.uint64)
    zero = np.zeros(count, np.uint64)
    r = philox([zero, zero + np.uint64(int(sensors.ids[i])), idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32)], (seed & 0xFFFFFFFF, seed >> 32))
    q = [u01(x).astype(np.float64) for x in r]
    rays = [sensors.ray(i, q[0][k], q[1][k], q[2][k], q[3][k]) for k in range(count)]
    return np.array([o for o, _ in rays]), np.array([d for _, d in rays])


def direct_factor(normal, mu0, phi0):
    """c of a planar sensor, in double, from the float direction the library holds"""
    s = sun_vector(mu0, phi0)
    s = s / np.linalg.norm(s)
    n = np.asarray(normal, float) / np.linalg.norm(normal)
    return max(0.0, float(n @ s)) / abs(s[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. vacuum over a Lambertian surface: exact
# ---------------------------------------------------------------------------------------------------------------------------------
def _vacuum(a=0.3, surface=None):
    return _integrator(_medium(VAC["xe"], VAC["ye"], VAC["ze"], np.zeros((2, 2, 2)), albedo=a), 0.5, 30.0, surface=surface, tables=101, fwd=181)[0]


def test_point_sensors_in_a_vacuum_are_exact():
    a, mu0 = 0.3, 0.5
    integ = _vacuum(a)
    heights = (0.0, 0.11, 0.25)
    pos = [(0.1, 0.2, z) for z in heights]
    s = _sensors(pos * 3, tilt=[180.0] * 3 + [0.0] * 6, kind=["planar"] * 6 + ["spherical"] * 3)
    seed, _ = _seed_with_every_sample_off_the_horizon(s, 2 * 197)   # (a path along the horizon is as long as a leg's bound allows)
    out = _render(integ, s, 197, 2, seed=seed)
    integ.finalize()
    down, up, sph = slice(0, 3), slice(3, 6), slice(6, 9)
    assert _exact(out["diffuse"][down], a, PI) and np.all(out["direct"][down] == 0.0)          # facing down: the surface's a / pi, no sun
    assert np.all(out["diffuse"][up] == 0.0) and _exact(out["direct"][up], 1.0, PI)            # facing up: the sun alone
    assert _exact(out["direct"][sph], 1.0 / mu0, 4.0 * PI)
    for k in ("diffuse_StdErr", "direct_StdErr", "irradiance_StdErr"):
        assert np.all(out[k][:6] == 0.0), k
    assert np.all(out["direct_StdErr"] == 0.0)   # (a spherical point sensor's diffuse part counts its downward samples: test below)
    assert out["batchMeans"].shape == (2, 2, 9) and np.array_equal(out["batchMeans"][0, 1], out["batchMeans"][1, 1])


def _seed_with_every_sample_off_the_horizon(sensors, count, check=None):
    """the first seed from SEED on, found on the CPU from the reference alone, whose samples all have |d.z| > 1e-3 (and pass `check`)"""
    for seed in range(SEED, SEED + 200):
        rays = [mirror_directions(sensors, i, seed, 0, count) for i in range(len(sensors))]
        if all(np.all(np.abs(d[:, 2]) > 1e-3) for _, d in rays) and (check is None or check(rays)):
            return seed, rays
    raise AssertionError("no seed found")


def test_tilted_and_spherical_sensors_in_a_vacuum_count_their_downward_samples():
    a, mu0, phi0, samples = 0.3, 0.5, 30.0, 197
    s = _sensors([(0.1, 0.2, 0.11), (0.3, 0.1, 0.11)], tilt=[35.0, 0.0], azimuth=[200.0, 0.0], kind=["planar", "spherical"], ids=[11, 5])
    seed, rays = _seed_with_every_sample_off_the_horizon(s, 2 * samples)
    integ = _vacuum(a)
    out = _render(integ, s, samples, 2, seed=seed)
    integ.finalize()
    for i, kind in enumerate(s.kindNames()):
        dz = rays[i][1][:, 2]
        assert np.all(np.abs(dz) > 1e-3) and dz.size == 2 * samples     # every sample, none left out
        for b in range(2):
            count = int((dz[b * samples:(b + 1) * samples] < 0).sum())
            assert 0 < count < samples
            assert _exact(out["batchMeans"][b, 0, i], W0[kind] * (a / PI) * count / samples, W0[kind]), (kind, b, count)
        c = direct_factor(s.normals[i], mu0, phi0) if kind == "planar" else 1.0 / mu0
        assert c > 0 and _exact(out["batchMeans"][:, 1, i], c, W0[kind]) and _exact(out["direct"][i], c, W0[kind])
        assert out["direct_StdErr"][i] == 0.0 and out["diffuse_StdErr"][i] > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. geometry through the periodic fold: exact
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkerboard_surface_through_the_periodic_fold():
    import mcbrat3d_amd as M
    refl = np.array([[0.1, 0.8], [0.6, 0.25]], np.float32)  # [x patch, y patch]
    sx, sy = np.array([0.0, 0.25, 0.5]), np.array([0.0, 0.2, 0.5])
    samples, z = 197, 0.2
    s = _sensors([(0.31, 0.07, z)], tilt=115.0, azimuth=200.0, ids=[3])

    def hits(rays):
        o, d = rays[0]
        downward = d[:, 2] < 0
        t = (0.0 - o[downward, 2]) / d[downward, 2]
        return downward, o[downward, 0] + d[downward, 0] * t, o[downward, 1] + d[downward, 1] * t

    def margin(rays):
        _, hx, hy = hits(rays)
        fx, fy = hx % 0.5, hy % 0.5
        return min(np.abs(fx[:, None] - sx[None, :]).min(), np.abs(fy[:, None] - sy[None, :]).min())

    seed, rays = _seed_with_every_sample_off_the_horizon(s, 2 * samples, check=lambda r: margin(r) > 1e-4)
    downward, hx, hy = hits(rays)
    periods = {(int(np.floor(x / 0.5)), int(np.floor(y / 0.5))) for x, y in zip(hx, hy)}
    assert margin(rays) > 1e-4 and len(periods) >= 6, (margin(rays), len(periods))   # no hit on a patch boundary; several domain periods
    assert np.all(np.abs(rays[0][1][:, 2]) > 1e-3)
    value = np.zeros(2 * samples)
    value[downward] = refl[(hx % 0.5 >= sx[1]).astype(int), (hy % 0.5 >= sy[1]).astype(int)]
    assert len(set(value[downward])) == 4 and (~downward).sum() > 10
    integ = _vacuum(0.0, surface=M.new_SurfaceDescription(refl[None], sx, sy))
    out = _render(integ, s, samples, 2, seed=seed)
    integ.finalize()
    for b in range(2):  # pi times the mean of refl / pi over the batch's samples
        assert _exact(out["batchMeans"][b, 0, 0], value[b * samples:(b + 1) * samples].sum() / samples, PI)
    c = direct_factor(s.normals[0], 0.5, 30.0)  # (25 degrees below the horizon, but turned toward the sun)
    assert c > 0.5 and _exact(out["batchMeans"][:, 1, 0], c, PI)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. transport theory: slabs
# ---------------------------------------------------------------------------------------------------------------------------------
def _theory_check(what, mean, err, theory, w0):
    """the camera's _slab_check; a value that is the same in every batch (error exactly 0: the direct beam alone, or nothing)
    is held to the exact tolerance instead"""
    mean, err = float(mean), float(err)
    print("%-34s mean %.6g theory %.6g stderr %.3g (%.2f sigma, %.3f %%)" % (what, mean, theory, err, (mean - theory) / err if err else 0.0,
                                                                             100 * err / theory if theory else 0.0))
    if err == 0.0:
        assert _exact(mean, theory, w0), (what, mean, theory)
        return
    assert err < 0.01 * theory, (what, err, theory)               # the power condition
    assert abs(mean - theory) < 4.5 * err, (what, mean, theory, err)


def test_absorbing_slab_over_a_reflecting_surface():
    """16 x 16384 paths per sensor (the hit probability 2 E3(1) = 0.22 asks for 36000 paths for 1 %).  Measured on the MI355X:
    0.0148428 against 0.0148452, standard error 0.47 % of theory, -0.03 sigma."""
    from scipy.special import expn
    from tests.test_analytic import slab
    tau, a, mu0 = 1.0, 0.5, 0.5
    integ, _ = _integrator(slab(tau, 0.0, albedo=a), mu0, 20.0, tables=101, fwd=181)
    out = _render(integ, _sensors([(0.1, 0.2, 0.25), (0.1, 0.2, 0.0)], tilt=[180.0, 0.0]), 16384, 16)
    integ.finalize()
    _theory_check("facing down at the top", out["irradiance"][0], out["irradiance_StdErr"][0], a * np.exp(-tau / mu0) * 2.0 * float(expn(3, tau)), PI)
    assert out["direct"][0] == 0.0
    assert out["diffuse"][1] == 0.0 and out["diffuse_StdErr"][1] == 0.0 and out["direct_StdErr"][1] == 0.0
    assert abs(-np.log(float(out["direct"][1])) - tau / mu0) < TAU_RTOL * tau / mu0     # the sun ray's tolerance, in tau


@pytest.mark.parametrize("albedo", [0.0, 0.3])
@pytest.mark.parametrize("b,omega,mu0", [(1.0, 1.0, 0.6), (3.0, 0.9, 1.0)])
def test_irradiance_and_actinic_flux_inside_isotropically_scattering_slabs(b, omega, mu0, albedo):
    """planar sensors facing up and down at tau = 0, b / 2 and b against layered_isotropic_profile, a spherical one at a cell
    centre of the solver near b / 2 against 4 pi J.  16 x 16384 paths per sensor.  Measured on the MI355X (standard error as a
    share of theory over the planar sensors that have one; largest deviation; then the actinic flux):
      (1, 1, 0.6) albedo 0    0.11-0.28 %, 1.73 sigma;  0.20 %, -0.17 sigma        albedo 0.3  0.12-0.30 %, 2.10 sigma;  0.18 %, -0.06 sigma
      (3, 0.9, 1) albedo 0    0.08-0.24 %, 0.57 sigma;  0.13 %, -0.85 sigma        albedo 0.3  0.08-0.39 %, 0.85 sigma;  0.12 %, -0.44 sigma
    The top facing up (1, the sun alone) and the bottom over a black surface facing down (0) are the same in every batch."""
    from tests.test_analytic import _layered_solution, layered_isotropic_profile, slab
    H, cells = 0.25, 150
    integ, _ = _integrator(slab(b, omega, albedo=albedo, nz=16), mu0, 33.0, tables=9001)
    taus = np.array([0.0, 0.5 * b, b])
    up, down = layered_isotropic_profile([b], [omega], mu0, taus, albedo=albedo, cells_per_layer=cells)
    edges, _, _, _, _, J = _layered_solution([b], [omega], mu0, albedo, cells)
    cell = cells // 2
    tauc = 0.5 * (edges[cell] + edges[cell + 1])
    zs = [H * (1.0 - t / b) for t in taus]
    s = _sensors([(0.1, 0.2, z) for z in zs] * 2 + [(0.1, 0.2, H * (1.0 - tauc / b))], tilt=[0.0] * 3 + [180.0] * 3 + [0.0],
                 kind=["planar"] * 6 + ["spherical"])
    out = _render(integ, s, 16384, 16)
    integ.finalize()
    for k in range(3):
        _theory_check("tau %.2f facing up (flux down)" % taus[k], out["irradiance"][k], out["irradiance_StdErr"][k], float(down[k]), PI)
        _theory_check("tau %.2f facing down (flux up)" % taus[k], out["irradiance"][3 + k], out["irradiance_StdErr"][3 + k], float(up[k]), PI)
    _theory_check("actinic flux at tau %.3f" % tauc, out["irradiance"][6], out["irradiance_StdErr"][6], 4.0 * PI * float(J[cell]), 4.0 * PI)
    # the direct part alone is the beam: e^(-tau / mu0) on the plane, that over mu0 on the sphere
    for k in range(3):
        assert abs(float(out["direct"][k]) - np.exp(-taus[k] / mu0)) < 1e-5 and out["direct"][3 + k] == 0.0
    assert abs(float(out["direct"][6]) - np.exp(-tauc / mu0) / mu0) < 1e-5 / mu0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the tie to the forward level fluxes, face by face
# ---------------------------------------------------------------------------------------------------------------------------------
def _level_tie(case, mu0, phi0, levels, photons, batches, samples):
    """forward run with recLevelFluxes + recDirectLevelFluxes and area sensors equal to every column's face at `levels`, facing up
    and down -> [(name, forward mean, its error, backward mean, its error)], arrays [level, iy, ix]"""
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=9001, minForwardTableSize=1801, recLevelFluxes=True, recDirectLevelFluxes=True,
                            surfaceBDRF=cases.product_surface(case))
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12), photons, batches)
    nx, ny, nz = dom.numX, dom.numY, dom.numZ
    st = driver.statistics(driver.unpack_moments(integ.moments(), nx, ny, nz, levelFluxes=True, directLevelFluxes=True))
    xe, ye, ze = (np.asarray(case[k], float) for k in ("xe", "ye", "ze"))
    pos, ext = [], []
    for k in levels:
        for j in range(ny):
            for i in range(nx):
                pos.append((xe[i], ye[j], ze[k]))
                ext.append(((xe[i + 1] - xe[i], 0.0, 0.0), (0.0, ye[j + 1] - ye[j], 0.0)))
    n = len(pos)
    s = _sensors(pos * 2, tilt=[0.0] * n + [180.0] * n, extents=ext * 2)
    out = _render(integ, s, samples, 16, seed=SEED + 1)
    integ.finalize()

    def fwd(name):
        a = np.asarray(st[name], np.float64)
        assert a.shape == (nx, ny, nz + 1), (name, a.shape)
        return a[:, :, list(levels)].transpose(2, 1, 0)

    def bwd(name, part):
        return out[name].astype(np.float64)[part].reshape(len(levels), ny, nx)

    upf, downf = slice(0, n), slice(n, 2 * n)
    area = np.outer(np.diff(ye), np.diff(xe)) / ((ye[-1] - ye[0]) * (xe[-1] - xe[0]))                  # [iy, ix]: a column's share of the photons
    floor = 11.9 / (photons * batches * np.broadcast_to(area, (len(levels), ny, nx)))
    return floor, [(name, fwd(f), fwd(f + "_StdErr"), bwd(key, part), bwd(key + "_StdErr", part)) for name, f, key, part in (
        ("flux down", "levelFluxDown", "irradiance", upf), ("direct", "levelFluxDownDirect", "direct", upf),
        ("diffuse", "levelFluxDownDiffuse", "diffuse", upf), ("flux up", "levelFluxUp", "irradiance", downf))]


def _tie_check(tie):
    """the criteria of the camera's _reciprocity_check, per compared quantity.  Two kinds of face have no sigma to be held to, and
    are not left out but held to something else:
      * a face through which the forward run sent NO photon (mean and error exactly 0: the direct beam under the step cloud's
        thick half, e^-36) -- zero counts are no error estimate.  A Poisson mean of lambda gives no count with probability
        e^-lambda, which is the two-sided 4.5 sigma level (6.8e-6) at lambda = 11.9: the backward value must lie below 11.9
        photons' worth of that column, 11.9 / (photons x the column's share of the area);
      * a face both sides know without noise (combined error exactly 0, mean not 0: the top of the domain facing up, where the
        direct beam is 1) is held to the number formats, 1e-6 (float results of fixed-point tallies).
    On the first run of this test the step cloud's direct part failed the plain criterion by 1700 sigma in exactly those
    faces of the first kind (forward 0 +- 0, backward 2e-16 with an error of 1e-19); the domain means agreed to 0.002 %."""
    floor, res = tie
    for name, fwd, ferr, bwd, berr in res:
        err = np.sqrt(ferr ** 2 + berr ** 2)
        empty = (fwd == 0.0) & (ferr == 0.0)
        assert np.all(bwd[empty] <= floor[empty]), (name, bwd[empty], floor[empty])
        exact = (err == 0.0) & ~empty
        assert np.all(np.abs(bwd[exact] - fwd[exact]) <= 1e-6), (name, bwd[exact], fwd[exact])
        noisy = ~empty & ~exact
        z = (bwd[noisy] - fwd[noisy]) / err[noisy]
        mean_err = np.sqrt((ferr ** 2).sum() + (berr ** 2).sum()) / fwd.size
        print("%-9s faces: %d without a forward photon, %d exact, %d with noise, worst %.2f sigma; domain mean forward %.6g backward %.6g, combined error %.3g (%.2f %%)" % (
            name, int(empty.sum()), int(exact.sum()), z.size, np.abs(z).max() if z.size else 0.0, fwd.mean(), bwd.mean(), mean_err, 100 * mean_err / fwd.mean()))
        assert np.all(np.abs(z) < 4.5), (name, z)                           # every face, none left out
        assert mean_err < 0.01 * fwd.mean(), name                           # the power condition on the domain mean
        assert abs(bwd.mean() - fwd.mean()) < 4.5 * mean_err, name


def test_level_fluxes_of_the_step_cloud_face_by_face():
    """32 columns x levels 0, 16, 32 x facing up and down: 192 area sensors of a column's width x Ly.  Forward 40 x 200000
    photons, backward 16 x 8192 paths per sensor.  Measured on the MI355X, for flux down / direct / diffuse / flux up: combined
    error of the domain mean 0.08 / 0.03 / 0.15 / 0.16 % of it, worst face 2.49 / 2.67 / 2.49 / 2.73 sigma, domain means 0.66269 against
    0.66205, 0.341079 / 0.341087, 0.32161 / 0.32096, 0.27748 / 0.27801; 40 (direct) and 32 (diffuse) faces without a forward photon."""
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    _tie_check(_level_tie(case, 0.5, 30.0, (0, 16, 32), 200000, 40, 8192))


def test_level_fluxes_of_a_small_domain_face_by_face():
    """4 x 3 columns, two components, unequal layers and a per-patch surface, levels 0 and 2: forward 40 x 200000 photons,
    backward 16 x 16384 paths per sensor.  Measured on the MI355X, for flux down / direct / diffuse / flux up: combined error of the
    domain mean 0.04 / 0.03 / 0.11 / 0.09 %, worst face 2.11 / 2.24 / 1.89 / 2.02 sigma."""
    _tie_check(_level_tie(small_domain(), 0.5, 30.0, (0, 2), 200000, 40, 16384))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def _mixed():
    return dict(positions=[(0.13, 0.2, 0.05), (0.4, 0.1, 0.0), (0.3, 0.3, 0.25), (0.05, 0.2, 0.12), (0.26, 0.0, 0.2)],
                tilt=[0.0, 0.0, 180.0, 35.0, 0.0], azimuth=[0.0, 0.0, 0.0, 200.0, 0.0], kind=["planar", "planar", "planar", "planar", "spherical"],
                extents=[((0, 0, 0), (0, 0, 0)), ((0.1, 0, 0), (0, 0.5, 0)), ((0.03, 0, 0), (0, 0.02, 0)), ((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 0))],
                ids=[0, 1, 2, 3, 77])


def test_batch_means_are_bitwise_reproducible():
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    integ, _ = _integrator(case, 0.5, 30.0)
    s, n = _sensors(**_mixed()), 1000  # (not a multiple of 64)
    means = lambda **kw: _render(integ, s, n, **kw)["batchMeans"]  # noqa: E731
    two = means(batches=2)
    assert means(batches=2).tobytes() == two.tobytes()                                                   # two identical calls
    assert means(first=0).tobytes() == two[:1].tobytes() and means(first=n).tobytes() == two[1:].tobytes()  # two batches = two calls
    assert means(batches=2, lds=0).tobytes() == means(batches=2, lds=1).tobytes() == two.tobytes()       # the grid in LDS or not
    # a sensor alone = the same sensor (the same id) among the others
    m = _mixed()
    for i in range(5):
        one = _sensors(**{k: [v[i]] for k, v in m.items()})
        assert _render(integ, one, n, 2)["batchMeans"][:, :, 0].tobytes() == np.ascontiguousarray(two[:, :, i]).tobytes(), i
    # the same samples as part of a longer range
    longer = means(batches=3, first=2 ** 40 - n)
    assert means(first=2 ** 40).tobytes() == longer[1:2].tobytes()
    assert two[:, 0].std() > 0 and np.all(two[:, 0] > 0)
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals, and a context left as it was
# ---------------------------------------------------------------------------------------------------------------------------------
def _struct(**kw):
    from mcbrat3d_amd._capi import Sensor
    s = Sensor()
    s.kind, s.id = 0, 0
    s.position[:], s.e1[:], s.e2[:], s.normal[:] = (0.5, 0.5, 0.5), (0.2, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 2.0)
    for k, v in kw.items():
        if k in ("position", "e1", "e2", "normal"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def _call(ctx, sensors, samples=64, batches=1, lds=-1, n=None):
    from mcbrat3d_amd._capi import Sensor
    n = len(sensors) if n is None else n
    arr = (Sensor * max(len(sensors), 1))(*sensors)
    dif, dirc = np.zeros(max(len(sensors), 1), np.float32), np.zeros(max(len(sensors), 1), np.float32)
    rc = ctx.L.mcbrat_render_sensors(ctx.ctx, n, C.addressof(arr), SEED, 0, samples, batches, lds, ctx.ptr(dif), ctx.ptr(dirc), None, None, None, None, None)
    return rc, (ctx.L.mcbrat_last_error(ctx.ctx).decode() if rc else ""), dif, dirc


NAN, INF = float("nan"), float("inf")
REFUSED_SENSORS = [
    (dict(kind=2), "kind"), (dict(kind=-1), "kind"), (dict(position=(0.5, NAN, 0.5)), "not finite"), (dict(e1=(INF, 0.0, 0.0)), "not finite"),
    (dict(e2=(0.0, NAN, 0.0)), "not finite"), (dict(normal=(0.0, 0.0, INF)), "not finite"), (dict(kind=1, normal=(NAN, 0.0, 0.0)), "not finite"),
    (dict(normal=(0.0, 0.0, 0.0)), "non-zero normal"), (dict(e1=(0.2, 0.0, 1e-5)), "perpendicular"), (dict(normal=(0.1, 0.0, 1.0)), "perpendicular"),
    (dict(position=(0.5, 0.5, 1.01)), "corner"), (dict(position=(0.5, 0.5, -0.01)), "corner"),
    (dict(position=(0.5, 0.5, 0.9), normal=(1.0, 0.0, 0.0), e1=(0.0, 0.0, 0.2)), "corner"),
    (dict(position=(0.5, 0.5, 0.1), normal=(1.0, 0.0, 0.0), e1=(0.0, 0.3, 0.0), e2=(0.0, 0.0, -0.2)), "corner"),
]


def test_refusals_leave_the_context_untouched():
    from tests.test_gpu_refusal_matrix import Context
    fresh = Context()
    _, reference = fresh.trace()
    fresh.close()
    c = Context()
    before = c.state()
    for kw, word in REFUSED_SENSORS:
        for sensors in ([_struct(**kw)], [_struct(), _struct(**kw)]):   # alone, and behind a good one
            rc, text, _, _ = _call(c, sensors)
            assert rc != 0 and word in text and text.startswith("renderSensors:"), (kw, rc, text)
    for kwargs, word in ((dict(n=0), "n < 1"), (dict(n=-3), "n < 1"), (dict(samples=0), "samplesPerSensor"), (dict(batches=0), "numBatches"),
                         (dict(lds=2), "gridInLds"), (dict(n=2 ** 28, batches=2), "tally budget")):
        rc, text, _, _ = _call(c, [_struct()], **kwargs)
        assert rc != 0 and word in text and text.startswith("renderSensors:"), (kwargs, rc, text)
    assert c.state() == before
    # a spherical sensor ignores its normal; a successful render: sensible numbers, and the context still as a fresh one
    rc, text, dif, dirc = _call(c, [_struct(), _struct(kind=1, normal=(0.0, 0.0, 0.0))], samples=256, batches=2)
    assert rc == 0 and np.all(dif > 0) and np.all(dirc > 0), (rc, text, dif, dirc)
    assert c.state() == before
    rc, mom = c.trace()
    assert rc == [0, ""] and mom.tobytes() == reference.tobytes()
    c.close()
    # a source other than the Directional one, a BRDF surface, missing pieces: the camera's rules, in the sensors' name
    c = Context(thermal=True)
    rc, text, _, _ = _call(c, [_struct()])
    assert rc != 0 and "Directional solar source" in text and text.startswith("renderSensors:")
    c.close()
    c = Context()
    c.ok(c.L.mcbrat_set_source_random_azimuth(c.ctx, C.c_float(0.5)))
    assert "Directional solar source" in _call(c, [_struct()])[1]
    c.ok(c.L.mcbrat_set_source_solar(c.ctx, C.c_float(0.5), C.c_float(0.0)))
    c.ok(c.setters["rpv"]())
    text = _call(c, [_struct()])[1]
    assert "BRDF surface" in text and text.startswith("renderSensors:")
    c.close()
    L, ptr = c.L, c.ptr
    bare = L.mcbrat_create(0)
    holder = type("Bare", (), dict(L=L, ptr=staticmethod(ptr), ctx=bare))
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
        rc, text, _, _ = _call(holder, [_struct()])
        assert rc != 0
        texts.append(text)
    L.mcbrat_destroy(bare)
    assert "not completely specified" in texts[0] and "not completely specified" in texts[1], texts
    assert "forward phase function table" in texts[2] and "inverse phase function table" in texts[3], texts


def test_grid_in_lds_is_refused_where_the_grid_does_not_fit():
    """landsatLike128-sized: 128 x 128 x 64 floats are 4 MiB, no LDS share holds them"""
    from mcbrat3d_amd._capi import McbratError
    n = 128
    xe, ze = np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, 65)
    integ, _ = _integrator(_medium(xe, xe, ze, np.full((n, n, 64), 1.0)), 0.5, 30.0, tables=101, fwd=181)
    s = _sensors([(0.5, 0.5, 0.0)])
    with pytest.raises(McbratError, match="renderSensors: gridInLds = 1.*do not fit"):
        _render(integ, s, 64, lds=1)
    assert np.array_equal(_render(integ, s, 64, lds=0)["batchMeans"], _render(integ, s, 64, lds=-1)["batchMeans"])
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the camera is untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_camera_renders_what_the_parent_commit_rendered():
    """tests/golden/camera_batchmeans_parent.npy: batchMeans [gridInLds 0 | 1][2][3][5] of the pinhole of the camera's
    test_batch_means_are_bitwise_reproducible (step cloud, 1000 samples, 2 batches), recorded on the MI355X with the library of
    the commit before the sensors.  The tallies are integers, so the image does not depend on scheduling: bit for bit."""
    from tests.test_gpu_camera import _render as render_camera
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_batchmeans_parent.npy"))
    assert golden.shape == (2, 2, 3, 5) and golden.dtype == np.float32
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    integ, _ = _integrator(case, 0.5, 30.0)
    for lds in (0, 1):
        cam = _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)
        assert render_camera(integ, cam, 1000, 2)["batchMeans"].tobytes() == golden[lds].tobytes(), lds
    integ.finalize()


# ---------------------------------------------------------------------------------------------------------------------------------
# the namelist driver with a /sensors/ group, end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_namelist_driver_renders_and_writes_the_sensors(tmp_path):
    from mcbrat3d_amd import driver_cli, ncio
    nml, s_nc, res_nc = tmp_path / "run.nml", tmp_path / "sensors.nc", tmp_path / "out.nc"
    text = ("&radiativeTransfer solarMu = 0.5, solarAzimuth = 30. /\n&monteCarlo numPhotonsPerBatch = 2000, numBatches = 4, iseed = 7, nPhaseIntervals = 2001 /\n"
            "&fileNames physDomainFile = 'builtin:i3rcStepCloud', outputNetcdfFile = '%s' /\n" % res_nc)
    nml.write_text(text)
    plain = driver_cli.main([str(nml)])
    nml.write_text(text + "&sensors sensorKind = 'planar', sensorPositions = 0.1, 0.25, 0., 0.4, 0.25, 0., 0.4, 0.25, 0.25, sensorTilt = 0., 35., 0.,\n"
                          " sensorAzimuth = 30., sensorSamples = 512, sensorBatches = 4, outputSensorFile = '%s' /\n" % s_nc)
    stats = driver_cli.main([str(nml)])
    for k in ("meanFluxUp", "meanFluxDown", "fluxUp"):  # the group changes nothing else
        assert np.array_equal(np.asarray(stats[k]), np.asarray(plain[k])), k
    a, b = ncio.readSensors_netcdf(str(s_nc)), ncio.readSensors_netcdf(str(res_nc))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["sensorIrradiance"].shape == (3,) and np.all(a["sensorIrradiance"] > 0) and np.all(a["sensorIrradiance_StdErr"][:2] > 0)
    assert np.allclose(a["sensorIrradiance"], a["sensorDiffuse"] + a["sensorDirect"], rtol=1e-6)
    assert _exact(a["sensorDirect"][2], 1.0, PI) and a["sensorDiffuse"][2] == 0.0          # at the top, facing up: the sun alone
    assert (a["sensorSamples"], a["sensorBatches"], a["sensorDroppedPaths"]) == (512, 4, 0)
