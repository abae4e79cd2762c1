"""The emission renders without a GPU: mcbrat_planck_radiance against the closed form and against what
mcbrat_emission_weighting builds from the same function, planck_sources, the NetCDF variables, the namelist key, the binding's
prototypes and the Fortran shim."""
import os

import numpy as np

from tests import cases
from tests.test_analytic import planck

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# The library evaluates B = 2 h c^2 / (lambda^5 (e^x - 1)), x = h c / (k lambda T), in double, with the reference's h, c and k:
# decimal constants ROUNDED TO FLOAT, each within 2^-24 of its decimal value.  tests/test_analytic.planck has x = C2 / (lambda T)
# with C2 = 14387.77 um K.  In a ratio of two values the factor 2 h c^2 cancels, so the two disagree through x alone, by at most
#     DELTA = 3 * 2^-24 + |C2 - 1e6 h c / k| / C2                      (relative, in x)
# and d ln B / d ln x = -x e^x / (e^x - 1) =: -s(x), so a ratio B(x1) / B(x2) moves by at most (s(x1) + s(x2)) DELTA, to first
# order (the second order is DELTA^2 s^2 < 1e-11 here); 1e-13 covers the double roundings of both evaluations.
H, C_LIGHT, K_B, C2 = 6.62606957e-34, 2.99792458e8, 1.3806488e-23, 14387.77
DELTA = 3.0 * 2.0 ** -24 + abs(C2 - 1.0e6 * H * C_LIGHT / K_B) / C2


def _s(x):
    return x * np.exp(x) / np.expm1(x)


def test_planck_radiance_is_the_closed_form_in_ratios():
    import mcbrat3d_amd as M
    temps = np.array([180.0, 220.0, 255.5, 273.15, 288.0, 300.0, 330.0])
    lams = [3.7, 6.7, 10.0, 11.03, 12.5, 50.0]
    assert DELTA < 4e-7
    worst = 0.0
    got = {lam: M.planck_radiance(lam, temps) for lam in lams}
    for lam in lams:
        assert got[lam].dtype == np.float64 and got[lam].shape == temps.shape and np.all(got[lam] > 0)
    for l1 in lams:            # every pair (wavelength, temperature) against every other: across temperatures, across wavelengths
        for l2 in lams:
            x1, x2 = C2 / (l1 * temps[:, None]), C2 / (l2 * temps[None, :])
            ratio = got[l1][:, None] / got[l2][None, :]
            ref = planck(l1, temps)[:, None] / planck(l2, temps)[None, :]
            dev = np.abs(ratio / ref - 1.0)
            tol = (_s(x1) + _s(x2)) * DELTA * (1.0 + 1e-3) + 1e-13
            worst = max(worst, float((dev / tol).max()))
            assert np.all(dev <= tol), (l1, l2, dev.max())
    print("planck ratios: largest deviation / tolerance %.3f" % worst)
    # the unit: W m-2 sr-1 um-1 (10 um, 300 K: 9.92 in every table)
    assert abs(M.planck_radiance(10.0, [300.0])[0] - 9.924) < 0.005
    # keeps the shape; refuses a wavelength that is not positive
    assert M.planck_radiance(10.0, np.full((2, 3), 280.0)).shape == (2, 3)
    try:
        M.planck_radiance(0.0, [280.0])
        raise AssertionError("a wavelength of 0 was accepted")
    except M.McbratError:
        pass


def _thermal_case():
    rng = np.random.default_rng(11)
    case = cases.homog_lw(n=3, ext=4.0, ssa=0.5, g=0.0, nleg=2, temp=280.0, sfc_temp=296.0, albedo=0.25, lam=10.5)
    case["temps"] = rng.uniform(240.0, 300.0, (3, 3, 3))
    case["components"][0]["ext"] = rng.uniform(1.0, 6.0, (3, 3, 3))
    case["components"][0]["ssa"] = rng.uniform(0.1, 0.9, (3, 3, 3))
    case["ze"] = np.array([0.0, 0.07, 0.2, 0.3])
    return case


def test_emission_weighting_is_built_from_this_planck_function():
    """The CDF's increments times its normalisation are 4 pi (1 - omega) sigma B dz with mcbrat_planck_radiance's B, and totalFlux
    is their column mean plus pi (1 - a) B_s, times dLambda.  To rounding: a CDF entry is a rounded quotient of two compensated
    sums, so an increment times the normalisation is off by a few units in the last place of the NORMALISATION."""
    import mcbrat3d_amd as M
    case = _thermal_case()
    dom = cases.product_domain(case)
    w = M.new_Weights(3, 3, 3)
    dl = 0.7
    flux = M.emission_weighting(dom, w, case["sfc_temp"], dLambda=dl)
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    assert cell.dtype == np.float32 and cell.shape == (3, 3, 3) and sfc.dtype == np.float32 and sfc.shape == (3, 3)
    b = M.planck_radiance(case["lambda_um"], case["temps"].transpose(2, 1, 0))        # [z, y, x], double
    b_s = float(M.planck_radiance(case["lambda_um"], [case["sfc_temp"]])[0])
    assert np.array_equal(cell, b.astype(np.float32)) and np.all(sfc == np.float32(b_s))
    comp = case["components"][0]
    absorb = (comp["ext"] * (1.0 - comp["ssa"])).transpose(2, 1, 0)
    dz = np.diff(case["ze"])[:, None, None]
    expected = (4.0 * np.pi * b * absorb * dz).reshape(-1)                             # x fastest
    last = flux * w.fracAtmsPower * 9.0 / dl                                           # the normalisation: the CDF's last entry before it
    inc = np.diff(np.concatenate([[0.0], w.voxelWeights])) * last
    assert np.all(np.abs(inc - expected) <= 8.0 * 2.0 ** -53 * last + 1e-13 * expected), np.abs(inc - expected).max() / last
    total = (expected.sum() / 9.0 + np.pi * (1.0 - case["albedo"]) * b_s) * dl
    assert abs(flux - total) <= 1e-13 * total, (flux, total)


def test_netcdf_round_trip_of_the_emission_variables(tmp_path):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import ncio
    from mcbrat3d_amd.camera import new_Camera
    from mcbrat3d_amd.sensors import new_Sensors
    rng = np.random.default_rng(3)
    cam = new_Camera("orthographic", npx=3, npy=2, mu=0.8, phi=20.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25)
    image = dict(radiance=rng.uniform(5, 9, (2, 3)).astype(np.float32), radiance_StdErr=rng.uniform(0, 0.1, (2, 3)).astype(np.float32),
                 batchMeans=np.zeros((4, 2, 3), np.float32), dropped=0, samplesPerPixel=128, emission=True)
    sens = new_Sensors([(0.1, 0.2, 0.0), (0.3, 0.1, 0.25)], tilt=[0.0, 180.0])
    irr = dict(irradiance=rng.uniform(20, 30, 2).astype(np.float32), irradiance_StdErr=rng.uniform(0, 0.1, 2).astype(np.float32),
               batchMeans=np.zeros((5, 2), np.float32), dropped=0, samplesPerSensor=64, emission=True)
    ncio.writeCamera_netcdf(str(tmp_path / "cam.nc"), cam, image)
    ncio.writeSensors_netcdf(str(tmp_path / "sen.nc"), sens, irr)
    back = ncio.readCamera_netcdf(str(tmp_path / "cam.nc"))
    assert np.array_equal(back["cameraEmission"], image["radiance"]) and np.array_equal(back["cameraEmission_StdErr"], image["radiance_StdErr"])
    assert "cameraRadiance" not in back and back["cameraSamplesPerPixel"] == 128 and back["cameraBatches"] == 4 and back["cameraDroppedPaths"] == 0
    back = ncio.readSensors_netcdf(str(tmp_path / "sen.nc"))
    assert np.array_equal(back["sensorEmission"], irr["irradiance"]) and np.array_equal(back["sensorEmission_StdErr"], irr["irradiance_StdErr"])
    assert "sensorIrradiance" not in back and "sensorDirect" not in back and back["sensorBatches"] == 5 and back["sensorSamples"] == 64
    assert np.array_equal(back["sensorKind"], [0, 0]) and np.array_equal(back["sensorPosition"], sens.positions)
    # a solar result still goes to the solar variables, and both sit beside each other in a results file's namespace
    solar = dict(image, emission=False)
    ncio.writeCamera_netcdf(str(tmp_path / "solar.nc"), cam, solar)
    back = ncio.readCamera_netcdf(str(tmp_path / "solar.nc"))
    assert np.array_equal(back["cameraRadiance"], image["radiance"]) and "cameraEmission" not in back
    f = netcdf_file(str(tmp_path / "cam.nc"), "r", mmap=False)
    try:
        assert f.variables["cameraEmission"].dimensions == ("cameraY", "cameraX") and f.cameraKind.decode() == "orthographic"
    finally:
        f.close()
    assert ncio.readCamera_netcdf(str(tmp_path / "sen.nc")) is None and ncio.readSensors_netcdf(str(tmp_path / "cam.nc")) is None


def test_the_namelist_key_emission_defaults_to_false(tmp_path):
    from mcbrat3d_amd import driver_cli
    head = "&monteCarlo numPhotonsPerBatch = 10 /\n"
    nml = tmp_path / "run.nml"
    nml.write_text(head + "&camera cameraKind = 'pinhole' /\n&sensors sensorKind = 'planar', sensorPositions = 0., 0., 0. /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemission"] is False and cfg["sensorsemission"] is False and "emission" not in cfg
    nml.write_text(head + "&camera cameraKind = 'pinhole', emission = .true. /\n&sensors sensorKind = 'planar' /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemission"] is True and cfg["sensorsemission"] is False
    nml.write_text(head + "&camera cameraKind = 'pinhole' /\n&sensors sensorKind = 'planar', emission = T, sensorSamples = 77 /\n&radiativeTransfer surfaceTemp = 291.5 /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemission"] is False and cfg["sensorsemission"] is True and cfg["sensorsamples"] == 77 and cfg["surfacetemp"] == 291.5
    nml.write_text(head)                                                               # neither group: as every existing namelist
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemission"] is False and cfg["sensorsemission"] is False and cfg["camerakind"] == "" and cfg["sensorkind"] == ""


def test_the_binding_has_the_prototypes():
    import ctypes as C
    from mcbrat3d_amd import _capi
    L = _capi.lib()
    for name, nargs in (("mcbrat_render_camera_emission", 12), ("mcbrat_render_sensors_emission", 14), ("mcbrat_planck_radiance", 4)):
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs and getattr(L, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    for name in ("mcbrat_render_camera_emission", "mcbrat_render_sensors_emission", "mcbrat_planck_radiance"):
        assert "int %s(" % name in header
    assert "#define MCBRAT_ABI_VERSION 3" in header and L.mcbrat_abi_version() == 3      # additions: the version stays
    # null arrays and a negative count are refused by the host function
    out = np.zeros(1)
    assert L.mcbrat_planck_radiance(10.0, 1, None, _capi.ptr(out)) == 1 and L.mcbrat_planck_radiance(10.0, -1, _capi.ptr(out), _capi.ptr(out)) == 1
    assert L.mcbrat_planck_radiance(10.0, 0, None, None) == 0


def test_the_fortran_shim_declares_the_emission_entries():
    src = open(os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")).read()
    for name in ("mcbrat_render_camera_emission", "mcbrat_render_sensors_emission"):
        assert 'bind(C, name="%s")' % name in src
    for name in ("renderCameraEmission", "renderSensorsEmission"):
        assert "subroutine %s(" % name in src and "end subroutine %s" % name in src
        assert name in src.split("contains")[0]                                      # public
