"""The backward sensors without a GPU: the ray mapping through tests/sensor_ray_dump.cpp -- a stand-alone
program over the shared mapping header, plain and under the address and undefined-behaviour sanitizers --, mcbrat_sensor_ray
against it and against the closed forms, new_Sensors, the /sensors/ namelist group, the NetCDF variables, the binding's symbols
and the Fortran shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.3, -0.5, 0.81), (-2.0, 0.1, -0.4), (0.57, 0.57, 0.59)]
DRAWS = [(0.2, 0.7, 0.4, 0.9), (0.0, 1.0, 0.0, 0.0), (1.0, 0.0, 1.0, 0.5), (0.5, 0.5, 0.013, 0.25), (0.9, 0.1, 0.999, 0.75), (0.3, 0.3, 0.5, 1.0)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the stand-alone program over the shared header, plain and sanitized
# ---------------------------------------------------------------------------------------------------------------------------------
def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "sensor_ray_dump.cpp")])
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sensors")
    return (_compile(str(d / "sensor_ray_dump")),
            _compile(str(d / "sensor_ray_dump_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_the_dump_program_includes_only_the_mapping_header():
    text = open(os.path.join(ROOT, "tests", "sensor_ray_dump.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_sensor_ray.h"]
    header = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_sensor_ray.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and re.findall(r'#include\s+"([^"]+)"', header) == ["../../include/mcbrat.h"]
    kernel = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_camera.hip")).read()
    # the kernel and the host function call the header's functions: sensor_ray() is its two halves, in this order
    assert '#include "mcbrat_sensor_ray.h"' in kernel and "sensor_direction(sg" in kernel and "sensor_origin(sg" in kernel
    assert "sensor_ray(g, u, v" in kernel
    body = re.search(r"inline void sensor_ray\(.*?\{(.*?)\n\}", header, re.S).group(1)
    assert [ln.strip() for ln in body.strip().splitlines()] == ["sensor_origin(g, u, v, origin);", "sensor_direction(g, a, c, direction);"]


def test_the_header_alone_passes_its_moment_checks_also_sanitized(exes):
    """unit length, d.n >= 2^-16, the first and second moments on the stratified 256 x 256 grid, the corners and the ends of a:
    every check of tests/sensor_ray_dump.cpp, for 9 normals and both kinds (a sanitizer's finding ends the program with a failure)"""
    outs = [subprocess.run([e], capture_output=True, text=True, timeout=300) for e in exes]
    for r in outs:
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 failure(s)", r.stdout[-2000:] + r.stderr[-2000:]
    assert outs[0].stdout == outs[1].stdout
    lines = outs[0].stdout.splitlines()
    assert sum(ln.startswith("ok ") for ln in lines) == 9 * 7 + 9 * 6 + 5 and not any(ln.startswith("FAILED") for ln in lines)
    for what in ("unit length", "d.n >= 2^-16", "mean d.n - 2/3", "mean d:", "mean d_i d_j - delta_ij / 3", "origin at the corners",
                 "directions at a = 0 and a = 1"):
        assert any(what in ln for ln in lines), what


def _sensor(kind, normal, **kw):
    """the sensor tests/sensor_ray_dump.cpp builds for a normal: the same position and edges"""
    from mcbrat3d_amd.sensors import new_Sensors
    n = np.asarray(normal, float)
    k = int(np.argmin(np.abs(n)))
    ax = np.zeros(3)
    ax[k] = 1.0
    c1 = np.cross(n, ax)
    c2 = np.cross(n, c1)
    return new_Sensors([(0.25, -1.5, 0.75)], normals=[n], kind=kind, extents=[(0.3 * c1, 0.2 * c2 + 0.1 * c1)], **kw)


def closed_form(kind, normal, pos, e1, e2, u, v, a, c):
    """the mapping as csrc/mcbrat_sensor_ray.h states it, in numpy"""
    n = np.asarray(normal, float) / np.linalg.norm(normal) if kind == "planar" else np.array([0.0, 0.0, 1.0])
    k = int(np.argmin(np.abs(n)))
    t1 = -n[k] * n
    t1[k] += 1.0
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    mu = max(np.sqrt(a), 2.0 ** -16) if kind == "planar" else 1.0 - 2.0 * a
    s = np.sqrt((1.0 - mu) * (1.0 + mu))
    return pos + u * e1 + v * e2, s * np.cos(2 * np.pi * c) * t1 + s * np.sin(2 * np.pi * c) * t2 + mu * n


@pytest.mark.parametrize("kind", ["planar", "spherical"])
def test_ray_is_the_library_s_the_header_s_and_the_closed_form(exes, kind):
    from mcbrat3d_amd import _capi
    L = _capi.lib()
    for normal in NORMALS:
        s = _sensor(kind, normal)
        for u, v, a, c in DRAWS:
            o, d = s.ray(0, u, v, a, c)
            st = s.structs()
            o2, d2 = np.zeros(3), np.zeros(3)
            assert L.mcbrat_sensor_ray(C.addressof(st[0]), u, v, a, c, _capi.ptr(o2), _capi.ptr(d2)) == 0
            assert np.array_equal(o, o2) and np.array_equal(d, d2)                      # .ray() is mcbrat_sensor_ray
            eo, ed = closed_form(kind, normal, s.positions[0], s.e1[0], s.e2[0], u, v, a, c)
            assert np.allclose(o, eo, rtol=0, atol=1e-15) and np.allclose(d, ed, rtol=0, atol=1e-14), (normal, u, v, a, c, d, ed)
            assert abs(np.linalg.norm(d) - 1.0) < 1e-14
            for exe in exes:                                                            # ... and the header's, digit for digit
                w = subprocess.run([exe, str(0 if kind == "planar" else 1), *[repr(float(x)) for x in normal], *[repr(x) for x in (u, v, a, c)]],
                                   check=True, capture_output=True, text=True, timeout=60).stdout.split()
                got = np.array([float(x) for x in w])
                assert np.allclose(got[:3], o, rtol=0, atol=1e-15) and np.allclose(got[3:], d, rtol=0, atol=1e-15), (normal, w)
    assert L.mcbrat_sensor_ray(None, 0.5, 0.5, 0.5, 0.5, _capi.ptr(np.zeros(3)), _capi.ptr(np.zeros(3))) != 0
    bad = _capi.Sensor()
    bad.kind = 3
    assert L.mcbrat_sensor_ray(C.addressof(bad), 0.5, 0.5, 0.5, 0.5, _capi.ptr(np.zeros(3)), _capi.ptr(np.zeros(3))) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# new_Sensors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tilt_and_azimuth_give_the_normal():
    from mcbrat3d_amd.sensors import new_Sensors
    s = new_Sensors([(0, 0, 0)] * 4, tilt=[0.0, 90.0, 35.0, 180.0], azimuth=[0.0, 90.0, 200.0, 0.0])
    b, a = np.radians(35.0), np.radians(200.0)
    want = [(0, 0, 1), (0, 1, 0), (np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), np.cos(b)), (0, 0, -1)]
    assert np.allclose(s.normals, want, rtol=0, atol=1e-15)
    assert np.allclose(new_Sensors([(0, 0, 0)] * 2, tilt=20.0, azimuth=90.0).normals, [(0, np.sin(np.radians(20)), np.cos(np.radians(20)))] * 2, atol=1e-15)
    # defaults: facing up, point sensors, ids 0, 1, ...; the struct is filled member for member
    s = new_Sensors([(1, 2, 3), (4, 5, 6)], kind=["planar", "spherical"], ids=[7, 2 ** 32 - 1], extents=[((1, 0, 0), (0, 2, 0))] * 2)
    st = s.structs()
    assert len(s) == 2 and [(x.kind, x.id, list(x.position), list(x.e1), list(x.e2), list(x.normal)) for x in st] == [
        (0, 7, [1.0, 2.0, 3.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]),
        (1, 2 ** 32 - 1, [4.0, 5.0, 6.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0])]
    assert list(new_Sensors([(0, 0, 0)] * 3).ids) == [0, 1, 2] and s.kindNames() == ["planar", "spherical"]


@pytest.mark.parametrize("kw,word", [
    (dict(positions=[]), "positions"), (dict(positions=[(0, 0)]), "positions"), (dict(positions=[(0, 0, float("nan"))]), "positions"),
    (dict(kind="fisheye"), "unknown sensor kind"), (dict(kind=["planar", "planar"]), "unknown sensor kind"),
    (dict(normals=[(0, 0, 0)]), "non-zero normal"), (dict(normals=[(0, 0, 1)], tilt=10.0), "not both"),
    (dict(normals=[(0, float("inf"), 1)]), "normals"), (dict(tilt=190.0), "tilt"), (dict(tilt=[1.0, 2.0]), "tilt"),
    (dict(azimuth=float("nan")), "azimuth"), (dict(extents=[((1, 0, 0), (0, 0, 1e-3))]), "perpendicular"),
    (dict(extents=[((1, 0, 0),)]), "extents"), (dict(ids=[-1]), "ids"), (dict(ids=[0.5]), "ids"), (dict(ids=[1, 2]), "ids"),
])
def test_new_sensors_refuses(kw, word):
    from mcbrat3d_amd._capi import McbratError
    from mcbrat3d_amd.sensors import new_Sensors
    args = dict(positions=[(0.0, 0.0, 0.0)])
    args.update(kw)
    with pytest.raises(McbratError, match=word):
        new_Sensors(**args)


# ---------------------------------------------------------------------------------------------------------------------------------
# the namelist group, the NetCDF variables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_namelist_reads_the_sensors_group(tmp_path):
    from mcbrat3d_amd import driver_cli
    from mcbrat3d_amd._capi import McbratError
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["sensorkind"] == "" and cfg["outputsensorfile"] == ""
    assert driver_cli.sensors_from_namelist(cfg) is None  # absent by default: nothing changes
    nml.write_text("&sensors sensorKind = 'planar', sensorPositions = 0.1, 0.2, 0., 0.3, 0.2, 0.5, sensorTilt = 0., 35., sensorAzimuth = 180.,\n"
                   " sensorSamples = 5000, sensorBatches = 4, outputSensorFile = 's.nc' /\n")
    cfg = driver_cli.read_namelists(str(nml))
    s = driver_cli.sensors_from_namelist(cfg)
    assert len(s) == 2 and s.kindNames() == ["planar", "planar"] and np.array_equal(s.positions, [(0.1, 0.2, 0.0), (0.3, 0.2, 0.5)])
    b = np.radians(35.0)
    assert np.allclose(s.normals, [(0, 0, 1), (-np.sin(b), 0, np.cos(b))], atol=1e-15)
    assert (cfg["sensorsamples"], cfg["sensorbatches"], cfg["outputsensorfile"]) == (5000, 4, "s.nc")
    nml.write_text("&sensors sensorKind = 'spherical', sensorPositions = 0.1, 0.2, 0.3 /\n")
    s = driver_cli.sensors_from_namelist(driver_cli.read_namelists(str(nml)))
    assert len(s) == 1 and s.kindNames() == ["spherical"]
    for body, word in (("sensorKind = 'planar'", "sensorPositions"), ("sensorKind = 'planar', sensorPositions = 1., 2.", "sensorPositions"),
                       ("sensorKind = 'cube', sensorPositions = 1., 2., 3.", "unknown sensor kind"),
                       ("sensorKind = 'planar', sensorPositions = 1., 2., 3., sensorTilt = 200.", "tilt"),
                       ("sensorKind = 'planar', sensorPositions = 1., 2., 3., sensorSamples = 0", "sensorSamples")):
        nml.write_text("&sensors %s /\n" % body)
        with pytest.raises(McbratError, match=word):
            driver_cli.sensors_from_namelist(driver_cli.read_namelists(str(nml)))


def _stop_before_tracing(monkeypatch, domains):
    from mcbrat3d_amd import driver_cli, driver
    import mcbrat3d_amd
    made, traced = [], []
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: domains)
    monkeypatch.setattr(driver, "run", lambda *a, **k: traced.append(a))
    return made, traced, mcbrat3d_amd


def test_the_namelist_driver_refuses_the_sensors_for_spectral_jobs(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    made, traced, M = _stop_before_tracing(monkeypatch, [object(), object()])
    monkeypatch.setattr(M, "new_Integrator", lambda *a, **k: made.append(a))
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&sensors sensorKind = 'planar', sensorPositions = 0., 0., 0. /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="sensorKind: the backward sensors are not available for spectrally integrated runs"):
        driver_cli.main([str(nml)])
    assert not made and not traced


def test_a_bad_sensors_group_ends_the_run_before_it_traces(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    from mcbrat3d_amd._capi import McbratError

    class Stub:
        def specifyParameters(self, **kw):
            pass

    dom = driver_cli.builtin_domain("i3rcStepCloud")
    made, traced, M = _stop_before_tracing(monkeypatch, [dom])
    monkeypatch.setattr(M, "new_Integrator", lambda *a, **k: made.append(a) or Stub())
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&sensors sensorKind = 'planar', sensorPositions = 0., 0. /\n&fileNames physDomainFile = 'builtin:i3rcStepCloud' /\n")
    with pytest.raises(McbratError, match="sensorPositions"):
        driver_cli.main([str(nml)])
    assert made and not traced


def _result(n, batches=3, seed=2):
    rng = np.random.default_rng(seed)
    r = {k: rng.random(n, np.float32) for k in ("irradiance", "irradiance_StdErr", "diffuse", "direct", "diffuse_StdErr", "direct_StdErr")}
    r.update(batchMeans=rng.random((batches, 2, n), np.float32), dropped=0, samplesPerSensor=5000)
    return r


def test_netcdf_round_trip_of_the_sensor_variables(tmp_path):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import ncio
    from mcbrat3d_amd.sensors import new_Sensors
    s = new_Sensors([(0.1, 0.2, 0.0), (0.3, 0.2, 0.5), (1.0, 1.0, 1.0)], tilt=[0.0, 35.0, 180.0], azimuth=200.0, kind=["planar", "planar", "spherical"])
    res = _result(3)
    alone = str(tmp_path / "s.nc")
    ncio.writeSensors_netcdf(alone, s, res)
    stats = {"totalPhotons": 10, "batches": 2}
    for name in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        stats[name] = stats[name + "_StdErr"] = np.zeros((2, 3), np.float32)
    e = np.array([0.0, 1.0, 2.0])
    with_s, without = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    ncio.writeResults_netcdf(with_s, "d", stats, e, np.array([0.0, 1.0, 2.0, 3.0]), e, sensors=s, sensorResult=res)
    ncio.writeResults_netcdf(without, "d", stats, e, np.array([0.0, 1.0, 2.0, 3.0]), e)
    assert ncio.readSensors_netcdf(without) is None
    for path in (alone, with_s):
        back = ncio.readSensors_netcdf(path)
        assert np.array_equal(back["sensorPosition"], s.positions) and np.array_equal(back["sensorNormal"], s.normals)
        assert list(back["sensorKind"]) == [0, 0, 1]
        for name, key in (("sensorIrradiance", "irradiance"), ("sensorIrradiance_StdErr", "irradiance_StdErr"), ("sensorDiffuse", "diffuse"), ("sensorDirect", "direct")):
            assert np.array_equal(back[name], res[key]), name
        assert (back["sensorSamples"], back["sensorBatches"], back["sensorDroppedPaths"]) == (5000, 3, 0)
    a, b = netcdf_file(with_s, "r", mmap=False), netcdf_file(without, "r", mmap=False)
    try:
        assert set(a.variables) - set(b.variables) == {"sensorPosition", "sensorNormal", "sensorKind", "sensorIrradiance", "sensorIrradiance_StdErr",
                                                       "sensorDiffuse", "sensorDirect"}
        assert a.variables["sensorIrradiance"].dimensions == ("sensor",) and a.dimensions["sensor"] == 3
        assert np.array_equal(a.variables["fluxUp"][:], b.variables["fluxUp"][:]) and not hasattr(b, "sensorSamples")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the binding, the Fortran shim
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_layer_declares_the_entries():
    import mcbrat3d_amd
    from mcbrat3d_amd import _capi, build, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    cam = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_camera.hip")).read()
    for sym, nargs in (("mcbrat_render_sensors", 15), ("mcbrat_sensor_ray", 7)):
        assert re.search(r"\bint %s\(" % sym, text) and re.search(r"\bint %s\(" % sym, cam)
        assert len(_capi.SYMBOLS[sym][1]) == nargs
        decl = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    L = _capi.lib()  # resolves every symbol of SYMBOLS
    assert L.mcbrat_abi_version() == 3
    # the struct of the binding is the header's, member for member
    members = re.search(r"typedef struct mcbrat_sensor \{(.*?)\} mcbrat_sensor;", text, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", members, flags=re.S)
    names = [n.split("[")[0] for decl in re.findall(r"(?:uint32_t|int32_t|double)\s+([^;]+);", members) for n in re.split(r",\s*", decl.strip())]
    assert names == [n for n, _ in _capi.Sensor._fields_]
    assert C.sizeof(_capi.Sensor) == 2 * 4 + 12 * 8 and _capi.Sensor.position.offset == 8 and _capi.Sensor.normal.offset == 80
    assert "mcbrat_sensor_ray.h" in build.DEPS and build.SOURCES == ["mcbrat_api.hip", "mcbrat_host.cpp", "mcbrat_camera.hip"]
    assert hasattr(integrator.Integrator, "renderSensors") and hasattr(mcbrat3d_amd, "new_Sensors") and hasattr(mcbrat3d_amd, "Sensors")
    # the kernel is the camera's, a third template parameter; nothing of it in the variant table or the parameter block
    assert "template <int BLOCK, bool GRID_LDS, bool SENSOR>" in cam
    for inst in ("camera_kernel<512, true, true>", "camera_kernel<256, false, true>", "camera_kernel<512, true, false>", "camera_kernel<256, false, false>"):
        assert inst in cam
    for other in ("mcbrat_variants.h", "mcbrat_device.h"):
        assert "ensor" not in open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", other)).read()


def test_fortran_shim_declares_the_sensor_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("sensor", "renderSensors"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    assert 'name="mcbrat_render_sensors"' in text
    # the bind(C) type mirrors the struct: the same members in the same order
    block = re.search(r"type, bind\(C\) :: sensor(.*?)end type sensor", text, re.S).group(1)
    names = [re.split(r"[ (=]", n.strip())[0] for decl in re.findall(r"::\s*(.+)", block) for n in re.split(r",\s*(?=[A-Za-z])", re.sub(r"\(/.*?/\)", "", decl))]
    from mcbrat3d_amd import _capi
    assert names == [n for n, _ in _capi.Sensor._fields_], names
    nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
    assert re.search(r"\bt\b.*rendersensors", symbols)
