"""The backward camera without a GPU: the pixel mapping of mcbrat_camera_ray against its closed forms
written out in numpy -- through the library and through tests/camera_ray_dump.cpp, a stand-alone program over the shared mapping
header, plain and under the address and undefined-behaviour sanitizers --, the host-side refusals of new_Camera, the /camera/
namelist group, the NetCDF variables, the binding's symbols and the Fortran shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
UV = (0.0, 0.5, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the closed forms
# ---------------------------------------------------------------------------------------------------------------------------------
def pinhole_ray(npx, npy, position, look, up, fov, i, j, u, v):
    look, up = np.asarray(look, float), np.asarray(up, float)
    lookHat = look / np.linalg.norm(look)
    right = np.cross(look, up)
    right /= np.linalg.norm(right)
    trueUp = np.cross(right, lookHat)
    tanHalf = np.tan(np.radians(float(np.float32(fov))) / 2.0)
    s = (2.0 * (i + u) / npx - 1.0) * tanHalf
    t = (2.0 * (j + v) / npy - 1.0) * tanHalf * npy / npx
    d = lookHat + s * right + t * trueUp
    return np.asarray(position, float), d / np.linalg.norm(d)


def orthographic_ray(npx, npy, mu, phi, footprint, z, i, j, u, v):
    xLo, xHi, yLo, yHi = footprint
    mu, phi = float(np.float32(mu)), np.radians(float(np.float32(phi)))
    s = np.sqrt(1.0 - mu * mu)
    travel = np.array([s * np.cos(phi), s * np.sin(phi), mu])
    return np.array([xLo + (i + u) * (xHi - xLo) / npx, yLo + (j + v) * (yHi - yLo) / npy, z]), -travel


PINHOLES = [
    dict(npx=4, npy=4, position=(0.1, 0.2, 0.3), look=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=60.0),
    dict(npx=7, npy=3, position=(-3.0, 12.5, 0.0), look=(1.0, 0.3, 0.2), up=(0.0, 0.0, 1.0), fov=100.0),          # non-square
    dict(npx=2, npy=5, position=(0.0, 0.0, 1.0), look=(-0.4, 2.0, -1.3), up=(0.3, -0.1, 5.0), fov=35.0),            # oblique look and up, not normalised
    dict(npx=1, npy=1, position=(1.0, 1.0, 1.0), look=(0.0, 3.0, 0.0), up=(1.0, 1.0, 0.0), fov=179.0),
]
ORTHOGRAPHICS = [dict(npx=3, npy=2, mu=mu, phi=phi, footprint=(-0.5, 1.0, 2.0, 2.6), height=0.7)
                 for mu, phi in ((1.0, 0.0), (0.6, 30.0), (0.6, 110.0), (0.3, 200.0), (0.3, 330.0), (-0.6, 75.0), (-1.0, 0.0), (-0.2, 250.0))]


def _pixels(npx, npy):
    return sorted({(0, 0), (npx - 1, 0), (0, npy - 1), (npx - 1, npy - 1), (npx // 2, npy // 2)})


def _camera(kind, c):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera(kind, **c)


@pytest.mark.parametrize("c", PINHOLES)
def test_pinhole_mapping_is_the_closed_form(c):
    cam = _camera("pinhole", c)
    for i, j in _pixels(c["npx"], c["npy"]):
        for u in UV:
            for v in UV:
                o, d = cam.ray(i, j, u, v)
                eo, ed = pinhole_ray(i=i, j=j, u=u, v=v, **c)
                assert np.array_equal(o, eo) and np.allclose(d, ed, rtol=0, atol=1e-14), (c, i, j, u, v, d, ed)
                assert abs(np.linalg.norm(d) - 1.0) < 1e-14
    # j grows upward along `up`, i to the right of the look direction
    _, lo = cam.ray(0, 0)
    _, hi = cam.ray(0, c["npy"] - 1, 0.5, 1.0)
    if c["npy"] > 1:
        assert np.dot(hi - lo, np.asarray(c["up"], float)) > 0


@pytest.mark.parametrize("c", ORTHOGRAPHICS)
def test_orthographic_mapping_is_the_closed_form(c):
    cam = _camera("orthographic", c)
    args = dict(npx=c["npx"], npy=c["npy"], mu=c["mu"], phi=c["phi"], footprint=c["footprint"], z=c["height"])
    for i, j in _pixels(c["npx"], c["npy"]):
        for u in UV:
            for v in UV:
                o, d = cam.ray(i, j, u, v)
                eo, ed = orthographic_ray(i=i, j=j, u=u, v=v, **args)
                assert np.allclose(o, eo, rtol=0, atol=1e-15) and np.allclose(d, ed, rtol=0, atol=1e-15), (c, i, j, u, v)
    # the backward direction points against the light's direction of travel: up for a camera that looks at light travelling down
    assert np.sign(cam.ray(0, 0)[1][2]) == -np.sign(c["mu"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the stand-alone program over the shared header, plain and sanitized
# ---------------------------------------------------------------------------------------------------------------------------------
def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "camera_ray_dump.cpp")])
    return out


def _argv(kind, c):
    o = dict(mu=1.0, phi=0.0, footprint=(0.0, 1.0, 0.0, 1.0), height=0.0, position=(0, 0, 0), look=(0, 0, -1), up=(0, 1, 0), fov=60.0)
    o.update(c)
    vals = [kind, o["npx"], o["npy"], o["mu"], o["phi"], *o["footprint"], o["height"], *o["position"], *o["look"], *o["up"], o["fov"]]
    return [repr(float(v)) if isinstance(v, float) else str(v) for v in vals]


def _dump(exe, kind, c):
    return subprocess.run([exe] + _argv(kind, c), check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("camera")
    return (_compile(str(d / "camera_ray_dump")),
            _compile(str(d / "camera_ray_dump_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_the_dump_program_includes_only_the_mapping_header():
    text = open(os.path.join(ROOT, "tests", "camera_ray_dump.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_camera_ray.h"]
    header = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_camera_ray.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and re.findall(r'#include\s+"([^"]+)"', header) == ["../../include/mcbrat.h"]
    kernel = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_camera.hip")).read()
    assert '#include "mcbrat_camera_ray.h"' in kernel and "camera_ray(cp.g" in kernel  # the kernel calls the same function


@pytest.mark.parametrize("kind,c", [(1, c) for c in PINHOLES] + [(0, c) for c in ORTHOGRAPHICS])
def test_the_header_alone_gives_the_closed_forms_also_sanitized(exes, kind, c):
    plain, sanitized = (_dump(e, kind, c) for e in exes)
    assert plain == sanitized and len(plain) == 9 * c["npx"] * c["npy"]  # (check=True: a sanitizer's finding ends the program with a failure)
    for line in plain:
        w = line.split()
        i, j, u, v = int(w[0]), int(w[1]), float(w[2]), float(w[3])
        got = np.array([float(x) for x in w[4:]])
        if kind == 1:
            eo, ed = pinhole_ray(i=i, j=j, u=u, v=v, **c)
        else:
            eo, ed = orthographic_ray(c["npx"], c["npy"], c["mu"], c["phi"], c["footprint"], c["height"], i, j, u, v)
        assert np.allclose(got[:3], eo, rtol=0, atol=1e-15) and np.allclose(got[3:], ed, rtol=0, atol=1e-14), line


def test_the_header_refuses_what_new_camera_refuses(exes):
    for kind, c, word in ((0, dict(npx=1, npy=1, mu=0.0), "mu"), (0, dict(npx=1, npy=1, footprint=(1.0, 1.0, 0.0, 1.0)), "footprint"),
                          (1, dict(npx=1, npy=1, look=(0, 2, 0), up=(0, -1, 0)), "parallel"), (1, dict(npx=1, npy=1, fov=180.0), "field of view"),
                          (2, dict(npx=1, npy=1), "kind"), (1, dict(npx=0, npy=1), "pixel")):
        for exe in exes:
            out = _dump(exe, kind, c)
            assert len(out) == 1 and out[0].startswith("refused: renderCamera:") and word in out[0], (kind, c, out)


# ---------------------------------------------------------------------------------------------------------------------------------
# new_Camera, the namelist group, the NetCDF variables, the binding, the Fortran shim
# ---------------------------------------------------------------------------------------------------------------------------------
OK_O = dict(npx=2, npy=2, mu=0.5, phi=10.0, footprint=(0.0, 1.0, 0.0, 1.0), height=0.5)
OK_P = dict(npx=2, npy=2, position=(0, 0, 0), look=(0, 0, 1), up=(0, 1, 0), fov=60.0)


@pytest.mark.parametrize("kind,change,word", [
    ("fisheye", {}, "unknown camera kind"), ("orthographic", dict(npx=0), "pixel"), ("orthographic", dict(npy=1.5), "pixel"),
    ("orthographic", dict(gridInLds=2), "gridInLds"), ("orthographic", dict(mu=0.0), "mu"), ("orthographic", dict(mu=1.5), "mu"),
    ("orthographic", dict(phi=-1.0), "phi"), ("orthographic", dict(phi=361.0), "phi"), ("orthographic", dict(footprint=None), "footprint"),
    ("orthographic", dict(footprint=(0.0, 0.0, 0.0, 1.0)), "footprint"), ("orthographic", dict(footprint=(0.0, 1.0, 2.0, 1.0)), "footprint"),
    ("orthographic", dict(footprint=(0.0, 1.0, 2.0)), "footprint"), ("orthographic", dict(height=float("nan")), "height"),
    ("pinhole", dict(position=None), "position"), ("pinhole", dict(look=(0, 0, 0)), "non-zero"), ("pinhole", dict(up=(0, 0)), "up"),
    ("pinhole", dict(look=(0, 2, 0), up=(0, -3, 0)), "parallel"), ("pinhole", dict(fov=0.0), "field of view"),
    ("pinhole", dict(fov=180.0), "field of view"), ("pinhole", dict(position=(0, float("inf"), 0)), "position"),
])
def test_new_camera_refuses(kind, change, word):
    from mcbrat3d_amd._capi import McbratError
    args = dict(OK_P if kind == "pinhole" else OK_O)
    args.update(change)
    with pytest.raises(McbratError, match=word):
        _camera(kind, args)


def test_new_camera_fills_the_struct():
    s = _camera("pinhole", dict(OK_P, npx=5, npy=3, jitter=False, gridInLds=1, position=(1, 2, 3), fov=75.0)).struct()
    assert (s.kind, s.npx, s.npy, s.jitter, s.gridInLds, list(s.position), list(s.look), list(s.up), s.fovXDeg) == \
        (1, 5, 3, 0, 1, [1.0, 2.0, 3.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], 75.0)
    s = _camera("orthographic", OK_O).struct()
    assert (s.kind, s.jitter, s.gridInLds, s.mu, s.phiDeg, s.xLo, s.xHi, s.yLo, s.yHi, s.z) == (0, 1, -1, 0.5, 10.0, 0.0, 1.0, 0.0, 1.0, 0.5)


def test_namelist_reads_the_camera_group(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["camerakind"] == "" and cfg["outputcamerafile"] == ""
    xe, ye, ze = np.array([0.0, 1.0, 2.0]), np.array([0.0, 3.0]), np.array([0.0, 0.5, 1.5])
    assert driver_cli.camera_from_namelist(cfg, xe, ye, ze) is None  # absent by default: nothing changes
    nml.write_text("&camera cameraKind = 'pinhole', cameraPixels = 64, 48, cameraPosition = 0.5, 1.0, 0.0, cameraLook = 0., 0., 1.,\n"
                   " cameraUp = 0., 1., 0., cameraFov = 90., cameraSamplesPerPixel = 5000, cameraBatches = 4, outputCameraFile = 'cam.nc' /\n")
    cfg = driver_cli.read_namelists(str(nml))
    cam = driver_cli.camera_from_namelist(cfg, xe, ye, ze)
    assert (cam.kind, cam.npx, cam.npy, cam.position, cam.look, cam.up, cam.fov) == ("pinhole", 64, 48, (0.5, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 90.0)
    assert (cfg["camerasamplesperpixel"], cfg["camerabatches"], cfg["outputcamerafile"]) == (5000, 4, "cam.nc")
    nml.write_text("&camera cameraKind = 'orthographic', cameraPixels = 8, 2, cameraMu = 0.6, cameraPhi = 110. /\n")
    cam = driver_cli.camera_from_namelist(driver_cli.read_namelists(str(nml)), xe, ye, ze)
    assert (cam.kind, cam.npx, cam.npy, cam.mu, cam.phi, cam.footprint, cam.height) == ("orthographic", 8, 2, 0.6, 110.0, (0.0, 2.0, 0.0, 3.0), 1.5)
    nml.write_text("&camera cameraKind = 'orthographic', cameraFootprint = 0.5, 1.5, 1., 2., cameraHeight = 0.25 /\n")
    cam = driver_cli.camera_from_namelist(driver_cli.read_namelists(str(nml)), xe, ye, ze)
    assert (cam.npx, cam.npy, cam.footprint, cam.height) == (1, 1, (0.5, 1.5, 1.0, 2.0), 0.25)


def test_the_namelist_driver_refuses_the_camera_for_spectral_jobs(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    made = []
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: [object(), object()])
    import mcbrat3d_amd
    monkeypatch.setattr(mcbrat3d_amd, "new_Integrator", lambda *a, **k: made.append(a))
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&camera cameraKind = 'pinhole' /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="cameraKind"):
        driver_cli.main([str(nml)])
    assert not made


def _result(cam, batches=3, seed=2):
    rng = np.random.default_rng(seed)
    return {"radiance": rng.random((cam.npy, cam.npx), np.float32), "radiance_StdErr": rng.random((cam.npy, cam.npx), np.float32),
            "batchMeans": rng.random((batches, cam.npy, cam.npx), np.float32), "dropped": 0, "samplesPerPixel": 5000}


@pytest.mark.parametrize("kind", ["pinhole", "orthographic"])
def test_netcdf_round_trip_of_the_camera_variables(tmp_path, kind):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import ncio
    cam = _camera(kind, dict(OK_P if kind == "pinhole" else OK_O, npx=5, npy=3))
    res = _result(cam)
    out = str(tmp_path / "cam.nc")
    ncio.writeCamera_netcdf(out, cam, res)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.variables["cameraRadiance"].dimensions == ("cameraY", "cameraX") and f.dimensions["cameraX"] == 5 and f.dimensions["cameraY"] == 3
        assert np.array_equal(f.variables["cameraRadiance"][:], res["radiance"])
        assert np.array_equal(f.variables["cameraRadiance_StdErr"][:], res["radiance_StdErr"])
        assert f.cameraKind.decode() == kind and list(f.cameraPixels) == [5, 3] and f.cameraBatches == 3 and f.cameraSamplesPerPixel == 5000
        if kind == "pinhole":
            assert list(f.cameraPosition) == [0.0, 0.0, 0.0] and list(f.cameraLook) == [0.0, 0.0, 1.0] and f.cameraFov == 60.0
        else:
            assert f.cameraMu == 0.5 and f.cameraPhi == 10.0 and list(f.cameraFootprint) == [0.0, 1.0, 0.0, 1.0] and f.cameraHeight == 0.5
    finally:
        f.close()


def test_the_result_file_carries_the_camera_beside_the_fluxes(tmp_path):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import ncio
    cam = _camera("orthographic", dict(OK_O, npx=2, npy=3))
    res = _result(cam)
    stats = {"totalPhotons": 10, "batches": 2}
    for name in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        stats[name] = stats[name + "_StdErr"] = np.zeros((2, 3), np.float32)
    e = np.array([0.0, 1.0, 2.0])
    with_cam, without = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    ncio.writeResults_netcdf(with_cam, "d", stats, e, np.array([0.0, 1.0, 2.0, 3.0]), e, camera=cam, cameraResult=res)
    ncio.writeResults_netcdf(without, "d", stats, e, np.array([0.0, 1.0, 2.0, 3.0]), e)
    a, b = netcdf_file(with_cam, "r", mmap=False), netcdf_file(without, "r", mmap=False)
    try:
        assert set(a.variables) - set(b.variables) == {"cameraRadiance", "cameraRadiance_StdErr"}
        assert np.array_equal(a.variables["cameraRadiance"][:], res["radiance"]) and np.array_equal(a.variables["fluxUp"][:], b.variables["fluxUp"][:])
        assert not hasattr(b, "cameraKind")
    finally:
        a.close()
        b.close()


def test_every_layer_declares_the_entries():
    from mcbrat3d_amd import _capi, build, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    cam = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_camera.hip")).read()
    for sym, nargs in (("mcbrat_render_camera", 10), ("mcbrat_camera_ray", 7), ("mcbrat_sun_transmittance", 4)):
        assert re.search(r"\bint %s\(" % sym, text) and re.search(r"\bint %s\(" % sym, cam)
        assert len(_capi.SYMBOLS[sym][1]) == nargs
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    L = _capi.lib()  # resolves every symbol of SYMBOLS
    assert L.mcbrat_abi_version() == 3
    # the struct of the binding is the header's, member for member
    members = re.search(r"typedef struct mcbrat_camera \{(.*?)\} mcbrat_camera;", text, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", members, flags=re.S)
    names = [n.split("[")[0] for decl in re.findall(r"(?:int32_t|float|double)\s+([^;]+);", members) for n in re.split(r",\s*", decl.strip())]
    assert names == [n for n, _ in _capi.Camera._fields_]
    assert C.sizeof(_capi.Camera) == 5 * 4 + 2 * 4 + 4 + 5 * 8 + 9 * 8 + 8  # (4 bytes of padding before the doubles, fovXDeg padded to 8)
    assert "mcbrat_camera.hip" in build.SOURCES and {"mcbrat_camera_ray.h", "mcbrat_camera_ctx.h"} <= set(build.DEPS)
    for name in ("renderCamera", "sunTransmittance"):
        assert hasattr(integrator.Integrator, name)
    # the messages live with the camera code: nothing of it in the variant table
    variants = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_variants.h")).read()
    assert "amera" not in variants


def test_the_library_maps_pixels_as_the_header_does():
    from mcbrat3d_amd import _capi
    L = _capi.lib()
    s = _camera("pinhole", PINHOLES[2]).struct()
    o, d = np.zeros(3), np.zeros(3)
    assert L.mcbrat_camera_ray(C.addressof(s), 1, 4, 0.25, 0.75, _capi.ptr(o), _capi.ptr(d)) == 0
    eo, ed = pinhole_ray(i=1, j=4, u=0.25, v=0.75, **PINHOLES[2])
    assert np.array_equal(o, eo) and np.allclose(d, ed, rtol=0, atol=1e-14)
    s.fovXDeg = 180.0
    assert L.mcbrat_camera_ray(C.addressof(s), 0, 0, 0.5, 0.5, _capi.ptr(o), _capi.ptr(d)) != 0
    assert L.mcbrat_camera_ray(None, 0, 0, 0.5, 0.5, _capi.ptr(o), _capi.ptr(d)) != 0


def test_fortran_shim_declares_the_camera_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("camera", "renderCamera", "sunTransmittance"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_render_camera", "mcbrat_sun_transmittance"):
        assert 'name="%s"' % sym in text
    # the bind(C) type mirrors the struct: the same members in the same order
    block = re.search(r"type, bind\(C\) :: camera(.*?)end type camera", text, re.S).group(1)
    names = [re.split(r"[ (=]", n.strip())[0] for decl in re.findall(r"::\s*(.+)", block) for n in re.split(r",\s*(?=[A-Za-z])", re.sub(r"\(/.*?/\)", "", decl))]
    from mcbrat3d_amd import _capi
    assert names == [n for n, _ in _capi.Camera._fields_], names
    nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("rendercamera", "suntransmittance"):
        assert re.search(r"\bt\b.*%s" % name, symbols), name
