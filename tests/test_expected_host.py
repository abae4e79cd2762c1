"""The expected-value estimator of the emission renders without a GPU: tests/expected_dump.cpp, a
stand-alone program over mcbrat3d_amd/csrc/mcbrat_expected.h alone, plain and under the address and undefined-behaviour
sanitizers, held to closed forms written out in double -- the segment term, E[v], the cut, the LDS byte count --, and what every
layer declares: the header, the binding, the shim, the namelist key, the NetCDF attribute."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")

# The largest relative deviation of expected_segment() from T_in (-expm1(-dtau)) in double over the grid below: 1.55e-7, 1.3
# units in the last place of a float.  The bound is four times that, and never looser than 16 units.
SEGMENT_MEASURED = 1.55e-7
SEGMENT_BOUND = min(4.0 * SEGMENT_MEASURED, 16.0 * 2.0 ** -24)


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "expected_dump.cpp")])
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("expected")
    return (_compile(str(d / "expected_dump")),
            _compile(str(d / "expected_dump_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def ask(exes, questions):
    """the answers of both builds, one list of words per question: the same lines from both (check=True: a sanitizer's finding
    ends the program with a failure)"""
    text = "".join(" ".join("%.9g" % x if isinstance(x, (float, np.floating)) else str(x) for x in q) + "\n" for q in questions)
    plain, sanitized = (subprocess.run([e], input=text, check=True, capture_output=True, text=True, timeout=120).stdout for e in exes)
    assert plain == sanitized
    lines = plain.splitlines()
    assert len(lines) == len(questions)
    return [ln.split() for ln in lines]


def test_the_dump_program_includes_only_the_header():
    text = open(os.path.join(ROOT, "tests", "expected_dump.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_expected.h"]
    header = open(os.path.join(CSRC, "mcbrat_expected.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and not re.findall(r'#include\s+"([^"]+)"', header)
    from mcbrat3d_amd import build
    assert "mcbrat_expected.h" in build.DEPS and "mcbrat_expected.h" not in build.SOURCES
    assert build.SOURCES == ["mcbrat_api.hip", "mcbrat_host.cpp", "mcbrat_camera.hip"]
    cam = open(os.path.join(CSRC, "mcbrat_camera.hip")).read()
    # the kernels and the host half call the header: nothing of it is stated a second time
    assert '#include "mcbrat_expected.h"' in cam
    for call in ("expected_segment(", "expected_emission(", "expected_lds_bytes(", "kExpectedTauCut"):
        assert call in cam, call
    assert "expm1f" not in cam and "30.0f" not in cam


def test_the_segment_term(exes):
    dtau = np.float32(10.0 ** np.linspace(-12.0, 2.0, 141))
    tin = np.float32(np.concatenate([[0.0], 10.0 ** np.linspace(-6.0, 0.0, 25), np.linspace(1.0, 40.0, 79)]))
    cases = [(a, b) for a in tin for b in dtau]
    got = np.array([float(w[0]) for w in ask(exes, [("seg", a, b) for a, b in cases])])
    ref = np.array([math.exp(-float(a)) * -math.expm1(-float(b)) for a, b in cases])
    dev = np.abs(got / ref - 1.0)
    worst = int(dev.argmax())
    print("segment term: largest relative deviation %.3g (%.2f units in the last place) at tau_in = %g, dtau = %g; bound %.3g" % (
        dev[worst], dev[worst] / 2.0 ** -23, cases[worst][0], cases[worst][1], SEGMENT_BOUND))
    assert dtau[0] == np.float32(1e-12) and dtau[-1] == 100.0 and tin[0] == 0.0 and tin[-1] == 40.0
    assert np.all(got > 0.0) and np.all(dev <= SEGMENT_BOUND), (dev[worst], cases[worst])
    # a thin segment is its optical depth, a thick one at the origin everything; nothing of a segment of length 0
    assert float(ask(exes, [("seg", 0.0, 0.0)])[0][0]) == 0.0
    assert float(ask(exes, [("seg", 0.0, 200.0)])[0][0]) == 1.0
    assert np.float32(float(ask(exes, [("seg", 0.0, 1e-9)])[0][0])) == np.float32(1e-9)


def test_the_cells_emission(exes):
    f32 = lambda *v: [float(np.float32(x)) for x in v]  # noqa: E731
    one = ask(exes, [("emis", 1, 1.5, 2.0, 0.25), ("emis", 1, 1.5, 2.0, 1.0), ("emis", 1, 1.5, 2.0, 0.0)])
    assert [np.float32(float(w[0])) for w in one] == [np.float32(2.0 * (1.0 - 0.25)), 0.0, 2.0]
    # two and three components: the sum written out in double over the floats the program reads
    S, = f32(3.7)
    c0, = f32(0.35)
    s0, s1 = f32(0.9, 0.3)
    two = float(np.float32(S * ((c0 - 0.0) * (1.0 - s0) + (1.0 - c0) * (1.0 - s1))))
    d0, d1 = f32(0.2, 0.7)
    t0, t1, t2 = f32(0.95, 0.3, 0.5)
    three = float(np.float32(S * (d0 * (1.0 - t0) + (d1 - d0) * (1.0 - t1) + (1.0 - d1) * (1.0 - t2))))
    got = ask(exes, [("emis", 2, 0.8, S, c0, s0, s1), ("emis2", 2, 0.8, S, c0, s0, s1), ("emis", 3, 0.8, S, d0, d1, t0, t1, t2),
                     ("emis2", 3, 0.8, S, d0, d1, t0, t1, t2)])
    assert [np.float32(float(w[0])) for w in got] == [np.float32(x) for x in (two, two, three, three)]   # (9 digits: the float's own bits)
    # the last cumulative fraction counts as 1 whatever the array holds behind it; a cell of extinction 0 gives exactly 0 whatever
    # ssa and the fractions hold there
    zero = ask(exes, [("emis", 1, 0.0, 5.0, "nan"), ("emis", 3, 0.0, 5.0, "nan", "nan", "nan", "nan", "nan"), ("emis2", 2, 0.0, 5.0, "nan", 0.5, "nan")])
    assert [w[0] for w in zero] == ["0", "0", "0"]


def test_the_cut_and_the_lds_bytes(exes):
    got = ask(exes, [("cut",), ("lds", 24, 24, 24), ("lds", 1, 1, 1), ("lds", 7, 3, 5), ("lds", 2048, 2048, 128)])
    cut = float(got[0][0])
    assert cut == 30.0 and math.exp(-cut) < 2.0 ** -43
    assert [int(w[0]) for w in got[1:]] == [4 * 24 ** 3, 4, 4 * 105, 4 * 2048 * 2048 * 128]   # 4 bytes per cell, 64-bit
    # the fit edge of DESIGN.md section 4.24: against 80 KB - 1 KB a grid of 24 x 24 x 24 fits alone and not with the second grid;
    # the largest cubes that fit with it and alone
    share = 80 * 1024 - 1024

    def grid_bytes(n):
        return 8 * (3 * n + 3) + 4 * n ** 3

    def pair(n):
        return ((grid_bytes(n) + 7) & ~7) + int(ask(exes, [("lds", n, n, n)])[0][0])
    assert grid_bytes(24) <= share < pair(24)
    assert pair(21) <= share < pair(22) and grid_bytes(27) <= share < grid_bytes(28)


def test_a_question_the_program_cannot_read_is_an_error(exes):
    for e in exes:
        assert subprocess.run([e], input="seg 1\n", capture_output=True, text=True, timeout=60).returncode == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# every layer declares the entries
# ---------------------------------------------------------------------------------------------------------------------------------
ENTRIES = (("mcbrat_render_camera_emission_expected", "mcbrat_render_camera_emission", 12),
           ("mcbrat_render_sensors_emission_expected", "mcbrat_render_sensors_emission", 14))


def _arguments(text, sym):
    decl = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]


def test_every_layer_declares_the_entries():
    from mcbrat3d_amd import _capi, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    cam = open(os.path.join(CSRC, "mcbrat_camera.hip")).read()
    L = _capi.lib()
    for sym, model, nargs in ENTRIES:
        assert re.search(r"\bint %s\(" % sym, text) and re.search(r"\bint %s\(" % sym, cam)
        assert _arguments(text, sym) == _arguments(text, model) and len(_arguments(text, sym)) == nargs   # exactly the emission entry's list
        res, args = _capi.SYMBOLS[sym]
        assert res is C.c_int and len(args) == nargs and args == _capi.SYMBOLS[model][1] and getattr(L, sym).argtypes == args
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3 and L.mcbrat_abi_version() == 3
    comment = re.search(r"/\* The emission renders with the expected-value.*?\*/", text, re.S).group(0)
    for word in ("collision estimator's paths", "optical depth 30", "counted in `dropped`", "formal\n * solution"):
        assert word in comment, word
    # the kernel: a sixth template parameter, instantiated for the two emission receivers, grid in LDS and in global memory
    assert "bool PATHLEN = false, bool EXPECT = false>" in cam
    for inst in ("camera_kernel<512, true, false, true, false, true>", "camera_kernel<256, false, false, true, false, true>",
                 "camera_kernel<512, true, true, true, false, true>", "camera_kernel<256, false, true, true, false, true>"):
        assert cam.count(inst) == 1, inst
    assert "march_expected(" in cam and cam.count("hipLaunchKernelGGL") <= 3 and "DeviceBuffer<float> dFwd, dSrcCell, dSrcSurface, dEdges, dEmis;" in cam
    assert cam.count('"renderCameraEmissionExpected"') == 1 and cam.count('"renderSensorsEmissionExpected"') == 1
    # CamParams gains its member at the end
    params = re.search(r"struct CamParams \{(.*?)\n\};", cam, re.S).group(1)
    assert re.findall(r"(\w+);\s*(?://.*)?$", params.strip().splitlines()[-1])[0] == "emisCell"
    import inspect
    for name in ("renderCameraEmission", "renderSensorsEmission"):
        sig = inspect.signature(getattr(integrator.Integrator, name))
        assert list(sig.parameters)[-1] == "estimator" and sig.parameters["estimator"].default == "collision"


def test_an_unknown_estimator_is_refused_before_anything_else():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import integrator
    bare = integrator.Integrator.__new__(integrator.Integrator)   # (no context: the keyword is looked at first)
    for name in ("renderCameraEmission", "renderSensorsEmission"):
        with pytest.raises(M.McbratError, match="estimator must be 'collision' or 'expected'"):
            getattr(bare, name)(None, None, 1, estimator="track-length")


def test_the_fortran_shim_declares_the_entries(tmp_path):
    src = open(os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")).read()
    for sym, _, _ in ENTRIES:
        assert 'bind(C, name="%s")' % sym in src
    for name in ("renderCameraEmissionExpected", "renderSensorsEmissionExpected"):
        assert "subroutine %s(" % name in src and "end subroutine %s" % name in src
        assert name in src.split("contains")[0]                                      # public
    assert re.search(r"ierr = mcbrat_render_camera_emission_expected\(", src) and re.search(r"ierr = mcbrat_render_sensors_emission_expected\(", src)
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is not None:   # (where there is a Fortran compiler: the shim compiles and defines both routines)
        subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90"), "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
        nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
        symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
        for name in ("rendercameraemissionexpected", "rendersensorsemissionexpected"):
            assert re.search(r"\bt\b.*%s" % name, symbols), name


def test_the_namelist_key_and_its_default(tmp_path):
    from mcbrat3d_amd import driver_cli
    head = "&monteCarlo numPhotonsPerBatch = 10 /\n"
    nml = tmp_path / "run.nml"
    nml.write_text(head + "&camera cameraKind = 'pinhole', emission = .true. /\n&sensors sensorKind = 'planar', emission = T /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemissionestimator"] == "collision" and cfg["sensorsemissionestimator"] == "collision" and "emissionestimator" not in cfg
    nml.write_text(head)                                                               # neither group: as every existing namelist
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemissionestimator"] == "collision" and cfg["sensorsemissionestimator"] == "collision" and cfg["cameraemission"] is False
    nml.write_text(head + "&camera cameraKind = 'pinhole', emission = .true., emissionEstimator = 'expected' /\n&sensors sensorKind = 'planar', emission = T /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemissionestimator"] == "expected" and cfg["sensorsemissionestimator"] == "collision" and cfg["cameraemission"] is True
    nml.write_text(head + "&camera cameraKind = 'pinhole' /\n&sensors sensorKind = 'planar', emission = T, emissionEstimator = 'expected', sensorSamples = 77 /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["cameraemissionestimator"] == "collision" and cfg["sensorsemissionestimator"] == "expected" and cfg["sensorsamples"] == 77
    # 'collision' may be spelled out with and without emission; 'expected' without emission and any other word are errors
    nml.write_text(head + "&camera cameraKind = 'pinhole', emissionEstimator = 'collision' /\n")
    assert driver_cli.read_namelists(str(nml))["cameraemissionestimator"] == "collision"
    for group, body, word in (("camera", "cameraKind = 'pinhole', emissionEstimator = 'expected'", "needs emission"),
                              ("sensors", "sensorKind = 'planar', emission = .false., emissionEstimator = 'expected'", "needs emission"),
                              ("camera", "cameraKind = 'pinhole', emission = .true., emissionEstimator = 'tracklength'", "must be")):
        nml.write_text(head + "&%s %s /\n" % (group, body))
        with pytest.raises(SystemExit, match=word) as err:
            driver_cli.read_namelists(str(nml))
        assert str(err.value).startswith(group + ":")


def _fixtures():
    """the dicts tests/golden/expected_*_parent.nc were written from, by the writer as it was before the attribute"""
    from mcbrat3d_amd.camera import new_Camera
    from mcbrat3d_amd.sensors import new_Sensors
    rng = np.random.default_rng(24)
    cam = new_Camera("orthographic", npx=3, npy=2, mu=0.8, phi=20.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25)
    image = dict(radiance=rng.uniform(5, 9, (2, 3)).astype(np.float32), radiance_StdErr=rng.uniform(0, 0.1, (2, 3)).astype(np.float32),
                 batchMeans=np.zeros((4, 2, 3), np.float32), dropped=0, samplesPerPixel=128, emission=True)
    sens = new_Sensors([(0.1, 0.2, 0.0), (0.3, 0.1, 0.25)], tilt=[0.0, 180.0])
    irr = dict(irradiance=rng.uniform(20, 30, 2).astype(np.float32), irradiance_StdErr=rng.uniform(0, 0.1, 2).astype(np.float32),
               batchMeans=np.zeros((5, 2), np.float32), dropped=0, samplesPerSensor=64, emission=True)
    return cam, image, sens, irr


def test_netcdf_round_trip_with_and_without_the_attribute(tmp_path):
    from scipy.io import netcdf_file
    from mcbrat3d_amd import ncio
    cam, image, sens, irr = _fixtures()
    # without the attribute -- no key, and the collision estimator named --: the bytes the writer gave before
    for k, (img, ir) in enumerate(((image, irr), (dict(image, estimator="collision"), dict(irr, estimator="collision")))):
        ncio.writeCamera_netcdf(str(tmp_path / ("cam%d.nc" % k)), cam, img)
        ncio.writeSensors_netcdf(str(tmp_path / ("sen%d.nc" % k)), sens, ir)
        assert open(str(tmp_path / ("cam%d.nc" % k)), "rb").read() == open(os.path.join(GOLDEN, "expected_camera_parent.nc"), "rb").read()
        assert open(str(tmp_path / ("sen%d.nc" % k)), "rb").read() == open(os.path.join(GOLDEN, "expected_sensors_parent.nc"), "rb").read()
    back = ncio.readCamera_netcdf(str(tmp_path / "cam0.nc"))
    assert "cameraEstimator" not in back and np.array_equal(back["cameraEmission"], image["radiance"])
    assert "sensorEstimator" not in ncio.readSensors_netcdf(str(tmp_path / "sen0.nc"))
    # with it: an attribute of the emission variable, returned by the readers; everything else as before
    ncio.writeCamera_netcdf(str(tmp_path / "camx.nc"), cam, dict(image, estimator="expected"))
    ncio.writeSensors_netcdf(str(tmp_path / "senx.nc"), sens, dict(irr, estimator="expected"))
    back = ncio.readCamera_netcdf(str(tmp_path / "camx.nc"))
    assert back["cameraEstimator"] == "expected" and np.array_equal(back["cameraEmission"], image["radiance"]) and back["cameraBatches"] == 4
    assert np.array_equal(back["cameraEmission_StdErr"], image["radiance_StdErr"]) and back["cameraSamplesPerPixel"] == 128
    back = ncio.readSensors_netcdf(str(tmp_path / "senx.nc"))
    assert back["sensorEstimator"] == "expected" and np.array_equal(back["sensorEmission"], irr["irradiance"]) and back["sensorBatches"] == 5
    for name, var in (("camx.nc", "cameraEmission"), ("senx.nc", "sensorEmission")):
        f = netcdf_file(str(tmp_path / name), "r", mmap=False)
        try:
            assert f.variables[var].estimator.decode() == "expected" and not hasattr(f.variables[var + "_StdErr"], "estimator")
        finally:
            f.close()
    # a solar result never carries it, whatever the dict says
    ncio.writeCamera_netcdf(str(tmp_path / "solar.nc"), cam, dict(image, emission=False, estimator="expected"))
    assert "cameraEstimator" not in ncio.readCamera_netcdf(str(tmp_path / "solar.nc"))
