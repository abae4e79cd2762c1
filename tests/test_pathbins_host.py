"""The path-length bins without a GPU: tests/pathbins_dump.cpp, a stand-alone program over
mcbrat3d_amd/csrc/mcbrat_pathbins.h alone, plain and under the address and undefined-behaviour sanitizers -- path_bin held to
numpy.searchsorted on and next to every edge, path_edges_refusal rule by rule --, the two brackets of mcbrat3d_amd.camera held to
closed forms, and the new entry in the library and in the binding."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")
F32 = np.float32


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "pathbins_dump.cpp")])
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("pathbins")
    return (_compile(str(d / "pathbins_dump")),
            _compile(str(d / "pathbins_dump_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _word(x):
    return repr(float(x)) if isinstance(x, (float, np.floating)) else str(x)


def ask(exes, questions):
    """the answers of both builds, one line per question: the same lines from both (check=True: a sanitizer's finding ends the
    program with a failure)"""
    text = "".join(" ".join(_word(x) for x in q) + "\n" for q in questions)
    plain, sanitized = (subprocess.run([e], input=text, check=True, capture_output=True, text=True, timeout=60).stdout for e in exes)
    assert plain == sanitized
    lines = plain.splitlines()
    assert len(lines) == len(questions)
    return lines


def test_the_dump_program_includes_only_the_header():
    text = open(os.path.join(ROOT, "tests", "pathbins_dump.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_pathbins.h"]
    header = open(os.path.join(CSRC, "mcbrat_pathbins.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and not re.findall(r'#include\s+"([^"]+)"', header)
    assert "kMaxPathBins = 256" in header
    from mcbrat3d_amd import build
    assert "mcbrat_pathbins.h" in build.DEPS and "mcbrat_pathbins.h" not in build.SOURCES
    cam = open(os.path.join(CSRC, "mcbrat_camera.hip")).read()
    assert '#include "mcbrat_pathbins.h"' in cam and "path_bin(" in cam and "path_edges_refusal(" in cam
    assert cam.count("hipLaunchKernelGGL") <= 3


EDGES = {
    1: np.array([0.0], F32),
    2: np.array([0.0, 0.75], F32),
    3: np.array([0.0, 1e-3, 7.5], F32),
    256: np.concatenate([[0.0], np.cumsum(np.random.default_rng(11).uniform(1e-3, 2.0, 255))]).astype(F32),
}


def _values(e):
    inf = F32(np.inf)
    v = [x for edge in e for x in (edge, np.nextafter(edge, -inf), np.nextafter(edge, inf))]
    v += [F32(0.0), F32(-0.0), F32(-1.0), F32(-1e30), -inf, F32(3e38), inf, F32(np.finfo(F32).tiny), F32(0.5) * (e[-1] + F32(1.0))]
    v += list(0.5 * (e[1:] + e[:-1]))
    return np.array(v, F32)


@pytest.mark.parametrize("n", sorted(EDGES))
def test_path_bin_is_searchsorted_right_minus_one(exes, n):
    e = EDGES[n]
    assert e.size == n and e[0] == 0.0 and np.all(np.diff(e) > 0)
    v = _values(e)
    got = np.array(ask(exes, [("bin",) + tuple(e) + ("|",) + tuple(v)])[0].split(), int)
    want = np.clip(np.searchsorted(e, v, "right") - 1, 0, n - 1)
    assert got.shape == want.shape and np.array_equal(got, want), (n, v[got != want], got[got != want], want[got != want])
    # every bin occurs; a value on an edge is in the upper bin, the one just below it in the lower one
    assert set(got) == set(range(n))
    assert all(got[3 * b] == b and got[3 * b + 1] == max(b - 1, 0) for b in range(n))
    if n > 1:
        assert ask(exes, [("bin",) + tuple(e) + ("|", float("nan"))]) == ["0"]   # (a NaN compares with nothing: bin 0; the kernel deposits none)


def test_path_edges_refusal_rule_by_rule(exes):
    ok = [0.0, 0.5, 2.0]
    q = [("edges", 3) + tuple(ok), ("edges", 1, 0.0), ("edges", 256) + tuple(float(x) for x in EDGES[256]),
         ("edges", 0), ("edges", 257) + tuple(float(x) for x in range(257)), ("edges", -1),
         ("edges", 3, "null"),
         ("edges", 3, 0.0, float("inf"), 2.0), ("edges", 3, 0.0, 1.0, float("nan")),
         ("edges", 3, 0.1, 0.5, 2.0), ("edges", 3, -1.0, 0.5, 2.0),
         ("edges", 3, 0.0, 0.5, 0.5), ("edges", 3, 0.0, 2.0, 0.5), ("edges", 2, 0.0, -0.0)]
    got = ask(exes, q)
    assert got[:3] == ["ok"] * 3
    for line in got[3:6]:
        assert "numBins must be between 1 and 256" in line
    assert "no pathEdges array" in got[6]
    assert all("not finite" in x for x in got[7:9])
    assert all("pathEdges[0] must be 0" in x for x in got[9:11])
    assert all("strictly ascending" in x for x in got[11:14])
    # -0 is 0
    assert ask(exes, [("edges", 2, -0.0, 1.0)]) == ["ok"]


def test_a_question_the_program_cannot_read_is_an_error(exes):
    for e in exes:
        assert subprocess.run([e], input="bin 0.0\n", capture_output=True, text=True, timeout=60).returncode == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the brackets
# ---------------------------------------------------------------------------------------------------------------------------------
def test_absorbed_radiance_closed_forms():
    from mcbrat3d_amd.camera import absorbed_radiance
    k = 0.7
    # one bin: it is the open one -- lengths from 0 up, the radiance under the absorber anywhere between 0 and all of it
    lo, up = absorbed_radiance(np.array([0.25]), [0.0], k)
    assert lo == 0.0 and up == 0.25
    # a delta in a closed bin: the two edges' exponentials
    e = np.array([0.0, 1.0, 1.5, 4.0])
    rad = np.array([0.0, 0.4, 0.0, 0.0])
    lo, up = absorbed_radiance(rad, e, k)
    assert lo == pytest.approx(0.4 * np.exp(-k * 1.5), rel=1e-15) and up == pytest.approx(0.4 * np.exp(-k * 1.0), rel=1e-15)
    # k = 0: both bounds are the sum, the open bin included
    rad = np.array([0.1, 0.2, 0.3, 0.05])
    lo, up = absorbed_radiance(rad, e, 0.0)
    assert lo == up == rad.sum()
    # the open bin: nothing to the lower bound, its lower edge to the upper bound
    lo, up = absorbed_radiance(np.array([0.0, 0.0, 0.0, 0.05]), e, k)
    assert lo == 0.0 and up == pytest.approx(0.05 * np.exp(-k * 4.0), rel=1e-15)
    # all of it, per pixel: images [bin, y, x]
    img = np.random.default_rng(3).uniform(0.0, 1.0, (4, 2, 3))
    lo, up = absorbed_radiance(img, e, k)
    assert lo.shape == up.shape == (2, 3)
    assert np.allclose(up, np.tensordot(np.exp(-k * e), img, 1), rtol=1e-15)
    assert np.allclose(lo, np.tensordot(np.exp(-k * e[1:]), img[:3], 1), rtol=1e-15)
    assert np.all(lo <= up)
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError):
        absorbed_radiance(img, e[:3], k)
    with pytest.raises(McbratError):
        absorbed_radiance(img, e, -1.0)


def test_mean_path_length_closed_forms():
    from mcbrat3d_amd.camera import mean_path_length
    e = np.array([0.0, 1.0, 1.5, 4.0])
    lo, up = mean_path_length(np.array([0.0, 0.4, 0.0, 0.0]), e)             # a delta in one bin: its two edges
    assert (lo, up) == pytest.approx((1.0, 1.5), rel=4e-16)                  # (0.4 x / 0.4 in double: an ulp)
    lo, up = mean_path_length(np.array([0.0, 0.4, 0.0, 9.0]), e)             # the open bin is left out
    assert (lo, up) == pytest.approx((1.0, 1.5), rel=4e-16)
    lo, up = mean_path_length(np.array([0.1, 0.1, 0.2, 0.0]), e)
    assert lo == pytest.approx((0.1 * 0.0 + 0.1 * 1.0 + 0.2 * 1.5) / 0.4, rel=1e-15) and up == pytest.approx((0.1 * 1.0 + 0.1 * 1.5 + 0.2 * 4.0) / 0.4, rel=1e-15)
    lo, up = mean_path_length(np.array([0.3]), [0.0])                       # one bin: no closed bin, no bracket
    assert np.isnan(lo) and np.isnan(up)
    img = np.random.default_rng(4).uniform(0.1, 1.0, (4, 2, 3))
    lo, up = mean_path_length(img, e)
    assert lo.shape == (2, 3) and np.all(lo < up) and np.all(up <= 4.0) and np.all(lo >= 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry: in the header, in the library, in the binding
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_the_binding_binds_it():
    import ctypes as C
    from mcbrat3d_amd import _capi
    header = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    assert re.search(r"\bint\s+mcbrat_render_camera_pathlengths\s*\(", header)
    assert "mcbrat_render_camera_pathlengths" in _capi.SYMBOLS
    res, args = _capi.SYMBOLS["mcbrat_render_camera_pathlengths"]
    assert res is C.c_int and len(args) == 12 and args[2] is C.c_int32 and args[4] is args[5] is C.c_uint64 and args[6] is C.c_int64
    assert hasattr(_capi.lib(), "mcbrat_render_camera_pathlengths")   # (lib() resolves every symbol of SYMBOLS in the built library)
    from mcbrat3d_amd.integrator import Integrator
    assert callable(getattr(Integrator, "renderCameraPathLengths"))
