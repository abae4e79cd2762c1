"""The host rules of a backward render without a GPU: tests/backward_dump.cpp, a stand-alone program over
mcbrat3d_amd/csrc/mcbrat_backward.h alone, plain and under the address and undefined-behaviour sanitizers, held to closed forms
written out here in double -- the two crossing bounds, the fixed-point scale, the capacity predicates at their edges, the launch
shape, the statistics of the batch means, the one reduction of the bins to the five entries' output layouts -- and that
mcbrat_camera.hip's host half states none of them, and no sentence of a refusal, a second time."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")
FLT_MIN = float(np.finfo(np.float32).tiny)
TWO62 = 2.0 ** 62


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "backward_dump.cpp")])
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("backward")
    return (_compile(str(d / "backward_dump")),
            _compile(str(d / "backward_dump_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def ask(exes, questions):
    """the answers of both builds to the questions, one list of words per question: the same lines from both (check=True: a
    sanitizer's finding ends the program with a failure)"""
    text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in q) + "\n" for q in questions)
    plain, sanitized = (subprocess.run([e], input=text, check=True, capture_output=True, text=True, timeout=60).stdout for e in exes)
    assert plain == sanitized
    lines = plain.splitlines()
    assert len(lines) == len(questions)
    return [ln.split() for ln in lines]


def test_the_dump_program_includes_only_the_header():
    text = open(os.path.join(ROOT, "tests", "backward_dump.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_backward.h"]
    header = open(os.path.join(CSRC, "mcbrat_backward.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and not re.findall(r'#include\s+"([^"]+)"', header)
    from mcbrat3d_amd import build
    assert "mcbrat_backward.h" in build.DEPS and "mcbrat_backward.h" not in build.SOURCES


def test_the_host_half_states_each_rule_once():
    cam = open(os.path.join(CSRC, "mcbrat_camera.hip")).read()
    assert '#include "mcbrat_backward.h"' in cam
    assert "65536.0" not in cam and "4.611686018427387904e18" not in cam
    assert cam.count("hipLaunchKernelGGL") <= 3
    assert cam.count("forward phase function table") == 1 and cam.count("phaseFunctionIndex exceeds forward table entries") == 1
    for call in ("sun_bound(", "leg_bound(", "fixed_point(", "bins_fit(", "paths_fit(", "launch_shape(", "reduce_batches("):
        assert call in cam, call
    # five entries, each rule once: no sentence of a refusal is worded twice, the batch statistics are the header's reduction alone,
    # the receivers' geometry is mapped in one front each (and in mcbrat_camera_ray, mcbrat_sensor_ray)
    sentences = re.findall(r'"([^"\n]{20,}\.)"', cam)
    assert len(sentences) >= 20 and [s for s in set(sentences) if sentences.count(s) > 1] == []
    for name in os.listdir(CSRC):
        if name.endswith((".h", ".hip", ".cpp")) and name != "mcbrat_backward.h":
            assert "BatchSeries" not in open(os.path.join(CSRC, name)).read(), name
    assert 1 <= cam.count("camera_geometry(") <= 2 and 1 <= cam.count("sensor_geometry(") <= 2 and 1 <= cam.count("std::memset(&cp") <= 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the crossing bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _sun(mu0, phi0):
    s = math.sqrt(1.0 - mu0 * mu0)
    return [float(np.float32(x)) for x in (s * math.cos(math.radians(phi0)), s * math.sin(math.radians(phi0)), mu0)]


BOXES = {  # nx, ny, nz, H, Lx, Ly
    "a 2 x 2 x 2 unit cube": (2, 2, 2, 1.0, 1.0, 1.0),
    "flat and wide": (2 ** 20, 2 ** 20, 4, 0.1, 100.0, 70.0),
    "unequal": (7, 3, 5, 0.35, 0.9, 2.5),
}
SUNS = {"overhead": [0.0, 0.0, 1.0], "0.5, 30": _sun(0.5, 30.0), "0.05, 200": _sun(0.05, 200.0),
        "grazing": [float(np.float32(0.6)), float(np.float32(-0.8)), 0.0]}  # (every component a float: the program reads them as floats)


def sun_bound(nx, ny, nz, H, Lx, Ly, sun):
    muz = max(abs(sun[2]), FLT_MIN)
    n = nz + (math.floor(H * abs(sun[0]) / muz / Lx) + 2.0) * nx + (math.floor(H * abs(sun[1]) / muz / Ly) + 2.0) * ny + 8.0
    return int(min(n, 2.0 ** 32 - 1)), np.float32(1.0 / (4.0 * math.pi * muz))


def leg_bound(nx, ny, nz, H, Lx, Ly):
    travel = H * 65536.0
    n = nz + (math.floor(travel / Lx) + 2.0) * nx + (math.floor(travel / Ly) + 2.0) * ny + 8.0
    return int(min(n, 2.0 ** 26))


def test_crossing_bounds(exes):
    cases = [(b, s) for b in BOXES for s in SUNS]
    got = ask(exes, [("sun",) + BOXES[b] + tuple(SUNS[s]) for b, s in cases] + [("leg",) + BOXES[b] for b in BOXES])
    for (b, s), w in zip(cases, got):
        n, inv = sun_bound(*BOXES[b], SUNS[s])
        assert int(w[0]) == n and np.float32(w[1]) == inv, (b, s, w, n, inv)
    legs = {b: int(w[0]) for b, w in zip(BOXES, got[len(cases):])}
    assert legs == {b: leg_bound(*BOXES[b]) for b in BOXES}
    # the cube by hand: overhead 2 + 2 * 2 + 2 * 2 + 8; a leg crosses 65536 domain lengths along x and along y
    assert sun_bound(*BOXES["a 2 x 2 x 2 unit cube"], SUNS["overhead"])[0] == 18 and legs["a 2 x 2 x 2 unit cube"] == 2 + 2 * 65538 * 2 + 8
    assert sun_bound(*BOXES["a 2 x 2 x 2 unit cube"], SUNS["0.5, 30"])[0] == 2 + (1 + 2) * 2 + (0 + 2) * 2 + 8  # tan(60 deg) cos / sin(30 deg) = 1.5, 0.87
    # where the cap binds, and where the clamp of mu to FLT_MIN saturates the sun's bound
    assert legs["flat and wide"] == 2 ** 26 and legs["unequal"] < 2 ** 26
    assert sun_bound(*BOXES["flat and wide"], SUNS["0.05, 200"])[0] < 2 ** 32 - 1
    for b in BOXES:
        assert sun_bound(*BOXES[b], SUNS["grazing"]) == (2 ** 32 - 1, np.float32(1.0 / (4.0 * math.pi * FLT_MIN)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixed-point scale
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fixed_point_scale(exes):
    cases = [(samples, largest) for samples in (1, 197, 2 ** 40) for largest in (1.0 / math.pi, 50.0, 1e30)]
    got = ask(exes, [("scale", s, big) for s, big in cases] + [("scale", 197, 0.1, 50.0, 0.3), ("scale", 197, 50.0, 1.0 / math.pi), ("scale", 197, 1.0 / math.pi, 50.0)])
    exponents = []
    for (samples, largest), w in zip(cases, got):
        scale, path_max = float(w[0]), float(w[1])
        m, e = math.frexp(scale)
        assert m == 0.5 and 0 <= e - 1 <= 40, (samples, largest, scale)      # a power of two
        e -= 1
        assert e == max(0, min(math.frexp(TWO62 / (float(samples) * largest * 64.0))[1] - 1, 40))
        if e > 0:
            assert float(samples) * 64.0 * largest * scale < TWO62, (samples, largest, scale)
        if 0 < e < 40:   # ... and the largest power of two that does
            assert float(samples) * 64.0 * largest * scale * 2.0 >= TWO62
        assert path_max == math.floor(TWO62 / float(samples))
        exponents.append(e)
    assert exponents == [40, 40, 0, 40, 40, 0, 17, 10, 0]   # both clamps and the free range occur
    assert got[len(cases)] == got[len(cases) + 1] == got[len(cases) + 2] == got[cases.index((197, 50.0))]   # the largest candidate, wherever it stands


# ---------------------------------------------------------------------------------------------------------------------------------
# capacity, launch shape
# ---------------------------------------------------------------------------------------------------------------------------------
def test_capacity_predicates_at_their_edges(exes):
    four_gib = 4 * 2 ** 30
    bins = [(n, nb, arrays) for arrays in (1, 2) for nb in (1, 2 ** 20) for n in (four_gib // (8 * arrays * nb), four_gib // (8 * arrays * nb) + 1)]
    bins += [(2 ** 31 - 1, 1, 1), (2 ** 31, 1, 1), (2 ** 31, 1, 2), (1, 2 ** 29, 1), (1, 2 ** 29 + 1, 1), (1, 2 ** 28 + 1, 2)]
    paths = [(9 * 10 ** 18 - 1024, 1, 0, 1), (9 * 10 ** 18, 1, 0, 1), (3 * 10 ** 9, 3 * 10 ** 9, 0, 1), (3 * 10 ** 9 - 1, 3 * 10 ** 9, 0, 1),
             (1, 1, 18 * 10 ** 18 - 4096, 1), (1, 1, 18 * 10 ** 18, 1), (1, 9 * 10 ** 18, 0, 2), (1, 2 ** 40, 2 ** 63, 3)]
    got = ask(exes, [("bins",) + b for b in bins] + [("paths",) + p for p in paths])
    for (n, nb, arrays), w in zip(bins, got):
        assert int(w[0]) == int(n <= 2 ** 31 - 1 and arrays * n * nb * 8 <= four_gib), (n, nb, arrays, w)
    for (nbins, samples, first, nb), w in zip(paths, got[len(bins):]):
        assert int(w[0]) == int(not (float(nbins) * float(samples) >= 9.0e18 or float(first) + float(nb) * float(samples) >= 1.8e19)), (nbins, samples, first, nb, w)
    # exactly at the edges: 4 GiB of bins fit, one bin more does not, with one array and with two; 9.0e18 paths and sample 1.8e19 do not
    assert [int(w[0]) for w in got[:4]] == [1, 0, 1, 0] and bins[0] == (2 ** 29, 1, 1) and bins[4] == (2 ** 28, 1, 2)
    assert [int(w[0]) for w in got[len(bins):]] == [1, 0, 0, 1, 1, 0, 0, 1]


def test_launch_shape_covers_the_total_and_not_a_block_more(exes):
    cases = [(total, 256, block) for total in (1, 63, 64, 65, 2 ** 40) for block in (256, 512)]
    for (total, cus, block), w in zip(cases, ask(exes, [("shape",) + c for c in cases])):
        per_lane, blocks = int(w[0]), int(w[1])
        assert per_lane == max(1, -(-total // (cus * 16 * 64)))
        assert blocks * per_lane * block >= total > (blocks - 1) * per_lane * block, (total, block, w)
    assert ask(exes, [("shape", 2 ** 40, 256, 256)])[0] == [str(2 ** 22), "1024"]   # 16 waves per compute unit: 2^18 lanes


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistics of the batch means
# ---------------------------------------------------------------------------------------------------------------------------------
def series(diffs):
    """(shift, error) of a series given by its differences to the first batch: the header's operations, in its order"""
    nb, s1, s2 = float(len(diffs)), 0.0, 0.0
    for x in diffs:
        s1 += x
        s2 += x * x
    dm = s1 / nb
    return dm, math.sqrt(max(0.0, s2 - nb * dm * dm) / (nb * (nb - 1.0)) if len(diffs) > 1 else 0.0)


def test_batch_statistics(exes):
    rng = np.random.default_rng(7)
    noisy = [float(x) for x in 0.3 + 1e-3 * rng.standard_normal(16)]
    offset = [1e8 + k for k in range(4)]
    f, d = [0.1, 0.3, 0.7, 0.2], [1e16, 1e16 + 2.0, 1e16 + 4.0, 1e16 + 2.0]
    got = ask(exes, [("stats", 0.1), ("stats", 0.1, 0.1, 0.1), ("stats", 1.0 / 3.0) + (1.0 / 3.0,) * 6, ("stats",) + tuple(offset), ("stats",) + tuple(noisy),
                     ("sum",) + tuple(f) + ("|",) + tuple(d)])
    assert [float(x) for x in got[0]] == [0.1, 0.0]                     # one batch
    assert [float(x) for x in got[1]] == [0.1, 0.0] and [float(x) for x in got[2]] == [1.0 / 3.0, 0.0]   # identical batches: the value's own bits
    mean, err = (float(x) for x in got[3])
    want = math.sqrt(np.var(np.arange(4.0), ddof=1) / 4.0)
    assert mean == 1e8 + 1.5 and abs(err - want) <= np.spacing(want), (mean, err, want)
    mean, err = (float(x) for x in got[4])
    dm, e = series([x - noisy[0] for x in noisy])
    assert (mean, err) == (noisy[0] + dm, e)
    assert abs(mean - np.mean(noisy)) < 1e-15 and abs(err - np.std(noisy, ddof=1) / 4.0) < 1e-12
    # the per-batch sum of two series is built from their differences, not from the sums' difference (which rounds f away)
    from_differences = series([(a - f[0]) + (b - d[0]) for a, b in zip(f, d)])[1]
    from_sums = series([(a + b) - (f[0] + d[0]) for a, b in zip(f, d)])[1]
    assert float(got[5][0]) == from_differences != from_sums


# ---------------------------------------------------------------------------------------------------------------------------------
# the one reduction of the bins to means, standard errors and batch means
# ---------------------------------------------------------------------------------------------------------------------------------
def reduce_reference(bins, unit):
    """bins [arrays, numBatches, n, slots] (int64), unit [n] -> (mean [2, slots, n], error [2, slots, n], totalError [slots, n],
    batchMeans [numBatches, arrays, slots, n]): reduce_batches' operations in its order, in double, then float32; -1: not written"""
    arrays, nb, n, slots = bins.shape
    m = bins.astype(np.float64) * np.asarray(unit, np.float64)[None, None, :, None]
    diff = m - m[:, :1]
    both = diff.sum(axis=0) if arrays == 2 else diff[0]     # (f - f0) + (d - d0)
    nbf = float(nb)

    def stats(d):  # d [numBatches, n, slots] -> (shift, error), each [slots, n]
        s1, s2 = np.zeros(d.shape[1:]), np.zeros(d.shape[1:])
        for b in range(nb):
            s1 = s1 + d[b]
            s2 = s2 + d[b] * d[b]
        dm = s1 / nbf
        err = np.sqrt(np.maximum(0.0, s2 - nbf * dm * dm) / (nbf * (nbf - 1.0))) if nb > 1 else np.zeros(dm.shape)
        return dm.T, err.T

    mean, error, total = np.full((2, slots, n), -1.0, np.float32), np.full((2, slots, n), -1.0, np.float32), np.full((slots, n), -1.0, np.float32)
    for a in range(arrays):
        shift, err = stats(diff[a])
        mean[a], error[a] = (m[a, 0].T + shift).astype(np.float32), err.astype(np.float32)
    if arrays == 2:
        total[:] = stats(both)[1].astype(np.float32)
    return mean, error, total, m.transpose(1, 0, 3, 2).astype(np.float32)


def reduced(exes, bins, unit):
    bins = np.asarray(bins, np.int64)
    arrays, nb, n, slots = bins.shape
    words = ask(exes, [("reduce", arrays, nb, n, slots) + tuple(float(x) for x in unit) + tuple(int(x) for x in bins.reshape(-1))])[0]
    got = np.array([np.float32(float(x)) for x in words], np.float32)
    v = slots * n
    assert got.size == 5 * v + bins.size
    got = got[:2 * v].reshape(2, slots, n), got[2 * v:4 * v].reshape(2, slots, n), got[4 * v:5 * v].reshape(slots, n), got[5 * v:].reshape(nb, arrays, slots, n)
    for g, w, what in zip(got, reduce_reference(bins, unit), ("mean", "error", "totalError", "batchMeans")):
        assert g.tobytes() == w.tobytes(), (what, g, w)
    return got


def test_the_reduction_is_the_arithmetic_written_out(exes):
    rng = np.random.default_rng(11)
    unit = 2.0 ** -40 / 197.0
    # one batch: the errors are exactly 0
    mean, error, total, means = reduced(exes, rng.integers(1, 2 ** 50, (1, 1, 3, 1)), [unit] * 3)
    assert np.all(error[0] == 0.0) and np.all(mean[0] > 0) and np.all(mean[1] == -1.0) and np.all(total == -1.0) and means.tobytes() == mean[0].tobytes()
    # the path-length layout, every bin another: [batch][n][slot] -> [slot][n] and [batch][slot][n]
    bins = (1 + np.arange(3 * 2 * 4, dtype=np.int64).reshape(1, 3, 2, 4)) * 2 ** 30
    mean, error, total, means = reduced(exes, bins, [unit, 1.0009765625 * unit])
    assert len(set(bins.reshape(-1))) == 24 and len(set(means.reshape(-1))) == 24
    for b in range(3):
        for i in range(2):
            for s in range(4):
                assert means[b, 0, s, i] == np.float32(float(bins[0, b, i, s]) * (unit, 1.0009765625 * unit)[i])
    assert mean.shape == (2, 4, 2) and np.all(error[0] > 0) and np.all(mean[1] == -1.0)
    # the sensors' three series, a unit per receiver of pi and 4 pi: the total's error is the sum series', not a sum of errors
    bins = rng.integers(2 ** 40, 2 ** 41, (2, 4, 3, 1))
    units = [unit * math.pi, unit * 4.0 * math.pi, unit * math.pi]
    mean, error, total, means = reduced(exes, bins, units)
    for i in range(3):
        f, d = ([float(bins[a, b, i, 0]) * units[i] for b in range(4)] for a in (0, 1))
        assert total[0, i] == np.float32(series([(x - f[0]) + (y - d[0]) for x, y in zip(f, d)])[1])
        assert error[0, 0, i] == np.float32(series([x - f[0] for x in f])[1]) and mean[1, 0, i] == np.float32(d[0] + series([y - d[0] for y in d])[0])
        assert 0 < total[0, i] < error[0, 0, i] + error[1, 0, i]
    assert means.shape == (4, 2, 1, 3) and np.all(means[:, 1, 0] == (bins[1, :, :, 0].astype(np.float64) * np.array(units)).astype(np.float32))
    # identical batches: errors exactly 0, the mean the first batch's value to the bit
    one = rng.integers(1, 2 ** 55, (2, 1, 3, 2))
    mean, error, total, means = reduced(exes, np.repeat(one, 5, axis=1), units)
    assert np.all(error == 0.0) and np.all(total == 0.0)
    assert mean.tobytes() == (one[:, 0].astype(np.float64) * np.array(units)[None, :, None]).transpose(0, 2, 1).astype(np.float32).tobytes()
    # bins near 2^61 (a bin's sum stays below 2^62)
    big = 2 ** 61 - rng.integers(0, 2 ** 20, (2, 3, 2, 2))
    mean, error, total, means = reduced(exes, big, [unit, unit])
    assert np.all(np.abs(mean / np.float32(2.0 ** 61 * unit) - 1.0) < 1e-6) and np.all(np.isfinite(error)) and np.all(np.isfinite(total))


def test_a_question_the_program_cannot_read_is_an_error(exes):
    for e in exes:
        assert subprocess.run([e], input="scale\n", capture_output=True, text=True, timeout=60).returncode == 2
