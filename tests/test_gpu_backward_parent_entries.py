"""The emission camera, the emission sensors and the camera by path length give what they gave before the five backward entries were
put on one camera front, one sensor front and one batch reduction, bit for bit and word for word:
tests/golden/backward_parent_entries.json holds, from the library of the commit before, in the manner of
tests/test_gpu_backward_parent.py and on its scene (the step cloud, the 5 x 3 pinhole, the three sensors, 197 samples, 3 batches),

  * renderCameraEmission and renderSensorsEmission with sources that differ from cell to cell, and renderCameraPathLengths with
    four edges (three bins or more are lit), the grid in global memory and in LDS, the path-length sums in LDS and straight in
    global memory (option cameraPathBinsInLds), as the bytes of the arrays;
  * the full text of every refusal that test_refusals of tests/test_gpu_emission.py and
    test_refusals_in_order_leave_the_context_untouched of tests/test_gpu_camera_pathlengths.py provoke;
  * the order of the refusals: for each entry one call per adjacent pair of its order with BOTH rules violated at once.

This same file recorded it, on an MI355X (the first seed from SEED on with which the emission entries drop no path is recorded):

    MCBRAT_LIB=<that library> python tests/test_gpu_backward_parent_entries.py --record tests/golden/backward_parent_entries.json

A refused call launches nothing."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_gpu_backward_parent import BATCHES, CAMERA_KEYS, SAMPLES, SEED, WORDS, _Contexts, _first_of_each_pair_refuses, _key, packed, scene  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "backward_parent_entries.json")
SENSOR_KEYS = ("irradiance", "irradiance_StdErr", "batchMeans")
EDGE_CANDIDATES = ([0.0, 0.5, 1.0, 1.5], [0.0, 0.3, 0.7, 1.5], [0.0, 0.2, 0.4, 0.8])
ENTRIES = (("emission camera order", "renderCameraEmission:"), ("emission sensors order", "renderSensorsEmission:"),
           ("pathlengths order", "renderCameraPathLengths:"))
NEW_WORDS = dict(WORDS, **{"null sources": "null", "null array": "no sensors or no array for the irradiance", "null arguments": "no camera, no array",
                           "edges": "pathEdges", "source values": "negative or not finite", "nothing emits": "nothing emits",
                           "LDS share": "edges do not fit the LDS share", "histograms": "histograms"})
RAW = (("emission camera order", "bad camera"), ("emission sensors order", "bad sensor"))   # (the path-length entry words them under its own name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the renders
# ---------------------------------------------------------------------------------------------------------------------------------
def renders(seed, edges):
    """-> {"emission camera 0" | 1, "emission sensors 0" | 1 (gridInLds), "pathlengths 0 0" .. "1 1" (gridInLds, cameraPathBinsInLds)}"""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ, dom, sensors, camera = scene()
    ncol, nvox = dom.numX * dom.numY, dom.numX * dom.numY * dom.numZ
    cell = (1.0 + 0.25 * (np.arange(nvox) % 13)).astype(np.float32).reshape(dom.numZ, dom.numY, dom.numX)
    sfc = (2.0 + 0.5 * (np.arange(ncol) % 7)).astype(np.float32).reshape(dom.numY, dom.numX)
    out = {}
    for lds in (0, 1):
        out["emission camera %d" % lds] = packed(integ.renderCameraEmission(camera(lds), new_RandomNumberSequence(seed), SAMPLES, BATCHES, cellSource=cell,
                                                                            surfaceSource=sfc), CAMERA_KEYS)
        out["emission sensors %d" % lds] = packed(integ.renderSensorsEmission(sensors, new_RandomNumberSequence(seed), SAMPLES, BATCHES, cellSource=cell,
                                                                              surfaceSource=sfc, gridInLds=lds), SENSOR_KEYS)
        for bins_in_lds in (0, 1):
            integ.setOption(cameraPathBinsInLds=bins_in_lds)
            out["pathlengths %d %d" % (lds, bins_in_lds)] = packed(integ.renderCameraPathLengths(camera(lds), edges, SAMPLES, BATCHES, seed=seed), CAMERA_KEYS)
    integ.finalize()
    return out


def lit_bins(rendered, edges):
    rad = np.frombuffer(bytes.fromhex(rendered["pathlengths 0 0"]["radiance"]), np.float32).reshape(len(edges), -1)
    return int((rad > 0).any(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _on(cx, where):
    """the context `where` as the callers of the two test files take one"""
    return type("Ctx", (), dict(L=cx.L, ptr=staticmethod(cx.ptr), ctx=cx(where)))


def _text(result):
    assert result[0] != 0, "a call that should have been refused was not"
    return result[1]


def _pathlengths_null(c, cam=True, rad=True, edges=True):
    """mcbrat_render_camera_pathlengths with null arguments and a faulty camera behind them"""
    from tests.test_gpu_camera import _struct
    s, out, e = _struct(kind=2), np.zeros(12, np.float32), np.array([0.0, 0.5, 2.0], np.float32)
    rc = c.L.mcbrat_render_camera_pathlengths(c.ctx, C.addressof(s) if cam else None, 3, c.ptr(e) if edges else None, SEED, 0, 64, 1,
                                              c.ptr(out) if rad else None, None, None, None)
    return rc, c.L.mcbrat_last_error(c.ctx).decode()


def refusals():
    """-> {"emission camera": {case: text}, "emission sensors", "pathlengths", and each with " order"}"""
    from tests.test_gpu_camera import REFUSED_CAMERAS, _struct as cam
    from tests.test_gpu_camera_pathlengths import EDGES, _call as by_length
    from tests.test_gpu_emission import CELL8, SFC4, _call_camera, _call_sensors, _sensor_structs as sen
    cx = _Contexts()
    full = _on(cx, "full")
    out = {part + order: {} for part in ("emission camera", "emission sensors", "pathlengths") for order in ("", " order")}
    bad, nan, dark = CELL8.copy(), SFC4.copy(), dict(cell=np.zeros(8, np.float32), sfc=np.zeros(4, np.float32))
    bad[3], nan[2] = -1.0, np.nan
    dim = dict(cell=np.where(np.arange(8) == 3, -1.0, 0.0).astype(np.float32), sfc=dark["sfc"])   # a negative value, and nothing that emits
    sources = {"no cellSource": dict(cell=None), "no surfaceSource": dict(sfc=None), "a negative cellSource": dict(cell=bad), "a NaN surfaceSource": dict(sfc=nan),
               "nothing emits": dark}
    big = dict(cell=np.ones(128 * 128 * 64, np.float32), sfc=np.ones(128 * 128, np.float32))
    # every single refusal of tests/test_gpu_emission.py::test_refusals
    r = out["emission camera"]
    for kw, _ in REFUSED_CAMERAS:
        r[_key(kw)] = _text(_call_camera(full, cam(**kw)))
    for kw in (dict(spp=0), dict(batches=0)):
        r[_key(kw)] = _text(_call_camera(full, cam(), **kw))
    for case, kw in sources.items():
        r[case] = _text(_call_camera(full, cam(), **kw))
    r["budget"] = _text(_call_camera(full, cam(npx=32768, npy=32768), batches=2, n=1))
    for where in ("rpv", "bare 0", "bare 1", "bare 2"):
        r[where] = _text(_call_camera(_on(cx, where), cam()))
    r["LDS share"] = _text(_call_camera(_on(cx, "big bare 4"), cam(gridInLds=1), **big))
    r = out["emission sensors"]
    for kw in (dict(n=0), dict(samples=0), dict(batches=0), dict(lds=2), dict(n=2 ** 30, batches=2)):
        r[_key(kw)] = _text(_call_sensors(full, sen(1), **kw))
    for case, kw in sources.items():
        r[case] = _text(_call_sensors(full, sen(1), **kw))
    for kw in (dict(kind=2), dict(normal=(0.0, 0.0, 0.0)), dict(position=(0.5, np.nan, 0.5)), dict(position=(0.5, 0.5, 1.5))):
        r[_key(kw)] = _text(_call_sensors(full, sen(1, **kw)))
    for where in ("rpv", "bare 0", "bare 1", "bare 2"):
        r[where] = _text(_call_sensors(_on(cx, where), sen(1)))
    r["LDS share"] = _text(_call_sensors(_on(cx, "big bare 4"), sen(1), lds=1, **big))
    # ... and of tests/test_gpu_camera_pathlengths.py::test_refusals_in_order_leave_the_context_untouched
    r = out["pathlengths"]
    bad_cam, tall, wide = cam(mu=0.0), cam(z=1.5), cam(z=1.5, npx=4096, npy=4096)
    for kw in (dict(cam=None, edges=None, nbins=0, spp=0, batches=0), dict(cam=bad_cam, rad=False, nbins=0, spp=0), dict(cam=bad_cam, edges=None, nbins=3),
               dict(cam=bad_cam, nbins=0, spp=0), dict(cam=tall, nbins=0, edges=[1.0, 0.5], spp=0), dict(cam=tall, nbins=257, edges=np.arange(257.0), spp=0),
               dict(cam=tall, edges=[0.0, np.inf, 1.0], spp=0), dict(cam=tall, edges=[0.0, np.nan], spp=0), dict(cam=tall, edges=[0.5, 1.0], spp=0),
               dict(cam=tall, edges=[0.0, 1.0, 1.0], spp=0), dict(cam=tall, edges=[0.0, 2.0, 1.0], spp=0), dict(cam=tall, spp=0, batches=0),
               dict(cam=wide, batches=0, n=1, edges=EDGES[256]), dict(cam=wide, n=1, edges=EDGES[256]),
               dict(cam=cam(z=1.5, npx=32768, npy=32768), n=1, edges=[0.0], batches=2), dict(cam=tall), dict(cam=cam(), spp=0)):
        args = dict(kw)
        r[str(len(r))] = _text(by_length(full, args.pop("cam"), **args))
    for kw, _ in REFUSED_CAMERAS:
        r[_key(kw)] = _text(by_length(full, cam(**kw)))
    for where in ("thermal", "random azimuth", "rpv", "bare 0", "bare 1", "bare 2", "bare 3"):
        r[where] = _text(by_length(_on(cx, where), cam()))
    # the order: both rules of each adjacent pair violated in one call
    late, far = 18 * 10 ** 18, 2 ** 62   # a first sample and a sample count past what a 64-bit index counts
    r = out["emission camera order"]
    rad = np.zeros(4, np.float32)
    kind2 = cam(kind=2)
    assert full.L.mcbrat_render_camera_emission(full.ctx, C.addressof(kind2), None, None, SEED, 0, 64, 1, None, None, None, None) != 0
    r["no array, null sources"] = full.L.mcbrat_last_error(full.ctx).decode()
    r["null sources, bad camera"] = _text(_call_camera(full, cam(kind=2), cell=None))
    r["bad camera, samples"] = _text(_call_camera(full, cam(kind=2), spp=0))
    r["samples, batches"] = _text(_call_camera(full, cam(), spp=0, batches=0))
    r["batches, budget"] = _text(_call_camera(full, cam(npx=65536, npy=65536), batches=0))
    r["budget, index count"] = _text(_call_camera(full, cam(npx=32768, npy=32768), spp=far, batches=2))
    good = cam()
    assert full.L.mcbrat_render_camera_emission(cx("bare 0"), C.addressof(good), cx.ptr(CELL8), cx.ptr(SFC4), SEED, late, 64, 1, cx.ptr(rad), None, None, None) != 0
    r["index count, grid and optics"] = cx.L.mcbrat_last_error(cx("bare 0")).decode()
    r["grid and optics, BRDF surface"] = _text(_call_camera(_on(cx, "bare 1 rpv"), cam()))
    r["BRDF surface, height"] = _text(_call_camera(_on(cx, "rpv"), cam(z=1.5)))
    r["height, source values"] = _text(_call_camera(full, cam(z=1.5), cell=bad))
    r["source values, nothing emits"] = _text(_call_camera(full, cam(), **dim))
    r["nothing emits, inverse tables"] = _text(_call_camera(_on(cx, "bare 2"), cam(), **dark))
    r["inverse tables, LDS share"] = _text(_call_camera(_on(cx, "big bare 3"), cam(gridInLds=1), **big))
    r = out["emission sensors order"]
    one = sen(1)
    assert full.L.mcbrat_render_sensors_emission(full.ctx, 0, C.addressof(one), None, None, SEED, 0, 64, 1, -1, None, None, None, None) != 0
    r["n < 1, null array"] = full.L.mcbrat_last_error(full.ctx).decode()
    assert full.L.mcbrat_render_sensors_emission(full.ctx, 1, C.addressof(one), None, None, SEED, 0, 64, 1, -1, None, None, None, None) != 0
    r["null array, null sources"] = full.L.mcbrat_last_error(full.ctx).decode()
    r["null sources, gridInLds"] = _text(_call_sensors(full, sen(1), cell=None, lds=2))
    r["gridInLds, samples"] = _text(_call_sensors(full, sen(1), lds=2, samples=0))
    r["samples, batches"] = _text(_call_sensors(full, sen(1), samples=0, batches=0))
    r["batches, budget"] = _text(_call_sensors(full, sen(1), n=2 ** 31, batches=0))
    r["budget, index count"] = _text(_call_sensors(full, sen(1), n=2 ** 30, batches=2, samples=far))
    bad_sensor = sen(1, kind=2)
    irr = np.zeros(1, np.float32)
    assert full.L.mcbrat_render_sensors_emission(full.ctx, 1, C.addressof(bad_sensor), cx.ptr(CELL8), cx.ptr(SFC4), SEED, late, 64, 1, -1, cx.ptr(irr), None, None, None) != 0
    r["index count, bad sensor"] = full.L.mcbrat_last_error(full.ctx).decode()
    r["bad sensor, grid and optics"] = _text(_call_sensors(_on(cx, "bare 0"), sen(1, kind=2)))
    r["grid and optics, BRDF surface"] = _text(_call_sensors(_on(cx, "bare 1 rpv"), sen(1)))
    r["BRDF surface, corners"] = _text(_call_sensors(_on(cx, "rpv"), sen(1, position=(0.5, 0.5, 1.01))))
    r["corners, source values"] = _text(_call_sensors(full, sen(1, position=(0.5, 0.5, 1.01)), cell=bad))
    r["source values, nothing emits"] = _text(_call_sensors(full, sen(1), **dim))
    r["nothing emits, inverse tables"] = _text(_call_sensors(_on(cx, "bare 2"), sen(1), **dark))
    r["inverse tables, LDS share"] = _text(_call_sensors(_on(cx, "big bare 3"), sen(1), lds=1, **big))
    r = out["pathlengths order"]
    r["null arguments, bad camera"] = _text(_pathlengths_null(full, rad=False))
    r["bad camera, edges"] = _text(by_length(full, cam(kind=2), edges=[0.5, 1.0]))
    r["edges, samples"] = _text(by_length(full, cam(), edges=[0.5, 1.0], spp=0))
    r["samples, batches"] = _text(by_length(full, cam(), spp=0, batches=0))
    r["batches, budget"] = _text(by_length(full, cam(npx=4096, npy=4096), batches=0, n=1, edges=EDGES[256]))
    r["budget, index count"] = _text(by_length(full, cam(npx=4096, npy=4096), spp=far, n=1, edges=EDGES[256]))
    bare0, plain = _on(cx, "bare 0"), cam()
    assert cx.L.mcbrat_render_camera_pathlengths(bare0.ctx, C.addressof(plain), 3, cx.ptr(np.array([0.0, 0.5, 2.0], np.float32)), SEED, late, 64, 1,
                                                 cx.ptr(np.zeros(12, np.float32)), None, None, None) != 0
    r["index count, grid and optics"] = cx.L.mcbrat_last_error(bare0.ctx).decode()
    r["grid and optics, source"] = _text(by_length(_on(cx, "bare 1"), cam()))
    r["source, BRDF surface"] = _text(by_length(_on(cx, "thermal rpv"), cam()))
    r["BRDF surface, height"] = _text(by_length(_on(cx, "rpv"), cam(z=1.5)))
    r["height, forward tables"] = _text(by_length(_on(cx, "bare 2"), cam(z=1.5)))
    r["forward tables, inverse tables"] = _text(by_length(_on(cx, "bare 2"), cam()))
    r["inverse tables, LDS share"] = _text(by_length(_on(cx, "big bare 3"), cam(gridInLds=1)))
    r["LDS share, histograms"] = _text(by_length(_on(cx, "big bare 4"), cam(gridInLds=1), edges=EDGES[256]))
    cx.close()
    return out


def _checked(refused):
    words = dict(NEW_WORDS, **{"no array": "no camera or no array for the radiance"})
    _first_of_each_pair_refuses(refused, ENTRIES, words, RAW)
    assert [len(refused[entry]) for entry, _ in ENTRIES] == [13, 15, 14]
    for entry, prefix in ENTRIES:   # the refusals of the tests: under the entry's name, but for the receiver's and the context's own
        for case, text in refused[entry[:-6]].items():
            assert text.startswith((prefix, "renderCamera:", "renderSensors:")) or "inverse phase function table" in text, (entry, case, text)
    assert not any("renderCamera:" in t for t in refused["pathlengths"].values())
    return refused


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
def test_the_renders_are_the_parent_commit_s_byte_for_byte(golden):
    edges = golden["pathEdges"]
    got = renders(golden["seed"], edges)
    assert sorted(got) == sorted(golden["renders"]) and len(got) == 8
    for name, want in golden["renders"].items():
        assert (want["dropped"] == 0 or name.startswith("pathlengths")) and sorted(want) == sorted(got[name])
        for key, value in want.items():
            assert got[name][key] == value, (name, key)
    # (what the recording itself shows: wherever the grid and the path-length sums lie, the same bytes)
    rec = golden["renders"]
    assert rec["emission camera 0"] == rec["emission camera 1"] and rec["emission sensors 0"] == rec["emission sensors 1"]
    assert rec["pathlengths 0 0"] == rec["pathlengths 0 1"] == rec["pathlengths 1 0"] == rec["pathlengths 1 1"]
    assert len(edges) == 4 and lit_bins(rec, edges) >= 3
    assert len(rec["pathlengths 0 0"]["batchMeans"]) == 2 * 4 * BATCHES * 4 * 15 and len(rec["emission sensors 0"]["batchMeans"]) == 2 * 4 * BATCHES * 3


@pytest.mark.gpu
def test_the_refusals_are_the_parent_commit_s_word_for_word_and_in_its_order(golden):
    got = _checked(refusals())
    want = {part: {case: golden["texts"][i] for case, i in cases.items()} for part, cases in golden["refusals"].items()}
    assert sorted(got) == sorted(want)
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), part
        for case, text in want[part].items():
            assert got[part][case] == text, (part, case, got[part][case], text)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record"
    for seed, edges in ((s, e) for s in range(SEED, SEED + 50) for e in EDGE_CANDIDATES):
        rendered = renders(seed, edges)
        if all(r["dropped"] == 0 for name, r in rendered.items() if name.startswith("emission")) and lit_bins(rendered, edges) >= 3:
            break
    else:
        raise SystemExit("no seed without a dropped path and with three lit bins")
    refused = _checked(refusals())
    texts = sorted({t for part in refused.values() for t in part.values()})
    record = {"seed": seed, "pathEdges": edges, "renders": rendered, "texts": texts,
              "refusals": {part: {case: texts.index(t) for case, t in cases.items()} for part, cases in refused.items()}}
    with open(sys.argv[2], "w") as out:
        json.dump(record, out, indent=0, sort_keys=True)
        out.write("\n")
    print("seed %d, edges %s, %d refusals, %d texts" % (seed, edges, sum(len(p) for p in refused.values()), len(texts)))
