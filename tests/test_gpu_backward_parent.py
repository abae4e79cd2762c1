"""The backward camera and the backward sensors give what they gave before their host code was put on one path (DESIGN.md section
4.21), bit for bit and word for word: tests/golden/backward_parent.json holds, from the library of the commit before,

  * the step cloud (ssa 0.99, albedo 0.2, mu0 0.5, azimuth 30) through the 5 x 3 pinhole inside the cloud -- radiance, its standard
    error, the batch means, the drop count -- and at three sensors in one call -- a tilted planar point (35, 200), a planar area
    receiver across the cloud's step, a spherical point inside the cloud: the five result arrays, the batch means, the drop count --,
    197 samples (no multiple of 64) in 3 batches, the grid in global memory and in LDS, as the bytes of the arrays;
  * the full text of every refusal that test_refusals_leave_the_context_untouched of tests/test_gpu_camera.py and of
    tests/test_gpu_sensors.py provokes;
  * the order of the refusals: for each entry one call per adjacent pair of its order with BOTH rules violated at once.

This same file recorded it, on an MI355X (`dropped` is 0 in the recording: the first seed from SEED on that gives 0 is recorded):

    MCBRAT_LIB=<that library> python tests/test_gpu_backward_parent.py --record tests/golden/backward_parent.json

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
GOLDEN = os.path.join(ROOT, "tests", "golden", "backward_parent.json")
SEED, SAMPLES, BATCHES = 20261022, 197, 3
CAMERA_KEYS = ("radiance", "radiance_StdErr", "batchMeans")
SENSOR_KEYS = ("diffuse", "direct", "diffuse_StdErr", "direct_StdErr", "irradiance_StdErr", "batchMeans")


# ---------------------------------------------------------------------------------------------------------------------------------
# the renders
# ---------------------------------------------------------------------------------------------------------------------------------
def scene():
    """-> (the integrator, its domain, the three sensors, camera(gridInLds): the 5 x 3 pinhole)"""
    from mcbrat3d_amd.sensors import new_Sensors
    from tests import cases
    from tests.test_gpu_camera import _integrator, _pinhole
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.2
    integ, dom = _integrator(case, 0.5, 30.0)
    point = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    sensors = new_Sensors([(0.13, 0.2, 0.05), (0.2, 0.1, 0.0), (0.35, 0.3, 0.12)], tilt=[35.0, 0.0, 0.0], azimuth=[200.0, 0.0, 0.0],
                          kind=["planar", "planar", "spherical"], extents=[point, ((0.1, 0.0, 0.0), (0.0, 0.2, 0.0)), point])
    return integ, dom, sensors, lambda lds: _pinhole(5, 3, (0.13, 0.2, 0.05), (0.4, 0.1, 1.0), fov=80.0, gridInLds=lds)


def packed(res, keys):
    return dict({k: np.ascontiguousarray(res[k]).tobytes().hex() for k in keys}, dropped=res["dropped"])


def renders(seed):
    """-> {"camera 0": {array: hex of its bytes, "dropped": count}, "camera 1", "sensors 0", "sensors 1"} (0 | 1: gridInLds)"""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ, _, sensors, camera = scene()
    out = {}
    for lds in (0, 1):
        out["camera %d" % lds] = packed(integ.renderCamera(camera(lds), new_RandomNumberSequence(seed), SAMPLES, BATCHES), CAMERA_KEYS)
        out["sensors %d" % lds] = packed(integ.renderSensors(sensors, new_RandomNumberSequence(seed), SAMPLES, BATCHES, gridInLds=lds), SENSOR_KEYS)
    integ.finalize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _bare(L, ptr, step, big=False, rpv=False):
    """a context with nothing (step 0); the grid (1); optics and the solar source, no table (2); the forward table alone (3); the
    inverse table too (4).  big: 128 x 128 x 64 cells, which no LDS share holds, instead of 2 x 2 x 2; rpv: a BRDF surface"""
    ctx = L.mcbrat_create(0)
    assert ctx
    nx, nz = (128, 64) if big else (2, 2)
    e, ez, one = np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 1.0, nz + 1), np.ones(nx * nx * nz)
    if step >= 1:
        assert L.mcbrat_set_grid(ctx, nx, nx, nz, ptr(e), ptr(e), ptr(ez)) == 0
    if step >= 2:
        assert L.mcbrat_set_optics(ctx, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(one.size, np.int32)), 0.2) == 0
        assert L.mcbrat_set_source_solar(ctx, C.c_float(0.5), C.c_float(0.0)) == 0
    if step >= 3:
        assert L.mcbrat_set_forward_table(ctx, 1, 181, 1, ptr(np.ones(181, np.float32)), None) == 0
    if step >= 4:
        inv, coef = np.zeros(101, np.float32), np.zeros(2, np.float32)
        assert L.mcbrat_inverse_table_legendre(len(coef), ptr(coef), len(inv), ptr(inv)) == 0
        assert L.mcbrat_set_inverse_table(ctx, 1, len(inv), 1, ptr(inv)) == 0
    if rpv:
        assert L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(np.array([0.0, 1.0])), ptr(np.array([0.0, 1.0])), 4, ptr(np.array([0.1, 0.8, -0.1, 0.5], np.float32))) == 0
    return ctx


class _Contexts:
    """the contexts the refusals are provoked on, by name; made when first asked for, destroyed by close()"""
    def __init__(self):
        from tests.test_gpu_refusal_matrix import Context, _lib
        self.Context, self.made = Context, {}
        self.L, self.ptr = _lib()

    def __call__(self, name):
        if name not in self.made:
            if name in ("full", "thermal", "random azimuth", "rpv", "thermal rpv"):
                c = self.Context(thermal=name.startswith("thermal"))
                if name == "random azimuth":
                    c.ok(c.L.mcbrat_set_source_random_azimuth(c.ctx, C.c_float(0.5)))
                if name.endswith("rpv"):
                    c.ok(c.setters["rpv"]())
                self.made[name] = c.ctx
            else:  # "bare 0" .. "bare 4", "big bare 3", "bare 1 rpv"
                step = name.replace(" rpv", "")
                self.made[name] = _bare(self.L, self.ptr, int(step[-1]), big=name.startswith("big"), rpv=step != name)
        return self.made[name]

    def close(self):
        for ctx in self.made.values():
            self.L.mcbrat_destroy(ctx)


def _camera_text(cx, where, cam, spp=64, batches=1, first=0, radiance=True):
    ctx = cx(where)
    rad = np.zeros(4, np.float32)
    rc = cx.L.mcbrat_render_camera(ctx, None if cam is None else C.addressof(cam), SEED, first, spp, batches, cx.ptr(rad) if radiance else None, None, None, None)
    assert rc != 0, "a call that should have been refused was not"
    return cx.L.mcbrat_last_error(ctx).decode()


def _sensors_text(cx, where, sensors, n=None, samples=64, batches=1, first=0, lds=-1, arrays=True):
    from mcbrat3d_amd._capi import Sensor
    ctx = cx(where)
    arr = (Sensor * len(sensors))(*sensors)
    dif, dirc = np.zeros(len(sensors), np.float32), np.zeros(len(sensors), np.float32)
    rc = cx.L.mcbrat_render_sensors(ctx, len(sensors) if n is None else n, C.addressof(arr), SEED, first, samples, batches, lds,
                                    cx.ptr(dif) if arrays else None, cx.ptr(dirc), None, None, None, None, None)
    assert rc != 0, "a call that should have been refused was not"
    return cx.L.mcbrat_last_error(ctx).decode()


def _key(kw):
    return repr(kw)[1:-1].replace("'", "")


def refusals():
    """-> {"camera": {case: text}, "sensors": ..., "camera order": ..., "sensors order": ...}"""
    from tests.test_gpu_camera import REFUSED_CAMERAS, _struct as cam
    from tests.test_gpu_sensors import REFUSED_SENSORS, _struct as sen
    cx = _Contexts()
    out = {"camera": {}, "sensors": {}, "camera order": {}, "sensors order": {}}
    # every single refusal of the two tests
    r = out["camera"]
    for kw, _ in REFUSED_CAMERAS:
        r[_key(kw)] = _camera_text(cx, "full", cam(**kw))
    r["spp = 0"] = _camera_text(cx, "full", cam(), spp=0)
    r["budget"] = _camera_text(cx, "full", cam(npx=32768, npy=32768), batches=2)
    for where in ("thermal", "random azimuth", "rpv", "bare 0", "bare 1", "bare 2", "bare 3"):
        r[where] = _camera_text(cx, where, cam())
    r = out["sensors"]
    for kw, _ in REFUSED_SENSORS:
        r[_key(kw)] = _sensors_text(cx, "full", [sen(**kw)])
        assert _sensors_text(cx, "full", [sen(), sen(**kw)]) == r[_key(kw)]   # behind a good one: the same words
    for kw in (dict(n=0), dict(n=-3), dict(samples=0), dict(batches=0), dict(lds=2), dict(n=2 ** 28, batches=2)):
        r[_key(kw)] = _sensors_text(cx, "full", [sen()], **kw)
    for where in ("thermal", "random azimuth", "rpv", "bare 0", "bare 1", "bare 2", "bare 3"):
        r[where] = _sensors_text(cx, where, [sen()])
    # the order: both rules of each adjacent pair violated in one call
    late, far = 18 * 10 ** 18, 2 ** 62   # a first sample and a sample count past what a 64-bit index counts
    r = out["camera order"]
    r["no array, bad camera"] = _camera_text(cx, "full", cam(kind=2), radiance=False)
    r["bad camera, samples"] = _camera_text(cx, "full", cam(kind=2), spp=0)
    r["samples, batches"] = _camera_text(cx, "full", cam(), spp=0, batches=0)
    r["batches, budget"] = _camera_text(cx, "full", cam(npx=65536, npy=65536), batches=0)
    r["budget, index count"] = _camera_text(cx, "full", cam(npx=32768, npy=32768), spp=far, batches=2)
    r["index count, context"] = _camera_text(cx, "bare 0", cam(), first=late)
    r["grid and optics, source"] = _camera_text(cx, "bare 1", cam())
    r["source, BRDF surface"] = _camera_text(cx, "thermal rpv", cam())
    r["BRDF surface, height"] = _camera_text(cx, "rpv", cam(z=1.5))
    r["height, forward tables"] = _camera_text(cx, "bare 2", cam(z=1.5))
    r["forward tables, inverse tables"] = _camera_text(cx, "bare 2", cam())
    r["inverse tables, LDS share"] = _camera_text(cx, "big bare 3", cam(gridInLds=1))
    r = out["sensors order"]
    r["n < 1, null arrays"] = _sensors_text(cx, "full", [sen()], n=0, arrays=False)
    r["null arrays, gridInLds"] = _sensors_text(cx, "full", [sen()], lds=2, arrays=False)
    r["gridInLds, samples"] = _sensors_text(cx, "full", [sen()], lds=2, samples=0)
    r["samples, batches"] = _sensors_text(cx, "full", [sen()], samples=0, batches=0)
    r["batches, budget"] = _sensors_text(cx, "full", [sen()], n=2 ** 31, batches=0)
    r["budget, index count"] = _sensors_text(cx, "full", [sen()], n=2 ** 28, batches=2, samples=far)
    r["index count, bad sensor"] = _sensors_text(cx, "full", [sen(kind=2)], first=late)
    r["bad sensor, context"] = _sensors_text(cx, "bare 0", [sen(kind=2)])
    r["grid and optics, source"] = _sensors_text(cx, "bare 1", [sen()])
    r["source, BRDF surface"] = _sensors_text(cx, "thermal rpv", [sen()])
    r["BRDF surface, corners"] = _sensors_text(cx, "rpv", [sen(position=(0.5, 0.5, 1.01))])
    r["corners, forward tables"] = _sensors_text(cx, "bare 2", [sen(position=(0.5, 0.5, 1.01))])
    r["forward tables, inverse tables"] = _sensors_text(cx, "bare 2", [sen()])
    r["inverse tables, LDS share"] = _sensors_text(cx, "big bare 3", [sen()], lds=1)
    cx.close()
    return out


WORDS = {"no array": "no camera or no array", "bad camera": "camera kind", "samples": "samplesPer", "batches": "numBatches", "budget": "tally budget",
         "index count": "64-bit index", "grid and optics": "not completely specified", "source": "Directional solar source",
         "BRDF surface": "BRDF surface", "height": "height", "forward tables": "forward phase function table",
         "inverse tables": "inverse phase function table", "n < 1": "n < 1", "null arrays": "no sensors or no arrays", "gridInLds": "gridInLds must be",
         "bad sensor": "sensor kind", "corners": "corner"}
ENTRIES = (("camera order", "renderCamera:"), ("sensors order", "renderSensors:"))


def _first_of_each_pair_refuses(rec, entries=ENTRIES, words=WORDS, raw=()):
    """what needs no golden file: in every pair the EARLIER rule of the order is the one that speaks.  raw: (entry, rule)s whose
    text is the receiver's own, under the solar entry's name"""
    for entry, prefix in entries:
        for pair, text in rec[entry].items():
            first, second = pair.split(", ")
            assert words[first] in text, (entry, pair, text)
            if (entry, first) in raw:
                assert text.startswith(dict(ENTRIES)[entry.split()[-2] + " order"]), (entry, pair, text)
            else:
                assert text.startswith(prefix) or first == "inverse tables", (entry, pair, text)   # (those: the context's own text)
            assert second == "context" or second == "LDS share" or words[second] not in text, (entry, pair, text)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
def test_the_renders_are_the_parent_commit_s_byte_for_byte(golden):
    got = renders(golden["seed"])
    assert sorted(got) == sorted(golden["renders"]) == ["camera 0", "camera 1", "sensors 0", "sensors 1"]
    for name, want in golden["renders"].items():
        assert want["dropped"] == 0 and sorted(want) == sorted(got[name])
        for key, value in want.items():
            assert got[name][key] == value, (name, key)
    # (what the recording itself shows: the grid in LDS or in global memory, the same bytes)
    assert golden["renders"]["camera 0"] == golden["renders"]["camera 1"] and golden["renders"]["sensors 0"] == golden["renders"]["sensors 1"]
    assert len(golden["renders"]["sensors 0"]["batchMeans"]) == 2 * 4 * BATCHES * 2 * 3 and len(golden["renders"]["camera 0"]["radiance"]) == 2 * 4 * 15


@pytest.mark.gpu
def test_the_refusals_are_the_parent_commit_s_word_for_word_and_in_its_order(golden):
    got = refusals()
    _first_of_each_pair_refuses(got)
    want = {part: {case: golden["texts"][i] for case, i in cases.items()} for part, cases in golden["refusals"].items()}
    assert sorted(got) == sorted(want)
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), part
        for case, text in want[part].items():
            assert got[part][case] == text, (part, case, got[part][case], text)
    assert len(want["camera order"]) == 12 and len(want["sensors order"]) == 14


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record"
    for seed in range(SEED, SEED + 50):
        rendered = renders(seed)
        if all(r["dropped"] == 0 for r in rendered.values()):
            break
    else:
        raise SystemExit("no seed without a dropped path")
    refused = refusals()
    _first_of_each_pair_refuses(refused)
    texts = sorted({t for part in refused.values() for t in part.values()})
    packed = {"seed": seed, "renders": rendered, "texts": texts, "refusals": {part: {case: texts.index(t) for case, t in cases.items()} for part, cases in refused.items()}}
    with open(sys.argv[2], "w") as out:
        json.dump(packed, out, indent=0, sort_keys=True)
        out.write("\n")
    print("seed %d, %d refusals, %d texts" % (seed, sum(len(p) for p in refused.values()), len(texts)))
