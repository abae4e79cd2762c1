"""What the radiance by photon path length costs (DESIGN.md sections 4.23 and 5): on the step cloud, a nadir image of the whole
domain from the top (one pixel per column), the plain render (mcbrat_render_camera) against renderCameraPathLengths with 8, 64
and 256 uniform bins, and 256 bins with every deposit forced straight to global memory (option cameraPathBinsInLds = 0: what the
histograms in LDS buy); and the same five for ONE pixel (the column next to the cloud's edge) with 32 times the samples -- as many
paths, every estimate of the launch on one pixel's bins.  After a warm-up of each, `reps` interleaved repetitions -- one of
every variant per round --, the median and all of them.  With --parent-lib, a library built from the parent commit's sources renders the plain image in a process of
its own, one repetition per round between the others: the baseline the plain render of this build is held to.

    python scripts/pathlength_cost.py [--parent-lib ab/libmcbrat_parent.so] [--out profiles/pathlength_cost.json]

Times are a host clock around the synchronous call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402

SPP, BATCHES, L_TOP = 65536, 16, 4.0


def setup():
    try:  # (where PyTorch is installed it comes first: one HIP runtime per process)
        import torch  # noqa: F401
    except Exception:
        pass
    import mcbrat3d_amd as M
    from mcbrat3d_amd.camera import new_Camera
    case = cases.step_cloud(0.99)
    case["albedo"] = 0.2
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, minForwardTableSize=1801)
    integ.prepare(dom, M.new_PhotonStream(0.5, 30.0, numberOfPhotons=10 ** 13))
    xe, ye, ze = case["xe"], case["ye"], case["ze"]
    cam = new_Camera("orthographic", npx=dom.numX, npy=dom.numY, mu=1.0, phi=0.0, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=ze[-1])
    i = dom.numX // 2
    one = new_Camera("orthographic", npx=1, npy=1, mu=1.0, phi=0.0, footprint=(xe[i], xe[i + 1], ye[0], ye[-1]), height=ze[-1])
    return integ, {"image": (cam, SPP), "one pixel": (one, SPP * dom.numX * dom.numY)}, dom.numX * dom.numY * SPP * BATCHES


def plain(integ, view, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    cam, spp = view
    t0 = time.perf_counter()
    out = integ.renderCamera(cam, new_RandomNumberSequence(seed), spp, BATCHES)
    dt = time.perf_counter() - t0
    assert out["dropped"] == 0
    return dt


def by_length(integ, view, bins, seed):
    cam, spp = view
    edges = (L_TOP / bins * np.arange(bins)).astype(np.float32)
    t0 = time.perf_counter()
    out = integ.renderCameraPathLengths(cam, edges, spp, numBatches=BATCHES, seed=seed)
    dt = time.perf_counter() - t0
    assert out["dropped"] == 0
    return dt


def child():
    """the plain render with whatever library MCBRAT_LIB names: a warm-up, then one repetition per line of standard input"""
    integ, views, _ = setup()
    plain(integ, views["image"], 1)
    print("ready", flush=True)
    for line in sys.stdin:
        print(repr(plain(integ, views["image"], int(line))), flush=True)
    integ.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    parent = None
    if a.parent_lib:
        env = dict(os.environ, MCBRAT_LIB=os.path.abspath(a.parent_lib), MCBRAT_LIB_OLD="1")
        parent = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = parent.stdout.readline()
        while line and line.strip() != "ready":  # (whatever a runtime prints while it loads)
            line = parent.stdout.readline()
        assert line, "the parent library's process ended before it was ready"
    integ, views, paths = setup()

    def direct(view, s):
        integ.setOption(cameraPathBinsInLds=0)
        try:
            return by_length(integ, view, 256, s)
        finally:
            integ.setOption(cameraPathBinsInLds=1)

    variants = {}
    for name, view in views.items():
        tag = "" if name == "image" else name + ": "
        variants[tag + "plain"] = lambda s, v=view: plain(integ, v, s)
        for bins in (8, 64, 256):
            variants[tag + "%d bins" % bins] = lambda s, v=view, b=bins: by_length(integ, v, b, s)
        variants[tag + "256 bins, deposits straight to global memory"] = lambda s, v=view: direct(v, s)
    times = {k: [] for k in variants}
    if parent:
        times["plain, parent commit"] = []
    for f in variants.values():
        f(1)  # warm-up
    for r in range(a.reps):
        for k, f in variants.items():
            times[k].append(f(100 + r))
        if parent:
            parent.stdin.write("%d\n" % (100 + r))
            parent.stdin.flush()
            times["plain, parent commit"].append(float(parent.stdout.readline()))
    if parent:
        parent.stdin.close()
        assert parent.wait(timeout=60) == 0
    integ.finalize()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = dict(workload="step cloud, nadir image 32 x 1 from the top", samplesPerPixel=SPP, batches=BATCHES, paths=paths, reps=a.reps,
               seconds_median=med, paths_per_s={k: paths / v for k, v in med.items()},
               ratio_to_plain={k: v / med["one pixel: plain" if k.startswith("one pixel") else "plain"] for k, v in med.items()}, seconds_all=times)
    if parent:
        res["plain_to_parent_plain"] = med["plain"] / med["plain, parent commit"]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
