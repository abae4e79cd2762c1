"""What the expected-value estimator of the emission renders costs and buys (DESIGN.md sections 4.24 and 5).  Three workloads, each
rendered by both estimators at equal samples:

  step cloud      the thermal set-up of scripts/emission_cost.py, a nadir image 32 x 1 from the top (the grid in LDS)
  thin column     the 2 x 2 x 4 clear-sky column of tests/test_gpu_emission_expected.py (optical depth 0.02), 64 x 64 pixels
  128 x 128 x 64  a cloud layer in clear air, 128 x 128 pixels, both grids in global memory (they do not fit LDS)

For each: seconds and paths per second of both estimators (after a warm-up of each, `reps` interleaved repetitions, the median and
all of them), the median over the pixels of their standard errors, and the figure of merit 1 / (sigma^2 t) of the expected-value
estimator over the collision estimator's.  And the entries that exist on the parent commit -- the emission camera (collision
estimator) and the solar camera on the step cloud --, with --parent-lib once more by a library built from the parent commit's
sources in a process of its own, one repetition per round between the others.

    python scripts/expected_emission_cost.py [--parent-lib ab/libmcbrat_parent.so] [--out profiles/expected_emission_cost.json]

Times are a host clock around the synchronous call (memset, uploads, set-up kernel, kernel, read-back)."""
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


def _integrator(case, solar=None):
    import mcbrat3d_amd as M
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, minForwardTableSize=1801)
    if solar:
        integ.prepare(dom, M.new_PhotonStream(solar[0], solar[1], numberOfPhotons=10 ** 13))
    else:
        integ.prepareDomain(dom)
    return integ, dom


def step_cloud():
    import mcbrat3d_amd as M
    from mcbrat3d_amd.camera import new_Camera
    case = cases.step_cloud(0.99)
    nx, ny, nz = 32, 1, 32
    case["temps"] = np.broadcast_to(290.0 - 40.0 * (np.arange(nz) + 0.5) / nz, (nx, ny, nz)).copy()
    case["lambda_um"], case["sfc_temp"] = 10.0, 295.0
    integ, dom = _integrator(case, solar=(1.0, 0.0))
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    xe, ye, ze = case["xe"], case["ye"], case["ze"]
    cam = new_Camera("orthographic", npx=nx, npy=ny, mu=1.0, phi=0.0, gridInLds=1, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=ze[-1])
    return integ, cam, cell, sfc, 4096, 16


def thin_column():
    """the column of tests/test_gpu_emission_expected.py's thin-air check: the one definition"""
    from mcbrat3d_amd.camera import new_Camera
    from tests.test_gpu_emission_expected import thin_column as column
    case, cell, sfc = column()
    integ, _ = _integrator(case)
    cam = new_Camera("orthographic", npx=64, npy=64, mu=1.0, phi=0.0, footprint=(0.0, 1.0, 0.0, 1.0), height=1.0)
    return integ, cam, cell, sfc, 256, 8


def large_scene():
    """128 x 128 x 64 over 12.8 x 12.8 x 6.4: clear air of extinction 0.01, a broken cloud layer (extinction 5 to 25, omega0 0.6)
    between 1.6 and 2.4, temperatures falling with height over a warm grey surface"""
    from mcbrat3d_amd.camera import new_Camera
    nx, ny, nz = 128, 128, 64
    e = 0.1 * np.arange(nx + 1)
    ze = 0.1 * np.arange(nz + 1)
    rng = np.random.default_rng(128)
    gas, cloud = np.full((nx, ny, nz), 0.01), np.zeros((nx, ny, nz))
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    broken = (np.sin(ix / 9.0) + np.cos(iy / 7.0) + 0.3 * rng.standard_normal((nx, ny))) > 0.2
    cloud[:, :, 16:24] = np.where(broken, rng.uniform(5.0, 25.0, (nx, ny)), 0.0)[:, :, None]
    ones = np.ones((nx, ny, nz), np.int32)
    case = dict(name="large", xe=e, ye=e.copy(), ze=ze, albedo=0.05,
                components=[dict(ext=gas, ssa=np.full_like(gas, 0.1), pfIndex=ones, legendre=[cases.hg_legendre(0.0, 2)]),
                            dict(ext=cloud, ssa=np.full_like(cloud, 0.6), pfIndex=ones, legendre=[cases.hg_legendre(0.85, 64)])])
    integ, _ = _integrator(case)
    cell = np.broadcast_to((9.0 - 4.0 * (np.arange(nz) + 0.5) / nz)[:, None, None], (nz, ny, nx)).astype(np.float32).copy()
    cam = new_Camera("orthographic", npx=128, npy=128, mu=1.0, phi=0.0, gridInLds=-1, footprint=(e[0], e[-1], e[0], e[-1]), height=ze[-1])
    return integ, cam, cell, np.full((ny, nx), 9.5, np.float32), 64, 8


WORKLOADS = {"step cloud, nadir image 32 x 1 from the top": step_cloud, "thin clear-sky column, 64 x 64 pixels": thin_column,
             "128 x 128 x 64, 128 x 128 pixels, global memory": large_scene}


def emission(integ, cam, cell, sfc, spp, nb, estimator, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    t0 = time.perf_counter()
    kw = {} if estimator == "collision" else dict(estimator=estimator)   # (the parent commit's binding has no keyword)
    out = integ.renderCameraEmission(cam, new_RandomNumberSequence(seed), spp, nb, cellSource=cell, surfaceSource=sfc, **kw)
    dt = time.perf_counter() - t0
    assert out["dropped"] == 0
    return dt, out


def solar(integ, cam, spp, nb, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    t0 = time.perf_counter()
    out = integ.renderCamera(cam, new_RandomNumberSequence(seed), spp, nb)
    dt = time.perf_counter() - t0
    assert out["dropped"] == 0
    return dt


def child():
    """the step cloud's emission camera and solar camera with whatever library MCBRAT_LIB names: a warm-up of each, then one
    repetition of both per line of standard input"""
    integ, cam, cell, sfc, spp, nb = step_cloud()
    emission(integ, cam, cell, sfc, spp, nb, "collision", 1)
    solar(integ, cam, spp, nb, 1)
    print("ready", flush=True)
    for line in sys.stdin:
        print(repr(emission(integ, cam, cell, sfc, spp, nb, "collision", int(line))[0]), repr(solar(integ, cam, spp, nb, int(line))), flush=True)
    integ.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    try:  # (where PyTorch is installed it comes first: one HIP runtime per process)
        import torch  # noqa: F401
    except Exception:
        pass
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
    res = dict(reps=a.reps, workloads={})
    for name, make in WORKLOADS.items():
        integ, cam, cell, sfc, spp, nb = make()
        paths = cam.npx * cam.npy * spp * nb
        times = {"collision": [], "expected": []}
        first = name.startswith("step cloud")
        if first:
            times["solar camera"] = []
            if parent:
                times["collision, parent commit"], times["solar camera, parent commit"] = [], []
            solar(integ, cam, spp, nb, 1)
        outs = {}
        for est in ("collision", "expected"):
            emission(integ, cam, cell, sfc, spp, nb, est, 1)  # warm-up
        for r in range(a.reps):
            for est in ("collision", "expected"):
                dt, outs[est] = emission(integ, cam, cell, sfc, spp, nb, est, 100 + r)
                times[est].append(dt)
            if first:
                times["solar camera"].append(solar(integ, cam, spp, nb, 100 + r))
                if parent:
                    parent.stdin.write("%d\n" % (100 + r))
                    parent.stdin.flush()
                    e, s = parent.stdout.readline().split()
                    times["collision, parent commit"].append(float(e))
                    times["solar camera, parent commit"].append(float(s))
        integ.finalize()
        med = {k: float(np.median(v)) for k, v in times.items()}
        sigma = {k: float(np.median(outs[k]["radiance_StdErr"])) for k in outs}   # (the last repetition's: the same seed for both)
        w = dict(paths=paths, samplesPerPixel=spp, batches=nb, seconds_median=med, paths_per_s={k: paths / v for k, v in med.items()},
                 ns_per_path={k: 1e9 * v / paths for k, v in med.items()}, median_standard_error=sigma,
                 mean_radiance={k: float(outs[k]["radiance"].mean()) for k in outs},
                 expected_to_collision_seconds=med["expected"] / med["collision"],
                 collision_to_expected_standard_error=sigma["collision"] / sigma["expected"] if sigma["expected"] > 0 else None,
                 figure_of_merit_expected_over_collision=(sigma["collision"] ** 2 * med["collision"]) / (sigma["expected"] ** 2 * med["expected"])
                 if sigma["expected"] > 0 else None, seconds_all=times)
        if first and parent:
            for k in ("collision", "solar camera"):
                p = times[k + ", parent commit"]
                w[k + ": this commit / parent commit"] = med[k] / med[k + ", parent commit"]
                w[k + ": the parent's spread (max - min) / median"] = (max(p) - min(p)) / med[k + ", parent commit"]
        res["workloads"][name] = w
    if parent:
        parent.stdin.close()
        assert parent.wait(timeout=60) == 0
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
