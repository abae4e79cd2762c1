"""What an emission render costs beside the solar camera (DESIGN.md sections 4.22 and 5): on the step cloud with a thermal set-up
(temperatures falling with height, a warm surface, 10 um), paths per second of a nadir image of the whole domain -- one pixel
per column, from the top, the pixels and samples of scripts/camera_cost.py -- for the emission camera and for the solar camera
(mu0 = 1, as section 5.00), each with the grid in global memory and in LDS; after a warm-up, five runs, median and all five.

    python scripts/emission_cost.py [--out profiles/emission_cost.json]

Times are a host clock around the synchronous call (memset, uploads, kernel, read-back), as section 5.00 timed the camera."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import mcbrat3d_amd as M
    from mcbrat3d_amd.camera import new_Camera
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    case = cases.step_cloud(0.99)
    nx, ny, nz = 32, 1, 32
    case["temps"] = np.broadcast_to(290.0 - 40.0 * (np.arange(nz) + 0.5) / nz, (nx, ny, nz)).copy()
    case["lambda_um"], case["sfc_temp"] = 10.0, 295.0
    dom = cases.product_domain(case)
    xe, ye, ze = case["xe"], case["ye"], case["ze"]
    cell, sfc = M.planck_sources(dom, case["sfc_temp"])
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, minForwardTableSize=1801)
    integ.prepare(dom, M.new_PhotonStream(1.0, 0.0, numberOfPhotons=10 ** 13))
    spp, nb = 4096, 16

    def cam(lds):
        return new_Camera("orthographic", npx=nx, npy=ny, mu=1.0, phi=0.0, gridInLds=lds, footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=ze[-1])

    def render(kind, lds, seed):
        rng = new_RandomNumberSequence(seed)
        t0 = time.perf_counter()
        if kind == "emission":
            out = integ.renderCameraEmission(cam(lds), rng, spp, nb, cellSource=cell, surfaceSource=sfc)
        else:
            out = integ.renderCamera(cam(lds), rng, spp, nb)
        secs = time.perf_counter() - t0
        assert out["dropped"] == 0
        return out, secs

    res = dict(workload="step cloud, thermal set-up", grid=[nx, ny, nz], paths=nx * ny * spp * nb, paths_per_s={}, all={})
    for kind in ("solar", "emission"):
        for lds in (0, 1):
            render(kind, lds, 1)  # warm-up
            rates = [nx * ny * spp * nb / render(kind, lds, 100 + r)[1] for r in range(a.reps)]
            key = "%s, gridInLds %d" % (kind, lds)
            res["paths_per_s"][key], res["all"][key] = float(np.median(rates)), rates
    out, _ = render("emission", -1, 7)
    res["emission_mean_radiance"] = float(out["radiance"].mean())
    res["emission_relative_error"] = float(np.median(out["radiance_StdErr"] / out["radiance"]))
    integ.finalize()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
