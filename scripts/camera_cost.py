"""What the backward camera costs and when it pays (DESIGN.md sections 4.19 and 5): on the step cloud and on landsatLike128,

  * throughput: paths per second of a nadir image of the whole domain (one pixel per column, from the top), camera_kernel with the
    grid in LDS and in global memory (where it fits LDS: both), after a warm-up, five runs, median and all five;
  * time to a 1 % standard error of the pixel mean for (i) the full nadir image, (ii) one pixel, (iii) an 8 x 8 window (the large
    scene only), forward (the INTEN kernels, nadir direction, every column at once) and backward (only the pixels asked for):
    a run of known size, its median relative standard error over the pixels in question, scaled by (error / 1 %)^2.

    python scripts/camera_cost.py [--out profiles/camera_cost.json]

Forward times are the tracing kernels' (lastTraceMs); backward times are a host clock around the synchronous call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402


def render(integ, cam, spp, nb, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    t0 = time.perf_counter()
    out = integ.renderCamera(cam, new_RandomNumberSequence(seed), spp, nb)
    assert out["dropped"] == 0
    return out, time.perf_counter() - t0


def to_one_percent(seconds, rel):
    return float(seconds * (rel / 0.01) ** 2)


def rel_error(mean, err, sel):
    m, e = np.asarray(mean, np.float64)[sel], np.asarray(err, np.float64)[sel]
    return float(np.median(e[m > 0] / m[m > 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.camera import new_Camera
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    work = [("step cloud", cases.step_cloud(0.99), (1.0, 0.0), 200000, 50, 4096, None),
            ("landsatLike128", cases.landsat_like(), (0.5, 30.0), 1000000, 50, 256, 8)]
    res = []
    for name, case, (mu0, phi0), ppb, nb, spp, window in work:
        dom = cases.product_domain(case)
        nx, ny, nz = dom.numX, dom.numY, dom.numZ
        xe, ye, ze = case["xe"], case["ye"], case["ze"]
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001, minForwardTableSize=1801, intensityMus=[1.0], intensityPhis=[0.0], computeIntensity=True)
        photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
        integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(1), photons, ppb, 2)  # warm-up: tables, code, the event threshold
        integ.resetMoments()
        n = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(77), photons, ppb, nb)
        fwd_s = integ.lastTraceMs() * 1e-3
        st = driver.statistics(driver.unpack_moments(integ.moments().copy(), nx, ny, nz, 1))
        fmean, ferr = st["intensity"][:, :, 0].T, st["intensity_StdErr"][:, :, 0].T  # [ny, nx]
        row = dict(workload=name, grid=[nx, ny, nz], mu0=mu0, forward=dict(photons=int(n), seconds=fwd_s, photons_per_s=n / fwd_s))

        def cam(i0, i1, j0, j1, lds=-1):
            return new_Camera("orthographic", npx=i1 - i0, npy=j1 - j0, mu=1.0, phi=0.0, gridInLds=lds,
                              footprint=(xe[i0], xe[i1], ye[j0], ye[j1]), height=ze[-1])

        fits = True
        try:
            render(integ, cam(0, nx, 0, ny, 1), 64, 1, 1)
        except M.McbratError:
            fits = False
        row["grid_fits_lds"] = fits
        rates = {}
        for lds in ([0, 1] if fits else [0]):
            render(integ, cam(0, nx, 0, ny, lds), spp, 16, 1)  # warm-up
            rates["gridInLds %d" % lds] = [nx * ny * spp * 16 / render(integ, cam(0, nx, 0, ny, lds), spp, 16, 100 + r)[1] for r in range(a.reps)]
        row["paths_per_s"] = {k: float(np.median(v)) for k, v in rates.items()}
        row["all"] = rates
        # time to 1 %
        everything = np.ones((ny, nx), bool)
        out, secs = render(integ, cam(0, nx, 0, ny), spp, 16, 7)
        full = dict(forward_s=to_one_percent(fwd_s, rel_error(fmean, ferr, everything)),
                    backward_s=to_one_percent(secs, rel_error(out["radiance"], out["radiance_StdErr"], everything)),
                    backward_paths=nx * ny * spp * 16, backward_seconds=secs)
        i, j = nx // 2, ny // 2
        one = np.zeros((ny, nx), bool)
        one[j, i] = True
        out, secs = render(integ, cam(i, i + 1, j, j + 1), 65536, 16, 8)
        pixel = dict(pixel=[i, j], forward_s=to_one_percent(fwd_s, rel_error(fmean, ferr, one)),
                     backward_s=to_one_percent(secs, rel_error(out["radiance"], out["radiance_StdErr"], np.ones((1, 1), bool))),
                     backward_paths=65536 * 16, backward_seconds=secs)
        row["seconds_to_1_percent"] = {"full nadir image": full, "one pixel": pixel}
        if window:
            i0, j0 = nx // 2 - window // 2, ny // 2 - window // 2
            win = np.zeros((ny, nx), bool)
            win[j0:j0 + window, i0:i0 + window] = True
            out, secs = render(integ, cam(i0, i0 + window, j0, j0 + window), 8192, 16, 9)
            row["seconds_to_1_percent"]["8 x 8 window"] = dict(
                window=[i0, j0, window], forward_s=to_one_percent(fwd_s, rel_error(fmean, ferr, win)),
                backward_s=to_one_percent(secs, rel_error(out["radiance"], out["radiance_StdErr"], np.ones((window, window), bool))),
                backward_paths=window * window * 8192 * 16, backward_seconds=secs)
        assert integ.badPhotons() == 0
        integ.finalize()
        res.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
