"""What the backward sensors cost and when they pay (DESIGN.md sections 4.20 and 5): on the step cloud and on landsatLike128,

  * throughput: paths per second of point sensors on the ground facing up, one under every column (the step cloud also: at the
    top, facing down), camera_kernel<.., SENSOR = true> with the grid in LDS and in global memory (where it fits LDS: both), after
    a warm-up, five runs, median and all five -- and, beside it, the camera's paths per second on the same scene in the same
    session (a nadir image from the top, one pixel per column: what scripts/camera_cost.py measures);
  * time to a 1 % standard error of the irradiance on the ground for (i) one sensor, (ii) a sensor under every column, backward
    (area sensors equal to the columns' faces: the quantity the forward run tallies) and forward (recLevelFluxes +
    recDirectLevelFluxes, levelFluxDown at level 0, every column at once): a run of known size, its median relative standard
    error over the columns in question, scaled by (error / 1 %)^2.

    python scripts/sensor_cost.py [--out profiles/sensor_cost.json]

Forward times are the tracing kernels' (lastTraceMs); backward times are a host clock around the synchronous call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    out = call()
    assert out["dropped"] == 0
    return out, time.perf_counter() - t0


def to_one_percent(seconds, rel):
    return float(seconds * (rel / 0.01) ** 2)


def rel_error(mean, err):
    m, e = np.asarray(mean, np.float64).ravel(), np.asarray(err, np.float64).ravel()
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
    from mcbrat3d_amd.sensors import new_Sensors
    rng = new_RandomNumberSequence
    work = [("step cloud", cases.step_cloud(0.99), (0.5, 30.0), 200000, 50, 4096, True),
            ("landsatLike128", cases.landsat_like(), (0.5, 30.0), 1000000, 50, 256, False)]
    res = []
    for name, case, (mu0, phi0), ppb, nb, samples, top_too in work:
        dom = cases.product_domain(case)
        nx, ny, nz = dom.numX, dom.numY, dom.numZ
        xe, ye, ze = (np.asarray(case[k], float) for k in ("xe", "ye", "ze"))
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001, minForwardTableSize=1801, recLevelFluxes=True, recDirectLevelFluxes=True)
        photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
        integ.computeRadiativeTransfer(dom, rng(1), photons, ppb, 2)  # warm-up: tables, code, the event threshold
        integ.resetMoments()
        n = integ.computeRadiativeTransfer(dom, rng(77), photons, ppb, nb)
        fwd_s = integ.lastTraceMs() * 1e-3
        st = driver.statistics(driver.unpack_moments(integ.moments().copy(), nx, ny, nz, levelFluxes=True, directLevelFluxes=True))
        fmean, ferr = st["levelFluxDown"][:, :, 0], st["levelFluxDown_StdErr"][:, :, 0]  # [ix, iy]
        row = dict(workload=name, grid=[nx, ny, nz], mu0=mu0, forward=dict(photons=int(n), seconds=fwd_s, photons_per_s=n / fwd_s))

        xc, yc = 0.5 * (xe[1:] + xe[:-1]), 0.5 * (ye[1:] + ye[:-1])
        centres = [(x, y) for y in yc for x in xc]
        ground = new_Sensors([(x, y, ze[0]) for x, y in centres])
        top = new_Sensors([(x, y, ze[-1]) for x, y in centres], tilt=180.0)
        faces = new_Sensors([(xe[i], ye[j], ze[0]) for j in range(ny) for i in range(nx)],
                            extents=[((xe[i + 1] - xe[i], 0, 0), (0, ye[j + 1] - ye[j], 0)) for j in range(ny) for i in range(nx)])
        cam = lambda lds: new_Camera("orthographic", npx=nx, npy=ny, mu=1.0, phi=0.0, gridInLds=lds,  # noqa: E731
                                     footprint=(xe[0], xe[-1], ye[0], ye[-1]), height=ze[-1])
        fits = True
        try:
            integ.renderSensors(ground, rng(1), 64, 1, gridInLds=1)
        except M.McbratError:
            fits = False
        row["grid_fits_lds"] = fits
        row["paths_per_s"], row["all"] = {}, {}
        sets = [("ground sensors facing up", ground)] + ([("top sensors facing down", top)] if top_too else [])
        for lds in ([0, 1] if fits else [0]):
            key = "gridInLds %d" % lds
            for what, s in sets:
                timed(lambda: integ.renderSensors(s, rng(1), samples, 16, gridInLds=lds))  # warm-up
                rates = [nx * ny * samples * 16 / timed(lambda: integ.renderSensors(s, rng(100 + r), samples, 16, gridInLds=lds))[1] for r in range(a.reps)]
                row["all"]["%s, %s" % (what, key)] = rates
                row["paths_per_s"]["%s, %s" % (what, key)] = float(np.median(rates))
            timed(lambda: integ.renderCamera(cam(lds), rng(1), samples, 16))  # warm-up
            rates = [nx * ny * samples * 16 / timed(lambda: integ.renderCamera(cam(lds), rng(100 + r), samples, 16))[1] for r in range(a.reps)]
            row["all"]["camera nadir image, %s" % key] = rates
            row["paths_per_s"]["camera nadir image, %s" % key] = float(np.median(rates))
        # time to a 1 % standard error of the irradiance on the ground
        out, secs = timed(lambda: integ.renderSensors(faces, rng(7), samples, 16))
        every = dict(forward_s=to_one_percent(fwd_s, rel_error(fmean, ferr)),
                     backward_s=to_one_percent(secs, rel_error(out["irradiance"], out["irradiance_StdErr"])),
                     backward_paths=nx * ny * samples * 16, backward_seconds=secs)
        i, j = nx // 2, ny // 2
        k = j * nx + i
        one_face = new_Sensors([faces.positions[k]], extents=[(faces.e1[k], faces.e2[k])])
        out, secs = timed(lambda: integ.renderSensors(one_face, rng(8), 65536, 16))
        one = dict(column=[i, j], forward_s=to_one_percent(fwd_s, float(ferr[i, j] / fmean[i, j])),
                   backward_s=to_one_percent(secs, rel_error(out["irradiance"], out["irradiance_StdErr"])),
                   backward_paths=65536 * 16, backward_seconds=secs)
        row["seconds_to_1_percent"] = {"a sensor under every column": every, "one ground sensor": one}
        assert integ.badPhotons() == 0
        integ.finalize()
        res.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
