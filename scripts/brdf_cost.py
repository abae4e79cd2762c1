"""What a BRDF surface costs: photons/s of the tracing kernel over a uniform surface described as
Lambertian (a = 0.3), as RPV in its Lambertian limit, as a vegetation-like RPV, as Ross-Li and as a Cox-Munk ocean (section
4.11.1) with its glint sampler and without (option glintSampling 1 / 0), fluxes only and with a nadir radiance, same photons,
repetitions interleaved.  Last, what the sampler is for: the batch standard error of the step cloud's fluxUp over the ocean at
mu0 = 0.2, with and without it.

    python scripts/brdf_cost.py [--out profiles/brdf_cost.json]

Every surface runs face by face (blockWalk = 0): BRDF surfaces have no block walk, so the Lambertian description is
measured on the same walk.  Workloads: the step cloud (tallies and grid in LDS) and landsatLike128 (tallies in global
memory).  A surface that reflects more sends more photons back up through the cloud: part of a difference is physics."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402

OCEAN = (7.0, 1.34, 0.22, 0.02)
# (label, model, parameters, options of the integrator)
SURFACES = (("Lambertian", "Lambertian", (0.3,), {}), ("RPV limit", "RPV", (0.3, 1.0, 0.0, 1.0), {}),
            ("RPV vegetation", "RPV", (0.3, 0.7, -0.1, 0.3), {}), ("RossLi", "RossLi", (0.3, 0.15, 0.05), {}),
            ("CoxMunk sampled", "CoxMunk", OCEAN, dict(glintSampling=1)), ("CoxMunk plain", "CoxMunk", OCEAN, dict(glintSampling=0)))


def rate(dom, integ, photons, ppb, nb, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ.resetMoments()
    n = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(seed), photons, ppb, nb)
    return n / (integ.lastTraceMs() * 1e-3)


def glint_noise(M, ppb=200000, nb=50, mu0=0.2):
    """Batch standard error of the step cloud's domain-mean fluxUp over the ocean, glintSampling 0 and 1, the same photons."""
    from mcbrat3d_amd import driver
    case = cases.step_cloud(0.99)
    dom = cases.product_domain(case)
    row = dict(workload="step cloud", quantity="meanFluxUp", mu0=mu0, photons_per_call=ppb * nb, batches=nb)
    for g in (0, 1):
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001, surfaceBDRF=M.new_SurfaceDescription(np.float32(OCEAN), model="CoxMunk"))
        integ.setTuning(blockWalk=0)
        integ.setOption(glintSampling=g)
        rate(dom, integ, M.new_PhotonStream(mu0, 0.0, numberOfPhotons=10 ** 13), ppb, nb, 4321)
        integ.synchronize()
        st = driver.statistics(driver.unpack_moments(integ.moments().copy(), 32, 1, 32))
        row["glintSampling %d" % g] = dict(meanFluxUp=float(st["meanFluxUp"]), stdErr=float(st["meanFluxUp_StdErr"]))
        integ.finalize()
    row["stdErr_ratio_plain_over_sampled"] = row["glintSampling 0"]["stdErr"] / row["glintSampling 1"]["stdErr"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import mcbrat3d_amd as M
    work = [("step cloud", cases.step_cloud(0.99), (1.0, 0.0), 200000, 50),
            ("landsatLike128", cases.landsat_like(), (0.5, 30.0), 200000, 50)]
    res = []
    for name, case, (mu0, phi0), ppb, nb in work:
        for radiance in (False, True):
            dom = cases.product_domain(case)
            photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
            integs = {}
            for label, model, q, options in SURFACES:
                integ = M.new_Integrator(dom)
                kw = dict(intensityMus=[1.0], intensityPhis=[0.0], computeIntensity=True, minForwardTableSize=1801) if radiance else {}
                integ.specifyParameters(minInverseTableSize=10001, surfaceBDRF=M.new_SurfaceDescription(np.float32(q), model=model), **kw)
                integ.setTuning(blockWalk=0)
                integ.setOption(**options)
                rate(dom, integ, photons, ppb, nb, 1)  # warm-up: tables, code, the event-threshold guess
                integs[label] = integ
            rates = {k: [] for k in integs}
            for r in range(a.reps):  # interleaved, so that clock drift hits every surface alike
                for k, integ in integs.items():
                    rates[k].append(rate(dom, integ, photons, ppb, nb, 1234 + r))
            med = {k: float(np.median(v)) for k, v in rates.items()}
            row = dict(workload=name, radiance="nadir" if radiance else None, photons_per_call=ppb * nb,
                       walk=integs["RossLi"].walkMode(), photons_per_s=med, all=rates,
                       vs_lambertian_pct={k: 100.0 * (med[k] / med["Lambertian"] - 1.0) for k in med})
            for integ in integs.values():
                assert integ.badPhotons() == 0
                integ.finalize()
            res.append(row)
            print("%-16s %-6s " % (name, "nadir" if radiance else "flux") +
                  "  ".join("%s %.3e (%+.1f %%)" % (k, med[k], row["vs_lambertian_pct"][k]) for k in med), flush=True)
    res.append(glint_noise(M))
    print("step cloud, mu0 0.2, fluxUp standard error: plain %.3e sampled %.3e ratio %.1f" % (
        res[-1]["glintSampling 0"]["stdErr"], res[-1]["glintSampling 1"]["stdErr"], res[-1]["stdErr_ratio_plain_over_sampled"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
