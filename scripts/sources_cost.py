"""What the solar sources cost: photons/s of the tracing kernel for the Directional, Flux,
RandomAzimuth and Spotlight sources on the plan the library picks, same photons, repetitions interleaved.

    python scripts/sources_cost.py [--out FILE]

Workloads: the step cloud (block walk, tallies in LDS) and landsatLike128 (face-by-face walk, tallies in global memory,
where a spotlight sends every photon into one column first).  Flux launches grazing photons whose first legs are long:
that is physics, not kernel cost."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402

KINDS = ("Directional", "Flux", "RandomAzimuth", "Spotlight")


def stream(M, kind, mu0, phi0):
    n = 10 ** 13
    if kind == "Directional":
        return M.new_PhotonStream(mu0, phi0, numberOfPhotons=n)
    if kind == "RandomAzimuth":
        return M.new_PhotonStream(mu0, numberOfPhotons=n)
    if kind == "Flux":
        return M.new_PhotonStream(numberOfPhotons=n)
    return M.new_PhotonStream(mu0, phi0, solarX=0.5, solarY=0.5, numberOfPhotons=n)


def rate(dom, integ, photons, ppb, nb, seed):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ.resetMoments()
    n = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(seed), photons, ppb, nb)
    return n / (integ.lastTraceMs() * 1e-3)


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
        dom = cases.product_domain(case)
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001)
        streams = {k: stream(M, k, mu0, phi0) for k in KINDS}
        for k in KINDS:  # warm-up: tables, code, the event-threshold guess
            rate(dom, integ, streams[k], ppb, nb, 1)
        rates = {k: [] for k in KINDS}
        for r in range(a.reps):  # interleaved, so that clock drift hits every kind alike
            for k in KINDS:
                rates[k].append(rate(dom, integ, streams[k], ppb, nb, 1234 + r))
        assert integ.badPhotons() == 0
        med = {k: float(np.median(v)) for k, v in rates.items()}
        row = dict(workload=name, photons_per_call=ppb * nb, walk=integ.walkMode(), photons_per_s=med, all=rates,
                   vs_directional_pct={k: 100.0 * (med[k] / med["Directional"] - 1.0) for k in KINDS})
        integ.finalize()
        res.append(row)
        print("%-16s " % name + "  ".join("%s %.3e (%+.1f %%)" % (k, med[k], row["vs_directional_pct"][k]) for k in KINDS),
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
