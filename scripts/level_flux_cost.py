"""What tallying level fluxes costs (recLevelFluxes): photons/s of the tracing kernel (median of the
repetitions, interleaved) with

    off      level fluxes off on the same walk (layerSkip = 0, blockWalk = 0: face by face), and
    on       level fluxes on,

and beside them the workload's rate on its default plan -- what giving up layer skipping, the clear-air flight and the block walk
costs a run that asks for level fluxes.

    python scripts/level_flux_cost.py [--reps 5] [--out profiles/level_flux_cost.json]

Workloads: the step cloud, the plane-parallel config 1 (every deposit of a level lands on ONE address) and landsatLike128."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402


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
            ("plane parallel (config 1)", cases.plane_parallel(0.99), (1.0, 0.0), 200000, 50),
            ("landsatLike128", cases.landsat_like(), (0.5, 30.0), 200000, 50)]
    res = []
    for name, case, (mu0, phi0), ppb, nb in work:
        dom = cases.product_domain(case)
        photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
        # one integrator per setting: switching level fluxes drops the moment arrays and the event threshold
        settings = {"default": (False, {}), "off": (False, dict(layerSkip=0, blockWalk=0)), "on": (True, {})}
        integs, walks = {}, {}
        for key, (levels, tuning) in settings.items():
            integ = M.new_Integrator(dom)
            integ.specifyParameters(minInverseTableSize=10001, recLevelFluxes=levels)
            if tuning:
                integ.setTuning(**tuning)
            rate(dom, integ, photons, ppb, nb, 99)  # warm-up: tables, code, the event-threshold guess
            integs[key], walks[key] = integ, integ.walkMode()
        rates = {key: [] for key in settings}
        for r in range(a.reps):  # interleaved, so that clock drift hits all alike
            for key in settings:
                rates[key].append(rate(dom, integs[key], photons, ppb, nb, 1234 + r))
        for integ in integs.values():
            integ.finalize()
        med = {key: float(np.median(v)) for key, v in rates.items()}
        row = dict(workload=name, photons_per_call=ppb * nb, default=med["default"], off=med["off"], on=med["on"], all=rates,
                   cost_pct=100.0 * (1.0 - med["on"] / med["off"]), plan_cost_pct=100.0 * (1.0 - med["off"] / med["default"]),
                   walk=walks)
        res.append(row)
        print("%-28s default plan %.3e  off %.3e  on %.3e photons/s  (levels %+.1f %%, the plan %+.1f %%)" % (
            name, row["default"], row["off"], row["on"], -row["cost_pct"], -row["plan_cost_pct"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
