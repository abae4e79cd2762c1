"""What recording scattering orders costs (recScatOrd): photons/s of the tracing kernel with the orders
off and on (numRecScatOrd = 10) on the same plan, same photons, repetitions interleaved.

    python scripts/orders_cost.py [--out FILE]

Workloads: landsatLike128 (flux), the same field with 4 view directions, and the step cloud on the face-by-face walk
(blockWalk = 0, the plan a run with orders gets) -- with the block walk's figure beside it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import cases  # noqa: E402


def rate(M, dom, integ, photons, ppb, nb, reps, orders, seed0=1234):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    integ.specifyParameters(numRecScatOrd=orders)
    out = []
    for r in range(reps):
        integ.resetMoments()
        n = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(seed0 + r), photons, ppb, nb)
        out.append(n / (integ.lastTraceMs() * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import mcbrat3d_amd as M
    landsat = cases.landsat_like()
    work = [
        ("landsatLike128 flux", landsat, (0.5, 30.0), {}, {}, 200000, 50),
        ("landsatLike128 4 directions", landsat, (0.5, 30.0),
         dict(minForwardTableSize=10001, intensityMus=[1.0, 0.8, 0.6, 0.4], intensityPhis=[0.0, 45.0, 90.0, 180.0],
              computeIntensity=True), {}, 100000, 20),
        ("step cloud, blockWalk=0", cases.step_cloud(0.99), (1.0, 0.0), {}, dict(blockWalk=0), 200000, 50),
    ]
    res = []
    for name, case, (mu0, phi0), params, tuning, ppb, nb in work:
        dom = cases.product_domain(case)
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001, **params)
        if tuning:
            integ.setTuning(**tuning)
        photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
        rate(M, dom, integ, photons, ppb, nb, 1, -1)  # warm-up: tables, code, the event-threshold guess
        rate(M, dom, integ, photons, ppb, nb, 1, 10)
        off, on = [], []
        for r in range(a.reps):  # interleaved, so that clock drift hits both alike
            off += rate(M, dom, integ, photons, ppb, nb, 1, -1, 1234 + r)
            on += rate(M, dom, integ, photons, ppb, nb, 1, 10, 1234 + r)
        row = dict(workload=name, photons_per_call=ppb * nb, off=float(np.median(off)), on=float(np.median(on)),
                   off_all=off, on_all=on, cost_pct=100.0 * (1.0 - float(np.median(on)) / float(np.median(off))),
                   walk_off=integ.walkMode())
        if name.startswith("step"):  # the plan with orders as it would be without the preference for the grid in LDS
            integ.setTuning(privateTallies=2)
            row["on_tables_in_lds_grid_in_hbm"] = float(np.median(rate(M, dom, integ, photons, ppb, nb, a.reps, 10)))
            integ.setTuning(privateTallies=1, blockWalk=1)
            row["blockWalk_off_orders"] = float(np.median(rate(M, dom, integ, photons, ppb, nb, a.reps, -1)))
        integ.finalize()
        res.append(row)
        print("%-30s off %.3e  on %.3e  photons/s  (%+.1f %%)%s" % (
            name, row["off"], row["on"], -row["cost_pct"],
            ("  on, grid in HBM: %.3e  block walk, orders off: %.3e" % (row["on_tables_in_lds_grid_in_hbm"], row["blockWalk_off_orders"]))
            if "blockWalk_off_orders" in row else ""), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
