"""What tallying the flux through the vertical faces of every cell costs (recSideFluxes): photons/s of
the tracing kernel (median of the repetitions, interleaved) with

    parent   level fluxes alone, on a library built from the parent commit (--parent-lib),
    levels   level fluxes alone, on this tree's library, and
    side     the setting on,

and the spread of the repetitions (max - min) of each.  The LVL kernels are meant to be the same code in both libraries: `levels`
must agree with `parent` within the measured spread.  What the side tally costs (`side` against `levels`) is reported.

    python scripts/side_flux_cost.py --parent-lib /path/to/parent/libmcbrat_hip.so [--reps 5] [--out profiles/side_flux_cost.json]

Each library lives in a process of its own (a process loads one); the parent of the two only hands out the turns.
Workloads: the step cloud, the plane-parallel config 1 (every deposit of a level lands on ONE address) and landsatLike128,
10^7 photons per call."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORK = [("step cloud", "step_cloud", (0.99,), (1.0, 0.0)), ("plane parallel (config 1)", "plane_parallel", (0.99,), (1.0, 0.0)),
        ("landsatLike128", "landsat_like", (), (0.5, 30.0))]
PPB, NB = 200000, 50


def worker():
    """Commands on stdin, one JSON answer per line on stdout: ["open", workload index, [settings]], ["rate", setting, seed], ["close"]."""
    import mcbrat3d_amd as M
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    from tests import cases
    out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)  # (whatever else prints goes to stderr: stdout carries the answers)
    dom = photons = None
    integs = {}

    def rate(integ, seed):
        integ.resetMoments()
        n = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(seed), photons, PPB, NB)
        return n / (integ.lastTraceMs() * 1e-3)

    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd[0] == "open":
            _, maker, args, (mu0, phi0) = WORK[cmd[1]]
            dom = cases.product_domain(getattr(cases, maker)(*args))
            photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 13)
            walks = {}
            for key in cmd[2]:  # one integrator per setting: switching drops the moment arrays and the event threshold
                integ = M.new_Integrator(dom)
                integ.specifyParameters(minInverseTableSize=10001, recLevelFluxes=True, **({"recSideFluxes": True} if key == "side" else {}))
                rate(integ, 99)  # warm-up: tables, code, the event-threshold guess
                integs[key], walks[key] = integ, integ.walkMode()
            ans = walks
        elif cmd[0] == "rate":
            ans = rate(integs[cmd[1]], cmd[2])
        else:
            for integ in integs.values():
                integ.finalize()
            integs = {}
            ans = None
        out.write(json.dumps(ans) + "\n")
        out.flush()


class Library:
    def __init__(self, path=None):
        env = dict(os.environ)
        if path:
            env.update(MCBRAT_LIB=os.path.abspath(path), MCBRAT_LIB_OLD="1")
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  env=env, cwd=ROOT, text=True)

    def ask(self, *cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("side_flux_cost: a worker ended (exit status %s)" % self.p.wait())
        return json.loads(line)

    def end(self):
        self.p.stdin.close()
        return self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libmcbrat_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    import numpy as np
    turns = [("levels", None, "levels"), ("side", None, "side")]
    libs = {None: Library()}
    if a.parent_lib:
        libs[a.parent_lib] = Library(a.parent_lib)
        turns.insert(0, ("parent", a.parent_lib, "levels"))
    res = []
    for w, (name, _, _, _) in enumerate(WORK):
        walks = {}
        for path, lib in libs.items():
            walks.update({("parent" if path else k): v for k, v in lib.ask("open", w, ["levels"] if path else ["levels", "side"]).items()})
        rates = {key: [] for key, _, _ in turns}
        for r in range(a.reps):  # interleaved, so that clock drift hits all alike
            for key, path, setting in turns:
                rates[key].append(libs[path].ask("rate", setting, 1234 + r))
        for lib in libs.values():
            lib.ask("close")
        med = {key: float(np.median(v)) for key, v in rates.items()}
        spread = {key: float(np.max(v) - np.min(v)) for key, v in rates.items()}
        row = dict(workload=name, photons_per_call=PPB * NB, median=med, spread=spread, all=rates, walk=walks,
                   side_cost_pct=100.0 * (1.0 - med["side"] / med["levels"]))
        text = "%-28s levels %.3e (spread %.1e)  side %.3e (spread %.1e) photons/s: the side tally %+.1f %%" % (
            name, med["levels"], spread["levels"], med["side"], spread["side"], -row["side_cost_pct"])
        if "parent" in med:
            row["levels_minus_parent"] = med["levels"] - med["parent"]
            row["levels_agree_with_parent"] = bool(abs(row["levels_minus_parent"]) <= max(spread["levels"], spread["parent"]))
            text += "; parent %.3e (spread %.1e), levels - parent %+.2e: %s the spread" % (
                med["parent"], spread["parent"], row["levels_minus_parent"], "within" if row["levels_agree_with_parent"] else "OUTSIDE")
        res.append(row)
        print(text, flush=True)
    for lib in libs.values():
        lib.end()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
