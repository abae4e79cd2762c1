"""What the actinic flux of every cell costs (recActinicFlux): photons/s of the tracing kernel (median of
the repetitions, interleaved) with

    default   the workload's default plan (layer skipping, clear-air flight, block walk: whatever the library chooses),
    facewalk  the setting off on the face-by-face walk (layerSkip = 0, blockWalk = 0): the walk the setting needs,
    actinic   the setting on,
    levels    level fluxes alone, on this tree's library, and
    parent    level fluxes alone, on a library built from the parent commit (--parent-lib),

and the spread of the repetitions (max - min) of each.  The tally is one memory-side atomic per cell crossed: what it costs is
`actinic` against `facewalk`; what the walk it needs costs is `facewalk` against `default`.  The LVL kernels are the same code in
both libraries: `levels` should agree with `parent` within the measured spread.

    python scripts/actinic_cost.py --parent-lib /path/to/parent/libmcbrat_hip.so [--reps 5] [--out profiles/actinic_cost.json]

Each library lives in a process of its own (a process loads one); the parent of the two only hands out the turns.
Workloads: the step cloud, the plane-parallel config 1 and landsatLike128, 10^7 photons per call."""
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
SETTINGS = {"default": {}, "facewalk": {}, "actinic": {"recActinicFlux": True}, "levels": {"recLevelFluxes": True}}


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
                integ.specifyParameters(minInverseTableSize=10001, **SETTINGS[key])
                if key == "facewalk":
                    integ.setTuning(layerSkip=0, blockWalk=0)
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
            raise RuntimeError("actinic_cost: a worker ended (exit status %s)" % self.p.wait())
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
    turns = [(key, None, key) for key in SETTINGS]
    libs = {None: Library()}
    if a.parent_lib:
        libs[a.parent_lib] = Library(a.parent_lib)
        turns.append(("parent", a.parent_lib, "levels"))
    res = []
    for w, (name, _, _, _) in enumerate(WORK):
        walks = {}
        for path, lib in libs.items():
            walks.update({("parent" if path else k): v for k, v in lib.ask("open", w, ["levels"] if path else list(SETTINGS)).items()})
        rates = {key: [] for key, _, _ in turns}
        for r in range(a.reps):  # interleaved, so that clock drift hits all alike
            for key, path, setting in turns:
                rates[key].append(libs[path].ask("rate", setting, 1234 + r))
        for lib in libs.values():
            lib.ask("close")
        med = {key: float(np.median(v)) for key, v in rates.items()}
        spread = {key: float(np.max(v) - np.min(v)) for key, v in rates.items()}
        row = dict(workload=name, photons_per_call=PPB * NB, median=med, spread=spread, all=rates, walk=walks,
                   facewalk_cost_pct=100.0 * (1.0 - med["facewalk"] / med["default"]),
                   actinic_cost_pct=100.0 * (1.0 - med["actinic"] / med["facewalk"]),
                   levels_cost_pct=100.0 * (1.0 - med["levels"] / med["facewalk"]))
        text = "%-28s default %.3e  facewalk %.3e (spread %.1e)  actinic %.3e (spread %.1e)  levels %.3e (spread %.1e) photons/s: the tally %+.1f %%" % (
            name, med["default"], med["facewalk"], spread["facewalk"], med["actinic"], spread["actinic"], med["levels"], spread["levels"],
            -row["actinic_cost_pct"])
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
