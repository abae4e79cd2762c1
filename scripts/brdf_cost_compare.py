"""Two builds of the library on scripts/brdf_cost.py: merges the files that `brdf_cost.py --out` wrote
in alternating runs of a parent commit and of this one into one record.

    python scripts/brdf_cost_compare.py --parent p1.json p2.json .. --this t1.json t2.json .. --out profiles/coxmunk_cost.json
                                        [--earlier FILE --earlier-note TEXT]...

Per workload and surface: every run's rate, the median, and the spread (max - min) / median; for the surfaces both builds know,
the difference of the medians next to the parent's own spread -- a smaller difference cannot be told from noise.  The last row
of this commit's files (the noise of fluxUp over the ocean with and without glint sampling: the same photons every run) is kept
once.  --earlier (repeatable): the medians of a record this script wrote for another shape of the change, kept beside the new ones."""
import argparse
import json

import numpy as np


def rates(runs, w):
    """{surface: every repetition of every run} of workload row w"""
    return {k: [v for r in runs for v in r[w]["all"][k]] for k in runs[0][w]["photons_per_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--this", nargs="+", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--earlier", action="append", default=[])
    ap.add_argument("--earlier-note", action="append", default=[])
    a = ap.parse_args()
    par = [json.load(open(f)) for f in a.parent]
    new = [json.load(open(f)) for f in a.this]
    nwork = len([r for r in par[0] if "photons_per_s" in r])
    out = dict(method="scripts/brdf_cost.py of the parent commit and of this one, built side by side, run alternately in one session on one MI355X; "
                      "medians over every repetition of every run", runs=dict(parent=len(par), this=len(new)), workloads=[])
    for w in range(nwork):
        row = dict(workload=par[0][w]["workload"], radiance=par[0][w]["radiance"], photons_per_call=par[0][w]["photons_per_call"])
        for side, runs in (("parent", par), ("this", new)):
            row[side] = {k: dict(all=v, median=float(np.median(v)), spread=float((max(v) - min(v)) / np.median(v))) for k, v in rates(runs, w).items()}
        row["vs_parent"] = {k: dict(difference=row["this"][k]["median"] / row["parent"][k]["median"] - 1.0, parent_spread=row["parent"][k]["spread"])
                            for k in row["parent"]}
        row["vs_lambertian_pct"] = {k: 100.0 * (row["this"][k]["median"] / row["this"]["Lambertian"]["median"] - 1.0) for k in row["this"]}
        out["workloads"].append(row)
        print("%s, %s" % (row["workload"], "nadir radiance" if row["radiance"] else "fluxes"))
        for k, v in row["vs_parent"].items():
            print("   %-16s parent %.3e this %.3e difference %+.2f %% (parent's spread %.2f %%)" % (
                k, row["parent"][k]["median"], row["this"][k]["median"], 100 * v["difference"], 100 * v["parent_spread"]))
        print("   against the Lambertian description: " + "  ".join("%s %+.1f %%" % kv for kv in row["vs_lambertian_pct"].items()))
    noise = [r for r in new[0] if "stdErr_ratio_plain_over_sampled" in r]
    if noise:
        out["glint_noise"] = noise[0]
        print("fluxUp standard error, step cloud, mu0 %g: plain / sampled = %.2f" % (noise[0]["mu0"], noise[0]["stdErr_ratio_plain_over_sampled"]))
    for f, note in zip(a.earlier, a.earlier_note):
        e = json.load(open(f))
        out.setdefault("earlier_shapes", []).append(dict(note=note, workloads=[
            dict(workload=w["workload"], radiance=w["radiance"], parent={k: v["median"] for k, v in w["parent"].items()},
                 this={k: v["median"] for k, v in w["this"].items()}) for w in e["workloads"]]))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
