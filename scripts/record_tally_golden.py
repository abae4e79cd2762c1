"""Record what the tallies of a small run hold, case by case, for tests/test_gpu_tally_layout.py.

    python scripts/record_tally_golden.py [--out tests/golden/tally_layout_parent.npz]

Only the public Python interface is used, so the script runs unchanged on any commit that has the settings: the committed file was
recorded on the commit before the tally layout moved into mcbrat_layout.h, and the test requires every later commit to give the same
bits.  Per case: the whole array of mcbrat_get_moments, momentsLength(), and every array of reportResults() (which calls every
report function that applies)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SEED = 20261018
PHOTONS_PER_BATCH, BATCHES = 2000, 3
TABLE = 2001
DIRECTIONS = dict(intensityMus=[0.8, 0.35], intensityPhis=[20.0, 200.0], computeIntensity=True)

# name -> (components, specifyParameters keywords)
CASES = {
    "plain fluxes": (1, {}),
    "two directions": (1, DIRECTIONS),
    "two directions, limited contributions, two components": (2, dict(DIRECTIONS, limitIntensityContributions=True, maxIntensityContribution=0.5)),
    "two orders, two directions": (1, dict(DIRECTIONS, recScatOrd=True, numRecScatOrd=2)),
    "levels": (1, dict(recLevelFluxes=True)),
    "levels and direct": (1, dict(recLevelFluxes=True, recDirectLevelFluxes=True)),
    "actinic": (1, dict(recActinicFlux=True)),
    "levels and actinic": (1, dict(recLevelFluxes=True, recActinicFlux=True)),
}


def hg(g, n):
    return np.array([float(np.float32(g)) ** l for l in range(1, n + 1)], np.float64).astype(np.float32)


def domain(M, components):
    """3 x 2 x 4 cells, x edges irregular (the columns' relative areas are used), every cell unlike its neighbours."""
    xe = np.array([0.0, 0.03, 0.08, 0.12])
    ye = 0.046875 * np.arange(3)
    ze = 0.0390625 * np.arange(5)
    shape = (3, 2, 4)
    rng = np.random.default_rng(5)
    dom = M.new_Domain(xe, ye, ze, surfaceAlbedo=0.25)
    share = rng.uniform(0.3, 0.7, shape) if components == 2 else np.ones(shape)
    ext = rng.uniform(8.0, 25.0, shape)
    table = M.new_PhaseFunctionTable([M.new_PhaseFunction(hg(g, 24)) for g in (0.85, 0.5)])
    dom.addOpticalComponent("component1", ext * share, rng.uniform(0.7, 1.0, shape), rng.integers(1, 3, shape).astype(np.int32), table)
    if components == 2:
        other = M.new_PhaseFunctionTable([M.new_PhaseFunction(hg(-0.2, 12))])
        dom.addOpticalComponent("component2", ext * (1.0 - share), rng.uniform(0.8, 1.0, shape), np.ones(shape, np.int32), other)
    dom.getOpticalPropertiesByComponent()
    return dom


def run_case(M, name):
    """-> {key: array} of one case: "moments", "momentsLength" and "report/<name>" for every entry of reportResults()."""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    components, params = CASES[name]
    dom = domain(M, components)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=TABLE, useRayTracing=True, useRussianRoulette=True, LW_flag=-1.0, **params)
    integ.setTuning(maxBatchesInFlight=1)  # one batch per launch round: three rounds
    photons = M.new_PhotonStream(solarMu=0.6, solarAzimuth=30.0, numberOfPhotons=10 ** 9)
    integ.resetMoments()
    done = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, PHOTONS_PER_BATCH, BATCHES)
    assert done == PHOTONS_PER_BATCH * BATCHES and integ.badPhotons() == 0
    out = {"moments": integ.moments().copy(), "momentsLength": np.int64(integ.momentsLength())}
    for k, v in integ.reportResults().items():
        out["report/" + k] = np.ascontiguousarray(v)
    integ.finalize()
    return out


def record(M):
    return {"%s/%s" % (name, k): v for name in CASES for k, v in run_case(M, name).items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "tally_layout_parent.npz"))
    args = ap.parse_args()
    import mcbrat3d_amd
    arrays = record(mcbrat3d_amd)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print("recorded %d arrays of %d cases into %s" % (len(arrays), len(CASES), args.out))
