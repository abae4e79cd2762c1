"""Writes tests/golden/blockwalk_moments.npz: the moment arrays and photon counts of the block walk on a few fixed runs (the
I3RC step cloud under two suns, three random box media), for tests/test_gpu_blockwalk_lean.py.  Tallies are fixed point, so
any later library that does the same arithmetic per photon reproduces them bit for bit.

    python tests/golden/make_blockwalk_moments.py [OUT.npz]     (on an MI355X; MCBRAT_LIB picks the library that makes them)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402

SEED = 2718
# (name, case maker, mu0, phi0, useRussianRoulette, photons per batch, batches, blockWalk option)
RUNS = [
    ("step_sun0", lambda: cases.step_cloud(0.99), 1.0, 0.0, True, 100000, 4, -1),
    ("step_sun60", lambda: cases.step_cloud(0.99), 0.5, 30.0, True, 50000, 3, -1),
] + [("boxes%d" % s, s, None, None, None, 20011, 3, 2) for s in (1, 4, 7)]


def run(M, name, make, mu0, phi0, rr, ppb, nb, block_walk, batch_units=0):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    if isinstance(make, int):
        from tests.test_gpu_block_walk import random_box_case
        case, mu0, phi0, rr = random_box_case(make)
    else:
        case = make()
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, useRayTracing=True, useRussianRoulette=rr)
    integ.setTuning(blockWalk=block_walk)
    integ.setOption(batchUnits=batch_units)
    photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
    integ.resetMoments()
    done = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, ppb, nb)
    mom = integ.moments().copy()
    walk = integ.walkMode()
    integ.finalize()
    return done, mom, walk


def main():
    try:
        import torch  # noqa: F401  (the same HIP runtime order as the test session)
    except Exception:
        pass
    import mcbrat3d_amd as M
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "blockwalk_moments.npz")
    arrays = {}
    for r in RUNS:
        done, mom, walk = run(M, *r)
        assert walk["blockWalk"], r[0]
        arrays[r[0]] = mom
        arrays[r[0] + "_photons"] = np.array([done], np.int64)
    np.savez_compressed(out, **arrays)
    print("wrote", out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
