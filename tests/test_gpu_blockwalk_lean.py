"""The block walk's collision iteration does the same arithmetic per photon as before it was trimmed.

Tallies are fixed point, so "the same arithmetic" means the same moment arrays bit for bit: against moments recorded with the
library from before the trim (tests/golden/blockwalk_moments.npz, made by tests/golden/make_blockwalk_moments.py), and between
the launch-wide work units and the per-batch cut.  (The instrumented instantiation's fates against the oracle:
tests/test_gpu_block_walk.py.)  Run on the MI355X box with `-m gpu`."""
import os

import numpy as np
import pytest

from tests.golden import make_blockwalk_moments as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blockwalk_moments.npz")


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("run", G.RUNS, ids=[r[0] for r in G.RUNS])
def test_block_walk_moments_equal_the_recorded_ones(M, golden, run):
    done, mom, walk = G.run(M, *run)
    assert walk["blockWalk"]
    assert done == run[5] * run[6] == int(golden[run[0] + "_photons"][0])
    assert mom.shape == golden[run[0]].shape
    assert np.array_equal(mom, golden[run[0]])


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("run", G.RUNS, ids=[r[0] for r in G.RUNS])
def test_block_walk_moments_equal_with_per_batch_units(M, run):
    done, wide, _ = G.run(M, *run)
    done1, cut, _ = G.run(M, *run, batch_units=1)
    assert done == done1 == run[5] * run[6]
    assert np.array_equal(wide, cut)

