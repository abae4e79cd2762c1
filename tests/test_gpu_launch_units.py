"""Work units of the block walk and the device's Philox generator.

The block walk deals each resident workgroup an equal share of the launch's photons, cut across batch boundaries, with the
tallies of the two batches a share may touch in two LDS slabs (mcbrat_api.hip: launch_kernel).  Only the schedule changes:
every photon keeps its arithmetic and tallies are integers, so the moment arrays must equal those of the per-batch cut
(option "batchUnits") bit for bit.  Run on the MI355X box with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_block_walk import random_box_case

pytestmark = pytest.mark.gpu
SEED = 31337


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _moments(M, case, mu0, phi0, rr, ppb, nb, batch_units, block_walk=-1):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
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


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("ppb,nb", [(100000, 100), (123457, 7), (3, 5), (250000, 1)])
def test_launch_wide_units_equal_the_per_batch_cut_on_the_step_cloud(M, ppb, nb):
    case = cases.step_cloud(0.99)
    done, wide, walk = _moments(M, case, 1.0, 0.0, True, ppb, nb, 0)
    assert walk["blockWalk"]
    done1, cut, _ = _moments(M, case, 1.0, 0.0, True, ppb, nb, 1)
    assert done == done1 == ppb * nb
    assert np.array_equal(wide, cut)


@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("seed", range(6))
def test_launch_wide_units_equal_the_per_batch_cut_on_random_box_media(M, seed):
    case, mu0, phi0, rr = random_box_case(seed)
    done, wide, _ = _moments(M, case, mu0, phi0, rr, 20011, 9, 0, block_walk=2)
    done1, cut, _ = _moments(M, case, mu0, phi0, rr, 20011, 9, 1, block_walk=2)
    assert done == done1 == 20011 * 9
    assert np.array_equal(wide, cut)


def test_device_philox_known_answers(M):
    """Random123 kat_vectors for philox4x32-10 (the oracle is pinned to the same ones: tests/test_oracle_pin.py)."""
    from mcbrat3d_amd import _capi
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    # and a few hundred blocks of the photons' own counters (event, slot, id) against the oracle's generator
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    extra = [([int(rng.integers(0, 64)), int(rng.integers(0, 3)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 4))],
              [int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))]) for _ in range(300)]
    rows = [(c, k) for c, k, _ in kat] + extra
    inp = np.array([c + k for c, k in rows], np.uint32)
    out = np.zeros((len(rows), 4), np.uint32)
    L = _capi.lib()
    ctx = L.mcbrat_create(0)
    assert ctx
    try:
        rc = L.mcbrat_philox4x32_10(ctx, len(rows), inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert rc == 0, L.mcbrat_last_error(ctx)
    finally:
        L.mcbrat_destroy(ctx)
    for i, (_, _, want) in enumerate(kat):
        assert [int(v) for v in out[i]] == want
    for i, (c, k) in enumerate(extra):
        assert [int(v) for v in out[len(kat) + i]] == O.philox4x32_10(c, k)
