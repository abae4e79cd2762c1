"""The block walk's instantiation without periodic folds inside blocks (NOSPAN) traces every photon as
the general one does, and only media none of whose blocks spans a periodic axis get it.

Tallies are fixed point, so "as the general one does" is equality of the moment arrays bit for bit: the library's own choice
against the general instantiation forced by the option "blockSpanKernel".  Run on the MI355X box with `-m gpu`."""
import numpy as np
import pytest

from tests import cases
from tests.golden import make_blockwalk_moments as G
from tests.test_block_decomposition import decompose
from tests.test_blockwalk_exact_steps import three_layers_middle_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def run(M, make, mu0, phi0, rr, ppb, nb, block_walk, span_kernel):
    """tests/golden/make_blockwalk_moments.py:run with the option blockSpanKernel, and the dropped photons besides."""
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
    integ.setOption(blockSpanKernel=span_kernel)
    photons = M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
    integ.resetMoments()
    done = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(G.SEED), photons, ppb, nb)
    mom = integ.moments().copy()
    walk = integ.walkMode()
    bad = integ.badPhotons()
    integ.finalize()
    assert done == ppb * nb
    assert bad == 0
    assert walk["blockWalk"]
    return mom, walk


def both(M, make, mu0, phi0, rr, ppb, nb, block_walk):
    auto, walk = run(M, make, mu0, phi0, rr, ppb, nb, block_walk, 0)
    general, walk1 = run(M, make, mu0, phi0, rr, ppb, nb, block_walk, 1)
    assert not walk1["foldsCompiledOut"]
    assert auto.shape == general.shape
    assert np.array_equal(auto, general)
    assert np.any(auto != 0)
    return walk["foldsCompiledOut"]


def simple_case(name, ext, ssa=0.98, albedo=0.3, cell=0.0625):
    """Equally spaced axes (a power of two: regular by the reference's own single-precision test), one component."""
    nx, ny, nz = ext.shape
    return dict(name=name, xe=cell * np.arange(nx + 1), ye=cell * np.arange(ny + 1), ze=cell * np.arange(nz + 1),
                components=[dict(ext=ext, ssa=np.where(ext > 0, ssa, 0.0), pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=[cases.hg_legendre(0.8, 24)])], albedo=albedo)


def checkerboard():
    """4 x 2 x 4 cells, the extinction a checkerboard in x-y: faces on both horizontal axes, no block spans either."""
    ext = np.zeros((4, 2, 4))
    ext[...] = np.where((np.arange(4)[:, None, None] + np.arange(2)[None, :, None]) % 2 == 0, 4.0, 12.0)
    return simple_case("checkerboard", ext)


# the grazing sun is the one that found the third block-walk hang: nearly every leg wraps through the domain edge
STEP_SUNS = [("overhead", 1.0, 0.0, 100000, 4), ("sun60", 0.5, 30.0, 50000, 3), ("grazing", 0.08, 0.0, 20011, 3)]


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("sun", STEP_SUNS, ids=[s[0] for s in STEP_SUNS])
def test_step_cloud_default_equals_the_general_kernel(M, sun):
    _, mu0, phi0, ppb, nb = sun
    assert both(M, lambda: cases.step_cloud(0.99), mu0, phi0, True, ppb, nb, -1)


@pytest.mark.timeout(300, method="thread")
def test_three_dimensional_medium_without_spanning_block(M):
    (sx, sy) = [bool(np.any(decompose(checkerboard()["components"][0]["ext"])[1][:, 6] & b)) for b in (1, 2)]
    assert not sx and not sy
    assert both(M, checkerboard, 0.35, 40.0, True, 20011, 3, 2)


SPANNING = [("slab", lambda: simple_case("slab", np.full((8, 1, 8), 5.0))),
            ("three_layers", lambda: simple_case("threeLayers", three_layers_middle_split()))]


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("medium", SPANNING, ids=[m[0] for m in SPANNING])
def test_media_with_a_spanning_block_keep_the_general_kernel(M, medium):
    ext = medium[1]()["components"][0]["ext"]
    assert np.any(decompose(ext)[1][:, 6] & 1)
    assert not both(M, medium[1], 0.35, 40.0, True, 20011, 3, 2)


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("seed", (1, 4, 7))
def test_random_box_media_flag_follows_the_records(M, seed):
    """(their moments have a recorded yardstick: tests/test_gpu_blockwalk_lean.py)"""
    from tests.test_gpu_block_walk import random_box_case
    ext = random_box_case(seed)[0]["components"][0]["ext"]
    flags = decompose(ext)[1][:, 6]
    no_span = not np.any(flags & 1) and (ext.shape[1] == 1 or not np.any(flags & 2))
    assert both(M, seed, None, None, None, 20011, 3, 2) == no_span
