"""The block walk's instantiation with a black surface and the parallel sun compiled into its exit and launch phases (RARE,
DESIGN.md section 4.5) traces every photon as the general one does, and only runs that are of that kind get it.

Tallies are fixed point, so "as the general one does" is equality of the whole moment array bit for bit: the library's own
choice against the general exit and launch phases forced by the option "blockRareKernel".  Run on the MI355X box with `-m gpu`."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

SEED = 2718
RARE = "blackSurfaceSunCompiledIn"


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def run(M, case, photons, ppb, nb, general, surface=None):
    """-> the moment array and walkMode() of one run; general: the option blockRareKernel"""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, useRayTracing=True, useRussianRoulette=True, surfaceBDRF=surface)
    integ.setTuning(blockWalk=2)  # (forced: the small media below have fewer than four cells per block)
    integ.setOption(blockRareKernel=general)
    integ.resetMoments()
    done = integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, ppb, nb)
    mom = integ.moments().copy()
    walk = integ.walkMode()  # (after the run: the source is part of the choice)
    bad = integ.badPhotons()
    integ.finalize()
    assert done == ppb * nb
    assert bad == 0
    assert walk["blockWalk"]
    return mom, walk


def both(M, case, photons, ppb, nb, surface=None):
    """the library's choice against the general phases: the same moments bit for bit -> whether the choice was RARE"""
    auto, walk = run(M, case, photons, ppb, nb, 0, surface)
    general, walk1 = run(M, case, photons, ppb, nb, 1, surface)
    assert not walk1[RARE]
    assert walk1["foldsCompiledOut"] == walk["foldsCompiledOut"]  # (the option changes the rare phases, nothing else)
    assert auto.shape == general.shape
    assert np.array_equal(auto, general)
    assert np.any(auto != 0)
    return walk[RARE]


def sun(M, mu0=1.0, phi0=0.0):
    return M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)


def test_step_cloud_default_equals_the_general_phases(M):
    """32 x 1 x 32, the smallest domain the plan picks this kernel for; 4 batches of 5 x 10^4: launch-wide units cross batch
    boundaries and both LDS slabs are used"""
    assert both(M, cases.step_cloud(0.99), sun(M), 50000, 4)


def slab(tau=(0.1, 0.1), albedo=0.0, ssa=1.0, cell=0.0625):
    """2 x 1 x 2 cells, conservative, the optical depth of each column given: nearly every photon reaches the surface with
    weight exactly 1.  (Equally spaced axes, a power of two: regular by the reference's own single-precision test.)"""
    ext = np.empty((2, 1, 2))
    ext[0], ext[1] = tau[0] / (2 * cell), tau[1] / (2 * cell)
    return dict(name="slab2x2", xe=cell * np.arange(3), ye=cell * np.arange(2), ze=cell * np.arange(3),
                components=[dict(ext=ext, ssa=np.where(ext > 0, ssa, 0.0), pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=[cases.hg_legendre(0.8, 24)])], albedo=albedo)


def test_thin_slab_nearly_every_photon_exits_through_the_surface(M):
    """the homogeneous slab is ONE block, which spans x: the folds stay (NOSPAN does not apply) and with them the general phases --
    the comparison holds trivially (the next test cuts the slab in two so that the new kernel runs it)"""
    assert not both(M, slab(), sun(M), 20000, 1)


def test_thin_slab_of_two_unlike_columns(M):
    """the same slab with columns of optical depth 0.1 and 0.05: two blocks, neither spans x -- this one runs the new kernel"""
    assert both(M, slab(tau=(0.1, 0.05)), sun(M), 20000, 1)


def test_thin_slab_of_two_unlike_columns_under_a_grazing_sun(M):
    """exits land on block and domain edges, where the forced fold and the clamp decide the column"""
    assert both(M, slab(tau=(0.1, 0.05)), sun(M, 0.08, 0.0), 20000, 1)
    assert both(M, slab(tau=(0.1, 0.05)), sun(M, 0.08, 180.0), 20000, 1)


def vacuum_corner(ssa_there):
    """the unlike columns with vacuum in the upper cell of the first one, whose single-scattering albedo is given"""
    case = slab(tau=(0.1, 0.05))
    comp = case["components"][0]
    comp["ext"][0, 0, 1] = 0.0
    comp["ssa"][0, 0, 1] = ssa_there
    return case


# what must yield the general instantiation, each one change away from a run that gets RARE
PICKER_ROWS = [
    ("albedo_1e-30", lambda M: (slab(tau=(0.1, 0.05), albedo=1e-30), sun(M), None), False),
    ("albedo_0_with_surface_description", lambda M: (slab(tau=(0.1, 0.05)), sun(M), M.new_SurfaceDescription([0.0])), False),
    ("random_azimuth_source", lambda M: (slab(tau=(0.1, 0.05)), M.new_PhotonStream(0.5, numberOfPhotons=10 ** 12), None), False),
    ("flux_source", lambda M: (slab(tau=(0.1, 0.05)), M.new_PhotonStream(numberOfPhotons=10 ** 12), None), False),
    ("one_NaN_in_the_albedos", lambda M: (vacuum_corner(np.nan), sun(M), None), False),
    ("no_NaN_in_the_albedos", lambda M: (vacuum_corner(0.0), sun(M), None), True),
    ("albedo_minus_0", lambda M: (slab(tau=(0.1, 0.05), albedo=-0.0), sun(M), None), True),
]


@pytest.mark.parametrize("row", PICKER_ROWS, ids=[r[0] for r in PICKER_ROWS])
def test_the_pickers_rows(M, row):
    _, make, want = row
    case, photons, surface = make(M)
    assert both(M, case, photons, 5000, 2, surface) == want
