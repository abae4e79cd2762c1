"""The Cox-Munk ocean surface and its glint sampler on the GPU.  The oracle has no BRDF, so the
evidence is that of tests/test_gpu_brdf.py, against the numpy statement of the model (tests/coxmunk_ref.py):

6. over vacuum the radiance over the surface divided by that over a white Lambertian one is R(d_sun, d_view), whichever way
   the reflected direction is drawn;
7. vacuum fluxes are the directional-hemispherical albedos;
8. the sampled and the plain estimator (option glintSampling 1 / 0) agree, and sampling is what it is for: far less noise;
9. the Lambertian limit follows a Lambertian description's photon histories bit for bit, patches mix, and the moments do not
   depend on the schedule."""
import numpy as np
import pytest

from tests import cases
from tests import coxmunk_ref as CM
from tests.test_gpu_brdf import _sun, _unpack, _vacuum, _view

pytestmark = pytest.mark.gpu
SEED = 5150
CALM = (2.0, 1.34, 0.0, 0.0)       # a glint and nothing else
ROUGH = (7.0, 1.34, 0.22, 0.02)    # glint, whitecaps, underlight
N, NB = 50000, 20                  # 10^6 photons in 20 batches


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _f32(q):
    return tuple(float(v) for v in np.float32(q))


def _ocean(M, q, x=None, y=None):
    q = np.asarray(q, np.float32)
    return M.new_SurfaceDescription(q, model="CoxMunk") if x is None else M.new_SurfaceDescription(q, x, y, model="CoxMunk")


def _run(M, case, surf, n, nb=1, mu0=0.6, phi0=30.0, glint=None, tuning=None, mus=None, phis=None, **params):
    """moments of nb batches of n photons; glint: the option glintSampling (None: the default, on)"""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    if mus is not None:
        params.update(minForwardTableSize=1801, intensityMus=list(mus), intensityPhis=list(phis), computeIntensity=True)
    integ.specifyParameters(minInverseTableSize=9001, useRayTracing=True, useRussianRoulette=True, surfaceBDRF=surf, **params)
    integ.setTuning(**dict(dict(blockWalk=0), **(tuning or {})))
    if glint is not None:
        integ.setOption(glintSampling=glint)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12), n, nb) == n * nb
    integ.synchronize()
    mom = integ.moments().copy()
    assert not integ.walkMode()["blockWalk"]
    assert integ.badPhotons() == 0
    integ.finalize()
    return mom


def _stats(case, mom, ndir=None):
    from mcbrat3d_amd import driver
    return driver.statistics(_unpack(case, mom, ndir))


# ---- 6. vacuum: the exact radiance --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0", [0.8, 0.35])
def test_vacuum_radiance_is_the_reflectance_factor(M, mu0):
    phi0 = 40.0
    mus, phis = [mu0, 1.0, 0.5], [phi0, 0.0, phi0 + 60.0]  # the specular direction, nadir, one off the principal plane
    case = _vacuum()
    kw = dict(mus=mus, phis=phis, useRussianRouletteForIntensity=False)
    white = _unpack(case, _run(M, case, M.new_SurfaceDescription(np.float32([1.0])), N, NB, mu0, phi0, **kw), 3)["intensity"][0]
    ref = np.array([CM.reflectance(_f32(ROUGH), _sun(mu0, phi0), _view(m, p)) for m, p in zip(mus, phis)])
    assert ref[0] > 3.0 * ref[1]  # (the first view does look into the glint)
    got = {}
    for glint in (0, 1):
        got[glint] = _unpack(case, _run(M, case, _ocean(M, ROUGH), N, NB, mu0, phi0, glint=glint, **kw), 3)["intensity"][0]
        ratio = got[glint] / white  # per column
        assert np.allclose(ratio, ref[None, None, :], rtol=1e-5, atol=0.0), (glint, ratio.mean(axis=(0, 1)), ref)
    assert np.array_equal(got[0], got[1])  # the estimate does not depend on the draw


# ---- 7. vacuum fluxes: the albedos --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [CALM, ROUGH])
@pytest.mark.parametrize("mu0", [0.6, 0.2])
def test_vacuum_fluxes_are_the_albedos(M, q, mu0):
    case = _vacuum()
    theory = CM.albedo(_f32(q), float(-_sun(mu0, 30.0)[2]))
    assert abs(theory - CM.TABLE[q][mu0]) <= 2e-6  # (float parameters and a float sun: the table's value still)
    st = _stats(case, _run(M, case, _ocean(M, q), N, NB, mu0))
    assert abs(st["meanFluxDown"] - 1.0) < 1e-6
    print("q %s mu0 %g: fluxUp %.6f rho_dh %.6f se %.2e" % (q, mu0, st["meanFluxUp"], theory, st["meanFluxUp_StdErr"]))
    assert st["meanFluxUp_StdErr"] < 0.01 * theory
    z = (st["meanFluxUp"] - theory) / st["meanFluxUp_StdErr"]
    assert abs(z) <= 4.0, (st["meanFluxUp"], theory, st["meanFluxUp_StdErr"])


# ---- 8. the sampled estimator against the plain one -----------------------------------------------------------------------
def test_vacuum_sampled_against_plain(M):
    case = _vacuum()
    a, b = (_stats(case, _run(M, case, _ocean(M, ROUGH), N, NB, 0.6, glint=g)) for g in (0, 1))
    d, se = abs(a["meanFluxUp"] - b["meanFluxUp"]), np.hypot(a["meanFluxUp_StdErr"], b["meanFluxUp_StdErr"])
    assert d <= 4.0 * se, (a["meanFluxUp"], b["meanFluxUp"], se)


def test_sampling_cuts_the_noise_at_low_sun(M):
    case = _vacuum()
    plain, sampled = (_stats(case, _run(M, case, _ocean(M, CALM), N, NB, 0.2, glint=g)) for g in (0, 1))
    ratio = plain["meanFluxUp_StdErr"] / sampled["meanFluxUp_StdErr"]
    print("batch standard error of fluxUp: plain %.3e sampled %.3e ratio %.1f" % (plain["meanFluxUp_StdErr"], sampled["meanFluxUp_StdErr"], ratio))
    assert ratio >= 5.0, (plain["meanFluxUp_StdErr"], sampled["meanFluxUp_StdErr"])


def test_step_cloud_sampled_against_plain(M):
    case = cases.step_cloud(ssa=0.99)
    kw = dict(mus=[1.0], phis=[0.0])
    a, b = (_stats(case, _run(M, case, _ocean(M, ROUGH), N, NB, 0.6, glint=g, **kw), 1) for g in (0, 1))
    worst = {}
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "intensity"):
        for name in (k, "mean" + k[0].upper() + k[1:]):
            if name == "meanIntensity":  # (no domain mean in the moments: that of the columns)
                d = abs(a[k].mean() - b[k].mean())
                se = np.hypot(np.sqrt(np.sum(a[k + "_StdErr"] ** 2)), np.sqrt(np.sum(b[k + "_StdErr"] ** 2))) / a[k].size
            else:
                d, se = np.abs(a[name] - b[name]), np.hypot(a[name + "_StdErr"], b[name + "_StdErr"])
            z = np.where(d == 0.0, 0.0, d / np.maximum(se, 1e-300))
            worst[name] = float(np.max(z))
    assert max(worst.values()) <= 4.0, "largest |z| per quantity (columns, then the domain mean): %s" % worst


# ---- 9. limits and neighbours -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orders", [False, True])
def test_lambertian_limit_is_bit_for_bit(M, orders):
    case = cases.patchy_surface(cases.step_cloud(ssa=0.99))
    refl, x, y = case["surface"]
    a = np.asarray(refl, np.float32)
    ocean = _ocean(M, np.stack([np.full_like(a, 5.0), np.ones_like(a), np.zeros_like(a), a]), x, y)
    kw = dict(recScatOrd=True, numRecScatOrd=3) if orders else {}
    ref = _run(M, case, cases.product_surface(case), 40000, 4, **kw)
    for glint in (1, 0):
        assert np.array_equal(_run(M, case, ocean, 40000, 4, glint=glint, **kw), ref), glint


def test_mixed_patches_nadir_radiance(M):
    case = _vacuum()
    L = case["xe"][-1]
    case = dict(case, xe=np.array([0.0, L / 2, L]))
    case["components"] = [dict(c, ext=np.zeros((2, 1, c["ext"].shape[2])), ssa=np.ones((2, 1, c["ext"].shape[2])),
                               pfIndex=np.ones((2, 1, c["ext"].shape[2]), np.int32)) for c in case["components"]]
    q = np.zeros((4, 2, 1), np.float32)
    q[:, 0, 0] = ROUGH                     # glinting
    q[:, 1, 0] = (12.0, 1.0, 0.3, 0.05)    # n = 1: whitecaps and underlight, no glint
    x, y = np.array([0.0, L / 2, L]), np.array([0.0, case["ye"][-1]])
    mu0, phi0, n = 0.7, 15.0, 8192
    kw = dict(mus=[1.0], phis=[0.0], useRussianRouletteForIntensity=False)
    white = _unpack(case, _run(M, case, M.new_SurfaceDescription(np.ones((1, 2, 1), np.float32), x, y), n, 2, mu0, phi0, **kw), 1)
    got = _unpack(case, _run(M, case, _ocean(M, q, x, y), n, 2, mu0, phi0, **kw), 1)
    ratio = got["intensity"][0][:, 0, 0] / white["intensity"][0][:, 0, 0]
    ref = [float(CM.reflectance(q[:, j, 0].astype(np.float64), _sun(mu0, phi0), _view(1.0, 0.0))) for j in range(2)]
    assert np.allclose(ratio, ref, rtol=1e-5, atol=0.0), (ratio, ref)


@pytest.mark.parametrize("glint", [1, 0])
def test_moments_do_not_depend_on_the_schedule(M, glint):
    case = cases.step_cloud(ssa=0.99)
    surf = _ocean(M, ROUGH)
    ref = _run(M, case, surf, 50000, 4, glint=glint)
    for tuning in (dict(privateTallies=0), dict(privateTallies=1), dict(layerSkip=0), dict(layerSkip=1)):
        assert np.array_equal(_run(M, case, surf, 50000, 4, glint=glint, tuning=tuning), ref), tuning
