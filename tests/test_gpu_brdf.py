"""Surface BRDFs (RPV, Ross-Li) on the GPU.  The photon-by-photon comparison with the oracle's own statement
of the models is tests/test_gpu_brdf_oracle.py; the evidence here is

1. the Lambertian limits (RPV with k = 1, Theta = 0, rhoC = 1; Ross-Li with fVol = fGeo = 0) follow the photon histories of a
   Lambertian surface description: identical flux and absorption moments, radiance to 1e-6 (the product w_in R / pi rounds
   differently from (w_in a) / pi);
2. over vacuum every photon contributes a known amount: the radiance over a BRDF surface divided by that over a white
   Lambertian one is R(d_sun, d_view) exactly, per column too;
3. vacuum fluxes: the black-sky and white-sky albedos by quadrature;
4. a scattering slab over a BRDF surface against matrix doubling with the surface as an operator;
5. schedule independence, and 6. the refusals."""
import numpy as np
import pytest

from tests import brdf_ref as B
from tests import cases
from tests.test_analytic import HG_STREAMS, doubling_matrices, hg_slab, sampled_moments, slab

pytestmark = pytest.mark.gpu
SEED = 5150
RPV_VEG = (0.3, 0.7, -0.1, 0.3)
ROSSLI = (0.3, 0.15, 0.05)


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _rng(seed=SEED):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    return new_RandomNumberSequence(seed)


def _uniform(M, model, q, x=None, y=None):
    q = np.asarray(q, np.float32)
    if x is None:
        return M.new_SurfaceDescription(q, model=model)
    return M.new_SurfaceDescription(q, x, y, model=model)


def _run(M, case, surf, n, nb=1, mu0=0.6, phi0=30.0, stream=None, tuning=None, table=9001, mus=None, phis=None, **params):
    """(moments, reportResults, integrator's walk mode) of one call."""
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    if mus is not None:
        params.update(minForwardTableSize=1801, intensityMus=list(mus), intensityPhis=list(phis), computeIntensity=True)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=True, surfaceBDRF=surf, **params)
    integ.setTuning(**dict(dict(blockWalk=0), **(tuning or {})))
    integ.resetMoments()
    photons = stream if stream is not None else M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
    assert integ.computeRadiativeTransfer(dom, _rng(), photons, n, nb) == n * nb
    integ.synchronize()
    mom = integ.moments().copy()
    rep = integ.reportResults()
    mode = integ.walkMode()
    assert integ.badPhotons() == 0
    integ.finalize()
    return mom, rep, mode


def _unpack(case, mom, ndir=None, nord=-1):
    from mcbrat3d_amd import driver
    nx, ny, nz = (len(case[k]) - 1 for k in ("xe", "ye", "ze"))
    return driver.unpack_moments(mom, nx, ny, nz, ndir, numRecScatOrd=nord)


def _sun(mu0, phi0):
    """The Directional source's float32 propagation direction (set_solar_direction)."""
    f = np.float32
    mu = -abs(f(mu0))
    phi = f(f(phi0) * np.arccos(f(-1.0))) / f(180.0)
    s = np.sqrt(f(1.0) - mu * mu)
    return np.array([s * np.cos(phi), s * np.sin(phi), mu], np.float64)


def _view(mu, phi):
    f = np.float32
    m, p = f(mu), f(phi) * f(3.14159265358979312) / f(180.0)
    s = np.sqrt(f(1.0) - m * m)
    return np.array([s * np.cos(p), s * np.sin(p), m], np.float64)


# ---- 1. the Lambertian limits -------------------------------------------------------------------------------------------
def _lambertian_cases():
    step = cases.patchy_surface(cases.step_cloud(ssa=0.99))
    cloud = cases.patchy_surface(cases.stretched_grid_cloud())
    return [("step", step), ("cloud3d", cloud)]


@pytest.mark.parametrize("name,case", _lambertian_cases())
@pytest.mark.parametrize("orders", [False, True])
def test_lambertian_limit_is_bit_for_bit(M, name, case, orders):
    refl, x, y = case["surface"]
    lam = cases.product_surface(case)
    a = np.asarray(refl, np.float32)
    rpv = _uniform(M, "RPV", np.stack([a, np.ones_like(a), np.zeros_like(a), np.ones_like(a)]), x, y)
    rl = _uniform(M, "RossLi", np.stack([a, np.zeros_like(a), np.zeros_like(a)]), x, y)
    kw = dict(recScatOrd=True, numRecScatOrd=3) if orders else {}
    ref = _run(M, case, lam, 40000, 4, **kw)
    for surf in (rpv, rl):
        got = _run(M, case, surf, 40000, 4, **kw)
        assert not got[2]["blockWalk"]
        assert np.array_equal(got[0], ref[0]), (name, surf.model)


@pytest.mark.parametrize("rr", [False, True])
def test_lambertian_limit_radiance(M, rr):
    case = cases.patchy_surface(cases.step_cloud(ssa=0.99))
    refl, x, y = case["surface"]
    a = np.asarray(refl, np.float32)
    rpv = _uniform(M, "RPV", np.stack([a, np.ones_like(a), np.zeros_like(a), np.ones_like(a)]), x, y)
    mus, phis = [1.0, 0.7, 0.45], [0.0, 30.0, 210.0]
    kw = dict(mus=mus, phis=phis, useRussianRouletteForIntensity=rr)
    ref = _unpack(case, _run(M, case, cases.product_surface(case), 20000, 8, **kw)[0], 3)
    got = _unpack(case, _run(M, case, rpv, 20000, 8, **kw)[0], 3)
    for k in ref:
        if k not in ("totalPhotons", "batches", "intensity"):  # the photon histories are the same
            assert np.array_equal(ref[k][0], got[k][0]) and np.array_equal(ref[k][1], got[k][1]), k
    if not rr:
        assert np.allclose(got["intensity"][0], ref["intensity"][0], rtol=1e-6, atol=0.0)
    else:  # the roulette plays for R instead of 1: another random stream, the same expectation
        from mcbrat3d_amd import driver
        a_, b_ = driver.statistics(ref), driver.statistics(got)
        d = np.abs(a_["intensity"] - b_["intensity"])
        assert np.all(d <= 5.0 * np.hypot(a_["intensity_StdErr"], b_["intensity_StdErr"]) + 1e-9), d.max()


# ---- 2. vacuum: the exact radiance --------------------------------------------------------------------------------------
def _vacuum():
    return slab(0.0, 1.0, nz=4)


@pytest.mark.parametrize("mu0", [0.8, 0.35])
@pytest.mark.parametrize("model,q", [("RPV", RPV_VEG), ("RossLi", ROSSLI)])
def test_vacuum_radiance_is_the_reflectance_factor(M, mu0, model, q):
    phi0 = 40.0
    mus = [mu0, mu0, 1.0, 0.5, 0.9]
    phis = [phi0 + 180.0, phi0, 0.0, 300.0, phi0 + 170.0]  # the hot spot, the forward direction, nadir, two others
    case = _vacuum()
    n = 4096
    white = _unpack(case, _run(M, case, _uniform(M, "Lambertian", [1.0]), n, 2, mu0, phi0, mus=mus, phis=phis,
                               useRussianRouletteForIntensity=False)[0], len(mus))["intensity"][0].mean(axis=(0, 1))
    got = _unpack(case, _run(M, case, _uniform(M, model, q), n, 2, mu0, phi0, mus=mus, phis=phis,
                             useRussianRouletteForIntensity=False)[0], len(mus))["intensity"][0].mean(axis=(0, 1))
    kind = B.KINDS[model]
    ref = np.array([B.reflectance(kind, np.float32(q).astype(np.float64), _sun(mu0, phi0), _view(m, p)) for m, p in zip(mus, phis)])
    assert np.allclose(got / white, ref, rtol=1e-5, atol=0.0), (got / white, ref)


@pytest.mark.parametrize("model,q,zeta", [("RPV", RPV_VEG, 0.6), ("RossLi", ROSSLI, 0.3)])
def test_vacuum_radiance_with_the_roulette(M, model, q, zeta):
    """With the Iwabuchi roulette a view whose R is above zetaMin is still exact; one below is played for, within statistics.
    (zetaMin per model, so that both kinds of view occur: the vegetation RPV's R lies between 0.46 and 0.89 here.)"""
    mu0, phi0 = 0.6, 40.0
    mus, phis = [mu0, 1.0, 0.3, 0.8], [phi0 + 180.0, 0.0, phi0, phi0 + 90.0]
    case = _vacuum()
    kind = B.KINDS[model]
    ref = np.array([B.reflectance(kind, np.float32(q).astype(np.float64), _sun(mu0, phi0), _view(m, p)) for m, p in zip(mus, phis)])
    assert np.any(ref > zeta) and np.any(ref < zeta), ref
    n, nb = 50000, 10
    kw = dict(mus=mus, phis=phis, useRussianRouletteForIntensity=True, zetaMin=zeta)
    white = _unpack(case, _run(M, case, _uniform(M, "Lambertian", [1.0]), n, nb, mu0, phi0, **kw)[0], len(mus))["intensity"][0]
    got = _unpack(case, _run(M, case, _uniform(M, model, q), n, nb, mu0, phi0, **kw)[0], len(mus))["intensity"][0]
    ratio = got.mean(axis=(0, 1)) / white.mean(axis=(0, 1))
    exact = ref > zeta
    assert np.allclose(ratio[exact], ref[exact], rtol=1e-5, atol=0.0), (ratio, ref)
    p = ref[~exact] / zeta  # a contribution zetaMin / pi with probability R / zetaMin
    sd = zeta * np.sqrt(p * (1.0 - p) / (n * nb))
    assert np.all(np.abs(ratio[~exact] - ref[~exact]) <= 4.0 * sd), (ratio[~exact], ref[~exact], sd)


def test_vacuum_nadir_radiance_per_patch(M):
    case = _vacuum()
    L = case["xe"][-1]
    case = dict(case, xe=np.array([0.0, L / 2, L]))
    case["components"] = [dict(c, ext=np.zeros((2, 1, c["ext"].shape[2])), ssa=np.ones((2, 1, c["ext"].shape[2])),
                               pfIndex=np.ones((2, 1, c["ext"].shape[2]), np.int32)) for c in case["components"]]
    q = np.zeros((4, 2, 1), np.float32)
    q[:, 0, 0] = (0.25, 0.8, -0.2, 0.4)
    q[:, 1, 0] = (0.45, 1.3, 0.3, 0.9)
    x, y = np.array([0.0, L / 2, L]), np.array([0.0, case["ye"][-1]])
    mu0, phi0, n = 0.7, 15.0, 8192
    kw = dict(mus=[1.0], phis=[0.0], useRussianRouletteForIntensity=False)
    white = _unpack(case, _run(M, case, _uniform(M, "Lambertian", np.ones((1, 2, 1), np.float32), x, y), n, 2, mu0, phi0, **kw)[0], 1)
    got = _unpack(case, _run(M, case, _uniform(M, "RPV", q, x, y), n, 2, mu0, phi0, **kw)[0], 1)
    ratio = got["intensity"][0][:, 0, 0] / white["intensity"][0][:, 0, 0]
    ref = [B.reflectance(1, q[:, j, 0].astype(np.float64), _sun(mu0, phi0), _view(1.0, 0.0)) for j in range(2)]
    assert np.allclose(ratio, ref, rtol=1e-5, atol=0.0), (ratio, ref)


# ---- 3. vacuum fluxes: black-sky and white-sky albedo -------------------------------------------------------------------
@pytest.mark.parametrize("model,q", [("RPV", RPV_VEG), ("RossLi", ROSSLI)])
def test_vacuum_fluxes_are_the_albedos(M, model, q):
    from mcbrat3d_amd import driver
    kind = B.KINDS[model]
    qd = np.float32(q).astype(np.float64)
    case = _vacuum()
    n, nb = 500000, 20
    for src, theory in (("Directional", B.albedo(kind, qd, float(-_sun(0.6, 30.0)[2]))), ("Flux", B.white_sky_albedo(kind, qd))):
        stream = M.new_PhotonStream(0.6, 30.0, numberOfPhotons=10 ** 12) if src == "Directional" else M.new_PhotonStream(numberOfPhotons=10 ** 12)
        mom, rep, _ = _run(M, case, _uniform(M, model, q), n, nb, stream=stream)
        st = driver.statistics(_unpack(case, mom))
        assert abs(st["meanFluxDown"] - 1.0) < 1e-6
        z = (st["meanFluxUp"] - theory) / st["meanFluxUp_StdErr"]
        assert abs(z) <= 4.0, (src, st["meanFluxUp"], theory, st["meanFluxUp_StdErr"])


# ---- 4. a scattering slab over a BRDF surface against matrix doubling ---------------------------------------------------
def doubling_over_brdf(b, omega, chi, kind, q, node, streams=HG_STREAMS):
    """(mu0, flux out of the top, flux onto the surface counting every arrival) for the sun along Gauss node `node`:
    the surface as the operator S_ij = 2 pi fbar(mu_i, mu_j) mu_j c_j on azimuthally averaged intensities (fbar: the azimuthal
    mean of R / pi, mu_j incident, mu_i reflected); top r + t S (E - r S)^-1 t, onto the surface (E - r S)^-1 t."""
    mu, c, r, t = doubling_matrices(b, omega, chi, streams)
    fbar = B.azimuthal_mean(kind, q, mu[None, :] + 0.0 * mu[:, None], mu[:, None] + 0.0 * mu[None, :]) / np.pi
    S = 2.0 * np.pi * fbar * (mu * c)[None, :]
    e = np.eye(streams)
    inc = np.zeros(streams)
    inc[node] = 1.0 / (2.0 * np.pi * mu[node] * c[node])
    down = np.linalg.solve(e - r @ S, t @ inc)
    top = r @ inc + t @ S @ down
    flux = lambda v: float(2.0 * np.pi * np.sum(mu * c * v))  # noqa: E731
    return float(mu[node]), flux(top), flux(down)


SLABS = [("iso", 1.0, 0.9, 0.0), ("hg", 2.0, 0.95, 0.6)]


@pytest.mark.parametrize("slabname,b,omega,g", SLABS)
@pytest.mark.parametrize("model,q", [("RPV", RPV_VEG), ("RossLi", ROSSLI)])
def test_slab_over_brdf_against_matrix_doubling(M, slabname, b, omega, g, model, q):
    from mcbrat3d_amd import driver
    if g == 0.0:
        case, chi = slab(b, omega, nz=16), np.array([1.0])
    else:
        case, chi = hg_slab(b, omega, g, 48)
        chi = sampled_moments(chi, table=9001)
    kind = B.KINDS[model]
    mu0, up, down = doubling_over_brdf(b, omega, chi, kind, np.float32(q).astype(np.float64), 64)
    assert mu0 == 0.5
    n, nb = 10000000, 10
    mom, _, _ = _run(M, case, _uniform(M, model, q), n, nb, mu0=mu0, phi0=0.0)
    st = driver.statistics(_unpack(case, mom))
    for k, theory in (("meanFluxUp", up), ("meanFluxDown", down)):
        z = (st[k] - theory) / st[k + "_StdErr"]
        assert abs(z) <= 4.0, (k, st[k], theory, st[k + "_StdErr"])


# ---- 5. schedule independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,q", [("RPV", RPV_VEG), ("RossLi", ROSSLI)])
def test_brdf_moments_do_not_depend_on_the_schedule(M, model, q):
    case = cases.step_cloud(ssa=0.99)
    surf = _uniform(M, model, q)
    ref = _run(M, case, surf, 50000, 4)[0]
    for tuning in (dict(privateTallies=0), dict(privateTallies=1), dict(layerSkip=0), dict(layerSkip=1)):
        assert np.array_equal(_run(M, case, surf, 50000, 4, tuning=tuning)[0], ref), tuning


# ---- 6. refusals, and the way back to the domain's albedo ----------------------------------------------------------------
def test_refusals_and_return_to_the_domain_albedo(M):
    from mcbrat3d_amd import McbratError, _capi
    from mcbrat3d_amd.broadband import SpectralRun
    case = cases.homog_lw(n=6)
    dom = cases.product_domain(case)
    w = M.new_Weights(6, 6, 6)
    M.emission_weighting(dom, w, case["sfc_temp"])
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=1001, LW_flag=1.0, surfaceBDRF=_uniform(M, "RPV", RPV_VEG))
    with pytest.raises(McbratError, match="BRDF surface cannot be used with the thermal source"):
        integ.computeRadiativeTransfer(dom, _rng(), M.new_PhotonStream(theseWeights=w, numberOfPhotons=10 ** 9), 10000)
    integ.finalize()
    with pytest.raises(McbratError, match="SpectralRun: BRDF surfaces"):
        SpectralRun(M, [cases.product_domain(cases.step_cloud())], surfaceBDRF=_uniform(M, "RossLi", ROSSLI))
    # numX <= 0 returns to the domain's albedo: the moments of a run without a description
    case = cases.step_cloud(ssa=0.99)
    case["albedo"] = 0.25
    ref = _run(M, case, None, 40000, 2)[0]
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=9001, useRayTracing=True, useRussianRoulette=True,
                            surfaceBDRF=_uniform(M, "RPV", RPV_VEG))
    integ.setTuning(blockWalk=0)
    integ._check(_capi.lib().mcbrat_set_surface_brdf(integ._ctx, 1, 0, 0, None, None, 4, None))
    integ.resetMoments()
    integ.computeRadiativeTransfer(dom, _rng(), M.new_PhotonStream(0.6, 30.0, numberOfPhotons=10 ** 12), 40000, 2)
    integ.synchronize()
    got = integ.moments().copy()
    integ.finalize()
    assert np.array_equal(got, ref)

