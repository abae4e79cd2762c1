"""The solar photon sources RandomAzimuth, Flux and Spotlight (new_PhotonStream, src/monteCarloIllumination.f95:103-216) on
the GPU.  The oracle has no such sources, so

1. the launch is pinned photon by photon: over a wide, nearly transparent slab every unscattered photon lands in the
   column a numpy mirror of its launch predicts (Philox4x32-10 on the photon's event-0 counter, the float32 uniforms and
   direction algebra of solar_launch, mcbrat_photon.h), on a regular and on an irregular x/y grid, on both walks;
2. the two walks agree photon by photon on the step cloud, as they do for the Directional source;
3. the physics is held to transport theory with the solvers of tests/test_analytic.py: isotropic incidence over an
   absorbing slab (2 E3), over Henyey-Greenstein slabs (matrix doubling) and its reflected radiance; a random azimuth
   (Beer-Lambert, the isotropic slab's integral equation); a spotlight over a homogeneous periodic slab (domain means as
   for the Directional source);
4. bookkeeping: closure over scattering orders, no dropped photons, a change of source on one integrator, and moments
   that do not depend on batch split or tuning."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import expn

from tests import cases
from tests.test_analytic import (HG_SLABS, HG_STREAMS, _sigma, doubling_matrices, hg_slab, isotropic_slab, sampled_moments,
                                 slab)

pytestmark = pytest.mark.gpu
SEED = 4242


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def _rng(seed=SEED):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    return new_RandomNumberSequence(seed)


def _stream(M, kind, mu0=0.6, phi0=30.0, x=0.3, y=0.7, n=10 ** 12):
    if kind == "Directional":
        return M.new_PhotonStream(mu0, phi0, numberOfPhotons=n)
    if kind == "RandomAzimuth":
        return M.new_PhotonStream(mu0, numberOfPhotons=n)
    if kind == "Flux":
        return M.new_PhotonStream(numberOfPhotons=n)
    return M.new_PhotonStream(mu0, phi0, solarX=x, solarY=y, numberOfPhotons=n)


# ---- the numpy mirror of the launch -------------------------------------------------------------------------------------
_MASK = np.uint64(0xFFFFFFFF)


def philox(ctr, key):
    """Philox4x32-10 on arrays of counters (4 uint32 each) under one key (2 uint32)."""
    c = [np.asarray(v, np.uint64) & _MASK for v in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _MASK, (k1 + np.uint64(0xBB67AE85)) & _MASK
    return [v.astype(np.uint32) for v in c]


def u01(u):
    return np.asarray(u, np.uint32).astype(np.float32) * np.float32(2.3283064365386963e-10)


def mirror_launch(kind, n, seed, mu0=0.6, phi0=30.0, x=0.3, y=0.7):
    """Launch fractions (fx, fy, float64) and direction cosines (float32) of photons 0..n-1 of the stream `seed`."""
    f32 = np.float32
    ids = np.arange(n, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros(n, np.uint64)
    r = philox([zero, zero, ids & _MASK, ids >> np.uint64(32)], key)
    if kind == "Spotlight":  # the host's direction (mcbrat_set_source_spotlight) and one point
        mu = -abs(f32(mu0))
        phi = f32(f32(phi0) * f32(np.arccos(f32(-1.0)))) / f32(180.0)
        st = np.sqrt(f32(1.0) - mu * mu)
        d = np.array([st * np.cos(phi), st * np.sin(phi), mu], np.float32)
        return np.full(n, float(f32(x))), np.full(n, float(f32(y))), np.tile(d[:, None], (1, n))
    fx, fy = u01(r[0]).astype(np.float64), u01(r[1]).astype(np.float64)
    if kind == "RandomAzimuth":
        mu = np.full(n, -abs(f32(mu0)), np.float32)
        u_phi = u01(r[2])
    else:  # Flux
        u = u01(r[2])
        redo = np.nonzero(u == 0.0)[0]  # (probability 2^-32 per photon: drawn again from block 1)
        for i in redo:
            b = philox([np.array([0]), np.array([1]), ids[i:i + 1] & _MASK, ids[i:i + 1] >> np.uint64(32)], key)
            u[i] = next(v for v in u01(np.concatenate(b)) if v > 0.0)
        mu = -np.sqrt(u)
        u_phi = u01(r[3])
    st = np.sqrt(f32(1.0) - mu * mu)
    phi = 2.0 * np.pi * u_phi.astype(np.float64)  # (sincos_2pi: within an ulp of the float32 cosines)
    return fx, fy, np.array([st * np.cos(phi).astype(np.float32), st * np.sin(phi).astype(np.float32), mu], np.float32)


# ---- 1. launch, photon by photon ----------------------------------------------------------------------------------------
def transparent_slab(irregular):
    """16 x 16 columns of about 1 km, 0.1 km thick, tau 1e-7, black surface."""
    if irregular:
        xe = np.concatenate([[0.0], np.cumsum(0.55 * 1.07 ** np.arange(16))])
        ye = np.concatenate([[0.0], np.cumsum(1.4 * 0.94 ** np.arange(16))])
    else:
        xe = np.arange(17, dtype=np.float64)
        ye = np.arange(17, dtype=np.float64)
    ze = np.array([0.0, 0.05, 0.1])
    ext = np.full((16, 16, 2), 1e-6)
    return dict(name="transparent", xe=xe, ye=ye, ze=ze, albedo=0.0,
                components=[dict(ext=ext, ssa=np.full_like(ext, 0.5), pfIndex=np.ones(ext.shape, np.int32),
                                 legendre=[cases.hg_legendre(0.0, 2)])])


@pytest.mark.parametrize("kind", ["RandomAzimuth", "Flux", "Spotlight"])
@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("blockWalk", [0, 2])
def test_every_unscattered_photon_lands_where_its_launch_says(M, kind, irregular, blockWalk):
    n = 50000
    case = transparent_slab(irregular)
    xe, ye = case["xe"], case["ye"]
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=1001, useRayTracing=True, useRussianRoulette=True)
    integ.setTuning(blockWalk=blockWalk)
    photons = _stream(M, kind)
    f = integ.traceFates(dom, _rng(), photons, n)
    assert integ.walkMode()["blockWalk"] == bool(blockWalk)  # (the plan of the loaded domain)
    assert integ.badPhotons() == 0
    integ.finalize()
    fx, fy, d = mirror_launch(kind, n, SEED)
    lx, ly = xe[-1] - xe[0], ye[-1] - ye[0]
    zl = float(np.float32(1.0) - np.float32(1.1920929e-07)) * 0.1  # the launch height (mcbrat_api.hip, set_solar_launch)
    path = zl / np.abs(d[2].astype(np.float64))
    x = xe[0] + np.mod(fx * lx + path * d[0], lx)
    y = ye[0] + np.mod(fy * ly + path * d[1], ly)
    ix = np.clip(np.searchsorted(xe, x, side="right") - 1, 0, 15) + 1
    iy = np.clip(np.searchsorted(ye, y, side="right") - 1, 0, 15) + 1
    edge = np.minimum(np.min(np.abs(x[:, None] - xe[None, :]), axis=1), np.min(np.abs(y[:, None] - ye[None, :]), axis=1))
    direct = (f["fate"] == 1) & (f["nScatter"] == 1)  # (absorbed by the black surface: its reflection counts as the first order)
    assert direct.mean() > 0.999
    check = direct & (np.abs(d[2]) >= 0.05) if kind == "Flux" else direct
    miss = check & ((f["ix"] != ix) | (f["iy"] != iy))
    assert miss.sum() <= 5 and np.all(edge[miss] < 1e-4), (miss.sum(), edge[miss][:10])
    if kind == "Spotlight":
        assert len(set(zip(ix.tolist(), iy.tolist()))) == 1
        assert np.all(f["ix"][direct] == ix[0]) and np.all(f["iy"][direct] == iy[0])
    else:  # the launch covers the domain: every column is hit
        assert len(set(zip(f["ix"][direct].tolist(), f["iy"][direct].tolist()))) == 256
    if kind == "Flux":  # isotropic incidence: the cosines are sqrt(U), so |mu|^2 is uniform
        assert abs(float(np.mean(d[2].astype(np.float64) ** 2)) - 0.5) < 0.01


# ---- 2. the walks agree -------------------------------------------------------------------------------------------------
def _same(a, b):
    return (a["fate"] == b["fate"]) & (a["ix"] == b["ix"]) & (a["iy"] == b["iy"]) & (a["iz"] == b["iz"]) & \
        (a["nScatter"] == b["nScatter"]) & (np.abs(a["weight"] - b["weight"]) <= 1e-6)


@pytest.mark.parametrize("kind", ["RandomAzimuth", "Flux", "Spotlight"])
def test_block_walk_and_face_by_face_walk_agree(M, kind):
    n = 200000
    case = cases.step_cloud(0.99)
    out = []
    for bw in (1, 0):
        dom = cases.product_domain(case)
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001, useRayTracing=True, useRussianRoulette=True)
        integ.setTuning(blockWalk=bw)
        assert bool(integ.walkMode()["blockWalk"]) == bool(bw)
        out.append(integ.traceFates(dom, _rng(), _stream(M, kind, mu0=0.7, phi0=20.0, x=0.4, y=0.5), n))
        assert integ.badPhotons() == 0
        integ.finalize()
    assert np.all(out[0]["fate"] >= 0) and np.all(out[1]["fate"] >= 0)
    assert _same(out[0], out[1]).mean() > 0.999, _same(out[0], out[1]).mean()


# ---- 3. physics ---------------------------------------------------------------------------------------------------------
def _fluxes(M, case, kind, n, table=101, mu0=0.6, phi0=30.0, x=0.3, y=0.7, **params):
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=table, useRayTracing=True, useRussianRoulette=True, **params)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, _rng(), _stream(M, kind, mu0, phi0, x, y), n) == n
    r = integ.reportResults()
    assert integ.badPhotons() == 0
    integ.finalize()
    return r


@pytest.mark.parametrize("tau", [0.3, 1.0, 3.0])
def test_isotropic_incidence_on_an_absorbing_slab_is_2E3(M, tau):
    n = 1000000
    r = _fluxes(M, slab(tau, 0.0), "Flux", n)
    t = 2.0 * float(expn(3, tau))
    assert r["meanFluxUp"] == 0.0
    assert abs(r["meanFluxDown"] - t) < 4.5 * _sigma(t, n) + 1e-6
    assert abs(r["meanFluxAbsorbed"] - (1.0 - t)) < 4.5 * _sigma(t, n) + 1e-6


def diffuse_incidence_doubling(b, omega, chi):
    """(reflected, transmitted) share of an isotropic incident field (intensity 1/pi: unit flux) by matrix doubling:
    2 sum mu c (r 1), 2 sum mu c (t_diffuse 1) + 2 E3(b)."""
    mu, c, r, t = doubling_matrices(b, omega, chi, HG_STREAMS)
    one = np.ones(len(mu))
    diffuse = t - np.diag(np.exp(-b / mu))
    return 2.0 * float(np.sum(mu * c * (r @ one))), 2.0 * float(np.sum(mu * c * (diffuse @ one))) + 2.0 * float(expn(3, b))


@pytest.mark.parametrize("b,omega,g,nleg,node", HG_SLABS)
def test_isotropic_incidence_on_henyey_greenstein_slabs_against_matrix_doubling(M, b, omega, g, nleg, node):
    n = 4000000
    case, chi = hg_slab(b, omega, g, nleg)
    up, down = diffuse_incidence_doubling(b, omega, sampled_moments(chi, table=9001))
    r = _fluxes(M, case, "Flux", n, table=9001)
    assert abs(r["meanFluxUp"] - up) < 6.0 * _sigma(up, n), (r["meanFluxUp"], up)  # (test_analytic's bound for doubling)
    assert abs(r["meanFluxDown"] - down) < 6.0 * _sigma(down, n), (r["meanFluxDown"], down)


def test_reflected_radiance_under_isotropic_incidence(M):
    """An isotropically scattering slab: the radiance leaving the top along Gauss nodes is (r 1) / pi in every azimuth."""
    from mcbrat3d_amd import driver
    b, omega, streams = 1.0, 0.9, 33
    mu, c, r, _ = doubling_matrices(b, omega, [1.0], streams)
    nodes = [32, 28, 24, 20]
    theory = (r @ np.ones(streams))[nodes] / np.pi
    mus = [float(np.float32(mu[k])) for k in nodes]
    phis = [0.0, 100.0, 200.0, 300.0]
    case = slab(b, omega, nz=16)
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=9001, minForwardTableSize=1801, intensityMus=mus, intensityPhis=phis,
                            computeIntensity=True)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, _rng(), _stream(M, "Flux"), 100000, 40) == 4000000
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ, len(mus)))
    assert integ.badPhotons() == 0
    integ.finalize()
    mean, err = st["intensity"][0, 0, :], st["intensity_StdErr"][0, 0, :]
    assert np.all(err < 0.01 * theory)
    assert np.all(np.abs(mean - theory) < 4.5 * err), (mean, theory, err)


@pytest.mark.parametrize("tau,mu0", [(0.5, 1.0), (2.0, 0.5)])
def test_random_azimuth_beer_lambert(M, tau, mu0):
    n = 1000000
    r = _fluxes(M, slab(tau, 0.0), "RandomAzimuth", n, mu0=mu0)
    t = float(np.exp(-tau / mu0))
    assert r["meanFluxUp"] == 0.0
    assert abs(r["meanFluxDown"] - t) < 4.5 * _sigma(t, n) + 1e-6


@pytest.mark.parametrize("b,omega,mu0", [(1.0, 1.0, 0.6), (2.0, 0.9, 0.35)])
def test_random_azimuth_isotropic_slab(M, b, omega, mu0):
    n = 4000000
    r = _fluxes(M, slab(b, omega, nz=16), "RandomAzimuth", n, table=9001, mu0=mu0)
    up, down, direct = isotropic_slab(b, omega, mu0)
    assert abs(r["meanFluxUp"] - up) < 6.0 * _sigma(up, n)  # (test_analytic's bound for the integral equation)
    assert abs(r["meanFluxDown"] - (down + direct)) < 6.0 * _sigma(down + direct, n)


def periodic_slab(b, omega, n=8):
    """A homogeneous slab over n x n columns of a periodic 0.5 km domain: a spotlight on it has the domain means of the
    Directional source."""
    pp = slab(b, omega, nz=16)
    ext = np.broadcast_to(pp["components"][0]["ext"], (n, n, 16)).copy()
    case = dict(pp, xe=np.linspace(0.0, 0.5, n + 1), ye=np.linspace(0.0, 0.5, n + 1))
    case["components"] = [dict(pp["components"][0], ext=ext, ssa=np.full_like(ext, omega), pfIndex=np.ones(ext.shape, np.int32))]
    return case


@pytest.mark.parametrize("b,omega,mu0", [(1.0, 0.9, 0.6), (0.5, 0.0, 0.8)])
def test_spotlight_domain_means_are_the_directional_theory(M, b, omega, mu0):
    n = 4000000
    r = _fluxes(M, periodic_slab(b, omega), "Spotlight", n, table=9001, mu0=mu0, phi0=50.0, x=0.3, y=0.8)
    up, down, direct = isotropic_slab(b, omega, mu0)
    assert abs(r["meanFluxUp"] - up) < 6.0 * _sigma(up, n) + 1e-6
    assert abs(r["meanFluxDown"] - (down + direct)) < 6.0 * _sigma(down + direct, n)
    # the light is where the spot sends it: the direct beam lands in one column, 0.25 km tan(theta) from the entry point
    fd = r["fluxDown"]
    assert float(fd.max()) > 10.0 * float(np.median(fd))
    assert float(fd.max()) > 0.9 * direct * fd.size


# ---- 4. bookkeeping -----------------------------------------------------------------------------------------------------
def test_flux_orders_sum_to_the_totals(M):
    case = cases.plane_parallel(ssa=0.5, tau=0.5, nz=8, g=0.0, nleg=2)
    r = _fluxes(M, case, "Flux", 200000, recScatOrd=True, numRecScatOrd=60)
    for k in ("fluxUp", "fluxDown"):
        s = r[k + "ByScatOrd"].astype(np.float64).sum(axis=-1)
        assert np.allclose(s, r[k], rtol=2e-5, atol=1e-7), k
        mk = "mean" + k[0].upper() + k[1:]
        assert abs(r[mk + "ByScatOrd"].astype(np.float64).sum() - r[mk]) < 1e-5
    # order 0 going down is the direct beam of isotropic incidence: 2 E3(tau)
    t0 = 2.0 * float(expn(3, 0.5))
    assert abs(float(r["meanFluxDownByScatOrd"][0]) - t0) < 4.5 * _sigma(t0, 200000)
    assert r["meanFluxUpByScatOrd"][0] == 0.0


def _moments(M, integ, dom, kind, ppb=20000, nb=3, calls=1):
    """nb batches of ppb photons, in `calls` calls: the moment array."""
    integ.resetMoments()
    photons, rng = _stream(M, kind), _rng()
    for _ in range(calls):
        integ.computeRadiativeTransfer(dom, rng, photons, ppb, nb // calls)
    assert integ.badPhotons() == 0
    return integ.moments().copy()


def test_a_change_of_source_on_one_integrator_gives_the_fresh_bits(M):
    case = cases.step_cloud(0.99)
    dom = cases.product_domain(case)
    fresh = {}
    for kind in ("Directional", "Flux", "RandomAzimuth", "Spotlight"):
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001)
        fresh[kind] = _moments(M, integ, dom, kind)
        integ.finalize()
    assert not np.array_equal(fresh["Directional"], fresh["RandomAzimuth"])  # (same mu0: the azimuth is drawn)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001)
    for kind in ("Directional", "Flux", "Directional", "RandomAzimuth", "Spotlight", "Flux", "Directional"):
        assert np.array_equal(_moments(M, integ, dom, kind), fresh[kind]), kind
    integ.finalize()


def test_the_library_refuses_what_the_reference_refuses(M):
    """The C ABI validates by itself (the Fortran shim calls it directly), with the reference's messages."""
    dom = cases.product_domain(cases.step_cloud(0.99))
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=101)
    integ.prepare(dom, _stream(M, "Directional"))
    L, ctx = integ._lib, integ._ctx
    f = C.c_float
    for call, msg in ((lambda: L.mcbrat_set_source_random_azimuth(ctx, f(0.0)), "solarMu out of bounds"),
                      (lambda: L.mcbrat_set_source_random_azimuth(ctx, f(1.5)), "solarMu out of bounds"),
                      (lambda: L.mcbrat_set_source_spotlight(ctx, f(0.5), f(400.0), f(0.5), f(0.5)), "solarAzimuth out of bounds"),
                      (lambda: L.mcbrat_set_source_spotlight(ctx, f(-2.0), f(10.0), f(0.5), f(0.5)), "solarMu out of bounds"),
                      (lambda: L.mcbrat_set_source_spotlight(ctx, f(0.5), f(10.0), f(0.0), f(0.5)), "x and y positions must be between 0 and 1"),
                      (lambda: L.mcbrat_set_source_spotlight(ctx, f(0.5), f(10.0), f(0.5), f(1.5)), "x and y positions must be between 0 and 1"),
                      (lambda: L.mcbrat_set_source_spotlight(ctx, f(0.5), f(10.0), f(-0.5), f(0.5)), "x and y positions must be between 0 and 1")):
        assert call() != 0 and msg in L.mcbrat_last_error(ctx).decode(), msg
    assert L.mcbrat_set_source_flux(ctx) == 0
    assert L.mcbrat_set_source_spotlight(ctx, f(0.5), f(10.0), f(1.0), f(1.0)) == 0
    integ.finalize()


# (walk, its base tuning, other tunings): the schedules of tests/test_gpu_tunings.py, fixed
WALKS = [
    ("face by face", dict(layerSkip=0, blockWalk=0), dict(eventThreshold=16, privateTallies=0, brickLayout=0),
     [dict(eventThreshold=4, launchThreshold=1, blockSize=256, privateTallies=1, brickLayout=1),
      dict(eventThreshold=40, surfaceThreshold=32, blocksPerCU=1, maxBatchesInFlight=1, blockSize=0, privateTallies=4)]),
    ("layers + flight", dict(layerSkip=3, blockWalk=0, privateTallies=0, brickLayout=0), dict(eventThreshold=16),
     [dict(eventThreshold=4, launchThreshold=1, blockSize=512), dict(eventThreshold=40, surfaceThreshold=32, blocksPerCU=1,
                                                                    maxBatchesInFlight=1, blockSize=256)]),
    ("block walk", dict(blockWalk=2), dict(eventThreshold=16),
     [dict(eventThreshold=4, launchThreshold=1, surfaceThreshold=1, privateTallies=4),
      dict(eventThreshold=64, launchThreshold=32, blocksPerCU=3, maxBatchesInFlight=2, privateTallies=6)]),
]


@pytest.mark.parametrize("kind", ["RandomAzimuth", "Flux", "Spotlight"])
@pytest.mark.parametrize("name,walk,base,tunings", WALKS)
def test_moments_do_not_depend_on_batch_split_or_tuning(M, kind, name, walk, base, tunings):
    case = cases.step_cloud(0.99)
    dom = cases.product_domain(case)

    def run(tuning, calls=1):
        integ = M.new_Integrator(dom)
        integ.specifyParameters(minInverseTableSize=10001)
        integ.setTuning(**{**walk, **tuning})
        m = _moments(M, integ, dom, kind, calls=calls)
        integ.finalize()
        return m

    ref = run(base)
    assert np.array_equal(run(base, calls=3), ref), name
    for tuning in tunings:
        assert np.array_equal(run(tuning), ref), (name, tuning)


# ---- 5. the large-grid plan ---------------------------------------------------------------------------------------------
# Dense grid in global memory, global tallies, layer-skipping walk with the clear-air flight, roulette, two components:
# where a Directional run takes a walk-specialised SPEC kernel (landsatLike128, radarLike).  The SPEC kernels launch the
# Directional source only, so the plan must send the other kinds to the general kernel.  Each kind on that plan is held
# to the same kind on an unrelated plan (face-by-face walk, no layer skipping), column by column, and must differ from the
# Directional photons the SPEC kernel would have launched in its place.
SPEC_PLAN = dict(layerSkip=3, blockWalk=0, privateTallies=0, brickLayout=0, blockSize=256)
REF_PLAN = dict(layerSkip=0, blockWalk=0)


def _stats(M, dom, tuning, photons, ppb=50000, nb=20):
    from mcbrat3d_amd import driver
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=10001, useRayTracing=True, useRussianRoulette=True)
    integ.setTuning(**tuning)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, _rng(), photons, ppb, nb) == ppb * nb
    mode = integ.walkMode()  # (the plan of the loaded domain)
    st = driver.statistics(driver.unpack_moments(integ.moments(), dom.numX, dom.numY, dom.numZ))
    assert integ.badPhotons() == 0
    integ.finalize()
    return mode, st


def _chi2(a, b, key):
    """Mean over columns of the squared difference in units of its standard error (about 1 for one distribution)."""
    d = a[key] - b[key]
    v = a[key + "_StdErr"] ** 2 + b[key + "_StdErr"] ** 2
    use = v > 0
    return float(np.mean(d[use] ** 2 / v[use]))


@pytest.mark.parametrize("kind", ["RandomAzimuth", "Flux", "Spotlight"])
def test_new_kinds_on_the_large_grid_plan(M, kind):
    case = cases.landsat_like(n=32, nz=24)
    dom = cases.product_domain(case)
    mu0, phi0 = 0.6, 30.0
    photons = _stream(M, kind, mu0=mu0, phi0=phi0, x=0.4, y=0.6)
    mode, got = _stats(M, dom, SPEC_PLAN, photons)
    assert mode["layerSkip"] and mode["clearAirFlight"] and not mode["privateTallies"] and not mode["blockWalk"], mode
    mode, ref = _stats(M, dom, REF_PLAN, photons)
    assert not mode["clearAirFlight"]
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        se = float(np.hypot(got[k + "_StdErr"], ref[k + "_StdErr"]))
        assert abs(float(got[k]) - float(ref[k])) < 5.0 * se + 1e-7, (k, got[k], ref[k], se)
    for k in ("fluxUp", "fluxDown"):
        assert _chi2(got, ref, k) < 1.6, (k, _chi2(got, ref, k))
    # what the SPEC kernel would have traced instead: Directional photons along the launch direction the host set
    standIn = M.new_PhotonStream(1.0, 0.0, numberOfPhotons=10 ** 12) if kind == "Flux" else \
        M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12)
    _, wrong = _stats(M, dom, SPEC_PLAN, standIn)
    assert _chi2(got, wrong, "fluxDown") > 5.0, _chi2(got, wrong, "fluxDown")
