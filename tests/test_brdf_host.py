"""Surface BRDFs on the host: the library's one evaluator against an independent numpy statement of the
formulas (tests/brdf_ref.py), its exact Lambertian limits, reciprocity, the albedo quadrature, the refusals of the Python mirror
and the C ABI / Fortran shim declarations.  No GPU needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import brdf_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    from mcbrat3d_amd import build
    build.build()  # hipcc cross-compiles without a GPU
    from mcbrat3d_amd import surface
    return surface


def _random_pairs(rng, n):
    mu_i = rng.uniform(0.0, 1.0, n)
    mu_r = rng.uniform(0.0, 1.0, n)
    d_in = B.direction(-mu_i, rng.uniform(0, 2 * np.pi, n))
    d_out = B.direction(mu_r, rng.uniform(0, 2 * np.pi, n))
    return d_in, d_out


def _params(rng, kind):
    if kind == 1:
        return np.array([rng.uniform(0, 1), rng.uniform(0.2, 2), rng.uniform(-0.95, 0.95), rng.uniform(0, 1)], np.float32)
    return np.array([rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 0.5)], np.float32)


@pytest.mark.parametrize("kind", [1, 2])
def test_evaluator_matches_numpy(S, kind):
    rng = np.random.default_rng(11 + kind)
    n = 10000
    d_in, d_out = _random_pairs(rng, n)
    worst = 0.0
    for i in range(n):
        q = _params(rng, kind) if i % 100 == 0 else q
        got = S.brdf_reflectance(kind, q, d_in[i], d_out[i])
        ref = float(B.reflectance(kind, q.astype(np.float64), d_in[i], d_out[i]))
        if ref > 1e-3:
            worst = max(worst, abs(got - ref) / ref)
        else:
            assert abs(got - ref) <= 2e-6 * max(1.0, ref) + 1e-9, (kind, q, d_in[i], d_out[i], got, ref)
    assert worst <= 2e-6, worst


def test_ross_li_kernels_vanish_at_nadir(S):
    down, up = np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, 1.0])
    # R = fIso + fVol Kvol + fGeo Kgeo: with fIso = 0 and one unit weight R is that kernel (clamped at 0), so compare both signs
    # through fIso = 1 as well
    for q in ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        assert abs(S.brdf_reflectance(2, np.array(q, np.float32), down, up)) <= 1e-7
        r = S.brdf_reflectance(2, np.array((1.0,) + q[1:], np.float32), down, up)
        assert abs(r - 1.0) <= 1e-7, (q, r)


@pytest.mark.parametrize("kind", [1, 2])
def test_reciprocity(S, kind):
    rng = np.random.default_rng(5 + kind)
    d_in, d_out = _random_pairs(rng, 2000)
    for i in range(d_in.shape[0]):
        q = _params(rng, kind) if i % 50 == 0 else q
        a = S.brdf_reflectance(kind, q, d_in[i], d_out[i])
        b = S.brdf_reflectance(kind, q, -d_out[i], -d_in[i])  # light going back along the same path
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (kind, q, a, b)


def test_lambertian_limits_bit_for_bit(S):
    rng = np.random.default_rng(3)
    d_in, d_out = _random_pairs(rng, 500)
    for a in np.float32([0.0, 0.3, 0.123456789, 0.7, 1.0]) + np.float32(rng.uniform(0, 1e-3)):
        a = np.float32(min(a, 1.0))
        for i in range(d_in.shape[0]):
            r1 = S.brdf_reflectance(1, np.array([a, 1.0, 0.0, 1.0], np.float32), d_in[i], d_out[i])
            r2 = S.brdf_reflectance(2, np.array([a, 0.0, 0.0], np.float32), d_in[i], d_out[i])
            assert np.float32(r1).tobytes() == a.tobytes() and np.float32(r2).tobytes() == a.tobytes(), (a, r1, r2)


@pytest.mark.parametrize("kind,q", [(1, (0.3, 0.7, -0.1, 0.3)), (1, (0.5, 1.4, 0.6, 0.0)), (2, (0.3, 0.15, 0.05)),
                                    (2, (0.1, 1.0, 0.3)), (1, (0.3, 1.0, 0.0, 1.0))])
def test_albedo_matches_numpy_quadrature(S, kind, q):
    q = np.array(q, np.float32)
    for mu in (0.05, 0.1, 0.37, 0.5, 0.8, 1.0):
        got = S.brdf_albedo(kind, q, mu)
        ref = B.albedo(kind, q.astype(np.float64), mu)
        assert abs(got - ref) <= 1e-5, (kind, q, mu, got, ref)


def test_parameter_and_energy_refusals(S):
    from mcbrat3d_amd import McbratError
    from mcbrat3d_amd.surface import new_SurfaceDescription
    ok = new_SurfaceDescription([0.3, 0.7, -0.1, 0.3], model="RPV")
    assert ok.kind == 1 and ok.BRDFParameters.shape == (4, 1, 1)
    assert new_SurfaceDescription([0.3, 0.15, 0.05], model="RossLi").kind == 2
    assert new_SurfaceDescription([0.3]).kind == 0
    cases = [
        (([0.3, 0.7, -0.1], "RPV"), "Wrong number of parameters supplied for surface BRDF."),
        (([1.2, 1.0, 0.0, 1.0], "RPV"), "RPV parameters must satisfy"),
        (([0.3, 0.1, 0.0, 1.0], "RPV"), "RPV parameters must satisfy"),
        (([0.3, 1.0, 0.96, 1.0], "RPV"), "RPV parameters must satisfy"),
        (([0.3, 1.0, 0.0, -0.1], "RPV"), "RPV parameters must satisfy"),
        (([0.3, -0.01, 0.0], "RossLi"), "Ross-Li kernel weights must not be negative"),
        (([1.0, 1.0, 0.0, 0.0], "RPV"), "directional-hemispherical albedo above 1"),  # rhoC = 0: a white surface with a hot spot
        (([0.9, 0.5, 0.0], "RossLi"), "directional-hemispherical albedo above 1"),
        (([0.3], "Glint"), "unknown surface BRDF model"),
    ]
    for (params, model), text in cases:
        with pytest.raises(McbratError, match=re.escape(text)):
            new_SurfaceDescription(params, model=model)
    # per patch: one bad patch among good ones
    q = np.tile(np.array([0.3, 0.15, 0.05], np.float32)[:, None, None], (1, 2, 1))
    q[1, 1, 0] = -1.0
    with pytest.raises(McbratError, match="Ross-Li kernel weights must not be negative"):
        new_SurfaceDescription(q, xPosition=[0.0, 1.0, 2.0], yPosition=[0.0, 1.0], model="RossLi")
    # the Lambertian path and its texts are as they were
    with pytest.raises(McbratError, match="surface reflectance must be between 0 and 1"):
        new_SurfaceDescription([1.5])


def test_compute_surface_reflectance_angles(S):
    from mcbrat3d_amd.surface import computeSurfaceReflectance, new_SurfaceDescription
    q = np.zeros((4, 2, 1), np.float32)
    q[:, 0, 0] = (0.2, 0.8, -0.3, 0.5)  # (Theta < 0: backward scattering, with the hot spot)
    q[:, 1, 0] = (0.4, 1.0, 0.0, 1.0)
    d = new_SurfaceDescription(q, xPosition=[0.0, 1.0, 2.0], yPosition=[0.0, 1.0], model="RPV")
    mu_i, mu_r, phi_i, phi_r = 0.6, 0.8, 30.0, 250.0
    d_in = B.direction(-mu_i, np.radians(phi_i))
    d_out = B.direction(mu_r, np.radians(phi_r))
    ref = float(B.reflectance(1, q[:, 0, 0].astype(np.float64), d_in, d_out))
    assert abs(computeSurfaceReflectance(d, 0.5, 0.5, mu_i, mu_r, phi_i, phi_r) - ref) <= 2e-6 * ref
    assert abs(computeSurfaceReflectance(d, 2.5, 0.5, mu_i, mu_r, phi_i, phi_r) - ref) <= 2e-6 * ref  # periodic
    assert computeSurfaceReflectance(d, 1.5, 0.5, mu_i, mu_r, phi_i, phi_r) == np.float32(0.4)
    # exact backscatter is the hot spot: the largest R among the azimuths
    hot = computeSurfaceReflectance(d, 0.5, 0.5, mu_i, mu_i, phi_i, phi_i + 180.0)
    assert all(hot >= computeSurfaceReflectance(d, 0.5, 0.5, mu_i, mu_i, phi_i, phi_i + a) for a in range(0, 360, 10))


def test_header_declares_and_library_exports(S):
    from mcbrat3d_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    for name in ("mcbrat_set_surface_brdf", "mcbrat_brdf_reflectance", "mcbrat_brdf_albedo"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _capi.SYMBOLS and hasattr(L, name), name


def test_fortran_shim_binds_set_surface_brdf(tmp_path):
    if shutil.which("amdflang") is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    text = open(src).read()
    assert re.search(r"public ::[^!]*\bsetSurfaceBRDF\b", text.replace("&\n", " "))
    assert re.search(r'bind\(C, name="mcbrat_set_surface_brdf"\)', text)
    obj = str(tmp_path / "shim.o")
    subprocess.check_call(["amdflang", "-c", src, "-o", obj], cwd=str(tmp_path))
    syms = subprocess.run(["nm", obj], capture_output=True, text=True).stdout
    assert re.search(r"T \S*setsurfacebrdf", syms) and re.search(r"U mcbrat_set_surface_brdf\b", syms)
