"""The Cox-Munk ocean surface on the host: the library's evaluator, albedo quadrature and reflection
sampler against an independent numpy statement of the model (tests/coxmunk_ref.py), the exact Lambertian limit, a stand-alone
program under the sanitizers, the refusals and the declarations.  No GPU needed, and nothing is loaded into Python under a
sanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import coxmunk_ref as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = 3
SAMPLER_CASES = [((2.0, 1.34, 0.0, 0.0), 0.6), ((2.0, 1.34, 0.0, 0.0), 0.2), ((7.0, 1.34, 0.22, 0.02), 0.6), ((7.0, 1.34, 0.22, 0.02), 0.2)]


@pytest.fixture(scope="module")
def S():
    from mcbrat3d_amd import build
    build.build()  # hipcc cross-compiles without a GPU
    from mcbrat3d_amd import surface
    return surface


def _random_pairs(rng, n):
    d_in = CM.direction(-rng.uniform(0.0, 1.0, n), rng.uniform(0, 2 * np.pi, n))
    d_out = CM.direction(rng.uniform(0.0, 1.0, n), rng.uniform(0, 2 * np.pi, n))
    return d_in, d_out


def _params(rng):
    return np.array([rng.uniform(0, 50), rng.uniform(1, 2), rng.choice([0.0, rng.uniform(0, 1)]), rng.uniform(0, 0.3)], np.float32)


# ---- 1. the evaluator ----

def test_evaluator_matches_numpy(S):
    rng = np.random.default_rng(31)
    n = 10000
    d_in, d_out = _random_pairs(rng, n)
    # every 10th pair looks into the glint: d_out within a few slope widths of the mirror direction of d_in
    spec = d_in[::10] * np.array([1.0, 1.0, -1.0]) + 0.1 * rng.normal(size=(n // 10, 3))
    spec[:, 2] = np.abs(spec[:, 2])
    d_out[::10] = spec / np.linalg.norm(spec, axis=1)[:, None]
    got, ref, floor = np.empty(n), np.empty(n), np.empty(n)
    for i in range(n):
        q = _params(rng) if i % 10 == 0 else q
        got[i] = S.brdf_reflectance(KIND, q, d_in[i], d_out[i])
        ref[i] = float(CM.reflectance(q.astype(np.float64), d_in[i], d_out[i]))
        W = CM.whitecaps(q.astype(np.float64))
        floor[i] = (1.0 - W) * q[3] + W * q[2]  # R without its glint term
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    tol = np.where(ref > 1e-3, 2e-6 * ref, 2e-6 * np.maximum(1.0, ref) + 1e-9)
    bad = ~(np.abs(got - ref) <= tol)  # (written so that a NaN is a miss)
    assert not np.any(bad), (int(bad.sum()), got[bad][:5], ref[bad][:5])
    # the glint term is exercised: a good share of the samples has R well above what whitecaps and underlight give
    glinting = ref > floor + 1e-2
    assert glinting.mean() >= 0.05 and np.sum(ref > floor + 1.0) >= 20, (glinting.mean(), np.sum(ref > floor + 1.0))


def test_reciprocity(S):
    rng = np.random.default_rng(32)
    d_in, d_out = _random_pairs(rng, 2000)
    for i in range(d_in.shape[0]):
        q = _params(rng) if i % 50 == 0 else q
        a = S.brdf_reflectance(KIND, q, d_in[i], d_out[i])
        b = S.brdf_reflectance(KIND, q, -d_out[i], -d_in[i])  # light going back along the same path
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (q, a, b)


def test_lambertian_limit_bit_for_bit(S):
    rng = np.random.default_rng(33)
    d_in, d_out = _random_pairs(rng, 500)
    for a in np.float32([0.0, 0.3, 0.123456789, 0.7, 1.0]) + np.float32(rng.uniform(0, 1e-3)):
        a = np.float32(min(a, 1.0))
        for i in range(d_in.shape[0]):
            U = np.float32(rng.uniform(0, 50))
            r = S.brdf_reflectance(KIND, np.array([U, 1.0, 0.0, a], np.float32), d_in[i], d_out[i])
            assert np.float32(r).tobytes() == a.tobytes(), (U, a, r, d_in[i], d_out[i])


# ---- 2. the albedo ----

@pytest.fixture(scope="module")
def ref_albedo():
    """rho_dh of the numpy statement by its own 400 x 800 nodes at the twelve (q, mu0) of the model's table: computed once"""
    return {(q, mu): CM.albedo(q, mu) for q, row in CM.TABLE.items() for mu in row}


def test_albedo_matches_the_finer_quadrature(S, ref_albedo):
    for (q, mu), ref in ref_albedo.items():
        assert abs(ref - CM.TABLE[q][mu]) <= 2e-6, (q, mu, ref, CM.TABLE[q][mu])  # the reference's values against the table
        got = S.brdf_albedo(KIND, np.array(q, np.float32), mu)
        # (the reference at the library's float parameters: 1.34 and 0.22 are not floats)
        ref32 = ref if all(float(np.float32(v)) == v for v in q) else CM.albedo(tuple(float(np.float32(v)) for v in q), mu)
        assert abs(got - ref32) <= 1e-5, (q, mu, got, ref32)
    got = S.brdf_albedo(KIND, np.array((0.0, 1.34, 0.0, 0.0), np.float32), 0.6)  # U = 0: the narrowest lobe
    assert abs(got - CM.albedo((0.0, float(np.float32(1.34)), 0.0, 0.0), 0.6)) <= 1e-5


# ---- 3. the sampler ----

@pytest.mark.parametrize("q,mu0", SAMPLER_CASES)
def test_sampler_mean_is_the_albedo(S, q, mu0):
    rng = np.random.default_rng(int(1000 * mu0) + int(q[0]))
    n = 10 ** 6
    u = rng.random((n, 3))
    d_in = CM.direction(-mu0, 0.7)
    d_out, w = S.brdf_sample(KIND, np.array(q, np.float32), d_in, u)
    w = w.astype(np.float64)
    rho = CM.TABLE[q][mu0]
    se = w.std(ddof=1) / np.sqrt(n)
    print("q %s mu0 %g: mean %.6f rho_dh %.6f se %.2e (%.3f %% of rho_dh) largest weight %.3f" % (q, mu0, w.mean(), rho, se, 100 * se / rho, w.max()))
    assert se < 0.01 * rho, (se, rho)
    assert abs(w.mean() - rho) <= 4.0 * se, (w.mean(), rho, se)
    assert np.all(w >= 0.0) and w.max() < 1.2  # (the sampler's point: bounded weights)
    alive = w > 0.0
    assert np.all(np.abs(np.linalg.norm(d_out[alive], axis=1) - 1.0) <= 1e-6) and np.all(d_out[alive, 2] > 0.0)
    # the library's draws are the numpy statement's, draw by draw
    d_ref, w_ref = CM.sample(tuple(float(np.float32(v)) for v in q), d_in, u)
    assert np.array_equal(alive, w_ref > 0.0)
    assert np.max(np.abs(w - w_ref)) <= 2e-6 * 1.2
    # (both sides in double; the glint component passes through two square roots and a normalisation)
    assert np.max(np.abs(d_out[alive] - d_ref[alive])) <= 1e-9


def test_sampler_lambertian_limit(S):
    rng = np.random.default_rng(35)
    u = rng.random((20000, 3))
    for a in (0.0, 0.3, 1.0):
        for mu0 in (0.9, 0.05):
            d_out, w = S.brdf_sample(KIND, np.array([5.0, 1.0, 0.0, a], np.float32), CM.direction(-mu0, 1.0), u)
            assert np.all(w == np.float32(a))
            # the Lambertian direction of (u_X, u_Y) = (u1, u2), which the host entry forms in double
            assert np.max(np.abs(d_out - CM.lambert_direction(u[:, 1], u[:, 2]))) <= 1e-12
            d_lam, w_lam = S.brdf_sample(0, np.array([a], np.float32), CM.direction(-mu0, 1.0), u)
            assert np.array_equal(d_out, d_lam) and np.array_equal(w, w_lam)


def test_sampler_leaves_the_land_models_on_the_lambertian_draw(S):
    u = np.random.default_rng(36).random((1000, 3))
    d_in = CM.direction(-0.5, 0.2)
    d_lam, _ = S.brdf_sample(0, np.array([0.5], np.float32), d_in, u)
    for kind, q in ((1, (0.3, 0.7, -0.1, 0.3)), (2, (0.3, 0.15, 0.05))):
        d_out, w = S.brdf_sample(kind, np.array(q, np.float32), d_in, u)
        assert np.array_equal(d_out, d_lam)
        assert all(w[i] == np.float32(S.brdf_reflectance(kind, q, d_in, d_out[i])) for i in range(0, 1000, 50))


# ---- 4. the header alone, plain and under the sanitizers ----

def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "coxmunk_dump.cpp")])
    return out


def test_the_header_is_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program under the undefined-behaviour and address sanitizers, which end it at the first finding, prints
    what the plain one prints: every line finite, grazing geometry, U = 0 and n = 1 included"""
    plain = subprocess.run([_compile(str(tmp_path / "coxmunk_dump"))], capture_output=True, text=True, check=True).stdout
    san = subprocess.run([_compile(str(tmp_path / "coxmunk_dump_san"), "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")],
                         capture_output=True, text=True, check=True).stdout
    assert plain == san
    lines = plain.splitlines()
    assert lines[-1] == "lines %d" % (len(lines) - 1) and len(lines) > 4000
    assert not re.search(r"nan|inf", plain, re.I)
    for line in lines:
        if line.startswith("R "):  # R >= 0, and reciprocal
            r, rr = (float(v) for v in line.split("|")[2].split())
            assert r >= 0.0 and abs(r - rr) <= 1e-6 * max(1.0, r), line
        elif line.startswith("S ") and "|" in line:
            q = [float(v) for v in line.split("|")[0].split()[1:]]
            x, y, z, f = (float(v) for v in line.split("|")[4].split())
            assert f >= 0.0 and (f == 0.0 or (z > 0.0 and abs(x * x + y * y + z * z - 1.0) <= 1e-6) or z == 0.0), line
            if q[1] == 1.0 and q[2] == 0.0:  # the Lambertian limit: the factor is a_w
                assert np.float32(f) == np.float32(q[3]), line  # (%.9g and %g both name the float)


# ---- 5. refusals and bindings ----

def test_parameter_refusals(S):
    from mcbrat3d_amd import McbratError
    from mcbrat3d_amd.surface import computeSurfaceReflectance, new_SurfaceDescription
    ok = new_SurfaceDescription([7.0, 1.34, 0.22, 0.02], model="CoxMunk")
    assert ok.kind == KIND and ok.BRDFParameters.shape == (4, 1, 1)
    for q in ([0.0, 1.0, 0.0, 0.0], [50.0, 2.0, 1.0, 0.0], [50.0, 1.0, 0.0, 1.0]):  # the bounds themselves are allowed
        new_SurfaceDescription(q, model="CoxMunk")
    bad = "Cox-Munk parameters must satisfy 0 <= U <= 50, 1 <= n <= 2, 0 <= rhoWc <= 1, 0 <= aW <= 1"
    cases = [
        (([7.0, 1.34, 0.22], "CoxMunk"), "Wrong number of parameters supplied for surface BRDF."),
        (([7.0, 1.34, 0.22, 0.02, 0.0], "CoxMunk"), "Wrong number of parameters supplied for surface BRDF."),
        (([-0.1, 1.34, 0.0, 0.0], "CoxMunk"), bad),
        (([50.1, 1.34, 0.0, 0.0], "CoxMunk"), bad),
        (([7.0, 0.99, 0.0, 0.0], "CoxMunk"), bad),
        (([7.0, 2.01, 0.0, 0.0], "CoxMunk"), bad),
        (([7.0, 1.34, -0.1, 0.0], "CoxMunk"), bad),
        (([7.0, 1.34, 1.1, 0.0], "CoxMunk"), bad),
        (([7.0, 1.34, 0.0, -0.1], "CoxMunk"), bad),
        (([7.0, 1.34, 0.0, 1.1], "CoxMunk"), bad),
        (([float("nan"), 1.34, 0.0, 0.0], "CoxMunk"), bad),
        (([2.0, 1.34, 0.0, 1.0], "CoxMunk"), "directional-hemispherical albedo above 1"),  # a white sea under its own glint
        (([0.3], "Glint"), "unknown surface BRDF model"),
    ]
    for (params, model), text in cases:
        with pytest.raises(McbratError, match=re.escape(text)):
            new_SurfaceDescription(params, model=model)
    with pytest.raises(McbratError, match="CoxMunk"):  # the unknown-model text names the models there are
        new_SurfaceDescription([0.3], model="Glint")
    # per patch: one bad patch among good ones
    q = np.tile(np.array([7.0, 1.34, 0.22, 0.02], np.float32)[:, None, None], (1, 2, 1))
    new_SurfaceDescription(q, xPosition=[0.0, 1.0, 2.0], yPosition=[0.0, 1.0], model="CoxMunk")
    q[1, 1, 0] = 2.5
    with pytest.raises(McbratError, match=re.escape(bad)):
        new_SurfaceDescription(q, xPosition=[0.0, 1.0, 2.0], yPosition=[0.0, 1.0], model="CoxMunk")
    # the library's own check says the same (mcbrat_brdf_albedo of a refused vector still evaluates; the sampler needs a known kind)
    with pytest.raises(McbratError, match="unknown surface BRDF model"):
        S.brdf_sample(4, [0.0] * 4, (0.0, 0.0, -1.0), np.zeros((1, 3)))
    # computeSurfaceReflectance goes through the evaluator
    q[1, 1, 0] = 1.0
    d = new_SurfaceDescription(q, xPosition=[0.0, 1.0, 2.0], yPosition=[0.0, 1.0], model="CoxMunk")
    mu_i, mu_r, phi_i, phi_r = 0.6, 0.55, 30.0, 40.0
    ref = float(CM.reflectance(q[:, 0, 0].astype(np.float64), CM.direction(-mu_i, np.radians(phi_i)), CM.direction(mu_r, np.radians(phi_r))))
    assert ref > 0.1 and abs(computeSurfaceReflectance(d, 0.5, 0.5, mu_i, mu_r, phi_i, phi_r) - ref) <= 2e-6 * ref
    W = CM.whitecaps((7.0, 1.0, 0.22, 0.02))
    assert abs(computeSurfaceReflectance(d, 1.5, 0.5, mu_i, mu_r, phi_i, phi_r) - ((1 - W) * 0.02 + W * 0.22)) <= 1e-7  # n = 1: no glint


def test_header_declares_and_library_exports(S):
    from mcbrat3d_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    name = "mcbrat_brdf_sample"
    assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in _capi.SYMBOLS and hasattr(L, name)
    assert len(_capi.SYMBOLS[name][1]) == 7
    decl = re.search(r"%s\s*\(([^)]*)\)" % name, header).group(1)
    assert len(decl.split(",")) == 7
    assert '"glintSampling"' in header
    brdf_h = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_brdf.h")).read()
    assert re.search(r"BRDF_COXMUNK\s*=\s*3\b", brdf_h)
    assert S.MODELS["CoxMunk"] == (3, 4)


def test_fortran_shim_maps_coxmunk(tmp_path):
    if shutil.which("amdflang") is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    text = open(src).read()
    assert re.search(r'case \("CoxMunk"\)\s*\n\s*kind = 3\b', text)
    obj = str(tmp_path / "shim.o")
    subprocess.check_call(["amdflang", "-c", src, "-o", obj], cwd=str(tmp_path))
    syms = subprocess.run(["nm", obj], capture_output=True, text=True).stdout
    assert re.search(r"T \S*setsurfacebrdf", syms) and re.search(r"U mcbrat_set_surface_brdf\b", syms)
