"""The solar photon sources RandomAzimuth, Flux and Spotlight (new_PhotonStream, src/monteCarloIllumination.f95:103-216),
the parts that need no GPU: the overload resolution, the reference's validation messages, the C ABI's new names and the
Fortran shim's new entries.  The launches themselves are pinned on the GPU (tests/test_gpu_sources.py)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


def test_overload_resolves_by_the_arguments_given(M):
    p = M.new_PhotonStream(0.5, 30.0, numberOfPhotons=10)
    assert p.kind == "Directional" and (p.solarMu, p.solarAzimuth) == (0.5, 30.0)
    p = M.new_PhotonStream(0.5, numberOfPhotons=10)
    assert p.kind == "RandomAzimuth" and p.solarMu == 0.5
    p = M.new_PhotonStream(-0.3, numberOfPhotons=10)  # (the reference takes -abs(solarMu))
    assert p.kind == "RandomAzimuth" and p.solarMu == -0.3
    p = M.new_PhotonStream(numberOfPhotons=10)
    assert p.kind == "Flux" and p.numberOfPhotons == 10
    p = M.new_PhotonStream(0.8, 120.0, solarX=0.25, solarY=1.0, numberOfPhotons=10)
    assert p.kind == "Spotlight" and (p.solarMu, p.solarAzimuth, p.solarX, p.solarY) == (0.8, 120.0, 0.25, 1.0)
    # randomNumbers= is accepted, as in the reference's argument lists, and changes nothing: photons come from the GPU
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    p = M.new_PhotonStream(numberOfPhotons=7, randomNumbers=new_RandomNumberSequence(3))
    assert p.kind == "Flux" and p.numberOfPhotons == 7 and p.morePhotonsExist()


def test_emission_form_is_unchanged(M):
    w = M.new_Weights(2, 2, 2)
    with pytest.raises(M.McbratError, match="weights have not been computed"):
        M.new_PhotonStream(theseWeights=w, numberOfPhotons=10)
    w.voxelWeights = np.linspace(0.1, 1.0, 8)
    assert M.new_PhotonStream(theseWeights=w, numberOfPhotons=10).kind == "BBEmission"
    p = M.new_PhotonStream(0.5, 30.0, theseWeights=w, numberOfPhotons=10)  # (the geometry is ignored, as before)
    assert p.kind == "BBEmission" and p.weights is w


@pytest.mark.parametrize("args,kw,msg", [
    ((), dict(numberOfPhotons=-1), "must ask for non-negative number of photons"),
    ((0.5,), dict(numberOfPhotons=-1), "must ask for non-negative number of photons"),
    ((0.5, 10.0), dict(solarX=0.5, solarY=0.5, numberOfPhotons=-1), "must ask for non-negative number of photons"),
    ((0.0,), dict(numberOfPhotons=10), "solarMu out of bounds"),
    ((1.5,), dict(numberOfPhotons=10), "solarMu out of bounds"),
    ((-1.01,), dict(numberOfPhotons=10), "solarMu out of bounds"),
    ((1e-40,), dict(numberOfPhotons=10), "solarMu out of bounds"),
    ((0.0, 10.0), dict(solarX=0.5, solarY=0.5, numberOfPhotons=10), "solarMu out of bounds"),
    ((0.5, -1.0), dict(solarX=0.5, solarY=0.5, numberOfPhotons=10), "solarAzimuth out of bounds"),
    ((0.5, 360.5), dict(solarX=0.5, solarY=0.5, numberOfPhotons=10), "solarAzimuth out of bounds"),
    ((0.5, 10.0), dict(solarX=0.0, solarY=0.5, numberOfPhotons=10), "x and y positions must be between 0 and 1"),
    ((0.5, 10.0), dict(solarX=0.5, solarY=1.0001, numberOfPhotons=10), "x and y positions must be between 0 and 1"),
    ((0.5, 10.0), dict(solarX=-0.5, solarY=0.5, numberOfPhotons=10), "x and y positions must be between 0 and 1"),  # deviation
    ((0.5, 10.0), dict(solarX=0.5, solarY=-0.25, numberOfPhotons=10), "x and y positions must be between 0 and 1"),
    ((0.5, 10.0), dict(solarX=0.5, numberOfPhotons=10), "a spotlight needs"),
    ((0.5,), dict(solarX=0.5, solarY=0.5, numberOfPhotons=10), "a spotlight needs"),
    ((), dict(solarAzimuth=10.0, numberOfPhotons=10), "solarAzimuth needs solarMu"),
])
def test_every_validation_message(M, args, kw, msg):
    with pytest.raises(M.McbratError, match=msg):
        M.new_PhotonStream(*args, **kw)


def test_the_mirror_generator_is_philox():
    """tests/test_gpu_sources.py mirrors each photon's launch in numpy: its Philox4x32-10 against the oracle's."""
    from oracle import oracle as O
    from tests.test_gpu_sources import philox
    rng = np.random.default_rng(3)
    ctr = [rng.integers(0, 2 ** 32, 64, dtype=np.uint64) for _ in range(4)]
    key = (0x9ABCDEF1, 0x12345)
    got = philox(ctr, key)
    for i in range(64):
        assert [int(v[i]) for v in got] == O.philox4x32_10([int(c[i]) for c in ctr], key)


def test_spotlight_accepts_the_closed_end_of_the_interval(M):
    for x, y in ((1.0, 1.0), (1e-6, 0.5), (np.float32(0.3), np.float32(0.7))):
        assert M.new_PhotonStream(1.0, 0.0, solarX=x, solarY=y, numberOfPhotons=1).kind == "Spotlight"


def test_integrator_token_carries_the_kind_and_its_parameters():
    """A Directional stream and a Flux stream (or a RandomAzimuth one with the same solarMu) must not share a token:
    the integrator would keep the previous source uploaded."""
    from mcbrat3d_amd import integrator
    import mcbrat3d_amd as M
    calls = []

    class FakeLib:
        def __getattr__(self, name):
            def f(ctx, *args):
                calls.append((name, tuple(float(a.value) for a in args)))
                return 0
            return f

    integ = integrator.Integrator.__new__(integrator.Integrator)
    integ._lib, integ._ctx, integ._source_token, integ._loaded_weights = FakeLib(), None, None, None
    integ._check = lambda rc: None
    streams = [M.new_PhotonStream(0.5, 0.0, numberOfPhotons=1), M.new_PhotonStream(0.5, numberOfPhotons=1),
               M.new_PhotonStream(numberOfPhotons=1), M.new_PhotonStream(0.5, 0.0, solarX=0.5, solarY=0.5, numberOfPhotons=1),
               M.new_PhotonStream(0.5, 0.0, solarX=0.5, solarY=0.25, numberOfPhotons=1),
               M.new_PhotonStream(0.5, 0.0, numberOfPhotons=1)]
    for s in streams:
        integ._load_source(s)
        integ._load_source(s)  # the same source again: no upload
    assert calls == [("mcbrat_set_source_solar", (0.5, 0.0)), ("mcbrat_set_source_random_azimuth", (0.5,)),
                     ("mcbrat_set_source_flux", ()), ("mcbrat_set_source_spotlight", (0.5, 0.0, 0.5, 0.5)),
                     ("mcbrat_set_source_spotlight", (0.5, 0.0, 0.5, 0.25)), ("mcbrat_set_source_solar", (0.5, 0.0))]


def test_the_library_exports_the_new_source_functions():
    from mcbrat3d_amd import build, _capi
    build.build()
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    for name in ("mcbrat_set_source_random_azimuth", "mcbrat_set_source_flux", "mcbrat_set_source_spotlight"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _capi.SYMBOLS and hasattr(L, name), name


def test_fortran_shim_declares_the_source_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("setRandomAzimuthSource", "setFluxSource", "setSpotlightSource"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
        assert re.search(r"subroutine %s\b" % name, text), name
    for sym in ("mcbrat_set_source_random_azimuth", "mcbrat_set_source_flux", "mcbrat_set_source_spotlight"):
        assert 'name="%s"' % sym in text
