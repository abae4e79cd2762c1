"""The flux through the vertical faces of every cell (recSideFluxes), the parts that need no GPU:

1. the tally layout with the side part (tests/side_layout_dump.cpp, a program of its own), against the program that knows nothing
   of it (tests/tally_layout_dump.cpp) and against the formulas of the definition;
2. the moment layout the host unpacks, the statistics, the NetCDF writer, both namelist parsers, the declarations of every layer;
3. the ray-cast helper of tests/side_cases.py, on which tests/test_gpu_side_flux.py leans photon by photon."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from tests import level_cases as LC
from tests import side_cases as SC
from tests import test_tally_layout_host as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = SC.MEANS + SC.NAMES


# 1 ---------------------------------------------------------------------------------------------------------------------------
def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "side_layout_dump.cpp")])
    return out


def _dump(exe, shapes, side, budget=TL.BUDGET):
    return TL._dump(exe, [s + (side,) for s in shapes], budget)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("side_layout")
    return _compile(str(d / "side_layout_dump")), TL._compile(str(d / "tally_layout_dump"))


SIDE_FIELDS = ("slabSide", "momSide", "scalSide")


def test_without_the_side_part_every_field_is_unchanged(exes):
    new, old = exes
    assert len(TL.SHAPES) == 90
    for budget in (TL.BUDGET, 8 * 60, 8 * 200):
        shapes = TL.SHAPES + TL.NEAR
        for s, d, o in zip(shapes, _dump(new, shapes, 0, budget), TL._dump(old, shapes, budget)):
            assert {k: v for k, v in d.items() if k not in SIDE_FIELDS} == o, (s, budget)
            # an empty part starts where the forward pass has got to: the end
            assert (d["slabSide"], d["momSide"], d["scalSide"]) == (d["slabStride"], d["momentsLen"], d["scalPerBatch"]), s


def test_with_the_side_part_the_new_starts_and_lengths_are_the_formulas(exes):
    new, old = exes
    for s, d, o in zip(TL.SHAPES, _dump(new, TL.SHAPES, 1), TL._dump(old, TL.SHAPES)):
        nx, ny, nz = s[:3]
        ncol = nx * ny
        # the three new starts: behind everything there was; the three lengths: 4 ncol nz bins, 4 nz (1 + ncol) moments, 4 nz scalars
        assert (d["slabSide"], d["momSide"], d["scalSide"]) == (o["slabStride"], o["momentsLen"], o["scalPerBatch"]), s
        assert d["slabStride"] == o["slabStride"] + 4 * ncol * nz, s
        assert d["momentsLen"] == o["momentsLen"] + 4 * nz * (1 + ncol), s
        assert d["scalPerBatch"] == o["scalPerBatch"] + 4 * nz, s
        assert d["fluxRunStride"] == o["fluxRunStride"] + 4 * ncol * nz, s
        # every older start stays, and the part a workgroup may keep in LDS
        moved = SIDE_FIELDS + ("slabStride", "momentsLen", "scalPerBatch", "fluxRunStride", "fitGlobalBins", "fitStride", "verdict")
        assert {k: v for k, v in d.items() if k not in moved} == {k: v for k, v in o.items() if k not in moved}, s
        assert d["slabLds"] == o["slabLds"], s


def test_the_side_starts_trace_kernel_computes_for_itself(exes):
    """trace_kernel: sideBins = lvlDown + ncol (nz + 1), part q (x plus, x minus, y plus, y minus) at sideBins + q ncol nz -- the
    SIDE instantiations are flux runs with level fluxes, without orders, the direct tally and the actinic flux."""
    new, _ = exes
    seen = 0
    for s, d in zip(TL.SHAPES, _dump(new, TL.SHAPES, 1)):
        p = TL.Parent(*s)
        if p.levels_on() and not p.direct_on() and not p.actinic_on() and p.nDir == 0 and not p.orders_on():
            assert (d["slabLevels"], d["slabLevels"] + p.ncol * p.nLvl()) == (p.t_lvlUp(), p.t_lvlDown()), s
            assert d["slabSide"] == p.t_lvlDown() + p.ncol * (p.nz + 1), s
            assert d["slabStride"] == d["slabSide"] + 4 * p.ncol * p.nz, s  # (sidePart = ncol nz, four of them)
            seen += 1
    assert seen == 2  # (one and two components)


def test_the_budget_counts_the_side_part(exes):
    """8192 x 8192 columns (tests/test_gpu_side_flux.py): two level parts of 3 levels are 3 GiB and fit, with the four side parts
    of 2 layers (4 GiB) they do not; on one layer 2 + 2 GiB are exactly the budget."""
    new, _ = exes
    shapes = [(8192, 8192, 2, 1, 0, 0, -1, 1, 0, 0), (8192, 8192, 1, 1, 0, 0, -1, 1, 0, 0), (8192, 8192, 1, 1, 0, 0, -1, 0, 0, 0)]
    assert [d["fitGlobalBins"] for d in _dump(new, shapes, 0)] == [1, 1, 1]
    assert [d["fitGlobalBins"] for d in _dump(new, shapes, 1)] == [0, 1, 1]
    for budget in (TL.BUDGET, 8 * 60, 8 * 200):
        for s, d in zip(TL.SHAPES, _dump(new, TL.SHAPES, 1, budget)):
            assert d["fitGlobalBins"] == ((d["slabStride"] - d["slabLds"]) * 8 <= budget), (s, budget)
            assert d["fitStride"] == (d["slabStride"] * 8 <= budget), (s, budget)


def test_shapes_that_would_overflow_do_not_fit_and_do_not_overflow(tmp_path):
    """The saturating shapes of tests/test_tally_layout_host.py with the side part, and 2^30 cells with it alone: under the
    undefined-behaviour and address sanitizers, which end the program at the first finding (a stand-alone program)."""
    exe = _compile(str(tmp_path / "side_layout_dump_san"), "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
    big = 2 ** 31 - 1
    shapes = [(32768, 32768, 1, 1, big, 0, big - 1, 0, 0, 0), (32768, 32768, 1, 2, big, 1, big - 1, 1, 1, 1),
              (1024, 1024, 1024, 1, 2, 1, 2, 1, 1, 1), (2 ** 30, 1, 1, 8, big, 1, big - 1, 1, 1, 1), (big, big, big, 1, 0, 0, -1, 1, 0, 0)]
    for side in (0, 1):
        dumps = _dump(exe, shapes, side)
        for d in dumps:
            assert d["verdict"] == "does not fit" and not d["fitStride"]
        assert [d["fitOrders"] for d in dumps] == [0, 0, 1, 0, 0]  # (the last: every part in front of the orders is saturated already)
    assert all(d["verdict"] == "fits" for d in _dump(exe, TL.SHAPES[:10], 1))


# 2 ---------------------------------------------------------------------------------------------------------------------------
def _buffer(nx, ny, nz, nDir, quantities=2, side=True):
    """A moment array whose S1 holds its own offsets 0, 1, 2, ... and whose S2 holds them + 0.5."""
    ncol = nx * ny
    M = 3 + 3 * ncol + nz + ncol * nz + nDir * ncol + quantities * (nz + 1) * (1 + ncol) + (4 * nz * (1 + ncol) if side else 0)
    buf = np.zeros(8 + 2 * M)
    buf[0], buf[1] = 12345.0, 7.0
    buf[8:8 + M] = np.arange(M)
    buf[8 + M:] = np.arange(M) + 0.5
    return buf, M


@pytest.mark.parametrize("nDir", [0, 2])
@pytest.mark.parametrize("quantities", [2, 4])
def test_unpack_moments_finds_the_side_tail_behind_every_other(nDir, quantities, exes):
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    ncol, nLvl = nx * ny, nz + 1
    buf, M = _buffer(nx, ny, nz, nDir, quantities)
    kw = dict(levelFluxes=True, directLevelFluxes=quantities == 4)
    # where the header puts the tail
    d = _dump(exes[0], [(nx, ny, nz, 1, nDir, 0, -1, 1, int(quantities == 4), 0)], 1)[0]
    assert d["momentsLen"] == M
    S = d["momSide"]
    assert S == M - 4 * nz * (1 + ncol)
    for given in (nDir, None):  # the number of directions given, or told by the length
        out = driver.unpack_moments(buf, nx, ny, nz, nDirections=given, sideFluxes=True, **kw)
        for q, (name, mean) in enumerate(zip(SC.NAMES, SC.MEANS)):
            assert np.array_equal(out[mean][0], S + q * nz + np.arange(nz)) and np.array_equal(out[mean][1], S + q * nz + np.arange(nz) + 0.5)
            a = out[name][0]
            assert a.shape == (nx, ny, nz)
            for ix in range(nx):
                for iy in range(ny):
                    for k in range(nz):  # part slowest, then layer, x fastest
                        assert a[ix, iy, k] == S + 4 * nz + q * ncol * nz + (k * ny + iy) * nx + ix
        assert out["sideFluxYMinus"][0][nx - 1, ny - 1, nz - 1] == M - 1  # the last entry of the array
        T = S - quantities * nLvl * (1 + ncol)  # the older tails are where they are without the setting
        assert np.array_equal(out["meanLevelFluxUp"][0], T + np.arange(nLvl)) and T == d["momLevels"]
        old_buf = np.concatenate([buf[:8 + S], buf[8 + M:8 + M + S]])
        old = driver.unpack_moments(old_buf, nx, ny, nz, nDirections=given, **kw)
        assert set(out) == set(old) | set(NEW)
        for k, v in old.items():
            assert np.array_equal(np.asarray(out[k]), np.asarray(v)), k


def test_unpack_moments_refuses_what_does_not_fit():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, _ = _buffer(nx, ny, nz, 0)
    with pytest.raises(ValueError):  # a buffer without the side tail
        driver.unpack_moments(_buffer(nx, ny, nz, 0, side=False)[0], nx, ny, nz, nDirections=0, levelFluxes=True, sideFluxes=True)
    with pytest.raises(ValueError):  # a buffer with it, unpacked without the keyword
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True)
    with pytest.raises(ValueError):  # one double short
        driver.unpack_moments(buf[:-1], nx, ny, nz, nDirections=0, levelFluxes=True, sideFluxes=True)
    with pytest.raises(ValueError, match="sideFluxes needs levelFluxes"):
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, sideFluxes=True)


def test_sideFluxes_off_gives_exactly_the_old_dictionaries():
    from mcbrat3d_amd import driver
    from tests.test_actinic_host import _buffer as old_buffer
    nx, ny, nz = 3, 2, 4
    for quantities, nDir, actinic in ((0, 0, False), (0, 2, False), (2, 0, False), (4, 0, False), (2, 0, True), (0, 0, True)):
        buf, _ = old_buffer(nx, ny, nz, nDir, quantities, actinic=actinic)
        kw = dict(levelFluxes=quantities >= 2, directLevelFluxes=quantities == 4, actinicFlux=actinic)
        a = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, **kw)
        b = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, sideFluxes=False, **kw)
        assert list(a) == list(b) and not any(k in a for k in NEW)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]))
        sa, sb = driver.statistics(a, 2.0), driver.statistics(b, 2.0)
        assert list(sa) == list(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)


def test_statistics_returns_the_side_keys():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, M = _buffer(nx, ny, nz, 0)
    st = driver.statistics(driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True, sideFluxes=True), solarFlux=2.0)
    for name, mean in zip(SC.NAMES, SC.MEANS):
        assert st[name].shape == st[name + "_StdErr"].shape == (nx, ny, nz) and st[mean].shape == st[mean + "_StdErr"].shape == (nz,)
    assert st["meanSideFluxXPlus"][0] == 2.0 * (M - 4 * nz * (1 + nx * ny)) / 12345.0


class _FakeIntegrator:
    """What driver.run asks of an integrator, for a one-rank run that traces nothing."""
    numRecScatOrd, recLevelFluxes, recDirectLevelFluxes, recActinicFlux, recSideFluxes, _dims = -1, True, False, False, True, (3, 2, 4)

    def resetMoments(self):
        pass

    def computeRadiativeTransfer(self, *a):
        pass

    def numIntensityDirections(self):
        return 0

    def moments(self):
        return _buffer(3, 2, 4, 0)[0]


def test_driver_run_carries_the_setting():
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.illumination import new_PhotonStream
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    st = driver.run(_FakeIntegrator(), None, new_PhotonStream(0.5, 0.0, numberOfPhotons=10), 5, 2, new_RandomNumberSequence(1))
    assert all(k in st and k + "_StdErr" in st for k in NEW) and "levelFluxUp" in st


def test_namelist_reads_reportSideFluxes(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&output reportLevelFluxes = .true. reportSideFluxes = .true. /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["reportsidefluxes"] is True and cfg["reportlevelfluxes"] is True and cfg["reportactinicflux"] is False
    nml.write_text("&output reportLevelFluxes = .true. /\n")
    assert driver_cli.read_namelists(str(nml))["reportsidefluxes"] is False


def test_the_namelist_driver_refuses_the_key_for_spectral_jobs(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    made = []
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: [object(), object()])
    import mcbrat3d_amd
    monkeypatch.setattr(mcbrat3d_amd, "new_Integrator", lambda *a, **k: made.append(a))
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&output reportSideFluxes = .true. /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="reportSideFluxes"):
        driver_cli.main([str(nml)])
    assert not made  # refused before any integrator is made


def test_spectral_run_refuses_the_setting():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match="side fluxes"):
        broadband.SpectralRun(M, [object()], recSideFluxes=True)


def _stats(nx, ny, nz, side, seed=4):
    from tests.test_actinic_host import _stats as old_stats
    st = old_stats(nx, ny, nz, False, seed)
    if side:
        rng = np.random.default_rng(seed + 1)
        for name, mean in zip(SC.NAMES, SC.MEANS):
            st[name], st[name + "_StdErr"] = rng.random((nx, ny, nz)) * 2.0, rng.random((nx, ny, nz)) * 1e-3
            st[mean], st[mean + "_StdErr"] = rng.random(nz) * 2.0, rng.random(nz) * 1e-3
    return st


@pytest.mark.parametrize("withZ", [False, True])
def test_netcdf_round_trip_of_the_side_fluxes(tmp_path, withZ):
    from mcbrat3d_amd import ncio
    nx, ny, nz = 4, 3, 5
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.array([0.0, 0.1, 0.4, 0.5, 1.1, 2.0])
    st = _stats(nx, ny, nz, True)
    kw = dict(reportAbsorptionProfile=withZ, reportVolumeAbsorption=withZ)
    out = ncio.writeResults_netcdf(str(tmp_path / "o.nc"), "dom", st, xe, ye, ze, **kw)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.dimensions["z"] == nz and np.array_equal(f.variables["z"][:], 0.5 * (ze[1:] + ze[:-1]))
        for name, mean in zip(SC.NAMES, SC.MEANS):
            for k in (name, name + "_StdErr"):
                v = f.variables[k]
                assert v.dimensions == ("z", "y", "x")  # Fortran (x, y, z)
                assert np.array_equal(np.asarray(v[:]).transpose(2, 1, 0), st[k].astype(np.float32))
            for k in (mean, mean + "_StdErr"):
                assert f.variables[k].dimensions == ("z",) and np.array_equal(np.asarray(f.variables[k][:]), st[k].astype(np.float32))
        assert ("absorbedVolume" in f.variables) == withZ
    finally:
        f.close()
    # a file written without the keys is byte for byte what the same call wrote before
    plain = {k: v for k, v in st.items() if "ideFlux" not in k}
    a = ncio.writeResults_netcdf(str(tmp_path / "a.nc"), "dom", plain, xe, ye, ze, **kw)
    b = ncio.writeResults_netcdf(str(tmp_path / "b.nc"), "dom", _stats(nx, ny, nz, False), xe, ye, ze, **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(a, "r", mmap=False)
    try:
        assert "fluxUp" in f.variables and not any("ideFlux" in k for k in f.variables) and (("z" in f.dimensions) == withZ)
    finally:
        f.close()


def test_every_layer_declares_the_entries():
    import inspect
    from mcbrat3d_amd import _capi, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    api = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_api.hip")).read()
    for sym in ("mcbrat_specify_side_fluxes", "mcbrat_report_side_fluxes"):
        assert re.search(r"\bint %s\(mcbrat_ctx \*ctx" % sym, text) and sym in _capi.SYMBOLS
        assert re.search(r"\bint %s\(mcbrat_ctx \*c\b" % sym, api)
    assert len(_capi.SYMBOLS["mcbrat_specify_side_fluxes"][1]) == 2 and len(_capi.SYMBOLS["mcbrat_report_side_fluxes"][1]) == 3
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    assert "meanSideFluxXPlus[nz]" in text  # the moment tail, next to the actinic one
    assert "recSideFluxes" in inspect.signature(integrator.Integrator.specifyParameters).parameters
    assert "recSideFluxes=self.recSideFluxes" in inspect.getsource(integrator.Integrator.copy_Integrator)
    assert hasattr(integrator.Integrator, "reportSideFluxes")
    assert integrator.SIDE_FLUX_NAMES == SC.NAMES


def test_fortran_shim_declares_the_side_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("specifySideFluxes", "reportSideFluxes"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_specify_side_fluxes", "mcbrat_report_side_fluxes"):
        assert 'name="%s"' % sym in text
    nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("specifysidefluxes", "reportsidefluxes"):
        assert re.search(r"\bt\b.*%s" % name, symbols), name
    drv = open(os.path.join(ROOT, "fortran", "mcbrat_driver.f90")).read().replace("&\n", " ")
    assert re.search(r"namelist /output/[^!]*\breportSideFluxes\b", drv)
    assert re.search(r"if \(reportSideFluxes \.and\. \(numLambda > 1 \.or\. LW_flag >= 0\.\)\)\s+stop \"reportSideFluxes", drv)
    subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_driver.f90"), "-o", str(tmp_path / "drv.o")],
                          cwd=str(tmp_path))


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rays():
    """The helper's answer for every case of the GPU test, computed once and shared (never modified)."""
    return {case: SC.ray_cast(*case) for case in SC.RAY_CASES}


def test_the_uniforms_are_the_oracles_philox_draws():
    """Photon id i, event 0 (launch) and event 1 (the first leg), block 0: the oracle's generator through its Python binding, and a
    leg of the oracle itself -- a photon over a black surface in a vacuum lands in the column the helper's start and direction give."""
    from oracle import oracle as O
    u = SC.launch_uniforms(LC.SEED, LC.N_IDS)
    assert u.shape == (LC.N_IDS, 3) and u.dtype == np.float32 and np.all((u >= 0) & (u <= 1))
    assert abs(float(u.mean()) - 0.5) < 0.01 and len(np.unique(u[:, 0])) > 0.99 * LC.N_IDS
    case = SC.medium_on("irregular", 0.0)
    P = cases_problem(case)
    n = 2000
    fates = O.compute_rt(P, O.solar_source(0.5, 30.0), O.philox_rng(LC.SEED, 0), n, want_fates=True)["fates"]
    rc = SC.ray_cast("irregular", 0.0, 0.5, 30.0, n=LC.N_IDS)
    xe, ye = case["xe"], case["ye"]
    end = rc["start"][:n] + rc["disp"][:n]
    ix = np.searchsorted(xe, np.mod(end[:, 0] - xe[0], xe[-1] - xe[0]) + xe[0], side="right")
    iy = np.searchsorted(ye, np.mod(end[:, 1] - ye[0], ye[-1] - ye[0]) + ye[0], side="right")
    clean = ~rc["flagged"][:n]
    assert clean.mean() > 0.95 and np.all(fates["fate"][clean] == 1)
    assert np.array_equal(fates["ix"][clean], ix[clean]) and np.array_equal(fates["iy"][clean], iy[clean])


def cases_problem(case):
    from tests import cases
    return cases.oracle_problem(case, nsteps=2001, use_russian_roulette=True)


def test_the_flagged_share_is_capped(rays):
    """At most 5 % of the ids are left out of the photon-by-photon comparison on every case: a cap, not a measurement (the
    full-history flags of the same delta are 0.14-1.6 % in DESIGN.md section 4.14; first legs alone lie far below)."""
    for case, rc in rays.items():
        share = float(rc["flagged"].mean())
        print("flagged share %.5f: %s" % (share, case))
        assert share <= 0.05, case
        assert rc["flagged"].size == LC.N_IDS and len(LC.clean_runs(rc["flagged"])) >= 1


def test_in_a_vacuum_the_crossings_are_the_face_positions_between_the_ends(rays):
    """Every photon's crossing count per axis equals the number of face positions {edge_j + m L} between the ends of its known
    displacement (height / mu0 along the direction), counted here by position on the unwrapped axis, not by the helper's planes."""
    for case, rc in rays.items():
        grid, ext, mu0, phi0 = case
        if ext != 0.0:
            continue
        xe, ye, ze = SC.axes(grid)
        d = SC.direction(mu0, phi0)
        path = (SC.launch_height(ze) - ze[0]) / abs(d[2])
        assert np.all(rc["lands"]) and np.allclose(rc["disp"], path * d[:2][None, :], rtol=1e-14)
        for a, e in ((0, np.asarray(xe, np.float64)), (1, np.asarray(ye, np.float64))):
            L = e[-1] - e[0]
            p0, p1 = rc["start"][:, a], rc["start"][:, a] + path * d[a]
            lo, hi = np.minimum(p0, p1), np.maximum(p0, p1)

            def below(x):  # face positions <= x on the unwrapped axis, up to a constant
                m = np.floor((x - e[0]) / L)
                return m * (len(e) - 1) + np.searchsorted(e[:-1], x - m * L, side="right")
            want = below(hi) - below(lo)
            exact = np.abs(want - rc["ncross"][:, a]) == 0
            assert exact[~rc["flagged"]].all(), (case, a)
            assert (~exact).sum() <= rc["flagged"].sum()
        nx, ny, nz = rc["dims"]
        b = rc["bins"]
        assert np.all((b[:, 0] >= 0) & (b[:, 0] < 4) & (b[:, 1] < nz) & (b[:, 2] < ny) & (b[:, 3] < nx) & (b.min() >= 0))
        assert len(b) == rc["ncross"].sum() and np.array_equal(np.bincount(rc["ids"], minlength=LC.N_IDS), rc["ncross"].sum(axis=1))
        # nothing travels against the beam
        assert set(np.unique(b[:, 0])) <= ({0} if d[0] > 0 else {1}) | ({2} if d[1] > 0 else {3})


def test_the_helpers_own_counts_obey_the_closed_forms(rays):
    """Over the unflagged ids, batches of 500 ids pushed through the written-out epilogue: the layer means of the four parts against
    tan(theta0) cos(phi0), tan(theta0) sin(phi0) in a vacuum and times the beam's layer average in the absorber, within 4.5
    standard errors of the batch spread plus 1e-5 -- the check tests/test_gpu_side_flux.py makes of the product."""
    from tests import epilogue_mirror as EM
    for case, rc in rays.items():
        grid, ext, mu0, phi0 = case
        xe, ye, ze = SC.axes(grid)
        g = EM.Grid(xe, ye, ze)
        clean = np.flatnonzero(~rc["flagged"])
        per = 500
        vals = []
        keep = np.zeros(LC.N_IDS, bool)
        for b in range(len(clean) // per):
            keep[:] = False
            keep[clean[b * per:(b + 1) * per]] = True
            sel = keep[rc["ids"]]
            raw = np.zeros((4, g.nz, g.ny, g.nx), np.int64)
            c = rc["bins"][sel]
            np.add.at(raw, (c[:, 0], c[:, 1], c[:, 2], c[:, 3]), 1)
            vals.append(SC.side_values(g, (raw << 32).reshape(4, g.nz, g.ncol), per)[0].astype(np.float64).reshape(4, g.nz))
        vals = np.asarray(vals)
        mean = vals.mean(axis=0)
        err = np.sqrt(np.maximum(0.0, (vals * vals).mean(axis=0) - mean ** 2) / (len(vals) - 1.0))
        fx, fy = SC.horizontal(mu0, phi0)
        prof = SC.absorber_profile(ze, ext, mu0) if ext else np.ones(g.nz)
        want = np.stack([max(fx, 0.0) * prof, max(-fx, 0.0) * prof, max(fy, 0.0) * prof, max(-fy, 0.0) * prof])
        z = (mean - want) / np.where(err > 0, err, 1.0)
        print("helper against the closed forms, %s: max |z| %.2f" % (case, np.abs(z).max()))
        assert np.all(np.abs(mean - want) <= 4.5 * err + 1e-5), (case, mean, want, err)
        assert np.all(mean[want == 0] == 0)
