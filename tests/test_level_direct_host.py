"""The direct / diffuse separation of the level fluxes (recDirectLevelFluxes), the parts that need no GPU:
the moment layout the host unpacks, the statistics, the /output/ namelist keyword of both drivers, the NetCDF writer, the
declarations of every layer, the Fortran shim, and the black-twin identity on the oracle alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from tests import cases
from tests import level_cases as LC
from tests import level_direct_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("meanLevelFluxDownDirect", "meanLevelFluxDownDiffuse", "levelFluxDownDirect", "levelFluxDownDiffuse")


def _buffer(nx, ny, nz, nDir, quantities=4):
    """A moment array whose S1 holds its own offsets 0, 1, 2, ... and whose S2 holds them + 0.5."""
    ncol = nx * ny
    M = 3 + 3 * ncol + nz + ncol * nz + nDir * ncol + quantities * (nz + 1) * (1 + ncol)
    buf = np.zeros(8 + 2 * M)
    buf[0], buf[1] = 12345.0, 7.0
    buf[8:8 + M] = np.arange(M)
    buf[8 + M:] = np.arange(M) + 0.5
    return buf, M


@pytest.mark.parametrize("nDir", [0, 2])
def test_unpack_moments_with_the_direct_tail(nDir):
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    ncol, nLvl = nx * ny, nz + 1
    buf, M = _buffer(nx, ny, nz, nDir)
    for given in (nDir, None):  # the number of directions given, or told by the length
        out = driver.unpack_moments(buf, nx, ny, nz, nDirections=given, levelFluxes=True, directLevelFluxes=True)
        T = M - 4 * nLvl * (1 + ncol)   # where the level tail starts
        D = T + 2 * nLvl * (1 + ncol)   # where the direct / diffuse tail starts
        # the level tail is where it is without the setting ...
        assert np.array_equal(out["meanLevelFluxUp"][0], T + np.arange(nLvl))
        assert np.array_equal(out["meanLevelFluxDown"][0], T + nLvl + np.arange(nLvl))
        assert out["levelFluxDown"][0][1, 1, 2] == T + 2 * nLvl + ncol * nLvl + (2 * ny + 1) * nx + 1
        # ... and the new tail follows it: [meanDirect | meanDiffuse | direct | diffuse]
        assert np.array_equal(out["meanLevelFluxDownDirect"][0], D + np.arange(nLvl))
        assert np.array_equal(out["meanLevelFluxDownDiffuse"][0], D + nLvl + np.arange(nLvl))
        assert np.array_equal(out["meanLevelFluxDownDiffuse"][1], D + nLvl + np.arange(nLvl) + 0.5)
        direct, diffuse = out["levelFluxDownDirect"][0], out["levelFluxDownDiffuse"][0]
        assert direct.shape == diffuse.shape == (nx, ny, nLvl)
        for ix in range(nx):
            for iy in range(ny):
                for k in range(nLvl):  # level slowest, x fastest
                    assert direct[ix, iy, k] == D + 2 * nLvl + (k * ny + iy) * nx + ix
                    assert diffuse[ix, iy, k] == D + 2 * nLvl + ncol * nLvl + (k * ny + iy) * nx + ix
        assert diffuse[nx - 1, ny - 1, nLvl - 1] == M - 1  # the last entry of the array
        assert ("intensity" in out) == (nDir > 0)


def test_unpack_moments_refuses_what_does_not_fit():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, _ = _buffer(nx, ny, nz, 0)
    with pytest.raises(ValueError):  # the setting needs the level tail
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, directLevelFluxes=True)
    with pytest.raises(ValueError):  # a buffer with the level tail only
        driver.unpack_moments(_buffer(nx, ny, nz, 0, quantities=2)[0], nx, ny, nz, nDirections=0, levelFluxes=True, directLevelFluxes=True)
    with pytest.raises(ValueError):  # and the other way round
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True)
    # without the keyword nothing changes
    out = driver.unpack_moments(_buffer(nx, ny, nz, 0, quantities=2)[0], nx, ny, nz, nDirections=0, levelFluxes=True)
    assert "levelFluxDown" in out and not any(k in out for k in NEW)


def test_statistics_returns_the_direct_keys():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, M = _buffer(nx, ny, nz, 0)
    st = driver.statistics(driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True, directLevelFluxes=True), solarFlux=2.0)
    for k in ("levelFluxDownDirect", "levelFluxDownDiffuse"):
        assert st[k].shape == st[k + "_StdErr"].shape == (nx, ny, nz + 1)
    for k in ("meanLevelFluxDownDirect", "meanLevelFluxDownDiffuse"):
        assert st[k].shape == st[k + "_StdErr"].shape == (nz + 1,)
    assert st["meanLevelFluxDownDirect"][0] == 2.0 * (M - 2 * (nz + 1) * (1 + nx * ny)) / 12345.0


class _FakeIntegrator:
    """What driver.run asks of an integrator, for a one-rank run that traces nothing."""
    numRecScatOrd, recLevelFluxes, recDirectLevelFluxes, _dims = -1, True, True, (3, 2, 4)

    def resetMoments(self):
        pass

    def computeRadiativeTransfer(self, *a):
        pass

    def numIntensityDirections(self):
        return 0

    def moments(self):
        return _buffer(3, 2, 4, 0)[0]


def test_driver_run_unpacks_the_direct_tail():
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.illumination import new_PhotonStream
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    st = driver.run(_FakeIntegrator(), None, new_PhotonStream(0.5, 0.0, numberOfPhotons=10), 5, 2, new_RandomNumberSequence(1))
    assert all(k in st and k + "_StdErr" in st for k in NEW)


def test_namelist_reads_reportDirectLevelFluxes(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&output reportLevelFluxes = .true., reportDirectLevelFluxes = .true. /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["reportdirectlevelfluxes"] is True and cfg["reportlevelfluxes"] is True
    nml.write_text("&output reportLevelFluxes = .true. /\n")
    assert driver_cli.read_namelists(str(nml))["reportdirectlevelfluxes"] is False


def test_the_namelist_driver_refuses_the_key_for_spectral_jobs(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: [object(), object()])
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&output reportDirectLevelFluxes = .true. /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="reportDirectLevelFluxes"):
        driver_cli.main([str(nml)])


def test_spectral_run_refuses_the_setting():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match="direct level fluxes"):
        broadband.SpectralRun(M, [object()], recDirectLevelFluxes=True)


def _stats(nx, ny, nz, direct, seed=4):
    rng = np.random.default_rng(seed)
    st = {"totalPhotons": 100000, "batches": 10}
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        st[k], st[k + "_StdErr"] = rng.random((nx, ny)), rng.random((nx, ny)) * 1e-3
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        st[k], st[k + "_StdErr"] = float(rng.random()), 1e-4
    for k in ("levelFluxUp", "levelFluxDown"):
        st[k], st[k + "_StdErr"] = rng.random((nx, ny, nz + 1)), rng.random((nx, ny, nz + 1)) * 1e-3
    for k in ("meanLevelFluxUp", "meanLevelFluxDown"):
        st[k], st[k + "_StdErr"] = rng.random(nz + 1), rng.random(nz + 1) * 1e-3
    if direct:
        for k in ("levelFluxDownDirect", "levelFluxDownDiffuse"):
            st[k], st[k + "_StdErr"] = rng.random((nx, ny, nz + 1)), rng.random((nx, ny, nz + 1)) * 1e-3
        for k in ("meanLevelFluxDownDirect", "meanLevelFluxDownDiffuse"):
            st[k], st[k + "_StdErr"] = rng.random(nz + 1), rng.random(nz + 1) * 1e-3
    return st


def test_netcdf_writer_direct_level_fluxes(tmp_path):
    from mcbrat3d_amd import ncio
    nx, ny, nz = 4, 3, 5
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.array([0.0, 0.1, 0.4, 0.5, 1.1, 2.0])
    st = _stats(nx, ny, nz, True)
    out = ncio.writeResults_netcdf(str(tmp_path / "o.nc"), "dom", st, xe, ye, ze)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.dimensions["zLevel"] == nz + 1
        for k in ("levelFluxDownDirect", "levelFluxDownDiffuse", "levelFluxDownDirect_StdErr", "levelFluxDownDiffuse_StdErr", "levelFluxDown"):
            v = f.variables[k]
            assert v.dimensions == ("zLevel", "y", "x")  # Fortran (x, y, zLevel)
            assert np.array_equal(np.asarray(v[:]).transpose(2, 1, 0), st[k].astype(np.float32))
    finally:
        f.close()
    # a file written without the keys is byte for byte the file of level fluxes alone
    plain = {k: v for k, v in st.items() if "Direct" not in k and "Diffuse" not in k}
    a = ncio.writeResults_netcdf(str(tmp_path / "a.nc"), "dom", plain, xe, ye, ze)
    b = ncio.writeResults_netcdf(str(tmp_path / "b.nc"), "dom", _stats(nx, ny, nz, False), xe, ye, ze)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(a, "r", mmap=False)
    try:
        assert "levelFluxDown" in f.variables and "levelFluxDownDirect" not in f.variables
    finally:
        f.close()


def test_every_layer_declares_the_entries():
    import inspect
    from mcbrat3d_amd import _capi, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    for sym in ("mcbrat_specify_direct_level_fluxes", "mcbrat_report_direct_level_fluxes"):
        assert re.search(r"\bint %s\(mcbrat_ctx \*ctx" % sym, text) and sym in _capi.SYMBOLS
        assert re.search(r"\bint %s\(mcbrat_ctx \*c\b" % sym, open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_api.hip")).read())
    assert len(_capi.SYMBOLS["mcbrat_report_direct_level_fluxes"][1]) == 5
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    assert "recDirectLevelFluxes" in inspect.signature(integrator.Integrator.specifyParameters).parameters
    assert "recDirectLevelFluxes=self.recDirectLevelFluxes" in inspect.getsource(integrator.Integrator.copy_Integrator)


def test_fortran_shim_declares_the_direct_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("specifyDirectLevelFluxes", "reportDirectLevelFluxes"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_specify_direct_level_fluxes", "mcbrat_report_direct_level_fluxes"):
        assert 'name="%s"' % sym in text
    # the object file exports the module procedures
    nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("specifydirectlevelfluxes", "reportdirectlevelfluxes"):
        assert re.search(r"\bt\b.*%s" % name, symbols), name
    drv = open(os.path.join(ROOT, "fortran", "mcbrat_driver.f90")).read().replace("&\n", " ")
    assert re.search(r"namelist /output/[^!]*\breportDirectLevelFluxes\b", drv)
    assert re.search(r"if \(reportDirectLevelFluxes \.and\. \(numLambda > 1 \.or\. LW_flag >= 0\.\)\)\s+stop \"reportDirectLevelFluxes", drv)
    subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_driver.f90"), "-o", str(tmp_path / "drv.o")],
                          cwd=str(tmp_path))


@pytest.mark.parametrize("name", ["regular, oblique, flat walk", "irregular, oblique back, nested walk"])
def test_the_black_twin_identity_on_the_oracle(name):
    """On the oracle alone: the twin's level sums are its deposit counts (every direct weight is 1), it deposits nothing upward,
    level numZ holds every photon, the beam only loses photons on its way down, the twin's flagged ids are among the real
    medium's, and no bin of the twin exceeds the real medium's downward bin by more than the rounding of the latter's sum."""
    from oracle import oracle as O
    O.build()
    n = 4000
    grid, mu0, phi0, _, _, rr = LC.EXACT[name]
    case, P, src = LC.oracle_setup(name)
    Pt = cases.oracle_problem(DC.black_twin(case), nsteps=LC.TABLE, use_russian_roulette=rr)
    real = O.compute_rt_levels(P, src, O.philox_rng(LC.SEED, 0), n)
    twin = O.compute_rt_levels(Pt, src, O.philox_rng(LC.SEED, 0), n)
    assert np.array_equal(twin["levelDown"], twin["levelDownCount"]) and not twin["levelUpCount"].any() and not twin["levelUp"].any()
    per_level = twin["levelDownCount"].reshape(P.nz + 1, -1).sum(axis=1)
    assert per_level[P.nz] == n and np.all(np.diff(per_level) >= 0) and per_level[0] < n and per_level.sum() > n
    assert not np.any(twin["nearFace"] & ~real["nearFace"])
    assert np.all(twin["levelDownCount"] <= real["levelDownCount"])
    assert np.all(twin["levelDown"] <= real["levelDown"] * (1.0 + real["levelDownCount"] * 2.0 ** -52))
