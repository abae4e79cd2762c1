"""Level fluxes (recLevelFluxes), the parts that need no GPU: the moment layout the host unpacks, the
statistics, the /output/ namelist keyword, the NetCDF writer, the refusals decided on the Python side, and the Fortran shim."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _buffer(nx, ny, nz, nDir):
    """A moment array whose S1 holds its own offsets 0, 1, 2, ... and whose S2 holds them + 0.5."""
    ncol = nx * ny
    M = 3 + 3 * ncol + nz + ncol * nz + nDir * ncol + 2 * (nz + 1) * (1 + ncol)
    buf = np.zeros(8 + 2 * M)
    buf[0], buf[1] = 12345.0, 7.0
    buf[8:8 + M] = np.arange(M)
    buf[8 + M:] = np.arange(M) + 0.5
    return buf, M


@pytest.mark.parametrize("nDir", [0, 2])
def test_unpack_moments_with_the_level_tail(nDir):
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    ncol, nLvl = nx * ny, nz + 1
    buf, M = _buffer(nx, ny, nz, nDir)
    for given in (nDir, None):  # the number of directions given, or told by the length
        out = driver.unpack_moments(buf, nx, ny, nz, nDirections=given, levelFluxes=True)
        T = M - 2 * nLvl * (1 + ncol)  # where the tail starts
        assert out["totalPhotons"] == 12345.0 and out["batches"] == 7.0
        assert np.array_equal(out["meanLevelFluxUp"][0], T + np.arange(nLvl))
        assert np.array_equal(out["meanLevelFluxDown"][0], T + nLvl + np.arange(nLvl))
        assert np.array_equal(out["meanLevelFluxDown"][1], T + nLvl + np.arange(nLvl) + 0.5)
        up, down = out["levelFluxUp"][0], out["levelFluxDown"][0]
        assert up.shape == down.shape == (nx, ny, nLvl)
        for ix in range(nx):
            for iy in range(ny):
                for k in range(nLvl):  # level slowest, x fastest
                    assert up[ix, iy, k] == T + 2 * nLvl + (k * ny + iy) * nx + ix
                    assert down[ix, iy, k] == T + 2 * nLvl + ncol * nLvl + (k * ny + iy) * nx + ix
        # what comes before the tail is where it always was
        assert out["fluxUp"][0][1, 1] == 3 + 1 * nx + 1 and out["absorbedVolume"][0].shape == (nx, ny, nz)
        assert ("intensity" in out) == (nDir > 0)
        if nDir:
            assert out["intensity"][0].shape == (nx, ny, nDir)
            assert out["intensity"][0][0, 0, 0] == 3 + 3 * ncol + nz + ncol * nz


def test_unpack_moments_refuses_a_wrong_length():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, _ = _buffer(nx, ny, nz, 0)
    with pytest.raises(ValueError):
        driver.unpack_moments(buf[:-2], nx, ny, nz, nDirections=0, levelFluxes=True)
    with pytest.raises(ValueError):
        driver.unpack_moments(buf, nx, ny, nz, nDirections=1, levelFluxes=True)
    with pytest.raises(ValueError):  # a buffer without the tail
        driver.unpack_moments(np.zeros(8 + 2 * (3 + 3 * 6 + nz + 6 * nz)), nx, ny, nz, levelFluxes=True)
    # and without the keyword nothing changes
    plain = np.zeros(8 + 2 * (3 + 3 * 6 + nz + 6 * nz))
    assert "levelFluxUp" not in driver.unpack_moments(plain, nx, ny, nz)


def test_statistics_returns_the_level_keys():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, _ = _buffer(nx, ny, nz, 0)
    st = driver.statistics(driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True), solarFlux=2.0)
    for k in ("levelFluxUp", "levelFluxDown"):
        assert st[k].shape == st[k + "_StdErr"].shape == (nx, ny, nz + 1)
    for k in ("meanLevelFluxUp", "meanLevelFluxDown"):
        assert st[k].shape == st[k + "_StdErr"].shape == (nz + 1,)
    assert st["meanLevelFluxUp"][0] == 2.0 * (3 + 3 * 6 + nz + 6 * nz) / 12345.0


def test_namelist_reads_reportLevelFluxes(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&output reportLevelFluxes = .true. /\n")
    assert driver_cli.read_namelists(str(nml))["reportlevelfluxes"] is True
    nml.write_text("&output /\n")
    assert driver_cli.read_namelists(str(nml))["reportlevelfluxes"] is False


def _stats(nx, ny, nz, levels, seed=4):
    rng = np.random.default_rng(seed)
    st = {"totalPhotons": 100000, "batches": 10}
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        st[k], st[k + "_StdErr"] = rng.random((nx, ny)), rng.random((nx, ny)) * 1e-3
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        st[k], st[k + "_StdErr"] = float(rng.random()), 1e-4
    if levels:
        for k in ("levelFluxUp", "levelFluxDown"):
            st[k], st[k + "_StdErr"] = rng.random((nx, ny, nz + 1)), rng.random((nx, ny, nz + 1)) * 1e-3
        for k in ("meanLevelFluxUp", "meanLevelFluxDown"):
            st[k], st[k + "_StdErr"] = rng.random(nz + 1), rng.random(nz + 1) * 1e-3
    return st


def test_netcdf_writer_level_fluxes(tmp_path):
    from mcbrat3d_amd import ncio
    nx, ny, nz = 4, 3, 5
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.array([0.0, 0.1, 0.4, 0.5, 1.1, 2.0])
    st = _stats(nx, ny, nz, True)
    out = ncio.writeResults_netcdf(str(tmp_path / "o.nc"), "dom", st, xe, ye, ze)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.dimensions["zLevel"] == nz + 1
        assert np.array_equal(f.variables["zLevel"][:], ze)  # the edges, not mid-points
        for k in ("levelFluxUp", "levelFluxDown", "levelFluxUp_StdErr", "levelFluxDown_StdErr"):
            v = f.variables[k]
            assert v.dimensions == ("zLevel", "y", "x")  # Fortran (x, y, zLevel)
            assert np.array_equal(np.asarray(v[:]).transpose(2, 1, 0), st[k].astype(np.float32))
    finally:
        f.close()
    # only when the setting is on: without the keys the file is the one written before
    plain = {k: v for k, v in st.items() if "evel" not in k}
    a = ncio.writeResults_netcdf(str(tmp_path / "a.nc"), "dom", plain, xe, ye, ze)
    b = ncio.writeResults_netcdf(str(tmp_path / "b.nc"), "dom", _stats(nx, ny, nz, False), xe, ye, ze)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(a, "r", mmap=False)
    try:
        assert "zLevel" not in f.dimensions and "levelFluxUp" not in f.variables
    finally:
        f.close()


def test_spectral_run_refuses_level_fluxes():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match="level fluxes"):
        broadband.SpectralRun(M, [object()], recLevelFluxes=True)


def test_the_namelist_driver_refuses_level_fluxes_for_spectral_jobs(tmp_path, monkeypatch):
    """numLambda > 1 or thermal emission: refused before any integrator is made."""
    from mcbrat3d_amd import driver_cli
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: [object(), object()])
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&output reportLevelFluxes = .true. /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="reportLevelFluxes"):
        driver_cli.main([str(nml)])


def test_the_c_header_and_the_binding_declare_the_entries():
    from mcbrat3d_amd import _capi
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    for sym in ("mcbrat_specify_level_fluxes", "mcbrat_report_level_fluxes"):
        assert re.search(r"\bint %s\(mcbrat_ctx \*ctx" % sym, text) and sym in _capi.SYMBOLS
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3


def test_fortran_shim_declares_level_flux_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("specifyLevelFluxes", "reportLevelFluxes"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_specify_level_fluxes", "mcbrat_report_level_fluxes"):
        assert 'name="%s"' % sym in text
    drv = open(os.path.join(ROOT, "fortran", "mcbrat_driver.f90")).read().replace("&\n", " ")
    assert re.search(r"namelist /output/[^!]*\breportLevelFluxes\b", drv)
    subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_driver.f90"), "-o", str(tmp_path / "drv.o")],
                          cwd=str(tmp_path))
