"""The actinic flux of every cell (recActinicFlux), the parts that need no GPU: the moment layout the
host unpacks, the statistics, the /output/ namelist keyword of both drivers, the spectral refusals, the NetCDF writer, the
declarations of every layer, the Fortran shim, and the units of the plane-parallel reference of tests/test_gpu_actinic.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from tests import actinic_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("meanActinicFlux", "actinicFlux")


def _buffer(nx, ny, nz, nDir, quantities=4, actinic=True):
    """A moment array whose S1 holds its own offsets 0, 1, 2, ... and whose S2 holds them + 0.5."""
    ncol = nx * ny
    M = 3 + 3 * ncol + nz + ncol * nz + nDir * ncol + quantities * (nz + 1) * (1 + ncol) + (nz * (1 + ncol) if actinic else 0)
    buf = np.zeros(8 + 2 * M)
    buf[0], buf[1] = 12345.0, 7.0
    buf[8:8 + M] = np.arange(M)
    buf[8 + M:] = np.arange(M) + 0.5
    return buf, M


@pytest.mark.parametrize("nDir", [0, 2])
@pytest.mark.parametrize("quantities", [0, 2, 4])
def test_unpack_moments_finds_the_actinic_tail_behind_every_other(nDir, quantities):
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    ncol, nLvl = nx * ny, nz + 1
    buf, M = _buffer(nx, ny, nz, nDir, quantities)
    kw = dict(levelFluxes=quantities >= 2, directLevelFluxes=quantities == 4)
    for given in (nDir, None):  # the number of directions given, or told by the length
        out = driver.unpack_moments(buf, nx, ny, nz, nDirections=given, actinicFlux=True, **kw)
        A = M - nz * (1 + ncol)  # where the actinic tail starts: behind the level and direct tails
        assert np.array_equal(out["meanActinicFlux"][0], A + np.arange(nz))
        assert np.array_equal(out["meanActinicFlux"][1], A + np.arange(nz) + 0.5)
        act = out["actinicFlux"][0]
        assert act.shape == (nx, ny, nz)
        for ix in range(nx):
            for iy in range(ny):
                for k in range(nz):  # layer slowest, x fastest
                    assert act[ix, iy, k] == A + nz + (k * ny + iy) * nx + ix
        assert act[nx - 1, ny - 1, nz - 1] == M - 1  # the last entry of the array
        assert ("intensity" in out) == (nDir > 0)
        if quantities:  # the older tails are where they are without the setting
            T = A - quantities * nLvl * (1 + ncol)
            assert np.array_equal(out["meanLevelFluxUp"][0], T + np.arange(nLvl))
            assert out["levelFluxDown"][0][1, 1, 2] == T + 2 * nLvl + ncol * nLvl + (2 * ny + 1) * nx + 1
        if quantities == 4:
            D = A - 2 * nLvl * (1 + ncol)
            assert np.array_equal(out["meanLevelFluxDownDirect"][0], D + np.arange(nLvl))
        # every older part equals what the array without the tail unpacks to
        old_buf = np.concatenate([buf[:8 + A], buf[8 + M:8 + M + A]])
        old = driver.unpack_moments(old_buf, nx, ny, nz, nDirections=given, **kw)
        assert set(out) == set(old) | set(NEW)
        for k, v in old.items():
            assert np.array_equal(np.asarray(out[k]), np.asarray(v)), k


def test_unpack_moments_refuses_a_wrong_length():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, _ = _buffer(nx, ny, nz, 0, 2)
    with pytest.raises(ValueError):  # a buffer without the actinic tail
        driver.unpack_moments(_buffer(nx, ny, nz, 0, 2, actinic=False)[0], nx, ny, nz, nDirections=0, levelFluxes=True, actinicFlux=True)
    with pytest.raises(ValueError):  # a buffer with it, unpacked without the keyword
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True)
    with pytest.raises(ValueError):  # one double short
        driver.unpack_moments(buf[:-1], nx, ny, nz, nDirections=0, levelFluxes=True, actinicFlux=True)
    with pytest.raises(ValueError):  # no level tail in the layout asked for
        driver.unpack_moments(buf, nx, ny, nz, nDirections=0, actinicFlux=True)


def test_actinicFlux_off_gives_exactly_the_old_dictionaries():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    for quantities, nDir in ((0, 0), (0, 2), (2, 0), (4, 0)):
        buf, _ = _buffer(nx, ny, nz, nDir, quantities, actinic=False)
        kw = dict(levelFluxes=quantities >= 2, directLevelFluxes=quantities == 4)
        a = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, **kw)
        b = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, actinicFlux=False, **kw)
        assert list(a) == list(b) and not any(k in a for k in NEW)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]))
        sa, sb = driver.statistics(a, 2.0), driver.statistics(b, 2.0)
        assert list(sa) == list(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)


def test_statistics_returns_the_actinic_keys():
    from mcbrat3d_amd import driver
    nx, ny, nz = 3, 2, 4
    buf, M = _buffer(nx, ny, nz, 0, 2)
    st = driver.statistics(driver.unpack_moments(buf, nx, ny, nz, nDirections=0, levelFluxes=True, actinicFlux=True), solarFlux=2.0)
    assert st["actinicFlux"].shape == st["actinicFlux_StdErr"].shape == (nx, ny, nz)
    assert st["meanActinicFlux"].shape == st["meanActinicFlux_StdErr"].shape == (nz,)
    assert st["meanActinicFlux"][0] == 2.0 * (M - nz * (1 + nx * ny)) / 12345.0


class _FakeIntegrator:
    """What driver.run asks of an integrator, for a one-rank run that traces nothing."""
    numRecScatOrd, recLevelFluxes, recDirectLevelFluxes, recActinicFlux, _dims = -1, True, False, True, (3, 2, 4)

    def resetMoments(self):
        pass

    def computeRadiativeTransfer(self, *a):
        pass

    def numIntensityDirections(self):
        return 0

    def moments(self):
        return _buffer(3, 2, 4, 0, 2)[0]


def test_driver_run_carries_the_setting():
    from mcbrat3d_amd import driver
    from mcbrat3d_amd.illumination import new_PhotonStream
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    st = driver.run(_FakeIntegrator(), None, new_PhotonStream(0.5, 0.0, numberOfPhotons=10), 5, 2, new_RandomNumberSequence(1))
    assert all(k in st and k + "_StdErr" in st for k in NEW) and "levelFluxUp" in st


def test_namelist_reads_reportActinicFlux(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&output reportActinicFlux = .true. /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["reportactinicflux"] is True and cfg["reportlevelfluxes"] is False
    nml.write_text("&output reportLevelFluxes = .true. /\n")
    assert driver_cli.read_namelists(str(nml))["reportactinicflux"] is False


def test_the_namelist_driver_refuses_the_key_for_spectral_jobs(tmp_path, monkeypatch):
    from mcbrat3d_amd import driver_cli
    made = []
    monkeypatch.setattr(driver_cli, "load_domains", lambda cfg: [object(), object()])
    import mcbrat3d_amd
    monkeypatch.setattr(mcbrat3d_amd, "new_Integrator", lambda *a, **k: made.append(a))
    nml = tmp_path / "r.nml"
    nml.write_text("&monteCarlo numPhotonsPerBatch = 10 /\n&output reportActinicFlux = .true. /\n&fileNames physDomainFile = 'builtin:x' /\n")
    with pytest.raises(SystemExit, match="reportActinicFlux"):
        driver_cli.main([str(nml)])
    assert not made  # refused before any integrator is made


def test_spectral_run_refuses_the_setting():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match="actinic flux"):
        broadband.SpectralRun(M, [object()], recActinicFlux=True)


def _stats(nx, ny, nz, actinic, seed=4):
    rng = np.random.default_rng(seed)
    st = {"totalPhotons": 100000, "batches": 10}
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        st[k], st[k + "_StdErr"] = rng.random((nx, ny)), rng.random((nx, ny)) * 1e-3
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        st[k], st[k + "_StdErr"] = float(rng.random()), 1e-4
    st["absorbedProfile"], st["absorbedProfile_StdErr"] = rng.random(nz), rng.random(nz) * 1e-3
    st["absorbedVolume"], st["absorbedVolume_StdErr"] = rng.random((nx, ny, nz)), rng.random((nx, ny, nz)) * 1e-3
    if actinic:
        st["actinicFlux"], st["actinicFlux_StdErr"] = rng.random((nx, ny, nz)) * 3.0, rng.random((nx, ny, nz)) * 1e-3
        st["meanActinicFlux"], st["meanActinicFlux_StdErr"] = rng.random(nz) * 3.0, rng.random(nz) * 1e-3
    return st


@pytest.mark.parametrize("withZ", [False, True])
def test_netcdf_round_trip_of_the_actinic_flux(tmp_path, withZ):
    from mcbrat3d_amd import ncio
    nx, ny, nz = 4, 3, 5
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.array([0.0, 0.1, 0.4, 0.5, 1.1, 2.0])
    st = _stats(nx, ny, nz, True)
    kw = dict(reportAbsorptionProfile=withZ, reportVolumeAbsorption=withZ)
    out = ncio.writeResults_netcdf(str(tmp_path / "o.nc"), "dom", st, xe, ye, ze, **kw)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.dimensions["z"] == nz and np.array_equal(f.variables["z"][:], 0.5 * (ze[1:] + ze[:-1]))
        for k in ("actinicFlux", "actinicFlux_StdErr"):
            v = f.variables[k]
            assert v.dimensions == ("z", "y", "x")  # Fortran (x, y, z)
            assert np.array_equal(np.asarray(v[:]).transpose(2, 1, 0), st[k].astype(np.float32))
        for k in ("meanActinicFlux", "meanActinicFlux_StdErr"):
            assert f.variables[k].dimensions == ("z",) and np.array_equal(np.asarray(f.variables[k][:]), st[k].astype(np.float32))
        assert ("absorbedVolume" in f.variables) == withZ
    finally:
        f.close()
    # a file written without the keys is byte for byte what the same call wrote before
    plain = {k: v for k, v in st.items() if "ctinic" not in k}
    a = ncio.writeResults_netcdf(str(tmp_path / "a.nc"), "dom", plain, xe, ye, ze, **kw)
    b = ncio.writeResults_netcdf(str(tmp_path / "b.nc"), "dom", _stats(nx, ny, nz, False), xe, ye, ze, **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(a, "r", mmap=False)
    try:
        assert "fluxUp" in f.variables and not any("ctinic" in k for k in f.variables) and (("z" in f.dimensions) == withZ)
    finally:
        f.close()


def test_every_layer_declares_the_entries():
    import inspect
    from mcbrat3d_amd import _capi, integrator
    text = open(os.path.join(ROOT, "include", "mcbrat.h")).read()
    api = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_api.hip")).read()
    for sym in ("mcbrat_specify_actinic_flux", "mcbrat_report_actinic_flux"):
        assert re.search(r"\bint %s\(mcbrat_ctx \*ctx" % sym, text) and sym in _capi.SYMBOLS
        assert re.search(r"\bint %s\(mcbrat_ctx \*c\b" % sym, api)
    assert len(_capi.SYMBOLS["mcbrat_specify_actinic_flux"][1]) == 2 and len(_capi.SYMBOLS["mcbrat_report_actinic_flux"][1]) == 3
    assert "#define MCBRAT_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    assert "recActinicFlux" in inspect.signature(integrator.Integrator.specifyParameters).parameters
    assert "recActinicFlux=self.recActinicFlux" in inspect.getsource(integrator.Integrator.copy_Integrator)
    assert hasattr(integrator.Integrator, "reportActinicFlux")


def test_fortran_shim_declares_the_actinic_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("specifyActinicFlux", "reportActinicFlux"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_specify_actinic_flux", "mcbrat_report_actinic_flux"):
        assert 'name="%s"' % sym in text
    # the object file exports the module procedures
    nm = shutil.which("llvm-nm") or shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    symbols = subprocess.run([nm, str(tmp_path / "shim.o")], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("specifyactinicflux", "reportactinicflux"):
        assert re.search(r"\bt\b.*%s" % name, symbols), name
    drv = open(os.path.join(ROOT, "fortran", "mcbrat_driver.f90")).read().replace("&\n", " ")
    assert re.search(r"namelist /output/[^!]*\breportActinicFlux\b", drv)
    assert re.search(r"if \(reportActinicFlux \.and\. \(numLambda > 1 \.or\. LW_flag >= 0\.\)\)\s+stop \"reportActinicFlux", drv)
    subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_driver.f90"), "-o", str(tmp_path / "drv.o")],
                          cwd=str(tmp_path))


def test_the_units_of_the_layered_reference():
    """4 pi (1 - omega) J dtau summed over a layer is the flux the layer absorbs: tests.test_analytic's own absorption of the
    slab, from the same solution.  This pins the normalisation of the mean intensity the GPU test compares the actinic flux with
    (per unit flux through a horizontal unit area at the top, whatever mu0)."""
    from tests import test_analytic as A
    ref = AC.layered_reference()
    absorbed = A.layered_isotropic_absorption(AC.SLAB["dtaus"], AC.SLAB["omegas"], AC.SLAB["mu0"], albedo=AC.SLAB["albedo"])
    assert np.allclose(ref["absorbed"], absorbed, rtol=2e-6, atol=1e-9), (ref["absorbed"], absorbed)
    assert ref["absorbed"][0] == 0.0 and ref["absorbed"][1] > 0.05     # the conservative layer absorbs nothing, the other does
    # sanity of the scale: under mu0 the unscattered beam alone gives exp(-tau / mu0) / mu0, and scattering only adds to it
    assert ref["actinic"][0] > (1.0 - np.exp(-0.5 / 0.6)) / 0.5 and np.all(ref["actinic"] > 0)
    # the mirror of the kernel's scale: the smallest power of two above the longest step
    assert AC.actinic_unit([0.0, 1.0], [0.0, 1.0], [0.0, 1.0]) == 2.0 and AC.actinic_unit([0, 0.5], [0, 0.5], [0, 0.5]) == 1.0
    assert AC.actinic_unit([0, 0.03, 0.08], [0, 0.05], [0, 0.04]) == 0.125
