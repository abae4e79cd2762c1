"""Fluxes and radiances by scattering order (recScatOrd), the parts that need no GPU: the moment layout the host unpacks,
the NetCDF names of the reference's writer, the broadband refusal and the Fortran shim's new entries."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic(nx, ny, nz, nDir, N):
    """A moment buffer whose every S1 entry is its own index and every S2 entry minus its index."""
    ncol, nvox, nOrd = nx * ny, nx * ny * nz, N + 1
    M = 3 + 3 * ncol + nz + nvox + nDir * ncol + (nOrd * (2 + nDir) * (1 + ncol) if N >= 0 else 0)
    buf = np.zeros(8 + 2 * M)
    buf[0], buf[1] = 1000.0, 10.0
    buf[8:8 + M] = np.arange(M)
    buf[8 + M:] = -np.arange(M)
    return buf, M


def test_unpack_moments_order_tail_offsets_and_shapes():
    from mcbrat3d_amd import driver
    nx, ny, nz, nDir, N = 3, 2, 4, 2, 3
    ncol, nOrd = nx * ny, N + 1
    buf, M = _synthetic(nx, ny, nz, nDir, N)
    out = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, numRecScatOrd=N)
    T = 3 + 3 * ncol + nz + nx * ny * nz + nDir * ncol  # where the order tail starts (include/mcbrat.h)
    s1, s2 = out["meanFluxUpByScatOrd"]
    assert s1.shape == (nOrd,) and np.array_equal(s1, T + np.arange(nOrd)) and np.array_equal(s2, -s1)
    assert np.array_equal(out["meanFluxDownByScatOrd"][0], T + nOrd + np.arange(nOrd))
    up = out["fluxUpByScatOrd"][0]
    down = out["fluxDownByScatOrd"][0]
    assert up.shape == down.shape == (nx, ny, nOrd)
    mi = out["meanIntensityByScatOrd"][0]
    inten = out["intensityByScatOrd"][0]
    assert mi.shape == (nDir, nOrd) and inten.shape == (nx, ny, nDir, nOrd)
    for p in range(nOrd):
        for iy in range(ny):
            for ix in range(nx):
                col = ix + nx * iy
                assert up[ix, iy, p] == T + 2 * nOrd + col + ncol * p
                assert down[ix, iy, p] == T + 2 * nOrd + ncol * nOrd + col + ncol * p
                for d in range(nDir):
                    assert inten[ix, iy, d, p] == T + 2 * nOrd + 2 * ncol * nOrd + nDir * nOrd + col + ncol * (d + nDir * p)
        for d in range(nDir):
            assert mi[d, p] == T + 2 * nOrd + 2 * ncol * nOrd + d + nDir * p
    assert T + 2 * nOrd + 2 * ncol * nOrd + nDir * nOrd + ncol * nDir * nOrd == M  # nothing after the tail
    # the order-blind part is where it always was
    plain = driver.unpack_moments(_synthetic(nx, ny, nz, nDir, -1)[0], nx, ny, nz)
    for k, v in plain.items():
        if k not in ("totalPhotons", "batches"):
            assert np.array_equal(out[k][0], v[0]) and np.array_equal(out[k][1], v[1]), k
    # statistics carries the new names through with no change of its own
    st = driver.statistics(out)
    for k in ("meanFluxUpByScatOrd", "fluxDownByScatOrd", "intensityByScatOrd"):
        assert k in st and k + "_StdErr" in st


def test_unpack_moments_flux_only_orders_and_default_unchanged():
    from mcbrat3d_amd import driver
    nx, ny, nz, N = 4, 3, 2, 5
    buf, M = _synthetic(nx, ny, nz, 0, N)
    out = driver.unpack_moments(buf, nx, ny, nz, nDirections=0, numRecScatOrd=N)
    assert out["fluxUpByScatOrd"][0].shape == (nx, ny, N + 1)
    assert "intensityByScatOrd" not in out and "intensity" not in out
    with pytest.raises(ValueError):  # the length no longer tells the number of directions
        driver.unpack_moments(buf, nx, ny, nz, numRecScatOrd=N)
    # default: the same names and values as before for buffers with and without directions
    for nDir in (0, 3):
        plain, _ = _synthetic(nx, ny, nz, nDir, -1)
        a = driver.unpack_moments(plain, nx, ny, nz)
        b = driver.unpack_moments(plain, nx, ny, nz, numRecScatOrd=-1)
        assert sorted(a) == sorted(b) and not any("ScatOrd" in k for k in a)
        assert ("intensity" in a) == (nDir > 0)


def _stats(nx, ny, nDir, N, seed=3):
    rng = np.random.default_rng(seed)
    st = {"totalPhotons": 100000, "batches": 10}
    for k in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        st[k] = rng.random((nx, ny))
        st[k + "_StdErr"] = rng.random((nx, ny)) * 1e-3
    for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed"):
        st[k], st[k + "_StdErr"] = float(rng.random()), 1e-4
    if nDir:
        st["intensity"], st["intensity_StdErr"] = rng.random((nx, ny, nDir)), rng.random((nx, ny, nDir)) * 1e-3
    if N >= 0:
        for k in ("fluxUpByScatOrd", "fluxDownByScatOrd"):
            st[k], st[k + "_StdErr"] = rng.random((nx, ny, N + 1)), rng.random((nx, ny, N + 1)) * 1e-3
        if nDir:
            st["intensityByScatOrd"] = rng.random((nx, ny, nDir, N + 1))
            st["intensityByScatOrd_StdErr"] = rng.random((nx, ny, nDir, N + 1)) * 1e-3
    return st


def test_netcdf_writer_reference_names_by_order(tmp_path):
    from mcbrat3d_amd import ncio
    nx, ny, nDir, N = 4, 3, 2, 3
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.linspace(0, 2, 6)
    st = _stats(nx, ny, nDir, N)
    mus, phis = np.array([1.0, 0.5], np.float32), np.array([0.0, 90.0], np.float32)
    out = ncio.writeResults_netcdf(str(tmp_path / "o.nc"), "dom", st, xe, ye, ze, intensityMus=mus, intensityPhis=phis)
    f = netcdf_file(out, "r", mmap=False)
    try:
        assert f.dimensions["numRecScatOrd"] == N + 1
        assert int(f.Highest_recorded_scattering_order) == N
        assert np.array_equal(f.variables["Scattering_Order"][:], np.arange(N + 1, dtype=np.float32))
        for k in ("fluxUpByScatOrd", "fluxDownByScatOrd", "fluxUpByScatOrd_StdErr", "fluxDownByScatOrd_StdErr"):
            v = f.variables[k]
            assert v.dimensions == ("numRecScatOrd", "y", "x")  # Fortran (x, y, numRecScatOrd)
            assert np.array_equal(np.asarray(v[:]).transpose(2, 1, 0), st[k].astype(np.float32))
        for k in ("intensityByScatOrd", "intensityByScatOrd_StdErr"):
            v = f.variables[k]
            assert v.dimensions == ("numRecScatOrd", "direction", "y", "x")  # Fortran (x, y, direction, numRecScatOrd)
            assert np.array_equal(np.asarray(v[:]).transpose(3, 2, 1, 0), st[k].astype(np.float32))
    finally:
        f.close()


def test_netcdf_writer_without_orders_is_unchanged(tmp_path):
    """A file from stats without orders carries none of the new names, and equals the file written from stats whose order
    entries are dropped: the order branch adds nothing to it."""
    from mcbrat3d_amd import ncio
    nx, ny = 4, 3
    xe, ye, ze = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.linspace(0, 2, 6)
    withOrders = _stats(nx, ny, 0, 2)
    plain = {k: v for k, v in withOrders.items() if "ScatOrd" not in k}
    a = ncio.writeResults_netcdf(str(tmp_path / "a.nc"), "dom", plain, xe, ye, ze)
    b = ncio.writeResults_netcdf(str(tmp_path / "b.nc"), "dom", _stats(nx, ny, 0, -1), xe, ye, ze)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(a, "r", mmap=False)
    try:
        assert "numRecScatOrd" not in f.dimensions and "Scattering_Order" not in f.variables
        assert not hasattr(f, "Highest_recorded_scattering_order")
    finally:
        f.close()
    c = ncio.writeResults_netcdf(str(tmp_path / "c.nc"), "dom", withOrders, xe, ye, ze)
    assert open(c, "rb").read() != open(a, "rb").read()


def test_spectral_run_refuses_orders():
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband
    from mcbrat3d_amd._capi import McbratError
    with pytest.raises(McbratError, match="scattering order"):
        broadband.SpectralRun(M, [object()], recScatOrd=True, numRecScatOrd=3)


def test_namelist_reads_scattering_order_keywords(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "r.nml"
    nml.write_text("&output recScatOrd = .true., numRecScatOrd = 7 /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["recscatord"] is True and cfg["numrecscatord"] == 7
    nml.write_text("&output /\n")
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["recscatord"] is False and cfg["numrecscatord"] == 0  # the reference driver's defaults (:98-99)


def test_fortran_shim_declares_scattering_order_entries(tmp_path):
    flang = shutil.which("amdflang") or ("/opt/rocm/llvm/bin/amdflang" if os.path.exists("/opt/rocm/llvm/bin/amdflang") else None)
    if flang is None:
        pytest.skip("no Fortran compiler")
    src = os.path.join(ROOT, "fortran", "mcbrat_hip_integrator.f90")
    subprocess.check_call([flang, "-O2", "-c", src, "-o", str(tmp_path / "shim.o")], cwd=str(tmp_path))
    text = open(src).read().replace("&\n", " ")
    for name in ("specifyScatteringOrders", "reportResultsByScatOrd"):
        assert re.search(r"public ::[^!]*\b%s\b" % name, text), name
    for sym in ("mcbrat_specify_scattering_orders", "mcbrat_report_scattering_orders"):
        assert 'name="%s"' % sym in text
    # and the driver compiles against it
    subprocess.check_call([flang, "-O2", "-c", os.path.join(ROOT, "fortran", "mcbrat_driver.f90"), "-o", str(tmp_path / "drv.o")],
                          cwd=str(tmp_path))
