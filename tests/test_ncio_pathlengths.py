"""The driver surface of the radiance by photon path length without a GPU: the NetCDF variables
round-trip, a file written without them is byte for byte what the writer wrote before they existed, and the /camera/ group's
pathLengthEdges is parsed."""
import numpy as np
from scipy.io import netcdf_file


def _camera():
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=3, npy=2, position=(0.2, 0.25, 0.0), look=(0.2, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=70.0)


def _result(edges=None, seed=5):
    rng = np.random.default_rng(seed)
    r = {"radiance": rng.uniform(0.0, 1.0, (2, 3)).astype(np.float32), "radiance_StdErr": rng.uniform(0.0, 0.01, (2, 3)).astype(np.float32),
         "batchMeans": np.zeros((4, 2, 3), np.float32), "dropped": 0, "samplesPerPixel": 512}
    if edges is not None:
        n = len(edges)
        r.update(radianceByPathLength=rng.uniform(0.0, 1.0, (n, 2, 3)).astype(np.float32),
                 radianceByPathLength_StdErr=rng.uniform(0.0, 0.01, (n, 2, 3)).astype(np.float32), pathLengthEdges=np.asarray(edges, np.float32))
    return r


def test_the_path_length_variables_round_trip(tmp_path):
    from mcbrat3d_amd import ncio
    edges = [0.0, 0.25, 0.5, 1.0, 4.0]
    r = _result(edges)
    path = str(tmp_path / "camera.nc")
    ncio.writeCamera_netcdf(path, _camera(), r)
    f = netcdf_file(path, "r", mmap=False)
    try:
        assert f.dimensions["cameraPathBin"] == 5 and f.dimensions["cameraY"] == 2 and f.dimensions["cameraX"] == 3
        for name in ("cameraRadianceByPathLength", "cameraRadianceByPathLength_StdErr"):
            assert f.variables[name].dimensions == ("cameraPathBin", "cameraY", "cameraX")
        assert f.variables["cameraPathLengthEdges"].dimensions == ("cameraPathBin",)
    finally:
        f.close()
    back = ncio.readCamera_netcdf(path)
    # (the file holds big-endian floats: the values, bit for bit)
    assert np.array_equal(back["cameraRadianceByPathLength"], r["radianceByPathLength"]) and back["cameraRadianceByPathLength"].shape == (5, 2, 3)
    assert np.array_equal(back["cameraRadianceByPathLength_StdErr"], r["radianceByPathLength_StdErr"])
    assert np.array_equal(back["cameraPathLengthEdges"], np.asarray(edges, np.float32))
    assert np.array_equal(back["cameraRadiance"], r["radiance"]) and back["cameraBatches"] == 4
    assert ncio.CAMERA_PATH_VARIABLES == ("cameraRadianceByPathLength", "cameraRadianceByPathLength_StdErr", "cameraPathLengthEdges")


def _write_as_before(path, camera, result):
    """the camera file as the writer wrote it before the path-length variables existed, call for call"""
    f = netcdf_file(path, "w", version=2)
    try:
        f.description = "Backward Monte Carlo camera image"
        for name, value in camera.attributes().items():
            if isinstance(value, str):
                setattr(f, name, value)
            elif name in ("cameraPixels", "cameraJitter"):
                setattr(f, name, np.asarray(value, np.int32))
            else:
                setattr(f, name, np.asarray(value, np.float64))
        f.cameraSamplesPerPixel = np.float64(result.get("samplesPerPixel", 0))
        f.cameraBatches = np.int32(np.asarray(result["batchMeans"]).shape[0])
        f.cameraDroppedPaths = np.float64(result["dropped"])
        f.createDimension("cameraX", camera.npx)
        f.createDimension("cameraY", camera.npy)
        f.createVariable("cameraRadiance", "f", ("cameraY", "cameraX"))[:] = np.asarray(result["radiance"], np.float32)
        f.createVariable("cameraRadiance_StdErr", "f", ("cameraY", "cameraX"))[:] = np.asarray(result["radiance_StdErr"], np.float32)
    finally:
        f.close()


def test_a_file_without_the_key_is_byte_for_byte_what_it_was(tmp_path):
    from mcbrat3d_amd import ncio
    now, before, with_bins = (str(tmp_path / n) for n in ("now.nc", "before.nc", "bins.nc"))
    ncio.writeCamera_netcdf(now, _camera(), _result())
    _write_as_before(before, _camera(), _result())
    assert open(now, "rb").read() == open(before, "rb").read()
    ncio.writeCamera_netcdf(with_bins, _camera(), _result([0.0, 1.0]))
    assert open(with_bins, "rb").read() != open(now, "rb").read()
    back = ncio.readCamera_netcdf(now)
    assert not any(k in back for k in ncio.CAMERA_PATH_VARIABLES)


def test_the_namelist_key_is_parsed(tmp_path):
    from mcbrat3d_amd import driver_cli
    nml = tmp_path / "run.nml"
    head = "&radiativeTransfer solarMu = 0.5 /\n&fileNames physDomainFile = 'builtin:i3rcStepCloud' /\n"
    nml.write_text(head + "&camera cameraKind = 'pinhole', cameraPixels = 6, 4,\n pathLengthEdges = 0., 0.25, 0.5, 1., 2.5,\n cameraFov = 70. /\n")
    cfg = driver_cli.read_namelists(str(nml))
    edges = driver_cli.path_length_edges(cfg)
    assert edges.dtype == np.float32 and edges.tolist() == [0.0, 0.25, 0.5, 1.0, 2.5]
    assert cfg["camerafov"] == 70.0 and list(cfg["camerapixels"]) == [6, 4]
    nml.write_text(head + "&camera cameraKind = 'pinhole', pathLengthEdges = 0. /\n")     # one bin: the open one
    assert driver_cli.path_length_edges(driver_cli.read_namelists(str(nml))).tolist() == [0.0]
    nml.write_text(head + "&camera cameraKind = 'pinhole' /\n")                           # absent: no path-length render
    cfg = driver_cli.read_namelists(str(nml))
    assert cfg["pathlengthedges"] == [] and driver_cli.path_length_edges(cfg) is None
