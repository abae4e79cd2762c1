"""`python -m mcbrat3d_amd.driver_cli run.nml` -- the reference driver's surface around the HIP
integrator: the five namelists of Drivers/monteCarloDriver.f95:103-121 (same names and defaults,
:58-99), a `.dom` domain file (ncio.read_Domain) or a built-in I3RC generator, batch statistics
(:1188-1228) and the ASCII / NetCDF writers (:1324-1495, :1499-1807).

Monochromatic solar runs (LW_flag < 0).  One process per GPU: start it with
`python -m torch.distributed.run --nproc-per-node N -m mcbrat3d_amd.driver_cli run.nml` to shard the
batches over N GPUs; rank 0 writes the output."""
import os
import re
import sys
import time

import numpy as np

DEFAULTS = {  # monteCarloDriver.f95:58-99
    "radiativetransfer": dict(solarmu=1.0, solarazimuth=0.0, surfacetemp=300.0, lw_flag=-1.0, numlambda=1, calcrayl=True,
                              intensitymus=[], intensityphis=[]),
    "montecarlo": dict(numphotonsperbatch=0, numbatches=100, iseed=10, nphaseintervals=10001),
    "algorithms": dict(useraytracing=True, userussianroulette=True, usehybridphasefunsforintencalcs=False,
                       hybridphasefunwidth=7.0, numordersorigphasefunintencalcs=0, userussianrouletteforintensity=True,
                       zetamin=0.3, limitintensitycontributions=False, maxintensitycontribution=77.0),
    "output": dict(reportvolumeabsorption=False, reportabsorptionprofile=False, recscatord=False, numrecscatord=0,
                   reportlevelfluxes=False, reportdirectlevelfluxes=False, reportactinicflux=False, reportsidefluxes=False),
    "filenames": dict(physdomainfile="", domainfilename="", sspfilename="", solarsourcefile="", instrresponsefile="",
                      outputfluxfile="", outputabsproffile="", outputabsvolumefile="", outputnetcdffile="", outputradfile=""),
    # the backward camera (no counterpart in the reference driver): absent -- cameraKind empty -- it changes
    # nothing.  cameraFootprint = xLo, xHi, yLo, yHi (default: the domain), cameraHeight (default: the top of the domain).
    # emission = .true. (here and in /sensors/; read as cameraEmission and sensorsEmission): the emission render of DESIGN.md
    # section 4.22 on the Planck radiances of the domain's temperatures and surfaceTemp, instead of the solar one.
    # emissionEstimator = 'collision' | 'expected' (here and in /sensors/, read as emission is): the estimator of the emission
    # render, 'expected' the expected-value one of DESIGN.md section 4.24; an error where it is given without emission = .true.
    "camera": dict(camerakind="", camerapixels=[1, 1], cameraposition=[0.0, 0.0, 0.0], cameralook=[0.0, 0.0, -1.0],
                   cameraup=[0.0, 1.0, 0.0], camerafov=60.0, cameramu=1.0, cameraphi=0.0, camerafootprint=[], cameraheight=None,
                   camerasamplesperpixel=1000, camerabatches=10, outputcamerafile="", emission=False, emissionestimator="collision",
                   # pathLengthEdges = 0., e1, ...: the image also by photon path length, the bins' lower edges
                   pathlengthedges=[]),
    # backward sensors (no counterpart in the reference driver): absent -- sensorKind empty -- they change
    # nothing.  sensorPositions = x, y, z of every sensor in turn; sensorTilt, sensorAzimuth in degrees, one for all or one per sensor
    "sensors": dict(sensorkind="", sensorpositions=[], sensortilt=0.0, sensorazimuth=0.0, sensorsamples=10000, sensorbatches=10,
                    outputsensorfile="", emission=False, emissionestimator="collision"),
}


def _value(tok):
    t = tok.strip()
    if not t:
        return None
    if t[0] in "'\"":
        return t[1:-1]
    low = t.lower().strip(".")
    if low in ("true", "t"):
        return True
    if low in ("false", "f"):
        return False
    try:
        return int(t)
    except ValueError:
        return float(t.lower().replace("d", "e"))


def read_namelists(path):
    """Minimal Fortran namelist reader: &group key = value[, value...] ... /"""
    text = open(path).read()
    text = re.sub(r"!.*", "", text)
    groups = {}
    for m in re.finditer(r"&(\w+)(.*?)(?:^|\s)/", text, re.S | re.M):
        body = m.group(2)
        keys = list(re.finditer(r"(\w+)\s*=", body))
        items = {}
        for k, nxt in zip(keys, keys[1:] + [None]):
            raw = body[k.end():nxt.start() if nxt else len(body)]
            vals = [_value(v) for v in re.findall(r"'[^']*'|\"[^\"]*\"|[^,\s]+", raw)]
            vals = [v for v in vals if v is not None]
            items[k.group(1).lower()] = vals[0] if len(vals) == 1 else vals
        groups[m.group(1).lower()] = items
    cfg = {}
    for g, d in DEFAULTS.items():
        cfg.update({k.lower(): v for k, v in d.items()})
        cfg.update(groups.get(g, {}))
        if "emission" in d:  # (one key in two groups: kept apart as cameraemission and sensorsemission)
            cfg[g + "emission"] = bool(cfg.pop("emission"))
            estimator = cfg.pop("emissionestimator")
            if estimator not in ("collision", "expected"):
                raise SystemExit("%s: emissionEstimator must be 'collision' or 'expected' (got %r)." % (g, estimator))
            if estimator == "expected" and not cfg[g + "emission"]:
                raise SystemExit("%s: emissionEstimator = 'expected' needs emission = .true. (the solar render has one estimator)." % g)
            cfg[g + "emissionestimator"] = estimator
    return cfg


def writeResults_ASCII(path, cfg, domainName, stats, xe, ye, ze, solarFlux, albedo):
    """Flux file, monteCarloDriver.f95:1376-1399."""
    b = lambda v: "T" if v else "F"  # noqa: E731
    with open(path, "w") as f:
        f.write("!   I3RC Monte Carlo 3D Solar Radiative Transfer: Flux\n")
        f.write("!  Property_File=%60s\n" % domainName[:60])
        f.write("!  Num_Photons=%10d\n" % stats["totalPhotons"])
        f.write("!  PhotonTracing=%s    Russian_Roulette=%s\n" % (b(cfg["useraytracing"]), b(cfg["userussianroulette"])))
        f.write("!  Hybrid_Phase_Func_for_Radiance=F   Gaussian_Phase_Func_Width_deg= 7.00\n")
        f.write("!  Solar_Flux=%13.6E   Solar_Mu=%10.7f   Solar_Phi=%7.3f\n" % (solarFlux, cfg["solarmu"], cfg["solarazimuth"]))
        f.write("!  Lambertian_Surface_Albedo=%7.4f\n" % albedo)
        f.write("!  Output_Type= Pixel Flux\n")
        f.write("!  Upwelling_Level=%7.3f   Downwelling_level=%7.3f\n" % (ze[-1], ze[0]))
        f.write("!   X      Y           Flux_Up             Flux_Down            Flux_Absorbed \n")
        f.write("!                  Mean     StdErr       Mean     StdErr       Mean     StdErr\n")
        f.write("!  Average:   " + "".join(" %10.4f%10.4f" % (stats[k], stats[k + "_StdErr"])
                                           for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed")) + "\n")
        for j in range(len(ye) - 1):
            for i in range(len(xe) - 1):
                f.write("%7.3f%7.3f" % (0.5 * (xe[i] + xe[i + 1]), 0.5 * (ye[j] + ye[j + 1])) +
                        "".join(" %10.4f%10.4f" % (stats[k][i, j], stats[k + "_StdErr"][i, j])
                                for k in ("fluxUp", "fluxDown", "fluxAbsorbed")) + "\n")


def writeResults_ASCII_radiance(path, cfg, domainName, stats, xe, ye, ze, solarFlux, albedo, mus, phis):
    """The radiance file, monteCarloDriver.f95:1459-1494."""
    nx, ny, nz = len(xe) - 1, len(ye) - 1, len(ze) - 1
    b = lambda v: "T" if v else "F"  # noqa: E731
    with open(path, "w") as f:
        f.write("!   I3RC Monte Carlo 3D Solar Radiative Transfer: Radiance\n")
        f.write("!  Property_File=%60s\n" % domainName[:60])
        f.write("!  Num_Photons=%10d\n" % int(stats["totalPhotons"]))
        f.write("!  PhotonTracing=%s    Russian_Roulette=%s\n" % (b(cfg["useraytracing"]), b(cfg["userussianroulette"])))
        f.write("!  Hybrid_Phase_Func_for_Radiance=%s   Gaussian_Phase_Func_Width_deg=%5.2f\n"
                % (b(cfg["usehybridphasefunsforintencalcs"]), cfg["hybridphasefunwidth"]))
        f.write("!  Intensity_uses_Russian_Roulette=%s   Intensity_Russian_Roulette_zeta_min=%5.2f\n"
                % (b(cfg["userussianrouletteforintensity"]), cfg["zetamin"]))
        f.write("!  limited_intensity_contributions=%s   max_intensity_contribution=%5.2f\n"
                % (b(cfg["limitintensitycontributions"]), cfg["maxintensitycontribution"]))
        f.write("!  Solar_Flux=%13.6E   Solar_Mu=%10.7f   Solar_Phi=%7.3f\n" % (solarFlux, cfg["solarmu"], cfg["solarazimuth"]))
        f.write("!  Lambertian_Surface_Albedo=%7.4f\n" % albedo)
        f.write("!  Output_Type= Pixel Radiance\n")
        f.write("!  RADIANCE AT Z=%7.3f   NXO=%4d   NYO=%4d   NDIR=%4d\n" % (ze[nz], nx, ny, len(mus)))
        f.write("!   X      Y         Radiance (Mean, StdErr)\n")
        for k in range(len(mus)):
            f.write("!  %8.5f %6.2f  <- (mu,phi)\n" % (mus[k], phis[k]))
            for j in range(ny):
                for i in range(nx):
                    f.write("%7.3f%7.3f %9.4f %9.4f\n" % (0.5 * (xe[i] + xe[i + 1]), 0.5 * (ye[j] + ye[j + 1]),
                                                        stats["intensity"][i, j, k], stats["intensity_StdErr"][i, j, k]))


def path_length_edges(cfg):
    """pathLengthEdges of the /camera/ group as an array of floats, or None where the key is absent (the library checks them)."""
    edges = np.atleast_1d(np.asarray(cfg.get("pathlengthedges", []), np.float32)).reshape(-1)
    return edges if edges.size else None


def camera_from_namelist(cfg, xe, ye, ze):
    """The camera of the /camera/ group (None where cameraKind is empty), with the domain for the defaults of the footprint and
    the height."""
    from mcbrat3d_amd.camera import new_Camera
    kind = str(cfg["camerakind"]).strip().lower()
    if not kind:
        return None
    pixels = np.atleast_1d(cfg["camerapixels"]).astype(int)
    npx, npy = int(pixels[0]), int(pixels[1] if pixels.size > 1 else pixels[0])
    if kind == "orthographic":
        fp = list(np.atleast_1d(cfg["camerafootprint"]).astype(float)) or [xe[0], xe[-1], ye[0], ye[-1]]
        height = ze[-1] if cfg["cameraheight"] is None else float(cfg["cameraheight"])
        return new_Camera(kind, npx=npx, npy=npy, mu=float(cfg["cameramu"]), phi=float(cfg["cameraphi"]), footprint=fp, height=height)
    return new_Camera(kind, npx=npx, npy=npy, position=cfg["cameraposition"], look=cfg["cameralook"], up=cfg["cameraup"],
                      fov=float(cfg["camerafov"]))


def sensors_from_namelist(cfg):
    """The sensors of the /sensors/ group (None where sensorKind is empty)."""
    from mcbrat3d_amd.sensors import new_Sensors
    from mcbrat3d_amd._capi import McbratError
    kind = str(cfg["sensorkind"]).strip().lower()
    if not kind:
        return None
    pos = np.atleast_1d(np.asarray(cfg["sensorpositions"], np.float64)).reshape(-1)
    if pos.size < 3 or pos.size % 3:
        raise McbratError("sensorPositions: x, y, z of at least one sensor are needed (a multiple of three numbers).")
    if int(cfg["sensorsamples"]) < 1 or int(cfg["sensorbatches"]) < 1:
        raise McbratError("sensorSamples and sensorBatches must be at least 1.")
    return new_Sensors(pos.reshape(-1, 3), tilt=cfg["sensortilt"], azimuth=cfg["sensorazimuth"], kind=kind)


def builtin_domain(name):
    """Domain-Files/i3rcStepCloud.f95, planeParallel.f95 (km)."""
    import mcbrat3d_amd as M
    g = float(np.float32(0.85))
    coef = np.array([g ** l for l in range(1, 65)]).astype(np.float32)
    table = M.new_PhaseFunctionTable([M.new_PhaseFunction(coef)])
    ssa = 1.0 if "Conservative" in name else 0.99
    if name.startswith("i3rcStepCloud"):
        nx = 32
        xe = 0.015625 * np.arange(nx + 1)
        ext = np.zeros((nx, 1, 32)); ext[:16] = 8.0; ext[16:] = 72.0
    elif name.startswith("planeParallel"):
        xe = np.array([0.0, 0.5])
        ext = np.full((1, 1, 32), 2.0)
    else:
        raise SystemExit("unknown builtin domain " + name)
    dom = M.new_Domain(xe, [0.0, 0.5], 0.0078125 * np.arange(33), surfaceAlbedo=0.0)
    dom.addOpticalComponent("cloud", ext, np.full_like(ext, ssa), np.ones(ext.shape, np.int32), table)
    return dom


def load_domains(cfg):
    """The optical domain of every wavelength of the run.  The current driver's file family (monteCarloDriver.f95:299,
    :936): `physDomainFile` (read_Common) + up to four `SSPfilename` tables (read_SSPTable), numLambda wavelengths,
    Rayleigh scattering added when calcRayl.  Otherwise one domain: a `.dom` file (read_Domain) or a built-in I3RC
    generator ("builtin:i3rcStepCloud")."""
    from mcbrat3d_amd import ncio
    ssp = cfg["sspfilename"]
    ssp = [ssp] if isinstance(ssp, str) else list(ssp)
    ssp = [n for n in ssp if n]
    if ssp:
        if not cfg["physdomainfile"]:
            raise SystemExit("SSPfilename given without physDomainFile")
        common = ncio.read_Common(cfg["physdomainfile"])
        return [ncio.read_SSPTable(ssp, i, common, setup=False, calcRayl=bool(cfg["calcrayl"]))
                for i in range(1, int(cfg["numlambda"]) + 1)]
    domfile = cfg["physdomainfile"] or cfg["domainfilename"]
    dom = builtin_domain(domfile[8:]) if domfile.startswith("builtin:") else ncio.read_Domain(domfile)
    dom.getOpticalPropertiesByComponent()
    return [dom]


def run_spectral(cfg, doms, rank, world, local, dist):
    """Spectrally integrated run (numLambda > 1, or thermal emission): every wavelength resident on the GPU
    (broadband.SpectralRun), photons split over wavelengths on the device, ranks take contiguous blocks of batches."""
    import mcbrat3d_amd as M
    from mcbrat3d_amd import broadband, driver, ncio
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    run = broadband.SpectralRun(M, doms, device=local, minInverseTableSize=cfg["nphaseintervals"],
                                useRayTracing=cfg["useraytracing"], useRussianRoulette=cfg["userussianroulette"])
    if cfg["lw_flag"] >= 0:
        flux = run.prepare_thermal(cfg["surfacetemp"])
    else:
        nlam = len(doms)
        if not cfg["solarsourcefile"]:
            raise SystemExit("a solar run over several wavelengths needs solarSourceFile")
        src, lam = ncio.read_SolarSource(cfg["solarsourcefile"], nlam)
        srf = ncio.read_specResponseFunction(cfg["instrresponsefile"], nlam) if cfg["instrresponsefile"] else None
        flux = run.prepare_solar(cfg["solarmu"], cfg["solarazimuth"], src, lam, srf)
    ppb, nbAll = int(cfg["numphotonsperbatch"]), int(cfg["numbatches"])
    lo, nb = driver.split_batches(nbAll, rank, world)
    moments = None
    if dist is not None:
        import torch
        moments = torch.zeros(8 + 2 * run.first.momentsLength(), dtype=torch.float64, device="cuda:%d" % local)
        run.bindMoments(moments.data_ptr())
    run.resetMoments()
    if nb > 0:
        # this rank's photons: ids and wavelength draws [lo * ppb, (lo + nb) * ppb)
        counts = broadband.device_frequency_distribution(run.first, run.cdf, ppb * nb, cfg["iseed"], firstDraw=lo * ppb)
        run.run(ppb, nb, new_RandomNumberSequence(cfg["iseed"], lo * ppb), seed=cfg["iseed"], counts=counts)
    for it in run.integrators:
        it.synchronize()
    if dist is not None and world > 1:
        import torch
        dist.all_reduce(moments, op=dist.ReduceOp.SUM)  # sumAcrossProcesses, monteCarloDriver.f95:1151-1166
        torch.cuda.synchronize()
        buf = moments.cpu().numpy()
    else:
        buf = run.moments()
    nx, ny, nz = run.first._dims
    stats = driver.statistics(driver.unpack_moments(buf, nx, ny, nz), solarFlux=flux)
    run.finalize()
    return stats, flux


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit("usage: python -m mcbrat3d_amd.driver_cli <namelist file>")
    t0 = time.time()
    cfg = read_namelists(argv[0])
    if cfg["numphotonsperbatch"] <= 0:
        raise SystemExit("must specify numPhotonsPerBatch")
    import mcbrat3d_amd as M
    from mcbrat3d_amd import driver, ncio
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    domfile = cfg["physdomainfile"] or cfg["domainfilename"]
    doms = load_domains(cfg)
    dom = doms[0]
    # scattering orders (:98-115): recorded when asked for, and -- as the reference driver reads it (:284-287) -- not for a
    # negative numRecScatOrd
    numRecScatOrd = int(cfg["numrecscatord"]) if cfg["recscatord"] and int(cfg["numrecscatord"]) >= 0 else -1
    if len(doms) > 1 or cfg["lw_flag"] >= 0:
        if numRecScatOrd >= 0:
            raise SystemExit("recScatOrd: fluxes and radiances by scattering order are not available for spectrally integrated "
                             "runs (numLambda > 1 or thermal emission)")
        if cfg["reportlevelfluxes"]:
            raise SystemExit("reportLevelFluxes: level fluxes are not available for spectrally integrated runs (numLambda > 1 "
                             "or thermal emission)")
        if cfg["reportdirectlevelfluxes"]:
            raise SystemExit("reportDirectLevelFluxes: direct level fluxes are not available for spectrally integrated runs "
                             "(numLambda > 1 or thermal emission)")
        if cfg["reportactinicflux"]:
            raise SystemExit("reportActinicFlux: the actinic flux is not available for spectrally integrated runs (numLambda > 1 "
                             "or thermal emission)")
        if cfg["reportsidefluxes"]:
            raise SystemExit("reportSideFluxes: side fluxes are not available for spectrally integrated runs (numLambda > 1 or "
                             "thermal emission)")
        if str(cfg["camerakind"]).strip():
            raise SystemExit("cameraKind: the backward camera is not available for spectrally integrated runs (numLambda > 1 or "
                             "thermal emission)")
        if str(cfg["sensorkind"]).strip():
            raise SystemExit("sensorKind: the backward sensors are not available for spectrally integrated runs (numLambda > 1 or "
                             "thermal emission)")
        setup = time.time() - t0
        stats, flux = run_spectral(cfg, doms, rank, world, local, dist)
        if rank == 0:
            print(" spectrally integrated flux %.6g; mean flux up/down/absorbed: " % flux +
                  "  ".join("%9.6f +-%9.6f" % (stats[k], stats[k + "_StdErr"]) for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed")))
            xe, ye, ze = dom.xPosition, dom.yPosition, dom.zPosition
            if cfg["outputfluxfile"]:
                writeResults_ASCII(cfg["outputfluxfile"], cfg, domfile, stats, xe, ye, ze, flux, dom.surfaceAlbedo)
            if cfg["outputnetcdffile"]:
                ncio.writeResults_netcdf(cfg["outputnetcdffile"], domfile, stats, xe, ye, ze, solarFlux=flux, solarMu=cfg["solarmu"],
                                         solarAzimuth=cfg["solarazimuth"], surfaceAlbedo=dom.surfaceAlbedo, iseed=cfg["iseed"],
                                         nPhaseIntervals=cfg["nphaseintervals"], reportAbsorptionProfile=cfg["reportabsorptionprofile"],
                                         reportVolumeAbsorption=cfg["reportvolumeabsorption"], cpuTimeTotal=time.time() - t0,
                                         cpuTimeSetup=setup, numProcs=world)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return stats
    integ = M.new_Integrator(dom, device=local)
    integ.specifyParameters(minInverseTableSize=cfg["nphaseintervals"], useRayTracing=cfg["useraytracing"],
                            useRussianRoulette=cfg["userussianroulette"], LW_flag=cfg["lw_flag"])
    # intensity directions: every entry with |mu| > 0, and only if a file will hold them (monteCarloDriver.f95:279-282)
    mus = np.atleast_1d(np.asarray(cfg["intensitymus"], np.float32))
    phis = np.atleast_1d(np.asarray(cfg["intensityphis"], np.float32))
    if phis.size < mus.size:
        phis = np.concatenate([phis, np.zeros(mus.size - phis.size, np.float32)])
    keep = np.abs(mus) > 0.0
    mus, phis = mus[keep], phis[:mus.size][keep]
    computeIntensity = mus.size > 0 and bool(cfg["outputradfile"] or cfg["outputnetcdffile"])
    if computeIntensity:  # :547-552, :579-594
        integ.specifyParameters(minForwardTableSize=cfg["nphaseintervals"], intensityMus=mus, intensityPhis=phis,
                                computeIntensity=True,
                                useHybridPhaseFunsForIntenCalcs=cfg["usehybridphasefunsforintencalcs"],
                                hybridPhaseFunWidth=cfg["hybridphasefunwidth"],
                                numOrdersOrigPhaseFunIntenCalcs=cfg["numordersorigphasefunintencalcs"],
                                useRussianRouletteForIntensity=cfg["userussianrouletteforintensity"], zetaMin=cfg["zetamin"],
                                limitIntensityContributions=cfg["limitintensitycontributions"],
                                maxIntensityContribution=cfg["maxintensitycontribution"])
    if numRecScatOrd >= 0:
        integ.specifyParameters(recScatOrd=True, numRecScatOrd=numRecScatOrd)
    if cfg["reportlevelfluxes"]:  # (refused by specifyParameters together with intensity directions or scattering orders)
        integ.specifyParameters(recLevelFluxes=True)
    if cfg["reportdirectlevelfluxes"]:  # (refused by specifyParameters without reportLevelFluxes)
        integ.specifyParameters(recDirectLevelFluxes=True)
    if cfg["reportactinicflux"]:  # (refused by specifyParameters together with directions, orders or the direct level tally)
        integ.specifyParameters(recActinicFlux=True)
    if cfg["reportsidefluxes"]:  # (refused by specifyParameters without reportLevelFluxes, with the direct tally or the actinic flux)
        integ.specifyParameters(recSideFluxes=True)
    camera = camera_from_namelist(cfg, dom.xPosition, dom.yPosition, dom.zPosition)  # (a bad camera ends the run before it traces)
    sensors = sensors_from_namelist(cfg)  # (bad sensors end the run before it traces)
    photons = M.new_PhotonStream(cfg["solarmu"], cfg["solarazimuth"], numberOfPhotons=cfg["numphotonsperbatch"] * cfg["numbatches"])
    moments = None
    if dist is not None:
        import torch
        moments = torch.zeros(8 + 2 * integ.momentsLength(), dtype=torch.float64, device="cuda:%d" % local)
        integ.bindMoments(moments.data_ptr())
    setup = time.time() - t0
    stats = driver.run(integ, dom, photons, cfg["numphotonsperbatch"], cfg["numbatches"], new_RandomNumberSequence(cfg["iseed"]),
                       solarFlux=1.0, dist=dist, moments_tensor=moments)
    cameraResult = None
    if camera is not None and rank == 0:  # the image: rank 0 renders it after the forward run, with sample indices of its own stream
        if cfg["cameraemission"]:
            cellSource, surfaceSource = M.planck_sources(dom, cfg["surfacetemp"])
            cameraResult = integ.renderCameraEmission(camera, new_RandomNumberSequence(cfg["iseed"]), int(cfg["camerasamplesperpixel"]),
                                                      int(cfg["camerabatches"]), cellSource=cellSource, surfaceSource=surfaceSource,
                                                      estimator=cfg["cameraemissionestimator"])
        else:
            cameraResult = integ.renderCamera(camera, new_RandomNumberSequence(cfg["iseed"]), int(cfg["camerasamplesperpixel"]),
                                              int(cfg["camerabatches"]))
        edges = path_length_edges(cfg)
        if edges is not None:  # the same paths once more, every estimate in the bin of its path length (the image itself stays what it was)
            if cfg["cameraemission"]:
                raise SystemExit("pathLengthEdges: an emission render has no path-length bins.")
            byLength = integ.renderCameraPathLengths(camera, edges, int(cfg["camerasamplesperpixel"]), int(cfg["camerabatches"]),
                                                     seed=new_RandomNumberSequence(cfg["iseed"]).seed, firstSample=0)
            cameraResult.update(radianceByPathLength=byLength["radiance"], radianceByPathLength_StdErr=byLength["radiance_StdErr"],
                                pathLengthEdges=byLength["pathEdges"], dropped=cameraResult["dropped"] + byLength["dropped"])
        cameraResult["samplesPerPixel"] = int(cfg["camerasamplesperpixel"])
        print(" camera %s %d x %d: mean radiance %.6g, largest standard error %.3g, %d paths dropped" % (
            camera.kind, camera.npx, camera.npy, cameraResult["radiance"].mean(), cameraResult["radiance_StdErr"].max(), cameraResult["dropped"]))
        if cfg["outputcamerafile"]:
            ncio.writeCamera_netcdf(cfg["outputcamerafile"], camera, cameraResult)
    sensorResult = None
    if sensors is not None and rank == 0:  # rank 0 renders the sensors after the forward run, with sample indices of their own stream
        if cfg["sensorsemission"]:
            cellSource, surfaceSource = M.planck_sources(dom, cfg["surfacetemp"])
            sensorResult = integ.renderSensorsEmission(sensors, new_RandomNumberSequence(cfg["iseed"]), int(cfg["sensorsamples"]),
                                                       int(cfg["sensorbatches"]), cellSource=cellSource, surfaceSource=surfaceSource,
                                                       estimator=cfg["sensorsemissionestimator"])
        else:
            sensorResult = integ.renderSensors(sensors, new_RandomNumberSequence(cfg["iseed"]), int(cfg["sensorsamples"]), int(cfg["sensorbatches"]))
        sensorResult["samplesPerSensor"] = int(cfg["sensorsamples"])
        for i in range(len(sensors)):
            if cfg["sensorsemission"]:
                print(" sensor %3d %-9s at %9.4f %9.4f %9.4f: emitted %12.6g +-%12.6g" % (
                    i, sensors.kindNames()[i], *sensors.positions[i], sensorResult["irradiance"][i], sensorResult["irradiance_StdErr"][i]))
                continue
            print(" sensor %3d %-9s at %9.4f %9.4f %9.4f: %9.6f +-%9.6f  direct/diffuse: %9.6f  %9.6f" % (
                i, sensors.kindNames()[i], *sensors.positions[i], sensorResult["irradiance"][i], sensorResult["irradiance_StdErr"][i],
                sensorResult["direct"][i], sensorResult["diffuse"][i]))
        print(" sensors: %d paths dropped" % sensorResult["dropped"])
        if cfg["outputsensorfile"]:
            ncio.writeSensors_netcdf(cfg["outputsensorfile"], sensors, sensorResult)
    if rank == 0:
        print(" mean flux up/down/absorbed: " + "  ".join("%9.6f +-%9.6f" % (stats[k], stats[k + "_StdErr"])
                                                            for k in ("meanFluxUp", "meanFluxDown", "meanFluxAbsorbed")))
        if numRecScatOrd >= 0:  # domain-mean fluxes by scattering order, one line per order
            for p in range(numRecScatOrd + 1):
                print(" order %3d mean flux up/down: %9.6f +-%9.6f  %9.6f +-%9.6f" % (
                    p, stats["meanFluxUpByScatOrd"][p], stats["meanFluxUpByScatOrd_StdErr"][p],
                    stats["meanFluxDownByScatOrd"][p], stats["meanFluxDownByScatOrd_StdErr"][p]))
        if cfg["reportlevelfluxes"]:  # domain-mean fluxes through every level, one line per level from the top down
            for k in range(len(dom.zPosition) - 1, -1, -1):
                print(" level %3d z %9.4f mean flux up/down: %9.6f +-%9.6f  %9.6f +-%9.6f" % (
                    k, dom.zPosition[k], stats["meanLevelFluxUp"][k], stats["meanLevelFluxUp_StdErr"][k],
                    stats["meanLevelFluxDown"][k], stats["meanLevelFluxDown_StdErr"][k]) + (
                    "  direct/diffuse: %9.6f +-%9.6f  %9.6f +-%9.6f" % (
                        stats["meanLevelFluxDownDirect"][k], stats["meanLevelFluxDownDirect_StdErr"][k],
                        stats["meanLevelFluxDownDiffuse"][k], stats["meanLevelFluxDownDiffuse_StdErr"][k])
                    if cfg["reportdirectlevelfluxes"] else ""))
        if cfg["reportactinicflux"]:  # layer means of the actinic flux, one line per layer from the top down
            for k in range(len(dom.zPosition) - 2, -1, -1):
                print(" layer %3d z %9.4f - %9.4f mean actinic flux: %9.6f +-%9.6f" % (
                    k, dom.zPosition[k], dom.zPosition[k + 1], stats["meanActinicFlux"][k], stats["meanActinicFlux_StdErr"][k]))
        if cfg["reportsidefluxes"]:  # layer means of the four side fluxes, one line per layer from the top down
            for k in range(len(dom.zPosition) - 2, -1, -1):
                print(" layer %3d z %9.4f - %9.4f mean side flux x+ x- y+ y-: %9.6f %9.6f %9.6f %9.6f" % (
                    k, dom.zPosition[k], dom.zPosition[k + 1], stats["meanSideFluxXPlus"][k], stats["meanSideFluxXMinus"][k],
                    stats["meanSideFluxYPlus"][k], stats["meanSideFluxYMinus"][k]))
        xe, ye, ze = dom.xPosition, dom.yPosition, dom.zPosition
        if cfg["outputfluxfile"]:
            writeResults_ASCII(cfg["outputfluxfile"], cfg, domfile, stats, xe, ye, ze, 1.0, dom.surfaceAlbedo)
        if cfg["outputradfile"] and computeIntensity:
            writeResults_ASCII_radiance(cfg["outputradfile"], cfg, domfile, stats, xe, ye, ze, 1.0, dom.surfaceAlbedo, mus, phis)
        if cfg["outputnetcdffile"]:
            ncio.writeResults_netcdf(cfg["outputnetcdffile"], domfile, stats, xe, ye, ze, solarFlux=1.0, solarMu=cfg["solarmu"],
                                     solarAzimuth=cfg["solarazimuth"], surfaceAlbedo=dom.surfaceAlbedo, iseed=cfg["iseed"],
                                     nPhaseIntervals=cfg["nphaseintervals"],
                                     reportAbsorptionProfile=cfg["reportabsorptionprofile"],
                                     reportVolumeAbsorption=cfg["reportvolumeabsorption"],
                                     cpuTimeTotal=time.time() - t0, cpuTimeSetup=setup, numProcs=world,
                                     intensityMus=mus if computeIntensity else None,
                                     intensityPhis=phis if computeIntensity else None,
                                     useHybridPhaseFunsForIntenCalcs=cfg["usehybridphasefunsforintencalcs"],
                                     hybridPhaseFunWidth=cfg["hybridphasefunwidth"],
                                     useRussianRouletteForIntensity=cfg["userussianrouletteforintensity"], zetaMin=cfg["zetamin"],
                                     limitIntensityContributions=cfg["limitintensitycontributions"],
                                     maxIntensityContribution=cfg["maxintensitycontribution"],
                                     camera=camera, cameraResult=cameraResult, sensors=sensors, sensorResult=sensorResult)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    integ.finalize()
    return stats


if __name__ == "__main__":
    main()
