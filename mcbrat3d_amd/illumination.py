"""Photon sources.  Mirrors src/monteCarloIllumination.f95 (new_PhotonStream:
Directional :62-101, RandomAzimuth :103-140, Flux :142-176, Spotlight :178-216 and
BBEmission :431-522 forms) and the part of
src/emissionAndBroadBandWeights.f95 the thermal source needs (new_Weights,
emission_weighting :424-550).

The reference pre-generates every photon of a batch on the host (32 B/photon);
here a PhotonStream only carries the source description and a count -- photons are
generated on the GPU from the counter-based generator."""
import ctypes as C

import numpy as np

from ._capi import McbratError, lib, ptr


class Weights:
    """type(Weights): running voxel CDF + fraction of power emitted by the atmosphere."""

    def __init__(self, numX, numY, numZ, numLambda=1):
        self.numX, self.numY, self.numZ, self.numLambda = numX, numY, numZ, numLambda
        self._version = 0  # bumped by emission_weighting: integrators re-upload the voxel CDF when it moves
        self.voxelWeights = None
        self.fracAtmsPower = 0.0
        self.spectrIntgrFlux = 0.0


def new_Weights(numX, numY, numZ, numLambda=1):
    return Weights(numX, numY, numZ, numLambda)


def emission_weighting(thisDomain, theseWeights, sfcTemp, dLambda=1.0):
    """emission_weightingNEW: fills theseWeights, returns the emitted flux [W m-2]."""
    info = thisDomain.getInfo_Domain()
    if info["temps"] is None:
        raise McbratError("emission_weighting: domain has no temperatures")
    nx, ny, nz, nc = info["numX"], info["numY"], info["numZ"], info["numberOfComponents"]
    temps = np.ascontiguousarray(info["temps"].transpose(2, 1, 0)).reshape(-1)  # x fastest
    vw = np.zeros(nx * ny * nz, np.float64)
    frac, flux = C.c_double(), C.c_double()
    tot = np.ascontiguousarray(info["totalExt"]).reshape(-1)
    cum = np.ascontiguousarray(info["cumExt"]).reshape(-1)
    ssa = np.ascontiguousarray(info["ssa"]).reshape(-1)
    rc = lib().mcbrat_emission_weighting(nx, ny, nz, nc, ptr(info["xPosition"]), ptr(info["yPosition"]),
                                         ptr(info["zPosition"]), ptr(temps), ptr(tot), ptr(cum), ptr(ssa),
                                         info["albedo"], thisDomain.lambda_um, float(sfcTemp), float(dLambda),
                                         ptr(vw), C.byref(frac), C.byref(flux))
    if rc != 0:
        raise McbratError("emission_weightingNEW: Neither surface nor atmosphere will emitt photons since "
                          "total power is 0. Not a valid solution")
    theseWeights.voxelWeights, theseWeights.fracAtmsPower, theseWeights.spectrIntgrFlux = vw, frac.value, flux.value
    theseWeights._version += 1
    return flux.value


def planck_radiance(lambda_um, temps):
    """The Planck function as emission_weighting evaluates it (mcbrat_planck_radiance), W m-2 sr-1 um-1, in double; the
    shape of `temps` is kept."""
    t = np.ascontiguousarray(temps, np.float64)
    out = np.zeros(t.shape, np.float64)
    if lib().mcbrat_planck_radiance(float(lambda_um), t.size, ptr(t), ptr(out)) != 0:
        raise McbratError("planck_radiance: the wavelength must be positive")
    return out


def planck_sources(thisDomain, surfaceTemp):
    """(cellSource, surfaceSource) for Integrator.renderCameraEmission / renderSensorsEmission: the
    Planck radiance of the domain's temperatures, [nz, ny, nx] float32, and that of surfaceTemp, [ny, nx] float32 (one value for
    every column), at the domain's wavelength, in W m-2 sr-1 um-1."""
    info = thisDomain.getInfo_Domain()
    if info["temps"] is None:
        raise McbratError("planck_sources: domain has no temperatures")
    nx, ny = info["numX"], info["numY"]
    cell = planck_radiance(thisDomain.lambda_um, np.ascontiguousarray(info["temps"].transpose(2, 1, 0)))
    sfc = planck_radiance(thisDomain.lambda_um, np.full((ny, nx), float(surfaceTemp)))
    return cell.astype(np.float32), sfc.astype(np.float32)


def _check_mu(solarMu):
    if abs(solarMu) > 1.0 or abs(solarMu) <= np.finfo(np.float32).tiny:
        raise McbratError("setIllumination: solarMu out of bounds")


def _check_azimuth(solarAzimuth):
    if solarAzimuth < 0.0 or solarAzimuth > 360.0:
        raise McbratError("setIllumination: solarAzimuth out of bounds")


class PhotonStream:
    """kind: "Directional", "RandomAzimuth", "Flux", "Spotlight" (the solar forms) or "BBEmission"."""

    def __init__(self, numberOfPhotons, solarMu=None, solarAzimuth=None, theseWeights=None, solarX=None, solarY=None):
        if numberOfPhotons < 0:
            raise McbratError("setIllumination: must ask for non-negative number of photons.")
        self.numberOfPhotons = int(numberOfPhotons)
        self.currentPhoton = 1
        spot = solarX is not None or solarY is not None
        if theseWeights is not None:  # (BBEmission: any solar geometry given with it is ignored, as it always was)
            if theseWeights.voxelWeights is None:
                raise McbratError("setIllumination: weights have not been computed (call emission_weighting).")
            self.kind, self.weights = "BBEmission", theseWeights
        elif spot:
            if solarMu is None or solarAzimuth is None or solarX is None or solarY is None:
                raise McbratError("new_PhotonStream: a spotlight needs solarMu, solarAzimuth, solarX and solarY")
            _check_azimuth(solarAzimuth)
            _check_mu(solarMu)
            # the reference tests abs(solarX), abs(solarY) (:193-195); a negative fraction is refused here as well
            x, y = np.float32(solarX), np.float32(solarY)
            if not (0.0 < x <= 1.0 and 0.0 < y <= 1.0):
                raise McbratError("setIllumination: x and y positions must be between 0 and 1")
            self.kind, self.solarMu, self.solarAzimuth = "Spotlight", float(solarMu), float(solarAzimuth)
            self.solarX, self.solarY = float(solarX), float(solarY)
        elif solarAzimuth is not None:
            if solarMu is None:
                raise McbratError("new_PhotonStream: solarAzimuth needs solarMu")
            _check_azimuth(solarAzimuth)
            _check_mu(solarMu)
            self.kind, self.solarMu, self.solarAzimuth = "Directional", float(solarMu), float(solarAzimuth)
        elif solarMu is not None:
            _check_mu(solarMu)
            self.kind, self.solarMu = "RandomAzimuth", float(solarMu)
        else:
            self.kind = "Flux"

    def morePhotonsExist(self):
        return 0 < self.currentPhoton <= self.numberOfPhotons


def new_PhotonStream(solarMu=None, solarAzimuth=None, numberOfPhotons=0, theseWeights=None, solarX=None, solarY=None,
                     randomNumbers=None):
    """Resolves like the reference's overload, by the arguments given:
    (solarMu, solarAzimuth) Directional; (solarMu) RandomAzimuth; () Flux; (solarMu, solarAzimuth, solarX=, solarY=)
    Spotlight; (theseWeights=) BBEmission.  randomNumbers is accepted and ignored: photons are generated on the GPU."""
    return PhotonStream(numberOfPhotons, solarMu, solarAzimuth, theseWeights, solarX, solarY)
