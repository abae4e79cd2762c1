"""Host-side mirror of src/surfaceProperties.f95: a surface whose reflectance varies with horizontal position.  The
reference's template for "a few parameters per patch" surface models has one parameter (Lambertian); the RPV and Ross-Li
BRDFs fill it with four and three, the Cox-Munk ocean surface with four (section 4.11.1)."""
import ctypes as C

import numpy as np

from ._capi import McbratError

numberOfParameters = 1  # :28 (Lambertian)
MODELS = {"Lambertian": (0, 1), "RPV": (1, 4), "RossLi": (2, 3), "CoxMunk": (3, 4)}  # model: (kind of mcbrat_set_surface_brdf, numberOfParameters)
ENERGY_GRID = np.arange(1, 11) / 10.0  # incidence cosines of the energy rule (kBrdfAlbedoGrid in mcbrat_brdf.h)


class SurfaceDescription:
    def __init__(self, xPosition, yPosition, BRDFParameters, model="Lambertian"):
        self.xPosition = xPosition
        self.yPosition = yPosition
        self.BRDFParameters = BRDFParameters  # [numberOfParameters, numX - 1, numY - 1]
        self.model = model

    @property
    def kind(self):
        return MODELS[self.model][0]

    def isReady_surfaceDescription(self):  # :165-172
        return self.xPosition is not None and self.yPosition is not None and self.BRDFParameters is not None


def new_SurfaceDescription(surfaceParameters, xPosition=None, yPosition=None, model="Lambertian"):
    """newSurfaceDescriptionXY (:58-94) when positions are given, newSurfaceUniform (:96-115) otherwise.  model: "Lambertian"
    (one parameter, the reflectance), "RPV" (rho0, k, Theta, rhoC), "RossLi" (fIso, fVol, fGeo) or "CoxMunk" (U wind speed in
    m/s, n refractive index, rhoWc whitecap reflectance, aW water-leaving albedo); surfaceParameters is
    [numberOfParameters, numX - 1, numY - 1], or numberOfParameters values for a uniform surface."""
    if model not in MODELS:
        raise McbratError("new_SurfaceDescription: unknown surface BRDF model '%s' (Lambertian, RPV, RossLi or CoxMunk)." % (model,))
    nParams = MODELS[model][1]
    params = np.asarray(surfaceParameters, np.float32)
    if xPosition is None and yPosition is None:
        if params.reshape(-1).size != nParams:
            raise McbratError("new_SurfaceDescription: Wrong number of parameters supplied for surface BRDF.")
        huge = float(np.finfo(np.float32).max)
        xPosition, yPosition = (0.0, huge), (0.0, huge)
        params = params.reshape(nParams, 1, 1)
    x = np.ascontiguousarray(xPosition, np.float64)
    y = np.ascontiguousarray(yPosition, np.float64)
    if params.ndim != 3 or params.shape[0] != nParams:
        raise McbratError("new_SurfaceDescription: Wrong number of parameters supplied for surface BRDF.")
    if params.shape[1] != x.size - 1 or params.shape[2] != y.size - 1:
        raise McbratError("new_SurfaceDescription: position vector(s) are incorrect length.")
    if np.any(np.diff(x) <= 0.0) or np.any(np.diff(y) <= 0.0):
        raise McbratError("new_SurfaceDescription: positions must be unique, increasing.")
    if model == "Lambertian":
        if np.any(params[0] < 0.0) or np.any(params[0] > 1.0):
            raise McbratError("new_SurfaceDescription: surface reflectance must be between 0 and 1")
    else:
        _check_brdf(model, params)
    return SurfaceDescription(x, y, params.copy(), model)


def _check_brdf(model, params):
    """The parameter domains and the energy rule of mcbrat_set_surface_brdf, with its texts (once per distinct parameter vector)."""
    kind, n = MODELS[model]
    for q in np.unique(params.reshape(n, -1).T, axis=0):
        if model == "RPV":
            rho0, k, th, rhoC = q
            if not (0.0 <= rho0 <= 1.0 and 0.2 <= k <= 2.0 and abs(th) <= 0.95 and 0.0 <= rhoC <= 1.0):
                raise McbratError("new_SurfaceDescription: RPV parameters must satisfy 0 <= rho0 <= 1, 0.2 <= k <= 2, "
                                  "|Theta| <= 0.95, 0 <= rhoC <= 1")
        elif model == "CoxMunk":
            U, n_, rhoWc, aW = q
            if not (0.0 <= U <= 50.0 and 1.0 <= n_ <= 2.0 and 0.0 <= rhoWc <= 1.0 and 0.0 <= aW <= 1.0):
                raise McbratError("new_SurfaceDescription: Cox-Munk parameters must satisfy 0 <= U <= 50, 1 <= n <= 2, "
                                  "0 <= rhoWc <= 1, 0 <= aW <= 1")
        elif not np.all(q >= 0.0):
            raise McbratError("new_SurfaceDescription: Ross-Li kernel weights must not be negative")
        if any(not (brdf_albedo(kind, q, mu) <= 1.0 + 1e-3) for mu in ENERGY_GRID):
            raise McbratError("new_SurfaceDescription: surface reflects more energy than it receives "
                              "(directional-hemispherical albedo above 1)")


def _lib():
    from ._capi import lib
    return lib()


def brdf_reflectance(kind, params, d_in, d_out):
    """The reflectance factor R = pi f of the library's evaluator (mcbrat_brdf_reflectance) for one parameter vector and the
    propagation directions d_in (arriving, z < 0) and d_out (leaving, z > 0)."""
    q = np.ascontiguousarray(params, np.float32)
    a = np.ascontiguousarray(d_in, np.float64)
    b = np.ascontiguousarray(d_out, np.float64)
    return float(_lib().mcbrat_brdf_reflectance(int(kind), q.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                                b.ctypes.data_as(C.c_void_p)))


def brdf_albedo(kind, params, mu_i):
    """Directional-hemispherical albedo rho_dh(mu_i) of one parameter vector (mcbrat_brdf_albedo)."""
    q = np.ascontiguousarray(params, np.float32)
    return float(_lib().mcbrat_brdf_albedo(int(kind), q.ctypes.data_as(C.c_void_p), float(mu_i)))


def brdf_sample(kind, params, d_in, u):
    """The reflection's sampler as the tracing kernel applies it (mcbrat_brdf_sample; no GPU): for one parameter vector, the
    arriving direction d_in and uniforms u[n, 3] = (component, u1, u2) -> (d_out[n, 3], weight[n]), the leaving directions and
    the factors of the photon's weight (0: the photon ends).  The Lambertian draw is mu = sqrt(u1), azimuth 2 pi u2; Cox-Munk
    mixes it with a draw from the glint lobe.  The mean weight estimates brdf_albedo(kind, params, -d_in[2])."""
    q = np.ascontiguousarray(params, np.float32)
    a = np.ascontiguousarray(d_in, np.float64)
    uu = np.ascontiguousarray(u, np.float64)
    if uu.ndim != 2 or uu.shape[1] != 3 or a.shape != (3,):
        raise McbratError("brdf_sample: d_in must be a 3-vector and u an [n, 3] array")
    d_out = np.empty(uu.shape, np.float64)
    w = np.empty(uu.shape[0], np.float32)
    if _lib().mcbrat_brdf_sample(int(kind), q.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), uu.shape[0],
                                 uu.ctypes.data_as(C.c_void_p), d_out.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)) != 0:
        raise McbratError("brdf_sample: unknown surface BRDF model")
    return d_out, w


def _patch(edges, v):
    """The patch under v on a description's positions, periodic, as the kernels find it (mcbrat_kernels.hip surface_patch)."""
    lo, hi = float(edges[0]), float(edges[-1])
    r = float(np.float32(v))
    if not (lo < r <= hi):
        r = lo + (r - lo) % (hi - lo)
        if r == lo:
            r = hi
    return int(min(max(np.searchsorted(edges, r, side="right"), 1), edges.size - 1)) - 1


def computeSurfaceReflectance(surfaceDescription, xPos, yPos, incomingMu, outgoingMu, incomingPhi, outgoingPhi):
    """computeSurfaceReflectance (:119-147): the reflectance factor R = pi f of the patch under (xPos, yPos).

    The angles give the photon's propagation directions: it arrives along d_in = (s_i cos(incomingPhi), s_i sin(incomingPhi),
    -|incomingMu|) and leaves along d_out = (s_r cos(outgoingPhi), s_r sin(outgoingPhi), |outgoingMu|), s = sqrt(1 - mu^2),
    azimuths in degrees.  So outgoingPhi = incomingPhi + 180 with |outgoingMu| = |incomingMu| is exact backscatter (the hot
    spot).  A Lambertian patch returns its reflectance whatever the angles."""
    d = surfaceDescription
    ix, iy = _patch(d.xPosition, xPos), _patch(d.yPosition, yPos)
    q = d.BRDFParameters[:, ix, iy]
    mi, mr = abs(float(incomingMu)), abs(float(outgoingMu))
    pi_, pr = np.radians(float(incomingPhi)), np.radians(float(outgoingPhi))
    si, sr = np.sqrt(max(0.0, 1.0 - mi * mi)), np.sqrt(max(0.0, 1.0 - mr * mr))
    return brdf_reflectance(d.kind, q, (si * np.cos(pi_), si * np.sin(pi_), -mi), (sr * np.cos(pr), sr * np.sin(pr), mr))
