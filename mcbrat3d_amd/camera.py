"""The backward Monte Carlo camera: a sensor anywhere in the domain, per pixel.

    cam = new_Camera("pinhole", npx=64, npy=48, position=(1.0, 2.0, 0.0), look=(0, 0, 1), up=(0, 1, 0), fov=90.0)
    cam = new_Camera("orthographic", npx=32, npy=1, mu=1.0, phi=0.0, footprint=(0.0, 16.0, 0.0, 0.5), height=2.4)
    out = integrator.renderCamera(cam, new_RandomNumberSequence(seed), samplesPerPixel=10000, numBatches=4)

new_Camera makes the checks that need no GPU (the library repeats them, and adds those that need the domain: the height against
[z0, zMax], the tally budget).  Conventions (include/mcbrat.h, csrc/mcbrat_camera_ray.h): the orthographic camera sees the light
that travels along (mu, phi), the convention of intensityMus / intensityPhis -- mu > 0 looks down; pixel (i, j) is cell (i, j)
of the footprint.  The pinhole's row j grows upward along `up`; arrays are [npy, npx]."""
import ctypes as C
import math

import numpy as np

from ._capi import Camera as _CameraStruct, McbratError

KINDS = {"orthographic": 0, "pinhole": 1}


class Camera:
    def __init__(self, kind, npx, npy, jitter, gridInLds, mu, phi, footprint, height, position, look, up, fov):
        self.kind, self.npx, self.npy, self.jitter, self.gridInLds = kind, npx, npy, jitter, gridInLds
        self.mu, self.phi, self.footprint, self.height = mu, phi, footprint, height
        self.position, self.look, self.up, self.fov = position, look, up, fov

    def struct(self):
        """The mcbrat_camera the library takes."""
        s = _CameraStruct()
        s.kind, s.npx, s.npy, s.jitter, s.gridInLds = KINDS[self.kind], self.npx, self.npy, int(self.jitter), int(self.gridInLds)
        s.mu, s.phiDeg = self.mu, self.phi
        s.xLo, s.xHi, s.yLo, s.yHi = self.footprint
        s.z = self.height
        s.position[:] = self.position
        s.look[:] = self.look
        s.up[:] = self.up
        s.fovXDeg = self.fov
        return s

    def ray(self, i, j, u=0.5, v=0.5):
        """Origin and backward direction of the position (i + u, j + v) of the image: the mapping the kernel uses
        (mcbrat_camera_ray; the origin is not folded into the domain)."""
        from ._capi import lib, ptr
        o, d = np.zeros(3), np.zeros(3)
        s = self.struct()
        if lib().mcbrat_camera_ray(C.addressof(s), int(i), int(j), float(u), float(v), ptr(o), ptr(d)) != 0:
            raise McbratError("camera ray: the library refuses this camera")
        return o, d

    def attributes(self):
        """The camera's parameters as the attributes written with its image (ncio)."""
        a = {"cameraKind": self.kind, "cameraPixels": [self.npx, self.npy], "cameraJitter": int(self.jitter)}
        if self.kind == "orthographic":
            a.update(cameraMu=self.mu, cameraPhi=self.phi, cameraFootprint=list(self.footprint), cameraHeight=self.height)
        else:
            a.update(cameraPosition=list(self.position), cameraLook=list(self.look), cameraUp=list(self.up), cameraFov=self.fov)
        return a


def _vec3(name, v):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size != 3 or not np.all(np.isfinite(a)):
        raise McbratError("new_Camera: %s must be three finite numbers." % name)
    return tuple(float(x) for x in a)


def new_Camera(kind="orthographic", npx=1, npy=1, jitter=True, gridInLds=-1, mu=1.0, phi=0.0, footprint=None, height=None,
               position=None, look=None, up=(0.0, 0.0, 1.0), fov=60.0):
    """A camera for Integrator.renderCamera.  orthographic: mu, phi (degrees), footprint = (xLo, xHi, yLo, yHi), height.
    pinhole: position, look, up (need not be normalised, not parallel), fov = full horizontal field of view in degrees."""
    if kind not in KINDS:
        raise McbratError("new_Camera: unknown camera kind '%s' (orthographic or pinhole)." % (kind,))
    if int(npx) != npx or int(npy) != npy or npx < 1 or npy < 1 or npx * npy > 2 ** 31 - 1:
        raise McbratError("new_Camera: the image needs at least one pixel in x and in y (and fewer than 2^31 in all).")
    if gridInLds not in (-1, 0, 1):
        raise McbratError("new_Camera: gridInLds must be -1, 0 or 1.")
    if kind == "orthographic":
        mu, phi = float(mu), float(phi)
        if not (abs(mu) <= 1.0) or mu == 0.0:
            raise McbratError("new_Camera: mu must be in [-1, 1] and can't be 0 (directly sideways).")
        if not (0.0 <= phi <= 360.0):
            raise McbratError("new_Camera: phi must be between 0 and 360.")
        if footprint is None or height is None:
            raise McbratError("new_Camera: an orthographic camera needs footprint = (xLo, xHi, yLo, yHi) and height.")
        f = np.asarray(footprint, np.float64).reshape(-1)
        if f.size != 4 or not np.all(np.isfinite(f)) or not (f[1] > f[0] and f[3] > f[2]):
            raise McbratError("new_Camera: degenerate footprint (xHi > xLo and yHi > yLo are needed).")
        if not math.isfinite(float(height)):
            raise McbratError("new_Camera: the camera's height is not finite.")
        return Camera(kind, int(npx), int(npy), bool(jitter), int(gridInLds), mu, phi, tuple(float(x) for x in f), float(height),
                      (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0)
    if position is None or look is None:
        raise McbratError("new_Camera: a pinhole camera needs position and look.")
    position, look, up = _vec3("position", position), _vec3("look", look), _vec3("up", up)
    l2, u2 = sum(x * x for x in look), sum(x * x for x in up)
    if not (l2 > 0.0 and u2 > 0.0):
        raise McbratError("new_Camera: look and up must be non-zero vectors.")
    cross = np.cross(look, up)
    if not (float(cross @ cross) > 1e-24 * l2 * u2):
        raise McbratError("new_Camera: look and up are parallel.")
    fov = float(fov)
    if not (0.0 < fov < 180.0):
        raise McbratError("new_Camera: the field of view must be in (0, 180) degrees.")
    return Camera(kind, int(npx), int(npy), bool(jitter), int(gridInLds), 1.0, 0.0, (0.0, 1.0, 0.0, 1.0), 0.0, position, look, up, fov)


# -- the radiance by photon path length (Integrator.renderCameraPathLengths) ---------------------------
def _by_length(radianceByLength, pathEdges):
    rad = np.asarray(radianceByLength, np.float64)
    e = np.asarray(pathEdges, np.float64).reshape(-1)
    if rad.ndim < 1 or rad.shape[0] != e.size or e.size < 1:
        raise McbratError("path lengths: radianceByLength must be [bin, ...] with one bin per edge of pathEdges.")
    return rad, e.reshape((-1,) + (1,) * (rad.ndim - 1))


def absorbed_radiance(radianceByLength, pathEdges, k):
    """(lower, upper) bounds of the radiance under a uniform absorber of extinction k (per unit length of pathEdges), from a
    render WITHOUT it -- the equivalence theorem, I(k) = sum_b I_b exp(-k L_b), with every length of bin b put at its upper edge
    (lower: the open last bin gives 0) and at its lower edge (upper).  radianceByLength is [bin, ...]; the bounds have its
    remaining shape.  k = 0: both are the sum of the bins."""
    rad, e = _by_length(radianceByLength, pathEdges)
    k = float(k)
    if not (k >= 0.0) or not math.isfinite(k):
        raise McbratError("absorbed_radiance: k must be finite and not negative.")
    upper = (rad * np.exp(-k * e)).sum(axis=0)
    if k == 0.0:
        return upper.copy(), upper
    lower = (rad[:-1] * np.exp(-k * e[1:])).sum(axis=0)
    return lower, upper


def mean_path_length(radianceByLength, pathEdges):
    """(lower, upper) bounds of the radiance-weighted mean path length <L> = sum_b I_b L_b / sum_b I_b over the CLOSED bins (all but
    the open last one, whose lengths have no upper bound): every length at its bin's lower edge, and at its upper edge.  NaN
    where the closed bins hold nothing."""
    rad, e = _by_length(radianceByLength, pathEdges)
    closed = rad[:-1]
    total = closed.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lower = (closed * e[:-1]).sum(axis=0) / total
        upper = (closed * e[1:]).sum(axis=0) / total
    return lower, upper
