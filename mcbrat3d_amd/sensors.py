"""Backward sensors: irradiance on a plane and actinic flux at a point, anywhere in the domain.

    s = new_Sensors([(1.0, 2.0, 0.0)])                                   # a pyranometer on the ground, facing up
    s = new_Sensors([(1.0, 2.0, 0.0)], tilt=35.0, azimuth=180.0)         # a panel tilted 35 degrees toward -x
    s = new_Sensors(centres, kind="spherical")                           # actinic flux along a flight track
    s = new_Sensors([(0.0, 0.0, 0.0)], extents=[((0.5, 0, 0), (0, 0.5, 0))])   # the mean over a column's face
    out = integrator.renderSensors(s, new_RandomNumberSequence(seed), samplesPerSensor=10000, numBatches=4)

new_Sensors makes the checks that need no GPU (the library repeats them, and adds those that need the domain: the receivers'
corners against [z0, zMax], the tally budget).  Conventions (include/mcbrat.h, csrc/mcbrat_sensor_ray.h): a planar sensor
receives on the side its normal points to, with a cosine response; tilt beta and azimuth alpha in degrees give the normal
(sin(beta) cos(alpha), sin(beta) sin(alpha), cos(beta)) -- tilt 0 faces up, tilt 180 down; a spherical sensor has a uniform
response and ignores the normal.  Values are per unit solar flux through a horizontal plane at the top."""
import ctypes as C
import math

import numpy as np

from ._capi import Sensor as _SensorStruct, McbratError

KINDS = {"planar": 0, "spherical": 1}


class Sensors:
    def __init__(self, kinds, ids, positions, normals, e1, e2):
        self.kinds, self.ids, self.positions, self.normals, self.e1, self.e2 = kinds, ids, positions, normals, e1, e2
        self._structs = None  # (built once: the members are not meant to be changed after new_Sensors)

    def __len__(self):
        return self.positions.shape[0]

    def structs(self):
        """The array of mcbrat_sensor the library takes."""
        if self._structs is not None:
            return self._structs
        arr = self._structs = (_SensorStruct * len(self))()
        for i, s in enumerate(arr):
            s.kind, s.id = int(self.kinds[i]), int(self.ids[i])
            s.position[:] = self.positions[i]
            s.e1[:] = self.e1[i]
            s.e2[:] = self.e2[i]
            s.normal[:] = self.normals[i]
        return arr

    def ray(self, i, u=0.5, v=0.5, a=0.5, c=0.5):
        """Origin and backward direction of sensor i for the draws [u, v, a, c]: the mapping the kernel uses
        (mcbrat_sensor_ray; the origin is not folded into the domain)."""
        from ._capi import lib, ptr
        o, d = np.zeros(3), np.zeros(3)
        arr = self.structs()
        if lib().mcbrat_sensor_ray(C.addressof(arr[int(i)]), float(u), float(v), float(a), float(c), ptr(o), ptr(d)) != 0:
            raise McbratError("sensor ray: the library refuses this sensor")
        return o, d

    def kindNames(self):
        return ["spherical" if k else "planar" for k in self.kinds]


def _rows(name, v, n):
    a = np.asarray(v, np.float64)
    if a.ndim == 1 and a.size == 3:
        a = np.tile(a, (n, 1))
    if a.shape != (n, 3) or not np.all(np.isfinite(a)):
        raise McbratError("new_Sensors: %s must be three finite numbers, or one such row per sensor." % name)
    return np.ascontiguousarray(a)


def _per_sensor(name, v, n):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, n)
    if a.size != n or not np.all(np.isfinite(a)):
        raise McbratError("new_Sensors: %s must be one finite number, or one per sensor." % name)
    return a


def new_Sensors(positions, normals=None, tilt=None, azimuth=None, kind="planar", extents=None, ids=None):
    """Sensors for Integrator.renderSensors.  positions: [n, 3].  kind: "planar" or "spherical", one for all or one per sensor.
    The normal of a planar sensor: `normals` ([n, 3] or one vector), or `tilt` / `azimuth` in degrees (scalars or per sensor;
    default: tilt 0, facing up).  extents: None for point sensors, or per sensor a pair of edge vectors (e1, e2), [n, 2, 3] or
    one pair for all -- the receiver is position + u e1 + v e2, both perpendicular to the normal.  ids: the word each sensor's
    random numbers are keyed by (default 0, 1, ...): a sensor keeps its result when it keeps its id."""
    pos = np.asarray(positions, np.float64)
    if pos.ndim == 1 and pos.size == 3:
        pos = pos.reshape(1, 3)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] < 1 or not np.all(np.isfinite(pos)):
        raise McbratError("new_Sensors: positions must be at least one row of three finite numbers.")
    n = pos.shape[0]
    names = [kind] * n if isinstance(kind, str) else list(kind)
    if len(names) != n or any(k not in KINDS for k in names):
        raise McbratError("new_Sensors: unknown sensor kind (planar or spherical; one for all, or one per sensor).")
    kinds = np.array([KINDS[k] for k in names], np.int32)
    if normals is not None and (tilt is not None or azimuth is not None):
        raise McbratError("new_Sensors: give normals, or tilt and azimuth, not both.")
    if normals is not None:
        nrm = _rows("normals", normals, n)
    else:
        beta = np.radians(_per_sensor("tilt", 0.0 if tilt is None else tilt, n))
        alpha = np.radians(_per_sensor("azimuth", 0.0 if azimuth is None else azimuth, n))
        if np.any(beta < 0.0) or np.any(beta > math.pi):
            raise McbratError("new_Sensors: tilt must be between 0 and 180 degrees.")
        nrm = np.stack([np.sin(beta) * np.cos(alpha), np.sin(beta) * np.sin(alpha), np.cos(beta)], axis=1)
    if extents is None:
        e1, e2 = np.zeros((n, 3)), np.zeros((n, 3))
    else:
        ext = np.asarray(extents, np.float64)
        if ext.shape == (2, 3):
            ext = np.tile(ext, (n, 1, 1))
        if ext.shape != (n, 2, 3) or not np.all(np.isfinite(ext)):
            raise McbratError("new_Sensors: extents must be a pair of edge vectors (e1, e2), or one pair per sensor.")
        e1, e2 = np.ascontiguousarray(ext[:, 0]), np.ascontiguousarray(ext[:, 1])
    for i in range(n):
        if kinds[i] != 0:
            continue
        nn = math.sqrt(float(nrm[i] @ nrm[i]))
        if not nn > 0.0:
            raise McbratError("new_Sensors: a planar sensor needs a non-zero normal.")
        for e in (e1[i], e2[i]):
            if abs(float(e @ nrm[i])) / nn > 1e-6 * math.sqrt(float(e @ e)):
                raise McbratError("new_Sensors: an edge of a planar sensor is not perpendicular to its normal.")
    if ids is None:
        idv = np.arange(n, dtype=np.uint32)
    else:
        raw = np.asarray(ids).reshape(-1)
        if raw.size != n or np.any(raw != np.floor(raw)) or np.any(raw < 0) or np.any(raw > 2 ** 32 - 1):
            raise McbratError("new_Sensors: ids must be one integer in [0, 2^32) per sensor.")
        idv = raw.astype(np.uint32)
    return Sensors(kinds, idv, np.ascontiguousarray(pos), nrm, e1, e2)
