"""The cases of the backward oracle (DESIGN.md sections 3, 4.19, 4.20, 4.22, 4.23): what tests/test_oracle_backward.py (host)
and tests/test_gpu_backward_oracle.py (GPU) share.

Every case is ONE render with one sample per bin and N batches, so that bin (batch b, receiver r) of `batchMeans` holds the sum
of ONE path: the one with counter id r (a pixel, or a sensor's id) and sample index firstSample + b.  firstSample is 2^32 - N/2:
the range straddles 2^32 and both halves of the sample counter are exercised.  The oracle (oracle.backward_paths) traces the same
paths from the event-0 draws put through the host mirrors Camera.ray / Sensors.ray.

A path is CLEAN when the oracle does not flag it `near` (a discrete decision within the margins of DESIGN.md section 3) and its
decision record (fate, number of events, hash of every event's leg end, cell, component, patch and roulette outcome) is the
same with floatState on and off.  Clean paths are compared one by one, the others only through the case's mean.

RTOL, the relative tolerance of a clean path, is 4 x the largest relative difference between the floatState and the double run
over all clean paths of all cases -- a statement about float arithmetic made by the oracle alone, on the CPU.  Measured: see
MEASURED_FLOAT_DIFFERENCE below; tests/test_oracle_backward.py asserts that the constant is not above 4 x what it measures."""
import functools

import numpy as np

from tests import cases

SEED = 20261023
TABLE, FWD = 9001, 9001     # points of the inverse and of the forward tables, both sides (the product's smallest sizes)
MEASURED_FLOAT_DIFFERENCE = 2.57e-4  # largest |float - double| / double of a clean path, all cases (tests/test_oracle_backward.py measures it)
RTOL = 1.0e-3                        # 4 x that, rounded down
STEP = 2.0 ** -40           # the fixed-point step of a one-sample bin, in the entry's units (w0, or the largest source value)
MAX_EXCLUDED, MAX_EXCLUDED_PER_RECEIVER, MIN_PER_CLASS = 0.05, 0.10, 200
PATH_EDGES = np.array([0.0, 0.25, 0.4, 0.6, 1.0], np.float32)


def small_domain(emitting=False):
    """tests/test_gpu_camera.small_domain (4 x 3 x 2, unequal layers, two Henyey-Greenstein components, a per-patch surface); for
    the emission renders with ssa < 1 in both components."""
    from tests.test_gpu_camera import small_domain as make
    case = make()
    if emitting:
        comps = [dict(c) for c in case["components"]]
        comps[0]["ssa"], comps[1]["ssa"] = np.full_like(comps[0]["ssa"], 0.9), np.full_like(comps[1]["ssa"], 0.8)
        case["components"] = comps
    return case


def emitting_domain():
    return small_domain(True)


def step_cloud():
    """cases.step_cloud(ssa=0.99) over albedo 0.2 on an 8 x 1 x 8 grid: the same medium (optical depth 2 | 18, the same extent) in
    cells four times as wide and as high.  On the 32 x 1 x 32 grid 8.5 % of the paths came within the margin of a face (42 events
    a path, cells of 0.0078 km, measured with the oracle): above the 5 % a case may exclude, so the case has the coarser grid."""
    case = cases.step_cloud(ssa=0.99)
    ext = case["components"][0]["ext"][::4, :, ::4].copy()
    case.update(xe=case["xe"][::4].copy(), ye=case["ye"].copy(), ze=case["ze"][::4].copy(), albedo=0.2)
    case["components"] = [dict(case["components"][0], ext=ext, ssa=np.full_like(ext, 0.99), pfIndex=np.ones(ext.shape, np.int32))]
    return case


def one_cell():
    """1 x 1 x 1: every sun ray at mu0 = 0.05 and most legs wrap many periods.  Two components, optical depth 1.125.  The first has
    ssa = 0.705: its second collision leaves w = 0.497, between 0.49 and the roulette's threshold.  The second is a TABULATED phase
    function with a ripple (Henyey-Greenstein, g = 0.3, on 181 angles, every other value halved, as the ripple of a Mie table):
    between two of its angles P changes by a factor of two, so the forward table's 9001 angles are not finer than P needs
    and the interpolation between them shows in a path's value."""
    e1, e2 = np.full((1, 1, 1), 3.0), np.full((1, 1, 1), 1.5)
    ang = np.linspace(0.0, np.pi, 181).astype(np.float32)
    ang[-1] = np.float32(np.pi)
    hg = (1 - 0.09) / (1 + 0.09 - 0.6 * np.cos(ang.astype(np.float64))) ** 1.5
    ripple = (hg * np.where(np.arange(181) % 2, 0.5, 1.0)).astype(np.float32)
    return dict(name="oneCell", xe=np.array([0.0, 0.3]), ye=np.array([0.0, 0.4]), ze=np.array([0.0, 0.25]), albedo=0.6,
                components=[dict(ext=e1, ssa=np.full_like(e1, 0.705), pfIndex=np.ones(e1.shape, np.int32), legendre=[cases.hg_legendre(0.7, 64)]),
                            dict(ext=e2, ssa=np.full_like(e2, 1.0), pfIndex=np.ones(e2.shape, np.int32), tabulated=[(ang, ripple)])])


def emission_sources(case):
    """distinct values for every cell and every column (the caller's units)"""
    nx, ny, nz = len(case["xe"]) - 1, len(case["ye"]) - 1, len(case["ze"]) - 1
    cell = (1.0 + 0.37 * np.arange(nx * ny * nz)).astype(np.float32).reshape(nz, ny, nx)
    return cell, (11.0 + 0.53 * np.arange(nx * ny)).astype(np.float32).reshape(ny, nx)


def _pinhole_a(gridInLds=-1):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=4, npy=3, position=(0.21, 0.13, 0.09), look=(0.8, 0.5, 0.1), up=(0.0, 0.0, 1.0), fov=100.0, gridInLds=gridInLds)


def _ortho_a(gridInLds=-1):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("orthographic", npx=2, npy=2, mu=0.6, phi=110.0, footprint=(-0.3, 0.9, -0.2, 0.55), height=0.2, gridInLds=gridInLds)


def _ortho_b(gridInLds=-1):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("orthographic", npx=8, npy=1, mu=1.0, phi=0.0, footprint=(0.0, 0.5, 0.0, 0.5), height=0.25, gridInLds=gridInLds)


def _pinhole_c(gridInLds=-1):
    from mcbrat3d_amd.camera import new_Camera
    return new_Camera("pinhole", npx=2, npy=2, position=(0.11, 0.17, 0.0), look=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=90.0, gridInLds=gridInLds)


def _sensors_a(gridInLds=-1):
    """a tilted planar sensor, a horizontal one at z0, a spherical point; ids that are not their positions in the call"""
    from mcbrat3d_amd.sensors import new_Sensors
    return new_Sensors([(0.27, 0.14, 0.11), (0.4, 0.07, 0.0), (0.06, 0.22, 0.15)], tilt=[35.0, 0.0, 0.0], azimuth=[200.0, 0.0, 0.0],
                       kind=["planar", "planar", "spherical"], ids=[7, 3, 11])


# name -> (group, domain, sun (mu0, phi0) or None, roulette, entry, receiver, paths per receiver)
CASES = {
    "A pinhole": ("A", small_domain, (0.5, 30.0), True, "renderCamera", _pinhole_a, 1024),
    "A orthographic": ("A", small_domain, (0.5, 30.0), True, "renderCamera", _ortho_a, 2048),
    "B": ("B", step_cloud, (0.3, 37.0), False, "renderCamera", _ortho_b, 256),
    "C": ("C", one_cell, (0.05, 200.0), True, "renderCamera", _pinhole_c, 2048),
    "A sensors": ("A", small_domain, (0.5, 30.0), True, "renderSensors", _sensors_a, 2048),
    "A emission camera": ("A emission", emitting_domain, None, True, "renderCameraEmission", _pinhole_a, 1024),
    "A emission sensors": ("A emission", emitting_domain, None, True, "renderSensorsEmission", _sensors_a, 2048),
    "A path lengths": ("A", small_domain, (0.5, 30.0), True, "renderCameraPathLengths", _pinhole_a, 1024),
}
# the classes a group's clean paths must hold MIN_PER_CLASS of (the issue's list); B has one component, no roulette and a camera
# that looks down from the top (no path leaves at once); the roulette class is asked of A only; an emission path has no value 0
CLASSES = {
    "A": ("threeCollisions", "reflectionThenCollision", "rouletteSurvivals", "secondComponent", "wrappedLegs", "zero"),
    "B": ("threeCollisions", "reflectionThenCollision", "wrappedLegs"),
    "C": ("threeCollisions", "reflectionThenCollision", "secondComponent", "wrappedLegs", "zero"),
    "A emission": ("threeCollisions", "reflectionThenCollision", "rouletteSurvivals", "secondComponent", "wrappedLegs"),
}
MODE = {"renderCamera": "solar", "renderSensors": "solar", "renderCameraEmission": "emission", "renderSensorsEmission": "emission",
        "renderCameraPathLengths": "pathlengths"}


def first_sample(n):
    return 2 ** 32 - n // 2


def u01(words):
    """the kernel's map of a Philox word to [0, 1]: float(u) * 2^-32, in float"""
    return (np.asarray(words, np.uint32).astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float64)


def sun_vector(mu0, phi0):
    """the unit vector toward the sun: minus the float direction of travel of the Directional source"""
    from oracle import oracle as O
    return -O.intensity_directions([-abs(mu0)], [phi0])[0].astype(np.float64)


def direct_factor(sensors, i, sun):
    """c / w0 of sensor i as mcbrat_render_sensors forms it: max(0, n . s) / mu0 / pi (planar), 1 / mu0 / (4 pi) (spherical)"""
    s = sun_vector(*sun)
    s = s / np.sqrt(s @ s)
    mu0 = abs(s[2])
    if sensors.kinds[i] == 1:
        return float(np.float32(1.0 / mu0 / (4.0 * np.pi)))
    n = sensors.normals[i] / np.sqrt(sensors.normals[i] @ sensors.normals[i])
    return float(np.float32(max(0.0, float(n @ s)) / mu0 / np.pi))


@functools.lru_cache(maxsize=None)
def paths(name):
    """The paths of a case, receiver-major: dict(receiver [m], batch [m], ids [m], samples [m], origins [m, 3], directions [m, 3],
    n (paths per receiver), receivers, w0 [receivers])."""
    from oracle import oracle as O
    _, _, _, _, entry, make, n = CASES[name]
    rcv = make()
    sensors = "Sensors" in entry
    nr = len(rcv) if sensors else rcv.npx * rcv.npy
    ids = np.array([int(rcv.ids[r]) for r in range(nr)] if sensors else np.arange(nr), np.uint32)
    first = first_sample(n)
    receiver, batch = np.repeat(np.arange(nr), n), np.tile(np.arange(n), nr)
    samples = (first + batch).astype(np.uint64)
    key = (SEED & 0xffffffff, SEED >> 32)
    o, d = np.zeros((nr * n, 3)), np.zeros((nr * n, 3))
    for k in range(nr * n):
        s, r = int(samples[k]), int(receiver[k])
        u = u01(O.philox4x32_10((0, int(ids[r]), s & 0xffffffff, s >> 32), key))
        if sensors:
            o[k], d[k] = rcv.ray(r, u[0], u[1], u[2], u[3])
        else:
            o[k], d[k] = rcv.ray(r % rcv.npx, r // rcv.npx, u[0], u[1]) if rcv.jitter else rcv.ray(r % rcv.npx, r // rcv.npx)
    w0 = np.array([(4.0 * np.pi if rcv.kinds[r] else np.pi) for r in range(nr)] if sensors else np.ones(nr))
    return dict(receiver=receiver, batch=batch, ids=ids[receiver], samples=samples, origins=o, directions=d, n=n, receivers=nr, w0=w0, rcv=rcv)


@functools.lru_cache(maxsize=None)
def oracle_setup(name):
    _, domain, sun, rr, _, _, _ = CASES[name]
    case = domain()
    P = cases.oracle_problem(case, nsteps=TABLE, use_russian_roulette=rr)
    inten = cases.oracle_intensity(case, [1.0], [0.0], n_angles=FWD) if sun is not None else None
    return case, P, inten


def oracle_run(name, float_state=False, mutation=None, **kw):
    """oracle.backward_paths of the case's paths (a sensor case: one call per sensor, for its direct factor); arrays receiver-major
    like paths(name)"""
    from oracle import oracle as O
    _, _, sun, _, entry, _, _ = CASES[name]
    case, P, inten = oracle_setup(name)
    p = paths(name)
    more = dict(kw)
    if MODE[entry] == "emission":
        more["cell_source"], more["surface_source"] = emission_sources(case)
    if MODE[entry] == "pathlengths":
        more["path_edges"] = PATH_EDGES
    parts = []
    for r in (range(p["receivers"]) if entry == "renderSensors" else [None]):
        sel = slice(None) if r is None else slice(r * p["n"], (r + 1) * p["n"])
        direct = direct_factor(p["rcv"], r, sun) if r is not None else 0.0
        parts.append(O.backward_paths(P, inten, SEED, p["origins"][sel], p["directions"][sel], p["ids"][sel], p["samples"][sel], mode=MODE[entry],
                                      sun=sun, float_state=float_state, mutation=mutation, direct=direct, **more))
    if len(parts) == 1:
        return parts[0]
    out = {k: np.concatenate([q[k] for q in parts]) for k in ("sum", "direct", "nEvents", "fate", "near", "hash", "binSum", "record")}
    out["classes"] = {c: np.concatenate([q["classes"][c] for q in parts]) for c in parts[0]["classes"]}
    return out


def values(name, run):
    """what a path is compared by, [m, parts]: the sum; diffuse and direct of a solar sensor; the bins of a path-length render"""
    entry = CASES[name][4]
    if entry == "renderSensors":
        return np.stack([run["sum"], run["direct"]], axis=1)
    if entry == "renderCameraPathLengths":
        return run["binSum"]
    return run["sum"][:, None]


@functools.lru_cache(maxsize=None)
def design(name):
    """The double and the floatState run of a case and what follows from the two: clean [m], the excluded share in all and per
    receiver, the largest relative difference of a clean path's values, the class counts of the clean paths."""
    p = paths(name)
    ref, flt = oracle_run(name), oracle_run(name, float_state=True)
    same = (ref["fate"] == flt["fate"]) & (ref["nEvents"] == flt["nEvents"]) & (ref["hash"] == flt["hash"])
    clean = same & ~ref["near"] & ~flt["near"]
    a, b = values(name, ref), values(name, flt)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(a != 0.0, np.abs(b - a) / np.abs(a), np.where(b != 0.0, np.inf, 0.0))
    rel = rel[clean]
    per_receiver = np.array([1.0 - clean[p["receiver"] == r].mean() for r in range(p["receivers"])])
    c = ref["classes"]
    classes = dict(threeCollisions=c["collisions"] >= 3, reflectionThenCollision=c["reflectionThenCollision"] > 0,
                   rouletteSurvivals=c["rouletteSurvivals"] > 0, secondComponent=c["secondComponent"] > 0, wrappedLegs=c["wrappedLegs"] > 0,
                   zero=(ref["fate"] == 0) & (ref["nEvents"] == 1))
    return dict(ref=ref, flt=flt, clean=clean, excluded=1.0 - clean.mean(), excludedPerReceiver=per_receiver,
                floatDifference=float(rel.max()) if rel.size else 0.0, classes={k: int((v & clean).sum()) for k, v in classes.items()})
