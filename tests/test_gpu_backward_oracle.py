"""camera_kernel held to the backward oracle path by path (DESIGN.md sections 3, 4.19, 4.20, 4.22, 4.23).

Every case of tests/backward_cases.py is rendered with ONE sample per bin and N batches, so that `batchMeans` holds every path's
own sum, once with gridInLds 0 and once with 1 (the same bytes, dropped == 0).  Every clean path is compared with the oracle's
double run within RTOL * ref + the fixed-point step + 2^-24 * ref (RTOL: backward_cases.py, from the oracle's two float states
alone); a path the oracle sends out of the top with nothing reads exactly 0, and so does a path-length bin the oracle deposited
nothing in.  The paths that are not clean are held through the mean over ALL paths of the case, 1e-3 relative.  On case A the
same sample range at 197 samples per pixel in 3 batches must give the means of the kernel's own per-path values.

Measured on the MI355X: the docstring of test_every_clean_path_agrees_with_the_oracle."""
import numpy as np
import pytest

from tests import backward_cases as BC
from tests import cases

pytestmark = pytest.mark.gpu


def _integrator(name):
    import mcbrat3d_amd as M
    _, domain, sun, rr, _, _, _ = BC.CASES[name]
    case = domain()
    dom = cases.product_domain(case)
    integ = M.new_Integrator(dom)
    integ.specifyParameters(minInverseTableSize=BC.TABLE, minForwardTableSize=BC.FWD, useRayTracing=True, useRussianRoulette=rr,
                            surfaceBDRF=cases.product_surface(case))
    mu0, phi0 = sun if sun is not None else (0.5, 30.0)  # (an emission render does not consult the source)
    integ.prepare(dom, M.new_PhotonStream(mu0, phi0, numberOfPhotons=10 ** 12))
    return integ, case


def _render(integ, name, case, grid_in_lds, samples, batches):
    """one call of the case's entry -> (batch means [batches, parts, receivers] in the oracle's units, the raw array)"""
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    _, _, _, _, entry, make, n = BC.CASES[name]
    rcv, rng = make(gridInLds=grid_in_lds), new_RandomNumberSequence(BC.SEED, BC.first_sample(n))
    if entry == "renderCamera":
        out = integ.renderCamera(rcv, rng, samples, batches)
    elif entry == "renderSensors":
        out = integ.renderSensors(rcv, rng, samples, batches, gridInLds=grid_in_lds)
    elif entry == "renderCameraPathLengths":
        out = integ.renderCameraPathLengths(rcv, BC.PATH_EDGES, samples, batches, seed=BC.SEED, firstSample=BC.first_sample(n))
    else:
        cell, sfc = BC.emission_sources(case)
        if entry == "renderCameraEmission":
            out = integ.renderCameraEmission(rcv, rng, samples, batches, cellSource=cell, surfaceSource=sfc)
        else:
            out = integ.renderSensorsEmission(rcv, rng, samples, batches, cellSource=cell, surfaceSource=sfc, gridInLds=grid_in_lds)
    assert out["dropped"] == 0
    raw = out["batchMeans"]
    nr = BC.paths(name)["receivers"]
    return raw.astype(np.float64).reshape(batches, -1, nr), raw


def _units(name, case):
    """per receiver: what the oracle's value is multiplied by (a sensor's w0), and the fixed-point step of a one-sample bin"""
    w0 = BC.paths(name)["w0"]
    largest = float(max(s.max() for s in BC.emission_sources(case))) if BC.MODE[BC.CASES[name][4]] == "emission" else 1.0
    return w0, BC.STEP * largest * w0


@pytest.mark.parametrize("name", list(BC.CASES))
def test_every_clean_path_agrees_with_the_oracle(name):
    """Measured on the MI355X, largest relative deviation of a clean path (its share of the tolerance): A pinhole 5.5e-4 (0.55), A
    orthographic 4.4e-5 (0.04), B 5.2e-4 (0.52), C 0.47 of the tolerance on a value of 5e-11, sensors 1.6e-5 (0.016), emission
    2.3e-7 and 2.0e-7, path lengths 7.8e-4 in one bin (0.78); medians 3e-8 to 1.2e-6; the means over all paths agree to 1e-8 ..
    7e-8, B 4e-6.  Each case runs in about a second."""
    integ, case = _integrator(name)
    n = BC.CASES[name][6]
    got, raw0 = _render(integ, name, case, 0, 1, n)
    _, raw1 = _render(integ, name, case, 1, 1, n)
    integ.finalize()
    assert raw0.tobytes() == raw1.tobytes()                                  # gridInLds 0 and 1: the same bytes
    p, d = BC.paths(name), BC.design(name)
    w0, step = _units(name, case)
    got = got.transpose(2, 0, 1).reshape(p["receivers"] * n, -1)              # receiver-major like the oracle's arrays, [m, parts]
    ref = BC.values(name, d["ref"]) * w0[p["receiver"]][:, None]
    tol = BC.RTOL * np.abs(ref) + step[p["receiver"]][:, None] + 2.0 ** -24 * np.abs(ref)
    clean = d["clean"]
    dev = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref[clean] > 0, dev[clean] / ref[clean], 0.0)
    worst = int(np.argmax((dev / tol)[clean].max(axis=1)))
    print("%s: %d clean paths of %d; largest deviation / tolerance %.3g; largest relative deviation %.3g (99.9th percentile %.3g, median %.3g)" % (
        name, clean.sum(), clean.size, (dev / tol)[clean].max(), rel.max(), np.percentile(rel, 99.9), np.median(rel)))
    print("   the path furthest out: index %d, kernel %s, oracle %s, events %d" % (
        np.flatnonzero(clean)[worst], got[clean][worst], ref[clean][worst], d["ref"]["nEvents"][clean][worst]))
    # the mean over ALL paths, excluded ones included
    m_got, m_ref = got.mean(axis=0), ref.mean(axis=0)
    print("   mean over all paths: kernel %s oracle %s (relative %s)" % (m_got, m_ref, np.abs(m_got - m_ref) / m_ref))
    assert np.all(dev[clean] <= tol[clean]), "%d clean paths outside the tolerance" % int((dev[clean] > tol[clean]).any(axis=1).sum())
    # nothing deposited: exactly 0 (a path straight out of the top; a path-length bin without a deposit)
    nothing = clean[:, None] & (ref == 0.0)
    if BC.CASES[name][4] == "renderSensors":
        nothing[:, 1] = False                                                 # (the direct part is the sun ray's alone)
    assert np.all(got[nothing] == 0.0)
    assert np.all(np.abs(m_got - m_ref) <= 1e-3 * m_ref)


def test_batches_of_many_samples_are_the_means_of_the_paths():
    """Case A's pinhole, the same sample range at 197 samples per pixel in 3 batches: each batch mean is the mean of the kernel's
    own per-path values to float rounding (197 * 2^-24 relative) -- the pending-bin and wave-reduction paths, which a one-sample
    render skips.  Both renders have the scale 2^40 (mcbrat_backward.h: fixed_point -- the largest power of two, at most 2^40,
    that keeps 64 * samples of the largest estimate below 2^62), asserted from the largest value of the forward tables."""
    name, spp, batches = "A pinhole", 197, 3
    integ, case = _integrator(name)
    n = BC.CASES[name][6]
    assert spp * batches <= n
    per_path, _ = _render(integ, name, case, -1, 1, n)
    many, _ = _render(integ, name, case, -1, spp, batches)
    integ.finalize()
    inten = BC.oracle_setup(name)[2]
    largest = max(float(inten.tab.max()) / (4.0 * np.pi * 0.5), 1.0 / np.pi)
    for samples in (1, spp):
        assert 64.0 * samples * largest * 2.0 ** 40 < 2.0 ** 62                # the scale of both renders is the cap, 2^40
    want = per_path[:spp * batches, 0].reshape(batches, spp, -1).mean(axis=1)
    print("largest relative difference %.3g" % np.max(np.abs(many[:, 0] - want) / want))
    assert np.all(np.abs(many[:, 0] - want) <= spp * 2.0 ** -24 * want)
