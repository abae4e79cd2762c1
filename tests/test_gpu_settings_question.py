"""specifyParameters asks the library one question (mcbrat_settings_refusal), keeps the settings, and pushes them in one order
(mcbrat3d_amd/integrator.py: _push_order), on the 2 x 2 x 2 one-component domain of the refusal matrix
with 64 photons per trace:

1. every refusal specifyParameters can meet leaves the integrator as it was: its public fields, the moments' length, the walk
   mode, and the next trace, bit for bit that of a fresh integrator that was given the accepted settings only;
2. a surface given in the call that switches off what it is refused with is accepted;
3. a seeded walk over acceptable full settings ends, wherever it is stopped, where one call on a fresh integrator ends;
4. the question itself changes nothing."""
import numpy as np
import pytest

from tests import cases
from tests import side_cases as SC
from tests.test_kernel_variants_host import combinable

pytestmark = pytest.mark.gpu

SEED, PHOTONS = 4242, 64
MUS, PHIS = [0.5, 0.8], [0.0, 90.0]
RPV = (0.1, 0.8, -0.1, 0.5)  # rho0, k, Theta, rhoC


@pytest.fixture(scope="module")
def M():
    import mcbrat3d_amd
    return mcbrat3d_amd


@pytest.fixture(scope="module")
def dom():
    e = np.array([0.0, 0.5, 1.0])
    return cases.product_domain(SC.black(e, e, e, 2.0, albedo=0.2, ssa=0.9))


def _integrator(M, dom, counters=False, **settings):
    integ = M.new_Integrator(dom)
    if counters:
        integ.enableCounters(True)
    integ.specifyParameters(**settings)
    return integ


def _state(M, dom, integ):
    """(the public fields, the moments' length, the walk mode) with the domain loaded"""
    integ.prepare(dom, M.new_PhotonStream(solarMu=0.5, solarAzimuth=0.0, numberOfPhotons=10 ** 9))
    fields = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(integ).items() if not k.startswith("_")}
    return fields, integ.momentsLength(), integ.walkMode()


def _same_fields(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] is b[k] or a[k] == b[k] for k in a)


def _trace(M, dom, integ):
    from mcbrat3d_amd.integrator import new_RandomNumberSequence
    photons = M.new_PhotonStream(solarMu=0.5, solarAzimuth=0.0, numberOfPhotons=10 ** 9)
    integ.resetMoments()
    assert integ.computeRadiativeTransfer(dom, new_RandomNumberSequence(SEED), photons, PHOTONS) == PHOTONS
    return integ.moments().copy()


def _refusals(M):
    """(what the integrator holds, the call that is refused, its text): one call per rule of the question that specifyParameters
    can meet, in the rules' order (mcbrat_variants.h) -- the budget rules but the orders' need a grid of 2^26 columns: below"""
    rpv = M.new_SurfaceDescription(RPV, model="RPV")
    inten, limit, orders = dict(intensityMus=MUS, intensityPhis=PHIS), dict(limitIntensityContributions=True, maxIntensityContribution=5.0), dict(recScatOrd=True, numRecScatOrd=2)
    levels, direct, actinic, side = (dict(recLevelFluxes=True), dict(recLevelFluxes=True, recDirectLevelFluxes=True), dict(recActinicFlux=True),
                                     dict(recLevelFluxes=True, recSideFluxes=True))
    return [
        (orders, limit, "limitIntensityContributions cannot be combined with scattering orders"),
        (limit, orders, "limitIntensityContributions cannot be combined with scattering orders"),
        (levels, inten, "level fluxes.*cannot be combined with intensity directions"),
        (inten, levels, "level fluxes.*cannot be combined with intensity directions"),
        (levels, orders, "level fluxes.*cannot be combined with scattering orders"),
        (orders, levels, "level fluxes.*cannot be combined with scattering orders"),
        (levels, dict(surfaceBDRF=rpv), "level fluxes.*cannot be combined with a BRDF surface"),
        (dict(surfaceBDRF=rpv), levels, "level fluxes.*cannot be combined with a BRDF surface"),
        (dict(counters=True), levels, "level fluxes.*not available together with event counters / photon fates"),
        ({}, dict(recDirectLevelFluxes=True), "direct level fluxes.*need level fluxes"),
        (direct, dict(recLevelFluxes=False), "direct level fluxes.*need level fluxes"),
        (actinic, inten, "actinic flux.*cannot be combined with intensity directions"),
        (inten, actinic, "actinic flux.*cannot be combined with intensity directions"),
        (actinic, orders, "actinic flux.*cannot be combined with scattering orders"),
        (orders, actinic, "actinic flux.*cannot be combined with scattering orders"),
        (actinic, dict(surfaceBDRF=rpv), "actinic flux.*cannot be combined with a BRDF surface"),
        (dict(surfaceBDRF=rpv), actinic, "actinic flux.*cannot be combined with a BRDF surface"),
        (dict(counters=True), actinic, "actinic flux.*not available together with event counters / photon fates"),
        ({}, dict(numRecScatOrd=10 ** 8), "numRecScatOrd is too large.*4 GiB tally budget"),
        (actinic, direct, "actinic flux.*cannot be combined with direct level fluxes"),
        (direct, actinic, "actinic flux.*cannot be combined with direct level fluxes"),
        (side, dict(recDirectLevelFluxes=True), "side fluxes.*cannot be combined with direct level fluxes"),
        (side, actinic, "side fluxes.*cannot be combined with the actinic flux"),
        ({}, dict(recSideFluxes=True), "side fluxes.*need level fluxes"),
        (side, dict(recLevelFluxes=False), "side fluxes.*need level fluxes"),
    ]


def test_every_refusal_leaves_the_integrator_as_it_was(M, dom):
    from mcbrat3d_amd._capi import McbratError
    fresh = {}
    for held, asked, text in _refusals(M):
        key = repr(sorted((k, getattr(v, "model", v)) for k, v in held.items()))
        if key not in fresh:  # the trace of a fresh integrator that was given the accepted settings only
            other = _integrator(M, dom, **held)
            fresh[key] = _trace(M, dom, other)
            other.finalize()
        integ = _integrator(M, dom, **held)
        before = _state(M, dom, integ)
        with pytest.raises(McbratError, match=text):  # (with keywords that no rule is about: they are not kept either)
            integ.specifyParameters(useRussianRoulette=False, zetaMin=0.1, minForwardTableSize=10001, **asked)
        after = _state(M, dom, integ)
        assert _same_fields(before[0], after[0]) and before[1:] == after[1:], (held, asked, before, after)
        assert integ.useRussianRoulette and integ.zetaMin != 0.1
        assert np.array_equal(_trace(M, dom, integ), fresh[key]), (held, asked)
        integ.finalize()


def test_a_refused_budget_leaves_the_integrator_as_it_was(M, dom):
    """8192 x 8192 columns, set through the C ABI (no domain of that size is made): on 3 levels the two level parts are 3 GiB and
    fit, the three with the direct tally (4.5 GiB) and the level and side parts (7 GiB) do not; on 4 levels the level parts are
    4 GiB, the budget, and the actinic bins beside them 1.5 GiB more; on 5 levels the level parts are 5 GiB"""
    from mcbrat3d_amd._capi import McbratError, ptr
    integ = _integrator(M, dom)
    xe = np.arange(8193, dtype=np.float64)
    grid = lambda nz: integ._check(integ._lib.mcbrat_set_grid(integ._ctx, 8192, 8192, nz, ptr(xe), ptr(xe), ptr(np.arange(nz + 1, dtype=np.float64))))  # noqa: E731
    public = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(integ).items() if not k.startswith("_")}  # noqa: E731
    for nz, held, asked, text in ((2, dict(recLevelFluxes=True), dict(recDirectLevelFluxes=True), "direct level fluxes.*level bins.*4 GiB tally budget"),
                                  (2, dict(recLevelFluxes=True), dict(recSideFluxes=True), "side fluxes.*4 GiB tally budget"),
                                  (3, dict(recLevelFluxes=True), dict(recActinicFlux=True), "actinic flux.*4 GiB tally budget"),
                                  (3, dict(recActinicFlux=True), dict(recLevelFluxes=True), "actinic flux.*4 GiB tally budget"),
                                  (4, {}, dict(recLevelFluxes=True), "level fluxes.*level bins.*4 GiB tally budget")):
        integ.specifyParameters(recLevelFluxes=False, recDirectLevelFluxes=False, recActinicFlux=False, recSideFluxes=False)
        grid(nz)
        integ.specifyParameters(**held)
        before = public(), integ.momentsLength()
        with pytest.raises(McbratError, match=text):
            integ.specifyParameters(useRussianRoulette=False, **asked)
        assert _same_fields(before[0], public()) and integ.momentsLength() == before[1], (nz, held, asked)
    integ.finalize()


def test_a_surface_comes_after_what_it_is_refused_with_is_switched_off(M, dom):
    from mcbrat3d_amd._capi import McbratError
    rpv = M.new_SurfaceDescription(RPV, model="RPV")
    integ = _integrator(M, dom, recLevelFluxes=True)
    before = _state(M, dom, integ)
    with pytest.raises(McbratError, match="level fluxes.*cannot be combined with a BRDF surface"):
        integ.specifyParameters(surfaceBDRF=rpv)
    after = _state(M, dom, integ)
    assert _same_fields(before[0], after[0]) and before[1:] == after[1:] and integ.surfaceBDRF is None
    integ.specifyParameters(recLevelFluxes=False, surfaceBDRF=rpv)
    assert not integ.recLevelFluxes and integ.surfaceBDRF is rpv and integ.useSurfaceBDRF
    other = _integrator(M, dom, surfaceBDRF=rpv)
    assert integ.momentsLength() == other.momentsLength()
    assert np.array_equal(_trace(M, dom, integ), _trace(M, dom, other))
    integ.finalize()
    other.finalize()


def test_a_seeded_walk_ends_where_one_call_ends(M, dom):
    """40 calls, each with a random acceptable full setting (drawn on the host, by the predicate of
    tests/test_kernel_variants_host.py: nothing here asks the code under test what is acceptable)"""
    rng = np.random.default_rng(20261020)
    integ = _integrator(M, dom)
    seen = set()
    for call in range(1, 41):
        while True:
            nDir, limit, orders = int(rng.choice((0, 2))), bool(rng.integers(2)), int(rng.choice((-1, 0, 2)))
            levels, direct, actinic, side = (bool(b) for b in rng.integers(2, size=4))
            if combinable(dict(inten=nDir > 0, orders=orders >= 0, limit=limit, levels=levels, direct=direct, actinic=actinic, side=side, brdf=0, counters=0)):
                break
        setting = dict(intensityMus=MUS[:nDir], intensityPhis=PHIS[:nDir], limitIntensityContributions=limit, maxIntensityContribution=5.0,
                       recScatOrd=orders >= 0, numRecScatOrd=orders, recLevelFluxes=levels, recDirectLevelFluxes=direct, recActinicFlux=actinic,
                       recSideFluxes=side)
        integ.specifyParameters(**setting)
        seen.add((nDir, limit, orders, levels, direct, actinic, side))
        if call % 10 == 0:
            other = _integrator(M, dom, **setting)
            assert integ.momentsLength() == other.momentsLength(), (call, setting)
            assert np.array_equal(_trace(M, dom, integ), _trace(M, dom, other)), (call, setting)
            other.finalize()
    assert len(seen) > 10 and any(s[3] for s in seen) and any(s[5] for s in seen) and any(s[0] for s in seen) and any(s[2] >= 0 for s in seen)
    integ.finalize()


def test_the_question_changes_nothing(M, dom):
    integ = _integrator(M, dom, recLevelFluxes=True)
    L, ctx = integ._lib, integ._ctx
    assert L.mcbrat_specify_scattering_orders(ctx, 2) != 0  # (refused: an error text of the context's to keep)
    integ.prepare(dom, M.new_PhotonStream(solarMu=0.5, solarAzimuth=0.0, numberOfPhotons=10 ** 9))
    before = L.mcbrat_last_error(ctx), integ.momentsLength(), integ.walkMode()
    assert b"scattering orders" in before[0]
    #                                  nDir limit orders levels direct actinic side brdf
    assert L.mcbrat_settings_refusal(ctx, 0, 0, -1, 1, 1, 0, 0, 0) is None
    assert L.mcbrat_settings_refusal(ctx, 0, 0, -1, 0, 0, 1, 0, 0) is None
    assert L.mcbrat_settings_refusal(ctx, 2, 1, -1, 0, 0, 0, 0, 1) is None
    assert L.mcbrat_settings_refusal(ctx, 2, 0, -1, 1, 0, 0, 0, 0).startswith(b"specifyParameters: level fluxes (recLevelFluxes) cannot be combined with intensity directions")
    assert L.mcbrat_settings_refusal(ctx, 0, 0, -1, 0, 0, 0, 1, 0).startswith(b"specifyParameters: side fluxes (recSideFluxes) need level fluxes")
    assert L.mcbrat_settings_refusal(ctx, 0, 0, 10 ** 8, 0, 0, 0, 0, 0).startswith(b"specifyParameters: numRecScatOrd is too large")
    assert (L.mcbrat_last_error(ctx), integ.momentsLength(), integ.walkMode()) == before
    assert integ.recLevelFluxes and np.array_equal(_trace(M, dom, integ), _trace(M, dom, integ))
    integ.finalize()
