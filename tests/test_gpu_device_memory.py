"""Every device allocation of the host library has one owner (mcbrat3d_amd/csrc/mcbrat_devmem.h): what a context allocates over
its life goes with it, and a failed or refused call leaves nothing behind.  Through the C ABI, on
mcbrat_live_device_allocations(): every assertion is on the difference around the test's own contexts (other contexts of the
process may be alive)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_refusal_matrix import Context, _lib

pytestmark = pytest.mark.gpu
SEED = 4242


def _live():
    return int(_lib()[0].mcbrat_live_device_allocations())


def _f(x):
    return C.c_float(x)


class Life:
    """a context driven through the C ABI, call by call"""
    def __init__(self):
        self.L, self.ptr = _lib()
        self.ctx = self.L.mcbrat_create(0)
        assert self.ctx
        coef = (np.float32(0.85).astype(np.float64) ** np.arange(1, 17)).astype(np.float32)
        self.inv, self.fwd = np.zeros(101, np.float32), np.zeros(181, np.float32)
        assert self.L.mcbrat_inverse_table_legendre(len(coef), self.ptr(coef), len(self.inv), self.ptr(self.inv)) == 0
        assert self.L.mcbrat_forward_table_legendre(len(coef), self.ptr(coef), len(self.fwd), self.ptr(self.fwd)) == 0

    def ok(self, rc):
        assert rc == 0, self.L.mcbrat_last_error(self.ctx)

    def refused(self, rc, text):
        assert rc != 0 and text in self.L.mcbrat_last_error(self.ctx).decode(), (rc, self.L.mcbrat_last_error(self.ctx))

    def domain(self, nx, ny, nz, nc, layerExt):
        """the grid on the unit cube and a medium of horizontal slabs (layerExt: the extinction of every layer), nc components
        whose other optics are one value each: uniform per block of the block decomposition.  Tables and the solar source follow,
        as a caller sets a domain up."""
        L, ptr, ctx = self.L, self.ptr, self.ctx
        xe, ye, ze = (np.linspace(0.0, 1.0, n + 1) for n in (nx, ny, nz))
        self.ok(L.mcbrat_set_grid(ctx, nx, ny, nz, ptr(xe), ptr(ye), ptr(ze)))
        ncol, nvox = nx * ny, nx * ny * nz
        ext = np.repeat(np.asarray(layerExt, np.float64), ncol)
        cum = np.concatenate([np.full(nvox, (k + 1.0) / nc) for k in range(nc)])
        ssa = np.concatenate([np.full(nvox, 0.9 - 0.1 * k) for k in range(nc)])
        self.optics = (nc, ext, cum, ssa, np.ones(nc * nvox, np.int32))
        self.ok(self.set_optics())
        for k in range(nc):
            self.ok(L.mcbrat_set_inverse_table(ctx, k + 1, len(self.inv), 1, ptr(self.inv)))
            self.ok(L.mcbrat_set_forward_table(ctx, k + 1, len(self.fwd), 1, ptr(self.fwd), None))
        self.ok(L.mcbrat_specify_parameters(ctx, 1, 1, _f(-1.0)))
        self.solar()

    def set_optics(self, ext=None):
        """-> the return code (ext: another extinction array than the domain's)"""
        nc, e, cum, ssa, pfi = self.optics
        return self.L.mcbrat_set_optics(self.ctx, nc, self.ptr(e if ext is None else ext), self.ptr(cum), self.ptr(ssa), self.ptr(pfi), 0.2)

    def solar(self):
        self.ok(self.L.mcbrat_set_source_solar(self.ctx, _f(0.5), _f(0.0)))

    def directions(self, n, limit):
        mus, phis = np.array([0.5, 0.8], np.float32), np.array([0.0, 90.0], np.float32)
        self.ok(self.L.mcbrat_specify_intensity(self.ctx, n, self.ptr(mus) if n else None, self.ptr(phis) if n else None, 0, _f(0.3), 0, 0,
                                                1 if limit else 0, _f(1.0 if limit else 1e30)))

    def rpv(self, patches):
        """an RPV surface of patches x patches patches over the domain; 0: back to the domain's albedo"""
        if not patches:
            return self.ok(self.L.mcbrat_set_surface_brdf(self.ctx, 1, 0, 0, None, None, 0, None))
        xs = np.linspace(0.0, 1.0, patches + 1)
        params = np.repeat(np.array([0.1, 0.8, -0.1, 0.5], np.float32), patches * patches)  # [nParams][numY-1][numX-1]
        self.ok(self.L.mcbrat_set_surface_brdf(self.ctx, 1, patches + 1, patches + 1, self.ptr(xs), self.ptr(xs), 4, self.ptr(params)))

    def fates(self, n=64):
        out = np.zeros(n, dtype=np.dtype([("fate", "<i4"), ("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("nScatter", "<i4"), ("nEvents", "<i4"), ("weight", "<f4")]))
        return self.L.mcbrat_trace_fates(self.ctx, SEED, 0, n, self.ptr(out))

    def call(self, ppb=4096, nBatches=2):
        done = C.c_int64(0)
        self.ok(self.L.mcbrat_compute_radiative_transfer(self.ctx, SEED, 0, ppb, nBatches, C.byref(done)))
        assert done.value == ppb * nBatches

    def moments(self):
        mom = np.zeros(8 + 2 * int(self.L.mcbrat_moments_length(self.ctx)))
        self.ok(self.L.mcbrat_get_moments(self.ctx, self.ptr(mom)))
        return mom

    def destroy(self):
        self.L.mcbrat_destroy(self.ctx)
        self.ctx = None


def test_a_full_life_frees_everything_it_allocated():
    """Every buffer the library can allocate, most of them more than once.  The refusal rules (mcbrat_variants.h) do not accept
    all the tallies at once, so they are on in turn, a call each: directions with limitIntensityContributions over the BRDF
    surface; directions with scattering orders over it; level fluxes with their direct tally; level fluxes with side fluxes --
    the last one for three calls, so that every lane of the asynchronous mode has traced."""
    before = _live()
    c = Life()
    L, ptr, ctx = c.L, c.ptr, c.ctx
    assert _live() > before
    # 8 x 8 x 5: divisible by four with nz >= 2 (flight tables), no more than 65536 cells (block tables); two components (collision
    # records); two slabs, uniform per block (optics per block)
    c.domain(8, 8, 5, 2, [2.0, 2.0, 0.5, 0.5, 0.5])
    assert int(L.mcbrat_get_walk_mode(ctx)) & 2  # (the block walk applies: its tables are in use)
    c.ok(c.fates())  # instrumented trace, before any tally is on
    nvox = 8 * 8 * 5
    c.ok(L.mcbrat_set_source_emission(ctx, ptr(np.arange(1, nvox + 1) / float(nvox)), 0.5))
    c.solar()
    for numLambda in (4, 9):  # (the second grows the buffers)
        dist = np.zeros(numLambda, np.int64)
        c.ok(L.mcbrat_frequency_distribution(ctx, SEED, 0, numLambda, ptr(np.linspace(1.0 / numLambda, 1.0, numLambda)), 1000, ptr(dist)))
        assert dist.sum() == 1000
    inp, out = np.arange(30, dtype=np.uint32), np.zeros(20, np.uint32)
    c.ok(L.mcbrat_philox4x32_10(ctx, 5, ptr(inp), ptr(out)))
    assert out.any()
    c.ok(L.mcbrat_set_async(ctx, 1))  # all four lanes
    c.directions(2, limit=True)
    c.rpv(3)
    c.call()
    # the tables are uploaded: a refused instrumented trace allocates nothing and frees nothing
    held = _live()
    assert held > before + 40  # (the counter counts: the grid, the optics, the walk's tables, the lanes)
    c.refused(c.fates(), "trace_fates: not available together with intensity directions.")
    assert _live() == held
    c.directions(2, limit=False)
    c.ok(L.mcbrat_specify_scattering_orders(ctx, 2))
    c.call()
    c.directions(0, limit=False)
    c.ok(L.mcbrat_specify_scattering_orders(ctx, -1))
    c.rpv(0)
    c.ok(L.mcbrat_specify_level_fluxes(ctx, 1))
    c.ok(L.mcbrat_specify_direct_level_fluxes(ctx, 1))
    c.call()
    c.ok(L.mcbrat_specify_direct_level_fluxes(ctx, 0))
    c.ok(L.mcbrat_specify_side_fluxes(ctx, 1))
    for _ in range(3):
        c.call()
    # another grid, not divisible by four, three components (no collision records): everything sized by the grid is made again
    c.domain(3, 2, 4, 3, [1.0, 1.0, 3.0, 3.0])
    c.call()
    c.domain(8, 8, 5, 2, [2.0, 2.0, 0.5, 0.5, 0.5])
    c.call()
    c.ok(L.mcbrat_synchronize(ctx))
    mom = c.moments()
    assert mom[8:].any()
    c.destroy()
    assert _live() == before


def test_failed_and_refused_calls_leave_the_count_as_it_was():
    before = _live()
    c = Life()
    L, ptr, ctx = c.L, c.ptr, c.ctx
    c.domain(2, 2, 2, 1, [2.0, 2.0])
    c.ok(L.mcbrat_reset_moments(ctx))
    c.call(64, 1)
    first = c.moments()

    def still_computes(want):
        c.ok(L.mcbrat_reset_moments(ctx))
        c.call(64, 1)
        assert np.array_equal(c.moments(), want)

    held = _live()
    bad = c.optics[1].copy()
    bad[3] = -1.0
    c.refused(c.set_optics(bad), "validateOpticalComponent: extinction must be >= 0.")
    assert _live() == held
    xs = np.array([0.0, 1.0])
    c.refused(L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(xs), 4, ptr(np.array([0.1, 0.8, -0.1, 1.5], np.float32))), "RPV parameters must satisfy")
    assert _live() == held
    c.refused(L.mcbrat_compute_radiative_transfer(ctx, SEED, 0, 0, 1, None), "computeRadiativeTransfer: Didn't process any photons.")
    assert _live() == held
    still_computes(first)
    assert _live() == held
    # level fluxes beside intensity directions: refused where they are asked for
    c.directions(2, limit=False)
    c.ok(L.mcbrat_reset_moments(ctx))
    c.call(64, 1)
    radiance = c.moments()
    held = _live()
    c.refused(L.mcbrat_specify_level_fluxes(ctx, 1), "level fluxes (recLevelFluxes) cannot be combined with intensity directions")
    assert _live() == held
    c.refused(L.mcbrat_compute_radiative_transfer(ctx, SEED, 0, 0, 1, None), "computeRadiativeTransfer: Didn't process any photons.")
    assert _live() == held
    still_computes(radiance)
    assert _live() == held
    c.destroy()
    assert _live() == before


def test_twenty_contexts_created_and_destroyed_in_a_row():
    before = _live()
    for _ in range(20):
        c = Context()
        rc, mom = c.trace()
        assert rc == [0, ""] and mom[8:].any()
        assert _live() > before
        c.close()
    assert _live() == before


def test_a_bound_moment_buffer_stays_the_callers():
    import torch
    before = _live()
    c = Life()
    L, ctx = c.L, c.ctx
    c.domain(2, 2, 2, 1, [2.0, 2.0])
    buf = torch.zeros(8 + 2 * int(L.mcbrat_moments_length(ctx)), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    c.ok(L.mcbrat_bind_moments(ctx, C.c_void_p(buf.data_ptr())))
    assert int(L.mcbrat_moments_device_pointer(ctx)) == buf.data_ptr()
    c.call(64, 1)
    want = c.moments()  # (synchronises; read through the library from the bound buffer)
    assert want[8:].any()
    c.destroy()
    assert _live() == before
    assert np.array_equal(buf.cpu().numpy(), want)  # still readable, and holds the moments
    # and the library's own moments, for the same photons, are these
    d = Life()
    d.domain(2, 2, 2, 1, [2.0, 2.0])
    d.call(64, 1)
    assert np.array_equal(d.moments(), want)
    d.destroy()
    assert _live() == before
