"""What may not be combined, through the C ABI: every ordered pair of the settings below on a 2 x 2 x 2 grid with one component,
and every single setting under the thermal source (the direct and the side tally after level fluxes, which they need) followed
by a trace of one batch of 64 photons (only those cases trace to be refused: no other tally is refused only at trace time).
The return code of every call and the text of mcbrat_last_error are
held to tests/golden/refusal_matrix.json, which this same file recorded from the library as it was before the rules were put
into one list (mcbrat_variants.h):

    MCBRAT_LIB=<that library> python tests/test_gpu_refusal_matrix.py --record tests/golden/refusal_matrix.json

A refused call must also leave the context as it was: the moments' length and the walk mode do not change, and the next trace
of 64 photons succeeds and gives, bit for bit, the moments of a fresh context that was only given the accepted setting."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(ROOT, "tests", "golden", "refusal_matrix.json")
SEED, PHOTONS = 4242, 64


def _lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    try:  # (where PyTorch is installed it comes first: one HIP runtime per process)
        import torch  # noqa: F401
    except Exception:
        pass
    from mcbrat3d_amd import _capi
    return _capi.lib(), _capi.ptr


class Context:
    """a context with the 2 x 2 x 2 domain loaded: one component, Henyey-Greenstein, inverse and forward tables, a solar source"""
    def __init__(self, thermal=False):
        self.L, self.ptr = _lib()
        L, ptr = self.L, self.ptr
        self.ctx = L.mcbrat_create(0)
        assert self.ctx
        e = np.array([0.0, 0.5, 1.0])
        one = np.ones(8)
        coef = (np.float32(0.85).astype(np.float64) ** np.arange(1, 17)).astype(np.float32)
        inv, fwd = np.zeros(101, np.float32), np.zeros(181, np.float32)
        self.ok(L.mcbrat_set_grid(self.ctx, 2, 2, 2, ptr(e), ptr(e), ptr(e)))
        self.ok(L.mcbrat_set_optics(self.ctx, 1, ptr(2.0 * one), ptr(one), ptr(0.9 * one), ptr(np.ones(8, np.int32)), 0.2))
        assert L.mcbrat_inverse_table_legendre(len(coef), ptr(coef), len(inv), ptr(inv)) == 0
        assert L.mcbrat_forward_table_legendre(len(coef), ptr(coef), len(fwd), ptr(fwd)) == 0
        self.ok(L.mcbrat_set_inverse_table(self.ctx, 1, len(inv), 1, ptr(inv)))
        self.ok(L.mcbrat_set_forward_table(self.ctx, 1, len(fwd), 1, ptr(fwd), None))
        self.ok(L.mcbrat_specify_parameters(self.ctx, 1, 1, C.c_float(-1.0)))
        if thermal:
            self.ok(L.mcbrat_set_source_emission(self.ctx, ptr(np.arange(1, 9) / 8.0), 0.5))
        else:
            self.ok(L.mcbrat_set_source_solar(self.ctx, C.c_float(0.5), C.c_float(0.0)))
        mus, phis = np.array([0.5, 0.8], np.float32), np.array([0.0, 90.0], np.float32)
        xs = np.array([0.0, 1.0])
        rpv = np.array([0.1, 0.8, -0.1, 0.5], np.float32)
        ctx = self.ctx
        self.setters = {
            "intensity": lambda: L.mcbrat_specify_intensity(ctx, 2, ptr(mus), ptr(phis), 0, C.c_float(0.3), 0, 0, 0, C.c_float(1e30)),
            "orders": lambda: L.mcbrat_specify_scattering_orders(ctx, 1),
            "limit": lambda: L.mcbrat_specify_intensity(ctx, 0, None, None, 0, C.c_float(0.3), 0, 0, 1, C.c_float(1.0)),
            "levels": lambda: L.mcbrat_specify_level_fluxes(ctx, 1),
            "direct": lambda: L.mcbrat_specify_direct_level_fluxes(ctx, 1),
            "actinic": lambda: L.mcbrat_specify_actinic_flux(ctx, 1),
            "side": lambda: L.mcbrat_specify_side_fluxes(ctx, 1),
            "rpv": lambda: L.mcbrat_set_surface_brdf(ctx, 1, 2, 2, ptr(xs), ptr(xs), 4, ptr(rpv)),
            "counters": lambda: L.mcbrat_enable_counters(ctx, 1),
        }

    def ok(self, rc):
        assert rc == 0, self.L.mcbrat_last_error(self.ctx)

    def state(self):
        return int(self.L.mcbrat_moments_length(self.ctx)), int(self.L.mcbrat_get_walk_mode(self.ctx))

    def call(self, name):
        """-> [return code, the error text of a failure]; a refused call has left the moments' length and the walk mode alone"""
        before = self.state()
        rc = self.setters[name]()
        if rc != 0:
            assert self.state() == before, (name, before, self.state())
        return [int(rc), self.L.mcbrat_last_error(self.ctx).decode() if rc else ""]

    def trace(self):
        """one batch of 64 photons -> ([return code, error text], the moments)"""
        self.ok(self.L.mcbrat_reset_moments(self.ctx))
        done = C.c_int64(0)
        rc = self.L.mcbrat_compute_radiative_transfer(self.ctx, SEED, 0, PHOTONS, 1, C.byref(done))
        if rc != 0:
            return [int(rc), self.L.mcbrat_last_error(self.ctx).decode()], None
        mom = np.zeros(8 + 2 * self.state()[0])
        self.ok(self.L.mcbrat_get_moments(self.ctx, self.ptr(mom)))
        return [0, ""], mom

    def close(self):
        self.L.mcbrat_destroy(self.ctx)


NAMES = ("intensity", "orders", "limit", "levels", "direct", "actinic", "side", "rpv", "counters")


def run_matrix():
    """-> (the record that is held to the golden file, the failures of the checks that need no golden file)"""
    record, wrong = {"pairs": {}, "thermal": {}}, []
    # the moments of a fresh context with no setting and with each single setting that is accepted alone
    alone = {}
    for name in (None,) + NAMES:
        c = Context()
        if name is None or c.call(name)[0] == 0:
            rc, alone[name] = c.trace()
            if rc[0] != 0:
                wrong.append(("a fresh context does not trace", name, rc))
        c.close()
    for a, b in itertools.permutations(NAMES, 2):
        c = Context()
        first = c.call(a)
        second = c.call(b)
        record["pairs"]["%s,%s" % (a, b)] = [first, second]
        # after a refusal: the context traces, and as a fresh one with what it had accepted would
        had = None if first[0] else a
        if second[0] != 0 and had in alone:
            rc, mom = c.trace()
            if rc[0] != 0 or not np.array_equal(mom, alone[had]):
                wrong.append(("the context is not as it was after the refusal", a, b, rc))
        c.close()
    for a in NAMES:  # (the direct and the side tally need level fluxes: those first, so that the trace is what refuses them)
        c = Context(thermal=True)
        record["thermal"][a] = [c.call(n) for n in (("levels", a) if a in ("direct", "side") else (a,))] + [c.trace()[0]]
        c.close()
    return record, wrong


def _pack(record):
    """the record as it is committed: every error text once, a call as its index (-1: accepted), one line per case"""
    texts = sorted({r[1] for part in record.values() for calls in part.values() for r in calls if r[0]})
    lines = ['{"texts": [\n%s\n]' % ",\n".join(json.dumps(t) for t in texts)]
    for part in ("pairs", "thermal"):
        rows = ['"%s": %s' % (key, json.dumps([texts.index(r[1]) if r[0] else -1 for r in calls])) for key, calls in sorted(record[part].items())]
        lines.append('"%s": {\n%s\n}' % (part, ",\n".join(rows)))
    return ",\n".join(lines) + "}\n"


def _unpack(packed):
    return {part: {key: [[1, packed["texts"][i]] if i >= 0 else [0, ""] for i in calls] for key, calls in packed[part].items()} for part in ("pairs", "thermal")}


@pytest.mark.gpu
def test_refusal_matrix():
    record, wrong = run_matrix()
    assert not wrong, wrong
    with open(GOLDEN) as f:
        golden = _unpack(json.load(f))
    assert sorted(record["pairs"]) == sorted(golden["pairs"]) and sorted(record["thermal"]) == sorted(golden["thermal"])
    for part in ("pairs", "thermal"):
        for key, want in golden[part].items():
            assert record[part][key] == want, (part, key, record[part][key], want)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record"
    rec, bad = run_matrix()
    assert not bad, bad
    with open(sys.argv[2], "w") as out:
        out.write(_pack(rec))
    print("%d pairs, %d thermal cases, %d refusals" % (len(rec["pairs"]), len(rec["thermal"]),
                                                      sum(r[0] != 0 for v in list(rec["pairs"].values()) + list(rec["thermal"].values()) for r in v)))
