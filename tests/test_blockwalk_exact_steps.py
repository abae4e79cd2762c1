"""The arithmetic identities the block walk's trimmed collision iteration rests on, and the host
predicate that picks its instantiation without periodic folds.  CPU only.

1. p + s * d, with s and d floats widened to double, equals fma(s, d, p) bit for bit: the product is exact.
2. A leg's Philox block (event, 0, idLo, idHi) from what is constant per photon -- the second round's product q0 and the low
   word of the first round's p1 -- equals plain Philox4x32-10.
3. "No record of mcbrat_block_decomposition has bit 0 (1) of w" means "no block covers the whole x (y) axis"."""
import ctypes as C
import ctypes.util
import math

import numpy as np

from oracle import oracle as O
from tests import cases
from tests.test_block_decomposition import decompose

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def _fma():
    if hasattr(math, "fma"):
        return math.fma
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = C.c_double
    libm.fma.argtypes = [C.c_double, C.c_double, C.c_double]
    return libm.fma


def _special_floats(rng, n):
    """float32 values of every kind: random bit patterns (all exponents, subnormals, NaN among them) and the edge values."""
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                     np.finfo(np.float32).tiny, 1.401298464324817e-45, -1.401298464324817e-45, 1.0, -1.0], np.float32)
    k = rng.integers(0, n, 200 * len(edge))
    v[k] = np.tile(edge, 200)
    # (exponent field 0: subnormals; exponent field 254: the largest binade)
    sub = rng.integers(0, n, n // 50)
    v[sub] = (rng.integers(1, 2 ** 23, len(sub), dtype=np.uint64).astype(np.uint32) | (rng.integers(0, 2, len(sub)).astype(np.uint32) << 31)).view(np.float32)
    big = rng.integers(0, n, n // 50)
    v[big] = (rng.integers(0, 2 ** 23, len(big), dtype=np.uint64).astype(np.uint32) | np.uint32(254 << 23)).view(np.float32)
    return v


def test_exact_product_makes_the_sum_an_fma():
    fma = _fma()
    rng = np.random.default_rng(31)
    n = 10 ** 6
    s, d = _special_floats(rng, n), _special_floats(rng, n)
    p = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
    half = n // 2  # (half of the positions as the kernel has them: finite, of the size of a domain)
    p[:half] = rng.uniform(-4.0, 4.0, half)
    p[rng.integers(0, n, 800)] = np.tile(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1.7976931348623157e308, -1.7976931348623157e308]), 100)
    with np.errstate(all="ignore"):
        s64, d64 = s.astype(np.float64), d.astype(np.float64)
        two = p + s64 * d64
    one = np.array([fma(a, b, c) for a, b, c in zip(s64.tolist(), d64.tolist(), p.tolist())], np.float64)
    nan2, nan1 = np.isnan(two), np.isnan(one)
    assert np.array_equal(nan2, nan1)
    assert np.array_equal(two.view(np.uint64)[~nan2], one.view(np.uint64)[~nan1])
    with np.errstate(all="ignore"):
        assert nan2.sum() > 100 and np.isinf(two).sum() > 100 and (np.abs(s64 * d64) < 1e-60).sum() > 100  # (the special kinds were there)


def _mulhilo(a, b):
    p = a.astype(np.uint64) * np.uint64(b)
    return (p >> np.uint64(32)).astype(np.uint32), (p & U32).astype(np.uint32)


def philox_plain(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, np.uint32).copy() for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        h0, l0 = _mulhilo(c0, M0)
        h1, l1 = _mulhilo(c2, M1)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = k0 + np.uint32(W0), k1 + np.uint32(W1)
    return np.stack([c0, c1, c2, c3], axis=-1)


def photon_constants(id_lo, k0, c1=0):
    """Once per photon: (q0 hi, q0 lo, lo(p1)) with p1 = M1 * idLo and q0 = M0 * (hi(p1) ^ c1 ^ k0)."""
    h1, l1 = _mulhilo(np.asarray(id_lo, np.uint32), M1)
    qh, ql = _mulhilo(h1 ^ np.asarray(c1, np.uint32) ^ np.asarray(k0, np.uint32), M0)
    return qh, ql, l1


def philox_leg(event, qh, ql, p1lo, id_hi, k0, k1):
    """The leg's block from the photon's constants: round 1's event half, round 2 with q0, then eight plain rounds."""
    event, id_hi, k0, k1 = (np.asarray(v, np.uint32).copy() for v in (event, id_hi, k0, k1))
    h0, l0 = _mulhilo(event, M0)
    e2, e3 = h0 ^ id_hi ^ k1, l0
    k0, k1 = k0 + np.uint32(W0), k1 + np.uint32(W1)
    h1, l1 = _mulhilo(e2, M1)
    d0, d1, d2, d3 = h1 ^ p1lo ^ k0, l1, qh ^ e3 ^ k1, ql
    for _ in range(8):
        k0, k1 = k0 + np.uint32(W0), k1 + np.uint32(W1)
        h0, l0 = _mulhilo(d0, M0)
        h1, l1 = _mulhilo(d2, M1)
        d0, d1, d2, d3 = h1 ^ d1 ^ k0, l1, h0 ^ d3 ^ k1, l0
    return np.stack([d0, d1, d2, d3], axis=-1)


def test_hoisted_philox_equals_plain_philox():
    rng = np.random.default_rng(32)
    n = 10 ** 4
    draw = lambda: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    id_lo, id_hi, k0, k1 = draw(), draw(), draw(), draw()
    event = rng.integers(0, 2 ** 20, n, dtype=np.uint64).astype(np.uint32)
    event[:100] = draw()[:100]
    with np.errstate(over="ignore"):
        qh, ql, p1lo = photon_constants(id_lo, k0)
        got = philox_leg(event, qh, ql, p1lo, id_hi, k0, k1)
        want = philox_plain(event, np.zeros(n, np.uint32), id_lo, id_hi, k0, k1)
    assert np.array_equal(got, want)
    for i in range(0, n, 997):  # (and the numpy restatement of plain Philox is the oracle's generator)
        assert [int(v) for v in want[i]] == O.philox4x32_10([int(event[i]), 0, int(id_lo[i]), int(id_hi[i])], [int(k0[i]), int(k1[i])])


def test_hoisted_philox_reproduces_the_known_answers():
    """Random123 kat_vectors for philox4x32-10 (tests/test_oracle_pin.py, tests/test_gpu_launch_units.py): the second counter
    word, 0 in a leg's block, enters the photon's constant where it is not."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for c, k, want in kat:
        with np.errstate(over="ignore"):
            qh, ql, p1lo = photon_constants([c[2]], [k[0]], [c[1]])
            got = philox_leg([c[0]], qh, ql, p1lo, [c[3]], [k[0]], [k[1]])
            assert [int(v) for v in philox_plain([c[0]], [c[1]], [c[2]], [c[3]], [k[0]], [k[1]])[0]] == want
        assert [int(v) for v in got[0]] == want


def three_layers_middle_split():
    """Three layers of one extinction each, the middle one alone split in x: the top and bottom blocks span x."""
    ext = np.zeros((8, 1, 6))
    ext[:, :, 0:2], ext[:, :, 4:6] = 3.0, 7.0
    ext[:4, :, 2:4], ext[4:, :, 2:4] = 20.0, 1.0
    return ext


def span_bits(ext):
    """(some record has bit 0, some record has bit 1) and the same by brute force from the records' cell ranges."""
    _, boxes = decompose(ext)
    nx, ny, _ = ext.shape
    by_bits = (bool(np.any(boxes[:, 6] & 1)), bool(np.any(boxes[:, 6] & 2)))
    brute = (any(x0 == 0 and x1 == nx for x0, x1 in boxes[:, 0:2]), any(y0 == 0 and y1 == ny for y0, y1 in boxes[:, 2:4]))
    return by_bits, brute


def test_span_predicate_is_the_brute_force_one():
    by_bits, brute = span_bits(cases.step_cloud()["components"][0]["ext"])
    assert by_bits == brute == (False, True)  # no block of the step cloud spans x (one cell in y: every block spans y)
    by_bits, brute = span_bits(np.full((8, 1, 8), 5.0))
    assert by_bits == brute == (True, True)
    by_bits, brute = span_bits(three_layers_middle_split())
    assert by_bits == brute == (True, True)
    checker = np.zeros((4, 2, 4))
    checker[...] = np.where((np.arange(4)[:, None, None] + np.arange(2)[None, :, None]) % 2 == 0, 4.0, 12.0)
    by_bits, brute = span_bits(checker)
    assert by_bits == brute == (False, False)
    seen = set()
    for seed in range(50):
        rng = np.random.default_rng(900 + seed)
        nx, ny, nz = int(rng.integers(1, 9)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
        ext = np.full((nx, ny, nz), float(rng.choice([0.0, 0.3, 4.0])))
        for _ in range(int(rng.integers(0, 6))):
            i0, j0, k0 = int(rng.integers(0, nx)), int(rng.integers(0, ny)), int(rng.integers(0, nz))
            i1 = nx if rng.random() < 0.3 else int(rng.integers(i0 + 1, nx + 1))
            j1 = ny if rng.random() < 0.3 else int(rng.integers(j0 + 1, ny + 1))
            ext[i0:i1, j0:j1, k0:int(rng.integers(k0 + 1, nz + 1))] = float(rng.choice([0.0, rng.uniform(0.5, 30.0)]))
        by_bits, brute = span_bits(ext)
        assert by_bits == brute, seed
        seen.add(by_bits)
    assert len(seen) >= 3  # (the random media hold both kinds on both axes)
