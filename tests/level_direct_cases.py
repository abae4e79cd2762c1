"""Helpers shared by the tests of the direct / diffuse separation of the level fluxes (recDirectLevelFluxes, DESIGN.md section
4.13): the black twin of a medium, the media of the product-against-product comparison, and the optical depth above a level.

The black twin is the same medium with omega0 = 0 in every component, albedo 0 and no surface description.  On the same Philox
streams its photons make the first leg of the real medium's photons and end at the first collision or at the surface: its downward
level tally is, photon for photon, the direct tally of the real medium, and every weight in it is 1."""
import numpy as np

from tests import cases
from tests import level_cases as LC


def black_twin(case):
    out = {k: v for k, v in case.items() if k != "surface"}
    out["albedo"] = 0.0
    out["components"] = [dict(c, ssa=np.zeros_like(np.asarray(c["ssa"], np.float64))) for c in case["components"]]
    return out


def _cells(xe, ye, ze, seed, albedo=0.3):
    """Unlike cells of two components on the given edges, over a grey surface."""
    shape = (len(xe) - 1, len(ye) - 1, len(ze) - 1)
    rng = np.random.default_rng(seed)
    ext = rng.uniform(4.0, 30.0, shape)
    share = rng.uniform(0.2, 0.8, shape)
    comps = [dict(ext=ext * share, ssa=rng.uniform(0.6, 1.0, shape), pfIndex=np.ones(shape, np.int32), legendre=[cases.hg_legendre(0.7, 24)]),
             dict(ext=ext * (1.0 - share), ssa=rng.uniform(0.8, 1.0, shape), pfIndex=np.ones(shape, np.int32), legendre=[np.zeros(2, np.float32)])]
    return dict(name="direct", xe=np.asarray(xe, np.float64), ye=np.asarray(ye, np.float64), ze=np.asarray(ze, np.float64), albedo=albedo,
                components=comps)


def one_cell():
    return _cells([0.0, 0.0625], [0.0, 0.0625], [0.0, 0.046875], 21)


def thirty_three_columns():
    """33 x 1 x 2: more columns than half a wave and no multiple of anything -- the lanes of a wave deposit into different columns."""
    return _cells(0.015625 * np.arange(34), [0.0, 0.0625], [0.0, 0.03, 0.07], 22)


def vacuum():
    case = _cells(0.03125 * np.arange(4), 0.046875 * np.arange(3), [0.0, 0.03, 0.08, 0.1], 23, albedo=0.5)
    for c in case["components"]:
        c["ext"] = np.zeros_like(c["ext"])
    return case


# name -> (case maker, source, privateTallies, blockSize, roulette); source: keyword arguments of new_PhotonStream
def _exact(name):
    grid, mu0, phi0, priv, block, rr = LC.EXACT[name]
    return (lambda: LC.medium(grid)), dict(solarMu=mu0, solarAzimuth=phi0), priv, block, rr


MEDIA = {name: _exact(name) for name, v in LC.EXACT.items() if v[1] is not None}
MEDIA.update({
    "RandomAzimuth source": ((lambda: LC.medium("irregular")), dict(solarMu=0.5), 0, 256, True),
    "Flux source": ((lambda: LC.medium("irregular z")), dict(), 2, 512, True),
    "Spotlight source": ((lambda: LC.medium("irregular x y")), dict(solarMu=0.6, solarAzimuth=210.0, solarX=0.3, solarY=0.7), 0, 512, False),
    "one cell": (one_cell, dict(solarMu=0.5, solarAzimuth=30.0), 2, 256, True),
    "33 x 1 x 2": (thirty_three_columns, dict(solarMu=0.6, solarAzimuth=200.0), 0, 256, False),
})


def optical_depth_above_levels(case):
    """tau_k of a horizontally uniform case: the vertical optical depth between level k and the top, k = 0 .. nz."""
    ext = sum(np.asarray(c["ext"], np.float64) for c in case["components"])
    if ext.ndim == 3:
        assert np.all(ext == ext[:1, :1, :])
        ext = ext[0, 0]
    dtau = ext * np.diff(np.asarray(case["ze"], np.float64))
    return np.concatenate([np.cumsum(dtau[::-1])[::-1], [0.0]])
