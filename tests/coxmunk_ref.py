"""Independent numpy statement of the Cox-Munk ocean surface of DESIGN.md section 4.11.1 (reflectance factor R = pi f), written
from the formulas as the section states them -- Fresnel through the refraction angle, not through the library's rearrangement --
with the quadrature and the reference sampler the Cox-Munk tests compare against.

q = (U, n, rho_wc, a_w): wind speed at 10 m (m/s), refractive index, whitecap reflectance (0: none), water-leaving albedo."""
import functools
import math

import numpy as np

MU_MIN = 0.01
SAMPLE_MU_MIN = 2.0 ** -16  # the smallest cosine a sampled reflection leaves with: that of the Lambertian draw, sqrt(2^-32)
KIND = 3

# rho_dh from a 400 x 800-node quadrature of these formulas, as the model's statement records them: {q: {mu0: rho_dh}}
TABLE = {
    (2.0, 1.34, 0.0, 0.0): {1.0: 0.021116, 0.6: 0.041769, 0.2: 0.241818, 0.05: 0.443546},
    (7.0, 1.34, 0.22, 0.02): {1.0: 0.041642, 0.6: 0.063487, 0.2: 0.203276, 0.05: 0.348669},
    (15.0, 1.34, 0.22, 0.0): {1.0: 0.029330, 0.6: 0.048057, 0.2: 0.147102, 0.05: 0.249426},
}


def sigma2(U):
    return 0.003 + 0.00512 * U


def fresnel(n, cw):
    """Unpolarised Fresnel reflectance at local incidence cosine cw."""
    cw = np.asarray(cw, np.float64)
    ct = np.sqrt(1.0 - (1.0 - cw * cw) / (n * n))
    rs = (cw - n * ct) / (cw + n * ct)
    rp = (n * cw - ct) / (n * cw + ct)
    return 0.5 * (rs * rs + rp * rp)


def erfc(x):
    """math.erfc over an array, once per distinct value (a quadrature grid repeats its cosines along the azimuth)"""
    x = np.asarray(x, np.float64)
    u, inv = np.unique(x, return_inverse=True)
    return np.array([math.erfc(v) for v in u])[inv].reshape(x.shape)


def shadow_lambda(s2, mu):
    mu = np.asarray(mu, np.float64)
    s = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    sig = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        arg = np.where(s > 0.0, mu / (sig * np.where(s > 0.0, s, 1.0)), np.inf)
        lam = 0.5 * (sig * s / (mu * np.sqrt(np.pi)) * np.exp(-mu * mu / (s2 * s * s)) - erfc(arg))
    return np.where(s > 0.0, lam, 0.0)


def whitecaps(q):
    U, _, rho_wc, _ = q
    return min(1.0, 2.95e-6 * U ** 3.52) if rho_wc > 0.0 else 0.0


def slope_density(U, d_in, d_out):
    """-> (P, cos beta, cos omega) of the facet that mirrors d_in into d_out."""
    h = d_out - d_in
    hn = np.sqrt(np.sum(h * h, axis=-1))
    cb = h[..., 2] / hn
    cw = 0.5 * hn
    s2 = sigma2(U)
    with np.errstate(divide="ignore", over="ignore"):
        P = np.exp(-((1.0 - cb * cb) / (cb * cb)) / s2) / (np.pi * s2)
    return P, cb, cw


def reflectance(q, d_in, d_out):
    """R for arrays of directions d_in (..., 3) (arriving, z < 0) and d_out (..., 3) (leaving, z > 0)."""
    U, n, rho_wc, a_w = (float(v) for v in q)
    d_in, d_out = np.broadcast_arrays(np.asarray(d_in, np.float64), np.asarray(d_out, np.float64))
    mi = np.maximum(-d_in[..., 2], MU_MIN)
    mr = np.maximum(d_out[..., 2], MU_MIN)
    P, cb, cw = slope_density(U, d_in, d_out)
    S = 1.0 / (1.0 + shadow_lambda(sigma2(U), mi) + shadow_lambda(sigma2(U), mr))
    glint = np.pi * P * fresnel(n, cw) * S / (4.0 * mi * mr * cb ** 4)
    W = whitecaps((U, n, rho_wc, a_w))
    return (1.0 - W) * (glint + a_w) + W * rho_wc


def direction(mu, phi):
    """Unit vector of cosine mu (z) and azimuth phi."""
    mu, phi = np.broadcast_arrays(np.asarray(mu, np.float64), np.asarray(phi, np.float64))
    s = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    return np.stack([s * np.cos(phi), s * np.sin(phi), mu], axis=-1)


_leggauss = functools.lru_cache(maxsize=None)(np.polynomial.legendre.leggauss)  # (an eigenvalue problem: seconds at 800 nodes)


def _gauss(n, a, b):
    x, w = _leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def albedo(q, mu_i, n=400, nphi=800):
    """rho_dh(mu_i) = (1/pi) int R mu_r dOmega: n Gauss nodes in mu_r on each of [0, MU_MIN], [MU_MIN, mu_i], [mu_i, 1] (R has
    kinks at the clamp, and its glint peaks near mu_r = mu_i), nphi in the relative azimuth over [0, pi]."""
    cuts = sorted({0.0, MU_MIN, float(mu_i), 1.0})
    phi, wphi = _gauss(nphi, 0.0, np.pi)
    d_in = direction(-float(mu_i), 0.0)
    tot = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        x, w = _gauss(n, a, b)
        R = reflectance(q, d_in, direction(x[:, None], phi[None, :]))
        tot += np.sum(2.0 * (R @ wphi) / np.pi * x * w)
    return float(tot)


def glint_probability(q, mu_i):
    """p_g of the sampler's mixture."""
    U, n, rho_wc, a_w = (float(v) for v in q)
    W = whitecaps((U, n, rho_wc, a_w))
    g = (1.0 - W) * float(fresnel(n, mu_i))
    L = (1.0 - W) * a_w + W * rho_wc
    return g / (g + L) if g + L > 0.0 else 0.0


def lambert_direction(uX, uY):
    return direction(np.sqrt(uX), 2.0 * np.pi * uY)


def sample(q, d_in, u):
    """The sampler of section 4.11.1 for uniforms u (n, 3) = (component, u1, u2) -> (d_out (n, 3), weight (n,)): the glint
    component where u[:, 0] <= p_g, else the Lambertian draw of (u1, u2).  A mirror direction below the horizon, or closer to it
    than SAMPLE_MU_MIN, ends the photon (weight 0)."""
    U = float(q[0])
    d_in = np.asarray(d_in, np.float64)
    u = np.asarray(u, np.float64)
    pg = glint_probability(q, -d_in[2])
    d_out = lambert_direction(u[:, 1], u[:, 2])
    glint = (u[:, 0] <= pg) & (pg > 0.0)
    t2 = -sigma2(U) * np.log(np.maximum(1.0 - u[:, 1], np.finfo(np.float64).tiny))
    t = np.sqrt(t2)
    m = np.stack([t * np.cos(2 * np.pi * u[:, 2]), t * np.sin(2 * np.pi * u[:, 2]), np.ones_like(t)], axis=-1) / np.sqrt(1.0 + t2)[:, None]
    c = -(m @ d_in)
    mirror = d_in[None, :] + 2.0 * c[:, None] * m
    d_out = np.where(glint[:, None], mirror, d_out)
    dead = glint & ((c <= 0.0) | (mirror[:, 2] < SAMPLE_MU_MIN))
    safe = np.where(dead[:, None], np.array([0.0, 0.0, 1.0]), d_out)
    P, cb, cw = slope_density(U, d_in[None, :], safe)
    lam = safe[:, 2] / np.pi
    den = pg * P / (4.0 * cb ** 3 * cw) + (1.0 - pg) * lam
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(den > 0.0, reflectance(q, d_in[None, :], safe) * lam / den, 0.0)
    return d_out, np.where(dead, 0.0, w)
