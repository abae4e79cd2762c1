"""Independent numpy statement of the surface BRDF models of DESIGN.md section 4.11 (reflectance factor R = pi f), and the
quadratures the BRDF tests compare against: directional-hemispherical (black-sky) and bi-hemispherical (white-sky) albedo,
and the azimuthal mean that the doubling solver's surface operator needs."""
import numpy as np

MU_MIN = 0.01
KINDS = {"Lambertian": 0, "RPV": 1, "RossLi": 2}


def reflectance(kind, q, d_in, d_out):
    """R for arrays of directions d_in (..., 3) (arriving, z < 0) and d_out (..., 3) (leaving, z > 0); q the parameters."""
    q = np.asarray(q, np.float64)
    d_in = np.asarray(d_in, np.float64)
    d_out = np.asarray(d_out, np.float64)
    shape = np.broadcast(d_in[..., 0], d_out[..., 0]).shape
    if kind == 0:
        return np.full(shape, q[0])
    mi = np.maximum(-d_in[..., 2], MU_MIN)
    mr = np.maximum(d_out[..., 2], MU_MIN)
    cg = np.clip(-np.sum(d_in * d_out, axis=-1), -1.0, 1.0)
    a = d_in[..., :2] / mi[..., None]
    b = d_out[..., :2] / mr[..., None]
    G = np.hypot(a[..., 0] + b[..., 0], a[..., 1] + b[..., 1])
    if kind == 1:
        rho0, k, th, rhoC = q
        R = (rho0 * (mi * mr * (mi + mr)) ** (k - 1.0) * (1.0 - th * th) / (1.0 + 2.0 * th * cg + th * th) ** 1.5
             * (1.0 + (1.0 - rhoC) / (1.0 + G)))
    else:
        fIso, fVol, fGeo = q
        g = np.arccos(cg)
        kvol = ((np.pi / 2 - g) * cg + np.sin(g)) / (mi + mr) - np.pi / 4
        S = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        si, sr = 1.0 / mi, 1.0 / mr
        ct = np.clip(2.0 * np.sqrt(G * G + S * S) / (si + sr), -1.0, 1.0)
        t = np.arccos(ct)
        O = (t - np.sin(t) * ct) * (si + sr) / np.pi
        kgeo = O - si - sr + (1.0 + cg) * si * sr / 2.0
        R = fIso + fVol * kvol + fGeo * kgeo
    return np.maximum(R, 0.0)


def direction(mu, phi):
    """Unit vector of cosine mu (z) and azimuth phi."""
    mu, phi = np.broadcast_arrays(np.asarray(mu, np.float64), np.asarray(phi, np.float64))
    s = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    return np.stack([s * np.cos(phi), s * np.sin(phi), mu], axis=-1)


def _gauss(n, a, b):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def azimuthal_mean(kind, q, mu_i, mu_r, nphi=256):
    """(1 / 2 pi) int R(mu_i -> mu_r, phi) dphi for arrays mu_i (incidence cosine, > 0) and mu_r: R depends on the relative azimuth only."""
    mu_i = np.asarray(mu_i, np.float64)[..., None]
    mu_r = np.asarray(mu_r, np.float64)[..., None]
    phi, wphi = _gauss(nphi, 0.0, np.pi)  # (symmetric in the relative azimuth)
    d_in = direction(-mu_i, 0.0 * phi)
    d_out = direction(mu_r, phi + np.pi)  # phi = 0: exact backscatter
    return np.sum(reflectance(kind, q, d_in, d_out) * wphi, axis=-1) / np.pi


def albedo(kind, q, mu_i, n=96, nphi=128):
    """Directional-hemispherical albedo rho_dh(mu_i) = (1/pi) int R mu_r dOmega (the mu_r axis cut at mu_i and MU_MIN, where R has kinks)."""
    cuts = sorted({0.0, MU_MIN, float(mu_i), 1.0})
    tot = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            x, w = _gauss(n, a, b)
            tot += np.sum(2.0 * azimuthal_mean(kind, q, np.full_like(x, mu_i), x, nphi) * x * w)
    return tot


def white_sky_albedo(kind, q, n=48):
    x, w = _gauss(n, 0.0, 1.0)
    return 2.0 * sum(albedo(kind, q, m) * m * wi for m, wi in zip(x, w))
