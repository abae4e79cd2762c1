// mcbrat_brdf.h -- surface BRDF models: one evaluator, compiled for the kernels and for the host
// (parameter checks, mcbrat_brdf_reflectance / mcbrat_brdf_albedo).
//
// The evaluator returns the reflectance factor R = pi f (f the BRDF; a Lambertian surface of albedo a has R = a) for the
// propagation direction d_in of the arriving photon (d_in.z < 0) and d_out of the leaving ray (d_out.z > 0), in the vector form
// of the geometry, so that no azimuth convention enters:
//   mu_i = max(-d_in.z, kBrdfMuMin), mu_r = max(d_out.z, kBrdfMuMin)   (the clamp is part of the model: it bounds R at grazing angles)
//   cos g = -(d_in . d_out)                                             (phase angle; g = 0 is exact backscatter, the hot spot)
//   G = | h_in / mu_i + h_out / mu_r |, S = | (h_in / mu_i) x (h_out / mu_r) |   (h: the horizontal part of a direction)
// R is clamped below at 0 (Ross-Li goes negative at grazing angles).  Arithmetic in double, rounded to float once.
//
// Cox-Munk (the ocean, section 4.11.1) is the one model with a sampler of its own, brdf_sample below: its glint lobe is too sharp
// for the Lambertian draw of the direction.  The evaluator and the sampler share coxmunk_terms, one statement of the model.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MCBRAT_HD __host__ __device__
#else
#define MCBRAT_HD
#endif

namespace mcbrat {

enum : int { BRDF_LAMBERTIAN = 0, BRDF_RPV = 1, BRDF_ROSSLI = 2, BRDF_COXMUNK = 3 };
constexpr int kBrdfMaxParams = 4;   // parameters per patch, padded to four on the device (float4 per patch)
constexpr double kBrdfMuMin = 0.01;
// Energy rule: a patch is refused if its directional-hemispherical albedo exceeds 1 + 1e-3 at mu_i = 1/N, 2/N, .., 1 (N below).
// (Not down to mu_min: at incidence beyond 84 degrees the kernel-driven models exceed 1 for ordinary land parameters --
// RPV (0.3, 0.7, -0.1, 0.3) reaches 1.05 at mu_i = 0.05 and Ross-Li (0.3, 0.15, 0.05) 1.86 at 0.01.)
constexpr int kBrdfAlbedoGrid = 10;
// The smallest cosine a sampled reflection leaves with: 2^-16 = sqrt(2^-32), the smallest the Lambertian draw mu = sqrt(u_X) can
// give.  The walk keeps distances along a leg in float and is built for that: a leg 2^24 cell widths long stops advancing.
constexpr double kBrdfSampleMuMin = 1.52587890625e-05;

MCBRAT_HD inline int brdf_num_params(int kind) {
  return (kind == BRDF_RPV || kind == BRDF_COXMUNK) ? 4 : (kind == BRDF_ROSSLI ? 3 : (kind == BRDF_LAMBERTIAN ? 1 : 0));
}

// ---- Cox-Munk: q = {U, n, rhoWc, aW} -- wind speed at 10 m (m/s), real refractive index of the water, whitecap reflectance
// (0: no whitecaps), Lambertian water-leaving albedo.  Isotropic slopes, sigma^2 = 0.003 + 0.00512 U (no wind direction).
//   h = d_out - d_in, cos b = h.z / |h| (facet tilt), cos w = |h| / 2 (local incidence), P = exp(-tan^2 b / sigma^2) / (pi sigma^2)
//   R_glint = pi P F(cos w) S / (4 mu_i mu_r cos^4 b), S = 1 / (1 + Lambda(mu_i) + Lambda(mu_r))
//   R = (1 - W)(R_glint + aW) + W rhoWc, W = min(1, 2.95e-6 U^3.52) where rhoWc > 0, else 0
// The clamps mu_i, mu_r >= kBrdfMuMin enter the denominator and Lambda only.

// Unpolarised Fresnel reflectance of the water at local incidence cosine c.  With g = n cos(theta_t) = sqrt((n^2 - 1) + c^2):
// r_s = (c - g) / (c + g), r_p = (n^2 c - g) / (n^2 c + g).  n = 1: n^2 - 1 = 0 and sqrt(c c) = c exactly, so F is an exact 0.
MCBRAT_HD inline double coxmunk_fresnel(double n, double c) {
  const double n2 = n * n;
  const double g = sqrt((n2 - 1.0) + c * c);
  const double sd = c + g, pd = n2 * c + g;
  if (!(sd > 0.0) || !(pd > 0.0)) return 0.0;  // (c = 0 with n = 1, the only such case: no interface, nothing is reflected)
  const double rs = (c - g) / sd, rp = (n2 * c - g) / pd;
  return 0.5 * (rs * rs + rp * rp);
}
// Lambda(mu) = [ sigma s / (mu sqrt(pi)) exp(-mu^2 / (sigma^2 s^2)) - erfc(mu / (sigma s)) ] / 2, s = sqrt(1 - mu^2); Lambda(1) = 0
MCBRAT_HD inline double coxmunk_lambda(double sigma2, double mu) {
  const double s2 = 1.0 - mu * mu;
  if (!(s2 > 0.0)) return 0.0;
  const double sigma = sqrt(sigma2), s = sqrt(s2);
  return 0.5 * (sigma * s / (mu * 1.7724538509055160273) * exp(-(mu * mu) / (sigma2 * s2)) - erfc(mu / (sigma * s)));
}
// whitecap fraction W
MCBRAT_HD inline double coxmunk_whitecaps(const float *q) {
  return q[2] > 0.f ? fmin(1.0, 2.95e-6 * pow((double)q[0], 3.52)) : 0.0;
}
// The glint term R_glint of the pair (d_in, d_out), and the density per solid angle of d_out with which the sampler's glint
// component draws it: P / (4 cos^3 b cos w).  Both 0 where the pair has no facet (h.z <= 0) or the water does not reflect (F = 0).
MCBRAT_HD inline void coxmunk_terms(const float *q, double ix, double iy, double iz, double ox, double oy, double oz, double &glint, double &pdf) {
  constexpr double kPi = 3.14159265358979323846;
  glint = 0.0;
  pdf = 0.0;
  const double hx = ox - ix, hy = oy - iy, hz = oz - iz;
  const double h2 = hx * hx + hy * hy + hz * hz;
  if (!(hz > 0.0)) return;
  const double hn = sqrt(h2);
  const double cb = fmin(hz / hn, 1.0), cw = 0.5 * hn;
  const double cb2 = cb * cb;
  const double sigma2 = 0.003 + 0.00512 * (double)q[0];
  const double P = exp(-((1.0 - cb2) / cb2) / sigma2) / (kPi * sigma2);
  pdf = P / (4.0 * cb2 * cb * cw);
  const double F = coxmunk_fresnel((double)q[1], cw);
  if (F == 0.0) return;
  const double mi = fmax(-iz, kBrdfMuMin), mr = fmax(oz, kBrdfMuMin);
  const double S = 1.0 / (1.0 + coxmunk_lambda(sigma2, mi) + coxmunk_lambda(sigma2, mr));
  glint = kPi * P * F * S / (4.0 * mi * mr * (cb2 * cb2));
}
// R of a Cox-Munk patch in double.  q = {U, 1, 0, a}: W = 0 and glint = 0 exactly, so R = (1 - 0)(0 + a) + 0 = a bit for bit.
MCBRAT_HD inline double coxmunk_reflectance(const float *q, double glint) {
  const double W = coxmunk_whitecaps(q);
  return (1.0 - W) * (glint + (double)q[3]) + W * (double)q[2];
}

// q: the patch's parameters -- Lambertian {a}; RPV {rho0, k, Theta, rhoC}; Ross-Li {fIso, fVol, fGeo}; Cox-Munk {U, n, rhoWc, aW}
MCBRAT_HD inline float brdf_reflectance(int kind, const float *q, double ix, double iy, double iz, double ox, double oy, double oz) {
  if (kind == BRDF_LAMBERTIAN) return q[0];
  if (kind == BRDF_COXMUNK) {
    double glint, pdf;
    coxmunk_terms(q, ix, iy, iz, ox, oy, oz, glint, pdf);
    return (float)fmax(coxmunk_reflectance(q, glint), 0.0);
  }
  const double mi = fmax(-iz, kBrdfMuMin), mr = fmax(oz, kBrdfMuMin);
  double cg = -(ix * ox + iy * oy + iz * oz);
  cg = fmin(fmax(cg, -1.0), 1.0);
  const double ax = ix / mi, ay = iy / mi, bx = ox / mr, by = oy / mr;
  const double gx = ax + bx, gy = ay + by;
  const double G2 = gx * gx + gy * gy;
  double R;
  if (kind == BRDF_RPV) {
    // rho0 [mu_i mu_r (mu_i + mu_r)]^(k-1) (1 - Theta^2) / (1 + 2 Theta cos g + Theta^2)^1.5 (1 + (1 - rhoC) / (1 + G)):
    // with k = 1, Theta = 0, rhoC = 1 every factor is exactly 1 and R = rho0 bit for bit
    const double rho0 = q[0], k = q[1], th = q[2], rhoC = q[3];
    const double m = pow(mi * mr * (mi + mr), k - 1.0);
    const double d = 1.0 + 2.0 * th * cg + th * th;
    const double hg = (1.0 - th * th) / (d * sqrt(d));
    const double hot = 1.0 + (1.0 - rhoC) / (1.0 + sqrt(G2));
    R = rho0 * m * hg * hot;
  } else {
    // RossThick + LiSparse-Reciprocal (h/b = 2, b/r = 1): fIso + fVol Kvol + fGeo Kgeo; with fVol = fGeo = 0, R = fIso bit for bit
    constexpr double kPi = 3.14159265358979323846;
    const double g = acos(cg), sg = sqrt(fmax(0.0, 1.0 - cg * cg));
    const double kvol = ((0.5 * kPi - g) * cg + sg) / (mi + mr) - 0.25 * kPi;
    const double si = 1.0 / mi, sr = 1.0 / mr, ss = si + sr;
    const double S = ax * by - ay * bx;
    const double ct = fmin(fmax(2.0 * sqrt(G2 + S * S) / ss, -1.0), 1.0);
    const double t = acos(ct), st = sqrt(fmax(0.0, 1.0 - ct * ct));
    const double O = (t - st * ct) * ss / kPi;
    const double kgeo = O - si - sr + 0.5 * (1.0 + cg) * si * sr;
    R = (double)q[0] + (double)q[1] * kvol + (double)q[2] * kgeo;
  }
  return (float)fmax(R, 0.0);
}

// The reflection's sampler: the direction a photon arriving along d_in leaves in, and the factor its weight is multiplied by.
// On entry d_out holds the Lambertian draw of the direction (mu = sqrt(u_X), azimuth 2 pi u_Y: the caller's, so that the kernel's
// own float expression stays the one statement of it).  Every model but Cox-Munk keeps it: factor = R(d_in, d_out).
// Cox-Munk draws from a one-sample mixture of the glint lobe and the Lambertian draw under the balance heuristic; u = {component,
// u1, u2} are three uniforms on [0, 1] that nothing else uses:
//   F0 = F(-d_in.z), L = (1 - W) aW + W rhoWc, pG = (1 - W) F0 / ((1 - W) F0 + L), 0 where that denominator is 0
//   glint (u[0] <= pG, pG > 0): a facet slope from P -- tan^2 b = -sigma^2 ln(1 - u1), azimuth 2 pi u2, normal m -- and the mirror
//     direction d_out = d_in + 2 c m, c = -d_in . m.  c <= 0 (the facet faces away) or d_out.z < kBrdfSampleMuMin (into the water,
//     or along it: what the estimate loses there is below R mu^2 = 2.4e-10 R): the photon ends, factor 0.
//     The density of d_out per solid angle is P / (4 cos^3 b cos w): P / cos^3 b for the normal, 1 / (4 cos w) for the mirror map.
//   Lambertian (else): the draw as it came, density d_out.z / pi.
//   factor = R (d_out.z / pi) / [ pG P / (4 cos^3 b cos w) + (1 - pG) d_out.z / pi ]
// With pG = 0 (n = 1, or a black sea surface under whitecaps alone) the factor is R itself and d_out is untouched: the photon's
// history is that of the plain estimator, bit for bit.  `glintSampling` = false asks for that plain estimator outright.
MCBRAT_HD inline void brdf_sample(int kind, const float *q, const double *d_in, const double *u, double *d_out, float &factor, bool glintSampling = true) {
  constexpr double kPi = 3.14159265358979323846;
  if (kind != BRDF_COXMUNK || !glintSampling) {
    factor = brdf_reflectance(kind, q, d_in[0], d_in[1], d_in[2], d_out[0], d_out[1], d_out[2]);
    return;
  }
  const double W = coxmunk_whitecaps(q);
  const double gw = (1.0 - W) * coxmunk_fresnel((double)q[1], fmin(fmax(-d_in[2], 0.0), 1.0));
  const double L = (1.0 - W) * (double)q[3] + W * (double)q[2];
  const double pG = (gw + L > 0.0) ? gw / (gw + L) : 0.0;
  if (!(pG > 0.0)) {
    factor = brdf_reflectance(kind, q, d_in[0], d_in[1], d_in[2], d_out[0], d_out[1], d_out[2]);
    return;
  }
  if (u[0] <= pG) {
    const double sigma2 = 0.003 + 0.00512 * (double)q[0];
    const double t2 = -sigma2 * log(fmax(1.0 - u[1], 2.2250738585072014e-308));  // (the log's argument: a positive normal number)
    const double t = sqrt(fmax(t2, 0.0)), cb = 1.0 / sqrt(1.0 + t2);
    const double phi = 2.0 * kPi * u[2];
    const double mx = t * cos(phi) * cb, my = t * sin(phi) * cb, mz = cb;
    const double c = -(d_in[0] * mx + d_in[1] * my + d_in[2] * mz);
    factor = 0.f;
    if (!(c > 0.0)) return;
    double ox = d_in[0] + 2.0 * c * mx, oy = d_in[1] + 2.0 * c * my, oz = d_in[2] + 2.0 * c * mz;
    const double on = sqrt(ox * ox + oy * oy + oz * oz);  // (1 but for rounding, and for a d_in that is a unit vector in float only)
    ox /= on; oy /= on; oz /= on;
    d_out[0] = ox; d_out[1] = oy; d_out[2] = oz;
    if (!(oz >= kBrdfSampleMuMin)) return;
  }
  double glint, pdf;
  coxmunk_terms(q, d_in[0], d_in[1], d_in[2], d_out[0], d_out[1], d_out[2], glint, pdf);
  const double R = fmax(coxmunk_reflectance(q, glint), 0.0);
  const double lam = d_out[2] / kPi;
  const double den = pG * pdf + (1.0 - pG) * lam;
  factor = den > 0.0 ? (float)(R * lam / den) : 0.f;
}

// host only (mcbrat_host.cpp): the parameter domains and the energy rule; null when q is allowed, else the refusal's text
const char *brdf_param_error(int kind, const float *q);

}  // namespace mcbrat
