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
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MCBRAT_HD __host__ __device__
#else
#define MCBRAT_HD
#endif

namespace mcbrat {

enum : int { BRDF_LAMBERTIAN = 0, BRDF_RPV = 1, BRDF_ROSSLI = 2 };
constexpr int kBrdfMaxParams = 4;   // parameters per patch, padded to four on the device (float4 per patch)
constexpr double kBrdfMuMin = 0.01;
// Energy rule: a patch is refused if its directional-hemispherical albedo exceeds 1 + 1e-3 at mu_i = 1/N, 2/N, .., 1 (N below).
// (Not down to mu_min: at incidence beyond 84 degrees the kernel-driven models exceed 1 for ordinary land parameters --
// RPV (0.3, 0.7, -0.1, 0.3) reaches 1.05 at mu_i = 0.05 and Ross-Li (0.3, 0.15, 0.05) 1.86 at 0.01.)
constexpr int kBrdfAlbedoGrid = 10;

MCBRAT_HD inline int brdf_num_params(int kind) { return kind == BRDF_RPV ? 4 : (kind == BRDF_ROSSLI ? 3 : (kind == BRDF_LAMBERTIAN ? 1 : 0)); }

// q: the patch's parameters -- Lambertian {a}; RPV {rho0, k, Theta, rhoC}; Ross-Li {fIso, fVol, fGeo}
MCBRAT_HD inline float brdf_reflectance(int kind, const float *q, double ix, double iy, double iz, double ox, double oy, double oz) {
  if (kind == BRDF_LAMBERTIAN) return q[0];
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

// host only (mcbrat_host.cpp): the parameter domains and the energy rule; null when q is allowed, else the refusal's text
const char *brdf_param_error(int kind, const float *q);

}  // namespace mcbrat
