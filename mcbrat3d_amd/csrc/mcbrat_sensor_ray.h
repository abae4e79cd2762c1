// mcbrat_sensor_ray.h -- the one statement of the backward sensors' ray mapping: which point and which
// backward direction belong to the four numbers [u, v, a, c] of a path's first Philox block.  camera_kernel<.., SENSOR = true>
// (mcbrat_camera.hip) and the host function mcbrat_sensor_ray call the same sensor_ray() over the same SensorGeometry, which
// sensor_geometry() derives from a mcbrat_sensor on the host.  Plain C++ in double: no HIP header is needed to read it
// (tests/sensor_ray_dump.cpp includes nothing else); under hipcc sensor_ray() is __host__ __device__.
//
//   origin     position + u e1 + v e2 (a point sensor has e1 = e2 = 0: the position itself)
//   planar     cosine-weighted about the unit normal n: mu = max(sqrt(a), 2^-16), azimuth 2 pi c
//   spherical  uniform on the sphere: mu = 1 - 2 a, azimuth 2 pi c, about n = (0, 0, 1) whatever the sensor's normal
//   direction  d = sqrt((1 - mu)(1 + mu)) (cos(2 pi c) t1 + sin(2 pi c) t2) + mu n
//   basis      k = the axis with the smallest |n_k| (the lowest such axis on a tie), t1 = normalize(x_k - n_k n), t2 = n x t1:
//              (t1, t2, n) is right-handed, and n = (0, 0, 1) gives t1 = x, t2 = y -- the direction cosines of a Lambertian
//              reflection off the surface.
#pragma once
#include <math.h>

#include "../../include/mcbrat.h"

#if defined(__HIPCC__)
#define MCBRAT_SENSOR_HD __host__ __device__
#else
#define MCBRAT_SENSOR_HD
#endif

namespace mcbrat {

struct SensorGeometry {
  double position[3], e1[3], e2[3];
  double n[3], t1[3], t2[3];  // the basis the direction is formed in (spherical: x, y, z)
  int kind;
  unsigned id;                // stands where the camera's pixel stands in the Philox counter
  float direct;               // c / w0: what a path's direct estimate multiplies T_sun by (mcbrat_render_sensors sets it)
  float pad;
};

// What is wrong with a sensor that no context is needed to see, or NULL.  (Heights against the domain, and the tally budget,
// are mcbrat_render_sensors'.)
inline const char *sensor_refusal(const mcbrat_sensor &s) {
  if (s.kind != 0 && s.kind != 1) return "renderSensors: sensor kind must be 0 (planar) or 1 (spherical).";
  for (int a = 0; a < 3; ++a)
    if (!isfinite(s.position[a]) || !isfinite(s.e1[a]) || !isfinite(s.e2[a]) || !isfinite(s.normal[a]))
      return "renderSensors: a member of a sensor (position, e1, e2, normal) is not finite.";
  if (s.kind == 0) {
    const double n2 = s.normal[0] * s.normal[0] + s.normal[1] * s.normal[1] + s.normal[2] * s.normal[2];
    if (!(n2 > 0.0) || !isfinite(n2)) return "renderSensors: a planar sensor needs a non-zero normal.";
    const double nn = sqrt(n2);
    const double *e[2] = {s.e1, s.e2};
    for (int k = 0; k < 2; ++k) {
      const double dot = (e[k][0] * s.normal[0] + e[k][1] * s.normal[1] + e[k][2] * s.normal[2]) / nn;
      const double len = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
      if (!isfinite(len) || fabs(dot) > 1e-6 * len) return "renderSensors: an edge of a planar sensor is not perpendicular to its normal.";
    }
  }
  return 0;
}

// The geometry of a sensor that sensor_refusal() passes (direct = 0: the caller sets it)
inline void sensor_geometry(const mcbrat_sensor &s, SensorGeometry &g) {
  g = SensorGeometry();
  g.kind = s.kind; g.id = s.id;
  for (int a = 0; a < 3; ++a) { g.position[a] = s.position[a]; g.e1[a] = s.e1[a]; g.e2[a] = s.e2[a]; }
  if (s.kind == 0) {
    const double nn = sqrt(s.normal[0] * s.normal[0] + s.normal[1] * s.normal[1] + s.normal[2] * s.normal[2]);
    for (int a = 0; a < 3; ++a) g.n[a] = s.normal[a] / nn;
  } else {
    g.n[2] = 1.0;
  }
  int k = 0;
  for (int a = 1; a < 3; ++a)
    if (fabs(g.n[a]) < fabs(g.n[k])) k = a;
  double t[3], t2 = 0.0;
  for (int a = 0; a < 3; ++a) { t[a] = (a == k ? 1.0 : 0.0) - g.n[k] * g.n[a]; t2 += t[a] * t[a]; }
  const double inv = 1.0 / sqrt(t2);
  for (int a = 0; a < 3; ++a) g.t1[a] = t[a] * inv;
  g.t2[0] = g.n[1] * g.t1[2] - g.n[2] * g.t1[1];
  g.t2[1] = g.n[2] * g.t1[0] - g.n[0] * g.t1[2];
  g.t2[2] = g.n[0] * g.t1[1] - g.n[1] * g.t1[0];
}

// (cos, sin) of 2 pi c for c in [0, 1]: the quadrant from c itself, then the two kernels of fdlibm (k_cos.c, k_sin.c) on
// |r| <= pi / 4 -- no argument reduction of a general angle, and the same digits on the host and in the kernel
MCBRAT_SENSOR_HD inline void sensor_sincos_2pi(double c, double &cs, double &sn) {
  const double q = floor(4.0 * c + 0.5);
  const double r = (c - 0.25 * q) * 6.28318530717958647692;
  const double z = r * r;
  const double ss = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                    z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
  const double cc = 1.0 - 0.5 * z + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                    z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const int qi = (int)q & 3;
  cs = qi == 0 ? cc : (qi == 1 ? -ss : (qi == 2 ? -cc : ss));
  sn = qi == 0 ? ss : (qi == 1 ? cc : (qi == 2 ? -ss : -cc));
}

// Origin and backward direction (unit) of the draws [u, v, a, c], each in [0, 1]: sensor_ray(), in its two halves
MCBRAT_SENSOR_HD inline void sensor_origin(const SensorGeometry &g, double u, double v, double origin[3]) {
  for (int i = 0; i < 3; ++i) origin[i] = g.position[i] + u * g.e1[i] + v * g.e2[i];
}

MCBRAT_SENSOR_HD inline void sensor_direction(const SensorGeometry &g, double a, double c, double direction[3]) {
  double mu;
  if (g.kind == 0) {
    mu = sqrt(a);
    if (!(mu >= 1.52587890625e-05)) mu = 1.52587890625e-05;  // 2^-16, the smallest cosine of a Lambertian reflection
  } else {
    mu = 1.0 - 2.0 * a;
  }
  const double sinTheta = sqrt((1.0 - mu) * (1.0 + mu));
  double cphi, sphi;
  sensor_sincos_2pi(c, cphi, sphi);
  const double x = sinTheta * cphi, y = sinTheta * sphi;
  // (t1, t2, n) is orthonormal and x^2 + y^2 + mu^2 = 1, each to a few units of 2^-53: so is the length, and nothing is renormalised
  for (int i = 0; i < 3; ++i) direction[i] = x * g.t1[i] + y * g.t2[i] + mu * g.n[i];
}

MCBRAT_SENSOR_HD inline void sensor_ray(const SensorGeometry &g, double u, double v, double a, double c, double origin[3], double direction[3]) {
  sensor_origin(g, u, v, origin);
  sensor_direction(g, a, c, direction);
}

}  // namespace mcbrat
