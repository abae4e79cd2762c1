// sensor_ray_dump -- a stand-alone program over mcbrat_sensor_ray.h alone: the ray mapping of the backward
// sensors checked against its closed forms, with no library and no GPU.  tests/test_sensors_host.py builds it plain and with
// -fsanitize=address,undefined and runs both.
//   sensor_ray_dump                                 every check below; prints one line per check, exit status 1 where one fails
//   sensor_ray_dump kind nx ny nz u v a c           origin and direction of one draw of the sensor at (0.25, -1.5, 0.75) with edges
//                                                   built perpendicular to the normal (the comparison with mcbrat_sensor_ray)
//
// The grid: a_i = (i + 1/2) h, c_j = (j + 1/2) h, h = 1/256 -- the midpoint rule in both draws.  Its errors, on which the moment
// tolerances below rest:
//   azimuth    256 equally spaced points over the full period integrate cos(k phi), sin(k phi) exactly for 0 < k < 256: every
//              first and second moment's azimuthal factor (k = 1, 2) is exact, up to the rounding of a sum of 65536 terms of size
//              <= 1 (<= 65536 * 2^-53 in the sum, 2^-53 in the mean; with the rounding of the terms themselves: 1e-13 is generous).
//   planar     mean d.n = sum h sqrt(a_i) -> int_0^1 sqrt(a) da = 2/3.  sqrt has a branch point at a = 0: the generalised
//              Euler-Maclaurin expansion (Navot 1961) gives the error zeta(-1/2, 1/2) h^(3/2) - h^2 f'(1) / 24 + O(h^4), with
//              zeta(-1/2, 1/2) = (2^(-1/2) - 1) zeta(-1/2) = 0.060888: 1.486e-5 - 3.2e-7 = 1.455e-5 at h = 1/256.  Tolerance
//              2e-5 (the prediction and a third of it); half the prediction, 7e-6, must be exceeded (the grid is the one assumed).
//   spherical  mu = 1 - 2a is linear: mean d = 0 to rounding.  mu^2 is a quadratic, for which the midpoint rule's error is exactly
//              -h^2 f'' / 24 = -h^2 / 3: mean mu^2 = 1/3 - h^2/3, and mean d_x^2 = mean d_y^2 = (1 - mean mu^2) / 2 = 1/3 + h^2/6.
//              Tolerance on mean d_i d_j - delta_ij / 3: h^2 / 3 + 1e-13 (5.1e-6), and the predicted values themselves to 1e-13.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../mcbrat3d_amd/csrc/mcbrat_sensor_ray.h"

namespace {

int failures = 0;

void check(bool ok, const char *what, double got, double bound) {
  std::printf("%s %s: %.6g (bound %.6g)\n", ok ? "ok    " : "FAILED", what, got, bound);
  if (!ok) failures++;
}

mcbrat_sensor make(int kind, const double n[3]) {
  mcbrat_sensor s = mcbrat_sensor();
  s.kind = kind; s.id = 7u;
  s.position[0] = 0.25; s.position[1] = -1.5; s.position[2] = 0.75;
  for (int a = 0; a < 3; ++a) s.normal[a] = n[a];
  // two edges perpendicular to the normal, of different lengths, not perpendicular to each other
  int k = 0;
  for (int a = 1; a < 3; ++a)
    if (std::fabs(n[a]) < std::fabs(n[k])) k = a;
  double ax[3] = {0.0, 0.0, 0.0};
  ax[k] = 1.0;
  const double c1[3] = {n[1] * ax[2] - n[2] * ax[1], n[2] * ax[0] - n[0] * ax[2], n[0] * ax[1] - n[1] * ax[0]};
  const double c2[3] = {n[1] * c1[2] - n[2] * c1[1], n[2] * c1[0] - n[0] * c1[2], n[0] * c1[1] - n[1] * c1[0]};
  for (int a = 0; a < 3; ++a) { s.e1[a] = 0.3 * c1[a]; s.e2[a] = 0.2 * c2[a] + 0.1 * c1[a]; }
  return s;
}

}  // namespace

int main(int argc, char **argv) {
  using namespace mcbrat;
  if (argc == 9) {
    const double n[3] = {std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4])};
    const mcbrat_sensor s = make(std::atoi(argv[1]), n);
    if (const char *msg = sensor_refusal(s)) {
      std::printf("refused: %s\n", msg);
      return 0;
    }
    SensorGeometry g;
    sensor_geometry(s, g);
    double o[3], d[3];
    sensor_ray(g, std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]), o, d);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", o[0], o[1], o[2], d[0], d[1], d[2]);
    return 0;
  }
  const double normals[9][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
                                {0.3, -0.5, 0.81}, {-2.0, 0.1, -0.4}, {0.57, 0.57, 0.59}};
  const int N = 256;
  const double h = 1.0 / N, two16 = 1.52587890625e-05;
  for (int kind = 0; kind < 2; ++kind) {
    for (int in = 0; in < 9; ++in) {
      const mcbrat_sensor s = make(kind, normals[in]);
      if (sensor_refusal(s)) { check(false, "sensor refused", (double)in, 0.0); continue; }
      SensorGeometry g;
      sensor_geometry(s, g);
      const double nn = std::sqrt(normals[in][0] * normals[in][0] + normals[in][1] * normals[in][1] + normals[in][2] * normals[in][2]);
      double n[3] = {0.0, 0.0, 1.0};
      if (kind == 0)
        for (int a = 0; a < 3; ++a) n[a] = normals[in][a] / nn;
      double worstLen = 0.0, minDot = 2.0, m1[3] = {0, 0, 0}, m2[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, mDot = 0.0;
      for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
          double o[3], d[3];
          sensor_ray(g, 0.5, 0.5, (i + 0.5) * h, (j + 0.5) * h, o, d);
          const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), dot = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
          worstLen = std::fmax(worstLen, std::fabs(len - 1.0));
          minDot = std::fmin(minDot, dot);
          mDot += dot;
          for (int a = 0; a < 3; ++a) {
            m1[a] += d[a];
            for (int b = 0; b < 3; ++b) m2[a][b] += d[a] * d[b];
          }
        }
      const double cnt = (double)N * N;
      std::printf("kind %d normal %g %g %g\n", kind, normals[in][0], normals[in][1], normals[in][2]);
      check(worstLen <= 1e-14, "unit length", worstLen, 1e-14);
      if (kind == 0) {
        check(minDot >= two16, "d.n >= 2^-16", minDot, two16);
        const double e = mDot / cnt - 2.0 / 3.0;
        check(std::fabs(e) <= 2e-5, "mean d.n - 2/3", e, 2e-5);
        check(std::fabs(e) >= 7e-6, "mean d.n - 2/3 is the midpoint rule's", e, 7e-6);
        // the components in the receiver's plane vanish: mean d = (mean d.n) n
        double worst = 0.0;
        for (int a = 0; a < 3; ++a) worst = std::fmax(worst, std::fabs(m1[a] / cnt - (mDot / cnt) * n[a]));
        check(worst <= 1e-13, "mean d - (mean d.n) n", worst, 1e-13);
      } else {
        double worst1 = 0.0, worst2 = 0.0, worstPred = 0.0;
        for (int a = 0; a < 3; ++a) {
          worst1 = std::fmax(worst1, std::fabs(m1[a] / cnt));
          for (int b = 0; b < 3; ++b) {
            const double m = m2[a][b] / cnt;
            worst2 = std::fmax(worst2, std::fabs(m - (a == b ? 1.0 / 3.0 : 0.0)));
            const double pred = a != b ? 0.0 : (a == 2 ? 1.0 / 3.0 - h * h / 3.0 : 1.0 / 3.0 + h * h / 6.0);
            worstPred = std::fmax(worstPred, std::fabs(m - pred));
          }
        }
        check(worst1 <= 1e-13, "mean d", worst1, 1e-13);
        check(worst2 <= h * h / 3.0 + 1e-13, "mean d_i d_j - delta_ij / 3", worst2, h * h / 3.0 + 1e-13);
        check(worstPred <= 1e-13, "mean d_i d_j - the midpoint rule's own value", worstPred, 1e-13);
      }
      // the origin: the four corners of the receiver, whatever a and c
      double worstO = 0.0;
      for (int cu = 0; cu < 2; ++cu)
        for (int cv = 0; cv < 2; ++cv) {
          double o[3], d[3];
          sensor_ray(g, (double)cu, (double)cv, 0.3, 0.9, o, d);
          for (int a = 0; a < 3; ++a) worstO = std::fmax(worstO, std::fabs(o[a] - (s.position[a] + cu * s.e1[a] + cv * s.e2[a])));
        }
      check(worstO <= 1e-15, "origin at the corners", worstO, 1e-15);
      // the ends of a: the clamp at 2^-16 (planar, a = 0), the normal itself (planar, a = 1), the two poles (spherical)
      double worstEnd = 0.0;
      for (int jc = 0; jc < 5; ++jc) {
        double o[3], d0[3], d1[3];
        sensor_ray(g, 0.5, 0.5, 0.0, 0.25 * jc, o, d0);
        sensor_ray(g, 0.5, 0.5, 1.0, 0.25 * jc, o, d1);
        const double dot0 = d0[0] * n[0] + d0[1] * n[1] + d0[2] * n[2];
        worstEnd = std::fmax(worstEnd, std::fabs(dot0 - (kind == 0 ? two16 : 1.0)));
        for (int a = 0; a < 3; ++a) worstEnd = std::fmax(worstEnd, std::fabs(d1[a] - (kind == 0 ? n[a] : -n[a])));
        worstEnd = std::fmax(worstEnd, std::fabs(std::sqrt(d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2]) - 1.0));
      }
      check(worstEnd <= 1e-15, "directions at a = 0 and a = 1", worstEnd, 1e-15);
    }
  }
  // what the header refuses
  {
    const double z[3] = {0.0, 0.0, 1.0}, zero[3] = {0.0, 0.0, 0.0};
    mcbrat_sensor s = make(2, z);
    check(sensor_refusal(s) != 0, "kind 2 refused", 0.0, 0.0);
    s = make(0, zero);
    s.e1[0] = s.e1[1] = s.e1[2] = s.e2[0] = s.e2[1] = s.e2[2] = 0.0;
    check(sensor_refusal(s) != 0, "zero normal refused", 0.0, 0.0);
    s = make(0, z);
    s.e1[2] = 1e-5;
    check(sensor_refusal(s) != 0, "edge not perpendicular refused", 0.0, 0.0);
    s = make(1, z);
    s.position[1] = NAN;
    check(sensor_refusal(s) != 0, "non-finite member refused", 0.0, 0.0);
    s = make(1, zero);
    check(sensor_refusal(s) == 0, "a spherical sensor ignores its normal", 0.0, 0.0);
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
