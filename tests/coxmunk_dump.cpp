// coxmunk_dump -- evaluates and samples a fixed list of Cox-Munk inputs through mcbrat_brdf.h alone, one line each
// (tests/test_coxmunk_host.py builds it plain and under the sanitizers with the host compiler and compares the lines).
#include <stdio.h>

#include "../mcbrat3d_amd/csrc/mcbrat_brdf.h"

using namespace mcbrat;

static void unit(double mu, double phi, double *d) {
  const double s = sqrt(fmax(0.0, 1.0 - mu * mu));
  d[0] = s * cos(phi); d[1] = s * sin(phi); d[2] = mu;
}

int main() {
  const float qs[][4] = {{2.f, 1.34f, 0.f, 0.f}, {7.f, 1.34f, 0.22f, 0.02f}, {15.f, 1.34f, 0.22f, 0.f}, {0.f, 1.34f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f},
                         {5.f, 1.f, 0.f, 0.3f}, {50.f, 2.f, 1.f, 1.f}, {0.f, 1.f, 1.f, 0.f}, {50.f, 1.f, 0.f, 1.f}};
  // incidence and exit cosines: ordinary, grazing at and below the clamp (0.01), and the exact limits 0 and 1
  const double mus[] = {1.0, 0.6, 0.2, 0.05, 0.01, 0.005, 1e-4, 1e-12, 0.0};
  const double phis[] = {0.0, 0.4, 3.14159265358979323846, 5.0};
  const double us[][3] = {{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, {0.0, 1.0, 0.5}, {0.5, 0.5, 0.25}, {0.01, 0.999999, 0.75}, {0.3, 1e-300, 0.1},
                          {0.99, 0.2, 0.9}, {0.0, 0.9, 0.5}, {0.0, 0.9, 0.0}};
  int lines = 0;
  for (const auto &q : qs)
    for (double mi : mus) {
      double dIn[3];
      unit(-mi, 0.3, dIn);
      for (double mr : mus)
        for (double phi : phis) {
          double dOut[3];
          unit(mr, phi, dOut);
          const float r = brdf_reflectance(BRDF_COXMUNK, q, dIn[0], dIn[1], dIn[2], dOut[0], dOut[1], dOut[2]);
          const float rr = brdf_reflectance(BRDF_COXMUNK, q, -dOut[0], -dOut[1], -dOut[2], -dIn[0], -dIn[1], -dIn[2]);
          printf("R %g %g %g %g | %g %g %g | %.9g %.9g\n", q[0], q[1], q[2], q[3], mi, mr, phi, r, rr);
          ++lines;
        }
      for (const auto &u : us)
        for (int sampling = 0; sampling < 2; ++sampling) {
          double dOut[3];
          unit(sqrt(u[1]), 6.283185307179586 * u[2], dOut);
          float f = -1.f;
          brdf_sample(BRDF_COXMUNK, q, dIn, u, dOut, f, sampling != 0);
          printf("S %g %g %g %g | %g | %g %g %g | %d | %.17g %.17g %.17g %.9g\n", q[0], q[1], q[2], q[3], mi, u[0], u[1], u[2], sampling, dOut[0], dOut[1],
                 dOut[2], f);
          ++lines;
        }
    }
  // the other models keep the Lambertian draw: factor = R
  const float rpv[4] = {0.3f, 0.7f, -0.1f, 0.3f}, lam[1] = {0.25f};
  const double dIn[3] = {0.6, 0.0, -0.8}, u[3] = {0.2, 0.3, 0.4};
  double dOut[3] = {0.0, 0.6, 0.8};
  float f;
  brdf_sample(BRDF_RPV, rpv, dIn, u, dOut, f);
  printf("S rpv %.9g %.9g\n", f, brdf_reflectance(BRDF_RPV, rpv, dIn[0], dIn[1], dIn[2], dOut[0], dOut[1], dOut[2]));
  brdf_sample(BRDF_LAMBERTIAN, lam, dIn, u, dOut, f);
  printf("S lambertian %.9g\n", f);
  printf("lines %d\n", lines + 2);
  return 0;
}
