// mcbrat_expected.h -- the arithmetic of the expected-value estimator of the emission renders (DESIGN.md section 4.24;
// mcbrat_render_camera_emission_expected, mcbrat_render_sensors_emission_expected), each piece stated once and compiled for the
// kernels (camera_kernel<.., EXPECT = true>, emission_grid_kernel) and for the host (the entries' LDS rule;
// tests/expected_dump.cpp includes nothing else).  Plain C++, no HIP header.
//
// Every leg of a path deposits, with the weight w it starts with, the formal solution along its whole ray:
//     w sum over the cells v crossed   E[v] e^(-tau_in) (1 - e^(-dtau))      tau from the leg's origin
//   + w e^(-tau_sfc) (1 - a) S_sfc                                           where the ray meets the surface
// E[v] is the cell's emission per unit extinction.  Collisions and surface hits deposit nothing.
#pragma once
#include <math.h>
#include <stddef.h>

#ifndef MCBRAT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MCBRAT_HD __host__ __device__
#else
#define MCBRAT_HD
#endif
#endif

namespace mcbrat {

// Where a ray may stop adding.  A leg's weight is at most 1 and E[v] at most srcMax, the largest source value, so what is left
// of a ray behind optical depth tau is at most srcMax e^(-tau).  A path's sum is tallied in units of srcMax in steps of
// 2^-40 at the finest.  e^(-30) = 9.36e-14 < 2^-43 = 1.14e-13: what a cut at 30 leaves out is below an eighth of that step.
constexpr float kExpectedTauCut = 30.0f;

// e^(-tauIn) (1 - e^(-dTau)): the share of a segment of optical depth dTau that begins tauIn from the leg's origin.  Two
// library calls, each good to a few units in the last place at every argument: 1 - e^(-dTau) is -expm1f(-dTau), which does not
// cancel where dTau is small (thin air: the case the estimator is for); e^(-tauIn) is taken from the running optical depth
// itself and not as a running product, so that a ray through many thousand cells does not add up a rounding per cell.
MCBRAT_HD inline float expected_segment(float tauIn, float dTau) { return expf(-tauIn) * (-expm1f(-dTau)); }

// E[v] = S sum_c f_c (1 - omega0_c): f_c is the extinction share of component c, the differences of the cumulative fractions the
// component pick reads (cum[k * stride], k < nc - 1; the last one counts as 1 and is not read), ssa[c * stride] its
// single-scattering albedo.  Summed in double.  Exactly 0 where the cell's extinction is 0, whatever ssa and cum hold there.
MCBRAT_HD inline float expected_emission(int nc, const float *cum, const float *ssa, long long stride, float ext, float S) {
  if (!(ext > 0.0f)) return 0.0f;
  double below = 0.0, sum = 0.0;
  for (int c = 0; c < nc; ++c) {
    const double upto = c < nc - 1 ? (double)cum[c * stride] : 1.0;
    sum += (upto - below) * (1.0 - (double)ssa[c * stride]);
    below = upto;
  }
  return (float)((double)S * sum);
}

// The second grid in LDS: E[v] as floats, 4 bytes per cell as the extinction grid has, behind the edges and the extinction grid
// (where mcbrat_backward.h's path_lds_offset puts what an entry keeps beside them).  These bytes count against the LDS share
// together with the grid's: gridInLds = 1 is refused where the pair does not fit, -1 then leaves both in global memory.
MCBRAT_HD constexpr size_t grid_lds_bytes(int nx, int ny, int nz) {  // the edges (doubles), then the extinction grid (floats)
  return sizeof(double) * (size_t)(nx + ny + nz + 3) + sizeof(float) * (size_t)nx * (size_t)ny * (size_t)nz;
}
// where the second grid begins: behind the first, rounded up to 8 bytes
MCBRAT_HD constexpr size_t expected_lds_offset(int nx, int ny, int nz) { return (grid_lds_bytes(nx, ny, nz) + 7) & ~(size_t)7; }
MCBRAT_HD constexpr size_t expected_lds_bytes(int nx, int ny, int nz) { return sizeof(float) * (size_t)nx * (size_t)ny * (size_t)nz; }

}  // namespace mcbrat
