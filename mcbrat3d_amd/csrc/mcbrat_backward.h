// mcbrat_backward.h -- the host rules of a backward render, each stated once: the loop bounds the kernel
// is given, the fixed-point scale of its bins, what a call may ask for, the launch shape, the statistics of the batch means.
// mcbrat_camera.hip's entries call these; tests/backward_dump.cpp includes nothing else.  Plain C++17 in double, no HIP header;
// every operation in a fixed order (the library is built with -ffp-contract=off, its outputs are compared bit for bit).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <initializer_list>

namespace mcbrat {

constexpr size_t kBackwardBinBudget = (size_t)4 << 30;  // bytes of bins at most, as the tracing kernels' batch slabs
constexpr double kTwoTo62 = 4.611686018427387904e18;    // a bin's sum stays below this
constexpr double kFlattestLeg = 65536.0;                // 1 / |cosine| of the flattest leg: 2^-16 is the smallest a Lambertian draw gives

// A ray toward the sun (`sun`: unit vector toward it) from anywhere in a domain H high and Lx x Ly wide, to the top: nz layers,
// and nx (ny) faces per domain length travelled along x (y), one length more for the part periods at both ends
struct SunBound { unsigned maxCross; float invFourPiMu0, invMu0; };  // invMu0: the ray's length per unit height (section 4.23)
inline SunBound sun_bound(int nx, int ny, int nz, double H, double Lx, double Ly, const float sun[3]) {
  const double muz = std::max((double)std::fabs(sun[2]), (double)FLT_MIN);
  const double wrapsX = std::floor(H * std::fabs((double)sun[0]) / muz / Lx) + 2.0, wrapsY = std::floor(H * std::fabs((double)sun[1]) / muz / Ly) + 2.0;
  const double n = (double)nz + wrapsX * nx + wrapsY * ny + 8.0;
  return {(unsigned)std::min(n, 4294967295.0), (float)(1.0 / (4.0 * 3.14159265358979323846 * muz)), (float)(1.0 / muz)};
}

// A leg: as a ray whose |cosine| is 2^-16; a flatter one that has not ended by then (in a vacuum) is dropped and counted
inline unsigned leg_bound(int nx, int ny, int nz, double H, double Lx, double Ly) {
  const double travel = H * kFlattestLeg;
  const double n = (double)nz + (std::floor(travel / Lx) + 2.0) * nx + (std::floor(travel / Ly) + 2.0) * ny + 8.0;
  return (unsigned)std::min(n, (double)(1u << 26));
}

// The fixed-point scale, as actScale is chosen: the power of two that keeps a bin's sum of `samples` paths that each hold 64 of the
// largest possible estimate (the largest of `candidates`) below 2^62; a path's own sum saturates where `samples` of it would pass that
struct FixedPoint { double scale, pathMax; };
inline FixedPoint fixed_point(long long samples, std::initializer_list<double> candidates) {
  int e = 0;
  std::frexp(kTwoTo62 / ((double)samples * std::max(candidates) * 64.0), &e);
  e = std::max(0, std::min(e - 1, 40));
  return {std::ldexp(1.0, e), std::floor(kTwoTo62 / (double)samples)};
}

// `arrays` (1 or 2) arrays of numBatches x n bins of 8 bytes fit the budget, and a bin's index fits 31 bits
inline bool bins_fit(unsigned long long n, unsigned long long numBatches, int arrays) {
  return n <= 0x7fffffffull && (unsigned long long)arrays * (n * numBatches) <= kBackwardBinBudget / sizeof(long long);
}
// a 64-bit index counts the paths of the call and the samples up to its last one
inline bool paths_fit(unsigned long long nBins, long long samples, unsigned long long firstSample, int numBatches) {
  return !((double)nBins * (double)samples >= 9.0e18 || (double)firstSample + (double)numBatches * (double)samples >= 1.8e19);
}

// 16 waves per compute unit (four per SIMD); a wave's lanes take 64 consecutive indices at a time, pathsPerLane times
struct LaunchShape { unsigned long long pathsPerLane, blocks; };
inline LaunchShape launch_shape(unsigned long long total, int numCUs, int block) {
  const unsigned long long lanes = (unsigned long long)numCUs * 16ull * 64ull;
  const unsigned long long perLane = std::max<unsigned long long>(1, (total + lanes - 1) / lanes), perBlock = perLane * (unsigned long long)block;
  return {perLane, (total + perBlock - 1) / perBlock};
}

// A path-length render keeps, behind the grid's share of LDS (rounded up to the 8 bytes a sum needs),
// one histogram of numBins 8-byte sums per wave of the workgroup and then the numBins edges as floats
constexpr size_t path_lds_offset(size_t gridBytes) { return (gridBytes + 7) & ~(size_t)7; }
constexpr size_t path_lds_bytes(int numBins, int block) { return (size_t)numBins * (8 * (size_t)(block / 64) + 4); }

// One series of batch means, given as its DIFFERENCES to the first batch (identical batches: exactly 0 throughout): the mean of
// the series is the first batch's value plus shift(), error() is the standard error of that mean
struct BatchSeries {
  double s1 = 0.0, s2 = 0.0;
  void add(double diff) { s1 += diff; s2 += diff * diff; }
  double shift(int numBatches) const { return s1 / (double)numBatches; }
  double error(int numBatches) const {
    const double nb = (double)numBatches, dm = s1 / nb;
    return std::sqrt(numBatches > 1 ? std::max(0.0, s2 - nb * dm * dm) / (nb * (nb - 1.0)) : 0.0);
  }
};

// The one reduction of a render's integer bins [arrays][numBatches][n][slots] -- n receivers (pixels, sensors) with `slots` sums
// each per batch (the path-length bins of a pixel), `arrays` 1 or 2 (the sensors' diffuse part, then their direct part) -- to
// floats: a value is its bin times unit[receiver], in double; every series is taken as differences to its first batch.
// mean, error: [array][slot][n]; totalError [slot][n]: of the per-batch sum of the two arrays, a series of its own formed as
// (f - f0) + (d - d0); batchMeans [batch][array][slot][n].  Any output pointer may be NULL.
struct BatchOutputs { float *mean[2], *error[2], *totalError, *batchMeans; };
inline void reduce_batches(const long long *bins, int arrays, int numBatches, size_t n, size_t slots, const double *unit, const BatchOutputs &out) {
  const size_t perArray = (size_t)numBatches * n * slots;
  for (size_t i = 0; i < n; ++i) {
    for (size_t s = 0; s < slots; ++s) {
      const long long *firstBin = bins + i * slots + s;  // of batch 0 of array 0: batch b of array a lies a * perArray + b * n * slots on
      double first[2] = {0.0, 0.0};
      for (int a = 0; a < arrays; ++a) first[a] = (double)firstBin[(size_t)a * perArray] * unit[i];
      BatchSeries series[3];
      for (int b = 0; b < numBatches; ++b) {
        double diff[2] = {0.0, 0.0};
        for (int a = 0; a < arrays; ++a) {
          const double m = (double)firstBin[(size_t)a * perArray + (size_t)b * n * slots] * unit[i];
          if (out.batchMeans) out.batchMeans[(((size_t)b * arrays + a) * slots + s) * n + i] = (float)m;
          diff[a] = m - first[a];
          series[a].add(diff[a]);
        }
        series[2].add(diff[0] + diff[1]);
      }
      for (int a = 0; a < arrays; ++a) {
        if (out.mean[a]) out.mean[a][s * n + i] = (float)(first[a] + series[a].shift(numBatches));
        if (out.error[a]) out.error[a][s * n + i] = (float)series[a].error(numBatches);
      }
      if (out.totalError) out.totalError[s * n + i] = (float)series[2].error(numBatches);
    }
  }
}

}  // namespace mcbrat
