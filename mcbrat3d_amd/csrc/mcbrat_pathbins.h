// mcbrat_pathbins.h -- the path-length bins of mcbrat_render_camera_pathlengths: the one statement of
// which bin a length belongs to, compiled for the kernel (camera_kernel<.., PATHLEN = true>) and for the host (the entry's
// check of its edges; tests/pathbins_dump.cpp includes nothing else).  Plain C++, no HIP header.
//
// Bins are given by n LOWER edges e[0] = 0 < e[1] < .. < e[n - 1], floats: bin b holds e[b] <= L < e[b + 1], the last bin is
// open above, so every length has a bin and the bins of a pixel sum to its whole radiance.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MCBRAT_HD __host__ __device__
#else
#define MCBRAT_HD
#endif

namespace mcbrat {

constexpr int kMaxPathBins = 256;

// The bin of length L: the last b with edges[b] <= L, by binary search.  A value on an edge goes to the upper bin; anything
// below edges[0] (and a NaN, which compares with nothing) goes to bin 0.
MCBRAT_HD inline int path_bin(const float *edges, int n, float L) {
  int lo = 0, hi = n;  // edges[lo] <= L (or lo = 0), L < edges[hi] (or hi = n)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L >= edges[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// Why these n edges are refused, or null: 1 <= n <= kMaxPathBins; then the first edge is 0, every edge is finite, and they are
// strictly ascending
inline const char *path_edges_refusal(const float *edges, int n) {
  if (n < 1 || n > kMaxPathBins) return "numBins must be between 1 and 256.";
  if (!edges) return "no pathEdges array (a null pointer).";
  for (int b = 0; b < n; ++b)
    if (!isfinite(edges[b])) return "pathEdges holds a value that is not finite.";
  if (edges[0] != 0.0f) return "pathEdges[0] must be 0 (the bins are given by their lower edges).";
  for (int b = 1; b < n; ++b)
    if (!(edges[b] > edges[b - 1])) return "pathEdges must be strictly ascending.";
  return nullptr;
}

}  // namespace mcbrat
