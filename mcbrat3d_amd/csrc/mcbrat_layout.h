// The tally layout: where every part lies in one batch's tally slab, in the moment arrays (and the last batch's results, which
// have the moments' layout) and in the per-batch scalar scratch of the finish kernels.  This header is the definition: the host
// library sizes and reads its buffers by it, the finish kernels index by it (FinishParams carries a TallyLayout by value), and
// tests/tally_layout_dump.cpp prints it.  Plain C++17, no HIP.  (trace_kernel keeps lines of its own for its slab starts -- they
// are folded per template instantiation; tests/test_tally_layout_host.py holds them to this header.)
//
// One batch's slab, in elements (long long bins), nLvl = nz + 1:
//   [fluxUp ncol | fluxDown ncol | volume ncol nz | intensity ncol nDir |
//    (limitIntensityContributions:) intensity by component ncol nDir (nc+1) | excess nDir (nc+1) |
//    (scattering orders:) upByOrd ncol nOrd | downByOrd ncol nOrd | intensityByOrd ncol nDir nOrd |
//    (level fluxes:) levelUp ncol nLvl | levelDown ncol nLvl (with the direct tally: diffuse) | (direct tally:) levelDirect ncol nLvl |
//    (actinic flux:) actinic ncol nz |
//    (side fluxes:) sideXPlus ncol nz | sideXMinus ncol nz | sideYPlus ncol nz | sideYMinus ncol nz]
// The level, actinic and side bins always stay in global memory; what lies in front of them may live in LDS (slabLds elements).
// One sum of the moments (the array is header(8) + S1 + S2; the caller's view is in include/mcbrat.h): the means, column fluxes,
// profile, volume and intensity, then a tail per tally, each [domain means | column or cell bins]: orders, levels, direct, actinic, side
// (side: [means 4 nz | bins 4 ncol nz], both in the order x plus, x minus, y plus, y minus).
// The scalar scratch of a launch round of nb batches: [nb][3 + nz], then the order, level, actinic and side means: part X at scalX * nb.
#pragma once
#include <cstdint>

namespace mcbrat {

struct TallyShape {
  int32_t nx, ny, nz, nc, nDir, limitContrib;
  int32_t nOrd;  // numRecScatOrd + 1, 0 when off
  int32_t levels, direct, actinic;
  int32_t side = 0;  // the flux through the vertical faces of every cell (needs levels)
};

// Starts in elements: slab* within one batch's slab, mom* within one sum of the moments (and within the last batch's results), scal*
// within the scalar scratch per batch.  Kept tally by tally: a finish kernel's part reads neighbours (the kernel argument loads of
// neighbouring fields are merged, and a merged load that serves several parts stays in scalar registers across all of them).
struct TallyLayout {
  int64_t slabStride, slabLds, momentsLen, scalPerBatch;  // the lengths; slabLds: the elements in front of the level and actinic bins
  int64_t slabFluxUp, slabFluxDown, momMeans, momColumns, momProfile;
  int64_t slabVolume, momVolume;
  int64_t slabIntensity, momIntensity, slabByComponent, slabExcess;  // (the last two: limitIntensityContributions)
  int64_t slabOrders, momOrders, scalOrders;
  int64_t slabLevels, momLevels, momDirect, scalLevels;
  int64_t slabActinic, momActinic, scalActinic;
  int64_t slabSide, momSide, scalSide;
};

// Products and sums of counts that saturate: numRecScatOrd and the number of directions arrive unchecked, and a part's length
// may pass 2^64.  A saturated layout fits no budget (tally_fit) and is never indexed by.
constexpr int64_t kTallySaturated = INT64_MAX;
constexpr int64_t tally_times(int64_t a, int64_t b) {
  return a <= 0 || b <= 0 ? 0 : (a > kTallySaturated / b ? kTallySaturated : a * b);
}

// One forward pass: every part starts where the one before it ended.
inline TallyLayout tally_layout(const TallyShape &s) {
  int64_t at = 0;
  const auto take = [&at](int64_t n) {  // -> where the part of n elements starts
    const int64_t start = at;
    at = n > kTallySaturated - at ? kTallySaturated : at + n;
    return start;
  };
  const auto times = [](int64_t a, int64_t b, int64_t c = 1, int64_t d = 1) { return tally_times(tally_times(a, b), tally_times(c, d)); };
  const int64_t ncol = times(s.nx, s.ny), nz = s.nz, nLvl = s.levels ? nz + 1 : 0;
  const int64_t nDir = s.nDir, nOrd = s.nOrd, nComp = s.limitContrib ? (int64_t)s.nc + 1 : 0;
  const bool direct = s.levels && s.direct;
  const int64_t nAct = s.actinic ? nz : 0;
  const int64_t nSide = s.side ? times(4, nz) : 0;  // (layers of the four side parts)
  TallyLayout l{};
  l.slabFluxUp = take(ncol);
  l.slabFluxDown = take(ncol);
  l.slabVolume = take(times(ncol, nz));
  l.slabIntensity = take(times(ncol, nDir));
  l.slabByComponent = take(times(ncol, nDir, nComp));
  l.slabExcess = take(times(nDir, nComp));
  l.slabOrders = take(times(ncol, 2 + nDir, nOrd));
  l.slabLds = at;
  l.slabLevels = take(times(ncol, nLvl, direct ? 3 : 2));
  l.slabActinic = take(times(ncol, nAct));
  l.slabSide = take(times(ncol, nSide));
  l.slabStride = at;
  at = 0;
  l.momMeans = take(3);
  l.momColumns = take(times(3, ncol));
  l.momProfile = take(nz);
  l.momVolume = take(times(ncol, nz));
  l.momIntensity = take(times(ncol, nDir));
  l.momOrders = take(times(1 + ncol, 2 + nDir, nOrd));
  l.momLevels = take(times(1 + ncol, 2, nLvl));
  l.momDirect = take(direct ? times(1 + ncol, 2, nLvl) : 0);
  l.momActinic = take(times(1 + ncol, nAct));
  l.momSide = take(times(1 + ncol, nSide));
  l.momentsLen = at;
  at = 0;
  take(3 + nz);
  l.scalOrders = take(times(2 + nDir, nOrd));
  l.scalLevels = take(times(direct ? 4 : 2, nLvl));
  l.scalActinic = take(nAct);
  l.scalSide = take(nSide);
  l.scalPerBatch = at;
  return l;
}

// The slab of a flux launch of the same domain: no intensity parts.
inline TallyShape flux_run(TallyShape s) { s.nDir = 0; s.limitContrib = 0; return s; }

// Whether one batch's bins fit a budget in bytes: the order part alone, the level, actinic and side bins alone, the whole stride.
struct TallyFit { bool orders, globalBins, stride; };
inline TallyFit tally_fit(const TallyShape &s, uint64_t budgetBytes) {
  const TallyLayout l = tally_layout(s);
  const int64_t most = (int64_t)(budgetBytes / sizeof(int64_t) < (uint64_t)kTallySaturated ? budgetBytes / sizeof(int64_t) : (uint64_t)kTallySaturated - 1);
  const auto fits = [&](int64_t from, int64_t to) { return to != kTallySaturated && to - from <= most; };
  return TallyFit{fits(l.slabOrders, l.slabLds), fits(l.slabLds, l.slabStride), fits(0, l.slabStride)};
}

}  // namespace mcbrat
