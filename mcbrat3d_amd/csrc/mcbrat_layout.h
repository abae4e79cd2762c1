// The tally layout: where every part lies in one batch's tally slab, in the moment arrays (and the last batch's results, which
// have the moments' layout) and in the per-batch scalar scratch of the finish kernels.  This header is the definition: the host
// library sizes and reads its buffers by it, the finish kernels index by it (FinishParams carries a TallyLayout by value), and
// tests/tally_layout_dump.cpp prints it.  Plain C++17, no HIP.  trace_kernel takes its slab starts from the slab_*_start functions
// below, from its own counts and template flags, so that they fold per instantiation.
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
// (equal shapes have equal layouts: what a setter asks to learn whether the moments change length)
constexpr bool operator==(const TallyShape &a, const TallyShape &b) {
  return a.nx == b.nx && a.ny == b.ny && a.nz == b.nz && a.nc == b.nc && a.nDir == b.nDir && a.limitContrib == b.limitContrib && a.nOrd == b.nOrd &&
         a.levels == b.levels && a.direct == b.direct && a.actinic == b.actinic && a.side == b.side;
}

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

// A count that saturates instead of overflowing: the number type of the host's layout.
struct TallyCount {
  int64_t v;
  constexpr TallyCount(int64_t n) : v(n < 0 ? 0 : n) {}
  friend constexpr TallyCount operator*(TallyCount a, TallyCount b) { return tally_times(a.v, b.v); }
  friend constexpr TallyCount operator+(TallyCount a, TallyCount b) { return b.v > kTallySaturated - a.v ? kTallySaturated : a.v + b.v; }
};

// Where the parts of one batch's slab start: every part starts where the one before it ends.  Functions of counts in a number
// type N -- TallyCount for tally_layout(), a plain 64-bit integer for trace_kernel, which calls them with its own counts and
// template flags (the host has seen to it that nothing overflows there) and must not pay for the saturation.
//   nComp: nc + 1 with limitIntensityContributions, else 0; nOrd: numRecScatOrd + 1, 0 when off; levelParts: 0, 2, or 3 with the
//   direct tally; nAct: nz with the actinic flux, else 0.  Orders are refused with limitIntensityContributions (nComp defaults
//   to 0); the level, actinic and side bins belong to flux runs without orders, and trace_kernel says so at its calls (nDir = nOrd = 0).
template <class N> constexpr N slab_volume_start(N ncol) { return N(2) * ncol; }
template <class N> constexpr N slab_intensity_start(N ncol, N nz) { return slab_volume_start(ncol) + ncol * nz; }
template <class N> constexpr N slab_by_component_start(N ncol, N nz, N nDir) { return slab_intensity_start(ncol, nz) + ncol * nDir; }
template <class N> constexpr N slab_excess_start(N ncol, N nz, N nDir, N nComp) { return slab_by_component_start(ncol, nz, nDir) + ncol * nDir * nComp; }
// the order parts: 0 fluxUp by order, 1 fluxDown by order, 2 intensity by order (ncol nOrd bins each, the last nDir times that)
template <class N> constexpr N slab_orders_start(N ncol, N nz, N nDir, N nOrd, int part, N nComp = N(0)) {
  return slab_excess_start(ncol, nz, nDir, nComp) + nDir * nComp + N(part) * ncol * nOrd;
}
// the level parts: 0 up, 1 down (with the direct tally: diffuse), 2 direct (ncol (nz + 1) bins each)
template <class N> constexpr N slab_levels_start(N ncol, N nz, int part, N nDir, N nOrd, N nComp = N(0)) {
  return slab_orders_start(ncol, nz, nDir, nOrd, 0, nComp) + ncol * (N(2) + nDir) * nOrd + N(part) * ncol * (nz + N(1));
}
template <class N> constexpr N slab_actinic_start(N ncol, N nz, int levelParts, N nDir, N nOrd, N nComp = N(0)) {
  return slab_levels_start(ncol, nz, levelParts, nDir, nOrd, nComp);
}
template <class N> constexpr N slab_side_start(N ncol, N nz, int levelParts, N nAct, N nDir, N nOrd, N nComp = N(0)) {
  return slab_actinic_start(ncol, nz, levelParts, nDir, nOrd, nComp) + ncol * nAct;
}

// The slab through the functions above; the moments and the scalar scratch in one forward pass each.
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
  {
    using C = TallyCount;
    const C cCol = ncol, cNz = nz, cDir = nDir, cOrd = nOrd, cComp = nComp;
    const int levelParts = s.levels ? (direct ? 3 : 2) : 0;
    l.slabFluxUp = 0;
    l.slabFluxDown = ncol;
    l.slabVolume = slab_volume_start(cCol).v;
    l.slabIntensity = slab_intensity_start(cCol, cNz).v;
    l.slabByComponent = slab_by_component_start(cCol, cNz, cDir).v;
    l.slabExcess = slab_excess_start(cCol, cNz, cDir, cComp).v;
    l.slabOrders = slab_orders_start(cCol, cNz, cDir, cOrd, 0, cComp).v;
    l.slabLds = l.slabLevels = slab_levels_start(cCol, cNz, 0, cDir, cOrd, cComp).v;
    l.slabActinic = slab_actinic_start(cCol, cNz, levelParts, cDir, cOrd, cComp).v;
    l.slabSide = slab_side_start(cCol, cNz, levelParts, C(nAct), cDir, cOrd, cComp).v;
    l.slabStride = (C(l.slabSide) + cCol * C(nSide)).v;
  }
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

// ---------------------------------------------------------------------------------------------------------------------------------
// The parts of the two finish kernels (mcbrat_kernels.hip), in the order their workgroups are dealt out -- the order decides which
// workgroups start first.  finish_parts() is the one statement of that order and of every part's size: the host sizes both launches by
// it, FinishParams carries its result, and both kernels find a workgroup's part by walking the same arrays.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kFinishBlock = 256;                                                  // lanes of a finish workgroup
constexpr int kVolVox = 32, kVolGroups = kFinishBlock / kVolVox, kVolChunk = 64;  // the cell fold: bins / batch groups per workgroup, batches per pass

enum GatherPart { kGatherColumns, kGatherVolume, kGatherReduce, kGatherIntensity, kGatherOrders, kGatherOrderMeans, kGatherLevels,
                  kGatherLevelMeans, kGatherActinic, kGatherActinicMeans, kGatherSide, kGatherSideMeans, kGatherParts };
enum FoldPart { kFoldColumns, kFoldScalars, kFoldOrderMeans, kFoldLevelMeans, kFoldActinicMeans, kFoldSideMeans, kFoldParts };

// The means per batch of every tally with a scratch behind scalVals (0 when the tally is off), and the level quantities
// (up, down; with the direct tally direct and diffuse too).
constexpr int64_t level_quantities(const TallyShape &s) { return s.levels ? (s.direct ? 4 : 2) : 0; }
constexpr int64_t order_means(const TallyShape &s) { return (2 + (int64_t)s.nDir) * s.nOrd; }
constexpr int64_t level_means(const TallyShape &s) { return level_quantities(s) * ((int64_t)s.nz + 1); }
constexpr int64_t actinic_means(const TallyShape &s) { return s.actinic ? (int64_t)s.nz : 0; }
constexpr int64_t side_means(const TallyShape &s) { return s.side ? 4 * (int64_t)s.nz : 0; }

// Where every part's workgroups end in its launch: the running sums of the parts' workgroup counts, in the enums' order.
struct FinishParts {
  uint32_t gatherEnd[kGatherParts], foldEnd[kFoldParts];
  constexpr uint32_t gatherGrid() const { return gatherEnd[kGatherParts - 1]; }  // the launches' grid sizes
  constexpr uint32_t foldGrid() const { return foldEnd[kFoldParts - 1]; }
  constexpr uint32_t gather(int part) const { return gatherEnd[part] - (part > 0 ? gatherEnd[part - 1] : 0); }  // a part's workgroups
  constexpr uint32_t fold(int part) const { return foldEnd[part] - (part > 0 ? foldEnd[part - 1] : 0); }
};

// nb: the batches of the launch round.  Three sizes of part: one thread per element (a bin, or a mean to fold), one workgroup per
// (batch, mean), kVolVox cells per workgroup.
inline FinishParts finish_parts(const TallyShape &s, int nb) {
  const auto threads = [](int64_t n) { return (uint32_t)((n + kFinishBlock - 1) / kFinishBlock); };
  const auto cells = [](int64_t n) { return (uint32_t)((n + kVolVox - 1) / kVolVox); };
  const auto perBatch = [nb](int64_t nMeans) { return (uint32_t)(nMeans * nb); };
  const int64_t ncol = (int64_t)s.nx * s.ny, nvox = ncol * s.nz;
  uint32_t gather[kGatherParts], fold[kFoldParts];
  gather[kGatherColumns] = threads(ncol * nb);
  gather[kGatherVolume] = cells(nvox);
  gather[kGatherReduce] = perBatch(3 + s.nz);
  gather[kGatherIntensity] = threads(ncol * s.nDir);
  gather[kGatherOrders] = threads(order_means(s) * ncol);
  gather[kGatherOrderMeans] = perBatch(order_means(s));
  gather[kGatherLevels] = threads(level_means(s) * ncol);
  gather[kGatherLevelMeans] = perBatch(level_means(s));
  gather[kGatherActinic] = s.actinic ? cells(nvox) : 0;
  gather[kGatherActinicMeans] = perBatch(actinic_means(s));
  gather[kGatherSide] = s.side ? cells(4 * nvox) : 0;
  gather[kGatherSideMeans] = perBatch(side_means(s));
  fold[kFoldColumns] = threads(3 * ncol);
  fold[kFoldScalars] = threads(3 + s.nz);
  fold[kFoldOrderMeans] = threads(order_means(s));
  fold[kFoldLevelMeans] = threads(level_means(s));
  fold[kFoldActinicMeans] = threads(actinic_means(s));
  fold[kFoldSideMeans] = threads(side_means(s));
  FinishParts p{};
  uint32_t at = 0;
  for (int i = 0; i < kGatherParts; ++i) p.gatherEnd[i] = at += gather[i];
  at = 0;
  for (int i = 0; i < kFoldParts; ++i) p.foldEnd[i] = at += fold[i];
  return p;
}

}  // namespace mcbrat
