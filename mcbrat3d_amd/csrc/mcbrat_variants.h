// mcbrat_variants.h -- which instantiations of trace_kernel and trace_block_kernel exist, and which of them a launch runs.
// Plain C++17, no HIP (like mcbrat_layout.h): the kernels assert valid() on their own flags, mcbrat_api.hip builds one table of
// kernel pointers from the lists below and asks pick_trace / pick_block on every launch, and tests/kernel_variants_dump.cpp holds the
// pickers to the recorded choice of every input (tests/golden/kernel_choice.txt) on the CPU.
//
// Adding a tally flag: a field of TraceVariant (and the template parameter it stands for), a line in valid(), a family in
// trace_variants(), a branch in pick_trace() -- DESIGN.md section 4.16.
#pragma once
#include <cstddef>
#include <tuple>

namespace mcbrat {

// One named field per template parameter of trace_kernel, in the parameters' order (mcbrat_kernels.hip).
struct TraceVariant {
  int block;    // lanes per workgroup
  bool tblLds;  // inverse phase-function tables in LDS
  int priv;     // tallies: 0 global atomics, 1 private in LDS beside a grid in global memory, 2 private with the grid in LDS too
  bool brick, debug, inten, emit;
  int spec;     // walk-specialised flux kernels: bits 0-1 the walk's spacing flags, 2-3 the component count, 4 solar with roulette
  bool ord, brdf, lvl, direct, act, side;
};
// ... and of trace_block_kernel (mcbrat_blockwalk.hip)
struct BlockVariant {
  int block;
  bool tblLds, debug, emit;
  int simple, opt;
  bool nospan;
  int rare;  // RARE: bit 0 a black surface, bit 1 the parallel sun, compiled into the exit and launch phases (0: neither)
};

constexpr auto fields(const TraceVariant &v) { return std::tie(v.block, v.tblLds, v.priv, v.brick, v.debug, v.inten, v.emit, v.spec, v.ord, v.brdf, v.lvl, v.direct, v.act, v.side); }
constexpr auto fields(const BlockVariant &v) { return std::tie(v.block, v.tblLds, v.debug, v.emit, v.simple, v.opt, v.nospan, v.rare); }

// What trace_kernel can be instantiated with.
constexpr bool valid(const TraceVariant &v) {
  const bool general = v.spec == 0 && !v.debug;  // (no tally flag is built into a walk-specialised or an instrumented kernel)
  // the component count and the roulette are fixed in the walk-specialised instantiations only
  if (v.spec != 0 && (v.spec & 3) == 0) return false;
  // scattering orders: the general dense-grid instantiations
  if (v.ord && !(general && !v.brick)) return false;
  // BRDF surfaces: the general solar instantiations
  if (v.brdf && !(general && !v.emit)) return false;
  // level fluxes: the general dense-grid flux instantiations, tallies in global memory or everything in LDS
  if (v.lvl && !(general && !v.brick && !v.inten && !v.ord && !v.brdf && v.priv != 1)) return false;
  // the direct level tally: the solar level-flux instantiations
  if (v.direct && !(v.lvl && !v.emit)) return false;
  // the actinic tally: the general dense-grid solar flux instantiations without the direct level tally
  if (v.act && !(general && !v.brick && v.priv != 1 && !v.emit && !v.inten && !v.ord && !v.brdf && !v.direct)) return false;
  // the side tally: the solar level-flux instantiations without the direct and actinic tallies
  if (v.side && !(v.lvl && !v.emit && !v.direct && !v.act)) return false;
  return true;
}
// trace_block_kernel takes every combination of its flags that is listed below.
constexpr bool valid(const BlockVariant &v) {
  return v.simple >= 0 && v.simple <= 3 && v.opt >= 0 && v.opt <= 2 && (!v.nospan || (!v.debug && !v.emit && (v.simple == 1 || v.simple == 2) && v.opt == 0)) &&
         (v.rare == 0 || (v.rare == 3 && v.nospan && v.block == 768));  // (both facts together, in the NOSPAN kernels only)
}

template <class V, int N>
struct VariantList {
  V v[N];
  int n;
  constexpr void add(const V &x) { v[n++] = x; }
};
constexpr int kTraceVariants = 272, kBlockVariants = 104;

// THE BUILT INSTANTIATIONS OF trace_kernel: this list is what is compiled.  Every family with the tables in LDS and in L2; "source":
// with the solar and the thermal-emission launch (the source kind is a template parameter: the emission launch costs the solar
// instantiations registers).  Private tallies (small domains) and bricks (large ones) never coincide; radiance runs read dense grids
// and are not instrumented.
constexpr VariantList<TraceVariant, kTraceVariants> trace_variants() {
  VariantList<TraceVariant, kTraceVariants> l{};
  for (int t = 0; t < 2; ++t) {
    const bool tbl = t != 0;
    for (int block = 256; block <= 512; block += 256) {
      for (int priv = 0; priv < 3; ++priv) {
        for (int e = 0; e < 2; ++e) {
          const bool emit = e != 0;
          // flux runs, production and instrumented: PRIV 0 / 1 / 2 and bricks x source -- 64 kernels
          for (int d = 0; d < 2; ++d) {
            l.add({block, tbl, priv, false, d != 0, false, emit, 0, false, false, false, false, false, false});
            if (priv == 0) l.add({block, tbl, 0, true, d != 0, false, emit, 0, false, false, false, false, false, false});
          }
          // radiance runs (INTEN): PRIV 0 / 1 / 2 x source -- 24 kernels
          l.add({block, tbl, priv, false, false, true, emit, 0, false, false, false, false, false, false});
          // scattering orders (ORD): PRIV 0 / 1 / 2 x INTEN x source, dense grids, not instrumented -- 48 kernels
          for (int i = 0; i < 2; ++i) l.add({block, tbl, priv, false, false, i != 0, emit, 0, true, false, false, false, false, false});
        }
        // BRDF surfaces, solar sources only, not instrumented: PRIV 0 / 1 / 2 / bricks x INTEN x ORD -- 52 kernels
        for (int i = 0; i < 2; ++i)
          for (int o = 0; o < 2; ++o) l.add({block, tbl, priv, false, false, i != 0, false, 0, o != 0, true, false, false, false, false});
        if (priv == 0) l.add({block, tbl, 0, true, false, false, false, 0, false, true, false, false, false, false});
        if (priv == 1) continue;  // the face-walk tallies: global atomics (PRIV 0) or everything in LDS (PRIV 2)
        // level fluxes (LVL): PRIV 0 / 2 x source -- 16 kernels
        for (int e = 0; e < 2; ++e) l.add({block, tbl, priv, false, false, false, e != 0, 0, false, false, true, false, false, false});
        // their DIRECT variants, solar sources only: PRIV 0 / 2 -- 8 kernels
        l.add({block, tbl, priv, false, false, false, false, 0, false, false, true, true, false, false});
        // the actinic flux (ACT), solar sources only: PRIV 0 / 2 x LVL -- 16 kernels
        for (int v = 0; v < 2; ++v) l.add({block, tbl, priv, false, false, false, false, 0, false, false, v != 0, false, true, false});
        // side fluxes (SIDE), solar sources only: PRIV 0 / 2 -- 8 kernels
        l.add({block, tbl, priv, false, false, false, false, 0, false, false, true, false, false, true});
      }
    }
    // the large flux runs: 256 lanes, dense grid in global memory, the walk's spacing flags decided at
    // compile time (SPEC 1, 2, 3: the thermal source), with the component count and the roulette too (| nc << 2 | 16: the
    // Directional solar source with roulette, one or two components) -- 18 kernels
    for (int walk = 1; walk <= 3; ++walk) {
      l.add({256, tbl, 0, false, false, false, true, walk, false, false, false, false, false, false});
      for (int nc = 1; nc <= 2; ++nc) l.add({256, tbl, 0, false, false, false, false, walk | nc << 2 | 16, false, false, false, false, false, false});
    }
    // the 768-lane kernel of the small domains (grid, tables and tallies in LDS: two workgroups of 12 waves per compute unit),
    // flux runs, source or BRDF -- 6 kernels; the wide plan's 1024 lanes (one workgroup per compute unit), PRIV 1 / 2 -- 12 kernels
    for (int block = 768; block <= 1024; block += 256)
      for (int priv = block == 768 ? 2 : 1; priv <= 2; ++priv) {
        for (int e = 0; e < 2; ++e) l.add({block, tbl, priv, false, false, false, e != 0, 0, false, false, false, false, false, false});
        l.add({block, tbl, priv, false, false, false, false, 0, false, true, false, false, false, false});
      }
  }
  return l;
}

// THE BUILT INSTANTIATIONS OF trace_block_kernel: every one with the tables in LDS and in L2.
constexpr VariantList<BlockVariant, kBlockVariants> block_variants() {
  VariantList<BlockVariant, kBlockVariants> l{};
  for (int t = 0; t < 2; ++t) {
    const bool tbl = t != 0;
    for (int e = 0; e < 2; ++e) {
      const bool emit = e != 0;
      // the shared plan: 256, 512 or 768 lanes (the option blockSize; 768 is the library's own) x SIMPLE 0, 1, 2 (x-z problems);
      // 768 lanes also SIMPLE 3 (near-uniform axes) -- 40 kernels
      for (int block = 256; block <= 768; block += 256)
        for (int simple = 0; simple <= (block == 768 ? 3 : 2); ++simple) l.add({block, tbl, false, emit, simple, 0, false, 0});
      // the wide plan: 1024 lanes x OPT 0, 1, 2 x SIMPLE 0, 1, 3 -- 36 kernels
      for (int opt = 0; opt <= 2; ++opt)
        for (int simple = 0; simple <= 3; ++simple)
          if (simple != 2) l.add({1024, tbl, false, emit, simple, opt, false, 0});
      // instrumented: 512 lanes x OPT 0, 1, 2 x SIMPLE 0, 1 (it keeps y: no x-z instantiation) -- 24 kernels
      for (int opt = 0; opt <= 2; ++opt)
        for (int simple = 0; simple <= 1; ++simple) l.add({512, tbl, true, emit, simple, opt, false, 0});
    }
    // NOSPAN (mcbrat_blockwalk.hip): the solar SIMPLE 1 and 2 kernels of 768 lanes, for media none of whose blocks spans a
    // periodic axis the kernel looks at -- 4 kernels
    for (int simple = 1; simple <= 2; ++simple) l.add({768, tbl, false, false, simple, 0, true, 0});
  }
  return l;
}
// ... and the RARE instantiations, a list of their own: the NOSPAN kernels again, with a black surface and the parallel sun compiled
// into their exit and launch phases (RARE = 3) -- 4 kernels.  The list above is the recorded one (tests/golden/kernel_choice.txt: its
// inputs are the plan and the walk's geometry, and every one of them picks RARE = 0); what picks these is the medium's surface, its
// single-scattering albedos and the source, pick_block below.
constexpr int kBlockRareVariants = 4;
constexpr VariantList<BlockVariant, kBlockRareVariants> block_rare_variants() {
  VariantList<BlockVariant, kBlockRareVariants> l{};
  for (int t = 0; t < 2; ++t)
    for (int simple = 1; simple <= 2; ++simple) l.add({768, t != 0, false, false, simple, 0, true, 3});
  return l;
}

template <class V, int N>
constexpr int find_variant(const VariantList<V, N> &l, const V &x) {
  for (int i = 0; i < l.n; ++i)
    if (fields(l.v[i]) == fields(x)) return i;
  return -1;
}

// What plan_launch (mcbrat_api.hip) decides for a launch.
struct LaunchPlan {
  bool tblLds, priv, brick, gridLds;
  bool fly;  // clear-air flight: dense grid in global memory, flux run, tables built, room in LDS
  // Wide plan (MI355X: 160 KB of LDS per compute unit): a tally slab too large to share a compute unit's LDS with a second
  // workgroup -- the broadband 20 x 20 x 20 domain's is 70 KB -- gets the compute unit to itself: ONE workgroup of 1024 lanes
  // (16 waves, 4 per SIMD) with up to the whole LDS, tallies in LDS as for the small domains instead of one memory-side
  // atomic per deposit (config 4 waited 57 % of its wave time behind them).  Flux runs only.
  bool wide;
  bool blockLite;  // wide plan, block walk without the per-cell optics in LDS (trace_block_kernel<..., OPT = 1 or 2>)
  int optics;      // block walk: where a collision finds its cell's optics: 0 per cell in LDS, 1 per cell in global memory, 2 per block in LDS
  bool cdfTop;     // block walk, thermal source: level and row sums of the emission CDF staged in LDS
  int block;
  size_t lds;
};

// What the caller has asked for (or, in a setter, would have asked for after it): read by the choice of a kernel and by refusal().
struct Settings {
  bool inten;         // intensity directions
  bool orders;        // scattering orders
  bool limitContrib;  // limitIntensityContributions
  bool levels, direct, actinic, side;  // the tallies' flags as set (direct and side count with levels only)
  bool brdf;          // a surface description with a BRDF
  bool debug;         // event counters / photon fates: the instrumented kernels
  bool emit;          // the thermal source
  // whether one batch's bins fit the tally budget: the order part, the level bins (with the direct ones), all level, actinic and side bins, the whole slab
  bool fitOrders, fitLevels, fitBins, fitStride;
};
// What the face-by-face walk of this launch looks like: read for the walk-specialised kernels only.
struct TraceWalk {
  bool rec, layerSkip, fly, surface, xyRegularWalk, zRegularWalk, useRR;  // (surface: a surface description instead of the albedo)
  int nc, solarKind;
};
// What the block walk's instantiations decide at compile time.
struct BlockWalk {
  bool xyRegular, zRegular, oneComponent, surface, xz;  // (xz: ny == 1)
  bool xyNearUniform, zNearUniform, noSimple3;
  bool spansX, spansY, spanKernel;  // a block spans the whole periodic x / y axis; the option blockSpanKernel
  int blockSize;                    // the option blockSize, 0: the library's choice
  // RARE.  blackSurface: the Lambertian albedo compares equal to 0, no surface description or BRDF is set, and every
  // single-scattering albedo handed over is finite (a NaN weight is reflected by the general kernel, albedo * NaN <= FLT_MIN being
  // false, and would be killed by BLACK).  sun: solarKind == 0.  rareKernel: the option blockRareKernel, which keeps the general phases.
  bool blackSurface, sun, rareKernel;
};

// WHAT MAY NOT BE COMBINED, and the words it is refused with.
// Level fluxes are tallied by the general flux kernels on the face-by-face walk only:
constexpr const char *kLevelsIntensityMsg = "specifyParameters: level fluxes (recLevelFluxes) cannot be combined with intensity directions: the radiance kernels have no level tallies.";
constexpr const char *kLevelsOrdersMsg = "specifyParameters: level fluxes (recLevelFluxes) cannot be combined with scattering orders (recScatOrd): no kernel tallies both.";
constexpr const char *kLevelsBrdfMsg = "specifyParameters: level fluxes (recLevelFluxes) cannot be combined with a BRDF surface: a reflected weight may exceed 1, which the level tallies do not hold.";
constexpr const char *kLevelsCountersMsg = "specifyParameters: level fluxes (recLevelFluxes) are not available together with event counters / photon fates: the instrumented kernels have no level tallies.";
constexpr const char *kLevelsBudgetMsg = "specifyParameters: level fluxes (recLevelFluxes): the level bins of one batch would not fit the 4 GiB tally budget.";
constexpr const char *kDirectNeedsLevelsMsg = "specifyParameters: direct level fluxes (recDirectLevelFluxes) need level fluxes (recLevelFluxes): they separate the downward level flux.";
constexpr const char *kDirectThermalMsg = "computeRadiativeTransfer: direct level fluxes (recDirectLevelFluxes) are not available with the thermal source: there is no direct beam.";
constexpr const char *kDirectBudgetMsg = "specifyParameters: direct level fluxes (recDirectLevelFluxes): the level bins of one batch would not fit the 4 GiB tally budget.";
// The actinic flux is tallied by solar flux kernels on the face-by-face walk only:
constexpr const char *kActinicIntensityMsg = "specifyParameters: the actinic flux (recActinicFlux) cannot be combined with intensity directions: the radiance kernels have no track-length tally.";
constexpr const char *kActinicOrdersMsg = "specifyParameters: the actinic flux (recActinicFlux) cannot be combined with scattering orders (recScatOrd): no kernel tallies both.";
constexpr const char *kActinicBrdfMsg = "specifyParameters: the actinic flux (recActinicFlux) cannot be combined with a BRDF surface: a reflected weight may exceed 1, which the track-length tally does not hold.";
constexpr const char *kActinicCountersMsg = "specifyParameters: the actinic flux (recActinicFlux) is not available together with event counters / photon fates: the instrumented kernels have no track-length tally.";
constexpr const char *kActinicDirectMsg = "specifyParameters: the actinic flux (recActinicFlux) cannot be combined with direct level fluxes (recDirectLevelFluxes): no kernel tallies both.";
constexpr const char *kActinicBudgetMsg = "specifyParameters: the actinic flux (recActinicFlux): the level and actinic bins of one batch would not fit the 4 GiB tally budget.";
constexpr const char *kActinicThermalMsg = "computeRadiativeTransfer: the actinic flux (recActinicFlux) is not available with the thermal source: the track-length tally is built for solar sources only.";
// Side fluxes are a tally of the solar level-flux kernels (and refused with everything level fluxes are
// refused with, by those messages: the setting needs them):
constexpr const char *kSideNeedsLevelsMsg = "specifyParameters: side fluxes (recSideFluxes) need level fluxes (recLevelFluxes): the kernels that stop at every face tally both.";
constexpr const char *kSideDirectMsg = "specifyParameters: side fluxes (recSideFluxes) cannot be combined with direct level fluxes (recDirectLevelFluxes): no kernel tallies both.";
constexpr const char *kSideActinicMsg = "specifyParameters: side fluxes (recSideFluxes) cannot be combined with the actinic flux (recActinicFlux): no kernel tallies both.";
constexpr const char *kSideBudgetMsg = "specifyParameters: side fluxes (recSideFluxes): the level and side bins of one batch would not fit the 4 GiB tally budget.";
constexpr const char *kSideThermalMsg = "computeRadiativeTransfer: side fluxes (recSideFluxes) are not available with the thermal source: the side tally is built for solar sources only.";
// The reference's commented redistribution (computeRadiativeTransfer :307-313) adds each direction's clipped excess to EVERY order.
constexpr const char *kOrdersLimitMsg = "specifyParameters: limitIntensityContributions cannot be combined with scattering orders (recScatOrd): the reference's redistribution adds each direction's clipped excess to every order, which would count it numRecScatOrd + 1 times.";
constexpr const char *kOrdersBudgetMsg = "specifyParameters: numRecScatOrd is too large: the tallies of one batch by scattering order would not fit the 4 GiB tally budget.";
constexpr const char *kOrdersStrideMsg = "computeRadiativeTransfer: numRecScatOrd is too large: one batch's tallies by scattering order need more than the 4 GiB tally budget.";
constexpr const char *kOrdersCountersMsg = "computeRadiativeTransfer: event counters are not available together with scattering orders.";
constexpr const char *kBrdfThermalMsg = "computeRadiativeTransfer: a BRDF surface cannot be used with the thermal source (its emissivity would be 1 - rho_dh(mu)).";
constexpr const char *kBrdfCountersMsg = "computeRadiativeTransfer: event counters / photon fates are not available together with a BRDF surface.";
constexpr const char *kFatesIntensityMsg = "trace_fates: not available together with intensity directions.";
constexpr const char *kCountersIntensityMsg = "computeRadiativeTransfer: event counters / photon fates are not available together with intensity directions.";
constexpr const char *kCountersOrdersMsg = "computeRadiativeTransfer: event counters / photon fates are not available together with scattering orders.";

// Where a refusal is asked for: a setter asking for its setting (the Settings are the context's with that one change; LevelsOff:
// level fluxes being switched off), the checks before every trace (Ready: check_ready), before a production trace (Trace) and
// before an instrumented one (Fates), and launch_trace's second line of defence (Launch: debug is the launch's, not the setting).
enum Stage : unsigned {
  SetGrid = 1, SetIntensity = 2, SetOrders = 4, SetLevels = 8, LevelsOff = 16, SetDirect = 32, SetActinic = 64, SetSide = 128, SetBrdf = 256,
  SetCounters = 512, Ready = 1024, Trace = 2048, Fates = 4096, Launch = 8192
};
// THE RULES, in the order of precedence: at a stage, the first rule of that stage that fires refuses.  (Where two call sites always
// ordered two rules differently, the rule stands twice.)
struct Rule { unsigned stages; bool (*fires)(const Settings &); const char *message; };
#define MCBRAT_RULE(stages, condition, message) {stages, [](const Settings &s) -> bool { return condition; }, message}
inline const Rule kRules[] = {
    MCBRAT_RULE(SetIntensity | SetOrders, s.limitContrib && s.orders, kOrdersLimitMsg),
    MCBRAT_RULE(Ready, s.brdf && s.emit, kBrdfThermalMsg),
    MCBRAT_RULE(Fates, s.inten, kFatesIntensityMsg),
    MCBRAT_RULE(Trace, s.orders && !s.fitStride, kOrdersStrideMsg),
    MCBRAT_RULE(Trace, s.orders && s.debug, kOrdersCountersMsg),
    MCBRAT_RULE(SetIntensity | SetLevels | Ready | Launch, s.levels && s.inten, kLevelsIntensityMsg),
    MCBRAT_RULE(SetOrders | SetLevels | Ready | Launch, s.levels && s.orders, kLevelsOrdersMsg),
    MCBRAT_RULE(SetBrdf | SetLevels | Ready | Launch, s.levels && s.brdf, kLevelsBrdfMsg),
    MCBRAT_RULE(SetCounters | SetLevels | Trace | Fates | Launch, s.levels && s.debug, kLevelsCountersMsg),
    MCBRAT_RULE(Trace, s.levels && s.side && !s.fitStride, kSideBudgetMsg),
    MCBRAT_RULE(Trace, s.levels && s.direct && !s.actinic && !s.fitStride, kDirectBudgetMsg),
    MCBRAT_RULE(Trace, s.levels && !s.actinic && !s.fitStride, kLevelsBudgetMsg),
    MCBRAT_RULE(SetLevels | SetGrid | Ready, s.levels && s.direct && !s.fitLevels, kDirectBudgetMsg),
    MCBRAT_RULE(SetLevels | SetGrid | Ready, s.levels && !s.fitLevels, kLevelsBudgetMsg),
    MCBRAT_RULE(LevelsOff | SetDirect, !s.levels && s.direct, kDirectNeedsLevelsMsg),
    MCBRAT_RULE(Ready | Launch, s.levels && s.direct && s.emit, kDirectThermalMsg),
    MCBRAT_RULE(SetIntensity | SetActinic | Ready | Launch, s.actinic && s.inten, kActinicIntensityMsg),
    MCBRAT_RULE(SetOrders | SetActinic | Ready | Launch, s.actinic && s.orders, kActinicOrdersMsg),
    MCBRAT_RULE(SetBrdf | SetActinic | Ready | Launch, s.actinic && s.brdf, kActinicBrdfMsg),
    MCBRAT_RULE(SetCounters | SetActinic | Trace | Fates | Launch, s.actinic && s.debug, kActinicCountersMsg),
    MCBRAT_RULE(SetOrders, s.orders && !s.fitOrders, kOrdersBudgetMsg),
    MCBRAT_RULE(SetDirect | SetActinic | Ready | Launch, s.actinic && s.levels && s.direct, kActinicDirectMsg),
    MCBRAT_RULE(SetDirect, s.levels && s.side && s.direct, kSideDirectMsg),
    MCBRAT_RULE(SetDirect, s.levels && s.direct && !s.fitLevels, kDirectBudgetMsg),
    MCBRAT_RULE(SetActinic, s.levels && s.side && s.actinic, kSideActinicMsg),
    MCBRAT_RULE(SetLevels | SetActinic | SetGrid | Ready, s.actinic && !s.fitBins, kActinicBudgetMsg),
    MCBRAT_RULE(Trace, s.actinic && !s.fitStride, kActinicBudgetMsg),
    MCBRAT_RULE(Ready | Launch, s.actinic && s.emit, kActinicThermalMsg),
    MCBRAT_RULE(LevelsOff | SetSide | Ready, !s.levels && s.side, kSideNeedsLevelsMsg),
    MCBRAT_RULE(SetSide | Ready | Launch, s.levels && s.side && s.direct, kSideDirectMsg),
    MCBRAT_RULE(SetSide | Ready | Launch, s.levels && s.side && s.actinic, kSideActinicMsg),
    MCBRAT_RULE(SetSide | SetGrid | Ready, s.levels && s.side && !s.fitBins, kSideBudgetMsg),
    MCBRAT_RULE(Ready | Launch, s.levels && s.side && s.emit, kSideThermalMsg),
    MCBRAT_RULE(Launch, s.brdf && s.debug, kBrdfCountersMsg),
    MCBRAT_RULE(Launch, s.inten && s.debug, kCountersIntensityMsg),
    MCBRAT_RULE(Launch, s.orders && s.debug, kCountersOrdersMsg),
};
#undef MCBRAT_RULE
inline const char *refusal(const Settings &s, Stage at) {
  for (const Rule &r : kRules)
    if ((r.stages & at) && r.fires(s)) return r.message;
  return nullptr;
}

// The trace_kernel of a launch (a plan for which the block walk does not apply; the settings have passed the refusals).
constexpr TraceVariant pick_trace(const LaunchPlan &L, const Settings &s, const TraceWalk &w) {
  TraceVariant v{256, L.tblLds, 0, false, false, false, s.emit, 0, false, false, false, false, false, false};
  const int privLds = (L.priv && L.gridLds) ? 2 : 0;
  if (L.wide && !s.debug) {  // one workgroup of 1024 lanes per compute unit, tallies (and what else fits) in its LDS; instrumented: 512 lanes
    v.block = 1024; v.priv = L.gridLds ? 2 : 1;
    v.brdf = s.brdf;
  } else if (L.block == 768 && privLds && !s.inten && !s.debug && !s.orders && !s.levels && !s.actinic) {
    // small domains (grid, tables and tallies in LDS): LDS holds two workgroups per CU, and two workgroups of 12 waves
    // (6 per SIMD, 80 VGPRs) beat two of 8 (4 per SIMD, no spills) by 10 % on the step cloud (640 and 896 lanes lose)
    // (radiance on LDS-resident domains keeps 512 lanes: 768 lanes at 80 VGPRs lose 20 % there)
    v.block = 768; v.priv = 2;
    v.brdf = s.brdf;
  } else {
    v.block = L.block >= 512 ? 512 : 256;
    if (s.actinic || s.levels) {  // the face-walk tallies (thermal source with direct, actinic or side: refused, check_ready)
      v.priv = privLds;
      v.lvl = s.levels; v.act = s.actinic; v.side = !s.actinic && s.levels && s.side; v.direct = !s.actinic && !v.side && s.levels && s.direct;
      if (v.act || v.side || v.direct) v.emit = false;
      return v;
    }
    v.priv = L.priv ? (L.gridLds ? 2 : 1) : 0;
    v.brdf = s.brdf;
    v.ord = s.orders;
    v.inten = s.inten;
    v.brick = !v.inten && !v.ord && !L.priv && L.brick;
    v.debug = !v.brdf && !v.inten && s.debug;
    if (v.block == 256 && !v.debug && !v.brdf && !v.ord && !v.inten && !L.priv && !L.brick) {
      // the large flux runs: dense grid in global memory, collision records (nc <= 2), layer-skipping walk, albedo
      // surface -- with the walk's spacing flags decided at compile time too (SPEC, mcbrat_kernels.hip)
      // A solar run with roulette (every bench workload) also has its component count and the roulette decided at compile
      // time (SPEC bits 2-3 and 4); without roulette it runs the general kernel.  (Each SPEC is built for one source: EMIT = SPEC < 16.)
      // The solar SPEC kernels launch the Directional source only: the other solar kinds run the general kernel.
      if (w.rec && w.layerSkip && w.fly && !w.surface && (w.xyRegularWalk || !w.zRegularWalk)) {
        const int walk = w.xyRegularWalk ? (w.zRegularWalk ? 2 : 3) : 1;
        v.spec = s.emit ? walk : ((w.useRR && (w.nc == 1 || w.nc == 2) && w.solarKind == 0) ? (walk | w.nc << 2 | 16) : 0);
      }
    }
  }
  if (v.brdf) v.emit = false;  // (solar sources only: a BRDF surface is refused with the thermal one, check_ready)
  return v;
}

// Radiance runs: the waves' buffers of unfinished long rays (80 B per ray) take what LDS is left at the residency the kernel is
// built for: 4 workgroups of 256 lanes per CU on grids in global memory, 2 workgroups otherwise.  packable: a ray record packs
// edge-table indices and the direction in 16 bits.  Returns the rays per wave (0: no buffers).
constexpr size_t ray_lds_base(size_t planLds) { return (planLds + 15) & ~(size_t)15; }
constexpr int ray_cap(int block, bool priv, size_t planLds, size_t ldsPerCU, bool rayDefer, bool packable) {
  const size_t waves = (size_t)block / 64, base = ray_lds_base(planLds);
  const size_t budget = ldsPerCU / (priv ? 2 : (block == 256 ? 4 : 2));
  size_t cap = (rayDefer && budget > base + 64) ? (budget - base - 64) / (waves * 80) : 0;
  if (cap > 64) cap = 64;
  return (cap < 24 || !packable) ? 0 : (int)cap;
}
constexpr size_t ray_lds(int block, size_t planLds, int cap) { return ray_lds_base(planLds) + (size_t)block / 64 * (size_t)cap * 80; }

// The trace_block_kernel of a launch the block walk applies to.
constexpr BlockVariant pick_block(const LaunchPlan &L, bool debug, bool emit, const BlockWalk &w) {
  BlockVariant v{512, L.tblLds, debug, emit, 0, 0, false, 0};
  if (L.wide) {  // one workgroup per compute unit: 1024 lanes (the instrumented instantiation: 512)
    if (!debug) v.block = 1024;
    v.opt = L.blockLite ? L.optics : 0;
  } else if (!debug) {
    const int want = w.blockSize > 0 ? w.blockSize : 768;
    v.block = (want == 768 || want == 256) ? want : 512;
  }
  // equally spaced axes, one component, no surface description: the instantiation with those decided at compile time
  const bool simple = w.xyRegular && w.zRegular && w.oneComponent && !w.surface;
  v.simple = simple ? 1 : 0;
  // no axis equally spaced by the reference's single-precision test, every axis equally spaced to 1e-6 of a cell (0.1 km cells):
  // the same cells as the general instantiation finds, with nothing left to decide at run time (SIMPLE = 3)
  if (!debug && v.block >= 768 && !w.xyRegular && !w.zRegular && w.xyNearUniform && w.zNearUniform && w.oneComponent && !w.surface && !w.noSimple3)
    v.simple = 3;
  if (simple && w.xz && !debug && v.opt == 0 && v.block != 1024) v.simple = 2;  // an x-z problem
  // NOSPAN: the 768-lane solar SIMPLE 1 and 2 kernels, where no block spans a periodic axis the kernel looks at (an x-z problem has no y)
  v.nospan = simple && v.block == 768 && !emit && !w.spanKernel && !w.spansX && (w.xz || !w.spansY);
  // RARE: built for both facts together, in the NOSPAN kernels (where the library's own plan lands with the step cloud)
  v.rare = (v.nospan && w.blackSurface && !w.surface && w.sun && !w.rareKernel) ? 3 : 0;
  return v;
}

}  // namespace mcbrat
