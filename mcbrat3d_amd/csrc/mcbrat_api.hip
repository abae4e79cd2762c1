// mcbrat_api.hip -- C ABI (include/mcbrat.h) over the gfx950 kernels.  Host plumbing only:
// device buffers, launches on one HIP stream per context, HIP-event timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mcbrat_kernels.hip"
#include "mcbrat_blockwalk.hip"
#include "mcbrat_variants.h"
#include "mcbrat_devmem.h"
#include "mcbrat_camera_ctx.h"

using namespace mcbrat;

struct mcbrat_ctx {
  int device = 0;
  // Per-launch resources.  Synchronous mode uses lane 0 only; asynchronous mode (mcbrat_set_async) rotates
  // over kLanes so that the drain of one call's tracing kernel overlaps the next call's (a launch ends
  // with its longest photon history: DESIGN.md section 5, "launch tail").
  struct LaneHandles {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the tracing kernel (synchronous mode)
    hipEvent_t evDone = nullptr;              // after the finish kernels of the lane's latest call
    ~LaneHandles() {
      if (ev0) (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
      if (evDone) (void)hipEventDestroy(evDone);
      if (stream) (void)hipStreamDestroy(stream);
    }
  };
  // Buffers are freed before streams are destroyed: a lane's handles are its base (destroyed after its members), and the lanes
  // stand in front of every buffer of the context (members go in reverse order).
  struct Lane : LaneHandles {
    DeviceBuffer<unsigned long long> dCounter;
    DeviceBuffer<long long> dSlabs;  // (sized in ELEMENTS, not batches: the stride changes with nc, nDir and the grid)
    DeviceBuffer<float> dColVals, dScalVals;
  };
  static constexpr int kLanes = 4;
  Lane lane[kLanes];
  int cur = 0, nextLane = 0;
  bool asyncOn = false;
  hipEvent_t lastDone = nullptr;   // evDone of the most recent call: the next finish chain waits for it
  hipEvent_t evExternal = nullptr; // recorded on a caller's stream by mcbrat_wait_stream
  bool externalPending = false;
  bool chainAfter = false;          // mcbrat_chain_after: this context's next finish chain follows another context's
  hipEvent_t chainSnapshot = nullptr; // ... namely what that context had enqueued when the chain was asked for: an event of THIS context,
                                    // recorded on the other's stream at that moment (no handle of the other context is kept: it may be
                                    // destroyed, or go on to other calls, before this context's next one)
  hipEvent_t evChain = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timing, eventPool;  // asynchronous mode: kernel brackets not yet read
  Lane &L() { return lane[cur]; }
  std::string err, dropText;
  int numCUs = 256;
  size_t ldsPerCU = 160 * 1024;
  // grid
  int nx = 0, ny = 0, nz = 0, nc = 0;
  bool haveGrid = false, haveOptics = false, haveSource = false;
  std::vector<double> xe, ye, ze;
  int xyRegular = 0, zRegular = 0;
  double dX = 0, dY = 0, dZ = 0;
  // device buffers
  DeviceBuffer<double> dEdges;
  DeviceBuffer<float> dExt, dCum, dSsa, dRelArea;
  DeviceBuffer<uint16_t> dPfi;
  // brick layout (see mcbrat_kernels.hip locate_cell)
  DeviceBuffer<uint32_t> dBrickTable;
  DeviceBuffer<uint32_t> dRec;  // packed collision record per cell (nc <= 2), see DevParams::rec
  DeviceBuffer<float> dLayerExt;  // [nz] extinction of a horizontally uniform layer, -1 otherwise
  DeviceBuffer<int> dLayerRun;  // [nz] runs of such layers (DevParams::layerRun)
  DeviceBuffer<double> dLayerRunT;  // [nz+1]
  // clear-air flight (DevParams::fly...)
  DeviceBuffer<float> dExtWalk, dBgVal;
  DeviceBuffer<uint16_t> dFlyRange;
  int flyNbx = 0, flyNby = 0;
  bool flyBuilt = false;
  double flyDepth = 0.0;         // vertical optical depth of the background through the layers a flight can cross
  double flightMaxDepth = 0.5;   // MCBRAT_FLIGHT_MAX_DEPTH: largest vertical optical depth of the background with which flights are used
  // block walk (mcbrat_blockwalk.hip)
  DeviceBuffer<uint32_t> dBlockRec;
  DeviceBuffer<uint16_t> dBlockOf;
  DeviceBuffer<float> dBlockExt;  // [nBlocks] extinction of each block
  DeviceBuffer<float> dBlockSsa, dBlockCum;  // [nc][nBlocks] optics per block, where uniform (blockOpticsUniform)
  DeviceBuffer<uint16_t> dBlockPfi;
  bool blockOpticsUniform = false;
  int nBlocks = 0;
  int crossThreshold = 8;      // MCBRAT_CROSS_THRESHOLD
  int batchUnits = 0;          // MCBRAT_BATCH_UNITS / option "batchUnits": 1 cuts the block walk's work units inside batches (launch_kernel)
  int jumpThreshold = 8;       // MCBRAT_JUMP_THRESHOLD
  // no record of the block decomposition has bit 0 / bit 1 of w: no block spans the whole periodic x / y axis (build_blocks)
  bool blockSpansX = true, blockSpansY = true;
  int blockSpanKernel = 0;     // option "blockSpanKernel": 1 keeps the general block-walk instantiation where NOSPAN would do (tests)
  // every single-scattering albedo handed to set_optics is finite (build_blocks walks them); with an albedo of 0, no surface
  // description and the parallel sun: the block walk's RARE instantiation (pick_block)
  bool ssaFinite = false;
  int blockRareKernel = 0;     // option "blockRareKernel": 1 keeps the general exit and launch phases where RARE would do (tests)
  bool noSimple3 = false;      // MCBRAT_NO_SIMPLE3 (tests): the block walk's near-uniform grids run the general kernel, not SIMPLE = 3
  DeviceBuffer<float> dExtB, dCumB, dSsaB, dBgExt, dBgCum, dBgSsa;
  DeviceBuffer<uint16_t> dPfiB, dBgPfi;
  int nbx = 0, nby = 0, nbz = 0;
  long long nStored = 0;
  double backgroundFraction = 0.0;  // share of bricks that are pure background
  bool bricksBuilt = false;
  int brickMode = 2;               // 0 dense, 1 bricks, 2 automatic
  DeviceBuffer<float> dTables;
  // surface description (specifyParameters(surfaceBDRF=)); surfNumX == 0: the domain's albedo
  int surfNumX = 0, surfNumY = 0;
  DeviceBuffer<double> dSurfX, dSurfY;
  DeviceBuffer<float> dSurfRefl;
  int surfKind = 0;                // mcbrat_set_surface_brdf: 0 Lambertian (dSurfRefl), 1 RPV, 2 Ross-Li, 3 Cox-Munk (dSurfBrdf)
  bool glintSampling = true;       // option "glintSampling": a Cox-Munk reflection draws from the glint mixture (brdf_sample)
  DeviceBuffer<float4> dSurfBrdf;  // [numY-1][numX-1] the patches' parameters, padded to four
  DeviceBuffer<double> dVoxelCDF;
  DeviceBuffer<unsigned long long> dEventCounters;
  DeviceBuffer<float> dLast;
  DeviceBuffer<double> dMomentsOwned;
  double *dMoments = nullptr;  // not owned: dMomentsOwned, or the caller's buffer (mcbrat_bind_moments)
  // tables (host, per component)
  std::vector<std::vector<float>> tables;
  std::vector<int> tblNSteps, tblNEntries;
  std::vector<int> maxPfi;  // largest 0-based entry referenced per component
  bool tablesDirty = true;
  int tblTotalFloats = 0;
  int tblOffset[MCBRAT_MAX_COMPONENTS] = {0};
  // radiance by local estimation
  int nDir = 0;
  std::vector<float> dirData;  // [nDir][8], see DevParams
  DeviceBuffer<float> dDirData, dFwd, dFwdOrig;
  std::vector<std::vector<float>> fwd, fwdOrig;  // per component [nEntries][nAngles]
  std::vector<int> fwdNAngles, fwdNEntries;
  int fwdOffset[MCBRAT_MAX_COMPONENTS] = {0};
  bool fwdDirty = true;
  int useHybrid = 0, numOrdersOrig = 0, useRRIntensity = 0, limitContrib = 0;
  float zetaMin = 0.3f, maxContrib = FLT_MAX;
  // fluxes and radiances by scattering order (mcbrat_specify_scattering_orders): highest order recorded, -1 off
  int numRecScatOrd = -1;
  // upward and downward flux through every level of every column (mcbrat_specify_level_fluxes)
  int levelFluxes = 0;
  // the direct beam apart from the diffuse light in the downward level flux (mcbrat_specify_direct_level_fluxes)
  int directLevelFluxes = 0;
  // the actinic flux of every cell by track length (mcbrat_specify_actinic_flux)
  int actinicFlux = 0;
  // the flux through the vertical faces of every cell (mcbrat_specify_side_fluxes); needs levelFluxes
  int sideFluxes = 0;
  // parameters
  float albedo = 0.f;
  int useRR = 1;
  float lwFlag = -1.f;
  int srcKind = 0;
  int solarKind = 0;            // srcKind 0: 0 Directional, 1 RandomAzimuth, 2 Flux, 3 Spotlight
  double spotX = 0, spotY = 0;  // spotlight: launch point as fractions of the domain
  float dir0[3] = {0, 0, -1};
  double zLaunch = 0;
  int izLaunch = 0;
  double fracAtms = 0;
  // tuning / measurement
  int blocksPerCU = 0;  // 0: from the occupancy query
  int eventThreshold = 16;     // measured optimum 16 (step cloud) .. 32 (128x128x64); see DESIGN.md
  int launchThreshold = 8, surfaceThreshold = 12;  // (exits -- top and surface -- queue together: 12-16 measured best)
  bool surfaceThresholdSet = false;  // by the caller: the block walk otherwise uses its own measured default
  bool launchThresholdSet = false;   // by the caller: the thermal source otherwise launches 32 lanes at a time (below)
  bool autoTune = true;        // pick eventThreshold by timing short trial launches (once per domain/source)
  bool tuned = false;
  int maxBatchesInFlight = 0;  // 0: bounded by memory
  int privMode = 1;            // 1: LDS-private tallies when the slab fits, 0: always global atomics
  int wideDefault = 1;         // MCBRAT_WIDE
  int wideMode = 1;            // 1: a tally slab too large for the shared plan may take a compute unit's whole LDS (one workgroup of 1024 lanes per CU;
                               //    MCBRAT_WIDE=0 / set_tuning(privateTallies = 3) turn it off: such domains then tally with global atomics)
  int blockSize = 0;           // 0: chosen by plan_launch
  unsigned long long tuneTrialPhotons = 1ull << 26;  // MCBRAT_TUNE_PHOTONS
  int regularWalk = 1;         // equally spaced grids: incremental face distances (MCBRAT_REGULAR_WALK=0 turns it off)
  int gridLdsMode = 1;         // stage the optical grid in LDS when it fits (private-tally mode)
  int rayShort = 0, rayPassIters = 0, rayPassAt = 0;  // 0: chosen in launch_trace (MCBRAT_RAY_SHORT, MCBRAT_RAY_PASS_ITERS, MCBRAT_RAY_PASS_AT)
  int rayDefer = 1;            // radiance: long rays are put aside and finished in dense passes (MCBRAT_RAY_DEFER=0: inside their event phase)
  int blockWalk = 1;           // LDS-resident grids: blocks of cells with one extinction value are crossed in one step (MCBRAT_BLOCK_WALK=0 / mcbrat_set_walk_options)
  int layerSkip = 1;           // layers of one extinction value: cross z faces only; clear-air flight outside the brick columns' cloud
                               // ranges (MCBRAT_LAYER_SKIP / mcbrat_set_walk_options: 0 off, 1 both, 2 the layers only)
  // loop bounds of the kernels (DevParams::bad ...) and the count of what they dropped
  DeviceBuffer<unsigned long long> dBad;  // device: photons / rays dropped since the context was created
  PinnedBuffer<unsigned long long> hBad;  // pinned host copy, written by the last finish kernel of every call (hBadDev: the same word as the device sees it)
  unsigned long long *hBadDev = nullptr;
  unsigned maxEvents = 1u << 24, maxEventsNaN = 1u << 20, watchdog = 1u << 20;  // MCBRAT_MAX_EVENTS, MCBRAT_MAX_EVENTS_NAN, MCBRAT_WATCHDOG
  int legacyTies = 0;
  float testRayMaxLen = 0.0f;  // TEST ONLY (MCBRAT_TEST_RAY_MAX_LEN, km): replaces the geometric bound on a view ray's length                   // MCBRAT_TEST_LEGACY_TIES (tests only)
  // mcbrat_frequency_distribution's device buffers, kept and grown with numLambda
  DeviceBuffer<double> dFreqCdf;
  DeviceBuffer<unsigned long long> dFreqCounts;
  int cameraGridInLds = -1;  // option "cameraGridInLds": where mcbrat_sun_transmittance reads the grid (-1: LDS where it fits)
  int cameraPathBinsInLds = 1;  // option "cameraPathBinsInLds": 0, a path-length render deposits straight to global memory
  bool countersOn = false;
  float lastTraceMs = 0.f;
  mcbrat_counters lastCounters{};
  bool haveLast = false;
  ~mcbrat_ctx() {
    for (auto &pr : eventPool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (evExternal) (void)hipEventDestroy(evExternal);
    if (evChain) (void)hipEventDestroy(evChain);
  }
};

// The seam of mcbrat_devmem.h: every allocation of the library, and every free, goes through these four.
namespace mcbrat {

static std::atomic<long long> liveDeviceAllocations{0};  // mcbrat_live_device_allocations

// -DMCBRAT_POISON (audit build): fresh memory is filled with 0xff, so that a kernel that reads what nothing wrote reads
// NaNs / huge indices instead of whatever an earlier context left there.
int device_alloc(void **ptr, size_t bytes) {
  hipError_t e = hipMalloc(ptr, bytes);
#ifdef MCBRAT_POISON
  if (e == hipSuccess) e = hipMemset(*ptr, 0xff, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess && *ptr) (void)hipFree(*ptr);
#endif
  if (e == hipSuccess) ++liveDeviceAllocations;
  else *ptr = nullptr;
  return (int)e;
}
void device_free(void *ptr) {
  (void)hipFree(ptr);
  --liveDeviceAllocations;
}
int pinned_alloc(void **ptr, size_t bytes) {
  const hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocMapped);
  if (e != hipSuccess) *ptr = nullptr;
  return (int)e;
}
void pinned_free(void *ptr) { (void)hipHostFree(ptr); }

}  // namespace mcbrat

namespace {

int fail(mcbrat_ctx *c, const std::string &msg) {
  if (c) c->err = msg;
  return 1;
}
// (call: a hipError_t, or the int an owner of mcbrat_devmem.h hands back for one)
#define HIP_OK(c, call)                                                                                   \
  do {                                                                                                    \
    const hipError_t e_ = static_cast<hipError_t>(call);                                                  \
    if (e_ != hipSuccess) return fail(c, std::string(#call) + ": " + hipGetErrorString(e_));              \
  } while (0)

int init_lane(mcbrat_ctx *c, int i) {
  mcbrat_ctx::Lane &L = c->lane[i];
  if (L.stream) return 0;
  HIP_OK(c, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  HIP_OK(c, hipEventCreate(&L.ev0));
  HIP_OK(c, hipEventCreate(&L.ev1));
  HIP_OK(c, hipEventCreateWithFlags(&L.evDone, hipEventDisableTiming));
  HIP_OK(c, L.dCounter.allocate(1));
  return 0;
}

// Waits for everything the context has enqueued and reads the kernel brackets of asynchronous calls.
int sync_all(mcbrat_ctx *c) {
  for (int i = 0; i < mcbrat_ctx::kLanes; ++i)
    if (c->lane[i].stream) HIP_OK(c, hipStreamSynchronize(c->lane[i].stream));
  if (!c->timing.empty()) {
    float total = 0.f;
    for (auto &pr : c->timing) {
      float ms = 0.f;
      HIP_OK(c, hipEventElapsedTime(&ms, pr.first, pr.second));
      total += ms;
      c->eventPool.push_back(pr);
    }
    c->timing.clear();
    c->lastTraceMs = total;
  }
  if (c->hBad) c->lastCounters.badPhotons = (int64_t)*c->hBad.get();
  return 0;
}

int event_pair(mcbrat_ctx *c, std::pair<hipEvent_t, hipEvent_t> &pr) {
  if (!c->eventPool.empty()) { pr = c->eventPool.back(); c->eventPool.pop_back(); return 0; }
  HIP_OK(c, hipEventCreate(&pr.first));
  HIP_OK(c, hipEventCreate(&pr.second));
  return 0;
}

double spacing_d(double x) {
  if (x == 0.0) return DBL_MIN;
  int e;
  std::frexp(std::fabs(x), &e);
  const double s = std::ldexp(1.0, e - 53);
  return s < DBL_MIN ? DBL_MIN : s;
}

template <typename T>
int upload(mcbrat_ctx *c, DeviceBuffer<T> *dst, const T *src, size_t n) {
  HIP_OK(c, dst->allocate(std::max<size_t>(n, 1)));
  if (n) HIP_OK(c, hipMemcpy(dst->get(), src, sizeof(T) * n, hipMemcpyHostToDevice));
  return 0;
}

bool orders_on(const mcbrat_ctx *c) { return c->numRecScatOrd >= 0; }

bool levels_on(const mcbrat_ctx *c) { return c->levelFluxes != 0; }
bool direct_on(const mcbrat_ctx *c) { return c->levelFluxes != 0 && c->directLevelFluxes != 0; }
// the actinic flux of every cell
bool actinic_on(const mcbrat_ctx *c) { return c->actinicFlux != 0; }
// the tallies that make every cell face a stop: the plan then walks face by face (no layer skipping, flight, block walk, wide
// plan, bricks or 768-lane kernel), and their bins stay in global memory
bool facewalk_on(const mcbrat_ctx *c) { return levels_on(c) || actinic_on(c); }
// the flux through the vertical faces of every cell: a tally of the level-flux kernels, on their walk
bool side_on(const mcbrat_ctx *c) { return c->levelFluxes != 0 && c->sideFluxes != 0; }

// Where every tally lies -- in one batch's slab, in the moments and the last batch's results, in the finish kernels' scalar
// scratch -- is defined by mcbrat_layout.h; nothing here derives an offset of its own.
int32_t order_count(int32_t numRecScatOrd) { return numRecScatOrd < 0 ? 0 : (numRecScatOrd < INT32_MAX ? numRecScatOrd + 1 : INT32_MAX); }
TallyShape tally_shape(const mcbrat_ctx *c) {
  return TallyShape{c->nx, c->ny, c->nz, c->nc, c->nDir, c->limitContrib, order_count(c->numRecScatOrd), levels_on(c), direct_on(c), actinic_on(c), side_on(c)};
}
TallyLayout tally_layout(const mcbrat_ctx *c) { return tally_layout(tally_shape(c)); }
constexpr size_t kSlabBudget = (size_t)4 << 30;  // bytes of batch slabs in flight at most (one batch's slab must fit it)
// whether the bins of one batch of a (candidate) shape fit that budget: its order part, its level and actinic bins, all of it
TallyFit budget_fit(const TallyShape &s) { return tally_fit(s, kSlabBudget); }
// What a call asks refusal() (mcbrat_variants.h) about: the context's settings -- a setter first changes the one field it is about
struct Asked { int nx, ny, nz, nDir, limitContrib, numRecScatOrd, levels, direct, actinic, side; bool brdf, debug; };
Asked asked(const mcbrat_ctx *c) {
  return Asked{c->nx, c->ny, c->nz, c->nDir, c->limitContrib, c->numRecScatOrd, c->levelFluxes, c->directLevelFluxes, c->actinicFlux, c->sideFluxes,
               c->surfNumX > 0 && c->surfKind != 0, c->countersOn};
}
Settings settings_of(const mcbrat_ctx *c, const Asked &a) {
  const TallyShape s{a.nx, a.ny, a.nz, c->nc, a.nDir, a.limitContrib, order_count(a.numRecScatOrd), a.levels != 0, a.levels && a.direct, a.actinic != 0, a.levels && a.side};
  TallyShape l = s;  // (without the actinic flux and the side fluxes a refusal is the level tallies')
  l.actinic = l.side = 0;
  const TallyFit all = budget_fit(s), levels = budget_fit(l);
  return Settings{a.nDir > 0, a.numRecScatOrd >= 0, a.limitContrib != 0, a.levels != 0, a.direct != 0, a.actinic != 0, a.side != 0, a.brdf, a.debug, c->srcKind != 0,
                  all.orders, levels.globalBins, all.globalBins, all.stride};
}
// (a refused call leaves the context as it was, but for its error text)
#define REFUSE(c, a, stage) \
  do { if (const char *m_ = refusal(settings_of(c, a), stage)) return fail(c, m_); } while (0)
constexpr int64_t kMaxPhotonsPerBatch = 0x7fffffffLL;  // a unit weight per photon in one bin stays below 2^63 (2^-32 units)
// The fixed point of an actinic deposit: 2^e km, e the smallest integer that keeps the longest possible step of the walk below
// 2^e -- the diagonal of the largest spacings of the three axes, times 1 + 2^-10 for the float rounding of tmin - tcur (a few
// ulp of the distance along the leg, which may be many steps long).  The kernel deposits w l 2^-e, the epilogue multiplies
// 2^e back in double: a power of two, so the scaling itself is exact.  Chosen once per grid.
double actinic_unit(const mcbrat_ctx *c) {
  const auto widest = [](const std::vector<double> &e) {
    double m = 0.0;
    for (size_t i = 0; i + 1 < e.size(); ++i) m = std::max(m, e[i + 1] - e[i]);
    return m;
  };
  const double wx = widest(c->xe), wy = widest(c->ye), wz = widest(c->ze);
  const double longest = std::sqrt(wx * wx + wy * wy + wz * wz) * (1.0 + 1.0 / 1024.0);
  int e = 0;
  (void)std::frexp(longest, &e);  // longest = m 2^e with m in [0.5, 1)
  return std::ldexp(1.0, e);
}
// The last batch's results from element `base` on (they are laid out as one sum of the moments), once everything enqueued is done
int read_last(mcbrat_ctx *c, size_t base, std::vector<float> &h) {
  if (!c->haveLast) return fail(c, "reportResults: no batch has been traced yet.");
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  HIP_OK(c, hipMemcpy(h.data(), c->dLast.get() + base, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
  return 0;
}
// ... dealt out to the caller's arrays in the order the parts lie in, already in Fortran order (a null array is skipped)
using LastPart = std::pair<float *, size_t>;
int deal_last(mcbrat_ctx *c, size_t base, std::initializer_list<LastPart> parts) {
  size_t n = 0;
  for (const LastPart &p : parts) n += p.second;
  std::vector<float> h(n);
  if (read_last(c, base, h)) return 1;
  const float *q = h.data();
  for (const LastPart &p : parts) { if (p.first) std::memcpy(p.first, q, sizeof(float) * p.second); q += p.second; }
  return 0;
}

// A setting changed the length of the moments: the moment arrays and the last batch's results (both laid out by the old length)
// go, to be made afresh by the next call.  retune: the setting also changes the walk or the kernels, so the event threshold is
// chosen again.
void drop_results(mcbrat_ctx *c, bool retune) {
  c->dMomentsOwned.reset();
  c->dMoments = nullptr;
  c->dLast.reset();
  c->haveLast = false;
  if (retune) c->tuned = false;
}

int ensure_moments(mcbrat_ctx *c) {
  if (c->dMoments) return 0;
  const size_t n = 8 + 2 * (size_t)tally_layout(c).momentsLen;
  HIP_OK(c, c->dMomentsOwned.allocate(n));
  // (on the stream the finish kernels run on: hipMemset on the null stream is asynchronous for device memory and the
  // context's streams are non-blocking, so nothing would order a null-stream memset before the first finish kernels)
  if (init_lane(c, c->cur)) return 1;
  HIP_OK(c, hipMemsetAsync(c->dMomentsOwned.get(), 0, sizeof(double) * n, c->L().stream));
  HIP_OK(c, hipStreamSynchronize(c->L().stream));
  c->dMoments = c->dMomentsOwned.get();
  return 0;
}

int sync_tables(mcbrat_ctx *c) {
  if (!c->tablesDirty) return 0;
  if (sync_all(c)) return 1;
  std::vector<float> all;
  for (int k = 0; k < c->nc; ++k) {
    if ((int)c->tables.size() <= k || c->tables[k].empty())
      return fail(c, "computeRadiativeTransfer: no inverse phase function table for component " + std::to_string(k + 1));
    if (c->maxPfi[k] >= c->tblNEntries[k])
      return fail(c, "computeRadiativeTransfer: phaseFunctionIndex exceeds table entries for component " + std::to_string(k + 1));
    c->tblOffset[k] = (int)all.size();
    all.insert(all.end(), c->tables[k].begin(), c->tables[k].end());
  }
  c->tblTotalFloats = (int)all.size();
  if (upload(c, &c->dTables, all.data(), all.size())) return 1;
  c->tablesDirty = false;
  return 0;
}

// forward tables for radiance, uploaded before the first launch that needs them
int sync_forward_tables(mcbrat_ctx *c) {
  if (c->nDir == 0 || !c->fwdDirty) return 0;
  if (sync_all(c)) return 1;
  std::vector<float> all, allOrig;
  for (int k = 0; k < c->nc; ++k) {
    if ((int)c->fwd.size() <= k || c->fwd[k].empty())
      return fail(c, "tabulateForwardPhaseFunctions: no forward phase function table for component " + std::to_string(k + 1));
    if (c->maxPfi[k] >= c->fwdNEntries[k])
      return fail(c, "tabulateForwardPhaseFunctions: phaseFunctionIndex exceeds table entries for component " + std::to_string(k + 1));
    c->fwdOffset[k] = (int)all.size();
    all.insert(all.end(), c->fwd[k].begin(), c->fwd[k].end());
    allOrig.insert(allOrig.end(), c->fwdOrig[k].begin(), c->fwdOrig[k].end());
  }
  if (upload(c, &c->dFwd, all.data(), all.size()) || upload(c, &c->dFwdOrig, allOrig.data(), allOrig.size())) return 1;
  if (upload(c, &c->dDirData, c->dirData.data(), c->dirData.size())) return 1;
  c->fwdDirty = false;
  return 0;
}

// Brick layout of the optical grids: 4x4x4 bricks; a brick is "background" when each of its cells
// carries exactly its layer's most common record (extinction + every component's cumExt/ssa/phase
// index).  Background bricks are not stored.  Lossless: the kernel reads the same floats either way.
int build_bricks(mcbrat_ctx *c, const std::vector<float> &e, const std::vector<float> &cu, const std::vector<float> &s,
                 const std::vector<uint16_t> &pf, int nc) {
  const int nx = c->nx, ny = c->ny, nz = c->nz;
  const size_t ncol = (size_t)nx * ny, nvox = ncol * nz;
  std::vector<float> bgExt(nz), bgCum((size_t)nc * nz), bgSsa((size_t)nc * nz), layerExt(nz);
  std::vector<uint16_t> bgPfi((size_t)nc * nz);
  // the layers' background extinction, the brick columns' cloud ranges, the walk's marked copy of the extinction and the
  // vertical optical depth of the background (layer-skipping walk, clear-air flight): mcbrat_flight_tables, mcbrat_host.cpp
  const bool bricks4 = nx % 4 == 0 && ny % 4 == 0 && nz >= 2 && nz <= 255;
  std::vector<uint16_t> range(bricks4 ? (size_t)(nx / 4) * (ny / 4) : 0);
  std::vector<float> walk(bricks4 ? nvox : 0);
  std::vector<double> runT(nz + 1, 0.0);
  int32_t flights = 0;
  if (mcbrat_flight_tables(nx, ny, nz, e.data(), c->ze.data(), bgExt.data(), bricks4 ? range.data() : nullptr,
                           bricks4 ? walk.data() : nullptr, runT.data(), &flights))
    return fail(c, "getOpticalPropertiesByComponent: could not build the tables of the walk.");
  for (int k = 0; k < nz; ++k) {
    const float best = bgExt[k];
    bool uniform = true;
    for (size_t v = ncol * k; v < ncol * (k + 1) && uniform; ++v) uniform = e[v] == best;
    layerExt[k] = uniform ? best : -1.0f;  // a layer of one extinction value needs no gather in the walk
    size_t rep = ncol * k;
    while (e[rep] != best) ++rep;  // a representative background cell of this layer
    for (int q = 0; q < nc; ++q) {
      bgCum[(size_t)q * nz + k] = cu[(size_t)q * nvox + rep];
      bgSsa[(size_t)q * nz + k] = s[(size_t)q * nvox + rep];
      bgPfi[(size_t)q * nz + k] = pf[(size_t)q * nvox + rep];
    }
  }
  if (upload(c, &c->dLayerExt, layerExt.data(), layerExt.size())) return 1;
  c->flyBuilt = false;
  c->flyNbx = c->flyNby = 0;
  if (bricks4) {
    if (upload(c, &c->dFlyRange, range.data(), range.size()) || upload(c, &c->dExtWalk, walk.data(), walk.size()) ||
        upload(c, &c->dBgVal, bgExt.data(), bgExt.size()))
      return 1;
    c->flyNbx = nx / 4; c->flyNby = ny / 4;
    // A flight is only granted to a lane the background cannot stop before the domain boundary.  In a haze (vertical
    // optical depth of the background not small against 1) most requests are refused, and asking costs a turn in the
    // queue: measured -10 % on the 128x128x64 field in a haze of optical depth 2.3; Rayleigh air (0.02) is what the
    // flight is for.  In between (same field, 5 / 10 / 20 / 40 times the Rayleigh extinction = 0.12 / 0.23 / 0.46 / 0.92):
    // +13 / +8 / +2 / -5 %, so the limit is 0.5 (flight_wanted).
    c->flyBuilt = flights != 0;
    c->flyDepth = runT[nz];
  }
  {
    // runs of consecutive one-extinction layers (layer-skipping walk): for layer k the face where its run ends
    // upwards / downwards.  (runT: inside a run of one-extinction layers its differences are the run's own; a layer no
    // flight can cross adds nothing to it -- differences across such a layer are only used as the bound on what the
    // background can take from a lane before its flight ends.)
    std::vector<int> run(nz, 0);
    for (int k = 0; k < nz; ++k) {
      int up = k + 1, down = k;
      while (up < nz && layerExt[up] >= 0.f) ++up;
      while (down > 0 && layerExt[down - 1] >= 0.f) --down;
      run[k] = (up << 16) | down;
    }
    if (upload(c, &c->dLayerRun, run.data(), run.size()) || upload(c, &c->dLayerRunT, runT.data(), runT.size())) return 1;
  }
  auto isBackground = [&](size_t v, int k) {
    if (e[v] != bgExt[k]) return false;
    for (int q = 0; q < nc; ++q)
      if (cu[(size_t)q * nvox + v] != bgCum[(size_t)q * nz + k] || s[(size_t)q * nvox + v] != bgSsa[(size_t)q * nz + k] ||
          pf[(size_t)q * nvox + v] != bgPfi[(size_t)q * nz + k])
        return false;
    return true;
  };
  const int nbx = (nx + 3) / 4, nby = (ny + 3) / 4, nbz = (nz + 3) / 4;
  std::vector<uint32_t> table((size_t)nbx * nby * nbz, 0xffffffffu);
  size_t stored = 0;
  for (int bz = 0; bz < nbz; ++bz)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) {
        bool bg = true;
        for (int k = bz * 4; k < std::min(nz, bz * 4 + 4) && bg; ++k)
          for (int j = by * 4; j < std::min(ny, by * 4 + 4) && bg; ++j)
            for (int i = bx * 4; i < std::min(nx, bx * 4 + 4) && bg; ++i)
              bg = isBackground((size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * k), k);
        if (!bg) table[(size_t)bx + (size_t)nbx * ((size_t)by + (size_t)nby * bz)] = (uint32_t)(64 * stored++);
      }
  const size_t nS = std::max<size_t>(64 * stored, 64);
  std::vector<float> eB(nS, 0.f), cuB(nS * nc, 0.f), sB(nS * nc, 0.f);
  std::vector<uint16_t> pfB(nS * nc, 0);
  for (int bz = 0; bz < nbz; ++bz)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) {
        const uint32_t base = table[(size_t)bx + (size_t)nbx * ((size_t)by + (size_t)nby * bz)];
        if (base == 0xffffffffu) continue;
        for (int lk = 0; lk < 4; ++lk)
          for (int lj = 0; lj < 4; ++lj)
            for (int li = 0; li < 4; ++li) {
              const int i = bx * 4 + li, j = by * 4 + lj, k = bz * 4 + lk;
              if (i >= nx || j >= ny || k >= nz) continue;
              const size_t v = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * k), o = base + li + 4 * (lj + 4 * lk);
              eB[o] = e[v];
              for (int q = 0; q < nc; ++q) {
                cuB[(size_t)q * nS + o] = cu[(size_t)q * nvox + v];
                sB[(size_t)q * nS + o] = s[(size_t)q * nvox + v];
                pfB[(size_t)q * nS + o] = pf[(size_t)q * nvox + v];
              }
            }
      }
  c->nbx = nbx; c->nby = nby; c->nbz = nbz;
  c->nStored = (long long)nS;
  c->backgroundFraction = 1.0 - (double)stored / (double)table.size();
  if (upload(c, &c->dBrickTable, table.data(), table.size()) || upload(c, &c->dExtB, eB.data(), eB.size()) ||
      upload(c, &c->dCumB, cuB.data(), cuB.size()) || upload(c, &c->dSsaB, sB.data(), sB.size()) ||
      upload(c, &c->dPfiB, pfB.data(), pfB.size()) || upload(c, &c->dBgExt, bgExt.data(), bgExt.size()) ||
      upload(c, &c->dBgCum, bgCum.data(), bgCum.size()) || upload(c, &c->dBgSsa, bgSsa.data(), bgSsa.size()) ||
      upload(c, &c->dBgPfi, bgPfi.data(), bgPfi.size()))
    return 1;
  c->bricksBuilt = true;
  return 0;
}

// Block walk (mcbrat_blockwalk.hip): the grid cut into axis-aligned blocks of cells that carry one extinction value
// (mcbrat_block_decomposition, mcbrat_host.cpp), uploaded for the kernel.
int build_blocks(mcbrat_ctx *c, const std::vector<float> &e, const std::vector<float> &cu, const std::vector<float> &ssa,
                 const std::vector<uint16_t> &pf, int nc, const double *ssaGiven) {
  const int nx = c->nx, ny = c->ny, nz = c->nz;
  const size_t nvox = (size_t)nx * ny * nz;
  c->nBlocks = 0;
  // RARE (mcbrat_variants.h): no weight can become a NaN.  Read from the array as it was handed over, vacuum cells included (the
  // upload stores 0 there, and set_optics has refused a NaN where there is extinction): one NaN anywhere keeps the general kernel.
  c->ssaFinite = true;
  for (size_t i = 0; i < nvox * (size_t)nc && c->ssaFinite; ++i) c->ssaFinite = std::isfinite(ssaGiven[i]) && std::isfinite(ssa[i]);
  c->dBlockRec.reset(); c->dBlockOf.reset(); c->dBlockExt.reset();
  c->dBlockSsa.reset(); c->dBlockCum.reset(); c->dBlockPfi.reset();
  c->blockOpticsUniform = false;
  c->blockSpansX = c->blockSpansY = true;
  // only grids that can live in LDS are walked this way (plan_launch decides); bounds are packed in 16 bits
  if (nvox > 65536 || nx > 65535 || ny > 65535 || nz > 65535) return 0;
  std::vector<uint16_t> of(nvox);
  std::vector<uint32_t> rec(4 * nvox);
  int32_t nb = 0;
  if (mcbrat_block_decomposition(nx, ny, nz, e.data(), of.data(), rec.data(), &nb) != 0) return 0;  // (more than 65535 blocks: face-by-face walk)
  std::vector<float> blockExt((size_t)nb, 0.0f);
  for (size_t v = 0; v < nvox; ++v) blockExt[of[v]] = e[v];  // (one value per block by construction)
  if (upload(c, &c->dBlockRec, rec.data(), (size_t)4 * nb) || upload(c, &c->dBlockOf, of.data(), of.size()) ||
      upload(c, &c->dBlockExt, blockExt.data(), blockExt.size())) return 1;
  // Blocks are cut by extinction; where every block is uniform in the other optics too (a homogeneous medium, slabs: the
  // broadband and I3RC test domains) a collision needs no per-cell record at all -- optics per block, in LDS
  std::vector<float> bSsa((size_t)nc * nb), bCum((size_t)nc * nb);
  std::vector<uint16_t> bPfi((size_t)nc * nb);
  std::vector<char> seen((size_t)nb, 0);
  bool uniform = true;
  for (size_t v = 0; v < nvox && uniform; ++v) {
    const size_t b = of[v];
    for (int k = 0; k < nc && uniform; ++k) {
      const size_t i = (size_t)k * nvox + v, j = (size_t)k * nb + b;
      if (!seen[b]) { bSsa[j] = ssa[i]; bCum[j] = cu[i]; bPfi[j] = pf[i]; }
      else uniform = std::memcmp(&bSsa[j], &ssa[i], 4) == 0 && std::memcmp(&bCum[j], &cu[i], 4) == 0 && bPfi[j] == pf[i];
    }
    seen[b] = 1;
  }
  if (uniform) {
    if (upload(c, &c->dBlockSsa, bSsa.data(), bSsa.size()) || upload(c, &c->dBlockCum, bCum.data(), bCum.size()) ||
        upload(c, &c->dBlockPfi, bPfi.data(), bPfi.size())) return 1;
    c->blockOpticsUniform = true;
  }
  bool sx = false, sy = false;  // (mcbrat_block_decomposition sets bit 0 / 1 of w where a block covers the whole x / y axis)
  for (int32_t b = 0; b < nb; ++b) { sx = sx || (rec[4 * (size_t)b + 3] & 1u); sy = sy || (rec[4 * (size_t)b + 3] & 2u); }
  c->blockSpansX = sx; c->blockSpansY = sy;
  c->nBlocks = nb;
  return 0;
}

// Bricks are for grids that no longer fit the cache hierarchy (32 MiB of L2 + 256 MiB Infinity
// Cache) and are mostly background.  Measured on MI355X: at 128x128x64 (4 MiB of extinction) the
// dense grid is as fast or 1-3 % faster, so the automatic rule only switches
// for grids of 64 MiB and more.
bool use_bricks(const mcbrat_ctx *c) {
  if (!c->bricksBuilt || c->brickMode == 0 || c->nDir > 0 || orders_on(c) || facewalk_on(c)) return false;  // (radiance rays read the dense grid; no ORD, LVL or ACT kernel reads bricks)
  if (c->brickMode == 1) return true;
  const size_t nvox = (size_t)c->nx * c->ny * c->nz;
  // automatic: the dense layout is the faster one wherever measured (128x128x64: equal; 512x512x128: 83 vs 105 ms per
  // 2e7 photons), so bricks are a memory saver for the very largest grids only (dense optics: 24 B per cell and component)
  return nvox * sizeof(float) >= ((size_t)2 << 30) && c->backgroundFraction >= 0.5;
}

void fill_params(mcbrat_ctx *c, DevParams &p) {
  std::memset(&p, 0, sizeof(p));
  p.nx = c->nx; p.ny = c->ny; p.nz = c->nz; p.nc = c->nc;
  p.xyRegular = c->xyRegular; p.zRegular = c->zRegular;
  p.x0 = c->xe.front(); p.xMax = c->xe.back();
  p.y0 = c->ye.front(); p.yMax = c->ye.back();
  p.z0 = c->ze.front(); p.zMax = c->ze.back();
  p.Lx = p.xMax - p.x0; p.Ly = p.yMax - p.y0;
  p.zSurf = p.z0 + spacing_d(p.z0);
  p.invDX = c->xyRegular ? 1.0 / c->dX : 0.0;
  p.invDY = c->xyRegular ? 1.0 / c->dY : 0.0;
  // (only where the reference itself calls the axis regular -- its test uses a float spacing, new_Integrator
  // :163-181.  Float steps accumulate rounding over a leg: on 0.03 km cells, which that test calls irregular, long
  // clear-air legs lost 0.7 % of the per-photon identity with the oracle for a 2 % gain, so those keep the table.)
  p.xyRegularWalk = (c->xyRegular && c->regularWalk) ? 1 : 0;
  p.zRegularWalk = (c->zRegular && c->regularWalk) ? 1 : 0;
  p.dXf = (float)((p.xMax - p.x0) / c->nx); p.dYf = (float)((p.yMax - p.y0) / c->ny); p.dZf = (float)((p.zMax - p.z0) / c->nz);
  p.layerSkip = (c->layerSkip && !facewalk_on(c)) ? 1 : 0;  // (level fluxes: every z face is a stop; actinic flux: every face)
  p.actScale = actinic_on(c) ? (float)(1.0 / actinic_unit(c)) : 0.0f;
  p.layerRun = c->dLayerRun.get(); p.layerRunT = c->dLayerRunT.get();
  p.fly = 0; p.flyNbx = p.flyNby = 0;  // (switched on by launch_trace where the plan allows it)
  p.flyRange = c->dFlyRange.get(); p.bgVal = c->dBgVal.get();
  p.invLx = 1.0 / p.Lx; p.invLy = 1.0 / p.Ly;
  p.invCellX = (double)c->nx / p.Lx; p.invCellY = (double)c->ny / p.Ly;
  {
    bool u = true;  // equally spaced to a millionth of a cell: the cell of a position is guessed by division
    for (int i = 0; i <= c->nx && u; ++i) u = std::fabs((c->xe[i] - p.x0) * p.invCellX - i) <= 1e-6;
    for (int i = 0; i <= c->ny && u; ++i) u = std::fabs((c->ye[i] - p.y0) * p.invCellY - i) <= 1e-6;
    p.xyNearUniform = u ? 1 : 0;
    bool uz = true;
    const double invCellZ = (double)c->nz / (p.zMax - p.z0);
    for (int i = 0; i <= c->nz && uz; ++i) uz = std::fabs((c->ze[i] - p.z0) * invCellZ - i) <= 1e-6;
    p.zNearUniform = uz ? 1 : 0;
  }
  p.edges = c->dEdges.get();
  if (use_bricks(c)) {
    p.ext = c->dExtB.get(); p.cum = c->dCumB.get(); p.ssa = c->dSsaB.get(); p.pfi = c->dPfiB.get();
    p.extWalk = p.ext;
    p.brickTable = c->dBrickTable.get(); p.nbx = c->nbx; p.nby = c->nby; p.nbz = c->nbz; p.nStored = c->nStored;
    p.bgExt = c->dBgExt.get(); p.bgCum = c->dBgCum.get(); p.bgSsa = c->dBgSsa.get(); p.bgPfi = c->dBgPfi.get();
  } else {
    p.ext = c->dExt.get(); p.cum = c->dCum.get(); p.ssa = c->dSsa.get(); p.pfi = c->dPfi.get();
    p.extWalk = p.ext;
    p.bgExt = c->dLayerExt.get();  // dense layout: the per-layer slot holds the uniform-layer shortcut
    p.rec = reinterpret_cast<const uint4 *>(c->dRec.get());
  }
  p.albedo = c->albedo;
  p.surfNumX = c->surfNumX; p.surfNumY = c->surfNumY; p.surfX = c->dSurfX.get(); p.surfY = c->dSurfY.get(); p.surfRefl = c->dSurfRefl.get();
  p.surfKind = c->surfNumX > 0 ? c->surfKind : 0;
  if (p.surfKind != 0) p.surfRefl = reinterpret_cast<const float *>(c->dSurfBrdf.get());  // (float4 per patch)
  if (p.surfKind == BRDF_COXMUNK && c->glintSampling) p.surfKind |= kSurfKindSampled;
  p.tables = c->dTables.get();
  for (int k = 0; k < c->nc; ++k) { p.tblOffset[k] = c->tblOffset[k]; p.tblNSteps[k] = c->tblNSteps[k]; p.tblInvN[k] = 1.0f / (float)c->tblNSteps[k]; }
  p.tblTotalFloats = c->tblTotalFloats;
  p.useRR = c->useRR;
  p.lwFlag = c->lwFlag > 0.f ? 1 : 0;
  p.srcKind = c->srcKind;
  p.dir0[0] = c->dir0[0]; p.dir0[1] = c->dir0[1]; p.dir0[2] = c->dir0[2];
  p.zLaunch = c->zLaunch; p.izLaunch = c->izLaunch;
  p.solarKind = c->solarKind; p.spotX = c->spotX; p.spotY = c->spotY;
  p.voxelCDF = c->dVoxelCDF.get(); p.fracAtms = c->fracAtms;
  p.nDir = c->nDir;
  p.dirData = c->dDirData.get(); p.fwdTables = c->dFwd.get(); p.fwdOrig = c->dFwdOrig.get();
  for (int k = 0; k < c->nc && c->nDir > 0; ++k) { p.fwdOffset[k] = c->fwdOffset[k]; p.fwdNAngles[k] = c->fwdNAngles[k]; }
  p.useHybrid = c->useHybrid; p.numOrdersOrig = c->numOrdersOrig; p.useRRIntensity = c->useRRIntensity; p.zetaMin = c->zetaMin;
  p.limitContrib = c->limitContrib; p.maxContrib = c->maxContrib;
  p.nBlocks = c->nBlocks; p.blockRec = reinterpret_cast<const uint4 *>(c->dBlockRec.get()); p.blockOf = c->dBlockOf.get(); p.blockExt = c->dBlockExt.get();
  p.blockSsa = c->dBlockSsa.get(); p.blockCum = c->dBlockCum.get(); p.blockPfi = c->dBlockPfi.get();
  p.crossThreshold = std::max(1, std::min(64, c->crossThreshold));
  p.jumpThreshold = std::max(1, std::min(64, c->jumpThreshold));
  p.bad = c->dBad.get();
  p.maxEvents = c->maxEvents; p.maxEventsNaN = std::min(c->maxEventsNaN, c->maxEvents); p.watchdog = c->watchdog;  // (the kernels test the smaller one first)
  p.legacyTies = c->legacyTies;
  {
    // no view ray is longer than the domain's height over the smallest |mu| of the views (and a hair for rounding)
    float muMin = 1.0f;
    for (int i = 0; i < c->nDir; ++i) muMin = std::min(muMin, std::fabs(c->dirData[(size_t)8 * i + 2]));
    p.rayMaxLen = (float)((p.zMax - p.z0) / (double)std::max(muMin, FLT_MIN)) * 1.0001f + 1e-6f;
    if (c->testRayMaxLen > 0.0f) p.rayMaxLen = c->testRayMaxLen;  // TEST ONLY (MCBRAT_TEST_RAY_MAX_LEN): drive the bound on purpose
  }
  p.counter = c->L().dCounter.get();
  p.numRecScatOrd = -1;  // (mcbrat_compute_radiative_transfer switches the order tallies on)
  p.eventThreshold = std::max(1, std::min(64, c->eventThreshold));
  // The thermal source's launch is several hundred instructions (three searches of the emission CDF, double divisions,
  // sine and cosine in full precision) for photons that live two or three legs: served eight lanes at a time it was half
  // of config 4's kernel time.  Dead lanes wait for company instead: 32 (config 4: 3.8 -> 5.1e9 photons/s; 24-40 are level).
  p.launchThreshold = std::max(1, std::min(64, c->launchThresholdSet ? c->launchThreshold : (c->srcKind != 0 ? 32 : c->launchThreshold)));
  p.surfaceThreshold = std::max(1, std::min(64, c->surfaceThreshold));
}

constexpr size_t kLdsBudget = 64 * 1024;      // dynamic LDS of a workgroup that shares its compute unit with another one (two workgroups of 768 lanes, four of 256)
constexpr size_t kTableLdsLimit = 48 * 1024;   // tables above this stay in L2 (shared plans)
constexpr size_t kPrivSlabLimit = 32 * 1024;   // private tally slab above this -> the wide plan, else global atomics
constexpr size_t kStaticLds = 6 * 1024;        // room kept for the kernels' static __shared__ arrays (descriptors; trace_kernel's s_flyTC is 4 KB at 1024 lanes)

// LDS of the per-layer tables: extinction (float), run (int), cumulative optical depth (double, nz + 1 padded to even);
// clear-air flight: background extinction (float), the brick columns' cloud ranges as heights (2 floats) and layers (u16)
size_t per_layer_lds(int nz, int flyCols = 0) {
  return 2 * sizeof(float) * (size_t)((nz + 3) & ~3) + sizeof(double) * (size_t)((nz + 2) & ~1) +
         (flyCols ? sizeof(float) * (size_t)((nz + 3) & ~3) + 2 * sizeof(float) * (size_t)flyCols + sizeof(uint16_t) * (size_t)((flyCols + 3) & ~3) : 0);
}

// clear-air flight: asked for (layerSkip 1: where the background is thin enough for it to pay; 3: regardless) and possible
bool flight_wanted(const mcbrat_ctx *c) {
  return !facewalk_on(c) && c->flyBuilt && (c->layerSkip == 3 || (c->layerSkip == 1 && c->flyDepth <= c->flightMaxDepth));
}

bool blocks_worth_it(const mcbrat_ctx *c) {
  if (!c->blockWalk || c->nDir > 0 || c->nBlocks <= 0 || orders_on(c) || facewalk_on(c)) return false;  // (the block walk has no ORD, LVL or ACT variant)
  if (c->surfNumX > 0 && c->surfKind != 0) return false;  // (nor a BRDF one: such surfaces go face by face)
  const size_t nvox = (size_t)c->nx * c->ny * c->nz;
  return (size_t)c->nBlocks * 4 <= nvox || c->blockWalk == 2;  // (2: forced, for tests of heterogeneous media)
}

LaunchPlan plan_launch(const mcbrat_ctx *c, size_t slabStride) {
  LaunchPlan L;
  L.wide = false; L.blockLite = false; L.optics = 0; L.cdfTop = false;
  const size_t edges = sizeof(double) * (size_t)(c->nx + c->ny + c->nz + 3);
  const size_t tbl = sizeof(float) * (size_t)c->tblTotalFloats;
  // (the level and actinic bins, which lie behind slabLds in every slab of this context, are never part of the LDS slab)
  const size_t slab = sizeof(long long) * std::min(slabStride, (size_t)tally_layout(c).slabLds) + 16;
  L.priv = c->privMode != 0 && slab <= kPrivSlabLimit;
  L.brick = use_bricks(c);
  const size_t bg = per_layer_lds(c->nz);  // per-layer extinction (background / one-extinction layers) and the runs of such layers
  L.tblLds = tbl <= kTableLdsLimit && edges + bg + tbl + (L.priv ? slab : 0) <= kLdsBudget;
  if (L.priv && edges + bg + slab + (L.tblLds ? tbl : 0) > kLdsBudget) L.priv = false;
  // small domains: the optical grid itself (ext + per-component cum, ssa, phase index) goes to LDS when it fits
  const size_t nvox = (size_t)c->nx * c->ny * c->nz;
  const size_t grid = nvox * 4 + (size_t)c->nc * nvox * (4 + 4) + (((size_t)c->nc * nvox + 1) & ~(size_t)1) * 2;
  L.gridLds = L.priv && c->gridLdsMode != 0 && edges + bg + slab + grid + (L.tblLds ? tbl : 0) <= kLdsBudget;
  // scattering orders: where the order bins leave room for the grid or the tables but not both, the grid stays in LDS (every walk
  // step reads it, a collision one table entry) and the tables go to L2 (the step cloud: DESIGN.md section 4.9)
  if (orders_on(c) && L.priv && L.tblLds && !L.gridLds && c->gridLdsMode != 0 && edges + bg + slab + grid <= kLdsBudget) {
    L.tblLds = false;
    L.gridLds = true;
  }
  // level fluxes, actinic flux: the LVL and ACT kernels are built for everything in LDS (PRIV = 2) and for global atomics (PRIV = 0);
  // private tallies beside a grid in global memory give way to the latter
  if (facewalk_on(c) && L.priv && !L.gridLds) {
    L.priv = false;
    L.tblLds = tbl <= kTableLdsLimit && edges + bg + tbl <= kLdsBudget;
  }
  L.lds = edges + bg + (L.priv ? slab : 0) + (L.gridLds ? grid : 0) + (L.tblLds ? tbl : 0);
  // the wide plan: the slab did not fit beside another workgroup, but it fits a compute unit
  const size_t cuLds = c->ldsPerCU > kStaticLds ? c->ldsPerCU - kStaticLds : 0;
  if ((!L.priv || c->wideMode == 2) && c->privMode != 0 && c->wideMode != 0 && c->nDir == 0 && !orders_on(c) && !facewalk_on(c) && !L.brick && c->blockSize == 0 && edges + bg + slab <= cuLds) {
    L.wide = true; L.priv = true; L.fly = false;
    size_t need = edges + bg + slab;
    L.tblLds = need + tbl <= cuLds;
    if (L.tblLds) need += tbl;
    L.gridLds = c->gridLdsMode == 1 && need + grid <= cuLds;
    if (L.gridLds) need += grid;
    L.lds = need;
    L.block = 1024;
    // block walk with the per-cell optics left in global memory: what a medium made of blocks whose grid does not fit still gets
    if (!L.gridLds && blocks_worth_it(c) && c->gridLdsMode != 0) {
      const int opt = (c->blockOpticsUniform && c->gridLdsMode != 2) ? 2 : 1;  // (gridLdsMode 2: per-cell optics in global memory asked for, tests)
      const BlockLds B = block_lds_layout(c->nx, c->ny, c->nz, c->nc, slabStride, c->nBlocks, (size_t)c->tblTotalFloats, opt);
      const BlockLds B0 = block_lds_layout(c->nx, c->ny, c->nz, c->nc, slabStride, c->nBlocks, 0, opt);
      if (B.total <= cuLds) { L.blockLite = true; L.tblLds = true; L.optics = opt; }
      else if (B0.total <= cuLds) { L.blockLite = true; L.tblLds = false; L.optics = opt; }
    }
    if (blocks_worth_it(c) && (L.gridLds || L.blockLite) && c->srcKind != 0)  // the emission CDF's level and row sums beside them, where they fit
      L.cdfTop = block_lds_layout(c->nx, c->ny, c->nz, c->nc, slabStride, c->nBlocks, L.tblLds ? (size_t)c->tblTotalFloats : 0, L.optics, true).total <= cuLds;
    return L;
  }
  const size_t flyLds = per_layer_lds(c->nz, c->flyNbx * c->flyNby) - bg;
  L.fly = flight_wanted(c) && !L.gridLds && !L.brick && c->nDir == 0 && L.lds + flyLds <= kLdsBudget;
  if (L.fly) L.lds += flyLds;
  L.block = c->blockSize > 0 ? c->blockSize : (L.gridLds ? 768 : ((L.tblLds || L.priv) && L.lds > 16 * 1024 ? 512 : 256));
  if (facewalk_on(c) && L.block > 512) L.block = 512;  // (no 768-lane LVL or ACT kernel)
  if (blocks_worth_it(c) && L.priv && L.gridLds && c->srcKind != 0)
    L.cdfTop = block_lds_layout(c->nx, c->ny, c->nz, c->nc, slabStride, c->nBlocks, L.tblLds ? (size_t)c->tblTotalFloats : 0, 0, true).total <= kLdsBudget;
  // fill_params chose the brick arrays: private tallies give way.  Decided last, so that tblLds, block and cdfTop stay
  // those of the plan with private tallies.  (No flight over bricks: the LDS is the edge, layer and table part.)
  if (L.priv && L.brick) {
    L.priv = false;
    L.gridLds = false;
    L.lds = edges + bg + (L.tblLds ? tbl : 0);
  }
  return L;
}

// Units per batch for the kernels whose workgroups keep one batch's tallies in LDS (a workgroup traces photons of one
// batch at a time).  A unit ends with a drain -- its lanes fall idle while its last histories finish, about 0.3 ms on
// the step cloud, the time of ~4000 photons of a workgroup's throughput -- and units are dealt out to `blocks` resident
// workgroups in rounds: the choice minimises rounds x (photons per unit + drain).  (The former rule, blocks / batches
// rounded down, left a fifth of the workgroup slots empty for 200 or 400 batches: 4.7-4.9 instead of 5.3e9 photons/s.)
inline unsigned long long units_per_batch(unsigned long long blocks, unsigned long long ppb, int nBatches, int blockSize) {
  const unsigned long long maxUpb = std::max<unsigned long long>(1, ppb / (unsigned long long)(blockSize * 8));
  const double drainPhotons = 4000.0;
  unsigned long long best = 1;
  double bestCost = 1e300;
  // (up to one unit per resident workgroup and a few rounds of them: a call of ONE large batch -- a wavelength's whole share
  // of a broadband run -- must still reach every compute unit; the cap was 64, a quarter of the wide plan's 256 workgroups)
  for (unsigned long long upb = 1; upb <= std::min<unsigned long long>(maxUpb, std::max<unsigned long long>(64, 4 * blocks)); ++upb) {
    const unsigned long long units = upb * (unsigned long long)nBatches;
    const unsigned long long rounds = (units + blocks - 1) / blocks;
    const double cost = (double)rounds * ((double)ppb / (double)upb + drainPhotons);
    if (cost < bestCost * (1.0 - 1e-9)) { bestCost = cost; best = upb; }
  }
  return best;
}

// How a launch cuts its photons into work units
enum class Units {
  PerBlock,   // tallies in global memory: one workgroup per `block` photons, no more than are resident
  PerBatch,   // every workgroup traces photons of one batch at a time: each batch cut into units_per_batch units
  // The block walk.  Launch-wide (the default): every resident workgroup gets the same share of the launch's photons, cut
  // across batch boundaries, and keeps the tallies of the two batches its share may touch in two LDS slabs -- no workgroup
  // slot stays empty (cut inside batches, 100 batches of the step cloud make 500 units for 512 slots) and all units end
  // together.  Per batch: where a share would be longer than a batch, or where two slabs would cost residency or not fit.
  BlockWalk,
};

// Launches one instantiation of trace_kernel or trace_block_kernel on the lane's stream: as many workgroups as are resident
// at `lds` bytes of dynamic LDS (the occupancy query, or the option blocksPerCU), and no more than there are work units.
// ldsTwoSlabs: the block walk's layout with the slabs of launch-wide units.
int launch_kernel(mcbrat_ctx *c, DevParams &p, const void *kernel, int block, size_t lds, Units units, int nBatches,
                  size_t ldsTwoSlabs = 0) {
  size_t allowed = kLdsBudget;  // dynamic LDS the kernel may take (above the default limit of a workgroup: by attribute)
  int perCU = c->blocksPerCU;
  if (perCU <= 0) {
    if (lds > allowed) {
      HIP_OK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      allowed = lds;
    }
    HIP_OK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, block, lds));
    perCU = std::max(1, std::min(perCU, 8));
  }
  unsigned long long blocks = (unsigned long long)perCU * c->numCUs;
  bool launchWide = false;
  if (units == Units::BlockWalk) {  // (512 bytes: the kernel's static LDS)
    const unsigned long long n = std::max<unsigned long long>(1, std::min(blocks, p.total));
    launchWide = !c->batchUnits && (p.total + n - 1) / n <= p.ppb && (size_t)perCU * (ldsTwoSlabs + 512) <= c->ldsPerCU;
    p.unitsWide = launchWide;
    if (launchWide) {
      lds = ldsTwoSlabs;
      p.nUnits = blocks = n;
    }
  }
  if (units == Units::PerBlock) {
    blocks = std::min(blocks, (p.total + block - 1) / block);
  } else if (!launchWide) {  // about one unit per resident workgroup
    const unsigned long long upb = units_per_batch(blocks, p.ppb, nBatches, block);
    p.unitsPerBatch = upb;
    p.nUnits = upb * (unsigned long long)nBatches;
    blocks = std::min(blocks, p.nUnits);
  }
  if (lds > allowed) HIP_OK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  p.ldsBytes = (unsigned)lds;
  void *args[] = {&p};
  (void)hipLaunchKernel(kernel, dim3((unsigned)std::max<unsigned long long>(1, blocks)), dim3(block), args, lds, c->L().stream);
  HIP_OK(c, hipGetLastError());  // (the launch's error, if any)
  return 0;
}

// One table of kernel pointers per kernel, built from the lists of mcbrat_variants.h: entry I is the instantiation that entry I of
// the list names.  These two templates are the only places where the kernels' positional template arguments are written out.
constexpr auto kTraceList = trace_variants();
constexpr auto kBlockList = block_variants();
static_assert(kTraceList.n == kTraceVariants && kBlockList.n == kBlockVariants, "the lists are as long as they say");
template <int I>
const void *trace_entry() {
  constexpr TraceVariant v = kTraceList.v[I];
  return (const void *)trace_kernel<v.block, v.tblLds, v.priv, v.brick, v.debug, v.inten, v.emit, v.spec, v.ord, v.brdf, v.lvl, v.direct, v.act, v.side>;
}
template <int I>
const void *block_entry() {
  constexpr BlockVariant v = kBlockList.v[I];
  return (const void *)trace_block_kernel<v.block, v.tblLds, v.debug, v.emit, v.simple, v.opt, v.nospan, v.rare>;
}
constexpr auto kBlockRareList = block_rare_variants();
static_assert(kBlockRareList.n == kBlockRareVariants, "the list is as long as it says");
template <int I>
const void *block_rare_entry() {
  constexpr BlockVariant v = kBlockRareList.v[I];
  static_assert(valid(v) && v.rare != 0, "the RARE list holds RARE instantiations");
  return (const void *)trace_block_kernel<v.block, v.tblLds, v.debug, v.emit, v.simple, v.opt, v.nospan, v.rare>;
}
template <int... I>
std::array<const void *, sizeof...(I)> trace_table(std::integer_sequence<int, I...>) { return {{trace_entry<I>()...}}; }
template <int... I>
std::array<const void *, sizeof...(I)> block_table(std::integer_sequence<int, I...>) { return {{block_entry<I>()...}}; }
const std::array<const void *, kTraceVariants> kTraceKernels = trace_table(std::make_integer_sequence<int, kTraceVariants>{});
const std::array<const void *, kBlockVariants> kBlockKernels = block_table(std::make_integer_sequence<int, kBlockVariants>{});
template <int... I>
std::array<const void *, sizeof...(I)> block_rare_table(std::integer_sequence<int, I...>) { return {{block_rare_entry<I>()...}}; }
const std::array<const void *, kBlockRareVariants> kBlockRareKernels = block_rare_table(std::make_integer_sequence<int, kBlockRareVariants>{});
const char *const kNoKernelMsg = "computeRadiativeTransfer: no kernel is built for this combination of settings.";

// What the block walk's instantiations decide at compile time, of this context (the near-uniform flags: fill_params)
BlockWalk block_walk_of(const mcbrat_ctx *c, bool xyNearUniform, bool zNearUniform) {
  return BlockWalk{c->xyRegular != 0, c->zRegular != 0, c->nc == 1, c->surfNumX != 0, c->ny == 1, xyNearUniform, zNearUniform, c->noSimple3,
                   c->blockSpansX, c->blockSpansY, c->blockSpanKernel != 0, c->blockSize,
                   c->albedo == 0.0f && c->surfNumX == 0 && c->ssaFinite, c->solarKind == 0, c->blockRareKernel != 0};
}

// The block walk applies where the face-by-face plan already keeps grid, tallies (and tables) in LDS -- or, in the wide
// plan, tallies and the cells' block numbers (blockLite) -- radiance is off, and blocks are worth it: at least four cells
// per block on average (a medium that differs from cell to cell would pay a position look-up at every face for nothing).
bool block_walk_applies(const mcbrat_ctx *c, const LaunchPlan &L) {
  return blocks_worth_it(c) && ((L.priv && L.gridLds) || L.blockLite);
}

// What a launch runs: one instantiation, its workgroup size and its dynamic LDS.  kernel == nullptr: refused, the context's error says why.
struct KernelChoice { const void *kernel; int block; size_t lds; };

// (lds: the layout of launch_block, which knows the slabs)
KernelChoice choose_block(mcbrat_ctx *c, const DevParams &p, const LaunchPlan &L, bool debug) {
  const BlockVariant v = pick_block(L, debug, c->srcKind != 0, block_walk_of(c, p.xyNearUniform != 0, p.zNearUniform != 0));
  const int i = v.rare != 0 ? find_variant(kBlockRareList, v) : find_variant(kBlockList, v);
  if (i < 0) { fail(c, kNoKernelMsg); return {nullptr, 0, 0}; }
  return {v.rare != 0 ? kBlockRareKernels[(size_t)i] : kBlockKernels[(size_t)i], v.block, 0};
}

int launch_block(mcbrat_ctx *c, DevParams &p, const LaunchPlan &L, bool debug, int nBatches) {
  p.cdfTopLds = L.cdfTop ? 1 : 0;
  const int opt = L.blockLite ? L.optics : 0;
  const auto lds = [&](size_t slabs) {  // the kernel's layout with the tallies of one batch, or of two (launch-wide units)
    return block_lds_layout(c->nx, c->ny, c->nz, c->nc, slabs * (size_t)p.slabStride, c->nBlocks, L.tblLds ? (size_t)c->tblTotalFloats : 0,
                            opt, L.cdfTop).total;
  };
  if (lds(1) + 512 > c->ldsPerCU) return fail(c, "computeRadiativeTransfer: the block-walk tables do not fit the LDS of a compute unit.");
  const KernelChoice k = choose_block(c, p, L, debug);
  if (!k.kernel) return 1;
  return launch_kernel(c, p, k.kernel, k.block, lds(1), Units::BlockWalk, nBatches, lds(2));
}

// The settings of a launch: the order tallies are the parameter block's (an instrumented trace has none), debug the launch's
Asked launch_asked(const mcbrat_ctx *c, const DevParams &p, bool debug) {
  Asked a = asked(c);
  a.numRecScatOrd = p.numRecScatOrd; a.debug = debug;
  return a;
}

// The choosing part of launch_trace: the instantiation for a plan and the context's settings, after launch_trace's refusals (each
// but the instrumented radiance and order runs is refused where it is asked for and by check_ready: a second line of defence);
// sets the ray fields of the parameter block on radiance runs.
KernelChoice choose_trace(mcbrat_ctx *c, DevParams &p, const LaunchPlan &L, bool debug) {
  const Settings s = settings_of(c, launch_asked(c, p, debug));
  const TraceWalk w{p.rec != nullptr, p.layerSkip != 0, p.fly != 0, p.surfNumX != 0, p.xyRegularWalk != 0, p.zRegularWalk != 0, p.useRR != 0, p.nc, p.solarKind};
  const TraceVariant v = pick_trace(L, s, w);
  const int i = find_variant(kTraceList, v);
  const char *why = refusal(s, Launch);
  if (why || i < 0) {  // (never a null pointer to launch)
    fail(c, why ? why : kNoKernelMsg);
    return {nullptr, 0, 0};
  }
  size_t lds = L.lds;
  if (v.inten) {  // radiance runs: the waves' buffers of unfinished long rays (ray_cap, mcbrat_variants.h)
    const int cap = ray_cap(v.block, L.priv, L.lds, c->ldsPerCU, c->rayDefer != 0, c->nx + c->ny + c->nz + 3 <= 0xffff && c->nDir <= 0xffff);
    p.rayCap = cap;
    // measured on the 128x128x64 cloud field, 4 directions: with roulette most rays end within a few cells and the long
    // ones are best served in short, dense passes; without it every ray runs to the boundary and long passes pay
    p.rayShort = c->rayShort > 0 ? c->rayShort : (c->useRRIntensity ? 4 : 8);
    p.rayPassIters = c->rayPassIters > 0 ? c->rayPassIters : (c->useRRIntensity ? 16 : 64);
    p.rayPassAt = std::min<int>(c->rayPassAt > 0 ? c->rayPassAt : (c->useRRIntensity ? 56 : 40), cap);
    lds = ray_lds(v.block, L.lds, cap);
  }
  return {kTraceKernels[(size_t)i], v.block, lds};
}

int launch_trace(mcbrat_ctx *c, DevParams &p, bool debug, int nBatches) {
  const LaunchPlan L = plan_launch(c, (size_t)p.slabStride);
  if (L.fly) {
    p.fly = 1; p.flyNbx = c->flyNbx; p.flyNby = c->flyNby; p.extWalk = c->dExtWalk.get();
    p.flyInvBrickX = (float)(c->flyNbx / p.Lx); p.flyInvBrickY = (float)(c->flyNby / p.Ly);
  }
  if (block_walk_applies(c, L)) return launch_block(c, p, L, debug, nBatches);
  const KernelChoice k = choose_trace(c, p, L, debug);
  if (!k.kernel) return 1;
  // (very tall grids: the per-layer tables alone can pass the default limit of a workgroup)
  if (k.lds + kStaticLds > c->ldsPerCU && k.lds > kLdsBudget) return fail(c, "computeRadiativeTransfer: the grid's edge and layer tables do not fit the LDS of a compute unit.");
  return launch_kernel(c, p, k.kernel, k.block, k.lds, L.priv ? Units::PerBatch : Units::PerBlock, nBatches);
}

int check_ready(mcbrat_ctx *c) {
  if (!c) return 1;
  if (!c->haveGrid || !c->haveOptics) return fail(c, "computeRadiativeTransfer: problem not completely specified.");
  if (!c->haveSource) return fail(c, "computeRadiativeTransfer: no photon source set.");
  REFUSE(c, asked(c), Ready);  // (each is also refused where it is asked for, whichever call comes first; the thermal source only here)
  if (sync_tables(c)) return 1;
  return sync_forward_tables(c);
}

// Times short trial launches at a few event thresholds and keeps the fastest.  The best value
// depends on how many voxel faces a leg crosses (step cloud ~3, 128x128x64 cloud field ~14).
int autotune(mcbrat_ctx *c, DevParams p, unsigned long long ppb, int nBatches) {
  // about 170 photons per resident lane (6.7e7): with fewer the synchronised start and the drain of the launch favour too
  // low a threshold -- measured on the two 128x128x64 workloads, trials of 1.7e7 / 3.4e7 / 6.7e7 / 1.3e8 photons chose
  // 8 / 16 / 20-24 / 24 on the radar-like field (8 costs 13 % of the rate of 24) and 20-32 / 20 / 24 / 24 on the cloud field
  // (radiance runs cost several times more per photon: fewer trial photons, so that the ten trial launches stay well under a second)
  const unsigned long long want = c->tuneTrialPhotons / (unsigned long long)(1 + 2 * c->nDir);
  const unsigned long long total = ppb * (unsigned long long)nBatches;
  if (total < want) {
    // too few photons for a meaningful trial: a guess by domain size (few faces per leg on small grids, many on
    // large ones), and the trial is left for a later, larger call
    // (the thermal source: photons start inside the medium and most end at their first roulette -- few lanes are ever on a
    // long walk, and waiting for 24 of them starves the event phase: 4-8 measured best on config 4, 24 costs 8 %)
    // (the block walk has no walk loop: its threshold only says when a wave has little else to do than its queued work --
    // 16-32 measured best on config 4's wide kernel too, 8 costs it 2.5 %)
    const LaunchPlan L0 = plan_launch(c, (size_t)p.slabStride);
    c->eventThreshold = block_walk_applies(c, L0) ? 16 : (c->srcKind != 0 ? 8 : (L0.gridLds ? 16 : 24));
    return 0;
  }
  const int nb = (int)std::max<unsigned long long>(1, std::min<unsigned long long>((unsigned long long)nBatches, want / std::max<unsigned long long>(1, ppb)));
  p.total = std::min(want, ppb * (unsigned long long)nb);
  p.fates = nullptr; p.counters = nullptr;
  const int candidates[] = {8, 16, 20, 24, 32, 48};
  float best = 1e30f;
  int bestThr = c->eventThreshold;
  for (int thr : candidates) {
    p.eventThreshold = thr;
    float ms = 1e30f;
    for (int rep = 0; rep < 2; ++rep) {  // first repetition warms caches / code
      HIP_OK(c, hipMemsetAsync(c->L().dSlabs.get(), 0, sizeof(long long) * p.slabStride * nb, c->L().stream));
      HIP_OK(c, hipMemsetAsync(c->L().dCounter.get(), 0, sizeof(unsigned long long), c->L().stream));
      HIP_OK(c, hipEventRecord(c->L().ev0, c->L().stream));
      if (launch_trace(c, p, false, nb)) return 1;
      HIP_OK(c, hipEventRecord(c->L().ev1, c->L().stream));
      HIP_OK(c, hipStreamSynchronize(c->L().stream));
      HIP_OK(c, hipEventElapsedTime(&ms, c->L().ev0, c->L().ev1));
    }
    if (ms < best) { best = ms; bestThr = thr; }
  }
  c->eventThreshold = bestThr;
  c->tuned = true;
  return 0;
}

}  // namespace

// The backward camera's view of a context (mcbrat_camera_ctx.h; mcbrat_camera.hip is a translation unit of its own)
int mcbrat_camera_fail(mcbrat_ctx *c, const char *msg) { return fail(c, msg); }
int mcbrat_camera_context(mcbrat_ctx *c, CameraContext *out, bool needTables) {
  if (!c || !out) return 1;
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  *out = CameraContext{};
  out->device = c->device; out->numCUs = c->numCUs; out->ldsPerCU = c->ldsPerCU;
  out->haveGrid = c->haveGrid; out->haveOptics = c->haveGrid && c->haveOptics; out->haveSource = c->haveSource;
  out->solarDirectional = c->haveSource && c->srcKind == 0 && c->solarKind == 0;
  out->brdfSurface = c->surfNumX > 0 && c->surfKind != 0;
  out->nc = c->nc; out->gridInLds = c->cameraGridInLds; out->pathBinsInLds = c->cameraPathBinsInLds;
  out->xe = &c->xe; out->ye = &c->ye; out->ze = &c->ze;
  out->fwd = &c->fwdOrig; out->fwdNAngles = &c->fwdNAngles; out->fwdNEntries = &c->fwdNEntries; out->maxPfi = &c->maxPfi;
  if (!out->haveOptics) return 0;
  if (init_lane(c, c->cur)) return 1;
  out->stream = c->L().stream;
  if (needTables) {
    if (sync_tables(c)) return 1;
    out->haveInverseTables = true;
  }
  fill_params(c, out->p);
  out->p.ext = c->dExt.get(); out->p.cum = c->dCum.get(); out->p.ssa = c->dSsa.get(); out->p.pfi = c->dPfi.get();
  out->p.extWalk = out->p.ext;
  out->p.brickTable = nullptr;
  return 0;
}

extern "C" {

int mcbrat_abi_version(void) { return MCBRAT_ABI_VERSION; }

mcbrat_ctx *mcbrat_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mcbrat_ctx *c = new mcbrat_ctx();
  c->device = device;
  if (const char *e = getenv("MCBRAT_REGULAR_WALK")) c->regularWalk = atoi(e);
  if (const char *e = getenv("MCBRAT_LAYER_SKIP")) c->layerSkip = atoi(e);
  if (const char *e = getenv("MCBRAT_BLOCK_WALK")) c->blockWalk = atoi(e);
  if (const char *e = getenv("MCBRAT_FLIGHT_MAX_DEPTH")) c->flightMaxDepth = atof(e);
  if (const char *e = getenv("MCBRAT_WIDE")) c->wideDefault = c->wideMode = std::max(0, std::min(2, atoi(e)));
  if (const char *e = getenv("MCBRAT_JUMP_THRESHOLD")) c->jumpThreshold = std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MCBRAT_CROSS_THRESHOLD")) c->crossThreshold = std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MCBRAT_BATCH_UNITS")) c->batchUnits = atoi(e) != 0;
  if (getenv("MCBRAT_NO_SIMPLE3")) c->noSimple3 = true;
  if (const char *e = getenv("MCBRAT_RAY_DEFER")) c->rayDefer = atoi(e);
  if (const char *e = getenv("MCBRAT_RAY_SHORT")) c->rayShort = std::max(1, atoi(e));
  if (const char *e = getenv("MCBRAT_RAY_PASS_ITERS")) c->rayPassIters = std::max(1, atoi(e));
  if (const char *e = getenv("MCBRAT_RAY_PASS_AT")) c->rayPassAt = std::max(1, atoi(e));
  if (const char *e = getenv("MCBRAT_TUNE_PHOTONS")) c->tuneTrialPhotons = strtoull(e, nullptr, 10);
  if (const char *e = getenv("MCBRAT_WATCHDOG")) c->watchdog = (unsigned)std::max(16ll, atoll(e));
  if (const char *e = getenv("MCBRAT_MAX_EVENTS")) c->maxEvents = (unsigned)std::max(16ll, atoll(e));
  if (const char *e = getenv("MCBRAT_MAX_EVENTS_NAN")) c->maxEventsNaN = (unsigned)std::max(16ll, atoll(e));
  if (const char *e = getenv("MCBRAT_TEST_LEGACY_TIES")) c->legacyTies = atoi(e);
  if (const char *e = getenv("MCBRAT_TEST_RAY_MAX_LEN")) c->testRayMaxLen = (float)atof(e);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    c->numCUs = prop.multiProcessorCount;
    if (prop.maxSharedMemoryPerMultiProcessor > 0) c->ldsPerCU = prop.maxSharedMemoryPerMultiProcessor;
  }
  if (init_lane(c, 0) || hipEventCreateWithFlags(&c->evExternal, hipEventDisableTiming) != hipSuccess ||
      c->dEventCounters.allocate(32) != 0 ||
      c->dBad.allocate(kBadWords) != 0 ||  // count, claim word, record of the first drop
      hipMemsetAsync(c->dBad.get(), 0, kBadWords * sizeof(unsigned long long), c->lane[0].stream) != hipSuccess ||
      hipStreamSynchronize(c->lane[0].stream) != hipSuccess ||
      c->hBad.allocate(1) != 0 ||
      hipHostGetDevicePointer((void **)&c->hBadDev, c->hBad.get(), 0) != hipSuccess) {
    mcbrat_destroy(c);
    return nullptr;
  }
  *c->hBad.get() = 0ull;
  return c;
}

void mcbrat_destroy(mcbrat_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)sync_all(c);
  delete c;  // (the owners free and destroy: ~mcbrat_ctx, ~LaneHandles, mcbrat_devmem.h; a half-built context of mcbrat_create holds nulls)
}

const char *mcbrat_last_error(const mcbrat_ctx *c) { return c ? c->err.c_str() : "mcbrat: no context (no usable HIP device)"; }

int mcbrat_set_grid(mcbrat_ctx *c, int32_t nx, int32_t ny, int32_t nz, const double *xe, const double *ye,
                    const double *ze) {
  if (!c) return 1;
  if (nx < 1 || ny < 1 || nz < 1 || !xe || !ye || !ze) return fail(c, "new_Integrator: Problems reading domain.");
  for (int i = 0; i < nx; ++i) if (!(xe[i + 1] > xe[i])) return fail(c, "new_Domain: x edges must be increasing, unique.");
  for (int i = 0; i < ny; ++i) if (!(ye[i + 1] > ye[i])) return fail(c, "new_Domain: y edges must be increasing, unique.");
  for (int i = 0; i < nz; ++i) if (!(ze[i + 1] > ze[i])) return fail(c, "new_Domain: z edges must be increasing, unique.");
  if ((long long)nx * ny * nz > 0x7fffffffLL / 2) return fail(c, "new_Integrator: more than 2^30 cells are not supported.");
  Asked a = asked(c);
  a.nx = nx; a.ny = ny; a.nz = nz;
  REFUSE(c, a, SetGrid);
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  c->nx = nx; c->ny = ny; c->nz = nz;
  c->xe.assign(xe, xe + nx + 1); c->ye.assign(ye, ye + ny + 1); c->ze.assign(ze, ze + nz + 1);
  // regular-spacing flags exactly as new_Integrator :163-181 (deltaX/Y/Z are default-real locals, :140)
  const float fX = (float)(xe[1] - xe[0]), fY = (float)(ye[1] - ye[0]), fZ = (float)(ze[1] - ze[0]);
  bool xr = true, yr = true, zr = true;
  for (int i = 0; i < nx; ++i) xr = xr && std::fabs((xe[i + 1] - xe[i]) - (double)fX) <= 2.0 * spacing_d(xe[i + 1]);
  for (int i = 0; i < ny; ++i) yr = yr && std::fabs((ye[i + 1] - ye[i]) - (double)fY) <= 2.0 * spacing_d(ye[i + 1]);
  for (int i = 0; i < nz; ++i) zr = zr && std::fabs((ze[i + 1] - ze[i]) - (double)fZ) <= spacing_d(ze[i + 1]);
  c->xyRegular = xr && yr; c->zRegular = zr;
  c->dX = fX; c->dY = fY; c->dZ = fZ;
  std::vector<double> edges;
  edges.insert(edges.end(), c->xe.begin(), c->xe.end());
  edges.insert(edges.end(), c->ye.begin(), c->ye.end());
  edges.insert(edges.end(), c->ze.begin(), c->ze.end());
  if (upload(c, &c->dEdges, edges.data(), edges.size())) return 1;
  // relative column areas, computeRadiativeTransfer :334-340 (real(8) expression stored to default real)
  std::vector<float> rel((size_t)nx * ny);
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i)
      rel[(size_t)i + (size_t)nx * j] = (float)(((ye[j + 1] - ye[j]) * (xe[i + 1] - xe[i])) / ((xe[nx] - xe[0]) * (ye[ny] - ye[0])));
  if (upload(c, &c->dRelArea, rel.data(), rel.size())) return 1;
  c->haveGrid = true; c->haveOptics = false; c->haveSource = false;
  // everything sized by the old grid goes: the moment arrays and the last batch's results; the per-lane buffers are re-sized by
  // the next call (their capacities are kept in elements and compared with what that call needs)
  drop_results(c, true);
  return 0;
}

int mcbrat_set_optics(mcbrat_ctx *c, int32_t nc, const double *totalExt, const double *cumExt, const double *ssa,
                      const int32_t *pfIndex, double albedo) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "getInfo_Domain: domain hasn't been initialized.");
  if (nc < 1 || nc > MCBRAT_MAX_COMPONENTS) return fail(c, "getOpticalPropertiesByComponent: unsupported number of components.");
  if (!totalExt || !cumExt || !ssa || !pfIndex) return fail(c, "getOpticalPropertiesByComponent: domain contains no optical components.");
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  const size_t nvox = (size_t)c->nx * c->ny * c->nz;
  std::vector<float> e(nvox), cu(nvox * nc), s(nvox * nc);
  std::vector<uint16_t> pf(nvox * nc);
  std::vector<int> maxPfi(nc, 0);
  for (size_t v = 0; v < nvox; ++v) {
    if (!(totalExt[v] >= 0.0)) return fail(c, "validateOpticalComponent: extinction must be >= 0.");
    e[v] = (float)totalExt[v];
  }
  for (int k = 0; k < nc; ++k)
    for (size_t v = 0; v < nvox; ++v) {
      const size_t i = (size_t)k * nvox + v;
      if (totalExt[v] > 0.0 && !(ssa[i] >= 0.0 && ssa[i] <= 1.0)) return fail(c, "validateOpticalComponent: singleScatteringAlbedo must be between 0 and 1.");
      cu[i] = (float)cumExt[i];
      s[i] = totalExt[v] > 0.0 ? (float)ssa[i] : 0.0f;  // (nothing collides without extinction; the block walk tells vacuum by this 0)
      int idx = pfIndex[i];
      if (totalExt[v] > 0.0 && (idx < 1 || idx > 65535)) return fail(c, "validateOpticalComponent: phaseFunctionIndex out of range.");
      if (idx < 1) idx = 1;
      pf[i] = (uint16_t)(idx - 1);
      if (totalExt[v] > 0.0) maxPfi[k] = std::max(maxPfi[k], idx - 1);
    }
  if (!(albedo >= 0.0 && albedo <= 1.0)) return fail(c, "new_Domain: surfaceAlbedo must be between 0 and 1.");
  if (upload(c, &c->dExt, e.data(), e.size()) || upload(c, &c->dCum, cu.data(), cu.size()) ||
      upload(c, &c->dSsa, s.data(), s.size()) || upload(c, &c->dPfi, pf.data(), pf.size()))
    return 1;
  c->dRec.reset();
  if (nc <= 2) {
    std::vector<uint32_t> rec(4 * nvox);
    for (size_t v = 0; v < nvox; ++v) {
      const float c0 = nc > 1 ? cu[v] : 2.0f;  // uniform >= c0 picks the second component: never with one component
      std::memcpy(&rec[4 * v + 0], &c0, 4);
      std::memcpy(&rec[4 * v + 1], &s[v], 4);
      const float s1 = nc > 1 ? s[nvox + v] : 0.0f;
      std::memcpy(&rec[4 * v + 2], &s1, 4);
      rec[4 * v + 3] = (uint32_t)pf[v] | ((uint32_t)(nc > 1 ? pf[nvox + v] : 0) << 16);
    }
    if (upload(c, &c->dRec, rec.data(), rec.size())) return 1;
  }
  c->bricksBuilt = false;
  if (build_bricks(c, e, cu, s, pf, nc)) return 1;
  if (build_blocks(c, e, cu, s, pf, nc, ssa)) return 1;
  c->nc = nc;
  c->albedo = (float)albedo;
  c->maxPfi = maxPfi;
  c->tables.resize(nc); c->tblNSteps.resize(nc, 0); c->tblNEntries.resize(nc, 0);
  c->tablesDirty = true;
  c->haveOptics = true;
  c->tuned = false;
  return 0;
}

int mcbrat_set_inverse_table(mcbrat_ctx *c, int32_t component, int32_t nSteps, int32_t nEntries, const float *table) {
  if (!c) return 1;
  if (!c->haveOptics) return fail(c, "tabulateInversePhaseFunctions: domain has no optical components yet.");
  if (component < 1 || component > c->nc) return fail(c, "tabulateInversePhaseFunctions: failed on component" + std::to_string(component));
  if (nSteps < 2 || nEntries < 1 || !table) return fail(c, "computeInversePhaseFunctionTable: Array for inverse table has the wrong number of entries");
  c->tables[component - 1].assign(table, table + (size_t)nSteps * nEntries);
  c->tblNSteps[component - 1] = nSteps;
  c->tblNEntries[component - 1] = nEntries;
  c->tablesDirty = true;
  return 0;
}

int mcbrat_specify_parameters(mcbrat_ctx *c, int32_t useRayTracing, int32_t useRussianRoulette, float lwFlag) {
  if (!c) return 1;
  if (!useRayTracing)
    return fail(c, "specifyParameters: useRayTracing=.false. (maximum cross-section) is not supported: "
                   "that branch of the reference never refreshes the cell indices (SURVEY.md 8a quirk 4).");
  c->useRR = useRussianRoulette ? 1 : 0;
  c->lwFlag = lwFlag;
  return 0;
}

// The launch height every solar kind shares: z = 1 - spacing(1.) of the column (monteCarloIllumination.f95:93, :128, :167,
// :207), mapped as computeRT :484-493.  Then the source is solar (srcKind 0) of the given kind.
static int set_solar_launch(mcbrat_ctx *c, int kind) {
  const double frac = (double)(1.0f - 1.1920929e-07f);
  const double z0 = c->ze.front(), zMax = c->ze.back();
  if (c->zRegular) {
    c->zLaunch = z0 + frac * (zMax - z0);
    int zi = (int)((c->zLaunch - z0) / c->dZ) + 1;
    zi = std::min(zi, c->nz);
    if (std::fabs(c->ze[zi] - c->zLaunch) < spacing_d(c->zLaunch)) zi++;
    c->izLaunch = std::min(zi, c->nz) - 1;
  } else {
    const double t = (frac - z0) * (double)c->nz;
    const double fl = std::floor(t);
    int zi = std::min((int)fl + 1, c->nz);
    zi = std::max(zi, 1);
    c->izLaunch = zi - 1;
    c->zLaunch = c->ze[zi - 1] + (t - fl) * (c->ze[zi] - c->ze[zi - 1]);
  }
  if (c->srcKind != 0) c->tuned = false;
  c->srcKind = 0;
  c->solarKind = kind;
  c->haveSource = true;
  return 0;
}

// -abs(solarMu) and the azimuth in degrees -> launch direction cosines (:95-96, then makeDirectionCosines :1876-1894)
static void set_solar_direction(mcbrat_ctx *c, float solarMu, float solarAzimuthDeg) {
  const float mu = -std::fabs(solarMu);
  const float phi = (solarAzimuthDeg * std::acos(-1.0f)) / 180.0f;
  const float sinTheta = std::sqrt(1.0f - mu * mu);
  c->dir0[0] = sinTheta * std::cos(phi); c->dir0[1] = sinTheta * std::sin(phi); c->dir0[2] = mu;
}

int mcbrat_set_source_solar(mcbrat_ctx *c, float solarMu, float solarAzimuthDeg) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "setIllumination: domain hasn't been initialized.");
  if (solarAzimuthDeg < 0.f || solarAzimuthDeg > 360.f) return fail(c, "setIllumination: solarAzimuth out of bounds");
  if (std::fabs(solarMu) > 1.f || std::fabs(solarMu) <= FLT_MIN) return fail(c, "setIllumination: solarMu out of bounds");
  set_solar_direction(c, solarMu, solarAzimuthDeg);  // newPhotonStream_Directional, monteCarloIllumination.f95:93-96
  return set_solar_launch(c, 0);
}

int mcbrat_set_source_random_azimuth(mcbrat_ctx *c, float solarMu) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "setIllumination: domain hasn't been initialized.");
  if (std::fabs(solarMu) > 1.f || std::fabs(solarMu) <= FLT_MIN) return fail(c, "setIllumination: solarMu out of bounds");
  // newPhotonStream_RandomAzimuth :103-140: mu = -abs(solarMu); the azimuth is drawn per photon (solar_launch)
  c->dir0[0] = 0.f; c->dir0[1] = 0.f; c->dir0[2] = -std::fabs(solarMu);
  return set_solar_launch(c, 1);
}

int mcbrat_set_source_flux(mcbrat_ctx *c) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "setIllumination: domain hasn't been initialized.");
  // newPhotonStream_Flux :142-176: mu and the azimuth are drawn per photon (solar_launch)
  c->dir0[0] = 0.f; c->dir0[1] = 0.f; c->dir0[2] = -1.f;
  return set_solar_launch(c, 2);
}

int mcbrat_set_source_spotlight(mcbrat_ctx *c, float solarMu, float solarAzimuthDeg, float solarX, float solarY) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "setIllumination: domain hasn't been initialized.");
  if (solarAzimuthDeg < 0.f || solarAzimuthDeg > 360.f) return fail(c, "setIllumination: solarAzimuth out of bounds");
  if (std::fabs(solarMu) > 1.f || std::fabs(solarMu) <= FLT_MIN) return fail(c, "setIllumination: solarMu out of bounds");
  // :193-195 tests abs(solarX), abs(solarY) in (0, 1]; a negative fraction would launch outside the domain, so it is refused too
  if (!(solarX > 0.f && solarX <= 1.f && solarY > 0.f && solarY <= 1.f))
    return fail(c, "setIllumination: x and y positions must be between 0 and 1");
  set_solar_direction(c, solarMu, solarAzimuthDeg);  // newPhotonStream_Spotlight :178-216
  c->spotX = (double)solarX; c->spotY = (double)solarY;  // (real(8) = real)
  return set_solar_launch(c, 3);
}

int mcbrat_set_source_emission(mcbrat_ctx *c, const double *voxelWeights, double fracAtmsPower) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "setIllumination: domain hasn't been initialized.");
  if (!voxelWeights || !(fracAtmsPower >= 0.0 && fracAtmsPower <= 1.0)) return fail(c, "setIllumination: invalid emission weights.");
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  if (upload(c, &c->dVoxelCDF, voxelWeights, (size_t)c->nx * c->ny * c->nz)) return 1;
  c->fracAtms = fracAtmsPower;
  if (c->srcKind != 1) c->tuned = false;
  c->srcKind = 1;
  c->haveSource = true;
  return 0;
}

int64_t mcbrat_moments_length(const mcbrat_ctx *c) { return c && c->haveGrid ? tally_layout(c).momentsLen : 0; }

int mcbrat_bind_moments(mcbrat_ctx *c, double *deviceBuffer) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "bind_moments: set the grid first.");
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  if (deviceBuffer) c->dMoments = deviceBuffer;
  else { c->dMoments = c->dMomentsOwned.get(); return ensure_moments(c); }
  return 0;
}

int mcbrat_reset_moments(mcbrat_ctx *c) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "reset_moments: set the grid first.");
  (void)hipSetDevice(c->device);
  if (ensure_moments(c)) return 1;
  // c->cur is the lane of the latest call: its stream already orders this after every earlier finish chain
  if (c->externalPending) { HIP_OK(c, hipStreamWaitEvent(c->L().stream, c->evExternal, 0)); c->externalPending = false; }
  if (c->chainAfter) {
    if (c->chainSnapshot) HIP_OK(c, hipStreamWaitEvent(c->L().stream, c->chainSnapshot, 0));
    c->chainAfter = false; c->chainSnapshot = nullptr;
  }
  HIP_OK(c, hipMemsetAsync(c->dMoments, 0, sizeof(double) * (8 + 2 * (size_t)tally_layout(c).momentsLen), c->L().stream));
  // stream-ordered before whatever the context enqueues next; readers synchronise (get_moments, report_results)
  HIP_OK(c, hipEventRecord(c->L().evDone, c->L().stream));
  c->lastDone = c->L().evDone;
  return 0;
}

int mcbrat_get_moments(mcbrat_ctx *c, double *host) {
  if (!c || !host) return 1;
  (void)hipSetDevice(c->device);
  if (ensure_moments(c)) return 1;
  if (sync_all(c)) return 1;
  HIP_OK(c, hipMemcpy(host, c->dMoments, sizeof(double) * (8 + 2 * (size_t)tally_layout(c).momentsLen), hipMemcpyDeviceToHost));
  return 0;
}

int mcbrat_enable_counters(mcbrat_ctx *c, int32_t enable) {
  if (!c) return 1;
  Asked a = asked(c);
  a.debug = enable != 0;
  REFUSE(c, a, SetCounters);
  c->countersOn = enable != 0;
  return 0;
}
int mcbrat_get_counters(mcbrat_ctx *c, mcbrat_counters *out) {
  if (!c || !out) return 1;
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;  // (asynchronous mode: badPhotons is read when the enqueued work has finished)
  *out = c->lastCounters;
  return 0;
}
float mcbrat_last_trace_ms(const mcbrat_ctx *c) { return c ? c->lastTraceMs : 0.f; }

int mcbrat_set_forward_table(mcbrat_ctx *c, int32_t component, int32_t nAngles, int32_t nEntries, const float *table,
                             const float *origTable) {
  if (!c) return 1;
  if (!c->haveOptics) return fail(c, "tabulateForwardPhaseFunctions: domain has no optical components yet.");
  if (component < 1 || component > c->nc) return fail(c, "tabulatePhaseFunctions: failed on component" + std::to_string(component));
  if (nAngles < 2 || nEntries < 1 || !table) return fail(c, "tabulateForwardPhaseFunctions: table has the wrong number of entries");
  c->fwd.resize(c->nc); c->fwdOrig.resize(c->nc); c->fwdNAngles.resize(c->nc, 0); c->fwdNEntries.resize(c->nc, 0);
  c->fwd[component - 1].assign(table, table + (size_t)nAngles * nEntries);
  const float *o = origTable ? origTable : table;
  c->fwdOrig[component - 1].assign(o, o + (size_t)nAngles * nEntries);
  c->fwdNAngles[component - 1] = nAngles;
  c->fwdNEntries[component - 1] = nEntries;
  c->fwdDirty = true;
  return 0;
}

int mcbrat_specify_intensity(mcbrat_ctx *c, int32_t nDirections, const float *mus, const float *phisDeg,
                             int32_t useRussianRouletteForIntensity, float zetaMin,
                             int32_t useHybridPhaseFunsForIntenCalcs, int32_t numOrdersOrigPhaseFunIntenCalcs,
                             int32_t limitIntensityContributions, float maxIntensityContribution) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "specifyParameters: set the grid first.");
  if (nDirections < 0 || nDirections > MCBRAT_MAX_DIRECTIONS || (nDirections > 0 && (!mus || !phisDeg)))
    return fail(c, "specifyParameters: invalid number of intensity directions.");
  for (int i = 0; i < nDirections; ++i) {  // specifyParameters :1140-1145
    if (mus[i] < -1.f || mus[i] > 1.f) return fail(c, "specifyParameters: intensityMus must be between -1 and 1");
    if (std::fabs(mus[i]) < FLT_MIN) return fail(c, "specifyParameters: intensityMus can't be 0 (directly sideways)");
    if (phisDeg[i] < 0.f || phisDeg[i] > 360.f) return fail(c, "specifyParameters: intensityPhis must be between 0 and 360");
  }
  if (limitIntensityContributions && !(maxIntensityContribution > 0.f))
    return fail(c, "specifyParameters: maxIntensityContribution must be > 0");
  if (zetaMin < 0.f) return fail(c, "specifyParameters: zetaMin must be >= 0.");
  Asked a = asked(c);
  a.nDir = nDirections; a.limitContrib = limitIntensityContributions != 0;
  REFUSE(c, a, SetIntensity);
  if (numOrdersOrigPhaseFunIntenCalcs < 0) return fail(c, "specifyParameters: numOrdersOrigPhaseFunIntenCalcs must be >= 0");
  if (useRussianRouletteForIntensity)
    for (int i = 0; i < nDirections; ++i)
      if (mus[i] < 0.f)
        return fail(c, "specifyParameters: useRussianRouletteForIntensity only works for upward directions "
                       "(the reference restarts the walk below the surface for mu < 0).");
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  constexpr float kPi = 3.14159265358979312f;
  c->dirData.assign((size_t)8 * std::max(nDirections, 1), 0.f);
  for (int i = 0; i < nDirections; ++i) {  // makeDirectionCosines(mu, phi * Pi/180) :1270-1272, :1876-1894
    const float mu = mus[i], phi = phisDeg[i] * kPi / 180.0f;
    const float sinTheta = std::sqrt(1.0f - mu * mu);
    float *d = &c->dirData[(size_t)8 * i];
    d[0] = sinTheta * std::cos(phi); d[1] = sinTheta * std::sin(phi); d[2] = mu;
    d[3] = (4.0f * kPi) * std::fabs(d[2]);
    for (int a = 0; a < 3; ++a) d[4 + a] = std::fabs(d[a]) >= 2.0f * FLT_MIN ? 1.0f / d[a] : 0.0f;
  }
  const int limit = (limitIntensityContributions && maxIntensityContribution < FLT_MAX) ? 1 : 0;
  c->limitContrib = limit;  // (the batch slabs change length: the next call compares element counts)
  c->maxContrib = maxIntensityContribution;
  if (nDirections != c->nDir) drop_results(c, true);  // the moment arrays change length: start them afresh
  c->nDir = nDirections;
  c->useRRIntensity = useRussianRouletteForIntensity ? 1 : 0;
  c->zetaMin = zetaMin;
  c->useHybrid = useHybridPhaseFunsForIntenCalcs ? 1 : 0;
  c->numOrdersOrig = numOrdersOrigPhaseFunIntenCalcs;
  c->fwdDirty = true;
  return 0;
}

// What the setters below, mcbrat_specify_intensity and mcbrat_set_surface_brdf would refuse these settings with, asked in one
// question and without a change: host arithmetic on the context's grid, components, counters and source.  (LevelsOff is not
// asked: its two rules stand under SetDirect and SetSide too.)
const char *mcbrat_settings_refusal(const mcbrat_ctx *c, int32_t nDirections, int32_t limitIntensityContributions, int32_t numRecScatOrd,
                                    int32_t levelFluxes, int32_t directLevelFluxes, int32_t actinicFlux, int32_t sideFluxes, int32_t brdfSurface) {
  if (!c) return mcbrat_last_error(c);
  if (!c->haveGrid) return "specifyParameters: set the grid first.";
  Asked a = asked(c);
  a.nDir = nDirections; a.limitContrib = limitIntensityContributions != 0; a.numRecScatOrd = numRecScatOrd < 0 ? -1 : numRecScatOrd;
  a.levels = levelFluxes != 0; a.direct = directLevelFluxes != 0; a.actinic = actinicFlux != 0; a.side = sideFluxes != 0; a.brdf = brdfSurface != 0;
  return refusal(settings_of(c, a), (Stage)(SetIntensity | SetOrders | SetLevels | SetDirect | SetActinic | SetSide | SetBrdf));
}

// The five recording setters: the setting as the context holds it and as refusal() is asked about it, its new value, the stage
// asked when it switches on and when it switches off (0: nothing to ask), and whether another walk or other kernels go with it.
static int specify_recording(mcbrat_ctx *c, int mcbrat_ctx::*held, int Asked::*about, int value, bool on, unsigned onStage, unsigned offStage, bool retune) {
  if (!c) return 1;
  if (!c->haveGrid) return fail(c, "specifyParameters: set the grid first.");
  Asked a = asked(c);
  a.*about = value;
  REFUSE(c, a, (Stage)(on ? onStage : offStage));
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  const TallyShape before = tally_shape(c);
  c->*held = value;
  if (!(tally_shape(c) == before)) drop_results(c, retune);  // the moment arrays change length: start them afresh
  return 0;
}

// (the slab of one batch must fit the tally budget; mcbrat_compute_radiative_transfer checks again, directions may change)
int mcbrat_specify_scattering_orders(mcbrat_ctx *c, int32_t numRecScatOrd) {
  return specify_recording(c, &mcbrat_ctx::numRecScatOrd, &Asked::numRecScatOrd, numRecScatOrd < 0 ? -1 : numRecScatOrd, numRecScatOrd >= 0, SetOrders, 0, false);
}

int mcbrat_report_scattering_orders(mcbrat_ctx *c, float *meanFluxUpByScatOrd, float *meanFluxDownByScatOrd, float *fluxUpByScatOrd,
                                    float *fluxDownByScatOrd, float *meanIntensityByScatOrd, float *intensityByScatOrd) {
  if (!c) return 1;
  if (!orders_on(c)) return fail(c, "reportResults: scattering-order information not available");
  if ((meanIntensityByScatOrd || intensityByScatOrd) && c->nDir == 0)
    return fail(c, "reportResults: intensityByScatOrd information not available");
  const size_t ncol = (size_t)c->nx * c->ny, nOrd = (size_t)c->numRecScatOrd + 1, nDir = (size_t)c->nDir;
  return deal_last(c, (size_t)tally_layout(c).momOrders, {{meanFluxUpByScatOrd, nOrd}, {meanFluxDownByScatOrd, nOrd}, {fluxUpByScatOrd, ncol * nOrd},
                   {fluxDownByScatOrd, ncol * nOrd}, {meanIntensityByScatOrd, nDir * nOrd}, {intensityByScatOrd, ncol * nDir * nOrd}});
}

// (off: switch the direct and the side tally off first)
int mcbrat_specify_level_fluxes(mcbrat_ctx *c, int32_t enable) {
  return specify_recording(c, &mcbrat_ctx::levelFluxes, &Asked::levels, enable ? 1 : 0, enable != 0, SetLevels, LevelsOff, true);
}

int mcbrat_report_level_fluxes(mcbrat_ctx *c, float *meanLevelFluxUp, float *meanLevelFluxDown, float *levelFluxUp, float *levelFluxDown) {
  if (!c) return 1;
  if (!levels_on(c)) return fail(c, "reportResults: level-flux information not available");
  const size_t ncol = (size_t)c->nx * c->ny, nLvl = (size_t)c->nz + 1;  // (the arrays are (nx, ny, 0:nz))
  return deal_last(c, (size_t)tally_layout(c).momLevels, {{meanLevelFluxUp, nLvl}, {meanLevelFluxDown, nLvl}, {levelFluxUp, ncol * nLvl}, {levelFluxDown, ncol * nLvl}});
}

// (what level fluxes are refused with is refused with them: the setting needs them)
int mcbrat_specify_direct_level_fluxes(mcbrat_ctx *c, int32_t enable) {
  return specify_recording(c, &mcbrat_ctx::directLevelFluxes, &Asked::direct, enable ? 1 : 0, enable != 0, SetDirect, 0, true);
}

int mcbrat_report_direct_level_fluxes(mcbrat_ctx *c, float *meanLevelFluxDownDirect, float *meanLevelFluxDownDiffuse, float *levelFluxDownDirect,
                                      float *levelFluxDownDiffuse) {
  if (!c) return 1;
  if (!direct_on(c)) return fail(c, "reportResults: direct level-flux information not available");
  const size_t ncol = (size_t)c->nx * c->ny, nLvl = (size_t)c->nz + 1;
  return deal_last(c, (size_t)tally_layout(c).momDirect, {{meanLevelFluxDownDirect, nLvl}, {meanLevelFluxDownDiffuse, nLvl}, {levelFluxDownDirect, ncol * nLvl},
                   {levelFluxDownDiffuse, ncol * nLvl}});
}

// (level fluxes may be on together with it; their direct tally may not: no kernel has both flags)
int mcbrat_specify_actinic_flux(mcbrat_ctx *c, int32_t enable) {
  return specify_recording(c, &mcbrat_ctx::actinicFlux, &Asked::actinic, enable ? 1 : 0, enable != 0, SetActinic, 0, true);
}

int mcbrat_report_actinic_flux(mcbrat_ctx *c, float *meanActinicFlux, float *actinicFlux) {
  if (!c) return 1;
  if (!actinic_on(c)) return fail(c, "reportResults: actinic-flux information not available");
  return deal_last(c, (size_t)tally_layout(c).momActinic, {{meanActinicFlux, (size_t)c->nz}, {actinicFlux, (size_t)c->nx * c->ny * (size_t)c->nz}});
}

// (what level fluxes are refused with is refused with them: the setting needs them)
int mcbrat_specify_side_fluxes(mcbrat_ctx *c, int32_t enable) {
  return specify_recording(c, &mcbrat_ctx::sideFluxes, &Asked::side, enable ? 1 : 0, enable != 0, SetSide, 0, true);
}

int mcbrat_report_side_fluxes(mcbrat_ctx *c, float *meanSideFluxes, float *sideFluxes) {
  if (!c) return 1;
  if (!side_on(c)) return fail(c, "reportResults: side-flux information not available");
  return deal_last(c, (size_t)tally_layout(c).momSide, {{meanSideFluxes, 4 * (size_t)c->nz}, {sideFluxes, 4 * (size_t)c->nx * c->ny * (size_t)c->nz}});
}

int mcbrat_report_intensity(mcbrat_ctx *c, float *meanIntensity, float *intensity) {
  if (!c) return 1;
  if (c->nDir == 0) return fail(c, "reportResults: intensity information not available");
  const size_t ncol = (size_t)c->nx * c->ny;
  std::vector<float> h(ncol * c->nDir);
  if (read_last(c, (size_t)tally_layout(c).momIntensity, h)) return 1;
  if (intensity) std::memcpy(intensity, h.data(), sizeof(float) * h.size());
  if (meanIntensity)
    for (int d = 0; d < c->nDir; ++d) {  // reportResults :980-992
      float s = 0.f;
      for (size_t i = 0; i < ncol; ++i) s += h[(size_t)d * ncol + i];
      meanIntensity[d] = s / (float)ncol;
    }
  return 0;
}

int mcbrat_get_event_threshold(const mcbrat_ctx *c) { return c ? c->eventThreshold : 0; }

int mcbrat_set_async(mcbrat_ctx *c, int32_t enable) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  c->asyncOn = enable != 0;
  c->cur = 0; c->nextLane = 0;
  if (c->asyncOn)  // (every stream now: the first asynchronous call sizes all of them at once -- allocation synchronises the device)
    for (int i = 0; i < mcbrat_ctx::kLanes; ++i)
      if (init_lane(c, i)) return 1;
  return 0;
}

int mcbrat_synchronize(mcbrat_ctx *c) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  return sync_all(c);
}

int mcbrat_stream_wait_done(mcbrat_ctx *c, void *stream) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  if (c->lastDone) HIP_OK(c, hipStreamWaitEvent((hipStream_t)stream, c->lastDone, 0));
  return 0;
}

int mcbrat_wait_stream(mcbrat_ctx *c, void *stream) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  HIP_OK(c, hipEventRecord(c->evExternal, (hipStream_t)stream));
  c->externalPending = true;
  return 0;
}

int mcbrat_chain_after(mcbrat_ctx *c, mcbrat_ctx *previous) {
  if (!c || !previous) return 1;
  if (c == previous) return fail(c, "chain_after: a context follows its own calls by itself.");
  if (c->device != previous->device) return fail(c, "chain_after: the two contexts are on different devices.");
  (void)hipSetDevice(c->device);
  c->chainAfter = false; c->chainSnapshot = nullptr;
  if (!previous->lastDone) return 0;  // (nothing enqueued there yet: nothing to follow)
  // "so far" is fixed NOW: an event of this context on the stream of `previous`'s latest call, whose finish chain follows all
  // of its earlier ones.  `previous` may be destroyed or re-used afterwards; what is waited for does not change.
  if (!c->evChain) HIP_OK(c, hipEventCreateWithFlags(&c->evChain, hipEventDisableTiming));
  HIP_OK(c, hipEventRecord(c->evChain, previous->L().stream));
  c->chainAfter = true;
  c->chainSnapshot = c->evChain;
  return 0;
}

int mcbrat_set_tuning(mcbrat_ctx *c, int32_t blocksPerCU, int32_t eventThreshold, int32_t maxBatchesInFlight,
                      int32_t privateTallies, int32_t blockSize, int32_t launchThreshold, int32_t surfaceThreshold,
                      int32_t brickLayout) {
  if (!c) return 1;
  if (blocksPerCU >= 0) c->blocksPerCU = blocksPerCU;
  if (eventThreshold > 0) { c->eventThreshold = eventThreshold; c->autoTune = false; }
  if (eventThreshold == 0) { c->autoTune = true; c->tuned = false; }
  if (maxBatchesInFlight >= 0) c->maxBatchesInFlight = maxBatchesInFlight;
  // privateTallies: 0 global atomics; 1 the library's plan; 2 private tallies without the optical grid in LDS; 3 as 1 without the
  // wide plan (a slab too large for a shared compute unit then tallies with global atomics); 4 the wide plan (one workgroup
  // of 1024 lanes per compute unit) even where the shared plan would do; 5 as 4 with the per-cell optics left in global memory;
  // 6 as 4 without the per-cell optics in LDS: per block in LDS where every block is uniform in them, else as 5
  if (privateTallies >= 0) {
    if (privateTallies > 6) return fail(c, "set_tuning: privateTallies must be 0 ... 6");
    c->privMode = privateTallies ? 1 : 0;
    c->gridLdsMode = privateTallies == 2 ? 0 : (privateTallies == 5 ? 2 : (privateTallies == 6 ? 3 : 1));
    c->wideMode = privateTallies == 3 ? 0 : (privateTallies >= 4 ? 2 : c->wideDefault);
    c->tuned = false;
  }
  if (blockSize == 0 || blockSize == 256 || blockSize == 512 || blockSize == 768) c->blockSize = blockSize;
  else if (blockSize > 0) return fail(c, "set_tuning: blockSize must be 0, 256, 512 or 768");
  if (launchThreshold > 0) { c->launchThreshold = launchThreshold; c->launchThresholdSet = true; }
  if (surfaceThreshold > 0) { c->surfaceThreshold = surfaceThreshold; c->surfaceThresholdSet = true; }
  if (brickLayout >= 0 && brickLayout <= 2) { if (brickLayout != c->brickMode) c->tuned = false; c->brickMode = brickLayout; }
  return 0;
}

const char *mcbrat_first_drop(mcbrat_ctx *c) {
  if (!c) return "";
  (void)hipSetDevice(c->device);
  c->dropText.clear();
  unsigned long long h[kBadWords] = {0};
  if (sync_all(c) || hipMemcpy(h, c->dBad.get(), sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return c->dropText.c_str();
  if (h[0] == 0ull) return c->dropText.c_str();
  static const char *kinds[] = {"?", "leg budget (maxEvents)", "leg budget of a photon with a NaN direction at full weight (maxEventsNaN)", "wave watchdog (no lane made progress)",
                                "block crossings of one leg", "horizontal leg through vacuum in a block that spans both periodic axes", "view ray longer than the geometry allows"};
  char buf[768];
  int at = snprintf(buf, sizeof(buf), "%llu dropped; bounds that fired:", h[0]);
  for (unsigned k = 1; k < 7; ++k)
    if ((h[7] >> (k - 1)) & 1ull) at += snprintf(buf + at, sizeof(buf) - (size_t)at, " [%s]", kinds[k]);
  if (h[1] != 0ull) {  // (the instrumented instantiations also record the first one)
    const unsigned kind = (unsigned)(h[2] & 0xffu), kernel = (unsigned)((h[2] >> 8) & 0xffu), state = (unsigned)((h[2] >> 16) & 0xffffu);
    snprintf(buf + at, sizeof(buf) - (size_t)at, "; first recorded: %s in %s, photon id %llu, %s %u, leg %u", kind < 7 ? kinds[kind] : "?",
             kernel == 2 ? "trace_block_kernel" : "trace_kernel", h[3], kind == DROP_RAY ? "view direction" : "state", state, (unsigned)(h[2] >> 32));
  } else {
    snprintf(buf + at, sizeof(buf) - (size_t)at, "; no photon record (production kernels keep none: trace the same photons with mcbrat_trace_fates)");
  }
  c->dropText = buf;
  return c->dropText.c_str();
}

int mcbrat_set_option(mcbrat_ctx *c, const char *name, int32_t value) {
  if (!c) return 1;
  if (!name) return fail(c, "set_option: no option name");
  const std::string n(name);
  if (n == "jumpThreshold") c->jumpThreshold = std::max(1, std::min(64, (int)value));
  else if (n == "crossThreshold") c->crossThreshold = std::max(1, std::min(64, (int)value));
  else if (n == "batchUnits") c->batchUnits = value != 0;
  else if (n == "blockSpanKernel") c->blockSpanKernel = value != 0;
  else if (n == "blockRareKernel") c->blockRareKernel = value != 0;
  else if (n == "glintSampling") c->glintSampling = value != 0;
  else if (n == "cameraGridInLds") c->cameraGridInLds = std::max(-1, std::min(1, (int)value));
  else if (n == "cameraPathBinsInLds") c->cameraPathBinsInLds = value != 0;
  else return fail(c, "set_option: unknown option '" + n + "'");
  return 0;
}

int mcbrat_set_surface_description(mcbrat_ctx *c, int32_t numX, int32_t numY, const double *xPosition, const double *yPosition,
                                   const float *reflectance) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  if (numX <= 0 || numY <= 0) { c->surfNumX = c->surfNumY = 0; return 0; }  // back to the domain's albedo
  // the checks of newSurfaceDescriptionXY, src/surfaceProperties.f95:66-82
  if (numX < 2 || numY < 2 || !xPosition || !yPosition || !reflectance)
    return fail(c, "new_SurfaceDescription: position vector(s) are incorrect length.");
  for (int i = 1; i < numX; ++i) if (!(xPosition[i] - xPosition[i - 1] > 0.)) return fail(c, "new_SurfaceDescription: positions must be unique, increasing.");
  for (int i = 1; i < numY; ++i) if (!(yPosition[i] - yPosition[i - 1] > 0.)) return fail(c, "new_SurfaceDescription: positions must be unique, increasing.");
  for (size_t i = 0; i < (size_t)(numX - 1) * (numY - 1); ++i)
    if (!(reflectance[i] >= 0.f && reflectance[i] <= 1.f)) return fail(c, "new_SurfaceDescription: surface reflectance must be between 0 and 1");
  if (upload(c, &c->dSurfX, xPosition, (size_t)numX) || upload(c, &c->dSurfY, yPosition, (size_t)numY) ||
      upload(c, &c->dSurfRefl, reflectance, (size_t)(numX - 1) * (numY - 1)))
    return 1;
  c->surfNumX = numX; c->surfNumY = numY;
  c->surfKind = 0;
  return 0;
}

int mcbrat_set_surface_brdf(mcbrat_ctx *c, int32_t kind, int32_t numX, int32_t numY, const double *xPosition, const double *yPosition,
                            int32_t nParams, const float *params) {
  if (!c) return 1;
  if (kind == 0) {  // Lambertian: the surface description as it was
    if (numX > 0 && numY > 0 && nParams != 1) return fail(c, "new_SurfaceDescription: Wrong number of parameters supplied for surface BRDF.");
    return mcbrat_set_surface_description(c, numX, numY, xPosition, yPosition, params);
  }
  (void)hipSetDevice(c->device);
  if (sync_all(c)) return 1;
  if (numX <= 0 || numY <= 0) { c->surfNumX = c->surfNumY = 0; c->surfKind = 0; return 0; }  // back to the domain's albedo
  if (brdf_num_params(kind) == 0 || kind == BRDF_LAMBERTIAN) return fail(c, "new_SurfaceDescription: unknown surface BRDF model.");
  Asked a = asked(c);
  a.brdf = true;
  REFUSE(c, a, SetBrdf);
  if (nParams != brdf_num_params(kind)) return fail(c, "new_SurfaceDescription: Wrong number of parameters supplied for surface BRDF.");
  if (numX < 2 || numY < 2 || !xPosition || !yPosition || !params)
    return fail(c, "new_SurfaceDescription: position vector(s) are incorrect length.");
  for (int i = 1; i < numX; ++i) if (!(xPosition[i] - xPosition[i - 1] > 0.)) return fail(c, "new_SurfaceDescription: positions must be unique, increasing.");
  for (int i = 1; i < numY; ++i) if (!(yPosition[i] - yPosition[i - 1] > 0.)) return fail(c, "new_SurfaceDescription: positions must be unique, increasing.");
  const size_t nPatch = (size_t)(numX - 1) * (numY - 1);
  std::vector<float4> q(nPatch);
  std::vector<std::array<float, 4>> seen;  // the parameter checks and the energy rule, once per distinct parameter vector
  for (size_t i = 0; i < nPatch; ++i) {
    std::array<float, 4> v = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < nParams; ++k) v[(size_t)k] = params[(size_t)k * nPatch + i];  // [nParams][numY-1][numX-1]
    q[i] = make_float4(v[0], v[1], v[2], v[3]);
    if (std::find(seen.begin(), seen.end(), v) != seen.end()) continue;
    if (const char *err = brdf_param_error(kind, v.data())) return fail(c, err);
    seen.push_back(v);
  }
  if (upload(c, &c->dSurfX, xPosition, (size_t)numX) || upload(c, &c->dSurfY, yPosition, (size_t)numY) || upload(c, &c->dSurfBrdf, q.data(), nPatch))
    return 1;
  c->surfNumX = numX; c->surfNumY = numY;
  c->surfKind = kind;
  return 0;
}

int mcbrat_set_walk_options(mcbrat_ctx *c, int32_t layerSkip, int32_t blockWalk) {
  if (!c) return 1;
  if (layerSkip >= 0) { if (layerSkip != c->layerSkip) c->tuned = false; c->layerSkip = layerSkip > 3 ? 1 : layerSkip; }
  if (blockWalk >= 0) { if (blockWalk != c->blockWalk) c->tuned = false; c->blockWalk = std::min(blockWalk, 2); }
  return 0;
}

double *mcbrat_moments_device_pointer(mcbrat_ctx *c) {
  if (!c || !c->haveGrid) return nullptr;
  (void)hipSetDevice(c->device);
  if (ensure_moments(c)) return nullptr;
  return c->dMoments;
}

int mcbrat_frequency_distribution(mcbrat_ctx *c, uint64_t seed, uint64_t firstDraw, int32_t numLambda, const double *cdf,
                                  int64_t totalPhotons, int64_t *distribution) {
  if (!c) return 1;
  if (numLambda < 1 || !cdf || !distribution || totalPhotons < 0) return fail(c, "getFrequencyDistr: invalid arguments.");
  for (int i = 1; i < numLambda; ++i)
    if (!(cdf[i] >= cdf[i - 1])) return fail(c, "getFrequencyDistr: the power CDF must not decrease.");
  (void)hipSetDevice(c->device);
  if (init_lane(c, 0)) return 1;
  hipStream_t st = c->lane[0].stream;
  const size_t nl = (size_t)numLambda;
  if (c->dFreqCdf.capacity() < nl || c->dFreqCounts.capacity() < nl) {  // the context's own buffers, grown when a longer CDF arrives
    HIP_OK(c, hipStreamSynchronize(st));
    HIP_OK(c, c->dFreqCdf.reserve(nl));
    HIP_OK(c, c->dFreqCounts.reserve(nl));
  }
  double *dCdf = c->dFreqCdf.get();
  unsigned long long *dCounts = c->dFreqCounts.get();
  HIP_OK(c, hipMemcpyAsync(dCdf, cdf, sizeof(double) * numLambda, hipMemcpyHostToDevice, st));
  HIP_OK(c, hipMemsetAsync(dCounts, 0, sizeof(unsigned long long) * numLambda, st));
  if (totalPhotons > 0) {
    const unsigned long long blocks4 = ((unsigned long long)totalPhotons + 3) / 4 + 1;
    const unsigned grid = (unsigned)std::min<unsigned long long>((blocks4 + 255) / 256, (unsigned long long)c->numCUs * 8);
    const size_t lds = numLambda <= 8192 ? sizeof(unsigned) * (size_t)numLambda : 0;
    hipLaunchKernelGGL(frequency_distribution_kernel, dim3(std::max(1u, grid)), dim3(256), lds, st, dCdf, numLambda,
                       (unsigned long long)totalPhotons, (unsigned long long)firstDraw, (uint32_t)seed, (uint32_t)(seed >> 32), dCounts);
    HIP_OK(c, hipGetLastError());
  }
  std::vector<unsigned long long> h(numLambda);
  HIP_OK(c, hipMemcpyAsync(h.data(), dCounts, sizeof(unsigned long long) * numLambda, hipMemcpyDeviceToHost, st));
  HIP_OK(c, hipStreamSynchronize(st));
  for (int i = 0; i < numLambda; ++i) distribution[i] = (int64_t)h[i];
  return 0;
}

int mcbrat_philox4x32_10(mcbrat_ctx *c, int32_t n, const uint32_t *in, uint32_t *out) {
  if (!c) return 1;
  if (n < 0 || (n > 0 && (!in || !out))) return fail(c, "philox4x32_10: invalid arguments.");
  if (n == 0) return 0;
  (void)hipSetDevice(c->device);
  if (init_lane(c, 0)) return 1;
  hipStream_t st = c->lane[0].stream;
  DeviceBuffer<uint32_t> dIn, dOut;
  HIP_OK(c, dIn.allocate(6 * (size_t)n));
  HIP_OK(c, dOut.allocate(4 * (size_t)n));
  HIP_OK(c, hipMemcpyAsync(dIn.get(), in, sizeof(uint32_t) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dIn.get(), (int)n, dOut.get());
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpyAsync(out, dOut.get(), sizeof(uint32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(c, hipStreamSynchronize(st));
  return 0;
}

int64_t mcbrat_live_device_allocations(void) { return (int64_t)liveDeviceAllocations.load(); }

int mcbrat_get_walk_mode(const mcbrat_ctx *c) {
  if (!c) return 0;
  int m = (c->layerSkip ? 1 : 0) | (c->blockWalk ? 2 : 0);
  if (c->haveGrid && c->haveOptics) {  // what a flux launch of the loaded domain would do (the plan decides, as launch_trace does)
    // (the flux run's slab: with scattering orders its order bins too, so that private tallies give way where they no longer fit)
    const LaunchPlan L = plan_launch(c, (size_t)tally_layout(flux_run(tally_shape(c))).slabStride);
    m = ((c->layerSkip && !facewalk_on(c)) ? 1 : 0) | (block_walk_applies(c, L) ? 2 : 0) | (L.fly ? 4 : 0) | (c->blockWalk ? 8 : 0) |
        (L.wide ? 16 : 0) | ((L.blockLite && L.optics == 1) ? 32 : 0) | (L.priv ? 64 : 0) | ((L.blockLite && L.optics == 2) ? 128 : 0) |
        (L.cdfTop ? 256 : 0);
    // (a NOSPAN instantiation: the near-uniform flags have no say in that)
    if (block_walk_applies(c, L)) {
      const BlockVariant v = pick_block(L, false, c->srcKind != 0, block_walk_of(c, false, false));
      m |= (v.nospan ? 512 : 0) | (v.rare != 0 ? 1024 : 0);  // (1024: RARE, a black surface and the parallel sun compiled in)
    }
  }
  return m;
}

int mcbrat_compute_radiative_transfer(mcbrat_ctx *c, uint64_t seed, uint64_t firstPhotonId, int64_t ppb, int32_t nBatches,
                                      int64_t *numPhotonsProcessed) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  if (check_ready(c)) return 1;
  if (ppb < 1 || nBatches < 1) return fail(c, "computeRadiativeTransfer: Didn't process any photons.");
  // the capacity of the tallies: a bin holds less than 2^31 unit weights (2^63 in 2^-32 units)
  if (ppb > kMaxPhotonsPerBatch)
    return fail(c, "computeRadiativeTransfer: numPhotonsPerBatch is too large: at most 2^31 - 1 photons per batch fit the tallies.");
  if (ensure_moments(c)) return 1;
  // the trial launches that choose the event threshold run synchronously, once, on the first call large enough
  const bool tuneNow = c->autoTune && !c->tuned && (unsigned long long)ppb * (unsigned long long)nBatches >= c->tuneTrialPhotons;
  const bool async = c->asyncOn && !c->countersOn;
  if ((!async || tuneNow) && sync_all(c)) return 1;
  if (c->asyncOn) {  // rotate over the lanes
    c->cur = c->nextLane;
    c->nextLane = (c->nextLane + 1) % mcbrat_ctx::kLanes;
    if (init_lane(c, c->cur)) return 1;
  } else {
    c->cur = 0;
  }
  const size_t ncol = (size_t)c->nx * c->ny;
  const TallyLayout lay = tally_layout(c);
  const size_t slabStride = (size_t)lay.slabStride;
  REFUSE(c, asked(c), Trace);
  // batches in flight: bounded by a memory budget (slabs are 8 B per tally bin per batch)
  size_t inFlight = std::max<size_t>(1, kSlabBudget / (slabStride * sizeof(long long)));
  if (c->maxBatchesInFlight > 0) inFlight = std::min<size_t>(inFlight, (size_t)c->maxBatchesInFlight);
  inFlight = std::min<size_t>(inFlight, (size_t)nBatches);
  // asynchronous mode sizes every lane at once: allocation synchronises the device, so it must not recur
  for (int li = 0; li < mcbrat_ctx::kLanes; ++li) {
    mcbrat_ctx::Lane &L = c->lane[li];
    if (li != c->cur && !(c->asyncOn && L.stream)) continue;
    // (+ 1: the launch's photon cursor sits behind the slabs in use, zeroed with them)
    const size_t needSlab = slabStride * inFlight + 1, needCol = 3 * ncol * inFlight, needScal = (size_t)lay.scalPerBatch * inFlight;
    if (L.dSlabs.capacity() >= needSlab && L.dColVals.capacity() >= needCol && L.dScalVals.capacity() >= needScal) continue;
    HIP_OK(c, hipStreamSynchronize(L.stream));  // (before any of the three may free)
    HIP_OK(c, L.dSlabs.reserve(needSlab));
    HIP_OK(c, L.dColVals.reserve(needCol));
    HIP_OK(c, L.dScalVals.reserve(needScal));
  }
  if (!c->dLast) HIP_OK(c, c->dLast.allocate((size_t)tally_layout(c).momentsLen));

  DevParams p;
  fill_params(c, p);
  p.seedLo = (uint32_t)seed; p.seedHi = (uint32_t)(seed >> 32);
  p.slabs = c->L().dSlabs.get(); p.slabStride = slabStride;
  p.numRecScatOrd = c->numRecScatOrd;
  p.ppb = (unsigned long long)ppb;
  p.fates = nullptr;
  p.counters = c->countersOn ? c->dEventCounters.get() : nullptr;
  if (c->countersOn) HIP_OK(c, hipMemsetAsync(c->dEventCounters.get(), 0, 32 * sizeof(unsigned long long), c->L().stream));

  if (c->autoTune && !c->tuned) {
    if (autotune(c, p, (unsigned long long)ppb, (int)inFlight)) return 1;
    p.eventThreshold = c->eventThreshold;
  }

  float traceMs = 0.f;
  for (int b0 = 0; b0 < nBatches; b0 += (int)inFlight) {
    const int nb = std::min<int>((int)inFlight, nBatches - b0);
    p.total = (unsigned long long)ppb * (unsigned long long)nb;
    p.firstPhoton = firstPhotonId + (unsigned long long)b0 * (unsigned long long)ppb;
    HIP_OK(c, hipMemsetAsync(c->L().dSlabs.get(), 0, sizeof(long long) * (slabStride * nb + 1), c->L().stream));  // zero tallies :248-252, and the cursor
    p.counter = reinterpret_cast<unsigned long long *>(c->L().dSlabs.get() + slabStride * nb);
    std::pair<hipEvent_t, hipEvent_t> bracket(c->L().ev0, c->L().ev1);
    if (async && event_pair(c, bracket)) return 1;
    HIP_OK(c, hipEventRecord(bracket.first, c->L().stream));
    if (launch_trace(c, p, c->countersOn, nb)) return 1;
    HIP_OK(c, hipEventRecord(bracket.second, c->L().stream));
    if (async) c->timing.push_back(bracket);
    if (c->timing.size() > 1024) { if (sync_all(c)) return 1; }  // bound the number of live events
    // the finish kernels accumulate into one moment array: they run in call order across lanes, and after
    // whatever a caller's stream did to that array (mcbrat_wait_stream)
    if (c->lastDone && c->lastDone != c->L().evDone) HIP_OK(c, hipStreamWaitEvent(c->L().stream, c->lastDone, 0));
    if (c->externalPending) { HIP_OK(c, hipStreamWaitEvent(c->L().stream, c->evExternal, 0)); c->externalPending = false; }
    if (c->chainAfter) {  // contexts that share one moment array (one per wavelength): this finish chain after the other context's
      if (c->chainSnapshot) HIP_OK(c, hipStreamWaitEvent(c->L().stream, c->chainSnapshot, 0));
      c->chainAfter = false; c->chainSnapshot = nullptr;
    }
    FinishParams f;
    f.shape = tally_shape(c); f.nBatches = nb; f.xyRegular = c->xyRegular;
    f.ppb = p.ppb; f.total = p.total; f.lay = lay;
    f.parts = finish_parts(f.shape, nb);
    f.slabs = c->L().dSlabs.get(); f.relArea = c->dRelArea.get();
    f.xe = c->dEdges.get(); f.ye = f.xe + (c->nx + 1); f.ze = f.ye + (c->ny + 1);
    f.colVals = c->L().dColVals.get(); f.scalVals = c->L().dScalVals.get(); f.moments = c->dMoments; f.last = c->dLast.get();
    f.bad = c->dBad.get(); f.badHost = c->hBadDev;
    f.actUnit = actinic_unit(c);
    if (c->nDir > 0 && c->limitContrib)
      hipLaunchKernelGGL(finish_excess, dim3(c->nDir, nb), dim3(256), 0, c->L().stream, f);
    hipLaunchKernelGGL(finish_gather, dim3(f.parts.gatherGrid()), dim3(kFinishBlock), 0, c->L().stream, f);
    hipLaunchKernelGGL(finish_fold, dim3(f.parts.foldGrid()), dim3(kFinishBlock), 0, c->L().stream, f);  // (also hands the dropped-photon count to the host)
    HIP_OK(c, hipGetLastError());
    HIP_OK(c, hipEventRecord(c->L().evDone, c->L().stream));
    c->lastDone = c->L().evDone;
    if (async) continue;
    HIP_OK(c, hipStreamSynchronize(c->L().stream));
    float ms = 0.f;
    HIP_OK(c, hipEventElapsedTime(&ms, c->L().ev0, c->L().ev1));
    traceMs += ms;
  }
  if (!async) { c->lastTraceMs = traceMs; c->lastCounters.badPhotons = (int64_t)*c->hBad.get(); }
  if (c->countersOn) {
    unsigned long long h[16];
    HIP_OK(c, hipMemcpy(h, c->dEventCounters.get(), sizeof(h), hipMemcpyDeviceToHost));
#ifdef MCBRAT_STAMPS  // development aid: wave cycles per section of the tracing loop
    {
      unsigned long long st[16];
      HIP_OK(c, hipMemcpy(st, c->dEventCounters.get() + 16, sizeof(st), hipMemcpyDeviceToHost));
      const char *names[9] = {"launch", "block crossings (block walk)", "collideA(pos,optics,absorb,roulette)", "collideB(angle,cos)", "collideC(next_direct)",
                              "exits(top,surface)", "leg", "walk", "phase-head(jump,column look-up)"};
      double tot = 0;
      for (int i = 0; i < 9; i++) tot += (double)st[i];
      for (int i = 0; i < 9; i++) fprintf(stderr, "stamp %-40s %14llu  %5.1f %%\n", names[i], st[i], 100.0 * (double)st[i] / tot);
    }
#endif
    c->lastCounters = mcbrat_counters{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3],
                                      (int64_t)h[4], (int64_t)h[5], (int64_t)h[6], (int64_t)h[7],
                                      (int64_t)h[8], (int64_t)h[9], (int64_t)h[10], (int64_t)h[11], (int64_t)h[12], (int64_t)h[13],
                                      (int64_t)*c->hBad.get()};
  }
  c->haveLast = true;
  if (numPhotonsProcessed) *numPhotonsProcessed = ppb * (int64_t)nBatches;
  c->err = "computeRadiativeTransfer: finished with photons";
  return 0;
}

int mcbrat_report_results(mcbrat_ctx *c, float *meanUp, float *meanDown, float *meanAbs, float *fluxUp, float *fluxDown,
                          float *fluxAbs, float *absorbedProfile, float *volumeAbsorption) {
  if (!c) return 1;
  const size_t ncol = (size_t)c->nx * c->ny, nvox = ncol * c->nz;
  const TallyLayout lay = tally_layout(c);
  std::vector<float> h((size_t)lay.momentsLen);
  if (read_last(c, 0, h)) return 1;
  if (meanUp) *meanUp = h[lay.momMeans];
  if (meanDown) *meanDown = h[lay.momMeans + 1];
  if (meanAbs) *meanAbs = h[lay.momMeans + 2];
  if (fluxUp) std::memcpy(fluxUp, &h[lay.momColumns], sizeof(float) * ncol);
  if (fluxDown) std::memcpy(fluxDown, &h[lay.momColumns + ncol], sizeof(float) * ncol);
  if (fluxAbs) std::memcpy(fluxAbs, &h[lay.momColumns + 2 * ncol], sizeof(float) * ncol);
  if (absorbedProfile) std::memcpy(absorbedProfile, &h[lay.momProfile], sizeof(float) * c->nz);
  if (volumeAbsorption) std::memcpy(volumeAbsorption, &h[lay.momVolume], sizeof(float) * nvox);
  return 0;
}

int mcbrat_trace_fates(mcbrat_ctx *c, uint64_t seed, uint64_t firstPhotonId, int64_t n, mcbrat_fate *fates) {
  if (!c) return 1;
  (void)hipSetDevice(c->device);
  if (check_ready(c)) return 1;
  if (n < 1 || !fates) return fail(c, "trace_fates: nothing to trace.");
  if (sync_all(c)) return 1;
  Asked a = asked(c);
  a.debug = true;
  REFUSE(c, a, Fates);
  TallyShape fluxes = flux_run(tally_shape(c));  // the slab of the instrumented kernels: the fluxes and the volume only
  fluxes.nOrd = 0;
  const size_t slabStride = (size_t)tally_layout(fluxes).slabStride;
  DeviceBuffer<long long> scratch;  // (the three temporaries of this call go with it, however it returns)
  DeviceBuffer<mcbrat_fate> dF;
  DeviceBuffer<double> dTrace;
  HIP_OK(c, scratch.allocate(slabStride));
  HIP_OK(c, dF.allocate((size_t)n));
  HIP_OK(c, hipMemsetAsync(scratch.get(), 0, sizeof(long long) * slabStride, c->L().stream));
  HIP_OK(c, hipMemsetAsync(dF.get(), 0xff, sizeof(mcbrat_fate) * (size_t)n, c->L().stream));
  HIP_OK(c, hipMemsetAsync(c->L().dCounter.get(), 0, sizeof(unsigned long long), c->L().stream));
  HIP_OK(c, hipMemsetAsync(c->dEventCounters.get(), 0, 32 * sizeof(unsigned long long), c->L().stream));
  DevParams p;
  fill_params(c, p);
  p.seedLo = (uint32_t)seed; p.seedHi = (uint32_t)(seed >> 32);
  p.slabs = scratch.get(); p.slabStride = slabStride;
  p.ppb = (unsigned long long)n; p.total = (unsigned long long)n; p.firstPhoton = firstPhotonId;
  p.fates = dF.get(); p.counters = c->dEventCounters.get();
  const int traceCap = 4096;
  if (const char *tp = getenv("MCBRAT_TRACE_PHOTON")) {  // development aid: per-collision records of one photon
    HIP_OK(c, dTrace.allocate((size_t)12 * traceCap));
    HIP_OK(c, hipMemsetAsync(dTrace.get(), 0, sizeof(double) * 12 * traceCap, c->L().stream));
    p.traceBuf = dTrace.get(); p.traceIndex = strtoull(tp, nullptr, 10); p.traceCap = traceCap;
  }
  int rc = launch_trace(c, p, true, 1);
  if (!rc && dTrace) {
    std::vector<double> h(12 * traceCap);
    (void)hipStreamSynchronize(c->L().stream);
    (void)hipMemcpy(h.data(), dTrace.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost);
    if (h[0] == 777) {
      for (int r = 0; r < 64 && h[20 * r] == 777; ++r) {  // (-DMCBRAT_STUCK_PROBE: state tcur tnx tny tnz rx ry rz px py pz dx dy dz acc tau ext spans id)
        fprintf(stderr, "STUCK %d:", r);
        for (int i = 1; i < 20; ++i) fprintf(stderr, " %.9g", h[20 * r + i]);
        fprintf(stderr, "\n");
      }
    }
    for (int i = 0; i < traceCap && h[0] != 777; ++i)  // (indexed by scattering order: surface reflections leave gaps)
      if (h[12 * i] > 0) fprintf(stderr, "GPUTRACE %d ev %.0f cell %.0f %.0f %.0f pos %.17g %.17g %.17g dir %.9g %.9g %.9g tau %.9g w %.9g\n", i, h[12 * i],
              h[12 * i + 1], h[12 * i + 2], h[12 * i + 3], h[12 * i + 4], h[12 * i + 5], h[12 * i + 6], h[12 * i + 7], h[12 * i + 8],
              h[12 * i + 9], h[12 * i + 10], h[12 * i + 11]);
  }
  if (!rc) {
    hipError_t e = hipStreamSynchronize(c->L().stream);
    if (e == hipSuccess) e = hipMemcpy(fates, dF.get(), sizeof(mcbrat_fate) * (size_t)n, hipMemcpyDeviceToHost);
    unsigned long long h[16];
    if (e == hipSuccess) e = hipMemcpy(h, c->dEventCounters.get(), sizeof(h), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(c->hBad.get(), c->dBad.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, std::string("trace_fates: ") + hipGetErrorString(e));
    else c->lastCounters = mcbrat_counters{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3],
                                           (int64_t)h[4], (int64_t)h[5], (int64_t)h[6], (int64_t)h[7],
                                           (int64_t)h[8], (int64_t)h[9], (int64_t)h[10], (int64_t)h[11], (int64_t)h[12], (int64_t)h[13],
                                           (int64_t)*c->hBad.get()};
  }
  return rc;
}

}  // extern "C"
