// mcbrat_kernels.hip -- gfx950 (CDNA4) kernels of the photon-tracing path.
//
// What is replaced: computeRT, Integrators/monteCarloRadiativeTransfer.f95:393-841, and
// the routines it calls per photon (getNextPhoton src/monteCarloIllumination.f95:561,
// accumulateExtinctionAlongPath src/opticalProperties.f95:1656-1815, computeScatteringAngle
// :1594, next_direct :1921, makeDirectionCosines :1876), plus the per-batch epilogue
// (computeRadiativeTransfer :328-364, reportResults :845-1042, driver moments
// Drivers/monteCarloDriver.f95:1023-1050).
//
// Design (MI355X first, not a translation):
//  * one photon per work-item in persistent 64-wide waves.  Idle lanes are refilled in place
//    (regeneration) with ballot/popcount ranks: from a chunk of photon ids the wave took from
//    one global counter, or -- PRIV mode -- from the workgroup's own range via an LDS counter.
//  * the loop is split in two dense halves.  A tight walk loop in which every walking lane
//    crosses exactly one voxel face per iteration runs until fewer than `eventThreshold` lanes
//    of the wave are still walking; then one event phase serves all waiting lanes at once
//    (launch, collision, surface reflection, next leg set-up).
//  * cell-authoritative voxel walk: the distance along the leg to the next x/y/z face is kept
//    per axis in registers (float); only the crossed axis is updated -- by one cell spacing on
//    equally spaced axes, from the edge table in LDS otherwise; periodic wrap shifts the leg
//    origin; the position (double, as in the reference) is materialised once per leg.  Statistically,
//    not bitwise, identical to the reference's position-stepping walk with spacing() snaps.
//  * layer-skipping walk: a layer with one extinction value (clear air above and below a cloud field) needs no
//    extinction read and no x/y faces; a run of such layers is taken in one step, and the column is found again
//    from the position when the lane collides, leaves, or reaches a layer with cell-to-cell extinction
//    (ST_JUMP / ST_ENTER, tryJump / resolveXY below).  The radiance rays do the same.
//  * counter-based Philox4x32-10: key = seed, counter = (event, block, photon id); every role has a fixed slot, so that ONE
//    block serves a whole leg in the common case.  The slot table is in mcbrat_photon.h.
//  * cell edges and, when they fit, the inverse phase-function tables are staged in LDS by
//    coalesced loads; extinction / ssa / phase index are float / float / u16 grids in HBM that
//    stay resident in L1/L2/Infinity Cache.
//  * tallies are signed 64-bit fixed point (2^-32): integer sums are order independent, so
//    results are bitwise reproducible and independent of the number of GPUs.  Small domains
//    (PRIV): each workgroup traces photons of ONE batch and tallies into an LDS slab that is
//    flushed once with global atomics; large domains: global atomics into the batch's slab.
//    fluxAbsorbed is the column sum of the volume tally (same deposits, :766-769).
//  * radiance by local estimation (INTEN instantiations): see the block after the surface
//    reflection in the event phase and DESIGN.md section 4.3.
#include <float.h>
#include <type_traits>

#include "mcbrat_device.h"
#include "mcbrat_brdf.h"
#include "mcbrat_layout.h"
#include "mcbrat_photon.h"
#include "mcbrat_variants.h"

namespace mcbrat {

constexpr unsigned kChunk = 256;  // photon ids a wave takes per global atomic (global mode)
#ifndef MCBRAT_FLY_MIN_BRICKS
#define MCBRAT_FLY_MIN_BRICKS 8.0f
#endif
constexpr float kFlyMinBricks = MCBRAT_FLY_MIN_BRICKS;  // brick columns a flight that ends in a clear-air collision must cross to be worth taking
constexpr int kWalkCap = 256;     // walk-loop iterations between two event phases at most (a leg crosses ~4-15 faces)

#ifndef MCBRAT_WAVES_GLOBAL_GRID
#define MCBRAT_WAVES_GLOBAL_GRID 6  // (round 2: without the emission launch code the solar kernel needs 73 VGPRs, no scratch; 7 waves: the same rate with 2-4 spilled; 8: -6 %)
#endif
#ifndef MCBRAT_WAVES_GLOBAL_GRID_INTEN  // radiance instantiations
#define MCBRAT_WAVES_GLOBAL_GRID_INTEN 4
#endif

// the same patch look-up, returning the patch (BRDF surfaces).  (Not shared with surface_reflectance: written in terms of it, the
// instrumented kernels' register allocation changed.)
__device__ __forceinline__ int surface_patch(const DevParams &p, double x, double y) {
  const int xi = min(max(find_index_mixed(p.surfX, p.surfNumX, make_periodic_f(x, p.surfX[0], p.surfX[p.surfNumX - 1])), 1), p.surfNumX - 1);
  const int yi = min(max(find_index_mixed(p.surfY, p.surfNumY, make_periodic_f(y, p.surfY[0], p.surfY[p.surfNumY - 1])), 1), p.surfNumY - 1);
  return (xi - 1) + (p.surfNumX - 1) * (yi - 1);
}
// A reflection off a BRDF patch: the direction taken and, in w, the factor of the weight.  (lx, ly, lz) is the Lambertian draw,
// which every model keeps (factor R) but Cox-Munk with the glint mixture (kind 3 | kSurfKindSampled: brdf_sample, mcbrat_brdf.h,
// DESIGN.md section 4.11.1), whose three uniforms are block kGlintBlock of the photon's event.  ONE called function for all of
// them, the Philox block included, and for the local estimate's R too (surface_brdf below).  Called, not inlined: inlined, the
// evaluator's double-precision pow / acos added their registers to the whole tracing loop (the BRDF flux kernels spilled 35-129
// VGPRs to scratch and ran at 72-84 % of a Lambertian description's rate).  And one function, not two: with
// the sampler as a second called function beside the evaluator's, the land models' flux kernels ran at 42-55 % of their rate, and
// with two in the radiance kernels alone those lost 6-7 % on landsatLike128 (profiles/coxmunk_cost.json).
// (The sampler never returns a cosine below kBrdfSampleMuMin with a factor above 0: the walk's float distances along a leg are
// built for the Lambertian draw's cosines, and a leg a million times longer than the domain is high stops advancing.)
__device__ __noinline__ float4 surface_reflect_call(int kind, float4 q4, float ix, float iy, float iz, float lx, float ly, float lz, uint32_t event,
                                                    uint32_t idLo, uint32_t idHi, uint32_t seedLo, uint32_t seedHi) {
  const float q[4] = {q4.x, q4.y, q4.z, q4.w};
  if (kind != (BRDF_COXMUNK | kSurfKindSampled))
    return make_float4(lx, ly, lz, brdf_reflectance(kind & kSurfKindMask, q, (double)ix, (double)iy, (double)iz, (double)lx, (double)ly, (double)lz));
  uint32_t g[4];
  philox4x32_10(event, kGlintBlock, idLo, idHi, seedLo, seedHi, g);
  const double dIn[3] = {(double)ix, (double)iy, (double)iz}, u[3] = {(double)u01(g[0]), (double)u01(g[1]), (double)u01(g[2])};
  double dOut[3] = {(double)lx, (double)ly, (double)lz};
  float factor;
  brdf_sample(BRDF_COXMUNK, q, dIn, u, dOut, factor);
  return make_float4((float)dOut[0], (float)dOut[1], (float)dOut[2], factor);
}
// the reflectance factor R = pi f of a BRDF patch for the propagation directions d_in (arriving) and d_out (leaving): the same
// called function with the model alone as its kind, which evaluates and draws nothing
__device__ __forceinline__ float surface_brdf(const DevParams &p, int patch, float ix, float iy, float iz, float ox, float oy, float oz) {
  // (a BRDF surface's parameters, DevParams::surfRefl)
  return surface_reflect_call(p.surfKind & kSurfKindMask, reinterpret_cast<const float4 *>(p.surfRefl)[patch], ix, iy, iz, ox, oy, oz, 0u, 0u, 0u, 0u, 0u).w;
}

// Optical-property lookup.  Dense: one gather from the [nz][ny][nx] grid.  BRICK: the grid is cut
// into 4x4x4 bricks; a brick whose 64 cells all equal their layer's background value (clear air:
// most of a cloud scene) has no storage -- its cells read the per-layer background from LDS --
// and only the other bricks are stored, 64 cells each.  The brick table (4 B per 64 cells) and the
// stored bricks are a fraction of the dense grid, so the walk's working set fits the XCD's 4 MiB
// L2 instead of thrashing it (L2 hit rate 72 % -> measured there).
struct CellRef {
  int dense;   // dense cell index (tallies, and optics when !BRICK)
  int stored;  // BRICK: index into the stored-brick arrays, or -1 for a background cell
};

template <bool BRICK>
__device__ __forceinline__ CellRef locate_cell(const DevParams &p, int ix, int iy, int iz) {
  CellRef r;
  r.dense = ix + p.nx * (iy + p.ny * iz);
  r.stored = -1;
  if (BRICK) {
    const uint32_t base = p.brickTable[(ix >> 2) + p.nbx * ((iy >> 2) + p.nby * (iz >> 2))];
    if (base != 0xffffffffu) r.stored = (int)(base + (uint32_t)((ix & 3) + 4 * ((iy & 3) + 4 * (iz & 3))));
  }
  return r;
}

template <bool BRICK>
__device__ __forceinline__ float load_ext(const DevParams &p, const float *s_bgExt, const CellRef &r, int iz) {
  if (!BRICK) return p.extWalk[r.dense];  // (the walk's copy: sign bit = outside the brick column's range, see FLY)
  return r.stored >= 0 ? p.ext[r.stored] : s_bgExt[iz];
}

// The slab a lane of trace_kernel deposits into: its workgroup's private one in LDS (PRIV), else its batch's in global memory
// (tally_slab<0>: the batch's slab whatever the kernel -- the level, actinic and side bins, the combined volume deposits)
template <int PRIV>
__device__ __forceinline__ long long *tally_slab(long long *s_slab, const DevParams &p, uint32_t batch) {
  return PRIV ? s_slab : p.slabs + (unsigned long long)batch * p.slabStride;
}
__device__ __forceinline__ void deposit(long long *bin, unsigned long long dep) { atomicAdd(reinterpret_cast<unsigned long long *>(bin), dep); }

// PRIV: 0 tallies by global atomics, 1 LDS-private tally slab, 2 private slab and the optical grid in LDS too
// INTEN: radiance by local estimation (computeIntensityContribution :1623-1832): every launch of an emitted
// photon, surface reflection and scattering event sends a contribution along each view direction.
// EMIT: the thermal-emission source (newPhotonStream_BBEmission): its launch code is compiled out of the solar
// instantiations -- it cost them a dozen registers (the 768-lane build of the block-walk kernel: 80 VGPRs + 26 spilled
// with it, 71 and no scratch without).
// SPEC: what the general kernel decides at run time from wave-uniform parameters, decided at compile time for the
// configurations that carry the large flux runs (dense grid in global memory, one or two components, layer-skipping
// walk and clear-air flight on, the domain's Lambertian albedo): 1 = no axis of the walk equally spaced, 2 = all of
// them, 3 = x and y but not z (a cloud scene on stretched layers); 0 = general.
// The branches and the scalar registers they keep alive leave the loop (the block-walk kernel gained 18 % this way).
// On top of a walk (SPEC & 3), solar instantiations fix the component count ((SPEC >> 2) & 3 = 1 or 2) and the roulette
// (SPEC & 16: on): measured on the 128x128x64 bench domain with these as constants, +2.2 % and +2.3 %
// (profiles/r04_experiments.txt; grid sizes as constants +0.5 %, queue thresholds nothing).
// ORD: fluxes and radiances by scattering order as well (recScatOrd): every fluxUp / fluxDown deposit and
// every local estimate also goes to the bin of the photon's order nScat when nScat <= numRecScatOrd.  Built for BLOCK 256 / 512,
// SPEC 0, BRICK and DEBUG off only; everything it adds sits behind `if constexpr (ORD)`.
// BRDF: a surface description whose model is not Lambertian (DevParams::surfKind): a reflection keeps the
// Lambertian draw of its direction and multiplies the weight by R(d_in, d_out) of the patch; its local estimates use R / pi.
// A Cox-Munk patch (surfKind 3 | kSurfKindSampled) draws from the mixture of its glint lobe and the Lambertian draw instead
// (surface_reflect_call; three uniforms of block kGlintBlock of the event, mcbrat_photon.h), local estimates as before.
// Solar sources, SPEC 0 and DEBUG off only; everything it adds sits behind `if constexpr (BRDF)`.
// LVL: upward and downward flux through every level (z face) of every column as well (recLevelFluxes):
// a photon that crosses face k adds its weight to the up or down bin (k, column).  The bins follow [fluxUp | fluxDown | volume] in
// the batch slab -- [levelUp ncol (nz+1) | levelDown ncol (nz+1)], level slowest -- and are never part of a workgroup's LDS
// slab: every deposit is a global atomic.  The face-by-face walk only (no layer skipping, no flight: both cross levels without
// stopping at them).  Built for BLOCK 256 / 512, PRIV 0 / 2, flux runs, SPEC 0, ORD, BRDF, BRICK and DEBUG off; everything it
// adds sits behind `if constexpr (LVL)`.
// DIRECT: the direct beam apart from the diffuse light in the downward level flux (recDirectLevelFluxes).
// A photon is direct from its launch to its first collision or surface arrival (the arrival itself included).  The slab gains a
// third level part, [levelUp | levelDown | levelDirect]: a downward crossing of a direct photon goes to levelDirect INSTEAD of
// levelDown, which then holds the diffuse crossings only (the epilogue adds the two raw bins for the total: integers, exact).
// The bit lives in state the lane already holds: `event` is 1 on the first leg and on no other (the launch zeroes it; the leg
// set-up, which every collision and every reflection that goes on passes through, increments it) -- no new register.  Solar LVL
// instantiations only; everything it adds sits behind `if constexpr (DIRECT)`.
// ACT: the actinic flux of every cell by track length (recActinicFlux): every committed step of the
// face-by-face walk adds w (tmin - tcur) to the cell it leaves, and every collision adds w (tc - tcur), the piece from the
// cell's entry to the collision point, before the weight changes.  The bins follow the level parts in the batch slab --
// [... | actinic ncol nz], layer slowest as the volume part -- and are never part of a workgroup's LDS slab: every deposit is
// a global atomic of weight_to_fixed(w l 2^-e), 2^-e = DevParams::actScale (the longest possible step stays below 2^e).  Solar
// sources and the face-by-face walk only, as LVL; with or without LVL, never with DIRECT; everything it adds sits behind
// `if constexpr (ACT)`.
// SIDE: the flux through the vertical faces of every cell (recSideFluxes): a committed step of the
// face-by-face walk that crosses an x or y face adds the weight the leg carries to the bin of that face -- the cell on its low
// side, in the patch (row or column, layer) of the cell being left -- by direction of travel.  The four parts follow the level
// parts in the batch slab, [... | levelDown | xPlus ncol nz | xMinus ncol nz | yPlus ncol nz | yMinus ncol nz], layer slowest as
// the volume part, and are never part of a workgroup's LDS slab: every deposit is a global atomic, MCBRAT_LEVEL_DEPOSIT of
// weight_to_fixed(w).  Solar LVL instantiations without DIRECT and ACT only; everything it adds sits behind `if constexpr (SIDE)`.
template <int BLOCK, bool TBL_LDS, int PRIV, bool BRICK, bool DEBUG, bool INTEN = false, bool EMIT = true, int SPEC = 0, bool ORD = false, bool BRDF = false,
          bool LVL = false, bool DIRECT = false, bool ACT = false, bool SIDE = false>
__global__ void __launch_bounds__(BLOCK, BLOCK == 1024 ? 4 : BLOCK > 512 ? BLOCK / 128 : ((PRIV == 0 && !DEBUG) ? (INTEN ? MCBRAT_WAVES_GLOBAL_GRID_INTEN : MCBRAT_WAVES_GLOBAL_GRID) : MCBRAT_MIN_WAVES_PER_SIMD))
trace_kernel(const DevParams p) {
  constexpr int WALKSPEC = SPEC & 3, NCSPEC = (SPEC >> 2) & 3;
  static_assert(valid(TraceVariant{BLOCK, TBL_LDS, PRIV, BRICK, DEBUG, INTEN, EMIT, SPEC, ORD, BRDF, LVL, DIRECT, ACT, SIDE}), "no such instantiation: see valid(), mcbrat_variants.h");
  const bool layerSkipOn = (LVL || ACT) ? false : (SPEC ? true : p.layerSkip != 0);
  const bool useRec = SPEC ? true : p.rec != nullptr;
  const bool xyRegularWalk = (WALKSPEC == 2 || WALKSPEC == 3) ? true : (WALKSPEC == 1 ? false : p.xyRegularWalk != 0);
  const bool zRegularWalk = WALKSPEC == 2 ? true : ((WALKSPEC == 1 || WALKSPEC == 3) ? false : p.zRegularWalk != 0);
  const bool surfaceDescription = SPEC ? false : p.surfNumX > 0;
  const int nc = NCSPEC ? NCSPEC : p.nc;
  const bool useRR = (SPEC & 16) ? true : p.useRR != 0;
  extern __shared__ __align__(16) unsigned char smem_raw[];
#ifdef MCBRAT_POISON  // audit build: whatever the kernel reads from LDS before it wrote it reads 0xff..
  for (unsigned i = threadIdx.x; i < p.ldsBytes / 4u; i += BLOCK) reinterpret_cast<unsigned *>(smem_raw)[i] = 0xffffffffu;
  __syncthreads();
#endif
  // LDS map: [edges x|y|z (double)] [private tally slab (i64), PRIV] [unit cursor, PRIV]
  //          [extinction per layer: background (BRICK) / one-extinction layers] [layer runs] [optical grid, PRIV == 2]
  //          [tables (float), TBL_LDS]
  double *s_edge = reinterpret_cast<double *>(smem_raw);
  const int nEdges = p.nx + p.ny + p.nz + 3;
  const int offZ0 = p.nx + p.ny + 2;
  const int ncol = p.nx * p.ny;
  // The starts of the slab parts (mcbrat_layout.h), from this kernel's own counts and flags: they fold per instantiation
  const int slabLen = PRIV ? ((LVL || ACT) ? (int)slab_intensity_start<long long>(ncol, p.nz) : (int)p.slabStride) : 0;  // (LVL, ACT: the level and actinic bins stay in global memory)
  // ORD: the order bins behind [fluxUp | fluxDown | volume | intensity] of the batch slab (DevParams::numRecScatOrd)
  const long long ordUp = ORD ? slab_orders_start<long long>(ncol, p.nz, p.nDir, p.numRecScatOrd + 1, 0) : 0;
  const long long ordDown = ORD ? slab_orders_start<long long>(ncol, p.nz, p.nDir, p.numRecScatOrd + 1, 1) : 0;
  // LVL: the level bins behind [fluxUp | fluxDown | volume] of the batch slab (a flux run: nothing else lies between)
  constexpr long long kFluxRun = 0;  // the LVL, ACT and SIDE kernels trace flux runs without orders: no directions, no order parts in front
  const long long lvlUp = LVL ? slab_levels_start<long long>(ncol, p.nz, 0, kFluxRun, kFluxRun) : 0;
  const long long lvlDown = LVL ? slab_levels_start<long long>(ncol, p.nz, 1, kFluxRun, kFluxRun) : 0;
  const long long lvlDirect = DIRECT ? slab_levels_start<long long>(ncol, p.nz, 2, kFluxRun, kFluxRun) : 0;  // DIRECT: the third part, behind levelDown
  // ACT: the actinic bins behind the level parts (LVL: two of them; DIRECT and ACT are never together), or behind the volume
  const long long actBins = ACT ? slab_actinic_start<long long>(ncol, p.nz, LVL ? 2 : 0, kFluxRun, kFluxRun) : 0;
  // SIDE: the four side parts behind the two level parts (DIRECT and ACT are never together with it), ncol nz bins each
  const long long sideBins = SIDE ? slab_side_start<long long>(ncol, p.nz, 2, 0, kFluxRun, kFluxRun) : 0;
  const long long sidePart = SIDE ? (long long)ncol * p.nz : 0;
  long long *s_slab = reinterpret_cast<long long *>(s_edge + nEdges);
  unsigned *s_cursor = reinterpret_cast<unsigned *>(s_slab + slabLen);
  float *s_bgExt = reinterpret_cast<float *>(s_cursor + (PRIV ? 4 : 0));  // BRICK: background extinction per layer
  // PRIV (small domains): the whole optical grid is staged in LDS too -- extinction, ssa, phase index
  constexpr bool gridLds = PRIV == 2;
  const int nvoxS = gridLds ? ncol * p.nz : 0;
  int *s_run = reinterpret_cast<int *>(s_bgExt + ((p.nz + 3) & ~3));           // runs of one-extinction layers (DevParams::layerRun)
  double *s_runT = reinterpret_cast<double *>(s_run + ((p.nz + 3) & ~3));      // [nz+1] their cumulative vertical optical depth
  // clear-air flight: background extinction of every layer, cloud range of every brick column (DevParams::flyRange)
  constexpr bool FLY = PRIV != 2 && !BRICK && !INTEN && !LVL && !ACT;
  const bool flyOn = FLY && (SPEC ? true : p.fly != 0);
  const int flyCols = FLY ? p.flyNbx * p.flyNby : 0;
  float *s_bgVal = reinterpret_cast<float *>(s_runT + ((p.nz + 2) & ~1));
  float2 *s_rangeZ = reinterpret_cast<float2 *>(s_bgVal + (flyCols ? ((p.nz + 3) & ~3) : 0));  // heights of the faces lo, hi
  uint16_t *s_range = reinterpret_cast<uint16_t *>(s_rangeZ + flyCols);
  float *s_ext = reinterpret_cast<float *>(s_range + ((flyCols + 3) & ~3));
  float *s_ssa = s_ext + nvoxS;                       // [nc][nvox]
  float *s_cum = s_ssa + (size_t)nc * nvoxS;        // [nc][nvox]
  uint16_t *s_pfi = reinterpret_cast<uint16_t *>(s_cum + (size_t)nc * nvoxS);  // [nc][nvox]
  float *s_tbl = reinterpret_cast<float *>(s_pfi + (((size_t)nc * nvoxS + 1) & ~(size_t)1));
  // per-component table descriptors: indexed by a per-lane component number, so they must not stay in the
  // kernel-argument segment (a vector load from there costs a trip to memory on every collision)
  __shared__ int s_tblOffset[MCBRAT_MAX_COMPONENTS], s_tblNSteps[MCBRAT_MAX_COMPONENTS];
  __shared__ float s_tblInvN[MCBRAT_MAX_COMPONENTS];
  __shared__ int s_fwdOffset[MCBRAT_MAX_COMPONENTS], s_fwdNAngles[MCBRAT_MAX_COMPONENTS];
  // clear-air flight: the distance along the leg at which the background itself uses up the lane's optical depth (FLT_MAX: it
  // does not before the domain boundary).  Per lane, in LDS rather than in a register: written at take-off, read by flight steps only.
  __shared__ float s_flyTC[(PRIV != 2 && !BRICK && !INTEN && !LVL && !ACT) ? BLOCK : 1];
  if (INTEN && threadIdx.x < MCBRAT_MAX_COMPONENTS) {
    s_fwdOffset[threadIdx.x] = p.fwdOffset[threadIdx.x];
    s_fwdNAngles[threadIdx.x] = p.fwdNAngles[threadIdx.x];
  }
  if (threadIdx.x < MCBRAT_MAX_COMPONENTS) {
    s_tblOffset[threadIdx.x] = p.tblOffset[threadIdx.x];
    s_tblNSteps[threadIdx.x] = p.tblNSteps[threadIdx.x];
    s_tblInvN[threadIdx.x] = p.tblInvN[threadIdx.x];
  }
  for (int i = threadIdx.x; i < nEdges; i += BLOCK) s_edge[i] = p.edges[i];
  if (TBL_LDS)
    for (int i = threadIdx.x; i < p.tblTotalFloats; i += BLOCK) s_tbl[i] = p.tables[i];
  if (PRIV) {
    for (int i = threadIdx.x; i < slabLen; i += BLOCK) s_slab[i] = 0;
    if (threadIdx.x == 0) s_cursor[0] = 0;
  }
  // per layer: BRICK the background extinction; dense the extinction of a horizontally uniform layer or -1
  for (int i = threadIdx.x; i < p.nz; i += BLOCK) { s_bgExt[i] = p.bgExt[i]; s_run[i] = p.layerRun[i]; }
  for (int i = threadIdx.x; i <= p.nz; i += BLOCK) s_runT[i] = p.layerRunT[i];
  if (FLY && flyCols) {
    for (int i = threadIdx.x; i < p.nz; i += BLOCK) s_bgVal[i] = p.bgVal[i];
    for (int i = threadIdx.x; i < flyCols; i += BLOCK) {
      const unsigned r = p.flyRange[i];
      s_range[i] = (uint16_t)r;
      s_rangeZ[i] = make_float2((float)p.edges[offZ0 + (r & 0xffu)], (float)p.edges[offZ0 + (r >> 8)]);
    }
  }
  if (gridLds) {  // coalesced HBM reads, once per workgroup
    for (int i = threadIdx.x; i < nvoxS; i += BLOCK) s_ext[i] = p.ext[i];
    for (int i = threadIdx.x; i < nc * nvoxS; i += BLOCK) { s_ssa[i] = p.ssa[i]; s_cum[i] = p.cum[i]; s_pfi[i] = p.pfi[i]; }
  }
  __syncthreads();
  const float *__restrict__ tbl = TBL_LDS ? s_tbl : p.tables;
  const int offY = p.nx + 1, offZ = p.nx + p.ny + 2;  // edge table offsets
  // the walk loop's gather base in a scalar register pair of its own: as part of the 8-dword kernel-argument block it
  // arrived in, the register allocator spills and reloads the whole block around every gather
  // (declared in the global address space: after the pin below the compiler no longer knows where the pointer came
  // from and would gather with flat_load, which counts on the LDS counter as well as on the vector-memory one)
  typedef const float __attribute__((address_space(1))) *GlobalFloats;
  GlobalFloats extG = (GlobalFloats)p.extWalk;
  const float zTopF = (float)p.zMax, zBotF = (float)p.z0;
  if constexpr (!INTEN) asm volatile("" : "+s"(extG));  // (the radiance instantiations do not compile with the pin: "illegal VGPR to SGPR copy")

  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long laneBelow = (1ull << lane) - 1ull;

  // PRIV: this workgroup's unit = photons [unitFirst, unitFirst + unitCount) of ONE batch
  unsigned long long unitFirst = 0;
  unsigned unitCount = 0;
  long long *unitSlab = nullptr;

  // lane state --------------------------------------------------------------------------
  int state = ST_DEAD;
  bool more = true;
  uint32_t idLo = 0, idHi = 0, event = 0, batch = 0;
  // block (c0, c1) of the photon's Philox stream, for the rules of mcbrat_photon.h
  auto rng = [&](uint32_t c0, uint32_t c1, uint32_t (&out)[4]) __attribute__((always_inline)) { philox4x32_10(c0, c1, idLo, idHi, p.seedLo, p.seedHi, out); };
  double px = 0, py = 0, pz = 0;      // leg origin (in the periodic image the walk is currently in)
  float dx = 0, dy = 0, dz = 1;       // direction cosines
  float ivx = 0, ivy = 0, ivz = 0;    // 1/direction
  float tnx = 0, tny = 0, tnz = 0, tcur = 0;  // distance along the leg to the next x/y/z face
  float acc = 0, tau = 0, w = 0, extCur = 0, uX = 0, uY = 0, uZ = 0;
  int ex = 0, ey = 0, ez = 0;  // index in the LDS edge table of the next x / y / z face of the leg
  int cell = 0;                // linear index of the current cell
  // Tallies in global memory: the deposits of consecutive collisions in ONE cell (a photon in a dense cell scatters
  // several times before it leaves it) go out as one atomic add when the photon deposits elsewhere or ends.  Integer
  // sums: bitwise the same tallies.  Every global atomic travels to the memory side on this part, and 128x128x64 issued
  // them at most of the rate the chip sustains: a third fewer of them was worth 9 %.
  int pendCell = -1;
  unsigned long long pendDep = 0ull;
  unsigned nBadLane = 0;  // photons this lane dropped at a loop bound; added to *p.bad when the kernel ends
#define MCBRAT_FLUSH_PENDING() do { if (!PRIV && pendCell >= 0) { \
    deposit(tally_slab<0>(s_slab, p, batch) + 2 * ncol + pendCell, pendDep); pendCell = -1; } } while (0)
  // A photon that exceeds one of the loop bounds (DevParams::bad) is dropped and counted, as computeRT :562-563 does with
  // a photon whose step is not positive.
#define MCBRAT_DROP_PHOTON(kind_) do { \
    if constexpr (DEBUG || kTestBounds) record_first_drop(p.bad, (kind_), 1u, idLo, idHi, state, event);  /* (which bound, which photon) */ \
    if (DEBUG) record_fate(p, idLo, idHi, 3, 0, 0, 0, nScat, nLegs, w); \
    MCBRAT_FLUSH_PENDING(); \
    state = ST_DEAD; \
    nBadLane = count_drop(nBadLane, (kind_));  /* (added to *p.bad when the kernel ends: no atomic, no pointer in the loop) */ \
  } while (0)
  // LVL: one crossing of level `lev_` in column `col_` with the fixed-point weight `dep_`, into the batch's slab in global memory
#define MCBRAT_LEVEL_DEPOSIT(base_, lev_, col_, dep_) \
    deposit(tally_slab<0>(s_slab, p, batch) + (base_) + (long long)ncol * (lev_) + (col_), (dep_))
  // ACT: one piece of path of length `len_` (km) in cell `cell_` carried at weight `w_`, into the batch's slab in global memory
#define MCBRAT_ACTINIC_DEPOSIT(cell_, w_, len_) \
    deposit(tally_slab<0>(s_slab, p, batch) + actBins + (cell_), weight_to_fixed((w_) * (len_) * p.actScale))
  // Layer-skipping walk (dense grids in global memory): while `lazy`, the lane is in a layer with one extinction
  // value, crosses z faces only (tnx = tny = FLT_MAX) and its x/y state (ex, ey, the x/y part of cell, the periodic
  // image of px/py) is stale; the event phase brings it up to date from the position before anything uses it.
  constexpr bool LAZY = PRIV != 2 && !BRICK && !LVL && !ACT;
  bool lazy = false;
  double dbgU0 = 0, dbgV0 = 0;  // DEBUG: fractional cell coordinates where the lane went lazy (faces skipped = crossings)
  // Clear-air flight (FLY).  The host groups the columns 4 x 4 into brick columns and records for
  // each the layers [lo, hi) that hold a cell differing from its layer's background extinction: a cloud field is
  // background -- clear air -- outside those ranges, and that is where its photons cross most of their cells (the way
  // down to the cloud tops and back up).  Clear air attenuates by its height alone: between two heights the optical
  // depth of ANY path through background cells is (T(z1) - T(z0)) / mu, T the vertical optical depth of the
  // background (s_runT).  So a lane whose remaining optical depth cannot be used up by the background between here and
  // the domain boundary (clear air: nearly always) needs neither the cells nor their extinction while it stays outside
  // the ranges: it steps from brick column to brick column (stride = 4 cells; x/y faces of the brick column, and the z
  // face where the column's range begins) with extCur = 0, and gets its optical depth from T when the flight ends -- at
  // the domain boundary (x/y cell from the position), at the face of a range, or on an x/y face of a brick column whose
  // range it enters sideways (ST_ENTER; cell from the position, inside the brick column the stepping has tracked).  The
  // walk reads a copy of the extinction grid in which the cells outside their brick column's range carry the sign bit:
  // a lane that steps into one asks for a flight (ST_JUMP, served with the other rare transitions); a lane that is
  // refused (noFly: its optical depth may run out in the clear air) walks on cell by cell with |extinction|.
  int stride = 1;       // cells per x/y step: 4 in flight
  bool noFly = false;   // this leg stays on the face-by-face walk
  bool flyToCollision = false;  // the flight under way ends in a collision with the background at s_flyTC (a lane mask: no vector register)
  int dbgK0 = 0;        // DEBUG: layer where the flight began
  // BRICK: the brick the lane is in and its table entry (offset of its 64 stored cells, or 0xffffffff for an
  // unstored background brick), re-read only when the walk enters another brick
  int brickId = -1;
  uint32_t brickBase = 0xffffffffu;
  int nScat = 0, nLegs = 0;
  // INTEN: a pending local estimate of this lane: 0 none, 1 Lambertian surface (component 0 of the reference),
  // 2 isotropic emission (component -1), 3 + c scattering by component c; its weight, incoming direction and
  // the offset of the phase-function entry in the forward tables
  int iFlag = 0, iEntry = 0;
  float iW = 0, iDx = 0, iDy = 0, iDz = 0;
  unsigned long long chunkNext = 0, chunkEnd = 0;  // global mode, wave-uniform
  unsigned int cLegs = 0, cCross = 0, cColl = 0, cAbs = 0, cTop = 0, cSurf = 0, cKill = 0, cSurv = 0;
  // DEBUG, wave level (lane 0): loop iterations and how many lanes each kind of phase served
#ifdef MCBRAT_STAMPS
  __shared__ unsigned long long s_tprev[BLOCK / 64], s_stamp[BLOCK / 64][9];
  if (lane == 0) { s_tprev[threadIdx.x >> 6] = clock64(); for (int i = 0; i < 9; i++) s_stamp[threadIdx.x >> 6][i] = 0; }
#endif
  unsigned long long wWalkIters = 0, wWalkLanes = 0, wEventPhases = 0, wEventLanes = 0, wLaunchPhases = 0, wSurfPhases = 0;

  // Layer-skipping walk, event-phase halves.  tryJump: a lane in a run of one-extinction layers takes the rest of
  // the run in one step when its optical depth is not used up inside it (clear air: nearly always) -- it then stands
  // at the domain top, at the surface, or at the face of a layer with cell-to-cell extinction (ST_ENTER); otherwise
  // it walks the run layer by layer to its collision.
  auto tryJump = [&]() {
    const bool up = dz >= 0.0f;
    const int k = ez - offZ - (up ? 1 : 0);
    const int run = s_run[k];
    const int fEnd = up ? (run >> 16) : (run & 0xffff);
    const double dT = up ? s_runT[fEnd] - s_runT[k + 1] : s_runT[k] - s_runT[fEnd];
    extCur = fabsf(extCur);  // (a leg that starts here still holds the walk's marked copy of the extinction, see FLY)
    const float accEnd = acc + (tnz - tcur) * extCur + (float)dT * fabsf(ivz);
    if (DEBUG) { dbgU0 = (px + (double)tcur * (double)dx - p.x0) * p.invCellX; dbgV0 = (py + (double)tcur * (double)dy - p.y0) * p.invCellY; }
    lazy = true;
    tnx = FLT_MAX; tny = FLT_MAX;
    state = ST_WALK;
    if (accEnd <= tau) {
      acc = accEnd;
      tcur = (float)(s_edge[offZ + fEnd] - pz) * ivz;
      if (DEBUG) cCross += (unsigned)(up ? fEnd - k : k + 1 - fEnd);
      if (up) { ez = offZ + fEnd + 1; state = fEnd == p.nz ? ST_TOP : ST_ENTER; }
      else { ez = offZ + fEnd - 1; state = fEnd == 0 ? ST_SURFACE : ST_ENTER; }
      if (state == ST_SURFACE) extCur = s_bgExt[0];
      tnz = (float)(s_edge[min(max(ez, offZ), offZ + p.nz)] - pz) * ivz;
    }
  };
  // resolveXY: x/y state of a lane that leaves the layer-skipping walk, from the position it has reached
  auto resolveXY = [&]() {
    const float tc = state == ST_COLLIDE ? tcur + div_fast(tau - acc, fabsf(extCur)) : tcur;
    const double xw = px + (double)tc * (double)dx, yw = py + (double)tc * (double)dy;
    if (DEBUG) cCross += (unsigned)(fabs(floor((xw - p.x0) * p.invCellX) - floor(dbgU0)) + fabs(floor((yw - p.y0) * p.invCellY) - floor(dbgV0)));
    const int jx = locate_periodic(s_edge, p.nx, p.x0, p.Lx, p.invLx, p.invCellX, p.xyNearUniform != 0, px, xw);
    const int jy = locate_periodic(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, p.invCellY, p.xyNearUniform != 0, py, yw);
    ex = jx + (dx >= 0.0f ? 1 : 0);
    ey = offY + jy + (dy >= 0.0f ? 1 : 0);
    tnx = ivx != 0.0f ? (float)(s_edge[ex] - px) * ivx : FLT_MAX;
    tny = ivy != 0.0f ? (float)(s_edge[ey] - py) * ivy : FLT_MAX;
    cell = jx + p.nx * (jy + p.ny * (ez - offZ - (dz >= 0.0f ? 1 : 0)));
    lazy = false;
    if (state == ST_ENTER) { extCur = extG[cell]; state = ST_WALK; noFly = false; }  // (the optical depth has moved on: it may fly now)
  };
  // tryFly: a lane on the face-by-face walk (at a leg start, or anywhere inside a cell) takes off if the background
  // between its height and the domain boundary cannot use up its optical depth and its brick column's range is not
  // around it.  acc then holds (optical depth so far) - T(here) / mu until the flight ends.
  auto tryFly = [&]() -> bool {
    const bool up = dz >= 0.0f;
    const int k = ez - offZ - (up ? 1 : 0);
    const int jx = ex - (dx >= 0.0f ? 1 : 0), jy = ey - offY - (dy >= 0.0f ? 1 : 0);
    const double zw = pz + (double)tcur * (double)dz;
    const double Tz = s_runT[k] + (double)s_bgVal[k] * (zw - s_edge[offZ + k]);
    const float dT = (float)((up ? s_runT[p.nz] : 0.0) - Tz) * ivz;
    // Where the background itself uses up the optical depth before the domain boundary (a grazing leg through Rayleigh air:
    // the optical depth of a 1000 km path is not small) the flight is not refused -- refused, such a leg walked thousands of
    // clear cells one by one and its photons were the tail of every launch -- but ends in a collision at the height where
    // T(z) has grown by (tau - acc) |mu|: T is piecewise linear in z, so that height is one division away.
    float tC = FLT_MAX;
    if (!(acc + dT <= tau)) {
      const double Tt = Tz + (double)(tau - acc) * (double)dz;  // T at the collision height (falls for a downward leg)
      int kc = k;
      if (up) { while (kc < p.nz - 1 && s_runT[kc + 1] <= Tt) ++kc; }
      else { while (kc > 0 && s_runT[kc] >= Tt) --kc; }
      const float bg = s_bgVal[kc];
      if (!(bg > 0.0f)) return false;  // (T does not grow in this layer: no flight crosses it, the face-by-face walk decides)
      const double zc = s_edge[offZ + kc] + (Tt - s_runT[kc]) / (double)bg;
      tC = (float)(zc - pz) * ivz;
      // (a collision a few cells away is found faster by walking there than by a take-off and a landing: the flight is for
      // the stretches that are long -- more than kFlyMinBricks brick columns -- which also leaves out a collision that
      // rounding put behind the lane)
      if (!((tC - tcur) * (fabsf(dx) * p.flyInvBrickX + fabsf(dy) * p.flyInvBrickY) > kFlyMinBricks)) return false;
    }
    const unsigned rng = s_range[(jx >> 2) + p.flyNbx * (jy >> 2)];
    const int lo = (int)(rng & 0xffu), hi = (int)(rng >> 8);
    if (k >= lo && k < hi) return false;  // (cannot happen for a cell that carries the mark)
    const int limF = up ? (k < lo ? lo : p.nz) : (k >= hi ? hi : 0);  // (the layer index decides here, not rounded distances)
    const float tLim = (float)(s_edge[offZ + limF] - pz) * ivz;
    if (s_bgExt[k] >= 0.0f) {
      // in a run of one-extinction layers that reaches as far as the flight would: the run takes the stretch in ONE step
      // (tryJump), the flight in one step per brick column crossed -- a photon entering above a stratus deck would
      // cross a dozen.  Short hops (under the cloud base to the surface) stay flights: they spare most event phases the
      // run and column look-up code altogether.
      const int run = s_run[k];
      if ((up ? (run >> 16) : (run & 0xffff)) == limF &&
          (tLim - tcur) * (fabsf(dx) * p.flyInvBrickX + fabsf(dy) * p.flyInvBrickY) > 3.0f) return false;
    }
    tnz = fminf(tLim, tC);
    flyToCollision = tC < FLT_MAX;
    if (flyToCollision) s_flyTC[threadIdx.x] = tC;
    // in flight ez only says what the z limit is: the domain boundary (its face, so that the walk's own exit test
    // fires), or the face where the range begins / the height of the collision (any inner face; resolveFly looks up where that is)
    ez = (tC < tLim) ? offZ + 1 : (limF == p.nz ? offZ + p.nz : (limF == 0 ? offZ : offZ + 1));
    // In flight acc holds (optical depth so far) - U(here) / mu, with U = T for an upward leg and T - T(top) for a downward
    // one: either way the offset is not positive, so that the walk loop's own test `acc > tau` cannot fire while the lane
    // flies (a downward, collision-limited flight offset by T itself would carry T(here) / |mu|, which may well exceed tau).
    acc = acc - (float)(Tz - (up ? 0.0 : s_runT[p.nz])) * ivz;
    ex = ((jx >> 2) + (dx >= 0.0f ? 1 : 0)) << 2;
    ey = offY + (((jy >> 2) + (dy >= 0.0f ? 1 : 0)) << 2);
    tnx = ivx != 0.0f ? (float)(s_edge[ex] - px) * ivx : FLT_MAX;
    tny = ivy != 0.0f ? (float)(s_edge[ey] - py) * ivy : FLT_MAX;
    extCur = 0.0f;
    stride = 4;
    state = ST_WALK;
    if (DEBUG) { dbgU0 = (double)jx; dbgV0 = (double)jy; dbgK0 = k; }  // (the cell it leaves from; follows the leg origin through the periodic images)
    return true;
  };
  // resolveFly: the end of a flight.  The cell from the position, inside the brick column the stepping has tracked
  // (three edge comparisons per axis: a position on a face of the brick column falls into its first or last cell
  // whatever the rounding, so a lane can never be handed back to the brick column it came from); the optical depth
  // from T at the height reached.
  auto resolveFly = [&]() {
    const bool up = dz >= 0.0f;
    const double xw = px + (double)tcur * (double)dx, yw = py + (double)tcur * (double)dy;
    const int cx = ((ex >> 2) - (dx >= 0.0f ? 1 : 0)) << 2, cy = (((ey - offY) >> 2) - (dy >= 0.0f ? 1 : 0)) << 2;
    const int jx = cx + (xw >= s_edge[cx + 1] ? 1 : 0) + (xw >= s_edge[cx + 2] ? 1 : 0) + (xw >= s_edge[cx + 3] ? 1 : 0);
    const int jy = cy + (yw >= s_edge[offY + cy + 1] ? 1 : 0) + (yw >= s_edge[offY + cy + 2] ? 1 : 0) + (yw >= s_edge[offY + cy + 3] ? 1 : 0);
    int k;
    if ((state == ST_ENTER && ez < 0) || state == ST_COLLIDE) {  // sideways into a range, or a collision in the clear air: the layer from the height
      const double zw = pz + (double)tcur * (double)dz;
      k = find_cell(s_edge + offZ, p.nz, zw);
      // (a collision height that rounding put on the face of a layer without background extinction: the layer the leg came through)
      if (state == ST_COLLIDE && !(s_bgVal[k] > 0.0f)) k = min(max(k + (up ? -1 : 1), 0), p.nz - 1);
      acc += (float)(s_runT[k] + (double)s_bgVal[k] * (zw - s_edge[offZ + k]) - (up ? 0.0 : s_runT[p.nz])) * ivz;
      ez = offZ + k + (up ? 1 : 0);
    } else if (state == ST_ENTER) {     // through the face where the range begins
      const unsigned rng = s_range[(cx >> 2) + p.flyNbx * (cy >> 2)];
      const int f = up ? (int)(rng & 0xffu) : (int)(rng >> 8);
      acc += (float)(s_runT[f] - (up ? 0.0 : s_runT[p.nz])) * ivz;
      k = up ? f : f - 1;
      ez = offZ + f + (up ? 1 : -1);
    } else {
      k = up ? p.nz - 1 : 0;            // out of the domain
    }
    if (DEBUG) {
      const int kEnd = (state == ST_ENTER || state == ST_COLLIDE) ? k : (up ? p.nz : -1);
      cCross += (unsigned)(fabs((double)jx - dbgU0) + fabs((double)jy - dbgV0)) + (unsigned)abs(kEnd - dbgK0);  // faces between the two cells
    }
    tnz = (float)(s_edge[min(max(ez, offZ), offZ + p.nz)] - pz) * ivz;
    ex = jx + (dx >= 0.0f ? 1 : 0);
    ey = offY + jy + (dy >= 0.0f ? 1 : 0);
    tnx = ivx != 0.0f ? (float)(s_edge[ex] - px) * ivx : FLT_MAX;
    tny = ivy != 0.0f ? (float)(s_edge[ey] - py) * ivy : FLT_MAX;
    cell = jx + p.nx * (jy + p.ny * k);
    stride = 1;
    if (state == ST_ENTER) { extCur = extG[cell]; state = ST_WALK; }
    else if (state == ST_SURFACE || state == ST_COLLIDE) extCur = extG[cell];  // (the reflected leg starts in this cell / the collision is in it)
    if (state == ST_COLLIDE && !(fabsf(extCur) > 0.0f)) { extCur = 1.0f; acc = tau; }  // (never: the collision point stays where the flight ended)
  };
  // a lane waiting in ST_JUMP is served: the flight if it may take off (also where a run of one-extinction layers would do:
  // then the run and column look-up code below is skipped by most event phases of a cloud field); else the run of
  // one-extinction layers it stands in; else (a cell outside its brick column's range, but the optical depth may run
  // out in the clear air) the face-by-face walk for the rest of this leg.
#define MCBRAT_SERVE_JUMP() do { \
    const int k_ = ez - offZ - (dz >= 0.0f ? 1 : 0); \
    const bool uni_ = s_bgExt[k_] >= 0.0f; \
    bool done_ = false; \
    if (FLY && flyOn && !noFly) done_ = tryFly(); \
    if (!done_) { \
      noFly = true; \
      if (uni_) tryJump(); \
      else { \
        state = ST_WALK; \
        tnx = ivx != 0.0f ? (float)(s_edge[ex] - px) * ivx : FLT_MAX; \
        tny = ivy != 0.0f ? (float)(s_edge[ey] - py) * ivy : FLT_MAX; \
      } \
    } \
  } while (0)

  // ---- radiance rays (INTEN): state of the ray a lane walks, and the wave's buffer of unfinished long rays ----
  double qx = 0, qy = 0, rpz = 0;
  float rcur = 0, racc = 0, limit = 0, tauFree = 0, u2 = 0, rext = 0, rW = 0, rNpf = 0, rtx = 0, rty = 0, rtz = 0;
  float ddx = 0, ddy = 0, ddz = 1, jvx = 0, jvy = 0, jvz = 0;
  int rex = 0, rey = 0, rez = 0, rcell = 0, rphase = 0, rpend = 0, rd = 0, rcomp = 0;
  uint32_t rbatch = 0;
  int rord = 0;  // ORD: the scattering order the estimate was taken at
  bool ract = false, rlazy = false, outTop = false, outBottom = false;
  int sgX = 1, sgY = 1, sgZ = 1;  // step signs of the ray's direction (ints, not bools: uniform inside an event phase, per lane in a ray pass)
  int rayCount = 0;  // wave-uniform: rays in this wave's buffer
  uint4 *s_rays = reinterpret_cast<uint4 *>(smem_raw + ((((size_t)(reinterpret_cast<unsigned char *>(s_tbl + (TBL_LDS ? p.tblTotalFloats : 0)) - smem_raw)) + 15) & ~(size_t)15)) +
                  (size_t)(threadIdx.x >> 6) * (size_t)p.rayCap * 5;
  // Walks the lanes' rays in lockstep for at most maxIt iterations (accumulateExtinctionAlongPath as called by
  // computeIntensityContribution :1729-1813); rays skip layers of one extinction value the way photons do: a lazy ray
  // crosses z faces only, rpend marks a ray that waits to take a run of such layers in one step (1) or to find its
  // column again at the face of a layer with cell-to-cell extinction (2); waiting rays are served together.
#define MCBRAT_RAY_WALK(maxIt_) do { \
    const int maxIt = (maxIt_); \
    constexpr bool RLAZY = PRIV != 2; \
    const bool skipRays = RLAZY && layerSkipOn; \
    int it = 0; \
    for (;;) { \
      int nGo = __popcll(__ballot(ract && rpend == 0)); \
      while (nGo > 0 && it < maxIt) { \
        ++it; \
        if (ract && rpend == 0) { \
          const bool yLtX = rty < rtx; \
          const float m2 = yLtX ? rty : rtx; \
          const bool isZ = rtz < m2; \
          const float tmin = isZ ? rtz : m2; \
          const float accNew = racc + (tmin - rcur) * rext; \
          if (accNew > limit) { \
            if (rphase == 1) { \
              rcur = rcur + (limit - racc) / rext; \
              racc = 0.0f; limit = tauFree; rphase = 2; \
            } else { \
              ract = false; \
            } \
          } else { \
            racc = accNew; \
            rcur = tmin; \
            if (!(rcur <= p.rayMaxLen)) {  /* longer than any ray can be (or NaN): dropped, counted */ \
              ract = false; atomicAdd(p.bad, 1ull); atomicOr(p.bad + 7, 1ull << (DROP_RAY - 1u)); \
              record_first_drop(p.bad, DROP_RAY, 1u, idLo, idHi, rd, event); \
            } \
            else if (isZ) { \
              rez += sgZ; \
              if (rez > offZ + p.nz) { ract = false; outTop = true; } \
              else if (rez < offZ) { ract = false; outBottom = true; } \
              else rcell += sgZ * ncol; \
            } else if (yLtX) { \
              rey += sgY; \
              rcell += sgY * p.nx; \
              if (rey > offY + p.ny) { rey = offY + 1; rcell -= ncol; qy -= p.Ly; } \
              else if (rey < offY) { rey = offY + p.ny - 1; rcell += ncol; qy += p.Ly; } \
            } else { \
              rex += sgX; \
              rcell += sgX; \
              if (rex > p.nx) { rex = 1; rcell -= p.nx; qx -= p.Lx; } \
              else if (rex < 0) { rex = p.nx - 1; rcell += p.nx; qx += p.Lx; } \
            } \
            if (ract) { \
              if (gridLds) rext = s_ext[rcell]; \
              else { \
                const float lv = s_bgExt[rez - offZ - (sgZ > 0 ? 1 : 0)]; \
                if (skipRays && jvz != 0.0f && isZ && (lv >= 0.0f) != rlazy) rpend = rlazy ? 2 : 1; \
                rext = lv; \
                if (lv < 0.0f && rpend == 0) rext = p.ext[rcell]; \
              } \
              const int eSel = isZ ? rez : (yLtX ? rey : rex); \
              const double origin = isZ ? rpz : (yLtX ? qy : qx); \
              const float jv = isZ ? jvz : (yLtX ? jvy : jvx); \
              const float tNew = (float)(s_edge[eSel] - origin) * jv; \
              rtz = isZ ? tNew : rtz; \
              rty = (!isZ && yLtX) ? tNew : rty; \
              rtx = (!isZ && !yLtX) ? tNew : rtx; \
            } \
          } \
        } \
        nGo = __popcll(__ballot(ract && rpend == 0)); \
        if (RLAZY && __popcll(__ballot(ract && rpend != 0)) >= 16) break; \
      } \
      if (!RLAZY || __ballot(ract && rpend != 0) == 0ull) break; \
      if (ract && rpend == 1) { \
        const int k = rez - offZ - (sgZ > 0 ? 1 : 0); \
        const int run = s_run[k]; \
        const int fEnd = sgZ > 0 ? (run >> 16) : (run & 0xffff); \
        const double dT = sgZ > 0 ? s_runT[fEnd] - s_runT[k + 1] : s_runT[k] - s_runT[fEnd]; \
        const float accEnd = racc + (rtz - rcur) * rext + (float)dT * fabsf(jvz); \
        rlazy = true; \
        rtx = FLT_MAX; rty = FLT_MAX; \
        rpend = 0; \
        if (accEnd <= limit) { \
          racc = accEnd; \
          rcur = (float)(s_edge[offZ + fEnd] - rpz) * jvz; \
          if (sgZ > 0) { rez = offZ + fEnd + 1; if (fEnd == p.nz) { ract = false; outTop = true; } else rpend = 2; } \
          else { rez = offZ + fEnd - 1; if (fEnd == 0) { ract = false; outBottom = true; } else rpend = 2; } \
          rtz = (float)(s_edge[min(max(rez, offZ), offZ + p.nz)] - rpz) * jvz; \
        } \
      } \
      if (ract && rpend == 2) { \
        const double xw = qx + (double)rcur * (double)ddx, yw = qy + (double)rcur * (double)ddy; \
        const int jx = locate_periodic(s_edge, p.nx, p.x0, p.Lx, p.invLx, p.invCellX, p.xyNearUniform != 0, qx, xw); \
        const int jy = locate_periodic(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, p.invCellY, p.xyNearUniform != 0, qy, yw); \
        rex = jx + (sgX > 0 ? 1 : 0); \
        rey = offY + jy + (sgY > 0 ? 1 : 0); \
        rtx = jvx != 0.0f ? (float)(s_edge[rex] - qx) * jvx : FLT_MAX; \
        rty = jvy != 0.0f ? (float)(s_edge[rey] - qy) * jvy : FLT_MAX; \
        rcell = jx + p.nx * (jy + p.ny * (rez - offZ - (sgZ > 0 ? 1 : 0))); \
        rext = p.ext[rcell]; \
        rlazy = false; \
        rpend = 0; \
      } \
      if (it >= maxIt && __ballot(ract && rpend != 0) == 0ull) break; \
    } \
  } while (0)
  // the contribution of a finished ray and its tally (:1745-1826); ord: the ray's scattering order (ORD).  (The order comes in as
  // an argument, and the lambdas name no variable of their own for it: a capture would change the order-blind kernels' code.)
  auto rayFinish = [&](int ord) __attribute__((always_inline)) {
    constexpr float kPi = 3.14159265358979312f;
    if (PRIV != 2 && rlazy && (outTop || outBottom)) {  // a ray that left the domain on the layer-skipping walk: its exit column
      const double xw = qx + (double)rcur * (double)ddx, yw = qy + (double)rcur * (double)ddy;
      const int jx = locate_periodic(s_edge, p.nx, p.x0, p.Lx, p.invLx, p.invCellX, p.xyNearUniform != 0, qx, xw);
      const int jy = locate_periodic(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, p.invCellY, p.xyNearUniform != 0, qy, yw);
      rcell = jx + p.nx * jy + (outTop ? ncol * (p.nz - 1) : 0);
    }
    float contrib = 0.0f;
    if (!p.useRRIntensity) {  // :1745-1752 transmission to the boundary the ray leaves through
      contrib = (rW * rNpf) * expf(-racc);
    } else if (kPi * rNpf <= p.zetaMin) {  // :1760-1775
      if (u2 <= kPi * rNpf / p.zetaMin && outTop) contrib = rW * p.zetaMin / kPi;
    } else if (outTop) {  // :1782-1806
      contrib = rphase == 1 ? (rW * rNpf) * expf(-racc) : rW * p.zetaMin / kPi;
    }
    if (contrib != 0.0f && (outTop || outBottom)) {  // (a truncated Legendre series can go negative: tallied as is)
      const int col = outTop ? rcell - ncol * (p.nz - 1) : rcell;
      const long long ibase = slab_intensity_start<long long>(ncol, p.nz);  // [intensity nDir*ncol | byComponent (nc+1)*nDir*ncol | excess (nc+1)*nDir]
      long long *slab = tally_slab<PRIV>(s_slab, p, rbatch);
      if (p.limitContrib && contrib > p.maxContrib) {  // :1815-1826 keep track of the excess per direction and component
        const unsigned long long ex = (unsigned long long)__double2ll_rn((double)(contrib - p.maxContrib) * kTallyScale);
        deposit(slab + ibase + (long long)(nc + 2) * p.nDir * ncol + (long long)rcomp * p.nDir + rd, ex);
        contrib = p.maxContrib;
      }
      const unsigned long long dep = (unsigned long long)__double2ll_rn((double)contrib * kTallyScale);
      deposit(slab + ibase + (long long)rd * ncol + col, dep);
      if (p.limitContrib)
        deposit(slab + ibase + ((long long)(1 + rcomp) * p.nDir + rd) * ncol + col, dep);
      if constexpr (ORD) {  // intensityByScatOrd (limitIntensityContributions is refused together with orders)
        if (ord <= p.numRecScatOrd) {
          const long long ordI = slab_orders_start<long long>(ncol, p.nz, p.nDir, p.numRecScatOrd + 1, 2);  // (ordInten)
          deposit(slab + ordI + ((long long)ord * p.nDir + rd) * ncol + col, dep);
        }
      }
    }
  };
  // ray record in the wave's buffer, 5 x 16 bytes: {qx, qy} {pz, rcur, racc} {limit, tauFree, u2, rext} {weight, npf, rex | rey << 16,
  // rez | phase << 16 | lazy << 18 | pend << 19} {cell, direction | component << 16, batch, scattering order (ORD)}; face distances are recomputed
  auto rayStore = [&](int slot, unsigned ordWord) __attribute__((always_inline)) {
    uint4 *r = s_rays + 5 * slot;
    r[0] = make_uint4((unsigned)__double2loint(qx), (unsigned)__double2hiint(qx), (unsigned)__double2loint(qy), (unsigned)__double2hiint(qy));
    r[1] = make_uint4((unsigned)__double2loint(rpz), (unsigned)__double2hiint(rpz), __float_as_uint(rcur), __float_as_uint(racc));
    r[2] = make_uint4(__float_as_uint(limit), __float_as_uint(tauFree), __float_as_uint(u2), __float_as_uint(rext));
    r[3] = make_uint4(__float_as_uint(rW), __float_as_uint(rNpf), (unsigned)rex | ((unsigned)rey << 16),
                      (unsigned)rez | ((unsigned)rphase << 16) | ((rlazy ? 1u : 0u) << 18) | ((unsigned)rpend << 19));
    r[4] = make_uint4((unsigned)rcell, (unsigned)rd | ((unsigned)rcomp << 16), rbatch, ordWord);
  };
  // finishes the rays in the wave's buffer: one dense lockstep pass over up to 64 long rays of mixed directions
  // (a macro, not a lambda: a closure that calls the other closures keeps the lane state in scratch memory)
#define MCBRAT_RAY_PASS() do { \
    const int n_ = rayCount; \
    rayCount = 0; \
    ract = lane < n_; \
    outTop = false; outBottom = false; \
 \
    qx = 0.0; qy = 0.0; rpz = 0.0; rcur = 0.0f; racc = 0.0f; limit = 0.0f; tauFree = 0.0f; u2 = 0.0f; rext = 0.0f; rW = 0.0f; rNpf = 0.0f; \
    rex = 0; rey = 0; rez = 0; rcell = 0; rphase = 0; rpend = 0; rd = 0; rcomp = 0; rbatch = 0u; rlazy = false; \
    ddx = 0.0f; ddy = 0.0f; ddz = 1.0f; jvx = 0.0f; jvy = 0.0f; jvz = 0.0f; sgX = 1; sgY = 1; sgZ = 1; \
    rtx = FLT_MAX; rty = FLT_MAX; rtz = FLT_MAX; \
    if (ract) { \
      const uint4 *r = s_rays + 5 * lane; \
      const uint4 a0 = r[0], a1 = r[1], a2 = r[2], a3 = r[3], a4 = r[4]; \
      qx = __hiloint2double((int)a0.y, (int)a0.x); qy = __hiloint2double((int)a0.w, (int)a0.z); \
      rpz = __hiloint2double((int)a1.y, (int)a1.x); rcur = __uint_as_float(a1.z); racc = __uint_as_float(a1.w); \
      limit = __uint_as_float(a2.x); tauFree = __uint_as_float(a2.y); u2 = __uint_as_float(a2.z); rext = __uint_as_float(a2.w); \
      rW = __uint_as_float(a3.x); rNpf = __uint_as_float(a3.y); \
      rex = (int)(a3.z & 0xffffu); rey = (int)(a3.z >> 16); \
      rez = (int)(a3.w & 0xffffu); rphase = (int)((a3.w >> 16) & 3u); rlazy = ((a3.w >> 18) & 1u) != 0u; rpend = (int)((a3.w >> 19) & 3u); \
      rcell = (int)a4.x; rd = (int)(a4.y & 0xffffu); rcomp = (int)(a4.y >> 16); rbatch = a4.z; \
      if constexpr (ORD) rord = (int)a4.w; \
      const float *dd = p.dirData + 8 * rd; \
      ddx = dd[0]; ddy = dd[1]; ddz = dd[2]; jvx = dd[4]; jvy = dd[5]; jvz = dd[6]; \
      sgX = ddx >= 0.0f ? 1 : -1; sgY = ddy >= 0.0f ? 1 : -1; sgZ = ddz >= 0.0f ? 1 : -1; \
      rtx = (rlazy || jvx == 0.0f) ? FLT_MAX : (float)(s_edge[rex] - qx) * jvx; \
      rty = (rlazy || jvy == 0.0f) ? FLT_MAX : (float)(s_edge[rey] - qy) * jvy; \
      rtz = jvz != 0.0f ? (float)(s_edge[min(max(rez, offZ), offZ + p.nz)] - rpz) * jvz : FLT_MAX; \
    } \
    MCBRAT_RAY_WALK(p.rayPassIters); \
    { \
      const unsigned long long mLeft_ = __ballot(ract); \
      if (ract) rayStore(__popcll(mLeft_ & laneBelow), ORD ? (unsigned)rord : 0u); \
      rayCount = __popcll(mLeft_); \
      if (lane < n_ && !ract) rayFinish(ORD ? rord : 0); \
    } \
  } while (0)

  // Watchdog (wave-uniform, scalar): loop iterations in which no lane of the wave started a leg, took a new photon or was
  // refused one.  Legs per photon and photons per launch are bounded, so with this bound the loop ends whatever a lane's
  // state does; when it fires, every lane that is not dead has been on one leg for that many iterations and is dropped.
  unsigned sinceProgress = 0;
  const unsigned maxEvents = (DEBUG || kTestBounds) ? p.maxEvents : kMaxEvents, maxEventsNaN = (DEBUG || kTestBounds) ? p.maxEventsNaN : kMaxEventsNaN,
                 watchdog = (DEBUG || kTestBounds) ? p.watchdog : kWatchdog;
  for (unsigned long long unit = blockIdx.x;; unit += gridDim.x) {
    if (PRIV) {  // workgroup-uniform
      if (unit >= p.nUnits) break;
      const unsigned long long b = unit / p.unitsPerBatch, s = unit % p.unitsPerBatch;
      const unsigned long long bp = (p.total - b * p.ppb) < p.ppb ? (p.total - b * p.ppb) : p.ppb;
      const unsigned long long lo = (bp * s) / p.unitsPerBatch, hi = (bp * (s + 1)) / p.unitsPerBatch;
      unitFirst = b * p.ppb + lo;
      unitCount = (unsigned)(hi - lo);
      unitSlab = p.slabs + b * p.slabStride;
      batch = (uint32_t)b;
      more = true;
    }

    for (;;) {
      // ================= event phase: every lane that is not walking =====================
      bool needLeg = false;

      // Launches, exits (top / surface) and the transitions of the layer-skipping walk are rare next to collisions (1, 1
      // and a few per ~20 legs).  Serving them whenever a single lane asks would run their code at a few percent lane
      // occupancy in almost every event phase, so each kind waits until enough lanes have queued up -- or until the
      // wave has little else to do.
      const int nBusy = __popcll(__ballot(state == ST_WALK || state == ST_COLLIDE));
      const bool idle = nBusy < p.eventThreshold;
      const unsigned long long mSurf = __ballot(state == ST_SURFACE || state == ST_TOP);  // exits
      const bool doSurface = __popcll(mSurf) >= p.surfaceThreshold || idle;
      if (LAZY) {
        const bool doJump = __popcll(__ballot(state == ST_JUMP || state == ST_ENTER)) >= p.jumpThreshold || idle;
        if (state == ST_JUMP && doJump) MCBRAT_SERVE_JUMP();
        // Lanes that come out of the layer-skipping walk: x/y state from the position the walk has reached -- the
        // collision point, the exit point (when exits are served), or the face of the layer with cell-to-cell
        // extinction (ST_ENTER, when those are served).
        const bool exitNow = (state == ST_TOP || state == ST_SURFACE) && doSurface;
        if (lazy && (state == ST_COLLIDE || exitNow || (state == ST_ENTER && doJump))) resolveXY();
        if (FLY && stride != 1 && (exitNow || state == ST_COLLIDE || (state == ST_ENTER && doJump))) resolveFly();
      }
      // 0-based cell of a waiting lane: the face ahead minus one where the leg runs forward
      int ix = ex - (dx >= 0.0f ? 1 : 0), iy = ey - offY - (dy >= 0.0f ? 1 : 0), iz = ez - offZ - (dz >= 0.0f ? 1 : 0);
      if (DEBUG) {
        wEventPhases++;
        wEventLanes += __popcll(__ballot(state == ST_COLLIDE));
        if (doSurface && mSurf) wSurfPhases++;
      }
      STAMP(8);
      // ---- exits: out the top (computeRT :573-617) or down to the surface (:619-676) -----------
      // Rare next to collisions (0.3 and 0.7 per ~17 legs on the step cloud): served together when enough lanes have
      // queued up.  They come BEFORE the launches: under a black surface every exit frees its lane, and the lanes
      // that have just left are refilled in the same phase instead of queueing once more.
      if (state == ST_TOP && doSurface) {
        // out the top: tally and free the lane
        const unsigned long long dep = weight_fixed<BRDF>(w);
        deposit(tally_slab<PRIV>(s_slab, p, batch) + (ix + p.nx * iy), dep);
        if constexpr (ORD) {  // fluxUpByScatOrd: the order the photon leaves with
          if (nScat <= p.numRecScatOrd) deposit(tally_slab<PRIV>(s_slab, p, batch) + ordUp + (long long)ncol * nScat + (ix + p.nx * iy), dep);
        }
        if constexpr (LVL) MCBRAT_LEVEL_DEPOSIT(lvlUp, p.nz, ix + p.nx * iy, dep);  // the top exit is an upward crossing of level nz
        if (DEBUG) {
          cTop++;
          record_fate(p, idLo, idHi, 0, ix + 1, iy + 1, p.nz + 1, nScat, nLegs, w);
        }
        MCBRAT_FLUSH_PENDING();
        state = ST_DEAD;
      }
      if (state == ST_SURFACE && doSurface) {
        // surface, computeRT :619-676 (Lambertian); fluxDown gets the incident weight :634
        px = px + (double)tcur * (double)dx;  // where the leg met z0 (:1809-1812)
        py = py + (double)tcur * (double)dy;
        pz = p.zSurf;
        iz = 0;
        cell = ix + p.nx * iy;
        const unsigned long long dep = weight_fixed<BRDF>(w);
        deposit(tally_slab<PRIV>(s_slab, p, batch) + ncol + (ix + p.nx * iy), dep);
        if constexpr (ORD) {  // fluxDownByScatOrd: the order before the reflection (computeRT :635-643)
          if (nScat <= p.numRecScatOrd) deposit(tally_slab<PRIV>(s_slab, p, batch) + ordDown + (long long)ncol * nScat + (ix + p.nx * iy), dep);
        }
        if constexpr (DIRECT) MCBRAT_LEVEL_DEPOSIT(event == 1u ? lvlDirect : lvlDown, 0, ix + p.nx * iy, dep);  // (still direct: the reflection below ends it)
        else if constexpr (LVL) MCBRAT_LEVEL_DEPOSIT(lvlDown, 0, ix + p.nx * iy, dep);  // the arrival is a downward crossing of level 0
        if (DEBUG && p.traceBuf && photon_index(p, idLo, idHi) == p.traceIndex && nScat < p.traceCap) {
          double *t = p.traceBuf + 12 * nScat;  // (development aid: the landing point of the traced photon, marked by a negative layer)
          t[0] = event; t[1] = ix + 1; t[2] = iy + 1; t[3] = -1; t[4] = px; t[5] = py; t[6] = pz;
          t[7] = dx; t[8] = dy; t[9] = dz; t[10] = extCur; t[11] = w;
        }
        nScat++;
        if (DEBUG) cSurf++;
        // Cosine of the Lambertian reflection: sqrt(X) of the leg's block; below 2 FLT_MIN, Z, then blocks 2.. of the leg's event.
        // (The same lines stand in trace_block_kernel, mcbrat_blockwalk.hip: as one function of mcbrat_photon.h they cost this
        // kernel's general instantiation 16 bytes of scratch and the 768-lane block walk two registers, however the function was shaped.)
        float mu = sqrtf(uX);
        if (!(fabsf(mu) > 2.0f * FLT_MIN)) {
          mu = sqrtf(uZ);
          uint32_t r[4];
          for (uint32_t j = 0; !(fabsf(mu) > 2.0f * FLT_MIN); j++) {
            if ((j & 3u) == 0) rng(event, 2u + (j >> 2), r);
            mu = sqrtf(u01(pick4(r, j & 3u)));
          }
        }
        const float wIn = w;
        int patch = 0;
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        if constexpr (BRDF) {  // the Lambertian draw of the direction, the weight times R(d_in, d_out) of the patch
          lambert_direction(mu, uY, ox, oy, oz);
          patch = surface_patch(p, px, py);
          const float4 s = surface_reflect_call(p.surfKind, reinterpret_cast<const float4 *>(p.surfRefl)[patch], dx, dy, dz, ox, oy, oz, event, idLo, idHi, p.seedLo, p.seedHi);
          ox = s.x; oy = s.y; oz = s.z;  // (the Lambertian draw as it went in, but for a glint-sampled direction)
          w = w * s.w;
          // local estimates from a BRDF reflection: the weight before it and R(d_in, d_view) / pi (iFlag -1; iEntry: the patch).
          // Also when R(d_in, d_out) = 0 ends the photon: the estimate does not depend on the direction drawn.
          if (INTEN) { iFlag = -1; iW = wIn; iDx = dx; iDy = dy; iDz = dz; iEntry = patch; }
        } else if (surfaceDescription) w = w * surface_reflectance(p, px, py);  // useSurfaceBDRF :667-670
        else w = (float)((double)w * (double)p.albedo);              // :673
        if (w <= FLT_MIN) {
          if (DEBUG) record_fate(p, idLo, idHi, 1, ix + 1, iy + 1, 1, nScat, nLegs, wIn);
          MCBRAT_FLUSH_PENDING();
          state = ST_DEAD;
        } else if constexpr (BRDF) {
          dx = ox; dy = oy; dz = oz;
          needLeg = true;
        } else {
          lambert_direction(mu, uY, dx, dy, dz);
          needLeg = true;
          if constexpr (LVL) MCBRAT_LEVEL_DEPOSIT(lvlUp, 0, ix + p.nx * iy, weight_to_fixed(w));  // the reflected photon crosses level 0 upward
          if (INTEN) { iFlag = 1; iW = w; }  // :680-702 reflected weight, Lambertian
        }
      }
      // (BRDF radiance: a lane whose photon R(d_in, d_out) = 0 has just ended keeps its state until its local estimate has gone out)
      const bool hold = BRDF && INTEN && iFlag == -1;
      const unsigned long long mDead = __ballot(state == ST_DEAD && more && !hold);
      const bool doLaunch = __popcll(mDead) >= p.launchThreshold || nBusy < p.eventThreshold;
      const unsigned long long want = doLaunch ? mDead : 0ull;
      if (DEBUG && want) wLaunchPhases++;
      STAMP(5);
      if (want != 0ull) {  // wave-uniform
        const int nWant = __popcll(want);
        const int rank = __popcll(want & laneBelow);
        unsigned long long myIdx;  // photon index inside this launch
        bool valid;
        if (PRIV) {
          unsigned base = 0;
          if (lane == 0) base = atomicAdd(&s_cursor[0], (unsigned)nWant);
          base = (unsigned)__shfl((int)base, 0);
          const unsigned k = base + (unsigned)rank;
          valid = k < unitCount;
          myIdx = unitFirst + k;
        } else {
          myIdx = chunkNext + (unsigned long long)rank;
          const unsigned long long avail = chunkEnd - chunkNext;
          if (avail < (unsigned long long)nWant) {  // wave-uniform: take a new chunk
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(p.counter, (unsigned long long)kChunk);
            const uint32_t bl = __shfl((int)(uint32_t)base, 0), bh = __shfl((int)(uint32_t)(base >> 32), 0);
            base = ((unsigned long long)bh << 32) | bl;
            if ((unsigned long long)rank >= avail) myIdx = base + ((unsigned long long)rank - avail);
            chunkNext = base + ((unsigned long long)nWant - avail);
            chunkEnd = base + kChunk;
          } else {
            chunkNext += (unsigned long long)nWant;
          }
          valid = myIdx < p.total;
        }
        if (state == ST_DEAD && more && !hold) {
          if (valid) {
            // ---- launch: getNextPhoton + computeRT :466-508 --------------------------------
            if (!PRIV) batch = (uint32_t)(myIdx / p.ppb);
            const unsigned long long id = p.firstPhoton + myIdx;
            idLo = (uint32_t)id; idHi = (uint32_t)(id >> 32);
            event = 0; nScat = 0; nLegs = 0;
            double fx, fy, fz;  // fractional launch position in [0,1]
            if (!EMIT) {  // (the SPEC kernels' only kind of solar source: Directional)
              fz = 0.0;
              launch_solar(p, SPEC != 0 || p.solarKind == 0, rng, fx, fy, dx, dy, dz);
            } else {
              launch_emission(p, rng, [&](float rn, int &ik, int &ij) { emission_level_row(p, rn, ik, ij); }, fx, fy, fz, dx, dy, dz);
            }
            w = 1.0f;
            px = p.x0 + fx * (p.xMax - p.x0);  // :480-482
            py = p.y0 + fy * (p.yMax - p.y0);
            if (p.xyRegular) {  // findXYIndicies :1558-1562
              ix = min((int)((px - p.x0) * p.invDX), p.nx - 1);
              iy = min((int)((py - p.y0) * p.invDY), p.ny - 1);
            } else {
              ix = find_cell(s_edge, p.nx, px);
              iy = find_cell(s_edge + offY, p.ny, py);
            }
            if (!EMIT) {
              pz = p.zLaunch; iz = p.izLaunch;
            } else {
              launch_height(p, p.zRegular != 0, s_edge + offZ, fz, pz, iz);
            }
            cell = ix + p.nx * (iy + p.ny * iz);
            extCur = gridLds ? s_ext[cell] : load_ext<BRICK>(p, s_bgExt, locate_cell<BRICK>(p, ix, iy, iz), iz);
            brickId = -1;
            if (EMIT && p.lwFlag && pz > 0.0) deposit(tally_slab<PRIV>(s_slab, p, batch) + 2 * ncol + cell, to_fixed(-1.0));  // :504-508 emission counts as negative absorption
            if constexpr (LVL) {
              // a solar launch lies just inside the top cell: it counts as the downward crossing of level nz the walk never makes;
              // a surface-emitted thermal photon (fz = 0 exactly: an atmospheric launch has fz > 0) crosses level 0 upward
              if (!EMIT) MCBRAT_LEVEL_DEPOSIT(DIRECT ? lvlDirect : lvlDown, p.nz, ix + p.nx * iy, 1ull << 32);  // (DIRECT: level nz is all direct)
              else if (fz == 0.0) MCBRAT_LEVEL_DEPOSIT(lvlUp, 0, ix + p.nx * iy, 1ull << 32);
            }
            if (INTEN && EMIT && p.lwFlag) { iFlag = pz == 0.0 ? 1 : 2; iW = w; }  // :510-541 emission seen directly
            needLeg = true;
          } else {
            more = false;
          }
        }
      }
      STAMP(0);
      if (state == ST_COLLIDE) {
        // scattering event, computeRT :703-821 (the zero-extinction back-step :728-754 cannot
        // arise: a collision is only declared inside a cell with extinction > 0)
        {  // opticalProperties.f95:1729-1738: the point inside the cell where tau is used up
          if constexpr (ACT) MCBRAT_ACTINIC_DEPOSIT(cell, w, div_fast(tau - acc, fabsf(extCur)));  // the piece tc - tcur, at the weight the leg carried
          const double s = (double)(tcur + div_fast(tau - acc, fabsf(extCur)));
          px = px + s * (double)dx;
          py = py + s * (double)dy;
          pz = pz + s * (double)dz;
        }
        if (DEBUG && p.traceBuf && photon_index(p, idLo, idHi) == p.traceIndex && nScat < p.traceCap) {
          double *t = p.traceBuf + 12 * nScat;  // one record per collision of the traced photon
          t[0] = event; t[1] = ix + 1; t[2] = iy + 1; t[3] = iz + 1; t[4] = px; t[5] = py; t[6] = pz;
          t[7] = dx; t[8] = dy; t[9] = dz; t[10] = tau; t[11] = w;
        }
        nScat++;
        if (DEBUG) cColl++;
        CellRef cr;
        cr.dense = cell;
        cr.stored = -1;
        if (BRICK) cr = locate_cell<BRICK>(p, ix, iy, iz);
        // optics of this cell: dense grid, stored brick, or the layer's background record
        const long long nvox = BRICK ? (cr.stored >= 0 ? p.nStored : (long long)p.nz) : (long long)ncol * p.nz;
        const int oc = BRICK ? (cr.stored >= 0 ? cr.stored : iz) : cell;
        const float *cumA = gridLds ? s_cum : ((BRICK && cr.stored < 0) ? p.bgCum : p.cum);
        const float *ssaA = gridLds ? s_ssa : ((BRICK && cr.stored < 0) ? p.bgSsa : p.ssa);
        const uint16_t *pfiA = gridLds ? s_pfi : ((BRICK && cr.stored < 0) ? p.bgPfi : p.pfi);
        int c = 0;  // component pick :759-760 (findIndex over [0, cumExt(:)]), uniform = slot Z of the leg's block
        float ssa;
        int pfEntry;
        if (!BRICK && !gridLds && useRec) {
          // dense grids with one or two components: cumulative fraction, both albedos and both phase-function
          // indices of the cell come in ONE 16-byte gather instead of three dependent ones
          const uint4 rc = p.rec[cell];
          c = uZ >= __uint_as_float(rc.x) ? 1 : 0;  // (one component: the host stores 2.0 here, never reached)
          ssa = __uint_as_float(c ? rc.z : rc.y);
          pfEntry = (int)(c ? (rc.w >> 16) : (rc.w & 0xffffu));
        } else {
          if (nc > 1) {  // (the component pick: one of the HOT ROWS below)
            for (int k = 0; k < nc - 1; k++)
              if (uZ >= cumA[(long long)k * nvox + oc]) c = k + 1;
          }
          ssa = ssaA[(long long)c * nvox + oc];
          pfEntry = pfiA[(long long)c * nvox + oc];
        }
        if (ssa < 1.0f) {  // absorption :765-771
          const unsigned long long dep = weight_fixed<BRDF>(w * (1.0f - ssa));
#ifdef MCBRAT_NO_COMBINE  // A/B: every deposit goes out as its own atomic add
          constexpr bool combine = false;
#else
          constexpr bool combine = !PRIV;  // (the pending deposit above: tallies in global memory)
#endif
          if (!combine) deposit(tally_slab<PRIV>(s_slab, p, batch) + 2 * ncol + cell, dep);
          else if (cell == pendCell) pendDep += dep;
          else { MCBRAT_FLUSH_PENDING(); pendCell = cell; pendDep = dep; }
          w = w * ssa;
          if (DEBUG) cAbs++;
        }
        if (INTEN) {  // :776-790: weight after the single scattering albedo, before roulette; incoming direction
          iFlag = 3 + c; iW = w; iDx = dx; iDy = dy; iDz = dz;
          iEntry = s_fwdOffset[c] + pfEntry * s_fwdNAngles[c];
        }
        // HOT ROWS.  The component pick above and, from here to the leg set-up, roulette, scattering angle, new direction and the
        // leg's draws with the zero-cosine rule stand in trace_block_kernel too (mcbrat_blockwalk.hip, HOT ROWS): a change to one
        // of them is made in both.  (As functions of mcbrat_photon.h called from here, they changed this kernel's register
        // allocation into one whose radiance-by-order instantiations misreport dropped photons: DESIGN.md section 4.18.)
        if (useRR && w < 0.5f) {  // Russian roulette :805-811, RussianRouletteW = 1
          float uR = uZ;  // one component: Z decides nothing at the component pick and serves here (no second block)
          if (nc != 1) {  // (wave-uniform)
            uint32_t r1[4];
            rng(event, 1u, r1);
            uR = u01(r1[1]);
          }
          if (uR >= w) { w = 0.0f; if (DEBUG) cKill++; }
          else { w = 1.0f; if (DEBUG) cSurv++; }
        }
        STAMP(2);
        if (w <= FLT_MIN) {  // :812
          if (DEBUG) record_fate(p, idLo, idHi, 2, ix + 1, iy + 1, iz + 1, nScat, nLegs, 0.0f);
          MCBRAT_FLUSH_PENDING();
          state = ST_DEAD;
        } else {
          const int n = s_tblNSteps[c];
          // computeScatteringAngle :1594-1621 (table point count N, floor-type lookup as written)
          const float *t = tbl + s_tblOffset[c] + (long long)pfEntry * n;
          const int ai = (int)(uX * (float)n) + 1;
          float ang;
          if (ai < n) {
#ifdef MCBRAT_PRECISE_MATH
            const float left = uX - (float)(ai - 1) / (float)n;
#else
            const float left = uX - (float)(ai - 1) * s_tblInvN[c];
#endif
            ang = (1.0f - left) * t[ai - 1] + left * t[ai];
          } else {
            ang = t[n - 1];
          }
#ifdef MCBRAT_PRECISE_MATH
          const float cs = cosf(ang);
#else
          const float cs = cos_0_pi(ang);
#endif
          STAMP(3);
          // next_direct :1921-1948 with (AX, AY)/sqrt(D) = (cos, sin) of a uniform azimuth
          float AX, AY;
          sincos_2pi(uY, AX, AY);
#ifdef MCBRAT_PRECISE_MATH
          float B = sqrtf(1.0f - cs * cs);
#else
          float B = __builtin_amdgcn_sqrtf(1.0f - cs * cs);
#endif
          AX = AX * B;
          AY = AY * B;
          B = dx * AX - dy * AY;
          float D = cs - div_fast(B, 1.0f + fabsf(dz));
          dx = dx * D + AX;
          dy = dy * D - AY;
          dz = dz * cs - copysignf(fabsf(B), dz * B);
          needLeg = true;
          STAMP(4);
        }
      }
      STAMP(4);
      // ---- local estimates: one ray per view direction from every lane with a pending contribution ----
      // All rays of a direction are parallel, so the lanes of the wave walk them in lockstep.  Most rays end within a
      // few cells (roulette inside a cloud); the few that cross a whole cloud field would keep the wave in the loop
      // at a few percent lane occupancy, so after a few (rayShort) iterations what is left of a ray is put into the wave's
      // LDS ray buffer and finished later, together with other long rays, in a pass of its own (rayPass).
      if (INTEN) {
        // (no ray from a position that is NaN: a photon that drew a NaN from the inverse table -- a reference quirk, DESIGN.md
        // section 8 -- collides on in its cell with a NaN direction and, from its next collision, a NaN position; a ray that
        // starts there has NaN face distances and would circle the periodic domain for ever.  In the reference its
        // contribution would be NaN too.)
        if (iFlag != 0 && !(px == px)) iFlag = 0;
        if (__ballot(iFlag != 0) != 0ull) {
          constexpr float kPi = 3.14159265358979312f;
          for (int d = 0; d < p.nDir; ++d) {
            if (p.rayCap > 0 && rayCount >= p.rayPassAt) MCBRAT_RAY_PASS();  // (wave-uniform)
            const float *dd = p.dirData + 8 * d;  // uniform address: scalar loads
            const float fourPiMu = dd[3];
            ddx = dd[0]; ddy = dd[1]; ddz = dd[2]; jvx = dd[4]; jvy = dd[5]; jvz = dd[6];
            sgX = ddx >= 0.0f ? 1 : -1; sgY = ddy >= 0.0f ? 1 : -1; sgZ = ddz >= 0.0f ? 1 : -1;
            ract = iFlag != 0;
            float npf = 0.0f;  // normalizedPhaseFunc :1685-1727
            if (iFlag == 1) npf = 1.0f / kPi;
            else if (iFlag == 2) npf = 1.0f / fourPiMu;
            else if (iFlag >= 3) {
              float proj = iDx * ddx + iDy * ddy + iDz * ddz;
              if (fabsf(proj) > 1.0f) proj = copysignf(1.0f, proj);
              const float ang = acosf(proj);
              const int nA = s_fwdNAngles[iFlag - 3];
              const float *t = ((p.useHybrid && nScat <= p.numOrdersOrig) ? p.fwdOrig : p.fwdTables) + iEntry;
              const float deltaTheta = kPi / (float)(nA - 1);  // lookUpPhaseFuncValsFromTable :1835-1870
              const int ai = (int)(ang / deltaTheta) + 1;
              float val;
              if (ai < nA) {
                const float wt = 1.0f - (ang - (float)(ai - 1) * deltaTheta) / deltaTheta;
                val = wt * t[ai - 1] + (1.0f - wt) * t[ai];
              } else {
                val = t[nA - 1];
              }
              npf = val / fourPiMu;
            }
            if constexpr (BRDF) {
              if (iFlag == -1) npf = surface_brdf(p, iEntry, iDx, iDy, iDz, ddx, ddy, ddz) / kPi;
            }
            // Iwabuchi (2006) roulette :1753-1813: phase 2 = free path tauFree, phase 1 = tauMax first
            limit = FLT_MAX; tauFree = 0.0f; u2 = 0.0f;
            rphase = 0;
            if (p.useRRIntensity && ract) {
              uint32_t r[4];
              philox4x32_10(event, 0x100u + (uint32_t)d, idLo, idHi, p.seedLo, p.seedHi, r);
              tauFree = -logf(fmaxf(FLT_MIN, u01(r[0])));
              u2 = u01(r[1]);
              if (kPi * npf <= p.zetaMin) { rphase = 2; limit = tauFree; }
              else { rphase = 1; limit = -logf(p.zetaMin / fmaxf(FLT_MIN, kPi * npf)); }
            }
            // ray state (the photon's own walk state is left alone)
            qx = px; qy = py; rpz = pz;
            rex = ix + (sgX > 0 ? 1 : 0); rey = offY + iy + (sgY > 0 ? 1 : 0); rez = offZ + iz + (sgZ > 0 ? 1 : 0); rcell = cell;
            rtx = jvx != 0.0f ? (float)(s_edge[ract ? rex : 0] - qx) * jvx : FLT_MAX;
            rty = jvy != 0.0f ? (float)(s_edge[ract ? rey : 0] - qy) * jvy : FLT_MAX;
            rtz = jvz != 0.0f ? (float)(s_edge[ract ? rez : 0] - rpz) * jvz : FLT_MAX;
            rcur = 0.0f; racc = 0.0f;
            rext = 0.0f;
            if (ract) rext = gridLds ? s_ext[rcell] : p.ext[rcell];
            outTop = false; outBottom = false;
            rlazy = false;
            rpend = 0;
            rW = iW; rNpf = npf; rd = d; rbatch = batch;
            if constexpr (ORD) rord = nScat;  // 0 for an emission launch, the post-increment order after a reflection or a scattering
            rcomp = iFlag >= 3 ? iFlag - 2 : 0;  // 0 = surface / emission, c + 1 = component c (:535-540, :785-790)
            if (!gridLds && layerSkipOn && jvz != 0.0f && ract && s_bgExt[iz] >= 0.0f) { rlazy = true; rtx = FLT_MAX; rty = FLT_MAX; rpend = 1; }
            MCBRAT_RAY_WALK(p.rayCap > 0 ? p.rayShort : 0x7fffffff);
            bool stored = false;
            if (p.rayCap > 0) {  // what is left of the long rays: into the buffer while it has room, else finished here
              const unsigned long long mLeft = __ballot(ract);
              if (mLeft != 0ull) {
                const int slot = rayCount + __popcll(mLeft & laneBelow);
                stored = ract && slot < p.rayCap;
                if (stored) rayStore(slot, ORD ? (unsigned)rord : 0u);
                rayCount += __popcll(__ballot(stored));
                ract = ract && !stored;
                if (__ballot(ract) != 0ull) MCBRAT_RAY_WALK(0x7fffffff);
              }
            }
            if (iFlag != 0 && !stored) rayFinish(ORD ? rord : 0);
          }
          iFlag = 0;
        }
      }
      STAMP(4);
      // ---- start the next leg: tau and the per-axis face distances -------------------------
      sinceProgress = (__ballot(needLeg) != 0ull || want != 0ull) ? 0u : sinceProgress + 1u;
      if (sinceProgress > watchdog) {  // (wave-uniform; never in a run whose every lane makes progress)
        if (state != ST_DEAD) MCBRAT_DROP_PHOTON(DROP_WATCHDOG);
        sinceProgress = 0u;
      }
      // (a photon is allowed maxEvents legs; one whose direction is NaN -- a NaN entry of the reference's inverse tables,
      // DESIGN.md section 8 -- collides on in its cell until its weight is gone: that ends by itself where it loses weight
      // (roulette, or the decay to tiny(w) without it: up to 10^5 collisions, as in the reference), and never where
      // omega0 = 1 -- a photon with a NaN direction that is at full weight after maxEventsNaN = 2^20 legs is dropped.  (Full
      // weight is also what a photon has right after it survived roulette: with 4096 legs a 2000-seed soak dropped one such
      // photon -- omega0 = 0.9993, 937 collisions per roulette round -- so the budget is a million legs, about a second.)
      if (needLeg && event >= maxEventsNaN) {  // (one compare on the hot path: maxEventsNaN <= maxEvents; the rule itself in the rare branch)
        if (event >= maxEvents || !(dz == dz || w < 1.0f)) { needLeg = false; MCBRAT_DROP_PHOTON(event >= maxEvents ? DROP_LEGS : DROP_NAN_LEGS); }
      }
      if (needLeg) {
        event++;
#ifndef MCBRAT_FATE_STEPS
        nLegs++;
#endif
        if (DEBUG) cLegs++;
        uint32_t r[4];
        rng(event, 0u, r);
#ifdef MCBRAT_PRECISE_MATH
        tau = -logf(fmaxf(FLT_MIN, u01(r[0])));
#else
        tau = -0.693147182f * __builtin_amdgcn_logf(fmaxf(FLT_MIN, u01(r[0])));  // :554 (hardware log2 * ln 2; u >= 2^-32, no denormals)
#endif
        uX = u01(r[1]); uY = u01(r[2]); uZ = u01(r[3]);
        acc = 0.0f; tcur = 0.0f;
        // opticalProperties.f95:1690-1712: side 1 where direction >= 0; huge step for a zero cosine
        ex = ix + (dx >= 0.0f ? 1 : 0);
        ey = offY + iy + (dy >= 0.0f ? 1 : 0);
        ez = offZ + iz + (dz >= 0.0f ? 1 : 0);
        if (fabsf(dz) >= 2.0f * FLT_MIN) { ivz = rcp_fast(dz); tnz = (float)(s_edge[ez] - pz) * ivz; }
        else { ivz = 0.0f; tnz = FLT_MAX; }
        ivx = fabsf(dx) >= 2.0f * FLT_MIN ? rcp_fast(dx) : 0.0f;
        ivy = fabsf(dy) >= 2.0f * FLT_MIN ? rcp_fast(dy) : 0.0f;
        // a leg that starts in a layer with one extinction value only needs the z faces (a leg without a vertical
        // component never leaves its layer and keeps the face-by-face walk)
        state = ST_WALK;
        noFly = ivz == 0.0f;  // (a leg without a vertical component has no use for T(z) / mu)
        if (LAZY && layerSkipOn && ivz != 0.0f && (s_bgExt[iz] >= 0.0f || (FLY && flyOn && __float_as_int(extCur) < 0))) {
          state = ST_JUMP;  // (decided below, wave-wide)
        } else {
          tnx = ivx != 0.0f ? (float)(s_edge[ex] - px) * ivx : FLT_MAX;
          tny = ivy != 0.0f ? (float)(s_edge[ey] - py) * ivy : FLT_MAX;
        }
      }
      if (LAZY) {
        // Legs that start in a layer of one extinction value.  In a cloud field one or two lanes of a phase do (a
        // scattering in clear air): they queue with the other transitions of the layer-skipping walk and are served at the
        // head of a later phase, instead of running the jump and the column look-up here at a few percent lane occupancy.
        // In a medium made of such layers (homogeneous domains) every leg does: then the jump is taken here, densely.
        const unsigned long long mStart = __ballot(needLeg && state == ST_JUMP);
        if (__popcll(mStart) >= p.jumpThreshold && needLeg && state == ST_JUMP) {
          MCBRAT_SERVE_JUMP();
          if (state == ST_ENTER) resolveXY();
        }
      }
      // wave-uniform exit: nothing alive and every lane has already been refused a new photon.
      // (A lane that died in THIS phase still has `more` set: it gets its refill attempt next time.)
      STAMP(6);
      if (__ballot(state != ST_DEAD || more) == 0ull) {
        if (INTEN) while (rayCount > 0) MCBRAT_RAY_PASS();  // the long rays still in the wave's buffer
        break;
      }

      // ================= walk phase: one voxel face per iteration ===========================
      // accumulateExtinctionAlongPath :1697-1814.  Per axis the lane holds the index of the NEXT face
      // in the LDS edge table (ex, ey, ez) and the distance to it; `cell` is the linear cell index.
      // The crossed axis is served by its own short predicated block (add, bounds test, one LDS read),
      // so no three-way selects over the axes are needed.
      int nWalk;
      int walkIt = 0;  // (scalar) the walk loop hands over to the event phase after kWalkCap iterations at the latest: the watchdog lives there
      do {
        if (DEBUG) { wWalkIters++; wWalkLanes += __popcll(__ballot(state == ST_WALK)); }
#ifdef MCBRAT_FATE_STEPS  // development aid: the fates' nEvents field counts the photon's walk iterations instead of its legs
        if (DEBUG && state == ST_WALK) nLegs++;
#endif
        // Grids in global memory (FLATWALK): the three tests -- walking? asks for a flight? collides? -- are selects and ONE divergent
        // `if` surrounds the step, and the crossed axis is served by ONE predicated block: every divergent `if` is three or four
        // scalar instructions, and scalar issue -- one instruction per 4.25 cycles and SIMD -- is what a walk iteration of those
        // kernels spends most of its SIMD cycles on (128x128x64 +3 %, profiles/r04_experiments.txt).  The step's geometry comes
        // BEFORE the cell's extinction is looked at (+1.6 %: the gather's trip to L2 overlaps it).  The LDS-resident
        // instantiations keep the nested form, which is 5 % faster THERE (vector issue binds them).
        constexpr bool FLATWALK = PRIV != 2;
        const bool yLtX = tny < tnx;
        const float m2 = yLtX ? tny : tnx;
        const bool isZ = tnz < m2;
        const float tmin = isZ ? tnz : m2;
        if constexpr (FLATWALK) {
          // (a) The geometry of the step, for every lane, BEFORE the extinction of the cell is looked at: which face, the
          // indices beyond it, the periodic wrap, the distance to the face after it.  None of it needs the gather the
          // previous iteration sent out last, so that gather's trip to L2 overlaps all of it; the lanes that turn out to
          // collide in this cell (or to ask for a flight) simply do not commit it.  A lane that does not walk computes
          // garbage here and commits nothing (its edge index is clamped: no read outside the table).
          const bool walking = state == ST_WALK;
          const float dAx = isZ ? dz : (yLtX ? dy : dx);
          const bool fwd = dAx >= 0.0f;
          const int st = isZ ? 1 : stride;
          int e = isZ ? ez : (yLtX ? ey : ex);
          e += fwd ? st : -st;
          const int cs = isZ ? ncol : (yLtX ? p.nx : 1);  // cells per step along the axis
          const int lo = isZ ? offZ : (yLtX ? offY : 0);
          const int n = isZ ? p.nz : (yLtX ? p.ny : p.nx);
          const bool over = e > lo + n, under = e < lo;
          const bool leaves = isZ && (over || under);       // :1801-1812 through the top or the surface
          const bool wraps = walking && !isZ && (over || under);  // periodic x / y :1782-1796: continue in the next image
          int dc = fwd ? cs : -cs;
          double origin = isZ ? pz : (yLtX ? py : px);
          if (wraps) {  // (rare: one branch for both axes and ends)
            e = over ? lo + st : lo + n - st;
            dc += over ? -n * cs : n * cs;
            const double L = yLtX ? p.Ly : p.Lx;
            origin += over ? -L : L;
          }
          // Equally spaced faces: the next face of the crossed axis is one cell spacing further along the leg
          // (float, relative to the leg's start; no edge-table read, no double arithmetic).  Other axes: the
          // face position from the edge table.
          const bool spaced = isZ ? zRegularWalk : xyRegularWalk;
          float tNew = tmin + (isZ ? p.dZf * fabsf(ivz) : (float)stride * (yLtX ? p.dYf * fabsf(ivy) : p.dXf * fabsf(ivx)));
          if (!spaced) {
            const int eSel = min(max(e, lo), lo + n);
            const double edge = s_edge[eSel];
            const float iv = isZ ? ivz : (yLtX ? ivy : ivx);
            tNew = (float)(edge - origin) * iv;
          }
          __builtin_amdgcn_sched_barrier(0);
          // (b) Now the cell's extinction: does the lane reach the face?
          const float accNew = acc + (tmin - tcur) * fabsf(extCur);  // :1743
          const bool askFly = FLY && flyOn && __float_as_int(extCur) < 0 && !noFly;  // a cell outside its brick column's cloud range: ask for the clear-air flight
          const bool collides = accNew > tau;                                          // :1729-1738: the stop point inside this cell is resolved in the event phase
          state = walking ? (askFly ? ST_JUMP : (collides ? ST_COLLIDE : ST_WALK)) : state;
          if (state == ST_WALK) {  // (c) commit the step
            if constexpr (ACT) MCBRAT_ACTINIC_DEPOSIT(cell, w, tmin - tcur);  // the piece inside the cell being left (an exit through the top or the surface too)
            acc = accNew;
            tcur = tmin;
            if (DEBUG && stride == 1) cCross++;
            state = leaves ? (over ? ST_TOP : ST_SURFACE) : state;  // tallied in the event phase
            if constexpr (LVL) {  // an inner z face: level ez - offZ, in the column both its cells share (the cell left: layer ez - offZ - 1 upward)
              // (DIRECT: a first leg -- event 1 -- goes down: no solar source launches upward)
              const long long down = (DIRECT && event == 1u) ? lvlDirect : lvlDown;
              if constexpr (SIDE) {
                // ONE deposit site for whichever face the step crosses: base and bin are selects.  An x or y face: the part by
                // axis and direction of travel, the bin of the cell on the face's low side (`dc` carries the periodic wrap)
                const long long base = isZ ? (fwd ? lvlUp : down) : sideBins + sidePart * ((yLtX ? 2 : 0) + (fwd ? 0 : 1));
                const int lev = isZ ? ez - offZ : 0;
                const int bin = isZ ? cell - ncol * (ez - offZ - (fwd ? 1 : 0)) : (fwd ? cell : cell + dc);
                if (!leaves) MCBRAT_LEVEL_DEPOSIT(base, lev, bin, weight_to_fixed(w));
              } else
              if (isZ && !leaves) MCBRAT_LEVEL_DEPOSIT(fwd ? lvlUp : down, ez - offZ, cell - ncol * (ez - offZ - (fwd ? 1 : 0)), weight_to_fixed(w));
            }
            cell += leaves ? 0 : dc;
            ez = isZ ? e : ez;
            ey = (!isZ && yLtX) ? e : ey;
            ex = (!isZ && !yLtX) ? e : ex;
            if (wraps) {  // (rare) the leg's origin moves with the image
              if (yLtX) { py = origin; if (DEBUG && stride != 1) dbgV0 += over ? -p.ny : p.ny; }
              else { px = origin; if (DEBUG && stride != 1) dbgU0 += over ? -p.nx : p.nx; }
            }
            // ... then ONE extinction read for whichever axis it was (a lane that just left through the top or the
            // surface reads nothing)
            if (!BRICK) {
              // a layer with one extinction value (clear air above and below the clouds) needs no gather: every
              // scattered gather is an L2 request, and those bound large domains
              if (FLY && stride != 1) {
                if (state == ST_WALK) {
                  // z limit reached: the face where this brick column's range begins.  x/y face: the next brick column --
                  // its range begins ahead (the new z limit), lies behind (then the limit is the domain boundary), or is
                  // around the lane (the flight ends here, sideways).  Heights in float: one LDS read, no double arithmetic.
                  const float2 zr = s_rangeZ[((ex >> 2) - (dx >= 0.0f ? 1 : 0)) + p.flyNbx * (((ey - offY) >> 2) - (dy >= 0.0f ? 1 : 0))];
                  const bool up = dz >= 0.0f;
                  const float pzf = (float)pz;
                  const float tNear = ((up ? zr.x : zr.y) - pzf) * ivz, tFar = ((up ? zr.y : zr.x) - pzf) * ivz;
                  const float tEnd = ((up ? zTopF : zBotF) - pzf) * ivz;
                  float tC = FLT_MAX;  // where the background ends the leg in a collision (tryFly): few flights, the others skip the read
                  if (flyToCollision) tC = s_flyTC[threadIdx.x];
                  const bool ahead = tNear > tcur, sideways = !ahead && tFar > tcur;
                  const float tLim = fminf(ahead ? tNear : tEnd, tC);
                  const int eLim = tLim >= tEnd ? (up ? offZ + p.nz : offZ) : offZ + 1;
                  tnz = isZ ? tnz : tLim;
                  ez = isZ ? ez : (sideways ? -1 : eLim);
                  state = isZ ? (tcur >= tC ? ST_COLLIDE : ST_ENTER) : (sideways ? ST_ENTER : ST_WALK);
                }
              } else if (state == ST_WALK) {
                const int k = ez - offZ - (dz >= 0.0f ? 1 : 0);
                const float lv = s_bgExt[k];
                // leaving / entering the layers of one extinction value (on a z face): the event phase does the rest
                if (LAZY && layerSkipOn && isZ && (lv >= 0.0f) != lazy) state = lazy ? ST_ENTER : ST_JUMP;
                // (the gather goes straight into extCur: its latency overlaps the next iteration's geometry; reading the
                // layer's value ahead, with the edge, cost 6 %)
                extCur = lv;
                if (lv < 0.0f && state == ST_WALK) extCur = extG[cell];
              }
            } else if (state == ST_WALK) {
              // most crossings stay inside a 4x4x4 brick, and most bricks of a cloud scene are clear air whose
              // extinction depends on the layer only: one table gather per brick entered, no gather at all inside
              // background bricks (every scattered gather is one L2 request, and those bound large domains)
              const int bx = ex - (dx >= 0.0f ? 1 : 0), by = ey - offY - (dy >= 0.0f ? 1 : 0), bz = ez - offZ - (dz >= 0.0f ? 1 : 0);
              const int id = (bx >> 2) + p.nbx * ((by >> 2) + p.nby * (bz >> 2));
              if (id != brickId) { brickId = id; brickBase = p.brickTable[id]; }
              extCur = brickBase != 0xffffffffu ? p.ext[brickBase + (uint32_t)((bx & 3) + 4 * ((by & 3) + 4 * (bz & 3)))] : s_bgExt[bz];
            }
            tnz = isZ ? tNew : tnz;
            tny = (!isZ && yLtX) ? tNew : tny;
            tnx = (!isZ && !yLtX) ? tNew : tnx;
          }
        } else {
        const float accNew = acc + (tmin - tcur) * fabsf(extCur);  // :1743
        bool stepNow = state == ST_WALK;
        if (stepNow) {
          if (FLY && flyOn && __float_as_int(extCur) < 0 && !noFly) { state = ST_JUMP; stepNow = false; }
          else if (accNew > tau) { state = ST_COLLIDE; stepNow = false; }
        }
        if (stepNow) {
          {
            if constexpr (ACT) MCBRAT_ACTINIC_DEPOSIT(cell, w, tmin - tcur);  // the piece inside the cell being left (an exit through the top or the surface too)
            acc = accNew;
            tcur = tmin;
            if (DEBUG && stride == 1) cCross++;
            // integer state of the crossed axis ...
            if (isZ) {  // (short predicated blocks per axis)
              ez += dz >= 0.0f ? 1 : -1;
              if (ez > offZ + p.nz) state = ST_TOP;        // :1801-1812; tallied in the event phase
              else if (ez < offZ) state = ST_SURFACE;
              else {
                if constexpr (LVL) {  // the face just crossed: level ez - 1 upward, ez + 1 downward; `cell` is still the cell left
                  const bool up = dz >= 0.0f;
                  const int lev = ez - offZ - (up ? 1 : -1);
                  const long long down = (DIRECT && event == 1u) ? lvlDirect : lvlDown;
                  MCBRAT_LEVEL_DEPOSIT(up ? lvlUp : down, lev, cell - ncol * (lev - (up ? 1 : 0)), weight_to_fixed(w));
                }
                cell += dz >= 0.0f ? ncol : -ncol;
              }
            } else if (yLtX) {  // (stride: 1 cell, or the 4 of a brick column in flight -- `cell` is then unused)
              ey += dy >= 0.0f ? stride : -stride;
              cell += dy >= 0.0f ? p.nx : -p.nx;
              if (ey > offY + p.ny) { ey = offY + stride; cell -= ncol; py -= p.Ly; if (DEBUG && stride != 1) dbgV0 -= p.ny; }          // periodic y :1782-1796:
              else if (ey < offY) { ey = offY + p.ny - stride; cell += ncol; py += p.Ly; if (DEBUG && stride != 1) dbgV0 += p.ny; }     // continue in the next image
              // SIDE: the y face just crossed, after the wrap: the cell on its low side is the one left going forward (a row below
              // the cell entered, the last row of the layer where the step wrapped), the one entered going backward
              if constexpr (SIDE)
                MCBRAT_LEVEL_DEPOSIT(sideBins + sidePart * (dy >= 0.0f ? 2 : 3), 0, dy >= 0.0f ? cell - p.nx + (ey == offY + 1 ? ncol : 0) : cell, weight_to_fixed(w));
            } else {
              ex += dx >= 0.0f ? stride : -stride;
              cell += dx >= 0.0f ? 1 : -1;
              if (ex > p.nx) { ex = stride; cell -= p.nx; px -= p.Lx; if (DEBUG && stride != 1) dbgU0 -= p.nx; }
              else if (ex < 0) { ex = p.nx - stride; cell += p.nx; px += p.Lx; if (DEBUG && stride != 1) dbgU0 += p.nx; }
              if constexpr (SIDE)  // the x face just crossed, likewise
                MCBRAT_LEVEL_DEPOSIT(sideBins + sidePart * (dx >= 0.0f ? 0 : 1), 0, dx >= 0.0f ? cell - 1 + (ex == 1 ? p.nx : 0) : cell, weight_to_fixed(w));
            }
            // ... then ONE extinction read and ONE edge read for whichever axis it was (a lane that just
            // left through the top or the surface reads a valid, unused entry)
            if (gridLds) extCur = s_ext[cell];
            // (the nested form serves the LDS-resident grids only: PRIV == 2)
            const bool spaced = isZ ? zRegularWalk : xyRegularWalk;
            float tNew = tmin + (isZ ? p.dZf * fabsf(ivz) : (float)stride * (yLtX ? p.dYf * fabsf(ivy) : p.dXf * fabsf(ivx)));
            if (!spaced) {
              const int eSel = isZ ? min(max(ez, offZ), offZ + p.nz) : (yLtX ? ey : ex);
              const double edge = s_edge[eSel];
              const double origin = isZ ? pz : (yLtX ? py : px);
              const float iv = isZ ? ivz : (yLtX ? ivy : ivx);
              tNew = (float)(edge - origin) * iv;
            }
            tnz = isZ ? tNew : tnz;
            tny = (!isZ && yLtX) ? tNew : tny;
            tnx = (!isZ && !yLtX) ? tNew : tnx;
          }
        }
        }
        nWalk = __popcll(__ballot(state == ST_WALK));
        // (the tail of a launch: when no lane waits for anything an event phase could give it -- every live lane walks, no
        // photon is left to launch -- the few walkers go on walking instead of visiting an empty event phase after every
        // step; a lone lane on a long flight advanced one step per ~0.8 us that way, most of it the empty phase)
        // (looked at only when the loop would otherwise end: the ballot is not on the path of a full walk loop)
      } while ((nWalk >= p.eventThreshold || (nWalk > 0 && __ballot(state != ST_WALK && (state != ST_DEAD || more)) == 0ull)) && ++walkIt < kWalkCap);
      STAMP(7);
    }

    if (!PRIV) break;
    flush_unit_slab<BLOCK>(s_slab, slabLen, unitSlab, s_cursor);  // PRIV: this unit's private tallies into the batch slab, once
  }

  publish_drops(p.bad, nBadLane);
#ifdef MCBRAT_STAMPS
  if (DEBUG && p.counters && lane == 0) for (int i = 0; i < 9; i++) atomicAdd(p.counters + 16 + i, s_stamp[threadIdx.x >> 6][i]);
#endif
  if (DEBUG && p.counters)
    publish_counters(p.counters, lane == 0, cLegs, cCross, cColl, cAbs, cTop, cSurf, cKill, cSurv, wWalkIters, wWalkLanes, wEventPhases, wEventLanes,
                     wLaunchPhases, wSurfPhases);
}

// the generator itself, for its known-answer test (mcbrat_philox4x32_10): in[6 i ..] = counter[4], key[2]; out[4 i ..] = block
__global__ void philox_kernel(const uint32_t *in, int n, uint32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *a = in + 6 * (size_t)i;
  uint32_t r[4];
  philox4x32_10(a[0], a[1], a[2], a[3], a[4], a[5], r);
  for (int e = 0; e < 4; ++e) out[4 * (size_t)i + e] = r[e];
}

// ---------------------------------------------------------------------------------------
// getFrequencyDistr (src/emissionAndBroadBandWeights.f95:552-572): how many of the run's photons go to each
// wavelength.  The reference draws one uniform per photon from its MT stream on the host and counts the interval
// of the power CDF it falls into (findCDFIndex: smallest i with U <= CDF(i)) -- an O(numPhotons) host loop, 10^9
// draws for a production run.  Same rule here, one Philox uniform per photon on the device: draw d of the run is
// element d % 4 of block (0xFFFFFFFF, 0, d / 4) under the run's key; counts are histogrammed in LDS per workgroup.
// ---------------------------------------------------------------------------------------
__global__ void frequency_distribution_kernel(const double *cdf, int n, unsigned long long total, unsigned long long firstDraw,
                                              uint32_t seedLo, uint32_t seedHi, unsigned long long *counts) {
  extern __shared__ unsigned int s_hist[];
  const bool useLds = n <= 8192;
  if (useLds) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_hist[i] = 0u;
    __syncthreads();
  }
  const unsigned long long nBlocks4 = (firstDraw + total + 3) / 4 - firstDraw / 4;  // Philox blocks that hold the run's draws
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < nBlocks4;
       j += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long blk = firstDraw / 4 + j;
    uint32_t r[4];
    philox4x32_10(0xFFFFFFFFu, 0u, (uint32_t)blk, (uint32_t)(blk >> 32), seedLo, seedHi, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned long long d = blk * 4 + (unsigned)e;
      if (d < firstDraw || d >= firstDraw + total) continue;
      const int i = find_cdf(cdf, n, 1, u01(r[e])) - 1;  // findCDFIndex, 1-based answer
      if (useLds) atomicAdd(&s_hist[min(i, n - 1)], 1u);
      else atomicAdd(&counts[min(i, n - 1)], 1ull);
    }
  }
  if (useLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x)
      if (s_hist[i]) atomicAdd(&counts[i], (unsigned long long)s_hist[i]);
  }
}

// ---------------------------------------------------------------------------------------
// Per-batch epilogue on the device: normalisation (computeRadiativeTransfer :328-364),
// reportResults (:877-884, :966) and the driver's moments (monteCarloDriver.f95:1023-1050).
// Batches are folded in index order by one owner thread per output element, so the
// double sums are reproducible.
//
// Two launches per call (three with limitIntensityContributions): finish_gather does everything that reads the tallies,
// finish_fold the folds over batches that read what finish_gather wrote.  A small domain's epilogue is launch-bound -- five
// back-to-back launches of a few microseconds each were 2 % of a step of the step cloud.  The workgroups of a launch are dealt
// out to its parts by index range: finish_parts() (mcbrat_layout.h) states the parts, their order and their sizes, and
// walk_parts() below finds a workgroup's part from the same arrays.
//
// Every part is one of four shapes -- bin_fold, cell_fold, batch_mean, mean_fold -- and supplies only its offsets and its value
// expression.
// ---------------------------------------------------------------------------------------
struct FinishParams {
  // What every workgroup reads first lies first: a workgroup's first kernel-argument loads then come from the block's first cache
  // lines in one round trip (with the part list behind the layout, finish_fold waited for two: +0.2 us on a 7 us kernel).
  FinishParts parts;      // where the workgroups of every part of finish_gather and of finish_fold end
  int nBatches, xyRegular;
  unsigned long long ppb, total;
  const long long *slabs;
  const float *relArea;   // [ncol] relative column area (irregular xy)
  const double *ze;       // device edges z
  float *colVals;         // [nBatches][3][ncol] scratch: normalised fluxUp/Down/Absorbed per batch
  float *scalVals;        // scratch: [nBatches][3 + nz] means and absorption profile per batch, then the means of every tally
                          // with a tail, [nBatches][its means] at lay.scalX * nBatches
  double *moments;        // header(8) + S1[M] + S2[M]
  float *last;            // normalised results of the last batch, laid out as one sum of the moments
  const unsigned long long *bad;  // photons dropped so far (device counter) ...
  unsigned long long *badHost;    // ... and where the host reads it after the call (pinned host memory)
  // actinic flux: actUnit = 2^e km undoes the kernel's scaling of a deposit (DevParams::actScale = 2^-e)
  double actUnit;
  // side fluxes: the normalisation needs the cell's extent along the crossed axis
  const double *xe, *ye;  // device edges x, y
  TallyShape shape;       // the dimensions and which tallies are on (nOrd = numRecScatOrd + 1, 0 off)
  TallyLayout lay;        // where every part of a slab, of the moments (and of `last`) and of scalVals lies: mcbrat_layout.h
};

__device__ __forceinline__ float photons_per_column(const FinishParams &f, int col, unsigned long long n) {
  const int ncol = f.shape.nx * f.shape.ny;
  return f.xyRegular ? (float)(long long)n / (float)ncol : f.relArea[col] * (float)(long long)n;  // :331, :342
}
__device__ __forceinline__ unsigned long long batch_photons(const FinishParams &f, int b) {
  const unsigned long long start = (unsigned long long)b * f.ppb;
  return (f.total - start) < f.ppb ? (f.total - start) : f.ppb;
}
__device__ __forceinline__ const long long *batch_slab(const FinishParams &f, int b) { return f.slabs + (unsigned long long)b * f.lay.slabStride; }
__device__ __forceinline__ double layer_dz(const FinishParams &f, int k) { return f.ze[k + 1] - f.ze[k]; }

// ---- the value expressions: one raw bin (units of 2^-32 photon weights) of one batch -> its normalised float ----
// the column rule (:348-350, :369-371): over the photons of the bin's column
__device__ __forceinline__ float bin_value(long long raw, float nppc) { return (float)((double)raw * kTallyInv) / nppc; }
// normalised column flux q (0 up, 1 down, 2 absorbed) of one batch
__device__ __forceinline__ float column_value(const FinishParams &f, const long long *slab, int q, int col, float nppc) {
  const int ncol = f.shape.nx * f.shape.ny;
  long long raw;
  if (q < 2) {
    raw = slab[q * ncol + col];  // (part q of the two the slab starts with: lay.slabFluxUp = 0, lay.slabFluxDown = ncol)
  } else {
    raw = 0;
#pragma unroll 8
    for (int k = 0; k < f.shape.nz; k++) raw += slab[f.lay.slabVolume + col + (long long)ncol * k];
  }
  return bin_value(raw, nppc);
}
// volume absorption (:361-364): one written-out double expression, one conversion
__device__ __forceinline__ float volume_value(long long raw, float nppc, double dz) {
  return (float)(((double)raw * kTallyInv) / (((double)nppc * dz) * 1000.0));
}
// one normalised actinic bin: raw 2^-32 2^e / (nppc dz), the shape of the volume absorption without its factor 1000
__device__ __forceinline__ float actinic_value(const FinishParams &f, long long raw, float nppc, double dz) {
  return (float)((((double)raw * kTallyInv) * f.actUnit) / ((double)nppc * dz));
}
// one normalised side bin: raw 2^-32 len / (nppc dz), len the cell's extent along the crossed axis (dx of an x face, dy of a y
// face) and nppc the photons of the cell's column -- the flux density through the vertical face, len dy dz / (dx dy) per photon
// weight of the column's share
__device__ __forceinline__ float side_value(long long raw, float nppc, double len, double dz) {
  return (float)((((double)raw * kTallyInv) * len) / ((double)nppc * dz));
}
// the extent of column `col` along the axis of side part q (0, 1: x; 2, 3: y)
__device__ __forceinline__ double side_extent(const FinishParams &f, int q, int col) {
  const int ix = col % f.shape.nx, iy = col / f.shape.nx;
  return q < 2 ? f.xe[ix + 1] - f.xe[ix] : f.ye[iy + 1] - f.ye[iy];
}
// Where level quantity q (0 up, 1 down, 2 direct, 3 diffuse) lies in a batch's level part, in parts of ncol nLvl bins: its raw bin is
// the bin of part level_part(q), plus that of part 2 where level_adds_direct.  With the direct tally the slab's second part holds the
// diffuse crossings only and the downward total is its sum with the third: integers, so the total keeps its bits.
__device__ __forceinline__ int level_part(const FinishParams &f, int q) { return !f.shape.direct ? q : (q == 0 ? 0 : (q == 2 ? 2 : 1)); }
__device__ __forceinline__ bool level_adds_direct(const FinishParams &f, int q) { return f.shape.direct && q == 1; }

// ---- the two helpers every shape ends in ----
// The ordered f64 fold of one output element over the batches: S1 += x n, S2 += n x^2, and the last batch's x.
struct MomentSum {
  double s1 = 0, s2 = 0;
  float lastv = 0;
  __device__ __forceinline__ void add(float x, unsigned long long photons) {
    const double n = (double)(long long)photons;
    s1 += (double)x * n;
    s2 += n * ((double)x * (double)x);
    lastv = x;
  }
  __device__ __forceinline__ void store(const FinishParams &f, long long off) const {  // off: within one sum of the moments
    f.moments[8 + off] += s1;
    f.moments[8 + f.lay.momentsLen + off] += s2;
    f.last[off] = lastv;
  }
};
// The fixed-shape float tree over the kFinishBlock lanes of a workgroup: the sum, in red[0]
__device__ __forceinline__ float tree_sum(float *red, float s) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kFinishBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ long long finish_element(unsigned blk) { return (long long)blk * kFinishBlock + threadIdx.x; }

// ---- the four shapes ----
// bin fold: one thread per output bin e of nBins, col = e % ncol; the batches folded in order from the column-rule value of
// raw(slab of the batch, e).  off(e): the bin's moment offset.  (Unrolled: the batch values are independent loads, only the f64
// fold is ordered.)
template <int UNROLL, class Raw, class Off>
__device__ __forceinline__ void bin_fold(const FinishParams &f, unsigned blk, long long nBins, Raw raw, Off off) {
  const int ncol = f.shape.nx * f.shape.ny;
  const long long e = finish_element(blk);
  if (e >= nBins) return;
  const int col = (int)(e % ncol);
  MomentSum a;
#pragma unroll UNROLL
  for (int b = 0; b < f.nBatches; b++) {
    const unsigned long long n = batch_photons(f, b);
    const float nppc = photons_per_column(f, col, n);
    a.add(bin_value(raw(batch_slab(f, b), e), nppc), n);
  }
  a.store(f, off(e));
}

// cell fold: P parts of nvox bins, part slowest, then layer.  A workgroup owns kVolVox consecutive bins; its kVolGroups groups of
// lanes share the batches of a pass out between them (the normalisation is a double division per value), then one lane per bin
// folds the pass's values in batch order.  value(part, column, dz of the layer) sets a bin up and returns its
// (raw, photons of the column) -> float.
template <int P, class Value>
__device__ __forceinline__ void cell_fold(const FinishParams &f, unsigned blk, float *sh, long long slabStart, long long momStart, Value value) {
  const int ncol = f.shape.nx * f.shape.ny;
  const long long nvox = (long long)ncol * f.shape.nz;
  const int vi = threadIdx.x % kVolVox, g = threadIdx.x / kVolVox;
  const long long v = (long long)blk * kVolVox + vi;
  const bool live = v < P * nvox;
  const int q = P > 1 && live ? (int)(v / nvox) : 0;
  const long long cellv = live ? (P > 1 ? v % nvox : v) : 0;
  const int col = (int)(cellv % ncol), k = (int)(cellv / ncol);
  const auto of = value(q, col, layer_dz(f, k));
  MomentSum a;
  for (int b0 = 0; b0 < f.nBatches; b0 += kVolChunk) {
    const int nb = min(kVolChunk, f.nBatches - b0);
    if (live)
      for (int j = g; j < nb; j += kVolGroups) {
        const float nppc = photons_per_column(f, col, batch_photons(f, b0 + j));
        sh[j * kVolVox + vi] = of(batch_slab(f, b0 + j)[slabStart + v], nppc);
      }
    __syncthreads();
    if (g == 0 && live)
      for (int j = 0; j < nb; j++) a.add(sh[j * kVolVox + vi], batch_photons(f, b0 + j));
    __syncthreads();
  }
  if (g == 0 && live) a.store(f, momStart + v);
}

// batch mean: one workgroup per (batch, mean m of nMeans); the mean over the columns of that batch's normalised values by the
// fixed float tree, into the scratch [nBatches][nMeans] at scal (a lay.scalX; 0: the flux means and the profile).
// value(m, the batch's slab) sets the mean up and returns its (column, photons of the column) -> float.
template <class Value>
__device__ __forceinline__ void batch_mean(const FinishParams &f, unsigned blk, float *red, unsigned nMeans, long long scal, Value value) {
  const int ncol = f.shape.nx * f.shape.ny;
  const int m = (int)(blk % nMeans), b = (int)(blk / nMeans);
  const unsigned long long n = batch_photons(f, b);
  const auto of = value(m, batch_slab(f, b));
  float s = 0.0f;
  for (int c = threadIdx.x; c < ncol; c += kFinishBlock) s += of(c, photons_per_column(f, c, n));
  const float sum = tree_sum(red, s);
  if (threadIdx.x == 0) f.scalVals[scal * f.nBatches + (long long)b * nMeans + m] = sum / (float)ncol;
}

// mean fold: one thread per mean m of nMeans; the batches folded in order from the scratch vals [nBatches][nMeans].
// off(m): the mean's moment offset.
template <class Off>
__device__ __forceinline__ void mean_fold(const FinishParams &f, unsigned blk, const float *vals, int nMeans, Off off) {
  const int m = (int)finish_element(blk);
  if (m >= nMeans) return;
  MomentSum a;
#pragma unroll 8
  for (int b = 0; b < f.nBatches; b++) a.add(vals[(long long)b * nMeans + m], batch_photons(f, b));
  a.store(f, off(m));
}

// Workgroup blk of a launch whose parts LO .. HI-1 end at end[LO], ... (running sums, in the parts' order): run(part, index within
// the part), the part as a compile-time constant.  Found by halving: every workgroup of a launch pays for the search, and most of a
// launch's workgroups are those of the means, one per batch and mean.  (Workgroup-uniform: a part is entered by whole workgroups.)
template <int LO, int HI, int N, class Run>
__device__ __forceinline__ void walk_parts(const uint32_t (&end)[N], unsigned blk, Run run) {
  if constexpr (HI - LO > 1) {
    constexpr int MID = (LO + HI) / 2;
    if (blk < end[MID - 1])
      walk_parts<LO, MID>(end, blk, run);
    else
      walk_parts<MID, HI>(end, blk, run);
  } else {
    run(std::integral_constant<int, LO>{}, LO > 0 ? blk - end[LO - 1] : blk);
  }
}

// ---- finish_gather: everything that reads the tallies, one specialisation per part of GatherPart ----
template <int PART>
__device__ __forceinline__ void gather_part(const FinishParams &f, unsigned blk, float *sh);

// one thread per (batch, column): normalised column fluxes of every batch
template <>
__device__ __forceinline__ void gather_part<kGatherColumns>(const FinishParams &f, unsigned blk, float *) {
  const int ncol = f.shape.nx * f.shape.ny;
  const long long i = finish_element(blk);
  if (i >= (long long)ncol * f.nBatches) return;
  const int col = (int)(i % ncol), b = (int)(i / ncol);
  const float nppc = photons_per_column(f, col, batch_photons(f, b));
  for (int q = 0; q < 3; q++) f.colVals[((long long)b * 3 + q) * ncol + col] = column_value(f, batch_slab(f, b), q, col, nppc);
}
template <>
__device__ __forceinline__ void gather_part<kGatherVolume>(const FinishParams &f, unsigned blk, float *sh) {
  cell_fold<1>(f, blk, sh, f.lay.slabVolume, f.lay.momVolume,
               [](int, int, double dz) { return [dz](long long raw, float nppc) { return volume_value(raw, nppc, dz); }; });
}
// mean 0..2 = domain-mean fluxes (reportResults :881-884; the column values are formed again here, exactly as the columns part
// forms them), 3.. = absorbedProfile(k) (:966)
template <>
__device__ __forceinline__ void gather_part<kGatherReduce>(const FinishParams &f, unsigned blk, float *sh) {
  const unsigned nMeans = (unsigned)(3 + f.shape.nz);
  if (blk % nMeans < 3)  // (workgroup-uniform)
    batch_mean(f, blk, sh, nMeans, 0, [&f](int q, const long long *slab) {
      return [&f, q, slab](int c, float nppc) { return column_value(f, slab, q, c, nppc); };
    });
  else
    batch_mean(f, blk, sh, nMeans, 0, [&f](int m, const long long *slab) {
      const double dz = layer_dz(f, m - 3);
      const long long *layer = slab + f.lay.slabVolume + (long long)(f.shape.nx * f.shape.ny) * (m - 3);
      return [dz, layer](int c, float nppc) { return volume_value(layer[c], nppc, dz); };
    });
}
// intensity(:, :, d) / numPhotonsPerColumn (:369-371), then the driver's RadianceStats moments
template <>
__device__ __forceinline__ void gather_part<kGatherIntensity>(const FinishParams &f, unsigned blk, float *) {
  const long long ncol = (long long)f.shape.nx * f.shape.ny;
  bin_fold<8>(f, blk, ncol * f.shape.nDir, [&f](const long long *slab, long long e) { return slab[f.lay.slabIntensity + e]; },
              [&f](long long e) { return f.lay.momIntensity + e; });
}
// Scattering orders (computeRadiativeTransfer :352-356, :381-387), order slowest in every part: the slab's order tail is
// [up | down | intensity]; the moment tail puts the domain means in front of each block of column bins
template <>
__device__ __forceinline__ void gather_part<kGatherOrders>(const FinishParams &f, unsigned blk, float *) {
  const long long ncol = (long long)f.shape.nx * f.shape.ny, nOrd = f.shape.nOrd, nDir = f.shape.nDir;
  bin_fold<8>(f, blk, order_means(f.shape) * ncol, [&f](const long long *slab, long long e) { return slab[f.lay.slabOrders + e]; },
              [=, &f](long long e) { return f.lay.momOrders + 2 * nOrd + (e < 2 * ncol * nOrd ? e : e + nDir * nOrd); });
}
template <>
__device__ __forceinline__ void gather_part<kGatherOrderMeans>(const FinishParams &f, unsigned blk, float *sh) {
  batch_mean(f, blk, sh, (unsigned)order_means(f.shape), f.lay.scalOrders, [&f](int m, const long long *slab) {
    const long long *bins = slab + f.lay.slabOrders + (long long)(f.shape.nx * f.shape.ny) * m;
    return [bins](int c, float nppc) { return bin_value(bins[c], nppc); };
  });
}
// Level fluxes, level slowest in every part.  The slab's level part is [up | down], with the direct tally
// [up | diffuse | direct]; the quantities are then 4 (up, down, direct, diffuse) instead of 2, the first two in the level tail and
// the last two in the direct tail, each tail with its domain means in front.
template <>
__device__ __forceinline__ void gather_part<kGatherLevels>(const FinishParams &f, unsigned blk, float *) {
  const long long nLvl = f.shape.nz + 1, nPart = (long long)f.shape.nx * f.shape.ny * nLvl;
  if (!f.shape.direct) {
    bin_fold<8>(f, blk, 2 * nPart, [&f](const long long *slab, long long e) { return slab[f.lay.slabLevels + e]; },
                [=, &f](long long e) { return f.lay.momLevels + 2 * nLvl + e; });
  } else {  // (two loads per batch for the downward total: a shorter unroll keeps the kernel's registers)
    const long long own = finish_element(blk);
    const int q = (int)(own / nPart);
    const long long i = own - q * nPart;
    const long long first = f.lay.slabLevels + level_part(f, q) * nPart + i, second = f.lay.slabLevels + 2 * nPart + i;
    const bool two = level_adds_direct(f, q);
    bin_fold<2>(f, blk, 4 * nPart, [=](const long long *slab, long long) { return two ? slab[first] + slab[second] : slab[first]; },
                [=, &f](long long e) { return q < 2 ? f.lay.momLevels + 2 * nLvl + e : f.lay.momDirect + 2 * nLvl + (e - 2 * nPart); });
  }
}
// (level nz upward and level 0 downward then equal meanFluxUp / meanFluxDown bit for bit)
template <>
__device__ __forceinline__ void gather_part<kGatherLevelMeans>(const FinishParams &f, unsigned blk, float *sh) {
  const int ncol = f.shape.nx * f.shape.ny, nLvl = f.shape.nz + 1;
  const unsigned nMeans = (unsigned)level_means(f.shape);
  const long long nPart = (long long)ncol * nLvl;
  const auto bins = [=, &f](int m, const long long *slab, int part) { return slab + f.lay.slabLevels + part * nPart + (long long)ncol * (m % nLvl); };
  if (!level_adds_direct(f, (int)(blk % nMeans) / nLvl))  // (workgroup-uniform)
    batch_mean(f, blk, sh, nMeans, f.lay.scalLevels, [&](int m, const long long *slab) {
      const long long *own = bins(m, slab, level_part(f, m / nLvl));
      return [own](int c, float nppc) { return bin_value(own[c], nppc); };
    });
  else
    batch_mean(f, blk, sh, nMeans, f.lay.scalLevels, [&](int m, const long long *slab) {
      const long long *diffuse = bins(m, slab, 1), *direct = bins(m, slab, 2);
      return [diffuse, direct](int c, float nppc) { return bin_value(diffuse[c] + direct[c], nppc); };
    });
}
// Actinic flux, layer slowest; the layer means come first in the tail
template <>
__device__ __forceinline__ void gather_part<kGatherActinic>(const FinishParams &f, unsigned blk, float *sh) {
  cell_fold<1>(f, blk, sh, f.lay.slabActinic, f.lay.momActinic + f.shape.nz,
               [&f](int, int, double dz) { return [&f, dz](long long raw, float nppc) { return actinic_value(f, raw, nppc, dz); }; });
}
template <>
__device__ __forceinline__ void gather_part<kGatherActinicMeans>(const FinishParams &f, unsigned blk, float *sh) {
  batch_mean(f, blk, sh, (unsigned)f.shape.nz, f.lay.scalActinic, [&f](int k, const long long *slab) {
    const double dz = layer_dz(f, k);
    const long long *bins = slab + f.lay.slabActinic + (long long)(f.shape.nx * f.shape.ny) * k;
    return [&f, dz, bins](int c, float nppc) { return actinic_value(f, bins[c], nppc, dz); };
  });
}
// Side fluxes: four parts of ncol nz bins, layer slowest -- x plus, x minus, y plus, y minus; the layer
// means of the four parts come first in the tail
template <>
__device__ __forceinline__ void gather_part<kGatherSide>(const FinishParams &f, unsigned blk, float *sh) {
  cell_fold<4>(f, blk, sh, f.lay.slabSide, f.lay.momSide + 4LL * f.shape.nz, [&f](int q, int col, double dz) {
    const double len = side_extent(f, q, col);
    return [len, dz](long long raw, float nppc) { return side_value(raw, nppc, len, dz); };
  });
}
template <>
__device__ __forceinline__ void gather_part<kGatherSideMeans>(const FinishParams &f, unsigned blk, float *sh) {
  batch_mean(f, blk, sh, 4u * (unsigned)f.shape.nz, f.lay.scalSide, [&f](int m, const long long *slab) {
    const int q = m / f.shape.nz;
    const double dz = layer_dz(f, m % f.shape.nz);
    const long long *bins = slab + f.lay.slabSide + (long long)(f.shape.nx * f.shape.ny) * m;
    return [&f, q, dz, bins](int c, float nppc) { return side_value(bins[c], nppc, side_extent(f, q, c), dz); };
  });
}

__global__ void __launch_bounds__(kFinishBlock) finish_gather(const FinishParams f) {
  __shared__ float sh[kVolChunk * kVolVox];  // (the tree uses its first kFinishBlock entries)
  static_assert(kVolChunk * kVolVox >= kFinishBlock, "the tree's scratch");
  walk_parts<0, kGatherParts>(f.parts.gatherEnd, blockIdx.x, [&f](auto part, unsigned blk) { gather_part<decltype(part)::value>(f, blk, sh); });
}

// limitIntensityContributions: redistribute each (component, direction)'s clipped excess over the pixels in
// proportion to that component's own radiance field (computeRadiativeTransfer :294-320).  One block per
// (batch, direction); components in turn, so that no two threads touch one pixel.  Runs before finish_gather.
__global__ void finish_excess(const FinishParams f) {
  __shared__ double red[256];
  const int ncol = f.shape.nx * f.shape.ny;
  const int b = blockIdx.y, d = blockIdx.x;
  long long *slab = const_cast<long long *>(f.slabs) + (unsigned long long)b * f.lay.slabStride;
  long long *inten = slab + f.lay.slabIntensity + (long long)d * ncol;
  for (int j = 0; j <= f.shape.nc; j++) {
    const long long excess = slab[f.lay.slabExcess + (long long)j * f.shape.nDir + d];
    if (excess <= 0) continue;  // block-uniform
    const long long *byc = slab + f.lay.slabByComponent + ((long long)j * f.shape.nDir + d) * ncol;
    double s = 0.0;
    for (int c = threadIdx.x; c < ncol; c += blockDim.x) s += (double)byc[c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    if (total != 0.0)
      for (int c = threadIdx.x; c < ncol; c += blockDim.x) inten[c] += __double2ll_rn(((double)byc[c] / total) * (double)excess);
  }
}

// ---- finish_fold: the folds over batches of what finish_gather wrote, one specialisation per part of FoldPart ----
__device__ __forceinline__ const float *batch_means(const FinishParams &f, long long scal) { return f.scalVals + scal * f.nBatches; }

template <int PART>
__device__ __forceinline__ void fold_part(const FinishParams &f, unsigned blk);

// the column fluxes: colVals [nBatches][3][ncol] is [nBatches][3 ncol] in the moments' order
template <>
__device__ __forceinline__ void fold_part<kFoldColumns>(const FinishParams &f, unsigned blk) {
  mean_fold(f, blk, f.colVals, 3 * f.shape.nx * f.shape.ny, [&f](int i) { return f.lay.momColumns + i; });
}
// domain means and the absorption profile; the header; the dropped-photon count for the host
template <>
__device__ __forceinline__ void fold_part<kFoldScalars>(const FinishParams &f, unsigned blk) {
  if (finish_element(blk) == 0) {  // header: photons and batches done
    f.moments[0] += (double)(long long)f.total;
    f.moments[1] += (double)f.nBatches;
    *f.badHost = *f.bad;  // (the tracing kernel has ended: stream order)
  }
  mean_fold(f, blk, f.scalVals, 3 + f.shape.nz, [&f](int q) { return q < 3 ? f.lay.momMeans + q : f.lay.momProfile + (q - 3); });
}
template <>
__device__ __forceinline__ void fold_part<kFoldOrderMeans>(const FinishParams &f, unsigned blk) {
  const long long ncol = (long long)f.shape.nx * f.shape.ny, nOrd = f.shape.nOrd;
  mean_fold(f, blk, batch_means(f, f.lay.scalOrders), (int)order_means(f.shape),
            [=, &f](int m) { return f.lay.momOrders + (m < 2 * nOrd ? m : 2 * nOrd + 2 * ncol * nOrd + (m - 2 * nOrd)); });
}
template <>
__device__ __forceinline__ void fold_part<kFoldLevelMeans>(const FinishParams &f, unsigned blk) {
  const int nLvl = f.shape.nz + 1;
  mean_fold(f, blk, batch_means(f, f.lay.scalLevels), (int)level_means(f.shape),
            [=, &f](int m) { return m < 2 * nLvl ? f.lay.momLevels + m : f.lay.momDirect + (m - 2 * nLvl); });
}
template <>
__device__ __forceinline__ void fold_part<kFoldActinicMeans>(const FinishParams &f, unsigned blk) {
  mean_fold(f, blk, batch_means(f, f.lay.scalActinic), f.shape.nz, [&f](int k) { return f.lay.momActinic + k; });
}
template <>
__device__ __forceinline__ void fold_part<kFoldSideMeans>(const FinishParams &f, unsigned blk) {
  mean_fold(f, blk, batch_means(f, f.lay.scalSide), 4 * f.shape.nz, [&f](int m) { return f.lay.momSide + m; });
}

__global__ void __launch_bounds__(kFinishBlock) finish_fold(const FinishParams f) {
  walk_parts<0, kFoldParts>(f.parts.foldEnd, blockIdx.x, [&f](auto part, unsigned blk) { fold_part<decltype(part)::value>(f, blk); });
}

}  // namespace mcbrat
