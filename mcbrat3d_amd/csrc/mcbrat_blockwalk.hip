// mcbrat_blockwalk.hip -- the photon loop for domains whose optical grid is resident in LDS, walking from BLOCK
// face to block face.
//
// What is replaced: the same computeRT loop as mcbrat_kernels.hip (Integrators/monteCarloRadiativeTransfer.f95:393-841,
// accumulateExtinctionAlongPath src/opticalProperties.f95:1656-1815).  The reference's walk stops at every cell face
// to add `segment x extinction of the cell` (:1743).  Where neighbouring cells carry the SAME extinction those stops
// add the same product in pieces: the I3RC step cloud is two homogeneous slabs side by side, a plane-parallel
// medium is one, and a leg of either crosses 3-4 cell faces on average before it collides.  Here the host cuts the
// grid into axis-aligned blocks of cells with one extinction value (mcbrat_api.hip: build_blocks) and a leg goes from
// block face to block face; the cell of a collision (tallies, single-scattering albedo, phase function entry) and
// the column of an exit come from the POSITION.  Same physics, the optical depth of a leg summed per block instead
// of per cell (float rounding, as with the layer-skipping walk of the large-domain kernel).
//
// Why it is a kernel of its own and not an option of trace_kernel: with 3-4 cell faces per leg trace_kernel
// alternates between a walk loop and an event phase, each at about half lane occupancy.  With blocks nearly every
// leg of the step cloud ends in the block it starts in, so there is no walk loop left: ONE loop in which every
// lane that has a collision pending is served each iteration (collision -> new direction -> next leg's free path
// -> distance to the block faces -> collide again or not), and the rare kinds of work -- launches, surface
// reflections, block crossings -- wait until enough lanes have queued up, as launches and reflections already did.
//
// Shared with mcbrat_kernels.hip, through mcbrat_photon.h: the generator and its slots (same table: the oracle's Philox mode
// replays these photons), the fixed point conversions, the look-ups, the launch rules, the direction of a surface reflection
// and the flush of a unit's private LDS tally slab, each ONE function that both kernels call.  Written out here AND in
// trace_kernel, bit for bit, each copy naming the other: the cosine of a Lambertian reflection and the HOT ROWS (component
// pick, roulette, scattering angle, new direction, a leg's draws).  This file adds the Philox flavour (p1 per photon, the leg
// block's hoisted half), the accessors to where it keeps the optics, and the walk itself.
#include <float.h>

#include "mcbrat_device.h"
#include "mcbrat_photon.h"

namespace mcbrat {

// lane states of this kernel
enum : int { BW_DEAD = 0, BW_MOVE = 1, BW_COLLIDE = 2, BW_SURFACE = 3, BW_TOP = 4, BW_CROSS = 5 };

// 0-based layer of height z (no periodicity in z): by division where the reference calls z regular, bisection otherwise
__device__ __forceinline__ int locate_z(const double *ze, int nz, bool regular, double z0, double invDz, double z) {
  if (!regular) return find_cell(ze, nz, z);
  return min(max((int)((z - z0) * invDz), 0), nz - 1);  // the reference's own map on a regular axis (findZIndex :1580-1592)
}
// find_cell's answer -- the largest i with e[i] <= v, clamped to [0, n-1] -- on an axis whose edges are equally spaced to 1e-6 of
// a cell: the division is right to within one cell, the edge table decides (no bisection)
__device__ __forceinline__ int locate_near_uniform(const double *e, int n, double x0, double invCell, double v) {
  int i = min(max((int)((v - x0) * invCell), 0), n - 1);
  const double lo = e[i], hi = e[i + 1];
  i += (v >= hi && i < n - 1) ? 1 : 0;
  i -= (v < lo && i > 0) ? 1 : 0;
  return i;
}

// DEBUG: cell index along a periodic axis counted through the periodic images (faces crossed = |difference|)
__device__ __forceinline__ long long unwrapped_index(const double *e, int n, double x0, double L, double invL, double x) {
  const double k = floor((x - x0) * invL);
  return (long long)k * n + find_cell(e, n, x - k * L);
}

// LDS layout of trace_block_kernel (byte offsets), computed the same way by the host (plan_launch) and the kernel
struct BlockLds {
  size_t slab, cursor, rec, invExt, cdf, ext, ssa, cum, pfi, blockOf, tbl, total;
};
// optics: where a collision finds single-scattering albedo, cumulative fractions and phase-function index of its cell (OPT below)
//   0  per cell in LDS, beside the extinction per cell (the small domains: step cloud, plane parallel);
//   1  per cell in global memory (L2: a few tens of KB), LDS holds the extinction per BLOCK -- 2 bytes per cell (its block)
//      instead of 12, for domains whose tally slab takes most of a compute unit's 160 KB (broadband 20 x 20 x 20: 70 KB of
//      tallies + 36 KB of table + 16 KB of block numbers);
//   2  per BLOCK in LDS, where every block is uniform in them too (a homogeneous medium, slabs): no gather at a collision.
// cdfTop: the thermal source's level and row sums of the emission CDF (nz + ny * nz doubles) staged in LDS: ten of the fifteen
// dependent reads of a launch's three bisections stay on chip.
__host__ __device__ inline BlockLds block_lds_layout(int nx, int ny, int nz, int nc, size_t slabLen, int nBlocks, size_t tblFloats,
                                                      int optics = 0, bool cdfTop = false) {
  BlockLds L;
  const size_t nvox = (size_t)nx * ny * nz;
  const size_t nB4 = ((size_t)nBlocks + 3) & ~(size_t)3;
  size_t o = sizeof(double) * (size_t)(nx + ny + nz + 3);
  L.slab = o; o += sizeof(long long) * slabLen;
  L.cursor = o; o += 16;
  o = (o + 15) & ~(size_t)15;
  L.rec = o; o += 16 * (size_t)nBlocks;
  L.invExt = o; o += 4 * nB4;  // 1 / extinction of each block (the collision's step), beside the records: nB4 floats keep the alignment
  L.cdf = o; o += cdfTop ? sizeof(double) * ((size_t)nz + (size_t)ny * nz) : 0;
  L.ext = o; o += optics == 0 ? 4 * nvox : 4 * nB4;
  L.ssa = o; o += optics == 0 ? 4 * nvox * nc : (optics == 2 ? 4 * nB4 * nc : 0);
  L.cum = o; o += nc > 1 ? (optics == 0 ? 4 * nvox * nc : (optics == 2 ? 4 * nB4 * nc : 0)) : 0;  // (read only when there is more than one component)
  L.pfi = o; o += optics == 0 ? 2 * ((nvox * nc + 1) & ~(size_t)1) : (optics == 2 ? 2 * nB4 * nc : 0);
  L.blockOf = o; o += 2 * ((nvox + 1) & ~(size_t)1);
  o = (o + 3) & ~(size_t)3;
  L.tbl = o; o += 4 * tblFloats;
  L.total = o;
  return L;
}

// EMIT: the thermal-emission source (newPhotonStream_BBEmission); its launch code and parameters are compiled out of the
// solar instantiations (registers and instruction cache for the loop that matters).
// SIMPLE: equally spaced axes (as the reference's own test says, new_Integrator :163-181), one component, the domain's
// Lambertian albedo -- the I3RC step cloud, plane-parallel and homogeneous domains.  What the general kernel decides
// at run time from wave-uniform parameters (bisection or division, how many components, surface description or albedo)
// is decided at compile time here: the branches and the scalar registers they keep alive leave the loop.
// SIMPLE = 3 (round 4): one component and the domain's albedo as 1, on axes that the reference's test calls NOT equally spaced but
// that are equally spaced to 1e-6 of a cell -- its test compares with a spacing held in single precision (new_Integrator :140,
// :163-181), so a grid of 0.1 km cells, config 4's, fails it.  Cells are then what the edge table says (find_cell's answer, bit for
// bit the general instantiation's), found by division + table check instead of bisection, with nothing left to decide at run
// time: the general instantiation spills 116 scalar registers into vector lanes on that domain.
// SIMPLE = 2: as 1, and the domain is one cell wide in y (the I3RC step cloud and the plane-parallel cases are x-z
// problems): with a uniform surface nothing depends on the y position, so the y part of the leg origin, of the face
// distances and of the cell look-ups is compiled out (the direction keeps its y component; the instrumented
// instantiation keeps y, it counts the periodic y faces a leg crosses as the reference does).
// OPT: where a collision finds the optics of its cell (0 per cell in LDS, 1 per cell in global memory, 2 per block in LDS), see
// block_lds_layout.  Workgroups of 1024 lanes are ONE per compute unit (they own most of its 160 KB of LDS): 4 waves per SIMD.
// NOSPAN: no block of the medium spans a whole periodic axis that this instantiation looks at (x; y too unless SIMPLE = 2) -- the
// host has seen every record (build_blocks) and picks the instantiation (block_kernel_for).  A lane then never leaves the
// principal image inside a block: the `spans` bits do not exist, the periodic folds that depend on them (collision, block
// crossing) and the tests of rec.w are compiled out.  The forced fold of an exit and the wrap through the domain boundary of a
// crossing stay.  Any medium with horizontal structure is of this kind; plane-parallel and homogeneous media are not.
// RARE: two facts about the run that the host has checked (pick_block, mcbrat_variants.h), compiled into the rare phases, which
// run at 8-12 of 64 lanes.  Bit 0, BLACK: the surface is the domain's albedo and that albedo is 0, and no weight is a NaN --
// every photon that reaches the surface is tallied and dies; nothing of the reflection is compiled, nor the repair of the leg
// origin against the clamped column (an exit of either kind ends its lane).  Bit 1, SUN: the source is the parallel sun
// (solarKind 0); the other solar sources and the reloads of their kind leave the launch.
template <int BLOCK, bool TBL_LDS, bool DEBUG, bool EMIT, int SIMPLE, int OPT = 0, bool NOSPAN = false, int RARE = 0>
__global__ void __launch_bounds__(BLOCK, BLOCK == 1024 ? 4 : (BLOCK > 512 ? BLOCK / 128 : MCBRAT_MIN_WAVES_PER_SIMD))
trace_block_kernel(const DevParams p) {
  constexpr bool NOY = SIMPLE == 2 && !DEBUG;
  constexpr bool BLACK = (RARE & 1) != 0, SUN = (RARE & 2) != 0;
  static_assert(RARE == 0 || (!DEBUG && !EMIT && (SIMPLE == 1 || SIMPLE == 2)), "the instrumented, thermal and general instantiations keep the general rare phases");
  // HOIST: what is constant per photon (Philox) and per block (1 / extinction) is kept in the lane instead of being formed in every
  // leg and collision.  Two lane registers: taken where the budget has them -- the kernels of 128 registers and, of the 768-lane
  // ones (80 registers), the solar x-z instantiation; the others and the instrumented ones would pay with scratch.
  constexpr bool HOIST = !DEBUG && (BLOCK != 768 || (SIMPLE == 2 && !EMIT));
  constexpr bool NEAR = SIMPLE == 3;  // every axis: not regular by the reference's test, equally spaced to 1e-6 of a cell
  const bool xyRegular = NEAR ? false : (SIMPLE != 0 ? true : p.xyRegular != 0);
  const bool zRegular = NEAR ? false : (SIMPLE != 0 ? true : p.zRegular != 0);
  const int nc = SIMPLE != 0 ? 1 : p.nc;
  extern __shared__ __align__(16) unsigned char smem_raw[];
#ifdef MCBRAT_POISON  // audit build: whatever the kernel reads from LDS before it wrote it reads 0xff..
  for (unsigned i = threadIdx.x; i < p.ldsBytes / 4u; i += BLOCK) reinterpret_cast<unsigned *>(smem_raw)[i] = 0xffffffffu;
  __syncthreads();
#endif
  // LDS map: [edges x|y|z (double)] [private tally slab (i64)] [unit cursor] [block records (uint4)] [extinction]
  //          [ssa] [cum] [phase index (u16)] [block of each cell (u16)] [tables (float), TBL_LDS]
  double *s_edge = reinterpret_cast<double *>(smem_raw);
  const int nEdges = p.nx + p.ny + p.nz + 3;
  const int ncol = p.nx * p.ny;
  const int nvox = ncol * p.nz;
  const int slabLen = (int)p.slabStride;
  const int slabsLen = p.unitsWide ? 2 * slabLen : slabLen;  // launch-wide units: the slabs of the two batches a unit may touch, side by side
  const bool cdfTop = EMIT && p.cdfTopLds != 0;  // (wave-uniform)
  const BlockLds lay = block_lds_layout(p.nx, p.ny, p.nz, nc, (size_t)slabsLen, p.nBlocks, TBL_LDS ? (size_t)p.tblTotalFloats : 0, OPT, cdfTop);
  const int nB4 = (p.nBlocks + 3) & ~3;
  long long *s_slab = reinterpret_cast<long long *>(smem_raw + lay.slab);
  unsigned *s_cursor = reinterpret_cast<unsigned *>(smem_raw + lay.cursor);
  uint4 *s_blockRec = reinterpret_cast<uint4 *>(smem_raw + lay.rec);
  float *s_invExt = reinterpret_cast<float *>(smem_raw + lay.invExt);   // [nBlocks] rcp_fast of the blocks' extinction
  float *s_ext = reinterpret_cast<float *>(smem_raw + lay.ext);         // [nvox]; OPT != 0: [nBlocks], the blocks' extinction
  double *s_cdfLevel = reinterpret_cast<double *>(smem_raw + lay.cdf);  // [nz] level sums of the emission CDF, then [nz][ny] row sums (cdfTop)
  double *s_cdfRow = s_cdfLevel + p.nz;
  float *s_ssa = reinterpret_cast<float *>(smem_raw + lay.ssa);         // [nc][nvox]
  float *s_cum = reinterpret_cast<float *>(smem_raw + lay.cum);         // [nc][nvox]
  uint16_t *s_pfi = reinterpret_cast<uint16_t *>(smem_raw + lay.pfi);   // [nc][nvox]
  uint16_t *s_blockOf = reinterpret_cast<uint16_t *>(smem_raw + lay.blockOf);  // [nvox]
  float *s_tbl = reinterpret_cast<float *>(smem_raw + lay.tbl);
  __shared__ int s_tblOffset[MCBRAT_MAX_COMPONENTS], s_tblNSteps[MCBRAT_MAX_COMPONENTS];
  __shared__ float s_tblInvN[MCBRAT_MAX_COMPONENTS];
  if (threadIdx.x < MCBRAT_MAX_COMPONENTS) {
    s_tblOffset[threadIdx.x] = p.tblOffset[threadIdx.x];
    s_tblNSteps[threadIdx.x] = p.tblNSteps[threadIdx.x];
    s_tblInvN[threadIdx.x] = p.tblInvN[threadIdx.x];
  }
  for (int i = threadIdx.x; i < nEdges; i += BLOCK) s_edge[i] = p.edges[i];
  if (TBL_LDS)
    for (int i = threadIdx.x; i < p.tblTotalFloats; i += BLOCK) s_tbl[i] = p.tables[i];
  for (int i = threadIdx.x; i < slabsLen; i += BLOCK) s_slab[i] = 0;
  if (threadIdx.x == 0) s_cursor[0] = 0;
  for (int i = threadIdx.x; i < p.nBlocks; i += BLOCK) { s_blockRec[i] = p.blockRec[i]; s_invExt[i] = rcp_fast(p.blockExt[i]); }
  for (int i = threadIdx.x; i < nvox; i += BLOCK) s_blockOf[i] = p.blockOf[i];
  if (OPT == 0) {
    for (int i = threadIdx.x; i < nvox; i += BLOCK) s_ext[i] = p.ext[i];
    for (int i = threadIdx.x; i < nc * nvox; i += BLOCK) { s_ssa[i] = p.ssa[i]; s_pfi[i] = p.pfi[i]; }
    if (nc > 1)
      for (int i = threadIdx.x; i < nc * nvox; i += BLOCK) s_cum[i] = p.cum[i];
  } else {
    for (int i = threadIdx.x; i < p.nBlocks; i += BLOCK) s_ext[i] = p.blockExt[i];
    if (OPT == 2) {  // per-block optics, [component][nB4]
      for (int i = threadIdx.x; i < nc * nB4; i += BLOCK) {
        const int k = i / nB4, b = i - k * nB4;
        if (b < p.nBlocks) { s_ssa[i] = p.blockSsa[k * p.nBlocks + b]; s_pfi[i] = p.blockPfi[k * p.nBlocks + b]; if (nc > 1) s_cum[i] = p.blockCum[k * p.nBlocks + b]; }
      }
    }
  }
  if (cdfTop) {  // newPhotonStream_BBEmission's levelWeights(k) = voxelWeights(nx, ny, k) and colWeights(j, k) = voxelWeights(nx, j, k) (monteCarloIllumination.f95:56-57)
    const long long nxy = (long long)p.nx * p.ny;
    for (int i = threadIdx.x; i < p.nz; i += BLOCK) s_cdfLevel[i] = p.voxelCDF[((long long)p.nx - 1) + (long long)p.nx * (p.ny - 1) + nxy * i];
    for (int i = threadIdx.x; i < p.ny * p.nz; i += BLOCK) { const int k = i / p.ny, j = i - k * p.ny; s_cdfRow[i] = p.voxelCDF[((long long)p.nx - 1) + (long long)p.nx * j + nxy * k]; }
  }
  __syncthreads();
  // optics of a cell (collisions): component k of cell `cell`
  auto cumAt = [&](int k, int cell) -> float { if constexpr (OPT == 0) return s_cum[k * nvox + cell]; else if constexpr (OPT == 1) return p.cum[k * nvox + cell]; else return s_cum[k * nB4 + s_blockOf[cell]]; };
  auto ssaAt = [&](int k, int cell) -> float { if constexpr (OPT == 0) return s_ssa[k * nvox + cell]; else if constexpr (OPT == 1) return p.ssa[k * nvox + cell]; else return s_ssa[k * nB4 + s_blockOf[cell]]; };
  auto pfiAt = [&](int k, int cell) -> int { if constexpr (OPT == 0) return (int)s_pfi[k * nvox + cell]; else if constexpr (OPT == 1) return (int)p.pfi[k * nvox + cell]; else return (int)s_pfi[k * nB4 + s_blockOf[cell]]; };
  auto extOfCell = [&](int cell) -> float { if constexpr (OPT == 0) return s_ext[cell]; else return s_ext[s_blockOf[cell]]; };
  const float *__restrict__ tbl = TBL_LDS ? s_tbl : p.tables;
  const int offY = p.nx + 1, offZ = p.nx + p.ny + 2;  // edge table offsets
  const double invDz = (double)p.nz / (p.zMax - p.z0);

  const int lane = threadIdx.x & (kWave - 1);

  // this workgroup's unit = photons [unitFirst, unitFirst + unitCount) of the launch; the first unitSplit of them belong to the
  // batch of unitSlab, the others (launch-wide units only) to the next batch, whose tallies go to the second LDS slab
  unsigned long long unitFirst = 0;
  unsigned unitCount = 0, unitSplit = 0;
  long long *unitSlab = nullptr;

  // lane state --------------------------------------------------------------------------
  int state = BW_DEAD;
  // lanes that may still take a photon of this unit: a wave-uniform mask, not a per-lane flag -- ballots and the lane
  // test of the launch then combine it with scalar logic (a per-lane flag turns each ballot of it into a select + compare)
  unsigned long long moreMask = ~0ull;
  int slabOff = 0;                     // the LDS slab of the lane's photon: 0, or slabLen for the second batch of a launch-wide unit
  uint32_t idLo = 0, idHi = 0, event = 0;
  // what every leg block (event, 0, idLo, idHi) of the photon shares: the second round's product q0 and the low word of the
  // first round's p1 (philox4x32_10_leg; the rare blocks with another second counter word recompute philox_p1(idLo))
  unsigned long long legQ0 = 0;
  uint32_t legD1 = 0;
  unsigned long long idP1 = 0;         // !HOIST: philox_p1(idLo), the first round's product shared by every block of the photon's stream
  // block (c0, c1) of the photon's Philox stream, for the rules of mcbrat_photon.h
  auto rng = [&](uint32_t c0, uint32_t c1, uint32_t (&out)[4]) __attribute__((always_inline)) {
    philox4x32_10_p1(c0, c1, HOIST ? philox_p1(idLo) : idP1, idHi, p.seedLo, p.seedHi, out);
  };
  double px = 0, py = 0, pz = 0;      // leg origin (in the periodic image the leg is currently in)
  float dx = 0, dy = 0, dz = 1;       // direction cosines
  float ivx = 0, ivy = 0, ivz = 0;    // 1/direction
  float tnx = 0, tny = 0, tnz = 0, tcur = 0;  // distance along the leg to the x/y/z face of the current BLOCK
  float acc = 0, tau = 0, w = 0, extCur = 0, invExtCur = 0, uX = 0, uY = 0, uZ = 0;
  // cell range of the current block per axis, lo | hi << 16 (the face ahead of the lane is hi or lo by its direction).
  // Kept whole, not just the face ahead: the cell a lane enters on the far side of a face comes from its POSITION on the
  // two other axes, and a position that lies on a second face of the block (a leg through an edge of the block: float
  // ties do occur, equal spacing and a diagonal sun make them common) may round to either side.  Clamped to the range of
  // the block the lane is leaving it cannot fall behind a face the leg has already passed -- unclamped, two position
  // look-ups that both round backwards hand the lane to and fro between two blocks for ever (found by the soak run of
  // test_random_box_media_against_face_by_face_kernel).
  unsigned rx = 0, ry = 0, rz = 0;
  unsigned spans = 0;                  // bit 0 / 1: the current block spans the whole periodic x / y axis (NOSPAN: never set, never read)
  auto spanX = [&]() { return !NOSPAN && (spans & 1u) != 0; };
  auto spanY = [&]() { return !NOSPAN && (spans & 2u) != 0; };
  int nScat = 0, nLegs = 0;
  long long dbgX = 0, dbgY = 0;        // DEBUG: cell of the leg's start counted through the periodic images
  int dbgZ = 0;
  unsigned int cLegs = 0, cCross = 0, cColl = 0, cAbs = 0, cTop = 0, cSurf = 0, cKill = 0, cSurv = 0;
  unsigned long long wIters = 0, wCrossPhases = 0, wCrossLanes = 0, wEventLanes = 0, wLaunchPhases = 0, wSurfPhases = 0;

  // faces crossed by the leg that ends at (x, y) / layer index kz (DEBUG: the reference's crossing count)
  auto countCrossings = [&](double x, double y, int kzEnd) {
    const long long ex = unwrapped_index(s_edge, p.nx, p.x0, p.Lx, p.invLx, x);
    const long long ey = unwrapped_index(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, y);
    cCross += (unsigned)(llabs(ex - dbgX) + llabs(ey - dbgY) + abs(kzEnd - dbgZ));
  };

  // Cell of position xw / yw on a periodic axis; folds the leg origin into the image that position lies in (DEBUG:
  // the leg's start index follows the origin through the images, so that index differences stay face counts).
  // `canLeave`: the position may lie outside the principal image (the lane comes out of a block that spans the whole
  // axis); otherwise it is inside the domain and no fold is needed.  On axes the reference itself calls equally
  // spaced the cell is its own formula, int((x - x0) / delta) (findXYIndicies :1558-1562); else the edge table decides.
  auto locX = [&](double xw, bool canLeave, bool force = false) {
    if (p.nx == 1 && !force) return 0;  // (one column: nothing to find; the origin is folded where the position itself is used)
    if (canLeave) {
      const double shift = floor((xw - p.x0) * p.invLx) * p.Lx;
      px -= shift; xw -= shift;
      if (DEBUG) dbgX -= (long long)rint(shift * p.invLx) * p.nx;
    }
    if (xyRegular) return min(max((int)((xw - p.x0) * p.invDX), 0), p.nx - 1);
    double o = 0.0;
    return locate_periodic(s_edge, p.nx, p.x0, p.Lx, p.invLx, p.invCellX, NEAR || p.xyNearUniform != 0, o, xw);
  };
  auto locY = [&](double yw, bool canLeave, bool force = false) {
    if (NOY) return 0;
    if (p.ny == 1 && !force) return 0;
    if (canLeave) {
      const double shift = floor((yw - p.y0) * p.invLy) * p.Ly;
      py -= shift; yw -= shift;
      if (DEBUG) dbgY -= (long long)rint(shift * p.invLy) * p.ny;
    }
    if (xyRegular) return min(max((int)((yw - p.y0) * p.invDY), 0), p.ny - 1);
    double o = 0.0;
    return locate_periodic(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, p.invCellY, NEAR || p.xyNearUniform != 0, o, yw);
  };
  auto inRange = [](int j, unsigned r) { return min(max(j, (int)(r & 0xffffu)), (int)(r >> 16) - 1); };
  // TEST ONLY (DevParams::legacyTies): the tie handling from before the three fixes the soak runs led to, to show that the
  // bounds below end the kernel without them (tests/test_gpu_edge_cases.py).  Wave-uniform, read in the rare phases only.
  // (compiled into the instrumented instantiation only -- the one mcbrat_trace_fates runs: the production kernels carry none of it)
  const bool legacyNoClamp = (DEBUG || kTestBounds) && (p.legacyTies & 1) != 0, legacyMoveNaN = (DEBUG || kTestBounds) && (p.legacyTies & 2) != 0,
             legacyKeepSpans = (DEBUG || kTestBounds) && (p.legacyTies & 4) != 0;
  auto inRangeX = [&](int j, unsigned r) { return legacyNoClamp ? j : inRange(j, r); };  // clamp of a block crossing
  // cell number of (ix, iy, iz): 24-bit multiplies (full rate; a 32-bit one is a 64-bit multiply-add on this target), exact
  // because the grid is resident in LDS -- every index and product is below 2^17
  const unsigned nx24 = (unsigned)p.nx, ncol24 = (unsigned)ncol;
  auto cellOf = [&](int ix, int iy, int iz) -> int {
    if (NOY) return ix + (int)__umul24(ncol24, (unsigned)iz);
    return ix + (int)__umul24(nx24, (unsigned)(iy + (int)__umul24((unsigned)p.ny, (unsigned)iz)));
  };
  // Distances along the leg to the faces of the block that holds cell (ix, iy, iz); its extinction.
  auto enterBlock = [&](int ix, int iy, int iz) {
    const int cell = cellOf(ix, iy, iz);
    const unsigned blk = s_blockOf[cell];
    const uint4 rec = s_blockRec[blk];
    if constexpr (OPT == 0) extCur = s_ext[cell]; else extCur = s_ext[blk];
    if constexpr (HOIST) invExtCur = s_invExt[blk];
    rx = rec.x; rz = rec.z;
    if (!NOY) ry = rec.y;
    const int fx = dx >= 0.0f ? (int)(rx >> 16) : (int)(rx & 0xffffu);
    const int fy = NOY ? 0 : (dy >= 0.0f ? (int)(ry >> 16) : (int)(ry & 0xffffu));
    const int fz = dz >= 0.0f ? (int)(rz >> 16) : (int)(rz & 0xffffu);
    // a block that spans a whole periodic axis has no face on it (the lane's position runs through the images)
    if constexpr (!NOSPAN) spans |= rec.w;  // (in such a block the lane may leave the principal image: folded when it leaves the block)
    // (the edges are read whether or not the select keeps them -- every face index is in the table: selects, no branches)
    const float ex = (float)(s_edge[fx] - px), ez = (float)(s_edge[offZ + fz] - pz);
    tnx = ((!NOSPAN && (rec.w & 1u)) || ivx == 0.0f) ? FLT_MAX : ex * ivx;
    tny = (NOY || (!NOSPAN && (rec.w & 2u)) || ivy == 0.0f) ? FLT_MAX : (float)(s_edge[offY + fy] - py) * ivy;
    tnz = ivz == 0.0f ? FLT_MAX : ez * ivz;
  };

  // Why the loop ends.  In one iteration a lane in BW_MOVE always leaves that state (collision, block face, exit or
  // drop) and a lane in BW_COLLIDE dies or starts a leg; lanes waiting for a crossing or an exit are served as soon as
  // fewer than eventThreshold lanes collide.  So every iteration starts a leg, serves a crossing or ends a photon, and
  // two counters bound the lot: legs per photon (maxEvents) and block crossings per leg (the `watchdog` figure, here a
  // per-lane count -- the kernel has VGPRs to spare and no SGPR).  Neither costs the iteration anything: the first is
  // one compare where a leg starts, the second lives in the crossing's own branch.
  unsigned nCrossLeg = 0;
  unsigned nBadLane = 0;  // photons this lane dropped at a loop bound; added to *p.bad when the kernel ends
  const unsigned maxEvents = (DEBUG || kTestBounds) ? p.maxEvents : kMaxEvents, maxEventsNaN = (DEBUG || kTestBounds) ? p.maxEventsNaN : kMaxEventsNaN,
                 watchdog = (DEBUG || kTestBounds) ? p.watchdog : kWatchdog;
#define MCBRAT_BW_DROP(kind_) do { \
    if constexpr (DEBUG || kTestBounds) record_first_drop(p.bad, (kind_), 2u, idLo, idHi, state, event);  /* (which bound, which photon) */ \
    if (DEBUG) record_fate(p, idLo, idHi, 3, 0, 0, 0, nScat, nLegs, w); \
    state = BW_DEAD; \
    nBadLane = count_drop(nBadLane, (kind_));  /* (added to *p.bad when the kernel ends: no atomic, no pointer in the loop) */ \
  } while (0)
#ifdef MCBRAT_STAMPS  // development aid (-DMCBRAT_STAMPS): wave cycles per section of the loop, reported with the event counters
  __shared__ unsigned long long s_tprev[BLOCK / 64], s_stamp[BLOCK / 64][9];
  if (lane == 0) { s_tprev[threadIdx.x >> 6] = clock64(); for (int i = 0; i < 9; i++) s_stamp[threadIdx.x >> 6][i] = 0; }
#endif
  for (unsigned long long unit = blockIdx.x;; unit += gridDim.x) {
    if (unit >= p.nUnits) break;  // workgroup-uniform
    if (p.unitsWide) {  // (hi - lo <= ppb, the host's condition: at most one batch boundary inside the unit)
      const unsigned long long lo = p.total * unit / p.nUnits, hi = p.total * (unit + 1) / p.nUnits;
      const unsigned long long b = lo / p.ppb, end = (b + 1) * p.ppb;
      unitFirst = lo;
      unitCount = (unsigned)(hi - lo);
      unitSplit = (unsigned)((hi < end ? hi : end) - lo);
      unitSlab = p.slabs + b * p.slabStride;
    } else {
      const unsigned long long b = unit / p.unitsPerBatch, s = unit % p.unitsPerBatch;
      const unsigned long long bp = (p.total - b * p.ppb) < p.ppb ? (p.total - b * p.ppb) : p.ppb;
      const unsigned long long lo = (bp * s) / p.unitsPerBatch, hi = (bp * (s + 1)) / p.unitsPerBatch;
      unitFirst = b * p.ppb + lo;
      unitCount = (unsigned)(hi - lo);
      unitSplit = unitCount;
      unitSlab = p.slabs + b * p.slabStride;
    }
    moreMask = ~0ull;

    for (;;) {
      bool needLeg = false;
      int ix = 0, iy = 0, iz = 0;  // cell of a lane that starts a leg in this iteration

      // Rare kinds of work -- exits, launches, block crossings -- wait until enough lanes ask for them, or until the
      // wave has little else to do.  Exits come first and launches right after them: under a black surface every exit
      // frees its lane, so the lanes that have just left are refilled in the same iteration instead of queueing again.
      const unsigned long long mSurf = __ballot(state == BW_SURFACE || state == BW_TOP);  // exits, served together
      const unsigned long long mCross = __ballot(state == BW_CROSS);
      const int nBusy = __popcll(__ballot(state == BW_COLLIDE));
      const bool idle = nBusy < p.eventThreshold;
      const bool doSurface = __popcll(mSurf) >= p.surfaceThreshold || idle;
      const bool doCross = __popcll(mCross) >= p.crossThreshold || idle;
      // ---- exits: out the top (computeRT :573-617) or down to the surface (:619-676, Lambertian) ----
      // Both need the column the leg left through, from the position; fluxDown gets the incident weight (:634).
      if ((state == BW_SURFACE || state == BW_TOP) && doSurface) {
        const bool top = state == BW_TOP;
        {
          const double xw = __fma_rn((double)tcur, (double)dx, px), yw = __fma_rn((double)tcur, (double)dy, py);  // where the leg met the face (:1801-1812); exact product, see the collision
          if (DEBUG) countCrossings(xw, yw, top ? p.nz : -1);
          if constexpr (!BLACK) {  // (BLACK: the lane dies below, its origin is never read again)
            px = xw;
            if (!NOY) py = yw;
          }
          // (always folded here: the surface description takes the position itself.  A position on the domain boundary
          // folds to either side of it by rounding: where the clamp then keeps a cell at the other end of the axis, the
          // origin takes the image next to that cell -- cell and position must agree when the reflected leg starts.)
          const int jx = locX(xw, true, true);
          ix = inRange(jx, rx);
          if (!BLACK && ix != jx) {
            const double lo = s_edge[rx & 0xffffu], hi = s_edge[rx >> 16];
            if (px < lo && lo - px > px + p.Lx - hi) px += p.Lx;
            else if (px > hi && px - hi > lo - (px - p.Lx)) px -= p.Lx;
          }
          iy = 0;
          if (!NOY) {
            const int jy = locY(yw, true, true);
            iy = inRange(jy, ry);
            if (!BLACK && iy != jy) {
              const double lo = s_edge[offY + (ry & 0xffffu)], hi = s_edge[offY + (ry >> 16)];
              if (py < lo && lo - py > py + p.Ly - hi) py += p.Ly;
              else if (py > hi && py - hi > lo - (py - p.Ly)) py -= p.Ly;
            }
          }
        }
        atomicAdd(reinterpret_cast<unsigned long long *>(s_slab + slabOff + (top ? 0 : ncol) + (ix + p.nx * iy)), weight_to_fixed(w));
        if (top) {
          if (DEBUG) {
            cTop++;
            record_fate(p, idLo, idHi, 0, ix + 1, iy + 1, p.nz + 1, nScat, nLegs, w);
          }
          state = BW_DEAD;
        } else if constexpr (BLACK) {
          state = BW_DEAD;  // (albedo 0: fluxDown has the incident weight (:634), the product with the albedo is 0 <= FLT_MIN, :673-676)
        } else {
          pz = p.zSurf;
          iz = 0;
          nScat++;
          if (DEBUG) cSurf++;
          // (the cosine of the Lambertian reflection: the same lines stand in trace_kernel, mcbrat_kernels.hip -- see there why)
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
          if (SIMPLE == 0 && p.surfNumX > 0) w = w * surface_reflectance(p, px, py);  // useSurfaceBDRF :667-670
          else w = (float)((double)w * (double)p.albedo);              // :673
          if (w <= FLT_MIN) {
            if (DEBUG) record_fate(p, idLo, idHi, 1, ix + 1, iy + 1, 1, nScat, nLegs, wIn);
            state = BW_DEAD;
          } else {
            lambert_direction(mu, uY, dx, dy, dz);
            needLeg = true;
          }
        }
      }
      STAMP(5);
      const unsigned long long mDead = __ballot(state == BW_DEAD) & moreMask;
      const bool doLaunch = __popcll(mDead) >= p.launchThreshold || idle;
      const unsigned long long want = doLaunch ? mDead : 0ull;
      if (DEBUG) {
        wIters++;
        wEventLanes += nBusy;
        if (want) wLaunchPhases++;
        if (doSurface && mSurf) wSurfPhases++;
        if (doCross && mCross) { wCrossPhases++; wCrossLanes += __popcll(mCross); }
      }
      if (want != 0ull) {  // wave-uniform
        const int nWant = __popcll(want);
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(want >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)want, 0u));  // lanes of `want` below this one
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&s_cursor[0], (unsigned)nWant);
        base = (unsigned)__shfl((int)base, 0);
        const unsigned k = base + rank;
        const bool valid = k < unitCount;
        const unsigned long long myIdx = unitFirst + k;
        const unsigned long long mValid = __ballot(valid);
        if (__builtin_amdgcn_inverse_ballot_w64(want)) {  // (this lane is in `want`: dead, and may take a photon)
          if (valid) {
            // ---- launch: getNextPhoton + computeRT :466-508 (the rules trace_kernel calls, mcbrat_photon.h) ----
            const unsigned long long id = p.firstPhoton + myIdx;
            idLo = (uint32_t)id; idHi = (uint32_t)(id >> 32);
            idP1 = philox_p1(idLo);
            if constexpr (HOIST) { legQ0 = philox_leg_q0(idP1, p.seedLo); legD1 = (uint32_t)idP1; }
            event = 0; nScat = 0; nLegs = 0;
            slabOff = k < unitSplit ? 0 : slabLen;
            double lx, ly, lz;  // fractional launch position in [0,1]
            if (!EMIT) {
              lz = 0.0;
              launch_solar(p, SUN || p.solarKind == 0, rng, lx, ly, dx, dy, dz);
            } else {
              launch_emission(p, rng, [&](float rn, int &ik, int &ij) {
                if (!cdfTop) { emission_level_row(p, rn, ik, ij); return; }
                // (level and row from the sums staged in LDS where they are: the same doubles, the same comparisons)
                ik = find_cdf(s_cdfLevel, p.nz, 1, rn);
                ij = find_cdf(s_cdfRow + p.ny * (ik - 1), p.ny, 1, rn);
              }, lx, ly, lz, dx, dy, dz);
            }
            w = 1.0f;
            px = p.x0 + lx * (p.xMax - p.x0);  // :480-482
            if (!NOY) py = p.y0 + ly * (p.yMax - p.y0);
            if (xyRegular) {  // findXYIndicies :1558-1562
              ix = min((int)((px - p.x0) * p.invDX), p.nx - 1);
              iy = NOY ? 0 : min((int)((py - p.y0) * p.invDY), p.ny - 1);
            } else {
              ix = NEAR ? locate_near_uniform(s_edge, p.nx, p.x0, p.invCellX, px) : find_cell(s_edge, p.nx, px);
              iy = NOY ? 0 : (NEAR ? locate_near_uniform(s_edge + offY, p.ny, p.y0, p.invCellY, py) : find_cell(s_edge + offY, p.ny, py));
            }
            if (!EMIT) {
              pz = p.zLaunch; iz = p.izLaunch;
            } else {
              launch_height(p, zRegular, s_edge + offZ, lz, pz, iz);
            }
            if (EMIT && p.lwFlag && pz > 0.0)  // :504-508 emission counts as negative absorption
              atomicAdd(reinterpret_cast<unsigned long long *>(s_slab + slabOff + 2 * ncol + (ix + p.nx * (iy + p.ny * iz))), to_fixed(-1.0));
            needLeg = true;
          }
        }
        moreMask &= ~want | mValid;  // a lane refused a photon takes none again
      }
      STAMP(0);
      // ---- scattering event, computeRT :703-821 ----
      if (state == BW_COLLIDE) {
        // opticalProperties.f95:1729-1738: the point inside the block where tau is used up.  (Not for a leg whose direction
        // is NaN: the reference's inverse phase-function tables can hold a NaN -- a negative discriminant in the closed-form
        // inversion, inversePhaseFunctions.f95:148-166; one entry in 9001 for a 64-term HG series with g = 0.5 -- and a photon
        // that draws it keeps a NaN direction from then on.  In the reference, the oracle and the face-by-face kernel such a
        // photon goes on colliding in the CELL it is in until its weight is gone; here the cell comes from the position, so
        // the position must stay where it is -- moved along a NaN it would never die: found by the soak run against the oracle.)
        if (dz == dz || legacyMoveNaN) {
#ifdef MCBRAT_PRECISE_MATH
          const double s = (double)(tcur + div_fast(tau - acc, extCur));
#else
          // (HOIST: invExtCur = rcp_fast(extCur), formed once per launch -- div_fast's own instruction on the same input, the same float)
          const double s = (double)(tcur + (HOIST ? (tau - acc) * invExtCur : div_fast(tau - acc, extCur)));
#endif
          // p + s * d as ONE f64 fma.  s and d are floats widened to double: their product has at most 48 significant bits and an
          // exponent far inside double's range, so it is exact -- the multiply of `p + s * d` rounds nothing, and the sum rounds
          // once, as the fma does.  Bit for bit the same (NaN and infinities included); the library is built with
          // -ffp-contract=off, hence the explicit call.
          px = __fma_rn(s, (double)dx, px);
          if (!NOY) py = __fma_rn(s, (double)dy, py);
          pz = __fma_rn(s, (double)dz, pz);
        }
        // its cell, from the position (the periodic fold moves the position into the domain)
        {
          const double xw = px, yw = py;
          iz = NEAR ? locate_near_uniform(s_edge + offZ, p.nz, p.z0, invDz, pz) : locate_z(s_edge + offZ, p.nz, zRegular, p.z0, invDz, pz);
          ix = locX(xw, spanX());
          iy = locY(yw, spanY());
        }
        int cell = cellOf(ix, iy, iz);
        nScat++;
        if (DEBUG) cColl++;
        // HOT ROWS: component pick, roulette, scattering angle, new direction and the leg's draws below stand in trace_kernel too
        // (mcbrat_kernels.hip, HOT ROWS): a change to one of them is made in both.
        int c = 0;  // component pick :759-760 (findIndex over [0, cumExt(:)]), uniform = slot Z of the leg's block
        if (nc > 1) {
          for (int k = 0; k < nc - 1; k++)
            if (uZ >= cumAt(k, cell)) c = k + 1;
        }
        float ssa = ssaAt(c, cell);
        int pfEntry = pfiAt(c, cell);
        // A collision point within an ulp of a face of its block can be located next door -- harmless (the deposit and the
        // phase function of a cell an ulp away) unless next door is vacuum, where nothing collides: booked there the photon
        // would lose its whole weight (the host stores a single-scattering albedo of 0 where there is no extinction; the
        // soak run of the random box media caught one such photon in 8 million).  Then, and only then (clamping every
        // collision cost the step cloud 3 %), the cell is clamped to the block the lane is in.
        if (ssa <= 0.0f && extOfCell(cell) != extCur) {
          ix = inRange(ix, rx); iz = inRange(iz, rz);
          if (!NOY) iy = inRange(iy, ry);
          cell = cellOf(ix, iy, iz);
          c = 0;
          if (nc > 1) {
            for (int k = 0; k < nc - 1; k++)
              if (uZ >= cumAt(k, cell)) c = k + 1;
          }
          ssa = ssaAt(c, cell);
          pfEntry = pfiAt(c, cell);
        }
        if (DEBUG) countCrossings(px, py, iz);  // (after the fold of the look-ups above: px, py are the collision point)
        if (ssa < 1.0f) {  // absorption :765-771
          atomicAdd(reinterpret_cast<unsigned long long *>(s_slab + slabOff + 2 * ncol + cell), weight_to_fixed(w * (1.0f - ssa)));
          w = w * ssa;
          if (DEBUG) cAbs++;
        }
        if (p.useRR && w < 0.5f) {  // Russian roulette :805-811, RussianRouletteW = 1
          float uR = uZ;  // one component: Z decides nothing at the component pick and serves here (no second block)
          if (nc != 1) {  // (wave-uniform; compile time in the SIMPLE instantiations)
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
          state = BW_DEAD;
        } else {
          const int n = s_tblNSteps[c];
          // (in LDS the table is below 2^16 floats: a 24-bit multiply)
          const float *t = tbl + s_tblOffset[c] + (TBL_LDS ? (long long)__umul24((unsigned)pfEntry, (unsigned)n) : (long long)pfEntry * n);
          // computeScatteringAngle :1594-1621 (table point count N, floor-type lookup as written)
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
      // ---- start the next leg: tau, 1/direction, the block the leg starts in ----
      // (a photon is allowed maxEvents legs; one with a NaN direction -- see the collision above -- maxEventsNaN: where
      // omega0 = 1 its weight never falls and neither the reference nor the roulette would ever end it)
      if (needLeg && event >= maxEventsNaN) {  // (one compare on the hot path: maxEventsNaN <= maxEvents; the rule itself in the rare branch)
        if (event >= maxEvents || !(dz == dz || w < 1.0f)) { needLeg = false; MCBRAT_BW_DROP(event >= maxEvents ? DROP_LEGS : DROP_NAN_LEGS); }
      }
      if (needLeg) {
        event++;
        nLegs++;
        if (DEBUG) {
          cLegs++;
          dbgX = unwrapped_index(s_edge, p.nx, p.x0, p.Lx, p.invLx, px);
          dbgY = unwrapped_index(s_edge + offY, p.ny, p.y0, p.Ly, p.invLy, py);
          dbgZ = iz;
        }
        uint32_t r[4];  // (HOIST: the leg's block from what the lane keeps of it -- the same words as rng(event, 0, r))
        if constexpr (HOIST) philox4x32_10_leg(event, legQ0, legD1, idHi, p.seedLo, p.seedHi, r);
        else rng(event, 0u, r);
#ifdef MCBRAT_PRECISE_MATH
        tau = -logf(fmaxf(FLT_MIN, u01(r[0])));
#else
        tau = -0.693147182f * __builtin_amdgcn_logf(fmaxf(FLT_MIN, u01(r[0])));  // :554
#endif
        uX = u01(r[1]); uY = u01(r[2]); uZ = u01(r[3]);
        acc = 0.0f; tcur = 0.0f;
        // opticalProperties.f95:1705-1712: huge step for a zero cosine
        ivx = fabsf(dx) >= 2.0f * FLT_MIN ? rcp_fast(dx) : 0.0f;
        ivy = (!NOY && fabsf(dy) >= 2.0f * FLT_MIN) ? rcp_fast(dy) : 0.0f;
        ivz = fabsf(dz) >= 2.0f * FLT_MIN ? rcp_fast(dz) : 0.0f;
        if constexpr (!NOSPAN) spans = 0;  // (the leg starts inside the domain: its origin was folded where it was located)
        nCrossLeg = 0u;
        enterBlock(ix, iy, iz);
        state = BW_MOVE;
      }
      STAMP(6);
      // ---- block crossings: the cell on the other side of the face, from the position; its block ----
      if (state == BW_CROSS && doCross) {
        const bool yLtX = !NOY && tny < tnx;
        const float m2 = yLtX ? tny : tnx;
        const bool isZ = tnz < m2;  // (the axis whose face was reached: the same comparison the move made)
        const double xw = __fma_rn((double)tcur, (double)dx, px), yw = __fma_rn((double)tcur, (double)dy, py), zw = __fma_rn((double)tcur, (double)dz, pz);  // (exact products: see the collision)
        // (the face crossed gives its axis' index exactly; the two others come from the position, clamped to the
        // range of the block the lane is leaving -- see rx, ry, rz above)
        int jx, jy, jz;
        if (isZ) {
          jz = dz >= 0.0f ? (int)(rz >> 16) : (int)(rz & 0xffffu) - 1;  // (0 <= jz < nz: leaving the domain was decided when the face was reached)
          jx = inRangeX(locX(xw, spanX()), rx);
          jy = NOY ? 0 : inRangeX(locY(yw, spanY()), ry);
        } else if (yLtX) {
          jy = dy >= 0.0f ? (int)(ry >> 16) : (int)(ry & 0xffffu) - 1;
          if (jy >= p.ny) { jy = 0; py -= p.Ly; if (DEBUG) dbgY -= p.ny; }            // periodic y :1790-1796: continue in the next image
          else if (jy < 0) { jy = p.ny - 1; py += p.Ly; if (DEBUG) dbgY += p.ny; }
          jx = inRangeX(locX(xw, spanX()), rx);
          jz = inRangeX(NEAR ? locate_near_uniform(s_edge + offZ, p.nz, p.z0, invDz, zw) : locate_z(s_edge + offZ, p.nz, zRegular, p.z0, invDz, zw), rz);
        } else {
          jx = dx >= 0.0f ? (int)(rx >> 16) : (int)(rx & 0xffffu) - 1;
          if (jx >= p.nx) { jx = 0; px -= p.Lx; if (DEBUG) dbgX -= p.nx; }            // periodic x :1782-1788
          else if (jx < 0) { jx = p.nx - 1; px += p.Lx; if (DEBUG) dbgX += p.nx; }
          jy = NOY ? 0 : inRangeX(locY(yw, spanY()), ry);
          jz = inRangeX(NEAR ? locate_near_uniform(s_edge + offZ, p.nz, p.z0, invDz, zw) : locate_z(s_edge + offZ, p.nz, zRegular, p.z0, invDz, zw), rz);
        }
        // (every axis the block left spans has just been folded -- it cannot be the axis crossed, a spanning block has no
        // face there.  The bits must not outlive the fold: a lane that has just WRAPPED stands on the domain boundary, and
        // a second fold by floor() may take the image on the far side of it while the clamp keeps the cell on this side;
        // the next face then lies behind the lane, tcur steps back, and the lane goes round a corner of four blocks for
        // ever -- the third hang the soak runs found, test_random_domains_against_the_oracle seed 763, a grazing sun.)
        if (!NOSPAN && !legacyKeepSpans) spans = 0;
        enterBlock(jx, jy, jz);
        state = BW_MOVE;
        if (++nCrossLeg > watchdog) MCBRAT_BW_DROP(DROP_CROSSINGS);  // (a leg that has crossed 2^20 blocks is going round in circles)
      }
      STAMP(1);
      // wave-uniform exit: nothing alive and every lane has already been refused a new photon
      if ((__ballot(state != BW_DEAD) | moreMask) == 0ull) break;

#ifdef MCBRAT_STUCK_PROBE  // development aid: a wave still looping after 3e6 iterations records 64 iterations of its first live lane, then drops it
      if (DEBUG && p.traceBuf && wIters > 3000000ull) {
        const unsigned long long live = __ballot(state != BW_DEAD);
        if (live != 0ull && lane == __ffsll((long long)live) - 1) {
          const unsigned long long r = wIters - 3000001ull;
          if (r < 64ull) {
            double *t = p.traceBuf + 20 * r;
            t[0] = 777; t[1] = state; t[2] = tcur; t[3] = tnx; t[4] = tny; t[5] = tnz; t[6] = (double)rx; t[7] = (double)ry; t[8] = (double)rz;
            t[9] = px; t[10] = py; t[11] = pz; t[12] = dx; t[13] = dy; t[14] = dz; t[15] = acc; t[16] = tau; t[17] = extCur; t[18] = spans; t[19] = idLo;
          } else {
            state = BW_DEAD;
          }
        }
      }
#endif
      // ---- move: to the collision point inside this block, or to the block face ahead (:1718-1744) ----
      if (state == BW_MOVE) {
        const bool yLtX = !NOY && tny < tnx;
        const float m2 = yLtX ? tny : tnx;
        const bool isZ = tnz < m2;
        const float tmin = isZ ? tnz : m2;
        const float accNew = acc + (tmin - tcur) * extCur;  // :1743
        const bool coll = accNew > tau;  // :1729-1738: the stop point is resolved at the head of the next iteration
        // (selects, not nested branches: every outcome but the drop is a few moves, and the wave nearly always holds several)
        const bool up = dz >= 0.0f;
        const bool out = isZ && (up ? (int)(rz >> 16) == p.nz : (rz & 0xffffu) == 0u);  // :1801-1812
        const int next = coll ? BW_COLLIDE : (out ? (up ? BW_TOP : BW_SURFACE) : BW_CROSS);
        acc = coll ? acc : accNew;
        tcur = coll ? tcur : tmin;
        if (!coll && !(tmin < FLT_MAX))
          MCBRAT_BW_DROP(DROP_VACUUM);    // no face ahead and nothing to collide with (a horizontal leg through vacuum): the reference walks for ever
        else
          state = next;
      }
      STAMP(7);
    }

    // flush this unit's private tallies into the batch slab, once (launch-wide units: the second LDS slab into the next
    // batch's, which follows in memory; it holds nothing unless the unit reached that batch)
    flush_unit_slab<BLOCK>(s_slab, slabsLen, unitSlab, s_cursor);
  }

  publish_drops(p.bad, nBadLane);
#ifdef MCBRAT_STAMPS
  if (DEBUG && p.counters && lane == 0) for (int i = 0; i < 9; i++) atomicAdd(p.counters + 16 + i, s_stamp[threadIdx.x >> 6][i]);
#endif
  // (slots shared with trace_kernel's report: "walk" = block-crossing phases, "event" = loop iterations)
  if (DEBUG && p.counters)
    publish_counters(p.counters, lane == 0, cLegs, cCross, cColl, cAbs, cTop, cSurf, cKill, cSurv, wCrossPhases, wCrossLanes, wIters, wEventLanes,
                     wLaunchPhases, wSurfPhases);
}

}  // namespace mcbrat
