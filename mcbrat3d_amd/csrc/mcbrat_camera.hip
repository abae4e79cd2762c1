// mcbrat_camera.hip -- the backward Monte Carlo camera (include/mcbrat.h: mcbrat_render_camera,
// mcbrat_camera_ray, mcbrat_sun_transmittance).  A translation unit of its own: camera_kernel and its host code; the tracing
// kernels, their variant table and their parameter block are not touched.
//
// The host half: the seven render entries keep their null checks and go through camera_front() or
// sensor_front() -- the receiver's rules, check_counts(), backward_context(), height or corners, geometry --, backward_render() of
// a Request and reduce_batches(), worded by the entry's Entry; the arithmetic (bounds, scale, capacity, launch shape, the
// reduction of the bins) is mcbrat_backward.h's, plain C++ that runs without a GPU.  launch() is the one LDS-or-global launch,
// mcbrat_sun_transmittance's too.
//
// One lane per path.  A path starts at the sensor (mcbrat_camera_ray.h) and walks BACKWARD.  Leg: tau = -ln u, cell face by cell
// face through the periodic grid until tau is used up, the top (the path ends: nothing diffuse comes in from above) or the
// surface.  Collision: component pick, w *= omega0, local estimate w P(Theta) T_sun(r) / (4 pi mu0) toward the sun, roulette,
// new direction from the inverse table (the phase function is symmetric: the sampler is the forward one).  Surface (Lambertian):
// w *= a(x, y), estimate w T_sun / pi, cosine-weighted upward direction from zSurf.  T_sun walks from the point against the
// sun's direction of travel to the top: deterministic, no roulette.  march() below is both walks: the hot path.
//
// Random numbers: Philox4x32-10, key = seed, counter = (event | block << 24, pixel, sample index lo, hi).
//    event 0          block 0 = [u, v, -, -]            the position in the pixel (jitter)
//    event e >= 1     block 0 = [tau, X, Y, Z]          collision: scattering angle X, azimuth 2 pi Y, component Z
//                                                       surface:   mu = sqrt(X) (X = 0: Z), azimuth 2 pi Y
//                     block 1 = [-, roulette, -, -]
// Tally: a lane sums its path's estimates in a float, converts the sum to i64 fixed point (CamParams::scale) at the path's end
// and adds it to the bin (batch, pixel): integer sums, so an image does not depend on scheduling.
//
// Backward sensors (mcbrat_render_sensors, mcbrat_sensor_ray): camera_kernel<.., SENSOR = true> is the same
// path started on a receiver (mcbrat_sensor_ray.h) -- event 0, block 0 = [u, v, a, c]: the point of the receiver, and a
// cosine-weighted (planar) or uniform (spherical) direction; the sensor's id stands where the pixel stands in the counter --,
// with a second bin array for the direct beam at the path's origin.
//
// Emission renders (mcbrat_render_camera_emission, mcbrat_render_sensors_emission): camera_kernel<.., EMIT =
// true> is the same path with the thermal estimator -- a collision deposits w (1 - omega0) S_cell and the surface w (1 - a) S_sfc
// before the weight is cut, no ray walks toward the sun, a sensor has no direct part.
//
// The radiance by photon path length (mcbrat_render_camera_pathlengths): camera_kernel<.., PATHLEN = true>
// is the solar camera's path with the lane carrying the length of the legs walked -- every estimate goes to fixed point on its
// own and is added to the bin (mcbrat_pathbins.h) of that length plus the sun ray's (zMax - z) / mu0: a histogram per wave in
// LDS, flushed to the strip [batch][pixel][bin] of global memory when the wave moves on to another pixel.
//
// The expected-value estimator of the emission renders (mcbrat_render_camera_emission_expected,
// mcbrat_render_sensors_emission_expected): camera_kernel<.., EMIT = true, .., EXPECT = true> walks the collision estimator's
// paths -- the same counters, legs, collision points, weights -- with march_expected() for march(): every leg deposits the formal
// solution along its whole ray (mcbrat_expected.h), collisions and surface hits deposit nothing.
//
// Component pick, roulette, scattering angle and new direction are written out here as they are in trace_kernel
// (mcbrat_kernels.hip, HOT ROWS) and trace_block_kernel (mcbrat_blockwalk.hip, HOT ROWS): a change to one of those rules is made
// in all three.  What mcbrat_photon.h shares (Philox, u01, lambert_direction, find_cell, surface_reflectance, ...) is called.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "mcbrat_photon.h"
#include "mcbrat_camera_ray.h"
#include "mcbrat_sensor_ray.h"
#include "mcbrat_camera_ctx.h"
#include "mcbrat_backward.h"
#include "mcbrat_pathbins.h"
#include "mcbrat_expected.h"
#include "mcbrat_devmem.h"

namespace mcbrat {

constexpr unsigned kCameraMaxEvents = 1u << 20;  // legs per path (the event has 24 bits of the counter)
// The sensor instantiations carry a second pending sum and the direct estimate through the path: the register budget of six
// waves per SIMD (80 VGPRs), the occupancy the camera instantiations have by their 79 registers, is asked for by name
constexpr int kSensorWavesPerSimd = 6;

struct CamParams {
  CameraGeometry g;
  int jitter;
  unsigned long long spp;          // samples per pixel and batch
  unsigned long long npix;
  unsigned long long firstSample;
  unsigned long long total;        // paths of the launch: bins * spp, index = (batch * npix + pixel) * spp + k
  unsigned long long pathsPerLane; // a wave takes 64 * pathsPerLane consecutive indices, lane l the indices l, l + 64, ...
  long long *bins;                 // [nBatches][npix] fixed point
  unsigned long long *dropped;
  double scale;                    // fixed-point units per unit radiance (a power of two)
  double pathMax;                  // a path's sum saturates here, in units: spp * pathMax < 2^62
  unsigned maxSunCross, maxLegCross, maxEvents;  // loop bounds (host, from the geometry)
  float sun[3];                    // unit vector TOWARD the sun: minus the direction of travel
  float invFourPiMu0;
  const float *fwd;                // forward tables, components concatenated, [entry][angle]
  int fwdOffset[MCBRAT_MAX_COMPONENTS], fwdNAngles[MCBRAT_MAX_COMPONENTS];
  // mcbrat_sun_transmittance
  const double *points;
  float *transmittance;
  long long nPoints;
  // mcbrat_render_sensors (SENSOR instantiations; npix = the number of sensors, spp = samples per sensor and batch)
  const SensorGeometry *sensors;   // [npix]
  long long *binsDirect;           // [nBatches][npix] fixed point, in units of w0 like bins
  // the emission renders (EMIT instantiations): the caller's Planck radiances, left in global memory
  const float *srcCell;            // [nz][ny][nx], x fastest
  const float *srcSurface;         // [ny][nx]
  double invSrcMax;                // 1 / the largest source value: a path's sum is tallied in units of it
  // mcbrat_render_camera_pathlengths (PATHLEN instantiations): bins is [nBatches][npix][numBins]
  const float *pathEdges;          // [numBins] lower edges of the path-length bins
  int numBins;
  int pathDirect;                  // every deposit straight to global memory (option cameraPathBinsInLds = 0: a measurement)
  float invMu0;                    // 1 / mu0: the sun ray's geometric length is (zMax - z) / mu0
  // the expected-value estimator (EXPECT instantiations)
  const float *emisCell;           // [nz][ny][nx] E[v], the cell's emission per unit extinction: emission_grid_kernel's, per render
};

struct GridView { const double *xe, *ye, *ze; const float *ext; };

// The extinction grid and the edges: staged in LDS (every lane of the workgroup calls this), or where they lie in global memory
template <int BLOCK, bool GRID_LDS>
__device__ __forceinline__ GridView grid_view(const DevParams &p, unsigned char *smem) {
  GridView g;
  if (GRID_LDS) {
    double *s_edge = reinterpret_cast<double *>(smem);
    const int nEdge = p.nx + p.ny + p.nz + 3, nvox = p.nx * p.ny * p.nz;
    float *s_ext = reinterpret_cast<float *>(s_edge + nEdge);
    for (int i = threadIdx.x; i < nEdge; i += BLOCK) s_edge[i] = p.edges[i];
    for (int i = threadIdx.x; i < nvox; i += BLOCK) s_ext[i] = p.ext[i];
    __syncthreads();
    g.xe = s_edge; g.ext = s_ext;
  } else {
    g.xe = p.edges; g.ext = p.ext;
  }
  g.ye = g.xe + p.nx + 1;
  g.ze = g.ye + p.ny + 1;
  return g;
}

struct Ray {
  double ox, oy, oz;   // origin, in the periodic image the walk stands in
  float dx, dy, dz;
  int ix, iy, iz;      // cell, 0-based
};
enum : int { END_COLLISION = 0, END_TOP = 1, END_SURFACE = 2, END_BOUND = 3 };

// Folds (x, y) into the domain and finds the cell of the point (z clamped to the layers: zMax belongs to the top one)
__device__ __forceinline__ void locate(const DevParams &p, const GridView &g, Ray &r) {
  r.ox -= floor((r.ox - p.x0) * p.invLx) * p.Lx;
  if (r.ox < p.x0) r.ox += p.Lx;
  if (r.ox >= p.xMax) r.ox -= p.Lx;
  r.oy -= floor((r.oy - p.y0) * p.invLy) * p.Ly;
  if (r.oy < p.y0) r.oy += p.Ly;
  if (r.oy >= p.yMax) r.oy -= p.Ly;
  r.ix = find_cell(g.xe, p.nx, r.ox);
  r.iy = find_cell(g.ye, p.ny, r.oy);
  r.iz = find_cell(g.ze, p.nz, r.oz);
}

// Walks from the ray's origin along its direction, cell face by cell face, periodic in x and y, marching by cell INDEX (a face
// is crossed exactly once, whatever the rounding of its distance), until `target` optical depth is used up (END_COLLISION), the
// top, the surface, or maxCross crossings.  tEnd: the distance walked; acc: the optical depth walked through.  Distances to
// faces are differences in double against the origin, times 1 / direction in float; a tie crosses its faces one after the other
// over a segment of length 0.  r.ix, iy, iz, ox, oy end as the cell and the periodic image of the end point.
__device__ __forceinline__ int march(const DevParams &p, const GridView &g, Ray &r, float target, unsigned maxCross, float &tEnd, float &acc) {
  const float jx = fabsf(r.dx) >= 2.0f * FLT_MIN ? 1.0f / r.dx : 0.0f;
  const float jy = fabsf(r.dy) >= 2.0f * FLT_MIN ? 1.0f / r.dy : 0.0f;
  const float jz = fabsf(r.dz) >= 2.0f * FLT_MIN ? 1.0f / r.dz : 0.0f;
  const int hx = r.dx >= 0.0f ? 1 : 0, hy = r.dy >= 0.0f ? 1 : 0, hz = r.dz >= 0.0f ? 1 : 0;
  int ix = r.ix, iy = r.iy, iz = r.iz;
  double ox = r.ox, oy = r.oy;
  float tx = jx != 0.0f ? (float)(g.xe[ix + hx] - ox) * jx : FLT_MAX;
  float ty = jy != 0.0f ? (float)(g.ye[iy + hy] - oy) * jy : FLT_MAX;
  float tz = jz != 0.0f ? (float)(g.ze[iz + hz] - r.oz) * jz : FLT_MAX;
  float tcur = 0.0f;
  int end = END_BOUND;
  acc = 0.0f;
  for (unsigned n = 0; n < maxCross; ++n) {
    const float e = g.ext[(iz * p.ny + iy) * p.nx + ix];
    const float tmin = fminf(tx, fminf(ty, tz));
    const float seg = fmaxf(tmin - tcur, 0.0f);
    const float tauSeg = seg * e;
    if (e > 0.0f && acc + tauSeg >= target) {
      tcur = fminf(tcur + (target - acc) / e, fmaxf(tmin, tcur));
      acc = target;
      end = END_COLLISION;
      break;
    }
    acc += tauSeg;
    tcur = fmaxf(tmin, tcur);
    if (tz <= tx && tz <= ty) {
      iz += hz ? 1 : -1;
      if (iz < 0) { iz = 0; end = END_SURFACE; break; }
      if (iz >= p.nz) { iz = p.nz - 1; end = END_TOP; break; }
      tz = (float)(g.ze[iz + hz] - r.oz) * jz;
    } else if (tx <= ty) {
      ix += hx ? 1 : -1;
      if (ix < 0) { ix = p.nx - 1; ox += p.Lx; }
      if (ix >= p.nx) { ix = 0; ox -= p.Lx; }
      tx = (float)(g.xe[ix + hx] - ox) * jx;
    } else {
      iy += hy ? 1 : -1;
      if (iy < 0) { iy = p.ny - 1; oy += p.Ly; }
      if (iy >= p.ny) { iy = 0; oy -= p.Ly; }
      ty = (float)(g.ye[iy + hy] - oy) * jy;
    }
  }
  r.ix = ix; r.iy = iy; r.iz = iz; r.ox = ox; r.oy = oy;
  tEnd = tcur;
  return end;
}

__device__ __forceinline__ float camera_albedo(const DevParams &p, double x, double y) {
  return p.surfNumX > 0 ? surface_reflectance(p, x, y) : p.albedo;
}

// How the RAY of a leg ended (march_expected): at the top, on the surface (in `column`, behind optical depth tauSfc), at
// maxCross crossings, or behind kExpectedTauCut
enum : int { RAY_TOP = END_TOP, RAY_SURFACE = END_SURFACE, RAY_BOUND = END_BOUND, RAY_CUT = 4 };
struct RayEnd { int how, column; float tauSfc; };

// The walk of an EXPECT instantiation: march() for the leg -- the same cells in the same order, the
// same sums in the same order, so the value returned, tEnd, acc and r's cell and periodic image are march()'s bit for bit -- and
// in the same pass the emission of the whole ray, on past the collision point to the boundary or to the cut:
//     emitted = sum over the segments  E[v] e^(-tau_in) (1 - e^(-dtau))  +  e^(-tau_sfc) (1 - a) S_sfc where it meets the surface
// with tau from the leg's origin (mcbrat_expected.h: expected_segment).  `emis`: E[v], in LDS or in global memory.
__device__ __forceinline__ int march_expected(const DevParams &p, const CamParams &cp, const GridView &g, const float *emis, Ray &r, float target,
                                              unsigned maxCross, float &tEnd, float &acc, float &emitted, RayEnd &ray) {
  const float jx = fabsf(r.dx) >= 2.0f * FLT_MIN ? 1.0f / r.dx : 0.0f;
  const float jy = fabsf(r.dy) >= 2.0f * FLT_MIN ? 1.0f / r.dy : 0.0f;
  const float jz = fabsf(r.dz) >= 2.0f * FLT_MIN ? 1.0f / r.dz : 0.0f;
  const int hx = r.dx >= 0.0f ? 1 : 0, hy = r.dy >= 0.0f ? 1 : 0, hz = r.dz >= 0.0f ? 1 : 0;
  int ix = r.ix, iy = r.iy, iz = r.iz;
  double ox = r.ox, oy = r.oy;
  float tx = jx != 0.0f ? (float)(g.xe[ix + hx] - ox) * jx : FLT_MAX;
  float ty = jy != 0.0f ? (float)(g.ye[iy + hy] - oy) * jy : FLT_MAX;
  float tz = jz != 0.0f ? (float)(g.ze[iz + hz] - r.oz) * jz : FLT_MAX;
  float tcur = 0.0f;
  float tau = 0.0f;   // the ray's optical depth: the leg's while the leg is open
  bool open = true;   // the leg has not ended
  int end = END_BOUND;
  emitted = 0.0f;
  ray.how = RAY_BOUND;
  for (unsigned n = 0; n < maxCross; ++n) {
    const int cell = (iz * p.ny + iy) * p.nx + ix;
    const float e = g.ext[cell];
    const float tmin = fminf(tx, fminf(ty, tz));
    const float seg = fmaxf(tmin - tcur, 0.0f);
    const float tauSeg = seg * e;
    if (open && e > 0.0f && tau + tauSeg >= target) {
      // the collision point, as march() finds it; the ray goes on, and the cell's segment is deposited whole below
      tEnd = fminf(tcur + (target - tau) / e, fmaxf(tmin, tcur));
      acc = target;
      end = END_COLLISION;
      open = false;
      r.ix = ix; r.iy = iy; r.iz = iz; r.ox = ox; r.oy = oy;
    }
    if (tauSeg > 0.0f) {
      const float E = emis[cell];
      if (E > 0.0f) emitted += E * expected_segment(tau, tauSeg);
    }
    tau += tauSeg;
    if (!open && tau >= kExpectedTauCut) { ray.how = RAY_CUT; break; }
    tcur = fmaxf(tmin, tcur);
    if (tz <= tx && tz <= ty) {
      iz += hz ? 1 : -1;
      if (iz < 0) { iz = 0; ray.how = RAY_SURFACE; break; }
      if (iz >= p.nz) { iz = p.nz - 1; ray.how = RAY_TOP; break; }
      tz = (float)(g.ze[iz + hz] - r.oz) * jz;
    } else if (tx <= ty) {
      ix += hx ? 1 : -1;
      if (ix < 0) { ix = p.nx - 1; ox += p.Lx; }
      if (ix >= p.nx) { ix = 0; ox -= p.Lx; }
      tx = (float)(g.xe[ix + hx] - ox) * jx;
    } else {
      iy += hy ? 1 : -1;
      if (iy < 0) { iy = p.ny - 1; oy += p.Ly; }
      if (iy >= p.ny) { iy = 0; oy -= p.Ly; }
      ty = (float)(g.ye[iy + hy] - oy) * jy;
    }
  }
  ray.column = iy * p.nx + ix;
  ray.tauSfc = tau;
  if (ray.how == RAY_SURFACE) {
    // (the point as the caller forms it where the leg itself ends here: the same albedo to the bit)
    const float a = camera_albedo(p, ox + (double)r.dx * (double)tcur, oy + (double)r.dy * (double)tcur);
    emitted += expf(-tau) * ((1.0f - a) * cp.srcSurface[ray.column]);
  }
  if (open) {  // the leg is the ray: it ends where march() ends it
    end = ray.how;
    r.ix = ix; r.iy = iy; r.iz = iz; r.ox = ox; r.oy = oy;
    tEnd = tcur;
    acc = tau;
  }
  return end;
}

// exp(-optical depth) from (x, y, z) in cell (ix, iy, iz) toward the sun up to the top; `bound`: the walk did not get there
__device__ __forceinline__ float sun_transmittance(const DevParams &p, const CamParams &cp, const GridView &g, double x, double y, double z,
                                                   int ix, int iy, int iz, bool &bound) {
  Ray s{x, y, z, cp.sun[0], cp.sun[1], cp.sun[2], ix, iy, iz};
  float t, tau;
  const int end = march(p, g, s, FLT_MAX, cp.maxSunCross, t, tau);
  bound = end != END_TOP;
  return expf(-tau);
}

// Every lane of a wave calls this in step: adds the lanes' values to their bins -- one atomic for the wave where the lanes that
// have something share a bin (sensor-major indices, samplesPerSensor >= 64), one per lane otherwise
__device__ __forceinline__ void wave_add(long long *bins, uint32_t bin, long long value, int lane) {
  const bool have = value != 0;
  const unsigned long long haveMask = __ballot(have);
  if (haveMask == 0ull) return;
  const int first = __ffsll((long long)haveMask) - 1;
  const uint32_t firstBin = __shfl(bin, first);
  if (__ballot(have && bin != firstBin) == 0ull) {
    long long v = value;
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(bins + firstBin), (unsigned long long)v);
  } else if (have) {
    atomicAdd(reinterpret_cast<unsigned long long *>(bins + bin), (unsigned long long)value);
  }
}

// One estimate of a path of a PATHLEN instantiation: to fixed point on its own, capped by what the path
// has left of its budget, and added to bin path_bin(L) of the path's pixel -- in the wave's histogram in LDS (`hist`, where the
// wave's 64 indices share a pixel: `toLds`) or straight in global memory (`strip`: the pixel's numBins sums).  false: the
// estimate is a NaN, nothing is deposited
using LdsSum = __attribute__((address_space(3))) unsigned long long;  // a sum of a wave's histogram: in LDS by its type
__device__ __forceinline__ bool path_deposit(const CamParams &cp, const float *edges, LdsSum *hist, bool toLds, long long *strip, float est,
                                             float L, long long &left) {
  if (!(est == est)) return false;
  long long v = __double2ll_rn(fmin((double)est * cp.scale, cp.pathMax));
  v = v < left ? v : left;
  left -= v;
  if (v != 0) {
    const int b = path_bin(edges, cp.numBins, L);
    if (toLds) __hip_atomic_fetch_add(hist + b, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    else atomicAdd(reinterpret_cast<unsigned long long *>(strip + b), (unsigned long long)v);
  }
  return true;
}

// Every lane of a wave calls this in step: the wave's non-empty sums go to the strip of its pixel in global memory, one atomic
// each, and the histogram is empty again
__device__ __forceinline__ void path_flush(LdsSum *hist, long long *strip, int numBins, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int b = lane; b < numBins; b += kWave) {
    const unsigned long long v = hist[b];
    if (v != 0ull) {
      atomicAdd(reinterpret_cast<unsigned long long *>(strip + b), v);
      hist[b] = 0ull;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// SENSOR: the path starts on a receiver (mcbrat_sensor_ray.h) instead of in a pixel, the sensor's id
// stands where the pixel stands in the counter, and a second sum takes the direct beam at the origin; from there on the path is
// the camera's.
// EMIT: the thermal estimator on the same path.  No ray toward the sun and no forward table: a collision
// deposits w (1 - omega0) S_cell BEFORE w *= omega0, the surface w (1 - a) S_sfc before w *= a, and a sensor has no direct part.
// PATHLEN (the solar camera only): the radiance by photon path length.  The lane carries the length L of
// the legs walked; every estimate is tallied on its own, at L plus the sun ray's (zMax - z) / mu0, in a histogram per wave.
// EXPECT (the emission renders only): the expected-value estimator on EMIT's path.  march_expected() is
// the walk; the leg deposits w times its ray's emission, whatever ends it; EMIT's two deposits are not compiled.  A path whose
// sum reaches pathMax is dropped and counted: a leg's deposit is not tied to the weight lost on it, so srcMax does not bound it.
template <int BLOCK, bool GRID_LDS, bool SENSOR, bool EMIT, bool PATHLEN = false, bool EXPECT = false>
__global__ void __launch_bounds__(BLOCK, SENSOR ? kSensorWavesPerSimd : MCBRAT_MIN_WAVES_PER_SIMD) camera_kernel(const DevParams p, const CamParams cp) {
  static_assert(!PATHLEN || (!SENSOR && !EMIT), "path lengths: the solar camera only");
  static_assert(!EXPECT || (EMIT && !PATHLEN), "the expected-value estimator: the emission renders only");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  // EXPECT: E[v], staged behind the grid where the grid is staged (expected_lds_offset: the one statement of where, the host's
  // too), before grid_view() and under its barrier
  const float *emis = nullptr;
  if constexpr (EXPECT) {
    emis = cp.emisCell;
    if constexpr (GRID_LDS) {
      float *s_emis = reinterpret_cast<float *>(smem_raw + expected_lds_offset(p.nx, p.ny, p.nz));
      for (int i = threadIdx.x; i < p.nx * p.ny * p.nz; i += BLOCK) s_emis[i] = cp.emisCell[i];
      emis = s_emis;
    }
  }
  const GridView g = grid_view<BLOCK, GRID_LDS>(p, smem_raw);
  // PATHLEN: behind the grid, a histogram per wave and the edges (mcbrat_backward.h: path_lds_offset, path_lds_bytes)
  LdsSum *hist = nullptr;
  const float *edges = nullptr;
  if constexpr (PATHLEN) {
    const size_t gridBytes = GRID_LDS ? sizeof(double) * (size_t)(p.nx + p.ny + p.nz + 3) + sizeof(float) * (size_t)p.nx * p.ny * p.nz : 0;
    unsigned long long *s_hist = reinterpret_cast<unsigned long long *>(smem_raw + path_lds_offset(gridBytes));
    float *s_edges = reinterpret_cast<float *>(s_hist + (size_t)(BLOCK / kWave) * cp.numBins);
    for (int i = threadIdx.x; i < (BLOCK / kWave) * cp.numBins; i += BLOCK) s_hist[i] = 0ull;
    for (int i = threadIdx.x; i < cp.numBins; i += BLOCK) s_edges[i] = cp.pathEdges[i];
    __syncthreads();
    hist = (LdsSum *)(s_hist + (size_t)(threadIdx.x >> 6) * cp.numBins);
    edges = s_edges;
  }
  constexpr float kPi = 3.14159265358979312f;
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long wave = ((unsigned long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const unsigned long long chunk = wave * (unsigned long long)kWave * cp.pathsPerLane;
  const int nvox = p.nx * p.ny * p.nz;

  unsigned long long pendBin = ~0ull;  // the bin the lane is summing for, and its sum (the camera; a sensor's wave adds after every path)
  long long pend = 0;
  unsigned nDropped = 0;
  unsigned long long tag = ~0ull;      // PATHLEN: the (batch, pixel) the wave's histogram holds sums of; ~0: none
  bool shared = false;                 // PATHLEN: the round's 64 indices share a (batch, pixel): its deposits go to the histogram

  for (unsigned long long j = 0; j < cp.pathsPerLane; ++j) {
    const unsigned long long index = chunk + j * kWave + (unsigned long long)lane;
    if constexpr (PATHLEN) {
      // the same for every lane of the wave, and before any lane leaves the loop: all 64 take part in a flush
      const unsigned long long base = chunk + j * kWave;
      if (base >= cp.total) break;
      const unsigned long long last = base + (kWave - 1) < cp.total ? base + (kWave - 1) : cp.total - 1;
      const unsigned long long binFirst = base / cp.spp;
      shared = !cp.pathDirect && last / cp.spp == binFirst;
      if (tag != ~0ull && !(shared && tag == binFirst)) {
        path_flush(hist, cp.bins + tag * (unsigned long long)cp.numBins, cp.numBins, lane);
        tag = ~0ull;
      }
      if (shared) tag = binFirst;
    }
    if constexpr (!SENSOR) {
      if (index >= cp.total) break;
    }
    // SENSOR: every lane of the wave goes through every round, so that the wave can add its two sums together after each path;
    // a lane past the last index walks nothing (its sensor, read below, is one of the call's: pixel < npix whatever the index)
    const bool valid = SENSOR ? index < cp.total : true;
    const unsigned long long bin = index / cp.spp, k = index - bin * cp.spp;
    const unsigned long long batch = bin / cp.npix, pixel = bin - batch * cp.npix;
    const unsigned long long sample = cp.firstSample + batch * cp.spp + k;
    const uint32_t sLo = (uint32_t)sample, sHi = (uint32_t)(sample >> 32);
    uint32_t pix = (uint32_t)pixel;
    if constexpr (!SENSOR && !PATHLEN) {
      if (bin != pendBin) {
        if (pend != 0) atomicAdd(reinterpret_cast<unsigned long long *>(cp.bins + pendBin), (unsigned long long)pend);
        pendBin = bin; pend = 0;
      }
    }
    Ray r;
    bool dropped = !valid;
    const uint32_t bin32 = (uint32_t)bin;  // (SENSOR: 2 * bins fit the 4 GiB budget, so 32 bits hold a bin's index through the path)
    if constexpr (SENSOR) {
      const SensorGeometry &sg = cp.sensors[pixel];
      pix = sg.id;
      uint32_t q[4];
      philox4x32_10(0u, pix, sLo, sHi, p.seedLo, p.seedHi, q);
      double o[3], d[3];
      // sensor_ray() in its two halves, one after the other: taken together their eighteen doubles of geometry are the
      // kernel's widest point by registers
      sensor_direction(sg, (double)u01(q[2]), (double)u01(q[3]), d);
      r.dx = (float)d[0]; r.dy = (float)d[1]; r.dz = (float)d[2];
      __builtin_amdgcn_sched_barrier(0);
      sensor_origin(sg, (double)u01(q[0]), (double)u01(q[1]), o);
      r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
      locate(p, g, r);
    } else {
      double u = 0.5, v = 0.5, o[3], d[3];
      if (cp.jitter) {
        uint32_t q[4];
        philox4x32_10(0u, pix, sLo, sHi, p.seedLo, p.seedHi, q);
        u = (double)u01(q[0]); v = (double)u01(q[1]);
      }
      camera_ray(cp.g, (int)(pixel % (unsigned long long)cp.g.npx), (int)(pixel / (unsigned long long)cp.g.npx), u, v, o, d);
      r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
      r.dx = (float)d[0]; r.dy = (float)d[1]; r.dz = (float)d[2];
      locate(p, g, r);
    }
    float w = 1.0f, sum = 0.0f;
    float pathL = 0.0f;                  // PATHLEN: the length of the legs walked, and what the path may still deposit
    long long left = (long long)cp.pathMax;
    long long *const strip = PATHLEN ? cp.bins + bin * (unsigned long long)cp.numBins : nullptr;
    for (uint32_t event = 1;; ++event) {
      if constexpr (SENSOR) {
        if (dropped) break;
      }
      if (event > cp.maxEvents) { dropped = true; break; }
      uint32_t q[4];
      philox4x32_10(event, pix, sLo, sHi, p.seedLo, p.seedHi, q);
      const float uX = u01(q[1]), uY = u01(q[2]), uZ = u01(q[3]);
      const float tau = fmaxf(-logf(fmaxf(u01(q[0]), FLT_MIN)), FLT_MIN);
      float t, acc;
      int end;
      if constexpr (EXPECT) {
        // the leg's whole ray, with the weight the leg starts with; a ray a bound ends drops the path, as a leg does
        float emitted;
        RayEnd ray;
        end = march_expected(p, cp, g, emis, r, tau, cp.maxLegCross, t, acc, emitted, ray);
        if (ray.how == RAY_BOUND) { dropped = true; break; }
        sum += w * emitted;
      } else {
        end = march(p, g, r, tau, cp.maxLegCross, t, acc);
      }
      if (end == END_TOP) break;
      if (end == END_BOUND) { dropped = true; break; }
      // where the leg ended, in the periodic image the walk stands in
      r.ox = r.ox + (double)r.dx * (double)t;
      r.oy = r.oy + (double)r.dy * (double)t;
      if constexpr (PATHLEN) pathL += t;
      if (end == END_SURFACE) {
        r.oz = p.zSurf;
        if constexpr (EMIT) {
          // The surface emits (1 - a) S_sfc of the column march() ended in, then reflects the rest of the path.  The whole event,
          // ending in `continue`: what follows is the solar event, left word for word as it was and dead in these instantiations
          // (a scope around its sun ray moves the sensor instantiations' control flow: their assembly is held to the parent's)
          const float a = camera_albedo(p, r.ox, r.oy);
          if constexpr (!EXPECT) sum += (w * (1.0f - a)) * cp.srcSurface[r.iy * p.nx + r.ix];
          w *= a;
          if (!(w > 0.0f)) break;
          float mu = sqrtf(uX);
          if (mu == 0.0f) mu = fmaxf(sqrtf(uZ), 1.52587890625e-05f);
          lambert_direction(mu, uY, r.dx, r.dy, r.dz);
          continue;
        }
        w *= camera_albedo(p, r.ox, r.oy);
        if (!(w > 0.0f)) break;
        bool bound;
        const float T = sun_transmittance(p, cp, g, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, bound);
        if (bound) { dropped = true; break; }
        if constexpr (PATHLEN) {
          const float Lsun = (float)(p.zMax - r.oz) * cp.invMu0;
          if (!path_deposit(cp, edges, hist, shared, strip, w * T * (1.0f / kPi), pathL + Lsun, left)) { dropped = true; break; }
        } else {
          sum += w * T * (1.0f / kPi);
        }
        float mu = sqrtf(uX);
        if (mu == 0.0f) mu = fmaxf(sqrtf(uZ), 1.52587890625e-05f);  // (a draw of exactly 0: the spare number, at least 2^-16)
        lambert_direction(mu, uY, r.dx, r.dy, r.dz);
        continue;
      }
      r.oz = r.oz + (double)r.dz * (double)t;
      const int cell = (r.iz * p.ny + r.iy) * p.nx + r.ix;
      int c = 0;  // component pick: findIndex over [0, cumExt(:)]
      for (int kc = 0; kc < p.nc - 1; kc++)
        if (uZ >= p.cum[(long long)kc * nvox + cell]) c = kc + 1;
      if constexpr (EMIT) {
        // the cell's emission along the path, before the weight is cut: a purely absorbing medium deposits and ends
        const float ssa = p.ssa[(long long)c * nvox + cell];
        if constexpr (!EXPECT) sum += (w * (1.0f - ssa)) * cp.srcCell[cell];
        w *= ssa;
      } else {
        w *= p.ssa[(long long)c * nvox + cell];
      }
      if (!(w > 0.0f)) break;
      const int pfEntry = p.pfi[(long long)c * nvox + cell];
      if constexpr (!EMIT) {
        // the local estimate toward the sun: Theta between the sun's direction of travel and -d, the direction the light
        // travels along this leg; P by the reference's linear interpolation in angle (lookUpPhaseFuncValsFromTable)
        float proj = r.dx * cp.sun[0] + r.dy * cp.sun[1] + r.dz * cp.sun[2];
        if (fabsf(proj) > 1.0f) proj = copysignf(1.0f, proj);
        const float ang = acosf(proj);
        const int nA = cp.fwdNAngles[c];
        const float *ft = cp.fwd + cp.fwdOffset[c] + (long long)pfEntry * nA;
        const float deltaTheta = kPi / (float)(nA - 1);
        const int ai = (int)(ang / deltaTheta) + 1;
        float val;
        if (ai < nA) {
          const float wt = 1.0f - (ang - (float)(ai - 1) * deltaTheta) / deltaTheta;
          val = wt * ft[ai - 1] + (1.0f - wt) * ft[ai];
        } else {
          val = ft[nA - 1];
        }
        bool bound;
        const float T = sun_transmittance(p, cp, g, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, bound);
        if (bound) { dropped = true; break; }
        if constexpr (PATHLEN) {
          const float Lsun = (float)(p.zMax - r.oz) * cp.invMu0;
          if (!path_deposit(cp, edges, hist, shared, strip, (w * val) * (T * cp.invFourPiMu0), pathL + Lsun, left)) { dropped = true; break; }
        } else {
          sum += (w * val) * (T * cp.invFourPiMu0);
        }
      }
      if (p.useRR && w < 0.5f) {  // Russian roulette, RussianRouletteW = 1
        uint32_t q1[4];
        philox4x32_10(event | (1u << 24), pix, sLo, sHi, p.seedLo, p.seedHi, q1);
        const float uR = u01(q1[1]);
        if (uR >= w) break;
        w = 1.0f;
      }
      {
        // computeScatteringAngle (floor-type lookup of the inverse table) and next_direct with (cos, sin) of a uniform azimuth
        const int n = p.tblNSteps[c];
        const float *tb = p.tables + p.tblOffset[c] + (long long)pfEntry * n;
        const int ai = (int)(uX * (float)n) + 1;
        float ang;
        if (ai < n) {
          const float left = uX - (float)(ai - 1) * p.tblInvN[c];
          ang = (1.0f - left) * tb[ai - 1] + left * tb[ai];
        } else {
          ang = tb[n - 1];
        }
        const float cs = cos_0_pi(ang);
        float AX, AY;
        sincos_2pi(uY, AX, AY);
        float B = sqrtf(fmaxf(1.0f - cs * cs, 0.0f));
        AX = AX * B;
        AY = AY * B;
        B = r.dx * AX - r.dy * AY;
        const float D = cs - B / (1.0f + fabsf(r.dz));
        r.dx = r.dx * D + AX;
        r.dy = r.dy * D - AY;
        r.dz = r.dz * cs - copysignf(fabsf(B), r.dz * B);
      }
    }
    if constexpr (SENSOR && EMIT) {
      // no direct part (c = 0 for every sensor): one bin array, the sum in units of the largest source value
      bool ok = !dropped && sum == sum;
      if constexpr (EXPECT) ok = ok && (double)sum * cp.invSrcMax * cp.scale < cp.pathMax;
      if (valid && !ok) atomicAdd(cp.dropped, 1ull);
      const long long vEmitted = ok ? __double2ll_rn(fmin((double)sum * cp.invSrcMax * cp.scale, cp.pathMax)) : 0;
      wave_add(cp.bins, bin32, vEmitted, lane);
    } else if constexpr (SENSOR) {
      // (a NaN from a table: counted like a path a bound ended, contributes to neither part)
      // The direct beam on the receiver at the path's origin, found again from the path's first block: nothing of it is carried
      // through the legs (registers).  A sun ray a bound ends drops the path.
      float sumDirect = 0.0f;
      {
        const SensorGeometry &sg = cp.sensors[bin32 % (uint32_t)cp.npix];
        const float direct = sg.direct;
        if (!dropped && direct > 0.0f) {
          uint32_t q[4];
          philox4x32_10(0u, pix, sLo, sHi, p.seedLo, p.seedHi, q);
          double o[3];
          sensor_origin(sg, (double)u01(q[0]), (double)u01(q[1]), o);
          Ray s;
          s.ox = o[0]; s.oy = o[1]; s.oz = o[2];
          locate(p, g, s);
          const float T = sun_transmittance(p, cp, g, s.ox, s.oy, s.oz, s.ix, s.iy, s.iz, dropped);
          sumDirect = T * direct;
        }
      }
      const bool ok = !dropped && sum == sum;
      if (valid && !ok) atomicAdd(cp.dropped, 1ull);  // (rare: counted at once, not carried in a register from path to path)
      const long long vDiffuse = ok ? __double2ll_rn(fmin((double)sum * cp.scale, cp.pathMax)) : 0;
      const long long vDirect = ok ? __double2ll_rn(fmin((double)sumDirect * cp.scale, cp.pathMax)) : 0;
      wave_add(cp.bins, bin32, vDiffuse, lane);
      wave_add(cp.binsDirect, bin32, vDirect, lane);
    } else if constexpr (PATHLEN) {
      // (what the path deposited before a bound or a NaN ended it stays in its bins: the plain camera drops such a path whole)
      if (dropped) nDropped++;
    } else {
      if (dropped || !(sum == sum)) {  // (a NaN from a table: counted like a path a bound ended, contributes nothing)
        nDropped++;
      } else if (EXPECT && !((double)sum * cp.invSrcMax * cp.scale < cp.pathMax)) {
        nDropped++;
      } else if constexpr (EMIT) {
        pend += __double2ll_rn(fmin((double)sum * cp.invSrcMax * cp.scale, cp.pathMax));
      } else {
        pend += __double2ll_rn(fmin((double)sum * cp.scale, cp.pathMax));
      }
    }
  }

  if constexpr (PATHLEN) {
    if (tag != ~0ull) path_flush(hist, cp.bins + tag * (unsigned long long)cp.numBins, cp.numBins, lane);
  }
  if constexpr (!SENSOR && !PATHLEN) {
    // The lanes of a wave mostly hold sums for ONE bin (pixel-major indices, samplesPerPixel >= 64): then one add per wave.
    const bool have = pend != 0;
    const unsigned long long haveMask = __ballot(have);
    if (haveMask != 0ull) {
      const int first = __ffsll((long long)haveMask) - 1;
      const unsigned long long firstBin = __shfl(pendBin, first);
      if (__ballot(have && pendBin != firstBin) == 0ull) {
        long long v = have ? pend : 0;
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(cp.bins + firstBin), (unsigned long long)v);
      } else if (have) {
        atomicAdd(reinterpret_cast<unsigned long long *>(cp.bins + pendBin), (unsigned long long)pend);
      }
    }
  }
  if constexpr (!SENSOR) {
    if (nDropped != 0u) atomicAdd(cp.dropped, (unsigned long long)nDropped);
  }
}

// mcbrat_sun_transmittance: the kernel's own T_sun on given points, one lane per point
template <int BLOCK, bool GRID_LDS>
__global__ void __launch_bounds__(BLOCK) sun_transmittance_kernel(const DevParams p, const CamParams cp) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const GridView g = grid_view<BLOCK, GRID_LDS>(p, smem_raw);
  unsigned nDropped = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < cp.nPoints; i += (long long)gridDim.x * BLOCK) {
    Ray r{cp.points[3 * i], cp.points[3 * i + 1], cp.points[3 * i + 2], 0.f, 0.f, 0.f, 0, 0, 0};
    locate(p, g, r);
    bool bound;
    const float T = sun_transmittance(p, cp, g, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, bound);
    cp.transmittance[i] = bound ? __uint_as_float(0x7fc00000u) : T;
    if (bound) nDropped++;
  }
  if (nDropped != 0u) atomicAdd(cp.dropped, (unsigned long long)nDropped);
}

// The set-up of a render with the expected-value estimator: E[v] of every cell, from the context's dense
// grids and the caller's cellSource (mcbrat_expected.h: expected_emission), one lane per cell
__global__ void __launch_bounds__(256) emission_grid_kernel(const DevParams p, const float *srcCell, float *emis) {
  const long long nvox = (long long)p.nx * p.ny * p.nz, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < nvox) emis[i] = expected_emission(p.nc, p.nc > 1 ? p.cum + i : nullptr, p.ssa + i, nvox, p.ext[i], srcCell[i]);
}

}  // namespace mcbrat

using namespace mcbrat;

namespace {

constexpr size_t kCameraGridLds = 80 * 1024 - 1024;   // half of a compute unit's 160 KB, less the static part: two workgroups of 512 lanes
constexpr double kPi = 3.14159265358979323846;
// the refusals more than one entry words the same
constexpr const char *kNoCamera = "no camera or no array for the radiance.", *kNoSensor = "at least one sensor is needed (n < 1).",
                     *kNoSources = "no cellSource or no surfaceSource array (a null pointer).";

#define CAM_HIP(c, call)                                                                                          \
  do {                                                                                                            \
    const hipError_t e_ = static_cast<hipError_t>(call);                                                          \
    if (e_ != hipSuccess) return mcbrat_camera_fail(c, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

size_t grid_lds_bytes(const DevParams &p) { return mcbrat::grid_lds_bytes(p.nx, p.ny, p.nz); }  // (mcbrat_expected.h: the kernel's too)
static_assert(expected_lds_offset(24, 24, 24) == path_lds_offset(mcbrat::grid_lds_bytes(24, 24, 24)) && expected_lds_offset(1, 1, 2) == path_lds_offset(mcbrat::grid_lds_bytes(1, 1, 2)),
              "the emission grid lies where launch() and choose_grid_lds() count it: at path_lds_offset of the grid's bytes");
bool inside(const DevParams &p, double z) { return z >= p.z0 && z <= p.zMax; }

// the sun: unit vector toward it, the bound on the crossings of a ray toward it, 1 / (4 pi mu0)
void sun_setup(const DevParams &p, CamParams &cp) {
  for (int a = 0; a < 3; ++a) cp.sun[a] = -p.dir0[a];
  const SunBound b = sun_bound(p.nx, p.ny, p.nz, p.zMax - p.z0, p.Lx, p.Ly, cp.sun);
  cp.maxSunCross = b.maxCross; cp.invFourPiMu0 = b.invFourPiMu0; cp.invMu0 = b.invMu0;
}

// 0: global memory, 1: LDS; refused (asked for, does not fit): -1 the grid and the edges alone, -2 those with `extra`, what the
// entry keeps in LDS beside them (at path_lds_offset; 0: nothing): a path-length render's histograms, the emission grid of the
// expected-value estimator
int choose_grid_lds(const CameraContext &v, int asked, size_t extra) {
  const size_t share = std::min(kCameraGridLds, v.ldsPerCU / 2), grid = grid_lds_bytes(v.p);
  const bool gridFits = grid <= share, fits = extra ? path_lds_offset(grid) + extra <= share : gridFits;
  if (asked == 1 && !fits) return gridFits ? -2 : -1;
  return asked == 0 ? 0 : (fits ? 1 : 0);
}

// One launch of a kernel that has an instantiation for the grid in LDS and one for the grid in global memory
using BackwardKernel = void (*)(const DevParams, const CamParams);
// The solar instantiations (EMIT = false) by the three parameters they have had since section 4.20
template <int BLOCK, bool GRID_LDS, bool SENSOR>
constexpr BackwardKernel solar_camera_kernel() { return camera_kernel<BLOCK, GRID_LDS, SENSOR, false>; }
// extra: the entry's own LDS behind the grid's (a path-length render's histograms and edges, the expected-value estimator's
// emission grid, at path_lds_offset), or 0
int launch(mcbrat_ctx *c, const CameraContext &v, int lds, BackwardKernel inLds, BackwardKernel inGlobal, unsigned grid, int block, const CamParams &cp,
           size_t extra) {
  const BackwardKernel kernel = lds ? inLds : inGlobal;
  const size_t gridBytes = lds ? grid_lds_bytes(v.p) : 0, bytes = extra ? path_lds_offset(gridBytes) + extra : gridBytes;
  if (bytes > 48 * 1024) CAM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), bytes, v.stream, v.p, cp);
  CAM_HIP(c, hipGetLastError());
  return 0;
}

// What is an entry's own in the shared path of a backward render: how it words the refusals, its bin arrays, its instantiations
struct Entry {
  const char *name;                // the prefix of every message
  const char *samples;             // its argument for the samples per bin
  const char *bins;                // its bins, as the budget's refusal names them
  const char *subject;             // "the backward camera", "the backward sensors"
  unsigned long long arrays;       // bin arrays: 1, or 2 (diffuse, then direct)
  BackwardKernel inLds, inGlobal;  // workgroups of 512 and of 256 lanes
  bool ownName = false;            // camera_refusal's texts go out under `name` (false: as they are, under the solar camera's)
};
// n: pixels or sensors; slots: the sums each of them has per batch (the path-length bins of a pixel)
struct Counts { unsigned long long n; int64_t samples; int32_t numBatches; uint64_t firstSample; unsigned long long slots = 1; };
// The sources of an emission render, as the caller handed them over; srcMax, the largest value: emission_sources()'s
struct EmissionSources { const float *cell, *surface; double srcMax; };
struct PathEdges { const float *edges; int numBins; };  // the caller's array: checked by the camera front, uploaded by backward_render
// One backward render, as its entry asks for it: host only.  What not every entry has is a member that is present or absent
struct Request {
  Counts counts;                          // (n and slots: the front's)
  uint64_t seed;
  int gridInLds;                          // (a camera's: the front's)
  std::vector<SensorGeometry> sensors;    // a sensor entry: the receivers (the front's); empty: a camera, its geometry is cp.g
  std::optional<double> largestOwn;       // the largest estimate the entry adds to the paths' own
  std::optional<EmissionSources> sources; // an emission render: no sun, no forward tables, no rule about the source
  std::optional<PathEdges> path;          // a render by path length
  bool expected = false;                  // an emission render with the expected-value estimator
};

int fail(mcbrat_ctx *c, const Entry &e, const std::string &text) { return mcbrat_camera_fail(c, (std::string(e.name) + ": " + text).c_str()); }
// A text of camera_refusal or sensor_refusal: as it is, under the solar entry's name, or under the entry's own
int receiver_fail(mcbrat_ctx *c, const Entry &e, const char *msg) {
  const char *colon = std::strchr(msg, ':');
  return e.ownName ? fail(c, e, colon ? colon + 2 : msg) : mcbrat_camera_fail(c, msg);
}

// Stage 1, before anything of the call's arrays or of the context is read: samples, batches, budget, index count
int check_counts(mcbrat_ctx *c, const Entry &e, const Counts &k) {
  if (k.samples < 1) return fail(c, e, std::string(e.samples) + " must be at least 1.");
  if (k.numBatches < 1) return fail(c, e, "numBatches must be at least 1.");
  if (!bins_fit(k.n * k.slots, (unsigned long long)k.numBatches, (int)e.arrays)) return fail(c, e, std::string("the bins of ") + e.bins + " do not fit the tally budget of 4 GiB.");
  if (!paths_fit(k.n * (unsigned long long)k.numBatches, k.samples, k.firstSample, k.numBatches)) return fail(c, e, "more paths than a 64-bit index counts.");
  return 0;
}

// Stage 2: the view of the context, and what a backward render needs of it (solar: the Directional source too)
int backward_context(mcbrat_ctx *c, const Entry &e, bool solar, CameraContext &v) {
  if (mcbrat_camera_context(c, &v, false)) return 1;
  if (!v.haveGrid || !v.haveOptics) return fail(c, e, "problem not completely specified (grid and optical properties).");
  const std::string subject = e.subject;
  if (solar && (!v.haveSource || !v.solarDirectional)) return fail(c, e, subject + (subject.back() == 's' ? " need" : " needs") + " the Directional solar source.");
  if (v.brdfSurface) return fail(c, e, "a BRDF surface is not supported by " + subject + " (Lambertian surfaces only).");
  return 0;
}

// The front of the three camera entries, behind their own null checks: the camera's rules and the edges', stage 1 with the
// entry's slots, stage 2, the height.  -> q.counts, q.gridInLds, v, and cp zeroed but for the camera's geometry
int camera_front(mcbrat_ctx *c, const Entry &e, const mcbrat_camera &cam, Request &q, CameraContext &v, CamParams &cp) {
  if (const char *msg = camera_refusal(cam)) return receiver_fail(c, e, msg);
  if (q.path)
    if (const char *msg = path_edges_refusal(q.path->edges, q.path->numBins)) return fail(c, e, msg);
  q.counts.n = (unsigned long long)cam.npx * (unsigned long long)cam.npy;
  q.counts.slots = q.path ? (unsigned long long)q.path->numBins : 1;
  q.gridInLds = cam.gridInLds;
  if (check_counts(c, e, q.counts) || backward_context(c, e, !q.sources, v)) return 1;
  if (!inside(v.p, cam.kind == 0 ? cam.z : cam.position[2])) return fail(c, e, "the camera's height lies outside the domain [z0, zMax].");
  std::memset(&cp, 0, sizeof(cp));
  camera_geometry(cam, cp.g); cp.jitter = cam.jitter != 0;
  return 0;
}

// The front of the two sensor entries, behind their own null checks: gridInLds, stage 1, the sensors' rules, stage 2, the
// corners.  -> q.counts, q.sensors (direct: 0), v, and cp zeroed
int sensor_front(mcbrat_ctx *c, const Entry &e, int64_t n, const mcbrat_sensor *sensors, Request &q, CameraContext &v, CamParams &cp) {
  if (q.gridInLds < -1 || q.gridInLds > 1) return fail(c, e, "gridInLds must be -1, 0 or 1.");
  q.counts.n = (unsigned long long)n;
  if (check_counts(c, e, q.counts)) return 1;
  for (int64_t i = 0; i < n; ++i)  // (after the budget: n sensors are read)
    if (const char *msg = sensor_refusal(sensors[i])) return receiver_fail(c, e, msg);
  if (backward_context(c, e, !q.sources, v)) return 1;
  for (int64_t i = 0; i < 4 * n; ++i) {  // (sensor i / 4, corner i % 4)
    const mcbrat_sensor &s = sensors[i / 4];
    if (!inside(v.p, s.position[2] + ((i & 1) ? s.e1[2] : 0.0) + ((i & 2) ? s.e2[2] : 0.0)))
      return fail(c, e, "a corner of a sensor's receiver lies outside the domain [z0, zMax].");
  }
  q.sensors.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) sensor_geometry(sensors[i], q.sensors[(size_t)i]);
  std::memset(&cp, 0, sizeof(cp));
  return 0;
}
// w0, the solid angle a sensor's parts are tallied in units of: pi (planar), 4 pi (spherical); the value of one count of its bins
double sensor_w0(const mcbrat_sensor &s) { return s.kind == 0 ? kPi : 4.0 * kPi; }
std::vector<double> sensor_units(int64_t n, const mcbrat_sensor *sensors, double unit) {
  std::vector<double> units((size_t)n);
  for (int64_t i = 0; i < n; ++i) units[(size_t)i] = unit * sensor_w0(sensors[i]);
  return units;
}

// An emission entry's own check of its two source arrays against the grid: every value finite and not negative, not all zero.
// -> src.srcMax, the largest value
int emission_sources(mcbrat_ctx *c, const Entry &e, const CameraContext &v, EmissionSources &src) {
  const size_t ncol = (size_t)v.p.nx * (size_t)v.p.ny, nvox = ncol * (size_t)v.p.nz;
  float largest = 0.0f;
  for (int part = 0; part < 2; ++part) {
    const float *s = part ? src.surface : src.cell;
    const size_t n = part ? ncol : nvox;
    for (size_t i = 0; i < n; ++i) {
      if (!std::isfinite(s[i]) || s[i] < 0.0f) return fail(c, e, std::string(part ? "surfaceSource" : "cellSource") + " holds a value that is negative or not finite.");
      largest = std::max(largest, s[i]);
    }
  }
  if (!(largest > 0.0f)) return fail(c, e, "cellSource and surfaceSource are all zero: nothing emits.");
  src.srcMax = (double)largest;
  return 0;
}

// Stage 3, behind the front and the entry's own checks: the forward and the inverse tables, the LDS share, then the launch.
// cp: as the front left it.  With q.sources no sun is set up and no forward table is read.
// -> bins [arrays][numBatches][n][slots] and `unit`, the value of one count of a bin in the caller's units; *dropped
int backward_render(mcbrat_ctx *c, const Entry &e, CameraContext &v, const Request &q, CamParams &cp, std::vector<long long> &bins, double &unit,
                    int64_t *dropped) {
  const Counts &k = q.counts;
  std::vector<float> fwdAll;  // the forward tables, components concatenated, and the largest value they hold
  float fwdMax = 0.0f;
  for (int i = 0; i < (q.sources ? 0 : v.nc); ++i) {
    if ((int)v.fwd->size() <= i || (*v.fwd)[i].empty()) return fail(c, e, "no forward phase function table for component " + std::to_string(i + 1));
    if ((*v.maxPfi)[i] >= (*v.fwdNEntries)[i]) return fail(c, e, "phaseFunctionIndex exceeds forward table entries for component " + std::to_string(i + 1));
    cp.fwdOffset[i] = (int)fwdAll.size(); cp.fwdNAngles[i] = (*v.fwdNAngles)[i];
    fwdAll.insert(fwdAll.end(), (*v.fwd)[i].begin(), (*v.fwd)[i].end());
    for (float x : (*v.fwd)[i]) if (x > fwdMax) fwdMax = x;  // (a NaN never compares greater)
  }
  if (mcbrat_camera_context(c, &v, true)) return 1;  // (the inverse tables: the context's own refusal text where one is missing)
  // (a path-length render: histograms and edges for the 512 lanes of the LDS instantiation count against the share with the grid)
  // (the expected-value estimator: the emission grid, as large as the extinction grid, counts in the same way)
  const int numBins = q.path ? q.path->numBins : 0;
  const size_t emisBytes = q.expected ? expected_lds_bytes(v.p.nx, v.p.ny, v.p.nz) : 0;
  const int lds = choose_grid_lds(v, q.gridInLds, numBins ? path_lds_bytes(numBins, 512) : emisBytes);
  if (lds == -1) return fail(c, e, "gridInLds = 1, but the extinction grid and the edges do not fit the LDS share.");
  if (lds == -2 && q.expected) return fail(c, e, "gridInLds = 1, but the extinction grid and the emission grid do not fit the LDS share together.");
  if (lds == -2) return fail(c, e, "gridInLds = 1, but the extinction grid and the path-length histograms do not fit the LDS share together.");

  const unsigned long long nBins = k.n * (unsigned long long)k.numBatches;
  cp.spp = (unsigned long long)k.samples; cp.npix = k.n; cp.firstSample = k.firstSample;
  cp.total = nBins * cp.spp;
  cp.numBins = numBins; cp.pathDirect = q.path && v.pathBinsInLds == 0;
  if (!q.sources) sun_setup(v.p, cp);
  cp.maxLegCross = leg_bound(v.p.nx, v.p.ny, v.p.nz, v.p.zMax - v.p.z0, v.p.Lx, v.p.Ly); cp.maxEvents = kCameraMaxEvents;
  // (an emission path's deposits are tallied in units of the largest source value: the candidate is 1)
  const FixedPoint fixed = q.sources ? fixed_point(k.samples, {1.0}) : fixed_point(k.samples, {(double)fwdMax * (double)cp.invFourPiMu0, 1.0 / kPi, q.largestOwn.value_or(0.0)});
  cp.scale = fixed.scale; cp.pathMax = fixed.pathMax;
  v.p.seedLo = (uint32_t)q.seed; v.p.seedHi = (uint32_t)(q.seed >> 32);

  DeviceBuffer<long long> dBins;
  DeviceBuffer<float> dFwd, dSrcCell, dSrcSurface, dEdges, dEmis;
  DeviceBuffer<unsigned long long> dDropped;
  DeviceBuffer<SensorGeometry> dGeo;
  const size_t allBins = (size_t)(e.arrays * nBins * k.slots);
  CAM_HIP(c, dBins.allocate(allBins));
  CAM_HIP(c, dFwd.allocate(std::max<size_t>(fwdAll.size(), 1)));
  CAM_HIP(c, dDropped.allocate(1));
  CAM_HIP(c, hipMemsetAsync(dBins.get(), 0, sizeof(long long) * allBins, v.stream));
  CAM_HIP(c, hipMemsetAsync(dDropped.get(), 0, sizeof(unsigned long long), v.stream));
  CAM_HIP(c, hipMemcpyAsync(dFwd.get(), fwdAll.data(), sizeof(float) * fwdAll.size(), hipMemcpyHostToDevice, v.stream));
  cp.bins = dBins.get(); cp.binsDirect = e.arrays == 2 ? dBins.get() + nBins : nullptr; cp.fwd = dFwd.get(); cp.dropped = dDropped.get();
  if (q.sources) {
    const size_t ncol = (size_t)v.p.nx * (size_t)v.p.ny, nvox = ncol * (size_t)v.p.nz;
    CAM_HIP(c, dSrcCell.allocate(nvox));
    CAM_HIP(c, dSrcSurface.allocate(ncol));
    CAM_HIP(c, hipMemcpyAsync(dSrcCell.get(), q.sources->cell, sizeof(float) * nvox, hipMemcpyHostToDevice, v.stream));
    CAM_HIP(c, hipMemcpyAsync(dSrcSurface.get(), q.sources->surface, sizeof(float) * ncol, hipMemcpyHostToDevice, v.stream));
    cp.srcCell = dSrcCell.get(); cp.srcSurface = dSrcSurface.get(); cp.invSrcMax = 1.0 / q.sources->srcMax;
    if (q.expected) {
      CAM_HIP(c, dEmis.allocate(nvox));
      hipLaunchKernelGGL(emission_grid_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, v.stream, v.p, cp.srcCell, dEmis.get());
      CAM_HIP(c, hipGetLastError());
      cp.emisCell = dEmis.get();
    }
  }
  if (q.path) {
    CAM_HIP(c, dEdges.allocate((size_t)numBins));
    CAM_HIP(c, hipMemcpyAsync(dEdges.get(), q.path->edges, sizeof(float) * (size_t)numBins, hipMemcpyHostToDevice, v.stream));
    cp.pathEdges = dEdges.get();
  }
  if (!q.sensors.empty()) {
    CAM_HIP(c, dGeo.allocate(q.sensors.size()));
    CAM_HIP(c, hipMemcpyAsync(dGeo.get(), q.sensors.data(), sizeof(SensorGeometry) * q.sensors.size(), hipMemcpyHostToDevice, v.stream));
    cp.sensors = dGeo.get();
  }

  // indices are bin-major, so a wave's lanes share a bin wherever the samples per bin are 64 or more
  const int block = lds ? 512 : 256;
  const LaunchShape shape = launch_shape(cp.total, v.numCUs, block);
  cp.pathsPerLane = shape.pathsPerLane;
  if (shape.blocks > 0x7fffffffull) return fail(c, e, "more paths than one launch takes.");
  if (launch(c, v, lds, e.inLds, e.inGlobal, (unsigned)shape.blocks, block, cp, numBins ? path_lds_bytes(numBins, block) : (lds ? emisBytes : 0))) return 1;
  bins.resize(allBins);
  unsigned long long nDropped = 0;
  CAM_HIP(c, hipMemcpyAsync(bins.data(), dBins.get(), sizeof(long long) * allBins, hipMemcpyDeviceToHost, v.stream));
  CAM_HIP(c, hipMemcpyAsync(&nDropped, dDropped.get(), sizeof(nDropped), hipMemcpyDeviceToHost, v.stream));
  CAM_HIP(c, hipStreamSynchronize(v.stream));
  if (dropped) *dropped = (int64_t)nDropped;
  // (an emission render's bins are in units of srcMax: the caller's units come back here, in double)
  unit = (q.sources ? q.sources->srcMax : 1.0) / (cp.scale * (double)k.samples);
  return 0;
}

// The three camera entries behind their null checks: the front, the emission entry's sources, stage 3, the reduction to images
// [slot][pixel]
int render_camera(mcbrat_ctx *c, const Entry &e, const mcbrat_camera &cam, Request &q, float *radiance, float *radianceStdErr, float *batchMeans,
                  int64_t *dropped) {
  CameraContext v;
  CamParams cp;
  if (camera_front(c, e, cam, q, v, cp)) return 1;
  if (q.sources && emission_sources(c, e, v, *q.sources)) return 1;
  std::vector<long long> bins;  // [numBatches][npix][slots]: a pixel's bins lie together on the device
  double unit;
  if (backward_render(c, e, v, q, cp, bins, unit, dropped)) return 1;
  const std::vector<double> units((size_t)q.counts.n, unit);
  reduce_batches(bins.data(), 1, q.counts.numBatches, (size_t)q.counts.n, (size_t)q.counts.slots, units.data(), {{radiance, nullptr}, {radianceStdErr, nullptr}, nullptr, batchMeans});
  return 0;
}

// The two emission sensor entries behind their Entry: the null checks, the front, the sources, stage 3, the reduction
int render_sensors_emission(mcbrat_ctx *c, const Entry &e, bool expected, int64_t n, const mcbrat_sensor *sensors, const float *cellSource,
                            const float *surfaceSource, uint64_t seed, uint64_t firstSample, int64_t samplesPerSensor, int32_t numBatches, int32_t gridInLds,
                            float *irradiance, float *irradianceStdErr, float *batchMeans, int64_t *dropped) {
  if (!c) return 1;
  if (n < 1) return fail(c, e, kNoSensor);
  if (!sensors || !irradiance) return fail(c, e, "no sensors or no array for the irradiance.");
  if (!cellSource || !surfaceSource) return fail(c, e, kNoSources);
  Request q = {{0, samplesPerSensor, numBatches, firstSample}, seed, gridInLds};
  q.sources = EmissionSources{cellSource, surfaceSource, 0.0};
  q.expected = expected;
  CameraContext v;
  CamParams cp;
  if (sensor_front(c, e, n, sensors, q, v, cp) || emission_sources(c, e, v, *q.sources)) return 1;
  for (SensorGeometry &g : q.sensors) g.direct = 0.0f;
  std::vector<long long> bins;  // [numBatches][n]
  double unit;
  if (backward_render(c, e, v, q, cp, bins, unit, dropped)) return 1;
  reduce_batches(bins.data(), 1, numBatches, (size_t)n, 1, sensor_units(n, sensors, unit).data(), {{irradiance, nullptr}, {irradianceStdErr, nullptr}, nullptr, batchMeans});
  return 0;
}

}  // namespace

extern "C" {

int mcbrat_camera_ray(const mcbrat_camera *cam, int32_t i, int32_t j, double u, double v, double origin[3], double direction[3]) {
  if (!cam || !origin || !direction || camera_refusal(*cam)) return 1;
  CameraGeometry g;
  camera_geometry(*cam, g);
  camera_ray(g, i, j, u, v, origin, direction);
  return 0;
}

int mcbrat_sun_transmittance(mcbrat_ctx *c, int64_t n, const double *xyz, float *transmittance) {
  if (!c) return 1;
  if (n < 0 || (n > 0 && (!xyz || !transmittance))) return mcbrat_camera_fail(c, "sunTransmittance: no points.");
  CameraContext v;
  if (mcbrat_camera_context(c, &v, false)) return 1;
  if (!v.haveGrid || !v.haveOptics) return mcbrat_camera_fail(c, "sunTransmittance: problem not completely specified (grid and optical properties).");
  if (!v.solarDirectional) return mcbrat_camera_fail(c, "sunTransmittance: needs the Directional solar source.");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !inside(v.p, xyz[3 * i + 2]))
      return mcbrat_camera_fail(c, "sunTransmittance: a point is not finite or lies outside [z0, zMax].");
  if (n == 0) return 0;
  const int lds = choose_grid_lds(v, v.gridInLds, 0);
  if (lds < 0) return mcbrat_camera_fail(c, "sunTransmittance: the grid does not fit the LDS share (option cameraGridInLds = 1).");
  DeviceBuffer<double> dPoints;
  DeviceBuffer<float> dT;
  DeviceBuffer<unsigned long long> dDropped;
  CAM_HIP(c, dPoints.allocate((size_t)3 * n));
  CAM_HIP(c, dT.allocate((size_t)n));
  CAM_HIP(c, dDropped.allocate(1));
  CAM_HIP(c, hipMemcpyAsync(dPoints.get(), xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, v.stream));
  CAM_HIP(c, hipMemsetAsync(dDropped.get(), 0, sizeof(unsigned long long), v.stream));
  CamParams cp;
  std::memset(&cp, 0, sizeof(cp));
  sun_setup(v.p, cp);
  cp.points = dPoints.get(); cp.transmittance = dT.get(); cp.nPoints = n; cp.dropped = dDropped.get();
  constexpr int kBlock = 256;
  const unsigned grid = (unsigned)std::min<long long>((n + kBlock - 1) / kBlock, (long long)v.numCUs * 8);
  if (launch(c, v, lds, sun_transmittance_kernel<kBlock, true>, sun_transmittance_kernel<kBlock, false>, grid, kBlock, cp, 0)) return 1;
  unsigned long long dropped = 0;
  CAM_HIP(c, hipMemcpyAsync(transmittance, dT.get(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, v.stream));
  CAM_HIP(c, hipMemcpyAsync(&dropped, dDropped.get(), sizeof(dropped), hipMemcpyDeviceToHost, v.stream));
  CAM_HIP(c, hipStreamSynchronize(v.stream));
  if (dropped != 0) return mcbrat_camera_fail(c, "sunTransmittance: a ray did not reach the top within the bound on its crossings.");
  return 0;
}

int mcbrat_render_camera(mcbrat_ctx *c, const mcbrat_camera *cam, uint64_t seed, uint64_t firstSample, int64_t samplesPerPixel,
                         int32_t numBatches, float *radiance, float *radianceStdErr, float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderCamera", "samplesPerPixel", "the image's batches (npx * npy * numBatches)", "the backward camera", 1,
                   solar_camera_kernel<512, true, false>(), solar_camera_kernel<256, false, false>()};
  if (!c) return 1;
  if (!cam || !radiance) return fail(c, e, kNoCamera);
  Request q = {{0, samplesPerPixel, numBatches, firstSample}, seed};
  return render_camera(c, e, *cam, q, radiance, radianceStdErr, batchMeans, dropped);
}

// The radiance by photon path length: mcbrat_render_camera's paths, every estimate tallied on its own in
// the path-length bin of its pixel; numBins sums per pixel and batch
int mcbrat_render_camera_pathlengths(mcbrat_ctx *c, const mcbrat_camera *cam, int32_t numBins, const float *pathEdges, uint64_t seed,
                                     uint64_t firstSample, int64_t samplesPerPixel, int32_t numBatches, float *radiance, float *radianceStdErr,
                                     float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderCameraPathLengths", "samplesPerPixel", "the image's batches (npx * npy * numBins * numBatches)", "the backward camera", 1,
                   camera_kernel<512, true, false, false, true>, camera_kernel<256, false, false, false, true>, true};
  if (!c) return 1;
  if (!cam || !radiance || !pathEdges) return fail(c, e, "no camera, no array for the radiance or no pathEdges array.");
  Request q = {{0, samplesPerPixel, numBatches, firstSample}, seed};
  q.path = PathEdges{pathEdges, numBins};
  return render_camera(c, e, *cam, q, radiance, radianceStdErr, batchMeans, dropped);
}

int mcbrat_sensor_ray(const mcbrat_sensor *sensor, double u, double v, double a, double cc, double origin[3], double direction[3]) {
  if (!sensor || !origin || !direction || sensor_refusal(*sensor)) return 1;
  SensorGeometry g;
  sensor_geometry(*sensor, g);
  sensor_ray(g, u, v, a, cc, origin, direction);
  return 0;
}

int mcbrat_render_sensors(mcbrat_ctx *c, int64_t n, const mcbrat_sensor *sensors, uint64_t seed, uint64_t firstSample,
                          int64_t samplesPerSensor, int32_t numBatches, int32_t gridInLds, float *diffuse, float *direct,
                          float *diffuseStdErr, float *directStdErr, float *totalStdErr, float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderSensors", "samplesPerSensor", "the sensors' batches (2 * n * numBatches)", "the backward sensors", 2,
                   solar_camera_kernel<512, true, true>(), solar_camera_kernel<256, false, true>()};
  if (!c) return 1;
  if (n < 1) return fail(c, e, kNoSensor);
  if (!sensors || !diffuse || !direct) return fail(c, e, "no sensors or no arrays for the diffuse and the direct part.");
  Request q = {{0, samplesPerSensor, numBatches, firstSample}, seed, gridInLds};
  CameraContext v;
  CamParams cp;
  if (sensor_front(c, e, n, sensors, q, v, cp)) return 1;
  // the sun in double, as mcbrat_set_source_solar's float direction gives it; mu0 = its cosine
  double sun[3], sn = 0.0;
  for (int a = 0; a < 3; ++a) { sun[a] = -(double)v.p.dir0[a]; sn += sun[a] * sun[a]; }
  sn = std::sqrt(sn);
  for (int a = 0; a < 3; ++a) sun[a] /= sn;
  const double mu0 = std::max(std::fabs(sun[2]), (double)FLT_MIN);
  for (int64_t i = 0; i < n; ++i) {
    double cDirect = 1.0 / mu0;
    if (sensors[i].kind == 0) {
      const double *nv = q.sensors[(size_t)i].n;
      cDirect = std::max(0.0, nv[0] * sun[0] + nv[1] * sun[1] + nv[2] * sun[2]) / mu0;
    }
    q.sensors[(size_t)i].direct = (float)(cDirect / sensor_w0(sensors[i]));  // (both parts are tallied in units of w0)
  }
  q.largestOwn = 1.0 / (kPi * mu0);  // (the direct estimate, c / w0, is at most 1 / (pi mu0))
  std::vector<long long> bins;      // [2][numBatches][n]: diffuse, then direct
  double unit;
  if (backward_render(c, e, v, q, cp, bins, unit, dropped)) return 1;
  // the diffuse part, the direct part and the per-batch sum of the two, each a series of its own
  reduce_batches(bins.data(), 2, numBatches, (size_t)n, 1, sensor_units(n, sensors, unit).data(), {{diffuse, direct}, {diffuseStdErr, directStdErr}, totalStdErr, batchMeans});
  return 0;
}

// The emission camera: one bin array, the caller's sources
int mcbrat_render_camera_emission(mcbrat_ctx *c, const mcbrat_camera *cam, const float *cellSource, const float *surfaceSource, uint64_t seed,
                                  uint64_t firstSample, int64_t samplesPerPixel, int32_t numBatches, float *radiance, float *radianceStdErr,
                                  float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderCameraEmission", "samplesPerPixel", "the image's batches (npx * npy * numBatches)", "the emission camera", 1,
                   camera_kernel<512, true, false, true>, camera_kernel<256, false, false, true>};
  if (!c) return 1;
  if (!cam || !radiance) return fail(c, e, kNoCamera);
  if (!cellSource || !surfaceSource) return fail(c, e, kNoSources);
  Request q = {{0, samplesPerPixel, numBatches, firstSample}, seed};
  q.sources = EmissionSources{cellSource, surfaceSource, 0.0};
  return render_camera(c, e, *cam, q, radiance, radianceStdErr, batchMeans, dropped);
}

// The emission sensors: one bin array, no direct part (nothing comes in from above)
int mcbrat_render_sensors_emission(mcbrat_ctx *c, int64_t n, const mcbrat_sensor *sensors, const float *cellSource, const float *surfaceSource,
                                   uint64_t seed, uint64_t firstSample, int64_t samplesPerSensor, int32_t numBatches, int32_t gridInLds,
                                   float *irradiance, float *irradianceStdErr, float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderSensorsEmission", "samplesPerSensor", "the sensors' batches (n * numBatches)", "the emission sensors", 1,
                   camera_kernel<512, true, true, true>, camera_kernel<256, false, true, true>};
  return render_sensors_emission(c, e, false, n, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, numBatches, gridInLds, irradiance,
                                 irradianceStdErr, batchMeans, dropped);
}

// The emission renders with the expected-value estimator: the emission entries' arguments, checks and
// outputs; the collision estimator's paths, every leg depositing its whole ray
int mcbrat_render_camera_emission_expected(mcbrat_ctx *c, const mcbrat_camera *cam, const float *cellSource, const float *surfaceSource, uint64_t seed,
                                           uint64_t firstSample, int64_t samplesPerPixel, int32_t numBatches, float *radiance, float *radianceStdErr,
                                           float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderCameraEmissionExpected", "samplesPerPixel", "the image's batches (npx * npy * numBatches)", "the emission camera", 1,
                   camera_kernel<512, true, false, true, false, true>, camera_kernel<256, false, false, true, false, true>, true};
  if (!c) return 1;
  if (!cam || !radiance) return fail(c, e, kNoCamera);
  if (!cellSource || !surfaceSource) return fail(c, e, kNoSources);
  Request q = {{0, samplesPerPixel, numBatches, firstSample}, seed};
  q.sources = EmissionSources{cellSource, surfaceSource, 0.0};
  q.expected = true;
  return render_camera(c, e, *cam, q, radiance, radianceStdErr, batchMeans, dropped);
}

int mcbrat_render_sensors_emission_expected(mcbrat_ctx *c, int64_t n, const mcbrat_sensor *sensors, const float *cellSource, const float *surfaceSource,
                                            uint64_t seed, uint64_t firstSample, int64_t samplesPerSensor, int32_t numBatches, int32_t gridInLds,
                                            float *irradiance, float *irradianceStdErr, float *batchMeans, int64_t *dropped) {
  const Entry e = {"renderSensorsEmissionExpected", "samplesPerSensor", "the sensors' batches (n * numBatches)", "the emission sensors", 1,
                   camera_kernel<512, true, true, true, false, true>, camera_kernel<256, false, true, true, false, true>, true};
  return render_sensors_emission(c, e, true, n, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, numBatches, gridInLds, irradiance,
                                 irradianceStdErr, batchMeans, dropped);
}

}  // extern "C"
