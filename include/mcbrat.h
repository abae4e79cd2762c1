/*
 * mcbrat.h -- C ABI of the MI355X-native photon-tracing integrator.
 *
 * This is the drop-in boundary for ONE path of MCBRaT3D: the integrator module
 * `monteCarloRadiativeTransfer` (Integrators/monteCarloRadiativeTransfer.f95,
 * public list :121-123).  Each entry point names the reference interface it
 * replaces.  Plain C types only: pointers, sizes, scalars.  All 3-D arrays are
 * Fortran order (x fastest, then y, z, component slowest) exactly as the
 * reference's getInfo_Domain hands them to computeRT (:434-443), so a Fortran
 * caller passes its arrays unchanged (see INTEGRATION.md for the
 * ISO_C_BINDING module).
 *
 * Error convention: every call returns 0 on success, non-zero on failure;
 * mcbrat_last_error() then holds the text the Fortran shim pushes with
 * setStateToFailure (src/ErrorMessages.f95:171-245).
 *
 * Threading: one context per GPU, not shared between host threads (the
 * reference integrator holds mutable tallies and is not thread-safe either).
 * There is no CPU fallback: mcbrat_create fails if no HIP device is usable.
 */
#ifndef MCBRAT_H
#define MCBRAT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCBRAT_MAX_COMPONENTS 8
#define MCBRAT_MAX_DIRECTIONS 64 /* intensity directions per run */
#define MCBRAT_ABI_VERSION 3

typedef struct mcbrat_ctx mcbrat_ctx;

/* Per-photon record written by mcbrat_trace_fates (parity/debug only). */
typedef struct {
  int32_t fate;     /* 0 top exit, 1 absorbed by surface, 2 roulette kill, 3 dropped by a loop bound (counters.badPhotons) */
  int32_t ix, iy, iz; /* 1-based cell of the final event */
  int32_t nScatter; /* scattering order at the end (:469, :643, :713) */
  int32_t nEvents;  /* legs traced */
  float weight;     /* weight tallied at the final event */
} mcbrat_fate;

/* Event counters of the last run (sums over photons), for the roofline figure. */
typedef struct {
  int64_t legs, crossings, collisions, absorbEvents, topExits, surfaceHits,
          rouletteKills, rouletteSurvivals;
  /* wave-level loop statistics: iterations of the walk loop and lanes walking in them, event
   * phases and lanes served in them, phases that launched photons / reflected off the surface */
  int64_t walkIterations, walkLanes, eventPhases, eventLanes, launchPhases, surfacePhases;
  /* Photons (and radiance rays) dropped since the context was created because they exceeded a loop bound of the
   * kernels -- the analogue of computeRT's nBad (Integrators/monteCarloRadiativeTransfer.f95:562-563: a photon whose
   * step is not positive is dropped and counted).  The reference's walk ends because it marches by cell index; the
   * kernels here bound every loop instead (legs per photon, loop iterations of a wave without any lane starting a
   * leg, length of a view ray), so that no input can keep a kernel from ending.  Always collected; 0 in every run
   * the tests and bench.py make.  (ABI version 2.) */
  int64_t badPhotons;
} mcbrat_counters;

int mcbrat_abi_version(void);

/* new_Integrator (:129-201) / finalize_Integrator (:1486-1547).
 * device: HIP device ordinal. */
mcbrat_ctx *mcbrat_create(int device);
void mcbrat_destroy(mcbrat_ctx *ctx);
const char *mcbrat_last_error(const mcbrat_ctx *ctx);

/* Domain geometry: getInfo_Domain(xPosition, yPosition, zPosition) as used by
 * new_Integrator :147-181.  Edges in km, nx+1 / ny+1 / nz+1 values. */
int mcbrat_set_grid(mcbrat_ctx *ctx, int32_t nx, int32_t ny, int32_t nz,
                    const double *xEdges, const double *yEdges, const double *zEdges);

/* Optical properties: getInfo_Domain(albedo, totalExt, cumExt, ssa, phaseFuncI)
 * as pulled by computeRT :441-443 (built by getOpticalPropertiesByComponent,
 * src/opticalProperties.f95:966-1072).  phaseFuncIndex is 1-based. */
int mcbrat_set_optics(mcbrat_ctx *ctx, int32_t nComponents, const double *totalExt,
                      const double *cumExt, const double *ssa, const int32_t *phaseFuncIndex,
                      double surfaceAlbedo);

/* inversePhaseFuncs(component)%values(nSteps, nEntries) (computeRT :443, :816-818;
 * built by tabulateInversePhaseFunctions, opticalProperties.f95:1817-1870).
 * component is 1-based; table is column-major (nSteps fastest). */
int mcbrat_set_inverse_table(mcbrat_ctx *ctx, int32_t component, int32_t nSteps,
                             int32_t nEntries, const float *table);

/* specifyParameters (:1046-1484): the keywords the driver passes
 * (monteCarloDriver.f95:540-572).  useRayTracing must be non-zero: the
 * max-cross-section branch is broken in the reference
 * and is rejected here. */
int mcbrat_specify_parameters(mcbrat_ctx *ctx, int32_t useRayTracing, int32_t useRussianRoulette,
                              float LW_flag);

/* new_PhotonStream, Directional form (src/monteCarloIllumination.f95:62-101). */
int mcbrat_set_source_solar(mcbrat_ctx *ctx, float solarMu, float solarAzimuthDeg);
/* new_PhotonStream, RandomAzimuth form (:103-140): mu = -|solarMu|, azimuth
 * uniform in [0, 2 pi) and position uniform per photon. */
int mcbrat_set_source_random_azimuth(mcbrat_ctx *ctx, float solarMu);
/* new_PhotonStream, Flux form (:142-176): isotropic (diffuse) incidence,
 * mu = -sqrt(U), azimuth and position uniform per photon.  A draw of mu = 0
 * is drawn again (the reference would launch that photon horizontally). */
int mcbrat_set_source_flux(mcbrat_ctx *ctx);
/* new_PhotonStream, Spotlight form (:178-216): every photon enters at the
 * point (solarX, solarY), given as fractions of the domain in (0, 1], in the
 * direction (solarMu, solarAzimuthDeg).  Negative fractions are refused (the
 * reference tests their absolute values and launches outside the domain). */
int mcbrat_set_source_spotlight(mcbrat_ctx *ctx, float solarMu, float solarAzimuthDeg, float solarX,
                                float solarY);
/* new_PhotonStream, BBEmission form (:431-522): the running voxel CDF and
 * atmosphere fraction from emission_weighting / getInfo_Weights. */
int mcbrat_set_source_emission(mcbrat_ctx *ctx, const double *voxelWeights, double fracAtmsPower);

/* computeRadiativeTransfer (:209-391) for nBatches consecutive batches of
 * photonsPerBatch photons, followed on the device by reportResults (:845-1042)
 * and the driver's moment accumulation (monteCarloDriver.f95:1023-1050) for each
 * batch.  Photon i of batch b has the global id firstPhotonId + b*photonsPerBatch + i;
 * its random numbers are Philox4x32-10(key = seed, counter = (event, block, id)),
 * so results do not depend on how photons are spread over GPUs.
 * numPhotonsProcessed (may be NULL) receives the total.
 * Capacity: the tallies are 64-bit integers of 2^-32 photon weights, so a bin holds
 * less than 2^31 unit weights per batch.  photonsPerBatch > 2^31 - 1 is refused
 * before anything is traced.  That bounds fluxUp and fluxDown over a black surface (a
 * photon reaches them once, with a weight of at most 1), and the volume absorption
 * without Russian roulette; it does NOT bound fluxDown over a reflecting surface (a
 * photon may arrive many times), fluxUp over a BRDF surface (mcbrat_set_surface_brdf: a
 * reflected weight may exceed 1), radiance, or the bins by scattering order of those,
 * which wrap around unreported. */
int mcbrat_compute_radiative_transfer(mcbrat_ctx *ctx, uint64_t seed, uint64_t firstPhotonId,
                                      int64_t photonsPerBatch, int32_t nBatches,
                                      int64_t *numPhotonsProcessed);

/* reportResults (:845-1042) for the LAST batch traced: normalised exactly as
 * computeRadiativeTransfer :328-364.  Any pointer may be NULL. */
int mcbrat_report_results(mcbrat_ctx *ctx, float *meanFluxUp, float *meanFluxDown,
                          float *meanFluxAbsorbed, float *fluxUp, float *fluxDown,
                          float *fluxAbsorbed, float *absorbedProfile, float *volumeAbsorption);

/* ---- radiance by local estimation (computeIntensityContribution :1623-1832) ---------------
 * specifyParameters(intensityMus, intensityPhis, computeIntensity, useRussianRouletteForIntensity,
 * zetaMin, useHybridPhaseFunsForIntenCalcs, numOrdersOrigPhaseFunIntenCalcs,
 * limitIntensityContributions, maxIntensityContribution) (:1046-1292).  nDirections = 0 turns the
 * intensity calculation off.  mus in [-1, 1] \ {0}, phis in degrees [0, 360].  Every emitted-photon
 * launch, surface reflection and scattering event then adds weight * phase function /
 * (4 pi |mu|) * transmission to the pixel where the view ray leaves the domain.
 * Roulette (Iwabuchi 2006, the driver's default) is accepted for upward directions only: for
 * mu < 0 the reference restarts its walk below the surface.  With limitIntensityContributions each
 * local estimate is clipped at maxIntensityContribution and the clipped excess of a (component,
 * direction) is spread over the pixels in proportion to that component's radiance field at the end
 * of the batch (:294-320, :1815-1826).  Changing the number of directions changes
 * mcbrat_moments_length(): a caller-bound moment buffer must be bound again. */
int mcbrat_specify_intensity(mcbrat_ctx *ctx, int32_t nDirections, const float *intensityMus,
                             const float *intensityPhisDeg, int32_t useRussianRouletteForIntensity,
                             float zetaMin, int32_t useHybridPhaseFunsForIntenCalcs,
                             int32_t numOrdersOrigPhaseFunIntenCalcs,
                             int32_t limitIntensityContributions, float maxIntensityContribution);
/* tabulatedPhaseFunctions(component)%values(nAngles, nEntries) and tabulatedOrigPhaseFunctions
 * (tabulateForwardPhaseFunctions, opticalProperties.f95:1872-1935; pulled by
 * computeIntensityContribution :1672): phase function values at nAngles scattering angles equally
 * spaced on [0, pi], angle fastest.  origTable = NULL when no hybrid tables are used. */
int mcbrat_set_forward_table(mcbrat_ctx *ctx, int32_t component, int32_t nAngles, int32_t nEntries,
                             const float *table, const float *origTable);
/* reportResults(meanIntensity, intensity) (:980-1010) for the LAST batch: intensity is
 * [nDirections][ny][nx] (x fastest).  Either pointer may be NULL. */
int mcbrat_report_intensity(mcbrat_ctx *ctx, float *meanIntensity, float *intensity);

/* ---- fluxes and radiances by scattering order ---------------------------------------------------
 * specifyParameters(recScatOrd, numRecScatOrd) (:1159-1171, :1293-1330).  numRecScatOrd < 0 turns the
 * recording off; >= 0 records orders 0..numRecScatOrd (no overflow bin: a higher order is not recorded,
 * :611).  A photon's order starts at 0 at launch and grows by one at every surface reflection (after the
 * fluxDown tally, :643) and every scattering event (before the local estimate, :713).  fluxUpByScatOrd gets
 * the weight of a top exit at the photon's order (:595-599), fluxDownByScatOrd that of a surface arrival at
 * the order before the reflection (:611-614, :635-638), intensityByScatOrd every local estimate at the order
 * the photon has when it is taken (:527-531, :688-692, :792-796).  Normalised as fluxUp and intensity
 * (:352-356, :381-387).  Fails together with limitIntensityContributions: the reference's redistribution
 * (:307-313) would add each clipped excess to every order.  Fails where one batch's order tallies would
 * not fit the tally budget.  Changes mcbrat_moments_length(): a caller-bound moment buffer must be bound
 * again.  Flux runs of small domains then run on the face-by-face kernels, not the block walk. */
int mcbrat_specify_scattering_orders(mcbrat_ctx *ctx, int32_t numRecScatOrd);
/* reportResults(meanFluxUpByScatOrd, meanFluxDownByScatOrd, fluxUpByScatOrd, fluxDownByScatOrd,
 * meanIntensityByScatOrd, intensityByScatOrd) (:850-864, :887-903, :1010-1040) for the LAST batch, Fortran
 * order with the order slowest: mean*(0:N), flux*(nx, ny, 0:N), meanIntensityByScatOrd(nDirections, 0:N),
 * intensityByScatOrd(nx, ny, nDirections, 0:N), N = numRecScatOrd.  Domain means are sums over the columns
 * divided by their number.  Any pointer may be NULL; the intensity ones must be NULL without directions. */
int mcbrat_report_scattering_orders(mcbrat_ctx *ctx, float *meanFluxUpByScatOrd, float *meanFluxDownByScatOrd,
                                    float *fluxUpByScatOrd, float *fluxDownByScatOrd,
                                    float *meanIntensityByScatOrd, float *intensityByScatOrd);

/* Upward and downward flux through every level of every column (specifyParameters(recLevelFluxes); an addition under ABI
 * version 3).  Level k = 0 .. nz is the face zPosition[k]: 0 the surface, nz the top.  A photon that
 * crosses level k adds its weight to levelFluxUp(x, y, k) or levelFluxDown(x, y, k) of the column it crosses in.  The launch of
 * a solar photon counts as a downward crossing of level nz (weight 1), a top exit as an upward one (the fluxUp deposit), a
 * surface arrival as a downward crossing of level 0 (the fluxDown deposit, before the albedo), the reflected photon as an
 * upward one with the reflected weight, a surface-emitted thermal photon as an upward one with weight 1.  Normalised as
 * fluxUp; levelFluxUp(:, :, nz) = fluxUp and levelFluxDown(:, :, 0) = fluxDown bit for bit.  Such runs use the face-by-face
 * walk: no layer skipping, no clear-air flight, no block walk (mcbrat_get_walk_mode reports it).  Fails together with
 * intensity directions, scattering orders, a BRDF surface, event counters / photon fates, and where one batch's level bins
 * would not fit the tally budget -- whichever call comes first.  Changes mcbrat_moments_length(): a caller-bound moment
 * buffer must be bound again. */
int mcbrat_specify_level_fluxes(mcbrat_ctx *ctx, int32_t enable);
/* The LAST batch, Fortran order with the level slowest: meanLevelFlux*(0:nz), levelFlux*(nx, ny, 0:nz).  Domain means are
 * sums over the columns divided by their number.  Any pointer may be NULL. */
int mcbrat_report_level_fluxes(mcbrat_ctx *ctx, float *meanLevelFluxUp, float *meanLevelFluxDown, float *levelFluxUp,
                               float *levelFluxDown);

/* The direct beam apart from the diffuse light in the downward level flux (specifyParameters(recDirectLevelFluxes); an addition
 * under ABI version 3).  A photon is direct from its launch until its first collision or its first
 * surface arrival, whichever comes first: any collision ends it, whatever the single-scattering albedo; periodic wrapping does
 * not; the surface arrival itself (the downward crossing of level 0) still counts, the reflection ends it.
 * levelFluxDownDirect(x, y, k) is the part of levelFluxDown(x, y, k) carried by direct photons, levelFluxDownDiffuse the rest:
 * the kernel tallies every downward crossing to ONE of the two and the total is the integer sum of the raw bins, so levelFluxUp
 * and levelFluxDown keep their bits.  Level nz is all direct (the launch is the crossing); there is no upward direct flux.
 * Needs level fluxes (fails without them, and mcbrat_specify_level_fluxes(0) fails while it is on) and a solar source
 * (mcbrat_compute_radiative_transfer fails with the thermal one); fails where one batch's three level parts would not fit the
 * tally budget.  Changes mcbrat_moments_length(): a caller-bound moment buffer must be bound again. */
int mcbrat_specify_direct_level_fluxes(mcbrat_ctx *ctx, int32_t enable);
/* The LAST batch, as mcbrat_report_level_fluxes: meanLevelFluxDownDirect / Diffuse(0:nz), levelFluxDownDirect / Diffuse(nx, ny, 0:nz).
 * Any pointer may be NULL. */
int mcbrat_report_direct_level_fluxes(mcbrat_ctx *ctx, float *meanLevelFluxDownDirect, float *meanLevelFluxDownDiffuse,
                                      float *levelFluxDownDirect, float *levelFluxDownDiffuse);

/* The actinic flux of every cell by track length (specifyParameters(recActinicFlux); an addition under ABI version 3; DESIGN.md
 * section 4.14).  The raw tally of cell (x, y, k) is the sum of w l over every piece of a photon's path inside the cell: w the
 * weight carried on that leg, l the piece's length in km -- the launch leg and the legs after a Lambertian reflection (with the
 * weight after the albedo) included.  actinicFlux(x, y, k) = sum / (photons per column * dz_k): dimensionless, per unit flux
 * through a horizontal unit area at the top (a vacuum under an overhead sun gives 1 in every cell, under mu0 the layer mean is
 * 1 / mu0).  The expectation of volumeAbsorption is sigma_abs * actinicFlux / 1000 (sigma_abs in 1/km).  meanActinicFlux(k) is
 * the sum over the columns of layer k divided by their number.  Such runs use the face-by-face walk, as level fluxes do, and
 * may be combined with them.  Solar sources only (mcbrat_compute_radiative_transfer fails with the thermal one); fails together
 * with intensity directions, scattering orders, a BRDF surface, event counters / photon fates, direct level fluxes, and where
 * one batch's level and actinic bins would not fit the tally budget -- whichever call comes first.  Changes
 * mcbrat_moments_length(): a caller-bound moment buffer must be bound again. */
int mcbrat_specify_actinic_flux(mcbrat_ctx *ctx, int32_t enable);
/* The LAST batch, Fortran order with the layer slowest: meanActinicFlux(nz), actinicFlux(nx, ny, nz).  Any pointer may be NULL. */
int mcbrat_report_actinic_flux(mcbrat_ctx *ctx, float *meanActinicFlux, float *actinicFlux);

/* The flux through the vertical faces of every cell (specifyParameters(recSideFluxes); an addition under ABI version 3; DESIGN.md
 * section 4.15).  Four quantities per cell, each (nx, ny, nz): sideFluxXPlus(x, y, k) is the weight that crossed the face
 * x = xPosition[x+1] of the patch (row y, layer k) -- the high-x face of cell (x, y, k); for x = nx-1 the periodic boundary --
 * towards +x, sideFluxXMinus the weight that crossed it towards -x; sideFluxYPlus / sideFluxYMinus the same for the face
 * y = yPosition[y+1].  A crossing adds the weight the photon carries on that leg, a periodic wrap is a crossing like any other,
 * and the patch of a crossing is that of the cell being left.  F_x = sum * dx_x / (photons per column * dz_k), F_y = sum * dy_y /
 * (photons per column * dz_k): the flux density through the vertical face per unit flux through a horizontal unit area at the
 * top (a vacuum under a sun at (mu0, phi0) gives F_x+ - F_x- = sqrt(1 - mu0^2) cos(phi0) / mu0 in every face).  The layer means
 * are the sum over the columns of layer k divided by their number.  A tally of the solar level-flux kernels: fails without
 * level fluxes (which cannot be switched off under it), with everything level fluxes fail with, with direct level fluxes and
 * the actinic flux, with the thermal source (mcbrat_compute_radiative_transfer), and where one batch's level and side bins
 * would not fit the tally budget -- whichever call comes first.  Changes mcbrat_moments_length(): a caller-bound moment buffer
 * must be bound again. */
int mcbrat_specify_side_fluxes(mcbrat_ctx *ctx, int32_t enable);
/* The LAST batch, Fortran order with the layer slowest, the four quantities in the order x plus, x minus, y plus, y minus:
 * meanSideFluxes(nz, 4), sideFluxes(nx, ny, nz, 4).  Either pointer may be NULL. */
int mcbrat_report_side_fluxes(mcbrat_ctx *ctx, float *meanSideFluxes, float *sideFluxes);

/* Whether the context could be brought to these settings (an addition under ABI version 3; no Fortran binding): NULL, or the
 * message with which one of mcbrat_specify_intensity, the five recording setters above and mcbrat_set_surface_brdf would refuse
 * them together -- a static string that lives as long as the library.  nDirections, limitIntensityContributions: as passed to
 * mcbrat_specify_intensity; numRecScatOrd: < 0 off; brdfSurface: nonzero for a surface of kind 1 to 3.  The grid, the component
 * count, the counters and the source are the context's.  Host arithmetic only: it changes nothing -- not mcbrat_last_error
 * either -- and does not synchronise.  A caller that changes several settings at once asks before it calls the first setter,
 * which refuse one at a time. */
const char *mcbrat_settings_refusal(const mcbrat_ctx *ctx, int32_t nDirections, int32_t limitIntensityContributions,
                                    int32_t numRecScatOrd, int32_t levelFluxes, int32_t directLevelFluxes,
                                    int32_t actinicFlux, int32_t sideFluxes, int32_t brdfSurface);

/* Batch moments: what the driver keeps in *Stats(...,1:2)
 * (monteCarloDriver.f95:603-616) and reduces with sumAcrossProcesses
 * (:1151-1166).  One double array:
 *   [0] total photons  [1] batches completed  [2..7] reserved
 *   then S1 = sum n*x and S2 = sum n*x^2, each of length mcbrat_moments_length():
 *   meanFluxUp, meanFluxDown, meanFluxAbsorbed, fluxUp[nx*ny], fluxDown[nx*ny],
 *   fluxAbsorbed[nx*ny], absorbedProfile[nz], absorbedVolume[nx*ny*nz],
 *   intensity[nDirections*nx*ny] (RadianceStats, monteCarloDriver.f95:1047-1050),
 *   and with scattering orders (N = numRecScatOrd): meanFluxUpByScatOrd[N+1], meanFluxDownByScatOrd[N+1],
 *   fluxUpByScatOrd[(N+1)*nx*ny], fluxDownByScatOrd[(N+1)*nx*ny], meanIntensityByScatOrd[(N+1)*nDirections],
 *   intensityByScatOrd[(N+1)*nDirections*nx*ny] (order slowest, x fastest),
 *   and with level fluxes, after everything else: meanLevelFluxUp[nz+1], meanLevelFluxDown[nz+1],
 *   levelFluxUp[(nz+1)*nx*ny], levelFluxDown[(nz+1)*nx*ny] (level slowest, x fastest),
 *   and with direct level fluxes, behind those: meanLevelFluxDownDirect[nz+1], meanLevelFluxDownDiffuse[nz+1],
 *   levelFluxDownDirect[(nz+1)*nx*ny], levelFluxDownDiffuse[(nz+1)*nx*ny],
 *   and with the actinic flux, behind every other tail: meanActinicFlux[nz], actinicFlux[nz*nx*ny] (layer slowest, x fastest),
 *   and with side fluxes, behind every other tail: meanSideFluxXPlus[nz], meanSideFluxXMinus[nz], meanSideFluxYPlus[nz],
 *   meanSideFluxYMinus[nz], then sideFluxXPlus, sideFluxXMinus, sideFluxYPlus, sideFluxYMinus, [nz*nx*ny] each (layer slowest).
 * Total doubles = 8 + 2*length.  The buffer is device memory; a caller that
 * wants to all-reduce it with RCCL binds its own device buffer. */
int64_t mcbrat_moments_length(const mcbrat_ctx *ctx);
int mcbrat_bind_moments(mcbrat_ctx *ctx, double *deviceBuffer); /* NULL: library-owned */
/* The device buffer the moments are accumulated in (library-owned unless one was bound).  Several contexts on one
 * grid -- one per wavelength of a spectrally integrated run, each with its optical properties resident -- accumulate
 * into ONE array when the others bind the first one's pointer (monteCarloDriver.f95:1023-1050 keeps one set of
 * *Stats arrays over all wavelengths).  Calls into contexts that share a buffer must not overlap (synchronous mode). */
double *mcbrat_moments_device_pointer(mcbrat_ctx *ctx);

/* getFrequencyDistr (src/emissionAndBroadBandWeights.f95:552-572, driver :438-449): the number of photons each of
 * numLambda wavelengths receives out of totalPhotons, one uniform per photon against the running power CDF
 * (findCDFIndex: smallest i with U <= CDF(i)).  The reference draws the uniforms from its MT stream in a host loop
 * over all photons; here draw d of the run is a Philox uniform keyed by `seed` (counter (0xFFFFFFFF, 0, d / 4),
 * element d % 4; d counts from firstDraw), drawn and counted on the device.  cdf and distribution are host arrays. */
int mcbrat_frequency_distribution(mcbrat_ctx *ctx, uint64_t seed, uint64_t firstDraw, int32_t numLambda, const double *cdf,
                                  int64_t totalPhotons, int64_t *distribution);
/* The device's Philox4x32-10 (the generator every kernel draws from), for its known-answer test: block i of n from
 * in[6 i .. 6 i + 5] = counter[4], key[2] into out[4 i .. 4 i + 3].  Host arrays; returns when out is written. */
int mcbrat_philox4x32_10(mcbrat_ctx *ctx, int32_t n, const uint32_t *in, uint32_t *out);
/* Device allocations the library holds at this moment, over every context of the process (a test aid, an addition under ABI
 * version 3): the difference around a context's whole life, or around a failed call, is 0. */
int64_t mcbrat_live_device_allocations(void);
int mcbrat_reset_moments(mcbrat_ctx *ctx); /* stream-ordered: enqueued before whatever the context does next; a caller
                                              that reads a bound buffer itself calls mcbrat_synchronize first */
int mcbrat_get_moments(mcbrat_ctx *ctx, double *hostBuffer);

/* Measurement: HIP-event duration of the tracing kernel(s) of the last
 * mcbrat_compute_radiative_transfer call, and its event counters (counters
 * are only collected when enabled; they cost a few percent). */
int mcbrat_enable_counters(mcbrat_ctx *ctx, int32_t enable);
int mcbrat_get_counters(mcbrat_ctx *ctx, mcbrat_counters *out); /* synchronises; badPhotons is valid whether or not counters are enabled */
/* What was dropped FIRST since the context was created (badPhotons > 0): which bound fired, in which kernel, the photon's id,
 * state and leg count -- one occurrence is then enough to trace that photon again alone and find the cause (computeRT only counts, :562-563).  An empty
 * string while nothing was dropped.  Synchronises; the text lives until the next call of this function on the context.  ABI 3. */
const char *mcbrat_first_drop(mcbrat_ctx *ctx);
float mcbrat_last_trace_ms(const mcbrat_ctx *ctx);
/* Asynchronous mode.  A launch ends with its longest photon history, so every call carries a fixed
 * drain time; a caller that issues many calls -- the reference's driver calls
 * computeRadiativeTransfer once per batch, monteCarloDriver.f95:1008 -- can let consecutive calls
 * overlap: with mcbrat_set_async(ctx, 1), mcbrat_compute_radiative_transfer and mcbrat_reset_moments
 * only enqueue work (on a small set of HIP streams owned by the context; per-batch results and
 * moments are still folded in call order, so results are bitwise the same as in synchronous mode)
 * and return.  Every call that reads results or replaces inputs (report_results, get_moments,
 * set_*, bind_moments, trace_fates, destroy) synchronises first; mcbrat_synchronize does so
 * explicitly, after which mcbrat_last_trace_ms is the summed tracing-kernel time of the calls since
 * the previous synchronisation. */
int mcbrat_set_async(mcbrat_ctx *ctx, int32_t enable);
int mcbrat_synchronize(mcbrat_ctx *ctx);
/* Stream interop for a caller that reduces the bound moment buffer on its own HIP stream (RCCL):
 * mcbrat_stream_wait_done makes `hipStream` (a hipStream_t) wait for everything enqueued so far;
 * mcbrat_wait_stream makes the context's next write to the moments wait for what `hipStream` has
 * enqueued so far.  Neither blocks the host. */
int mcbrat_stream_wait_done(mcbrat_ctx *ctx, void *hipStream);
int mcbrat_wait_stream(mcbrat_ctx *ctx, void *hipStream);
/* Several contexts that accumulate into ONE moment array (mcbrat_bind_moments with another context's
 * mcbrat_moments_device_pointer: one context per wavelength of a spectrally integrated run, monteCarloDriver.f95:889-1085) must
 * fold their batches one context after the other.  In synchronous mode the host does that by waiting for every call.  With
 * mcbrat_set_async on each of them, mcbrat_chain_after(ctx, previous) orders the device instead: the finish kernels (and the
 * reset) of ctx's NEXT call run after everything `previous` has enqueued so far, while the tracing kernels of the two contexts
 * overlap -- the tail of one wavelength's launch is filled by the next wavelength's photons.  Results are bitwise those of
 * synchronous calls in the same order.  Both contexts must live on the same device.  "So far" is fixed when this function is
 * called: ctx records an event of its OWN on `previous`'s stream and waits for that, so `previous` may be destroyed, or go on
 * to further calls, before ctx's next one. */
int mcbrat_chain_after(mcbrat_ctx *ctx, mcbrat_ctx *previous);
/* Tuning knobs (negative = leave unchanged): workgroups per CU (0 = occupancy query), number of
 * walking lanes below which a wave serves its waiting lanes (0 = choose by timing short trial
 * launches, the default), batches in flight per launch
 * (0 = memory bound), privateTallies (0 global atomics; 1 the library's plan: tallies private to a workgroup in LDS where the
 * slab fits beside a second workgroup, else the wide plan -- one workgroup of 1024 lanes per compute unit with up to its
 * whole 160 KB of LDS -- else global atomics; 2 private tallies without the optical grid in LDS; 3 as 1 without the wide plan;
 * 4 the wide plan even where the shared one would do; 5 as 4 with the per-cell optics left in global memory; 6 as 4 without
 * the per-cell optics in LDS -- per block in LDS where every block is uniform in them, else as 5),
 * workgroup size (0 = automatic, 256, 512, 768; a fixed size rules the wide plan out), and how
 * many idle / surface lanes queue up before launches / surface reflections are served; brickLayout:
 * 0 dense optical grids, 1 4x4x4 bricks with unstored background bricks, 2 automatic (default). */
int mcbrat_set_tuning(mcbrat_ctx *ctx, int32_t blocksPerCU, int32_t eventThreshold, int32_t maxBatchesInFlight,
                      int32_t privateTallies, int32_t blockSize, int32_t launchThreshold, int32_t surfaceThreshold,
                      int32_t brickLayout);

/* Scheduling options by name (none of them changes a result: the same photons, the same arithmetic per photon, integer
 * tallies -- tests/test_gpu_tunings.py holds random choices against the defaults bit for bit).  ABI 3.
 *   "jumpThreshold", "crossThreshold"  lanes queued before transitions of the layer-skipping walk / block crossings are served
 *   "batchUnits"  1: the block walk cuts its workgroups' work units inside batches, as the flat walk does (default 0: units
 *                 across the launch, two batches' tallies per workgroup where they fit; environment MCBRAT_BATCH_UNITS)
 *   "blockSpanKernel"  1: the block walk keeps its general instantiation where the one without periodic folds inside blocks
 *                 would do (default 0: automatic; both trace every photon bit for bit alike -- tests/test_gpu_blockwalk_nospan.py)
 *   "blockRareKernel"  1: the block walk keeps its general exit and launch phases where the instantiation with a black surface
 *                 and the parallel sun compiled in would do (default 0: automatic; both trace every photon bit for bit alike --
 *                 tests/test_gpu_blockwalk_rare.py)
 *   "cameraGridInLds"  where mcbrat_sun_transmittance reads the grid: -1 (default) LDS where it fits, 0 global memory, 1 LDS
 *   "cameraPathBinsInLds"  0: mcbrat_render_camera_pathlengths adds every estimate straight to global memory (default 1: a
 *                 histogram per wave in LDS; integer sums, the same bytes either way)
 * One option does change results, within their noise -- it chooses between two unbiased estimators:
 *   "glintSampling"  1 (default): a reflection off a Cox-Munk patch draws its direction from the mixture of the glint lobe and
 *                 the Lambertian draw (mcbrat_set_surface_brdf); 0: the Lambertian draw times R, as the land models
 * The reference has no counterpart (its loop is one photon at a time, monteCarloRadiativeTransfer.f95:463-466). */
int mcbrat_set_option(mcbrat_ctx *ctx, const char *name, int32_t value);

/* specifyParameters(surfaceBDRF = new_SurfaceDescription(surfaceParameters, xPosition, yPosition))
 * (Integrators/monteCarloRadiativeTransfer.f95:1173-1176, src/surfaceProperties.f95:58-94): a reflecting surface whose
 * Lambertian reflectance varies from patch to patch on its own horizontal positions (numX x-positions bound numX-1
 * patches; `reflectance` is BRDFParameters(1, :, :), x fastest).  A photon that reaches the surface is multiplied by
 * the reflectance of the patch under it (computeSurfaceReflectance :119-147) instead of the domain's albedo
 * (computeRT :667-673).  The uniform surface of newSurfaceUniform is numX = numY = 2 with positions (0, huge(1.)).
 * numX <= 0 returns to the domain's albedo.  Error texts are the reference's. */
int mcbrat_set_surface_description(mcbrat_ctx *ctx, int32_t numX, int32_t numY, const double *xPosition,
                                   const double *yPosition, const float *reflectance);

/* A surface BRDF per patch (the reference's template, src/surfaceProperties.f95:8-14, with
 * numberOfParameters > 1).  kind 0 Lambertian {a} (what mcbrat_set_surface_description sets), 1 RPV {rho0, k, Theta, rhoC},
 * 2 Ross-Li (RossThick + LiSparse-Reciprocal) {fIso, fVol, fGeo}, 3 Cox-Munk (the ocean: isotropic wave slopes, Fresnel
 * reflection, shadowing, whitecaps) {U wind speed at 10 m in m/s, n refractive index, rhoWc whitecap reflectance, aW
 * water-leaving albedo}; `params` is BRDFParameters(nParams, numX-1, numY-1), x fastest, nParams 1 / 4 / 3 / 4.
 * A reflected photon keeps the Lambertian (cosine-weighted) draw of its direction and its weight is multiplied by the
 * reflectance factor R = pi f of the patch for its arriving and leaving directions; the local estimates of radiance from a
 * reflection use R / pi.  A Cox-Munk patch draws the direction from a one-sample mixture of its glint lobe and the
 * Lambertian draw instead (balance heuristic; option "glintSampling"), which keeps the reflected weight below about 1.1
 * where the Lambertian draw times R reaches thousands at low sun; a sampled direction whose cosine is below 2^-16, the
 * smallest the Lambertian draw gives, ends the photon.
 * Refused: parameters outside RPV's 0 <= rho0 <= 1, 0.2 <= k <= 2, |Theta| <= 0.95, 0 <= rhoC <= 1, negative Ross-Li
 * weights, Cox-Munk parameters outside 0 <= U <= 50, 1 <= n <= 2, 0 <= rhoWc <= 1, 0 <= aW <= 1, and a patch whose
 * directional-hemispherical albedo exceeds 1 + 1e-3 at mu_i = 0.1, 0.2, .., 1.  A non-Lambertian surface is refused
 * together with the thermal source, event counters and photon fates (at computeRadiativeTransfer).  Over it fluxUp, like
 * fluxDown, is not bounded by the capacity rule of mcbrat_compute_radiative_transfer (a reflected weight may exceed 1).
 * numX <= 0 returns to the domain's albedo. */
int mcbrat_set_surface_brdf(mcbrat_ctx *ctx, int32_t kind, int32_t numX, int32_t numY, const double *xPosition,
                            const double *yPosition, int32_t nParams, const float *params);

/* The BRDF evaluator on the host (no context, no GPU): the reflectance factor R = pi f of one patch's parameters for the
 * propagation directions dIn (arriving, dIn[2] < 0) and dOut (leaving, dOut[2] > 0), unit vectors; NaN for an unknown kind. */
float mcbrat_brdf_reflectance(int32_t kind, const float *params, const double *dIn, const double *dOut);

/* Directional-hemispherical albedo rho_dh(muIn) = (1/pi) int R mu_r dOmega (black-sky albedo at incidence cosine muIn),
 * by Gauss quadrature; NaN for an unknown kind or muIn outside (0, 1]. */
double mcbrat_brdf_albedo(int32_t kind, const float *params, double muIn);

/* The reflection's sampler on the host (no context, no GPU): the function the tracing kernel calls at a BRDF reflection.
 * For the arriving direction dIn and n triples of uniforms u[n][3] = {component, u1, u2}: the leaving directions dOut[n][3]
 * and the factors weight[n] the photon's weight is multiplied by (0: the photon ends).  The Lambertian draw -- all there is
 * for kinds 0 to 2, one of the two components for Cox-Munk -- is mu = sqrt(u1), azimuth 2 pi u2, formed in double.  Unlike
 * the kernel, where the Lambertian draw comes from the leg's Philox block and (u1, u2) of the glint component from a block
 * of their own, both components read the one pair here; a draw uses one component only, so the estimate is the same.
 * The mean of `weight` estimates mcbrat_brdf_albedo(-dIn[2]).  Returns 0, or 1 for a null argument, a negative n or an
 * unknown kind. */
int mcbrat_brdf_sample(int32_t kind, const float *params, const double *dIn, int64_t n, const double *u, double *dOut,
                       float *weight);

/* ---- backward Monte Carlo camera (an addition under ABI version 3) -------------------------------------
 * Radiance at a sensor anywhere in the domain, per pixel: paths start at the sensor and walk BACKWARD; every collision and
 * every surface reflection takes a local estimate toward the sun.  Units: radiance per unit solar flux through a horizontal
 * plane at the top, as `intensity` (a vacuum over a Lambertian albedo a gives a / pi).  Needs the grid, the optics, the inverse
 * and the forward tables (mcbrat_set_forward_table; of a hybrid pair the original ones) and the Directional solar source
 * (mcbrat_set_source_solar); the surface is Lambertian -- the domain's albedo or mcbrat_set_surface_description. */
typedef struct mcbrat_camera {
  int32_t kind;          /* 0 orthographic, 1 pinhole */
  int32_t npx, npy;
  int32_t jitter;        /* 1: samples uniform in the pixel; 0: every sample at the pixel centre */
  int32_t gridInLds;     /* -1 library's choice, 0, 1: the extinction grid and the edges staged in LDS (1 is refused where they do not fit) */
  /* orthographic: the light arriving travels along (mu, phiDeg) -- the convention of intensityMus / intensityPhis;
     pixel (i, j) is the footprint cell of [xLo, xHi] x [yLo, yHi] cut npx x npy, at height z (z0 <= z <= zMax) */
  float mu, phiDeg;
  double xLo, xHi, yLo, yHi, z;
  /* pinhole: position (folded periodically in x, y; z0 <= z <= zMax), look and up vectors (need not be normalised,
     not parallel), full horizontal field of view in degrees (0 < fov < 180) */
  double position[3], look[3], up[3];
  float fovXDeg;
} mcbrat_camera;

/* numBatches batches of samplesPerPixel paths per pixel.  Sample k of batch b of a pixel has the index firstSample +
 * b * samplesPerPixel + k; its random numbers are Philox4x32-10(key = seed, counter = (event | block << 24, pixel, index)), and
 * the tallies are 64-bit integers, so the result of a (pixel, sample range) depends on nothing else -- not on scheduling, not
 * on gridInLds, not on what else the call renders.  radiance[npy][npx] (x fastest; j grows upward for the pinhole) is the mean
 * of the batch means, radianceStdErr its standard error (0 where numBatches == 1), batchMeans[numBatches][npy][npx] the means
 * themselves; *dropped counts the paths a loop bound ended (section 4.7; they contribute nothing).  Any of the last three may
 * be NULL.  The call waits for what the context has in flight, works on device buffers of its own and leaves the context's
 * settings, tallies, moments and walk mode as they were.
 * Refused, before any launch: no grid / optics / inverse or forward tables; a source other than the Directional solar one; a
 * BRDF surface (mcbrat_set_surface_brdf kinds 1 to 3); mu == 0, z or position[2] outside [z0, zMax], a degenerate footprint,
 * look parallel to up, a field of view outside (0, 180); more bins (npx * npy * numBatches) than the 4 GiB tally budget holds;
 * samplesPerPixel < 1 or numBatches < 1. */
int mcbrat_render_camera(mcbrat_ctx *ctx, const mcbrat_camera *cam, uint64_t seed, uint64_t firstSample,
                         int64_t samplesPerPixel /* per batch */, int32_t numBatches,
                         float *radiance /* [npy][npx] mean of the batch means */,
                         float *radianceStdErr /* [npy][npx], may be NULL; 0 where numBatches == 1 */,
                         float *batchMeans /* [numBatches][npy][npx], may be NULL */,
                         int64_t *dropped /* may be NULL */);
/* The mapping the kernel uses, on the host (no context): origin and backward direction (unit vector) of the position (i + u,
 * j + v) of the image, 0 <= u, v <= 1.  The origin is not folded into the domain.  Non-zero for a camera that
 * mcbrat_render_camera refuses on its own members. */
int mcbrat_camera_ray(const mcbrat_camera *cam, int32_t i, int32_t j, double u, double v,
                      double origin[3], double direction[3]);
/* exp(-optical depth) from each of n points (x, y, z; x and y folded periodically, z0 <= z <= zMax) against the sun's direction
 * of travel to the top of the domain: the direct transmittance / cloud shadow at a point, without noise -- the camera kernel's
 * own device function.  Needs grid, optics and the Directional solar source.  Option "cameraGridInLds" (mcbrat_set_option: -1
 * library's choice, 0, 1) chooses where it reads the grid; the results are the same bit for bit. */
int mcbrat_sun_transmittance(mcbrat_ctx *ctx, int64_t n, const double *xyz /* [n][3] */, float *transmittance /* [n] */);

/* ---- backward sensors (an addition under ABI version 3) --------------------------------------------------
 * Irradiance on a plane and actinic flux at a point, anywhere in the domain: the camera's backward paths, started on a receiver
 * with a cosine-weighted (planar) or a uniform (spherical) direction.  Units: per unit solar flux through a horizontal plane at
 * the top -- a horizontal planar sensor measures what levelFluxDown / levelFluxUp average over a column's face, a spherical one
 * what actinicFlux averages over a cell (1 / mu0 in a vacuum over a black surface).  Needs what mcbrat_render_camera needs. */
typedef struct mcbrat_sensor {
  int32_t kind;        /* 0 planar (cosine response on the side the normal points to), 1 spherical (uniform response) */
  uint32_t id;         /* stands where the camera's pixel stands in the Philox counter: the sensor's random numbers */
  double position[3];  /* x and y are folded periodically; z0 <= z <= zMax for every corner of the receiver */
  double e1[3], e2[3]; /* the receiver is position + u e1 + v e2, 0 <= u, v <= 1; both zero: a point */
  double normal[3];    /* planar: the side that receives light; need not be normalised; perpendicular to e1 and e2.  Spherical: ignored */
} mcbrat_sensor;

/* numBatches batches of samplesPerSensor paths per sensor.  Sample k of batch b has the index firstSample + b * samplesPerSensor
 * + k; its random numbers are Philox4x32-10(key = seed, counter = (event | block << 24, id, index)): event 0, block 0 is
 * [u, v, a, c] of mcbrat_sensor_ray, events >= 1 are the camera's.  Every path adds its sum of local estimates S to the sensor's
 * diffuse bin and T_sun(origin) c to its direct bin, c = max(0, n . s) / mu0 (planar; s the unit vector toward the sun) or
 * 1 / mu0 (spherical); where c = 0 no sun ray is walked.  diffuse[n] = w0 mean(S) with w0 = pi (planar) or 4 pi (spherical),
 * direct[n] = mean(T_sun c); the irradiance (the actinic flux) is their sum.  Tallies are 64-bit integers, so the result of an
 * (id, geometry, seed, sample range) depends on nothing else -- not on scheduling, not on gridInLds, not on the other sensors
 * of the call.  The three standard errors are those of the mean of the batch means (0 where numBatches == 1; the direct part
 * of a point sensor: exactly 0), totalStdErr that of the per-batch sums diffuse + direct.  batchMeans[b][0][i] is batch b's
 * diffuse mean of sensor i, batchMeans[b][1][i] its direct mean.  *dropped counts the paths a loop bound ended; they contribute
 * to neither part.  The optional outputs may be NULL.  The context's settings, tallies, moments and walk mode stay as they were.
 * Refused, before any launch: n < 1; a kind other than 0 or 1; a member that is not finite; a planar sensor with a zero normal
 * or an edge that is not perpendicular to its normal (|e . n| > 1e-6 |e|); a corner of a receiver outside [z0, zMax];
 * samplesPerSensor < 1 or numBatches < 1; 2 n numBatches bins beyond the 4 GiB tally budget; gridInLds outside -1, 0, 1, or 1
 * where the grid does not fit; and what mcbrat_render_camera refuses about the context. */
int mcbrat_render_sensors(mcbrat_ctx *ctx, int64_t n, const mcbrat_sensor *sensors, uint64_t seed, uint64_t firstSample,
                          int64_t samplesPerSensor /* per batch */, int32_t numBatches,
                          int32_t gridInLds /* -1 library's choice, 0, 1 */,
                          float *diffuse /* [n] */, float *direct /* [n] */,
                          float *diffuseStdErr /* [n], may be NULL */, float *directStdErr /* [n], may be NULL */,
                          float *totalStdErr /* [n], may be NULL */,
                          float *batchMeans /* [numBatches][2][n], may be NULL */, int64_t *dropped /* may be NULL */);
/* The mapping the kernel uses, on the host (no context; csrc/mcbrat_sensor_ray.h): origin (not folded into the domain) and
 * backward direction (unit vector) of the draws u, v, a, c in [0, 1].  Non-zero for a sensor that mcbrat_render_sensors
 * refuses on its own members. */
int mcbrat_sensor_ray(const mcbrat_sensor *sensor, double u, double v, double a, double c, double origin[3], double direction[3]);

/* ---- emission renders: the backward thermal camera and sensors (additions under ABI version 3) ---------
 * The radiance a medium and its surface EMIT, by the camera's and the sensors' backward paths: same (origin, direction), same
 * Philox counters, same bounds; no ray toward the sun, no forward table.  A collision in cell v, component c adds
 * w (1 - omega0[c, v]) cellSource[v] and then takes w *= omega0; the surface at (x, y) adds w (1 - a(x, y)) surfaceSource[column]
 * and then takes w *= a; at the top the path ends.  cellSource[nz][ny][nx] (x fastest) and surfaceSource[ny][nx] are the caller's
 * Planck radiances in the caller's units (mcbrat_planck_radiance: W m-2 sr-1 um-1); results are in the same units.  1 - omega0
 * and 1 - a come from the optics and the Lambertian surface the context holds; its SOURCE is not consulted -- a thermal context,
 * a solar one and one with no source set render the same bytes.  Needs the grid, the optics and the inverse tables (no forward
 * tables).  Outputs, batches, sample indices, determinism and `dropped` are those of mcbrat_render_camera and
 * mcbrat_render_sensors; a sensor has no direct part: irradiance[i] = w0 mean(S), batchMeans[numBatches][n].
 * Refused, before any launch: what the solar entries refuse about the camera, the sensors, the counts, the budget (one bin
 * array), grid, optics, inverse tables and gridInLds; a BRDF surface (its emissivity is directional); a null source array; a
 * source value that is negative or not finite; sources that are all zero (nothing emits). */
int mcbrat_render_camera_emission(mcbrat_ctx *ctx, const mcbrat_camera *cam, const float *cellSource /* [nz][ny][nx] */,
                                  const float *surfaceSource /* [ny][nx] */, uint64_t seed, uint64_t firstSample,
                                  int64_t samplesPerPixel /* per batch */, int32_t numBatches,
                                  float *radiance /* [npy][npx] */, float *radianceStdErr /* may be NULL */,
                                  float *batchMeans /* [numBatches][npy][npx], may be NULL */, int64_t *dropped /* may be NULL */);
int mcbrat_render_sensors_emission(mcbrat_ctx *ctx, int64_t n, const mcbrat_sensor *sensors, const float *cellSource,
                                   const float *surfaceSource, uint64_t seed, uint64_t firstSample,
                                   int64_t samplesPerSensor /* per batch */, int32_t numBatches,
                                   int32_t gridInLds /* -1 library's choice, 0, 1 */,
                                   float *irradiance /* [n] */, float *irradianceStdErr /* [n], may be NULL */,
                                   float *batchMeans /* [numBatches][n], may be NULL */, int64_t *dropped /* may be NULL */);
/* The emission renders with the expected-value (track-length) estimator (additions under ABI version 3).
 * Arguments, checks, refusals (worded under the entries' own names), outputs and units are those of mcbrat_render_camera_emission
 * and mcbrat_render_sensors_emission.  The same (seed, sample range) walks the collision estimator's paths: the same origins,
 * directions, Philox counters, leg lengths, collision points, components, weights, roulette and reflections.  Only the deposits
 * differ.  Collisions and surface hits deposit nothing; every leg, with the weight w it starts with, deposits the formal
 * solution along its whole ray, on past its collision point up to the domain's boundary:
 *     w sum over the cells v crossed  E[v] e^(-tau_in) (1 - e^(-dtau))   +   w e^(-tau_sfc) (1 - a(x, y)) surfaceSource[column]
 * with tau counted from the leg's origin, the second term where the ray meets the surface (nothing at the top), and
 * E[v] = cellSource[v] sum_c f_c(v) (1 - omega0[c, v]), f_c the extinction share of component c (0 where the extinction is 0).
 * The two estimators have the same mean; a medium that does not scatter is rendered without variance.  A ray stops adding
 * behind optical depth 30: what is left is below e^(-30) < 2^-43 of the largest source value, an eighth of the finest step of
 * the tally.  A path's sum is not bounded by the largest source value; a path whose sum reaches the tally's saturation value is
 * dropped and counted in `dropped`, as is one whose ray a loop bound ends -- the RAY, which goes on past the leg's collision
 * point: for the same seed `dropped` may be larger than the collision estimator's, whose leg ended inside the bound (a nearly
 * horizontal leg through a near-vacuum).  gridInLds = 1 asks for the extinction grid AND E[v]
 * in LDS (8 bytes per cell) and is refused where the pair does not fit; -1 then renders from global memory. */
int mcbrat_render_camera_emission_expected(mcbrat_ctx *ctx, const mcbrat_camera *cam, const float *cellSource /* [nz][ny][nx] */,
                                           const float *surfaceSource /* [ny][nx] */, uint64_t seed, uint64_t firstSample,
                                           int64_t samplesPerPixel /* per batch */, int32_t numBatches,
                                           float *radiance /* [npy][npx] */, float *radianceStdErr /* may be NULL */,
                                           float *batchMeans /* [numBatches][npy][npx], may be NULL */, int64_t *dropped /* may be NULL */);
int mcbrat_render_sensors_emission_expected(mcbrat_ctx *ctx, int64_t n, const mcbrat_sensor *sensors, const float *cellSource,
                                            const float *surfaceSource, uint64_t seed, uint64_t firstSample,
                                            int64_t samplesPerSensor /* per batch */, int32_t numBatches,
                                            int32_t gridInLds /* -1 library's choice, 0, 1 */,
                                            float *irradiance /* [n] */, float *irradianceStdErr /* [n], may be NULL */,
                                            float *batchMeans /* [numBatches][n], may be NULL */, int64_t *dropped /* may be NULL */);
/* The Planck function exactly as mcbrat_emission_weighting evaluates it (one function serves both): out[i] = B(lambda, temps[i])
 * in W m-2 sr-1 um-1, so that forward `intensity` x totalFlux / dLambda and the emission camera's radiance on these sources are
 * one quantity.  Host arithmetic only.  Returns 1 for a null array, a negative n or a wavelength that is not positive. */
int mcbrat_planck_radiance(double lambdaMicrons, int64_t n, const double *temps, double *out);

/* ---- the radiance by photon path length (an addition under ABI version 3) ---------------------------------
 * mcbrat_render_camera's radiance split by how far the light travelled inside the domain: the same camera, sample indices,
 * Philox counters, batches and statistics -- the same (seed, sample range) walks the same paths --, every local estimate tallied
 * on its own in the bin of its path length L = sum of the backward legs walked up to the event + (zMax - z_event) / mu0, the
 * geometric length (in the domain's length unit) from where the light enters at zMax to the camera.  Bins are given by numBins
 * LOWER edges, floats: pathEdges[0] = 0, strictly ascending, finite; bin b holds pathEdges[b] <= L < pathEdges[b + 1], the last
 * bin is open above, so the bins of a pixel sum to its radiance (to the rounding of a per-estimate fixed point against
 * mcbrat_render_camera's per-path one).  1 <= numBins <= 256.  The sums are integers: an image is bitwise independent of
 * scheduling and of gridInLds.  By the equivalence theorem, sum_b I_b exp(-k L_b) is the radiance under a uniform absorber k.
 * `dropped` counts the paths a bound ended or that produced a NaN estimate; unlike mcbrat_render_camera's, such a path keeps
 * what it had deposited before.  Option "cameraPathBinsInLds" (mcbrat_set_option: 1 default, 0 every deposit straight to global
 * memory -- the same integers, a measurement of what the histograms in LDS buy).
 * Refused, before any launch, with texts that begin "renderCameraPathLengths:": a null array; what mcbrat_render_camera refuses
 * about the camera's own members; numBins outside [1, 256]; edges that are not finite, do not begin at 0 or do not ascend; then
 * everything mcbrat_render_camera refuses, in its order (the budget counts npx * npy * numBins * numBatches sums); gridInLds = 1
 * where the grid fits the LDS share alone but not with the histograms (-1 then renders from global memory). */
int mcbrat_render_camera_pathlengths(mcbrat_ctx *ctx, const mcbrat_camera *cam, int32_t numBins, const float *pathEdges /* [numBins] */,
                                     uint64_t seed, uint64_t firstSample, int64_t samplesPerPixel /* per batch */, int32_t numBatches,
                                     float *radiance /* [numBins][npy][npx] */, float *radianceStdErr /* same shape, may be NULL */,
                                     float *batchMeans /* [numBatches][numBins][npy][npx], may be NULL */, int64_t *dropped /* may be NULL */);

/* Walk options (negative = leave unchanged).
 * layerSkip (default 1): inside a horizontal layer whose cells all carry one extinction value -- the clear air
 * above and below a cloud field -- a photon crosses z faces only; its column is found again from its position when
 * it collides, leaves the domain or reaches a layer with cell-to-cell extinction.  The reference's
 * accumulateExtinctionAlongPath (src/opticalProperties.f95:1697-1814) stops at every x and y face too, which changes
 * nothing inside such a layer but the float rounding of the accumulated optical depth; 0 restores that face-by-face
 * walk (used by the per-photon identity tests).
 * With layerSkip = 1 the same idea is applied inside the other layers too (the clear-air flight): columns are grouped
 * 4 x 4 into brick columns; outside the layers in which a brick column holds a cell that differs from its layer's most
 * common ("background") extinction, a photon whose remaining optical depth cannot be used up by the background
 * between its height and the domain boundary steps from brick column to brick column, and takes its optical depth
 * from the background's vertical optical depth when that flight ends (at a cloud, or at the domain boundary).  Grids
 * whose column counts are multiples of four, at most 255 layers, fluxes only, and a background whose vertical optical
 * depth is at most 0.5 (in a haze most flights would be refused, and asking costs a turn in a queue).  layerSkip = 2:
 * the one-extinction layers only, no flight; 3: flights whatever the optical depth of the background (tests).
 * blockWalk (default 1): domains whose optical grid is resident in LDS (I3RC step cloud, plane-parallel and other
 * small domains): the grid is cut into axis-aligned blocks of cells that carry one extinction value, and a leg goes
 * from block face to block face instead of from cell face to cell face; the cell of a collision or an exit is found
 * from the position.  Same argument as for layerSkip: inside a block the reference's stops at cell faces only add
 * `segment x the same extinction` again.  0 restores the face-by-face walk; 2 uses the block walk even where blocks
 * hold fewer than four cells on average (a medium that differs from cell to cell: slower, meant for tests). */
int mcbrat_set_walk_options(mcbrat_ctx *ctx, int32_t layerSkip, int32_t blockWalk);
/* The walk a flux run of the loaded grid and optics uses, decided by the same plan as the launch itself: bit 0
 * layerSkip, bit 1 the block walk (asked for AND applicable: grid, tallies and tables fit in LDS, blocks hold four
 * cells or more on average, no radiance directions), bit 2 the clear-air flight (asked for and possible: brick columns
 * exist, the background is thin enough or layerSkip = 3, no radiance directions, the grid is not held in LDS and the
 * flight's tables fit beside the rest), bit 3 the blockWalk option as set, bit 6 tallies private to a workgroup in LDS,
 * bit 4 the wide plan (a tally slab too large to share a compute unit's LDS: one workgroup of 1024 lanes per compute unit
 * owns up to its whole 160 KB), bit 5 the block walk with the per-cell optics left in global memory (extinction per block
 * in LDS), bit 7 the block walk with the optics per BLOCK in LDS (every block uniform in them), bit 8 the thermal source's level
 * and row sums of the emission CDF staged in LDS, bit 9 (512) the block walk's instantiation with the periodic folds inside blocks
 * compiled out (no block of the medium spans a whole periodic axis, solar source, equally spaced axes, one component, the
 * domain's albedo, 768-lane workgroups, option "blockSpanKernel" not set), bit 10 (1024) that instantiation with a black surface
 * and the parallel sun compiled into its exit and launch phases (bit 9, and: the albedo compares equal to 0, no surface
 * description, every single-scattering albedo handed over is finite, the Directional solar source, option "blockRareKernel" not
 * set).  Before grid and optics are loaded: the options. */
int mcbrat_get_walk_mode(const mcbrat_ctx *ctx);

/* The event threshold in use (after the first call of a domain: the one chosen by the trial launches). */
int mcbrat_get_event_threshold(const mcbrat_ctx *ctx);

/* Parity/debug: trace n photons (ids firstPhotonId..) and record what became
 * of each one.  Tallies and moments of the context are left untouched. */
int mcbrat_trace_fates(mcbrat_ctx *ctx, uint64_t seed, uint64_t firstPhotonId, int64_t n,
                       mcbrat_fate *fates);

/* ---- host-side set-up routines on the path (no GPU needed) ------------- */
/* computeInversePhaseFunction (src/inversePhaseFunctions.f95:66-174) for a
 * phase function stored as Legendre coefficients chi_1..chi_n (P0 = 1 implied). */
int mcbrat_inverse_table_legendre(int32_t nCoefficients, const float *coefficients,
                                  int32_t nSteps, float *table);
/* ...and for one stored as (scatteringAngle, value) pairs; values are
 * normalised as new_PhaseFunction does (scatteringPhaseFunctions.f95:156). */
int mcbrat_inverse_table_tabulated(int32_t nAngles, const float *scatteringAngle,
                                   const float *value, int32_t nSteps, float *table);
/* tabulateForwardPhaseFunctions for one phase function (opticalProperties.f95:1914-1916 ->
 * getPhaseFunctionValues, scatteringPhaseFunctions.f95:480-527): values at nAngles angles equally
 * spaced on [0, pi], from Legendre coefficients or from (angle, value) pairs. */
int mcbrat_forward_table_legendre(int32_t nCoefficients, const float *coefficients, int32_t nAngles,
                                  float *table);
int mcbrat_forward_table_tabulated(int32_t nStored, const float *scatteringAngle, const float *value,
                                   int32_t nAngles, float *table);
/* computeHybridPhaseFunctions (opticalProperties.f95:1937-2009) on values[nEntries][nAngles]. */
int mcbrat_hybrid_phase_functions(int32_t nAngles, int32_t nEntries, const float *values,
                                  float gaussianWidthDeg, float *hybridValues);
/* The decomposition the block walk uses (mcbrat_set_walk_options, blockWalk): axis-aligned boxes of cells with one
 * extinction value, found greedily (x, then y, then z).  extinction[nx*ny*nz] (x fastest, as the kernels hold it:
 * float); blockOf[nx*ny*nz]: the block of each cell; blockRec[4*nBlocks] (room for 4*nx*ny*nz): per block
 * {x0 | x1 << 16, y0 | y1 << 16, z0 | z1 << 16, flags}, cell range [lo, hi) per axis, flag bit 0 / 1 = the block
 * spans the whole periodic x / y axis.  Host arithmetic only.  Returns 1 for more than 65535 blocks / cells per axis. */
int mcbrat_block_decomposition(int32_t nx, int32_t ny, int32_t nz, const float *extinction, uint16_t *blockOf,
                               uint32_t *blockRec, int32_t *nBlocks);
/* The tables of the layer-skipping walk and the clear-air flight (mcbrat_set_walk_options, layerSkip), as the library
 * builds them when the optics are set.  extinction[nx*ny*nz] (x fastest, float), zEdges[nz+1].  background[nz]: the
 * most common extinction of every layer; range[(ny/4)*(nx/4)]: per brick column of 4 x 4 columns lo | hi << 8, the
 * layers [lo, hi) that hold a cell differing from its layer's background (lo = nz, hi = 0: none); walk[nx*ny*nz]: the
 * extinction with the sign bit set in every cell outside the range of its brick column; depth[nz+1]: vertical optical
 * depth of the background below every face, over the layers a flight can cross; *flights: 1 when brick columns exist
 * (nx, ny multiples of four, 2..255 layers) and some range is not empty.  range / walk are written only when brick
 * columns exist.  Host arithmetic only. */
int mcbrat_flight_tables(int32_t nx, int32_t ny, int32_t nz, const float *extinction, const double *zEdges,
                         float *background, uint16_t *range, float *walk, double *depth, int32_t *flights);

/* emission_weighting (src/emissionAndBroadBandWeights.f95:424-550): builds
 * voxelWeights (running CDF, x fastest), fracAtmsPower and the emitted flux. */
int mcbrat_emission_weighting(int32_t nx, int32_t ny, int32_t nz, int32_t nComponents,
                              const double *xEdges, const double *yEdges, const double *zEdges,
                              const double *temps, const double *totalExt, const double *cumExt,
                              const double *ssa, double surfaceAlbedo, double lambdaMicrons,
                              double surfaceTemp, double dLambda, double *voxelWeights,
                              double *fracAtmsPower, double *totalFlux);

#ifdef __cplusplus
}
#endif
#endif
