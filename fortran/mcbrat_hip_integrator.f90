! mcbrat_hip_integrator.f90 -- ISO_C_BINDING shim over include/mcbrat.h.
!
! Stands where Integrators/monteCarloRadiativeTransfer.f95 stands: the same public names
! (integrator, new_Integrator, specifyParameters, computeRadiativeTransfer, reportResults,
! finalize_Integrator; reference public list :121-123), with the photon loop computeRT
! (:393-841) running in the HIP library.  The domain is handed over as the raw arrays that
! computeRT itself pulls out of type(domain) with getInfo_Domain (:434-443); INTEGRATION.md
! shows the three-line wrapper that does that inside the reference tree.
!
! Status convention: each routine returns `ierr` (0 = success) and leaves the text in
! lastMessage(); the in-tree wrapper maps it to setStateToFailure / setStateToCompleteSuccess.
module mcbrat_hip_integrator
  use, intrinsic :: iso_c_binding
  implicit none
  private

  type integrator
    private
    type(c_ptr) :: ctx = c_null_ptr
    integer     :: numX = 0, numY = 0, numZ = 0
    integer     :: numRecScatOrd = -1   ! highest scattering order recorded, -1 off (specifyScatteringOrders)
    logical     :: readyToCompute = .false.
  end type integrator

  public :: integrator, new_Integrator, isReady_Integrator, finalize_Integrator, &
            setOpticalProperties, setInverseTable, setSolarSource, setEmissionSource, &
            setRandomAzimuthSource, setFluxSource, setSpotlightSource, &
            specifyParameters, computeRadiativeTransfer, reportResults, &
            resetMoments, getMoments, momentsLength, lastMessage, &
            inverseTableLegendre, lastTraceMilliseconds, setAsynchronous, synchronize, &
            specifyIntensity, setForwardTable, reportIntensity, forwardTableLegendre, &
            setSurfaceDescription, setSurfaceBRDF, setWalkOptions, setOption, getFrequencyDistr, shareMoments, chainAfter, numBadPhotons, &
            specifyScatteringOrders, reportResultsByScatOrd, specifyLevelFluxes, reportLevelFluxes, &
            specifyDirectLevelFluxes, reportDirectLevelFluxes, specifyActinicFlux, reportActinicFlux, &
            specifySideFluxes, reportSideFluxes, &
            camera, renderCamera, sunTransmittance, &
            sensor, renderSensors, &
            renderCameraEmission, renderSensorsEmission, renderCameraEmissionExpected, renderSensorsEmissionExpected, &
            renderCameraPathLengths

  ! mcbrat_camera of include/mcbrat.h, member for member (the backward camera, DESIGN.md section 4.19): kind 0 orthographic --
  ! mu, phiDeg, the footprint xLo .. yHi and the height z -- or 1 pinhole -- position, look, up, fovXDeg
  type, bind(C) :: camera
    integer(c_int32_t) :: kind = 0, npx = 1, npy = 1, jitter = 1, gridInLds = -1
    real(c_float)      :: mu = 1., phiDeg = 0.
    real(c_double)     :: xLo = 0., xHi = 1., yLo = 0., yHi = 1., z = 0.
    real(c_double)     :: position(3) = 0., look(3) = (/ 0._c_double, 0._c_double, -1._c_double /), &
                          up(3) = (/ 0._c_double, 1._c_double, 0._c_double /)
    real(c_float)      :: fovXDeg = 60.
  end type camera

  ! mcbrat_sensor of include/mcbrat.h, member for member (the backward sensors, DESIGN.md section 4.20): kind 0 planar -- a cosine
  ! response on the side `normal` points to -- or 1 spherical; id keys the sensor's random numbers (an unsigned 32-bit word);
  ! the receiver is position + u e1 + v e2 (both zero: a point)
  type, bind(C) :: sensor
    integer(c_int32_t) :: kind = 0, id = 0
    real(c_double)     :: position(3) = 0., e1(3) = 0., e2(3) = 0., &
                          normal(3) = (/ 0._c_double, 0._c_double, 1._c_double /)
  end type sensor

  ! MCBRAT_ABI_VERSION of include/mcbrat.h this module was written against: mcbrat_counters has 15 fields (badPhotons) since 2
  integer(c_int), parameter :: expectedAbiVersion = 3
  interface
    function mcbrat_abi_version() bind(C, name="mcbrat_abi_version") result(v)
      import :: c_int
      integer(c_int) :: v
    end function
    function mcbrat_create(device) bind(C, name="mcbrat_create") result(ctx)
      import :: c_ptr, c_int
      integer(c_int), value :: device
      type(c_ptr) :: ctx
    end function
    subroutine mcbrat_destroy(ctx) bind(C, name="mcbrat_destroy")
      import :: c_ptr
      type(c_ptr), value :: ctx
    end subroutine
    function mcbrat_last_error(ctx) bind(C, name="mcbrat_last_error") result(msg)
      import :: c_ptr
      type(c_ptr), value :: ctx
      type(c_ptr) :: msg
    end function
    function mcbrat_set_grid(ctx, nx, ny, nz, xe, ye, ze) bind(C, name="mcbrat_set_grid") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nx, ny, nz
      real(c_double), intent(in) :: xe(*), ye(*), ze(*)
      integer(c_int) :: rc
    end function
    function mcbrat_set_optics(ctx, nc, totalExt, cumExt, ssa, pfi, albedo) bind(C, name="mcbrat_set_optics") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nc
      real(c_double), intent(in) :: totalExt(*), cumExt(*), ssa(*)
      integer(c_int32_t), intent(in) :: pfi(*)
      real(c_double), value :: albedo
      integer(c_int) :: rc
    end function
    function mcbrat_set_inverse_table(ctx, comp, nSteps, nEntries, table) bind(C, name="mcbrat_set_inverse_table") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: comp, nSteps, nEntries
      real(c_float), intent(in) :: table(*)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_parameters(ctx, rayTracing, roulette, lwFlag) bind(C, name="mcbrat_specify_parameters") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: rayTracing, roulette
      real(c_float), value :: lwFlag
      integer(c_int) :: rc
    end function
    function mcbrat_set_surface_description(ctx, numX, numY, xPosition, yPosition, reflectance) &
        bind(C, name="mcbrat_set_surface_description") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: numX, numY
      real(c_double), dimension(*), intent(in) :: xPosition, yPosition
      real(c_float), dimension(*), intent(in) :: reflectance
      integer(c_int) :: rc
    end function
    function mcbrat_set_surface_brdf(ctx, kind, numX, numY, xPosition, yPosition, nParams, params) &
        bind(C, name="mcbrat_set_surface_brdf") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: kind, numX, numY, nParams
      real(c_double), dimension(*), intent(in) :: xPosition, yPosition
      real(c_float), dimension(*), intent(in) :: params
      integer(c_int) :: rc
    end function
    function mcbrat_set_source_solar(ctx, mu, azimuth) bind(C, name="mcbrat_set_source_solar") result(rc)
      import :: c_ptr, c_int, c_float
      type(c_ptr), value :: ctx
      real(c_float), value :: mu, azimuth
      integer(c_int) :: rc
    end function
    function mcbrat_set_source_random_azimuth(ctx, mu) bind(C, name="mcbrat_set_source_random_azimuth") result(rc)
      import :: c_ptr, c_int, c_float
      type(c_ptr), value :: ctx
      real(c_float), value :: mu
      integer(c_int) :: rc
    end function
    function mcbrat_set_source_flux(ctx) bind(C, name="mcbrat_set_source_flux") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
      integer(c_int) :: rc
    end function
    function mcbrat_set_source_spotlight(ctx, mu, azimuth, x, y) bind(C, name="mcbrat_set_source_spotlight") result(rc)
      import :: c_ptr, c_int, c_float
      type(c_ptr), value :: ctx
      real(c_float), value :: mu, azimuth, x, y
      integer(c_int) :: rc
    end function
    function mcbrat_set_source_emission(ctx, voxelWeights, fracAtms) bind(C, name="mcbrat_set_source_emission") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(in) :: voxelWeights(*)
      real(c_double), value :: fracAtms
      integer(c_int) :: rc
    end function
    function mcbrat_compute_radiative_transfer(ctx, seed, firstId, ppb, nBatches, nDone) &
        bind(C, name="mcbrat_compute_radiative_transfer") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: seed, firstId, ppb
      integer(c_int32_t), value :: nBatches
      integer(c_int64_t), intent(out) :: nDone
      integer(c_int) :: rc
    end function
    function mcbrat_report_results(ctx, mUp, mDown, mAbs, fUp, fDown, fAbs, prof, vol) &
        bind(C, name="mcbrat_report_results") result(rc)
      import :: c_ptr, c_int, c_float
      type(c_ptr), value :: ctx
      real(c_float), intent(out) :: mUp, mDown, mAbs
      real(c_float), intent(out) :: fUp(*), fDown(*), fAbs(*), prof(*), vol(*)
      integer(c_int) :: rc
    end function
    function mcbrat_moments_length(ctx) bind(C, name="mcbrat_moments_length") result(n)
      import :: c_ptr, c_int64_t
      type(c_ptr), value :: ctx
      integer(c_int64_t) :: n
    end function
    function mcbrat_reset_moments(ctx) bind(C, name="mcbrat_reset_moments") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
      integer(c_int) :: rc
    end function
    function mcbrat_get_moments(ctx, buf) bind(C, name="mcbrat_get_moments") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(out) :: buf(*)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_intensity(ctx, nDir, mus, phis, useRRI, zetaMin, useHybrid, numOrdersOrig, limitC, maxC) &
        bind(C, name="mcbrat_specify_intensity") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nDir, useRRI, useHybrid, numOrdersOrig, limitC
      real(c_float), intent(in) :: mus(*), phis(*)
      real(c_float), value :: zetaMin, maxC
      integer(c_int) :: rc
    end function
    function mcbrat_set_forward_table(ctx, component, nAngles, nEntries, table, origTable) &
        bind(C, name="mcbrat_set_forward_table") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_float
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: component, nAngles, nEntries
      real(c_float), intent(in) :: table(*), origTable(*)
      integer(c_int) :: rc
    end function
    function mcbrat_report_intensity(ctx, meanIntensity, intensity) bind(C, name="mcbrat_report_intensity") result(rc)
      import :: c_ptr, c_int, c_float
      type(c_ptr), value :: ctx
      real(c_float), intent(out) :: meanIntensity(*), intensity(*)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_scattering_orders(ctx, numRecScatOrd) bind(C, name="mcbrat_specify_scattering_orders") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: numRecScatOrd
      integer(c_int) :: rc
    end function
    function mcbrat_report_scattering_orders(ctx, mUp, mDown, fUp, fDown, mI, inten) &
        bind(C, name="mcbrat_report_scattering_orders") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, mUp, mDown, fUp, fDown, mI, inten   ! (c_null_ptr: not wanted)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_level_fluxes(ctx, enable) bind(C, name="mcbrat_specify_level_fluxes") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: enable
      integer(c_int) :: rc
    end function
    function mcbrat_report_level_fluxes(ctx, mUp, mDown, fUp, fDown) bind(C, name="mcbrat_report_level_fluxes") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, mUp, mDown, fUp, fDown   ! (c_null_ptr: not wanted)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_direct_level_fluxes(ctx, enable) bind(C, name="mcbrat_specify_direct_level_fluxes") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: enable
      integer(c_int) :: rc
    end function
    function mcbrat_report_direct_level_fluxes(ctx, mDirect, mDiffuse, fDirect, fDiffuse) &
        bind(C, name="mcbrat_report_direct_level_fluxes") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, mDirect, mDiffuse, fDirect, fDiffuse   ! (c_null_ptr: not wanted)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_actinic_flux(ctx, enable) bind(C, name="mcbrat_specify_actinic_flux") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: enable
      integer(c_int) :: rc
    end function
    function mcbrat_report_actinic_flux(ctx, mActinic, fActinic) bind(C, name="mcbrat_report_actinic_flux") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, mActinic, fActinic   ! (c_null_ptr: not wanted)
      integer(c_int) :: rc
    end function
    function mcbrat_specify_side_fluxes(ctx, enable) bind(C, name="mcbrat_specify_side_fluxes") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: enable
      integer(c_int) :: rc
    end function
    function mcbrat_report_side_fluxes(ctx, mSide, fSide) bind(C, name="mcbrat_report_side_fluxes") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, mSide, fSide   ! (c_null_ptr: not wanted)
      integer(c_int) :: rc
    end function
    function mcbrat_render_camera(ctx, cam, seed, firstSample, samplesPerPixel, numBatches, radiance, radianceStdErr, &
                                  batchMeans, dropped) bind(C, name="mcbrat_render_camera") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, camera
      type(c_ptr), value :: ctx
      type(camera), intent(in) :: cam
      integer(c_int64_t), value :: seed, firstSample, samplesPerPixel
      integer(c_int32_t), value :: numBatches
      type(c_ptr), value :: radiance, radianceStdErr, batchMeans   ! (c_null_ptr: not wanted; radiance is needed)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_camera_pathlengths(ctx, cam, numBins, pathEdges, seed, firstSample, samplesPerPixel, numBatches, &
                                              radiance, radianceStdErr, batchMeans, dropped) &
                                              bind(C, name="mcbrat_render_camera_pathlengths") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, camera
      type(c_ptr), value :: ctx
      type(camera), intent(in) :: cam
      integer(c_int32_t), value :: numBins
      real(c_float), intent(in) :: pathEdges(*)
      integer(c_int64_t), value :: seed, firstSample, samplesPerPixel
      integer(c_int32_t), value :: numBatches
      type(c_ptr), value :: radiance, radianceStdErr, batchMeans   ! (c_null_ptr: not wanted; radiance is needed)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_sensors(ctx, n, sensors, seed, firstSample, samplesPerSensor, numBatches, gridInLds, diffuse, direct, &
                                   diffuseStdErr, directStdErr, totalStdErr, batchMeans, dropped) &
                                   bind(C, name="mcbrat_render_sensors") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, sensor
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n, seed, firstSample, samplesPerSensor
      type(sensor), intent(in) :: sensors(*)
      integer(c_int32_t), value :: numBatches, gridInLds
      real(c_float), intent(out) :: diffuse(*), direct(*)
      type(c_ptr), value :: diffuseStdErr, directStdErr, totalStdErr, batchMeans   ! (c_null_ptr: not wanted)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_camera_emission(ctx, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, numBatches, &
                                           radiance, radianceStdErr, batchMeans, dropped) &
                                           bind(C, name="mcbrat_render_camera_emission") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, camera
      type(c_ptr), value :: ctx
      type(camera), intent(in) :: cam
      real(c_float), intent(in) :: cellSource(*), surfaceSource(*)
      integer(c_int64_t), value :: seed, firstSample, samplesPerPixel
      integer(c_int32_t), value :: numBatches
      type(c_ptr), value :: radiance, radianceStdErr, batchMeans   ! (c_null_ptr: not wanted; radiance is needed)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_sensors_emission(ctx, n, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, &
                                            numBatches, gridInLds, irradiance, irradianceStdErr, batchMeans, dropped) &
                                            bind(C, name="mcbrat_render_sensors_emission") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, sensor
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n, seed, firstSample, samplesPerSensor
      type(sensor), intent(in) :: sensors(*)
      real(c_float), intent(in) :: cellSource(*), surfaceSource(*)
      integer(c_int32_t), value :: numBatches, gridInLds
      real(c_float), intent(out) :: irradiance(*)
      type(c_ptr), value :: irradianceStdErr, batchMeans   ! (c_null_ptr: not wanted)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_camera_emission_expected(ctx, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, numBatches, &
                                           radiance, radianceStdErr, batchMeans, dropped) &
                                           bind(C, name="mcbrat_render_camera_emission_expected") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, camera
      type(c_ptr), value :: ctx
      type(camera), intent(in) :: cam
      real(c_float), intent(in) :: cellSource(*), surfaceSource(*)
      integer(c_int64_t), value :: seed, firstSample, samplesPerPixel
      integer(c_int32_t), value :: numBatches
      type(c_ptr), value :: radiance, radianceStdErr, batchMeans   ! (c_null_ptr: not wanted; radiance is needed)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_render_sensors_emission_expected(ctx, n, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, &
                                            numBatches, gridInLds, irradiance, irradianceStdErr, batchMeans, dropped) &
                                            bind(C, name="mcbrat_render_sensors_emission_expected") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_float, sensor
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n, seed, firstSample, samplesPerSensor
      type(sensor), intent(in) :: sensors(*)
      real(c_float), intent(in) :: cellSource(*), surfaceSource(*)
      integer(c_int32_t), value :: numBatches, gridInLds
      real(c_float), intent(out) :: irradiance(*)
      type(c_ptr), value :: irradianceStdErr, batchMeans   ! (c_null_ptr: not wanted)
      integer(c_int64_t), intent(out) :: dropped
      integer(c_int) :: rc
    end function
    function mcbrat_sun_transmittance(ctx, n, xyz, transmittance) bind(C, name="mcbrat_sun_transmittance") result(rc)
      import :: c_ptr, c_int, c_int64_t, c_double, c_float
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n
      real(c_double), intent(in) :: xyz(*)
      real(c_float), intent(out) :: transmittance(*)
      integer(c_int) :: rc
    end function
    function mcbrat_forward_table_legendre(nCoef, coef, nAngles, table) bind(C, name="mcbrat_forward_table_legendre") result(rc)
      import :: c_int, c_int32_t, c_float
      integer(c_int32_t), value :: nCoef, nAngles
      real(c_float), intent(in) :: coef(*)
      real(c_float), intent(out) :: table(*)
      integer(c_int) :: rc
    end function
    function mcbrat_set_async(ctx, enable) bind(C, name="mcbrat_set_async") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: enable
      integer(c_int) :: rc
    end function
    function mcbrat_synchronize(ctx) bind(C, name="mcbrat_synchronize") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
      integer(c_int) :: rc
    end function
    function mcbrat_last_trace_ms(ctx) bind(C, name="mcbrat_last_trace_ms") result(ms)
      import :: c_ptr, c_float
      type(c_ptr), value :: ctx
      real(c_float) :: ms
    end function
    function mcbrat_chain_after(ctx, previous) bind(C, name="mcbrat_chain_after") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, previous
      integer(c_int) :: rc
    end function
    function mcbrat_get_counters(ctx, counters) bind(C, name="mcbrat_get_counters") result(rc)
      import :: c_ptr, c_int, c_int64_t
      type(c_ptr), value :: ctx
      integer(c_int64_t), dimension(15), intent(out) :: counters   ! mcbrat_counters: 14 event / loop counters, then badPhotons
      integer(c_int) :: rc
    end function
    function mcbrat_set_walk_options(ctx, layerSkip, blockWalk) bind(C, name="mcbrat_set_walk_options") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: layerSkip, blockWalk
      integer(c_int) :: rc
    end function
    function mcbrat_set_option(ctx, name, value) bind(C, name="mcbrat_set_option") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_char
      type(c_ptr), value :: ctx
      character(kind=c_char), dimension(*), intent(in) :: name
      integer(c_int32_t), value :: value
      integer(c_int) :: rc
    end function
    function mcbrat_frequency_distribution(ctx, seed, firstDraw, numLambda, cdf, totalPhotons, distribution) &
        bind(C, name="mcbrat_frequency_distribution") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: seed, firstDraw, totalPhotons
      integer(c_int32_t), value :: numLambda
      real(c_double), intent(in) :: cdf(*)
      integer(c_int64_t), intent(out) :: distribution(*)
      integer(c_int) :: rc
    end function
    function mcbrat_moments_device_pointer(ctx) bind(C, name="mcbrat_moments_device_pointer") result(p)
      import :: c_ptr
      type(c_ptr), value :: ctx
      type(c_ptr) :: p
    end function
    function mcbrat_bind_moments(ctx, deviceBuffer) bind(C, name="mcbrat_bind_moments") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, deviceBuffer
      integer(c_int) :: rc
    end function
    function mcbrat_inverse_table_legendre(nCoef, coef, nSteps, table) bind(C, name="mcbrat_inverse_table_legendre") result(rc)
      import :: c_int, c_int32_t, c_float
      integer(c_int32_t), value :: nCoef, nSteps
      real(c_float), intent(in) :: coef(*)
      real(c_float), intent(out) :: table(*)
      integer(c_int) :: rc
    end function
  end interface

contains
  !------------------------------------------------------------------------------------------
  function lastMessage(this) result(msg)
    type(integrator), intent(in) :: this
    character(len=256) :: msg
    character(kind=c_char), pointer :: chars(:)
    type(c_ptr) :: p
    integer :: i
    msg = ""
    p = mcbrat_last_error(this%ctx)
    if (.not. c_associated(p)) return
    call c_f_pointer(p, chars, (/ 256 /))
    do i = 1, 256
      if (chars(i) == c_null_char) exit
      msg(i:i) = chars(i)
    end do
  end function lastMessage
  !------------------------------------------------------------------------------------------
  ! new_Integrator(atmosphere, status): here from the cell edges getInfo_Domain returns
  function new_Integrator(xPosition, yPosition, zPosition, device, ierr) result(new)
    real(8), dimension(:), intent(in) :: xPosition, yPosition, zPosition
    integer,               intent(in) :: device
    integer,               intent(out):: ierr
    type(integrator) :: new
    new%ctx = c_null_ptr
    if (mcbrat_abi_version() /= expectedAbiVersion) then
      ierr = 2   ! "new_Integrator: libmcbrat_hip.so is of another ABI version than this module" (a stale build: the
      return     !  dimension(15) counter buffer of numBadPhotons would not be what the library writes)
    end if
    new%ctx = mcbrat_create(int(device, c_int))
    if (.not. c_associated(new%ctx)) then
      ierr = 1   ! "new_Integrator: no usable HIP device" -- there is no CPU fallback
      return
    end if
    new%numX = size(xPosition) - 1; new%numY = size(yPosition) - 1; new%numZ = size(zPosition) - 1
    ierr = mcbrat_set_grid(new%ctx, int(new%numX, c_int32_t), int(new%numY, c_int32_t), int(new%numZ, c_int32_t), &
                           xPosition, yPosition, zPosition)
    new%readyToCompute = (ierr == 0)
  end function new_Integrator
  !------------------------------------------------------------------------------------------
  logical function isReady_Integrator(this)
    type(integrator), intent(in) :: this
    isReady_Integrator = this%readyToCompute
  end function isReady_Integrator
  !------------------------------------------------------------------------------------------
  subroutine finalize_Integrator(this)
    type(integrator), intent(inout) :: this
    if (c_associated(this%ctx)) call mcbrat_destroy(this%ctx)
    this%ctx = c_null_ptr
    this%readyToCompute = .false.
  end subroutine finalize_Integrator
  !------------------------------------------------------------------------------------------
  ! What computeRT pulls from the domain (getInfo_Domain :441-443)
  subroutine setOpticalProperties(this, totalExt, cumExt, ssa, phaseFuncI, albedo, ierr)
    type(integrator),            intent(inout) :: this
    real(8), dimension(:,:,:),   intent(in)    :: totalExt
    real(8), dimension(:,:,:,:), intent(in)    :: cumExt, ssa
    integer, dimension(:,:,:,:), intent(in)    :: phaseFuncI
    real(8),                     intent(in)    :: albedo
    integer,                     intent(out)   :: ierr
    ierr = mcbrat_set_optics(this%ctx, int(size(cumExt, 4), c_int32_t), totalExt, cumExt, ssa, phaseFuncI, albedo)
  end subroutine setOpticalProperties
  !------------------------------------------------------------------------------------------
  subroutine setInverseTable(this, component, values, ierr)   ! inversePhaseFuncs(component)%values
    type(integrator),     intent(inout) :: this
    integer,              intent(in)    :: component
    real, dimension(:,:), intent(in)    :: values
    integer,              intent(out)   :: ierr
    ierr = mcbrat_set_inverse_table(this%ctx, int(component, c_int32_t), int(size(values, 1), c_int32_t), &
                                    int(size(values, 2), c_int32_t), values)
  end subroutine setInverseTable
  !------------------------------------------------------------------------------------------
  ! specifyParameters(surfaceBDRF = new_SurfaceDescription(surfaceParameters, xPosition, yPosition))
  ! (monteCarloRadiativeTransfer.f95:1173-1176): reflectance = surfaceParameters(1, :, :)
  subroutine setSurfaceDescription(this, reflectance, xPosition, yPosition, ierr)
    type(integrator),      intent(inout) :: this
    real, dimension(:,:),  intent(in)    :: reflectance
    real(8), dimension(:), intent(in)    :: xPosition, yPosition
    integer,               intent(out)   :: ierr
    if (size(reflectance, 1) /= size(xPosition) - 1 .or. size(reflectance, 2) /= size(yPosition) - 1) then
      ierr = 2   ! "new_SurfaceDescription: position vector(s) are incorrect length."
      return
    end if
    ierr = mcbrat_set_surface_description(this%ctx, int(size(xPosition), c_int32_t), int(size(yPosition), c_int32_t), &
                                          xPosition, yPosition, reflectance)
  end subroutine setSurfaceDescription
  !------------------------------------------------------------------------------------------
  ! A surface BRDF per patch (DESIGN.md section 4.11): model "Lambertian" (1 parameter), "RPV" (rho0, k, Theta, rhoC) or
  ! "RossLi" (fIso, fVol, fGeo), or "CoxMunk" (U, n, rhoWc, aW: section 4.11.1);
  ! parameters(numberOfParameters, numX-1, numY-1) as the reference's BRDFParameters
  subroutine setSurfaceBRDF(this, model, parameters, xPosition, yPosition, ierr)
    type(integrator),        intent(inout) :: this
    character(len=*),        intent(in)    :: model
    real, dimension(:,:,:),  intent(in)    :: parameters
    real(8), dimension(:),   intent(in)    :: xPosition, yPosition
    integer,                 intent(out)   :: ierr
    integer(c_int32_t) :: kind
    real, dimension(size(parameters, 2), size(parameters, 3), size(parameters, 1)) :: packed   ! the C layout: x fastest, parameter slowest
    integer :: k
    select case (trim(model))
    case ("Lambertian")
      kind = 0
    case ("RPV")
      kind = 1
    case ("RossLi")
      kind = 2
    case ("CoxMunk")
      kind = 3
    case default
      ierr = 2   ! "new_SurfaceDescription: unknown surface BRDF model"
      return
    end select
    if (size(parameters, 2) /= size(xPosition) - 1 .or. size(parameters, 3) /= size(yPosition) - 1) then
      ierr = 2   ! "new_SurfaceDescription: position vector(s) are incorrect length."
      return
    end if
    do k = 1, size(parameters, 1)
      packed(:, :, k) = parameters(k, :, :)
    end do
    ierr = mcbrat_set_surface_brdf(this%ctx, kind, int(size(xPosition), c_int32_t), int(size(yPosition), c_int32_t), &
                                   xPosition, yPosition, int(size(parameters, 1), c_int32_t), packed)
  end subroutine setSurfaceBRDF
  !------------------------------------------------------------------------------------------
  subroutine setSolarSource(this, solarMu, solarAzimuth, ierr)   ! new_PhotonStream, Directional
    type(integrator), intent(inout) :: this
    real,             intent(in)    :: solarMu, solarAzimuth
    integer,          intent(out)   :: ierr
    ierr = mcbrat_set_source_solar(this%ctx, solarMu, solarAzimuth)
  end subroutine setSolarSource
  !------------------------------------------------------------------------------------------
  subroutine setRandomAzimuthSource(this, solarMu, ierr)   ! new_PhotonStream, RandomAzimuth
    type(integrator), intent(inout) :: this
    real,             intent(in)    :: solarMu
    integer,          intent(out)   :: ierr
    ierr = mcbrat_set_source_random_azimuth(this%ctx, solarMu)
  end subroutine setRandomAzimuthSource
  !------------------------------------------------------------------------------------------
  subroutine setFluxSource(this, ierr)   ! new_PhotonStream, Flux (isotropic incidence)
    type(integrator), intent(inout) :: this
    integer,          intent(out)   :: ierr
    ierr = mcbrat_set_source_flux(this%ctx)
  end subroutine setFluxSource
  !------------------------------------------------------------------------------------------
  subroutine setSpotlightSource(this, solarMu, solarAzimuth, solarX, solarY, ierr)   ! new_PhotonStream, Spotlight
    type(integrator), intent(inout) :: this
    real,             intent(in)    :: solarMu, solarAzimuth, solarX, solarY   ! solarX, solarY: fractions of the domain in (0, 1]
    integer,          intent(out)   :: ierr
    ierr = mcbrat_set_source_spotlight(this%ctx, solarMu, solarAzimuth, solarX, solarY)
  end subroutine setSpotlightSource
  !------------------------------------------------------------------------------------------
  subroutine setEmissionSource(this, voxelWeights, fracAtmsPower, ierr)   ! new_PhotonStream, BBEmission
    type(integrator),          intent(inout) :: this
    real(8), dimension(:,:,:), intent(in)    :: voxelWeights
    real(8),                   intent(in)    :: fracAtmsPower
    integer,                   intent(out)   :: ierr
    ierr = mcbrat_set_source_emission(this%ctx, voxelWeights, fracAtmsPower)
  end subroutine setEmissionSource
  !------------------------------------------------------------------------------------------
  ! specifyParameters: the keywords the driver passes (monteCarloDriver.f95:540-572)
  subroutine specifyParameters(this, useRayTracing, useRussianRoulette, LW_flag, ierr)
    type(integrator), intent(inout) :: this
    logical,          intent(in)    :: useRayTracing, useRussianRoulette
    real,             intent(in)    :: LW_flag
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_parameters(this%ctx, merge(1_c_int32_t, 0_c_int32_t, useRayTracing), &
                                     merge(1_c_int32_t, 0_c_int32_t, useRussianRoulette), LW_flag)
  end subroutine specifyParameters
  !------------------------------------------------------------------------------------------
  ! computeRadiativeTransfer(thisIntegrator, thisDomain, randomNumbers, incomingPhotons,
  !                          numPhotonsPerBatch, numPhotonsProcessed, status)
  ! randomNumbers -> (seed, firstPhotonId): counter-based generator keyed by photon id.
  subroutine computeRadiativeTransfer(this, seed, firstPhotonId, numPhotonsPerBatch, numBatches, &
                                      numPhotonsProcessed, ierr)
    type(integrator), intent(inout) :: this
    integer(8),       intent(in)    :: seed, firstPhotonId, numPhotonsPerBatch
    integer,          intent(in)    :: numBatches
    integer(8),       intent(out)   :: numPhotonsProcessed
    integer,          intent(out)   :: ierr
    if (.not. this%readyToCompute) then
      ierr = 1; numPhotonsProcessed = 0
      return
    end if
    ierr = mcbrat_compute_radiative_transfer(this%ctx, seed, firstPhotonId, numPhotonsPerBatch, &
                                             int(numBatches, c_int32_t), numPhotonsProcessed)
  end subroutine computeRadiativeTransfer
  !------------------------------------------------------------------------------------------
  subroutine reportResults(this, meanFluxUp, meanFluxDown, meanFluxAbsorbed, fluxUp, fluxDown, fluxAbsorbed, &
                           absorbedProfile, volumeAbsorption, ierr)
    type(integrator),         intent(in)  :: this
    real,                     intent(out) :: meanFluxUp, meanFluxDown, meanFluxAbsorbed
    real, dimension(:,:),     intent(out) :: fluxUp, fluxDown, fluxAbsorbed
    real, dimension(:),       intent(out) :: absorbedProfile
    real, dimension(:,:,:),   intent(out) :: volumeAbsorption
    integer,                  intent(out) :: ierr
    if (any(shape(fluxUp) /= (/ this%numX, this%numY /)) .or. size(absorbedProfile) /= this%numZ .or. &
        any(shape(volumeAbsorption) /= (/ this%numX, this%numY, this%numZ /))) then
      ierr = 2   ! "reportResults: ... array is the wrong size"
      return
    end if
    ierr = mcbrat_report_results(this%ctx, meanFluxUp, meanFluxDown, meanFluxAbsorbed, fluxUp, fluxDown, fluxAbsorbed, &
                                 absorbedProfile, volumeAbsorption)
  end subroutine reportResults
  !------------------------------------------------------------------------------------------
  integer(8) function momentsLength(this)
    type(integrator), intent(in) :: this
    momentsLength = mcbrat_moments_length(this%ctx)
  end function momentsLength
  subroutine resetMoments(this, ierr)
    type(integrator), intent(inout) :: this
    integer, intent(out) :: ierr
    ierr = mcbrat_reset_moments(this%ctx)
  end subroutine resetMoments
  subroutine getMoments(this, buffer, ierr)   ! header(8) + S1(M) + S2(M), see include/mcbrat.h
    type(integrator), intent(inout) :: this
    real(8), dimension(:), intent(out) :: buffer
    integer, intent(out) :: ierr
    ierr = mcbrat_get_moments(this%ctx, buffer)
  end subroutine getMoments
  ! specifyParameters, intensity keywords (:1046-1292): directions and variance-reduction choices
  subroutine specifyIntensity(this, intensityMus, intensityPhis, useRussianRouletteForIntensity, zetaMin, &
                              useHybridPhaseFunsForIntenCalcs, numOrdersOrigPhaseFunIntenCalcs, &
                              limitIntensityContributions, maxIntensityContribution, ierr)
    type(integrator),   intent(inout) :: this
    real, dimension(:), intent(in)    :: intensityMus, intensityPhis
    logical,            intent(in)    :: useRussianRouletteForIntensity, useHybridPhaseFunsForIntenCalcs, &
                                         limitIntensityContributions
    real,               intent(in)    :: zetaMin, maxIntensityContribution
    integer,            intent(in)    :: numOrdersOrigPhaseFunIntenCalcs
    integer,            intent(out)   :: ierr
    ierr = mcbrat_specify_intensity(this%ctx, int(size(intensityMus), c_int32_t), intensityMus, intensityPhis, &
                                    merge(1_c_int32_t, 0_c_int32_t, useRussianRouletteForIntensity), zetaMin, &
                                    merge(1_c_int32_t, 0_c_int32_t, useHybridPhaseFunsForIntenCalcs), &
                                    int(numOrdersOrigPhaseFunIntenCalcs, c_int32_t), &
                                    merge(1_c_int32_t, 0_c_int32_t, limitIntensityContributions), maxIntensityContribution)
  end subroutine specifyIntensity
  ! tabulatedPhaseFunctions(component)%values / tabulatedOrigPhaseFunctions(component)%values (nAngles, nEntries)
  subroutine setForwardTable(this, component, values, origValues, ierr)
    type(integrator),     intent(inout) :: this
    integer,              intent(in)    :: component
    real, dimension(:,:), intent(in)    :: values, origValues
    integer,              intent(out)   :: ierr
    ierr = mcbrat_set_forward_table(this%ctx, int(component, c_int32_t), int(size(values, 1), c_int32_t), &
                                    int(size(values, 2), c_int32_t), values, origValues)
  end subroutine setForwardTable
  subroutine reportIntensity(this, meanIntensity, intensity, ierr)   ! reportResults(meanIntensity, intensity) :980-1010
    type(integrator),       intent(in)  :: this
    real, dimension(:),     intent(out) :: meanIntensity
    real, dimension(:,:,:), intent(out) :: intensity
    integer,                intent(out) :: ierr
    if (size(intensity, 1) /= this%numX .or. size(intensity, 2) /= this%numY .or. size(intensity, 3) /= size(meanIntensity)) then
      ierr = 1   ! "reportResults: intensity array has wrong dimensions."
      return
    end if
    ierr = mcbrat_report_intensity(this%ctx, meanIntensity, intensity)
  end subroutine reportIntensity
  subroutine forwardTableLegendre(coefficients, table, ierr)   ! tabulateForwardPhaseFunctions for one Legendre entry
    real, dimension(:), intent(in)  :: coefficients
    real, dimension(:), intent(out) :: table
    integer,            intent(out) :: ierr
    ierr = mcbrat_forward_table_legendre(int(size(coefficients), c_int32_t), coefficients, int(size(table), c_int32_t), table)
  end subroutine forwardTableLegendre
  ! Per-batch callers (the driver's loop, monteCarloDriver.f95:1008): let consecutive calls overlap on the GPU;
  ! reportResults / getMoments synchronise by themselves.
  subroutine setAsynchronous(this, enable, ierr)
    type(integrator), intent(inout) :: this
    logical, intent(in) :: enable
    integer, intent(out) :: ierr
    ierr = mcbrat_set_async(this%ctx, merge(1_c_int32_t, 0_c_int32_t, enable))
  end subroutine setAsynchronous
  subroutine synchronize(this, ierr)
    type(integrator), intent(inout) :: this
    integer, intent(out) :: ierr
    ierr = mcbrat_synchronize(this%ctx)
  end subroutine synchronize
  !------------------------------------------------------------------------------------------
  ! layerSkip (one-extinction layers and the clear-air flight) / blockWalk: .false. restores the reference's face-by-face walk (include/mcbrat.h)
  subroutine setWalkOptions(this, layerSkip, blockWalk, ierr)
    type(integrator), intent(inout) :: this
    logical, intent(in) :: layerSkip, blockWalk
    integer, intent(out) :: ierr
    ierr = mcbrat_set_walk_options(this%ctx, merge(1_c_int32_t, 0_c_int32_t, layerSkip), merge(1_c_int32_t, 0_c_int32_t, blockWalk))
  end subroutine setWalkOptions
  ! Scheduling options by name (include/mcbrat.h: mcbrat_set_option), e.g. setOption(this, "jumpThreshold", 16, ierr); none of them
  ! changes a result.  The reference has no counterpart.
  subroutine setOption(this, name, value, ierr)
    type(integrator), intent(inout) :: this
    character(len=*), intent(in) :: name
    integer, intent(in) :: value
    integer, intent(out) :: ierr
    ierr = mcbrat_set_option(this%ctx, trim(name) // c_null_char, int(value, c_int32_t))
  end subroutine setOption
  ! computeRT's nBad (Integrators/monteCarloRadiativeTransfer.f95:420, :562-563: photons dropped because their step was not
  ! positive): here the photons dropped because a loop bound of the kernels was reached, since this integrator was created
  ! (mcbrat_counters.badPhotons, include/mcbrat.h).  Synchronises.
  ! specifyParameters(recScatOrd, numRecScatOrd) (:1159-1171, :1293-1330): fluxes and radiances by scattering order
  ! 0..numRecScatOrd; numRecScatOrd < 0 records nothing.  Changes momentsLength().
  subroutine specifyScatteringOrders(this, numRecScatOrd, ierr)
    type(integrator), intent(inout) :: this
    integer,          intent(in)    :: numRecScatOrd
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_scattering_orders(this%ctx, int(numRecScatOrd, c_int32_t))
    if (ierr == 0) this%numRecScatOrd = max(numRecScatOrd, -1)
  end subroutine specifyScatteringOrders

  ! reportResults(meanFluxUpByScatOrd, meanFluxDownByScatOrd, fluxUpByScatOrd, fluxDownByScatOrd, meanIntensityByScatOrd,
  ! intensityByScatOrd) (:850-864, :887-903, :1010-1040) for the last batch; the reference's shapes, order last
  subroutine reportResultsByScatOrd(this, meanFluxUpByScatOrd, meanFluxDownByScatOrd, fluxUpByScatOrd, fluxDownByScatOrd, &
                                    meanIntensityByScatOrd, intensityByScatOrd, ierr)
    type(integrator), intent(inout) :: this
    real, dimension(0:),          contiguous, optional, target, intent(out) :: meanFluxUpByScatOrd, meanFluxDownByScatOrd
    real, dimension(:, :, 0:),    contiguous, optional, target, intent(out) :: fluxUpByScatOrd, fluxDownByScatOrd
    real, dimension(:, 0:),       contiguous, optional, target, intent(out) :: meanIntensityByScatOrd
    real, dimension(:, :, :, 0:), contiguous, optional, target, intent(out) :: intensityByScatOrd
    integer,                      intent(out) :: ierr
    type(c_ptr) :: mUp, mDown, fUp, fDown, mI, inten
    integer :: n
    n = this%numRecScatOrd + 1
    mUp = c_null_ptr; mDown = c_null_ptr; fUp = c_null_ptr; fDown = c_null_ptr; mI = c_null_ptr; inten = c_null_ptr
    ierr = 2   ! "reportResults: ...ByScatOrd is the wrong size"
    if (present(meanFluxUpByScatOrd)) then
      if (size(meanFluxUpByScatOrd) /= n) return
      mUp = c_loc(meanFluxUpByScatOrd)
    end if
    if (present(meanFluxDownByScatOrd)) then
      if (size(meanFluxDownByScatOrd) /= n) return
      mDown = c_loc(meanFluxDownByScatOrd)
    end if
    if (present(fluxUpByScatOrd)) then
      if (any(shape(fluxUpByScatOrd) /= (/ this%numX, this%numY, n /))) return
      fUp = c_loc(fluxUpByScatOrd)
    end if
    if (present(fluxDownByScatOrd)) then
      if (any(shape(fluxDownByScatOrd) /= (/ this%numX, this%numY, n /))) return
      fDown = c_loc(fluxDownByScatOrd)
    end if
    if (present(meanIntensityByScatOrd)) then
      if (size(meanIntensityByScatOrd, 2) /= n) return
      mI = c_loc(meanIntensityByScatOrd)
    end if
    if (present(intensityByScatOrd)) then
      if (size(intensityByScatOrd, 1) /= this%numX .or. size(intensityByScatOrd, 2) /= this%numY .or. &
          size(intensityByScatOrd, 4) /= n) return
      inten = c_loc(intensityByScatOrd)
    end if
    ierr = mcbrat_report_scattering_orders(this%ctx, mUp, mDown, fUp, fDown, mI, inten)
  end subroutine reportResultsByScatOrd

  ! specifyParameters(recLevelFluxes): upward and downward flux through every level (z face) of every column.  Refused together
  ! with intensity directions, scattering orders and BRDF surfaces.  Changes momentsLength().
  subroutine specifyLevelFluxes(this, enable, ierr)
    type(integrator), intent(inout) :: this
    logical,          intent(in)    :: enable
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_level_fluxes(this%ctx, merge(1_c_int32_t, 0_c_int32_t, enable))
  end subroutine specifyLevelFluxes

  ! the last batch's level fluxes: meanLevelFlux*(0:numZ), levelFlux*(numX, numY, 0:numZ); level 0 is the surface, numZ the top
  subroutine reportLevelFluxes(this, meanLevelFluxUp, meanLevelFluxDown, levelFluxUp, levelFluxDown, ierr)
    type(integrator), intent(inout) :: this
    real, dimension(0:),       contiguous, optional, target, intent(out) :: meanLevelFluxUp, meanLevelFluxDown
    real, dimension(:, :, 0:), contiguous, optional, target, intent(out) :: levelFluxUp, levelFluxDown
    integer,                   intent(out) :: ierr
    type(c_ptr) :: mUp, mDown, fUp, fDown
    integer :: n
    n = this%numZ + 1
    mUp = c_null_ptr; mDown = c_null_ptr; fUp = c_null_ptr; fDown = c_null_ptr
    ierr = 2   ! "reportResults: levelFlux... is the wrong size"
    if (present(meanLevelFluxUp)) then
      if (size(meanLevelFluxUp) /= n) return
      mUp = c_loc(meanLevelFluxUp)
    end if
    if (present(meanLevelFluxDown)) then
      if (size(meanLevelFluxDown) /= n) return
      mDown = c_loc(meanLevelFluxDown)
    end if
    if (present(levelFluxUp)) then
      if (any(shape(levelFluxUp) /= (/ this%numX, this%numY, n /))) return
      fUp = c_loc(levelFluxUp)
    end if
    if (present(levelFluxDown)) then
      if (any(shape(levelFluxDown) /= (/ this%numX, this%numY, n /))) return
      fDown = c_loc(levelFluxDown)
    end if
    ierr = mcbrat_report_level_fluxes(this%ctx, mUp, mDown, fUp, fDown)
  end subroutine reportLevelFluxes

  ! specifyParameters(recDirectLevelFluxes): the direct beam apart from the diffuse light in the downward level flux.  Needs
  ! level fluxes (specifyLevelFluxes first) and a solar source.  Changes momentsLength().
  subroutine specifyDirectLevelFluxes(this, enable, ierr)
    type(integrator), intent(inout) :: this
    logical,          intent(in)    :: enable
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_direct_level_fluxes(this%ctx, merge(1_c_int32_t, 0_c_int32_t, enable))
  end subroutine specifyDirectLevelFluxes

  ! the last batch's direct and diffuse parts of levelFluxDown: mean*(0:numZ), levelFluxDown*(numX, numY, 0:numZ)
  subroutine reportDirectLevelFluxes(this, meanLevelFluxDownDirect, meanLevelFluxDownDiffuse, levelFluxDownDirect, &
                                     levelFluxDownDiffuse, ierr)
    type(integrator), intent(inout) :: this
    real, dimension(0:),       contiguous, optional, target, intent(out) :: meanLevelFluxDownDirect, meanLevelFluxDownDiffuse
    real, dimension(:, :, 0:), contiguous, optional, target, intent(out) :: levelFluxDownDirect, levelFluxDownDiffuse
    integer,                   intent(out) :: ierr
    type(c_ptr) :: mDirect, mDiffuse, fDirect, fDiffuse
    integer :: n
    n = this%numZ + 1
    mDirect = c_null_ptr; mDiffuse = c_null_ptr; fDirect = c_null_ptr; fDiffuse = c_null_ptr
    ierr = 2   ! "reportResults: levelFluxDown... is the wrong size"
    if (present(meanLevelFluxDownDirect)) then
      if (size(meanLevelFluxDownDirect) /= n) return
      mDirect = c_loc(meanLevelFluxDownDirect)
    end if
    if (present(meanLevelFluxDownDiffuse)) then
      if (size(meanLevelFluxDownDiffuse) /= n) return
      mDiffuse = c_loc(meanLevelFluxDownDiffuse)
    end if
    if (present(levelFluxDownDirect)) then
      if (any(shape(levelFluxDownDirect) /= (/ this%numX, this%numY, n /))) return
      fDirect = c_loc(levelFluxDownDirect)
    end if
    if (present(levelFluxDownDiffuse)) then
      if (any(shape(levelFluxDownDiffuse) /= (/ this%numX, this%numY, n /))) return
      fDiffuse = c_loc(levelFluxDownDiffuse)
    end if
    ierr = mcbrat_report_direct_level_fluxes(this%ctx, mDirect, mDiffuse, fDirect, fDiffuse)
  end subroutine reportDirectLevelFluxes

  ! specifyParameters(recActinicFlux): the actinic flux of every cell by track length.  Solar sources only; may be combined with
  ! level fluxes, not with their direct tally.  Changes momentsLength().
  subroutine specifyActinicFlux(this, enable, ierr)
    type(integrator), intent(inout) :: this
    logical,          intent(in)    :: enable
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_actinic_flux(this%ctx, merge(1_c_int32_t, 0_c_int32_t, enable))
  end subroutine specifyActinicFlux

  ! the last batch's actinic flux: meanActinicFlux(numZ), actinicFlux(numX, numY, numZ)
  subroutine reportActinicFlux(this, meanActinicFlux, actinicFlux, ierr)
    type(integrator), intent(inout) :: this
    real, dimension(:),       contiguous, optional, target, intent(out) :: meanActinicFlux
    real, dimension(:, :, :), contiguous, optional, target, intent(out) :: actinicFlux
    integer,                  intent(out) :: ierr
    type(c_ptr) :: mActinic, fActinic
    mActinic = c_null_ptr; fActinic = c_null_ptr
    ierr = 2   ! "reportResults: actinicFlux is the wrong size"
    if (present(meanActinicFlux)) then
      if (size(meanActinicFlux) /= this%numZ) return
      mActinic = c_loc(meanActinicFlux)
    end if
    if (present(actinicFlux)) then
      if (any(shape(actinicFlux) /= (/ this%numX, this%numY, this%numZ /))) return
      fActinic = c_loc(actinicFlux)
    end if
    ierr = mcbrat_report_actinic_flux(this%ctx, mActinic, fActinic)
  end subroutine reportActinicFlux

  ! specifyParameters(recSideFluxes): the flux through the vertical faces of every cell.  Solar sources only; needs level fluxes
  ! (specifyLevelFluxes first), not together with their direct tally or the actinic flux.  Changes momentsLength().
  subroutine specifySideFluxes(this, enable, ierr)
    type(integrator), intent(inout) :: this
    logical,          intent(in)    :: enable
    integer,          intent(out)   :: ierr
    ierr = mcbrat_specify_side_fluxes(this%ctx, merge(1_c_int32_t, 0_c_int32_t, enable))
  end subroutine specifySideFluxes

  ! the last batch's side fluxes, the last index 1 .. 4: x plus, x minus, y plus, y minus --
  ! meanSideFluxes(numZ, 4), sideFluxes(numX, numY, numZ, 4)
  subroutine reportSideFluxes(this, meanSideFluxes, sideFluxes, ierr)
    type(integrator), intent(inout) :: this
    real, dimension(:, :),       contiguous, optional, target, intent(out) :: meanSideFluxes
    real, dimension(:, :, :, :), contiguous, optional, target, intent(out) :: sideFluxes
    integer,                     intent(out) :: ierr
    type(c_ptr) :: mSide, fSide
    mSide = c_null_ptr; fSide = c_null_ptr
    ierr = 2   ! "reportResults: sideFluxes is the wrong size"
    if (present(meanSideFluxes)) then
      if (any(shape(meanSideFluxes) /= (/ this%numZ, 4 /))) return
      mSide = c_loc(meanSideFluxes)
    end if
    if (present(sideFluxes)) then
      if (any(shape(sideFluxes) /= (/ this%numX, this%numY, this%numZ, 4 /))) return
      fSide = c_loc(sideFluxes)
    end if
    ierr = mcbrat_report_side_fluxes(this%ctx, mSide, fSide)
  end subroutine reportSideFluxes

  integer(8) function numBadPhotons(this)
    type(integrator), intent(in) :: this
    integer(c_int64_t), dimension(15) :: counters
    numBadPhotons = -1
    if (mcbrat_get_counters(this%ctx, counters) == 0) numBadPhotons = counters(15)
  end function numBadPhotons
  ! getFrequencyDistr (src/emissionAndBroadBandWeights.f95:552-572) with the draws made and counted on the device
  subroutine getFrequencyDistr(this, CDF, totalPhotons, iseed, distribution, ierr)
    type(integrator), intent(inout) :: this
    real(8), dimension(:), intent(in) :: CDF
    integer(8), intent(in) :: totalPhotons
    integer, intent(in) :: iseed
    integer(8), dimension(:), intent(out) :: distribution
    integer, intent(out) :: ierr
    ierr = mcbrat_frequency_distribution(this%ctx, int(iseed, c_int64_t), 0_c_int64_t, int(size(CDF), c_int32_t), CDF, &
                                         int(totalPhotons, c_int64_t), distribution)
  end subroutine getFrequencyDistr
  ! spectrally integrated runs: `this` (another wavelength's integrator on the same grid) accumulates into `first`'s moments
  subroutine shareMoments(this, first, ierr)
    type(integrator), intent(inout) :: this, first
    integer, intent(out) :: ierr
    ierr = mcbrat_bind_moments(this%ctx, mcbrat_moments_device_pointer(first%ctx))
  end subroutine shareMoments
  ! ... and, with both integrators asynchronous (setAsynchronous), `this` folds the batches of its NEXT call after everything
  ! `previous` has enqueued so far, while the two integrators' tracing kernels overlap (mcbrat_chain_after, include/mcbrat.h)
  subroutine chainAfter(this, previous, ierr)
    type(integrator), intent(inout) :: this, previous
    integer, intent(out) :: ierr
    ierr = mcbrat_chain_after(this%ctx, previous%ctx)
  end subroutine chainAfter
  real function lastTraceMilliseconds(this)
    type(integrator), intent(in) :: this
    lastTraceMilliseconds = mcbrat_last_trace_ms(this%ctx)
  end function lastTraceMilliseconds
  !------------------------------------------------------------------------------------------
  subroutine inverseTableLegendre(coefficients, table, ierr)   ! computeInversePhaseFunction
    real, dimension(:), intent(in)  :: coefficients
    real, dimension(:), intent(out) :: table
    integer,            intent(out) :: ierr
    ierr = mcbrat_inverse_table_legendre(int(size(coefficients), c_int32_t), coefficients, &
                                         int(size(table), c_int32_t), table)
  end subroutine inverseTableLegendre
  !------------------------------------------------------------------------------------------
  ! The backward camera (include/mcbrat.h: mcbrat_render_camera): numBatches batches of samplesPerPixel paths per pixel for the
  ! domain and the Directional solar source the integrator holds (the forward tables must have been set: setForwardTable).
  ! radiance(npx, npy) is the mean of the batch means, radianceStdErr its standard error; numDropped the paths a loop bound ended.
  subroutine renderCamera(this, cam, seed, firstSample, samplesPerPixel, numBatches, radiance, radianceStdErr, numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(camera), intent(in) :: cam
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerPixel
    integer, intent(in) :: numBatches
    real, dimension(:, :), contiguous, target, intent(out) :: radiance
    real, dimension(:, :), contiguous, optional, target, intent(out) :: radianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (any(shape(radiance) /= (/ cam%npx, cam%npy /))) return
    pErr = c_null_ptr
    if (present(radianceStdErr)) then
      if (any(shape(radianceStdErr) /= (/ cam%npx, cam%npy /))) return
      pErr = c_loc(radianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_camera(this%ctx, cam, seed, firstSample, samplesPerPixel, int(numBatches, c_int32_t), c_loc(radiance), &
                                pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderCamera

  ! The radiance by photon path length (include/mcbrat.h: mcbrat_render_camera_pathlengths): renderCamera's paths, every estimate in
  ! the bin of its path length.  pathEdges: the bins' lower edges (the first 0, ascending, at most 256; the last bin is open
  ! above); radiance(npx, npy, size(pathEdges)) sums over its last dimension to renderCamera's image.
  subroutine renderCameraPathLengths(this, cam, pathEdges, seed, firstSample, samplesPerPixel, numBatches, radiance, radianceStdErr, &
                                     numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(camera), intent(in) :: cam
    real, dimension(:), contiguous, intent(in) :: pathEdges
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerPixel
    integer, intent(in) :: numBatches
    real, dimension(:, :, :), contiguous, target, intent(out) :: radiance
    real, dimension(:, :, :), contiguous, optional, target, intent(out) :: radianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (size(pathEdges) < 1) return
    if (any(shape(radiance) /= (/ cam%npx, cam%npy, size(pathEdges) /))) return
    pErr = c_null_ptr
    if (present(radianceStdErr)) then
      if (any(shape(radianceStdErr) /= (/ cam%npx, cam%npy, size(pathEdges) /))) return
      pErr = c_loc(radianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_camera_pathlengths(this%ctx, cam, int(size(pathEdges), c_int32_t), pathEdges, seed, firstSample, &
                                            samplesPerPixel, int(numBatches, c_int32_t), c_loc(radiance), pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderCameraPathLengths

  ! Backward sensors (include/mcbrat.h: mcbrat_render_sensors): numBatches batches of samplesPerSensor paths per sensor for the
  ! domain and the Directional solar source the integrator holds (the forward tables must have been set: setForwardTable).
  ! diffuse + direct is the irradiance of a planar sensor, the actinic flux of a spherical one; totalStdErr the standard error
  ! of that sum; numDropped the paths a loop bound ended.
  subroutine renderSensors(this, sensors, seed, firstSample, samplesPerSensor, numBatches, diffuse, direct, totalStdErr, &
                           numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(sensor), dimension(:), contiguous, intent(in) :: sensors
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerSensor
    integer, intent(in) :: numBatches
    real, dimension(:), contiguous, intent(out) :: diffuse, direct
    real, dimension(:), contiguous, optional, target, intent(out) :: totalStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (size(diffuse) /= size(sensors) .or. size(direct) /= size(sensors)) return
    pErr = c_null_ptr
    if (present(totalStdErr)) then
      if (size(totalStdErr) /= size(sensors)) return
      pErr = c_loc(totalStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_sensors(this%ctx, int(size(sensors), c_int64_t), sensors, seed, firstSample, samplesPerSensor, &
                                 int(numBatches, c_int32_t), -1_c_int32_t, diffuse, direct, c_null_ptr, c_null_ptr, pErr, &
                                 c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderSensors

  ! The emission renders (include/mcbrat.h: mcbrat_render_camera_emission, mcbrat_render_sensors_emission): the emitted (thermal)
  ! radiance at a camera and irradiance at sensors, for the domain the integrator holds (its source is not consulted) and the
  ! caller's Planck radiances cellSource(nx, ny, nz), surfaceSource(nx, ny); results in the sources' units.
  subroutine renderCameraEmission(this, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, numBatches, radiance, &
                                  radianceStdErr, numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(camera), intent(in) :: cam
    real, dimension(:, :, :), contiguous, intent(in) :: cellSource
    real, dimension(:, :), contiguous, intent(in) :: surfaceSource
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerPixel
    integer, intent(in) :: numBatches
    real, dimension(:, :), contiguous, target, intent(out) :: radiance
    real, dimension(:, :), contiguous, optional, target, intent(out) :: radianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (any(shape(radiance) /= (/ cam%npx, cam%npy /))) return
    if (any(shape(cellSource) /= (/ this%numX, this%numY, this%numZ /)) .or. any(shape(surfaceSource) /= (/ this%numX, this%numY /))) return
    pErr = c_null_ptr
    if (present(radianceStdErr)) then
      if (any(shape(radianceStdErr) /= (/ cam%npx, cam%npy /))) return
      pErr = c_loc(radianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_camera_emission(this%ctx, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, &
                                         int(numBatches, c_int32_t), c_loc(radiance), pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderCameraEmission

  subroutine renderSensorsEmission(this, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, numBatches, &
                                   irradiance, irradianceStdErr, numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(sensor), dimension(:), contiguous, intent(in) :: sensors
    real, dimension(:, :, :), contiguous, intent(in) :: cellSource
    real, dimension(:, :), contiguous, intent(in) :: surfaceSource
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerSensor
    integer, intent(in) :: numBatches
    real, dimension(:), contiguous, intent(out) :: irradiance
    real, dimension(:), contiguous, optional, target, intent(out) :: irradianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (size(irradiance) /= size(sensors)) return
    if (any(shape(cellSource) /= (/ this%numX, this%numY, this%numZ /)) .or. any(shape(surfaceSource) /= (/ this%numX, this%numY /))) return
    pErr = c_null_ptr
    if (present(irradianceStdErr)) then
      if (size(irradianceStdErr) /= size(sensors)) return
      pErr = c_loc(irradianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_sensors_emission(this%ctx, int(size(sensors), c_int64_t), sensors, cellSource, surfaceSource, seed, &
                                          firstSample, samplesPerSensor, int(numBatches, c_int32_t), -1_c_int32_t, irradiance, &
                                          pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderSensorsEmission

  ! The emission renders with the expected-value estimator (include/mcbrat.h: mcbrat_render_camera_emission_expected,
  ! mcbrat_render_sensors_emission_expected): the arguments of renderCameraEmission and renderSensorsEmission, the same paths;
  ! every leg deposits the emission along its whole ray, collisions and surface hits deposit nothing.
  subroutine renderCameraEmissionExpected(this, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, numBatches, radiance, &
                                  radianceStdErr, numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(camera), intent(in) :: cam
    real, dimension(:, :, :), contiguous, intent(in) :: cellSource
    real, dimension(:, :), contiguous, intent(in) :: surfaceSource
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerPixel
    integer, intent(in) :: numBatches
    real, dimension(:, :), contiguous, target, intent(out) :: radiance
    real, dimension(:, :), contiguous, optional, target, intent(out) :: radianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (any(shape(radiance) /= (/ cam%npx, cam%npy /))) return
    if (any(shape(cellSource) /= (/ this%numX, this%numY, this%numZ /)) .or. any(shape(surfaceSource) /= (/ this%numX, this%numY /))) return
    pErr = c_null_ptr
    if (present(radianceStdErr)) then
      if (any(shape(radianceStdErr) /= (/ cam%npx, cam%npy /))) return
      pErr = c_loc(radianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_camera_emission_expected(this%ctx, cam, cellSource, surfaceSource, seed, firstSample, samplesPerPixel, &
                                         int(numBatches, c_int32_t), c_loc(radiance), pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderCameraEmissionExpected

  subroutine renderSensorsEmissionExpected(this, sensors, cellSource, surfaceSource, seed, firstSample, samplesPerSensor, numBatches, &
                                   irradiance, irradianceStdErr, numDropped, ierr)
    type(integrator), intent(inout) :: this
    type(sensor), dimension(:), contiguous, intent(in) :: sensors
    real, dimension(:, :, :), contiguous, intent(in) :: cellSource
    real, dimension(:, :), contiguous, intent(in) :: surfaceSource
    integer(c_int64_t), intent(in) :: seed, firstSample, samplesPerSensor
    integer, intent(in) :: numBatches
    real, dimension(:), contiguous, intent(out) :: irradiance
    real, dimension(:), contiguous, optional, target, intent(out) :: irradianceStdErr
    integer(c_int64_t), optional, intent(out) :: numDropped
    integer, intent(out) :: ierr
    type(c_ptr) :: pErr
    integer(c_int64_t) :: dropped
    ierr = 1
    if (size(irradiance) /= size(sensors)) return
    if (any(shape(cellSource) /= (/ this%numX, this%numY, this%numZ /)) .or. any(shape(surfaceSource) /= (/ this%numX, this%numY /))) return
    pErr = c_null_ptr
    if (present(irradianceStdErr)) then
      if (size(irradianceStdErr) /= size(sensors)) return
      pErr = c_loc(irradianceStdErr)
    end if
    dropped = 0
    ierr = mcbrat_render_sensors_emission_expected(this%ctx, int(size(sensors), c_int64_t), sensors, cellSource, surfaceSource, seed, &
                                          firstSample, samplesPerSensor, int(numBatches, c_int32_t), -1_c_int32_t, irradiance, &
                                          pErr, c_null_ptr, dropped)
    if (present(numDropped)) numDropped = dropped
  end subroutine renderSensorsEmissionExpected

  ! exp(-optical depth) from each point xyz(3, n) toward the sun up to the top of the domain (mcbrat_sun_transmittance)
  subroutine sunTransmittance(this, xyz, transmittance, ierr)
    type(integrator), intent(inout) :: this
    real(c_double), dimension(:, :), contiguous, intent(in) :: xyz
    real, dimension(:), contiguous, intent(out) :: transmittance
    integer, intent(out) :: ierr
    ierr = 1
    if (size(xyz, 1) /= 3 .or. size(xyz, 2) /= size(transmittance)) return
    ierr = mcbrat_sun_transmittance(this%ctx, int(size(transmittance), c_int64_t), xyz, transmittance)
  end subroutine sunTransmittance

end module mcbrat_hip_integrator
