"""The integrator: host-side mirror of module monteCarloRadiativeTransfer
(Integrators/monteCarloRadiativeTransfer.f95, public list :121-123) over the C ABI.

    new_Integrator(domain)                    :129-201
    specifyParameters(...)                    :1046-1484
    computeRadiativeTransfer(...)             :209-391  (photon loop computeRT :393-841 on the GPU)
    reportResults(...)                        :845-1042
    finalize_Integrator                       :1486-1547

Failures raise McbratError with the message the reference would push on its
ErrorMessage stack; there is no CPU path."""
import ctypes as C

import numpy as np

from ._capi import Counters, FATE_DTYPE, McbratError, check, lib, ptr

defaultMinInverseTableSize = 9001  # :24-25
defaultMinForwardTableSize = 9001
defaultHybridPhaseFunWidth, maxHybridPhaseFunWidth = 7.0, 30.0  # :26-27
defaultZetaMin = 0.3  # :29

# the solar forms of new_PhotonStream: the stream's attributes each one passes, in order, and the C function that sets it
_SOLAR_ARGS = {"Directional": ("solarMu", "solarAzimuth"), "RandomAzimuth": ("solarMu",), "Flux": (),
               "Spotlight": ("solarMu", "solarAzimuth", "solarX", "solarY")}
_SOLAR_SETTERS = {"Directional": "mcbrat_set_source_solar", "RandomAzimuth": "mcbrat_set_source_random_azimuth",
                  "Flux": "mcbrat_set_source_flux", "Spotlight": "mcbrat_set_source_spotlight"}


# The recording settings in dependency order -- a row needs, if anything, rows above it: the integrator's field, its off value
# and the C setter that takes it
_RECORDING = {"numRecScatOrd": (-1, "mcbrat_specify_scattering_orders"),
              "recLevelFluxes": (False, "mcbrat_specify_level_fluxes"),
              "recDirectLevelFluxes": (False, "mcbrat_specify_direct_level_fluxes"),
              "recActinicFlux": (False, "mcbrat_specify_actinic_flux"),
              "recSideFluxes": (False, "mcbrat_specify_side_fluxes")}
# the fields mcbrat_settings_refusal is asked about, beside the surface
_ASKED_ABOUT = frozenset(_RECORDING) | {"intensityMus", "computeIntensity", "limitIntensityContributions"}


def _push_order(held, wanted, intensityChanged, surfaceGiven):
    """The calls that bring the library from the recording settings it holds to the wanted ones, in an order in which its
    setters, which refuse one at a time, refuse none of them where the wanted settings as a whole are acceptable (DESIGN.md
    section 4.16): the settings that go off, dependents first; "surface"; "intensity"; every other changed setting."""
    changed = [name for name in _RECORDING if wanted[name] != held[name]]
    off = [name for name in changed if wanted[name] == _RECORDING[name][0]]
    return off[::-1] + ["surface"] * bool(surfaceGiven) + ["intensity"] * bool(intensityChanged) + [name for name in changed if name not in off]


class RandomNumberSequence:
    """Stands where the reference passes type(randomNumberSequence): the Philox key and the
    id of the next photon.  Photon ids, not generator state, carry the stream, so any split
    of a run over GPUs or batches reproduces the same photons."""

    def __init__(self, seed=10, firstPhotonId=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.nextPhotonId = int(firstPhotonId)


# the four side-flux quantities in the order of the library's parts
SIDE_FLUX_NAMES = ("sideFluxXPlus", "sideFluxXMinus", "sideFluxYPlus", "sideFluxYMinus")


def new_RandomNumberSequence(seed=10, firstPhotonId=0):
    if not np.isscalar(seed):  # (/ iseed, thisProc, thisThread /), monteCarloDriver.f95:901
        s = [int(x) & 0xFFFFFFFF for x in seed]
        seed = s[0] | ((s[1] if len(s) > 1 else 0) << 32)
        seed ^= (s[2] if len(s) > 2 else 0) << 48
    return RandomNumberSequence(seed, firstPhotonId)


class Integrator:
    def __init__(self, atmosphere, device=0):
        """new_Integrator(atmosphere, status)."""
        self._lib = lib()
        self._ctx = self._lib.mcbrat_create(int(device))
        if not self._ctx:
            raise McbratError("new_Integrator: no usable HIP device %d (the MI355X library has no CPU fallback)" % device)
        self.device = int(device)
        self._atmosphere = atmosphere
        self.useSurfaceBDRF = False
        self.surfaceBDRF = None
        self.minInverseTableSize = defaultMinInverseTableSize
        self.useRayTracing = True
        self.useRussianRoulette = True
        self.LW_flag = -1.0
        # radiance by local estimation (:72-97)
        self.computeIntensity = False
        self.intensityMus = np.zeros(0, np.float32)
        self.intensityPhis = np.zeros(0, np.float32)
        self.minForwardTableSize = defaultMinForwardTableSize
        self.useHybridPhaseFunsForIntenCalcs = False
        self.hybridPhaseFunWidth = defaultHybridPhaseFunWidth
        self.numOrdersOrigPhaseFunIntenCalcs = 0
        self.useRussianRouletteForIntensity = False
        self.zetaMin = defaultZetaMin
        self.limitIntensityContributions = False
        self.maxIntensityContribution = float(np.finfo(np.float32).max)
        # fluxes and radiances by scattering order (:1159-1171, :1293-1330): highest order recorded, -1 off
        self.recScatOrd = False
        self.numRecScatOrd = -1
        # upward and downward flux through every level of every column
        self.recLevelFluxes = False
        # the direct beam apart from the diffuse light in the downward level flux; needs recLevelFluxes
        self.recDirectLevelFluxes = False
        # the actinic flux of every cell by track length; solar sources, with or without recLevelFluxes
        self.recActinicFlux = False
        # the flux through the vertical faces of every cell; solar sources, needs recLevelFluxes
        self.recSideFluxes = False
        self._held = {name: off for name, (off, _) in _RECORDING.items()}  # the recording settings the library holds
        self._param_token = None
        self._intensity_token = None
        self._domain_token = None
        self._source_token = None
        self._loaded_domain = None   # strong references: what the device buffers were filled from
        self._loaded_weights = None
        self._dims = None
        self._load_grid(atmosphere)
        self.readyToCompute = True

    # -- life cycle -----------------------------------------------------------------
    def finalize(self):
        if getattr(self, "_ctx", None):
            self._lib.mcbrat_destroy(self._ctx)
            self._ctx = None
        self.readyToCompute = False

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def isReady_Integrator(self):
        return bool(self.readyToCompute)

    def copy_Integrator(self):
        """copy_Integrator (:1296-1376): a second integrator on the same domain with the same parameters.  The
        reference also copies the last batch's results; here results live in the context that computed them."""
        new = Integrator(self._atmosphere, self.device)
        new.specifyParameters(minInverseTableSize=self.minInverseTableSize, useRayTracing=self.useRayTracing,
                              useRussianRoulette=self.useRussianRoulette, LW_flag=self.LW_flag,
                              intensityMus=self.intensityMus, intensityPhis=self.intensityPhis,
                              computeIntensity=self.computeIntensity, minForwardTableSize=self.minForwardTableSize,
                              useRussianRouletteForIntensity=self.useRussianRouletteForIntensity, zetaMin=self.zetaMin,
                              useHybridPhaseFunsForIntenCalcs=self.useHybridPhaseFunsForIntenCalcs,
                              hybridPhaseFunWidth=self.hybridPhaseFunWidth,
                              numOrdersOrigPhaseFunIntenCalcs=self.numOrdersOrigPhaseFunIntenCalcs,
                              limitIntensityContributions=self.limitIntensityContributions,
                              maxIntensityContribution=self.maxIntensityContribution, surfaceBDRF=self.surfaceBDRF,
                              numRecScatOrd=self.numRecScatOrd, recLevelFluxes=self.recLevelFluxes,
                              recDirectLevelFluxes=self.recDirectLevelFluxes, recActinicFlux=self.recActinicFlux,
                              recSideFluxes=self.recSideFluxes)
        return new

    def _check(self, rc):
        check(self._ctx, rc)

    def _load_grid(self, dom):
        info = dom.getInfo_Domain()
        self._check(self._lib.mcbrat_set_grid(self._ctx, info["numX"], info["numY"], info["numZ"],
                                              ptr(info["xPosition"]), ptr(info["yPosition"]), ptr(info["zPosition"])))
        self._dims = (info["numX"], info["numY"], info["numZ"])
        self._domain_token = None
        self._source_token = None

    # -- specifyParameters ------------------------------------------------------------
    def specifyParameters(self, minInverseTableSize=None, useRayTracing=None, useRussianRoulette=None, LW_flag=None,
                          computeIntensity=None, intensityMus=None, intensityPhis=None, minForwardTableSize=None,
                          useRussianRouletteForIntensity=None, zetaMin=None, useHybridPhaseFunsForIntenCalcs=None,
                          hybridPhaseFunWidth=None, numOrdersOrigPhaseFunIntenCalcs=None,
                          limitIntensityContributions=None, maxIntensityContribution=None, surfaceBDRF=None,
                          recScatOrd=None, numRecScatOrd=None, recLevelFluxes=None, recDirectLevelFluxes=None, recActinicFlux=None,
                          recSideFluxes=None, **unsupported):
        # What the fields would become is worked out first and kept only when nothing has refused it, so that a refused call
        # leaves the integrator as it was.  What may not be combined is the library's to say (mcbrat_settings_refusal).
        new = {}
        want = lambda name: new.get(name, getattr(self, name))  # noqa: E731
        for k, v in unsupported.items():
            if v not in (None, False):
                raise McbratError("specifyParameters: keyword %s is not supported by the MI355X integrator" % k)
        if minInverseTableSize is not None:  # :1103-1106, :1183-1184 (smaller values are ignored)
            new["minInverseTableSize"] = max(int(minInverseTableSize), defaultMinInverseTableSize)
        if useRayTracing is not None:
            new["useRayTracing"] = bool(useRayTracing)
        if useRussianRoulette is not None:
            new["useRussianRoulette"] = bool(useRussianRoulette)
        if LW_flag is not None:
            new["LW_flag"] = float(LW_flag)
        # intensity keywords, :1130-1160 and :1186-1283
        if (intensityMus is None) != (intensityPhis is None):
            raise McbratError("specifyParameters: Both or neither of intensityMus, intensityPhis must be supplied")
        if intensityMus is not None:
            mus = np.ascontiguousarray(intensityMus, np.float32).reshape(-1)
            phis = np.ascontiguousarray(intensityPhis, np.float32).reshape(-1)
            if mus.size != phis.size:
                raise McbratError("specifyParameters: intensityMus, intensityPhis must be the same length")
            new.update(intensityMus=mus, intensityPhis=phis, computeIntensity=mus.size > 0)
        if computeIntensity is not None:
            if computeIntensity and want("intensityMus").size == 0:
                raise McbratError("specifyParameters: Can't compute intensity without specifying directions.")
            if not computeIntensity and intensityMus is None:
                new["computeIntensity"] = False
        if minForwardTableSize is not None:
            new["minForwardTableSize"] = max(int(minForwardTableSize), defaultMinForwardTableSize)
        if useRussianRouletteForIntensity is not None:
            new["useRussianRouletteForIntensity"] = bool(useRussianRouletteForIntensity)
        if zetaMin is not None and zetaMin >= 0.0:  # :1194-1201 (a negative value is ignored with a warning)
            new["zetaMin"] = float(zetaMin)
        if useHybridPhaseFunsForIntenCalcs is not None:
            new["useHybridPhaseFunsForIntenCalcs"] = bool(useHybridPhaseFunsForIntenCalcs)
        if hybridPhaseFunWidth is not None:  # :1108-1114, :1209-1215
            if hybridPhaseFunWidth > maxHybridPhaseFunWidth or hybridPhaseFunWidth < 0.0:
                raise McbratError("specifyParameters: hybridPhaseFunWidth out of range (0 to 30degrees).")
            new["hybridPhaseFunWidth"] = float(hybridPhaseFunWidth) if 0 < hybridPhaseFunWidth < maxHybridPhaseFunWidth \
                else defaultHybridPhaseFunWidth
        if numOrdersOrigPhaseFunIntenCalcs is not None:
            if numOrdersOrigPhaseFunIntenCalcs < 0:
                raise McbratError("specifyParameters: numOrdersOrigPhaseFunIntenCalcs must be >= 0")
            new["numOrdersOrigPhaseFunIntenCalcs"] = int(numOrdersOrigPhaseFunIntenCalcs)
        if limitIntensityContributions is not None:
            new["limitIntensityContributions"] = bool(limitIntensityContributions)
        if maxIntensityContribution is not None and maxIntensityContribution > 0.0:
            new["maxIntensityContribution"] = float(maxIntensityContribution)
        # scattering orders (:1159-1171): recScatOrd=True needs numRecScatOrd; numRecScatOrd decides when given (< 0: off)
        if recScatOrd and numRecScatOrd is None:
            raise McbratError("specifyParameters: set recScatOrd to true, but did not provide number of orders to track.")
        if numRecScatOrd is not None or (recScatOrd is not None and not recScatOrd):
            orders = -1 if numRecScatOrd is None or int(numRecScatOrd) < 0 else int(numRecScatOrd)
            new.update(numRecScatOrd=orders, recScatOrd=orders >= 0)
        # the tallies (DESIGN.md sections 4.12 to 4.15)
        if recLevelFluxes is not None:
            new["recLevelFluxes"] = bool(recLevelFluxes)
        if recDirectLevelFluxes is not None:
            new["recDirectLevelFluxes"] = bool(recDirectLevelFluxes)
        if recActinicFlux is not None:
            new["recActinicFlux"] = bool(recActinicFlux)
        if recSideFluxes is not None:
            new["recSideFluxes"] = bool(recSideFluxes)
        if surfaceBDRF is not None:  # :1091-1094, :1173-1176
            if not (hasattr(surfaceBDRF, "isReady_surfaceDescription") and surfaceBDRF.isReady_surfaceDescription()):
                raise McbratError("specifyParameters: surface description isn't valid.")
        # one question to the library, when this call sets something the question is about (a library of an A/B run may lack it:
        # the push refuses then)
        question = (surfaceBDRF is not None or not new.keys().isdisjoint(_ASKED_ABOUT)) and getattr(self._lib, "mcbrat_settings_refusal", None)
        if question:
            surface = surfaceBDRF if surfaceBDRF is not None else self.surfaceBDRF
            refused = question(self._ctx, int(want("intensityMus").size) if want("computeIntensity") else 0,
                               int(want("limitIntensityContributions")), *(int(want(name)) for name in _RECORDING),
                               int(getattr(surface, "kind", 0) != 0))
            if refused:
                raise McbratError(refused.decode())
        for name, value in new.items():
            setattr(self, name, value)
        if not new.keys().isdisjoint(("minInverseTableSize", "minForwardTableSize", "useHybridPhaseFunsForIntenCalcs", "hybridPhaseFunWidth")):
            self._domain_token = None  # (the tables depend on them)
        self._push_parameters(surfaceBDRF)

    def _push_parameters(self, surface=None):
        # (what the library holds is remembered by content: a step of a small domain is two milliseconds, and the host side
        # of a call is part of it)
        token = (self.useRayTracing, self.useRussianRoulette, self.LW_flag)
        if token != self._param_token:
            self._check(self._lib.mcbrat_specify_parameters(self._ctx, int(self.useRayTracing),
                                                            int(self.useRussianRoulette), C.c_float(self.LW_flag)))
            self._param_token = token
        n = int(self.intensityMus.size) if self.computeIntensity else 0
        intensity = (n, self.intensityMus.tobytes(), self.intensityPhis.tobytes(), self.useRussianRouletteForIntensity, self.zetaMin,
                     self.useHybridPhaseFunsForIntenCalcs, self.numOrdersOrigPhaseFunIntenCalcs, self.limitIntensityContributions,
                     self.maxIntensityContribution)
        wanted = {name: getattr(self, name) for name in _RECORDING}
        if wanted == self._held and intensity == self._intensity_token and surface is None:
            return
        for step in _push_order(self._held, wanted, intensity != self._intensity_token, surface is not None):
            if step == "surface":
                self._push_surface(surface)
            elif step == "intensity":
                self._check(self._lib.mcbrat_specify_intensity(
                    self._ctx, n, ptr(self.intensityMus) if n else None, ptr(self.intensityPhis) if n else None,
                    int(self.useRussianRouletteForIntensity), C.c_float(self.zetaMin), int(self.useHybridPhaseFunsForIntenCalcs),
                    int(self.numOrdersOrigPhaseFunIntenCalcs), int(self.limitIntensityContributions),
                    C.c_float(self.maxIntensityContribution)))
                self._intensity_token = intensity
                self._domain_token = None  # forward tables go with the optics
            else:
                self._check(getattr(self._lib, _RECORDING[step][1])(self._ctx, int(wanted[step])))
                self._held[step] = wanted[step]

    def _push_surface(self, surface):
        x, y = surface.xPosition, surface.yPosition
        kind = getattr(surface, "kind", 0)
        if kind == 0:
            refl = np.ascontiguousarray(surface.BRDFParameters[0].T, np.float32)  # x fastest
            self._check(self._lib.mcbrat_set_surface_description(self._ctx, int(x.size), int(y.size), ptr(x), ptr(y), ptr(refl)))
        else:  # RPV, Ross-Li, Cox-Munk: [nParams][numY-1][numX-1], x fastest
            q = np.ascontiguousarray(np.transpose(surface.BRDFParameters, (0, 2, 1)), np.float32)
            self._check(self._lib.mcbrat_set_surface_brdf(self._ctx, int(kind), int(x.size), int(y.size), ptr(x), ptr(y),
                                                          int(q.shape[0]), ptr(q)))
        self.useSurfaceBDRF = True
        self.surfaceBDRF = surface

    def numIntensityDirections(self):
        return int(self.intensityMus.size) if self.computeIntensity else 0

    def setTuning(self, blocksPerCU=-1, eventThreshold=0, maxBatchesInFlight=-1, privateTallies=-1, blockSize=-1,
                  launchThreshold=0, surfaceThreshold=0, brickLayout=-1, layerSkip=-1, blockWalk=-1):
        self._check(self._lib.mcbrat_set_tuning(self._ctx, blocksPerCU, eventThreshold, maxBatchesInFlight,
                                                privateTallies, blockSize, launchThreshold, surfaceThreshold, brickLayout))
        if layerSkip >= 0 or blockWalk >= 0:
            self._check(self._lib.mcbrat_set_walk_options(self._ctx, int(layerSkip), int(blockWalk)))

    def setOption(self, **options):
        """Scheduling options by name (include/mcbrat.h: mcbrat_set_option), e.g. jumpThreshold=16."""
        for name, value in options.items():
            self._check(self._lib.mcbrat_set_option(self._ctx, name.encode(), int(value)))

    def walkMode(self):
        """The walk a flux run of the loaded domain uses (decided by the library's launch plan, mcbrat_get_walk_mode)."""
        m = int(self._lib.mcbrat_get_walk_mode(self._ctx))
        return {"layerSkip": bool(m & 1), "blockWalk": bool(m & 2), "clearAirFlight": bool(m & 4),
                # tallies private to a workgroup in LDS; the wide plan: one workgroup of 1024 lanes per compute unit owns its LDS;
                # the block walk with the per-cell optics left in global memory (extinction per block in LDS)
                "privateTallies": bool(m & 64), "widePlan": bool(m & 16), "opticsInGlobalMemory": bool(m & 32),
                "opticsPerBlock": bool(m & 128), "emissionCdfTopInLds": bool(m & 256),
                # the block walk's instantiation without periodic folds inside blocks (no block of the medium spans a periodic axis)
                "foldsCompiledOut": bool(m & 512),
                # ... with a black surface and the parallel sun compiled into its exit and launch phases (albedo 0, no surface
                # description, finite single-scattering albedos, the Directional source; option blockRareKernel=1 keeps the general one)
                "blackSurfaceSunCompiledIn": bool(m & 1024)}

    def badPhotons(self):
        """Photons dropped by a loop bound of the kernels since this integrator was created (the reference's nBad, :562-563)."""
        return self.counters()["badPhotons"]

    def firstDrop(self):
        """What a loop bound dropped first since this integrator was created (which bound, photon id, state, cell, direction);
        "" while badPhotons() is 0."""
        msg = self._lib.mcbrat_first_drop(self._ctx)
        return msg.decode() if msg else ""

    def eventThreshold(self):
        return int(self._lib.mcbrat_get_event_threshold(self._ctx))

    def setAsync(self, enable=True, _chained=False):
        """Let consecutive computeRadiativeTransfer / resetMoments calls overlap on the GPU (include/mcbrat.h)."""
        if enable and getattr(self, "_shares_moments", False) and not _chained:
            raise McbratError("setAsync: this integrator accumulates into a moment array it shares with other integrators "
                              "(SpectralRun); their finish kernels are only ordered in synchronous mode, or by chainAfter")
        self._check(self._lib.mcbrat_set_async(self._ctx, int(bool(enable))))

    def chainAfter(self, previous):
        """The finish kernels of this integrator's next call follow everything `previous` (an integrator that accumulates
        into the same moment array) has enqueued so far (mcbrat_chain_after)."""
        self._check(self._lib.mcbrat_chain_after(self._ctx, previous._ctx))

    def synchronize(self):
        self._check(self._lib.mcbrat_synchronize(self._ctx))

    def streamWaitDone(self, hip_stream):
        """Make a caller's HIP stream (raw handle, e.g. torch.cuda.current_stream().cuda_stream) wait for the work enqueued so far."""
        self._check(self._lib.mcbrat_stream_wait_done(self._ctx, C.c_void_p(hip_stream)))

    def waitStream(self, hip_stream):
        """Make the next write to the moments wait for what the caller's HIP stream has enqueued so far."""
        self._check(self._lib.mcbrat_wait_stream(self._ctx, C.c_void_p(hip_stream)))

    # -- computeRadiativeTransfer -------------------------------------------------------
    def _load_domain(self, dom):
        # What is on the device is remembered by CONTENT, never by object identity (CPython reuses the ids of freed
        # objects): a strong reference to the domain, its version counter (addOpticalComponent and the albedo setter
        # bump it) and the parameters the tables depend on.
        token = (dom._version, self.minInverseTableSize, self.numIntensityDirections() > 0,
                 self.minForwardTableSize, self.useHybridPhaseFunsForIntenCalcs, self.hybridPhaseFunWidth)
        if dom is self._loaded_domain and token == self._domain_token:
            return
        info = dom.getInfo_Domain()  # (expands the component arrays if they are stale)
        token = (dom._version,) + token[1:]
        if (info["numX"], info["numY"], info["numZ"]) != self._dims:
            raise McbratError("computeRadiativeTransfer: domain does not match the integrator's grid")
        nc = info["numberOfComponents"]
        tot = np.ascontiguousarray(info["totalExt"], np.float64).reshape(-1)
        cum = np.ascontiguousarray(info["cumExt"], np.float64).reshape(-1)
        ssa = np.ascontiguousarray(info["ssa"], np.float64).reshape(-1)
        pfi = np.ascontiguousarray(info["phaseFuncI"], np.int32).reshape(-1)
        self._check(self._lib.mcbrat_set_optics(self._ctx, nc, ptr(tot), ptr(cum), ptr(ssa), ptr(pfi), info["albedo"]))
        tables = dom.tabulateInversePhaseFunctions(self.minInverseTableSize)  # :280
        for c, t in enumerate(tables):
            t = np.ascontiguousarray(t, np.float32)
            self._check(self._lib.mcbrat_set_inverse_table(self._ctx, c + 1, t.shape[1], t.shape[0], ptr(t)))
        if self.numIntensityDirections() > 0:  # :281-285 forward tables only when intensity is computed
            tab, orig = dom.tabulateForwardPhaseFunctions(self.minForwardTableSize, self.useHybridPhaseFunsForIntenCalcs,
                                                          self.hybridPhaseFunWidth)
            for c, (t, o) in enumerate(zip(tab, orig)):
                t = np.ascontiguousarray(t, np.float32)
                o = np.ascontiguousarray(o, np.float32)
                self._check(self._lib.mcbrat_set_forward_table(self._ctx, c + 1, t.shape[1], t.shape[0], ptr(t),
                                                               ptr(o) if self.useHybridPhaseFunsForIntenCalcs else None))
        self._loaded_domain = dom
        self._domain_token = token
        self._source_token = None
        self._loaded_weights = None

    def _load_source(self, photons):
        kind = photons.kind
        if kind == "BBEmission":  # strong reference to the weights + their version (emission_weighting bumps it)
            token = ("BBEmission", photons.weights._version, float(photons.weights.fracAtmsPower))
            if photons.weights is not self._loaded_weights:
                self._source_token = None
        else:  # the solar kinds: the kind and its geometry are the token
            token = (kind,) + tuple(float(getattr(photons, a)) for a in _SOLAR_ARGS[kind])
        if token == self._source_token:
            return
        if kind == "BBEmission":
            self._check(self._lib.mcbrat_set_source_emission(self._ctx, ptr(photons.weights.voxelWeights),
                                                             photons.weights.fracAtmsPower))
            self._loaded_weights = photons.weights
        else:
            setter = getattr(self._lib, _SOLAR_SETTERS[kind])
            self._check(setter(self._ctx, *(C.c_float(v) for v in token[1:])))
        self._source_token = token

    def prepare(self, thisDomain, incomingPhotons):
        """Everything computeRadiativeTransfer would upload for this domain and source -- optical grids, inverse (and
        forward) tables, emission CDF -- now, so that later calls with the same objects trace without touching the host
        data again (spectrally integrated runs keep one prepared integrator per wavelength)."""
        self.specifyParameters()
        self._load_domain(thisDomain)
        self._load_source(incomingPhotons)

    def computeRadiativeTransfer(self, thisDomain, randomNumbers, incomingPhotons, numPhotonsPerBatch, numBatches=1):
        """Traces numBatches batches of numPhotonsPerBatch photons (the reference call is
        numBatches = 1).  Returns numPhotonsProcessed.  reportResults() then returns the
        LAST batch, and the moment arrays hold every batch (see moments())."""
        if not self.readyToCompute:
            raise McbratError("computeRadiativeTransfer: problem not completely specified.")
        n = min(int(numPhotonsPerBatch), incomingPhotons.numberOfPhotons - incomingPhotons.currentPhoton + 1) \
            if numBatches == 1 else int(numPhotonsPerBatch)
        if n < 1:
            raise McbratError("computeRadiativeTransfer: Didn't process any photons.")
        self._push_parameters()  # push current flags
        self._load_domain(thisDomain)
        self._load_source(incomingPhotons)
        done = C.c_int64(0)
        self._check(self._lib.mcbrat_compute_radiative_transfer(self._ctx, randomNumbers.seed, randomNumbers.nextPhotonId,
                                                                n, int(numBatches), C.byref(done)))
        randomNumbers.nextPhotonId += done.value
        incomingPhotons.currentPhoton += done.value
        return done.value

    # -- the backward camera -----------------------------------------
    def _load_camera_tables(self):
        """The forward tables the camera's local estimates read: pushed for the loaded domain where no intensity
        directions have brought them (_load_domain pushes them only then)."""
        dom = self._loaded_domain
        if dom is None:
            raise McbratError("renderCamera: no domain loaded: call prepare(domain, photons) or computeRadiativeTransfer first.")
        if self.numIntensityDirections() > 0:
            return
        token = (dom._version, self._domain_token, self.minForwardTableSize)
        if token == getattr(self, "_camera_token", None):
            return
        tab, _ = dom.tabulateForwardPhaseFunctions(self.minForwardTableSize, False, self.hybridPhaseFunWidth)
        for c, t in enumerate(tab):
            t = np.ascontiguousarray(t, np.float32)
            self._check(self._lib.mcbrat_set_forward_table(self._ctx, c + 1, t.shape[1], t.shape[0], ptr(t), None))
        self._camera_token = token

    def _render_camera(self, entry, camera, before, seed, firstSample, samplesPerPixel, numBatches, randomNumbers=None, bins=(), **more):
        """One camera-shaped call: entry(ctx, camera, *before, seed, firstSample, samples, batches, radiance, error, batch means,
        dropped) into zeroed arrays [*bins, npy, npx]; the sample indices of randomNumbers, where given, move on."""
        s, nb, shape = camera.struct(), int(numBatches), tuple(bins) + (camera.npy, camera.npx)
        rad, err, means = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros((max(nb, 1),) + shape, np.float32)
        dropped = C.c_int64(0)
        self._check(entry(self._ctx, C.addressof(s), *before, int(seed), int(firstSample), int(samplesPerPixel), nb, ptr(rad), ptr(err), ptr(means),
                          C.addressof(dropped)))
        if randomNumbers is not None:
            randomNumbers.nextPhotonId += int(samplesPerPixel) * nb
        return dict({"radiance": rad, "radiance_StdErr": err, "batchMeans": means}, dropped=int(dropped.value), **more)

    def _render_sensors(self, entry, sensors, before, randomNumbers, samplesPerSensor, numBatches, gridInLds, values, parts=()):
        """One sensor-shaped call: entry(ctx, n, sensors, *before, seed, firstSample, samples, batches, gridInLds, the `values`
        arrays of one float per sensor, batch means, dropped) into zeroed arrays; batch means [numBatches, *parts, n].
        -> (the value arrays, the batch means, dropped); the sample indices of randomNumbers move on."""
        n, nb, arr = len(sensors), int(numBatches), sensors.structs()
        out, means = [np.zeros(n, np.float32) for _ in range(values)], np.zeros((max(nb, 1),) + tuple(parts) + (n,), np.float32)
        dropped = C.c_int64(0)
        self._check(entry(self._ctx, n, C.addressof(arr), *before, randomNumbers.seed, randomNumbers.nextPhotonId, int(samplesPerSensor), nb,
                          int(gridInLds), *[ptr(a) for a in out], ptr(means), C.addressof(dropped)))
        randomNumbers.nextPhotonId += int(samplesPerSensor) * nb
        return out, means, int(dropped.value)

    def renderCamera(self, camera, randomNumbers, samplesPerPixel, numBatches=1):
        """The radiance at `camera` (mcbrat3d_amd.camera.new_Camera) by backward Monte Carlo, numBatches batches of
        samplesPerPixel paths per pixel, for the domain and the Directional solar source this integrator has loaded (prepare,
        computeRadiativeTransfer).  Returns {"radiance", "radiance_StdErr", "batchMeans", "dropped"}: [npy, npx] arrays (batchMeans
        [numBatches, npy, npx]) in units of radiance per unit solar flux through a horizontal plane at the top, and the number of
        paths a loop bound ended.  Sample indices continue from randomNumbers.nextPhotonId; tallies, moments and settings of the
        integrator are left alone."""
        self._load_camera_tables()
        return self._render_camera(self._lib.mcbrat_render_camera, camera, (), randomNumbers.seed, randomNumbers.nextPhotonId, samplesPerPixel,
                                   numBatches, randomNumbers)

    def renderSensors(self, sensors, randomNumbers, samplesPerSensor, numBatches=1, gridInLds=-1):
        """Irradiance (planar sensors) and actinic flux (spherical ones) at `sensors` (mcbrat3d_amd.sensors.new_Sensors) by
        backward Monte Carlo: numBatches batches of samplesPerSensor paths per sensor, for the domain
        and the Directional solar source this integrator has loaded.  Returns arrays of one value per sensor, per unit solar
        flux through a horizontal plane at the top: "irradiance" (= "diffuse" + "direct") with "irradiance_StdErr",
        "diffuse_StdErr", "direct_StdErr" (standard errors of the mean of the batch means), "batchMeans" [numBatches, 2, n]
        (diffuse, direct) and "dropped", the number of paths a loop bound ended.  Sample indices continue from
        randomNumbers.nextPhotonId; tallies, moments and settings of the integrator are left alone."""
        self._load_camera_tables()
        (dif, dirc, eDif, eDir, eTot), means, dropped = self._render_sensors(self._lib.mcbrat_render_sensors, sensors, (), randomNumbers,
                                                                             samplesPerSensor, numBatches, gridInLds, 5, parts=(2,))
        return {"irradiance": dif + dirc, "irradiance_StdErr": eTot, "diffuse": dif, "direct": dirc, "diffuse_StdErr": eDif,
                "direct_StdErr": eDir, "batchMeans": means, "dropped": dropped}

    def renderCameraPathLengths(self, camera, pathEdges, samplesPerPixel, numBatches=1, seed=0, firstSample=0):
        """renderCamera's radiance split by photon path length: the geometric length, in the domain's
        length unit, from where the light enters the domain at its top to the camera.  pathEdges: the bins' LOWER edges, floats,
        pathEdges[0] = 0, strictly ascending, at most 256; the last bin is open above, so the bins sum to renderCamera's image.
        The same (seed, firstSample) walks the paths of renderCamera with new_RandomNumberSequence(seed, firstSample).  Returns {"radiance" [bin, y, x], "radiance_StdErr", "batchMeans"
        [batch, bin, y, x], "pathEdges", "dropped"}; mcbrat3d_amd.camera.absorbed_radiance and mean_path_length read them."""
        self._load_camera_tables()
        edges = np.ascontiguousarray(np.asarray(pathEdges, np.float32).reshape(-1))
        return self._render_camera(self._lib.mcbrat_render_camera_pathlengths, camera, (int(edges.size), ptr(edges)), seed, firstSample, samplesPerPixel,
                                   numBatches, bins=(max(int(edges.size), 1),), pathEdges=edges)

    # -- the emission renders ----------------------------------------
    def prepareDomain(self, thisDomain):
        """What prepare() uploads of the domain -- optical grids and tables -- without a source: all an emission render needs."""
        self.specifyParameters()
        self._load_domain(thisDomain)

    def _emission_sources(self, name, cellSource, surfaceSource):
        if self._loaded_domain is None:
            raise McbratError(name + ": no domain loaded: call prepareDomain(domain), prepare(domain, photons) or "
                              "computeRadiativeTransfer first.")
        if cellSource is None or surfaceSource is None:
            raise McbratError(name + ": cellSource and surfaceSource are needed (mcbrat3d_amd.planck_sources).")
        nx, ny, nz = self._dims
        cell, sfc = np.ascontiguousarray(cellSource, np.float32), np.ascontiguousarray(surfaceSource, np.float32)
        if cell.size != nx * ny * nz or sfc.size != nx * ny:
            raise McbratError(name + ": cellSource must hold numZ x numY x numX values and surfaceSource numY x numX.")
        return cell, sfc

    def _emission_entry(self, name, estimator, collision, expected):
        """The library's entry for `estimator`: "collision"  or "expected" (section 4.24)"""
        if estimator not in ("collision", "expected"):
            raise McbratError(name + ": estimator must be 'collision' or 'expected' (got %r)." % (estimator,))
        return getattr(self._lib, expected if estimator == "expected" else collision)

    def renderCameraEmission(self, camera, randomNumbers, samplesPerPixel, numBatches=1, cellSource=None, surfaceSource=None, estimator="collision"):
        """The emitted (thermal) radiance at `camera` by backward Monte Carlo: renderCamera's paths, which deposit the source
        function where they collide and where they meet the surface instead of looking toward the sun.  cellSource [nz, ny, nx]
        and surfaceSource [ny, nx] are Planck radiances (mcbrat3d_amd.planck_sources); the result has their units.  The loaded
        source is not consulted (none need be loaded: prepareDomain).  Returns what renderCamera returns, and "estimator".
        estimator="expected"  walks the same paths with the expected-value estimator: every leg deposits
        the emission along its whole ray, collisions deposit nothing -- the same mean, no variance without scattering, and far
        less of it in optically thin air."""
        entry = self._emission_entry("renderCameraEmission", estimator, "mcbrat_render_camera_emission", "mcbrat_render_camera_emission_expected")
        cell, sfc = self._emission_sources("renderCameraEmission", cellSource, surfaceSource)
        return self._render_camera(entry, camera, (ptr(cell), ptr(sfc)), randomNumbers.seed, randomNumbers.nextPhotonId,
                                   samplesPerPixel, numBatches, randomNumbers, emission=True, estimator=estimator)

    def renderSensorsEmission(self, sensors, randomNumbers, samplesPerSensor, numBatches=1, cellSource=None, surfaceSource=None,
                              gridInLds=-1, estimator="collision"):
        """The emitted (thermal) irradiance (planar sensors: a pyrgeometer) and actinic flux (spherical ones) at `sensors`, in
        the sources' units times steradians.  Returns "irradiance", "irradiance_StdErr" (one value per sensor), "batchMeans"
        [numBatches, n], "dropped" and "estimator"; there is no direct part ("emission": True marks the dict for the NetCDF
        writers).  estimator="expected": as for renderCameraEmission."""
        entry = self._emission_entry("renderSensorsEmission", estimator, "mcbrat_render_sensors_emission", "mcbrat_render_sensors_emission_expected")
        cell, sfc = self._emission_sources("renderSensorsEmission", cellSource, surfaceSource)
        (irr, err), means, dropped = self._render_sensors(entry, sensors, (ptr(cell), ptr(sfc)), randomNumbers,
                                                          samplesPerSensor, numBatches, gridInLds, 2)
        return {"irradiance": irr, "irradiance_StdErr": err, "batchMeans": means, "dropped": dropped, "emission": True, "estimator": estimator}

    def sunTransmittance(self, points):
        """exp(-optical depth) from each point (an [n, 3] array of x, y, z) toward the sun up to the top of the loaded
        domain: the direct transmittance at a point, without noise (mcbrat_sun_transmittance)."""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        out = np.zeros(pts.shape[0], np.float32)
        self._check(self._lib.mcbrat_sun_transmittance(self._ctx, pts.shape[0], ptr(pts), ptr(out)))
        return out

    # -- reportResults ----------------------------------------------------------------
    def reportResults(self):
        nx, ny, nz = self._dims
        mu, md, ma = C.c_float(), C.c_float(), C.c_float()
        up, dn, ab = (np.zeros(nx * ny, np.float32) for _ in range(3))
        prof = np.zeros(nz, np.float32)
        vol = np.zeros(nx * ny * nz, np.float32)
        self._check(self._lib.mcbrat_report_results(self._ctx, C.addressof(mu), C.addressof(md), C.addressof(ma), ptr(up),
                                                    ptr(dn), ptr(ab), ptr(prof), ptr(vol)))
        f2 = lambda a: a.reshape(ny, nx).T  # noqa: E731  -> [ix, iy]
        res = dict(meanFluxUp=mu.value, meanFluxDown=md.value, meanFluxAbsorbed=ma.value,
                   fluxUp=f2(up), fluxDown=f2(dn), fluxAbsorbed=f2(ab), absorbedProfile=prof,
                   volumeAbsorption=vol.reshape(nz, ny, nx).transpose(2, 1, 0))
        nd = self.numIntensityDirections()
        if nd > 0:  # meanIntensity(direction), intensity(x, y, direction) :980-1010
            mean_i = np.zeros(nd, np.float32)
            inten = np.zeros(nd * nx * ny, np.float32)
            self._check(self._lib.mcbrat_report_intensity(self._ctx, ptr(mean_i), ptr(inten)))
            res.update(meanIntensity=mean_i, intensity=inten.reshape(nd, ny, nx).transpose(2, 1, 0))
        if self.recLevelFluxes:
            res.update(self.reportLevelFluxes())
        if self.recActinicFlux:
            res.update(self.reportActinicFlux())
        if self.recSideFluxes:
            res.update(self.reportSideFluxes())
        if self.numRecScatOrd >= 0:  # reportResults(...ByScatOrd) :850-864, :887-903, :1010-1040; order last, as the reference's arrays
            no = self.numRecScatOrd + 1
            mu_o, md_o = np.zeros(no, np.float32), np.zeros(no, np.float32)
            up_o, dn_o = np.zeros(no * nx * ny, np.float32), np.zeros(no * nx * ny, np.float32)
            mi_o = np.zeros(no * nd, np.float32) if nd > 0 else None
            in_o = np.zeros(no * nd * nx * ny, np.float32) if nd > 0 else None
            self._check(self._lib.mcbrat_report_scattering_orders(self._ctx, ptr(mu_o), ptr(md_o), ptr(up_o), ptr(dn_o),
                                                                  ptr(mi_o), ptr(in_o)))
            res.update(meanFluxUpByScatOrd=mu_o, meanFluxDownByScatOrd=md_o,
                       fluxUpByScatOrd=up_o.reshape(no, ny, nx).transpose(2, 1, 0),
                       fluxDownByScatOrd=dn_o.reshape(no, ny, nx).transpose(2, 1, 0))
            if nd > 0:
                res.update(meanIntensityByScatOrd=mi_o.reshape(no, nd).T,
                           intensityByScatOrd=in_o.reshape(no, nd, ny, nx).transpose(3, 2, 1, 0))
        return res

    def reportLevelFluxes(self):
        """The last batch's upward and downward flux through every level: levelFluxUp[ix, iy, k], levelFluxDown[ix, iy, k] and
        their domain means meanLevelFluxUp[k], meanLevelFluxDown[k]; level k = 0 .. numZ is the face zPosition[k].  With
        recDirectLevelFluxes also levelFluxDownDirect / levelFluxDownDiffuse[ix, iy, k] -- the parts of levelFluxDown carried by
        photons that have not yet collided or reached the surface, and by the others -- and their domain means."""
        nx, ny, nz = self._dims
        nl = nz + 1
        mu, md = np.zeros(nl, np.float32), np.zeros(nl, np.float32)
        up, dn = np.zeros(nl * nx * ny, np.float32), np.zeros(nl * nx * ny, np.float32)
        self._check(self._lib.mcbrat_report_level_fluxes(self._ctx, ptr(mu), ptr(md), ptr(up), ptr(dn)))
        res = dict(meanLevelFluxUp=mu, meanLevelFluxDown=md, levelFluxUp=up.reshape(nl, ny, nx).transpose(2, 1, 0),
                   levelFluxDown=dn.reshape(nl, ny, nx).transpose(2, 1, 0))
        if self.recDirectLevelFluxes:
            mdir, mdif = np.zeros(nl, np.float32), np.zeros(nl, np.float32)
            dirc, dif = np.zeros(nl * nx * ny, np.float32), np.zeros(nl * nx * ny, np.float32)
            self._check(self._lib.mcbrat_report_direct_level_fluxes(self._ctx, ptr(mdir), ptr(mdif), ptr(dirc), ptr(dif)))
            res.update(meanLevelFluxDownDirect=mdir, meanLevelFluxDownDiffuse=mdif,
                       levelFluxDownDirect=dirc.reshape(nl, ny, nx).transpose(2, 1, 0),
                       levelFluxDownDiffuse=dif.reshape(nl, ny, nx).transpose(2, 1, 0))
        return res

    def reportActinicFlux(self):
        """The last batch's actinic flux by track length: actinicFlux[ix, iy, iz], the weighted path length inside the cell per
        photon of its column and per km of its depth (dimensionless: 1 in a vacuum under an overhead sun), and the layer means
        meanActinicFlux[iz] (the sum over the columns divided by their number)."""
        nx, ny, nz = self._dims
        mean, act = np.zeros(nz, np.float32), np.zeros(nx * ny * nz, np.float32)
        self._check(self._lib.mcbrat_report_actinic_flux(self._ctx, ptr(mean), ptr(act)))
        return dict(meanActinicFlux=mean, actinicFlux=act.reshape(nz, ny, nx).transpose(2, 1, 0))

    def reportSideFluxes(self):
        """The last batch's flux through the vertical faces of every cell: sideFluxXPlus[ix, iy, iz] and sideFluxXMinus[ix, iy, iz],
        the weight that crossed the face x = xPosition[ix+1] of the patch (iy, iz) towards +x and towards -x, per photon of the
        column and scaled by dx / dz to a flux density per unit flux through a horizontal unit area at the top; sideFluxYPlus and
        sideFluxYMinus likewise for the face y = yPosition[iy+1]; and their layer means meanSideFluxXPlus[iz] ... (the sum over
        the columns divided by their number)."""
        nx, ny, nz = self._dims
        mean, bins = np.zeros(4 * nz, np.float32), np.zeros(4 * nx * ny * nz, np.float32)
        self._check(self._lib.mcbrat_report_side_fluxes(self._ctx, ptr(mean), ptr(bins)))
        res = {}
        for q, name in enumerate(SIDE_FLUX_NAMES):
            res["mean" + name[0].upper() + name[1:]] = mean[q * nz:(q + 1) * nz].copy()
            res[name] = bins[q * nx * ny * nz:(q + 1) * nx * ny * nz].reshape(nz, ny, nx).transpose(2, 1, 0)
        return res

    # -- batch moments (what the driver keeps in *Stats and reduces over processes) -----
    def momentsLength(self):
        return int(self._lib.mcbrat_moments_length(self._ctx))

    def bindMoments(self, device_ptr):
        self._check(self._lib.mcbrat_bind_moments(self._ctx, C.c_void_p(device_ptr)))

    def momentsDevicePointer(self):
        """Device address of the moment array in use (to be bound by the integrators of the other wavelengths)."""
        ptr_ = self._lib.mcbrat_moments_device_pointer(self._ctx)
        if not ptr_:
            raise McbratError("moments: no moment array (grid not set)")
        return int(ptr_)

    def frequencyDistribution(self, cdf, totalPhotons, seed=10, firstDraw=0):
        """getFrequencyDistr on the device: photons per wavelength (one uniform per photon against the power CDF)."""
        cdf = np.ascontiguousarray(cdf, np.float64)
        out = np.zeros(cdf.size, np.int64)
        self._check(self._lib.mcbrat_frequency_distribution(self._ctx, int(seed) & 0xFFFFFFFFFFFFFFFF, int(firstDraw), int(cdf.size),
                                                            ptr(cdf), int(totalPhotons), ptr(out)))
        return out

    def resetMoments(self):
        self._check(self._lib.mcbrat_reset_moments(self._ctx))

    def moments(self):
        buf = np.zeros(8 + 2 * self.momentsLength(), np.float64)
        self._check(self._lib.mcbrat_get_moments(self._ctx, ptr(buf)))
        return buf

    # -- measurement / parity ----------------------------------------------------------
    def enableCounters(self, on=True):
        self._check(self._lib.mcbrat_enable_counters(self._ctx, int(bool(on))))

    def counters(self):
        c = Counters()
        self._check(self._lib.mcbrat_get_counters(self._ctx, C.addressof(c)))
        d = c.as_dict()
        if getattr(self._lib, "_mcbrat_abi", 2) < 2:
            d["badPhotons"] = None  # (an A/B library from before ABI 2 does not write the field: unknown, not zero)
        return d

    def lastTraceMs(self):
        return float(self._lib.mcbrat_last_trace_ms(self._ctx))

    def traceFates(self, thisDomain, randomNumbers, incomingPhotons, n):
        self.specifyParameters()
        self._load_domain(thisDomain)
        self._load_source(incomingPhotons)
        fates = np.zeros(int(n), FATE_DTYPE)
        self._check(self._lib.mcbrat_trace_fates(self._ctx, randomNumbers.seed, randomNumbers.nextPhotonId, int(n), ptr(fates)))
        return fates


def new_Integrator(atmosphere, device=0):
    return Integrator(atmosphere, device)
