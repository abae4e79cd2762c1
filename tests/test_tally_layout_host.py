"""The one statement of the tally layout (mcbrat3d_amd/csrc/mcbrat_layout.h) against what it replaced.

tests/tally_layout_dump.cpp, which includes nothing but that header, is compiled with the host C++ compiler and prints the layout
of every shape asked for.  Every field is compared with the formulas the library and the finish kernels had before the header --
written out below in Python, function by function under the names they had -- never with anything the header computes.  Then the
consumers of the documented layout (driver.unpack_moments, tests/epilogue_mirror.py), the slab starts trace_kernel computes for
itself, the parts of the finish kernels (finish_parts: their order, their workgroups, the two grid sizes) against the lines the host
had, and the shapes whose products would overflow (with the sanitizers: a stand-alone program, nothing is loaded into Python)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
BUDGET = 4 << 30
NX, NY, NZ = 3, 2, 4  # all different: a swapped factor shows

# (nDir, nc, limitContrib) x numRecScatOrd x (levels, direct, actinic): also the combinations the library refuses -- the layout
# function is total, and the old formulas are defined for them
INTENSITY = [(0, 1, 0), (0, 2, 0)] + [(2, nc, limit) for nc in (1, 2) for limit in (0, 1)]
ORDERS = [-1, 0, 2]
FACE = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)]
SHAPES = [(NX, NY, NZ, nc, nDir, limit, N, lv, di, ac) for (nDir, nc, limit), N, (lv, di, ac) in itertools.product(INTENSITY, ORDERS, FACE)]
# near the budget (tests/test_gpu_actinic.py: 8192 x 8192 columns): two level parts of 4 levels are exactly 4 GiB, nine actinic
# layers 4.5 GiB, three 1.5 GiB; and order parts on either side of it
NEAR = [(8192, 8192, 3, 1, 0, 0, -1, 1, 0, 0), (8192, 8192, 3, 1, 0, 0, -1, 1, 1, 0), (8192, 8192, 3, 1, 0, 0, -1, 0, 0, 1),
        (8192, 8192, 3, 1, 0, 0, -1, 1, 0, 1), (8192, 8192, 9, 1, 0, 0, -1, 0, 0, 1), (8192, 8192, 4, 1, 0, 0, -1, 1, 0, 0),
        (4096, 4096, 2, 1, 2, 0, 7, 0, 0, 0), (4096, 4096, 2, 1, 2, 0, 8, 0, 0, 0), (4096, 4096, 2, 1, 0, 0, 15, 0, 0, 0),
        (4096, 4096, 2, 1, 0, 0, 16, 0, 0, 0)]


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "tally_layout_dump.cpp")])
    return out


def _dump(exe, shapes, budget=BUDGET):
    """-> one dict of integers per shape (numRecScatOrd is handed over as nOrd = numRecScatOrd + 1, 0 off), and the line's last words"""
    args = [",".join(str(v) for v in (s[:6] + (max(s[6] + 1, 0),) + s[7:])) for s in shapes]
    text = subprocess.run([exe, str(budget)] + args, check=True, capture_output=True, text=True, timeout=60).stdout
    lines = text.strip().split("\n")
    assert len(lines) == len(shapes)
    out = []
    for line in lines:
        words = line.split()
        d = {k: int(v) for k, v in (w.split("=") for w in words if "=" in w)}
        d["verdict"] = " ".join(w for w in words if "=" not in w)
        out.append(d)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("layout") / "tally_layout_dump"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the formulas of the commit before the header, under their old names
# ---------------------------------------------------------------------------------------------------------------------------------
class Parent:
    def __init__(self, nx, ny, nz, nc, nDir, limitContrib, numRecScatOrd, levelFluxes, directLevelFluxes, actinicFlux, sideFluxes=0):
        self.nx, self.ny, self.nz, self.nc, self.nDir, self.limitContrib = nx, ny, nz, nc, nDir, limitContrib
        self.numRecScatOrd, self.levelFluxes, self.directLevelFluxes, self.actinicFlux = numRecScatOrd, levelFluxes, directLevelFluxes, actinicFlux
        self.sideFluxes = sideFluxes
        self.ncol = nx * ny

    # mcbrat_api.hip
    def orders_on(self): return self.numRecScatOrd >= 0
    def levels_on(self): return self.levelFluxes != 0
    def direct_on(self): return self.levelFluxes != 0 and self.directLevelFluxes != 0
    def actinic_on(self): return self.actinicFlux != 0
    def level_parts(self): return (3 if self.direct_on() else 2) if self.levels_on() else 0
    def level_quantities(self): return (4 if self.direct_on() else 2) if self.levels_on() else 0
    def level_bins(self): return self.level_parts() * self.nx * self.ny * (self.nz + 1)
    def actinic_bins(self): return self.nx * self.ny * self.nz if self.actinic_on() else 0
    def global_bins(self): return self.level_bins() + self.actinic_bins()
    def moments_actinic_len(self): return self.nz * (1 + self.nx * self.ny) if self.actinic_on() else 0

    def moments_len(self):
        ncol = self.ncol
        return 3 + 3 * ncol + self.nz + ncol * self.nz + self.nDir * ncol + \
            ((self.numRecScatOrd + 1) * (2 + self.nDir) * (1 + ncol) if self.orders_on() else 0) + \
            self.level_quantities() * (self.nz + 1) * (1 + ncol) + self.moments_actinic_len()

    def moments_actinic_at(self): return self.moments_len() - self.moments_actinic_len()
    def moments_levels_at(self): return self.moments_actinic_at() - self.level_quantities() * (self.nz + 1) * (1 + self.nx * self.ny)
    def moments_direct_at(self): return self.moments_levels_at() + 2 * (self.nz + 1) * (1 + self.nx * self.ny)

    def slab_stride(self, fluxRun=False):
        ncol, nvox, nDir = self.ncol, self.ncol * self.nz, 0 if fluxRun else self.nDir
        return 2 * ncol + nvox + nDir * ncol + ((self.nc + 1) * nDir * (ncol + 1) if self.limitContrib and not fluxRun else 0) + \
            ((self.numRecScatOrd + 1) * (2 + nDir) * ncol if self.orders_on() else 0) + self.global_bins()

    def level_bins_fit(self, parts, budget): return float(parts) * self.nx * self.ny * (self.nz + 1.0) * 8 <= float(budget)

    def global_bins_fit(self, levelParts, actinic, budget):
        nx, ny, nz = float(self.nx), float(self.ny), float(self.nz)
        return (levelParts * nx * ny * (nz + 1.0) + (nx * ny * nz if actinic else 0.0)) * 8 <= float(budget)

    def orders_fit(self, budget):  # mcbrat_specify_scattering_orders, inline
        return not (float(self.numRecScatOrd + 1) * (2 + self.nDir) * self.ncol * 8 > float(budget))

    # mcbrat_compute_radiative_transfer: the scratch behind scalVals, per batch, and the parts of FinishParams
    def nOrd(self): return self.numRecScatOrd + 1 if self.orders_on() else 0
    def nLvl(self): return self.nz + 1 if self.levels_on() else 0
    def ordVals(self): return 3 + self.nz
    def lvlVals(self): return self.ordVals() + (2 + self.nDir) * self.nOrd()
    def actVals(self): return self.lvlVals() + self.level_quantities() * self.nLvl()
    def needScal(self): return 3 + self.nz + self.nOrd() * (2 + self.nDir) + self.level_quantities() * (self.nz + 1) + (self.nz if self.actinic_on() else 0)
    def lvlSlab(self): return self.slab_stride() - self.global_bins()
    def actSlab(self): return self.slab_stride() - self.actinic_bins()
    def slabLds(self): return self.slab_stride() - self.global_bins()  # plan_launch

    # mcbrat_compute_radiative_transfer: the workgroups of every part of finish_gather and finish_fold in a launch round of nb
    # batches, as the lines f.gatherColumns = ... f.foldSideMeans = filled them before finish_parts() (kFinishBlock = 256 lanes,
    # kVolVox = 32 cells per workgroup), in the order of the two dispatch chains the kernels had
    def side_on(self): return self.levelFluxes != 0 and self.sideFluxes != 0

    def finish_counts(self, nb):
        ncol, nvox, nz, nDir = self.ncol, self.ncol * self.nz, self.nz, self.nDir
        nOrd, nLvl, nLvlQ, act, side = self.nOrd(), self.nLvl(), self.level_quantities(), self.actinic_on(), self.side_on()
        gather = [("gatherColumns", (ncol * nb + 256 - 1) // 256),
                  ("gatherVolume", (nvox + 32 - 1) // 32),
                  ("gatherReduce", (3 + nz) * nb),
                  ("gatherIntensity", (ncol * nDir + 256 - 1) // 256),
                  ("gatherOrders", ((2 + nDir) * ncol * nOrd + 256 - 1) // 256),
                  ("gatherOrderMeans", (2 + nDir) * nOrd * nb),
                  ("gatherLevels", (nLvlQ * ncol * nLvl + 256 - 1) // 256),
                  ("gatherLevelMeans", nLvlQ * nLvl * nb),
                  ("gatherActinic", (nvox + 32 - 1) // 32 if act else 0),
                  ("gatherActinicMeans", nz * nb if act else 0),
                  ("gatherSide", (4 * nvox + 32 - 1) // 32 if side else 0),
                  ("gatherSideMeans", 4 * nz * nb if side else 0)]
        fold = [("foldColumns", (3 * ncol + 256 - 1) // 256),
                ("foldScalars", (3 + nz + 256 - 1) // 256),
                ("foldOrderMeans", ((2 + nDir) * nOrd + 256 - 1) // 256),
                ("foldLevelMeans", (nLvlQ * nLvl + 256 - 1) // 256),
                ("foldActinicMeans", (nz + 256 - 1) // 256 if act else 0),
                ("foldSideMeans", (4 * nz + 256 - 1) // 256 if side else 0)]
        return gather, fold

    # mcbrat_kernels.hip, the finish kernels (from FinishParams: nOrd, nLvl as above, lvlDirect = direct_on, act = actinic_on)
    def k_moments_base(self): return 3 + 3 * self.ncol + self.nz + self.ncol * self.nz + self.nDir * self.ncol

    def k_moments_total(self):
        return self.k_moments_base() + (self.nOrd() * (2 + self.nDir) + (4 if self.direct_on() else 2) * self.nLvl() +
                                        (self.nz if self.actinic_on() else 0)) * (1 + self.nx * self.ny)

    def k_moments_actinic(self): return self.k_moments_total() - self.nz * (1 + self.nx * self.ny)
    def k_moments_levels(self): return self.k_moments_base() + self.nOrd() * (2 + self.nDir) * (1 + self.nx * self.ny)
    def k_moments_direct(self): return self.k_moments_levels() + 2 * self.nLvl() * (1 + self.nx * self.ny)
    def k_slab_orders(self): return 2 * self.ncol + self.ncol * self.nz + self.nDir * self.ncol
    def k_slab_intensity(self): return 2 * self.ncol + self.ncol * self.nz  # the intensity part, finish_excess
    def k_slab_by_component(self): return self.k_slab_intensity() + (1 + 0) * self.nDir * self.ncol  # finish_excess: byc of j = 0, d = 0
    def k_slab_excess(self): return self.k_slab_intensity() + (self.nc + 2) * self.nDir * self.ncol

    # mcbrat_kernels.hip, trace_kernel (ORD, LVL, DIRECT, ACT: the template flags)
    def t_ordUp(self): return 2 * self.ncol + self.ncol * self.nz + self.nDir * self.ncol
    def t_ordDown(self): return self.t_ordUp() + self.ncol * (self.numRecScatOrd + 1)
    def t_lvlUp(self): return 2 * self.ncol + self.ncol * self.nz
    def t_lvlDown(self): return self.t_lvlUp() + self.ncol * (self.nz + 1)
    def t_lvlDirect(self): return self.t_lvlDown() + self.ncol * (self.nz + 1)
    def t_actBins(self): return 2 * self.ncol + self.ncol * self.nz + (2 * self.ncol * (self.nz + 1) if self.levels_on() else 0)
    def t_sideBins(self): return self.t_lvlDown() + self.ncol * (self.nz + 1)
    def t_ibase(self): return 2 * self.ncol + self.ncol * self.nz  # rayFinish; also the LDS slab of the LVL and ACT kernels
    def t_ordI(self): return (2 + self.nDir) * self.ncol + self.ncol * self.nz + 2 * self.ncol * (self.numRecScatOrd + 1)


def test_the_shapes_cover_what_was_asked_for():
    assert len(SHAPES) == len(set(SHAPES)) == 6 * 3 * 5
    assert {s[4] for s in SHAPES} == {0, 2} and {s[6] for s in SHAPES} == {-1, 0, 2}
    assert {(s[3], s[5]) for s in SHAPES if s[4] > 0} == {(1, 0), (1, 1), (2, 0), (2, 1)}


def test_every_field_is_what_the_old_formulas_give(exe):
    for s, d in zip(SHAPES, _dump(exe, SHAPES)):
        p = Parent(*s)
        ncol, nvox = p.ncol, p.ncol * p.nz
        # the slab
        assert (d["slabFluxUp"], d["slabFluxDown"], d["slabVolume"]) == (0, ncol, 2 * ncol), s  # (column_value, the volume part)
        assert d["slabIntensity"] == p.k_slab_intensity() == 2 * ncol + nvox, s
        assert d["slabStride"] == p.slab_stride() and d["fluxRunStride"] == p.slab_stride(True), s
        assert d["slabLds"] == p.slabLds() and d["slabLevels"] == p.lvlSlab() and d["slabActinic"] == p.actSlab(), s
        if p.limitContrib:
            assert d["slabByComponent"] == p.k_slab_by_component() and d["slabExcess"] == p.k_slab_excess(), s
        # the order part, where there is one (an empty part starts where the forward pass has got to).
        # limitIntensityContributions with scattering orders is refused by the library (kOrdersLimitMsg), and the old formulas
        # contradict each other there: slab_stride counts both parts, slab_orders puts the orders where the by-component part
        # lies.  There the orders are held to the one reading slab_stride allows, which holds everywhere: the part ends where the
        # level part starts.
        if p.orders_on() and not p.limitContrib:
            assert d["slabOrders"] == p.k_slab_orders(), s
        assert d["slabOrders"] + p.nOrd() * (2 + p.nDir) * ncol == p.lvlSlab(), s
        # the moments
        assert (d["momMeans"], d["momColumns"], d["momProfile"], d["momVolume"]) == (0, 3, 3 + 3 * ncol, 3 + 3 * ncol + p.nz), s
        assert d["momIntensity"] == 3 + 3 * ncol + p.nz + nvox, s  # (mcbrat_report_intensity, the intensity part)
        assert d["momOrders"] == p.k_moments_base(), s
        assert d["momentsLen"] == p.moments_len() == p.k_moments_total(), s
        assert d["momLevels"] == p.moments_levels_at() == p.k_moments_levels(), s
        assert d["momDirect"] == p.k_moments_direct(), s
        if p.levels_on():
            assert d["momDirect"] == p.moments_direct_at(), s
        assert d["momActinic"] == p.moments_actinic_at(), s
        if p.actinic_on():
            assert d["momActinic"] == p.k_moments_actinic(), s
        # the scalar scratch
        assert (d["scalOrders"], d["scalLevels"], d["scalActinic"], d["scalPerBatch"]) == (p.ordVals(), p.lvlVals(), p.actVals(), p.needScal()), s


def _starts(exe, shapes):
    """-> per shape what the slab_*_start functions return as trace_kernel calls them (the dump program's `starts` mode)"""
    args = [",".join(str(v) for v in (s[:6] + (max(s[6] + 1, 0),) + s[7:])) for s in shapes]
    lines = subprocess.run([exe, "starts"] + args, check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")
    assert len(lines) == len(shapes)
    return [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in lines]


def test_the_slab_starts_trace_kernel_computes_for_itself(exe):
    seen = set()
    for s, d, k in zip(SHAPES, _dump(exe, SHAPES), _starts(exe, SHAPES)):
        p = Parent(*s)
        # what the kernel calls, against the lines it had: the level, actinic and side starts and the intensity part whatever the
        # shape (the lines did not look at directions or orders: the flux runs they serve have none), the order parts where orders are on
        assert (k["lvlUp"], k["lvlDown"], k["lvlDirect"], k["sideBins"]) == (p.t_lvlUp(), p.t_lvlDown(), p.t_lvlDirect(), p.t_sideBins()), s
        assert k["actBins"] == p.t_actBins() and k["ibase"] == p.t_ibase(), s
        if p.orders_on():
            assert (k["ordUp"], k["ordDown"], k["ordI"]) == (p.t_ordUp(), p.t_ordDown(), p.t_ordI()), s
        face = p.levels_on() or p.actinic_on()
        if p.orders_on() and not p.limitContrib and not face:  # ORD
            assert (d["slabOrders"], d["slabOrders"] + p.ncol * p.nOrd()) == (p.t_ordUp(), p.t_ordDown()), s
            seen.add("ORD")
        if face and p.nDir == 0 and not p.orders_on() and not (p.actinic_on() and p.direct_on()):
            if p.levels_on():  # LVL
                assert (d["slabLevels"], d["slabLevels"] + p.ncol * p.nLvl()) == (p.t_lvlUp(), p.t_lvlDown()), s
                seen.add("LVL")
            if p.direct_on():  # DIRECT: the third part
                assert d["slabLevels"] + 2 * p.ncol * p.nLvl() == p.t_lvlDirect(), s
                seen.add("DIRECT")
            if p.actinic_on():  # ACT, with LVL and without
                assert d["slabActinic"] == p.t_actBins(), s
                seen.add("ACT+LVL" if p.levels_on() else "ACT")
    assert seen == {"ORD", "LVL", "DIRECT", "ACT", "ACT+LVL"}


def test_the_fit_answers_are_the_old_ones(exe):
    shapes = SHAPES + NEAR
    for budget in (BUDGET, 8 * 60, 8 * 200):  # the library's, and two that divide the small shapes
        for s, d in zip(shapes, _dump(exe, shapes, budget)):
            p = Parent(*s)
            assert d["fitOrders"] == p.orders_fit(budget), (s, budget)
            assert d["fitGlobalBins"] == p.global_bins_fit(float(p.level_parts()), p.actinic_on(), budget), (s, budget)
            if not p.actinic_on():
                assert d["fitGlobalBins"] == p.level_bins_fit(p.level_parts(), budget), (s, budget)
            assert d["fitStride"] == (not p.slab_stride() * 8 > budget), (s, budget)
            assert d["verdict"] == ("fits" if d["fitStride"] else "does not fit")
    near = _dump(exe, NEAR)
    assert [d["fitGlobalBins"] for d in near[:6]] == [1, 0, 1, 0, 0, 0]  # (2 parts x 4 levels: exactly 4 GiB)
    assert [d["fitOrders"] for d in near[6:]] == [1, 0, 1, 0]         # (2^24 columns x 4 x 8 orders, x 2 x 16: exactly 4 GiB)


def _parts(exe, shapes, nb):
    """-> per shape (11 values, the last one side) the words of finish_parts() in a launch round of nb batches: [(name, count)] in
    the order printed -- the order of the enums -- and the dict of them"""
    args = [",".join(str(v) for v in (s[:6] + (max(s[6] + 1, 0),) + s[7:])) for s in shapes]
    text = subprocess.run([exe, "parts", str(nb)] + args, check=True, capture_output=True, text=True, timeout=60).stdout
    lines = text.strip().split("\n")
    assert len(lines) == len(shapes)
    return [[(k, int(v)) for k, v in (w.split("=") for w in line.split())] for line in lines]


ROUNDS = (1, 3, 64, 65)
# a wider domain beside the small one: more than one workgroup in every thread-per-element and cell part
PART_DIMS = ((NX, NY, NZ), (37, 29, 11))


def _part_shapes():
    for nx, ny, nz in PART_DIMS:
        for s in SHAPES:
            for side in (0, 1):
                yield (nx, ny, nz) + s[3:] + (side,)


def _check_parts(exe):
    shapes = list(_part_shapes())
    assert len(shapes) == 2 * 2 * len(SHAPES)
    on = set()
    for nb in ROUNDS:
        for s, words in zip(shapes, _parts(exe, [s[:10] + (int(bool(s[7] and s[10])),) for s in shapes], nb)):  # (side as tally_shape hands it over)
            p = Parent(*s)
            gather, fold = p.finish_counts(nb)
            d = dict(words)
            # every count is the old formula's, and the printed order -- the enums', which both kernels walk -- is the old chains'
            assert words[:len(gather) + len(fold)] == gather + fold, (s, nb)
            assert (d["gatherParts"], d["foldParts"]) == (len(gather), len(fold)) == (12, 6)
            # each grid is the sum of its parts (the two launch lines)
            assert d["gatherGrid"] == sum(n for _, n in gather) and d["foldGrid"] == sum(n for _, n in fold), (s, nb)
            # a part that is off has no workgroup, one that is on has some
            for names, live in ((("gatherIntensity",), p.nDir > 0), (("gatherOrders", "gatherOrderMeans", "foldOrderMeans"), p.orders_on()),
                                (("gatherLevels", "gatherLevelMeans", "foldLevelMeans"), p.levels_on()),
                                (("gatherActinic", "gatherActinicMeans", "foldActinicMeans"), p.actinic_on()),
                                (("gatherSide", "gatherSideMeans", "foldSideMeans"), p.side_on())):
                assert all((d[n] > 0) == live for n in names), (s, nb, names)
                on.update(n for n in names if live)
            assert all(d[n] > 0 for n in ("gatherColumns", "gatherVolume", "gatherReduce", "foldColumns", "foldScalars"))
    assert len(on) == 13  # (every optional part was on somewhere)


def test_the_finish_parts_are_what_the_old_host_lines_give(exe):
    _check_parts(exe)


def test_the_consumers_place_every_part_where_the_header_does(exe):
    from mcbrat3d_amd import driver
    from tests import epilogue_mirror as EM
    xe, ye, ze = np.arange(NX + 1.0), np.arange(NY + 1.0), np.arange(NZ + 1.0)
    names = dict(meanFluxUp="momMeans", fluxUp="momColumns", absorbedProfile="momProfile", absorbedVolume="momVolume", intensity="momIntensity",
                 meanFluxUpByScatOrd="momOrders", meanLevelFluxUp="momLevels", meanLevelFluxDownDirect="momDirect", meanActinicFlux="momActinic")
    for s, d in zip(SHAPES, _dump(exe, SHAPES)):
        nx, ny, nz, nc, nDir, limit, N, levels, direct, actinic = s
        if nc != 1 or limit:  # (neither is part of the moments: the same moments as the shape without them)
            continue
        M = d["momentsLen"]
        buf = np.zeros(8 + 2 * M)
        buf[8:8 + M], buf[8 + M:] = np.arange(M), np.arange(M) + 0.5
        out = driver.unpack_moments(buf, nx, ny, nz, nDirections=nDir, numRecScatOrd=N, levelFluxes=bool(levels),
                                    directLevelFluxes=bool(levels and direct), actinicFlux=bool(actinic))
        first = {k: (float(np.min(v[0])), float(np.min(v[1]))) for k, v in out.items() if k not in ("totalPhotons", "batches")}
        for name, field in names.items():
            if name in first:
                assert first[name] == (d[field], d[field] + 0.5), (s, name)
        assert first["fluxDown"][0] == d["momColumns"] + nx * ny and first["fluxAbsorbed"][0] == d["momColumns"] + 2 * nx * ny
        assert ("intensity" in first, "meanFluxUpByScatOrd" in first, "meanLevelFluxUp" in first, "meanLevelFluxDownDirect" in first,
                "meanActinicFlux" in first) == (nDir > 0, N >= 0, bool(levels), bool(levels and direct), bool(actinic)), s
        last = max(first, key=lambda k: first[k][0])  # the part that ends the array ends it at M
        assert first[last][0] + np.size(out[last][0]) == M, s
        if not (levels or actinic):  # what the epilogue mirror covers: directions and orders
            g = EM.Grid(xe, ye, ze, nDir=nDir, nOrd=max(N + 1, 0))
            assert (g.M, g.S, g.base, g.slabOrders) == (M, d["slabStride"], d["momOrders"], d["slabOrders"]), s


def test_shapes_that_would_overflow_do_not_fit_and_do_not_overflow(tmp_path):
    """numRecScatOrd = 2^31 - 2 with 2^31 - 1 directions on 32768 x 32768 x 1 (the order part alone passes 2^64 elements), and 2^30
    cells with every tally on: under the undefined-behaviour and address sanitizers, which end the program at the first finding."""
    exe = _compile(str(tmp_path / "tally_layout_dump_san"), "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
    big = 2 ** 31 - 1
    shapes = [(32768, 32768, 1, 1, big, 0, big - 1, 0, 0, 0), (32768, 32768, 1, 2, big, 1, big - 1, 1, 1, 1),
              (1024, 1024, 1024, 1, 2, 1, 2, 1, 1, 1), (2 ** 30, 1, 1, 8, big, 1, big - 1, 1, 1, 1)]
    for d in _dump(exe, shapes):
        assert d["verdict"] == "does not fit" and not d["fitStride"]
    assert [d["fitOrders"] for d in _dump(exe, shapes)] == [0, 0, 1, 0]
    # (and the sanitized program agrees with the plain one where nothing is near overflowing)
    small = _dump(exe, SHAPES[:10])
    assert all(d["verdict"] == "fits" for d in small)
    # the part list under the same sanitizers: every count as the plain program gives it
    _check_parts(exe)
