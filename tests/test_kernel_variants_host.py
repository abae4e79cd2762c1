"""The one statement of the kernel variants (mcbrat3d_amd/csrc/mcbrat_variants.h) against what it replaced.

tests/golden/kernel_choice.txt is the kernel, workgroup size and dynamic LDS that the host library chose for every input its choice
reads, recorded from the ladder of helper templates the header replaced (scripts/kernel_choice.py writes it, by naming the host
stub the library returns; the enumeration and its pruning rules are at the top of scripts/kernel_choice.hip).
tests/kernel_variants_dump.cpp, which includes nothing but the header, is compiled with the host C++ compiler and picks for the
same inputs.  No GPU, and nothing is loaded into Python: the sanitizers run a stand-alone program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_choice.txt")
# what the ladder built (the host stubs of a host-only compile of mcbrat_api.hip before the header) ...
BUILT_BEFORE = {"trace": 272, "block": 108}
# ... and what nothing reaches: the instrumented block walk has no x-z instantiation to pick (it keeps y), but the ladder instantiated one
DROPPED = {"trace_block_kernel<512, %s, true, %s, 2, 0, false>" % (t, e) for t in ("true", "false") for e in ("true", "false")}


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "kernel_variants_dump.cpp")])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("variants") / "kernel_variants_dump"))


@pytest.fixture(scope="module")
def golden():
    """-> [(kind, code, expected)]: expected is "<block> <lds> <kernel>" or "!<refusal>".  One line per kernel or refusal, then
    " | <block> <lds>:" and the inputs as base/mask pairs: every code base | m, m a subset of the mask (scripts/kernel_choice.py)"""
    inputs = []
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith("#"):
                continue
            name, *parts = line.rstrip("\n").split(" | ")
            kind = "B" if name.startswith("trace_block_kernel") else "T"
            for part in parts:
                how, codes = part.split(":")
                for pair in codes.split():
                    base, mask = (int(v, 16) for v in pair.split("/"))
                    sub = mask
                    while True:
                        inputs.append((kind, "%x" % (base | sub), name if name.startswith("!") else "%s %s" % (how, name)))
                        if sub == 0:
                            break
                        sub = (sub - 1) & mask
    assert len({(k, c) for k, c, _ in inputs}) == len(inputs)  # (no input twice)
    return sorted(inputs, key=lambda i: (i[0], int(i[1], 16)))


def _pick(exe, golden):
    text = subprocess.run([exe, "pick"], input="".join("%s %s\n" % (k, c) for k, c, _ in golden), check=True, capture_output=True, text=True, timeout=120).stdout
    return text.rstrip("\n").split("\n")


def _built(exe):
    lines = subprocess.run([exe, "list"], check=True, capture_output=True, text=True, timeout=60).stdout.rstrip("\n").split("\n")
    return [tuple(l.split(" ", 2)) for l in lines]  # (trace|block, valid, name)


@pytest.fixture(scope="module")
def picked(exe, golden):
    return _pick(exe, golden)


def test_the_golden_file_is_small_and_covers_both_kernels(golden):
    assert os.path.getsize(GOLDEN) < 300 * 1000
    assert sum(k == "T" for k, _, _ in golden) > 4000 and sum(k == "B" for k, _, _ in golden) > 10000


def test_same_choice_input_for_input(golden, picked):
    """the pickers give the kernel, the workgroup size and the dynamic LDS the ladder gave (the block walk's LDS is its launch's
    layout, 0 in both), and refuse what it refused in its words"""
    assert len(picked) == len(golden)
    for (kind, code, want), got in zip(golden, picked):
        assert got == "%s %s %s" % (kind, code, want)


def test_every_pick_is_valid_and_built(picked):
    # (the dump program appends " invalid" / " unbuilt" to such a line)
    assert not [l for l in picked if l.endswith("invalid") or l.endswith("unbuilt")]


def test_every_built_variant_is_valid_unique_and_reached(exe, golden):
    built = _built(exe)
    assert all(valid == "1" for _, valid, _ in built)
    names = [n for _, _, n in built]
    assert len(set(names)) == len(names)
    # reachability: by the enumeration, which includes the options that reach a kernel (blockSize; privateTallies and gridLdsMode
    # through the plan's fields; blockSpanKernel, noSimple3); nothing built is left unreached
    reached = {want.split(" ", 2)[2] for _, _, want in golden if not want.startswith("!")}
    assert set(names) == reached


def test_counts(exe):
    built = _built(exe)
    assert sum(k == "trace" for k, _, _ in built) == BUILT_BEFORE["trace"]
    assert sum(k == "block" for k, _, _ in built) == BUILT_BEFORE["block"] - len(DROPPED)
    assert not DROPPED & {n for _, _, n in built}


def test_the_header_is_clean_under_the_sanitizers(tmp_path, golden, picked):
    """a stand-alone program under the undefined-behaviour and address sanitizers, which end it at the first finding, agrees with
    the plain one"""
    exe = _compile(str(tmp_path / "kernel_variants_dump_san"), "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
    assert _pick(exe, golden) == picked
    assert len(_built(exe)) == BUILT_BEFORE["trace"] + BUILT_BEFORE["block"] - len(DROPPED)


# ---------------------------------------------------------------------------------------------------------------------------------
# the refusals: the rule list of the header against the checks the call sites had before it, written out below site by site, in
# their order, under the names of the message constants
# ---------------------------------------------------------------------------------------------------------------------------------
STAGES = dict(SetGrid=1, SetIntensity=2, SetOrders=4, SetLevels=8, LevelsOff=16, SetDirect=32, SetActinic=64, SetSide=128, SetBrdf=256,
              SetCounters=512, Ready=1024, Trace=2048, Fates=4096, Launch=8192)
FLAGS = ("inten", "orders", "limit", "levels", "direct", "actinic", "side", "brdf", "counters", "emit")


class Asked(dict):
    """the settings of a context (direct and side as set: they count with levels only), and the sizes of the tally parts in a made-up
    unit: the level bins, what the direct tally adds, the actinic bins, the side bins, the order bins, everything else, the budget"""
    __getattr__ = dict.__getitem__

    def direct_on(self): return self.levels and self.direct
    def side_on(self): return self.levels and self.side
    def bins(self, levels, direct, actinic, side=0):  # budget_fit(with_tallies(shape, levels, direct, actinic, side)).globalBins
        return self.L * levels + self.D * (levels and direct) + self.A * actinic + self.S * (levels and side) <= self.B
    def all_bins(self): return self.bins(self.levels, self.direct, self.actinic, self.side)
    def stride(self): return self.rest + self.O * self.orders + self.L * self.levels + self.D * self.direct_on() + self.A * self.actinic + self.S * self.side_on() <= self.B
    def with_(self, **kw): return Asked(self, **kw)


def parent_set_intensity(c, nDir, limit):
    if limit and c.orders: return "kOrdersLimitMsg"
    if nDir and c.levels: return "kLevelsIntensityMsg"
    if nDir and c.actinic: return "kActinicIntensityMsg"

def parent_set_orders(c):
    if c.limit: return "kOrdersLimitMsg"
    if c.levels: return "kLevelsOrdersMsg"
    if c.actinic: return "kActinicOrdersMsg"
    if not c.O <= c.B: return "kOrdersBudgetMsg"

def parent_set_levels(c, on):
    if on:
        if c.inten: return "kLevelsIntensityMsg"
        if c.orders: return "kLevelsOrdersMsg"
        if c.brdf: return "kLevelsBrdfMsg"
        if c.counters: return "kLevelsCountersMsg"
        if not c.bins(1, 0, 0): return "kLevelsBudgetMsg"
        if c.direct and not c.bins(1, 1, 0): return "kDirectBudgetMsg"
        if c.actinic and not c.bins(1, 0, 1): return "kActinicBudgetMsg"
    elif c.direct: return "kDirectNeedsLevelsMsg"
    elif c.side: return "kSideNeedsLevelsMsg"

def parent_set_direct(c):
    if not c.levels: return "kDirectNeedsLevelsMsg"
    if c.actinic: return "kActinicDirectMsg"
    if c.side_on(): return "kSideDirectMsg"
    if not c.bins(1, 1, 0): return "kDirectBudgetMsg"

def parent_set_actinic(c):
    if c.inten: return "kActinicIntensityMsg"
    if c.orders: return "kActinicOrdersMsg"
    if c.brdf: return "kActinicBrdfMsg"
    if c.counters: return "kActinicCountersMsg"
    if c.direct_on(): return "kActinicDirectMsg"
    if c.side_on(): return "kSideActinicMsg"
    if not c.bins(c.levels, c.direct_on(), 1): return "kActinicBudgetMsg"

def parent_set_side(c):
    if not c.levels: return "kSideNeedsLevelsMsg"
    if c.direct_on(): return "kSideDirectMsg"
    if c.actinic: return "kSideActinicMsg"
    if not c.bins(1, 0, 0, 1): return "kSideBudgetMsg"

def parent_set_brdf(c):
    if c.levels: return "kLevelsBrdfMsg"
    if c.actinic: return "kActinicBrdfMsg"

def parent_enable_counters(c):
    if c.levels: return "kLevelsCountersMsg"
    if c.actinic: return "kActinicCountersMsg"

def parent_set_grid(c):  # (c: with the sizes of the grid asked for)
    if c.levels and not c.bins(c.levels, c.direct_on(), 0): return "kDirectBudgetMsg" if c.direct_on() else "kLevelsBudgetMsg"
    if c.actinic and not c.all_bins(): return "kActinicBudgetMsg"
    if c.side_on() and not c.all_bins(): return "kSideBudgetMsg"

def parent_check_ready(c):
    if c.brdf and c.emit: return "kBrdfThermalMsg"
    if c.levels:
        if c.inten: return "kLevelsIntensityMsg"
        if c.orders: return "kLevelsOrdersMsg"
        if c.brdf: return "kLevelsBrdfMsg"
        if not c.bins(c.levels, c.direct_on(), 0): return "kDirectBudgetMsg" if c.direct_on() else "kLevelsBudgetMsg"
        if c.direct_on() and c.emit: return "kDirectThermalMsg"
    if c.actinic:
        if c.inten: return "kActinicIntensityMsg"
        if c.orders: return "kActinicOrdersMsg"
        if c.brdf: return "kActinicBrdfMsg"
        if c.direct_on(): return "kActinicDirectMsg"
        if not c.all_bins(): return "kActinicBudgetMsg"
        if c.emit: return "kActinicThermalMsg"
    if c.side:
        if not c.levels: return "kSideNeedsLevelsMsg"
        if c.direct_on(): return "kSideDirectMsg"
        if c.actinic: return "kSideActinicMsg"
        if not c.all_bins(): return "kSideBudgetMsg"
        if c.emit: return "kSideThermalMsg"

def parent_compute(c):  # (after check_ready)
    if c.orders and not c.stride(): return "kOrdersStrideMsg"
    if c.orders and c.counters: return "kOrdersCountersMsg"
    if c.levels and c.counters: return "kLevelsCountersMsg"
    if c.side_on() and not c.stride(): return "kSideBudgetMsg"
    if c.levels and not c.actinic and not c.stride(): return "kDirectBudgetMsg" if c.direct_on() else "kLevelsBudgetMsg"
    if c.actinic and c.counters: return "kActinicCountersMsg"
    if c.actinic and not c.stride(): return "kActinicBudgetMsg"

def parent_trace_fates(c):  # (after check_ready)
    if c.inten: return "kFatesIntensityMsg"
    if c.levels: return "kLevelsCountersMsg"
    if c.actinic: return "kActinicCountersMsg"

def parent_launch_trace(c, debug):
    """the second line of defence -> (what the site says, every message of its checks whose own condition holds)"""
    says, holds = [], []
    def check(*cases):  # one `if` of the site: it fires when any case holds, with the message of the first that does
        on = [m for cond, m in cases if cond]
        says.extend(on[:1]); holds.extend(on)
    check((c.levels and debug, "kLevelsCountersMsg"), (c.levels and c.brdf, "kLevelsBrdfMsg"), (c.levels and c.inten, "kLevelsIntensityMsg"),
          (c.levels and c.orders, "kLevelsOrdersMsg"))
    check((c.direct_on() and c.emit, "kDirectThermalMsg"))
    check((c.actinic and debug, "kActinicCountersMsg"), (c.actinic and c.brdf, "kActinicBrdfMsg"), (c.actinic and c.inten, "kActinicIntensityMsg"),
          (c.actinic and c.orders, "kActinicOrdersMsg"))
    check((c.actinic and c.emit, "kActinicThermalMsg"), (c.actinic and c.direct_on(), "kActinicDirectMsg"))
    check((c.side_on() and c.emit, "kSideThermalMsg"), (c.side_on() and c.actinic, "kSideActinicMsg"), (c.side_on() and c.direct_on(), "kSideDirectMsg"))
    check((c.brdf and debug, "kBrdfCountersMsg"))
    check((c.inten and debug, "kCountersIntensityMsg"), (c.orders and debug, "kCountersOrdersMsg"))  # (in its choosing part)
    return (says[0] if says else None), holds


# The order of the checks at every site, for the pairs of rules that can fire together there (a budget check: direct before levels,
# one expression at the sites that tell them apart by the direct tally)
PRECEDENCE = {
    "SetIntensity": ["kOrdersLimitMsg", "kLevelsIntensityMsg", "kActinicIntensityMsg"],
    "SetOrders": ["kOrdersLimitMsg", "kLevelsOrdersMsg", "kActinicOrdersMsg", "kOrdersBudgetMsg"],
    "SetLevels": ["kLevelsIntensityMsg", "kLevelsOrdersMsg", "kLevelsBrdfMsg", "kLevelsCountersMsg", "kLevelsBudgetMsg", "kActinicBudgetMsg"],
    "LevelsOff": ["kDirectNeedsLevelsMsg", "kSideNeedsLevelsMsg"],
    "SetDirect": ["kDirectNeedsLevelsMsg", "kActinicDirectMsg", "kSideDirectMsg", "kDirectBudgetMsg"],
    "SetActinic": ["kActinicIntensityMsg", "kActinicOrdersMsg", "kActinicBrdfMsg", "kActinicCountersMsg", "kActinicDirectMsg", "kSideActinicMsg", "kActinicBudgetMsg"],
    "SetSide": ["kSideNeedsLevelsMsg", "kSideDirectMsg", "kSideActinicMsg", "kSideBudgetMsg"],
    "SetBrdf": ["kLevelsBrdfMsg", "kActinicBrdfMsg"],
    "SetCounters": ["kLevelsCountersMsg", "kActinicCountersMsg"],
    "SetGrid": ["kDirectBudgetMsg", "kLevelsBudgetMsg", "kActinicBudgetMsg", "kSideBudgetMsg"],
    "Ready": ["kBrdfThermalMsg", "kLevelsIntensityMsg", "kLevelsOrdersMsg", "kLevelsBrdfMsg", "kDirectBudgetMsg", "kLevelsBudgetMsg", "kDirectThermalMsg",
              "kActinicIntensityMsg", "kActinicOrdersMsg", "kActinicBrdfMsg", "kActinicDirectMsg", "kActinicBudgetMsg", "kActinicThermalMsg",
              "kSideNeedsLevelsMsg", "kSideDirectMsg", "kSideActinicMsg", "kSideBudgetMsg", "kSideThermalMsg"],
    "Trace": ["kOrdersStrideMsg", "kOrdersCountersMsg", "kLevelsCountersMsg", "kSideBudgetMsg", "kDirectBudgetMsg", "kLevelsBudgetMsg", "kActinicCountersMsg",
              "kActinicBudgetMsg"],
    "Fates": ["kFatesIntensityMsg", "kLevelsCountersMsg", "kActinicCountersMsg"],
}


# specify_level_fluxes asked whether the level bins fit without the direct ones (kLevelsBudgetMsg) and then with them (kDirectBudgetMsg); the
# list tells the two apart by the direct tally being set, as set_grid and check_ready did.  A context whose direct tally is set
# has level fluxes on and level bins that fit, so the site never saw either check fire with it set: no pair to order.
UNORDERED = {"SetLevels": {"kDirectBudgetMsg"}}


@pytest.fixture(scope="module")
def messages():
    """{text: name} of the message constants, read from the header"""
    import re
    src = open(os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_variants.h")).read()
    out = {}
    for m in re.finditer(r'constexpr const char \*(k\w+Msg) =\s*((?:"[^"\n]*"\s*)+);', src):
        out["".join(re.findall(r'"([^"\n]*)"', m.group(2)))] = m.group(1)
    assert len(out) == 29
    return out


def _refuse(exe, messages, asks):
    """asks: [(stage name or mask of stages, Asked, debug)] -> the rule list's answer to each, by the constant's name (None: not refused)"""
    lines = []
    for stage, c, debug in asks:
        bits = [c.inten, c.orders, c.limit, c.levels, c.direct, c.actinic, c.side, c.brdf, debug, c.emit,
                c.O * c.orders <= c.B, c.bins(c.levels, c.direct, 0), c.all_bins(), c.stride()]
        lines.append("%x %x\n" % (STAGES.get(stage, stage), sum(1 << i for i, b in enumerate(bits) if b)))
    text = subprocess.run([exe, "refuse"], input="".join(lines), check=True, capture_output=True, text=True, timeout=300).stdout
    got = text.rstrip("\n").split("\n")
    assert len(got) == len(asks)
    return [None if g == "-" else messages[g] for g in got]


def combinable(f):
    """whether the setters let a context hold these flags together (the sizes apart)"""
    if (f["direct"] or f["side"]) and not f["levels"]: return False
    if (f["levels"] or f["actinic"]) and (f["inten"] or f["orders"] or f["brdf"] or f["counters"]): return False
    if f["actinic"] and f["direct"]: return False
    if f["side"] and (f["direct"] or f["actinic"]): return False
    return not (f["limit"] and f["orders"])


def _contexts():
    """every setting a context can be in (what the setters and set_grid let through), with sizes of the tally parts on either side
    of the budget: the states a call can find"""
    import itertools
    out = []
    for flags in itertools.product((0, 1), repeat=len(FLAGS)):
        f = dict(zip(FLAGS, flags))
        if not combinable(f): continue
        for L, D, A, S, O, rest in itertools.product((1, 5), (1, 5), (1, 5), (1, 5), (1, 5), (0, 5)):
            c = Asked(f, L=L, D=D, A=A, S=S, O=O, rest=rest, B=4)
            if c.levels and not c.bins(c.levels, c.direct, 0): continue
            if (c.actinic or c.side) and not c.all_bins(): continue
            out.append(c)
    return out


def test_every_site_refuses_what_it_refused_in_the_same_words(exe, messages):
    """every call site, on every state a context can be in and with every change the call can ask for: the rule list's answer is
    the answer of the checks the site had"""
    asks, want = [], []
    def ask(stage, cand, expected, debug=None):
        asks.append((stage, cand, cand.counters if debug is None else debug)); want.append(expected)
    for c in _contexts():
        for nDir in (0, 1):
            for limit in (0, 1): ask("SetIntensity", c.with_(inten=nDir, limit=limit), parent_set_intensity(c, nDir, limit))
        ask("SetOrders", c.with_(orders=1), parent_set_orders(c))
        ask("SetLevels", c.with_(levels=1), parent_set_levels(c, 1))
        ask("LevelsOff", c.with_(levels=0), parent_set_levels(c, 0))
        ask("SetDirect", c.with_(direct=1), parent_set_direct(c))
        ask("SetActinic", c.with_(actinic=1), parent_set_actinic(c))
        ask("SetSide", c.with_(side=1), parent_set_side(c))
        ask("SetBrdf", c.with_(brdf=1), parent_set_brdf(c))
        ask("SetCounters", c.with_(counters=1), parent_enable_counters(c))
        ask("Ready", c, parent_check_ready(c))
        ask("Trace", c, parent_compute(c))
        ask("Fates", c, parent_trace_fates(c), debug=1)
        for L, A in ((1, 1), (5, 1), (1, 5), (3, 3)):  # a new grid: other sizes, whatever the old ones were
            g = c.with_(L=L, A=A)
            ask("SetGrid", g, parent_set_grid(g))
    got = _refuse(exe, messages, asks)
    wrong = [(a[0], dict(a[1]), w, g) for a, w, g in zip(asks, want, got) if w != g]
    assert not wrong, wrong[:5]


def test_the_second_line_of_defence_refuses_the_same_settings(exe, messages):
    """launch_trace, over EVERY combination of the settings (a context cannot be in most of them): refused by the rule list exactly
    when the site's checks refused, with the site's message where one condition holds, and otherwise with the message of one of
    the conditions that hold (the site is never reached with even one: the list's order there is the order of check_ready); and nothing the checks before a trace let through is refused there"""
    import itertools
    asks = []
    for flags in itertools.product((0, 1), repeat=len(FLAGS)):
        c = Asked(dict(zip(FLAGS, flags)), L=1, D=1, A=1, S=1, O=1, rest=0, B=9)
        asks += [("Launch", c, 0), ("Launch", c, 1)]
    got = _refuse(exe, messages, asks)
    for (_, c, debug), g in zip(asks, got):
        says, holds = parent_launch_trace(c, debug)
        assert (g is None) == (says is None), (dict(c), debug, g, says)
        assert g is None or g in holds, (dict(c), debug, g, holds)
        assert len(holds) != 1 or g == says
        if parent_check_ready(c) is None and (parent_trace_fates(c) if debug else parent_compute(c.with_(counters=0))) is None and not (debug and (c.brdf or c.inten or c.orders)):
            assert g is None


# ---------------------------------------------------------------------------------------------------------------------------------
# the one question (mcbrat_settings_refusal): refusal() at the union of the setters' stages, and the order in which the Python
# integrator then calls the setters (mcbrat3d_amd/integrator.py: _push_order)
# ---------------------------------------------------------------------------------------------------------------------------------
QUESTION = ("SetIntensity", "SetOrders", "SetLevels", "SetDirect", "SetActinic", "SetSide", "SetBrdf")  # (LevelsOff stays out: its rules stand under SetDirect and SetSide)
UNION = sum(STAGES[s] for s in QUESTION)


def test_the_question_passes_every_state_a_context_can_be_in(exe, messages):
    """... but those whose order bins do not fit: a context gets there through set_grid only (mcbrat_specify_scattering_orders
    refuses the orders on such a grid, and a trace of that context refuses them again), an integrator never -- it sets its grid
    once, before any setting -- and the question says of them what the setter would"""
    states = _contexts()
    got = _refuse(exe, messages, [(UNION, c, c.counters) for c in states])
    for c, g in zip(states, got):
        assert g == ("kOrdersBudgetMsg" if c.orders and not c.O <= c.B else None), (dict(c), g)


def test_the_question_refuses_what_a_setter_refuses(exe, messages):
    """over EVERY combination of the settings, at sizes that fit: refused exactly when one of the setters' stages refuses the same
    settings, with the message of one of them -- and so with the rule's own where one rule holds (the allowance of the second
    line of defence above)"""
    import itertools
    asks = []
    for flags in itertools.product((0, 1), repeat=len(FLAGS)):
        c = Asked(dict(zip(FLAGS, flags)), L=1, D=1, A=1, S=1, O=1, rest=0, B=9)
        asks += [(UNION, c, c.counters)] + [(s, c, c.counters) for s in QUESTION]
    got = _refuse(exe, messages, asks)
    n = 1 + len(QUESTION)
    refused = 0
    for i in range(0, len(asks), n):
        union, single = got[i], {g for g in got[i + 1:i + n] if g is not None}
        assert (union is None) == (not single), (dict(asks[i][1]), union, single)
        assert union is None or union in single, (dict(asks[i][1]), union, single)
        refused += union is not None
    assert 0 < refused < len(asks) // n


def _push_steps(old, new):
    """_push_order's steps from the state old to the state new -> [(the step's own stage or None, the state after it)]; the
    intensity is always pushed and a BRDF surface given whenever new has one (a call may carry them unchanged: the steps of a
    call that does not are these without some that change nothing)"""
    from mcbrat3d_amd.integrator import _push_order
    fields = {"numRecScatOrd": "orders", "recLevelFluxes": "levels", "recDirectLevelFluxes": "direct", "recActinicFlux": "actinic", "recSideFluxes": "side"}
    on = {"orders": "SetOrders", "levels": "SetLevels", "direct": "SetDirect", "actinic": "SetActinic", "side": "SetSide"}
    value = lambda c, name: (2 if c.orders else -1) if name == "numRecScatOrd" else bool(c[fields[name]])  # noqa: E731
    held, wanted = ({name: value(c, name) for name in fields} for c in (old, new))
    out, state = [], old
    for step in _push_order(held, wanted, True, bool(new.brdf)):
        if step == "surface":
            stage, state = "SetBrdf", state.with_(brdf=1)
        elif step == "intensity":
            stage, state = "SetIntensity", state.with_(inten=new.inten, limit=new.limit)
        else:
            flag = fields[step]
            stage = on[flag] if new[flag] else ("LevelsOff" if flag == "levels" else None)  # (the other setters ask nothing when they switch off)
            state = state.with_(**{flag: new[flag]})
        out.append((stage, state))
    return out


def test_the_push_order_is_never_refused_on_the_way(exe, messages):
    """every ordered pair of states a context can be in, on one grid with the counters and the source as they are -- but a BRDF
    surface taken away, which the integrator cannot do, and a new state the question refuses (above): none of the setter calls
    from the old state to the new one is refused, and they end in the new state"""
    import collections
    groups = collections.defaultdict(list)
    for c in _contexts():
        groups[(c.L, c.D, c.A, c.S, c.O, c.rest, c.B, c.counters, c.emit)].append(c)
    pairs = 0
    lines = []
    for states in groups.values():
        for old in states:
            for new in states:
                if (old.brdf and not new.brdf) or (new.orders and not new.O <= new.B):
                    continue
                steps = _push_steps(old, new)
                assert steps[-1][1] == new, (dict(old), dict(new))
                lines += [(stage, state, state.counters, old, new) for stage, state in steps if stage]
                pairs += 1
    got = _refuse(exe, messages, [l[:3] for l in lines])
    wrong = [(stage, dict(old), dict(new), g) for (stage, _, _, old, new), g in zip(lines, got) if g is not None]
    assert not wrong, wrong[:5]
    assert pairs > 10000 and len(lines) > pairs


def test_the_push_order_needs_no_native_library():
    import sys
    code = "from mcbrat3d_amd.integrator import _push_order; from mcbrat3d_amd import _capi; assert _capi._lib is None"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=120)


def test_rule_precedence(exe, messages):
    """for every site, the rules of its stage stand in the list in the order of the site's checks"""
    by_text = messages
    rules = [l.split(" ", 1) for l in subprocess.run([exe, "rules"], check=True, capture_output=True, text=True).stdout.rstrip("\n").split("\n")]
    rules = [(int(stages, 16), by_text[text]) for stages, text in rules]
    for stage, order in PRECEDENCE.items():
        at = [name for stages, name in rules if stages & STAGES[stage]]
        assert set(at) == set(order) | UNORDERED.get(stage, set()), (stage, at)   # the stage has the site's rules, no others
        first = [at.index(name) for name in order]
        assert first == sorted(first), (stage, at)
    assert {n for _, n in rules} == set(by_text.values())  # every message constant is a rule's


def test_the_enumerated_launches_pass_the_rules(picked):
    """the pruning of scripts/kernel_choice.hip by the refusals is the rule list's: the only enumerated launches it refuses are the
    instrumented radiance and order runs, which the choosing part refused; every other one has a built kernel (above) -- settings
    that pass the rules always find their kernel in the table"""
    refused = {l.split("!", 1)[1] for l in picked if "!" in l}
    assert all(r.startswith("computeRadiativeTransfer: event counters / photon fates are not available together with") for r in refused) and len(refused) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the two kernel files the variants are instantiated from, and the header of what they share (mcbrat_photon.h)
# ---------------------------------------------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")


def test_the_block_walk_is_a_translation_unit_of_its_own(tmp_path):
    """mcbrat_blockwalk.hip declares what it uses: alone in a translation unit (nothing instantiated) the device compiler accepts it"""
    from mcbrat3d_amd import build
    tu = tmp_path / "blockwalk_alone.hip"
    tu.write_text('#include "mcbrat_blockwalk.hip"\n')
    subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-I", CSRC, str(tu)],
                   check=True, timeout=300)


# one distinctive expression of every rule both kernels take from mcbrat_photon.h: written there, and in neither kernel file
SHARED_RULES = {
    "source sampling, solar": "uMu = o[0] ? o[0]",
    "source sampling, thermal": "(j - 2) & 3u",
    "launch height": "(t - fl) * (",
    "Lambertian direction": "sinTheta * cphi",
    "slab flush": "unitSlab + i",
    "counters": "counters + 7",
    "fate record": "mcbrat_fate{",
}
# ... and of the rules that stay written out in both kernels, each copy naming the other: once in each
# kernel file (the component pick twice in the block walk, which picks again after its clamp), and not in the header
KEPT_IN_BOTH = {
    "Lambertian cosine": "float mu = sqrtf(uX);",
    "component pick": "c = k + 1",
    "roulette": "uR >= w",
    "scattering angle": "left * t[ai]",
    "new direction": "copysignf(fabsf(B), dz * B)",
    "leg draws": "0.693147182f * __builtin_amdgcn_logf",
}


def test_the_shared_photon_rules_are_written_once():
    header = open(os.path.join(CSRC, "mcbrat_photon.h")).read()
    kernels = {f: open(os.path.join(CSRC, f)).read() for f in ("mcbrat_kernels.hip", "mcbrat_blockwalk.hip")}
    for f, source in kernels.items():
        assert '#include "mcbrat_photon.h"' in source, f
    for rule, text in SHARED_RULES.items():
        assert text in header, rule
        for f, source in kernels.items():
            assert text not in source, (rule, f)
    for rule, text in KEPT_IN_BOTH.items():
        assert text not in header, rule
        assert kernels["mcbrat_kernels.hip"].count(text) == 1, rule
        assert kernels["mcbrat_blockwalk.hip"].count(text) == (2 if rule == "component pick" else 1), rule
    # both copies of the kept rules say where the other one is
    assert "HOT ROWS" in kernels["mcbrat_kernels.hip"] and "HOT ROWS" in kernels["mcbrat_blockwalk.hip"]
    # every function the header defines is called by both kernels (helpers only one kernel uses stay in its file)
    for name in ("launch_solar", "launch_emission", "launch_height", "lambert_direction", "flush_unit_slab", "publish_counters", "record_fate"):
        assert ("%s(" % name) in header
        for f, source in kernels.items():
            assert re.search(r"\b%s(<\w+>)?\(" % name, source), (name, f)
