"""The owners of the host library's allocations (mcbrat3d_amd/csrc/mcbrat_devmem.h) without a GPU.

tests/device_buffer_check.cpp, which includes nothing of the project but that header and defines the seam functions over malloc and
free, is compiled with the host C++ compiler and prints one line per scenario: what the scenario did to the count of allocations,
of frees and of live blocks.  The lines are compared with what the rules of the header say (written out below, not taken from a
run), for DeviceBuffer and for PinnedBuffer; then the same program is built with the undefined-behaviour and address sanitizers,
leak checker included, and must print the same (a stand-alone program: nothing is loaded into Python).  Last, a text check:
the allocation calls of the HIP runtime occur in the seam definitions of mcbrat_api.hip and nowhere else under csrc/."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")

# {who}: device, pinned.  Every allocs / frees / live is the change the scenario made; capacity is in elements (9 elements of 8 bytes)
SCENARIOS = """\
{who} allocate twice, same size: status=0,0 full=1 capacity=8 allocs=2 frees=1 live=1
{who} allocate for no elements: status=0 nonnull=1 capacity=1 allocs=1 frees=0 live=1
{who} reserve: status=0,0,0 smaller kept=1 equal kept=1 (allocs=0 frees=0) larger capacity=9 bytes=72 allocs=1 frees=1 live=0
{who} failing allocate, empty buffer: status=2 full=0 null=1 capacity=0 allocs=0 frees=0 live=0
{who} failing reserve, empty buffer: status=2 full=0 null=1 capacity=0 allocs=0 frees=0 live=0
{who} failing allocate, full buffer: status=2 full=0 null=1 capacity=0 allocs=0 frees=1 live=-1
{who} failing reserve, full buffer: status=2 full=0 null=1 capacity=0 allocs=0 frees=1 live=-1
{who} move construction: source empty=1 capacity=0 target holds=1 capacity=4 allocs=1 frees=0 live=1
{who} move assignment over a full buffer: source empty=1 capacity=0 target holds=1 capacity=4 allocs=1 frees=1 live=0
{who} self-move: holds=1 capacity=4 allocs=0 frees=0 live=0
{who} three buffers, the second allocation fails: status=2 allocs=1 frees=1 live=0
{who} reset twice: empty=1 capacity=0 allocs=1 frees=1 live=0
"""
EXPECTED = (SCENARIOS.format(who="device") + SCENARIOS.format(who="pinned") +
            "end: device live=0 allocs-frees=0 pinned live=0 allocs-frees=0\n").splitlines()


def _compile(out, *flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, os.path.join(ROOT, "tests", "device_buffer_check.cpp")])
    return out


def _lines(exe):
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _lines(_compile(str(tmp_path_factory.mktemp("devmem") / "device_buffer_check")))


def test_every_scenario_leaves_the_counts_the_rules_give(plain):
    assert plain == EXPECTED


def test_the_sanitized_program_prints_the_same_and_leaks_nothing(plain, tmp_path):
    exe = _compile(str(tmp_path / "device_buffer_check_san"), "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
    assert _lines(exe) == plain  # (check=True: a finding of a sanitizer, a leak among them, ends the program with a failure status)


def test_the_check_program_includes_only_the_header():
    text = open(os.path.join(ROOT, "tests", "device_buffer_check.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../mcbrat3d_amd/csrc/mcbrat_devmem.h"]
    header = open(os.path.join(CSRC, "mcbrat_devmem.h")).read()
    assert not re.search(r'#include\s+[<"]hip', header) and not re.findall(r'#include\s+"', header)  # plain C++, no HIP, nothing of the project


ALLOCATION_CALLS = r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b"


def test_the_runtime_allocation_calls_occur_only_in_the_seam():
    api = open(os.path.join(CSRC, "mcbrat_api.hip")).read()
    # the seam: the one `namespace mcbrat { ... }` block of the file, which defines the four functions the header declares
    blocks = re.findall(r"^namespace mcbrat \{\n.*?^\}  // namespace mcbrat\n", api, flags=re.S | re.M)
    assert len(blocks) == 1
    seam = blocks[0]
    for name in ("int device_alloc(void **ptr, size_t bytes) {", "void device_free(void *ptr) {", "int pinned_alloc(void **ptr, size_t bytes) {",
                 "void pinned_free(void *ptr) {"):
        assert seam.count(name) == 1, name
    assert {m for m in re.findall(ALLOCATION_CALLS, seam)} == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"}
    assert re.findall(ALLOCATION_CALLS, api.replace(seam, "")) == []
    others = [f for f in sorted(os.listdir(CSRC)) if f != "mcbrat_api.hip" and f.endswith((".hip", ".h", ".cpp"))]
    assert "mcbrat_kernels.hip" in others and "mcbrat_devmem.h" in others
    for f in others:
        assert re.findall(ALLOCATION_CALLS, open(os.path.join(CSRC, f)).read()) == [], f
