"""The tallies of a small run, bit for bit what they were before the tally layout moved into csrc/mcbrat_layout.h.

tests/golden/tally_layout_parent.npz was written by scripts/record_tally_golden.py on the commit before that change (and seen to be
the same in two runs there): per case the whole moment array, momentsLength() and every array reportResults() returns.  A part of
the slab, of the moments or of the per-batch scratch that moved by one element shows here as different bits."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_tally_golden", os.path.join(ROOT, "scripts", "record_tally_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "tally_layout_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_every_case_of_the_recorder_is_in_the_file(golden):
    assert {k.split("/")[0] for k in golden} == set(R.CASES)


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_same_bits_as_before_the_layout_header(golden, name):
    import mcbrat3d_amd
    got = R.run_case(mcbrat3d_amd, name)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert set(got) == set(want) and "moments" in got and len(got) >= 2 + 8
    assert int(got["momentsLength"]) == int(want["momentsLength"]) and got["moments"].size == 8 + 2 * int(want["momentsLength"])
    assert np.all(got["moments"][8:8 + 3] > 0)  # (something was traced)
    for k in sorted(want):
        a, b = np.asarray(got[k]), want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), "%s: %s: %d of %d elements differ" % (name, k, int((a != b).sum()), a.size)
