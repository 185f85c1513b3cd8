"""tools/launch_trace.py: the normalised launch list of the recorded training step is a function of the plan alone — the same for
two fresh plans in one process (addresses are renamed in order of first appearance) — and it sees a change of schedule.  Emulator
build only: the digest is what two checkouts are compared by, no value of it is pinned here."""
import os
import sys

import pytest

from conftest import ROOT, _build_emulator

sys.path.insert(0, os.path.join(ROOT, "tools"))
import launch_trace                                                  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    """The SIMT-emulator build bound for this module's tests; whatever library was bound before is bound again afterwards."""
    from streamyolo_amd import _lib
    before = (_lib._lib, _lib._lib_path)
    _lib.use_library(_build_emulator())
    assert _lib.is_emulator()
    yield "cpu"
    _lib._lib, _lib._lib_path = before


@pytest.fixture(scope="module")
def traces(emu):
    """nano, 2 x 32 x 64, fp32: the one-launch backward twice (two fresh models and plans), the split backward once."""
    run = lambda bwd: launch_trace.trace("nano", (2, 32, 64), "fp32", emu, [("BWD_SPLIT_FRAMES", bwd)])      # noqa: E731
    return run("0"), run("0"), run("1")


def test_two_fresh_plans_give_the_same_digest(traces):
    a, b, _ = traces
    assert a == b and launch_trace.digest(a) == launch_trace.digest(b)
    calls = [e for e in a if not e.startswith(("mark ", "snippet"))]
    assert len(calls) > 500 and any(e.startswith("sy_conv2d(") for e in calls) and any(e.startswith("mark join") for e in a)
    assert not any("0x" in e for e in a)                             # nothing address-like is left in an entry
    import re
    assert all(abs(int(v)) < 1 << 32 for e in calls for v in re.findall(r"(?<![\w.])-?\d+(?![\w.])", e))


def test_the_digest_changes_with_the_backward_schedule(traces):
    a, _, c = traces
    assert launch_trace.digest(a) != launch_trace.digest(c)
    assert len(c) > len(a)                                           # per-frame launches and their stream marks


def test_switches_are_put_back_and_proxies_removed(traces):
    from streamyolo_amd import _lib, train_engine
    assert train_engine.BWD_SPLIT_FRAMES == os.environ.get("STREAMYOLO_BWD_SPLIT_FRAMES", "auto")
    assert _lib.lib.__module__ == _lib.__name__ and _lib.NativeTape.mark.__module__ == _lib.__name__
