"""The bytes that the workspace-size functions of the range decode, the window
decode of one stream and of a set of streams, and the stream set return,
against a recording (tests/golden/window_workspace.json, written by
tests/golden/make_window_workspace.py): the layouts behind them share their
carving code, and this is the check that none of them lost or gained a buffer.
No device is touched."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_workspace_bytes_are_the_recorded_ones():
    import bitshuffle_amd as B
    spec = importlib.util.spec_from_file_location("make_window_workspace",
                                                  os.path.join(GOLDEN, "make_window_workspace.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(GOLDEN, "window_workspace.json")) as f:
        golden = json.load(f)
    assert golden["grid"] == json.loads(json.dumps(rec.GRID)), "the recording is of another grid"
    got = rec.walk(B.lib, golden["grid"])
    assert sorted(got) == sorted(golden["values"])
    for name, want in golden["values"].items():
        assert len(got[name]) == len(want), name
        diff = [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b]
        assert not diff, "%s: %d of %d values differ, first at %d: %d, recorded %d" % (
            name, len(diff), len(want), diff[0], got[name][diff[0]], want[diff[0]])
    # the grid holds refused shapes (0) and served ones, with the shared and the
    # private token-position area
    for name, want in golden["values"].items():
        assert 0 in want and max(want) > 0, name
