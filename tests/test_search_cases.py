"""The crafted blocks of tests/search_cases.py, settled on the CPU: every
family's census (tests/parse_census.py) holds each event it is meant to hold,
for every element size the GPU test (test_gpu_search_cases.py) runs it with,
and the instrumented serial parse gives the oracle's sequences on every block.
A layout that lost its event fails here, without a GPU.

Reached catch-ups that stop at block position 0 (the longest the layouts
give): 15 bytes in the default block of every element size, 63 bytes in a
32 KiB block.
"""
import pytest

from tests import search_cases as S
from tests.emit_model import parse_record
from tests.parse_census import WIDE_LIMIT, census, parse


def checked(oracle, blocks):
    """Events of all blocks; the serial parse must be the oracle's."""
    ev = []
    for i, b in enumerate(blocks):
        seqs, la, e = parse(b, traffic=True)
        want, wla = parse_record(oracle.lz4_compress_block(b), b.size)
        assert seqs == want and la == wla, i
        ev += e
    return ev


@pytest.mark.parametrize("E", [2, 4, 3])
def test_a_catch_up_lengths(oracle, E):
    n = S.block_bytes(oracle, E)
    cases = S.catchup_cases(n)
    ev = checked(oracle, [b for b, _ in cases])
    c = census(ev)
    assert {(t, "mismatch") for t in S.A_BACKS} <= c["back_stop"], sorted(c["back_stop"])
    assert any(b >= 192 and s == "mismatch" for b, s in c["back_stop"])
    # search_entry's back = -1 together with the count's `while (c0 == kWinBytes)`
    assert any(e["back"] >= 64 and e["count"] >= 256 for e in S.searches(ev))
    ev = checked(oracle, [b for b, _ in S.anchor_cases(n)])
    c = census(ev)
    assert {(t, "anchor") for t in (1, 2, 3, 63, 64, 65)} <= c["back_stop"], sorted(c["back_stop"])
    assert all(e["lit"] == 0 for e in S.searches(ev) if e["stop"] == "anchor")
    blk, back = S.block_start_case(n)
    assert (back, "zero") in census(checked(oracle, [blk]))["back_stop"] and back >= 8, back
    blk, back = S.block_start_case(S.block_bytes(oracle, E, 32768))
    assert (back, "zero") in census(checked(oracle, [blk]))["back_stop"] and back >= 16, back


@pytest.mark.parametrize("E", [2, 3])
def test_b_probe_schedule(oracle, E):
    n = S.block_bytes(oracle, E)
    c = census(checked(oracle, [S.probe_cases(n)]))
    assert {(w, l) for w in (0, 1, 2, 4) for l in (0, 1, 62, 63)} <= c["hits"], sorted(c["hits"])
    assert {64, 65} <= c["probes"]
    ends = S.block_end_cases(n)
    ev = {k: checked(oracle, [b]) for k, b in ends.items()}
    limit, mlimit = n - 11, n - 5

    def runout(name):
        return [(e["window"], e["valid"]) for e in ev[name] if e["kind"] == "runout"]
    assert runout("runout_1") == [(1, 1)] and runout("runout_1_w0") == [(0, 1)]
    assert runout("runout_63") == [(0, 63)]
    assert any(e["at_limit"] and e["last_valid"] and e["valid"] < 64 for e in S.searches(ev["hit_at_limit"]))
    assert any(e["last_valid"] and e["window"] == 1 and not e["at_limit"] for e in S.searches(ev["last_lane_w1"]))
    assert any(e["at_mlimit"] for e in S.searches(ev["ends_at_mlimit"]))
    assert any(e["ip"] + e["ml"] == mlimit - 1 for e in S.searches(ev["ends_at_mlimit_1"]))
    for name, hit in (("retest_at_limit_miss", False), ("retest_at_limit_hit", True)):
        assert any(e["kind"] == "retest_try" and e["ip"] == limit - 1 and e["hit"] == hit for e in ev[name]), name
    assert any(e["kind"] == "retest" and e["at_limit"] for e in ev["retest_at_limit_hit"])


@pytest.mark.parametrize("n", [16, 24, 32, 40])
def test_b_blocks_around_the_minimum_length(oracle, n):
    seen, unseen = S.tiny_cases(n)
    ev = checked(oracle, [seen])
    assert [e["mpos"] for e in S.searches(ev)] == [n - 12]      # limit - 1: the last probe
    ev = checked(oracle, [unseen])
    assert not S.searches(ev) and unseen[n - 11:n - 7].tobytes() == unseen[n - 15:n - 11].tobytes()


@pytest.mark.parametrize("E", [2, 3])
def test_c_window_traffic(oracle, E):
    n = S.block_bytes(oracle, E)
    first, second = S.window_cases(n)
    ev = checked(oracle, [first])
    s = S.searches(ev)
    # the source in the hit's own window, `off` lanes in front (step 1)
    assert {1, 2, 3, 4, 63} <= {e["off"] for e in s if e["window"] == 0 and e["off"] <= e["lane"]}
    assert any(e["k"] == 64 and e["off"] == 1 for e in s)        # lane 63 -> lane 0 of the next window
    c = census(ev)
    assert (2, True, False) in c["same_slot"]                    # lanes <= js, equal bytes
    # (origin, later lanes on the slot, observed, deciding)
    assert any(x[0] == "old" and x[2] and x[3] for x in c["restores"])
    assert any(x[0] == "inwin" and x[2] and x[3] for x in c["restores"])
    c = census(checked(oracle, [second]))
    assert {(2, False, True), (3, False, True)} <= c["same_slot"]            # all before js
    # around js: (lanes <= js, lanes > js, all bytes different), groups of two and three
    assert {(1, 1, True), (2, 1, True)} <= c["spanning"], sorted(c["spanning"])
    assert any(x[0] == "inwin" and x[2] for x in c["restores"])              # ... and its restore is read
    assert {("old", 2, True, False), ("old", 3, True, False)} <= c["restores"]   # all behind js
    assert ("old", 3, True, True) in c["restores"]               # later lanes share the slot: deciding


@pytest.mark.parametrize("E", [2, 3])
def test_d_count_window_edges(oracle, E):
    n = S.block_bytes(oracle, E)
    ev = checked(oracle, S.count_cases(n))
    c = census(ev)
    want = set(S.D_COUNTS) | {4}
    assert want <= c["search_counts"], sorted(want - c["search_counts"])
    assert want <= c["retest_counts"], sorted(want - c["retest_counts"])
    # kPcSlow: counts of 252..257 and 508..513 from the count's origin
    slow = {e["count"] for e in ev if e["kind"] in ("search", "retest") and e["slow"]}
    assert slow & want == set(range(252, 258)) | set(range(508, 514)), sorted(slow)
    assert c["slow_retests"] >= 12 and c["slow_retest_hits"] >= 6
    # kPcLong: re-test counts that end at 256 and at 257
    assert {256, 257} <= c["retest_counts"]


@pytest.mark.parametrize("E,n", [(1, 98304), (3, 98304), (1, 262144), (3, 262152)])
def test_e_distance_rule(oracle, E, n):
    assert n % (8 * E) == 0 and n >= WIDE_LIMIT
    ev = checked(oracle, [S.far_case(n)])
    c = census(ev)
    assert {("search", True), ("retest", True)} <= c["far"]      # the check decides
    assert c["far65535"] == {"search", "retest"}                 # exactly 65,535: accepted
    assert {65534, 65535} <= c["offsets"] and not c["offsets"] & {65536, 65537, 70000}
    # behind a rejection the third copy reads the entry the rejected probe left
    assert {9000 + 300 * i for i in (2, 3, 4, 7, 8, 9)} <= c["offsets"], sorted(c["offsets"])


@pytest.mark.parametrize("E,n", [(1, 65552), (3, 65568)])
def test_e_distance_rule_in_the_smallest_wide_block(oracle, E, n):
    """One far copy per block: its source is position 2, the copy stands in the
    block's last 20 bytes.  Distance 70,000 and a third copy cannot fit."""
    assert n % (8 * E) == 0 and n >= WIDE_LIMIT > n - 8 * E
    for retest in (False, True):
        where = "retest" if retest else "search"
        for dist in (65534, 65535, 65536, 65537):
            ev = checked(oracle, [S.small_far_case(n, dist, retest)])
            c = census(ev)
            if dist <= 65535:
                assert any(e["kind"] == where and e["off"] == dist for e in ev), (where, dist)
                assert (where in c["far65535"]) == (dist == 65535)
            else:
                assert any(e["kind"] == "far" and e["where"] == where and e["equal"] and
                           e["pos"] - e["cand"] == dist for e in ev), (where, dist)
                assert dist not in c["offsets"]


@pytest.mark.parametrize("E,n", [(1, 65536), (1, 65544), (3, 65544), (1, 65552), (3, 65568)])
def test_e_table_type_boundary(oracle, E, n):
    assert n % (8 * E) == 0
    ev = checked(oracle, [S.boundary_case(n)])
    s = [e for e in ev if e["kind"] in ("search", "retest")]
    assert any(e["off"] > 60000 for e in s) and any(e["ip"] - e["off"] > 65000 for e in s)
    assert any(e["back"] >= 64 for e in S.searches(ev))
    assert (n >= WIDE_LIMIT) == (n >= 65552)
