"""CPU checks of the crafted decoder streams (tests/lz4_craft.py) that the
device tests of tests/test_gpu_decode_paths.py run:

* every payload of every family, at every block size used on the device,
  decodes the same with the byte-at-a-time decoder, the oracle and (where it
  is built) the compiled reference; the host build of the scan accepts it and
  the lane model of phase 2 rebuilds it;
* the families visit what they are for -- asserted from classify() / batches(),
  the restatement of the executor's dispatch and batching;
* the in-place decoder's margin test (csrc/inplace.h through the host build):
  which streams fail it, and that the value the scan hands over is the one it
  measured.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import lz4_craft as C
from tests.exec_model import exec_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")


class HostCheck:
    """lz4_scan.h and inplace.h as the device code uses them."""

    def __init__(self):
        if not os.path.exists(HOSTCHECK):
            import subprocess
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"), HOSTCHECK])
        lib = ctypes.CDLL(HOSTCHECK)
        ip = ctypes.POINTER(ctypes.c_int)
        self._scan = lib.bshuf_hostcheck_scan_mx
        self._scan.restype = ctypes.c_int
        self._scan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ip, ip, ip]
        self._place = lib.bshuf_hostcheck_inplace
        self._place.restype = ctypes.c_int
        self._place.argtypes = [ctypes.c_int] * 4 + [ip, ip]

    def scan(self, pay, n):
        """(result, token positions, mx as measured, mx as the decoder sees it)"""
        comp = np.frombuffer(bytes(pay), dtype=np.uint8)
        pos = np.zeros(comp.size // 3 + 2, dtype=np.uint32)
        cnt, raw, seen = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        r = self._scan(comp.ctypes.data, comp.size, n, pos.ctypes.data, ctypes.byref(cnt),
                       ctypes.byref(raw), ctypes.byref(seen))
        return r, pos[:cnt.value].copy(), raw.value, seen.value

    def fits(self, n, shift, span_bytes, mx):
        """Does a block of n bytes whose record span (span_bytes, starting
        `shift` bytes into a 16-byte granule) is placed in its buffer pass the
        in-place test?  Also checks the placement itself."""
        cap = (n + 15) & ~15
        end, off = ctypes.c_int(0), ctypes.c_int(0)
        ok = self._place(cap, shift, span_bytes, mx, ctypes.byref(end), ctypes.byref(off))
        assert end.value % 16 == 0 and end.value >= cap + C.IN_PLACE_MARGIN
        assert off.value % 16 == 0 and off.value >= 0, "the span starts inside the buffer"
        assert off.value + shift + span_bytes <= end.value
        return bool(ok)

    def last_block_fits(self, stream, pays, n):
        """The in-place verdict of the last block of a framed stream (its span
        runs to the stream's end, at most the largest record)."""
        o0 = sum(4 + len(p) for p in pays[:-1])
        span = min(len(stream) - o0, 4 + C.lz4_bound(n))
        r, _, raw, seen = self.scan(pays[-1], n)
        assert r == n and raw == seen
        return self.fits(n, o0 & 15, span, seen)


@pytest.fixture(scope="module")
def host():
    return HostCheck()


@pytest.fixture(scope="module")
def ref():
    import oracle as oracle_mod
    return oracle_mod.Reference() if oracle_mod.reference_available() else None


CASE_NAMES = sorted(C.cases())


# ----------------------------------------------------- every payload is valid
@pytest.mark.parametrize("name", CASE_NAMES)
def test_payloads_decode_scan_and_rebuild(oracle, ref, host, name):
    n, pays = C.cases()[name]
    assert pays
    for i, pay in enumerate(pays):
        comp = np.frombuffer(pay, dtype=np.uint8)
        assert comp.size <= C.lz4_bound(n)
        want = C.decode(pay, n)
        assert oracle.lz4_decompress_block(comp, n).tobytes() == want, (name, i)
        if ref is not None:
            assert ref.lz4_decompress_block(comp, n).tobytes() == want, (name, i)
        r, pos, raw, seen = host.scan(pay, n)
        assert r == n, (name, i, r)
        assert [int(p) for p in pos] == [s["tp"] for s in C.walk(pay)], (name, i)
        if n < C.BIG:   # (larger blocks are not decoded in LDS: no margin value)
            assert raw == seen, (name, i, raw, seen)
        assert exec_block(comp, pos, n).tobytes() == want, (name, i)


def test_decode_rejects_what_the_oracle_rejects(oracle):
    """decode() is a decoder, not an echo of the builder: an offset before the
    block start and a wrong length fail in both."""
    src = C.Lits(9)
    good = C.payload([(src.take(8), 8, 10)], src.take(6))
    bad = C.payload([(src.take(8), 9, 10)], src.take(6))
    assert C.decode(good, 24) == oracle.lz4_decompress_block(np.frombuffer(good, np.uint8), 24).tobytes()
    for pay, n in ((bad, 24), (good, 32)):
        with pytest.raises(ValueError):
            C.decode(pay, n)
    with pytest.raises(RuntimeError):
        oracle.lz4_decompress_block(np.frombuffer(bad, np.uint8), 24)
    # offset 0 writes zeros
    z = C.payload([(src.take(8), 0, 10)], src.take(6))
    assert C.decode(z, 24)[8:18] == bytes(10)
    assert oracle.lz4_decompress_block(np.frombuffer(z, np.uint8), 24).tobytes() == C.decode(z, 24)


# ------------------------------------------------------------------ coverage
def _match_cells_possible():
    """(label, mop & 3, (mop - off) & 3) that can exist.  Impossible: offset 0
    has no source (its cells are listed with source == destination); an offset
    of 1, 2 or 4 never puts the source 3 bytes (mod 4) behind the destination."""
    out = set()
    for lab in C.MATCH_LABELS:
        for d in range(4):
            for s in range(4):
                if lab == "wave_zero" and s != d:
                    continue
                if lab in ("lane_fill124", "wave_fill124") and (d - s) & 3 == 3:
                    continue
                out.add((lab, d, s))
    return out


@pytest.mark.parametrize("n", [8192, 1024])
def test_f1_visits_every_match_path_at_every_alignment(n):
    pays = C.cases()["f1_%d" % n][1]
    mc, _, _ = C.survey(pays)
    want = _match_cells_possible()
    assert want - mc == set()
    assert mc - want == set(), "a cell listed as impossible exists"
    seen = {(s["off"], s["ml"], s["mop"] & 3) for p in pays for s in C.walk(p) if s["ml"]}
    fit = [m for m in C.F1_MLS if m + 280 <= n]   # (n = 1024 cannot hold ml = 1000)
    assert len(fit) >= len(C.F1_MLS) - 1
    assert {(o, m, a) for o in C.F1_OFFS for m in fit for a in range(4)} <= seen


def test_f1_large_block_has_far_offsets_and_every_label():
    pays = C.cases()["f1_%d" % C.BIG][1]
    assert len(pays) <= 3
    mc, _, _ = C.survey(pays)
    assert {c[0] for c in mc} == set(C.MATCH_LABELS)
    seen = {(s["off"], s["ml"]) for p in pays for s in C.walk(p) if s["ml"]}
    assert {(o, m) for o in C.F1_OFFS + C.F1_FAR for m in C.F1_MLS} <= seen


def test_f2_visits_every_literal_path_at_every_alignment():
    n, pays = C.cases()["f2_8192"]
    _, lc, starts = C.survey(pays)
    # (every destination x source pair exists for every label: nothing impossible)
    assert {(lab, d, s) for lab in C.LIT_LABELS for d in range(4) for s in range(4)} - lc == set()
    lits = {s["lit"] for p in pays for s in C.walk(p)[:-1]}
    assert set(C.F2_LITS) <= lits
    assert {len(p) % 16 for p in pays} == set(range(16)), "payload lengths of every residue mod 16"
    assert len({o & 15 for o in starts}) >= 8
    # the arrangement blocks: long runs at 0, 1, 62, 63, 64, every rotation
    rots = set()
    arr = C.f2_arrangements(n)
    assert len(arr) == 7
    for p in arr:
        w = C.walk(p)
        assert len(w) >= 131 and any(C.walk(q)[:130] == w[:130] for q in pays), "part of f2"
        kind = "".join("L" if s["lit"] > 16 else "S" for s in w)
        assert all(kind[i] == "L" for i in C.F2_LONG_AT)
        # short runs between two long ones and long runs back to back
        assert "LSSL" in kind and "LLL" in kind and "SLS" in kind
        rots.add(kind[2:9])
    assert len(rots) == 7


def test_f3_length_fields():
    for name, ks in (("f3_8192", range(10)), ("f3_%d" % C.BIG, range(10))):
        pays = C.cases()[name][1]
        seqs = [s for p in pays for s in C.walk(p)]
        lits = {s["lit"] for s in seqs}
        mls = {(s["ml"] - C.MINMATCH, s["lit"]) for s in seqs if s["ml"]}
        for k in range(15):
            for last in (0, 254):
                assert 15 + 255 * k + last in lits
                assert any(m == 15 + 255 * k + last for m, _ in mls)
        if name == "f3_8192":
            # the offset inside (lit <= 5) and outside the token's 8-byte read
            assert {(15 + 255 * k + last, lit) for k in ks for last in (0, 254) for lit in range(8)} <= mls
    # terminating byte of an extension run on every window position: the first
    # window holds 7 bytes behind the token, later ones 8
    runs = {(s["lit"] - 15) // 255 for p in C.cases()["f3_8192"][1] for s in C.walk(p) if s["lit"] >= 15}
    assert {k for k in runs if k < 7} == set(range(7))
    assert {(k - 7) % 8 for k in runs if k >= 7} == set(range(8))


def _f4(n):
    return {name: C.walk(p) for name, p in C.f4_named(n)}


@pytest.mark.parametrize("n", [8192, 1024, C.BIG])
def test_f4_holds_every_dependency_pattern(n):
    f4 = _f4(n)

    def batch_of(w, j, rule="lds"):
        for chunk in C.batches(w, rule):
            for b in chunk:
                if j in b:
                    return b
    for ml in (6, 20):
        for d, same in ((-1, True), (0, True), (1, False)):
            w = f4["rend%+d_ml%d" % (d, ml)]
            assert w[1]["mop"] - w[1]["off"] + w[1]["ml"] == w[0]["mop"] + d
            assert (batch_of(w, 1) == batch_of(w, 0)) is same
            assert C.is_coop(w[1]["off"], w[1]["ml"]) is (ml == 20)
    prev = f4["src_in_prev_match"]
    s0, s1 = prev[0], prev[1]
    assert s0["mop"] <= s1["mop"] - s1["off"] and s1["mop"] - s1["off"] + s1["ml"] <= s0["mop"] + s0["ml"]
    s1 = f4["src_in_own_literals"][1]
    assert s1["op"] <= s1["mop"] - s1["off"] and s1["mop"] - s1["off"] + s1["ml"] <= s1["mop"]
    s1 = f4["src_straddles"][1]
    assert s1["mop"] - s1["off"] < s1["op"] < s1["mop"] - s1["off"] + s1["ml"] <= s1["mop"]
    s1 = f4["src_into_own_output"][1]
    assert s1["mop"] - s1["off"] < s1["op"] and s1["off"] < s1["ml"]
    for rule in ("lds", "big"):
        ch = C.batches(f4["chain64"], rule)
        assert len(ch[0]) == 64 and all(len(b) == 1 for b in ch[0])
        ch = C.batches(f4["independent64"], rule)
        assert len(ch[0]) == 1 and len(ch[0][0]) == 64
        w = f4["alternating"]
        ch = C.batches(w, rule)
        assert len(ch[0]) == 1
        kinds = [C.is_coop(w[j]["off"], w[j]["ml"]) for j in ch[0][0]]
        assert all(a != b for a, b in zip(kinds, kinds[1:])) and len(kinds) >= 30
        for lane in (0, 1, 62, 63):
            w = f4["self_overlap_lane%d" % lane]
            assert len(w) == 65 and w[lane]["off"] < w[lane]["ml"]
            assert batch_of(w, lane, rule)[0] == lane, "the self-overlapping match heads its batch"
    w = f4["dep_63_to_64"]
    assert w[63]["mop"] <= w[64]["mop"] - w[64]["off"] < w[63]["mop"] + w[63]["ml"]
    for cnt in (1, 2, 63, 64, 65, 128, 129):
        w = f4["nseq%d" % cnt]
        assert len(w) == cnt
    assert len(C.payload([], bytes(n))) > n, "a literal-only record is longer than its block"
    assert set(C.F4_BIG) <= set(f4)


def test_f5_one_fill_per_offset():
    for name, offs in (("f5_8192", C.F5_OFFS), ("f5_65536", C.F5_OFFS + C.F5_FAR),
                       ("f5_%d" % C.BIG, C.F5_BIG_OFFS), ("f5_%d" % C.LDS_TOP, C.F5_BIG_OFFS)):
        n, pays = C.cases()[name]
        got = []
        for p in pays:
            w = C.walk(p)
            assert len(w) == 2 and w[0]["lit"] == w[0]["off"] and w[0]["mop"] + w[0]["ml"] == n - 5
            got.append(w[0]["off"])
        # an offset whose literals end behind n - 12 cannot be followed by a match
        assert got == [o for o in offs if o <= n - 12 and n - 5 - o >= C.MINMATCH]
        assert len(got) >= len(offs) - 2
    # small_mod's domain: ml in the tens of thousands against odd periods
    assert any(C.walk(p)[0]["off"] % 2 == 1 and C.walk(p)[0]["ml"] > 60000
               for p in C.cases()["f5_65536"][1])


# ------------------------------------------------------ the in-place margin
def _adversarial(n):
    """Records that push the in-place test hardest: the output as far ahead of
    the record as possible early on (one long match first), the largest
    literal-length overhead at the end (one long literal run last, or a
    literal-only record), many minimal sequences."""
    out = [C.payload([], C.Lits(n).take(n))]
    for last in (5, 270, n // 2, n - 40):
        b = C.Block(n, C.Lits(n + last))
        if n - 1 - last >= C.MINMATCH and b.fits(1, n - 1 - last):
            b.add(1, 1, n - 1 - last)
            out.append(b.close())
    if n >= 64:
        b = C.Block(n, C.Lits(n + 1))
        b.add(n // 3, 8, 4)
        out.append(b.close())
        b = C.Block(n, C.Lits(n + 2))
        b.add(8, 8, 4)
        while b.fits(0, 4, 16):
            b.add(0, 8, 4)
        out.append(b.close())
    return out


def _margin_payloads():
    out = []
    for n in (16, 64, 1024, 8192, 65536, 81600):
        out += [(n, p) for p in _adversarial(n)]
    for name, (n, pays) in C.cases().items():
        if n <= 65536:
            out += [(n, p) for p in pays[::3]]
    return out


def test_in_place_margin_holds_for_every_block_but_a_last_one_with_a_long_tail(host):
    """Case A of the two the margin question allowed: valid streams DO fail the
    in-place test, but only a stream's LAST block, whose span runs on over the
    raw tail: the record then lands `tail` bytes further down the buffer.  A
    record that ends its span (every other block, at any of the 16 shifts) and
    a last block whose tail t has t + n / 255 + 2 + 15 <= 704 always pass; so
    the global-record fallback needs a tail of more than 430 (64 KiB blocks) to
    655 bytes (8 KiB blocks), i.e. 7 tail elements of 62 bytes and more each."""
    fails = []
    for n, pay in _margin_payloads():
        r, _, raw, seen = host.scan(pay, n)
        assert r == n and raw == seen
        cap_span = 4 + C.lz4_bound(n)
        for shift in range(16):
            assert host.fits(n, shift, 4 + len(pay), seen), (n, len(pay), shift)
        safe = C.IN_PLACE_MARGIN - 15 - (n // 255 + 2)
        tails = sorted({k * E for E in (1, 2, 3, 4, 8, 12, 16, 24, 53, 64, 82, 100, 128, 256, 512, 1024)
                        for k in range(8)} | set(range(safe - 40, 760, 3)) | {safe})
        for t in tails:
            if t < 0:
                continue
            span = min(4 + len(pay) + t, cap_span)
            for shift in (range(16) if t >= safe - 40 else (0, 7, 15)):
                ok = host.fits(n, shift, span, seen)
                assert ok or t > safe, (n, len(pay), t, shift)
                if not ok:
                    fails.append((n, t))
    assert fails and min(t for _, t in fails) > 430
    assert min(t for nn, t in fails if nn == 8192) > 655
    assert any(t < 800 for _, t in fails)


def test_f7_sweeps_the_in_place_threshold(host):
    side = {True: 0, False: 0}
    for E in C.F7_ES:
        st, pays, n = C.f7(E)
        side[host.last_block_fits(st, pays, n)] += 1
        # every block but the last is decoded in place
        r, _, raw, seen = host.scan(pays[0], n)
        assert host.fits(n, 0, 4 + len(pays[0]), seen)
    assert side[True] >= 8 and side[False] >= 8, side
    # ... and at a block size where the margin value exceeds 16 bits
    st, pays, n = C.f7(*C.F7_LARGE)
    assert not host.last_block_fits(st, pays, n)
    assert host.scan(pays[-1], n)[2] > 0xFFFF - (1 << 14)
