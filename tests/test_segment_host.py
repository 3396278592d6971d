"""What tests/test_gpu_segments.py rests on, checked without a GPU: every geometry its cases are written for is really in
their collections.  All of it is read from the CPU oracle's output (tests/segment_model.py: segments() and runs() from the
LCP array, the designed reads' rows from the suffix array): sizes and size classes, positions relative to the chunk border
and the look-ahead, the per-class counts above the launch grids, the slots and sub-segments every radix round leaves,
K = 65536 / 65537 tied sub-segments.  The model's constants are held to the #define lines of the sources."""
import os
import re
import numpy as np
import pytest
from tests import segment_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bfqzip_amd", "csrc")


def _out(orc, case):
    bwt, qs, lcp, sa = orc.build_ebwt(case.b, case.q, case.r, want_sa=True)
    assert len(bwt) == case.n
    return lcp, sa, sm.segments(lcp)


def _designed(orc, case, tag=1):
    """(lcp, all segments, (first, rows) of the segment of the reads with that tag)."""
    lcp, sa, segs = _out(orc, case)
    return lcp, segs, sm.segment_of(segs, sm.read_rows(sa, case, tag))


def _huge(segs):
    return [(int(a), int(s)) for a, s in segs if s > sm.HUGE]


# ---------------------------------------------------------------------------------------------------- the constants
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert len(m) == 1, (name, m)
    return int(m[0])


def test_constants_match_the_sources():
    refine, scan = _src("k_refine.hip"), _src("k_scan.hip")
    assert _define(refine, "RF_CHUNK") == sm.RF_CHUNK
    assert _define(refine, "RB_SMALL") == sm.RB_SMALL
    assert _define(_src("bfq_internal.h"), "BFQ_HUGE_SEG") == sm.HUGE
    assert _define(_src("bfq_common.h"), "BFQ_KEY_SYMS") == sm.KEY
    assert _define(_src("bfq_common.h"), "BFQ_SYMS_PER_WORD") == sm.WORD
    assert _define(scan, "SC_THREADS") * _define(scan, "SC_ITEMS") == sm.SCAN_TILE
    val = {"RB_SMALL": sm.RB_SMALL, "2 * RB_SMALL": 2 * sm.RB_SMALL, "BFQ_HUGE_SEG": sm.HUGE}
    launches = re.findall(r"^\s*RB_LAUNCH\((\d+), ([^,]+), ([^,]+), (true|false), (\d+)\);", refine, re.M)
    assert len(launches) == 5
    got = [(int(nt), val.get(lo) or int(lo), val.get(hi) or int(hi), int(grid)) for nt, lo, hi, first, grid in launches]
    assert got == [(nt, lo - 1, hi, grid) for nt, (lo, hi), grid in zip(sm.THREADS, sm.CLASSES, sm.GRIDS)]
    assert [x[3] for x in launches] == ["true"] + ["false"] * 4                     # the end search is the first launch's
    assert "if (li0 >= RF_CHUNK + %d)" % sm.LOOK in refine                          # the look-ahead
    assert "wi < RF_CHUNK / 64 + 2;" in refine and sm.LOOK == 2 * 64                # ... and the head words that are searched
    assert "b0 += NT * 8" in refine and 64 * 8 == 512                               # the 512-row scan of the first launch
    assert "c0 += NT" in refine
    big = _src("k_bigseg.hip")
    assert "nsub <= (1ull << 16) ? 2 : 4" in big and sm.PASS_SWITCH == 1 << 16
    assert "depth += BFQ_KEY_SYMS" in big                                           # a radix round is 16 symbols


def test_the_model_reads_segments_like_the_sorted_keys():
    """segments() from the LCP against the runs of equal 16-symbol keys without a terminator, on a hand-made LCP."""
    lcp = np.array([0, 16, 20, 15, 16, 0, 3, 99, 16, 16], np.uint32)
    assert sm.segments(lcp).tolist() == [[0, 3], [3, 2], [6, 4]]
    assert sm.runs(lcp, 17, 0, 10).tolist() == [[1, 2], [6, 2]]
    assert sm.runs(lcp, 16, 7, 3).tolist() == [[7, 3]]                               # the range's first row joins nothing
    assert sm.segments(np.zeros(0, np.uint32)).shape == (0, 2)
    assert [sm.class_of(x) for x in (64, 65, 128, 129, 512, 513, 2048, 2049)] == [None, 0, 0, 1, 2, 3, 4, 5]
    assert [sm.padded(x) for x in (65, 128, 129, 2047, 2048)] == [128, 128, 256, 2048, 2048]


# ---------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("form", [1, 2, 4])
def test_part_a_sizes_and_classes(orc, form):
    classes = set()
    for g in sm.G_ALL if form < 4 else sm.G_BORDER:
        case = sm.class_case(g, form)
        lcp, segs, (st, sz) = _designed(orc, case)
        assert sz == g and 65 <= g <= sm.HUGE, case
        k = sm.class_of(sz)
        assert sm.CLASSES[k][0] <= g <= sm.CLASSES[k][1] and sm.padded(g) in (128, 256, 512, 1024, 2048)
        classes.add((k, sm.padded(g) == g, sm.CLASSES[k][0] == g))
        inner = lcp[st + 1:st + sz]
        if form == 1:
            assert (inner == sm.KEY).all()                                          # identical reads: only the read index decides
        if form == 2:                                                               # both words of a round decide somewhere
            assert ((inner >= sm.KEY) & (inner < sm.KEY + sm.WORD)).any()
            assert ((inner >= sm.KEY + sm.WORD) & (inner < sm.KEY + 2 * sm.WORD)).any()
            assert (inner >= sm.KEY + 2 * sm.WORD).any() and len(set(inner.tolist())) >= 15      # later rounds; real sorting
        if form == 4:
            rr = sm.runs(lcp, sm.KEY + 2 * sm.WORD, st, sz)                         # tied behind round 0
            sub = set(rr[:, 1].tolist())
            assert 2 in sub and max(sub) > 64 and int(rr[:, 1].sum()) < sz          # sizes 2, > 64 and rows on their own
            alone = np.ones(sz, bool)
            for a, s in rr:
                alone[a - st:a - st + s] = False
            beside = alone[:-1] != alone[1:]
            assert beside.sum() >= 2                                                # ... side by side
            assert (inner == sm.KEY + 50).sum() >= 69                               # exact copies (tied to the terminator)
            assert (inner == sm.KEY + 44).any()                                     # ... among near copies
            assert (inner == sm.KEY + 10).sum() >= 2                                # a terminator inside round 0's first word
    assert {k for k, _, _ in classes} == {0, 1, 2, 3, 4}
    assert {k for k, full, _ in classes if full} == {0, 1, 2, 3, 4}                 # no padding slot at all
    assert {k for k, _, low in classes if low} >= ({0, 1, 2, 3, 4} if form < 4 else {1, 2, 3, 4})


def test_part_a_deciding_symbol(orc):
    """Form 3: LCP values of exactly 16 + D inside the segment, for D on both sides of the word border (16 + 21), the round
    border (16 + 42) and in rounds 2 and 3."""
    assert {(sm.KEY + D - sm.KEY) // sm.WORD for D in sm.DS} == {0, 1, 2, 4} and 21 in sm.DS and 42 in sm.DS and 84 in sm.DS
    assert {D // (2 * sm.WORD) for D in sm.DS} == {0, 1, 2}                         # rounds 0 (behind the key), 1 and 2 of 42 symbols
    for g in sm.G_BORDER:
        for D in sm.DS:
            case = sm.class_case(g, 3, D)
            lcp, segs, (st, sz) = _designed(orc, case)
            assert sz == g, case
            inner = lcp[st + 1:st + sz]
            assert int(inner.min()) == sm.KEY + D and (inner == sm.KEY + D).sum() >= 3, case
            assert (inner > sm.KEY + D).any(), case


# ---------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("name", [x[0] for x in sm.PART_B])
def test_part_b_positions(orc, name):
    case = sm.part_b(name)
    lcp, segs, (st, sz) = _designed(orc, case)
    end, n = st + sz, case.n
    border = (st // sm.RF_CHUNK + 1) * sm.RF_CHUNK
    assert sz == case.g and st == case.head and border == case.border
    assert st == border - case.d and (case.d < sm.RF_CHUNK or st % sm.RF_CHUNK == 0)
    assert (end == n) == (case.kind == "T")
    if case.kind == "G":
        assert n - end == case.behind and lcp[end] == 0                             # a head on the row behind the segment
    known = sm.length_known(st, end)
    if name.startswith("end_1"):
        assert end - border == int(name[4:]) and known == (end - border <= sm.LOOK - 1)
    if name == "last_row":
        assert st % sm.RF_CHUNK == sm.RF_CHUNK - 1 and not known
    if name.startswith("row0"):
        assert st % sm.RF_CHUNK == 0 and known == (sz <= sm.RF_CHUNK + sm.LOOK - 1)
        assert -(-(border - st - 1) // 512) == 4                                   # steps of the 512-row scan over the chunk's rest
    if name == "end_on_border":
        assert end % sm.RF_CHUNK == 0 and end < n and not known
    if name == "no_head_chunk":
        assert st < border and end > border + sm.RF_CHUNK and not known             # chunk `border / RF_CHUNK` holds no head
    if name.startswith("end_T") or name.startswith("end_G"):
        res = int(name.split("_")[2][1:])
        assert n % sm.RF_CHUNK == res and end % sm.RF_CHUNK == res and not known
    assert {x[0] for x in sm.PART_B} >= set(sm.PART_B_PILES)


def test_part_b_known_and_searched_both_occur():
    """From the builders' own numbers (asserted equal to the oracle's above): which cases the first launch has to search."""
    known = {x[0]: x[2] - x[3] <= sm.LOOK - 1 if x[3] < sm.RF_CHUNK else x[2] <= sm.RF_CHUNK + sm.LOOK - 1 for x in sm.PART_B}
    assert known["end_127"] and not known["end_128"] and not known["end_129"]
    assert known["row0_513"] and known["row0_1025"] and known["row0_2047"] and not known["row0_2177"]
    assert sum(known.values()) == 4


def test_part_b_more_than_64_chunks(orc):
    case = sm.part_b(sm.LONG[0])
    lcp, segs, (st, sz) = _designed(orc, case)
    assert sz == 140_000 and st + sz == case.n and 2_500_000 < case.n < 2_600_000
    whole = (st + sz) // sm.RF_CHUNK - (st // sm.RF_CHUNK + 1)                      # chunks without a head behind the head's
    assert 64 < whole <= 128                                                        # found in the second step of 64 chunks


# ---------------------------------------------------------------------------------------------------- part C
def test_part_c_more_segments_than_workgroups(orc):
    case = sm.grids_case()
    lcp, sa, segs = _out(orc, case)
    assert 9_000_000 < case.n < 11_000_000
    sizes = segs[:, 1]
    for (lo, hi), grid in zip(sm.CLASSES, sm.GRIDS):
        assert int(((sizes >= lo) & (sizes <= hi)).sum()) > grid, (lo, hi, grid)


# ---------------------------------------------------------------------------------------------------- part D
def test_part_d_smallest_huge_segment(orc):
    for form in (1, 2, 4):
        case = sm.g2049_case(form)
        lcp, segs, (st, sz) = _designed(orc, case)
        assert sz == sm.HUGE + 1 and _huge(segs) == [(st, sz)]
        left = sm.rounds_left(lcp, [(st, sz)])
        assert (len(left) == 1) == (form == 1)                                      # form 1: finished in its first round


def test_part_d_copies(orc):
    case = sm.copies_case()
    lcp, sa, segs = _out(orc, case)
    huge = _huge(segs)
    assert case.n == 2049 * 301 and len(huge) == 300 - 15 and all(s == 2049 for _, s in huge) and len(segs) == len(huge)
    assert int(lcp.max()) == 300
    whole = sm.segment_of(segs, sm.read_rows(sa, case, 1))
    left = sm.rounds_left(lcp, [whole])                                             # the offset-0 segment: 284 bases in rounds of 16
    assert len(left) == 18 and left[:-1] == [(2049, 1)] * 17                        # tied to the terminator
    assert len(sm.rounds_left(lcp, huge)) == 18 and sm.rounds_left(lcp, huge)[0][1] == 285 - 16


def test_part_d_compaction(orc):
    case = sm.compaction_case()
    lcp, sa, segs = _out(orc, case)
    huge = _huge(segs)
    des = [sm.segment_of(segs, sm.read_rows(sa, case, t)) for t in (1, 2, 3)]
    assert sorted(huge) == sorted(des) and [s for _, s in des] == [4095, 4096, 4097]    # these three and no other
    assert sum(s for _, s in des) == 3 * sm.SCAN_TILE
    left = sm.rounds_left(lcp, huge)
    assert left == case.left
    assert [x[0] for x in left[:2]] == [sm.SCAN_TILE + 1, sm.SCAN_TILE]             # both sides of the scan's tile border
    x, y, z = ([sm.rounds_left(lcp, [s]) for s in des])
    assert x == [(0, 0)]                                                            # finishes in round 1
    assert y == [(3072, 1024), (3071, 1024), (0, 0)] and len(z) == 4                # four rounds
    rr = sm.runs(lcp, 2 * sm.KEY, *des[1])
    gaps = rr[1:, 0] - (rr[:-1, 0] + rr[:-1, 1])
    assert (rr[:, 1] == 3).all() and (gaps == 1).sum() > 1000                       # single slots between tied ones


def test_part_d_equal_keys_across_a_segment_border(orc):
    case = sm.border_case()
    lcp, sa, segs = _out(orc, case)
    (s1, z1), (s2, z2) = (sm.segment_of(segs, sm.read_rows(sa, case, t)) for t in (1, 2))
    assert z1 == z2 == 2049 and s1 + z1 == s2 and lcp[s2] == sm.KEY - 1             # adjacent, LCP below the key
    assert sm.rounds_left(lcp, [(s1, z1)])[0] == (2049, 1) and sm.rounds_left(lcp, [(s2, z2)])[0] == (2049, 1)
    huge = _huge(segs)
    pairs = sum(1 for (a, s), (b, t) in zip(huge, huge[1:]) if a + s == b)
    assert pairs >= 5                                                               # the same at some of the offsets 1 .. 14


@pytest.mark.parametrize("K", [sm.PASS_SWITCH, sm.PASS_SWITCH + 1])
def test_part_d_pass_switch(orc, K):
    case = sm.passes_case(K)
    lcp, segs, (st, sz) = _designed(orc, case)
    assert case.n == 2 * K * 34 and sz == 2 * K and int(lcp.max()) == 2 * sm.KEY
    tied = sm.runs(lcp, 2 * sm.KEY, 0, case.n)
    assert len(tied) == K and (tied[:, 1] == 2).all()
    assert tied[0, 0] >= st and tied[-1, 0] + 2 <= st + sz                          # all of them in the one segment
    bwt = orc.build_ebwt(*case.bqr)[0]
    first = bwt[tied[:, 0]]
    assert set(bwt[st:st + sz].tolist()) == {ord("A"), ord("C")} and 0.3 < (first == ord("A")).mean() < 0.7   # the order shows
    huge = _huge(segs)
    assert (st, sz) in huge and len(huge) < sm.PASS_SWITCH                          # nsub of round 1: the 2-pass side
    assert sm.rounds_left(lcp, huge) == [(2 * K, K), (0, 0)]                        # nsub of round 2 is exactly K


def test_part_d_cap_cases(orc):
    for case in (sm.cap_case(), sm.two_case()):
        lcp, sa, segs = _out(orc, case)
        des = [sm.segment_of(segs, sm.read_rows(sa, case, t)) for t in range(1, len(case.sizes) + 1)]
        assert tuple(s for _, s in des) == case.sizes and sorted(_huge(segs)) == sorted(des)
        assert any(s & (s - 1) for s in case.sizes)                                 # not a power of two: the virtual padding
        for st, sz in des[:2]:                                                      # forms 2 and 4: the network really sorts
            assert len(set(lcp[st + 1:st + sz].tolist())) >= 15
