"""The suffix sorts behind the 16-symbol key (k_refine.hip: k_refine_big / block_sort, k_refine_listed / big_sort;
k_bigseg.hip: huge_batch, bfq_refine_huge) with segments placed on their size-class, padding, chunk, look-ahead, grid, tile,
round and pass borders by construction.  Every assertion is engine.build_ebwt == the CPU oracle for BWT, QS and LCP, bit for
bit (the cases called full go through tests.test_gpu_parity._check_against_oracle: reads, qualities and all statistics as
well).  Never one GPU path against another.  The collections come from tests/segment_model.py; tests/test_segment_host.py
asserts without a GPU, from the oracle's LCP, that every geometry named here is really in them.  The launch counts some
tests read (engine.prof) only confirm the route a case was built for; what is compared is the oracle.

Every designed read starts with a lead base of its own in front of the common head, so the designed suffixes are not whole
reads: the rows of whole reads all show the terminator and '#', and no output depends on the order of equal ones.  Behind
the lead base a wrong order among equal suffixes shows in BWT and QS.

  A  one designed segment of g rows (g reads with a common 16-base head) for g on both sides of every class and padding
     border of k_refine_big (65, 127 | 128 | 129, 255 | 256 | 257, 511 | 512 | 513, 1023 | 1024 | 1025, 2047 | 2048), with
     no tail (tied to the terminator: the read index decides), tails of 0 .. 100 bases that share starts of every length,
     D common bases then random ones (the deciding symbol in the first word, on the word border, in the second word, on
     the round border, in rounds 2 and 3), and tails from a small set (sub-segments of 1, 2 and > 64 rows side by side
     after round 0, exact copies among near copies).  One g per class is full.
  B  a T x 16 segment (the collection's last rows) or a G x 16 one (with rows behind it) with its head d rows before a chunk
     border: the next head on the last rows the look-ahead has a head bit for and on the first it has none for, the head on a
     chunk's last row and on its row 0, the end on a chunk border, a whole chunk without a head, more than 64 chunks, and
     the end of the collection with n = 0, 1 and 2047 modulo the chunk.
  C  more segments in every class than its launch has workgroups: the grid-stride loops' second trip.
  D  the radix rounds: the smallest huge segment, 285 of them in one batch over 18 rounds, three that leave 4097 and 4096
     slots (the scan's tile border) and single slots between tied ones, equal keys on both sides of a segment border,
     65536 and 65537 tied sub-segments in a round (2 and 4 passes of its second sort), BFQ_HUGE_CAP at g, g - 1 (the
     global-memory network with its virtual padding, on tails that need sorting), g1 + g2 and g1 + g2 - 1.
  The same pile by pile (piles=1, then BFQ_PILES_SPLIT=1 as well) and on engines whose workspace holds 0x41 / 0xFF.

Not reached, and why:
  * more than 65536 huge segments in ONE batch (the other way to nsub > 65536): 65537 segments of 2049 rows are 134 M
    rows, far beyond a test.  Round 2's nsub = 65537 takes the same branch.
  * the 1 << 30 segments-per-batch and 1 << 31 slots-per-batch limits of bfq_refine_huge: billions of rows.
  * the side buffer of bfq_refine_huge: tests/test_gpu_parity.py::test_huge_segment_side_buffer holds it (BFQ_HUGE_CAP
    switches it off, and without the cap it needs a segment the arena has no room for).
  * the depth limit beyond BFQ_MAX_READ_LEN (65000 bases): a read that long in >= 2049 copies is 133 M rows.
  * a wavefront's second chunk in k_refine_chunk (tests/test_gpu_refine_pipe.py says why)."""
import numpy as np
import pytest
from bfqzip_amd import api
from tests import segment_model as sm
from tests.test_gpu_parity import _check_against_oracle
from tests.test_gpu_poison import poisoned

pytestmark = pytest.mark.gpu
_WANT = {}


def _want(orc, case):
    """The oracle's (BWT, QS, LCP) of a case, computed once for the cases that several tests share."""
    if case.name not in _WANT:
        out = orc.build_ebwt(*case.bqr)
        if case.n > 5_000_000:
            return out
        _WANT[case.name] = out
    return _WANT[case.name]


def _ebwt(e, orc, case, *what):
    eb, eq, el = _want(orc, case)
    gb, gq, gl = e.build_ebwt(*case.bqr)
    assert len(gb) == case.n
    assert np.array_equal(gb, eb), ("bwt", case.name) + what
    assert np.array_equal(gq, eq), ("qs", case.name) + what
    assert np.array_equal(gl.astype(np.uint32), el), ("lcp", case.name) + what
    return el


def _full(e, orc, case, **par):
    try:
        return _check_against_oracle(e, orc, *case.bqr, **par)
    finally:
        e.set_params()


def _launches(e, name):
    return e.prof().get(name, {"launches": 0})["launches"]


# ---------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("g", sm.G_ALL)
def test_class_no_tail(engine, orc, g):
    """g identical 16-base reads: block_sort's round 0 sees g equal words holding the terminator and leaves the slot order."""
    _ebwt(engine, orc, sm.class_case(g, 1))


@pytest.mark.parametrize("g", sm.G_ALL)
def test_class_random_tails(engine, orc, g):
    case = sm.class_case(g, 2)
    _ebwt(engine, orc, case)
    if g in sm.G_FULL:
        assert _full(engine, orc, case)["n_big_segments"] >= 1


@pytest.mark.parametrize("g", sm.G_BORDER)
def test_class_deciding_symbol(engine, orc, g):
    """The LCP formula of block_sort by the word that decides: D common bases behind the key, D around 21, 42 and 84."""
    for D in sm.DS:
        _ebwt(engine, orc, sm.class_case(g, 3, D))


@pytest.mark.parametrize("g", sm.G_BORDER)
def test_class_small_tail_set(engine, orc, g):
    """Rows that are alone after round 0 beside sub-segments of 2 and > 64 rows: word 0, dense ids, ties behind a terminator."""
    _ebwt(engine, orc, sm.class_case(g, 4))


# ---------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("name", [x[0] for x in sm.PART_B])
def test_segment_position(engine, orc, name):
    """The end search of k_refine_big's first launch (tests/test_segment_host.py::test_part_b_positions has the positions)."""
    _ebwt(engine, orc, sm.part_b(name))


def test_more_than_64_chunks(engine, orc):
    """One segment of 140 000 rows (2.57 M rows in all): the search by firstHead[] takes a second step of 64 chunks."""
    _ebwt(engine, orc, sm.part_b(sm.LONG[0]))


# ---------------------------------------------------------------------------------------------------- part C
def test_more_segments_than_workgroups(engine, orc):
    """10 M rows with more segments in each class than its launch has workgroups (8192, 8192, 4096, 2048, 1024): every
    launch's workgroups sort a second segment in the same LDS.  The one slow case (the oracle takes seconds)."""
    _ebwt(engine, orc, sm.grids_case())


# ---------------------------------------------------------------------------------------------------- part D
@pytest.mark.parametrize("form", [1, 2, 4])
def test_smallest_huge_segment(engine, orc, form):
    engine.prof_reset()
    _ebwt(engine, orc, sm.g2049_case(form))
    assert _launches(engine, "k_huge_round") >= 6 and _launches(engine, "k_refine_big") == 5


def test_copies_in_one_batch(engine, orc):
    """2049 copies of a 300-base read: 285 huge segments, 18 rounds, the slot order decides everything.  Full."""
    case = sm.copies_case()
    engine.prof_reset()
    _ebwt(engine, orc, case)
    assert _launches(engine, "k_huge_round") == 1 + 5 * 18                # one batch: k_huge_expand once, five kernels a round
    _full(engine, orc, case)


def test_compaction(engine, orc):
    """12288 -> 4097 -> 4096 -> 1024 -> 0 slots: k_huge_compact's dense ids, bfq_exscan_u8 on both sides of a tile."""
    case = sm.compaction_case()
    engine.prof_reset()
    _ebwt(engine, orc, case)
    assert _launches(engine, "k_huge_round") == 1 + 5 * len(case.left)


def test_equal_keys_across_a_segment_border(engine, orc):
    _ebwt(engine, orc, sm.border_case())


@pytest.mark.parametrize("K", [sm.PASS_SWITCH, sm.PASS_SWITCH + 1])
def test_pass_switch(engine, orc, K):
    """Round 2 of the batch runs with nsub = K: 2 radix passes for 65536, 4 for 65537.  Every tied pair is an A row and a C
    row, so a pair that the second sort puts into another pair's slots shows in the BWT."""
    _ebwt(engine, orc, sm.passes_case(K))


def _capped(e, orc, monkeypatch, case, cap, listed, huge_launches=None):
    """One build under BFQ_HUGE_CAP=cap; `listed`: k_refine_listed ran (a sixth k_refine_big launch)."""
    try:
        monkeypatch.setenv("BFQ_HUGE_CAP", str(cap))
        e.set_params()                                                    # (the environment is read here)
        e.prof_reset()
        lcp = _ebwt(e, orc, case, "cap", cap)
        assert _launches(e, "k_refine_big") == 5 + (1 if listed else 0), (case.name, cap)
        if huge_launches is not None:
            assert _launches(e, "k_huge_round") == huge_launches, (case.name, cap)
        return lcp
    finally:
        monkeypatch.delenv("BFQ_HUGE_CAP", raising=False)
        e.set_params()


@pytest.mark.parametrize("form", [1, 2, 4])
def test_huge_cap_one_segment(engine, orc, monkeypatch, form):
    case = sm.g2049_case(form)
    _capped(engine, orc, monkeypatch, case, 2049, listed=False)
    _capped(engine, orc, monkeypatch, case, 2048, listed=True, huge_launches=0)


def test_huge_cap_three_segments(engine, orc, monkeypatch):
    """3000 (random tails), 4096 (tails from a small set) and 4097 rows (tied to the terminator)."""
    case = sm.cap_case()
    _capped(engine, orc, monkeypatch, case, 4097, listed=False)
    _capped(engine, orc, monkeypatch, case, 4096, listed=True)
    _capped(engine, orc, monkeypatch, case, 3000, listed=True)
    _capped(engine, orc, monkeypatch, case, 2999, listed=True, huge_launches=0)


def test_huge_cap_two_batches(engine, orc, monkeypatch):
    """cap = g1 + g2: one batch, whichever segment was listed first; one slot less: two."""
    case = sm.two_case()
    g1, g2 = case.sizes
    lcp = _want(orc, case)[2]
    segs = [(int(a), int(s)) for a, s in sm.segments(lcp) if s > sm.HUGE]
    assert sorted(s for _, s in segs) == [g1, g2]
    together = len(sm.rounds_left(lcp, segs))
    apart = sum(len(sm.rounds_left(lcp, [s])) for s in segs)
    _capped(engine, orc, monkeypatch, case, g1 + g2, listed=False, huge_launches=1 + 5 * together)
    _capped(engine, orc, monkeypatch, case, g1 + g2 - 1, listed=False, huge_launches=2 + 5 * apart)


# ---------------------------------------------------------------------------------------------------- other paths
def _pile_cases():
    for g in sm.G_BORDER:
        yield sm.class_case(g, 2)
    for name in sm.PART_B_PILES:
        yield sm.part_b(name)
    yield sm.g2049_case(1)
    yield sm.copies_case()
    yield sm.compaction_case()


@pytest.mark.parametrize("split", [False, True], ids=["piles", "piles_split"])
def test_pile_by_pile(engine, orc, monkeypatch, split):
    """bfq_refine once per first-symbol pile (and per second symbol with BFQ_PILES_SPLIT): other n, other chunk borders."""
    try:
        if split:
            monkeypatch.setenv("BFQ_PILES_SPLIT", "1")
        for case in _pile_cases():
            _full(engine, orc, case, piles=1)
    finally:
        monkeypatch.delenv("BFQ_PILES_SPLIT", raising=False)
        engine.set_params()


@pytest.mark.parametrize("byte", [0x41, 0xFF], ids=["0x41", "0xFF"])
def test_poisoned_workspace(orc, monkeypatch, byte):
    """The rounds' buffers, the m + 16 record pads, biglen[] and firstHead[] come out of the arena as the last call left
    them: here with every byte of it set before each call."""
    with poisoned(byte):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 16)
            assert e.workspace_bytes() > 0 and (e.workspace_read(0, 1 << 16) == byte).all()     # the switch is on for this engine
            for g in (127, 255, 511, 1023, 2047):
                _ebwt(e, orc, sm.class_case(g, 2), "poison", byte)
            _ebwt(e, orc, sm.part_b("end_129"), "poison", byte)
            _ebwt(e, orc, sm.copies_case(), "poison", byte)
            _ebwt(e, orc, sm.passes_case(sm.PASS_SWITCH + 1), "poison", byte)
            try:
                monkeypatch.setenv("BFQ_HUGE_CAP", "2999")
                e.set_params()
                _ebwt(e, orc, sm.cap_case(), "poison", byte, "cap", 2999)
            finally:
                monkeypatch.delenv("BFQ_HUGE_CAP", raising=False)
                e.set_params()
        finally:
            e.close()
