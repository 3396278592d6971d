"""k_refine_chunk fetches a round's three text words by two loads issued side by side; before, the third word's load stood
behind the wait for the first two.  BFQ_REFINE_PIPE=0 launches the earlier kernel (k_refine_chunk_seq) from the same build,
and bfq_refine_form() tells which one a context runs.  Every case builds the eBWT on the same input both ways and requires
equal BWT, QS and LCP; the cases of a few thousand rows are compared with the CPU oracle as well.

The switch and the shapes come from the experiment this change was found in: running the batches of a chunk as a software
pipeline (profiles/r7_refine_pipe; measured, not kept).  The shapes sit on the edges of the chunk kernel's batch loops, in
collections of at most a few chunks of 2048 rows.  What a shape is meant to hold (segments, their sizes, where they lie) is
computed here from the sorted 16-symbol keys and asserted, and the number of segments is compared with the n_segments the
device counted:
  * a chunk with no batch at all, then exactly 1, 2 and 3 batches;
  * batches that come out empty: a segment of exactly 64 rows, one of 63 followed by one of 2 (and the other way round), a
    segment of 65 rows (listed for k_refine_big: nothing is left for the batch), a chunk's group of segments nearly all above
    64 rows with small ones among them.  (64 such segments in ONE group cannot be: a group's segments start in one chunk,
    and 64 x 65 rows do not fit into 2048.  31 do, and that is what the case holds.);
  * more than 64 segments in a chunk: pairs of identical reads, several groups of 64 segments;
  * many rounds: 20 copies of a 300-base read with 1 % substitutions and 20 exact copies (tied up to the terminator, resolved
    by position): 7 rounds of text words;
  * chunk borders: 2047, 2048, 2049 and 4097 rows, a segment with its head in the last rows of chunk 0 and the rest in chunk 1,
    a segment that runs past the 128-row look-ahead (listed without its length);
  * keys holding terminators: reads shorter than the key, empty reads, N's.

A wavefront's SECOND chunk (the grid-stride loop) is not reached here: the grid covers 4.3 G rows before a wavefront takes
another chunk, so no test of this size can reach it.  The output comparison of the benchmark's 30 M x 150 workload against the
parent commit (profiles/r7_refine_pipe/README.md) covers it: 2.21 M chunks on 2.10 M wavefront slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 2048                                                          # rows per wavefront chunk (k_refine.hip)
KEY = 16                                                              # symbols of the sorted key


def _switch(engine, monkeypatch, value):
    if value is None:
        monkeypatch.delenv("BFQ_REFINE_PIPE", raising=False)
    else:
        monkeypatch.setenv("BFQ_REFINE_PIPE", value)
    engine.set_params()                                               # (the environment is read here)


def _both(engine, monkeypatch, b, q, r, orc=None):
    """eBWT by the default against BFQ_REFINE_PIPE=0, then (orc given) against the oracle; returns n_segments of a whole run."""
    r = np.asarray(r, np.uint64)
    b = np.ascontiguousarray(b, np.uint8); q = np.ascontiguousarray(q, np.uint8)
    try:
        _switch(engine, monkeypatch, None)
        nb, nq, nl = engine.build_ebwt(b, q, r)
        nseg = engine.run_reads(b, q, r)[2]["n_segments"]
        _switch(engine, monkeypatch, "0")
        wb, wq, wl = engine.build_ebwt(b, q, r)
        assert np.array_equal(nb, wb), "bwt"
        assert np.array_equal(nq, wq), "qs"
        assert np.array_equal(nl, wl), "lcp"
        assert engine.run_reads(b, q, r)[2]["n_segments"] == nseg
    finally:
        _switch(engine, monkeypatch, None)
    assert len(nb) == int(r[-1]) + len(r) - 1
    if orc is not None:
        eb, eq, el = orc.build_ebwt(b, q, r)
        assert np.array_equal(nb, eb) and np.array_equal(nq, eq) and np.array_equal(nl.astype(np.uint32), el), "oracle"
    return nseg


def _segments(b, r):
    """(first row, rows) of every segment the refinement meets: runs of >= 2 equal 16-symbol keys without a terminator, in
    suffix order (#_i < #_j < A < C < G < N < T: a terminator sorts below every base, terminators among themselves by read)."""
    b = bytes(np.asarray(b, np.uint8)); r = [int(x) for x in r]
    keys = []
    for i in range(len(r) - 1):
        s = b[r[i]:r[i + 1]]
        for o in range(len(s) + 1):
            k = s[o:o + KEY]
            keys.append((k + b"\x00", i) if len(k) < KEY else (k, -1))
    keys.sort()
    out, i = [], 0
    while i < len(keys):
        j = i + 1
        if keys[i][1] < 0:
            while j < len(keys) and keys[j] == keys[i]:
                j += 1
            if j - i >= 2:
                out.append((i, j - i))
        i = j
    return out


def _pack(reads, rng):
    b = np.concatenate([np.frombuffer(x, np.uint8) for x in reads]) if reads else np.zeros(0, np.uint8)
    q = rng.integers(35, 75, len(b)).astype(np.uint8)
    r = np.zeros(len(reads) + 1, np.uint64); r[1:] = np.cumsum([len(x) for x in reads])
    return b, q, r


def _rand(rng, L, alphabet=b"ACGT"):
    return bytes(np.array(list(alphabet), np.uint8)[rng.integers(0, len(alphabet), L)])


def _reads(rng, lens, alphabet=b"ACGT", err=0.02):
    """Reads of the given lengths drawn from a short genome (long common prefixes, equal keys), with a few substitutions."""
    genome = np.array(list(alphabet), np.uint8)[rng.integers(0, len(alphabet), 700)]
    out = []
    for L in [int(x) for x in lens]:
        st = int(rng.integers(0, 700))
        s = np.tile(genome, L // 700 + 2)[st:st + L].copy()
        hit = rng.random(L) < err
        s[hit] = np.array(list(b"ACGTN"), np.uint8)[rng.integers(0, 5, int(hit.sum()))]
        out.append(bytes(s))
    return _pack(out, rng)


def _lens_for_rows(rows, L=100):
    """Read lengths (L, the last one shorter) whose bases + reads make exactly `rows` rows."""
    k = rows // (L + 1)
    rest = rows - k * (L + 1)
    lens = [L] * k
    if rest:
        lens.append(rest - 1)                                         # (rest = 1: an empty read)
    assert sum(lens) + len(lens) == rows
    return lens


def test_the_default_is_the_new_kernel(engine, monkeypatch):
    try:
        _switch(engine, monkeypatch, None)
        assert engine.refine_form() == 1
        _switch(engine, monkeypatch, "0")
        assert engine.refine_form() == 0
        _switch(engine, monkeypatch, "1")
        assert engine.refine_form() == 1
    finally:
        _switch(engine, monkeypatch, None)
    assert engine.refine_form() == 1


def test_no_batch_at_all(engine, orc, monkeypatch):
    rng = np.random.default_rng(700)
    b, q, r = _pack([_rand(rng, 40) for _ in range(30)], rng)         # 1230 rows, every key on its own
    assert _segments(b, r) == []
    assert _both(engine, monkeypatch, b, q, r, orc) == 0


@pytest.mark.parametrize("batches", [1, 2, 3])
def test_fill_and_drain(engine, orc, monkeypatch, batches):
    """4 copies of one random read of L bases: offset o gives one segment of 4 rows while L - o >= 16, 16 segments to a batch."""
    rng = np.random.default_rng(710 + batches)
    c, L = 4, 15 + 16 * batches
    b, q, r = _pack([_rand(rng, L)] * c, rng)
    segs = _segments(b, r)
    assert len(segs) == L - 15 and all(sz == c for _, sz in segs)
    assert 64 * (batches - 1) < c * (L - 15) <= 64 * batches and c * (L + 1) <= CHUNK
    assert _both(engine, monkeypatch, b, q, r, orc) == len(segs)


@pytest.mark.parametrize("sizes", [(64,), (63, 2), (2, 63), (65,), (65, 2, 64, 3)])
def test_batches_on_the_64_row_edge(engine, orc, monkeypatch, sizes):
    """Segments of exactly these sizes in this order: c copies of a 16-base read make one segment of c rows."""
    rng = np.random.default_rng(720 + 7 * len(sizes) + sizes[0])
    heads = b"ACGT"                                                   # the first base fixes the order of the segments
    reads = []
    for k, c in enumerate(sizes):
        reads += [heads[k:k + 1] + _rand(rng, 15)] * c
    b, q, r = _pack(reads, rng)
    assert [sz for _, sz in _segments(b, r)] == list(sizes)
    assert _both(engine, monkeypatch, b, q, r, orc) == len(sizes)


def test_a_group_of_large_segments_with_small_ones(engine, orc, monkeypatch):
    """65 copies of a 46-base read: 31 segments of 65 rows (about as many as can start in one chunk), all left to k_refine_big;
    pairs of other reads put segments of 2 rows among and after them."""
    rng = np.random.default_rng(730)
    reads = [_rand(rng, 46)] * 65
    for _ in range(6):
        reads += [_rand(rng, 20)] * 2
    b, q, r = _pack(reads, rng)
    sizes = [sz for _, sz in _segments(b, r)]
    assert sizes.count(65) == 31 and sizes.count(2) == 6 * 5 and len(sizes) == 31 + 30
    assert _both(engine, monkeypatch, b, q, r, orc) == len(sizes)


def test_more_than_64_segments_in_a_chunk(engine, orc, monkeypatch):
    rng = np.random.default_rng(740)
    reads = []
    for _ in range(40):
        reads += [_rand(rng, 30)] * 2                                 # 15 segments of 2 rows each
    b, q, r = _pack(reads, rng)
    segs = _segments(b, r)
    assert len(segs) == 600 and len(b) + len(r) - 1 == 2480
    per_chunk = np.bincount([st // CHUNK for st, _ in segs])
    assert per_chunk.max() > 4 * 64                                   # several groups of 64 segments in one chunk
    assert _both(engine, monkeypatch, b, q, r, orc) == len(segs)


def test_many_rounds(engine, orc, monkeypatch):
    rng = np.random.default_rng(750)
    base = np.frombuffer(_rand(rng, 300), np.uint8)
    reads = []
    for _ in range(20):
        s = base.copy()
        hit = rng.random(300) < 0.01
        s[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        reads.append(bytes(s))
    reads += [bytes(base)] * 20                                       # tied up to the terminator: (300 - 16) / 42 -> 7 rounds
    b, q, r = _pack(reads, rng)
    assert max(sz for _, sz in _segments(b, r)) >= 20
    _both(engine, monkeypatch, b, q, r, orc)


@pytest.mark.parametrize("rows", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_border_sizes(engine, orc, monkeypatch, rows):
    rng = np.random.default_rng(760 + rows)
    b, q, r = _reads(rng, _lens_for_rows(rows))
    assert len(b) + len(r) - 1 == rows
    _both(engine, monkeypatch, b, q, r, orc)


@pytest.mark.parametrize("copies,before_border", [(20, 10), (300, 50)])
def test_segment_across_the_chunk_border(engine, orc, monkeypatch, copies, before_border):
    """`copies` reads of 16 T's: the largest key there is, so their segment is the last rows of the collection (their 16 shorter
    suffixes each hold terminators and sort before it).  Filler reads put its head `before_border` rows before the end of a
    chunk; 300 copies run past the 128-row look-ahead as well."""
    rng = np.random.default_rng(770 + copies)
    j = (16 * copies + before_border + 101) // CHUNK + 1              # the chunk the head lies in, + 1
    fb, fq, fr = _reads(rng, _lens_for_rows(j * CHUNK - before_border - 16 * copies), err=0.0)
    reads = [bytes(fb[int(fr[i]):int(fr[i + 1])]) for i in range(len(fr) - 1)] + [b"T" * 16] * copies
    b, q, r = _pack(reads, rng)
    st, sz = _segments(b, r)[-1]
    assert sz == copies and st + sz == len(b) + len(r) - 1
    assert st == j * CHUNK - before_border and st + sz > j * CHUNK
    if copies > 128 + before_border:
        assert st + sz > j * CHUNK + 128                              # beyond the look-ahead
    _both(engine, monkeypatch, b, q, r, orc)


def test_reads_shorter_than_the_key(engine, orc, monkeypatch):
    rng = np.random.default_rng(781)
    lens = np.array([0, 1, 2, 15])[rng.integers(0, 4, 1500)]
    lens[:6] = [0, 0, 15, 0, 1, 0]                                    # terminators side by side, at the very start as well
    b, q, r = _reads(rng, lens)
    _both(engine, monkeypatch, b, q, r, orc)


def test_reads_with_ns(engine, orc, monkeypatch):
    rng = np.random.default_rng(782)
    b, q, r = _reads(rng, [100] * 80, alphabet=b"ACGTNN", err=0.1)
    assert (b == ord("N")).sum() > 1000
    _both(engine, monkeypatch, b, q, r, orc)
