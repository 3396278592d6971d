"""Interleaved paired FASTQ in plain Python: the definition of csrc/bfq_pairs.h over lists of lines, and the named cases the
host and GPU tests share.  Nothing here imports the library.

  split(text, ...)   -> ([text 0 (singletons), text 1, text 2], stats)      the model of bfq_fastq_deinterleave*
  merge(texts, ...)  -> (the interleaved text, stats)                       the model of bfq_fastq_interleave*
  Refused            what both raise: .code and .msg as the library words them

Cases (every one built once and shared):
  edges     empty text; one pair; reads of length 0; CRLF lines; no final LF; "+name" third lines; header comments behind a
            blank and behind a tab; x/1 + x/2, x/1 + x/1 (equal by the one-rule definition), "/1" alone (nothing removed), "@"
            alone; a key longer than 255 bytes
  lanes     record sizes 6 .. 70 bytes in sequence, up and down and shifted by one record, so that every destination alignment
            0..15 meets every head / body / tail length of the copy
  mismatch  refusals: a differing pair at k = 0, in the middle and last; two differing pairs (the lower one is named); odd N;
            counts 3 vs 2 for the merge
  orphans   runs of length 1, 2, 3, 4, 5; singles first, in the middle and last; a file of singles only; empty keys only
  long      one record of BFQ_MAX_READ_LEN bases between short ones
  wide      70 000 records of 20-40 bases, about 5 MB, seeded: crosses the grid stride of every kernel, the 4 KiB chunks of
            the line index, the chunks of the prefix sums and of the run-start scan, and 2^16 records.  Its orphan form holds
            one run of 5 001 equal keys, one of 4 000 and singles on both sides: run starts are carried over several scan
            chunks, and an odd long run ends in a single.
"""
import functools
import random

E_ARG, E_TOO_LONG, E_NOMEM = -1, -5, -7
MAX_READ_LEN = 65000
SCAN_CHUNK = 4096          # records per chunk of the run-start max-scan the "wide" case assumes (k_pairs.hip: PR_SCAN_CHUNK)


class Refused(Exception):
    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code, self.msg = code, msg


# ---------------------------------------------------------------- the rule
def lines_of(text):
    """the lines of a text, without their LF; a last line without its LF counts"""
    if not text:
        return []
    ls = bytes(text).split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    return ls


def records(text):
    """the records of a text: (header line, the record's bytes -- its four lines, each with its LF)"""
    ls = lines_of(text)
    if len(ls) % 4:
        raise Refused(E_ARG, "FASTQ: number of lines is not a multiple of 4")
    out, bad_len, too_long = [], False, False
    for i in range(0, len(ls), 4):
        seq, qual = ls[i + 1], ls[i + 3]
        if seq.endswith(b"\r"):
            seq = seq[:-1]
        if qual.endswith(b"\r"):
            qual = qual[:-1]
        bad_len = bad_len or len(seq) != len(qual)
        too_long = too_long or len(seq) > MAX_READ_LEN
        out.append((ls[i], b"".join(l + b"\n" for l in ls[i:i + 4])))
    if bad_len:
        raise Refused(E_ARG, "FASTQ: len(DNA) != len(QS) in a record")
    if too_long:
        raise Refused(E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN")
    return out


def key(header, mate_suffix=1):
    """the bytes behind '@' up to the first blank, tab, CR or line end; a trailing /1 or /2 removed where a byte remains"""
    k = header[1:]
    for j, ch in enumerate(k):
        if ch in b" \t\r":
            k = k[:j]
            break
    if mate_suffix and len(k) > 2 and k[-2:] in (b"/1", b"/2"):
        k = k[:-2]
    return k


def _gzip(text, what):
    if text is not None and len(text) >= 2 and text[0] == 0x1F and text[1] == 0x8B:
        raise Refused(E_ARG, what + " compressed (it begins with 1f 8b): inflate the text first")


def _opts(check_names=1, mate_suffix=1, orphans=0, reserved=0):
    if reserved:
        raise Refused(E_ARG, "bfq_pairs_opts.reserved: must be 0")
    return check_names, mate_suffix, orphans


def roles(keys, orphans):
    """the output (0, 1, 2) of every record; strict mode: by parity (the caller has checked the count and the names)"""
    if not orphans:
        return [1 + (i & 1) for i in range(len(keys))]
    out, i, n = [], 0, len(keys)
    while i < n:                                   # a maximal run of equal keys: [i, j)
        j = i + 1
        while j < n and keys[j] == keys[i]:
            j += 1
        r = j - i
        for d in range(r):
            out.append(2 if d & 1 else 0 if d == r - 1 else 1)
        i = j
    return out


def split(text, **opts):
    check_names, mate_suffix, orphans = _opts(**opts)
    _gzip(text, "interleaved FASTQ: the text is")
    recs = records(text)
    n = len(recs)
    keys = [key(h, mate_suffix) for h, _ in recs]
    if not orphans:
        if n & 1:
            raise Refused(E_ARG, "interleaved FASTQ: %d records, an odd number" % n)
        if check_names:
            for k in range(n // 2):
                if keys[2 * k] != keys[2 * k + 1]:
                    raise Refused(E_ARG, "interleaved FASTQ: pair %d (records %d and %d): the names differ" % (k, 2 * k, 2 * k + 1))
    role = roles(keys, orphans)
    outs = [b"".join(r for (_, r), w in zip(recs, role) if w == k) for k in range(3)]
    n_reads = [role.count(k) for k in range(3)]
    st = dict(records=n, pairs=n_reads[1], singles=n_reads[0], out_len=[len(o) for o in outs])
    assert n_reads[1] == n_reads[2]
    return outs, st


def merge(texts, **opts):
    check_names, mate_suffix, _ = _opts(**opts)
    texts = list(texts) + [None] * (3 - len(texts))
    for k in range(3):
        _gzip(texts[k], "FASTQ interleave: text %d is" % k)
    recs = [records(t) if t is not None else [] for t in texts]
    if len(recs[1]) != len(recs[2]):
        raise Refused(E_ARG, "FASTQ interleave: text 1 holds %d reads, text 2 holds %d" % (len(recs[1]), len(recs[2])))
    if check_names:
        for k, ((h1, _), (h2, _)) in enumerate(zip(recs[1], recs[2])):
            if key(h1, mate_suffix) != key(h2, mate_suffix):
                raise Refused(E_ARG, "FASTQ interleave: pair %d: the names differ" % k)
    out = b"".join(a + b for (_, a), (_, b) in zip(recs[1], recs[2])) + b"".join(r for _, r in recs[0])
    st = dict(records=2 * len(recs[1]) + len(recs[0]), pairs=len(recs[1]), singles=len(recs[0]), out_len=[len(out), 0, 0])
    return out, st


# ---------------------------------------------------------------- the cases
def rec(header, seq, qual=None, plus=b"+", eol=b"\n"):
    return header + eol + seq + eol + plus + eol + (qual if qual is not None else b"I" * len(seq)) + eol


def _edge_pairs():
    long_key = b"@" + b"k" * 300
    return [
        (b"@x/1", b"@x/2"), (b"@x/1", b"@x/1"), (b"@/1", b"@/1"), (b"@", b"@"), (b"@r1 1:N:0:ACGT", b"@r1\tBC:Z:AC GT"),
        (b"@r2 comment/1", b"@r2/2 other"), (long_key + b"/1", long_key + b"/2 c"), (b"@a/1/1", b"@a/1/2"), (b"@y/2", b"@y/1"),
    ]


@functools.lru_cache(maxsize=None)
def edges_text():
    t = b""
    for j, (h1, h2) in enumerate(_edge_pairs()):
        L = (0, 1, 7, 16, 33)[j % 5]
        t += rec(h1, b"ACGTN"[j % 5:j % 5 + 1] * L) + rec(h2, b"T" * L, plus=b"+" + h2[1:] if j & 1 else b"+")
    t += rec(b"@zero", b"") + rec(b"@zero", b"")
    t += rec(b"@crlf/1", b"ACGT", eol=b"\r\n") + rec(b"@crlf/2 c", b"GGCC", eol=b"\r\n")   # (last: a text cannot lose the LF of an empty line)
    return t


@functools.lru_cache(maxsize=None)
def lanes_text():
    """record sizes 6 .. 70: "@" [" " filler] LF seq LF + LF qual LF; every key is empty, so every couple is a pair"""
    sizes = list(range(6, 71)) + list(range(70, 5, -1)) + [9] + list(range(6, 71)) + list(range(70, 6, -1))
    assert len(sizes) % 2 == 0
    t = b""
    for s in sizes:
        L = (s - 6) // 2
        r = rec(b"@" + b" " * (s - 6 - 2 * L), b"ACGT"[s & 3:][:1] * L, b"#5AI"[s & 3:][:1] * L)
        assert len(r) == s
        t += r
    return t


def _runs(lengths, seed=5):
    """an orphan-mode text: run j has lengths[j] records named q<j> (a single: length 1)"""
    rng = random.Random(seed)
    t = b""
    for j, r in enumerate(lengths):
        for d in range(r):
            L = rng.randrange(0, 40)
            t += rec(b"@q%d%s" % (j, (b"", b"/1", b"/2", b" c")[(j + d) & 3]), bytes(rng.choice(b"ACGT") for _ in range(L)))
    return t


@functools.lru_cache(maxsize=None)
def long_text():
    big = b"ACGT" * (MAX_READ_LEN // 4)
    return (rec(b"@s/1", b"ACG") + rec(b"@s/2", b"TTT") + rec(b"@big/1", big, b"F" * MAX_READ_LEN) + rec(b"@big/2", b"AC") +
            rec(b"@e/1", b"A") + rec(b"@e/2", b"C"))


def _wide_rec(rng, header):
    L = rng.randrange(20, 41)
    return rec(header, bytes(rng.choice(b"ACGTN") for _ in range(L)), bytes(rng.randrange(35, 75) for _ in range(L)))


@functools.lru_cache(maxsize=None)
def wide_text():
    """70 000 records, 35 000 proper pairs"""
    rng = random.Random(20241020)
    parts = []
    for k in range(35000):
        c = (b"", b" 1:N:0", b"\tRX:Z:AC")[k % 3]
        parts.append(_wide_rec(rng, b"@w%d/1%s" % (k, c)))
        parts.append(_wide_rec(rng, b"@w%d/2%s" % (k, c)))
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def wide_orphans_text():
    """70 000 records: 4 000 singles, a run of 5 001 equal keys (records 4 000 .. 9 000: it lies in three chunks of the
    run-start scan and its start is carried over two boundaries), pairs, singles, a run of 4 000 (records 39 502 .. 43 501,
    over the boundary at 40 960), pairs, two singles"""
    rng = random.Random(20241021)
    plan = [1] * 4000 + [5001] + [2] * 15000 + [1] * 501 + [4000] + [2] * 13248 + [1, 1]
    assert sum(plan) == 70000 and 4000 // SCAN_CHUNK + 2 == 9000 // SCAN_CHUNK and 39502 // SCAN_CHUNK + 1 == 43501 // SCAN_CHUNK
    parts = []
    for j, r in enumerate(plan):
        for d in range(r):
            parts.append(_wide_rec(rng, b"@o%d%s" % (j, (b"/1", b"/2")[d & 1] if r > 1 else b"")))
    assert len(parts) == 70000
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def split_cases():
    """label -> (text, opts)"""
    e = edges_text()
    one = rec(b"@p/1", b"ACGT") + rec(b"@p/2", b"TTTT")
    c = {
        "edges": (e, {}), "edges-nolf": (e[:-1], {}), "edges-keep-suffix-unchecked": (e, dict(mate_suffix=0, check_names=0)),
        "edges-orphans": (e, dict(orphans=1)), "edges-orphans-keep-suffix": (e, dict(orphans=1, mate_suffix=0)),
        "empty": (b"", {}), "empty-orphans": (b"", dict(orphans=1)), "one-pair": (one, {}), "one-pair-nolf": (one[:-1], dict(orphans=1)),
        "lanes": (lanes_text(), {}), "lanes-orphans": (lanes_text()[6:], dict(orphans=1)),
        "unchecked": (rec(b"@a", b"AC") + rec(b"@b", b"GT"), dict(check_names=0)),
        "orphans-runs": (_runs([1, 2, 3, 4, 5]), dict(orphans=1)), "orphans-singles-first": (_runs([1, 1, 2, 2, 1, 2, 3]), dict(orphans=1)),
        "orphans-single-last": (_runs([2, 4, 1]), dict(orphans=1, mate_suffix=1)), "orphans-singles-only": (_runs([1] * 9), dict(orphans=1)),
        "orphans-empty-keys": (rec(b"@", b"ACG") * 5, dict(orphans=1)), "orphans-one": (rec(b"@only", b"A"), dict(orphans=1)),
        "long": (long_text(), {}), "long-orphans": (long_text(), dict(orphans=1)),
        "wide": (wide_text(), {}), "wide-orphans": (wide_orphans_text(), dict(orphans=1)),
    }
    return c


SMALL_SPLIT = tuple(k for k in ("edges", "edges-nolf", "edges-keep-suffix-unchecked", "edges-orphans", "edges-orphans-keep-suffix", "empty", "empty-orphans",
                                "one-pair", "one-pair-nolf", "lanes", "lanes-orphans", "unchecked", "orphans-runs", "orphans-singles-first",
                                "orphans-single-last", "orphans-singles-only", "orphans-empty-keys", "orphans-one", "long", "long-orphans"))
SPLIT_NAMES = SMALL_SPLIT + ("wide", "wide-orphans")


@functools.lru_cache(maxsize=None)
def expect_split(name):
    text, opts = split_cases()[name]
    return split(text, **opts)


@functools.lru_cache(maxsize=None)
def merge_cases():
    """label -> (texts, opts): the mates the model splits the split cases into, and a few of their own"""
    c = {}
    for name in ("edges", "edges-nolf", "empty", "one-pair", "lanes", "long", "wide"):
        (t0, t1, t2), _ = expect_split(name)
        c[name] = ((None, t1, t2), {})
    (s0, s1, s2), _ = expect_split("orphans-singles-first")
    c["with-singles"] = ((s0, s1, s2), {})
    c["with-singles-nolf"] = ((s0[:-1], s1[:-1], s2[:-1]), {})
    c["singles-only"] = ((s0, None, None), {})
    c["lanes-with-singles"] = ((lanes_text()[6:6 + 7 + 8 + 9], expect_split("lanes")[0][1], expect_split("lanes")[0][2]), {})
    c["unchecked"] = ((None, rec(b"@a", b"AC"), rec(b"@b", b"GT")), dict(check_names=0))
    c["keep-suffix-unchecked"] = ((None, rec(b"@a/1", b"AC"), rec(b"@a/2", b"GT")), dict(check_names=0, mate_suffix=0))
    return c


MERGE_NAMES = ("edges", "edges-nolf", "empty", "one-pair", "lanes", "long", "wide", "with-singles", "with-singles-nolf", "singles-only", "lanes-with-singles",
               "unchecked", "keep-suffix-unchecked")


@functools.lru_cache(maxsize=None)
def expect_merge(name):
    texts, opts = merge_cases()[name]
    return merge(texts, **opts)


def _pairs_text(n, bad=()):
    return b"".join(rec(b"@m%d/1" % k, b"ACGT") + rec(b"@%s%d/2" % (b"X" if k in bad else b"m", k), b"GGTT") for k in range(n))


@functools.lru_cache(maxsize=None)
def split_refusals():
    """label -> (text, opts, code, message)"""
    good = _pairs_text(9)
    long_key = b"@" + b"k" * 299
    r = {
        "first": (_pairs_text(9, (0,)), {}, E_ARG, "interleaved FASTQ: pair 0 (records 0 and 1): the names differ"),
        "middle": (_pairs_text(9, (4,)), {}, E_ARG, "interleaved FASTQ: pair 4 (records 8 and 9): the names differ"),
        "last": (_pairs_text(9, (8,)), {}, E_ARG, "interleaved FASTQ: pair 8 (records 16 and 17): the names differ"),
        "two": (_pairs_text(300, (288, 17)), {}, E_ARG, "interleaved FASTQ: pair 17 (records 34 and 35): the names differ"),
        "suffix-kept": (good, dict(mate_suffix=0), E_ARG, "interleaved FASTQ: pair 0 (records 0 and 1): the names differ"),
        "bare-suffixes": (rec(b"@/1", b"A") + rec(b"@/2", b"C"), {}, E_ARG, "interleaved FASTQ: pair 0 (records 0 and 1): the names differ"),
        "long-key": (rec(long_key + b"a", b"A") + rec(long_key + b"b", b"C"), {}, E_ARG, "interleaved FASTQ: pair 0 (records 0 and 1): the names differ"),
        "prefix-key": (rec(b"@ab", b"A") + rec(b"@abc", b"C"), {}, E_ARG, "interleaved FASTQ: pair 0 (records 0 and 1): the names differ"),
        "odd": (good + rec(b"@z", b"A"), {}, E_ARG, "interleaved FASTQ: 19 records, an odd number"),
        "odd-unchecked": (rec(b"@z", b"A"), dict(check_names=0), E_ARG, "interleaved FASTQ: 1 records, an odd number"),
        "wide-late": (wide_text() + rec(b"@t/1", b"A") + rec(b"@u/2", b"C"), {}, E_ARG,
                      "interleaved FASTQ: pair 35000 (records 70000 and 70001): the names differ"),
        "lines": (good + b"@x\nA\n", {}, E_ARG, "FASTQ: number of lines is not a multiple of 4"),
        "lengths": (good + rec(b"@x", b"ACG", b"II") * 2, dict(orphans=1), E_ARG, "FASTQ: len(DNA) != len(QS) in a record"),
        "too-long": (rec(b"@x", b"A" * (MAX_READ_LEN + 1)) * 2, {}, E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN"),
        "gzip": (b"\x1f\x8b\x08\x04" + good, {}, E_ARG, "interleaved FASTQ: the text is compressed (it begins with 1f 8b): inflate the text first"),
        "reserved": (good, dict(reserved=7), E_ARG, "bfq_pairs_opts.reserved: must be 0"),
    }
    for name, (text, opts, code, msg) in r.items():                # the model agrees with the table
        try:
            split(text, **opts)
            raise AssertionError(name)
        except Refused as e:
            assert (e.code, e.msg) == (code, msg), (name, e.msg)
    return r


@functools.lru_cache(maxsize=None)
def merge_refusals():
    """label -> (texts, opts, code, message)"""
    m = lambda n, w, bad=(): b"".join(rec(b"@%s%d/%d" % (b"X" if k in bad else b"m", k, w), b"ACGT") for k in range(n))
    r = {
        "counts": ((None, m(3, 1), m(2, 2)), {}, E_ARG, "FASTQ interleave: text 1 holds 3 reads, text 2 holds 2"),
        "absent-mate": ((None, None, m(2, 2)), {}, E_ARG, "FASTQ interleave: text 1 holds 0 reads, text 2 holds 2"),
        "first": ((None, m(9, 1, (0,)), m(9, 2)), {}, E_ARG, "FASTQ interleave: pair 0: the names differ"),
        "middle": ((m(2, 1), m(9, 1), m(9, 2, (5,))), {}, E_ARG, "FASTQ interleave: pair 5: the names differ"),
        "last": ((None, m(9, 1, (8,)), m(9, 2)), {}, E_ARG, "FASTQ interleave: pair 8: the names differ"),
        "two": ((None, m(300, 1, (299, 41)), m(300, 2)), {}, E_ARG, "FASTQ interleave: pair 41: the names differ"),
        "suffix-kept": ((None, m(3, 1), m(3, 2)), dict(mate_suffix=0), E_ARG, "FASTQ interleave: pair 0: the names differ"),
        "lines": ((None, m(3, 1), m(3, 2) + b"@x\n"), {}, E_ARG, "FASTQ: number of lines is not a multiple of 4"),
        "lengths-in-singles": ((rec(b"@x", b"ACG", b"I"), m(3, 1), m(3, 2)), {}, E_ARG, "FASTQ: len(DNA) != len(QS) in a record"),
        "gzip": ((None, m(3, 1), b"\x1f\x8b" + m(3, 2)), {}, E_ARG, "FASTQ interleave: text 2 is compressed (it begins with 1f 8b): inflate the text first"),
        "reserved": ((None, m(3, 1), m(3, 2)), dict(reserved=1), E_ARG, "bfq_pairs_opts.reserved: must be 0"),
    }
    for name, (texts, opts, code, msg) in r.items():
        try:
            merge(texts, **opts)
            raise AssertionError(name)
        except Refused as e:
            assert (e.code, e.msg) == (code, msg), (name, e.msg)
    return r


def wide_counts():
    """what the model alone yields for the orphan form of "wide", by counting: (singles, pairs, the longest run)"""
    recs = records(wide_orphans_text())
    keys = [key(h) for h, _ in recs]
    longest, i = 0, 0
    while i < len(keys):
        j = i + 1
        while j < len(keys) and keys[j] == keys[i]:
            j += 1
        longest = max(longest, j - i)
        i = j
    role = roles(keys, 1)
    return role.count(0), role.count(1), longest
