"""Exact duplicate removal in plain Python: the definition of bfq_fastq_dedup* (csrc/bfq_dedup.h) as a dictionary keyed by
sequence, the stated hash, and the named cases the host and GPU tests share.  Nothing here imports the library.

  dedup(texts, ...) -> ([kept 0, kept 1], [removed 0, removed 1], stats)      the model of bfq_fastq_dedup*
  unit_hash(keys, seed)                                                        the hash of csrc/bfq_dedup.h

The outputs are computed from the definition alone -- groups of equal keys, the kept unit by `keep` --; the hash enters only
the statistics mixed_runs, max_run and rounds and the refusal of a run with more than KINDS_MAX different keys.

Cases (every one built once and shared; texts = (text 0, text 1), text 1 None: single-end):
  sizes     no text, 0 records, 1 record, 2 equal, 2 different -- single-end and paired
  lengths   sequence lengths 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, each as an equal couple, a couple that
            differs in the last byte only and one that differs in the first byte only (the hash chunks of 8, the 16-byte
            steps and the 8-lane shares of the comparison); the same with the couples in mate 2 and in mate 1 of pairs
  collide   different sequences with EQUAL full hashes, built from the hash's own structure: of one length, differing in the
            first 16-byte step only, in the last chunks and the byte tail only, and in two steps of one lane's loop, at 16 / 17,
            64 / 65 and 256 / 257 bytes; a sequence and a proper prefix of it; single-end, in mate 1 and in mate 2.  Only the
            comparison of lengths and bytes keeps them apart: rounds >= 2 at hash_bits 40
  keys      a proper prefix of another sequence (at 8, 9, 16, 17 and 33 bytes), lower against upper case, N reads
  lines     CR LF against LF records of one sequence (equal, each leaves byte for byte); different headers, '+' lines and
            qualities (still duplicates); no final LF
  pairs     equal mate 1 and different mate 2; ("AC","G") against ("A","CG"); swapped mates; a duplicated pair among singles
  groups    sizes 1, 2, 3, 64, 65, 256, 257, 1024, 1025 and 4097 in one text, the members scattered: no bound at 1024
  wide      70 000 units of 36 bases, about 6 MB: one sequence 40 000 times, forty groups of 3..300, the rest unique; crosses
            2^16 units and the grid stride of every kernel
  keep      a group of 300 with the best unit first, last and in the middle; score ties; qualities below '!'; both rules
  knobs     40 different keys with 1..5 units each: at hash_bits 1 and 3 every run mixes keys and takes several rounds
  VARIANTS  hash_bits 1, 3, 8, 40 x seed 0, 5 on the small cases: same bytes and statistics but mixed_runs, max_run, rounds
"""
import functools
import random
from tests import pairs_model as P
from tests.pairs_model import Refused, E_ARG, E_TOO_LONG, MAX_READ_LEN, rec
from tests.pairs_repair_model import fmix64, name_hash, sort_key, M64, GOLD

KINDS_MAX = 1024
HASH_STATS = ("mixed_runs", "max_run", "rounds")


# ---------------------------------------------------------------- the hash
def unit_hash(keys, seed=0):
    """single-end: H(seq) = name_hash; paired: fmix64(H(seq1) ^ fmix64(H(seq2) + GOLD)) -- not commutative"""
    h = name_hash(keys[0], seed)
    for k in keys[1:]:
        h = fmix64(h ^ fmix64((name_hash(k, seed) + GOLD) & M64))
    return h


# ---------------------------------------------------------------- the definition
def _opts(keep=0, hash_bits=40, seed=0, reserved=(0, 0)):
    reserved = tuple(reserved) if hasattr(reserved, "__len__") else (reserved, 0)
    if any(reserved):
        raise Refused(E_ARG, "bfq_dedup_opts.reserved: must be 0")
    if keep > 1:
        raise Refused(E_ARG, "bfq_dedup_opts.keep: must be 0 or 1")
    if not 1 <= hash_bits <= 40:
        raise Refused(E_ARG, "bfq_dedup_opts.hash_bits: must be 1..40")
    return keep, hash_bits, seed


def _line(body, k):
    """line k of a record's bytes without its LF and one trailing CR"""
    l = body.split(b"\n")[k]
    return l[:-1] if l.endswith(b"\r") else l


def dedup(texts, **opts):
    keep, hash_bits, seed = _opts(**opts)
    texts = list(texts) + [None] * (2 - len(texts))
    nt = 1 if texts[1] is None else 2
    for k in range(nt):
        P._gzip(texts[k], "FASTQ dedup: text %d is" % k)
    recs = [[body for _, body in P.records(t)] if t is not None else [] for t in texts[:nt]]
    if nt == 2 and len(recs[0]) != len(recs[1]):
        raise Refused(E_ARG, "FASTQ dedup: text 0 holds %d reads, text 1 holds %d" % (len(recs[0]), len(recs[1])))
    N = len(recs[0])
    keys = [tuple(_line(recs[k][g], 1) for k in range(nt)) for g in range(N)]
    score = [sum(max(b - 33, 0) for k in range(nt) for b in _line(recs[k][g], 3)) & M64 for g in range(N)]
    # the runs of equal sort key: what the library cuts into groups in rounds, and what it refuses
    runs = {}
    for g, k in enumerate(keys):
        runs.setdefault(sort_key(unit_hash(k, seed), hash_bits), []).append(g)
    kinds = {s: len({keys[g] for g in r}) for s, r in runs.items()}
    bad = [r[0] for s, r in runs.items() if kinds[s] > KINDS_MAX]
    if bad:
        raise Refused(E_ARG, "FASTQ dedup: more than 1024 different sequences share a hash (the first: record %d)" % min(bad))
    groups = {}
    for g, k in enumerate(keys):
        groups.setdefault(k, []).append(g)
    kept = set()
    for members in groups.values():
        kept.add(members[0] if not keep else min(members, key=lambda g: (-score[g], g)))
    outs = [b"".join(recs[k][g] for g in range(N) if g in kept) for k in range(nt)] + [b""] * (2 - nt)
    dups = [b"".join(recs[k][g] for g in range(N) if g not in kept) for k in range(nt)] + [b""] * (2 - nt)
    sizes = [len(m) for m in groups.values()]
    big = max(sizes or [0])
    lg, lu = [0] * 32, [0] * 32
    for n in sizes:
        lg[min(n.bit_length() - 1, 31)] += 1
        lu[min(n.bit_length() - 1, 31)] += n
    st = dict(units=N, kept=len(kept), removed=N - len(kept), dup_groups=sum(n >= 2 for n in sizes), max_group=big,
              max_group_first=min([m[0] for m in groups.values() if len(m) == big] or [0]), level_groups=lg, level_units=lu,
              out_len=[len(o) for o in outs], dup_len=[len(d) for d in dups], mixed_runs=sum(v > 1 for v in kinds.values()),
              max_run=max([len(r) for r in runs.values()] or [0]), rounds=max(list(kinds.values()) or [0]))
    return outs, dups, st


# ---------------------------------------------------------------- the cases
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def _seq(rng, L, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(L))


def _quals(rng, L):
    return bytes(rng.randrange(35, 75) for _ in range(L))


def length_couples():
    """[(a, b, equal)]: per length an equal couple, one that differs in the last byte only, one in the first byte only"""
    rng = random.Random(31)
    out = [(b"", b"", True), (b"A", b"A", True), (b"C", b"G", False), (b"T", b"N", False)]
    for L in LENGTHS[2:]:
        a, b, c = (_seq(rng, L) for _ in range(3))
        out += [(a, a, True), (b, b[:-1] + (b"N" if b[-1:] != b"N" else b"A"), False), (c, (b"N" if c[:1] != b"N" else b"A") + c[1:], False)]
    return out


def _lengths_text():
    rng = random.Random(32)
    seqs = [s for a, b, _ in length_couples() for s in (a, b)]
    order = list(range(len(seqs)))
    rng.shuffle(order)
    return b"".join(rec(b"@l%d" % j, seqs[j], _quals(rng, len(seqs[j]))) for j in order), len(seqs)


def _const_text(n, seq=b"ACGTTGCA"):
    return b"".join(rec(b"@c%d" % j, seq) for j in range(n))


def _keys_text():
    rng = random.Random(33)
    base = _seq(rng, 40)
    seqs = [base[:L] for L in (8, 9, 16, 17, 33, 34)] + [b"acgtacgt", b"ACGTACGT", b"ACGTACGt", b"NNNN", b"NNNN", b"NNNNN", b"NNNN", b"N" * 150, b"N" * 150]
    return b"".join(rec(b"@k%d" % j, s, _quals(rng, len(s))) for j, s in enumerate(seqs))


def _lines_text():
    s = b"ACGTACGTACGTACGTAC"
    return (rec(b"@a", s, eol=b"\r\n") + rec(b"@b other", s, b"#" * len(s), plus=b"+b") + rec(b"@c", s[:-1], eol=b"\r\n") +
            rec(b"@d", s[:-1] + b"\r", b"I" * 17) + rec(b"@f", b"", eol=b"\r\n") + rec(b"@g", b"") + rec(b"@e", s, b"J" * len(s), eol=b"\r\n"))


# ---- different sequences with EQUAL full hashes: what the comparison of lengths and bytes alone keeps apart
# The hash is a sum of fmix64(w_j + GOLD * (j + 1)) over the 8-byte chunks, so two chunks j < k may change places: with
# d = GOLD * (k - j), the lines (.. w_j .. w_k ..) and (.. w_k + d .. w_j - d ..) have equal sums, equal lengths and so equal
# hashes under every seed.  (Lines of one length that differ inside ONE chunk only -- "the last byte only" -- cannot collide:
# fmix64 is a bijection.)  A line and the line with one more chunk behind it collide where that chunk is solved for through
# the inverse of fmix64; this holds for the seed it was solved for.
def fmix64_inverse(x):
    x ^= x >> 33
    x = (x * pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)) & M64
    x ^= x >> 33
    x = (x * pow(0xff51afd7ed558ccd, -1, 1 << 64)) & M64
    x ^= x >> 33
    return x


def _clean(b):
    return 10 not in b and 13 not in b


def collide_swap(rng, L, j, k):
    """two different lines of L bytes with equal hashes that differ in chunks j and k only; chunk k may be the partial last one"""
    nk = min(8, L - 8 * k)
    assert 0 <= j < k and 8 * k < L and 1 <= nk
    d = (GOLD * (k - j)) & M64
    while True:
        x = bytearray(_seq(rng, L))
        xk = int.from_bytes(x[8 * k:8 * k + nk], "little")
        if nk == 8:
            xj = int.from_bytes(x[8 * j:8 * j + 8], "little")
            yj, yk = (xk + d) & M64, (xj - d) & M64
        else:                                                      # both last chunks stay inside their nk bytes
            yk = int.from_bytes(_seq(rng, nk), "little")
            xj, yj = (yk + d) & M64, (xk + d) & M64
            x[8 * j:8 * j + 8] = xj.to_bytes(8, "little")
        y = bytearray(x)
        y[8 * j:8 * j + 8] = yj.to_bytes(8, "little")
        y[8 * k:8 * k + nk] = yk.to_bytes(nk, "little")
        x, y = bytes(x), bytes(y)
        if x != y and _clean(x) and _clean(y):
            assert name_hash(x) == name_hash(y) and name_hash(x, 5) == name_hash(y, 5) and len(x) == len(y) == L
            return x, y


def collide_prefix(rng, L, seed=0):
    """a line of L bytes (a multiple of 8) and the line of L + 8 bytes that it is a proper prefix of, with equal hashes at `seed`"""
    assert L % 8 == 0
    while True:
        x = _seq(rng, L)
        acc = 0
        for j in range(0, L, 8):
            acc = (acc + fmix64((int.from_bytes(x[j:j + 8], "little") + GOLD * (j // 8 + 1)) & M64)) & M64
        want = acc ^ fmix64((L ^ seed) & M64) ^ fmix64(((L + 8) ^ seed) & M64)      # the sum the longer line must have
        w = (fmix64_inverse((want - acc) & M64) - GOLD * (L // 8 + 1)) & M64
        y = x + w.to_bytes(8, "little")
        if _clean(y):
            assert name_hash(x, seed) == name_hash(y, seed)
            return x, y


@functools.lru_cache(maxsize=None)
def collide_couples():
    """[(a, b, what)]: at 16 / 17, 64 / 65 and 256 / 257 bytes a couple that differs in the first 16-byte step only and one that
    differs in the last chunks only (at 17, 65, 257: in the byte behind the last whole step and the chunk before it); at 256 /
    257 one whose chunks lie in 16-byte steps 7 and 8 (two turns of a lane's loop); prefixes of 8, 16, 64 and 256 bytes"""
    rng = random.Random(40)
    out = []
    for L in (16, 17, 64, 65, 256, 257):
        last = (L - 1) // 8
        if L > 17:
            out.append(collide_swap(rng, L, 0, 1) + ("first",))
        out.append(collide_swap(rng, L, last - 1, last) + ("last",))
        if L >= 256:
            out.append(collide_swap(rng, L, 15, 16) + ("middle",))
    for L in (8, 16, 64, 256):
        out.append(collide_prefix(rng, L) + ("prefix",))
    return out


def _collide_text():
    """every couple's first line twice and its second once, scattered: kept are one of each"""
    rng = random.Random(41)
    seqs = [s for a, b, _ in collide_couples() for s in (a, b, a)]
    rng.shuffle(seqs)
    return b"".join(rec(b"@x%d" % j, s, _quals(rng, len(s))) for j, s in enumerate(seqs)), len(seqs)


def _pairs_mix():
    """pairs that must stay apart, and one duplicated pair among them"""
    m1 = [b"ACGTACGT", b"ACGTACGT", b"AC", b"A", b"GATTACA", b"TTTT", b"ACGTACGT", b"GATTACA", b"", b"C", b"TTTG"]
    m2 = [b"TTTT", b"TTTA", b"G", b"CG", b"TTTT", b"GATTACA", b"TTTT", b"TTTG", b"C", b"", b"GATTACA"]
    rng = random.Random(34)
    return (b"".join(rec(b"@p%d/1" % j, s, _quals(rng, len(s))) for j, s in enumerate(m1)),
            b"".join(rec(b"@p%d/2" % j, s, _quals(rng, len(s))) for j, s in enumerate(m2)))


GROUP_SIZES = (1, 2, 3, 64, 65, 256, 257, 1024, 1025, 4097)


@functools.lru_cache(maxsize=None)
def _groups_text():
    rng = random.Random(35)
    seqs = []
    for n in GROUP_SIZES:
        s = _seq(rng, rng.randrange(20, 41))
        seqs += [s] * n
    rng.shuffle(seqs)
    return b"".join(rec(b"@g%d" % j, s, _quals(rng, len(s))) for j, s in enumerate(seqs))


WIDE_N, WIDE_BIG = 70000, 40000


@functools.lru_cache(maxsize=None)
def _wide_text():
    rng = random.Random(20250301)
    big = _seq(rng, 36)
    seqs = [big] * WIDE_BIG
    for j in range(40):
        seqs += [_seq(rng, 36)] * (3 + (j * 297) // 39)
    while len(seqs) < WIDE_N:
        seqs.append(_seq(rng, 36))
    rng.shuffle(seqs)
    q = bytes(rng.randrange(35, 75) for _ in range(36 + 997))
    return b"".join(rec(b"@w%d" % j, s, q[j % 997:j % 997 + 36]) for j, s in enumerate(seqs))


def _keep_text(best_at):
    """a group of 300 scattered among 100 others; the unit with the best qualities is the group's first, last or middle one;
    two units tie below it; a unit whose qualities lie below '!' counts 0"""
    rng = random.Random(36)
    s = _seq(rng, 50)
    members = [rec(b"@m%d" % j, s, bytes(rng.randrange(40, 60) for _ in range(50))) for j in range(300)]
    members[{"first": 0, "last": 299, "middle": 150}[best_at]] = rec(b"@best", s, b"~" * 50)
    members[7 if best_at != "first" else 9] = rec(b"@low", s, b" \x01 \x1f " * 10)
    others = [rec(b"@o%d" % j, _seq(rng, 50), _quals(rng, 50)) for j in range(100)]
    slots = sorted(rng.sample(range(400), 300))
    out, mi, oi = [], 0, 0
    for j in range(400):
        if mi < 300 and slots[mi] == j:
            out.append(members[mi]); mi += 1
        else:
            out.append(others[oi]); oi += 1
    return b"".join(out)


def _ties_text():
    """score ties go to the smallest g; qualities below '!' count 0, not negative"""
    a, b = b"ACGTACGTAC", b"TTGACCAGTA"
    return (rec(b"@t0", a, b"5555555555") + rec(b"@t1", b, b" " * 10) + rec(b"@t2", a, b"::::::::::") + rec(b"@t3", a, b"::::::::::") +
            rec(b"@t4", b, b"\x01" * 10) + rec(b"@t5", b, b"!" * 10) + rec(b"@t6", a, b"5:5:5:5:5:") + rec(b"@t7", b, b"!!!!!!!!!\"") + rec(b"@t8", b, b"\"!!!!!!!!!"))


def _knobs_text():
    rng = random.Random(37)
    seqs = []
    for j in range(40):
        seqs += [_seq(rng, 10 + j)] * (1 + j % 5)
    rng.shuffle(seqs)
    return b"".join(rec(b"@h%d" % j, s, _quals(rng, len(s))) for j, s in enumerate(seqs))


@functools.lru_cache(maxsize=None)
def cases():
    """label -> (texts, opts)"""
    rng = random.Random(38)
    one, other = rec(b"@solo", b"ACGTTGCAAC", b"IIIIIHHHHH"), rec(b"@else", b"ACGTTGCAAT")
    lt, ln = _lengths_text()
    p1, p2 = _pairs_mix()
    c = {
        "absent": ((None, None), {}), "empty": ((b"", None), {}), "empty-paired": ((b"", b""), {}),
        "n1": ((one, None), {}), "n1-paired": ((one, other), {}),
        "two-equal": ((one + rec(b"@again x", b"ACGTTGCAAC", b"##########", plus=b"+again"), None), {}), "two-different": ((one + other, None), {}),
        "two-equal-paired": ((one + one, other + other), {}), "two-different-paired": ((one + one, other + one), {}),
        "lengths": ((lt, None), {}), "lengths-mate-2": ((_const_text(ln), lt), {}), "lengths-mate-1": ((lt, _const_text(ln)), {}),
        "collide": ((_collide_text()[0], None), {}), "collide-mate-2": ((_const_text(_collide_text()[1]), _collide_text()[0]), {}),
        "collide-mate-1": ((_collide_text()[0], _const_text(_collide_text()[1])), dict(keep=1)),
        "keys": ((_keys_text(), None), {}), "lines": ((_lines_text(), None), {}), "lines-nolf": ((_lines_text()[:-1], None), {}),
        "lines-paired-nolf": ((_lines_text()[:-1], _lines_text()[:-1]), {}),
        "pairs-mix": ((p1, p2), {}), "pairs-mix-best": ((p1, p2), dict(keep=1)),
        "groups": ((_groups_text(), None), {}), "groups-best": ((_groups_text(), None), dict(keep=1)),
        "wide": ((_wide_text(), None), {}),
        "keep-first": ((_keep_text("first"), None), dict(keep=1)), "keep-last": ((_keep_text("last"), None), dict(keep=1)),
        "keep-middle": ((_keep_text("middle"), None), dict(keep=1)), "keep-middle-rule-0": ((_keep_text("middle"), None), dict(keep=0)),
        "keep-middle-paired": ((_const_text(400), _keep_text("middle")), dict(keep=1)),
        "ties": ((_ties_text(), None), dict(keep=1)), "ties-rule-0": ((_ties_text(), None), dict(keep=0)),
        "knobs": ((_knobs_text(), None), {}), "knobs-best": ((_knobs_text(), None), dict(keep=1)),
    }
    return c


VARIANTS = tuple(dict(hash_bits=b, seed=s) for b in (1, 3, 8, 40) for s in (0, 5) if (b, s) != (40, 0))
LARGE = ("groups", "groups-best", "wide")
BASE_NAMES = tuple(cases().keys())
VARIED = ("collide", "collide-mate-2", "knobs", "knobs-best", "lengths", "lengths-mate-2", "keys", "lines", "pairs-mix", "pairs-mix-best", "ties", "two-equal-paired")


def _label(name, var):
    return name + "".join("~%s=%d" % kv for kv in sorted(var.items()))


@functools.lru_cache(maxsize=None)
def all_cases():
    c = dict(cases())
    for name in VARIED:
        texts, opts = cases()[name]
        for var in VARIANTS:
            c[_label(name, var)] = (texts, dict(opts, **var))
    c["groups~hash_bits=3"] = (cases()["groups"][0], dict(hash_bits=3))           # the large groups inside mixed runs
    c["groups-best~hash_bits=1"] = (cases()["groups"][0], dict(keep=1, hash_bits=1))
    return c


NAMES = tuple(all_cases().keys())
SMALL_NAMES = tuple(n for n in NAMES if n.split("~")[0] not in LARGE)


@functools.lru_cache(maxsize=None)
def expect(name):
    """(kept[2], removed[2], stats) of a case by the model"""
    texts, opts = all_cases()[name]
    outs, dups, st = dedup(texts, **opts)
    base = name.split("~")[0]
    if base != name:                                               # a variant: the bytes and every statistic but three are the base case's
        bo, bd, bst = expect(base)
        assert (outs, dups) == (bo, bd) and {k: v for k, v in st.items() if k not in HASH_STATS} == {k: v for k, v in bst.items() if k not in HASH_STATS}, name
        if opts.get("hash_bits", 40) <= 3 and st["units"] >= 20:
            assert st["mixed_runs"] >= 1 and 2 <= st["rounds"] <= 40, name     # the case really mixes keys in a run, and not too many
    return outs, dups, st


def _different(n, L=12, seed=39):
    rng, seen = random.Random(seed), set()
    while len(seen) < n:
        seen.add(_seq(rng, L))
    return sorted(seen)


KINDS_MSG = "FASTQ dedup: more than 1024 different sequences share a hash (the first: record %d)"


@functools.lru_cache(maxsize=None)
def kinds_text():
    """2100 different sequences behind three equal ones: at hash_bits = 1 one of the two runs holds more than 1024 keys"""
    return rec(b"@s", b"ACGT") * 3 + b"".join(rec(b"@d%d" % j, s) for j, s in enumerate(_different(2100)))


@functools.lru_cache(maxsize=None)
def refusals():
    """label -> (texts, opts, code, message)"""
    g = _knobs_text()
    n = len(P.records(g))
    kt = kinds_text()
    first = min(r[0] for r in _runs(kt, 1, 0).values() if len({k for _, k in r_keys(kt, r)}) > KINDS_MAX)
    r = {
        "gzip": ((b"\x1f\x8b\x08\x04" + g, None), {}, E_ARG, "FASTQ dedup: text 0 is compressed (it begins with 1f 8b): inflate the text first"),
        "gzip-1": ((g, b"\x1f\x8b" + g), {}, E_ARG, "FASTQ dedup: text 1 is compressed (it begins with 1f 8b): inflate the text first"),
        "lines": ((g + b"@x\nA\n", None), {}, E_ARG, "FASTQ: number of lines is not a multiple of 4"),
        "lines-1": ((g, g + b"@x\nA\n"), {}, E_ARG, "FASTQ: number of lines is not a multiple of 4"),
        "lengths": ((g + rec(b"@x", b"ACG", b"II"), None), {}, E_ARG, "FASTQ: len(DNA) != len(QS) in a record"),
        "too-long": ((g, g + rec(b"@x", b"A" * (MAX_READ_LEN + 1))), {}, E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN"),
        "counts": ((g, g + rec(b"@x", b"A")), {}, E_ARG, "FASTQ dedup: text 0 holds %d reads, text 1 holds %d" % (n, n + 1)),
        "counts-empty": ((g, b""), {}, E_ARG, "FASTQ dedup: text 0 holds %d reads, text 1 holds 0" % n),
        "reserved": ((g, None), dict(reserved=(1, 0)), E_ARG, "bfq_dedup_opts.reserved: must be 0"),
        "reserved-1": ((g, None), dict(reserved=(0, 7)), E_ARG, "bfq_dedup_opts.reserved: must be 0"),
        "keep-2": ((g, None), dict(keep=2), E_ARG, "bfq_dedup_opts.keep: must be 0 or 1"),
        "hash-bits-0": ((g, None), dict(hash_bits=0), E_ARG, "bfq_dedup_opts.hash_bits: must be 1..40"),
        "hash-bits-41": ((g, None), dict(hash_bits=41), E_ARG, "bfq_dedup_opts.hash_bits: must be 1..40"),
        "kinds": ((kt, None), dict(hash_bits=1), E_ARG, KINDS_MSG % first),
        "kinds-best": ((kt, None), dict(hash_bits=1, keep=1), E_ARG, KINDS_MSG % first),
    }
    for name, (texts, opts, code, msg) in r.items():                # the model agrees with the table
        try:
            dedup(texts, **opts)
            raise AssertionError(name)
        except Refused as e:
            assert (e.code, e.msg) == (code, msg), (name, e.msg)
    st = dedup((kt, None), hash_bits=2)[2]                          # the same text is no refusal at 2 bits: four runs of about 525 keys
    assert st["units"] == 2103 and st["kept"] == 2101 and st["rounds"] <= KINDS_MAX
    return r


def r_keys(text, run):
    recs = [b for _, b in P.records(text)]
    return [(g, _line(recs[g], 1)) for g in run]


def _runs(text, hash_bits, seed):
    runs = {}
    for g, (_, body) in enumerate(P.records(text)):
        runs.setdefault(sort_key(unit_hash((_line(body, 1),), seed), hash_bits), []).append(g)
    return runs


def wide_counts():
    """(units, the largest group, groups of 3..300, unique units) of the wide case, by counting sequences"""
    count = {}
    for _, body in P.records(_wide_text()):
        count[_line(body, 1)] = count.get(_line(body, 1), 0) + 1
    sizes = sorted(count.values())
    return sum(sizes), sizes[-1], sum(3 <= n <= 300 for n in sizes), sum(n == 1 for n in sizes)
