"""Repair of paired FASTQ in plain Python: the definition of bfq_fastq_repair* (csrc/bfq_pairs.h) over lists of records, the
name hash, and the named cases the host and GPU tests share.  Nothing here imports the library.

  repair(texts, ...) -> ([text 0 (singletons), text 1, text 2], stats)      the model of bfq_fastq_repair*
  name_hash(key, seed)                                                       the hash of csrc/bfq_pairs.h (bfq_repair_hash)

The outputs are computed from the definition alone -- groups of equal keys, the lists L1, L2, L0, the order by anchor --; the
hash enters only the statistics mixed_runs and max_run and the refusal of a run above RUN_MAX, as in the library.

Cases (every one built once and shared; texts = (text 0, text 1, text 2)):
  counts    N = 0 (absent texts, empty texts), 1, 2; two filtered mate files of 65, 300, 3073, 4097 and 6200 records in all
            (a wave, a workgroup, a radix tile, the scan chunk, two radix tiles); "wide": about 70 000 short records, about
            5 MB, shuffled mates, a tenth dropped on each side, some names twice
  sources   filtered mate files; one mixed text 0 with /1 /2 where /2 stands in front of /1; a text 0 without suffixes (L0
            is paired); all three texts at once; the same bytes as text 1 and as text 0 (different, defined results)
  keys      lengths 0, 1, 7, 8, 9, 16, 17 and 300; keys that differ only in the last byte, only in length, or only by a trailing
            zero byte against the end of the key; CR, tab and comment behind the key; mate_suffix = 0
  groups    sizes 1, 2, 3 and 4 with every mix of hints, in the mate files + text 0 and in one mixed text 0; a name twice in
            text 1 against once in text 2
  bound     1024 equal names: 512 pairs from L0
  form      no final LF in each text; CRLF lines
  VARIANTS  the small cases again at hash_bits 1 and 3 and at other seeds: same bytes, other mixed_runs / max_run
"""
import functools
import random
from tests import pairs_model as P
from tests.pairs_model import Refused, E_ARG, E_TOO_LONG, MAX_READ_LEN, rec

RUN_MAX = 1024
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------- the hash
def fmix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def name_hash(key, seed=0):
    """8-byte little-endian chunks w_j, the last zero-padded: acc = sum fmix64(w_j + GOLD * (j + 1)); h = fmix64(acc ^ fmix64(L ^ seed))"""
    acc = 0
    for j in range(0, len(key), 8):
        acc = (acc + fmix64((int.from_bytes(key[j:j + 8], "little") + GOLD * (j // 8 + 1)) & M64)) & M64
    return fmix64(acc ^ fmix64((len(key) ^ seed) & M64))


def sort_key(h, hash_bits):
    return h >> (64 - hash_bits)


# ---------------------------------------------------------------- the definition
def _opts(mate_suffix=1, hash_bits=40, seed=0, reserved=(0, 0)):
    reserved = tuple(reserved) if hasattr(reserved, "__len__") else (reserved, 0)
    if any(reserved):
        raise Refused(E_ARG, "bfq_repair_opts.reserved: must be 0")
    if not 1 <= hash_bits <= 40:
        raise Refused(E_ARG, "bfq_repair_opts.hash_bits: must be 1..40")
    return mate_suffix, hash_bits, seed


def hint(header, src, mate_suffix):
    """1 from text 1, 2 from text 2; from text 0, with mate_suffix, by the suffix the key lost; else 0"""
    if src:
        return src
    raw, k = P.key(header, 0), P.key(header, mate_suffix)
    return 0 if len(raw) == len(k) else 1 if raw.endswith(b"/1") else 2


def repair(texts, **opts):
    mate_suffix, hash_bits, seed = _opts(**opts)
    texts = list(texts) + [None] * (3 - len(texts))
    for k in range(3):
        P._gzip(texts[k], "FASTQ repair: text %d is" % k)
    recs = [P.records(t) if t is not None else [] for t in texts]
    G = [(src, i, h, body) for src in (1, 2, 0) for i, (h, body) in enumerate(recs[src])]       # global order: texts 1, 2, 0
    keys = [P.key(h, mate_suffix) for _, _, h, _ in G]
    hints = [hint(h, src, mate_suffix) for src, _, h, _ in G]
    # the runs of equal sort key: what the library walks, and what it refuses
    runs = {}
    for g, k in enumerate(keys):
        runs.setdefault(sort_key(name_hash(k, seed), hash_bits), []).append(g)
    too_long = [r[0] for r in runs.values() if len(r) > RUN_MAX]
    if too_long:
        src, i = G[min(too_long)][:2]
        raise Refused(E_ARG, "FASTQ repair: more than 1024 records share a name or a name hash (the first: record %d of text %d): "
                             "names do not identify the mates" % (i, src))
    groups = {}
    for g, k in enumerate(keys):
        groups.setdefault(k, []).append(g)
    pairs, role = [], [0] * len(G)
    for members in groups.values():
        L = [[g for g in members if hints[g] == w] for w in range(3)]
        for k in range(min(len(L[1]), len(L[2]))):
            pairs.append((L[1][k], L[2][k]))
        for j in range(len(L[0]) // 2):
            pairs.append((L[0][2 * j], L[0][2 * j + 1]))
    pairs.sort()
    for a, b in pairs:
        role[a], role[b] = 1, 2
    outs = [b"".join(G[g][3] for g in range(len(G)) if role[g] == 0), b"".join(G[a][3] for a, _ in pairs), b"".join(G[b][3] for _, b in pairs)]
    st = dict(records=len(G), pairs=len(pairs), singles=role.count(0), out_len=[len(o) for o in outs], n_in=[len(r) for r in recs],
              dup_groups=sum(len(m) > 2 for m in groups.values()), mixed_runs=sum(len({keys[g] for g in r}) > 1 for r in runs.values()),
              max_run=max([len(r) for r in runs.values()] or [0]))
    return outs, st


# ---------------------------------------------------------------- the cases
def _read(rng, header, lo=5, hi=40):
    L = rng.randrange(lo, hi + 1)
    return rec(header, bytes(rng.choice(b"ACGTN") for _ in range(L)), bytes(rng.randrange(35, 75) for _ in range(L)))


def filtered(total, seed, dups=0):
    """two mate files of `total` records in all: names f<k>, a tenth of each side dropped on its own, text 2 shuffled; `dups`
    names stand twice in text 1"""
    rng = random.Random(seed)
    names = list(range(total * 5 // 9 + 2))
    one = [k for k in names if rng.random() >= 0.1]
    two = [k for k in names if rng.random() >= 0.1]
    one += one[:dups]
    rng.shuffle(two)
    while len(one) + len(two) > total:
        two.pop()
    extra = 0
    while len(one) + len(two) < total:
        one.append(10 ** 7 + extra)
        extra += 1
    c = (b"", b" 1:N:0:ACGT", b"\tBC:Z:AC")
    t1 = b"".join(_read(rng, b"@f%d/1%s" % (k, c[k % 3])) for k in one)
    t2 = b"".join(_read(rng, b"@f%d/2%s" % (k, c[(k + 1) % 3])) for k in two)
    return (None, t1, t2)


def _mixed_suffix(seed=11):
    """one text 0: names with /1 and /2 in any order (for every third name /2 in front of /1), some mates missing"""
    rng = random.Random(seed)
    items = []
    for k in range(120):
        w = [b"/2", b"/1"] if k % 3 == 0 else [b"/1", b"/2"]
        if k % 10 == 7:
            w = w[:1]
        items.append([_read(rng, b"@m%d%s" % (k, s)) for s in w])
    order = [(rng.random(), j, d) for j, it in enumerate(items) for d in range(len(it))]
    order.sort(key=lambda x: (x[0] if x[1] % 2 else x[1], x[2]))       # even names keep their place, odd ones are scattered
    return b"".join(items[j][d] for _, j, d in order)


def _mixed_plain(seed=12):
    """one text 0 without suffixes: groups of 1, 2, 3 and 4 records of one name, scattered"""
    rng = random.Random(seed)
    rs = [_read(rng, b"@p%d%s" % (k, (b"", b" c")[d & 1])) for k in range(80) for d in range(1 + k % 4)]
    rng.shuffle(rs)
    return b"".join(rs)


KEYS = (b"", b"a", b"abcdefg", b"abcdefgh", b"abcdefghi", b"0123456789abcdef", b"0123456789abcdefg", b"k" * 300)
NEAR = ((b"abcdefgh", b"abcdefgi"), (b"abcdefg", b"abcdefg\0"), (b"abcdefgh\0", b"abcdefgh"), (b"abcdefgh\0\0\0\0\0\0\0\0", b"abcdefgh\0\0\0\0\0\0\0"),
        (b"k" * 299 + b"j", b"k" * 299 + b"i"), (b"0123456789abcdeX", b"0123456789abcdeY"), (b"z", b"zz"), (b"\0", b""))


def _keys_texts(suffix=True):
    """mates under keys of every chunk shape, and near-miss keys that must stay apart: one of each in text 1, the other in text 2"""
    rng = random.Random(13)
    t1, t2 = [], []
    for j, k in enumerate(KEYS):
        tail = (b"", b" comment", b"\tRX:Z:A", b"\r")[j % 4]
        s1, s2 = (b"/1", b"/2") if suffix and len(k) else (b"", b"")
        t1.append(_read(rng, b"@" + k + s1 + tail))
        t2.append(_read(rng, b"@" + k + s2 + (b" other", b"", b"\tRX:Z:C", b"")[j % 4]))
    for a, b in NEAR:
        if not suffix or (a and b):                               # ("@" + "/1" alone keeps its suffix: an empty key takes none)
            t1.append(_read(rng, b"@" + a + (b"/1" if suffix else b"")))
            t2.append(_read(rng, b"@" + b + (b"/2" if suffix else b"")))
    rng.shuffle(t2)
    return (None, b"".join(t1), b"".join(t2))


def _groups(mixed):
    """every mix of hints in groups of 1 .. 4 records: (c0, c1, c2) records with hints 0, 1, 2 of the name g<j>.  mixed: all of
    them in text 0, the hints through /1 and /2; else in texts 1 and 2 and, the hint-0 ones, in text 0"""
    rng = random.Random(14 + mixed)
    mixes = [(a, b, c) for a in range(5) for b in range(5) for c in range(5) if 1 <= a + b + c <= 4]
    assert len(mixes) == 34
    t = [[], [], []]
    for j, cnt in enumerate(mixes):
        for w in range(3):
            for d in range(cnt[w]):
                h = b"@g%d%s%s" % (j, (b"", b"/1", b"/2")[w] if mixed or (w and d & 1) else b"", (b"", b" x")[d & 1])
                t[0 if mixed else w].append(_read(rng, h))
    for w in range(3):
        rng.shuffle(t[w])
    return tuple(b"".join(x) if x else None for x in t)


def _all_three():
    rng = random.Random(15)
    _, t1, t2 = filtered(200, 16)
    r1, r2 = P.records(t1), P.records(t2)
    extra = [b for _, b in r1[:5]] + [b for _, b in r2[:5]]       # names that stand twice: once in a mate file, once in the mixed one
    extra += [_read(rng, b"@only%d" % k) for k in range(7)] + [_read(rng, b"@f100000/2"), _read(rng, b"@f100000/1")]
    rng.shuffle(extra)
    return (b"".join(extra), t1, t2)


@functools.lru_cache(maxsize=None)
def _wide():
    return filtered(70000, 20241101, dups=50)


@functools.lru_cache(maxsize=None)
def cases():
    """label -> (texts, opts)"""
    one = _read(random.Random(1), b"@solo/1")
    f300 = filtered(300, 3)
    both = P.merge(filtered(64, 4)[:1] + tuple(repair(filtered(64, 4))[0][1:]))[0]    # proper pairs, interleaved: x/1 x/2 x/1 ...
    kt = _keys_texts()
    c = {
        "absent": ((None, None, None), {}), "empty": ((b"", b"", b""), {}), "n1": ((None, one, None), {}),
        "n2": ((None, one, _read(random.Random(2), b"@solo/2 c")), {}), "n2-apart": ((None, one, _read(random.Random(2), b"@sole/2")), {}),
        "filtered-65": (filtered(65, 5), {}), "filtered-300": (f300, {}), "filtered-3073": (filtered(3073, 6), {}),
        "filtered-4097": (filtered(4097, 7), {}), "filtered-6200": (filtered(6200, 8, dups=9), {}),
        "mixed-suffix": ((_mixed_suffix(), None, None), {}), "mixed-suffix-kept": ((_mixed_suffix(), None, None), dict(mate_suffix=0)),
        "mixed-plain": ((_mixed_plain(), None, None), {}), "all-three": (_all_three(), {}),
        "as-text-1": ((None, both, None), {}), "as-text-0": ((both, None, None), {}),
        "keys": (kt, {}), "keys-kept": (_keys_texts(False), dict(mate_suffix=0)), "keys-mixed": ((kt[1] + kt[2], None, None), {}),
        "groups": (_groups(0), {}), "groups-mixed": (_groups(1), {}),
        "dup-r1": ((None, rec(b"@d/1", b"ACGT") + rec(b"@e/1", b"A") + rec(b"@d/1", b"TT"), rec(b"@d/2", b"GG")), {}),
        "bound-1024": ((rec(b"@same", b"ACGT") * 1024, None, None), {}),
        "nolf": (tuple(t[:-1] for t in _all_three()), {}),
        "crlf": ((None, rec(b"@c/1 x", b"ACGT", eol=b"\r\n") + rec(b"@d", b"AC", eol=b"\r\n"), rec(b"@d\r", b"GG") + rec(b"@c/2", b"TTTT", eol=b"\r\n")), {}),
        "wide": (_wide(), {}),
    }
    return c


VARIANTS = (dict(hash_bits=1), dict(hash_bits=3), dict(seed=0x1234567), dict(hash_bits=3, seed=99))
LARGE = ("filtered-3073", "filtered-4097", "filtered-6200", "wide")
BASE_NAMES = tuple(cases().keys())
SMALL = tuple(n for n in BASE_NAMES if n not in LARGE and n != "bound-1024")


def _label(name, var):
    return name + "".join("~%s=%d" % kv for kv in sorted(var.items()))


@functools.lru_cache(maxsize=None)
def all_cases():
    """label -> (texts, opts): the cases, and the small ones again under every variant"""
    c = dict(cases())
    for name in SMALL:
        texts, opts = cases()[name]
        for var in VARIANTS:
            c[_label(name, var)] = (texts, dict(opts, **var))
    return c


NAMES = BASE_NAMES + tuple(_label(n, v) for n in SMALL for v in VARIANTS)
SMALL_NAMES = tuple(n for n in NAMES if n.split("~")[0] in SMALL)


@functools.lru_cache(maxsize=None)
def expect(name):
    texts, opts = all_cases()[name]
    outs, st = repair(texts, **opts)
    base = name.split("~")[0]
    if base != name:                                               # a variant: the bytes and every statistic but two are the base case's
        bouts, bst = expect(base)
        assert outs == bouts and {k: v for k, v in st.items() if k not in ("mixed_runs", "max_run")} == {k: v for k, v in bst.items() if k not in ("mixed_runs", "max_run")}
        if opts.get("hash_bits", 40) <= 3 and st["records"] >= 20:
            assert st["mixed_runs"] >= 1, name                     # the case really holds runs of several names
    return outs, st


def _one_bucket(n, hash_bits=1, seed=0):
    """n distinct names whose sort keys at hash_bits are all 0"""
    out, k = [], 0
    while len(out) < n:
        if sort_key(name_hash(b"b%d" % k, seed), hash_bits) == 0:
            out.append(b"b%d" % k)
        k += 1
    return out


RUN_MSG = "FASTQ repair: more than 1024 records share a name or a name hash (the first: record %d of text %d): names do not identify the mates"


@functools.lru_cache(maxsize=None)
def refusals():
    """label -> (texts, opts, code, message)"""
    _, g1, g2 = filtered(40, 30)
    bucket = b"".join(rec(b"@" + n + b"/1", b"AC") for n in _one_bucket(1025))
    r = {
        "gzip": ((None, g1, b"\x1f\x8b\x08\x04" + g2), {}, E_ARG, "FASTQ repair: text 2 is compressed (it begins with 1f 8b): inflate the text first"),
        "gzip-0": ((b"\x1f\x8b" + g1, g1, g2), {}, E_ARG, "FASTQ repair: text 0 is compressed (it begins with 1f 8b): inflate the text first"),
        "lines": ((None, g1, g2 + b"@x\nA\n"), {}, E_ARG, "FASTQ: number of lines is not a multiple of 4"),
        "lengths": ((rec(b"@x", b"ACG", b"II"), g1, g2), {}, E_ARG, "FASTQ: len(DNA) != len(QS) in a record"),
        "too-long": ((None, g1 + rec(b"@x", b"A" * (MAX_READ_LEN + 1)), g2), {}, E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN"),
        "reserved": ((None, g1, g2), dict(reserved=(1, 0)), E_ARG, "bfq_repair_opts.reserved: must be 0"),
        "reserved-1": ((None, g1, g2), dict(reserved=(0, 7)), E_ARG, "bfq_repair_opts.reserved: must be 0"),
        "hash-bits-0": ((None, g1, g2), dict(hash_bits=0), E_ARG, "bfq_repair_opts.hash_bits: must be 1..40"),
        "hash-bits-41": ((None, g1, g2), dict(hash_bits=41), E_ARG, "bfq_repair_opts.hash_bits: must be 1..40"),
        "1025-equal": ((rec(b"@u", b"A") + rec(b"@v", b"C") + rec(b"@same x", b"ACGT") * 1025, g1, g2), {}, E_ARG, RUN_MSG % (2, 0)),
        "1025-equal-text-2": ((None, g1, g2 + rec(b"@", b"ACGT") * 1025), {}, E_ARG, RUN_MSG % (len(P.records(g2)), 2)),
        "1025-one-bucket": ((None, bucket, None), dict(hash_bits=1), E_ARG, RUN_MSG % (0, 1)),
    }
    for name, (texts, opts, code, msg) in r.items():                # the model agrees with the table
        try:
            repair(texts, **opts)
            raise AssertionError(name)
        except Refused as e:
            assert (e.code, e.msg) == (code, msg), (name, e.msg)
    # 1025 names of one bucket at hash_bits = 1 are no refusal at 40 bits, nor are 1024 of them at 1 bit
    assert repair((None, bucket, None))[1]["singles"] == 1025
    assert repair((None, bucket[:len(bucket) - len(rec(b"@" + _one_bucket(1025)[-1] + b"/1", b"AC"))], None), hash_bits=1)[1]["max_run"] == 1024
    return r
