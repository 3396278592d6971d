"""The k-mer spectrum report (include/bfqzip_hip.h, bfq_fastq_kmers) stated in Python: collections.Counter over byte strings.
Shares no code with the library.  kmers(a_parts, b_parts, ...) -> the report as a dict of ints and lists, with the key "list":
every listed k-mer (solid -> absent or absent -> solid) as (value, count_a, count_b), ascending, uncut."""
import functools
from collections import Counter

SCALARS = ("k", "solid", "canonical", "n_partitions", "n_reads_a", "n_reads_b", "reads_short_a", "reads_short_b", "windows_a", "windows_b",
           "windows_skipped_a", "windows_skipped_b", "distinct_a", "distinct_b", "distinct_both", "only_a", "only_b", "occ_only_a",
           "occ_only_b", "distinct_changed", "n_listed")
ARRAYS = ("hist_a", "hist_b", "joint", "trans")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
CODE = {65: 0, 67: 1, 71: 2, 84: 3}
MAX_READ_LEN = 65000
TOP_BITS = 12


class Malformed(Exception):
    pass


def sequences(parts):
    """The sequence lines of a text given in parts: a part without its final newline gets one; four lines per record; a CR
    before the LF is dropped."""
    text = b"".join(p if not p or p.endswith(b"\n") else p + b"\n" for p in (bytes(p) for p in parts))
    lines = text.split(b"\n")[:-1] if text else []
    if len(lines) % 4:
        raise Malformed("FASTQ: number of lines is not a multiple of 4")
    strip = lambda l: l[:-1] if l.endswith(b"\r") else l
    seqs = [strip(l) for l in lines[1::4]]
    if any(len(s) != len(strip(q)) for s, q in zip(seqs, lines[3::4])):
        raise Malformed("FASTQ: len(DNA) != len(QS) in a record")
    if any(len(s) > MAX_READ_LEN for s in seqs):
        raise Malformed("read longer than BFQ_MAX_READ_LEN")
    return seqs


def value(w):
    v = 0
    for c in w:
        v = 4 * v + CODE[c]
    return v


def count(seqs, k, canonical):
    """(Counter of k-mer strings, reads shorter than k, valid windows, skipped windows)"""
    cnt, short, valid, skipped = Counter(), 0, 0, 0
    for s in seqs:
        if len(s) < k:
            short += 1
            continue
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if len(w.translate(None, b"ACGT")):
                skipped += 1
                continue
            valid += 1
            if canonical:
                r = w.translate(COMP)[::-1]
                if r < w:                                        # A < C < G < T as bytes and as codes
                    w = r
            cnt[w] += 1
    return cnt, short, valid, skipped


def ranges(cnt_a, cnt_b, k, part_records):
    """The value ranges as lists of bins: the non-empty bins of the top 12 bits in ascending order, a bin joining the range
    before it while the range's records stay within part_records (0: no bound).  Empty bins belong to nobody."""
    bins = Counter()
    for c in (cnt_a, cnt_b):
        for w, n in c.items():
            bins[value(w) >> (2 * k - TOP_BITS)] += n
    out, s = [], 0
    for b in sorted(bins):
        if not out or (part_records and s + bins[b] > part_records):
            out.append([])
            s = 0
        out[-1].append(b)
        s += bins[b]
    return out, bins


@functools.lru_cache(maxsize=64)
def _counted(parts, k, canonical):
    return count(sequences(parts), k, canonical)


def kmers(a_parts, b_parts=None, k=21, solid=3, canonical=True, part_records=0):
    sa = sequences(a_parts)
    sb = sequences(b_parts) if b_parts else []
    ca, short_a, va, ska = _counted(tuple(bytes(p) for p in a_parts), k, bool(canonical))
    cb, short_b, vb, skb = _counted(tuple(bytes(p) for p in b_parts), k, bool(canonical)) if b_parts else (Counter(), 0, 0, 0)
    R = {"k": k, "solid": solid, "canonical": int(bool(canonical)), "n_partitions": len(ranges(ca, cb, k, part_records)[0]),
         "n_reads_a": len(sa), "n_reads_b": len(sb), "reads_short_a": short_a, "reads_short_b": short_b, "windows_a": va, "windows_b": vb,
         "windows_skipped_a": ska, "windows_skipped_b": skb, "distinct_a": len(ca), "distinct_b": len(cb)}
    hist_a, hist_b, joint, trans = [0] * 256, [0] * 256, [0] * 256, [0] * 9
    both = only_a = only_b = occ_a = occ_b = changed = 0
    cls = lambda c: 0 if c == 0 else 1 if c < solid else 2
    listed = []
    for w in set(ca) | set(cb):
        x, y = ca.get(w, 0), cb.get(w, 0)
        if x:
            hist_a[min(x, 255)] += 1
        if y:
            hist_b[min(y, 255)] += 1
        joint[16 * min(x, 15) + min(y, 15)] += 1
        trans[3 * cls(x) + cls(y)] += 1
        both += 1 if x and y else 0
        if not y:
            only_a += 1; occ_a += x
        if not x:
            only_b += 1; occ_b += y
        changed += 1 if x != y else 0
        if (cls(x), cls(y)) in ((2, 0), (0, 2)):
            listed.append((value(w), min(x, 2 ** 32 - 1), min(y, 2 ** 32 - 1)))
    listed.sort()
    R.update(distinct_both=both, only_a=only_a, only_b=only_b, occ_only_a=occ_a, occ_only_b=occ_b, distinct_changed=changed,
             n_listed=len(listed), counts=(ca, cb), hist_a=hist_a, hist_b=hist_b, joint=joint, trans=trans, list=listed)
    return R


def kmer_string(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))
