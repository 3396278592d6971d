"""The statement of bfq_fastq_compare (include/bfqzip_hip.h) in numpy: what the GPU report and diff list are tested against.

compare(a_parts, b_parts, perm=None, max_diffs=0) -> dict with the fields of bfq_compare_report (ints and uint64 arrays;
'subst' flat, 36 entries) plus 'diffs' (structured array, the first max_diffs differing positions in (read, pos) order).
A refusal of the library is a Refused exception here: .kind names it, .index the read / position the message must name.
"""
import numpy as np

SYMS, POS = 6, 512
NO_READ = (1 << 64) - 1
DIFF_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("base_a", "u1"), ("base_b", "u1"), ("qual_a", "u1"), ("qual_b", "u1")])
SCALARS = ("n_reads", "total_bases", "n_diffs", "reads_changed", "reads_bases_changed", "reads_quals_changed", "bases_changed",
           "quals_changed", "quals_raised", "quals_lowered", "qual_abs_sum", "qual_sq_sum", "qual_abs_max", "first_changed_read",
           "headers_same", "headers_dropped", "headers_changed")
ARRAYS = ("subst", "qual_hist_a", "qual_hist_b", "changed_base_qual_hist", "pos_len", "pos_bases", "pos_quals", "pos_abs")

CLASS = np.full(256, 5, np.int64)
for _k, _c in enumerate(b"ACGNT"):                      # the project's order
    CLASS[_c] = _k


class Refused(ValueError):
    """kind: 'text' (malformed: .which is 'A' or 'B'), 'counts' (.counts), 'length' (.index = smallest A index, .lens),
    'perm_n' (.counts = (N of the container, records)), 'perm_entry' (.index = first offending position)."""

    def __init__(self, kind, **kw):
        super().__init__(f"{kind} {kw}")
        self.kind = kind
        self.__dict__.update(kw)


def join_parts(parts):
    """The parts as one text: a part that lacks its final newline gets one."""
    out = []
    for p in parts:
        b = bytes(p) if isinstance(p, (bytes, bytearray)) else np.asarray(p, np.uint8).tobytes()
        if b and not b.endswith(b"\n"):
            b += b"\n"
        out.append(b)
    return b"".join(out)


def records(text, which):
    """[(header, sequence, qualities)] of a text: four lines per record, a CR before LF dropped from lines 1, 2 and 4."""
    lines = text.split(b"\n")
    assert lines.pop() == b""                            # (join_parts ended the text with a newline, or it is empty)
    if len(lines) % 4:
        raise Refused("text", which=which)
    strip = lambda l: l[:-1] if l.endswith(b"\r") else l
    recs = []
    for i in range(0, len(lines), 4):
        h, s, q = strip(lines[i]), strip(lines[i + 1]), strip(lines[i + 3])
        if len(s) != len(q):
            raise Refused("text", which=which)
        recs.append((h, s, q))
    return recs


def compare(a_parts, b_parts, perm=None, max_diffs=0):
    A, B = records(join_parts(a_parts), "A"), records(join_parts(b_parts), "B")
    if len(A) != len(B):
        raise Refused("counts", counts=(len(A), len(B)))
    N = len(A)
    if perm is not None:                                 # record j of B pairs with record perm[j] of A
        perm = [int(v) for v in perm]
        if len(perm) != N:
            raise Refused("perm_n", counts=(len(perm), N))
        seen, Bo = set(), [None] * N
        for j, v in enumerate(perm):
            if v >= N or v in seen:
                raise Refused("perm_entry", index=j)
            seen.add(v)
            Bo[v] = B[j]
        B = Bo
    for i in range(N):
        if len(A[i][1]) != len(B[i][1]):
            raise Refused("length", index=i, lens=(len(A[i][1]), len(B[i][1])))
    cat = lambda k, R: np.frombuffer(b"".join(r[k] for r in R), np.uint8).astype(np.int64)
    ba, bb, qa, qb = cat(1, A), cat(1, B), cat(2, A), cat(2, B)
    lens = np.array([len(r[1]) for r in A], np.int64)
    read = np.repeat(np.arange(N, dtype=np.int64), lens)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1] if N else np.zeros(0, np.int64)
    pos = np.arange(len(ba), dtype=np.int64) - np.repeat(start, lens)
    bch, qch = ba != bb, qa != qb
    df = bch | qch
    d = qb - qa
    ad = np.abs(d)
    bins = np.minimum(pos, POS - 1)
    u64 = lambda x: np.asarray(x).astype(np.uint64)
    per_read = lambda m: int(np.count_nonzero(np.bincount(read[m], minlength=N))) if N else 0
    R = dict(n_reads=N, total_bases=int(len(ba)), n_diffs=int(df.sum()),
             reads_changed=per_read(df), reads_bases_changed=per_read(bch), reads_quals_changed=per_read(qch),
             bases_changed=int(bch.sum()), quals_changed=int(qch.sum()), quals_raised=int((d > 0).sum()), quals_lowered=int((d < 0).sum()),
             qual_abs_sum=int(ad.sum()), qual_sq_sum=int((ad * ad).sum()), qual_abs_max=int(ad.max()) if len(ad) else 0,
             first_changed_read=int(read[df][0]) if df.any() else NO_READ)
    same = sum(1 for x, y in zip(A, B) if x[0] == y[0])
    dropped = sum(1 for x, y in zip(A, B) if x[0] != y[0] and y[0] == b"@")
    R.update(headers_same=same, headers_dropped=dropped, headers_changed=N - same - dropped)
    R["subst"] = u64(np.bincount(SYMS * CLASS[ba] + CLASS[bb], minlength=SYMS * SYMS))
    R["qual_hist_a"] = u64(np.bincount(qa, minlength=256))
    R["qual_hist_b"] = u64(np.bincount(qb, minlength=256))
    R["changed_base_qual_hist"] = u64(np.bincount(qa[bch], minlength=256))
    R["pos_len"] = u64(np.bincount(bins, minlength=POS))
    R["pos_bases"] = u64(np.bincount(bins[bch], minlength=POS))
    R["pos_quals"] = u64(np.bincount(bins[qch], minlength=POS))
    R["pos_abs"] = u64(np.bincount(bins, weights=ad, minlength=POS).round())
    k = np.flatnonzero(df)[:max_diffs]
    diffs = np.zeros(len(k), DIFF_DTYPE)
    diffs["read"], diffs["pos"] = read[k], pos[k]
    diffs["base_a"], diffs["base_b"], diffs["qual_a"], diffs["qual_b"] = ba[k], bb[k], qa[k], qb[k]
    R["diffs"] = diffs
    return R
