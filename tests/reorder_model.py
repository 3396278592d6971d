"""numpy restatement of the read reordering (include/bfqzip_hip.h, bfq_fastq_reorder): the key, the order and the record
permutation, written from the interface's words alone.  The CPU tests pin bfq_reorder_key to key_of(), the GPU tests pin the
kernels' output text and permutation to reorder()."""
import numpy as np

NOKEY = (1 << 40) - 1
CHUNK = 100_000                                         # reads per slice of the vectorised passes (bounds the memory)


def fmix64(x):
    """MurmurHash3's 64-bit finaliser on a uint64 array (products wrap)."""
    x = np.array(x, np.uint64)
    x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def key_of(seq, k=21):
    """Mode-2 key of one sequence line, window by window."""
    best = None
    for p in range(len(seq) - k + 1):
        w = seq[p:p + k]
        if all(c in b"ACGT" for c in w):
            x = 0
            for c in w:
                x = (x << 2) | b"ACGT".index(c)
            h = int(fmix64([x])[0])
            best = h if best is None else min(best, h)
    return NOKEY if best is None else best >> 24


def _seg(starts, lens):
    ex = np.cumsum(lens) - lens
    return np.repeat(starts - ex, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def records(text):
    """(buffer with its final newline, record starts, record sizes, sequence starts, sequence lengths without CR)."""
    a = np.frombuffer(bytes(text), np.uint8)
    if len(a) and a[-1] != 10:
        a = np.append(a, np.uint8(10))
    end = np.flatnonzero(a == 10).astype(np.int64)
    if len(end) % 4:
        raise ValueError("FASTQ: number of lines is not a multiple of 4")
    start = np.concatenate([[0], end[:-1] + 1]).astype(np.int64)[:len(end)]
    s, e = start[1::4], end[1::4].copy()
    e -= (e > s) & (a[np.maximum(e - 1, 0)] == 13)
    return a, start[0::4], end[3::4] + 1 - start[0::4], s, e - s


def locus_keys(a, s, L, k=21):
    """Mode-2 keys of all reads (vectorised key_of) and which reads have a valid window."""
    lut = np.full(256, 4, np.uint8)
    lut[list(b"ACGT")] = [0, 1, 2, 3]
    keys = np.full(len(s), NOKEY, np.uint64)
    found = np.zeros(len(s), bool)
    for c0 in range(0, len(s), CHUNK):
        ss, LL = s[c0:c0 + CHUNK], L[c0:c0 + CHUNK]
        code = np.concatenate([lut[a[_seg(ss, LL)]], np.full(k, 4, np.uint8)])
        n = len(code) - k
        first = np.cumsum(LL) - LL
        left = np.repeat(first + LL, LL) - np.arange(n)             # bases from here to the end of the read
        bad = np.concatenate([[0], np.cumsum(code > 3)])
        ok = (bad[k:k + n] == bad[:n]) & (left >= k)
        x = np.zeros(n, np.uint64)
        for j in range(k):
            x = (x << np.uint64(2)) | (code[j:j + n] & 3).astype(np.uint64)
        h = np.where(ok, fmix64(x), np.uint64(0xFFFFFFFFFFFFFFFF))
        have = LL > 0                                               # (reduceat wants non-empty segments)
        mn = np.minimum.reduceat(h, first[have]) if have.any() else np.zeros(0, np.uint64)
        anyok = np.logical_or.reduceat(ok, first[have]) if have.any() else np.zeros(0, bool)
        kk = np.full(len(LL), NOKEY, np.uint64)
        kk[np.flatnonzero(have)[anyok]] = mn[anyok] >> np.uint64(24)
        keys[c0:c0 + CHUNK] = kk
        found[c0 + np.flatnonzero(have)[anyok]] = True
    return keys, found


def reorder(texts, mode=2, k=21, seed=0):
    """texts: [text] or [mates 1, mates 2] -> ([reordered text per file as bytes], perm)."""
    recs = [records(t) for t in texts]
    N = len(recs[0][1])
    if any(len(r[1]) != N for r in recs):
        raise ValueError("mates differ in record count")
    if mode == 1:
        keys = fmix64(np.uint64(seed) + np.arange(N, dtype=np.uint64)) >> np.uint64(24)
    else:
        keys, found = locus_keys(recs[0][0], recs[0][3], recs[0][4], k)
        if len(recs) > 1:
            none = np.flatnonzero(~found)                        # mate 1 has no valid window: mate 2's key
            keys[none] = locus_keys(recs[1][0], recs[1][3][none], recs[1][4][none], k)[0]
    perm = np.argsort(keys, kind="stable")
    out = []
    for a, rs, rl, _, _ in recs:
        parts = [a[_seg(rs[perm[c0:c0 + CHUNK]], rl[perm[c0:c0 + CHUNK]])] for c0 in range(0, N, CHUNK)]
        out.append(np.concatenate(parts).tobytes() if parts else b"")
    return out, perm.astype(np.uint64)
