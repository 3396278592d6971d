"""numpy / big-int restatement of the BFQPERM1 container and of the way back from a reordering (include/bfqzip_hip.h, "the way
back to the input order"), written from the header's words alone.  The CPU tests pin bfq_perm_encode / bfq_perm_decode to
encode() / decode(), the GPU tests pin the kernels' containers and texts to encode() / unreorder()."""
import struct
import numpy as np
from tests import reorder_model

MAGIC = b"BFQPERM1"
HDR = 40


def width(N):
    """Bits per entry: the bit length of N - 1, and 1 when N <= 2."""
    return 1 if N <= 2 else int(N - 1).bit_length()


def bound(N):
    return HDR + 8 * ((N * width(N) + 63) // 64)


def header(N, w, mode=0, k=0, seed=0):
    return MAGIC + struct.pack("<QIIIIQ", N, w, mode & 0xFFFFFFFF, k & 0xFFFFFFFF, 0, seed)


def encode(perm, N=None, opts=None):
    """perm[j] = input index of output record j -> the container's bytes.  Entry j in bits [j w, (j + 1) w) of the bit
    stream; bit b of the stream is bit b % 64 of (little-endian) word b / 64 -- i.e. bit b of the payload read as one
    little-endian integer."""
    perm = [int(x) for x in perm]
    N = len(perm) if N is None else N
    opts = opts or {}
    w = width(N)
    nbytes = 8 * ((N * w + 63) // 64)
    if N > 4096:                                                    # the same with numpy shifts: entry j -> its (at most two) words
        p = np.asarray(perm, np.uint64)
        bit = np.arange(N, dtype=np.uint64) * np.uint64(w)
        q, sh = (bit >> np.uint64(6)).astype(np.int64), bit & np.uint64(63)
        words = np.zeros(nbytes // 8 + 1, np.uint64)
        np.bitwise_or.at(words, q, p << sh)
        over = (sh + np.uint64(w)) > np.uint64(64)
        np.bitwise_or.at(words, q[over] + 1, p[over] >> (np.uint64(64) - sh[over]))
        payload = words[:nbytes // 8].astype("<u8").tobytes()
    else:
        big = 0
        for j, v in enumerate(perm):
            big |= v << (j * w)
        payload = big.to_bytes(nbytes, "little")
    return header(N, w, opts.get("mode", 0), opts.get("k", 0), opts.get("seed", 0)) + payload


def first_bad(perm, N):
    """The smallest j with perm[j] >= N or perm[j] met at an earlier position; None: a permutation of 0..N-1."""
    seen = set()
    for j, v in enumerate(perm):
        if v >= N or v in seen:
            return j
        seen.add(v)
    return None


def decode(z):
    """Container bytes -> (perm as a list, dict(mode, k, seed)).  Raises ValueError(first_bad) when the container is not well
    formed: first_bad None for the header (magic, w, total length, padding), else the first offending position."""
    z = bytes(z)
    if len(z) < HDR or z[:8] != MAGIC:
        raise ValueError(None)
    N, w, mode, k, _, seed = struct.unpack("<QIIIIQ", z[8:HDR])
    if N >= 1 << 56 or w != width(N) or len(z) != bound(N):
        raise ValueError(None)
    mask = (1 << w) - 1
    if N > 4096:                                                    # the same with numpy shifts
        words = np.concatenate([np.frombuffer(z[HDR:], "<u8").astype(np.uint64), np.zeros(1, np.uint64)])
        if N * w % 64 and int(words[-2]) >> (N * w % 64):
            raise ValueError(None)
        bit = np.arange(N, dtype=np.uint64) * np.uint64(w)
        q, sh = (bit >> np.uint64(6)).astype(np.int64), bit & np.uint64(63)
        over = (sh + np.uint64(w)) > np.uint64(64)
        v = words[q] >> sh
        v[over] |= words[q[over] + 1] << (np.uint64(64) - sh[over])
        perm = [int(x) for x in v & np.uint64(mask)]
    else:
        big = int.from_bytes(z[HDR:], "little")
        if big >> (N * w):
            raise ValueError(None)                                   # a padding bit is set
        perm = [(big >> (j * w)) & mask for j in range(N)]
    bad = first_bad(perm, N)
    if bad is not None:
        raise ValueError(bad)
    return perm, dict(mode=mode if mode < 1 << 31 else mode - (1 << 32), k=k if k < 1 << 31 else k - (1 << 32), seed=seed)


def unreorder(texts, perm):
    """texts: [text] or [mates 1, mates 2] in the order of a reordered run; perm[j] = input index of output record j of that
    run -> [text per file as bytes] with output record perm[j] = input record j, byte for byte (a missing final newline is
    added)."""
    perm = np.asarray(perm, np.int64)
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm), dtype=np.int64)
    out = []
    for t in texts:
        a, rs, rl, _, _ = reorder_model.records(t)
        if len(rs) != len(perm):
            raise ValueError("a permutation of %d reads for a text of %d records" % (len(perm), len(rs)))
        C = reorder_model.CHUNK
        parts = [a[reorder_model._seg(rs[inv[c0:c0 + C]], rl[inv[c0:c0 + C]])] for c0 in range(0, len(perm), C)]
        out.append(np.concatenate(parts).tobytes() if parts else b"")
    return out
