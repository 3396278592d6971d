"""The texts the BGZF writer is tested on (host program, host form and GPU alike): the smallest that reach the member seam
(65 279 / 65 280 / 65 281 bytes), a member of one byte, the stored fallback (random bytes), length-258 chains at distance 1
(one byte repeated), code-length limiting (Fibonacci counts) and every literal."""
import random
from tests import bgzf_model as M

PIECE = 65280


def repeated(text, n):
    return (text * (n // len(text) + 1))[:n]


def fibonacci_text():
    """a seeded shuffle of 22 byte values with Fibonacci counts: 46 367 bytes whose Huffman tree is 21 levels deep"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    b = bytearray()
    for v, c in zip(range(40, 62), fib):
        b += bytes([v]) * c
    b = list(b)
    random.Random(5).shuffle(b)
    return bytes(b)


_TEXTS = None


def texts():
    """name -> text, made once"""
    global _TEXTS
    if _TEXTS is None:
        ex = M.golden_text("example.fastq")
        rng = random.Random(9)
        _TEXTS = {
            "empty": b"", "one-byte": b"A",
            "example-65279": repeated(ex, PIECE - 1), "example-65280": repeated(ex, PIECE), "example-65281": repeated(ex, PIECE + 1),
            "A-run": b"A" * (2 * PIECE + 5),
            "random-65280": bytes(rng.getrandbits(8) for _ in range(PIECE)),
            "all-256": repeated(bytes(range(256)), 70000),
            "fibonacci": fibonacci_text(),
            "example": ex, "synth_var": M.synth_var(),
        }
        assert len(_TEXTS["fibonacci"]) == 46367
    return _TEXTS


def members(n):
    return (n + PIECE - 1) // PIECE


def bound(n):
    return n + 31 * members(n) + 28
