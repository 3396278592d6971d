"""The BFQNAME1 container (include/bfqzip_hip.h, bfqzip_amd/csrc/k_names.hip) as pure Python: the statement the kernels are
compared with, byte for byte.  The four members are made by the CPU statement of the general codec (oracle.orc.codec_encode),
which is what bfq_stream_compress is held to."""
import re
import struct
import numpy as np
from oracle import orc

R = 256
MAX_LINE = 65535
LIMIT = 10 ** 18
END, INC, DELTA, TEXT, SAME = 0, 2, 3, 4, 15
_TOK = re.compile(rb"[0-9]+|[^0-9]+", re.S)


def _bytes(data):
    return data.tobytes() if isinstance(data, np.ndarray) else bytes(data)


def tokens(line):
    return _TOK.findall(line)


def numeric(tok):
    return tok[:1].isdigit() and len(tok) <= 18 and (len(tok) == 1 or tok[:1] != b"0")


def leb(z):
    out = bytearray()
    while z >= 128:
        out.append((z & 127) | 128)
        z >>= 7
    out.append(z)
    return bytes(out)


def eligible(data):
    data = _bytes(data)
    return len(data) > 0 and data.endswith(b"\n") and max(len(x) for x in data[:-1].split(b"\n")) <= MAX_LINE


def encode_line(line, prev):
    """(ops, num, text) of one line against the tokens `prev` of the line before."""
    ops, num, text = bytearray(), bytearray(), bytearray()
    run = 0

    def flush():
        nonlocal run
        while run > 240:
            ops.append(SAME + 240)
            run -= 240
        if run:
            ops.append(SAME + run)
        run = 0
    for t, tok in enumerate(tokens(line)):
        p = prev[t] if t < len(prev) else None
        if p == tok:
            run += 1
            continue
        flush()
        if numeric(tok):
            d = int(tok) - (int(p) if p is not None and numeric(p) else 0)
            if d == 1:
                ops.append(INC)
            else:
                ops.append(DELTA)
                num += leb(2 * d if d >= 0 else -2 * d - 1)
        else:
            ops.append(TEXT)
            text += leb(len(tok)) + tok
    flush()
    ops.append(END)
    return bytes(ops), bytes(num), bytes(text)


def transform(data):
    """(index, ops, num, text) of an eligible stream."""
    data = _bytes(data)
    assert eligible(data)
    lines = data[:-1].split(b"\n")
    index, ops, num, text = bytearray(), bytearray(), bytearray(), bytearray()
    for g in range(0, len(lines), R):
        prev = []
        go, gn, gt, raw = bytearray(), bytearray(), bytearray(), 0
        for line in lines[g:g + R]:
            o, n, t = encode_line(line, prev)
            go += o; gn += n; gt += t
            raw += len(line) + 1
            prev = tokens(line)
        index += struct.pack("<4I", len(go), len(gn), len(gt), raw)
        ops += go; num += gn; text += gt
    return bytes(index), bytes(ops), bytes(num), bytes(text)


def build(members, raw_len, nlines, r=R, reserved=0, member_lens=None):
    """A container of hand-made streams: members = (index, ops, num, text) raw bytes, each coded by the general codec (so
    that the member checksums hold whatever the streams say)."""
    z = [orc.codec_encode(np.frombuffer(m, np.uint8)).tobytes() for m in members]
    lens = member_lens if member_lens is not None else [len(x) for x in z]
    return b"BFQNAME1" + struct.pack("<QIIQ4Q", raw_len, r, reserved, nlines, *lens) + b"".join(z)


def container(data):
    data = _bytes(data)
    return build(transform(data), len(data), data.count(b"\n"))


def general(data):
    """What bfq_stream_compress writes for these bytes."""
    return orc.codec_encode(np.frombuffer(_bytes(data), np.uint8)).tobytes()


def choose(data, always=False):
    """What bfq_names_compress gives: flags 0 keeps the shorter (BFQNAME1 only when strictly shorter); ineligible streams
    take the general container with either flag."""
    data = _bytes(data)
    if not eligible(data):
        return general(data)
    c = container(data)
    if always:
        return c
    g = general(data)
    return c if len(c) < len(g) else g


class Damaged(Exception):
    pass


def _leb_read(buf, pos, end):
    z = 0
    for k in range(9):
        if pos >= end:
            raise Damaged("share ends inside a LEB128")
        b = buf[pos]
        pos += 1
        z |= (b & 127) << (7 * k)
        if not b & 128:
            return z, pos
    raise Damaged("LEB128 of more than nine bytes")


def decode_group(ops, num, text, raw, want):
    """The `want` lines of one group from its shares; every share must be consumed exactly."""
    out = bytearray()
    po = pn = pt = 0
    prev = []
    for _ in range(want):
        line = bytearray()
        t = 0
        while True:
            if po >= len(ops):
                raise Damaged("ops share ends inside a line")
            op = ops[po]
            po += 1
            if op == END:
                break
            p = prev[t] if t < len(prev) else None
            if op > SAME:
                k = op - SAME
                if t + k > len(prev):
                    raise Damaged("SAME run past the previous line's tokens")
                line += b"".join(prev[t:t + k])
                t += k
                continue
            if op in (INC, DELTA):
                u = int(p) if p is not None and numeric(p) else 0
                if op == INC:
                    v = u + 1
                else:
                    z, pn = _leb_read(num, pn, len(num))
                    v = u + (z >> 1 if not z & 1 else -((z + 1) >> 1))
                if not 0 <= v < LIMIT:
                    raise Damaged("number outside 0 .. 10^18 - 1")
                line += b"%d" % v
            elif op == TEXT:
                n, pt = _leb_read(text, pt, len(text))
                if n == 0 or n > len(text) - pt:
                    raise Damaged("TEXT length")
                line += text[pt:pt + n]
                pt += n
            else:
                raise Damaged("byte %d is not an operation" % op)
            t += 1
        if len(line) > MAX_LINE:
            raise Damaged("line beyond 65535 bytes")
        out += line + b"\n"
        if len(out) > raw:
            raise Damaged("raw share overrun")
        prev = tokens(bytes(line))
    if po != len(ops) or pn != len(num) or pt != len(text) or len(out) != raw:
        raise Damaged("a share is not consumed exactly")
    return bytes(out)


def decode(blob):
    blob = _bytes(blob)
    if len(blob) < 64 or blob[:8] != b"BFQNAME1":
        raise Damaged("magic")
    raw_len, r, reserved, nl, *lens = struct.unpack("<QIIQ4Q", blob[8:64])
    if r != R or reserved or nl == 0 or nl > raw_len or 64 + sum(lens) != len(blob):
        raise Damaged("header")
    members, pos = [], 64
    for n in lens:
        members.append(orc.codec_decode(np.frombuffer(blob[pos:pos + n], np.uint8)).tobytes() if n else b"")
        pos += n
    index, ops, num, text = members
    ng = (nl + R - 1) // R
    if len(index) != 16 * ng:
        raise Damaged("index length")
    idx = struct.unpack("<%dI" % (4 * ng), index)
    if (sum(idx[0::4]), sum(idx[1::4]), sum(idx[2::4]), sum(idx[3::4])) != (len(ops), len(num), len(text), raw_len):
        raise Damaged("index columns")
    out = []
    po = pn = pt = 0
    for g in range(ng):
        o, n, t, raw = idx[4 * g:4 * g + 4]
        out.append(decode_group(ops[po:po + o], num[pn:pn + n], text[pt:pt + t], raw, min(R, nl - g * R)))
        po += o; pn += n; pt += t
    return b"".join(out)


# ---- the inputs of the tests
def sra_names(n, first=1):
    return b"".join(b"@SRR1770413.%d %d length=%d\n" % (i, i, 100 if i % 7 else 99 - i % 3) for i in range(first, first + n))


def illumina_names(n, seed=1):
    rng = np.random.default_rng(seed)
    out, tile, x, y = [], 1101, 1000, 2000
    for _ in range(n):
        x += int(rng.integers(1, 40))
        if x > 30000:
            x = 1000 + int(rng.integers(0, 50)); y += int(rng.integers(1, 200))
        if y > 200000:
            y = 2000; tile += 1
        out.append(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ATCACGTT\n" % (tile, x, y + int(rng.integers(0, 30))))
    return b"".join(out)


def syn_names(n):
    return b"".join(b"@SYN.%d\n" % i for i in range(n))


def random_lines(n, width, seed=2):
    rng = np.random.default_rng(seed)
    a = rng.integers(33, 127, (n, width + 1), dtype=np.uint8)
    a[:, -1] = 10
    return a.tobytes()


def random_stream(rng, nlines, max_tokens=12):
    """Lines over the alphabet `0123456789 :./@ab`: empty lines, 15- to 25-digit runs, lines that repeat or nearly repeat the
    one before, now and then a line of 600 tokens."""
    alpha = np.frombuffer(b"0123456789 :./@ab", np.uint8)
    out, prev = [], b""
    for _ in range(nlines):
        r = rng.random()
        if r < 0.08:
            line = b""
        elif r < 0.25 and prev:
            line = prev                                           # SAME runs
        elif r < 0.45 and prev:                                   # counters move, some text changes
            toks = tokens(prev)
            for k in range(len(toks)):
                if rng.random() < 0.4:
                    toks[k] = (b"%d" % (int(toks[k]) + int(rng.integers(-3, 4)) if numeric(toks[k]) and int(toks[k]) > 3 else int(rng.integers(0, 10 ** 6)))
                               if toks[k][:1].isdigit() else bytes(alpha[rng.integers(10, len(alpha), int(rng.integers(1, 4)))]))
            line = b"".join(toks)
        elif r < 0.47:
            line = b"".join(b"%d%s" % (int(rng.integers(0, 1000)), bytes(alpha[rng.integers(10, len(alpha), 1)])) for _ in range(300))   # 600 tokens
        else:
            parts = []
            for _ in range(int(rng.integers(1, max_tokens))):
                k = rng.random()
                if k < 0.15:
                    parts.append(bytes(alpha[rng.integers(0, 10, int(rng.integers(15, 26)))]))       # 15 .. 25 digits
                else:
                    parts.append(bytes(alpha[rng.integers(0, len(alpha), int(rng.integers(1, 9)))]))
            line = b"".join(parts)
        out.append(line)
        prev = line
    return b"".join(x + b"\n" for x in out)


def edge_cases():
    """name -> stream: what the kernels are held to with always = True (all eligible)."""
    rng = np.random.default_rng(20261018)
    c = {"sra_3000": sra_names(3000), "illumina_3000": illumina_names(3000), "syn_3000": syn_names(3000)}
    for n in (1, 255, 256, 257, 513):
        c["sra_%d" % n] = sra_names(n, first=95)
    c["empty_lines"] = b"\n" * 700
    c["one_empty_line"] = b"\n"
    c["same_600"] = b"a1" * 300 + b"\n" + b"a1" * 300 + b"\n" + b"a1" * 299 + b"a2\n"         # SAME runs of 240 + 240 + 120
    c["counters_down"] = b"".join(b"@r.%d x%d\n" % (5000 - 3 * i, 10 ** 17 - i * 10 ** 15) for i in range(600))
    c["zeros"] = b"0\n007\n0\n7\n123456789012345678\n1234567890123456789\n123456789012345679\n999999999999999999\n0\n00\n1000000000000000000\n1\n"
    c["numeric_vs_text"] = b"ab 12\n34 cd\nab 12\n007 5\n8 007\n9 8\n" * 50
    c["high_bytes"] = bytes(range(128, 256)) + b"\r\n" + b"x\xff9\r\n\r\n\x00\x01 7\r\n" * 3
    c["line_65535"] = b"@r1\n" + b"ab12" * 16383 + b"abc\n" + b"ab12" * 16383 + b"abd\n@r2\n"
    c["long_tokens"] = b"x" * 200 + b"\n" + b"x" * 20000 + b"7\n" + b"9" * 300 + b"\n"
    c["random"] = random_stream(rng, 1500)
    return c


def ineligible_cases():
    return {"line_65536": b"@r1\n" + b"a" * 65536 + b"\n@r2\n", "no_final_newline": b"@r1\n@r2", "empty": b""}


def refusal_cases():
    """name -> container that parses, whose member checksums hold, and that the decoder must refuse."""
    good = b"ab 12\nab 13\n"
    index, ops, num, text = transform(good)
    assert ops == bytes([TEXT, DELTA, END, SAME + 1, INC, END])
    ix = lambda o, n, t, raw: struct.pack("<4I", o, n, t, raw)
    c = {}
    o = bytes([TEXT, DELTA, END, SAME + 3, END])                                             # the line before has two tokens
    c["same_past_previous"] = build((ix(len(o), len(num), len(text), 12), o, num, text), 12, 2)
    c["raw_share_short"] = build((ix(len(ops), len(num), len(text), 11), ops, num, text), 11, 2)
    o = bytes([TEXT, DELTA, END, SAME + 1, 1, END])
    c["op_byte_1"] = build((ix(len(o), len(num), len(text), 12), o, num, text), 12, 2)
    o, n = bytes([TEXT, DELTA, END, SAME + 1, DELTA, END]), num + leb(2 * 13 - 1)           # 12 - 13
    c["delta_below_zero"] = build((ix(len(o), len(n), len(text), 12), o, n, text), 12, 2)
    t = leb(9) + b"ab "                                                                      # nine bytes promised, three there
    c["text_past_share"] = build((ix(len(ops), len(num), len(t), 12), ops, num, t), 12, 2)
    o = ops[:-1]
    c["one_end_too_few"] = build((ix(len(o), len(num), len(text), 12), o, num, text), 12, 2)
    z = [len(general(m)) for m in (index, ops, num, text)]
    c["member_lengths"] = build((index, ops, num, text), 12, 2, member_lens=[z[0], z[1], z[2], z[3] + 1])
    return good, c
