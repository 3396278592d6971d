"""Measurements behind profiles/bam/README.md (not a test): N x 150 synthetic reads (Engine.synth_fastq) written as an
unaligned BAM file -- flag 4, an RG tag, numpy-vectorised -- wrapped as BGZF at zlib level 6, then
  (a) wall time around bfq_bam_to_fastq_device (text into a device buffer) at several piece sizes, best of 3 after a warm-up,
      the text compared with the FASTQ it was made from;
  (b) the floor: bfq_bgzf_inflate_device alone on the same file in the same build (the conversion contains it);
  (c) the one-thread host form (bfq_bam_to_fastq_host) on the inflated stream.
--save BLOB keeps the BAM bytes; --load BLOB --only-bam PIECE runs (a) alone at one piece size from them, three calls: what a
`rocprofv3 --kernel-trace --stats` run of its own wraps for the per-kernel split.
--patch measures the way back instead (bfq_bam_patch*): the file's own text with a seeded 2 % of the bases and 10 % of the
qualities changed goes back into the file,
  (p1) wall time around bfq_bam_patch_device (text in a device buffer, the patched stream into a device buffer);
  (p2) wall time around bfq_bam_patch (text in pinned host memory, the compressed BAM into pinned host memory), its size;
  (f1) the floor of p1: bfq_bgzf_inflate_device alone;  (f2) the floor of p2: that plus bfq_bgzf_deflate_device of the stream;
the result of p1 converted again and compared with the text it was given.  --only-patch: p1 alone, three calls, for rocprofv3.

    python profiles/bam/measure.py --reads 3000000 --out bam_measure.json"""
import argparse
import json
import os
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "bgzf"))
from bfqzip_amd import api  # noqa: E402
import measure as bgzf_measure  # noqa: E402  (profiles/bgzf/measure.py: the BGZF writer over zlib)

say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)
RG = b"RGZgrp1\0"


def ubam_stream(text, L):
    """The inflated stream of an unaligned BAM file with the reads of a FASTQ text whose sequences all have L bases (L
    even).  Reads with names of one length have records of one size: one 2-D array per name length, filled column-wise."""
    nl = np.flatnonzero(text == 10)
    assert len(nl) % 4 == 0 and L % 2 == 0
    start = np.concatenate(([0], nl[:-1] + 1)).astype(np.int64)     # where every line begins
    h, s, q = start[0::4], start[1::4], start[3::4]
    assert ((nl[1::4] - s) == L).all() and ((nl[3::4] - q) == L).all()
    name_len = (nl[0::4] - h - 1).astype(np.int64)                   # without '@'
    assert (np.diff(name_len) >= 0).all()                            # "SYN.<n>": groups of one length are runs of the file
    nib = np.zeros(256, np.uint8)
    for i, ch in enumerate(b"=ACMGRSVTWYHKDBN"):
        nib[ch] = i
    parts = [b"BAM\1" + struct.pack("<ii", 0, 0)]
    for m in np.unique(name_len):
        sel = np.flatnonzero(name_len == m)
        size = 36 + (m + 1) + L // 2 + L + len(RG)
        rec = np.zeros((len(sel), size), np.uint8)
        fixed = struct.pack("<IiiBBHHHIiii", size - 4, -1, -1, m + 1, 0, 4680, 0, 4, L, -1, -1, 0)
        rec[:, :36] = np.frombuffer(fixed, np.uint8)
        rec[:, 36:36 + m] = text[h[sel, None] + 1 + np.arange(m)]
        at = 36 + m + 1
        codes = nib[text[s[sel, None] + np.arange(L)]]
        rec[:, at:at + L // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
        rec[:, at + L // 2:at + L // 2 + L] = text[q[sel, None] + np.arange(L)] - 33
        rec[:, at + L // 2 + L:] = np.frombuffer(RG, np.uint8)
        parts.append(rec.tobytes())
        say("records with names of", int(m), "bytes:", len(sel))
    return b"".join(parts)


def measure_patch(a, eng, pin, d_text, n, res):
    """the way back: see the module's text"""
    import torch
    eng.bam_to_fastq_device(pin.array, [d_text.data_ptr(), 0, 0], [n, 0, 0])
    g = torch.Generator(device="cuda").manual_seed(1)
    t = d_text[:n]
    nl = torch.nonzero(t == 10).flatten()
    line = torch.zeros(n, dtype=torch.int32, device="cuda")
    line[nl[:-1] + 1] = 1
    line = torch.cumsum(line, 0) % 4                                # which line of its record a byte is in
    r = torch.rand(n, generator=g, device="cuda")
    base = (line == 1) & (t != 10) & (r < 0.02)
    qual = (line == 3) & (t != 10) & (r < 0.10)
    t[base] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (int(base.sum()),), generator=g, device="cuda")]
    t[qual] = torch.randint(35, 74, (int(qual.sum()),), generator=g, device="cuda").to(torch.uint8)
    del line, r, base, qual, nl
    raw = api.text_len(pin.array) - 1
    d_raw = torch.empty(raw + 64, dtype=torch.uint8, device="cuda")
    call_dev = lambda: eng.bam_patch_device(pin.array, [d_text.data_ptr(), 0, 0], [n, 0, 0], d_raw.data_ptr(), raw)
    if a.only_patch:
        for _ in range(3):
            call_dev()
        return
    _, st = call_dev()                                              # warm-up: arena, staging buffers
    back = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    eng.bam_to_fastq_device(d_raw[:raw].cpu().numpy(), [back.data_ptr(), 0, 0], [n, 0, 0])
    assert torch.equal(back[:n], d_text[:n])
    del back
    eng.prof_reset()
    wall, walls = bgzf_measure.best(call_dev)
    k = eng.prof()["k_bgzf_inflate"]
    res["stream_bytes"] = raw
    res["p1_patch_device"] = dict(wall_s=wall, walls=walls, stream_GBps=raw / wall / 1e9, kernels_ms=k["ms"] / 3, launches=k["launches"] / 3, stats=st.as_dict())
    say("patch_device", wall, k["ms"] / 3, st)
    text_pin = api.PinnedBuffer(n)
    text_pin.array[:] = d_text[:n].cpu().numpy()
    out_pin = api.PinnedBuffer(api.bgzf_deflate_bound(raw))
    call_host = lambda: eng.bam_patch(pin.array, [text_pin.array[:n]], out=out_pin.array)
    z, _ = call_host()
    wall, walls = bgzf_measure.best(call_host)
    res["p2_patch"] = dict(wall_s=wall, walls=walls, stream_GBps=raw / wall / 1e9, out_bytes=len(z), in_bytes=len(pin.array))
    say("patch", wall, len(z), len(pin.array))
    inflate = lambda: eng.bgzf_inflate_device(pin.array, d_raw.data_ptr(), raw)
    inflate()
    wall, walls = bgzf_measure.best(inflate)
    res["f1_inflate_device"] = dict(wall_s=wall, walls=walls)
    import ctypes as C

    def deflate():                                                  # (into the pinned buffer, as p2 writes: Engine.bgzf_deflate_device allocates its own)
        ol = C.c_uint64(0)
        eng._ck(eng.L.bfq_bgzf_deflate_device(eng.h, C.c_void_p(d_raw.data_ptr()), raw, 1, out_pin.array.ctypes.data_as(C.c_void_p), len(out_pin.array), C.byref(ol)))
    both = lambda: (inflate(), deflate())
    both()
    wall, walls = bgzf_measure.best(both)
    res["f2_inflate_deflate_device"] = dict(wall_s=wall, walls=walls)
    say("floors", res["f1_inflate_device"]["wall_s"], wall)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--pieces", default="32768,65536,131072")
    ap.add_argument("--out", default="")
    ap.add_argument("--save", default="")
    ap.add_argument("--load", default="")
    ap.add_argument("--only-bam", type=int, default=-1)
    ap.add_argument("--patch", action="store_true")
    ap.add_argument("--only-patch", action="store_true")
    a = ap.parse_args()
    import torch
    eng = api.Engine(0, m=5)
    text = stream = None
    if a.load:
        blob = open(a.load, "rb").read()
    else:
        spec = api.synth_spec(a.reads, 150)
        text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
        n = eng.synth_fastq(spec, text_pin.array)
        text = text_pin.array[:n]
        t0 = time.perf_counter()
        stream = ubam_stream(text, 150)
        say("stream", len(stream), time.perf_counter() - t0)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(bgzf_measure.THREADS) as pool:
            blob = bgzf_measure.write_bgzf(np.frombuffer(stream, np.uint8), pool)
        say("bam written", time.perf_counter() - t0, len(blob))
        if a.save:
            with open(a.save, "wb") as f:
                f.write(blob)
    pin = api.PinnedBuffer(len(blob))
    pin.array[:] = np.frombuffer(blob, np.uint8)
    lens, reads, st = eng.bam_measure(pin.array)
    n = lens[0]
    res = {"reads": reads[0], "text_bytes": n, "bam_bytes": len(blob), "stats": st.as_dict()}
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    outs, caps = [d_out.data_ptr(), 0, 0], [n, 0, 0]
    if a.only_bam >= 0:
        for _ in range(3):
            eng.bam_to_fastq_device(pin.array, outs, caps, piece=a.only_bam)
        return
    if a.patch or a.only_patch:
        return measure_patch(a, eng, pin, d_out, n, res)
    # (a) the conversion
    res["a"] = {}
    for piece in [int(c) for c in a.pieces.split(",")]:
        _, _, st = eng.bam_to_fastq_device(pin.array, outs, caps, piece=piece)                  # warm-up: arena, staging buffers
        if text is not None:
            assert np.array_equal(d_out[:n].cpu().numpy(), text)
        eng.prof_reset()
        wall, walls = bgzf_measure.best(lambda: eng.bam_to_fastq_device(pin.array, outs, caps, piece=piece))
        k = eng.prof()["k_bgzf_inflate"]
        res["a"][str(piece)] = dict(wall_s=wall, walls=walls, text_GBps=n / wall / 1e9, kernels_ms=k["ms"] / 3, launches=k["launches"] / 3, stats=st.as_dict())
        say("bam", piece, wall, k["ms"] / 3, st)
    # (b) the inflate alone
    raw = len(stream) if stream is not None else api.text_len(pin.array) - 1
    d_raw = torch.empty(raw + 64, dtype=torch.uint8, device="cuda")
    eng.bgzf_inflate_device(pin.array, d_raw.data_ptr(), raw)
    eng.prof_reset()
    wall, walls = bgzf_measure.best(lambda: eng.bgzf_inflate_device(pin.array, d_raw.data_ptr(), raw))
    k = eng.prof()["k_bgzf_inflate"]
    res["stream_bytes"] = raw
    res["b_bgzf_inflate"] = dict(wall_s=wall, walls=walls, stream_GBps=raw / wall / 1e9, kernel_ms=k["ms"] / k["launches"])
    say("bgzf", wall)
    # (c) the host form, one thread, on the inflated stream
    h_stream = d_raw[:raw].cpu().numpy()
    h_outs = [np.empty(n, np.uint8), np.empty(0, np.uint8), np.empty(0, np.uint8)]
    t0 = time.perf_counter()
    got, _ = api.bam_to_fastq_host(h_stream, outs=h_outs)
    res["c_host_1thread_s"] = time.perf_counter() - t0
    res["c_host_text_GBps"] = n / res["c_host_1thread_s"] / 1e9
    if text is not None:
        assert np.array_equal(got[0], text)
    say("host", res["c_host_1thread_s"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
