"""Measurements behind the tags section of profiles/bam/README.md (not a test): N x 150 synthetic reads (Engine.synth_fastq)
as the inflated stream of an unaligned BAM -- flag 4, and on every record RG:Z:grp1, RX:Z:<8 bases> and BC:Z:<8 bases>-<8
bases> (17 bytes), numpy-vectorised --, handed to the calls as it is (a source that begins with "BAM\\1" is uploaded, so no
inflate stands in front of the walks), then, five calls each after a warm-up call,
  (in)  wall time around bfq_bam_to_fastq_device with plain options and with every tag asked for;
  (out) wall time around bfq_fastq_to_bam_device on the tagged text of (in) with plain options and with tags on,
        and the per-kernel times of k_ubam_size / k_ubam_write from the library's events;
the tagged text checked against the stream's records (every header line carries its three fields) and the stream that comes
back compared with the one that went in.
--save DIR keeps the stream and the tagged text; --load DIR takes them from there (what a build without the tag options, such
as the parent commit's, measures its plain calls on: --plain-only).  --only in-off | in-on: that call alone, three times: what
a `rocprofv3 --kernel-trace --stats` run of its own wraps for k_bam_walk / k_bam_place.

    python profiles/bam/measure_tags.py --reads 3000000 --out bam_tags_measure.json"""
import argparse
import json
import os
import struct
import sys
import time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=3_000_000)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), help="the tree whose bfqzip_amd is measured")
ap.add_argument("--out", default="")
ap.add_argument("--save", default="")
ap.add_argument("--load", default="")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--only", default="")
ap.add_argument("--calls", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, a.root)
from bfqzip_amd import api  # noqa: E402

say = lambda *x: print("[measure_tags]", *x, file=sys.stderr, flush=True)


def tagged_stream(text, L, seed=7):
    """as profiles/bam/measure.py's ubam_stream, with the three tags behind the qualities"""
    nl = np.flatnonzero(text == 10)
    start = np.concatenate(([0], nl[:-1] + 1)).astype(np.int64)
    h, s, q = start[0::4], start[1::4], start[3::4]
    assert ((nl[1::4] - s) == L).all() and ((nl[3::4] - q) == L).all() and L % 2 == 0
    name_len = (nl[0::4] - h - 1).astype(np.int64)
    assert (np.diff(name_len) >= 0).all()
    nib = np.zeros(256, np.uint8)
    for i, ch in enumerate(b"=ACMGRSVTWYHKDBN"):
        nib[ch] = i
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    aux_len = 8 + (3 + 8 + 1) + (3 + 17 + 1)
    parts = [b"BAM\1" + struct.pack("<ii", 0, 0)]
    for m in np.unique(name_len):
        sel = np.flatnonzero(name_len == m)
        size = 36 + (m + 1) + L // 2 + L + aux_len
        rec = np.zeros((len(sel), size), np.uint8)
        rec[:, :36] = np.frombuffer(struct.pack("<IiiBBHHHIiii", size - 4, -1, -1, m + 1, 0, 4680, 0, 4, L, -1, -1, 0), np.uint8)
        rec[:, 36:36 + m] = text[h[sel, None] + 1 + np.arange(m)]
        at = 36 + m + 1
        codes = nib[text[s[sel, None] + np.arange(L)]]
        rec[:, at:at + L // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
        rec[:, at + L // 2:at + L // 2 + L] = text[q[sel, None] + np.arange(L)] - 33
        at += L // 2 + L
        rec[:, at:at + 8] = np.frombuffer(b"RGZgrp1\0", np.uint8)
        rec[:, at + 8:at + 11] = np.frombuffer(b"RXZ", np.uint8)
        rec[:, at + 11:at + 19] = acgt[rng.integers(0, 4, (len(sel), 8))]
        rec[:, at + 20:at + 23] = np.frombuffer(b"BCZ", np.uint8)
        rec[:, at + 23:at + 40] = acgt[rng.integers(0, 4, (len(sel), 17))]
        rec[:, at + 31] = ord("-")
        parts.append(rec.tobytes())
    return np.frombuffer(b"".join(parts), np.uint8), aux_len


def walls(call, n):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(best_ms=1e3 * min(out), all_ms=[round(1e3 * w, 2) for w in out], spread_ms=round(1e3 * (max(out) - min(out)), 2))


def main():
    import torch
    eng = api.Engine(0, m=5)
    if a.load:
        stream = np.fromfile(os.path.join(a.load, "stream.bin"), np.uint8)
        tagged = np.fromfile(os.path.join(a.load, "tagged.fq"), np.uint8)
        aux_len = 41
    else:
        text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
        n = eng.synth_fastq(api.synth_spec(a.reads, 150), text_pin.array)
        stream, aux_len = tagged_stream(text_pin.array[:n], 150)
        tagged = None
        del text_pin
    pin = api.PinnedBuffer(len(stream))
    pin.array[:] = stream
    on = {} if a.plain_only else dict(tags="*")
    lens, reads, st = eng.bam_measure(pin.array)
    res = dict(reads=reads[0], stream_bytes=len(stream), tag_bytes_of_stream=aux_len * reads[0], tag_share_of_stream=aux_len * reads[0] / len(stream),
               plain_text_bytes=lens[0])
    lens_on = eng.bam_measure(pin.array, **on)[0] if on else lens
    res["tagged_text_bytes"] = lens_on[0]
    d_out = torch.empty(max(lens_on[0], len(tagged) if tagged is not None else 0) + 64, dtype=torch.uint8, device="cuda")
    outs = [d_out.data_ptr(), 0, 0]
    in_off = lambda: eng.bam_to_fastq_device(pin.array, outs, [lens[0], 0, 0])
    in_on = lambda: eng.bam_to_fastq_device(pin.array, outs, [lens_on[0], 0, 0], **on)
    if a.only:
        for _ in range(3):
            {"in-off": in_off, "in-on": in_on}[a.only]()
        return
    in_off()
    res["in_off"] = walls(in_off, a.calls)
    say("in_off", res["in_off"])
    if on:
        _, _, st = in_on()
        res["in_on"] = dict(walls(in_on, a.calls), tags=st.tags.as_dict())
        say("in_on", res["in_on"])
        tagged = d_out[:lens_on[0]].cpu().numpy()
        head = bytes(tagged[:200]).split(b"\n")[0]
        assert head.count(b"\t") == 3 and b"\tRG:Z:grp1\tRX:Z:" in head and b"\tBC:Z:" in head, head
        assert st.tags.tags_written == 3 * reads[0] and st.tags.tag_bytes == lens_on[0] - lens[0]
        if a.save:
            os.makedirs(a.save, exist_ok=True)
            stream.tofile(os.path.join(a.save, "stream.bin"))
            tagged.tofile(os.path.join(a.save, "tagged.fq"))
    # the way out, on the tagged text
    nt = len(tagged)
    d_text = torch.from_numpy(np.ascontiguousarray(tagged)).cuda()
    raw_off = eng.fastq_to_bam_measure([tagged], header_text=b"")[0]
    raw_on = eng.fastq_to_bam_measure([tagged], header_text=b"", **on)[0] if on else raw_off
    d_raw = torch.empty(max(raw_on, raw_off) + 64, dtype=torch.uint8, device="cuda")
    out_off = lambda: eng.fastq_to_bam_device([d_text.data_ptr(), 0, 0], [nt, 0, 0], d_raw.data_ptr(), raw_off, header_text=b"")
    out_on = lambda: eng.fastq_to_bam_device([d_text.data_ptr(), 0, 0], [nt, 0, 0], d_raw.data_ptr(), raw_on, header_text=b"", **on)

    def kernels(call):
        eng.prof_reset()
        w = walls(call, a.calls)
        p = eng.prof()
        return dict(w, kernels_ms={k: round(v["ms"] / a.calls, 3) for k, v in p.items() if k.startswith("k_ubam") or "line" in k or "nl" in k})

    out_off()
    res["out_off"] = kernels(out_off)
    say("out_off", res["out_off"])
    if on:
        _, ust = out_on()
        assert raw_on == len(stream) and np.array_equal(d_raw[:raw_on].cpu().numpy(), stream)      # the stream that went in
        res["out_on"] = dict(kernels(out_on), tags=ust.tags.as_dict())
        say("out_on", res["out_on"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
