"""Measurements behind profiles/bgzf/README.md (not a test): N x 150 synthetic reads as FASTQ text (Engine.synth_fastq),
written as BGZF at level 6 by at most 16 threads, then
  (a) bfq_bgzf_inflate_device: GB/s of text out, wall and kernel time (Engine.prof);
  (b) the job host to host (pinned FASTQ bytes in, pinned streams out), once from the BGZF bytes and once from the text;
  (c) the CPU alternative: zlib inflating the members on 16 threads.
    python profiles/bgzf/measure.py [--reads 3000000] [--out result.json]
"""
import argparse
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bfqzip_amd import api  # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
CHUNK = 65280


def member(piece):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    pay = co.compress(piece) + co.flush()
    total = 18 + len(pay) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + pay +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def write_bgzf(text, pool):
    mv = memoryview(text)
    parts = list(pool.map(lambda at: member(mv[at:at + CHUNK]), range(0, len(text), CHUNK)))
    parts.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(parts)


def cpu_inflate(blob, members, pool):
    def work(rng):
        n = 0
        for in_off, _, in_len, _ in members[rng[0]:rng[1]]:
            n += len(zlib.decompressobj(-15).decompress(blob[in_off + 18:in_off + in_len - 8]))
        return n
    step = (len(members) + THREADS - 1) // THREADS
    t0 = time.perf_counter()
    n = sum(pool.map(work, [(i, min(i + step, len(members))) for i in range(0, len(members), step)]))
    return n, time.perf_counter() - t0


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    eng = api.Engine(0, m=5)
    spec = api.synth_spec(a.reads, 150)
    text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
    n = eng.synth_fastq(spec, text_pin.array)
    text = text_pin.array[:n]
    res = {"reads": a.reads, "text_bytes": n, "threads": THREADS}
    say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)
    say("text", n)
    with ThreadPoolExecutor(THREADS) as pool:
        t0 = time.perf_counter()
        blob_b = write_bgzf(text, pool)
        res["bgzf_write_s"] = time.perf_counter() - t0
        blob_pin = api.PinnedBuffer(len(blob_b))
        blob_pin.array[:] = np.frombuffer(blob_b, np.uint8)
        blob = blob_pin.array
        members, raw = api.bgzf_index(blob)
        assert raw == n
        res.update(bgzf_bytes=len(blob), members=len(members), ratio=n / len(blob))
        # (c) zlib on the CPU
        got, _ = cpu_inflate(blob_b, members, pool)
        assert got == n
        res["c_cpu_zlib_s"] = min(cpu_inflate(blob_b, members, pool)[1] for _ in range(2))
        res["c_cpu_zlib_GBps"] = n / res["c_cpu_zlib_s"] / 1e9
        say("written", res["bgzf_write_s"], "cpu", res["c_cpu_zlib_GBps"])
    del blob_b
    # (a) inflate into device memory
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    eng.bgzf_inflate_device(blob, d_out.data_ptr(), n)            # warm-up: arena, staging buffers
    assert np.array_equal(d_out[:n].cpu().numpy(), text)
    eng.prof_reset()
    wall, walls = best(lambda: eng.bgzf_inflate_device(blob, d_out.data_ptr(), n))
    k = eng.prof()["k_bgzf_inflate"]
    res.update(a_wall_s=wall, a_walls=walls, a_wall_GBps=n / wall / 1e9, a_kernel_ms=k["ms"] / k["launches"],
               a_kernel_GBps=n / (k["ms"] / k["launches"] / 1e3) / 1e9)
    del d_out
    say("a", res["a_wall_GBps"], res["a_kernel_GBps"])
    say(json.dumps(res))
    # (b) the job, host to host
    pins = {key: api.PinnedBuffer(n + 4096) for key in ("dna", "qs", "hdr")}     # (kept: a PinnedBuffer frees its memory when it goes)
    outs = {key: b.array for key, b in pins.items()}
    job = lambda part: eng.fastq_job([part], fastq=False, streams=True, hdr=True, out=outs)
    r_text = job(text)
    dna = r_text.dna.copy()
    r_bgzf = job(blob)
    assert np.array_equal(r_bgzf.dna, dna) and r_bgzf.n_reads == a.reads
    res["b_job_text_s"], res["b_job_text_all"] = best(lambda: job(text))
    res["b_job_bgzf_s"], res["b_job_bgzf_all"] = best(lambda: job(blob))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
