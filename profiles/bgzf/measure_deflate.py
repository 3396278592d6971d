"""Measurements behind the deflate section of profiles/bgzf/README.md (not a test): N x 150 synthetic reads as FASTQ text
(Engine.synth_fastq) and the smoothed output of that text (fastq_job, M=2 B=1), then
  (a) size: the BGZF bytes of the GPU writer beside zlib level 1, level 6 and Z_HUFFMAN_ONLY on the same 65 280-byte members,
      for the text and for its smoothed output;
  (b) time: bfq_bgzf_deflate_device from the text on the device, wall around the call and k_bgzf_deflate from the library's
      events, against zlib level 1 on at most 16 threads over the same members;
  (c) dropin/bfq_restore to plain text against bfq_restore -z, file to file on /dev/shm.
    python profiles/bgzf/measure_deflate.py [--reads 3000000] [--out result.json]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bfqzip_amd import api  # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
CHUNK = 65280


def zlib_size(text, pool, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """(BGZF bytes, seconds) of zlib over the members of `text` on the pool"""
    mv = memoryview(text)

    def work(at):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        return len(co.compress(mv[at:at + CHUNK])) + len(co.flush()) + 26
    t0 = time.perf_counter()
    n = sum(pool.map(work, range(0, len(text), CHUNK), chunksize=64)) + 28
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
    ap.add_argument("--tmp", default="/dev/shm")
    a = ap.parse_args()
    import torch
    say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)
    eng = api.Engine(0, M=2, B=1)
    spec = api.synth_spec(a.reads, 150)
    text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
    n = eng.synth_fastq(spec, text_pin.array)
    text = text_pin.array[:n]
    res = {"reads": a.reads, "text_bytes": n, "threads": THREADS, "members": (n + CHUNK - 1) // CHUNK}
    say("text", n)
    smooth = eng.fastq_job([text], keep_headers=True).fastq.copy()
    job = eng.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=True)   # the containers of (c)
    res["smoothed_bytes"] = len(smooth)
    say("smoothed", len(smooth), job.stats)
    # (a) sizes, and zlib level 1's time for (b)
    with ThreadPoolExecutor(THREADS) as pool:
        for tag, t in (("text", text), ("smoothed", smooth)):
            d = torch.from_numpy(np.ascontiguousarray(t)).cuda()
            blob = eng.bgzf_deflate_device(d.data_ptr(), len(t))
            if tag == "text":
                assert gzip.decompress(blob[:api.bgzf_index(blob)[0][3][0]].tobytes()) == t[:3 * CHUNK].tobytes()
                assert np.array_equal(eng.bgzf_inflate(blob), t)
            res[tag + "_gpu"] = len(blob)
            del d, blob
            z1, s1 = zlib_size(t, pool, 1)
            res[tag + "_zlib1"], res[tag + "_zlib6"] = z1, zlib_size(t, pool, 6)[0]
            res[tag + "_huffman_only"] = zlib_size(t, pool, 6, zlib.Z_HUFFMAN_ONLY)[0]
            if tag == "text":
                res["b_cpu_zlib1_s"] = min(s1, zlib_size(t, pool, 1)[1])
            say(tag, {k: v for k, v in res.items() if k.startswith(tag)})
    # (b) the device form: text on the device, BGZF bytes into host memory
    d = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    eng.bgzf_deflate_device(d.data_ptr(), n)                          # warm-up: arena, writers
    eng.prof_reset()
    wall, walls = best(lambda: eng.bgzf_deflate_device(d.data_ptr(), n))
    k = eng.prof()["k_bgzf_deflate"]
    res.update(b_wall_s=wall, b_walls=walls, b_wall_GBps=n / wall / 1e9, b_kernel_ms_per_call=k["ms"] / 3, b_kernel_launches=k["launches"],
               b_kernel_GBps=n / (k["ms"] / 3 / 1e3) / 1e9, b_cpu_zlib1_GBps=n / res["b_cpu_zlib1_s"] / 1e9)
    del d
    say(json.dumps(res))
    # (c) bfq_restore, file to file
    tmp = tempfile.mkdtemp(prefix="bfq_deflate_", dir=a.tmp)
    try:
        P = lambda name: os.path.join(tmp, name)
        for key in ("dna", "qs", "hdr"):
            with open(P(key), "wb") as f:
                f.write(getattr(job, key).tobytes())
        eng.close()
        cmd = [os.path.join(ROOT, "dropin", "bfq_restore"), "-d", P("dna"), "-q", P("qs"), "-H", P("hdr")]
        run = lambda extra, out: subprocess.run(cmd + extra + ["-o", P(out)], check=True, stdout=subprocess.DEVNULL)
        run([], "out.fq"); run(["-z"], "out.fq.gz")                  # warm-up: page cache, device start
        res["c_restore_plain_s"], res["c_restore_plain_all"] = best(lambda: run([], "out.fq"))
        res["c_restore_bgzf_s"], res["c_restore_bgzf_all"] = best(lambda: run(["-z"], "out.fq.gz"))
        res.update(c_plain_bytes=os.path.getsize(P("out.fq")), c_bgzf_bytes=os.path.getsize(P("out.fq.gz")))
        res["c_same_as_job"] = res["c_plain_bytes"] == len(smooth) and res["c_bgzf_bytes"] == res["smoothed_gpu"]
    finally:
        for name in os.listdir(tmp):
            os.unlink(os.path.join(tmp, name))
        os.rmdir(tmp)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
