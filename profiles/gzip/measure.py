"""Measurements behind profiles/gzip/README.md (not a test): N x 150 synthetic reads as FASTQ text (Engine.synth_fastq),
written by zlib at level 6 with the default memLevel as ONE gzip member, then
  (a) wall time around bfq_gzip_inflate_device (text into device memory) at several piece sizes, best of 3 after a warm-up,
      with the statistics of the chain;
  (b) what a user has today: zlib.decompress of the same bytes on one thread;
  (c) the ceiling: bfq_bgzf_inflate_device on the same text as BGZF level 6 (the same bytes decoded once, no second pass).
--save BLOB keeps the gzip bytes; --load BLOB --only-gzip CHUNK runs (a) alone at one piece size from them, three calls: what a
`rocprofv3 --kernel-trace --stats` run of its own wraps for the per-kernel split.

    python profiles/gzip/measure.py --reads 3000000 --out gzip_measure.json"""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "bgzf"))
from bfqzip_amd import api  # noqa: E402
import measure as bgzf_measure  # noqa: E402  (profiles/bgzf/measure.py: the BGZF writer over zlib)

say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)


def gzip_one_member(text):
    """zlib level 6, default memLevel, one member; fed in slices so that progress shows"""
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out, step = [], 64 << 20
    for at in range(0, len(text), step):
        out.append(co.compress(text[at:at + step].tobytes()))
        say("deflated", min(at + step, len(text)))
    out.append(co.flush())
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--chunks", default="65536,131072,262144")
    ap.add_argument("--out", default="")
    ap.add_argument("--save", default="")
    ap.add_argument("--load", default="")
    ap.add_argument("--only-gzip", type=int, default=-1)
    a = ap.parse_args()
    import torch
    eng = api.Engine(0, m=5)
    if a.load:
        blob_g = open(a.load, "rb").read()
        n = eng.gzip_measure(blob_g)[0]
        text = None
    else:
        spec = api.synth_spec(a.reads, 150)
        text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
        n = eng.synth_fastq(spec, text_pin.array)
        text = text_pin.array[:n]
        say("text", n)
        t0 = time.perf_counter()
        blob_g = gzip_one_member(text)
        say("gzip written", time.perf_counter() - t0, len(blob_g))
        if a.save:
            with open(a.save, "wb") as f:
                f.write(blob_g)
    res = {"reads": a.reads, "text_bytes": n, "gzip_bytes": len(blob_g)}
    pin = api.PinnedBuffer(len(blob_g))
    pin.array[:] = np.frombuffer(blob_g, np.uint8)
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    if a.only_gzip >= 0:
        for _ in range(3):
            eng.gzip_inflate_device(pin.array, d_out.data_ptr(), n, chunk=a.only_gzip)
        return
    # (b) one zlib thread
    t0 = time.perf_counter()
    got = zlib.decompress(blob_g, 31)
    res["b_zlib_1thread_s"] = time.perf_counter() - t0
    assert len(got) == n
    t0 = time.perf_counter()
    zlib.decompress(blob_g, 31)
    res["b_zlib_1thread_s"] = min(res["b_zlib_1thread_s"], time.perf_counter() - t0)
    res["b_zlib_1thread_GBps"] = n / res["b_zlib_1thread_s"] / 1e9
    say("zlib", res["b_zlib_1thread_s"])
    # (a) the side-by-side inflate
    res["a"] = {}
    for chunk in [int(c) for c in a.chunks.split(",")]:
        _, st = eng.gzip_inflate_device(pin.array, d_out.data_ptr(), n, chunk=chunk)          # warm-up: arena, staging buffers
        if text is not None:
            assert np.array_equal(d_out[:n].cpu().numpy(), text)
        eng.prof_reset()
        wall, walls = bgzf_measure.best(lambda: eng.gzip_inflate_device(pin.array, d_out.data_ptr(), n, chunk=chunk))
        k = eng.prof()["k_bgzf_inflate"]
        res["a"][str(chunk)] = dict(wall_s=wall, walls=walls, wall_GBps=n / wall / 1e9, kernels_ms=k["ms"] / 3, launches=k["launches"] / 3, stats=st.as_dict())
        say("gzip", chunk, wall, k["ms"] / 3, st)
    # (c) the same text as BGZF
    if text is not None:
        with ThreadPoolExecutor(bgzf_measure.THREADS) as pool:
            blob_b = bgzf_measure.write_bgzf(text, pool)
        pin_b = api.PinnedBuffer(len(blob_b))
        pin_b.array[:] = np.frombuffer(blob_b, np.uint8)
        eng.bgzf_inflate_device(pin_b.array, d_out.data_ptr(), n)
        eng.prof_reset()
        wall, walls = bgzf_measure.best(lambda: eng.bgzf_inflate_device(pin_b.array, d_out.data_ptr(), n))
        k = eng.prof()["k_bgzf_inflate"]
        res["c_bgzf"] = dict(bytes=len(blob_b), wall_s=wall, walls=walls, wall_GBps=n / wall / 1e9, kernel_ms=k["ms"] / k["launches"])
        say("bgzf", wall)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
