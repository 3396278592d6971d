"""Measurements behind the unaligned BAM output's section of profiles/bam/README.md (not a test): N x 150 synthetic reads as
FASTQ text (Engine.synth_fastq, headers "@SYN.<n>"), then
  (u1) wall time around bfq_fastq_to_bam_device (text in a device buffer, the stream into a device buffer), best of 3 after a
       warm-up call, and the library's events of the two new passes (k_ubam_size, k_ubam_write) and of the line index;
  (u2) wall time around bfq_fastq_to_bam (text in pinned host memory, the compressed BAM into pinned host memory), its size;
  (f)  the floor of u2's compression: bfq_bgzf_deflate_device alone on the stream u1 left on the device;
  (h)  the one-thread host form (bfq_fastq_to_bam_host) on the same text;
the stream of u1 converted back (bfq_bam_to_fastq_device) and compared with the text it was made from.

    python profiles/bam/measure_ubam.py --reads 3000000 --out ubam_measure.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "bgzf"))
from bfqzip_amd import api  # noqa: E402
import measure as bgzf_measure  # noqa: E402  (profiles/bgzf/measure.py: best())

say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    eng = api.Engine(0, m=5)
    spec = api.synth_spec(a.reads, 150)
    text_pin = api.PinnedBuffer(a.reads * 330 + 4096)
    n = eng.synth_fastq(spec, text_pin.array)
    text = text_pin.array[:n]
    d_text = torch.from_numpy(text).cuda()
    raw, reads, st = eng.fastq_to_bam_measure([text])
    res = {"reads": reads[0], "text_bytes": n, "stream_bytes": raw, "stats": st.as_dict()}
    say("text", n, "stream", raw)
    d_raw = torch.empty(raw + 64, dtype=torch.uint8, device="cuda")
    call_dev = lambda: eng.fastq_to_bam_device([d_text.data_ptr(), 0, 0], [n, 0, 0], d_raw.data_ptr(), raw)
    _, st = call_dev()                                              # warm-up: arena
    back = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    eng.bam_to_fastq_device(d_raw[:raw].cpu().numpy(), [back.data_ptr(), 0, 0], [n, 0, 0])
    assert torch.equal(back[:n], d_text[:n])
    del back
    eng.prof_reset()
    wall, walls = bgzf_measure.best(call_dev)
    prof = {k: dict(v, ms=v["ms"] / 3, launches=v["launches"] / 3, alg_bytes=v["alg_bytes"] / 3) for k, v in eng.prof().items()}
    res["u1_device"] = dict(wall_s=wall, walls=walls, text_GBps=n / wall / 1e9, kernels=prof, stats=st.as_dict())
    say("device", wall, {k: round(v["ms"], 3) for k, v in prof.items()})
    out_pin = api.PinnedBuffer(api.bgzf_deflate_bound(raw))
    call_host = lambda: eng.fastq_to_bam([text], out=out_pin.array)
    z, _ = call_host()
    wall, walls = bgzf_measure.best(call_host)
    res["u2_host_to_host"] = dict(wall_s=wall, walls=walls, text_GBps=n / wall / 1e9, out_bytes=len(z))
    say("host to host", wall, len(z))
    call_dev()

    def deflate():
        ol = C.c_uint64(0)
        eng._ck(eng.L.bfq_bgzf_deflate_device(eng.h, C.c_void_p(d_raw.data_ptr()), raw, 1, out_pin.array.ctypes.data_as(C.c_void_p), len(out_pin.array), C.byref(ol)))
        return ol.value
    assert deflate() == len(z)
    wall, walls = bgzf_measure.best(deflate)
    res["f_deflate_device"] = dict(wall_s=wall, walls=walls, stream_GBps=raw / wall / 1e9)
    say("deflate alone", wall)
    if not a.no_host:
        h_out = np.empty(raw, np.uint8)
        t0 = time.perf_counter()
        got, hst = api.fastq_to_bam_host([text], out=h_out)
        res["h_host_1thread_s"] = time.perf_counter() - t0
        res["h_host_text_GBps"] = n / res["h_host_1thread_s"] / 1e9
        assert np.array_equal(got, d_raw[:raw].cpu().numpy()) and hst.as_dict() == st.as_dict()
        say("host form", res["h_host_1thread_s"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
