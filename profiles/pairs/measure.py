"""Measurements behind profiles/pairs/README.md (not a test): N / 2 x 150 synthetic reads as FASTQ text
(Engine.synth_fastq, headers "@SYN.<n>"), merged with themselves on the device into an interleaved text of N records whose
mates carry equal names, then, every call 5 times after a warm-up (the minimum and all five are kept: the spread):
  (s1) bfq_fastq_deinterleave, the text in pinned host memory, the two mates into pinned host memory, with the name check;
  (s2) bfq_fastq_deinterleave_device, device to device, strict mode with and without the name check, and orphan mode;
  (m1) bfq_fastq_interleave, pinned host to pinned host; (m2) bfq_fastq_interleave_device;
  (k)  the library's events per kernel of one s2 / orphan / m2 call;
  (y1) the first yardstick: bfq_fastq_reorder mode 1 on the same text, pinned host to pinned host (the same input buffer, an
       output buffer of the text's size), alternating with s1;
  (y2) the second: a device-to-device copy of the same bytes (the floor of the move kernel), timed with events.
The outputs of the split are compared with the text they were merged from.

    python profiles/pairs/measure.py --reads 3000000 --out pairs_measure.json"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bfqzip_amd import api  # noqa: E402

say = lambda *x: print("[measure]", *x, file=sys.stderr, flush=True)
REPS = 5


def timed(f, sync):
    t0 = time.perf_counter()
    f()
    sync()
    return time.perf_counter() - t0


def best(f, sync, reps=REPS):
    ts = [timed(f, sync) for _ in range(reps)]
    return dict(wall_s=min(ts), walls=ts)


def kernels(eng, f):
    eng.prof_reset()
    f()
    return {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000, help="records of the interleaved text")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    sync = torch.cuda.synchronize
    eng = api.Engine(0, m=5)
    half = a.reads // 2
    mate_pin = api.PinnedBuffer(half * 330 + 4096)
    n1 = eng.synth_fastq(api.synth_spec(half, 150), mate_pin.array)
    mate = mate_pin.array[:n1]
    d_mate = torch.from_numpy(mate).cuda()
    n = 2 * n1
    d_il = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    merge_dev = lambda: eng.fastq_interleave_device([0, d_mate.data_ptr(), d_mate.data_ptr()], [0, n1, n1], d_il.data_ptr(), n)
    got, st = merge_dev()
    assert got == n and st.pairs == half
    res = {"records": 2 * half, "text_bytes": n, "reps": REPS}
    say("interleaved text", n, "bytes,", 2 * half, "records")
    il_pin = api.PinnedBuffer(n)
    il_pin.array[:] = d_il[:n].cpu().numpy()
    il = il_pin.array[:n]
    o1, o2, o0 = api.PinnedBuffer(n1), api.PinnedBuffer(n1), api.PinnedBuffer(1)
    outs = [o0.array[:0], o1.array, o2.array]
    split_host = lambda: eng.fastq_deinterleave(il, outs=outs)
    got, st = split_host()                                          # warm-up: arena, text buffer, staging
    assert np.array_equal(got[1], mate) and np.array_equal(got[2], mate) and st.pairs == half
    ro_pin = api.PinnedBuffer(n)
    reorder = lambda: eng.fastq_reorder([il], mode=1, seed=1, out=[ro_pin.array])
    reorder()
    # s1 and y1 alternating, on the same buffers
    s1, y1 = [], []
    for _ in range(REPS):
        s1.append(timed(split_host, sync))
        y1.append(timed(reorder, sync))
    res["s1_split_host_to_host"] = dict(wall_s=min(s1), walls=s1, text_GBps=n / min(s1) / 1e9)
    res["y1_reorder_mode1_host_to_host"] = dict(wall_s=min(y1), walls=y1, text_GBps=n / min(y1) / 1e9)
    res["y1_kernels"] = kernels(eng, reorder)
    say("split h2h", min(s1), "reorder mode 1 h2h", min(y1))
    d1 = torch.empty(n1 + 64, dtype=torch.uint8, device="cuda")
    d2 = torch.empty(n1 + 64, dtype=torch.uint8, device="cuda")
    d0 = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    for tag, opts, caps in (("s2_split_device", {}, [0, n1, n1]), ("s2_split_device_unchecked", dict(check_names=0), [0, n1, n1]),
                            ("s2_split_device_orphans", dict(orphans=1), [n, n1, n1])):
        call = lambda: eng.fastq_deinterleave_device(d_il.data_ptr(), n, [d0.data_ptr(), d1.data_ptr(), d2.data_ptr()], caps, **opts)
        ol, nr, st = call()
        assert ol == [0, n1, n1] and torch.equal(d1[:n1], d_mate[:n1]) and torch.equal(d2[:n1], d_mate[:n1]), tag
        res[tag] = dict(best(call, sync), kernels=kernels(eng, call))
        res[tag]["text_GBps"] = n / res[tag]["wall_s"] / 1e9
        say(tag, res[tag]["wall_s"], res[tag]["kernels"])
    res["m2_merge_device"] = dict(best(merge_dev, sync), kernels=kernels(eng, merge_dev))
    res["m2_merge_device"]["text_GBps"] = n / res["m2_merge_device"]["wall_s"] / 1e9
    say("merge device", res["m2_merge_device"]["wall_s"], res["m2_merge_device"]["kernels"])
    merge_host = lambda: eng.fastq_interleave([None, mate, mate], out=ro_pin.array)
    got, st = merge_host()
    assert np.array_equal(got, il)
    res["m1_merge_host_to_host"] = best(merge_host, sync)
    res["m1_merge_host_to_host"]["text_GBps"] = n / res["m1_merge_host_to_host"]["wall_s"] / 1e9
    say("merge h2h", res["m1_merge_host_to_host"]["wall_s"])
    # y2: a device-to-device copy of the same bytes, events around 10 copies
    d0[:n].copy_(d_il[:n])
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        e0.record()
        for _ in range(10):
            d0[:n].copy_(d_il[:n])
        e1.record()
        sync()
        ms.append(e0.elapsed_time(e1) / 10)
    res["y2_d2d_copy"] = dict(ms=min(ms), all_ms=ms, GBps_read_plus_write=2 * n / (min(ms) * 1e-3) / 1e9)
    say("d2d copy", min(ms), "ms")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
