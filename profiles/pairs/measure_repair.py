"""Measurements of the repair behind profiles/pairs/README.md (not a test): N / 2 x 150 synthetic reads as FASTQ text
(Engine.synth_fastq, headers "@SYN.<n>") as two mate texts, each with 5 % of its records dropped on its own (seeded), text 2
shuffled (bfq_fastq_reorder mode 1); then, every call 5 times after a warm-up (all five are kept; the median is compared):
  (r1) bfq_fastq_repair, the two texts in pinned host memory, the three outputs into pinned host memory, alternating with
  (y1) bfq_fastq_reorder mode 1 on the same bytes (the two texts one behind the other), pinned host to pinned host;
  (r2) bfq_fastq_repair_device, device to device, with the library's events per kernel of one call;
  (s2) bfq_fastq_deinterleave_device in orphan mode on the repaired mates interleaved (the same pairs, adjacent);
  (y2) a device-to-device copy of the same bytes, timed with events;
  (h)  bfq_fastq_repair_host, one CPU thread, once.
The outputs of r1 and r2 are compared with those of the host form.

    python profiles/pairs/measure_repair.py --reads 3000000 --out repair_measure.json"""
import argparse
import json
import os
import statistics
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


def summary(ts, n):
    return dict(median_s=statistics.median(ts), min_s=min(ts), walls=ts, text_GBps=n / statistics.median(ts) / 1e9)


def kernels(eng, f):
    eng.prof_reset()
    f()
    return {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items()}


def drop(text, frac, seed):
    """the text without a seeded `frac` of its records"""
    ends = np.flatnonzero(text == 10)[3::4] + 1
    lens = np.diff(np.concatenate([[0], ends]))
    keep = np.random.default_rng(seed).random(len(lens)) >= frac
    return text[np.repeat(keep, lens)], int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000, help="records of the two mate texts before the drop")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    sync = torch.cuda.synchronize
    eng = api.Engine(0, m=5)
    half = a.reads // 2
    mate = np.empty(half * 330 + 4096, np.uint8)
    mate = mate[:eng.synth_fastq(api.synth_spec(half, 150), mate)]
    t1, k1 = drop(mate, 0.05, 1)
    t2, k2 = drop(mate, 0.05, 2)
    t2 = eng.fastq_reorder([t2], mode=1, seed=7)[0][0].copy()
    n = len(t1) + len(t2)
    pin = api.PinnedBuffer(n)
    pin.array[:len(t1)] = t1
    pin.array[len(t1):n] = t2
    p1, p2, both = pin.array[:len(t1)], pin.array[len(t1):n], pin.array[:n]
    res = {"records": k1 + k2, "text_bytes": n, "reps": REPS}
    say("texts", len(t1), len(t2), "bytes,", k1, k2, "records")
    t0 = time.perf_counter()
    want, hst = api.HostText.fastq_repair_host([None, p1, p2])
    res["h_host_form_one_thread"] = dict(wall_s=time.perf_counter() - t0)
    res["stats"] = hst.as_dict()
    say("host form", res["h_host_form_one_thread"], hst)
    outs = [api.PinnedBuffer(len(w) + 1) for w in want]
    views = [o.array[:len(w)] for o, w in zip(outs, want)]
    repair = lambda: eng.fastq_repair([None, p1, p2], outs=views)
    got, st = repair()                                              # warm-up: arena, text buffer, staging
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and st.as_dict() == hst.as_dict()
    ro = api.PinnedBuffer(n)
    reorder = lambda: eng.fastq_reorder([both], mode=1, seed=1, out=[ro.array])
    reorder()
    r1, y1 = [], []
    for _ in range(REPS):
        r1.append(timed(repair, sync))
        y1.append(timed(reorder, sync))
    res["r1_repair_host_to_host"] = summary(r1, n)
    res["y1_reorder_mode1_host_to_host"] = summary(y1, n)
    res["r1_over_y1_medians"] = res["r1_repair_host_to_host"]["median_s"] / res["y1_reorder_mode1_host_to_host"]["median_s"]
    res["r1_kernels"] = kernels(eng, repair)
    res["y1_kernels"] = kernels(eng, reorder)
    say("repair h2h", r1, "reorder mode 1 h2h", y1, "ratio", res["r1_over_y1_medians"])
    d_in = torch.from_numpy(both).cuda()
    d_out = [torch.empty(len(w) + 64, dtype=torch.uint8, device="cuda") for w in want]
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()      # (each at an aligned address: taken where they lie)
    dev = lambda: eng.fastq_repair_device([0, d1.data_ptr(), d2.data_ptr()], [0, len(t1), len(t2)], [o.data_ptr() for o in d_out], [len(w) for w in want])
    ol, nr, st = dev()
    assert ol == [len(w) for w in want] and all(np.array_equal(o[:len(w)].cpu().numpy(), w) for o, w in zip(d_out, want))
    ts = [timed(dev, sync) for _ in range(REPS)]
    res["r2_repair_device"] = dict(summary(ts, n), kernels=kernels(eng, dev))
    say("repair device", ts, res["r2_repair_device"]["kernels"])
    m = len(want[1]) + len(want[2])
    d_il = torch.empty(m + 64, dtype=torch.uint8, device="cuda")
    assert eng.fastq_interleave_device([0, d_out[1].data_ptr(), d_out[2].data_ptr()], [0, len(want[1]), len(want[2])], d_il.data_ptr(), m)[0] == m
    d_s = [torch.empty(m + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    split = lambda: eng.fastq_deinterleave_device(d_il.data_ptr(), m, [o.data_ptr() for o in d_s], [m, m, m], orphans=1)
    assert split()[0] == [0, len(want[1]), len(want[2])]
    ts = [timed(split, sync) for _ in range(REPS)]
    res["s2_split_device_orphans"] = dict(summary(ts, m), kernels=kernels(eng, split), text_bytes=m)
    say("orphan split device", ts)
    d_copy = torch.empty(n, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS + 1):
        e0.record()
        for _ in range(10):
            d_copy.copy_(d_in)
        e1.record()
        sync()
        ms.append(e0.elapsed_time(e1) / 10)
    res["y2_d2d_copy"] = dict(ms=min(ms[1:]), all_ms=ms[1:], GBps_read_plus_write=2 * n / (min(ms[1:]) * 1e-3) / 1e9)
    say("d2d copy", ms)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
