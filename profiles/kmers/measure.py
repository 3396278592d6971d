"""Measurements behind profiles/kmers/README.md (not a test): N x 150 synthetic reads as FASTQ text (Engine.synth_fastq), A, and
the smoothed output of a run on them (Engine.fastq_run, headers kept), B, both in pinned host memory.  Every call 5 times after
a warm-up (the minimum and all five are kept: the spread):
  (w)  bfq_fastq_kmers A against B at k = 21, 20 and 31: the wall time around the call, and the library's events per kernel
       of one call (its own profile counters: no counter collection in the same run);
  (s)  the scatter time per row and pass of the k-mer sort (k_radix_scatter over passes x records), beside the suffix sort's
       on the same machine in the same process: the events of one Engine.fastq_run on A (five passes over bases + reads rows);
  (f)  the floor of the extraction: a device-to-device copy of the two texts' bytes, timed with events;
  (p)  with --part-records R: the same call cut into value ranges, its time, and the report equal to the uncut one;
  (c)  with --cap-mib M: a second engine under ws_cap_mib = M: the number of ranges, the time, the report equal to the first's;
  (h)  with --host: the one-thread host form on the same pair;
  (t)  with --trace: the scatter passes one by one (bfq_prof_trace), three calls each, of the suffix sort and of the k-mer
       sort at k = 21: the suffix sort's first pass generates its records (14.5 bytes per row, not 24), so only its passes
       1..4 are the kernel the k-mer sort runs.
--reps 1 --no-copy: one timed call per k and no copy, for the 30 M x 150 pair.

    python profiles/kmers/measure.py --reads 3000000 --host --out kmers_measure.json"""
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


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def kernels(eng, f):
    eng.prof_reset()
    f()
    return {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items() if v["launches"]}


def copy_floor(torch, A, B):
    """a device-to-device copy of as many bytes as both texts hold, events around 10 copies"""
    na = len(A)
    d_src = torch.from_numpy(np.concatenate([A[:1 << 20], B[:1 << 20]])).cuda()      # (any bytes will do)
    n = int(na) + int(len(B))
    d_a = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_a[:len(d_src)] = d_src
    d_b.copy_(d_a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        e0.record()
        for _ in range(10):
            d_b.copy_(d_a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    del d_a, d_b, d_src
    torch.cuda.empty_cache()
    return dict(ms=min(ms), all_ms=ms, GBps_read_plus_write=2 * n / (min(ms) * 1e-3) / 1e9)


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--part-records", type=int, default=0)
    ap.add_argument("--cap-mib", type=int, default=0)
    ap.add_argument("--ks", default="21,20,31")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    REPS = a.reps
    import torch
    eng = api.Engine(0, m=5)
    pa = api.PinnedBuffer(a.reads * 330 + 4096)
    na = eng.synth_fastq(api.synth_spec(a.reads, 150), pa.array)
    A = pa.array[:na]
    eng.prof_reset()
    t_run, (out, st) = timed(lambda: eng.fastq_run(A, keep_headers=True))
    prof_run = {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items() if v["launches"]}
    pb = api.PinnedBuffer(len(out))
    pb.array[:len(out)] = np.frombuffer(out, np.uint8)
    B = pb.array[:len(out)]
    del out
    res = {"reads": a.reads, "text_bytes": [int(na), int(len(B))], "reps": REPS, "run_s": t_run, "run_rows": int(st["n_rows"]),
           "run_kernels": prof_run}
    sc = prof_run.get("k_radix_scatter")
    if sc:
        res["suffix_sort_scatter_ns_per_row_pass"] = sc["ms"] * 1e6 / (sc["launches"] * st["n_rows"])
    say("texts", na, len(B), "run", t_run, "suffix scatter", sc)
    reports = {}
    for k in [int(v) for v in a.ks.split(",")]:
        call = lambda: eng.fastq_kmers([A], [B], k=k)
        _, rep = timed(call)                                        # warm-up: arena, text buffer, staging
        walls = [timed(call)[0] for _ in range(REPS)]
        kern = kernels(eng, call)
        rows = rep.windows_a + rep.windows_b
        passes = (2 * k + 7) // 8 if 2 * k <= 40 else (2 * k - 40 + 7) // 8 + 5
        r = dict(wall_s=min(walls), walls=walls, kernels=kern, records=rows, passes=passes, n_partitions=rep.n_partitions,
                 report={key: getattr(rep, key) for key in ("windows_a", "windows_b", "distinct_a", "distinct_b", "only_a", "only_b", "distinct_changed")},
                 trans=[int(v) for v in rep.trans.reshape(-1)])
        if "k_radix_scatter" in kern:
            r["scatter_ns_per_row_pass"] = kern["k_radix_scatter"]["ms"] * 1e6 / (passes * rows)
        res["k%d" % k] = r
        reports[k] = rep.as_dict()
        say("k", k, "wall", min(walls), "kernels", kern)
    if a.trace:
        eng.prof_trace_select("k_radix_scatter")
        tr = {"suffix_sort": [], "kmers_k21": []}
        for _ in range(3):
            eng.prof_reset()
            eng.fastq_run(A, keep_headers=True)
            tr["suffix_sort"].append([round(float(v), 4) for v in eng.prof_trace()])
            eng.prof_reset()
            eng.fastq_kmers([A], [B], k=21)
            tr["kmers_k21"].append([round(float(v), 4) for v in eng.prof_trace()])
        eng.prof_trace_select(None)
        res["scatter_passes_ms"] = tr
        say("trace", tr)
    if not a.no_copy:
        res["d2d_copy_of_both_texts"] = copy_floor(torch, A, B)
        say("d2d copy", res["d2d_copy_of_both_texts"]["ms"], "ms")
    if a.part_records:
        call = lambda: eng.fastq_kmers([A], [B], k=21, part_records=a.part_records)
        _, rep = timed(call)
        walls = [timed(call)[0] for _ in range(3)]
        d = rep.as_dict()
        same = {key: v for key, v in d.items() if key != "n_partitions"} == {key: v for key, v in reports[21].items() if key != "n_partitions"}
        res["partitioned"] = dict(part_records=a.part_records, n_partitions=rep.n_partitions, wall_s=min(walls), walls=walls, equal_to_uncut=same,
                                  kernels=kernels(eng, call))
        say("partitioned", res["partitioned"])
    if a.cap_mib:
        small = api.Engine(0, m=5, ws_cap_mib=a.cap_mib)
        call = lambda: small.fastq_kmers([A], [B], k=21)
        _, rep = timed(call)
        walls = [timed(call)[0] for _ in range(3)]
        d = rep.as_dict()
        same = {key: v for key, v in d.items() if key != "n_partitions"} == {key: v for key, v in reports[21].items() if key != "n_partitions"}
        res["capped"] = dict(cap_mib=a.cap_mib, n_partitions=rep.n_partitions, wall_s=min(walls), walls=walls, equal_to_uncapped=same)
        small.close()
        say("capped", res["capped"])
    if a.host:
        t, rep = timed(lambda: api.fastq_kmers_host(A, B, k=21))
        d = rep.as_dict()
        res["host_one_thread"] = dict(wall_s=t, equal_to_device={key: v for key, v in d.items() if key != "n_partitions"} ==
                                      {key: v for key, v in reports[21].items() if key != "n_partitions"})
        say("host", res["host_one_thread"])
    finish(res, a, eng)


def finish(res, a, eng):
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
