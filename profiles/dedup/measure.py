"""Measurements behind profiles/dedup/README.md (not a test).  The workload: N x 150 synthetic reads as FASTQ text
(Engine.synth_fastq) in pinned host memory, 10 % of the records given the sequence of an earlier record (their own header and
qualities stay: fresh qualities) and `--polyg` per cent given one poly-G read; paired: a second text from another seed with
the same records replaced from the same earlier ones.  Every call five times after a warm-up, alternating with the call it is
compared to; medians and ranges are kept, and all five.
  (h)  bfq_fastq_dedup, pinned host to pinned host, against bfq_fastq_reorder mode 1 on the same bytes
  (d)  bfq_fastq_dedup_device against bfq_fastq_repair_device on the same device texts, and a device-to-device copy of the bytes
  (k)  the library's events per kernel id of one device call (the names per kernel come from a rocprofv3 --kernel-trace run of
       --one-call: no counters and no tracing in the timed runs)
  (g)  the same at 4 x the poly-G share: no kernel may grow faster than the group
  (o)  the one-thread host form
  (r)  Engine.fastq_run_streams on the text before and after the dedup (the path of bfq_run_reads behind the FASTQ parser; not
       that call itself, which takes parsed reads): time, and the bytes of its three streams through stream_compress
--one-call: a warm-up and one device call, for a profiler around the process.

    python profiles/dedup/measure.py --reads 3000000 --out profiles/dedup/measure_3Mx150.json"""
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


def spread(v):
    v = sorted(v)
    return dict(median_s=v[len(v) // 2], min_s=v[0], max_s=v[-1], all_s=v)


def alternate(f, g):
    """f and g in turn, REPS times each after a warm-up of both"""
    f(); g()
    tf, tg = [], []
    for _ in range(REPS):
        tf.append(timed(f)[0])
        tg.append(timed(g)[0])
    return spread(tf), spread(tg)


def seq_starts(text):
    """where the sequence line of every record starts"""
    lf = np.flatnonzero(text == 10)
    assert len(lf) % 4 == 0
    return lf[0::4] + 1


def workload(eng, reads, polyg_pct, paired):
    """([pinned text per mate], their lengths); the replaced records and their sources are the same in both mates"""
    rng = np.random.default_rng(7)
    n_dup, n_g = reads // 10, reads * polyg_pct // 100
    victims = rng.choice(np.arange(1, reads), n_dup + n_g, replace=False)
    dup_v, g_v = np.sort(victims[:n_dup]), victims[n_dup:]
    src = (rng.random(n_dup) * dup_v).astype(np.int64)             # an earlier record each
    col = np.arange(150)
    texts = []
    for m in range(2 if paired else 1):
        pb = api.PinnedBuffer(reads * 330 + 4096)
        n = eng.synth_fastq(api.synth_spec(reads, 150, seed=1 + m), pb.array)
        t = pb.array[:n]
        ss = seq_starts(t)
        assert len(ss) == reads
        for lo in range(0, n_dup, 1 << 16):                        # in order: a source may itself be a copy
            v, s = dup_v[lo:lo + (1 << 16)], src[lo:lo + (1 << 16)]
            t[ss[v][:, None] + col] = t[ss[s][:, None] + col]
        t[ss[g_v][:, None] + col] = ord("G")
        texts.append((pb, t))
    return texts


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--polyg", type=int, default=1)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--skip-run", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    REPS = a.reps
    import torch
    eng = api.Engine(0, m=5)
    res = {"reads": a.reads, "polyg_pct": a.polyg, "reps": REPS}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    def device_forms(texts, label, with_repair=True):
        """(d), (k): the device texts, the outputs, the two calls in turn"""
        d_in = [torch.from_numpy(t).cuda() for _, t in texts]
        lens = [len(t) for _, t in texts]
        d_out = [torch.empty(n + 16, dtype=torch.uint8, device="cuda") for n in lens] + [torch.empty(16, dtype=torch.uint8, device="cuda")] * (2 - len(lens))
        d_dup = [torch.empty(n + 16, dtype=torch.uint8, device="cuda") for n in lens] + [torch.empty(16, dtype=torch.uint8, device="cuda")] * (2 - len(lens))
        ptr = lambda ts: [t.data_ptr() for t in ts]
        caps = [len(t) for t in d_out]
        dd = lambda **o: eng.fastq_dedup_device(ptr(d_in), lens, ptr(d_out), caps, ptr(d_dup), caps, **o)
        r = {}
        if with_repair:
            # the repair takes the mates as texts 1 and 2 and writes three outputs: the singletons of a single text are all of it
            r_in = [None] + ptr(d_in) + [None] * (2 - len(d_in))
            r_len = [0] + lens + [0] * (2 - len(lens))
            r_out = [torch.empty(sum(lens) + 16, dtype=torch.uint8, device="cuda") for _ in range(3)]
            rp = lambda: eng.fastq_repair_device(r_in, r_len, ptr(r_out), [len(t) for t in r_out])
            r["dedup_device"], r["repair_device"] = alternate(dd, rp)
            del r_out
        else:
            dd()
            r["dedup_device"] = spread([timed(dd)[0] for _ in range(REPS)])
        r["dedup_device_best"] = spread([timed(lambda: dd(keep=1))[0] for _ in range(REPS)])
        ol, dl, st = dd()
        r["stats"] = {k: v for k, v in st.as_dict().items() if not k.startswith("level")}
        r["levels"] = {str(k): [g, u] for k, (g, u) in enumerate(zip(st.level_groups, st.level_units)) if g}
        for key, o in (("kernel_ids", {}), ("kernel_ids_best", dict(keep=1))):
            eng.prof_reset()
            dd(**o)
            r[key] = {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items() if v["launches"]}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(REPS):
            e0.record()
            for d, s in zip(d_out, d_in):
                d[:len(s)].copy_(s)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e-3)
        r["d2d_copy"] = spread(ms)
        res[label] = r
        say(label, "dedup", r["dedup_device"]["median_s"], "best", r["dedup_device_best"]["median_s"], "repair", r.get("repair_device", {}).get("median_s"),
            "copy", r["d2d_copy"]["median_s"], r["stats"], r["kernel_ids"])
        save()
        return dd

    single = workload(eng, a.reads, a.polyg, False)
    say("single text", len(single[0][1]))
    if a.one_call:
        dd = device_forms(single, "one_call", with_repair=False)
        eng.close()
        return
    A = single[0][1]
    # (h) pinned host to pinned host against the reorder
    po, pd, pr = api.PinnedBuffer(len(A) + 16), api.PinnedBuffer(len(A) + 16), api.PinnedBuffer(len(A) + 16)
    f = lambda: eng.fastq_dedup([A], outs=[po.array, np.empty(0, np.uint8)], dups=[pd.array, np.empty(0, np.uint8)])
    g = lambda: eng.fastq_reorder([A], mode=1, out=[pr.array])
    res["host_single"] = dict(zip(("dedup", "reorder_mode_1"), alternate(f, g)))
    res["host_single"]["ratio_of_medians"] = res["host_single"]["dedup"]["median_s"] / res["host_single"]["reorder_mode_1"]["median_s"]
    say("host single", res["host_single"]["dedup"]["median_s"], res["host_single"]["reorder_mode_1"]["median_s"])
    save()
    outs, _, st = f()
    kept_text = outs[0].copy()
    device_forms(single, "device_single")
    # (o) the one-thread host form
    t, (ho, hd, hst) = timed(lambda: api.fastq_dedup_host([A], dups=True))
    res["host_one_thread"] = dict(wall_s=t, equal_to_device=bool(ho[0].tobytes() == kept_text.tobytes() and hst.as_dict() == st.as_dict()))
    say("host form", res["host_one_thread"])
    save()
    # (r) what the run gains
    if not a.skip_run:
        try:
            rr = {}
            for key, text in (("before", A), ("after", kept_text)):
                eng.fastq_run_streams(text)
                t, (dna, qs, hdr, rst) = timed(lambda: eng.fastq_run_streams(text))
                z = [len(eng.stream_compress(np.frombuffer(s, np.uint8))) for s in (dna, qs, hdr) if s]
                rr[key] = dict(text_bytes=int(len(text)), run_s=t, reads=int(rst["n_reads"]), compressed_bytes=z, compressed_total=sum(z))
                say("run", key, rr[key])
            res["run"] = rr
        except Exception as e:                                      # (the rest of the numbers stand without it)
            res["run"] = dict(error=repr(e))
        save()
    del po, pd, pr
    # paired
    pair = workload(eng, a.reads, a.polyg, True)
    P1, P2 = pair[0][1], pair[1][1]
    o1, o2, d1, d2 = (api.PinnedBuffer(len(t) + 16) for t in (P1, P2, P1, P2))
    r1, r2 = api.PinnedBuffer(len(P1) + 16), api.PinnedBuffer(len(P2) + 16)
    f = lambda: eng.fastq_dedup([P1, P2], outs=[o1.array, o2.array], dups=[d1.array, d2.array])
    g = lambda: eng.fastq_reorder([P1, P2], mode=1, out=[r1.array, r2.array])
    res["host_paired"] = dict(zip(("dedup", "reorder_mode_1"), alternate(f, g)))
    res["host_paired"]["ratio_of_medians"] = res["host_paired"]["dedup"]["median_s"] / res["host_paired"]["reorder_mode_1"]["median_s"]
    say("host paired", res["host_paired"]["dedup"]["median_s"], res["host_paired"]["reorder_mode_1"]["median_s"])
    save()
    del o1, o2, d1, d2, r1, r2
    device_forms(pair, "device_paired")
    del pair, P1, P2
    # (g) four times the poly-G group
    big = workload(eng, a.reads, 4 * a.polyg, False)
    device_forms(big, "device_single_polyg_x4", with_repair=False)
    print(json.dumps({k: v for k, v in res.items()}))
    save()
    eng.close()


if __name__ == "__main__":
    main()
