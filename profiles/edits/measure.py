"""Measurements behind profiles/edits/README.md (not a test): N x L synthetic reads as FASTQ text (Engine.synth_fastq), m = 5.
  (size) fastq_job(compress=True, streams=True, edits=True): E, the member's bytes, bits per edit, its share of the DNA container;
  (job)  fastq_job(fastq=True) into pinned buffers with and without edits=True, the two variants alternated, REPS rounds after a
         warm-up: every wall time is kept (the spread), and the library's events per kernel of one call of each;
  (make) fastq_edits on the input and the job's output text, and fastq_compare on the same two texts: the events per kernel
         (k_edit_* against k_cmp_*), and the wall time around each call from pinned memory;
  (back) fastq_unedit of the output text: wall time and events.
With --job-only only (job) without edits runs: the form that also runs on the parent commit's package.

    python profiles/edits/measure.py --reads 3000000 --len 150 --out edits_measure.json"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.environ.get("BFQ_MEASURE_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    r = f()
    return {k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in eng.prof().items()}, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--out", default="")
    ap.add_argument("--job-only", action="store_true")
    ap.add_argument("--no-size", action="store_true")
    a = ap.parse_args()
    eng = api.Engine(0, m=5)
    pin_in = api.PinnedBuffer(a.reads * (2 * a.len + 30))
    n = eng.synth_fastq(api.synth_spec(a.reads, a.len), pin_in.array)
    text = pin_in.array[:n]
    pins = {k: api.PinnedBuffer(n + 4096) for k in ("fastq",)}
    pins["edits"] = api.PinnedBuffer(n // 8 + 4096)
    out = {k: p.array for k, p in pins.items()}
    res = dict(reads=a.reads, length=a.len, text_bytes=int(n), root=ROOT)
    job = lambda **kw: eng.fastq_job([text], fastq=True, out=dict(out), **kw)
    job()                                                          # warm-up: arena, text buffer
    if a.job_only:
        res["job_plain_walls"] = [round(timed(job)[0], 5) for _ in range(REPS)]
        say(res)
    else:
        job(edits=True)
        plain, withe = [], []
        for _ in range(REPS):
            plain.append(round(timed(job)[0], 5))
            withe.append(round(timed(lambda: job(edits=True))[0], 5))
        res["job_plain_walls"], res["job_edits_walls"] = plain, withe
        res["job_plain_kernels"], _ = kernels(eng, job)
        res["job_edits_kernels"], r = kernels(eng, lambda: job(edits=True))
        res["job_edits_kernels"] = {k: v for k, v in res["job_edits_kernels"].items() if k.startswith("k_edit") or k == "k_scan"}
        res["job_plain_has_k_edit"] = any(k.startswith("k_edit") for k in res["job_plain_kernels"])
        res["job_plain_kernels"] = {k: v for k, v in res["job_plain_kernels"].items() if k == "k_scan"}
        info = api.edits_info(r.edits)
        res["edits"] = dict(info, bytes=len(r.edits), bits_per_edit=round(8 * len(r.edits) / max(info["n_edits"], 1), 3))
        say("job", plain, withe, res["edits"])
        outtext = api.PinnedBuffer(len(r.fastq))
        outtext.array[:] = r.fastq
        member = r.edits.copy()
        zbuf = api.PinnedBuffer(len(member) + 64)
        mk = lambda: eng.fastq_edits([text], [outtext.array], out=zbuf.array)
        z, st = mk()
        assert z.tobytes() == member.tobytes(), "the member of the two texts is not the job's"
        res["make_walls"] = [round(timed(mk)[0], 5) for _ in range(REPS)]
        res["make_kernels"], _ = kernels(eng, mk)
        cmpf = lambda: eng.fastq_compare([text], [outtext.array])
        rep = cmpf()
        assert rep.bases_changed == info["n_edits"]
        res["compare_walls"] = [round(timed(cmpf)[0], 5) for _ in range(REPS)]
        res["compare_kernels"], _ = kernels(eng, cmpf)
        back = api.PinnedBuffer(len(r.fastq) + 8)
        un = lambda: eng.fastq_unedit(outtext.array, member, out=back.array)
        un()
        res["unedit_walls"] = [round(timed(un)[0], 5) for _ in range(REPS)]
        res["unedit_kernels"], _ = kernels(eng, un)
        say("make", res["make_walls"], "compare", res["compare_walls"], "unedit", res["unedit_walls"])
        if not a.no_size:
            zr = eng.fastq_job([text], fastq=False, streams=True, compress=True, edits=True)
            assert zr.edits.tobytes() == member.tobytes()
            res["size"] = dict(edits_bytes=len(zr.edits), dna_container_bytes=len(zr.dna), qs_container_bytes=len(zr.qs),
                               share_of_dna_container=round(len(zr.edits) / len(zr.dna), 5), total_bases=info["total_bases"],
                               edits_per_base=round(info["n_edits"] / info["total_bases"], 6))
            say("size", res["size"])
    js = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(js + "\n")
    print(js)
    eng.close()


if __name__ == "__main__":
    main()
