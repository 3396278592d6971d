"""Host side of the interleaved paired FASTQ calls (csrc/bfq_pairs.h): the host forms (HostText.fastq_deinterleave_host,
HostText.fastq_interleave_host) against the plain-Python statement of the definition (tests/pairs_model.py) -- bytes,
statistics and every refusal's message --, the identities between the two directions, and the same code compiled for the
host with sanitizers and run as a program of its own."""
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import pairs_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


def guarded(lengths):
    """one 0xA5 buffer with a window of the exact size per length, 32 bytes of guard around each"""
    buf = np.full(sum(n + 64 for n in lengths) + 64, 0xA5, np.uint8)
    wins, at = [], 32
    for n in lengths:
        wins.append(buf[at:at + n])
        at += n + 64
    return buf, wins


def untouched(buf, wins):
    """the guards of a guarded() buffer hold their byte"""
    mask = np.ones(len(buf), bool)
    base = buf.ctypes.data
    for w in wins:
        o = w.ctypes.data - base
        mask[o:o + len(w)] = False
    return bool((buf[mask] == 0xA5).all())


@pytest.mark.parametrize("name", P.SPLIT_NAMES)
def test_host_split_equals_the_model(name):
    text, opts = P.split_cases()[name]
    want, wst = P.expect_split(name)
    got, st = host.fastq_deinterleave_host(text, **opts)
    assert [g.tobytes() for g in got] == want, name
    assert st.as_dict() == wst and st.n_reads == [wst["singles"], wst["pairs"], wst["pairs"]], name
    buf, wins = guarded([len(w) for w in want])                   # into guarded buffers of the exact size
    got, st = host.fastq_deinterleave_host(text, outs=wins, **opts)
    assert [g.tobytes() for g in got] == want and untouched(buf, wins), name


@pytest.mark.parametrize("name", P.MERGE_NAMES)
def test_host_merge_equals_the_model(name):
    texts, opts = P.merge_cases()[name]
    want, wst = P.expect_merge(name)
    got, st = host.fastq_interleave_host(texts, **opts)
    assert got.tobytes() == want and st.as_dict() == wst, name
    buf, (win,) = guarded([len(want)])
    got, st = host.fastq_interleave_host(texts, out=win, **opts)
    assert got.tobytes() == want and untouched(buf, [win]), name


def test_the_wide_case_holds_what_it_is_for():
    """by counting, on the model alone: singles, pairs, and a run longer than the scan chunk the kernels use"""
    singles, pairs, longest = P.wide_counts()
    assert singles >= 1 and pairs >= 1 and longest == 5001 > P.SCAN_CHUNK
    assert singles + 2 * pairs == 70000 and 70000 > 1 << 16
    with open(os.path.join(ROOT, "bfqzip_amd", "csrc", "k_pairs.hip")) as f:
        assert "#define PR_SCAN_CHUNK (PR_SCAN_THREADS * PR_SCAN_ITEMS)" in f.read() and P.SCAN_CHUNK == 256 * 16
    (t0, t1, t2), st = P.expect_split("wide-orphans")
    assert st["singles"] == singles and b"@o4000/1\n" in t0               # the odd long run ends in a single
    assert 4_500_000 < len(P.wide_text()) < 6_500_000


def test_the_key_rule():
    k = P.key
    assert k(b"@x/1") == k(b"@x/2") == b"x" and k(b"@/1") == b"/1" and k(b"@") == b"" and k(b"") == b""
    assert k(b"@a b/1") == b"a" and k(b"@a\tb") == b"a" and k(b"@a\r") == b"a" and k(b"@a/1/2") == b"a/1" and k(b"@x/1", 0) == b"x/1"
    one = lambda h1, h2, **o: host.fastq_deinterleave_host(P.rec(h1, b"A") + P.rec(h2, b"C"), **o)[1].pairs
    assert one(b"@x/1", b"@x/1") == 1 and one(b"@/1", b"@/1") == 1 and one(b"@", b"@ c") == 1 and one(b"@a\r", b"@a") == 1
    assert one(b"@x/1", b"@x/2", orphans=1, mate_suffix=0) == 0 and one(b"@x/3", b"@x/3") == 1


def test_refusals_carry_the_models_message_and_write_nothing():
    for name, (text, opts, code, msg) in P.split_refusals().items():
        buf, wins = guarded([len(text) + 1] * 3)
        with pytest.raises(api.BfqError) as e:
            host.fastq_deinterleave_host(text, outs=wins, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all() and e.value.needed == [0, 0, 0], name
    for name, (texts, opts, code, msg) in P.merge_refusals().items():
        buf, (win,) = guarded([sum(len(t) + 1 for t in texts if t is not None)])
        with pytest.raises(api.BfqError) as e:
            host.fastq_interleave_host(texts, out=win, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all() and e.value.needed == 0, name


@pytest.mark.parametrize("name", ("edges", "lanes", "orphans-singles-first", "wide-orphans"))
def test_a_buffer_one_byte_short(name):
    text, opts = P.split_cases()[name]
    want, _ = P.expect_split(name)
    for short in range(3):
        if not len(want[short]):
            continue
        buf, wins = guarded([len(w) - (k == short) for k, w in enumerate(want)])
        with pytest.raises(api.BfqError) as e:
            host.fastq_deinterleave_host(text, outs=wins, **opts)
        assert e.value.code == -1 and e.value.needed == [len(w) for w in want] and (buf == 0xA5).all()
    if name in P.merge_cases():
        texts, mo = P.merge_cases()[name]
        mw, _ = P.expect_merge(name)
        buf, (win,) = guarded([len(mw) - 1])
        with pytest.raises(api.BfqError) as e:
            host.fastq_interleave_host(texts, out=win, **mo)
        assert e.value.code == -1 and e.value.needed == len(mw) and (buf == 0xA5).all()


@pytest.mark.parametrize("name", ("edges", "edges-nolf", "lanes", "long", "wide", "one-pair", "empty"))
def test_merge_of_the_split_is_the_text(name):
    text, opts = P.split_cases()[name]
    (t0, t1, t2), _ = host.fastq_deinterleave_host(text, **opts)
    back, _ = host.fastq_interleave_host([None, t1, t2], **opts)
    assert back.tobytes() == text + (b"\n" if text and not text.endswith(b"\n") else b"")
    (_, u1, u2), _ = host.fastq_deinterleave_host(back, **opts)    # and the split of the merge gives the mates
    assert u1.tobytes() == t1.tobytes() and u2.tobytes() == t2.tobytes()


@pytest.mark.parametrize("name", [n for n in P.SPLIT_NAMES if "orphans" in n])
def test_the_orphan_split_holds_every_record_once(name):
    text, opts = P.split_cases()[name]
    outs, st = host.fastq_deinterleave_host(text, **opts)
    recs = lambda t: sorted(r for _, r in P.records(t.tobytes() if hasattr(t, "tobytes") else t))
    assert sorted(recs(outs[0]) + recs(outs[1]) + recs(outs[2])) == recs(text)
    assert st.records == st.singles + 2 * st.pairs


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_pairs_default_opts", "bfq_pairs_host_error", "bfq_fastq_deinterleave_measure", "bfq_fastq_deinterleave", "bfq_fastq_deinterleave_device",
              "bfq_fastq_deinterleave_fd", "bfq_fastq_deinterleave_host", "bfq_fastq_interleave_measure", "bfq_fastq_interleave",
              "bfq_fastq_interleave_device", "bfq_fastq_interleave_fd", "bfq_fastq_interleave_host"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.PairsOpts) == 16 and C.sizeof(_lib.PairsStats) == 48
    o = _lib.PairsOpts(9, 9, 9, 9)
    L.bfq_pairs_default_opts(C.byref(o))
    assert (o.check_names, o.mate_suffix, o.orphans, o.reserved) == (1, 1, 0, 0)


def test_pairs_opts_defaults_and_reserved():
    o = api.pairs_opts()
    assert (o.check_names, o.mate_suffix, o.orphans, o.reserved) == (1, 1, 0, 0)
    text = P.split_cases()["one-pair"][0]
    for call in (lambda: host.fastq_deinterleave_host(text, reserved=1), lambda: host.fastq_interleave_host([None, text, text], reserved=2)):
        with pytest.raises(api.BfqError) as e:
            call()
        assert e.value.code == -1 and "bfq_pairs_opts.reserved: must be 0" in str(e.value)


def test_pairs_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_pairs")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_pairs.cpp")])
    lines, n = [], [0]

    def put(data):
        n[0] += 1
        p = str(tmp_path / ("f%d" % n[0]))
        with open(p, "wb") as f:
            f.write(data if data is not None else b"")
        return p if data is not None else "-"

    words = lambda o: "%d %d %d %d" % (o.get("check_names", 1), o.get("mate_suffix", 1), o.get("orphans", 0), o.get("reserved", 0))
    for name in P.SPLIT_NAMES:
        text, opts = P.split_cases()[name]
        want, st = P.expect_split(name)
        lines.append("split %s %s %s %s %s %d %d" % (put(text), words(opts), put(want[0]), put(want[1]), put(want[2]), st["pairs"], st["singles"]))
    for name in P.MERGE_NAMES:
        texts, opts = P.merge_cases()[name]
        want, st = P.expect_merge(name)
        lines.append("merge %s %s %s %s %s %d %d" % (put(texts[0]), put(texts[1]), put(texts[2]), words(opts), put(want), st["pairs"], st["singles"]))
    for name, (text, opts, code, msg) in P.split_refusals().items():
        lines.append("badsplit %s %s %s %d" % (put(text), words(opts), put(msg.encode()), code))
    for name, (texts, opts, code, msg) in P.merge_refusals().items():
        lines.append("badmerge %s %s %s %s %s %d" % (put(texts[0]), put(texts[1]), put(texts[2]), words(opts), put(msg.encode()), code))
    man = put(("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert b"%d cases, 0 failures" % len(lines) in r.stdout


# ---- parallel.py --interleaved / --interleaved-out ------------------------------------------------------------------------
import hashlib
import sys
from bfqzip_amd import parallel
from tests import util
from tests.test_parallel_gloo import paired_inputs


class ModelPairsEngine(util.OracleEngine):
    """The CPU oracle per block, the model as Engine.fastq_deinterleave_files / fastq_interleave_files; every call leaves a
    line in `journal`."""
    journal = None

    def _note(self, what):
        if self.journal:
            with open(self.journal, "a") as f:
                f.write("rank %s: %s\n" % (os.environ.get("RANK", "0"), what))

    def fastq_deinterleave_files(self, src, dsts, **opts):
        try:
            outs, st = P.split(open(src, "rb").read(), **opts)
        except P.Refused as e:
            raise api.BfqError(e.code, e.msg)
        for d, o in zip(dsts, outs):
            if d is not None:
                open(d, "wb").write(o)
        self._note("split " + " ".join(d for d in dsts if d))
        return st["out_len"], [st["singles"], st["pairs"], st["pairs"]], st

    def fastq_interleave_files(self, texts, dst, **opts):
        try:
            out, st = P.merge([None if t is None else open(t, "rb").read() for t in texts], **opts)
        except P.Refused as e:
            raise api.BfqError(e.code, e.msg)
        open(dst, "wb").write(out)
        self._note("merge " + dst)
        return len(out), st

    def close(self):
        pass


def _interleaved(tmp):
    """(the interleaved file of the paired golden input, the two texts the model splits it into)"""
    f1, f2 = paired_inputs(tmp)
    text = P.merge([None, open(f1, "rb").read(), open(f2, "rb").read()])[0]
    path = os.path.join(tmp, "both.fq")
    open(path, "wb").write(text)
    (_, t1, t2), _ = P.split(text)
    assert (t1, t2) == (open(f1, "rb").read(), open(f2, "rb").read())
    return path, (f1, f2)


def _paired_run(orc, mates, tmp, headers=False):
    """`-p -t 4` on the two files the model gives, written elsewhere: the bytes the --interleaved run must give"""
    names = parallel.output_names(list(mates), os.path.join(tmp, "WANT"), True)
    parallel.run_files(util.OracleEngine(orc, m=5), parallel.Comm(), list(mates), 4, names, paired=True, headers=headers)
    return [open(n["fastq"], "rb").read() for n in names]


def test_driver_splits_then_runs_then_merges(orc, tmp_path, monkeypatch):
    tmp = str(tmp_path)
    os.mkdir(os.path.join(tmp, "o"))
    path, mates = _interleaved(tmp)
    journal = os.path.join(tmp, "journal")
    monkeypatch.setattr(ModelPairsEngine, "journal", journal)
    monkeypatch.setattr(api, "Engine", lambda dev, **par: ModelPairsEngine(orc, **par))
    out, il = os.path.join(tmp, "o", "OUT"), os.path.join(tmp, "o", "il.fq")
    mids = [os.path.join(tmp, "o", "both_1.fastq"), os.path.join(tmp, "o", "both_2.fastq")]      # named as one paired BAM's texts
    assert parallel.bam_names(path, out, True) == mids
    for headers in (False, True):
        want = _paired_run(orc, mates, tmp, headers=headers)
        assert parallel.main([path, "--interleaved", "-t", "4", "-o", out, "--interleaved-out", il] + (["-H"] if headers else [])) == 0
        got = [open(out + "_1.fastq", "rb").read(), open(out + "_2.fastq", "rb").read()]
        assert got == want                                         # byte-identical to -p on the two files the model gives
        assert open(il, "rb").read() == P.merge([None] + want)[0]   # the interleaved output: the model's merge of those outputs
        assert not any(os.path.exists(m) for m in mids)             # the intermediates are removed ...
    assert parallel.main([path, "--interleaved", "-t", "4", "-o", out, "--keep-inflated"]) == 0
    assert [open(m, "rb").read() for m in mids] == [open(f, "rb").read() for f in mates]          # ... unless they are kept
    # -p on two files with --interleaved-out alone, and with --reorder --keep-order: merged after the order is restored
    assert parallel.main(list(mates) + ["-p", "-t", "4", "-o", out, "-H", "--interleaved-out", il]) == 0
    assert open(il, "rb").read() == P.merge([None] + _paired_run(orc, mates, tmp, headers=True))[0]
    lines = open(journal).read().splitlines()
    assert [l.split()[2] for l in lines] == ["split", "merge", "split", "merge", "split", "merge"]


def test_driver_refuses_up_front_and_names_the_bad_pair(orc, tmp_path, monkeypatch, capsys):
    tmp = str(tmp_path)
    os.mkdir(os.path.join(tmp, "o"))
    path, mates = _interleaved(tmp)
    out, il = os.path.join(tmp, "o", "OUT"), os.path.join(tmp, "o", "il.fq")
    made = []
    monkeypatch.setattr(api, "Engine", lambda dev, **par: made.append(1) or ModelPairsEngine(orc, **par))
    for args in ([path, path, "--interleaved"], [path, "--interleaved", "--bam"], [path, "--interleaved-out", il],
                 [path, "--interleaved", "--interleaved-out", il, "--m2", "--streams-only"], [path, "--interleaved", "--interleaved-out", il, "--compress"],
                 list(mates) + ["--interleaved-out", il]):
        assert parallel.main(args + ["-o", out, "-t", "2"]) == 1, args
    assert not made and os.listdir(os.path.join(tmp, "o")) == []     # before an engine exists, nothing written
    # a file that is not properly paired: the library's message, before any block runs
    text = open(path, "rb").read()
    recs = [r for _, r in P.records(text)]
    bad = os.path.join(tmp, "bad.fq")
    open(bad, "wb").write(b"".join(recs[:7] + recs[8:]))            # record 7 lost: pair 3 holds records of two names
    capsys.readouterr()
    assert parallel.main([bad, "--interleaved", "-o", out, "-t", "2"]) == 1
    err = capsys.readouterr().err
    assert "interleaved FASTQ: 199 records, an odd number" in err
    open(bad, "wb").write(b"".join(recs[:7] + recs[8:] + recs[7:8]))
    assert parallel.main([bad, "--interleaved", "-o", out, "-t", "2"]) == 1
    assert "interleaved FASTQ: pair 3 (records 6 and 7): the names differ" in capsys.readouterr().err
    assert os.listdir(os.path.join(tmp, "o")) == []                  # no output, no intermediate left behind


def _pairs_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import orc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = parallel.Comm(dist)
    ModelPairsEngine.journal = os.path.join(tmp, "journal2")
    eng = ModelPairsEngine(orc, m=5)
    try:
        new, mids, why = parallel.split_interleaved_input(eng, comm, [os.path.join(tmp, "both.fq")], os.path.join(tmp, "G"))
        assert why is None and new == mids
        names = parallel.output_names(new, os.path.join(tmp, "G"), True)
        parallel.run_files(eng, comm, new, 4, names, paired=True)
        il = os.path.join(tmp, "G.il.fq")
        assert parallel.merge_interleaved_output(eng, comm, [n["fastq"] for n in names], il, False) is None
        bad, _, why = parallel.split_interleaved_input(eng, comm, [os.path.join(tmp, "odd.fq")], os.path.join(tmp, "B"))
        assert why and (rank or "an odd number" in why) and bad == [os.path.join(tmp, "odd.fq")]   # every rank learns of the refusal, rank 0 of its words
        if rank == 0:
            q.put("|".join(new + [hashlib.md5(open(f, "rb").read()).hexdigest() for f in [n["fastq"] for n in names] + [il]]))
    except Exception as e:                                     # surface the failure instead of a queue timeout
        q.put(f"rank {rank}: {type(e).__name__}: {e}")
        raise
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_gloo_interleaved(orc, tmp_path):
    """2 ranks: rank 0 alone splits and merges, both run on the mates after the barrier."""
    import torch.multiprocessing as mp
    tmp = str(tmp_path)
    path, mates = _interleaved(tmp)
    open(os.path.join(tmp, "odd.fq"), "wb").write(P.rec(b"@z", b"ACGT"))
    want = _paired_run(orc, mates, tmp)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 34600 + (os.getpid() * 7) % 2000
    ps = [ctx.Process(target=_pairs_worker, args=(rk, 2, port, tmp, q)) for rk in range(2)]
    for p in ps:
        p.start()
    got = q.get(timeout=180)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0, got
    mids = [os.path.join(tmp, "both_1.fastq"), os.path.join(tmp, "both_2.fastq")]
    assert got.split("|") == mids + [hashlib.md5(w).hexdigest() for w in want + [P.merge([None] + want)[0]]]
    assert [open(m, "rb").read() for m in mids] == [open(f, "rb").read() for f in mates]
    lines = open(os.path.join(tmp, "journal2")).read().splitlines()
    assert len(lines) == 2 and all(l.startswith("rank 0: ") for l in lines)                       # only rank 0 writes
