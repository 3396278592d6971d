"""Host side of the repair of paired FASTQ (bfq_fastq_repair*, csrc/bfq_pairs.h): the host form (HostText.fastq_repair_host)
against the plain-Python statement of the definition (tests/pairs_repair_model.py) -- bytes, statistics and every refusal's
message --, the identities of a repair, the hash, and the same code compiled for the host with sanitizers and run as a
program of its own."""
import os
import random
import subprocess
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import pairs_model as P
from tests import pairs_repair_model as R
from tests.test_pairs_host import guarded, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


@pytest.mark.parametrize("name", R.NAMES)
def test_host_repair_equals_the_model(name):
    texts, opts = R.all_cases()[name]
    want, wst = R.expect(name)
    got, st = host.fastq_repair_host(texts, **opts)
    assert [g.tobytes() for g in got] == want, name
    assert st.as_dict() == wst and st.n_reads == [wst["singles"], wst["pairs"], wst["pairs"]], name
    buf, wins = guarded([len(w) for w in want])                   # into guarded buffers of the exact size
    got, st = host.fastq_repair_host(texts, outs=wins, **opts)
    assert [g.tobytes() for g in got] == want and untouched(buf, wins), name


def test_the_cases_hold_what_they_are_for():
    """by counting, on the model alone"""
    n = lambda name: R.expect(name)[1]["records"]
    assert [n("absent"), n("empty"), n("n1"), n("n2"), n("filtered-65"), n("filtered-300"), n("filtered-3073"), n("filtered-4097"), n("filtered-6200")] == \
        [0, 0, 1, 2, 65, 300, 3073, 4097, 6200]
    st = R.expect("wide")[1]
    assert st["records"] == 70000 > 1 << 16 and st["singles"] > 5000 and st["pairs"] > 25000 and st["dup_groups"] >= 40
    assert 4_500_000 < sum(len(t) for t in R.cases()["wide"][0] if t) < 6_500_000
    for name in ("filtered-300", "mixed-suffix", "mixed-plain", "all-three", "groups", "groups-mixed", "keys"):
        st = R.expect(name)[1]
        assert st["pairs"] >= 1 and st["singles"] >= 1, name
    assert R.expect("groups")[1]["dup_groups"] == R.expect("groups-mixed")[1]["dup_groups"] == 25      # the mixes of 3 and 4 records
    assert R.expect("dup-r1")[1] == dict(records=4, pairs=1, singles=2, out_len=[24, 17, 13], n_in=[0, 3, 1], dup_groups=1, mixed_runs=0, max_run=3)
    assert R.expect("bound-1024")[1]["pairs"] == 512 and R.expect("bound-1024")[1]["max_run"] == 1024
    # the same bytes as text 1 and as text 0: nothing pairs inside text 1, everything pairs in text 0
    a, b = R.expect("as-text-1"), R.expect("as-text-0")
    assert a[1]["pairs"] == 0 and a[0][0] == R.cases()["as-text-1"][0][1] and b[1]["singles"] == 0 and b[1]["pairs"] * 2 == b[1]["records"]
    # /2 in front of /1 in the mixed text: the /1 record still goes to output 1
    o = R.expect("mixed-suffix")[0]
    assert all(P.key(h, 0).endswith(b"/1") for h, _ in P.records(o[1])) and all(P.key(h, 0).endswith(b"/2") for h, _ in P.records(o[2]))
    # the near-miss keys stay apart
    singles = {P.key(h) for h, _ in P.records(R.expect("keys")[0][0])}
    for a, b in R.NEAR:
        for k in (a, b) if a and b else ():
            assert k in R.KEYS or k in singles, (a, b)             # (a key of KEYS has its proper mate in the case)


def test_the_hash():
    h = R.name_hash
    assert len({h(k) for k in (b"", b"\0", b"\0\0", b"a", b"a\0", b"abcdefgh", b"abcdefgh\0", b"abcdefg", b"abcdefg\0")}) == 9
    assert h(b"abc") != h(b"abc", 1) and h(b"abcdefgh12345678") != h(b"12345678abcdefgh")               # the seed; the order of the chunks
    # the library's hash is the model's: 1025 names the model puts into one bucket at one bit are refused there by the library
    texts, opts, code, msg = R.refusals()["1025-one-bucket"]
    with pytest.raises(api.BfqError) as e:
        host.fastq_repair_host(texts, **opts)
    assert msg in str(e.value)
    assert host.fastq_repair_host(texts, hash_bits=1, seed=5)[1].max_run < 1025                           # another seed spreads them


def test_refusals_carry_the_models_message_and_write_nothing():
    for name, (texts, opts, code, msg) in R.refusals().items():
        buf, wins = guarded([sum(len(t) + 1 for t in texts if t is not None)] * 3)
        with pytest.raises(api.BfqError) as e:
            host.fastq_repair_host(texts, outs=wins, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all() and e.value.needed == [0, 0, 0], name


@pytest.mark.parametrize("name", ("filtered-300", "all-three", "groups-mixed"))
def test_a_buffer_one_byte_short(name):
    texts, opts = R.cases()[name]
    want, _ = R.expect(name)
    for short in range(3):
        assert len(want[short])
        buf, wins = guarded([len(w) - (k == short) for k, w in enumerate(want)])
        with pytest.raises(api.BfqError) as e:
            host.fastq_repair_host(texts, outs=wins, **opts)
        assert e.value.code == -1 and e.value.needed == [len(w) for w in want] and (buf == 0xA5).all()


def test_identities():
    # a proper pair of files comes back unchanged
    (_, t1, t2), _ = P.expect_split("wide")
    got, st = host.fastq_repair_host([None, t1, t2])
    assert got[1].tobytes() == t1 and got[2].tobytes() == t2 and len(got[0]) == 0 and st.singles == 0 and st.pairs == 35000
    # repair(shuffle(x)) == repair(x) on the pair outputs, for any shuffle of text 2
    _, f1, f2 = R.cases()["filtered-300"][0]
    want = R.expect("filtered-300")[0]
    recs = [b for _, b in P.records(f2)]
    for seed in (1, 2, 3):
        random.Random(seed).shuffle(recs)
        got, _ = host.fastq_repair_host([None, f1, b"".join(recs)])
        assert [got[1].tobytes(), got[2].tobytes()] == want[1:] and sorted(P.records(got[0].tobytes())) == sorted(P.records(want[0]))
    # the repaired mates merge with their names checked
    for name in ("filtered-300", "mixed-suffix", "mixed-plain", "all-three", "groups", "keys", "wide"):
        texts, opts = R.cases()[name]
        got, st = host.fastq_repair_host(texts, **opts)
        merged, mst = host.fastq_interleave_host([None, got[1], got[2]], check_names=1)
        assert mst.pairs == st.pairs and len(merged) == len(got[1]) + len(got[2]), name
        ins = sorted(b for t in texts if t is not None for _, b in P.records(t if t.endswith(b"\n") else t + b"\n"))
        assert sorted(b for g in got for _, b in P.records(g.tobytes())) == ins, name                 # every record once


def test_symbols_and_options():
    L = _lib.lib()
    for s in ("bfq_repair_default_opts", "bfq_fastq_repair_measure", "bfq_fastq_repair", "bfq_fastq_repair_device", "bfq_fastq_repair_fd", "bfq_fastq_repair_host"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.RepairOpts) == 24 and C.sizeof(_lib.RepairStats) == 96
    o = _lib.RepairOpts(9, 9, 9, (9, 9))
    L.bfq_repair_default_opts(C.byref(o))
    assert (o.mate_suffix, o.hash_bits, o.seed, o.reserved[0], o.reserved[1]) == (1, 40, 0, 0, 0)
    o = api.repair_opts()
    assert (o.mate_suffix, o.hash_bits, o.seed, o.reserved[0], o.reserved[1]) == (1, 40, 0, 0, 0)


def _opt_words(o):
    r = o.get("reserved", (0, 0))
    return "%d %d %d %d %d" % (o.get("mate_suffix", 1), o.get("hash_bits", 40), o.get("seed", 0), r[0], r[1])


def test_repair_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_repair")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_repair.cpp")])
    lines, n, files = [], [0], {}

    def put(data):
        if data is None:
            return "-"
        if data not in files:
            n[0] += 1
            files[data] = str(tmp_path / ("f%d" % n[0]))
            with open(files[data], "wb") as f:
                f.write(data)
        return files[data]

    for name in R.NAMES:
        texts, opts = R.all_cases()[name]
        want, st = R.expect(name)
        lines.append("repair %s %s %s %s %s %s %s %d %d %d %d %d" % (put(texts[0]), put(texts[1]), put(texts[2]), _opt_words(opts), put(want[0]), put(want[1]),
                                                                    put(want[2]), st["pairs"], st["singles"], st["dup_groups"], st["mixed_runs"], st["max_run"]))
    for name, (texts, opts, code, msg) in R.refusals().items():
        lines.append("bad %s %s %s %s %s %d" % (put(texts[0]), put(texts[1]), put(texts[2]), _opt_words(opts), put(msg.encode()), code))
    man = put(("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert b"%d cases, 0 failures" % len(lines) in r.stdout


# ---- parallel.py --repair ---------------------------------------------------------------------------------------------------
from bfqzip_amd import parallel
from tests import util
from tests.test_parallel_gloo import paired_inputs


class ModelRepairEngine(util.OracleEngine):
    """The CPU oracle per block, the model as Engine.fastq_repair_files."""

    def fastq_repair_files(self, texts, dsts, **opts):
        try:
            outs, st = R.repair([None if t is None else open(t, "rb").read() for t in texts], **opts)
        except P.Refused as e:
            for d in dsts:
                if d is not None:
                    open(d, "wb").close()
            raise api.BfqError(e.code, e.msg)
        for d, o in zip(dsts, outs):
            if d is not None:
                open(d, "wb").write(o)
        return st["out_len"], [st["singles"], st["pairs"], st["pairs"]], st

    def close(self):
        pass


def filtered_golden(tmp):
    """the paired golden input with different records lost from each mate file and mate 2 shuffled: (the two paths, the model's repair)"""
    f1, f2 = paired_inputs(tmp)
    a, b = [r for _, r in P.records(open(f1, "rb").read())], [r for _, r in P.records(open(f2, "rb").read())]
    a = [r for k, r in enumerate(a) if k not in (3, 50)]
    b = [r for k, r in enumerate(b) if k not in (7, 50, 99)]
    random.Random(9).shuffle(b)
    g1, g2 = os.path.join(tmp, "thin_R1.fq"), os.path.join(tmp, "thin_R2.fq")
    open(g1, "wb").write(b"".join(a))
    open(g2, "wb").write(b"".join(b))
    want, st = R.repair((None, b"".join(a), b"".join(b)))
    assert st["pairs"] == 96 and st["singles"] == 3
    return (g1, g2), want


def test_driver_repairs_then_runs(orc, tmp_path, monkeypatch, capsys):
    tmp = str(tmp_path)
    os.mkdir(os.path.join(tmp, "o"))
    (g1, g2), want = filtered_golden(tmp)
    monkeypatch.setattr(api, "Engine", lambda dev, **par: ModelRepairEngine(orc, **par))
    out = os.path.join(tmp, "o", "OUT")
    mids = [os.path.join(tmp, "o", "thin_R1_1.fastq"), os.path.join(tmp, "o", "thin_R1_2.fastq")]
    singles = os.path.join(tmp, "o", "thin_R1_singles.fastq")
    assert parallel.main([g1, g2, "-p", "--repair", "-t", "4", "-o", out, "--keep-inflated"]) == 0
    assert [open(m, "rb").read() for m in mids] == want[1:] and open(singles, "rb").read() == want[0]
    got = [open(out + "_%d.fastq" % k, "rb").read() for k in (1, 2)]
    names = parallel.output_names(mids, os.path.join(tmp, "WANT"), True)            # -p on the model's repaired files gives the same bytes
    parallel.run_files(util.OracleEngine(orc, m=5), parallel.Comm(), mids, 4, names, paired=True)
    assert got == [open(n["fastq"], "rb").read() for n in names]
    assert parallel.main([g1, g2, "-p", "--repair", "-t", "4", "-o", out]) == 0    # the intermediates go, the singletons stay
    assert not any(os.path.exists(m) for m in mids) and open(singles, "rb").read() == want[0]
    for args in ([g1, g2, "--repair"], [g1, "-p", "--repair"], [g1, "--repair", "--interleaved"]):
        assert parallel.main(args + ["-o", out, "-t", "2"]) == 1, args
    # a refusal: the library's message before any block runs, nothing left behind
    os.remove(singles)
    for k in (1, 2):
        os.remove(out + "_%d.fastq" % k)
    bad = os.path.join(tmp, "bad.fq")
    open(bad, "wb").write(R.refusals()["1025-equal"][0][0])
    capsys.readouterr()
    assert parallel.main([bad, "--repair", "-o", out, "-t", "2"]) == 1
    assert "more than 1024 records share a name" in capsys.readouterr().err and os.listdir(os.path.join(tmp, "o")) == []
