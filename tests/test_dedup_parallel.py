"""parallel.py --dedup / --dedup-best (CPU): rank 0 removes the duplicates in front of the run -- the model (tests/dedup_model.py)
as Engine.fastq_dedup_files, the CPU oracle per block --, the run goes on with the kept files, the removed records stay beside
the outputs, and a refusal ends the run with the library's message before any block runs."""
import os
import pytest
from bfqzip_amd import api, parallel
from tests import dedup_model as M
from tests import util
from tests.pairs_model import records
from tests.test_parallel_gloo import paired_inputs


class ModelDedupEngine(util.OracleEngine):
    calls = []

    def fastq_dedup_files(self, texts, outs, dups=None, **opts):
        read = lambda p: None if p is None else open(p, "rb").read()
        try:
            kept, removed, st = M.dedup([read(t) for t in texts], **opts)
        except M.Refused as e:
            raise api.BfqError(e.code, e.msg)
        for paths, data in ((outs, kept), (dups or [], removed)):
            for p, d in zip(paths, data):
                if p is not None:
                    open(p, "wb").write(d)
        type(self).calls.append(dict(opts))
        return st["out_len"], st["dup_len"], type("S", (), st)()

    def close(self):
        pass


def _with_duplicates(tmp):
    """the two mates of the paired golden input with records 3, 10 and 3 again appended under other names and qualities"""
    f1, f2 = paired_inputs(tmp)
    outs = []
    for k, f in enumerate((f1, f2)):
        text = open(f, "rb").read()
        recs = [b for _, b in records(text)]
        extra = []
        for j in (3, 10, 3):
            l = recs[j].split(b"\n")
            extra.append(b"\n".join([b"@again%d/%d" % (j, k + 1), l[1], l[2], b"~" * len(l[3]), b""]))
        p = os.path.join(tmp, "dup_%d.fq" % (k + 1))
        open(p, "wb").write(text + b"".join(extra))
        outs.append(p)
    return outs


def _run(orc, inputs, tmp, paired):
    names = parallel.output_names(list(inputs), os.path.join(tmp, "WANT"), paired)
    parallel.run_files(util.OracleEngine(orc, m=5), parallel.Comm(), list(inputs), 4, names, paired=paired)
    return [open(n["fastq"], "rb").read() for n in names]


@pytest.mark.parametrize("paired", (False, True))
def test_driver_dedups_then_runs(orc, tmp_path, monkeypatch, paired):
    tmp = str(tmp_path)
    os.mkdir(os.path.join(tmp, "o"))
    ins = _with_duplicates(tmp)[:2 if paired else 1]
    monkeypatch.setattr(ModelDedupEngine, "calls", [])
    monkeypatch.setattr(api, "Engine", lambda dev, **par: ModelDedupEngine(orc, **par))
    out = os.path.join(tmp, "o", "OUT")
    kept, dups = parallel.dedup_names(ins, out, paired)
    tags = ("_1", "_2") if paired else ("",)
    assert kept == [os.path.join(tmp, "o", "dup_1.dedup%s.fastq" % t) for t in tags] and dups == [os.path.join(tmp, "o", "dup_1.dups%s.fastq" % t) for t in tags]
    for best in (False, True):
        texts = [open(p, "rb").read() for p in ins] + [None] * (2 - len(ins))
        mk, md, st = M.dedup(texts, keep=int(best))
        assert st["removed"] == 3 and (b"@again3/1\n" in mk[0]) == best
        wk = []
        for t, d in zip(tags, mk):                                  # the run on the model's kept texts, written elsewhere
            wk.append(os.path.join(tmp, "want%s.fq" % t))
            open(wk[-1], "wb").write(d)
        want = _run(orc, wk, tmp, paired)
        args = ins + ["--dedup-best" if best else "--dedup", "-t", "4", "-o", out] + (["-p"] if paired else [])
        assert parallel.main(args) == 0
        got = [open(out + t + ".fastq", "rb").read() for t in tags] if paired else [open(out + ".fastq", "rb").read()]
        assert got == want
        assert [open(d, "rb").read() for d in dups] == md[:len(dups)]            # the removed records stay, the kept files are intermediates
        assert not any(os.path.exists(k) for k in kept)
    assert [c["keep"] for c in ModelDedupEngine.calls] == [0, 1]
    assert parallel.main(ins + ["--dedup", "-t", "4", "-o", out, "--keep-inflated"] + (["-p"] if paired else [])) == 0
    assert [open(k, "rb").read() for k in kept] == M.dedup(texts)[0][:len(kept)]


def test_driver_refuses_before_any_block_runs(orc, tmp_path, monkeypatch, capsys):
    tmp = str(tmp_path)
    os.mkdir(os.path.join(tmp, "o"))
    f1, f2 = _with_duplicates(tmp)
    out = os.path.join(tmp, "o", "OUT")
    made = []
    monkeypatch.setattr(api, "Engine", lambda dev, **par: made.append(1) or ModelDedupEngine(orc, **par))
    for args in ([f1, f2, "--dedup"], [f1, "--dedup", "-p"], [f1, f2, "DNA", "--dedup", "--restore"]):
        assert parallel.main(args + ["-o", out, "-t", "2"]) == 1, args
    assert not made and os.listdir(os.path.join(tmp, "o")) == []     # before an engine exists, nothing written
    short = os.path.join(tmp, "short.fq")
    open(short, "wb").write(b"".join(b for _, b in records(open(f2, "rb").read())[:-1]))
    capsys.readouterr()
    assert parallel.main([f1, short, "-p", "--dedup", "-o", out, "-t", "2"]) == 1
    assert "--dedup: " in capsys.readouterr().err.replace("libbfqhip error -1: ", "") and os.listdir(os.path.join(tmp, "o")) == []
