"""CPU tests of the read reordering: the key as the library states it on the host (bfq_reorder_key) against the numpy
restatement of the interface (tests/reorder_model.py), and `parallel.py --reorder` -- intermediate file names of the
reference (BFQzip_parallel.py:398,421), output names that follow the replaced inputs, only rank 0 writes -- with the CPU
oracle as the per-block engine and the model as its fastq_reorder_files.  No GPU in this tier; tests/test_gpu_reorder.py
pins the kernels to the same model."""
import hashlib, os, sys
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import reorder_model as model, util
from tests.test_parallel_gloo import EXAMPLE, paired_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fmix64_int(x):
    """The finaliser once more on Python integers (no numpy): the known answers below are made with it."""
    M = (1 << 64) - 1
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M
    x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M
    return x ^ (x >> 33)


def test_known_keys():
    assert api.reorder_key(b"AAAAAAAA", 8) == 0                                  # x = 0, fmix64(0) = 0
    assert api.reorder_key(b"AAAAAAAC", 8) == _fmix64_int(1) >> 24               # C = 1 in the lowest two bits
    assert api.reorder_key(b"TAAAAAAA", 8) == _fmix64_int(3 << 14) >> 24         # first base most significant
    # two windows: the smaller hash wins
    assert api.reorder_key(b"AAAAAAACG", 8) == min(_fmix64_int(1), _fmix64_int(6)) >> 24
    # 21 bases = one window of the default k; one base less, an N or a lower-case letter inside: no window
    x = 0
    for c in b"ACGTACGTACGTACGTACGTA":
        x = x << 2 | b"ACGT".index(c)
    assert api.reorder_key(b"ACGTACGTACGTACGTACGTA") == _fmix64_int(x) >> 24 == 952589878535
    for s in (b"ACGTACGTACGTACGTACGT", b"ACGTACGTACNTACGTACGTA", b"ACGTACGTACgTACGTACGTA", b""):
        assert api.reorder_key(s) == model.NOKEY == (1 << 40) - 1
    assert api.reorder_key(b"ACGTACGTACNTACGTACGTA", 8) != model.NOKEY            # ... but windows of 8 on either side
    # k = 32 fills the 64 bits
    assert api.reorder_key(b"T" * 32, 32) == _fmix64_int((1 << 64) - 1) >> 24
    for k in (7, 33, 0, -1):
        assert api.reorder_key(b"ACGT" * 20, k) == (1 << 64) - 1                  # k outside 8..32


@pytest.mark.parametrize("k", [8, 21, 32])
@pytest.mark.parametrize("p_other", [0.0, 0.05, 0.5])
def test_key_equals_model_on_random_sequences(k, p_other):
    rng = np.random.default_rng(1000 * k + int(100 * p_other))
    alphabet = np.frombuffer(b"ACGTNacgt", np.uint8)
    p = np.array([(1 - p_other) / 4] * 4 + [p_other / 2] + [p_other / 8] * 4)
    seqs = [b"", b"A" * (k - 1), b"C" * k]
    for L in list(range(0, 70)) + [int(x) for x in rng.integers(70, 301, 130)]:
        seqs.append(alphabet[rng.choice(9, L, p=p)].tobytes())
    for s in seqs:
        assert api.reorder_key(s, k) == model.key_of(s, k), (s, k)
    # ... and the vectorised form of the model the GPU tests use
    text = b"".join(b"@%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    a, _, _, st, ln = model.records(text)
    keys, found = model.locus_keys(a, st, ln, k)
    assert [int(x) for x in keys] == [api.reorder_key(s, k) for s in seqs]
    assert [bool(f) for f in found] == [any(all(c in b"ACGT" for c in s[i:i + k]) for i in range(len(s) - k + 1)) for s in seqs]


def test_model_moves_records_verbatim():
    text = b"@a x\r\nACGTACGTAC\r\n+a x\r\nIIIIIIIIII\r\n@b\nNNNN\n+\nIIII\n@c\nAAAAAAAAAA\n+\nIIIIIIIIII"
    (out,), perm = model.reorder([text], k=8)
    recs = [b"@a x\r\nACGTACGTAC\r\n+a x\r\nIIIIIIIIII\r\n", b"@b\nNNNN\n+\nIIII\n", b"@c\nAAAAAAAAAA\n+\nIIIIIIIIII\n"]
    assert list(perm) == [2, 0, 1] and out == recs[2] + recs[0] + recs[1]          # fmix64(0) = 0 first, no window last
    m1 = b"@1\nNNNNNNNN\n+\nIIIIIIII\n@2\nAAAAAAAA\n+\nIIIIIIII\n"
    m2 = b"@1\nAAAAAAAA\n+\nIIIIIIII\n@2\nNN\n+\nII\n"
    (o1, o2), perm = model.reorder([m1, m2], k=8)                                  # mate 2 lends its key; ties in input order
    assert list(perm) == [0, 1] and (o1, o2) == (m1, m2)
    a, b = model.reorder([text], mode=1, seed=1), model.reorder([text], mode=1, seed=1)
    assert a[0] == b[0] and sorted(a[1]) == [0, 1, 2]


# ---- parallel.py --reorder ------------------------------------------------------------------------------------------------
class ModelReorderEngine(util.OracleEngine):
    """The CPU oracle per block, the numpy model as Engine.fastq_reorder_files; every call leaves a line in `journal`."""
    journal = None

    def fastq_reorder_files(self, inputs, outputs, mode=2, k=21, seed=0):
        outs, perm = model.reorder([open(p, "rb").read() for p in inputs], mode=mode, k=k, seed=seed)
        for p, o in zip(outputs, outs):
            open(p, "wb").write(o)
        if self.journal:
            with open(self.journal, "a") as f:
                f.write("rank %s: %s\n" % (os.environ.get("RANK", "0"), " ".join(outputs)))
        return [len(o) for o in outs], len(perm)

    def close(self):
        pass


def _expected(orc, inputs, t, out, paired, tmp, mode=2, **kw):
    """run_files on the model-reordered text, written elsewhere: the bytes the --reorder run must give."""
    texts, _ = model.reorder([open(p, "rb").read() for p in inputs], mode=mode, **kw)
    srcs = []
    for i, tx in enumerate(texts):
        srcs.append(os.path.join(tmp, "want_in_%d%s" % (i, os.path.splitext(inputs[i])[1])))
        open(srcs[-1], "wb").write(tx)
    names = parallel.output_names(srcs, os.path.join(tmp, "WANT"), paired)
    parallel.run_files(util.OracleEngine(orc, m=5), parallel.Comm(), srcs, t, names, paired=paired)
    return texts, [open(n["fastq"], "rb").read() for n in names]


@pytest.mark.parametrize("paired", [False, True])
def test_driver_reorders_then_runs(orc, tmp_path, monkeypatch, paired):
    """`parallel.py IN [IN2 -p] -t 4 --reorder 2`, once with -o and once without: the intermediates carry the reference's
    names and the model's bytes, the merged outputs are named after the REPLACED inputs and equal the plain run on them."""
    tmp = str(tmp_path)
    if paired:
        inputs = list(paired_inputs(tmp))
    else:
        inputs = [os.path.join(tmp, "in.fastq")]
        open(inputs[0], "wb").write(open(EXAMPLE, "rb").read())
    journal = os.path.join(tmp, "journal")
    monkeypatch.setattr(ModelReorderEngine, "journal", journal)
    monkeypatch.setattr(api, "Engine", lambda dev, **par: ModelReorderEngine(orc, **par))
    texts, want = _expected(orc, inputs, 4, "", paired, tmp)
    flags = ["-p"] if paired else []
    assert parallel.main(inputs + flags + ["-t", "4", "--reorder", "2", "-o", os.path.join(tmp, "OUT")]) == 0
    mids = [os.path.splitext(p)[0] + ".reordered" + os.path.splitext(p)[1] for p in inputs]
    assert [open(m, "rb").read() for m in mids] == texts
    assert texts[0] != open(inputs[0], "rb").read() and sorted(texts[0].split(b"\n")) == sorted(open(inputs[0], "rb").read().split(b"\n"))
    outs = [os.path.join(tmp, "OUT_1.fastq"), os.path.join(tmp, "OUT_2.fastq")] if paired else [os.path.join(tmp, "OUT.fastq")]
    assert [open(o, "rb").read() for o in outs] == want
    # without -o the names come from the replaced inputs (define_basename after the replacement): <root>.reordered.cat<ext>
    assert parallel.main(inputs + flags + ["-t", "4", "--reorder", "2"]) == 0
    cats = [os.path.splitext(m)[0] + ".cat" + os.path.splitext(m)[1] for m in mids]
    assert [open(o, "rb").read() for o in cats] == want
    assert not os.path.exists(os.path.splitext(inputs[0])[0] + ".cat.fastq")
    # mode 1: <root>.random<ext>, seeded
    _, want1 = _expected(orc, inputs, 4, "", paired, tmp, mode=1, seed=7)
    assert parallel.main(inputs + flags + ["-t", "4", "--reorder", "1", "--seed", "7", "-o", os.path.join(tmp, "RND")]) == 0
    assert all(os.path.exists(os.path.splitext(p)[0] + ".random" + os.path.splitext(p)[1]) for p in inputs)
    rnd = [os.path.join(tmp, "RND_1.fastq"), os.path.join(tmp, "RND_2.fastq")] if paired else [os.path.join(tmp, "RND.fastq")]
    assert [open(o, "rb").read() for o in rnd] == want1
    assert len(open(journal).read().splitlines()) == 3
    # the default changes nothing: no intermediate, the plain run's output
    for m in mids:
        os.remove(m)
    assert parallel.main(inputs + flags + ["-t", "4", "-o", os.path.join(tmp, "PLAIN")]) == 0
    assert not any(os.path.exists(m) for m in mids)
    plain = parallel.output_names(inputs, os.path.join(tmp, "P2"), paired)
    parallel.run_files(util.OracleEngine(orc, m=5), parallel.Comm(), inputs, 4, plain, paired=paired)
    got = [os.path.join(tmp, "PLAIN_1.fastq"), os.path.join(tmp, "PLAIN_2.fastq")] if paired else [os.path.join(tmp, "PLAIN.fastq")]
    assert [open(o, "rb").read() for o in got] == [open(n["fastq"], "rb").read() for n in plain]


def test_reorder_inputs_contract(orc, tmp_path):
    eng = ModelReorderEngine(orc, m=5)
    f = str(tmp_path / "a.b.fq")
    open(f, "wb").write(open(EXAMPLE, "rb").read())
    assert parallel.reorder_inputs(eng, parallel.Comm(), [f], 0) == [f]
    assert parallel.reorder_inputs(eng, parallel.Comm(), [f], 2, k=16) == [str(tmp_path / "a.b.reordered.fq")]
    assert open(str(tmp_path / "a.b.reordered.fq"), "rb").read() == model.reorder([open(f, "rb").read()], k=16)[0][0]
    assert parallel.reorder_inputs(eng, parallel.Comm(), [f], 1, seed=3) == [str(tmp_path / "a.b.random.fq")]
    with pytest.raises(ValueError):
        parallel.reorder_inputs(eng, parallel.Comm(), [f], 3)
    assert parallel.reordered_names(["x/r_1.fastq", "x/r_2.fastq"], 1) == ["x/r_1.random.fastq", "x/r_2.random.fastq"]   # BFQzip_parallel.py:421


def _worker(rank, world, port, paired, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import orc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = parallel.Comm(dist)
    ModelReorderEngine.journal = os.path.join(tmp, "journal2")
    eng = ModelReorderEngine(orc, m=5)
    try:
        inputs = [os.path.join(tmp, "r1.fastq"), os.path.join(tmp, "r2.fastq")] if paired else [os.path.join(tmp, "in.fastq")]
        new = parallel.reorder_inputs(eng, comm, inputs, 2, paired=paired)
        names = parallel.output_names(new, os.path.join(tmp, "G"), paired)
        parallel.run_files(eng, comm, new, 4, names, paired=paired)
        if rank == 0:
            q.put("|".join(new + [hashlib.md5(open(n["fastq"], "rb").read()).hexdigest() for n in names]))
    except Exception as e:                                     # surface the failure instead of a queue timeout
        q.put(f"rank {rank}: {type(e).__name__}: {e}")
        raise
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("paired", [False, True])
def test_two_ranks_gloo_reorder(orc, tmp_path, paired):
    """2 ranks: rank 0 alone writes the intermediate, both run on it after the barrier."""
    import torch.multiprocessing as mp
    tmp = str(tmp_path)
    if paired:
        inputs = list(paired_inputs(tmp))
    else:
        inputs = [os.path.join(tmp, "in.fastq")]
        open(inputs[0], "wb").write(open(EXAMPLE, "rb").read())
    texts, want = _expected(orc, inputs, 4, "", paired, tmp)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32600 + (os.getpid() * 7 + int(paired)) % 2000
    ps = [ctx.Process(target=_worker, args=(rk, 2, port, paired, tmp, q)) for rk in range(2)]
    for p in ps:
        p.start()
    got = q.get(timeout=180)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0, got
    mids = [os.path.splitext(p)[0] + ".reordered" + os.path.splitext(p)[1] for p in inputs]
    assert got.split("|") == mids + [hashlib.md5(w).hexdigest() for w in want]
    assert [open(m, "rb").read() for m in mids] == texts
    lines = open(os.path.join(tmp, "journal2")).read().splitlines()
    assert lines == ["rank 0: " + " ".join(mids)]
