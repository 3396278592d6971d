"""CPU tests of the way back from a reordering: the BFQPERM1 container as the library states it on the host (bfq_perm_bound /
_reads / _encode / _decode) against the restatement of the header's words (tests/perm_model.py), byte for byte, every refusal
with its first offending position, the same arithmetic as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/cxx/test_perm.cpp), and `parallel.py --reorder 2 --keep-order` with the CPU oracle as the per-block engine
and the models as its fastq_reorder_files / fastq_unreorder_files.  No GPU in this tier; tests/test_gpu_unreorder.py pins the
kernels to the same models."""
import ctypes as C
import os, subprocess
import numpy as np
import pytest
from bfqzip_amd import _lib, api, parallel
from tests import perm_model as pm, reorder_model as model, util
from tests.test_parallel_gloo import EXAMPLE, paired_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 3, 4, 5, 64, 65] + [x for m in (16, 17) for x in (1 << m, (1 << m) + 1)] + [1_000_003]   # (2^6, 2^6 + 1 are 64, 65)
NOPOS = (1 << 64) - 1


def test_widths_of_the_model():
    """The model's own arithmetic, by hand: w is the bit length of N - 1, 1 up to N = 2; the lengths follow."""
    assert [pm.width(n) for n in (0, 1, 2, 3, 4, 5, 64, 65, 1 << 16, (1 << 16) + 1, 1_000_003)] == [1, 1, 1, 2, 2, 3, 6, 7, 16, 17, 20]
    assert [pm.bound(n) for n in (0, 1, 2, 3, 64, 65, 1_000_003)] == [40, 48, 48, 48, 40 + 48, 40 + 64, 40 + 8 * 312501]
    # perm = [2, 0, 1], w = 2: bits 10 | 00 << 2 | 01 << 4 = 0b010010
    z = pm.encode([2, 0, 1], opts=dict(mode=2, k=21, seed=7))
    assert z == b"BFQPERM1" + (3).to_bytes(8, "little") + (2).to_bytes(4, "little") + (2).to_bytes(4, "little") + \
        (21).to_bytes(4, "little") + bytes(4) + (7).to_bytes(8, "little") + (0b010010).to_bytes(8, "little")
    assert pm.decode(z) == ([2, 0, 1], dict(mode=2, k=21, seed=7))


@pytest.mark.parametrize("N", SIZES)
def test_host_functions_equal_the_model(N):
    rng = np.random.default_rng(N)
    perms = [np.arange(N, dtype=np.uint64), np.arange(N, dtype=np.uint64)[::-1].copy(), rng.permutation(N).astype(np.uint64)]
    if N <= 65:
        perms += [rng.permutation(N).astype(np.uint64) for _ in range(5)]
    assert api.perm_bound(N) == pm.bound(N)
    for i, p in enumerate(perms):
        opts = dict(mode=1 + i % 2, k=(0, 21, 32)[i % 3], seed=int(rng.integers(0, 1 << 63)) * 2 + 1)
        want = pm.encode(p, opts=opts)
        z = api.perm_encode(p, **opts)
        assert len(z) == pm.bound(N) and z.tobytes() == want
        assert api.perm_reads(z) == N
        got, o = api.perm_decode(want)
        assert np.array_equal(got, p) and o == opts
        if N <= 1 << 17 or i == 2:
            mp, mo = pm.decode(z)
            assert mp == [int(x) for x in p] and mo == opts


def _decode_raw(z, room=None):
    """bfq_perm_decode on raw bytes with sentinels in every output: (rc, first_bad, outputs untouched)."""
    L = _lib.lib()
    a = np.frombuffer(bytes(z), np.uint8) if len(z) else np.zeros(0, np.uint8)
    n = room if room is not None else 64
    out = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    N, bad = C.c_uint64(77), C.c_uint64(5)
    O = _lib.ReorderOpts(mode=-3, k=-4, seed=99)
    rc = L.bfq_perm_decode(api._ptr(a) if len(a) else None, len(a), api._ptr(out), n, C.byref(N), C.byref(O), C.byref(bad))
    clean = bool((out == 0xA5A5A5A5A5A5A5A5).all()) and N.value == 77 and (O.mode, O.k, O.seed) == (-3, -4, 99)
    return rc, bad.value, clean


def _poke(z, j, v):
    """The container with entry j overwritten (through the model's layout: one little-endian integer)."""
    w = int.from_bytes(z[16:20], "little")
    big = int.from_bytes(z[pm.HDR:], "little")
    big = (big & ~(((1 << w) - 1) << (j * w))) | (v << (j * w))
    return z[:pm.HDR] + big.to_bytes(len(z) - pm.HDR, "little")


def test_refusals_name_the_first_offending_position():
    p = [(i * 7 + 3) % 37 for i in range(37)]                       # w = 6: 222 bits, 34 padding bits
    good = pm.encode(p)
    assert _decode_raw(good) == (0, NOPOS, False)
    cases = {
        "magic": (good[:7] + b"2" + good[8:], None),
        "w + 1": (good[:16] + bytes([7]) + good[17:], None),
        "w - 1": (good[:16] + bytes([5]) + good[17:], None),
        "length + 8": (good + bytes(8), None),
        "length - 8": (good[:-8], None),
        "shorter than its header": (good[:39], None),
        "empty": (b"", None),
        "last padding bit": (good[:-1] + bytes([good[-1] | 0x80]), None),
        "first padding bit": (_poke(good + b"", 37, 1), None),
        "entry == N": (_poke(good, 20, 37), 20),
        "last entry out of range": (_poke(good, 36, 63), 36),
        "a value twice": (_poke(good, 30, p[4]), 30),
        "a value twice, seen from the earlier entry": (_poke(good, 4, p[30]), 30),
        "two faults": (_poke(_poke(good, 9, 40), 3, p[2]), 3),
    }
    for name, (z, want) in cases.items():
        with pytest.raises(ValueError) as e:                        # the model refuses the same container for the same reason
            pm.decode(z)
        assert e.value.args[0] == want, name
        rc, bad, clean = _decode_raw(z)
        assert (rc, bad, clean) == (-1, NOPOS if want is None else want, True), name
        assert api.perm_reads(z) == (-1 if want is None else 37), name
        with pytest.raises(api.PermError) as e:
            api.perm_decode(z)
        assert e.value.code == -1 and e.value.first_bad == want, name
    # room for fewer entries than the container has: refused, nothing written
    assert _decode_raw(good, room=36) == (-1, NOPOS, True)
    # encode: not a permutation, or no room -- nothing written
    L = _lib.lib()
    for q in ([0, 1, 5, 3, 4], [0, 1, 2, 1, 4]):
        a = np.array(q, np.uint64)
        out = np.full(64, 0xEE, np.uint8)
        ol = C.c_uint64(3)
        assert L.bfq_perm_encode(api._ptr(a), 5, None, api._ptr(out), 64, C.byref(ol)) == -1 and ol.value == 3 and (out == 0xEE).all()
        with pytest.raises(api.PermError):
            api.perm_encode(a)
    a = np.arange(37, dtype=np.uint64)
    out = np.full(len(good), 0xEE, np.uint8)
    assert L.bfq_perm_encode(api._ptr(a), 37, None, api._ptr(out), len(good) - 1, None) == -1 and (out == 0xEE).all()
    assert L.bfq_perm_encode(api._ptr(a), 37, None, api._ptr(out), len(good), None) == 0 and out.tobytes() == pm.encode(a)
    assert api.perm_bound(1 << 56) == 0 and api.perm_bound((1 << 56) - 1) == 40 + 8 * (((1 << 56) - 1) * 56 + 63 >> 6)


def test_container_program_under_sanitizers(tmp_path):
    """tests/cxx/test_perm.cpp: bfq_perm.h compiled for the host with -fsanitize=address,undefined and run as a program of its
    own -- exact-size heap buffers, so a byte read or written beside the container or the permutation ends the run."""
    exe = str(tmp_path / "test_perm")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_perm.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_model_unreorder_undoes_the_model_reorder():
    text = b"@a x\r\nACGTACGTAC\r\n+a x\r\nIIIIIIIIII\r\n@b\nNNNN\n+\nIIII\n@c\nAAAAAAAAAA\n+\nIIIIIIIIII"
    (out,), perm = model.reorder([text], k=8)
    assert list(perm) == [2, 0, 1]
    assert pm.unreorder([out], perm) == [text + b"\n"]
    assert pm.unreorder([out[:-1]], perm) == [text + b"\n"]         # the final newline is supplied
    recs = [b"@0\nA\n+\nI\n", b"@1\n\n+\n\n", b"@2\nCC\n+\nII\n"]
    # output record perm[j] = input record j
    assert pm.unreorder([b"".join(recs)], [1, 2, 0]) == [recs[2] + recs[0] + recs[1]]
    with pytest.raises(ValueError):
        pm.unreorder([b"".join(recs)], [1, 0])


# ---- parallel.py --reorder 2 --keep-order -------------------------------------------------------------------------------------
class ModelKeepEngine(util.OracleEngine):
    """The CPU oracle per block; the numpy models as Engine.fastq_reorder_files(perm_path=) / fastq_unreorder_files."""

    def fastq_reorder_files(self, inputs, outputs, mode=2, k=21, seed=0, perm_path=None):
        outs, perm = model.reorder([open(p, "rb").read() for p in inputs], mode=mode, k=k, seed=seed)
        for p, o in zip(outputs, outs):
            open(p, "wb").write(o)
        if perm_path is not None:
            open(perm_path, "wb").write(pm.encode(perm, opts=dict(mode=mode, k=k, seed=seed)))
        return [len(o) for o in outs], len(perm)

    def fastq_unreorder_files(self, inputs, outputs, perm_path):
        perm, _ = pm.decode(open(perm_path, "rb").read())
        outs = pm.unreorder([open(p, "rb").read() for p in inputs], perm)
        for p, o in zip(outputs, outs):
            open(p, "wb").write(o)
        return [len(o) for o in outs], len(perm)

    def close(self):
        pass


@pytest.mark.parametrize("paired", [False, True])
def test_driver_keeps_the_order(orc, tmp_path, monkeypatch, paired):
    """`parallel.py IN [IN2 -p] -t 4 --reorder 2 --keep-order`: the .perm file beside the first intermediate decodes to the
    model's permutation, the merged outputs are those of the same run without the flag with their records un-reordered, and
    nothing else is left behind; without the flag no .perm file appears."""
    tmp = str(tmp_path)
    if paired:
        inputs = list(paired_inputs(tmp))
    else:
        inputs = [os.path.join(tmp, "in.fastq")]
        open(inputs[0], "wb").write(open(EXAMPLE, "rb").read())
    monkeypatch.setattr(api, "Engine", lambda dev, **par: ModelKeepEngine(orc, **par))
    flags = (["-p"] if paired else []) + ["-t", "4", "--reorder", "2"]
    permfile = parallel.reordered_names(inputs, 2)[0] + ".perm"
    assert permfile == os.path.splitext(inputs[0])[0] + ".reordered" + os.path.splitext(inputs[0])[1] + ".perm"
    assert parallel.main(inputs + flags + ["-o", os.path.join(tmp, "RUN")]) == 0
    assert not os.path.exists(permfile)
    assert parallel.main(inputs + ["--keep-order"] + flags + ["-o", os.path.join(tmp, "KEPT"), "-v", "1"]) == 0
    _, wperm = model.reorder([open(p, "rb").read() for p in inputs])
    perm, opts = pm.decode(open(permfile, "rb").read())
    assert perm == [int(x) for x in wperm] and opts == dict(mode=2, k=21, seed=0)
    assert perm != sorted(perm)
    tag = ["_1.fastq", "_2.fastq"] if paired else [".fastq"]
    run = [open(os.path.join(tmp, "RUN" + t), "rb").read() for t in tag]
    kept = [open(os.path.join(tmp, "KEPT" + t), "rb").read() for t in tag]
    assert kept == pm.unreorder(run, perm) and kept != run
    # record i of the result is read i of the input again (the oracle keeps no header: compare the read lengths)
    for k_, src in zip(kept, inputs):
        assert [len(x) for x in k_.split(b"\n")[1::4]] == [len(x) for x in open(src, "rb").read().split(b"\n")[1::4]]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("KEPT")) == sorted("KEPT" + t for t in tag)   # no temporary left
    # --keep-order without --reorder does nothing
    os.remove(permfile)
    assert parallel.main(inputs + ["--keep-order"] + (["-p"] if paired else []) + ["-t", "4", "-o", os.path.join(tmp, "PLAIN")]) == 0
    assert not os.path.exists(permfile) and not [f for f in os.listdir(tmp) if f.endswith(".perm")]
    # raw streams stay in run order, the merged text comes back
    assert parallel.main(inputs + ["--keep-order", "--m2"] + flags + ["-o", os.path.join(tmp, "M2")]) == 0
    assert parallel.main(inputs + ["--m2"] + flags + ["-o", os.path.join(tmp, "M2R")]) == 0
    for t in tag:
        assert open(os.path.join(tmp, "M2" + t), "rb").read() == kept[tag.index(t)]
        assert open(os.path.join(tmp, "M2" + t + ".dna"), "rb").read() == open(os.path.join(tmp, "M2R" + t + ".dna"), "rb").read()


def test_reorder_inputs_passes_perm_path_only_when_asked(orc, tmp_path):
    """An engine whose fastq_reorder_files does not know perm_path keeps working without --keep-order."""
    calls = []

    class Plain(util.OracleEngine):
        def fastq_reorder_files(self, inputs, outputs, mode=2, k=21, seed=0):
            calls.append((tuple(inputs), tuple(outputs)))
            for o in outputs:
                open(o, "wb").close()
            return [0] * len(outputs), 0

    f = str(tmp_path / "a.fq")
    open(f, "wb").write(open(EXAMPLE, "rb").read())
    assert parallel.reorder_inputs(Plain(orc, m=5), parallel.Comm(), [f], 2) == [str(tmp_path / "a.reordered.fq")]
    with pytest.raises(TypeError):
        parallel.reorder_inputs(Plain(orc, m=5), parallel.Comm(), [f], 2, perm_path=str(tmp_path / "p.perm"))
    assert len(calls) == 1
    eng = ModelKeepEngine(orc, m=5)
    parallel.reorder_inputs(eng, parallel.Comm(), [f], 2, perm_path=str(tmp_path / "p.perm"))
    assert pm.decode(open(str(tmp_path / "p.perm"), "rb").read())[0] == [int(x) for x in model.reorder([open(f, "rb").read()])[1]]
