"""The one staging path of the entry points that take plain FASTQ texts (csrc/bfq_texts.h, bfq_io.hip) at the shapes where
their four earlier copies differed: texts of exactly 4095, 4096 and 4097 bytes -- one chunk of the line kernels, less a byte
and plus a byte --, with and without their final LF, on the device at an aligned address and one byte past it, and a text
that is present but empty.  Every device form must equal its host form in bytes and stats; reordering and undoing it must
give the text back.  Every case runs on an Engine of its own, whose arena and text buffer do not exist yet, and once more
on the same Engine."""
import numpy as np
import pytest
from bfqzip_amd import api
from tests.test_gpu_bam_patch import patch_device
from tests.test_gpu_pairs import merge_device, split_device
from tests.test_gpu_pairs_repair import repair_device
from tests.test_gpu_ubam import to_bam_device

pytestmark = pytest.mark.gpu
host = api.HostText

SHAPES = [(total, n, lf) for total, n in ((4095, 2), (4096, 4), (4097, 8)) for lf in (True, False)]
ALIGNS = (0, 1)


def text_of(total, n, lf, mate=0, qual=None, order=None):
    """n records in `total` bytes: read i // 2 of an interleaved text (mate = 0: names r<i>/1, r<i>/2 in turn), or mate 1 / 2
    of read i; one header is padded by a comment to reach the length; lf: with its final LF.  The bases are the same for a
    given (total, n), whatever the rest; qual: one quality for all, else varied; order: the records in another order"""
    rng = np.random.RandomState(total * 16 + n)
    L = (total - 12 * n - 8) // (2 * n)
    recs = []
    for i in range(n):
        name = "r%d/%d" % ((i // 2, 1 + i % 2) if mate == 0 else (i, mate))
        seq = "".join("ACGT"[b] for b in rng.randint(0, 4, L))
        q = (qual * L) if qual else "".join(chr(40 + (7 * i + j) % 30) for j in range(L))
        recs.append([name, seq, q])
    size = lambda: sum(len(a) + 2 * L + 6 for a, _, _ in recs) - (0 if lf else 1)
    pad = total - size()
    assert pad >= 0
    if pad:
        recs[n // 2][0] += " " + "c" * (pad - 1)
    if order is not None:
        recs = [recs[i] for i in order]
    text = "".join("@%s\n%s\n+\n%s\n" % tuple(r) for r in recs).encode()
    text = text if lf else text[:-1]
    assert len(text) == total
    return text


def outcome(call):
    """what a call gave, or the code and words it refused with (behind the entry point's name)"""
    try:
        return ("ok",) + tuple(call())
    except api.BfqError as e:
        return ("refused", e.code, str(e).split(": ", 1)[-1])


def on_a_fresh_engine(run):
    e = api.Engine(0)
    try:
        first = run(e)
        assert run(e) == first
    finally:
        e.close()


@pytest.mark.parametrize("total,n,lf", SHAPES)
def test_to_bam_and_patch(total, n, lf):
    text = text_of(total, n, lf)
    edited = text_of(total, n, lf, qual="5")
    want, wst = host.fastq_to_bam_host([text, None, None])
    pwant, pst = host.bam_patch_host(want.tobytes(), [edited, None, None])
    assert pst.quals_changed > 0
    blob = host.bgzf_deflate_model(want.tobytes(), 1).tobytes()     # the BAM file fastq_to_bam makes of the text (checked below)
    for align in ALIGNS:
        def run(e):
            got, st = to_bam_device(e, [text, None, None], len(want), align=align)
            assert got == want.tobytes() and st.as_dict() == wst.as_dict(), (total, lf, align)
            return got

        def run_patch(e):                                           # (the first call of its Engine)
            got, st = patch_device(e, blob, [edited, None, None], len(want), align=align)
            assert got == pwant.tobytes() and st.as_dict() == pst.as_dict(), (total, lf, align)
            return got
        on_a_fresh_engine(run)
        on_a_fresh_engine(run_patch)

    def run_file(e):
        got = e.fastq_to_bam([text, None, None])[0].tobytes()
        assert got == blob, (total, lf)
        return got
    on_a_fresh_engine(run_file)


@pytest.mark.parametrize("total,n,lf", SHAPES)
def test_split_merge_repair(total, n, lf):
    inter = text_of(total, n, lf)
    mates = [None, text_of(total, n, lf, mate=1), text_of(total, n, not lf, mate=2)]
    repair_in = mates[:2] + [text_of(total, n, not lf, mate=2, order=list(range(n))[::-1])]     # the second file the other way round
    swant, sst = host.fastq_deinterleave_host(inter)
    mwant, mst = host.fastq_interleave_host(mates)
    rwant, rst = host.fastq_repair_host(repair_in)
    sst, mst, rst = sst.as_dict(), mst.as_dict(), rst.as_dict()
    assert sst["pairs"] == n // 2 and mst["pairs"] == n and rst["pairs"] == n
    for align in ALIGNS:
        def run(e):
            got, nr, st = split_device(e, inter, list(sst["out_len"]), align=align)
            assert got == [w.tobytes() for w in swant] and st.as_dict() == sst, (total, lf, align)
            return got

        def run_merge(e):
            got, st = merge_device(e, mates, len(mwant), align=align)
            assert got == mwant.tobytes() and st.as_dict() == mst, (total, lf, align)
            return got

        def run_repair(e):
            got, nr, st = repair_device(e, repair_in, list(rst["out_len"]), align=align)
            assert got == [w.tobytes() for w in rwant] and st.as_dict() == rst, (total, lf, align)
            return got
        for r in (run, run_merge, run_repair):
            on_a_fresh_engine(r)


@pytest.mark.parametrize("total,n,lf", SHAPES)
def test_reorder_and_back(total, n, lf):
    text = text_of(total, n, lf)
    whole = text if lf else text + b"\n"
    two = [text, text_of(total, n, not lf, mate=2)]

    def run(e):
        out, perm = e.fastq_reorder([text], keep=True)
        assert len(out[0]) == len(whole) and sorted(out[0].tobytes().split(b"\n")) == sorted(whole.split(b"\n"))
        back = e.fastq_unreorder(out, perm)
        assert [b.tobytes() for b in back] == [whole], (total, lf)
        return out[0].tobytes(), perm.tobytes()

    def run_mates(e):
        out, perm = e.fastq_reorder(two, mode=1, seed=5, keep=True)
        back = e.fastq_unreorder(out, perm)
        assert [b.tobytes() for b in back] == [t if t.endswith(b"\n") else t + b"\n" for t in two], (total, lf)
        return [o.tobytes() for o in out]
    on_a_fresh_engine(run)
    on_a_fresh_engine(run_mates)


def test_a_text_that_is_present_but_empty():
    """beside texts that are not: no reads of its own in the uBAM and in the patch, no records in the merge and the repair"""
    mates = [b"", text_of(4096, 4, True, mate=1), text_of(4097, 4, False, mate=2)]
    wants = [outcome(lambda: dicts_of(host.fastq_to_bam_host(mates))), outcome(lambda: dicts_of(host.fastq_interleave_host(mates))),
             outcome(lambda: dicts_of(host.fastq_repair_host(mates)))]
    assert [w[0] for w in wants] == ["ok"] * 3
    stream = host.fastq_to_bam_host(mates)[0]
    pwant = outcome(lambda: dicts_of(host.bam_patch_host(stream, mates)))
    blob = host.bgzf_deflate_model(stream.tobytes(), 1).tobytes()
    cap = sum(len(m) + 1 for m in mates)
    for align in ALIGNS:
        calls = [lambda e: to_bam_device(e, mates, len(stream), align=align), lambda e: merge_device(e, mates, cap, align=align),
                 lambda e: repair_device(e, mates, [cap] * 3, align=align)[::2], lambda e: patch_device(e, blob, mates, len(stream), align=align)]
        for call, want in zip(calls, wants + [pwant]):
            def run(e):
                got = outcome(lambda: dicts_of(call(e)))
                assert got == want, align
                return got
            on_a_fresh_engine(run)


def dicts_of(result):
    """(bytes, stats as a dictionary) of what a form returned: (text or texts, stats)"""
    data, st = result
    data = [d if isinstance(d, bytes) else d.tobytes() for d in data] if isinstance(data, (list, tuple)) else (data if isinstance(data, bytes) else data.tobytes())
    return data, st.as_dict()
