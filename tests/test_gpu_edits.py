"""GPU tests of the base edits (BFQEDIT1: bfq_fastq_edits*, bfq_fastq_unedit*, bfq_edits_make_device / _apply_device,
bfq_fastq_run_job_edits, bfq_fastq_restore_edited, dropin/bfq_edits, bfq_restore -E, parallel.py --keep-bases): the device's
container equals the model's (tests/edits_model.py) byte for byte, the way back gives the input's bases, and every refusal
leaves sentinel-filled outputs untouched."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import edits_model as em, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dropin", "bfq_edits")
RESTORE = os.path.join(ROOT, "dropin", "bfq_restore")
NAMES = ("example", "paired", "synth_fix", "synth_var")
GOLDEN_EDITS = {"example": 10, "paired": 0, "synth_fix": 429, "synth_var": 598}
SENT = 0xA5
MODES = {"fused": 0, "piles": 1, "capped": 2}                    # bfq_params.piles


def _raw(name, ext=".fastq"):
    return open(os.path.join(util.GOLDEN, name + ext), "rb").read()


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0, m=5)                                        # the flags of the goldens' "M2B0 -m 5"
    yield e
    e.close()


def sentinel(n):
    return np.full(n, SENT, np.uint8)


def seq_lines(text):
    return bytes(text).split(b"\n")[1::4]


def qual_lines(text):
    return bytes(text).split(b"\n")[3::4]


# ---- model-made pairs -----------------------------------------------------------------------------------------------------
def text_of(seqs, eol=b"\n", final=True, hdr=lambda i: b"@r%d" % i):
    t = b"".join(hdr(i) + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))
    return t if final else t[:len(t) - len(eol)]


def random_seqs(rng, lens):
    return [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(l))) for l in lens]


def mutated(seqs, where):
    """where: {read: [positions]}; a changed base becomes another letter"""
    out = [bytearray(s) for s in seqs]
    for r, ps in where.items():
        for p in ps:
            out[r][p] = ord("C") if out[r][p] == ord("A") else ord("A")
    return [bytes(s) for s in out]


def pair_edge_lengths(rng):
    """read lengths 0, 1, 7, 8, 9, 127, 128, 129, 300 twice over; edits at the first and the last base of every read (so of the
    collection), around every 8-byte word border and 128-base sweep border, and one read changed entirely"""
    lens = [0, 1, 7, 8, 9, 127, 128, 129, 300, 300, 129, 128, 127, 9, 8, 7, 1, 0, 65, 64]
    seqs = random_seqs(rng, lens)
    where = {}
    for r, l in enumerate(lens):
        ps = {p for p in (0, l - 1, 7, 8, 9, 15, 16, 120, 127, 128, 129, 135, 136, 255, 256, 257, l - 8, l - 9) if 0 <= p < l}
        where[r] = sorted(ps)
    where[9] = list(range(300))
    return seqs, mutated(seqs, where)


def pair_with_E(rng, E):
    """400 reads of 20..90 bases with exactly E changed bases"""
    lens = rng.integers(20, 91, 400)
    seqs = random_seqs(rng, lens)
    total = int(lens.sum())
    g = np.sort(rng.choice(total, E, replace=False))
    off = np.concatenate([[0], np.cumsum(lens)])
    where = {}
    for x in g:
        r = int(np.searchsorted(off, x, side="right") - 1)
        where.setdefault(r, []).append(int(x - off[r]))
    return seqs, mutated(seqs, where)


def check_pair(eng, a_parts, b_parts, a_text, b_text):
    want = em.container(a_text, b_text)
    buf = sentinel(len(want) + 64)
    z, st = eng.fastq_edits(a_parts, b_parts, out=buf)
    assert z.tobytes() == want
    assert (buf[len(want):] == SENT).all()
    pos, _, N, T, _, _, touched = em.edit_list(a_text, b_text)
    assert (st.reads, st.bases, st.edits, st.reads_touched, st.bytes) == (N, T, len(pos), touched, len(want))
    return z


@pytest.mark.parametrize("name", NAMES)
def test_device_container_equals_model_on_the_goldens(eng, name):
    a, b = _raw(name), _raw(name, ".M2B0.fq")
    z = check_pair(eng, [a], [b], a, b)
    assert api.edits_info(z)["n_edits"] == GOLDEN_EDITS[name]
    back, st = eng.fastq_unedit(b, z)
    assert back.tobytes() == em.apply(b, z.tobytes()) and seq_lines(back) == seq_lines(a) and st.edits == GOLDEN_EDITS[name]
    p = eng.prof()
    assert p["k_edit_unpack" if GOLDEN_EDITS[name] else "k_edit_check"]["launches"] >= 1


def test_device_container_equals_model_at_the_length_and_position_borders(eng):
    seqs, mut = pair_edge_lengths(np.random.default_rng(3))
    a, b = text_of(seqs), text_of(mut, hdr=lambda i: b"@")
    z = check_pair(eng, [a], [b], a, b)
    assert seq_lines(eng.fastq_unedit(b, z)[0]) == seq_lines(a)
    # CRLF in A only; B without its final newline and in two parts; A in two parts cut elsewhere
    a2, b2 = text_of(seqs, eol=b"\r\n"), text_of(mut, final=False, hdr=lambda i: b"@")
    cb, ca = len(text_of(mut[:10], hdr=lambda i: b"@")), len(text_of(seqs[:7]))
    assert check_pair(eng, [a2], [b2[:cb], b2[cb:]], a2, b2).tobytes() == z.tobytes()
    assert check_pair(eng, [a[:ca], a[ca:]], [b[:cb - 1], b[cb:]], a, b).tobytes() == z.tobytes()      # (a part that lacks its newline gets one)
    back, _ = eng.fastq_unedit(b2, z)                              # the newline the text lacks is not handed back
    assert back.tobytes() == text_of(seqs, final=False, hdr=lambda i: b"@")
    back, _ = eng.fastq_unedit(text_of(mut, eol=b"\r\n"), z)
    assert back.tobytes() == a2


@pytest.mark.parametrize("E", (0, 1, 1023, 1024, 1025, 2049))
def test_device_container_equals_model_at_the_segment_borders(eng, E):
    seqs, mut = pair_with_E(np.random.default_rng(E + 1), E)
    a, b = text_of(seqs), text_of(mut)
    z = check_pair(eng, [a], [b], a, b)
    assert api.edits_info(z)["n_edits"] == E
    out = sentinel(len(b) + 8)
    back, st = eng.fastq_unedit(b, z, out=out)
    assert back.tobytes() == a and st.edits == E and (out[len(b):] == SENT).all()


def test_more_reads_and_edits_than_one_trip_of_the_grids(eng):
    """the walks run on 2048 workgroups of 16 reads, the check on 128 of 256 reads, the locate pass on 1024 of 256 edits:
    40 000 reads and 300 000 edits make every one of them stride"""
    rng = np.random.default_rng(77)
    lens = rng.integers(8, 31, 40000)
    seqs = random_seqs(rng, lens)
    total = int(lens.sum())
    flat = np.frombuffer(b"".join(seqs), np.uint8).copy()
    at = np.sort(rng.choice(total, 300000, replace=False))
    flat[at] = np.where(flat[at] == ord("A"), ord("C"), ord("A"))
    off = np.concatenate([[0], np.cumsum(lens)])
    mut = [flat[off[i]:off[i + 1]].tobytes() for i in range(len(lens))]
    a, b = text_of(seqs, hdr=lambda i: b"@"), text_of(mut, hdr=lambda i: b"@")
    z = check_pair(eng, [a], [b], a, b)
    assert api.edits_info(z)["n_edits"] == 300000
    assert eng.fastq_unedit(b, z)[0].tobytes() == a
    with pytest.raises(api.BfqError):
        eng.fastq_unedit(a, z)


def test_base_arrays_on_the_device_make_and_apply(eng):
    """bfq_edits_make_device / bfq_edits_apply_device: the layout of run_reads_device, and a line stream as the target"""
    import torch
    seqs, mut = pair_edge_lengths(np.random.default_rng(11))
    lens = np.array([len(s) for s in seqs])
    roff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    N, T = len(seqs), int(lens.sum())
    ba, bb = np.frombuffer(b"".join(seqs), np.uint8), np.frombuffer(b"".join(mut), np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    d_a, d_b, d_r = dev(ba), dev(bb), dev(roff)
    want = em.container(text_of(seqs), text_of(mut))
    d_z = torch.full((len(want) + 64,), SENT, dtype=torch.uint8, device="cuda")
    n, st = eng.edits_make_device(d_a.data_ptr(), d_b.data_ptr(), d_r.data_ptr(), N, T, d_z.data_ptr(), len(want))
    got = d_z.cpu().numpy()
    assert n == len(want) and got[:n].tobytes() == want and (got[n:] == SENT).all() and st.edits == em.decode(want)["E"]
    # a buffer one byte short: refused with the size, nothing written
    d_z.fill_(SENT)
    with pytest.raises(api.BfqError) as e:
        eng.edits_make_device(d_a.data_ptr(), d_b.data_ptr(), d_r.data_ptr(), N, T, d_z.data_ptr(), len(want) - 1)
    assert e.value.code == -1 and e.value.needed == len(want) and str(len(want)) in str(e.value) and (d_z.cpu().numpy() == SENT).all()
    # the way back into the base array, and into a line stream
    d_t = d_b.clone()
    st = eng.edits_apply_device(want, d_t.data_ptr(), d_r.data_ptr(), N, T)
    assert d_t.cpu().numpy().tobytes() == ba.tobytes() and st.edits == em.decode(want)["E"]
    lines_b, lines_a = b"".join(s + b"\n" for s in mut), b"".join(s + b"\n" for s in seqs)
    d_l = dev(np.frombuffer(lines_b, np.uint8))
    eng.edits_apply_device(want, d_l.data_ptr(), d_r.data_ptr(), N, T, lines=True)
    assert d_l.cpu().numpy().tobytes() == lines_a
    # applied to the input's bases: target_sum; nothing written
    d_t = d_a.clone()
    with pytest.raises(api.BfqError) as e:
        eng.edits_apply_device(want, d_t.data_ptr(), d_r.data_ptr(), N, T)
    assert "not the output these edits were made from" in str(e.value) and d_t.cpu().numpy().tobytes() == ba.tobytes()
    # both texts on the device
    ta, tb = text_of(seqs), text_of(mut)
    d_ta, d_tb = dev(np.frombuffer(ta, np.uint8)), dev(np.frombuffer(tb, np.uint8))
    d_z.fill_(SENT)
    n, _ = eng.fastq_edits_device(d_ta.data_ptr(), len(ta), d_tb.data_ptr(), len(tb), d_z.data_ptr(), len(d_z))
    assert d_z.cpu().numpy()[:n].tobytes() == want


# ---- the job --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_job_with_edits_on_the_goldens(eng, name, mode):
    a, ref = _raw(name), _raw(name, ".M2B0.fq")
    eng.set_params(m=5, piles=MODES[mode])
    try:
        eng.prof_reset()
        plain = eng.fastq_job([a], fastq=True, streams=True, hdr=True)
        assert not [k for k in eng.prof() if k.startswith("k_edit")]
        eng.prof_reset()
        r = eng.fastq_job([a], fastq=True, streams=True, hdr=True, edits=True)
        assert eng.prof()["k_edit_count"]["launches"] == 1
    finally:
        eng.set_params(m=5)
    assert r.fastq.tobytes() == ref
    assert r.edits.tobytes() == em.container(a, ref) and api.edits_info(r.edits)["n_edits"] == GOLDEN_EDITS[name]
    for k in ("fastq", "dna", "qs", "hdr"):
        assert getattr(r, k).tobytes() == getattr(plain, k).tobytes(), k
    assert r.stats == plain.stats and r.part_fastq_off == plain.part_fastq_off and plain.edits is None
    assert seq_lines(eng.fastq_unedit(r.fastq, r.edits)[0]) == seq_lines(a)


def test_job_without_the_streams_and_in_two_parts(eng):
    a, ref = _raw("synth_var"), _raw("synth_var", ".M2B0.fq")
    cut = a.index(b"\n@", len(a) // 2) + 1
    r = eng.fastq_job([a[:cut], a[cut:]], fastq=True, edits=True)             # (no line streams: the output bases lie back to back)
    assert r.fastq.tobytes() == ref and r.edits.tobytes() == em.container(a, ref)
    r = eng.fastq_job([a], fastq=False, streams=True, compress=True, edits=True)
    assert r.edits.tobytes() == em.container(a, ref)


def test_job_refusals(eng):
    a, ref = _raw("synth_fix"), _raw("synth_fix", ".M2B0.fq")
    want = em.container(a, ref)
    out = dict(edits=sentinel(len(want) - 1), fastq=sentinel(len(a) + 64))
    with pytest.raises(api.BfqError) as e:
        eng.fastq_job([a], fastq=True, edits=True, out=out)
    assert e.value.code == -1 and e.value.needed == len(want) and str(len(want)) in str(e.value)
    assert (out["edits"] == SENT).all() and (out["fastq"] == SENT).all()
    out = dict(edits=sentinel(200), fastq=sentinel(len(a) + 64))                 # not even a byte per edit fits: a size that suffices
    with pytest.raises(api.BfqError) as e:
        eng.fastq_job([a], fastq=True, edits=True, out=out)
    assert e.value.needed >= len(want) and (out["edits"] == SENT).all()
    out = dict(edits=sentinel(e.value.needed))
    assert eng.fastq_job([a], fastq=False, streams=True, edits=True, out=out).edits.tobytes() == want
    for cs in (2, 3):
        out = dict(edits=sentinel(4096), dna=sentinel(2 * len(a) + 4096), qs=sentinel(2 * len(a) + 4096))
        with pytest.raises(api.BfqError) as e:
            eng.fastq_job([a], fastq=False, streams=True, compress=cs, edits=True, out=out)
        assert e.value.code == -1 and "compress_streams" in str(e.value)
        assert all((v == SENT).all() for v in out.values())


# ---- refusals of the text forms ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(eng, tmp_path):
    rec = lambda i, s: b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s))
    a = b"".join(rec(i, b"ACGT" * 5) for i in range(12))
    b = b"".join(rec(i, b"ACGT" * 4 + (b"AAGT" if i % 3 == 0 else b"ACGT")) for i in range(12))
    z = em.container(a, b)
    out = sentinel(len(a) + 64)

    def refused(call, *words):
        with pytest.raises(api.BfqError) as e:
            call()
        assert e.value.code == -1 and (out == SENT).all()
        for w in words:
            assert w in str(e.value), str(e.value)
    refused(lambda: eng.fastq_edits([a], [b[:len(b) - len(rec(11, b"ACGT" * 5))]], out=out), "12 in A", "11 in B")
    longer = b"".join(rec(i, b"ACGT" * 5 + (b"A" if i in (5, 9) else b"")) for i in range(12))
    refused(lambda: eng.fastq_edits([a], [longer], out=out), "read 5", "20 bases in A and 21 in B")
    refused(lambda: eng.fastq_edits([a], [b], out=out[:len(z) - 1]), str(len(z)))
    tab = a.replace(b"ACGTACGTACGTACGTACGT\n+\nI", b"ACGTACGTACGTACGTAC\tT\n+\nI", 1)
    refused(lambda: eng.fastq_edits([tab], [a], out=out), "outside 33..126")
    refused(lambda: eng.fastq_unedit(a, z, out=out), "not the output these edits were made from")          # applied to the INPUT
    refused(lambda: eng.fastq_unedit(b, em.container(longer, longer), out=out), "242", "240")              # another collection: bases
    refused(lambda: eng.fastq_unedit(b + rec(12, b"ACGT" * 5), z, out=out), "12", "13")                    # ... reads
    other = b"".join(rec(i, b"ACGT" * (4 if i == 0 else 6 if i == 1 else 5)) for i in range(12))
    refused(lambda: eng.fastq_unedit(b, em.container(other, other), out=out), "shape")                     # same N and T, other lengths
    bad = bytearray(z); bad[len(bad) - 8 + 2] = 10
    refused(lambda: eng.fastq_unedit(b, bytes(bad), out=out), "edit 2")                                    # a damaged member: first_bad
    pos, byt, N, T, shape, tsum, _ = em.edit_list(a, b)
    refused(lambda: eng.fastq_unedit(b, em.encode(pos, byt, N, T, shape, tsum, widths={0: 9}), out=out), "edit 0")
    refused(lambda: eng.fastq_unedit(b, z[:-8], out=out), "member 0")
    refused(lambda: eng.fastq_unedit(b, z + z, out=out), "24", "12")
    refused(lambda: eng.fastq_unedit(b, z, out=out[:len(b) - 1]), str(len(b)))
    # the file forms leave their outputs empty
    pa, pb, pz, po = (str(tmp_path / n) for n in ("a.fq", "b.fq", "z.edits", "o"))
    open(pa, "wb").write(a); open(pb, "wb").write(longer); open(pz, "wb").write(z)
    open(po, "wb").write(b"stale")
    with pytest.raises(api.BfqError):
        eng.fastq_edits_files(pa, pb, po)
    assert os.path.getsize(po) == 0
    open(po, "wb").write(b"stale")
    with pytest.raises(api.BfqError):
        eng.fastq_unedit_files(pa, pz, po)
    assert os.path.getsize(po) == 0
    open(pb, "wb").write(b)
    n, st = eng.fastq_edits_files(pa, pb, po)
    assert open(po, "rb").read() == z and n == len(z) and st.edits == 4
    n, st = eng.fastq_unedit_files(pb, po, pa + ".back")
    assert seq_lines(open(pa + ".back", "rb").read()) == seq_lines(a) and n == len(b)


def test_two_members_for_two_blocks(eng):
    a1, b1 = _raw("example"), _raw("example", ".M2B0.fq")
    a2, b2 = _raw("synth_var"), _raw("synth_var", ".M2B0.fq")
    zz = em.container(a1, b1) + em.container(a2, b2) + em.container(a1, b1)
    back, st = eng.fastq_unedit(b1 + b2 + b1, zz)
    assert back.tobytes() == em.apply(b1 + b2 + b1, zz) and seq_lines(back) == seq_lines(a1 + a2 + a1) and st.edits == 618
    out = sentinel(len(b1) * 2 + len(b2) + 8)
    with pytest.raises(api.BfqError) as e:                           # the blocks in another order
        eng.fastq_unedit(b2 + b1 + b1, zz, out=out)
    assert "member 0" in str(e.value) and (out == SENT).all()


# ---- the round trip ---------------------------------------------------------------------------------------------------------
def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, **kw)


@pytest.mark.parametrize("name", ("example", "synth_var"))
def test_round_trip_through_the_restore(eng, name):
    """compress + edits, then fastq_restore(edits=): the input's sequence lines, the plain restore's quality lines"""
    a = _raw(name)
    r = eng.fastq_job([a], keep_headers=True, fastq=True, streams=True, hdr=True, compress=True, edits=True)
    plain, n = eng.fastq_restore(r.dna, r.qs, r.hdr)
    assert plain.tobytes() == r.fastq.tobytes() and n == r.n_reads
    out = sentinel(len(plain) + 64)
    back, n = eng.fastq_restore(r.dna, r.qs, r.hdr, edits=r.edits, out=out)
    assert seq_lines(back) == seq_lines(a) and qual_lines(back) == qual_lines(plain) and (out[len(back):] == SENT).all()
    assert back.tobytes() == em.apply(plain.tobytes(), r.edits.tobytes()) == eng.fastq_unedit(plain, r.edits)[0].tobytes()
    assert eng.prof()["k_edit_apply" if GOLDEN_EDITS[name] else "k_edit_check"]["launches"] >= 1
    # refusals of the restore: the edits of another run, a damaged member, edits that are none; nothing written
    other = eng.fastq_job([_raw("synth_fix")], fastq=False, streams=True, compress=True, edits=True).edits
    bad = r.edits.copy(); bad[len(bad) - em.pad8(GOLDEN_EDITS[name])] = 10               # the byte of edit 0
    for z, word in ((other, "reads"), (bad, "edit 0"), (r.edits[:40], "member 0"), (b"", "BFQEDIT1")):
        out = sentinel(len(plain) + 64)
        with pytest.raises(api.BfqError) as e:
            eng.fastq_restore(r.dna, r.qs, r.hdr, edits=z, out=out)
        assert e.value.code == -1 and word in str(e.value) and (out == SENT).all(), str(e.value)
    with pytest.raises(ValueError):
        eng.fastq_restore(r.dna, r.qs, r.hdr, edits=r.edits, groups=True)


def test_round_trip_after_a_reordering(eng):
    """fastq_reorder(keep=True), the job on the reordered text, then fastq_restore(perm=, edits=): the edits are in run order
    and go in first, the permutation then gives the order -- and the bases -- of the original file"""
    a = _raw("synth_var")
    (ro,), permz = eng.fastq_reorder([a], keep=True)
    r = eng.fastq_job([ro], keep_headers=True, fastq=True, streams=True, hdr=True, compress=True, edits=True)
    assert api.edits_info(r.edits)["n_edits"] > 0
    back, n = eng.fastq_restore(r.dna, r.qs, r.hdr, perm=permz, edits=r.edits)
    plain, _ = eng.fastq_restore(r.dna, r.qs, r.hdr, perm=permz)
    assert seq_lines(back) == seq_lines(a) and qual_lines(back) == qual_lines(plain) and back.tobytes().split(b"\n")[0::4] == a.split(b"\n")[0::4]
    assert seq_lines(plain) != seq_lines(a)


def test_tools_round_trip(eng, tmp_path):
    """bfq_edits (make, list, apply), bfq_restore -E, parallel.py --compress --keep-bases -t 3 and --restore --keep-bases"""
    from bfqzip_amd import parallel
    assert os.path.exists(TOOL) and os.path.exists(RESTORE), "tools missing: run __graft_entry__.build()"
    P = lambda n: str(tmp_path / n)
    src = os.path.join(util.GOLDEN, "synth_var.fastq")
    a, ref = _raw("synth_var"), _raw("synth_var", ".M2B0.fq")
    open(P("out.fq"), "wb").write(ref)
    r = _run([TOOL, "-a", src, "-b", P("out.fq"), "-o", P("run.edits"), "-V"])
    assert r.returncode == 1 and b"598 edits" in r.stdout and b"[bfq phases]" in r.stdout, r.stdout          # cmp's status: they differ
    assert open(P("run.edits"), "rb").read() == em.container(a, ref)
    assert _run([TOOL, "-a", src, "-b", src, "-o", P("none.edits")]).returncode == 0 and os.path.getsize(P("none.edits")) == 64
    r = _run([TOOL, "-l", P("run.edits")])
    assert r.returncode == 0 and b"0  2000  89495  598  " in r.stdout and b"1 members" in r.stdout, r.stdout
    r = _run([TOOL, "-u", "-E", P("run.edits"), "-i", P("out.fq"), "-o", P("back.fq")])
    assert r.returncode == 0, r.stdout
    assert open(P("back.fq"), "rb").read() == em.apply(ref, em.container(a, ref))
    r = _run([TOOL, "-u", "-E", P("run.edits"), "-i", src, "-o", P("back.fq")])                               # applied to the input
    assert r.returncode == 2 and b"not the output these edits were made from" in r.stdout and os.path.getsize(P("back.fq")) == 0
    r = _run([TOOL, "-a", src, "-b", os.path.join(util.GOLDEN, "example.fastq"), "-o", P("x.edits")])
    assert r.returncode == 2 and b"2000 in A, 100 in B" in r.stdout and os.path.getsize(P("x.edits")) == 0
    # the sharded route: one member per block beside the .bsc files
    for args in (["-H", "--m3", "--streams-only"], ["-H", "--m3"]):
        assert parallel.main([src, "-o", P("Z"), "-t", "3", "--compress", "--keep-bases"] + args) == 0
        z = open(P("Z.edits"), "rb").read()
        assert api.edits_info(z)["members"] == 3 and api.edits_info(z)["n_reads"] == 2000
        bsc = [P("Z.fastq.dna.bsc"), P("Z.fastq.qs.bsc"), P("Z.h.bsc")]
        assert parallel.main(["--restore"] + bsc + ["-o", P("plain.fq")]) == 0
        assert parallel.main(["--restore", "--keep-bases"] + bsc + ["-o", P("Z.fq")]) == 0
        back, plain = open(P("Z.fq"), "rb").read(), open(P("plain.fq"), "rb").read()
        assert back.split(b"\n")[0::4] == a.split(b"\n")[0::4] and seq_lines(back) == seq_lines(a) and qual_lines(back) == qual_lines(plain)
        assert back == em.apply(plain, z)
        r = _run([RESTORE, "-d", bsc[0], "-q", bsc[1], "-H", bsc[2], "-E", P("Z.edits"), "-o", P("tool.fq")])
        assert r.returncode == 0 and open(P("tool.fq"), "rb").read() == back, r.stdout
    for flag in (["-g"], ["-G", "0:1"], ["-l"], ["-z"]):
        r = _run([RESTORE, "-d", bsc[0], "-q", bsc[1], "-E", P("Z.edits"), "-o", P("no.fq")] + flag)
        assert r.returncode == 1 and b"-E does not go with" in r.stdout, r.stdout
    r = _run([RESTORE, "-d", bsc[0], "-q", bsc[1], "-E", P("run.edits"), "-o", P("no.fq")])                  # one member for three blocks: shape
    assert r.returncode == 1 and os.path.getsize(P("no.fq")) == 0, r.stdout
    assert parallel.main([src, "-o", P("G"), "--global", "--keep-bases"]) == 1
    assert parallel.main([src, src, "-p", "-o", P("G"), "-t", "2", "--keep-bases"]) == 1


def test_member_counts_that_wrap_are_refused_before_any_launch_uses_them(eng):
    """N is bounded by nothing in a member: members whose read counts add up to the target's only mod 2^64 are held against
    what the target has left, member by member, and refused with nothing written -- text, base array and restore alike"""
    import torch
    rec = lambda i, s: b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s))
    empty = b"".join(rec(i, b"") for i in range(6))
    M = (1 << 64) - 1
    out = sentinel(len(empty) + 8)
    d_r = torch.zeros(7, dtype=torch.int64, device="cuda")
    d_b = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    for ns in ((M, 7), (3, M, 4), (M - 1, 8), (7,), (M,)):
        z = b"".join(em.encode([], [], n, 0, em.shape_of([0] * min(n, 6)), 0) for n in ns)
        for call in (lambda: eng.fastq_unedit(empty, z, out=out), lambda: eng.edits_apply_device(z, d_b.data_ptr(), d_r.data_ptr(), 6, 0)):
            with pytest.raises(api.BfqError) as e:
                call()
            assert e.value.code == -1 and "reads" in str(e.value) and (out == SENT).all() and bool((d_b == SENT).all()), (ns, str(e.value))
    z = em.encode([], [], 2, 0, em.shape_of([0, 0]), 0) + em.encode([], [], 4, 0, em.shape_of([0] * 4), 0)
    assert eng.fastq_unedit(empty, z, out=out)[0].tobytes() == empty
    # a block that claims more bases than are left
    a, b = _raw("example"), _raw("example", ".M2B0.fq")
    good = em.decode(em.container(a, b))
    big = em.encode(good["pos"], good["byte"], good["N"], 1 << 40, good["shape"], good["target_sum"])
    out = sentinel(len(b) + 8)
    with pytest.raises(api.BfqError) as e:
        eng.fastq_unedit(b, big, out=out)
    assert "bases" in str(e.value) and (out == SENT).all()
    r = eng.fastq_job([a], fastq=False, streams=True, compress=True)
    out = sentinel(len(b) + 64)
    wrap = em.encode([], [], M, 0, 0, 0) + em.encode(good["pos"], good["byte"], good["N"] + 1, good["T"], good["shape"], good["target_sum"])
    with pytest.raises(api.BfqError) as e:
        eng.fastq_restore(r.dna, r.qs, edits=wrap, out=out)
    assert e.value.code == -1 and "reads" in str(e.value) and (out == SENT).all()


def test_read_offsets_that_are_no_offsets_are_refused_before_a_base_is_read(eng):
    import torch
    seqs, mut = pair_edge_lengths(np.random.default_rng(5))
    lens = np.array([len(s) for s in seqs])
    roff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    N, T = len(seqs), int(lens.sum())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    d_a, d_b = dev(np.frombuffer(b"".join(seqs), np.uint8)), dev(np.frombuffer(b"".join(mut), np.uint8))
    d_z = torch.full((1 << 16,), SENT, dtype=torch.uint8, device="cuda")
    swapped = roff.copy(); swapped[[5, 6]] = swapped[[6, 5]]                       # not ascending
    shifted = roff + np.uint64(1)                                                   # does not start at 0
    for bad, total, word in ((swapped, T, "read 5"), (shifted, T + 1, "from 1"), (roff, T + 8, "bases stated"), (roff[:-1], T, "bases stated")):
        d_r = dev(bad)
        with pytest.raises(api.BfqError) as e:
            eng.edits_make_device(d_a.data_ptr(), d_b.data_ptr(), d_r.data_ptr(), len(bad) - 1, total, d_z.data_ptr(), len(d_z))
        assert e.value.code == -1 and word in str(e.value) and bool((d_z == SENT).all()), str(e.value)
    want = em.container(text_of(seqs), text_of(mut))
    d_t = d_b.clone()
    with pytest.raises(api.BfqError) as e:
        eng.edits_apply_device(want, d_t.data_ptr(), dev(swapped).data_ptr(), N, T)
    assert e.value.code == -1 and torch.equal(d_t, d_b)


def test_file_form_has_no_capacity_of_its_own(eng, tmp_path):
    """every base differs: the member outgrows input length / 8 + 4096 and is made again in the size it asked for"""
    rng = np.random.default_rng(9)
    seqs = random_seqs(rng, rng.integers(30, 80, 300))
    mut = mutated(seqs, {r: list(range(len(s))) for r, s in enumerate(seqs)})
    a, b = text_of(seqs), text_of(mut)
    want = em.container(a, b)
    assert len(want) > len(a) // 8 + 4096
    pa, pb, po = (str(tmp_path / n) for n in ("a.fq", "b.fq", "z.edits"))
    open(pa, "wb").write(a); open(pb, "wb").write(b)
    n, st = eng.fastq_edits_files(pa, pb, po)
    assert open(po, "rb").read() == want and n == len(want) and st.edits == em.decode(want)["E"]
    r = _run([TOOL, "-a", pa, "-b", pb, "-o", po])
    assert r.returncode == 1 and open(po, "rb").read() == want, r.stdout
