"""GPU tests of the block-by-block way back (bfq_fastq_restore_grouped / _fd, dropin/bfq_restore -g / -G / -l): an archive
as a sequence of groups that decode on their own, restored one after another in a workspace sized by the largest of them.
Pinned to the whole-archive call (bfq_fastq_restore, where it takes the archive), to the forward path (the .fastq of the run
without step 5) and to the input itself where nothing is smoothed."""
import ctypes as C
import os, subprocess
import numpy as np
import pytest
from bfqzip_amd import api, fastq, parallel
from tests import util
from tests.test_parallel_gloo import paired_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dropin", "bfq_restore")
E_ARG, E_NOMEM = -1, -7
SENTINEL = 0xA5


def _collection(rng, nreads, lmin, lmax, **kw):
    b, q, r = util.random_reads(rng, nreads, lmin, lmax, **kw)
    hdrs = [b"@r%d/%d len=%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), int(r[i + 1] - r[i])) for i in range(nreads)]
    return fastq.format_fastq(b, q, r, hdrs)


def _written(engine, tmp, paired=False, **codecs):
    """parallel.run_files with t = 3 on synth_var (or the paired golden input), with and without step 5: per output
    ({kind: .bsc path}, the .fastq text of the plain run)."""
    inputs = list(paired_inputs(tmp)) if paired else [os.path.join(util.GOLDEN, "synth_var.fastq")]
    engine.set_params(m=5)
    try:
        plain = parallel.output_names(inputs, os.path.join(tmp, "P"), paired)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, plain, paired=paired, headers=True, want_streams=True, want_hdr=True)
        z = parallel.output_names(inputs, os.path.join(tmp, "Z"), paired)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, z, paired=paired, headers=True, want_streams=True, want_hdr=True, compress=True,
                           **codecs)
    finally:
        engine.set_params()
    return [({k: z[o][k] + ".bsc" for k in ("dna", "qs", "hdr")}, open(plain[o]["fastq"], "rb").read()) for o in range(len(plain))]


@pytest.fixture(scope="module")
def plain_archive(engine, tmp_path_factory):
    return _written(engine, str(tmp_path_factory.mktemp("groups_plain")))


def _all_ways(engine, tmp, files, want):
    dna, qs, hdr = (np.fromfile(files[k], np.uint8) for k in ("dna", "qs", "hdr"))
    plan = api.HostText.restore_groups(dna, qs, hdr)
    assert len(plan) == 3 and all(g["members"] == (1, 1, 1) for g in plan)
    whole, nr = engine.fastq_restore(dna, qs, hdr)
    assert whole.tobytes() == want and nr == want.count(b"\n") // 4
    got, ng = engine.fastq_restore(dna, qs, hdr, groups=True)           # memory
    assert got.tobytes() == want and ng == nr
    pin = api.PinnedBuffer(sum(g["text_bound"] for g in plan) + 64)      # a pinned destination: direct DMA, two buffers in turn
    try:
        pin.array[:] = SENTINEL
        got, ng = engine.fastq_restore(dna, qs, hdr, out=pin.array, groups=True)
        assert got.tobytes() == want and ng == nr and (pin.array[len(want):] == SENTINEL).all()
    finally:
        pin.free()
    back = os.path.join(tmp, "back.fastq")                                # the file form
    ol, ng = engine.fastq_restore_files(files["dna"], files["qs"], files["hdr"], back, grouped=True)
    assert ol == len(want) and ng == nr and open(back, "rb").read() == want
    # the groups one at a time: the same bytes, and the read counts add up
    singles = [engine.fastq_restore(dna, qs, hdr, groups=(k, 1)) for k in range(len(plan))]
    assert b"".join(t.tobytes() for t, _ in singles) == want and sum(n for _, n in singles) == nr
    assert all(n == (g["reads"] if g["reads"] is not None else n) for (_, n), g in zip(singles, plan))
    tail, nt = engine.fastq_restore(dna, qs, hdr, groups=(1, None))
    assert singles[0][0].tobytes() + tail.tobytes() == want and singles[0][1] + nt == nr
    ol, n1 = engine.fastq_restore_files(files["dna"], files["qs"], files["hdr"], back, grouped=(1, 1))
    assert open(back, "rb").read() == singles[1][0].tobytes() and n1 == singles[1][1] and ol == len(singles[1][0])
    # without the header input: "@" lines
    bare, nb = engine.fastq_restore(dna, qs, groups=True)
    lines = want.split(b"\n")[:-1]
    assert bare.tobytes() == b"".join((b"@" if i % 4 == 0 else x) + b"\n" for i, x in enumerate(lines)) and nb == nr


def test_plain_archive(engine, tmp_path, plain_archive):
    files, want = plain_archive[0]
    _all_ways(engine, str(tmp_path), files, want)
    prof = engine.prof()
    assert prof["k_restore_index"]["launches"] >= 3 and prof["k_fq_format_lines"]["launches"] >= 3


def test_paired_archive(engine, tmp_path):
    for files, want in _written(engine, str(tmp_path), paired=True):
        _all_ways(engine, str(tmp_path), files, want)


def test_archive_with_name_and_quality_containers(engine, tmp_path):
    (files, want), = _written(engine, str(tmp_path), name_codec=True, qual_codec=True)
    _all_ways(engine, str(tmp_path), files, want)


def test_buffers_alternate_and_the_largest_group_is_not_the_first(engine):
    """Blocks of 1, 700, 40, 0, 2500 and 3 reads, each compressed by its own job: six groups, the reservation is the fifth's;
    the last line of the last group has lost its newline (the end of an archive: it gets one, as in the whole-archive call)."""
    rng = np.random.default_rng(20250101)
    texts = [_collection(rng, n, 20, 150) if n else b"" for n in (1, 700, 40, 0, 2500, 3)]
    engine.set_params(m=3, k=8)
    try:
        z = [engine.fastq_job([t], keep_headers=True, fastq=True, streams=True, hdr=True, compress=1) for t in texts[:-1]]
        last = engine.fastq_job([texts[-1]], keep_headers=True, fastq=True, streams=True, hdr=True)
    finally:
        engine.set_params()
    blobs = {k: [np.array(getattr(j, k)) for j in z] for k in ("dna", "qs", "hdr")}
    for k in blobs:
        raw = np.asarray(getattr(last, k))
        assert raw[-1] == 10
        blobs[k].append(np.array(engine.stream_compress(raw[:-1])))
    dna, qs, hdr = (np.concatenate(blobs[k]) for k in ("dna", "qs", "hdr"))
    want = b"".join(j.fastq.tobytes() for j in z) + last.fastq.tobytes()
    plan = api.HostText.restore_groups(dna, qs, hdr)
    assert len(plan) == 6 and plan[3]["raw_stream"] == 0 and max(range(6), key=lambda k: plan[k]["text_bound"]) == 4
    whole, nr = engine.fastq_restore(dna, qs, hdr)
    got, ng = engine.fastq_restore(dna, qs, hdr, groups=True)
    assert nr == ng == 3244 and whole.tobytes() == want and got.tobytes() == want
    pin = api.PinnedBuffer(len(want) + 64)
    try:
        got, ng = engine.fastq_restore(dna, qs, hdr, out=pin.array, groups=True)
        assert got.tobytes() == want
    finally:
        pin.free()
    assert b"".join(engine.fastq_restore(dna, qs, hdr, groups=(k, 1))[0].tobytes() for k in range(6)) == want


def test_under_a_cap(engine, tmp_path):
    """2 M x 100 with headers, K above every LCP (nothing is smoothed: the archive restores to the input), written in 64
    blocks.  Under a 512 MiB workspace cap the whole archive is refused (measured: 13.3 GiB wanted -- the static DNA
    containers state no read count, so its index is sized for one read per byte) and every group fits (measured: 392 MB).  By the reservation formula, with n = 3.2 MB per stream and group: a block this small gets the static DNA
    container, which states no read count, so the index is sized for one read per byte (64 n = 202 MB) against 9 n + 294 MB
    for the codec's workspace; with the streams (2 n), two text buffers (8 n) and 64 MiB about 390 MB.  (32 blocks: 64 n =
    404 MB of index, 540 MB in all -- measured: refused by a few MB.)"""
    sp = api.synth_spec(2_000_000, 100, seed=3)
    text = np.empty(2_000_000 * 260, np.uint8)
    text = text[:engine.synth_fastq(sp, text)]
    src = str(tmp_path / "big.fastq")
    text.tofile(src)
    names = parallel.output_names([src], str(tmp_path / "Z"), False)
    engine.set_params(k=10000)
    try:
        parallel.run_files(engine, parallel.Comm(), [src], 64, names, headers=True, want_fastq=False, want_streams=True, want_hdr=True, compress=True)
    finally:
        engine.set_params()
    dna, qs, hdr = (np.fromfile(names[0][k] + ".bsc", np.uint8) for k in ("dna", "qs", "hdr"))
    assert len(api.HostText.restore_groups(dna, qs, hdr)) == 64
    rng = np.random.default_rng(11)
    small_text = _collection(rng, 500, 30, 120)
    zs = engine.fastq_job([small_text], keep_headers=True, fastq=True, streams=True, hdr=True, compress=1)
    small = api.Engine(0, ws_cap_mib=512)
    try:
        out = np.full(1 << 20, SENTINEL, np.uint8)
        with pytest.raises(api.BfqError, match="GiB") as e:
            small.fastq_restore(dna, qs, hdr, out=out)
        print("whole archive:", e.value)
        assert e.value.code == E_NOMEM and "cap" in str(e.value) and (out == SENTINEL).all()
        got, nr = small.fastq_restore(dna, qs, hdr, groups=True)
        print("grouped: workspace of", small.L.bfq_workspace_bytes(small.h), "bytes")
        assert nr == 2_000_000 and len(got) == len(text) and np.array_equal(got, text)
        assert small.L.bfq_workspace_bytes(small.h) <= 512 << 20
        got, nr = small.fastq_restore(zs.dna, zs.qs, zs.hdr)             # the same engine goes on
        assert got.tobytes() == zs.fastq.tobytes() and nr == 500
        # a cap below one group: BFQ_E_NOMEM names the group that sized the reservation and the cap
        small.set_params(ws_cap_mib=128)
        with pytest.raises(api.BfqError, match=r"cap.*sized by group \d+") as e:
            small.fastq_restore(dna, qs, hdr, out=out, groups=True)
        assert e.value.code == E_NOMEM and (out == SENTINEL).all()
    finally:
        small.close()


def _streams(text):
    lines = text.split(b"\n")[:-1]
    cat = lambda xs: b"".join(x + b"\n" for x in xs)
    return cat(lines[1::4]), cat(lines[3::4]), cat(lines[0::4])


def _zs(engine, raw):
    return np.array(engine.stream_compress(np.frombuffer(raw, np.uint8)))


def _grouped_refused(engine, code, dna, qs, hdr, match, groups=True, size=1 << 20):
    out = np.full(size, SENTINEL, np.uint8)
    with pytest.raises(api.BfqError, match=match) as e:
        engine.fastq_restore(dna, qs, hdr, out=out, groups=groups)
    assert e.value.code == code, str(e.value)
    return out, str(e.value)


def test_refusals(engine, tmp_path):
    rng = np.random.default_rng(77)
    blocks = [_streams(_collection(rng, n, 30, 120)) for n in (300, 400, 350)]
    z = [[_zs(engine, s) for s in b] for b in blocks]
    dna, qs, hdr = (np.concatenate([m[i] for m in z]) for i in range(3))
    want = b"".join(fastq.restore_text(*b) for b in blocks)
    got, nr = engine.fastq_restore(dna, qs, hdr, groups=True)
    assert got.tobytes() == want and nr == 1050
    # group 1's qualities from another collection of the same raw length: the same line lengths in another order
    ql = blocks[1][1].split(b"\n")[:-1]
    other = ql[1:] + ql[:1]
    first = next(i for i in range(400) if len(other[i]) != len(ql[i]))
    bad_qs = np.concatenate([z[0][1], _zs(engine, b"".join(x + b"\n" for x in other)), z[2][1]])
    assert len(api.HostText.restore_groups(dna, bad_qs, hdr)) == 3
    out, msg = _grouped_refused(engine, E_ARG, dna, bad_qs, hdr, rf"read {300 + first} \(read {first} of group 1\)", size=len(want) + 64)
    assert (out[len(fastq.restore_text(*blocks[0])):] == SENTINEL).all()      # (memory: written up to the failing group at most)
    _grouped_refused(engine, E_ARG, dna, bad_qs, hdr, rf"read {first} of group 1", groups=(1, 1))   # reads before the range unknown: BFQRANS2 states none
    # members cut mid-line: DNA and qualities of block 0 cut at the same byte inside a line, two members each
    d0, q0 = blocks[0][0], blocks[0][1]
    at = d0.index(b"\n", len(d0) // 2) + 4
    assert d0[at - 1] != 10 and d0[at] != 10
    cut_d = np.concatenate([_zs(engine, d0[:at]), _zs(engine, d0[at:]), z[1][0], z[2][0]])
    cut_q = np.concatenate([_zs(engine, q0[:at]), _zs(engine, q0[at:]), z[1][1], z[2][1]])
    assert len(api.HostText.restore_groups(cut_d, cut_q)) == 4
    out, _ = _grouped_refused(engine, E_ARG, cut_d, cut_q, None, r"group 0: its DNA stream does not end with a line end.*not cut at reads.*one piece")
    assert (out == SENTINEL).all()
    whole, _ = engine.fastq_restore(cut_d, cut_q)                        # in one piece the cut does not matter
    assert whole.tobytes() == b"".join(fastq.restore_text(b[0], b[1]) for b in blocks)
    # a payload byte of group 2 flipped: the member's checksum, BFQ_E_ARG, out_len = 0; the file form leaves the file empty
    flip = dna.copy()
    flip[len(dna) - 1500] ^= 0x40
    assert len(z[2][0]) > 3000
    out = np.full(len(want) + 64, SENTINEL, np.uint8)
    ol, nr = C.c_uint64(123), C.c_uint64(123)
    rc = engine.L.bfq_fastq_restore_grouped(engine.h, api._ptr(flip), len(flip), api._ptr(qs), len(qs), api._ptr(hdr), len(hdr), 0, api.ALL_GROUPS,
                                            api._ptr(out), len(out), C.byref(ol), C.byref(nr))
    assert rc == E_ARG and ol.value == 0 and nr.value == 0, engine.L.bfq_last_error(engine.h)
    p = {}
    for k, a in (("dna", flip), ("qs", qs), ("hdr", hdr)):
        p[k] = str(tmp_path / (k + ".bsc"))
        a.tofile(p[k])
    back = str(tmp_path / "back.fq")
    with pytest.raises(api.BfqError) as e:
        engine.fastq_restore_files(p["dna"], p["qs"], p["hdr"], back, grouped=True)
    assert e.value.code == E_ARG and os.path.getsize(back) == 0
    # a header input of two members for three groups: refused from the plan, nothing written
    out, _ = _grouped_refused(engine, E_ARG, dna, qs, np.concatenate([z[0][2], z[1][2]]), r"2 header members for 3 groups.*one piece")
    assert (out == SENTINEL).all()
    # groups with perm: before any call is made
    with pytest.raises(ValueError, match="perm"):
        engine.fastq_restore(dna, qs, hdr, perm=np.zeros(8, np.uint8), groups=True)
    with pytest.raises(ValueError, match="perm"):
        engine.fastq_restore_files(p["dna"], p["qs"], p["hdr"], back, perm_path="x.perm", grouped=True)
    # a range outside the plan
    for rg in ((3, None), (3, 1), (7, None), (1, 3), (0, 4)):
        out, _ = _grouped_refused(engine, E_ARG, dna, qs, hdr, r"outside the plan of 3 groups", groups=rg)
        assert (out == SENTINEL).all()
    got, nr = engine.fastq_restore(dna, qs, hdr, groups=(0, 3))
    assert got.tobytes() == want


@pytest.mark.parametrize("mode", [2, 3])
def test_ebwt_domain_archives(engine, mode):
    """The outputs of two compress_streams = 2 / 3 jobs back to back: one BFQEBWT1 member per group, each through the LF walk
    on its own; the whole-archive call still refuses them."""
    rng = np.random.default_rng(5 + mode)
    texts = [_collection(rng, 600, 20, 150), _collection(rng, 250, 1, 80, p_n=0.2, dup=0.5)]
    engine.set_params(m=3, k=8)
    try:
        for kh in (True, False):
            z = [engine.fastq_job([t], keep_headers=kh, fastq=False, streams=True, hdr=kh, compress=mode) for t in texts]
            want = b"".join(engine.fastq_job([t], keep_headers=kh, fastq=True).fastq.tobytes() for t in texts)
            dna, qs = (np.concatenate([np.asarray(getattr(j, k)) for j in z]) for k in ("dna", "qs"))
            hdr = np.concatenate([np.asarray(j.hdr) for j in z]) if kh else None
            assert dna[:8].tobytes() == b"BFQEBWT1"
            plan = api.HostText.restore_groups(dna, qs, hdr)
            assert [g["reads"] for g in plan] == [600, 250] and [g["members"][:2] for g in plan] == [(1, 1), (1, 1)]
            got, nr = engine.fastq_restore(dna, qs, hdr, groups=True)
            assert nr == 850 and got.tobytes() == want, (mode, kh)
            one, n1 = engine.fastq_restore(dna, qs, hdr, groups=(1, 1))
            assert n1 == 250 and got.tobytes().endswith(one.tobytes()) and len(one) == len(want) - len(engine.fastq_restore(dna, qs, hdr, groups=(0, 1))[0])
            with pytest.raises(api.BfqError, match="more than one BFQEBWT1"):
                engine.fastq_restore(dna, qs, hdr, out=np.empty(len(want) + 64, np.uint8))
    finally:
        engine.set_params()


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_front_end(engine, tmp_path, plain_archive):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    files, want = plain_archive[0]
    dna, qs, hdr = (np.fromfile(files[k], np.uint8) for k in ("dna", "qs", "hdr"))
    out = str(tmp_path / "OUT.fq")
    io = ["-d", files["dna"], "-q", files["qs"], "-H", files["hdr"], "-o", out]
    r = _run([EXE, "-g", "-V"] + io)
    assert r.returncode == 0 and b"[bfq phases]" in r.stdout and b"d2h_write" in r.stdout, r.stdout
    assert open(out, "rb").read() == want and b"%d reads, %d bytes" % (want.count(b"\n") // 4, len(want)) in r.stdout
    r = _run([EXE, "-G", "1:1"] + io)
    assert r.returncode == 0, r.stdout
    assert open(out, "rb").read() == engine.fastq_restore(dna, qs, hdr, groups=(1, 1))[0].tobytes()
    r = _run([EXE, "-G", "2"] + io)
    assert r.returncode == 0 and want.endswith(open(out, "rb").read()) and os.path.getsize(out) > 0
    r = _run([EXE, "-G", "3"] + io)                                     # outside the plan: exit 1, the file left empty
    assert r.returncode == 1 and b"outside the plan" in r.stdout and os.path.getsize(out) == 0
    os.remove(out)
    r = _run([EXE, "-l"] + io)
    plan = api.HostText.restore_groups(dna, qs, hdr)
    rows = [l.split() for l in r.stdout.decode().splitlines() if l and l[0].isdigit() and "groups" not in l]
    assert r.returncode == 0 and not os.path.exists(out)
    assert [[int(x) if x != "?" else None for x in row] for row in rows] == [
        [k, *g["members"], g["dna_len"] + g["qs_len"] + g["hdr_len"], 2 * g["raw_stream"] + g["raw_hdr"], g["reads"], g["text_bound"]]
        for k, g in enumerate(plan)]
