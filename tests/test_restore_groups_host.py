"""The group plan of the block-by-block way back (bfq_fastq_restore_groups through api.HostText.restore_groups), the
front-end's -l / -g -P handling and parallel.restore_files on the CPU oracle, single process and as two gloo ranks.
Containers come from orc.codec_encode, expected texts from fastq.restore_text.  No GPU needed."""
import os, subprocess, sys
import numpy as np
import pytest
from bfqzip_amd import api, fastq, parallel
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dropin", "bfq_restore")
EXAMPLE = os.path.join(util.GOLDEN, "example.fastq")
E_ARG = -1
KEYS = ("dna_off", "dna_len", "qs_off", "qs_len", "hdr_off", "hdr_len", "raw_stream", "raw_hdr")


def _block(rng, nreads, lmin=5, lmax=60, tag=b"b"):
    """(DNA lines, quality lines, header lines) of a block of random reads, each a byte string of whole lines."""
    b, q, r = util.random_reads(rng, nreads, lmin, lmax) if nreads else (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    hdr = b"".join(b"@%s.%d len=%d\n" % (tag, i, int(r[i + 1] - r[i])) for i in range(nreads))
    return fastq.format_lines(b, r), fastq.format_lines(q, r), hdr


def _z(orc, raw):
    return orc.codec_encode(np.frombuffer(raw, np.uint8)).tobytes()


def _cat(blobs):
    return np.frombuffer(b"".join(blobs), np.uint8)


def _check(orc, plan, dna, qs, hdr, want):
    """Every entry against `want` = [(DNA blobs, quality blobs, header blob or None, raw stream, raw header)] per group; the
    group's slices decode to its own text."""
    assert len(plan) == len(want)
    od = oq = oh = 0
    for g, (zd, zq, zh, rd, rq, rh) in zip(plan, want):
        ld, lq, lh = sum(map(len, zd)), sum(map(len, zq)), len(zh) if zh is not None else 0
        got = tuple(g[k] for k in KEYS)
        assert got == (od, ld, oq, lq, oh if zh is not None else 0, lh, len(rd), len(rh) if zh is not None else 0), (got, od, oq, oh)
        assert g["members"] == (len(zd), len(zq), 1 if zh is not None else 0)
        assert g["reads"] is None                                      # a BFQRANS2 member states no read count
        assert g["text_bound"] >= len(fastq.restore_text(rd, rq, rh if zh is not None else None))
        sl = lambda a, o, n: orc.codec_decode(a[o:o + n]).tobytes() if n else b""
        assert sl(dna, g["dna_off"], g["dna_len"]) == rd and sl(qs, g["qs_off"], g["qs_len"]) == rq
        if zh is not None:
            assert sl(hdr, g["hdr_off"], g["hdr_len"]) == rh
        od += ld; oq += lq; oh += lh


def _archive(orc, blocks, cut_dna=()):
    """blocks: [(DNA, qualities, headers)] -> (dna, qs, hdr arrays, the `want` list of _check).  cut_dna: blocks whose DNA stream
    is cut at a line end into two containers."""
    want = []
    for k, (d, q, h) in enumerate(blocks):
        if k in cut_dna:
            at = d.index(b"\n", len(d) // 2) + 1
            assert 0 < at < len(d)
            zd = [_z(orc, d[:at]), _z(orc, d[at:])]
        else:
            zd = [_z(orc, d)]
        want.append((zd, [_z(orc, q)], _z(orc, h), d, q, h))
    return _cat(b for w in want for b in w[0]), _cat(w[1][0] for w in want), _cat(w[2] for w in want), want


def test_three_aligned_blocks_with_headers(orc):
    rng = np.random.default_rng(1)
    dna, qs, hdr, want = _archive(orc, [_block(rng, n, tag=b"t%d" % n) for n in (40, 7, 120)])
    plan = api.HostText.restore_groups(dna, qs, hdr)
    _check(orc, plan, dna, qs, hdr, want)
    # without the header input: the same cut, no header fields
    bare = api.HostText.restore_groups(dna, qs)
    _check(orc, bare, dna, qs, None, [(zd, zq, None, rd, rq, rh) for zd, zq, _, rd, rq, rh in want])
    # cap = 1: the count is still 3, one entry is filled
    L = api._lib.lib()
    arr = (api._lib.RestoreGroup * 3)()
    for k in range(3):
        arr[k].dna_len = 0xDEAD
    G = L.bfq_fastq_restore_groups(api._ptr(dna), len(dna), api._ptr(qs), len(qs), api._ptr(hdr), len(hdr), arr, 1, None, 0)
    assert G == 3 and arr[0].dna_len == plan[0]["dna_len"] and arr[1].dna_len == 0xDEAD and arr[2].dna_len == 0xDEAD
    assert L.bfq_stream_members(api._ptr(dna), len(dna)) == 3 and L.bfq_stream_members(api._ptr(dna), len(dna) - 1) == -1


def test_a_stream_cut_into_more_pieces_still_groups(orc):
    rng = np.random.default_rng(2)
    blocks = [_block(rng, n, tag=b"c%d" % n) for n in (30, 50, 20)]
    dna, qs, hdr, want = _archive(orc, blocks, cut_dna=(1,))
    plan = api.HostText.restore_groups(dna, qs, hdr)                   # three header members for three groups: accepted
    _check(orc, plan, dna, qs, hdr, want)
    assert plan[1]["members"] == (2, 1, 1)
    two = _cat(w[2] for w in want[:2])                                 # two header members for three groups
    with pytest.raises(api.BfqError, match=r"\b2 header members for 3 groups\b.*one piece") as e:
        api.HostText.restore_groups(dna, qs, two)
    assert e.value.code == E_ARG
    four = _cat([w[2] for w in want] + [want[0][2]])
    with pytest.raises(api.BfqError, match=r"\b4 header members for 3 groups\b"):
        api.HostText.restore_groups(dna, qs, four)


def test_edge_cases(orc):
    rng = np.random.default_rng(3)
    # an empty block in the middle, and a group of exactly one read
    blocks = [_block(rng, 10), _block(rng, 0), _block(rng, 1, 1, 1), _block(rng, 25)]
    dna, qs, hdr, want = _archive(orc, blocks)
    plan = api.HostText.restore_groups(dna, qs, hdr)
    _check(orc, plan, dna, qs, hdr, want)
    assert plan[1]["raw_stream"] == 0 and plan[1]["raw_hdr"] == 0 and plan[1]["dna_len"] > 0
    assert plan[2]["raw_stream"] == 2                                   # one base and its newline
    # an archive of one group
    dna, qs, hdr, want = _archive(orc, [_block(rng, 33)])
    _check(orc, api.HostText.restore_groups(dna, qs, hdr), dna, qs, hdr, want)


def test_refusals(orc):
    rng = np.random.default_rng(4)
    blocks = [_block(rng, 20), _block(rng, 30)]
    dna, qs, hdr, want = _archive(orc, blocks)
    # quality members whose total differs from the DNA total by one byte
    q1 = blocks[1][1][:-1]
    short = _cat([want[0][1][0], _z(orc, q1)])
    totD, totQ = sum(len(b[0]) for b in blocks), len(blocks[0][1]) + len(q1)
    with pytest.raises(api.BfqError, match=rf"{totD} bytes.*{totQ}\b.*not of the same collection") as e:
        api.HostText.restore_groups(dna, short, hdr)
    assert e.value.code == E_ARG
    # trailing bytes that are no container: their position
    for junk in (b"garbage!" * 4, b"\0" * 700):
        with pytest.raises(api.BfqError, match=rf"dna: not a container at byte {len(dna)} ") as e:
            api.HostText.restore_groups(np.concatenate([dna, np.frombuffer(junk, np.uint8)]), qs, hdr)
        assert e.value.code == E_ARG
    with pytest.raises(api.BfqError, match=rf"qs: not a container at byte {len(want[0][1][0])} "):
        api.HostText.restore_groups(dna, np.concatenate([qs[:len(want[0][1][0])], np.zeros(100, np.uint8)]), hdr)
    # an empty input
    for a, name in ((0, "dna"), (1, "qs"), (2, "hdr")):
        args = [dna, qs, hdr]
        args[a] = np.zeros(0, np.uint8)
        with pytest.raises(api.BfqError, match=rf"{name}: not a container \(empty input\)") as e:
            api.HostText.restore_groups(*args)
        assert e.value.code == E_ARG


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_front_end_lists_the_plan_without_a_gpu(orc, tmp_path):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    rng = np.random.default_rng(5)
    dna, qs, hdr, want = _archive(orc, [_block(rng, n) for n in (12, 0, 40)], cut_dna=(2,))
    p = {k: str(tmp_path / (k + ".bsc")) for k in ("d", "q", "h")}
    for k, a in zip("dqh", (dna, qs, hdr)):
        a.tofile(p[k])
    out = str(tmp_path / "never.fq")
    plan = api.HostText.restore_groups(dna, qs, hdr)
    r = _run([EXE, "-l", "-d", p["d"], "-q", p["q"], "-H", p["h"], "-o", out])
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.decode().splitlines() if l and l[0].isdigit() and "groups" not in l]
    assert [[int(x) if x != "?" else None for x in row] for row in rows] == [
        [k, *g["members"], g["dna_len"] + g["qs_len"] + g["hdr_len"], 2 * g["raw_stream"] + g["raw_hdr"], g["reads"], g["text_bound"]]
        for k, g in enumerate(plan)]
    assert b"3 groups" in r.stdout and not os.path.exists(out)
    r = _run([EXE, "-l", "-d", p["d"], "-q", p["q"]])                   # -o is not needed to list
    assert r.returncode == 0 and len(r.stdout.decode().splitlines()) == len(rows) + 2
    r = _run([EXE, "-l", "-d", p["d"], "-q", p["h"]])                   # what does not group: the library's reason, status 1
    assert r.returncode == 1 and b"not of the same collection" in r.stderr
    # the permutation does not go with the groups: a usage error that names it
    for flags in (["-g"], ["-G", "1:1"]):
        r = _run([EXE, *flags, "-P", "x.perm", "-d", p["d"], "-q", p["q"], "-o", out])
        assert r.returncode == 1 and b"usage:" in r.stderr and b"permutation -P x.perm" in r.stderr, r.stderr
        assert not os.path.exists(out)
    r = _run([EXE, "-G", "1:", "-d", p["d"], "-q", p["q"], "-o", out])  # a malformed range
    assert r.returncode == 1 and b"usage:" in r.stderr and not os.path.exists(out)


class RestoringOracle(util.OracleEngine):
    """OracleEngine with the grouped way back: the plan from the library's host code, every group decoded by the CPU
    statement of the codec and formatted by fastq.restore_text."""

    def fastq_restore(self, dna, qs, hdr=None, out=None, groups=None):
        assert groups is not None
        plan = self.host.restore_groups(dna, qs, hdr)
        first, count = (0, None) if groups is True else groups
        texts = []
        for g in plan[first:] if count is None else plan[first:first + count]:
            dec = lambda a, o, n: self.orc.codec_decode(np.asarray(a[o:o + n])).tobytes()
            texts.append(fastq.restore_text(dec(dna, g["dna_off"], g["dna_len"]), dec(qs, g["qs_off"], g["qs_len"]),
                                            dec(hdr, g["hdr_off"], g["hdr_len"]) if hdr is not None else None))
        text = b"".join(texts)
        return np.frombuffer(text, np.uint8), text.count(b"\n") // 4


def _archive_of_run(orc, t, tmp):
    """run_files on the example with and without step 5: (names of the plain run, names of the compressed one)."""
    eng = RestoringOracle(orc, m=5)
    plain = parallel.output_names([EXAMPLE], os.path.join(tmp, f"P{t}"), False)
    parallel.run_files(eng, parallel.Comm(), [EXAMPLE], t, plain, headers=True, want_streams=True, want_hdr=True)
    z = parallel.output_names([EXAMPLE], os.path.join(tmp, f"Z{t}"), False)
    parallel.run_files(eng, parallel.Comm(), [EXAMPLE], t, z, headers=True, want_streams=True, want_hdr=True, compress=True)
    return plain[0], {k: v + ".bsc" for k, v in z[0].items()}


@pytest.mark.parametrize("t", [3, 8])
def test_restore_files_single_process(orc, tmp_path, t):
    plain, z = _archive_of_run(orc, t, str(tmp_path))
    eng = RestoringOracle(orc, m=5)
    assert len(eng.host.restore_groups(parallel.map_file(z["dna"]), parallel.map_file(z["qs"]), parallel.map_file(z["hdr"]))) == len(parallel.split_blocks(100, t))
    back = str(tmp_path / "back.fastq")
    tot = parallel.restore_files(eng, parallel.Comm(), z["dna"], z["qs"], z["hdr"], back)
    want = open(plain["fastq"], "rb").read()
    assert open(back, "rb").read() == want
    assert tot["reads"] == 100 and tot["groups"] == len(parallel.split_blocks(100, t)) and tot["bytes_all"] == len(want)
    parallel.restore_files(eng, parallel.Comm(), z["dna"], z["qs"], None, back)       # without headers: "@" lines, a shorter file
    lines = want.split(b"\n")[:-1]
    assert open(back, "rb").read() == b"".join((b"@" if i % 4 == 0 else x) + b"\n" for i, x in enumerate(lines))


def _worker(rank, world, port, z, back, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import orc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tot = parallel.restore_files(RestoringOracle(orc, m=5), parallel.Comm(dist), z["dna"], z["qs"], z["hdr"], back)
        q.put((rank, tot["groups"], tot["reads"]))
    except Exception as e:                                     # surface the failure instead of a queue timeout
        q.put((rank, f"{type(e).__name__}: {e}", -1))
        raise
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("t", [3, 8])
def test_restore_files_two_ranks_gloo(orc, tmp_path, t):
    """More groups than ranks and an odd count: group k by rank k mod 2, the lengths all-gathered round by round, every rank
    writing at its final offset."""
    import torch.multiprocessing as mp
    plain, z = _archive_of_run(orc, t, str(tmp_path))
    back = str(tmp_path / "back2.fastq")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32500 + (os.getpid() * 7 + t) % 3000
    ps = [ctx.Process(target=_worker, args=(rk, 2, port, z, back, q)) for rk in range(2)]
    for p in ps:
        p.start()
    got = sorted(q.get(timeout=180) for _ in ps)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0, got
    nb = len(parallel.split_blocks(100, t))
    assert [g[1] for g in got] == [(nb + 1) // 2, nb // 2] and sum(g[2] for g in got) == 100, got
    assert open(back, "rb").read() == open(plain["fastq"], "rb").read()
