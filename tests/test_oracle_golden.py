"""CPU tests: the oracle (oracle/bfq_oracle.c) against the golden vectors made by the
compiled reference (tests/golden/make_golden.py), and against the reference
binary's outputs on random small inputs (tests/golden/ref_cases.*; the binary itself is run
again where oracle/_ref is built)."""
import os, subprocess
import numpy as np
import pytest
from bfqzip_amd import fastq
from tests import util

IDX = util.golden_index()
CASES = [(name, key) for name in IDX for key in IDX[name]["out"]]


@pytest.mark.parametrize("name", list(IDX))
def test_oracle_ebwt_matches_golden(orc, name):
    b, q, r, h, bwt, qs, lcp = util.golden_set(name)
    bwt2, qs2, lcp2 = orc.build_ebwt(b, q, r)
    assert util.md5(bwt2.tobytes()) == IDX[name]["bwt_md5"]
    assert util.md5(qs2.tobytes()) == IDX[name]["qs_md5"]
    assert np.array_equal(lcp2.astype(np.uint16), lcp)
    assert len(bwt2) == IDX[name]["n"]


@pytest.mark.parametrize("name,key", CASES)
def test_oracle_matches_reference_output(orc, name, key):
    b, q, r, h, bwt, qs, lcp = util.golden_set(name)
    d, hdr = util.parse_case(key)
    p = orc.params(K=d["k"], m=d["m"], v=d["v"], f=d["f"], t=d["t"], M=d["M"], B=d["B"])
    ob, oq, oroff, st = orc.smooth_invert(bwt, qs, None, p)           # LCP deduced from the BWT
    out = fastq.format_fastq(ob, oq, oroff, h if hdr else None)
    assert util.md5(out) == IDX[name]["out"][key]
    ob2, oq2, oroff2, st2 = orc.smooth_invert(bwt, qs, lcp.astype(np.uint32), p)   # explicit LCP (bfq_ext mode)
    assert np.array_equal(ob, ob2) and np.array_equal(oq, oq2) and st == st2
    if key == "M2B0 -m 5":
        assert out == open(os.path.join(util.GOLDEN, name + ".M2B0.fq"), "rb").read()


def test_example_known_answers(orc):
    """SURVEY Appendix B facts for example/reads.fastq, M=2 B=0 -m 5."""
    b, q, r, h, bwt, qs, lcp = util.golden_set("example")
    assert bwt[:40].tobytes() == b"CCTGGAAAGAGGGTGCGGCGCCCCCCTATGATAACACTGT"
    ob, oq, oroff, st = orc.smooth_invert(bwt, qs, None, orc.params(m=5))
    assert (st["num_clust"], st["bases_inside"], st["qs_smoothed"], st["modified"]) == (387, 4210, 4198, 10)
    ob, oq, oroff, st = orc.smooth_invert(bwt, qs, None, orc.params(K=10000))
    assert np.array_equal(ob, b) and np.array_equal(oq, q) and st["num_clust"] == 0


def test_oracle_vs_reference_binary_fuzz(orc, tmp_path):
    """Differential fuzz against the reference bfq_int: 60 random small inputs with the md5 of the reference's output
    for each (tests/golden/ref_cases.*, written by make_golden.py from oracle/_ref/bfq_int_M?_B?); the binaries
    themselves are run again where they are built."""
    cases, arr = util.ref_cases()
    assert len(cases["fuzz"]) == 60
    for it, c in enumerate(cases["fuzz"]):
        b, q, r = arr[f"fuzz{it}_bases"], arr[f"fuzz{it}_quals"], arr[f"fuzz{it}_roff"]
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        assert util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], it
        p = orc.params(K=c["K"], m=c["m"], v=c["v"], f=c["f"], t=c["t"], M=c["M"], B=c["B"])
        ob, oq, oroff, st = orc.smooth_invert(bwt, qs, None, p)
        assert util.md5(fastq.format_fastq(ob, oq, oroff)) == c["out_md5"], (it, c)
        ref = orc.ref_binary(c["M"], c["B"])
        if ref is not None:
            d = str(tmp_path)
            bwt.tofile(d + "/x.bwt"); qs.tofile(d + "/x.bwt.qs")
            cmd = [ref, "-e", d + "/x.bwt", "-q", d + "/x.bwt.qs", "-o", d + "/o.fq",
                   "-k", str(c["K"]), "-m", str(c["m"]), "-v", str(c["v"]), "-t", str(c["t"]), "-f", str(c["f"])]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL, timeout=60)
            assert util.md5(open(d + "/o.fq", "rb").read()) == c["out_md5"], (it, c)


def test_tie_order_of_identical_suffixes_is_free(orc, tmp_path):
    """The reference sees ONE terminator symbol: an eBWT whose identical suffixes (and terminator rows) are in any
    order is processed all the same, LCP by the usual convention.  Pins, against the reference's output on eBWTs with
    shuffled ties (tests/golden/ref_cases.*; the compiled reference is run again where it is built), the contract the
    GPU's BWT-only LCP deduction (k_bfs.hip) is tested with in tests/test_gpu_parity.py."""
    cases, arr = util.ref_cases()
    ref = orc.ref_binary(2, 0)
    done = 0
    for it, c in enumerate(cases["tie"]):
        sb, sq = arr[f"tie{it}_bwt"], arr[f"tie{it}_qs"]
        suf, reads = util.decode_rows(sb)
        lc = util.lcp_of_rows(suf)
        p = orc.params(m=2, K=c["K"])
        ob, oq, oroff, st = orc.smooth_invert(sb, sq, lc, p)
        ob2, oq2, oroff2, st2 = orc.smooth_invert(sb, sq, None, p)            # the oracle's own BWT-only deduction
        assert np.array_equal(ob, ob2) and np.array_equal(oq, oq2) and st == st2
        assert util.md5(fastq.format_fastq(ob, oq, oroff)) == c["out_md5"], (it, c)
        if ref is not None:
            sb.tofile(str(tmp_path / "x.bwt")); sq.tofile(str(tmp_path / "x.bwt.qs"))
            subprocess.check_call([ref, "-e", str(tmp_path / "x.bwt"), "-q", str(tmp_path / "x.bwt.qs"), "-o", str(tmp_path / "o.fq"),
                                   "-m", "2", "-k", str(p.K)], stdout=subprocess.DEVNULL)
            assert util.md5(open(str(tmp_path / "o.fq"), "rb").read()) == c["out_md5"], (it, c)
        done += 1
    assert done >= 6


def _ref_rerun(orc, tmp_path, c, bwt, qs):
    """The compiled reference again, where it is built: (md5 of its output, its eight counters); None where it is not."""
    ref = orc.ref_binary(c["M"], c["B"])
    if ref is None:
        return None
    d = str(tmp_path)
    bwt.tofile(d + "/x.bwt"); qs.tofile(d + "/x.bwt.qs")
    cmd = [ref, "-e", d + "/x.bwt", "-q", d + "/x.bwt.qs", "-o", d + "/o.fq",
           "-k", str(c["k"]), "-m", str(c["m"]), "-v", str(c["v"]), "-t", str(c["t"]), "-f", str(c["f"])]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=120, check=True).stdout
    return util.md5(open(d + "/o.fq", "rb").read()), util.parse_stats(out)


def _stats8(st):
    return {k: st[k] for k in util.STAT_KEYS}


def test_oracle_vs_reference_wide(orc, tmp_path):
    """The oracle over the input space tests/soak_gpu.py draws from, against what the reference bfq_int itself wrote and
    printed there (tests/golden/ref_wide*, made by make_golden.py --ref-wide): collection shapes with plateaus of equal LCP,
    empty / one-base / N-only reads, clusters beyond 2048 rows with two frequent symbols, qualities up to 126 and as raw bytes
    (signed char in the reference), -k 1..39 -m 1..8 -v 33..99 -f 34..100 -t 0..44 in every (M,B) build.  The output's md5
    and all eight counters, in bfq_int mode (LCP deduced from the BWT), with the explicit LCP, and through orc.run_reads."""
    cases, _, _ = util.ref_wide()
    assert len(cases) >= 200 and sum(c["family"] == "raw" for c in cases) == 12
    for c in cases:
        b, q, r = c["bases"], c["quals"], c["roff"]
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        assert util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], c["id"]
        p = orc.params(K=c["k"], m=c["m"], v=c["v"], f=c["f"], t=c["t"], M=c["M"], B=c["B"])
        for given in (None, lcp):
            ob, oq, oroff, st = orc.smooth_invert(bwt, qs, given, p)
            assert util.md5(fastq.format_fastq(ob, oq, oroff)) == c["out_md5"], (c["id"], given is None)
            assert _stats8(st) == c["stats"], (c["id"], given is None)
        ob, oq, st = orc.run_reads(b, q, r, p)
        assert util.md5(fastq.format_fastq(ob, oq, r)) == c["out_md5"] and _stats8(st) == c["stats"], c["id"]
        again = _ref_rerun(orc, tmp_path, c, bwt, qs)
        if again is not None:
            assert again == (c["out_md5"], c["stats"]), c["id"]


def test_oracle_vs_reference_wide_ties(orc, tmp_path):
    """Tie-shuffled eBWTs (identical suffixes and terminator rows in any order) in every (M,B) build and K in {1,2,3,5,8}:
    the oracle's output and counters against the reference's (tests/golden/ref_wide_tie.npz), with its own BWT-only LCP
    deduction and with the LCP of the decoded rows."""
    _, ties, _ = util.ref_wide()
    assert len(ties) == 24 and {(c["M"], c["B"]) for c in ties} == {(M, B) for M in range(4) for B in range(2)}
    assert {c["k"] for c in ties} == {1, 2, 3, 5, 8}
    for c in ties:
        sb, sq = c["bwt"], c["qs"]
        suf, _ = util.decode_rows(sb)
        p = orc.params(K=c["k"], m=c["m"], v=c["v"], f=c["f"], t=c["t"], M=c["M"], B=c["B"])
        for given in (None, util.lcp_of_rows(suf)):
            ob, oq, oroff, st = orc.smooth_invert(sb, sq, given, p)
            assert util.md5(fastq.format_fastq(ob, oq, oroff)) == c["out_md5"], (c["id"], given is None)
            assert _stats8(st) == c["stats"], (c["id"], given is None)
        again = _ref_rerun(orc, tmp_path, c, sb, sq)
        if again is not None:
            assert again == (c["out_md5"], c["stats"]), c["id"]
