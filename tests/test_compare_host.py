"""The compare model (tests/compare_model.py, the statement of bfq_fastq_compare) against facts that need no GPU: the
reference-made goldens, and the oracle's own counters."""
import os
import numpy as np
import pytest
from bfqzip_amd import fastq
from tests import compare_model as cm, util

NAMES = ("example", "paired", "synth_fix", "synth_var")
# golden input -> reference-made *.M2B0.fq (-m 5): reads, bases, bases changed, qualities changed
TABLE = {"example": (100, 10100, 10, 4131), "paired": (200, 20200, 0, 19),
         "synth_fix": (1500, 90000, 429, 53565), "synth_var": (2000, 89495, 598, 19286)}


def golden_pair(name):
    rd = lambda f: open(os.path.join(util.GOLDEN, f), "rb").read()
    return rd(name + ".fastq"), rd(name + ".M2B0.fq")


def check_invariants(R):
    assert int(R["subst"].sum()) == R["total_bases"] == int(R["pos_len"].sum()) == int(R["qual_hist_a"].sum()) == int(R["qual_hist_b"].sum())
    assert R["headers_same"] + R["headers_dropped"] + R["headers_changed"] == R["n_reads"]
    assert int(R["pos_bases"].sum()) == R["bases_changed"] == int(R["changed_base_qual_hist"].sum())
    assert int(R["pos_quals"].sum()) == R["quals_changed"] == R["quals_raised"] + R["quals_lowered"]
    assert int(R["pos_abs"].sum()) == R["qual_abs_sum"]
    assert max(R["bases_changed"], R["quals_changed"]) <= R["n_diffs"] <= R["bases_changed"] + R["quals_changed"]


@pytest.mark.parametrize("name", NAMES)
def test_model_reproduces_the_golden_table(name):
    a, b = golden_pair(name)
    R = cm.compare([a], [b], max_diffs=5)
    assert (R["n_reads"], R["total_bases"], R["bases_changed"], R["quals_changed"]) == TABLE[name]
    check_invariants(R)
    assert R["headers_changed"] == 0                         # the goldens were written without --headers: "@", as some inputs have it
    assert len(R["diffs"]) == min(5, R["n_diffs"]) and (R["n_diffs"] == 0 or int(R["diffs"]["read"][0]) == R["first_changed_read"])


@pytest.mark.parametrize("m", (5, 2))
@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_oracle_counters(orc, name, m):
    """What the oracle says it did is what the compare finds: every base replacement shows (modified), a quality rewrite
    may have written the value that stood there (qs_smoothed counts it, the compare does not)."""
    b, q, r, h = fastq.read_fastq(os.path.join(util.GOLDEN, name + ".fastq"))
    ob, oq, st = orc.run_reads(b, q, r, orc.params(m=m, M=2, B=0))
    a = open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read()
    R = cm.compare([a], [fastq.format_fastq(ob, oq, r, h)])
    assert R["bases_changed"] == st["modified"]
    assert R["quals_changed"] <= st["qs_smoothed"]
    check_invariants(R)
    assert R["headers_same"] == R["n_reads"]
    if (name, m) == ("example", 5):
        assert (R["quals_changed"], st["qs_smoothed"]) == (4131, 4198)
    if (name, m) == ("paired", 2):
        assert (R["quals_changed"], st["qs_smoothed"]) == (307, 585)


def test_model_refusals_name_what_the_library_must_name():
    rec = lambda i, L: b"@r%d\n%s\n+\n%s\n" % (i, b"A" * L, b"I" * L)
    a = b"".join(rec(i, 20) for i in range(50))
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [b"".join(rec(i, 20) for i in range(49))])
    assert e.value.kind == "counts" and e.value.counts == (50, 49)
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [b"".join(rec(i, 21 if i in (37, 12) else 20) for i in range(50))])
    assert e.value.kind == "length" and e.value.index == 12 and e.value.lens == (20, 21)
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [a[:-3] + b"\n"])
    assert e.value.kind == "text" and e.value.which == "B"
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [a], perm=np.arange(51))
    assert e.value.kind == "perm_n" and e.value.counts == (51, 50)
    p = np.arange(50); p[30] = 4
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [a], perm=p)
    assert e.value.kind == "perm_entry" and e.value.index == 30


def test_model_pairs_through_the_permutation_and_ignores_part_cuts():
    rng = np.random.default_rng(5)
    b, q, r = util.random_reads(rng, 40, 5, 90)
    a = fastq.format_fastq(b, q, r, None)
    q2 = q.copy(); q2[::7] = 35
    bt = fastq.format_fastq(b, q2, r, None)
    recs = [bt[s:e] for s, e in zip(*_record_spans(bt))]
    perm = rng.permutation(40)
    shuffled = b"".join(recs[int(v)] for v in perm)          # record j of B is record perm[j] of A's order
    cut = int(_record_spans(a)[0][17])
    R0, R1 = cm.compare([a], [bt], max_diffs=1000), cm.compare([a[:cut], a[cut:-1]], [shuffled], perm=perm, max_diffs=1000)
    for k in cm.SCALARS:
        assert R0[k] == R1[k], k
    for k in cm.ARRAYS + ("diffs",):
        assert np.array_equal(R0[k], R1[k]), k


def _record_spans(text):
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    ends = nl[3::4] + 1
    return np.concatenate([[0], ends[:-1]]), ends
