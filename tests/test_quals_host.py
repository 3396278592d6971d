"""The BFQQUAL1 container on the host: the Python statement (tests/quals_model.py) round-trips, pays on the shaped stream,
refuses what it must, and the library's host-only entry points read a container the statement made.  No GPU needed."""
import os
import re
import subprocess
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import quals_model as qm, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qm.cases()


def golden_quals():
    return b"".join(open(os.path.join(util.GOLDEN, "synth_var.M2B0.fq"), "rb").readlines()[3::4])


@pytest.mark.parametrize("name", list(CASES) + ["golden_synth_var"])
def test_model_round_trips(name):
    data = CASES[name] if name in CASES else golden_quals()
    assert qm.eligible(data)
    c = qm.container(data)
    assert c[:8] == b"BFQQUAL1" and qm.decode(c) == data
    assert qm.choose(data, always=True) == c
    top = qm.container(data, rung=3)                               # every feature of the context in use
    assert int.from_bytes(top[44:48], "little") == 3 and qm.decode(top) == data


def test_cases_hold_what_the_format_has_to_get_right():
    lens, vals = qm.split(CASES["variable_with_empty_lines"])
    assert lens[0] == 0 and lens[-1] == 0 and lens.max() <= 150
    lens, _ = qm.split(CASES["long_read_then_empty_segments"])
    p = qm.parts(CASES["long_read_then_empty_segments"])
    assert lens.max() == 5000 and p.nseg == 5 and p.seg_bytes[1:4] == [0, 0, 0] and p.seg_bytes[4] > 0 and lens[-1] == 0
    assert qm.parts(CASES["one_line_of_65535"]).maxlen == 65535
    assert qm.parts(CASES["maxlen_below_16"]).maxlen < 16
    assert qm.parts(CASES["alphabet_of_1"]).A == 1 and qm.parts(CASES["alphabet_of_64"]).A == 64 and qm.parts(CASES["binned_8_levels"]).A == 8
    lens, vals = qm.split(CASES["delta_crosses_8_32_128"])
    alphabet = np.unique(vals)
    rank = np.zeros(256, np.int64); rank[alphabet] = np.arange(len(alphabet))
    d4 = qm.features(rank[vals], lens, len(alphabet), int(lens.max()))[4]
    assert set(d4[:int(lens[0])].tolist()) == {0, 1, 2, 3}


def test_context_statement():
    """The features of one read, spelled out: ranks 0 3 3 1 over an alphabet of 4, maxlen 4 (W = 1)."""
    q1, m8, e, p16, d4 = qm.features(np.array([0, 3, 3, 1]), np.array([4]), 4, 4)
    assert q1.tolist() == [0, 0, 3, 3] and m8.tolist() == [0, 0, 0, 6] and e.tolist() == [1, 1, 1, 0]
    assert p16.tolist() == [0, 1, 2, 3] and d4.tolist() == [0, 0, 0, 0]
    assert qm.context(3, 4, q1, m8, e, p16, d4).tolist() == [32, 288, 547, 795]
    assert [qm.rung_rows(r, 40) for r in range(4)] == [40, 1280, 10240, 40960]
    assert qm.rung_max(40, 2_000_000) == 1 and qm.rung_max(40, 200_000) == 0 and qm.rung_max(8, 2_000_000) == 3
    assert qm.sample_step(2 ** 25 + 2 ** 20) == 2 and qm.sample_step(2 ** 25 - 1) == 1 and qm.sample_step(2 ** 40) == 64
    # a coarser rung's counts are sums of a finer rung's
    cnt = np.arange(qm.rung_rows(3, 3) * 3).reshape(-1, 3)
    for r in range(4):
        assert qm.collapse(cnt, 3, r, 3).sum() == cnt.sum() and len(qm.collapse(cnt, 3, r, 3)) == qm.rung_rows(r, 3)
    assert np.array_equal(qm.collapse(qm.collapse(cnt, 3, 2, 3), 2, 1, 3), qm.collapse(cnt, 3, 1, 3))


def test_checksum_is_the_codecs(orc):
    for data in (b"", b"I", CASES["one_read"], CASES["binned_8_levels"]):
        z = qm.general(data)
        assert int.from_bytes(z[36:44], "little") == qm.checksum(data)


def test_shaped_stream_comes_out_smaller():
    data = qm.shaped(20000, 100, 7)
    p = qm.parts(data)
    c, g = p.bytes(), qm.general(data)
    print("shaped 20000 x 100: general", len(g), "BFQQUAL1", len(c), "rung", p.rung)
    assert p.rung >= 1 and len(c) < len(g) and qm.choose(data) == c


def test_eligibility():
    for name, data in qm.ineligible_cases().items():
        assert not qm.eligible(data) and qm.choose(data, always=True) == qm.general(data), name
    assert qm.eligible(b"I\n") and not qm.eligible(b"") and not qm.eligible(b"\n")
    assert qm.eligible(b"I" * 65535 + b"\n") and not qm.eligible(b"I" * 65536 + b"\n")
    rnd = qm.lines_of(np.random.default_rng(1).integers(33, 73, 300).reshape(3, 100))
    assert qm.eligible(rnd) and qm.choose(rnd) == qm.general(rnd)    # 300 random values: the general container stays


def test_model_refuses_what_the_decoder_must_refuse():
    good, cases = qm.refusal_cases()
    assert qm.decode(qm.container(good, rung=1)) == good
    assert len(cases) == 41
    for name, blob in cases.items():
        with pytest.raises(qm.Damaged):
            qm.decode(blob)


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "bfqzip_hip.h")).read()
    declared = set(re.findall(r"\b(bfq_quals_\w+)\s*\(bfq_ctx", header))
    assert declared == {"bfq_quals_compress", "bfq_quals_compress_device"}
    L = _lib.lib()
    for s in declared:
        assert s in _lib.SYMBOLS and getattr(L, s) is not None


def test_host_entry_points_read_a_model_made_container(orc):
    """bfq_stream_raw_len and bfq_fastq_restore_bound are host only: they take a BFQQUAL1 member beside the others."""
    L = _lib.lib()
    qs = CASES["variable_with_empty_lines"]
    c = np.frombuffer(qm.container(qs, rung=2), np.uint8)
    assert L.bfq_stream_raw_len(api._ptr(c), len(c)) == len(qs)
    more = CASES["one_read"]
    both = np.concatenate([c, np.frombuffer(qm.general(more), np.uint8), c])
    assert L.bfq_stream_raw_len(api._ptr(both), len(both)) == 2 * len(qs) + len(more)
    dna = orc.codec_encode(np.frombuffer(qs.translate(bytes(10 if b == 10 else 65 for b in range(256))), np.uint8))
    bound = L.bfq_fastq_restore_bound(api._ptr(dna), len(dna), api._ptr(c), len(c), None, 0)
    assert bound >= 2 * len(qs)
    assert L.bfq_stream_raw_len(api._ptr(c), len(c) - 1) == -1
    _, cases = qm.refusal_cases()
    for name in ("S", "scale", "A_0", "A_65", "rung_4", "nseg", "nvals", "raw_len", "alphabet_not_ascending", "alphabet_with_newline", "cut", "cut_in_the_table"):
        bad = np.frombuffer(cases[name], np.uint8)
        assert L.bfq_stream_raw_len(api._ptr(bad), len(bad)) == -1, name


def test_job_fields_keep_their_places():
    import ctypes as C
    J = _lib.FastqJob
    assert J.qual_codec.offset == J.hdr_bytes.offset + 8 and J.qual_codec.size == 4 and J.reserved1.offset == J.qual_codec.offset + 4
    assert J.name_codec.offset == J.compress_streams.offset + 4 and J.dna_bytes.offset == J.compress_streams.offset + 8
    assert C.sizeof(J) == J.reserved1.offset + 4 and C.sizeof(J) % 8 == 0


def test_kernels_emulated_on_the_cpu_under_sanitizers(tmp_path):
    """tests/cxx/emu_quals.cpp: the kernels of k_quals.hip compiled for the host and run single-threaded as a program of its own
    with -fsanitize=address,undefined.  Counts, every segment's stream and the decoded bytes must equal the statement's, and
    the decoder must stay inside its shares on a payload damaged at one byte after another."""
    text = open(os.path.join(ROOT, "bfqzip_amd", "csrc", "k_quals.hip")).read()
    a, b = text.index("#define QL_S"), text.index("// ---- host side")
    assert 0 < a < b
    open(tmp_path / "k_quals_kernels.inc", "w").write(text[a:b])
    exe = str(tmp_path / "emu_quals")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(tmp_path),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "emu_quals.cpp")])
    good, _ = qm.refusal_cases()
    streams = dict(CASES, golden_synth_var=golden_quals(), refusal_base=good)
    for name in ("variable_with_empty_lines", "long_read_then_empty_segments", "one_line_of_65535", "maxlen_below_16", "delta_crosses_8_32_128",
                 "alphabet_of_1", "alphabet_of_64", "binned_8_levels", "one_read", "golden_synth_var", "refusal_base"):
        data = streams[name]
        lens, vals = qm.split(data)
        alphabet = np.unique(vals)
        rank = np.zeros(256, np.int64); rank[alphabet] = np.arange(len(alphabet))
        feats = qm.features(rank[vals], lens, len(alphabet), int(lens.max()))
        for rung in ((0, 1, 2, 3) if len(data) < 20000 else (3,)):
            d = tmp_path / ("%s_%d" % (name, rung))
            os.makedirs(d)
            open(d / "in.bin", "wb").write(data)
            open(d / "cont.bin", "wb").write(qm.container(data, rung))
            key = qm.context(rung, len(alphabet), *feats) * len(alphabet) + rank[vals]
            np.bincount(key, minlength=qm.rung_rows(rung, len(alphabet)) * len(alphabet)).astype("<u4").tofile(d / "cnt.bin")
            r = subprocess.run([exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert r.returncode == 0 and r.stdout.startswith(b"ok "), (name, rung, r.stdout[-2000:])
