"""The BFQNAME1 container on the host: the Python statement (tests/names_model.py) round-trips, pays where the issue says
it pays and loses where it says it loses, refuses what it must, and the library's host-only entry points read a container
the statement made.  No GPU needed."""
import os
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import names_model as nm, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example_names():
    return b"".join(open(os.path.join(util.GOLDEN, "example.fastq"), "rb").readlines()[0::4])


def test_model_round_trips_random_lines():
    rng = np.random.default_rng(20261018)
    for n in (1, 2, 255, 256, 257, 700):
        data = nm.random_stream(rng, n)
        index, ops, num, text = nm.transform(data)
        assert len(index) == 16 * ((n + nm.R - 1) // nm.R)
        assert nm.decode(nm.container(data)) == data, n
    # the stream the parametrised sizes are drawn from holds what the format has to get right
    data = nm.random_stream(np.random.default_rng(3), 3000)
    lines = data.split(b"\n")[:-1]
    assert b"" in lines and any(len(nm.tokens(x)) >= 600 for x in lines)
    runs = [len(t) for x in lines for t in nm.tokens(x) if t[:1].isdigit()]
    assert min(r for r in runs if r >= 15) == 15 and max(runs) >= 25 and 18 in runs and 19 in runs
    assert nm.decode(nm.container(data)) == data


@pytest.mark.parametrize("name", list(nm.edge_cases()))
def test_model_round_trips_the_edge_cases(name):
    data = nm.edge_cases()[name]
    assert nm.eligible(data)
    assert nm.decode(nm.container(data)) == data
    assert nm.choose(data, always=True) == nm.container(data)


def test_model_statement_of_the_operations():
    """The streams of a few lines, spelled out."""
    T, D, I, E, S = nm.TEXT, nm.DELTA, nm.INC, nm.END, nm.SAME
    index, ops, num, text = nm.transform(b"@r.9 x\n@r.10 x\n@r.10 x\n@r.7 y\n007 5\n")
    assert ops == bytes([T, D, T, E, S + 1, I, S + 1, E, S + 3, E, S + 1, D, T, E, T, T, D, E])
    assert num == nm.leb(18) + nm.leb(5) + nm.leb(10)                   # 9 - 0, 7 - 10 -> 2 * 3 - 1, 5 - 0 (" y" is no number)
    assert text == b"\x03@r.\x02 x\x02 y\x03007\x01 "
    # a run of 600 SAME tokens: 240, 240, 120
    _, ops, _, _ = nm.transform(nm.edge_cases()["same_600"])
    second = ops[ops.index(E) + 1:]
    assert second[:4] == bytes([S + 240, S + 240, S + 120, E])
    assert second[4:] == bytes([S + 240, S + 240, S + 119, I, E])       # ... a1 -> ... a2
    # 18 digits are a number, 19 digits and leading zeros are text; the empty line against which a group starts has no tokens
    _, ops, num, _ = nm.transform(b"123456789012345678\n1234567890123456789\n" + b"5\n" * 255)
    assert ops[:4] == bytes([D, E, T, E]) and ops[4:6] == bytes([D, E])
    _, ops, _, _ = nm.transform(b"5\n" * 257)
    assert ops == bytes([D, E]) + bytes([S + 1, E]) * 255 + bytes([D, E])


@pytest.mark.parametrize("family", ["sra", "illumina", "syn"])
def test_families_come_out_smaller(family):
    data = {"sra": nm.sra_names, "illumina": nm.illumina_names, "syn": nm.syn_names}[family](30000)
    c, g = nm.container(data), nm.general(data)
    print(family, "general", len(g), "BFQNAME1", len(c))
    assert len(c) < len(g) and nm.choose(data) == c
    assert nm.decode(c) == data


def test_fallback_cases_do_not_come_out_smaller():
    for name, data in (("300 @SYN names", nm.syn_names(300)), ("3000 random 40-byte lines", nm.random_lines(3000, 40)),
                       ("names of example.fastq", _example_names())):
        c, g = nm.container(data), nm.general(data)
        print(name, "general", len(g), "BFQNAME1", len(c))
        assert len(c) >= len(g) and nm.choose(data) == g, name
        assert nm.decode(c) == data
    for name, data in nm.ineligible_cases().items():
        assert not nm.eligible(data) and nm.choose(data, always=True) == nm.general(data), name


def test_model_refuses_what_the_decoder_must_refuse():
    good, cases = nm.refusal_cases()
    assert nm.decode(nm.container(good)) == good
    assert len(cases) == 7
    for name, blob in cases.items():
        with pytest.raises(nm.Damaged):
            nm.decode(blob)


def test_host_entry_points_read_a_model_made_container(orc):
    """bfq_stream_raw_len and bfq_fastq_restore_bound are host only: they take a BFQNAME1 member beside the others."""
    L = _lib.lib()
    names = nm.sra_names(600)
    c = np.frombuffer(nm.container(names), np.uint8)
    assert c[:8].tobytes() == b"BFQNAME1"
    assert L.bfq_stream_raw_len(api._ptr(c), len(c)) == len(names)
    # two members back to back, the second one of another kind
    more = nm.syn_names(50)
    both = np.concatenate([c, np.frombuffer(nm.general(more), np.uint8)])
    assert L.bfq_stream_raw_len(api._ptr(both), len(both)) == len(names) + len(more)
    dna = orc.codec_encode(np.frombuffer(b"ACGTACGTAC\n" * 600, np.uint8))
    qs = orc.codec_encode(np.frombuffer(b"IIIIIIIIII\n" * 600, np.uint8))
    bound = L.bfq_fastq_restore_bound(api._ptr(dna), len(dna), api._ptr(qs), len(qs), api._ptr(c), len(c))
    assert bound >= len(names) + 600 * (11 + 2 + 11)
    # what is no container stays refused: a header that lies about its members, a truncated container, a nested one
    _, cases = nm.refusal_cases()
    bad = np.frombuffer(cases["member_lengths"], np.uint8)
    assert L.bfq_stream_raw_len(api._ptr(bad), len(bad)) == -1
    assert L.bfq_stream_raw_len(api._ptr(c), len(c) - 1) == -1
    assert L.bfq_fastq_restore_bound(api._ptr(dna), len(dna), api._ptr(qs), len(qs), api._ptr(c), len(c) - 1) == -1
    nested = bytearray(c.tobytes())
    nested[64:72] = b"BFQNAME1"
    nested = np.frombuffer(bytes(nested), np.uint8)
    assert L.bfq_stream_raw_len(api._ptr(nested), len(nested)) == -1


def test_job_field_keeps_its_place():
    import ctypes as C
    assert _lib.FastqJob.name_codec.offset == _lib.FastqJob.compress_streams.offset + 4
    assert _lib.FastqJob.name_codec.size == 4 and _lib.FastqJob.dna_bytes.offset == _lib.FastqJob.compress_streams.offset + 8
    assert C.sizeof(_lib.FastqJob) % 8 == 0
