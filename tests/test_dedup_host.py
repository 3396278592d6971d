"""Host side of the exact duplicate removal (csrc/bfq_dedup.h): the host form (HostText.fastq_dedup_host) against the
plain-Python statement of the definition (tests/dedup_model.py) -- bytes, every statistic and every refusal's message --, into
guarded buffers of the exact size; what the cases hold, counted on the model alone; and the same code compiled for the host
with sanitizers and run as a program of its own."""
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import dedup_model as M
from tests.test_pairs_host import guarded, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


@pytest.mark.parametrize("name", M.NAMES)
def test_host_form_equals_the_model(name):
    texts, opts = M.all_cases()[name]
    kept, removed, wst = M.expect(name)
    outs, dups, st = host.fastq_dedup_host(texts, dups=True, **opts)
    assert [o.tobytes() for o in outs] == kept and [d.tobytes() for d in dups] == removed, name
    assert st.as_dict() == wst, name
    buf, wins = guarded([len(w) for w in kept + removed])          # into guarded buffers of the exact size
    outs, dups, st = host.fastq_dedup_host(texts, outs=wins[:2], dups=wins[2:], **opts)
    assert [o.tobytes() for o in outs] == kept and [d.tobytes() for d in dups] == removed and untouched(buf, wins) and st.as_dict() == wst, name
    buf, wins = guarded([len(w) for w in kept])                     # the removed records counted, not written
    outs, dups, st = host.fastq_dedup_host(texts, outs=wins, **opts)
    assert [o.tobytes() for o in outs] == kept and dups is None and untouched(buf, wins) and st.as_dict() == wst, name


def test_the_cases_hold_what_they_are_for():
    """by counting, on the model alone"""
    assert M.wide_counts() == (70000, 40000, 40, 70000 - 40000 - sum(3 + (j * 297) // 39 for j in range(40)))
    assert 70000 > 1 << 16 and 5_500_000 < len(M.cases()["wide"][0][0]) < 6_500_000
    wst = M.expect("wide")[2]
    assert (wst["units"], wst["kept"], wst["max_group"], wst["dup_groups"], wst["rounds"]) == (70000, 23999, 40000, 41, 1)
    assert wst["level_groups"][15] == 1 and wst["level_units"][15] == 40000 and wst["level_groups"][0] == 23958
    # every length in its three forms, and the couples are what they are said to be
    cp = M.length_couples()
    assert sorted({len(a) for a, _, _ in cp}) == list(M.LENGTHS) and len(cp) == 4 + 3 * 12
    for a, b, equal in cp:
        assert len(a) == len(b) and (a == b) == equal
        assert equal or a[1:] == b[1:] or a[:-1] == b[:-1]
    lst = M.expect("lengths")[2]
    assert lst["dup_groups"] == sum(e for _, _, e in cp) == 14 and lst["removed"] == 14 and lst["units"] == 2 * len(cp)
    assert M.expect("lengths-mate-2")[2]["removed"] == M.expect("lengths-mate-1")[2]["removed"] == 14
    # the group sizes, in one text, scattered: the largest group's members are not adjacent
    gst = M.expect("groups")[2]
    assert gst["units"] == sum(M.GROUP_SIZES) and gst["kept"] == len(M.GROUP_SIZES) and gst["max_group"] == 4097 > 1024
    assert [gst["level_units"][k] for k in (0, 1, 6, 8, 10, 12)] == [1, 2 + 3, 64 + 65, 256 + 257, 1024 + 1025, 4097]
    assert M.expect("groups~hash_bits=3")[2]["rounds"] >= 2 and M.expect("groups-best~hash_bits=1")[2]["rounds"] >= 3
    assert M.expect("groups-best")[0] != M.expect("groups")[0] and M.expect("groups-best")[2]["kept"] == 10
    # equal full hashes, different sequences: every couple collides (at the same length under any seed), is of the shape it
    # is said to be, and is kept apart with a second round at hash_bits 40 -- single-end, in mate 1 and in mate 2
    cc = M.collide_couples()
    assert sorted({len(a) for a, b, w in cc if w != "prefix"}) == [16, 17, 64, 65, 256, 257] and {w for _, _, w in cc} == {"first", "last", "middle", "prefix"}
    for a, b, what in cc:
        assert a != b and M.name_hash(a) == M.name_hash(b) and M.unit_hash((a, b"ACGTTGCA")) == M.unit_hash((b, b"ACGTTGCA")), what
        assert M.unit_hash((b"ACGTTGCA", a)) == M.unit_hash((b"ACGTTGCA", b)), what
        diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
        if what == "prefix":
            assert b.startswith(a) and len(b) == len(a) + 8
        else:
            assert len(a) == len(b) and M.name_hash(a, 5) == M.name_hash(b, 5)
            assert {"first": diff[-1] < 16, "last": diff[0] >= (len(a) - 1) // 8 * 8 - 8 and diff[-1] >= len(a) // 16 * 16 - (len(a) % 16 == 0),
                    "middle": diff[0] // 16 == 7 and diff[-1] // 16 == 8}[what], (what, len(a), diff)
    tails = [a for a, b, w in cc if w == "last" and len(a) % 16 == 1]
    assert len(tails) == 3 and all(a[-1] != b[-1] for a, b, w in cc if w == "last" and len(a) % 16 == 1)        # the byte behind the last whole step differs
    for name in ("collide", "collide-mate-1", "collide-mate-2"):
        st = M.expect(name)[2]
        assert (st["units"], st["kept"], st["dup_groups"], st["rounds"], st["mixed_runs"], st["max_run"]) == (3 * len(cc), 2 * len(cc), len(cc), 2, len(cc), 3), name
    assert M.expect("collide~hash_bits=40~seed=5")[2]["mixed_runs"] == sum(w != "prefix" for _, _, w in cc) and M.expect("collide~hash_bits=40~seed=5")[2]["rounds"] == 2
    # keys: prefixes, case and N
    kst = M.expect("keys")[2]
    assert kst["kept"] == 12 and kst["removed"] == 3
    # lines: CR LF and LF records of one sequence are equal and leave byte for byte
    kept, removed, lst = M.expect("lines")
    assert lst["kept"] == 3 and kept[0].count(b"\r\n") == 12 and b"@b other" in removed[0] and b"+b\n" in removed[0] and b"@d\n" in removed[0]
    # pairs
    kept, removed, pst = M.expect("pairs-mix")
    assert pst["units"] == 11 and pst["removed"] == 1 and removed[0].startswith(b"@p6/1\n") and removed[1].startswith(b"@p6/2\n")
    # keep: the best unit first, last and in the middle; the rules differ; the kept units stay in input order
    for name in ("keep-first", "keep-last", "keep-middle"):
        kept, removed, st = M.expect(name)
        assert st["max_group"] == 300 and st["kept"] == 101 and b"@best\n" in kept[0] and b"@low\n" in removed[0], name
        heads = [l for l in kept[0].split(b"\n")[0::4] if l]
        order = [l for l in M.cases()[name][0][0].split(b"\n")[0::4] if l in set(heads)]
        assert heads == order, name
    assert b"@best\n" in M.expect("keep-middle-rule-0")[1][0]
    assert b"@best\n" in M.expect("keep-middle-paired")[0][1]
    assert [l for l in M.expect("ties")[0][0].split(b"\n")[0::4] if l] == [b"@t2", b"@t7"]
    assert [l for l in M.expect("ties-rule-0")[0][0].split(b"\n")[0::4] if l] == [b"@t0", b"@t1"]
    # the hash knobs: several rounds at 1 and 3 bits, at most 40 different keys in a run
    for name in M.NAMES:
        opts = M.all_cases()[name][1]
        if name.split("~")[0] in M.VARIED and opts.get("hash_bits", 40) <= 3:
            assert M.expect(name)[2]["rounds"] <= 40, name
    assert M.expect("knobs~hash_bits=1~seed=0")[2]["rounds"] >= 10 and M.expect("knobs~hash_bits=3~seed=5")[2]["rounds"] >= 3
    assert M.expect("knobs~hash_bits=40~seed=5")[2]["rounds"] == 1
    assert len(M.P.records(M.kinds_text())) == 2103


def test_the_hash():
    h = M.unit_hash
    assert h((b"AC", b"G")) != h((b"A", b"CG")) and h((b"ACGT", b"TTTT")) != h((b"TTTT", b"ACGT")) and h((b"ACGT",)) != h((b"ACGT",), 5)
    assert h((b"",)) == M.name_hash(b"") and h((b"A" * 8,)) != h((b"A" * 8 + b"\0",))


def test_refusals_carry_the_models_message_and_write_nothing():
    for name, (texts, opts, code, msg) in M.refusals().items():
        cap = max(len(t) + 1 for t in texts if t is not None)
        buf, wins = guarded([cap] * 4)
        with pytest.raises(api.BfqError) as e:
            host.fastq_dedup_host(texts, outs=wins[:2], dups=wins[2:], **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all() and e.value.needed == [0, 0, 0, 0], name
        with pytest.raises(api.BfqError) as e:
            host.fastq_dedup_host(texts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value), msg)


@pytest.mark.parametrize("name", ("lengths", "pairs-mix", "keep-middle-paired", "lines-paired-nolf"))
def test_a_buffer_one_byte_short(name):
    texts, opts = M.all_cases()[name]
    kept, removed, _ = M.expect(name)
    want = [len(w) for w in kept + removed]
    for short in range(4):
        if not want[short]:
            continue
        buf, wins = guarded([n - (k == short) for k, n in enumerate(want)])
        with pytest.raises(api.BfqError) as e:
            host.fastq_dedup_host(texts, outs=wins[:2], dups=wins[2:], **opts)
        assert e.value.code == -1 and e.value.needed == want and (buf == 0xA5).all(), (name, short)
        assert "output buffer smaller than the text it receives" in str(e.value)


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_dedup_default_opts", "bfq_dedup_host_error", "bfq_fastq_dedup_measure", "bfq_fastq_dedup", "bfq_fastq_dedup_device", "bfq_fastq_dedup_fd",
              "bfq_fastq_dedup_host"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.DedupOpts) == 24 and C.sizeof(_lib.DedupStats) == 616
    o = _lib.DedupOpts(9, 9, 9, (C.c_uint32 * 2)(9, 9))
    L.bfq_dedup_default_opts(C.byref(o))
    assert (o.keep, o.hash_bits, o.seed, o.reserved[0], o.reserved[1]) == (0, 40, 0, 0, 0)
    d = api.dedup_opts()
    assert (d.keep, d.hash_bits, d.seed, d.reserved[0], d.reserved[1]) == (0, 40, 0, 0, 0)


def test_the_tool_is_built():
    assert os.access(os.path.join(ROOT, "dropin", "bfq_dedup"), os.X_OK)


def test_dedup_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_dedup")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_dedup.cpp")])
    lines, files = [], {}

    def put(data):
        if data is None:
            return "-"
        if data not in files:
            files[data] = str(tmp_path / ("f%d" % len(files)))
            with open(files[data], "wb") as f:
                f.write(data)
        return files[data]

    def words(o):
        r = o.get("reserved", (0, 0))
        return "%d %d %d %d %d" % (o.get("keep", 0), o.get("hash_bits", 40), o.get("seed", 0), r[0], r[1])

    for name in M.NAMES:
        texts, opts = M.all_cases()[name]
        kept, removed, st = M.expect(name)
        stats = " ".join(str(st[k]) for k in ("kept", "removed", "dup_groups", "max_group", "max_group_first", "mixed_runs", "max_run", "rounds"))
        lines.append("dedup %s %s %s %s %s" % (put(texts[0]), put(texts[1]), words(opts), " ".join(put(w) for w in kept + removed), stats))
    for name, (texts, opts, code, msg) in M.refusals().items():
        lines.append("bad %s %s %s %s %d" % (put(texts[0]), put(texts[1]), words(opts), put(msg.encode()), code))
    man = str(tmp_path / "manifest")
    with open(man, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert b"%d cases, 0 failures" % len(lines) in r.stdout
