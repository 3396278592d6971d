#!/usr/bin/env python3
"""Regenerates tests/golden/ from the REFERENCE itself (run in the build container only).

Inputs : example/reads.fastq of the reference (a data file) and two seeded
         synthetic sets (bfq_synth_host of libbfqhip.so, host code only).
eBWT   : built by the oracle's suffix sorter (gsufsort is an absent submodule);
         pinned by the round trip `reference bfq_int -k 10000` == input reads.
Outputs: FASTQ written by the reference bfq_int compiled by oracle/Makefile into
         oracle/_ref/ (one binary per -DM/-DB), for every (M,B) and a few flag sets.
Only data is stored: inputs, eBWT/QS/LCP bytes, expected FASTQ (or its md5).
"""
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from bfqzip_amd import api, fastq
from oracle import orc

REF = "/root/reference"


def run_ref(M, B, bwt, qs, flags, headers=None):
    with tempfile.TemporaryDirectory() as d:
        open(d + "/x.bwt", "wb").write(bwt.tobytes()); open(d + "/x.bwt.qs", "wb").write(qs.tobytes())
        cmd = [orc.ref_binary(M, B), "-e", d + "/x.bwt", "-q", d + "/x.bwt.qs", "-o", d + "/o.fq"] + flags
        if headers is not None:
            open(d + "/x.h", "wb").write(b"".join(h + b"\n" for h in headers))
            cmd += ["-H", d + "/x.h"]
        subprocess.check_call(cmd, stdout=subprocess.DEVNULL, timeout=120)
        return open(d + "/o.fq", "rb").read()


def main():
    orc.build()
    sets = {}
    b, q, r, h = fastq.read_fastq(REF + "/example/reads.fastq")
    sets["example"] = (b, q, r, h)
    b1, q1, r1, h1 = fastq.read_fastq(REF + "/example/reads_1.fastq")
    b2, q2, r2, h2 = fastq.read_fastq(REF + "/example/reads_2.fastq")
    sets["paired"] = (np.concatenate([b1, b2]), np.concatenate([q1, q2]),
                      np.concatenate([r1, r2[1:] + r1[-1]]), h1 + h2)   # BFQzip_parallel.py:325-360 appends mate block
    sp = api.synth_spec(2000, 30, Lmax=60, seed=11, coverage=30, err_ppm=20000, n_ppm=15000, snp_every=97, dsnp_every=131)
    sets["synth_var"] = api.synth_host(sp) + (None,)
    sp = api.synth_spec(1500, 60, seed=12, coverage=30)
    sets["synth_fix"] = api.synth_host(sp) + (None,)
    index = {}
    for name, (b, q, r, h) in sets.items():
        open(f"{HERE}/{name}.fastq", "wb").write(fastq.format_fastq(b, q, r, h))
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        open(f"{HERE}/{name}.bwt", "wb").write(bwt.tobytes())
        open(f"{HERE}/{name}.bwt.qs", "wb").write(qs.tobytes())
        open(f"{HERE}/{name}.lcp16", "wb").write(lcp.astype(np.uint16).tobytes())
        ent = {"n": int(len(bwt)), "reads": int(len(r) - 1), "bwt_md5": hashlib.md5(bwt.tobytes()).hexdigest(),
               "qs_md5": hashlib.md5(qs.tobytes()).hexdigest(), "out": {}}
        # identity: the reference inverts our eBWT back to the input (pins the step-1 contract)
        ident = run_ref(2, 0, bwt, qs, ["-k", "10000"])
        assert ident == fastq.format_fastq(b, q, r, None), name
        cases = [(M, B, ["-m", "5"]) for M in range(4) for B in range(2)]
        cases += [(2, 0, ["-m", "2"]), (2, 0, ["-m", "5", "-k", "8", "-v", "53", "-t", "35", "-f", "50"]),
                  (1, 1, ["-m", "3", "-k", "3", "-t", "5"]), (0, 0, ["-m", "9", "-k", "5", "-f", "70", "-v", "73"])]
        for M, B, flags in cases:
            out = run_ref(M, B, bwt, qs, flags)
            key = f"M{M}B{B} " + " ".join(flags)
            ent["out"][key] = hashlib.md5(out).hexdigest()
            if (M, B) == (2, 0) and flags == ["-m", "5"]:
                open(f"{HERE}/{name}.M2B0.fq", "wb").write(out)
        if h is not None:
            out = run_ref(2, 0, bwt, qs, ["-m", "5"], headers=h)
            ent["out"]["M2B0 -m 5 -H"] = hashlib.md5(out).hexdigest()
        index[name] = ent
        print(name, ent["n"], len(ent["out"]))
    json.dump(index, open(f"{HERE}/index.json", "w"), indent=1, sort_keys=True)
    ref_cases()
    ref_wide()


def ref_cases():
    """ref_cases.npz / ref_cases.json: the random small inputs of tests/test_oracle_golden.py's two differential tests
    (the same seeded draws those tests once made live) with the md5 of the reference bfq_int's output for each."""
    from tests import util
    arrays, meta = {}, {"fuzz": [], "tie": []}
    rng = np.random.default_rng(7)
    for it in range(60):
        nreads = int(rng.integers(1, 120)); lmax = int(rng.integers(1, 50))
        b, q, r = util.random_reads(rng, nreads, 1, lmax)
        M, B = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        K = int(rng.choice([1, 2, 3, 5, 8, 16])); m = int(rng.choice([2, 3, 5, 9]))
        v = int(rng.choice([62, 53, 73])); t = int(rng.choice([5, 20, 35])); f = int(rng.choice([40, 50, 70]))
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        out = run_ref(M, B, bwt, qs, ["-k", str(K), "-m", str(m), "-v", str(v), "-t", str(t), "-f", str(f)])
        arrays[f"fuzz{it}_bases"], arrays[f"fuzz{it}_quals"], arrays[f"fuzz{it}_roff"] = b, q, np.asarray(r, np.uint64)
        meta["fuzz"].append({"M": M, "B": B, "K": K, "m": m, "v": v, "t": t, "f": f,
                             "bwt_md5": util.md5(bwt.tobytes()), "qs_md5": util.md5(qs.tobytes()), "out_md5": util.md5(out)})
    rng = np.random.default_rng(99)
    for it in range(12):
        b, q, r = util.random_reads(rng, int(rng.integers(5, 60)), 1, int(rng.integers(4, 40)), dup=0.45, p_n=0.02)
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        sb, sq = util.shuffle_ties(bwt, qs, rng)
        if np.array_equal(sb, bwt):
            continue
        K = int(rng.choice([2, 3, 5]))
        out = run_ref(2, 0, sb, sq, ["-m", "2", "-k", str(K)])
        i = len(meta["tie"])
        arrays[f"tie{i}_bwt"], arrays[f"tie{i}_qs"] = sb, sq
        meta["tie"].append({"K": K, "out_md5": util.md5(out)})
    np.savez_compressed(f"{HERE}/ref_cases.npz", **arrays)
    json.dump(meta, open(f"{HERE}/ref_cases.json", "w"), indent=1, sort_keys=True)
    print("ref_cases", len(meta["fuzz"]), len(meta["tie"]))


# ---- the wide fixture: the input space of tests/soak_gpu.py shown to the reference itself --------------------------------
ACGT = np.array(list(b"ACGT"), np.uint8)
CL_BIG = 2048      # bfq_internal.h: clusters beyond this many rows go to the k_big_* kernels
SEG_BIG = 64       # a run of identical suffixes beyond this many rows counts as a long segment


def stats_block(stdout):
    a = stdout.index(b"**** Cluster statistics ****")
    b = stdout.index(b"**** Bases statistics ****")
    return stdout[a:stdout.index(b"***********************", b)].decode()


def run_ref_stats(M, B, bwt, qs, flags):
    """(output FASTQ, the eight counters, stdout) of the reference bfq_int; a non-zero exit status is an error."""
    with tempfile.TemporaryDirectory() as d:
        bwt.tofile(d + "/x.bwt"); qs.tofile(d + "/x.bwt.qs")
        p = subprocess.run([orc.ref_binary(M, B), "-e", d + "/x.bwt", "-q", d + "/x.bwt.qs", "-o", d + "/o.fq"] + flags,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, (p.returncode, flags, p.stdout[-400:])
        from tests import util
        return open(d + "/o.fq", "rb").read(), util.parse_stats(p.stdout), p.stdout


def _pack(reads, rng, qual=None):
    b = np.concatenate(reads).astype(np.uint8) if sum(len(x) for x in reads) else np.zeros(0, np.uint8)
    q = rng.integers(33, 127, len(b)).astype(np.uint8) if qual is None else qual
    r = np.zeros(len(reads) + 1, np.uint64); r[1:] = np.cumsum([len(x) for x in reads])
    return b, q, r


def _two_frequent(rng, big, trusted):
    """The recipe of test_long_cluster_two_frequent_bases: a cluster whose eBWT symbols are C and G half and half, each with
    its own preceding base, plus a few odd bases: never trusted ones that get replaced and (trusted=True) trusted ones that
    are kept.  big: 2 x 1100 + 2 x 20 reads, the cluster beyond CL_BIG rows."""
    U = ACGT[rng.integers(0, 4, int(rng.integers(3, 5)) if big else int(rng.integers(3, 12)))]
    mk = lambda pre: np.concatenate([np.frombuffer(pre, np.uint8), U])
    a, o = (1100, 20) if big else (int(rng.integers(8, 40)), int(rng.integers(1, 4)))
    reads = [mk(b"AC")] * a + [mk(b"TG")] * a + [mk(b"AT")] * o + [mk(b"TA")] * o
    reads = [reads[i] for i in rng.permutation(len(reads))]
    b, q, r = _pack(reads, rng)
    need = dict(k=len(U), f=int(rng.integers(34, 50)), t=int(rng.integers(1, 45)))
    if trusted:   # the odd A's are trusted and carry exactly the replacement quality (M = 2): `newqs < QUAL[j]` at equality
        need["v"] = int(rng.integers(34, 100)); need["t"] = int(rng.integers(1, min(44, need["v"] - 33) + 1)); need["M"] = 2
    for i, x in enumerate(reads):
        if bytes(x[:2]) in (b"AT", b"TA"):
            q[int(r[i]) + 1] = need["v"] if trusted and bytes(x[:2]) == b"TA" else 33      # 33: below every -t >= 1
    return (b, q, r), need


def wide_gen(fam, i, rng):
    """One collection of family `fam` (the six of tests/soak_gpu.gen scaled down, 'prefix' and 'raw'), qualities 33..126.
    Returns ((bases, quals, roff), parameters this collection needs to show its trait ({} = all free))."""
    from tests import util
    if fam == "rand":         # random small sets with N and duplicates (empty reads: lmin 0)
        b, q, r = util.random_reads(rng, int(rng.integers(1, 110)), 0, int(rng.integers(1, 36)), p_n=float(rng.random() * 0.2),
                                    dup=float(rng.random() * 0.5), qhi=126)
        if i % 5 == 0:        # N-only reads among them
            L = np.diff(r.astype(np.int64))
            for j in np.flatnonzero(rng.random(len(L)) < 0.2):
                b[int(r[j]):int(r[j + 1])] = ord("N")
        return (b, q, r), {}
    if fam == "synth":        # the synthetic generator, fixed or variable length
        L = int(rng.integers(12, 34))
        sp = api.synth_spec(int(rng.integers(30, 120)), L, Lmax=int(L + rng.integers(0, 20)) if rng.random() < 0.5 else None,
                            seed=int(rng.integers(1, 1 << 30)), coverage=int(rng.integers(5, 60)), err_ppm=int(rng.integers(0, 40000)),
                            n_ppm=int(rng.integers(0, 20000)), snp_every=int(rng.integers(50, 2000)), dsnp_every=int(rng.integers(100, 20000)))
        b, q, r = api.synth_host(sp)
        return (b, rng.integers(33, 127, len(b)).astype(np.uint8), r), {}
    reads = []
    if fam == "lowcx":        # homopolymers / short tandem repeats with noise; the first three: one clean homopolymer,
        if i < 3:             # i.e. one cluster and one run of identical suffixes per length beyond every threshold
            reads = [np.full(80, ACGT[i], np.uint8)] * 66
        else:
            for _ in range(int(rng.integers(8, 70))):
                L = int(rng.integers(1, 50)); unit = ACGT[rng.integers(0, 4, int(rng.integers(1, 4)))]
                s = np.resize(unit, L).copy()
                e = rng.random(L) < rng.random() * 0.03; s[e] = ACGT[rng.integers(0, 4, int(e.sum()))]
                s[rng.random(L) < 0.003] = ord("N")
                reads.append(s)
    elif fam == "long":       # a few long reads sharing long stretches
        g = ACGT[rng.integers(0, 4, 3000)]
        for _ in range(int(rng.integers(1, 7))):
            a = int(rng.integers(0, 2000)); reads.append(g[a:a + int(rng.integers(1, 700))].copy())
    elif fam == "tiny":       # tiny genome, huge coverage: long clusters, two-symbol sites; the first twelve by recipe
        if i < 12:
            return _two_frequent(rng, big=i < 4, trusted=i % 2 == 1)
        g = ACGT[rng.integers(0, 4, int(rng.integers(12, 40)))]
        g2 = g.copy(); p = rng.integers(0, len(g), max(1, len(g) // 20)); g2[p] = ACGT[rng.integers(0, 4, len(p))]
        for _ in range(int(rng.integers(30, 150))):
            src = g if rng.random() < 0.5 else g2
            L = int(rng.integers(1, len(g) + 1)); a = int(rng.integers(0, len(g) - L + 1))
            s = src[a:a + L].copy()
            e = rng.random(L) < 0.01; s[e] = ACGT[rng.integers(0, 4, int(e.sum()))]
            reads.append(s)
    elif fam == "empty":      # many empty / one-base reads mixed with ordinary ones (and some N-only reads)
        g = ACGT[rng.integers(0, 4, 120)]
        for _ in range(int(rng.integers(2, 160))):
            x = rng.random()
            if x < 0.3: reads.append(np.zeros(0, np.uint8))
            elif x < 0.5: reads.append(ACGT[rng.integers(0, 4, 1)])
            elif x < 0.56: reads.append(np.full(int(rng.integers(1, 6)), ord("N"), np.uint8))
            else:
                a = int(rng.integers(0, 100)); reads.append(g[a:a + int(rng.integers(2, 30))].copy())
        if not sum(len(x) for x in reads):
            reads.append(ACGT[:1].copy())                          # the reference refuses a collection of empty reads only
    elif fam == "prefix":     # reads that are prefixes or duplicates of others, in large blocks: plateaus of equal LCP
        for _ in range(int(rng.integers(1, 4))):
            s = ACGT[rng.integers(0, 4, int(rng.integers(4, 26)))]
            if rng.random() < 0.3:
                s[int(rng.integers(0, len(s)))] = ord("N")
            for _ in range(int(rng.integers(10, 60))):
                reads.append(s.copy() if rng.random() < 0.5 else s[:int(rng.integers(0 if i % 3 == 0 else 1, len(s) + 1))].copy())
            if i % 4 == 0:
                reads += [s.copy()] * 70                           # one block of duplicates beyond SEG_BIG
        reads = [reads[j] for j in rng.permutation(len(reads))]
    elif fam == "raw":        # qualities as raw bytes (array entry points only): 1..32, 127, 128..255 among normal ones
        (b, q, r), _ = wide_gen("rand", 1, rng)
        pool = [np.arange(1, 33), np.array([127]), np.arange(128, 256), np.concatenate([np.arange(1, 33), [127], np.arange(128, 256)])][(i + i // 4) % 4]
        mask = rng.random(len(q)) < (0.3, 0.6, 1.0)[i // 4]        # the last four: no normal value left
        q = q.copy(); q[mask] = rng.choice(pool, int(mask.sum())).astype(np.uint8)
        return (b, q, r), {}
    return _pack(reads, rng), {}


WIDE_FAMILIES = (("rand", 48), ("synth", 14), ("lowcx", 26), ("long", 14), ("tiny", 32), ("empty", 36), ("prefix", 38), ("raw", 12))
CORNERS = (("k", 1), ("m", 1), ("t", 0), ("t", 44), ("f", 34), ("f", 50), ("f", 100), ("v", 33), ("v", 99))


def _traits(b, r, bwt, lcp, K):
    """What a collection holds, for the generator's own counts (cluster spans by the scan of bfq_int.cpp:685-711)."""
    L = np.diff(r.astype(np.int64))
    n = len(bwt)
    l = lcp.astype(np.int64)
    mn = np.zeros(n, bool)
    if n > 2:
        mn[1:n - 1] = (l[:n - 2] > l[1:n - 1]) & (l[2:] >= l[1:n - 1])
    inn = (l >= K) & ~mn; inn[:1] = False
    d = np.diff(np.concatenate([[0], inn.astype(np.int8), [0]]))
    spans = np.flatnonzero(d == -1) - np.flatnonzero(d == 1) + 1     # rows begin-1 .. i-1
    return dict(max_cluster=int(spans.max(initial=0)), empty=int((L == 0).sum()),
                n_only=int(sum(1 for j in np.flatnonzero(L > 0) if np.all(b[int(r[j]):int(r[j + 1])] == ord("N")))))


def _max_identical_run(b, r):
    """Longest run of identical suffixes: the most frequent suffix string of the collection (small inputs only)."""
    from collections import Counter
    c = Counter()
    for j in range(len(r) - 1):
        s = b[int(r[j]):int(r[j + 1])].tobytes()
        for a in range(len(s) + 1):
            c[s[a:]] += 1
    return max(c.values(), default=0)


def ref_wide():
    """ref_wide_<family>.npz / ref_wide_tie.npz / ref_wide.json: ~220 collections over the input space tests/soak_gpu.py draws
    from (shapes, qualities up to 126 and as raw bytes, -k 1..39 -m 1..8 -v 33..99 -f 34..100 -t 0..44, every M and B) and 24
    tie-shuffled eBWTs, each with the md5 of the reference bfq_int's output and the eight counters it printed."""
    from tests import util
    orc.build()
    meta = {"cases": [], "tie": [], "counts": {}, "sizes": {}}
    rows = 0
    drawn = []
    for fi, (fam, cnt) in enumerate(WIDE_FAMILIES):
        for i in range(cnt):
            rng = np.random.default_rng([20260, fi, i])
            (b, q, r), need = wide_gen(fam, i, rng)
            par = dict(k=int(rng.integers(1, 40)), m=int(rng.integers(1, 9)), v=int(rng.integers(33, 100)), f=int(rng.integers(34, 101)),
                       t=int(rng.integers(0, 45)), M=int(rng.integers(0, 4)), B=int(rng.integers(0, 2)))
            if fam == "raw":
                par["M"] = i % 4                                   # each smoothing mode on each kind of byte
            if (i % 3 or fam == "raw") and "k" not in need:
                # a -k beyond the collection's largest LCP finds no cluster at all and checks the inversion only: one case of
                # three keeps the uniform draw, one folds it into 1..max LCP, one (and the raw bytes) into the lower third of that
                top = int(orc.build_ebwt(b, q, r)[2].max(initial=0))
                par["k"] = 1 + (par["k"] - 1) % max(1, min(39, top if i % 3 == 1 and fam != "raw" else top // 3))
            par.update(need)
            drawn.append((fam, i, b, q, r, par, need))
    for gi, (fam, i, b, q, r, par, need) in enumerate(drawn):      # the corners of the ranges, in five collections each
        key, val = CORNERS[gi % len(CORNERS)]
        if gi % 4 == 0 and key not in need and not (fam == "lowcx" and i < 3):
            par[key] = val
    arrays = {fam: {} for fam, _ in WIDE_FAMILIES}
    cnt = dict(big_cluster=0, big_segment=0, processed=0, processed_big=0, empty_reads=0, n_only_reads=0, modified=0, amb=0)
    for fam, i, b, q, r, par, need in drawn:
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        rows += len(bwt)
        ident = run_ref(2, 0, bwt, qs, ["-k", "10000"])
        assert ident == fastq.format_fastq(b, q, r, None), (fam, i)
        flags = ["-k", str(par["k"]), "-m", str(par["m"]), "-v", str(par["v"]), "-t", str(par["t"]), "-f", str(par["f"])]
        out, st, _ = run_ref_stats(par["M"], par["B"], bwt, qs, flags)
        tr = _traits(b, r, bwt, lcp, par["k"])
        seg = _max_identical_run(b, r) if len(bwt) <= 6000 else 0
        big = tr["max_cluster"] > CL_BIG
        cnt["big_cluster"] += big; cnt["big_segment"] += seg > SEG_BIG
        cnt["processed"] += st["num_clust_mod"] > 0
        cnt["processed_big"] += bool(big and need and st["num_clust_mod"] > 0 and st["modified"] >= 20)   # odd bases of the recipe
        cnt["empty_reads"] += tr["empty"] > 0; cnt["n_only_reads"] += tr["n_only"] > 0
        cnt["modified"] += st["modified"] > 0; cnt["amb"] += st["num_clust_amb_discarded"] > 0
        a = arrays[fam]
        a[f"{i}_bases"], a[f"{i}_quals"], a[f"{i}_len"] = b, q, np.diff(r.astype(np.int64)).astype(np.uint32)
        meta["cases"].append(dict(par, family=fam, i=i, n=int(len(bwt)), reads=int(len(r) - 1), max_cluster=tr["max_cluster"],
                                  bwt_md5=util.md5(bwt.tobytes()), qs_md5=util.md5(qs.tobytes()), out_md5=util.md5(out), stats=st))
    # ties of identical suffixes in any order, all (M,B), K in {1,2,3,5,8}
    rng = np.random.default_rng(2026)
    tie = {}
    while len(meta["tie"]) < 24:
        j = len(meta["tie"])
        b, q, r = util.random_reads(rng, int(rng.integers(5, 60)), 0 if j % 4 == 0 else 1, int(rng.integers(4, 30)), dup=0.45, p_n=0.02, qhi=126)
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        sb, sq = util.shuffle_ties(bwt, qs, rng)
        if np.array_equal(sb, bwt) and np.array_equal(sq, qs):
            continue
        par = dict(k=(1, 2, 3, 5, 8)[j % 5], m=int(rng.integers(1, 6)), v=int(rng.integers(33, 100)), f=int(rng.integers(34, 101)),
                   t=int(rng.integers(0, 45)), M=j % 4, B=j // 4 % 2)
        # identical suffixes swap their (symbol, quality) pairs between reads: the same base lines and the same quality bytes,
        # each as a multiset, is what the inversion of a tie-shuffled eBWT must give back
        parts = lambda t: (sorted(t.split(b"\n")[1::4]), sorted(b"".join(t.split(b"\n")[3::4])))
        assert parts(run_ref(2, 0, sb, sq, ["-k", "10000"])) == parts(fastq.format_fastq(b, q, r, None)), j
        out, st, _ = run_ref_stats(par["M"], par["B"], sb, sq, ["-k", str(par["k"]), "-m", str(par["m"]), "-v", str(par["v"]),
                                                               "-t", str(par["t"]), "-f", str(par["f"])])
        rows += len(sb)
        tie[f"{j}_bwt"], tie[f"{j}_qs"] = sb, sq
        meta["tie"].append(dict(par, n=int(len(sb)), out_md5=util.md5(out), stats=st))
    assert {(c["M"], c["B"]) for c in meta["tie"]} == {(M, B) for M in range(4) for B in range(2)}
    # the statistics block of the example run of the README (dropin/src_int_mem/bfq_int -m 5; tests/test_gpu_cli.py)
    bwt = np.fromfile(f"{HERE}/example.bwt", np.uint8); qs = np.fromfile(f"{HERE}/example.bwt.qs", np.uint8)
    out, st, stdout = run_ref_stats(2, 0, bwt, qs, ["-m", "5"])
    assert out == open(f"{HERE}/example.M2B0.fq", "rb").read()
    meta["example_m5"] = {"stats": st, "block": stats_block(stdout)}
    # what the set must hold
    cases = meta["cases"]
    cnt = {k: int(v) for k, v in cnt.items()}
    cnt["cases"], cnt["tie_cases"], cnt["rows"] = len(cases), len(meta["tie"]), int(rows)
    cnt["families"] = {fam: n for fam, n in WIDE_FAMILIES}
    cnt["corners"] = {f"{k}={v}": sum(1 for c in cases if c[k] == v) for k, v in CORNERS}
    cnt["MB"] = {f"M{M}B{B}": sum(1 for c in cases if (c["M"], c["B"]) == (M, B)) for M in range(4) for B in range(2)}
    meta["counts"] = cnt
    print(json.dumps(cnt, indent=1))
    assert cnt["big_cluster"] >= 6 and cnt["big_segment"] >= 6 and cnt["processed"] >= 10 and cnt["processed_big"] >= 4
    assert cnt["empty_reads"] >= 15 and cnt["n_only_reads"] >= 10 and rows <= 300000
    assert all(v >= 3 for v in cnt["corners"].values()), cnt["corners"]
    assert sum(1 for c in cases if c["family"] == "raw") == 12
    for fam, a in list(arrays.items()) + [("tie", tie)]:
        path = f"{HERE}/ref_wide_{fam}.npz"
        np.savez_compressed(path, **a)
        meta["sizes"][os.path.basename(path)] = os.path.getsize(path)
        assert os.path.getsize(path) <= 256 << 10, path
    json.dump(meta, open(f"{HERE}/ref_wide.json", "w"), indent=1, sort_keys=True)
    assert os.path.getsize(f"{HERE}/ref_wide.json") <= 256 << 10
    print("ref_wide", len(cases), len(meta["tie"]), rows, meta["sizes"])


if __name__ == "__main__":
    if sys.argv[1:] == ["--ref-cases"]:
        ref_cases()
    elif sys.argv[1:] == ["--ref-wide"]:
        ref_wide()
    else:
        main()
