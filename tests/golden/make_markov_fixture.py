#!/usr/bin/env python3
"""Witnesses for filt's Markov models (build container only: `main` compiles and runs the REFERENCE's own lib/src/markov_model.cc).

markov_witness.cc (beside this file, own code) is compiled in a scratch directory against that file of the reference checkout,
unchanged, behind three stub Boost headers written into that directory (boost/algorithm/string.hpp with an ASCII to_upper_copy,
boost/exception/all.hpp, boost/lexical_cast.hpp).  Committed under tests/golden/markov/: cases.json (per case the eight models'
size() after training and again after scoring) and <case>.u64 (every getScore result of every row, the doubles' bits, little-endian,
[rows, 14] in the order of SCORE_NAMES; NOT_ASKED where setRow does not ask).  The genomes are NOT committed: `genomes` makes them
again from the seeds, and the tests import everything from here (importing this module touches neither the reference nor a device).

What the reference's code says here is the Markov part alone: training, sizes, scores.  The strings it is given are cut by `windows`
and `training_strings` below, a plain-Python restatement of faidx_fetch_seq's clamp (deps/htslib-1.3/faidx.c:455-459), of
SeqUtils::reverseComplement and of the coordinates of junction.cc:1331-1346, 1365-1374 and model_features.cc:81-158; and
`compose` states junction.cc:1353-1356, 1376-1378 and the two isEmpty gates of model_features.cc:198-204.

The cases (CASES, JUNCTIONS):
  * the 16-bit gate of markov_model.cc:36, `(uint16_t)s.size() > order + 1`: introns of 65 539 and 65 542 bases (left out of the
    intron model) and of 65 543 bases (counted in full) on a 70 kb contig; training strings of 6 bases (left out) and of 7 (counted),
    made by the clamp at a contig's end;
  * the no_count penalty: donor windows with no_count 2 (no penalty) and 3 (the first), planted as near-copies of a training window,
    and an untrained F model beside a trained T model (no_count = every step);
  * code 4 as context and as next base: N, IUPAC letters (U among them: its complement is A) and lower-case stretches in the windows;
  * both strands, on contig 0 and on contig 1; a 90-base contig 1 on which every coding window is clamped, windows of 5 bases or
    fewer (log 1 = 0), position windows of one base, and -- on a contig of no bases, the only place where the clamp leaves begin past
    end -- empty windows;
  * the position sentinel: a base never seen at some position gives exactly -300;
  * untrained models of every kind; an untrained PosMarkovModel has size 0 before a 24-base window is scored and 23 after.
KmerMarkovModel's -100 needs a product of probabilities that underflows to zero: with windows of at most 81 bases that asks for
factors near 1e-4, hence contexts seen ten thousand times and more -- no small fixture reaches it, and none here pretends to.

Rows with a position window of one base or none come first: isPWModelEmpty() looks at maps that every earlier row's lookups have
grown, so behind a longer window of an untrained model they would be scored differently than in front of it.

Never run by a test or by build().

    python tests/golden/make_markov_fixture.py        (needs /root/reference)
"""
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "markov")

MODEL_NAMES = ["exon", "intron", "donor_t", "donor_f", "acceptor_t", "acceptor_f", "donor_pw", "acceptor_pw"]
# one row of <case>.u64: model, window
SCORE_NAMES = [("donor_pw", "donor"), ("acceptor_pw", "acceptor"), ("donor_t", "donor"), ("donor_f", "donor"), ("acceptor_t", "acceptor"),
               ("acceptor_f", "acceptor"), ("exon", "left_exon"), ("intron", "left_exon"), ("intron", "left_intron"), ("exon", "left_intron"),
               ("intron", "right_intron"), ("exon", "right_intron"), ("exon", "right_exon"), ("intron", "right_exon")]
WINDOW_NAMES = ["donor", "acceptor", "left_exon", "left_intron", "right_intron", "right_exon"]
NOT_ASKED = 0x7FF8000000000BAD  # a NaN no getScore returns: calcCodingPotential is not called while a coding model is empty
POS, NEG = 0, 1  # consensus strand, as ROW_DTYPE's cons_strand holds it

SEEDS = [9301, 9302, 9303]
P_ROW = 5  # the junction whose donor window the planted copies repeat


def genomes():
    """The contigs, as they are uploaded (soft-masked, IUPAC letters in place): 0 = 1500 bases, 1 = 90 bases, 2 = 70 000 bases (the
    long introns; training only), 3 = no bases."""
    def rand(seed, n):
        return np.random.RandomState(seed).choice(list("ACGT"), n).tolist()
    g0 = rand(SEEDS[0], 1500)
    for i in range(300, 420):                      # a soft-masked stretch
        g0[i] = g0[i].lower()
    g0[500:512] = "N" * 12                         # a run of N, and single ones
    g0[530], g0[547] = "N", "n"
    for k, c in enumerate("RYKMSWBDHVUXryu"):      # IUPAC letters, three bases apart
        g0[600 + 3 * k] = c
    g0[5] = "N"                                    # inside the windows the clamp at the contig's start cuts short
    don = g0[697:721]                              # the donor window of JUNCTIONS[P_ROW]
    g0[997:1021] = don                             # two copies: the last base but one / but two changed -> no_count 2 / 3
    g0[997 + 22] = "ACGT"[("ACGT".index(don[22]) + 1) % 4]
    g0[1197:1221] = don
    g0[1197 + 21] = "ACGT"[("ACGT".index(don[21]) + 1) % 4]
    g1 = rand(SEEDS[1], 90)
    for i in range(20, 36):
        g1[i] = g1[i].lower()
    g1[10], g1[50], g1[60], g1[86] = "R", "N", "u", "N"
    g2 = rand(SEEDS[2], 70000)
    g2[40000:40003] = "NNN"
    return ["".join(g0), "".join(g1), "".join(g2), ""]


# (refid, start, end, consensus strand)
JUNCTIONS = [
    (3, 10, 50, POS),       # 0  a contig of no bases: every window is empty
    (1, 95, 120, POS),      # 1  past the end of contig 1: both position windows are its last base
    (1, 95, 120, NEG),      # 2
    (1, 95, 99, POS),       # 3  donor window one base, acceptor window 11; the 201-base exon windows are the whole contig
    (0, 2, 60, POS),        # 4  left exon: one base
    (0, 700, 820, POS),     # 5  P_ROW
    (0, 705, 900, NEG),     # 6
    (0, 310, 400, POS),     # 7  soft-masked
    (0, 330, 415, NEG),     # 8
    (0, 505, 580, POS),     # 9  N run
    (0, 495, 560, NEG),     # 10
    (0, 610, 700, POS),     # 11 IUPAC
    (0, 615, 660, NEG),     # 12
    (0, 1000, 1100, POS),   # 13 donor window = P_ROW's but for its last base but one
    (0, 1200, 1300, POS),   # 14 ... but for its last base but two
    (0, 6, 90, POS),        # 15 left exon: 5 bases
    (0, 7, 95, NEG),        # 16 left exon: 6 bases, also as a training string
    (0, 8, 100, POS),       # 17 left exon: 7 bases
    (0, 1400, 1495, POS),   # 18 right exon: 4 bases
    (0, 1380, 1493, NEG),   # 19 right exon: 6 bases
    (1, 30, 60, POS),       # 20 contig 1: every coding window clamped
    (1, 25, 70, NEG),       # 21
    (1, 87, 89, POS),       # 22 donor window 6 bases
    (1, 86, 88, POS),       # 23 donor window 7 bases
    (1, 3, 40, NEG),        # 24 acceptor (the left window) clamped at the start
    (2, 500, 540, POS),     # 25 intron of 41 bases
    (2, 1000, 66538, POS),  # 26 65 539
    (2, 2000, 67541, NEG),  # 27 65 542
    (2, 3000, 68542, POS),  # 28 65 543
    (2, 69000, 69950, NEG),  # 29 right windows clamped at the end of contig 2
]
_SMALL = list(range(1, 25))  # the rows on contigs 0 and 1
# rows: the rows scored, None = all; cp / passing / failing: the training sets, as indices into JUNCTIONS
CASES = [
    dict(name="all", rows=None, cp=_SMALL + [25], passing=_SMALL[0::2] + [25], failing=_SMALL[1::2] + [29]),
    dict(name="gate_skipped", rows=None, cp=[25, 26, 27], passing=[5, 6], failing=[7]),
    dict(name="gate_counted", rows=None, cp=[25, 28], passing=[5, 6], failing=[7]),
    dict(name="one_pass", rows=None, cp=[], passing=[P_ROW], failing=[]),
    dict(name="fail_only", rows=None, cp=[16, 21], passing=[], failing=[5, 8, 20, 24]),
    dict(name="intron_gated", rows=None, cp=[26, 27], passing=[6, 12, 21], failing=[9, 11]),  # exon model trained, intron model empty
    dict(name="short6", rows=None, cp=[16], passing=[22], failing=[22]),
    dict(name="short7", rows=None, cp=[17], passing=[23], failing=[23]),
    dict(name="none", rows=None, cp=[], passing=[], failing=[]),
    dict(name="none_one_row", rows=[P_ROW], cp=[], passing=[], failing=[]),
]

_COMPLEMENT = dict(zip("ACGTUDHMNRSVWXY", "TGCAAHDKNYWBSXR"))  # every other letter, K and B among them, has no entry in the reference's table


def fetch(genome, beg, end):
    """GenomeMapper::fetchBases(name, beg, end) on a contig held in memory: faidx_fetch_seq's clamp, both ends inclusive.  On a contig
    of no bases the reference would seek to offset -1; here, as in the project, the answer is no bases."""
    n = len(genome)
    if n == 0:
        return ""
    if end < beg:
        beg = end
    beg = 0 if beg < 0 else (n - 1 if n <= beg else beg)
    end = 0 if end < 0 else (n - 1 if n <= end else end)
    return genome[beg:end + 1]


def revcomp(s):
    """SeqUtils::reverseComplement.  The reference's table has entries for upper-case letters only (a lower-case one indexes past its
    end), so the bases are upper-cased first, as the project does; a letter the table holds no complement for becomes N here, the
    reference's NUL being one more character that makeClean turns into N."""
    return "".join(_COMPLEMENT.get(c, "N") for c in reversed(s.upper()))


def oriented(genome, beg, end, strand):
    s = fetch(genome, beg, end)
    return revcomp(s) if strand == NEG else s


def splice_windows(genome, start, end, strand):
    """(donor, acceptor): junction.cc:1365-1374, model_features.cc:116-131"""
    left = oriented(genome, start - 3, start + 20, strand)
    right = oriented(genome, end - 20, end + 2, strand)
    return (right, left) if strand == NEG else (left, right)


def windows(g, junction):
    """The six strings setRow has scored for a junction, in the order of WINDOW_NAMES (junction.cc:1331-1346, 1365-1374)"""
    refid, start, end, strand = junction
    don, acc = splice_windows(g[refid], start, end, strand)
    return [don, acc, oriented(g[refid], start - 82, start - 2, strand), oriented(g[refid], start, start + 80, strand),
            oriented(g[refid], end - 80, end, strand), oriented(g[refid], end + 1, end + 81, strand)]


def training_strings(g, case):
    """model name -> the strings trainCodingPotentialModel / trainSplicingModels hand to train() (model_features.cc:81-158)"""
    t = {m: [] for m in MODEL_NAMES}
    for k in case["cp"]:
        refid, start, end, strand = JUNCTIONS[k]
        t["exon"].append(oriented(g[refid], start - 202, start - 2, strand))
        t["intron"].append(oriented(g[refid], start, end, strand))
        t["exon"].append(oriented(g[refid], end + 1, end + 201, strand))
    for key, names in (("passing", ("donor_pw", "donor_t", "acceptor_pw", "acceptor_t")), ("failing", ("donor_f", "acceptor_f"))):
        for k in case[key]:
            refid, start, end, strand = JUNCTIONS[k]
            don, acc = splice_windows(g[refid], start, end, strand)
            for nm in names:
                t[nm].append(don if nm.startswith("donor") else acc)
    return t


def case_rows(case):
    """the indices into JUNCTIONS of the rows a case scores"""
    return list(range(len(JUNCTIONS))) if case["rows"] is None else list(case["rows"])


def witness_input(g, cases):
    """The text markov_witness / markov_witness_check read"""
    out = [f"cases {len(cases)}"]
    for case in cases:
        out.append("case " + case["name"])
        t = training_strings(g, case)
        for m in MODEL_NAMES:
            out.append(f"train {len(t[m])}")
            out += t[m]
        rows = case_rows(case)
        out.append(f"rows {len(rows)}")
        for k in rows:
            out += windows(g, JUNCTIONS[k])
    return "\n".join(out) + "\n"


def parse_output(text):
    """What the witness program printed: name -> dict(trained=[8], scored=[8], bits=uint64 [rows, 14])"""
    res, cur = {}, None
    for ln in text.splitlines():
        p = ln.split()
        if p[0] == "case":
            cur = res[p[1]] = dict(trained=None, scored=None, bits=[])
        elif p[0] in ("trained", "scored"):
            cur[p[0]] = [int(v) for v in p[1:]]
        else:
            assert p[0] == "row" and int(p[1]) == len(cur["bits"]) and len(p) == 16
            cur["bits"].append([NOT_ASKED if v == "-" else int(v, 16) for v in p[2:]])
    for r in res.values():
        r["bits"] = np.array(r["bits"], dtype=np.uint64).reshape(-1, 14)
    return res


def load_cases():
    """cases.json as committed (what the tests read): a list of dict(name, trained, scored), sizes in the order of MODEL_NAMES"""
    with open(os.path.join(OUT, "cases.json")) as f:
        return json.load(f)["cases"]


def load_bits(name):
    """uint64 [rows, 14]: the bits of the case's scores"""
    return np.fromfile(os.path.join(OUT, name + ".u64"), dtype="<u8").reshape(-1, 14)


def compose(case, bits, trained, g):
    """Columns 11, 12 and 13 of the case's rows from the witness's scores, float64 [rows, 3], in the reference's order of operations
    (junction.cc:1353-1356 and 1376-1378, left to right), behind isCodingPotentialModelEmpty / isPWModelEmpty as setRow asks them:
    the sizes are those of the maps when the row is reached, which the lookups of the rows before it have grown."""
    s = bits.view(np.float64)
    out = np.zeros((len(s), 3))
    don_size, acc_size = trained[6], trained[7]
    for r, k in enumerate(case_rows(case)):
        don, acc = windows(g, JUNCTIONS[k])[:2]
        don_size, acc_size = max(don_size, len(don) - 1), max(acc_size, len(acc) - 1)   # positions 1 .. len-1 are looked up
        if bits[r, 6] != NOT_ASKED:
            out[r, 0] = (s[r, 6] - s[r, 7]) + (s[r, 8] - s[r, 9]) + (s[r, 10] - s[r, 11]) + (s[r, 12] - s[r, 13])
        if don_size > 0 and acc_size > 0:
            out[r, 1] = s[r, 0] + s[r, 1]
            out[r, 2] = (s[r, 2] - s[r, 3]) + (s[r, 4] - s[r, 5])
    return out


def exact_rows(bits):
    """bool [rows, 3]: the composed columns whose every term is exact on any machine -- a sentinel (-100, -300) or log 1 = 0 -- so
    that no libm takes part in them"""
    s = bits.view(np.float64)
    ok = (bits == NOT_ASKED) | (s == 0.0) | (s == -300.0) | (s == -100.0)
    return np.stack([ok[:, 6:].all(axis=1), ok[:, :2].all(axis=1), ok[:, 2:6].all(axis=1)], axis=1)


def assert_columns(got, want, exact, rel):
    """got, want: float64 [rows, 3].  Bit for bit where `exact` says so, elsewhere within rel * max(1, |want|)."""
    assert got.shape == want.shape == exact.shape
    same = got.view(np.uint64) == want.view(np.uint64)
    assert same[exact].all(), ("not bit-equal", np.argwhere(exact & ~same)[:5].tolist())
    d = np.abs(got - want)
    bad = np.argwhere(~(d <= rel * np.maximum(1.0, np.abs(want))))
    assert bad.size == 0, (bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return float(d.max())


def junction_rows(dtype, indices):
    """Rows of `dtype` (the oracle's ROW_DTYPE or the device's) for the junctions `indices`; the columns 11 to 13 read none of the
    other fields, which hold small valid numbers"""
    rows = np.zeros(len(indices), dtype=dtype)
    for r, k in enumerate(indices):
        rows["refid"][r], rows["start"][r], rows["end"][r], rows["cons_strand"][r] = JUNCTIONS[k]
    rows["nb_raw"], rows["nb_rel"], rows["nb_dist"] = 10, 5, 4
    if "mean_readlen" in dtype.names:
        rows["mean_readlen"] = 100.0
    return rows


STUBS = {
    "boost/algorithm/string.hpp": """#pragma once
#include <string>
namespace boost {
inline std::string to_upper_copy(const std::string &s) {
    std::string r(s);
    for (auto &c : r) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return r;
}
}
""",
    "boost/exception/all.hpp": """#pragma once
#include <exception>
#include <stdexcept>
#include <string>
namespace boost {
struct exception { virtual ~exception() {} };
template <class Tag, class T> struct error_info { T v; error_info(const T &x) : v(x) {} };
template <class E, class Tag, class T> const E &operator<<(const E &e, const error_info<Tag, T> &) { return e; }
}
#define BOOST_THROW_EXCEPTION(x) throw std::runtime_error("witness: exception")
""",
    "boost/lexical_cast.hpp": """#pragma once
#include <sstream>
#include <string>
namespace boost {
template <class T, class S> T lexical_cast(const S &s) { std::stringstream ss; ss << s; T t; ss >> t; return t; }
}
""",
}


def build_witness(d):
    """markov_witness in the directory d; returns its path"""
    for name, text in STUBS.items():
        os.makedirs(os.path.dirname(os.path.join(d, name)), exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            f.write(text)
    exe = os.path.join(d, "markov_witness")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-w", f"-I{d}", f"-I{REF}/lib/include", "-include", "cmath", "-include", "boost/exception/all.hpp",
                           "-o", exe, os.path.join(HERE, "markov_witness.cc"), os.path.join(REF, "lib", "src", "markov_model.cc")])
    return exe


def _no_count(train, s):
    """how many steps of s an order-5 model trained on `train` has no entry for (only to assert that the cases are what they say)"""
    seen = {t[i - 5:i + 1].upper() for t in train if (len(t) & 0xFFFF) > 6 for i in range(5, len(t))}
    return sum(s[i - 5:i + 1].upper() not in seen for i in range(5, len(s)))


def main():
    os.makedirs(OUT, exist_ok=True)
    g = genomes()
    with tempfile.TemporaryDirectory() as d:
        exe = build_witness(d)
        with open(os.path.join(d, "in.txt"), "w") as f:
            f.write(witness_input(g, CASES))
        res = parse_output(subprocess.check_output([exe, os.path.join(d, "in.txt")], text=True))
    by = {c["name"]: c for c in CASES}
    size = {n: dict(zip(MODEL_NAMES, r["trained"])) for n, r in res.items()}
    after = {n: dict(zip(MODEL_NAMES, r["scored"])) for n, r in res.items()}
    score = {n: r["bits"].view(np.float64) for n, r in res.items()}
    # the cases are what the docstring says they are
    lens = {k: [len(w) for w in windows(g, JUNCTIONS[k])] for k in range(len(JUNCTIONS))}
    assert lens[0] == [0] * 6 and lens[1][:2] == [1, 1] and lens[2][:2] == [1, 1] and lens[3][:2] == [1, 11]
    assert lens[4][2] == 1 and lens[15][2] == 5 and lens[16][2] == 6 and lens[17][2] == 7 and lens[18][5] == 4 and lens[22][0] == 6 and lens[23][0] == 7
    assert all(n < 81 for k in (20, 21) for n in lens[k][2:]) and lens[5][:2] == [24, 23]
    t6, t7 = training_strings(g, by["short6"]), training_strings(g, by["short7"])
    assert sorted(map(len, t6["exon"])) == [6, 201] and sorted(map(len, t7["exon"])) == [7, 201]
    assert [len(s) for s in t6["donor_t"]] == [6] and [len(s) for s in t7["donor_t"]] == [7]
    assert size["short6"]["donor_t"] == 0 and size["short7"]["donor_t"] == 2 and size["short6"]["donor_pw"] == 5
    for t, sz, more in ((t6, size["short6"], 0), (t7, size["short7"], 2)):
        long = max(t["exon"], key=len).upper()
        assert sz["exon"] == len({long[i - 5:i] for i in range(5, len(long))}) + more, "6 bases add nothing, 7 bases two contexts"
    assert [len(s) for s in training_strings(g, by["gate_skipped"])["intron"]] == [41, 65539, 65542]
    assert [len(s) for s in training_strings(g, by["gate_counted"])["intron"]] == [41, 65543]
    assert size["gate_skipped"]["intron"] <= 36 and size["gate_counted"]["intron"] > 1000, "markov_model.cc:36 cuts the length to 16 bits"
    tp = training_strings(g, by["one_pass"])["donor_t"]
    w = {k: windows(g, JUNCTIONS[k])[0] for k in (5, 13, 14)}
    assert (_no_count(tp, w[5]), _no_count(tp, w[13]), _no_count(tp, w[14])) == (0, 2, 3)
    rows = case_rows(by["one_pass"])
    sc = score["one_pass"]
    assert sc[rows.index(5), 2] == 0.0 and sc[rows.index(13), 2] == 0.0 and sc[rows.index(14), 2] == np.log(1.0 / 1.5)
    assert sc[rows.index(5), 3] == np.log(1.0 / (19 * 0.5)), "an untrained F model: no_count is every step"
    assert size["one_pass"]["donor_f"] == 0 and after["one_pass"]["donor_f"] > 0 and (res["one_pass"]["bits"][:, 6:] == NOT_ASKED).all()
    assert (score["all"][:, :2] == -300.0).any() and (np.isfinite(score["all"]) & (score["all"] < 0) & (score["all"] > -100)).any()
    assert not (score["all"] == -100.0).any()
    assert res["none_one_row"]["trained"] == [0] * 8 and res["none_one_row"]["scored"][6:] == [23, 22]
    assert res["intron_gated"]["trained"][0] > 0 and res["intron_gated"]["trained"][1] == 0 and res["fail_only"]["trained"][6:] == [0, 0] and res["fail_only"]["trained"][0] > 0
    for name, r in res.items():
        assert r["bits"].shape == (len(case_rows(by[name])), 14)
        r["bits"].astype("<u8").tofile(os.path.join(OUT, name + ".u64"))
        print(f"{name}: trained {r['trained']}, scored {r['scored']}")
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(cases=[dict(name=c["name"], trained=res[c["name"]]["trained"], scored=res[c["name"]]["scored"]) for c in CASES]), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
