#!/usr/bin/env python3
"""Witnesses for self-training's nearest neighbours, SMOTE, ENN and under-sampling (build container only: `main` compiles and runs
the REFERENCE's own lib/src/{knn,smote,enn}.cc).

knn_witness.cc (beside this file, own code) is compiled in a scratch directory against those three files of the reference checkout,
unchanged, behind two stub Boost headers written into that directory (boost/exception/all.hpp, boost/timer/timer.hpp).  Committed
under tests/golden/selftrain/: the neighbour lists (<case>.nn.npy, uint32 [rows, k]), SMOTE's synthetic rows (<case>.synth.u64: the
doubles' bits, little-endian), ENN's keep mask (<case>.keep.u8), the under-sampling survivors (<case>.left.npy) and cases.json.
The matrices are NOT committed: `case_matrix` makes them again from the seeds, and the tests import it from here (importing this
module touches neither the reference nor the device).

This file also holds the Python restatement of what the reference draws, which the tests pin against the witness: std::mt19937 and
libstdc++ 11's uniform_int_distribution / uniform_real_distribution on it (bits/uniform_int_dist.h, bits/random.tcc).

Never run by a test or by build().

    python tests/golden/make_knn_fixture.py        (needs /root/reference)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "selftrain")
SEED = 12345  # the seed of every generator of trainInstance's balancing

KNN_CASES = [
    # 40 rows are copies of others: ties between a row, its copy and itself
    dict(name="K700", kind="normal", rows=700, cols=28, k=5, rng=8101, copies=40),
    # fewer rows than defaultK: KNN's constructor takes k = rows
    dict(name="R1", kind="normal", rows=1, cols=28, k=5, rng=8111),
    dict(name="R2", kind="normal", rows=2, cols=28, k=5, rng=8112),
    dict(name="R3", kind="normal", rows=3, cols=28, k=5, rng=8113),
    dict(name="R4", kind="normal", rows=4, cols=28, k=5, rng=8114),
    dict(name="R5", kind="normal", rows=5, cols=28, k=5, rng=8115),
    # the edges of a wave of 64 test rows
    dict(name="E63", kind="normal", rows=63, cols=28, k=3, rng=8121),
    dict(name="E64", kind="normal", rows=64, cols=28, k=3, rng=8122),
    dict(name="E65", kind="normal", rows=65, cols=28, k=3, rng=8123),
    dict(name="E129", kind="normal", rows=129, cols=28, k=3, rng=8124),
    # small integers: masses of equal distances, the index order decides
    dict(name="I1", kind="ints", rows=200, cols=1, k=5, rng=8131),
    dict(name="I32", kind="ints", rows=200, cols=32, k=5, rng=8132),
    # several chunks of the base range
    dict(name="C2500", kind="normal", rows=2500, cols=28, k=5, rng=8141, copies=25),
    # the anchors of tests/knn_model.py beyond k = 5 and the compiled widths: whole lists of 8, a width between 28 and 32, and
    # small integers in one and in two columns -- far more than 8 base rows at one distance, lying in several chunks of 64
    dict(name="K8", kind="normal", rows=200, cols=28, k=8, rng=8151, copies=10),
    dict(name="C31", kind="normal", rows=200, cols=31, k=5, rng=8152),
    dict(name="T1", kind="ints", rows=300, cols=1, k=8, rng=8153, chunk=64),
    dict(name="T2", kind="ints", rows=300, cols=2, k=8, rng=8154, chunk=64),
]
SMOTE_CASES = [
    dict(name="S120", kind="normal", rows=120, cols=28, smoteness=2, rng=8201, copies=6),
    dict(name="S3", kind="normal", rows=3, cols=28, smoteness=3, rng=8202),  # k = 3: the integer draw is over 0..2
]
ENN_CASES = [dict(name="N400", kind="blobs", rows=400, cols=28, rng=8301)]
# the first 180 draws of mt19937(12345) never hit the end of the vector, whatever its size; the 240 of U300b do, once
UNDER_CASES = [dict(name="U300", size=300, keep=120), dict(name="U300b", size=300, keep=60)]


def case_matrix(case):
    """The case's matrix, float64 [rows, cols]."""
    rng = np.random.RandomState(case["rng"])
    n, c = case["rows"], case["cols"]
    if case["kind"] == "ints":
        return rng.randint(0, 3, (n, c)).astype(np.float64)
    if case["kind"] == "blobs":  # two overlapping clouds: ENN keeps some rows of each label and discards some
        m = rng.normal(0.0, 1.0, (n, c))
        m[case_labels(case) == 1, :4] += 1.5
        return m
    m = rng.normal(0.0, 1.0, (n, c)) * rng.uniform(0.5, 40.0, c)
    for _ in range(case.get("copies", 0)):
        a, b = rng.randint(0, n, 2)
        m[a] = m[b]
    return m


def case_labels(case):
    """uint8 [rows]: the labels of an ENN case"""
    return (np.random.RandomState(case["rng"] + 1).uniform(size=case["rows"]) < 0.6).astype(np.uint8)


def load_cases():
    """cases.json as committed (what the tests read)"""
    with open(os.path.join(OUT, "cases.json")) as f:
        return json.load(f)


def path(name):
    return os.path.join(OUT, name)


def knn_order(m, k):
    """The k smallest of every row under (squared distance, index): columns summed in ascending order, each step rounded."""
    n = len(m)
    s = np.zeros((n, n))
    for c in range(m.shape[1]):
        d = m[None, :, c] - m[:, None, c]
        s = s + d * d
    return np.argsort(s, axis=1, kind="stable")[:, :k].astype(np.uint32), np.sort(s, axis=1)[:, :k]


class Mt19937:
    """std::mt19937"""

    def __init__(self, seed):
        self.s = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            x = self.s[-1]
            self.s.append((1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF)
        self.at = 624

    def __call__(self):
        s = self.s
        if self.at >= 624:
            for i in range(624):
                y = (s[i] & 0x80000000) | (s[(i + 1) % 624] & 0x7FFFFFFF)
                s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.at = 0
        y = s[self.at]
        self.at += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y


def uniform_int(gen, hi):
    """uniform_int_distribution<T>(0, hi) of libstdc++ 11 on a 32-bit generator, hi < 2^32 - 1: Lemire's multiply-high with a
    rejection threshold (_S_nd<uint64_t>)"""
    rng = hi + 1
    prod = gen() * rng
    low = prod & 0xFFFFFFFF
    if low < rng:
        thr = ((1 << 32) - rng) % rng
        while low < thr:
            prod = gen() * rng
            low = prod & 0xFFFFFFFF
    return prod >> 32


def uniform_real(gen):
    """uniform_real_distribution<double>(0, 1): generate_canonical<double, 53> takes two draws, the low word first"""
    lo = float(gen())
    s = lo + float(gen()) * 4294967296.0
    r = s / 18446744073709551616.0
    return r if r < 1.0 else float(np.nextafter(1.0, 0.0))


def smote(m, nn, smoteness):
    """Smote::execute (lib/src/smote.cc:43-69) on the matrix m and its neighbour lists nn [rows, k]: float64 [smoteness * rows, cols]"""
    gen = Mt19937(SEED)
    k = nn.shape[1]
    out = np.empty((max(smoteness, 1) * len(m), m.shape[1]))
    at = 0
    for i in range(len(m)):
        for _ in range(max(smoteness, 1)):
            j = int(nn[i, uniform_int(gen, k - 1)])
            for c in range(m.shape[1]):
                dif = m[j, c] - m[i, c]
                gap = uniform_real(gen)
                out[at, c] = m[i, c] + gap * dif
            at += 1
    return out


def enn_keep(nn, labels):
    """ENN::execute with setThreshold(3) on k = 3 lists: a row stays iff all of its neighbours (itself among them) carry its label"""
    same = labels[nn.astype(np.int64)] == labels[:, None]
    return (same.sum(axis=1) >= 3).astype(np.uint8)


def undersample(size, keep):
    """model_features.cc:289-294 on the indices 0..size-1 with `keep` positives: the survivors, and how many draws hit the end
    (vector::erase(end()) of libstdc++ destroys the last element)"""
    gen = Mt19937(SEED)
    left = list(range(size))
    at_end = 0
    while len(left) > keep:
        i = uniform_int(gen, len(left))  # inclusive upper bound
        if i == len(left):
            at_end += 1
            left.pop()
        else:
            del left[i]
    return np.array(left, dtype=np.uint32), at_end


STUBS = {
    "boost/exception/all.hpp": """#pragma once
#include <exception>
#include <stdexcept>
namespace boost {
struct exception { virtual ~exception() {} };
template <class Tag, class T> struct error_info { T v; error_info(const T &x) : v(x) {} };
template <class E, class Tag, class T> const E &operator<<(const E &e, const error_info<Tag, T> &) { return e; }
}
#define BOOST_THROW_EXCEPTION(x) throw std::runtime_error("witness: exception")
""",
    "boost/timer/timer.hpp": """#pragma once
namespace boost { namespace timer { struct auto_cpu_timer { auto_cpu_timer(int, const char *) {} }; } }
""",
}


def build_witness(d):
    """knn_witness in the directory d; returns its path"""
    for name, text in STUBS.items():
        os.makedirs(os.path.dirname(os.path.join(d, name)), exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            f.write(text)
    exe = os.path.join(d, "knn_witness")
    srcs = [os.path.join(REF, "lib", "src", s) for s in ("knn.cc", "smote.cc", "enn.cc")]
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-w", f"-I{d}", f"-I{REF}/lib/include", f"-I{REF}/deps/ranger-0.3.8/include", "-o", exe,
                           os.path.join(HERE, "knn_witness.cc")] + srcs + ["-lpthread"])
    return exe


def main():
    os.makedirs(OUT, exist_ok=True)
    rec = dict(seed=SEED, knn=[], smote=[], enn=[], under=[])
    with tempfile.TemporaryDirectory() as d:
        exe = build_witness(d)
        mat, out = os.path.join(d, "m.f64"), os.path.join(d, "out.bin")

        def run(*args):
            return subprocess.check_output([exe] + [str(a) for a in args], text=True).split()[-1]

        for case in KNN_CASES:
            m = case_matrix(case)
            assert m.shape == (case["rows"], case["cols"])
            m.astype("<f8").tofile(mat)
            lists = {}
            for threads in (1, 3, 7) if case["rows"] >= 7 else (1,):
                k = int(run("knn", mat, case["rows"], case["cols"], case["k"], threads, out))
                lists[threads] = np.fromfile(out, dtype="<u4").reshape(case["rows"], k)
            nn = lists[1]
            assert all(np.array_equal(nn, v) for v in lists.values()), "the reference's lists depend on its thread count"
            assert nn.shape[1] == min(case["k"], case["rows"])
            order, dist = knn_order(m, nn.shape[1])
            assert np.array_equal(nn, order), "the reference's lists are not in (distance, index) order"
            ties = int(sum(len(np.unique(r)) < len(r) for r in dist))
            np.save(path(case["name"] + ".nn.npy"), nn)
            more = {}
            if "chunk" in case:  # (stated by the model of tests/knn_model.py, which the tests hold against these very lists)
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import knn_model
                more["rows_tied_across_chunks"] = knn_model.rows_tied_across_chunks(m, nn.shape[1], case["chunk"])
            rec["knn"].append(dict(case, k_used=int(nn.shape[1]), rows_with_equal_distances=ties, **more))
            print(f"{case['name']}: {nn.shape}, {ties} rows with equal distances in their list")
        for case in SMOTE_CASES:
            m = case_matrix(case)
            m.astype("<f8").tofile(mat)
            n_synth = int(run("smote", mat, case["rows"], case["cols"], case["smoteness"], out))
            synth = np.fromfile(out, dtype="<f8").reshape(n_synth, case["cols"])
            k = int(run("knn", mat, case["rows"], case["cols"], 5, 1, out))
            nn = np.fromfile(out, dtype="<u4").reshape(case["rows"], k)
            assert np.array_equal(smote(m, nn, case["smoteness"]).view(np.uint64), synth.view(np.uint64)), "the restatement of Smote::execute"
            synth.view("<u8").tofile(path(case["name"] + ".synth.u64"))
            np.save(path(case["name"] + ".nn.npy"), nn)
            rec["smote"].append(dict(case, k_used=k, synthetic_rows=n_synth))
            print(f"{case['name']}: {n_synth} synthetic rows, k = {k}")
        for case in ENN_CASES:
            m, lab = case_matrix(case), case_labels(case)
            m.astype("<f8").tofile(mat)
            lab.tofile(os.path.join(d, "lab.u8"))
            discard = int(run("enn", mat, case["rows"], case["cols"], os.path.join(d, "lab.u8"), out))
            keep = np.fromfile(out, dtype=np.uint8)
            k = int(run("knn", mat, case["rows"], case["cols"], 3, 1, out))
            nn = np.fromfile(out, dtype="<u4").reshape(case["rows"], k)
            assert discard == int((keep == 0).sum()) and np.array_equal(enn_keep(nn, lab), keep), "the restatement of ENN::execute"
            for label in (0, 1):
                assert 0 < keep[lab == label].sum() < (lab == label).sum(), "ENN must keep some and discard some rows of each label"
            keep.tofile(path(case["name"] + ".keep.u8"))
            np.save(path(case["name"] + ".nn.npy"), nn)
            rec["enn"].append(dict(case, kept=int(keep.sum())))
            print(f"{case['name']}: {int(keep.sum())} of {len(keep)} rows kept")
        for case in UNDER_CASES:
            at_end = int(run("under", case["size"], case["keep"], out))
            left = np.fromfile(out, dtype="<u4")
            mine, mine_end = undersample(case["size"], case["keep"])
            assert len(left) == case["keep"] and np.array_equal(mine, left) and mine_end == at_end, "the restatement of the under-sampling"
            np.save(path(case["name"] + ".left.npy"), left)
            rec["under"].append(dict(case, draws_at_end=at_end))
            print(f"{case['name']}: {len(left)} survivors, {at_end} draw(s) hit the end")
        assert any(c["draws_at_end"] for c in rec["under"]), "no draw hit the end of the vector: choose another size"
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
