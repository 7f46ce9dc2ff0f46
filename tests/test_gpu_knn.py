"""K nearest neighbours on the device (pjb_knn, kernels kn_* of pjb_knn.hip.h) against the lists the reference's own KNN::doSlice
wrote for the same matrices (tests/golden/selftrain, made by tests/golden/make_knn_fixture.py with the reference's lib/src/knn.cc).
The matrices are made again from the seeds in cases.json.  Every comparison is bit for bit: the lists are indices.

Beyond those lists -- k up to 8, the column counts between the compiled widths, chunks shorter than a list, a last chunk of one row --
the device is compared with tests/knn_model.py, the numpy restatement that tests/test_knn_model.py pins to every list of the
reference without a device; K8, C31, T1 and T2 are the reference's own lists for three of those properties."""
import os
import sys

import numpy as np
import pytest

import knn_model as km

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_knn_fixture as fx  # noqa: E402  (the generator of the matrices; it touches nothing on import)

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in fx.load_cases()["knn"]}


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def ctx(ffi):
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def want():
    """name -> (matrix, the reference's lists); made once, never changed"""
    out = {}
    for name, case in CASES.items():
        m = fx.case_matrix(case)
        nn = np.load(fx.path(name + ".nn.npy"))
        m.setflags(write=False)
        nn.setflags(write=False)
        out[name] = (m, nn)
    return out


def assert_same_lists(got, ref):
    assert got.dtype == np.uint32 and got.shape == ref.shape
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, the first is row {bad[0]}: {got[bad[0]]} instead of {ref[bad[0]]}"


def test_cases_cover_the_issue():
    assert {"K700", "R1", "R2", "R3", "R4", "R5", "E63", "E64", "E65", "E129", "I1", "I32", "C2500", "K8", "C31", "T1", "T2"} == set(CASES)
    assert CASES["K700"]["copies"] == 40 and CASES["K700"]["rows_with_equal_distances"] > 0
    assert CASES["I1"]["rows_with_equal_distances"] == 200 and CASES["I32"]["rows_with_equal_distances"] > 100
    assert (CASES["I1"]["cols"], CASES["I32"]["cols"]) == (1, 32)
    assert (CASES["K8"]["k_used"], CASES["C31"]["cols"], CASES["T1"]["cols"], CASES["T2"]["cols"]) == (8, 31, 1, 2)
    for name in ("T1", "T2"):  # (the count is the model's: tests/test_knn_model.py states it again)
        assert CASES[name]["rows_tied_across_chunks"] == CASES[name]["rows"] == 300 and CASES[name]["chunk"] == 64 and CASES[name]["k_used"] == 8


@pytest.mark.parametrize("name", ["K700", "R1", "R2", "R3", "R4", "R5", "E63", "E64", "E65", "E129", "I1", "I32", "K8", "C31"])
def test_lists_equal_the_reference(ctx, want, name):
    """ties between a row, its copy and itself; fewer rows than k asks for; the edges of a wave; masses of equal distances; whole
    lists of 8; 31 columns padded to 32"""
    m, ref = want[name]
    assert ref.shape == (CASES[name]["rows"], min(CASES[name]["k"], CASES[name]["rows"]))
    assert_same_lists(ctx.knn(m, ref.shape[1]), ref)


def test_every_chunk_size_gives_the_same_lists(ctx, want):
    """2 500 rows in chunks of 64 and of 100 base rows (not a divisor) and in the default chunks: (distance, index) is a total order"""
    m, ref = want["C2500"]
    got = {}
    try:
        for chunk in (64, 100, 0):
            ctx.set_option("knn_chunk", chunk)
            got[chunk] = ctx.knn(m, 5)
    finally:
        ctx.set_option("knn_chunk", 0)
    for chunk, lists in got.items():
        assert_same_lists(lists, ref)


@pytest.mark.parametrize("name", ["T1", "T2"])
def test_equal_distances_spread_over_chunks(ctx, want, name):
    """300 rows of small integers in one and in two columns, chunks of 64 base rows: every row has more than 8 base rows at the
    distance of its eighth neighbour, in several chunks, and the index decides between the chunks' partial lists"""
    m, ref = want[name]
    assert ref.shape == (300, 8)
    try:
        ctx.set_option("knn_chunk", CASES[name]["chunk"])
        got = ctx.knn(m, 8)
    finally:
        ctx.set_option("knn_chunk", 0)
    assert_same_lists(got, ref)
    assert_same_lists(ctx.knn(m, 8), ref)


def model_case(kind, rows, cols, rng):
    m = fx.case_matrix(dict(kind=kind, rows=rows, cols=cols, rng=rng, copies=rows // 20))
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("k", [6, 7, 8])
@pytest.mark.parametrize("rows", [8, 9, 200])
def test_k_above_five_against_the_model(ctx, rows, k):
    """the lists hold 8: as many rows as places, one more, and many"""
    m = model_case("normal", rows, 28, 8400 + rows)
    assert_same_lists(ctx.knn(m, k), km.knn(m, k))


@pytest.mark.parametrize("kind", ["normal", "ints"])
@pytest.mark.parametrize("cols", [2, 27, 29, 31])
def test_column_counts_between_the_compiled_widths(ctx, cols, kind):
    """2 and 27 columns are padded with zeros to 28, 29 and 31 to 32"""
    m = model_case(kind, 150, cols, 8500 + cols)
    assert_same_lists(ctx.knn(m, 8), km.knn(m, 8))


@pytest.fixture(scope="module")
def rows130():
    m = model_case("normal", 130, 28, 8600)
    ref = km.knn(m, 8)
    ref.setflags(write=False)
    return m, ref


@pytest.mark.parametrize("chunk", [1, 3, 7, 8, 43, 129])
def test_chunks_shorter_than_a_list_and_a_last_chunk_of_one_row(ctx, rows130, chunk):
    """130 rows, k = 8: chunks of 1, 3 and 7 base rows leave partial lists with empty places, 8 fills them exactly; chunks of 43
    and of 129 leave a last chunk of one row"""
    m, ref = rows130
    assert chunk not in (43, 129) or 130 % chunk == 1
    try:
        ctx.set_option("knn_chunk", chunk)
        got = ctx.knn(m, 8)
    finally:
        ctx.set_option("knn_chunk", 0)
    assert_same_lists(got, ref)


def test_a_smaller_k_is_a_prefix(ctx, want):
    m, ref = want["K700"]
    for k in (1, 3):
        assert_same_lists(ctx.knn(m, k), ref[:, :k])


def test_bad_arguments_are_refused_before_anything_is_launched(ffi, want):
    m, _ = want["E65"]
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS | ffi.FLAG_KERNEL_TIMING) as c:
        for data, k, word in ((m, 0, "k = 0"), (m, 9, "k = 9"), (m[:2], 3, "k = 3"), (np.zeros((10, 33)), 3, "33 columns"), (np.zeros((10, 0)), 3, "0 columns")):
            with pytest.raises(ffi.PjbError) as e:
                c.knn(data, k)
            assert e.value.code == -16 and word in str(e.value), str(e.value)
        for bad in (np.nan, np.inf, -np.inf, 1e200):
            x = m.copy()
            x[17, 5] = bad
            with pytest.raises(ffi.PjbError) as e:
                c.knn(x, 3)
            assert e.value.code == -16 and "row 17, column 5" in str(e.value), str(e.value)
        assert not [k for k in c.kernel_timing() if k.startswith("kn_")], "a kernel was launched for refused arguments"
        assert_same_lists(c.knn(m, 3), want["E65"][1])  # the context still works
        assert {k for k in c.kernel_timing() if k.startswith("kn_")} == {"kn_partial", "kn_merge"}
