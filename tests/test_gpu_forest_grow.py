"""A forest grown on the device (pjb_forest_grow, kernels kt_* of pjb_grow.hip.h) against the files ranger 0.3.8 saved for the same
matrices (tests/golden/forest_grow and filt_forest/witness.forest, made by tests/golden/make_forest_grow_fixture.py with the reference's
library).  The matrices are made again from the seeds in cases.json.  Every comparison is bit for bit.

Seventeen more cases (W1 .. S2 of cases.json) and a seeded sweep are compared with tests/grow_model.py, the plain restatement of
ranger's growing that tests/test_grow_model.py pins to ranger without a device -- the model supplies every byte and the place of the
first difference -- and the cases with SHA-256 and length of the bytes ranger itself saved."""
import hashlib
import os
import sys

import numpy as np
import pytest

import forest_util as fu
import grow_model as gm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_forest_grow_fixture as fx  # noqa: E402  (the generator of the matrices; it touches nothing on import)

pytestmark = pytest.mark.gpu

ALL = {c["name"]: c for c in fx.load_cases()}
CASES = {n: c for n, c in ALL.items() if "sha256" not in c}  # G1 .. G5: ranger's files
MORE = {n: c for n, c in ALL.items() if "sha256" in c}       # W1 .. S2: the model's bytes and ranger's hash
ARRAYS = ("tree_off", "left", "right", "split_var", "count_off")


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
def want(ffi):
    """name -> (matrix, ranger's forest, ranger's bytes); made once, never changed"""
    out = {}
    for name, case in CASES.items():
        m = fx.case_matrix(case)
        m.setflags(write=False)
        out[name] = (m, ffi.Forest.from_file(fx.forest_path(case)), open(fx.forest_path(case), "rb").read())
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def first_difference(got, ref):
    """(tree, node, what) of the first node that differs, for the message"""
    for t in range(min(got.n_trees, ref.n_trees)):
        a, b = int(ref.tree_off[t]), int(ref.tree_off[t + 1])
        c = int(got.tree_off[t])
        for k in range(b - a):
            if c + k >= len(got.left):
                return t, k, "missing"
            for name in ("left", "right", "split_var"):
                if getattr(got, name)[c + k] != getattr(ref, name)[a + k]:
                    return t, k, name
            if bits(got.split_value[c + k:c + k + 1])[0] != bits(ref.split_value[a + k:a + k + 1])[0]:
                return t, k, "split_value"
    return None


def assert_same_forest(got, ref, raw=None):
    assert (got.n_trees, got.n_classes, got.n_vars, got.dependent_var) == (ref.n_trees, ref.n_classes, ref.n_vars, ref.dependent_var)
    assert list(got.class_values) == list(ref.class_values)
    assert first_difference(got, ref) is None, first_difference(got, ref)
    for name in ARRAYS:
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert np.array_equal(bits(got.split_value), bits(ref.split_value))
    assert np.array_equal(bits(got.counts), bits(ref.counts))
    assert got.check() is None
    if raw is not None:
        assert got.to_bytes() == raw


@pytest.fixture(scope="module")
def model():
    """name -> (matrix, the model's forest, its bytes) of the cases W1 .. S2; made once, never changed"""
    out = {}
    for name, case in MORE.items():
        cols, dep, mtry, min_node, seed = fx.case_args(case)
        m = fx.case_matrix(case)
        m.setflags(write=False)
        forest = gm.grow(m, case["trees"], seed, mtry, min_node, dep)[0]
        out[name] = (m, forest, forest.to_bytes())
    return out


def grow_case(ffi, ctx, case, m):
    cols, dep, mtry, min_node, seed = fx.case_args(case)
    return ffi.Forest.grow(ctx, m, n_trees=case["trees"], seed=seed, mtry=mtry, min_node_size=min_node, dependent_col=dep)


def test_cases_cover_the_issue():
    assert set(CASES) == {"G1", "G2", "G3", "G4a", "G4b", "G5"}
    assert CASES["G1"]["file"].endswith("filt_forest/witness.forest") and CASES["G5"]["rows"] > 20 * fx.TRIP
    # (what each of these reaches is asserted from the model's facts, without a device: tests/test_grow_model.py)
    assert set(MORE) == {"W1", "W2", "T250", "T17", "D1", "D2", "C4", "C33", "C65", "C130", "M1", "Mmax", "N1", "N3", "Z0", "ZS", "S2"}
    assert (MORE["W1"]["rows"], MORE["W2"]["rows"], MORE["T250"]["trees"], MORE["T17"]["trees"]) == (4000, 2500, 250, 17)
    assert all(len(c["sha256"]) == 64 and c["bytes"] > 0 for c in MORE.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_grown_forest_is_rangers_file(ffi, ctx, want, name):
    m, ref, raw = want[name]
    got = ffi.Forest.grow(ctx, m, n_trees=CASES[name]["trees"])
    assert_same_forest(got, ref, raw)
    if name == "G3":
        assert got.n_classes == 1 and got.class_values == [1.0] and list(np.diff(got.tree_off)) == [1] * 4 and list(got.counts) == [1.0] * 4


@pytest.mark.parametrize("name", sorted(MORE))
def test_grown_forest_is_the_models_and_has_rangers_hash(ffi, ctx, model, name):
    """levels of two and three waves of nodes, 250 and 17 trees, the label in other columns, 4 to 130 columns, both ends of mtry,
    node sizes 1 and 3, the class 0 alone, a column with both zeros, another seed"""
    m, ref, raw = model[name]
    got = grow_case(ffi, ctx, MORE[name], m)
    assert_same_forest(got, ref, raw)
    if name != "ZS":
        assert (len(raw), hashlib.sha256(got.to_bytes()).hexdigest()) == (MORE[name]["bytes"], MORE[name]["sha256"])
    if name == "Z0":
        assert got.n_classes == 1 and got.class_values == [0.0] and list(np.diff(got.tree_off)) == [1] * 4 and list(got.counts) == [1.0] * 4


def test_signed_zeros(ffi, model):
    """ZS: where a column holds -0.0 and +0.0, ranger saves the zero its std::sort left first, the device the zero of the last row
    of the left child.  Equal but for that sign, and the same predictions bit for bit."""
    m, _, raw = model["ZS"]
    ranger = ffi.Forest.from_file(fx.forest_path(MORE["ZS"]))
    with ffi.Context(0) as c:
        got = grow_case(ffi, c, MORE["ZS"], m)
        assert got.to_bytes() == raw
        assert_same_forest(gm.clear_zero_signs(got), gm.clear_zero_signs(ranger), gm.clear_zero_signs(ranger).to_bytes())
        c.forest_load(got)
        mine = c.forest_predict(m)
        c.forest_load(ranger)
        assert np.array_equal(bits(mine), bits(c.forest_predict(m)))
    assert len(np.unique(bits(mine))) > 2


def test_250_trees_in_batches_of_48(ffi, model):
    """five full batches and one of 10 trees: a tree depends on its number only"""
    m, ref, raw = model["T250"]
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as c:
        c.set_option("grow_batch", 48)
        got = grow_case(ffi, c, MORE["T250"], m)
    assert_same_forest(got, ref, raw)
    assert hashlib.sha256(got.to_bytes()).hexdigest() == MORE["T250"]["sha256"]


@pytest.mark.parametrize("shape", gm.sweep_shapes(), ids=gm.sweep_id)
def test_sweep_against_the_model(ffi, ctx, shape):
    m = gm.sweep_matrix(shape)
    ref = gm.grow(m, shape["trees"], fx.SEED, 0, shape["min_node"], shape["dep"])[0]
    got = ffi.Forest.grow(ctx, m, n_trees=shape["trees"], min_node_size=shape["min_node"], dependent_col=shape["dep"])
    assert_same_forest(got, ref, ref.to_bytes())


def test_g1_end_to_end(ffi, want):
    """grow, load, predict: ranger's recorded predictions of the committed test matrix"""
    _, X, P = fu.witness()
    with ffi.Context(0) as c:
        c.forest_load(ffi.Forest.grow(c, want["G1"][0], n_trees=8))
        got = c.forest_predict(X)
    assert np.array_equal(bits(got), bits(P))


def test_state_between_calls(ffi, want):
    forest, X, P = fu.witness()
    with ffi.Context(0) as c:
        for name in ("G2", "G1", "G2"):
            assert ffi.Forest.grow(c, want[name][0], n_trees=CASES[name]["trees"]).to_bytes() == want[name][2], name
        c.forest_load(forest)
        assert np.array_equal(bits(c.forest_predict(X)), bits(P))
        assert ffi.Forest.grow(c, want["G4b"][0], n_trees=4).to_bytes() == want["G4b"][2]
        assert np.array_equal(bits(c.forest_predict(X)), bits(P))  # (still the loaded forest: a grown one is not loaded by growing it)


@pytest.mark.parametrize("batch", [0, 3])
def test_tree_counts_and_batches(ffi, want, batch):
    """1 and 9 trees: a tree depends on its number only; `grow_batch` 3: three batches of three trees"""
    m, ref, _ = want["G1"]
    with ffi.Context(0) as c:
        c.set_option("grow_batch", batch)
        nine, one = ffi.Forest.grow(c, m, n_trees=9), ffi.Forest.grow(c, m, n_trees=1)
    assert nine.n_trees == 9 and one.n_trees == 1 and nine.check() is None
    n8, c8 = int(ref.tree_off[8]), len(ref.counts)
    for name in ARRAYS[:-1]:
        assert np.array_equal(getattr(nine, name)[:9 if name == "tree_off" else n8], getattr(ref, name)), name
    assert np.array_equal(nine.count_off[:n8], ref.count_off)
    assert np.array_equal(bits(nine.split_value[:n8]), bits(ref.split_value)) and np.array_equal(bits(nine.counts[:c8]), bits(ref.counts))
    n1 = int(ref.tree_off[1])
    assert np.array_equal(one.left, ref.left[:n1]) and np.array_equal(bits(one.split_value), bits(ref.split_value[:n1]))


def test_errors_are_found_before_any_launch(ffi, want):
    m = np.array(want["G1"][0])
    bad = []
    nan, inf, lab = m.copy(), m.copy(), m.copy()
    nan[7, 3], inf[299, 28], lab[5, 0] = np.nan, -np.inf, 2.0
    bad.append((dict(data=nan, n_trees=2), "row 7, column 3 is not finite"))
    bad.append((dict(data=inf, n_trees=2), "row 299, column 28 is not finite"))
    bad.append((dict(data=lab, n_trees=2), "row 5 has the label 2 (0 or 1)"))
    bad.append((dict(data=m, n_trees=0), "0 trees (at least one is needed)"))
    bad.append((dict(data=m[:0], n_trees=2), "0 rows (at least one is needed)"))
    bad.append((dict(data=m[:, :1], n_trees=2), "1 columns (the labels and one variable at least)"))
    bad.append((dict(data=m, n_trees=2, mtry=14), "mtry 14 of 29 columns: from n_cols / 2 on ranger draws by Knuth's algorithm, which is not built"))
    bad.append((dict(data=m[:, :3], n_trees=2), "mtry 1 of 3 columns"))
    bad.append((dict(data=np.zeros((4, 2049)), n_trees=2), "2049 variables (1 to 2048 can be walked)"))
    bad.append((dict(data=m, n_trees=2, dependent_col=29), "dependent column 29 of 29 columns"))
    with ffi.Context(0, flags=ffi.FLAG_KERNEL_TIMING) as c:
        for kw, msg in bad:
            with pytest.raises(ffi.PjbError) as e:
                ffi.Forest.grow(c, **kw)
            assert e.value.code == -16 and "pjb_forest_grow: " in str(e.value) and msg in str(e.value), (msg, str(e.value))
        assert not [k for k in c.kernel_timing() if k.startswith("kt_")]
        got = ffi.Forest.grow(c, m, n_trees=8, mtry=13)  # (the largest mtry the simple draw serves) -- and the context still works
        assert got.check() is None and got.n_trees == 8
        assert ffi.Forest.grow(c, m, n_trees=8).to_bytes() == want["G1"][2]
        assert c.kernel_timing()["kt_split"][0] > 0
