"""k-fold cross-validation on the device (pjb_forest_cv, kernels kc_* of pjb_cv.hip.h over the level loop of pjb_grow.hip.h), bit for bit:

  against tests/cv_model.py -- per fold grow_model.grow on the sub-matrix and forest_util.walk_predict on the held-out rows: plain
  Python that knows nothing of the library (MODEL_CASES);
  against forest_grow / forest_load / forest_predict of the same library on the sub-matrices, at sizes the model is too slow for
  (SWEEP_CASES): growing is pinned to ranger in test_gpu_forest_grow.py, the walk in test_gpu_forest.py.

What the cases reach -- n_f of 63, 64 and 65 beside the 64 positions of a trip, a tail of 64 rows and more, folds of unequal size, a
fold of one held-out row, fold ids interleaved and in blocks, folds whose trees differ in depth, the label first, in the middle and
last -- is computed from their inputs in test_cases_cover_the_issue.  Then: a batch that cuts through a fold, the launch count that shows
the folds share one level loop, every refusal before a launch, and the state a call leaves behind."""
import numpy as np
import pytest

import cv_model as cm
import forest_util as fu
import grow_model as gm
from test_gpu_forest_grow import assert_same_forest, bits

pytestmark = pytest.mark.gpu

SEED = 1236456789
TRIP = gm.TRIP


def case(name, rows, cols, folds, trees, min_node, dep, ints, how):
    return dict(name=name, rows=rows, cols=cols, folds=folds, trees=trees, min_node=min_node, dep=dep, ints=ints, how=how, rng=7000 + rows + cols + folds)


# rows x cols x folds of the issue, 3 trees, node sizes 1 and ranger's default
MODEL_CASES = [case(f"m{rows}x{cols}x{folds}-node{node}", rows, cols, folds, 3, node, dep, ints, how)
               for rows, cols, folds, dep, ints, how in ((11, 6, 2, 0, True, "shuffle"), (65, 6, 3, 3, False, "round"), (96, 29, 3, 28, False, "shuffle"))
               for node in (1, 0)]
# rows (64, 128, 129, 200) x folds (2, 3, 5), the columns, trees, label's place, node size and kind of values going round; then the
# explicit fold arrays: 65 | 63 rows held out of 128 (n_f = 63 and 65), one row held out of 129
SWEEP_CASES = [case(f"s{rows}x{cols}x{folds}-{how}", rows, cols, folds, (3, 7)[i % 2], (0, 1, 3)[i % 3], (0, cols // 2, cols - 1)[(i + i // 3) % 3], bool(i % 2), how)
               for i, (rows, folds) in enumerate((r, k) for r in (64, 128, 129, 200) for k in (2, 3, 5))
               for cols in ((6, 29)[(i + i // 2) % 2],) for how in (("shuffle", "round", "blocks")[i % 3],)]
SWEEP_CASES += [case("s128x6-sizes65+63", 128, 6, 2, 3, 1, 5, False, (65, 63)), case("s129x29-sizes1+64+64", 129, 29, 3, 3, 0, 0, True, (1, 64, 64)),
                case("s128x29x2-blocks", 128, 29, 2, 7, 1, 14, True, "blocks")]
ALL_CASES = MODEL_CASES + SWEEP_CASES


def matrix_of(c):
    m = gm.sweep_matrix(c)
    m.setflags(write=False)
    return m


def folds_of(c):
    n, k, how = c["rows"], c["folds"], c["how"]
    if how == "shuffle":
        return cm.assign_folds(n, k, SEED)
    if how == "round":
        return (np.arange(n) % k).astype(np.int32)
    if how == "blocks":
        return np.sort(np.arange(n) % k).astype(np.int32)
    assert sum(how) == n and len(how) == k
    return np.repeat(np.arange(k), how).astype(np.int32)


def kw_of(c):
    return dict(n_trees=c["trees"], min_node_size=c["min_node"], dependent_col=c["dep"])


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
def other(ffi):
    """the context the sub-matrices' own forests are grown, loaded and walked on"""
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def model():
    """name -> (pred, forests, facts) of the model cases; made once, never changed"""
    out = {}
    for c in MODEL_CASES:
        pred, forests, facts = cm.cv(matrix_of(c), folds_of(c), c["folds"], c["trees"], SEED, 0, c["min_node"], c["dep"])
        pred.setflags(write=False)
        out[c["name"]] = (pred, forests, facts)
    return out


def assert_same_cv(got, want):
    (pred, forests), (ref_pred, ref_forests) = got, want
    assert len(forests) == len(ref_forests)
    for f, (a, b) in enumerate(zip(forests, ref_forests)):
        assert_same_forest(a, b, b.to_bytes())
    diff = np.flatnonzero((bits(pred) != bits(ref_pred)).any(axis=1))
    assert diff.size == 0, (diff[:5], pred[diff[:5]], ref_pred[diff[:5]])


def by_library(other, m, fold, k, kw):
    """the same work the only way the library could do it before: per fold grow on the sub-matrix, load, predict the held-out rows"""
    pred, forests = np.zeros((len(m), 2)), []
    for f in range(k):
        forest = other.forest_grow(m[fold != f], **kw)
        other.forest_load(forest)
        pred[fold == f] = other.forest_predict(m[fold == f])
        forests.append(forest)
    return pred, forests


def test_cases_cover_the_issue(model):
    assert [(c["rows"], c["cols"], c["folds"]) for c in MODEL_CASES[::2]] == [(11, 6, 2), (65, 6, 3), (96, 29, 3)]
    assert all(c["trees"] == 3 for c in MODEL_CASES) and {c["min_node"] for c in MODEL_CASES} == {0, 1}
    sweep = SWEEP_CASES
    assert {c["rows"] for c in sweep} == {64, 128, 129, 200} and {c["cols"] for c in sweep} == {6, 29}
    assert {c["folds"] for c in sweep} == {2, 3, 5} and {c["trees"] for c in sweep} == {3, 7} and {c["ints"] for c in sweep} == {True, False}
    assert {(c["rows"], c["folds"]) for c in sweep} >= {(r, k) for r in (64, 128, 129, 200) for k in (2, 3, 5)}
    assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)
    n_f, tails, held_one, unequal, interleaved, blocks, place = set(), set(), False, False, False, False, set()
    for c in ALL_CASES:
        m, fold = matrix_of(c), folds_of(c)
        held = np.bincount(fold, minlength=c["folds"])
        assert len(fold) == c["rows"] and held.min() >= 1 and len(held) == c["folds"]
        for f in range(c["folds"]):  # every fold trains on both labels: none of these is refused
            assert 0 < m[fold != f, c["dep"]].sum() < c["rows"] - held[f], (c["name"], f)
        n_f |= {int(c["rows"] - h) for h in held}
        tails |= {int(h) for h in held}
        held_one |= 1 in held
        unequal |= len(set(held)) > 1
        changes = int((np.diff(fold) != 0).sum())
        blocks |= changes == c["folds"] - 1
        interleaved |= changes > c["rows"] // 2
        place.add("first" if c["dep"] == 0 else "last" if c["dep"] == c["cols"] - 1 else "middle")
    assert {TRIP - 1, TRIP, TRIP + 1} <= n_f, sorted(n_f)
    assert max(tails) >= TRIP and any(c["rows"] == 200 and c["folds"] == 2 for c in sweep)
    assert held_one and unequal and interleaved and blocks and place == {"first", "middle", "last"}
    # folds whose trees differ in depth (the level loop goes on for one fold's trees when another's have finished): from the model's facts
    depths = {name: [max(len(t["levels"]) for t in fold_facts) for fold_facts in facts] for name, (_, _, facts) in model.items()}
    assert any(len(set(d)) > 1 for d in depths.values()), depths
    assert any(len({len(t["levels"]) for t in fold_facts}) > 1 for _, _, facts in model.values() for fold_facts in facts)


@pytest.mark.parametrize("c", MODEL_CASES, ids=lambda c: c["name"])
def test_cv_is_the_models(ctx, model, c):
    ref_pred, ref_forests, _ = model[c["name"]]
    got = ctx.forest_cv(matrix_of(c), folds_of(c), c["folds"], **kw_of(c))
    assert_same_cv(got, (ref_pred, ref_forests))
    assert len(np.unique(bits(got[0]))) > 2


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: c["name"])
def test_cv_is_grow_load_predict_of_the_sub_matrices(ctx, other, c):
    m, fold = matrix_of(c), folds_of(c)
    assert_same_cv(ctx.forest_cv(m, fold, c["folds"], **kw_of(c)), by_library(other, m, fold, c["folds"], kw_of(c)))


def test_a_batch_that_cuts_through_a_fold(ffi):
    """3 folds x 5 trees in batches of 4: trees 0-3 | 4, 5-7 | 8-9, 10-11 | 12-14"""
    c = case("batches", 129, 29, 3, 5, 1, 0, False, "shuffle")
    m, fold = matrix_of(c), folds_of(c)
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as one:
        whole = one.forest_cv(m, fold, 3, **kw_of(c))
    for batch in (4, 1, 7):
        with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as cut:
            cut.set_option("grow_batch", batch)
            assert_same_cv(cut.forest_cv(m, fold, 3, **kw_of(c)), whole)


def test_the_folds_share_the_level_loop(ffi):
    """one batch: kt_split is launched once a level, and the call has as many levels as its deepest fold on its own -- not their sum"""
    c = case("loop", 200, 29, 5, 7, 1, 0, False, "shuffle")
    m, fold = matrix_of(c), folds_of(c)
    with ffi.Context(0, flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as t:
        t.forest_cv(m, fold, 5, **kw_of(c))
        kt = {k: v[0] for k, v in t.kernel_timing().items()}
        together = kt["kt_split"]
        assert kt["kc_seed"] == kt["kc_lists"] == kt["kc_park"] == kt["kc_score"] == 1 and not kt.get("kt_fill") and not kt.get("kr_forest")
        assert kt["kt_draw"] == kt["kt_decide"] == together and kt["kt_partition"] == kt["kt_assign"] == together - 1
        alone = []
        for f in range(5):
            t.reset_kernel_timing()
            t.forest_grow(m[fold != f], **kw_of(c))
            alone.append(t.kernel_timing()["kt_split"][0])
    assert together == max(alone) and max(alone) < sum(alone), (together, alone)


def test_errors_are_found_before_any_launch(ffi):
    c = case("errors", 65, 6, 3, 3, 1, 0, False, "round")
    m, fold = np.array(matrix_of(c)), folds_of(c)
    one_label = m.copy()
    one_label[:, 0] = (fold == 1)  # fold 1 holds every row of label 1 out
    inverse = one_label.copy()
    inverse[:, 0] = 1.0 - one_label[:, 0]
    outside, negative, empty = fold.copy(), fold.copy(), fold.copy()
    outside[9], negative[4] = 3, -1
    empty[empty == 2] = 0
    nan = m.copy()
    nan[7, 3] = np.nan
    bad = [
        (dict(data=m, fold=fold, n_folds=1), "1 folds of 65 rows (2 to the number of rows)"),
        (dict(data=m, fold=fold, n_folds=0), "0 folds of 65 rows"),
        (dict(data=m[:2], fold=[0, 1], n_folds=3), "3 folds of 2 rows"),
        (dict(data=m, fold=outside, n_folds=3), "row 9 is in fold 3 (0 to 2)"),
        (dict(data=m, fold=negative, n_folds=3), "row 4 is in fold -1 (0 to 2)"),
        (dict(data=m, fold=empty, n_folds=3), "fold 2 holds no row"),
        (dict(data=one_label, fold=fold, n_folds=3), "rows fold 1 trains on all have the label 0"),
        (dict(data=inverse, fold=fold, n_folds=3), "rows fold 1 trains on all have the label 1"),
        # everything pjb_forest_grow refuses
        (dict(data=nan, fold=fold, n_folds=3), "row 7, column 3 is not finite"),
        (dict(data=m, fold=fold, n_folds=3, n_trees=0), "0 trees (at least one is needed)"),
        (dict(data=m[:, :3], fold=fold, n_folds=3), "mtry 1 of 3 columns"),
        (dict(data=m, fold=fold, n_folds=3, dependent_col=6), "dependent column 6 of 6 columns"),
        (dict(data=m, fold=fold, n_folds=3, mtry=3), "mtry 3 of 6 columns"),
    ]
    with ffi.Context(0, flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as t:
        for kw, msg in bad:
            kw = dict(dict(n_trees=3), **kw)
            with pytest.raises(ffi.PjbError) as e:
                t.forest_cv(**kw)
            assert e.value.code == ffi.ERR_ARG and "pjb_forest_cv: " in str(e.value) and msg in str(e.value), (msg, str(e.value))
        assert not [k for k, v in t.kernel_timing().items() if v[0]], t.kernel_timing()
        pred, forests = t.forest_cv(m, fold, 3, n_trees=3, min_node_size=1)  # ... and the context still works
        assert len(forests) == 3 and t.kernel_timing()["kt_split"][0] > 0


def test_state_between_calls(ffi):
    forest, X, P = fu.witness()
    c = case("state", 129, 29, 3, 3, 0, 0, False, "shuffle")
    m, fold = matrix_of(c), folds_of(c)
    with ffi.Context(0) as fresh:
        want = fresh.forest_grow(m, n_trees=4).to_bytes()
    with ffi.Context(0) as t:
        t.forest_load(forest)
        assert np.array_equal(bits(t.forest_predict(X)), bits(P))
        first = t.forest_cv(m, fold, 3, **kw_of(c))
        assert np.array_equal(bits(t.forest_predict(X)), bits(P))  # (still the loaded forest)
        assert t.forest_grow(m, n_trees=4).to_bytes() == want
        assert_same_cv(t.forest_cv(m, fold, 3, **kw_of(c)), first)   # after a grow, and a second time: the same
        small = case("state2", 64, 6, 2, 3, 1, 0, True, "round")     # a smaller call in the pool the larger one left
        with ffi.Context(0) as fresh:
            ref = fresh.forest_cv(matrix_of(small), folds_of(small), 2, **kw_of(small))
        assert_same_cv(t.forest_cv(matrix_of(small), folds_of(small), 2, **kw_of(small)), ref)
        assert np.array_equal(bits(t.forest_predict(X)), bits(P))
