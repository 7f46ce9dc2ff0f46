"""filt's forest stage on the device (pjb_forest_load / pjb_forest_predict / pjb_filt_scores, kernel kr_forest) against ranger's recorded
predictions (tests/golden/filt_forest, made by tests/golden/make_forest_fixture.py with the reference's library) and against the Python
restatement of Tree::predict in forest_util.py.  Every comparison is bit for bit: the per-class sums are sequential f64 sums in tree order."""
import numpy as np
import pytest

import forest_util as fu

pytestmark = pytest.mark.gpu

BLOCK = 256                      # rows per block of kr_forest (FOREST_BLOCK)
ROW_COUNTS = (1, 63, 64, 65, BLOCK + 1)


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (len(bad), bad[:3], got[tuple(bad[0])], want[tuple(bad[0])])


def test_witness_predictions_bit_for_bit(ffi):
    forest, X, P = fu.witness()
    assert X.shape == (200, 29) and P.shape == (200, 2)
    with ffi.Context(0) as ctx:
        ctx.forest_load(forest)
        assert_bit_equal(ctx.forest_predict(X), P)


GRID = np.arange(-1.0, 11.25, 0.25)


def _forest(ffi, kind, n_classes, n_vars=9, dep=2):
    rng = np.random.RandomState({"leaf": 1, "depth1": 2, "seven": 3, "spine": 4}[kind] * 10 + n_classes)
    if kind == "leaf":
        trees = [fu.random_tree(rng, n_vars, n_classes, dep, 0)]
    elif kind == "depth1":
        trees = [fu.random_tree(rng, n_vars, n_classes, dep, 1, values=GRID)]
    elif kind == "seven":
        trees = [fu.random_tree(rng, n_vars, n_classes, dep, 8, values=GRID, force_var=n_vars - 1 if t == 3 else None) for t in range(7)]
    else:
        trees = [fu.left_spine(rng, n_vars, n_classes, dep, 40), fu.random_tree(rng, n_vars, n_classes, dep, 5, values=GRID)]
    f = ffi.Forest(n_vars, n_classes, trees, dependent_var=dep)
    assert f.check() is None
    return f, rng


@pytest.mark.parametrize("n_classes", [2, 3])
@pytest.mark.parametrize("kind", ["leaf", "depth1", "seven", "spine"])
def test_shapes_against_the_python_walk(ffi, kind, n_classes):
    forest, rng = _forest(ffi, kind, n_classes)
    n = max(ROW_COUNTS)
    X = GRID[rng.randint(0, len(GRID), (n, forest.n_vars))]          # the grid the split values come from: values equal to split values
    X[::5] = -1.0                                                    # rows that go all the way down a left spine
    X[rng.rand(*X.shape) < 0.03] = np.nan                            # a NaN goes right
    X[:, forest.dependent_var] = 1e300                               # poison: never read
    want = fu.walk_predict(forest, X)
    if kind in ("seven", "spine"):
        assert len(np.unique(bits(want[:, 0]))) > 5
        splits = forest.split_value[forest.left >= 0]
        assert np.isin(X[~np.isnan(X)], splits).any() and np.isnan(X).any()
    with ffi.Context(0) as ctx:
        ctx.forest_load(forest)
        for rows in ROW_COUNTS:
            assert_bit_equal(ctx.forest_predict(X[:rows]), want[:rows])
        Y = X.copy()
        Y[:, forest.dependent_var] = np.nan
        assert_bit_equal(ctx.forest_predict(Y), want)


def test_state(ffi):
    forest, X, P = fu.witness()
    other, rng = _forest(ffi, "seven", 3, n_vars=29, dep=0)
    with ffi.Context(0) as ctx:
        with pytest.raises(ffi.PjbError) as e:
            ctx.forest_predict(X)
        assert e.value.code == -19                                    # PJB_ERR_STATE
        with pytest.raises(ffi.PjbError) as e:
            ctx.filt_scores(np.zeros(1, dtype=ffi.ROW_DTYPE), 30.0, 0, {}, fu.ACTIVE_FEATURES)
        assert e.value.code == -19
        ctx.forest_load(forest)
        assert_bit_equal(ctx.forest_predict(X), P)
        ctx.forest_load(other)                                        # replaces the first
        assert_bit_equal(ctx.forest_predict(X), fu.walk_predict(other, X))
        # a forest that fails the check never reaches the device: refused, and the loaded one still answers
        bad = ffi.Forest(29, 3, [dict(left=[1, -1, -1], right=[0, -1, -1], split_var=[1, 0, 0], split_value=[0.0, 0.0, 0.0], counts=[[], [1, 2, 3], [3, 2, 1]])])
        with pytest.raises(ffi.PjbError) as e:
            ctx.forest_load(bad)
        assert e.value.code == -16 and "tree 0, node 0" in str(e.value)
        assert_bit_equal(ctx.forest_predict(X), fu.walk_predict(other, X))
        with pytest.raises(ffi.PjbError) as e:
            ctx.forest_predict(X[:, :28])
        assert e.value.code == -16


def _feature_forest(ffi, F, n_classes, seed):
    """29 variables (the active columns); split values taken from the feature rows themselves, so that some walks meet value == split"""
    rng = np.random.RandomState(seed)
    vals = F[:, fu.ACTIVE_FEATURES[1:]].ravel()
    vals = vals[np.isfinite(vals)]
    trees = [fu.random_tree(rng, 29, n_classes, 0, 7, values=vals, force_var=28 if t == 0 else None) for t in range(7)]
    f = ffi.Forest(29, n_classes, trees, dependent_var=0)
    assert f.check() is None
    return f


def _check_fused(ffi, ctx, drows, mrl, l95, models, n_classes, seed):
    F = ctx.filt_features(drows, mrl, l95, models)
    forest = _feature_forest(ffi, F, n_classes, seed)
    ctx.forest_load(forest)
    want = ctx.forest_predict(F[:, fu.ACTIVE_FEATURES])
    assert_bit_equal(want, fu.walk_predict(forest, F[:, fu.ACTIVE_FEATURES]))
    pred, F2 = ctx.filt_scores(drows, mrl, l95, models, fu.ACTIVE_FEATURES, want_features=True)
    assert_bit_equal(F2, F)
    assert_bit_equal(pred, want)
    assert_bit_equal(ctx.filt_scores(drows, mrl, l95, models, fu.ACTIVE_FEATURES), want)
    return want


def test_fused_path_at_contig_edges(ffi, orc):
    """the junctions of test_feature_windows_at_contig_edges: windows clamped at either end of a short contig; 4 rows, a partial wavefront"""
    from portcullis_amd.records import ReadBatch
    g = ("ACGTTGCAAGGCTTAACCGGTTAACG" * 8)[:200]
    reads = [dict(pos=0, cigar="4M20N30M", seq="A" * 34, xs="+"), dict(pos=2, cigar="3M19N30M", seq="C" * 33, xs="-"),
             dict(pos=150, cigar="20M25N5M", seq="G" * 25, xs="-"), dict(pos=151, cigar="20M20N9M", seq="T" * 29, xs="+")]
    b = ReadBatch.from_reads(reads)
    rows, reg = orc.find_juncs(0, len(g), g, b, "UNKNOWN")
    orows = orc.finalize(rows, 30.0)
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(g)])
        ctx.upload_contig(0, g.encode())
        ctx.clear_rows()
        ctx.submit_batch(0, b)
        ctx.finish_contig(0)
        ctx.upload_contig(0, g.encode())
        drows = ctx.collect()
        assert 0 < len(drows) < 64
        idx = np.arange(len(orows))
        _, models, l95 = orc.filt_features([len(g)], {0: g}, orows, idx, idx, idx[:2], idx[2:])
        _check_fused(ffi, ctx, drows, 30.0, 0, {}, 2, 5)             # what this filt passes: untrained models, L95 = 0
        _check_fused(ffi, ctx, drows, 30.0, l95, models, 3, 6)       # the ABI is general: trained models, l95 != 0


def test_fused_path_on_fuzz_contigs(ffi, orc):
    """three targets, more rows than a wavefront and no multiple of one; untrained models with L95 = 0 (what filt passes) and trained ones"""
    from fuzzgen import make_reads, to_batch
    seeds = (61, 62, 63)
    made = [make_reads(seed, n_reads=2500, glen=24000) for seed in seeds]
    contigs = [g.upper() for g, _ in made]
    lens = [len(g) for g in contigs]
    rows_all, tot_len, tot_n = [], 0, 0
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs(lens)
        ctx.clear_rows()
        for tid, (_, reads) in enumerate(made):
            b = to_batch(reads)
            rows, reg = orc.find_juncs(tid, lens[tid], contigs[tid], b, "UNKNOWN")
            rows_all.append(rows)
            tot_len += reg["sum_len"]
            tot_n += reg["spliced"] + reg["unspliced"]
            ctx.upload_contig(tid, contigs[tid].encode())
            ctx.submit_batch(tid, b)
            ctx.finish_contig(tid)
            ctx.upload_contig(tid, contigs[tid].encode())      # (finish does not release it; kept for the feature windows)
        orows = orc.finalize(np.concatenate(rows_all), tot_len / tot_n)
        drows = ctx.collect().copy()
        assert len(drows) == len(orows)
        if len(drows) % 64 == 0:
            drows, orows = drows[:-1], orows[:-1]
        n = len(drows)
        assert n > 64 and n % 64 != 0
        idx = np.arange(n)
        good, bad = idx[orows["nb_raw"] >= 3], idx[orows["nb_raw"] < 3]
        sizes = orows["end"] - orows["start"] + 1
        _, models, l95 = orc.filt_features(lens, dict(enumerate(contigs)), orows, idx[sizes <= np.median(sizes)], good, good, bad)
        mrl = float(orows["mean_readlen"][0])
        assert l95 > 0 and models["exon_size"] > 0
        a = _check_fused(ffi, ctx, drows, mrl, 0, {}, 2, 7)
        b2 = _check_fused(ffi, ctx, drows, mrl, l95, models, 2, 7)
        assert len(np.unique(bits(a[:, 0]))) > 5 and len(np.unique(bits(b2[:, 0]))) > 5
