"""The growing of a ranger 0.3.8 probability forest in plain Python: the yardstick of the device's grower (pjb_forest_grow).

`grow(matrix, n_trees, seed, ...)` restates, node by node, what Forest::grow does for ForestProbability as
ModelFeatures::trainInstance sets it up (no replacement, sample fraction 1, every variable ordered, Gini importance):

  Tree::grow                       nodes are split in the order of their numbers, children get the next two numbers, left first
  Tree::splitNode                  the candidates are drawn first, whatever becomes of the node; rows with value <= split go left
  createPossibleSplitVarSubset     mtry distinct columns other than the label, by drawWithoutReplacementSimple on the tree's
                                   std::mt19937_64, seeded (uint)((tree + 1) * seed); the bootstrap takes the generator by value
                                   and so draws nothing from it
  splitNodeInternal                terminal when the node has at most min_node_size rows or one label only, or when no candidate
                                   has two values in it
  findBestSplitValue{SmallQ,LargeQ}  per candidate, in draw order, every value but the largest, ascending: with the label sum sl of
                                   the nl rows <= value and sr, nr of the others, the score sl * sl / nl + sr * sr / nr in doubles;
                                   a score wins only if it is strictly above everything before it
  addToTerminalNodes               per class the count of the node's rows, divided once by the node's size

Label sums and counts are integers here; ranger sums doubles that are 0 or 1, which is the same below 2^53.  The saved split value
is the column's value in the last row of the left child, rows of equal value in row order: ranger saves an entry of a sorted table
of the distinct values, which is the same number, and the same bytes unless the column holds both zeros.

The generator and the draw are imported from tests/golden/make_forest_grow_fixture.py, which pins them against ranger's roots.
tests/test_grow_model.py pins this file to every committed forest and to the recorded hashes of the others, without a GPU.

Beside the forest, `grow` returns per tree the facts the coverage conditions of the tests are stated in: see `grow`.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_forest_grow_fixture import Mt19937_64, draw_candidates  # noqa: E402  (numpy only; touches nothing on import)

DEFAULT_MIN_NODE_SIZE = 10


def best_split(values, labels):
    """(score, rows going left, their label sum, split value) of the first best value of one candidate in one node, or None if the
    candidate has one value only there"""
    order = np.argsort(values, kind="stable")
    v = values[order]
    at = np.flatnonzero(v[1:] != v[:-1])  # the last row of every value but the largest
    if at.size == 0:
        return None
    total = len(v)
    below = np.cumsum(labels[order])
    sl = below[at].astype(np.float64)
    sr = float(below[-1]) - sl
    nl = (at + 1).astype(np.float64)
    nr = float(total) - nl
    score = sl * sl / nl + sr * sr / nr
    k = int(np.argmax(score))  # the first of the largest
    return float(score[k]), int(at[k]) + 1, int(below[at[k]]), float(v[at[k]])


def grow_tree(m, y, gen, mtry, min_node, dep):
    """One tree: the dict ffi.Forest takes, and its facts."""
    n, n_cols = m.shape
    rows = [np.arange(n)]
    start, depth = [0], [0]
    left, right, var, val, counts = [], [], [], [], []
    splits, no_split = [], []
    k = 0
    while k < len(rows):
        r = rows[k]
        cand = draw_candidates(gen, n_cols, dep, mtry)
        lab = y[r]
        ones = int(lab.sum())
        best = None
        if len(r) > min_node and 0 < ones < len(r):
            found = []
            for c in cand:
                b = best_split(m[r, c], lab)
                if b is not None:
                    found.append(b[0])
                    if best is None or b[0] > best[0][0]:
                        best = (b, c)
            if best is None:
                no_split.append(k)
        if best is None:
            left.append(-1), right.append(-1), var.append(0), val.append(0.0)
            counts.append((len(r) - ones, ones))
        else:
            (score, n_left, _, value), c = best
            goes_left = m[r, c] <= value
            assert int(goes_left.sum()) == n_left
            left.append(len(rows)), right.append(len(rows) + 1), var.append(c), val.append(value)
            counts.append(None)
            rows.append(r[goes_left]), rows.append(r[~goes_left])
            start.extend((start[k], start[k] + n_left))
            depth.extend((depth[k] + 1, depth[k] + 1))
            splits.append(dict(node=k, left_last=start[k] + n_left - 1, tied=sum(s == score for s in found) > 1))
        k += 1
    assert depth == sorted(depth), "a level is a run of node numbers"
    facts = dict(levels=np.bincount(depth).tolist(), start=start, count=[len(r) for r in rows], splits=splits, no_split=no_split)
    return dict(left=left, right=right, split_var=var, split_value=val, counts=counts), facts


TRIP = 64  # positions of a list, and nodes of a level, that one wave of the device's kernels takes at a time


def conditions(facts, n_rows):
    """What the trees of one forest reach, from their facts: the names the tests ask for, each True or False.
      wide64, wide128   a level of more than 64 / 128 nodes: kt_decide numbers its children in two / three trips
      start64           a node that starts at a trip border inside the list
      end64             a node that ends at a trip border inside the list
      span3             a node other than a root that lies in three trips or more
      left63            a split whose left child ends in the last lane of a trip: the next value is read from the next trip
      uneven            trees of different depth: at some level one tree has finished and another has not
      no_split          a node above the node size, of both labels, terminal because every candidate had one value only
      tied              a split at which two candidates reached the best score and the one drawn first won"""
    nodes = [(s, c, k) for f in facts for k, (s, c) in enumerate(zip(f["start"], f["count"]))]
    return dict(
        wide64=any(w > TRIP for f in facts for w in f["levels"]),
        wide128=any(w > 2 * TRIP for f in facts for w in f["levels"]),
        start64=any(s and s % TRIP == 0 for s, _, _ in nodes),
        end64=any((s + c) % TRIP == 0 and s + c < n_rows for s, c, _ in nodes),
        span3=any(k and (s + c - 1) // TRIP - s // TRIP >= 2 for s, c, k in nodes),
        left63=any(s["left_last"] % TRIP == TRIP - 1 for f in facts for s in f["splits"]),
        uneven=len({len(f["levels"]) for f in facts}) > 1,
        no_split=any(f["no_split"] for f in facts),
        tied=any(s["tied"] for f in facts for s in f["splits"]),
    )


SWEEP_ROWS = (1, 2, 11, 63, 64, 65, 127, 128, 129)
SWEEP_COLS = (4, 6, 29, 33)


def sweep_shapes():
    """The 27 shapes of the seeded sweep: every row count three times, with the column counts, the label's place (first, middle,
    last), the node sizes (1, 3, ranger's default) and the kind of values (small integers, reals) going round at their own pace."""
    out = []
    for i, rows in enumerate(SWEEP_ROWS * 3):
        cols = SWEEP_COLS[i % 4]
        dep = (0, cols // 2, cols - 1)[(i + i // 9) % 3]
        out.append(dict(rows=rows, cols=cols, dep=dep, min_node=(1, 3, 0)[(i // 2) % 3], ints=bool((i + i // 4) % 2), trees=(2, 5, 7)[i % 3], rng=5000 + i))
    return out


def sweep_id(s):
    return f"{s['rows']}x{s['cols']}-label{s['dep']}-node{s['min_node']}-{'ints' if s['ints'] else 'reals'}-{s['trees']}trees-rng{s['rng']}"


def sweep_matrix(s):
    rng = np.random.RandomState(s["rng"])
    m = rng.randint(0, 4, (s["rows"], s["cols"])).astype(np.float64) if s["ints"] else rng.normal(size=(s["rows"], s["cols"])).round(2) + 0.0
    m[:, s["dep"]] = rng.randint(0, 2, s["rows"])
    return m


def clear_zero_signs(forest):
    """The forest with +0.0 for every split value -0.0 (a copy of the one array): what ranger and the device agree on when a column
    holds both zeros"""
    import copy
    out = copy.copy(forest)
    out.split_value = forest.split_value + 0.0
    return out


def grow(matrix, n_trees, seed, mtry=0, min_node_size=0, dependent_col=0):
    """(ffi.Forest, facts): the forest ranger grows from `matrix` (float64 [rows, columns], labels 0 / 1 in `dependent_col`), and per
    tree a dict of
      levels    the number of nodes of every level, the root's first
      start, count   per node its positions [start, start + count) in the tree's per-column lists of rows (children share the
                parent's positions, the left child first)
      splits    per split node, in node order: node, left_last (the last position of its left child), tied (another candidate
                reached the winning score)
      no_split  the nodes above the node size, of both labels, in which every candidate had one value only"""
    from portcullis_amd import ffi
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    n, n_cols = m.shape
    mtry = mtry or max(1, int(math.sqrt(n_cols - 1)))
    min_node = min_node_size or DEFAULT_MIN_NODE_SIZE
    assert mtry < n_cols // 2, "from n_cols / 2 on ranger draws by another algorithm"
    y = (m[:, dependent_col] == 1.0).astype(np.int64)
    assert ((m[:, dependent_col] == 0.0) | (y == 1)).all()
    classes = [v for v in (0.0, 1.0) if (m[:, dependent_col] == v).any()]
    trees, facts = [], []
    for t in range(n_trees):
        tree, f = grow_tree(m, y, Mt19937_64(((t + 1) * seed) & 0xFFFFFFFF), mtry, min_node, dependent_col)
        for k, c in enumerate(tree["counts"]):
            if c is None:
                tree["counts"][k] = []
            else:
                size = float(c[0] + c[1])
                tree["counts"][k] = [float(c[0]) / size, float(c[1]) / size] if len(classes) == 2 else [size / size]
        trees.append(tree)
        facts.append(f)
    forest = ffi.Forest(n_cols, len(classes), trees, dependent_col, np.ones(n_cols, dtype=np.uint8))
    forest.class_values = classes
    return forest, facts
