"""Shared by the filt forest tests: a restatement of ranger's Tree::predict / ForestProbability::predictInternal in Python (the sequential
f64 sum in tree order that the device must match bit for bit), random forests, and the witness fixture."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WITNESS_DIR = os.path.join(HERE, "golden", "filt_forest")
# the columns of the PJB_N_FEATURES row that the reference leaves active: the forest's variables, in order
ACTIVE_FEATURES = [0, 3, 5, 7, 8, 9, 10, 12, 13] + list(range(14, 34))


def walk_predict(forest, data):
    """float64 [n, n_classes]: from node 0, value <= split goes left, anything else (a NaN too) right; counts[c] / n_trees added tree after tree"""
    data = np.asarray(data, dtype=np.float64)
    out = np.zeros((len(data), forest.n_classes), dtype=np.float64)
    nt = np.float64(forest.n_trees)
    for t in range(forest.n_trees):
        base = int(forest.tree_off[t])
        left, right = forest.left[base:], forest.right[base:]
        var, val = forest.split_var[base:], forest.split_value[base:]
        for r in range(len(data)):
            k = 0
            while left[k] >= 0:
                k = left[k] if data[r, var[k]] <= val[k] else right[k]
            at = int(forest.count_off[base + k])
            for c in range(forest.n_classes):
                out[r, c] = out[r, c] + forest.counts[at + c] / nt
    return out


def random_tree(rng, n_vars, n_classes, dependent_var, max_depth, p_split=0.8, values=None, force_var=None):
    """one tree, numbered as ranger numbers it (children behind their parent, appended in pairs)"""
    left, right, var, val, counts, depth = [-1], [-1], [0], [0.0], [[]], [0]
    k = 0
    usable = [v for v in range(n_vars) if v != dependent_var]
    while k < len(left):
        if depth[k] < max_depth and (k == 0 or rng.rand() < p_split):
            left[k], right[k] = len(left), len(left) + 1
            var[k] = force_var if (force_var is not None and k == 0) else int(usable[rng.randint(len(usable))])
            val[k] = float(values[rng.randint(len(values))]) if values is not None else float(np.round(rng.normal(0, 1), 2))
            for _ in range(2):
                left.append(-1), right.append(-1), var.append(0), val.append(0.0), counts.append([]), depth.append(depth[k] + 1)
        else:
            counts[k] = [float(v) for v in rng.randint(0, 50, n_classes)]
        k += 1
    return dict(left=left, right=right, split_var=var, split_value=val, counts=counts)


def left_spine(rng, n_vars, n_classes, dependent_var, depth):
    """`depth` splits in a row down the left side: node 2d is internal with a terminal right child 2d + 1 and the next split 2d + 2 on its left"""
    usable = [v for v in range(n_vars) if v != dependent_var]
    leaf = lambda: [float(v) for v in rng.randint(0, 50, n_classes)]
    left, right, var, val, counts = [], [], [], [], []
    for d in range(depth):
        left += [2 * d + 2, -1]
        right += [2 * d + 1, -1]
        var += [int(usable[d % len(usable)]), 0]
        val += [float(10 - d * 0.25), 0.0]
        counts += [[], leaf()]
    left.append(-1), right.append(-1), var.append(0), val.append(0.0), counts.append(leaf())
    return dict(left=left, right=right, split_var=var, split_value=val, counts=counts)


def witness():
    from portcullis_amd import ffi
    forest = ffi.Forest.from_file(os.path.join(WITNESS_DIR, "witness.forest"))
    return forest, np.load(os.path.join(WITNESS_DIR, "test_matrix.npy")), np.load(os.path.join(WITNESS_DIR, "predictions.npy"))
