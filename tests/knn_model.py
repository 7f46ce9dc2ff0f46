"""K nearest neighbours in plain numpy: the yardstick of the device's search (pjb_knn) beyond the lists the reference wrote.

KNN::doSlice (lib/src/knn.cc of the reference) restated per test row t: over all base rows at once,
    s = 0;  s = s + (base[:, c] - t[c]) * (base[:, c] - t[c])   for the columns c in ascending order, every step rounded to a double,
and the answer is the k smallest base rows under (s, index), the row itself among them -- `np.lexsort`, no partial lists, no
chunks, no padding.  tests/test_knn_model.py pins this file to every committed list of the reference without a GPU.
"""
import numpy as np


def distances(m, row):
    """float64 [rows]: the squared distance of every row of m to row `row`, summed as the reference sums it"""
    m = np.asarray(m, dtype=np.float64)
    s = np.zeros(len(m))
    for c in range(m.shape[1]):
        d = m[:, c] - m[row, c]
        s = s + d * d
    return s


def knn(m, k):
    """uint32 [rows, k]: per row the k nearest rows under (squared distance, index)"""
    m = np.asarray(m, dtype=np.float64)
    n = len(m)
    assert 1 <= k <= n
    index = np.arange(n)
    out = np.empty((n, k), dtype=np.uint32)
    for r in range(n):
        out[r] = np.lexsort((index, distances(m, r)))[:k]
    return out


def rows_tied_across_chunks(m, k, chunk, more_than=8):
    """How many rows have, at the distance of the last entry of their list of k, more than `more_than` base rows lying in more than
    one chunk of `chunk` base rows: there the index alone decides, and it decides between the partial lists of different chunks."""
    m = np.asarray(m, dtype=np.float64)
    count = 0
    for r in range(len(m)):
        s = distances(m, r)
        tied = np.flatnonzero(s == np.sort(s)[k - 1])
        count += len(tied) > more_than and len(set((tied // chunk).tolist())) > 1
    return int(count)
