"""k-fold cross-validation as `train --folds` and pjb_forest_cv define it, in plain Python: the yardstick of both.

  assign_folds   row i starts in fold i % k; the vector is shuffled by Fisher-Yates from the back with std::mt19937_64 (the
                 Mt19937_64 of tests/grow_model.py) seeded with the forest's seed: for i = n-1 .. 1: swap v[i], v[next() % (i + 1)]
  Performance    the reference's confusion-matrix rates (lib/include/portcullis/ml/performance.hpp) and their two-decimal long
                 string; F1 and MCC are 0 where the reference's arithmetic leaves a NaN (or the root of -0.0)
  mean_lines     PerformanceList::outputMeanPerformance: ten lines "Mean <name padded to 13>: <mean>% (+/- <stdev>%)"
  cv_results     the text of <prefix>.cv_results from the held-out scores
  cv             per fold grow_model.grow on the sub-matrix of the other folds' rows + forest_util.walk_predict on the held-out rows
"""
import math

import numpy as np

import forest_util as fu
import grow_model as gm

LONG_HEADER = "TP\tTN\tFP\tFN\tPREV\tBIAS\tSENS\tSPEC\tPPV\tNPV\tF1\tACC\tINFO\tMARK\tMCC"
MEAN_NAMES = ("prevalence", "bias", "recall", "precision", "F1", "specificity", "accuracy", "informedness", "markededness", "MCC")


def assign_folds(n, k, seed):
    v = [i % k for i in range(n)]
    nxt = gm.Mt19937_64(seed & 0xFFFFFFFF)
    for i in range(n - 1, 0, -1):
        j = nxt() % (i + 1)
        v[i], v[j] = v[j], v[i]
    return np.array(v, dtype=np.int32)


def _pct(part, whole):
    return 0.0 if whole == 0 else 100.0 * float(part) / float(whole)


class Performance:
    def __init__(self, tp, tn, fp, fn):
        self.tp, self.tn, self.fp, self.fn = int(tp), int(tn), int(fp), int(fn)

    def n(self):
        return self.tp + self.tn + self.fp + self.fn

    def precision(self):
        return _pct(self.tp, self.tp + self.fp)

    def recall(self):
        return _pct(self.tp, self.tp + self.fn)

    def specificity(self):
        return _pct(self.tn, self.fp + self.tn)

    def npv(self):
        return _pct(self.tn, self.tn + self.fn)

    def prevalence(self):
        return _pct(self.tp + self.fn, self.n())

    def bias(self):
        return _pct(self.tp + self.fp, self.n())

    def accuracy(self):
        return _pct(self.tn + self.tp, self.n())

    def informedness(self):
        return self.recall() + self.specificity() - 100.0

    def markedness(self):
        return self.precision() + self.npv() - 100.0

    def f1(self):
        p, r = self.precision(), self.recall()
        below = (1.0 * p) + r
        return (1.0 + 1.0) * (p * r) / below if below > 0.0 else 0.0

    @staticmethod
    def mcc_of(informedness, markedness):
        x = informedness * markedness
        return math.sqrt(x) if x > 0.0 else 0.0

    def mcc(self):
        return self.mcc_of(self.informedness(), self.markedness())

    def values(self):
        """the eleven rates of the long string, in its order"""
        return [self.prevalence(), self.bias(), self.recall(), self.specificity(), self.precision(), self.npv(), self.f1(), self.accuracy(),
                self.informedness(), self.markedness(), self.mcc()]

    def mean_values(self):
        """the ten rates of the mean lines, in their order"""
        return [self.prevalence(), self.bias(), self.recall(), self.precision(), self.f1(), self.specificity(), self.accuracy(), self.informedness(),
                self.markedness(), self.mcc()]

    def long_string(self):
        return "\t".join([str(self.tp), str(self.tn), str(self.fp), str(self.fn)] + ["%.2f" % v for v in self.values()])


def mean_line(name, values):
    total = 0.0
    for v in values:
        total = total + v
    sq = 0.0
    for v in values:
        sq = sq + v * v
    n = float(len(values))
    mean = total / n
    var = sq / n - mean * mean
    stdev = math.sqrt(var) if var > 0.0 else 0.0
    return "Mean %-13s: %.2f%% (+/- %.2f%%)\n" % (name, mean, stdev)


def mean_lines(perfs):
    cols = list(zip(*[p.mean_values() for p in perfs]))
    return "".join(mean_line(name, cols[k]) for k, name in enumerate(MEAN_NAMES))


def fold_performances(fold, n_folds, genuine, score, threshold=0.5):
    out = []
    fold, genuine, called = np.asarray(fold), np.asarray(genuine, dtype=bool), np.asarray(score) >= threshold
    for f in range(n_folds):
        m = fold == f
        out.append(Performance((m & genuine & called).sum(), (m & ~genuine & ~called).sum(), (m & ~genuine & called).sum(), (m & genuine & ~called).sum()))
    return out


def cv_results(fold, n_folds, genuine, score, threshold=0.5):
    perfs = fold_performances(fold, n_folds, genuine, score, threshold)
    return "Fold\t" + LONG_HEADER + "\n" + "".join("%d\t%s\n" % (f + 1, p.long_string()) for f, p in enumerate(perfs)) + mean_lines(perfs)


def cv(matrix, fold, n_folds, n_trees, seed, mtry=0, min_node_size=0, dependent_col=0):
    """(pred float64 [n, 2], forests, facts per fold): fold f's forest is grow_model.grow of the rows with fold != f, in their order;
    row r of pred is that forest's walk of row r, for f = fold[r]"""
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    fold = np.asarray(fold)
    pred = np.zeros((len(m), 2), dtype=np.float64)
    forests, facts = [], []
    for f in range(n_folds):
        forest, fact = gm.grow(m[fold != f], n_trees, seed, mtry, min_node_size, dependent_col)
        assert forest.n_classes == 2
        pred[fold == f] = fu.walk_predict(forest, m[fold == f])
        forests.append(forest)
        facts.append(fact)
    return pred, forests, facts
