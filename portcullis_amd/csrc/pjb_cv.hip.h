// pjb_cv.hip.h -- `train --folds`: k-fold cross-validation behind pjb_forest_cv (pjb_model_api.hip).  Fold f's forest is the forest
// pjb_forest_grow grows on the rows the fold does not hold out; the n_folds * n_trees trees of a call are numbered fold after fold
// (tree g: fold g / n_trees, the fold's tree g % n_trees) and grown by the level loop of pjb_grow.hip.h, a batch of them at a time,
// whatever folds the batch cuts through.  Included behind pjb_grow.hip.h (GrowNodes, grow_seed_tree).
//   A tree of fold f sees fewer rows, not another matrix: its lists hold the fold's n_f training rows in their first n_f positions,
// in the column's value order (a stable filter of the sorted rows: rows of one value stay in row order, as the sub-matrix's own stable
// sort leaves them), and the held-out rows behind them.  The root owns [0, n_f).  The held-out rows' node_of is the node slot M - 1,
// which a tree of n_f < n rows never makes (2 n_f - 1 nodes at most) and whose `child` stays 0: kt_split sees such a row as a closed
// segment of its own, kt_partition leaves it where it is, kt_assign does not move it.  kt_draw .. kt_pack run unchanged; every list
// walk takes n positions where the sub-matrix's own tree would take n_f.
//     kc_seed    one lane per tree: the generator of the fold's tree, the root over the fold's training rows, slot M - 1 closed
//     kc_lists   one wave per (tree, column): the column's sorted rows, training rows first, held-out rows behind (a ballot prefix)
//     kc_park    one lane per (tree, row): node_of 0 for a training row, M - 1 for a held-out one
//     kc_score   one lane per row: the row walks the trees of its own fold that the batch holds, in tree order, from the root by
//                kt_assign's rule (`<=` goes left), and adds the terminal node's ((count - sum) / count) / n_trees and
//                (sum / count) / n_trees to its two sums -- the quotients pjb_forest_load makes, added as kr_forest adds them; the
//                sums stay on the device from batch to batch, so the order is the tree order however the trees were batched
#pragma once

namespace pjb {

__global__ __launch_bounds__(64) void kc_seed(u64 *state, u32 T, u32 g0, u32 n_trees, u32 seed, GrowNodes nd, u32 M, u32 *lvl, const u32 *fold_n,
                                               const u32 *fold_sum) {
    const u32 t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const u32 g = g0 + t, f = g / n_trees;
    grow_seed_tree(state, T, t, g % n_trees, seed, nd, M, lvl, fold_n[f], fold_sum[f]);
    nd.child[(size_t)t * M + M - 1] = 0; // the slot the held-out rows are parked on: never split, never open
}

// column blockIdx.x of tree blockIdx.y; fold_n[f]: the rows fold f trains on
__global__ __launch_bounds__(64) void kc_lists(const u32 *sorted, u32 *lists, const u32 *fold, const u32 *fold_n, u32 g0, u32 n_trees, u32 n, u32 C, u32 dep) {
    const u32 c = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    if (c == dep) return; // (its list is never read)
    const u32 f = (g0 + t) / n_trees, nf = fold_n[f];
    const u32 *src = sorted + (size_t)c * n;
    u32 *dst = lists + ((size_t)t * C + c) * n;
    u32 kept = 0; // training rows in front of this trip
    for (u32 base = 0; base < n; base += 64) {
        const u32 i = base + lane;
        const bool valid = i < n;
        const u32 row = valid ? src[i] : 0u;
        const bool train = valid && fold[row] != f;
        const u64 mask = __ballot(train);
        const u32 before = kept + (u32)__popcll(mask & ((1ull << lane) - 1ull));
        if (valid) {
            const u32 to = train ? before : nf + (i - before);
            if (to < n) dst[to] = row; // (always: nf is the number of rows with fold[row] != f)
        }
        kept += (u32)__popcll(mask);
    }
}

__global__ __launch_bounds__(256) void kc_park(u32 *node_of, const u32 *fold, u32 g0, u32 n_trees, u32 n, u32 M) {
    const u32 row = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (row >= n) return;
    node_of[(size_t)t * n + row] = fold[row] == (g0 + t) / n_trees ? M - 1 : 0u;
}

// the trees g0 .. g0 + T - 1 are grown; pred: n x 2, the sums so far
__global__ __launch_bounds__(256) void kc_score(GrowNodes nd, u32 M, const double *col, const u32 *fold, u32 g0, u32 T, u32 n_trees, u32 n, double *pred) {
    const u32 row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const u64 first = (u64)fold[row] * n_trees; // the row's fold's trees: first .. first + n_trees - 1
    const u64 lo = first > g0 ? first : g0, hi = first + n_trees < (u64)g0 + T ? first + n_trees : (u64)g0 + T;
    if (lo >= hi) return;
    double p0 = pred[(size_t)row * 2], p1 = pred[(size_t)row * 2 + 1];
    const double nt = (double)n_trees;
    for (u64 g = lo; g < hi; g++) {
        const size_t tree = (size_t)(g - g0) * M;
        u32 node = 0;
        for (u32 ch; (ch = nd.child[tree + node]) != 0 && ch + 1 < M;) // (ch + 1 < M: true of every child kt_decide numbered)
            node = col[(size_t)nd.var[tree + node] * n + row] <= nd.val[tree + node] ? ch : ch + 1;
        const double cnt = (double)nd.count[tree + node], ones = (double)nd.sum[tree + node];
        p0 += (cnt - ones) / cnt / nt;
        p1 += ones / cnt / nt;
    }
    pred[(size_t)row * 2] = p0;
    pred[(size_t)row * 2 + 1] = p1;
}

} // namespace pjb
