// pjb_forest.hip.h -- `filt`'s forest stage: a saved ranger probability forest walked on the device (kr_forest), behind
// pjb_forest_load / pjb_forest_predict / pjb_filt_scores (pjb_model_api.hip).
//   Semantics: Tree::predict (deps/ranger-0.3.8/src/Tree.cpp:125-180) and ForestProbability::predictInternal
// (src/ForestProbability.cpp:111-131): from the root, value <= split value goes left, anything else -- a NaN too -- goes right; the
// terminal node's counts[c] / n_trees are added class by class, tree after tree in file order.
//   Mapping: one lane per row, 256 rows per block, every lane walks tree 0, then tree 1, ...: the per-class sums are the sequential
// f64 sums of the reference, bit for bit (the quotients counts[c] / n_trees are made once, on the host, when the forest is packed: one
// IEEE division each, as in the reference).  The lanes of a block are in the same tree at the same time, so its upper nodes are hits.
//   Node: one 16-byte load (global_load_dwordx4) per visited node -- { f64 split value | u32 child | u32 var }: `child` is the index
// of the LEFT child in the node array of the whole forest, the right child is child + 1 (the host renumbers each tree breadth first
// so that siblings are neighbours); at a terminal node bit 31 of `var` is set and `child` is the node's row in the table of
// quotients (n_classes per row).  The walk ends because pjb_forest_check has made sure that it does before a node is packed.
//   No scratch: nothing is indexed by a run-time value in registers.  The split variable picks a column of the lane's row in global
// memory (a row is 29 or 34 doubles: two to three cache lines the lane comes back to for every node); the column map (variable ->
// column: the identity for pjb_forest_predict, var_feature for the fused path) and the per-class sums live in LDS, the sums as
// [class][lane] so that a wavefront's accesses fall on 64 different banks.
#pragma once

namespace pjb {

struct __attribute__((aligned(16))) ForestNode {
    double split;
    u32 child; // internal: the left child (right = child + 1); terminal: row of the quotient table
    u32 var;   // bit 31: terminal
};
static_assert(sizeof(ForestNode) == 16, "a visited node is one 16-byte load");
constexpr u32 FOREST_LEAF = 0x80000000u;
constexpr int FOREST_BLOCK = 256;

// dynamic LDS: FOREST_BLOCK * n_classes doubles, then n_vars column numbers
__global__ __launch_bounds__(FOREST_BLOCK) void kr_forest(const ForestNode *nodes, const u32 *roots, u32 n_trees, u32 n_classes, u32 n_vars,
                                                           const double *leaf, const double *data, u32 n_rows, u32 stride, const int32_t *colmap,
                                                           double *pred) {
    extern __shared__ double forest_lds[];
    double *acc = forest_lds;
    int32_t *col = (int32_t *)(forest_lds + (size_t)FOREST_BLOCK * n_classes);
    const u32 lane = threadIdx.x;
    for (u32 v = lane; v < n_vars; v += FOREST_BLOCK) col[v] = colmap ? colmap[v] : (int32_t)v;
    for (u32 k = 0; k < n_classes; k++) acc[k * FOREST_BLOCK + lane] = 0.0;
    __syncthreads();
    const u32 r = blockIdx.x * FOREST_BLOCK + lane;
    if (r >= n_rows) return;
    const double *row = data + (size_t)r * stride;
    const uint4 *nd = (const uint4 *)nodes;
    for (u32 t = 0; t < n_trees; t++) {
        uint4 q = nd[roots[t]];
        while (!(q.w & FOREST_LEAF)) {
            const double split = __hiloint2double((int)q.y, (int)q.x);
            const double v = row[col[q.w]];
            q = nd[q.z + (v <= split ? 0u : 1u)];
        }
        const double *lf = leaf + (size_t)q.z * n_classes;
        for (u32 k = 0; k < n_classes; k++) acc[k * FOREST_BLOCK + lane] += lf[k];
    }
    for (u32 k = 0; k < n_classes; k++) pred[(size_t)r * n_classes + k] = acc[k * FOREST_BLOCK + lane];
}

} // namespace pjb
