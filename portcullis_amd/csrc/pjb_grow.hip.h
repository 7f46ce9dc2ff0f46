// pjb_grow.hip.h -- `train`'s forest stage: a ranger 0.3.8 probability forest grown on the device, behind pjb_forest_grow
// (pjb_model_api.hip).  The saved forest is byte for byte the one Forest::saveToFile leaves when ModelFeatures::trainInstance
// calls it (no replacement, sample fraction 1: every tree trains on every row).
//   Semantics: Tree::grow (deps/ranger-0.3.8/src/Tree.cpp:88-123), Tree::splitNode / createPossibleSplitVarSubset (Tree.cpp:232-300),
// drawWithoutReplacementSimple (src/utility.cpp:108-131), TreeProbability::splitNodeInternal / findBestSplit* / addToTerminalNodes
// (src/TreeProbability.cpp:57-73, 91-123, 143-312).  Nodes are numbered in creation order and split in index order, so a level of a
// tree is a contiguous run of node numbers and the whole forest grows level by level, every tree at once.
//   Lists: per tree and column one list of the row numbers, ordered by the column's value inside every node; a node owns the same
// positions [start, start + count) in all lists of its tree, its children share them (left first).  One wave64 walks one list, 64
// positions a trip, with segmented scans across the wave (shuffles; the sums carried from trip to trip in registers): no LDS, no
// atomics on the placement, no size threshold -- a node of 2 rows and a node of 2^28 take the same path.
//     kt_seed       one lane per tree: its mt19937_64 is seeded, its root made
//     kt_fill       the columns' sorted row lists are copied to every tree
//     kt_draw       one lane per tree: the candidate columns of the level's nodes, in node order (the one sequential stream)
//     kt_split      one wave per (tree, column): prefix label sums, the score at every value boundary, the first best per node
//     kt_decide     one wave per tree: terminal rule, first best candidate in draw order, children numbered by a ballot prefix
//     kt_partition  one wave per (tree, column): stable partition of every split node's positions
//     kt_assign     one lane per (tree, row): the row's new node
//     kt_pack       the trees' nodes one after the other for the copy back
//   Exactness: counts and label sums are integers; a score is sl * sl / nl + sr * sr / nr in IEEE doubles, two multiplications, two
// divisions, one addition, nothing contracted (the unit is built with -ffp-contract=off, as the entropy kernel needs it).
#pragma once

namespace pjb {

constexpr int GROW_MT_N = 312, GROW_MT_M = 156;
constexpr int GROW_DRAW_TREES = 16;  // trees of a kt_draw block: their generators live in LDS, 16 * 312 * 8 = 39 936 bytes
constexpr int GROW_SEEN_WORDS = 64;  // PJB_FOREST_MAX_VARS / 32: the "already drawn" bits of one tree's current node

struct __attribute__((aligned(16))) GrowBest {
    double score; // -1: the column has one value only in this node
    u32 pos;      // position of the last row of the left child in the column's list
    u32 sl;       // label sum of the left child
};
static_assert(sizeof(GrowBest) == 16, "one 16-byte store per (node, candidate)");

// The trees' arrays, `M` nodes of room a tree (M = 2 * n_rows: a tree of n rows has at most 2 n - 1 nodes).
struct GrowNodes {
    u32 *start, *count, *sum; // the node's positions in its tree's lists, its rows, its rows of label 1
    u32 *child;               // left child (right = child + 1); 0: terminal (or not decided yet)
    u32 *var;
    double *val;
};

// mt state in global memory between levels: word i of tree t at state[i * T + t]; word 312 is the position.  Tree t of the batch gets
// the generator of the forest's tree `index` and a root of `count` rows, `sum` of them of label 1 (kt_seed; kc_seed of pjb_cv.hip.h).
__device__ inline void grow_seed_tree(u64 *state, u32 T, u32 t, u32 index, u32 seed, GrowNodes nd, u32 M, u32 *lvl, u32 count, u32 sum) {
    // Forest.cpp:409-416: tree_seed = (uint)((i + 1) * seed); std::mt19937_64::seed(value)
    u64 x = (u64)(u32)((index + 1u) * seed);
    state[t] = x;
    for (u32 i = 1; i < GROW_MT_N; i++) {
        x = 6364136223846793005ull * (x ^ (x >> 62)) + i;
        state[(size_t)i * T + t] = x;
    }
    state[(size_t)GROW_MT_N * T + t] = GROW_MT_N;
    const size_t r = (size_t)t * M;
    nd.start[r] = 0;
    nd.count[r] = count;
    nd.sum[r] = sum;
    nd.child[r] = 0;
    nd.var[r] = 0;
    nd.val[r] = 0.0;
    lvl[t] = 0;
    lvl[T + t] = 1;
}

__global__ __launch_bounds__(64) void kt_seed(u64 *state, u32 T, u32 tree0, u32 seed, GrowNodes nd, u32 M, u32 *lvl, u32 n, u32 label_sum) {
    const u32 t = blockIdx.x * 64 + threadIdx.x;
    if (t < T) grow_seed_tree(state, T, t, tree0 + t, seed, nd, M, lvl, n, label_sum);
}

__global__ __launch_bounds__(256) void kt_fill(const u32 *sorted, u32 *lists, u64 per_tree, u64 total) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < total) lists[i] = sorted[i % per_tree];
}

// The draws of one level.  std::uniform_int_distribution<size_t>(0, n_cols - 2) as libstdc++ 11 (GCC 11.4, bits/uniform_int_dist.h,
// _S_nd<unsigned __int128>) makes it from a 64-bit generator: Lemire's multiply-high with a rejection threshold -- product = g() * range
// in 128 bits, the low half below range is looked at again, below (2^64 - range) % range it is drawn again, the result is the high half.
__global__ __launch_bounds__(GROW_DRAW_TREES) void kt_draw(u64 *state, u32 T, const u32 *lvl, u32 n_cols, u32 dep, u32 mtry, uint16_t *cand, u32 M) {
    __shared__ u64 mt[GROW_MT_N][GROW_DRAW_TREES];
    __shared__ u32 seen[GROW_SEEN_WORDS][GROW_DRAW_TREES];
    const u32 k = threadIdx.x, t = blockIdx.x * GROW_DRAW_TREES + k;
    if (t >= T) return; // (no barrier below: a lane touches its own column of the arrays only)
    const u32 lb = lvl[t], le = lvl[T + t];
    if (lb >= le) return;
    for (u32 i = 0; i < GROW_MT_N; i++) mt[i][k] = state[(size_t)i * T + t];
    u32 at = (u32)state[(size_t)GROW_MT_N * T + t];
    const u32 words = (n_cols + 31) / 32;
    for (u32 w = 0; w < words; w++) seen[w][k] = 0;
    auto next = [&]() -> u64 {
        if (at >= GROW_MT_N) {
            for (u32 i = 0; i < GROW_MT_N; i++) {
                const u32 i1 = i + 1 < GROW_MT_N ? i + 1 : 0, im = i + GROW_MT_M < GROW_MT_N ? i + GROW_MT_M : i + GROW_MT_M - GROW_MT_N;
                const u64 y = (mt[i][k] & 0xFFFFFFFF80000000ull) | (mt[i1][k] & 0x7FFFFFFFull);
                mt[i][k] = mt[im][k] ^ (y >> 1) ^ ((y & 1) ? 0xB5026F5AA96619E9ull : 0ull);
            }
            at = 0;
        }
        u64 y = mt[at++][k];
        y ^= (y >> 29) & 0x5555555555555555ull;
        y ^= (y << 17) & 0x71D67FFFEDA60000ull;
        y ^= (y << 37) & 0xFFF7EEE000000000ull;
        y ^= y >> 43;
        return y;
    };
    const u64 range = (u64)n_cols - 1, threshold = (0ull - range) % range;
    for (u32 node = lb; node < le; node++) {
        uint16_t *out = cand + ((size_t)t * M + node) * mtry;
        for (u32 r = 0; r < mtry; r++) {
            u32 draw;
            do {
                u64 g = next();
                u64 low = g * range;
                if (low < range)
                    while (low < threshold) {
                        g = next();
                        low = g * range;
                    }
                draw = (u32)__umul64hi(g, range);
                if (draw >= dep) draw++;
            } while (seen[draw >> 5][k] >> (draw & 31) & 1u);
            seen[draw >> 5][k] |= 1u << (draw & 31);
            out[r] = (uint16_t)draw;
        }
        for (u32 w = 0; w < words; w++) seen[w][k] = 0;
    }
    for (u32 i = 0; i < GROW_MT_N; i++) state[(size_t)i * T + t] = mt[i][k];
    state[(size_t)GROW_MT_N * T + t] = at;
}

// findBestSplitValueSmallQ / LargeQ for every open node that drew column blockIdx.x, tree blockIdx.y.
__global__ __launch_bounds__(64) void kt_split(const u32 *lists, const u32 *node_of, const double *col, const uint8_t *label, const u32 *lvl, u32 T,
                                                GrowNodes nd, const uint16_t *cand, GrowBest *best, u32 n, u32 C, u32 dep, u32 mtry, u32 M) {
    const u32 c = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    if (c == dep) return;
    const u32 lb = lvl[t], le = lvl[T + t];
    if (lb >= le) return;
    const u32 *list = lists + ((size_t)t * C + c) * n;
    const double *cv = col + (size_t)c * n;
    u32 carry_sum = 0, carry_pos = 0, carry_sl = 0;
    double carry_score = -1.0;
    for (u32 base = 0; base < n; base += 64) {
        const u32 i = base + lane;
        const bool valid = i < n;
        u32 row = 0, node = 0, st = 0, cnt = 0, sm = 0;
        int rank = -1;
        bool open = false;
        if (valid) {
            row = list[i];
            node = node_of[(size_t)t * n + row];
            open = node >= lb && node < le;
        }
        if (open) {
            const size_t at = (size_t)t * M + node;
            st = nd.start[at];
            cnt = nd.count[at];
            sm = nd.sum[at];
            for (u32 r = 0; r < mtry; r++)
                if (cand[at * mtry + r] == c) rank = (int)r;
        }
        const bool mine = open && rank >= 0;
        // label sums from the node's first position (a row outside the open nodes is a segment of its own)
        u32 s = open ? label[row] : 0u;
        int f = open ? (i == st) : 1;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 ps = __shfl_up(s, d);
            const int pf = __shfl_up(f, d);
            if ((int)lane >= d && !f) {
                s += ps;
                f |= pf;
            }
        }
        if (!f) s += carry_sum;
        carry_sum = __shfl(s, 63);
        // the score where the next row of the node has another value (the node's largest value never splits)
        double score = -1.0;
        if (mine && i + 1 < st + cnt && i + 1 < n) {
            if (cv[list[i + 1]] != cv[row]) {
                const double sl = (double)s, sr = (double)(sm - s), nl = (double)(i - st + 1), nr = (double)(st + cnt - i - 1);
                score = sl * sl / nl + sr * sr / nr;
            }
        }
        // the first best of the node: strict `>` in ascending value order
        double bs = score;
        u32 bp = i, bl = s;
        f = open ? (i == st) : 1;
        for (int d = 1; d < 64; d <<= 1) {
            const double ps = __shfl_up(bs, d);
            const u32 pp = __shfl_up(bp, d), pl = __shfl_up(bl, d);
            const int pf = __shfl_up(f, d);
            if ((int)lane >= d && !f) {
                if (ps >= bs) {
                    bs = ps;
                    bp = pp;
                    bl = pl;
                }
                f |= pf;
            }
        }
        if (!f && carry_score >= bs) {
            bs = carry_score;
            bp = carry_pos;
            bl = carry_sl;
        }
        carry_score = __shfl(bs, 63);
        carry_pos = __shfl(bp, 63);
        carry_sl = __shfl(bl, 63);
        if (mine && i == st + cnt - 1) {
            GrowBest b;
            b.score = bs;
            b.pos = bp;
            b.sl = bl;
            best[((size_t)t * M + node) * mtry + rank] = b;
        }
    }
}

// splitNodeInternal for the level's nodes of tree blockIdx.x, then the numbering of Tree::splitNode: children in node order.
__global__ __launch_bounds__(64) void kt_decide(const u32 *lists, const double *col, u32 *lvl, u32 T, GrowNodes nd, const uint16_t *cand, const GrowBest *best,
                                                 u32 n, u32 C, u32 mtry, u32 M, u32 min_node, u32 *n_new) {
    const u32 t = blockIdx.x, lane = threadIdx.x;
    const u32 lb = lvl[t], le = lvl[T + t];
    if (lb >= le) return;
    u32 next = le;
    for (u32 base = lb; base < le; base += 64) {
        const u32 node = base + lane;
        const size_t at = (size_t)t * M + node;
        bool split = false;
        u32 st = 0, cnt = 0, sm = 0, bvar = 0, bpos = 0, bsl = 0;
        if (node < le) {
            st = nd.start[at];
            cnt = nd.count[at];
            sm = nd.sum[at];
            if (cnt > min_node && sm != 0 && sm != cnt) {
                double bscore = -1.0;
                for (u32 r = 0; r < mtry; r++) {
                    const GrowBest b = best[at * mtry + r];
                    if (b.score > bscore) {
                        bscore = b.score;
                        bvar = cand[at * mtry + r];
                        bpos = b.pos;
                        bsl = b.sl;
                    }
                }
                split = bscore >= 0.0 && bpos >= st && bpos < st + cnt - 1 && bpos < n; // (the positions: true of every score kt_split wrote)
            }
        }
        const u64 mask = __ballot(split);
        const u32 l = next + 2u * (u32)__popcll(mask & ((1ull << lane) - 1ull));
        if (split && l + 1 < M) { // (2 n - 1 nodes at most: always)
            const u32 nl = bpos - st + 1;
            nd.child[at] = l;
            nd.var[at] = bvar;
            nd.val[at] = col[(size_t)bvar * n + lists[((size_t)t * C + bvar) * n + bpos]];
            const size_t a = (size_t)t * M + l;
            nd.start[a] = st;
            nd.count[a] = nl;
            nd.sum[a] = bsl;
            nd.start[a + 1] = st + nl;
            nd.count[a + 1] = cnt - nl;
            nd.sum[a + 1] = sm - bsl;
            nd.child[a] = nd.child[a + 1] = 0;
            nd.var[a] = nd.var[a + 1] = 0;
            nd.val[a] = nd.val[a + 1] = 0.0;
        }
        next += 2u * (u32)__popcll(mask);
    }
    if (lane == 0) {
        lvl[t] = le;
        lvl[T + t] = next < M ? next : M;
        if (next > le) atomicAdd(n_new, next - le);
    }
}

// Tree::splitNode's assignment of the rows, for every list: `<=` goes left, the order inside a child stays.
__global__ __launch_bounds__(64) void kt_partition(const u32 *in, u32 *out, const u32 *node_of, const double *col, const u32 *lvl, u32 T, GrowNodes nd,
                                                    u32 n, u32 C, u32 dep, u32 M) {
    const u32 c = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    if (c == dep) return;
    if (lvl[t] >= lvl[T + t]) return; // nothing was split in this tree: it is finished and its lists are not read again
    const u32 *list = in + ((size_t)t * C + c) * n;
    u32 *dst = out + ((size_t)t * C + c) * n;
    u32 carry = 0;
    for (u32 base = 0; base < n; base += 64) {
        const u32 i = base + lane;
        const bool valid = i < n;
        u32 row = 0, st = 0, ch = 0, gl = 0;
        size_t at = 0;
        if (valid) {
            row = list[i];
            at = (size_t)t * M + node_of[(size_t)t * n + row];
            ch = nd.child[at];
        }
        if (ch) {
            st = nd.start[at];
            gl = col[(size_t)nd.var[at] * n + row] <= nd.val[at] ? 1u : 0u;
        }
        u32 s = gl;
        int f = ch ? (i == st) : 1;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 ps = __shfl_up(s, d);
            const int pf = __shfl_up(f, d);
            if ((int)lane >= d && !f) {
                s += ps;
                f |= pf;
            }
        }
        if (!f) s += carry;
        carry = __shfl(s, 63);
        if (valid) {
            u32 to = i;
            if (ch) {
                const u32 before = s - gl; // rows of the node in front of this one that go left
                to = gl ? st + before : st + nd.count[(size_t)t * M + ch] + (i - st - before);
            }
            if (to < n) dst[to] = row;
        }
    }
}

__global__ __launch_bounds__(256) void kt_assign(u32 *node_of, const double *col, GrowNodes nd, u32 n, u32 M) {
    const u32 row = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (row >= n) return;
    const size_t at = (size_t)t * M + node_of[(size_t)t * n + row];
    const u32 ch = nd.child[at];
    if (ch) node_of[(size_t)t * n + row] = col[(size_t)nd.var[at] * n + row] <= nd.val[at] ? ch : ch + 1;
}

// tree t's nodes to off[t] .. off[t + 1] of the packed arrays
__global__ __launch_bounds__(256) void kt_pack(GrowNodes nd, u32 M, const u64 *off, u32 *child, u32 *var, double *val, u32 *count, u32 *sum) {
    const u32 t = blockIdx.y;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x, lo = off[t], hi = off[t + 1];
    if (lo + k >= hi) return;
    const size_t at = (size_t)t * M + k;
    child[lo + k] = nd.child[at];
    var[lo + k] = nd.var[at];
    val[lo + k] = nd.val[at];
    count[lo + k] = nd.count[at];
    sum[lo + k] = nd.sum[at];
}

} // namespace pjb
