// pjb_model_api.hip -- the part of the C ABI behind `filt` and `train`: feature rows and the walk of a saved forest (pjb_filt_features,
// pjb_forest_check / _load / _predict, pjb_filt_scores), the training of the Markov models (pjb_markov_train), the growing of a forest
// (pjb_forest_grow), cross-validation (pjb_forest_cv) and self-training's nearest neighbours (pjb_knn); kernels in pjb_features.hip.h,
// pjb_markov.hip.h, pjb_forest.hip.h, pjb_grow.hip.h, pjb_cv.hip.h and pjb_knn.hip.h.  What a context keeps for them is pjb_ctx::model (ModelState, pjb_host.hip.h).
#include "pjb_host.hip.h"
#include "pjb_features.hip.h"
#include "pjb_markov.hip.h"
#include "pjb_forest.hip.h"
#include "pjb_grow.hip.h"
#include "pjb_cv.hip.h"
#include "pjb_knn.hip.h"

// the uploaded genomes as the kernels of `filt` and `train` look them up (c->model.g_refs), and the "a genome is missing" flag cleared
static int genome_refs_queue(pjb_ctx *c) {
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->model.g_refs, std::max<size_t>(c->contigs.size(), 1) * sizeof(GenomeRef)))) return rc;
    if ((rc = ensure(c, c->model.g_bad, sizeof(int)))) return rc;
    std::vector<GenomeRef> refs(std::max<size_t>(c->contigs.size(), 1));
    for (size_t t = 0; t < c->contigs.size(); t++) {
        refs[t].d = c->contigs[t].present ? c->contigs[t].d : nullptr;
        refs[t].len = (int32_t)c->contigs[t].len;
    }
    HIP_TRY(c, hipMemcpyAsync(c->model.g_refs.p, refs.data(), refs.size() * sizeof(GenomeRef), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->model.g_bad.p, 0, sizeof(int), st));
    return PJB_OK;
}

// `filt`: uploads the junctions and the models and queues kg_features on the context's stream; the rows are in c->model.g_out, the "a genome
// is missing" flag in c->model.g_bad.  Nothing waits here (rows and models are pageable: the caller's wait comes before it returns).
static int features_queue(pjb_ctx *c, const pjb_junction_row *rows, size_t n, double mean_read_length, uint32_t l95, const pjb_markov_models *models) {
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->model.g_rows, n * sizeof(pjb_junction_row)))) return rc;
    if ((rc = ensure(c, c->model.g_models, ((size_t)6 * PJB_KMER_TABLE + 2 * PJB_PW_LEN * 5) * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->model.g_out, n * PJB_N_FEATURES * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->model.g_rows.p, rows, n * sizeof(pjb_junction_row), hipMemcpyHostToDevice, st));
    DevModels M;
    memset(&M, 0, sizeof M);
    double *dm = (double *)c->model.g_models.p;
    const double *src[8] = {models->exon, models->intron, models->donor_t, models->donor_f, models->acceptor_t, models->acceptor_f,
                            models->donor_pw, models->acceptor_pw};
    const double **dst[8] = {&M.exon, &M.intron, &M.don_t, &M.don_f, &M.acc_t, &M.acc_f, &M.don_pw, &M.acc_pw};
    size_t at = 0;
    for (int k = 0; k < 8; k++) {
        const size_t cnt = k < 6 ? (size_t)PJB_KMER_TABLE : (size_t)PJB_PW_LEN * 5;
        if (src[k]) {
            HIP_TRY(c, hipMemcpyAsync(dm + at, src[k], cnt * sizeof(double), hipMemcpyHostToDevice, st));
            *dst[k] = dm + at;
        }
        at += cnt;
    }
    M.exon_size = models->exon ? models->exon_size : 0;
    M.intron_size = models->intron ? models->intron_size : 0;
    M.don_pw_size = models->donor_pw ? models->donor_pw_size : 0;
    M.acc_pw_size = models->acceptor_pw ? models->acceptor_pw_size : 0;
    if ((rc = genome_refs_queue(c))) return rc;
    LAUNCH(c, "kg_features", kg_features, dim3((unsigned)((n + 255) / 256)), dim3(256), (const pjb_junction_row *)c->model.g_rows.p, (u32)n,
           (const GenomeRef *)c->model.g_refs.p, (int)c->contigs.size(), M, mean_read_length, (u32)l95, (double *)c->model.g_out.p, (int *)c->model.g_bad.p);
    return PJB_OK;
}

// queues the walk of the context's forest over n rows of `data` (device; `stride` doubles a row); predictions to c->model.r_pred
static int forest_queue(pjb_ctx *c, const double *data, size_t n, u32 stride, const int32_t *colmap) {
    int rc;
    if ((rc = ensure(c, c->model.r_pred, n * (size_t)c->model.r_classes * sizeof(double)))) return rc;
    const size_t lds = (size_t)FOREST_BLOCK * (size_t)c->model.r_classes * sizeof(double) + (size_t)c->model.r_vars * sizeof(int32_t);
    LAUNCH_LDS(c, "kr_forest", kr_forest, dim3((unsigned)((n + FOREST_BLOCK - 1) / FOREST_BLOCK)), dim3(FOREST_BLOCK), lds,
               (const ForestNode *)c->model.r_nodes.p, (const u32 *)c->model.r_roots.p, (u32)c->model.r_trees, (u32)c->model.r_classes, (u32)c->model.r_vars,
               (const double *)c->model.r_leaf.p, data, (u32)n, stride, colmap, (double *)c->model.r_pred.p);
    return PJB_OK;
}

// ---- the stages of pjb_forest_grow and pjb_forest_cv, in the order they call them ------------------------------------
// Device memory one batch of trees may take (lists, nodes, candidates, scores); more trees than fit are grown batch after batch.
static constexpr size_t GROW_POOL_BYTES = (size_t)6 << 30;
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct GrowPlan { // a call that passed its checks
    const char *who;  // the entry point, for the messages
    size_t n, C, dep; // rows, columns, the dependent column
    size_t M;         // node slots of a tree
    size_t n_trees;   // of a forest
    u32 seed, mtry, min_node;
    size_t n_folds;   // pjb_forest_cv: the forests grown side by side, n_folds * n_trees trees in all (pjb_cv.hip.h); 0: pjb_forest_grow
    size_t trees_all() const { return n_trees * std::max<size_t>(n_folds, 1); }
};
struct GrowFolds { // pjb_forest_cv: per row the fold that holds it out; per fold the rows it trains on and those of label 1 among them
    std::vector<u32> fold, train_n, train_sum;
};
struct GrowInput { // the caller's matrix as the kernels read it
    std::vector<double> colmajor;
    std::vector<uint8_t> label; // the dependent column
    u32 label_sum = 0;          // rows of class 1
    std::vector<u32> sorted;    // column by column: the rows in the order of their values
};
struct GrowRoom { // c->model.w_pool, carved for `batch` trees side by side
    size_t batch;
    double *col;
    uint8_t *label;
    u32 *sorted, *n_new, *lists[2], *node_of;
    GrowNodes nd;
    uint16_t *cand;
    GrowBest *best;
    u64 *state;
    u32 *lvl;
    u32 *fold, *fold_n, *fold_sum; // pjb_forest_cv: GrowFolds on the device ...
    double *pred;                  // ... and the held-out rows' sums, n x 2
};

// the argument checks and ranger's defaults
static int grow_plan(pjb_ctx *c, const char *who, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, const void *out, GrowPlan &P) {
    if (!p || !out) return fail(c, PJB_ERR_ARG, "%s: bad arguments", who);
    if (p->n_trees < 1) return fail(c, PJB_ERR_ARG, "%s: %d trees (at least one is needed)", who, p->n_trees);
    if (n_rows < 1) return fail(c, PJB_ERR_ARG, "%s: %lld rows (at least one is needed)", who, (long long)n_rows);
    if (n_cols < 2) return fail(c, PJB_ERR_ARG, "%s: %d columns (the labels and one variable at least)", who, n_cols);
    if (n_cols > PJB_FOREST_MAX_VARS) return fail(c, PJB_ERR_ARG, "%s: %d variables (1 to %d can be walked)", who, n_cols, PJB_FOREST_MAX_VARS);
    if (!data || n_rows > (1ll << 28) || p->n_trees > (1 << 24)) return fail(c, PJB_ERR_ARG, "%s: bad arguments", who);
    if (p->dependent_col < 0 || p->dependent_col >= n_cols)
        return fail(c, PJB_ERR_ARG, "%s: dependent column %d of %d columns", who, p->dependent_col, n_cols);
    if (p->mtry < 0 || p->min_node_size < 0) return fail(c, PJB_ERR_ARG, "%s: mtry %d, node size %d", who, p->mtry, p->min_node_size);
    // ForestProbability::initInternal (ForestProbability.cpp:64-75)
    const u32 mtry = p->mtry ? (u32)p->mtry : std::max<u32>(1, (u32)sqrt((double)(n_cols - 1)));
    const u32 min_node = p->min_node_size ? (u32)p->min_node_size : 10u;
    if (mtry >= (u32)n_cols / 2)
        return fail(c, PJB_ERR_ARG, "%s: mtry %u of %d columns: from n_cols / 2 on ranger draws by Knuth's algorithm, which is not built", who, mtry, n_cols);
    P = GrowPlan{who, (size_t)n_rows, (size_t)n_cols, (size_t)p->dependent_col, 2 * (size_t)n_rows, (size_t)p->n_trees, (u32)p->seed, mtry, min_node, 0};
    return PJB_OK;
}

// the matrix column-major, the labels, and every column's rows in the order of their values
static int grow_input(pjb_ctx *c, const double *data, const GrowPlan &P, GrowInput &in) {
    const size_t n = P.n, C = P.C, dep = P.dep;
    in.colmajor.resize(C * n);
    in.label.resize(n);
    for (size_t r = 0; r < n; r++)
        for (size_t k = 0; k < C; k++) {
            const double v = data[r * C + k];
            if (!std::isfinite(v)) return fail(c, PJB_ERR_ARG, "%s: row %zu, column %zu is not finite", P.who, r, k);
            if (k == dep) {
                if (v != 0.0 && v != 1.0) return fail(c, PJB_ERR_ARG, "%s: row %zu has the label %g (0 or 1)", P.who, r, v);
                in.label[r] = v == 1.0;
                in.label_sum += in.label[r];
            }
            in.colmajor[k * n + r] = v;
        }
    // one sort per column, shared by all trees (Data::sort's order of values; rows of one value in row order)
    in.sorted.resize(C * n);
    for (size_t k = 0; k < C; k++) {
        u32 *s = in.sorted.data() + k * n;
        for (size_t r = 0; r < n; r++) s[r] = (u32)r;
        if (k == dep) continue;
        const double *v = in.colmajor.data() + k * n;
        std::stable_sort(s, s + n, [v](u32 a, u32 b) { return v[a] < v[b]; });
    }
    return PJB_OK;
}

// the room of one batch of trees: how many trees it holds, the pool, and what lies where in it
static int grow_room(pjb_ctx *c, const GrowPlan &P, GrowRoom &R) {
    const size_t n = P.n, C = P.C, M = P.M;
    const u32 mtry = P.mtry;
    // (pjb_forest_cv adds nothing to a tree: the held-out rows lie in the tails of its lists, and are scored from its nodes)
    const size_t cv_bytes = P.n_folds ? up256(n * 4) + 2 * up256(P.n_folds * 4) + up256(n * 16) : 0;
    const size_t shared_bytes = up256(C * n * 8) + up256(n) + up256(C * n * 4) + 256 + cv_bytes;
    const size_t tree_bytes = 2 * C * n * 4 + n * 4 + M * (5 * 4 + 8) + M * mtry * (2 + sizeof(GrowBest)) + (GROW_MT_N + 1) * 8 + 2 * 4;
    size_t batch = c->model.grow_batch ? c->model.grow_batch : std::max<size_t>(1, GROW_POOL_BYTES / tree_bytes);
    batch = std::min<size_t>(std::min<size_t>(batch, P.trees_all()), 32768);
    int rc;
    if ((rc = ensure(c, c->model.w_pool, shared_bytes + batch * tree_bytes + 16 * 256))) return rc;
    uint8_t *at = (uint8_t *)c->model.w_pool.p;
    auto carve = [&](size_t bytes) {
        uint8_t *q = at;
        at += up256(bytes);
        return q;
    };
    R.batch = batch;
    R.col = (double *)carve(C * n * 8);
    R.label = carve(n);
    R.sorted = (u32 *)carve(C * n * 4);
    R.n_new = (u32 *)carve(4);
    R.lists[0] = (u32 *)carve(batch * C * n * 4);
    R.lists[1] = (u32 *)carve(batch * C * n * 4);
    R.node_of = (u32 *)carve(batch * n * 4);
    R.nd.start = (u32 *)carve(batch * M * 4);
    R.nd.count = (u32 *)carve(batch * M * 4);
    R.nd.sum = (u32 *)carve(batch * M * 4);
    R.nd.child = (u32 *)carve(batch * M * 4);
    R.nd.var = (u32 *)carve(batch * M * 4);
    R.nd.val = (double *)carve(batch * M * 8);
    R.cand = (uint16_t *)carve(batch * M * mtry * 2);
    R.best = (GrowBest *)carve(batch * M * mtry * sizeof(GrowBest));
    R.state = (u64 *)carve(batch * (GROW_MT_N + 1) * 8);
    R.lvl = (u32 *)carve(batch * 2 * 4);
    R.fold = R.fold_n = R.fold_sum = nullptr;
    R.pred = nullptr;
    if (P.n_folds) {
        R.fold = (u32 *)carve(n * 4);
        R.fold_n = (u32 *)carve(P.n_folds * 4);
        R.fold_sum = (u32 *)carve(P.n_folds * 4);
        R.pred = (double *)carve(n * 16);
    }
    return PJB_OK;
}

// grows the trees t0 .. t0 + T - 1 level by level until none of them makes a node: one wait per level.  Trees of pjb_forest_cv are
// numbered fold after fold and start from their fold's rows (pjb_cv.hip.h); the level loop is the same and does not know of folds.
static int grow_batch(pjb_ctx *c, const GrowPlan &P, const GrowRoom &R, u32 label_sum, size_t t0, u32 T) {
    hipStream_t st = c->stream;
    const size_t n = P.n, C = P.C, dep = P.dep, M = P.M;
    const u32 mtry = P.mtry;
    if (P.n_folds) {
        LAUNCH(c, "kc_seed", kc_seed, dim3((T + 63) / 64), dim3(64), R.state, T, (u32)t0, (u32)P.n_trees, P.seed, R.nd, (u32)M, R.lvl, (const u32 *)R.fold_n,
               (const u32 *)R.fold_sum);
        LAUNCH(c, "kc_lists", kc_lists, dim3((unsigned)C, T), dim3(64), (const u32 *)R.sorted, R.lists[0], (const u32 *)R.fold, (const u32 *)R.fold_n, (u32)t0,
               (u32)P.n_trees, (u32)n, (u32)C, (u32)dep);
        LAUNCH(c, "kc_park", kc_park, dim3((unsigned)((n + 255) / 256), T), dim3(256), R.node_of, (const u32 *)R.fold, (u32)t0, (u32)P.n_trees, (u32)n, (u32)M);
    } else {
        LAUNCH(c, "kt_seed", kt_seed, dim3((T + 63) / 64), dim3(64), R.state, T, (u32)t0, P.seed, R.nd, (u32)M, R.lvl, (u32)n, label_sum);
        const u64 total = (u64)T * C * n;
        LAUNCH(c, "kt_fill", kt_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), (const u32 *)R.sorted, R.lists[0], (u64)(C * n), total);
        HIP_TRY(c, hipMemsetAsync(R.node_of, 0, (size_t)T * n * 4, st));
    }
    int cur = 0;
    // one trip per level: at most n_rows levels (every split leaves both children smaller); the one read-back says whether nodes were made
    for (size_t level = 0; level <= n; level++) {
        u32 n_new = 0;
        HIP_TRY(c, hipMemsetAsync(R.n_new, 0, 4, st));
        LAUNCH(c, "kt_draw", kt_draw, dim3((T + GROW_DRAW_TREES - 1) / GROW_DRAW_TREES), dim3(GROW_DRAW_TREES), R.state, T, (const u32 *)R.lvl, (u32)C, (u32)dep,
               mtry, R.cand, (u32)M);
        LAUNCH(c, "kt_split", kt_split, dim3((unsigned)C, T), dim3(64), (const u32 *)R.lists[cur], (const u32 *)R.node_of, (const double *)R.col,
               (const uint8_t *)R.label, (const u32 *)R.lvl, T, R.nd, (const uint16_t *)R.cand, R.best, (u32)n, (u32)C, (u32)dep, mtry, (u32)M);
        LAUNCH(c, "kt_decide", kt_decide, dim3(T), dim3(64), (const u32 *)R.lists[cur], (const double *)R.col, R.lvl, T, R.nd, (const uint16_t *)R.cand,
               (const GrowBest *)R.best, (u32)n, (u32)C, mtry, (u32)M, P.min_node, R.n_new);
        HIP_TRY(c, hipMemcpyAsync(&n_new, R.n_new, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->ktime) ev_collect(c, MISC_POOL);
        if (!n_new) break;
        LAUNCH(c, "kt_partition", kt_partition, dim3((unsigned)C, T), dim3(64), (const u32 *)R.lists[cur], R.lists[cur ^ 1], (const u32 *)R.node_of,
               (const double *)R.col, (const u32 *)R.lvl, T, R.nd, (u32)n, (u32)C, (u32)dep, (u32)M);
        LAUNCH(c, "kt_assign", kt_assign, dim3((unsigned)((n + 255) / 256), T), dim3(256), R.node_of, (const double *)R.col, R.nd, (u32)n, (u32)M);
        cur ^= 1;
    }
    return PJB_OK;
}

struct GrowPacked { // the nodes of a batch's trees on the host: tree t owns off[t] .. off[t + 1]
    std::vector<u64> off;
    std::vector<u32> child, var, count, sum;
    std::vector<double> val;
};

// the nodes of the batch's trees, packed one tree after the other on the device and read back: two waits
static int grow_read(pjb_ctx *c, const GrowPlan &P, const GrowRoom &R, size_t t0, u32 T, GrowPacked &K) {
    hipStream_t st = c->stream;
    const size_t M = P.M;
    int rc;
    std::vector<u32> lvl((size_t)2 * T);
    HIP_TRY(c, hipMemcpyAsync(lvl.data(), R.lvl, (size_t)2 * T * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    std::vector<u64> &off = K.off;
    off.assign((size_t)T + 1, 0);
    u32 most = 0;
    for (u32 t = 0; t < T; t++) {
        const u32 nodes = lvl[(size_t)T + t]; // (the end of the last level: the tree's node count)
        if (lvl[t] != nodes || nodes < 1 || nodes >= M) return fail(c, PJB_ERR_STATE, "%s: tree %zu did not finish (%u nodes)", P.who, t0 + t, nodes);
        off[t + 1] = off[t] + nodes;
        most = std::max(most, nodes);
    }
    const size_t N = (size_t)off[T];
    if ((rc = ensure(c, c->model.w_pack, up256((T + 1) * 8) + 4 * up256(N * 4) + up256(N * 8)))) return rc;
    uint8_t *q = (uint8_t *)c->model.w_pack.p;
    u64 *d_off = (u64 *)q;
    q += up256((T + 1) * 8);
    u32 *p_child = (u32 *)q, *p_var = (u32 *)(q + up256(N * 4)), *p_count = (u32 *)(q + 2 * up256(N * 4)), *p_sum = (u32 *)(q + 3 * up256(N * 4));
    double *p_val = (double *)(q + 4 * up256(N * 4));
    HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), (T + 1) * 8, hipMemcpyHostToDevice, st));
    LAUNCH(c, "kt_pack", kt_pack, dim3((most + 255) / 256, T), dim3(256), R.nd, (u32)M, (const u64 *)d_off, p_child, p_var, p_val, p_count, p_sum);
    std::vector<u32> &h_child = K.child, &h_var = K.var, &h_count = K.count, &h_sum = K.sum;
    std::vector<double> &h_val = K.val;
    for (std::vector<u32> *v : {&h_child, &h_var, &h_count, &h_sum}) v->resize(N);
    h_val.resize(N);
    HIP_TRY(c, hipMemcpyAsync(h_child.data(), p_child, N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_var.data(), p_var, N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_count.data(), p_count, N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_sum.data(), p_sum, N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_val.data(), p_val, N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

// the batch's trees ta .. tb - 1 appended to G
static void grow_append(const GrowPacked &B, u32 ta, u32 tb, u32 label_sum, ModelState::GrowOut &G) {
    const std::vector<u64> &off = B.off;
    const std::vector<u32> &h_child = B.child, &h_var = B.var, &h_count = B.count, &h_sum = B.sum;
    const std::vector<double> &h_val = B.val;
    const size_t K = G.class_values.size();
    for (u32 t = ta; t < tb; t++) {
        for (u64 k = off[t]; k < off[t + 1]; k++) {
            if (h_child[k]) {
                G.left.push_back((int32_t)h_child[k]);
                G.right.push_back((int32_t)h_child[k] + 1);
                G.count_off.push_back(-1);
            } else { // addToTerminalNodes: count[class] / n, one division each
                G.left.push_back(-1);
                G.right.push_back(-1);
                G.count_off.push_back((int64_t)G.counts.size());
                const double cnt = (double)h_count[k], ones = (double)h_sum[k];
                if (K == 2) G.counts.push_back((cnt - ones) / cnt);
                G.counts.push_back((K == 2 || label_sum > 0 ? ones : cnt) / cnt);
            }
            G.split_var.push_back((int32_t)h_var[k]);
            G.split_value.push_back(h_val[k]);
        }
        G.tree_off.push_back((int64_t)G.left.size());
    }
}

// what the caller gets: a view of G (it lives until the context's next call of the same entry point), checked like a forest from a file
static int grow_view(pjb_ctx *c, const GrowPlan &P, const ModelState::GrowOut &G, pjb_grow_result *out) {
    pjb_forest &f = out->forest;
    memset(&f, 0, sizeof f);
    f.n_trees = (int32_t)P.n_trees;
    f.n_classes = (int32_t)G.class_values.size();
    f.n_vars = (int32_t)P.C;
    f.dependent_var = (int32_t)P.dep;
    f.is_ordered = G.is_ordered.data();
    f.tree_off = G.tree_off.data();
    f.left = G.left.data();
    f.right = G.right.data();
    f.split_var = G.split_var.data();
    f.split_value = G.split_value.data();
    f.count_off = G.count_off.data();
    f.counts = G.counts.data();
    f.n_counts = (int64_t)G.counts.size();
    out->class_values = G.class_values.data();
    char msg[200] = "";
    if (pjb_forest_check(&f, msg, (int)sizeof msg) != PJB_OK) return fail(c, PJB_ERR_STATE, "%s: the grown forest cannot be walked: %s", P.who, msg);
    return PJB_OK;
}

extern "C" {
int pjb_filt_features(pjb_ctx *c, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                      const pjb_markov_models *models, double *features_out) {
    if (!c) return PJB_ERR_ARG;
    if (n_rows < 0 || (n_rows > 0 && (!rows || !features_out)) || !models || n_rows > 0xfffffff0ll)
        return fail(c, PJB_ERR_ARG, "pjb_filt_features: bad arguments");
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = features_queue(c, rows, n, mean_read_length, l95, models))) return rc;
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(features_out, c->model.g_out.p, n * PJB_N_FEATURES * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, c->model.g_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (bad) return fail(c, PJB_ERR_STATE, "pjb_filt_features: a junction lies on a target whose genome was not uploaded");
    return PJB_OK;
}

// Blocks km_count spreads one model's segments over: two fit a CU beside each other (LDS), and every block pays for clearing and
// flushing 15 625 counters, so a block gets MARKOV_MIN_SEGS segments at least.
static constexpr u64 MARKOV_MAX_BLOCKS = 512, MARKOV_MIN_SEGS = 16;
// ... and at most this many: 2^19 segments of 4096 bases keep every u32 counter of a block's LDS below 2^31
static constexpr u64 MARKOV_MAX_SEGS = (u64)1 << 19;

int pjb_markov_train(pjb_ctx *c, const pjb_junction_row *rows, int64_t n_rows, const int64_t *cp_idx, int64_t n_cp, const int64_t *pass_idx,
                     int64_t n_pass, const int64_t *fail_idx, int64_t n_fail, pjb_markov_tables *out) {
    if (!c) return PJB_ERR_ARG;
    const int64_t *idx[MK_LISTS] = {cp_idx, pass_idx, fail_idx};
    const int64_t n_idx[MK_LISTS] = {n_cp, n_pass, n_fail};
    static const char *const list_name[MK_LISTS] = {"cp", "pass", "fail"};
    if (!out || n_rows < 0 || (n_rows > 0 && !rows) || n_rows > 0xfffffff0ll) return fail(c, PJB_ERR_ARG, "pjb_markov_train: bad arguments");
    size_t n_all = 0;
    for (int l = 0; l < MK_LISTS; l++) {
        if (n_idx[l] < 0 || n_idx[l] > 0x3ffffff0ll || (n_idx[l] > 0 && !idx[l]))
            return fail(c, PJB_ERR_ARG, "pjb_markov_train: the %s list has %lld entries", list_name[l], (long long)n_idx[l]);
        for (int64_t k = 0; k < n_idx[l]; k++)
            if (idx[l][k] < 0 || idx[l][k] >= n_rows)
                return fail(c, PJB_ERR_ARG, "pjb_markov_train: entry %lld of the %s list is row %lld of %lld rows", (long long)k, list_name[l],
                            (long long)idx[l][k], (long long)n_rows);
        n_all += (size_t)n_idx[l];
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows, TAB = (size_t)MARKOV_ROWS * 5;
    int rc;
    if ((rc = ensure(c, c->model.g_rows, std::max<size_t>(n, 1) * sizeof(pjb_junction_row)))) return rc;
    if ((rc = ensure(c, c->model.m_idx, std::max<size_t>(n_all, 1) * sizeof(int64_t)))) return rc;
    if ((rc = ensure(c, c->model.m_counts, TAB * sizeof(u64)))) return rc;
    if ((rc = ensure(c, c->model.m_tables, TAB * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->model.m_sizes, 8 * sizeof(int) + sizeof(u64)))) return rc;
    MarkovJob J;
    memset(&J, 0, sizeof J);
    J.rows = (const pjb_junction_row *)c->model.g_rows.p;
    J.n_refs = (int)c->contigs.size();
    if (n) HIP_TRY(c, hipMemcpyAsync(c->model.g_rows.p, rows, n * sizeof(pjb_junction_row), hipMemcpyHostToDevice, st));
    size_t at = 0;
    for (int l = 0; l < MK_LISTS; l++) {
        J.idx[l] = (const int64_t *)c->model.m_idx.p + at;
        J.n_idx[l] = (u32)n_idx[l];
        if (n_idx[l]) HIP_TRY(c, hipMemcpyAsync((int64_t *)c->model.m_idx.p + at, idx[l], (size_t)n_idx[l] * sizeof(int64_t), hipMemcpyHostToDevice, st));
        at += (size_t)n_idx[l];
    }
    const u64 wins[MK_KMER_MODELS] = {2 * (u64)n_cp, (u64)n_cp, (u64)n_pass, (u64)n_fail, (u64)n_pass, (u64)n_fail};
    u64 W = 0;
    for (int m = 0; m < MK_KMER_MODELS; m++) {
        J.win_off[m] = (u32)W;
        W += wins[m];
    }
    if (W > 0xfffffff0ull) return fail(c, PJB_ERR_ARG, "pjb_markov_train: %llu windows", (unsigned long long)W);
    J.win_off[MK_KMER_MODELS] = (u32)W;
    if ((rc = ensure(c, c->model.m_nseg, std::max<size_t>((size_t)W, 1) * sizeof(u32)))) return rc;
    if ((rc = ensure(c, c->model.m_off, ((size_t)W + 1) * sizeof(u64)))) return rc;
    if ((rc = genome_refs_queue(c))) return rc;
    J.genomes = (const GenomeRef *)c->model.g_refs.p;
    u64 *counts = (u64 *)c->model.m_counts.p, *seg_off = (u64 *)c->model.m_off.p;
    int *sizes = (int *)c->model.m_sizes.p, *bad_d = (int *)c->model.g_bad.p;
    HIP_TRY(c, hipMemsetAsync(counts, 0, TAB * sizeof(u64), st));
    HIP_TRY(c, hipMemsetAsync(sizes, 0, 8 * sizeof(int) + sizeof(u64), st));
    // the windows' segments and their prefix; the six models' totals come back (one wait) to size the grids
    u64 bound[MK_KMER_MODELS + 1] = {};
    if (W) {
        LAUNCH(c, "km_windows", km_windows, dim3((unsigned)((W + 255) / 256)), dim3(256), J, (u32 *)c->model.m_nseg.p, bad_d);
        if ((rc = run_scan(c, "km_scan", ArrU32Fn{(const u32 *)c->model.m_nseg.p}, MarkovOffSink{seg_off}, W, seg_off + W))) return rc;
        for (int m = 0; m <= MK_KMER_MODELS; m++) HIP_TRY(c, hipMemcpyAsync(&bound[m], seg_off + J.win_off[m], sizeof(u64), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    for (int m = 0; m < MK_KMER_MODELS; m++) {
        const u64 segs = bound[m + 1] - bound[m];
        if (!segs) continue;
        const u64 blocks = std::max(std::min(MARKOV_MAX_BLOCKS, (segs + MARKOV_MIN_SEGS - 1) / MARKOV_MIN_SEGS), (segs + MARKOV_MAX_SEGS - 1) / MARKOV_MAX_SEGS);
        if (blocks > 0x7fffffffull) return fail(c, PJB_ERR_ARG, "pjb_markov_train: %llu segments in one model", (unsigned long long)segs);
        LAUNCH(c, "km_count", km_count, dim3((unsigned)blocks), dim3(256), J, m, (const u64 *)seg_off, counts);
    }
    if (n_pass) LAUNCH(c, "km_pos", km_pos, dim3((unsigned)((n_pass + 255) / 256)), dim3(256), J, counts, bad_d);
    LAUNCH(c, "km_normalise", km_normalise, dim3((MARKOV_ROWS + 255) / 256), dim3(256), (const u64 *)counts, (double *)c->model.m_tables.p, sizes,
           (unsigned long long *)(sizes + 8));
    c->model.markov_out.assign(TAB, 0.0);
    int bad = 0;
    struct { int sizes[8]; u64 transitions; } tail;
    HIP_TRY(c, hipMemcpyAsync(c->model.markov_out.data(), c->model.m_tables.p, TAB * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&tail, sizes, sizeof tail, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, bad_d, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (bad) return fail(c, PJB_ERR_STATE, "pjb_markov_train: a junction lies on a target whose genome was not uploaded");
    const double *t = c->model.markov_out.data();
    memset(out, 0, sizeof *out);
    const double **dst[8] = {&out->models.exon, &out->models.intron, &out->models.donor_t, &out->models.donor_f, &out->models.acceptor_t,
                             &out->models.acceptor_f, &out->models.donor_pw, &out->models.acceptor_pw};
    for (int k = 0; k < 8; k++) {
        *dst[k] = t + (k < 6 ? (size_t)k * PJB_KMER_TABLE : (size_t)6 * PJB_KMER_TABLE + (size_t)(k - 6) * PJB_PW_LEN * 5);
        out->sizes[k] = tail.sizes[k];
    }
    out->models.exon_size = tail.sizes[0];
    out->models.intron_size = tail.sizes[1];
    out->models.donor_pw_size = tail.sizes[6];
    out->models.acceptor_pw_size = tail.sizes[7];
    out->transitions = tail.transitions;
    return PJB_OK;
}

int pjb_forest_check(const pjb_forest *f, char *msg, int len) {
    auto no = [&](const char *fmt, long long a, long long b) {
        if (msg && len > 0) snprintf(msg, (size_t)len, fmt, a, b);
        return PJB_ERR_ARG;
    };
    if (!f) return no("pjb_forest_check: no forest", 0, 0);
    if (f->n_trees < 1) return no("forest: %lld trees (at least one is needed)", f->n_trees, 0);
    if (f->n_classes < 1 || f->n_classes > PJB_FOREST_MAX_CLASSES) return no("forest: %lld classes (1 to %lld can be walked)", f->n_classes, PJB_FOREST_MAX_CLASSES);
    if (f->n_vars < 1 || f->n_vars > PJB_FOREST_MAX_VARS) return no("forest: %lld variables (1 to %lld can be walked)", f->n_vars, PJB_FOREST_MAX_VARS);
    if (f->dependent_var < 0 || f->dependent_var >= f->n_vars) return no("forest: dependent variable %lld of %lld variables", f->dependent_var, f->n_vars);
    if (!f->tree_off || !f->left || !f->right || !f->split_var || !f->split_value || !f->count_off || (!f->counts && f->n_counts > 0) || f->n_counts < 0)
        return no("forest: an array is missing", 0, 0);
    if (f->is_ordered)
        for (int32_t v = 0; v < f->n_vars; v++)
            if (!f->is_ordered[v]) return no("forest: variable %lld is unordered (only ordered variables can be walked)", v, 0);
    if (f->tree_off[0] != 0) return no("forest: the first tree starts at node %lld", (long long)f->tree_off[0], 0);
    if (f->tree_off[f->n_trees] > 0x7ffffff0ll) return no("forest: %lld nodes", (long long)f->tree_off[f->n_trees], 0);
    std::vector<uint8_t> has_parent;
    for (int32_t t = 0; t < f->n_trees; t++) {
        const int64_t base = f->tree_off[t], n = f->tree_off[t + 1] - base;
        if (n < 1 || n > 0x7ffffff0ll) return no("forest: tree %lld has %lld nodes", t, (long long)n);
        has_parent.assign((size_t)n, 0);
        for (int64_t k = 0; k < n; k++) {
            const int64_t l = f->left[base + k], r = f->right[base + k];
            if (l < 0 && r < 0) { // terminal
                const int64_t at = f->count_off[base + k];
                if (at < 0 || at > f->n_counts - f->n_classes) return no("forest: tree %lld, node %lld: a terminal node without its class counts", t, (long long)k);
                continue;
            }
            if (l < 0 || r < 0) return no("forest: tree %lld, node %lld has one child only", t, (long long)k);
            if (l >= n || r >= n) return no("forest: tree %lld, node %lld: a child lies outside the tree", t, (long long)k);
            if (l <= k || r <= k) return no("forest: tree %lld, node %lld: a child is not behind its parent", t, (long long)k);
            if (l == r || has_parent[(size_t)l] || has_parent[(size_t)r]) return no("forest: tree %lld, node %lld: a child has two parents", t, (long long)k);
            has_parent[(size_t)l] = has_parent[(size_t)r] = 1;
            const int32_t v = f->split_var[base + k];
            if (v < 0 || v >= f->n_vars) return no("forest: tree %lld, node %lld splits on a variable the data does not have", t, (long long)k);
            if (v == f->dependent_var) return no("forest: tree %lld, node %lld splits on the dependent variable", t, (long long)k);
        }
    }
    return PJB_OK;
}

int pjb_forest_load(pjb_ctx *c, const pjb_forest *f) {
    if (!c) return PJB_ERR_ARG;
    char msg[200] = "";
    if (pjb_forest_check(f, msg, (int)sizeof msg) != PJB_OK) return fail(c, PJB_ERR_ARG, "pjb_forest_load: %s", msg);
    // pack: each tree breadth first from its root, so that the two children of a node are neighbours (nodes nothing leads to are dropped)
    std::vector<ForestNode> nodes;
    std::vector<double> leaf;
    std::vector<u32> roots((size_t)f->n_trees);
    std::vector<int64_t> order;
    nodes.reserve((size_t)f->tree_off[f->n_trees]);
    for (int32_t t = 0; t < f->n_trees; t++) {
        const int64_t base = f->tree_off[t];
        const size_t first = nodes.size();
        roots[(size_t)t] = (u32)first;
        order.assign(1, 0);
        for (size_t at = 0; at < order.size(); at++) {
            const int64_t k = base + order[at];
            ForestNode nd;
            if (f->left[k] < 0) {
                nd.split = 0.0;
                nd.child = (u32)(leaf.size() / (size_t)f->n_classes);
                nd.var = FOREST_LEAF;
                for (int32_t cl = 0; cl < f->n_classes; cl++) leaf.push_back(f->counts[f->count_off[k] + cl] / (double)f->n_trees);
            } else {
                nd.split = f->split_value[k];
                nd.child = (u32)(first + order.size());
                nd.var = (u32)f->split_var[k];
                order.push_back(f->left[k]);
                order.push_back(f->right[k]);
            }
            nodes.push_back(nd);
        }
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    HIP_TRY(c, hipStreamSynchronize(st)); // (the arrays below are pageable, and a walk of the old forest may be queued)
    c->model.r_trees = 0;
    int rc;
    if ((rc = ensure(c, c->model.r_nodes, nodes.size() * sizeof(ForestNode)))) return rc;
    if ((rc = ensure(c, c->model.r_leaf, leaf.size() * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->model.r_roots, roots.size() * sizeof(u32)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->model.r_nodes.p, nodes.data(), nodes.size() * sizeof(ForestNode), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->model.r_leaf.p, leaf.data(), leaf.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->model.r_roots.p, roots.data(), roots.size() * sizeof(u32), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->model.r_trees = f->n_trees;
    c->model.r_classes = f->n_classes;
    c->model.r_vars = f->n_vars;
    c->model.r_dep = f->dependent_var;
    return PJB_OK;
}

int pjb_forest_predict(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, double *pred) {
    if (!c) return PJB_ERR_ARG;
    if (!c->model.r_trees) return fail(c, PJB_ERR_STATE, "pjb_forest_predict: no forest was loaded (pjb_forest_load)");
    if (n_rows < 0 || n_rows > 0xfffffff0ll || (n_rows > 0 && (!data || !pred))) return fail(c, PJB_ERR_ARG, "pjb_forest_predict: bad arguments");
    if (n_cols != c->model.r_vars) return fail(c, PJB_ERR_ARG, "pjb_forest_predict: the data has %d columns, the forest %d variables", n_cols, c->model.r_vars);
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = ensure(c, c->model.r_data, n * (size_t)n_cols * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->model.r_data.p, data, n * (size_t)n_cols * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = forest_queue(c, (const double *)c->model.r_data.p, n, (u32)n_cols, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(pred, c->model.r_pred.p, n * (size_t)c->model.r_classes * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

int pjb_filt_scores(pjb_ctx *c, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                    const pjb_markov_models *models, const int32_t *var_feature, double *pred, double *features_out) {
    if (!c) return PJB_ERR_ARG;
    if (!c->model.r_trees) return fail(c, PJB_ERR_STATE, "pjb_filt_scores: no forest was loaded (pjb_forest_load)");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !pred)) || !models || !var_feature || n_rows > 0xfffffff0ll)
        return fail(c, PJB_ERR_ARG, "pjb_filt_scores: bad arguments");
    std::vector<int32_t> colmap((size_t)c->model.r_vars, 0);
    for (int32_t v = 0; v < c->model.r_vars; v++) {
        if (v == c->model.r_dep) continue; // (never read)
        if (var_feature[v] < 0 || var_feature[v] >= PJB_N_FEATURES)
            return fail(c, PJB_ERR_ARG, "pjb_filt_scores: variable %d is column %d of a feature row of %d", v, var_feature[v], PJB_N_FEATURES);
        colmap[(size_t)v] = var_feature[v];
    }
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = ensure(c, c->model.r_colmap, colmap.size() * sizeof(int32_t)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->model.r_colmap.p, colmap.data(), colmap.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = features_queue(c, rows, n, mean_read_length, l95, models))) return rc;
    if ((rc = forest_queue(c, (const double *)c->model.g_out.p, n, (u32)PJB_N_FEATURES, (const int32_t *)c->model.r_colmap.p))) return rc;
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(pred, c->model.r_pred.p, n * (size_t)c->model.r_classes * sizeof(double), hipMemcpyDeviceToHost, st));
    if (features_out) HIP_TRY(c, hipMemcpyAsync(features_out, c->model.g_out.p, n * PJB_N_FEATURES * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, c->model.g_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st)); // (the one wait; colmap is pageable and lives until here)
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (bad) return fail(c, PJB_ERR_STATE, "pjb_filt_scores: a junction lies on a target whose genome was not uploaded");
    return PJB_OK;
}

// Forest::grow for ForestProbability as ModelFeatures::trainInstance sets it up: see include/portcullis_amd.h and pjb_grow.hip.h.
int pjb_forest_grow(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, pjb_grow_result *out) {
    if (!c) return PJB_ERR_ARG;
    GrowPlan P;
    GrowInput in;
    GrowRoom R;
    int rc;
    GrowPacked B;
    if ((rc = grow_plan(c, "pjb_forest_grow", data, n_rows, n_cols, p, out, P))) return rc;
    if ((rc = grow_input(c, data, P, in))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    if ((rc = grow_room(c, P, R))) return rc;
    HIP_TRY(c, hipMemcpyAsync(R.col, in.colmajor.data(), P.C * P.n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.label, in.label.data(), P.n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.sorted, in.sorted.data(), P.C * P.n * 4, hipMemcpyHostToDevice, st));

    ModelState::GrowOut &G = c->model.grow_out;
    G = ModelState::GrowOut();
    G.is_ordered.assign(P.C, 1);
    if (in.label_sum < P.n) G.class_values.push_back(0.0);
    if (in.label_sum > 0) G.class_values.push_back(1.0);
    G.tree_off.push_back(0);
    for (size_t t0 = 0; t0 < P.n_trees; t0 += R.batch) {
        const u32 T = (u32)std::min<size_t>(R.batch, P.n_trees - t0);
        if ((rc = grow_batch(c, P, R, in.label_sum, t0, T))) return rc;
        if ((rc = grow_read(c, P, R, t0, T, B))) return rc;
        grow_append(B, 0, T, in.label_sum, G);
    }
    return grow_view(c, P, G, out);
}

// k-fold cross-validation: see include/portcullis_amd.h and pjb_cv.hip.h.
int pjb_forest_cv(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, const int32_t *fold, int32_t n_folds,
                  double *pred, pjb_grow_result *forests) {
    if (!c) return PJB_ERR_ARG;
    static const char *const who = "pjb_forest_cv";
    GrowPlan P;
    GrowInput in;
    GrowFolds F;
    GrowRoom R;
    GrowPacked B;
    int rc;
    if ((rc = grow_plan(c, who, data, n_rows, n_cols, p, pred, P))) return rc;
    if (!fold) return fail(c, PJB_ERR_ARG, "%s: bad arguments", who);
    if (n_folds < 2 || n_folds > n_rows) return fail(c, PJB_ERR_ARG, "%s: %d folds of %lld rows (2 to the number of rows)", who, n_folds, (long long)n_rows);
    P.n_folds = (size_t)n_folds;
    if (P.trees_all() > ((size_t)1 << 30)) return fail(c, PJB_ERR_ARG, "%s: %d folds of %d trees", who, n_folds, p->n_trees);
    std::vector<u32> held(P.n_folds, 0), held_sum(P.n_folds, 0);
    F.fold.resize(P.n);
    for (size_t r = 0; r < P.n; r++) {
        if (fold[r] < 0 || fold[r] >= n_folds) return fail(c, PJB_ERR_ARG, "%s: row %zu is in fold %d (0 to %d)", who, r, fold[r], n_folds - 1);
        F.fold[r] = (u32)fold[r];
        held[F.fold[r]]++;
    }
    for (size_t f = 0; f < P.n_folds; f++)
        if (!held[f]) return fail(c, PJB_ERR_ARG, "%s: fold %zu holds no row", who, f);
    if ((rc = grow_input(c, data, P, in))) return rc;
    for (size_t r = 0; r < P.n; r++) held_sum[F.fold[r]] += in.label[r];
    F.train_n.resize(P.n_folds);
    F.train_sum.resize(P.n_folds);
    for (size_t f = 0; f < P.n_folds; f++) {
        F.train_n[f] = (u32)P.n - held[f];
        F.train_sum[f] = in.label_sum - held_sum[f];
        if (F.train_sum[f] == 0 || F.train_sum[f] == F.train_n[f])
            return fail(c, PJB_ERR_ARG, "%s: the %u rows fold %zu trains on all have the label %d", who, F.train_n[f], f, F.train_sum[f] ? 1 : 0);
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    if ((rc = grow_room(c, P, R))) return rc;
    HIP_TRY(c, hipMemcpyAsync(R.col, in.colmajor.data(), P.C * P.n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.label, in.label.data(), P.n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.sorted, in.sorted.data(), P.C * P.n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.fold, F.fold.data(), P.n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.fold_n, F.train_n.data(), P.n_folds * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(R.fold_sum, F.train_sum.data(), P.n_folds * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(R.pred, 0, P.n * 16, st));

    std::vector<ModelState::GrowOut> &GG = c->model.cv_out;
    GG.assign(P.n_folds, ModelState::GrowOut());
    for (ModelState::GrowOut &G : GG) {
        G.is_ordered.assign(P.C, 1);
        G.class_values = {0.0, 1.0};
        G.tree_off.push_back(0);
    }
    const size_t all = P.trees_all();
    for (size_t t0 = 0; t0 < all; t0 += R.batch) {
        const u32 T = (u32)std::min<size_t>(R.batch, all - t0);
        if ((rc = grow_batch(c, P, R, 0, t0, T))) return rc;
        LAUNCH(c, "kc_score", kc_score, dim3((unsigned)((P.n + 255) / 256)), dim3(256), R.nd, (u32)P.M, (const double *)R.col, (const u32 *)R.fold, (u32)t0, T,
               (u32)P.n_trees, (u32)P.n, R.pred);
        if ((rc = grow_read(c, P, R, t0, T, B))) return rc;
        for (size_t f = t0 / P.n_trees; f * P.n_trees < t0 + T; f++) { // the folds the batch cuts through
            const size_t ta = std::max(f * P.n_trees, t0) - t0, tb = std::min((f + 1) * P.n_trees, t0 + T) - t0;
            grow_append(B, (u32)ta, (u32)tb, F.train_sum[f], GG[f]);
        }
    }
    HIP_TRY(c, hipMemcpyAsync(pred, R.pred, P.n * 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (forests)
        for (size_t f = 0; f < P.n_folds; f++)
            if ((rc = grow_view(c, P, GG[f], &forests[f]))) return rc;
    return PJB_OK;
}

// Waves the default chunking of pjb_knn aims at: 256 CUs x 4 SIMDs x 4 waves, so that scalar-load latency has other waves to hide behind.
static constexpr size_t KNN_WAVES = 4096;
// A chunk shorter than this spends its time filling the lists (every one of the first rows of a chunk is an insertion).
static constexpr size_t KNN_MIN_CHUNK = 256;
// |value| <= this: 32 squared differences cannot overflow (32 * (2e153)^2 = 1.28e308), so every distance is finite and ordered.
static constexpr double KNN_MAX_ABS = 1e153;
static_assert(KN_LIST == PJB_KNN_MAX_K, "the lists of pjb_knn.hip.h hold PJB_KNN_MAX_K entries");

// KNN::execute (lib/src/knn.cc): see include/portcullis_amd.h and pjb_knn.hip.h.
int pjb_knn(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, int32_t k, uint32_t *nn_out) {
    if (!c) return PJB_ERR_ARG;
    if (!data || !nn_out) return fail(c, PJB_ERR_ARG, "pjb_knn: bad arguments");
    if (n_cols < 1 || n_cols > PJB_KNN_MAX_COLS) return fail(c, PJB_ERR_ARG, "pjb_knn: %d columns (1 to %d)", n_cols, PJB_KNN_MAX_COLS);
    if (n_rows < 1 || n_rows > (1ll << 22)) return fail(c, PJB_ERR_ARG, "pjb_knn: %lld rows (1 to %d)", (long long)n_rows, 1 << 22);
    if (k < 1 || k > PJB_KNN_MAX_K || k > n_rows)
        return fail(c, PJB_ERR_ARG, "pjb_knn: k = %d (1 to %d, and no more than the %lld rows)", k, PJB_KNN_MAX_K, (long long)n_rows);
    const size_t n = (size_t)n_rows, C = (size_t)n_cols;
    const size_t NC = n_cols <= 28 ? 28 : 32; // the compiled widths: the 28 features of self-training, and the limit
    std::vector<double> padded(n * NC, 0.0);
    for (size_t r = 0; r < n; r++)
        for (size_t j = 0; j < C; j++) {
            const double v = data[r * C + j];
            if (!(fabs(v) <= KNN_MAX_ABS)) // (a NaN too)
                return fail(c, PJB_ERR_ARG, "pjb_knn: row %zu, column %zu is %g: not finite, or so large that a distance could overflow", r, j, v);
            padded[r * NC + j] = v;
        }
    size_t chunk = c->model.knn_chunk;
    if (!chunk) {
        const size_t row_waves = (n + 63) / 64;
        const size_t want = (KNN_WAVES + row_waves - 1) / row_waves;
        chunk = std::max(KNN_MIN_CHUNK, (n + want - 1) / want);
    }
    chunk = std::min(chunk, n);
    const size_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks > 65535) return fail(c, PJB_ERR_ARG, "pjb_knn: knn_chunk %zu makes %zu chunks of %zu rows (65535 at most)", chunk, n_chunks, n);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->model.n_data, n * NC * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->model.n_part_d, n_chunks * KN_LIST * n * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->model.n_part_i, n_chunks * KN_LIST * n * sizeof(u32)))) return rc;
    if ((rc = ensure(c, c->model.n_out, n * (size_t)k * sizeof(u32)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->model.n_data.p, padded.data(), n * NC * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)n_chunks);
    if (NC == 28)
        LAUNCH(c, "kn_partial", kn_partial<28>, grid, dim3(64), (const double *)c->model.n_data.p, (u32)n, (u32)chunk, (double *)c->model.n_part_d.p, (u32 *)c->model.n_part_i.p);
    else
        LAUNCH(c, "kn_partial", kn_partial<32>, grid, dim3(64), (const double *)c->model.n_data.p, (u32)n, (u32)chunk, (double *)c->model.n_part_d.p, (u32 *)c->model.n_part_i.p);
    LAUNCH(c, "kn_merge", kn_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), (const double *)c->model.n_part_d.p, (const u32 *)c->model.n_part_i.p, (u32)n,
           (u32)n_chunks, (u32)k, (u32 *)c->model.n_out.p);
    HIP_TRY(c, hipMemcpyAsync(nn_out, c->model.n_out.p, n * (size_t)k * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st)); // (the one wait; `padded` is pageable and lives until here)
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

} // extern "C"
