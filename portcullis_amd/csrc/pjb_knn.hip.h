// pjb_knn.hip.h -- brute-force K nearest neighbours in f64, the search under SMOTE and ENN of self-training (pjb_knn).
//
// KNN::doSlice (lib/src/knn.cc:46-99) restated: for every test row the distance to every base row is
//   s = sum over the columns, ascending, of (base[c] - test[c])^2      (subtract, multiply and add each round on their own)
// and the answer is the k smallest under the total order (s, base index): the reference walks the base rows in ascending order and
// puts a candidate behind the entries of equal distance.  A row's own index takes part (distance 0).
//
// kn_partial: one lane per test row, the row in registers (padded with zero columns: (0 - 0)^2 adds nothing).  The base rows of a
// chunk are walked by the whole wave together, so their addresses are wave-uniform and they come through the scalar cache.  Each
// lane keeps the KN_LIST best (s, index) of its chunk in registers -- every index into the list is a compile-time constant -- and
// writes them out.  The grid's second dimension runs over the chunks of the base range: `rows / 64` waves alone do not fill the chip.
// kn_merge: one lane per test row folds the chunks' lists, chunk after chunk, into the final one.  Chunks ascend in base index and
// each list is in (s, index) order, so "strictly smaller goes in front" is the total order again, and the result is the same for
// every chunk size.
// All loops are bounded by the chunk length or the chunk count; no kernel waits for another.
#pragma once
#include "pjb_device.hip.h"

constexpr int KN_LIST = 8; // PJB_KNN_MAX_K: the length of every list, whatever k the caller reads from it
constexpr u32 KN_NONE = 0xffffffffu;

// (s, idx) into the list d / ix, behind every entry with a distance <= s.  The caller's candidates arrive in ascending index order.
__device__ __forceinline__ void kn_insert(double (&d)[KN_LIST], u32 (&ix)[KN_LIST], double s, u32 idx) {
#pragma unroll
    for (int p = KN_LIST - 1; p > 0; p--) {
        const bool shift = s < d[p - 1]; // the entry in front moves back one place
        const bool here = !shift && s < d[p];
        d[p] = shift ? d[p - 1] : (here ? s : d[p]);
        ix[p] = shift ? ix[p - 1] : (here ? idx : ix[p]);
    }
    const bool first = s < d[0];
    d[0] = first ? s : d[0];
    ix[0] = first ? idx : ix[0];
}

// Lists are stored [chunk][place][row]: the lanes of a wave write and read neighbouring rows.
__device__ __forceinline__ size_t kn_at(u32 chunk, int place, u32 row, u32 n_rows) { return ((size_t)chunk * KN_LIST + (size_t)place) * n_rows + row; }

// data: n_rows x NC, row-major, the columns past the caller's filled with zeros.  grid (ceil(n_rows / 64), n_chunks), block 64.
template <int NC>
__global__ __launch_bounds__(64) void kn_partial(const double *__restrict__ data, u32 n_rows, u32 chunk, double *__restrict__ part_d,
                                                 u32 *__restrict__ part_i) {
#pragma clang fp contract(off)
    const u32 row = blockIdx.x * 64 + threadIdx.x;
    const u32 mine = row < n_rows ? row : n_rows - 1; // (lanes past the end walk the last row and write nothing)
    double t[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) t[c] = data[(size_t)mine * NC + c];
    double d[KN_LIST];
    u32 ix[KN_LIST];
#pragma unroll
    for (int p = 0; p < KN_LIST; p++) {
        d[p] = __builtin_inf();
        ix[p] = KN_NONE;
    }
    const u32 b0 = blockIdx.y * chunk;
    const u32 b1 = b0 + chunk < n_rows ? b0 + chunk : n_rows; // (b0 < n_rows: the host sizes the grid by ceil(n_rows / chunk))
    for (u32 b = b0; b < b1; b++) {
        const double *__restrict__ base = data + (size_t)b * NC; // wave-uniform
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const double diff = base[c] - t[c];
            const double sq = diff * diff;
            s = s + sq;
        }
        if (s < d[KN_LIST - 1]) kn_insert(d, ix, s, b);
    }
    if (row < n_rows) {
#pragma unroll
        for (int p = 0; p < KN_LIST; p++) {
            part_d[kn_at(blockIdx.y, p, row, n_rows)] = d[p];
            part_i[kn_at(blockIdx.y, p, row, n_rows)] = ix[p];
        }
    }
}

// nn_out: n_rows x k.  Every distance is finite and k <= n_rows (the host checked both), so the first k places are all taken.
__global__ __launch_bounds__(256) void kn_merge(const double *__restrict__ part_d, const u32 *__restrict__ part_i, u32 n_rows, u32 n_chunks, u32 k,
                                                u32 *__restrict__ nn_out) {
    const u32 row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    double d[KN_LIST];
    u32 ix[KN_LIST];
#pragma unroll
    for (int p = 0; p < KN_LIST; p++) {
        d[p] = __builtin_inf();
        ix[p] = KN_NONE;
    }
    for (u32 ch = 0; ch < n_chunks; ch++) {
#pragma unroll
        for (int p = 0; p < KN_LIST; p++) {
            const double s = part_d[kn_at(ch, p, row, n_rows)];
            const u32 idx = part_i[kn_at(ch, p, row, n_rows)];
            if (s < d[KN_LIST - 1]) kn_insert(d, ix, s, idx);
        }
    }
#pragma unroll
    for (int p = 0; p < KN_LIST; p++)
        if ((u32)p < k) nn_out[(size_t)row * k + p] = ix[p];
}
