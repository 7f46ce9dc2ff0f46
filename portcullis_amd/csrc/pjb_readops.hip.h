// pjb_readops.hip.h -- shared by k1_emit, k1_generic and k4b_generic: a spliced read's CIGAR operations as the walks see them.
// The operations behind an LDS column (OpsViewT, fetch_ops8), the chain's batches in LDS (BatchTab) and the cursor over a read's N
// operations (NCursor).  No kernel; whoever walks reads includes it.
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// CIGAR ops of one alignment: the first OPS_LDS ops are staged in LDS (one column per thread), the
// rest (long reads) are read from global memory
constexpr int OPS_LDS = 8;
template <int STRIDE, int NLDS>
struct OpsViewT {
    const uint32_t *g;
    const u32 *lds; // &s_ops[0][column]: NLDS rows of STRIDE columns
    __device__ __forceinline__ u32 operator[](u32 k) const { return k < (u32)NLDS ? lds[k * STRIDE] : gload(g + k); }
};
typedef OpsViewT<256, OPS_LDS> OpsView;
// The first OPS_LDS operations of a read whose operations start at word c0 of its batch's `cig_words` words: two 16-byte loads (a lane's
// eight words are neighbours: eight word gathers cost the addresser eight times as much).  The batch's last operations are read from
// eight words before its end and shifted -- the loads never leave the array --; what lies behind the read's last operation is the next
// read's, the caller masks it.
__device__ __forceinline__ void fetch_ops8(const PJB_GLOBAL u32 *cigar, u32 c0, u32 cig_words, u32 (&w)[OPS_LDS]) {
    static_assert(OPS_LDS == 8, "two 16-byte loads");
    if (cig_words >= (u32)OPS_LDS) {
        const u32 c0c = c0 + (u32)OPS_LDS <= cig_words ? c0 : cig_words - (u32)OPS_LDS;
        const Words4 lo4 = gload_as<Words4>(cigar + c0c), hi4 = gload_as<Words4>(cigar + c0c + 4);
        w[0] = lo4.x, w[1] = lo4.y, w[2] = lo4.z, w[3] = lo4.w, w[4] = hi4.x, w[5] = hi4.y, w[6] = hi4.z, w[7] = hi4.w;
        if (c0c != c0) { // (shifted: at most seven words)
            const u32 sh = c0 - c0c;
#pragma unroll
            for (int q = 0; q < OPS_LDS; q++) {
                u32 v = 0;
#pragma unroll
                for (int j = q; j < OPS_LDS; j++) v = (u32)(j - q) == sh ? w[j] : v;
                w[q] = v;
            }
        }
    } else { // (a batch of fewer than eight operations: word by word, guarded)
#pragma unroll
        for (int q = 0; q < OPS_LDS; q++) w[q] = c0 + (u32)q < cig_words ? cigar[c0 + (u32)q] : 0u;
    }
}
// What k1_generic and k4b_generic keep of the chain's batches in LDS, filled once per block (256 threads): a read's batch is found from
// its tile without a load, and the ends of the batch's arrays -- nothing reads past them -- are at hand.  A chain of more batches than
// the table holds searches the descriptors in device memory.
constexpr int GEN_MAXB = 256;
struct BatchTab {
    u32 tbase[GEN_MAXB], seqw[GEN_MAXB], cigw[GEN_MAXB]; // the batch's first tile; words of packed bases / of operations in it
    __device__ __forceinline__ void fill(const DevBatch *batches, int n_batches) { // (the caller's barrier follows)
        if ((int)threadIdx.x < n_batches && threadIdx.x < (u32)GEN_MAXB) {
            const PJB_GLOBAL DevBatch *d = as_global(batches + threadIdx.x);
            tbase[threadIdx.x] = d->tile_base;
            seqw[threadIdx.x] = as_global(d->seq_off)[d->n];
            cigw[threadIdx.x] = as_global(d->cig_off)[d->n];
        }
    }
    __device__ __forceinline__ int find(const DevBatch *batches, int n_batches, u32 tile) const { // the last batch with tile_base <= tile
        int lo = 0, hi = n_batches - 1;
        if (n_batches <= GEN_MAXB) {
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (tbase[mid] <= tile) lo = mid;
                else hi = mid - 1;
            }
        } else {
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (gload(&batches[mid].tile_base) <= tile) lo = mid;
                else hi = mid - 1;
            }
        }
        return lo;
    }
    __device__ __forceinline__ u32 seq_words(const DevBatch &b, int bi) const { return bi < GEN_MAXB ? seqw[bi] : gload(b.seq_off + b.n); }
    __device__ __forceinline__ u32 cig_words(const DevBatch &b, int bi) const { return bi < GEN_MAXB ? cigw[bi] : gload(b.cig_off + b.n); }
};

struct NCursor { // walks the N ops of one CIGAR yielding the unclamped position after each N
    u32 i;
    int32_t acc;
    bool has;
    int32_t peek;
};
template <typename Ops>
__device__ __forceinline__ void ncursor_advance(NCursor &c, const Ops cig, u32 n) {
    c.has = false;
    while (c.i < n) {
        u32 op = cig[c.i++];
        u32 ty = op & 15u;
        if (op_consumes_ref(ty)) c.acc += (int32_t)(op >> 4);
        if (ty == OP_N) {
            c.has = true;
            c.peek = c.acc;
            return;
        }
    }
}

} // namespace pjb
