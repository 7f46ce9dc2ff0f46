// pjb_limits.hip.h -- the limits a `junc` chain is queued with, as pure functions: the first ones (first_limits), what a chain that closed
// itself on an overflow is queued with next (relimit), how many repeats it gets (attempt_budget), a member's share of a group's virtual
// sequence (group_span).  Host code with no context, no HIP call and no globals -- values in, values out -- behind pjb_host.hip.h and
// nothing else: tests/cpp/chain_limits.cc runs it on a machine without a GPU.  Included by pjb_flight.hip.h, which applies the results.
#pragma once

// a member's share of a group's virtual sequence: its bases, the gap that keeps a window from reaching the next member, whole bitmap words
inline int64_t group_span(int32_t ref_len) { return (((int64_t)std::max(ref_len, 1) + GROUP_GAP) + 63) & ~(int64_t)63; }

// what the first limits of a chain follow from: the flight (prepare_flight) and what the context has learnt and been told
struct LimitInputs {
    int64_t n_reads;      // of all members
    int n_members;
    int64_t vlen;         // the sequence the chain works on: the target, or the group's virtual sequence
    bool genomes_ok;      // every member with reads has its genome
    u32 junc_seen;        // the context: most junctions a chain has had (a group's: per member)
    int lbits_seen;       // the context: bits of the longest intron met
    double junc_per_read; // the context: most junctions per read a chain has had
    u32 sort_floor;       // pjb_set_option
    bool dense_ids, run_sort;
};

// Pairs: a share of the reads (a chain with more N operations than that is repeated once with the exact count).  Junctions: a share of
// the pair limit, at least twice what a chain of this context has had.  Key: coordinates of the (virtual) sequence and the longest
// intron seen by this context so far.
inline ContigLimits first_limits(const LimitInputs &in) {
    ContigLimits lim;
    const u64 guess = std::min<u64>(0xffffff00ull, (u64)in.n_reads * 5 / 8 + 4096);
    lim.pair_limit = (u32)std::max<u64>(guess, 4096);
    lim.junc_limit = std::max<u32>(std::max<u32>(lim.pair_limit / 32, 4096), 2 * in.junc_seen * (u32)(in.n_members > 1 ? 2 : 1));
    if (!in.genomes_ok) lim.pair_limit = 0; // without a target's genome only the counting stage may run: any pair then shows up as an overflow
    lim.kf.raw = 0;
    lim.kf.lbits = std::max(1, in.lbits_seen);
    lim.kf.total_bits = lim.kf.lbits + std::max(1, bits_of((uint64_t)std::max<int64_t>(in.vlen, 1)));
    lim.dense = in.dense_ids;
    lim.run_sort = in.run_sort;
    // (twice what a chain of this context's targets has had, per member; a chain with more is repeated with digits for junc_limit)
    // (junctions per read: chains of one file have about the same, whatever their targets' number and size)
    lim.sort_limit = in.junc_per_read > 0 ? std::min<u32>(lim.junc_limit, std::max<u32>(in.sort_floor, (u32)std::min<double>(4.0e9, 2.0 * in.junc_per_read * (double)in.n_reads + 64.0))) : 0u;
    return lim;
}

// what becomes of a chain that closed itself on an overflow
struct Relimit {
    enum What {
        REPEAT,        // queue it again with `lim` as it is now
        APART,         // a group with alignments outside a member's own sequence: its members one by one (lim is not used again)
        TOO_MANY_PAIRS // more than 2^32 spliced pairs: an error
    } what;
    bool run_sort_off; // with REPEAT: the radix route for this chain, those taken back behind it and those to come (the caller's: run_sort of
                       // the context and of every flight's limits, these included)
};
inline const char *too_many_pairs_text(bool group) {
    return group ? "finish_group: more than 2^32 spliced pairs in one group: finish its targets in smaller groups"
                 : "finish: more than 2^32 spliced pairs on one target are not supported";
}

// A limit was too small: the control block says by how much.  ref_len: the sequence the chain works on (a group's: the virtual one).
inline Relimit relimit(ContigLimits &lim, const ContigStats &cs, int32_t ref_len, bool group) {
    if (cs.overflow & OVF_PAIRS) {
        if (cs.n_pairs >= 0xfffffff0ull) return Relimit{Relimit::TOO_MANY_PAIRS, false};
        lim.pair_limit = (u32)cs.n_pairs + 64;
        lim.junc_limit = std::max<u32>(lim.junc_limit, lim.pair_limit / 8);
    }
    if (cs.overflow & OVF_KEYFMT) {
        const bool weird = cs.min_pos < 0 || cs.max_end > ref_len || cs.max_end < 0;
        if (weird && group) return Relimit{Relimit::APART, false}; // (k1_count reports INT32_MAX for a member whose alignments leave it)
        if (weird) {
            lim.kf.raw = 1;
            lim.kf.lbits = 32;
            lim.kf.total_bits = 64;
            lim.dense = false; // the bitmap of intron starts needs coordinates inside the contig
        } else {
            lim.kf.lbits = std::max(1, bits_of((uint64_t)cs.max_nlen));
            lim.kf.total_bits = lim.kf.lbits + std::max(1, bits_of((uint64_t)std::max(ref_len, 1)));
        }
    }
    const bool sort_only = (cs.overflow & OVF_JUNC) && lim.sort_limit && cs.n_junc <= lim.junc_limit; // (the buffers were large enough)
    if (cs.overflow & OVF_JUNC) lim.sort_limit = 0;
    if ((cs.overflow & OVF_JUNC) && !sort_only) lim.junc_limit = std::max<u32>(cs.n_junc + 64, (cs.overflow & OVF_DENSE) || !lim.dense ? 0u : lim.junc_limit * 4);
    // tiles whose ids do not lie in a window (an unsorted or pathological file), or more runs than the list holds: the radix route
    const bool run_sort_off = (cs.overflow & OVF_RUNS) != 0;
    if (cs.overflow & OVF_DENSE) lim.dense = false; // a donor with more alternative acceptors than K2d keeps: sort the full keys
    if (cs.overflow & OVF_LISTS) lim.list_cap = std::max(gen_list_cap(lim.pair_limit), (cs.list_need + cs.list_need / 4 + 511u) & ~255u); // (k1_generic's entries depend on the appends' order: some slack)
    return Relimit{Relimit::REPEAT, run_sort_off};
}

// May a chain that closed itself with `overflow` be repeated?  A repeat for the read lists' room alone (exactly OVF_LISTS) has a budget of
// its own, three: it must not use up the attempts the other limits may need.  Any other repeat -- and a fourth for the lists alone --
// draws on `attempt`: three, and false at the fourth ("limits did not settle").  Both counters are the flight's and survive a take-back.
inline bool attempt_budget(u32 overflow, int &attempt, int &list_attempt) {
    if (overflow == OVF_LISTS && list_attempt < 3) {
        list_attempt++;
        return true;
    }
    if (attempt >= 3) return false;
    attempt++;
    return true;
}
