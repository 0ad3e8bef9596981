// group_route.h -- the plan of one call of the multi-GPU group driver (plspm_group.cpp plspm_group_bootstrap): how a call of B replicates is cut into sub-batches, how
// each sub-batch is sharded over the ranks, and where every shard lies in the send and receive buffers -- i.e. how many collectives every rank of a job issues and of
// what sizes.  Pure functions of rank-INVARIANT inputs only (B, the rank count, the record pitch, the group's options, the alignment the ranks agreed on): a rank that
// planned differently would hang the job, not miscompute.  plspm_bootstrap() cuts its PCIe sub-batches with the same chunk_plan.  Free of the HIP runtime and of RCCL:
// the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace plspm {

static constexpr int kBootChunksMax = 8;      // sub-batches of one call at most ("chunks", "boot_chunks")

// The contiguous shard of rank `rank` of B units over nranks ranks: the first B % nranks ranks hold one unit more.
inline void shard_of(int64_t B, int nranks, int rank, int64_t* first, int64_t* count) {
    const int64_t base = B / nranks, extra = B % nranks;
    *first = rank * base + std::min<int64_t>(rank, extra);
    *count = base + (rank < extra ? 1 : 0);
}

// plspm_detail_chunk_plan (model.h): the parts of B units in a geometric progression, every part but the last a multiple of `align`.
inline int chunk_plan(int64_t B, int64_t bytes_per_unit, int chunks_opt, int ratio_pct, int64_t* parts, int64_t align) {
    parts[0] = B;
    if (B < 1) return 1;
    if (align < 1) align = 64;
    int n = chunks_opt;
    if (n <= 0) n = (B * bytes_per_unit < ((int64_t)2 << 20)) ? 1 : 3;           // automatic: nothing worth hiding below 2 MiB of results
    n = std::min(n, kBootChunksMax);
    // no part below 512 units (a sub-batch's fixed costs: three launches + an event) -- nor below one alignment unit (a round of the machine)
    n = (int)std::min<int64_t>(n, std::max<int64_t>(1, (B + align / 2) / std::max<int64_t>(512, align)));
    if (n <= 1) return 1;
    const double q = std::min(100, std::max(10, ratio_pct)) / 100.0;
    double wsum = 0.0, w = 1.0;
    for (int k = 0; k < n; ++k, w *= q) wsum += w;
    int64_t left = B;
    w = 1.0;
    int k = 0;
    for (; k < n - 1; ++k, w *= q) {
        int64_t c = (int64_t)((double)B * w / wsum + 0.5);
        c = std::max<int64_t>(align, (c + align / 2) / align * align);
        if (left - c < std::min<int64_t>(align, 64)) break;                        // the remainder would be no part of its own
        parts[k] = c; left -= c;
    }
    parts[k] = left;
    return k + 1;
}

// plspm_group_set_option "chunks" (0: automatic), "chunk_ratio" (per cent), "chunk_align" (0: whole rounds of the device -- the `units` the ranks agreed on;
// n > 0: multiples of n replicates per rank)
struct GroupOptions { int chunks, ratio, align; };

// Sub-batch k = the global replicate ids [first, first + B), sharded over the ranks like a call of its own: `cap` records per rank (ceil(B / nranks), the ragged
// shards padded), starting at record `off` of a rank's send buffer and at record nranks * off of the receive buffer.
struct GroupSub { int64_t first, B, cap, off; };
struct GroupPlan {
    int64_t B;                   // replicates of the call
    int nranks, RS;              // ranks of the job; doubles per record (plspm_row_stride)
    int K;                       // sub-batches: one collective each
    GroupSub sub[kBootChunksMax];
    int64_t cap;                 // records per rank, all sub-batches
    size_t send_bytes, recv_bytes;
};
struct GroupShard { int64_t first, count; };             // within its sub-batch
struct GroupSegment { int64_t rec0, first, count; };     // first record in the receive buffer; global id of its first replicate within the call; replicates

// nothing_to_hide: one rank, or ranks that share a device -- one copy launch of microseconds: nothing travels, so there is one sub-batch unless sub-batches are asked
// for by number.  The caller computes it once for the two functions below, which must agree on every rank.
// The plan reads the alignment the ranks agree on (one blocking all-reduce before the first call that does).
inline bool group_consults_units(const GroupOptions& o, bool nothing_to_hide) { return !(nothing_to_hide && o.chunks <= 0) && o.chunks != 1 && o.align <= 0; }

inline GroupPlan group_plan(int64_t B, int nranks, int RS, const GroupOptions& o, int64_t units, bool nothing_to_hide) {
    GroupPlan p{};
    p.B = B; p.nranks = nranks; p.RS = RS;
    const int64_t per_rank = (B + nranks - 1) / nranks;
    int64_t parts[kBootChunksMax];
    const int K = (nothing_to_hide && o.chunks <= 0) ? 1 : chunk_plan(per_rank, (int64_t)RS * (int64_t)sizeof(double), o.chunks, o.ratio, parts, o.align > 0 ? o.align : units);
    int64_t at = 0;
    for (int k = 0; k < K && at < B; ++k) {
        const int64_t take = (k == K - 1) ? B - at : std::min<int64_t>(B - at, parts[k] * nranks);
        p.sub[p.K].first = at; p.sub[p.K].B = take; at += take; ++p.K;
    }
    if (at < B) p.sub[p.K - 1].B += B - at;
    for (int k = 0; k < p.K; ++k) { p.sub[k].cap = (p.sub[k].B + nranks - 1) / nranks; p.sub[k].off = p.cap; p.cap += p.sub[k].cap; }
    p.send_bytes = (size_t)p.cap * RS * sizeof(double);
    p.recv_bytes = p.send_bytes * nranks;
    return p;
}

inline GroupShard group_shard(const GroupPlan& p, int k, int rank) {
    GroupShard s{};
    shard_of(p.sub[k].B, p.nranks, rank, &s.first, &s.count);
    return s;
}
// A full shard fills its `cap` records: nothing to pad behind it (the driver lets its last kernel signal `computed` itself).
inline bool group_shard_full(const GroupPlan& p, int k, int64_t count) { return count == p.sub[k].cap && count > 0; }
// Segment (sub-batch k, rank) of the gathered records.
inline GroupSegment group_segment(const GroupPlan& p, int k, int rank) {
    const GroupShard s = group_shard(p, k, rank);
    return GroupSegment{p.nranks * p.sub[k].off + (int64_t)rank * p.sub[k].cap, p.sub[k].first + s.first, s.count};
}

}  // namespace plspm
