// The plan of one mutual-information launch of the Carrington header-shift sweep (coreg_sweep_carrington with
// COREG_METHOD_MUTUAL_INFORMATION): the groups of lag slots, the number of chunks the launch's tile list is
// cut in per group, the LDS and global histogram bytes, and every refusal with its code and message.  Plain C++ with no HIP
// dependency: included by kernels_sweep_mi.hpp (the constants and the chunk walk the kernel shares with the host) and used by
// host_sweep_mi.hpp, parts of libcoreg_hip.so's one translation unit; tests/native/sweep_mi_rules.cpp walks it on the host
// under sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/coreg_hip.h"

#if defined(__HIPCC__)
#define COREG_MI_HD __host__ __device__ __forceinline__
#else
#define COREG_MI_HD inline
#endif

namespace coreg {

constexpr int kMiG = 16;            // lag slots per work item: the sixteen histograms one point's sixteen lanes add to
constexpr int kMiThreads = 256;     // threads of a work item: kMiThreads / kMiG points per step
constexpr int kMiMaxEdges = 31;     // edges per list at most (csrc/pixels_bins.hpp: kPixMaxEdges), 32 bins
constexpr int kMiMaxChunks = 64;    // chunks of the tile list per slot group at most (option "mi_chunks")
constexpr int kMiFillItems = 1024;  // work items a launch of few slot groups is cut in, about (see sweep_mi_chunks)
constexpr long long kMiMaxHistBytes = 2147483647ll;  // the global histograms of one launch, uint32 [slot][cell]

// One group of lag slots: slots [first, first + count) of the launch; live: one of them has an output index (the others, and
// every slot of a group that is not live, are padding: NaN parameters, nothing to write)
struct MiGroup {
    int first, count;
    bool live;
};

// The chunk walk: work item (group, chunk) of a launch with n_chunks chunks takes the entries mi_chunk_first, + mi_chunk_step,
// ... of the launch's tile list -- each entry belongs to exactly one chunk.  (The integer counters make any partition give
// the same histograms; this one spreads neighbouring tiles over the chunks, as k_refine's does.)
COREG_MI_HD int mi_chunk_first(int chunk, int n_chunks) {
    (void)n_chunks;
    return chunk;
}
COREG_MI_HD int mi_chunk_step(int n_chunks) { return n_chunks; }

// bytes of the LDS histograms of a work item, uint32 [cell][kMiG], and of the global ones of a launch, uint32 [slot][cell]
inline size_t sweep_mi_lds_bytes(int n_edges_small, int n_edges_large) {
    return (size_t)kMiG * (size_t)(n_edges_small + 1) * (size_t)(n_edges_large + 1) * sizeof(uint32_t);
}
inline long long sweep_mi_hist_bytes(long long n_slots, int n_edges_small, int n_edges_large) {
    return n_slots * (long long)(n_edges_small + 1) * (long long)(n_edges_large + 1) * (long long)sizeof(uint32_t);
}

// Chunks per slot group when the caller leaves the choice: enough work items to fill the device when the live groups are
// few, 1 when they are many.  A HEURISTIC WITHOUT A MEASURED BASIS: kMiFillItems is four work items for each of the 256
// compute units, nobody has timed another value.  More chunks cost one more flush of the non-zero cells each.
inline int sweep_mi_chunks(int n_live_groups) {
    if (n_live_groups < 1) return 1;
    return std::max(1, std::min(kMiMaxChunks, kMiFillItems / n_live_groups));
}

// What a sweep call must have before anything is planned
struct MiHave {
    long long shard_world;             // option "shard_world"
    int n_edges_small, n_edges_large;  // coreg_sweep_set_bins; 0: not set
};

struct MiRequest {
    MiHave have;
    long long n_slots;        // slots of the launch, padding included: a multiple of kMiG
    const long long* outidx;  // [n_slots] output index of every slot, < 0: padding
    long long opt_chunks;     // option "mi_chunks"; 0: sweep_mi_chunks
};

// A refusal (code != COREG_OK, msg) or everything the launch needs
struct MiPlan {
    int code = COREG_OK;
    const char* msg = nullptr;
    MiPlan() {}
    MiPlan(int refusal, const char* why) : code(refusal), msg(why) {}
    std::vector<MiGroup> groups;  // every slot of the launch in exactly one, in slot order
    int n_live = 0;               // groups that are live
    int chunks = 1;               // per group
    int na = 0, nb = 0;           // bins of the image to align (rows), of the reference (columns)
    size_t lds_bytes = 0;
    long long hist_bytes = 0;
    unsigned grid = 0;            // work items: groups x chunks (a work item of a group that is not live leaves at once)
};

// the refusals that do not depend on a launch, in the order a caller sees them
inline MiPlan sweep_mi_admit(const MiHave& have) {
    if (have.shard_world > 1)
        return MiPlan(COREG_ENOTIMPL, "mutual information: a grid-shared sweep (shard_world > 1) is not implemented (six sums "
                                      "can be all-reduced, per-rank histograms are not)");
    if (have.n_edges_small < 1 || have.n_edges_large < 1)
        return MiPlan(COREG_ESTATE, "mutual information needs its bins (coreg_sweep_set_bins)");
    if (have.n_edges_small > kMiMaxEdges || have.n_edges_large > kMiMaxEdges)
        return MiPlan(COREG_EINVAL, "mutual information: more than 31 edges in a list");
    return MiPlan();
}

inline MiPlan sweep_mi_plan(const MiRequest& rq) {
    MiPlan p = sweep_mi_admit(rq.have);
    if (p.code != COREG_OK) return p;
    if (rq.opt_chunks < 0 || rq.opt_chunks > kMiMaxChunks) return MiPlan(COREG_EINVAL, "mi_chunks must be in [0, 64]");
    if (!rq.outidx || rq.n_slots < kMiG || rq.n_slots % kMiG != 0)
        return MiPlan(COREG_EINVAL, "mutual information: a launch needs a positive multiple of 16 lag slots");
    p.hist_bytes = sweep_mi_hist_bytes(rq.n_slots, rq.have.n_edges_small, rq.have.n_edges_large);
    if (p.hist_bytes > kMiMaxHistBytes || rq.n_slots > kMiMaxHistBytes)
        return MiPlan(COREG_EINVAL, "mutual information: work space too large (lag slots x bins of one launch)");
    p.na = rq.have.n_edges_small + 1;
    p.nb = rq.have.n_edges_large + 1;
    p.lds_bytes = sweep_mi_lds_bytes(rq.have.n_edges_small, rq.have.n_edges_large);
    for (long long first = 0; first < rq.n_slots; first += kMiG) {
        MiGroup g = {(int)first, kMiG, false};
        for (int k = 0; k < kMiG; ++k) g.live = g.live || rq.outidx[first + k] >= 0;
        p.n_live += g.live ? 1 : 0;
        p.groups.push_back(g);
    }
    p.chunks = rq.opt_chunks > 0 ? (int)rq.opt_chunks : sweep_mi_chunks(p.n_live);
    if ((long long)p.groups.size() * p.chunks > kMiMaxHistBytes)
        return MiPlan(COREG_EINVAL, "mutual information: too many work items");
    p.grid = (unsigned)(p.groups.size() * (size_t)p.chunks);
    return p;
}

}  // namespace coreg
