// The planner of the mutual-information launches of the Carrington sweep (csrc/sweep_mi_plan.hpp) on the host, under
// sanitizers.  What is checked is stated here on its own, not taken from the planner:
//   * groups: for launches of 16 to 1024 slots with seven padding patterns every slot lies in exactly one group, the groups
//     are in slot order with 16 slots each, a group is live exactly when one of its slots has an output index, and n_live
//     counts them;
//   * chunks: for 1..40 tiles and 1..7 chunks the walks mi_chunk_first / mi_chunk_step of the chunks visit every entry of
//     the tile list exactly once;
//   * bytes: for all 31 x 31 pairs of edge counts the LDS bytes are the 16 x (a + 1) x (b + 1) counters counted one by one,
//     the histogram bytes that times the slots / 16, and no launch asks for more LDS than 64 KiB;
//   * the chunk count left to the planner is within [1, 64], is 1 from 1024 live groups on and fills at least half of
//     kMiFillItems below; a forced count is taken as it is; grid = groups x chunks;
//   * refusals: every check with its code and message, the requests either side of each limit, and the order (a grid share
//     before the missing bins before the rest).
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../euispice_coreg_amd/csrc/sweep_mi_plan.hpp"

using namespace coreg;

namespace {
int n_bad = 0, n_checked = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        ++n_checked;                           \
        if (!(cond)) {                         \
            ++n_bad;                           \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
        }                                      \
    } while (0)

MiRequest request(const std::vector<long long>& outidx, int ns = 7, int nl = 15, long long chunks = 0, long long world = 1) {
    return MiRequest{MiHave{world, ns, nl}, (long long)outidx.size(), outidx.data(), chunks};
}

// ---- groups ---------------------------------------------------------------------------------------------------------
std::vector<long long> pattern(int n_slots, int kind) {
    std::vector<long long> o((size_t)n_slots);
    for (int s = 0; s < n_slots; ++s) {
        bool live = true;
        switch (kind) {
            case 0: live = true; break;                   // no padding
            case 1: live = s < n_slots - 5; break;        // a ragged end
            case 2: live = s % 16 == 15; break;           // one live slot at the end of every group
            case 3: live = (s / 16) % 2 == 0; break;      // every other group padding only
            case 4: live = s == n_slots / 2; break;       // one live slot in all
            case 5: live = false; break;                  // padding only
            default: live = (s * 7 + 3) % 5 != 0; break;  // scattered
        }
        o[(size_t)s] = live ? 1000 + s : -1;
    }
    return o;
}

void check_groups() {
    for (int n_slots = 16; n_slots <= 1024; n_slots += (n_slots < 64 ? 16 : 240)) {
        for (int kind = 0; kind < 7; ++kind) {
            const std::vector<long long> o = pattern(n_slots, kind);
            const MiPlan p = sweep_mi_plan(request(o));
            CHECK(p.code == COREG_OK, "groups %d/%d: refused (%s)", n_slots, kind, p.msg ? p.msg : "");
            if (p.code != COREG_OK) continue;
            std::vector<int> seen((size_t)n_slots, 0);
            int next = 0, live_groups = 0;
            for (size_t k = 0; k < p.groups.size(); ++k) {
                const MiGroup& g = p.groups[k];
                CHECK(g.first == next && g.count == 16, "groups %d/%d: group %zu is [%d, +%d), expected [%d, +16)", n_slots, kind,
                      k, g.first, g.count, next);
                if (g.first < 0 || g.count < 0 || g.first + g.count > n_slots) break;
                bool any = false;
                for (int s = g.first; s < g.first + g.count; ++s) {
                    ++seen[(size_t)s];
                    any = any || o[(size_t)s] >= 0;
                }
                CHECK(g.live == any, "groups %d/%d: group %zu live = %d, its slots say %d", n_slots, kind, k, (int)g.live, (int)any);
                live_groups += any ? 1 : 0;
                next += g.count;
            }
            for (int s = 0; s < n_slots; ++s) CHECK(seen[(size_t)s] == 1, "groups %d/%d: slot %d in %d groups", n_slots, kind, s, seen[(size_t)s]);
            CHECK(p.n_live == live_groups, "groups %d/%d: n_live %d, counted %d", n_slots, kind, p.n_live, live_groups);
            CHECK(p.grid == (unsigned)(p.groups.size() * (size_t)p.chunks), "groups %d/%d: grid %u", n_slots, kind, p.grid);
            CHECK(p.chunks >= 1 && p.chunks <= 64, "groups %d/%d: %d chunks", n_slots, kind, p.chunks);
        }
    }
}

// ---- chunks ---------------------------------------------------------------------------------------------------------
void check_chunks() {
    for (int n_tiles = 1; n_tiles <= 40; ++n_tiles)
        for (int n_chunks = 1; n_chunks <= 7; ++n_chunks) {
            std::vector<int> seen((size_t)n_tiles, 0);
            for (int c = 0; c < n_chunks; ++c) {
                CHECK(mi_chunk_step(n_chunks) >= 1, "chunks: step %d", mi_chunk_step(n_chunks));
                if (mi_chunk_step(n_chunks) < 1) return;
                for (int tl = mi_chunk_first(c, n_chunks); tl < n_tiles; tl += mi_chunk_step(n_chunks)) {
                    CHECK(tl >= 0, "chunks: entry %d", tl);
                    if (tl >= 0) ++seen[(size_t)tl];
                }
            }
            for (int t = 0; t < n_tiles; ++t)
                CHECK(seen[(size_t)t] == 1, "chunks: %d tiles, %d chunks: entry %d visited %d times", n_tiles, n_chunks, t, seen[(size_t)t]);
        }
    // the planner's own count
    for (int live = 0; live <= 5000; live += (live < 70 ? 1 : 97)) {
        const int c = sweep_mi_chunks(live);
        CHECK(c >= 1 && c <= kMiMaxChunks, "chunks: %d live groups give %d chunks", live, c);
        if (live >= kMiFillItems) CHECK(c == 1, "chunks: %d live groups give %d chunks", live, c);
        if (live >= 1 && live * kMiMaxChunks >= kMiFillItems && live < kMiFillItems)
            CHECK((long long)live * c > kMiFillItems / 2 && (long long)live * c <= kMiFillItems, "chunks: %d x %d work items", live, c);
        if (live >= 1 && live * kMiMaxChunks < kMiFillItems) CHECK(c == kMiMaxChunks, "chunks: %d live groups give %d chunks", live, c);
    }
    const std::vector<long long> o = pattern(64, 0);
    for (int forced = 1; forced <= 64; forced += 9) {
        const MiPlan p = sweep_mi_plan(request(o, 7, 15, forced));
        CHECK(p.code == COREG_OK && p.chunks == forced && p.grid == 4u * (unsigned)forced, "chunks: forced %d gives %d", forced, p.chunks);
    }
    CHECK(sweep_mi_plan(request(o)).chunks == sweep_mi_chunks(4), "chunks: the planner's choice is sweep_mi_chunks");
}

// ---- bytes ----------------------------------------------------------------------------------------------------------
void check_bytes() {
    const std::vector<long long> o = pattern(48, 1);
    for (int a = 1; a <= 31; ++a)
        for (int b = 1; b <= 31; ++b) {
            size_t counters = 0;
            for (int s = 0; s < 16; ++s)
                for (int i = 0; i <= a; ++i)
                    for (int j = 0; j <= b; ++j) ++counters;
            const MiPlan p = sweep_mi_plan(request(o, a, b));
            CHECK(p.code == COREG_OK, "bytes %d x %d: refused", a, b);
            CHECK(p.lds_bytes == 4 * counters && sweep_mi_lds_bytes(a, b) == 4 * counters, "bytes %d x %d: LDS %zu, counted %zu", a, b,
                  p.lds_bytes, 4 * counters);
            CHECK(p.hist_bytes == (long long)(4 * counters * 3) && sweep_mi_hist_bytes(48, a, b) == p.hist_bytes,
                  "bytes %d x %d: histograms %lld, counted %zu", a, b, p.hist_bytes, 4 * counters * 3);
            CHECK(p.lds_bytes <= 64 * 1024, "bytes %d x %d: %zu bytes of LDS", a, b, p.lds_bytes);
            CHECK(p.na == a + 1 && p.nb == b + 1, "bytes %d x %d: bins %d x %d", a, b, p.na, p.nb);
        }
    CHECK(sweep_mi_lds_bytes(31, 31) == 64 * 1024, "bytes: 32 x 32 bins are 64 KiB");
}

// ---- refusals -------------------------------------------------------------------------------------------------------
void refused(const char* name, const MiPlan& p, int code, const char* part) {
    CHECK(p.code == code, "%s: code %d, expected %d", name, p.code, code);
    CHECK(p.msg && std::strstr(p.msg, part), "%s: message '%s' lacks '%s'", name, p.msg ? p.msg : "(none)", part);
    CHECK(p.groups.empty() && p.grid == 0, "%s: a refusal with a plan", name);
}
void accepted(const char* name, const MiPlan& p) { CHECK(p.code == COREG_OK && !p.msg && p.grid > 0, "%s: refused (%s)", name, p.msg ? p.msg : ""); }

void check_refusals() {
    const std::vector<long long> o = pattern(32, 0);
    // a grid share
    refused("shard_world 2", sweep_mi_plan(request(o, 7, 15, 0, 2)), COREG_ENOTIMPL, "shard_world");
    accepted("shard_world 1", sweep_mi_plan(request(o, 7, 15, 0, 1)));
    refused("admit: shard_world 2", sweep_mi_admit(MiHave{2, 7, 15}), COREG_ENOTIMPL, "shard_world");
    // the bins
    refused("no bins", sweep_mi_plan(request(o, 0, 0)), COREG_ESTATE, "coreg_sweep_set_bins");
    refused("no small bins", sweep_mi_plan(request(o, 0, 15)), COREG_ESTATE, "coreg_sweep_set_bins");
    refused("no large bins", sweep_mi_plan(request(o, 7, 0)), COREG_ESTATE, "coreg_sweep_set_bins");
    refused("admit: no bins", sweep_mi_admit(MiHave{1, 0, 0}), COREG_ESTATE, "coreg_sweep_set_bins");
    accepted("one edge each", sweep_mi_plan(request(o, 1, 1)));
    accepted("31 edges each", sweep_mi_plan(request(o, 31, 31)));
    refused("32 small edges", sweep_mi_plan(request(o, 32, 31)), COREG_EINVAL, "31 edges");
    refused("32 large edges", sweep_mi_plan(request(o, 31, 32)), COREG_EINVAL, "31 edges");
    CHECK(sweep_mi_admit(MiHave{1, 31, 1}).code == COREG_OK, "admit: 31 x 1 edges refused");
    // the order: a grid share first, then the bins
    refused("shard_world 2 without bins", sweep_mi_plan(request(o, 0, 0, 0, 2)), COREG_ENOTIMPL, "shard_world");
    refused("no bins, bad chunks", sweep_mi_plan(request(o, 0, 0, -1)), COREG_ESTATE, "coreg_sweep_set_bins");
    // the chunks
    refused("mi_chunks -1", sweep_mi_plan(request(o, 7, 15, -1)), COREG_EINVAL, "mi_chunks");
    refused("mi_chunks 65", sweep_mi_plan(request(o, 7, 15, 65)), COREG_EINVAL, "mi_chunks");
    accepted("mi_chunks 64", sweep_mi_plan(request(o, 7, 15, 64)));
    accepted("mi_chunks 0", sweep_mi_plan(request(o, 7, 15, 0)));
    // the slots
    std::vector<long long> odd = pattern(24, 0), none;
    refused("24 slots", sweep_mi_plan(request(odd)), COREG_EINVAL, "multiple of 16");
    refused("no slots", sweep_mi_plan(MiRequest{MiHave{1, 7, 15}, 0, o.data(), 0}), COREG_EINVAL, "multiple of 16");
    refused("null output indices", sweep_mi_plan(MiRequest{MiHave{1, 7, 15}, 32, nullptr, 0}), COREG_EINVAL, "multiple of 16");
    accepted("16 slots", sweep_mi_plan(request(pattern(16, 0))));
    // the work space: 2^31 - 1 bytes at most (32 x 32 bins are 4096 bytes per slot); only the size is read before the refusal
    const long long fits = (kMiMaxHistBytes / 4096) / 16 * 16, over = fits + 16;
    CHECK(sweep_mi_hist_bytes(fits, 31, 31) <= kMiMaxHistBytes && sweep_mi_hist_bytes(over, 31, 31) > kMiMaxHistBytes,
          "work space: %lld / %lld slots do not straddle the limit", fits, over);
    refused("work space", sweep_mi_plan(MiRequest{MiHave{1, 31, 31}, over, o.data(), 0}), COREG_EINVAL, "work space too large");
    std::vector<long long> big((size_t)fits, 5);
    accepted("largest work space", sweep_mi_plan(MiRequest{MiHave{1, 31, 31}, fits, big.data(), 1}));
}
}  // namespace

int main() {
    check_groups();
    check_chunks();
    check_bytes();
    check_refusals();
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: sweep mi rules, %d checks\n", n_checked);
    return 0;
}
