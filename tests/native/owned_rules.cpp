// The four owning types of the library (csrc/host_owned.hpp: DevBuf, PinBuf, Event, Stream) against a stub of the HIP
// calls they make.  The stub hands out heap blocks and keeps a journal of every call, so the rules below are read off
// the journal; built with -fsanitize=address,undefined a double free, a use after a move or a block nobody freed also
// ends the run.  No GPU, no HIP runtime.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// ---- the stub --------------------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct StubEvent* hipEvent_t;
typedef struct StubStream* hipStream_t;
struct StubEvent { int unused; };
struct StubStream { int unused; };
constexpr unsigned hipHostMallocDefault = 0, hipHostMallocPortable = 1;

struct Call {
    char what;  // 'M' hipMalloc, 'F' hipFree, 'H' hipHostMalloc, 'f' hipHostFree, 'e' hipEventDestroy, 's' hipStreamDestroy
    void* p;
    size_t bytes;
    unsigned flags;
};
static std::vector<Call> g_calls;
static bool g_fail_alloc = false;

static hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_alloc) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    g_calls.push_back({'M', *p, bytes, 0});
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    g_calls.push_back({'F', p, 0, 0});
    std::free(p);
    return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    if (g_fail_alloc) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    g_calls.push_back({'H', *p, bytes, flags});
    return hipSuccess;
}
static hipError_t hipHostFree(void* p) {
    g_calls.push_back({'f', p, 0, 0});
    std::free(p);
    return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
    g_calls.push_back({'e', e, 0, 0});
    delete e;
    return hipSuccess;
}
static hipError_t hipStreamDestroy(hipStream_t s) {
    g_calls.push_back({'s', s, 0, 0});
    delete s;
    return hipSuccess;
}

#include "../../euispice_coreg_amd/csrc/host_owned.hpp"

// ---- the rules -------------------------------------------------------------------------------------------------------
static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++g_bad;                                                         \
        }                                                                    \
    } while (0)

static std::string journal() {  // the calls so far, one letter each; the journal starts again
    std::string s;
    for (const Call& c : g_calls) s += c.what;
    g_calls.clear();
    return s;
}
static size_t count(char what, const void* p) {
    size_t n = 0;
    for (const Call& c : g_calls) n += c.what == what && c.p == p;
    return n;
}

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf copies");
static_assert(!std::is_copy_constructible<PinBuf>::value && !std::is_copy_assignable<PinBuf>::value, "PinBuf copies");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "Event copies");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "Stream copies");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_constructible<PinBuf>::value &&
                  std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_constructible<Stream>::value,
              "a move may not throw: std::vector would copy instead");

// reserve: the growth sizes, nothing done when the block is large enough, the old block freed BEFORE the new one is made
static void rule_reserve() {
    {
        DevBuf d;
        CHECK(d.reserve(0) == hipSuccess && d.p == nullptr && journal() == "");
        CHECK(d.reserve(1000) == hipSuccess && d.cap == 1000 + 250 + 256 && d.p != nullptr);
        CHECK(g_calls.size() == 1 && g_calls[0].what == 'M' && g_calls[0].bytes == 1506 && g_calls[0].p == d.p);
        void* first = d.p;
        g_calls.clear();
        CHECK(d.reserve(1506) == hipSuccess && d.p == first && journal() == "");
        CHECK(d.reserve(1507) == hipSuccess && d.cap == 1507 + 376 + 256);
        CHECK(g_calls.size() == 2 && g_calls[0].what == 'F' && g_calls[0].p == first && g_calls[1].what == 'M' &&
              g_calls[1].bytes == 2139);
        CHECK(d.as<double>() == (double*)d.p);
        g_calls.clear();
        g_fail_alloc = true;  // a refused allocation leaves the buffer empty: nothing to free later
        CHECK(d.reserve(5000) == hipErrorOutOfMemory && d.p == nullptr && d.cap == 0 && journal() == "F");
        g_fail_alloc = false;
    }
    CHECK(journal() == "");
    {
        PinBuf b;
        CHECK(b.reserve(1000) == hipSuccess && b.cap == 1000 + 500 + 4096);
        CHECK(g_calls.size() == 1 && g_calls[0].what == 'H' && g_calls[0].bytes == 5596 && g_calls[0].flags == hipHostMallocDefault);
        void* first = b.p;
        g_calls.clear();
        CHECK(b.reserve(5596) == hipSuccess && b.p == first && journal() == "");
        CHECK(b.reserve(8000, hipHostMallocPortable, 8) == hipSuccess && b.cap == 8000 + 1000 + 4096);
        CHECK(g_calls.size() == 2 && g_calls[0].what == 'f' && g_calls[0].p == first && g_calls[1].what == 'H' &&
              g_calls[1].bytes == 13096 && g_calls[1].flags == hipHostMallocPortable);
        g_calls.clear();
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && journal() == "f");
        b.release();
        CHECK(journal() == "");
    }
    CHECK(journal() == "");
}

// a move leaves the source empty and frees nothing; whoever holds the block at the end frees it, once
template <typename Buf>
static void rule_move_buf(char free_call) {
    void* block = nullptr;
    {
        Buf a;
        CHECK(a.reserve(64) == hipSuccess);
        block = a.p;
        const size_t cap = a.cap;
        g_calls.clear();
        Buf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == block && b.cap == cap && journal() == "");
        Buf c;
        CHECK(c.reserve(8) == hipSuccess);
        void* old = c.p;
        g_calls.clear();
        c = std::move(b);  // the target's own block goes, once; the moved block does not
        CHECK(b.p == nullptr && b.cap == 0 && c.p == block && c.cap == cap);
        CHECK(g_calls.size() == 1 && g_calls[0].what == free_call && g_calls[0].p == old);
        g_calls.clear();
        Buf& self = c;
        c = std::move(self);
        CHECK(c.p == block && journal() == "");
    }
    CHECK(g_calls.size() == 1 && count(free_call, block) == 1);  // a, b: nothing; c: the block
    g_calls.clear();
}

static void rule_event() {
    hipEvent_t raw = new StubEvent();
    {
        Event a;
        CHECK(!a);
        a.e = raw;  // (as hipEventCreate(&a.e) leaves it)
        Event b(std::move(a));
        CHECK(a.e == nullptr && (hipEvent_t)b == raw && journal() == "");
        std::vector<Event> v;
        v.push_back(std::move(b));
        v.resize(40);  // reallocates: moves, no destroy
        CHECK(b.e == nullptr && (hipEvent_t)v[0] == raw && journal() == "");
        v[0].reset();
        CHECK(!v[0] && g_calls.size() == 1 && count('e', raw) == 1);
        g_calls.clear();
        v[0].reset();
    }
    CHECK(journal() == "");
    hipEvent_t raw2 = new StubEvent();
    {
        Event a;
        a.e = raw2;
    }
    CHECK(g_calls.size() == 1 && count('e', raw2) == 1);
    g_calls.clear();
}

// a stream of the library's is destroyed once; a borrowed one never, and borrowing lets go of the library's own first
static void rule_stream() {
    StubStream callers;
    hipStream_t own = new StubStream();
    {
        Stream s;
        CHECK(!s && s.owned);
        s.s = own;  // (as hipStreamCreateWithFlags(&s.s, ...) leaves it)
        Stream t(std::move(s));
        CHECK(s.s == nullptr && (hipStream_t)t == own && t.owned && journal() == "");
        CHECK(t.borrow(&callers) == hipSuccess && (hipStream_t)t == &callers && !t.owned);
        CHECK(g_calls.size() == 1 && count('s', own) == 1);
        g_calls.clear();
        Stream u(std::move(t));  // being borrowed moves along
        CHECK(!u.owned && (hipStream_t)u == &callers && t.s == nullptr && t.owned);
        StubStream other;
        CHECK(u.borrow(&other) == hipSuccess && (hipStream_t)u == &other && journal() == "");
    }
    CHECK(journal() == "");
    hipStream_t own2 = new StubStream();
    {
        Stream s;
        s.s = own2;
    }
    CHECK(g_calls.size() == 1 && count('s', own2) == 1);
    g_calls.clear();
}

// a std::vector of buffers, grown (it moves its elements to a new array) and cleared: every block freed once
static void rule_vector() {
    std::vector<void*> blocks;
    {
        std::vector<DevBuf> v;
        v.resize(3);
        for (DevBuf& d : v) {
            CHECK(d.reserve(100) == hipSuccess);
            blocks.push_back(d.p);
        }
        g_calls.clear();
        v.resize(v.capacity() + 50);
        CHECK(journal() == "");
        for (size_t k = 0; k < 3; ++k) CHECK(v[k].p == blocks[k]);
        CHECK(v[7].reserve(100) == hipSuccess);
        blocks.push_back(v[7].p);
        g_calls.clear();
        v.resize(2);  // drops [2] and [7]
        CHECK(g_calls.size() == 2 && count('F', blocks[2]) == 1 && count('F', blocks[3]) == 1);
        g_calls.clear();
        v.clear();
        CHECK(g_calls.size() == 2 && count('F', blocks[0]) == 1 && count('F', blocks[1]) == 1);
        g_calls.clear();
    }
    CHECK(journal() == "");
    {
        std::vector<PinBuf> v(4);
        CHECK(v[1].reserve(10) == hipSuccess);
        void* block = v[1].p;
        g_calls.clear();
        v.resize(v.capacity() + 9);
        v.clear();
        CHECK(g_calls.size() == 1 && count('f', block) == 1);
        g_calls.clear();
    }
    CHECK(journal() == "");
}

int main() {
    rule_reserve();
    rule_move_buf<DevBuf>('F');
    rule_move_buf<PinBuf>('f');
    rule_event();
    rule_stream();
    rule_vector();
    if (g_bad) return 1;
    std::printf("ok: owned rules\n");
    return 0;
}
