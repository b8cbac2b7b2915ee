// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the four types that own a
// GPU resource -- device buffer, page-locked buffer, event, stream.  Each is move-only and frees what it holds in its
// destructor, on whatever device is current: whoever holds them sees to the device and to idle streams (coreg_handle,
// coreg_multi).  Needs nothing but the HIP runtime's declarations (tests/native/owned_rules.cpp supplies counting ones).
#pragma once
namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            cap = 0;
        }
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const {
        return (T*)p;
    }
};

struct PinBuf {  // page-locked host staging (async H2D without a host sync)
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~PinBuf() { release(); }
    // grows to bytes + bytes / slack_div + 4096
    hipError_t reserve(size_t bytes, unsigned flags = hipHostMallocDefault, size_t slack_div = 2) {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / slack_div + 4096;
        hipError_t e = hipHostMalloc(&p, want, flags);
        if (e != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

static_assert(!std::is_copy_constructible<DevBuf>::value && std::is_nothrow_move_constructible<DevBuf>::value, "DevBuf owns");
static_assert(!std::is_copy_constructible<PinBuf>::value && std::is_nothrow_move_constructible<PinBuf>::value, "PinBuf owns");

// an event the library created (hipEventCreate*(&ev.e)); reads as the hipEvent_t it holds
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    ~Event() { reset(); }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// a stream the library created (hipStreamCreate*(&st.s)), or one it was lent (borrow): that one is never destroyed
struct Stream {
    hipStream_t s = nullptr;
    bool owned = true;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)), owned(std::exchange(o.owned, true)) {}
    ~Stream() {
        if (s && owned) (void)hipStreamDestroy(s);
    }
    hipError_t borrow(hipStream_t other) {  // (a stream of the library's that cannot be destroyed stays held)
        if (s && owned) {
            const hipError_t e = hipStreamDestroy(s);
            if (e != hipSuccess) return e;
        }
        s = other;
        owned = false;
        return hipSuccess;
    }
    operator hipStream_t() const { return s; }
};

}  // namespace
