// devbuf.h -- who owns device memory: an owning, move-only, grow-only buffer (device or pinned host), the walk that carves one
// block into typed members, and the process-wide count of live bytes.  Knows nothing of bohip_gp (DESIGN.md "Who owns device memory").
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace devbuf {

enum Kind { DEVICE = 0, PINNED = 1 };

// bytes held by live buffers, per kind; touched only where a buffer allocates or frees (bohip_debug_live_bytes)
inline std::atomic<int64_t> g_live_bytes[2];

// How much a buffer that must grow to `need` elements allocates.  The rules differ on purpose: they decide when the next
// reallocation happens and how much a handle holds.  Exact: scratch sized by the call (a repeat of the largest call never
// reallocates).  Half: blocks a caller's loop grows step by step (q, K, S creep up): amortised.  Quarter: the small-batch pass,
// whose need moves with the tile split the device picks.
enum class Grow { Exact, Half, Quarter };
inline size_t grown(Grow rule, size_t need, size_t old) {
    if (rule == Grow::Half) return need > old + old / 2 ? need : old + old / 2;
    if (rule == Grow::Quarter) return need + need / 4;
    return need;
}

#if defined(__HIPCC__)
struct HipAlloc {
    using error_t = hipError_t;
    using stream_t = hipStream_t;
    static constexpr error_t ok = hipSuccess;
    static error_t alloc(void** p, size_t bytes, Kind k) {
        return k == PINNED ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    }
    static error_t free(void* p, Kind k) { return k == PINNED ? hipHostFree(p) : hipFree(p); }
    static error_t sync(stream_t s) { return hipStreamSynchronize(s); }
};
using DefaultAlloc = HipAlloc;
#else
struct DefaultAlloc;   // host-only builds (tests/host/devbuf_check.cpp) name their own allocator
#endif

template <class T, Kind K = DEVICE, class A = DefaultAlloc>
class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements

    typename A::error_t grow(size_t n, typename A::stream_t s, Grow rule, bool* grew) {
        const size_t cap = grown(rule, n, cap_);
        if (p_) {   // a launch of an earlier call may still be using the old block
            typename A::error_t e = A::sync(s);
            if (e != A::ok) return e;
            e = release();
            if (e != A::ok) return e;
        }
        void* q = nullptr;
        const typename A::error_t e = A::alloc(&q, cap * sizeof(T), K);
        if (e != A::ok) return e;   // the buffer stays (nullptr, 0)
        p_ = static_cast<T*>(q);
        cap_ = cap;
        g_live_bytes[K] += (int64_t)(cap * sizeof(T));
        if (grew) *grew = true;
        return A::ok;
    }

public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Buf() { release(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }   // elements

    // Room for n elements.  The steady state is the one compare.  Otherwise: wait for `s`, free the old block (the contents are
    // NOT kept), allocate by `rule`; *grew is set (never cleared) so the caller can clear memory that must start at zero.
    typename A::error_t reserve(size_t n, typename A::stream_t s, Grow rule = Grow::Exact, bool* grew = nullptr) {
        if (n <= cap_) return A::ok;
        return grow(n, s, rule, grew);
    }
    typename A::error_t release() {
        if (!p_) return A::ok;
        const typename A::error_t e = A::free(p_, K);
        g_live_bytes[K] -= (int64_t)(cap_ * sizeof(T));
        p_ = nullptr;
        cap_ = 0;
        return e;
    }
};
template <class T, class A = DefaultAlloc>
using PinnedBuf = Buf<T, PINNED, A>;

// Walks a block: take<T>(n, align) is the next n elements of T at a multiple of `align` bytes from the base.  A layout is ONE
// function that takes its members from a Carve and returns total(); run on a null base it sizes the block, run on the block it
// yields the pointers -- the size and the pointers cannot disagree.
class Carve {
    uintptr_t base_;
    size_t off_ = 0;

public:
    explicit Carve(const void* base) : base_(reinterpret_cast<uintptr_t>(base)) {}
    template <class T>
    T* take(size_t n, size_t align = alignof(T)) {
        off_ = (off_ + align - 1) / align * align;
        T* p = reinterpret_cast<T*>(base_ + off_);
        off_ += n * sizeof(T);
        return p;
    }
    size_t total() const { return off_; }
};

}   // namespace devbuf
