// Owning types of libd2d.so's host side: device buffers and the handles of events, streams and pinned memory.  Every one
// is move-only and frees what it holds in its destructor: a d2d_ctx (or a local of an entry point) needs no clean-up list.
// No HIP header, no HIP type: the runtime is reached through the five functions below.  d2d.hip defines them with the real
// calls, tests/native/d2d_host_san.cpp with counting stand-ins (g++ -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <utility>

namespace d2d_own {

int dev_alloc(void** p, size_t bytes);  // 0, or D2D_ERR_HIP through fail() with the HIP error string
void dev_free(void* p);
void pinned_free(void* p);
void event_destroy(void* h);
void stream_destroy(void* h);

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // at least `count` elements (0: one); a buffer that grows is freed first, its contents are not kept
    int ensure(size_t count) {
        if (count <= n && p) return 0;
        release();
        if (count == 0) count = 1;
        if (int rc = dev_alloc(reinterpret_cast<void**>(&p), count * sizeof(T))) return rc;
        n = count;
        return 0;
    }
    void release() {
        if (T* q = std::exchange(p, nullptr)) dev_free(q);
        n = 0;
    }
};

// A raw handle H (a pointer type) destroyed by Destroy.  Creation stays with the caller: create(x.put(), ...) on an
// empty handle.  Converts to H, so x goes wherever the raw handle went.
template <typename H, void (*Destroy)(void*)>
struct Unique {
    Unique() = default;
    Unique(Unique&& o) noexcept : h(std::exchange(o.h, H())) {}
    Unique& operator=(Unique&& o) noexcept {
        if (this != &o) {
            if (h) Destroy((void*)h);
            h = std::exchange(o.h, H());
        }
        return *this;
    }
    ~Unique() { if (h) Destroy((void*)h); }
    operator H() const { return h; }
    H* put() { return &h; }  // (of an empty handle only)

private:
    H h = H();
};

}  // namespace d2d_own
