// C entry points over differt2d_amd/csrc/d2d_host.hpp -- the host-only logic of libd2d.so (candidate enumeration,
// parameter validation, sweep thresholds, launch buffer sizes, the reverse sweep's trajectory chunks) -- for the CPU sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared -fPIC
// (tests/test_host_sanitizers.py).  The product compiles the very same header into libd2d.so with hipcc.
// The same for differt2d_amd/csrc/d2d_own.hpp, the owning types of the context's GPU resources, over a counting stand-in
// for the five runtime functions it calls (d2d.hip defines those with the HIP calls).
#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_own.hpp"

#include <cstdlib>
#include <cstring>
#include <map>

// ---- the stand-in runtime: every allocation is a malloc of EXACTLY the bytes asked for (an overrun is an ASan report), kept
// in a ledger; a free or destroy of something the ledger does not hold (a second free, a moved-from copy) is counted, not done
namespace {
struct Ledger {
    std::map<void*, size_t> live;
    long long allocs = 0, frees = 0, bad_frees = 0;
    bool fail_next = false;
    void* take(size_t bytes) {
        void* q = std::malloc(bytes);
        live[q] = bytes;
        ++allocs;
        return q;
    }
    void give(void* q) {
        auto it = live.find(q);
        if (it == live.end()) {
            ++bad_frees;
            return;
        }
        live.erase(it);
        std::free(q);
        ++frees;
    }
} g_led;
}  // namespace

int d2d_own::dev_alloc(void** p, size_t bytes) {
    if (g_led.fail_next) {
        g_led.fail_next = false;
        return D2D_ERR_HIP;
    }
    *p = g_led.take(bytes);
    return 0;
}
void d2d_own::dev_free(void* p) { g_led.give(p); }
void d2d_own::pinned_free(void* p) { g_led.give(p); }
void d2d_own::event_destroy(void* h) { g_led.give(h); }
void d2d_own::stream_destroy(void* h) { g_led.give(h); }

namespace {
using d2d_own::DevBuf;
struct FakeEvent;
struct FakeStream;
using Event = d2d_own::Unique<FakeEvent*, d2d_own::event_destroy>;
using Stream = d2d_own::Unique<FakeStream*, d2d_own::stream_destroy>;
using Pinned = d2d_own::Unique<int*, d2d_own::pinned_free>;
template <class H> void create(H* h) { *h = static_cast<H>(g_led.take(1)); }

// the shape of d2d_ctx::PrepSet: buffers, a pointer into one of them, plain flags and an event
struct Set {
    DevBuf<unsigned long long> d_shadow;
    DevBuf<int> d_sched;
    long long cost_tiles = 0;
    int* rl_meta_ptr = nullptr;
    bool swept_pending = false;
    Event ev_swept;
};
// ... and of d2d_ctx: the main stream first, owners in between, three rotating sets
struct Ctx {
    Stream stream;
    Event ev0;
    DevBuf<float> d_a, d_b, d_c;
    Pinned h_meta;
    Set cur, spare[2];
    Stream aux;
};
}  // namespace

extern "C" {

int san_count(int32_t n, const uint8_t* allowed, int32_t lo, int32_t hi, int64_t* count) {
    std::string err;
    return d2d_host::count_candidates(n, allowed, lo, hi, count, err);
}

int san_enumerate(int32_t n, const uint8_t* allowed, int32_t lo, int32_t hi, int32_t* cand, int32_t* order, int64_t capacity) {
    std::string err;
    return d2d_host::enumerate_candidates(n, allowed, lo, hi, cand, order, capacity, err);
}

int san_check_params(const d2d_params* p, char* msg, int cap) {
    std::string err;
    const int rc = d2d_host::check_params(p, err);
    if (msg && cap > 0) {
        std::strncpy(msg, err.c_str(), (size_t)cap - 1);
        msg[cap - 1] = 0;
    }
    return rc;
}

float san_integer_pow(float x, int n) { return d2d_host::integer_pow(x, n); }

uint64_t san_hash_floats(const float* p, uint64_t n, uint64_t seed) { return d2d_host::hash_floats(p, (size_t)n, seed); }

void san_lds(int n_objects, int W, int list_len, uint64_t* tab, uint64_t* split_base, uint64_t* split_total) {
    *tab = d2d_host::tab_lds_bytes(n_objects);
    const d2d_host::SplitLds s = d2d_host::split_lds_bytes(n_objects, W, list_len);
    *split_base = s.base;
    *split_total = s.total;
}

void san_heavy_plan(long long tiles, long long Nc, long long heavy_split, long long parts, long long* out4) {
    const d2d_host::HeavyPlan hp = d2d_host::heavy_plan(tiles, Nc, heavy_split, parts);
    out4[0] = hp.H;
    out4[1] = hp.cap;
    out4[2] = hp.list_floats;
    out4[3] = hp.cnt_ints;
}

// out: on, top.R, top.S, top.regions, top.slots, leaf.R, leaf.S, leaf.regions, leaf.slots, n_static, max_chunks, k_lo
void san_region_plan(int tiles_x, int tiles_y, long long Nc, int min_order, int max_order, int R_leaf, int R_top, int S_req,
                     long long budget_bytes, int chunk, long long* out12) {
    const d2d_host::RegionPlan rp = d2d_host::region_plan(tiles_x, tiles_y, Nc, min_order, max_order, R_leaf, R_top, S_req, budget_bytes, chunk);
    out12[0] = rp.on ? 1 : 0;
    out12[1] = rp.top.R; out12[2] = rp.top.S; out12[3] = rp.top.regions; out12[4] = rp.top.slots;
    out12[5] = rp.leaf.R; out12[6] = rp.leaf.S; out12[7] = rp.leaf.regions; out12[8] = rp.leaf.slots;
    out12[9] = rp.n_static; out12[10] = rp.max_chunks; out12[11] = rp.k_lo;
}

// d: widen, widen_in, widen_flt; f: flt_lo, flt_hi, on_lo, on_hi, loss_skip, h2, sig_l2f, fnum[0 .. D2D_MAX_ORDER];
// i: mode, sig_mono, degenerate_invalid
void san_sweep_thresholds(const d2d_params* p, int grad, double* d3, float* f12, int* i3) {
    const d2d_host::SweepThresholds t = d2d_host::sweep_thresholds(*p, grad != 0);
    d3[0] = t.widen; d3[1] = t.widen_in; d3[2] = t.widen_flt;
    f12[0] = t.flt_lo; f12[1] = t.flt_hi; f12[2] = t.on_lo; f12[3] = t.on_hi; f12[4] = t.loss_skip; f12[5] = t.h2; f12[6] = t.sig_l2f;
    for (int k = 0; k <= D2D_MAX_ORDER; ++k) f12[7 + k] = t.fnum[k];
    i3[0] = t.mode; i3[1] = t.sig_mono; i3[2] = t.degenerate_invalid ? 1 : 0;
}

long long san_opt_chunk_cells(long long cells, long long floats_per_cell, long long traj_mb, int mem_known, long long free_bytes,
                              long long resident_bytes) {
    return d2d_host::opt_chunk_cells(cells, floats_per_cell, traj_mb, mem_known != 0, free_bytes, resident_bytes);
}

// ---- d2d_own.hpp ----
void san_own_counts(long long* out4) {
    out4[0] = g_led.allocs; out4[1] = g_led.frees; out4[2] = g_led.bad_frees; out4[3] = (long long)g_led.live.size();
}
void* san_buf_new() { return new DevBuf<float>(); }
void san_buf_delete(void* b) { delete static_cast<DevBuf<float>*>(b); }
int san_buf_ensure(void* b, uint64_t count, int fail) {
    g_led.fail_next = fail != 0;
    const int rc = static_cast<DevBuf<float>*>(b)->ensure((size_t)count);
    g_led.fail_next = false;
    return rc;
}
void san_buf_release(void* b) { static_cast<DevBuf<float>*>(b)->release(); }
// n, whether p is set, and the bytes the stand-in was asked for when it handed p out (-1: p is not a live allocation)
void san_buf_query(void* b, long long* out3) {
    const DevBuf<float>* d = static_cast<DevBuf<float>*>(b);
    out3[0] = (long long)d->n;
    out3[1] = d->p != nullptr;
    auto it = g_led.live.find(d->p);
    out3[2] = it == g_led.live.end() ? -1 : (long long)it->second;
    if (d->p) std::memset(d->p, 0x5a, d->n * sizeof(float));  // all of it is writable
}
void* san_buf_move_construct(void* b) { return new DevBuf<float>(std::move(*static_cast<DevBuf<float>*>(b))); }
void san_buf_move_assign(void* dst, void* src) {
    DevBuf<float>& d = *static_cast<DevBuf<float>*>(dst);
    DevBuf<float>& s = *static_cast<DevBuf<float>*>(src);  // (through references: dst == src is the self-assignment case)
    d = std::move(s);
}

// A context-like aggregate.  built: how many of its steps succeed (the next allocation fails and the rest is never created),
// as a d2d_create that fails half way; 9 or more: all of it.  Sets are tagged 100, 101, 102 (cur, spare[0], spare[1]).
void* san_ctx_new(int built) {
    Ctx* c = new Ctx();
    int step = 0;
    auto more = [&] { return step++ < built; };
    if (more()) create(c->stream.put());
    if (more()) create(c->ev0.put());
    if (more()) c->d_a.ensure(10);
    if (more()) c->d_b.ensure(0);
    if (more()) create(c->h_meta.put());
    Set* sets[3] = {&c->cur, &c->spare[0], &c->spare[1]};
    for (int i = 0; i < 3; ++i) {
        if (!more()) break;
        create(sets[i]->ev_swept.put());
        sets[i]->d_shadow.ensure(16 + (size_t)i);
        sets[i]->rl_meta_ptr = reinterpret_cast<int*>(sets[i]->d_shadow.p + 4);
        sets[i]->cost_tiles = 100 + i;
        sets[i]->swept_pending = i == 1;
    }
    if (more()) create(c->aux.put());
    if (built >= 9) return c;
    g_led.fail_next = true;
    (void)c->d_c.ensure(5);  // the failure itself: nothing allocated, nothing to free
    return c;
}
void san_ctx_delete(void* c) { delete static_cast<Ctx*>(c); }
// take_prep_set's rotation, `times` times: the oldest set becomes the current one, the current one the newest spare
void san_ctx_rotate(void* cv, int times) {
    Ctx* c = static_cast<Ctx*>(cv);
    for (int t = 0; t < times; ++t) {
        std::swap(c->cur, c->spare[0]);
        for (int i = 0; i + 1 < 2; ++i) std::swap(c->spare[i], c->spare[i + 1]);
        if (c->cur.d_sched.ensure(8 + (size_t)(t % 5) * 8)) return;  // (the sets also grow while they rotate)
    }
}
// per set (cur, spare[0], spare[1]): tag, d_shadow.n, whether rl_meta_ptr still points into its own d_shadow, swept_pending,
// whether the event is a live handle
void san_ctx_sets(void* cv, long long* out15) {
    Ctx* c = static_cast<Ctx*>(cv);
    const Set* sets[3] = {&c->cur, &c->spare[0], &c->spare[1]};
    for (int i = 0; i < 3; ++i) {
        const Set& s = *sets[i];
        out15[5 * i + 0] = s.cost_tiles;
        out15[5 * i + 1] = (long long)s.d_shadow.n;
        out15[5 * i + 2] = s.rl_meta_ptr == reinterpret_cast<const int*>(s.d_shadow.p + 4);
        out15[5 * i + 3] = s.swept_pending;
        out15[5 * i + 4] = g_led.live.count((FakeEvent*)s.ev_swept) == 1;
    }
}

}  // extern "C"
