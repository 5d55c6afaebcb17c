// The insertion of d2d_strongest_paths_launch's sink (differt2d_amd/csrc/d2d_top.hpp: top_insert, the kernel's own text) and the
// host's memory check (d2d_host.hpp: outputs_fit with top_bytes_per_cell), compiled with plain g++ and driven through ctypes by
// tests/test_strongest_paths_cpu.py.  The product compiles the very same headers into libd2d.so with hipcc, where
// d2d::TopSink::put calls top_insert once per candidate and lane.
#include <cstring>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_top.hpp"

extern "C" {

// d2d_host.hpp's share of the launch: what the outputs take per cell, and whether they fit half of the free device memory
long long sp_bytes_per_cell(int k) { return (long long)d2d_host::top_bytes_per_cell(k); }
int sp_top_fits(long long cells, int k, long long mem_free, long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::top_bytes_per_cell(k), (size_t)mem_free, (size_t)held) ? 1 : 0;
}

int sp_top_slots() { return d2d::TOP_SLOTS; }

// Feeds the n items (t[i], r[i], tag i) through TopSink::put's steps -- zeros of either sign are counted out, everything else is
// inserted -- and writes all TOP_SLOTS slots: t_out, r_out (bit patterns as stored), tag_out (-1: empty).  Returns the number of
// items inserted.
int sp_top_stream(int n, const float* t, const float* r, float* t_out, float* r_out, int* tag_out) {
    d2d::TopSlots s;
    d2d::top_clear(s);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i] == 0.0f) continue;
        uint32_t tb, rb;
        std::memcpy(&tb, t + i, 4);
        std::memcpy(&rb, r + i, 4);
        ++count;
        d2d::top_insert(s, tb, rb, (uint32_t)i, (uint32_t)(i >> 3) | (5u << 24));
    }
    for (int j = 0; j < d2d::TOP_SLOTS; ++j) {
        std::memcpy(t_out + j, &s.tb[j], 4);
        std::memcpy(r_out + j, &s.rb[j], 4);
        const bool empty = d2d::top_key(s.tb[j]) == 0u;
        // (lo and hi travel with their slot: an entry whose halves were torn apart shows as a tag that does not match)
        tag_out[j] = empty ? -1 : (s.hi[j] == ((s.lo[j] >> 3) | (5u << 24)) ? (int)s.lo[j] : -2);
    }
    return count;
}
}
