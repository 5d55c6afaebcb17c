// The k strongest contributions of a cell (d2d_strongest_paths_launch, d2d::TopSink): TOP_SLOTS slots per lane, sorted by
//     key = bit pattern of fabsf(t), compared as uint32      (a total order: NaN ranks above inf; an empty slot has key 0)
// descending; among equal keys the earlier candidate comes first.  top_insert puts a new entry in front of the first slot whose
// key is STRICTLY smaller, and the entry past the last slot falls off -- so an entry that ties with kept ones goes behind them,
// and one that ties across the cut is the one that is dropped.
//
// Written once, with compile-time slot indices (a lane's slots are registers: an index that is not a constant would send them to
// scratch), and free of HIP builtins: the position comes from the strict comparisons first -- the slots are sorted, so the ones
// that are not strictly smaller are a prefix and their number is the position -- then the slots move from the bottom up, every
// one reading its upper neighbour before that is overwritten.  (A bubble that swaps with `>` all the way down mis-places a
// displaced entry among equal keys.)  tests/native/strongest_paths_host.cpp compiles this text with g++ and
// tests/test_strongest_paths_cpu.py holds it to a stable sort.
#pragma once
#include <stdint.h>

namespace d2d {

constexpr int TOP_SLOTS = 8;  // = D2D_TOP_MAX (include/d2d.h)

// One lane's slots.  tb: the contribution's bits (0 = +0.0: empty, a contribution that is exactly zero never gets here); rb: the
// path length's bits; lo: code bits 0..31; hi: code bits 32..47 | order << 24 (the record's packing, RecSink).
struct TopSlots {
    uint32_t tb[TOP_SLOTS], rb[TOP_SLOTS], lo[TOP_SLOTS], hi[TOP_SLOTS];
};

constexpr uint32_t top_key(uint32_t tb) { return tb & 0x7fffffffu; }

template <int I>
struct TopStep {
    __attribute__((always_inline)) static constexpr int position(const TopSlots& s, uint32_t key) {
        return TopStep<I - 1>::position(s, key) + (top_key(s.tb[I - 1]) >= key ? 1 : 0);
    }
    // slots I-1 down to 0
    __attribute__((always_inline)) static constexpr void shift(TopSlots& s, int pos, uint32_t tb, uint32_t rb, uint32_t lo, uint32_t hi) {
        constexpr int i = I - 1;
        constexpr int up = i > 0 ? i - 1 : 0;
        const bool moves = i > pos, lands = i == pos;
        // (both neighbours are read first, so that the choice is one between values: a choice between the two loads is
        // turned into a load at a chosen address, and that is an indexed register array)
        const uint32_t tb_up = s.tb[up], rb_up = s.rb[up], lo_up = s.lo[up], hi_up = s.hi[up];
        const uint32_t tb_i = s.tb[i], rb_i = s.rb[i], lo_i = s.lo[i], hi_i = s.hi[i];
        s.tb[i] = moves ? tb_up : lands ? tb : tb_i;
        s.rb[i] = moves ? rb_up : lands ? rb : rb_i;
        s.lo[i] = moves ? lo_up : lands ? lo : lo_i;
        s.hi[i] = moves ? hi_up : lands ? hi : hi_i;
        TopStep<I - 1>::shift(s, pos, tb, rb, lo, hi);
    }
    __attribute__((always_inline)) static constexpr void clear(TopSlots& s) {
        s.tb[I - 1] = s.rb[I - 1] = s.lo[I - 1] = s.hi[I - 1] = 0u;
        TopStep<I - 1>::clear(s);
    }
};
template <>
struct TopStep<0> {
    __attribute__((always_inline)) static constexpr int position(const TopSlots&, uint32_t) { return 0; }
    __attribute__((always_inline)) static constexpr void shift(TopSlots&, int, uint32_t, uint32_t, uint32_t, uint32_t) {}
    __attribute__((always_inline)) static constexpr void clear(TopSlots&) {}
};

__attribute__((always_inline)) constexpr void top_clear(TopSlots& s) { TopStep<TOP_SLOTS>::clear(s); }

// tb's key must not be 0.  A position of TOP_SLOTS: every slot is at least as strong, the entry itself falls off.
__attribute__((always_inline)) constexpr void top_insert(TopSlots& s, uint32_t tb, uint32_t rb, uint32_t lo, uint32_t hi) {
    const int pos = TopStep<TOP_SLOTS>::position(s, top_key(tb));
    TopStep<TOP_SLOTS>::shift(s, pos, tb, rb, lo, hi);
}

}  // namespace d2d
