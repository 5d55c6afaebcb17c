// One translation unit per (kernel family, validity mode): instantiates the sweep kernels of that pair and defines the
// per-mode launcher (declared in d2d_launch.hpp) that d2d.hip's dispatchers call.  Compiled by the Makefile with
//   -DD2D_TU_FAMILY={0 fwd, 1 fwd_grad, 2 fwd_split, 3 txg, 4 vg, 6 fwd / 7 fwd_grad / 8 fwd_split with the orders >= 2
//   taken from the region lists (LISTED), 9 fwd_coop}  -DD2D_TU_MODE={0 hard, 1 hard_sigmoid, 2 sigmoid}: all 27 pairs;
//   5 region lists and 10 NaN scan once each (-DD2D_TU_MODE=0);
//   11 the sink kernel, one object per sink of D2D_SINKS (d2d_sinks.hpp) and mode 0 or 1 (no sigmoid instance): -DD2D_TU_SINK=<Sink>
#include <type_traits>

#include "d2d_launch.hpp"
#if D2D_TU_FAMILY == 10
#include "d2d_nanscan.hpp"
#elif D2D_TU_FAMILY == 11
#include "d2d_sinks.hpp"
#endif

#ifndef D2D_TU_FAMILY
#error "compile with -DD2D_TU_FAMILY=<0..11> -DD2D_TU_MODE=<0..2> (see the Makefile for the pairs that exist)"
#endif

namespace d2d {

constexpr int TU_MODE = D2D_TU_MODE;

// the kernels' MAXK for a launch of orders up to max_order (2 also covers orders 0 and 1): f(std::integral_constant<int, MAXK>)
template <class F>
static void by_maxk(int max_order, F f) {
    if (max_order <= 2) f(std::integral_constant<int, 2>{});
    else if (max_order == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

#if D2D_TU_FAMILY == 0
template <>
hipError_t launch_fwd_m<TU_MODE>(bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64);
    if (stats) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, true, decltype(K)::value>), grid, block, lds, s, a); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, false, decltype(K)::value>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 1
template <>
hipError_t launch_fwd_grad_m<TU_MODE>(int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64);
    by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, false, decltype(K)::value, true>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 2
template <>
hipError_t launch_fwd_split_m<TU_MODE>(bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64 * SPLIT_W);
    if (stats) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_split_kernel<TU_MODE, true, decltype(K)::value, SPLIT_W>), grid, block, lds, s, a); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_split_kernel<TU_MODE, false, decltype(K)::value, SPLIT_W>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 3
template <>
hipError_t launch_txg_m<TU_MODE>(bool listed, bool grad, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64);
    if (listed && grad) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_txg_kernel<TU_MODE, decltype(K)::value, true, true>), grid, block, lds, s, a); });
    else if (listed) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_txg_kernel<TU_MODE, decltype(K)::value, false, true>), grid, block, lds, s, a); });
    else if (grad) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_txg_kernel<TU_MODE, decltype(K)::value, true>), grid, block, lds, s, a); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_txg_kernel<TU_MODE, decltype(K)::value>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 4
template <>
hipError_t launch_vg_m<TU_MODE>(bool txg, bool grad, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64);
    if (txg && grad) hipLaunchKernelGGL((power_vg_kernel<TU_MODE, true, true>), grid, block, lds, s, a);
    else if (txg) hipLaunchKernelGGL((power_vg_kernel<TU_MODE, true, false>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((power_vg_kernel<TU_MODE, false, true>), grid, block, lds, s, a);  // (RX grid, values only: launch_fwd)
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 6
template <>
hipError_t launch_fwd_listed_m<TU_MODE>(bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const bool wide = grid.y == 4;  // (grid.y carries the waves per workgroup: 1 or 4)
    const dim3 block(wide ? 256 : 64);
    grid.y = 1;
    if (stats) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, true, decltype(K)::value, false, true>), grid, block, lds, s, a); });
    else if (wide) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, false, decltype(K)::value, false, true, 4>), grid, block, lds, s, a); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, false, decltype(K)::value, false, true>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 7
template <>
hipError_t launch_fwd_grad_listed_m<TU_MODE>(int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64);
    by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_kernel<TU_MODE, false, decltype(K)::value, true, true>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 8
template <>
hipError_t launch_fwd_split_listed_m<TU_MODE>(bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64 * SPLIT_W);
    if (stats) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_split_kernel<TU_MODE, true, decltype(K)::value, SPLIT_W, true>), grid, block, lds, s, a); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_split_kernel<TU_MODE, false, decltype(K)::value, SPLIT_W, true>), grid, block, lds, s, a); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 9
template <int W>
static void launch_fwd_coop_w(int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    const dim3 block(64 * W);
    by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_fwd_coop_kernel<TU_MODE, decltype(K)::value, W>), grid, block, lds, s, a); });
}
template <>
hipError_t launch_fwd_coop_m<TU_MODE>(int max_order, int W, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    if (W == 16) launch_fwd_coop_w<16>(max_order, grid, lds, s, a);
    else if (W == 8) launch_fwd_coop_w<8>(max_order, grid, lds, s, a);
    else launch_fwd_coop_w<4>(max_order, grid, lds, s, a);
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 5
// region_list_kernel / region_refine_kernel <K, GRAD>: independent of the validity mode (compiled once, -DD2D_TU_MODE=0)
// (GRAD = false always: the value+grad sweeps read the forward sweeps' lists, their NaN positions come from d2d_nanscan.hpp)
hipError_t launch_region_lists(int K, bool txg, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const RegionLevel& lv,
                               const ListPool& lp) {
    const dim3 block(64);
    if (txg) by_maxk(K, [&](auto KK) { hipLaunchKernelGGL((region_list_kernel<decltype(KK)::value, false, true>), grid, block, lds, s, a, lv, lp); });
    else by_maxk(K, [&](auto KK) { hipLaunchKernelGGL((region_list_kernel<decltype(KK)::value, false, false>), grid, block, lds, s, a, lv, lp); });
    return hipGetLastError();
}
hipError_t launch_region_refine(int K, bool txg, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const RegionLevel& lv,
                                const RegionLevel& parent, const ListPool& lp, int* flag) {
    const dim3 block(64);
    if (txg) by_maxk(K, [&](auto KK) { hipLaunchKernelGGL((region_refine_kernel<decltype(KK)::value, false, true>), grid, block, lds, s, a, lv, parent, lp, flag); });
    else by_maxk(K, [&](auto KK) { hipLaunchKernelGGL((region_refine_kernel<decltype(KK)::value, false, false>), grid, block, lds, s, a, lv, parent, lp, flag); });
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 10
// nan_scan_kernel<APPROX, TXG, MAXK>: depends on hard / approx only (compiled once, -DD2D_TU_MODE=0)
// regions: nan_scan_region_kernel, and its DBG instance (run-time buffer sizes and counters -- tests; the product launches DBG = false)
template <bool APPROX, bool TXG>
static void launch_nan_scan_regions(int max_order, bool dbg, dim3 grid, dim3 block, size_t lds, hipStream_t s, const SweepArgs& a, unsigned long long* stats) {
    if (dbg) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((nan_scan_region_kernel<APPROX, TXG, decltype(K)::value, true>), grid, block, lds, s, a, stats); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((nan_scan_region_kernel<APPROX, TXG, decltype(K)::value>), grid, block, lds, s, a, stats); });
}
template <bool APPROX, bool TXG>
static void launch_nan_scan_patches(int max_order, dim3 grid, dim3 block, size_t lds, hipStream_t s, const SweepArgs& a, unsigned long long* stats) {
    by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((nan_scan_kernel<APPROX, TXG, decltype(K)::value>), grid, block, lds, s, a, stats); });
}
hipError_t launch_nan_scan(bool approx, bool txg, int max_order, bool regions, bool dbg, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a,
                           unsigned long long* stats) {
    const dim3 block(regions ? 64 * NAN_W : 64);
    if (regions) {
        if (approx && txg) launch_nan_scan_regions<true, true>(max_order, dbg, grid, block, lds, s, a, stats);
        else if (approx) launch_nan_scan_regions<true, false>(max_order, dbg, grid, block, lds, s, a, stats);
        else if (txg) launch_nan_scan_regions<false, true>(max_order, dbg, grid, block, lds, s, a, stats);
        else launch_nan_scan_regions<false, false>(max_order, dbg, grid, block, lds, s, a, stats);
    } else {
        if (approx && txg) launch_nan_scan_patches<true, true>(max_order, grid, block, lds, s, a, stats);
        else if (approx) launch_nan_scan_patches<true, false>(max_order, grid, block, lds, s, a, stats);
        else if (txg) launch_nan_scan_patches<false, true>(max_order, grid, block, lds, s, a, stats);
        else launch_nan_scan_patches<false, false>(max_order, grid, block, lds, s, a, stats);
    }
    return hipGetLastError();
}
hipError_t launch_nan_apply(hipStream_t s, const SweepArgs& a, long tiles) {
    hipLaunchKernelGGL(nan_apply_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, a.grad, a.partial, a.nan_cell_bits, a.nan_row_bits,
                       a.nan_row_words, a.N, a.m, a.n, tiles);
    return hipGetLastError();
}
#elif D2D_TU_FAMILY == 11
// power_sink_kernel<MODE, MAXK, TXG, Sink>: hard and hard_sigmoid only (the sigmoid sweeps' skips depend on the fused function's sum)
template <class Sink>
static hipError_t launch_sink_tu(bool txg, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const typename Sink::Args& x) {
    static_assert(TU_MODE == MODE_HARD || TU_MODE == MODE_HSIG, "the sink kernel has no sigmoid instance");
    const dim3 block(64);
    if (txg) by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_sink_kernel<TU_MODE, decltype(K)::value, true, Sink>), grid, block, lds, s, a, x); });
    else by_maxk(max_order, [&](auto K) { hipLaunchKernelGGL((power_sink_kernel<TU_MODE, decltype(K)::value, false, Sink>), grid, block, lds, s, a, x); });
    return hipGetLastError();
}
#ifndef D2D_TU_SINK
#error "family 11 is one object per sink: compile with -DD2D_TU_SINK=<a sink of D2D_SINKS>"
#endif
#define D2D_IS_TU_SINK(S) || std::is_same_v<S, D2D_TU_SINK>
static_assert(false D2D_SINKS(D2D_IS_TU_SINK), "D2D_TU_SINK is not in D2D_SINKS (d2d_sinks.hpp): the Makefile's SINKS and that list disagree");
#undef D2D_IS_TU_SINK
template <>
hipError_t launch_sink_m<TU_MODE, D2D_TU_SINK>(bool txg, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const D2D_TU_SINK::Args& x) {
    return launch_sink_tu<D2D_TU_SINK>(txg, max_order, grid, lds, s, a, x);
}
#else
#error "unknown D2D_TU_FAMILY"
#endif

}  // namespace d2d
