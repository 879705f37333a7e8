// mn_dispatch.hpp — the one row-length dispatch of the launchers (host code only).
//
// A kernel that walks rows is instantiated per (ORDER, NCH): the reference's order has one walk (NCH 0), the wave order one per
// chunk count — NCH x 256 floats cover a row of ld floats, 0 is the generic loop (mn_dist.hpp).  Eight pairs in all; the helpers
// below call a generic callable with the pair as compile-time constants and instantiate it for exactly those eight:
//   mn_for_row_walk(ix.order, ix.ld, [&](auto O, auto N) { hipLaunchKernelGGL((k<O(), N()>), ...); });
#pragma once
#include "mn_device.hpp"
#include <type_traits>

// the wave order's chunk count for rows of ld floats: the one table
inline int mn_pick_nch(int ld) {
    const int need = (ld + 255) / 256;
    if (need <= 1) return 1;
    if (need <= 2) return 2;
    if (need <= 3) return 3;
    if (need <= 4) return 4;
    if (need <= 6) return 6;
    if (need <= 8) return 8;
    return 0;
}

// the wave order alone (mn_launch_search picks its reference-order walk by another rule)
template <typename F> inline auto mn_for_wave_walk(int ld, F &&f) {
    using O = std::integral_constant<int, MN_ORDER_WAVE_V>;
    switch (mn_pick_nch(ld)) {
    case 1: return f(O(), std::integral_constant<int, 1>());
    case 2: return f(O(), std::integral_constant<int, 2>());
    case 3: return f(O(), std::integral_constant<int, 3>());
    case 4: return f(O(), std::integral_constant<int, 4>());
    case 6: return f(O(), std::integral_constant<int, 6>());
    case 8: return f(O(), std::integral_constant<int, 8>());
    default: return f(O(), std::integral_constant<int, 0>());
    }
}

template <typename F> inline auto mn_for_row_walk(int order, int ld, F &&f) {
    if (order == MN_ORDER_SSE_V)
        return f(std::integral_constant<int, MN_ORDER_SSE_V>(), std::integral_constant<int, 0>());
    return mn_for_wave_walk(ld, f);
}
