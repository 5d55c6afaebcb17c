// Translation unit of the reverse-mode MinPath / FermatPath value+gradient sweep (d2d_optrev.hpp).
#define D2D_OPTREV_KERNELS 1
#include "d2d_optrev.hpp"

namespace d2d {

template <bool CUST, bool SGD>
static void launch_opt_rev_t(int K, const OptRevArgs& a, int c_first, dim3 grid, size_t lds, hipStream_t stream) {
    switch (K) {
        // order 0 runs no optimiser: the Adam instance serves every optimiser there
        case 0: hipLaunchKernelGGL((power_opt_rev_kernel<0, CUST, false>), grid, dim3(64), lds, stream, a, c_first); break;
        case 1: hipLaunchKernelGGL((power_opt_rev_kernel<1, CUST, SGD>), grid, dim3(64), lds, stream, a, c_first); break;
        case 2: hipLaunchKernelGGL((power_opt_rev_kernel<2, CUST, SGD>), grid, dim3(64), lds, stream, a, c_first); break;
        case 3: hipLaunchKernelGGL((power_opt_rev_kernel<3, CUST, SGD>), grid, dim3(64), lds, stream, a, c_first); break;
        default: hipLaunchKernelGGL((power_opt_rev_kernel<4, CUST, SGD>), grid, dim3(64), lds, stream, a, c_first); break;
    }
}

hipError_t launch_opt_rev(int K, const OptRevArgs& a, int c_first, dim3 grid, size_t lds, hipStream_t stream) {
    const bool cust = a.g.s.fun_id == D2D_FUN_CUSTOM;
    if (a.g.s.A.sgd) {
        if (cust) launch_opt_rev_t<true, true>(K, a, c_first, grid, lds, stream);
        else launch_opt_rev_t<false, true>(K, a, c_first, grid, lds, stream);
    } else {
        if (cust) launch_opt_rev_t<true, false>(K, a, c_first, grid, lds, stream);
        else launch_opt_rev_t<false, false>(K, a, c_first, grid, lds, stream);
    }
    return hipGetLastError();
}

}  // namespace d2d
