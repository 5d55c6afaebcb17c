// Host-only logic of libd2d.so that D2D_FUN_RECEIVED_POWER_PER_OBJECT touches (differt2d_amd/csrc/d2d_host.hpp: check_params and
// sweep_thresholds' optional coefficient arguments), compiled with plain g++ and driven through ctypes by
// tests/test_object_coefs_cpu.py.  The product compiles the very same header into libd2d.so with hipcc.
#include "../../differt2d_amd/csrc/d2d_host.hpp"

extern "C" {

int oc_check_params(const d2d_params* p) {
    std::string err;
    return d2d_host::check_params(p, err);
}

// out: {sig_l2f, sig_mono, fnum[2], h2}
void oc_sweep_thresholds(const d2d_params* p, int grad, const float* coef, const uint8_t* allowed, int n, float* out) {
    const d2d_host::SweepThresholds t = d2d_host::sweep_thresholds(*p, grad != 0, coef, allowed, n);
    out[0] = t.sig_l2f;
    out[1] = (float)t.sig_mono;
    out[2] = t.fnum[2];
    out[3] = t.h2;
}
}
