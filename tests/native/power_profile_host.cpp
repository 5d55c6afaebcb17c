// Host-only logic of libd2d.so that d2d_power_profile_launch touches (differt2d_amd/csrc/d2d_host.hpp: profile_bins, the one place
// the length range is checked and `inv` is formed), compiled with plain g++ and driven through ctypes by
// tests/test_power_profile_cpu.py.  The product compiles the very same header into libd2d.so with hipcc.
#include <cstring>

#include "../../differt2d_amd/csrc/d2d_host.hpp"

extern "C" {

// returns profile_bins' status; out: {r_min, inv, (float)nbins}; msg (cap bytes): the refusal's reason
int pp_profile_bins(float r_min, float r_max, int32_t nbins, float* out, char* msg, int cap) {
    d2d_host::ProfileBins b;
    std::string err;
    const int rc = d2d_host::profile_bins(r_min, r_max, nbins, b, err);
    out[0] = b.r_min;
    out[1] = b.inv;
    out[2] = (float)b.nbins;
    if (msg && cap > 0) {
        std::strncpy(msg, err.c_str(), (size_t)cap - 1);
        msg[cap - 1] = 0;
    }
    return rc;
}
}
