// Wavelengths per pass of the chunked sink products and the register tables' sizes, stated once for the kernels (d2d_sinks.hpp) and
// the host's chunk plans (d2d_host.hpp).  Plain C++: tests/native/*.cpp compile it with g++.  The chunk sizes are internal, not in
// the ABI (POS_CHUNK, which is part of its product's definition, is d2d_posgrad.hpp's).
#pragma once

#include "../../include/d2d.h"

namespace d2d {

constexpr int FREQ_CHUNK = 8;   // frequency response and its coefficient adjoint: wavelengths per launch
constexpr int MAT_CHUNK = 8;    // material response and its permittivity adjoint
constexpr int WIDE_CHUNK = 32;  // wideband array response
constexpr int BEAM_CHUNK = 64;  // beam-space response
constexpr int ARRAY_MAX = D2D_ARRAY_MAX;
constexpr int BEAM_MAX = D2D_BEAM_MAX;

}  // namespace d2d
