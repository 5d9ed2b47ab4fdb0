// grb_jit.hpp — the hipRTC binding and the code-object cache on disk that grb_chain_jit.cpp owns, for the other run-time compiled kernels (grb_userop.cpp).
#pragma once
#include "grb_internal.hpp"
#include <string>

namespace grb {

bool jit_available();      // libhiprtc was found and bound (tried once per process)
// `src` -> a loaded function named `entry`: from <cache dir>/<file_prefix>-<hash>.co when it is there, else compiled (-O3, -ffp-contract=off, the device's
// architecture) and written there.  The hash covers the source, the architecture, the hipRTC version and the options.  Holds no lock; `log` (may be
// nullptr) receives the compiler's log when the compilation fails.
bool jit_build_kernel(const std::string& src, const char* entry, const char* file_prefix, hipModule_t* mod, hipFunction_t* fn, bool* from_disk, std::string* log);

}  // namespace grb
