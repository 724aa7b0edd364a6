// CPU emulation of the summary statistics, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/stats.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_stats.py.
#include "hip_emu.h"

// shims: LDS integer atomics, the float64 square root, bit casts
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline double __dsqrt_rn(double a) { return std::sqrt(a); }
static inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }

#include "../../syncopy_amd/csrc/stats.hip"
#include "emu_unit.h"
