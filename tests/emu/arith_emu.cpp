// CPU emulation of the operator arithmetic, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/arith.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_arith.py.
#include "hip_emu.h"

// the correctly rounded float64 square root
static inline double __dsqrt_rn(double a) { return std::sqrt(a); }

#include "../../syncopy_amd/csrc/arith.hip"
#include "emu_unit.h"
