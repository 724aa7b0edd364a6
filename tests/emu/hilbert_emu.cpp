// CPU emulation of the Hilbert transform, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own plan and launchers
// (syncopy_amd/csrc/hilbert.hip, hilbert_packed.hip, hilbert_blue.hip) and kernels, on the runtime stand-in
// hip/hip_runtime.h.  Built by tests/test_hilbert.py.
#include "../../syncopy_amd/csrc/hilbert.hip"
#include "../../syncopy_amd/csrc/hilbert_packed.hip"
#include "../../syncopy_amd/csrc/hilbert_blue.hip"
#include "emu_unit.h"
