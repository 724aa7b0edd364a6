// CPU emulation of the peristimulus histogram, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/psth.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/psth_drive.py.
#include "hip_emu.h"

// the LDS integer add the counting kernels use
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "../../syncopy_amd/csrc/psth.hip"
#include "emu_unit.h"

extern "C" int emu_psth_tiles(int* bin_tile, int* col_tile, int* unit_tile, int* prop_tile, int* threads) {
    *bin_tile = spypsth::BIN_TILE; *col_tile = spypsth::COL_TILE; *unit_tile = spypsth::UNIT_TILE;
    *prop_tile = spypsth::PROP_TILE; *threads = spypsth::THREADS;
    return 0;
}
