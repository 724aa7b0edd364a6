// The padded 3M instances csd3m_kernel<CH, 8, false> the kernel emulator builds (TEST INFRASTRUCTURE ONLY): a sample of
// the multiples of 16 up to 512 that the library holds.  The one list behind the emulator's "is it built" answer, its
// dispatch switch (csd_emu.cpp) and the route shim's sample (csd_route_shim.cpp).
#pragma once

#define EMU_M3_WIDTHS(X) X(16) X(32) X(48) X(64) X(96) X(128) X(192) X(240) X(256) X(304) X(320) X(384)

inline bool emu_have_m3(int chp) {
    switch (chp) {
#define EMU_M3_CASE(CH) case CH:
        EMU_M3_WIDTHS(EMU_M3_CASE)
#undef EMU_M3_CASE
        return true;
        default: return false;
    }
}
