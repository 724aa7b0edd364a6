// The compile-time schedules of the float32 tapered FFT (mtmfft_dec_kernel.h) - one place: the instance units
// (mtmfft_dec_{a..o}.hip), the sub-transforms of the decimation through HBM (mtmfft_declong_{a,b}.hip) and the kernel
// emulator of the tests read the names, so a length means the same schedule to all of them.  The lengths themselves are
// listed in mtmfft_route.h (DEC_LENGTHS, HALF_LENGTHS).
#pragma once
#include "mtmfft_dec_kernel.h"

namespace spyfft {

//                    V   R1  R2  R3  G   P  SPLIT
using D_100   = CfgD<10, 10, 1,  1,  16>;
using D_200   = CfgD<10, 10, 2,  1,  8>;
using D_400   = CfgD<10, 10, 2,  2,  8>;
using D_500   = CfgD<10, 10, 5,  1,  4>;
using D_800   = CfgD<20, 20, 2,  1,  4>;
using D_1000  = CfgD<10, 10, 10, 1,  2>;
using D_1600  = CfgD<20, 20, 4,  1,  2>;
using D_2000  = CfgD<10, 10, 10, 2,  1>;
using D_2000_C2 = CfgD<20, 10, 10, 1, 2>;       // complex spectra of every taper, two quads per workgroup (mtmfft_dec_c.hip)
using D_2500  = CfgD<10, 10, 5,  5,  1>;
using D_3200  = CfgD<20, 20, 4,  2,  1>;
using D_4000  = CfgD<20, 20, 10, 1,  1>;
using D_4096  = CfgD<16, 16, 16, 1,  1>;        // (sub-transform of the decimation through HBM only)
using D_5000  = CfgD<10, 10, 10, 5,  1>;
using D_8000  = CfgD<20, 20, 20, 1,  1>;
using D_10000 = CfgD<20, 20, 5,  5,  1, 1, true>;
// 3 x (a schedule): three sub-transforms side by side + one radix-3 combine (CfgD::P)
using D_300   = CfgD<10, 10, 1,  1,  8, 3>;
using D_600   = CfgD<10, 10, 2,  1,  4, 3>;
using D_768   = CfgD<16, 16, 1,  1,  4, 3>;
using D_1200  = CfgD<10, 10, 2,  2,  2, 3>;
using D_1500  = CfgD<10, 10, 5,  1,  2, 3>;
using D_1536  = CfgD<16, 16, 2,  1,  2, 3>;
using D_2400  = CfgD<20, 20, 2,  1,  1, 3>;
using D_3000  = CfgD<10, 10, 10, 1,  1, 3>;
using D_3072  = CfgD<16, 16, 4,  1,  1, 3>;
using D_4800  = CfgD<20, 20, 4,  1,  1, 3>;
using D_6000  = CfgD<10, 10, 10, 2,  1, 3>;
using D_6144  = CfgD<16, 16, 8,  1,  1, 3>;
using D_7500  = CfgD<10, 10, 5,  5,  1, 3>;
// HALF form: channel pairs, the real transform of 2 N samples through the schedule of N
//                     V   R1  R2  R3  G   P  SPLIT  HALF
using DH_5000  = CfgD<10, 10, 5,  5,  1, 1, false, true>;
using DH_10000 = CfgD<10, 10, 10, 5,  1, 1, false, true>;
using DH_12000 = CfgD<10, 10, 10, 2,  1, 3, false, true>;
using DH_12288 = CfgD<16, 16, 8,  1,  1, 3, false, true>;
using DH_15000 = CfgD<10, 10, 5,  5,  1, 3, false, true>;
using DH_16000 = CfgD<20, 20, 20, 1,  1, 1, false, true>;
using DH_20000 = CfgD<20, 20, 5,  5,  1, 1, true,  true>;

}  // namespace spyfft
