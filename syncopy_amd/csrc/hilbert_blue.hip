// Instances of hilbert_packed_kernel in Bluestein's form: transform lengths M = 256 ... 8192 (hilbert_route.h: BLUE).
#include "hilbert_launch.h"

int spyhil::launch_blue(hipStream_t stream, const HilArgs& a, int log2n, bool cplx, unsigned grid) {
    switch (log2n) {
        case 8: return launch_one<8, true>(stream, a, cplx, grid);
        case 9: return launch_one<9, true>(stream, a, cplx, grid);
        case 10: return launch_one<10, true>(stream, a, cplx, grid);
        case 11: return launch_one<11, true>(stream, a, cplx, grid);
        case 12: return launch_one<12, true>(stream, a, cplx, grid);
        case 13: return launch_one<13, true>(stream, a, cplx, grid);
        default: return NO_INSTANCE;
    }
}
