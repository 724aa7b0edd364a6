// Instances of hilbert_packed_kernel for the power-of-two trial lengths 16 ... 8192 (hilbert_route.h: PACKED).
#include "hilbert_launch.h"

int spyhil::launch_packed(hipStream_t stream, const HilArgs& a, int log2n, bool cplx, unsigned grid) {
    switch (log2n) {
        case 4: return launch_one<4, false>(stream, a, cplx, grid);
        case 5: return launch_one<5, false>(stream, a, cplx, grid);
        case 6: return launch_one<6, false>(stream, a, cplx, grid);
        case 7: return launch_one<7, false>(stream, a, cplx, grid);
        case 8: return launch_one<8, false>(stream, a, cplx, grid);
        case 9: return launch_one<9, false>(stream, a, cplx, grid);
        case 10: return launch_one<10, false>(stream, a, cplx, grid);
        case 11: return launch_one<11, false>(stream, a, cplx, grid);
        case 12: return launch_one<12, false>(stream, a, cplx, grid);
        case 13: return launch_one<13, false>(stream, a, cplx, grid);
        default: return NO_INSTANCE;
    }
}
