// mtmfft_dec_kernel instances for 3 x a scheduled length: N = 300, 600, 1500, 3000 (see mtmfft_dec_launch.h)
#include "mtmfft_dec_launch.h"

namespace spyfft {
int dec_launch_f(hipStream_t stream, const MtmArgs& a, int nfft, int nquads, int outk, bool mean) {
    switch (nfft) {
        case 300: return dec_launch_mode<D_300>(stream, a, nquads, outk, mean);
        case 600: return dec_launch_mode<D_600>(stream, a, nquads, outk, mean);
        case 1500: return dec_launch_mode<D_1500>(stream, a, nquads, outk, mean);
        case 3000: return dec_launch_mode<D_3000>(stream, a, nquads, outk, mean);
        default: return -100;
    }
}
}  // namespace spyfft
