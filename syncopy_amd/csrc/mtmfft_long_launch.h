// Host-side launch of the statistics pass of the transforms that go through HBM (mtmfft_long.h, mtmfft_declong.h,
// mtmfft_declong64.h).
#pragma once
#include "spy_common.h"
#include "mtmfft_long.h"

namespace spyfft {

// stats[seg][chan][2 + ntaper] (sum x, sum (n - mid) x, sum w_k x) of the a.nseg segments, for the polynomial removal
// and the post-taper mean.  Both buffers grow as needed; the kernels run only when something will read the sums.
inline int long_stats_pass(hipStream_t stream, const MtmArgs& a, spy::DevBuf<double>& stats, spy::DevBuf<double>& part) {
    const int nz = a.demean_taper ? a.ntaper + 1 : 1;
    if (stats.reserve((size_t)a.nseg * a.nchan * (2 + a.ntaper), stream) ||
        part.reserve((size_t)a.nseg * (a.ntaper + 1) * LONG_SPLITS * a.nchan * 2, stream)) return -2;
    // (constant detrending with the reference-order means of seq_mean_kernel needs no sums of its own)
    if (!((a.detrend >= 0 && !(a.detrend == 0 && a.means)) || a.demean_taper)) return 0;
    if (a.nseg > 65535 || nz * LONG_SPLITS > 65535) { spy::set_error("fft_exec: too many segments / tapers per call"); return -1; }
    hipLaunchKernelGGL(long_stats_kernel, dim3((a.nchan + 63) / 64, a.nseg, nz * LONG_SPLITS), dim3(256), 0, stream, a, part.p, nz);
    hipLaunchKernelGGL(long_stats_final_kernel, dim3((unsigned)(((size_t)a.nseg * a.nchan + 255) / 256)), dim3(256), 0, stream,
                       a, part.p, nz, stats.p);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace spyfft
