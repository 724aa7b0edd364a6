// C view of the pure route of the tapered FFT (syncopy_amd/csrc/mtmfft_route.h) for tests/test_fft_route.py
// (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include <cstdio>
#include <cstring>

#include "../../syncopy_amd/csrc/mtmfft_route.h"

static void put(char* dst, int cap, const std::string& s) {
    std::snprintf(dst, cap, "%s", s.c_str());
}

extern "C" {

// params: log2n, G, P, M, l1, l2, direct, lds_bytes
int route32(int nsig, int nfft, int nchan, int ntaper, int output, int keeptapers, long long lds_per_block, int force_generic,
            int* family, long long* params, char* name, char* message, int cap) {
    const spyfft::Route r = spyfft::fft_route(nsig, nfft, nchan, ntaper, output, keeptapers, (size_t)lds_per_block, force_generic != 0);
    *family = (int)r.family;
    const long long v[8] = {r.log2n, r.G, r.P, r.M, r.l1, r.l2, r.direct, (long long)r.lds_bytes};
    std::memcpy(params, v, sizeof v);
    put(name, cap, r.kernel_name);
    put(message, cap, r.message);
    return r.err;
}

// params: P, M, blue_M.  The float32 route of the same plan (5 channels, 2 tapers, nsig = nfft) goes in, as in set_precision.
int route64(int nfft, int output, int keeptapers, long long lds_per_block, int force_generic, int* family, long long* params,
            char* name, char* message, int cap) {
    const spyfft::Route f32 = spyfft::fft_route(nfft, nfft, 5, 2, output, keeptapers, (size_t)lds_per_block, force_generic != 0);
    const spyfft::Route64 r = spyfft::fft_route64(nfft, output, keeptapers, f32);
    *family = (int)r.family;
    params[0] = r.P; params[1] = r.M; params[2] = r.blue_M;
    put(name, cap, r.kernel_name);
    put(message, cap, r.message);
    return r.err;
}

// which: 0 DEC_LENGTHS, 1 HALF_LENGTHS, 2 DEC64_LENGTHS; returns the count
int route_table(int which, int* out, int cap) {
    const int* t = which == 0 ? spyfft::DEC_LENGTHS : which == 1 ? spyfft::HALF_LENGTHS : spyfft::DEC64_LENGTHS;
    const int n = which == 0 ? (int)(sizeof spyfft::DEC_LENGTHS / sizeof(int))
                  : which == 1 ? (int)(sizeof spyfft::HALF_LENGTHS / sizeof(int)) : (int)(sizeof spyfft::DEC64_LENGTHS / sizeof(int));
    for (int i = 0; i < n && i < cap; ++i) out[i] = t[i];
    return n;
}
}
