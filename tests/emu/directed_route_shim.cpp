// C view of the pure route of spyhip_directed_norm (syncopy_amd/csrc/directed_route.h) for tests/test_directed.py
// (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include "../../syncopy_amd/csrc/directed_route.h"

using namespace spydir;

extern "C" {

// out: {ok, cached, kc, strips, grid, threads, lds, row stride of the tile in doubles}
void dr_norm(int n, int nfreq, unsigned long long lds_per_block, long long* out) {
    const NormRoute r = norm_route(n, nfreq, (size_t)lds_per_block);
    out[0] = r.ok; out[1] = r.cached; out[2] = r.kc; out[3] = r.strips; out[4] = r.grid; out[5] = r.threads;
    out[6] = (long long)r.lds; out[7] = r.ok ? norm_ld(r.kc) : 0;
}

int dr_const(int which) {
    const int c[4] = {DL, DT, DW, DKC};
    return c[which];
}

}  // extern "C"
