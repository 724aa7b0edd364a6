// C view of the pure route of the channel concatenation (syncopy_amd/csrc/concat_route.h) for tests/test_concat.py and
// tests/test_gpu_concat.py (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include "../../syncopy_amd/csrc/concat_route.h"

using namespace spycat;

extern "C" {

// out: {lane bytes, lanes on 16-byte boundaries, elements of an output line, first output row, rows, cum[0 .. 8]}; returns
// 0, or -1 where the launcher would refuse the arguments, with the reason in *err
int cr_route(int elem_bytes, int nsrc, const int64_t* src_rows, const int64_t* run, long long pre, const int64_t* desc,
             long long ntrials, const unsigned long long* src_addr, unsigned long long out_addr, long long out_rows,
             long long* out, const char** err) {
    uint64_t addr[MAX_SRC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < nsrc && s < MAX_SRC; ++s) addr[s] = src_addr[s];
    const Route r = concat_route(elem_bytes, nsrc, src_rows, run, pre, desc, ntrials, addr, out_addr, out_rows);
    *err = r.err;
    if (r.err) return -1;
    out[0] = r.lane_bytes; out[1] = r.lane_aligned; out[2] = r.w; out[3] = r.row0; out[4] = r.nrows;
    for (int s = 0; s <= MAX_SRC; ++s) out[5 + s] = r.cum[s];
    return 0;
}

int cr_max_sources() { return MAX_SRC; }

}  // extern "C"
