// C view of the pure route of the data selection (syncopy_amd/csrc/select_route.h) for tests/test_select.py and
// tests/test_gpu_select.py (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include "../../syncopy_amd/csrc/select_route.h"

using namespace spysel;

extern "C" {

// out: {mode, lane bytes, lanes on 16-byte boundaries, run elements, output row elements, source row elements, n[3], s[3],
// start[3], loff[3], index entries}; returns 0, or -1 where the launcher would refuse the arguments
int sr_route(int elem_bytes, long long src_rows, long long out_rows, const int64_t* extent, const int32_t* kind,
             const int64_t* start, const int64_t* count, const int32_t* idx, const int64_t* desc, long long ntrials,
             unsigned long long src_addr, unsigned long long out_addr, long long* out) {
    const Route r = select_route(elem_bytes, src_rows, out_rows, extent, kind, start, count, idx, desc, ntrials, src_addr,
                                 out_addr);
    if (r.err) return -1;
    out[0] = r.mode; out[1] = r.lane_bytes; out[2] = r.lane_aligned; out[3] = r.run; out[4] = r.wo; out[5] = r.ws;
    for (int i = 0; i < 3; ++i) { out[6 + i] = r.n[i]; out[9 + i] = r.s[i]; out[12 + i] = r.start[i]; out[15 + i] = r.loff[i]; }
    out[18] = r.nidx;
    return 0;
}

long long sr_lds_cap() { return LDS_CAP; }

}  // extern "C"
