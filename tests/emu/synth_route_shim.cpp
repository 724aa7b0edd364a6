// C view of the pure route of the synthetic-data kernels (syncopy_amd/csrc/synth_route.h) for tests/test_synth.py
// (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include "../../syncopy_amd/csrc/synth_route.h"

using namespace spysyn;

extern "C" {

// out: {coupled, table in LDS, threads of a workgroup, workgroups, LDS bytes, entries of the table}; returns 0, or -1 where
// the launcher would refuse the arguments, with the reason in *err
int sr_ar2(long long ntrials, long long nsamples, long long nchan, const int32_t* rowptr, const int32_t* col,
           long long lds_per_block, long long* out, const char** err) {
    const Ar2Route r = ar2_route(ntrials, nsamples, nchan, rowptr, col, (size_t)lds_per_block);
    *err = r.err;
    if (r.err) return -1;
    out[0] = r.coupled; out[1] = r.csr_in_lds; out[2] = r.block; out[3] = r.grid; out[4] = (long long)r.lds_bytes; out[5] = r.nnz;
    return 0;
}

// out: {threads of a workgroup, workgroups}
int sr_phase(long long ntrials, long long nsamples, long long nchan, long long* out, const char** err) {
    const SeriesRoute r = phase_route(ntrials, nsamples, nchan);
    *err = r.err;
    if (r.err) return -1;
    out[0] = r.block; out[1] = r.grid;
    return 0;
}

// out: {lane bytes, lanes, workgroups}
int sr_tile(long long ntrials, long long nsamples, long long nchan, unsigned long long out_addr, long long max_blocks,
            long long* out, const char** err) {
    const TileRoute r = tile_route(ntrials, nsamples, nchan, out_addr, max_blocks);
    *err = r.err;
    if (r.err) return -1;
    out[0] = r.lane_bytes; out[1] = r.lanes; out[2] = r.grid;
    return 0;
}

int sr_max_channels() { return MAX_CHAN; }

}  // extern "C"
