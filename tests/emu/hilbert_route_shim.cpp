// C entry to syncopy_amd/csrc/hilbert_route.h for tests/test_hilbert.py: the route of a trial length as plain values.
#include <cstring>

#include "../../syncopy_amd/csrc/hilbert_route.h"

extern "C" {

// returns the route's error code; family: 0 COPY, 1 PACKED, 2 BLUE, 3 ANY64; text (>= 256 bytes): the kernel name, or
// the refusal message
int hilbert_route_query(long long nsamp, int* family, int* M, int* log2n, int* G, int* threads, long long* lds_bytes,
                        int* bluestein, int* max_radix, char* text) {
    const spyhil::Route r = spyhil::hilbert_route(nsamp);
    *family = (int)r.family;
    *M = r.M; *log2n = r.log2n; *G = r.G; *threads = r.threads; *lds_bytes = (long long)r.lds_bytes;
    *bluestein = r.bluestein ? 1 : 0;
    int big = 0;
    for (int i = 0; i < r.plan.nfac; ++i) big = r.plan.radix[i] > big ? r.plan.radix[i] : big;
    *max_radix = big;
    std::snprintf(text, 256, "%s", r.err ? r.message.c_str() : r.kernel_name.c_str());
    return r.err;
}

int hilbert_weight_query(int k, int N) { return spyhil::hilbert_weight(k, N); }

void hilbert_grid_query(long long ntrials, int nchan, int G, int* npg, int* S, int* ncl, unsigned* grid) {
    const spyhil::PackedGrid g = spyhil::packed_grid(ntrials, nchan, G);
    *npg = g.npg; *S = g.S; *ncl = g.ncl; *grid = g.grid;
}

}  // extern "C"
