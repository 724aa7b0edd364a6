// CPU emulation of the peristimulus-histogram kernels (syncopy_amd/csrc/psth_kernel.h), TEST INFRASTRUCTURE ONLY (see
// hip_emu.h).  Launches the kernels with the grids of psth.hip.  Built by tests/test_psth.py.
#include "hip_emu.h"

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

// the LDS integer add the counting kernels use
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "../../syncopy_amd/csrc/psth_kernel.h"

namespace {
using ll = long long;
unsigned cdiv(ll a, ll b) { return (unsigned)((a + b - 1) / b); }
}  // namespace

extern "C" {

int emu_psth_tiles(int* bin_tile, int* col_tile, int* unit_tile, int* prop_tile, int* threads) {
    *bin_tile = spypsth::BIN_TILE; *col_tile = spypsth::COL_TILE; *unit_tile = spypsth::UNIT_TILE;
    *prop_tile = spypsth::PROP_TILE; *threads = spypsth::THREADS;
    return 0;
}

void emu_psth_presence(const int* chan, const int* unit, const ll* row_lo, const ll* row_hi, ll T, ll max_rows,
                       const unsigned char* chan_ok, ll nchan, const unsigned char* unit_ok, ll nunit,
                       unsigned char* flags) {
    if (T == 0 || max_rows < 1) return;
    ll nblk = (max_rows + 16 * spypsth::THREADS - 1) / (16 * spypsth::THREADS);
    if (nblk > spypsth::MAX_ROW_BLOCKS) nblk = spypsth::MAX_ROW_BLOCKS;
    emu::launch(dim3((unsigned)T, (unsigned)nblk), dim3(spypsth::THREADS), 0, [&] {
        spypsth::psth_presence_kernel(chan, unit, row_lo, row_hi, chan_ok, unit_ok, nchan, nunit, flags);
    });
}

void emu_psth_bin_rows(const ll* sample, const ll* row_lo, const ll* row_hi, const ll* start, const ll* onset, ll T,
                       const double* edges, ll nedges, double samplerate, ll* rows) {
    emu::launch(dim3(cdiv(T * nedges, spypsth::THREADS)), dim3(spypsth::THREADS), 0, [&] {
        spypsth::psth_bin_rows_kernel(sample, row_lo, row_hi, start, onset, T, edges, nedges, samplerate, rows);
    });
}

// returns the number of workgroups
ll emu_psth_count(const int* chan, const int* unit, const ll* rows, const int* lut, ll nchan, ll nunit, const int* lohi,
                  ll T, ll nbins, ll ncols, double scale, float* out) {
    const dim3 grid((unsigned)T, cdiv(nbins, spypsth::BIN_TILE), cdiv(ncols, spypsth::COL_TILE));
    emu::launch(grid, dim3(spypsth::THREADS), 0, [&] {
        spypsth::psth_count_kernel(chan, unit, rows, lut, nchan, nunit, lohi, nbins, ncols, scale, out);
    });
    return (ll)grid.x * grid.y * grid.z;
}

void emu_psth_proportion(const int* chan, const int* unit, const ll* row_lo, const ll* row_hi, const ll* rows,
                         const int* lut, ll nchan, ll nunit, const int* unit_k, const int* col_k, ll nk,
                         const double* edges, ll T, ll nbins, ll ncols, int* S, float* out) {
    emu::launch(dim3((unsigned)T, cdiv(nk, spypsth::UNIT_TILE)), dim3(spypsth::THREADS), 0, [&] {
        spypsth::psth_unit_count_kernel(chan, unit, row_lo, row_hi, rows, lut, unit_k, nchan, nunit, nk, nbins, S);
    });
    emu::launch(dim3((unsigned)T, cdiv(ncols, spypsth::PROP_TILE)), dim3(spypsth::PROP_TILE), 0, [&] {
        spypsth::psth_proportion_kernel(S, col_k, edges, nk, nbins, ncols, out);
    });
}

}  // extern "C"
