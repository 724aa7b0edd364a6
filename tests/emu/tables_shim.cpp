// C view of the host table builders of the tapered FFT (syncopy_amd/csrc/host_fft.h) for tests/test_fft_tables.py
// (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include <cstdio>
#include <cstring>

#include "../../syncopy_amd/csrc/host_fft.h"

namespace {
struct f2 { float x, y; };
struct d2 { double x, y; };
}  // namespace

extern "C" {

// out: [ntaper][2]
void shim_taper_moments(const float* tf, int ntaper, int nsig, double* out) {
    const std::vector<double> w = spy::taper_moments(std::vector<float>(tf, tf + (size_t)ntaper * nsig), ntaper, nsig);
    std::memcpy(out, w.data(), w.size() * sizeof(double));
}

void shim_taper_half(const double* tapers, long long count, double scale, float* out) {
    const std::vector<float> t = spy::taper_half_table(tapers, (size_t)count, scale);
    std::memcpy(out, t.data(), t.size() * sizeof(float));
}

// returns 0 and fills fpos[nf], *ident; or -1 with the refusal in message
int shim_fpos_map(const int* freq_idx, int nfsel, int nf, int* fpos, int* ident, char* message, int cap) {
    bool id = false;
    std::string err;
    const std::vector<int> m = spy::fpos_map(freq_idx, nfsel, nf, &id, &err);
    std::snprintf(message, cap, "%s", err.c_str());
    if (!err.empty()) return -1;
    std::memcpy(fpos, m.data(), m.size() * sizeof(int));
    *ident = id ? 1 : 0;
    return 0;
}

// chirp[nfft][2], bhat[M][2] as float32 (wide = 0) or float64 (wide = 1)
void shim_bluestein(int nfft, int M, int M1, int wide, void* chirp, void* bhat) {
    if (wide) {
        std::vector<d2> c, b;
        spy::bluestein_tables(nfft, M, M1, &c, &b);
        std::memcpy(chirp, c.data(), c.size() * sizeof(d2));
        std::memcpy(bhat, b.data(), b.size() * sizeof(d2));
    } else {
        std::vector<f2> c, b;
        spy::bluestein_tables(nfft, M, M1, &c, &b);
        std::memcpy(chirp, c.data(), c.size() * sizeof(f2));
        std::memcpy(bhat, b.data(), b.size() * sizeof(f2));
    }
}

// the first `count` entries of exp(-2 pi i m / n) as float32
void shim_twiddles(int n, int count, float* out) {
    const std::vector<f2> t = spy::twiddle_table<f2>(n, count);
    std::memcpy(out, t.data(), t.size() * sizeof(f2));
}
}
