// Small fp64 host FFT (iterative radix-2) used once per plan to build filter spectra
// (Bluestein chirp filter, Morlet kernel spectra), and the host tables the plans upload: twiddles, Bluestein tables, taper
// moments, the pre-scaled windows and the frequency map.  Pure functions, no HIP header (tests/test_fft_tables.py).
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace spy {
inline void fft_host(std::vector<double>& re, std::vector<double>& im) {
    const double PI = 3.14159265358979323846264338327950288;
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * PI / (double)len;
        for (size_t k = 0; k < len / 2; ++k) {
            const double wr = std::cos(ang * k), wi = std::sin(ang * k);
            for (size_t i = 0; i < n; i += len) {
                const size_t a = i + k, b = i + k + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr;
                im[b] = im[a] - ti;
                re[a] += tr;
                im[a] += ti;
            }
        }
    }
}

// the first `count` entries of exp(-2 pi i m / n), as float2 or double2
template <class T2>
std::vector<T2> twiddle_table(int n, int count = -1) {
    const double PI = 3.14159265358979323846264338327950288;
    std::vector<T2> t(count < 0 ? n : count);
    for (size_t m = 0; m < t.size(); ++m) {
        const double ang = -2.0 * PI * (double)m / (double)n;
        t[m].x = (decltype(T2::x))std::cos(ang);
        t[m].y = (decltype(T2::x))std::sin(ang);
    }
    return t;
}

// Bluestein: chirp[n] = exp(-i pi n^2 / nfft) and bhat = FFT_M of the wrapped conjugate chirp, / M.  M1 > 0: bhat in the
// [k1][k2] order of a four-step transform with M = M1 x M2.
template <class T2>
void bluestein_tables(int nfft, int M, int M1, std::vector<T2>* chirp, std::vector<T2>* bhat) {
    using T = decltype(T2::x);
    const double PI = 3.14159265358979323846264338327950288;
    chirp->resize(nfft);
    std::vector<double> br(M, 0.0), bi(M, 0.0);
    for (long long n = 0; n < nfft; ++n) {
        const long long m = (n * n) % (2LL * nfft);  // exact phase reduction
        const double ang = PI * (double)m / (double)nfft;
        (*chirp)[n].x = (T)std::cos(ang);
        (*chirp)[n].y = (T)-std::sin(ang);
        br[n] = std::cos(ang);
        bi[n] = std::sin(ang);
        if (n > 0) { br[M - n] = br[n]; bi[M - n] = bi[n]; }
    }
    fft_host(br, bi);
    bhat->resize(M);
    if (M1 <= 0) M1 = M;
    const int M2 = M / M1;
    for (int k1 = 0; k1 < M1; ++k1)
        for (int k2 = 0; k2 < M2; ++k2) {
            const size_t k = (size_t)k1 + (size_t)M1 * k2;
            (*bhat)[(size_t)k1 * M2 + k2].x = (T)(br[k] / M);
            (*bhat)[(size_t)k1 * M2 + k2].y = (T)(bi[k] / M);
        }
}

// [ntaper][2]: sum w_k, sum w_k (n - mid) of the float32 windows (trend removal of the transforms through HBM)
inline std::vector<double> taper_moments(const std::vector<float>& tf, int ntaper, int nsig) {
    std::vector<double> ws((size_t)2 * ntaper);
    const double mid = 0.5 * (nsig - 1);
    for (int k = 0; k < ntaper; ++k) {
        double s0 = 0.0, s1 = 0.0;
        for (int n = 0; n < nsig; ++n) { const double w = tf[(size_t)k * nsig + n]; s0 += w; s1 += w * (n - mid); }
        ws[2 * k] = s0;
        ws[2 * k + 1] = s1;
    }
    return ws;
}

// the windows times scale / 2 (mtmfft_quad_kernel: no scaling left in its epilogue)
inline std::vector<float> taper_half_table(const double* tapers, size_t count, double scale) {
    std::vector<float> th(count);
    for (size_t i = 0; i < count; ++i) th[i] = (float)(tapers[i] * (0.5 * scale));
    return th;
}

// frequency selection -> inverse map bin -> output slot (-1: bin not kept); *ident: every bin, in order.  A selection that
// names a bin outside [0, nf) or twice is refused: empty map, the reason in *err
inline std::vector<int> fpos_map(const int* freq_idx, int nfsel, int nf, bool* ident, std::string* err) {
    std::vector<int> fpos(nf, -1);
    char msg[96];
    *ident = (nfsel == nf);
    for (int i = 0; i < nfsel; ++i) {
        const int f = freq_idx[i];
        if (f < 0 || f >= nf) { std::snprintf(msg, sizeof msg, "freq_idx[%d]=%d outside [0,%d)", i, f, nf); *err = msg; return {}; }
        if (fpos[f] >= 0) { std::snprintf(msg, sizeof msg, "freq_idx holds duplicate bin %d", f); *err = msg; return {}; }
        fpos[f] = i;
        *ident = *ident && (f == i);
    }
    return fpos;
}
}  // namespace spy
