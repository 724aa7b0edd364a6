// Small fp64 host FFT (iterative radix-2) used once per plan to build filter spectra
// (Bluestein chirp filter, Morlet kernel spectra), the twiddle tables and the Bluestein tables the plans upload.
#pragma once
#include <cmath>
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
}  // namespace spy
