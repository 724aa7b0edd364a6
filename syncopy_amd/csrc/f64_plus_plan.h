// Factor schedule of the any-radix complex128 Stockham passes (f64_stockham.h).  Plain C++: the pure route of the tapered
// FFT (mtmfft_route.h) shares it with the kernels.
#pragma once

namespace spywil {

constexpr int PO_MAXFAC = 24;
struct PlusPlan {
    int L, nfac;
    int radix[PO_MAXFAC];
};

// factors of L in the order the passes take them: 4, 2, 3, 5, 7, 11, 13, then the remaining primes
inline bool plus_plan(int L, PlusPlan* pl) {
    pl->L = L;
    int k = 0, n = L;
    static const int cand[] = {4, 2, 3, 5, 7, 11, 13};
    for (int c : cand)
        while (n % c == 0 && n > 1) { if (k >= PO_MAXFAC) return false; pl->radix[k++] = c; n /= c; }
    for (int p = 17; n > 1; p += 2)
        while (n % p == 0) { if (k >= PO_MAXFAC) return false; pl->radix[k++] = p; n /= p; }
    pl->nfac = k;
    return true;
}

}  // namespace spywil
