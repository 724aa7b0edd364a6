// NumPy's NaN-skipping summation orders, shared by the mean kernels (api.hip) and the other summary statistics
// (stats_kernel.h).
#pragma once

// element k of a run with NaNs replaced by zero as np.nanmean does before it sums (pofs != 0: complex data - the element
// counts as NaN if either component is)
__device__ __forceinline__ float nan0(const float* a, long long idx, long long pofs) {
    const float v = a[idx];
    if (pofs == 0) return (v != v) ? 0.f : v;
    const float w = a[idx + pofs];
    return ((v != v) || (w != w)) ? 0.f : v;
}

// NumPy's float32 sum of n values that are contiguous in memory (pairwise_sum_FLOAT: eight running sums over blocks of
// at most 128 values, halves of longer runs added recursively) - followed literally so that means over the LAST axis
// agree with the reference to the last bit whenever its divide does
__device__ float np_pairwise_sum(const float* a, long long n) {
    if (n < 8) {
        float res = 0.f;
        for (long long i = 0; i < n; ++i) res = __fadd_rn(res, nan0(a, i, 0));
        return res;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = nan0(a, j, 0);
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], nan0(a, i + j, 0));
        float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                              __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
        for (; i < n; ++i) res = __fadd_rn(res, nan0(a, i, 0));
        return res;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return __fadd_rn(np_pairwise_sum(a, n2), np_pairwise_sum(a + n2, n - n2));
}

// one component of m complex values (interleaved floats): pairwise_sum_CFLOAT on 2m floats - fewer than 4 complex: plain
// loop; up to 64: this component's four running sums r[c], r[c+2], r[c+4], r[c+6]; longer: halves (multiples of 4)
__device__ float np_pairwise_sum_c(const float* a, long long m, long long pofs) {
    if (m < 4) {
        float r = 0.f;
        for (long long k = 0; k < m; ++k) r = __fadd_rn(r, nan0(a, 2 * k, pofs));
        return r;
    }
    if (m <= 64) {
        float r[4];
        for (int j = 0; j < 4; ++j) r[j] = nan0(a, 2 * j, pofs);
        long long k = 4;
        for (; k < m - (m % 4); k += 4)
            for (int j = 0; j < 4; ++j) r[j] = __fadd_rn(r[j], nan0(a, 2 * (k + j), pofs));
        float res = __fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3]));
        for (; k < m; ++k) res = __fadd_rn(res, nan0(a, 2 * k, pofs));
        return res;
    }
    long long m2 = m / 2;
    m2 -= m2 % 4;
    return __fadd_rn(np_pairwise_sum_c(a, m2, pofs), np_pairwise_sum_c(a + 2 * m2, m - m2, pofs));
}
