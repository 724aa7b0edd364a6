// Kernels of the operator arithmetic on data objects (datatype/arithmetic.py): out = a (op) b, element by element, over
// the selected trials of a data object.  One family, memory-bound: the operation, the operand mode, the base's type, the
// result's type and the access width are template parameters, so that pow's registers stay out of add and the index
// arithmetic of a broadcast operand out of a scalar one.
//
// Addressing.  The output rows of one launch follow each other (the trials are stacked in selection order); a row has
// `width` elements.  Trial k of the launch owns the output rows [desc[4k], desc[4k] + desc[4k + 3]), reads the base from
// row desc[4k + 1] on and a full-tensor operand from row desc[4k + 2] on: any trial order, repeats and latency windows
// are rows of this table and nothing else.  A workgroup takes a contiguous range of the launch's items (V elements each)
// and its threads walk it side by side; a thread looks its trial up by binary search only when it leaves the trial it
// was in.  All index arithmetic is int64.
#pragma once
#include <cstdint>

namespace spyarith {

constexpr int THREADS = 256;

enum Op { ADD = 0, SUB, MUL, DIV, RSUB, RDIV, POW, SQUARE, COPY, ONES, SQRT, NOPS };
enum Mode { SCALAR = 0, BCAST, FULL };
enum Type { F32 = 0, F64, C64, C128 };

template <class R> struct cx { R re, im; };
template <class T> struct real_of { using type = T; };
template <class R> struct real_of<cx<R>> { using type = R; };
template <class T> struct is_cx { static constexpr bool value = false; };
template <class R> struct is_cx<cx<R>> { static constexpr bool value = true; };

// V elements that travel together: 16 bytes of the base, 16 ... 64 bytes of the result
template <class E, int N>
struct alignas(sizeof(E) * N >= 16 ? 16 : sizeof(E) * N) Pack { E v[N]; };

struct Args {
    const void* a;              // base tensor (rows x a_width elements)
    const void* b;              // BCAST: the operand array, FULL: the operand tensor (rows x width), both of the result type
    void* out;                  // result tensor (rows x width)
    const long long* desc;      // (ntrials, 4): output row, base row, operand row, rows
    const int* chan;            // channel selection of the base (nchan_out indices < nchan_in), or nullptr
    long long ntrials, row0, nrows, width, nchan_out, nchan_in;
    long long ext[3];           // BCAST: a trial is (rows, ext[0], ext[1], ext[2]), ext[0] * ext[1] * ext[2] = width
    long long str[4];           // BCAST: the operand's element stride along each of the four axes, 0 where it broadcasts
    double sre, sim;            // SCALAR: the operand
};

// ---- arithmetic in the result type -----------------------------------------------------------------------------------
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }
// the correctly rounded float32 root through float64 (53 >= 2 * 24 + 2 bits: the second rounding is the right one);
// __fsqrt_rn may lower to the hardware's approximate v_sqrt_f32
__device__ __forceinline__ float sqrt_rn(float a) { return (float)__dsqrt_rn((double)a); }
__device__ __forceinline__ double sqrt_rn(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ float abs_of(float a) { return fabsf(a); }
__device__ __forceinline__ double abs_of(double a) { return fabs(a); }
// float32 powers through float64: the rounding of pow's own error (below 1 float64 ulp) to float32 is all that is left
__device__ __forceinline__ float pow_of(float a, float b) { return (float)pow((double)a, (double)b); }
__device__ __forceinline__ double pow_of(double a, double b) { return pow(a, b); }

template <class T, class A> struct Conv { static __device__ __forceinline__ T of(A a) { return (T)a; } };
template <class R, class A> struct Conv<cx<R>, A> { static __device__ __forceinline__ cx<R> of(A a) { return cx<R>{(R)a, (R)0}; } };
template <class R, class Q> struct Conv<cx<R>, cx<Q>> {
    static __device__ __forceinline__ cx<R> of(cx<Q> a) { return cx<R>{(R)a.re, (R)a.im}; }
};

template <class T> struct Scalar { static __device__ __forceinline__ T of(double re, double) { return (T)re; } };
template <class R> struct Scalar<cx<R>> { static __device__ __forceinline__ cx<R> of(double re, double im) { return cx<R>{(R)re, (R)im}; } };

// NumPy's complex quotient (Smith's method, the branch on the larger component of the divisor)
template <class R>
__device__ __forceinline__ cx<R> cdiv(cx<R> x, cx<R> y) {
    const R ar = abs_of(y.re), ai = abs_of(y.im);
    if (ar >= ai) {
        if (ar == (R)0 && ai == (R)0) return cx<R>{div_rn(x.re, ar), div_rn(x.im, ar)};
        const R rat = div_rn(y.im, y.re), scl = div_rn((R)1, y.re + y.im * rat);
        return cx<R>{(x.re + x.im * rat) * scl, (x.im - x.re * rat) * scl};
    }
    const R rat = div_rn(y.re, y.im), scl = div_rn((R)1, y.im + y.re * rat);
    return cx<R>{(x.re * rat + x.im) * scl, (x.im * rat - x.re) * scl};
}

template <int OP, class T> struct Apply {                   // real result
    static __device__ __forceinline__ T of(T a, T b) {
        if constexpr (OP == ADD) return a + b;
        else if constexpr (OP == SUB) return a - b;
        else if constexpr (OP == MUL) return a * b;
        else if constexpr (OP == DIV) return div_rn(a, b);
        else if constexpr (OP == RSUB) return b - a;
        else if constexpr (OP == RDIV) return div_rn(b, a);
        else if constexpr (OP == POW) return pow_of(a, b);
        else if constexpr (OP == SQUARE) return a * a;
        else if constexpr (OP == ONES) return (T)1;
        else if constexpr (OP == SQRT) return sqrt_rn(a);
        else return a;
    }
};
template <int OP, class R> struct Apply<OP, cx<R>> {        // complex result: + - * / and the copy
    static __device__ __forceinline__ cx<R> of(cx<R> a, cx<R> b) {
        if constexpr (OP == ADD) return cx<R>{a.re + b.re, a.im + b.im};
        else if constexpr (OP == SUB) return cx<R>{a.re - b.re, a.im - b.im};
        else if constexpr (OP == RSUB) return cx<R>{b.re - a.re, b.im - a.im};
        else if constexpr (OP == MUL) return cx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
        else if constexpr (OP == DIV) return cdiv(a, b);
        else if constexpr (OP == RDIV) return cdiv(b, a);
        else return a;
    }
};

// a / b for 0 <= a, 0 < b: the 32-bit division where both fit
__device__ __forceinline__ long long idiv(long long a, long long b) {
    if ((((unsigned long long)a | (unsigned long long)b) >> 32) == 0) return (long long)((unsigned)a / (unsigned)b);
    return a / b;
}

// the last trial whose first output row is <= row (trials without rows share their row with the one that follows)
__device__ __forceinline__ long long find_trial(const long long* desc, long long n, long long row) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (desc[4 * mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// V = 16 / sizeof(A) elements per item when every trial starts on an item boundary in all three tensors (the launcher
// checks that on the host table), else V = 1; only the V = 1 instance serves a channel selection.  The last item of the
// launch may be short: it goes element by element.
template <int OP, int MODE, class A, class T, int V>
__global__ __launch_bounds__(THREADS) void arith_kernel(const Args g) {
    const A* __restrict__ a = reinterpret_cast<const A*>(g.a);
    const T* __restrict__ b = reinterpret_cast<const T*>(g.b);
    T* __restrict__ out = reinterpret_cast<T*>(g.out);
    const long long total = g.nrows * g.width;
    const long long nitem = (total + V - 1) / V;
    long long per = (nitem + gridDim.x - 1) / gridDim.x;
    per = (per + THREADS - 1) / THREADS * THREADS;
    const long long lo = (long long)blockIdx.x * per;
    const long long hi = lo + per < nitem ? lo + per : nitem;
    const long long a_width = g.chan ? g.width / g.nchan_out * g.nchan_in : g.width;
    const T s = Scalar<T>::of(g.sre, g.sim);
    long long t_out = 0, t_rows = 0, t_a = 0, t_b = 0;           // the trial this thread is in: none yet
    for (long long it = lo + threadIdx.x; it < hi; it += THREADS) {
        const long long e = it * V;
        const long long rrow = idiv(e, g.width), col = e - rrow * g.width, row = g.row0 + rrow;
        if (row < t_out || row >= t_out + t_rows) {
            const long long k = find_trial(g.desc, g.ntrials, row);
            t_out = g.desc[4 * k]; t_a = g.desc[4 * k + 1]; t_b = g.desc[4 * k + 2]; t_rows = g.desc[4 * k + 3];
        }
        const long long r = row - t_out;                          // row inside the trial
        const long long oi = row * g.width + col;
        long long ai = (t_a + r) * a_width + col;
        if (V == 1 && g.chan) {
            const long long q = idiv(col, g.nchan_out);
            ai = (t_a + r) * a_width + q * g.nchan_in + g.chan[col - q * g.nchan_out];
        }
        long long bi = 0, bstep = 0;
        if constexpr (MODE == FULL) { bi = (t_b + r) * g.width + col; bstep = 1; }
        if constexpr (MODE == BCAST) {
            const long long q2 = idiv(col, g.ext[2]), i3 = col - q2 * g.ext[2];
            const long long i1 = idiv(q2, g.ext[1]), i2 = q2 - i1 * g.ext[1];
            bi = r * g.str[0] + i1 * g.str[1] + i2 * g.str[2] + i3 * g.str[3];
            bstep = g.str[3];                                     // (V divides ext[2]: an item stays on the last axis)
        }
        if (V == 1 || e + V > total) {
            const long long n = total - e < V ? total - e : V;
            for (long long j = 0; j < n; ++j) {
                const T x = Conv<T, A>::of(a[ai + j]);
                const T y = MODE == SCALAR ? s : b[bi + j * bstep];
                out[oi + j] = Apply<OP, T>::of(x, y);
            }
            continue;
        }
        const Pack<A, V> xa = *reinterpret_cast<const Pack<A, V>*>(a + ai);
        Pack<T, V> y, res;
        if constexpr (MODE == FULL) y = *reinterpret_cast<const Pack<T, V>*>(b + bi);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if constexpr (MODE == SCALAR) y.v[j] = s;
            if constexpr (MODE == BCAST) y.v[j] = b[bi + j * bstep];
            res.v[j] = Apply<OP, T>::of(Conv<T, A>::of(xa.v[j]), y.v[j]);
        }
        *reinterpret_cast<Pack<T, V>*>(out + oi) = res;
    }
}

}  // namespace spyarith
