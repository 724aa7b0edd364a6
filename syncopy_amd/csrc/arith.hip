// Launcher of the operator arithmetic on data objects (kernels in arith_kernel.h): one launch per call, whatever the
// number of trials.  Every buffer belongs to the caller; nothing here allocates or synchronises.
#include "spy_common.h"
#include "arith_kernel.h"

namespace {

using namespace spyarith;

constexpr size_t TYPE_BYTES[4] = {4, 8, 8, 16};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Launch {
    spyhip_ctx* ctx;
    Args g;
    bool vec;           // every trial starts on a 16-byte boundary of the base (and so of the wider result)
};

template <int OP, int MODE, class A, class T>
void launch(const Launch& l) {
    constexpr int V = 16 / (int)sizeof(A);
    const long long total = l.g.nrows * l.g.width;
    const bool vec = l.vec && V > 1;
    const long long nitem = vec ? (total + V - 1) / V : total;
    long long blocks = (nitem + THREADS - 1) / THREADS;
    if (blocks > l.ctx->limits.elementwise_blocks) blocks = l.ctx->limits.elementwise_blocks;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks)), block(THREADS);
    if (vec)
        hipLaunchKernelGGL((arith_kernel<OP, MODE, A, T, V>), grid, block, 0, l.ctx->stream, l.g);
    else
        hipLaunchKernelGGL((arith_kernel<OP, MODE, A, T, 1>), grid, block, 0, l.ctx->stream, l.g);
}

// the nine base -> result pairs; powers, squares, ones and roots are real
template <int OP, int MODE>
bool launch_types(const Launch& l, int a_type, int out_type) {
    constexpr bool real_only = OP == POW || OP == SQUARE || OP == ONES || OP == SQRT;
    switch (a_type * 4 + out_type) {
        case F32 * 4 + F32: launch<OP, MODE, float, float>(l); return true;
        case F32 * 4 + F64: launch<OP, MODE, float, double>(l); return true;
        case F64 * 4 + F64: launch<OP, MODE, double, double>(l); return true;
        default: break;
    }
    if constexpr (!real_only) {
        switch (a_type * 4 + out_type) {
            case F32 * 4 + C64: launch<OP, MODE, float, cx<float>>(l); return true;
            case F32 * 4 + C128: launch<OP, MODE, float, cx<double>>(l); return true;
            case F64 * 4 + C128: launch<OP, MODE, double, cx<double>>(l); return true;
            case C64 * 4 + C64: launch<OP, MODE, cx<float>, cx<float>>(l); return true;
            case C64 * 4 + C128: launch<OP, MODE, cx<float>, cx<double>>(l); return true;
            case C128 * 4 + C128: launch<OP, MODE, cx<double>, cx<double>>(l); return true;
            default: break;
        }
    }
    return false;
}

// the reflected operators have no second data object; the one-argument operations take no operand at all
template <int OP>
bool launch_mode(const Launch& l, int mode, int a_type, int out_type) {
    constexpr bool unary = OP == SQUARE || OP == COPY || OP == ONES || OP == SQRT;
    if (mode == SCALAR) return launch_types<OP, SCALAR>(l, a_type, out_type);
    if constexpr (!unary) {
        if (mode == BCAST) return launch_types<OP, BCAST>(l, a_type, out_type);
        if constexpr (OP != RSUB && OP != RDIV)
            if (mode == FULL) return launch_types<OP, FULL>(l, a_type, out_type);
    }
    return false;
}

bool launch_op(const Launch& l, int op, int mode, int a_type, int out_type) {
    switch (op) {
        case ADD: return launch_mode<ADD>(l, mode, a_type, out_type);
        case SUB: return launch_mode<SUB>(l, mode, a_type, out_type);
        case MUL: return launch_mode<MUL>(l, mode, a_type, out_type);
        case DIV: return launch_mode<DIV>(l, mode, a_type, out_type);
        case RSUB: return launch_mode<RSUB>(l, mode, a_type, out_type);
        case RDIV: return launch_mode<RDIV>(l, mode, a_type, out_type);
        case POW: return launch_mode<POW>(l, mode, a_type, out_type);
        case SQUARE: return launch_mode<SQUARE>(l, mode, a_type, out_type);
        case COPY: return launch_mode<COPY>(l, mode, a_type, out_type);
        case ONES: return launch_mode<ONES>(l, mode, a_type, out_type);
        case SQRT: return launch_mode<SQRT>(l, mode, a_type, out_type);
        default: return false;
    }
}

}  // namespace

extern "C" int spyhip_arith(spyhip_ctx* ctx, int op, int mode, int a_type, int out_type, const void* a_d, int64_t a_rows,
                            const void* b_d, int64_t b_rows, const int64_t* b_extent, const int64_t* b_stride,
                            double b_re, double b_im, const int64_t* desc, const int64_t* desc_d, int64_t ntrials,
                            int64_t width, const int32_t* chan, const int32_t* chan_d, int64_t nchan_out,
                            int64_t nchan_in, void* out_d, int64_t out_rows) {
    if (!ctx || !a_d || !out_d || !desc || !desc_d || ntrials < 0 || width < 1 || a_rows < 0 || out_rows < 0 ||
        op < 0 || op >= NOPS || mode < SCALAR || mode > FULL || a_type < F32 || a_type > C128 || out_type < F32 ||
        out_type > C128 || (mode != SCALAR && !b_d) || (mode == BCAST && (!b_extent || !b_stride)) ||
        (mode != SCALAR && b_rows < 0) || a_d == out_d || (mode == FULL && b_d == out_d)) {
        spy::set_error("arith: bad argument");
        return -1;
    }
    if (ntrials == 0) return 0;
    if (width > (INT64_MAX >> 5) / (out_rows > 0 ? out_rows : 1) || (!chan != !chan_d)) {
        spy::set_error("arith: %lld rows of %lld elements", (long long)out_rows, (long long)width);
        return -1;
    }
    Launch l;
    l.ctx = ctx;
    Args& g = l.g;
    g.a = a_d; g.b = b_d; g.out = out_d; g.desc = (const long long*)desc_d; g.chan = chan_d;
    g.ntrials = ntrials; g.width = width; g.nchan_out = g.nchan_in = 1;
    g.sre = b_re; g.sim = b_im;
    long long a_width = width;
    if (chan) {                         // the channel axis is the fastest one of a row
        if (nchan_out < 1 || nchan_in < 1 || width % nchan_out != 0 || nchan_in > INT32_MAX ||
            width / nchan_out > (INT64_MAX >> 5) / nchan_in / (a_rows > 0 ? a_rows : 1)) {
            spy::set_error("arith: %lld of %lld channels in rows of %lld elements", (long long)nchan_out,
                           (long long)nchan_in, (long long)width);
            return -1;
        }
        for (int64_t c = 0; c < nchan_out; ++c)
            if (chan[c] < 0 || chan[c] >= nchan_in) { spy::set_error("arith: channel %d of %lld", chan[c], (long long)nchan_in); return -1; }
        g.nchan_out = nchan_out; g.nchan_in = nchan_in;
        a_width = width / nchan_out * nchan_in;
    }
    for (int i = 0; i < 3; ++i) g.ext[i] = 1;
    for (int i = 0; i < 4; ++i) g.str[i] = 0;
    int64_t b_rows_view = 1;            // BCAST: rows of a trial the operand has of its own (1: it broadcasts along them)
    if (mode == BCAST) {
        if (b_extent[0] < 1 || b_extent[1] < 1 || b_extent[2] < 1 || b_extent[3] < 1 ||
            b_extent[1] * b_extent[2] * b_extent[3] != width) {
            spy::set_error("arith: a broadcast view of %lld x %lld x %lld for rows of %lld elements", (long long)b_extent[1],
                           (long long)b_extent[2], (long long)b_extent[3], (long long)width);
            return -1;
        }
        for (int i = 0; i < 4; ++i)
            if (b_stride[i] < 0) { spy::set_error("arith: negative operand stride"); return -1; }
        for (int i = 0; i < 3; ++i) g.ext[i] = b_extent[i + 1];
        for (int i = 0; i < 4; ++i) g.str[i] = b_stride[i];
        b_rows_view = b_stride[0] ? b_extent[0] : 1;
        int64_t last = 0;               // the operand's last element that the view reaches
        for (int i = 0; i < 4; ++i) {
            if (b_stride[i] && b_extent[i] - 1 > (INT64_MAX >> 5) / b_stride[i]) last = INT64_MAX;
            else if (last != INT64_MAX) last += (b_extent[i] - 1) * b_stride[i];
        }
        if (last >= b_rows) {
            spy::set_error("arith: the broadcast view reaches element %lld of %lld", (long long)last, (long long)b_rows);
            return -1;
        }
    }
    // the host copy of the table: every trial inside its tensors, output rows stacked, and what the starts are aligned to
    const int V = (int)(16 / TYPE_BYTES[a_type]);
    bool vec = V > 1 && !chan && aligned16(a_d) && aligned16(out_d) && (mode != FULL || aligned16(b_d)) &&
               (mode != BCAST || g.ext[2] % V == 0);
    int64_t next = desc[0], nrows = 0;
    for (int64_t k = 0; k < ntrials; ++k) {
        const int64_t o = desc[4 * k], a0 = desc[4 * k + 1], b0 = desc[4 * k + 2], n = desc[4 * k + 3];
        if (n < 0 || o != next || o < 0 || a0 < 0 || o > out_rows - n || a0 > a_rows - n ||
            (mode == FULL && (b0 < 0 || b0 > b_rows - n)) || (mode == BCAST && b_rows_view > 1 && n > b_rows_view)) {
            spy::set_error("arith: trial %lld (output row %lld, base row %lld, operand row %lld, %lld rows) does not fit",
                           (long long)k, (long long)o, (long long)a0, (long long)b0, (long long)n);
            return -1;
        }
        next = o + n; nrows += n;
        if (n > 0 && ((o * width) % V || (a0 * a_width) % V || (mode == FULL && (b0 * width) % V))) vec = false;
    }
    if (nrows == 0) return 0;
    g.row0 = desc[0]; g.nrows = nrows;
    l.vec = vec;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (!launch_op(l, op, mode, a_type, out_type)) {
        spy::set_error("arith: operation %d in mode %d from type %d to type %d is not provided", op, mode, a_type, out_type);
        return -1;
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
