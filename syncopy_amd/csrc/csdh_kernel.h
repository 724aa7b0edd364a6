// K4h - the cross-spectral update for 256 channels on the HALF-PRECISION matrix cores with SPLIT float32 operands:
//
//     acc[f,i,j] += sum_r X[r,f,i] * conj(X[r,f,j])                                  (i >= j at 16-channel granularity)
//
// Reference semantics as csd_kernel.h (connectivity/csd.py:94-102 + the trial sum of
// shared/computational_routine.py:1022-1032).  The float32-input matrix instructions of csd3m_kernel.h run at 1/16 of
// the half-precision rate; this kernel feeds the fast ones without giving up float32-class products:
//
//   * every real number y = x * 2^k(channel) (k from the channel's largest |re|, |im| of the batch, `absmax`, so that
//     |y| < 2^15: a power of two, exact, taken out again in the epilogue) is split ONCE, on its way into LDS, into
//     hi = fp16(y) and lo = fp16(y - hi): hi + lo carries 22 significant bits (|y - hi - lo| <= 2^-22 |y|, or
//     2^-25 absolute where lo is subnormal);
//   * a real product is hi hi' + hi lo' + lo hi' (the dropped lo lo' is <= 2^-22 of it), products exact in the matrix
//     core, float32 accumulation: three v_mfma_f32_16x16x32_f16 (16 cycles, K = 32 rows) where the float32 path needs
//     eight v_mfma_f32_16x16x4_f32 (32 cycles each) - 5.3 x less matrix time per real product;
//   * the complex product is the plain 4-multiplication one (Re = Ar Br + Ai Bi, Im = Ai Br - Ar Bi, each a K-extended
//     sum of the above): 12 instructions per 16 x 16 sub-tile and 32 rows.  The imaginary part is summed directly
//     (no difference of large sums as in the 3-multiplication scheme), so this kernel also serves the phase-exact
//     outputs.  The minus sign costs no operand negation: the Im accumulator changes sign once per chunk between the
//     two product groups (Ai Br first, negate, Ar Bi; the next chunk finds the planes swapped by the loader and so runs
//     the same instructions as Ar Bi first, negate, Ai Br), and the epilogue takes the parity of the chunk count out.
//   * the 16 DIAGONAL sub-tiles (row block = column block) repeat nothing Hermitian symmetry provides: with the fp16
//     planes Rh, Rl, Ih, Il of the block (rows x 16 each) the 12 products are Re = Rh'Rh + Rh'Rl + Rl'Rh + Ih'Ih + Ih'Il
//     + Il'Ih and Im = I'R - R'I, but Rl'Rh = (Rh'Rl)' and R'I = (I'R)'.  Such a tile accumulates
//         S = Rh'Rh + Ih'Ih (2 instructions),  P = Rh'Rl + Ih'Il (2),  M = Ih'Rh + Ih'Rl + Il'Rh (3)
//     - 7 instructions instead of 12, one operand block instead of two - and the epilogue forms Re = S + P + P' and
//     Im = M - M' ONCE (csdh_fold_diagonal: transposes of the 16 x 16 float32 tiles through the LDS the loop has left).
//     S and P do not notice the loader's plane swap; M does (an odd chunk adds R'I = the transpose of what an even one
//     adds), so it changes sign once per chunk like every other Im accumulator: then M - M' is the chunks' sum of
//     (I'R - R'I) up to the same parity of the chunk count.  Re of such a block is symmetric, Im antisymmetric with a
//     zero diagonal, bit for bit.  Per chunk and workgroup: 120 x 12 + 16 x 7 = 1552 matrix instructions (1632 without).
//
// Work decomposition: one 512-thread workgroup per frequency, the 136 lower-triangle sub-tiles dealt to the 8 waves by
// HTab (below).  The two waves of a SIMD have different roles: a MATRIX-HEAVY wave owns 22 off-diagonal sub-tiles (264
// matrix instructions per chunk, 176 accumulator registers) and does nothing else; its partner, a LOADER wave, owns 8
// off-diagonal and 4 diagonal sub-tiles (124 instructions, 112 registers) and brings in the chunk.  A chunk = 32 rows of
// X[., f, :] (64 KiB of spectra): loader L fetches rows 8 L ... 8 L + 7 of all 256 channels in four phases (4 rows x
// the channel pairs 2 lane, 2 lane + 1 of one half of the channels: 16-byte loads, 1 KiB contiguous per wave
// instruction, two phases in flight), splits them in pieces placed between its own matrix instructions, and writes
// half (4 rows) of the 16-byte unit = 8 rows of one channel of one plane per 8 bytes into the layout the fragments are
// read in:
//
//     LDS[buffer][plane: re hi, re lo, im hi, im lo][row group kg = 0..3][channel 0..255][8 rows] fp16
//
// A fragment read (lane l: channel 16 b + l % 16, row group l / 16) is one conflict-free ds_read_b128 whatever the
// block.  Two buffers: chunk c + 1 is converted into the other buffer while chunk c is multiplied; one barrier per
// chunk.
//
// Validity: a channel whose rms at this frequency sits more than 2^18 below the channel's batch-wide peak would see
// lo go subnormal for its TYPICAL value (absolute error 2^-25 against an rms below 2^-3).  The workgroup checks the
// diagonal of what it accumulated (sum |y|^2 >= rows 2^-6 and finite, or 0 for a channel whose range is 0) BEFORE committing; a frequency
// that fails is left untouched and flagged, and the float32 kernel (csd3m_kernel<256, 8> with CsdArgs::only_flagged)
// redoes exactly those.  Non-finite input takes the same route, so NaN / Inf propagate as before.
#pragma once
#include "csd3m_kernel.h"

#ifndef CSDH_FENCE
#define CSDH_FENCE 0x78f    // __builtin_amdgcn_sched_barrier mask behind the loader's fetches: everything but vector memory may cross
#endif
#ifndef CSDH_NH
#define CSDH_NH 22      // off-diagonal sub-tiles of a matrix-heavy wave (a loader wave: 30 - CSDH_NH + its 4 diagonal ones)
#endif
#ifndef CSDH_HEAVY_HI
#define CSDH_HEAVY_HI 0 // 0: waves 0-3 are the matrix-heavy ones and waves 4-7 their loader partners, 1: the other way round
#endif
#ifndef CSDH_PRIO
#define CSDH_PRIO 1     // 1: constant raised priority for the heavy waves, none for the loaders; 0: raised around every sub-tile
#endif

#ifndef CSDH_ABL
#define CSDH_ABL 0      // development ablations (tools/csdh_probe.hip): 1 no global loads, 2 no conversion, 4 no LDS writes,
#endif                  // 8 no fragment reads, 16 no barrier, 32 no negation

#ifdef CSDH_STAMPS
#define CSDH_STAMP(k) do { if (blockIdx.x == 0 && c >= 20 && c < 24) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        const unsigned long long t__ = __builtin_readcyclecounter(); \
        if (lane == 0) a.stamps[((c - 20) * 8 + G) * 8 + (k)] = t__; } } while (0)
#define CSDH_STAMP_HWID() do { if (blockIdx.x == 0 && lane == 0) \
        a.stamps[256 + G] = __builtin_amdgcn_s_getreg(4 | (31 << 11)); } while (0)      /* HW_ID: wave 3:0, SIMD 5:4, CU 11:8 */
#else
#define CSDH_STAMP_HWID() do { } while (0)
#define CSDH_STAMP(k) do { } while (0)
#endif

namespace spycsd {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct CsdhArgs {
    const float2* spec;     // (nrows, F, 256) complex64; 16-BYTE ALIGNED (the loader fetches two channels per lane and load)
    long long nrows;
    int F;
    float2* acc;            // (F, 256, 256) complex64
    const float* absmax;    // [256]: max over the batch of |re|, |im| per channel (>= the true maximum)
    int* flags;             // [F]: 1 = this launch did NOT add frequency f (float32 kernel must), 0 = added
    int f0;                 // block b -> frequency f0 + b
    int nf;                 // frequencies of this launch
    unsigned long long* stamps;   // development timeline (tools/csdh_probe.hip, -DCSDH_STAMPS): [4 chunks][8 waves][8 points] + [8] hardware ids
    long long rs, fs;       // strides (complex elements) between rows and between frequencies: (nrows, F, 256) -> F * 256, 256;
                            // both EVEN, so that every row of every frequency starts 16-byte aligned like `spec`
};

constexpr int CSDH_PLANE = 16 * 1024;                 // 4 row groups x 256 channels x 16 bytes
constexpr int CSDH_BUF = 4 * CSDH_PLANE;              // 32 rows of 256 complex values as fp16 pairs
constexpr int CSDH_LDS_BYTES = 2 * CSDH_BUF + 1024 + 16;   // + the channels' scale exponents + the validity word
constexpr int CSDH_KROWS = 32;

// ---- the deal: which of the 136 lower-triangle sub-tiles (row block, column block; 16 channels each) a wave owns.
// The two waves that share a SIMD (w and w + 4) have different ROLES, so that the non-matrix work of one lies under the
// matrix work of the other:
//   * a MATRIX-HEAVY wave (one per SIMD) owns NH off-diagonal sub-tiles and nothing else: no fetching, no conversion, no
//     LDS writes - 12 NH matrix instructions and its fragment reads per chunk;
//   * a LOADER wave (its partner) fetches, splits and writes the whole chunk's rows 8 L ... 8 L + 7 (L = 0..3) and owns
//     30 - NH off-diagonal sub-tiles + FOUR diagonal ones (7 instructions each).
// NH = 20: 240 matrix instructions against 10 x 12 + 4 x 7 = 148; NH = 22 (the default, the fastest measured:
// profiles/k4h_roles_probe.txt): 264 against 124; 388 per SIMD and chunk whatever NH.
// The 96 sub-tiles that lie in full rows of the 4-block column strips {0-3}, {4-7}, {8-11} (rows below the strip's own
// triangle) are put in a sequence (strip, row block, column block): heavy wave h takes the h-th run of NH - at NH = 20 rows
// 4-8 and 9-13 of strip 0 (5 x 4 rectangles), rows 14-15 of strip 0 + 8-10 of strip 1, rows 11-15 of strip 1 - and each
// column block is fetched once, each row block twice (HPlan).  Loader L takes 1 / 4 of what is left of the sequence (at
// NH = 20: row 12 + L of strip 2), the 6 sub-tiles below the diagonal of blocks 4 L ... 4 L + 3 and those 4 diagonal ones:
// its triangle's operands are its diagonal sub-tiles' operands.
template <int NH_ = CSDH_NH>
struct HTabT {
    static constexpr int NH = NH_, NLO = 30 - NH_, NDL = 4;      // off-diagonal sub-tiles heavy / loader, diagonal ones of a loader
    static constexpr int NTMAX = NH > NLO + NDL ? NH : NLO + NDL;
    static_assert(NH >= 17 && NH <= 24 && (96 - 4 * NH) % 4 == 0, "the heavy runs come out of the 96 full-row sub-tiles");
    static constexpr bool heavy(int g) { return CSDH_HEAVY_HI ? g >= 4 : g < 4; }
    static constexpr int idx(int g) { return g & 3; }                         // h of a heavy wave, L of a loader: the SIMD
    static constexpr int nt(int g) { return heavy(g) ? NH : NLO + NDL; }      // sub-tiles of wave g
    static constexpr int nd(int g) { return heavy(g) ? 0 : NDL; }             // ... of which diagonal
    struct Gen { int ta[8][NTMAX], tb[8][NTMAX]; };
    static constexpr Gen make() {
        int sr[96] = {}, sc[96] = {};
        int m = 0;
        for (int s = 0; s < 3; ++s)
            for (int r = 4 * (s + 1); r < 16; ++r)
                for (int c = 4 * s; c < 4 * s + 4; ++c) { sr[m] = r; sc[m] = c; ++m; }
        Gen g{};
        constexpr int per = (96 - 4 * NH) / 4;
        for (int w = 0; w < 8; ++w) {
            const int i = idx(w);
            int n = 0;
            if (heavy(w)) {
                for (int k = 0; k < NH; ++k) { g.ta[w][n] = sr[i * NH + k]; g.tb[w][n] = sc[i * NH + k]; ++n; }
            } else {
                for (int k = 0; k < per; ++k) { g.ta[w][n] = sr[4 * NH + i * per + k]; g.tb[w][n] = sc[4 * NH + i * per + k]; ++n; }
                for (int r = 4 * i; r < 4 * i + 4; ++r)
                    for (int c = 4 * i; c < r; ++c) { g.ta[w][n] = r; g.tb[w][n] = c; ++n; }
                for (int d = 4 * i; d < 4 * i + 4; ++d) { g.ta[w][n] = d; g.tb[w][n] = d; ++n; }
            }
        }
        return g;
    }
    static constexpr Gen T = make();
    static constexpr int ta(int g, int t) { return T.ta[g][t]; }       // row block (0..15) of sub-tile t of wave g
    static constexpr int tb(int g, int t) { return T.tb[g][t]; }       // column block
    static constexpr bool diag(int g, int t) { return T.ta[g][t] == T.tb[g][t]; }
    static constexpr int didx(int g, int t) {                          // a diagonal sub-tile's place among the wave's
        int d = 0;
        for (int u = 0; u < t; ++u) d += diag(g, u) ? 1 : 0;
        return d;
    }
    // every sub-tile on or below the diagonal exactly once; nd(w) diagonal ones in wave w; one wave of either role per SIMD
    static constexpr bool complete() {
        int seen[16][16] = {};
        for (int w = 0; w < 8; ++w) {
            int nd_ = 0;
            for (int t = 0; t < nt(w); ++t) {
                if (T.ta[w][t] < T.tb[w][t] || T.ta[w][t] > 15 || T.tb[w][t] < 0) return false;
                ++seen[T.ta[w][t]][T.tb[w][t]];
                nd_ += diag(w, t) ? 1 : 0;
            }
            if (nd_ != nd(w)) return false;
            if (w < 4 && heavy(w) == heavy(w + 4)) return false;
        }
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c <= r; ++c)
                if (seen[r][c] != 1) return false;
        return true;
    }
};
using HTab = HTabT<>;       // (a template so that its table is built where it is first used: after the class is complete)
static_assert(HTab::complete(), "the deal of K4h's sub-tiles");

// ---- per-wave schedule: the order of the wave's sub-tiles and which fragment slot every operand block sits in.
// Two A slots (ping-pong: the next row block lands while the current one is multiplied), two B slots; a diagonal
// sub-tile has ONE operand block: it is looked for (and fetched) among the B slots if the wave otherwise uses the block
// as a column block only, among the A slots if not.  Sub-tiles are walked column pair by column pair: a heavy wave's run
// of full rows of a 4-block column strip (5 rows x 4 columns, or two pieces of two neighbouring strips) then loads each
// column block once and each row block twice; a loader's triangle finds its operands among those of its diagonal
// sub-tiles.
template <int G>
struct HPlan {
    using TAB = HTab;
    static constexpr int NT = TAB::nt(G);
    struct P {
        int tile[NT];       // walk order -> index into TAB::ta / tb
        int ablk[NT], bblk[NT];      // block indices (0..15) of the operands
        int aslot[NT], bslot[NT];
        bool aload[NT], bload[NT];   // the operand is fetched for this step (else it is still in its slot)
        bool diag[NT], dinb[NT];     // diagonal sub-tile; ... whose one operand is B[bslot] (else A[aslot])
    };
    static constexpr bool column_only(int x) {       // block x: a column block, never a row block, of the other sub-tiles
        bool col = false;
        for (int t = 0; t < NT; ++t) {
            if (TAB::diag(G, t)) continue;
            if (TAB::ta(G, t) == x) return false;
            col = col || TAB::tb(G, t) == x;
        }
        return col;
    }
    static constexpr P make() {
        P p{};
        int key[NT] = {};
        for (int t = 0; t < NT; ++t) {
            p.tile[t] = t;
            key[t] = (TAB::tb(G, t) >> 1) * 256 + TAB::ta(G, t) * 16 + TAB::tb(G, t);
        }
        for (int i = 1; i < NT; ++i)            // insertion sort by (column pair, row block, column block)
            for (int j = i; j > 0 && key[j] < key[j - 1]; --j) {
                int k = key[j]; key[j] = key[j - 1]; key[j - 1] = k;
                int u = p.tile[j]; p.tile[j] = p.tile[j - 1]; p.tile[j - 1] = u;
            }
        int ac[2] = {-1, -1}, bc[2] = {-1, -1};
        int alast = 1, blast = 1;               // slot used by the previous step (the other one is the victim)
        for (int s = 0; s < NT; ++s) {
            const int t = p.tile[s];
            const int x = TAB::ta(G, t), y = TAB::tb(G, t);
            p.ablk[s] = x;
            p.bblk[s] = y;
            p.diag[s] = x == y;
            p.dinb[s] = x == y && column_only(x);
            p.aslot[s] = alast; p.aload[s] = false;
            p.bslot[s] = blast; p.bload[s] = false;
            if (!p.dinb[s]) {
                if (ac[0] == x) { p.aslot[s] = 0; }
                else if (ac[1] == x) { p.aslot[s] = 1; }
                else { p.aslot[s] = 1 - alast; p.aload[s] = true; ac[1 - alast] = x; }
                alast = p.aslot[s];
            }
            if (!p.diag[s] || p.dinb[s]) {
                if (bc[0] == y) { p.bslot[s] = 0; }
                else if (bc[1] == y) { p.bslot[s] = 1; }
                else { p.bslot[s] = 1 - blast; p.bload[s] = true; bc[1 - blast] = y; }
                blast = p.bslot[s];
            }
        }
        return p;
    }
    static constexpr P T = make();
};

// scale exponent of a channel: y = x * 2^k with |y| < 2^15 for every |x| <= absmax
__device__ __forceinline__ int csdh_exponent(float absmax) {
    const int e = (int)((__float_as_uint(absmax) >> 23) & 0xffu);    // biased exponent; 0 for zero / subnormal
    int k = 141 - e;                                                  // 14 - (e - 127)
    return k > 127 ? 127 : k;                                         // (e = 255, Inf / NaN: k = -114, the data decide)
}

// Between two sub-tiles, and around every piece of other work placed inside one, the instruction order is pinned: left
// to interleave two sub-tiles the compiler runs out of registers in a heavy wave, and it moves a loader's conversion
// out from under the matrix instructions into one block.  (CSDH_PRIO 0: the priority is raised around every sub-tile
// as before the waves had roles; 1: the heavy wave raised it once, csdh_wave.)
__device__ __forceinline__ void csdh_tile_begin() { __builtin_amdgcn_sched_barrier(0); if (!CSDH_PRIO) __builtin_amdgcn_s_setprio(1); }
__device__ __forceinline__ void csdh_tile_end() { if (!CSDH_PRIO) __builtin_amdgcn_s_setprio(0); __builtin_amdgcn_sched_barrier(0); }
struct CsdhNoWork { __device__ __forceinline__ void operator()(int) const {} };

// One sub-tile, 32 rows: X / Y = [plane 0 hi, plane 0 lo, plane 1 hi, plane 1 lo] fragments of the row / column block.
// Re += P0 P0' + P1 P1'; Im: first group P1 P0', then the accumulator changes sign, then P0 P1' (see the header: with the
// planes (re, im) in even and (im, re) in odd chunks this is Ai Br - Ar Bi up to the parity of the chunk count).
// work(0 ... 3): a loader wave's conversion pieces, issued in the shadow of the matrix instruction in front of them.
template <class W>
__device__ __forceinline__ void csdh_tile(const f16x8 (&X)[4], const f16x8 (&Y)[4], f32x4& re, f32x4& im, W&& work) {
    csdh_tile_begin();
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], Y[0], im, 0, 0, 0);
    work(0);
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], Y[1], im, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[3], Y[0], im, 0, 0, 0);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], Y[0], re, 0, 0, 0);
    work(1);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], Y[1], re, 0, 0, 0);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[1], Y[0], re, 0, 0, 0);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], Y[2], re, 0, 0, 0);
    work(2);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], Y[3], re, 0, 0, 0);
    re = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[3], Y[2], re, 0, 0, 0);
    if (!(CSDH_ABL & 32)) im = -im;
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], Y[2], im, 0, 0, 0);
    work(3);
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], Y[3], im, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[1], Y[2], im, 0, 0, 0);
    csdh_tile_end();
}

// One DIAGONAL sub-tile, 32 rows: X = the fragments of its one block.  S += P0h'P0h + P1h'P1h, P += P0h'P0l + P1h'P1l (the
// same whichever of the planes is the real part); M += P1'P0 without the lo lo' term, then M changes sign like `im`
// above: even chunks add Ih'R.. = I'R, odd ones R'I = its transpose to the negated sum, so that M - M' (the epilogue's)
// is the sum over the chunks of I'R - R'I up to the sign (-1)^chunks.
template <class W>
__device__ __forceinline__ void csdh_diag_tile(const f16x8 (&X)[4], f32x4& s, f32x4& p, f32x4& m, W&& work) {
    csdh_tile_begin();
    m = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], X[0], m, 0, 0, 0);
    work(0);
    m = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], X[1], m, 0, 0, 0);
    m = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[3], X[0], m, 0, 0, 0);
    work(1);
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], X[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], X[2], s, 0, 0, 0);
    work(2);
    p = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[0], X[1], p, 0, 0, 0);
    work(3);
    p = __builtin_amdgcn_mfma_f32_16x16x32_f16(X[2], X[3], p, 0, 0, 0);
    if (!(CSDH_ABL & 32)) m = -m;
    csdh_tile_end();
}

// Step s of wave G's walk on the fragment slots A, B: re / im = the accumulators of the wave's sub-tiles (a diagonal
// one keeps S in re and M in im), pd = P of its diagonal sub-tiles (one unused entry in a wave that has none).
constexpr int csdh_npd(int g) { return HTab::nd(g) ? HTab::nd(g) : 1; }
template <int G, int s, class W = CsdhNoWork>
__device__ __forceinline__ void csdh_step(const f16x8 (&A)[2][4], const f16x8 (&B)[2][4], f32x4 (&re)[HTab::nt(G)],
                                          f32x4 (&im)[HTab::nt(G)], f32x4 (&pd)[csdh_npd(G)], W&& work = W()) {
    using PL = HPlan<G>;
    constexpr int t = PL::T.tile[s];
    if constexpr (PL::T.diag[s]) {
        const f16x8(&X)[4] = PL::T.dinb[s] ? B[PL::T.bslot[s]] : A[PL::T.aslot[s]];
        csdh_diag_tile(X, re[t], pd[HTab::didx(G, t)], im[t], work);
    } else {
        csdh_tile(A[PL::T.aslot[s]], B[PL::T.bslot[s]], re[t], im[t], work);
    }
}

// After the last chunk (and the barrier behind it: the operand buffers are free), for the diagonal sub-tiles of wave G:
// re <- S + P + P', im <- M - M'.  The transposes go through `ts`, 16 x 17 floats of LDS that belong to this wave.  Lane
// l holds column l & 15 and rows 4 (l >> 4) + r of a tile.  (S + S') / 2 is S wherever the matrix core gave S[i][j] and
// S[j][i] the same bits, and symmetric by construction in any case.
template <int G>
__device__ __forceinline__ void csdh_fold_diagonal(f32x4 (&re)[HTab::nt(G)], f32x4 (&im)[HTab::nt(G)], f32x4 (&pd)[csdh_npd(G)],
                                                   float* ts, int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
    auto transposed = [&](const f32x4& v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ts[(4 * lq + r) * 17 + l15] = v[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = ts[l15 * 17 + 4 * lq + r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // read before the next tile overwrites it
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        return o;
    };
    m3_for<0, HTab::nt(G)>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if constexpr (HTab::diag(G, t)) {
            constexpr int d = HTab::didx(G, t);
            const f32x4 st = transposed(re[t]), pt = transposed(pd[d]), mt = transposed(im[t]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                re[t][r] = 0.5f * (re[t][r] + st[r]) + (pd[d][r] + pt[r]);
                im[t][r] = im[t][r] - mt[r];
            }
        }
    });
}

// After the last chunk: validity of the frequency, then acc += sub-tile / (2^k_i 2^k_j).  `kexp(channel)` = the scale
// exponent the operands were split with; `ts`: see csdh_fold_diagonal.
template <int G, class KEXP>
__device__ __forceinline__ void csdh_finish(const CsdhArgs& a, f32x4 (&re)[HTab::nt(G)], f32x4 (&im)[HTab::nt(G)],
                                            f32x4 (&pd)[csdh_npd(G)], float* ts, int nchunk, int f, int lane, int* vword, KEXP kexp) {
    using TAB = HTab;
    constexpr int NT = TAB::nt(G);
    const int l15 = lane & 15, lq = lane >> 4;
    const long long nrows = a.nrows;
    csdh_fold_diagonal<G>(re, im, pd, ts, lane);       // from here on a diagonal sub-tile holds Re and Im like any other
    // ---- the Im accumulators carry the sign (-1)^nchunk relative to (even chunks) Im = Ai Br - Ar Bi ... :
    // even chunk: planes (re, im): first group = Ai Br (+), then negated, + Ar Bi  ->  -(I + Ai Br - Ar Bi)
    // odd chunk:  planes (im, re): first group = Ar Bi added to -(I...), negated -> I... - Ar Bi, + Ai Br
    const float isign = (nchunk & 1) ? -1.f : 1.f;

    // ---- validity of the frequency: the diagonal of the scaled accumulation (the diagonal sub-tiles of the table: four in
    // every loader wave, none in a heavy one, which only joins the barrier below)
    {
        const float floor2 = (float)nrows * 0.015625f;            // rms^2 >= 2^-6 in scaled units
        bool bad = false;
        m3_for<0, NT>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            if constexpr (TAB::diag(G, t)) {
                // an all-zero diagonal entry is only innocent for a channel that IS zero (a scale of 2^-114 for an
                // Inf "maximum" would flush a whole channel to zero otherwise)
                const bool dead = a.absmax[TAB::ta(G, t) * 16 + l15] == 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * lq + r == l15) {
                        const float v = re[t][r];
                        bad = bad || !((v >= floor2 && v < __builtin_inff()) || (v == 0.f && dead));
                    }
            }
        });
        if (__any(bad) && lane == 0) *vword = 0;
    }
    __syncthreads();
    const bool valid = *vword != 0;
    if (a.flags && G == 0 && lane == 0) a.flags[f] = valid ? 0 : 1;
    if (!valid) return;

    // ---- acc += sub-tile / (2^k_i 2^k_j).  Lane l holds column (l & 15) and rows 4 (l >> 4) + r of the 16 x 16 block.
    m3_for<0, NT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr int bi = TAB::ta(G, t), bj = TAB::tb(G, t);
        static_assert(bi >= bj, "a sub-tile lies on or below the diagonal");
        float2* const pb = a.acc + (size_t)f * 65536 + (size_t)(bi * 16 + 4 * lq) * 256 + bj * 16 + l15;
        const int kj = kexp(bj * 16 + l15);
        float2 old[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) old[r] = pb[(size_t)r * 256];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = -(kexp(bi * 16 + 4 * lq + r) + kj);
            pb[(size_t)r * 256] = make_float2(old[r].x + ldexpf(re[t][r], kk), old[r].y + ldexpf(isign * im[t][r], kk));
        }
    });
}

constexpr int csdh_cpoint(int nt, int ph) { return ((2 * ph + 1) * nt) / 8; }      // step of a loader's walk under which phase ph is converted
constexpr int csdh_cphase(int nt, int s) {
    for (int ph = 0; ph < 4; ++ph)
        if (csdh_cpoint(nt, ph) == s) return ph;
    return -1;
}

template <int G>
__device__ __forceinline__ void csdh_wave(const CsdhArgs& a, char* lds, int f, int lane) {
    using TAB = HTab;
    using PL = HPlan<G>;
    constexpr int NT = TAB::nt(G), NPD = csdh_npd(G);
    constexpr bool LOADER = !TAB::heavy(G);
    constexpr int KG = TAB::idx(G);                   // a loader wave converts rows 8 KG ... 8 KG + 7 of ALL 256 channels
    const int l15 = lane & 15, lq = lane >> 4;
    int* const kexp = reinterpret_cast<int*>(lds + 2 * CSDH_BUF);          // [256] scale exponents
    int* const vword = reinterpret_cast<int*>(lds + 2 * CSDH_BUF + 1024);  // validity of the frequency
    CSDH_STAMP_HWID();

    // ---- scales of this lane's four loader channels: 128 h + 2 lane + k (h, k = 0, 1)
    float sc00 = 0.f, sc01 = 0.f, sc10 = 0.f, sc11 = 0.f;
    if constexpr (LOADER) {
        const int k00 = csdh_exponent(a.absmax[2 * lane]), k01 = csdh_exponent(a.absmax[2 * lane + 1]);
        const int k10 = csdh_exponent(a.absmax[128 + 2 * lane]), k11 = csdh_exponent(a.absmax[129 + 2 * lane]);
        sc00 = __uint_as_float((unsigned)(k00 + 127) << 23); sc01 = __uint_as_float((unsigned)(k01 + 127) << 23);
        sc10 = __uint_as_float((unsigned)(k10 + 127) << 23); sc11 = __uint_as_float((unsigned)(k11 + 127) << 23);
        if (KG == 0) { kexp[2 * lane] = k00; kexp[2 * lane + 1] = k01; kexp[128 + 2 * lane] = k10; kexp[129 + 2 * lane] = k11; }
    }
    if (G == 0 && lane == 0) *vword = 1;

    const long long nrows = a.nrows;
    const int nchunk = (int)((nrows + CSDH_KROWS - 1) / CSDH_KROWS);
    const size_t rowstride = (size_t)a.rs;                            // float2 elements between rows

    // ---- loader: phase ph = rows 8 KG + 4 (ph / 2) ... + 3 of the channel PAIRS 128 (ph % 2) + 2 lane, + 1: 16-byte
    // loads, 1 KiB contiguous per wave instruction (8-byte loads fetch at ~0.6 of that rate per CU, and the fetch rate,
    // not the matrix pipe, is what a chunk waited for: profiles/ROUND_LOGS.md).  TWO phases in flight (staging set
    // ph & 1, 2 x 16 registers): with one, the four requests of a chunk wait for memory one after the other.
    // Everything that is not a matrix instruction competes with the matrix instructions of BOTH waves of the SIMD for its one issue
    // port, so the common case - all 32 rows of the chunk exist - is kept lean: row addresses = one scalar pointer per
    // chunk + i row strides, two v_fma_mix per value for the split (product with the scale, rounding to fp16 and packing
    // in one instruction; the residual the same way), no per-row selects.  Only the last one or two chunks of a launch
    // take the general path (rows past the end are fetched from the last row and given the scale 0).
    f32x4 stg[2][4];
    const int nrows_i = (int)nrows;                  // (the host keeps launches below 2^31 rows)
    const int nfull = nrows_i / CSDH_KROWS;          // chunks whose 32 rows all exist
    const char* const gb = reinterpret_cast<const char*>(a.spec) + (size_t)f * a.fs * 8;       // wave-uniform
    const size_t rowbytes = rowstride * 8;
    const unsigned voff = (unsigned)lane * 16u;
    const char* nextp = gb + (size_t)(8 * KG) * rowbytes;            // rows 8 KG ... of the chunk AFTER the one multiplied
    auto fetch = [&](const char* cp, int c, int ph) {                // cp: rows 8 KG ... of chunk c, if c < nfull
        f32x4(&st)[4] = stg[ph & 1];
        const int rh = ph >> 1, ch = ph & 1;
        if (c < nfull) {                                             // (uniform)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (CSDH_ABL & 1) st[i] = f32x4{(float)(i + lane), (float)(c - lane), (float)(i - lane), (float)(c + lane)};
                else if ((CSDH_ABL & 128) && c > 2) asm volatile("" : "+v"(st[i]));      // keep the (real) values of chunk 2
                else {
                    // the row's address stays a scalar pair (global_load with an SGPR base and the lane's 32-bit offset):
                    // left alone, the compiler folds i * rowbytes + voff into 64-bit VECTOR offsets that live
                    // across the whole loop - registers the accumulators need
                    typedef const __attribute__((address_space(1))) char gchar;          // (global memory, said out loud:
                    typedef const __attribute__((address_space(1))) f32x4 gf32x4;       // behind the asm nothing infers it)
                    gchar* rowp = (gchar*)(cp + (4 * rh + i) * rowbytes);
                    asm("" : "+s"(rowp));
                    st[i] = *(gf32x4*)(rowp + voff + 1024 * ch);
                }
            }
        } else {
            const long long r0 = (long long)c * CSDH_KROWS + 8 * KG + 4 * rh;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long r = r0 + i < nrows ? r0 + i : nrows - 1;
                st[i] = *reinterpret_cast<const f32x4*>(gb + (size_t)r * rowbytes + 1024 * ch + voff);
            }
        }
    };
    // One PIECE of a phase's conversion = one channel k = j / 2 and row pair i = j % 2 of the staged values: (hi, lo) fp16
    // pairs of re and im of rows 2 i and 2 i + 1, packed (row 2 i in the low halves): hi = fp16(x s), lo = fp16(x s - hi),
    // two v_fma_mix per value (product with the scale, rounding and packing in one instruction; the residual the same
    // way), re and im alternating so that no instruction waits for the one in front of it.  A row past the end of the
    // spectra (last chunk only) was fetched from the last row and gets the scale 0 - if that row holds Inf / NaN the
    // product is NaN, in channels that the row itself has already made non-finite.
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 cv[2][4];                                  // [channel k][re hi, re lo, im hi, im lo][row pair]
    auto piece = [&](int c, int ph, int j) {
        const f32x4(&st)[4] = stg[ph & 1];
        const int rhalf = ph >> 1, ch = ph & 1, k = j >> 1, i = j & 1;
        const float sc = ch == 0 ? (k == 0 ? sc00 : sc01) : (k == 0 ? sc10 : sc11);
        float sa = sc, sb = sc;
        if (c >= nfull) {                            // (uniform)
            const long long r0 = (long long)c * CSDH_KROWS + 8 * KG + 4 * rhalf + 2 * i;
            sa = r0 < nrows ? sc : 0.f;
            sb = r0 + 1 < nrows ? sc : 0.f;
        }
        unsigned rh, rl, ih, il;
        if (CSDH_ABL & 2) {
            rh = rl = __float_as_uint(st[2 * i][2 * k]); ih = il = __float_as_uint(st[2 * i + 1][2 * k + 1]);
        } else {
            asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\t"
                "v_fma_mixlo_f16 %2, %6, %8, 0\n\t"
                "v_fma_mixhi_f16 %0, %5, %9, 0\n\t"
                "v_fma_mixhi_f16 %2, %7, %9, 0\n\t"
                "v_fma_mixlo_f16 %1, %4, %8, -%0 op_sel_hi:[0,0,1]\n\t"
                "v_fma_mixlo_f16 %3, %6, %8, -%2 op_sel_hi:[0,0,1]\n\t"
                "v_fma_mixhi_f16 %1, %5, %9, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
                "v_fma_mixhi_f16 %3, %7, %9, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                : "=&v"(rh), "=&v"(rl), "=&v"(ih), "=&v"(il)
                : "v"(st[2 * i][2 * k]), "v"(st[2 * i + 1][2 * k]), "v"(st[2 * i][2 * k + 1]), "v"(st[2 * i + 1][2 * k + 1]), "v"(sa), "v"(sb));
        }
        cv[k][0][i] = rh; cv[k][1][i] = rl; cv[k][2][i] = ih; cv[k][3][i] = il;
    };
    // ... and behind its four pieces the phase's 8 LDS writes: chunk c lives in buffer c & 1 with the planes (re, im) in the
    // order (c & 1) ? (im, re) : (re, im); a phase fills half (4 rows = 8 bytes) of the 16-byte units of its two channels
    // in each plane
    auto flush = [&](int c, int ph) {
        const int rhalf = ph >> 1, ch = ph & 1;
        const int odd = c & 1;
        char* const w = lds + odd * CSDH_BUF + KG * 4096 + (128 * ch + 2 * lane) * 16 + 8 * rhalf;
        char* const wr = w + (odd ? 2 * CSDH_PLANE : 0);
        char* const wi = w + (odd ? 0 : 2 * CSDH_PLANE);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (CSDH_ABL & 4) {
                if (cv[k][0][0] + cv[k][1][1] + cv[k][2][0] + cv[k][3][1] == 123456u) *reinterpret_cast<u32x2*>(wr) = cv[k][0];
                continue;
            }
            *reinterpret_cast<u32x2*>(wr + 16 * k) = cv[k][0];
            *reinterpret_cast<u32x2*>(wr + 16 * k + CSDH_PLANE) = cv[k][1];
            *reinterpret_cast<u32x2*>(wi + 16 * k) = cv[k][2];
            *reinterpret_cast<u32x2*>(wi + 16 * k + CSDH_PLANE) = cv[k][3];
        }
    };
    auto convert = [&](int c, int ph) {
#pragma unroll
        for (int j = 0; j < 4; ++j) piece(c, ph, j);
        flush(c, ph);
    };

    f32x4 re[NT], im[NT], pd[NPD];               // (a diagonal sub-tile: S in re, M in im, P in pd)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { re[t][r] = 0.f; im[t][r] = 0.f; }
#pragma unroll
    for (int d = 0; d < NPD; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) pd[d][r] = 0.f;

    if constexpr (LOADER) {                      // chunk 0, and the first two phases of chunk 1 on their way
        fetch(nextp, 0, 0);
        fetch(nextp, 0, 1);
        convert(0, 0);
        fetch(nextp, 0, 2);
        convert(0, 1);
        fetch(nextp, 0, 3);
        convert(0, 2);
        convert(0, 3);
        nextp += (size_t)CSDH_KROWS * rowbytes;
        fetch(nextp, 1, 0);
        fetch(nextp, 1, 1);
        __builtin_amdgcn_sched_barrier(CSDH_FENCE);
    }
    __syncthreads();

    // fragment slots: [plane 0 hi, plane 0 lo, plane 1 hi, plane 1 lo]
    f16x8 A[2][4], B[2][4];
    unsigned rb = (unsigned)(lq * 4096 + l15 * 16);          // this lane's fragment base in the current buffer
    bool nofrag = false;
    auto ldfrag = [&](f16x8 (&dst)[4], int blk) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (CSDH_ABL & 8) {
                asm volatile("" : "+v"(dst[p]));            // keep the registers alive, read nothing
                continue;
            }
            if ((CSDH_ABL & 64) && nofrag) continue;        // real operand bits, fetched in the first chunk only
            dst[p] = *reinterpret_cast<const f16x8*>(lds + rb + p * CSDH_PLANE + blk * 256);
        }
    };
    // a loader's four conversions go behind the steps csdh_cpoint() of its walk; each frees its staging set for the
    // request of the phase after next (phases 0 and 1 were requested during the previous chunk)
    static_assert(csdh_cpoint(NT, 0) < csdh_cpoint(NT, 1) && csdh_cpoint(NT, 1) < csdh_cpoint(NT, 2) &&
                  csdh_cpoint(NT, 2) < csdh_cpoint(NT, 3) && csdh_cpoint(NT, 3) < NT, "four conversion points in the walk");

    // the matrix instructions of the heavy wave go ahead of its partner's vector work, all the time
    if (CSDH_PRIO && !LOADER) __builtin_amdgcn_s_setprio(1);
    for (int c = 0; c < nchunk; ++c) {
        CSDH_STAMP(0);
        if constexpr (PL::T.aload[0]) ldfrag(A[PL::T.aslot[0]], PL::T.ablk[0]);
        if constexpr (PL::T.bload[0]) ldfrag(B[PL::T.bslot[0]], PL::T.bblk[0]);
        m3_for<0, NT>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            // operands of the next step land while this one multiplies
            if constexpr (s + 1 < NT) {
                if constexpr (PL::T.aload[s + 1]) ldfrag(A[PL::T.aslot[s + 1]], PL::T.ablk[s + 1]);
                if constexpr (PL::T.bload[s + 1]) ldfrag(B[PL::T.bslot[s + 1]], PL::T.bblk[s + 1]);
            }
            constexpr int cph = LOADER ? csdh_cphase(NT, s) : -1;       // the phase converted under this step, or -1
            if constexpr (cph < 0) {
                csdh_step<G, s>(A, B, re, im, pd);
            } else {
                if constexpr (cph == 0) CSDH_STAMP(2);
                if constexpr (cph == 3) CSDH_STAMP(5);
                csdh_step<G, s>(A, B, re, im, pd, [&](int j) {
                    __builtin_amdgcn_sched_barrier(0);
                    piece(c + 1, cph, j);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
            if constexpr (s == 0) CSDH_STAMP(1);
            if constexpr (LOADER) {
                // (the last iterations convert rows that do not exist into the idle buffer: zeros)
                m3_for<0, 4>([&](auto pc) {
                    constexpr int ph = decltype(pc)::value;
                    if constexpr (s == csdh_cpoint(NT, ph)) {
                        if constexpr (ph == 0) CSDH_STAMP(3);
                        flush(c + 1, ph);
                        if constexpr (ph < 2) {
                            fetch(nextp, c + 1, ph + 2);
                        } else {
                            if constexpr (ph == 2) nextp += (size_t)CSDH_KROWS * rowbytes;
                            fetch(nextp, c + 2, ph - 2);
                        }
                        __builtin_amdgcn_sched_barrier(CSDH_FENCE);
                        if constexpr (ph == 0) CSDH_STAMP(4);
                        if constexpr (ph == 3) CSDH_STAMP(6);
                    }
                });
            }
        });
        CSDH_STAMP(7);
        if (!(CSDH_ABL & 16)) __syncthreads();
        if (CSDH_ABL & 64) nofrag = true;
        rb ^= (unsigned)CSDH_BUF;
    }
    if (CSDH_PRIO && !LOADER) __builtin_amdgcn_s_setprio(0);

    // (behind the loop's last barrier nobody reads or writes the operand buffers any more: 2 KiB of them per wave for
    // the epilogue's transposes)
    csdh_finish<G>(a, re, im, pd, reinterpret_cast<float*>(lds + G * 2048), nchunk, f, lane, vword, [&](int ch) { return kexp[ch]; });
}

template <int G0, int G1>
__device__ __forceinline__ void csdh_dispatch(int g, const CsdhArgs& a, char* lds, int f, int lane) {
    if constexpr (G0 + 1 == G1) {
        csdh_wave<G0>(a, lds, f, lane);
    } else {
        constexpr int GM = (G0 + G1) / 2;
        if (g < GM) csdh_dispatch<G0, GM>(g, a, lds, f, lane);
        else csdh_dispatch<GM, G1>(g, a, lds, f, lane);
    }
}

__global__ void __launch_bounds__(512) SPY_M3_KATTR(8) csdh_kernel(CsdhArgs a) {
    SPY_DYN_SMEM(char, lds);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = a.f0 + (int)blockIdx.x;
    csdh_dispatch<0, 8>(wave, a, lds, f, lane);
}

// max over a batch of spectra of |re|, |im| per channel (the kernels of mtmfft.hip deliver it for free; this pass is for
// spectra that come from somewhere else): out[c] = max(out[c], ...), bit pattern compare (non-negative floats)
__global__ void __launch_bounds__(256) csdh_absmax_kernel(const float4* __restrict__ spec, long long nquads, int C,
                                                          unsigned* __restrict__ out) {
    // a thread walks elements of constant channel pair: stride = multiple of C / 2 float4s
    __shared__ unsigned sm[512];
    for (int i = threadIdx.x; i < 512; i += 256) sm[i] = 0u;
    __syncthreads();
    const long long per = C / 2;                                  // float4 (two channels) per (row, frequency)
    const long long stride = (long long)gridDim.x * 256;
    float m0 = 0.f, m1 = 0.f;
    long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cp = (int)(q % per);                                // stride is a multiple of `per` (host: grid * 256 % per == 0)
    for (; q < nquads; q += stride) {
        const float4 v = spec[q];
        m0 = fmaxf(m0, fmaxf(fabsf(v.x), fabsf(v.y)));
        m1 = fmaxf(m1, fmaxf(fabsf(v.z), fabsf(v.w)));
        // NaN: fmaxf drops it - a NaN / Inf spectrum fails the validity check of csdh_kernel instead
    }
    atomicMax(&sm[2 * cp], __float_as_uint(m0));
    atomicMax(&sm[2 * cp + 1], __float_as_uint(m1));
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256)
        if (sm[i]) atomicMax(&out[i], sm[i]);
}

}  // namespace spycsd
