/*
 * spyhip.h - C ABI of the MI355X (gfx950) spectral-estimation / cross-spectral
 * connectivity hot path.
 *
 * This is the drop-in boundary underneath Syncopy's `computeFunction` plug-in
 * surface (reference: syncopy/shared/computational_routine.py:51-1108 and the
 * cF contract in doc/source/developer/compute_kernels.rst:63-88).  The
 * reference has no native code; every entry point below names the reference
 * *Python* function whose arithmetic it replaces.  Python binds this header
 * through ctypes (syncopy_amd/backend.py); INTEGRATION.md shows the stub a
 * Syncopy maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; spyhip_last_error()
 *    returns a thread-local message for the last failure;
 *  - pointers suffixed `_d` are DEVICE pointers (HBM), all others are host
 *    pointers that are consumed before the call returns;
 *  - all work is enqueued on the context's HIP stream (spyhip_ctx_set_stream),
 *    nothing synchronises unless stated; caller owns every buffer;
 *  - complex64 = interleaved (re, im) float pairs, complex128 = double pairs;
 *  - trial data live in ONE (rows x ld) float32 matrix, channel fastest, as
 *    AnalogData does (syncopy/datatype/continuous_data.py:405); a "segment" is
 *    `nsig` consecutive rows starting at `seg_start[b]` of which only rows in
 *    [seg_lo[b], seg_hi[b]) are read (others count as 0.0f - this is the zero
 *    extension of stft.py:101-117); a trial is the segment
 *    start=lo=sampleinfo[t,0], hi=sampleinfo[t,1].
 */
#ifndef SPYHIP_H
#define SPYHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spyhip_ctx spyhip_ctx;
typedef struct spyhip_fft_plan spyhip_fft_plan;
typedef struct spyhip_cwt_plan spyhip_cwt_plan;
typedef struct spyhip_queue spyhip_queue;
typedef struct spyhip_hilbert_plan spyhip_hilbert_plan;

/* output conversions = syncopy/shared/const_def.py:25-37 `spectralConversions` */
enum spyhip_output {
    SPYHIP_OUT_POW = 0,
    SPYHIP_OUT_ABS = 1,
    SPYHIP_OUT_FOURIER = 2, /* complex64 ("fourier" / "complex") */
    SPYHIP_OUT_REAL = 3,
    SPYHIP_OUT_IMAG = 4,
    SPYHIP_OUT_ANGLE = 5,
    SPYHIP_OUT_ABSREAL = 6,
    SPYHIP_OUT_ABSIMAG = 7
};

/* polynomial removal before tapering = scipy.signal.detrend call sites
 * specest/compRoutines.py:169-172, connectivity/ST_compRoutines.py:405-409,
 * per segment in specest/stft.py:131-132 */
enum spyhip_detrend { SPYHIP_DETREND_NONE = -1, SPYHIP_DETREND_CONSTANT = 0, SPYHIP_DETREND_LINEAR = 1 };

/* ---- context ------------------------------------------------------------ */
int spyhip_version(void);
const char* spyhip_last_error(void);
int spyhip_ctx_create(int device, spyhip_ctx** ctx);
int spyhip_ctx_destroy(spyhip_ctx* ctx);
/* `stream` is a hipStream_t (NULL = the null stream) */
/* Give back the device memory a context keeps between calls (split-launch scratch, the work arrays of spyhip_granger). */
int spyhip_ctx_trim(spyhip_ctx* ctx);
int spyhip_ctx_set_stream(spyhip_ctx* ctx, void* stream);
int spyhip_ctx_synchronize(spyhip_ctx* ctx);

/* ---- device memory ---------------------------------------------------------
 * The library can be driven from a host that has nothing but this header (NumPy + ctypes, C, ...): it allocates
 * HBM, moves data and synchronises by itself.  Hosts that already own device memory (PyTorch tensors) pass their
 * pointers instead - the two can be mixed freely.  Copies are enqueued on the context's stream and are complete
 * when the call returns (the stream is synchronised). */
int spyhip_alloc(spyhip_ctx* ctx, size_t bytes, void** ptr_d);
int spyhip_free(spyhip_ctx* ctx, void* ptr_d);
int spyhip_memset(spyhip_ctx* ctx, void* ptr_d, int value, size_t bytes);            /* asynchronous */
int spyhip_upload(spyhip_ctx* ctx, void* dst_d, const void* src, size_t bytes);
int spyhip_download(spyhip_ctx* ctx, void* dst, const void* src_d, size_t bytes);

/* ---- the in-HBM trial queue -------------------------------------------------
 * Replaces the per-trial HDF5 slab reads of ComputationalRoutine.compute_sequential
 * (shared/computational_routine.py:1001-1007) and the trial bookkeeping of AnalogData
 * (datatype/continuous_data.py:255,405; sampleinfo: datatype/base_data.py:993): the whole (nrows x nchan) float32
 * matrix goes to HBM once, together with the trials' row ranges.  Trial t = rows
 * [sampleinfo[2t], sampleinfo[2t+1]) - any order, overlaps and repeats allowed, exactly as given (integer work).
 * spyhip_queue_segments hands out the device arrays spyhip_fft_exec / spyhip_cwt_exec take as
 * seg_start_d (= seg_lo_d) and seg_hi_d. */
int spyhip_queue_upload(spyhip_ctx* ctx, const float* data, int64_t nrows, int nchan, const int64_t* sampleinfo,
                        int ntrials, spyhip_queue** queue);
int spyhip_queue_destroy(spyhip_queue* queue);
const float* spyhip_queue_data(const spyhip_queue* queue);            /* device pointer, ld = nchan */
int spyhip_queue_segments(const spyhip_queue* queue, const int64_t** start_d, const int64_t** stop_d, int* ntrials);

/* ---- C1: sums over ranks (RCCL) ---------------------------------------------
 * Replaces the mutex-guarded `+=` of the reference's parallel trial map (shared/kwarg_decorators.py:723-735,
 * shared/computational_routine.py:939-942): one process per GPU, each with the accumulator of its trial shard.
 * Bootstrap: ONE rank calls spyhip_comm_unique_id, the host distributes the 128 bytes by any means it has (file,
 * environment, MPI, a torch.distributed store ...), every rank calls spyhip_comm_init with the same id.  RCCL
 * (librccl.so) is loaded on first use; single-GPU users never need it.
 * spyhip_allreduce_csd: acc_d complex64 (nfreq, nchan, nchan) raw accumulator of spyhip_csd_accumulate; only its
 *   lower triangle carries data, so that is what travels (packed into library scratch, summed over all ranks,
 *   unpacked): 0.54 GB instead of 1.07 GB at 2049 x 256 x 256.
 * spyhip_allreduce: in-place sum of n float32 (dtype 0) or float64 (dtype 1) values (phasor sums of K7, the
 *   jackknife sums, trial sums of averaged spectra; complex arrays as interleaved reals).
 * All are enqueued on the context's stream.  With a communicator of one rank they run all the same (identity). */
#define SPYHIP_UNIQUE_ID_BYTES 128
int spyhip_comm_unique_id(void* id_out);
int spyhip_comm_init(spyhip_ctx* ctx, const void* id, int rank, int nranks);
int spyhip_comm_destroy(spyhip_ctx* ctx);
int spyhip_comm_info(const spyhip_ctx* ctx, int* rank, int* nranks);     /* -1 if there is no communicator */
int spyhip_allreduce_csd(spyhip_ctx* ctx, void* acc_d, int nfreq, int nchan);
int spyhip_allreduce(spyhip_ctx* ctx, void* buf_d, int64_t n, int dtype);

/* ---- K1/K2: (multi-)tapered FFT of segments ------------------------------
 * Replaces mtmfft (specest/mtmfft.py:16-129) + the tail of mtmfft_cF
 * (specest/compRoutines.py:169-189), and, with nsig == nfft == nperseg and
 * one segment per frame, stft/mtmconvol (specest/stft.py:16-159,
 * specest/mtmconvol.py:136-150).
 *
 *   X[b,k,f,c] = scale * sum_{n<nsig} w[k,n] * x_b[n,c] * exp(-2 pi i f n / nfft)
 *
 * tapers : K x nsig float64, already normalised as _norm_taper
 *          (specest/_norm_spec.py:27-46); scale as _norm_spec (:10-24).
 * detrend: enum spyhip_detrend, applied per segment to the (zero-extended)
 *          nsig samples; demean_taper: subtract the per-channel mean again
 *          after tapering (mtmfft.py:115-116).
 * freq_idx: nfsel indices into the nfft/2+1 rfft bins (NULL = all bins);
 *          duplicates must already be squashed (shared/tools.py:334-336).
 * output  : enum spyhip_output; keeptapers=0 averages the converted values
 *          over tapers (compRoutines.py:188-189).
 * Result  : (B, Kout, nfsel, nchan) float32 or complex64, Kout = keeptapers ? K : 1.
 */
int spyhip_fft_plan_create(spyhip_ctx* ctx, int nsig, int nfft, int nchan, int ntaper,
                           const double* tapers, double scale, int detrend, int demean_taper,
                           const int32_t* freq_idx, int nfsel, int output, int keeptapers,
                           spyhip_fft_plan** plan);
int spyhip_fft_plan_destroy(spyhip_fft_plan* plan);
/* data_d: float32 (rows x ld); chan_idx_d: nchan column indices or NULL
 * (=0..nchan-1); seg_*_d: B int64 each; out_d: see above. */
int spyhip_fft_exec(spyhip_fft_plan* plan, const float* data_d, int64_t ld,
                    const int32_t* chan_idx_d, const int64_t* seg_start_d, const int64_t* seg_lo_d,
                    const int64_t* seg_hi_d, int nseg, void* out_d);
/* Internal hand-over layout between spyhip_fft_exec and spyhip_csd_accumulate_blocked (the coherence path
 * never shows the per-trial spectra to the host): with on != 0 a FOURIER / keeptapers=1 plan writes
 * (nseg*ntaper, ceil(nchan/4), nfsel, 4) complex64 - the four channels of a quad contiguous in frequency -
 * so that every wave stores whole 2-KiB runs.  Channels beyond nchan in the last quad are written as 0.
 * Returns -3 for plans that cannot use it (other outputs, nfft not a power of two in 256..8192). */
int spyhip_fft_plan_set_blocked(spyhip_fft_plan* plan, int on);
/* Precision of the transform.  reference = 0 (default): taper product and FFT in float32 - error ~1e-7 of a
 * channel's largest bin, inside the parity criterion |a-b| <= 1e-5 |b| + 1e-6 max|b|.  reference = 1: float64 taper
 * product and float64 FFT, the spectrum rounded to complex64 and scaled in float32 exactly where
 * specest/mtmfft.py:104-127 does it - every bin to ~1e-7 of ITSELF (pure rtol 1e-5 also 60 dB below the peak).  Cost:
 * ~2x float32 where a compile-time radix schedule exists (mtmfft_dec64_kernel.h: nfft = 256 ... 16384 powers of two, 200,
 * 500, 1000, 2000, 2500, 4000, 5000, 10000); every other nfft up to 2^20 runs generic Stockham passes over work arrays in
 * LDS (nfft <= 5120) or global memory (4-10x), in Bluestein's chirp-z form when nfft has a prime factor above 61;
 * standard layout only; -3 beyond 2^20 points. */
int spyhip_fft_plan_set_precision(spyhip_fft_plan* plan, int reference);
/* Constant detrending (detrend = SPYHIP_DETREND_CONSTANT) with the per-channel mean taken EXACTLY as the reference
 * takes it for whole trials: scipy.signal.detrend on the float32 (time x channel) array is data - np.mean(data, 0),
 * and NumPy sums the slow axis sequentially in ONE float32 accumulator per channel (then one float32 division).
 * For channels riding on an offset that rounding sequence is what the bins next to DC consist of.  on = 1: a
 * pre-pass reproduces it literally (one thread per channel walks the rows in order); on = 0 (default): float64
 * block sums inside the transform kernel - the better match for per-segment detrending of sliding windows, which
 * the reference does in float64 (specest/stft.py:112-132); on = 2: the same, and the plan is told that the reference
 * holds these segments as FLOAT64 arrays (zero-extended / padded windows): the reference-precision kernels
 * (spyhip_fft_plan_set_precision) then subtract the trend in float64 instead of rounding the samples to float32. */
int spyhip_fft_plan_set_reference_mean(spyhip_fft_plan* plan, int on);
/* Range of the spectra for spyhip_csd_accumulate_split: with absmax_d != NULL (nchan floats on the device, zeroed by the
 * caller) every spyhip_fft_exec of a FOURIER / keeptapers=1 plan raises absmax_d[c] to a BOUND of every |re|, |im| it
 * writes for channel c: max over tapers of ||w scale||_2 times the 2-norm of the detrended segment (Cauchy-Schwarz; one sum
 * of squares per segment from samples that are in registers anyway - a maximum over the values written costs the
 * transform kernel 6 %).  The bound sits sqrt(nsig) / (crest factor) above the largest bin of noise-like data (3-4 bits of
 * the ~18 the half-precision kernel has) and is tight for offset- or line-dominated channels, where the bits matter.
 * Float32 transforms of a power-of-two length 256 ... 8192 form it inside the transform kernel; every other length and the
 * float64 transforms (spyhip_fft_plan_set_precision) take one pass over the segments ahead of the transform.  Returns -3
 * (and stores nothing) for plans that do not write complex all-taper spectra in the standard layout; NULL switches it off. */
int spyhip_fft_plan_set_absmax(spyhip_fft_plan* plan, float* absmax_d);
/* name of the dominant kernel a plan launches (for rocprof matching) */
const char* spyhip_fft_plan_kernel_name(const spyhip_fft_plan* plan);

/* ---- K4: cross-spectral density accumulation (MFMA) -----------------------
 * Replaces the outer product + taper mean of csd (connectivity/csd.py:94-115),
 * spectral_dyadic_product_cF (connectivity/ST_compRoutines.py:30-117) and the
 * trial sum of ComputationalRoutine.compute_sequential
 * (shared/computational_routine.py:1022-1032):
 *
 *   acc[f,i,j] += sum_{r<nrows} X[r,f,i] * conj(X[r,f,j])        (i >= j)
 *
 * spec_d: complex64 (nrows, nfreq, nchan), nrows = trials x tapers (the
 * layout spyhip_fft_exec writes with output=FOURIER, keeptapers=1);
 * acc_d: complex64 (nfreq, nchan, nchan); only the lower triangle (incl.
 * diagonal, 32x32 tile granularity) is maintained until spyhip_csd_finalize. */
int spyhip_csd_accumulate(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                          void* acc_d);
/* Arithmetic of the accumulation.  Default (0): the 3-multiplication complex product where a kernel is built for the
 * channel count: re = P1 + P2, im = P3 - P1 + P2 from three fp32 row sums.  Its imaginary part carries an ABSOLUTE
 * error of ~6e-8 * sqrt(nrows) * |Re acc| (three independently rounded sums are subtracted): within rtol 1e-5 of
 * the complex value and of abs / pow / real outputs, but not of the imaginary part or the phase of strongly
 * coherent channel pairs near zero lag.  on = 1: the 4-multiplication kernels everywhere, whose imaginary part is
 * summed directly like the reference's complex64 products (connectivity/csd.py:98-102) - what the front ends select
 * for output = "imag" / "angle".  Per context; costs ~25 % of K4's throughput at 256 channels. */
int spyhip_csd_set_phase_exact(spyhip_ctx* ctx, int on);
/* Name of the dominant kernel an update of `nchan` channels launches on this context (blocked: through
 * spyhip_csd_accumulate_blocked, else through spyhip_csd_accumulate_split), written to buf[cap]; for rocprof matching.
 * Follows spyhip_csd_set_phase_exact and SPYHIP_CSD_F32. */
int spyhip_csd_kernel_name(spyhip_ctx* ctx, int nchan, int blocked, char* buf, int cap);
/* The same accumulation on the HALF-PRECISION matrix cores (K4h, csrc/csdh_kernel.h) for nchan = 256: every float32
 * operand, scaled by a power of two per channel, is split once into an fp16 pair hi + lo (22 significant bits) and a
 * real product is hi hi' + hi lo' + lo hi' with float32 accumulation - float32-class products at 5.3 x less matrix time
 * than the float32 instructions, with the plain 4-multiplication complex product (the imaginary part is summed directly:
 * this path also serves spyhip_csd_set_phase_exact contexts).  absmax_d: 256 floats on the device, per channel an upper
 * bound of |re| and |im| over the spectra of this call - what spyhip_fft_plan_set_absmax makes spyhip_fft_exec deliver
 * for free - or NULL: the library takes one extra pass over the spectra.  A frequency where a channel's rms sits more
 * than ~2^18 below that bound (or that holds Inf / NaN) is left to the float32 kernels by the half-precision kernel
 * itself (checked on the diagonal it accumulated, before anything is added): results never depend on the data's dynamic
 * range, only the speed does.  Other channel counts, and SPYHIP_CSD_F32=1 in the environment: identical to
 * spyhip_csd_accumulate.  Same reference lines (connectivity/csd.py:94-102). */
int spyhip_csd_accumulate_split(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                void* acc_d, const float* absmax_d);
/* The same update for the frequencies [f0, f0 + nf) only (spec_d and acc_d still point at frequency 0; nchan = 256 and
 * absmax_d are required): a caller that launches range by range can normalise and ship the results of range r while range
 * r + 1 is being accumulated - the coherence pipeline of the front end hides three quarters of its 0.54 GB host copy this
 * way.  The ranges of one accumulation may come in any order but must not overlap; together they equal one full call; a
 * range that reaches into the last partial round of workgroups (nfreq % CUs frequencies at the end) must end at nfreq.
 * Reference lines: connectivity/csd.py:94-102 (products), shared/computational_routine.py:1022-1036 (a result the caller
 * can read). */
int spyhip_csd_accumulate_split_range(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                      void* acc_d, const float* absmax_d, int f0, int nf);
/* number of frequencies the last spyhip_csd_accumulate_split call of this context handed to the float32 kernels
 * (synchronises the stream; for tests and benchmarks) */
int spyhip_csd_split_fallbacks(spyhip_ctx* ctx, int* count);
/* same accumulation from spectra in the channel-blocked layout of spyhip_fft_plan_set_blocked:
 * spec_d = (nrows, ceil(nchan/4), nfreq, 4) complex64.  Bit-identical results. */
int spyhip_csd_accumulate_blocked(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                  void* acc_d);
/* Lower triangle (i >= j) of the accumulator <-> packed (nfreq, nchan(nchan+1)/2) complex64: what the multi-GPU
 * path all-reduces between spyhip_csd_accumulate and spyhip_csd_finalize (the mutex-guarded `+=` of
 * shared/kwarg_decorators.py:723-735 ships 0.54 GB instead of 1.07 GB at 256 channels).  Unpack writes only the lower
 * triangle of acc_d. */
int spyhip_csd_tril_pack(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, void* packed_d);
int spyhip_csd_tril_unpack(spyhip_ctx* ctx, const void* packed_d, int nfreq, int nchan, void* acc_d);
/* acc[f,i,j] *= scale on the lower triangle and acc[f,j,i] = conj(acc[f,i,j]):
 * scale = 1/(ntaper*ntrials) turns the sum into the taper- and trial-mean. */
int spyhip_csd_finalize(spyhip_ctx* ctx, void* acc_d, int nfreq, int nchan, double scale);

/* ---- K5: coherence normalisation ------------------------------------------
 * Replaces normalize_csd (connectivity/csd.py:118-172):
 *   out[f,i,j] = conv( csd[f,i,j] / sqrt(csd[f,i,i]*csd[f,j,j]) )
 * output: POW/ABS/FOURIER/REAL/IMAG/ANGLE; out_d float32 or complex64
 * (nfreq, nchan, nchan); csd_d must be a full Hermitian array. */
int spyhip_coh_normalize(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, int output,
                         void* out_d);

/* K5 fused for the coherence pipeline: out = conv( (acc*scale)[f,i,j] / sqrt((acc*scale)[f,i,i] (acc*scale)[f,j,j]) ) for the
 * whole Hermitian (nfreq, nchan, nchan) output, read from the RAW lower-triangle accumulator of
 * spyhip_csd_accumulate (acc_d is not modified).  Equals spyhip_csd_finalize + spyhip_coh_normalize bit for bit
 * at a third of the HBM traffic. */
int spyhip_coh_from_accumulator(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, double scale, int output,
                                void* out_d);

/* ---- K3s: superlets ----------------------------------------------------------
 * spyhip_cwt_plan_create_sl: a CWT plan (same exec / destroy as above) whose kernels are the superlet formulation
 *   MorletSL (specest/superlet.py:268-292) sampled as cwtSL does (:311-375): support 10*s*cycles/dt samples, norm
 *   sqrt(dt)/(4 pi), k_sd standard deviations of the Gaussian envelope (the reference uses 5).
 * spyhip_slt_combine: one factor of the geometric mean of multiplicativeSLT / FASLT (superlet.py:97-211):
 *   acc[r, s0+q, c] = (init ? 1 : acc[r, s0+q, c]) * spec[r, q, c] ^ expo[q]     principal branch, 0^e = 0 (e > 0)
 *   acc_d complex64 (nrows, nscales, nchan); spec_d complex64 (nrows, nsub, nchan) = FOURIER output of one order's
 *   plan over the scales [s0, s0+nsub); expo = nsub host doubles (0 leaves the element as it is); modulus_only = 1
 *   folds |spec|^expo instead (all that the POW / ABS outputs need: no phase arithmetic); modulus_only = 2: acc_d and
 *   spec_d are float32 arrays of moduli (ABS output of the plan), half the traffic; | 4: the product is squared on
 *   store (last factor of a POW output).
 * spyhip_spec_convert: spectralConversions (shared/const_def.py:25-33) of n complex64 values to a real output kind. */
int spyhip_cwt_plan_create_sl(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales, double dt,
                              double cycles, double k_sd, int detrend, int output, const int32_t* tpos, int ntime_out,
                              spyhip_cwt_plan** out);
int spyhip_slt_combine(spyhip_ctx* ctx, void* acc_d, const void* spec_d, int64_t nrows, int nscales, int nsub, int s0,
                       int nchan, const double* expo, int init, int modulus_only);
int spyhip_spec_convert(spyhip_ctx* ctx, const void* in_d, int64_t n, int output, void* out_d);

/* ---- K7: pairwise phase consistency -----------------------------------------
 * Replaces ppc_column_cF (connectivity/ST_compRoutines.py:159-233) and the loop over all trial pairs with its
 * weighted average (connectivity/connectivity_analysis.py:624-663):
 *   ppc[f,i,j] = 2/(T(T-1)) sum_{a<b} cos(arg(S_a[f,i,j] conj(S_b[f,i,j])))  =  (|sum_t u_t|^2 - T) / (T(T-1)),
 *   u_t = S_t/|S_t| (1 where S_t = 0, as np.angle(0) = 0),  S_t = taper mean of X conj(X)^T of trial t.
 * spyhip_ppc_accumulate: acc[f,i,j] += sum_t u_t straight from the tapered spectra of spyhip_fft_exec
 *   (spec_d complex64 (ntrials*ntaper, nfreq, nchan), the ntaper rows of a trial adjacent); acc_d complex64
 *   (nfreq, nchan, nchan), maintained on the lower triangle (32x32 tile granularity).
 * spyhip_ppc_accumulate_csd: the same sum from single-trial cross spectra that exist already
 *   (csd_d complex64 (ntrials, nelem), acc_d complex64 (nelem): any block shape, e.g. channelcmb rectangles).
 * spyhip_ppc_finalize: out float32 (nfreq, ni, nj) from the accumulator and the total number of trials;
 *   lower_only = 1 for accumulators of spyhip_ppc_accumulate (the upper triangle is mirrored). */
int spyhip_ppc_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq, int nchan,
                          void* acc_d);
int spyhip_ppc_accumulate_csd(spyhip_ctx* ctx, const void* csd_d, int ntrials, int64_t nelem, void* acc_d);
int spyhip_ppc_finalize(spyhip_ctx* ctx, const void* acc_d, int nfreq, int ni, int nj, int lower_only,
                        int64_t ntrials, void* out_d);

/* ---- K10: phase-lag index, weighted phase-lag index, phase-locking value ------
 * Not in the reference (Stam 2007; Vinck 2011).  With S_t as for K7 and s_t = Im S_t (a positive scale changes nothing):
 *   A = sum_t s_t,  B = sum_t |s_t|,  Q = sum_t s_t^2,  N = sum_t sign(s_t)   (sign(0) = 0),
 *   pli = |N| / T,  wpli = |A| / B (0 where B = 0),  wpli_debiased = (A^2 - Q) / (B^2 - Q) (0 where B^2 - Q <= 0),
 *   plv = |sum_t u_t| / T  with K7's unit phasors.
 * spyhip_phaselag_accumulate: acc[f,i,j] += {A, B, Q, N} of the batch straight from the tapered spectra (spec_d as for
 *   spyhip_ppc_accumulate); acc_d float32 (nfreq, nchan, nchan, 4), zeroed by the caller, maintained on the lower
 *   triangle (32x32 tile granularity); plain sums, so ranks are combined by one sum.  -3: the tapers do not fit the LDS.
 * spyhip_phaselag_accumulate_csd: the same sums from single-trial cross spectra that exist already
 *   (csd_d complex64 (ntrials, nelem), acc_d float32 (nelem, 4)).
 * spyhip_phaselag_finalize: out float32 (nfreq, ni, nj) for one `measure` from the accumulator and the total number of
 *   trials (at least 2), evaluated in float64; lower_only = 1 for accumulators of spyhip_phaselag_accumulate: the upper
 *   triangle is mirrored and the diagonal is exactly 0.  Without it the rectangle is evaluated element by element.
 * spyhip_plv_finalize: out float32 (nfreq, ni, nj) = |U| / ntrials from an accumulator of spyhip_ppc_accumulate
 *   (lower_only = 1) or spyhip_ppc_accumulate_csd. */
enum { SPYHIP_PHASELAG_PLI = 0, SPYHIP_PHASELAG_WPLI = 1, SPYHIP_PHASELAG_WPLI_DEBIASED = 2 };
int spyhip_phaselag_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq, int nchan,
                               void* acc_d);
int spyhip_phaselag_accumulate_csd(spyhip_ctx* ctx, const void* csd_d, int ntrials, int64_t nelem, void* acc_d);
int spyhip_phaselag_finalize(spyhip_ctx* ctx, const void* acc_d, int nfreq, int ni, int nj, int lower_only,
                             int64_t ntrials, int measure, void* out_d);
int spyhip_plv_finalize(spyhip_ctx* ctx, const void* acc_d, int nfreq, int ni, int nj, int lower_only,
                        int64_t ntrials, void* out_d);

/* ---- K12: envelope correlations - amplitude, power, orthogonalised power ------
 * Not in the reference (Hipp et al. 2012).  Over the R = ntrials x ntaper repetitions r = (trial, taper) of the tapered
 * spectra x_i(r) of one frequency - every taper is a repetition, nothing is summed over tapers - and with
 *   corr(X; E1a, E2a, E1b, E2b) = (X - E1a E1b / R) / sqrt(va vb),  va = E2a - E1a^2 / R,  vb = E2b - E1b^2 / R,
 *   0 (not NaN) where a variance is zero, which is v <= 2^-40 E2:
 *   amplcorr (e = |x|), powcorr (e = |x|^2):  corr(sum e_i e_j; sum e_i, sum e_i^2, sum e_j, sum e_j^2);
 *   powcorr_ortho:  p = |x|^2,  s = Im(x_i conj(x_j)),  q_j|i = s^2 / p_i (0 where p_i = 0),  Z = sum s^2,
 *     c_j|i = corr(Z; sum p_i, sum p_i^2, sum q_j|i, sum q_j|i^2),  result (c_j|i + c_i|j) / 2, 0 unless both exist.
 *   |x|, p, 1 / p, s, s^2 and q are float32; their products and every sum are float64.  No spectral normalisation is
 *   needed: a positive scale per channel changes no result.
 * spyhip_envcorr_accumulate: the sums of the batch straight from the tapered spectra (spec_d as for
 *   spyhip_ppc_accumulate).  pair_d float64 (NP, nfreq, nchan, nchan), planar, NP = 1 {sum e_i e_j} for amplcorr and
 *   powcorr, NP = 5 {Z, sum q_j|i, sum q_j|i^2, sum q_i|j, sum q_i|j^2} at [i, j] for powcorr_ortho, maintained on the
 *   lower triangle (32x32 tile granularity); chan_d float64 (nfreq, nchan, 2) {sum e, sum e^2}, for powcorr_ortho
 *   {sum p, sum p^2}.  Both zeroed by the caller; plain sums, so ranks are combined by one sum each.  ntrials = 0 does
 *   nothing.  -3: the tapers do not fit the LDS: the two staging buffers take 1 KiB per taper for amplcorr and powcorr
 *   (160 tapers in 160 KiB, as K7 and K10) and 2 KiB per taper for powcorr_ortho (80 tapers).
 * spyhip_envcorr_finalize: out float32 (nfreq, nchan, nchan) for `measure` from the two accumulators and the total
 *   number of repetitions nrep (at least 2), evaluated in float64, clamped to [-1, 1] and rounded once; the upper
 *   triangle is mirrored; the diagonal is exact: 1 where the channel's variance is not zero and 0 elsewhere for amplcorr
 *   and powcorr, 0 for powcorr_ortho.
 * -1: a null or non-positive argument, an unknown measure, nrep < 2. */
enum { SPYHIP_ENVCORR_AMPL = 0, SPYHIP_ENVCORR_POW = 1, SPYHIP_ENVCORR_POW_ORTHO = 2 };
int spyhip_envcorr_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq, int nchan,
                              int measure, void* pair_d, void* chan_d);
int spyhip_envcorr_finalize(spyhip_ctx* ctx, const void* pair_d, const void* chan_d, int nfreq, int nchan, int64_t nrep,
                            int measure, void* out_d);

/* ---- K13: phase slope index --------------------------------------------------
 * Not in the reference (Nolte et al. 2008; FieldTrip's `psi`).  With c_ij(f) the complex64 coherency of
 * spyhip_coh_normalize / spyhip_coh_from_accumulator (output 'fourier'; the diagonal's imaginary part zeroed) - but 0,
 * not NaN, where the product of the two diagonal values is not positive - edge e joins the bins e and e + 1:
 *   p_ij(e) = Im(conj(c_ij(e)) c_ij(e + 1)) = c.x(e) c.y(e + 1) - c.y(e) c.x(e + 1),  both products exact in float64;
 *   half >= 1:  out[k, i, j] = sum_{e = k - half}^{k + half - 1} p_ij(e)  for half <= k <= nfreq - 1 - half, whole planes
 *     NaN for the other k (the band does not fit); out float32 (nfreq, nchan, nchan);
 *   half = 0:   out[0, i, j] = sum_{e = 0}^{nfreq - 2} p_ij(e); out float32 (1, nchan, nchan), nothing beyond is written.
 *   Every sum over edges is float64 (a running window sum: newest edge added, oldest subtracted), rounded to float32
 *   once.  Layout [f, sender, receiver]: out[f, i, j] > 0 where i leads j (S_ij = <x_i conj(x_j)>).  The result is
 *   antisymmetric bit for bit (the upper triangle is the negated mirror of the lower), the diagonal exactly +0.
 * spyhip_phaseslope: csd_d complex64 (nfreq, nchan, nchan), full Hermitian (its lower triangle is read).
 * spyhip_phaseslope_from_accumulator: acc_d the raw lower-triangle accumulator of spyhip_csd_accumulate, not modified;
 *   `scale` applied as spyhip_coh_from_accumulator applies it.  The same bits as spyhip_phaseslope on the finalised CSD.
 *   half = 0 with more than one run of frequencies uses the context's scratch for float64 partial sums.
 * -1: a null or non-positive argument, half < 0, nfreq < 2, 2 * half > nfreq - 1. */
int spyhip_phaseslope(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, int half, void* out_d);
int spyhip_phaseslope_from_accumulator(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, double scale, int half,
                                       void* out_d);

/* ---- K9: streaming jackknife of the coherence --------------------------------
 * Replaces, for method='coh' with jackknife=True, the T leave-one-out trial averages (statistics/jackknifing.py:14-108),
 * the AV stage on every replicate (connectivity_analysis.py:736-745) and the sums behind bias_var (:111-184):
 *   for every trial t of the batch:  S_t = taper mean of X conj(X)^T,  loo = (T*S - S_t)/(T-1)  (complex64),
 *   c_t = conv(loo_ij / sqrt(loo_ii loo_jj)),  d_t = c_t - direct;   sum_d += d_t,  sum_d2 += |d_t|^2   (float64)
 * spec_d complex64 (ntrials*ntaper, nfreq, nchan) as for spyhip_ppc_accumulate; csd_d complex64 (nfreq, nchan, nchan)
 * = the finalised trial average S; direct_d = spyhip_coh_normalize(S) in the same output kind (float32, or complex64
 * for FOURIER); sum_d float64 (nfreq, nchan, nchan) - or complex128 for FOURIER -, sum_d2 float64; T = ntrials_total.
 * bias = (T-1) sum_d / T,  var = (T-1) (sum_d2 - |sum_d|^2 / T). */
int spyhip_jack_coh_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq, int nchan,
                               const void* csd_d, const void* direct_d, int output, int64_t ntrials_total,
                               void* sum_d, void* sum_d2);

/* ---- K8: cross-covariance / cross-correlation -------------------------------
 * Replaces cross_covariance_cF (connectivity/ST_compRoutines.py:466-584: one fftconvolve per channel pair and
 * trial, lags 0 .. N/2 divided by the overlap N - lag, norm=True: divided by the products of np.std), the trial
 * average, and normalize_ccov_cF (connectivity/AV_compRoutines.py:166-228).
 * The trial sum is taken on the cross spectra: feed spyhip_csd_accumulate with the spectra of the trials
 * zero-padded to nfft = spyhip_ccov_nfft(nsamples) points (spyhip_fft_exec, boxcar, FOURIER; 1 row per trial),
 * then ONE inverse transform per channel pair:
 *   out[l,a,b] = scale * R_ab(l) / (N - l)         a >= b,   R_ab(tau) = sum_n x_a[n] x_b[n - tau]
 *   out[l,a,b] = scale * R_ab(l + q) / (N - l)     a <  b,   q = 1 for even N, 0 for odd N (the reference's
 *                                                            reversed "same" crop), l = 0 .. ceil(N/2) - 1
 * acc_d: raw lower-triangle accumulator (nfft/2 + 1, nchan, nchan) complex64; out_d float32 (ceil(N/2), nchan,
 * nchan); scale = 1 / (ntrials * fft_scale^2) (the 1/nfft of the inverse transform is applied inside).  norm: 0 none; 1 divide by sqrt(out[0,a,a] out[0,b,b])
 * (normalize_ccov_cF); 2 divide by np.std(x_a) np.std(x_b) of the ONE trial in acc_d (cross_covariance_cF norm=True).
 * spyhip_ccov_nfft: transform length for trials of nsamples (power of two >= N + ceil(N/2), 1024 .. 8192), or -1. */
int spyhip_ccov_nfft(int nsamples);
int spyhip_ccov_from_accumulator(spyhip_ctx* ctx, const void* acc_d, int nfft, int nchan, int nsamples, double scale,
                                 int norm, void* out_d);
/* normalize_ccov_cF alone, in place on a cross-covariance cc_d float32 (nlag, nchan, nchan):
 * cc[l,a,b] /= sqrt(cc[0,a,a] cc[0,b,b]). */
int spyhip_ccov_normalize(spyhip_ctx* ctx, void* cc_d, int nlag, int nchan);

/* ---- K3: Morlet continuous wavelet transform ------------------------------
 * Replaces cwt_time (specest/wavelets/transform.py:88-108) with Morlet.time
 * (specest/wavelets/wavelets.py:27-86) and the tail of wavelet_cF
 * (specest/compRoutines.py:582-595): detrend the whole trial, full linear
 * convolution of the nsig pre-selected samples with the sampled complete Morlet
 * kernel of every scale (M = 10*s/dt taps, amplitude sqrt(dt)/(8 pi s)), cropped
 * like scipy.signal.fftconvolve(mode="same"), converted with `output`.
 * tpos (host, nsig entries or NULL): output slot of sample n or -1 (post-selection).
 * Result per segment: (ntime_out, 1, nscales, nchan) float32 / complex64. */
int spyhip_cwt_plan_create(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales,
                           double dt, double w0, int detrend, int output, const int32_t* tpos,
                           int ntime_out, spyhip_cwt_plan** plan);
/* The same transform with another sampled kernel family (the convolution kernels do not care which):
 * family 0 Morlet(w0 = p0), 1 MorletSL(cycles = p0, k_sd = p1) (= spyhip_cwt_plan_create_sl), 2 Paul(m = p0),
 * 3 DOG(m = p0) - Ricker / Marr / Mexican_hat are DOG(2) (specest/wavelets/wavelets.py:140-223; freqanalysis.py:55). */
int spyhip_cwt_plan_create_family(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales,
                                  double dt, int family, double p0, double p1, int detrend, int output,
                                  const int32_t* tpos, int ntime_out, spyhip_cwt_plan** plan);
int spyhip_cwt_plan_destroy(spyhip_cwt_plan* plan);
/* reference = 1: the transform as scipy.signal.fftconvolve computes it for cwt_time / cwtSL (specest/wavelets/
 * transform.py:88-108, specest/superlet.py:311-375): float64 FFT convolution of the detrended float32 trial with the
 * complex128 taps, rounded to complex64 where the reference stores it - one length-2^m >= nsig + taps - 1 convolution per
 * (segment, channel), generic Stockham passes over work arrays in global memory (~50x the float32 kernels: for
 * precision="reference" and the per-trial route, where the copies cost as much).  0 (default): the float32 overlap-save
 * kernels (~5e-7 of a trial's largest coefficient). */
int spyhip_cwt_plan_set_precision(spyhip_cwt_plan* plan, int reference);
/* on = 1 (default): scales whose kernel support fits 1024- / 2048-point blocks leave their transform kernel in the output's
 * own (segment, time, scale, channel) layout (cwt2d_kernel: 16 / 8 channels per workgroup, 64- / 32-byte runs) for
 * accumulate = 0 / 1; trial sums (accumulate = 2) and float64 precision always go through the staging buffer.  Plans whose
 * time slots do not increase with the samples, or whose tiles' slots span 4 GiB or more of the output (gapped tpos), are
 * staged only: on = 1 fails for them (-3).  0: every scale through the time-contiguous staging buffer and the
 * transposition pass (rounds 1-5; kept for A/B measurements and as the cross-check of the direct kernels).
 * Replaces the (nScales, N, C) array the reference writes once per trial: specest/wavelets/transform.py:88-108. */
int spyhip_cwt_plan_set_direct(spyhip_cwt_plan* plan, int on);
/* seg_start_d: row of sample 0 of each pre-selected signal; trial_lo_d/trial_hi_d: rows of the
 * whole trial (detrending range); accumulate: 0 = store, 1 = out_d[b] += result of segment b,
 * 2 = out_d[0] += sum over the nseg segments (trial averaging: one read-modify-write of the output per chunk
 * of segments instead of one per trial). */
int spyhip_cwt_exec(spyhip_cwt_plan* plan, const float* data_d, int64_t ld,
                    const int32_t* chan_idx_d, const int64_t* seg_start_d, const int64_t* trial_lo_d,
                    const int64_t* trial_hi_d, int nseg, void* out_d, int accumulate);

/* ---- K6: Wilson spectral factorisation + Granger-Geweke causality ---------
 * Replaces regularize_csd / wilson_sf (connectivity/wilson_sf.py:16-254) and
 * granger (connectivity/granger.py:10-79) as called from granger_cF
 * (connectivity/AV_compRoutines.py:293-412).  csd_d: complex64 (nfreq, C, C)
 * trial-averaged CSD.  granger_d: float32 (nfreq, C, C).  info (host, 4
 * doubles): converged, max rel. err, reg. factor, initial cond. num.
 * H_d / Sigma_d (complex128 (nfreq,C,C) / complex128 (C,C)) may be NULL.
 * Return -6: a Cholesky factorisation met a matrix that is not positive definite (np.linalg.cholesky's LinAlgError at
 * wilson_sf.py:76,144-151; the Python host mirror raises that type). */
int spyhip_granger(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, double rtol, int niter,
                   double cond_max, double eps_max, void* granger_d, void* H_d, void* Sigma_d,
                   double* info);

/* ---- K6 in steps, for frequency shards ---------------------------
 * One rank holds the bins [f_lo, f_lo + nf) of the nftot rfft bins of the trial-averaged CSD.  Regularisation,
 * Cholesky factor, inverse, products and the error are per frequency (local); the plus operator
 * (wilson_sf.py:154-184) works along the frequency axis: the host transposes g between "my frequencies x all entries"
 * and "all frequencies x my entries" around spyhip_wilson_plus (one all-to-all each way) and reduces three small
 * quantities over ranks (gamma_0: sum; condition number, error: max).  Host side:
 * syncopy_amd/connectivity/wilson_sharded.py; with one rank the sequence equals spyhip_granger.
 * Arrays are complex128 on the device unless stated; "work" arrays are scratch of the stated size.
 *   spyhip_wilson_cond   A = complex128(csd) + eps I (regularize_csd, wilson_sf.py:239-248); *cond_out = largest
 *                        2-norm condition number of the local bins.  work_d: 3 nf n^2.
 *   spyhip_wilson_init   U = Cholesky factor of A per bin (:76); gamma_part_d (n, n) = this shard's part of
 *                        gamma_0 = fft(CSD_full)[0] (:135-140), to be summed over ranks.
 *   spyhip_wilson_psi0   psi0 = chol(gamma_0)^T (:144-151) from the summed gamma_0 (overwritten), tiled into psi_d.
 *   spyhip_wilson_g      g = (psi^-1 U)(psi^-1 U)^H + I (:80-92).  work_d: 2 nf n^2.  Returns 1 (not an error) if
 *                        the block inverse met a tiny pivot: restart the factorisation with pivoted = 1.
 *   spyhip_wilson_plus   g+ and the halved zero-lag coefficients g0 for nent entries over all nftot frequencies:
 *                        g_d, gp_d (nftot, nent), g0_d (nent).
 *   spyhip_wilson_update psi <- psi (g+ + S), psi0 <- psi0 (g0 + S), S = triu(g0) - triu(g0)^H (:97-101);
 *                        *err_out = this shard's max |A - psi psi^H| / |A| (:103,190-194).  g0_d: all n^2 entries.
 *                        work_d: nf n^2.
 *   spyhip_wilson_finish Sigma = psi0 psi0^T, H = psi psi0^-1, Granger causality (granger.py:53-77) on the local
 *                        bins: granger_d float32 (nf, n, n); H_d / Sigma_d may be NULL.  work_d: nf n^2. */
int spyhip_wilson_cond(spyhip_ctx* ctx, const void* csd_c64_d, int nf, int n, double eps, void* A_d, void* work_d,
                       double* cond_out);
int spyhip_wilson_init(spyhip_ctx* ctx, const void* A_d, int nf, int n, int f_lo, int nftot, void* U_d,
                       void* gamma_part_d);
int spyhip_wilson_psi0(spyhip_ctx* ctx, void* gamma0_d, int n, int nf, void* psi0_d, void* psi_d);
int spyhip_wilson_g(spyhip_ctx* ctx, const void* psi_d, const void* U_d, int nf, int n, int pivoted, void* work_d,
                    void* g_d);
int spyhip_wilson_plus(spyhip_ctx* ctx, const void* g_d, int nftot, int64_t nent, void* gp_d, void* g0_d);
int spyhip_wilson_update(spyhip_ctx* ctx, void* psi_d, const void* gp_d, const void* g0_d, void* psi0_d,
                         const void* A_d, int nf, int n, void* work_d, double* err_out);
int spyhip_wilson_finish(spyhip_ctx* ctx, const void* A_d, const void* psi_d, const void* psi0_d, int nf, int n,
                         void* work_d, void* granger_d, void* H_d, void* Sigma_d);

/* Wilson iterations the last spyhip_granger call on this context ran (the reference's loop counter,
 * wilson_sf.py:77-109); for benchmarks and diagnostics. */
int spyhip_granger_last_iterations(const spyhip_ctx* ctx);

/* ---- K11: directed transfer function and partial directed coherence from the factors of K6 (not in the reference) ----
 * spyhip_zinv: dst[b] = src[b]^-1 for `batch` complex128 n x n matrices on the device; dst_d may equal src_d.  The block
 *   Gauss-Jordan kernel of the size class runs first (K6's inverse of the iteration, csrc/granger_route.h); if a matrix
 *   flags a tiny pivot the whole batch is repeated with the partially pivoted kernel.  The flags (and, in place, a copy
 *   of the input) live in the context's work arrays: nothing is allocated per call once they are large enough.
 *   Return -7: a matrix is singular (a zero pivot under partial pivoting); dst is undefined then.
 * spyhip_directed_norm: M_d complex128 (nfreq, n, n), w_d n doubles on the device or NULL (all ones), out_d float32
 *   (nfreq, n, n) in the layout [f, sender, receiver] - the transpose of M's index order:
 *     axis 0 (DTF, M = H):     out[f,s,r] = w_s |M[f,r,s]| / sqrt(sum_k w_k^2 |M[f,r,k]|^2)
 *     axis 1 (PDC, M = H^-1):  out[f,s,r] = w_r |M[f,r,s]| / sqrt(sum_k w_k^2 |M[f,k,s]|^2)
 *   squared = 1: the square.  A zero norm gives 0.  float64 arithmetic, one rounding to float32.  w = sqrt(diag Sigma)
 *   with axis 0 is the directed coherence, w = 1 / sqrt(diag Sigma) with axis 1 the generalised PDC.  out_d must not be
 *   M_d.  -3 if no tile fits the LDS of a workgroup (csrc/directed_route.h). */
int spyhip_zinv(spyhip_ctx* ctx, const void* src_d, void* dst_d, int batch, int n);
int spyhip_directed_norm(spyhip_ctx* ctx, const void* M_d, const void* w_d, int nfreq, int n, int axis, int squared,
                         void* out_d);

/* ---- utilities on the in-HBM trial queue ---------------------------------- */
/* out[r, :] = alpha * sum_t in[t, r, :]  (trial mean of (T, n) float32) */
int spyhip_trial_mean_f32(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t n);
/* the same for (T, n) complex64: sums per component, then the reference's complex division by the real count - a
 * multiplication by the float32 reciprocal 1/T (NumPy's Smith division, summary_stats.py:426) */
int spyhip_trial_mean_c64(spyhip_ctx* ctx, const void* in_d, void* out_d, int64_t ntrials, int64_t n);
/* spy.mean(data, dim=<axis label>) for one trial (statistics/summary_stats.py:24, statistics/compRoutines.py:22-57:
 * np.nanmean(trial, axis, keepdims=True)): x_d (outer, n, inner) float32 or complex64 -> out_d (outer, inner); NaN
 * elements are skipped; float32 sums in NumPy's order (rows in order for an axis that is not the last, pairwise
 * blocks for the last one), one division in float64. */
int spyhip_axis_nanmean(spyhip_ctx* ctx, const void* x_d, int64_t outer, int64_t n, int64_t inner, int is_complex,
                        void* out_d);

/* ---- spy.var / spy.std / spy.median / spy.itc (statistics/summary_stats.py:156-205, 321-486; statistics/compRoutines.py:
 * 22-141).  All pointers are device pointers; the accumulators belong to the caller, who zeroes them before the first
 * chunk, so trials can be streamed in chunks of any size with the same bits. */
/* dim="trials", pass 1 (_trial_average, summary_stats.py:408-428): acc_d[i] += in_d[0, i] + ... + in_d[ntrials-1, i] in
 * trial order, in float32; nfloat floats per trial (complex64: 2 per element, the components are summed apart) */
int spyhip_trial_sum(spyhip_ctx* ctx, const void* in_d, float* acc_d, int64_t ntrials, int64_t nfloat);
/* mean_d = acc_d / ntotal over n elements (float32: a division; complex64: times fl(1/ntotal), NumPy's Smith division by
 * the real count); mean_d may be acc_d */
int spyhip_trial_sum_finalize(spyhip_ctx* ctx, const float* acc_d, void* mean_d, int64_t ntotal, int64_t n, int is_complex);
/* dim="trials", pass 2 (_trial_var, summary_stats.py:431-456): acc_d[i] (float32, n elements) += fl(|x - mean|)^2 over the
 * chunk's trials in order; |.| of complex64 correctly rounded */
int spyhip_trial_sqdev(spyhip_ctx* ctx, const void* in_d, const void* mean_d, float* acc_d, int64_t ntrials, int64_t n,
                       int is_complex);
/* out_d = acc_d / ntotal (complex64: times fl(1/ntotal), written as (v, 0)); take_sqrt: np.sqrt of it (spy.std,
 * summary_stats.py:362) */
int spyhip_trial_var_finalize(spyhip_ctx* ctx, const float* acc_d, void* out_d, int64_t ntotal, int64_t n, int is_complex,
                              int take_sqrt);
/* spy.itc pass (_trial_circ_average, summary_stats.py:459-486): acc_d[i] (complex64, n elements) += z / |z| over the
 * chunk's trials in order; z = 0 or a non-finite z gives NaN */
int spyhip_itc_accumulate(spyhip_ctx* ctx, const void* in_d, void* acc_d, int64_t ntrials, int64_t n);
/* acc_d (outer, ntaper, inner) complex64 -> out_d (outer, inner) float32: / ntotal, mean over the tapers, |.| correctly
 * rounded (summary_stats.py:364-373) */
int spyhip_itc_finalize(spyhip_ctx* ctx, const void* acc_d, float* out_d, int64_t ntotal, int64_t outer, int64_t ntaper,
                        int64_t inner);
/* spy.var / spy.std (dim=<axis label>) for one trial (compRoutines.py:22-57: np.nanvar / np.nanstd(trial, axis,
 * keepdims=True), ddof 0): x_d (outer, n, inner) float32 or complex64 -> out_d (outer, inner) of the same dtype (complex:
 * imaginary part 0); NaN elements skipped, an all-NaN slice gives NaN */
int spyhip_axis_nanvar(spyhip_ctx* ctx, const void* x_d, int64_t outer, int64_t n, int64_t inner, int is_complex,
                       int take_sqrt, void* out_d);
/* spy.median (dim=<axis label>) for one trial (np.nanmedian(trial, axis, keepdims=True)): x_d (outer, n, inner) float32
 * or complex64 (ordered by real, then imaginary part) -> out_d (outer, inner); work_d holds outer*n*inner elements when
 * inner > 1 (the slices are made contiguous there) and may be NULL otherwise; n < 2^31 */
int spyhip_axis_nanmedian(spyhip_ctx* ctx, const void* x_d, int64_t outer, int64_t n, int64_t inner, int is_complex,
                          void* work_d, void* out_d);

/* ---- spy.preprocessing (preproc/preprocessing.py; preproc/compRoutines.py: detrending_cF, standardize_cF,
 * but_filtering_cF, sinc_filtering_cF, rectify_cF; preproc/firws.py: apply_fir).  in_d / out_d: a batch of equal-length
 * trials (ntrials, nsamp, nchan) float32 on the device, channel fastest; at most 2^31 - 1 elements per trial.  All
 * buffers belong to the caller.  nan_d: one int32 per trial, zeroed by the caller; a call sets nan_d[t] = 1 when
 * trial t of its input holds a NaN (the reference's has_nan) and never clears it.  rectify != 0 stores |.|
 * (rectify_cF) instead of a pass of its own.  The filter designs (sos, zi, taps) are the caller's, in float64. */
/* scipy.signal.detrend(trial, type="constant" | "linear", axis=0) for order 0 | 1.  Order 0 takes the float32 mean as
 * NumPy does (rows added in time order, one division; pairwise when nchan == 1); order 1 fits the line in float64.
 * out_d may be in_d. */
int spyhip_detrend(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                   int order, int rectify, int32_t* nan_d);
/* (x - np.mean(x, 0)) / np.std(x, 0) per channel and trial in float32 with NumPy's summation order (standardize_cF
 * after its optional detrend); out_d must not be in_d */
int spyhip_standardize(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                       int rectify, int32_t* nan_d);
/* scipy.signal.sosfilt(sos, trial, axis=0): sos = nsec x 6 host doubles [b0 b1 b2 1 a1 a2], nsec <= 12; state and
 * arithmetic in float64; out_d may be in_d */
int spyhip_sosfilt(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                   const double* sos, int nsec, int rectify, int32_t* nan_d);
/* scipy.signal.sosfiltfilt(sos, trial, axis=0): zi = nsec x 2 host doubles (sosfilt_zi), edge = samples of odd
 * extension at either end (SciPy's 3 * ntaps; nsamp > edge); work_d holds ntrials * (nsamp + 2 * edge) * nchan doubles
 * (the forward pass in float64) */
int spyhip_sosfiltfilt(spyhip_ctx* ctx, const float* in_d, float* out_d, double* work_d, int64_t ntrials, int64_t nsamp,
                       int64_t nchan, const double* sos, const double* zi, int nsec, int edge, int rectify,
                       int32_t* nan_d);
/* scipy.signal.convolve(trial, taps[:, None], mode="same") as a direct float64 sum (apply_fir): taps_d = ntaps doubles
 * ON THE DEVICE, any length (also longer than the trial); a NaN sample spoils the ntaps outputs around it in its own
 * channel only; out_d must not be in_d */
int spyhip_fir_same(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                    const double* taps_d, int ntaps, int rectify, int32_t* nan_d);
/* scipy.signal.resample_poly(trial, up, down, window=taps / up, axis=0) and trial[::down] (resample_cF, downsample_cF) as
 * one up-FIR-down pass: out[m] = sum_i taps[m * down + (ntaps - 1) / 2 - i * up] * x[i] for m < nout, a float64 sum,
 * in_d (ntrials, nsamp, nchan) -> out_d (ntrials, nout, nchan).  taps_d = ntaps doubles ON THE DEVICE, already
 * multiplied by up, any length; up = 1 with the one tap 1.0 is the plain decimation, up = 1 with a filter keeps every
 * down-th sample of spyhip_fir_same.  No NaN report; out_d must not be in_d */
int spyhip_upfirdn(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                   int64_t nout, const double* taps_d, int ntaps, int up, int down);

/* The Hilbert option (hilbert_cF): scipy.signal.hilbert(trial, axis=0), circular over the trial length nsamp with no
 * padding, followed by spectralConversions[output].  A plan owns the tables of one trial length, 1 ... 2^20 samples
 * (-3 beyond); which kernel family serves it is decided in csrc/hilbert_route.h and named by ..._kernel_name.
 * exec (asynchronous, on the context's stream): in_d (ntrials, nsamp, nchan) float32 -> out_d of the same shape,
 * complex64 for output = SPYHIP_OUT_FOURIER ("complex"), float32 for SPYHIP_OUT_ABS, _REAL, _IMAG, _ANGLE, _ABSREAL and
 * _ABSIMAG; out_d must not be in_d.  The real part of the analytic signal is the input itself.  A channel of a trial
 * that holds a non-finite sample (NaN or +-inf: SciPy leaves a mix of the two there) comes out all-NaN and raises
 * nan_d[trial]; no other channel is touched by it.  Lengths that are no power of two up to 8192 and are longer than
 * 4096 samples run in complex128 over work arrays in the context's scratch buffer (at most 512 MiB per launch). */
int spyhip_hilbert_plan_create(spyhip_ctx* ctx, int64_t nsamp, spyhip_hilbert_plan** plan);
int spyhip_hilbert_exec(spyhip_hilbert_plan* plan, const float* in_d, void* out_d, int64_t ntrials, int64_t nchan,
                        int output, int* nan_d);
int spyhip_hilbert_plan_destroy(spyhip_hilbert_plan* plan);
const char* spyhip_hilbert_plan_kernel_name(const spyhip_hilbert_plan* plan);

/* ---- spy.timelockanalysis (statistics/timelockanalysis.py; statistics/compRoutines.py: cov_cF).  The channel
 * covariance np.cov(trial, ddof=ddof, rowvar=False) of every trial of a batch of equal-length trials: x_d (ntrials, n,
 * nchan) float32 on the device, channel fastest -> out_d (ntrials, nchan, nchan) float32.  Column means, centring,
 * products and their sums in float64 (v_mfma_f64_16x16x4_f64), times 1.0 / (n - ddof), rounded to float32 once; the
 * order of every sum is fixed, so two calls give the same bits.  A NaN in channel c of a trial makes row and column c
 * of that trial's matrix NaN and nothing else.  ddof >= 0 and n - ddof > 0 (NumPy's ddof=None is 1); any nchan >= 1;
 * out_d must not be x_d.  Uses the context's scratch buffer (ntrials * nchan doubles, at most 65535 trials' worth). */
int spyhip_cov_f32(spyhip_ctx* ctx, const float* x_d, float* out_d, int64_t ntrials, int64_t n, int64_t nchan,
                   int64_t ddof);

/* ---- spy.spike_psth (statistics/spike_psth.py; statistics/psth.py: psth, get_chan_unit_combs; statistics/
 * compRoutines.py: psth_cF, PSTH).  The spike table lives on the device as three arrays of one entry per spike, SORTED
 * BY SAMPLE: sample_d int64, chan_d int32, unit_d int32 (16 bytes per spike).  Trial t owns the rows [row_lo_d[t],
 * row_hi_d[t]) (np.searchsorted(sample, [start, end]), datatype/discrete_data.py:186-196; a repeated trial names its
 * rows again) and puts a spike at time = (double)(sample - start_d[t] + onset_d[t]) / samplerate, one IEEE float64
 * division (psth.py: _calc_time).  A spike counts in bin b when edges[b] <= time < edges[b + 1], the last bin also
 * takes time == edges[nbins] (np.histogram2d with explicit edges); edges_d holds nedges = nbins + 1 float64 values as
 * the host computed them.  Counts are integer sums in LDS: every result is bitwise reproducible, and spikecount and
 * rate are the reference's bits.  No entry point allocates, synchronises, or uses a global atomic; all run on the
 * context's stream.  channel < nchan and unit < nunit for every row of a trial (rows that break this are ignored),
 * nchan * nunit <= 2^24, ntrials < 2^31.
 * DEVIATION, on purpose: a spike on channel c, unit u counts in column (c, u).  The reference hands raw channel numbers
 * to histogram2d with the channel bins arange(k + 1), k = distinct channels of the trial, and miscounts whenever a
 * trial's channels are not exactly 0 .. k-1. */
/* get_chan_unit_combs without the per-trial np.unique loop: flags_d[c * nunit + u] = 1 (uint8, zeroed by the caller)
 * for every row of the trials whose channel c has chan_ok_d[c] != 0 and whose unit u has unit_ok_d[u] != 0 (uint8
 * masks of nchan and nunit entries: the selection).  max_rows = the longest trial, which sizes the grid. */
int spyhip_psth_presence(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d, const int64_t* row_lo_d,
                         const int64_t* row_hi_d, int64_t ntrials, int64_t max_rows, const uint8_t* chan_ok_d,
                         int64_t nchan, const uint8_t* unit_ok_d, int64_t nunit, uint8_t* flags_d);
/* rows_d (ntrials, nedges) int64: rows_d[t][e] = the first row of trial t with time >= edges_d[e], for the last edge
 * with time > edges_d[e] (row_hi_d[t] when there is none): the spikes of (t, bin b) are rows [rows_d[t][b],
 * rows_d[t][b + 1]).  A binary search per (trial, edge). */
int spyhip_psth_bin_rows(spyhip_ctx* ctx, const int64_t* sample_d, const int64_t* row_lo_d, const int64_t* row_hi_d,
                         const int64_t* start_d, const int64_t* onset_d, int64_t ntrials, const double* edges_d,
                         int64_t nedges, double samplerate, int64_t* rows_d);
/* out_d (ntrials, nbins, ncols) float32, every element written once: NaN for the bins outside [lohi_d[2 t],
 * lohi_d[2 t + 1]) (int32 pairs: the mask of psth.py:133-155, worked out by the host), else (float)(count * scale) with
 * the product in float64: scale = 1 for "spikecount" (and ahead of spyhip_psth_proportion), 1 / np.diff(edges)[0] for
 * "rate".  lut_d[c * nunit + u] (int32) = the column of (c, u), or -1 for a pair that is not selected. */
int spyhip_psth_count(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d, const int64_t* rows_d,
                      const int32_t* lut_d, int64_t nchan, int64_t nunit, const int32_t* lohi_d, int64_t ntrials,
                      int64_t nbins, int64_t ncols, double scale, float* out_d);
/* output = "proportion", in place on the out_d of spyhip_psth_count(scale = 1).  Per trial and column (c, u), in
 * float64: v[b] = count[b] / (edges[b + 1] - edges[b]) / S, S = the trial's selected spikes of unit u with edges[0] <=
 * time <= edges[nbins] (histogram2d's density=True; 0 / 0 = NaN when the unit occurs in the trial but not in the
 * window), v = 0 for a unit that does not occur in the trial; NaN where the count is masked; then v[b] / nansum_b v[b]
 * with a sum of 0 replaced by 1, the sum taken in bin order, and one rounding to float32.  unit_k_d[u] (int32, nunit
 * entries) = dense index < nk of a unit that has a column, col_k_d[column] (int32) = the dense index of its unit; s_d =
 * ntrials * nk int32 of work space (S, or -1 for an absent unit, on return). */
int spyhip_psth_proportion(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d, const int64_t* row_lo_d,
                           const int64_t* row_hi_d, const int64_t* rows_d, const int32_t* lut_d, int64_t nchan,
                           int64_t nunit, const int32_t* unit_k_d, const int32_t* col_k_d, int64_t nk,
                           const double* edges_d, int64_t ntrials, int64_t nbins, int64_t ncols, int32_t* s_d,
                           float* out_d);

/* ---- operator arithmetic on data objects (datatype/arithmetic.py; datatype/methods/arithmetic.py: arithmetic_cF).
 * out = a (op) b, element by element, over the selected trials of a data object, in one launch.  A tensor is a matrix of
 * rows (time is the slowest axis of every data class) of `width` elements; `desc` holds four int64 per trial: the first
 * output row, the first base row, the first row of a full-tensor operand, and the trial's rows.  The output rows of the
 * trials follow each other (the result is stacked); the base rows may repeat, overlap and come in any order, which is
 * all that a trial selection, a repeated trial or a latency window needs.  desc is the host copy, which is checked
 * against a_rows, b_rows and out_rows (the tensors' row counts) before anything runs, desc_d the same table on the device.
 * chan / chan_d (host and device copy, or both NULL): nchan_out indices < nchan_in, a channel selection of the base whose
 * rows then have width / nchan_out * nchan_in elements (the channel axis is the fastest one).
 * The base is read as a_type and converted to out_type in the load: float32 -> any, float64 -> float64 / complex128,
 * complex64 -> complex64 / complex128, complex128 -> complex128.  The operand is of out_type already:
 *   mode SPYHIP_ARITH_SCALAR: b_re + i b_im, by value (rounded to out_type first, as NumPy does);
 *   mode SPYHIP_ARITH_BCAST : b_d, an array of b_rows ELEMENTS seen through a view of the trial's shape: the trial is
 *                             (rows, b_extent[1], b_extent[2], b_extent[3]) with b_extent[1..3] multiplying to width,
 *                             b_stride[0..3] the array's element stride along each axis, 0 where it broadcasts
 *                             (b_extent[0]: its rows, if b_stride[0] != 0: no trial may have more);
 *   mode SPYHIP_ARITH_FULL  : b_d, a tensor of b_rows rows of width elements, its trials' rows in desc.
 * Real arithmetic is IEEE: + - * /, the correctly rounded square root; no fast-math.  Complex products are the textbook
 * four multiplications (the compiler may fuse them), complex quotients NumPy's (Smith's method); float32 powers are
 * float64 powers rounded once.  SPYHIP_ARITH_RSUB / _RDIV are b - a and b / a; _SQUARE, _COPY, _ONES and _SQRT take no
 * operand (mode SCALAR) and are NumPy's fast paths of ** 2, 1, 0 and 0.5 (_COPY is also the cast); powers, squares, ones
 * and roots exist for the real types only, the reflected operations not for mode FULL: -1 for what is not provided.
 * Where every trial starts on a 16-byte boundary of the base, the result and the operand tensor, and there is no channel
 * selection, a lane moves 16 bytes of the base at a time, else single elements.  Asynchronous on the context's stream;
 * nothing is allocated; out_d must be neither a_d nor b_d. */
enum spyhip_arith_op {
    SPYHIP_ARITH_ADD = 0, SPYHIP_ARITH_SUB = 1, SPYHIP_ARITH_MUL = 2, SPYHIP_ARITH_DIV = 3, SPYHIP_ARITH_RSUB = 4,
    SPYHIP_ARITH_RDIV = 5, SPYHIP_ARITH_POW = 6, SPYHIP_ARITH_SQUARE = 7, SPYHIP_ARITH_COPY = 8, SPYHIP_ARITH_ONES = 9,
    SPYHIP_ARITH_SQRT = 10
};
enum spyhip_arith_mode { SPYHIP_ARITH_SCALAR = 0, SPYHIP_ARITH_BCAST = 1, SPYHIP_ARITH_FULL = 2 };
enum spyhip_arith_type { SPYHIP_ARITH_F32 = 0, SPYHIP_ARITH_F64 = 1, SPYHIP_ARITH_C64 = 2, SPYHIP_ARITH_C128 = 3 };
int spyhip_arith(spyhip_ctx* ctx, int op, int mode, int a_type, int out_type, const void* a_d, int64_t a_rows,
                 const void* b_d, int64_t b_rows, const int64_t* b_extent, const int64_t* b_stride, double b_re,
                 double b_im, const int64_t* desc, const int64_t* desc_d, int64_t ntrials, int64_t width,
                 const int32_t* chan, const int32_t* chan_d, int64_t nchan_out, int64_t nchan_in, void* out_d,
                 int64_t out_rows);

/* ---- data selection (datatype/selectdata.py; datatype/methods/selectdata.py: DataSelection, _selectdata).
 * out = the selected rows of a tensor, of every row the selected elements, stacked and contiguous, in one launch.  The
 * source is src_rows rows (time is the slowest axis of every data class) of extent[0] x extent[1] x extent[2] elements of
 * elem_bytes bytes (4, 8 or 16), C-order; elements move as raw bits, so NaN payloads and signed zeros arrive unchanged.
 * `desc` holds three int64 per trial: the first output row, the first source row and the trial's rows.  The output rows
 * of the trials follow each other; the source rows may repeat, overlap and come in any order, and a trial may have no
 * rows.  Inner axis i is taken whole (kind[i] = SPYHIP_SELECT_WHOLE), as the range [start[i], start[i] + count[i])
 * (_RANGE) or through count[i] int32 indices (_LIST), unsorted and repeated as they come; the lists of the LIST axes
 * follow each other in idx, in axis order.  desc and idx are the host copies, which are checked before anything runs,
 * desc_d and idx_d the same tables on the device (idx and idx_d both NULL without a list).  -1 for an element size other
 * than 4, 8 or 16, an output that is or overlaps the source, a trial outside src_rows or out_rows, output rows that
 * are not stacked, an index or a range outside its extent, and a count of 0.
 * Adjacent whole axes collapse (a selection of rows alone moves one contiguous run per trial).  A lane moves 16 bytes
 * where the length of the innermost contiguous run and every run's byte offset in both tensors (the base addresses
 * included) are multiples of 16, else one element; an index list on the fastest axis always means element lanes.  Lists
 * of up to 4096 entries in all are read from LDS, longer ones from global memory.  Asynchronous on the context's stream;
 * nothing is allocated, no atomics. */
enum spyhip_select_kind { SPYHIP_SELECT_WHOLE = 0, SPYHIP_SELECT_RANGE = 1, SPYHIP_SELECT_LIST = 2 };
int spyhip_select(spyhip_ctx* ctx, int elem_bytes, const void* src_d, int64_t src_rows, const int64_t* extent,
                  const int32_t* kind, const int64_t* start, const int64_t* count, const int32_t* idx,
                  const int32_t* idx_d, const int64_t* desc, const int64_t* desc_d, int64_t ntrials, void* out_d,
                  int64_t out_rows);

/* ---- channel concatenation (datatype/concat.py; datatype/methods/concat.py: concat, concat_cF).
 * out = the rows of nsrc tensors (2 .. SPYHIP_CONCAT_MAX) side by side, in one launch.  Source s is src_rows[s] rows
 * (time is the slowest axis of every data class) of `pre` lines of run[s] elements of elem_bytes bytes (4, 8 or 16),
 * C-order; an output row is `pre` lines of W = run[0] + ... + run[nsrc - 1] elements, and in every line the run of
 * source s begins at element run[0] + ... + run[s - 1].  Elements move as raw bits, so NaN payloads and signed zeros
 * arrive unchanged.  Channel as the fastest axis: pre = the product of the axes between time and channel, run[s] = the
 * channels of s; channel in the middle: pre = 1, run[s] = channels x the axes behind them.  src_d, src_rows and run are
 * host arrays of nsrc entries (src_d: device pointers).  `desc` holds 2 + nsrc int64 per trial: the first output row,
 * the trial's rows, and the first row in each source.  The output rows of the trials follow each other; the source rows
 * may repeat, overlap and come in any order, and a trial may have no rows.  desc is the host copy, which is checked
 * before anything runs, desc_d the same table on the device.  -1 for nsrc outside 2 .. SPYHIP_CONCAT_MAX, an element
 * size other than 4, 8 or 16, pre < 1 or a run < 1, a trial outside a source or outside out_rows, output rows that are
 * not stacked, an output that is or overlaps a source, a tensor too large for 64-bit byte offsets, and a base that is
 * not aligned to its element type (8 bytes for 16-byte elements).
 * A lane moves 16 bytes where every run[s] * elem_bytes is a multiple of 16 and every base address lies on a 16-byte
 * boundary (every line and run offset then does too), else one element.  Consecutive lanes take consecutive output
 * addresses and every output byte is written exactly once.  Asynchronous on the context's stream; nothing is
 * allocated, no atomics, no LDS. */
#define SPYHIP_CONCAT_MAX 8
int spyhip_concat(spyhip_ctx* ctx, int elem_bytes, int nsrc, const void* const* src_d, const int64_t* src_rows,
                  const int64_t* run, int64_t pre, const int64_t* desc, const int64_t* desc_d, int64_t ntrials,
                  void* out_d, int64_t out_rows);

/* ---- synthetic data (synthdata.py; syncopy/synthdata/analog.py).  The deterministic part of a trial, assembled from
 * random numbers that the HOST drew (there is no device random stream, so every result has a reference value for every
 * seed).  Every tensor is (ntrials, nsamples, nchan), C-order.  Asynchronous on the context's stream; nothing is
 * allocated, no atomics, no workgroup waits on another.
 *
 * spyhip_synth_ar2: the network of coupled AR(2) processes.  noise_d holds the float64 innovations; out[t][0] and
 * out[t][1] are noise[t][0] and noise[t][1] rounded to float32, and for i >= 2
 *     acc = sum_j M[c][j] * (double)out[t][i-1][j]      (float64, ascending j, fused multiply-adds)
 *     v   = (float)(acc + (double)((float)alpha2 * out[t][i-2][c]))
 *     out[t][i][c] = (float)((double)v + noise[t][i][c])
 * with M = diag(alpha1) + AdjMat.T.  The coupling is the CSR table of the non-zeros of AdjMat.T: receiver c has the
 * senders col[rowptr[c] .. rowptr[c + 1]), strictly ascending, with the float32 weights w; alpha1 joins the sum at j = c
 * (added to the table's weight in float64 where the table has a diagonal entry).  rowptr and col are the host copies,
 * which are checked before anything runs, rowptr_d, col_d and w_d the table on the device (col, col_d and w_d may be
 * NULL for an empty table).  -1 for fewer than 2 samples, nchan outside 1 .. 1024, a tensor too large for 64-bit
 * offsets and a malformed table.  With an entry off the diagonal one workgroup walks a trial, one thread per channel,
 * the table in LDS where it fits; without one, one thread walks each (trial, channel) series.
 *
 * spyhip_synth_phase: phase diffusion.  wn_d is float32 white noise, lin_d (nsamples) the linear phase, ps0_d (ntrials, nchan)
 * the initial phases: phase[t][i][c] = (lin[i] + ps0[t][c]) + S[t][i][c], S the running float32 sum of (float)rel_eps * wn in
 * sample order (np.cumsum's); out is the phase, or cosf(phase) where want_cos is set.  All float32, single operations.
 *
 * spyhip_synth_tile: out[t][i][c] = col_d[i] (nsamples float32 values), in 16-byte lanes where nchan is a multiple of 4
 * and out_d lies on a 16-byte boundary. */
int spyhip_synth_ar2(spyhip_ctx* ctx, const double* noise_d, int64_t ntrials, int64_t nsamples, int nchan, double alpha1,
                     double alpha2, const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_d,
                     const int32_t* col_d, const float* w_d, float* out_d);
int spyhip_synth_phase(spyhip_ctx* ctx, const float* wn_d, const float* lin_d, const float* ps0_d, double rel_eps,
                       int64_t ntrials, int64_t nsamples, int nchan, int want_cos, float* out_d);
int spyhip_synth_tile(spyhip_ctx* ctx, const float* col_d, int64_t ntrials, int64_t nsamples, int nchan, float* out_d);

#ifdef __cplusplus
}
#endif
#endif /* SPYHIP_H */
