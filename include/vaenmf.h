/*
 * vaenmf.h -- C ABI of libvaenmf.so: the MI355X (gfx950) engine for the VAE-NMF
 * "reconstruct" hot path of sp-uhh/guided-vae-nmf.
 *
 * The reference has no FFI boundary (it is pure Python on torch); the boundary it
 * does have is the Python object surface that scripts/evaluate_M1.py:111-166 and
 * scripts/evaluate_M2_vad.py:95-166 touch (python/models/mcem.py MCEM_M1/MCEM_M2,
 * python/models/models.py, python/processing/stft.py).  Each entry point below
 * names the reference lines it replaces; guided-vae-nmf_amd/vaenmf binds them with
 * ctypes and re-creates that Python surface on top.
 *
 * Conventions
 *   - every function returns 0 on success or a negative code; vaenmf_last_error()
 *     returns a thread-local message.  Nothing throws.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  All work is
 *     enqueued asynchronously; no call synchronises the device unless stated.  Every kernel, memset and copy of a call goes
 *     to the stream it is given and to no other, the null stream included; a call that does not say that it waits returns
 *     while its stream is still busy, and -- once the tables of its first use are on the device -- may be made while the
 *     caller captures that stream into a graph: device buffers, maps and seeds are read when the graph runs, host tables and
 *     scalars when it is captured.  Two calls may not be captured: vaenmf_em_run and vaenmf_bind_batch_async (see there).
 *     tests/test_gpu_streams.py holds every entry point to this paragraph.
 *   - pointers marked DEV are device pointers owned by the caller (e.g. the
 *     PyTorch-ROCm allocator), never freed by the callee.  Required alignment: 16 bytes, and no more: the rows of X, X2,
 *     Vb, W, Ht, Z, Zs, B1, the replay draws and every [..][Fs] output are read and written with 16-byte vector accesses,
 *     and their row strides (Fs, Kp, Lp, H1 floats) are multiples of 16 bytes; g, u, acc_out, y, cost_frames and cost are
 *     accessed element by element and need their natural alignment only.  Required size: exactly the extent stated, not
 *     one byte more -- no entry point writes outside it (tests/test_gpu_buffer_contract.py); reads are kept inside by the
 *     buffer resources of the wave chains, the frame and sample clamps and the bin masks of the other kernels.
 *     Pointers marked HOST are host memory read during the call.
 *   - no allocation happens after vaenmf_plan_create / vaenmf_set_decoder_weights /
 *     vaenmf_bind_batch.
 *
 * Data layout in HBM (all "frame-major": one row per STFT frame, frames of all
 * utterances of the bound batch concatenated, NT = total frames)
 *   Fs  = F rounded up to 16        (query VAENMF_Q_FS)    feature row stride
 *   Kp  = 8, 16 or 32 (>= K)        (query VAENMF_Q_KP)    padded NMF rank
 *   Lp  = 32, or 128 on a wide plan (query VAENMF_Q_LP)    latent row stride
 * The padding of a row -- bins F..Fs-1, ranks K..Kp-1, latent columns L..Lp-1, sample rows nsamples..Rcap-1 -- is one of
 *   must be zero     the caller's duty when it fills the buffer (results are undefined otherwise);
 *   ignored          any bits, NaN included: no result depends on them;
 *   written as zero  by every entry point that writes the buffer;
 *   left alone       neither read into a result nor written.
 * One buffer needs a fifth word, `must be finite`: zero or any finite value; a NaN or Inf there reaches results.
 *
 *   buffer                                                    padding as an input      padding as an output
 *   X2  float  [NT][Fs]   mixture power spectrogram |X|^2     ignored                  vaenmf_power_spec: |X|^2 of X's padding
 *                         (mcem.py:47, transposed)                                     (zero, as X's must be zero)
 *   X   float2 [NT][Fs]   mixture STFT, complex64             must be zero             vaenmf_stft_batch_ex: written as zero
 *                         (mcem.py:46, transposed)            (the Wiener filters write mask * X there with mask = 0: a
 *                                                             finite value still gives the zeros promised for S_hat / N_hat,
 *                                                             a NaN or Inf shows in their padding)
 *   Vb  float  [NT][Fs]   fixed noise PSD                     ignored                  --
 *                         (vaenmf_set_noise_psd)
 *   W   float  [U][Fs][Kp] NMF dictionary per utterance       must be zero             written as zero (vaenmf_init_nmf,
 *                         (mcem.py:48)                        (bins and ranks)         the M-steps, vaenmf_em_run)
 *   Ht  float  [NT][Kp]   NMF activations, transposed         must be zero             written as zero (the same)
 *                         (mcem.py:49)
 *   g   float  [NT]       per-frame gain (mcem.py:51)         --                       --
 *   Z   float  [NT][Lp]   last draw of the latent variables   must be zero             written as zero (update_Z != 0),
 *                         (mcem.py:368, transposed)                                    else left alone like all of Z
 *   Zs  float  [NT][Rcap][Lp] posterior samples (mcem.py:386) columns L..Lp-1 of the   columns L..Lp-1 of the nsamples rows:
 *                                                             R rows read: must be     written as zero; rows nsamples..Rcap-1:
 *                                                             zero; rows R..Rcap-1:    left alone
 *                                                             ignored
 *   B1  float  [NT][H1]   per-frame first-layer bias b1 + W1[:,L:] y_n  (M2: the label part of decoder(cat([Z,y]))
 *                         folded once, mcem.py:242); NULL = M1                          --
 *   eps float  [S][NT][Lp] replay draws (vaenmf_rng)          wide plan: ignored.      vaenmf_rng_fill: finite draws (a narrow
 *                                                             Narrow plan with L = 16: plan fills all 32 columns)
 *                                                             must be finite (the wave chains multiply columns 16..31
 *                                                             by a zero step instead of masking them)
 *   u, acc_out float [S][NT]; cost_frames double [NT]; cost double [U][niter]           no padding
 *   S_hat, N_hat float2 [NT][Fs]; WFs, WFn float [NT][Fs];    --                       written as zero
 *   Vs_out of vaenmf_decode float [NT][R][Fs]
 *   Vs_out of vaenmf_sample_store_gather [NT][nsamples][Fs]   --                       unspecified (inside the buffer)
 * Rows: no entry point touches a row >= NT (>= U for W) of any buffer, whatever the tiling of the batch leaves idle.
 *
 * Supported value range
 *   The chain's energy takes one logarithm and one reciprocal for two bins, log(Vx0 Vx1) and
 *   (X2_0 Vx1 + X2_1 Vx0) / (Vx0 Vx1) with Vx = g Vs + (W H); the cost of the stored M-step does the same
 *   for two sample rows of a bin; the M-step squares 1 / Vx (as the reference does).  Supported
 *   are inputs for which every such product -- Vx of bins f and f + 2 of a group of four, Vx of
 *   the same bin in neighbouring samples, |X|^2 of one bin times Vx of its partner, and Vx^2 --
 *   is a normal float32, [2^-126, 2^128).  The range holds per PAIR, not per value: Vx = 1e-25
 *   next to Vx = 1e5 is fine, two neighbours at 1e-20 are not.  With Vx and |X|^2 inside
 *   [1e-19, 1.8e19] every pair is.  Outside it nothing is reported: v_rcp_f32 / v_log_f32 flush
 *   denormals, a product that under- or overflows gives an infinite energy or inf - inf, and the
 *   results of that frame -- from the next M-step on those of its utterance -- are non-finite or
 *   wrong.  Utterances do not share sums: a non-finite
 *   utterance leaves the others of its batch bit for bit as they are without it.  int16-scaled
 *   audio at full scale (|X|^2 <= 2^48.6 at n_fft 1278, the longest window F <= 640 allows) and
 *   audio at -80 dBFS with 80 dB of range inside a frame lie 2^10 and more inside.
 */
#ifndef VAENMF_H
#define VAENMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vaenmf_plan vaenmf_plan;

enum { VAENMF_PREC_BF16X3 = 0,   /* bf16 MFMA, 3-term hi/lo split, fp32 accumulate (~fp32 accuracy) */
       VAENMF_PREC_BF16   = 1 }; /* plain bf16 MFMA, fp32 accumulate                                   */

enum { VAENMF_RNG_REPLAY = 0,    /* caller supplies the normal / uniform draws (parity runs)          */
       VAENMF_RNG_DEVICE = 1 };  /* counter-seeded xoshiro128+ / Box-Muller streams on the device     */

enum { VAENMF_Q_FS = 0, VAENMF_Q_KP = 1, VAENMF_Q_TILES = 2, VAENMF_Q_NT = 3, VAENMF_Q_NUTT = 4,
       VAENMF_Q_MSTEP_PATH = 5,  /* M-step path of the last vaenmf_em_run: 1 = streaming the sample store, 2 = decoding */
       VAENMF_Q_WTILES = 6,      /* 16-frame wave tiles of the bound batch */
       VAENMF_Q_EM_GRAPH = 7,    /* 1 when the last vaenmf_em_run was launched as a captured HIP graph, 0 when launch by launch */
       VAENMF_Q_W_FUSED = 9,     /* 1 when the last stored M-step ran the W statistics fused with the W update's sums over frames
                                    (2: per 16-frame group, the small-batch form; the same bits) */
       VAENMF_Q_CHAIN_KERNEL = 10, /* kernel of the last MH chain: 0 = team kernel (64-bit addresses), 1 = one wavefront per 16 frames,
                                      2 = four wavefronts per 16 frames (bench shape, batches of at most one wave tile per CU),
                                      3 = the wide-decoder kernel (a workgroup of four wavefronts per 16 frames; wide plans only) */
       VAENMF_Q_LP = 11,         /* latent columns Lp of Z, Zs and the replay draws: 32, or 128 on a wide plan (L > 32 or a hidden layer of 256) */
       VAENMF_Q_STORE_ALIGNED = 12, /* 1 when the last MH chain that filled the sample store wrote the line-aligned layout (vaenmf_store_layout) */
       VAENMF_Q_DEV_ALLOCS = 8 };/* device allocations the library has made in this process so far (any plan): a caller that
                                    reuses a plan can check that a call allocated nothing */

enum { VAENMF_ACT_NONE = 0, VAENMF_ACT_TANH = 1, VAENMF_ACT_RELU = 2, VAENMF_ACT_SIGMOID = 3,
       VAENMF_ACT_STEP = 4,     /* 1 if x > 0 else 0: sigmoid(x) > 0.5, scripts/evaluate_M2_vad.py:131 */
       VAENMF_ACT_EXP = 5 };    /* the training layers only (vaenmf_train_dense_*): the decoder's output, models.py:133 */

typedef struct {
  int32_t F;          /* frequency bins, n_fft/2+1: any value in 1..640 (n_fft need not be a power of two; padding bins
                         F..Fs-1 of every output are zero)                          */
  int32_t K;          /* NMF rank (<= 32)                                           */
  int32_t L;          /* latent dimension: 16, 32, 64 or 128                        */
  int32_t H1, H2;     /* decoder hidden sizes, first and second layer (decoder.hidden.0 / .1, which the reference builds over
                         reversed(h_dim), models.py:133): (128,128), (128,0) = one hidden layer, (128,256) = h_dim [256,128],
                         (256,128) = h_dim [128,256].  A plan with L > 32 or a 256-wide layer is WIDE: Lp = 128 latent columns,
                         the MH chain is the wide kernel, and the M-step / Wiener filter exist in their stored forms only (see
                         vaenmf_sample_store)                                                                                */
  int32_t max_frames; /* capacity: total frames of a bound batch                    */
  int32_t max_utts;   /* capacity: utterances of a bound batch                      */
  int32_t precision;  /* VAENMF_PREC_*                                              */
} vaenmf_config;

typedef struct {
  int32_t  mode;        /* VAENMF_RNG_*                                             */
  uint32_t call;        /* chain-invocation counter (EM iteration index; WF = niter) */
  const float* eps;     /* DEV [S][NT][Lp] N(0,1) draws, step-major  (REPLAY only; mcem.py:407) */
  const float* u;       /* DEV [S][NT]    U(0,1) draws               (REPLAY only; mcem.py:420) */
} vaenmf_rng;

const char* vaenmf_last_error(void);

/* Plan = shapes + device-resident decoder weights + batch tiling + workspace. */
int  vaenmf_plan_create(const vaenmf_config* cfg, vaenmf_plan** out);
void vaenmf_plan_destroy(vaenmf_plan* p);
int  vaenmf_plan_query(const vaenmf_plan* p, int32_t what);

/* Decoder weights, HOST, nn.Linear layout [out][in] row-major as in the state_dict
 * keys decoder.hidden.{0,1}.{weight,bias}, decoder.reconstruction.{weight,bias}
 * (models.py:107-121).  in1 = L + Dy; the first L columns of W1 feed the MFMA path,
 * the remaining Dy columns are kept for vaenmf_layer1_bias. */
int vaenmf_set_decoder_weights(vaenmf_plan* p, const float* W1, int32_t in1, const float* b1,
                               const float* W2, const float* b2, const float* W3, const float* b3);

/* Bind a batch: frame_offsets HOST [n_utt+1] (frames of utterance u are rows
 * frame_offsets[u] .. frame_offsets[u+1]-1); utt_seeds HOST [n_utt] or NULL (device RNG
 * streams are keyed by (utt seed, frame index within the utterance), so results do not
 * depend on how utterances are batched). */
int vaenmf_bind_batch(vaenmf_plan* p, int32_t n_utt, const int32_t* frame_offsets,
                      const uint64_t* utt_seeds);
/* The same without waiting for the GPU when the batch's frame structure repeats the bound one:
 * the frame tables stay, the seeds go up stream-ordered from pinned memory.  A caller that never
 * synchronises (results collected later) can prepare batch k+1 while batch k runs.  A batch with
 * another frame structure synchronises `stream` and uploads the tables as vaenmf_bind_batch does.
 * STREAM CONTRACT: the seed upload is ordered on `stream` only -- the calls that consume the batch (vaenmf_mh_chain,
 * vaenmf_em_run, ...) must be enqueued on the same stream, or after an event / synchronisation that orders them behind it.
 * The pinned slot of the seeds is one of a ring of eight, guarded by an event the call records on `stream` and waits for
 * eight binds later: the call may not be called while a caller's stream capture is open (an event recorded into a graph cannot
 * be waited for), and a ninth bind behind work that has not run waits for the first. */
int vaenmf_bind_batch_async(vaenmf_plan* p, int32_t n_utt, const int32_t* frame_offsets,
                            const uint64_t* utt_seeds, void* stream);

/* EM.init_parameters (mcem.py:42-44, :51) for the bound batch on the device: W = max(U(0,1), eps) (F x K per utterance),
 * H = max(U(0,1), eps) (K x N), g = 1; padding zero.  Counter-based draws keyed by (utterance seed of vaenmf_bind_batch,
 * salt, element): an utterance's initialisation does not depend on the batch it sits in.  W DEV [U][Fs][Kp], Ht DEV
 * [NT][Kp], g DEV [NT].  (The drop-in classes draw W0 / H0 on the host in the reference's order instead.) */
int vaenmf_init_nmf(vaenmf_plan* p, float* W, float* Ht, float* g, uint64_t salt, float eps, void* stream);

/* B1[n][h] = b1[h] + sum_d W1[h][L+d] * y[n][d]   (label half of mcem.py:242/261/283).
 * y DEV [NT][Dy]. */
int vaenmf_layer1_bias(vaenmf_plan* p, const float* y, int32_t Dy, float* B1, void* stream);

/* Fixed noise variance for the *_noNMF variants (EM_noNMF / MCEM_M2_noNMF, mcem.py:493-760): Vb DEV [NT][Fs]
 * (caller-owned, must stay valid) replaces W H in every later call and vaenmf_m_step then updates the gains only
 * (mcem.py:543-578); NULL restores the NMF noise model. */
int vaenmf_set_noise_psd(vaenmf_plan* p, const float* Vb);

/* Metropolis-Hastings chain of one E-step / Wiener phase -- replaces
 * MCEM_M1.sample_posterior (mcem.py:371-441) and MCEM_M2.sample_posterior (:218-294):
 * nsamples+burnin random-walk steps per frame, samples after burn-in to Zs[:, 0..nsamples-1, :].
 * update_Z != 0: Z is overwritten with the last draw, as E_step does (mcem.py:466);
 * update_Z == 0: Z is only read, as compute_WF does (mcem.py:477-478).  acc_out (DEV
 * [S][NT], may be NULL) receives the log-acceptance of every step (mcem.py:415-417).
 * Zs may be NULL on a wide plan and where the wave-private chain kernels run (vaenmf_wchain_addressable; every narrow shape
 * but F > 528 and bf16x3 with F > 272): the samples are then not recorded -- with the sample-variance store on nothing reads them (vaenmf_em_run does
 * this for its E-steps). */
int vaenmf_mh_chain(vaenmf_plan* p, const float* X2, const float* W, const float* Ht, const float* g,
                    float* Z, int32_t update_Z, const float* B1, float* Zs, int32_t Rcap,
                    int32_t nsamples, int32_t burnin, float var_rw,
                    const vaenmf_rng* rng, float* acc_out, void* stream);

/* 1 when the wave-private chain kernel (32-bit buffer offsets per lane) can address every buffer of a batch of NT frames
 * (Zs [NT][Rcap][L], the replay draws [steps][NT][L], X2 [NT][Fs], W [n_utt][Fs][Kp], ...), 0 when vaenmf_mh_chain runs
 * the 64-bit team kernel for it instead.  Pure host arithmetic (no GPU needed). */
int vaenmf_wchain_addressable(int64_t NT, int32_t Rcap, int32_t steps, int32_t Fs, int32_t Kp, int32_t n_utt, int32_t replay);

/* The draws the DEVICE generator hands to step s of chain invocation rng->call:
 * eps_out DEV [S][NT][Lp], u_out DEV [S][NT].  Test/debug aid: a REPLAY run fed with
 * these buffers is bit-identical to the DEVICE run.  (Lp / 4 streams of four latents per frame.) */
int vaenmf_rng_fill(vaenmf_plan* p, uint32_t call, int32_t S, float* eps_out, float* u_out, void* stream);

/* Vs = decoder(Z_samples): replaces compute_Vs (mcem.py:444-454 / :297-307).
 * Vs_out DEV [NT][R][Fs] (the reference's (R,F,N) tensor, frame-major).
 * vaenmf_decode, vaenmf_m_step and vaenmf_wiener return an error on a wide plan: there the chain's sample store
 * (vaenmf_sample_store, vaenmf_sample_store_gather, vaenmf_m_step_stored, vaenmf_wiener_stored) is the only path. */
int vaenmf_decode(vaenmf_plan* p, const float* Zs, int32_t Rcap, int32_t R, const float* B1,
                  float* Vs_out, void* stream);

/* One M-step -- replaces EM.M_step (mcem.py:90-152) plus
 * compute_expected_neg_log_like (:68-70): multiplicative updates of W, H (exponent 1/2),
 * L1 column normalisation, gain update.  The R posterior samples are re-decoded on
 * chip instead of being streamed from HBM.  W, Ht, g are updated in place.
 * cost_frames DEV [NT] double: sum_{r,f}(log Vx + X2/Vx) per frame (after the update);
 * the mean over (R,F,N) of an utterance is mcem.py:70. */
int vaenmf_m_step(vaenmf_plan* p, const float* X2, float* W, float* Ht, float* g,
                  const float* Zs, int32_t Rcap, int32_t R, const float* B1,
                  double* cost_frames, void* stream);

/* Wiener filter from the R samples in Zs -- replaces compute_WF's averaging
 * (mcem.py:486-488) and the complex products of EM.run (:175-176):
 * S_hat = mean_r(g Vs/Vx) * X,  N_hat = mean_r(Vb/Vx) * X.   X, S_hat, N_hat DEV
 * complex64 [NT][Fs] (interleaved re,im); WFs/WFn DEV [NT][Fs] optional (NULL). */
int vaenmf_wiener(vaenmf_plan* p, const float* X2, const float* W, const float* Ht, const float* g,
                  const float* Zs, int32_t Rcap, int32_t R, const float* B1,
                  const float* X, float* S_hat, float* N_hat, float* WFs, float* WFn, void* stream);

/* Fused driver -- replaces EM.run (mcem.py:155-178) for the whole bound batch with no
 * host synchronisation per iteration: niter x (E-step, M-step, cost), then the Wiener
 * chain and filter.  cost DEV [n_utt][niter] double.  (nsE, biE) / (nsWF, biWF) are the
 * EFFECTIVE sample/burn-in counts (the caller applies MCEM_M1's positional-shift quirk,
 * mcem.py:461-462).  Device RNG only (rng_mode REPLAY is served step by step by the
 * calls above).  On a wide plan the sample store must be on (there is no decoding path); a batch
 * whose store would not fit is an error, not a fall back.
 * A call signature (buffers, shapes, frame offsets, counts, var_rw, the kernel switches) runs launch
 * by launch at its first appearance on a plan, is captured into a HIP graph at its second --
 * whatever other calls came between -- and is replayed from then on: one launch per call instead
 * of ~600.  A plan keeps four graphs (the least recently used one is dropped, and captured again
 * when its signature returns) and remembers the last eight signatures it has run once; one that has
 * been forgotten starts over with a launch-by-launch call.  The batch's contents (spectrogram,
 * seeds, frame tables) sit behind the same pointers and are read at run time.  Profiling
 * (vaenmf_profile_*) and VAENMF_GRAPH=0 keep the launch-by-launch path; results are the same
 * either way.  The graphs are captured on a stream of the plan's own and launched on `stream`: vaenmf_em_run itself may not be
 * called while a caller's stream capture is open. */
int vaenmf_em_run(vaenmf_plan* p, const float* X2, float* W, float* Ht, float* g, float* Z,
                  const float* B1, float* Zs, int32_t Rcap, int32_t niter,
                  int32_t nsE, int32_t biE, int32_t nsWF, int32_t biWF, float var_rw,
                  const float* X, float* S_hat, float* N_hat, double* cost, void* stream);

/* Dense layer Y = act(X Wt^T + b): encoder / classifier forwards
 * (models.py:101-104, 33-38, 57-62).  X DEV [M][in], Wt DEV [out][in], b DEV [out],
 * Y DEV [M][ldy] (first `out` columns written). */
int vaenmf_dense(const float* X, int32_t M, int32_t in, int32_t ldx, const float* Wt, const float* b,
                 int32_t out, int32_t act, float* Y, int32_t ldy, void* stream);

/* Sample-variance store.  With the store enabled, vaenmf_mh_chain also writes the decoded
 * variances Vs = exp(decoder(Z')) of every post-burn-in proposal (they are in registers
 * anyway) to a plan-owned buffer VsS DEV [NT][Rs][Fs], Rs = nsamples + 1 -- float rows in
 * bf16x3 mode, bf16 rows in bf16 mode (half the traffic; rounding of the size the bf16
 * decoder products carry anyway) -- and a map
 * src DEV int32 [Rs][NT]: the variances of sample r of frame n (the state after post-burn-in
 * step r, mcem.py:429-437) are the row VsS[n][src[r][n]] (at F = 257 and 513 the rows are kept on whole 128-byte lines,
 * without their odd last bin: vaenmf_store_layout below).  The M-step and the Wiener
 * filter can then stream the samples' variances from HBM instead of decoding Zs again
 * (vaenmf_m_step_stored, vaenmf_wiener_stored; vaenmf_em_run does so by itself).  The store
 * describes the most recent vaenmf_mh_chain call only.  vaenmf_sample_store_gather copies
 * the samples' rows out densely, Vs_out DEV float [NT][nsamples][Fs] (what vaenmf_decode
 * computes from Zs; bins >= F unspecified).
 * vaenmf_sample_store(plan, max_samples): max_samples > 0 switches the store on and sizes it -- an ALLOCATING call,
 * like vaenmf_plan_create -- for the bound batch (call it after vaenmf_bind_batch; before any batch is bound: for
 * the plan's frame capacity) and chains of up to max_samples samples per frame; 0 switches it off (memory kept).
 * vaenmf_mh_chain never allocates: it fails with a message if the store is too small for its batch. */
int vaenmf_sample_store(vaenmf_plan* plan, int32_t max_samples);
int vaenmf_sample_store_gather(vaenmf_plan* plan, float* Vs_out, void* stream);
/* Where the store keeps its rows, in elements of elt_bytes (2: bf16 rows, 4: float rows).  Bin f < row of (frame n, slot s)
 * is element n * frame + s * row + f; bin F-1 is element xbase + n * xframe + s * xslot.  With aligned != 0 and F = 257 or
 * 513 a row holds bins 0..F-2 alone (whole 128-byte lines) and the odd bins F-1 of a frame's Rs slots form one block padded
 * to 64 bytes, the blocks behind the rows of all `frames` frame blocks; otherwise a row is Fs elements with bin F-1 inside it.
 * HOST out7: row, frame, xslot, xframe, xbase, aligned (the layout in effect), bytes of the whole store.  Pure host
 * arithmetic (no GPU needed).  The library picks the aligned layout by itself; VAENMF_STORE_ALIGNED=0 keeps the padded one. */
int vaenmf_store_layout(int32_t F, int32_t Fs, int32_t elt_bytes, int32_t Rs, int64_t frames, int32_t aligned, int64_t* out7);
/* vaenmf_m_step / vaenmf_wiener over the store of the most recent chain (same updates, same
 * outputs; the samples are the store's, so no Zs / B1 arguments). */
int vaenmf_m_step_stored(vaenmf_plan* plan, const float* X2, float* W, float* Ht, float* g,
                         double* cost_frames, void* stream);
int vaenmf_wiener_stored(vaenmf_plan* plan, const float* W, const float* Ht, const float* g,
                         const float* X, float* S_hat, float* N_hat, float* WFs, float* WFn,
                         void* stream);

/* |X|^2 (mcem.py:47): X DEV complex64 [n], X2 DEV float [n]. */
int vaenmf_power_spec(const float* X, float* X2, int64_t n, void* stream);

/* STFT front end -- replaces python/processing/stft.py:16-63 (librosa.core.stft).
 * Any n_fft in [16, 4096]; every entry rejects other lengths with a message.
 * vaenmf_stft_geometry applies the integer-window check (:37-38) and the end-pad rule
 * (:48-53) on the host and returns n_fft, hop, the frame count and the padded length Tp
 * of one utterance: 1 + (Tp + 2*(n_fft/2) - n_fft)/hop frames with center (librosa pads
 * n_fft/2 samples on both sides), 1 + (Tp - n_fft)/hop without (fails when Tp < n_fft).
 * vaenmf_stft_batch_ex: wav DEV float [sum T]; sample_offsets DEV int64 [n_utt+1];
 * frame_offsets DEV int32 [n_utt+1]; frame_utt DEV int32 [NT]; padded_len DEV int32
 * [n_utt]; X DEV complex64 [NT][Fs] (Fs >= n_fft/2+1, bins >= n_fft/2+1 zeroed); the
 * window, the centring and the pad mode come from `opts` (the reference's own: periodic
 * Hann, center, reflect padding).  Reflect padding is np.pad(mode="reflect") of the
 * end-padded signal at any length: a signal shorter than the n_fft/2 samples of padding is
 * reflected as often as needed (period 2 (Tp - 1); a single sample is repeated).
 * Kernels: power-of-two n_fft <= 2048 with periodic Hann, center and reflect padding run
 * the radix-2 kernels; everything else a mixed-radix (radices 2, 3, 4, 5, 7) or, for
 * lengths with a prime factor above 7, a Bluestein FFT.  Per-size twiddle / chirp tables
 * are built and uploaded on the first call with that size on a device and kept.
 * The transform runs in float64 and is rounded once to complex64 like the reference. */
#define VAENMF_PAD_REFLECT 0
#define VAENMF_PAD_CONSTANT 1
typedef struct vaenmf_stft_opts {
  int32_t nfft;           /* window / transform length, [16, 4096]                      */
  int32_t hop;            /* hop in samples                                             */
  int32_t center;         /* 1: frames centred, padded by n_fft/2 on both sides         */
  int32_t pad_mode;       /* VAENMF_PAD_REFLECT or VAENMF_PAD_CONSTANT (zeros)          */
  const double* window;   /* DEV float64 [nfft] analysis / synthesis window; NULL: Hann  */
} vaenmf_stft_opts;
int vaenmf_stft_geometry(int64_t n_samples, double fs, double wlen_sec, double hop_percent,
                         int32_t center, int32_t* nfft, int32_t* hop, int32_t* n_frames,
                         int32_t* n_padded);
int vaenmf_stft_batch_ex(const float* wav, int32_t n_frames_total, const int64_t* sample_offsets,
                         const int32_t* frame_offsets, const int32_t* frame_utt,
                         const int32_t* padded_len, const vaenmf_stft_opts* opts, int32_t Fs,
                         float* X, void* stream);
/* iSTFT back end -- replaces stft.py:66-102 (librosa.core.istft with length=max_len,
 * window-sum-square normalised overlap-add): S DEV complex64 [NT][Fs] -> wav_out DEV
 * float [sum T] (T = sample_offsets[u+1]-sample_offsets[u] = max_len of utterance u;
 * samples past the last frame are zero); work DEV float [NT][nfft] scratch (the windowed
 * frames).  With center the first n_fft/2 samples of the overlap-add are dropped.
 * Window and centring come from `opts` (pad_mode is not used). */
int vaenmf_istft_batch_ex(const float* S, int32_t n_utt, int32_t n_frames_total,
                          const int64_t* sample_offsets, const int32_t* frame_offsets,
                          const vaenmf_stft_opts* opts, int32_t Fs, float* work,
                          float* wav_out, void* stream);

/* Rational-ratio resampler -- replaces the librosa.resample calls of python/dataset/qut_database.py and
 * demand_database.py (preprocess_noise) and lets audio at another rate than the model's enter and leave on the device.
 * It is scipy.signal.resample_poly(x, up, down, window=('kaiser', beta)) with zero padding in closed form: with
 * M = max(up, down), half = zeros M and the 2 half + 1 taps
 *   h[i] = up s[i] w[i] / sum_j s[j] w[j],   t = i - half,   s[i] = sin(pi t / M) / (pi t)  (1 / M at t = 0),
 *   w[i] = I0(beta sqrt(1 - (t / half)^2)) / I0(beta)                   (scipy's defaults: zeros = 10, beta = 5.0)
 * an utterance of n_in samples gives n_out = ceil(n_in up / down) samples
 *   y[m] = sum_n x[n] h[half + m down - n up],   n in [0, n_in) with the tap index in [0, 2 half]
 * (x is zero outside its own utterance: nothing leaks between the utterances of a batch).  The taps are float64 (built in
 * long double, I0 by its power series, rounded once), the sum runs in float64 in ascending n and is rounded once to
 * float32, so an utterance has the same bits in any batch.
 * vaenmf_resample_ratio, HOST only: up = fs_out / g, down = fs_in / g, g = gcd(fs_in, fs_out), rates in Hz; -1 for a rate
 *   <= 0, -3 when up or down exceeds 1024 (the message names the limit).
 * vaenmf_resample_length, HOST only: ceil(n_in up / down), or -1 on bad arguments.
 * vaenmf_resample_taps, HOST only: h HOST float64 [2 zeros max(up, down) + 1], natural order, for up / down AS GIVEN (it
 *   does not reduce them) -- the values vaenmf_resample_batch uploads for its reduced ratio.  up, down <= 1024 (else -3),
 *   zeros in [1, 64], beta in [0, 100].
 * vaenmf_resample_batch: x DEV float [in_offsets[n_utt]], y DEV float [out_offsets[n_utt]], natural (4-byte) alignment,
 *   read and written element by element: no read leaves [in_offsets[u], in_offsets[u+1]), no write leaves [out_offsets[u],
 *   out_offsets[u+1]).  in_offsets / out_offsets HOST int64 [n_utt+1], non-decreasing; the ratio is reduced by its gcd
 *   first, and every out_offsets[u+1] - out_offsets[u] must equal vaenmf_resample_length of the utterance's input length
 *   (else -1).  up == down is one device copy; n_utt == 0 and empty utterances are no-ops.  The tap table is built and
 *   uploaded at the first call with a (device, up, down, zeros, beta), the workgroup-to-utterance table at the first call
 *   with a batch shape (the offsets and the ratio; the 16 most recent shapes are kept): those calls allocate and wait for
 *   the upload, every later one only launches. */
int vaenmf_resample_ratio(int64_t fs_in, int64_t fs_out, int32_t* up, int32_t* down);
int64_t vaenmf_resample_length(int64_t n_in, int32_t up, int32_t down);
int vaenmf_resample_taps(int32_t up, int32_t down, int32_t zeros, double beta, double* h);
int vaenmf_resample_batch(const float* x, int32_t n_utt, const int64_t* in_offsets, const int64_t* out_offsets,
                          int32_t up, int32_t down, int32_t zeros, double beta, float* y, void* stream);

/* Long recordings as batches of short utterances (no reference counterpart: its scripts process utterances of a few
 * seconds).  A recording of n frames is cut on the frame grid into segments of L >= 2 frames that overlap by V frames,
 * 0 <= V <= L / 2: stride = L - V, m = max(1, floor((n - V) / stride)) segments, segment k starts at frame k stride,
 * segments 0 .. m-2 have L frames and the last one runs to frame n (n frames when m = 1, else L <= length < L + stride).
 * A recording of fewer than L + stride frames is one segment; every frame lies in one segment or in two consecutive ones,
 * every overlap has exactly V frames.  The i-th frame of an overlap (i = 0 .. V-1) is blended with the weight
 * w_b = float((i + 1) / (V + 1)) (double, rounded once) for the later segment and w_a = 1.0f - w_b (float) for the earlier.
 * Processing order of the segments of a batch: first every segment of L frames that is not its recording's last (recording
 * order, then segment order), then the recordings' last segments in recording order.  Segment rows are the frames of the
 * segments concatenated in that order; recording-order frames are the frames of the recordings concatenated.
 * vaenmf_segment_count, HOST only: frame_counts HOST int32 [n_utt], each >= 1.  *n_segments = sum of m, *n_segment_rows =
 *   sum of (n + (m - 1) V).  -1 (the message names the numbers) for L < 2, V < 0 or V > L / 2, or an empty recording.
 * vaenmf_segment_table, HOST only: fills, in processing order,
 *   seg_utt, seg_index, seg_first, seg_len  HOST int32 [n_segments]: the segment's recording, its index j inside the
 *                                           recording, its first frame j stride inside the recording, its length;
 *   src_row  HOST int32 [n_segment_rows]    the recording-order frame every segment row copies;
 *   row_a, row_b  HOST int32, w_b HOST float, [sum of frame_counts]: per recording-order frame the segment row that holds
 *                                           it -- row_b = -1 and w_b = 0 for a frame with one owner; in an overlap row_a is
 *                                           the earlier segment's row, row_b the later one's and w_b the later one's weight.
 *   Every array is written in full and nothing beside it.  Beyond the refusals of vaenmf_segment_count: -1 when the longest
 *   possible segment, L + stride - 1 frames, exceeds max_frames (the capacity of the plan that will run the segments), or
 *   when the segment rows exceed 2^31 - 1.
 * vaenmf_gather_rows: dst[r] = src[row_map[r]] for r < n_rows, rows of row_floats floats.  src DEV float [rows][row_floats]
 *   with rows > max(row_map) (the caller's duty: the map is not checked on the device), row_map DEV int32 [n_rows] (repeats
 *   allowed), dst DEV float [n_rows][row_floats], not overlapping src.  Rows are moved bit for bit, padding included.
 * vaenmf_blend_rows: for t < n_frames, dst[t] = seg[row_a[t]] bit for bit when row_b[t] < 0, else per float
 *   (1.0f - w_b[t]) seg[row_a[t]] + w_b[t] seg[row_b[t]] with each product rounded to float32 and then their sum (no fused
 *   multiply-add): the same bits whichever of the two operands is called a.  seg DEV float [rows][row_floats], row_a,
 *   row_b DEV int32 [n_frames], w_b DEV float [n_frames] (not read where row_b < 0), dst DEV float [n_frames][row_floats],
 *   not overlapping seg.  Padding bins need no mask: zeros blend to zeros.
 * Both kernels take any row_floats >= 0 and buffers of exactly the extents stated at their natural (4-byte) alignment:
 *   16-byte accesses are used when row_floats is a multiple of 4 and both float buffers are 16-byte aligned, float
 *   accesses otherwise.  No plan, no allocation, no synchronisation; every output row is written by its own lanes alone
 *   (no atomics), so a row's value does not depend on what else the call moves.  n_rows / n_frames = 0 is a no-op. */
int vaenmf_segment_count(int32_t n_utt, const int32_t* frame_counts, int32_t L, int32_t V, int64_t* n_segments,
                         int64_t* n_segment_rows);
int vaenmf_segment_table(int32_t n_utt, const int32_t* frame_counts, int32_t L, int32_t V, int32_t max_frames,
                         int32_t* seg_utt, int32_t* seg_index, int32_t* seg_first, int32_t* seg_len, int32_t* src_row,
                         int32_t* row_a, int32_t* row_b, float* w_b);
int vaenmf_gather_rows(const float* src, const int32_t* row_map, int64_t n_rows, int32_t row_floats, float* dst, void* stream);
int vaenmf_blend_rows(const float* seg, const int32_t* row_a, const int32_t* row_b, const float* w_b, int64_t n_frames,
                      int32_t row_floats, float* dst, void* stream);

/* Label / guide front-ends of the M2 path -- replace python/processing/target.py.
 * vaenmf_lorenz_labels: clean_speech_IBM (target.py:7-28, mode VAENMF_LABEL_IBM) and
 * clean_speech_VAD (:30-50, mode VAENMF_LABEL_VAD) for a batch of utterances: power =
 * |X|^2 (VAD: summed over the bins of a frame), descending sort per utterance, Lorenz
 * curve cumsum/sum, threshold = last sorted power whose Lorenz value is < quantile_fraction,
 * label = power > threshold ? hi : lo, where lo/hi are the caller's softened and rounded
 * values round(0.5 -/+ 0.5 quantile_weight) (:24-27).  The float32 arithmetic follows
 * numpy's operation order, so the 0/1 decisions are those of the reference bit for bit.
 * X DEV complex64 [NT][Fs]; frame_offsets HOST int32 [n_utt+1]; labels DEV float
 * [NT][ld] (IBM, bins < F written) or [NT] (VAD); thr_out DEV float [n_utt] or null;
 * work DEV scratch of vaenmf_lorenz_work_bytes() bytes.  Synchronises the stream; an
 * utterance with no Lorenz value below the fraction is the reference's IndexError. */
enum { VAENMF_LABEL_IBM = 0, VAENMF_LABEL_VAD = 1 };
int64_t vaenmf_lorenz_work_bytes(int32_t n_frames_total, int32_t F, int32_t n_utt, int32_t mode);
int vaenmf_lorenz_labels(const float* X, int32_t n_utt, const int32_t* frame_offsets, int32_t F,
                         int32_t Fs, int32_t mode, float quantile_fraction, float lo, float hi,
                         float* labels, int32_t ld, float* thr_out, void* work,
                         int64_t work_bytes, void* stream);
/* ideal_wiener_mask (target.py:104-116): |S|^2 / (|S|^2 + |N|^2 + eps), S, N DEV
 * complex64 [n], mask DEV float [n]. */
int vaenmf_wiener_mask(const float* S, const float* N, int64_t n, float eps, float* mask,
                       void* stream);
/* Supervised Wiener-mask baseline, scripts/evaluate_wiener_filter.py:99: S_hat = mask * X.
 * X, S_hat DEV complex64 [NT][Fs]; mask DEV float [NT][ldm] (bins < F read; bins >= F of
 * S_hat zeroed). */
int vaenmf_apply_mask(const float* X, const float* mask, int32_t ldm, int32_t NT, int32_t F,
                      int32_t Fs, float* S_hat, void* stream);

/* SPP-based speech-presence / noise-PSD estimator -- replaces SPPNoiseEstimator.update
 * driven frame by frame (python/models/spp_estimation.py:17-160; timo_mask_estimation
 * :163-183 is spp_out, the noise PSD the first return value).  per DEV float [NT][ld]
 * noisy periodogram |Y|^2, frame_offsets DEV int32 [n_utt+1]; the recursion runs in
 * float64 per (utterance, bin) and restarts at every utterance.  spp_out / psd_out DEV
 * float [NT][ldo], either may be null.  Defaults of the reference: fixed_smooth 0.8,
 * prob_smooth 0.9, prior 0.5, snr_opt_db 15, num_frames_init 10 (:10-14).
 * vaenmf_spp_noise_given: the v_spp_in branch (:145-153, timo_noise_estimation
 * :218-235), elementwise over n entries. */
int vaenmf_spp_estimate(const float* per, int32_t ld, int32_t n_utt, const int32_t* frame_offsets,
                        int32_t F, double fixed_smooth, double prob_smooth, double prior,
                        double snr_opt_db, int32_t num_frames_init, float* spp_out,
                        float* psd_out, int32_t ldo, void* stream);
int vaenmf_spp_noise_given(const float* per, const float* spp_in, int64_t n, double fixed_smooth,
                           float* psd_out, void* stream);

/* SI-SDR sufficient statistics -- python/metrics.py:12-60: per utterance the Gram
 * matrix of (s_hat, s, n) in float64: out DEV [n_utt][6] =
 * {<sh,sh>, <sh,s>, <sh,n>, <s,s>, <s,n>, <n,n>}; sample_offsets DEV int64 [n_utt+1]. */
int vaenmf_gram3_batch(const float* s_hat, const float* s, const float* n, int32_t n_utt,
                       const int64_t* sample_offsets, double* out, void* stream);

/* STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) -- replace pystoi's stoi(x, y, fs, extended) as the reference
 * calls it (scripts/run_metrics_M1.py / run_metrics_M2.py:117, extended=True) for ragged batches of device signals at
 * 10 kHz (another rate goes through vaenmf_resample_batch first).  clean x and processed y of one utterance have the same
 * T samples.  Constants: frame 256, hop 128, FFT 512, 15 third-octave bands from 150 Hz, segments of N = 30 frames,
 * beta = -15 dB, dynamic range 40 dB, EPS = 2^-52.  Everything below is float64 on the float32 samples.
 *   window     w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255: the symmetric Hann of 258 points without its two
 *              zero ends (numpy.hanning(258)[1:-1]).
 *   silence    frames start at 0, 128, .. < T - 256 (strictly: n_frames = ceil((T - 256) / 128) for T > 256, else 0; the
 *              last full frame is dropped when 128 divides T - 256).  e_j = 20 log10(||w x[128 j : 128 j + 256]|| + EPS),
 *              on the clean signal only; frame j is kept iff max_j e - 40 - e_j < 0.  k frames are kept, src[0 .. k-1]
 *              their indices in order.  Both signals are rebuilt by overlap-adding their kept windowed frames at hop
 *              128: sample 128 q + r (0 <= r < 128) is w[r] s[128 src[q] + r] (q <= k - 1) plus
 *              w[r + 128] s[128 src[q-1] + r + 128] (q >= 1); the length is 128 (k - 1) + 256.
 *   bands      frames of the rebuilt signals start at 0, 128, .. < length - 256: M = k - 1 frames, each windowed by w
 *              again, zero-padded to 512 and transformed.  tob[m][b] = sqrt(sum of |.|^2 over the bins lo_b <= bin <
 *              hi_b), lo_b / hi_b the bins of the grid 10000 i / 512 (i = 0 .. 256) nearest to 150 2^((2b-1)/6) and
 *              150 2^((2b+1)/6) Hz (least squared distance, the first index on a tie).
 *   segments   for m = 30 .. M the frames m-30 .. m-1 are one segment: J = M - 29 of them; with M < 30 the score is 1e-5
 *              (the value pystoi returns with a warning).
 *   ESTOI      in every segment and for both signals: each band row minus its mean over the 30 frames, divided by its
 *              2-norm; then each frame column minus its mean over the 15 bands, divided by its 2-norm.
 *              d = sum over the segments of sum(x_n y_n) / 30 / J.
 *   STOI       per segment and band row: c = ||x|| / (||y|| + EPS), y' = min(c y, x (1 + 10^(15/20))); x and y' minus
 *              their row means, each divided by (its norm + EPS); d = sum of x y' / (15 J).
 * Deviations from pystoi, both on purpose:
 *   - no dither.  pystoi adds EPS randn to the rows and columns it normalises, which makes the score of digital silence
 *     a random number; here a row or column whose norm is exactly zero is scaled by 0 and nothing random is added
 *     anywhere: the score is deterministic and that of an all-zero utterance is 0.
 *   - the rate change.  pystoi resamples with an Octave-style filter of its own; the callers here use
 *     vaenmf_resample_batch (scipy's default Kaiser filter).  On the reference's committed utterances the ESTOI of the
 *     whole path rounds to the two decimals the reference printed.
 *   Also: T <= 256 (no frame) gives 1e-5 and counts of zero, where pystoi raises on the maximum of an empty array.
 * Per utterance the results are the same bits in any batch: no atomics, every sum in a fixed order by fixed lanes.  k, M
 * and J stay on the device (no host synchronisation): the grids cover the worst case k = n_frames.
 * vaenmf_stoi_geometry, HOST only: n_frames as above, max_spec_frames = max(n_frames - 1, 0) (M when every frame is
 *   kept), max_segments = max(max_spec_frames - 29, 0); -1 for n_samples < 0 or more than 2^31 - 1 frames.
 * vaenmf_stoi_bands, HOST only: lo, hi HOST int32 [15], the bin ranges above.
 * vaenmf_stoi_work_bytes: the bytes of `work` for a batch with these sample_offsets (HOST int64 [n_utt+1], non-decreasing),
 *   the same for the three calls below; -1 on bad arguments.
 * Buffers of the three device calls: sample_offsets HOST int64 [n_utt+1]; clean, proc DEV float [sample_offsets[n_utt]],
 *   utterance u at [sample_offsets[u], sample_offsets[u+1]), read only; keep DEV int32 [sum n_frames] (1 kept, 0 dropped,
 *   utterances concatenated); counts DEV int32 [n_utt][3] = {n_frames, k, J}; tob_x, tob_y DEV double
 *   [sum max_spec_frames][16]: row m < M of an utterance holds its 15 band magnitudes and a zero, rows >= M are neither
 *   read nor written; d DEV double [n_utt]; work DEV, 8-byte aligned, work_bytes >= vaenmf_stoi_work_bytes (its contents
 *   mean nothing between calls).  Every buffer has exactly the stated extent at its natural alignment (4 bytes for
 *   float / int32, 8 for double); nothing is read or written outside them, and a buffer of extent zero may be null.
 *   The offset tables the kernels need travel as kernel arguments; nothing is allocated except, at the first call on a
 *   device, a table of 6 KiB (the window and the FFT twiddles, built in long double on the host; that call waits for
 *   its upload), every later call only launches.  n_utt == 0 is a no-op.
 * vaenmf_stoi_tob: silence removal and band magnitudes; writes keep, counts and rows < M of tob_x / tob_y.
 * vaenmf_stoi_segments: d from tob_x / tob_y and counts as vaenmf_stoi_tob left them (a J larger than max_segments is
 *   read as max_segments); extended != 0: ESTOI, else STOI.
 * vaenmf_stoi_batch: both in one pass, the intermediates in `work`; counts may be null. */
int vaenmf_stoi_geometry(int64_t n_samples, int32_t* n_frames, int32_t* max_spec_frames, int32_t* max_segments);
int vaenmf_stoi_bands(int32_t* lo, int32_t* hi);
int64_t vaenmf_stoi_work_bytes(int32_t n_utt, const int64_t* sample_offsets);
int vaenmf_stoi_tob(const float* clean, const float* proc, int32_t n_utt, const int64_t* sample_offsets, int32_t* keep,
                    int32_t* counts, double* tob_x, double* tob_y, void* work, int64_t work_bytes, void* stream);
int vaenmf_stoi_segments(const double* tob_x, const double* tob_y, const int32_t* counts, int32_t n_utt,
                         const int64_t* sample_offsets, int32_t extended, double* d, void* work, int64_t work_bytes,
                         void* stream);
int vaenmf_stoi_batch(const float* clean, const float* proc, int32_t n_utt, const int64_t* sample_offsets, int32_t extended,
                      double* d, int32_t* counts, void* work, int64_t work_bytes, void* stream);

/* Noisy data sets -- the arithmetic of the reference's scripts/create_test_set.py:80-103 (process_save_utt) and
 * scripts/create_noisy_train_set.py:219-250, 299-303 for ragged batches of device signals: mixing speech with noise at a
 * signal-to-noise ratio, and the per-bin running sums behind trainset_mean.npy / trainset_std.npy.
 *
 * vaenmf_mix_batch.  Utterance u has the speech row a[0 .. T) (T = in_offsets[u+1] - in_offsets[u]), a cut c = cuts[u] of
 *   samples dropped at its start (the reference drops int(0.1 fs)), a start b = starts[u] into the ONE noise buffer of
 *   noise_len samples that the batch shares, and a factor f = factors[u] = 10^(-snr_db / 10) computed by the caller.  With
 *   T' = T - c, everything in float64 on the float32 samples:
 *     p   = max |a[i]| over i >= c                                     (speech[int(0.1 fs):]; speech / max|speech|)
 *     s_i = a[i + c] / p,   v_i = noise[b + i],   i in [0, T')
 *     Es  = sum s_i^2,  En = sum v_i^2,  k = Es f / En,  n_i = sqrt(k) v_i,  x_i = s_i + n_i
 *     joint_norm != 0 (create_test_set.py:99-103):       m = max_i max(|s_i|, |n_i|, |x_i|);  s_i / m, n_i / m, x_i / m
 *     joint_norm == 0 (create_noisy_train_set.py:244):   m = 1
 *   s, n, x receive the three signals, each rounded ONCE from its float64 value to float32, utterance u at
 *   [out_offsets[u], out_offsets[u+1]), which must span exactly T' samples; stats[u] = {p, Es, En, k, m}.
 *   Determinism: the samples of an utterance are cut into min(16, ceil(T' / 4096)) consecutive spans of equal length, one
 *   workgroup each -- a function of T' alone -- every workgroup sums in a fixed order and leaves one partial, and the
 *   partials are combined in span order; no atomics.  An utterance therefore has the same bits in s, n, x and stats alone,
 *   in any batch and in every run.  Multiplying the speech, or the noise, by a power of two changes no bit of s, n, x
 *   (short of underflow).
 *   Degenerate utterances: p == 0 (silent speech), En == 0 (silent noise segment) or a k that is not finite give zeros in
 *   that utterance's s, n, x and stats {p, Es, En, 0, 0}; no NaN or Inf is written.  k == 0 is how a caller tells.
 *   Refused with -1 before any launch (nothing is written; the message names the utterance): T' < 1, c < 0, b < 0,
 *   b + T' > noise_len, an out_offsets span other than T', a factor that is not positive and finite.
 *   Buffers: speech DEV float [in_offsets[n_utt]], noise DEV float [noise_len], s, n, x DEV float [out_offsets[n_utt]], all
 *   at their natural (4-byte) alignment and read / written one float at a time: nothing is read outside [c, T) of a speech
 *   row and [b, b + T') of the noise, nothing written outside an utterance's output span.  in_offsets, out_offsets HOST
 *   int64 [n_utt+1]; cuts, starts HOST int64 [n_utt]; factors HOST double [n_utt]; stats DEV double [n_utt][5], 8-byte
 *   aligned; work DEV, 8-byte aligned, work_bytes >= vaenmf_mix_work_bytes(n_utt) (its contents mean nothing between
 *   calls).  The tables travel as kernel arguments: no allocation, no copy, no synchronisation.  n_utt == 0 is a no-op.
 * vaenmf_mix_work_bytes: 552 n_utt, or -1 for n_utt outside [0, 2^24].
 *
 * vaenmf_feature_moments.  P DEV float [n_frames][ld], frame-major; bins f < F are read, columns F .. ld-1 may hold
 *   anything.  S1[f] = sum_t (double)P[t][f], S2[f] = sum_t ((double)P[t][f])^2 (create_noisy_train_set.py:302-303, which
 *   keeps these sums in float32), S1, S2 DEV double [F], 8-byte aligned.  accumulate == 0 overwrites S1 / S2; accumulate
 *   != 0 adds the call's sums onto their contents with exactly one float64 addition per bin, so a set can be streamed batch
 *   by batch.  The frames are cut into min(256, ceil(n_frames / 64)) spans of equal length -- a function of n_frames alone --
 *   each summed in a fixed order, and the spans' partials are added in span order: the same bits in every run.  n_frames
 *   == 0 leaves S1 / S2 alone (accumulate) or zeroes them.  work DEV, 8-byte aligned, work_bytes >=
 *   vaenmf_moments_work_bytes(n_frames, F).  -1 for n_frames < 0, F < 1 or ld < F.  No allocation, no synchronisation. */
int64_t vaenmf_mix_work_bytes(int32_t n_utt);
int vaenmf_mix_batch(const float* speech, int32_t n_utt, const int64_t* in_offsets, const int64_t* cuts, const float* noise,
                     int64_t noise_len, const int64_t* starts, const double* factors, int32_t joint_norm,
                     const int64_t* out_offsets, float* s, float* n, float* x, double* stats, void* work, int64_t work_bytes,
                     void* stream);
int64_t vaenmf_moments_work_bytes(int64_t n_frames, int32_t F);
int vaenmf_feature_moments(const float* P, int64_t n_frames, int32_t F, int32_t ld, int32_t accumulate, double* S1, double* S2,
                           void* work, int64_t work_bytes, void* stream);

/* ---- Training (scripts/training_M1.py, training_M2.py, training_classifier.py) ---------------------------------------
 * All arithmetic is fp32 with fp32 accumulation, loss sums are double.  Nothing here allocates, copies to the host or
 * synchronises except vaenmf_trainer_create / _destroy; every call is a few launches on `stream`.  The same inputs give the
 * same bits in every run: no atomics, no split reductions.
 *
 * Dense layers on v_mfma_f32_16x16x4_f32: every output element is the sum of four chains c_j = fmaf(a_k, b_k, c_j) over
 * the k with (k / 4) % 4 == j, ascending, each from 0, and of the bias: (c0 + c1), (c2 + c3), their sum and the bias are
 * added by fp32 two-sums, and the four rounding errors ((e01 + e23) + e) + eb are added to the result once.
 * Rows carry leading dimensions; columns between a row's width and its leading dimension are never read and never written.
 *   vaenmf_train_dense_fwd  Y[M][out] = act(X[M][in] W[out][in]^T + b), act one of NONE, TANH, RELU, SIGMOID, EXP; b may be
 *                           NULL (no bias).  W rows are ldw apart.
 *   vaenmf_train_dense_dx   dX[M][in] = (dZ[M][out] W[out][in]) * act'(Yprev[M][in]), the derivative of the PREVIOUS layer's
 *                           activation from its saved output: tanh 1 - y^2, relu y > 0, exp y, sigmoid y (1 - y), NONE 1
 *                           (Yprev may then be NULL).  `in` may be fewer than W's columns: the first `in` are used.
 *   vaenmf_train_dense_dw   dW[out][in] = dZ[M][out]^T X[M][in]; db[out] = column sums of dZ from the same pass (NULL: not
 *                           wanted).  The reduction is the batch M, walked by one workgroup per tile in row order.
 *   Refused with -1: M outside [1, 65536], in / out outside [1, 4096], a leading dimension below its width.
 *
 * Heads.  B rows, one workgroup (or wavefront) per row; the per-row sums are double.
 *   vaenmf_elbo_out         a = the decoder's output BEFORE the exponential, r = exp(a) (utils.py:66-69):
 *                           row_recon[b] = sum_f (x / r - log(x + eps) + a - 1), dA[b][f] = (1 - x / r) / B (NULL: no gradient).
 *   vaenmf_elbo_latent_fwd  ML[b] = [mu (z) | logvar (z)]; Z[b][j] = mu + exp(logvar / 2) eps[b][j], j < z (eps DEV [B][z]).
 *   vaenmf_elbo_latent_bwd  row_kl[b] = -1/2 sum_j (logvar - mu^2 - exp(logvar)); with dML: dML[b] = [dmu | dlogvar],
 *                           dmu = mu / B + dz, dlogvar = (exp(logvar) - 1) / (2 B) + dz exp(logvar / 2) eps / 2.
 *   vaenmf_bce_head         a = the classifier's output BEFORE the sigmoid, yh = sigmoid(a), evaluated in double with
 *                           1 - yh = sigmoid(-a) (utils.py:55-56): row_loss[b] = -sum_j (y log(yh + eps) + (1 - y) log(1 - yh + eps)),
 *                           dA = -(y / (yh + eps) - (1 - y) / (1 - yh + eps)) yh (1 - yh) / B,
 *                           row_cnt[b] = {tp, tn, fp, fn} of (yh > 0.5) against (y > 0.5) (training_classifier.py:148-154).
 *   vaenmf_loss_reduce      out (DEV, 64 bytes, 8-byte aligned): double {a + b, a, b, 0} with a = sum(row_a) / B, b =
 *                           sum(row_b) / B (row_b NULL: 0), then int64 {tp, tn, fp, fn} summed over row_cnt (NULL: zeros).
 * vaenmf_train_gather: dst[b][col0 + c] = src[idx[b]][c] for c < ncol, or (src - mean[c]) / (std[c] + eps) when mean / std
 *   (DEV [ncol]) are given (training_classifier.py:133-135).  idx DEV int32 [B], each in [0, NT); a row outside is not read
 *   and yields NaN.
 * vaenmf_adam: torch.optim.Adam's default update (no weight decay, no amsgrad) of n parameters in one launch, `step` = 1 for
 *   the first: m += (1 - beta1) (g - m); v = beta2 v + (1 - beta2) g g; p += (-(lr / (1 - beta1^step)) m) / (sqrt(v) /
 *   sqrt(1 - beta2^step) + eps), the bias corrections computed on the host in double.
 * vaenmf_train_eps_fill: the N(0,1) draws [B][z] of training step `step` (>= 1) under `seed`: the generator of the MH
 *   chains (z / 4 streams of four per row), keyed by (seed, step, row).  z a multiple of 4. */
int vaenmf_train_dense_fwd(const float* X, int32_t M, int32_t in, int32_t ldx, const float* W, int32_t ldw, const float* b,
                           int32_t out, int32_t act, float* Y, int32_t ldy, void* stream);
int vaenmf_train_dense_dx(const float* dZ, int32_t M, int32_t out, int32_t ldz, const float* W, int32_t ldw, int32_t in,
                          const float* Yprev, int32_t ldp, int32_t act, float* dX, int32_t lddx, void* stream);
int vaenmf_train_dense_dw(const float* dZ, int32_t M, int32_t out, int32_t ldz, const float* X, int32_t in, int32_t ldx,
                          float* dW, int32_t lddw, float* db, void* stream);
int vaenmf_elbo_out(const float* X, int32_t ldx, const float* A, int32_t lda, int32_t B, int32_t F, double eps, float* dA,
                    int32_t ldd, double* row_recon, void* stream);
int vaenmf_elbo_latent_fwd(const float* ML, int32_t ldm, const float* eps, int32_t B, int32_t z, float* Z, int32_t ldz, void* stream);
int vaenmf_elbo_latent_bwd(const float* ML, int32_t ldm, const float* eps, const float* dZ, int32_t lddz, int32_t B, int32_t z,
                           float* dML, int32_t lddm, double* row_kl, void* stream);
int vaenmf_bce_head(const float* A, int32_t lda, const float* Y, int32_t ldy, int32_t B, int32_t D, double eps, float* dA, int32_t ldd,
                    double* row_loss, int32_t* row_cnt, void* stream);
int vaenmf_loss_reduce(const double* row_a, const double* row_b, const int32_t* row_cnt, int32_t B, double* out, void* stream);
int vaenmf_train_gather(const float* src, int32_t lds, int64_t NT, const int32_t* idx, int32_t B, int32_t ncol, const float* mean,
                        const float* std, float eps, float* dst, int32_t ldd, int32_t col0, void* stream);
int vaenmf_adam(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, double lr, double beta1, double beta2,
                double eps, void* stream);
int vaenmf_train_eps_fill(uint64_t seed, int64_t step, int32_t B, int32_t z, float* eps_out, void* stream);

/* The trainer: a model's parameters, gradients and Adam state in one device arena, and the buffers of a step.
 *   kind M1: encoder x -> hidden (tanh) -> [mu | logvar], decoder z -> reversed(hidden) (tanh) -> exp (models.py:90-133);
 *   M2: the same over [x | y] and [z | y] (models.py:184-197); CLASSIFIER: x -> hidden (relu) -> sigmoid, y_dim outputs
 *   (models.py:41-62, batch_norm = False).  One or two hidden layers of any width in [1, 4096]; x_dim, y_dim in [1, 4096]
 *   with x_dim + y_dim <= 4096 (M1: y_dim = 0); z_dim a multiple of 4 in [4, 1024]; max_batch in [1, 65536].  Anything
 *   else is refused with -1 and a message.
 * Tensors are numbered in the order of the reference's state_dict (weight [out][in] then bias of every layer: encoder
 *   hidden layers, mu, log_var, decoder hidden layers, reconstruction; classifier: hidden layers, output_layer);
 *   vaenmf_trainer_tensor_shape gives rows and cols (cols = 0 for a bias).  set / get copy one tensor (src / dst DEV or
 *   HOST, contiguous) asynchronously on `stream`; `which` selects parameters, the gradients of the last step, or Adam's m / v.
 * vaenmf_trainer_step: one step on the rows idx[0..B) (DEV int32) of X DEV [NT][ldx] (and Y DEV [NT][ldy]; M1: NULL):
 *   gather, forward, loss, backward, Adam.  eps DEV [B][z_dim] replays the reparameterisation draws; NULL draws them on the
 *   device, keyed by (seed, the step's number, row) -- the draws vaenmf_trainer_eps_fill(t, step number, ..) returns, the
 *   first step's number being vaenmf_trainer_step_count() + 1 = 1.  losses DEV, 64 bytes as vaenmf_loss_reduce writes them:
 *   {loss, recon, KL} (classifier: {loss, loss, 0}) and {tp, tn, fp, fn} (VAEs: zeros).  Means are over B.
 * vaenmf_trainer_eval: forward and loss only; parameters, gradients, Adam state and the step count stay as they are.
 * vaenmf_trainer_set_norm: the classifier's input becomes (x - mean) / (std + eps); mean, std DEV [x_dim], caller-owned,
 *   read at every step (NULL, NULL: no normalisation). */
typedef struct vaenmf_trainer vaenmf_trainer;
enum { VAENMF_TRAIN_M1 = 0, VAENMF_TRAIN_M2 = 1, VAENMF_TRAIN_CLASSIFIER = 2 };
enum { VAENMF_TRAIN_PARAM = 0, VAENMF_TRAIN_GRAD = 1, VAENMF_TRAIN_ADAM_M = 2, VAENMF_TRAIN_ADAM_V = 3 };
typedef struct {
  int32_t kind;                  /* VAENMF_TRAIN_* */
  int32_t x_dim, y_dim, z_dim;
  int32_t n_hidden, hidden[2];   /* h_dim as the reference's constructors take it */
  int32_t max_batch;
  double lr, beta1, beta2, adam_eps;   /* torch.optim.Adam(lr, betas, eps) */
  double loss_eps;               /* eps of elbo / binary_cross_entropy (the scripts: 1e-8) */
} vaenmf_trainer_config;
int vaenmf_trainer_create(const vaenmf_trainer_config* cfg, vaenmf_trainer** out);
void vaenmf_trainer_destroy(vaenmf_trainer* t);
int vaenmf_trainer_num_tensors(const vaenmf_trainer* t);
int vaenmf_trainer_tensor_shape(const vaenmf_trainer* t, int32_t i, int32_t* rows, int32_t* cols);
int vaenmf_trainer_set_tensor(vaenmf_trainer* t, int32_t which, int32_t i, const float* src, void* stream);
int vaenmf_trainer_get_tensor(const vaenmf_trainer* t, int32_t which, int32_t i, float* dst, void* stream);
int vaenmf_trainer_set_params(vaenmf_trainer* t, int32_t i, const float* src, void* stream);
int vaenmf_trainer_get_params(const vaenmf_trainer* t, int32_t i, float* dst, void* stream);
int vaenmf_trainer_set_norm(vaenmf_trainer* t, const float* mean, const float* std, float eps);
int64_t vaenmf_trainer_step_count(const vaenmf_trainer* t);
int vaenmf_trainer_set_step_count(vaenmf_trainer* t, int64_t step);
int vaenmf_trainer_step(vaenmf_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx,
                        int32_t B, const float* eps, uint64_t seed, double* losses, void* stream);
int vaenmf_trainer_eval(vaenmf_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx,
                        int32_t B, const float* eps, uint64_t seed, double* losses, void* stream);
int vaenmf_trainer_eps_fill(const vaenmf_trainer* t, int64_t step, int32_t B, uint64_t seed, float* eps_out, void* stream);

/* Per-kernel device timing with HIP events recorded on the launch stream around every
 * hot-path launch (kinds: 0 mh_chain, 1 decode+W-statistics, 2 W update, 3 decode+H/g/cost,
 * 4 decode+Wiener).  enable(max_launches>0) pre-creates the events (no allocation at
 * launch time); read() synchronises, returns summed milliseconds and launch counts per
 * kind (arrays of 5) and resets. */
int vaenmf_profile_enable(vaenmf_plan* p, int32_t max_launches);
int vaenmf_profile_read(vaenmf_plan* p, double* ms, int64_t* counts);

/* Measurement aid of bench.py (no reference counterpart; not on the hot path): the rate in GB/s at which the GPU delivers
 * a plain streaming read of `bytes` bytes of buf (DEV, 16-byte aligned) to a hand-written kernel (16 bytes per lane, 8
 * wavefronts per SIMD, grid = resident set) -- the measured ceiling the streaming M-step kernels are compared with.
 * `reps` timed sweeps after one untimed one; sink DEV (4 bytes, never written in practice).  Synchronises the stream. */
int vaenmf_hbm_read_probe(const void* buf, int64_t bytes, int32_t reps, void* sink, double* gbps_out, void* stream);

/* Test aid (no reference counterpart; not on the hot path): the wavefront sums the streaming kernels are built on, run on
 * n sets of 4 x 64 floats, x DEV [n][4][64].  Every lane writes what it holds afterwards: one DEV [n][4][64], each of the
 * four values summed on its own; x4 DEV [n][64], the four through one shared cross-row stage (lanes 16 j .. 16 j + 15 hold
 * total j); x2 DEV [n][2][64], the pairs (0, 1) and (2, 3) (lanes 0-15 and 32-47 hold the pair's first total, lanes 16-31
 * and 48-63 its second). */
int vaenmf_wave_sum_probe(const float* x, int32_t n, float* one, float* x4, float* x2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAENMF_H */
