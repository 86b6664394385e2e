/*
 * mlggd.h -- C-ABI of the MI355X (gfx950) training engine: the drop-in boundary for the
 * reference's device engine `class BP_GPU` (Train_code_ML_GGD/BP_GPU.h:45-70), which has
 * no FFI layer of its own.  Plain pointers and sizes only; every entry point returns an int
 * status (0 = MLGGD_OK) and mlggd_last_error() gives the message, where the reference
 * printf()s and exit(0)s (BP_GPU.cu:20,534,578).
 *
 * Conventions shared with the reference:
 *  - host matrices are row-major: in [n_frames][layersizes[0]], targ/out
 *    [n_frames][layersizes[L-1]], weights[l] [layersizes[l-1]][layersizes[l]];
 *  - weights[] / bias[] are arrays of numlayers pointers indexed by layer l = 1..L-1
 *    (slot 0 unused), exactly as BP_GPU's float** arguments (BPtrain.cc:77-78,108);
 *  - the caller owns all host buffers; the engine copies on entry and owns device memory;
 *  - calls are synchronous unless stated otherwise and must come from one thread.
 */
#ifndef MLGGD_H
#define MLGGD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLGGD_MAXLAYER 10          /* BP_GPU.h:6  MAXLAYER */
#define MLGGD_MAXCACHEFRAME 200000 /* BP_GPU.h:7  MAXCACHEFRAME */
#define MLGGD_UNIQUE_ID_BYTES 128  /* sizeof(ncclUniqueId) */
#define MLGGD_MAX_BETAS 32         /* shapes per mlggd_error_stats call */

enum {
    MLGGD_OK = 0,
    MLGGD_ERR_ARG = 1,     /* bad argument / shape */
    MLGGD_ERR_DEVICE = 2,  /* HIP runtime error (no device, alloc, launch) */
    MLGGD_ERR_COMM = 3,    /* RCCL error */
    MLGGD_ERR_STATE = 4    /* call not valid in the engine's current state */
};

/* mlggd_config.activation: what every hidden layer applies to x = sum + bias.  The output layer is linear either way.
 * MLGGD_ACT_RELU: y = (x < 0) ? 0 : x -- a NaN stays a NaN -- and dE/dx = (y > 0) ? dE/dy : 0; the rectifier sibling of
 * the reference's BPtrain_Sigmoid (its Gen_rand_wts_for_ReLUs.pl initialises such nets).  Any other value is
 * MLGGD_ERR_ARG at mlggd_create, found before a device is touched. */
enum { MLGGD_ACT_SIGMOID = 0, MLGGD_ACT_RELU = 1 };

typedef struct mlggd_engine *mlggd_handle;

/* One int32 slot of mlggd_config under a name of its own: the struct ends in `reserved[5]` as it always did, and a
 * reserved slot that takes a meaning is reached under its name through an anonymous union (C11, C++) with that array,
 * so that code which fills or checks `reserved` keeps compiling and the layout cannot move. */
#define MLGGD_CONFIG_SLOT(name) int32_t name

/* Constructor arguments of BP_GPU (BP_GPU.h:48-49, BP_GPU.cu:9-11), same meaning. */
typedef struct mlggd_config {
    int32_t struct_size;     /* = sizeof(mlggd_config), ABI guard */
    int32_t random_seed;     /* seeds the dropout generator (BP_GPU.cu:59-60) */
    int32_t device;          /* GPU ordinal, BP_GPU.cu:15-23 (gpu_used=) */
    int32_t numlayers;       /* 2..MLGGD_MAXLAYER */
    int32_t layersizes[MLGGD_MAXLAYER];
    int32_t bunchsize;       /* frames per minibatch on THIS rank */
    float lrate;
    float momentum;
    float weightcost;
    float shapefactor;       /* beta of the GGD / beta-norm */
    int32_t MLflag;          /* 1: ML-GGD objective, else beta-norm (BP_GPU.cu:408-424) */
    int32_t dropoutflag;     /* BP_GPU.cu:344-355,484-501 */
    float visible_omit;
    float hid_omit;
    int32_t max_cache_frames; /* rows of the resident chunk buffers; 0 -> MLGGD_MAXCACHEFRAME */
    int32_t activation;      /* hidden units: MLGGD_ACT_SIGMOID (0, the default of a zeroed struct) or MLGGD_ACT_RELU */
    int32_t nat_frames;      /* noise-aware training: 0 (a zeroed struct) = off; T >= 1: every input row ends in its utterance's
                              * noise row over the first T frames, layersizes[0] = (fea_context + 1) * D; < 0: MLGGD_ERR_ARG */
    union {                  /* the five reserved slots stay one array; a slot that takes a meaning is also a named member */
        MLGGD_CONFIG_SLOT(mask_bins); /* = reserved[0].  Multi-objective net: 0 (a zeroed struct) = off; M >= 1: the last layer
                              * has 2 * M units, the first M the clean LPS, the last M a ratio mask (mlggd_set_mask); < 0 or
                              * another width: MLGGD_ERR_ARG */
        int32_t reserved[5];
    };
} mlggd_config;

/* ---- lifetime: BP_GPU::BP_GPU / ~BP_GPU (BP_GPU.cu:9-150) ---- */
int mlggd_create(const mlggd_config *cfg, const float *const *weights, const float *const *bias,
                 mlggd_handle *out);
int mlggd_destroy(mlggd_handle h);
const char *mlggd_last_error(void);
int mlggd_device_count(int *count); /* cudaGetDeviceCount, BP_GPU.cu:15 */

/* ---- training: BP_GPU::train (BP_GPU.cu:152-185) ----
 * Uploads the chunk, runs train_bunch_single (BP_GPU.cu:308-440) on every FULL bunch and
 * skips the trailing partial bunch, returns after the last step has completed.
 * *bunches_trained (optional) receives the number of steps run. */
int mlggd_train_chunk(mlggd_handle h, int n_frames, const float *in, const float *targ,
                      int *bunches_trained);

/* The same, split so a benchmark can time steps on HBM-resident data:
 * mlggd_load_chunk = the two todev_vf_vf calls (BP_GPU.cu:163-164);
 * mlggd_train_resident = the bunch loop (BP_GPU.cu:170-184) over frames
 * [first_frame, first_frame + n_frames) of the resident chunk; asynchronous --
 * mlggd_sync() waits for completion. */
int mlggd_load_chunk(mlggd_handle h, int n_frames, const float *in, const float *targ);
int mlggd_train_resident(mlggd_handle h, int first_frame, int n_frames, int *bunches_trained);
int mlggd_sync(mlggd_handle h);

/* ---- cross-validation: BP_GPU::CrossValid / CrossValiddB / CrossValid2
 * (BP_GPU.cu:187-306) over cv_bunch_single (BP_GPU.cu:442-512).  Each returns the chunk's
 * sum exactly as the reference accumulates it (host fp32 scalar, frame-major order):
 * sqerr = sum (o-t)^2 ; abserr = sum |o-t| / D ; loglik = GGD log-likelihood with the
 * alpha of the last training minibatch. */
int mlggd_cv_sqerr(mlggd_handle h, int n_frames, const float *in, const float *targ, float *out);
int mlggd_cv_abserr(mlggd_handle h, int n_frames, const float *in, const float *targ, float *out);
int mlggd_cv_loglik(mlggd_handle h, int n_frames, const float *in, const float *targ, float *out);
/* All three from ONE forward pass (same accumulation order; loglik only if MLflag==1). */
int mlggd_cv_all(mlggd_handle h, int n_frames, const float *in, const float *targ,
                 float *sqerr, float *abserr, float *loglik);
/* cv_bunch_single over a whole chunk: out[n_frames][D] network outputs (forward only). */
int mlggd_forward(mlggd_handle h, int n_frames, const float *in, float *out);

/* ---- input pipeline on the device (no counterpart in the reference, which
 * context-expands every chunk on one host thread, Interface.cc:778-785, and uploads the 11x
 * larger matrix, BP_GPU.cu:163-164).  A sample is a window of fea_context CONSECUTIVE frames,
 * i.e. a contiguous slice of the normalised frame stream, so the caller uploads the chunk's
 * frames once -- feat [n_frames][layersizes[0]/fea_context], targ [n_frames][D] -- plus, for
 * every sample ROW (in the shuffled row order Readchunk would have produced), the index of its
 * first frame; sample i's target is frame first_frame[i] + targ_offset.  Rows are gathered by
 * the input-staging kernel; results are bit-identical to the expanded path.
 * After mlggd_load_frames, mlggd_train_resident indexes SAMPLES of this chunk.
 * fea_context may differ from call to call on one engine (any value that divides layersizes[0]):
 * the device buffers are sized in floats for the context of the call at hand. */
int mlggd_load_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                      int n_samples, const int32_t *first_frame, int targ_offset);
int mlggd_train_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                       int n_samples, const int32_t *first_frame, int targ_offset, int *bunches_trained);
/* mlggd_train_frames without the final wait: returns when the chunk is on the device and its steps are enqueued;
 * the next chunk's upload then overlaps them (two device buffer sets).  mlggd_sync() waits. */
int mlggd_train_frames_async(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                       int n_samples, const int32_t *first_frame, int targ_offset, int *bunches_trained);
int mlggd_cv_all_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                        int n_samples, const int32_t *first_frame, int targ_offset, float *sqerr, float *abserr,
                        float *loglik);
int mlggd_forward_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, int n_samples,
                         const int32_t *first_frame, float *out);
/* ---- noise-aware training, NAT (csrc/nat_rule.h; Xu, Du, Dai and Lee 2014 / 2015; no counterpart in the reference).
 * An engine created with mlggd_config.nat_frames = T >= 1 takes input rows that end in a noise estimate of their
 * utterance: the window of fea_context frames, then the D values of the utterance's noise row, so layersizes[0] =
 * (fea_context + 1) * D and a stream row is layersizes[0] / (fea_context + 1) wide.  The rule: an utterance u of
 * F_u >= 1 frames uses T_u = min(T, F_u) of them; with x_t[k] = (lps_t[k] - mean[k]) * inv_std[k] (two fp32
 * operations, the stream's own) its noise row is z_u[k] = (((x_0[k] + x_1[k]) + x_2[k]) + ... + x_{T_u-1}[k]) /
 * (float)T_u: fp32 additions from left to right, one fp32 division, nothing contracted.  An utterance without frames
 * has a zero row.  Targets are unchanged.
 *
 * The *_frames_nat entries are the *_frames entries with the noise table nat [n_nat][fdim] and, per sample row, the
 * index nat_row[i] of its noise row (rows may repeat and come in any order); the staging kernel gathers both parts, and
 * every result equals, bit for bit, the expanded entry (mlggd_train_chunk, mlggd_cv_all, mlggd_forward, ...) on rows
 * [window | nat[nat_row[i]]] built by the caller -- the expanded entries work on a NAT engine as they are.  After
 * mlggd_load_frames_nat, mlggd_train_resident indexes these samples.  A nat_row outside [0, n_nat) (the message names
 * the sample), NULL pointers and a fea_context with (fea_context + 1) * fdim != layersizes[0] are MLGGD_ERR_ARG, found
 * before any device call.  The _nat entries on an engine with nat_frames = 0, and the plain *_frames entries
 * (mlggd_error_stats_frames and mlggd_train_frames_async included) on a NAT engine, are MLGGD_ERR_STATE; the engine
 * stays usable and unchanged.
 * On a NAT engine mlggd_load_waves / mlggd_cv_all_waves / mlggd_train_waves and mlggd_enhance_wave / _waves / _scored /
 * _scored_stoi keep their signatures, need (fea_context + 1) * D == layersizes[0] and form every utterance's noise row
 * on the device from its noisy LPS rows (once per call, before any chunk: the decoders' results still do not depend on
 * max_cache_frames, the batch or the position); neither the noisy rows nor the noise rows visit the host.
 * mlggd_live_open, mlggd_comm_init and mlggd_debug_fake_world on a NAT engine are MLGGD_ERR_STATE.
 * mlggd_nat_estimate / mlggd_nat_rows: host only, no device.  rows [sum F][D] are NORMALISED rows, utterance u's from
 * frame_off[u] (frame_off [n_utts+1], non-decreasing); out [n_utts][D].  nat_row[i] = the utterance that holds packed
 * frame first_frame[i] (utterances without frames are stepped over). */
int mlggd_load_frames_nat(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                          int n_samples, const int32_t *first_frame, int targ_offset, int n_nat,
                          const float *nat /* [n_nat][fdim] */, const int32_t *nat_row /* [n_samples] */);
int mlggd_train_frames_nat(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                           int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                           const int32_t *nat_row, int *bunches_trained);
int mlggd_cv_all_frames_nat(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                            int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                            const int32_t *nat_row, float *sqerr, float *abserr, float *loglik);
int mlggd_forward_frames_nat(mlggd_handle h, int n_frames, int fea_context, const float *feat, int n_samples,
                             const int32_t *first_frame, int n_nat, const float *nat, const int32_t *nat_row,
                             float *out);
int mlggd_nat_estimate(int D, int n_utts, const int32_t *frame_off /* [n_utts+1] */, const float *rows,
                       int nat_frames, float *out /* [n_utts][D] */);
int mlggd_nat_rows(int n_utts, const int32_t *frame_off /* [n_utts+1] */, int n_samples, const int32_t *first_frame,
                   int32_t *nat_row /* [n_samples] */);
int mlggd_get_nat_frames(mlggd_handle h, int *nat_frames); /* the nat_frames the engine was created with */

/* ---- the GGD error model on the device (no counterpart in the reference, which only ever holds the alpha of the
 * last training minibatch and evaluates CrossValid2 at it, BP_GPU.cu:271-301).  The ML criterion models the error
 * e = out - targ of every output bin d as a generalized Gaussian  beta / (2 alpha_d Gamma(1/beta)) exp(-(|e|/alpha_d)^beta);
 * its sufficient statistics are per-bin sums over a CV pass.
 *
 * mlggd_error_stats / mlggd_error_stats_frames mirror mlggd_cv_all / mlggd_cv_all_frames: the chunk is loaded WITH
 * its targets, the CV forward runs per bunch (trailing partial bunch included), and one kernel per bunch folds the
 * bunch into sums kept on the device.  Per element x = slab sum + bias in fp32 (the bits mlggd_forward returns),
 * e = x - t in fp32; the terms e, e*e, (e*e)*e, (e*e)*(e*e) are formed in double from that fp32 e, and for each k the
 * fp32 value pow_or_self(|e|, betas[k]) of the trainer's own power is widened to double.  On return
 *   sums[0..3][d] = sum e, e^2, e^3, e^4        sums[4 + k][d] = sum |e|^betas[k]        (sums is [4 + n_betas][D])
 * OVERWRITTEN, not accumulated: the statistics are additive, a caller with several chunks adds the arrays.  The
 * order of every addition is fixed by the sample's position in its bunch, the bunch index and bunchsize: two calls
 * return the same bits, and the two entries return the same bits for the same rows.  (4 + n_betas) * D doubles come
 * back, nothing of size n x D.  n_frames / n_samples == 0 returns zeros.
 * NULL pointers, n_betas outside 1..MLGGD_MAX_BETAS, a beta <= 0 or not finite and a shape mismatch are
 * MLGGD_ERR_ARG, found before any device call.  An engine with a communicator or an emulated world, or with
 * dropoutflag != 0, is MLGGD_ERR_STATE; the engine stays usable. */
int mlggd_error_stats(mlggd_handle h, int n_frames, const float *in, const float *targ,
                      int n_betas, const float *betas, double *sums /* [4 + n_betas][D] */);
int mlggd_error_stats_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                             int n_samples, const int32_t *first_frame, int targ_offset,
                             int n_betas, const float *betas, double *sums);
/* mlggd_ggd_fit: host only, no device, all in double: the fit of the model to sums over n samples (added over the
 * chunks by the caller).  mean = S1/n, var = the central second moment, kurt = m4/m2^2 - 3 (central moments from the
 * raw sums).  For every grid shape the ML scale is alpha_d(beta)^beta = beta * P_beta,d / n -- the trainer's
 * scalefactor expression over the whole set -- at which sum (|e|/alpha)^beta = n/beta, so the profile log-likelihood
 * is  l_d(beta) = n [ln beta - ln 2 - lgamma(1/beta) - ln alpha_d(beta) - 1/beta]  (libm lgamma).
 * alpha, loglik: [n_betas][D]; best[d] = the grid index with the largest l_d; loglik_shared[k] = sum_d l_d(beta_k)
 * and best_shared its argmax -- the value for `shapefactor`, since the trainer shares one beta over all bins with an
 * alpha per bin.  Ties go to the lower index.  A bin with sum e^2 == 0 has no fit: alpha 0, loglik and kurt NaN,
 * best -1, left out of the shared totals (no bin with a fit: best_shared -1).  Every output pointer is optional.
 * n <= 0, D < 1, NULL betas / sums and a bad grid are MLGGD_ERR_ARG. */
int mlggd_ggd_fit(int D, int64_t n, int n_betas, const float *betas, const double *sums,
                  double *mean, double *var, double *kurt, double *alpha, double *loglik, int32_t *best,
                  double *loglik_shared, int32_t *best_shared);
/* pinned host memory for chunk buffers (optional; faster H2D than pageable memory) */
int mlggd_alloc_pinned(size_t bytes, void **out);
/* the same from a thread that has not selected a device (host IO threads): pins through `device`'s context */
int mlggd_alloc_pinned_on(int device, size_t bytes, void **out);
int mlggd_free_pinned(void *p);

/* ---- spectral front end / back end: the original project's Wav2LPS_be and LPS2Wav_be (Wav2LogSpec_be.c,
 * LogSpec2Wav.c with OLA_KIND 1) and its decoder decode.m, on the device.  fs_khz in {8, 11, 16}: frame L / hop S /
 * FFT N = 256/128/256, 256/110/256, 512/256/512; D = N/2 + 1 bins.  A wave of n int16 samples gives
 * F = (n - (L - S)) / S frames (0 if n < L; trailing samples dropped); a synthesised wave has F*S + L - S samples.
 *
 * mlggd_wave_to_lps: lps [F][D] = log |FFT(frame * Hamming)|^2 (floored at -50).  Stateless, any device; lps NULL =
 * query F only.
 * mlggd_lps_to_wave: the noisy wave's phase with the magnitude sqrt(exp(lps)), inverse FFT, window, overlap-add
 * / sum w^2; out = trunc toward zero, saturated to int16; out_f32 (optional) = the value before the cast.  n_frames
 * must be the F of n_samples.
 * mlggd_enhance_wave: the whole of decode.m on the engine's stream: noisy -> LPS -> (lps - mean) * inv_std ->
 * edge-replicated windows of fea_context frames -> forward pass -> y / inv_std + mean -> synthesis against the same
 * noisy wave.  Needs fea_context * D == layersizes[0] and layersizes[L-1] == D; n_samples >= L.  Inputs longer than
 * the chunk capacity (max_cache_frames) run in chunks whose frame streams overlap by fea_context - 1 frames: the
 * result does not depend on the chunking.  *n_out (optional) receives F*S + L - S. */
int mlggd_wave_to_lps(int device, int fs_khz, int n_samples, const int16_t *wave, int *n_frames, float *lps);
int mlggd_lps_to_wave(int device, int fs_khz, int n_samples, const int16_t *noisy, int n_frames, const float *lps,
                      int16_t *out, float *out_f32);
int mlggd_enhance_wave(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                       int n_samples, const int16_t *noisy, int16_t *out, float *out_f32, int *n_out);
/* mlggd_enhance_waves: mlggd_enhance_wave over a list of utterances in one pass.  Utterance u is
 * noisy[offsets[u] .. offsets[u+1]) (offsets non-decreasing, every utterance at least one frame long: otherwise
 * MLGGD_ERR_ARG naming the utterance) and has F_u frames by the rule above; the frames of all utterances form one
 * packed stream, so every forward bunch but the last is full, while the analysis, the context replication and the
 * overlap-add keep to each utterance's own edges.  Utterance u's F_u*S + L - S output samples start at out[out_off[u]]
 * (out_f32, optional, alike); lps_out (optional) [sum F][D] receives the de-normalised network output y / inv_std +
 * mean, utterance u's rows from frame_off[u].  Every bit of out / out_f32 equals mlggd_enhance_wave on the utterance
 * alone, whatever its neighbours, its position, the batch or max_cache_frames (chunks run over the packed frames).
 * The device buffers belong to the engine and only grow: after the first calls a call allocates nothing, uploads the
 * packed wave, downloads each requested output once and synchronises once.  n_utts == 0 does nothing.
 * mlggd_enhance_waves_layout: frame_off / out_off [n_utts+1] (each optional) of such a batch; host only. */
int mlggd_enhance_waves_layout(int fs_khz, int n_utts, const int64_t *offsets /* [n_utts+1] */,
                               int32_t *frame_off /* [n_utts+1] */, int64_t *out_off /* [n_utts+1] */);
int mlggd_enhance_waves(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                        int n_utts, const int16_t *noisy, const int64_t *offsets /* [n_utts+1] */, int16_t *out,
                        float *out_f32 /* optional */, float *lps_out /* optional */);

/* ---- the quality report of LPS2Wav_be on the device (csrc/score.hip.h): per utterance, the segmental SNR (frame
 * values 10 log10(sum clean^2 / sum (est - clean)^2) clamped to [-20, 30], est = the de-windowed enhanced frame) and
 * the log-spectral distortion (clean and enhanced power floored at 1e-5 of their maxima over the utterance's scored
 * frames) of enhanced LPS rows against the clean wave, in fp32.  `clean` is packed with the same `offsets` as `noisy`.
 * score_frames[u] (NULL: F_u) = the leading frames of utterance u that are scored, 0 <= score_frames[u] <= F_u; 0:
 * the utterance is not scored and both outputs are 0.  A clean wave shorter than its noisy wave is scored over the
 * frames it has: the caller pads its samples with zeros and passes that frame count.  An utterance's two numbers
 * depend on that utterance alone: the same bits whatever its neighbours, its position, the batch, max_cache_frames
 * and the run.  NULL pointers, decreasing offsets, an utterance shorter than one frame, a score_frames[u] out of range
 * and a bad fs_khz are MLGGD_ERR_ARG (the message names the utterance), found before any device call.
 * mlggd_score_waves: stateless, any device; lps [sum F][D], the rows of utterance u from frame_off[u].
 * mlggd_enhance_waves_scored: mlggd_enhance_waves plus the report on its de-normalised network output, from the
 * buffers of the same pass on the engine's stream (no second analysis, no second forward pass): the packed clean wave
 * goes up once and 2 n_utts floats come back.  out / out_f32 / lps_out are those of mlggd_enhance_waves bit for bit;
 * the buffers only grow, as there. */
int mlggd_score_waves(int device, int fs_khz, int n_utts, const int16_t *clean, const int16_t *noisy,
                      const int64_t *offsets /* [n_utts+1] */, const float *lps, const int32_t *score_frames /* optional */,
                      float *segsnr /* [n_utts] */, float *lsd /* [n_utts] */);
int mlggd_enhance_waves_scored(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean,
                               const float *norm_inv_std, int n_utts, const int16_t *noisy, const int16_t *clean,
                               const int64_t *offsets, const int32_t *score_frames /* optional */, int16_t *out,
                               float *out_f32 /* optional */, float *lps_out /* optional */, float *segsnr, float *lsd);

/* ---- STOI on the device (csrc/stoi.hip.h, csrc/stoi_rule.h): the short-time objective intelligibility measure of
 * Taal, Hendriks, Heusdens and Jensen (2011) of a processed int16 wave against the clean int16 wave, per utterance of
 * a packed batch, in fp32: both waves resampled to 10 kHz (8 kHz by 5/4, "11" = 11 000 Hz by 10/11, 16 kHz by 5/8; a
 * Kaiser-windowed sinc computed on the host in double), the frames (256 samples, hop 128) whose clean energy is more
 * than 40 dB below the loudest removed, 15 third-octave bands of 512-point spectra, segments of 30 frames, clipping at
 * -15 dB.  stoi_samples[u] (NULL: all) = the leading samples of utterance u that are scored, 0 <= stoi_samples[u] <=
 * its samples.  An utterance with fewer than 30 frames left after the removal (too short, a silent clean wave,
 * stoi_samples[u] = 0) has no value: stoi[u] = NaN and segments[u] = 0; that is not an error.  Nor has one whose
 * processed wave is exactly zero in a band over a whole segment (a muted output): NaN with segments[u] counted.
 * segments (optional)
 * [n_utts] receives the number of 30-frame segments behind each value.  An utterance's value depends on that utterance
 * alone: the same bits whatever its neighbours, its position, the batch, max_cache_frames and the run.  NULL pointers,
 * decreasing offsets, a stoi_samples[u] out of range and a bad fs_khz are MLGGD_ERR_ARG (the message names the
 * utterance), found before any device call.
 * mlggd_stoi_layout: host only, no device: the 10 kHz samples and the frames of an utterance of n_samples, and the
 * segments it has if every frame is kept (each output optional).
 * mlggd_stoi_waves: stateless, any device; `clean` and `proc` are packed with the same `offsets`.
 * mlggd_enhance_waves_scored_stoi: mlggd_enhance_waves_scored plus the STOI of the pass's own int16 output against
 * the clean wave, taken from device memory on the engine's stream: no host round trip of the waves, no second decoding
 * pass, the clean wave goes up once and 2 n_utts more words come back.  The enhanced wave of utterance u has F_u S + L
 * - S samples: stoi_samples[u] is checked against the utterance's samples and at most the enhanced wave's are scored.
 * out / out_f32 / lps_out / segsnr / lsd are those of mlggd_enhance_waves_scored bit for bit; the buffers only grow. */
int mlggd_stoi_layout(int fs_khz, int64_t n_samples, int64_t *len10, int64_t *frames, int64_t *min_segments);
int mlggd_stoi_waves(int device, int fs_khz, int n_utts, const int16_t *clean, const int16_t *proc,
                     const int64_t *offsets /* [n_utts+1] */, const int64_t *stoi_samples /* optional */,
                     float *stoi /* [n_utts] */, int32_t *segments /* optional [n_utts] */);
int mlggd_enhance_waves_scored_stoi(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean,
                                    const float *norm_inv_std, int n_utts, const int16_t *noisy, const int16_t *clean,
                                    const int64_t *offsets, const int32_t *score_frames /* optional */, int16_t *out,
                                    float *out_f32 /* optional */, float *lps_out /* optional */, float *segsnr,
                                    float *lsd, const int64_t *stoi_samples /* optional */, float *stoi,
                                    int32_t *segments /* optional */);

/* ---- live audio: a *live group* is n_sessions independent audio sessions decoded block by block on one engine; all
 * share fs_khz, fea_context and the norm vectors.  With half = (fea_context - 1) / 2 and F(n) the frame count above, a
 * session that has received n samples has decoded T = max(0, F(n) - half) frames while it runs (frame t needs the rows
 * up to t + half: no frame is decoded with a provisional right edge) and emitted T*S samples, each covered only by
 * decoded frames and therefore final; the push that ends it decodes the remaining frames against the right edge and
 * emits up to F*S + L - S.  A session ended with fewer than L samples in all emits nothing; that is not an error.
 * For any way of cutting a recording into pushes (empty blocks, blocks of one sample and an `end` with no samples
 * included) the concatenation of what a session emitted equals mlggd_enhance_wave of the whole recording in every bit
 * of out and out_f32, whatever the other sessions do, the slot, n_sessions, bunchsize, max_cache_frames (a push whose
 * decodable frames exceed the chunk capacity runs in chunks over the packed frames) and what the slot decoded before.
 * Between pushes a session keeps on the device its unconsumed samples (< L), the LPS rows that are left context or not
 * yet decoded (<= fea_context - 1), the noisy spectra of the frames not yet decoded (<= half) and the time blocks of
 * the last ceil(L/S) - 1 decoded frames; nothing is uploaded or analysed twice.  A push in the steady state allocates
 * nothing (buffers only grow), uploads the packed samples and one block of tables, launches a number of kernels that
 * does not depend on n_sessions, downloads each requested output once and synchronises once.  The state is the
 * group's own memory: other calls on the engine between two pushes (training, mlggd_enhance_waves, mlggd_set_weights)
 * do not disturb it; after mlggd_set_weights the contract refers to the new weights.  One recording may have up to
 * 2^31 - 1025 samples.
 *
 * mlggd_live_layout: host only, no device: out_off[n_sessions+1] of the push that adds add[u] samples to a session
 * that has received had[u] so far, ending it if end[u] (end NULL: none) -- the emission rule, stated once.
 * mlggd_live_open: needs a single-device engine (a communicator or an emulated world: MLGGD_ERR_STATE), fea_context
 * odd and fea_context * D == layersizes[0].  mlggd_destroy while a group of the engine is open is MLGGD_ERR_STATE and
 * leaves the engine usable: close the group first.
 * mlggd_live_push: session u receives samples[offsets[u] .. offsets[u+1]) (may be empty); its newly final output
 * samples go to out[out_off[u] .. out_off[u+1]) (out_f32 optional, alike); out_off is written by the call and equals
 * mlggd_live_layout's.  end[u] != 0: the session is finished after these samples: its remaining output is emitted and
 * the slot is empty again, ready for a new recording.  out_capacity (in samples) too small, NULL pointers and
 * decreasing offsets (the message names the session) are MLGGD_ERR_ARG before any device call, state unchanged.
 * mlggd_live_received: had[n_sessions], the samples each session has received since it began (host counters). */
typedef struct mlggd_live *mlggd_live_handle;
int mlggd_live_layout(int fs_khz, int fea_context, int n_sessions, const int64_t *had, const int64_t *add,
                      const uint8_t *end, int64_t *out_off);
int mlggd_live_open(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                    int n_sessions, mlggd_live_handle *out);
int mlggd_live_push(mlggd_live_handle s, const int16_t *samples, const int64_t *offsets, const uint8_t *end,
                    int16_t *out, float *out_f32, int64_t out_capacity, int64_t *out_off);
int mlggd_live_received(mlggd_live_handle s, int64_t *had /* [n_sessions] */);
int mlggd_live_close(mlggd_live_handle s);

/* ---- training data from waves (csrc/mix.hip.h, csrc/mix_rule.h; no counterpart in the original project, whose
 * training set is mixed by outside tools, analysed by Wav2LPS_be, packed into pfiles and normalised by qnnorm before
 * the trainer sees it).  Clean speech and noise are mixed at an SNR, both waves are analysed and normalised, and the
 * result is handed to the training loop on the device: no feature row is kept anywhere.
 *
 * The mixing rule.  A batch is n_utts clean int16 utterances packed with offsets[n_utts+1] as in mlggd_enhance_waves
 * (offsets[0] may be non-zero; an utterance may be empty); the noise is one packed int16 buffer of n_noise samples.
 * Utterance u names the segment [noise_lo[u], noise_lo[u] + noise_len[u]) of it and a start noise_start[u] inside the
 * segment: sample i is paired with noise[noise_lo[u] + (noise_start[u] + i) mod noise_len[u]], so a short segment
 * wraps (noise_len[u] = 1 is legal).  Ec = sum clean^2 and En = sum noise^2 over exactly those pairs are exact 64-bit
 * integers; gain[u] = sqrt((double)Ec / (double)En) * r[u], r[u] = pow(10, -snr_db[u] / 20) from the host's libm;
 * Ec == 0, En == 0 or snr_db[u] = +inf give gain[u] = 0 and the noisy wave is the clean wave.  noisy[i] =
 * sat16(rint(clean[i] + gain[u] * noise[.])): product and sum are two double operations, rint rounds to nearest even,
 * sat16 clamps to [-32768, 32767] and clipped[u] counts the samples it changed.  An utterance's samples depend on that
 * utterance alone: the same bits whatever its neighbours, its position, the batch and the run.
 *
 * mlggd_wave_samples: host only: all windows of fea_context frames that lie inside one utterance, in utterance and
 * frame order, as indices into the packed frame stream (F_u frames per utterance by the rule above, none for an
 * utterance shorter than a frame); first_frame NULL = count only.  An utterance with fewer than fea_context frames has
 * none.  Shuffling is the caller's: permute the table.
 * mlggd_mix_waves: stateless, any device; noisy is packed like clean; gain / clipped [n_utts] are optional.
 * mlggd_lps_stats: stateless, any device: sums [2][D] = sum x, sum x^2 per bin in double over the LPS rows of all
 * utterances (mlggd_wave_to_lps's rows), *n_frames their number.  OVERWRITTEN; the statistics are additive, a caller
 * with several batches adds the arrays.  A fixed number of rows per workgroup and an ordered fold: the same input
 * gives the same bits.  An utterance shorter than a frame contributes nothing.
 * mlggd_norm_from_stats: host only: mean = S1/n, inv_std = 1 / sqrt(S2/n - mean^2) (the population variance) in
 * double, rounded to float; a bin whose variance is not positive is MLGGD_ERR_ARG naming it.
 * mlggd_load_waves: the device-side mlggd_load_frames from a wave pair (noisy and clean packed with the same offsets):
 * feat = (lps(noisy) - mean) * inv_std, targ = (lps(clean) - mean) * inv_std -- the targets take the noisy statistics,
 * as the trainer's loader does -- over the packed frames, without edge replication; sample i is the window of
 * fea_context frames from first_frame[i] and its target is frame first_frame[i] + targ_offset.  Afterwards
 * mlggd_train_resident indexes these samples; every weight equals mlggd_train_frames on the same rows built on the
 * host, bit for bit.  Needs fea_context * D == layersizes[0] and layersizes[L-1] == D; fea_context need not be odd.
 * mlggd_cv_all_waves: mlggd_cv_all_frames from a wave pair, the same three sums bit for bit.
 * mlggd_set_noise: the noise bank stays on the device between calls; NULL / 0 frees it.
 * mlggd_train_waves: mix from the bank + load + train in one pass on the engine's stream and return after the steps
 * have completed; the noisy wave never visits the host unless noisy_out (packed like clean), gain or clipped ask.
 * Errors, all found before any device call: NULL pointers, decreasing offsets, a bad fs_khz, a segment outside the
 * noise, noise_len[u] < 1, a start outside its segment, an snr_db that is NaN or -inf (the message names the
 * utterance), a window that crosses an utterance boundary or leaves the packed frames (the message names the sample),
 * targ_offset outside [0, fea_context) and n_samples above the chunk capacity are MLGGD_ERR_ARG; mlggd_train_waves
 * without a noise bank and any of the engine calls on an engine with a communicator or an emulated world are
 * MLGGD_ERR_STATE, and the engine stays usable.  n_utts == 0 or n_samples == 0 does nothing and trains 0 bunches.
 * The device buffers belong to the engine and only grow. */
int mlggd_wave_samples(int fs_khz, int fea_context, int n_utts, const int64_t *offsets, int32_t *first_frame,
                       int64_t *n_samples);
int mlggd_mix_waves(int device, int n_utts, const int16_t *clean, const int64_t *offsets /* [n_utts+1] */,
                    const int16_t *noise, int64_t n_noise, const int64_t *noise_lo, const int64_t *noise_len,
                    const int64_t *noise_start, const double *snr_db, int16_t *noisy /* packed like clean */,
                    double *gain /* optional */, int32_t *clipped /* optional */);
int mlggd_lps_stats(int device, int fs_khz, int n_utts, const int16_t *wave, const int64_t *offsets,
                    double *sums /* [2][D] */, int64_t *n_frames);
int mlggd_norm_from_stats(int D, int64_t n, const double *sums, float *mean, float *inv_std);
int mlggd_load_waves(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                     int n_utts, const int16_t *noisy, const int16_t *clean, const int64_t *offsets, int n_samples,
                     const int32_t *first_frame, int targ_offset);
int mlggd_cv_all_waves(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                       int n_utts, const int16_t *noisy, const int16_t *clean, const int64_t *offsets, int n_samples,
                       const int32_t *first_frame, int targ_offset, float *sqerr, float *abserr, float *loglik);
int mlggd_set_noise(mlggd_handle h, int64_t n_noise, const int16_t *noise);
int mlggd_train_waves(mlggd_handle h, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                      int n_utts, const int16_t *clean, const int64_t *offsets, const int64_t *noise_lo,
                      const int64_t *noise_len, const int64_t *noise_start, const double *snr_db, int n_samples,
                      const int32_t *first_frame, int targ_offset, int16_t *noisy_out /* optional */,
                      double *gain /* optional */, int32_t *clipped /* optional */, int *bunches_trained);

/* ---- state: BP_GPU::returnWeights (BP_GPU.cu:514-525) and dev.scalefactor (:287) ---- */
int mlggd_get_weights(mlggd_handle h, float *const *weights, float *const *bias);
/* mlggd_set_weights replaces W and b of every layer and leaves the momentum buffers as they are; it is ordered after
 * every step already enqueued (mlggd_train_frames_async included) and returns when the upload has completed.  A NULL
 * layer pointer is MLGGD_ERR_ARG and changes no layer. */
int mlggd_set_weights(mlggd_handle h, const float *const *weights, const float *const *bias);
int mlggd_get_scalefactor(mlggd_handle h, float *alpha /* [D] */);
int mlggd_set_scalefactor(mlggd_handle h, const float *alpha /* [D] */);
/* One shape per output bin (no counterpart in the reference, whose shapefactor is one float).  With alpha_d in closed
 * form the ML-GGD objective is a sum over the bins, E = sum_d [ n ln alpha_d + sum_n |e_nd|^beta_d / alpha_d^beta_d ],
 * alpha_d^beta_d = (beta_d / n) sum_n |e_nd|^beta_d, so column d of the loss chain depends on column d's errors and on
 * beta_d alone: with a vector set, the loss kernels of every path (fused and MLGGD_LOSS_FUSE=0, a communicator, the
 * emulated worlds) and both CV log-likelihood paths read beta from a device array, in the expressions and the order
 * of the scalar kernels -- a uniform vector gives the bits of the scalar engine, and the columns of one value give
 * the bits of a scalar engine at that value.  CV: density1 = sum_d n logf(beta_d / (2 Gamma(1/beta_d))) in double,
 * density3 with beta_d per column, density2 as before.  mlggd_error_stats* keep their own grid and are not affected.
 * mlggd_set_shapefactors is ordered after every step already enqueued, takes effect from the next step or CV call
 * and leaves the weights, the momentum buffers and the current scalefactor alone.  betas NULL: back to
 * cfg.shapefactor, the launches of an engine that never had a vector.  A beta that is not positive and finite is
 * MLGGD_ERR_ARG, found before any device call, the message names the bin; an engine with MLflag != 1 is
 * MLGGD_ERR_STATE (a beta-norm whose exponent differs per bin has no per-bin scale).  In both cases the engine stays
 * usable and unchanged.  mlggd_get_shapefactors returns the D values in effect: cfg.shapefactor D times without a
 * vector. */
int mlggd_set_shapefactors(mlggd_handle h, const float *betas /* [D], NULL: back to cfg.shapefactor */);
int mlggd_get_shapefactors(mlggd_handle h, float *betas /* [D] */);
/* mlggd_read_shapefactors: host only, no device.  Reads D shapes from a plain white-space separated list of exactly D
 * numbers, or from the file MLGGD_ERRMODEL writes: '#' lines are skipped, the rows `d mean var kurt best_beta ...`
 * must be rows 0..D-1 in order and field 5 of row d is bin d's shape.  A `nan` best_beta marks a bin without a fit:
 * it takes the file's `# shared_beta` if that line is there and finite, else `fallback`.  A file counts as an error
 * model when a '#' line precedes its first number or its first data line has five or more fields and starts with 0.
 * A wrong row or number count, a row out of order, a field that is no number and a value that is not positive and
 * finite are MLGGD_ERR_ARG with "PATH line N: ..." as the message; so are a NULL pointer, D < 1 and an unreadable
 * file. */
int mlggd_read_shapefactors(const char *path, int D, float fallback, float *betas /* [D] */);

/* ---- asymmetric GGD error model: a skew per output bin (no counterpart in the reference; csrc/asym_rule.h).  An LPS
 * regression net over-smooths, so the error e = out - targ of a bin is skewed and a symmetric density spends its
 * likelihood on a tail that is not there.  Per bin d, with shape beta_d, scale alpha_d and skew kappa_d > 0:
 *   f(e) = beta / (alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e) / alpha)^beta),
 *   s(e) = kappa e (e > 0),  (-e) / kappa (e < 0),  0 (e == 0)   -- one fp32 multiplication or one fp32 division.
 * kappa > 1 charges over-estimates more, kappa < 1 under-estimates; kappa = 1 is the GGD.  The whole loss chain carries
 * over with |e| replaced by s(e): p = s^beta, the column sum, alpha = (beta colsum / n)^(1/beta), and the gradient
 * s^(beta-1) beta / alpha^beta times ds/de (times kappa for e > 0, divided by kappa for e < 0, with the sign).  With a
 * vector set every loss path (fused and MLGGD_LOSS_FUSE=0, a communicator, the emulated worlds) runs kernels of its
 * own, k_loss_ml_asym / k_loss_err_asym / k_loss_grad_asym, and both CV log-likelihood paths use s(o - t) / alpha_d
 * in density3 and take n sum_d logf((kappa_d + 1/kappa_d) / 2) off density1.  Two identities are exact in fp32: a
 * vector of ones gives the bits of the engine without a vector, and for kappa a power of two the engine with 1/kappa,
 * the negated last layer and negated targets is the exact mirror image.
 * mlggd_set_asymmetry is ordered after every step already enqueued, takes effect from the next step or CV call and
 * leaves the weights, the momentum buffers, the scalefactor and the shape vector alone; it composes with
 * mlggd_set_shapefactors in either order (without a shape vector every bin has cfg.shapefactor).  kappas NULL: off,
 * the launches of an engine that never had a vector.  A kappa that is not positive and finite is MLGGD_ERR_ARG, found
 * before any device call, the message names the bin; MLflag != 1 is MLGGD_ERR_STATE.  In both cases the engine stays
 * usable and unchanged.  mlggd_get_asymmetry returns the D values in effect: ones when asymmetry is off. */
int mlggd_set_asymmetry(mlggd_handle h, const float *kappas /* [D], NULL: off */);
int mlggd_get_asymmetry(mlggd_handle h, float *kappas /* [D] */);
/* The sufficient statistics of that model: mlggd_error_stats with the power sums split by the sign of e and no moment
 * rows.  sums is [2 n_betas][D] doubles: row k is P+_k[d] = sum_{e>0} pow(e, beta_k), row n_betas + k is
 * P-_k[d] = sum_{e<0} pow(-e, beta_k), each term the fp32 value of the trainer's own power widened to double.  Same
 * arguments, refusals, overwrite-not-accumulate rule and bit-reproducibility as mlggd_error_stats*; additive over
 * chunks; independent of the shape and skew vectors in effect. */
int mlggd_error_stats_signed(mlggd_handle h, int n_frames, const float *in, const float *targ, int n_betas,
                             const float *betas, double *sums /* [2 n_betas][D] */);
int mlggd_error_stats_signed_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat,
                                    const float *targ, int n_samples, const int32_t *first_frame, int targ_offset,
                                    int n_betas, const float *betas, double *sums /* [2 n_betas][D] */);
/* mlggd_asym_fit: host only, no device, everything in double.  For every bin and grid shape, from n samples per bin:
 *   kappa = (P- / P+)^(1 / (2 (beta + 1)))                     the ML skew in closed form (asym_rule.h)
 *   alpha^beta = (beta / n) (kappa^beta P+ + kappa^-beta P-)
 *   loglik = n [ln beta - ln(kappa + 1/kappa) - lgamma(1/beta) - ln alpha - 1/beta]
 * kappa, alpha, loglik are [n_betas][D]; best [D] is the argmax over the grid; loglik_shared [n_betas] sums loglik over
 * the bins and best_shared is its argmax.  Ties go to the lower index.  A bin with P+ == 0 or P- == 0 has no fit:
 * kappa and loglik NaN, alpha 0, best -1, and it is left out of the shared totals (best_shared -1 when no bin has a
 * fit).  Every output pointer may be NULL.  D < 1, n < 1, a bad grid and NULL sums are MLGGD_ERR_ARG. */
int mlggd_asym_fit(int D, int64_t n, int n_betas, const float *betas, const double *signed_sums, double *kappa,
                   double *alpha, double *loglik, int32_t *best, double *loglik_shared, int32_t *best_shared);
/* mlggd_read_asymmetry: host only, no device.  Reads D skews from a plain white-space separated list of exactly D
 * numbers, or from the file MLGGD_ASYMMODEL writes: '#' lines are skipped, the rows `d p_plus p_minus alpha best_beta
 * best_kappa ...` must be rows 0..D-1 in order and field 6 of row d is bin d's skew; a `nan` there, a bin without a
 * fit, takes `fallback`.  The same file reads as a shape file through mlggd_read_shapefactors (field 5).  Errors as
 * mlggd_read_shapefactors: MLGGD_ERR_ARG with "PATH line N: ..." as the message. */
int mlggd_read_asymmetry(const char *path, int D, float fallback, float *kappas /* [D] */);

/* ---- a learned scale per output bin (the paper's second optimisation of the ML-GGD objective; the reference ships
 * the alternating one only).  MLGGD_SCALE_ALTERNATING, the default, re-solves alpha_d in closed form from every
 * minibatch: the launches of an engine that never heard of this.  MLGGD_SCALE_LEARNED keeps a state (alpha_d, v_d) per
 * bin across minibatches and moves ln alpha_d by gradient descent with momentum beside the weights (csrc/scale_rule.h
 * states the rule): v' = momentum v - lrate (1 - beta S / alpha^beta), clamped to [-vmax, vmax], alpha' = alpha
 * exp(v'); the weight gradient of a step divides by alpha^beta of the alpha BEFORE that step's update.  A bin whose
 * alpha is 0 takes the closed form of its first minibatch (the alternating engine's bits) and v = 0.  lrate = momentum
 * = 0 trains under a fixed scale vector.  It composes with mlggd_set_shapefactors and mlggd_set_asymmetry, runs on every
 * loss path (one launch, MLGGD_LOSS_FUSE=0, a communicator: every rank applies the rule to the same all-reduced sums,
 * so replicas stay identical without a new exchange), and the CV log-likelihood and mlggd_get_scalefactor read alpha
 * as before.  The defaults (lrate 0.05, momentum 0.5, vmax 1) are a choice of this project, not a measured optimum.
 *
 * Entering the learned mode takes alpha from the current scalefactor (all zero on a fresh engine) and sets v = 0;
 * calling it again in learned mode only changes the parameters.  mlggd_set_scalefactor in learned mode sets alpha and
 * leaves v.  Going back to alternating leaves scalefactor as it is; the next step overwrites it as before.
 * Refused before any device call, the engine unchanged: MLflag != 1 (MLGGD_ERR_STATE, whichever mode is asked
 * for: a beta-norm has no scale); another mode, a lrate, momentum or vmax that is not finite, lrate < 0,
 * momentum outside [0, 1), vmax <= 0 (MLGGD_ERR_ARG).  mlggd_get_scale_state / mlggd_set_scale_state need the learned
 * mode (MLGGD_ERR_STATE); an alpha that is negative or not finite, or a velocity that is not finite, is MLGGD_ERR_ARG
 * naming the bin.  velocity NULL: zeros (set), not returned (get). */
enum { MLGGD_SCALE_ALTERNATING = 0, MLGGD_SCALE_LEARNED = 1 };
int mlggd_set_scale_mode(mlggd_handle h, int mode, float lrate, float momentum, float vmax);
int mlggd_get_scale_mode(mlggd_handle h, int *mode, float *lrate, float *momentum, float *vmax, int64_t *steps);
int mlggd_get_scale_state(mlggd_handle h, float *alpha /* [D] */, float *velocity /* [D] or NULL */);
int mlggd_set_scale_state(mlggd_handle h, const float *alpha /* [D] */, const float *velocity /* [D] or NULL: zeros */);
/* Host only, no device.  The state as a text file: '#' header lines with D, the mode's parameters and the step count,
 * then the rows `d alpha velocity`, every number in %.9g so that a round trip keeps every bit.  The reader skips '#'
 * lines; a wrong row count, a row out of order, a field that is no number, an alpha that is negative or not finite, a
 * velocity that is not finite and a file that cannot be read are MLGGD_ERR_ARG with "PATH line N: ..." as the message;
 * so are a NULL path or alpha and D < 1. */
int mlggd_read_scale_state(const char *path, int D, float *alpha /* [D] */, float *velocity /* [D] or NULL */);
int mlggd_write_scale_state(const char *path, int D, const float *alpha /* [D] */, const float *velocity /* [D] or NULL: zeros */,
                            float lrate, float momentum, float vmax, int64_t steps);

/* ---- Adam beside SGD with momentum (Kingma and Ba 2015; the reference ships the SGD rule only).  MLGGD_OPT_SGD, the
 * default, is the engine every other entry describes: the launches and allocations of an engine that never heard of
 * this.  MLGGD_OPT_ADAM keeps two moments (m, v) per weight and per bias on the device (csrc/adam_rule.h states the
 * rule): g = G / n + weightcost w (the SGD rule's gradient expression; no weightcost on a bias), m' = beta1 m +
 * (1 - beta1) g, v' = beta2 v + (1 - beta2) g g, w' = w - a_t m' / (sqrt(v') + eps), with the bias correction folded
 * into the step size a_t = lrate sqrt(1 - beta2^t) / (1 - beta1^t), formed on the host in double from running products.
 * A step forms the gradient with the unfused dW launches of the all-reduce exchange -- same kernels, same plan
 * (mlggd_debug_gemm_plan) -- and applies the rule in ONE more launch over all layers; nothing else in a step changes,
 * so every training entry, loss configuration, activation, dropout, mask and NAT engine works unchanged.  lrate and
 * mlggd_set_lrate are the Adam rate, momentum is ignored in the mode, weightcost stays the L2 term inside g.  RBM
 * sessions keep their own rule.  Not built: decoupled decay (AdamW), AMSGrad, a rate per layer, the data-parallel
 * exchanges.  No default here has been evaluated on speech.
 *
 * mlggd_set_optimizer: entering Adam -- also from Adam -- zeroes m and v and sets steps = 0, behind every step already
 * enqueued; the SGD momentum buffers are left alone in both directions, so going back to SGD continues from the deltas
 * it had.  Refused before any device call, the engine unchanged: a kind other than the two, beta1 or beta2 outside
 * [0, 1), an eps that is not finite or <= 0 (MLGGD_ERR_ARG, whichever kind is asked for); Adam on an engine that has
 * joined a communicator or an emulated world (MLGGD_ERR_STATE), as are mlggd_comm_init / mlggd_debug_fake_world on an
 * engine in the mode.  mlggd_get_optimizer: any pointer may be NULL; steps counts the updates since the mode was entered
 * or the state set.  mlggd_get_optimizer_state / mlggd_set_optimizer_state move the moments unpadded, in the shapes and
 * with the slot-0-unused pointer arrays of mlggd_get_weights; they need the mode (MLGGD_ERR_STATE); negative steps, a
 * moment that is not finite and a negative second moment are MLGGD_ERR_ARG. */
enum { MLGGD_OPT_SGD = 0, MLGGD_OPT_ADAM = 1 };
int mlggd_set_optimizer(mlggd_handle h, int kind, float beta1, float beta2, float eps);
int mlggd_get_optimizer(mlggd_handle h, int *kind, float *beta1, float *beta2, float *eps, int64_t *steps);
int mlggd_get_optimizer_state(mlggd_handle h, float *const *m_w, float *const *v_w, float *const *m_b, float *const *v_b);
int mlggd_set_optimizer_state(mlggd_handle h, const float *const *m_w, const float *const *v_w, const float *const *m_b,
                              const float *const *v_b, int64_t steps);
/* Host only, no device: the rule of csrc/adam_rule.h, compiled for the host, on n values in place -- update number
 * steps_before + 1 of a run.  G is the summed gradient, nf the minibatch size.  MLGGD_ERR_ARG: n or steps_before < 0, a
 * NULL array with n > 0, betas or eps mlggd_set_optimizer would refuse. */
int mlggd_adam_apply(float *w, float *m, float *v, const float *G, int64_t n, float nf, float weightcost, float lrate, float beta1,
                     float beta2, float eps, int64_t steps_before);
/* Host only, no device.  The state as a binary little-endian file (host/optfile.h states the format): a magic word, a
 * version, the layer sizes, the betas, eps and steps, then m and v per layer, unpadded.  The pointer arrays have slot 0
 * unused.  mlggd_read_optimizer_header returns the sizes (layersizes: room for MLGGD_MAXLAYER) so that a caller can
 * allocate; mlggd_read_optimizer_state is told the sizes it expects and refuses a file for another net naming both.
 * A file that ends early, bytes behind the last array, another magic or version and a file that cannot be read or
 * written are MLGGD_ERR_ARG with "PATH: ..." as the message. */
int mlggd_write_optimizer_state(const char *path, int numlayers, const int32_t *layersizes, const float *const *m_w,
                                const float *const *v_w, const float *const *m_b, const float *const *v_b, float beta1, float beta2,
                                float eps, int64_t steps);
int mlggd_read_optimizer_header(const char *path, int32_t *numlayers, int32_t *layersizes, float *beta1, float *beta2, float *eps,
                                int64_t *steps);
int mlggd_read_optimizer_state(const char *path, int numlayers, const int32_t *layersizes, float *const *m_w, float *const *v_w,
                               float *const *m_b, float *const *v_b, float *beta1, float *beta2, float *eps, int64_t *steps);

/* ---- global variance equalisation (Xu, Du, Dai and Lee 2015; no counterpart in the reference).  A regression net
 * trained under MMSE or ML over-smooths: per bin the variance of its output is smaller than the clean target's.  The
 * post-filter is one factor per bin (or one for all bins) multiplied onto the NORMALISED network output before it is
 * de-normalised.  The rule is csrc/gv_rule.h.
 *
 * mlggd_output_stats / mlggd_output_stats_frames mirror mlggd_error_stats / _frames: the chunk is loaded WITH its
 * targets, the CV forward runs per bunch (trailing partial bunch included) and one kernel per bunch folds the bunch
 * into sums kept on the device.  Per element y = slab sum + bias in fp32 (the bits mlggd_forward returns), t the fp32
 * target; on return
 *   sums[0][d] = sum y    sums[1][d] = sum y*y    sums[2][d] = sum t    sums[3][d] = sum t*t       (sums is [4][D])
 * every term formed in double from the fp32 value.  OVERWRITTEN, not accumulated: the statistics are additive, a
 * caller with several chunks adds the arrays.  Two calls return the same bits and the two entries return the same
 * bits for the same rows; 4 * D doubles come back, nothing of size n x D.  n_frames / n_samples == 0 returns zeros.
 * NULL pointers and a shape mismatch are MLGGD_ERR_ARG; an engine with a communicator or an emulated world, or with
 * dropoutflag != 0, and the _frames entry on a NAT engine (the expanded entry works there) are MLGGD_ERR_STATE.  All
 * are found before any device call and the engine stays usable and unchanged. */
int mlggd_output_stats(mlggd_handle h, int n_frames, const float *in, const float *targ, double *sums /* [4][D] */);
int mlggd_output_stats_frames(mlggd_handle h, int n_frames, int fea_context, const float *feat, const float *targ,
                              int n_samples, const int32_t *first_frame, int targ_offset, double *sums /* [4][D] */);
/* mlggd_gv_fit: host only, no device, all in double with + - * / sqrt alone: the fit to sums over n samples (added
 * over the chunks by the caller).  mu = S1/n, r2 = S2/n, gv = r2 - mu*mu for the outputs (gv_est) and the targets
 * (gv_ref); eta[d] = (float)sqrt(gv_ref[d] / gv_est[d]).  A bin with gv_est <= 0 or gv_ref <= 0 (a constant output, a
 * constant target, n == 1) has no fit: eta 1, fitted 0.  The shared factor is the same expressions on the sums of the
 * fitted bins, added in bin order, over n times the number of fitted bins (n * D when every bin has a fit) samples:
 * the paper's dimension-independent factor.  No fitted bin: eta_shared 1, fitted_shared 0.  Every output pointer is
 * optional.  n <= 0, D < 1 and NULL sums are MLGGD_ERR_ARG. */
int mlggd_gv_fit(int D, int64_t n, const double *sums /* [4][D] */, double *gv_est, double *gv_ref, float *eta,
                 uint8_t *fitted, double *gv_est_shared, double *gv_ref_shared, float *eta_shared,
                 int32_t *fitted_shared);
/* mlggd_set_gv: with a vector set, every decoder that de-normalises the net's output -- mlggd_enhance_wave, _waves,
 * _scored, _scored_stoi and mlggd_live_push -- forms  v = ((y * eta[k]) / inv_std[k]) + mean[k],  three IEEE fp32
 * operations from left to right; lps_out and the scores are those of the equalised rows, which are what is
 * synthesised.  A vector of exact ones gives the bits of an engine without factors.  mlggd_lps_to_wave,
 * mlggd_score_waves, mlggd_forward*, CV, training and mlggd_error_stats* / mlggd_output_stats* are not affected.
 * The upload is ordered after everything already enqueued and takes effect from the next decode call or push; the
 * weights, the momentum buffers, the scalefactor and the shape factors stay as they are.  eta NULL: off, the launches
 * of an engine that never had a vector.  An eta[d] that is not positive and finite is MLGGD_ERR_ARG, found before any
 * device call, the message names the bin, and the engine stays unchanged.  Works on sigmoid, ReLU and NAT engines.
 * A live group reads the engine's factors at each push: its bit-identity with mlggd_enhance_wave refers to the
 * factors in effect and holds while they do not change during a recording.
 * mlggd_get_gv returns the D values in effect: ones when off. */
int mlggd_set_gv(mlggd_handle h, const float *eta /* [D], NULL: off */);
int mlggd_get_gv(mlggd_handle h, float *eta /* [D]; ones when off */);
/* mlggd_read_gv: host only, no device.  Reads D factors from a plain white-space separated list of exactly D numbers,
 * or from the file MLGGD_GVFILE writes: '#' lines are skipped ('# shared_eta X' is remembered), the rows
 * `d gv_ref gv_est eta` must be rows 0..D-1 in order and field 4 of row d is bin d's factor.  A `nan` marks a bin
 * without a fit and takes 1.  shared != 0 fills all bins with the file's shared_eta (nan: 1); a plain list has none.
 * A file counts as the trainer's when a '#' line precedes its first number or its first data line has four or more
 * fields and starts with 0.  A wrong row or number count, a row out of order, a field that is no number, a value that
 * is not positive and finite and a file that cannot be read are MLGGD_ERR_ARG with "PATH line N: ..." as the
 * message; a NULL pointer and D < 1 are MLGGD_ERR_ARG too. */
int mlggd_read_gv(const char *path, int D, int shared, float *eta /* [D] */);

/* ---- multi-objective learning with mask-based post-processing (the regression-DNN recipe of Xu, Du, Dai and Lee; no
 * counterpart in the reference).  An engine created with mlggd_config.mask_bins = M >= 1 has 2 M outputs per frame:
 * the clean LPS and a ratio mask.  The rule is csrc/mask_rule.h; M must be the bin count D of the rate a wave entry is
 * called with.  All fp32, one IEEE operation per step, nothing contracted.
 *
 * Targets.  mlggd_load_waves, mlggd_cv_all_waves and mlggd_train_waves on a mask engine form target rows [clean LPS
 * normalised as before | t], t = scale * min(1, exp_det(0.5f * (c - y))) from the UN-normalised clean and noisy LPS c,
 * y: the clean-to-noisy magnitude ratio capped at 1, not z-normalised; exp_det is the kernels' IEEE-only exponential
 * ("exp_det" of mlggd_debug_math).  scale is the engine's (mlggd_set_mask).  mlggd_mask_targets runs the same device
 * arithmetic on n_frames given rows of D bins (out [n_frames][D]) for callers who build frame targets themselves; the
 * frame entries (mlggd_train_frames, ...) are generic in the output width and take such 2 M-wide rows as they are.
 * Under MMSE the mask half weighs scale^2 against the LPS half; under ML-GGD every bin has its own alpha and
 * mlggd_set_shapefactors can give the mask half beta = 2.  mlggd_cv_all* sum over all 2 M outputs.
 *
 * Decoding.  mlggd_enhance_wave, _waves, _scored and _scored_stoi take a mask engine as they are.  With o the 2 D
 * outputs of a frame, x the de-normalised estimate of bin k exactly as on an engine without a mask (o[k] / inv + mean,
 * or with the factors of mlggd_set_gv, of whose 2 D values the first D are read), n the noisy LPS of that frame and bin:
 *   m = o[D + k] / scale      v = m > hi ? n : (m >= lo ? 0.5f * (n + x) : x)          a NaN mask takes x
 * and v takes the place of x everywhere: the magnitudes, lps_out, the scores.  MLGGD_MASK_OFF: v = x, the mask half is
 * ignored.  A new engine has MLGGD_MASK_SELECT, lo 0.25, hi 0.75, scale 1: a choice, not a measured optimum.
 * mlggd_set_mask takes effect from the next call on; lo > hi, a value that is not finite, scale <= 0 and another mode
 * are MLGGD_ERR_ARG, any call on an engine without mask_bins is MLGGD_ERR_STATE, and the engine stays unchanged.
 * mlggd_live_open on a mask engine is MLGGD_ERR_STATE (a live group would need the noisy rows of the frames it
 * decodes in a second ring), and a wave entry at a rate whose D != mask_bins is MLGGD_ERR_ARG.
 * mlggd_mask_select: host only, no device; out[i] = the post-filter of (noisy_lps[i], lps[i], m = mask[i]) over n rows
 * of D values, straight from the header: the float32 statement tests and users compare against. */
enum { MLGGD_MASK_OFF = 0, MLGGD_MASK_SELECT = 1 };
int mlggd_set_mask(mlggd_handle h, int mode, float lo, float hi, float scale);
int mlggd_get_mask(mlggd_handle h, int *mode, float *lo, float *hi, float *scale); /* every pointer optional */
int mlggd_get_mask_bins(mlggd_handle h, int *mask_bins); /* the mask_bins the engine was created with */
int mlggd_mask_targets(int device, int D, int64_t n_frames, const float *noisy_lps, const float *clean_lps, float scale,
                       float *out /* [n_frames][D] */);
int mlggd_mask_select(int D, int64_t n, const float *noisy_lps, const float *lps, const float *mask, float lo, float hi,
                      float *out /* [n][D] */);
int mlggd_set_lrate(mlggd_handle h, float lrate);
int mlggd_get_activation(mlggd_handle h, int *act); /* MLGGD_ACT_* the engine was created with */
/* CV metrics: on = the three sums are formed on the device (per-tile partials in double, combined
 * on the host; no n x D copy, no host loop); off (default, or env MLGGD_CV_DEVICE=0) = outputs copied back and
 * accumulated on the host in fp32 in the reference's frame-major order (BP_GPU.cu:207-213), the values the
 * reference's log lines carry.  The two differ by the rounding of that fp32 accumulation, which grows with the size
 * of the CV set: 1e-5 relative at 1,200 frames, 1.4e-3 at 7,920 frames x 257 (the running sum is then ~1e7 times a
 * term); the device sums are the accurate ones, the host-order ones are what the reference prints. */
int mlggd_set_cv_device_reduce(mlggd_handle h, int on);
float mlggd_gamma(float x); /* BP_GPU::Gamma, BP_GPU.cu:593-640 */

/* Copies an internal tensor of the LAST step to the host in the reference's row-major
 * layout (parity tests).  name: "out" "y" "dedx" [bunchsize][units(layer)];
 * "delta_w" "weights" [K][N]; "delta_b" "bias" [N]; "scalefactor" [D].
 * count = capacity of dst in floats; fails if too small. */
int mlggd_debug_tensor(mlggd_handle h, const char *name, int layer, float *dst, size_t count);

/* ---- data parallel over the GPUs of one node (new work): one process per
 * GPU; rank r trains rows [r*bunchsize,(r+1)*bunchsize) of every global minibatch of
 * world*bunchsize frames.  Exchanges per step (RCCL): the per-dimension sum |e|^beta (ML only,
 * all-reduce of 257 floats) and ONE of three forms of the gradient exchange (mlggd_dp_mode below):
 * an all-reduce of the weight/bias gradients; an all-gather of the gradient's FACTORS (every rank's
 * Y_{l-1} and dEdX_l rows) after which each rank forms the global-minibatch gradient itself; or the
 * factor all-gather with each rank updating only its block of weight rows, followed by an all-gather
 * of W.  Every 1/n_frames factor uses the GLOBAL minibatch size, so the run equals a single-device
 * run with bunchsize = world*bunchsize.  rank 0 fills a unique id, the caller broadcasts it out of
 * band.  Status: tested on one GPU only (1-rank communicator; emulated worlds of 2-8 ranks with
 * different rows per rank); never run between two GPUs -- the mode thresholds are a cost model. */
int mlggd_comm_unique_id(void *id /* MLGGD_UNIQUE_ID_BYTES */);
int mlggd_comm_init(mlggd_handle h, const void *id, int world_size, int rank);
/* what RCCL itself reports for the engine's communicator (ncclCommCount / ncclCommUserRank); 0 / -1 without one.
 * bench.py prints it as `rccl_ranks` so a multi-GPU line proves the collectives ran over that many ranks. */
int mlggd_comm_info(mlggd_handle h, int *nranks, int *rank);

/* Per-step device time of the last mlggd_train_resident call, measured with HIP events
 * on the engine's stream: total ms over `steps` steps. */
int mlggd_last_train_ms(mlggd_handle h, float *ms, int *steps);

/* Kernel-class timing INSIDE a timed mlggd_train_resident region (bench.py's roofline
 * object): mlggd_profile_select times every launch of the named class ("transpose" "fwd"
 * "loss" "dx" "dw" "update"; layer 0 = all layers) with a pair of HIP events, up to
 * max_launches of this call (a later call with a smaller number lowers the limit); NULL/"" switches it off.  The GEMM classes ("fwd" "dx" "dw") take the pair INTO
 * the launch (hipExtLaunchKernelGGL start/stop events = the dispatch's own begin/end timestamps,
 * what rocprofv3 --kernel-trace reports); the other classes are bracketed by events recorded on
 * the stream before and after, which adds the bracket's cost.  mlggd_profile_read syncs and returns
 * the mean launch duration in microseconds and the number of launches seen.
 * mlggd_kernel_work gives the algorithmic FLOPs / bytes of ONE launch of (class, layer)
 * (layer 0 = summed over layers), the figures DESIGN.md states per kernel. */
int mlggd_profile_select(mlggd_handle h, const char *kernel_class, int layer, int max_launches);
int mlggd_profile_stride(mlggd_handle h, int every_nth_step); /* bracket only every n-th step (default 1) */
int mlggd_profile_read(mlggd_handle h, float *mean_usec, int *launches);
/* cost of one event bracket itself (in-process calibration: 2*T(one kernel) - T(two kernels)) */
int mlggd_profile_overhead(mlggd_handle h, float *usec);
int mlggd_kernel_work(mlggd_handle h, const char *kernel_class, int layer, double *flops, double *bytes);
/* how many launches of the weight-gradient/update kernel one training step issues: 1 when the
 * layers share one persistent launch (single GPU), numlayers-1 otherwise */
int mlggd_dw_launches_per_step(mlggd_handle h, int *launches);
/* 0 = single device, 1 = data parallel by all-reduce of the weight gradients, 2 = by all-gather of their
 * factors with the update replicated on every rank, 3 = the same with the update sharded over the ranks and
 * W all-gathered, 4 = 3 with the activations exchanged by all-to-all, each rank receiving only the units of its block
 * of weight rows (opt-in: MLGGD_DP_MODE=shard_a2a) (defaults: 2 up to 5 ranks, 3 from 6 ranks, 1 where the shape rules out the gather --
 * bunchsize % 32 != 0 or world*bunchsize not in {64,128,256,512,1024}; MLGGD_DP_MODE=allreduce|gather|shard
 * at comm init overrides) */
int mlggd_dp_mode(mlggd_handle h, int *mode);
/* Test hook: emulate `world_size` ranks on one GPU (device copies / adds instead of collectives).  Every
 * training step then consumes world_size*bunchsize rows of the resident chunk, emulated rank r owning rows
 * [r*bunchsize,(r+1)*bunchsize) of them.  mode: 0 = factor all-gather + replicated update, 1 = factor
 * all-gather + sharded update, 2 = gradient all-reduce, 3 = sharded update with the activations by all-to-all. */
int mlggd_debug_fake_world(mlggd_handle h, int world_size, int mode);
/* Test hook: per-rank read-back of a training step.  mlggd_debug_keep_ranks(h, 1) (after mlggd_debug_fake_world, or
 * before it, and before training) makes every step copy what emulated ranks 0..world-2 computed -- device-to-device
 * copies on the engine's stream, taken where each rank produced it; nothing else of the step changes.  Off (the
 * default): no allocation and no extra launch.  mlggd_debug_rank_tensor then returns rank `rank`'s tensor of the
 * last step, row-major and un-padded: "x" [bunchsize][units(0)] = the input rows the step's kernels consumed (after
 * input dropout); "y" (layer 1..numlayers-2), "dedx" (layer 1..numlayers-1) [bunchsize][units(layer)]; "out"
 * [bunchsize][units(numlayers-1)].  The rank whose step ran last (the last emulated rank; a communicator's own rank;
 * rank 0 on one device) reads the current buffers and needs no snapshot. */
int mlggd_debug_keep_ranks(mlggd_handle h, int on);
int mlggd_debug_rank_tensor(mlggd_handle h, const char *name, int layer, int rank, float *dst, size_t count);
/* Test hook: number of launch plans (tile-record tables) the persistent dW kernel has cached; constant after the
 * first steps of a run (2 on one GPU, a few in the data-parallel modes). */
int mlggd_debug_plan_count(mlggd_handle h, int *plans);
/* Test hook: the engine's growable device buffers (csrc/devbuf.h: raw sets, chunk buffers, workspaces, launch-plan
 * tables) and those of its open live groups.  allocations: device allocations they have made since mlggd_create, a
 * count that never falls; bytes: what they hold now.  A call in the steady state -- no capacity exceeded -- leaves
 * `allocations` as it was; mlggd_live_close lowers `bytes` by what the group held. */
int mlggd_debug_buffers(mlggd_handle h, int64_t *allocations, int64_t *bytes);

/* Test hook: the number of split-K slabs of the output-layer forward GEMM (the loss kernel adds them in order).  The
 * oracle's MFMA-order twin needs it to restate the HIP path's summation order (oracle/mlggd_oracle.c). */
int mlggd_debug_out_slabs(mlggd_handle h, int *slabs);
/* Test hook: into how many waves' contiguous ranges layer `layer`'s forward GEMM and its dX GEMM (the one that produces
 * dEdX of layer - 1) cut their reduction: 4 = one 32 x 32 output tile per workgroup (k_fwd / k_dx), 1 = the 64 x 64-tile
 * kernels for large minibatches (k_fwd64 / k_dx64: one chain per output element).  The MFMA-order twin restates it. */
int mlggd_debug_gemm_plan(mlggd_handle h, int layer, int *fwd_waves, int *dx_waves);

/* Diagnostic: out[i] = fn(x[i], y) evaluated on the device -- fn "pow_det" (the loss chain's power: kernindex2 / kernfunc2 /
 * kernSubClean2, DevFunc.cu:219-227,468-489,376-398), "exp_det", "sigmoid" = 1 / (1 + exp_det(-x)) (kernSigmoid,
 * DevFunc.cu:36-51), "relu" = (x < 0) ? 0 : x (the MLGGD_ACT_RELU epilogues' rule): what the kernels themselves evaluate, IEEE operations only, restated in the oracle's MFMA-order twin --
 * the parity tests require the SAME BITS on both sides for every argument; "div" = x / y (IEEE); and, for the record only,
 * ocml's own "powf" and "expf", which no kernel calls: how far they sit from the correctly rounded values, in ulps. */
int mlggd_debug_math(mlggd_handle h, const char *fn, const float *x, float y, float *out, size_t n);

/* Diagnostic (not part of the reference surface): in-kernel phase stamps of the NEXT launch of
 * (class "fwd"|"dx"|"dw", layer): 8 int64 slots per workgroup in 100 MHz ticks
 * (s_memrealtime); slot meaning per kernel is documented at stamp() call sites in
 * csrc/kernels.hip.h.  The stamps go to a debug buffer only.  The selection is consumed by the first launch that
 * takes it; mlggd_debug_stamp_read then returns one row per workgroup of that launch.  Launches that carry no stamps
 * (the output layer's forward GEMM, the 64 x 64-tile kernels k_fwd64 / k_dx64) and launches of more workgroups than the
 * buffer has rows (8192) leave it at 0 rows.  ("dw", -1): the phase twin of the merged update kernel, 2 x grid rows. */
int mlggd_debug_stamp_select(mlggd_handle h, const char *kernel_class, int layer);
int mlggd_debug_stamp_read(mlggd_handle h, long long *out /* [cap_blocks][8] */, int cap_blocks, int *blocks);

/* ---- pre-training (no counterpart in the reference, whose finetune.pl starts from ./pretraining_weights/...): one
 * restricted Boltzmann machine on hidden layer `layer` (1 .. numlayers - 2) of a sigmoid engine, trained by one-step
 * contrastive divergence as csrc/rbm_rule.h states it.  The session updates the engine's own W and bias of that layer in
 * place; the visible bias and the momentum of W, bias and visible bias are the session's (0 at open), the engine's
 * fine-tuning momentum is not touched.  visible: MLGGD_RBM_GAUSSIAN (unit variance, linear reconstruction: layer 1 on
 * z-normalised input) or MLGGD_RBM_BERNOULLI.  Layers below `layer` are run by the engine's ordinary forward pass.
 * Dropout flags are IGNORED by pre-training: nothing is omitted and no weight is scaled, whatever mlggd_config says.
 * MLGGD_TILE64 applies to the forward launches below `layer`; the RBM's own products always take the 32 x 32-tile kernels.
 * Refused before any device call: layer or visible out of range (MLGGD_ERR_ARG); a rectified-linear engine, a NAT
 * engine, an engine with a communicator or an emulated world, a second open session on the engine (MLGGD_ERR_STATE);
 * mlggd_destroy while a session is open (MLGGD_ERR_STATE).  Between two session calls every other entry works and sees W
 * and bias as pre-training left them.  Not built: CD-k for k > 1, persistent chains, sampled visibles, learnt variances. */
enum { MLGGD_RBM_GAUSSIAN = 0, MLGGD_RBM_BERNOULLI = 1 };
typedef struct mlggd_rbm *mlggd_rbm_handle;
int mlggd_rbm_open(mlggd_handle h, int layer, int visible, float lrate, float momentum, float weightcost, uint32_t seed,
                   mlggd_rbm_handle *out);
int mlggd_rbm_set_rates(mlggd_rbm_handle r, float lrate, float momentum); /* momentum ramp between epochs */
/* One CD-1 step on every FULL bunch of the chunk (a trailing partial bunch is skipped, as in mlggd_train_chunk);
 * *bunches: steps run; *recon_sqerr: sum over those steps of sum (v0 - v1)^2, float64 on the device, the same bits for
 * the same input.  _frames: the chunk as a frame stream and the first frame of every sample (mlggd_load_frames).
 * mlggd_last_train_ms then gives the device time and the step count of the call's steps (upload excluded). */
int mlggd_rbm_train_chunk(mlggd_rbm_handle r, int n_frames, const float *in, int *bunches, double *recon_sqerr);
int mlggd_rbm_train_frames(mlggd_rbm_handle r, int n_frames, int fea_context, const float *feat, int n_samples,
                           const int32_t *first_frame, int *bunches, double *recon_sqerr);
int mlggd_rbm_visible_bias(mlggd_rbm_handle r, float *c /* [K] */);
/* Test hook: a tensor of the last step, row-major and un-padded.  "v0", "v1" [B][K]; "h0p", "h0s", "h1p" [B][N];
 * "delta_w" [K][N]; "delta_b" [N]; "delta_c", "vbias" [K]  (K, N: units of layer - 1 and layer, B: bunchsize). */
int mlggd_rbm_debug_tensor(mlggd_rbm_handle r, const char *name, float *dst, size_t count);
int mlggd_rbm_close(mlggd_rbm_handle r); /* gives the session's device bytes back */
/* r [B][N] of step `step` of a session opened with `seed` (rbm_rule.h); host only */
int mlggd_rbm_draws(uint32_t seed, uint32_t step, int B, int N, float *r);

#ifdef __cplusplus
}
#endif
#endif /* MLGGD_H */
