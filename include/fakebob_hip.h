/*
 * fakebob_hip.h -- C ABI of libfakebob_hip.so, the MI355X (gfx950) engine for
 * the FAKEBOB NES attack hot path.
 *
 * The reference has no FFI: its hot path crosses a *process* boundary
 * (subprocess.Popen of Kaldi programs).  Each entry point below replaces one
 * Python-level interface of the reference; the reference-side binding a
 * maintainer would add is a ctypes stub.
 *
 *   entry point               replaces (reference file:line)
 *   ------------------------  -------------------------------------------------
 *   fb_load_gmm               model_list / ubm paths handed to the wrappers
 *                             (gmm_ubm_OSI.py:15,45; attackMain.py:55,73-83)
 *   fb_set_frontend           pre-models/conf/{mfcc,vad}.conf + delta_opts read
 *                             by gmm_ubm_kaldiHelper.py:133,153,191
 *   fb_set_input_transform    (none: the input-transformation defences of the paper's evaluation,
 *                             placed in front of the recogniser)
 *   fb_set_feature_compression (none: SpeakerGuard's feature-level defence FeCo -- k-means over an utterance's
 *                             frames, the cluster centres scored in their place)
 *   fb_score_i16 / _f64       gmm_ubm_kaldiHelper.score (:270-291) and the
 *                             int16 cast of gmm_ubm_OSI.py:83-85
 *   fb_system_scores          wrapper post-processing gmm_ubm_OSI.py:89,
 *                             gmm_ubm_SV.py:77, gmm_ubm_CSI.py:93
 *   fb_set_eot                (none: SpeakerGuard's EOT_size -- every NES sample scored under several draws of a
 *                             randomised victim, the losses averaged)
 *   fb_set_companions         (none: the universal perturbation of the speaker-recognition literature -- one delta for
 *                             several utterances of a speaker, the losses averaged over them)
 *   fb_get_grad               FakeBob.get_grad + loss_fn (FAKEBOB.py:223-299)
 *   fb_attack                 FakeBob.attack (FAKEBOB.py:139-221)
 *   fb_estimate_threshold     FakeBob.estimate_threshold (FAKEBOB.py:39-137)
 *   fb_attack_pso             (none in FAKEBOB: SirenAttack's particle-swarm optimisation, the other score-based black-box
 *                             attack of SpeakerGuard's evaluation, on this library's own systems)
 *   fb_attack_kenansville     (none in FAKEBOB: Kenansville, the decision-only black-box attack of that evaluation -- spectral
 *                             content is removed until the decision changes)
 *   fb_attack_hsj             (none in FAKEBOB: HopSkipJumpAttack, the decision-only attack that REACHES a decision -- from an
 *                             audio the system already decides as wanted, along the decision boundary towards the utterance)
 *   fb_get_grad_wb / fb_attack_wb     FakeBob.get_grad + loss_fn (FAKEBOB.py:223-299) and FakeBob.attack (:139-221) with the
 *                             ANALYTIC gradient of the loss in place of the NES estimate: the white-box attacks of
 *                             SpeakerGuard's evaluation (FGSM, PGD, the margin-loss CW-inf) on a GMM-UBM system
 *   fb_attack_cw2             (none in FAKEBOB: SpeakerGuard's CW2 -- Carlini-Wagner's L2 attack in tanh space with Adam and
 *                             a binary search over the constant, on that gradient; it minimises the distortion)
 *   fb_attack_psy             (none in FAKEBOB: that attack with Qin et al.'s psychoacoustic masking loss as the distortion)
 *   fb_set_wb_bpda / fb_get_grad_wb_iter   (none in FAKEBOB: the adaptive form of those attacks on a DEFENDED victim -- BPDA
 *                             through the input-transform chain and the codec, EOT over the random stages)
 *   fb_set_wb_xvector         (none in FAKEBOB: the same white-box calls on an x-vector system, the ReLU and pooling-floor decisions held constant)
 *   fb_set_wb_ivector         (none in FAKEBOB: the same white-box calls on an i-vector-PLDA system, the frames' component
 *                             selection and pruned sets held constant)
 *   fb_get_grad_ext / fb_attack_ext   the same around a foreign `model` (README.md:136)
 *   fb_get_grad_dev / fb_attack_dev   ... around a foreign model that runs on the
 *                             same GPU: the batch and the scores stay on the device
 *
 * Test / profiling hooks (no reference counterpart) live in fakebob_hip_test.h.
 *
 * Conventions: plain pointers and sizes, host memory unless a name ends in
 * _dev; every function returns 0 on success or a negative FB_E_* code and
 * leaves a message retrievable with fb_last_error() (the reference ignores
 * subprocess return codes, gmm_ubm_kaldiHelper.py:145-147 -- this is strictly
 * more).  One engine handle per (GPU, stream); a handle is not thread-safe,
 * different handles are independent.
 */
#ifndef FAKEBOB_HIP_H
#define FAKEBOB_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK 0
#define FB_E_ARG (-1)        /* bad argument / shape */
#define FB_E_HIP (-2)        /* HIP runtime error */
#define FB_E_STATE (-3)      /* model / frontend not loaded */
#define FB_E_NO_VOICED (-4)  /* an utterance has zero voiced frames (Kaldi
                                would silently drop it and mis-align rows) */
#define FB_E_NOMEM (-5)
#define FB_E_LIMIT (-6)      /* iteration cap reached (estimate_threshold) */
#define FB_E_CALLBACK (-7)   /* the score callback of a foreign model returned non-zero */

enum { FB_TASK_OSI = 0, FB_TASK_CSI = 1, FB_TASK_SV = 2 };
enum { FB_UNTARGETED = 0, FB_TARGETED = 1 };

typedef struct fb_engine fb_engine;

/* Kaldi front-end options ([EXT] conf/mfcc.conf, conf/vad.conf, delta_opts;
 * cmn flags fixed by gmm_ubm_kaldiHelper.py:196).  dither (the last field) defaults to 0. */
typedef struct {
  double sample_freq;
  int frame_length;   /* samples */
  int frame_shift;    /* samples */
  int padded_length;  /* power of two: 512 */
  int num_mel_bins;
  int num_ceps;
  double low_freq, high_freq;
  double preemph;
  double cepstral_lifter;
  int snip_edges;
  int remove_dc;
  int use_energy;
  int raw_energy;
  double energy_floor;
  double vad_energy_threshold;
  double vad_energy_mean_scale;
  double vad_proportion_threshold;
  int vad_frames_context;
  int delta_window;
  int delta_order;
  int cmn_window;
  /* 0 (default): scores keep full precision.  1: emulate the text round trip of the reference -- Kaldi prints
   * every score as a float with 6 significant digits (`ark,t` / score files) and the helpers parse that text
   * (gmm_ubm_kaldiHelper.py:236-248, ivector_PLDA_kaldiHelper.py:310-338): raw scores are rounded to float32
   * and then to 6 significant decimal digits before any post-processing. */
  int text_scores;
  /* 0 (default): later stages read the MFCC matrix as computed.  1: emulate steps/make_mfcc.sh's default
   * `copy-feats --compress=true` (gmm_ubm_kaldiHelper.py:138-140, ivector_PLDA_kaldiHelper.py:163-165): the
   * matrix takes Kaldi's lossy CompressedMatrix round trip (8-bit codes between per-column 16-bit percentile
   * anchors; 16-bit codes for <= 8 frames) before VAD, deltas and CMVN read it. */
  int compress_feats;
  /* 0 (default): the MFCC arithmetic between Kaldi's float32 storage points is float64 (k_mfcc_r16).  1: Kaldi's own
   * precision -- BaseFloat = float32 end to end --, k_mfcc_f32: float32 window / FFT / mel /
   * DCT with one rounding per operation in a fixed order (the CPU oracle's twin is bit-identical), the frame's raw
   * log-energy C0 -- what compute-vad-decision votes on -- from the exact integer energy.  Needs the recipe's shape
   * (padded_length 512, raw_energy, <= 31 mel bins); fb_set_frontend refuses it otherwise. */
  int mfcc_f32;
  /* Kaldi's --dither (compute-mfcc-feats; Kaldi's own default is 1.0 and the stock conf/mfcc.conf does not set it).
   * 0 (default): no noise, the front end is a pure function of the samples.  > 0: after a frame of frame_length samples
   * is extracted (reflection at the utterance edges included) and before DC removal, raw energy, pre-emphasis and the
   * window, sample i of frame t of utterance u becomes x[i] + dither * z(u, t, i), z standard normal, drawn per (utterance,
   * frame, sample-in-frame) -- a waveform sample gets independent noise in each of its overlapping frames, as in Kaldi -- by
   * the "Dither RNG contract" below.  Negative or non-finite: FB_E_ARG. */
  double dither;
} fb_frontend_cfg;

/* FakeBob hyper-parameters (FAKEBOB.py:21-37) + attack() arguments (:139) +
 * the RNG contract that replaces the unseeded np.random.normal (:234). */
typedef struct {
  int task;          /* FB_TASK_* */
  int attack_type;   /* FB_UNTARGETED / FB_TARGETED */
  double adver_thresh;
  double epsilon;
  int max_iter;
  double max_lr, min_lr;
  int samples_per_draw;
  double sigma;
  double momentum;
  int plateau_length;
  double plateau_drop;
  double threshold;  /* attack(threshold=...) */
  int target;        /* attack(target=...)  (index into speakers) */
  int true_label;    /* attack(true=...) */
  uint64_t seed;     /* Philox4x32-10 key */
  uint32_t stream;   /* Philox counter word 3 (utterance / attack id) */
  int bits_per_sample; /* attack(bits_per_sample=...): the int16 casts use 2^(bits_per_sample - 1) -- of every NES
                          sample before scoring (gmm_ubm_OSI.py:85) and of the returned audio (FAKEBOB.py:220).
                          2 .. 16; 0 means 16 */
} fb_nes_params;

/* ---- Dither RNG contract (fb_frontend_cfg.dither > 0) ------------------------------------------------------------------
 * The normals come from the generator of the NES contract -- Philox4x32-10 and the float32 Box-Muller built from exactly
 * rounded primitives -- on a key of their own, so the two streams never meet:
 *   key     = (seed_lo ^ 0x44495448 ("DITH"), seed_hi ^ stream)
 *   counter = (i >> 2, frame index within the utterance, utterance index within the call, epoch)
 * and the four output words give z(u, t, 4 (i >> 2) .. + 3): words 0, 1 the first Box-Muller pair, words 2, 3 the second.
 *  - fb_get_grad / fb_attack / fb_estimate_threshold: seed and stream are fb_nes_params'; the utterance index is the row of
 *    the NES batch (0 = the unperturbed audio); epoch is the NES iteration (fb_get_grad's `iter`, fb_attack's loop index)
 *    or, in fb_estimate_threshold, the call's running count of front-end launches.
 *  - fb_score_*, fb_gmm_acc_stats and the fb_debug_mfcc / fb_debug_feats hooks: seed is the engine's dither seed
 *    (fb_set_dither_seed; 0 at creation), stream is 0xFFFFFFFF, epoch is the engine's scoring-call serial: 0 for the first
 *    such call after fb_set_dither_seed, one more for every later one.
 * So an attack's result depends on (seed, stream) only -- not on the engine that ran it, on the launch chain or on how
 * many iterations the host queues ahead --, and an utterance's noise does not depend on what else is in its batch. */
int fb_set_dither_seed(fb_engine *e, uint64_t seed);

/* ---- Noise RNG contract (FB_TF_NOISE stages of the input-transform chain below) -----------------------------------------
 * The normals z of a noise stage come from the same generator -- Philox4x32-10 and the float32 Box-Muller -- on a third key:
 *   key     = (seed_lo ^ 0x4E4F4953 ("NOIS"), seed_hi ^ stream)
 *   counter = (i >> 2, stage index + 8 * replica, utterance row of the un-replicated batch, epoch)
 * and the four output words give z for samples 4 (i >> 2) .. + 3 of the utterance, as in the dither contract.  `stage index`
 * is the stage's position in the chain (0 .. 7), `replica` is 0 unless fb_set_eot replicates the batch.
 * Seed, stream and epoch follow exactly the rules of the dither contract: in fb_get_grad / fb_attack / fb_estimate_threshold
 * the call's seed and stream and the NES iteration; in scoring calls (fb_score_*, fb_gmm_acc_stats, fb_debug_mfcc / _feats)
 * the engine's fb_set_dither_seed seed, stream 0xFFFFFFFF and the scoring-call serial.
 * A sample's noise depends on its absolute index i within the utterance, on nothing else of the launch.  So a defended
 * victim answers two scoring calls differently (the serial advances), an attack's result depends on (seed, stream) only,
 * and the two other streams (NES, dither) are never met. */

/* ---- input-transform chain: a defended system ---------------------------------------------------------------
 * A short list of int16 -> int16 stages (the input transformations of the FAKEBOB paper's defence study: quantisation,
 * median smoothing, down-sampling; average smoothing, low-pass / band-pass filters and room impulse responses as FIR)
 * applied on the device, in one launch, to every utterance the engine's own front end reads, between the int16 cast and
 * the MFCC.  The filter sits inside the victim:
 *  - applied in fb_score_i16 / _f64, fb_gmm_acc_stats (a defended system enrols through its filter), fb_get_grad,
 *    fb_attack, fb_estimate_threshold and the fb_debug_mfcc / fb_debug_feats hooks, for GMM and i-vector systems on
 *    every MFCC route, with or without dither (dither acts on the frames extracted from the transformed samples);
 *  - NOT applied to the batch handed to foreign models (_ext, _dev: their defence is their own), to the returned
 *    adversarial audio or to the trace's distance column.
 * Stage contract.  A stage maps the samples x[0 .. n) of ONE utterance to y[0 .. n); indices outside [0, n) read as 0 at
 * every stage; every result is exactly reproducible in numpy:
 *   FB_TF_QUANT     k = q, 1 .. 16384    y = clip(q * floor_div(x + q / 2, q)): int32 arithmetic, q / 2 integer division,
 *                                        floor_div rounds toward -inf, clip to [-32768, 32767]
 *   FB_TF_MEDIAN    k odd, 3 .. 31       y[i] = median of x[i - r .. i + r], r = (k - 1) / 2 (scipy.signal.medfilt's
 *                                        zero-padded semantics)
 *   FB_TF_FIR       k = L odd, 1 .. 511  acc = 0.0; for j = 0 .. L - 1 ascending: acc = acc + taps[j] * x[i + c - j],
 *                   taps[L] float64,     c = (L - 1) / 2; every product is rounded to float64, then the sum is, with no
 *                   finite, |h| <= 2^20  fused multiply-add; y = clip(rint(acc)), ties to even
 *   FB_TF_DECIMATE  k = q, 2 .. 64       y[i] = x[i] if i mod q == 0, else 0, i counted from the utterance's first sample
 *   FB_TF_NOISE     k = mode, 0 or 1     y[i] = clip(rint(x[i] + s * z[i])): float64, z the float32 normal of the "Noise RNG
 *                   taps[1] float64      contract" widened exactly, the product rounded, then the sum (no fused multiply-add),
 *                                        rint ties to even, clip to [-32768, 32767]; indices outside [0, n) stay 0; radius 0
 *                     k = 0 (absolute)   s = taps[0], in int16 LSBs, finite, 0 <= s <= 32768
 *                     k = 1 (SNR)        taps[0] = rho = 10^(snr_db / 10), formed by the caller, finite and > 0;
 *                                        s = sqrt((double)E / (double)n / rho), division and square root correctly rounded,
 *                                        E the exact integer sum of squares of the utterance AS IT IS HANDED TO THE CHAIN
 *                                        (a silent utterance: s = 0, y = x)
 * (FB_TF_NOISE is SpeakerGuard's additive-noise transformation AT: white Gaussian noise at a set SNR, drawn afresh at every
 *  query.  Deviation: SpeakerGuard takes the power of the signal its AT layer receives; here E is taken at the chain's
 *  INPUT wherever the stage stands, by a launch of its own in front of the chain (k_tf_power) -- the same thing when the
 *  stage comes first, which is where SpeakerGuard puts it.  A noise stage may stand anywhere and more than once.)
 * (average smoothing = FIR with taps 1 / k; audio squeezing by q = FIR, DECIMATE(q), FIR with the gain q folded into the
 * second filter's taps.)  Limits: at most 8 stages; the stages' radii (r or c; 0 for QUANT and DECIMATE) sum to at most
 * 1024.  Anything outside the contract returns FB_E_ARG and keeps the previous chain, as fb_set_frontend does.
 * n = 0 clears the chain: no launch is added and nothing else changes.  `taps` is read for FB_TF_FIR (k values) and
 * FB_TF_NOISE (one value) only and copied. */
enum { FB_TF_QUANT = 0, FB_TF_MEDIAN = 1, FB_TF_FIR = 2, FB_TF_DECIMATE = 3 };
enum { FB_TF_NOISE = 4 };  /* the randomised kind */
typedef struct { int kind; int k; const double *taps; } fb_tf_stage;
int fb_set_input_transform(fb_engine *e, const fb_tf_stage *stages, int n);

/* ---- over-the-air channel: a random room in front of the victim ---------------------------------------------------------
 * An adversarial voice played over the air reaches the victim through a room.  With a channel set every utterance the
 * chain above would see is first convolved with a room impulse response of L = taps samples drawn afresh for every
 * (query, row, utterance, draw): a direct path, a predelay of silence, then Gaussian noise under an exponential decay --
 * hundreds of milliseconds of tail where a FIR stage holds 32 (a FIXED, SHORT response is still a FIR stage).
 * Where it acts.  Directly in front of the input-transform chain, wherever the chain acts: fb_score_*, fb_gmm_acc_stats,
 * every NES batch of fb_get_grad / fb_attack / fb_estimate_threshold, fb_attack_pso's swarm, the fb_debug_mfcc / _feats
 * hooks.  With companions it acts on the composed, clipped rows: composition, then air, then the chain, then the front end.
 * NOT applied to foreign models (_ext, _dev), to the returned audio or to the distance column.  FB_E_NO_VOICED and
 * FB_E_LIMIT rules are unchanged.
 * Random numbers.  Philox4x32-10 on a key of its own:
 *   key     = (seed_lo ^ 0x41495243 ("AIRC"), seed_hi ^ stream)
 *   counter = (c0, replica rho, utterance row of the un-replicated batch, epoch)
 * seed, stream, epoch, utterance row and replica exactly by the rules of the "Noise RNG contract" and of the "Row order"
 * paragraph of fb_set_companions (rho = u * eot + j; 0 without replication): a scoring call draws afresh, an attack
 * depends on (seed, stream) only.  c0 = k >> 2 yields the four float32 normals z[4 (k >> 2) .. + 3], the words paired
 * through the float32 Box-Muller as the noise stage pairs them (words 0, 1 -> z[0], z[1]; words 2, 3 -> z[2], z[3]);
 * c0 = 0xFFFFFFFF yields the decay's word w = output word 0.
 * Arithmetic.  Float64, round to nearest, one rounding per written operation, no fused multiply-add; integers exact.
 *   decay     U = ((double)w + 0.5) * 2^-32;  rho = clip(rho_lo + U * (rho_hi - rho_lo), rho_lo, rho_hi): the difference,
 *             the product, the sum
 *   envelope  Q[0] = 1, Q[i] = Q[i - 1] * rho (i = 1 .. 63);  S = Q[63] * rho;  P[0] = 1, P[j] = P[j - 1] * S (j = 1 .. 63);
 *             e[m] = P[m >> 6] * Q[m & 63]
 *   taps      int16, Q14, d = predelay:  t[0] = 16384 (the direct path);  t[k] = 0 for 0 < k < d;
 *             t[k] = (int)min(max(rint((amp * (double)z[k]) * e[k - d]), -32767), 32767) for d <= k < L
 *   output    y[i] = sum over k = 0 .. min(i, L - 1) of t[k] * x[i - k], exact integer (|y| < 2^42);
 *             o[i] = clip16((y[i] + 8192) >> 14), arithmetic shift (floor).  The output has the input's length.
 * So amp = 0 is the identity bit for bit, and a silent row stays silent.  The chain then runs on o with its own contract
 * untouched: its noise stages draw with (replica rho, utterance row b) as always, and an SNR stage takes E from the row
 * "as it is handed to the chain" -- the channel's output.  (T60 and the direct-to-reverberant ratio become rho_* and amp
 * on the host: fakebob_amd/air_channel.py.)
 * Limits.  taps in 2 .. 4096, predelay in 1 .. taps - 1, amp finite in [0, 16384], 0 < rho_lo <= rho_hi <= 1, both
 * finite.  Anything else returns FB_E_ARG and keeps the previous setting.  p == NULL or taps == 0 clears the channel (the
 * default: no launch is added, no code path differs). */
typedef struct { int taps; int predelay; double amp; double rho_lo, rho_hi; } fb_air_params;
int fb_set_air_channel(fb_engine *e, const fb_air_params *p);

/* ---- telephone-line codec: G.711 and IMA ADPCM in front of the victim ---------------------------------------------------
 * The commonest deployment of speaker verification hears the voice through a telephone line.  With a codec set every row
 * the front end reads first goes through the encode / decode round trip of a line codec: G.711 mu-law or A-law (a
 * memoryless companding) or IMA/DVI ADPCM, 4 bit (the 32 kbit/s family; its state runs along the whole row, so a
 * perturbation's effect is not local in time).  All three are integer-exact: the contracts below agree bit for bit with
 * Python's stdlib audioop (ulaw2lin(lin2ulaw), alaw2lin(lin2alaw), adpcm2lin(lin2adpcm) on 16-bit samples).
 * Where it acts.  Directly behind the input-transform chain, wherever the chain acts: fb_score_*, fb_gmm_acc_stats (a
 * defended system enrols through its line), every NES batch of fb_get_grad / fb_attack / fb_estimate_threshold,
 * fb_attack_pso's swarm, the fb_debug_mfcc / _feats hooks.  The order is: composition, air channel, chain, codec, front end
 * -- dither acts on frames cut from the coded samples -- for GMM and i-vector systems alike, on every row the front end
 * reads: all K * eot replicas, each with a state of its own.  NOT applied to foreign models (_ext, _dev), to the returned
 * audio or to the distance column.  An SNR noise stage still takes its power at the chain's input.  FB_E_NO_VOICED,
 * FB_E_LIMIT (a batch of up to 65535 rows, as for a chain), the stop flag and fb_stats follow the chain's rules.
 * Stage contract.  Each codec maps x[0 .. n) int16 of one row to y[0 .. n) int16: the output has the input's length.  All
 * arithmetic is int32, >> is an arithmetic shift, every row is treated independently.
 *   mu-law  v = x >> 2;  neg = v < 0;  m = min(neg ? -v : v, 8159) + 33;
 *           seg = the number of entries of {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF} that m exceeds;
 *           seg == 8 (m = 8192 only): seg = 7, q = 15;  otherwise q = (m >> (seg + 1)) & 15;
 *           t = (((q << 3) + 0x84) << seg) - 0x84;  y = neg ? -t : t
 *   A-law   v = x >> 3;  neg = v < 0;  m = neg ? -v - 1 : v;
 *           seg = the number of entries of {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF} that m exceeds (0 .. 7);
 *           q = seg < 2 ? (m >> 1) & 15 : (m >> seg) & 15;  t = q << 4;
 *           u = seg == 0 ? t + 8 : seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1);  y = neg ? -u : u
 *   ADPCM   the state (vp, ix) starts at (0, 0) for every row.  For i = 0 .. n - 1:
 *           step = STEP[ix];  d = x[i] - vp;  s = d < 0;  d = |d|;  delta = 0;  vd = step >> 3;
 *           if d >= step: delta = 4, d -= step, vd += step;
 *           step >>= 1;  if d >= step: delta |= 2, d -= step, vd += step;
 *           step >>= 1;  if d >= step: delta |= 1, vd += step;
 *           vp = clip(s ? vp - vd : vp + vd, -32768, 32767);  ix = clip(ix + IDX[delta], 0, 88);  y[i] = vp
 *           (the decoder's output is the encoder's predictor, so the round trip is this sequence).
 *           IDX = {-1, -1, -1, -1, 2, 4, 6, 8};  STEP[89], the IMA table = 7 8 9 10 11 12 13 14 16 17 19 21 23 25 28 31 34
 *           37 41 45 50 55 60 66 73 80 88 97 107 118 130 143 157 173 190 209 230 253 279 307 337 371 408 449 494 544 598 658
 *           724 796 876 963 1060 1166 1282 1411 1552 1707 1878 2066 2272 2499 2749 3024 3327 3660 4026 4428 4871 5358 5894
 *           6484 7132 7845 8630 9493 10442 11487 12635 13899 15289 16818 18500 20350 22385 24623 27086 29794 32767
 * Deviation.  The codec runs at the utterance's own sampling rate, on every sample: there is no rate change here
 * (FB_TF_DECIMATE keeps zeros in place, and the codec is last).  A narrow-band line is emulated by band-limiting with FIR
 * stages in the chain first.
 * kind: one of the values below; anything else returns FB_E_ARG and keeps the previous setting.  FB_CODEC_NONE clears the
 * codec (the default: no launch is added, no code path differs). */
enum { FB_CODEC_NONE = 0, FB_CODEC_ULAW = 1, FB_CODEC_ALAW = 2, FB_CODEC_ADPCM = 3 };
int fb_set_codec(fb_engine *e, int kind);

/* ---- expectation over transformation: attacking a randomised victim ---------------------------------------------------
 * With a noise stage in the chain or dither > 0 the victim answers every query with a fresh draw.  r > 1 makes fb_get_grad
 * and fb_attack score every row of the NES batch under r independent draws and average BEFORE the gradient estimate and the
 * stop test (SpeakerGuard's FAKEBOB: EOT_size):
 *  - the transform launch (a replicating copy when the chain is empty) writes replica j of NES row b to row b * r + j; its
 *    noise stages draw with `replica` = j; the front end sees a batch of B * r utterances, so the dither counter's utterance
 *    index is the replicated row and the replicas' dither differs too;
 *  - system scores and loss_fn are formed per replica row exactly as without EOT, then
 *      loss[b] = (l[b][0] + ... + l[b][r - 1]) / r,   scores[b][s] = (sc[b][0][s] + ... + sc[b][r - 1][s]) / r
 *    in float64, j ascending, one rounding per addition and one for the division;
 *  - everything behind that -- the mean of loss[1:], the stop rule on loss[0], the plateau rule, the trace row (averaged
 *    scores), the gradient estimate -- is unchanged and sees the B averaged rows.  FB_E_NO_VOICED if ANY replica has no
 *    voiced frames.
 * r = 1 (the default) changes nothing: no launch is added.  r = 2 .. 32; anything else is FB_E_ARG and keeps the previous
 * value.  Not applied to foreign models (_ext, _dev), as the chain is not.  fb_estimate_threshold returns FB_E_STATE while
 * r > 1.  An attack whose (samples_per_draw + 1) * r exceeds 65535 rows returns FB_E_LIMIT. */
int fb_set_eot(fb_engine *e, int r);

/* ---- companion utterances: one perturbation for several utterances (a "universal" attack) -----------------------------------
 * fb_get_grad and fb_attack search for an adversarial version of ONE recording.  With companions set they search for one
 * perturbation that works on K = K1 + 1 recordings at once: the utterance handed to the call stays utterance 0, `wav`
 * [K1][N] int16 holds K1 more of exactly N samples each (copied).  It is the expectation fb_set_eot takes over the victim's
 * coin flips, taken over utterances as well.
 * Composition.  q_b[i]: the int16 sample the NES batch holds for row b (what k_perturb and the fused update write); a_0: the
 * int16 cast of the ORIGINAL audio of the call (fb_get_grad's / fb_attack's `audio`), by the cast rule and bits_per_sample of
 * the batch, made once per call; a_u: companion u = 1 .. K1.  Utterance u of NES row b is
 *     w[b][0][i] = q_b[i]                                            (q_b itself: no a_0 - a_0 detour)
 *     w[b][u][i] = clip(a_u[i] + q_b[i] - a_0[i], -32768, 32767)     int32 arithmetic
 * -- the perturbation is exactly what the attacker would submit: the int16 difference, added to another recording.
 * Row order.  Everything downstream sees r' = K * eot replicas of every NES row: replica rho = u * eot + j (utterance u, draw
 * j of fb_set_eot) is row b * r' + rho of the batch the front end scores, and rho is the `replica` of the Noise, dither and
 * FeCo contracts (K * eot <= 32 keeps stage index + 8 * rho below the 0x100 of FeCo's counter word).  The composition runs
 * in the launch that already writes the replicas; the input-transform chain acts on the composed, clipped samples, indices
 * outside [0, N) reading 0 as before; an SNR-mode noise stage takes its power E from the composed row (b, u), "as it is
 * handed to the chain".
 * Averaging.  fb_set_eot's rule with r' in place of r: system scores and loss_fn per replica row as always, then
 *     loss[b] = (l[b][0] + ... + l[b][r' - 1]) / r',   scores[b][s] likewise
 * in float64, rho ascending, one rounding per addition and one for the division.
 * Everything behind the averaging is unchanged: the stop test on loss[0], the plateau rule, the trace row (averaged scores),
 * the gradient estimate, the momentum sign step, the epsilon ball and the [-1, 1] clip around utterance 0's audio, the
 * returned adv_i16 -- all utterance 0's, as is the trace's distance column.  The perturbation to carry over is adv_i16 - a_0.
 * THE STOP TEST READS A MEAN, NOT A MAXIMUM: a mean loss below zero does not say that every utterance succeeded.
 * adver_thresh is the margin a caller raises; the Python layer re-scores every composed utterance and reports each.
 * fb_set_companions(e, wav, K1, N): 1 <= K1 <= 31, N >= 1 and K * eot <= 32 (checked here, in fb_set_eot -- a setting that
 * would break the product is FB_E_ARG there and keeps the previous value -- and at the NES calls); K1 = 0 clears the companions
 * (the default: no launch is added, no code path differs; wav and N are not read).  FB_E_ARG, the previous setting kept: K1
 * out of range, wav NULL with K1 > 0, N out of range, or -- at fb_get_grad / fb_attack -- a call whose N differs from the
 * companions'.  FB_E_NO_VOICED if ANY composed row has no voiced frames, as with EOT.  The fused finalisation and the
 * i-vector tail-loss shortcut are off while K > 1, as they are for eot > 1; fb_stats counts what the front end scored (K * eot
 * rows per NES row).  fb_estimate_threshold returns FB_E_STATE while companions are set.  Foreign models (_ext, _dev),
 * fb_score_*, fb_gmm_acc_stats and the fb_debug_* hooks of the sections above ignore companions. */
int fb_set_companions(fb_engine *e, const int16_t *wav, int K1, int64_t N);

/* ---- play offset: the perturbation plays on a loop, the victim speaks whenever they speak ---------------------------------
 * Over the air the attacker cannot time the perturbation to the victim's speech: a loudspeaker plays it on a loop and the
 * recogniser hears speech plus the perturbation at an unknown offset.  With S > 0 every replica of every NES row carries the
 * perturbation rotated by an offset tau of its own, uniform in 0 .. S.  The loop has the utterance's length N, so the rotation
 * is circular.  It is the expectation of fb_set_eot and fb_set_companions, taken over the playback timing as well.
 * Setting.  fb_set_play_offset(e, S): 0 <= S <= 2^31 - 2; anything else is FB_E_ARG and keeps the previous value.  S = 0
 * clears the setting (the default: no launch is added, no code path differs).  An NES or white-box call whose N <= S returns
 * FB_E_ARG.
 * Draw.  Philox4x32-10 on a key of its own:
 *   key     = (seed_lo ^ 0x504C4159 ("PLAY"), seed_hi ^ stream)
 *   counter = (0, replica rho, utterance row b of the un-replicated batch, epoch)
 * seed, stream, epoch, row and replica exactly by the rules of the "Noise RNG contract" and of fb_set_companions' "Row order";
 * w = output word 0 and tau = (uint32_t)(((uint64_t)w * (uint64_t)(S + 1)) >> 32).  An attack's offsets depend on (seed,
 * stream) only.
 * Composition (the names of fb_set_companions).  d_b[i] = q_b[i] - a_0[i], int32.  Utterance u, draw j of NES row b is
 *     w[b][rho][i] = clip(a_u[i] + d_b[(i - tau) mod N], -32768, 32767)        FOR EVERY u, u = 0 INCLUDED
 * where a_0 is the int16 cast of the call's original audio (utterance 0) and tau = tau(b, rho).  At tau = 0, u = 0 this is
 * q_b[i] exactly; row 0 of an NES batch (q_0 = a_0) composes to the unperturbed utterances whatever the offsets are.
 * Row order.  rho = u * eot + j, r' = K * eot <= 32, order and averaging as in fb_set_companions.
 * Order of stages.  Composition with the offset, then the air channel, the chain, the codec, the front end, dither and FeCo.
 * Those stages' own contracts stay untouched -- they draw with (rho, b) as always --, and an SNR noise stage takes its power
 * from the composed, offset row "as it is handed to the chain" (under a channel: from the channel's output, as before).
 * Route.  With an offset set a call takes the route a call with eot > 1 takes, even at K * eot = 1: the unfused finalisation
 * and no i-vector tail-loss shortcut.  One launch (k_play_compose) in front of the air and chain launches writes the B * r'
 * composed rows and their offsets; fb_stats counts what the front end scored (K * eot rows per NES row).
 * Unchanged.  Everything behind the averaging: the stop test, the plateau rule, the trace, the gradient estimate, the sign
 * step, the epsilon ball, the returned adv_i16 and the distance column -- all utterance 0's at offset 0.  The loop to play is
 * adv_i16 - a_0.  THE STOP TEST READS A MEAN OVER OFFSETS, as it reads a mean over utterances.
 * Where it acts.  fb_get_grad and fb_attack; fb_get_grad_wb* and fb_attack_wb when fb_set_wb_universal is on (together with the
 * switches the other stages need).  fb_score_*, fb_gmm_acc_stats, the fb_debug_* hooks without a contract point and foreign
 * models (_ext, _dev) ignore it, as they ignore companions.
 * Refused by name (FB_E_STATE, "not in this version") while S > 0: fb_estimate_threshold; fb_attack_pso, fb_attack_kenansville
 * and fb_attack_hsj, with or without fb_set_query_eot; fb_attack_cw2 and fb_attack_psy; the white-box calls when
 * fb_set_wb_universal is off.  Not modelled either: a loop shorter than the utterance, zero-filled instead of circular offsets.
 * Transposed rule (white box; k_wb_play_compose_t in k_wb_compose_t's place, also at K = 1, one launch per iteration).  In
 * float64, from +0.0, with one rounding per addition and a masked term adding +0.0:
 *     grad[k] = sum over rho ascending of m_rho[i] * cot_rho[i]   at i = (k + tau_rho) mod N
 * m_rho[i] = 1 where a_u[i] + d[(i - tau_rho) mod N], taken before the clip, lies inside [-32768, 32767], 0 elsewhere: a sample
 * at a rail that was not clipped passes.  The offsets are the forward's; nothing is drawn again.  Under a channel cot_rho is
 * k_air_conv_t's dx row rho; a chain's transpose reads replica rho's row from the composed buffer.  At S = 0 this is
 * k_wb_compose_t's rule, including m_0 = 1. */
int fb_set_play_offset(fb_engine *e, int64_t S);

/* ---- feature compression: a feature-level defence (SpeakerGuard's FeCo) -------------------------------------------------
 * The victim clusters the T voiced feature vectors of an utterance with k-means and scores the k = ratio * T cluster centres
 * instead of the frames.  The stage is SpeakerGuard's "final" one: behind VAD, deltas, CMVN and voiced-frame selection, in
 * front of the GMM / gselect launches, one launch more per batch (k_feature_compress).  Randomised through the k-means
 * initialisation: the case fb_set_eot was built for.
 *  - applied to the features of every utterance whose scores the engine forms: fb_score_i16 / _f64, fb_get_grad, fb_attack,
 *    fb_estimate_threshold, for GMM and i-vector systems, on every launch chain and MFCC route, with or without an
 *    input-transform chain, dither and EOT (under fb_set_eot(r) the kernel sees the B * r replicated rows and draws an
 *    initialisation per replica);
 *  - NOT applied to foreign models (_ext, _dev), to fb_gmm_acc_stats (a decision: FeCo is a test-time defence, models are
 *    enrolled on uncompressed features), to the fb_debug_mfcc / fb_debug_feats hooks (they stay the front end's) or to the
 *    returned audio.  `tv` stays the VAD's count T (k > 0 exactly when T > 0); fb_stats' counters are unchanged (its
 *    scored_frames counts the frames the front end produced, voiced or not, as before).
 * fb_set_feature_compression(e, ratio, iters): 0 < ratio <= 1 and iters in 1 .. 64 switch it on; ratio = 0 with iters = 0
 * switches it off (the default: no launch is added, no code path differs).  Anything else, NaN included, is FB_E_ARG and
 * keeps the previous setting.
 * Stage contract.  Exactly reproducible in numpy (the assignment is an arg-min: a tolerance cannot be tested, bits can):
 *   input      X[T][D] float32, the voiced rows of ONE utterance row as the front end wrote them
 *   size       k = max(1, (int)floor((double)T * ratio)): one float64 product, one floor.  T = 0 gives k = 0.
 *   keys       frame t gets the 32-bit key = word (t & 3) of Philox4x32-10 with
 *                key     = (seed_lo ^ 0x4645434F ("FECO"), seed_hi ^ stream)
 *                counter = (t >> 2, 0x100 + replica, utterance row of the un-replicated batch, epoch)
 *              seed, stream, epoch, replica and utterance row exactly by the rules of the "Noise RNG contract": in
 *              fb_get_grad / fb_attack / fb_estimate_threshold the call's seed and stream and the NES iteration; in scoring
 *              calls fb_set_dither_seed's seed, stream 0xFFFFFFFF and the scoring-call serial, which the call consumes
 *   init       the k frames with the smallest (key, t) pairs are chosen; taken in ascending t they are the initial centres
 *              0 .. k - 1 (float32 copies)
 *   Lloyd      exactly `iters` iterations of {assign, update} (an implementation may stop once an iteration leaves every
 *              assignment unchanged: the result cannot change any more)
 *     assign   d(t, j): acc = 0; for dimension 0 .. D - 1 ascending: diff = x - c, sq = diff * diff, acc = acc + sq, each
 *              rounded to float32, no fused multiply-add.  Frame t goes to the centre of smallest d; the lowest j wins a
 *              tie (start at j = 0, replace on strict <)
 *     update   a centre with n > 0 members becomes (float)(S / (double)n), S the float64 sum of its members' rows added
 *              one by one in ascending t from 0.0, the division correctly rounded; a centre without members keeps its value
 *   output     the k centres in cluster order are the utterance's rows; the row offsets are the prefix sums of the k's
 * Deviations from SpeakerGuard: its k-means (kmeans_pytorch) runs to a tolerance on an unseeded generator and returns the
 * centres in its own order; here the iteration count is fixed, the generator is keyed and the order is defined. */
int fb_set_feature_compression(fb_engine *e, double ratio, int iters);

/* ---- particle-swarm attack: the other score-based black-box attack (SirenAttack's PSO, as SpeakerGuard runs it) ---------
 * fb_attack searches by estimating a gradient (NES); fb_attack_pso searches without one: a swarm of P particles -- P candidate
 * audios inside the epsilon ball -- is scored as ONE batch of P rows per iteration by the path that scores every NES batch,
 * and one element-wise launch (k_pso_step) moves the swarm.  The host looks at the P losses once per iteration, as
 * fb_estimate_threshold looks at its batch, and decides the bests and the stop.
 * Read from fb_nes_params: task, attack_type, adver_thresh, epsilon, max_iter, threshold, target, true_label, seed, stream and
 * bits_per_sample.  The NES-only fields (max_lr, min_lr, samples_per_draw, sigma, momentum, plateau_*) are neither read nor
 * validated.
 * Refusals.  FB_E_ARG: particles outside 2 .. 64; w_init, w_end, c1 or c2 not finite or < 0; v_max not finite or <= 0;
 * max_iter < 1; epsilon not finite or <= 0; the task, target, true-label and bits_per_sample rules of fb_attack.  FB_E_STATE:
 * no system loaded, or fb_set_eot(r > 1) or companions (fb_set_companions) in force while fb_set_query_eot is off (the
 * default; the "voted decisions" section below says what they mean with it on): set 1 / clear them.  FB_E_NO_VOICED: some particle of some iteration has no voiced frames.  The engine's own systems (GMM and
 * i-vector); fb_attack_pso_foreign (the "foreign victims" section) runs the same swarm on a foreign model.  The input-transform chain, dither and feature compression act as in fb_attack,
 * keyed by the call's (seed, stream) with epoch = the PSO iteration k and utterance row = the particle index.
 * Arithmetic.  Everything below is float64, round to nearest, one rounding per written operation, no fused multiply-add;
 * clip(s, l, h) = min(max(s, l), h); a = `audio` as given, i the sample index, p the particle.
 *   ball       lo[i] = clip(a[i] - eps, -1, 1), hi[i] = clip(a[i] + eps, -1, 1)                        (FAKEBOB.py:163-164)
 *   uniforms   U(w) = ((double)w + 0.5) * 2^-32 for a 32-bit word w: exact, inside (0, 1).  The words are Philox4x32-10's with
 *                key     = (seed_lo ^ 0x5053574D ("PSWM"), seed_hi ^ stream)
 *                counter = (i >> 1, p, t, 0)
 *              words 0, 1 serve element 2 (i >> 1), words 2, 3 element 2 (i >> 1) + 1; of a pair the first word is u_x (t = 0)
 *              or r1 (t > 0), the second u_v or r2.  t = 0 is the initialisation, t = k + 1 the update behind iteration k.
 *   init       particle 0: x = a, v = 0.  p >= 1: x = clip(lo + u_x * (hi - lo), lo, hi) -- the difference, the product, the
 *              sum, in that order --, v = (2 u_v - 1) * v_max (2 u_v - 1 is exact).
 *   iteration k = 0 .. max_iter - 1
 *     1 score  row p of the batch is the int16 cast of x_p (the cast of every NES row: trunc(x * 2^(bits_per_sample - 1)), low
 *              16 bits); l_p = loss_fn of row p's system scores, as fb_attack forms it.  losses[k][p] = l_p.
 *     2 bests  for every p: if k == 0 or l_p < pl_p (strict) then pl_p = l_p, pb_p = x_p ("p improved").
 *              g* = the lowest p with pl_p minimal.  If k == 0 or pl_g* < gl: gl = pl_g*, gb = pb_g*, g = g*, gs = row g*'s
 *              scores of this iteration (such a g* improved in this iteration, so pb_g* = x_g*).
 *     3 trace  trace[k] = {gl, (double)g, number of particles that improved in this iteration, gs[0 .. S)}
 *     4 stop   gl < 0: *success = 1, stop.  Otherwise k == max_iter - 1: *success = -1, stop.
 *     5 move   w_k = w_init - ((w_init - w_end) * (double)k) / (double)max_iter, formed on the host.  For every p (0 included)
 *              and i, with pb and gb as they stand after step 2 and r1, r2 of t = k + 1:
 *                v' = clip((w_k * v + (c1 * r1) * (pb - x)) + (c2 * r2) * (gb - x), -v_max, v_max);  x' = clip(x + v', lo, hi)
 *   result     adv_f64 = gb, adv_i16 = its int16 cast, *n_iters = k + 1.  gb is always a position that WAS scored, so the
 *              success decision is about exactly the samples returned, as in the reference (FAKEBOB.py:220).  Rows of trace
 *              [max_iter][3 + S] and losses [max_iter][P] beyond n_iters are not written; adv_f64 may be NULL.
 * fb_attack_iter_seconds reports the seconds per iteration of the last PSO call as the host measured them (an iteration ends
 * with the host's look at its losses).  fb_stats counts the P rows per iteration in scored_utts / scored_frames as for any
 * batch; nes_iters is not advanced.
 * Deviations from SirenAttack / SpeakerGuard's PSO: their swarm draws from an unseeded generator, here the uniforms are keyed;
 * the search runs inside the epsilon ball of fb_attack (theirs clips to a ball too, SirenAttack's own to [-1, 1] only);
 * particle 0 starts at the audio itself, so gl of iteration 0 is never worse than the clean audio's loss; one swarm per
 * call -- no restarts ("epochs") and no hand-over to a gradient stage; the inertia weight falls linearly from w_init to w_end
 * over max_iter iterations. */
typedef struct { int particles; double w_init, w_end, c1, c2, v_max; } fb_pso_params;
int fb_attack_pso(fb_engine *e, const fb_nes_params *p, const fb_pso_params *q, const double *audio, int64_t N,
                  int16_t *adv_i16, double *adv_f64 /*nullable*/, int *success, int *n_iters,
                  double *trace /*[max_iter][3 + S]*/, double *losses /*[max_iter][P]*/);

/* ---- decision-only attack: Kenansville, the third black-box attack SpeakerGuard runs -------------------------------------
 * fb_attack and fb_attack_pso read scores; many deployed recognisers return a decision only.  fb_attack_kenansville reads
 * nothing else: it removes the weakest spectral content of short windows of the utterance until the decision changes, and
 * looks for the smallest removal that does so.  It is the evasion attack of the three: an enrolled speaker is no longer
 * recognised.  Every candidate is a function of the audio and ONE integer, the factor q in 0 .. 65536 (the share q / 65536
 * of a window's spectral energy that is removed, weakest bins first), so the search is a chain of batches: one launch
 * analyses the utterance once (k_kv_analyse), one launch per round writes a round's candidates straight into the int16
 * batch the front end scores (k_kv_candidates), and the host looks once per round, as it does for PSO.
 * Read from fb_nes_params: task, attack_type, threshold, target, true_label, seed, stream and bits_per_sample.  adver_thresh
 * and the NES-only fields are not read.
 * Signal contract.  All integers; >> is an arithmetic shift; exactly reproducible in numpy (the mask is a sort and a
 * threshold: a tolerance cannot be tested, bits can).  Every intermediate stays below 2^53.
 *   input      x[0 .. N): the int16 cast of `audio` (the cast of every NES row, bits_per_sample).  W = window, 8 .. 128;
 *              K = floor(W / 2) + 1 bins; nw = ceil(N / W) windows; the last window reads 0 beyond N and writes only its
 *              first N mod W samples.  Below, n = 0 .. W - 1 counts inside ONE window.
 *   tables     the caller passes four int32 tables of W entries each, one after the other (no libm in the contract):
 *                CF[j] = rint(cos(2 pi j / W) 2^30), SF[j] = rint(sin(2 pi j / W) 2^30),
 *                CI[j] = rint(cos(2 pi j / W) 2^22), SI[j] = rint(sin(2 pi j / W) 2^22).
 *              Checked: CF[0] == 2^30, CI[0] == 2^22, SF[0] == SI[0] == 0 (FB_E_ARG otherwise).
 *   analysis   once per attack, per window:
 *                A[k] = sum_n x[n] CF[(n k) mod W],  B[k] = sum_n x[n] SF[(n k) mod W],  k = 0 .. K - 1   (|A|, |B| <= 2^52)
 *                a[k] = (A[k] + 2^29) >> 30,  b[k] likewise                                             (|a|, |b| <= 2^22)
 *                p[k] = a^2 + b^2;  m[k] = 1 for k = 0 and, W even, for k = W / 2, otherwise 2;  e[k] = m[k] p[k];  E = sum e[k]
 *                the bins sorted ascending by the pair (p[k], k);  cum[k] = the sum of e over the bins up to and
 *                including k in that order
 *   candidate  for a factor q in 0 .. 65536:
 *                thr = (E >> 16) q + (((E & 0xFFFF) q) >> 16)            (= floor(E q / 65536), no overflow)
 *                bin k is removed iff cum[k] <= thr
 *                R[n] = sum over removed k of m[k] (a[k] CI[(n k) mod W] + b[k] SI[(n k) mod W])   (sum of magnitudes <= 2^48)
 *                D = W 2^22;  r[n] = floor((2 R[n] + D) / (2 D));  y[n] = clip16(x[n] - r[n])
 *              Only what is removed is ever synthesised: q = 0 is the identity bit for bit, a silent window stays silent.
 * Decisions.  Per scored row the system scores are formed exactly as fb_attack forms them (fb_system_scores' values), then
 * the system classes' make_decisions rule: SV  s >= threshold ? 1 : -1;  OSI  the first maximum's index, -1 if the
 * maximum < threshold;  CSI  the first maximum's index.  A row with no voiced frames is NO DECISION: it is written as -2,
 * it is never a success, and it does not abort the call (high factors approach silence, so this happens in ordinary use:
 * there is no FB_E_NO_VOICED here).  Success is d != true_label (untargeted) or d == target (targeted); the label is a
 * decision value: SV +-1, OSI -1 .. S - 1, CSI 0 .. S - 1.
 * Search.  grid = G rows per round, 1 .. 64; q_max 1 .. 65536; max_rounds 1 .. 32.  The bracket is (lo, hi]: lo fails, hi
 * succeeds; it starts as lo = 0 (the audio itself: taken as failing, never scored) with no hi.
 *   round 0      q_j = floor((j + 1) q_max / G), j = 0 .. G - 1, duplicates and zeros dropped
 *   later        d = hi - lo.  d - 1 <= G: lo + 1 .. hi - 1, and this is the last round.  Otherwise
 *                q_j = lo + floor((j + 1) d / (G + 1)), j = 0 .. G - 1.
 *   after        hi becomes the smallest succeeding candidate, if any; lo the largest candidate below the new hi, if any.
 *                (G = 1 is plain bisection.)
 *   stops        no success in round 0 (*success = -1, adv_i16 = x, *factor = -1);  hi - lo == 1;  the last round as
 *                defined above;  max_rounds.
 *   result       *success = 1, *factor = hi, adv_i16 = the candidate of hi -- a row that WAS scored --, *n_queries = the rows
 *                scored, *n_rounds.  Per round r < *n_rounds: qs[r][G] (the candidates ascending, -1 in unused places),
 *                decisions[r][G], scores[r][G][S] (unused places not written), trace[r] = {lo, hi after the round, rows}.
 * fb_attack_iter_seconds reports the host's seconds per round, as for PSO.  fb_stats counts the rows as for any batch.
 * Victim.  The air channel, the input-transform chain, the codec, dither and feature compression act as in fb_attack_pso,
 * keyed by the call's (seed, stream) with epoch = the round and utterance row = the candidate's index in the round.
 * Refusals.  FB_E_ARG: anything outside the ranges above, a task other than the engine's, a label that is no decision of
 * the system, wrong tables, bits_per_sample outside 2 .. 16, audio shorter than one frame.  FB_E_STATE: no system loaded, or
 * fb_set_eot(r > 1) or companions in force while fb_set_query_eot is off (the default; "voted decisions" below): set 1 /
 * clear them.  The engine's own systems; the _foreign twin (the "foreign victims"
 * section) runs the same search on a foreign model.
 * Deviations from Kenansville / SpeakerGuard's version: theirs transforms with a floating-point FFT (or SSA) and bisects one
 * candidate per query; here the arithmetic is the integer contract above and a round scores G candidates. */
typedef struct { int window; int grid; int q_max; int max_rounds; } fb_kv_params;
int fb_attack_kenansville(fb_engine *e, const fb_nes_params *p, const fb_kv_params *k, const int32_t *tables /*[4][W]*/,
                          const double *audio, int64_t N, int16_t *adv_i16, int *success, int *factor, int *n_queries,
                          int *n_rounds, int *qs /*[max_rounds][G]*/, int *decisions /*[max_rounds][G]*/,
                          double *scores /*[max_rounds][G][S]*/, int *trace /*[max_rounds][3]*/);

/* ---- decision-only attack II: HopSkipJump (Chen, Jordan, Wainwright 2020), the decision-only attack that targets ----------
 * fb_attack_kenansville only removes spectral content: it makes an enrolled speaker unrecognised.  fb_attack_hsj goes the other
 * way from decisions alone: it starts from `init`, any audio of N samples that the system ALREADY decides as wanted (the
 * target speaker's own voice, say), and walks along the decision boundary towards `audio`, so that an impostor is accepted (SV)
 * or taken for a chosen speaker (OSI, CSI).  Every batch -- a round of a boundary search, an iteration's probes, its step
 * sizes -- is written as int16 rows into the batch the front end scores and scored by the path that scores an NES batch; the
 * host reads scores[rows][S] and tv[rows] once per batch and forms the decisions by the rule of the section above.
 * Read from fb_nes_params: task, attack_type, max_iter, threshold, target, true_label, seed, stream and bits_per_sample; the
 * labels are decision values, as in fb_attack_kenansville.  Nothing else of it is read or validated.
 * Arithmetic.  Everything below is float64, round to nearest, one rounding per written operation, no fused multiply-add;
 * clip(s, l, h) = min(max(s, l), h); the int16 cast is that of every NES row.  a = `audio` as given, i the sample index,
 * Q = 2^20, G = grid.  A scored row d is "adversarial" iff d == target (targeted) or d != true_label and d != -2 (untargeted);
 * -2 (no voiced frames) is no decision, never adversarial and never an error.
 *   ssq(v)     the sum of squares in a fixed order.  Samples in chunks of 1024; thread t = 0 .. 255 of chunk c owns samples
 *              1024 c + 4 t .. + 3 (zero beyond N):  s_t = ((v0^2 + v1^2) + v2^2) + v3^2, every square and every add rounded;
 *              then for stride = 128, 64, .., 1:  s_t = s_t + s_{t + stride} for t < stride;  P_c = s_0;
 *              ssq = ((0 + P_0) + P_1) + .. in ascending c.
 *   line(y, q) for q = 0 .. Q:  a + (q 2^-20) (y - a) -- the difference, the exact scale, the product, the sum.  The scored
 *              row is its cast.  line(y, 0) == a bit for bit.
 *   search     the boundary search between a and an end point y: fb_attack_kenansville's bracket (lo, hi] on q with q_max = Q
 *              and rows line(y, q_j) -- round 0  q_j = floor((j + 1) Q / G), so q = Q is scored; later rounds, the update of
 *              lo and hi and the stops (hi - lo == 1, the last round, max_rounds) exactly as there.  No success in round 0: the
 *              search FAILS and the caller keeps its x.  Otherwise x := line(y, hi) in float64 and D2 := ssq(x - a) (the
 *              rounded differences), and dist = sqrt(D2) on the host.  The int16 row of hi is copied aside when it is scored.
 *   start      the search between a and `init`.  Failure: *success = -1, adv_i16 = cast(a), adv_f64 = a, *dist2 = 0,
 *              *n_iters = 0.  trace[0] = {D2, 0, 0, -1, hi, rounds, queries so far, 0} (hi = -1 and D2 = 0 on failure).
 *   iteration  t = 1 .. max_iter:
 *     1 probes     B_t = min(num_evals_max, isqrt(num_evals_init^2 t)) (integer square root, on the host);
 *                  sigma_t = max(sigma_min, (probe_scale dist) / sqrt((double)N)) (host).  Row j = 0 .. B_t - 1 is the cast of
 *                  clip(x + sigma_t (double)z_j[i], -1, 1) -- the product, the sum --, z_j[i] the NES generator's float32
 *                  normal (the "NES RNG contract") with key (seed_lo ^ 0x48534A50 ("HSJP"), seed_hi) and counter
 *                  (i >> 2, j, t, stream): the NES counter layout under a key of the probes' own.
 *     2 direction  phi_j = +1 if row j is adversarial, else -1; n+ = the number of +1.  Integer weights
 *                  w_j = phi_j B_t - (2 n+ - B_t) when 0 < n+ < B_t, else w_j = phi_j.
 *                  v[i] = sum_j (double)w_j (double)z_j[i]: from 0.0, j ascending, one rounded add per j (every product is
 *                  exact).  S = ssq(v).
 *     3 step       xi_t = dist / sqrt((double)t) (host).  nrm = sqrt(S) (correctly rounded);
 *                  c_m = S > 0 ? (xi_t 2^-m) / nrm : 0;  y_m = clip(x + c_m v, -1, 1), m = 0 .. G - 1: G rows in one batch.
 *                  The smallest adversarial m is taken.  None: the iteration STALLS -- x, D2 and the returned row stay, m = -1.
 *                  Otherwise y := y_m in float64 and the search between a and y follows; a failed search is a stall as well
 *                  (line(y, Q) need not be y bit for bit).
 *     4 trace      trace[t] = {D2 after, B_t, n+, m, hi (-1: stall), the search's rounds (0: none), queries so far, sigma_t}.
 *   stops      max_iter; or max_queries > 0 and the NEXT batch would take the rows scored beyond it -- checked before every
 *              batch except round 0 of the start search.  A search stopped so after its round 0 ends there, like at
 *              max_rounds, and its iteration counts; an iteration stopped before its search has scored a round is dropped: it
 *              leaves no trace row and x stays.  Nothing is scored after a stop.
 *   result     *success = 1; adv_i16 = the row of hi of the last successful search -- ALWAYS a row that was scored and decided
 *              adversarial --; adv_f64 = x (may be NULL); *dist2 = D2; *n_iters = the last t with a trace row; *n_queries = the
 *              rows scored.  decisions[] holds every scored row's decision in scoring order; decisions_cap entries must hold
 *              fb_hsj_max_rows(max_iter, k) of them (FB_E_ARG before anything runs otherwise).  x_trace (may be NULL)
 *              [max_iter + 1][N]: x after the start (row 0) and after every iteration with a trace row.
 * Victim.  The air channel, the input-transform chain, the codec, dither and feature compression act as in
 * fb_attack_kenansville, keyed by the call's (seed, stream) with epoch = the running count of scoring batches in this call and
 * utterance row = the row's index in its batch: an attack on a randomised victim is a function of (seed, stream).
 * fb_attack_iter_seconds reports the host's seconds per iteration (entry 0: the start search).  fb_stats counts the rows as
 * for any batch; nes_iters is not advanced.
 * Parameters.  grid 1 .. 64; max_rounds 1 .. 32; 1 <= num_evals_init <= num_evals_max <= 1024; max_queries >= 0 (0: no cap);
 * sigma_min finite and > 0; probe_scale finite and >= 0.  Defaults of the Python layer: 15, 8, 32, 256, 0, 2^-15 (one int16
 * step), 0.05.
 * Refusals.  FB_E_ARG: anything outside those ranges, max_iter < 0, a null `init`, bits_per_sample outside 2 .. 16, audio
 * shorter than one frame, a task other than the engine's, a label that is no decision of the system, a decision log that is
 * too small.  FB_E_STATE: no system loaded, or fb_set_eot(r > 1) or companions in force while fb_set_query_eot is off (the
 * default; "voted decisions" below): set 1 / clear them.  The engine's own systems; the _foreign twin (the "foreign victims"
 * section) runs the same search on a foreign model.
 * Deviations from the paper: the L2 variant only; grid rounds of G rows instead of one-query bisection and one-query step
 * halving; Gaussian probes that are not normalised to the sphere; a probe radius with a floor of sigma_min, because the
 * paper's delta = dist / d lies far below one int16 step for audio and the cast would erase it; keyed draws; a stall instead
 * of unbounded halving. */
typedef struct { int grid; int max_rounds; int num_evals_init; int num_evals_max; int max_queries; double sigma_min;
                 double probe_scale; } fb_hsj_params;
long long fb_hsj_max_rows(int max_iter, const fb_hsj_params *k);   /* -1: parameters out of range */
int fb_attack_hsj(fb_engine *e, const fb_nes_params *p, const fb_hsj_params *k, const double *audio, const double *init,
                  int64_t N, int16_t *adv_i16, double *adv_f64 /*nullable*/, int *success, double *dist2, int *n_iters,
                  int *n_queries, double *trace /*[max_iter + 1][8]*/, int *decisions /*[decisions_cap]*/,
                  long long decisions_cap, double *x_trace /*nullable [max_iter + 1][N]*/);

/* ---- voted decisions: the particle-swarm and the two decision-only attacks on a randomised victim, and on companions ---------
 * Against a randomised victim (noise stages, dither, the air channel, feature compression) one query per candidate is a coin
 * flip: fb_attack_kenansville's bracket and fb_attack_hsj's boundary search assume that a candidate HAS a decision.  With this
 * switch on the three attacks of the sections above accept fb_set_eot(r), companions (fb_set_companions) and both together:
 * every candidate row is scored r' = K * eot <= 32 times in ONE replicating launch chain -- fb_attack's under EOT --, and
 * one launch (k_vote) turns the r' replica rows of a candidate into one vote.
 * fb_set_query_eot(e, quorum): FB_QUORUM_OFF = 0 (the default) -- the three attacks refuse EOT and companions with FB_E_STATE
 * exactly as their sections say; FB_QUORUM_MAJORITY = -1 -- a row needs r' / 2 + 1 (integer division) adversarial replicas;
 * 1 .. 32 -- it needs that many.  Anything else is FB_E_ARG and keeps the previous value.  An explicit quorum larger than
 * the r' in force is FB_E_ARG at the attack call, before anything runs (fb_attack_pso reads no quorum, and refuses it all
 * the same).  Switched on with r' = 1 nothing changes: no launch is added, every output is bit-identical to the switch-off
 * run, decisions[] keeps holding decisions.  fb_estimate_threshold keeps returning FB_E_STATE under EOT or companions, and
 * foreign models stay out.  Everything below is for r' > 1.
 * Replication.  Exactly fb_set_companions' rule.  The attack's `rows` candidate rows stand un-replicated in the batch buffer
 * (q_b: particle b, candidate b of the round, row b of a search round / of the probes / of the step sizes).  a_0 is the int16
 * cast of the call's `audio`, made once per call (for fb_attack_kenansville that is its x).  Utterance u of row b is q_b for
 * u = 0 and clip(a_u + q_b - a_0, -32768, 32767) for a companion; replica rho = u * eot + j is row b * r' + rho of what the
 * front end scores; the noise stages, dither, feature compression and the air channel draw with `replica` = rho, utterance
 * row = b (the row's index in its un-replicated batch), and epoch = the attack's own: the PSO iteration, the Kenansville
 * round, fb_attack_hsj's running count of scoring batches.  rows * r' > 65535 is FB_E_LIMIT before anything is scored: for
 * fb_attack_hsj max(grid, num_evals_max) * r' is checked up front.  A call whose N differs from the companions' is FB_E_ARG.
 * fb_attack_pso.  l_p and particle p's score row are fb_set_eot's means over its r' replicas: loss_fn and the system scores
 * per replica row, then (v_0 + v_1 + ... + v_{r' - 1}) / r' in float64, rho ascending, one rounding per addition and one for
 * the division (k_loss_eot, as in fb_attack).  FB_E_NO_VOICED if ANY replica of any particle has no voiced frames.  Everything
 * behind step 1 is unchanged and sees the P averaged rows; the ball, the returned audio and adv_f64 are utterance 0's, and
 * the perturbation to carry over to the companions is adv_i16 - a_0.  As in fb_attack THE STOP TEST READS A MEAN.
 * fb_attack_kenansville and fb_attack_hsj.  Per replica row the system scores are formed exactly as without replicas (the
 * device function of k_loss), then the decision d by the rule of the "decision-only attack" section (SV s >= threshold;
 * OSI / CSI the first maximum; OSI maximum < threshold -> -1; no voiced frames -> -2), then the replica's flag: adversarial
 * iff d == target (targeted), or d != true_label and d != -2 (untargeted).  A replica without voiced frames is a failed
 * replica, never an error.
 *   vote       of a candidate row: the number of its adversarial replicas, 0 .. r'.
 *   adversarial a row is adversarial ("succeeds") iff vote >= quorum.  Wherever the two sections say that a row succeeds, is
 *              adversarial or WAS scored and decided adversarial, read "voted adversarial": the bracket's update, n+ and the
 *              weights w_j, the smallest adversarial step size m, the row of hi that is returned.
 *   logs       decisions[] holds the VOTES, in the places the decisions had (one entry per candidate row; fb_hsj_max_rows is
 *              unchanged).  fb_attack_kenansville's scores[r][G][S] holds the fb_set_eot mean of the replicas' score rows.
 *   queries    *n_queries, max_queries, fb_attack_kenansville's trace[.][2] and fb_attack_hsj's trace[.][6] count VICTIM
 *              queries: candidate rows * r'.  max_queries stops before a batch whose rows * r' would pass it.
 *   the rest   of both searches is unchanged: candidates, bracket, probes, direction, step sizes, stalls, stops; the float64
 *              state and the returned row are utterance 0's.
 * The launch.  k_vote reads the finalised raw scores and tv of the rows * r' replica rows and writes ONE contiguous block
 * {votes[rows] int32, nodec[rows] int32 (replicas with -2), mean[rows][S] float64}; the host copies that block and nothing
 * per replica.  It stands where k_loss stood: the replicated chain gains no launch beyond fb_attack's under EOT.  One wave
 * per candidate row counts with two ballots and adds in a fixed order: no atomics, bit-reproducible. */
enum { FB_QUORUM_OFF = 0, FB_QUORUM_MAJORITY = -1 };
int fb_set_query_eot(fb_engine *e, int quorum);   /* 0 off (default) | -1 majority | 1 .. 32 */

/* ---- white-box gradients: backpropagation through the GMM-UBM victim ------------------------------------------------------
 * fb_get_grad estimates the gradient of the loss from scores (NES); the victim lives in the engine, so the gradient itself
 * can be computed.  fb_get_grad_wb returns it, fb_attack_wb runs FakeBob.attack's loop on it.  Scope of this version: GMM-UBM
 * systems (OSI, CSI, SV) on an UNDEFENDED victim; everything else is refused, not ignored ("Refusals").  With
 * fb_set_wb_bpda(e, 1) the same calls differentiate THROUGH an input-transform chain, a codec and the replicas of fb_set_eot
 * ("Defended victims: BPDA and EOT", below).  The air channel's transpose and the i-vector back end are out of this version.
 * The function that is differentiated.  Input: float audio a in [-1, 1].  The forward is the engine's ordinary one, as
 * configured: the int16 cast with 2^(bits_per_sample - 1); MFCC, VAD, add-deltas, sliding CMVN, the voiced rows; per-model mean
 * frame log-likelihood; fb_system_scores; the reference's loss_fn (FAKEBOB.py:248-299).  adver_loss and score0 are exactly
 * what fb_get_grad returns for a batch of that one row (samples_per_draw = 0): the same launches.  The gradient is that of the
 * real-valued function at the point the forward reached:
 *  - the cast, the float32 storage points and the compress_feats, text_scores and mfcc_f32 roundings are identities
 *    (straight-through);
 *  - the voiced mask is the forward's own, recomputed from the forward's MFCC matrix by the arithmetic of its VAD and checked
 *    against its count (FB_E_HIP if they ever differ), and held constant;
 *  - a floor that is active contributes zero: log(max(E, FLT_EPSILON)) on a mel bin or a frame energy, and energy_floor;
 *  - the loss's maxima take the subgradient of the index the forward's maximum selected: the first maximum, as make_decisions
 *    does; np.maximum(other, threshold) passes the speaker only when it is strictly greater.
 * grad[n] = d loss / d a[n], in the audio units of fb_get_grad's estimate: 2^(bits_per_sample - 1) times the derivative with
 * respect to the int16 sample.  The per-model weights w[M] = d loss / d raw[m] follow from the branch of loss_fn -- OSI / SV:
 * -+1 on at most two speakers, the opposite on the UBM; CSI: +-1 / z_std -- and are formed on the device from the scores it has.
 * The arithmetic behind them: for every voiced row x_t, gamma the posteriors of model m,
 *     g_t = (1 / Tv) sum_m w_m sum_c gamma_mtc (means_invvars_mc - inv_vars_mc * x_t)           (models with w_m = 0 skipped)
 * with float32 matrix-core products and a float32 online soft-max over component tiles, the per-model rows combined in
 * float64, models ascending; then the transposes of the front end in float64 -- scatter to the voiced frames, sliding CMVN
 * (both clamped ends, T > cmn_window), deltas (clamped time index), MFCC per frame (C0 from the raw log-energy when use_energy;
 * lifter, DCT, 1 / mel energy, mel weights; the frame's FFT recomputed from the int16 row, one inverse transform of dP_k F_k;
 * window, pre-emphasis, DC removal) -- and an overlap-add through the forward's frame index rule, repeated reflection
 * included.  No floating-point atomics: a sample sums its frames' contributions in ascending frame order, and the same call
 * gives the same bits on a fresh engine.  Every front-end shape fb_set_frontend takes is taken.
 * fb_get_grad_wb(e, p, audio, N, adver_loss, grad[N] (nullable), score0[S]).
 * fb_attack_wb: FakeBob.attack's loop with that gradient in place of get_grad.  Unchanged from the reference: the early stop
 * adver_loss < 0 before the step, the plateau rule, the trace rows {distance, adver_loss, lr_after, score0[S]}, the
 * iter < max_iter - 1 flag, the final cast, the step (FAKEBOB.py:193-203: grad_m = momentum grad_m + (1 - momentum) g;
 * adver -= lr sign(grad_m); the clips to the epsilon ball and to [-1, 1], float64 as in fb_attack).  One row is scored per
 * iteration; the plateau window holds adver_loss (there is no noisy mean); samples_per_draw and sigma are not read; seed
 * and stream are not read on an undefended victim and ARE read once a random stage is set (below).  momentum = 0 is plain PGD with the margin loss (SpeakerGuard's CW-inf / PGD), max_iter = 1 the single-step case;
 * there is no random start, so a result is reproducible.  The loop control runs on the device and the host looks at it once
 * per FB_ATTACK_BATCH iterations (default 4), as in fb_attack; fb_attack_iter_seconds and fb_stats work as for fb_attack.
 * Refusals, each with a message naming the cause.  FB_E_STATE: no model, an i-vector system is loaded, fb_set_eot(r > 1) is
 * in force, companions are set, an input-transform chain, an air channel or a codec is set, feature compression is on,
 * dither > 0.  FB_E_ARG: audio shorter than one frame, max_iter < 1 (fb_attack_wb), the task, target, true-label and
 * bits_per_sample rules of fb_attack_pso.  FB_E_NO_VOICED: a row without voiced frames, as in fb_attack.
 *
 * Defended victims: BPDA and EOT (fb_set_wb_bpda).  A defence judged only by score-based attacks is the textbook case of
 * obfuscated gradients; the adaptive white-box attack is PGD with BPDA (a differentiable surrogate in the backward pass)
 * through the non-differentiable stages and an expectation over the random ones.  It is an approximation the attacker
 * chooses, hence a switch: fb_set_wb_bpda(e, on), on = 0 or 1 (anything else: FB_E_ARG, the setting stays), 0 at engine
 * creation.  With 0 no call queues another launch or returns another value than before the switch existed, and every refusal
 * above stands.  With 1, fb_get_grad_wb, fb_get_grad_wb_iter and fb_attack_wb accept an input-transform chain (all five stage
 * kinds), a codec, fb_set_eot(r), 1 <= r <= 32, and any combination; with nothing of these set they queue exactly the
 * launches of the undefended call.  Still FB_E_STATE with the switch on, the cause named: an i-vector system, companions,
 * feature compression, dither > 0 (both: unless fb_set_wb_frontend, "Feature compression and dither", below) -- and an
 * AIR CHANNEL: refused unless fb_set_wb_air ("The over-the-air channel", below).
 * fb_get_grad_wb_iter is fb_get_grad_wb with the epoch of the random draws given: `iter` (>= 0) means what fb_get_grad's
 * iter means in the noise RNG contract; fb_get_grad_wb is iter = 0; fb_attack_wb draws with its loop index, as fb_attack
 * does.  p->seed and p->stream key the draws.
 * Forward.  The engine's ordinary forward for a batch of one row under the defences set: cast, chain, codec, front end, GMM,
 * fb_system_scores and loss_fn per replica, then the EOT mean in fb_set_eot's float64 order.  adver_loss and score0 are bit
 * for bit what fb_get_grad returns at samples_per_draw = 0 with the same iter, seed, stream and settings -- the same launches
 * -- so fb_attack_wb's stop test reads the mean over the replicas, as fb_attack's does.
 * Backward.  The gradient of a real-valued surrogate at the point the forward reached, replica by replica:
 *     grad = sum_j grad_j, j ascending, float64, grad_j computed with the weights w_j[M] / r of replica j's OWN scores (its
 *     first-maximum index may differ from another replica's): k_wb_gmm_bwd on replica j's voiced rows, the front-end
 *     backward on replica j's TRANSFORMED int16 row and MFCC matrix, then the transposes of the defence stages.
 * Every stage's VALUES are the forward's own (recomputed: the forward keeps no intermediates); its derivative is
 *   rounding (rint, floor_div)   the identity
 *   saturation                   a sample whose value after rounding, before the clip, lies outside [-32768, 32767] passes zero,
 *                                in any stage -- the rule "an active floor contributes zero"
 *   FB_TF_QUANT                  the identity (straight-through), except under saturation
 *   FB_TF_MEDIAN                 the exact subgradient: the cotangent of y[i] goes to the ONE window position the median
 *                                selected -- the 2r + 1 window entries, zero padding outside [0, n) included, ordered by
 *                                (value, position), both ascending; the entry of rank r.  A selected padding position absorbs it.
 *   FB_TF_FIR                    the transpose: dx[m] = sum_j taps[j] * dy[m - c + j] over the j whose index lies in [0, n),
 *                                j ascending, float64 (one rounding per product and per sum), dy zeroed where saturated
 *   FB_TF_DECIMATE               passes dy[i] where i mod q = 0, zero elsewhere
 *   FB_TF_NOISE                  the identity, except under saturation; the scale s of an SNR stage is held constant, as the
 *                                voiced mask is; the normals are redrawn by the forward's rule for (stage, replica j)
 *   codec (ulaw, alaw, adpcm)    the identity: BPDA in the strict sense.  A segment-slope derivative for G.711 is not in
 *                                this version.
 * No floating-point atomics and a fixed order in every sum: the same call on a fresh engine gives the same bits.  The
 * 2^(bits_per_sample - 1) scale and the units of grad are unchanged.
 * The over-the-air channel (fb_set_wb_air).  The gradient of the loss through the drawn room -- with fb_set_eot(r) the EOT-over-
 * rooms gradient of the robust over-the-air attack -- behind a third switch: fb_set_wb_air(e, on), on = 0 or 1 (anything else:
 * FB_E_ARG, the setting stays), 0 at engine creation, kept across fb_load_*.  With 0 every call, launch, value and refusal
 * message is what it was before the switch existed: an air channel is refused whatever the other two switches say.  With 1,
 * fb_get_grad_wb, fb_get_grad_wb_iter and fb_attack_wb accept an air channel: a GMM-UBM system in any combination the BPDA
 * switch allows -- the channel alone needs no other switch; a chain, a codec and fb_set_eot(r > 1) still need
 * fb_set_wb_bpda(e, 1) --, an i-vector system under fb_set_wb_ivector(e, 1), at r = 1 only, as without a channel.  Companions,
 * feature compression and dither (unless fb_set_wb_frontend) stay refused, by name; with no channel set the calls queue exactly the launches they
 * queued before.
 * Forward.  The engine's own, unchanged: cast, air channel, chain, codec, front end.  adver_loss and score0 are bit for bit
 * fb_get_grad's at samples_per_draw = 0 with the same iter, seed, stream and settings.
 * Backward.  Replica j of the one row runs the front-end backward, (codec: the identity), (the chain transposed: on the row the
 * chain read, the channel's output row j, with that row's SNR power and the noise counters of (utterance row 0, replica j)),
 * then the channel transposed.  The taps t_j[0 .. L) are the forward's own draw for (epoch, row 0, replica j) and are
 * constants.  Rounding and the shift are the identity.  An output whose value (y[i] + 8192) >> 14, before the clip, lies
 * outside [-32768, 32767] passes zero -- the saturation rule above, decided on the exact integer y (a sample AT a rail that
 * was not clipped passes).  With g_j the cotangent on the channel's output, saturated positions zeroed,
 *     dx_j[m] = 2^-14 * sum_{k = 0 .. min(L - 1, n - 1 - m)} t_j[k] * g_j[m + k]
 * in float64 on the matrix cores (k_air_conv_t); the order of the sum over k is the kernel's: fixed, not specified.  Then
 *     grad = sum_j dx_j, j ascending, float64.
 * No floating-point atomics: the same call on a fresh engine gives the same bits.
 * Feature compression and dither (fb_set_wb_frontend).  Both stages are differentiated by the rule of gselect, the min-post set
 * and the voiced mask -- the forward's hard decisions are held constant; no surrogate is invented -- behind a fourth switch:
 * fb_set_wb_frontend(e, on), on = 0 or 1 (anything else: FB_E_ARG, the setting stays), 0 at engine creation, kept across
 * fb_load_*.  With 0 every call, launch, value and refusal message is what it was before the switch existed: feature
 * compression and dither > 0 are refused whatever the other three switches say.  With 1, fb_get_grad_wb, fb_get_grad_wb_iter
 * and fb_attack_wb accept feature compression and dither > 0, alone or together; neither needs fb_set_wb_bpda at r = 1 (the
 * gradient at a fixed draw is exact).  A chain, a codec and fb_set_eot(r > 1) still need fb_set_wb_bpda, an air channel
 * fb_set_wb_air, an i-vector system fb_set_wb_ivector (r = 1 only); companions stay refused; with neither stage set the calls
 * queue exactly the launches they queued before.
 * Forward.  The engine's own, unchanged.  adver_loss and score0 are bit for bit fb_get_grad's at samples_per_draw = 0 with the
 * same iter, seed, stream and settings.
 * Feature compression: the final assignment is a constant.  For utterance row u the forward keeps the label of every voiced
 * frame, the member count n_j of every centre and k, taken where the centres were last written: after the last update, or at
 * the early break, where the assignment equals the one the last update used.  A centre with n_j > 0 is the mean of its members;
 * its float32 storage is the identity.  A centre with n_j = 0 kept an earlier value: a constant, its cotangent is dropped (the
 * rule "an active floor contributes zero").  The back end -- GMM or i-vector -- is differentiated on the k centre rows as it is
 * on the voiced rows without the stage; the mean over scored rows is over k, not over the VAD's count.  Then (k_wb_feco_t)
 *     xbar[t][d] = cbar[label[t]][d] / (double) n_label[t]
 * one correctly rounded float64 division per element, no atomics, nothing summed; from xbar the front-end backward is the one
 * above (its voiced mask is still recomputed from the forward's MFCC matrix and checked against the VAD's count).
 * Dither: the draws are the forward's, and constants.  The per-frame recomputation of the front-end backward reads
 * (double) x + amp * (double) z(u, t, s) where it reads (double) x without dither, z from the dither RNG contract at the call's
 * (seed, stream, epoch = iter) with utterance index = the replicated row j -- what k_mfcc and k_mfcc_f32 add; both form the
 * dithered sample in float64.  The noise is additive: the derivative with respect to the sample is unchanged.
 * EOT: replica j uses its own labels and its own dither; grad = sum_j grad_j, j ascending.  The same call on a fresh engine
 * gives the same bits.
 * Universal perturbations (fb_set_wb_universal).  The white-box twin of fb_set_companions: the exact gradient of the loss
 * averaged over the K = K1 + 1 utterances one delta is scored on, behind a fifth switch: fb_set_wb_universal(e, on), on = 0 or 1
 * (anything else: FB_E_ARG, the setting stays), 0 at engine creation, kept across fb_load_*.  With 0 every call, launch, value
 * and refusal message is what it was before the switch existed: companions are refused whatever the other four switches say.
 * With 1 and no companions set (K = 1) the calls queue exactly the launches they queued before.  With 1 and companions set,
 * fb_get_grad_wb, fb_get_grad_wb_iter, fb_get_grad_wb_from and fb_attack_wb accept them.
 * Forward.  The engine's own, unchanged: it scores R = K * eot replicas of the one row, replica rho = u * eot + j being the rho
 * of the Composition, Row order and Averaging paragraphs.  adver_loss and score0 are bit for bit fb_get_grad's at
 * samples_per_draw = 0 with the same iter, seed, stream, settings and a_0.
 * Backward.  The gradient of the AVERAGED loss: replica rho's weights are w_rho[M] / R, from its own scores (k_wb_ctl_rep with R
 * where it takes r).  Each replica goes through the backward above for the defences set, keyed by rho where it is keyed by j:
 * the noise and dither draws, feature compression's kept labels, counts and k, the room response and its saturation bytes; the
 * chain's transpose runs on the row the chain read -- utterance u(rho)'s composed row, or with an air channel the channel's
 * output row rho -- with that row's SNR power.  This yields g_rho[i], the cotangent on sample i of the composed row of
 * utterance u(rho) as it was handed to the air channel, the chain or the front end.
 * Composition transposed.  The saturation rule above, decided on the exact integer (a sample AT a rail that was not clipped
 * passes): m_0[i] = 1; for u >= 1, m_u[i] = 1 where v = a_u[i] + q[i] - a_0[i], in int32, lies inside [-32768, 32767], and 0
 * elsewhere (q: the int16 cast of the call's audio; a_0 is a constant).  Then (k_wb_compose_t, one launch)
 *     grad[i] = sum_rho m_{u(rho)}[i] * g_rho[i]
 * in float64, rho ascending, one rounding per addition, starting from +0.0; a masked term adds +0.0.  No atomics: the same
 * call on a fresh engine gives the same bits.  The 2^(bits_per_sample - 1) scale of the cast is applied where the front-end
 * backward applies it without companions.
 * a_0.  In fb_get_grad_wb and fb_get_grad_wb_iter a_0 is the cast of the call's own audio, so q = a_0, every composed row is
 * the companion itself and no sample clips.  fb_get_grad_wb_from(e, p, audio, original, N, iter, ...) is fb_get_grad_wb_iter
 * with a_0 given: original, float64 [N], is cast once, by the batch's cast rule, and becomes a_0; original == NULL means audio,
 * and the call is then fb_get_grad_wb_iter.  Without companions original is not read.  fb_attack_wb keeps a_0 = the audio it
 * was handed, as fb_attack does; its stop test reads the mean over the replicas and its trace rows hold the averaged scores.
 * What each setting needs, each refusal naming its cause: companions need this switch only (at eot = 1 the gradient at a fixed
 * victim is exact); a chain, a codec and fb_set_eot(r > 1) still need fb_set_wb_bpda, an air channel fb_set_wb_air, feature
 * compression and dither fb_set_wb_frontend, an i-vector system fb_set_wb_ivector.
 * i-vector systems.  With this switch on the forward keeps the contraction's matrix (quad) of ALL R rows -- R * R_iv (R_iv + 1) / 2
 * float64, about 20 MB at R = 32 for the recipe's size -- and replica rho's backward takes ITS weights (k_wb_iv_ctl_rep: k_wb_iv_ctl's
 * with R), ITS i-vector, ITS copy of quad for the adjoint solve, and ITS rows of the selection and the posteriors; the forward's
 * active list is the batch's, a superset of every replica's.  So an i-vector system then takes companions, and -- with or without
 * companions -- fb_set_eot(r > 1) under fb_set_wb_bpda, as a GMM-UBM system does; with the switch off both stay refused by the
 * messages of "The i-vector-PLDA victim" below.
 * Limits.  K * eot <= 32 (FB_E_ARG at the setters), N must equal the companions' N (FB_E_ARG), FB_E_NO_VOICED if any composed
 * row has no voiced frames -- all as in fb_get_grad.  fb_attack_pso, fb_attack_kenansville and fb_estimate_threshold still
 * refuse companions; foreign models ignore them, as before.
 *
 * The i-vector-PLDA victim (fb_set_wb_ivector).  A second switch, for the same reason as the first: fb_set_wb_ivector(e, on),
 * on = 0 or 1 (anything else: FB_E_ARG, the setting stays), 0 at engine creation, kept across fb_load_*.  With 0 every call,
 * launch, value and message is what it was before the switch existed.  With 1 a GMM-UBM system still takes the very same
 * launches, and fb_get_grad_wb, fb_get_grad_wb_iter and fb_attack_wb accept a loaded i-vector system, all three tasks and
 * both attack types.  The function that is differentiated is the engine's own forward:
 *  - the front end as above: straight-through cast, the voiced mask held constant, an active floor contributes zero;
 *  - gmm-gselect is a constant: the num_gselect components a frame selected on the diagonalised UBM are the forward's;
 *  - --min-post pruning is a constant set: the slots whose float32 posterior the forward dropped stay dropped, and on the
 *    kept set K_t the posterior is the soft-max of the full-covariance log-likelihoods
 *    ll_tk = gconst_k + (Sigma_k^-1 mu_k) . x - 1/2 x' Sigma_k^-1 x restricted to K_t (what "drop, renormalise" equals), so
 *    d gamma_tk / d ll_tj = gamma_tk (delta_kj - gamma_tj) for j, k in K_t; the rescue of a frame whose posteriors all
 *    fell below min_post (one slot set to 1) is a constant posterior;
 *  - the float32 storage points (features, ll, posteriors, the i-vector's text form) and text_scores are identities;
 *  - N_k = sum_t gamma_tk, F_k = sum_t gamma_tk x_t; lin = sum_k A_k' F_k + prior e_0 with A_k = Sigma_k^-1 M_k;
 *    quad = I + sum_k N_k U_k; w = quad^-1 lin; the i-vector is w - prior e_0;
 *  - the back end: - mean.vec; LDA, with or without the offset column; * sqrt(L) / |.|; PLDA y0 = A (c - m), then
 *    * sqrt(L / sum_i y0_i^2 / (psi_i + 1)); the closed-form LLR against each enrolled vector with n = 1; the wrappers'
 *    z-norm (every task); loss_fn with the first-maximum subgradient, as above.
 * Backward, all float64, the posteriors and the selection read from what the forward left on the device: the weights
 * w[S] = d loss / d raw[s] (k_wb_iv_ctl: the 1 / z_std inside); wbar = d (sum_s w_s LLR_s) / d ivec (k_wb_iv_backend_t: the
 * back end recomputed, then transposed); lambda = quad^-1 wbar by the forward's own k_iv_solve_ll on a copy of the matrix
 * taken before the forward factorised it; for the components of the forward's active list Fbar_k = A_k lambda and
 * Nbar_k = - lambda' U_k w (k_wb_iv_stats_t: one stream over Sigma^-1 M and the packed U; an off-diagonal packed element
 * stands for two, the diagonal for one); per voiced frame over its kept slots (k_wb_iv_post_t)
 *     gammabar_tk = Nbar_k + Fbar_k . x_t,   llbar_tk = gamma_tk (gammabar_tk - sum_j gamma_tj gammabar_tj),
 *     xbar_t = sum_k gamma_tk Fbar_k + sum_k llbar_tk (Sigma_k^-1 mu_k - Sigma_k^-1 x_t);
 * then the front-end backward above, unchanged.  adver_loss and score0 are bit for bit fb_get_grad's at samples_per_draw = 0:
 * the same scoring call.  fb_attack_wb is the same loop, trace layout and stop test.
 * Refused for an i-vector system with the switch on, FB_E_STATE, the cause named: companions (unless fb_set_wb_universal), an air channel (unless fb_set_wb_air), feature
 * compression and dither > 0 (unless fb_set_wb_frontend), and fb_set_eot(r > 1) -- the last with fb_set_wb_bpda on as well ("i-vector", "fb_set_eot": the
 * forward keeps one row's i-vector state, not r replicas' -- unless fb_set_wb_universal, "Universal perturbations" above).  An input-transform chain and a codec need fb_set_wb_bpda(e, 1), as
 * for a GMM-UBM system, and are then taken at r = 1.  FB_E_NO_VOICED and the "not positive definite" error are scoring's.
 *
 * The x-vector (TDNN) victim (fb_set_wb_xvector).  A sixth switch, for the same reason as the others: fb_set_wb_xvector(e, on),
 * on = 0 or 1 (anything else: FB_E_ARG, the setting stays), 0 at engine creation, kept across fb_load_*.  With 0 every call,
 * launch, value and message is what it was before the switch existed: an x-vector system is refused ("not in this version").
 * With 1 the other two kinds still take the very same launches, and fb_get_grad_wb, fb_get_grad_wb_iter, fb_get_grad_wb_from,
 * fb_attack_wb, fb_attack_cw2 and fb_attack_psy accept a loaded x-vector system, all three tasks and both attack types.  The
 * function that is differentiated is the engine's own forward ("x-vector (TDNN) system" below); its hard decisions are
 * constants:
 *  - the front end as above: straight-through cast, the voiced mask held constant, an active floor contributes zero;
 *  - frame layer: the derivative of max(z, 0) is 1 where the forward's own float32 z = W . splice + bias was > 0, else 0.  The
 *    decision is the one the forward took -- k_xv_affine writes a byte per (row, channel) when the scoring call asks for it --,
 *    not one re-derived from the output: y == bn_offset does not imply z <= 0 once bn_scale * t is absorbed by the offset.  A
 *    replicated edge row (clamp(t + ctx[j], 0, T - 1)) receives the cotangents of every place that read it;
 *  - pooling: the mean passes mbar / T; the standard deviation passes sbar (h - mean) / (T std) where E[h^2] - mean^2 > 1e-10
 *    and nothing where the floor is active -- every channel of a one-row utterance;
 *  - embedding to back end: the rounding to float32 is straight-through (k_wb_iv_backend_t treats it so); the back end, the
 *    z-norm and loss_fn as for the i-vector victim.
 * Backward: the weights (k_wb_iv_ctl; k_wb_iv_ctl_rep per replica) and ebar = d (sum_s w_s LLR_s) / d embedding
 * (k_wb_iv_backend_t) per replica, float64; then ONE pass over all voiced rows of the batch, as the forward runs:
 * sbar = seg_W' ebar (k_wb_xv_segment_t, float64); the pooling rule (k_wb_xv_pool_t, float64, rounded once to the float32
 * cotangent on the last layer's output); per frame layer, last to first, zbar = ybar * bn_scale * mask (k_wb_xv_act_t, one
 * rounding per multiplication, and max |zbar| of every row), G[t][n] = sum_c zbar[t][c] W[c][n] over the layer's n_ctx * din
 * columns (k_wb_xv_affine_t) and xbar[t'][d] = sum_j sum_{t : clamp(t + ctx[j], 0, T - 1) = t'} G[t][j din + d], j ascending
 * and then t ascending, summed in float64 and rounded once (k_wb_xv_unsplice; layer 0 hands its float64 sums to the front-end
 * backward unrounded).  Arithmetic of the transposed affine: the forward's -- the cotangent row as two f16 terms under a power
 * of two of its own row, W' as two f16 terms under one power of two per layer chosen at load time, three products per K step on
 * the matrix cores, float32 accumulation in an order that depends on the layer's shape alone.  Cotangents between frame
 * layers are float32; there are no floating-point atomics.  Hence (a) a run repeats bit for bit, and (b) the cotangent on an
 * utterance's feature rows does not depend on the batch the utterance sits in.  adver_loss and score0 are bit for bit
 * fb_get_grad's at samples_per_draw = 0: the same scoring call.
 * With fb_set_wb_bpda(e, 1) as well an x-vector system is differentiated through an input-transform chain, through a codec
 * and under fb_set_eot(r): the r replicas' embeddings each get their cotangent, the one TDNN backward runs over all r * T rows,
 * and the front-end backward and the chain's transpose follow per replica, summed ascending.  Refused for an x-vector system,
 * FB_E_STATE, the cause named, whatever their own switches say: an air channel, dither > 0, companions and a play offset;
 * fb_set_eot(r > 1), a chain and a codec without fb_set_wb_bpda as for a GMM-UBM system.  Feature compression cannot be on with
 * this system at all. */
int fb_set_wb_bpda(fb_engine *e, int on);
int fb_set_wb_ivector(fb_engine *e, int on);
int fb_set_wb_xvector(fb_engine *e, int on);
int fb_set_wb_air(fb_engine *e, int on);
int fb_set_wb_frontend(fb_engine *e, int on);
int fb_set_wb_universal(fb_engine *e, int on);
int fb_get_grad_wb_from(fb_engine *e, const fb_nes_params *p, const double *audio, const double *original /*[N], nullable*/,
                        int64_t N, int iter, double *adver_loss, double *grad /*[N], nullable*/, double *score0 /*[S]*/);
int fb_get_grad_wb_iter(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, int iter, double *adver_loss,
                        double *grad /*[N], nullable*/, double *score0 /*[S]*/);
int fb_get_grad_wb(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, double *adver_loss,
                   double *grad /*[N], nullable*/, double *score0 /*[S]*/);
int fb_attack_wb(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, int16_t *adv_i16, double *adver_f64,
                 double *trace, int *n_trace, int *success_flag);

/* ---- CW2: the L2 white-box attack (Carlini-Wagner in tanh space, Adam, a binary search over the constant c) -----------------
 * fb_attack_wb spends a fixed epsilon budget; fb_attack_cw2 MINIMISES the distortion: it answers "how small a perturbation
 * breaks this system".  The gradient is fb_get_grad_wb_iter's (the same launches), the loop control runs on the device and the
 * host looks once per FB_ATTACK_BATCH iterations and between search steps; the result does not depend on that variable.
 * Read of fb_nes_params: task, attack_type, target, true_label, threshold, adver_thresh (CW's confidence kappa: it sits
 * inside loss_fn), max_iter (iterations per search step), bits_per_sample; with a random stage set also seed and stream.  Not
 * read: epsilon, the learning rates, momentum, the plateau knobs.  fb_cw2_params: initial_const (SpeakerGuard: 1e-3),
 * search_steps (9), lr (1e-2), beta1 (0.9), beta2 (0.999), adam_eps (1e-8) -- torch.optim.Adam's --, abort_every (1000; 0: never).
 * a0[N]: the float audio in [-1, 1].  w0 = atanh(0.999999 a0) is computed on the host in float64 (libm) and uploaded.  All
 * device arithmetic is float64 with one rounding per operation, nothing contracted; products and quotients associate from the
 * left as written:
 *   c = initial_const; lo = 0; hi = 1e10; gbest_l2 = +inf; gbest_row = cast(a0); gbest_x = a0
 *   for s in 0 .. search_steps-1:
 *       mod = m1 = m2 = 0;  x = tanh(w0)                     (the first iterate is tanh(w0), not a0)
 *       p1 = p2 = 1;  prev = +inf;  found = False
 *       for t in 0 .. max_iter-1:
 *           epoch = s*max_iter + t                           (the `iter` of fb_get_grad_wb_iter: the draws of random stages)
 *           g, adver_loss, score0 = fb_get_grad_wb_iter at x (the forward casts x to int16)
 *           l2 = sum_n (x[n]-a0[n])^2                        (the fixed order below)
 *           gate = 1 if adver_loss > 0 else 0                (CW's max(f, 0): the margin stops pulling once past kappa)
 *           L = (c*gate)*adver_loss + l2
 *           trace row = {l2, adver_loss, c, score0[S]}       (rows are consecutive: an aborted step leaves no gap)
 *           if adver_loss < 0 and l2 < gbest_l2: gbest_l2 = l2; gbest_row = the int16 row the forward scored; gbest_x = x
 *           if adver_loss < 0: found = True
 *           if abort_every > 0 and t % abort_every == 0:
 *               if L > 0.9999*prev: break                    (the row is written, no step is taken)
 *               prev = L
 *           p1 *= beta1; p2 *= beta2                         (on the host, by repeated multiplication)
 *           G = ((c*gate)*g + 2*(x-a0)) * (1 - x*x)
 *           m1 = beta1*m1 + (1-beta1)*G;  m2 = beta2*m2 + ((1-beta2)*G)*G
 *           mod = mod - ((lr/(1-p1)) * m1) / (sqrt(m2)/sqrt(1-p2) + adam_eps)
 *           x = tanh(w0 + mod)
 *       if found: hi = min(hi, c); c = (lo+hi)/2
 *       else:     lo = max(lo, c); c = (lo+hi)/2 if hi < 1e9 else c*10
 *   adv_i16 = gbest_row, adver_f64 = gbest_x, success_flag = +1 if gbest_l2 < inf else -1, best_l2 = gbest_l2, final_const = c
 * The L2 sum: blocks of 256 consecutive samples, terms past N being +0.0; within a block d[i] += d[i + h] for all i < h, for
 * h = 128, 64, 32, 16, 8, 4, 2, 1 in this order, the block's partial being d[0]; the partials are added in ascending block order
 * from +0.0.  No floating-point atomics.  Division and square root are correctly rounded, so m1, m2 and mod are bit-exact
 * contracts; tanh is the device library's and is not: it is the one place where a host restatement agrees to a tolerance.
 * "Success" is FAKEBOB's own test adver_loss < 0 -- the loss of the int16 row actually scored, under fb_set_eot the mean over
 * the replicas.  SpeakerGuard's CW2 reads a decision instead; with kappa = 0 the two coincide except on ties.  Unlike
 * fb_attack_wb the loop does not stop at the first success: it keeps the smallest successful iterate.
 * trace [search_steps*max_iter][3 + S] (nullable), *n_trace rows written; rows_per_step[search_steps].  fb_attack_iter_seconds
 * and fb_stats (nes_iters: one per row) work as for fb_attack_wb.
 * Victims: an undefended GMM-UBM system; an i-vector system under fb_set_wb_ivector; an input-transform chain, a codec and
 * fb_set_eot(r) under fb_set_wb_bpda, exactly as fb_attack_wb accepts them.  Refused by name, FB_E_STATE, whatever the
 * switches say, in this version: companions, an air channel, feature compression, dither > 0.  FB_E_ARG: null arguments,
 * search_steps outside 1 .. 32, a non-finite or non-positive initial_const, lr or adam_eps, a beta outside [0, 1),
 * abort_every < 0, max_iter < 1, search_steps * max_iter above 2^30, and the task, target, true-label and bits_per_sample
 * rules of fb_attack_wb.  A refusal leaves the engine as it was. */
typedef struct { double initial_const; int search_steps; double lr, beta1, beta2, adam_eps; int abort_every; } fb_cw2_params;
int fb_attack_cw2(fb_engine *e, const fb_nes_params *p, const fb_cw2_params *q, const double *audio, int64_t N, int16_t *adv_i16,
                  double *adver_f64 /*[N], nullable*/, double *trace /*[search_steps*max_iter][3+S], nullable*/, int *n_trace,
                  int *rows_per_step /*[search_steps]*/, int *success_flag, double *best_l2, double *final_const);

/* ---- masking: the CW attack that hides under the voice (Qin et al., "Imperceptible, robust and targeted adversarial examples
 * for ASR": the perturbation's short-time power spectrum is pushed under the masking threshold of the speech it rides on) -----
 * fb_attack_psy is fb_attack_cw2 with a perceptual distortion in place of |delta|^2.  The threshold theta is host work, done
 * once per attack (fakebob_amd/masking.py states the model); the library takes it as data.
 * Framing.  Window W in {512, 1024, 2048}, hop = W/4, K = W/2 + 1 bins.  N >= W samples make F = 1 frames if N == W, else
 * ceil((N - W) / hop) + 1; the signal is extended with zeros to (F-1)*hop + W, so every sample lies in a frame.  The window is
 * the periodic Hann h[n] = 0.5 - 0.5 cos(2 pi n / W), and
 *   p(v)[f,k] = (8/3) * |sum_n h[n] v[f*hop + n] exp(-2 pi i k n / W)|^2 / W^2.
 * Loss.  With theta[F][K] >= 0 (linear power, from masking_threshold on a0) and psd_max = max p(a0):
 *   P = p(delta) * (10^9.6 / psd_max)
 *   D(delta) = (1 / (F K)) sum_{f,k} max(P - theta, 0)        n_over = #{(f,k) : P > theta}
 *   gd = dD / d delta; a bin at equality (P == theta) contributes nothing to D, n_over or gd.
 * The device evaluates P by a radix-2 FFT of the windowed frame in float64 (twiddles from a host table, exact at the octants),
 * and gd as the transpose: the one-sided spectrum times [P > theta], the inverse transform, the window again, the overlap-add of
 * the at most four frames that hold a sample in ascending f.  D is the frames' hinge sums added in ascending f, divided by
 * F K.  No floating-point atomics: every sum has one fixed order, so a run repeats bit for bit and does not depend on
 * FB_ATTACK_BATCH.  D, gd and P are NOT bit-exact contracts against a host DFT (an FFT rounds about log2 W times where a DFT
 * matrix rounds once; DESIGN.md section 6 has the bar); n_over is exact wherever no bin sits within that error of its threshold.
 * The attack is the pseudo-code of fb_attack_cw2 verbatim with these replacements:
 *   delta = x - a0
 *   dist = D(delta) + l2_weight * l2
 *   L = (c*gate)*adver_loss + dist
 *   G = (((c*gate)*g + gd) + l2_weight*(2*(x - a0))) * (1 - x*x)
 *   best-so-far and `take` are decided on dist (gbest_dist in place of gbest_l2)
 *   trace row = {dist, l2, n_over, adver_loss, c, score0[S]}
 * Outputs: best_dist (+inf without a success), best_l2 and best_n_over of the iterate that holds it, the rest as fb_attack_cw2.
 * Victims and refusals are those of fb_attack_cw2, by the same checks (one function serves both: its messages say "CW2").  Also FB_E_ARG: a null
 * fb_psy_params or theta; a window outside the three; N < W; n_frames != F(N, W); a non-finite or negative theta entry; a
 * non-finite or non-positive psd_max; a non-finite or negative l2_weight.  A refusal leaves the engine as it was. */
typedef struct { const double *theta /*[n_frames][window/2 + 1]*/; int n_frames; int window; double psd_max; double l2_weight; } fb_psy_params;
int fb_attack_psy(fb_engine *e, const fb_nes_params *p, const fb_cw2_params *q, const fb_psy_params *m, const double *audio, int64_t N,
                  int16_t *adv_i16, double *adver_f64 /*[N], nullable*/, double *trace /*[search_steps*max_iter][5+S], nullable*/,
                  int *n_trace, int *rows_per_step /*[search_steps]*/, int *success_flag, double *best_dist, double *best_l2,
                  int *best_n_over, double *final_const);

const char *fb_last_error(void);
int fb_version(void);
int fb_device_count(void);

int fb_engine_create(int device, fb_engine **out);
int fb_engine_destroy(fb_engine *e);

void fb_default_frontend(fb_frontend_cfg *cfg);
/* FB_E_ARG, the previous configuration kept, for options that describe no front end: besides the shapes the kernels do
 * not take, cmn_window < 1, vad_frames_context < 0, a mel bin that covers no FFT bin and a negative or non-finite dither. */
int fb_set_frontend(fb_engine *e, const fb_frontend_cfg *cfg);

/* Diagonal GMMs in Kaldi DiagGmm internal form (float32): gconsts[M*C],
 * means_invvars[M*C*D], inv_vars[M*C*D].  Models whose inv_vars are bitwise
 * identical (mean-only MAP adaptation, build_spk_models.py:170) share the
 * quadratic term on device.
 * At most 60 models per engine, the UBM included (the scoring kernels keep 2 KB of logsumexp state per model in LDS: at
 * 60 models and D = 78 .. 80 they ask for 159 744 of a compute unit's 163 840 bytes).  M > 60 is FB_E_ARG, "at most 60 models per engine
 * (got M)", refused before anything is touched: the system loaded before stays loaded and scores as it did. */
int fb_load_gmm(fb_engine *e, int M, int C, int D, const float *gconsts,
                const float *means_invvars, const float *inv_vars);

/* i-vector / PLDA system: everything `sid/extract_ivectors.sh` + `ivector-plda-scoring` read
 * from pre-models/ (final.ubm, final.ie, mean.vec, transform.mat, plda) plus the enrolled
 * i-vectors the wrappers list in ivector.scp (ivector_PLDA_OSI.py:59-60,
 * ivector_PLDA_kaldiHelper.py:197-213,251-280).  Derived variables (diagonalised UBM for
 * gmm-gselect, Sigma^-1 M, U, PLDA-space enrolled vectors) are computed by the engine. */
typedef struct {
  int C, D, R, L, S;                /* Gaussians, feature dim, i-vector dim, LDA dim, speakers */
  int lda_cols;                     /* R, or R+1 when transform.mat carries an offset column */
  int num_gselect;                  /* 20 */
  double min_post;                  /* 0.025 */
  double prior_offset;              /* IvectorExtractor::prior_offset_ */
  const float *fg_weights;          /* [C]          FullGmm */
  const float *fg_means_invcovars;  /* [C*D] */
  const float *fg_inv_covars;       /* [C*D(D+1)/2] packed lower-triangular (SpMatrix) */
  const double *ie_M;               /* [C][D][R]    IvectorExtractor::M_ */
  const double *ie_sigma_inv;       /* [C][D(D+1)/2] IvectorExtractor::Sigma_inv_ (packed) */
  const float *mean_vec;            /* [R]          mean.vec */
  const float *lda;                 /* [L][lda_cols] transform.mat */
  const double *plda_mean;          /* [L] */
  const double *plda_transform;     /* [L][L] */
  const double *plda_psi;           /* [L] */
  const float *enrolled;            /* [S][R] enrolment i-vectors as stored by ivector-extract */
  const double *z_mean, *z_std;     /* [S] z-norm statistics of the speaker-model pickles */
} fb_ivector_system;

/* Loads an i-vector/PLDA system; scores are PLDA LLRs [B*S]; fb_system_scores / the NES
 * kernels apply (llr - z_mean) / z_std for every task (ivector_PLDA_OSI.py:119).
 * At most 60 enrolled speakers per engine (the NES result block holds 62 scores).  S > 60 is FB_E_ARG, "at most 60
 * enrolled speakers per engine", refused before anything is touched: the system loaded before stays loaded. */
int fb_load_ivector(fb_engine *e, const fb_ivector_system *sys, int task);

/* ---- x-vector (TDNN) system ----------------------------------------------------------------------------
 * The Kaldi x-vector recogniser (egs/sre16/v2, egs/voxceleb/v2): frame-level TDNN layers over the voiced, normalised
 * feature rows the front end writes, statistics pooling, one segment-level affine whose output is the embedding, then
 * the back end of the i-vector system (mean subtraction, LDA, length normalisation, PLDA, z-norm).  The engine's system
 * kind 2; scored by fb_score_*, attacked by fb_get_grad, fb_attack, fb_estimate_threshold, fb_attack_pso,
 * fb_attack_kenansville and fb_attack_hsj; every defence in front of the front end, dither, fb_set_eot,
 * fb_set_companions and fb_set_play_offset apply as they do to the other two kinds.
 *
 * Function, for an utterance with T >= 1 voiced rows x[0 .. T):
 *   frame layer   h_out[t] = bn_scale * max(W . splice(h_in, t) + bias, 0) + bn_offset   (Kaldi's relu-batchnorm-layer,
 *                 the batchnorm folded into a scale and an offset per channel).  splice(h_in, t) concatenates
 *                 h_in[clamp(t + ctx[j], 0, T - 1)] for ascending j: the utterance's own edge rows are replicated, never
 *                 a neighbour's of the batch, so every layer keeps T rows and a one-frame utterance has an embedding.
 *                 (Kaldi's nnet3-xvector-compute drops the edge frames that lack their full context instead; a model is
 *                 scored here on T rows where Kaldi pools T - (left + right context) of them.)
 *   pooling       per channel of the last layer: mean and sqrt(max(E[h^2] - mean^2, 1e-10)) over the T rows, float64,
 *                 in an order that depends on T alone.
 *   embedding     seg_W . [mean; std] + seg_bias, float64, fixed order.  No ReLU behind it: Kaldi extracts at the affine.
 *   back end      the i-vector system's, unchanged, on the embedding rounded to float32 (Kaldi stores x-vectors, like
 *                 i-vectors, as float vectors) minus mean_vec.
 * An utterance without a voiced frame is FB_E_NO_VOICED.
 *
 * Arithmetic of the frame layers: values are float32; every product is formed to at least 22 bits (each operand as two
 * f16 terms under a power of two of its own -- one per layer for the weights, chosen at load time, one per row for the
 * spliced input, so operands of any finite magnitude keep their bits --, three of the four partial products on the matrix
 * cores) and accumulated in float32 in an order that depends on the layer's shape alone.  bias, ReLU, scale and offset
 * are float32 operations, each rounded.  Hence
 *   (a) a run repeats bit for bit, and
 *   (b) the embedding of a row does not depend on the batch it is scored in: not on B, its position, or its neighbours'
 *       lengths.
 *
 * Limits: D == the front end's feature dimension; 1 <= n_layers <= 8; 1 <= n_ctx <= 5 with ascending offsets,
 * |offset| <= 8; every dout in 1 .. 2048 (a multiple of 32 wastes no lane; Kaldi's stock pooling width, 1500, is none) and
 * n_ctx * din whatever it is; R a multiple of 32 in 32 .. 2048; L <= 512; S <= 60
 * (SV: S == 1); lda_cols R or R + 1.  Anything else is FB_E_ARG by name and the system loaded before stays loaded.
 * Refused by name ("not in this version") while an x-vector system is loaded: every white-box entry (fb_get_grad_wb*,
 * fb_attack_wb, fb_attack_cw2, fb_attack_psy) unless fb_set_wb_xvector(e, 1) ("white-box gradients" above: the analytic
 * gradient through the TDNN) -- the other fb_set_wb_* switches do not admit it --, fb_set_feature_compression with
 * iters > 0 (k-means discards the frame order a TDNN reads; fb_load_xvector is refused likewise while it is on) and
 * fb_gmm_acc_stats.  fb_last_ivectors returns the embeddings (B x R, float64) of the batch scored last. */
#define FB_XV_MAX_LAYERS 8
#define FB_XV_MAX_CTX 5
typedef struct {
  int dout;                         /* output channels */
  int n_ctx;                        /* 1 .. 5 */
  int ctx[FB_XV_MAX_CTX];           /* ascending frame offsets */
  const float *W;                   /* [dout][n_ctx * din]: Kaldi's affine layout, offsets-major along the columns;
                                       din = D for layer 0, else the previous layer's dout */
  const float *bias;                /* [dout] */
  const float *bn_scale, *bn_offset; /* [dout] */
} fb_xvector_layer;
typedef struct {
  int D;                            /* feature dim */
  int n_layers;                     /* frame-level layers */
  fb_xvector_layer layers[FB_XV_MAX_LAYERS];
  const float *seg_W;               /* [R][2 * P], P = the last frame-level dout: columns [mean; std] */
  const float *seg_bias;            /* [R] */
  int R, L, S;                      /* embedding dim, LDA dim, speakers */
  int lda_cols;                     /* R, or R+1 when transform.mat carries an offset column */
  const float *mean_vec;            /* [R] */
  const float *lda;                 /* [L][lda_cols] */
  const double *plda_mean;          /* [L] */
  const double *plda_transform;     /* [L][L] */
  const double *plda_psi;           /* [L] */
  const float *enrolled;            /* [S][R] enrolment embeddings */
  const double *z_mean, *z_std;     /* [S] */
} fb_xvector_system;
int fb_load_xvector(fb_engine *e, const fb_xvector_system *sys, int task);

/* How raw per-model log-likelihoods become system scores:
 *  OSI / SV: model 0 is the UBM, S = M-1, score = raw[1+s] - raw[0]
 *  CSI     : S = M, score = (raw - z_mean) / z_std                          */
int fb_set_system(fb_engine *e, int task, const double *z_mean, const double *z_std);
int fb_num_speakers(fb_engine *e);

/* Average voiced-frame log-likelihood of every utterance under every model.
 * wav: concatenated samples, off[B+1] offsets; raw[B*M]; tv[B] (nullable) =
 * voiced frame counts. */
int fb_score_i16(fb_engine *e, const int16_t *wav, const int64_t *off, int B,
                 double *raw, int *tv);
int fb_score_f64(fb_engine *e, const double *audio, const int64_t *off, int B,
                 int bits_per_sample, double *raw, int *tv);
/* raw[B*M] -> scores[B*S] per fb_set_system */
int fb_system_scores(fb_engine *e, const double *raw, int B, double *scores);

/* One NES gradient estimate at `audio` (FAKEBOB.py:223-246).  noise_pos:
 * NULL -> Philox(seed, iter, stream); else float64 [N][spd/2] row-major
 * (the tensor np.random.normal would have produced).  grad[N] nullable,
 * score0[S]. */
int fb_get_grad(fb_engine *e, const fb_nes_params *p, const double *audio,
                int64_t N, uint32_t iter, const double *noise_pos,
                double *final_loss, double *grad, double *adver_loss,
                double *score0);

/* Whole attack loop on device.  noise_all NULL or [max_iter][N*(spd/2)].
 * adv_i16[N]; adver_f64[N] nullable; trace[max_iter*(3+S)] nullable rows of
 * {distance, adver_loss, lr_after_iter, score0[S]}; *n_trace rows written;
 * *success_flag = +1/-1 with the reference's iter < max_iter-1 rule (:219). */
int fb_attack(fb_engine *e, const fb_nes_params *p, const double *audio,
              int64_t N, const double *noise_all, int16_t *adv_i16,
              double *adver_f64, double *trace, int *n_trace,
              int *success_flag);

/* Seconds each iteration of the LAST fb_attack / fb_attack_ext took, iteration 0 from the attack's start: the
 * `used_time` column of the reference's trace pickle (FAKEBOB.py:205-212 times every loop body with time.time()).
 * Taken from the device's constant-rate clock where iteration i's loss is evaluated, so it is exact although the
 * host only looks at the device once per batch of iterations.  n <= the number of trace rows of that attack. */
int fb_attack_iter_seconds(fb_engine *e, double *seconds, int n);

/* Threshold sweep (FAKEBOB.py:39-137).  model_threshold: the system's own
 * threshold consulted by make_decisions.  Returns FB_E_LIMIT if
 * max_total_iters gradient steps did not reach acceptance. */
int fb_estimate_threshold(fb_engine *e, const fb_nes_params *p,
                          double model_threshold, const double *audio,
                          int64_t N, const double *noise_all,
                          int max_total_iters, double *score_out,
                          int *n_iters, int *n_outer, double *thr_final,
                          double *adver_f64);

/* ---- foreign models: the reference's plugin API ---------------------------------------------------
 * FakeBob takes ANY `model` object with score / make_decisions (README.md:136; FAKEBOB.py:53,89,250).  For a
 * model that is not one of this library's systems the per-iteration scores come from this callback --
 * audios[B][N] float64, utterance-major: row 0 = the current adversarial audio, rows 1.. = the antithetic NES
 * samples, exactly the columns FAKEBOB.py:234-238 hands to model.score; scores[B*S] out; return 0 -- and
 * everything else of the NES iteration (Philox noise, perturbation, loss, gradient estimate, momentum sign step,
 * clipping, loop control) still runs on the device.  No model has to be loaded into the engine; S = number of
 * enrolled speakers (1 for SV).  Arguments otherwise as fb_get_grad / fb_attack.
 * Lifetime: `audios` points into the engine's staging memory and is valid only DURING the call -- it is reused by the
 * next iteration; a model that keeps its batch must copy it (the Python mirror hands the model a copy). */
typedef int (*fb_score_cb)(void *ctx, const double *audios, int64_t N, int B, double *scores);
int fb_get_grad_ext(fb_engine *e, const fb_nes_params *p, int S, fb_score_cb cb, void *cb_ctx,
                    const double *audio, int64_t N, uint32_t iter, const double *noise_pos,
                    double *final_loss, double *grad, double *adver_loss, double *score0);
int fb_attack_ext(fb_engine *e, const fb_nes_params *p, int S, fb_score_cb cb, void *cb_ctx,
                  const double *audio, int64_t N, const double *noise_all, int16_t *adv_i16,
                  double *adver_f64, double *trace, int *n_trace, int *success_flag);

/* ---- foreign models on the same GPU --------------------------------------------------------------------------
 * The plugin API above for a model that runs on the engine's GPU (a PyTorch model, say): the engine writes each NES
 * batch into the caller's device buffer x, the model reads it and writes its scores into the caller's device buffer
 * `scores`, in the order of the engine's stream, and the loss reads them there.  No copy of the batch or of the scores
 * passes through the host; on the Philox path with samples_per_draw / 2 <= 40 an iteration is 2 engine launches
 * (the loss; the momentum sign step fused with the next batch) around the model's own work.
 *
 * - Arguments, outputs, trace rows, the success flag and fb_attack_iter_seconds behave as in fb_get_grad_ext /
 *   fb_attack_ext; S, task, target and the other parameters are checked the same way.
 * - x[B][N] is utterance-major, rows exactly as fb_attack_ext's `audios`.  A float64 batch holds the same bits the
 *   host path hands its callback; each float32 element is the round-to-nearest of that float64 value (it equals
 *   torch.from_numpy(x64).float()).
 * - scores[B][S]: float32 scores are widened exactly to float64 before the loss.
 * - x and scores must be device memory on the engine's device (checked with hipPointerGetAttributes, and against the
 *   allocation's extent where the runtime reports it): a host or foreign-device pointer or a bad dtype is FB_E_ARG.
 * - The callback enqueues the model on `stream` (the engine's hipStream_t): it reads x and writes scores in stream
 *   order and returns 0; it may return before its work has run.  A non-zero return gives FB_E_CALLBACK.
 * - Both calls return only after the engine stream is idle: the caller may free or reuse its buffers afterwards.
 * - fb_attack_dev reads the loop control block every m->look_every iterations.  Iterations queued after the stopping
 *   one are no-ops on the device; the model may be called up to look_every - 1 more times and those scores are
 *   ignored.  With look_every = 1 the model is called exactly once per executed iteration, as in the host path. */
#define FB_DT_F32 0
#define FB_DT_F64 1
typedef struct {
  int x_dtype;        /* FB_DT_*: element type of the batch the engine writes */
  void *x;            /* caller-owned device buffer [B][N], utterance-major, rows exactly as fb_attack_ext's `audios` */
  int score_dtype;    /* FB_DT_*: element type the model writes */
  void *scores;       /* caller-owned device buffer [B][S] */
  int look_every;     /* fb_attack_dev: the host reads the loop control block every this many iterations; 0 = 4 */
} fb_dev_model;
/* Enqueue the model on `stream` (the engine's hipStream_t): read x and write scores in stream order; return 0.
 * The callback may return before its work has run. */
typedef int (*fb_score_dev_cb)(void *ctx, void *stream, int64_t N, int B, int S);
int fb_get_grad_dev(fb_engine *e, const fb_nes_params *p, int S, const fb_dev_model *m, fb_score_dev_cb cb, void *ctx,
                    const double *audio, int64_t N, uint32_t iter, const double *noise_pos,
                    double *final_loss, double *grad, double *adver_loss, double *score0);
int fb_attack_dev(fb_engine *e, const fb_nes_params *p, int S, const fb_dev_model *m, fb_score_dev_cb cb, void *ctx,
                  const double *audio, int64_t N, const double *noise_all, int16_t *adv_i16,
                  double *adver_f64, double *trace, int *n_trace, int *success_flag);

/* ---- foreign victims for the swarm and the decision-only attacks ----------------------------------------------------------
 * fb_attack_pso, fb_attack_kenansville and fb_attack_hsj against a model that is not one of this library's systems: the
 * victim a decision-only attack exists for -- a commercial API behind a host callback, a neural recogniser in PyTorch on
 * the same GPU.  Each call takes the arguments of its native call plus one descriptor, fb_victim, between the attack's
 * parameters and the native call's tail.
 * The search is the native one.  The candidates, particles, line rows, probes and step sizes, the bracket, the direction,
 *   ssq, the stops, the traces and the logs are those of the three sections "particle-swarm attack", "decision-only attack"
 *   and "decision-only attack II", made by the same launches: the int16 batch a _foreign call produces for a given history
 *   of decisions (losses, for PSO) equals, bit for bit, the batch the native call produces for that history.  Only who
 *   scores the batch differs.
 * What the victim sees.  Row b of a batch is x[b][i] = (double)q[b][i] * 2^-(bits_per_sample - 1), q the int16 row: exact,
 *   and the audio an attacker would submit as a wav file (k_rows_to_model, the one added pass over the batch).
 *   - FB_VICTIM_HOST_SCORES, FB_VICTIM_HOST_DECISIONS: the callback gets the rows as float64 [B][N], utterance-major, in the
 *     engine's staging memory; lifetime as for fb_score_cb (valid only DURING the call).
 *   - FB_VICTIM_DEVICE_SCORES: the rows go into dev->x as dev->x_dtype; the float32 value is exact too.  score_dev then
 *     enqueues the model on the engine's stream as for fb_attack_dev and writes dev->scores [B][S] as dev->score_dtype.
 *     dev->x must hold rows_max * N elements and dev->scores rows_max * S: rows_max = particles (PSO), grid (Kenansville),
 *     max(grid, num_evals_max) (HopSkipJump).  The device, dtype and extent checks are fb_attack_dev's (FB_E_ARG).
 *     dev->look_every is not read: these attacks look once per batch.
 *   - The callback runs exactly once per scored batch, with that batch's row count as B.
 * Decisions (fb_attack_kenansville_foreign, fb_attack_hsj_foreign).
 *   - FB_VICTIM_HOST_DECISIONS: decisions[B] are the callback's values, checked: a decision value of the task (SV +-1, OSI
 *     -1 .. S - 1, CSI 0 .. S - 1) or -2 = no decision (never adversarial, never a success, never an error, as a row without
 *     voiced frames in the native calls).  Anything else is FB_E_CALLBACK, the value named in fb_last_error.  scores[B * S]
 *     is prefilled with NaN by the engine; the model MAY write its scores there.
 *   - FB_VICTIM_HOST_SCORES, FB_VICTIM_DEVICE_SCORES: the model's scores are the system scores as they stand -- no UBM
 *     subtraction and no z-norm: the model's output is final, as for fb_attack_ext -- and the decision is the rule of the
 *     "decision-only attack" section: SV  s >= threshold ? 1 : -1;  OSI, CSI  the first maximum by strict > in ascending m, so
 *     that a NaN never displaces the running maximum (a NaN in column 0 stays it);  OSI  a maximum < threshold gives -1.
 *     float32 scores are widened exactly before any comparison.  -2 never arises.  One launch (k_decide_foreign) writes the
 *     look block {decisions [rows] int32, padding to 8 bytes, scores [rows][S] float64}, which the host copies once per batch.
 *   - fb_attack_kenansville_foreign's scores[r][G][S] log holds the model's scores, or NaN where a decision callback wrote
 *     none.
 * fb_attack_pso_foreign takes the two score modes; FB_VICTIM_HOST_DECISIONS is FB_E_ARG.  loss_fn is formed on the device
 *   from the model's scores exactly as fb_attack_ext / fb_attack_dev form it.  There is no FB_E_NO_VOICED.
 * No system need be loaded.  The engine's defences -- the input-transform chain, the codec, the air channel, feature
 *   compression and dither -- are NOT applied to a foreign batch, as documented for fb_attack_ext.
 * FB_E_STATE before anything runs, the setting named in the message, while fb_set_eot(r > 1), companions
 *   (fb_set_companions), a play offset (fb_set_play_offset) or fb_set_query_eot is in force: a foreign victim's randomness is
 *   its own.
 * FB_E_ARG: a null descriptor; an unknown mode; the callback of the mode missing (score for HOST_SCORES, decide for
 *   HOST_DECISIONS, dev and score_dev for DEVICE_SCORES); S outside 1 .. 62; FB_TASK_SV with S != 1; the native calls' own
 *   parameter and label rules (labels against the descriptor's S).  N >= 1 suffices: there is no front end, hence no
 *   "shorter than one frame" rule.
 * A non-zero callback return is FB_E_CALLBACK.  The engine stays usable after every refusal and every callback failure.
 * *n_queries, max_queries and the traces' query columns count rows handed to the model.  fb_attack_iter_seconds behaves as
 *   in the native calls; fb_stats does not count foreign rows.  fb_debug_foreign_path (fakebob_hip_test.h) reports host or
 *   device and the dtypes for these calls too. */
typedef int (*fb_decide_cb)(void *ctx, const double *audios /*[B][N]*/, int64_t N, int B, int *decisions /*[B] out*/,
                            double *scores /*[B*S], NaN on entry, optional out*/);
enum { FB_VICTIM_HOST_SCORES = 1, FB_VICTIM_HOST_DECISIONS = 2, FB_VICTIM_DEVICE_SCORES = 3 };
typedef struct {
  int mode;                    /* FB_VICTIM_* */
  int S;                       /* enrolled speakers (1 for SV) */
  fb_score_cb score;           /* FB_VICTIM_HOST_SCORES */
  fb_decide_cb decide;         /* FB_VICTIM_HOST_DECISIONS */
  const fb_dev_model *dev;     /* FB_VICTIM_DEVICE_SCORES: the caller's buffers ... */
  fb_score_dev_cb score_dev;   /* ... and the model */
  void *ctx;                   /* handed to the callback of the mode */
} fb_victim;
int fb_attack_pso_foreign(fb_engine *e, const fb_nes_params *p, const fb_pso_params *q, const fb_victim *v, const double *audio,
                          int64_t N, int16_t *adv_i16, double *adv_f64 /*nullable*/, int *success, int *n_iters,
                          double *trace /*[max_iter][3 + S]*/, double *losses /*[max_iter][P]*/);
int fb_attack_kenansville_foreign(fb_engine *e, const fb_nes_params *p, const fb_kv_params *k, const fb_victim *v,
                                  const int32_t *tables /*[4][W]*/, const double *audio, int64_t N, int16_t *adv_i16, int *success,
                                  int *factor, int *n_queries, int *n_rounds, int *qs /*[max_rounds][G]*/,
                                  int *decisions /*[max_rounds][G]*/, double *scores /*[max_rounds][G][S]*/,
                                  int *trace /*[max_rounds][3]*/);
int fb_attack_hsj_foreign(fb_engine *e, const fb_nes_params *p, const fb_hsj_params *k, const fb_victim *v, const double *audio,
                          const double *init, int64_t N, int16_t *adv_i16, double *adv_f64 /*nullable*/, int *success,
                          double *dist2, int *n_iters, int *n_queries, double *trace /*[max_iter + 1][8]*/,
                          int *decisions /*[decisions_cap]*/, long long decisions_cap, double *x_trace /*nullable*/);

/* Launch chain of the device-controlled attack loop.  on = 1: 4 launches per NES iteration of a GMM system (MFCC; VAD +
 * deltas + CMVN; GMM log-likelihoods; finalisation + loss + loop control + update of iteration i + perturbation of
 * i + 1 in one) and, for i-vector systems, the five-workgroups-per-matrix posterior solve -- fastest for ONE or TWO
 * attacks per GPU, the reference's own use; on = 0: 6 launches -- finalisation and loss on their own, the front-end kernel at its own LDS size --, which interleave
 * better when several engines share a GPU (3 or more attacks in flight: +7 % NES iterations/s, profiles/r05_*;
 * FB_NO_FUSE=1: all 8); -1: default (fused unless
 * FB_NO_FUSE is set).  Once three or more engines of the process on one device are set to 0 -- the shared GPU itself --
 * their attacks queue the next look's iterations before they wait for the last look's control block (FB_LOOK_AHEAD=0:
 * not; = 1: every attack of the engine's own systems on Philox noise), so that a stream does not run dry at a look; an
 * attack that stops has then queued one more look of launches, which return on the stop flag.  Trajectories are
 * bit-identical either way. */
int fb_set_fused_chain(fb_engine *e, int on);

/* Work counters since engine creation: what the driver reduces over ranks next to the success counter
 * (attackMain.py:312,411 keeps success_cnt / total_cnt only). */
int fb_stats(fb_engine *e, int64_t *scored_utts, int64_t *scored_frames,
             int64_t *voiced_frames, int64_t *nes_iters);

/* ---- enrolment (build_spk_models.py) ------------------------------------------
 * fb_gmm_acc_stats replaces `gmm-global-acc-stats --update-flags=m final.dubm feats acc`
 * (build_spk_models.py:197-204): with the UBM loaded ALONE (fb_load_gmm, M = 1) it returns the float64
 * zeroth / first order statistics occ[C], F[C*D] of one utterance's voiced, CMVN'd delta features.  The
 * MAP mean update itself (gmm-global-est-map.cc:62-92, `MapDiagGmmUpdate`, means only) is a C*D
 * element-wise formula done by the host mirror (fakebob_amd/enroll.py).
 * fb_last_ivectors returns the i-vectors (B x R, float64, before mean subtraction / LDA) of the batch scored
 * last with an i-vector system: the enrolment identity of ivector_PLDA (build_spk_models.py:104-150); with an x-vector
 * system the embeddings (B x R, float64). */
int fb_gmm_acc_stats(fb_engine *e, const int16_t *wav, int64_t n, double *occ, double *F, int *tv_out);
int fb_last_ivectors(fb_engine *e, int B, double *ivecs);

#ifdef __cplusplus
}
#endif
#endif
