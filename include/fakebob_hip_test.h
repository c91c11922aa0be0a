/*
 * fakebob_hip_test.h -- test / profiling hooks of libfakebob_hip.so.
 *
 * Not part of the drop-in boundary (include/fakebob_hip.h): these entry points have no counterpart in the
 * reference.  tests/ use them to compare intermediate stages with the oracle (noise stream, int16 cast, MFCC,
 * compacted features), bench.py to time the dominant kernel and a run of NES iterations without host round
 * trips.  Same conventions as fakebob_hip.h (0 / negative FB_E_* + fb_last_error()).
 */
#ifndef FAKEBOB_HIP_TEST_H
#define FAKEBOB_HIP_TEST_H
#include "fakebob_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* z[half*N] float32 from the device Philox/Box-Muller (bit-exact contract) */
int fb_debug_noise(fb_engine *e, uint64_t seed, uint32_t iter, uint32_t stream,
                   int64_t N, int half, float *z);
/* the device int16 cast of model.score's float input (gmm_ubm_OSI.py:83-85) */
int fb_debug_quantize(fb_engine *e, const double *x, int64_t n, int bits_per_sample, int16_t *q);
/* front-end only: MFCC [T*num_ceps] of one utterance */
int fb_debug_mfcc(fb_engine *e, const int16_t *wav, int64_t n, float *mfcc, int *T);
/* compacted voiced CMVN'd features of one utterance: feats[Tv*dim] */
int fb_debug_feats(fb_engine *e, const int16_t *wav, int64_t n, float *feats,
                   int *Tv, int *T);

/* Kaldi's dither (fakebob_hip.h, "Dither RNG contract").
 * fb_debug_dither_noise: the normals z[n_frames * L] the dithered MFCC kernels add to samples 0 .. L - 1 of frames t0 .. t0 + n_frames
 * - 1 of utterance `utt` at (seed, stream, epoch), produced by the device function the kernels call.
 * fb_debug_mfcc_dither / fb_debug_feats_dither: fb_debug_mfcc / fb_debug_feats of one utterance at that point of the contract
 * (it is utterance `utt` of a call with that seed, stream and epoch), on whatever route the current front-end selects; the
 * engine's own dither seed and scoring-call serial are neither used nor advanced.  With dither 0 they equal fb_debug_mfcc /
 * fb_debug_feats bit for bit. */
int fb_debug_dither_noise(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int t0, int n_frames,
                          int L, float *z);
int fb_debug_mfcc_dither(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream, uint32_t epoch,
                         uint32_t utt, float *mfcc, int *T);
int fb_debug_feats_dither(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream, uint32_t epoch,
                          uint32_t utt, float *feats, int *Tv, int *T);

/* The int16 batch the MFCC reads with the engine's input-transform chain (fb_set_input_transform): out, in wav's layout
 * (off[B + 1], off[0] = 0), from the kernel the scoring paths launch.  Utterances may be of any length >= 1 (shorter than a
 * frame included: nothing but the transform runs).  Without a chain out equals wav. */
int fb_debug_input_transform(fb_engine *e, const int16_t *wav, const int64_t *off, int B, int16_t *out);

/* Randomised stages and replication (fakebob_hip.h: FB_TF_NOISE, "Noise RNG contract", fb_set_eot).
 * fb_debug_tf_noise: the normals z[n] the noise stage at position `stage` of a chain adds to samples i0 .. i0 + n - 1 of
 * utterance `utt`, replica `replica`, at (seed, stream, epoch), from the device function the transform kernel calls.
 * fb_debug_input_transform_eot: fb_debug_input_transform at that point of the contract with every utterance written r
 * times: out holds B * r utterances, replica j of utterance b at row b * r + j (rows one after the other, each as long as
 * its utterance).  The engine's fb_set_eot value, dither seed and scoring-call serial are neither used nor advanced. */
int fb_debug_tf_noise(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica, int stage,
                      int64_t i0, int64_t n, float *z);
int fb_debug_input_transform_eot(fb_engine *e, const int16_t *wav, const int64_t *off, int B, int r, uint64_t seed,
                                 uint32_t stream, uint32_t epoch, int16_t *out);

/* Companion utterances (fakebob_hip.h: fb_set_companions, "Composition" and "Row order").
 * fb_debug_compose: the int16 rows the composing launch (the engine's input-transform chain included) writes for a hand-made
 * batch: q[B][N] the NES rows, a0[N] the cast original, r the draws per utterance at (seed, stream, epoch) of the noise
 * contract; out[B * K * r][N], replica u * r + j of row b at row b * K * r + u * r + j, K - 1 the engine's companions (none
 * set: K = 1, the rows are the chain's over q).  N must be the companions'.  The engine's fb_set_eot value, dither seed and
 * scoring-call serial are neither used nor advanced.
 * (fb_bench_nes below times the attack loop as it is configured, companions included, as it does for fb_set_eot.) */
int fb_debug_compose(fb_engine *e, const int16_t *q, int B, int64_t N, const int16_t *a0, int r, uint64_t seed,
                     uint32_t stream, uint32_t epoch, int16_t *out);

/* Over-the-air channel (fakebob_hip.h: fb_set_air_channel and its contract).  With a channel set,
 * fb_debug_input_transform_eot and fb_debug_compose above -- they carry a point of the contract -- apply it in front of the
 * chain, as the scoring path does; fb_debug_input_transform has no point and ignores the channel.
 * fb_debug_air_taps: what k_air_taps writes for ONE row -- utterance row `utt`, replica `replica` at (seed, stream, epoch) --
 * under the engine's channel setting (FB_E_STATE without one): taps[L] int16, and (both nullable) the normals z[L] and the
 * decay's word w it used.
 * fb_debug_air_convolve: k_air_conv on taps handed in as they are -- taps[B][L] int16, any values, L in 2 .. 4096 -- over B
 * rows of any length >= 1 (off[B + 1], off[0] = 0); out has wav's layout.  The engine's setting is neither used nor changed. */
int fb_debug_air_taps(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica, int16_t *taps,
                      float *z, uint32_t *w);
int fb_debug_air_convolve(fb_engine *e, const int16_t *wav, const int64_t *off, int B, const int16_t *taps, int L, int16_t *out);

/* Telephone-line codec (fakebob_hip.h: fb_set_codec and its stage contract).  The hooks above that return int16 rows
 * (fb_debug_input_transform*, fb_debug_compose -- unless a play offset is set, see below --, fb_debug_air_*) ignore the codec; fb_debug_mfcc / _feats apply it.
 * fb_debug_codec: k_codec on rows handed in as they are -- B rows of any length >= 1 (off[B + 1], off[0] = 0), B up to
 * 65535; out has wav's layout.  kind (FB_CODEC_ULAW, _ALAW or _ADPCM) comes from the argument: the engine's setting is
 * neither read nor changed.
 * FB_CODEC_TILE: the samples of a row the ADPCM kernel holds in LDS at a time (row lengths around its multiples are the
 * kernel's edges). */
#define FB_CODEC_TILE 512
int fb_debug_codec(fb_engine *e, int kind, const int16_t *wav, const int64_t *off, int B, int16_t *out);

/* Feature compression (fakebob_hip.h: fb_set_feature_compression and its stage contract).
 * fb_debug_feature_compress: the kernel the scoring paths launch, on feature rows handed in as they are (no front end, no
 * model; D = the front end's feature dimension): feats holds the rows of B * r utterance rows one after the other,
 * row_off[B * r + 1] their offsets (row_off[0] = 0; an empty row is allowed), row b * r + j being replica j of utterance b
 * at (seed, stream, epoch) of the contract.  out (as many floats as feats) receives the compressed rows, out_off[B * r + 1]
 * their offsets.  It uses the engine's ratio and iters (FB_E_STATE when the setting is off); the dither seed and the
 * scoring-call serial are neither used nor advanced.
 * fb_debug_feco_keys: keys[T] of the frames 0 .. T - 1 of (utterance `utt`, replica) at that point of the contract. */
int fb_debug_feature_compress(fb_engine *e, const float *feats, const int *row_off, int B, int r, uint64_t seed,
                              uint32_t stream, uint32_t epoch, float *out, int *out_off);
int fb_debug_feco_keys(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica, int T,
                       uint32_t *keys);

/* Particle-swarm attack (fakebob_hip.h: fb_attack_pso and its arithmetic).  Both hooks run exactly the launches the attack
 * runs, on swarms handed in as they are; no system has to be loaded.  P = 2 .. 64, N >= 1, bits = 2 .. 16.
 * fb_debug_pso_init: the swarm at t = 0 -- x, v [P][N] float64 and q [P][N], the int16 cast of x (the first batch).
 * fb_debug_pso_step: update t >= 1 of the swarm x, v, pb [P][N], gb [N] with what the host would have decided riding along:
 * pb_p = x_p for every p with improved[p] != 0, gb = x_{g_new} unless g_new = -1 (in an attack g_new improved in that
 * iteration, so this is pb_{g_new}; the hook takes any combination) -- both BEFORE the velocities read them.  Outputs: the new
 * x, v, pb, gb and q, the int16 cast of the new x (the next batch). */
int fb_debug_pso_init(fb_engine *e, const double *audio, int64_t N, double epsilon, int P, double v_max, uint64_t seed,
                      uint32_t stream, int bits, double *x, double *v, int16_t *q);
int fb_debug_pso_step(fb_engine *e, const double *audio, int64_t N, double epsilon, int P, const double *x, const double *v,
                      const double *pb, const double *gb, const int *improved, int g_new, double w, double c1, double c2,
                      double v_max, uint64_t seed, uint32_t stream, uint32_t t, int bits, double *x_out, double *v_out,
                      double *pb_out, double *gb_out, int16_t *q_out);

/* Decision-only attack (fakebob_hip.h: fb_attack_kenansville and its signal contract).  Both hooks run exactly the launches
 * the attack runs, on int16 samples handed in as they are; no system has to be loaded.  W = 8 .. 128, N >= 1, tables
 * [4][W] as the attack takes them; K = W / 2 + 1, nw = ceil(N / W).
 * fb_debug_kv_analyse: a, b [nw][K] (the device keeps m a and m b; the hook divides), cum [nw][K] in bin order, E [nw].
 * fb_debug_kv_candidates: the analysis, then one candidate launch for the factors q[0 .. rows), rows = 1 .. 64, each
 * 0 .. 65536 -> y [rows][N]. */
int fb_debug_kv_analyse(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, int32_t *a, int32_t *b,
                        int64_t *cum, int64_t *E);
int fb_debug_kv_candidates(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, const int *q, int rows,
                           int16_t *y);
/* tools/kenansville_rate.py: the two launches alone, `reps` of each between two events after one of each to warm up ->
 * ms[2] = milliseconds per analysis launch, per candidate launch of `rows` rows. */
int fb_bench_kv_kernels(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, const int *q, int rows, int reps,
                        double *ms);

/* Decision-only attack II (fakebob_hip.h: fb_attack_hsj and its contract).  Every hook runs exactly the launches the attack
 * runs, on float64 state handed in as it is; no system has to be loaded.  N >= 1, bits 2 .. 16.
 * fb_debug_hsj_line: the rows of line(y, q[0 .. rows)), rows = 1 .. 64, each q 0 .. 2^20 -> out [rows][N]; and the adopt
 *   launch for q[0]: x [N] = line(y, q[0]) in float64, *D2 = ssq(x - a).
 * fb_debug_hsj_probes: the probes of x at iteration t, B = 1 .. 1024 -> out [B][N].
 * fb_debug_hsj_dir: v [N] = sum_j w_j z_j of iteration t (|w_j| <= 2048) and *S = ssq(v); the normals come from a probes
 *   launch in front of it, as in the attack.
 * fb_debug_hsj_step: the G = 1 .. 64 step rows of (x, v, S, xi) -> out [G][N], and y [G][N]: the float64 launch of one m,
 *   for every m in turn. */
int fb_debug_hsj_line(fb_engine *e, const double *a, const double *y, int64_t N, const int *q, int rows, int bits, int16_t *out,
                      double *x, double *D2);
int fb_debug_hsj_probes(fb_engine *e, const double *x, int64_t N, double sigma, uint64_t seed, uint32_t stream, uint32_t t, int B,
                        int bits, int16_t *out);
int fb_debug_hsj_dir(fb_engine *e, const int32_t *w, int B, uint64_t seed, uint32_t stream, uint32_t t, int64_t N, double *v,
                     double *S);
int fb_debug_hsj_step(fb_engine *e, const double *x, const double *v, int64_t N, double S, double xi, int G, int bits,
                      int16_t *out, double *y);
/* tools/hsj_rate.py: every launch alone, `reps` of each between two events after one of each to warm up -> ms[8] =
 * milliseconds per launch of: line (G rows), adopt + sum, probes (B rows), probes that also keep their normals as float32
 * [B][N], direction + sum drawing the normals again, direction + sum reading the kept ones, step (G rows), the NES batch
 * launch (k_perturb) of 2 ceil(B / 2) + 1 rows. */
int fb_bench_hsj_kernels(fb_engine *e, const double *a, const double *y, int64_t N, int B, int G, int bits, int reps, double *ms);

/* Voted decisions (fakebob_hip.h: fb_set_query_eot).  fb_debug_vote runs k_vote alone, exactly the launch the attacks run, on
 * raw scores handed in: raw [rows][r][n_out] -- what fb_score_* returns for the loaded system, n_out columns per row -- and
 * tv [rows * r] (<= 0: that replica has no voiced frames).  The loaded system gives n_out, S and the z-norm tables; `task`
 * must be the engine's; label is the target (FB_TARGETED) or the true label (FB_UNTARGETED), a decision value.  rows * r <=
 * 65535, r = 1 .. 32.  Outputs: votes [rows], nodec [rows], mean [rows][S].
 * fb_bench_vote (tools/query_eot_rate.py): the same launch `reps` times between two events after one to warm up -> *ms per
 * launch. */
int fb_debug_vote(fb_engine *e, const double *raw, const int *tv, int rows, int r, int task, double threshold, int attack_type,
                  int label, int *votes, int *nodec, double *mean);
int fb_bench_vote(fb_engine *e, const double *raw, const int *tv, int rows, int r, int task, double threshold, int attack_type,
                  int label, int reps, double *ms);

/* Foreign victims of the swarm and the decision-only attacks (fakebob_hip.h: fb_attack_*_foreign).  No system need be loaded.
 * fb_debug_rows_to_model runs k_rows_to_model alone, exactly the launch the attacks run: rows_i16 [rows][N] -> out_host
 * [rows][N] of dtype (FB_DT_*), out = q * 2^-(bits - 1).
 * fb_debug_decide_foreign runs k_decide_foreign alone: scores_host [rows][S] of dtype -> decisions [rows] and the scores
 * widened to float64 [rows][S], the two parts of the look block.
 * fb_bench_foreign_rows (tools/foreign_rate.py): ms[5] = milliseconds per launch of k_rows_to_model<float>,
 * k_rows_to_model<double> (rows x N) and k_decide_foreign<double> (rows x S), `reps` of each between two events after one to
 * warm up; then, on the host's clock, the float64 rows copied to host memory, and the int16 rows copied and widened there. */
int fb_debug_rows_to_model(fb_engine *e, const int16_t *rows_i16, int rows, int64_t N, int bits, int dtype, void *out_host);
int fb_debug_decide_foreign(fb_engine *e, const void *scores_host, int dtype, int rows, int S, int task, double threshold,
                            int *decisions, double *scores_f64);
int fb_bench_foreign_rows(fb_engine *e, int rows, int64_t N, int bits, int S, int reps, double *ms);

/* What the front end of the last batch ran (fb_score_*, fb_get_grad, an NES iteration, fb_debug_mfcc / _feats, enrolment
 * statistics): info[5] = {the MFCC kernel, the chain after it, where the CompressedMatrix round trip ran, the longest
 * utterance of the batch in frames, the batch size}.  Recorded on the host when the kernels are enqueued; read only.
 * An entry is FB_ROUTE_NONE when that stage launched nothing (a call that failed before its chain was enqueued reports
 * no chain).  FB_E_STATE before the first batch. */
int fb_debug_frontend_route(fb_engine *e, int *info);
/* info[0] */
#define FB_ROUTE_NONE 0
#define FB_ROUTE_MFCC_F32_12 1       /* k_mfcc_f32<12> */
#define FB_ROUTE_MFCC_F32_0 2        /* k_mfcc_f32<0> */
#define FB_ROUTE_MFCC_R16_12_RAW 3   /* k_mfcc_r16<12, true> */
#define FB_ROUTE_MFCC_R16_12 4       /* k_mfcc_r16<12, false> */
#define FB_ROUTE_MFCC_R16_0_RAW 5    /* k_mfcc_r16<0, true> */
#define FB_ROUTE_MFCC_R16_0 6        /* k_mfcc_r16<0, false> */
#define FB_ROUTE_MFCC_GENERIC 7      /* k_mfcc<false> */
/* ... the dithered forms (fb_frontend_cfg.dither > 0) */
#define FB_ROUTE_MFCC_F32_12_DITHER 8      /* k_mfcc_f32<12, true> */
#define FB_ROUTE_MFCC_F32_0_DITHER 9       /* k_mfcc_f32<0, true> */
#define FB_ROUTE_MFCC_R16_12_RAW_DITHER 10 /* k_mfcc_r16<12, true, true> */
#define FB_ROUTE_MFCC_R16_12_DITHER 11     /* k_mfcc_r16<12, false, true> */
#define FB_ROUTE_MFCC_R16_0_RAW_DITHER 12  /* k_mfcc_r16<0, true, true> */
#define FB_ROUTE_MFCC_R16_0_DITHER 13      /* k_mfcc_r16<0, false, true> */
#define FB_ROUTE_MFCC_GENERIC_DITHER 14    /* k_mfcc<true> */
/* info[1] */
#define FB_ROUTE_CHAIN_SPLIT 1       /* k_vad_delta_cmvn_p: an utterance over four workgroups */
#define FB_ROUTE_CHAIN_WHOLE 2       /* k_vad_delta_cmvn: one workgroup per utterance */
#define FB_ROUTE_CHAIN_VAD_DC 3      /* k_vad, then k_delta_cmvn */
#define FB_ROUTE_CHAIN_SEPARATE 4    /* k_vad, k_deltas, k_cmvn (whole-utterance mean) */
#define FB_ROUTE_CHAIN_SLIDING 5     /* k_vad, k_deltas, k_cmvn, k_cmvn_sliding (some utterance longer than cmn_window) */
/* info[2] (FB_ROUTE_NONE: compress_feats off) */
#define FB_ROUTE_CM_FUSED 1          /* inside k_vad_delta_cmvn */
#define FB_ROUTE_CM_REGS 2           /* k_feat_compress, sort keys in registers */
#define FB_ROUTE_CM_LDS 3            /* k_feat_compress, sort keys in LDS */
#define FB_ROUTE_CM_GLOBAL 4         /* k_feat_compress, columns read from global memory (longer than LDS holds) */

/* The launch geometry of the last batch (fb_score_*, fb_get_grad, an NES iteration, fb_debug_gmm_frames, fb_debug_mfcc /
 * _feats, enrolment statistics), as the launchers chose it: info[13] = {the GMM kernel (FB_SHAPE_GMM_*: the scoring kernel,
 * or the per-component dump of an i-vector batch or of enrolment statistics), component chunks, chunks one k_gmm_fx2w
 * workgroup scores one after the other (1 when fxw_sub does not divide the chunk count), the grid's chunk dimension, the XCD
 * mapping (the chunk count it serves, 0: the plain 2-D grid), launches (k_gmm_fx2w's passes), frame strips, fewest and most
 * component tiles of any chunk, then k_mfcc_f32's compute units, rounds and workgroups, then the threads per workgroup of
 * the update launch that followed the batch inside an attack: 256 or 512 for k_update_perturb / k_update_perturb_x, 512
 * for the update workgroups of k_gmm_finalize_loss_update}.  A stage that launched nothing in
 * that batch reports zeros.  Recorded on the host when the kernels are enqueued; read only.  FB_E_STATE before the first
 * batch. */
int fb_debug_launch_shape(fb_engine *e, int *info);
/* The engines of this process on e's device whose chain is the shared-GPU one (fb_set_fused_chain(e, 0)), e included when its
 * own is: from three on, such an engine's next attack does not drain its stream between looks (FB_LOOK_AHEAD). */
int fb_debug_shared_chain_engines(fb_engine *e, int *count);
#define FB_SHAPE_GMM_NONE 0
#define FB_SHAPE_GMM_FX2W 1          /* k_gmm_fx2w */
#define FB_SHAPE_GMM_FX2 2           /* k_gmm_fx2 */
#define FB_SHAPE_GMM_BX3 3           /* k_gmm_bx3 */

/* The last foreign-model call (fb_get_grad_ext / fb_attack_ext or fb_get_grad_dev / fb_attack_dev): path (FB_FOREIGN_*),
 * the batch and score dtypes (FB_DT_*; the host path hands its callback float64 and reads float64 back), the engine
 * launches of one NES iteration, the model calls, and the bytes of the batch copied device -> host and of the scores
 * copied host -> device during the loop (final outputs and control-block reads not counted).  Recorded on the host as
 * the work is enqueued.  FB_E_STATE before the first foreign call.
 * fb_attack_pso_foreign, fb_attack_kenansville_foreign and fb_attack_hsj_foreign are recorded too: FB_FOREIGN_DEV for
 * FB_VICTIM_DEVICE_SCORES, FB_FOREIGN_HOST for the two host modes; launches_per_iter then counts the engine launches of one
 * scored BATCH (the conversion; k_loss or k_decide_foreign in the score modes), model_calls the scored batches. */
#define FB_FOREIGN_HOST 1   /* fb_get_grad_ext / fb_attack_ext */
#define FB_FOREIGN_DEV 2    /* fb_get_grad_dev / fb_attack_dev */
typedef struct {
  int path;
  int x_dtype;
  int score_dtype;
  int launches_per_iter;
  int64_t model_calls;
  int64_t batch_bytes_d2h;
  int64_t score_bytes_h2d;
} fb_foreign_path_info;
int fb_debug_foreign_path(fb_engine *e, fb_foreign_path_info *info);

/* Where the loss and the momentum step of the last fb_get_grad* / fb_attack* call ran: info[FB_NES_ROUTE_N] counts the
 * launches of each kind the call enqueued, one per NES iteration queued (those queued behind the stopping iteration
 * included).  Recorded on the host as the work is enqueued. */
#define FB_NES_ROUTE_IV_TAIL 0            /* the loss body in the tail of the i-vector solve kernel */
#define FB_NES_ROUTE_FIN_LOSS 1           /* k_gmm_finalize_loss: GMM finalisation + loss body */
#define FB_NES_ROUTE_FIN_LOSS_UPDATE 2    /* k_gmm_finalize_loss_update: ... + momentum step + the next batch */
#define FB_NES_ROUTE_K_LOSS 3             /* k_loss / k_loss_eot on their own */
#define FB_NES_ROUTE_K_UPDATE_PERTURB 4   /* k_update_perturb / k_update_perturb_x: momentum step + the next batch */
#define FB_NES_ROUTE_K_GRAD_UPDATE 5      /* k_grad_update on its own */
#define FB_NES_ROUTE_N 6
int fb_debug_nes_route(fb_engine *e, int *info);
/* What the last fb_get_grad* / fb_attack* / fb_bench_nes call left on the device, read only (no launch; the attack can be
 * continued afterwards): q[2 half + 1][N] the int16 batch of the engine's own systems (nullable; FB_E_STATE when q is asked for
 * after a foreign-model call, whose batch lives in the caller's x, or under fb_set_eot / fb_set_companions), z[half][N] the
 * float32 normals kept for the gradient (nullable; FB_E_STATE after a call on injected normals, which keeps none), *iter
 * (nullable) the Philox iteration index those rows were drawn for.  FB_E_STATE before the first such call, after one that
 * failed and after any call that reuses the buffers; FB_E_ARG when N or half is not the last call's.
 * Which batch that is, recorded on the host as the launches are enqueued: fb_get_grad*: the call's own.  An attack that ran to
 * max_iter on a route whose update launch writes the next batch (k_update_perturb(_x), k_gmm_finalize_loss_update): iteration
 * max_iter's, built from the returned float64 audio and never scored; on the other routes (k_perturb*, k_grad_update):
 * iteration max_iter - 1's, built from the iterate before the last step.  An attack that stopped early: the stopping
 * iteration's.  fb_attack's epilogue quantises the returned audio into row 0 of q: where the update launch wrote the batch that
 * is the value it wrote there. */
int fb_debug_nes_batch(fb_engine *e, int64_t N, int half, int16_t *q, float *z, long long *iter);

/* Which diagonal-GMM arithmetic the loaded model runs on: 2 = two-term f16 split (k_gmm_fx2w / k_gmm_fx2, default),
 * 1 = exact three-term bf16 split (k_gmm_bx3: chosen automatically when a parameter does not fit f16's exponent
 * range; FB_GMM_MODE=bx3 forces it).  Negative FB_E_* without a model.
 * (No reference counterpart: the reference runs Kaldi's float32 CPU code, gmm_ubm_kaldiHelper.py:202-221.) */
int fb_gmm_kernel_mode(fb_engine *e);
/* The kernel fb_score_* / the NES loop launch for the loaded GMM system: 1 = k_gmm_bx3, 2 = k_gmm_fx2 (any number of
 * variance groups, partial tiles, more than 28 models), 10 + P = k_gmm_fx2w (one variance group, 2 .. 28 models -- more than
 * 10 in two or three launches --: the
 * speaker models are scored as deltas from model 0 with 1 .. 3 partial products per K chunk (or class 6, below), chosen by fb_load_gmm PER
 * 32-COMPONENT TILE from how far the tile's components were adapted; P = the count most tiles run, *shift_rms
 * (nullable) returns the rms adaptation statistic; FB_GMM_DELTA_P forces one count for every tile; FB_GMM_NARROW=1
 * selects k_gmm_fx2 instead).  Negative FB_E_* without a model. */
int fb_gmm_kernel_variant(fb_engine *e, double *shift_rms);
/* k_gmm_fx2w's tile classes for the loaded model: how many component tiles run 1 / 2 / 3 partial products per K chunk
 * in their delta items (all zero, return value 0, when another kernel scores the model; 1 otherwise). */
int fb_gmm_delta_tiles(fb_engine *e, int *tiles_p1, int *tiles_p2, int *tiles_p3);
/* ... and how many run the F6 class: the leading f16 product plus the two correction products in block-scaled fp6
 * (fb_gmm_kernel_variant returns 16 when most tiles do; FB_GMM_DELTA_P=6 forces it for every tile, FB_GMM_DELTA_F6=0
 * keeps the rule from choosing it).  tiles_p1 + tiles_p2 + tiles_p3 + this = the model's component tiles. */
int fb_gmm_delta_tiles_f6(fb_engine *e);

/* The loaders' host preparation, without an engine and without a GPU: what fb_load_gmm, fb_load_ivector and
 * fb_set_frontend compute on the host before they touch the device (csrc/fb_prepare.h), under the same argument checks
 * and the same environment variables (FB_GMM_MODE, FB_GMM_DELTA_BUDGET, FB_GMM_DELTA_F6, FB_GMM_DELTA_P), with the
 * loaders' error codes and texts.  Named buffers come back size-then-fill: *size (nullable) receives the buffer's bytes;
 * with out != NULL the bytes are copied there, FB_E_ARG when cap is smaller.  A buffer the preparation did not build has
 * size 0.
 * fb_debug_prepare_gmm: plan (nullable) as below -- t3 / t6 / t2: tiles [0, t3) run three products, [t3, t6) the F6
 * class, [t6, t2) two, the rest one; all zero with delta_p = 0, when no delta images are built --; perm[C] (nullable): the
 * component at each place of the delta images (the identity without them); buffer (nullable): "fx", "bx", "fd" (of
 * pass `pass`), "anchor", "item_model".
 * fb_debug_prepare_ivector: "dg_gc", "dg_miv", "dg_iv" (the diagonalised UBM), "fg_gc", "tri", "fg64", "fgL" (the D = 72
 * Cholesky image; size 0 when not usable), "backend", "backend_offsets" (int64[6], in doubles: mean_vec, ldaT, plda_mean,
 * pldaT, plda_psi, train).
 * fb_debug_prepare_frontend: "blob" (the packed tables), "offsets" (int64[10], in bytes: window, tw_half, tw_full,
 * mel_first, mel_len, mel_off, mel_w, dct, lifter, dscale), "f32" (k_mfcc_f32's table; size 0 when the shape has none). */
typedef struct {
  int mode, NK, NKF, kx, kx2, kacc;
  int n_tiles, n_items, n_groups;
  int delta_p, t3, t6, t2, n_pass, pass_lo[4];
  double delta_rms;
} fb_gmm_plan;
int fb_debug_prepare_gmm(int M, int C, int D, const float *gconsts, const float *means_invvars, const float *inv_vars,
                         fb_gmm_plan *plan, int *perm, const char *buffer, int pass, void *out, int64_t cap, int64_t *size);
int fb_debug_prepare_ivector(const fb_ivector_system *sy, const char *buffer, void *out, int64_t cap, int64_t *size);
int fb_debug_prepare_frontend(const fb_frontend_cfg *c, const char *buffer, void *out, int64_t cap, int64_t *size);
/* fb_debug_prepare_xvector (fb_load_xvector's checks and images): "w<l>" -- layer l's weights as k_xv_affine reads them:
 * uint16 f16 bits [ceil(dout / 32)][ceil(n_ctx * din / 16)][2 terms][64 lanes][8], lane 32 h + c of K step s holding
 * W[32 tile + c][16 s + 8 h .. + 7] * 2^-kw (zero past n_ctx * din and past dout), term 0 = f16(v), term 1 = f16(v - term 0) --,
 * "kw" (int32[n_layers], the layers' powers of two), "segT" (float64 [2 P][R], seg_W transposed), "backend" and
 * "backend_offsets" as for an i-vector system; "wt<l>" -- layer l's weights transposed, as k_wb_xv_affine_t reads them: the
 * same layout for the [n_ctx * din][dout] matrix W', [ceil(n_ctx * din / 32)][ceil(dout / 16)][2 terms][64 lanes][8], lane
 * 32 h + c of K step s holding W[16 s + 8 h .. + 7][32 tile + c] * 2^-kwt --, "kwt" (int32[n_layers]). */
int fb_debug_prepare_xvector(const fb_xvector_system *sy, const char *buffer, void *out, int64_t cap, int64_t *size);

/* The x-vector chain of the loaded system on feature rows handed in as they are (no front end): feats[row_off[B]][D]
 * float32, row_off[B + 1] the utterances' first rows.  layer < n_layers: that frame layer's output, float32
 * [rows][dout]; layer == n_layers: the pooled statistics, float64 [B][2 P]; layer == n_layers + 1: the embeddings,
 * float64 [B][R]. */
int fb_debug_xv_embed(fb_engine *e, const float *feats, const int *row_off, int B, int layer, void *out);
/* White-box gradients through the TDNN (fakebob_hip.h: fb_set_wb_xvector; the switch need not be on for the hooks).
 * fb_debug_xv_backward: the chain on handed-in rows as fb_debug_xv_embed runs it, every layer's ReLU decisions kept, then the
 * backward from the cotangents ebar[B][R] on the embeddings down to `stage`: n_layers + 1 -- the cotangent on the statistics,
 * float64 [B][2 P]; n_layers -- on the last frame layer's output, float32 [rows][P]; l in 1 .. n_layers - 1 -- on the input of
 * layer l, float32 [rows][din_l]; 0 -- on the feature rows, float64 [rows][D].  cap: bytes out holds.
 * fb_debug_xv_masks: the ReLU decisions of frame layer `layer` for the batch scored last with them kept (any white-box call on
 * an x-vector system, fb_debug_xv_backward), bytes [rows][dout], 1 where z > 0; size-then-fill (out NULL: *size only).
 * fb_debug_wb_xv_route: info[FB_WB_XV_ROUTE_N] counts the launches of the TDNN backward the last white-box call (or
 * fb_debug_xv_backward) enqueued; fb_debug_wb_route's keys are as they were (an x-vector system counts its weights under
 * FB_WB_ROUTE_IV_CTL / FB_WB_ROUTE_CTL_REP, the front-end backward and the chain under theirs). */
#define FB_WB_XV_ROUTE_BACKEND_T 0  /* k_wb_iv_backend_t at a replica's embedding */
#define FB_WB_XV_ROUTE_SEGMENT_T 1  /* k_wb_xv_segment_t: once per call, all replicas */
#define FB_WB_XV_ROUTE_POOL_T 2     /* k_wb_xv_pool_t: once per call */
#define FB_WB_XV_ROUTE_ACT_T 3      /* k_wb_xv_act_t: once per frame layer */
#define FB_WB_XV_ROUTE_AFFINE_T 4   /* k_wb_xv_affine_t: once per frame layer */
#define FB_WB_XV_ROUTE_UNSPLICE 5   /* k_wb_xv_unsplice: once per frame layer */
#define FB_WB_XV_ROUTE_N 6
int fb_debug_xv_backward(fb_engine *e, const float *feats, const int *row_off, int B, const double *ebar /*[B][R]*/, int stage,
                         void *out, int64_t cap);
int fb_debug_xv_masks(fb_engine *e, int layer, unsigned char *out, int64_t cap, int64_t *size);
int fb_debug_wb_xv_route(fb_engine *e, int *info);
/* Benchmark hook: the launches of the TDNN backward one by one on rows handed in (the forward with its masks kept and one whole
 * backward first), each `reps` times between device events after one launch to warm up, milliseconds per launch: ms_act[l],
 * ms_affine[l] and ms_unsplice[l] (k_wb_xv_act_t, k_wb_xv_affine_t, k_wb_xv_unsplice of frame layer l), ms_tail[2]
 * (k_wb_xv_segment_t, k_wb_xv_pool_t). */
int fb_bench_xv_backward(fb_engine *e, const float *feats, const int *row_off, int B, int reps, double *ms_act, double *ms_affine,
                         double *ms_unsplice, double *ms_tail);
/* Benchmark hook: the launches of that chain one by one, each `reps` times between device events after one launch to warm
 * up, milliseconds per launch: ms_rowmax[l] and ms_affine[l] (k_xv_rowmax, k_xv_affine of frame layer l), ms_tail[3]
 * (k_xv_pool, k_xv_segment, k_iv_backend). */
int fb_bench_xvector(fb_engine *e, const float *feats, const int *row_off, int B, int reps, double *ms_rowmax, double *ms_affine,
                     double *ms_tail);

/* the GMM kernel the engine scores with, on T rows of D features handed in as they are (no front-end): per-frame
 * log-likelihoods out[m * T + t] of every model (gmm-global-get-frame-likes without --average).  Lets the tests reach
 * inputs the front-end never produces: outliers, huge magnitudes, frames far from every component. */
int fb_debug_gmm_frames(fb_engine *e, const float *feats, int T, double *out);

/* the launches of fb_gmm_acc_stats -- the single-model dump, k_gmm_lse, k_gmm_post_stats -- on T >= 1 rows of D features
 * handed in as they are (no front-end); exactly one diagonal GMM loaded, FB_E_STATE otherwise.  occ[C], F[C][D] as
 * fb_gmm_acc_stats returns them; with `ll` (nullable) the dump matrix, ll[t * C + k] = log-likelihood of row t under
 * component k, without the padding columns of the dump's last 32-component tile.  Lets the tests reach model sizes, row
 * counts and rows the front-end never produces, and compare the dump per component. */
int fb_debug_gmm_acc_rows(fb_engine *e, const float *feats, int T, float *ll, double *occ, double *F);

/* number of UBM components that received posterior mass in the last i-vector batch (only their
 * rows of Sigma^-1 M / U are streamed by the contraction kernels) */
int fb_debug_iv_active(fb_engine *e, int *n_active);
/* gmm-gselect of the last i-vector batch: sel[rows * num_gselect] (nullable), info[6] = {which path ran -- 0: every
 * log-likelihood dumped + k_iv_select, 1: the threshold selection's general form (k_gmm_fx2_sel: lists of survivors), 2: its
 * wide form (k_gsel_w: 16-value records of the groups that reach the threshold) --, the flag (path 1: a list overflowed and
 * the dump redid the batch), most entries of one (row, chunk) list, entries in total, rows, component chunks of the selection
 * kernels (0 on path 0)} */
int fb_debug_iv_gselect(fb_engine *e, int *sel, int64_t sel_cap, int64_t *info);
/* time `reps` back-to-back launches of the GMM log-likelihood kernel on the
 * engine's stream with HIP events over the current device feature buffer
 * (filled by the last score/get_grad call). ms_avg out. */
int fb_bench_gmm_kernel(fb_engine *e, int reps, double *ms_avg, int64_t *rows);
/* run `iters` NES iterations (get_grad + update, early stop disabled) on the
 * device without host round trips; returns elapsed ms (HIP events) and the
 * accumulated time of the GMM kernel alone (events around each launch when
 * time_gmm = 1; time_gmm = 2 with an i-vector system: around k_iv_solve_ll instead of the T-matrix contraction).  warmup < 0: continue the attack the previous call left on the
 * device -- nothing is uploaded or reset, `audio` is ignored (the timed region of
 * bench.py starts with its inputs resident in HBM). */
int fb_bench_nes(fb_engine *e, const fb_nes_params *p, const double *audio,
                 int64_t N, int warmup, int iters, int time_gmm,
                 double *ms_total, double *ms_gmm, int64_t *voiced_rows);
/* read back the attack fb_bench_nes left on the device (read only; it can be continued afterwards):
 * adver[N] the adversarial audio after the last update, scores[B*S] and loss[B] of the last NES batch
 * (row 0 = the unperturbed adversarial audio), summary[3] = {final_loss, adver_loss, distance} of that
 * iteration.  Any output may be NULL. */
int fb_bench_nes_state(fb_engine *e, double *adver, double *scores, double *loss, double *summary);

/* White-box gradients (fakebob_hip.h: "white-box gradients", fb_get_grad_wb / fb_attack_wb).  Each hook runs exactly the
 * launches an attack iteration runs for its stage.
 * fb_debug_gmm_feat_grad: the GMM backward alone on Tv rows of features handed in as they are (float32 [Tv][D]) with weights
 * w[M] = d loss / d raw[m]: out[Tv][D] float64 = (1 / Tv) sum_m w_m sum_c gamma_mtc (means_invvars_mc - inv_vars_mc * x_t).
 * Models with w_m = 0 are skipped; an all-zero w gives exact zeros.
 * fb_debug_frontend_vjp: the front-end backward alone: the forward of fb_debug_feats on wav[n], then the vector-Jacobian
 * product of the cotangent cot[Tv][dim] (float64, on the compacted voiced rows): dwav[n] float64 = d <cot, feats> / d wav in
 * int16 units, and voiced[T] (nullable; 0 / 1), the mask the backward used.  FB_E_NO_VOICED without voiced frames. */
int fb_debug_gmm_feat_grad(fb_engine *e, const float *feats, int Tv, const double *w, double *out);
int fb_debug_frontend_vjp(fb_engine *e, const int16_t *wav, int64_t n, const double *cot, double *dwav, unsigned char *voiced);

/* CW2 (fakebob_hip.h: "CW2", its pseudo-code).  fb_debug_cw2_step runs ONE k_cw2_ctl + k_cw2_step pair of an attack iteration on
 * arrays handed in as they are; no system has to be loaded.  In: the gradient g, the iterate x, a0, w0, mod, m1, m2 (all [N]
 * float64), adver_loss as the loss launch would have left it, the constant c, gbest_l2, the iteration t within its search step
 * (the abort rule of q->abort_every starts from prev = +inf), and p1 = beta1^(t+1), p2 = beta2^(t+1) as the host's repeated
 * multiplication has them.  q: lr, beta1, beta2, adam_eps, abort_every.  Out: the new mod, m1, m2, x_next = tanh(w0 + mod), l2_now of
 * x and l2_next of x_next in the contract's summation order, gate, take, and the best slots -- which start as an attack without a
 * success holds them, the 16-bit cast of a0 and a0, and hold the cast of x and x when take = 1. */
int fb_debug_cw2_step(fb_engine *e, const fb_cw2_params *q, int64_t N, const double *g, const double *x, const double *a0,
                      const double *w0, const double *mod, const double *m1, const double *m2, double adver_loss, double c,
                      double gbest_l2, int t, double p1, double p2, double *mod_out, double *m1_out, double *m2_out, double *x_next,
                      double *l2_now, double *l2_next, int *gate, int *take, int16_t *best_row, double *best_x);

/* Masking (fakebob_hip.h: "masking").  Neither hook needs a loaded system.
 * fb_debug_psy_loss: k_psy_frames and the overlap-add of k_psy_step on a perturbation delta[N] handed in -> D, n_over, gd[N] and
 * (nullable) P[F][K]; m as fb_attack_psy takes it (l2_weight is checked, not used), with its refusals.
 * fb_debug_psy_step: ONE k_psy_ctl + k_psy_step pair as fb_debug_cw2_step runs CW2's, with gd[N] handed in beside g, and D and
 * n_over of x as k_psy_frames would have left them.  Out, beside fb_debug_cw2_step's: dist_now = D + l2_weight * l2_now. */
int fb_debug_psy_loss(fb_engine *e, const fb_psy_params *m, int64_t N, const double *delta, double *D, int *n_over, double *gd,
                      double *P /*[F][K], nullable*/);
int fb_debug_psy_step(fb_engine *e, const fb_cw2_params *q, double l2_weight, int64_t N, const double *g, const double *gd,
                      const double *x, const double *a0, const double *w0, const double *mod, const double *m1, const double *m2,
                      double adver_loss, double c, double D, int n_over, double gbest_dist, int t, double p1, double p2,
                      double *mod_out, double *m1_out, double *m2_out, double *x_next, double *l2_now, double *dist_now,
                      double *l2_next, int *gate, int *take, int16_t *best_row, double *best_x);

/* White-box gradients through a defended victim (fakebob_hip.h: fb_set_wb_bpda).
 * fb_debug_defence_vjp: the defences alone.  The forward of the defences currently set -- input-transform chain, codec -- on
 * the ONE row wav[n] for the engine's r = fb_set_eot replicas at (seed, stream, epoch = iter) of the noise RNG contract, as the
 * scoring call of a white-box iteration runs it; then the transposes alone: dwav[j][n] = the vector-Jacobian product of the
 * cotangent cot[j][n] (on the row the front end would read) through codec and chain of replica j, by the derivative rules of the
 * contract; out[j][n] (nullable) = the transformed row the front end would read.  It runs exactly the launches an attack
 * iteration runs for this stage (an empty chain copies).  The switch need not be on.  FB_E_STATE with an air channel or
 * companions set.  With fb_set_wb_air(e, 1), and only then, an air channel is accepted: the forward is channel, chain, codec,
 * out[j] still the row the front end would read, and dwav[j] = cot[j] through codec, chain (when one is set) and the channel
 * of replica j -- k_air_conv_t's row j, all r in the one launch an iteration runs.
 * fb_debug_wb_route: info[FB_WB_ROUTE_N] counts the launches of the white-box backward the last fb_get_grad_wb* /
 * fb_attack_wb / fb_debug_defence_vjp call enqueued, recorded on the host as fb_debug_nes_route's are. */
#define FB_WB_ROUTE_CTL 0        /* k_wb_ctl: weights from the scores of the one row (+ loop control) */
#define FB_WB_ROUTE_CTL_REP 1    /* k_wb_ctl_rep: weights of one replica of r > 1 (replica 0: + loop control) */
#define FB_WB_ROUTE_BACKWARD 2   /* GMM backward + front-end backward of one replica (seven launches) */
#define FB_WB_ROUTE_CHAIN_T 3    /* k_wb_chain_t: the chain's transpose of one replica, adding it to the gradient */
#define FB_WB_ROUTE_IV_CTL 4        /* k_wb_iv_ctl: an i-vector system's weights (+ loop control) */
#define FB_WB_ROUTE_IV_BACKEND_T 5  /* k_wb_iv_backend_t: the cotangent on the i-vector */
#define FB_WB_ROUTE_IV_SOLVE 6      /* the adjoint solve (k_iv_solve_ll on the copy of the forward's matrix) */
#define FB_WB_ROUTE_IV_STATS_T 7    /* k_wb_iv_stats_t + k_wb_iv_nbar: the stream over Sigma^-1 M and U */
#define FB_WB_ROUTE_IV_POST_T 8     /* k_wb_iv_post_t: the cotangent on the voiced feature rows */
#define FB_WB_ROUTE_N 9
int fb_debug_defence_vjp(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream, int iter,
                         const double *cot /*[r][n]*/, double *dwav /*[r][n]*/, int16_t *out /*[r][n], nullable*/);
int fb_debug_wb_route(fb_engine *e, int *info);

/* White-box gradients through the over-the-air channel (fakebob_hip.h: fb_set_wb_air).
 * fb_debug_air_conv_t: k_air_conv_t alone, ONE launch, on taps handed in as they are -- taps[B][L] int16, any values, L in
 * 2 .. 4096 -- over B rows of n >= 1 samples each: dx[B][n] = 2^-14 * the correlation of cot[B][n] (float64), zeroed where
 * sat[B][n] is non-zero (nullable: nothing saturated), with the row's taps.  The engine's settings are neither used nor changed.
 * fb_debug_air_conv_t_chunk: the samples of dx one workgroup of k_air_conv_t computes (row lengths around its multiples are
 * the kernel's edges).
 * fb_debug_wb_air_route: *n_launches = the k_air_conv_t launches the last fb_get_grad_wb* / fb_attack_wb /
 * fb_debug_defence_vjp / fb_debug_air_conv_t call enqueued -- one per iteration whatever r, none without a channel.  (It is
 * not an index of fb_debug_wb_route: FB_WB_ROUTE_N stays 9.) */
int fb_debug_air_conv_t(fb_engine *e, const int16_t *taps /*[B][L]*/, int B, int L, int64_t n, const double *cot /*[B][n]*/,
                        const unsigned char *sat /*[B][n], nullable*/, double *dx /*[B][n]*/);
int fb_debug_air_conv_t_chunk(void);
int fb_debug_wb_air_route(fb_engine *e, int *n_launches);

/* White-box gradients through feature compression and dither (fakebob_hip.h: fb_set_wb_frontend).
 * fb_debug_feature_compress_vjp: fb_debug_feature_compress (same arguments, same launch) with the kernel's keep outputs on,
 * followed by ONE k_wb_feco_t launch over all B * r rows on cotangents handed in: cots, float64, laid out as the compressed rows
 * -- row R's k_R x D block at out_off[R], k_R = max(1, floor(T_R * ratio)), 0 for an empty row; cot_rows = the rows it holds
 * (FB_E_ARG unless that is the kernel's total).  Returned: out_off[B * r + 1]; labels, one per input row, = the centre (within
 * its utterance row) the frame belonged to when the centres were last written; counts, one per centre, laid out as the
 * compressed rows; xbar, float64, laid out as feats: xbar[t][d] = cots[label[t]][d] / (double) counts[label[t]].
 * fb_debug_wb_feco_route: *n_launches = the k_wb_feco_t launches of the last fb_get_grad_wb* / fb_attack_wb /
 * fb_debug_feature_compress_vjp call -- r per iteration with feature compression on, none otherwise.  (Not an index of
 * fb_debug_wb_route either.) */
int fb_debug_feature_compress_vjp(fb_engine *e, const float *feats, const int *row_off, int B, int r, uint64_t seed,
                                  uint32_t stream, uint32_t epoch, const double *cots, int cot_rows, int *out_off, int *labels,
                                  int *counts, double *xbar);
int fb_debug_wb_feco_route(fb_engine *e, int *n_launches);
/* fb_debug_wb_feco_state: what the forward of the last fb_get_grad_wb* call kept of replica j (0 <= j < the EOT size; with companions rho of K * eot), read
 * before any other scoring call: *Tv voiced rows, *k centres, labels[*Tv], counts[*k]; cap = the ints either array holds
 * (FB_E_ARG when too few).  FB_E_STATE without the switch, the stage and such a call. */
int fb_debug_wb_feco_state(fb_engine *e, int j, int cap, int *labels, int *counts, int *Tv, int *k);

/* White-box gradients of a universal perturbation (fakebob_hip.h: fb_set_wb_universal).
 * fb_debug_wb_compose_t: k_wb_compose_t alone, ONE launch, on arrays handed in as they are: cot[K * eot][n] float64, q[n], a0[n]
 * and comp[K - 1][n] int16 (K = 1: comp is not read), K >= 1, eot >= 1, K * eot <= 32, n >= 1; grad[n] = the sum of the
 * "Composition transposed" rule.  The engine's settings are neither used nor changed.
 * fb_debug_wb_universal_route: *n_launches = the k_wb_compose_t launches the last fb_get_grad_wb* / fb_attack_wb /
 * fb_debug_wb_compose_t call enqueued -- one per iteration with companions set, none at K = 1.  (Not an index of
 * fb_debug_wb_route: FB_WB_ROUTE_N stays 9.) */
int fb_debug_wb_compose_t(fb_engine *e, const double *cot /*[K*eot][n]*/, const int16_t *q, const int16_t *a0,
                          const int16_t *comp /*[K-1][n], nullable at K = 1*/, int K, int eot, int64_t n, double *grad /*[n]*/);
int fb_debug_wb_universal_route(fb_engine *e, int *n_launches);

/* Play offset (fakebob_hip.h: fb_set_play_offset, "Draw", "Composition" and "Transposed rule").
 * fb_debug_compose above applies the offset when one is set -- k_play_compose in front of the air and chain launches, exactly
 * the NES calls' path, at its (seed, stream, epoch) --; N must then exceed S.  With an offset set it returns the rows the front
 * end reads, so a codec (fb_set_codec) IS applied -- behind a chain or a channel in place on their buffer, else in place on the
 * composed buffer; without an offset the hook is unchanged and ignores the codec, as said above.
 * fb_debug_play_offsets: tau_out[B * r], the offset of replica rho of utterance row utt0 + b at slot b * r + rho, under the
 * engine's S (FB_E_STATE without one).
 * fb_debug_play_route: *n_launches = the k_play_compose launches since the last fb_set_play_offset call.
 * fb_debug_wb_play_compose_t: k_wb_play_compose_t alone, ONE launch, on arrays handed in as they are: fb_debug_wb_compose_t's
 * arguments and tau[K * eot], every one below n.  The engine's settings are neither used nor changed.
 * fb_debug_wb_play_route: *n_launches = the k_wb_play_compose_t launches the last fb_get_grad_wb* / fb_attack_wb /
 * fb_debug_wb_play_compose_t call enqueued -- one per iteration with an offset set (fb_debug_wb_universal_route then says
 * none), none without. */
int fb_debug_play_offsets(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt0, int B, int r,
                          uint32_t *tau_out /*[B*r]*/);
int fb_debug_play_route(fb_engine *e, int *n_launches);
/* fb_bench_play_compose: *ms = milliseconds per k_play_compose launch (device events around `reps` launches) on B rows of n
 * samples, K utterances per row (K - 1 companions of a fixed pattern) and eot draws of each, offsets up to n - 1; it writes
 * B * K * eot * n * 2 bytes per launch.  The engine's settings are neither used nor changed. */
int fb_bench_play_compose(fb_engine *e, int B, int64_t n, int K, int eot, int reps, double *ms);
int fb_debug_wb_play_compose_t(fb_engine *e, const double *cot /*[K*eot][n]*/, const int16_t *q, const int16_t *a0,
                               const int16_t *comp /*[K-1][n], nullable at K = 1*/, const uint32_t *tau /*[K*eot]*/, int K, int eot,
                               int64_t n, double *grad /*[n]*/);
int fb_debug_wb_play_route(fb_engine *e, int *n_launches);

/* White-box gradients through the i-vector-PLDA back end (fakebob_hip.h: fb_set_wb_ivector).  Both hooks need a loaded i-vector
 * system (FB_E_STATE otherwise) and run whatever the switch says, with exactly the launches an attack iteration runs for
 * their stage.
 * fb_debug_iv_backend_grad: out[R] = the gradient of sum_s w[s] LLR_s -- the raw LLRs, before the z-norm -- with respect to the
 * i-vector, at ivec[R].
 * fb_debug_iv_feat_grad: <cot, ivec(feats)> differentiated with respect to the Tv feature rows handed in as they are (float32
 * [Tv][D]; cot[R]): the forward's selection, posteriors, statistics and solve on those rows, then the adjoint solve,
 * k_wb_iv_stats_t and k_wb_iv_post_t; out[Tv][D] float64.  fb_debug_iv_gselect and fb_last_ivectors afterwards describe that
 * forward. */
int fb_debug_iv_backend_grad(fb_engine *e, const double *ivec /*[R]*/, const double *w /*[S]*/, double *out /*[R]*/);
int fb_debug_iv_feat_grad(fb_engine *e, const float *feats, int Tv, const double *cot /*[R]*/, double *out /*[Tv*D]*/);

#ifdef __cplusplus
}
#endif
#endif
