// fb_kernels.h -- host-callable launchers of the gfx950 kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fakebob_hip.h"
#include "../../include/fakebob_hip_test.h"
#include "fb_gmm_limits.h"  // FB_FXW_MAX_PASS, FB_FXW_MAX_M, FB_FXW_ANCHORS, FB_GMM_MODE_*: shared with fb_prepare.h

// ---- device-resident front-end tables (built on the host at fb_set_frontend)
struct FbFrontendDev {
  // scalars
  int L, P, shift, nb, nc, dim, order, dwin, cmn_window, snip_edges, remove_dc, use_energy,
      raw_energy, vad_ctx, mfcc_f32;
  double preemph, log_energy_floor;  // log_energy_floor = -inf when disabled
  double vad_thr, vad_mean_scale;
  float vad_prop;
  // tables (device pointers)
  const double *window;   // [L]   povey window (float32 values widened)
  const double *tw_half;  // [P/2][2] exp(-2 pi i m / (P/2))  (complex FFT of size P/2)
  const double *tw_full;  // [P/2+1][2] exp(-2 pi i k / P)    (real-FFT unpack)
  const int *mel_first;   // [nb]
  const int *mel_len;     // [nb]
  const int *mel_off;     // [nb] offset into mel_w
  const double *mel_w;    // packed weights (float32 values widened)
  const double *dct;      // [nc][nb] (float32 values widened)
  const double *lifter;   // [nc]
  const double *dscale;   // [(order+1)][2*order*dwin+1] delta kernels (float32 values widened)
  const float *f32_tab;   // k_mfcc_f32's tables as one float32 blob in its LDS layout (fb_mfcc_f32_table; null: not supported)
  const int *stop;        // nullable device flag: != 0 -> k_mfcc does nothing (attack already stopped)
  int mfcc_cus;           // k_mfcc_f32: compute units the launch may take (0 = all); set per batch by the engine
};

// What a front-end launch carries of the dither RNG contract (include/fakebob_hip.h): Kaldi's --dither, the Philox key
// (seed_lo ^ "DITH", seed_hi ^ stream), counter word 3 and the index of the batch's first utterance within the call
struct FbDitherKey {
  double amp;
  uint32_t k0, k1, epoch, utt0;
};
// The point of the RNG contracts a launch stands at (host side): the dither, noise and feature-compression keys below are
// derived from it at the launch that needs them, each with its own domain constant
struct FbRngPoint {
  uint64_t seed;
  uint32_t stream, epoch, utt0;
};
static inline FbDitherKey fb_dither_key(const FbRngPoint &pt, double amp) {
  return FbDitherKey{amp, (uint32_t)pt.seed ^ 0x44495448u, (uint32_t)(pt.seed >> 32) ^ pt.stream, pt.epoch, pt.utt0};
}
// the normals the dithered MFCC kernels add to frames t0 .. t0 + n_frames - 1 of utterance dk.utt0: z[n_frames][L]
void fb_launch_dither_noise(hipStream_t s, const FbDitherKey &dk, int t0, int n_frames, int L, float *z);

// ---- input-transform chain (fb_set_input_transform; input_transform_kernel.hip) ----------------------------------
#define FB_TF_MAX_STAGES 8
#define FB_TF_MAX_HALO 1024   // largest sum of the stages' radii
#define FB_TF_TILE 4096       // output samples of one workgroup
// the chain as the kernel takes it (by value): H = the sum of the radii, k[s] = the stage's parameter (q, k, L or the
// noise mode), tap_off[s] = where a FIR stage's taps (a noise stage's s or rho) start in the taps buffer
struct FbTfChain {
  int n, H;
  int kind[FB_TF_MAX_STAGES], k[FB_TF_MAX_STAGES], tap_off[FB_TF_MAX_STAGES];
};
// out (the layout of wav: wav_off[B + 1]) = the chain applied to every utterance of wav; n_max = the longest utterance;
// honours `stop` (nullable) like the MFCC kernels.  ch.n == 0 copies.
void fb_launch_input_transform(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                               const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int *stop);
size_t fb_input_transform_lds_bytes(const FbTfChain &ch, bool rnd = false);
// What a randomised / replicating transform launch carries of the noise RNG contract (include/fakebob_hip.h): the Philox
// key (seed_lo ^ "NOIS", seed_hi ^ stream), counter word 3, the row of the batch's first utterance within the call, the
// replicas written per utterance (fb_set_eot) and the per-utterance sums of squares k_tf_power left (SNR stages; else null).
// pre > 0: the input is already replicated (the over-the-air channel wrote it) -- input row R is replica R % pre of
// utterance row R / pre, draws as such, and is written once, to row R (r is not read)
struct FbTfRnd {
  uint32_t k0, k1, epoch, utt0;
  int r;
  const unsigned long long *power;
  int pre;
};
static inline FbTfRnd fb_tf_rnd(const FbRngPoint &pt, int r = 1) {
  return FbTfRnd{(uint32_t)pt.seed ^ 0x4E4F4953u, (uint32_t)(pt.seed >> 32) ^ pt.stream, pt.epoch, pt.utt0, r, nullptr, 0};
}
// power[u] = the exact sum of squares of utterance u of wav (zeroed here, then one integer atomic per tile); honours `stop`
// returns the memset's status
hipError_t fb_launch_tf_power(hipStream_t s, const int16_t *wav, const int64_t *wav_off, int B, int64_t n_max,
                              unsigned long long *power, const int *stop);
// the chain with FB_TF_NOISE stages and / or rn.r replicas per utterance: utterance u of wav (wav_off[B + 1]) is read once
// per tile and replica j written at out_off[u * rn.r + j] of out; an empty chain is a replicating copy
void fb_launch_input_transform_rnd(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                                   const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int64_t *out_off,
                                   const FbTfRnd &rn, const int *stop);
// Companion utterances (fb_set_companions; the "Composition" paragraph of include/fakebob_hip.h): K utterances per NES row
// -- the row itself and comp[K - 1][N] --, a0[N] the int16 cast of the call's original audio.  Every row of the batch is N long.
struct FbTfComp {
  int K;
  int64_t N;
  const int16_t *a0, *comp;
};
// the replicating launch over the composed utterances: NES row b of wav (B rows) is read once per tile and utterance, replica
// rho = c * rn.r + j (utterance c, draw j) written at out_off[b * cn.K * rn.r + rho], its noise stages drawing with replica rho
// and scaling by power[b * cn.K + c] (fb_launch_tf_power_cmp's layout)
void fb_launch_input_transform_cmp(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                                   const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int64_t *out_off,
                                   const FbTfRnd &rn, const FbTfComp &cn, const int *stop);
hipError_t fb_launch_tf_power_cmp(hipStream_t s, const int16_t *wav, const int64_t *wav_off, int B, int64_t n_max,
                                  unsigned long long *power, const FbTfComp &cn, const int *stop);
// z[n] = the normals a noise stage adds to samples i0 .. i0 + n - 1 of utterance rn.utt0 (fb_debug_tf_noise)
void fb_launch_tf_noise(hipStream_t s, const FbTfRnd &rn, int replica, int stage, int64_t i0, int64_t n, float *z);

// ---- play offset (fb_set_play_offset; play_offset_kernels.hip) ----------------------------------------------------
// What a launch carries of the "Play offset" contract (include/fakebob_hip.h): the Philox key (seed_lo ^ "PLAY", seed_hi ^
// stream), counter word 3, the row of the batch's first utterance within the call, and S (tau is uniform in 0 .. S)
struct FbPlay {
  uint32_t k0, k1, epoch, utt0, S;
};
static inline FbPlay fb_play_key(const FbRngPoint &pt, int64_t S) {
  return FbPlay{(uint32_t)pt.seed ^ 0x504C4159u, (uint32_t)(pt.seed >> 32) ^ pt.stream, pt.epoch, pt.utt0, (uint32_t)S};
}
// out [B * cn.K * eot][cn.N] (flat, padded to a multiple of eight samples): row b * r' + rho = utterance rho / eot of NES row b
// of q [B][cn.N] as composed under the offset tau[b * r' + rho], which the launch draws and writes too (cn.K == 1: cn.comp is
// not read; cn.N > pk.S).  Honours `stop`.
void fb_launch_play_compose(hipStream_t s, const FbPlay &pk, const int16_t *q, const FbTfComp &cn, int eot, int B, int16_t *out,
                            uint32_t *tau, const int *stop);
// tau[rows], row R = replica R % r of utterance row R / r: the draw alone (fb_debug_play_offsets)
void fb_launch_play_offsets(hipStream_t s, const FbPlay &pk, int r, int rows, uint32_t *tau);
// the composition under offsets transposed, ONE launch: cot [K * eot][n] on the composed rows of the one NES row q [n], the
// offsets tau [K * eot] as the forward drew them -> grad [n], rho ascending (the header's "Transposed rule")
void fb_launch_wb_play_compose_t(hipStream_t s, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp,
                                 const uint32_t *tau, int K, int eot, int64_t n, double *grad, const int *stop);

// ---- over-the-air channel (fb_set_air_channel; air_channel_kernel.hip) -------------------------------------------
// What a launch carries of the channel's contract (include/fakebob_hip.h): the setting (L == 0: no channel), the Philox key
// (seed_lo ^ "AIRC", seed_hi ^ stream), counter word 3, the row of the batch's first utterance within the call and the output
// rows per utterance row (K * eot)
struct FbAir {
  int L, d;
  double amp, rho_lo, rho_hi;
  uint32_t k0, k1, epoch, utt0;
  int r;
};
static inline FbAir fb_air_key(const FbRngPoint &pt, const FbAir &set, int r = 1) {
  return FbAir{set.L, set.d, set.amp, set.rho_lo, set.rho_hi, (uint32_t)pt.seed ^ 0x41495243u, (uint32_t)(pt.seed >> 32) ^ pt.stream,
               pt.epoch, pt.utt0, r};
}
// taps[rows][ac.L]: output row R is utterance row ac.utt0 + R / ac.r, replica rep0 + R % ac.r.  z (nullable): the normals
// [rows][4 * ceil(L / 4)] as drawn; w (nullable): [rows] the decay's words.  Honours `stop`.
void fb_launch_air_taps(hipStream_t s, const FbAir &ac, int rep0, int rows, int16_t *taps, float *z, uint32_t *w, const int *stop);
// out row R (at out_off[R]; R = 0 .. rows - 1) = row R / r of wav (in_off) -- with cn (nullable) utterance (R % r) / eot of
// that row as composed -- convolved with taps[R][L]; n_max = the longest row.  Honours `stop`.
// sat (nullable; laid out as out): one byte per output sample, 1 where the value before the clip lay outside the int16 range
// (k_air_conv<true>; null: the kernel every caller took before the white-box path through the channel existed)
void fb_launch_air_conv(hipStream_t s, const int16_t *wav, const int64_t *in_off, int rows, int r, int eot, int64_t n_max,
                        const int16_t *taps, int L, int16_t *out, const int64_t *out_off, const FbTfComp *cn, const int *stop,
                        unsigned char *sat = nullptr);
size_t fb_air_conv_lds_bytes(int L);
// the channel transposed (fb_set_wb_air; whitebox_air_kernels.hip): dx[rows][n] = 2^-14 * the correlation of cot[rows][n] --
// zeroed where sat[rows][n] (nullable) is set -- with taps[rows][L], one launch for all rows; then grad[n] = the sum of the
// r rows of dx, ascending.  Both honour `stop`.  fb_air_conv_t_chunk: samples of dx per workgroup.
void fb_launch_air_conv_t(hipStream_t s, const double *cot, const unsigned char *sat, int rows, int64_t n, const int16_t *taps, int L,
                          double *dx, const int *stop);
void fb_launch_air_sum_t(hipStream_t s, const double *dx, int r, int64_t n, double *grad, const int *stop);
int fb_air_conv_t_chunk(void);

// ---- telephone-line codec (fb_set_codec; codec_kernel.hip) -------------------------------------------------------
// out row R (at off[R], as in wav; R = 0 .. B - 1) = the round trip of row R of wav through codec `kind` (FB_CODEC_ULAW,
// _ALAW or _ADPCM; the stage contract is in include/fakebob_hip.h); n_max = the longest row.  out == wav is allowed.
// Honours `stop`.
void fb_launch_codec(hipStream_t s, int kind, const int16_t *wav, const int64_t *off, int B, int64_t n_max, int16_t *out, const int *stop);

// ---- feature compression (fb_set_feature_compression; feature_compress_kernel.hip) -------------------------------
// What a launch carries of the stage contract (include/fakebob_hip.h): the setting, the Philox key (seed_lo ^ "FECO",
// seed_hi ^ stream), counter word 3, the row of the batch's first utterance within the call and the replicas per utterance
struct FbFeco {
  double ratio;
  int iters;
  uint32_t k0, k1, epoch, utt0;
  int r;
};
static inline FbFeco fb_feco_key(const FbRngPoint &pt, double ratio, int iters, int r = 1) {
  return FbFeco{ratio, iters, (uint32_t)pt.seed ^ 0x4645434Fu, (uint32_t)(pt.seed >> 32) ^ pt.stream, pt.epoch, pt.utt0, r};
}
#define FB_FECO_WS_INTS 5  // ints of workspace per input row (rows that do not fit the LDS: keys, labels, sorted order, counts, starts)
// k-means over the rows of every utterance row (row_off[rows + 1]; row b * fc.r + j = replica j of utterance b): the centres
// to out, their offsets to out_off[rows + 1]; ws: FB_FECO_WS_INTS ints per input row; t_max: an upper bound of the longest
// row (it sizes the LDS request); honours `stop` (nullable) like the MFCC kernels.  false: the LDS opt-in failed
// keep_label / keep_cnt / keep_k (nullable, the white-box call under fb_set_wb_frontend): the final assignment -- the label of
// every input row (laid out as feats' rows), the member count of every centre (laid out as out's rows), k of every row --,
// written once at the end; with null pointers the results are what they were before the outputs existed
bool fb_launch_feature_compress(hipStream_t s, const FbFeco &fc, int D, const float *feats, const int *row_off, int rows,
                                int t_max, float *out, int *out_off, int *ws, const int *stop, int *keep_label = nullptr,
                                int *keep_cnt = nullptr, int *keep_k = nullptr);
// the stage transposed at that assignment (k_wb_feco_t): xbar[t][d] = cbar[label[t]][d] / (double) count[label[t]] for the rows
// row0 .. row0 + rows - 1 of the batch (in_off: the input rows' offsets, out_off: the centres'; t_max: an upper bound of a
// row's length).  packed: cbar / xbar are laid out as out / feats; else they hold ONE row (rows == 1), from index 0.
// Honours `stop`.
void fb_launch_wb_feco_t(hipStream_t s, int D, const int *label, const int *cnt, const int *in_off, const int *out_off, int row0,
                         int rows, int t_max, bool packed, const double *cbar, double *xbar, const int *stop);
// keys[T] of one (utterance fc.utt0, replica) of the contract (fb_debug_feco_keys)
void fb_launch_feco_keys(hipStream_t s, const FbFeco &fc, int replica, int T, uint32_t *keys);

// ---- NES ----------------------------------------------------------------
// q[b][n] = int16((adver[n] + sigma*noise_b[n]) * 2^15), b in [0, 2*half]; column 0 is the
// un-noised adver.  noise: Philox(seed, iter, stream) or explicit float64 [N][half].
// dist_part[gridDim.x] gets per-block max |audio - adver| (audio nullable).
void fb_launch_perturb(hipStream_t s, const double *adver, const double *audio, int64_t N, int half,
                       double sigma, uint64_t seed, uint32_t iter, uint32_t stream,
                       const double *noise_pos, int16_t *q, double *dist_part, int *n_dist_part,
                       float *zbuf /* nullable: float32 normals [half][N] for the gradient kernel */,
                       const int *stop = nullptr /* nullable: device flag, != 0 -> the launch does nothing */,
                       int bits = 16 /* bits_per_sample of the cast: scale 2^(bits - 1) */);
void fb_launch_perturb_f64(hipStream_t s, const double *adver, const double *audio, int64_t N, int half,
                           double sigma, uint64_t seed, uint32_t iter, uint32_t stream, const double *noise_pos,
                           double *x, double *dist_part, int *n_dist_part, float *zbuf);
// the same batch into a device-resident foreign model's x[B][N] as FB_DT_F32 / FB_DT_F64 (x_vec: x is 16-byte aligned);
// honours `stop` (nullable) like fb_launch_perturb
void fb_launch_perturb_x(hipStream_t s, int x_dtype, const double *adver, const double *audio, int64_t N, int half,
                         double sigma, uint64_t seed, uint32_t iter, uint32_t stream, const double *noise_pos, void *x,
                         int x_vec, double *dist_part, int *n_dist_part, float *zbuf, const int *stop);
// *t = the device's constant-rate clock (wall_clock64) when the stream gets there
void fb_launch_stamp(hipStream_t s, unsigned long long *t);
// plain quantisation of float64 audio (model.score on float input)
void fb_launch_quantize(hipStream_t s, const double *x, int64_t n, int bits, int16_t *q);
// noise dump (tests)
void fb_launch_noise(hipStream_t s, uint64_t seed, uint32_t iter, uint32_t stream, int64_t N, int half,
                     float *z);

// ---- particle-swarm attack (fb_attack_pso; pso_kernels.hip) --------------------------------------------------------
#define FB_PSO_KEY 0x5053574Du   // "PSWM": the swarm's uniforms have a Philox key of their own
#define FB_PSO_MAX_PARTICLES 64  // (the per-particle "improved" flags travel as one 64-bit kernel argument)
// the swarm at t = 0: x, v [P][N] and their int16 cast q [P][N] (the first batch)
void fb_launch_pso_init(hipStream_t s, const double *audio, int64_t N, int P, double eps, double vmax, uint64_t seed,
                        uint32_t stream, int bits, double *x, double *v, int16_t *q);
// the update `t` (= iteration + 1) of every particle, with what the host decided from the iteration's losses riding along:
// pb_p <- x_p where bit p of `improved` is set, gb <- x of particle g_new (-1: gb stays) -- both before the velocities read
// them --, and the int16 cast of the new positions in q [P][N] (the next batch)
void fb_launch_pso_step(hipStream_t s, const double *audio, int64_t N, int P, double eps, double *x, double *v, double *pb,
                        double *gb, unsigned long long improved, int g_new, double w, double c1, double c2, double vmax,
                        uint64_t seed, uint32_t stream, uint32_t t, int bits, int16_t *q);

// ---- decision-only attack (fb_attack_kenansville; kenansville_kernels.hip) ---------------------------------------------
#define FB_KV_MIN_WINDOW 8
#define FB_KV_MAX_WINDOW 128
#define FB_KV_MAX_ROWS 64        // rows of a round (the q list travels as one kernel argument)
#define FB_KV_MAX_ROUNDS 32
// the analysis of x[N] in windows of W (K = W / 2 + 1 bins, nw = ceil(N / W) windows): m a, m b [nw][K], cum [nw][K] in bin
// order, E [nw].  tab: the four tables CF, SF, CI, SI, W entries each, one after the other.
void fb_launch_kv_analyse(hipStream_t s, const int16_t *x, int64_t N, int W, const int32_t *tab, int32_t *ma, int32_t *mb,
                          long long *cum, long long *E);
// the candidates q[0 .. rows) (host array) of x, row j at out + j * N
void fb_launch_kv_candidates(hipStream_t s, const int16_t *x, int64_t N, int W, int rows, const int *q, const int32_t *tab,
                             const int32_t *ma, const int32_t *mb, const long long *cum, const long long *E, int16_t *out);

// ---- decision-only attack II: HopSkipJump (fb_attack_hsj; hsj_kernels.hip) ------------------------------------------
#define FB_HSJ_KEY 0x48534A50u   // "HSJP": the probes' normals have a Philox key of their own (seed_lo ^ key, seed_hi)
#define FB_HSJ_MAX_GRID 64       // rows of a search round or of a step batch (the q list travels as one kernel argument)
#define FB_HSJ_MAX_ROUNDS 32
#define FB_HSJ_MAX_EVALS 1024    // probes of an iteration (the weights sit in LDS)
#define FB_HSJ_Q 1048576         // Q = 2^20: line(y, Q) is the end point
int fb_hsj_chunks(int64_t N);    // chunks of 1024 samples = workgroups = entries of a partial-sum buffer
// rows j = 0 .. rows - 1 at out + j * N: the int16 cast of line(y, q[j]) = a + (q[j] 2^-20) (y - a); q a host array
void fb_launch_hsj_line(hipStream_t s, const double *a, const double *y, int64_t N, int rows, const int *q, int bits,
                        int16_t *out);
// x = line(y, q) in float64, part[c] = the chunk sums of ssq(x - a)
void fb_launch_hsj_adopt(hipStream_t s, const double *a, const double *y, int64_t N, int q, double *x, double *part);
// *out = part[0] + part[1] + ... + part[n - 1] in that order (one workgroup)
void fb_launch_hsj_sum(hipStream_t s, const double *part, int n, double *out);
// rows j = 0 .. B - 1: the int16 cast of clip(x + sigma z_j, -1, 1), z_j = the NES generator's normals of iteration t under
// the probes' key; zkeep (nullable): z as float32 [B][N] as well
void fb_launch_hsj_probes(hipStream_t s, const double *x, int64_t N, int B, double sigma, uint64_t seed, uint32_t stream,
                          uint32_t t, int bits, int16_t *out, float *zkeep);
// v = sum_j w_j z_j (j ascending; k_hsj_dir), then part[c] = the chunk sums of ssq(v) (k_hsj_ssq); w: device int32 [B];
// zkept (nullable): the probes launch's normals instead of drawing them again
void fb_launch_hsj_dir(hipStream_t s, const int32_t *w, int B, int64_t N, uint64_t seed, uint32_t stream, uint32_t t,
                       const float *zkept, double *v, double *part);
// y_m = clip(x + c_m v, -1, 1), c_m = *S_dev > 0 ? (xi 2^-m) / sqrt(*S_dev) : 0: rows != null -- m = m0 .. m0 + count - 1 as
// int16 rows; rows == null -- m = m0 alone, float64, in yout
void fb_launch_hsj_step(hipStream_t s, const double *x, const double *v, const double *S_dev, double xi, int m0, int count,
                        int64_t N, int bits, int16_t *rows, double *yout);

// Device-side control block of an attack (FAKEBOB.py:171-203): early stop on loss[0] < 0 (:181), the
// plateau learning-rate schedule (:195-200) and the per-iteration trace rows are handled by the loss
// kernel itself, so the host can queue several NES iterations ahead and only looks at the block once
// per batch.  Iterations queued behind the stopping one see `stop` and do nothing.
struct FbCtlDev {
  double lr, min_lr, plateau_drop;
  double *ls;  // [plateau_length] recent losses
  int n_ls, plateau_length;
  int stop, broke, stop_iter, iters_done, err, disable_stop;
  int pub_seq;   // the number of the last loss body that has published its results (k_gmm_finalize_loss_update: the
                 // update workgroups of the same launch poll it); the host counts the loss bodies it queues
  int pad_;
  unsigned long long *ticks;  // nullable: [1 + max_iter] device constant-rate clock (wall_clock64): [0] = start of the
                              // attack, [1 + it] = iteration it's loss evaluated -- the per-iteration times of the
                              // reference's trace (FAKEBOB.py:205-212)
};
struct FbNesDev {  // device control/result block of one NES iteration
  double adver_loss, final_loss, distance;
  int err;       // !=0: utterance (err-1) had no voiced frames
  int pad;
  double score0[62];
};
// scores + loss + summary (single block).  raw[B][M] -> scores[B][S] -> loss[B].
// znorm_all != 0 (i-vector systems): S = M and scores = (raw - z_mean)/z_std for every task.
void fb_launch_loss(hipStream_t s, const double *raw, const int *tv, int B, int M, int task, int znorm_all,
                    int attack_type, const double *z_mean, const double *z_std, double threshold,
                    double adver_thresh, int target, int true_label, const double *dist_part,
                    int n_dist_part, double *scores, double *loss, FbNesDev *out, FbCtlDev *ctl = nullptr,
                    double *trace = nullptr, int it = 0);
// ... a foreign model's float32 scores, read from its own buffer and widened exactly
void fb_launch_loss(hipStream_t s, const float *raw, const int *tv, int B, int M, int task, int znorm_all,
                    int attack_type, const double *z_mean, const double *z_std, double threshold,
                    double adver_thresh, int target, int true_label, const double *dist_part,
                    int n_dist_part, double *scores, double *loss, FbNesDev *out, FbCtlDev *ctl = nullptr,
                    double *trace = nullptr, int it = 0);
// the expectation-over-transformation loss (fb_set_eot, r > 1; k_loss_eot): raw[B * r][M] and tv[B * r] of the replicated
// batch (replica j of NES row b = row b * r + j) -> per-replica scores rep_sc[B * r][S] and losses rep_l[B * r] by the
// operations of k_loss, their float64 means over j ascending in scores[B][S] / loss[B], then k_loss's tail on those B rows
void fb_launch_loss_eot(hipStream_t s, const double *raw, const int *tv, int B, int r, int M, int task, int znorm_all,
                        int attack_type, const double *z_mean, const double *z_std, double threshold,
                        double adver_thresh, int target, int true_label, const double *dist_part, int n_dist_part,
                        double *rep_sc, double *rep_l, double *scores, double *loss, FbNesDev *out, FbCtlDev *ctl,
                        double *trace, int it);
// the voted decision of rows scored r times (fb_set_query_eot; k_vote): raw[rows * r][M] and tv[rows * r] of the replicated
// batch -> per-replica scores rep_sc[rows * r][S] by the operations of k_loss, and the look block: votes[rows] (adversarial
// replicas), nodec[rows] (replicas without voiced frames), mean[rows][S] (k_loss_eot's means).  label: a decision value
void fb_launch_vote(hipStream_t s, const double *raw, const int *tv, int rows, int r, int M, int task, int znorm_all,
                    const double *z_mean, const double *z_std, double threshold, int targeted, int label, double *rep_sc,
                    int *votes, int *nodec, double *mean);
// ---- foreign victims of the swarm and the decision-only attacks (fb_attack_*_foreign; foreign_rows_kernel.hip) ----------
// the int16 batch q[rows][N] as the audio a foreign model reads: x[rows][N] of x_dtype (FB_DT_*), x = q * 2^-(bits - 1),
// exact.  16-byte loads and stores when q and x are 16-byte aligned, element by element otherwise
void fb_launch_rows_to_model(hipStream_t s, int x_dtype, const int16_t *q, int rows, int64_t N, int bits, void *x);
// a foreign model's scores[rows][S] of score_dtype -> decisions[rows] by the make_decisions rule and the scores widened to
// float64 (k_decide_foreign)
void fb_launch_decide_foreign(hipStream_t s, int score_dtype, const void *scores, int rows, int S, int task, double threshold,
                              int *decisions, double *scores_out);
// k_grad_update (iteration `next_iter - 1`) + k_perturb (iteration next_iter) in one launch; device-controlled attacks
// with Philox noise and half <= FB_FUSE_MAX_HALF only.  Returns the number of distance partials written.
// threads: 256 or 512 per workgroup of 256 samples (the same bits either way; nes_kernels.hip says which when)
#define FB_FUSE_MAX_HALF 40
#define FB_FUSE_MAX_UPD_WG 192  // update workgroups k_gmm_finalize_loss_update may carry (N <= 49 152 samples; longer audio: k_update_perturb)
// the arguments of k_update_perturb, for the launch that carries it behind the GMM finalisation + loss (below)
struct FbUpdArgs {
  const double *loss;
  int64_t N;
  int half;
  double sigma;
  float *zbuf;
  double momentum, one_minus_m, epsilon;
  const double *audio;
  double *grad_m, *adver;
  uint64_t seed;
  uint32_t next_iter, stream;
  int16_t *q;
  double *dist_part;
  double qscale;
  unsigned long long *xch;  // nullable: B x M exchange slots of the finalising workgroups, every one FB_VAD_SENTINEL between launches
  int *role_ticket;         // nullable (FB_FIN_TICKET=1): k_gmm_finalize_loss_update's arrival ticket (zero between launches); null = roles by blockIdx
};
int fb_launch_update_perturb(hipStream_t s, const double *loss, int64_t N, int half, double sigma, float *zbuf,
                             double momentum, double one_minus_m, double epsilon, const double *audio, double *grad_m,
                             double *adver, const FbCtlDev *ctl, uint64_t seed, uint32_t next_iter, uint32_t stream,
                             int16_t *q, double *dist_part, int bits = 16, int threads = 512);
// ... and with the batch of iteration next_iter written into a device-resident foreign model's x[B][N] (x_dtype FB_DT_*,
// x_vec: x is 16-byte aligned) instead of the int16 batch
int fb_launch_update_perturb_x(hipStream_t s, int x_dtype, const double *loss, int64_t N, int half, double sigma,
                               float *zbuf, double momentum, double one_minus_m, double epsilon, const double *audio,
                               double *grad_m, double *adver, const FbCtlDev *ctl, uint64_t seed, uint32_t next_iter,
                               uint32_t stream, void *x, int x_vec, double *dist_part, int threads = 512);
// grad estimate (numpy-pairwise order) + optional momentum/sign/clip update.
// do_update: 0 = only grad_out; 1 = momentum+update with lr.
void fb_launch_grad_update(hipStream_t s, const double *loss, int64_t N, int half, double sigma,
                           const float *zbuf, const double *noise_pos, double *grad_out, int do_update,
                           double momentum, double one_minus_m, double lr, double epsilon,
                           const double *audio, double *grad_m, double *adver, const FbCtlDev *ctl = nullptr);

// ---- white-box gradients (fb_get_grad_wb / fb_attack_wb; whitebox_kernels.hip) --------------------------------------
// w[M] = d loss / d raw[m] from row 0 of the loss launch's scores[S] (first-maximum subgradients) and, with ctl, FakeBob.attack's
// loop control on out->adver_loss: the stop rule, the plateau rule (the window holds adver_loss), trace row `it`, the clock stamp.
// A launch behind the stopping iteration returns at once, as every launch below does on `stop`
void fb_launch_wb_ctl(hipStream_t s, const double *scores, const FbNesDev *out, int M, int task, int attack_type,
                      const double *z_std, double threshold, int target, int true_label, double *w, FbCtlDev *ctl, double *trace,
                      int it);
// g[t][d] = (1 / Tv) sum_m w[m] sum_c gamma_mtc (miv_mc[d] - iv_mc[d] x_t[d]) on the Tv = *n_rows_ptr (<= rows_cap) rows of feats;
// gc [M][C], miv / iv [M][C][D]: plain float32 parameters; part: [M][rows_cap][D] floats of workspace; models with w[m] == 0
// are skipped, all zero gives exact zeros
void fb_launch_wb_gmm_backward(hipStream_t s, int M, int C, int D, const float *gc, const float *miv, const float *iv,
                               const float *feats, const int *n_rows_ptr, int rows_cap, const double *w, float *part, double *g,
                               const int *stop, const int *row_base_ptr = nullptr);
// grad[n] = scale * d <cot, feats(wav)> / d wav for ONE utterance of n samples / T frames whose MFCC matrix the forward left in
// mfcc; cot [Tv][dim] on the compacted rows.  rank [T] (out: the voiced row of a frame or -1), dcm / ddf [T][dim], dmf [T][nc],
// dxf [T][L]: float64 workspace.  tv_fwd (nullable): the forward's voiced count; *status = 1 if the mask recomputed here counts
// differently.  dk (nullable; fb_set_wb_frontend): the forward's dither -- the frames are recomputed from x + amp z, z the normals
// of utterance dk->utt0 under the dither RNG contract; null or amp = 0 draws nothing
void fb_launch_wb_frontend_vjp(hipStream_t s, const FbFrontendDev &fe, const int16_t *wav, int64_t n, int T, const float *mfcc,
                               const double *cot, const int *tv_fwd, int *rank, double *dcm, double *ddf, double *dmf, double *dxf,
                               double scale, double *grad, int *status, const int *stop, const FbDitherKey *dk = nullptr);
// FAKEBOB.py:193-203 on the gradient vector g with the step size of ctl
void fb_launch_wb_update(hipStream_t s, const double *g, int64_t N, double momentum, double one_minus_m, double epsilon,
                         const double *audio, double *grad_m, double *adver, const FbCtlDev *ctl);

// ---- white-box gradients through a defended victim (fb_set_wb_bpda; whitebox_bpda_kernels.hip) ----------------------
#define FB_WBT_TILE 2048      // samples of dx of one k_wb_chain_t workgroup
// replica j's weights w = w_j / r from its own scores rep_scores[S]; with do_ctl the loop control of k_wb_ctl on `out` and
// mean_scores[S] (the EOT means k_loss_eot left) as well
void fb_launch_wb_ctl_rep(hipStream_t s, const double *rep_scores, const double *mean_scores, const FbNesDev *out, int M, int r,
                          int task, int attack_type, const double *z_std, double threshold, int target, int true_label, double *w,
                          FbCtlDev *ctl, int do_ctl, double *trace, int it);
// grad[n] (accumulate: += , else =) the vector-Jacobian product of cot[n], a cotangent on the chain's output, through the chain
// ch applied to wav[n] as replica `replica` of utterance 0 at rn's point of the noise contract (rn.power: k_tf_power's sum for
// SNR stages).  ch.n == 0 copies / adds.  false: the LDS opt-in failed (nothing was launched)
size_t fb_wb_chain_t_lds_bytes(const FbTfChain &ch);
bool fb_launch_wb_chain_t(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav, int64_t n, const FbTfRnd &rn,
                          int replica, const double *cot, double *grad, int accumulate, const int *stop);

// ---- white-box gradients of a universal perturbation (fb_set_wb_universal; whitebox_universal_kernels.hip) ----------
// the composition of fb_set_companions transposed, ONE launch for the R = K * eot replicas: grad[i] = sum over rho = u * eot + j,
// ascending, float64 from +0.0, of cot[rho][i] where u = 0 or comp[u - 1][i] + q[i] - a0[i] (int32) lies inside
// [-32768, 32767], of +0.0 elsewhere.  cot [R][n], comp [K - 1][n], q / a0 / grad [n]; cot and grad on 16-byte boundaries
void fb_launch_wb_compose_t(hipStream_t s, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp, int K, int eot,
                            int64_t n, double *grad, const int *stop);
// rows[K][n]: the composed rows as the forward's tf_composed forms them (row 0 = q), for the chain's transpose
void fb_launch_wb_compose_rows(hipStream_t s, const int16_t *q, const int16_t *a0, const int16_t *comp, int K, int64_t n, int16_t *rows,
                               const int *stop);

// ---- white-box gradients through the i-vector-PLDA back end (fb_set_wb_ivector; whitebox_iv_kernels.hip) ------------
struct FbIvDev;
// k_wb_ctl for an i-vector system: w[S] = d loss / d raw[s] (every task z-normalises: the 1 / z_std is in w), the same loop control
void fb_launch_wb_iv_ctl(hipStream_t s, const double *scores, const FbNesDev *out, int S, int task, int attack_type,
                         const double *z_std, double threshold, int target, int true_label, double *w, FbCtlDev *ctl, double *trace,
                         int it);
// wbar[R] = d (sum_s w[s] LLR_s) / d ivec at the i-vector ivec[R] (raw LLRs, before the z-norm)
void fb_launch_wb_iv_backend_t(hipStream_t s, const FbIvDev &iv, const double *ivec, const double *w, double *wbar, const int *stop);
// With lam = quad^-1 wbar and ivec the forward's i-vector, for the components of the forward's active list (active[C] = their
// number): fbar[k][D] = (Sigma^-1 M)_k lam and nbar[k] = - lam' U_k w.  npart: fb_wb_iv_uchunks(iv) * C doubles of workspace.
// Entries of the other components are not written
int fb_wb_iv_uchunks(const FbIvDev &iv);
void fb_launch_wb_iv_stats_t(hipStream_t s, const FbIvDev &iv, const int *active, const double *lam, const double *ivec, double *fbar,
                             double *npart, double *nbar, const int *stop);
// g[t][D] = the cotangent on the voiced feature rows t < *n_rows_ptr (<= rows_cap) from the forward's sel / post [rows][nsel]
// row_base_ptr (nullable): the first of the rows within feats / sel / post, when they are a replica's within the batch
void fb_launch_wb_iv_post_t(hipStream_t s, const FbIvDev &iv, const float *feats, const int *n_rows_ptr, int rows_cap, const int *sel,
                            const float *post, const double *fbar, const double *nbar, double *g, const int *stop,
                            const int *row_base_ptr = nullptr);
// k_wb_iv_ctl for replica rho of R > 1 (fb_set_wb_universal; whitebox_universal_kernels.hip): w[S] = the weights of ITS scores
// rep_scores[S], over R; with do_ctl the loop control on `out` and mean_scores[S] (the means k_loss_eot left) as well
void fb_launch_wb_iv_ctl_rep(hipStream_t s, const double *rep_scores, const double *mean_scores, const FbNesDev *out, int S, int R,
                             int task, int attack_type, const double *z_std, double threshold, int target, int true_label, double *w,
                             FbCtlDev *ctl, int do_ctl, double *trace, int it);

// ---- the L2 white-box attack (fb_attack_cw2; cw2_kernels.hip; the device code it shares with the masking attack below:
// ---- cw2_device.h; the host loop both run: tanh_attack, fb_engine.hip) -----------------------------------------------
// Device-side control of a CW2 search step: what k_cw2_ctl (one thread) decides for the element-wise launch behind it
struct FbCw2Dev {
  double c;          // the trade-off constant of the search step
  double gbest_l2;   // the smallest l2 over the successful iterates of the whole attack (+inf: none yet)
  double prev;       // the abort rule's last L (+inf at the start of a search step)
  double l2;         // l2 of the iterate just scored
  int gate;          // adver_loss > 0
  int take;          // this iterate goes to the best slots
  int mode;          // what k_cw2_step does: bit 0 the copy to the best slots, bit 1 the Adam step; 0 = return at once
  int found;         // some iterate of this search step had adver_loss < 0
  int aborted;       // the abort rule ended this search step
  int rows;          // trace rows written since the start of the attack
};
// the start of a search step with constant c: mod = m1 = m2 = 0, x = tanh(w0), l2_part[ceil(N / 256)] of x; found / prev / the
// abort flag and ctl->stop (unless ctl->err) start over
void fb_launch_cw2_reset(hipStream_t s, const double *w0, const double *a0, int64_t N, double c, double *mod, double *m1, double *m2,
                         double *x, double *l2_part, FbCw2Dev *cw, FbCtlDev *ctl);
// l2_part[b] = the sum of (x[n] - a0[n])^2 over block b of 256 consecutive samples, by the tree of cw2_block_sum (cw2_device.h)
void fb_launch_cw2_l2(hipStream_t s, const double *x, const double *a0, int64_t N, double *l2_part);
// gate / take / found / gbest_l2 / the abort rule / trace row cw->rows / the clock stamp, from the loss launch's block and the
// partials of the iterate it scored; a launch behind the stopping one only sets cw->mode = 0
void fb_launch_cw2_ctl(hipStream_t s, const FbNesDev *out, const double *scores, int S, const double *l2_part, int64_t N, FbCw2Dev *cw,
                       FbCtlDev *ctl, double *trace, int t, int abort_every);
// the copy of (row, x) to the best slots when cw->mode says so, then the Adam step on mod with the gradient g = d loss / d x and
// x = tanh(w0 + mod), l2_part of the new x; step_size = lr / (1 - beta1^(t+1)), bc2s = sqrt(1 - beta2^(t+1))
void fb_launch_cw2_step(hipStream_t s, const double *g, const double *a0, const double *w0, int64_t N, double beta1, double beta2,
                        double step_size, double bc2s, double adam_eps, double *mod, double *m1, double *m2, double *x,
                        const int16_t *row, int16_t *best_row, double *best_x, double *l2_part, const FbCw2Dev *cw);

// ---- the psychoacoustic white-box attack (fb_attack_psy; psy_kernels.hip, on cw2_device.h's sums, decisions and Adam step) ----
// Device-side control of a search step: k_cw2_reset starts `cw` over as for CW2; k_psy_ctl decides on dist instead of l2
struct FbPsyDev {
  FbCw2Dev cw;         // as in CW2; gbest_l2 is l2 of the best iterate (the best is chosen on gbest_dist)
  double gbest_dist;   // the smallest dist over the successful iterates of the whole attack (+inf: none yet)
  double dist, D;      // of the iterate just scored: dist = D + l2_weight * l2
  int n_over;          // bins of the iterate just scored with P > theta
  int gbest_n_over;    // n_over of the best iterate
};
// The masking loss of delta = x - a0 (zero past N), one workgroup per frame: W in {512, 1024, 2048}, hop W / 4, F frames.
// tw[W]: cos(2 pi t / W), t < W / 2, then sin(2 pi t / W).  theta_br[F][W]: theta[f][k] at position bitrev(k), +inf where
// k > W / 2.  P = |X|^2 * scale; d_part[f] = sum_k max(P - theta, 0), n_part[f] = #{P > theta}; gf[f][W] = the frame's share of
// dD / d delta with coef = 2 scale / (F K).  P_out [F][W/2+1] and ctl are nullable; behind a stop (ctl->stop) nothing is written.
void fb_launch_psy_frames(hipStream_t s, int W, int F, const double *x, const double *a0, int64_t N, const double *tw,
                          const double *theta_br, double scale, double coef, double *gf, double *d_part, int *n_part, double *P_out,
                          const FbCtlDev *ctl);
// gd[n] = the overlap-add of gf[F][W] at hop W / 4, ascending f (the test hook; k_psy_step does it in passing)
void fb_launch_psy_ola(hipStream_t s, const double *gf, int F, int W, int64_t N, double *gd);
// k_cw2_ctl's decisions with dist = (sum_f d_part[f]) / (F K) + l2_weight * l2; trace row {dist, l2, n_over, adver_loss, c, score0[S]}
void fb_launch_psy_ctl(hipStream_t s, const FbNesDev *out, const double *scores, int S, const double *l2_part, int64_t N,
                       const double *d_part, const int *n_part, int F, int K, double l2_weight, FbPsyDev *ps, FbCtlDev *ctl,
                       double *trace, int t, int abort_every);
// k_cw2_step's update with G = (((c gate) g + gd) + l2_weight (2 (x - a0))) (1 - x x); gd[n] = the overlap-add of gf[F][W] in
// ascending f, or gf[n] itself when F == 0
void fb_launch_psy_step(hipStream_t s, const double *g, const double *gf, int F, int W, const double *a0, const double *w0, int64_t N,
                        double l2_weight, double beta1, double beta2, double step_size, double bc2s, double adam_eps, double *mod,
                        double *m1, double *m2, double *x, const int16_t *row, int16_t *best_row, double *best_x, double *l2_part,
                        const FbPsyDev *ps);

// ---- front-end ------------------------------------------------------------
// MFCC of every frame of a (ragged) batch. wav_off[B+1], frame_off[B+1] device arrays.
// frame_rec: [total_frames][4] int32 = {absolute start sample (int64 in two words), start within the
// utterance, utterance length} (used by the P = 512 kernel instead of a search in frame_off).  Returns the kernel it
// launched: FB_ROUTE_MFCC_R16_* or FB_ROUTE_MFCC_GENERIC (fb_debug_frontend_route)
// dk != nullptr (dk->amp > 0): the dithered form of the same kernel (FB_ROUTE_MFCC_*_DITHER); frame_ut[total_frames][2] =
// {utterance, frame within it} then serves the kernels that read frame records
int fb_launch_mfcc(hipStream_t s, const FbFrontendDev &fe, int melw_n, const int16_t *wav,
                    const int64_t *wav_off, const int *frame_off, const int32_t *frame_rec, int B,
                    int total_frames, float *mfcc, const FbDitherKey *dk = nullptr, const int32_t *frame_ut = nullptr);
// fb_frontend_cfg.mfcc_f32: the float32 kernel (frontend_f32_kernels.hip); false = this configuration is not one it takes
bool fb_mfcc_f32_supported(const FbFrontendDev &fe);
// the float32 table blob of k_mfcc_f32 (its LDS image up to the per-wave buffers) from the float64 host tables
#include <vector>
int fb_mfcc_f32_mel_pieces(const int *mel_len, int nb);  // chunks of 12 weights the filters split into (k_mfcc_f32: <= 64)
std::vector<float> fb_mfcc_f32_table(int L, int nb, int nc, const double *window, const double *tw_half, const double *tw_full,
                                     const int *mel_first, const int *mel_len, const int *mel_off, const double *mel_w, int melw_n,
                                     const double *dct, const double *lifter);
// the launch k_mfcc_f32's launcher chose (fb_debug_launch_shape): compute units it may take, rounds of 16-wave groups, workgroups
struct FbMfccShape { int cus, rounds, blocks; };
// uni_T > 0: every utterance has uni_n samples / uni_T frames and the first one starts at sample uni_base -- a frame's
// record is computed, not loaded (one dependent global round trip less at the head of every wave).  shape (nullable): filled
// in with the launch's geometry when the kernel is launched
// dk / frame_ut: as fb_launch_mfcc
bool fb_launch_mfcc_f32(hipStream_t s, const FbFrontendDev &fe, int melw_n, const int16_t *wav, const int32_t *frame_rec,
                        int total_frames, float *mfcc, int uni_T = 0, int64_t uni_n = 0, int64_t uni_base = 0,
                        FbMfccShape *shape = nullptr, const FbDitherKey *dk = nullptr, const int32_t *frame_ut = nullptr);
// VAD + per-utt voiced ranks.  vrank[f] = rank among voiced frames of its utt or -1; tv[b].
// counter: one device int, zero before the first launch (the kernel leaves it at zero); row_off[B+1]
// = exclusive scan of max(tv, 0), written by the workgroup that finishes last
// Kaldi CompressedMatrix round trip of every utterance's MFCC matrix, in place (t_max: longest utterance, frames)
// returns FB_ROUTE_CM_REGS, _LDS or _GLOBAL: where the longest column's sort keys are kept
int fb_launch_feat_compress(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, float *out, const int *frame_off, int B,
                            int t_max);  // out != mfcc: every workgroup reads the whole input matrix
void fb_launch_vad(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, const int *frame_off, int B,
                   int *vrank, int *tv, int *counter, int *row_off);
// row_off[b] = sum_{b'<b} tv[b'] ; row_off[B] = total
// VAD + deltas + CMVN + voiced-row compaction of a batch whose utterances fit the CMVN window, one launch
// cm_out != nullptr (allowed when fb_vad_delta_cmvn_compresses(t_max)): the kernel also takes fb_launch_feat_compress's
// place -- the round trip on its LDS copy of the matrix, the compressed matrix written to cm_out (may be mfcc itself)
bool fb_vad_delta_cmvn_compresses(int t_max);
bool fb_launch_vad_delta_cmvn(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, const int *frame_off, int B,
                              int t_max, unsigned epoch, int *ticket, unsigned long long *pub, int *tv, int *row_off,
                              float *feats, float *cm_out);
// the same with every utterance split over FB_CMVN_PARTS (4) workgroups (no CompressedMatrix phase): part_sum = exchange
// slots, fb_vad_parts_doubles() 64-bit words, every 32-bit half FB_VAD_SENTINEL32 before the first launch; slot_set =
// launches of this kernel on the buffer since then (its two slot sets alternate with it)
#define FB_VAD_SENTINEL32 0x7ff87ff8u
#define FB_VAD_SENTINEL 0x7ff87ff87ff87ff8ull
size_t fb_vad_parts_doubles(const FbFrontendDev &fe, int B);
bool fb_launch_vad_delta_cmvn_p(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, const int *frame_off, int B,
                                int t_max, unsigned epoch, int *ticket, unsigned long long *pub, int *tv, int *row_off,
                                float *feats, double *part_sum, unsigned slot_set,
                                bool spread = true /* pad the LDS request to one workgroup per CU (an attack alone on the GPU) */);
bool fb_launch_delta_cmvn(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, const int *frame_off,
                          const int *vrank, const int *row_off, int B, int t_max, float *feats);
// add-deltas (one workgroup per 32-frame chunk; chunk_off[B+1] = prefix of ceil(T_b/32)) + per-chunk
// column sums for the CMVN mean
void fb_launch_deltas(hipStream_t s, const FbFrontendDev &fe, const float *mfcc, const int *frame_off,
                      const int *chunk_off, int B, int total_chunks, float *dfeat, double *chunk_sum);
// apply-cmvn-sliding + select-voiced-frames -> compact feats[row][dim]
void fb_launch_cmvn(hipStream_t s, const FbFrontendDev &fe, const float *dfeat, const int *frame_off,
                    const int *chunk_off, const double *chunk_sum, const int *vrank, const int *row_off, int B,
                    int total_chunks, bool any_long, float *feats);

// ---- diagonal GMM -----------------------------------------------------------
struct FbGmmDev {
  int M, C, D, n_tiles, n_items;      // items per tile = groups + models
  const int *item_model;              // [n_items]: -1 = quadratic (Q) item, else model index
  int item_model_host_q_first;        // 1: the item list is exactly {Q, model 0, 1, ..., M-1} (one variance group)
  // bf16x3 variant (k_gmm_bx3): K padded to 16*NK >= D + 3, images [n_tiles][n_items][3][NK][64] x 16 B
  int mode, NK;
  const unsigned int __attribute__((ext_vector_type(4))) * images_bx;
  // f16x2 variant (k_gmm_fx2): K padded to 16*NKF >= D + 1, images [n_tiles][n_items][2][NKF][64] x 16 B;
  // x^2 is scaled by 2^-sq_shift and the quadratic parameters by 2^+sq_shift
  int NKF;
  // power-of-two operand scalings (exact): frames x * 2^kx, x^2 * 2^kx2; the accumulators hold ll * 2^kacc
  int kx, kx2, kacc;
  const unsigned int __attribute__((ext_vector_type(4))) * images_fx;
  // k_gmm_fx2w (one variance group): images [n_tiles][1 + M][2][NKF][64] x 16 B of {Q, base model 0, delta_1 ..
  // delta_{M-1}}, delta_m = (means_invvars, gconst) of model m MINUS the base model's, all times log2 e and without
  // common power-of-two factor: every dimension is balanced by exact powers of two of its own, 2^kd / 2^kq, applied to
  // the frames in the kernel and inversely to the parameters here.  The COMPONENTS are stored sorted by how far the
  // other models moved them from the base model (the order is free under logsumexp), so that the partial products per K
  // chunk a delta item needs fall from tile to tile: tiles [0, delta_t3) are evaluated with 3, [delta_t6, delta_t2)
  // with 2, the rest with 1.  delta_p = the class most tiles use (1 .. 3, 6 = F6; 0: no delta images); anchor = the frames'
  // balancing factors and the components whose log2-likelihoods start the kernel's per-frame reference (layout:
  // fb_gmm_anchor_table; every image of this struct is packed by fb_prepare_gmm.cpp)
  const unsigned int __attribute__((ext_vector_type(4))) * images_fd;
  int delta_p, delta_t3, delta_t2;
  int delta_t6;  // tiles [delta_t3, delta_t6): the F6 class (delta_t3 <= delta_t6 <= delta_t2; fb_gmm_delta_plan, gmm_wide_kernel.hip)
  // passes of k_gmm_fx2w (more than FB_FXW_MAX_M models): pass p scores the base model and the models pass_lo[p] ..
  // pass_lo[p + 1] - 1 from its own image buffer {Q, base, its deltas}; the launcher hands the kernel a copy of this
  // struct with images_fd = pass_images[p] and pass_first = pass_lo[p] (local model m >= 1 is model pass_first + m - 1 of
  // the M the partial sums are laid out for)
  int n_pass, pass_first;
  const unsigned int __attribute__((ext_vector_type(4))) * pass_images[FB_FXW_MAX_PASS];
  int pass_lo[FB_FXW_MAX_PASS + 1];
  const float *anchor;
  const int *stop;  // nullable device flag: != 0 -> the launch does nothing (attack already stopped)
  const int *only_if;  // nullable device flag: == 0 -> the DUMP launch does nothing (the gselect rescue: fb_launch_gsel)
  int text_scores;  // fb_frontend_cfg.text_scores: raw scores through Kaldi's 6-significant-digit text output
  int fxw_sub;      // k_gmm_fx2w: component chunks ONE workgroup scores one after the other (0 / 1: one; 2: the launch of a GPU shared
                    // by three or more attacks -- half as many workgroups as compute units, the same partial sums bit for bit)
};
#ifndef FB_FX_OCC
#define FB_FX_OCC 2  // k_gmm_fx2 workgroups per CU (launch bound and the launch's target block count)

#endif

// hipFuncSetAttribute (the > 64 KiB dynamic-LDS opt-in) is per DEVICE: a process that creates engines on several
// GPUs must repeat it on each.  One bit per device; the calls are idempotent, so a race between two host threads
// on the same device only repeats them.
#include <atomic>
static inline bool fb_device_needs_optin(std::atomic<unsigned long long> &mask, unsigned long long *bit) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  *bit = 1ull << (dev & 63);
  return (mask.load(std::memory_order_acquire) & *bit) == 0;
}


// The geometry of a GMM scoring / dump launch as its launcher chose it (fb_debug_launch_shape; nullable `shape` arguments
// below): the kernel (FB_SHAPE_GMM_*), the component chunks, the chunks one k_gmm_fx2w workgroup scores one after the other
// (after the n_chunks % fxw_sub rule), the grid's chunk dimension, the XCD mapping (0: the plain 2-D grid), the launches
// (k_gmm_fx2w's passes), the frame strips and the fewest / most component tiles of any chunk
struct FbGmmShape { int kernel, n_chunks, sub, grid_chunks, xcd_map, passes, strips, tiles_min, tiles_max; };
// true when fb_launch_gmm runs the one-wave-per-SIMD scoring kernel k_gmm_fx2w (256-frame strips, one round of <= 256
// workgroups): the engine sizes the component chunks for it
bool fb_gmm_use_wide(const FbGmmDev &g);
// gmm_wide_kernel.hip: the launch of k_gmm_fx2w (chunk c scores the component tiles c, c + n_chunks, ...); called by
// fb_launch_gmm
void fb_launch_gmm_wide(hipStream_t s, const FbGmmDev &g, const float *feats, const int *n_rows_ptr, int rows_cap,
                        int n_chunks, float *part_m, float *part_s, FbGmmShape *shape = nullptr);
// part_m/part_s: [n_chunks][M][rows_pad]
void fb_launch_gmm(hipStream_t s, const FbGmmDev &g, const float *feats, const int *row_off_total,
                   int rows_cap, int n_chunks, float *part_m, float *part_s, FbGmmShape *shape = nullptr);
// single model (g.M == 1): ll[row][n_tiles*32] = every component log-likelihood (gmm-gselect input)
void fb_launch_gmm_dump(hipStream_t s, const FbGmmDev &g, const float *feats, const int *row_off_total,
                        int rows_cap, int n_chunks, float *ll, FbGmmShape *shape = nullptr);
// gmm-gselect WITHOUT the dump (round 6; k_gmm_fx2_sel / k_gsel_tau / k_gsel_final, gmm_kernels.hip): single model in
// the FX2 mode.  Workspace: gmax rows_cap x 2 n_tiles floats, tau rows_cap floats, glist rows_cap x n_chunks x cap 64-bit
// keys, gcnt rows_cap x n_chunks ints, flag 1 int (set when any row overflowed its lists: the caller then runs the dump +
// k_iv_select gated on it).  sel[row][nsel] as k_iv_select writes it.  fb_gsel_cap(n_chunks) = list entries per (row, chunk).
bool fb_gsel_applies(const FbGmmDev &g, int nsel, int n_chunks);
int fb_gsel_cap(int n_chunks);
int fb_gsel_chunks(int dump_chunks);   // the selection kernels' own chunk count (a power of two <= 8)
void fb_launch_gsel(hipStream_t s, const FbGmmDev &g, const float *feats, const int *n_rows_ptr, int rows_cap, int n_chunks,
                    int nsel, float *gmax, float *tau, unsigned long long *glist, int *gcnt, int *flag, int *sel);
// the wide form (k_gsel_w / k_gsel_final_w): fb_gsel_wide_chunks() > 0 = it applies, with that many component chunks.  gval:
// rows_cap x 32 n_tiles floats (the dump's buffer serves), gid: rows_cap x 2 n_tiles bytes, gcnt: rows_cap x n_chunks ints.
// No overflow and no rescue: sel[] is final (flag is raised by NaN features only).
int fb_gsel_wide_chunks(const FbGmmDev &g, int nsel, int rows_cap, int target_blocks = 256 /* workgroups the passes aim at */);
void fb_launch_gsel_wide(hipStream_t s, const FbGmmDev &g, const float *feats, const int *n_rows_ptr, int rows_cap, int n_chunks,
                         int nsel, float *gmax, float *tau, float *gval, unsigned char *gid, int *gcnt, int *flag, int *sel,
                         int *cnt /* nullable: fb_iv_bucket_cnt() -- the bucket sort's per-block counts, made here */, int Cpad);
// k_gmm_finalize + k_loss fused (GMM systems in the NES loop): counter = one int, zero before the first launch
void fb_launch_gmm_finalize_loss(hipStream_t s, const FbGmmDev &g, const float *part_m, const float *part_s,
                                 int rows_cap, int n_chunks, const int *row_off, int B, double *raw, int *counter,
                                 const int *tv, int task, int attack_type, const double *z_mean, const double *z_std,
                                 double threshold, double adver_thresh, int target, int true_label,
                                 const double *dist_part, int n_dist_part, double *scores, double *loss, FbNesDev *out,
                                 FbCtlDev *ctl, double *trace, int it, int pub_seq = 0, const FbUpdArgs *upd = nullptr);
// enrolment statistics of a single model from its dump matrix ll[rows][ld]: occ[C], F[C][D] (float64)
void fb_launch_gmm_post_stats(hipStream_t s, int C, int ld, int D, const float *ll, const float *feats,
                              const int *n_rows_ptr, int rows_cap, float *mx, float *inv_sum, double *occ,
                              double *F);
// raw[b][m] = mean over voiced rows of logsumexp (merging the chunk partials)
void fb_launch_gmm_finalize(hipStream_t s, const FbGmmDev &g, const float *part_m, const float *part_s,
                            int rows_cap, int n_chunks, const int *row_off, int B, double *raw);

// ---- i-vector / PLDA ------------------------------------------------------------
struct FbIvDev {
  int C, Cpad, D, R, L, S, lda_cols, nsel, triD, triR;
  float min_post;
  int text_scores;              // see fb_frontend_cfg
  double prior_offset;
  const float *fg_gconsts;      // [C]
  const float *fg_mic;          // [C][D]   means_invcovars
  const float *fg_P;            // [C][triD] inv_covars, packed lower-triangular
  const double *fg64;           // [C][triD + D + 1] float64 image for k_iv_fullcov_t: P with the diagonal halved,
                                //   then means_invcovars, then gconst
  const double *fgL;            // [C][FB_FCM_REC] (D = 72; else null): Cholesky image for k_iv_fullcov_mfma (ivector_kernels.hip)
  const unsigned char *tri_r, *tri_c;  // [triD] row / column of packed element e
  const double *sim;            // [C*D][R] Sigma^-1 M
  const double *u;              // [C][triR]
  const double *mean_vec;       // [R]
  const double *ldaT;           // [lda_cols][L]
  const double *plda_mean;      // [L]
  const double *pldaT;          // [L][L] transposed PLDA transform
  const double *plda_psi;       // [L]
  const double *train;          // [S][L] enrolled i-vectors in PLDA space
};
// What the posterior-solve kernels run BEHIND the solution of an utterance (round 5; fb_iv_tail.h): the back-end
// (ivector-subtract-global-mean | transform-vec | ivector-normalize-length, ivector-plda-scoring: k_iv_backend's body) in
// the workgroup that holds the solution, and -- inside the NES loop -- the loss / loop-control body of k_loss in the
// workgroup that finishes last (arrival counter, left at zero).  backend = 0: the solve kernels stop at the i-vectors
// and the caller launches k_iv_backend / k_loss itself (FB_IV_TAIL=split, shapes the tail does not take).
struct FbIvTail {
  int backend;          // 1: llr[b][s] written by the solving workgroup
  int loss;             // 1 (needs backend): the last arriver runs fb_loss_body<true, true>
  double *llr;          // [B][S]
  int *counter;         // arrivals (one int, zero before the first launch)
  const int *tv;        // voiced frames per row: filled in by run_scoring, behind the front end that may regrow the buffer
  int task, attack_type;
  const double *z_mean, *z_std;
  double threshold, adver_thresh;
  int target, true_label;
  const double *dist_part;
  int n_dist_part;
  double *scores, *loss_out;
  FbNesDev *out;
  FbCtlDev *ctl;
  double *trace;
  int it;
};
// doubles of LDS the tail needs behind the solve's own areas (back-end vectors + the loss body's two buffers)
size_t fb_iv_tail_lds_doubles(const FbIvDev &iv);
// true when the tail's loss part can run fused for a batch of B utterances (numpy's sum as one block: B - 1 <= 128)
bool fb_iv_tail_takes_loss(int B);
void fb_launch_iv_derive(hipStream_t s, int C, int D, int R, const double *M, const double *sinv_packed,
                         double *sim, double *u);
// bucket_ws: fb_iv_bucket_ws_ints() ints of workspace, zero before the first use; pairs / llf: rows_cap * nsel
size_t fb_iv_bucket_ws_ints(const FbIvDev &iv, int rows_cap);
// sel_gate: nullable device flag -- k_iv_select runs only when it is non-zero (sel[] then already holds fb_launch_gsel's
// selection; the gate is its overflow flag)
#define FB_IV_FB 64  // frames per partition block of the bucket sort (k_iv_bucket_count / _fill; k_gsel_final_w's workgroup)
int *fb_iv_bucket_cnt(const FbIvDev &iv, int *bucket_ws);   // where the per-block counts live inside bucket_ws
void fb_launch_iv_select_post(hipStream_t s, const FbIvDev &iv, const float *ll, const float *feats,
                              const int *n_rows_ptr, int rows_cap, int *sel, float *post, int *bucket_ws,
                              int *pairs, float *llf, const int *sel_gate = nullptr, bool run_select = true, bool run_count = true);
// gammaT [C][Bpad], XT [C*D][Bpad]: utterance-minor, zero-padded to Bpad (multiple of 32)
void fb_launch_iv_stats(hipStream_t s, const FbIvDev &iv, const float *feats, const int *row_off, const int *pairs,
                        const int *bucket_ws, const float *post, int B, int Bpad, double *gammaT, double *XT);
void fb_launch_iv_contract(hipStream_t s, const FbIvDev &iv, const double *gammaT, const double *XT, int B,
                           int Bpad, int n_kchunks, int *flags, int *active, int *n_active, double *linp,
                           double *quad, int *fail);
// ivector_solve.hip (k_iv_solve_ll): quad is consumed (factored in place); Aall = B x R right-hand sides + a row of
// R + 64 zeros behind them
void fb_launch_iv_solve_ll(hipStream_t s, const FbIvDev &iv, const double *quad, const double *linp, int n_kchunks,
                           int B, double *Aall, double *LinvAll, double *ivec, int *fail, const FbIvTail &tail);
// k_iv_solve_rw: the same system with the block rows of a matrix dealt over five workgroups (up-looking Cholesky); false
// = B x 5 workgroups are more than the chip holds at once (the caller runs fb_launch_iv_solve_ll).  LinvAll: TWO slot
// sets (fb_iv_solve_rw_linv_doubles), every 64-bit word 0x7ff87ff87ff87ff8 before the first launch and whenever `epoch`
// restarts; prog: fb_iv_solve_rw_prog_words() unsigned, zero then; ticket: one int, zero
size_t fb_iv_solve_rw_linv_doubles(const FbIvDev &iv, int B);
size_t fb_iv_solve_rw_prog_words(const FbIvDev &iv, int B);
bool fb_launch_iv_solve_rw(hipStream_t s, const FbIvDev &iv, const double *quad, const double *linp, int n_kchunks, int B,
                           double *Aall, double *LinvAll, double *ivec, int *fail, unsigned *prog, int *ticket, unsigned epoch,
                           const FbIvTail &tail);
void fb_launch_iv_backend(hipStream_t s, const FbIvDev &iv, const double *ivec, int B, double *llr);

// ---- x-vector (TDNN) system (xvector_kernels.hip; the "x-vector" section of fakebob_hip.h) ------------------------
struct FbXvLayerDev {
  int din, dout, n_ctx, ctx[FB_XV_MAX_CTX];
  int K, n_steps;            // n_ctx * din, ceil(K / 16)
  int kw;                    // the image holds W * 2^-kw
  const unsigned short *w;   // fb_xv_frag_index images, one per column tile of 32 channels (fb_prepare.h)
  const float *bias, *scale, *offset;
  int nt_steps, kwt;         // the transposed image (white-box backward): ceil(dout / 16) K steps, W' * 2^-kwt
  const unsigned short *wt;  // ... one image per tile of 32 of the K columns
};
struct FbXvDev {
  int D, n_layers, P, R, max_width;
  FbXvLayerDev layer[FB_XV_MAX_LAYERS];
  const double *segT;        // [2 P][R]
  const double *seg_bias;    // [R]
};
// rowinfo[row] = {first row, rows} of the utterance the row belongs to, for the rows below row_off[B] (rows_cap bounds them)
void fb_launch_xv_rowinfo(hipStream_t s, const int *row_off, int B, int2 *rowinfo);
// amax[row] = max |x[row][0 .. din)|
void fb_launch_xv_rowmax(hipStream_t s, const float *x, int din, const int *n_rows_ptr, int rows_cap, float *amax);
// one frame layer: y[row][dout] from x[row][din] (k_xv_affine); mask (nullable): mask[row][dout] = 1 where the layer's own
// float32 z = W . splice + bias was > 0, else 0 (what the white-box backward differentiates the ReLU by)
void fb_launch_xv_affine(hipStream_t s, const FbXvLayerDev &ly, const float *x, const float *amax, const int2 *rowinfo,
                         const int *n_rows_ptr, int rows_cap, float *y, unsigned char *mask = nullptr);
// stats[b][2 P] = {mean, std} over the utterance's rows of h[row][P]
void fb_launch_xv_pool(hipStream_t s, const float *h, int P, const int *row_off, int B, double *stats);
// emb[b][R] = segT' stats[b] + seg_bias
void fb_launch_xv_segment(hipStream_t s, const FbXvDev &xv, const double *stats, int B, double *emb);
// ---- the TDNN's backward (whitebox_xv_kernels.hip; fb_set_wb_xvector in fakebob_hip.h).  stop (nullable): a set flag skips
// the launch's work.  Rows are the batch's voiced rows, row_off / rowinfo the forward's.
// sbar[b][2 P] = seg_W' ebar[b]: the cotangent on the statistics from the one on the embedding (float64)
void fb_launch_wb_xv_segment_t(hipStream_t s, const FbXvDev &xv, const double *ebar, int B, double *sbar, const int *stop);
// ybar[row][P] (float32) = mbar / T + sbar (h - mean) / (T std) where the variance floor is not active: the cotangent on the
// last frame layer's output h from the one on its statistics
void fb_launch_wb_xv_pool_t(hipStream_t s, const float *h, int P, const int *row_off, int B, const double *stats, const double *sbar,
                            float *ybar, const int *stop);
// zbar[row][dout] = ybar * bn_scale * mask, and amax[row] = max |zbar[row]|
void fb_launch_wb_xv_act_t(hipStream_t s, const FbXvLayerDev &ly, const float *ybar, const unsigned char *mask, const int *n_rows_ptr,
                           int rows_cap, float *zbar, float *amax, const int *stop);
// G[row][K] = sum_c zbar[row][c] W[c][.] on the matrix cores (k_wb_xv_affine_t)
void fb_launch_wb_xv_affine_t(hipStream_t s, const FbXvLayerDev &ly, const float *zbar, const float *amax, const int *n_rows_ptr,
                              int rows_cap, float *G, const int *stop);
// the splice transposed: xbar[t'][din] = sum_j sum_{t : clamp(t + ctx[j]) = t'} G[t][j din + .], j then t ascending, float64
// sums rounded once.  out32 (layers above 0): [row][din] float32.  out64 (layer 0): utterance b's row t' at
// out64[(b * cap64 + t') * din], float64 -- b found from row_off[0 .. B]
void fb_launch_wb_xv_unsplice(hipStream_t s, const FbXvLayerDev &ly, const float *G, const int2 *rowinfo, const int *row_off, int B,
                              const int *n_rows_ptr, int rows_cap, float *out32, double *out64, int cap64, const int *stop);
