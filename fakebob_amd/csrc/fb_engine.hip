// fb_engine.hip -- host side of libfakebob_hip.so: engine state, device buffers and the C ABI (include/fakebob_hip.h).
//
// The tables a model or a front-end configuration needs on the device are computed by the GPU-free unit fb_prepare.h
// (fb_prepare_gmm.cpp, fb_prepare_ivector.cpp, fb_prepare_frontend.cpp).  The loaders here -- fb_load_gmm,
// fb_load_ivector, fb_set_frontend -- validate their arguments, read the environment, prepare on the host, and only
// then synchronise the stream, ensure every buffer, upload and assign the engine's fields: a call refused for its
// arguments or its environment leaves the engine and the device exactly as they were.
//
// One engine = one GPU + one HIP stream.  A NES iteration is a fixed chain of
// launches on that stream with a single 8-byte-aligned result block copied back
// through pinned memory; nothing else crosses PCIe inside the attack loop.
#include <float.h>
#include <algorithm>
#include <atomic>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "fb_kernels.h"
#include "fb_prepare.h"

static thread_local std::string g_err;
static int fb_fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t _e = (x);                                                                           \
    if (_e != hipSuccess)                                                                          \
      return fb_fail(FB_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define FBCHK(x)            \
  do {                      \
    int _r = (x);           \
    if (_r != FB_OK) return _r; \
  } while (0)

extern "C" const char *fb_last_error(void) { return g_err.c_str(); }
extern "C" int fb_version(void) { return 103; }
extern "C" int fb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// A device allocation and its owner: freed when the buffer goes out of scope (with its engine, or at the end of the call
// that made a temporary one); moving hands the allocation over and leaves the source empty
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return FB_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return fb_fail(FB_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    cap = want;
    return FB_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct fb_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int time_gmm = 0;            // bench: 1 = events around the GMM launch / the T-matrix contraction, 2 = around k_iv_solve_ll
  int fuse_opt = -1;           // fb_set_fused_chain: 1 / 0, -1 = the FB_NO_FUSE environment variable decides
  bool gmm_pending = false;
  double gmm_ms_acc = 0.0;
  int64_t gmm_launches = 0;
  // front-end
  bool have_fe = false;
  fb_frontend_cfg cfg;
  FbFrontendDev fe;
  int melw_n = 0;  // packed mel weight count
  DevBuf fe_tables, fe_tables32;
  // Kaldi's dither (cfg.dither > 0; the "Dither RNG contract" of fakebob_hip.h)
  uint64_t dither_seed = 0;     // fb_set_dither_seed: the seed of scoring calls outside an attack (scoring_call_point)
  uint32_t dither_serial = 0;   // ... and their epoch: scoring calls since it was set
  DevBuf frame_ut;              // [total_frames][2] {utterance, frame within it} of the batch (prepare_batch, dither > 0)
  std::vector<int32_t> h_frame_ut;
  // input-transform chain (fb_set_input_transform): tf.n == 0 -- none, launch_mfcc reads `wav` itself
  FbTfChain tf = {};
  DevBuf tf_taps;               // the FIR stages' taps, one after the other
  DevBuf wav_tf;                // the transformed batch, in wav's layout: what the MFCC reads when a chain is set
  // randomised stages and expectation over transformation (FB_TF_NOISE, fb_set_eot; the "Noise RNG contract" of fakebob_hip.h)
  DevBuf tf_power;              // k_tf_power's per-utterance sums of squares (chains with an SNR stage)
  int eot = 1;                  // fb_set_eot: replicas of every NES row (1: none)
  DevBuf eot_sc, eot_l;         // k_loss_eot's per-replica scores [B * r][S] and losses [B * r]
  int query_quorum = FB_QUORUM_OFF;  // fb_set_query_eot: 0 off | -1 majority | 1 .. 32
  DevBuf vote_look;             // k_vote's look block {votes[rows], nodec[rows], mean[rows][S]}
  // over-the-air channel (fb_set_air_channel; its contract is in fakebob_hip.h): air.L == 0 -- none
  FbAir air = {};               // the setting (the key fields are filled per launch: fb_air_key)
  DevBuf wav_air;               // the channel's output, in the replicated layout: what the chain -- or, without one, the MFCC -- reads
  DevBuf air_taps;              // k_air_taps' responses [rows][L] int16
  // telephone-line codec (fb_set_codec; its contract is in fakebob_hip.h): FB_CODEC_NONE -- none
  int codec = FB_CODEC_NONE;
  DevBuf wav_codec;             // k_codec's output when nothing in front of it wrote a buffer of its own (the source is e->wav)
  // companion utterances (fb_set_companions; the "Composition" paragraph of fakebob_hip.h): comp_K1 == 0 -- none
  int comp_K1 = 0;              // companions set; with the call's own utterance K = comp_K1 + 1
  int64_t comp_N = 0;           // ... their length
  DevBuf comp_wav, comp_a0;     // the companions [K1][N] and the int16 cast of the call's original audio [N] (cast once per call)
  // play offset (fb_set_play_offset; the "Play offset" section of fakebob_hip.h): play_S == 0 -- none
  int64_t play_S = 0;           // every replica's perturbation is rotated by a tau of its own, uniform in 0 .. play_S
  DevBuf wav_play, play_tau;    // k_play_compose's rows [B * r'][N] (padded to eight samples) and its offsets [B * r']
  int play_launches = 0;        // k_play_compose launches since fb_set_play_offset (fb_debug_play_route)
  int wb_play_launches = 0;     // k_wb_play_compose_t launches of the last white-box call (fb_debug_wb_play_route)
  // feature compression (fb_set_feature_compression; the stage contract of fakebob_hip.h): feco_iters == 0 -- off, the back
  // end reads `feats` / `row_off` as the front end wrote them
  double feco_ratio = 0.0;
  int feco_iters = 0;
  DevBuf feats_fc, row_off_fc;  // the compressed rows and their offsets: they swap roles with feats / row_off behind the launch
  DevBuf feco_ws;               // FB_FECO_WS_INTS ints per input row: the arrays of rows that do not fit the LDS
  // gmm
  bool have_gmm = false;
  FbGmmDev gmm;
  DevBuf gmm_items, gmm_images_bx, gmm_images_fx, gmm_images_fd, gmm_images_fd2, gmm_images_fd3, gmm_anchor;  // (fd, fd2, fd3: the delta images of k_gmm_fx2w's passes)
  double gmm_delta_rms = 0.0;  // fb_load_gmm's shift statistic behind gmm.delta_p
  int n_groups = 0;
  // i-vector system (kind == 1): the diagonalised UBM lives in `gmm` (M = 1)
  int kind = 0;   // 0 = GMM-UBM, 1 = i-vector/PLDA, 2 = x-vector/PLDA
  int n_out = 0;  // columns of `raw`: models (GMM) or enrolled speakers (i-vector, x-vector)
  // x-vector system (kind == 2): the layers in `xv`, the back end in the back-end fields of `iv` (the others stay unset), the
  // embeddings in iv_ivec; `gmm` holds a one-component placeholder so that what sizes the batch by it keeps working
  FbXvDev xv;
  DevBuf xv_w[FB_XV_MAX_LAYERS], xv_par, xv_seg;   // weight images; bias / scale / offset of every layer; segT + seg_bias
  DevBuf xv_rowinfo, xv_amax, xv_act[2], xv_stats;
  // white-box gradients through the TDNN (fb_set_wb_xvector)
  int wb_xvector = 0;                  // the switch: 0 (as created) refuses an x-vector system, as before it existed
  DevBuf xv_mask[FB_XV_MAX_LAYERS];    // the ReLU decisions of the batch scored last with FbScoreCall::keep_xv_mask: [row][dout] bytes
  int xv_mask_B = 0;                   // ... its utterances (0: none kept); its rows are row_off[B] of that call
  DevBuf xv_mask_rows;                 // ... that count, copied on the device behind the forward (row_off is reused)
  DevBuf wb_xv_ebar, wb_xv_sbar;       // cotangents on the embeddings [r][R] and on the statistics [r][2 P], float64
  DevBuf wb_xv_y[2], wb_xv_z, wb_xv_G, wb_xv_amax;   // float32: cotangents between layers (ping-pong), zbar, G [rows][K], max |zbar| per row
  DevBuf wb_xv_g;                      // float64 cotangent on the feature rows: utterance b's row t at (b * T + t) * D
  int wb_xv_route[FB_WB_XV_ROUTE_N] = {};   // launches of the TDNN backward the last call enqueued (fb_debug_wb_xv_route)
  FbIvDev iv;
  DevBuf iv_fg, iv_fg64, iv_fgL, iv_tri, iv_sim, iv_u, iv_backend;
  DevBuf iv_ll, iv_sel, iv_post, iv_gamma, iv_X, iv_linp, iv_quad, iv_A, iv_linv, iv_ivec, iv_fail, iv_active, iv_bws, iv_pairs, iv_llf;
  int iv_kchunks = 96;
  int iv_Bpad = 0;  // padding of the transposed statistics currently zero-initialised
  int iv_zeroC = -1;  // ... for this component count (position of the zero rows)
  int iv_A_B = -1;    // batch size the zero row behind iv_A was laid out for
  DevBuf iv_prog, iv_ticket;  // k_iv_solve_rw: progress words, ticket
  DevBuf iv_tail_counter;     // arrivals of the solve kernels' fused tail (fb_iv_tail.h)
  DevBuf gs_max, gs_tau, gs_list, gs_cnt, gs_flag, gs_gid;  // fb_launch_gsel's workspace (group maxima, thresholds, survivor lists, overflow flag; wide form: group ids)
  int gs_last_chunks = 0, gs_last_path = 0;  // the last i-vector batch: chunk count of the selection kernels, 0 dump / 1 k_gmm_fx2_sel / 2 k_gsel_w
  unsigned iv_rw_epoch = 0;
  int iv_rw_B = -1, iv_rw_R = -1;
  bool iv_linv_dirty = false;  // k_iv_solve_ll used the slot buffer as plain scratch: refill before k_iv_solve_rw polls it
  // system
  int task = FB_TASK_OSI;
  DevBuf zmean, zstd;
  std::vector<double> h_zmean, h_zstd;
  // batch scratch
  DevBuf frame_rec, vad_counter, vad_pub, vad_part, fin_counter, fin_xch, ctl, ctl_ls, trace_dev, ticks, enr_ll, enr_aux, enr_stats;
  std::vector<double> iter_seconds;  // per-iteration device times of the last fb_attack / fb_attack_ext / fb_attack_dev (fb_attack_pso: host times)
  int nes_route[FB_NES_ROUTE_N] = {};  // fb_debug_nes_route: launches the last fb_get_grad* / fb_attack* call enqueued
  fb_foreign_path_info foreign = {};  // fb_debug_foreign_path: the last foreign-model call (path 0: none yet)
  long long bench_it = -1;  // fb_bench_nes: next iteration index of the attack left resident (-1: none)
  int64_t bench_N = 0;
  int bench_B = 0;
  long long pre_iter = -1;  // >= 0: wav / zbuf / dist_part already hold the NES batch of this iteration (k_update_perturb)
  int pre_ndp = 0;
  // fb_debug_nes_batch: the NES batch the launches of the last fb_get_grad* / fb_attack* / fb_bench_nes call left in wav /
  // zbuf, recorded on the host as they are enqueued (`queued`) and published (`iter`) when the call has succeeded
  struct {
    long long iter = -1;    // Philox iteration index of the resident rows (-1: none; reset wherever bench_it is)
    long long queued = -1;  // ... of the batch launch enqueued last
    int64_t N = 0;
    int half = 0;
    bool q = false, z = false;  // wav holds its int16 rows (the engine's own systems), zbuf its normals (Philox noise)
  } nes_rec;
  int vad_part_B = -1, vad_part_dim = -1;  // slot layout the sentinel-filled exchange buffer of k_vad_delta_cmvn_p was prepared for
  int ctl_seq = 0;         // loss bodies queued on the control block since its reset (FbCtlDev::pub_seq)
  unsigned vad_epoch = 0;  // launches of the fused VAD/CMVN kernels on vad_pub (its published counts carry the epoch)
  bool fin_xch_clean = false;  // fin_xch holds sentinels everywhere (k_gmm_finalize_loss_update's exchange slots)
  unsigned vad_p_launches = 0;  // launches of k_vad_delta_cmvn_p on vad_part since its sentinel fill (its slot sets alternate with them)
  FbCtlDev *h_ctl = nullptr;  // pinned
  // attack_loop without the drain between looks: the control block of batch n lands in h_look[n & 1] and ev_look[n & 1] says
  // when, while batch n + 1 is already queued; what the host has read is then copied into h_ctl
  FbCtlDev *h_look[2] = {nullptr, nullptr};  // pinned
  hipEvent_t ev_look[2] = {nullptr, nullptr};
  // two banks of event pairs: the launches of the batch being queued record into bank evg_cur while the other bank's batch
  // may still be running
  hipEvent_t evg_ring[2][2 * 16] = {};
  int evg_n[2] = {0, 0};
  int evg_cur = 0;
  int t_max = 0;
  std::vector<int32_t> h_frame_rec;
  int uni_T = 0;        // frames per utterance when every utterance of the batch has the same length (NES batches), else 0
  int64_t uni_n = 0;    // ... and that length
  DevBuf wav, wav_off, frame_off, chunk_off, chunk_sum, mfcc, mfcc_cm, vrank, tv, row_off, dfeat, feats, part_m, part_s, raw;
  std::vector<int64_t> h_wav_off;
  std::vector<int> h_frame_off, h_chunk_off;
  bool any_long = false;  // some utterance has T > cmn_window
  int route[5] = {};      // fb_debug_frontend_route: what the last batch's front end ran
  bool have_route = false;  // ... once a batch has reached the MFCC launch
  FbGmmShape shape_gmm = {};    // fb_debug_launch_shape: the geometry of the last batch's GMM launch (the launchers fill it in)
  FbMfccShape shape_mfcc = {};  // ... and of its k_mfcc_f32 launch
  int shape_upd_threads = 0;    // ... and the threads per workgroup of the update launch that followed it (0: none did)
  bool have_shape = false;      // ... once a batch has chosen its launch shape
  int cached_B = -1;
  int64_t cached_N = -1;
  int last_total_frames = 0, last_B = 0, last_chunks = 1;
  // NES state
  DevBuf audio, adver, grad_m, grad, noise, zbuf, scores, loss, dist_part, nes_out, stage_f64, ext_x, ext_z;
  DevBuf pso_x, pso_v, pso_pb, pso_gb;  // fb_attack_pso's swarm: positions, velocities, personal bests [P][N], global best [N]
  DevBuf pso_look;                      // ... and what its host reads per iteration: {FbNesDev, loss[P], scores[P][S]}
  DevBuf kv_x, kv_best, kv_tab;         // fb_attack_kenansville: the int16 cast of the audio [N], the candidate of hi [N], the four tables [4][W]
  DevBuf kv_ma, kv_mb, kv_cum, kv_E;    // ... the analysis: m a, m b [nw][K] int32, cum [nw][K] and E [nw] int64
  DevBuf kv_look;                       // ... and what its host reads per round: {FbNesDev, loss[G], scores[G][S], tv[G]}
  DevBuf hsj_init, hsj_y, hsj_x, hsj_v; // fb_attack_hsj: the starting audio, the step's end point, the boundary point, the direction [N] float64
  DevBuf hsj_part, hsj_sc, hsj_w;       // ... ssq's chunk sums, the two sums {D2, S}, the probes' weights [B] int32
  DevBuf hsj_best, hsj_look, hsj_z;     // ... the row of hi [N] int16, the host's look {FbNesDev, loss, scores, tv}, the probes' normals [B][N] float32
  DevBuf fg_look;                       // fb_attack_*_foreign: k_decide_foreign's look block {decisions[rows] int32, scores[rows][S] float64}
  // white-box gradients (fb_get_grad_wb / fb_attack_wb): fb_load_gmm's plain float32 parameters, kept on the host and uploaded
  // by the first white-box call after the load; the weights w[M], the GMM backward's per-model rows and the cotangent g on the
  // compacted rows, the front-end backward's float64 stages, a status word (1: the recomputed voiced mask is not the forward's)
  std::vector<float> h_wb_gc, h_wb_miv, h_wb_iv;
  bool wb_uploaded = false;
  DevBuf wb_gc, wb_miv, wb_iv, wb_w, wb_part, wb_g, wb_rank, wb_dcm, wb_ddf, wb_dmf, wb_dxf, wb_status;
  // white-box gradients through a defended victim (fb_set_wb_bpda)
  // white-box gradients through the i-vector-PLDA back end (fb_set_wb_ivector)
  int wb_ivector = 0;                  // the switch: 0 (as created) refuses an i-vector system, as before it existed
  DevBuf wb_iv_quad, wb_iv_A, wb_iv_linv, wb_iv_fail;   // the adjoint solve: the forward's matrix, k_iv_solve_ll's workspace
  DevBuf wb_iv_wbar, wb_iv_lam, wb_iv_fbar, wb_iv_nbar, wb_iv_npart;   // wbar [R], lambda [R], Fbar [C][D], Nbar [C], partials
  int wb_iv_A_R = -1;
  int wb_bpda = 0;                     // the switch: 0 (as created) refuses every defence, as before it existed
  DevBuf wb_gj;                        // one replica's cotangent on the row the front end read [N]
  const int16_t *fe_wav = nullptr;     // the int16 batch the last launch_mfcc handed to the front end (a device buffer of the engine's)
  int wb_route[FB_WB_ROUTE_N] = {};    // launches of the white-box backward the last call enqueued (fb_debug_wb_route)
  // the L2 white-box attack (fb_attack_cw2): w0, mod, the second moment (the first lives in grad_m) and the best iterate
  // [N] float64, the best int16 row [N], the L2 partials [ceil(N / 256)], the search step's control block
  DevBuf cw2_w0, cw2_mod, cw2_m2, cw2_best_x, cw2_best_row, cw2_l2part, cw2_ctl;
  // the psychoacoustic attack (fb_attack_psy; it borrows the CW2 buffers above): the twiddle table [W] of psy_tw_W, the
  // threshold in bit-reversed order [F][W], the frames' gradients [F][W], their hinge and count partials [F], P [F][K] (the
  // test hook), the search step's control block
  DevBuf psy_tw, psy_theta, psy_gf, psy_dpart, psy_npart, psy_P, psy_ctl;
  int psy_tw_W = 0;
  // white-box gradients through the over-the-air channel (fb_set_wb_air)
  int wb_air = 0;                     // the switch: 0 (as created) refuses a channel, as before it existed
  DevBuf wb_air_cot, wb_air_dx;        // the replicas' cotangents on the channel's output [r][N], k_air_conv_t's output [r][N] (r > 1)
  DevBuf wb_air_sat;                   // the forward's saturation bytes, laid out as wav_air (k_air_conv<true>)
  int wb_air_launches = 0;             // k_air_conv_t launches of the last call (fb_debug_wb_air_route)
  // white-box gradients through feature compression and dither (fb_set_wb_frontend)
  int wb_frontend = 0;                 // the switch: 0 (as created) refuses both, as before it existed
  DevBuf wb_feco_label, wb_feco_cnt;   // the forward's final assignment: label per voiced row (laid out as feats_fc after the swap: the
                                       // input rows), member count per centre (laid out as feats: the centres)
  DevBuf wb_feco_k;                    // ... and k per replicated row: the rows the back end scored
  DevBuf wb_xbar;                      // k_wb_feco_t's output [T][dim]: the cotangent on one replica's voiced rows
  int wb_feco_launches = 0;            // k_wb_feco_t launches of the last call (fb_debug_wb_feco_route)
  // white-box gradients of a universal perturbation (fb_set_wb_universal)
  int wb_universal = 0;                // the switch: 0 (as created) refuses companions, as before it existed
  DevBuf wb_uni_cot;                   // the R replicas' cotangents on their composed rows [R][N] (K > 1, no air channel)
  DevBuf wb_uni_rows;                  // the K composed rows the chain read [K][N] (K > 1 under a chain without an air channel)
  int wb_universal_launches = 0;       // k_wb_compose_t launches of the last call (fb_debug_wb_universal_route)
  FbNesDev *h_out = nullptr;  // pinned
  int *h_tv = nullptr;        // pinned, grows
  size_t h_tv_cap = 0;
  // pinned staging arena: every host<->device copy of the API goes through it.  (An async copy from / to pageable
  // memory makes the runtime pin the pages on the fly; with other engines' kernels in flight on the same GPU that
  // driver call was observed to stall the calling thread for milliseconds.)
  char *pin = nullptr;
  size_t pin_cap = 0, pin_off = 0;
  struct PendingD2H { void *dst; const void *src; size_t n; };
  std::vector<PendingD2H> pin_pending;
  // stats
  int64_t scored_utts = 0, scored_frames = 0, voiced_frames = 0, nes_iters = 0;
};

// ------------------------------------------------------------ pinned staging
static const size_t FB_PIN_MAX = (size_t)256 << 20;  // larger copies take the runtime's own pageable path

// stream synchronize + completion of the staged device->host copies
static int sync_stream(fb_engine *e) {
  HIPCHK(hipStreamSynchronize(e->stream));
  for (const fb_engine::PendingD2H &q : e->pin_pending) memcpy(q.dst, q.src, q.n);
  e->pin_pending.clear();
  e->pin_off = 0;
  return FB_OK;
}
static int pin_reserve(fb_engine *e, size_t n, char **out) {
  const size_t need = (n + 255) & ~(size_t)255;
  if (e->pin_off + need > e->pin_cap) {
    FBCHK(sync_stream(e));  // arena empty from here on
    if (need > e->pin_cap) {
      if (e->pin) (void)hipHostFree(e->pin);
      e->pin = nullptr;
      e->pin_cap = 0;
      const size_t want = need + need / 2 + ((size_t)1 << 20);
      hipError_t er = hipHostMalloc((void **)&e->pin, want, hipHostMallocDefault);
      if (er != hipSuccess) return fb_fail(FB_E_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(er));
      e->pin_cap = want;
    }
  }
  *out = e->pin + e->pin_off;
  e->pin_off += need;
  return FB_OK;
}
// host -> device on the engine's stream; `src` may be reused as soon as this returns
static int h2d(fb_engine *e, void *dst_dev, const void *src, size_t n) {
  if (n == 0) return FB_OK;
  if (n > FB_PIN_MAX) {
    HIPCHK(hipMemcpyAsync(dst_dev, src, n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FB_OK;
  }
  char *st = nullptr;
  FBCHK(pin_reserve(e, n, &st));
  memcpy(st, src, n);
  HIPCHK(hipMemcpyAsync(dst_dev, st, n, hipMemcpyHostToDevice, e->stream));
  return FB_OK;
}
// device -> host on the engine's stream; `dst` is valid after the next sync_stream()
static int d2h(fb_engine *e, void *dst, const void *src_dev, size_t n) {
  if (n == 0) return FB_OK;
  if (n > FB_PIN_MAX) {
    HIPCHK(hipMemcpyAsync(dst, src_dev, n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FB_OK;
  }
  char *st = nullptr;
  FBCHK(pin_reserve(e, n, &st));
  HIPCHK(hipMemcpyAsync(st, src_dev, n, hipMemcpyDeviceToHost, e->stream));
  e->pin_pending.push_back({dst, st, n});
  return FB_OK;
}

// The engines of this process on one device whose chain is the shared-GPU one (fb_set_fused_chain(e, 0)): what the drivers
// set on every engine when three or more attacks share a GPU.  From three on the attack loop does not drain its stream
// between looks (loop_knobs, attack_loop): there a stopping attack's extra batch of empty launches is cheap beside what the
// other attacks run meanwhile.  A lone engine on that chain keeps its drained looks, like every lone attack: it queues
// exactly the looks it reads.
static std::atomic<int> g_shared_chain[64];
static int shared_chain_count(int device, int delta) {
  std::atomic<int> &c = g_shared_chain[device & 63];
  return delta ? c.fetch_add(delta) + delta : c.load();
}
static bool fb_shared_gpu(const fb_engine *e) { return e->fuse_opt == 0 && shared_chain_count(e->device, 0) >= 3; }

// ------------------------------------------------------------------ create
extern "C" int fb_engine_create(int device, fb_engine **out) {
  if (!out) return fb_fail(FB_E_ARG, "out is NULL");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fb_fail(FB_E_ARG, "device %d out of range (%d visible)", device, n);
  HIPCHK(hipSetDevice(device));
  fb_engine *e = new fb_engine();
  e->device = device;
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&e->ev0));
  HIPCHK(hipEventCreate(&e->ev1));
  for (auto &bank : e->evg_ring) for (hipEvent_t &ev : bank) HIPCHK(hipEventCreate(&ev));
  HIPCHK(hipHostMalloc((void **)&e->h_ctl, sizeof(FbCtlDev), hipHostMallocDefault));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(hipHostMalloc((void **)&e->h_look[i], sizeof(FbCtlDev), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&e->ev_look[i], hipEventDisableTiming));
  }
  HIPCHK(hipHostMalloc((void **)&e->h_out, sizeof(FbNesDev), hipHostMallocDefault));
  fb_frontend_cfg cfg;
  fb_default_frontend(&cfg);
  *out = e;
  int rc = fb_set_frontend(e, &cfg);
  if (rc != FB_OK) { fb_engine_destroy(e); *out = nullptr; return rc; }
  return FB_OK;
}

extern "C" int fb_engine_destroy(fb_engine *e) {
  if (!e) return FB_OK;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->h_out) (void)hipHostFree(e->h_out);
  if (e->h_tv) (void)hipHostFree(e->h_tv);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  for (auto &bank : e->evg_ring) for (hipEvent_t ev : bank) if (ev) (void)hipEventDestroy(ev);
  if (e->h_ctl) (void)hipHostFree(e->h_ctl);
  for (int i = 0; i < 2; ++i) {
    if (e->h_look[i]) (void)hipHostFree(e->h_look[i]);
    if (e->ev_look[i]) (void)hipEventDestroy(e->ev_look[i]);
  }
  shared_chain_count(e->device, e->fuse_opt == 0 ? -1 : 0);
  if (e->pin) (void)hipHostFree(e->pin);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;  // (the device buffers go with it: e->device is still the current one)
  return FB_OK;
}

// ---------------------------------------------------------------- frontend
extern "C" void fb_default_frontend(fb_frontend_cfg *c) {
  // [EXT] voxceleb/v1 conf/mfcc.conf, conf/vad.conf, delta_opts
  c->sample_freq = 16000.0; c->frame_length = 400; c->frame_shift = 160; c->padded_length = 512;
  c->num_mel_bins = 30; c->num_ceps = 24; c->low_freq = 20.0; c->high_freq = 7600.0;
  c->preemph = 0.97; c->cepstral_lifter = 22.0; c->snip_edges = 0; c->remove_dc = 1;
  c->use_energy = 1; c->raw_energy = 1; c->energy_floor = 0.0;
  c->vad_energy_threshold = 5.5; c->vad_energy_mean_scale = 0.5; c->vad_proportion_threshold = 0.12;
  c->vad_frames_context = 2; c->delta_window = 3; c->delta_order = 2; c->cmn_window = 300;
  c->text_scores = 0;
  c->compress_feats = 0;
  c->mfcc_f32 = 0;
  c->dither = 0.0;
}

int fb_mfcc_layout_doubles(int P, int L, int nb, int nc, int melw_n);  // frontend_kernels.hip

// fb_set_frontend's checks and host tables (fb_prepare.h), nothing of the engine: every check that can refuse the
// configuration runs here, on locals
struct FrontendPrepared {
  FbFrontendTables t;
  FbFrontendBlob blob;
  bool f32_shape = false;    // k_mfcc_f32's tables exist for this configuration
  std::vector<float> t32;    // ... and are these
  int dim = 0;
};
static int prepare_frontend(const fb_frontend_cfg *c, FrontendPrepared *out) {
  const int L = c->frame_length, P = c->padded_length, nb = c->num_mel_bins, nc = c->num_ceps;
  if (L <= 1 || L > 512 || P < L || (P & (P - 1)) || P < 8 || P > 512)
    return fb_fail(FB_E_ARG, "frame_length %d / padded_length %d unsupported (need L<=512, P power of 2)", L, P);
  if (nb <= 0 || nb > 128 || nc <= 0 || nc > nb || c->frame_shift <= 0)
    return fb_fail(FB_E_ARG, "bad mel/ceps/shift configuration");
  if (c->delta_order < 0 || c->delta_order > 4 || c->delta_window <= 0 || c->delta_window > 8)
    return fb_fail(FB_E_ARG, "bad delta options");
  // a CMVN window of no frames divides by zero in k_cmvn_sliding (NaN features, scored as they were); a negative VAD
  // context is no window at all
  if (c->cmn_window < 1) return fb_fail(FB_E_ARG, "cmn_window %d < 1", c->cmn_window);
  if (c->vad_frames_context < 0) return fb_fail(FB_E_ARG, "vad_frames_context %d < 0", c->vad_frames_context);
  if (!(c->dither >= 0.0) || !std::isfinite(c->dither)) return fb_fail(FB_E_ARG, "dither %g is not a finite value >= 0", c->dither);
  out->dim = nc * (c->delta_order + 1);
  if (out->dim > 256) return fb_fail(FB_E_ARG, "feature dim %d > 256 unsupported", out->dim);
  std::string err;
  const int rc = fb_frontend_tables(c, &out->t, &err);
  if (rc != FB_OK) return fb_fail(rc, "%s", err.c_str());
  const FbFrontendTables &t = out->t;
  out->blob = fb_frontend_pack(t);
  if (sizeof(double) * (size_t)(fb_mfcc_layout_doubles(P, L, nb, nc, (int)t.mel_w.size())) > 150 * 1024)
    return fb_fail(FB_E_ARG, "front-end tables do not fit LDS (padded_length %d, %d mel bins)", P, nb);
  out->f32_shape = P == 512 && nb <= 31 && nc <= 32 && (L & 1) == 0 && fb_mfcc_f32_mel_pieces(t.mel_len.data(), nb) <= 64;
  if (c->mfcc_f32 && !(out->f32_shape && c->raw_energy != 0))
    return fb_fail(FB_E_ARG, "mfcc_f32 needs padded_length 512, raw_energy, <= 31 mel bins, <= 32 cepstra and an even frame length");
  if (out->f32_shape)  // (any precision setting: the flag may come later)
    out->t32 = fb_mfcc_f32_table(L, nb, nc, t.window.data(), t.tw_half.data(), t.tw_full.data(), t.mel_first.data(), t.mel_len.data(),
                                 t.mel_off.data(), t.mel_w.data(), (int)t.mel_w.size(), t.dct.data(), t.lifter.data());
  return FB_OK;
}

extern "C" int fb_set_frontend(fb_engine *e, const fb_frontend_cfg *c) {
  if (!e || !c) return fb_fail(FB_E_ARG, "null argument");
  FrontendPrepared p;
  FBCHK(prepare_frontend(c, &p));  // a refused call leaves e->fe, e->cfg and the device tables exactly as they were
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  FBCHK(e->fe_tables.ensure(p.blob.bytes.size()));
  if (p.f32_shape) FBCHK(e->fe_tables32.ensure(sizeof(float) * p.t32.size()));
  HIPCHK(hipMemcpy(e->fe_tables.p, p.blob.bytes.data(), p.blob.bytes.size(), hipMemcpyHostToDevice));
  if (p.f32_shape) HIPCHK(hipMemcpy(e->fe_tables32.p, p.t32.data(), sizeof(float) * p.t32.size(), hipMemcpyHostToDevice));
  char *base = e->fe_tables.as<char>();
  const FbFrontendBlob &b = p.blob;
  FbFrontendDev &fe = e->fe;
  fe.L = c->frame_length; fe.P = c->padded_length; fe.shift = c->frame_shift; fe.nb = c->num_mel_bins; fe.nc = c->num_ceps;
  fe.dim = p.dim; fe.order = c->delta_order;
  fe.dwin = c->delta_window; fe.cmn_window = c->cmn_window; fe.snip_edges = c->snip_edges; fe.remove_dc = c->remove_dc;
  fe.use_energy = c->use_energy; fe.raw_energy = c->raw_energy; fe.vad_ctx = c->vad_frames_context;
  fe.preemph = c->preemph;
  fe.mfcc_f32 = c->mfcc_f32 ? 1 : 0;
  fe.log_energy_floor = c->energy_floor > 0.0 ? log(c->energy_floor) : -INFINITY;
  fe.vad_thr = c->vad_energy_threshold; fe.vad_mean_scale = c->vad_energy_mean_scale;
  fe.vad_prop = (float)c->vad_proportion_threshold;
  fe.window = (const double *)(base + b.o_window); fe.tw_half = (const double *)(base + b.o_twh);
  fe.tw_full = (const double *)(base + b.o_twf); fe.mel_first = (const int *)(base + b.o_mf);
  fe.mel_len = (const int *)(base + b.o_ml); fe.mel_off = (const int *)(base + b.o_mo);
  fe.mel_w = (const double *)(base + b.o_mw); fe.dct = (const double *)(base + b.o_dct);
  fe.lifter = (const double *)(base + b.o_lift); fe.dscale = (const double *)(base + b.o_ds);
  e->melw_n = (int)p.t.mel_w.size();
  fe.f32_tab = p.f32_shape ? e->fe_tables32.as<float>() : nullptr;
  e->cfg = *c;
  e->gmm.text_scores = c->text_scores;
  e->iv.text_scores = c->text_scores;
  e->have_fe = true;
  e->cached_B = -1;
  if (e->have_gmm && e->gmm.D != p.dim) e->have_gmm = false;
  return FB_OK;
}

static int num_frames(const fb_frontend_cfg &c, int64_t n) {
  if (c.snip_edges) return n < c.frame_length ? 0 : (int)(1 + (n - c.frame_length) / c.frame_shift);
  return (int)((n + c.frame_shift / 2) / c.frame_shift);
}

// --------------------------------------------------------------------- gmm
// FB_GMM_MODE, FB_GMM_DELTA_BUDGET, FB_GMM_DELTA_F6, FB_GMM_DELTA_P -> the options of fb_prepare_gmm; the one place that
// reads them.  A value that is refused is refused whatever the model's shape.
static int gmm_options_from_env(FbGmmPrepOptions *o) {
  *o = FbGmmPrepOptions();
  const char *mode_env = getenv("FB_GMM_MODE");
  if (mode_env && strcmp(mode_env, "bx3") == 0) o->forced_mode = FB_GMM_MODE_BX3;  // force the fallback kernel (tests)
  else if (mode_env && *mode_env && strcmp(mode_env, "fx2") != 0)
    return fb_fail(FB_E_ARG, "FB_GMM_MODE must be fx2 or bx3 (got '%s')", mode_env);
  if (const char *be = getenv("FB_GMM_DELTA_BUDGET")) {
    const double v = atof(be);
    if (!(v >= 1e-7 && v <= 1e-4)) return fb_fail(FB_E_ARG, "FB_GMM_DELTA_BUDGET must be in [1e-7, 1e-4] (got '%s')", be);
    o->budget = v;
  }
  if (const char *fe6 = getenv("FB_GMM_DELTA_F6")) o->use_f6 = !(fe6[0] == '0' && fe6[1] == 0);
  const char *pe = getenv("FB_GMM_DELTA_P");
  if (pe && *pe) {
    const int v = atoi(pe);
    if (!(v >= 1 && v <= 3) && v != 6) return fb_fail(FB_E_ARG, "FB_GMM_DELTA_P must be 1, 2, 3 or 6 (got '%s')", pe);
    o->forced_p = v;
  }
  return FB_OK;
}

// steps 1 and 2 of fb_load_gmm: the argument checks and the host images.  e == nullptr (fb_debug_prepare_gmm): no
// front end to agree with
static int prepare_gmm(const fb_engine *e, int M, int C, int D, const float *gconsts, const float *miv, const float *iv,
                       FbGmmPrepared *out) {
  if (!gconsts || !miv || !iv) return fb_fail(FB_E_ARG, "null argument");
  if (M <= 0 || C <= 0 || D <= 0) return fb_fail(FB_E_ARG, "bad GMM shape M=%d C=%d D=%d", M, C, D);
  if (M > 60) return fb_fail(FB_E_ARG, "at most 60 models per engine (got %d)", M);
  if (e && (!e->have_fe || e->fe.dim != D))
    return fb_fail(FB_E_ARG, "GMM dim %d != front-end feature dim %d", D, e->have_fe ? e->fe.dim : -1);
  FbGmmPrepOptions opt;
  FBCHK(gmm_options_from_env(&opt));
  std::string err;
  const int rc = fb_prepare_gmm(FbGmmParams{M, C, D, gconsts, miv, iv}, opt, out, &err);
  return rc == FB_OK ? FB_OK : fb_fail(rc, "%s", err.c_str());
}

// steps 4 to 6: ensure every buffer, upload, assign the engine's fields (the stream is idle: the caller synchronised)
static int commit_gmm(fb_engine *e, const FbGmmPrepared &p, const float *gconsts, const float *miv, const float *iv) {
  const int M = p.M, C = p.C, D = p.D;
  DevBuf *pass_buf[FB_FXW_MAX_PASS] = {&e->gmm_images_fd, &e->gmm_images_fd2, &e->gmm_images_fd3};
  auto bytes = [](const auto &v) { return sizeof(v[0]) * v.size(); };
  if (!p.fx.empty()) FBCHK(e->gmm_images_fx.ensure(bytes(p.fx)));
  if (!p.bx.empty()) FBCHK(e->gmm_images_bx.ensure(bytes(p.bx)));
  for (int q = 0; q < FB_FXW_MAX_PASS; ++q)
    if (!p.fd[q].empty()) FBCHK(pass_buf[q]->ensure(bytes(p.fd[q]) + 4096));  // k_gmm_fx2w fetches whole 1 KB pieces: up to 3 past the end
  if (!p.anchor.empty()) FBCHK(e->gmm_anchor.ensure(bytes(p.anchor)));
  FBCHK(e->gmm_items.ensure(bytes(p.item_model)));
  FBCHK(e->zmean.ensure(sizeof(double) * M));
  FBCHK(e->zstd.ensure(sizeof(double) * M));
  auto upload = [](DevBuf &dst, const auto &v) {
    return v.empty() ? hipSuccess : hipMemcpy(dst.p, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice);
  };
  HIPCHK(upload(e->gmm_images_fx, p.fx));
  HIPCHK(upload(e->gmm_images_bx, p.bx));
  for (int q = 0; q < FB_FXW_MAX_PASS; ++q) HIPCHK(upload(*pass_buf[q], p.fd[q]));
  HIPCHK(upload(e->gmm_anchor, p.anchor));
  HIPCHK(upload(e->gmm_items, p.item_model));
  // default system: OSI (UBM first) without z-norm
  e->h_zmean.assign(M, 0.0);
  e->h_zstd.assign(M, 1.0);
  HIPCHK(upload(e->zmean, e->h_zmean));
  HIPCHK(upload(e->zstd, e->h_zstd));
  using Images = decltype(e->gmm.images_fd);
  FbGmmDev &g = e->gmm;
  g.M = M; g.C = C; g.D = D; g.n_tiles = p.n_tiles; g.n_items = p.n_items;
  g.mode = p.mode; g.NK = p.NK;
  g.text_scores = e->cfg.text_scores;
  g.only_if = nullptr;
  g.fxw_sub = 0;
  g.images_bx = reinterpret_cast<Images>(e->gmm_images_bx.p);
  g.NKF = p.NKF;
  g.kx = p.kx; g.kx2 = p.kx2; g.kacc = p.kacc;
  g.images_fx = reinterpret_cast<Images>(e->gmm_images_fx.p);
  g.delta_p = p.delta_p; g.delta_t3 = p.delta_t3; g.delta_t2 = p.delta_t2; g.delta_t6 = p.delta_t6;
  g.images_fd = g.delta_p ? reinterpret_cast<Images>(e->gmm_images_fd.p) : nullptr;
  g.n_pass = p.n_pass;
  g.pass_first = 1;
  for (int q = 0; q < FB_FXW_MAX_PASS; ++q) g.pass_images[q] = q < p.n_pass ? reinterpret_cast<Images>(pass_buf[q]->p) : nullptr;
  for (int q = 0; q <= FB_FXW_MAX_PASS; ++q) g.pass_lo[q] = p.pass_lo[q];
  g.anchor = g.delta_p ? e->gmm_anchor.as<float>() : nullptr;
  g.item_model = e->gmm_items.as<int>();
  g.item_model_host_q_first = (p.n_groups == 1) ? 1 : 0;  // one group: the item list is {Q, 0, 1, ..., M-1}
  e->gmm_delta_rms = p.delta_rms;
  // the white-box path differentiates the plain parameters: kept here, uploaded by its first call, freed on reload
  e->h_wb_gc.assign(gconsts, gconsts + (size_t)M * C);
  e->h_wb_miv.assign(miv, miv + (size_t)M * C * D);
  e->h_wb_iv.assign(iv, iv + (size_t)M * C * D);
  e->wb_uploaded = false;
  e->wb_gc.release(); e->wb_miv.release(); e->wb_iv.release();
  e->n_groups = p.n_groups;
  e->have_gmm = true;
  e->kind = 0;
  e->n_out = M;
  return FB_OK;
}

static void note_too_many_for_wide(int M) {
  static bool warned = false;
  if (warned) return;
  warned = true;
  fprintf(stderr, "[fakebob_hip] note: %d models in one variance group: k_gmm_fx2w takes at most %d (in %d passes), this "
                  "system is scored by the general kernel k_gmm_fx2 (about twice the time per model)\n", M,
          fb_gmm_max_wide_models(), FB_FXW_MAX_PASS);
}

extern "C" int fb_load_gmm(fb_engine *e, int M, int C, int D, const float *gconsts, const float *miv,
                           const float *iv) {
  if (!e) return fb_fail(FB_E_ARG, "null argument");
  FbGmmPrepared p;
  FBCHK(prepare_gmm(e, M, C, D, gconsts, miv, iv, &p));  // a refused call leaves the engine and the device as they were
  if (p.too_many_for_wide) note_too_many_for_wide(M);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  return commit_gmm(e, p, gconsts, miv, iv);
}

extern "C" int fb_set_system(fb_engine *e, int task, const double *z_mean, const double *z_std) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "load a model first");
  if (task != FB_TASK_OSI && task != FB_TASK_CSI && task != FB_TASK_SV) return fb_fail(FB_E_ARG, "bad task");
  if (e->kind == 1) return fb_fail(FB_E_STATE, "i-vector systems take their task and z-norm from fb_load_ivector");
  if (e->kind == 2) return fb_fail(FB_E_STATE, "x-vector systems take their task and z-norm from fb_load_xvector");
  const int M = e->n_out;
  if (task != FB_TASK_CSI && M < 2) return fb_fail(FB_E_ARG, "OSI/SV need the UBM + >=1 speaker model");
  if (task == FB_TASK_SV && M != 2) return fb_fail(FB_E_ARG, "SV takes exactly [ubm, speaker]");
  HIPCHK(hipSetDevice(e->device));
  e->task = task;
  for (int m = 0; m < M; ++m) {
    e->h_zmean[m] = (task == FB_TASK_CSI && z_mean) ? z_mean[m] : 0.0;
    e->h_zstd[m] = (task == FB_TASK_CSI && z_std) ? z_std[m] : 1.0;
  }
  FBCHK(sync_stream(e));
  HIPCHK(hipMemcpy(e->zmean.p, e->h_zmean.data(), sizeof(double) * M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->zstd.p, e->h_zstd.data(), sizeof(double) * M, hipMemcpyHostToDevice));
  return FB_OK;
}

extern "C" int fb_num_speakers(fb_engine *e) {
  if (!e || !e->have_gmm) return 0;
  if (e->kind != 0) return e->n_out;
  return e->task == FB_TASK_CSI ? e->n_out : e->n_out - 1;
}

// ------------------------------------------------------- scoring pipeline
// Prepares offsets for a batch whose int16 samples are already in e->wav.
static int prepare_batch(fb_engine *e, const int64_t *off, int B) {
  e->bench_it = e->nes_rec.iter = -1;  // whatever attack fb_bench_nes left resident is gone with the batch layout
  if (e->vad_counter.p) HIPCHK(hipMemsetAsync(e->vad_counter.p, 0, sizeof(int), e->stream));  // see ctl_reset
  e->h_wav_off.assign(off, off + B + 1);
  e->h_frame_off.resize(B + 1);
  e->h_chunk_off.resize(B + 1);
  e->h_frame_off[0] = 0;
  e->h_chunk_off[0] = 0;
  e->any_long = false;
  e->t_max = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b];
    if (n <= 0) return fb_fail(FB_E_ARG, "utterance %d is empty", b);
    const int T = num_frames(e->cfg, n);
    if (T <= 0) return fb_fail(FB_E_ARG, "utterance %d (%lld samples) is shorter than one frame", b, (long long)n);
    e->h_frame_off[b + 1] = e->h_frame_off[b] + T;
    e->h_chunk_off[b + 1] = e->h_chunk_off[b] + (T + 31) / 32;
    if (T > e->cfg.cmn_window) e->any_long = true;
    if (T > e->t_max) e->t_max = T;
  }
  {  // equal lengths: k_mfcc_f32 computes a frame's record instead of loading it
    bool uni = true;
    for (int b = 1; b < B && uni; ++b) uni = (off[b + 1] - off[b]) == (off[1] - off[0]);
    e->uni_T = uni ? e->h_frame_off[1] : 0;
    e->uni_n = uni ? off[1] - off[0] : 0;
  }
  {  // per-frame records for k_mfcc_r16: {absolute start sample (int64), start within the utterance, n}
    const int total = e->h_frame_off[B];
    e->h_frame_rec.resize((size_t)4 * total);
    const fb_frontend_cfg &c = e->cfg;
    for (int b = 0; b < B; ++b) {
      const int64_t n = off[b + 1] - off[b];
      if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance %d longer than 2^31 samples", b);
      for (int f = e->h_frame_off[b]; f < e->h_frame_off[b + 1]; ++f) {
        const int64_t t = f - e->h_frame_off[b];
        const int64_t start = c.snip_edges ? t * c.frame_shift : t * c.frame_shift + c.frame_shift / 2 - c.frame_length / 2;
        const int64_t abs_start = off[b] + start;
        memcpy(&e->h_frame_rec[(size_t)4 * f], &abs_start, 8);
        e->h_frame_rec[(size_t)4 * f + 2] = (int32_t)start;
        e->h_frame_rec[(size_t)4 * f + 3] = (int32_t)n;
      }
    }
    FBCHK(e->frame_rec.ensure(sizeof(int32_t) * 4 * (size_t)(total > 0 ? total : 1)));
    FBCHK(h2d(e, e->frame_rec.p, e->h_frame_rec.data(), sizeof(int32_t) * 4 * (size_t)total));
    if (e->cfg.dither > 0.0) {  // the dithered kernels' counter words of a frame: {utterance, frame within it}
      e->h_frame_ut.resize((size_t)2 * total);
      for (int b = 0; b < B; ++b)
        for (int f = e->h_frame_off[b]; f < e->h_frame_off[b + 1]; ++f) {
          e->h_frame_ut[(size_t)2 * f] = b;
          e->h_frame_ut[(size_t)2 * f + 1] = f - e->h_frame_off[b];
        }
      FBCHK(e->frame_ut.ensure(sizeof(int32_t) * 2 * (size_t)(total > 0 ? total : 1)));
      FBCHK(h2d(e, e->frame_ut.p, e->h_frame_ut.data(), sizeof(int32_t) * 2 * (size_t)total));
    }
  }
  FBCHK(e->chunk_off.ensure(sizeof(int) * (B + 1)));
  FBCHK(h2d(e, e->chunk_off.p, e->h_chunk_off.data(), sizeof(int) * (B + 1)));
  FBCHK(e->wav_off.ensure(sizeof(int64_t) * (B + 1)));
  FBCHK(e->frame_off.ensure(sizeof(int) * (B + 1)));
  FBCHK(h2d(e, e->wav_off.p, e->h_wav_off.data(), sizeof(int64_t) * (B + 1)));
  FBCHK(h2d(e, e->frame_off.p, e->h_frame_off.data(), sizeof(int) * (B + 1)));
  return FB_OK;
}

// Split the component tiles into chunks so that the launch is ONE fully resident round:
// ~4 workgroups per CU (VGPR/LDS budget of k_gmm) x 256 CUs.  A second, partially filled round
// would idle most of the chip for a whole chunk's duration.
static int choose_chunks(const FbGmmDev &g, int rows_cap, bool scoring = true) {
  const bool wide = scoring && fb_gmm_use_wide(g);  // k_gmm_fx2w: 256-frame strips, one workgroup per CU
  const int strips = wide ? (rows_cap + 255) / 256 : (rows_cap + 127) / 128;
  const char *ev = getenv("FB_GMM_TARGET_BLOCKS");
  const int target = ev ? atoi(ev) : (wide ? 256 : (g.mode == FB_GMM_MODE_FX2 ? 256 * FB_FX_OCC : 512));
  int want = target / (strips > 0 ? strips : 1);
  if (want < 1) want = 1;
  if (want > g.n_tiles) want = g.n_tiles;
  const int tpc = (g.n_tiles + want - 1) / want;
  return (g.n_tiles + tpc - 1) / tpc;
}

// FB_DEBUG_SYNC=1: synchronise after every stage and report it on stderr (fault localisation)
static bool fb_debug_sync_on() {
  static int v = -1;
  if (v < 0) { const char *ev = getenv("FB_DEBUG_SYNC"); v = (ev && atoi(ev) != 0) ? 1 : 0; }
  return v == 1;
}
#define FB_DBG_SYNC(e, what)                                                                        \
  do {                                                                                              \
    if (fb_debug_sync_on()) {                                                                       \
      hipError_t err_ = hipStreamSynchronize((e)->stream);                                          \
      fprintf(stderr, "[fb] %s: %s\n", what, hipGetErrorString(err_));                               \
      fflush(stderr);                                                                               \
    }                                                                                               \
  } while (0)

// HIP-event timing of the dominant kernel (bench only): a ring of event pairs, because several
// iterations may be queued before the host looks at the stream again
// (one bank: its launches have completed, the other bank's need not have)
static int time_collect_bank(fb_engine *e, int bank) {
  for (int i = 0; i < e->evg_n[bank]; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->evg_ring[bank][2 * i], e->evg_ring[bank][2 * i + 1]));
    e->gmm_ms_acc += (double)ms;
    e->gmm_launches += 1;
  }
  e->evg_n[bank] = 0;
  e->gmm_pending = e->evg_n[0] + e->evg_n[1] > 0;
  return FB_OK;
}
// (the stream is idle: both banks)
static int time_collect(fb_engine *e) {
  FBCHK(time_collect_bank(e, 0));
  return time_collect_bank(e, 1);
}
static int time_begin(fb_engine *e, int what = 1) {
  if (e->time_gmm != what) return FB_OK;
  if (e->evg_n[e->evg_cur] >= 16) {  // ring full: drain (never happens with the batch sizes used)
    FBCHK(sync_stream(e));
    FBCHK(time_collect(e));
  }
  HIPCHK(hipEventRecord(e->evg_ring[e->evg_cur][2 * e->evg_n[e->evg_cur]], e->stream));
  return FB_OK;
}
static int time_end(fb_engine *e, int what = 1) {
  if (e->time_gmm != what) return FB_OK;
  HIPCHK(hipEventRecord(e->evg_ring[e->evg_cur][2 * e->evg_n[e->evg_cur] + 1], e->stream));
  e->evg_n[e->evg_cur] += 1;
  e->gmm_pending = true;
  return FB_OK;
}

static bool fb_fuse_on(const fb_engine *e);
static bool fb_fuse_part(const fb_engine *e, int part);  // 0: VAD + deltas + CMVN, 1: finalisation + loss, 2: update + next batch
// k_iv_solve_rw (five workgroups per matrix) is the LATENCY form of the posterior solve: it finishes a batch of 51 systems
// sooner, on 255 compute units instead of 51 -- right for one attack per GPU, wrong when several attacks share the chip
// and the idle units are what their kernels run on.  fb_set_fused_chain(e, 1) -- what the drivers choose for one or two
// attacks in flight -- selects it; FB_IV_SOLVE=rw | ll forces either.
static bool fb_iv_use_rw(const fb_engine *e) {
  const char *ev = getenv("FB_IV_SOLVE");
  if (ev && strcmp(ev, "rw") == 0) return true;
  if (ev && strcmp(ev, "ll") == 0) return false;
  return e->fuse_opt == 1;
}
// The launch shape of a batch on a GPU shared by three or more attacks (fb_set_fused_chain(e, 0)): k_gmm_fx2w with two
// component chunks per workgroup and k_mfcc_f32 on half of the compute units (run_scoring says why); FB_GMM_SUB=1 | 2 and
// FB_MFCC_CUS=n force either.  Every path that launches those kernels decides it here, at the start of its batch, so that
// none inherits the shape of the batch before it; the record fb_debug_launch_shape reads starts empty with it.
static void choose_launch_shape(fb_engine *e) {
  const char *sv = getenv("FB_GMM_SUB"), *cv = getenv("FB_MFCC_CUS");
  e->gmm.fxw_sub = sv ? atoi(sv) : (e->fuse_opt == 0 ? 2 : 1);
  e->fe.mfcc_cus = cv ? atoi(cv) : (e->fuse_opt == 0 ? 128 : 0);
  e->shape_gmm = FbGmmShape{};
  e->shape_mfcc = FbMfccShape{};
  e->shape_upd_threads = 0;
  e->have_shape = true;
}
// ... and the third part of that shape: the threads of a k_update_perturb(_x) workgroup.  On the shared GPU 256, one wave
// per SIMD: a k_gmm_fx2w workgroup leaves a SIMD 88 of its 512 registers, the kernel takes 56 per wave, so its workgroups run
// beside the other attacks' GMM launches instead of queueing for the compute units those leave free (nes_kernels.hip).  A
// lone attack keeps 512: nothing else is resident, and more waves draw the next batch sooner.  FB_UP_THREADS=256 | 512
// forces either.  Unlike the two above this one is an attack's, not a batch's: loop_knobs calls it once, at the start of the
// public call, and the loop carries the answer.
static int choose_update_threads(const fb_engine *e) {
  if (const char *uv = getenv("FB_UP_THREADS")) {
    const int t = atoi(uv);
    if (t == 256 || t == 512) return t;
  }
  return e->fuse_opt == 0 ? 256 : 512;
}
// the update launch of the batch as it went out (fb_debug_launch_shape); a foreign model's attack scores no batch of the
// engine's own, so its record starts here
static void record_update_threads(fb_engine *e, int threads) {
  e->shape_upd_threads = threads;
  e->have_shape = true;
}
// the NES batch of Philox iteration `iter` as its launch went out (fb_debug_nes_batch): q, the int16 rows are in e->wav; z, the
// launch kept its normals in e->zbuf
static void record_nes_batch(fb_engine *e, long long iter, int64_t N, int half, bool q, bool z) {
  e->nes_rec.queued = iter;
  e->nes_rec.N = N;
  e->nes_rec.half = half;
  e->nes_rec.q = q;
  e->nes_rec.z = z;
}
// The batch the MFCC reads: e->wav, or -- with an input-transform chain set -- its transform in e->wav_tf, one more launch.
// off: the batch's offsets on the host (off[0] = 0), already in e->wav_off on the device.
// stages of kind FB_TF_NOISE in the chain (snr_only: in SNR mode, the ones that need k_tf_power in front)
static int tf_noise_stages(const FbTfChain &ch, bool snr_only) {
  int c = 0;
  for (int s = 0; s < ch.n; ++s) c += ch.kind[s] == FB_TF_NOISE && (!snr_only || ch.k[s] == 1);
  return c;
}
// What one scoring call tells run_scoring and the helpers under it about its batch.  It lives on the caller's stack for the
// length of the call -- nothing of it is engine state --, and a default-constructed one plus a point is a scoring call
// outside an attack: one replica per utterance, no stop flag, no loss tail.
struct FbScoreCall {
  FbRngPoint pt = {};            // where the call stands in the dither, noise and feature-compression contracts
  int eot = 1;                   // draws of every utterance (fb_set_eot) ...
  int K = 1;                     // ... and utterances of every NES row (fb_set_companions): the batch holds K * eot rows per NES row
  const int *stop = nullptr;     // nullable device flag: != 0 -> the call's launches do nothing (attack already stopped)
  bool defer_finalize = false;   // the GMM finalisation is left to the caller's fused finalize + loss launch
  const FbIvTail *tail_loss = nullptr;  // i-vector systems: the loss body the solve kernels' tail should take along (null: none)
  bool tail_loss_done = false;   // out: it did
  bool feats_given = false;      // e->feats / e->row_off / e->tv already hold the batch's rows: no front end (fb_debug_iv_feat_grad)
  bool keep_iv_quad = false;     // i-vector systems: row 0 of quad as the contraction left it is copied to e->wb_iv_quad (white box)
  int keep_iv_quad_rows = 1;     // ... rows 0 .. this - 1: every replica's under fb_set_wb_universal
  bool keep_air_sat = false;     // an air channel: k_air_conv also writes its saturation bytes to e->wb_air_sat (white box)
  bool keep_xv_mask = false;     // x-vector systems: k_xv_affine also writes every layer's ReLU decisions to e->xv_mask (white box)
  bool keep_feco = false;        // feature compression: k_feature_compress also writes its final labels, counts and k's to e->wb_feco_* (white box)
  int64_t play = 0;              // > 0 (fb_set_play_offset): k_play_compose writes the K * eot replicas, each under its own offset in 0 .. play
  int replicas() const { return K * eot; }
};
// The replicating / composing transform launch: rn.r replicas of every utterance of `in` (in_off[B_in + 1]; longest: n_max) --
// with cn of every utterance of its composition -- written at out_off of `out`, behind the launch that leaves the chain's
// SNR stages their sums of squares: one E per (row, utterance), of the row as composed
static int launch_transform_replicas(fb_engine *e, const int16_t *in, const int64_t *in_off, int B_in, int64_t n_max, int16_t *out,
                                     const int64_t *out_off, FbTfRnd rn, const FbTfComp *cn, const int *stop) {
  rn.power = nullptr;
  if (tf_noise_stages(e->tf, true) > 0) {  // a launch of its own, read by the next one only
    FBCHK(e->tf_power.ensure(sizeof(unsigned long long) * (size_t)B_in * (cn ? cn->K : 1)));
    unsigned long long *power = e->tf_power.as<unsigned long long>();
    if (cn) HIPCHK(fb_launch_tf_power_cmp(e->stream, in, in_off, B_in, n_max, power, *cn, stop));
    else HIPCHK(fb_launch_tf_power(e->stream, in, in_off, B_in, n_max, power, stop));
    rn.power = power;
  }
  if (cn) fb_launch_input_transform_cmp(e->stream, e->tf, e->tf_taps.as<double>(), in, in_off, B_in, n_max, out, out_off, rn, *cn, stop);
  else fb_launch_input_transform_rnd(e->stream, e->tf, e->tf_taps.as<double>(), in, in_off, B_in, n_max, out, out_off, rn, stop);
  return FB_OK;
}
// The over-the-air channel and the chain behind it: rows = B_in * r output rows (row R = replica R % r of utterance row R / r
// of `in`; with cn utterance (R % r) / eot of that row as composed) go through k_air_taps + k_air_conv into e->wav_air at
// out_off, then -- if a chain is set -- through the chain's launch in its "input already replicated" mode into e->wav_tf
// (both buffers sized by the caller: out_samples).  *res: the buffer that holds the result.  keep_sat: the white-box call's
// FbScoreCall::keep_air_sat.
static int launch_air_path(fb_engine *e, const int16_t *in, const int64_t *in_off, int B_in, int r, int eot, int64_t n_max,
                           size_t out_samples, const int64_t *out_off, const FbRngPoint &pt, const FbTfComp *cn, const int *stop,
                           const int16_t **res, bool keep_sat = false, int pre = 0) {
  // pre > 0 (k_play_compose wrote `in`): the B_in rows are already the replicas -- row R is replica R % pre of utterance row
  // R / pre and draws as such; the convolution takes one input row per output row (r = 1, cn null)
  const int rows = B_in * r, L = e->air.L, draw_r = pre > 0 ? pre : r;
  FBCHK(e->wav_air.ensure(sizeof(int16_t) * out_samples));
  FBCHK(e->air_taps.ensure(sizeof(int16_t) * (size_t)rows * (size_t)L));
  if (keep_sat) FBCHK(e->wb_air_sat.ensure(out_samples));
  fb_launch_air_taps(e->stream, fb_air_key(pt, e->air, draw_r), 0, rows, e->air_taps.as<int16_t>(), nullptr, nullptr, stop);
  fb_launch_air_conv(e->stream, in, in_off, rows, r, eot, n_max, e->air_taps.as<int16_t>(), L, e->wav_air.as<int16_t>(), out_off, cn, stop,
                     keep_sat ? e->wb_air_sat.as<unsigned char>() : nullptr);
  *res = e->wav_air.as<int16_t>();
  if (e->tf.n == 0) return FB_OK;
  FBCHK(e->wav_tf.ensure(sizeof(int16_t) * out_samples));
  if (tf_noise_stages(e->tf, false) == 0) {
    fb_launch_input_transform(e->stream, e->tf, e->tf_taps.as<double>(), e->wav_air.as<int16_t>(), out_off, rows, n_max,
                              e->wav_tf.as<int16_t>(), stop);
  } else {  // the noise stages draw with (utterance row R / r, replica R % r); k_tf_power, the plain form, sums the channel's output rows
    FbTfRnd rn = fb_tf_rnd(pt, 1);
    rn.pre = draw_r;
    FBCHK(launch_transform_replicas(e, e->wav_air.as<int16_t>(), out_off, rows, n_max, e->wav_tf.as<int16_t>(), out_off, rn, nullptr, stop));
  }
  *res = e->wav_tf.as<int16_t>();
  return FB_OK;
}
// With r = call.replicas() > 1 (an NES batch under fb_set_eot) B counts the REPLICATED rows: e->wav holds B / r utterances of
// equal length -- the first B / r + 1 entries of e->wav_off describe them -- and replica j of utterance u goes to row
// u * r + j of e->wav_tf, every time and with an empty chain too.  With call.K > 1 (fb_set_companions) the same launch
// composes: replica c * eot + j is draw j over utterance c of the row (k_input_transform_cmp).
static int chained_wav(fb_engine *e, const FbScoreCall &call, const int64_t *off, int B, const int16_t **wav) {
  *wav = e->wav.as<int16_t>();
  const int r = call.replicas();
  if (e->tf.n == 0 && r == 1 && e->air.L == 0 && call.play == 0) return FB_OK;
  if (B > 65535) return fb_fail(FB_E_LIMIT, "an input-transform chain takes batches of up to 65535 utterances");
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) n_max = std::max(n_max, off[b + 1] - off[b]);
  if (n_max > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance longer than 2^31 samples");
  if (call.play > 0) {
    if (n_max <= call.play) return fb_fail(FB_E_ARG, "rows of %lld samples under a play offset of up to %lld", (long long)n_max, (long long)call.play);
    // (fb_set_play_offset) one launch composes the B rows -- B / r NES rows of n_max samples each, r replicas of every one, each
    // under its own offset -- into e->wav_play; what follows takes them as input that is already replicated
    const FbTfComp cn{call.K, n_max, e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>()};
    FBCHK(e->wav_play.ensure(sizeof(int16_t) * ((size_t)off[B] + 8)));
    FBCHK(e->play_tau.ensure(sizeof(uint32_t) * (size_t)B));
    fb_launch_play_compose(e->stream, fb_play_key(call.pt, call.play), e->wav.as<int16_t>(), cn, call.eot, B / r, e->wav_play.as<int16_t>(),
                           e->play_tau.as<uint32_t>(), call.stop);
    e->play_launches += 1;
    *wav = e->wav_play.as<int16_t>();
    if (e->air.L > 0)
      return launch_air_path(e, e->wav_play.as<int16_t>(), e->wav_off.as<int64_t>(), B, 1, call.eot, n_max, (size_t)off[B],
                             e->wav_off.as<int64_t>(), call.pt, nullptr, call.stop, wav, call.keep_air_sat, r);
    if (e->tf.n == 0) return FB_OK;  // the buffer is the batch the front end reads
    FBCHK(e->wav_tf.ensure(sizeof(int16_t) * (size_t)off[B]));
    if (tf_noise_stages(e->tf, false) == 0) {
      fb_launch_input_transform(e->stream, e->tf, e->tf_taps.as<double>(), e->wav_play.as<int16_t>(), e->wav_off.as<int64_t>(), B, n_max,
                                e->wav_tf.as<int16_t>(), call.stop);
    } else {  // (row R: utterance row R / r, replica R % r; k_tf_power, the plain form, sums the composed, offset rows)
      FbTfRnd rn = fb_tf_rnd(call.pt, 1);
      rn.pre = r;
      FBCHK(launch_transform_replicas(e, e->wav_play.as<int16_t>(), e->wav_off.as<int64_t>(), B, n_max, e->wav_tf.as<int16_t>(),
                                      e->wav_off.as<int64_t>(), rn, nullptr, call.stop));
    }
    *wav = e->wav_tf.as<int16_t>();
    return FB_OK;
  }
  if (e->air.L > 0) {  // (fb_set_air_channel) the channel writes the replicas, the chain follows row by row
    const FbTfComp cn{call.K, e->comp_N, e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>()};
    return launch_air_path(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B / r, r, call.eot, n_max, (size_t)off[B],
                           e->wav_off.as<int64_t>(), call.pt, call.K > 1 ? &cn : nullptr, call.stop, wav, call.keep_air_sat);
  }
  FBCHK(e->wav_tf.ensure(sizeof(int16_t) * (size_t)off[B]));
  if (r == 1 && tf_noise_stages(e->tf, false) == 0) {
    fb_launch_input_transform(e->stream, e->tf, e->tf_taps.as<double>(), e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, n_max,
                              e->wav_tf.as<int16_t>(), call.stop);
  } else {
    const FbTfComp cn{call.K, e->comp_N, e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>()};
    FBCHK(launch_transform_replicas(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B / r, n_max, e->wav_tf.as<int16_t>(),
                                    e->wav_off.as<int64_t>(), fb_tf_rnd(call.pt, call.eot), call.K > 1 ? &cn : nullptr, call.stop));
  }
  *wav = e->wav_tf.as<int16_t>();
  return FB_OK;
}
// The batch the front end reads: chained_wav's B rows, and -- with a codec set (fb_set_codec) -- their round trip through
// it, one more launch: in place on wav_tf / wav_air; e->wav itself, the batch other code reads and returns, is coded into a
// buffer of the codec's own.  The limits are the chain's.
static int transformed_wav(fb_engine *e, const FbScoreCall &call, const int64_t *off, int B, const int16_t **wav) {
  FBCHK(chained_wav(e, call, off, B, wav));
  if (e->codec == FB_CODEC_NONE) return FB_OK;
  if (B > 65535) return fb_fail(FB_E_LIMIT, "a codec takes batches of up to 65535 utterances");
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) n_max = std::max(n_max, off[b + 1] - off[b]);
  if (n_max > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance longer than 2^31 samples");
  int16_t *out = const_cast<int16_t *>(*wav);
  if (*wav == e->wav.as<int16_t>()) {
    FBCHK(e->wav_codec.ensure(sizeof(int16_t) * (size_t)off[B]));
    out = e->wav_codec.as<int16_t>();
  }
  fb_launch_codec(e->stream, e->codec, *wav, e->wav_off.as<int64_t>(), B, n_max, out, call.stop);
  *wav = out;
  return FB_OK;
}
// MFCC of every frame of the batch prepared in e->wav: k_mfcc_f32 when the configuration asks for it, else k_mfcc_r16 / k_mfcc
// fe: the engine's front end as the call's launches take it (run_scoring: with the call's stop flag)
static int launch_mfcc(fb_engine *e, const FbScoreCall &call, const FbFrontendDev &fe, int B, int total_frames) {
  hipStream_t s = e->stream;
  const int16_t *wav = nullptr;
  FBCHK(transformed_wav(e, call, e->h_wav_off.data(), B, &wav));
  e->fe_wav = wav;
  e->have_route = true;
  e->route[3] = e->t_max;
  e->route[4] = B;
  // Kaldi's dither: the dithered form of the same kernel, keyed by the call's point
  const bool dither = e->cfg.dither > 0.0;
  const FbDitherKey dith = fb_dither_key(call.pt, e->cfg.dither);
  const FbDitherKey *dk = dither ? &dith : nullptr;
  const int32_t *ut = dither ? e->frame_ut.as<int32_t>() : nullptr;
  if (fe.mfcc_f32 && fb_launch_mfcc_f32(s, fe, e->melw_n, wav, e->frame_rec.as<int32_t>(), total_frames,
                                        e->mfcc.as<float>(), e->uni_T, e->uni_n, e->h_wav_off[0], &e->shape_mfcc, dk, ut))
    e->route[0] = fe.L / 32 >= 12 ? (dither ? FB_ROUTE_MFCC_F32_12_DITHER : FB_ROUTE_MFCC_F32_12)
                                  : (dither ? FB_ROUTE_MFCC_F32_0_DITHER : FB_ROUTE_MFCC_F32_0);  // (fb_launch_mfcc_f32's instantiation rule)
  else
    e->route[0] = fb_launch_mfcc(s, fe, e->melw_n, wav, e->wav_off.as<int64_t>(), e->frame_off.as<int>(),
                                 e->frame_rec.as<int32_t>(), B, total_frames, e->mfcc.as<float>(), dk, ut);
  return FB_OK;
}
// the point of a scoring call outside an attack (fb_score_*, fb_gmm_acc_stats, fb_debug_mfcc / _feats): the engine's seed,
// stream 0xFFFFFFFF, epoch = the scoring-call serial, which the call consumes
static FbRngPoint scoring_call_point(fb_engine *e) { return FbRngPoint{e->dither_seed, 0xFFFFFFFFu, e->dither_serial++, 0}; }

// mfcc -> VAD (+ row offsets) -> deltas -> CMVN -> voiced-row compaction
static int run_post_mfcc(fb_engine *e, const FbFrontendDev &fe, int B) {
  hipStream_t s = e->stream;
  e->route[1] = FB_ROUTE_NONE;  // (until a chain is enqueued: a call that fails on the way reports none)
  e->route[2] = FB_ROUTE_NONE;
  if (!e->vad_counter.p) {
    FBCHK(e->vad_counter.ensure(sizeof(int)));
    HIPCHK(hipMemsetAsync(e->vad_counter.p, 0, sizeof(int), s));
  }
  // make_mfcc.sh's `copy-feats --compress=true`: what VAD / deltas / CMVN read.  The one-launch kernel below takes the
  // round trip along on its LDS copy of the matrix when it can (utterances of up to 512 frames: every NES batch)
  const bool cm = e->cfg.compress_feats != 0;
  const bool cm_fused = cm && fb_fuse_part(e, 0) && fb_vad_delta_cmvn_compresses(e->t_max);
  // (out of place -- every workgroup of k_feat_compress reduces the header from the whole input matrix --, then the two
  //  buffers swap roles: e->mfcc is the matrix the later stages and fb_debug_mfcc read)
  auto compress = [&]() -> int {
    FBCHK(e->mfcc_cm.ensure(sizeof(float) * (size_t)e->h_frame_off[B] * fe.nc));
    e->route[2] = fb_launch_feat_compress(s, fe, e->mfcc.as<float>(), e->mfcc_cm.as<float>(), e->frame_off.as<int>(), B, e->t_max);
    std::swap(e->mfcc, e->mfcc_cm);
    return FB_OK;
  };
  if (cm && !cm_fused) FBCHK(compress());
  {  // every utterance fits the CMVN window (all NES batches): VAD, deltas, CMVN and the row offsets in one launch
    const size_t had = e->vad_pub.cap, had_p = e->vad_part.cap;
    FBCHK(e->vad_pub.ensure(sizeof(unsigned long long) * (size_t)B));
    FBCHK(e->vad_part.ensure(sizeof(double) * fb_vad_parts_doubles(fe, B)));
    if (e->vad_pub.cap != had || e->vad_part.cap != had_p || e->vad_epoch == 0xffffffffu || e->vad_part_B != B || e->vad_part_dim != fe.dim) {
      // fresh buffers, another slot layout, or the epoch counter is about to wrap
      HIPCHK(hipMemsetAsync(e->vad_pub.p, 0, e->vad_pub.cap, s));
      HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->vad_part.p), (int)FB_VAD_SENTINEL32, e->vad_part.cap / 4, s));
      e->vad_epoch = 0;
      e->vad_p_launches = 0;
      e->vad_part_B = B;
      e->vad_part_dim = fe.dim;
    }
    // without the CompressedMatrix phase an utterance is split over four workgroups (k_vad_delta_cmvn_p); FB_VAD_WHOLE=1
    // keeps the one-workgroup kernel (A/B; same results bit for bit)
    if (fb_fuse_part(e, 0) && !cm_fused && getenv("FB_VAD_WHOLE") == nullptr &&
        fb_launch_vad_delta_cmvn_p(s, fe, e->mfcc.as<float>(), e->frame_off.as<int>(), B, e->t_max, e->vad_epoch + 1,
                                   e->vad_counter.as<int>(), e->vad_pub.as<unsigned long long>(), e->tv.as<int>(),
                                   e->row_off.as<int>(), e->feats.as<float>(), e->vad_part.as<double>(), e->vad_p_launches,
                                   e->fuse_opt != 0)) {
      e->vad_epoch += 1;
      e->vad_p_launches += 1;
      e->route[1] = FB_ROUTE_CHAIN_SPLIT;
      return FB_OK;
    }
    if (fb_fuse_part(e, 0) && fb_launch_vad_delta_cmvn(s, fe, e->mfcc.as<float>(), e->frame_off.as<int>(), B, e->t_max, e->vad_epoch + 1,
                                             e->vad_counter.as<int>(), e->vad_pub.as<unsigned long long>(), e->tv.as<int>(),
                                             e->row_off.as<int>(), e->feats.as<float>(), cm_fused ? e->mfcc.as<float>() : nullptr)) {
      e->vad_epoch += 1;
      e->route[1] = FB_ROUTE_CHAIN_WHOLE;
      if (cm_fused) e->route[2] = FB_ROUTE_CM_FUSED;
      return FB_OK;
    }
    if (cm_fused) FBCHK(compress());  // (the batch did not qualify)
  }
  fb_launch_vad(s, fe, e->mfcc.as<float>(), e->frame_off.as<int>(), B, e->vrank.as<int>(), e->tv.as<int>(),
                e->vad_counter.as<int>(), e->row_off.as<int>());
  if (fb_launch_delta_cmvn(s, fe, e->mfcc.as<float>(), e->frame_off.as<int>(), e->vrank.as<int>(),
                           e->row_off.as<int>(), B, e->t_max, e->feats.as<float>())) {
    e->route[1] = FB_ROUTE_CHAIN_VAD_DC;
    return FB_OK;
  }
  const int total_frames = e->h_frame_off[B], total_chunks = e->h_chunk_off[B];
  FBCHK(e->dfeat.ensure(sizeof(float) * (size_t)total_frames * fe.dim));
  FBCHK(e->chunk_sum.ensure(sizeof(double) * (size_t)total_chunks * fe.dim));
  fb_launch_deltas(s, fe, e->mfcc.as<float>(), e->frame_off.as<int>(), e->chunk_off.as<int>(), B, total_chunks,
                   e->dfeat.as<float>(), e->chunk_sum.as<double>());
  fb_launch_cmvn(s, fe, e->dfeat.as<float>(), e->frame_off.as<int>(), e->chunk_off.as<int>(),
                 e->chunk_sum.as<double>(), e->vrank.as<int>(), e->row_off.as<int>(), B, total_chunks, e->any_long,
                 e->feats.as<float>());
  e->route[1] = e->any_long ? FB_ROUTE_CHAIN_SLIDING : FB_ROUTE_CHAIN_SEPARATE;
  return FB_OK;
}

// Feature compression (fb_set_feature_compression): k-means over the voiced rows of every utterance row of the batch, one
// launch between the front end and the back end.  It reads e->feats / e->row_off and writes e->feats_fc / e->row_off_fc; the
// two pairs then swap roles (the mfcc / mfcc_cm idiom of run_post_mfcc), so every launch behind it -- the GMM and gselect
// kernels, the finalising launches, the i-vector chain -- takes the compressed rows and their counts from where it always did.
// With r = call.replicas() > 1 B counts the replicated rows and row b * r + j draws replica j's initialisation.
static int feature_compress(fb_engine *e, const FbScoreCall &call, int B, int total_frames) {
  const int D = e->fe.dim;
  FBCHK(e->feats_fc.ensure(sizeof(float) * (size_t)total_frames * D));
  FBCHK(e->row_off_fc.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(e->feco_ws.ensure(sizeof(int) * (size_t)FB_FECO_WS_INTS * (size_t)(total_frames > 0 ? total_frames : 1)));
  const FbFeco fc = fb_feco_key(call.pt, e->feco_ratio, e->feco_iters, call.replicas());
  if (call.keep_feco) {  // (FbScoreCall::keep_feco: the white-box call; k <= T per row, so the counts fit a buffer of the labels' size)
    FBCHK(e->wb_feco_label.ensure(sizeof(int) * (size_t)(total_frames > 0 ? total_frames : 1)));
    FBCHK(e->wb_feco_cnt.ensure(sizeof(int) * (size_t)(total_frames > 0 ? total_frames : 1)));
    FBCHK(e->wb_feco_k.ensure(sizeof(int) * (size_t)B));
  }
  if (!fb_launch_feature_compress(e->stream, fc, D, e->feats.as<float>(), e->row_off.as<int>(), B, e->t_max,
                                  e->feats_fc.as<float>(), e->row_off_fc.as<int>(), e->feco_ws.as<int>(), call.stop,
                                  call.keep_feco ? e->wb_feco_label.as<int>() : nullptr, call.keep_feco ? e->wb_feco_cnt.as<int>() : nullptr,
                                  call.keep_feco ? e->wb_feco_k.as<int>() : nullptr))
    return fb_fail(FB_E_HIP, "k_feature_compress: the dynamic-LDS opt-in failed");
  std::swap(e->feats, e->feats_fc);
  std::swap(e->row_off, e->row_off_fc);
  return FB_OK;
}

// The x-vector chain (xvector_kernels.hip) on e->feats / e->row_off: frame layers 0 .. min(upto, n_layers - 1), then -- with
// upto >= n_layers -- pooling into xv_stats and, with upto > n_layers, the segment affine into iv_ivec.  *last (nullable): the
// buffer that holds the last frame layer run.  Purely asynchronous.
// keep_mask: every layer run also leaves its ReLU decisions in e->xv_mask[l] (the white-box backward's)
static int run_xvector(fb_engine *e, int B, int total_frames, int upto, const float **last, bool keep_mask = false) {
  const FbXvDev &xv = e->xv;
  hipStream_t s = e->stream;
  const size_t rows = (size_t)(total_frames > 0 ? total_frames : 1);
  FBCHK(e->xv_rowinfo.ensure(sizeof(int2) * rows));
  FBCHK(e->xv_amax.ensure(sizeof(float) * rows));
  for (int i = 0; i < 2; ++i) FBCHK(e->xv_act[i].ensure(sizeof(float) * rows * (size_t)xv.max_width));
  FBCHK(e->xv_stats.ensure(sizeof(double) * (size_t)B * 2 * xv.P));
  FBCHK(e->iv_ivec.ensure(sizeof(double) * (size_t)B * xv.R));
  if (keep_mask) {
    for (int l = 0; l < xv.n_layers; ++l) FBCHK(e->xv_mask[l].ensure(rows * (size_t)xv.layer[l].dout));
    FBCHK(e->xv_mask_rows.ensure(sizeof(int)));
  }
  const int *n_rows = e->row_off.as<int>() + B;
  if (keep_mask) {
    HIPCHK(hipMemcpyAsync(e->xv_mask_rows.p, n_rows, sizeof(int), hipMemcpyDeviceToDevice, s));
    e->xv_mask_B = B;
  }
  fb_launch_xv_rowinfo(s, e->row_off.as<int>(), B, e->xv_rowinfo.as<int2>());
  const float *in = e->feats.as<float>();
  for (int l = 0; l < xv.n_layers && l <= upto; ++l) {
    float *out = e->xv_act[l & 1].as<float>();
    fb_launch_xv_rowmax(s, in, xv.layer[l].din, n_rows, total_frames, e->xv_amax.as<float>());
    fb_launch_xv_affine(s, xv.layer[l], in, e->xv_amax.as<float>(), e->xv_rowinfo.as<int2>(), n_rows, total_frames, out,
                        keep_mask ? e->xv_mask[l].as<unsigned char>() : nullptr);
    in = out;
  }
  if (last) *last = in;
  if (upto >= xv.n_layers) fb_launch_xv_pool(s, in, xv.P, e->row_off.as<int>(), B, e->xv_stats.as<double>());
  if (upto > xv.n_layers) fb_launch_xv_segment(s, xv, e->xv_stats.as<double>(), B, e->iv_ivec.as<double>());
  return FB_OK;
}

// wav (device) + offsets (device) -> raw[B][M] (device).  Purely asynchronous.
static int run_scoring(fb_engine *e, FbScoreCall &call, int B, int total_frames) {
  FBCHK(e->mfcc.ensure(sizeof(float) * (size_t)total_frames * e->fe.nc));
  FBCHK(e->vrank.ensure(sizeof(int) * (size_t)total_frames));
  FBCHK(e->tv.ensure(sizeof(int) * (size_t)B));
  FBCHK(e->row_off.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)total_frames * e->fe.dim));
  const int n_chunks = choose_chunks(e->gmm, total_frames, e->kind == 0);
  if (e->kind == 0) {
    FBCHK(e->part_m.ensure(sizeof(float) * (size_t)n_chunks * e->gmm.M * total_frames));
    FBCHK(e->part_s.ensure(sizeof(float) * (size_t)n_chunks * e->gmm.M * total_frames));
  }
  FBCHK(e->raw.ensure(sizeof(double) * (size_t)B * e->n_out));
  hipStream_t s = e->stream;
  choose_launch_shape(e);
  // the kernel-argument structs as this call's launches take them (by value): the engine's, with the call's stop flag
  FbFrontendDev fe = e->fe;
  FbGmmDev g = e->gmm;
  fe.stop = g.stop = call.stop;
  if (!call.feats_given) {
    FBCHK(launch_mfcc(e, call, fe, B, total_frames));
    FBCHK(run_post_mfcc(e, fe, B));
    if (e->feco_iters > 0) FBCHK(feature_compress(e, call, B, total_frames));
  }
  if (e->kind == 0) {
    // A GPU shared by three or more attacks (fb_set_fused_chain(e, 0)): k_gmm_fx2w takes a whole compute unit per workgroup (one
    // wave per SIMD with the full register file), and so does k_mfcc_f32 (four waves per SIMD at 122 registers) -- with a
    // workgroup on nearly every unit nothing of the other attacks' front-ends runs while it does, and the chip alternated
    // between one attack's k_gmm_fx2w and the others' k_mfcc_f32 / VAD (kernel trace, round 6: 62 + 19 us per iteration).
    // With HALF as many workgroups, each scoring two component chunks one after the other (the same partial sums, bit for
    // bit), the kernel alone is slower -- 92 us against 60 -- but the other half of the chip carries the other attacks'
    // front-ends meanwhile: 12 319 -> 12 800 - 13 000 it/s (tools/profile/r06_fewer_wg.sh).  choose_launch_shape decides it.
    FBCHK(time_begin(e));
    fb_launch_gmm(s, g, e->feats.as<float>(), e->row_off.as<int>() + B, total_frames, n_chunks,
                  e->part_m.as<float>(), e->part_s.as<float>(), &e->shape_gmm);
    FBCHK(time_end(e));
    if (!call.defer_finalize)
      fb_launch_gmm_finalize(s, g, e->part_m.as<float>(), e->part_s.as<float>(), total_frames, n_chunks,
                             e->row_off.as<int>(), B, e->raw.as<double>());
  } else if (e->kind == 2) {
    // x-vector systems: the layers, pooling and the segment affine, then the back end as its own launch; the caller's
    // k_loss / k_loss_eot / k_vote follows (the i-vector branch's "split" tail)
    FB_DBG_SYNC(e, "front-end");
    FBCHK(time_begin(e));
    FBCHK(run_xvector(e, B, total_frames, e->xv.n_layers + 1, nullptr, call.keep_xv_mask));
    FBCHK(time_end(e));
    fb_launch_iv_backend(s, e->iv, e->iv_ivec.as<double>(), B, e->raw.as<double>());
    FB_DBG_SYNC(e, "backend");
  } else {
    const FbIvDev &iv = e->iv;
    const int64_t Q = (int64_t)iv.C * iv.D;
    FBCHK(e->iv_ll.ensure(sizeof(float) * (size_t)total_frames * iv.Cpad));
    FBCHK(e->iv_sel.ensure(sizeof(int) * (size_t)total_frames * iv.nsel));
    FBCHK(e->iv_post.ensure(sizeof(float) * (size_t)total_frames * iv.nsel));
    {
      const size_t cap = e->iv_bws.cap;
      FBCHK(e->iv_bws.ensure(sizeof(int) * (fb_iv_bucket_ws_ints(iv, total_frames) + 8)));
      if (e->iv_bws.cap != cap) HIPCHK(hipMemsetAsync(e->iv_bws.p, 0, e->iv_bws.cap, s));  // flags start clean
    }
    FBCHK(e->iv_pairs.ensure(sizeof(int) * (size_t)total_frames * iv.nsel));
    FBCHK(e->iv_llf.ensure(sizeof(float) * (size_t)total_frames * iv.nsel));
    const int Bpad = (B + 31) / 32 * 32;
    {
      const size_t cg = e->iv_gamma.cap, cx = e->iv_X.cap;
      // one extra, always-zero row behind each matrix: the DMA contraction points padding rows of its last K stage at it
      FBCHK(e->iv_gamma.ensure(sizeof(double) * (size_t)Bpad * (iv.C + 1)));
      FBCHK(e->iv_X.ensure(sizeof(double) * (size_t)Bpad * (Q + 1)));
      if (Bpad != e->iv_Bpad || cg != e->iv_gamma.cap || cx != e->iv_X.cap || iv.C != e->iv_zeroC) {  // zero the padding once
        HIPCHK(hipMemsetAsync(e->iv_gamma.p, 0, sizeof(double) * (size_t)Bpad * (iv.C + 1), s));
        HIPCHK(hipMemsetAsync(e->iv_X.p, 0, sizeof(double) * (size_t)Bpad * (Q + 1), s));
        e->iv_zeroC = iv.C;
        e->iv_Bpad = Bpad;
      }
    }
    FBCHK(e->iv_linp.ensure(sizeof(double) * (size_t)e->iv_kchunks * B * iv.R));
    FBCHK(e->iv_quad.ensure(sizeof(double) * (size_t)B * iv.triR));
    {  // the right-hand side row each factorisation carries along, + a row of zeros behind them (k_iv_solve_ll points
       // the operand rows that do not exist at it)
      const size_t had = e->iv_A.cap;
      FBCHK(e->iv_A.ensure(sizeof(double) * ((size_t)B * iv.R + iv.R + 64)));
      if (e->iv_A.cap != had || e->iv_A_B != B) {
        HIPCHK(hipMemsetAsync(e->iv_A.p, 0, e->iv_A.cap, s));
        e->iv_A_B = B;
      }
    }
    {  // k_iv_solve_rw's slot sets (sentinel-filled), progress words and ticket; k_iv_solve_ll uses the first set only
      const size_t had = e->iv_linv.cap, had_p = e->iv_prog.cap;
      FBCHK(e->iv_linv.ensure(sizeof(double) * fb_iv_solve_rw_linv_doubles(iv, B)));
      FBCHK(e->iv_prog.ensure(sizeof(unsigned) * fb_iv_solve_rw_prog_words(iv, B)));
      if (!e->iv_ticket.p) {
        FBCHK(e->iv_ticket.ensure(sizeof(int)));
        HIPCHK(hipMemsetAsync(e->iv_ticket.p, 0, sizeof(int), s));
      }
      if (e->iv_linv.cap != had || e->iv_prog.cap != had_p || e->iv_rw_B != B || e->iv_rw_R != iv.R || e->iv_rw_epoch >= 0xfffff0u ||
          (e->iv_linv_dirty && fb_iv_use_rw(e))) {
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->iv_linv.p), (int)0x7ff87ff8u, e->iv_linv.cap / 4, s));
        HIPCHK(hipMemsetAsync(e->iv_prog.p, 0, e->iv_prog.cap, s));
        e->iv_rw_epoch = 0;
        e->iv_rw_B = B;
        e->iv_rw_R = iv.R;
        e->iv_linv_dirty = false;
      }
    }
    FBCHK(e->iv_ivec.ensure(sizeof(double) * (size_t)B * iv.R));
    FBCHK(e->iv_fail.ensure(sizeof(int)));
    FBCHK(e->iv_active.ensure(sizeof(int) * (size_t)(iv.C + 1)));
    FB_DBG_SYNC(e, "front-end");
    // gmm-gselect: threshold selection in the matrix-core kernel (round 6) with the dump + k_iv_select launches behind
    // it as its rescue -- they return at once unless a survivor list overflowed --, or the dump alone where the
    // threshold path does not apply (small models, the bf16 mode, FB_IV_GSEL_DUMP=1)
    const int *sel_gate = nullptr;
    FbGmmDev gd = g;
    const int sel_chunks = fb_gsel_chunks(n_chunks);
    const int wide_chunks = fb_gsel_wide_chunks(g, iv.nsel, total_frames);
    e->gs_last_path = 0;
    e->gs_last_chunks = 0;
    if (!e->gs_flag.p && (wide_chunks > 0 || fb_gsel_applies(g, iv.nsel, sel_chunks))) {
      FBCHK(e->gs_flag.ensure(sizeof(int)));
      HIPCHK(hipMemsetAsync(e->gs_flag.p, 0, sizeof(int), s));
    }
    if (wide_chunks > 0) {
      // k_gsel_w (gmm_wide_kernel.hip): the records of pass B go where the dump's values would (rows x C floats, sparsely
      // written); nothing can overflow, so neither the dump nor k_iv_select is launched at all
      FBCHK(e->gs_max.ensure(sizeof(float) * (size_t)total_frames * 2 * g.n_tiles));
      FBCHK(e->gs_tau.ensure(sizeof(float) * (size_t)total_frames));
      FBCHK(e->gs_cnt.ensure(sizeof(int) * (size_t)total_frames * wide_chunks));
      FBCHK(e->gs_gid.ensure((size_t)total_frames * 2 * g.n_tiles));
      fb_launch_gsel_wide(s, g, e->feats.as<float>(), e->row_off.as<int>() + B, total_frames, wide_chunks, iv.nsel, e->gs_max.as<float>(),
                          e->gs_tau.as<float>(), e->iv_ll.as<float>(), e->gs_gid.as<unsigned char>(), e->gs_cnt.as<int>(),
                          e->gs_flag.as<int>(), e->iv_sel.as<int>(), fb_iv_bucket_cnt(iv, e->iv_bws.as<int>()), iv.Cpad);
      FB_DBG_SYNC(e, "gsel_wide");
      e->gs_last_path = 2;
      e->gs_last_chunks = wide_chunks;
    } else {
      if (fb_gsel_applies(g, iv.nsel, sel_chunks)) {
        const int cap = fb_gsel_cap(sel_chunks);
        FBCHK(e->gs_max.ensure(sizeof(float) * (size_t)total_frames * 2 * g.n_tiles));
        FBCHK(e->gs_tau.ensure(sizeof(float) * (size_t)total_frames));
        FBCHK(e->gs_list.ensure(sizeof(unsigned long long) * (size_t)total_frames * sel_chunks * cap));
        FBCHK(e->gs_cnt.ensure(sizeof(int) * (size_t)total_frames * sel_chunks));
        fb_launch_gsel(s, g, e->feats.as<float>(), e->row_off.as<int>() + B, total_frames, sel_chunks, iv.nsel, e->gs_max.as<float>(),
                       e->gs_tau.as<float>(), e->gs_list.as<unsigned long long>(), e->gs_cnt.as<int>(), e->gs_flag.as<int>(),
                       e->iv_sel.as<int>());
        FB_DBG_SYNC(e, "gsel");
        sel_gate = e->gs_flag.as<int>();
        gd.only_if = sel_gate;
        e->gs_last_path = 1;
        e->gs_last_chunks = sel_chunks;
      }
      fb_launch_gmm_dump(s, gd, e->feats.as<float>(), e->row_off.as<int>() + B, total_frames, n_chunks,
                         e->iv_ll.as<float>(), &e->shape_gmm);
      FB_DBG_SYNC(e, "gmm_dump");
    }
    fb_launch_iv_select_post(s, iv, e->iv_ll.as<float>(), e->feats.as<float>(), e->row_off.as<int>() + B,
                             total_frames, e->iv_sel.as<int>(), e->iv_post.as<float>(), e->iv_bws.as<int>(),
                             e->iv_pairs.as<int>(), e->iv_llf.as<float>(), sel_gate, wide_chunks == 0, wide_chunks == 0);
    FB_DBG_SYNC(e, "select_post");
    fb_launch_iv_stats(s, iv, e->feats.as<float>(), e->row_off.as<int>(), e->iv_pairs.as<int>(), e->iv_bws.as<int>(),
                       e->iv_post.as<float>(), B, Bpad, e->iv_gamma.as<double>(), e->iv_X.as<double>());
    FB_DBG_SYNC(e, "stats");
    // bench timing of the T-matrix contraction (the two k_iv_contract_gemm launches)
    FBCHK(time_begin(e));
    fb_launch_iv_contract(s, iv, e->iv_gamma.as<double>(), e->iv_X.as<double>(), B, Bpad, e->iv_kchunks,
                          e->iv_bws.as<int>() + 3 * (size_t)iv.C + 2, e->iv_active.as<int>(),
                          e->iv_active.as<int>() + iv.C, e->iv_linp.as<double>(), e->iv_quad.as<double>(),
                          e->iv_fail.as<int>());
    FBCHK(time_end(e));
    FB_DBG_SYNC(e, "contract");
    // the solve below factorises quad in place: the white-box adjoint solve takes the matrix from this copy
    if (call.keep_iv_quad)
      HIPCHK(hipMemcpyAsync(e->wb_iv_quad.p, e->iv_quad.p, sizeof(double) * (size_t)std::min(call.keep_iv_quad_rows, B) * (size_t)iv.triR,
                            hipMemcpyDeviceToDevice, s));
    // the back-end and, inside the NES loop, the loss body run in the solve kernels' tail (fb_iv_tail.h); FB_IV_TAIL=split
    // keeps the separate k_iv_backend / k_loss launches (A/B, tests: same numbers bit for bit)
    FbIvTail tail = {};
    {
      const char *tv_env = getenv("FB_IV_TAIL");
      const bool split = (tv_env && strcmp(tv_env, "split") == 0) || call.replicas() > 1 || call.play > 0;  // (fb_set_eot: k_loss_eot follows k_iv_backend)
      if (!e->iv_tail_counter.p) {
        FBCHK(e->iv_tail_counter.ensure(sizeof(int)));
        HIPCHK(hipMemsetAsync(e->iv_tail_counter.p, 0, sizeof(int), s));
      }
      // (LDA dimension > 512: the tail's 512 threads would take two l each in the PLDA partial sums where k_iv_backend's
      //  1024 take one -- a different summation grouping; such a system keeps the separate launch and its rounding)
      if (!split && iv.L <= 512) {
        if (call.tail_loss && fb_iv_tail_takes_loss(B)) {
          tail = *call.tail_loss;
          tail.loss = 1;
          // (the voiced-frame counts as THIS batch's front end wrote them: e->tv grows with the batch up there, so a pointer
          //  the caller took before the call may be to the buffer that was freed)
          tail.tv = e->tv.as<int>();
        }
        tail.backend = 1;
        tail.llr = e->raw.as<double>();
        tail.counter = e->iv_tail_counter.as<int>();
      }
    }
    call.tail_loss_done = tail.loss != 0;
    FBCHK(time_begin(e, 2));
    // FB_IV_SOLVE=ll keeps the one-workgroup-per-matrix kernel (A/B); otherwise the row-wise kernel whenever its grid of
    // 5 workgroups per matrix is resident at once, which is when the chip has idle units to give it
    if (fb_iv_use_rw(e) &&
        fb_launch_iv_solve_rw(s, iv, e->iv_quad.as<double>(), e->iv_linp.as<double>(), e->iv_kchunks, B, e->iv_A.as<double>(),
                              e->iv_linv.as<double>(), e->iv_ivec.as<double>(), e->iv_fail.as<int>(), e->iv_prog.as<unsigned>(),
                              e->iv_ticket.as<int>(), e->iv_rw_epoch + 1, tail)) {
      e->iv_rw_epoch += 1;
    } else {
      e->iv_linv_dirty = true;
      fb_launch_iv_solve_ll(s, iv, e->iv_quad.as<double>(), e->iv_linp.as<double>(), e->iv_kchunks, B,
                            e->iv_A.as<double>(), e->iv_linv.as<double>(), e->iv_ivec.as<double>(), e->iv_fail.as<int>(), tail);
    }
    FBCHK(time_end(e, 2));
    FB_DBG_SYNC(e, "solve");
    if (!tail.backend) fb_launch_iv_backend(s, iv, e->iv_ivec.as<double>(), B, e->raw.as<double>());
    FB_DBG_SYNC(e, "backend");
  }
  HIPCHK(hipGetLastError());
  e->last_total_frames = total_frames;
  e->last_B = B;
  e->last_chunks = n_chunks;
  e->scored_utts += B;
  e->scored_frames += total_frames;
  return FB_OK;
}

static int ensure_host_tv(fb_engine *e, int B) {
  if ((size_t)B <= e->h_tv_cap) return FB_OK;
  if (e->h_tv) (void)hipHostFree(e->h_tv);
  e->h_tv = nullptr;
  e->h_tv_cap = 0;
  HIPCHK(hipHostMalloc((void **)&e->h_tv, sizeof(int) * (size_t)(B + 64), hipHostMallocDefault));
  e->h_tv_cap = (size_t)B + 64;
  return FB_OK;
}

static int finish_score(fb_engine *e, int B, double *raw, int *tv) {
  FBCHK(ensure_host_tv(e, B));
  FBCHK(d2h(e, raw, e->raw.p, sizeof(double) * (size_t)B * e->n_out));
  HIPCHK(hipMemcpyAsync(e->h_tv, e->tv.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, e->stream));
  FBCHK(sync_stream(e));
  if (e->kind == 1) {
    int fail = 0;
    HIPCHK(hipMemcpy(&fail, e->iv_fail.p, sizeof(int), hipMemcpyDeviceToHost));
    if (fail) return fb_fail(FB_E_ARG, "i-vector system of utterance %d is not positive definite", fail - 1);
  }
  int bad = -1;
  for (int b = 0; b < B; ++b) {
    if (tv) tv[b] = e->h_tv[b];
    e->voiced_frames += e->h_tv[b];
    if (e->h_tv[b] <= 0 && bad < 0) bad = b;
  }
  if (bad >= 0) return fb_fail(FB_E_NO_VOICED, "utterance %d has no voiced frames", bad);
  return FB_OK;
}

extern "C" int fb_score_i16(fb_engine *e, const int16_t *wav, const int64_t *off, int B, double *raw, int *tv) {
  if (!e || !wav || !off || !raw || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const int64_t total = off[B] - off[0];
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)total));
  FBCHK(h2d(e, e->wav.p, wav, sizeof(int16_t) * (size_t)total));
  FBCHK(prepare_batch(e, off, B));
  e->cached_B = -1;
  FbScoreCall call{scoring_call_point(e)};
  FBCHK(run_scoring(e, call, B, e->h_frame_off[B]));
  return finish_score(e, B, raw, tv);
}

extern "C" int fb_score_f64(fb_engine *e, const double *audio, const int64_t *off, int B, int bits, double *raw,
                            int *tv) {
  if (!e || !audio || !off || !raw || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported", bits);
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  const int64_t total = off[B];
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)total));
  FBCHK(e->stage_f64.ensure(sizeof(double) * (size_t)total));
  FBCHK(h2d(e, e->stage_f64.p, audio, sizeof(double) * (size_t)total));
  fb_launch_quantize(e->stream, e->stage_f64.as<double>(), total, bits, e->wav.as<int16_t>());
  FBCHK(prepare_batch(e, off, B));
  e->cached_B = -1;
  FbScoreCall call{scoring_call_point(e)};
  FBCHK(run_scoring(e, call, B, e->h_frame_off[B]));
  return finish_score(e, B, raw, tv);
}

extern "C" int fb_system_scores(fb_engine *e, const double *raw, int B, double *scores) {
  if (!e || !raw || !scores || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  const int M = e->n_out;
  if (e->task == FB_TASK_CSI || e->kind != 0) {
    for (int b = 0; b < B; ++b)
      for (int m = 0; m < M; ++m)
        scores[(size_t)b * M + m] = (raw[(size_t)b * M + m] - e->h_zmean[m]) / e->h_zstd[m];
  } else {
    const int S = M - 1;
    for (int b = 0; b < B; ++b)
      for (int s = 0; s < S; ++s) scores[(size_t)b * S + s] = raw[(size_t)b * M + 1 + s] - raw[(size_t)b * M];
  }
  return FB_OK;
}


// ----------------------------------------------------------------- i-vector
// fb_load_ivector's argument checks.  e == nullptr (fb_debug_prepare_ivector): no front end to agree with, no task
static int check_ivector_args(const fb_engine *e, const fb_ivector_system *sy, int task) {
  if (!sy) return fb_fail(FB_E_ARG, "null argument");
  if (e && task != FB_TASK_OSI && task != FB_TASK_CSI && task != FB_TASK_SV) return fb_fail(FB_E_ARG, "bad task");
  const int C = sy->C, D = sy->D, R = sy->R, L = sy->L, S = sy->S;
  if (C <= 0 || D <= 0 || R <= 0 || L <= 0 || S <= 0) return fb_fail(FB_E_ARG, "bad i-vector system shape");
  if (e && (!e->have_fe || e->fe.dim != D)) return fb_fail(FB_E_ARG, "UBM dim %d != front-end feature dim %d", D, e->have_fe ? e->fe.dim : -1);
  if (R > 512 || L > 512 || D > 80 || D > 255) return fb_fail(FB_E_ARG, "unsupported sizes R=%d L=%d D=%d (R,L <= 512, D <= 80)", R, L, D);
  if (C > 4096) return fb_fail(FB_E_LIMIT, "at most 4096 Gaussians in the i-vector UBM (got %d)", C);
  if (S > 60) return fb_fail(FB_E_ARG, "at most 60 enrolled speakers per engine");
  if (e && task == FB_TASK_SV && S != 1) return fb_fail(FB_E_ARG, "SV takes exactly one enrolled speaker");
  if (sy->num_gselect <= 0 || sy->num_gselect > 64 || sy->num_gselect > C) return fb_fail(FB_E_ARG, "num_gselect must be in [1, min(64, C)]");
  if (sy->lda_cols != R && sy->lda_cols != R + 1) return fb_fail(FB_E_ARG, "transform.mat must have R or R+1 columns");
  if (!sy->fg_weights || !sy->fg_means_invcovars || !sy->fg_inv_covars || !sy->ie_M || !sy->ie_sigma_inv ||
      !sy->mean_vec || !sy->lda || !sy->plda_mean || !sy->plda_transform || !sy->plda_psi || !sy->enrolled ||
      !sy->z_mean || !sy->z_std)
    return fb_fail(FB_E_ARG, "null array in fb_ivector_system");
  return FB_OK;
}
static int prepare_ivector(const fb_ivector_system *sy, FbIvPrepared *out) {
  std::string err;
  const int rc = fb_prepare_ivector(sy, out, &err);
  return rc == FB_OK ? FB_OK : fb_fail(rc, "%s", err.c_str());
}

extern "C" int fb_load_ivector(fb_engine *e, const fb_ivector_system *sy, int task) {
  if (!e) return fb_fail(FB_E_ARG, "null argument");
  FBCHK(check_ivector_args(e, sy, task));
  const int C = sy->C, D = sy->D, R = sy->R, L = sy->L, S = sy->S;
  // the system's own tables and the images of its diagonalised UBM (the GMM path, M = 1), all on the host: a refused
  // call leaves the engine and the device as they were
  FbIvPrepared p;
  FbGmmPrepared pg;
  FBCHK(prepare_ivector(sy, &p));
  FBCHK(prepare_gmm(e, 1, C, D, p.dg_gc.data(), p.dg_miv.data(), p.dg_iv.data(), &pg));
  const int triD = p.triD, triR = p.triR;
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  FBCHK(commit_gmm(e, pg, p.dg_gc.data(), p.dg_miv.data(), p.dg_iv.data()));
  // ---- ensure: the full UBM {gconsts, means_invcovars, inv_covars}, its images, the extractor, the back end
  const size_t n_gc = C, n_mic = (size_t)C * D, n_P = (size_t)C * triD, nM = (size_t)C * D * R;
  DevBuf dM, dS;  // the extractor's M and Sigma^-1 as they come: inputs of the derive launch, freed on return
  FBCHK(e->iv_fg.ensure(sizeof(float) * (n_gc + n_mic + n_P)));
  FBCHK(e->iv_tri.ensure(p.tri.size()));
  FBCHK(e->iv_fg64.ensure(sizeof(double) * p.fg64.size()));
  if (!p.fgL.empty()) FBCHK(e->iv_fgL.ensure(sizeof(double) * p.fgL.size()));
  FBCHK(dM.ensure(sizeof(double) * nM));
  FBCHK(dS.ensure(sizeof(double) * (size_t)C * triD));
  FBCHK(e->iv_sim.ensure(sizeof(double) * nM));
  FBCHK(e->iv_u.ensure(sizeof(double) * (size_t)C * triR));
  FBCHK(e->iv_backend.ensure(sizeof(double) * p.backend.size()));
  FBCHK(e->zmean.ensure(sizeof(double) * S));
  FBCHK(e->zstd.ensure(sizeof(double) * S));
  // ---- upload
  float *base = e->iv_fg.as<float>();
  HIPCHK(hipMemcpy(base, p.fg_gc.data(), sizeof(float) * n_gc, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(base + n_gc, sy->fg_means_invcovars, sizeof(float) * n_mic, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(base + n_gc + n_mic, sy->fg_inv_covars, sizeof(float) * n_P, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->iv_tri.p, p.tri.data(), p.tri.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->iv_fg64.p, p.fg64.data(), sizeof(double) * p.fg64.size(), hipMemcpyHostToDevice));
  if (!p.fgL.empty()) HIPCHK(hipMemcpy(e->iv_fgL.p, p.fgL.data(), sizeof(double) * p.fgL.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->iv_backend.p, p.backend.data(), sizeof(double) * p.backend.size(), hipMemcpyHostToDevice));
  e->h_zmean.assign(sy->z_mean, sy->z_mean + S);
  e->h_zstd.assign(sy->z_std, sy->z_std + S);
  HIPCHK(hipMemcpy(e->zmean.p, e->h_zmean.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->zstd.p, e->h_zstd.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  // the extractor: Sigma^-1 M and U derived on the device (IvectorExtractor::ComputeDerivedVars)
  HIPCHK(hipMemcpy(dM.p, sy->ie_M, sizeof(double) * nM, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dS.p, sy->ie_sigma_inv, sizeof(double) * (size_t)C * triD, hipMemcpyHostToDevice));
  fb_launch_iv_derive(e->stream, C, D, R, dM.as<double>(), dS.as<double>(), e->iv_sim.as<double>(), e->iv_u.as<double>());
  FBCHK(sync_stream(e));
  // the bucket workspace is laid out by C: a different system must not inherit stale `flags`
  if (e->iv_bws.p) HIPCHK(hipMemset(e->iv_bws.p, 0, e->iv_bws.cap));
  // ---- assign
  FbIvDev &iv = e->iv;
  iv.fg_gconsts = base; iv.fg_mic = base + n_gc; iv.fg_P = base + n_gc + n_mic;
  iv.fg64 = e->iv_fg64.as<double>();
  iv.fgL = p.fgL.empty() ? nullptr : e->iv_fgL.as<double>();
  iv.tri_r = e->iv_tri.as<unsigned char>(); iv.tri_c = iv.tri_r + triD;
  iv.sim = e->iv_sim.as<double>();
  iv.u = e->iv_u.as<double>();
  const double *b = e->iv_backend.as<double>();
  iv.mean_vec = b + p.o_mean; iv.ldaT = b + p.o_lda; iv.plda_mean = b + p.o_pm; iv.pldaT = b + p.o_pt;
  iv.plda_psi = b + p.o_psi; iv.train = b + p.o_tr;
  iv.text_scores = e->cfg.text_scores;
  iv.C = C; iv.Cpad = e->gmm.n_tiles * 32; iv.D = D; iv.R = R; iv.L = L; iv.S = S; iv.lda_cols = sy->lda_cols;
  iv.nsel = sy->num_gselect; iv.triD = triD; iv.triR = triR; iv.min_post = (float)sy->min_post;
  iv.prior_offset = sy->prior_offset;
  e->kind = 1;
  e->n_out = S;
  e->task = task;
  e->iv_kchunks = C / 8 > 128 ? 128 : (C / 8 < 1 ? 1 : C / 8);  // chunks of the active-component list
  return FB_OK;
}

// ----------------------------------------------------------------- x-vector
static int prepare_xvector(const fb_xvector_system *sy, FbXvPrepared *out) {
  std::string err;
  const int rc = fb_prepare_xvector(sy, out, &err);
  return rc == FB_OK ? FB_OK : fb_fail(rc, "%s", err.c_str());
}

extern "C" int fb_load_xvector(fb_engine *e, const fb_xvector_system *sy, int task) {
  if (!e || !sy) return fb_fail(FB_E_ARG, "null argument");
  if (task != FB_TASK_OSI && task != FB_TASK_CSI && task != FB_TASK_SV) return fb_fail(FB_E_ARG, "bad task");
  {
    std::string err;
    const int rc = fb_xvector_check(sy, &err);
    if (rc != FB_OK) return fb_fail(rc, "%s", err.c_str());
  }
  if (!e->have_fe || e->fe.dim != sy->D)
    return fb_fail(FB_E_ARG, "x-vector feature dim D=%d != front-end feature dim %d", sy->D, e->have_fe ? e->fe.dim : -1);
  if (task == FB_TASK_SV && sy->S != 1) return fb_fail(FB_E_ARG, "SV takes exactly one enrolled speaker");
  if (e->feco_iters > 0)
    return fb_fail(FB_E_STATE, "fb_load_xvector: feature compression is on (k-means discards the frame order a TDNN reads: switch it off)");
  // everything on the host first: a refused call leaves the engine and the device as they were
  FbXvPrepared p;
  FBCHK(prepare_xvector(sy, &p));
  const int D = sy->D, R = sy->R, L = sy->L, S = sy->S;
  // the placeholder in `gmm`: one component, zero mean, unit variance (never scored)
  const std::vector<float> ph_gc(1, 0.0f), ph_miv(D, 0.0f), ph_iv(D, 1.0f);
  FbGmmPrepared pg;
  FBCHK(prepare_gmm(e, 1, 1, D, ph_gc.data(), ph_miv.data(), ph_iv.data(), &pg));
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  // ---- ensure
  size_t n_par = 0;
  for (int l = 0; l < p.n_layers; ++l) {
    FBCHK(e->xv_w[l].ensure(sizeof(uint16_t) * (p.layer[l].w.size() + p.layer[l].wt.size())));   // the image, then the transposed one
    n_par += 3 * (size_t)p.layer[l].dout;
  }
  FBCHK(e->xv_par.ensure(sizeof(float) * n_par));
  FBCHK(e->xv_seg.ensure(sizeof(double) * (p.segT.size() + p.seg_bias.size())));
  FBCHK(e->iv_backend.ensure(sizeof(double) * p.be.backend.size()));
  FBCHK(commit_gmm(e, pg, ph_gc.data(), ph_miv.data(), ph_iv.data()));
  FBCHK(e->zmean.ensure(sizeof(double) * S));
  FBCHK(e->zstd.ensure(sizeof(double) * S));
  // ---- upload and assign
  FbXvDev &xv = e->xv;
  xv = FbXvDev{};
  xv.D = D; xv.n_layers = p.n_layers; xv.P = p.P; xv.R = R; xv.max_width = p.max_width;
  float *par = e->xv_par.as<float>();
  for (int l = 0; l < p.n_layers; ++l) {
    const FbXvLayerPrepared &q = p.layer[l];
    FbXvLayerDev &d = xv.layer[l];
    HIPCHK(hipMemcpy(e->xv_w[l].p, q.w.data(), sizeof(uint16_t) * q.w.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(par, q.bias.data(), sizeof(float) * q.dout, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(par + q.dout, q.scale.data(), sizeof(float) * q.dout, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(par + 2 * q.dout, q.offset.data(), sizeof(float) * q.dout, hipMemcpyHostToDevice));
    d.din = q.din; d.dout = q.dout; d.n_ctx = q.n_ctx;
    for (int j = 0; j < FB_XV_MAX_CTX; ++j) d.ctx[j] = q.ctx[j];
    d.K = q.K; d.n_steps = q.n_steps; d.kw = q.kw;
    d.w = e->xv_w[l].as<unsigned short>();
    HIPCHK(hipMemcpy(e->xv_w[l].as<unsigned short>() + q.w.size(), q.wt.data(), sizeof(uint16_t) * q.wt.size(), hipMemcpyHostToDevice));
    d.nt_steps = q.nt_steps; d.kwt = q.kwt;
    d.wt = e->xv_w[l].as<unsigned short>() + q.w.size();
    d.bias = par; d.scale = par + q.dout; d.offset = par + 2 * q.dout;
    par += 3 * (size_t)q.dout;
  }
  double *seg = e->xv_seg.as<double>();
  HIPCHK(hipMemcpy(seg, p.segT.data(), sizeof(double) * p.segT.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(seg + p.segT.size(), p.seg_bias.data(), sizeof(double) * p.seg_bias.size(), hipMemcpyHostToDevice));
  xv.segT = seg;
  xv.seg_bias = seg + p.segT.size();
  HIPCHK(hipMemcpy(e->iv_backend.p, p.be.backend.data(), sizeof(double) * p.be.backend.size(), hipMemcpyHostToDevice));
  e->h_zmean.assign(sy->z_mean, sy->z_mean + S);
  e->h_zstd.assign(sy->z_std, sy->z_std + S);
  HIPCHK(hipMemcpy(e->zmean.p, e->h_zmean.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->zstd.p, e->h_zstd.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  // the back-end fields of `iv`, and nothing else of it
  FbIvDev &iv = e->iv;
  iv = FbIvDev{};
  const double *b = e->iv_backend.as<double>();
  iv.mean_vec = b + p.be.o_mean; iv.ldaT = b + p.be.o_lda; iv.plda_mean = b + p.be.o_pm; iv.pldaT = b + p.be.o_pt;
  iv.plda_psi = b + p.be.o_psi; iv.train = b + p.be.o_tr;
  iv.text_scores = e->cfg.text_scores;
  iv.D = D; iv.R = R; iv.L = L; iv.S = S; iv.lda_cols = sy->lda_cols;
  e->kind = 2;
  e->n_out = S;
  e->task = task;
  e->xv_mask_B = 0;
  return FB_OK;
}

// ------------------------------------------------- the loaders' host preparation without an engine (fakebob_hip_test.h)
// size-then-fill: *size = the named buffer's bytes; with out != NULL it is copied there (cap bytes must hold it)
static int give_bytes(const char *name, const void *src, size_t n, void *out, int64_t cap, int64_t *size) {
  if (size) *size = (int64_t)n;
  if (!out) return FB_OK;
  if (cap < (int64_t)n) return fb_fail(FB_E_ARG, "out holds %lld bytes, buffer '%s' needs %lld", (long long)cap, name, (long long)n);
  if (n) memcpy(out, src, n);
  return FB_OK;
}
template <typename T> static int give_vector(const char *name, const std::vector<T> &v, void *out, int64_t cap, int64_t *size) {
  return give_bytes(name, v.data(), sizeof(T) * v.size(), out, cap, size);
}

extern "C" int fb_debug_prepare_gmm(int M, int C, int D, const float *gconsts, const float *means_invvars, const float *inv_vars,
                                    fb_gmm_plan *plan, int *perm, const char *buffer, int pass, void *out, int64_t cap,
                                    int64_t *size) {
  FbGmmPrepared p;
  FBCHK(prepare_gmm(nullptr, M, C, D, gconsts, means_invvars, inv_vars, &p));
  if (plan) {
    *plan = fb_gmm_plan{p.mode, p.NK, p.NKF, p.kx, p.kx2, p.kacc, p.n_tiles, p.n_items, p.n_groups, p.delta_p, p.delta_t3,
                        p.delta_t6, p.delta_t2, p.n_pass, {p.pass_lo[0], p.pass_lo[1], p.pass_lo[2], p.pass_lo[3]}, p.delta_rms};
  }
  if (perm)
    for (int c = 0; c < C; ++c) perm[c] = p.delta_p ? p.perm[c] : c;
  if (!buffer) return FB_OK;
  if (strcmp(buffer, "fx") == 0) return give_vector(buffer, p.fx, out, cap, size);
  if (strcmp(buffer, "bx") == 0) return give_vector(buffer, p.bx, out, cap, size);
  if (strcmp(buffer, "anchor") == 0) return give_vector(buffer, p.anchor, out, cap, size);
  if (strcmp(buffer, "item_model") == 0) return give_vector(buffer, p.item_model, out, cap, size);
  if (strcmp(buffer, "fd") == 0) {
    if (pass < 0 || pass >= FB_FXW_MAX_PASS) return fb_fail(FB_E_ARG, "pass %d out of range (0 .. %d)", pass, FB_FXW_MAX_PASS - 1);
    return give_vector(buffer, p.fd[pass], out, cap, size);
  }
  return fb_fail(FB_E_ARG, "no GMM buffer '%s' (fx, bx, fd, anchor, item_model)", buffer);
}

extern "C" int fb_debug_prepare_ivector(const fb_ivector_system *sy, const char *buffer, void *out, int64_t cap, int64_t *size) {
  FBCHK(check_ivector_args(nullptr, sy, 0));
  if (!buffer) return fb_fail(FB_E_ARG, "null argument");
  FbIvPrepared p;
  FBCHK(prepare_ivector(sy, &p));
  if (strcmp(buffer, "dg_gc") == 0) return give_vector(buffer, p.dg_gc, out, cap, size);
  if (strcmp(buffer, "dg_miv") == 0) return give_vector(buffer, p.dg_miv, out, cap, size);
  if (strcmp(buffer, "dg_iv") == 0) return give_vector(buffer, p.dg_iv, out, cap, size);
  if (strcmp(buffer, "fg_gc") == 0) return give_vector(buffer, p.fg_gc, out, cap, size);
  if (strcmp(buffer, "tri") == 0) return give_vector(buffer, p.tri, out, cap, size);
  if (strcmp(buffer, "fg64") == 0) return give_vector(buffer, p.fg64, out, cap, size);
  if (strcmp(buffer, "fgL") == 0) return give_vector(buffer, p.fgL, out, cap, size);
  if (strcmp(buffer, "backend") == 0) return give_vector(buffer, p.backend, out, cap, size);
  if (strcmp(buffer, "backend_offsets") == 0) {
    const std::vector<int64_t> o = {(int64_t)p.o_mean, (int64_t)p.o_lda, (int64_t)p.o_pm, (int64_t)p.o_pt, (int64_t)p.o_psi, (int64_t)p.o_tr};
    return give_vector(buffer, o, out, cap, size);
  }
  return fb_fail(FB_E_ARG, "no i-vector buffer '%s' (dg_gc, dg_miv, dg_iv, fg_gc, tri, fg64, fgL, backend, backend_offsets)", buffer);
}

extern "C" int fb_debug_prepare_xvector(const fb_xvector_system *sy, const char *buffer, void *out, int64_t cap, int64_t *size) {
  if (!sy || !buffer) return fb_fail(FB_E_ARG, "null argument");
  FbXvPrepared p;
  FBCHK(prepare_xvector(sy, &p));
  if (buffer[0] == 'w' && buffer[1] >= '0' && buffer[1] < '0' + p.n_layers && buffer[2] == 0)
    return give_vector(buffer, p.layer[buffer[1] - '0'].w, out, cap, size);
  if (strcmp(buffer, "kw") == 0) {
    std::vector<int32_t> kw;
    for (int l = 0; l < p.n_layers; ++l) kw.push_back(p.layer[l].kw);
    return give_vector(buffer, kw, out, cap, size);
  }
  if (buffer[0] == 'w' && buffer[1] == 't' && buffer[2] >= '0' && buffer[2] < '0' + p.n_layers && buffer[3] == 0)
    return give_vector(buffer, p.layer[buffer[2] - '0'].wt, out, cap, size);
  if (strcmp(buffer, "kwt") == 0) {
    std::vector<int32_t> kwt;
    for (int l = 0; l < p.n_layers; ++l) kwt.push_back(p.layer[l].kwt);
    return give_vector(buffer, kwt, out, cap, size);
  }
  if (strcmp(buffer, "segT") == 0) return give_vector(buffer, p.segT, out, cap, size);
  if (strcmp(buffer, "backend") == 0) return give_vector(buffer, p.be.backend, out, cap, size);
  if (strcmp(buffer, "backend_offsets") == 0) {
    const std::vector<int64_t> o = {(int64_t)p.be.o_mean, (int64_t)p.be.o_lda, (int64_t)p.be.o_pm, (int64_t)p.be.o_pt,
                                    (int64_t)p.be.o_psi, (int64_t)p.be.o_tr};
    return give_vector(buffer, o, out, cap, size);
  }
  return fb_fail(FB_E_ARG, "no x-vector buffer '%s' (w0 .. w%d, kw, wt0 .. wt%d, kwt, segT, backend, backend_offsets)", buffer, p.n_layers - 1,
                 p.n_layers - 1);
}

// Test hook: the x-vector chain on rows handed in (fakebob_hip_test.h)
extern "C" int fb_debug_xv_embed(fb_engine *e, const float *feats, const int *row_off, int B, int layer, void *out) {
  if (!e || !feats || !row_off || !out || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 2) return fb_fail(FB_E_STATE, "load an x-vector system first");
  const FbXvDev &xv = e->xv;
  if (layer < 0 || layer > xv.n_layers + 1) return fb_fail(FB_E_ARG, "layer %d outside 0 .. %d", layer, xv.n_layers + 1);
  if (row_off[0] != 0) return fb_fail(FB_E_ARG, "row_off[0] must be 0");
  for (int b = 0; b < B; ++b)
    if (row_off[b + 1] < row_off[b]) return fb_fail(FB_E_ARG, "row_off must not descend");
  const int rows = row_off[B];
  if (rows <= 0) return fb_fail(FB_E_ARG, "no rows");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  e->bench_it = e->nes_rec.iter = -1;
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)rows * xv.D));
  FBCHK(e->row_off.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(h2d(e, e->feats.p, feats, sizeof(float) * (size_t)rows * xv.D));
  FBCHK(h2d(e, e->row_off.p, row_off, sizeof(int) * (size_t)(B + 1)));
  const float *last = nullptr;
  FBCHK(run_xvector(e, B, rows, layer, &last));
  HIPCHK(hipGetLastError());
  if (layer < xv.n_layers) FBCHK(d2h(e, out, last, sizeof(float) * (size_t)rows * xv.layer[layer].dout));
  else if (layer == xv.n_layers) FBCHK(d2h(e, out, e->xv_stats.p, sizeof(double) * (size_t)B * 2 * xv.P));
  else FBCHK(d2h(e, out, e->iv_ivec.p, sizeof(double) * (size_t)B * xv.R));
  return sync_stream(e);
}

// Benchmark hook (tools/xvector_rate.py): every launch of the x-vector chain on rows handed in, `reps` times between device
// events after one launch to warm up
extern "C" int fb_bench_xvector(fb_engine *e, const float *feats, const int *row_off, int B, int reps, double *ms_rowmax,
                                double *ms_affine, double *ms_tail) {
  if (!e || !feats || !row_off || !ms_rowmax || !ms_affine || !ms_tail || B <= 0 || reps <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 2) return fb_fail(FB_E_STATE, "load an x-vector system first");
  const FbXvDev &xv = e->xv;
  const int rows = row_off[B];
  if (row_off[0] != 0 || rows <= 0) return fb_fail(FB_E_ARG, "bad row_off");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  e->bench_it = e->nes_rec.iter = -1;
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)rows * xv.D));
  FBCHK(e->row_off.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(e->raw.ensure(sizeof(double) * (size_t)B * e->n_out));
  FBCHK(h2d(e, e->feats.p, feats, sizeof(float) * (size_t)rows * xv.D));
  FBCHK(h2d(e, e->row_off.p, row_off, sizeof(int) * (size_t)(B + 1)));
  FBCHK(run_xvector(e, B, rows, xv.n_layers + 1, nullptr));   // every buffer sized, every stage's input in place
  FBCHK(sync_stream(e));
  hipStream_t s = e->stream;
  hipEvent_t ev0, ev1;
  HIPCHK(hipEventCreate(&ev0));
  HIPCHK(hipEventCreate(&ev1));
  auto timed = [&](auto &&launch, double *ms) -> int {
    launch();
    HIPCHK(hipEventRecord(ev0, s));
    for (int i = 0; i < reps; ++i) launch();
    HIPCHK(hipEventRecord(ev1, s));
    HIPCHK(hipEventSynchronize(ev1));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, ev0, ev1));
    *ms = (double)t / reps;
    return FB_OK;
  };
  const int *n_rows = e->row_off.as<int>() + B;
  int rc = FB_OK;
  const float *in = e->feats.as<float>();
  for (int l = 0; l < xv.n_layers && rc == FB_OK; ++l) {
    float *out = e->xv_act[l & 1].as<float>();
    rc = timed([&] { fb_launch_xv_rowmax(s, in, xv.layer[l].din, n_rows, rows, e->xv_amax.as<float>()); }, ms_rowmax + l);
    if (rc == FB_OK)
      rc = timed([&] { fb_launch_xv_affine(s, xv.layer[l], in, e->xv_amax.as<float>(), e->xv_rowinfo.as<int2>(), n_rows, rows, out); },
                 ms_affine + l);
    in = out;
  }
  if (rc == FB_OK) rc = timed([&] { fb_launch_xv_pool(s, in, xv.P, e->row_off.as<int>(), B, e->xv_stats.as<double>()); }, ms_tail + 0);
  if (rc == FB_OK) rc = timed([&] { fb_launch_xv_segment(s, xv, e->xv_stats.as<double>(), B, e->iv_ivec.as<double>()); }, ms_tail + 1);
  if (rc == FB_OK) rc = timed([&] { fb_launch_iv_backend(s, e->iv, e->iv_ivec.as<double>(), B, e->raw.as<double>()); }, ms_tail + 2);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  return rc;
}

extern "C" int fb_debug_prepare_frontend(const fb_frontend_cfg *c, const char *buffer, void *out, int64_t cap, int64_t *size) {
  if (!c || !buffer) return fb_fail(FB_E_ARG, "null argument");
  FrontendPrepared p;
  FBCHK(prepare_frontend(c, &p));
  const FbFrontendBlob &b = p.blob;
  if (strcmp(buffer, "blob") == 0) return give_vector(buffer, b.bytes, out, cap, size);
  if (strcmp(buffer, "f32") == 0) return give_vector(buffer, p.t32, out, cap, size);
  if (strcmp(buffer, "offsets") == 0) {
    const std::vector<int64_t> o = {(int64_t)b.o_window, (int64_t)b.o_twh, (int64_t)b.o_twf, (int64_t)b.o_mf, (int64_t)b.o_ml,
                                    (int64_t)b.o_mo, (int64_t)b.o_mw, (int64_t)b.o_dct, (int64_t)b.o_lift, (int64_t)b.o_ds};
    return give_vector(buffer, o, out, cap, size);
  }
  return fb_fail(FB_E_ARG, "no front-end buffer '%s' (blob, f32, offsets)", buffer);
}

extern "C" int fb_debug_iv_active(fb_engine *e, int *n_active) {
  if (!e || !n_active) return fb_fail(FB_E_ARG, "bad argument");
  if (e->kind != 1 || e->last_B <= 0) return fb_fail(FB_E_STATE, "score a batch with an i-vector system first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  HIPCHK(hipMemcpy(n_active, e->iv_active.as<int>() + e->iv.C, sizeof(int), hipMemcpyDeviceToHost));
  return FB_OK;
}

// the kernels the front end of the last batch ran (launch_mfcc / run_post_mfcc record them as they enqueue)
extern "C" int fb_debug_frontend_route(fb_engine *e, int *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_route) return fb_fail(FB_E_STATE, "no batch has run the front end yet");
  for (int i = 0; i < 5; ++i) info[i] = e->route[i];
  return FB_OK;
}

// the launch geometry of the last batch (choose_launch_shape starts the record, the launchers fill it in)
extern "C" int fb_debug_launch_shape(fb_engine *e, int *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_shape) return fb_fail(FB_E_STATE, "no batch has launched yet");
  const FbGmmShape &g = e->shape_gmm;
  const FbMfccShape &m = e->shape_mfcc;
  const int v[13] = {g.kernel, g.n_chunks, g.sub, g.grid_chunks, g.xcd_map, g.passes, g.strips, g.tiles_min, g.tiles_max,
                     m.cus, m.rounds, m.blocks, e->shape_upd_threads};
  for (int i = 0; i < 13; ++i) info[i] = v[i];
  return FB_OK;
}

// gmm-gselect of the last i-vector batch: sel[rows][nsel] (rows = the batch's voiced frames), and what the threshold path
// did: info[0] = 2 when fb_launch_gsel_wide ran (k_gsel_w), 1 when fb_launch_gsel did (k_gmm_fx2_sel), 0: the dump +
// k_iv_select path; info[1] = the flag (path 1: a list overflowed and the rescue launches redid the batch); info[2] = most
// entries in one (row, chunk) list, info[3] = entries in total (path 1: survivors; path 2: 16-value records of the groups that
// reach the threshold), info[4] = rows
extern "C" int fb_debug_iv_gselect(fb_engine *e, int *sel, int64_t sel_cap, int64_t *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "bad argument");
  if (e->kind != 1 || e->last_B <= 0) return fb_fail(FB_E_STATE, "score a batch with an i-vector system first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  int rows = 0;
  HIPCHK(hipMemcpy(&rows, e->row_off.as<int>() + e->last_B, sizeof(int), hipMemcpyDeviceToHost));
  const int nsel = e->iv.nsel;
  if (sel) {
    if (sel_cap < (int64_t)rows * nsel) return fb_fail(FB_E_ARG, "sel holds %lld ints, the batch needs %lld", (long long)sel_cap, (long long)rows * nsel);
    HIPCHK(hipMemcpy(sel, e->iv_sel.p, sizeof(int) * (size_t)rows * nsel, hipMemcpyDeviceToHost));
  }
  const int n_chunks = e->gs_last_chunks;
  info[0] = e->gs_last_path;   // 0: dump + k_iv_select, 1: k_gmm_fx2_sel (lists of survivors), 2: k_gsel_w (records of groups)
  info[1] = info[2] = info[3] = 0;
  info[4] = rows;
  info[5] = n_chunks;
  if (info[0]) {
    int flag = 0;
    HIPCHK(hipMemcpy(&flag, e->gs_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    info[1] = flag;
    std::vector<int> cnt((size_t)rows * n_chunks);
    HIPCHK(hipMemcpy(cnt.data(), e->gs_cnt.p, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    for (int c : cnt) { info[2] = c > info[2] ? c : info[2]; info[3] += c; }
  }
  return FB_OK;
}

// i-vectors of the last scored batch (enrolment: build_spk_models.py:104-150 keeps the enrolment utterance's
// i-vector as the speaker identity)
extern "C" int fb_last_ivectors(fb_engine *e, int B, double *ivecs) {
  if (!e || !ivecs || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (e->kind == 0 || e->last_B < B) return fb_fail(FB_E_STATE, "score a batch with an i-vector or x-vector system first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  HIPCHK(hipMemcpy(ivecs, e->iv_ivec.p, sizeof(double) * (size_t)B * e->iv.R, hipMemcpyDeviceToHost));
  return FB_OK;
}

// --------------------------------------------------------------------- NES
// the checks of fb_nes_params every NES call makes, for a system of S speakers
// ... the part every attack shares, whatever its search (fb_attack_pso reads none of the NES-only fields)
static int check_goal_params(const fb_nes_params *p, int S) {
  if (p->task != FB_TASK_SV && p->attack_type == FB_TARGETED && (p->target < 0 || p->target >= S))
    return fb_fail(FB_E_ARG, "target %d out of range", p->target);
  if (p->task == FB_TASK_CSI && p->attack_type == FB_UNTARGETED && (p->true_label < 0 || p->true_label >= S))
    return fb_fail(FB_E_ARG, "true label %d out of range", p->true_label);
  if (p->bits_per_sample != 0 && (p->bits_per_sample < 2 || p->bits_per_sample > 16))
    return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", p->bits_per_sample);
  return FB_OK;
}
static int check_nes_params(const fb_nes_params *p, int S) {
  if (p->samples_per_draw < 0 || p->samples_per_draw > 4094) return fb_fail(FB_E_ARG, "bad samples_per_draw");
  if (!(p->sigma > 0.0) && p->samples_per_draw >= 2) return fb_fail(FB_E_ARG, "sigma must be > 0");
  return check_goal_params(p, S);
}
static int check_params(fb_engine *e, const fb_nes_params *p, int64_t N) {
  if (!e || !p) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  if (p->task != e->task) return fb_fail(FB_E_ARG, "params.task %d != engine system task %d", p->task, e->task);
  const int S = fb_num_speakers(e);
  if (S > 62) return fb_fail(FB_E_ARG, "more than 62 speakers unsupported in the NES result block");
  FBCHK(check_nes_params(p, S));
  if (num_frames(e->cfg, N) <= 0) return fb_fail(FB_E_ARG, "audio shorter than one frame");
  return FB_OK;
}
static inline int nes_bits(const fb_nes_params *p) { return p->bits_per_sample ? p->bits_per_sample : 16; }
// replicas of every NES row the front end scores in the native NES calls: K * eot (fb_set_companions, fb_set_eot)
static inline int nes_replicas(const fb_engine *e) { return (e->comp_K1 + 1) * e->eot; }
// fb_set_play_offset: the loop the offset rotates has the utterance's length, so every offset must lie inside it
static int check_play_length(const fb_engine *e, int64_t N) {
  if (e->play_S > 0 && N <= e->play_S)
    return fb_fail(FB_E_ARG, "the audio has %lld samples, the play offset (fb_set_play_offset) goes up to %lld: it must stay below the length",
                   (long long)N, (long long)e->play_S);
  return FB_OK;
}
// the calls that do not model a play offset refuse it by name
static int refuse_play(const fb_engine *e, const char *who) {
  if (e && e->play_S > 0)
    return fb_fail(FB_E_STATE, "%s does not run under a play offset (fb_set_play_offset(%lld)): not in this version, set 0", who,
                   (long long)e->play_S);
  return FB_OK;
}
// The checks and buffers of a native NES call that scale with the replicas.  B: the rows of the NES batch.
// composes: the call composes its rows under the play offset when one is set (every native NES and white-box entry; false: a
// hook that ignores the setting) -- the offsets must then stay below N, which k_play_compose's single wrap relies on.
static int prepare_nes_batch(fb_engine *e, int64_t N, int B);
static int prepare_nes_replicas(fb_engine *e, int64_t N, int B, bool composes = true) {
  const int r = nes_replicas(e);
  if (composes) FBCHK(check_play_length(e, N));
  if (e->comp_K1 > 0 && N != e->comp_N)
    return fb_fail(FB_E_ARG, "the audio has %lld samples, the companions (fb_set_companions) %lld", (long long)N, (long long)e->comp_N);
  if (r > 32) return fb_fail(FB_E_ARG, "utterances * eot = %d replicas per NES row: at most 32", r);
  if ((int64_t)B * r > 65535)
    return fb_fail(FB_E_LIMIT, "(samples_per_draw + 1) * utterances * eot = %lld rows: a scoring batch takes up to 65535", (long long)B * r);
  FBCHK(prepare_nes_batch(e, N, B * r));
  if (r > 1 || e->play_S > 0) {
    FBCHK(e->eot_sc.ensure(sizeof(double) * (size_t)B * r * (size_t)std::max(fb_num_speakers(e), 1)));
    FBCHK(e->eot_l.ensure(sizeof(double) * (size_t)B * r));
  }
  if (e->comp_K1 > 0 || e->play_S > 0) FBCHK(e->comp_a0.ensure(sizeof(int16_t) * (size_t)N));
  return FB_OK;
}
// a_0 of the composition: the int16 cast of the call's original audio (x: device float64 [N]), once per call
static void cast_a0(fb_engine *e, const fb_nes_params *p, const double *x, int64_t N) {
  if (e->comp_K1 > 0 || e->play_S > 0) fb_launch_quantize(e->stream, x, N, nes_bits(p), e->comp_a0.as<int16_t>());
}

// (re)builds the equal-length batch layout of B utterances of N samples
static int prepare_nes_batch(fb_engine *e, int64_t N, int B) {
  if (e->cached_B == B && e->cached_N == N) return FB_OK;
  FBCHK(sync_stream(e));
  std::vector<int64_t> off(B + 1);
  for (int b = 0; b <= B; ++b) off[b] = (int64_t)b * N;
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * B));
  FBCHK(prepare_batch(e, off.data(), B));
  FBCHK(sync_stream(e));
  e->cached_B = B;
  e->cached_N = N;
  return FB_OK;
}

static int ensure_nes_buffers(fb_engine *e, int64_t N, int B, int S = -1) {
  if (S < 0) S = fb_num_speakers(e);
  FBCHK(e->audio.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->adver.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->grad_m.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->grad.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->scores.ensure(sizeof(double) * (size_t)B * (S > 0 ? S : 1)));
  FBCHK(e->loss.ensure(sizeof(double) * (size_t)B));
  FBCHK(e->dist_part.ensure(sizeof(double) * (size_t)((N + 255) / 256 + 1)));  // k_perturb: one per 1024 samples, k_update_perturb: per 256
  FBCHK(e->nes_out.ensure(sizeof(FbNesDev)));
  FBCHK(e->zbuf.ensure(sizeof(float) * (size_t)N * (size_t)((B - 1) / 2 > 0 ? (B - 1) / 2 : 1)));
  return FB_OK;
}

// One get_grad on the device-resident adver: perturb -> score -> loss.  Async.
// FB_FUSE_PARTS=<bit mask> chooses the fusions one by one whatever the chain setting says (experiments: bit 0 the
// front-end's k_vad_delta_cmvn(_p), bit 1 k_gmm_finalize_loss, bit 2 the update kernels); read per call
static bool fb_fuse_part(const fb_engine *e, int part) {
  if (const char *ev = getenv("FB_FUSE_PARTS")) return ((atoi(ev) >> part) & 1) != 0;
  // fb_set_fused_chain(e, 0) -- three or more attacks per GPU -- keeps TWO fusions: k_update_perturb (momentum step + the
  // next batch) instead of k_grad_update + k_perturb  Measured with three attacks in flight, every combination twice
  // (tools/profile/r05_parts.sh): none 11.69 / 11.74 k it/s, this one 11.87 / 11.87, the front-end's 11.52 / 11.50, all
  // three 11.31 / 11.26.  FB_NO_FUSE=1 still means every launch on its own.
  // ... and the front-end's (k_vad_delta_cmvn_p at its own 35 KB of LDS, not padded to a workgroup per CU -- so that it
  // runs BESIDE the other attacks' k_gmm_fx2w workgroups): 11.66 -> 12.08 k it/s; with the finalisation fused as well
  // 11.34 (tools/profile/r05_stack.sh; four attacks in flight: 10.7 k, two: 10.5 k).
  // (Not with the CompressedMatrix round trip on: its phase lives in the one-workgroup-per-utterance kernel, which a
  //  shared GPU does not take well -- the reference-pipeline secondary fell from 10.6 to 8.7 k it/s with it.)
  if ((part == 2 || (part == 0 && !e->cfg.compress_feats)) && e->fuse_opt == 0 && getenv("FB_NO_FUSE") == nullptr) return true;
  // (The finalisation's once more, in an experiment that is not in this tree: k_gmm_finalize_loss<true> under an occupancy
  //  bound of six waves per SIMD, which the compiler then reported at 75 registers per wave, so that it fits beside a resident
  //  k_gmm_fx2w workgroup, the update a launch of its own: 12.85 - 12.93 k it/s against 13.07 - 13.13 k -- the one launch
  //  took 23.3 us where k_gmm_finalize + k_loss take 9.7 + 9.1.  DESIGN.md section 6, the change itself as it was measured in
  //  docs/experiments/fused_finalize_bound.diff (kept for the record like the others there; nothing builds it).
  //  FB_FUSE_PARTS=7 FB_FUSE_UPD=0 runs
  //  the same five launches with the kernel as it is here, unbounded at 119 registers.)
  return fb_fuse_on(e);
}
static bool fb_fuse_on(const fb_engine *e) {
  if (e->fuse_opt >= 0) return e->fuse_opt != 0;  // fb_set_fused_chain
  return getenv("FB_NO_FUSE") == nullptr;  // FB_NO_FUSE=1: the 8-launch chain (A/B, debugging; read per call)
}

// Who scores the NES batch: this library's own system, a host callback (fb_score_cb) or a model on the same GPU
// (fb_score_dev_cb writing into fb_dev_model's buffers)
enum FbScorerKind { FB_SCORER_NATIVE, FB_SCORER_HOST, FB_SCORER_DEV };
struct FbScorer {
  FbScorerKind kind;
  int S = 0;                            // speakers scored (the native systems': filled in by nes_setup)
  fb_score_cb cb = nullptr;             // FB_SCORER_HOST
  const fb_dev_model *m = nullptr;      // FB_SCORER_DEV
  fb_score_dev_cb dcb = nullptr;
  void *ctx = nullptr;                  // the callback's
};

// How an attack's NES loop runs, fixed at the start of the public call: the A/B knobs are read from the environment
// there and nowhere in the loop (attack threads run it while the process may change its environment, and getenv
// racing setenv is undefined).  The default -- the host-callback path -- looks after every iteration and fuses nothing.
struct FbLoopKnobs {
  int look = 1;             // iterations queued per look at the control block
  bool fuse_fin = false;    // the GMM finalisation and the loss in one launch (fb_fuse_part(e, 1))
  bool fuse_upd = false;    // the momentum step and the next batch in one launch (fb_fuse_part(e, 2); the device path)
  bool upd_in_fin = false;  // ... riding in the finalising launch (FB_FUSE_UPD=0: two launches)
  bool fin_ticket = false;  // FB_FIN_TICKET=1: the finalising launch's roles by an arrival ticket
  bool fin_xch = false;     // its exchange slots (FB_FIN_COUNTER=1: the arrival counter instead)
  int upd_threads = 512;    // threads of a k_update_perturb(_x) workgroup (choose_update_threads)
  bool look_ahead = false;  // batch n + 1 is queued before the host waits for batch n's control block (FB_LOOK_AHEAD=0 | 1)
};
// FB_ATTACK_BATCH: iterations queued per host round trip (1 .. 16, default 4), read once at the start of an attack.  Beyond ~4
// the host is off the critical path anyway, and every iteration queued behind the stopping one is (cheap, but not free) wasted work.
static int attack_batch() {
  const char *ev = getenv("FB_ATTACK_BATCH");
  const int b = ev ? atoi(ev) : 4;
  return b < 1 ? 1 : (b > 16 ? 16 : b);
}
static FbLoopKnobs loop_knobs(const fb_engine *e, const FbScorer &sc) {
  FbLoopKnobs k;
  k.upd_threads = choose_update_threads(e);
  if (sc.kind == FB_SCORER_DEV) {
    k.look = sc.m->look_every > 0 ? sc.m->look_every : 4;
    k.fuse_upd = true;
  } else if (sc.kind == FB_SCORER_NATIVE) {
    k.look = attack_batch();
    k.fuse_fin = fb_fuse_part(e, 1) && nes_replicas(e) == 1 && e->play_S == 0;  // (fb_set_eot, fb_set_companions, fb_set_play_offset: the finalisation, then k_loss_eot)
    k.fuse_upd = fb_fuse_part(e, 2);
    const char *fu = getenv("FB_FUSE_UPD");
    k.upd_in_fin = !(fu && fu[0] == '0');
    // No drain between looks once three engines share the device; FB_LOOK_AHEAD=0: the draining loop,
    // = 1: for a lone attack as well.  A stopping attack queues one more batch of launches that return on the stop flag.
    const char *la = getenv("FB_LOOK_AHEAD");
    k.look_ahead = la ? la[0] == '1' : fb_shared_gpu(e);
    const char *tk = getenv("FB_FIN_TICKET");
    k.fin_ticket = tk && tk[0] == '1';
    k.fin_xch = getenv("FB_FIN_COUNTER") == nullptr;
  }
  return k;
}
// the momentum sign step of iteration i and the batch of i + 1 in one launch: Philox noise and a small enough batch
static bool fuses_update(const FbLoopKnobs &kn, const double *noise, int half) {
  return kn.fuse_upd && !noise && half > 0 && half <= FB_FUSE_MAX_HALF;
}

static int enqueue_get_grad(fb_engine *e, const fb_nes_params *p, int64_t N, uint32_t iter,
                            const double *noise_dev, bool with_dist, const FbLoopKnobs &kn = FbLoopKnobs(),
                            FbCtlDev *ctl = nullptr, double *trace_dev = nullptr, int trace_row = 0,
                            const FbUpdArgs *upd = nullptr, bool *upd_done = nullptr) {
  const int half = p->samples_per_draw / 2, B = 2 * half + 1;
  const int r = nes_replicas(e), BR = B * r;  // fb_set_eot, fb_set_companions: the front end scores r replicas of every row
  const bool rep = r > 1 || e->play_S > 0;    // ... and with a play offset the call takes that route at r = 1 too
  int ndp = 0;
  const int *stop = ctl ? &ctl->stop : nullptr;
  if (ctl && e->pre_iter == (long long)iter && !noise_dev) {
    ndp = e->pre_ndp;  // the fused update of the previous iteration already wrote this batch
  } else {
    fb_launch_perturb(e->stream, e->adver.as<double>(), with_dist ? e->audio.as<double>() : nullptr, N, half,
                      p->sigma, p->seed, iter, p->stream, noise_dev, e->wav.as<int16_t>(),
                      e->dist_part.as<double>(), &ndp, noise_dev ? nullptr : e->zbuf.as<float>(), stop, nes_bits(p));
    record_nes_batch(e, iter, N, half, !rep, !noise_dev);  // (replicated, or rotated by a play offset: the rows scored are pinned elsewhere)
  }
  e->pre_iter = -1;
  // GMM systems inside the device-controlled loop: finalisation and loss share one launch
  const bool fuse_fin = ctl && e->kind == 0 && kn.fuse_fin;  // (never with fb_set_eot r > 1: loop_knobs)
  // Kaldi's dither, the noise stages and feature compression inside an attack: keyed by the attack's own (seed, stream),
  // epoch = the NES iteration (in fb_estimate_threshold `iter` counts the call's front-end launches: one per pass of its loop)
  FbScoreCall call{FbRngPoint{p->seed, p->stream, iter, 0}};
  call.eot = e->eot;
  call.K = e->comp_K1 + 1;
  call.play = e->play_S;
  call.stop = stop;
  call.defer_finalize = fuse_fin;
  FbIvTail t = {};
  if (e->kind == 1 && !rep) {  // i-vector systems: the loss body rides in the tail of the solve kernel when the batch allows it
    t.task = p->task; t.attack_type = p->attack_type;
    t.z_mean = e->zmean.as<double>(); t.z_std = e->zstd.as<double>();
    t.threshold = p->threshold; t.adver_thresh = p->adver_thresh;
    t.target = p->target; t.true_label = p->true_label;
    t.dist_part = e->dist_part.as<double>(); t.n_dist_part = with_dist ? ndp : 0;
    t.scores = e->scores.as<double>(); t.loss_out = e->loss.as<double>();
    t.out = e->nes_out.as<FbNesDev>(); t.ctl = ctl; t.trace = trace_dev; t.it = trace_row;
    call.tail_loss = &t;
  }
  FBCHK(run_scoring(e, call, BR, e->h_frame_off[BR]));
  if (rep) {
    fb_launch_loss_eot(e->stream, e->raw.as<double>(), e->tv.as<int>(), B, r, e->n_out, p->task, e->kind, p->attack_type,
                       e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, p->adver_thresh, p->target, p->true_label,
                       e->dist_part.as<double>(), with_dist ? ndp : 0, e->eot_sc.as<double>(), e->eot_l.as<double>(),
                       e->scores.as<double>(), e->loss.as<double>(), e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row);
    e->nes_route[FB_NES_ROUTE_K_LOSS] += 1;
    return FB_OK;
  }
  if (call.tail_loss_done) {
    e->nes_route[FB_NES_ROUTE_IV_TAIL] += 1;
    return FB_OK;
  }
  if (fuse_fin) {
    if (!e->fin_counter.p) {
      FBCHK(e->fin_counter.ensure(2 * sizeof(int)));   // [0] the arrival counter, [1] the fused launch's role ticket
      HIPCHK(hipMemsetAsync(e->fin_counter.p, 0, 2 * sizeof(int), e->stream));
    }
    FbUpdArgs ux;
    if (upd) {
      // roles by blockIdx (the default again, round 6); FB_FIN_TICKET=1: by an arrival ticket (round 6's first answer to the
      // advisor's finding -- 494 returning atomics on one word in front of every workgroup's work: 6.8 us per iteration of
      // a lone attack, tools/profile/r06_fin.sh).  See the note at k_gmm_finalize_loss_update for why the launch cannot
      // deadlock either way (A/B between calls: FbLoopKnobs)
      ux = *upd;
      ux.role_ticket = kn.fin_ticket ? e->fin_counter.as<int>() + 1 : nullptr;
      upd = &ux;
    }
    if (upd && kn.fin_xch) {  // (FB_FIN_COUNTER=1: the arrival counter instead of the exchange slots, A/B)
      const size_t had = e->fin_xch.cap;
      FBCHK(e->fin_xch.ensure(sizeof(unsigned long long) * (size_t)B * e->gmm.M));
      if (e->fin_xch.cap != had || !e->fin_xch_clean) {
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->fin_xch.p), (int)FB_VAD_SENTINEL32, e->fin_xch.cap / 4, e->stream));
        e->fin_xch_clean = true;
      }
      ux.xch = e->fin_xch.as<unsigned long long>();
    }
    fb_launch_gmm_finalize_loss(e->stream, e->gmm, e->part_m.as<float>(), e->part_s.as<float>(), e->last_total_frames,
                                e->last_chunks, e->row_off.as<int>(), B, e->raw.as<double>(), e->fin_counter.as<int>(),
                                e->tv.as<int>(), p->task, p->attack_type, e->zmean.as<double>(), e->zstd.as<double>(),
                                p->threshold, p->adver_thresh, p->target, p->true_label, e->dist_part.as<double>(),
                                with_dist ? ndp : 0, e->scores.as<double>(), e->loss.as<double>(),
                                e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row, upd ? ++e->ctl_seq : 0, upd);
    if (upd && upd_done) *upd_done = true;
    e->nes_route[upd ? FB_NES_ROUTE_FIN_LOSS_UPDATE : FB_NES_ROUTE_FIN_LOSS] += 1;
    return FB_OK;
  }
  fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), B, e->n_out, p->task, e->kind, p->attack_type,
                 e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, p->adver_thresh, p->target,
                 p->true_label, e->dist_part.as<double>(), with_dist ? ndp : 0, e->scores.as<double>(),
                 e->loss.as<double>(), e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row);
  e->nes_route[FB_NES_ROUTE_K_LOSS] += 1;
  return FB_OK;
}

// the NES result block of the last iteration to the host (native: with the GMM timing of fb_bench_nes)
static int fetch_out(fb_engine *e, bool native) {
  HIPCHK(hipMemcpyAsync(e->h_out, e->nes_out.p, sizeof(FbNesDev), hipMemcpyDeviceToHost, e->stream));
  FBCHK(sync_stream(e));
  if (native && e->gmm_pending) FBCHK(time_collect(e));
  if (e->h_out->err != 0)  // (never set for a foreign model: see attack_loop)
    return fb_fail(FB_E_NO_VOICED, "NES sample %d has no voiced frames", e->h_out->err - 1);
  return FB_OK;
}

// device clock stamps of the attack that just ran -> seconds per iteration (e->iter_seconds)
static int collect_iter_seconds(fb_engine *e, int rows) {
  e->iter_seconds.assign((size_t)(rows > 0 ? rows : 0), 0.0);
  if (rows <= 0) return FB_OK;
  std::vector<unsigned long long> t((size_t)rows + 1);
  FBCHK(d2h(e, t.data(), e->ticks.p, sizeof(unsigned long long) * t.size()));
  FBCHK(sync_stream(e));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device) != hipSuccess || khz <= 0) khz = 100000;
  for (int i = 0; i < rows; ++i) e->iter_seconds[i] = (double)(t[i + 1] - t[i]) / (1.0e3 * khz);
  return FB_OK;
}

// ------------------------------------------------- foreign models (plugin API)
// The reference's FakeBob accepts ANY `model` with score / make_decisions (README.md:136; FAKEBOB.py:53,89,250).
// For a model that is not one of this library's systems the scores come from a host callback; everything else of
// the NES iteration stays on the device: Philox noise + perturbation (k_perturb_f64), loss + loop control (k_loss),
// gradient estimate + momentum sign step (k_grad_update).  One host round trip per iteration is inherent.
static int check_params_ext(fb_engine *e, const fb_nes_params *p, int64_t N, int S, bool have_cb) {
  if (!e || !p || !have_cb) return fb_fail(FB_E_ARG, "null argument");
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  if (p->task != FB_TASK_OSI && p->task != FB_TASK_CSI && p->task != FB_TASK_SV) return fb_fail(FB_E_ARG, "bad task");
  if (S <= 0 || S > 62) return fb_fail(FB_E_ARG, "number of speakers must be in [1, 62] (got %d)", S);
  if (p->task == FB_TASK_SV && S != 1) return fb_fail(FB_E_ARG, "SV scores one speaker (got S = %d)", S);
  return check_nes_params(p, S);
}

// fb_debug_foreign_path's record of the foreign-model call that starts now
static void foreign_begin(fb_engine *e, const FbScorer &sc, int launches_per_iter) {
  const bool dev = sc.kind == FB_SCORER_DEV;
  e->foreign = fb_foreign_path_info{};
  e->foreign.path = dev ? FB_FOREIGN_DEV : FB_FOREIGN_HOST;
  e->foreign.x_dtype = dev ? sc.m->x_dtype : FB_DT_F64;
  e->foreign.score_dtype = dev ? sc.m->score_dtype : FB_DT_F64;
  e->foreign.launches_per_iter = launches_per_iter;
}

// perturb -> float64 batch to the host -> callback -> scores to the device -> loss (+ loop control)
static int enqueue_get_grad_ext(fb_engine *e, const fb_nes_params *p, const FbScorer &sc, int64_t N, uint32_t iter,
                                const double *noise_dev, bool with_dist, FbCtlDev *ctl = nullptr,
                                double *trace_dev = nullptr, int trace_row = 0) {
  const int half = p->samples_per_draw / 2, B = 2 * half + 1, S = sc.S;
  int ndp = 0;
  fb_launch_perturb_f64(e->stream, e->adver.as<double>(), with_dist ? e->audio.as<double>() : nullptr, N, half,
                        p->sigma, p->seed, iter, p->stream, noise_dev, e->ext_x.as<double>(),
                        e->dist_part.as<double>(), &ndp, noise_dev ? nullptr : e->zbuf.as<float>());
  record_nes_batch(e, iter, N, half, false, !noise_dev);
  const size_t xb = sizeof(double) * (size_t)N * B;
  std::vector<double> sc_h((size_t)B * S);
  if (xb <= FB_PIN_MAX) {  // the callback reads the pinned staging area directly
    char *xh = nullptr;
    FBCHK(pin_reserve(e, xb, &xh));
    HIPCHK(hipMemcpyAsync(xh, e->ext_x.p, xb, hipMemcpyDeviceToHost, e->stream));
    FBCHK(sync_stream(e));
    const int rc = sc.cb(sc.ctx, reinterpret_cast<const double *>(xh), N, B, sc_h.data());
    if (rc != 0) return fb_fail(FB_E_CALLBACK, "score callback failed (rc %d)", rc);
  } else {
    std::vector<double> xh((size_t)N * B);
    FBCHK(sync_stream(e));
    HIPCHK(hipMemcpy(xh.data(), e->ext_x.p, xb, hipMemcpyDeviceToHost));
    const int rc = sc.cb(sc.ctx, xh.data(), N, B, sc_h.data());
    if (rc != 0) return fb_fail(FB_E_CALLBACK, "score callback failed (rc %d)", rc);
  }
  FBCHK(h2d(e, e->raw.p, sc_h.data(), sizeof(double) * sc_h.size()));
  e->foreign.model_calls += 1;
  e->foreign.batch_bytes_d2h += (int64_t)xb;
  e->foreign.score_bytes_h2d += (int64_t)(sizeof(double) * sc_h.size());
  fb_launch_loss(e->stream, e->raw.as<double>(), nullptr, B, S, p->task, 1, p->attack_type, e->ext_z.as<double>(),
                 e->ext_z.as<double>() + 64, p->threshold, p->adver_thresh, p->target, p->true_label,
                 e->dist_part.as<double>(), with_dist ? ndp : 0, e->scores.as<double>(), e->loss.as<double>(),
                 e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row);
  e->nes_route[FB_NES_ROUTE_K_LOSS] += 1;
  return FB_OK;
}

// ------------------------------------------- foreign models on the same GPU (fb_get_grad_dev / fb_attack_dev)
// The batch goes into the caller's device buffer (k_perturb_x, k_update_perturb_x), the callback enqueues the model on
// the engine's stream, and the loss reads the model's scores where it wrote them: no copy through the host, and the host
// looks at the control block every look_every iterations as fb_attack does.
static int check_dev_buffer(fb_engine *e, const char *what, const void *ptr, size_t bytes) {
  if (!ptr) return fb_fail(FB_E_ARG, "%s is NULL", what);
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  const hipError_t rc = hipPointerGetAttributes(&a, ptr);
  if (rc != hipSuccess) {
    (void)hipGetLastError();  // (an unknown host pointer: not a sticky error)
    return fb_fail(FB_E_ARG, "%s is not device memory (hipPointerGetAttributes: %s)", what, hipGetErrorString(rc));
  }
  if (a.type != hipMemoryTypeDevice) return fb_fail(FB_E_ARG, "%s is not device memory (memory type %d)", what, (int)a.type);
  if (a.device != e->device)
    return fb_fail(FB_E_ARG, "%s is memory of device %d, the engine runs on device %d", what, a.device, e->device);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) == hipSuccess) {
    const size_t room = (size_t)(static_cast<const char *>(base) + size - static_cast<const char *>(ptr));
    if (room < bytes) return fb_fail(FB_E_ARG, "%s: %zu bytes needed, its allocation holds %zu from there", what, bytes, room);
  } else {
    (void)hipGetLastError();
  }
  return FB_OK;
}

static int check_dev_model(fb_engine *e, const fb_dev_model *m, int64_t N, int B, int S) {
  if (!m) return fb_fail(FB_E_ARG, "null argument");
  if (m->x_dtype != FB_DT_F32 && m->x_dtype != FB_DT_F64)
    return fb_fail(FB_E_ARG, "x_dtype %d: FB_DT_F32 (%d) or FB_DT_F64 (%d)", m->x_dtype, FB_DT_F32, FB_DT_F64);
  if (m->score_dtype != FB_DT_F32 && m->score_dtype != FB_DT_F64)
    return fb_fail(FB_E_ARG, "score_dtype %d: FB_DT_F32 (%d) or FB_DT_F64 (%d)", m->score_dtype, FB_DT_F32, FB_DT_F64);
  if (m->look_every < 0) return fb_fail(FB_E_ARG, "look_every %d < 0", m->look_every);
  const size_t xe = m->x_dtype == FB_DT_F32 ? sizeof(float) : sizeof(double);
  const size_t se = m->score_dtype == FB_DT_F32 ? sizeof(float) : sizeof(double);
  FBCHK(check_dev_buffer(e, "x", m->x, xe * (size_t)N * (size_t)B));
  FBCHK(check_dev_buffer(e, "scores", m->scores, se * (size_t)B * (size_t)S));
  return FB_OK;
}

// the model's work on the engine's stream, then the loss (+ loop control) on its scores
static int enqueue_score_loss_dev(fb_engine *e, const fb_nes_params *p, const FbScorer &sc, int64_t N, int ndp,
                                  FbCtlDev *ctl, double *trace_dev, int trace_row) {
  const int B = 2 * (p->samples_per_draw / 2) + 1, S = sc.S;
  const int rc = sc.dcb(sc.ctx, (void *)e->stream, N, B, S);
  e->foreign.model_calls += 1;
  if (rc != 0) {
    (void)sync_stream(e);  // (whatever the model did enqueue has finished when the caller sees the error)
    return fb_fail(FB_E_CALLBACK, "score callback failed (rc %d)", rc);
  }
  if (sc.m->score_dtype == FB_DT_F32)
    fb_launch_loss(e->stream, static_cast<const float *>(sc.m->scores), nullptr, B, S, p->task, 1, p->attack_type,
                   e->ext_z.as<double>(), e->ext_z.as<double>() + 64, p->threshold, p->adver_thresh, p->target,
                   p->true_label, e->dist_part.as<double>(), ndp, e->scores.as<double>(), e->loss.as<double>(),
                   e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row);
  else
    fb_launch_loss(e->stream, static_cast<const double *>(sc.m->scores), nullptr, B, S, p->task, 1, p->attack_type,
                   e->ext_z.as<double>(), e->ext_z.as<double>() + 64, p->threshold, p->adver_thresh, p->target,
                   p->true_label, e->dist_part.as<double>(), ndp, e->scores.as<double>(), e->loss.as<double>(),
                   e->nes_out.as<FbNesDev>(), ctl, trace_dev, trace_row);
  e->nes_route[FB_NES_ROUTE_K_LOSS] += 1;
  return FB_OK;
}

static bool x_aligned(const fb_dev_model *m) { return (reinterpret_cast<uintptr_t>(m->x) & 15) == 0; }

// a foreign model's scores are final: k_loss reads them under the z-norm of the identity, (s - 0) / 1 == s bit for bit
static int ensure_identity_znorm(fb_engine *e) {
  const size_t had = e->ext_z.cap;
  FBCHK(e->ext_z.ensure(sizeof(double) * 2 * 64));
  if (e->ext_z.cap != had) {
    double z[128];
    for (int i = 0; i < 64; ++i) { z[i] = 0.0; z[64 + i] = 1.0; }
    FBCHK(h2d(e, e->ext_z.p, z, sizeof(z)));
  }
  return FB_OK;
}

// ------------------------------------------------- the NES driver of every scorer
// Checks and buffers of a NES call.  attack: fb_attack*, which also need max_iter > 0.
static int nes_setup(fb_engine *e, const fb_nes_params *p, int64_t N, FbScorer &sc, bool attack) {
  const bool native = sc.kind == FB_SCORER_NATIVE;
  FBCHK(native ? check_params(e, p, N) : check_params_ext(e, p, N, sc.S, sc.cb || sc.dcb));
  if (attack && p->max_iter <= 0) return fb_fail(FB_E_ARG, "max_iter must be > 0");
  HIPCHK(hipSetDevice(e->device));
  const int B = 2 * (p->samples_per_draw / 2) + 1;
  if (native) {
    sc.S = fb_num_speakers(e);
    FBCHK(prepare_nes_replicas(e, N, B));
    return ensure_nes_buffers(e, N, B);
  }
  FBCHK(sync_stream(e));
  if (sc.kind == FB_SCORER_DEV) FBCHK(check_dev_model(e, sc.m, N, B, sc.S));
  FBCHK(ensure_nes_buffers(e, N, B, sc.S));
  if (sc.kind == FB_SCORER_HOST) {
    FBCHK(e->ext_x.ensure(sizeof(double) * (size_t)N * B));
    FBCHK(e->raw.ensure(sizeof(double) * (size_t)B * sc.S));
  }
  return ensure_identity_znorm(e);
}

// fb_get_grad*: one NES gradient estimate at `audio`
static int nes_gradient(fb_engine *e, const fb_nes_params *p, FbScorer sc, const double *audio, int64_t N,
                        uint32_t iter, const double *noise_pos, double *final_loss, double *grad, double *adver_loss,
                        double *score0) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (e) memset(e->nes_route, 0, sizeof(e->nes_route));
  if (!audio) return fb_fail(FB_E_ARG, "audio is NULL");
  FBCHK(nes_setup(e, p, N, sc, false));
  const bool native = sc.kind == FB_SCORER_NATIVE;
  if (!native) foreign_begin(e, sc, 3);  // k_perturb_f64 / k_perturb_x, k_loss, k_grad_update
  const int half = p->samples_per_draw / 2;
  FBCHK(h2d(e, e->adver.p, audio, sizeof(double) * (size_t)N));
  if (native) cast_a0(e, p, e->adver.as<double>(), N);
  const double *noise_dev = nullptr;
  if (noise_pos && half > 0) {
    FBCHK(e->noise.ensure(sizeof(double) * (size_t)N * half));
    FBCHK(h2d(e, e->noise.p, noise_pos, sizeof(double) * (size_t)N * half));
    noise_dev = e->noise.as<double>();
  }
  switch (sc.kind) {
    case FB_SCORER_NATIVE:
      FBCHK(enqueue_get_grad(e, p, N, iter, noise_dev, false));
      break;
    case FB_SCORER_HOST:
      FBCHK(enqueue_get_grad_ext(e, p, sc, N, iter, noise_dev, false));
      break;
    case FB_SCORER_DEV:  // (no loop control: no stop flag)
      fb_launch_perturb_x(e->stream, sc.m->x_dtype, e->adver.as<double>(), nullptr, N, half, p->sigma, p->seed, iter,
                          p->stream, noise_dev, sc.m->x, x_aligned(sc.m), e->dist_part.as<double>(), nullptr,
                          noise_dev ? nullptr : e->zbuf.as<float>(), nullptr);
      record_nes_batch(e, iter, N, half, false, !noise_dev);
      FBCHK(enqueue_score_loss_dev(e, p, sc, N, 0, nullptr, nullptr, 0));
      break;
  }
  fb_launch_grad_update(e->stream, e->loss.as<double>(), N, half, p->sigma, e->zbuf.as<float>(), noise_dev,
                        e->grad.as<double>(), 0, 0.0, 0.0, 0.0, 0.0, nullptr, nullptr, nullptr);
  e->nes_route[FB_NES_ROUTE_K_GRAD_UPDATE] += 1;
  if (grad) FBCHK(d2h(e, grad, e->grad.p, sizeof(double) * (size_t)N));
  FBCHK(fetch_out(e, native));
  e->nes_iters += 1;
  e->nes_rec.iter = e->nes_rec.queued;
  if (final_loss) *final_loss = e->h_out->final_loss;
  if (adver_loss) *adver_loss = e->h_out->adver_loss;
  if (score0) for (int s = 0; s < sc.S; ++s) score0[s] = e->h_out->score0[s];
  return FB_OK;
}

// the start of an attack: adver = audio, grad = 0 (FAKEBOB.py:157), room for replayed normals
static int attack_start(fb_engine *e, const double *audio, int64_t N, int half, const double *noise_all) {
  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  HIPCHK(hipMemcpyAsync(e->adver.p, e->audio.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemsetAsync(e->grad_m.p, 0, sizeof(double) * (size_t)N, e->stream));
  if (noise_all && half > 0) FBCHK(e->noise.ensure(sizeof(double) * (size_t)N * half));
  return FB_OK;
}

// The engine's own launch state at the start of an attack on its own system
static int launch_state_reset(fb_engine *e) {
  e->pre_iter = -1;
  // The ticket of k_vad_delta_cmvn and the arrival counter of k_gmm_finalize_loss are left at zero by every launch
  // that completes; one that was aborted or failed would leave them elsewhere and every later launch would then
  // mis-assign utterances / skip its loss body.  A new attack starts them clean.
  if (e->vad_counter.p) HIPCHK(hipMemsetAsync(e->vad_counter.p, 0, sizeof(int), e->stream));
  if (e->fin_counter.p) HIPCHK(hipMemsetAsync(e->fin_counter.p, 0, 2 * sizeof(int), e->stream));
  e->fin_xch_clean = false;  // (refilled with sentinels before its next use)
  if (e->iv_tail_counter.p) HIPCHK(hipMemsetAsync(e->iv_tail_counter.p, 0, sizeof(int), e->stream));
  e->vad_part_B = -1;  // ... and k_vad_delta_cmvn_p's exchange slots are refilled with sentinels (run_post_mfcc)
  e->ctl_seq = 0;   // (h.pub_seq = 0: the loss bodies of this attack count from 1)
  return FB_OK;
}
// A new attack's loop control (lr = max_lr, empty loss history) on the device; ticks (nullable) get the start stamp.
// native: the engine's own launch state starts clean as well -- the foreign paths use none of it.
static int ctl_reset(fb_engine *e, const fb_nes_params *p, bool native, bool disable_stop, unsigned long long *ticks) {
  if (native) FBCHK(launch_state_reset(e));
  FBCHK(e->ctl.ensure(sizeof(FbCtlDev)));
  FBCHK(e->ctl_ls.ensure(sizeof(double) * (size_t)(p->plateau_length > 0 ? p->plateau_length : 1)));
  FbCtlDev h;
  memset(&h, 0, sizeof(h));
  h.lr = p->max_lr; h.min_lr = p->min_lr; h.plateau_drop = p->plateau_drop;
  h.ls = e->ctl_ls.as<double>();
  h.plateau_length = p->plateau_length;
  h.disable_stop = disable_stop ? 1 : 0;
  h.ticks = ticks;
  *e->h_ctl = h;
  HIPCHK(hipMemcpyAsync(e->ctl.p, e->h_ctl, sizeof(FbCtlDev), hipMemcpyHostToDevice, e->stream));
  FBCHK(sync_stream(e));  // h_ctl is reused for the read-back in attack_loop
  if (ticks) fb_launch_stamp(e->stream, ticks);
  return FB_OK;
}

// The NES loop of FakeBob.attack (FAKEBOB.py:171-216) with the loop control on the device (FbCtlDev): `count`
// iterations starting at Philox iteration index `it_base` are queued kn.look at a time; the host reads the control block
// once per look and stops when it is told to.  trace_dev rows are indexed from it_base.
static int attack_loop(fb_engine *e, const fb_nes_params *p, int64_t N, const FbScorer &sc, const FbLoopKnobs &kn,
                       const double *noise_all, int it_base, int count, double *trace_dev) {
  const int half = p->samples_per_draw / 2;
  const double one_minus_m = 1.0 - p->momentum;
  const bool upd_next = fuses_update(kn, noise_all, half);
  FbCtlDev *ctl = e->ctl.as<FbCtlDev>();
  int ndp = 0;              // FB_SCORER_DEV: the distance partials of the batch the previous iteration's update wrote
  bool have_batch = false;  // ... if it wrote one
  auto queue_iteration = [&](const int it) -> int {
    {
      const double *noise_dev = nullptr;
      if (noise_all && half > 0) {
        FBCHK(h2d(e, e->noise.p, noise_all + (size_t)it * N * half, sizeof(double) * (size_t)N * half));
        noise_dev = e->noise.as<double>();
      }
      bool updated = false;  // the momentum sign step of this iteration is queued
      switch (sc.kind) {
        case FB_SCORER_NATIVE: {
          if (fb_debug_sync_on()) fprintf(stderr, "[fb] iteration %d\n", it);
          // GMM systems on the fused chain: the update of this iteration and the batch of the next one ride in the
          // launch that finalises the scores and runs the loss body (k_gmm_finalize_loss_update; FB_FUSE_UPD=0: two
          // launches) (at most FB_FUSE_MAX_UPD_WG update workgroups in the finalising launch: the bound its no-deadlock
          // argument needs)
          FbUpdArgs ua = {};
          if (upd_next && kn.fuse_fin && kn.upd_in_fin && e->kind == 0 && (N + 255) / 256 <= FB_FUSE_MAX_UPD_WG) {
            ua.loss = e->loss.as<double>(); ua.N = N; ua.half = half; ua.sigma = p->sigma; ua.zbuf = e->zbuf.as<float>();
            ua.momentum = p->momentum; ua.one_minus_m = one_minus_m; ua.epsilon = p->epsilon; ua.audio = e->audio.as<double>();
            ua.grad_m = e->grad_m.as<double>(); ua.adver = e->adver.as<double>(); ua.seed = p->seed; ua.next_iter = (uint32_t)(it + 1);
            ua.stream = p->stream; ua.q = e->wav.as<int16_t>(); ua.dist_part = e->dist_part.as<double>();
            ua.qscale = ldexp(1.0, nes_bits(p) - 1);
          }
          FBCHK(enqueue_get_grad(e, p, N, (uint32_t)it, noise_dev, true, kn, ctl, trace_dev, it - it_base,
                                 ua.loss ? &ua : nullptr, &updated));
          FB_DBG_SYNC(e, "loss");
          if (updated) {
            e->pre_ndp = (int)((N + 255) / 256);
            e->pre_iter = (long long)it + 1;
            record_nes_batch(e, (long long)it + 1, N, half, nes_replicas(e) == 1, true);
            record_update_threads(e, 512);  // (the update workgroups of k_gmm_finalize_loss_update)
          } else if (upd_next) {
            e->pre_ndp = fb_launch_update_perturb(e->stream, e->loss.as<double>(), N, half, p->sigma, e->zbuf.as<float>(),
                                                  p->momentum, one_minus_m, p->epsilon, e->audio.as<double>(),
                                                  e->grad_m.as<double>(), e->adver.as<double>(), ctl, p->seed,
                                                  (uint32_t)(it + 1), p->stream, e->wav.as<int16_t>(),
                                                  e->dist_part.as<double>(), nes_bits(p), kn.upd_threads);
            record_update_threads(e, kn.upd_threads);
            e->nes_route[FB_NES_ROUTE_K_UPDATE_PERTURB] += 1;
            e->pre_iter = (long long)it + 1;
            record_nes_batch(e, (long long)it + 1, N, half, nes_replicas(e) == 1, true);
            updated = true;
          }
          break;
        }
        case FB_SCORER_HOST:
          FBCHK(enqueue_get_grad_ext(e, p, sc, N, (uint32_t)it, noise_dev, true, ctl, trace_dev, it - it_base));
          break;
        case FB_SCORER_DEV: {
          const int xv = x_aligned(sc.m) ? 1 : 0;
          if (!have_batch) {
            fb_launch_perturb_x(e->stream, sc.m->x_dtype, e->adver.as<double>(), e->audio.as<double>(), N, half, p->sigma,
                                p->seed, (uint32_t)it, p->stream, noise_dev, sc.m->x, xv, e->dist_part.as<double>(), &ndp,
                                noise_dev ? nullptr : e->zbuf.as<float>(), &ctl->stop);
            record_nes_batch(e, it, N, half, false, !noise_dev);
          }
          FBCHK(enqueue_score_loss_dev(e, p, sc, N, ndp, ctl, trace_dev, it - it_base));
          if (upd_next) {
            ndp = fb_launch_update_perturb_x(e->stream, sc.m->x_dtype, e->loss.as<double>(), N, half, p->sigma,
                                             e->zbuf.as<float>(), p->momentum, one_minus_m, p->epsilon,
                                             e->audio.as<double>(), e->grad_m.as<double>(), e->adver.as<double>(), ctl,
                                             p->seed, (uint32_t)(it + 1), p->stream, sc.m->x, xv,
                                             e->dist_part.as<double>(), kn.upd_threads);
            record_update_threads(e, kn.upd_threads);
            record_nes_batch(e, (long long)it + 1, N, half, false, true);
            e->nes_route[FB_NES_ROUTE_K_UPDATE_PERTURB] += 1;
            have_batch = updated = true;
          }
          break;
        }
      }
      if (!updated) {
        fb_launch_grad_update(e->stream, e->loss.as<double>(), N, half, p->sigma, e->zbuf.as<float>(), noise_dev,
                              nullptr, 1, p->momentum, one_minus_m, 0.0, p->epsilon, e->audio.as<double>(),
                              e->grad_m.as<double>(), e->adver.as<double>(), ctl);
        e->nes_route[FB_NES_ROUTE_K_GRAD_UPDATE] += 1;
      }
    }
    return FB_OK;
  };
  // The engine's own systems on Philox noise: batch n + 1 is queued BEFORE the host waits for batch n's control block, so the
  // stream never runs dry at a look (one stream synchronisation and the relaunch of an empty stream per look otherwise:
  // DESIGN.md section 7).  Two pinned copies of the block and an event each; the timing events alternate between two banks
  // with them.  Kernels queued behind the stopping iteration return on the stop flag and leave the block as it is, so the
  // block of the last batch waited for is the attack's final one.  Uploaded normals (e->noise is rewritten per iteration
  // from the host), a host callback and a foreign model on the device (every batch queued is a query of the victim) keep
  // the draining loop.
  const bool ahead = kn.look_ahead && sc.kind == FB_SCORER_NATIVE && !noise_all;
  int waiting = -1;  // the copy (and timing bank) of the batch the host has not looked at yet
  bool stop = false;
  // a failed call ends the attack: nothing of it stays in flight (the batch queued ahead included), and the next call
  // records its timing events into bank 0 again
  auto abandon = [&](int rc) {
    e->evg_cur = 0;
    (void)hipStreamSynchronize(e->stream);
    return rc;
  };
  for (int queued = 0, n = 0; (queued < count && !stop) || waiting >= 0; ++n) {
    int cur = -1;
    if (queued < count && !stop) {
      const int nb = count - queued < kn.look ? count - queued : kn.look;
      cur = ahead ? (n & 1) : 0;
      e->evg_cur = cur;
      int rc = FB_OK;
      for (int k = 0; k < nb && rc == FB_OK; ++k) rc = queue_iteration(it_base + queued + k);
      hipError_t he = hipSuccess;
      if (rc == FB_OK) he = hipMemcpyAsync(ahead ? e->h_look[cur] : e->h_ctl, ctl, sizeof(FbCtlDev), hipMemcpyDeviceToHost, e->stream);
      if (rc == FB_OK && he == hipSuccess && ahead) he = hipEventRecord(e->ev_look[cur], e->stream);
      if (rc != FB_OK || he != hipSuccess) {
        (void)abandon(rc);
        HIPCHK(he);
        return rc;
      }
      queued += nb;
    }
    const int look_at = ahead ? waiting : cur;
    waiting = ahead ? cur : -1;
    if (look_at < 0) continue;  // (the first batch of a loop that looks ahead: nothing to wait for yet)
    if (ahead) {
      const hipError_t he = hipEventSynchronize(e->ev_look[look_at]);
      if (he != hipSuccess) {
        (void)abandon(FB_OK);
        HIPCHK(he);
      }
      *e->h_ctl = *e->h_look[look_at];
    } else {
      FBCHK(sync_stream(e));
    }
    if (sc.kind == FB_SCORER_NATIVE && e->evg_n[look_at] > 0) {
      const int rc = time_collect_bank(e, look_at);
      if (rc != FB_OK) return abandon(rc);
    }
    // err on a foreign path is never set: k_loss sets it only when it has the voiced-frame counts (tv), and only the
    // native systems pass them (fb_nes_device.h)
    if (e->h_ctl->err != 0) {
      e->evg_cur = 0;
      if (waiting >= 0) {  // the batch queued ahead returns on the stop flag the error set
        FBCHK(sync_stream(e));
        FBCHK(time_collect(e));
      }
      return fb_fail(FB_E_NO_VOICED, "NES sample %d has no voiced frames", e->h_ctl->err - 1);
    }
    if (e->h_ctl->stop) stop = true;
  }
  e->evg_cur = 0;
  return FB_OK;
}

// fb_attack*: FakeBob.attack (FAKEBOB.py:157-220) -> int16 adver, success flag, float64 adver, trace
static int run_attack(fb_engine *e, const fb_nes_params *p, FbScorer sc, const double *audio, int64_t N,
                      const double *noise_all, int16_t *adv_i16, double *adver_f64, double *trace, int *n_trace,
                      int *success_flag) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (e) memset(e->nes_route, 0, sizeof(e->nes_route));
  if (!audio || !adv_i16 || !success_flag) return fb_fail(FB_E_ARG, "null argument");
  FBCHK(nes_setup(e, p, N, sc, true));
  const bool native = sc.kind == FB_SCORER_NATIVE;
  const int half = p->samples_per_draw / 2, B = 2 * half + 1, S = sc.S;
  const FbLoopKnobs kn = loop_knobs(e, sc);
  // the device path's update and next batch in one launch: k_update_perturb_x instead of k_grad_update + k_perturb_x
  if (!native) foreign_begin(e, sc, fuses_update(kn, noise_all, half) ? 2 : 3);
  FBCHK(attack_start(e, audio, N, half, noise_all));
  if (native) cast_a0(e, p, e->audio.as<double>(), N);
  double *trace_dev = nullptr;
  if (trace) {
    FBCHK(e->trace_dev.ensure(sizeof(double) * (size_t)p->max_iter * (3 + S)));
    trace_dev = e->trace_dev.as<double>();
  }
  FBCHK(e->ticks.ensure(sizeof(unsigned long long) * ((size_t)p->max_iter + 1)));
  FBCHK(ctl_reset(e, p, native, false, e->ticks.as<unsigned long long>()));
  FBCHK(attack_loop(e, p, N, sc, kn, noise_all, 0, p->max_iter, trace_dev));
  const int rows = e->h_ctl->iters_done;  // one trace row per executed iteration, the stopping one included
  e->nes_iters += rows;
  FBCHK(collect_iter_seconds(e, rows));
  if (trace && rows > 0) FBCHK(d2h(e, trace, trace_dev, sizeof(double) * (size_t)rows * (3 + S)));
  const int last_iter = e->h_ctl->broke ? e->h_ctl->stop_iter : p->max_iter - 1;
  *success_flag = (last_iter < p->max_iter - 1) ? 1 : -1;  // :219
  if (n_trace) *n_trace = rows;
  // adver -> int16 (:220)
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * (native ? B : 1)));
  if (!native) e->cached_B = -1;  // the scoring batch layout no longer describes e->wav
  fb_launch_quantize(e->stream, e->adver.as<double>(), N, nes_bits(p), e->wav.as<int16_t>());
  FBCHK(d2h(e, adv_i16, e->wav.p, sizeof(int16_t) * (size_t)N));
  if (adver_f64) FBCHK(d2h(e, adver_f64, e->adver.p, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  // the batch launches queued behind a stopping iteration returned on its flag: that iteration's rows are the resident ones
  e->nes_rec.iter = e->h_ctl->broke ? (long long)e->h_ctl->stop_iter : e->nes_rec.queued;
  return FB_OK;
}

// ------------------------------------------------- the public NES calls
extern "C" int fb_get_grad(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, uint32_t iter,
                           const double *noise_pos, double *final_loss, double *grad, double *adver_loss,
                           double *score0) {
  return nes_gradient(e, p, FbScorer{FB_SCORER_NATIVE}, audio, N, iter, noise_pos, final_loss, grad, adver_loss, score0);
}

extern "C" int fb_get_grad_ext(fb_engine *e, const fb_nes_params *p, int S, fb_score_cb cb, void *cb_ctx,
                               const double *audio, int64_t N, uint32_t iter, const double *noise_pos,
                               double *final_loss, double *grad, double *adver_loss, double *score0) {
  return nes_gradient(e, p, FbScorer{FB_SCORER_HOST, S, cb, nullptr, nullptr, cb_ctx}, audio, N, iter, noise_pos,
                      final_loss, grad, adver_loss, score0);
}

extern "C" int fb_get_grad_dev(fb_engine *e, const fb_nes_params *p, int S, const fb_dev_model *m, fb_score_dev_cb cb,
                               void *ctx, const double *audio, int64_t N, uint32_t iter, const double *noise_pos,
                               double *final_loss, double *grad, double *adver_loss, double *score0) {
  return nes_gradient(e, p, FbScorer{FB_SCORER_DEV, S, nullptr, m, cb, ctx}, audio, N, iter, noise_pos, final_loss,
                      grad, adver_loss, score0);
}

extern "C" int fb_attack(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N,
                         const double *noise_all, int16_t *adv_i16, double *adver_f64, double *trace,
                         int *n_trace, int *success_flag) {
  return run_attack(e, p, FbScorer{FB_SCORER_NATIVE}, audio, N, noise_all, adv_i16, adver_f64, trace, n_trace,
                    success_flag);
}

extern "C" int fb_attack_ext(fb_engine *e, const fb_nes_params *p, int S, fb_score_cb cb, void *cb_ctx,
                             const double *audio, int64_t N, const double *noise_all, int16_t *adv_i16,
                             double *adver_f64, double *trace, int *n_trace, int *success_flag) {
  return run_attack(e, p, FbScorer{FB_SCORER_HOST, S, cb, nullptr, nullptr, cb_ctx}, audio, N, noise_all, adv_i16,
                    adver_f64, trace, n_trace, success_flag);
}

extern "C" int fb_attack_dev(fb_engine *e, const fb_nes_params *p, int S, const fb_dev_model *m, fb_score_dev_cb cb,
                             void *ctx, const double *audio, int64_t N, const double *noise_all, int16_t *adv_i16,
                             double *adver_f64, double *trace, int *n_trace, int *success_flag) {
  return run_attack(e, p, FbScorer{FB_SCORER_DEV, S, nullptr, m, cb, ctx}, audio, N, noise_all, adv_i16, adver_f64,
                    trace, n_trace, success_flag);
}

// ------------------------------------------------- white-box gradients: fb_get_grad_wb / fb_attack_wb
// The analytic gradient of the loss with respect to the samples ("white-box gradients" in fakebob_hip.h): GMM-UBM systems on
// an undefended victim; with fb_set_wb_bpda(e, 1) through an input-transform chain, a codec and EOT replicas as well
// (BPDA / EOT, the same contract); with fb_set_wb_ivector(e, 1) i-vector-PLDA systems too; with fb_set_wb_xvector(e, 1) x-vector
// systems (undefended or under fb_set_wb_bpda; never with a channel, dither, companions or a play offset); with fb_set_wb_air(e, 1) through an
// over-the-air channel; with fb_set_wb_frontend(e, 1) through feature compression and dither; with fb_set_wb_universal(e, 1) over
// the companions of a universal perturbation.  Everything else is refused by name.
static int wb_check(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, fb_nes_params *q) {
  if (!e || !p || !audio) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  if (e->kind == 2 && !e->wb_xvector)
    return fb_fail(FB_E_STATE, "white-box gradients: an x-vector system is loaded (no gradient through the TDNN: not in this version)");
  if (e->kind == 2) {
    // fb_set_wb_xvector: undefended, or with fb_set_wb_bpda through a chain, a codec and EOT replicas (the generic checks below);
    // these four stay refused whatever their own switches say
    if (e->air.L > 0)
      return fb_fail(FB_E_STATE, "white-box gradients: an air channel is set (fb_set_air_channel: not through an x-vector system in this version: clear it)");
    if (e->cfg.dither > 0.0)
      return fb_fail(FB_E_STATE, "white-box gradients: dither %g > 0 (not through an x-vector system in this version)", e->cfg.dither);
    if (e->comp_K1 > 0)
      return fb_fail(FB_E_STATE, "white-box gradients: companions are set (fb_set_companions: not through an x-vector system in this version: clear them)");
    if (e->play_S > 0)
      return fb_fail(FB_E_STATE, "white-box gradients: a play offset is set (fb_set_play_offset(%lld): not through an x-vector system in this version)",
                     (long long)e->play_S);
  }
  if (e->kind == 1 && !e->wb_ivector)
    return fb_fail(FB_E_STATE, "white-box gradients: an i-vector system is loaded (GMM-UBM systems only in this version)");
  // (the forward keeps the selection, posteriors and statistics of ONE row for the backward, not those of r replicas)
  // (... unless fb_set_wb_universal: the forward then keeps quad of every replica, and sel / post / the i-vectors are per row anyway)
  if (e->kind == 1 && e->eot > 1 && !e->wb_universal)
    return fb_fail(FB_E_STATE, "white-box gradients: fb_set_eot(%d) is in force on an i-vector system (per-replica i-vector state is not kept: set 1)", e->eot);
  if (e->eot > 1 && !e->wb_bpda) return fb_fail(FB_E_STATE, "white-box gradients: fb_set_eot(%d) is in force (set 1)", e->eot);
  // (the universal perturbation has the fifth switch, fb_set_wb_universal: refused with the other four on as well)
  if (e->comp_K1 > 0 && !e->wb_universal) return fb_fail(FB_E_STATE, "white-box gradients: companions are set (fb_set_companions: clear them)");
  // (a play offset rides on the universal path: k_wb_play_compose_t in k_wb_compose_t's place)
  if (e->play_S > 0 && !e->wb_universal)
    return fb_fail(FB_E_STATE, "white-box gradients: a play offset is set (fb_set_play_offset(%lld)) without fb_set_wb_universal: not in this version",
                   (long long)e->play_S);
  FBCHK(check_play_length(e, N));
  if (e->tf.n > 0 && !e->wb_bpda)
    return fb_fail(FB_E_STATE, "white-box gradients: an input-transform chain is set (no BPDA through defences in this version)");
  // (the channel's transpose is a switch of its own, fb_set_wb_air: refused with the other two on as well)
  if (e->air.L > 0 && !e->wb_air) return fb_fail(FB_E_STATE, "white-box gradients: an air channel is set (fb_set_air_channel: clear it)");
  if (e->codec != FB_CODEC_NONE && !e->wb_bpda) return fb_fail(FB_E_STATE, "white-box gradients: a codec is set (fb_set_codec: clear it)");
  // (feature compression and dither have the fourth switch, fb_set_wb_frontend: refused with the other three on as well)
  if (e->feco_iters > 0 && !e->wb_frontend)
    return fb_fail(FB_E_STATE, "white-box gradients: feature compression is on (fb_set_feature_compression: switch it off)");
  if (e->cfg.dither > 0.0 && !e->wb_frontend) return fb_fail(FB_E_STATE, "white-box gradients: dither %g > 0 (the function is differentiated at a fixed victim)", e->cfg.dither);
  // one row is scored per iteration; of the NES-only fields seed and stream key the draws of a randomised defence
  *q = *p;
  q->samples_per_draw = 0;
  q->sigma = 1.0;
  return check_params(e, q, N);
}

// the TDNN backward's workspace for B utterances of `rows` rows in all; cap64: rows per utterance in e->wb_xv_g
static int wb_xv_ensure(fb_engine *e, int B, size_t rows, int cap64) {
  const FbXvDev &xv = e->xv;
  if (rows < 1) rows = 1;
  size_t maxK = 1;
  for (int l = 0; l < xv.n_layers; ++l) maxK = std::max(maxK, (size_t)xv.layer[l].K);
  FBCHK(e->wb_xv_ebar.ensure(sizeof(double) * (size_t)B * xv.R));
  FBCHK(e->wb_xv_sbar.ensure(sizeof(double) * (size_t)B * 2 * xv.P));
  for (int i = 0; i < 2; ++i) FBCHK(e->wb_xv_y[i].ensure(sizeof(float) * rows * (size_t)xv.max_width));
  FBCHK(e->wb_xv_z.ensure(sizeof(float) * rows * (size_t)xv.max_width));
  FBCHK(e->wb_xv_G.ensure(sizeof(float) * rows * maxK));
  FBCHK(e->wb_xv_amax.ensure(sizeof(float) * rows));
  FBCHK(e->wb_xv_g.ensure(sizeof(double) * (size_t)B * (size_t)(cap64 > 0 ? cap64 : 1) * xv.D));
  return FB_OK;
}
// The TDNN's backward over the whole batch the forward just scored with its masks kept (B utterances, at most rows_cap rows;
// e->row_off / e->xv_rowinfo / e->xv_stats / the last layer's output as the forward left them): from the cotangents
// e->wb_xv_ebar [B][R] on the embeddings down to stage `down_to` (fb_debug_xv_backward's numbering; 0: the feature rows, float64
// in e->wb_xv_g with cap64 rows per utterance).  *last32 (nullable): where a stage in 1 .. n_layers left its float32 cotangent.
// wb_xv_ensure has sized the buffers.
static void wb_xv_backward(fb_engine *e, int B, int rows_cap, int down_to, int cap64, const int *stop, const float **last32) {
  const FbXvDev &xv = e->xv;
  hipStream_t s = e->stream;
  const int *row_off = e->row_off.as<int>(), *n_rows = row_off + B;
  const int2 *rowinfo = e->xv_rowinfo.as<int2>();
  fb_launch_wb_xv_segment_t(s, xv, e->wb_xv_ebar.as<double>(), B, e->wb_xv_sbar.as<double>(), stop);
  e->wb_xv_route[FB_WB_XV_ROUTE_SEGMENT_T] += 1;
  if (down_to > xv.n_layers) return;
  int cur = 0;
  fb_launch_wb_xv_pool_t(s, e->xv_act[(xv.n_layers - 1) & 1].as<float>(), xv.P, row_off, B, e->xv_stats.as<double>(),
                         e->wb_xv_sbar.as<double>(), e->wb_xv_y[cur].as<float>(), stop);
  e->wb_xv_route[FB_WB_XV_ROUTE_POOL_T] += 1;
  for (int l = xv.n_layers - 1; l >= down_to; --l) {
    const FbXvLayerDev &ly = xv.layer[l];
    fb_launch_wb_xv_act_t(s, ly, e->wb_xv_y[cur].as<float>(), e->xv_mask[l].as<unsigned char>(), n_rows, rows_cap, e->wb_xv_z.as<float>(),
                          e->wb_xv_amax.as<float>(), stop);
    e->wb_xv_route[FB_WB_XV_ROUTE_ACT_T] += 1;
    fb_launch_wb_xv_affine_t(s, ly, e->wb_xv_z.as<float>(), e->wb_xv_amax.as<float>(), n_rows, rows_cap, e->wb_xv_G.as<float>(), stop);
    e->wb_xv_route[FB_WB_XV_ROUTE_AFFINE_T] += 1;
    fb_launch_wb_xv_unsplice(s, ly, e->wb_xv_G.as<float>(), rowinfo, row_off, B, n_rows, rows_cap, l > 0 ? e->wb_xv_y[cur ^ 1].as<float>() : nullptr,
                             l > 0 ? nullptr : e->wb_xv_g.as<double>(), cap64, stop);
    e->wb_xv_route[FB_WB_XV_ROUTE_UNSPLICE] += 1;
    cur ^= 1;
  }
  if (last32) *last32 = e->wb_xv_y[cur].as<float>();
}

// the plain parameters on the device (once per fb_load_gmm) and the workspace of one utterance of N samples / T frames
static int wb_prepare(fb_engine *e, int64_t N, int T, bool need_gmm) {
  const FbFrontendDev &fe = e->fe;
  if (need_gmm && e->kind == 1) {
    // the i-vector back end's backward: weights, the adjoint solve's matrix and workspace (k_iv_solve_ll wants a row of
    // R + 64 zeros behind the right-hand side row and its own slots for the inverted diagonal blocks), Fbar / Nbar
    const FbIvDev &iv = e->iv;
    const size_t npanel = ((size_t)iv.R + 31) / 32;
    FBCHK(e->wb_w.ensure(sizeof(double) * (size_t)iv.S));
    // (under fb_set_wb_universal every replica's copy of quad: R * triR doubles, about 20 MB at R = 32 for the recipe's size)
    FBCHK(e->wb_iv_quad.ensure(sizeof(double) * (size_t)(e->wb_universal ? nes_replicas(e) : 1) * (size_t)iv.triR));
    FBCHK(e->wb_iv_linv.ensure(sizeof(double) * npanel * 32 * 32));
    FBCHK(e->wb_iv_wbar.ensure(sizeof(double) * (size_t)iv.R));
    FBCHK(e->wb_iv_lam.ensure(sizeof(double) * (size_t)iv.R));
    FBCHK(e->wb_iv_fbar.ensure(sizeof(double) * (size_t)iv.C * iv.D));
    FBCHK(e->wb_iv_nbar.ensure(sizeof(double) * (size_t)iv.C));
    FBCHK(e->wb_iv_npart.ensure(sizeof(double) * (size_t)fb_wb_iv_uchunks(iv) * iv.C));
    if (!e->wb_iv_fail.p) FBCHK(e->wb_iv_fail.ensure(sizeof(int)));
    const size_t had = e->wb_iv_A.cap;
    FBCHK(e->wb_iv_A.ensure(sizeof(double) * (2 * (size_t)iv.R + 64)));
    if (e->wb_iv_A.cap != had || e->wb_iv_A_R != iv.R) {
      HIPCHK(hipMemsetAsync(e->wb_iv_A.p, 0, e->wb_iv_A.cap, e->stream));
      e->wb_iv_A_R = iv.R;
    }
  } else if (need_gmm && e->kind == 2) {
    FBCHK(e->wb_w.ensure(sizeof(double) * (size_t)e->iv.S));
    FBCHK(wb_xv_ensure(e, nes_replicas(e), (size_t)nes_replicas(e) * (size_t)T, T));
  } else if (need_gmm) {
    const FbGmmDev &g = e->gmm;
    if (!e->wb_uploaded) {
      FBCHK(e->wb_gc.ensure(sizeof(float) * e->h_wb_gc.size()));
      FBCHK(e->wb_miv.ensure(sizeof(float) * e->h_wb_miv.size()));
      FBCHK(e->wb_iv.ensure(sizeof(float) * e->h_wb_iv.size()));
      FBCHK(sync_stream(e));
      HIPCHK(hipMemcpy(e->wb_gc.p, e->h_wb_gc.data(), sizeof(float) * e->h_wb_gc.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->wb_miv.p, e->h_wb_miv.data(), sizeof(float) * e->h_wb_miv.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->wb_iv.p, e->h_wb_iv.data(), sizeof(float) * e->h_wb_iv.size(), hipMemcpyHostToDevice));
      e->wb_uploaded = true;
    }
    FBCHK(e->wb_w.ensure(sizeof(double) * (size_t)g.M));
    FBCHK(e->wb_part.ensure(sizeof(float) * (size_t)g.M * T * g.D));
  }
  FBCHK(e->wb_g.ensure(sizeof(double) * (size_t)T * fe.dim));
  FBCHK(e->wb_rank.ensure(sizeof(int) * (size_t)T));
  FBCHK(e->wb_dcm.ensure(sizeof(double) * (size_t)T * fe.dim));
  FBCHK(e->wb_ddf.ensure(sizeof(double) * (size_t)T * fe.dim));
  FBCHK(e->wb_dmf.ensure(sizeof(double) * (size_t)T * fe.nc));
  FBCHK(e->wb_dxf.ensure(sizeof(double) * (size_t)T * fe.L));
  FBCHK(e->grad.ensure(sizeof(double) * (size_t)N));
  // (the replicas of the one row: the EOT draws, times the utterances of a universal perturbation -- wb_check: only under
  //  fb_set_wb_universal)
  const size_t R = (size_t)nes_replicas(e);
  // (a play offset takes the universal route at K = 1 too; its chain transpose reads the composed rows from e->wav_play)
  const bool play = e->play_S > 0, uni = e->comp_K1 > 0 || play;
  if (e->wb_bpda || (uni && e->tf.n > 0)) FBCHK(e->wb_gj.ensure(sizeof(double) * (size_t)N));
  if (e->wb_air && e->air.L > 0) {  // the R replicas' cotangents are kept for the one k_air_conv_t launch behind the loop
    FBCHK(e->wb_air_cot.ensure(sizeof(double) * R * (size_t)N));
    if (R > 1 || play) FBCHK(e->wb_air_dx.ensure(sizeof(double) * R * (size_t)N));
  } else if (uni) {                 // ... and without a channel for k_wb_compose_t / k_wb_play_compose_t
    FBCHK(e->wb_uni_cot.ensure(sizeof(double) * R * (size_t)N));
    if (e->tf.n > 0 && !play) FBCHK(e->wb_uni_rows.ensure(sizeof(int16_t) * (size_t)(e->comp_K1 + 1) * (size_t)N));
  }
  if (e->wb_frontend && e->feco_iters > 0) {  // the R replicas' kept assignments, and one replica's cotangent on its voiced rows
    FBCHK(e->wb_feco_label.ensure(sizeof(int) * R * (size_t)T));
    FBCHK(e->wb_feco_cnt.ensure(sizeof(int) * R * (size_t)T));
    FBCHK(e->wb_feco_k.ensure(sizeof(int) * R));
    FBCHK(e->wb_xbar.ensure(sizeof(double) * (size_t)T * fe.dim));
  }
  if (!e->wb_status.p) FBCHK(e->wb_status.ensure(sizeof(int)));
  HIPCHK(hipMemsetAsync(e->wb_status.p, 0, sizeof(int), e->stream));
  return FB_OK;
}

// the GMM backward on the n rows (*n_rows_ptr <= T) of e->feats with the weights in e->wb_w: the cotangent lands in e->wb_g
// row_base_ptr (nullable): the first of the rows, when they are a replica's within the batch
static void wb_launch_gmm_backward(fb_engine *e, const int *n_rows_ptr, int T, const int *stop, const int *row_base_ptr = nullptr) {
  const FbGmmDev &g = e->gmm;
  fb_launch_wb_gmm_backward(e->stream, g.M, g.C, g.D, e->wb_gc.as<float>(), e->wb_miv.as<float>(), e->wb_iv.as<float>(),
                            e->feats.as<float>(), n_rows_ptr, T, e->wb_w.as<double>(), e->wb_part.as<float>(), e->wb_g.as<double>(),
                            stop, row_base_ptr);
}
// the i-vector back end's backward (fb_set_wb_ivector), in two parts.  First wbar = d (sum_s w_s LLR_s) / d ivec from the weights
// in e->wb_w at the i-vector `ivec` (device, [R]) ...
static void wb_launch_iv_backend_t(fb_engine *e, const double *ivec, const int *stop) {
  fb_launch_wb_iv_backend_t(e->stream, e->iv, ivec, e->wb_w.as<double>(), e->wb_iv_wbar.as<double>(), stop);
  e->wb_route[FB_WB_ROUTE_IV_BACKEND_T] += 1;
}
// ... then, from the cotangent e->wb_iv_wbar on the i-vector of row 0 of the batch the forward just scored (sel / post / the
// active list / the i-vector as it left them, quad in e->wb_iv_quad): the adjoint solve lambda = quad^-1 wbar -- the forward's
// own k_iv_solve_ll on the copy of the matrix, one right-hand side, no prior offset, no tail --, the parameter stream, and the
// per-frame transpose.  The cotangent on the *n_rows_ptr (<= T) voiced rows lands in e->wb_g.
// j, row_base_ptr (fb_set_wb_universal; 0 and null: the one row): replica j of the batch -- ITS copy of quad, ITS i-vector, and ITS
// rows of feats / sel / post from *row_base_ptr on.  k_iv_solve_ll leaves the zero padding of e->wb_iv_A as it found it, so the
// replicas' solves follow one another on the one workspace; a solve that fails sets the sticky e->wb_iv_fail, but the matrix is
// the one the forward factorised, and the forward's own flag (e->iv_fail, every row of the batch) is the one the calls read.
static void wb_launch_iv_backward(fb_engine *e, const int *n_rows_ptr, int T, const int *stop, int j = 0, const int *row_base_ptr = nullptr) {
  FbIvDev iv0 = e->iv;
  double *quad = e->wb_iv_quad.as<double>() + (size_t)j * (size_t)e->iv.triR;
  const double *ivec = e->iv_ivec.as<double>() + (size_t)j * (size_t)e->iv.R;
  iv0.prior_offset = 0.0;   // (the solve adds it to element 0 of the right-hand side and takes it off the solution: lin's, not wbar's)
  const FbIvTail none = {};
  fb_launch_iv_solve_ll(e->stream, iv0, quad, e->wb_iv_wbar.as<double>(), 1, 1, e->wb_iv_A.as<double>(),
                        e->wb_iv_linv.as<double>(), e->wb_iv_lam.as<double>(), e->wb_iv_fail.as<int>(), none);
  e->wb_route[FB_WB_ROUTE_IV_SOLVE] += 1;
  // (the active list is the batch's: a superset of every replica's own -- the components none of its frames kept get an Fbar /
  //  Nbar that k_wb_iv_post_t never reads)
  fb_launch_wb_iv_stats_t(e->stream, e->iv, e->iv_active.as<int>(), e->wb_iv_lam.as<double>(), ivec,
                          e->wb_iv_fbar.as<double>(), e->wb_iv_npart.as<double>(), e->wb_iv_nbar.as<double>(), stop);
  e->wb_route[FB_WB_ROUTE_IV_STATS_T] += 1;
  fb_launch_wb_iv_post_t(e->stream, e->iv, e->feats.as<float>(), n_rows_ptr, T, e->iv_sel.as<int>(), e->iv_post.as<float>(),
                         e->wb_iv_fbar.as<double>(), e->wb_iv_nbar.as<double>(), e->wb_g.as<double>(), stop, row_base_ptr);
  e->wb_route[FB_WB_ROUTE_IV_POST_T] += 1;
}
// the front-end backward of row j of the batch the front end read (`wav`: rows of N samples, T frames each, their MFCC
// matrices in e->mfcc): out = scale * the cotangent on that row's int16 samples.  cot (null: e->wb_g): the cotangent on the
// row's voiced rows; dk (nullable): the forward's dither key with the row's utterance index (fb_set_wb_frontend)
static void wb_launch_frontend_vjp(fb_engine *e, const int16_t *wav, int j, int64_t N, int T, double scale, double *out, const int *stop,
                                   const double *cot = nullptr, const FbDitherKey *dk = nullptr) {
  fb_launch_wb_frontend_vjp(e->stream, e->fe, wav + (size_t)j * (size_t)N, N, T, e->mfcc.as<float>() + (size_t)j * T * e->fe.nc,
                            cot ? cot : e->wb_g.as<double>(), e->tv.as<int>() + j, e->wb_rank.as<int>(), e->wb_dcm.as<double>(),
                            e->wb_ddf.as<double>(), e->wb_dmf.as<double>(), e->wb_dxf.as<double>(), scale, out, e->wb_status.as<int>(),
                            stop, dk);
}
// feature compression transposed for replica j of the batch the forward just scored (fb_set_wb_frontend): the cotangent on its
// k_j centres in e->wb_g goes back to its voiced rows in e->wb_xbar under the assignment the forward kept.  After the swap in
// feature_compress e->row_off holds the centres' offsets and e->row_off_fc the voiced rows'.
static void wb_launch_feco_t(fb_engine *e, int j, int T, const int *stop) {
  fb_launch_wb_feco_t(e->stream, e->fe.dim, e->wb_feco_label.as<int>(), e->wb_feco_cnt.as<int>(), e->row_off_fc.as<int>(),
                      e->row_off.as<int>(), j, 1, T, false, e->wb_g.as<double>(), e->wb_xbar.as<double>(), stop);
  e->wb_feco_launches += 1;
}
// the chain's transpose for replica j at the call's point: grad (+)= the vector-Jacobian product of cot through the chain
// applied to the un-replicated row in e->wav (k_tf_power's sum of the forward is still in e->tf_power).  With an air channel
// the chain read replica j's row of e->wav_air -- intact: a codec behind a chain runs in place on wav_tf -- and k_tf_power
// summed the channel's output rows, so the row's sum is tf_power[j]; the noise counters are (utterance row 0, replica j)
// either way (FbTfRnd::pre = r in the forward).
// With companions (fb_set_wb_universal) j is rho = u * eot + j': without a channel the chain read utterance u's COMPOSED row,
// which wb_enqueue wrote to e->wb_uni_rows (the forward had it in LDS only), and its SNR power is tf_power[0 * K + u], as the
// forward indexed it; the noise counters are (utterance row 0, replica rho) there as well.
// play: the forward of THIS call composed under a play offset (FbScoreCall::play > 0; a hook whose forward ignores the setting
// passes false whatever the engine holds).  Without a channel the chain then read replica j's row of e->wav_play, composed under
// ITS offset, and k_tf_power, the plain form, summed those rows: tf_power[j], as under a channel.
static int wb_launch_chain_t(fb_engine *e, const FbRngPoint &pt, int j, int64_t N, const double *cot, double *grad, bool accumulate,
                             const int *stop, bool play) {
  const bool air = e->air.L > 0;
  const int u = e->comp_K1 > 0 ? j / e->eot : 0;
  FbTfRnd rn = fb_tf_rnd(pt, e->eot);
  rn.power = tf_noise_stages(e->tf, true) > 0 ? e->tf_power.as<unsigned long long>() + (air || play ? j : u) : nullptr;
  const int16_t *row = air ? e->wav_air.as<int16_t>() + (size_t)j * (size_t)N
                       : play ? e->wav_play.as<int16_t>() + (size_t)j * (size_t)N
                       : e->comp_K1 > 0 ? e->wb_uni_rows.as<int16_t>() + (size_t)u * (size_t)N : e->wav.as<int16_t>();
  if (!fb_launch_wb_chain_t(e->stream, e->tf, e->tf_taps.as<double>(), row, N, rn, j, cot, grad, accumulate ? 1 : 0, stop))
    return fb_fail(FB_E_HIP, "k_wb_chain_t: %zu bytes of LDS were refused", fb_wb_chain_t_lds_bytes(e->tf));
  e->wb_route[FB_WB_ROUTE_CHAIN_T] += 1;
  return FB_OK;
}
// the composition transposed (fb_set_wb_universal), ONE launch: the R = K * eot cotangents cot [R][N] on the composed rows, the
// un-replicated q still in e->wav, a_0 and the companions give out [N], rho ascending
// play (the forward of this call composed under a play offset): k_wb_play_compose_t takes its place, at K = 1 too: the offsets
// are the forward's, still in e->play_tau.
static void wb_launch_compose_t(fb_engine *e, const double *cot, int64_t N, double *out, const int *stop, bool play) {
  if (play) {
    fb_launch_wb_play_compose_t(e->stream, cot, e->wav.as<int16_t>(), e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>(),
                                e->play_tau.as<uint32_t>(), e->comp_K1 + 1, e->eot, N, out, stop);
    e->wb_play_launches += 1;
    return;
  }
  fb_launch_wb_compose_t(e->stream, cot, e->wav.as<int16_t>(), e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>(), e->comp_K1 + 1, e->eot,
                         N, out, stop);
  e->wb_universal_launches += 1;
}
// the channel's transpose for all r replicas of the one row (fb_set_wb_air), ONE launch: the cotangents e->wb_air_cot [r][N] on
// the channel's output, the forward's saturation bytes and the forward's own responses in e->air_taps -- nothing is redrawn --
// give dx[r][N]; out (device, [N]) = their sum, j ascending (r = 1: k_air_conv_t writes out itself)
// play: as in wb_launch_chain_t (k_wb_play_compose_t reads dx at rotated indices: never in place)
static void wb_launch_air_t(fb_engine *e, int r, int64_t N, double *out, const int *stop, bool play) {
  double *dx = r > 1 || play ? e->wb_air_dx.as<double>() : out;
  fb_launch_air_conv_t(e->stream, e->wb_air_cot.as<double>(), e->wb_air_sat.as<unsigned char>(), r, N, e->air_taps.as<int16_t>(), e->air.L,
                       dx, stop);
  e->wb_air_launches += 1;
  if (e->comp_K1 > 0 || play) wb_launch_compose_t(e, dx, N, out, stop, play);  // (r = K * eot: dx_rho is the cotangent on utterance u(rho)'s composed row)
  else if (r > 1) fb_launch_air_sum_t(e->stream, dx, r, N, out, stop);
}

// One white-box iteration on the device-resident adver, asynchronous: the forward of fb_get_grad on ONE row -- the cast
// (k_perturb without noise), the scoring chain, k_loss --, then the weights (and, with ctl, the loop control), the GMM
// backward and the front-end backward.  q: the call's parameters with samples_per_draw = 0.
// With fb_set_wb_bpda on and a defence or EOT replicas set: the forward scores the r replicas of the row (k_loss_eot when
// r > 1), and behind it the replicas follow one by one -- weights of replica j, GMM backward on its voiced rows, front-end
// backward on the row ITS front end read, the chain's transpose, which also adds replica j to e->grad (j ascending).
// With fb_set_wb_ivector on and an i-vector system loaded (r = 1: wb_check): the same forward with a copy of quad kept, then
// k_wb_iv_ctl and the i-vector back end's backward (wb_launch_iv_backend_t, wb_launch_iv_backward) in the GMM backward's place.
// With fb_set_wb_air on and an air channel set: the forward keeps the channel's saturation bytes; replica j's cotangent on the
// channel's output -- the front-end backward's, or behind a chain the chain transpose's, non-accumulating -- goes to slot j of
// e->wb_air_cot, and behind the loop one k_air_conv_t launch over all r replicas and their ascending sum write e->grad.
// With fb_set_wb_frontend on: under feature compression the forward keeps every replica's final labels, counts and k; the back
// end's backward runs on replica j's k_j centres and k_wb_feco_t takes its cotangent back to the voiced rows (e->wb_xbar), which
// the front-end backward then reads; under dither the front-end backward gets the forward's key with utterance index j.
// With fb_set_wb_universal on and companions set: the forward scores the R = K * eot replicas of the composed utterances; replica
// rho's cotangent on ITS composed row goes to slot rho (of e->wb_uni_cot, or under a channel of e->wb_air_cot), a chain's
// transpose reading the composed row from e->wb_uni_rows; behind the loop ONE k_wb_compose_t launch masks the companions' clipped
// samples and sums the slots, rho ascending, into e->grad.  On an i-vector system the forward then keeps quad of all R rows and
// replica rho takes its own copy, i-vector and rows (k_wb_iv_ctl_rep for its weights) -- which is also what lets fb_set_eot(r > 1)
// run there without companions.
// With fb_set_wb_xvector on and an x-vector system loaded: the forward also keeps every layer's ReLU decisions (e->xv_mask); the
// loop becomes two -- per replica the weights and k_wb_iv_backend_t at ITS embedding, into slot j of e->wb_xv_ebar; then ONE TDNN
// backward over all rows of the batch (wb_xv_backward); then per replica, as for the other kinds, the front-end backward on ITS
// slice of e->wb_xv_g, the chain's transpose and the ascending sum.
static int wb_enqueue(fb_engine *e, const fb_nes_params *q, int64_t N, uint32_t it, bool with_dist, FbCtlDev *ctl, double *trace_dev) {
  const int *stop = ctl ? &ctl->stop : nullptr;
  // the replicas of the one row: the EOT draws, and under fb_set_wb_universal rho = u * eot + j over the K composed utterances
  // (with a play offset the call takes the universal, replicated route whatever K and r are)
  const int K = e->comp_K1 + 1, r = K * e->eot;
  const bool play = e->play_S > 0, uni = K > 1 || play, rep = r > 1 || play;
  int ndp = 0;
  fb_launch_perturb(e->stream, e->adver.as<double>(), with_dist ? e->audio.as<double>() : nullptr, N, 0, q->sigma, q->seed, it,
                    q->stream, nullptr, e->wav.as<int16_t>(), e->dist_part.as<double>(), &ndp, nullptr, stop, nes_bits(q));
  e->pre_iter = -1;
  const FbRngPoint pt{q->seed, q->stream, it, 0};
  FbScoreCall call{pt};
  call.eot = e->eot;
  call.K = K;
  call.play = e->play_S;
  call.stop = stop;
  call.keep_iv_quad = e->kind == 1;
  call.keep_iv_quad_rows = e->wb_universal ? r : 1;  // (r > 1 on an i-vector system: wb_check, only under fb_set_wb_universal)
  const bool xvk = e->kind == 2;  // (wb_check: only under fb_set_wb_xvector; no channel, dither, companions or play offset then)
  call.keep_xv_mask = xvk;
  const bool air = e->air.L > 0;  // (wb_check: only under fb_set_wb_air)
  call.keep_air_sat = air;
  const bool feco = e->feco_iters > 0;  // (wb_check: only under fb_set_wb_frontend, like a dither > 0)
  call.keep_feco = feco;
  const int T = e->h_frame_off[1];
  FBCHK(run_scoring(e, call, r, e->h_frame_off[r]));
  const double scale = ldexp(1.0, nes_bits(q) - 1);
  if (rep) {
    fb_launch_loss_eot(e->stream, e->raw.as<double>(), e->tv.as<int>(), 1, r, e->n_out, q->task, e->kind, q->attack_type,
                       e->zmean.as<double>(), e->zstd.as<double>(), q->threshold, q->adver_thresh, q->target, q->true_label,
                       e->dist_part.as<double>(), with_dist ? ndp : 0, e->eot_sc.as<double>(), e->eot_l.as<double>(),
                       e->scores.as<double>(), e->loss.as<double>(), e->nes_out.as<FbNesDev>(), nullptr, nullptr, 0);
  } else {
    fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), 1, e->n_out, q->task, e->kind, q->attack_type,
                   e->zmean.as<double>(), e->zstd.as<double>(), q->threshold, q->adver_thresh, q->target, q->true_label,
                   e->dist_part.as<double>(), with_dist ? ndp : 0, e->scores.as<double>(), e->loss.as<double>(),
                   e->nes_out.as<FbNesDev>());
  }
  e->nes_route[FB_NES_ROUTE_K_LOSS] += 1;
  // (a codec alone is the identity: the front-end backward writes e->grad -- or, with a channel, its slot of e->wb_air_cot,
  //  where the replicas are summed behind the channel's transpose and an empty chain has nothing to add)
  // (a universal perturbation: every replica's cotangent on ITS composed row goes to slot rho -- of e->wb_air_cot under a
  //  channel, of e->wb_uni_cot without -- and k_wb_compose_t behind the loop masks and sums them, so an empty chain adds nothing
  //  here either; a chain without a channel read utterance u's composed row, which existed in the forward's LDS only: the K
  //  rows are written once per iteration.  At K = 1 none of this is queued.)
  const bool through_chain = e->tf.n > 0 || (r > 1 && !air && !uni);
  if (uni && e->tf.n > 0 && !air && !play)
    fb_launch_wb_compose_rows(e->stream, e->wav.as<int16_t>(), e->comp_a0.as<int16_t>(), e->comp_wav.as<int16_t>(), K, N,
                              e->wb_uni_rows.as<int16_t>(), stop);
  const int S = fb_num_speakers(e);
  // An x-vector system: first every replica's weights and the back end's transpose at ITS embedding, into slot j of e->wb_xv_ebar;
  // then ONE TDNN backward over all rows of the batch, as the forward ran; the loop below then takes replica j's slice of the
  // cotangent on the feature rows through the front end and the chain.
  if (xvk) {
    for (int j = 0; j < r; ++j) {
      if (rep) {
        fb_launch_wb_iv_ctl_rep(e->stream, e->eot_sc.as<double>() + (size_t)j * S, e->scores.as<double>(), e->nes_out.as<FbNesDev>(), S, r,
                                q->task, q->attack_type, e->zstd.as<double>(), q->threshold, q->target, q->true_label,
                                e->wb_w.as<double>(), ctl, j == 0 ? 1 : 0, trace_dev, (int)it);
        e->wb_route[FB_WB_ROUTE_CTL_REP] += 1;
      } else {
        fb_launch_wb_iv_ctl(e->stream, e->scores.as<double>(), e->nes_out.as<FbNesDev>(), S, q->task, q->attack_type,
                            e->zstd.as<double>(), q->threshold, q->target, q->true_label, e->wb_w.as<double>(), ctl, trace_dev, (int)it);
        e->wb_route[FB_WB_ROUTE_IV_CTL] += 1;
      }
      fb_launch_wb_iv_backend_t(e->stream, e->iv, e->iv_ivec.as<double>() + (size_t)j * (size_t)e->iv.R, e->wb_w.as<double>(),
                                e->wb_xv_ebar.as<double>() + (size_t)j * (size_t)e->iv.R, stop);
      e->wb_xv_route[FB_WB_XV_ROUTE_BACKEND_T] += 1;
    }
    wb_xv_backward(e, r, e->h_frame_off[r], 0, T, stop, nullptr);
  }
  for (int j = 0; j < r; ++j) {
    if (xvk) {
      // (an x-vector system's weights were formed above, replica by replica)
    } else if (rep && e->kind == 1) {
      fb_launch_wb_iv_ctl_rep(e->stream, e->eot_sc.as<double>() + (size_t)j * S, e->scores.as<double>(), e->nes_out.as<FbNesDev>(), S, r,
                              q->task, q->attack_type, e->zstd.as<double>(), q->threshold, q->target, q->true_label,
                              e->wb_w.as<double>(), ctl, j == 0 ? 1 : 0, trace_dev, (int)it);
      e->wb_route[FB_WB_ROUTE_CTL_REP] += 1;
    } else if (rep) {
      fb_launch_wb_ctl_rep(e->stream, e->eot_sc.as<double>() + (size_t)j * S, e->scores.as<double>(), e->nes_out.as<FbNesDev>(),
                           e->gmm.M, r, q->task, q->attack_type, e->zstd.as<double>(), q->threshold, q->target, q->true_label,
                           e->wb_w.as<double>(), ctl, j == 0 ? 1 : 0, trace_dev, (int)it);
      e->wb_route[FB_WB_ROUTE_CTL_REP] += 1;
    } else if (e->kind == 1) {
      fb_launch_wb_iv_ctl(e->stream, e->scores.as<double>(), e->nes_out.as<FbNesDev>(), S, q->task, q->attack_type,
                          e->zstd.as<double>(), q->threshold, q->target, q->true_label, e->wb_w.as<double>(), ctl, trace_dev, (int)it);
      e->wb_route[FB_WB_ROUTE_IV_CTL] += 1;
    } else {
      fb_launch_wb_ctl(e->stream, e->scores.as<double>(), e->nes_out.as<FbNesDev>(), e->gmm.M, q->task, q->attack_type,
                       e->zstd.as<double>(), q->threshold, q->target, q->true_label, e->wb_w.as<double>(), ctl, trace_dev, (int)it);
      e->wb_route[FB_WB_ROUTE_CTL] += 1;
    }
    // (row_off[0] = 0 and tv[0] = row_off[1]: replica 0 of an unreplicated batch is what the launch always took)
    if (xvk) {
      // (the one TDNN backward above left replica j's cotangent in its slice of e->wb_xv_g)
    } else if (e->kind == 1 && rep) {  // replica j's own i-vector, quad, rows (under feature compression its k_j centres)
      wb_launch_iv_backend_t(e, e->iv_ivec.as<double>() + (size_t)j * (size_t)e->iv.R, stop);
      wb_launch_iv_backward(e, feco ? e->wb_feco_k.as<int>() + j : e->tv.as<int>() + j, T, stop, j, e->row_off.as<int>() + j);
    } else if (e->kind == 1) {
      wb_launch_iv_backend_t(e, e->iv_ivec.as<double>(), stop);
      wb_launch_iv_backward(e, e->row_off.as<int>() + 1, T, stop);
    } else {
      // (under feature compression the rows scored are replica j's k_j centres -- the kept k, not the VAD's count e->tv[j],
      //  which the front-end backward still checks its mask against; e->feats / e->row_off are the compressed pair)
      const int *n_rows = feco ? e->wb_feco_k.as<int>() + j : rep ? e->tv.as<int>() + j : e->row_off.as<int>() + 1;
      wb_launch_gmm_backward(e, n_rows, T, stop, rep ? e->row_off.as<int>() + j : nullptr);
    }
    if (feco) wb_launch_feco_t(e, j, T, stop);
    // replica j's cotangent on the channel's output, or (a universal perturbation without a channel) on its composed row
    double *slot = air ? e->wb_air_cot.as<double>() + (size_t)j * (size_t)N
                       : uni ? e->wb_uni_cot.as<double>() + (size_t)j * (size_t)N : nullptr;
    double *fe_out = through_chain ? e->wb_gj.as<double>() : slot ? slot : e->grad.as<double>();
    FbRngPoint ptj = pt;
    ptj.utt0 = pt.utt0 + (uint32_t)j;   // the forward's dither draws of replicated row j
    const FbDitherKey dith = fb_dither_key(ptj, e->cfg.dither);
    wb_launch_frontend_vjp(e, e->fe_wav, j, N, T, scale, fe_out, stop,
                           xvk ? e->wb_xv_g.as<double>() + (size_t)j * (size_t)T * (size_t)e->fe.dim : feco ? e->wb_xbar.as<double>() : nullptr,
                           e->cfg.dither > 0.0 ? &dith : nullptr);
    e->wb_route[FB_WB_ROUTE_BACKWARD] += 1;
    if (through_chain) FBCHK(wb_launch_chain_t(e, pt, j, N, e->wb_gj.as<double>(), slot ? slot : e->grad.as<double>(), !slot && j > 0, stop, play));
  }
  if (air) wb_launch_air_t(e, r, N, e->grad.as<double>(), stop, play);
  else if (uni) wb_launch_compose_t(e, e->wb_uni_cot.as<double>(), N, e->grad.as<double>(), stop, play);
  return FB_OK;
}

// the start of every white-box entry point, before its arguments are looked at: the route counters of the call start at zero
static void wb_call_begin(fb_engine *e) {
  if (!e) return;
  e->bench_it = e->nes_rec.iter = -1;
  memset(e->nes_route, 0, sizeof(e->nes_route));
  memset(e->wb_route, 0, sizeof(e->wb_route));
  memset(e->wb_xv_route, 0, sizeof(e->wb_xv_route));
  e->wb_air_launches = 0;
  e->wb_feco_launches = 0;
  e->wb_universal_launches = 0;
  e->wb_play_launches = 0;
}

static int wb_status_check(fb_engine *e, int status) {
  if (status != 0) return fb_fail(FB_E_HIP, "white-box gradients: the voiced mask recomputed by the backward is not the forward's");
  return FB_OK;
}
// The host's look at an attack's control block behind a batch of queued iterations: the block to e->h_ctl, the backward's
// status word and, where the attack keeps one, its own block (extra <- extra_dev), then the wait and what the three say.  The
// caller reads e->h_ctl->stop.
static int wb_look(fb_engine *e, void *extra, const void *extra_dev, size_t extra_bytes) {
  int status = 0, rc = FB_OK;
  const hipError_t he = hipMemcpyAsync(e->h_ctl, e->ctl.p, sizeof(FbCtlDev), hipMemcpyDeviceToHost, e->stream);
  if (he == hipSuccess) rc = d2h(e, &status, e->wb_status.p, sizeof(int));
  if (he == hipSuccess && rc == FB_OK && extra) rc = d2h(e, extra, extra_dev, extra_bytes);
  if (he != hipSuccess || rc != FB_OK) {
    (void)sync_stream(e);
    HIPCHK(he);
    return rc;
  }
  FBCHK(sync_stream(e));
  if (e->gmm_pending) FBCHK(time_collect(e));
  FBCHK(wb_status_check(e, status));
  if (e->h_ctl->err != 0) return fb_fail(FB_E_NO_VOICED, "the adversarial audio has no voiced frames");
  return FB_OK;
}

// mirrors FakeBob.get_grad + loss_fn (FAKEBOB.py:223-299) with the analytic gradient in place of the NES estimate
// original (nullable: audio itself): the audio whose int16 cast is a_0 of the composition (fb_set_wb_universal)
extern "C" int fb_get_grad_wb_from(fb_engine *e, const fb_nes_params *p, const double *audio, const double *original, int64_t N,
                                   int iter, double *adver_loss, double *grad, double *score0) {
  wb_call_begin(e);
  if (iter < 0) return fb_fail(FB_E_ARG, "iter must be >= 0");
  fb_nes_params q;
  FBCHK(wb_check(e, p, audio, N, &q));
  HIPCHK(hipSetDevice(e->device));
  FBCHK(prepare_nes_replicas(e, N, 1));
  FBCHK(ensure_nes_buffers(e, N, 1));
  FBCHK(wb_prepare(e, N, e->h_frame_off[1], true));
  FBCHK(h2d(e, e->adver.p, audio, sizeof(double) * (size_t)N));
  if (e->comp_K1 > 0 || e->play_S > 0) {  // a_0: cast once per call, by the batch's cast rule
    if (original) FBCHK(h2d(e, e->audio.p, original, sizeof(double) * (size_t)N));
    cast_a0(e, &q, original ? e->audio.as<double>() : e->adver.as<double>(), N);
  }
  FBCHK(wb_enqueue(e, &q, N, (uint32_t)iter, false, nullptr, nullptr));
  int status = 0;
  if (grad) FBCHK(d2h(e, grad, e->grad.p, sizeof(double) * (size_t)N));
  FBCHK(d2h(e, &status, e->wb_status.p, sizeof(int)));
  int iv_fail = 0;
  if (e->kind == 1) FBCHK(d2h(e, &iv_fail, e->iv_fail.p, sizeof(int)));
  FBCHK(fetch_out(e, true));
  HIPCHK(hipGetLastError());
  if (iv_fail) return fb_fail(FB_E_ARG, "i-vector system of utterance %d is not positive definite", iv_fail - 1);
  FBCHK(wb_status_check(e, status));
  e->nes_iters += 1;
  if (adver_loss) *adver_loss = e->h_out->adver_loss;
  if (score0) for (int s = 0; s < fb_num_speakers(e); ++s) score0[s] = e->h_out->score0[s];
  return FB_OK;
}
extern "C" int fb_get_grad_wb_iter(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, int iter,
                                   double *adver_loss, double *grad, double *score0) {
  return fb_get_grad_wb_from(e, p, audio, nullptr, N, iter, adver_loss, grad, score0);
}
extern "C" int fb_get_grad_wb(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, double *adver_loss,
                              double *grad, double *score0) {
  return fb_get_grad_wb_iter(e, p, audio, N, 0, adver_loss, grad, score0);
}

extern "C" int fb_set_wb_xvector(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_xvector takes 0 or 1, not %d", on);
  e->wb_xvector = on;
  return FB_OK;
}

extern "C" int fb_debug_wb_xv_route(fb_engine *e, int *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  for (int i = 0; i < FB_WB_XV_ROUTE_N; ++i) info[i] = e->wb_xv_route[i];
  return FB_OK;
}

// Test hook: the x-vector chain on rows handed in with every layer's masks kept, as fb_debug_xv_embed runs it, then the TDNN
// backward from the cotangents ebar [B][R] on the embeddings down to `stage` (fakebob_hip_test.h)
extern "C" int fb_debug_xv_backward(fb_engine *e, const float *feats, const int *row_off, int B, const double *ebar, int stage, void *out,
                                    int64_t cap) {
  if (!e || !feats || !row_off || !ebar || !out || B <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 2) return fb_fail(FB_E_STATE, "load an x-vector system first");
  const FbXvDev &xv = e->xv;
  if (stage < 0 || stage > xv.n_layers + 1) return fb_fail(FB_E_ARG, "stage %d outside 0 .. %d", stage, xv.n_layers + 1);
  if (row_off[0] != 0) return fb_fail(FB_E_ARG, "row_off[0] must be 0");
  int cap64 = 1;
  for (int b = 0; b < B; ++b) {
    if (row_off[b + 1] < row_off[b]) return fb_fail(FB_E_ARG, "row_off must not descend");
    cap64 = std::max(cap64, row_off[b + 1] - row_off[b]);
  }
  const int rows = row_off[B];
  if (rows <= 0) return fb_fail(FB_E_ARG, "no rows");
  // (stage n_layers: the last layer's OUTPUT, P wide; below it the INPUT of layer `stage`)
  const size_t want = stage > xv.n_layers    ? sizeof(double) * (size_t)B * 2 * xv.P
                      : stage == xv.n_layers ? sizeof(float) * (size_t)rows * (size_t)xv.P
                      : stage == 0           ? sizeof(double) * (size_t)rows * xv.D
                                             : sizeof(float) * (size_t)rows * (size_t)xv.layer[stage].din;
  if (cap < (int64_t)want) return fb_fail(FB_E_ARG, "out holds %lld bytes, stage %d needs %lld", (long long)cap, stage, (long long)want);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  e->bench_it = e->nes_rec.iter = -1;
  memset(e->wb_xv_route, 0, sizeof(e->wb_xv_route));
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)rows * xv.D));
  FBCHK(e->row_off.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(wb_xv_ensure(e, B, (size_t)rows, cap64));
  FBCHK(h2d(e, e->feats.p, feats, sizeof(float) * (size_t)rows * xv.D));
  FBCHK(h2d(e, e->row_off.p, row_off, sizeof(int) * (size_t)(B + 1)));
  FBCHK(h2d(e, e->wb_xv_ebar.p, ebar, sizeof(double) * (size_t)B * xv.R));
  FBCHK(run_xvector(e, B, rows, xv.n_layers + 1, nullptr, true));
  const float *last32 = nullptr;
  wb_xv_backward(e, B, rows, stage, cap64, nullptr, &last32);
  HIPCHK(hipGetLastError());
  if (stage > xv.n_layers) {
    FBCHK(d2h(e, out, e->wb_xv_sbar.p, want));
  } else if (stage > 0) {
    FBCHK(d2h(e, out, last32, want));
  } else {
    for (int b = 0; b < B; ++b) {   // utterance b's rows from its slot of cap64 rows
      const size_t n = sizeof(double) * (size_t)(row_off[b + 1] - row_off[b]) * xv.D;
      FBCHK(d2h(e, (char *)out + sizeof(double) * (size_t)row_off[b] * xv.D, e->wb_xv_g.as<double>() + (size_t)b * cap64 * xv.D, n));
    }
  }
  return sync_stream(e);
}

// Benchmark hook (tools/xvector_wb_rate.py): every launch of the TDNN backward on rows handed in, `reps` times between device
// events after one launch to warm up, each on the inputs the whole backward left it
extern "C" int fb_bench_xv_backward(fb_engine *e, const float *feats, const int *row_off, int B, int reps, double *ms_act, double *ms_affine,
                                    double *ms_unsplice, double *ms_tail) {
  if (!e || !feats || !row_off || !ms_act || !ms_affine || !ms_unsplice || !ms_tail || B <= 0 || reps <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 2) return fb_fail(FB_E_STATE, "load an x-vector system first");
  const FbXvDev &xv = e->xv;
  const int rows = row_off[B];
  if (row_off[0] != 0 || rows <= 0) return fb_fail(FB_E_ARG, "bad row_off");
  int cap64 = 1;
  for (int b = 0; b < B; ++b) {
    if (row_off[b + 1] < row_off[b]) return fb_fail(FB_E_ARG, "row_off must not descend");
    cap64 = std::max(cap64, row_off[b + 1] - row_off[b]);
  }
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  e->bench_it = e->nes_rec.iter = -1;
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)rows * xv.D));
  FBCHK(e->row_off.ensure(sizeof(int) * (size_t)(B + 1)));
  FBCHK(wb_xv_ensure(e, B, (size_t)rows, cap64));
  FBCHK(h2d(e, e->feats.p, feats, sizeof(float) * (size_t)rows * xv.D));
  FBCHK(h2d(e, e->row_off.p, row_off, sizeof(int) * (size_t)(B + 1)));
  {  // cotangents on the embeddings: a fixed pattern of unit scale
    std::vector<double> eb((size_t)B * xv.R);
    for (size_t i = 0; i < eb.size(); ++i) eb[i] = (double)((int)((i * 2654435761u) >> 20 & 2047) - 1024) / 1024.0;
    FBCHK(h2d(e, e->wb_xv_ebar.p, eb.data(), sizeof(double) * eb.size()));
  }
  FBCHK(run_xvector(e, B, rows, xv.n_layers + 1, nullptr, true));
  wb_xv_backward(e, B, rows, 0, cap64, nullptr, nullptr);   // every buffer sized; every layer's G and amax have been written once
  FBCHK(sync_stream(e));
  hipStream_t s = e->stream;
  hipEvent_t ev0, ev1;
  HIPCHK(hipEventCreate(&ev0));
  HIPCHK(hipEventCreate(&ev1));
  auto timed = [&](auto &&launch, double *ms) -> int {
    launch();
    HIPCHK(hipEventRecord(ev0, s));
    for (int i = 0; i < reps; ++i) launch();
    HIPCHK(hipEventRecord(ev1, s));
    HIPCHK(hipEventSynchronize(ev1));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, ev0, ev1));
    *ms = (double)t / reps;
    return FB_OK;
  };
  const int *ro = e->row_off.as<int>(), *n_rows = ro + B;
  const int2 *rowinfo = e->xv_rowinfo.as<int2>();
  int rc = timed([&] { fb_launch_wb_xv_segment_t(s, xv, e->wb_xv_ebar.as<double>(), B, e->wb_xv_sbar.as<double>(), nullptr); }, ms_tail + 0);
  int cur = 0;
  if (rc == FB_OK)
    rc = timed([&] { fb_launch_wb_xv_pool_t(s, e->xv_act[(xv.n_layers - 1) & 1].as<float>(), xv.P, ro, B, e->xv_stats.as<double>(),
                                            e->wb_xv_sbar.as<double>(), e->wb_xv_y[cur].as<float>(), nullptr); }, ms_tail + 1);
  for (int l = xv.n_layers - 1; l >= 0 && rc == FB_OK; --l) {
    const FbXvLayerDev &ly = xv.layer[l];
    rc = timed([&] { fb_launch_wb_xv_act_t(s, ly, e->wb_xv_y[cur].as<float>(), e->xv_mask[l].as<unsigned char>(), n_rows, rows,
                                           e->wb_xv_z.as<float>(), e->wb_xv_amax.as<float>(), nullptr); }, ms_act + l);
    if (rc == FB_OK)
      rc = timed([&] { fb_launch_wb_xv_affine_t(s, ly, e->wb_xv_z.as<float>(), e->wb_xv_amax.as<float>(), n_rows, rows, e->wb_xv_G.as<float>(), nullptr); },
                 ms_affine + l);
    if (rc == FB_OK)
      rc = timed([&] { fb_launch_wb_xv_unsplice(s, ly, e->wb_xv_G.as<float>(), rowinfo, ro, B, n_rows, rows, l > 0 ? e->wb_xv_y[cur ^ 1].as<float>() : nullptr,
                                                l > 0 ? nullptr : e->wb_xv_g.as<double>(), cap64, nullptr); }, ms_unsplice + l);
    cur ^= 1;
  }
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  return rc;
}

// Test hook: the ReLU decisions of layer `layer` for the batch scored last with its masks kept (a white-box call on an x-vector
// system, fb_debug_xv_backward): [rows][dout] bytes, size-then-fill
extern "C" int fb_debug_xv_masks(fb_engine *e, int layer, unsigned char *out, int64_t cap, int64_t *size) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm || e->kind != 2) return fb_fail(FB_E_STATE, "load an x-vector system first");
  if (layer < 0 || layer >= e->xv.n_layers) return fb_fail(FB_E_ARG, "layer %d outside 0 .. %d", layer, e->xv.n_layers - 1);
  if (e->xv_mask_B <= 0) return fb_fail(FB_E_STATE, "no batch has been scored with its masks kept");
  HIPCHK(hipSetDevice(e->device));
  int rows = 0;
  FBCHK(d2h(e, &rows, e->xv_mask_rows.p, sizeof(int)));
  FBCHK(sync_stream(e));
  const size_t n = (size_t)rows * (size_t)e->xv.layer[layer].dout;
  if (n > e->xv_mask[layer].cap) return fb_fail(FB_E_STATE, "the kept masks are smaller than the batch's rows");
  if (size) *size = (int64_t)n;
  if (!out) return FB_OK;
  if (cap < (int64_t)n) return fb_fail(FB_E_ARG, "out holds %lld bytes, the masks need %lld", (long long)cap, (long long)n);
  FBCHK(d2h(e, out, e->xv_mask[layer].p, n));
  return sync_stream(e);
}

extern "C" int fb_set_wb_universal(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_universal takes 0 or 1, not %d", on);
  e->wb_universal = on;
  return FB_OK;
}

extern "C" int fb_debug_wb_universal_route(fb_engine *e, int *n_launches) {
  if (!e || !n_launches) return fb_fail(FB_E_ARG, "null argument");
  *n_launches = e->wb_universal_launches;
  return FB_OK;
}

// Test hook: k_wb_compose_t alone, ONE launch, on arrays handed in: cot [K * eot][n], q / a0 [n], comp [K - 1][n] (K = 1: not read)
extern "C" int fb_debug_wb_compose_t(fb_engine *e, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp, int K,
                                     int eot, int64_t n, double *grad) {
  if (!e || !cot || !q || !a0 || !grad || K < 1 || eot < 1 || K * eot > 32 || n <= 0 || (K > 1 && !comp)) return fb_fail(FB_E_ARG, "bad argument");
  if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "row longer than 2^31 samples");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t R = (size_t)K * (size_t)eot, ns = (size_t)n;
  DevBuf d_cot, d_q, d_a0, d_comp, d_grad;
  FBCHK(d_cot.ensure(sizeof(double) * R * ns));
  FBCHK(d_q.ensure(sizeof(int16_t) * ns));
  FBCHK(d_a0.ensure(sizeof(int16_t) * ns));
  FBCHK(d_grad.ensure(sizeof(double) * ns));
  FBCHK(h2d(e, d_cot.p, cot, sizeof(double) * R * ns));
  FBCHK(h2d(e, d_q.p, q, sizeof(int16_t) * ns));
  FBCHK(h2d(e, d_a0.p, a0, sizeof(int16_t) * ns));
  if (K > 1) {
    FBCHK(d_comp.ensure(sizeof(int16_t) * (size_t)(K - 1) * ns));
    FBCHK(h2d(e, d_comp.p, comp, sizeof(int16_t) * (size_t)(K - 1) * ns));
  }
  e->wb_universal_launches = 0;
  fb_launch_wb_compose_t(e->stream, d_cot.as<double>(), d_q.as<int16_t>(), d_a0.as<int16_t>(), K > 1 ? d_comp.as<int16_t>() : nullptr, K, eot, n,
                         d_grad.as<double>(), nullptr);
  e->wb_universal_launches += 1;
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, grad, d_grad.p, sizeof(double) * ns));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_set_wb_bpda(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_bpda takes 0 or 1, not %d", on);
  e->wb_bpda = on;
  return FB_OK;
}

extern "C" int fb_set_wb_ivector(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_ivector takes 0 or 1, not %d", on);
  e->wb_ivector = on;
  return FB_OK;
}

extern "C" int fb_set_wb_air(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_air takes 0 or 1, not %d", on);
  e->wb_air = on;
  return FB_OK;
}

extern "C" int fb_set_wb_frontend(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (on != 0 && on != 1) return fb_fail(FB_E_ARG, "fb_set_wb_frontend takes 0 or 1, not %d", on);
  e->wb_frontend = on;
  return FB_OK;
}

extern "C" int fb_debug_wb_feco_route(fb_engine *e, int *n_launches) {
  if (!e || !n_launches) return fb_fail(FB_E_ARG, "null argument");
  *n_launches = e->wb_feco_launches;
  return FB_OK;
}

// Test hook: what the forward of the last fb_get_grad_wb* call kept of replica j's feature compression (valid until the next
// scoring call): *Tv voiced rows, *k centres, labels[Tv], counts[k]; cap = the ints each array holds
extern "C" int fb_debug_wb_feco_state(fb_engine *e, int j, int cap, int *labels, int *counts, int *Tv, int *k) {
  if (!e || !labels || !counts || !Tv || !k || cap < 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->wb_frontend || e->feco_iters <= 0 || !e->wb_feco_k.p || !e->row_off_fc.p)
    return fb_fail(FB_E_STATE, "no kept assignment: fb_set_wb_frontend, fb_set_feature_compression and a white-box call first");
  if (j < 0 || j >= nes_replicas(e)) return fb_fail(FB_E_ARG, "replica %d of %d", j, nes_replicas(e));   // (companions: rho of K * eot)
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  int in_off[2], out_off[2], kept = 0;
  FBCHK(d2h(e, in_off, e->row_off_fc.as<int>() + j, sizeof(in_off)));
  FBCHK(d2h(e, out_off, e->row_off.as<int>() + j, sizeof(out_off)));
  FBCHK(d2h(e, &kept, e->wb_feco_k.as<int>() + j, sizeof(int)));
  FBCHK(sync_stream(e));
  *Tv = in_off[1] - in_off[0];
  *k = out_off[1] - out_off[0];
  if (kept != *k) return fb_fail(FB_E_HIP, "the kept k %d is not the row's centre count %d", kept, *k);
  if (*Tv < 0 || *k < 0 || *Tv > cap || *k > cap) return fb_fail(FB_E_ARG, "%d rows, %d centres: more than the arrays hold (%d)", *Tv, *k, cap);
  if (*Tv > 0) FBCHK(d2h(e, labels, e->wb_feco_label.as<int>() + in_off[0], sizeof(int) * (size_t)*Tv));
  if (*k > 0) FBCHK(d2h(e, counts, e->wb_feco_cnt.as<int>() + out_off[0], sizeof(int) * (size_t)*k));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// Test hook: k_air_conv_t alone, on taps, cotangents and saturation bytes handed in: B rows of n samples, one launch
extern "C" int fb_debug_air_conv_t(fb_engine *e, const int16_t *taps, int B, int L, int64_t n, const double *cot, const unsigned char *sat,
                                   double *dx) {
  if (!e || !taps || !cot || !dx || B <= 0 || B > 65535 || L < 2 || L > 4096 || n <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "row longer than 2^31 samples");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t samples = (size_t)B * (size_t)n;
  DevBuf d_t, d_cot, d_sat, d_dx;
  FBCHK(d_t.ensure(sizeof(int16_t) * (size_t)B * (size_t)L));
  FBCHK(d_cot.ensure(sizeof(double) * samples));
  FBCHK(d_dx.ensure(sizeof(double) * samples));
  FBCHK(h2d(e, d_t.p, taps, sizeof(int16_t) * (size_t)B * (size_t)L));
  FBCHK(h2d(e, d_cot.p, cot, sizeof(double) * samples));
  if (sat) {
    FBCHK(d_sat.ensure(samples));
    FBCHK(h2d(e, d_sat.p, sat, samples));
  }
  e->wb_air_launches = 0;
  fb_launch_air_conv_t(e->stream, d_cot.as<double>(), sat ? d_sat.as<unsigned char>() : nullptr, B, n, d_t.as<int16_t>(), L, d_dx.as<double>(),
                       nullptr);
  e->wb_air_launches += 1;
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, dx, d_dx.p, sizeof(double) * samples));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_debug_wb_air_route(fb_engine *e, int *n_launches) {
  if (!e || !n_launches) return fb_fail(FB_E_ARG, "null argument");
  *n_launches = e->wb_air_launches;
  return FB_OK;
}

extern "C" int fb_debug_air_conv_t_chunk(void) { return fb_air_conv_t_chunk(); }

// Test hook: k_wb_iv_backend_t alone, on an i-vector and weights handed in
extern "C" int fb_debug_iv_backend_grad(fb_engine *e, const double *ivec, const double *w, double *out) {
  if (!e || !ivec || !w || !out) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_gmm || e->kind != 1) return fb_fail(FB_E_STATE, "load an i-vector system first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const FbIvDev &iv = e->iv;
  memset(e->wb_route, 0, sizeof(e->wb_route));
  FBCHK(e->wb_w.ensure(sizeof(double) * (size_t)iv.S));
  FBCHK(e->wb_iv_wbar.ensure(sizeof(double) * (size_t)iv.R));
  FBCHK(e->wb_iv_lam.ensure(sizeof(double) * (size_t)iv.R));
  FBCHK(h2d(e, e->wb_w.p, w, sizeof(double) * (size_t)iv.S));
  FBCHK(h2d(e, e->wb_iv_lam.p, ivec, sizeof(double) * (size_t)iv.R));   // (lambda's place is free until the solve)
  wb_launch_iv_backend_t(e, e->wb_iv_lam.as<double>(), nullptr);
  FBCHK(d2h(e, out, e->wb_iv_wbar.p, sizeof(double) * (size_t)iv.R));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// Test hook: the i-vector extractor's forward on Tv rows of features handed in as they are -- run_scoring's own launches behind
// the front end, as one utterance --, then wb_enqueue's launches from a cotangent cot[R] on the i-vector to the rows
extern "C" int fb_debug_iv_feat_grad(fb_engine *e, const float *feats, int Tv, const double *cot, double *out) {
  if (!e || !feats || !cot || !out || Tv <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 1) return fb_fail(FB_E_STATE, "load an i-vector system first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const FbIvDev &iv = e->iv;
  e->bench_it = e->nes_rec.iter = -1;
  memset(e->wb_route, 0, sizeof(e->wb_route));
  FBCHK(wb_prepare(e, 1, Tv, true));
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)Tv * iv.D));
  FBCHK(e->row_off.ensure(sizeof(int) * 2));
  FBCHK(e->tv.ensure(sizeof(int)));
  const int rows_host[2] = {0, Tv};
  HIPCHK(hipMemcpy(e->feats.p, feats, sizeof(float) * (size_t)Tv * iv.D, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->row_off.p, rows_host, sizeof(rows_host), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->tv.p, &Tv, sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->wb_iv_wbar.p, cot, sizeof(double) * (size_t)iv.R, hipMemcpyHostToDevice));
  e->cached_B = -1;
  FbScoreCall call{scoring_call_point(e)};
  call.feats_given = true;
  call.keep_iv_quad = true;
  FBCHK(run_scoring(e, call, 1, Tv));
  wb_launch_iv_backward(e, e->row_off.as<int>() + 1, Tv, nullptr);
  FBCHK(d2h(e, out, e->wb_g.p, sizeof(double) * (size_t)Tv * iv.D));
  int fail = 0;
  FBCHK(d2h(e, &fail, e->iv_fail.p, sizeof(int)));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  if (fail) return fb_fail(FB_E_ARG, "i-vector system of utterance %d is not positive definite", fail - 1);
  return FB_OK;
}

// mirrors FakeBob.attack (FAKEBOB.py:139-221) with the analytic gradient in place of get_grad: the loop control runs on the
// device (k_wb_ctl), the host looks at the control block once per FB_ATTACK_BATCH iterations, as attack_loop does
extern "C" int fb_attack_wb(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, int16_t *adv_i16,
                            double *adver_f64, double *trace, int *n_trace, int *success_flag) {
  wb_call_begin(e);
  if (!adv_i16 || !success_flag) return fb_fail(FB_E_ARG, "null argument");
  fb_nes_params q;
  FBCHK(wb_check(e, p, audio, N, &q));
  if (p->max_iter <= 0) return fb_fail(FB_E_ARG, "max_iter must be > 0");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(prepare_nes_replicas(e, N, 1));
  FBCHK(ensure_nes_buffers(e, N, 1));
  FBCHK(wb_prepare(e, N, e->h_frame_off[1], true));
  const int S = fb_num_speakers(e);
  FBCHK(attack_start(e, audio, N, 0, nullptr));
  cast_a0(e, &q, e->audio.as<double>(), N);  // (fb_set_wb_universal: a_0 = the audio the attack was handed, as in fb_attack)
  double *trace_dev = nullptr;
  if (trace) {
    FBCHK(e->trace_dev.ensure(sizeof(double) * (size_t)p->max_iter * (3 + S)));
    trace_dev = e->trace_dev.as<double>();
  }
  FBCHK(e->ticks.ensure(sizeof(unsigned long long) * ((size_t)p->max_iter + 1)));
  FBCHK(ctl_reset(e, &q, true, false, e->ticks.as<unsigned long long>()));
  FbCtlDev *ctl = e->ctl.as<FbCtlDev>();
  const int look = attack_batch();
  const double one_minus_m = 1.0 - p->momentum;
  for (int queued = 0; queued < p->max_iter;) {
    const int nb = p->max_iter - queued < look ? p->max_iter - queued : look;
    int rc = FB_OK;
    for (int k = 0; k < nb && rc == FB_OK; ++k) {
      rc = wb_enqueue(e, &q, N, (uint32_t)(queued + k), true, ctl, trace_dev);
      if (rc == FB_OK)
        fb_launch_wb_update(e->stream, e->grad.as<double>(), N, p->momentum, one_minus_m, p->epsilon, e->audio.as<double>(),
                            e->grad_m.as<double>(), e->adver.as<double>(), ctl);
    }
    if (rc != FB_OK) { (void)sync_stream(e); return rc; }   // (what was queued before the failure runs out first)
    FBCHK(wb_look(e, nullptr, nullptr, 0));
    queued += nb;
    if (e->h_ctl->stop) break;
  }
  HIPCHK(hipGetLastError());
  const int rows = e->h_ctl->iters_done;  // one trace row per executed iteration, the stopping one included
  e->nes_iters += rows;
  FBCHK(collect_iter_seconds(e, rows));
  if (trace && rows > 0) FBCHK(d2h(e, trace, trace_dev, sizeof(double) * (size_t)rows * (3 + S)));
  const int last_iter = e->h_ctl->broke ? e->h_ctl->stop_iter : p->max_iter - 1;
  *success_flag = (last_iter < p->max_iter - 1) ? 1 : -1;  // :219
  if (n_trace) *n_trace = rows;
  fb_launch_quantize(e->stream, e->adver.as<double>(), N, nes_bits(p), e->wav.as<int16_t>());  // :220
  FBCHK(d2h(e, adv_i16, e->wav.p, sizeof(int16_t) * (size_t)N));
  if (adver_f64) FBCHK(d2h(e, adver_f64, e->adver.p, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// ------------------------------------------------- the L2 white-box attack
// fb_attack_cw2 (the "CW2" section of fakebob_hip.h): Carlini-Wagner's L2 attack on wb_enqueue's gradient.  Per search step a
// reset launch; per iteration wb_enqueue (its control launch forms the weights with the stop on adver_loss < 0 disabled and
// writes no trace row) + k_cw2_ctl + k_cw2_step.  The host looks once per FB_ATTACK_BATCH iterations and between search steps,
// where it also moves the constant.  The loop itself is tanh_attack's, below the masking attack's helpers.
static int cw2_check(const fb_engine *e, const fb_nes_params *p, const fb_cw2_params *c) {
  // refused by name whatever the white-box switches say: none of them has a CW2 test of its own in this version
  if (e->comp_K1 > 0) return fb_fail(FB_E_STATE, "CW2: companions are set (fb_set_companions: clear them)");
  FBCHK(refuse_play(e, "CW2 / the masking attack"));
  if (e->air.L > 0) return fb_fail(FB_E_STATE, "CW2: an air channel is set (fb_set_air_channel: clear it)");
  if (e->feco_iters > 0) return fb_fail(FB_E_STATE, "CW2: feature compression is on (fb_set_feature_compression: switch it off)");
  if (e->cfg.dither > 0.0) return fb_fail(FB_E_STATE, "CW2: dither %g > 0 (set 0)", e->cfg.dither);
  if (c->search_steps < 1 || c->search_steps > 32) return fb_fail(FB_E_ARG, "CW2: search_steps %d outside 1 .. 32", c->search_steps);
  if (!isfinite(c->initial_const) || !(c->initial_const > 0.0)) return fb_fail(FB_E_ARG, "CW2: initial_const must be finite and > 0");
  if (!isfinite(c->lr) || !(c->lr > 0.0)) return fb_fail(FB_E_ARG, "CW2: lr must be finite and > 0");
  if (!isfinite(c->adam_eps) || !(c->adam_eps > 0.0)) return fb_fail(FB_E_ARG, "CW2: adam_eps must be finite and > 0");
  if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0))
    return fb_fail(FB_E_ARG, "CW2: beta1 and beta2 must lie in [0, 1)");
  if (c->abort_every < 0) return fb_fail(FB_E_ARG, "CW2: abort_every must be >= 0");
  if (p->max_iter < 1) return fb_fail(FB_E_ARG, "max_iter must be > 0");
  if ((int64_t)c->search_steps * p->max_iter > (int64_t)1 << 30)
    return fb_fail(FB_E_ARG, "CW2: search_steps * max_iter = %lld iterations: at most 2^30", (long long)c->search_steps * p->max_iter);
  return FB_OK;
}
static int cw2_buffers(fb_engine *e, int64_t N) {
  for (DevBuf *b : {&e->cw2_w0, &e->cw2_mod, &e->cw2_m2, &e->cw2_best_x}) FBCHK(b->ensure(sizeof(double) * (size_t)N));
  FBCHK(e->cw2_best_row.ensure(sizeof(int16_t) * (size_t)N));
  FBCHK(e->cw2_l2part.ensure(sizeof(double) * (size_t)((N + 255) / 256)));
  FBCHK(e->cw2_ctl.ensure(sizeof(FbCw2Dev)));
  return FB_OK;
}
// the binary search over the constant between two search steps (SpeakerGuard's CW2: lower / upper bound, tenfold while no
// success has bounded it)
static void cw2_next_const(bool found, double *lo, double *hi, double *c) {
  if (found) {
    *hi = *hi < *c ? *hi : *c;
    *c = (*lo + *hi) / 2.0;
  } else {
    *lo = *lo > *c ? *lo : *c;
    *c = *hi < 1e9 ? (*lo + *hi) / 2.0 : *c * 10.0;
  }
}

// ------------------------------------------------- the psychoacoustic white-box attack
// fb_attack_psy (the "masking" section of fakebob_hip.h): fb_attack_cw2's loop (tanh_attack) with the distortion D(delta) +
// l2_weight * l2.  Per iteration wb_enqueue + k_psy_frames + k_psy_ctl + k_psy_step; the reset launch of a search step is CW2's.
static int psy_frames_of(int64_t N, int W) {
  const int hop = W / 4;
  return N == W ? 1 : (int)((N - W + hop - 1) / hop) + 1;
}
static int psy_check(const fb_psy_params *m, int64_t N) {
  if (!m->theta) return fb_fail(FB_E_ARG, "masking: null threshold");
  const int W = m->window;
  if (W != 512 && W != 1024 && W != 2048) return fb_fail(FB_E_ARG, "masking: window %d is not 512, 1024 or 2048", W);
  if (N < W) return fb_fail(FB_E_ARG, "masking: %lld samples are fewer than the window %d", (long long)N, W);
  const int F = psy_frames_of(N, W);
  if (m->n_frames != F) return fb_fail(FB_E_ARG, "masking: n_frames %d, but %lld samples at window %d make %d", m->n_frames, (long long)N, W, F);
  if (!isfinite(m->psd_max) || !(m->psd_max > 0.0)) return fb_fail(FB_E_ARG, "masking: psd_max must be finite and > 0");
  if (!isfinite(m->l2_weight) || m->l2_weight < 0.0) return fb_fail(FB_E_ARG, "masking: l2_weight must be finite and >= 0");
  const size_t n = (size_t)F * (size_t)(W / 2 + 1);
  for (size_t i = 0; i < n; ++i)
    if (!isfinite(m->theta[i]) || m->theta[i] < 0.0)
      return fb_fail(FB_E_ARG, "masking: theta[%zu] = %g is not a finite, non-negative power", i, m->theta[i]);
  return FB_OK;
}
// cos and sin of 2 pi t / W for t < W / 2, from arguments of at most pi / 4: exact at the octants and symmetric about them,
// as sincospi would give them
static void psy_twiddle(int t, int W, double *c, double *s) {
  const double w = 2.0 * M_PI / (double)W;
  if (8 * t == W) { *c = M_SQRT1_2; *s = M_SQRT1_2; }
  else if (8 * t == 3 * W) { *c = -M_SQRT1_2; *s = M_SQRT1_2; }
  else if (8 * t < W) { *c = cos(w * t); *s = sin(w * t); }
  else if (4 * t <= W) { *c = sin(w * (W / 4 - t)); *s = cos(w * (W / 4 - t)); }
  else if (8 * t < 3 * W) { *c = -sin(w * (t - W / 4)); *s = cos(w * (t - W / 4)); }
  else { *c = -cos(w * (W / 2 - t)); *s = sin(w * (W / 2 - t)); }
}
// the twiddle table of the window (once per window), the threshold in bit-reversed order, the frames' workspace
static int psy_upload(fb_engine *e, const fb_psy_params *m, int64_t N, bool want_P) {
  const int W = m->window, H = W / 2, K = H + 1, F = m->n_frames;
  if (e->psy_tw_W != W) {
    std::vector<double> tw((size_t)W);
    for (int t = 0; t < H; ++t) psy_twiddle(t, W, &tw[(size_t)t], &tw[(size_t)(H + t)]);
    FBCHK(e->psy_tw.ensure(sizeof(double) * (size_t)W));
    FBCHK(h2d(e, e->psy_tw.p, tw.data(), sizeof(double) * (size_t)W));
    FBCHK(sync_stream(e));
    e->psy_tw_W = W;
  }
  int logw = 0;
  while ((1 << logw) < W) ++logw;
  std::vector<double> br((size_t)F * (size_t)W);
  for (int f = 0; f < F; ++f)
    for (int pos = 0; pos < W; ++pos) {
      int k = 0;
      for (int b = 0; b < logw; ++b) k |= ((pos >> b) & 1) << (logw - 1 - b);
      br[(size_t)f * W + pos] = k <= H ? m->theta[(size_t)f * K + k] : INFINITY;
    }
  FBCHK(e->psy_theta.ensure(sizeof(double) * br.size()));
  FBCHK(e->psy_gf.ensure(sizeof(double) * (br.size() > (size_t)N ? br.size() : (size_t)N)));
  FBCHK(e->psy_dpart.ensure(sizeof(double) * (size_t)F));
  FBCHK(e->psy_npart.ensure(sizeof(int) * (size_t)F));
  FBCHK(e->psy_ctl.ensure(sizeof(FbPsyDev)));
  if (want_P) FBCHK(e->psy_P.ensure(sizeof(double) * (size_t)F * K));
  FBCHK(h2d(e, e->psy_theta.p, br.data(), sizeof(double) * br.size()));
  FBCHK(sync_stream(e));   // (br is a local)
  return FB_OK;
}
static void psy_scales(const fb_psy_params *m, double *scale, double *coef) {
  const double W = (double)m->window;
  *scale = (8.0 / 3.0) / (W * W) * (pow(10.0, 9.6) / m->psd_max);
  *coef = 2.0 * *scale / ((double)m->n_frames * (double)(m->window / 2 + 1));
}

// The tanh-space attack both entry points run: m == nullptr is CW2, else the masking attack with *m.  The caller has looked at
// its own arguments; h: the control block as the last look left it (CW2: its `cw` member alone), final_const: the constant
// after the last search step.
static_assert(offsetof(FbPsyDev, cw) == 0, "a CW2 control block is the head of a masking one");
static int tanh_attack(fb_engine *e, const fb_nes_params *p, const fb_cw2_params *c, const fb_psy_params *m, const double *audio,
                       int64_t N, int16_t *adv_i16, double *adver_f64, double *trace, int *n_trace, int *rows_per_step, FbPsyDev *h,
                       double *final_const) {
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  FBCHK(cw2_check(e, p, c));   // (CW2's own checks and messages for both)
  fb_nes_params q;
  FBCHK(wb_check(e, p, audio, N, &q));
  if (m) FBCHK(psy_check(m, N));
  q.plateau_length = 0;   // (the loop control of wb_enqueue's control launch: no plateau rule, no stop of its own)
  HIPCHK(hipSetDevice(e->device));
  FBCHK(prepare_nes_replicas(e, N, 1));
  FBCHK(ensure_nes_buffers(e, N, 1));
  FBCHK(wb_prepare(e, N, e->h_frame_off[1], true));
  FBCHK(cw2_buffers(e, N));
  if (m) FBCHK(psy_upload(e, m, N, false));
  const int S = fb_num_speakers(e);
  const int W = m ? m->window : 0, F = m ? m->n_frames : 0, K = W / 2 + 1;
  double scale = 0.0, coef = 0.0;
  if (m) psy_scales(m, &scale, &coef);
  const int steps = c->search_steps, max_iter = p->max_iter;
  const size_t total = (size_t)steps * (size_t)max_iter, width = (size_t)((m ? 5 : 3) + S);
  {  // w0 = atanh(0.999999 a0) on the host: the device never evaluates atanh
    std::vector<double> w0((size_t)N);
    for (int64_t n = 0; n < N; ++n) w0[(size_t)n] = atanh(0.999999 * audio[n]);
    FBCHK(h2d(e, e->cw2_w0.p, w0.data(), sizeof(double) * (size_t)N));
    FBCHK(sync_stream(e));
  }
  FBCHK(attack_start(e, audio, N, 0, nullptr));
  // the best slots before any success: the cast of the original audio and the audio itself
  fb_launch_quantize(e->stream, e->audio.as<double>(), N, nes_bits(p), e->cw2_best_row.as<int16_t>());
  HIPCHK(hipMemcpyAsync(e->cw2_best_x.p, e->audio.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, e->stream));
  double *trace_dev = nullptr;
  if (trace) {
    FBCHK(e->trace_dev.ensure(sizeof(double) * total * width));
    trace_dev = e->trace_dev.as<double>();
  }
  FBCHK(e->ticks.ensure(sizeof(unsigned long long) * (total + 1)));
  FBCHK(ctl_reset(e, &q, true, true, e->ticks.as<unsigned long long>()));
  FbCtlDev *ctl = e->ctl.as<FbCtlDev>();
  FbPsyDev *ps = m ? e->psy_ctl.as<FbPsyDev>() : nullptr;
  FbCw2Dev *cw = m ? &ps->cw : e->cw2_ctl.as<FbCw2Dev>();
  const size_t block = m ? sizeof(FbPsyDev) : sizeof(FbCw2Dev);   // what is uploaded and fetched, at `cw` either way
  memset(h, 0, sizeof(*h));
  h->gbest_dist = INFINITY;
  h->cw.gbest_l2 = INFINITY;
  h->cw.prev = INFINITY;
  FBCHK(h2d(e, cw, h, block));
  const int look = attack_batch();
  double cc = c->initial_const, lo = 0.0, hi = 1e10;
  int rows = 0;
  for (int s = 0; s < steps; ++s) {
    fb_launch_cw2_reset(e->stream, e->cw2_w0.as<double>(), e->audio.as<double>(), N, cc, e->cw2_mod.as<double>(), e->grad_m.as<double>(),
                        e->cw2_m2.as<double>(), e->adver.as<double>(), e->cw2_l2part.as<double>(), cw, ctl);
    double p1 = 1.0, p2 = 1.0;
    for (int queued = 0; queued < max_iter;) {
      const int nb = max_iter - queued < look ? max_iter - queued : look;
      int rc = FB_OK;
      for (int k = 0; k < nb && rc == FB_OK; ++k) {
        const int t = queued + k;
        rc = wb_enqueue(e, &q, N, (uint32_t)((size_t)s * (size_t)max_iter + (size_t)t), false, ctl, nullptr);
        if (rc != FB_OK) break;
        p1 *= c->beta1;
        p2 *= c->beta2;
        const double step_size = c->lr / (1.0 - p1), bc2s = sqrt(1.0 - p2);
        if (m) {
          fb_launch_psy_frames(e->stream, W, F, e->adver.as<double>(), e->audio.as<double>(), N, e->psy_tw.as<double>(),
                               e->psy_theta.as<double>(), scale, coef, e->psy_gf.as<double>(), e->psy_dpart.as<double>(),
                               e->psy_npart.as<int>(), nullptr, ctl);
          fb_launch_psy_ctl(e->stream, e->nes_out.as<FbNesDev>(), e->scores.as<double>(), S, e->cw2_l2part.as<double>(), N,
                            e->psy_dpart.as<double>(), e->psy_npart.as<int>(), F, K, m->l2_weight, ps, ctl, trace_dev, t, c->abort_every);
          fb_launch_psy_step(e->stream, e->grad.as<double>(), e->psy_gf.as<double>(), F, W, e->audio.as<double>(), e->cw2_w0.as<double>(),
                             N, m->l2_weight, c->beta1, c->beta2, step_size, bc2s, c->adam_eps, e->cw2_mod.as<double>(),
                             e->grad_m.as<double>(), e->cw2_m2.as<double>(), e->adver.as<double>(), e->wav.as<int16_t>(),
                             e->cw2_best_row.as<int16_t>(), e->cw2_best_x.as<double>(), e->cw2_l2part.as<double>(), ps);
        } else {
          fb_launch_cw2_ctl(e->stream, e->nes_out.as<FbNesDev>(), e->scores.as<double>(), S, e->cw2_l2part.as<double>(), N, cw, ctl,
                            trace_dev, t, c->abort_every);
          fb_launch_cw2_step(e->stream, e->grad.as<double>(), e->audio.as<double>(), e->cw2_w0.as<double>(), N, c->beta1, c->beta2,
                             step_size, bc2s, c->adam_eps, e->cw2_mod.as<double>(), e->grad_m.as<double>(), e->cw2_m2.as<double>(),
                             e->adver.as<double>(), e->wav.as<int16_t>(), e->cw2_best_row.as<int16_t>(), e->cw2_best_x.as<double>(),
                             e->cw2_l2part.as<double>(), cw);
        }
      }
      if (rc != FB_OK) { (void)sync_stream(e); return rc; }   // (what was queued before the failure runs out first)
      FBCHK(wb_look(e, h, cw, block));
      queued += nb;
      if (e->h_ctl->stop) break;   // the abort rule
    }
    rows_per_step[s] = h->cw.rows - rows;
    rows = h->cw.rows;
    cw2_next_const(h->cw.found != 0, &lo, &hi, &cc);
  }
  HIPCHK(hipGetLastError());
  e->nes_iters += rows;
  FBCHK(collect_iter_seconds(e, rows));
  if (trace && rows > 0) FBCHK(d2h(e, trace, trace_dev, sizeof(double) * (size_t)rows * width));
  *final_const = cc;
  if (n_trace) *n_trace = rows;
  FBCHK(d2h(e, adv_i16, e->cw2_best_row.p, sizeof(int16_t) * (size_t)N));
  if (adver_f64) FBCHK(d2h(e, adver_f64, e->cw2_best_x.p, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_attack_cw2(fb_engine *e, const fb_nes_params *p, const fb_cw2_params *c, const double *audio, int64_t N,
                             int16_t *adv_i16, double *adver_f64, double *trace, int *n_trace, int *rows_per_step, int *success_flag,
                             double *best_l2, double *final_const) {
  wb_call_begin(e);
  if (!e || !p || !c || !audio || !adv_i16 || !success_flag || !rows_per_step || !best_l2 || !final_const)
    return fb_fail(FB_E_ARG, "null argument");
  FbPsyDev h;
  FBCHK(tanh_attack(e, p, c, nullptr, audio, N, adv_i16, adver_f64, trace, n_trace, rows_per_step, &h, final_const));
  *success_flag = h.cw.gbest_l2 < INFINITY ? 1 : -1;
  *best_l2 = h.cw.gbest_l2;
  return FB_OK;
}

extern "C" int fb_attack_psy(fb_engine *e, const fb_nes_params *p, const fb_cw2_params *c, const fb_psy_params *m,
                             const double *audio, int64_t N, int16_t *adv_i16, double *adver_f64, double *trace, int *n_trace,
                             int *rows_per_step, int *success_flag, double *best_dist, double *best_l2, int *best_n_over,
                             double *final_const) {
  wb_call_begin(e);
  if (!e || !p || !c || !m || !audio || !adv_i16 || !success_flag || !rows_per_step || !best_dist || !best_l2 || !best_n_over ||
      !final_const)
    return fb_fail(FB_E_ARG, "null argument");
  FbPsyDev h;
  FBCHK(tanh_attack(e, p, c, m, audio, N, adv_i16, adver_f64, trace, n_trace, rows_per_step, &h, final_const));
  *success_flag = h.gbest_dist < INFINITY ? 1 : -1;
  *best_dist = h.gbest_dist;
  *best_l2 = h.cw.gbest_l2;
  *best_n_over = h.gbest_dist < INFINITY ? h.gbest_n_over : 0;
  return FB_OK;
}

// Test hook: the masking loss and its gradient at a perturbation handed in (fakebob_hip_test.h); no system has to be loaded
extern "C" int fb_debug_psy_loss(fb_engine *e, const fb_psy_params *m, int64_t N, const double *delta, double *D, int *n_over,
                                 double *gd, double *P) {
  if (!e || !m || !delta || !D || !n_over || !gd || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(psy_check(m, N));
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  FBCHK(ensure_nes_buffers(e, N, 1, 1));
  FBCHK(psy_upload(e, m, N, P != nullptr));
  const int W = m->window, F = m->n_frames, K = W / 2 + 1;
  const size_t nb = sizeof(double) * (size_t)N;
  double scale, coef;
  psy_scales(m, &scale, &coef);
  FBCHK(h2d(e, e->adver.p, delta, nb));
  HIPCHK(hipMemsetAsync(e->audio.p, 0, nb, e->stream));   // delta = x - a0 with a0 = +0.0: exact
  fb_launch_psy_frames(e->stream, W, F, e->adver.as<double>(), e->audio.as<double>(), N, e->psy_tw.as<double>(),
                       e->psy_theta.as<double>(), scale, coef, e->psy_gf.as<double>(), e->psy_dpart.as<double>(), e->psy_npart.as<int>(),
                       P ? e->psy_P.as<double>() : nullptr, nullptr);
  fb_launch_psy_ola(e->stream, e->psy_gf.as<double>(), F, W, N, e->grad.as<double>());
  std::vector<double> dp((size_t)F);
  std::vector<int> np((size_t)F);
  FBCHK(d2h(e, dp.data(), e->psy_dpart.p, sizeof(double) * (size_t)F));
  FBCHK(d2h(e, np.data(), e->psy_npart.p, sizeof(int) * (size_t)F));
  FBCHK(d2h(e, gd, e->grad.p, nb));
  if (P) FBCHK(d2h(e, P, e->psy_P.p, sizeof(double) * (size_t)F * K));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  double d = 0.0;
  int cnt = 0;
  for (int f = 0; f < F; ++f) { d += dp[(size_t)f]; cnt += np[(size_t)f]; }   // ascending frames, as k_psy_ctl adds them
  *D = d / ((double)F * (double)K);
  *n_over = cnt;
  return FB_OK;
}

// What the two step hooks (fakebob_hip_test.h; no system has to be loaded) stage before their own control and step launches: the
// seven arrays, a fresh control block, adver_loss as the loss launch would have left it, the row the forward would have scored,
// the best slots as an attack without a success holds them, the l2 partials of x
static int tanh_step_stage(fb_engine *e, int64_t N, const double *g, const double *x, const double *a0, const double *w0,
                           const double *mod, const double *m1, const double *m2, double adver_loss) {
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  FBCHK(ensure_nes_buffers(e, N, 1, 1));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N));
  FBCHK(cw2_buffers(e, N));
  const size_t nb = sizeof(double) * (size_t)N;
  FBCHK(h2d(e, e->grad.p, g, nb));
  FBCHK(h2d(e, e->adver.p, x, nb));
  FBCHK(h2d(e, e->audio.p, a0, nb));
  FBCHK(h2d(e, e->cw2_w0.p, w0, nb));
  FBCHK(h2d(e, e->cw2_mod.p, mod, nb));
  FBCHK(h2d(e, e->grad_m.p, m1, nb));
  FBCHK(h2d(e, e->cw2_m2.p, m2, nb));
  fb_nes_params q;
  memset(&q, 0, sizeof(q));
  FBCHK(ctl_reset(e, &q, false, true, nullptr));
  FbNesDev h_out;
  memset(&h_out, 0, sizeof(h_out));
  h_out.adver_loss = adver_loss;
  FBCHK(h2d(e, e->nes_out.p, &h_out, sizeof(h_out)));
  fb_launch_quantize(e->stream, e->adver.as<double>(), N, 16, e->wav.as<int16_t>());
  fb_launch_quantize(e->stream, e->audio.as<double>(), N, 16, e->cw2_best_row.as<int16_t>());
  HIPCHK(hipMemcpyAsync(e->cw2_best_x.p, e->audio.p, nb, hipMemcpyDeviceToDevice, e->stream));
  fb_launch_cw2_l2(e->stream, e->adver.as<double>(), e->audio.as<double>(), N, e->cw2_l2part.as<double>());
  return FB_OK;
}
// ... and what they fetch behind the step launch: mod, m1, m2, x_next, the best slots, and l2 of x_next from its partials
static int tanh_step_fetch(fb_engine *e, int64_t N, double *mod_out, double *m1_out, double *m2_out, double *x_next, double *l2_next,
                           int16_t *best_row, double *best_x) {
  const size_t nb = sizeof(double) * (size_t)N, np = (size_t)((N + 255) / 256);
  std::vector<double> part(np);
  FBCHK(d2h(e, part.data(), e->cw2_l2part.p, sizeof(double) * np));
  FBCHK(d2h(e, mod_out, e->cw2_mod.p, nb));
  FBCHK(d2h(e, m1_out, e->grad_m.p, nb));
  FBCHK(d2h(e, m2_out, e->cw2_m2.p, nb));
  FBCHK(d2h(e, x_next, e->adver.p, nb));
  FBCHK(d2h(e, best_row, e->cw2_best_row.p, sizeof(int16_t) * (size_t)N));
  FBCHK(d2h(e, best_x, e->cw2_best_x.p, nb));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  double l2 = 0.0;
  for (size_t i = 0; i < np; ++i) l2 += part[i];   // ascending block order, as the control kernels add them
  *l2_next = l2;
  return FB_OK;
}

// Test hook: one k_cw2_ctl + k_cw2_step pair on arrays handed in
extern "C" int fb_debug_cw2_step(fb_engine *e, const fb_cw2_params *c, int64_t N, const double *g, const double *x, const double *a0,
                                 const double *w0, const double *mod, const double *m1, const double *m2, double adver_loss,
                                 double cc, double gbest_l2, int t, double p1, double p2, double *mod_out, double *m1_out,
                                 double *m2_out, double *x_next, double *l2_now, double *l2_next, int *gate, int *take,
                                 int16_t *best_row, double *best_x) {
  if (!e || !c || !g || !x || !a0 || !w0 || !mod || !m1 || !m2 || !mod_out || !m1_out || !m2_out || !x_next || !l2_now || !l2_next ||
      !gate || !take || !best_row || !best_x || N <= 0 || t < 0)
    return fb_fail(FB_E_ARG, "bad argument");
  if (!(p1 >= 0.0 && p1 < 1.0) || !(p2 >= 0.0 && p2 < 1.0)) return fb_fail(FB_E_ARG, "p1 and p2 must lie in [0, 1)");
  FBCHK(tanh_step_stage(e, N, g, x, a0, w0, mod, m1, m2, adver_loss));
  FbCw2Dev h_cw;
  memset(&h_cw, 0, sizeof(h_cw));
  h_cw.c = cc; h_cw.gbest_l2 = gbest_l2; h_cw.prev = INFINITY;
  FbCw2Dev *cw = e->cw2_ctl.as<FbCw2Dev>();
  FBCHK(h2d(e, cw, &h_cw, sizeof(h_cw)));
  fb_launch_cw2_ctl(e->stream, e->nes_out.as<FbNesDev>(), e->scores.as<double>(), 0, e->cw2_l2part.as<double>(), N, cw, e->ctl.as<FbCtlDev>(),
                    nullptr, t, c->abort_every);
  FBCHK(d2h(e, &h_cw, cw, sizeof(h_cw)));   // (queued before the step launch: l2 of x, gate and take as k_cw2_ctl left them)
  fb_launch_cw2_step(e->stream, e->grad.as<double>(), e->audio.as<double>(), e->cw2_w0.as<double>(), N, c->beta1, c->beta2,
                     c->lr / (1.0 - p1), sqrt(1.0 - p2), c->adam_eps, e->cw2_mod.as<double>(), e->grad_m.as<double>(),
                     e->cw2_m2.as<double>(), e->adver.as<double>(), e->wav.as<int16_t>(), e->cw2_best_row.as<int16_t>(),
                     e->cw2_best_x.as<double>(), e->cw2_l2part.as<double>(), cw);
  FBCHK(tanh_step_fetch(e, N, mod_out, m1_out, m2_out, x_next, l2_next, best_row, best_x));
  *l2_now = h_cw.l2;
  *gate = h_cw.gate;
  *take = h_cw.take;
  return FB_OK;
}

// Test hook: one k_psy_ctl + k_psy_step pair on arrays handed in; D and n_over as one "frame" of one bin: D = D / (1 * 1)
extern "C" int fb_debug_psy_step(fb_engine *e, const fb_cw2_params *c, double l2_weight, int64_t N, const double *g, const double *gd,
                                 const double *x, const double *a0, const double *w0, const double *mod, const double *m1,
                                 const double *m2, double adver_loss, double cc, double D, int n_over, double gbest_dist, int t,
                                 double p1, double p2, double *mod_out, double *m1_out, double *m2_out, double *x_next,
                                 double *l2_now, double *dist_now, double *l2_next, int *gate, int *take, int16_t *best_row,
                                 double *best_x) {
  if (!e || !c || !g || !gd || !x || !a0 || !w0 || !mod || !m1 || !m2 || !mod_out || !m1_out || !m2_out || !x_next || !l2_now ||
      !dist_now || !l2_next || !gate || !take || !best_row || !best_x || N <= 0 || t < 0)
    return fb_fail(FB_E_ARG, "bad argument");
  if (!(p1 >= 0.0 && p1 < 1.0) || !(p2 >= 0.0 && p2 < 1.0)) return fb_fail(FB_E_ARG, "p1 and p2 must lie in [0, 1)");
  if (!isfinite(l2_weight) || l2_weight < 0.0) return fb_fail(FB_E_ARG, "masking: l2_weight must be finite and >= 0");
  FBCHK(tanh_step_stage(e, N, g, x, a0, w0, mod, m1, m2, adver_loss));
  FBCHK(e->psy_gf.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->psy_dpart.ensure(sizeof(double)));
  FBCHK(e->psy_npart.ensure(sizeof(int)));
  FBCHK(e->psy_ctl.ensure(sizeof(FbPsyDev)));
  FBCHK(h2d(e, e->psy_gf.p, gd, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->psy_dpart.p, &D, sizeof(double)));
  FBCHK(h2d(e, e->psy_npart.p, &n_over, sizeof(int)));
  FbPsyDev h_ps;
  memset(&h_ps, 0, sizeof(h_ps));
  h_ps.cw.c = cc; h_ps.gbest_dist = gbest_dist; h_ps.cw.gbest_l2 = INFINITY; h_ps.cw.prev = INFINITY;
  FbPsyDev *ps = e->psy_ctl.as<FbPsyDev>();
  FBCHK(h2d(e, ps, &h_ps, sizeof(h_ps)));
  FBCHK(sync_stream(e));   // (D and n_over are arguments)
  fb_launch_psy_ctl(e->stream, e->nes_out.as<FbNesDev>(), e->scores.as<double>(), 0, e->cw2_l2part.as<double>(), N,
                    e->psy_dpart.as<double>(), e->psy_npart.as<int>(), 1, 1, l2_weight, ps, e->ctl.as<FbCtlDev>(), nullptr, t,
                    c->abort_every);
  FBCHK(d2h(e, &h_ps, ps, sizeof(h_ps)));   // (queued before the step launch: l2, dist, gate and take as k_psy_ctl left them)
  fb_launch_psy_step(e->stream, e->grad.as<double>(), e->psy_gf.as<double>(), 0, 0, e->audio.as<double>(), e->cw2_w0.as<double>(), N,
                     l2_weight, c->beta1, c->beta2, c->lr / (1.0 - p1), sqrt(1.0 - p2), c->adam_eps, e->cw2_mod.as<double>(),
                     e->grad_m.as<double>(), e->cw2_m2.as<double>(), e->adver.as<double>(), e->wav.as<int16_t>(),
                     e->cw2_best_row.as<int16_t>(), e->cw2_best_x.as<double>(), e->cw2_l2part.as<double>(), ps);
  FBCHK(tanh_step_fetch(e, N, mod_out, m1_out, m2_out, x_next, l2_next, best_row, best_x));
  *l2_now = h_ps.cw.l2;
  *dist_now = h_ps.dist;
  *gate = h_ps.cw.gate;
  *take = h_ps.cw.take;
  return FB_OK;
}

extern "C" int fb_debug_nes_route(fb_engine *e, int *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  for (int i = 0; i < FB_NES_ROUTE_N; ++i) info[i] = e->nes_route[i];
  return FB_OK;
}

extern "C" int fb_debug_nes_batch(fb_engine *e, int64_t N, int half, int16_t *q, float *z, long long *iter) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  const auto &r = e->nes_rec;
  if (r.iter < 0) return fb_fail(FB_E_STATE, "fb_debug_nes_batch: no NES batch is resident on the engine");
  if (N != r.N || half != r.half)
    return fb_fail(FB_E_ARG, "fb_debug_nes_batch: N %lld, half %d; the last call ran N %lld, half %d", (long long)N, half,
                   (long long)r.N, r.half);
  const int B = 2 * half + 1;
  const size_t nq = sizeof(int16_t) * (size_t)N * B, nz = sizeof(float) * (size_t)N * half;
  if (q && (!r.q || e->cached_B != B || e->cached_N != N || nq > e->wav.cap))
    return fb_fail(FB_E_STATE, "fb_debug_nes_batch: the engine holds no int16 batch of the last call (a foreign model's is in its x)");
  if (z && (!r.z || nz > e->zbuf.cap))
    return fb_fail(FB_E_STATE, "fb_debug_nes_batch: the last call kept no normals (it ran on injected ones)");
  HIPCHK(hipSetDevice(e->device));
  if (q) FBCHK(d2h(e, q, e->wav.p, nq));
  if (z) FBCHK(d2h(e, z, e->zbuf.p, nz));
  FBCHK(sync_stream(e));
  if (iter) *iter = r.iter;
  return FB_OK;
}

extern "C" int fb_debug_foreign_path(fb_engine *e, fb_foreign_path_info *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  if (e->foreign.path == 0) return fb_fail(FB_E_STATE, "no foreign-model call has run yet");
  *info = e->foreign;
  return FB_OK;
}

extern "C" int fb_attack_iter_seconds(fb_engine *e, double *seconds, int n) {
  if (!e || !seconds || n < 0) return fb_fail(FB_E_ARG, "bad argument");
  if ((size_t)n > e->iter_seconds.size()) return fb_fail(FB_E_STATE, "the last attack ran %zu iterations (asked for %d)", e->iter_seconds.size(), n);
  for (int i = 0; i < n; ++i) seconds[i] = e->iter_seconds[i];
  return FB_OK;
}

// ------------------------------------------------- particle-swarm attack
// fb_attack_pso (the "particle-swarm attack" section of fakebob_hip.h).  The swarm is a batch of P rows: the ordinary path
// scores it, k_loss forms loss[P] and scores[P][S], the host reads them once per iteration, decides the personal and global
// bests and the stop, and k_pso_step moves the swarm -- taking the best-copies and the next batch's int16 cast along.
// The fused finalisation, the i-vector tail-loss shortcut and the device control block are not used.
// Under fb_set_query_eot with R = K * eot > 1 replicas the batch of the three query attacks is the replicated one of fb_attack
// (prepare_nes_replicas, call.eot, call.K): PSO then reads k_loss_eot's means, the two decision-only attacks k_vote's look block.
// What fb_set_eot and fb_set_companions mean to the three query attacks (`who`: the public call).  Switch off
// (fb_set_query_eot): both are refused.  On: *r = K * eot replicas of every candidate row and *quorum = the adversarial
// replicas a row needs (majority: r / 2 + 1); an explicit quorum no row can reach is refused here, before anything runs.
static int query_replicas(const fb_engine *e, const char *who, int *r, int *quorum) {
  *r = 1;
  *quorum = 1;
  FBCHK(refuse_play(e, who));  // (with or without fb_set_query_eot)
  if (e->query_quorum == FB_QUORUM_OFF) {
    if (e->eot > 1)
      return fb_fail(FB_E_STATE, "%s does not run under expectation over transformation (fb_set_eot(%d)): set 1", who, e->eot);
    if (e->comp_K1 > 0)
      return fb_fail(FB_E_STATE, "%s does not run with companion utterances (fb_set_companions: %d set): clear them", who, e->comp_K1);
    return FB_OK;
  }
  *r = nes_replicas(e);
  *quorum = e->query_quorum == FB_QUORUM_MAJORITY ? *r / 2 + 1 : e->query_quorum;
  if (*quorum > *r)
    return fb_fail(FB_E_ARG, "quorum %d (fb_set_query_eot) with utterances * eot = %d replicas per row: no row can reach it", *quorum, *r);
  return FB_OK;
}
// k_vote's look block for `rows` candidate rows of S scores on the device (e->vote_look) and on the host: votes[rows],
// nodec[rows] (int32), mean[rows][S] (float64), contiguous
struct FbVoteLook {
  int *votes, *nodec;
  double *mean;
  size_t bytes;
};
static size_t vote_look_bytes(int rows, int S) { return sizeof(int) * 2 * (size_t)rows + sizeof(double) * (size_t)rows * S; }
static FbVoteLook vote_look_at(void *base, int rows, int S) {
  FbVoteLook v;
  v.votes = static_cast<int *>(base);
  v.nodec = v.votes + rows;
  v.mean = reinterpret_cast<double *>(v.nodec + rows);
  v.bytes = vote_look_bytes(rows, S);
  return v;
}
// the launch behind the replicated scoring path of rows * r rows: e->raw, e->tv -> e->vote_look
static void launch_vote(fb_engine *e, const fb_nes_params *p, int rows, int r, bool targeted, int label) {
  const FbVoteLook v = vote_look_at(e->vote_look.p, rows, fb_num_speakers(e));
  fb_launch_vote(e->stream, e->raw.as<double>(), e->tv.as<int>(), rows, r, e->n_out, p->task, e->kind, e->zmean.as<double>(),
                 e->zstd.as<double>(), p->threshold, targeted ? 1 : 0, label, e->eot_sc.as<double>(), v.votes, v.nodec, v.mean);
}

// ------------------------------------------------- foreign victims of the three query attacks
// fb_attack_pso_foreign / _kenansville_foreign / _hsj_foreign (the "foreign victims" section of fakebob_hip.h).  The three
// drivers below write their int16 batch into e->wav exactly as for the engine's own systems; where those call run_scoring,
// a foreign call converts the rows (k_rows_to_model), hands them to the model -- through the host's staging memory or in the
// model's own device buffer -- and reads scores or decisions back.  None of the engine's front end, defences or batch
// layout is touched, so no system need be loaded.
struct FbForeignRun {
  const fb_victim *v = nullptr;
  int S = 0, rows_max = 0, bits = 16, task = 0;
  int64_t N = 0;
  double threshold = 0.0;
  std::vector<double> sc_h, spill, look;   // the callback's scores, a batch too large for the staging arena, the look block
  std::vector<int> dec_h;
};
// k_decide_foreign's look block for `rows` rows of S scores: decisions[rows] int32, padded to 8 bytes, scores[rows][S] float64
static size_t foreign_look_doubles(int rows, int S) { return ((size_t)rows + 1) / 2 + (size_t)rows * S; }

// the descriptor's checks and the settings a foreign victim refuses (`who`: the public call; decisions_ok: the call takes
// FB_VICTIM_HOST_DECISIONS), then the buffers of batches of up to rows_max rows
static int foreign_setup(fb_engine *e, const char *who, const fb_nes_params *p, const fb_victim *v, int64_t N, int rows_max,
                         bool decisions_ok, FbForeignRun *fr) {
  if (v->mode != FB_VICTIM_HOST_SCORES && v->mode != FB_VICTIM_HOST_DECISIONS && v->mode != FB_VICTIM_DEVICE_SCORES)
    return fb_fail(FB_E_ARG, "%s: unknown victim mode %d", who, v->mode);
  if (v->mode == FB_VICTIM_HOST_DECISIONS && !decisions_ok)
    return fb_fail(FB_E_ARG, "%s reads scores: FB_VICTIM_HOST_DECISIONS is not for it", who);
  if (v->mode == FB_VICTIM_HOST_SCORES && !v->score) return fb_fail(FB_E_ARG, "%s: FB_VICTIM_HOST_SCORES without a score callback", who);
  if (v->mode == FB_VICTIM_HOST_DECISIONS && !v->decide) return fb_fail(FB_E_ARG, "%s: FB_VICTIM_HOST_DECISIONS without a decide callback", who);
  if (v->mode == FB_VICTIM_DEVICE_SCORES && (!v->dev || !v->score_dev))
    return fb_fail(FB_E_ARG, "%s: FB_VICTIM_DEVICE_SCORES without dev or score_dev", who);
  if (p->task != FB_TASK_OSI && p->task != FB_TASK_CSI && p->task != FB_TASK_SV) return fb_fail(FB_E_ARG, "bad task %d", p->task);
  if (v->S <= 0 || v->S > 62) return fb_fail(FB_E_ARG, "number of speakers must be in [1, 62] (got %d)", v->S);
  if (p->task == FB_TASK_SV && v->S != 1) return fb_fail(FB_E_ARG, "SV scores one speaker (got S = %d)", v->S);
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  // a foreign victim's randomness is its own
  if (e->eot > 1)
    return fb_fail(FB_E_STATE, "%s does not run under expectation over transformation (fb_set_eot(%d)): set 1", who, e->eot);
  if (e->comp_K1 > 0)
    return fb_fail(FB_E_STATE, "%s does not run with companion utterances (fb_set_companions: %d set): clear them", who, e->comp_K1);
  FBCHK(refuse_play(e, who));
  if (e->query_quorum != FB_QUORUM_OFF)
    return fb_fail(FB_E_STATE, "%s does not vote (fb_set_query_eot(%d)): set 0", who, e->query_quorum);
  fr->v = v;
  fr->S = v->S;
  fr->rows_max = rows_max;
  fr->bits = nes_bits(p);
  fr->task = p->task;
  fr->N = N;
  fr->threshold = p->threshold;
  return FB_OK;
}
// ... once the call's own parameters have passed as well (fr->rows_max rows of N samples at the most)
static int foreign_buffers(fb_engine *e, FbForeignRun *fr) {
  const fb_victim *v = fr->v;
  const size_t rows = (size_t)fr->rows_max, N = (size_t)fr->N, S = (size_t)fr->S;
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  if (v->mode == FB_VICTIM_DEVICE_SCORES) {   // fb_attack_dev's checks, without look_every
    const fb_dev_model *m = v->dev;
    if (m->x_dtype != FB_DT_F32 && m->x_dtype != FB_DT_F64)
      return fb_fail(FB_E_ARG, "x_dtype %d: FB_DT_F32 (%d) or FB_DT_F64 (%d)", m->x_dtype, FB_DT_F32, FB_DT_F64);
    if (m->score_dtype != FB_DT_F32 && m->score_dtype != FB_DT_F64)
      return fb_fail(FB_E_ARG, "score_dtype %d: FB_DT_F32 (%d) or FB_DT_F64 (%d)", m->score_dtype, FB_DT_F32, FB_DT_F64);
    FBCHK(check_dev_buffer(e, "x", m->x, (m->x_dtype == FB_DT_F32 ? sizeof(float) : sizeof(double)) * N * rows));
    FBCHK(check_dev_buffer(e, "scores", m->scores, (m->score_dtype == FB_DT_F32 ? sizeof(float) : sizeof(double)) * rows * S));
  } else {
    FBCHK(e->ext_x.ensure(sizeof(double) * N * rows));
    FBCHK(e->raw.ensure(sizeof(double) * rows * S));
    fr->sc_h.resize(rows * S);
    fr->dec_h.resize(rows);
  }
  e->cached_B = -1;   // (e->wav takes the batches, without a batch layout)
  FBCHK(e->wav.ensure(sizeof(int16_t) * N * rows));
  FBCHK(e->fg_look.ensure(sizeof(double) * foreign_look_doubles(fr->rows_max, fr->S)));
  fr->look.resize(foreign_look_doubles(fr->rows_max, fr->S));
  FBCHK(ensure_identity_znorm(e));
  const bool dev = v->mode == FB_VICTIM_DEVICE_SCORES;
  e->foreign = fb_foreign_path_info{};
  e->foreign.path = dev ? FB_FOREIGN_DEV : FB_FOREIGN_HOST;
  e->foreign.x_dtype = dev ? v->dev->x_dtype : FB_DT_F64;
  e->foreign.score_dtype = dev ? v->dev->score_dtype : FB_DT_F64;
  e->foreign.launches_per_iter = v->mode == FB_VICTIM_HOST_DECISIONS ? 1 : 2;   // per batch: the conversion; k_decide_foreign or k_loss
  return FB_OK;
}
// The `rows` rows of e->wav as the victim's audio.  Device mode: in dev->x.  Host modes: *xh points at float64 [rows][N] in
// the staging arena (or in fr->spill beyond its size), valid until the next copy through the arena; the stream is idle.
static int foreign_hand_rows(fb_engine *e, FbForeignRun *fr, int rows, const double **xh) {
  const fb_victim *v = fr->v;
  if (v->mode == FB_VICTIM_DEVICE_SCORES) {
    fb_launch_rows_to_model(e->stream, v->dev->x_dtype, e->wav.as<int16_t>(), rows, fr->N, fr->bits, v->dev->x);
    return FB_OK;
  }
  fb_launch_rows_to_model(e->stream, FB_DT_F64, e->wav.as<int16_t>(), rows, fr->N, fr->bits, e->ext_x.p);
  const size_t xb = sizeof(double) * (size_t)fr->N * (size_t)rows;
  if (xb <= FB_PIN_MAX) {  // the callback reads the pinned staging area directly
    char *st = nullptr;
    FBCHK(pin_reserve(e, xb, &st));
    HIPCHK(hipMemcpyAsync(st, e->ext_x.p, xb, hipMemcpyDeviceToHost, e->stream));
    FBCHK(sync_stream(e));
    *xh = reinterpret_cast<const double *>(st);
  } else {
    fr->spill.resize((size_t)fr->N * (size_t)rows);
    FBCHK(sync_stream(e));
    HIPCHK(hipMemcpy(fr->spill.data(), e->ext_x.p, xb, hipMemcpyDeviceToHost));
    *xh = fr->spill.data();
  }
  e->foreign.batch_bytes_d2h += (int64_t)xb;
  return FB_OK;
}
// The score modes: the model scores the `rows` rows of e->wav; *sc is device memory [rows][S] of *dtype, in stream order.
static int foreign_scores(fb_engine *e, FbForeignRun *fr, int rows, const void **sc, int *dtype) {
  const fb_victim *v = fr->v;
  const double *xh = nullptr;
  FBCHK(foreign_hand_rows(e, fr, rows, &xh));
  e->foreign.model_calls += 1;
  if (v->mode == FB_VICTIM_DEVICE_SCORES) {
    const int rc = v->score_dev(v->ctx, (void *)e->stream, fr->N, rows, fr->S);
    if (rc != 0) {
      (void)sync_stream(e);  // (whatever the model did enqueue has finished when the caller sees the error)
      return fb_fail(FB_E_CALLBACK, "score callback failed (rc %d)", rc);
    }
    *sc = v->dev->scores;
    *dtype = v->dev->score_dtype;
    return FB_OK;
  }
  const size_t n = (size_t)rows * fr->S;
  const int rc = v->score(v->ctx, xh, fr->N, rows, fr->sc_h.data());
  if (rc != 0) return fb_fail(FB_E_CALLBACK, "score callback failed (rc %d)", rc);
  FBCHK(h2d(e, e->raw.p, fr->sc_h.data(), sizeof(double) * n));
  e->foreign.score_bytes_h2d += (int64_t)(sizeof(double) * n);
  *sc = e->raw.p;
  *dtype = FB_DT_F64;
  return FB_OK;
}
// The decisions of the `rows` rows of e->wav: dec[rows], and the model's scores[rows][S] (NaN where a decision callback wrote
// none; nullable).  One look.
static int foreign_decide(fb_engine *e, FbForeignRun *fr, int rows, int *dec, double *scores) {
  const fb_victim *v = fr->v;
  const int S = fr->S;
  if (v->mode == FB_VICTIM_HOST_DECISIONS) {
    const double *xh = nullptr;
    FBCHK(foreign_hand_rows(e, fr, rows, &xh));
    for (size_t i = 0; i < (size_t)rows * S; ++i) fr->sc_h[i] = std::numeric_limits<double>::quiet_NaN();
    for (int j = 0; j < rows; ++j) fr->dec_h[j] = -2;
    e->foreign.model_calls += 1;
    const int rc = v->decide(v->ctx, xh, fr->N, rows, fr->dec_h.data(), fr->sc_h.data());
    if (rc != 0) return fb_fail(FB_E_CALLBACK, "decide callback failed (rc %d)", rc);
    for (int j = 0; j < rows; ++j) {
      const int d = fr->dec_h[j];
      const bool ok = d == -2 || (fr->task == FB_TASK_SV ? (d == 1 || d == -1)
                                  : fr->task == FB_TASK_OSI ? (d >= -1 && d < S) : (d >= 0 && d < S));
      if (!ok) return fb_fail(FB_E_CALLBACK, "the decide callback returned %d for row %d: no decision of this task and not -2", d, j);
      dec[j] = d;
    }
    if (scores) memcpy(scores, fr->sc_h.data(), sizeof(double) * (size_t)rows * S);
    return FB_OK;
  }
  const void *sc = nullptr;
  int dtype = FB_DT_F64;
  FBCHK(foreign_scores(e, fr, rows, &sc, &dtype));
  int *dec_dev = e->fg_look.as<int>();
  double *sc_dev = e->fg_look.as<double>() + ((size_t)rows + 1) / 2;
  fb_launch_decide_foreign(e->stream, dtype, sc, rows, S, fr->task, fr->threshold, dec_dev, sc_dev);
  const size_t nd = foreign_look_doubles(rows, S);
  FBCHK(d2h(e, fr->look.data(), e->fg_look.p, sizeof(double) * nd));
  FBCHK(sync_stream(e));
  memcpy(dec, fr->look.data(), sizeof(int) * (size_t)rows);
  if (scores) memcpy(scores, fr->look.data() + ((size_t)rows + 1) / 2, sizeof(double) * (size_t)rows * S);
  return FB_OK;
}

static int check_pso_swarm(int P, double eps, double v_max, int bits) {
  if (P < 2 || P > FB_PSO_MAX_PARTICLES) return fb_fail(FB_E_ARG, "particles %d outside 2 .. %d", P, FB_PSO_MAX_PARTICLES);
  if (!isfinite(eps) || !(eps > 0.0)) return fb_fail(FB_E_ARG, "epsilon must be finite and > 0");
  if (!isfinite(v_max) || !(v_max > 0.0)) return fb_fail(FB_E_ARG, "v_max must be finite and > 0");
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  return FB_OK;
}
static int ensure_pso_buffers(fb_engine *e, int64_t N, int P) {
  FBCHK(e->audio.ensure(sizeof(double) * (size_t)N));
  FBCHK(e->pso_x.ensure(sizeof(double) * (size_t)N * P));
  FBCHK(e->pso_v.ensure(sizeof(double) * (size_t)N * P));
  FBCHK(e->pso_pb.ensure(sizeof(double) * (size_t)N * P));
  FBCHK(e->pso_gb.ensure(sizeof(double) * (size_t)N));
  return FB_OK;
}

// vic: null for the engine's own system (fb_attack_pso), else the foreign victim that scores the swarm (fb_attack_pso_foreign)
static int pso_attack(fb_engine *e, const fb_nes_params *p, const fb_pso_params *q, const fb_victim *vic, const double *audio,
                      int64_t N, int16_t *adv_i16, double *adv_f64, int *success, int *n_iters, double *trace, double *losses) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (!e || !p || !q || !audio || !adv_i16 || !success || !n_iters || !trace || !losses) return fb_fail(FB_E_ARG, "null argument");
  FbForeignRun fr;
  if (vic) FBCHK(foreign_setup(e, "fb_attack_pso_foreign", p, vic, N, q->particles, false, &fr));
  else if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  int R = 1, quorum = 1;   // replicas of every particle (fb_set_query_eot; the quorum is the decision-only attacks')
  if (!vic) FBCHK(query_replicas(e, "fb_attack_pso", &R, &quorum));
  const int P = q->particles, bits = nes_bits(p);
  FBCHK(check_pso_swarm(P, p->epsilon, q->v_max, bits));
  for (double c : {q->w_init, q->w_end, q->c1, q->c2})
    if (!isfinite(c) || c < 0.0) return fb_fail(FB_E_ARG, "w_init, w_end, c1 and c2 must be finite and >= 0");
  if (p->max_iter < 1) return fb_fail(FB_E_ARG, "max_iter must be > 0");
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  if (!vic && p->task != e->task) return fb_fail(FB_E_ARG, "params.task %d != engine system task %d", p->task, e->task);
  const int S = vic ? vic->S : fb_num_speakers(e);
  FBCHK(check_goal_params(p, S));
  if (!vic && num_frames(e->cfg, N) <= 0) return fb_fail(FB_E_ARG, "audio shorter than one frame");
  HIPCHK(hipSetDevice(e->device));
  if (vic) FBCHK(foreign_buffers(e, &fr));
  else if (R > 1) FBCHK(prepare_nes_replicas(e, N, P));
  else FBCHK(prepare_nes_batch(e, N, P));
  FBCHK(ensure_pso_buffers(e, N, P));
  // what the host reads once per iteration, in one block: k_loss's result block (for its "no voiced frames" word), loss[P],
  // scores[P][S]
  static_assert(sizeof(FbNesDev) % sizeof(double) == 0, "the result block is followed by doubles");
  const size_t out_d = sizeof(FbNesDev) / sizeof(double), look_d = out_d + (size_t)P + (size_t)P * S;
  FBCHK(e->pso_look.ensure(sizeof(double) * look_d));
  FbNesDev *out_dev = e->pso_look.as<FbNesDev>();
  double *loss_dev = e->pso_look.as<double>() + out_d, *scores_dev = loss_dev + P;
  FBCHK(launch_state_reset(e));
  e->iter_seconds.clear();

  double *x = e->pso_x.as<double>(), *gb = e->pso_gb.as<double>();
  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  if (R > 1) cast_a0(e, p, e->audio.as<double>(), N);
  fb_launch_pso_init(e->stream, e->audio.as<double>(), N, P, p->epsilon, q->v_max, p->seed, p->stream, bits, x,
                     e->pso_v.as<double>(), e->wav.as<int16_t>());
  std::vector<double> look(look_d), pl((size_t)P, 0.0);
  const double *l = look.data() + out_d, *sc = l + P;
  double gl = 0.0;
  int g = 0, k = 0, g_new = -1;
  auto t_prev = std::chrono::steady_clock::now();
  for (;; ++k) {
    FbScoreCall call{FbRngPoint{p->seed, p->stream, (uint32_t)k, 0}};
    if (vic) {   // the model's scores are final: loss_fn on them as fb_attack_ext / fb_attack_dev form it
      const void *fsc = nullptr;
      int dtype = FB_DT_F64;
      FBCHK(foreign_scores(e, &fr, P, &fsc, &dtype));
      if (dtype == FB_DT_F32)
        fb_launch_loss(e->stream, static_cast<const float *>(fsc), nullptr, P, S, p->task, 1, p->attack_type, e->ext_z.as<double>(),
                       e->ext_z.as<double>() + 64, p->threshold, p->adver_thresh, p->target, p->true_label, nullptr, 0, scores_dev,
                       loss_dev, out_dev);
      else
        fb_launch_loss(e->stream, static_cast<const double *>(fsc), nullptr, P, S, p->task, 1, p->attack_type, e->ext_z.as<double>(),
                       e->ext_z.as<double>() + 64, p->threshold, p->adver_thresh, p->target, p->true_label, nullptr, 0, scores_dev,
                       loss_dev, out_dev);
    } else if (R > 1) {   // every particle under R replicas: l_p and its score row are fb_set_eot's means (k_loss_eot)
      call.eot = e->eot;
      call.K = e->comp_K1 + 1;
      FBCHK(run_scoring(e, call, P * R, e->h_frame_off[P * R]));
      fb_launch_loss_eot(e->stream, e->raw.as<double>(), e->tv.as<int>(), P, R, e->n_out, p->task, e->kind, p->attack_type,
                         e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, p->adver_thresh, p->target, p->true_label,
                         nullptr, 0, e->eot_sc.as<double>(), e->eot_l.as<double>(), scores_dev, loss_dev, out_dev, nullptr,
                         nullptr, 0);
    } else {
      FBCHK(run_scoring(e, call, P, e->h_frame_off[P]));
      fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), P, e->n_out, p->task, e->kind, p->attack_type,
                     e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, p->adver_thresh, p->target, p->true_label,
                     nullptr, 0, scores_dev, loss_dev, out_dev);
    }
    // the one look of the iteration: one copy through pinned memory, one synchronisation
    FBCHK(d2h(e, look.data(), e->pso_look.p, sizeof(double) * look_d));
    FBCHK(sync_stream(e));
    {
      FbNesDev out;
      memcpy(&out, look.data(), sizeof(out));
      if (out.err != 0) return fb_fail(FB_E_NO_VOICED, "particle %d of iteration %d has no voiced frames", out.err - 1, k);
    }
    // step 2: personal bests (strict <), then the global best -- the lowest particle among the minimal ones
    unsigned long long improved = 0;
    int n_improved = 0;
    for (int b = 0; b < P; ++b) {
      losses[(size_t)k * P + b] = l[b];
      if (k == 0 || l[b] < pl[b]) {
        pl[b] = l[b];
        improved |= 1ull << b;
        ++n_improved;
      }
    }
    int gs = 0;
    for (int b = 1; b < P; ++b) if (pl[b] < pl[gs]) gs = b;
    double *row = trace + (size_t)k * (3 + S);
    g_new = -1;
    if (k == 0 || pl[gs] < gl) {
      gl = pl[gs];
      g = g_new = gs;
      for (int s = 0; s < S; ++s) row[3 + s] = sc[(size_t)gs * S + s];
    } else {
      for (int s = 0; s < S; ++s) row[3 + s] = row[3 + s - (3 + S)];  // gs unchanged: the previous row's
    }
    row[0] = gl; row[1] = (double)g; row[2] = (double)n_improved;
    const auto t_now = std::chrono::steady_clock::now();
    e->iter_seconds.push_back(std::chrono::duration<double>(t_now - t_prev).count());
    t_prev = t_now;
    if (gl < 0.0) { *success = 1; break; }
    if (k == p->max_iter - 1) { *success = -1; break; }
    const double w_k = q->w_init - ((q->w_init - q->w_end) * (double)k) / (double)p->max_iter;
    fb_launch_pso_step(e->stream, e->audio.as<double>(), N, P, p->epsilon, x, e->pso_v.as<double>(), e->pso_pb.as<double>(), gb,
                       improved, g_new, w_k, q->c1, q->c2, q->v_max, p->seed, p->stream, (uint32_t)(k + 1), bits,
                       e->wav.as<int16_t>());
  }
  *n_iters = k + 1;
  // the last iteration's new global best has not been copied yet: that rides in the step that was not launched
  if (g_new >= 0)
    HIPCHK(hipMemcpyAsync(gb, x + (size_t)g_new * N, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, e->stream));
  fb_launch_quantize(e->stream, gb, N, bits, e->wav.as<int16_t>());
  FBCHK(d2h(e, adv_i16, e->wav.p, sizeof(int16_t) * (size_t)N));
  if (adv_f64) FBCHK(d2h(e, adv_f64, gb, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_attack_pso(fb_engine *e, const fb_nes_params *p, const fb_pso_params *q, const double *audio, int64_t N,
                             int16_t *adv_i16, double *adv_f64, int *success, int *n_iters, double *trace, double *losses) {
  return pso_attack(e, p, q, nullptr, audio, N, adv_i16, adv_f64, success, n_iters, trace, losses);
}
extern "C" int fb_attack_pso_foreign(fb_engine *e, const fb_nes_params *p, const fb_pso_params *q, const fb_victim *v,
                                     const double *audio, int64_t N, int16_t *adv_i16, double *adv_f64, int *success, int *n_iters,
                                     double *trace, double *losses) {
  if (!e || !p || !q || !v) return fb_fail(FB_E_ARG, "null argument (the victim descriptor included)");
  return pso_attack(e, p, q, v, audio, N, adv_i16, adv_f64, success, n_iters, trace, losses);
}

extern "C" int fb_debug_pso_init(fb_engine *e, const double *audio, int64_t N, double epsilon, int P, double v_max, uint64_t seed,
                                 uint32_t stream, int bits, double *x, double *v, int16_t *q) {
  if (!e || !audio || !x || !v || !q || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_pso_swarm(P, epsilon, v_max, bits));
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the batch, without a batch layout)
  const size_t n = (size_t)N * P;
  FBCHK(ensure_pso_buffers(e, N, P));
  FBCHK(e->wav.ensure(sizeof(int16_t) * n));
  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  fb_launch_pso_init(e->stream, e->audio.as<double>(), N, P, epsilon, v_max, seed, stream, bits, e->pso_x.as<double>(),
                     e->pso_v.as<double>(), e->wav.as<int16_t>());
  FBCHK(d2h(e, x, e->pso_x.p, sizeof(double) * n));
  FBCHK(d2h(e, v, e->pso_v.p, sizeof(double) * n));
  FBCHK(d2h(e, q, e->wav.p, sizeof(int16_t) * n));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_debug_pso_step(fb_engine *e, const double *audio, int64_t N, double epsilon, int P, const double *x,
                                 const double *v, const double *pb, const double *gb, const int *improved, int g_new, double w,
                                 double c1, double c2, double v_max, uint64_t seed, uint32_t stream, uint32_t t, int bits,
                                 double *x_out, double *v_out, double *pb_out, double *gb_out, int16_t *q_out) {
  if (!e || !audio || !x || !v || !pb || !gb || !improved || !x_out || !v_out || !pb_out || !gb_out || !q_out || N <= 0)
    return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_pso_swarm(P, epsilon, v_max, bits));
  if (g_new < -1 || g_new >= P) return fb_fail(FB_E_ARG, "g_new %d outside -1 .. %d", g_new, P - 1);
  for (double c : {w, c1, c2})
    if (!isfinite(c) || c < 0.0) return fb_fail(FB_E_ARG, "w, c1 and c2 must be finite and >= 0");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  const size_t n = (size_t)N * P;
  FBCHK(ensure_pso_buffers(e, N, P));
  FBCHK(e->wav.ensure(sizeof(int16_t) * n));
  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->pso_x.p, x, sizeof(double) * n));
  FBCHK(h2d(e, e->pso_v.p, v, sizeof(double) * n));
  FBCHK(h2d(e, e->pso_pb.p, pb, sizeof(double) * n));
  FBCHK(h2d(e, e->pso_gb.p, gb, sizeof(double) * (size_t)N));
  unsigned long long mask = 0;
  for (int b = 0; b < P; ++b) if (improved[b]) mask |= 1ull << b;
  fb_launch_pso_step(e->stream, e->audio.as<double>(), N, P, epsilon, e->pso_x.as<double>(), e->pso_v.as<double>(),
                     e->pso_pb.as<double>(), e->pso_gb.as<double>(), mask, g_new, w, c1, c2, v_max, seed, stream, t, bits,
                     e->wav.as<int16_t>());
  FBCHK(d2h(e, x_out, e->pso_x.p, sizeof(double) * n));
  FBCHK(d2h(e, v_out, e->pso_v.p, sizeof(double) * n));
  FBCHK(d2h(e, pb_out, e->pso_pb.p, sizeof(double) * n));
  FBCHK(d2h(e, gb_out, e->pso_gb.p, sizeof(double) * (size_t)N));
  FBCHK(d2h(e, q_out, e->wav.p, sizeof(int16_t) * n));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// ------------------------------------------------- decision-only attack
// fb_attack_kenansville (the "decision-only attack" section of fakebob_hip.h).  k_kv_analyse runs once; every round
// k_kv_candidates writes the round's rows into the NES batch, the ordinary path scores them, k_loss forms scores[rows][S],
// and the host reads them with tv[rows] once, decides and narrows the bracket.  The fused finalisation, the i-vector
// tail-loss shortcut and the device control block are not used.
static int check_kv_tables(int W, const int32_t *tab) {
  if (W < FB_KV_MIN_WINDOW || W > FB_KV_MAX_WINDOW)
    return fb_fail(FB_E_ARG, "window %d outside %d .. %d", W, FB_KV_MIN_WINDOW, FB_KV_MAX_WINDOW);
  if (!tab) return fb_fail(FB_E_ARG, "null tables");
  if (tab[0] != (1 << 30) || tab[W] != 0 || tab[2 * W] != (1 << 22) || tab[3 * W] != 0)
    return fb_fail(FB_E_ARG, "the tables do not start with CF[0] = 2^30, SF[0] = 0, CI[0] = 2^22, SI[0] = 0");
  return FB_OK;
}
// the tables and the analysis buffers of N samples in windows of W, the tables uploaded
static int prepare_kv(fb_engine *e, int64_t N, int W, const int32_t *tab) {
  const size_t nw = (size_t)((N + W - 1) / W), K = (size_t)W / 2 + 1;
  FBCHK(e->kv_x.ensure(sizeof(int16_t) * (size_t)N));
  FBCHK(e->kv_best.ensure(sizeof(int16_t) * (size_t)N));
  FBCHK(e->kv_tab.ensure(sizeof(int32_t) * 4 * (size_t)W));
  FBCHK(e->kv_ma.ensure(sizeof(int32_t) * nw * K));
  FBCHK(e->kv_mb.ensure(sizeof(int32_t) * nw * K));
  FBCHK(e->kv_cum.ensure(sizeof(long long) * nw * K));
  FBCHK(e->kv_E.ensure(sizeof(long long) * nw));
  FBCHK(h2d(e, e->kv_tab.p, tab, sizeof(int32_t) * 4 * (size_t)W));
  return FB_OK;
}
static void launch_kv_analyse(fb_engine *e, int64_t N, int W) {
  fb_launch_kv_analyse(e->stream, e->kv_x.as<int16_t>(), N, W, e->kv_tab.as<int32_t>(), e->kv_ma.as<int32_t>(),
                       e->kv_mb.as<int32_t>(), e->kv_cum.as<long long>(), e->kv_E.as<long long>());
}
static void launch_kv_candidates(fb_engine *e, int64_t N, int W, int rows, const int *q, int16_t *out) {
  fb_launch_kv_candidates(e->stream, e->kv_x.as<int16_t>(), N, W, rows, q, e->kv_tab.as<int32_t>(), e->kv_ma.as<int32_t>(),
                          e->kv_mb.as<int32_t>(), e->kv_cum.as<long long>(), e->kv_E.as<long long>(), out);
}

// vic: null for the engine's own system, else the foreign victim that decides the candidates (fb_attack_kenansville_foreign)
static int kv_attack(fb_engine *e, const fb_nes_params *p, const fb_kv_params *k, const fb_victim *vic, const int32_t *tables,
                     const double *audio, int64_t N, int16_t *adv_i16, int *success, int *factor, int *n_queries, int *n_rounds,
                     int *qs, int *decisions, double *scores, int *trace) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (!e || !p || !k || !audio || !adv_i16 || !success || !factor || !n_queries || !n_rounds || !qs || !decisions || !scores || !trace)
    return fb_fail(FB_E_ARG, "null argument");
  FbForeignRun fr;
  if (vic) FBCHK(foreign_setup(e, "fb_attack_kenansville_foreign", p, vic, N, k->grid, true, &fr));
  else if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  int R = 1, quorum = 1;   // replicas of every candidate row and the votes a row needs (fb_set_query_eot)
  if (!vic) FBCHK(query_replicas(e, "fb_attack_kenansville", &R, &quorum));
  const int W = k->window, G = k->grid, bits = nes_bits(p);
  FBCHK(check_kv_tables(W, tables));
  if (G < 1 || G > FB_KV_MAX_ROWS) return fb_fail(FB_E_ARG, "grid %d outside 1 .. %d", G, FB_KV_MAX_ROWS);
  if (k->q_max < 1 || k->q_max > 65536) return fb_fail(FB_E_ARG, "q_max %d outside 1 .. 65536", k->q_max);
  if (k->max_rounds < 1 || k->max_rounds > FB_KV_MAX_ROUNDS) return fb_fail(FB_E_ARG, "max_rounds %d outside 1 .. %d", k->max_rounds, FB_KV_MAX_ROUNDS);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  if (!vic && p->task != e->task) return fb_fail(FB_E_ARG, "params.task %d != engine system task %d", p->task, e->task);
  if (p->task != FB_TASK_SV && p->task != FB_TASK_OSI && p->task != FB_TASK_CSI) return fb_fail(FB_E_ARG, "bad task %d", p->task);
  if (p->attack_type != FB_TARGETED && p->attack_type != FB_UNTARGETED) return fb_fail(FB_E_ARG, "bad attack_type %d", p->attack_type);
  const int S = vic ? vic->S : fb_num_speakers(e);
  const bool targeted = p->attack_type == FB_TARGETED;
  const int label = targeted ? p->target : p->true_label;   // a decision value
  {
    const bool ok = p->task == FB_TASK_SV ? (label == 1 || label == -1)
                  : p->task == FB_TASK_OSI ? (label >= -1 && label < S) : (label >= 0 && label < S);
    if (!ok) return fb_fail(FB_E_ARG, "%s %d is no decision of this system", targeted ? "target" : "true label", label);
  }
  if (!vic && num_frames(e->cfg, N) <= 0) return fb_fail(FB_E_ARG, "audio shorter than one frame");
  HIPCHK(hipSetDevice(e->device));
  if (vic) FBCHK(foreign_buffers(e, &fr));
  FBCHK(e->audio.ensure(sizeof(double) * (size_t)N));
  FBCHK(prepare_kv(e, N, W, tables));
  // what the host reads once per round, in one block: k_loss's result block (not read), loss[G] (not read), scores[G][S], tv[G]
  static_assert(sizeof(FbNesDev) % sizeof(double) == 0, "the result block is followed by doubles");
  const size_t out_d = sizeof(FbNesDev) / sizeof(double), sc_d = out_d + (size_t)G, tv_d = sc_d + (size_t)G * S;
  const size_t look_d = tv_d + ((size_t)G + 1) / 2;
  FBCHK(e->kv_look.ensure(sizeof(double) * look_d));
  FbNesDev *out_dev = e->kv_look.as<FbNesDev>();
  double *loss_dev = e->kv_look.as<double>() + out_d, *scores_dev = e->kv_look.as<double>() + sc_d;
  int *tv_dev = reinterpret_cast<int *>(e->kv_look.as<double>() + tv_d);
  if (R > 1) {   // the replicated batch of a full round and k_vote's look block in place of k_loss's
    FBCHK(prepare_nes_replicas(e, N, G));
    FBCHK(e->vote_look.ensure(vote_look_bytes(G, S)));
  }
  FBCHK(launch_state_reset(e));
  e->iter_seconds.clear();

  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  fb_launch_quantize(e->stream, e->audio.as<double>(), N, bits, e->kv_x.as<int16_t>());
  if (R > 1) cast_a0(e, p, e->audio.as<double>(), N);   // (a_0 = x)
  launch_kv_analyse(e, N, W);
  std::vector<double> look(std::max(look_d, vote_look_bytes(G, S) / sizeof(double)));
  const double *sc = look.data() + sc_d;
  std::vector<int> cand;
  cand.reserve(G);
  int lo = 0, hi = -1, r = 0, queries = 0;
  *success = -1;
  auto t_prev = std::chrono::steady_clock::now();
  for (;; ++r) {
    // the round's candidates, ascending
    cand.clear();
    bool last = false;
    if (r == 0) {
      for (int j = 0; j < G; ++j) {
        const int qj = (int)(((long long)(j + 1) * k->q_max) / G);
        if (qj > 0 && (cand.empty() || qj != cand.back())) cand.push_back(qj);
      }
    } else {
      const int d = hi - lo;
      if (d - 1 <= G) {
        for (int qj = lo + 1; qj < hi; ++qj) cand.push_back(qj);
        last = true;
      } else {
        for (int j = 0; j < G; ++j) cand.push_back(lo + (int)(((long long)(j + 1) * d) / (G + 1)));
      }
    }
    const int rows = (int)cand.size();
    if (vic) {}   // (e->wav holds a full round's rows: foreign_buffers)
    else if (R > 1) FBCHK(prepare_nes_replicas(e, N, rows));
    else FBCHK(prepare_nes_batch(e, N, rows));
    launch_kv_candidates(e, N, W, rows, cand.data(), e->wav.as<int16_t>());
    FbScoreCall call{FbRngPoint{p->seed, p->stream, (uint32_t)r, 0}};
    int first = -1;   // the smallest succeeding candidate's row
    for (int j = 0; j < G; ++j) qs[(size_t)r * G + j] = j < rows ? cand[j] : -1;
    if (vic) {   // the model's decisions, or the rule on its scores: one look
      if (rows > 0) FBCHK(foreign_decide(e, &fr, rows, decisions + (size_t)r * G, scores + (size_t)r * G * S));
      for (int j = 0; j < rows && first < 0; ++j) {
        const int d = decisions[(size_t)r * G + j];
        if (d != -2 && (targeted ? d == label : d != label)) first = j;
      }
    } else if (R > 1) {
      call.eot = e->eot;
      call.K = e->comp_K1 + 1;
      FBCHK(run_scoring(e, call, rows * R, e->h_frame_off[rows * R]));
      launch_vote(e, p, rows, R, targeted, label);
      // the one look of the round: the votes and the mean scores, nothing per replica
      const FbVoteLook v = vote_look_at(look.data(), rows, S);
      FBCHK(d2h(e, look.data(), e->vote_look.p, v.bytes));
      FBCHK(sync_stream(e));
      for (int j = 0; j < rows; ++j) {
        for (int m = 0; m < S; ++m) scores[((size_t)r * G + j) * S + m] = v.mean[(size_t)j * S + m];
        decisions[(size_t)r * G + j] = v.votes[j];   // the row's vote
        if (v.votes[j] >= quorum && first < 0) first = j;
      }
    } else {
      FBCHK(run_scoring(e, call, rows, e->h_frame_off[rows]));
      // (k_loss is here for the system scores of fb_loss_row alone: its loss and its labels are not this attack's)
      fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), rows, e->n_out, p->task, e->kind, FB_UNTARGETED,
                     e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, 0.0, 0, 0, nullptr, 0, scores_dev, loss_dev, out_dev);
      HIPCHK(hipMemcpyAsync(tv_dev, e->tv.p, sizeof(int) * (size_t)rows, hipMemcpyDeviceToDevice, e->stream));
      // the one look of the round: one copy through pinned memory, one synchronisation
      FBCHK(d2h(e, look.data(), e->kv_look.p, sizeof(double) * look_d));
      FBCHK(sync_stream(e));
      const int *tv = reinterpret_cast<const int *>(look.data() + tv_d);
      for (int j = 0; j < rows; ++j) {
        const double *s = sc + (size_t)j * S;
        for (int m = 0; m < S; ++m) scores[((size_t)r * G + j) * S + m] = s[m];
        int d;
        if (tv[j] <= 0) {
          d = -2;   // no voiced frames: no decision
        } else if (p->task == FB_TASK_SV) {
          d = s[0] >= p->threshold ? 1 : -1;
        } else {
          int am = 0;
          for (int m = 1; m < S; ++m) if (s[m] > s[am]) am = m;   // the first maximum
          d = (p->task == FB_TASK_OSI && s[am] < p->threshold) ? -1 : am;
        }
        decisions[(size_t)r * G + j] = d;
        const bool ok = d != -2 && (targeted ? d == label : d != label);
        if (ok && first < 0) first = j;
      }
    }
    queries += rows * R;
    if (first >= 0) {
      hi = cand[first];
      // the candidate of hi is a row that was scored: kept before the next round's batch takes its place
      HIPCHK(hipMemcpyAsync(e->kv_best.p, e->wav.as<int16_t>() + (size_t)first * N, sizeof(int16_t) * (size_t)N,
                            hipMemcpyDeviceToDevice, e->stream));
      if (first > 0) lo = cand[first - 1];
    } else if (hi >= 0 && rows > 0) {
      lo = cand[rows - 1];
    }
    trace[3 * r] = lo; trace[3 * r + 1] = hi; trace[3 * r + 2] = rows * R;
    const auto t_now = std::chrono::steady_clock::now();
    e->iter_seconds.push_back(std::chrono::duration<double>(t_now - t_prev).count());
    t_prev = t_now;
    if (hi < 0) break;   // nothing succeeded in round 0
    if (hi - lo == 1 || last || r == k->max_rounds - 1) break;
  }
  *n_rounds = r + 1;
  *n_queries = queries;
  *success = hi >= 0 ? 1 : -1;
  *factor = hi;
  FBCHK(d2h(e, adv_i16, hi >= 0 ? e->kv_best.p : e->kv_x.p, sizeof(int16_t) * (size_t)N));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_attack_kenansville(fb_engine *e, const fb_nes_params *p, const fb_kv_params *k, const int32_t *tables,
                                     const double *audio, int64_t N, int16_t *adv_i16, int *success, int *factor,
                                     int *n_queries, int *n_rounds, int *qs, int *decisions, double *scores, int *trace) {
  return kv_attack(e, p, k, nullptr, tables, audio, N, adv_i16, success, factor, n_queries, n_rounds, qs, decisions, scores, trace);
}
extern "C" int fb_attack_kenansville_foreign(fb_engine *e, const fb_nes_params *p, const fb_kv_params *k, const fb_victim *v,
                                             const int32_t *tables, const double *audio, int64_t N, int16_t *adv_i16, int *success,
                                             int *factor, int *n_queries, int *n_rounds, int *qs, int *decisions, double *scores,
                                             int *trace) {
  if (!e || !p || !k || !v) return fb_fail(FB_E_ARG, "null argument (the victim descriptor included)");
  return kv_attack(e, p, k, v, tables, audio, N, adv_i16, success, factor, n_queries, n_rounds, qs, decisions, scores, trace);
}

extern "C" int fb_debug_kv_analyse(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, int32_t *a,
                                   int32_t *b, int64_t *cum, int64_t *E) {
  if (!e || !x || !a || !b || !cum || !E || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_kv_tables(W, tables));
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  FBCHK(prepare_kv(e, N, W, tables));
  FBCHK(h2d(e, e->kv_x.p, x, sizeof(int16_t) * (size_t)N));
  launch_kv_analyse(e, N, W);
  const size_t nw = (size_t)((N + W - 1) / W), K = (size_t)W / 2 + 1;
  FBCHK(d2h(e, a, e->kv_ma.p, sizeof(int32_t) * nw * K));
  FBCHK(d2h(e, b, e->kv_mb.p, sizeof(int32_t) * nw * K));
  FBCHK(d2h(e, cum, e->kv_cum.p, sizeof(int64_t) * nw * K));
  FBCHK(d2h(e, E, e->kv_E.p, sizeof(int64_t) * nw));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  // the device keeps m a and m b; the hook hands out a and b
  for (size_t w = 0; w < nw; ++w)
    for (size_t kb = 0; kb < K; ++kb)
      if (!(kb == 0 || (W % 2 == 0 && kb == (size_t)W / 2))) {
        a[w * K + kb] /= 2;
        b[w * K + kb] /= 2;
      }
  return FB_OK;
}

extern "C" int fb_debug_kv_candidates(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, const int *q,
                                      int rows, int16_t *y) {
  if (!e || !x || !q || !y || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_kv_tables(W, tables));
  if (rows < 1 || rows > FB_KV_MAX_ROWS) return fb_fail(FB_E_ARG, "rows %d outside 1 .. %d", rows, FB_KV_MAX_ROWS);
  for (int j = 0; j < rows; ++j)
    if (q[j] < 0 || q[j] > 65536) return fb_fail(FB_E_ARG, "factor %d outside 0 .. 65536", q[j]);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the batch, without a batch layout)
  FBCHK(prepare_kv(e, N, W, tables));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * rows));
  FBCHK(h2d(e, e->kv_x.p, x, sizeof(int16_t) * (size_t)N));
  launch_kv_analyse(e, N, W);
  launch_kv_candidates(e, N, W, rows, q, e->wav.as<int16_t>());
  FBCHK(d2h(e, y, e->wav.p, sizeof(int16_t) * (size_t)N * rows));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// tools/kenansville_rate.py: `reps` launches of each kernel between two events, after one of each to warm up
extern "C" int fb_bench_kv_kernels(fb_engine *e, const int16_t *x, int64_t N, int W, const int32_t *tables, const int *q, int rows,
                                   int reps, double *ms /*[2]: analysis, candidates -- per launch*/) {
  if (!e || !x || !q || !ms || N <= 0 || reps < 1) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_kv_tables(W, tables));
  if (rows < 1 || rows > FB_KV_MAX_ROWS) return fb_fail(FB_E_ARG, "rows %d outside 1 .. %d", rows, FB_KV_MAX_ROWS);
  for (int j = 0; j < rows; ++j)
    if (q[j] < 0 || q[j] > 65536) return fb_fail(FB_E_ARG, "factor %d outside 0 .. 65536", q[j]);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the batch, without a batch layout)
  FBCHK(prepare_kv(e, N, W, tables));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * rows));
  FBCHK(h2d(e, e->kv_x.p, x, sizeof(int16_t) * (size_t)N));
  launch_kv_analyse(e, N, W);
  launch_kv_candidates(e, N, W, rows, q, e->wav.as<int16_t>());
  for (int which = 0; which < 2; ++which) {
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; ++i) {
      if (which == 0) launch_kv_analyse(e, N, W);
      else launch_kv_candidates(e, N, W, rows, q, e->wav.as<int16_t>());
    }
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
    ms[which] = (double)t / reps;
  }
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// ------------------------------------------------- decision-only attack II: HopSkipJump
// fb_attack_hsj (the "decision-only attack II" section of fakebob_hip.h).  Every batch -- a search round (k_hsj_line), an
// iteration's probes (k_hsj_probes), its step sizes (k_hsj_step) -- goes as int16 rows into the NES batch, the ordinary path
// scores it, k_loss forms scores[rows][S], and the host reads them with tv[rows] once, as fb_attack_kenansville does.
static int check_hsj_params(const fb_hsj_params *k) {
  if (k->grid < 1 || k->grid > FB_HSJ_MAX_GRID) return fb_fail(FB_E_ARG, "grid %d outside 1 .. %d", k->grid, FB_HSJ_MAX_GRID);
  if (k->max_rounds < 1 || k->max_rounds > FB_HSJ_MAX_ROUNDS)
    return fb_fail(FB_E_ARG, "max_rounds %d outside 1 .. %d", k->max_rounds, FB_HSJ_MAX_ROUNDS);
  if (k->num_evals_init < 1 || k->num_evals_init > k->num_evals_max || k->num_evals_max > FB_HSJ_MAX_EVALS)
    return fb_fail(FB_E_ARG, "num_evals %d : %d outside 1 <= init <= max <= %d", k->num_evals_init, k->num_evals_max, FB_HSJ_MAX_EVALS);
  if (k->max_queries < 0) return fb_fail(FB_E_ARG, "max_queries %d < 0", k->max_queries);
  if (!std::isfinite(k->sigma_min) || !(k->sigma_min > 0.0)) return fb_fail(FB_E_ARG, "sigma_min must be finite and > 0");
  if (!std::isfinite(k->probe_scale) || !(k->probe_scale >= 0.0)) return fb_fail(FB_E_ARG, "probe_scale must be finite and >= 0");
  return FB_OK;
}
// B_t = min(num_evals_max, isqrt(num_evals_init^2 t))
static int hsj_evals(const fb_hsj_params *k, int t) {
  const long long n = (long long)k->num_evals_init * k->num_evals_init * t;
  long long r = (long long)std::sqrt((double)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return (int)std::min<long long>(r, k->num_evals_max);
}
extern "C" long long fb_hsj_max_rows(int max_iter, const fb_hsj_params *k) {
  if (!k || max_iter < 0 || check_hsj_params(k) != FB_OK) return -1;
  const long long G = k->grid, search = G * k->max_rounds;
  long long total = search;
  for (int t = 1; t <= max_iter; ++t) total += hsj_evals(k, t) + G + search;
  if (k->max_queries > 0) total = std::min(total, std::max<long long>(k->max_queries, G));
  return total;
}
// the buffers of N samples and of batches of up to max_rows rows
static int prepare_hsj(fb_engine *e, int64_t N, int max_rows) {
  const size_t n = (size_t)N;
  FBCHK(e->audio.ensure(sizeof(double) * n));
  FBCHK(e->hsj_init.ensure(sizeof(double) * n));
  FBCHK(e->hsj_y.ensure(sizeof(double) * n));
  FBCHK(e->hsj_x.ensure(sizeof(double) * n));
  FBCHK(e->hsj_v.ensure(sizeof(double) * n));
  FBCHK(e->hsj_part.ensure(sizeof(double) * (size_t)fb_hsj_chunks(N)));
  FBCHK(e->hsj_sc.ensure(sizeof(double) * 2));
  FBCHK(e->hsj_w.ensure(sizeof(int32_t) * FB_HSJ_MAX_EVALS));
  FBCHK(e->hsj_best.ensure(sizeof(int16_t) * n));
  (void)max_rows;
  return FB_OK;
}
// the adopt launch and the sum of its partials: x = line(y, q), hsj_sc[0] = ssq(x - a)
static void launch_hsj_adopt(fb_engine *e, const double *y, int64_t N, int q) {
  fb_launch_hsj_adopt(e->stream, e->audio.as<double>(), y, N, q, e->hsj_x.as<double>(), e->hsj_part.as<double>());
  fb_launch_hsj_sum(e->stream, e->hsj_part.as<double>(), fb_hsj_chunks(N), e->hsj_sc.as<double>());
}
// the direction launch and the sum of its partials: v = sum_j w_j z_j, hsj_sc[1] = ssq(v)
static void launch_hsj_dir(fb_engine *e, int B, int64_t N, uint64_t seed, uint32_t stream, uint32_t t, const float *zkept) {
  fb_launch_hsj_dir(e->stream, e->hsj_w.as<int32_t>(), B, N, seed, stream, t, zkept, e->hsj_v.as<double>(), e->hsj_part.as<double>());
  fb_launch_hsj_sum(e->stream, e->hsj_part.as<double>(), fb_hsj_chunks(N), e->hsj_sc.as<double>() + 1);
}

// vic: null for the engine's own system, else the foreign victim that decides every row (fb_attack_hsj_foreign)
static int hsj_attack(fb_engine *e, const fb_nes_params *p, const fb_hsj_params *k, const fb_victim *vic, const double *audio,
                      const double *init, int64_t N, int16_t *adv_i16, double *adv_f64, int *success, double *dist2, int *n_iters,
                      int *n_queries, double *trace, int *decisions, long long decisions_cap, double *x_trace) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (!e || !p || !k || !audio || !adv_i16 || !success || !dist2 || !n_iters || !n_queries || !trace || !decisions)
    return fb_fail(FB_E_ARG, "null argument");
  if (!init) return fb_fail(FB_E_ARG, "null init: HopSkipJump starts from an audio that is already decided as wanted");
  FbForeignRun fr;
  if (vic) FBCHK(foreign_setup(e, "fb_attack_hsj_foreign", p, vic, N, std::max(k->grid, k->num_evals_max), true, &fr));
  else if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  int R = 1, quorum = 1;   // replicas of every candidate row and the votes a row needs (fb_set_query_eot)
  if (!vic) FBCHK(query_replicas(e, "fb_attack_hsj", &R, &quorum));
  FBCHK(check_hsj_params(k));
  const int G = k->grid, bits = nes_bits(p);
  if (p->max_iter < 0) return fb_fail(FB_E_ARG, "max_iter %d < 0", p->max_iter);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  if (N <= 0) return fb_fail(FB_E_ARG, "empty audio");
  if (!vic && p->task != e->task) return fb_fail(FB_E_ARG, "params.task %d != engine system task %d", p->task, e->task);
  if (p->task != FB_TASK_SV && p->task != FB_TASK_OSI && p->task != FB_TASK_CSI) return fb_fail(FB_E_ARG, "bad task %d", p->task);
  if (p->attack_type != FB_TARGETED && p->attack_type != FB_UNTARGETED) return fb_fail(FB_E_ARG, "bad attack_type %d", p->attack_type);
  const int S = vic ? vic->S : fb_num_speakers(e);
  const bool targeted = p->attack_type == FB_TARGETED;
  const int label = targeted ? p->target : p->true_label;   // a decision value
  {
    const bool ok = p->task == FB_TASK_SV ? (label == 1 || label == -1)
                  : p->task == FB_TASK_OSI ? (label >= -1 && label < S) : (label >= 0 && label < S);
    if (!ok) return fb_fail(FB_E_ARG, "%s %d is no decision of this system", targeted ? "target" : "true label", label);
  }
  if (!vic && num_frames(e->cfg, N) <= 0) return fb_fail(FB_E_ARG, "audio shorter than one frame");
  const long long need = fb_hsj_max_rows(p->max_iter, k);
  if (decisions_cap < need)
    return fb_fail(FB_E_ARG, "the decision log holds %lld entries, this call may score %lld rows", decisions_cap, need);
  HIPCHK(hipSetDevice(e->device));
  const int max_rows = std::max(G, k->num_evals_max);
  if (R > 1) {   // the largest replicated batch, checked before anything is scored; k_vote's look block
    if ((int64_t)max_rows * R > 65535)
      return fb_fail(FB_E_LIMIT, "max(grid, num_evals_max) * utterances * eot = %lld rows: a scoring batch takes up to 65535",
                     (long long)max_rows * R);
    FBCHK(prepare_nes_replicas(e, N, max_rows));
    FBCHK(e->vote_look.ensure(vote_look_bytes(max_rows, S)));
  }
  if (vic) FBCHK(foreign_buffers(e, &fr));
  FBCHK(prepare_hsj(e, N, max_rows));
  // the probes launch keeps its normals as float32 [B][N] for the direction launch: at B = 1024, N = 48 000 the pair takes
  // 160 us so against 206 us with the direction launch drawing them again (tools/hsj_rate.py)
  FBCHK(e->hsj_z.ensure(sizeof(float) * (size_t)N * (size_t)k->num_evals_max));
  // what the host reads once per batch, in one block: k_loss's result block (not read), loss[R] (not read), scores[R][S], tv[R]
  static_assert(sizeof(FbNesDev) % sizeof(double) == 0, "the result block is followed by doubles");
  const size_t out_d = sizeof(FbNesDev) / sizeof(double), sc_d = out_d + (size_t)max_rows, tv_d = sc_d + (size_t)max_rows * S;
  const size_t look_d = tv_d + ((size_t)max_rows + 1) / 2;
  FBCHK(e->hsj_look.ensure(sizeof(double) * look_d));
  FbNesDev *out_dev = e->hsj_look.as<FbNesDev>();
  double *loss_dev = e->hsj_look.as<double>() + out_d, *scores_dev = e->hsj_look.as<double>() + sc_d;
  int *tv_dev = reinterpret_cast<int *>(e->hsj_look.as<double>() + tv_d);
  FBCHK(launch_state_reset(e));
  e->iter_seconds.clear();

  const double *a_dev = e->audio.as<double>();
  FBCHK(h2d(e, e->audio.p, audio, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->hsj_init.p, init, sizeof(double) * (size_t)N));
  if (R > 1) cast_a0(e, p, a_dev, N);
  std::vector<double> look(std::max(look_d, vote_look_bytes(max_rows, S) / sizeof(double)));
  std::vector<int> dec(max_rows), cand;
  cand.reserve(G);
  int queries = 0, logged = 0;   // victim queries (candidate rows * R) and entries of the decision log (candidate rows)
  uint32_t epoch = 0;
  bool stopped = false;   // max_queries: nothing is scored any more
  auto over = [&](int rows) { return k->max_queries > 0 && (long long)queries + (long long)rows * R > k->max_queries; };
  // the batch layout of `rows` candidate rows (under R replicas: of rows * R)
  // (a foreign victim: e->wav holds the largest batch already, foreign_buffers)
  auto layout = [&](int rows) -> int { return vic ? FB_OK : R > 1 ? prepare_nes_replicas(e, N, rows) : prepare_nes_batch(e, N, rows); };
  // scores the `rows` rows that stand in e->wav: dec[0 .. rows) and the log; one look
  auto score = [&](int rows) -> int {
    if (vic) {   // the model's decisions, or the rule on its scores: one look
      FBCHK(foreign_decide(e, &fr, rows, decisions + logged, nullptr));
      for (int j = 0; j < rows; ++j) {
        const int d = decisions[logged + j];
        dec[j] = (d != -2 && (targeted ? d == label : d != label)) ? 1 : 0;
      }
      logged += rows;
      queries += rows;
      return FB_OK;
    }
    FbScoreCall call{FbRngPoint{p->seed, p->stream, epoch++, 0}};
    if (R > 1) {   // R replicas of every row: the log holds the votes, a row is adversarial from `quorum` votes on
      call.eot = e->eot;
      call.K = e->comp_K1 + 1;
      FBCHK(run_scoring(e, call, rows * R, e->h_frame_off[rows * R]));
      launch_vote(e, p, rows, R, targeted, label);
      const FbVoteLook v = vote_look_at(look.data(), rows, S);
      FBCHK(d2h(e, look.data(), e->vote_look.p, v.bytes));
      FBCHK(sync_stream(e));
      for (int j = 0; j < rows; ++j) {
        decisions[logged + j] = v.votes[j];
        dec[j] = v.votes[j] >= quorum ? 1 : 0;
      }
      logged += rows;
      queries += rows * R;
      return FB_OK;
    }
    FBCHK(run_scoring(e, call, rows, e->h_frame_off[rows]));
    // (k_loss is here for the system scores of fb_loss_row alone: its loss and its labels are not this attack's)
    fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), rows, e->n_out, p->task, e->kind, FB_UNTARGETED,
                   e->zmean.as<double>(), e->zstd.as<double>(), p->threshold, 0.0, 0, 0, nullptr, 0, scores_dev, loss_dev, out_dev);
    HIPCHK(hipMemcpyAsync(tv_dev, e->tv.p, sizeof(int) * (size_t)rows, hipMemcpyDeviceToDevice, e->stream));
    FBCHK(d2h(e, look.data(), e->hsj_look.p, sizeof(double) * look_d));
    FBCHK(sync_stream(e));
    const double *sc = look.data() + sc_d;
    const int *tv = reinterpret_cast<const int *>(look.data() + tv_d);
    for (int j = 0; j < rows; ++j) {
      const double *s = sc + (size_t)j * S;
      int d;
      if (tv[j] <= 0) {
        d = -2;   // no voiced frames: no decision
      } else if (p->task == FB_TASK_SV) {
        d = s[0] >= p->threshold ? 1 : -1;
      } else {
        int am = 0;
        for (int m = 1; m < S; ++m) if (s[m] > s[am]) am = m;   // the first maximum
        d = (p->task == FB_TASK_OSI && s[am] < p->threshold) ? -1 : am;
      }
      decisions[logged + j] = d;
      dec[j] = (d != -2 && (targeted ? d == label : d != label)) ? 1 : 0;
    }
    logged += rows;
    queries += rows;
    return FB_OK;
  };
  // the boundary search between a and y: hi (-1: failed) and the rounds scored; on success x, hsj_sc[0] and hsj_best are new
  auto search = [&](const double *y_dev, bool first_exempt, int *hi_out, int *rounds_out) -> int {
    int lo = 0, hi = -1, r = 0, rounds = 0;
    for (;; ++r) {
      cand.clear();
      bool last = false;
      if (r == 0) {
        for (int j = 0; j < G; ++j) cand.push_back((int)(((long long)(j + 1) * FB_HSJ_Q) / G));
      } else {
        const int d = hi - lo;
        if (d - 1 <= G) {
          for (int qj = lo + 1; qj < hi; ++qj) cand.push_back(qj);
          last = true;
        } else {
          for (int j = 0; j < G; ++j) cand.push_back(lo + (int)(((long long)(j + 1) * d) / (G + 1)));
        }
      }
      const int rows = (int)cand.size();
      if (!(r == 0 && first_exempt) && over(rows)) { stopped = true; break; }
      FBCHK(layout(rows));
      fb_launch_hsj_line(e->stream, a_dev, y_dev, N, rows, cand.data(), bits, e->wav.as<int16_t>());
      FBCHK(score(rows));
      rounds = r + 1;
      int first = -1;
      for (int j = 0; j < rows && first < 0; ++j) if (dec[j]) first = j;
      if (first >= 0) {
        hi = cand[first];
        // the row of hi is a row that was scored: kept before the next batch takes its place
        HIPCHK(hipMemcpyAsync(e->hsj_best.p, e->wav.as<int16_t>() + (size_t)first * N, sizeof(int16_t) * (size_t)N,
                              hipMemcpyDeviceToDevice, e->stream));
        if (first > 0) lo = cand[first - 1];
      } else if (hi >= 0) {
        lo = cand[rows - 1];
      }
      if (hi < 0) break;   // nothing succeeded in round 0
      if (hi - lo == 1 || last || r == k->max_rounds - 1) break;
    }
    if (hi >= 0) launch_hsj_adopt(e, y_dev, N, hi);
    *hi_out = hi;
    *rounds_out = rounds;
    return FB_OK;
  };
  double D2 = 0.0;
  auto read_D2 = [&]() -> int {   // one double, and x for the caller who asked for every x_t
    FBCHK(d2h(e, &D2, e->hsj_sc.p, sizeof(double)));
    FBCHK(sync_stream(e));
    return FB_OK;
  };
  auto keep_x = [&](int t) -> int {
    if (x_trace) FBCHK(d2h(e, x_trace + (size_t)t * N, e->hsj_x.p, sizeof(double) * (size_t)N));
    return FB_OK;
  };
  auto row = [&](int t, double b, double np, double m, double hi, double rounds, double sigma) {
    double *tr = trace + (size_t)t * 8;
    tr[0] = D2; tr[1] = b; tr[2] = np; tr[3] = m; tr[4] = hi; tr[5] = rounds; tr[6] = (double)queries; tr[7] = sigma;
  };

  auto t_prev = std::chrono::steady_clock::now();
  auto tick = [&]() {
    const auto t_now = std::chrono::steady_clock::now();
    e->iter_seconds.push_back(std::chrono::duration<double>(t_now - t_prev).count());
    t_prev = t_now;
  };
  *success = -1;
  *n_iters = 0;
  int hi = -1, rounds = 0;
  FBCHK(search(e->hsj_init.as<double>(), true, &hi, &rounds));
  if (hi < 0) {   // the start is not decided as wanted: nothing to walk from
    row(0, 0.0, 0.0, -1.0, -1.0, (double)rounds, 0.0);
    tick();
    fb_launch_quantize(e->stream, a_dev, N, bits, e->hsj_best.as<int16_t>());
    FBCHK(d2h(e, adv_i16, e->hsj_best.p, sizeof(int16_t) * (size_t)N));
    if (adv_f64) FBCHK(d2h(e, adv_f64, e->audio.p, sizeof(double) * (size_t)N));
    FBCHK(sync_stream(e));
    HIPCHK(hipGetLastError());
    *dist2 = 0.0;
    *n_queries = queries;
    return FB_OK;
  }
  FBCHK(read_D2());
  FBCHK(keep_x(0));
  row(0, 0.0, 0.0, -1.0, (double)hi, (double)rounds, 0.0);
  tick();
  std::vector<int32_t> w(FB_HSJ_MAX_EVALS);
  for (int t = 1; t <= p->max_iter && !stopped; ++t) {
    const double dist = std::sqrt(D2);
    // 1 probes
    const int B = hsj_evals(k, t);
    if (over(B)) break;
    const double s0 = (k->probe_scale * dist) / std::sqrt((double)N), sigma = s0 > k->sigma_min ? s0 : k->sigma_min;
    FBCHK(layout(B));
    fb_launch_hsj_probes(e->stream, e->hsj_x.as<double>(), N, B, sigma, p->seed, p->stream, (uint32_t)t, bits,
                         e->wav.as<int16_t>(), e->hsj_z.as<float>());
    FBCHK(score(B));
    // 2 direction
    int np = 0;
    for (int j = 0; j < B; ++j) np += dec[j];
    const bool mixed = np > 0 && np < B;
    for (int j = 0; j < B; ++j) {
      const int phi = dec[j] ? 1 : -1;
      w[j] = mixed ? phi * B - (2 * np - B) : phi;
    }
    FBCHK(h2d(e, e->hsj_w.p, w.data(), sizeof(int32_t) * (size_t)B));
    launch_hsj_dir(e, B, N, p->seed, p->stream, (uint32_t)t, e->hsj_z.as<float>());
    // 3 step
    if (over(G)) break;
    const double xi = dist / std::sqrt((double)t);
    FBCHK(layout(G));
    fb_launch_hsj_step(e->stream, e->hsj_x.as<double>(), e->hsj_v.as<double>(), e->hsj_sc.as<double>() + 1, xi, 0, G, N, bits,
                       e->wav.as<int16_t>(), nullptr);
    FBCHK(score(G));
    int m = -1;
    for (int j = 0; j < G && m < 0; ++j) if (dec[j]) m = j;
    hi = -1;
    rounds = 0;
    if (m >= 0) {
      fb_launch_hsj_step(e->stream, e->hsj_x.as<double>(), e->hsj_v.as<double>(), e->hsj_sc.as<double>() + 1, xi, m, 1, N, bits,
                         nullptr, e->hsj_y.as<double>());
      FBCHK(search(e->hsj_y.as<double>(), false, &hi, &rounds));
      if (rounds == 0) break;   // stopped before the search scored a round: the iteration is dropped
      if (hi >= 0) FBCHK(read_D2());
    }
    FBCHK(keep_x(t));
    row(t, (double)B, (double)np, (double)m, (double)hi, (double)rounds, sigma);
    *n_iters = t;
    tick();
  }
  *success = 1;
  *dist2 = D2;
  *n_queries = queries;
  FBCHK(d2h(e, adv_i16, e->hsj_best.p, sizeof(int16_t) * (size_t)N));
  if (adv_f64) FBCHK(d2h(e, adv_f64, e->hsj_x.p, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_attack_hsj(fb_engine *e, const fb_nes_params *p, const fb_hsj_params *k, const double *audio, const double *init,
                             int64_t N, int16_t *adv_i16, double *adv_f64, int *success, double *dist2, int *n_iters,
                             int *n_queries, double *trace, int *decisions, long long decisions_cap, double *x_trace) {
  return hsj_attack(e, p, k, nullptr, audio, init, N, adv_i16, adv_f64, success, dist2, n_iters, n_queries, trace, decisions,
                    decisions_cap, x_trace);
}
extern "C" int fb_attack_hsj_foreign(fb_engine *e, const fb_nes_params *p, const fb_hsj_params *k, const fb_victim *v,
                                     const double *audio, const double *init, int64_t N, int16_t *adv_i16, double *adv_f64,
                                     int *success, double *dist2, int *n_iters, int *n_queries, double *trace, int *decisions,
                                     long long decisions_cap, double *x_trace) {
  if (!e || !p || !k || !v) return fb_fail(FB_E_ARG, "null argument (the victim descriptor included)");
  return hsj_attack(e, p, k, v, audio, init, N, adv_i16, adv_f64, success, dist2, n_iters, n_queries, trace, decisions,
                    decisions_cap, x_trace);
}

// ---- the hooks: exactly the launches of the attack, on state handed in
extern "C" int fb_debug_hsj_line(fb_engine *e, const double *a, const double *y, int64_t N, const int *q, int rows, int bits,
                                 int16_t *out, double *x, double *D2) {
  if (!e || !a || !y || !q || !out || !x || !D2 || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (rows < 1 || rows > FB_HSJ_MAX_GRID) return fb_fail(FB_E_ARG, "rows %d outside 1 .. %d", rows, FB_HSJ_MAX_GRID);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  for (int j = 0; j < rows; ++j)
    if (q[j] < 0 || q[j] > FB_HSJ_Q) return fb_fail(FB_E_ARG, "q %d outside 0 .. %d", q[j], FB_HSJ_Q);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the batch, without a batch layout)
  FBCHK(prepare_hsj(e, N, rows));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * rows));
  FBCHK(h2d(e, e->audio.p, a, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->hsj_y.p, y, sizeof(double) * (size_t)N));
  fb_launch_hsj_line(e->stream, e->audio.as<double>(), e->hsj_y.as<double>(), N, rows, q, bits, e->wav.as<int16_t>());
  launch_hsj_adopt(e, e->hsj_y.as<double>(), N, q[0]);
  FBCHK(d2h(e, out, e->wav.p, sizeof(int16_t) * (size_t)N * rows));
  FBCHK(d2h(e, x, e->hsj_x.p, sizeof(double) * (size_t)N));
  FBCHK(d2h(e, D2, e->hsj_sc.p, sizeof(double)));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_debug_hsj_probes(fb_engine *e, const double *x, int64_t N, double sigma, uint64_t seed, uint32_t stream,
                                   uint32_t t, int B, int bits, int16_t *out) {
  if (!e || !x || !out || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (B < 1 || B > FB_HSJ_MAX_EVALS) return fb_fail(FB_E_ARG, "B %d outside 1 .. %d", B, FB_HSJ_MAX_EVALS);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  FBCHK(prepare_hsj(e, N, B));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * B));
  FBCHK(e->hsj_z.ensure(sizeof(float) * (size_t)N * B));
  FBCHK(h2d(e, e->hsj_x.p, x, sizeof(double) * (size_t)N));
  fb_launch_hsj_probes(e->stream, e->hsj_x.as<double>(), N, B, sigma, seed, stream, t, bits, e->wav.as<int16_t>(),
                       e->hsj_z.as<float>());
  FBCHK(d2h(e, out, e->wav.p, sizeof(int16_t) * (size_t)N * B));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_debug_hsj_dir(fb_engine *e, const int32_t *w, int B, uint64_t seed, uint32_t stream, uint32_t t, int64_t N,
                                double *v, double *S) {
  if (!e || !w || !v || !S || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (B < 1 || B > FB_HSJ_MAX_EVALS) return fb_fail(FB_E_ARG, "B %d outside 1 .. %d", B, FB_HSJ_MAX_EVALS);
  for (int j = 0; j < B; ++j)
    if (w[j] < -2 * FB_HSJ_MAX_EVALS || w[j] > 2 * FB_HSJ_MAX_EVALS)
      return fb_fail(FB_E_ARG, "weight %d outside +-%d", w[j], 2 * FB_HSJ_MAX_EVALS);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the probes, without a batch layout)
  FBCHK(prepare_hsj(e, N, B));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * B));
  FBCHK(e->hsj_z.ensure(sizeof(float) * (size_t)N * B));
  FBCHK(h2d(e, e->hsj_w.p, w, sizeof(int32_t) * (size_t)B));
  // the attack's pair: the probes launch (here of x = 0, its rows not read) hands its normals to the direction launch
  HIPCHK(hipMemsetAsync(e->hsj_x.p, 0, sizeof(double) * (size_t)N, e->stream));
  fb_launch_hsj_probes(e->stream, e->hsj_x.as<double>(), N, B, 0x1p-15, seed, stream, t, 16, e->wav.as<int16_t>(), e->hsj_z.as<float>());
  launch_hsj_dir(e, B, N, seed, stream, t, e->hsj_z.as<float>());
  FBCHK(d2h(e, v, e->hsj_v.p, sizeof(double) * (size_t)N));
  FBCHK(d2h(e, S, e->hsj_sc.as<double>() + 1, sizeof(double)));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_debug_hsj_step(fb_engine *e, const double *x, const double *v, int64_t N, double S, double xi, int G, int bits,
                                 int16_t *out, double *y) {
  if (!e || !x || !v || !out || !y || N <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (G < 1 || G > FB_HSJ_MAX_GRID) return fb_fail(FB_E_ARG, "grid %d outside 1 .. %d", G, FB_HSJ_MAX_GRID);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  FBCHK(prepare_hsj(e, N, G));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * G));
  FBCHK(h2d(e, e->hsj_x.p, x, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->hsj_v.p, v, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->hsj_sc.as<double>() + 1, &S, sizeof(double)));
  fb_launch_hsj_step(e->stream, e->hsj_x.as<double>(), e->hsj_v.as<double>(), e->hsj_sc.as<double>() + 1, xi, 0, G, N, bits,
                     e->wav.as<int16_t>(), nullptr);
  FBCHK(d2h(e, out, e->wav.p, sizeof(int16_t) * (size_t)N * G));
  for (int m = 0; m < G; ++m) {   // the float64 launch of one m, as the attack runs it for the m it takes
    fb_launch_hsj_step(e->stream, e->hsj_x.as<double>(), e->hsj_v.as<double>(), e->hsj_sc.as<double>() + 1, xi, m, 1, N, bits,
                       nullptr, e->hsj_y.as<double>());
    FBCHK(d2h(e, y + (size_t)m * N, e->hsj_y.p, sizeof(double) * (size_t)N));
  }
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// tools/hsj_rate.py: `reps` launches of each kernel between two events, after one of each to warm up.  ms[8], per launch:
// line (G rows), adopt + its sum, probes (B rows), probes that keep their normals, direction + its sum drawing the normals
// again, direction + its sum reading the kept ones, step (G rows), the NES batch launch (k_perturb) of B rows (B odd: B - 1
// rows drawn and one clean row; B even: B + 1 rows)
extern "C" int fb_bench_hsj_kernels(fb_engine *e, const double *a, const double *y, int64_t N, int B, int G, int bits, int reps,
                                    double *ms) {
  if (!e || !a || !y || !ms || N <= 0 || reps < 1) return fb_fail(FB_E_ARG, "bad argument");
  if (B < 1 || B > FB_HSJ_MAX_EVALS) return fb_fail(FB_E_ARG, "B %d outside 1 .. %d", B, FB_HSJ_MAX_EVALS);
  if (G < 1 || G > FB_HSJ_MAX_GRID) return fb_fail(FB_E_ARG, "grid %d outside 1 .. %d", G, FB_HSJ_MAX_GRID);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  e->nes_rec.iter = -1;  // (the k_perturb launches below overwrite zbuf)
  const int half = (B + 1) / 2, nes_rows = 2 * half + 1, rows = std::max(std::max(B, G), nes_rows);
  FBCHK(prepare_hsj(e, N, rows));
  FBCHK(ensure_nes_buffers(e, N, nes_rows));
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)N * rows));
  FBCHK(e->hsj_z.ensure(sizeof(float) * (size_t)N * B));
  FBCHK(h2d(e, e->audio.p, a, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->hsj_y.p, y, sizeof(double) * (size_t)N));
  FBCHK(h2d(e, e->adver.p, y, sizeof(double) * (size_t)N));
  std::vector<int> q(G);
  for (int j = 0; j < G; ++j) q[j] = (int)(((long long)(j + 1) * FB_HSJ_Q) / G);
  std::vector<int32_t> w(B);
  for (int j = 0; j < B; ++j) w[j] = (j & 1) ? B : -B;
  FBCHK(h2d(e, e->hsj_w.p, w.data(), sizeof(int32_t) * (size_t)B));
  const double sigma = 0x1p-15;
  auto run = [&](int which) {
    switch (which) {
      case 0: fb_launch_hsj_line(e->stream, e->audio.as<double>(), e->hsj_y.as<double>(), N, G, q.data(), bits, e->wav.as<int16_t>()); break;
      case 1: launch_hsj_adopt(e, e->hsj_y.as<double>(), N, q[0]); break;
      case 2: fb_launch_hsj_probes(e->stream, e->hsj_x.as<double>(), N, B, sigma, 1234, 0, 1, bits, e->wav.as<int16_t>(), nullptr); break;
      case 3: fb_launch_hsj_probes(e->stream, e->hsj_x.as<double>(), N, B, sigma, 1234, 0, 1, bits, e->wav.as<int16_t>(), e->hsj_z.as<float>()); break;
      case 4: launch_hsj_dir(e, B, N, 1234, 0, 1, nullptr); break;
      case 5: launch_hsj_dir(e, B, N, 1234, 0, 1, e->hsj_z.as<float>()); break;
      case 6: fb_launch_hsj_step(e->stream, e->hsj_x.as<double>(), e->hsj_v.as<double>(), e->hsj_sc.as<double>() + 1, 0.01, 0, G, N, bits,
                                 e->wav.as<int16_t>(), nullptr); break;
      default: {
        int n_part = 0;
        fb_launch_perturb(e->stream, e->adver.as<double>(), e->audio.as<double>(), N, half, sigma, 1234, 1, 0, nullptr,
                          e->wav.as<int16_t>(), e->dist_part.as<double>(), &n_part, e->zbuf.as<float>(), nullptr, bits);
        break;
      }
    }
  };
  for (int which = 0; which < 8; ++which) run(which);   // warm up, in an order in which every launch finds its inputs
  for (int which = 0; which < 8; ++which) {
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; ++i) run(which);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
    ms[which] = (double)t / reps;
  }
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// ---- voted decisions: k_vote alone, on raw scores handed in (fakebob_hip_test.h)
// the checks and uploads of both hooks: raw[rows * r][n_out] -> e->raw, tv[rows * r] -> e->tv; the label by the attacks' rule
static int stage_vote(fb_engine *e, const double *raw, const int *tv, int rows, int r, int task, int attack_type, int label) {
  if (!e || !raw || !tv) return fb_fail(FB_E_ARG, "null argument");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no model loaded");
  if (task != e->task) return fb_fail(FB_E_ARG, "task %d != engine system task %d", task, e->task);
  if (attack_type != FB_TARGETED && attack_type != FB_UNTARGETED) return fb_fail(FB_E_ARG, "bad attack_type %d", attack_type);
  if (r < 1 || r > 32) return fb_fail(FB_E_ARG, "%d replicas per row: 1 .. 32", r);
  if (rows < 1 || (int64_t)rows * r > 65535) return fb_fail(FB_E_LIMIT, "rows %d * replicas %d outside 1 .. 65535", rows, r);
  const int S = fb_num_speakers(e);
  const bool ok = task == FB_TASK_SV ? (label == 1 || label == -1) : task == FB_TASK_OSI ? (label >= -1 && label < S) : (label >= 0 && label < S);
  if (!ok) return fb_fail(FB_E_ARG, "label %d is no decision of this system", label);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t n = (size_t)rows * r;
  FBCHK(e->raw.ensure(sizeof(double) * n * e->n_out));
  FBCHK(e->tv.ensure(sizeof(int) * n));
  FBCHK(e->eot_sc.ensure(sizeof(double) * n * (size_t)std::max(S, 1)));
  FBCHK(e->vote_look.ensure(vote_look_bytes(rows, S)));
  FBCHK(h2d(e, e->raw.p, raw, sizeof(double) * n * e->n_out));
  FBCHK(h2d(e, e->tv.p, tv, sizeof(int) * n));
  return FB_OK;
}
extern "C" int fb_debug_vote(fb_engine *e, const double *raw, const int *tv, int rows, int r, int task, double threshold,
                             int attack_type, int label, int *votes, int *nodec, double *mean) {
  if (!votes || !nodec || !mean) return fb_fail(FB_E_ARG, "null argument");
  FBCHK(stage_vote(e, raw, tv, rows, r, task, attack_type, label));
  fb_nes_params p = {};
  p.task = task;
  p.threshold = threshold;
  launch_vote(e, &p, rows, r, attack_type == FB_TARGETED, label);
  const int S = fb_num_speakers(e);
  std::vector<double> look(vote_look_bytes(rows, S) / sizeof(double));
  const FbVoteLook v = vote_look_at(look.data(), rows, S);
  FBCHK(d2h(e, look.data(), e->vote_look.p, v.bytes));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  memcpy(votes, v.votes, sizeof(int) * (size_t)rows);
  memcpy(nodec, v.nodec, sizeof(int) * (size_t)rows);
  memcpy(mean, v.mean, sizeof(double) * (size_t)rows * S);
  return FB_OK;
}
// tools/query_eot_rate.py: `reps` launches of k_vote between two events, after one to warm up -> *ms per launch
extern "C" int fb_bench_vote(fb_engine *e, const double *raw, const int *tv, int rows, int r, int task, double threshold,
                             int attack_type, int label, int reps, double *ms) {
  if (!ms || reps < 1) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(stage_vote(e, raw, tv, rows, r, task, attack_type, label));
  fb_nes_params p = {};
  p.task = task;
  p.threshold = threshold;
  launch_vote(e, &p, rows, r, attack_type == FB_TARGETED, label);
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  for (int i = 0; i < reps; ++i) launch_vote(e, &p, rows, r, attack_type == FB_TARGETED, label);
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
  *ms = (double)t / reps;
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// ---- foreign victims: the two launches alone, on arrays handed in (fakebob_hip_test.h)
extern "C" int fb_debug_rows_to_model(fb_engine *e, const int16_t *rows_i16, int rows, int64_t N, int bits, int dtype, void *out) {
  if (!e || !rows_i16 || !out) return fb_fail(FB_E_ARG, "null argument");
  if (rows < 1 || N < 1 || (int64_t)rows * N > ((int64_t)1 << 31)) return fb_fail(FB_E_ARG, "rows %d x N %lld outside 1 .. 2^31 elements", rows, (long long)N);
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported (2 .. 16)", bits);
  if (dtype != FB_DT_F32 && dtype != FB_DT_F64) return fb_fail(FB_E_ARG, "dtype %d: FB_DT_F32 or FB_DT_F64", dtype);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // (e->wav takes the rows, without a batch layout)
  const size_t n = (size_t)rows * (size_t)N, xb = n * (dtype == FB_DT_F32 ? sizeof(float) : sizeof(double));
  FBCHK(e->wav.ensure(sizeof(int16_t) * n));
  FBCHK(e->ext_x.ensure(xb));
  FBCHK(h2d(e, e->wav.p, rows_i16, sizeof(int16_t) * n));
  fb_launch_rows_to_model(e->stream, dtype, e->wav.as<int16_t>(), rows, N, bits, e->ext_x.p);
  FBCHK(d2h(e, out, e->ext_x.p, xb));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}
extern "C" int fb_debug_decide_foreign(fb_engine *e, const void *scores, int dtype, int rows, int S, int task, double threshold,
                                       int *decisions, double *scores_f64) {
  if (!e || !scores || !decisions || !scores_f64) return fb_fail(FB_E_ARG, "null argument");
  if (rows < 1 || rows > 65535) return fb_fail(FB_E_ARG, "rows %d outside 1 .. 65535", rows);
  if (S < 1 || S > 62) return fb_fail(FB_E_ARG, "S %d outside 1 .. 62", S);
  if (task != FB_TASK_SV && task != FB_TASK_OSI && task != FB_TASK_CSI) return fb_fail(FB_E_ARG, "bad task %d", task);
  if (task == FB_TASK_SV && S != 1) return fb_fail(FB_E_ARG, "SV scores one speaker (got S = %d)", S);
  if (dtype != FB_DT_F32 && dtype != FB_DT_F64) return fb_fail(FB_E_ARG, "dtype %d: FB_DT_F32 or FB_DT_F64", dtype);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t n = (size_t)rows * S, sb = n * (dtype == FB_DT_F32 ? sizeof(float) : sizeof(double));
  FBCHK(e->raw.ensure(sb));
  FBCHK(e->fg_look.ensure(sizeof(double) * foreign_look_doubles(rows, S)));
  FBCHK(h2d(e, e->raw.p, scores, sb));
  double *sc_dev = e->fg_look.as<double>() + ((size_t)rows + 1) / 2;
  fb_launch_decide_foreign(e->stream, dtype, e->raw.p, rows, S, task, threshold, e->fg_look.as<int>(), sc_dev);
  FBCHK(d2h(e, decisions, e->fg_look.p, sizeof(int) * (size_t)rows));
  FBCHK(d2h(e, scores_f64, sc_dev, sizeof(double) * n));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}
// tools/foreign_rate.py: ms[5] = milliseconds of k_rows_to_model<float>, k_rows_to_model<double>, k_decide_foreign<double>
// (`reps` launches of each between two events after one to warm up), and of the two ways a host victim can get its rows, on
// the host's clock, once each after one to warm up: the float64 rows copied to the host; the int16 rows copied and widened there
extern "C" int fb_bench_foreign_rows(fb_engine *e, int rows, int64_t N, int bits, int S, int reps, double *ms) {
  if (!e || !ms || reps < 1) return fb_fail(FB_E_ARG, "bad argument");
  if (rows < 1 || rows > 65535 || N < 1 || S < 1 || S > 62 || bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bad shape");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  const size_t n = (size_t)rows * (size_t)N;
  FBCHK(e->wav.ensure(sizeof(int16_t) * n));
  FBCHK(e->ext_x.ensure(sizeof(double) * n));
  FBCHK(e->raw.ensure(sizeof(double) * (size_t)rows * S));
  FBCHK(e->fg_look.ensure(sizeof(double) * foreign_look_doubles(rows, S)));
  HIPCHK(hipMemsetAsync(e->wav.p, 0x11, sizeof(int16_t) * n, e->stream));
  HIPCHK(hipMemsetAsync(e->raw.p, 0, sizeof(double) * (size_t)rows * S, e->stream));
  auto run = [&](int which) {
    if (which == 0) fb_launch_rows_to_model(e->stream, FB_DT_F32, e->wav.as<int16_t>(), rows, N, bits, e->ext_x.p);
    else if (which == 1) fb_launch_rows_to_model(e->stream, FB_DT_F64, e->wav.as<int16_t>(), rows, N, bits, e->ext_x.p);
    else fb_launch_decide_foreign(e->stream, FB_DT_F64, e->raw.p, rows, S, FB_TASK_CSI, 0.0, e->fg_look.as<int>(),
                                  e->fg_look.as<double>() + ((size_t)rows + 1) / 2);
  };
  for (int which = 0; which < 3; ++which) {
    run(which);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; ++i) run(which);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
    ms[which] = (double)t / reps;
  }
  run(1);
  std::vector<double> xh(n);
  std::vector<int16_t> qh(n);
  const double scale = ldexp(1.0, -(bits - 1));
  for (int pass = 0; pass < 2; ++pass) {   // (the first pass touches the pages)
    auto t0 = std::chrono::steady_clock::now();
    FBCHK(d2h(e, xh.data(), e->ext_x.p, sizeof(double) * n));
    FBCHK(sync_stream(e));
    auto t1 = std::chrono::steady_clock::now();
    FBCHK(d2h(e, qh.data(), e->wav.p, sizeof(int16_t) * n));
    FBCHK(sync_stream(e));
    for (size_t i = 0; i < n; ++i) xh[i] = (double)qh[i] * scale;
    auto t2 = std::chrono::steady_clock::now();
    ms[3] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[4] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  }
  HIPCHK(hipGetLastError());
  return FB_OK;
}

struct Plateau {  // FAKEBOB.py:195-200
  std::vector<double> ls;
  double lr;
  void step(double loss, const fb_nes_params *p) {
    ls.push_back(loss);
    if ((int)ls.size() > p->plateau_length) ls.erase(ls.begin(), ls.end() - p->plateau_length);
    if (!ls.empty() && ls.back() > ls.front() && (int)ls.size() == p->plateau_length) {
      if (lr > p->min_lr) { double l2 = lr / p->plateau_drop; lr = l2 > p->min_lr ? l2 : p->min_lr; }
      ls.clear();
    }
  }
};

extern "C" int fb_estimate_threshold(fb_engine *e, const fb_nes_params *p_in, double model_threshold,
                                     const double *audio, int64_t N, const double *noise_all, int max_total_iters,
                                     double *score_out, int *n_iters_out, int *n_outer_out, double *thr_final,
                                     double *adver_f64) {
  if (e) e->bench_it = e->nes_rec.iter = -1;
  if (!audio || !score_out) return fb_fail(FB_E_ARG, "null argument");
  if (!p_in) return fb_fail(FB_E_ARG, "null params");
  if (p_in->task == FB_TASK_CSI) return fb_fail(FB_E_ARG, "no threshold to estimate for CSI (FAKEBOB.py:41-43)");
  if (e && e->eot > 1)
    return fb_fail(FB_E_STATE, "fb_estimate_threshold does not run under expectation over transformation (fb_set_eot(%d)): set 1", e->eot);
  if (e && e->comp_K1 > 0)
    return fb_fail(FB_E_STATE, "fb_estimate_threshold does not run with companion utterances (fb_set_companions: %d set): clear them", e->comp_K1);
  FBCHK(refuse_play(e, "fb_estimate_threshold"));
  fb_nes_params q = *p_in;
  q.attack_type = FB_UNTARGETED;  // :73-74
  FbScorer sc{FB_SCORER_NATIVE};
  FBCHK(nes_setup(e, &q, N, sc, false));
  const int half = q.samples_per_draw / 2, B = 2 * half + 1, S = sc.S;
  FBCHK(attack_start(e, audio, N, half, noise_all));
  // Column 0 of every NES batch is the clean adver (noise 0), i.e. exactly what
  // model.score(audio) (:53) / model.make_decisions(adver) (:89) would score, so one batch
  // per inner iteration serves both the decision and the gradient.
  const double one_minus_m = 1.0 - q.momentum;
  bool have_init = false;
  double delta = 0.0;
  int n_iters = 0, n_outer = 0;
  Plateau pl;
  pl.lr = q.max_lr;
  q.threshold = 0.0;
  int rc = FB_OK;
  for (;;) {
    const double *noise_dev = nullptr;
    if (noise_all && half > 0) {
      if (n_iters >= max_total_iters) { rc = fb_fail(FB_E_LIMIT, "max_total_iters %d reached", max_total_iters); break; }
      FBCHK(h2d(e, e->noise.p, noise_all + (size_t)n_iters * N * half, sizeof(double) * (size_t)N * half));
      noise_dev = e->noise.as<double>();
    }
    // the loss depends on q.threshold, which may change below; scores do not.  Score first
    // with the current threshold, then (rarely) recompute the loss after a sweep step.
    FBCHK(enqueue_get_grad(e, &q, N, (uint32_t)n_iters, noise_dev, false));
    FBCHK(fetch_out(e, true));
    double s0 = e->h_out->score0[0];
    for (int s = 1; s < S; ++s) if (e->h_out->score0[s] > s0) s0 = e->h_out->score0[s];
    bool thr_changed = false;
    if (!have_init) {  // :53-59
      delta = fabs(s0 / 10.0);
      q.threshold = s0 + delta;
      have_init = true;
      thr_changed = true;
    }
    if (s0 >= model_threshold) { *score_out = s0; break; }  // decision != -1 (:96-103)
    while (s0 >= q.threshold) {  // early stop of the inner loop (:105-109) -> next outer (:135-137)
      q.threshold += delta;
      ++n_outer;
      pl.lr = q.max_lr;  // :82-83
      pl.ls.clear();
      thr_changed = true;
      if (!(delta > 0.0)) break;
    }
    if (n_iters >= max_total_iters) { rc = fb_fail(FB_E_LIMIT, "max_total_iters %d reached", max_total_iters); break; }
    if (thr_changed) {
      fb_launch_loss(e->stream, e->raw.as<double>(), e->tv.as<int>(), B, e->n_out, q.task, e->kind, q.attack_type,
                     e->zmean.as<double>(), e->zstd.as<double>(), q.threshold, q.adver_thresh, q.target,
                     q.true_label, e->dist_part.as<double>(), 0, e->scores.as<double>(), e->loss.as<double>(),
                     e->nes_out.as<FbNesDev>());
      FBCHK(fetch_out(e, true));
    }
    e->nes_iters += 1;
    pl.step(e->h_out->final_loss, &q);
    fb_launch_grad_update(e->stream, e->loss.as<double>(), N, half, q.sigma, e->zbuf.as<float>(), noise_dev,
                          nullptr, 1, q.momentum, one_minus_m, pl.lr, q.epsilon, e->audio.as<double>(),
                          e->grad_m.as<double>(), e->adver.as<double>());
    ++n_iters;
  }
  if (n_iters_out) *n_iters_out = n_iters;
  if (n_outer_out) *n_outer_out = n_outer;
  if (thr_final) *thr_final = q.threshold;
  if (adver_f64) FBCHK(d2h(e, adver_f64, e->adver.p, sizeof(double) * (size_t)N));
  FBCHK(sync_stream(e));
  return rc;
}

// ------------------------------------------------------------- debug hooks
extern "C" int fb_debug_noise(fb_engine *e, uint64_t seed, uint32_t iter, uint32_t stream, int64_t N, int half,
                              float *z) {
  if (!e || !z || N <= 0 || half <= 0) return fb_fail(FB_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  DevBuf tmp;
  FBCHK(tmp.ensure(sizeof(float) * (size_t)N * half));
  fb_launch_noise(e->stream, seed, iter, stream, N, half, tmp.as<float>());
  HIPCHK(hipMemcpyAsync(z, tmp.p, sizeof(float) * (size_t)N * half, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return FB_OK;
}

extern "C" int fb_debug_quantize(fb_engine *e, const double *x, int64_t n, int bits, int16_t *q) {
  if (!e || !x || !q || n <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (bits < 2 || bits > 16) return fb_fail(FB_E_ARG, "bits_per_sample %d unsupported", bits);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)n));
  FBCHK(e->stage_f64.ensure(sizeof(double) * (size_t)n));
  FBCHK(h2d(e, e->stage_f64.p, x, sizeof(double) * (size_t)n));
  fb_launch_quantize(e->stream, e->stage_f64.as<double>(), n, bits, e->wav.as<int16_t>());
  FBCHK(d2h(e, q, e->wav.p, sizeof(int16_t) * (size_t)n));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// pt (nullable): the point of the RNG contracts the utterance stands at; null = a scoring call of the engine's own
static int debug_frontend(fb_engine *e, const int16_t *wav, int64_t n, const FbRngPoint *pt = nullptr) {
  if (!e || !wav || n <= 0) return fb_fail(FB_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  int64_t off[2] = {0, n};
  FBCHK(e->wav.ensure(sizeof(int16_t) * (size_t)n));
  FBCHK(h2d(e, e->wav.p, wav, sizeof(int16_t) * (size_t)n));
  FBCHK(prepare_batch(e, off, 1));
  e->cached_B = -1;
  const int T = e->h_frame_off[1];
  const FbFrontendDev &fe = e->fe;
  FBCHK(e->mfcc.ensure(sizeof(float) * (size_t)T * fe.nc));
  FBCHK(e->vrank.ensure(sizeof(int) * (size_t)T));
  FBCHK(e->tv.ensure(sizeof(int)));
  FBCHK(e->row_off.ensure(sizeof(int) * 2));
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)T * fe.dim));
  choose_launch_shape(e);
  const FbScoreCall call{pt ? *pt : scoring_call_point(e)};
  FBCHK(launch_mfcc(e, call, fe, 1, T));
  FBCHK(run_post_mfcc(e, fe, 1));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// The launches of enrolment statistics on the n rows (*n_rows_ptr, at most T) of e->feats: the single-model dump, the
// float32 soft-max and the float64 accumulation; the copies of occ[C] and F[C][D] are queued, the caller synchronises.
static int gmm_stats_launch(fb_engine *e, const int *n_rows_ptr, int T, double *occ, double *F) {
  const FbGmmDev &g = e->gmm;
  const int ld = g.n_tiles * 32;
  FBCHK(e->enr_ll.ensure(sizeof(float) * (size_t)T * ld));
  FBCHK(e->enr_aux.ensure(sizeof(float) * 2 * (size_t)T));
  FBCHK(e->enr_stats.ensure(sizeof(double) * (size_t)g.C * (g.D + 1)));
  hipStream_t s = e->stream;
  fb_launch_gmm_dump(s, g, e->feats.as<float>(), n_rows_ptr, T, choose_chunks(g, T, false), e->enr_ll.as<float>(), &e->shape_gmm);
  double *d_occ = e->enr_stats.as<double>(), *d_F = d_occ + g.C;
  fb_launch_gmm_post_stats(s, g.C, ld, g.D, e->enr_ll.as<float>(), e->feats.as<float>(), n_rows_ptr, T,
                           e->enr_aux.as<float>(), e->enr_aux.as<float>() + T, d_occ, d_F);
  FBCHK(d2h(e, occ, d_occ, sizeof(double) * (size_t)g.C));
  FBCHK(d2h(e, F, d_F, sizeof(double) * (size_t)g.C * g.D));
  return FB_OK;
}

// Enrolment statistics (build_spk_models.py:184-216, `gmm-global-acc-stats --update-flags=m`): posteriors
// of the loaded GMM (the UBM, loaded alone) on the voiced frames of one utterance.
extern "C" int fb_gmm_acc_stats(fb_engine *e, const int16_t *wav, int64_t n, double *occ, double *F, int *tv_out) {
  if (!e || !wav || !occ || !F || n <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (e->have_gmm && e->kind == 2)
    return fb_fail(FB_E_STATE, "fb_gmm_acc_stats: an x-vector system is loaded (GMM statistics of a TDNN victim: not in this version)");
  if (!e->have_gmm || e->kind != 0 || e->gmm.M != 1)
    return fb_fail(FB_E_STATE, "load exactly one diagonal GMM (the UBM) before accumulating statistics");
  FBCHK(debug_frontend(e, wav, n));  // MFCC, VAD, deltas, CMVN, voiced rows of this utterance
  const int T = e->h_frame_off[1];
  int tv = 0;
  FBCHK(d2h(e, &tv, e->tv.p, sizeof(int)));
  FBCHK(gmm_stats_launch(e, e->row_off.as<int>() + 1, T, occ, F));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  if (tv_out) *tv_out = tv;
  if (tv <= 0) return fb_fail(FB_E_NO_VOICED, "enrolment utterance has no voiced frames");
  return FB_OK;
}

// Test hook: the launches of fb_gmm_acc_stats on T rows of features handed in as they are (no front-end); with `ll` the
// dump matrix comes back as [T][C], without the padding columns of its last 32-component tile.
extern "C" int fb_debug_gmm_acc_rows(fb_engine *e, const float *feats, int T, float *ll, double *occ, double *F) {
  if (!e || !feats || !occ || !F || T <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 0 || e->gmm.M != 1)
    return fb_fail(FB_E_STATE, "load exactly one diagonal GMM (the UBM) before accumulating statistics");
  HIPCHK(hipSetDevice(e->device));
  const FbGmmDev &g = e->gmm;
  FBCHK(sync_stream(e));
  choose_launch_shape(e);
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)T * g.D));
  FBCHK(e->row_off.ensure(sizeof(int) * 2));
  const int rows_host[2] = {0, T};
  HIPCHK(hipMemcpy(e->feats.p, feats, sizeof(float) * (size_t)T * g.D, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->row_off.p, rows_host, sizeof(rows_host), hipMemcpyHostToDevice));
  e->last_total_frames = 0;  // the feature buffer no longer belongs to a scored batch
  FBCHK(gmm_stats_launch(e, e->row_off.as<int>() + 1, T, occ, F));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  if (ll)
    HIPCHK(hipMemcpy2D(ll, sizeof(float) * (size_t)g.C, e->enr_ll.p, sizeof(float) * (size_t)g.n_tiles * 32,
                       sizeof(float) * (size_t)g.C, (size_t)T, hipMemcpyDeviceToHost));
  return FB_OK;
}


extern "C" int fb_set_fused_chain(fb_engine *e, int on) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  const int opt = on < 0 ? -1 : (on ? 1 : 0);
  shared_chain_count(e->device, (opt == 0) - (e->fuse_opt == 0));
  e->fuse_opt = opt;
  return FB_OK;
}

extern "C" int fb_debug_shared_chain_engines(fb_engine *e, int *count) {
  if (!e || !count) return fb_fail(FB_E_ARG, "null argument");
  *count = shared_chain_count(e->device, 0);
  return FB_OK;
}

extern "C" int fb_gmm_kernel_mode(fb_engine *e) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  return e->gmm.mode;
}

extern "C" int fb_gmm_kernel_variant(fb_engine *e, double *shift_rms) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  if (shift_rms) *shift_rms = e->gmm_delta_rms;
  if (e->kind == 0 && fb_gmm_use_wide(e->gmm)) return 10 + e->gmm.delta_p;
  return e->gmm.mode;
}

extern "C" int fb_gmm_delta_tiles(fb_engine *e, int *tiles_p1, int *tiles_p2, int *tiles_p3) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  const bool wide = e->kind == 0 && fb_gmm_use_wide(e->gmm);
  if (tiles_p3) *tiles_p3 = wide ? e->gmm.delta_t3 : 0;
  if (tiles_p2) *tiles_p2 = wide ? e->gmm.delta_t2 - e->gmm.delta_t6 : 0;
  if (tiles_p1) *tiles_p1 = wide ? e->gmm.n_tiles - e->gmm.delta_t2 : 0;
  return wide ? 1 : 0;
}

extern "C" int fb_gmm_delta_tiles_f6(fb_engine *e) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (!e->have_gmm) return fb_fail(FB_E_STATE, "no GMM loaded");
  const bool wide = e->kind == 0 && fb_gmm_use_wide(e->gmm);
  return wide ? e->gmm.delta_t6 - e->gmm.delta_t3 : 0;
}

static int debug_mfcc(fb_engine *e, const int16_t *wav, int64_t n, const FbRngPoint *pt, float *mfcc, int *T_out) {
  if (!mfcc) return fb_fail(FB_E_ARG, "mfcc is NULL");
  FBCHK(debug_frontend(e, wav, n, pt));
  const int T = e->h_frame_off[1];
  FBCHK(d2h(e, mfcc, e->mfcc.p, sizeof(float) * (size_t)T * e->fe.nc));
  FBCHK(sync_stream(e));
  if (T_out) *T_out = T;
  return FB_OK;
}
extern "C" int fb_debug_mfcc(fb_engine *e, const int16_t *wav, int64_t n, float *mfcc, int *T_out) {
  return debug_mfcc(e, wav, n, nullptr, mfcc, T_out);
}
extern "C" int fb_debug_mfcc_dither(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream,
                                    uint32_t epoch, uint32_t utt, float *mfcc, int *T_out) {
  const FbRngPoint pt{seed, stream, epoch, utt};
  return debug_mfcc(e, wav, n, &pt, mfcc, T_out);
}

// the normals of the dither contract, from the device function the MFCC kernels call
extern "C" int fb_debug_dither_noise(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int t0,
                                     int n_frames, int L, float *z) {
  if (!e || !z || t0 < 0 || n_frames <= 0 || L <= 0) return fb_fail(FB_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t bytes = sizeof(float) * (size_t)n_frames * L;
  DevBuf tmp;
  FBCHK(tmp.ensure(bytes));
  fb_launch_dither_noise(e->stream, fb_dither_key(FbRngPoint{seed, stream, epoch, utt}, 1.0), t0, n_frames, L, tmp.as<float>());
  HIPCHK(hipMemcpyAsync(z, tmp.p, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return FB_OK;
}

// ---- input-transform chain (the stage contract: include/fakebob_hip.h)
extern "C" int fb_set_input_transform(fb_engine *e, const fb_tf_stage *stages, int n) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (n < 0 || n > FB_TF_MAX_STAGES) return fb_fail(FB_E_ARG, "%d stages: an input-transform chain has 0 .. %d", n, FB_TF_MAX_STAGES);
  if (n > 0 && !stages) return fb_fail(FB_E_ARG, "stages is NULL");
  // everything is checked before anything is changed: a refusal keeps the previous chain
  FbTfChain ch = {};
  std::vector<double> taps;
  for (int s = 0; s < n; ++s) {
    const int kind = stages[s].kind, k = stages[s].k;
    int radius = 0;
    if (kind == FB_TF_QUANT) {
      if (k < 1 || k > 16384) return fb_fail(FB_E_ARG, "stage %d: quantisation step %d outside 1 .. 16384", s, k);
    } else if (kind == FB_TF_DECIMATE) {
      if (k < 2 || k > 64) return fb_fail(FB_E_ARG, "stage %d: decimation factor %d outside 2 .. 64", s, k);
    } else if (kind == FB_TF_MEDIAN) {
      if (k < 3 || k > 31 || !(k & 1)) return fb_fail(FB_E_ARG, "stage %d: median width %d is not odd in 3 .. 31", s, k);
      radius = (k - 1) / 2;
    } else if (kind == FB_TF_FIR) {
      if (k < 1 || k > 511 || !(k & 1)) return fb_fail(FB_E_ARG, "stage %d: FIR length %d is not odd in 1 .. 511", s, k);
      if (!stages[s].taps) return fb_fail(FB_E_ARG, "stage %d: FIR taps are NULL", s);
      for (int j = 0; j < k; ++j)
        if (!(fabs(stages[s].taps[j]) <= 1048576.0))  // (NaN fails the comparison too)
          return fb_fail(FB_E_ARG, "stage %d: tap %d is not finite or exceeds 2^20 in magnitude", s, j);
      radius = (k - 1) / 2;
      ch.tap_off[s] = (int)taps.size();
      taps.insert(taps.end(), stages[s].taps, stages[s].taps + k);
    } else if (kind == FB_TF_NOISE) {
      if (k != 0 && k != 1) return fb_fail(FB_E_ARG, "stage %d: noise mode %d is neither 0 (absolute) nor 1 (SNR)", s, k);
      if (!stages[s].taps) return fb_fail(FB_E_ARG, "stage %d: the noise stage's parameter (taps[0]) is NULL", s);
      const double v = stages[s].taps[0];
      if (k == 0 && !(v >= 0.0 && v <= 32768.0))  // (NaN fails the comparisons too)
        return fb_fail(FB_E_ARG, "stage %d: noise amplitude %g is not in 0 .. 32768", s, v);
      if (k == 1 && !(v > 0.0 && std::isfinite(v)))
        return fb_fail(FB_E_ARG, "stage %d: rho = %g (10^(snr_db / 10)) is not finite and positive", s, v);
      ch.tap_off[s] = (int)taps.size();
      taps.push_back(v);
    } else {
      return fb_fail(FB_E_ARG, "stage %d: unknown kind %d", s, kind);
    }
    ch.kind[s] = kind;
    ch.k[s] = k;
    ch.H += radius;
  }
  if (ch.H > FB_TF_MAX_HALO) return fb_fail(FB_E_ARG, "the stages' radii sum to %d: at most %d", ch.H, FB_TF_MAX_HALO);
  ch.n = n;
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));  // nothing in flight reads the taps any more
  DevBuf fresh;
  if (!taps.empty()) {
    FBCHK(fresh.ensure(sizeof(double) * taps.size()));
    FBCHK(h2d(e, fresh.p, taps.data(), sizeof(double) * taps.size()));
    FBCHK(sync_stream(e));
  }
  e->tf_taps = std::move(fresh);
  e->tf = ch;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was scored through the previous chain
  return FB_OK;
}

extern "C" int fb_debug_input_transform(fb_engine *e, const int16_t *wav, const int64_t *off, int B, int16_t *out) {
  if (!e || !wav || !off || !out || B <= 0 || B > 65535) return fb_fail(FB_E_ARG, "bad argument");
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b];
    if (n <= 0) return fb_fail(FB_E_ARG, "utterance %d is empty", b);
    if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance %d longer than 2^31 samples", b);
    n_max = std::max(n_max, n);
  }
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // the scoring batch layout no longer describes e->wav / e->wav_off
  e->bench_it = e->nes_rec.iter = -1;
  const size_t bytes = sizeof(int16_t) * (size_t)off[B];
  FBCHK(e->wav.ensure(bytes));
  FBCHK(e->wav_tf.ensure(bytes));
  FBCHK(e->wav_off.ensure(sizeof(int64_t) * (B + 1)));
  FBCHK(h2d(e, e->wav.p, wav, bytes));
  FBCHK(h2d(e, e->wav_off.p, off, sizeof(int64_t) * (B + 1)));
  fb_launch_input_transform(e->stream, e->tf, e->tf_taps.as<double>(), e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, n_max,
                            e->wav_tf.as<int16_t>(), nullptr);
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out, e->wav_tf.p, bytes));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// ---- over-the-air channel (the contract: include/fakebob_hip.h)
extern "C" int fb_set_air_channel(fb_engine *e, const fb_air_params *p) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  FbAir set = {};
  if (p && p->taps != 0) {  // everything is checked before anything is changed: a refusal keeps the previous setting
    if (p->taps < 2 || p->taps > 4096) return fb_fail(FB_E_ARG, "a room response of %d taps: 2 .. 4096, or 0 for none", p->taps);
    if (p->predelay < 1 || p->predelay > p->taps - 1) return fb_fail(FB_E_ARG, "predelay %d outside 1 .. taps - 1 = %d", p->predelay, p->taps - 1);
    if (!(p->amp >= 0.0 && p->amp <= 16384.0))  // (NaN fails the comparisons too)
      return fb_fail(FB_E_ARG, "amp = %g is not in 0 .. 16384", p->amp);
    if (!(p->rho_lo > 0.0 && p->rho_lo <= p->rho_hi && p->rho_hi <= 1.0))
      return fb_fail(FB_E_ARG, "decay range %g .. %g: 0 < rho_lo <= rho_hi <= 1", p->rho_lo, p->rho_hi);
    set.L = p->taps;
    set.d = p->predelay;
    set.amp = p->amp;
    set.rho_lo = p->rho_lo;
    set.rho_hi = p->rho_hi;
  }
  e->air = set;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was scored through the previous setting
  return FB_OK;
}

extern "C" int fb_debug_air_taps(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica, int16_t *taps,
                                 float *z, uint32_t *w) {
  if (!e || !taps || replica < 0 || replica > 31) return fb_fail(FB_E_ARG, "bad argument");
  if (e->air.L == 0) return fb_fail(FB_E_STATE, "no over-the-air channel is set: fb_set_air_channel first");
  const int L = e->air.L, L4 = 4 * ((L + 3) / 4);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf d_t, d_z, d_w;
  FBCHK(d_t.ensure(sizeof(int16_t) * (size_t)L));
  FBCHK(d_z.ensure(sizeof(float) * (size_t)L4));
  FBCHK(d_w.ensure(sizeof(uint32_t)));
  fb_launch_air_taps(e->stream, fb_air_key(FbRngPoint{seed, stream, epoch, utt}, e->air, 1), replica, 1, d_t.as<int16_t>(), d_z.as<float>(),
                     d_w.as<uint32_t>(), nullptr);
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, taps, d_t.p, sizeof(int16_t) * (size_t)L));
  if (z) FBCHK(d2h(e, z, d_z.p, sizeof(float) * (size_t)L));
  if (w) FBCHK(d2h(e, w, d_w.p, sizeof(uint32_t)));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_debug_air_convolve(fb_engine *e, const int16_t *wav, const int64_t *off, int B, const int16_t *taps, int L, int16_t *out) {
  if (!e || !wav || !off || !taps || !out || B <= 0 || B > 65535 || L < 2 || L > 4096) return fb_fail(FB_E_ARG, "bad argument");
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b];
    if (n <= 0) return fb_fail(FB_E_ARG, "utterance %d is empty", b);
    if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance %d longer than 2^31 samples", b);
    n_max = std::max(n_max, n);
  }
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t bytes = sizeof(int16_t) * (size_t)off[B];
  DevBuf d_in, d_off, d_t, d_out;
  FBCHK(d_in.ensure(bytes));
  FBCHK(d_out.ensure(bytes));
  FBCHK(d_off.ensure(sizeof(int64_t) * (size_t)(B + 1)));
  FBCHK(d_t.ensure(sizeof(int16_t) * (size_t)B * (size_t)L));
  FBCHK(h2d(e, d_in.p, wav, bytes));
  FBCHK(h2d(e, d_off.p, off, sizeof(int64_t) * (size_t)(B + 1)));
  FBCHK(h2d(e, d_t.p, taps, sizeof(int16_t) * (size_t)B * (size_t)L));
  fb_launch_air_conv(e->stream, d_in.as<int16_t>(), d_off.as<int64_t>(), B, 1, 1, n_max, d_t.as<int16_t>(), L, d_out.as<int16_t>(),
                     d_off.as<int64_t>(), nullptr, nullptr);
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out, d_out.p, bytes));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// ---- telephone-line codec (the contract: include/fakebob_hip.h)
extern "C" int fb_set_codec(fb_engine *e, int kind) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (kind != FB_CODEC_NONE && kind != FB_CODEC_ULAW && kind != FB_CODEC_ALAW && kind != FB_CODEC_ADPCM)
    return fb_fail(FB_E_ARG, "codec kind %d: 0 (none), 1 (mu-law), 2 (A-law) or 3 (IMA ADPCM)", kind);
  e->codec = kind;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was scored through the previous setting
  return FB_OK;
}

extern "C" int fb_debug_codec(fb_engine *e, int kind, const int16_t *wav, const int64_t *off, int B, int16_t *out) {
  if (!e || !wav || !off || !out || B <= 0 || B > 65535) return fb_fail(FB_E_ARG, "bad argument");
  if (kind != FB_CODEC_ULAW && kind != FB_CODEC_ALAW && kind != FB_CODEC_ADPCM) return fb_fail(FB_E_ARG, "codec kind %d: 1, 2 or 3", kind);
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b];
    if (n <= 0) return fb_fail(FB_E_ARG, "utterance %d is empty", b);
    if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance %d longer than 2^31 samples", b);
    n_max = std::max(n_max, n);
  }
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  const size_t bytes = sizeof(int16_t) * (size_t)off[B];
  DevBuf d_in, d_off, d_out;
  FBCHK(d_in.ensure(bytes));
  FBCHK(d_out.ensure(bytes));
  FBCHK(d_off.ensure(sizeof(int64_t) * (size_t)(B + 1)));
  FBCHK(h2d(e, d_in.p, wav, bytes));
  FBCHK(h2d(e, d_off.p, off, sizeof(int64_t) * (size_t)(B + 1)));
  fb_launch_codec(e->stream, kind, d_in.as<int16_t>(), d_off.as<int64_t>(), B, n_max, d_out.as<int16_t>(), nullptr);
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out, d_out.p, bytes));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// ---- expectation over transformation
extern "C" int fb_set_eot(fb_engine *e, int r) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (r < 1 || r > 32) return fb_fail(FB_E_ARG, "EOT size %d outside 1 .. 32", r);
  if ((e->comp_K1 + 1) * r > 32)
    return fb_fail(FB_E_ARG, "EOT size %d with %d utterances (fb_set_companions): utterances * eot is at most 32", r, e->comp_K1 + 1);
  e->eot = r;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was laid out for the previous size
  return FB_OK;
}

// ---- voted decisions: fb_attack_pso / _kenansville / _hsj under EOT and companions
extern "C" int fb_set_query_eot(fb_engine *e, int quorum) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (quorum != FB_QUORUM_OFF && quorum != FB_QUORUM_MAJORITY && (quorum < 1 || quorum > 32))
    return fb_fail(FB_E_ARG, "quorum %d: 0 (off), -1 (majority) or 1 .. 32", quorum);
  e->query_quorum = quorum;
  return FB_OK;
}

// ---- companion utterances: a universal perturbation
extern "C" int fb_set_companions(fb_engine *e, const int16_t *wav, int K1, int64_t N) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (K1 != 0) {
    if (K1 < 1 || K1 > 31) return fb_fail(FB_E_ARG, "%d companions: 1 .. 31, or 0 for none", K1);
    if (!wav) return fb_fail(FB_E_ARG, "wav is NULL");
    if (N < 1 || N > 0x7fffffffLL) return fb_fail(FB_E_ARG, "companions of %lld samples: 1 .. 2^31 - 1", (long long)N);
    if ((K1 + 1) * e->eot > 32)
      return fb_fail(FB_E_ARG, "%d utterances under fb_set_eot(%d): utterances * eot is at most 32", K1 + 1, e->eot);
    HIPCHK(hipSetDevice(e->device));
    FBCHK(sync_stream(e));  // (nothing in flight reads the previous companions)
    DevBuf nb;              // the previous setting stays whole until the new one is on the device
    FBCHK(nb.ensure(sizeof(int16_t) * (size_t)K1 * (size_t)N));
    FBCHK(h2d(e, nb.p, wav, sizeof(int16_t) * (size_t)K1 * (size_t)N));
    FBCHK(sync_stream(e));
    e->comp_wav = std::move(nb);
  }
  e->comp_K1 = K1;
  e->comp_N = K1 ? N : 0;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was laid out for the previous setting
  return FB_OK;
}

extern "C" int fb_debug_compose(fb_engine *e, const int16_t *q, int B, int64_t N, const int16_t *a0, int r, uint64_t seed,
                                uint32_t stream, uint32_t epoch, int16_t *out) {
  if (!e || !q || !a0 || !out || B <= 0 || N <= 0 || N > 0x7fffffffLL || r < 1) return fb_fail(FB_E_ARG, "bad argument");
  const int K = e->comp_K1 + 1, R = K * r;
  if (R > 32 || (int64_t)B * R > 65535) return fb_fail(FB_E_ARG, "utterances * r = %d replicas per row (at most 32), %d rows", R, B);
  if (e->comp_K1 > 0 && N != e->comp_N)
    return fb_fail(FB_E_ARG, "rows of %lld samples, the companions (fb_set_companions) have %lld", (long long)N, (long long)e->comp_N);
  std::vector<int64_t> off((size_t)B * R + 1);
  for (size_t b = 0; b < off.size(); ++b) off[b] = (int64_t)b * N;
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // the scoring batch layout no longer describes e->wav / e->wav_off
  e->bench_it = e->nes_rec.iter = -1;
  const size_t bytes = sizeof(int16_t) * (size_t)B * (size_t)N;
  DevBuf d_a0;
  FBCHK(e->wav.ensure(bytes));
  FBCHK(e->wav_tf.ensure(bytes * R));
  FBCHK(e->wav_off.ensure(sizeof(int64_t) * off.size()));
  FBCHK(d_a0.ensure(sizeof(int16_t) * (size_t)N));
  FBCHK(h2d(e, e->wav.p, q, bytes));
  FBCHK(h2d(e, e->wav_off.p, off.data(), sizeof(int64_t) * off.size()));
  FBCHK(h2d(e, d_a0.p, a0, sizeof(int16_t) * (size_t)N));
  const FbTfComp cn{K, N, d_a0.as<int16_t>(), e->comp_wav.as<int16_t>()};
  const int16_t *res = e->wav_tf.as<int16_t>();
  if (e->play_S > 0) {  // (fb_set_play_offset) the NES calls' own path whole: k_play_compose, the air and chain launches on its rows,
                        // and the codec where one is set -- in place on the composed buffer when nothing stands between
    FBCHK(check_play_length(e, N));
    FBCHK(e->comp_a0.ensure(sizeof(int16_t) * (size_t)N));
    FBCHK(h2d(e, e->comp_a0.p, a0, sizeof(int16_t) * (size_t)N));
    FbScoreCall call{FbRngPoint{seed, stream, epoch, 0}};
    call.eot = r;
    call.K = K;
    call.play = e->play_S;
    FBCHK(transformed_wav(e, call, off.data(), B * R, &res));
  } else if (e->air.L > 0)
    FBCHK(launch_air_path(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, R, r, N, (size_t)B * (size_t)N * R, e->wav_off.as<int64_t>(),
                          FbRngPoint{seed, stream, epoch, 0}, K > 1 ? &cn : nullptr, nullptr, &res));
  else
    FBCHK(launch_transform_replicas(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, N, e->wav_tf.as<int16_t>(),
                                    e->wav_off.as<int64_t>(), fb_tf_rnd(FbRngPoint{seed, stream, epoch, 0}, r), &cn, nullptr));
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out, res, bytes * R));
  FBCHK(sync_stream(e));
  return FB_OK;
}

// ---- play offset: the perturbation plays on a loop, the victim speaks whenever they speak
extern "C" int fb_set_play_offset(fb_engine *e, int64_t S) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (S < 0 || S > 0x7ffffffeLL) return fb_fail(FB_E_ARG, "play offset %lld outside 0 .. 2^31 - 2", (long long)S);
  e->play_S = S;
  e->play_launches = 0;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident was laid out for the previous setting
  return FB_OK;
}

extern "C" int fb_debug_play_offsets(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt0, int B, int r,
                                     uint32_t *tau_out) {
  if (!e || !tau_out || B <= 0 || r < 1 || r > 32 || (int64_t)B * r > 65535) return fb_fail(FB_E_ARG, "bad argument");
  if (e->play_S <= 0) return fb_fail(FB_E_STATE, "no play offset is set: fb_set_play_offset first");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf d_tau;
  FBCHK(d_tau.ensure(sizeof(uint32_t) * (size_t)B * r));
  fb_launch_play_offsets(e->stream, fb_play_key(FbRngPoint{seed, stream, epoch, utt0}, e->play_S), r, B * r, d_tau.as<uint32_t>());
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, tau_out, d_tau.p, sizeof(uint32_t) * (size_t)B * r));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_debug_play_route(fb_engine *e, int *n_launches) {
  if (!e || !n_launches) return fb_fail(FB_E_ARG, "null argument");
  *n_launches = e->play_launches;
  return FB_OK;
}

// k_play_compose alone: milliseconds per launch (device events around `reps` launches) on B rows of n samples, K utterances
// (K - 1 companions of a fixed pattern) and eot draws of each, offsets up to S = n - 1 at (seed, stream) = (1, 0)
extern "C" int fb_bench_play_compose(fb_engine *e, int B, int64_t n, int K, int eot, int reps, double *ms) {
  if (!e || !ms || B < 1 || K < 1 || eot < 1 || K * eot > 32 || (int64_t)B * K * eot > 65535 || n < 2 || n > 0x7fffffffLL || reps < 1)
    return fb_fail(FB_E_ARG, "bad argument");
  const int r = K * eot;
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf d_q, d_a0, d_comp, d_out, d_tau;
  FBCHK(d_q.ensure(sizeof(int16_t) * (size_t)B * (size_t)n));
  if (K > 1) {
    FBCHK(d_comp.ensure(sizeof(int16_t) * (size_t)(K - 1) * (size_t)n));
    HIPCHK(hipMemsetAsync(d_comp.p, 0x05, sizeof(int16_t) * (size_t)(K - 1) * (size_t)n, e->stream));
  }
  FBCHK(d_a0.ensure(sizeof(int16_t) * (size_t)n));
  FBCHK(d_out.ensure(sizeof(int16_t) * ((size_t)B * r * (size_t)n + 8)));
  FBCHK(d_tau.ensure(sizeof(uint32_t) * (size_t)B * r));
  HIPCHK(hipMemsetAsync(d_q.p, 0x11, sizeof(int16_t) * (size_t)B * (size_t)n, e->stream));
  HIPCHK(hipMemsetAsync(d_a0.p, 0x07, sizeof(int16_t) * (size_t)n, e->stream));
  const FbTfComp cn{K, n, d_a0.as<int16_t>(), K > 1 ? d_comp.as<int16_t>() : nullptr};
  const FbPlay pk = fb_play_key(FbRngPoint{1, 0, 0, 0}, n - 1);
  auto launch = [&]() { fb_launch_play_compose(e->stream, pk, d_q.as<int16_t>(), cn, eot, B, d_out.as<int16_t>(), d_tau.as<uint32_t>(), nullptr); };
  launch();
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  for (int i = 0; i < reps; ++i) launch();
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
  *ms = (double)t / reps;
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_debug_wb_play_route(fb_engine *e, int *n_launches) {
  if (!e || !n_launches) return fb_fail(FB_E_ARG, "null argument");
  *n_launches = e->wb_play_launches;
  return FB_OK;
}

// Test hook: k_wb_play_compose_t alone, ONE launch, on arrays handed in: cot [K * eot][n], q / a0 [n], comp [K - 1][n] (K = 1: not
// read), tau [K * eot], every one below n
extern "C" int fb_debug_wb_play_compose_t(fb_engine *e, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp,
                                          const uint32_t *tau, int K, int eot, int64_t n, double *grad) {
  if (!e || !cot || !q || !a0 || !tau || !grad || K < 1 || eot < 1 || K * eot > 32 || n <= 0 || (K > 1 && !comp))
    return fb_fail(FB_E_ARG, "bad argument");
  if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "row longer than 2^31 samples");
  const size_t R = (size_t)K * (size_t)eot, ns = (size_t)n;
  for (size_t rho = 0; rho < R; ++rho)
    if ((int64_t)tau[rho] >= n) return fb_fail(FB_E_ARG, "tau[%zu] = %u is not below n = %lld", rho, tau[rho], (long long)n);
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf d_cot, d_q, d_a0, d_comp, d_tau, d_grad;
  FBCHK(d_cot.ensure(sizeof(double) * R * ns));
  FBCHK(d_q.ensure(sizeof(int16_t) * ns));
  FBCHK(d_a0.ensure(sizeof(int16_t) * ns));
  FBCHK(d_tau.ensure(sizeof(uint32_t) * R));
  FBCHK(d_grad.ensure(sizeof(double) * ns));
  FBCHK(h2d(e, d_cot.p, cot, sizeof(double) * R * ns));
  FBCHK(h2d(e, d_q.p, q, sizeof(int16_t) * ns));
  FBCHK(h2d(e, d_a0.p, a0, sizeof(int16_t) * ns));
  FBCHK(h2d(e, d_tau.p, tau, sizeof(uint32_t) * R));
  if (K > 1) {
    FBCHK(d_comp.ensure(sizeof(int16_t) * (size_t)(K - 1) * ns));
    FBCHK(h2d(e, d_comp.p, comp, sizeof(int16_t) * (size_t)(K - 1) * ns));
  }
  e->wb_play_launches = 0;
  fb_launch_wb_play_compose_t(e->stream, d_cot.as<double>(), d_q.as<int16_t>(), d_a0.as<int16_t>(), K > 1 ? d_comp.as<int16_t>() : nullptr,
                              d_tau.as<uint32_t>(), K, eot, n, d_grad.as<double>(), nullptr);
  e->wb_play_launches += 1;
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, grad, d_grad.p, sizeof(double) * ns));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_set_feature_compression(fb_engine *e, double ratio, int iters) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  const bool off = ratio == 0.0 && iters == 0;
  if (!off && (!(ratio > 0.0 && ratio <= 1.0) || iters < 1 || iters > 64))
    return fb_fail(FB_E_ARG, "feature compression takes 0 < ratio <= 1 and 1 .. 64 iterations, or 0 and 0 for none (got %g, %d)", ratio, iters);
  if (!off && e->have_gmm && e->kind == 2)
    return fb_fail(FB_E_STATE, "feature compression: an x-vector system is loaded (k-means discards the frame order a TDNN reads: not in this version)");
  e->feco_ratio = off ? 0.0 : ratio;
  e->feco_iters = iters;
  e->bench_it = e->nes_rec.iter = -1;  // an attack fb_bench_nes left resident ran under the previous setting
  return FB_OK;
}

extern "C" int fb_debug_feature_compress(fb_engine *e, const float *feats, const int *row_off, int B, int r, uint64_t seed,
                                         uint32_t stream, uint32_t epoch, float *out, int *out_off) {
  if (!e || !feats || !row_off || !out || !out_off || B <= 0 || r < 1 || r > 32 || (int64_t)B * r > 65535)
    return fb_fail(FB_E_ARG, "bad argument");
  if (e->feco_iters <= 0) return fb_fail(FB_E_STATE, "feature compression is off: fb_set_feature_compression first");
  const int rows = B * r, D = e->fe.dim;
  if (row_off[0] != 0) return fb_fail(FB_E_ARG, "row_off[0] must be 0");
  int t_max = 0;
  for (int u = 0; u < rows; ++u) {
    if (row_off[u + 1] < row_off[u]) return fb_fail(FB_E_ARG, "row_off decreases at row %d", u);
    t_max = std::max(t_max, row_off[u + 1] - row_off[u]);
  }
  const size_t total = (size_t)row_off[rows];
  if (total == 0 || total * (size_t)D > 0x7fffffffull) return fb_fail(FB_E_ARG, "the batch holds no row, or more than the hook takes");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf d_in, d_off, d_out, d_ooff, d_ws;
  FBCHK(d_in.ensure(sizeof(float) * total * D));
  FBCHK(d_off.ensure(sizeof(int) * (size_t)(rows + 1)));
  FBCHK(d_out.ensure(sizeof(float) * total * D));
  FBCHK(d_ooff.ensure(sizeof(int) * (size_t)(rows + 1)));
  FBCHK(d_ws.ensure(sizeof(int) * FB_FECO_WS_INTS * total));
  FBCHK(h2d(e, d_in.p, feats, sizeof(float) * total * D));
  FBCHK(h2d(e, d_off.p, row_off, sizeof(int) * (size_t)(rows + 1)));
  const FbFeco fc = fb_feco_key(FbRngPoint{seed, stream, epoch, 0}, e->feco_ratio, e->feco_iters, r);
  if (!fb_launch_feature_compress(e->stream, fc, D, d_in.as<float>(), d_off.as<int>(), rows, t_max, d_out.as<float>(),
                                  d_ooff.as<int>(), d_ws.as<int>(), nullptr))
    return fb_fail(FB_E_HIP, "k_feature_compress: the dynamic-LDS opt-in failed");
  HIPCHK(hipGetLastError());
  // (k <= T per row: the compressed rows fit a buffer of the input's size; what lies behind them is left as it was)
  FBCHK(d2h(e, out_off, d_ooff.p, sizeof(int) * (size_t)(rows + 1)));
  FBCHK(sync_stream(e));
  if (out_off[rows] > 0) {
    FBCHK(d2h(e, out, d_out.p, sizeof(float) * (size_t)out_off[rows] * D));
    FBCHK(sync_stream(e));
  }
  return FB_OK;
}

// Test hook: fb_debug_feature_compress with the keep outputs on, then k_wb_feco_t on cotangents handed in.  cots: float64, laid
// out as `out` (row R's k_R x D block at out_off[R]; k_R = max(1, floor(T_R * ratio)), 0 for an empty row -- the caller sizes it
// by that rule, cot_rows = the rows it holds, checked here against the kernel's total); labels: one int per input row; counts: one
// per centre, laid out as out's rows; xbar: float64, laid out as feats.
extern "C" int fb_debug_feature_compress_vjp(fb_engine *e, const float *feats, const int *row_off, int B, int r, uint64_t seed,
                                             uint32_t stream, uint32_t epoch, const double *cots, int cot_rows, int *out_off,
                                             int *labels, int *counts, double *xbar) {
  if (!e || !feats || !row_off || !cots || !out_off || !labels || !counts || !xbar || B <= 0 || r < 1 || r > 32 || (int64_t)B * r > 65535)
    return fb_fail(FB_E_ARG, "bad argument");
  if (e->feco_iters <= 0) return fb_fail(FB_E_STATE, "feature compression is off: fb_set_feature_compression first");
  const int rows = B * r, D = e->fe.dim;
  if (row_off[0] != 0) return fb_fail(FB_E_ARG, "row_off[0] must be 0");
  int t_max = 0;
  for (int u = 0; u < rows; ++u) {
    if (row_off[u + 1] < row_off[u]) return fb_fail(FB_E_ARG, "row_off decreases at row %d", u);
    t_max = std::max(t_max, row_off[u + 1] - row_off[u]);
  }
  const size_t total = (size_t)row_off[rows];
  if (total == 0 || total * (size_t)D > 0x7fffffffull) return fb_fail(FB_E_ARG, "the batch holds no row, or more than the hook takes");
  if (cot_rows < 0 || (size_t)cot_rows > total) return fb_fail(FB_E_ARG, "more cotangent rows than input rows");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->wb_feco_launches = 0;
  DevBuf d_in, d_off, d_out, d_ooff, d_ws, d_lab, d_cnt, d_k, d_cot, d_xbar;
  FBCHK(d_in.ensure(sizeof(float) * total * D));
  FBCHK(d_off.ensure(sizeof(int) * (size_t)(rows + 1)));
  FBCHK(d_out.ensure(sizeof(float) * total * D));
  FBCHK(d_ooff.ensure(sizeof(int) * (size_t)(rows + 1)));
  FBCHK(d_ws.ensure(sizeof(int) * FB_FECO_WS_INTS * total));
  FBCHK(d_lab.ensure(sizeof(int) * total));
  FBCHK(d_cnt.ensure(sizeof(int) * total));
  FBCHK(d_k.ensure(sizeof(int) * (size_t)rows));
  FBCHK(d_cot.ensure(sizeof(double) * total * D));
  FBCHK(d_xbar.ensure(sizeof(double) * total * D));
  FBCHK(h2d(e, d_in.p, feats, sizeof(float) * total * D));
  FBCHK(h2d(e, d_off.p, row_off, sizeof(int) * (size_t)(rows + 1)));
  const FbFeco fc = fb_feco_key(FbRngPoint{seed, stream, epoch, 0}, e->feco_ratio, e->feco_iters, r);
  if (!fb_launch_feature_compress(e->stream, fc, D, d_in.as<float>(), d_off.as<int>(), rows, t_max, d_out.as<float>(),
                                  d_ooff.as<int>(), d_ws.as<int>(), nullptr, d_lab.as<int>(), d_cnt.as<int>(), d_k.as<int>()))
    return fb_fail(FB_E_HIP, "k_feature_compress: the dynamic-LDS opt-in failed");
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out_off, d_ooff.p, sizeof(int) * (size_t)(rows + 1)));
  FBCHK(sync_stream(e));
  if (out_off[rows] != cot_rows)
    return fb_fail(FB_E_ARG, "the cotangents hold %d rows, the kernel wrote %d centres", cot_rows, out_off[rows]);
  std::vector<int> ks((size_t)rows);
  FBCHK(d2h(e, ks.data(), d_k.p, sizeof(int) * (size_t)rows));
  FBCHK(sync_stream(e));
  for (int u = 0; u < rows; ++u)
    if (ks[(size_t)u] != out_off[u + 1] - out_off[u]) return fb_fail(FB_E_HIP, "the kept k of row %d is not the row's centre count", u);
  if (cot_rows > 0) FBCHK(h2d(e, d_cot.p, cots, sizeof(double) * (size_t)cot_rows * D));
  fb_launch_wb_feco_t(e->stream, D, d_lab.as<int>(), d_cnt.as<int>(), d_off.as<int>(), d_ooff.as<int>(), 0, rows, t_max, true,
                      d_cot.as<double>(), d_xbar.as<double>(), nullptr);
  e->wb_feco_launches += 1;
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, labels, d_lab.p, sizeof(int) * total));
  if (cot_rows > 0) FBCHK(d2h(e, counts, d_cnt.p, sizeof(int) * (size_t)cot_rows));
  FBCHK(d2h(e, xbar, d_xbar.p, sizeof(double) * total * D));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_debug_feco_keys(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica, int T,
                                  uint32_t *keys) {
  if (!e || !keys || T <= 0 || replica < 0 || replica > 31) return fb_fail(FB_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf tmp;
  FBCHK(tmp.ensure(sizeof(uint32_t) * (size_t)T));
  // (the keys depend on the point alone, not on the setting)
  fb_launch_feco_keys(e->stream, fb_feco_key(FbRngPoint{seed, stream, epoch, utt}, e->feco_ratio, e->feco_iters), replica, T, tmp.as<uint32_t>());
  HIPCHK(hipMemcpyAsync(keys, tmp.p, sizeof(uint32_t) * (size_t)T, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return FB_OK;
}

extern "C" int fb_debug_tf_noise(fb_engine *e, uint64_t seed, uint32_t stream, uint32_t epoch, uint32_t utt, int replica,
                                 int stage, int64_t i0, int64_t n, float *z) {
  if (!e || !z || i0 < 0 || n <= 0 || i0 + n > 0x7fffffffLL || replica < 0 || replica > 31 || stage < 0 || stage >= FB_TF_MAX_STAGES)
    return fb_fail(FB_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  DevBuf tmp;
  FBCHK(tmp.ensure(sizeof(float) * (size_t)n));
  fb_launch_tf_noise(e->stream, fb_tf_rnd(FbRngPoint{seed, stream, epoch, utt}), replica, stage, i0, n, tmp.as<float>());
  HIPCHK(hipMemcpyAsync(z, tmp.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return FB_OK;
}

extern "C" int fb_debug_input_transform_eot(fb_engine *e, const int16_t *wav, const int64_t *off, int B, int r, uint64_t seed,
                                            uint32_t stream, uint32_t epoch, int16_t *out) {
  if (!e || !wav || !off || !out || B <= 0 || r < 1 || r > 32 || (int64_t)B * r > 65535) return fb_fail(FB_E_ARG, "bad argument");
  if (off[0] != 0) return fb_fail(FB_E_ARG, "off[0] must be 0");
  int64_t n_max = 0;
  std::vector<int64_t> out_off((size_t)B * r + 1, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b];
    if (n <= 0) return fb_fail(FB_E_ARG, "utterance %d is empty", b);
    if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance %d longer than 2^31 samples", b);
    n_max = std::max(n_max, n);
    for (int j = 0; j < r; ++j) out_off[(size_t)b * r + j + 1] = out_off[(size_t)b * r + j] + n;
  }
  HIPCHK(hipSetDevice(e->device));
  FBCHK(sync_stream(e));
  e->cached_B = -1;  // the scoring batch layout no longer describes e->wav / e->wav_off
  e->bench_it = e->nes_rec.iter = -1;
  const size_t bytes = sizeof(int16_t) * (size_t)off[B];
  DevBuf d_out_off;
  FBCHK(e->wav.ensure(bytes));
  FBCHK(e->wav_tf.ensure(bytes * r));
  FBCHK(e->wav_off.ensure(sizeof(int64_t) * (B + 1)));
  FBCHK(d_out_off.ensure(sizeof(int64_t) * out_off.size()));
  FBCHK(h2d(e, e->wav.p, wav, bytes));
  FBCHK(h2d(e, e->wav_off.p, off, sizeof(int64_t) * (B + 1)));
  FBCHK(h2d(e, d_out_off.p, out_off.data(), sizeof(int64_t) * out_off.size()));
  const int16_t *res = e->wav_tf.as<int16_t>();
  if (e->air.L > 0)
    FBCHK(launch_air_path(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, r, r, n_max, (size_t)off[B] * r, d_out_off.as<int64_t>(),
                          FbRngPoint{seed, stream, epoch, 0}, nullptr, nullptr, &res));
  else
    FBCHK(launch_transform_replicas(e, e->wav.as<int16_t>(), e->wav_off.as<int64_t>(), B, n_max, e->wav_tf.as<int16_t>(),
                                    d_out_off.as<int64_t>(), fb_tf_rnd(FbRngPoint{seed, stream, epoch, 0}, r), nullptr, nullptr));
  HIPCHK(hipGetLastError());
  FBCHK(d2h(e, out, res, bytes * r));
  FBCHK(sync_stream(e));
  return FB_OK;
}

extern "C" int fb_set_dither_seed(fb_engine *e, uint64_t seed) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  e->dither_seed = seed;
  e->dither_serial = 0;
  return FB_OK;
}

static int debug_feats(fb_engine *e, const int16_t *wav, int64_t n, const FbRngPoint *pt, float *feats, int *Tv, int *T_out);
extern "C" int fb_debug_feats(fb_engine *e, const int16_t *wav, int64_t n, float *feats, int *Tv, int *T_out) {
  return debug_feats(e, wav, n, nullptr, feats, Tv, T_out);
}
extern "C" int fb_debug_feats_dither(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream,
                                     uint32_t epoch, uint32_t utt, float *feats, int *Tv, int *T_out) {
  const FbRngPoint pt{seed, stream, epoch, utt};
  return debug_feats(e, wav, n, &pt, feats, Tv, T_out);
}
static int debug_feats(fb_engine *e, const int16_t *wav, int64_t n, const FbRngPoint *pt, float *feats, int *Tv, int *T_out) {
  if (!feats || !Tv) return fb_fail(FB_E_ARG, "null output");
  FBCHK(debug_frontend(e, wav, n, pt));
  const int T = e->h_frame_off[1];
  int tv = 0;
  FBCHK(d2h(e, &tv, e->tv.p, sizeof(int)));
  FBCHK(sync_stream(e));
  if (tv > 0)
    HIPCHK(hipMemcpy(feats, e->feats.p, sizeof(float) * (size_t)tv * e->fe.dim, hipMemcpyDeviceToHost));
  *Tv = tv;
  if (T_out) *T_out = T;
  return FB_OK;
}

// Test hook: the GMM backward alone -- the launches of wb_enqueue's k_wb_gmm_bwd / k_wb_sum_models -- on Tv rows of features
// and weights w[M] handed in as they are; out[Tv][D] float64
extern "C" int fb_debug_gmm_feat_grad(fb_engine *e, const float *feats, int Tv, const double *w, double *out) {
  if (!e || !feats || !w || !out || Tv <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 0) return fb_fail(FB_E_STATE, "load a diagonal GMM system first");
  HIPCHK(hipSetDevice(e->device));
  const FbGmmDev &g = e->gmm;
  FBCHK(sync_stream(e));
  FBCHK(wb_prepare(e, 1, Tv, true));
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)Tv * g.D));
  FBCHK(e->row_off.ensure(sizeof(int) * 2));
  const int rows_host[2] = {0, Tv};
  HIPCHK(hipMemcpy(e->feats.p, feats, sizeof(float) * (size_t)Tv * g.D, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->row_off.p, rows_host, sizeof(rows_host), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->wb_w.p, w, sizeof(double) * (size_t)g.M, hipMemcpyHostToDevice));
  e->last_total_frames = 0;  // the feature buffer no longer belongs to a scored batch
  wb_launch_gmm_backward(e, e->row_off.as<int>() + 1, Tv, nullptr);
  FBCHK(d2h(e, out, e->wb_g.p, sizeof(double) * (size_t)Tv * g.D));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  return FB_OK;
}

// Test hook: the front-end backward alone -- the forward of fb_debug_feats, then wb_enqueue's front-end launches -- with a
// cotangent cot[Tv][dim] on the compacted rows handed in: dwav[n] = d <cot, feats> / d wav (int16 units, float64) and the
// voiced mask voiced[T] (0 / 1) the backward used
extern "C" int fb_debug_frontend_vjp(fb_engine *e, const int16_t *wav, int64_t n, const double *cot, double *dwav,
                                     unsigned char *voiced) {
  if (!cot || !dwav) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(debug_frontend(e, wav, n));
  const int T = e->h_frame_off[1];
  int tv = 0, status = 0;
  FBCHK(d2h(e, &tv, e->tv.p, sizeof(int)));
  FBCHK(sync_stream(e));
  if (tv <= 0) return fb_fail(FB_E_NO_VOICED, "the utterance has no voiced frames");
  FBCHK(wb_prepare(e, n, T, false));
  FBCHK(h2d(e, e->wb_g.p, cot, sizeof(double) * (size_t)tv * e->fe.dim));
  wb_launch_frontend_vjp(e, e->fe_wav, 0, n, T, 1.0, e->grad.as<double>(), nullptr);
  std::vector<int> rank((size_t)T);
  FBCHK(d2h(e, dwav, e->grad.p, sizeof(double) * (size_t)n));
  FBCHK(d2h(e, rank.data(), e->wb_rank.p, sizeof(int) * (size_t)T));
  FBCHK(d2h(e, &status, e->wb_status.p, sizeof(int)));
  FBCHK(sync_stream(e));
  HIPCHK(hipGetLastError());
  FBCHK(wb_status_check(e, status));
  if (voiced) for (int t = 0; t < T; ++t) voiced[t] = rank[t] >= 0 ? 1 : 0;
  return FB_OK;
}

extern "C" int fb_debug_wb_route(fb_engine *e, int *info) {
  if (!e || !info) return fb_fail(FB_E_ARG, "null argument");
  for (int i = 0; i < FB_WB_ROUTE_N; ++i) info[i] = e->wb_route[i];
  return FB_OK;
}

// Test hook: the defences alone -- the forward of the chain and the codec on ONE row for the engine's r replicas at the given
// point, as an attack iteration's scoring call runs it, then wb_enqueue's transposes on a cotangent per replica
extern "C" int fb_debug_defence_vjp(fb_engine *e, const int16_t *wav, int64_t n, uint64_t seed, uint32_t stream, int iter,
                                    const double *cot, double *dwav, int16_t *out) {
  if (!e || !wav || !cot || !dwav || n <= 0 || iter < 0) return fb_fail(FB_E_ARG, "bad argument");
  if (n > 0x7fffffffLL) return fb_fail(FB_E_LIMIT, "utterance longer than 2^31 samples");
  const bool air = e->air.L > 0;
  if (air && !e->wb_air) return fb_fail(FB_E_STATE, "white-box gradients: an air channel is set (fb_set_air_channel: clear it)");
  if (e->comp_K1 > 0) return fb_fail(FB_E_STATE, "white-box gradients: companions are set (fb_set_companions: clear them)");
  if (num_frames(e->cfg, n) <= 0) return fb_fail(FB_E_ARG, "audio shorter than one frame");
  HIPCHK(hipSetDevice(e->device));
  e->bench_it = e->nes_rec.iter = -1;
  memset(e->wb_route, 0, sizeof(e->wb_route));
  e->wb_air_launches = 0;
  const int r = e->eot;
  FBCHK(prepare_nes_replicas(e, n, 1, false));  // (no contract point of the play offset: the forward below leaves call.play at 0)
  FBCHK(e->wb_gj.ensure(sizeof(double) * (size_t)n));
  FBCHK(e->grad.ensure(sizeof(double) * (size_t)n));
  FBCHK(h2d(e, e->wav.p, wav, sizeof(int16_t) * (size_t)n));
  const FbRngPoint pt{seed, stream, (uint32_t)iter, 0};
  FbScoreCall call{pt};
  call.eot = r;
  call.keep_air_sat = air;
  const int16_t *res = nullptr;
  FBCHK(transformed_wav(e, call, e->h_wav_off.data(), r, &res));
  if (out) FBCHK(d2h(e, out, res, sizeof(int16_t) * (size_t)n * r));
  if (air) {  // wb_enqueue's order: every replica's cotangent to its slot (through the chain's transpose when a chain is set),
              // then the channel's transpose of all r in one launch; dwav row j = k_air_conv_t's row j, not the replicas' sum
    const size_t bytes = sizeof(double) * (size_t)r * (size_t)n;
    FBCHK(e->wb_air_cot.ensure(bytes));
    FBCHK(e->wb_air_dx.ensure(bytes));
    if (e->tf.n == 0) FBCHK(h2d(e, e->wb_air_cot.p, cot, bytes));
    for (int j = 0; j < r && e->tf.n > 0; ++j) {
      FBCHK(h2d(e, e->wb_gj.p, cot + (size_t)j * n, sizeof(double) * (size_t)n));
      FBCHK(wb_launch_chain_t(e, pt, j, n, e->wb_gj.as<double>(), e->wb_air_cot.as<double>() + (size_t)j * (size_t)n, false, nullptr, false));
      FBCHK(sync_stream(e));
    }
    fb_launch_air_conv_t(e->stream, e->wb_air_cot.as<double>(), e->wb_air_sat.as<unsigned char>(), r, n, e->air_taps.as<int16_t>(), e->air.L,
                         e->wb_air_dx.as<double>(), nullptr);
    e->wb_air_launches += 1;
    FBCHK(d2h(e, dwav, e->wb_air_dx.p, bytes));
    FBCHK(sync_stream(e));
    HIPCHK(hipGetLastError());
    return FB_OK;
  }
  for (int j = 0; j < r; ++j) {
    FBCHK(h2d(e, e->wb_gj.p, cot + (size_t)j * n, sizeof(double) * (size_t)n));
    FBCHK(wb_launch_chain_t(e, pt, j, n, e->wb_gj.as<double>(), e->grad.as<double>(), false, nullptr, false));
    FBCHK(d2h(e, dwav + (size_t)j * n, e->grad.p, sizeof(double) * (size_t)n));
    FBCHK(sync_stream(e));
  }
  HIPCHK(hipGetLastError());
  return FB_OK;
}

extern "C" int fb_stats(fb_engine *e, int64_t *scored_utts, int64_t *scored_frames, int64_t *voiced_frames,
                        int64_t *nes_iters) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (scored_utts) *scored_utts = e->scored_utts;
  if (scored_frames) *scored_frames = e->scored_frames;
  if (voiced_frames) *voiced_frames = e->voiced_frames;
  if (nes_iters) *nes_iters = e->nes_iters;
  return FB_OK;
}

// Test hook: the GMM kernel the engine runs for scoring, on T rows of features handed in as they are (no front-end),
// per-frame log-likelihoods out[m * T + t] -- the chunk partials merged here in float64.
extern "C" int fb_debug_gmm_frames(fb_engine *e, const float *feats, int T, double *out) {
  if (!e || !feats || !out || T <= 0) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->kind != 0) return fb_fail(FB_E_STATE, "no GMM system loaded");
  HIPCHK(hipSetDevice(e->device));
  const FbGmmDev &g = e->gmm;
  FBCHK(sync_stream(e));
  choose_launch_shape(e);
  const int n_chunks = choose_chunks(g, T, true);
  FBCHK(e->feats.ensure(sizeof(float) * (size_t)T * g.D));
  FBCHK(e->row_off.ensure(sizeof(int) * 2));
  FBCHK(e->part_m.ensure(sizeof(float) * (size_t)n_chunks * g.M * T));
  FBCHK(e->part_s.ensure(sizeof(float) * (size_t)n_chunks * g.M * T));
  const int rows_host[2] = {0, T};
  HIPCHK(hipMemcpy(e->feats.p, feats, sizeof(float) * (size_t)T * g.D, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->row_off.p, rows_host, sizeof(rows_host), hipMemcpyHostToDevice));
  fb_launch_gmm(e->stream, g, e->feats.as<float>(), e->row_off.as<int>() + 1, T, n_chunks, e->part_m.as<float>(),
                e->part_s.as<float>(), &e->shape_gmm);
  HIPCHK(hipGetLastError());
  FBCHK(sync_stream(e));
  std::vector<float> pm((size_t)n_chunks * g.M * T), ps(pm.size());
  HIPCHK(hipMemcpy(pm.data(), e->part_m.p, sizeof(float) * pm.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ps.data(), e->part_s.p, sizeof(float) * ps.size(), hipMemcpyDeviceToHost));
  for (int m = 0; m < g.M; ++m)
    for (int t = 0; t < T; ++t) {
      double mx = -INFINITY, sum = 0.0;
      for (int c = 0; c < n_chunks; ++c) mx = std::max(mx, (double)pm[((size_t)c * g.M + m) * T + t]);
      for (int c = 0; c < n_chunks; ++c) {
        const size_t o = ((size_t)c * g.M + m) * T + t;
        sum += (double)ps[o] * exp((double)pm[o] - mx);
      }
      out[(size_t)m * T + t] = mx + log(sum);
    }
  e->last_total_frames = 0;  // the feature buffer no longer belongs to a scored batch
  return FB_OK;
}

extern "C" int fb_bench_gmm_kernel(fb_engine *e, int reps, double *ms_avg, int64_t *rows) {
  if (!e || reps <= 0 || !ms_avg) return fb_fail(FB_E_ARG, "bad argument");
  if (!e->have_gmm || e->last_total_frames <= 0) return fb_fail(FB_E_STATE, "score a batch first");
  HIPCHK(hipSetDevice(e->device));
  const int B = e->last_B, tf = e->last_total_frames;
  FBCHK(sync_stream(e));
  FbGmmDev gb = e->gmm;   // the launch shape of the last batch (FB_GMM_SUB: the other one -- bench.py times both)
  if (const char *sv = getenv("FB_GMM_SUB")) gb.fxw_sub = atoi(sv);
  fb_launch_gmm(e->stream, gb, e->feats.as<float>(), e->row_off.as<int>() + B, tf, e->last_chunks,
                e->part_m.as<float>(), e->part_s.as<float>());
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  for (int r = 0; r < reps; ++r)
    fb_launch_gmm(e->stream, gb, e->feats.as<float>(), e->row_off.as<int>() + B, tf, e->last_chunks,
                  e->part_m.as<float>(), e->part_s.as<float>());
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  *ms_avg = (double)ms / reps;
  if (rows) {
    int r = 0;
    HIPCHK(hipMemcpy(&r, e->row_off.as<int>() + B, sizeof(int), hipMemcpyDeviceToHost));
    *rows = r;
  }
  return FB_OK;
}

extern "C" int fb_bench_nes(fb_engine *e, const fb_nes_params *p, const double *audio, int64_t N, int warmup,
                            int iters, int time_gmm, double *ms_total, double *ms_gmm, int64_t *voiced_rows) {
  if (!audio || !ms_total || iters <= 0) return fb_fail(FB_E_ARG, "bad argument");
  FBCHK(check_params(e, p, N));
  HIPCHK(hipSetDevice(e->device));
  const int half = p->samples_per_draw / 2, B = 2 * half + 1;
  const FbScorer sc{FB_SCORER_NATIVE};
  const FbLoopKnobs kn = loop_knobs(e, sc);
  const bool resume = warmup < 0;  // continue the attack a previous call left on the device: nothing is uploaded or reset
  if (resume) {
    if (e->bench_N != N || e->bench_B != B || e->bench_it < 0)
      return fb_fail(FB_E_STATE, "fb_bench_nes(warmup < 0): no attack of this shape is resident on the engine");
    warmup = 0;
  } else {
    FBCHK(prepare_nes_replicas(e, N, B));
    FBCHK(ensure_nes_buffers(e, N, B));
    FBCHK(attack_start(e, audio, N, half, nullptr));
    cast_a0(e, p, e->audio.as<double>(), N);
    e->bench_it = 0;
    // identical work to fb_attack's loop (early stop disabled for timing)
    FBCHK(ctl_reset(e, p, true, true, nullptr));
    FBCHK(attack_loop(e, p, N, sc, kn, nullptr, 0, warmup, nullptr));
  }
  double gmm_ms = 0.0;
  int64_t vrows = 0;
  const int it0 = (int)e->bench_it + warmup;
  e->nes_rec.iter = -1;
  FBCHK(sync_stream(e));
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  e->time_gmm = time_gmm;
  e->gmm_ms_acc = 0.0;
  e->gmm_launches = 0;
  FBCHK(attack_loop(e, p, N, sc, kn, nullptr, it0, iters, nullptr));
  e->bench_it = it0 + iters;
  e->nes_rec.iter = e->nes_rec.queued;
  e->bench_N = N;
  e->bench_B = B;
  e->nes_iters += warmup + iters;
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  e->time_gmm = 0;
  gmm_ms = e->gmm_ms_acc;  // sum over the timed launches
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  *ms_total = (double)ms;
  {
    int r = 0;
    HIPCHK(hipMemcpy(&r, e->row_off.as<int>() + B * nes_replicas(e), sizeof(int), hipMemcpyDeviceToHost));
    vrows = r;
  }
  if (ms_gmm) *ms_gmm = gmm_ms;
  if (voiced_rows) *voiced_rows = vrows;
  return FB_OK;
}

extern "C" int fb_bench_nes_state(fb_engine *e, double *adver, double *scores, double *loss, double *summary) {
  if (!e) return fb_fail(FB_E_ARG, "null engine");
  if (e->bench_it < 0) return fb_fail(FB_E_STATE, "fb_bench_nes_state: no attack is resident on the engine");
  HIPCHK(hipSetDevice(e->device));
  const int64_t N = e->bench_N;
  const int B = e->bench_B, S = fb_num_speakers(e);
  const size_t n_adv = sizeof(double) * (size_t)N, n_sc = sizeof(double) * (size_t)B * (S > 0 ? S : 1),
               n_loss = sizeof(double) * (size_t)B;
  if (n_adv > e->adver.cap || n_sc > e->scores.cap || n_loss > e->loss.cap || !e->nes_out.p)
    return fb_fail(FB_E_STATE, "fb_bench_nes_state: the resident attack's buffers no longer match the loaded system");
  if (adver) FBCHK(d2h(e, adver, e->adver.p, n_adv));
  if (scores) FBCHK(d2h(e, scores, e->scores.p, n_sc));
  if (loss) FBCHK(d2h(e, loss, e->loss.p, n_loss));
  HIPCHK(hipMemcpyAsync(e->h_out, e->nes_out.p, sizeof(FbNesDev), hipMemcpyDeviceToHost, e->stream));
  FBCHK(sync_stream(e));
  if (summary) {
    summary[0] = e->h_out->final_loss;
    summary[1] = e->h_out->adver_loss;
    summary[2] = e->h_out->distance;
  }
  return FB_OK;
}
