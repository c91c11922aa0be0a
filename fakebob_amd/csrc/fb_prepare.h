// fb_prepare.h -- the tables the three loaders upload, prepared in GPU-free host code.
//
// fb_load_gmm, fb_load_ivector and fb_set_frontend (fb_engine.hip) validate their arguments, call one of the
// fb_prepare_* functions below, and only then touch the device and the engine: ensure, upload, assign.  Everything here
// is plain C++17 over std::vector: no HIP, no environment, no engine, no global state -- it runs on a machine without
// a GPU (fb_debug_prepare_* of include/fakebob_hip_test.h, tools/host/prepare_check.cpp under the host sanitizers).
// This unit is the single description of the image layouts the GMM kernels read.
//
// A function that can refuse its input returns FB_OK or a negative FB_E_* and writes the message into *err; the engine
// hands both to its caller unchanged.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/fakebob_hip.h"
#include "fb_gmm_limits.h"

// ------------------------------------------------------------------------------------------------ diagonal GMM
// M models of C components over D dimensions in Kaldi's internal form: gconsts [M][C], means_invvars and inv_vars [M][C][D]
struct FbGmmParams {
  int M, C, D;
  const float *gconsts, *miv, *iv;
};

// What FB_GMM_MODE, FB_GMM_DELTA_BUDGET, FB_GMM_DELTA_F6 and FB_GMM_DELTA_P say (fb_engine.hip reads and validates them)
struct FbGmmPrepOptions {
  int forced_mode = 0;     // 0: the rule decides; FB_GMM_MODE_BX3 forces the fallback kernel (tests)
  double budget = 6.0e-6;  // the error budget of the delta rule (default: float32-equivalent scores)
  bool use_f6 = true;      // false: the rule of before the F6 class (P = 2 in the middle, no F6 tiles)
  int forced_p = 0;        // 1, 2, 3, 6: the same class in every tile (tests / worst-case benchmark); 0: the rule decides
};

// groups of models with bitwise-identical inv_vars, and the items of a component tile: per group its quadratic (Q) item
// (any negative entry: -1 - group) followed by the group's models
struct FbGmmGroups {
  std::vector<int> group_of, group_rep, item_model;
};
FbGmmGroups fb_gmm_group_by_variance(const FbGmmParams &g);

// the power-of-two operand scalings of k_gmm_fx2 (FbGmmDev::kx ..); ok == false: a parameter does not fit f16, bx3 scores
struct FbGmmFxScaling {
  bool ok;
  int kl, kx, kacc, kq, kx2;
};
FbGmmFxScaling fb_gmm_fx2_scaling(const FbGmmParams &g, int NKF, bool want_delta);

// Where K position k (0 .. 16 * n_chunks - 1) of component cc (0 .. 31) of partial term `term` stands in an item's MFMA
// fragment image [terms][n_chunks][64 lanes] x 8 values: lane = 32 * (k % 16 / 8) + cc holds places 8 * (k % 16 / 8) .. + 7
// of chunk k / 16.  Every image below (fx2, bx3, delta) is laid out by this one function.
static inline size_t fb_gmm_frag_index(int term, int n_chunks, int k, int cc) {
  const int ch = k / 16, hh = (k % 16) / 8, i = k % 8, lane = hh * 32 + cc;
  return (((size_t)term * n_chunks + ch) * 64 + lane) * 8 + i;
}

// images [n_tiles][n_items] of k_gmm_fx2 (two f16 terms, NKF chunks) and of k_gmm_bx3 (three bf16 terms, NK chunks)
std::vector<uint16_t> fb_gmm_pack_fx2(const FbGmmParams &g, const FbGmmGroups &gr, int NKF, const FbGmmFxScaling &sc);
std::vector<uint16_t> fb_gmm_pack_bx3(const FbGmmParams &g, const FbGmmGroups &gr, int NK);

// the delta rule of k_gmm_fx2w (one variance group, C a multiple of 32): the component order, the tile classes, the
// per-dimension balancing and the passes
struct FbGmmDeltaPlan {
  std::vector<int> perm;  // component perm[t * 32 + cc] stands at place cc of tile t
  int t3, t6, t2;         // tiles [0, t3): P = 3, [t3, t6): F6, [t6, t2): P = 2, [t2, n_tiles): P = 1
  int want_p;             // what most tiles run
  double delta_rms;       // the equal-weight shift statistic fb_gmm_kernel_variant reports
  std::vector<int> kd, kq;  // [16 * NKF]: the frames' x_d is multiplied by 2^kd[d], x_d^2 by 2^kq[d]
  bool fits;              // every balanced parameter is inside f16's range (else k_gmm_fx2 scores the system)
  int n_pass, pass_lo[FB_FXW_MAX_PASS + 1];  // pass p scores the base model and models pass_lo[p] .. pass_lo[p + 1] - 1
  int tile_p(int t) const { return t < t3 ? 3 : (t < t6 ? 6 : (t < t2 ? 2 : 1)); }
};
FbGmmDeltaPlan fb_gmm_delta_plan(const FbGmmParams &g, int NKF, const FbGmmPrepOptions &opt);
// images [n_tiles][2 + models of the pass] of one pass: {Q, base model, the pass's deltas}
std::vector<uint16_t> fb_gmm_pack_delta_pass(const FbGmmParams &g, int NKF, const FbGmmDeltaPlan &plan, int pass);
// FbGmmDev::anchor; *fits goes false when one of its f16 copies would overflow
std::vector<float> fb_gmm_anchor_table(const FbGmmParams &g, int NKF, const FbGmmDeltaPlan &plan, bool *fits);

// The F6 item of the delta images (the layout is described at fb_gmm_f6_pack_component): byte offsets inside the 10 KB item
enum {
  FB_F6_B0_LO = 5120,    // block 0 (e2m3) bits 0 .. 127: [64 lanes] x 16 B
  FB_F6_B0_HI = 6144,    // ... bits 128 .. 191: [64] x 8
  FB_F6_B1_LO = 6656,    // block 1 (e2m3) likewise
  FB_F6_B1_HI = 7680,
  FB_F6_BL = 8192,       // block L (e2m1): [64] x 16
  FB_F6_B2_LO = 9216,    // block 2 (e2m3, lanes kh = 0): [32] x 16
  FB_F6_B2_HI = 9728,    // ... [32] x 8
  FB_F6_SCALES = 9984,   // [64] x 4: the scale bytes (e8m0: 2^(byte - 127)) of blocks 0, 1, L, 2
};
int fb_f6_scale_for(const double *val, int n, double top);  // smallest e with max |val| 2^-e <= top
int fb_f6_code_e2m3(double v, int ex, double *got);         // nearest code (ties to even), |v| 2^-ex <= 7.5; *got = what it decodes to
int fb_f6_code_e2m1(double v, int ex, double *got);         // 0, .5, 1, 1.5, 2, 3, 4, 6
void fb_f6_put6(uint64_t (&bits)[3], int u, int code);      // code into bits [6u, 6u + 6)
// the fp6 / fp4 operands of component place cc of one F6 item: vv[k] the balanced linear parameters of its D dimensions,
// aa[k] their leading f16 terms, mean[k] the component's mean in the frames' balanced units; what the codes leave out
// at that mean is added to *cst, the item's constant
void fb_gmm_f6_pack_component(uint8_t *item, int cc, int D, const double *vv, const double *aa, const double *mean,
                              double *cst);

struct FbGmmPrepared {
  int M = 0, C = 0, D = 0, n_tiles = 0, n_items = 0, n_groups = 0;
  int mode = 0, NK = 0, NKF = 0;
  int kx = 0, kx2 = 0, kacc = 0;
  int delta_p = 0, delta_t3 = 0, delta_t6 = 0, delta_t2 = 0;  // delta_p == 0: no delta images, the others are 0 too
  int n_pass = 0, pass_lo[FB_FXW_MAX_PASS + 1] = {1, 1, 1, 1};
  double delta_rms = 0.0;
  bool too_many_for_wide = false;  // one variance group with more models than k_gmm_fx2w's passes take (the loader's note)
  std::vector<int> perm;           // the delta images' component order (empty without a delta plan)
  std::vector<int> item_model;
  std::vector<uint16_t> fx, bx;    // the image of `mode` is filled, the other is empty
  std::vector<uint16_t> fd[FB_FXW_MAX_PASS];
  std::vector<float> anchor;
};
int fb_prepare_gmm(const FbGmmParams &g, const FbGmmPrepOptions &opt, FbGmmPrepared *out, std::string *err);
static inline int fb_gmm_max_wide_models() { return 1 + (FB_FXW_MAX_M - 1) * FB_FXW_MAX_PASS; }

// ------------------------------------------------------------------------------------------------ i-vector
bool fb_host_chol(std::vector<double> &A, int n);  // in-place Cholesky of a dense SPD matrix (lower); false: not PD
void fb_host_chol_solve(const std::vector<double> &Lm, int n, double *b);
// raw i-vector -> PLDA space, host float64 (same math as k_iv_backend; once per enrolled speaker at load time)
void fb_host_backend(const fb_ivector_system *sy, const float *ivec, double *y);

struct FbIvPrepared {
  int triD = 0, triR = 0;
  std::vector<float> dg_gc, dg_miv, dg_iv;  // the diagonalised UBM (fgmm-global-to-gmm): one model for fb_prepare_gmm
  std::vector<float> fg_gc;                 // FullGmm::ComputeGconsts
  std::vector<unsigned char> tri;           // tri_r [triD], tri_c [triD]: row / column of a packed index
  std::vector<double> fg64;                 // [C][triD + D + 1]: the float64 image of the full UBM
  std::vector<double> fgL;                  // [C][50 * 64 + 72 + 2]: the D = 72 Cholesky image; empty when not usable
  std::vector<double> backend;              // mean_vec, ldaT, plda_mean, pldaT, plda_psi, the enrolled speakers
  size_t o_mean = 0, o_lda = 0, o_pm = 0, o_pt = 0, o_psi = 0, o_tr = 0;  // ... their offsets, in doubles
};
int fb_iv_full_to_diag(const fb_ivector_system *sy, FbIvPrepared *out, std::string *err);
std::vector<unsigned char> fb_iv_tri_table(int D);
std::vector<double> fb_iv_fg64_image(const fb_ivector_system *sy, const std::vector<float> &fg_gc);
bool fb_iv_chol_image(const fb_ivector_system *sy, const std::vector<float> &fg_gc, std::vector<double> *rec);  // D == 72
void fb_iv_backend_table(const fb_ivector_system *sy, FbIvPrepared *out);
int fb_prepare_ivector(const fb_ivector_system *sy, FbIvPrepared *out, std::string *err);

// ------------------------------------------------------------------------------------------------ x-vector
// Where K position k of output channel place cc (0 .. 31) of term `term` (0: f16(v), 1: f16(v - term 0)) stands in a
// column tile's image [n_steps][2 terms][64 lanes] x 8 values -- fb_gmm_frag_index's lane rule, the terms of a K step side
// by side (k_xv_affine fetches both with one address)
static inline size_t fb_xv_frag_index(int term, int k, int cc) {
  const int st = k / 16, hh = (k % 16) / 8, i = k % 8, lane = hh * 32 + cc;
  return (((size_t)st * 2 + term) * 64 + lane) * 8 + i;
}
struct FbXvLayerPrepared {
  int din = 0, dout = 0, n_ctx = 0, ctx[FB_XV_MAX_CTX] = {0, 0, 0, 0, 0};
  int K = 0, n_steps = 0;          // n_ctx * din, ceil(K / 16)
  int kw = 0;                      // the image holds W * 2^-kw: max |W| 2^-kw in [2^14, 2^15) (0 for an all-zero layer)
  std::vector<uint16_t> w;         // [ceil(dout / 32)] tiles of fb_xv_frag_index, zeros past dout
  std::vector<float> bias, scale, offset;
  // the transposed image, for the white-box backward (k_wb_xv_affine_t): W' as a [K][dout] matrix in the same layout -- the K
  // columns of the forward are its "channels" ([ceil(K / 32)] tiles), dout its contraction (nt_steps = ceil(dout / 16))
  int nt_steps = 0;
  int kwt = 0;                     // the image holds W' * 2^-kwt, by kw's rule
  std::vector<uint16_t> wt;
};
struct FbXvPrepared {
  int D = 0, n_layers = 0, P = 0, R = 0, max_width = 0;
  FbXvLayerPrepared layer[FB_XV_MAX_LAYERS];
  std::vector<double> segT;        // [2 P][R]: seg_W transposed, float64
  std::vector<double> seg_bias;    // [R]
  FbIvPrepared be;                 // the back end's table (backend, o_*): fb_iv_backend_table's
};
// FB_E_ARG with the limit's name in *err for a system outside the contract's limits (fakebob_hip.h, "x-vector")
int fb_xvector_check(const fb_xvector_system *sy, std::string *err);
int fb_prepare_xvector(const fb_xvector_system *sy, FbXvPrepared *out, std::string *err);

// ------------------------------------------------------------------------------------------------ front-end
struct FbFrontendTables {
  std::vector<double> window, tw_half, tw_full, mel_w, dct, lifter, dscale;
  std::vector<int> mel_first, mel_len, mel_off;
};
// the tables as one device allocation: 64-byte aligned pieces at these byte offsets
struct FbFrontendBlob {
  std::vector<char> bytes;
  size_t o_window = 0, o_twh = 0, o_twf = 0, o_mf = 0, o_ml = 0, o_mo = 0, o_mw = 0, o_dct = 0, o_lift = 0, o_ds = 0;
};
// c has passed fb_set_frontend's argument checks; refuses a bad mel frequency range and a mel bin without an FFT bin
int fb_frontend_tables(const fb_frontend_cfg *c, FbFrontendTables *out, std::string *err);
FbFrontendBlob fb_frontend_pack(const FbFrontendTables &t);
