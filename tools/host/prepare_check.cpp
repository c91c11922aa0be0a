// prepare_check.cpp -- the loaders' host preparation (fakebob_amd/csrc/fb_prepare.h) under the host sanitizers: a small
// deterministic GMM-UBM site, a small i-vector system and the stock front end go through every fb_prepare_* function, and
// every returned buffer is read to its last byte.  CPU only; build and run (tools/README.md):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/host/prepare_check.cpp \
//       fakebob_amd/csrc/fb_prepare_*.cpp -o prepare_check && ./prepare_check
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../fakebob_amd/csrc/fb_prepare.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {  // (0, 1), a 64-bit LCG's upper bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return sqrt(-2.0 * log(uniform())) * cos(2.0 * M_PI * uniform()); }

template <typename T> static double walk(const std::vector<T> &v) {  // reads every byte
  const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
  double s = 0.0;
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) s += p[i];
  return s;
}

struct Gmm {
  int M, C, D;
  std::vector<float> gc, miv, iv;
  FbGmmParams params() const { return FbGmmParams{M, C, D, gc.data(), miv.data(), iv.data()}; }
};
// a UBM and M - 1 mean-only adaptations of it: shared variances, means moved by a few percent of a standard deviation
static Gmm make_gmm(int M, int C, int D) {
  Gmm g{M, C, D, std::vector<float>((size_t)M * C), std::vector<float>((size_t)M * C * D), std::vector<float>((size_t)M * C * D)};
  std::vector<double> mu((size_t)C * D), var((size_t)C * D);
  for (size_t i = 0; i < mu.size(); ++i) { var[i] = exp(0.3 * normal()) * (i % 3 ? 1.0 : 9.0); mu[i] = normal() * sqrt(var[i]); }
  for (int m = 0; m < M; ++m)
    for (int c = 0; c < C; ++c) {
      double gcv = log(1.0 / C) - 0.5 * D * log(2.0 * M_PI);
      for (int k = 0; k < D; ++k) {
        const size_t i = (size_t)c * D + k;
        const double mean = mu[i] + (m ? 0.05 * normal() * sqrt(var[i]) * (c % 4 == 0) : 0.0);
        g.iv[((size_t)m * C + c) * D + k] = (float)(1.0 / var[i]);
        g.miv[((size_t)m * C + c) * D + k] = (float)(mean / var[i]);
        gcv += -0.5 * log(var[i]) - 0.5 * mean * mean / var[i];
      }
      g.gc[(size_t)m * C + c] = (float)gcv;
    }
  return g;
}

static int check_gmm(const char *name, const Gmm &g, const FbGmmPrepOptions &opt) {
  FbGmmPrepared p;
  std::string err;
  const int rc = fb_prepare_gmm(g.params(), opt, &p, &err);
  if (rc != FB_OK) { printf("%s: refused (%d) %s\n", name, rc, err.c_str()); return 1; }
  double s = walk(p.fx) + walk(p.bx) + walk(p.anchor) + walk(p.item_model) + walk(p.perm);
  for (const std::vector<uint16_t> &fd : p.fd) s += walk(fd);
  printf("%s: mode %d delta_p %d tiles %d/%d/%d of %d passes %d rms %.3g checksum %.0f\n", name, p.mode, p.delta_p, p.delta_t3,
         p.delta_t6, p.delta_t2, p.n_tiles, p.n_pass, p.delta_rms, s);
  return 0;
}

static int check_ivector(int C, int D, int R, int L, int S, int lda_cols) {
  const int triD = D * (D + 1) / 2;
  std::vector<float> w(C, 1.0f / C), mic((size_t)C * D), P((size_t)C * triD), mean_vec(R), lda((size_t)L * lda_cols), enrolled((size_t)S * R);
  std::vector<double> plda_mean(L, 0.01), plda_tr((size_t)L * L, 0.0), psi(L), zm(S, 0.0), zs(S, 1.0);
  for (int c = 0; c < C; ++c) {  // P = diag + a a' / D: symmetric positive definite
    std::vector<double> a(D);
    for (int d = 0; d < D; ++d) a[d] = 0.3 * normal();
    for (int r = 0, idx = 0; r < D; ++r)
      for (int q = 0; q <= r; ++q, ++idx) P[(size_t)c * triD + idx] = (float)((r == q ? 1.0 + 0.5 * uniform() : 0.0) + a[r] * a[q] / D);
    for (int d = 0; d < D; ++d) mic[(size_t)c * D + d] = (float)normal();
  }
  for (float &v : mean_vec) v = (float)(0.1 * normal());
  for (float &v : lda) v = (float)(normal() / sqrt((double)R));
  for (float &v : enrolled) v = (float)normal();
  for (int l = 0; l < L; ++l) { plda_tr[(size_t)l * L + l] = 1.0; psi[l] = 8.0 * pow(0.97, l); }
  fb_ivector_system sy;
  memset(&sy, 0, sizeof(sy));
  sy.C = C; sy.D = D; sy.R = R; sy.L = L; sy.S = S; sy.lda_cols = lda_cols; sy.num_gselect = 2; sy.min_post = 0.025; sy.prior_offset = 10.0;
  sy.fg_weights = w.data(); sy.fg_means_invcovars = mic.data(); sy.fg_inv_covars = P.data();
  sy.mean_vec = mean_vec.data(); sy.lda = lda.data(); sy.plda_mean = plda_mean.data(); sy.plda_transform = plda_tr.data();
  sy.plda_psi = psi.data(); sy.enrolled = enrolled.data(); sy.z_mean = zm.data(); sy.z_std = zs.data();
  FbIvPrepared p;
  std::string err;
  const int rc = fb_prepare_ivector(&sy, &p, &err);
  if (rc != FB_OK) { printf("ivector D=%d: refused (%d) %s\n", D, rc, err.c_str()); return 1; }
  const double s = walk(p.dg_gc) + walk(p.dg_miv) + walk(p.dg_iv) + walk(p.fg_gc) + walk(p.tri) + walk(p.fg64) + walk(p.fgL) + walk(p.backend);
  printf("ivector C=%d D=%d R=%d L=%d S=%d lda_cols=%d: fgL %zu doubles, backend %zu doubles (train at %zu), checksum %.0f\n", C, D, R, L,
         S, lda_cols, p.fgL.size(), p.backend.size(), p.o_tr, s);
  Gmm ubm{1, C, D, p.dg_gc, p.dg_miv, p.dg_iv};  // ... and its diagonal UBM through the GMM path, as fb_load_ivector does
  int bad = check_gmm("  its diagonal UBM", ubm, FbGmmPrepOptions());
  std::vector<float> notpd(P);
  notpd[0] = -1.0f;
  sy.fg_inv_covars = notpd.data();
  if (fb_prepare_ivector(&sy, &p, &err) != FB_E_ARG) { printf("a matrix that is not positive definite was accepted\n"); bad = 1; }
  else printf("  refusal: %s\n", err.c_str());
  return bad;
}

static int check_frontend() {
  fb_frontend_cfg c;
  memset(&c, 0, sizeof(c));
  c.sample_freq = 16000.0; c.frame_length = 400; c.frame_shift = 160; c.padded_length = 512; c.num_mel_bins = 30; c.num_ceps = 24;
  c.low_freq = 20.0; c.high_freq = 7600.0; c.preemph = 0.97; c.cepstral_lifter = 22.0; c.delta_window = 3; c.delta_order = 2;
  c.cmn_window = 300;
  FbFrontendTables t;
  std::string err;
  int rc = fb_frontend_tables(&c, &t, &err);
  if (rc != FB_OK) { printf("front end: refused (%d) %s\n", rc, err.c_str()); return 1; }
  const FbFrontendBlob b = fb_frontend_pack(t);
  printf("front end: %zu mel weights, blob %zu bytes (dscale at %zu), checksum %.0f\n", t.mel_w.size(), b.bytes.size(), b.o_ds, walk(b.bytes));
  c.num_mel_bins = 128; c.padded_length = 64; c.frame_length = 50;  // more bins than the FFT has: refused by the tables
  rc = fb_frontend_tables(&c, &t, &err);
  if (rc != FB_E_ARG) { printf("128 mel bins over 32 FFT bins were accepted\n"); return 1; }
  printf("  refusal: %s\n", err.c_str());
  return 0;
}

int main() {
  int bad = 0;
  FbGmmPrepOptions opt;
  const Gmm g3 = make_gmm(3, 64, 72);
  bad += check_gmm("gmm M=3 (rule)", g3, opt);
  for (int p : {1, 2, 3, 6}) {
    char name[32];
    snprintf(name, sizeof(name), "gmm M=3 P=%d", p);
    opt = FbGmmPrepOptions();
    opt.forced_p = p;
    bad += check_gmm(name, g3, opt);
  }
  opt = FbGmmPrepOptions();
  opt.use_f6 = false;
  opt.budget = 5e-5;
  bad += check_gmm("gmm M=3 no F6, budget 5e-5", g3, opt);
  opt = FbGmmPrepOptions();
  opt.forced_mode = FB_GMM_MODE_BX3;
  bad += check_gmm("gmm M=3 bx3", g3, opt);
  opt = FbGmmPrepOptions();
  bad += check_gmm("gmm M=11 (two passes)", make_gmm(11, 64, 72), opt);
  bad += check_gmm("gmm M=28 (three passes)", make_gmm(28, 32, 72), opt);
  bad += check_gmm("gmm M=29 (general kernel)", make_gmm(29, 32, 72), opt);
  bad += check_gmm("gmm C=48 (padded tile)", make_gmm(3, 48, 72), opt);
  bad += check_gmm("gmm D=60", make_gmm(3, 64, 60), opt);
  bad += check_gmm("gmm D=80", make_gmm(2, 32, 80), opt);
  Gmm far = make_gmm(2, 32, 72);
  far.miv[5] = 40000.0f;  // out of f16's range: bx3
  bad += check_gmm("gmm out of f16 range", far, opt);
  Gmm two = make_gmm(3, 32, 72);
  for (size_t i = 0; i < (size_t)32 * 72; ++i) two.iv[(size_t)2 * 32 * 72 + i] *= 1.5f;
  bad += check_gmm("gmm two variance groups", two, opt);
  bad += check_ivector(4, 72, 8, 4, 2, 8);
  bad += check_ivector(4, 72, 8, 4, 2, 9);
  bad += check_ivector(3, 60, 8, 4, 1, 8);
  bad += check_frontend();
  printf(bad ? "prepare_check: FAILED\n" : "prepare_check: ok\n");
  return bad ? 1 : 0;
}
