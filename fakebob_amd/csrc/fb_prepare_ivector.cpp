// fb_prepare_ivector.cpp -- the host tables of an i-vector / PLDA system (fb_prepare.h): the diagonalised UBM, the
// images of the full-covariance UBM and the back-end table.  Sigma^-1 M and U are derived on the device
// (fb_launch_iv_derive) and are not prepared here.
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "fb_prepare.h"

bool fb_host_chol(std::vector<double> &A, int n) {
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (!(d > 0.0)) return false;
    d = sqrt(d);
    A[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double v = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) v -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = v / d;
    }
  }
  return true;
}
void fb_host_chol_solve(const std::vector<double> &Lm, int n, double *b) {
  for (int i = 0; i < n; ++i) {
    double v = b[i];
    for (int k = 0; k < i; ++k) v -= Lm[(size_t)i * n + k] * b[k];
    b[i] = v / Lm[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = b[i];
    for (int k = i + 1; k < n; ++k) v -= Lm[(size_t)k * n + i] * b[k];
    b[i] = v / Lm[(size_t)i * n + i];
  }
}

// ivector-subtract-global-mean | transform-vec | ivector-normalize-length, then Plda::TransformIvector
// (normalize_length, n = 1)  ([EXT] SURVEY.md A.10)
void fb_host_backend(const fb_ivector_system *sy, const float *ivec, double *y) {
  const int R = sy->R, L = sy->L;
  std::vector<double> x(R), z(L);
  for (int r = 0; r < R; ++r) x[r] = (double)ivec[r] - (double)sy->mean_vec[r];
  double nrm = 0.0;
  for (int l = 0; l < L; ++l) {
    const float *row = sy->lda + (size_t)l * sy->lda_cols;
    double acc = sy->lda_cols == R + 1 ? (double)row[R] : 0.0;
    for (int r = 0; r < R; ++r) acc += (double)row[r] * x[r];
    z[l] = acc;
    nrm += acc * acc;
  }
  const double ratio = sqrt(nrm) / sqrt((double)L);
  if (ratio != 0.0) for (int l = 0; l < L; ++l) z[l] /= ratio;
  double dot = 0.0;
  for (int l = 0; l < L; ++l) {
    const double *row = sy->plda_transform + (size_t)l * L;
    double acc = 0.0;
    for (int m = 0; m < L; ++m) acc += row[m] * (z[m] - sy->plda_mean[m]);
    y[l] = acc;
    dot += acc * acc / (sy->plda_psi[l] + 1.0);
  }
  const double nf = sqrt((double)L / dot);
  for (int l = 0; l < L; ++l) y[l] *= nf;
}

// fgmm-global-to-gmm (DiagGmm::CopyFromFullGmm) + FullGmm::ComputeGconsts, float64 on host
int fb_iv_full_to_diag(const fb_ivector_system *sy, FbIvPrepared *out, std::string *err) {
  const int C = sy->C, D = sy->D, triD = D * (D + 1) / 2;
  std::vector<float> &dg_gc = out->dg_gc, &dg_miv = out->dg_miv, &dg_iv = out->dg_iv, &fg_gc = out->fg_gc;
  dg_gc.assign(C, 0.0f);
  dg_miv.assign((size_t)C * D, 0.0f);
  dg_iv.assign((size_t)C * D, 0.0f);
  fg_gc.assign(C, 0.0f);
  std::vector<double> P((size_t)D * D), col(D), mean(D);
  const double LOG2PI = 1.8378770664093454835606594728112;
  for (int k = 0; k < C; ++k) {
    const float *pk = sy->fg_inv_covars + (size_t)k * triD;
    for (int r = 0; r < D; ++r)
      for (int c = 0; c <= r; ++c) { P[(size_t)r * D + c] = (double)pk[(size_t)r * (r + 1) / 2 + c]; P[(size_t)c * D + r] = P[(size_t)r * D + c]; }
    std::vector<double> Lc(P);
    if (!fb_host_chol(Lc, D)) {
      char msg[96];
      snprintf(msg, sizeof(msg), "full-covariance Gaussian %d is not positive definite", k);
      *err = msg;
      return FB_E_ARG;
    }
    double logdet_inv = 0.0;
    for (int d = 0; d < D; ++d) logdet_inv += 2.0 * log(Lc[(size_t)d * D + d]);
    // mean = covar * means_invcovars ; covar diag via solves with unit vectors
    for (int d = 0; d < D; ++d) mean[d] = (double)sy->fg_means_invcovars[(size_t)k * D + d];
    double quad = 0.0;
    {
      std::vector<double> t(mean);
      fb_host_chol_solve(Lc, D, t.data());
      for (int d = 0; d < D; ++d) quad += (double)sy->fg_means_invcovars[(size_t)k * D + d] * t[d];
      mean = t;
    }
    const double w = (double)sy->fg_weights[k];
    fg_gc[k] = (float)(log(w) - 0.5 * (D * LOG2PI - logdet_inv + quad));
    double gc = log(w) - 0.5 * D * LOG2PI;
    for (int d = 0; d < D; ++d) {
      for (int q = 0; q < D; ++q) col[q] = q == d ? 1.0 : 0.0;
      fb_host_chol_solve(Lc, D, col.data());
      const float ivf = (float)(1.0 / col[d]);
      const float mivf = (float)(mean[d] * (1.0 / col[d]));
      dg_iv[(size_t)k * D + d] = ivf;
      dg_miv[(size_t)k * D + d] = mivf;
      gc += 0.5 * log((double)ivf) - 0.5 * (double)mivf * (double)mivf / (double)ivf;
    }
    dg_gc[k] = (float)gc;
  }
  return FB_OK;
}

std::vector<unsigned char> fb_iv_tri_table(int D) {
  const int triD = D * (D + 1) / 2;
  std::vector<unsigned char> tr(2 * (size_t)triD);
  for (int r = 0, idx = 0; r < D; ++r)
    for (int c = 0; c <= r; ++c, ++idx) { tr[idx] = (unsigned char)r; tr[triD + idx] = (unsigned char)c; }
  return tr;
}

// float64 image of the full UBM for the register-blocked full-covariance kernel: per component the packed triangle
// (diagonal halved), means_invcovars, gconst
std::vector<double> fb_iv_fg64_image(const fb_ivector_system *sy, const std::vector<float> &fg_gc) {
  const int C = sy->C, D = sy->D, triD = D * (D + 1) / 2;
  const size_t stride = (size_t)triD + D + 1;
  std::vector<double> f64((size_t)C * stride);
  for (int c = 0; c < C; ++c) {
    double *o = &f64[(size_t)c * stride];
    const float *P = sy->fg_inv_covars + (size_t)c * triD;
    for (int r = 0, idx = 0; r < D; ++r)
      for (int cc = 0; cc <= r; ++cc, ++idx) o[idx] = (cc == r) ? 0.5 * (double)P[idx] : (double)P[idx];
    for (int d = 0; d < D; ++d) o[triD + d] = (double)sy->fg_means_invcovars[(size_t)c * D + d];
    o[triD + D] = (double)fg_gc[c];
  }
  return f64;
}

// Cholesky image of the same function for k_iv_fullcov_mfma (ivector_kernels.hip, D = 72): with P = L L' and any mu,
//   gconst + mic . x - 1/2 x'Px = [gconst + 1/2 mu'P mu] + (mic - P mu) . x - 1/2 |L'(x - mu)|^2;
// mu = P^-1 mic refined in long double until the residual's term is far below the float64 rounding of the
// rest (it is then dropped); L from a long double factorisation of the float32 parameters as they are, rounded
// once.  A component whose residual cannot be brought down keeps the whole batch on the triangle-form kernel: false.
bool fb_iv_chol_image(const fb_ivector_system *sy, const std::vector<float> &fg_gc, std::vector<double> *out) {
  const int C = sy->C, D = sy->D, triD = D * (D + 1) / 2;
  if (D != 72) return false;
  const int NFR = 50, REC = NFR * 64 + 72 + 2;
  std::vector<double> rec((size_t)C * REC, 0.0);
  std::vector<long double> Pm((size_t)D * D), Lm((size_t)D * D), mu(D), rs(D), dx(D);
  auto solve = [&](std::vector<long double> &b) {  // b <- P^-1 b through L
    for (int i = 0; i < D; ++i) {
      long double v = b[i];
      for (int q = 0; q < i; ++q) v -= Lm[(size_t)i * D + q] * b[q];
      b[i] = v / Lm[(size_t)i * D + i];
    }
    for (int i = D - 1; i >= 0; --i) {
      long double v = b[i];
      for (int q = i + 1; q < D; ++q) v -= Lm[(size_t)q * D + i] * b[q];
      b[i] = v / Lm[(size_t)i * D + i];
    }
  };
  for (int c = 0; c < C; ++c) {
    const float *P = sy->fg_inv_covars + (size_t)c * triD;
    const float *mic = sy->fg_means_invcovars + (size_t)c * D;
    for (int r = 0, idx = 0; r < D; ++r)
      for (int cc = 0; cc <= r; ++cc, ++idx) Pm[(size_t)r * D + cc] = Pm[(size_t)cc * D + r] = (long double)P[idx];
    std::fill(Lm.begin(), Lm.end(), 0.0L);
    for (int j = 0; j < D; ++j) {
      long double d = Pm[(size_t)j * D + j];
      for (int q = 0; q < j; ++q) d -= Lm[(size_t)j * D + q] * Lm[(size_t)j * D + q];
      if (!(d > 0.0L)) return false;
      const long double lj = sqrtl(d);
      Lm[(size_t)j * D + j] = lj;
      for (int i = j + 1; i < D; ++i) {
        long double v = Pm[(size_t)i * D + j];
        for (int q = 0; q < j; ++q) v -= Lm[(size_t)i * D + q] * Lm[(size_t)j * D + q];
        Lm[(size_t)i * D + j] = v / lj;
      }
    }
    for (int d = 0; d < D; ++d) mu[d] = (long double)mic[d];
    solve(mu);
    double *o = &rec[(size_t)c * REC];
    long double res_term = 0.0L;
    for (int it = 0; it < 4; ++it) {
      // the kernel uses mu rounded to float64: refine THAT vector's residual
      long double mx = 0.0L, sc = 0.0L;
      for (int i = 0; i < D; ++i) {
        long double v = (long double)mic[i];
        for (int q = 0; q < D; ++q) v -= Pm[(size_t)i * D + q] * (long double)(double)mu[q];
        rs[i] = v;
        mx = std::max(mx, fabsl(v));
        sc = std::max(sc, fabsl((long double)mic[i]));
      }
      res_term = mx / (sc > 0.0L ? sc : 1.0L);
      if (it == 3) break;
      dx = rs;
      solve(dx);
      for (int i = 0; i < D; ++i) mu[i] = (long double)(double)mu[i] + dx[i];
    }
    // (mic - P mu) . x relative to mic . x: float64 rounding of mu leaves ~1e-16 kappa; the term is dropped, so it has
    // to be invisible next to the 1e-13 the float64 sums themselves carry
    if (!(res_term < 1.0e-11L)) return false;
    long double q2 = 0.0L;
    for (int i = 0; i < D; ++i)
      for (int q = 0; q < D; ++q) q2 += (long double)(double)mu[i] * Pm[(size_t)i * D + q] * (long double)(double)mu[q];
    int f = 0;
    for (int jt = 0; jt < 5; ++jt)
      for (int s2 = 4 * jt; s2 < D / 4; ++s2, ++f)
        for (int l = 0; l < 64; ++l) {
          const int q = l >> 4;  // the kernel's K order: a lane's four places of a 16-row block are consecutive rows
          const int row = s2 < 16 ? 16 * (s2 / 4) + 4 * q + (s2 % 4) : 64 + 2 * q + (s2 - 16), col = 16 * jt + (l & 15);
          o[(size_t)f * 64 + l] = (col <= row && col < D) ? (double)Lm[(size_t)row * D + col] : 0.0;
        }
    for (int d = 0; d < D; ++d) o[(size_t)NFR * 64 + d] = (double)mu[d];
    o[(size_t)NFR * 64 + D] = (double)((long double)fg_gc[c] + 0.5L * q2);
  }
  *out = std::move(rec);
  return true;
}

// back-end tables, float64: mean_vec [R], the LDA and PLDA transforms transposed, the enrolled speakers in PLDA space
void fb_iv_backend_table(const fb_ivector_system *sy, FbIvPrepared *out) {
  const int R = sy->R, L = sy->L, S = sy->S, lc = sy->lda_cols;
  std::vector<double> &host = out->backend;
  host.clear();
  out->o_mean = 0; host.resize(R);
  for (int r = 0; r < R; ++r) host[out->o_mean + r] = (double)sy->mean_vec[r];
  const size_t o_lda = out->o_lda = host.size(); host.resize(o_lda + (size_t)lc * L);
  for (int l = 0; l < L; ++l) for (int c = 0; c < lc; ++c) host[o_lda + (size_t)c * L + l] = (double)sy->lda[(size_t)l * lc + c];
  const size_t o_pm = out->o_pm = host.size(); host.resize(o_pm + L);
  for (int l = 0; l < L; ++l) host[o_pm + l] = sy->plda_mean[l];
  const size_t o_pt = out->o_pt = host.size(); host.resize(o_pt + (size_t)L * L);
  for (int l = 0; l < L; ++l) for (int m = 0; m < L; ++m) host[o_pt + (size_t)m * L + l] = sy->plda_transform[(size_t)l * L + m];
  const size_t o_psi = out->o_psi = host.size(); host.resize(o_psi + L);
  for (int l = 0; l < L; ++l) host[o_psi + l] = sy->plda_psi[l];
  const size_t o_tr = out->o_tr = host.size(); host.resize(o_tr + (size_t)S * L);
  for (int sp = 0; sp < S; ++sp) fb_host_backend(sy, sy->enrolled + (size_t)sp * R, &host[o_tr + (size_t)sp * L]);
}

int fb_prepare_ivector(const fb_ivector_system *sy, FbIvPrepared *out, std::string *err) {
  FbIvPrepared p;
  p.triD = sy->D * (sy->D + 1) / 2;
  p.triR = sy->R * (sy->R + 1) / 2;
  const int rc = fb_iv_full_to_diag(sy, &p, err);
  if (rc != FB_OK) return rc;
  p.tri = fb_iv_tri_table(sy->D);
  p.fg64 = fb_iv_fg64_image(sy, p.fg_gc);
  if (!fb_iv_chol_image(sy, p.fg_gc, &p.fgL)) p.fgL.clear();
  fb_iv_backend_table(sy, &p);
  *out = std::move(p);
  return FB_OK;
}
