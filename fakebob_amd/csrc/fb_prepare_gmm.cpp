// fb_prepare_gmm.cpp -- the diagonal-GMM images of k_gmm_bx3, k_gmm_fx2 and k_gmm_fx2w, from Kaldi's parameters
// (fb_prepare.h).  Host code only; the results depend on -ffp-contract=off -fno-fast-math like the rest of the library.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "fb_prepare.h"

static const double L2E = 1.4426950408889634;
static inline double f16r(double v) { return (double)(_Float16)v; }  // round to nearest even
static inline void put16(double v, uint16_t *out) {
  const _Float16 a = (_Float16)v;
  memcpy(out, &a, 2);
}

FbGmmGroups fb_gmm_group_by_variance(const FbGmmParams &g) {
  const int M = g.M, C = g.C, D = g.D;
  FbGmmGroups r;
  r.group_of.assign(M, -1);
  for (int m = 0; m < M; ++m) {
    for (size_t q = 0; q < r.group_rep.size(); ++q)
      if (memcmp(g.iv + (size_t)m * C * D, g.iv + (size_t)r.group_rep[q] * C * D, sizeof(float) * (size_t)C * D) == 0) {
        r.group_of[m] = (int)q;
        break;
      }
    if (r.group_of[m] < 0) { r.group_of[m] = (int)r.group_rep.size(); r.group_rep.push_back(m); }
  }
  for (int q = 0; q < (int)r.group_rep.size(); ++q) {
    r.item_model.push_back(-1 - q);  // Q item of group q (any negative = Q)
    for (int m = 0; m < M; ++m) if (r.group_of[m] == q) r.item_model.push_back(m);
  }
  return r;
}

// f16x2 images (k_gmm_fx2): two-term f16 split, gconst at K position D.  Needs every parameter inside f16's range; a model
// that does not fit runs on the bf16x3 kernel.
FbGmmFxScaling fb_gmm_fx2_scaling(const FbGmmParams &g, int NKF, bool want_delta) {
  const int M = g.M, C = g.C, D = g.D;
  const float *gconsts = g.gconsts, *miv = g.miv, *iv = g.iv;
  FbGmmFxScaling sc = {false, 0, 0, 0, 0, 0};
  const float lim = 32768.0f;
  float max_q = 0.0f, max_l = 0.0f, max_g = 0.0f;
  bool finite = true;
  for (size_t i = 0; i < (size_t)M * C * D; ++i) {
    max_q = std::max(max_q, 0.5f * fabsf(iv[i]));
    max_l = std::max(max_l, fabsf(miv[i]));
    finite = finite && std::isfinite(iv[i]) && std::isfinite(miv[i]);
  }
  for (size_t i = 0; i < (size_t)M * C; ++i) {
    max_g = std::max(max_g, fabsf(gconsts[i]));
    finite = finite && std::isfinite(gconsts[i]);
  }
  if (want_delta && finite) {  // the deltas share the scaling of the full parameters
    for (int m = 1; m < M; ++m) {
      for (size_t i = 0; i < (size_t)C * D; ++i) max_l = std::max(max_l, fabsf(miv[(size_t)m * C * D + i] - miv[i]));
      for (int c = 0; c < C; ++c) max_g = std::max(max_g, fabsf(gconsts[(size_t)m * C + c] - gconsts[c]));
    }
  }
  if (!finite || max_l >= lim || max_g >= lim || max_q >= lim || NKF > 6) return sc;
  // one accumulator, unscaled residuals: operands are moved up by exact powers of two so that the residuals
  // of typical values are normal f16 numbers (subnormal ones keep an absolute precision of 2^-25):
  //   linear:    (mu/sigma^2, gconst) * 2^kl  x  (x, 1) * 2^kx         kl <= 4, kx = 4
  //   quadratic: -1/(2 sigma^2)      * 2^kq  x  x^2 * 2^kx2           kq + kx2 = kl + kx = kacc
  auto headroom = [&](float mx) { int k = 0; while (k < 15 && mx * (float)(2 << k) < lim) ++k; return k; };
  sc.kl = std::min(4, headroom(std::max(max_l, max_g)));
  sc.kx = 4;
  sc.kacc = sc.kl + sc.kx;
  sc.kq = std::min(headroom(max_q), sc.kacc + 2);  // x^2 * 2^-2 at most: keeps |x| < 511 and small squares precise
  if (sc.kq < sc.kacc - 4) return sc;              // would need x^2 * 2^5 or more: |x| < 45 is too tight
  sc.kx2 = sc.kacc - sc.kq;
  sc.ok = true;
  return sc;
}

std::vector<uint16_t> fb_gmm_pack_fx2(const FbGmmParams &g, const FbGmmGroups &gr, int NKF, const FbGmmFxScaling &sc) {
  const int C = g.C, D = g.D, n_tiles = (C + 31) / 32, n_items = (int)gr.item_model.size();
  const size_t per_item = (size_t)2 * NKF * 64 * 8;  // f16 values
  std::vector<uint16_t> fx((size_t)n_tiles * n_items * per_item, 0);
  auto split2 = [](float v, uint16_t out[2]) {
    const _Float16 a = (_Float16)v;  // round to nearest even
    const float r = v - (float)a;    // exact; may be a subnormal f16 (kept by the matrix pipe)
    const _Float16 b = (_Float16)r;
    memcpy(&out[0], &a, 2);
    memcpy(&out[1], &b, 2);
  };
  const float qscale = -0.5f * ldexpf(1.0f, sc.kq), lscale = ldexpf(1.0f, sc.kl);
  for (int t = 0; t < n_tiles; ++t)
    for (int it = 0; it < n_items; ++it) {
      uint16_t *im = &fx[((size_t)t * n_items + it) * per_item];
      const int im_model = gr.item_model[it];
      for (int cc = 0; cc < 32; ++cc) {
        const int c = t * 32 + cc;
        for (int k = 0; k < 16 * NKF; ++k) {
          uint16_t sp[2] = {0, 0};
          if (k < D) {
            if (c < C)
              split2(im_model < 0 ? qscale * g.iv[((size_t)gr.group_rep[-1 - im_model] * C + c) * D + k]
                                  : lscale * g.miv[((size_t)im_model * C + c) * D + k], sp);
          } else if (k == D && im_model >= 0) {  // gconst against 2^kx in the frame operand
            split2(c < C ? lscale * g.gconsts[(size_t)im_model * C + c] : -60000.0f, sp);  // padding components: exp() == 0
          }
          for (int s2 = 0; s2 < 2; ++s2) im[fb_gmm_frag_index(s2, NKF, k, cc)] = sp[s2];
        }
      }
    }
  return fx;
}

// bf16x3 images (k_gmm_bx3): exact 3-way bf16 split of every parameter, gconst in the K padding
std::vector<uint16_t> fb_gmm_pack_bx3(const FbGmmParams &g, const FbGmmGroups &gr, int NK) {
  const int C = g.C, D = g.D, n_tiles = (C + 31) / 32, n_items = (int)gr.item_model.size();
  const size_t per_item = (size_t)3 * NK * 64 * 8;  // bf16 values
  std::vector<uint16_t> bx((size_t)n_tiles * n_items * per_item, 0);
  auto split3 = [](float v, uint16_t out[3]) {
    for (int s = 0; s < 3; ++s) {
      uint32_t u;
      memcpy(&u, &v, 4);
      u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;  // round to nearest even, 8 significant bits
      float t;
      memcpy(&t, &u, 4);
      out[s] = (uint16_t)(u >> 16);
      v -= t;  // exact
    }
  };
  for (int t = 0; t < n_tiles; ++t)
    for (int it = 0; it < n_items; ++it) {
      uint16_t *im = &bx[((size_t)t * n_items + it) * per_item];
      const int im_model = gr.item_model[it];
      for (int cc = 0; cc < 32; ++cc) {
        const int c = t * 32 + cc;
        for (int k = 0; k < 16 * NK; ++k) {
          float v = 0.0f;
          if (k < D) {
            if (c < C)
              v = im_model < 0 ? -0.5f * g.iv[((size_t)gr.group_rep[-1 - im_model] * C + c) * D + k]
                               : g.miv[((size_t)im_model * C + c) * D + k];
          }
          uint16_t sp[3] = {0, 0, 0};
          if (k < D) {
            split3(v, sp);
          } else if (k < D + 3 && im_model >= 0) {  // gconst term k-D against 1.0 in the frame operand
            uint16_t gs[3];
            split3(c < C ? g.gconsts[(size_t)im_model * C + c] : -1.0e30f, gs);
            sp[0] = gs[k - D];
          }
          for (int s = 0; s < 3; ++s) im[fb_gmm_frag_index(s, NK, k, cc)] = sp[s];
        }
      }
    }
  return bx;
}

// ------------------------------------------------------------------------------------------------ the delta rule
// Delta images of k_gmm_fx2w: items {Q, model 0, delta_1 .. delta_{M-1}} per tile.  Mean-only MAP adaptation
// (build_spk_models.py:170, gmm-global-est-map.cc:81) leaves weights and variances alone, so
//   ll_m,k(x) = ll_0,k(x) + (gconst_m,k - gconst_0,k) + (means_invvars_m,k - means_invvars_0,k) . x
// and the second line is small: the kernel continues the base model's finished accumulator with the delta
// item.  The deltas are float32 differences (exact by Sterbenz's lemma for the close values adaptation
// produces, correctly rounded otherwise).
//
// Products per K chunk of the delta items, PER COMPONENT TILE.  P = 2 drops the frames' second f16 term -- an
// error of 2^-12 |delta . x| per (frame, component), random in sign from frame to frame --, P = 1 also the
// deltas' second term.  b_mk = 2^-12 |delta_mk * (|mu_k| + 3 sigma_k)|_2 bounds the former where component k
// matters (x within 3 sigma of its mean).  A frame's error is that of the components that explain it, so the error
// of an utterance average is ~c sqrt(sum_k p_k b_mk^2), p_k the share of frames component k explains -- its weight
// w_k under the model's own distribution --, with c ~ 0.07 for P = 2 and ~0.14 for P = 1 measured in a float64
// numpy model of the split (with equal weights that is the 0.07 / 0.14 rms_k(b) of round 3).
// Means-only MAP adaptation moves a component by alpha_k = n_k / (n_k + tau) of the way to the enrolment data's
// mean (gmm-global-est-map.cc:31,81): the components the enrolment data occupied move far, the others hardly.  So
// the components are SORTED by their contribution w_k max_m b_mk^2 (the order is free under logsumexp; the same
// permutation for the quadratic item, the base model and every delta image), and the leading tiles get three
// products, the next ones two, the tail one: the smallest sets for which the predicted error of the worst model,
//     e^2 = 0.07^2 sum_{k in P = 2 tiles} w_k b_mk^2 + 0.14^2 sum_{k in P = 1 tiles} w_k b_mk^2,
// stays below (6e-6)^2 -- under half a float32 ulp of the ~-150 results and inside the ~3.3e-6 float32
// accumulation error every variant carries (tests/test_gpu_parity.py).  Models adapted far everywhere (enrolment
// on many frames, a small tau, unrelated means) get three products in every tile -- the arithmetic of the non-delta
// kernels.

// the weights w_k [C] of the base model, the bounds b2 [M - 1][C] and the sort key [C]
static void delta_weights_and_bounds(const FbGmmParams &g, std::vector<double> &wk, std::vector<double> &b2,
                                     std::vector<double> &key) {
  const int M = g.M, C = g.C, D = g.D;
  const float *gconsts = g.gconsts, *miv = g.miv, *iv = g.iv;
  b2.assign((size_t)(M - 1) * C, 0.0);
  wk.assign(C, 0.0);
  key.assign(C, 0.0);
  const double LOG2PI = 1.8378770664093454835606594728112;
  double wsum = 0.0;
  for (int c = 0; c < C; ++c) {  // w_k from the base model's gconst (DiagGmm::ComputeGconsts)
    double lw = (double)gconsts[c] + 0.5 * D * LOG2PI;
    for (int k = 0; k < D; ++k) {
      const double ivk = (double)iv[(size_t)c * D + k], mk = (double)miv[(size_t)c * D + k];
      lw += 0.5 * (mk * mk / ivk - log(ivk));
    }
    wk[c] = std::isfinite(lw) ? exp(std::min(lw, 0.0)) : 0.0;
    wsum += wk[c];
  }
  for (int c = 0; c < C; ++c) wk[c] = wsum > 0.0 ? wk[c] / wsum : 1.0 / C;
  for (int m = 1; m < M; ++m)
    for (int c = 0; c < C; ++c) {
      double sq = 0.0;
      for (int k = 0; k < D; ++k) {
        const double ivk = (double)iv[(size_t)c * D + k];
        const double reach = (fabs((double)miv[(size_t)c * D + k]) + 3.0 * sqrt(ivk)) / ivk;  // |mu| + 3 sigma
        const double dl = (double)miv[((size_t)m * C + c) * D + k] - (double)miv[(size_t)c * D + k];
        sq += dl * dl * reach * reach;
      }
      b2[(size_t)(m - 1) * C + c] = ldexp(sq, -24);
      // (the floor keeps a component no frame is expected in from hiding an arbitrarily large shift in the tail)
      key[c] = std::max(key[c], std::max(wk[c], 0.01 / C) * b2[(size_t)(m - 1) * C + c]);
    }
}

// t3 / t6 / t2 of the plan under opt's budget, then its forced class
static void delta_tile_classes(const FbGmmParams &g, const std::vector<double> &wk, const std::vector<double> &b2,
                               const FbGmmPrepOptions &opt, FbGmmDeltaPlan *plan) {
  const int M = g.M, C = g.C, n_tiles = C / 32;
  // tsum[m][t]: model m's sum over the components of tile t
  std::vector<std::vector<double>> tsum(M - 1, std::vector<double>(n_tiles, 0.0));
  for (int m = 0; m < M - 1; ++m)
    for (int t = 0; t < n_tiles; ++t)
      for (int cc = 0; cc < 32; ++cc) {
        const int c = plan->perm[t * 32 + cc];
        tsum[m][t] += std::max(wk[c], 0.01 / C) * b2[(size_t)m * C + c];
      }
  auto worst_sum = [&](int t_lo, int t_hi) {  // worst model's sum over the tiles [t_lo, t_hi)
    double w = 0.0;
    for (int m = 0; m < M - 1; ++m) {
      double a = 0.0;
      for (int t = t_lo; t < t_hi; ++t) a += tsum[m][t];
      w = std::max(w, a);
    }
    return w;
  };
  // opt.budget (FB_GMM_DELTA_BUDGET): the error budget of the rule (default 6e-6: float32-equivalent scores).  north_star asks
  // for 1e-4 against the reference; a caller who wants only that can say so (e.g. 5e-5) and gets two products where
  // the default insists on three -- measured and reported separately by bench.py, never the headline
  //
  // The F6 class (round 4): the two products P = 1 leaves out -- delta's second term against the frames' leading
  // term, delta's leading term against the frames' second -- taken in block-scaled fp6 / fp4 by four
  // v_mfma_scale_f32_32x32x64_f8f6f4 per 32-frame half (K = 64 each at the price of one K = 16 f16 product: ~20 ns,
  // tools/probes/f6_mfma_probe.hip) instead of ten f16 products; operands and their layout: fb_gmm_f6_pack_component.
  // What an utterance average keeps of their rounding, measured on the realistic enrolment with the class in every
  // tile: max |err| 7.1e-6 against 3.2e-4 for P = 1, 6.8e-5 for P = 2 and 3.3e-6 for P = 3 (the float32 accumulation
  // error every variant carries) -- c = 0.003 in the model above, cheaper AND closer than P = 2, which the rule
  // therefore no longer chooses (opt.use_f6 == false, FB_GMM_DELTA_F6=0, brings the earlier rule back: P = 2 in the
  // middle, no F6 tiles).
  // (ce6: 0.003 reproduced the MEAN of the measured cases; the worst one -- the class in every tile of the realistic
  //  enrolment, 8 utterances: 7.1e-6 in all, i.e. sqrt(7.1^2 - 3.3^2) = 6.3e-6 of its own beside the float32 floor --
  //  sat 20 % above the prediction: the parameters' rounding is the same for every frame and does not average out
  //  the way the sqrt(sum w b^2) model assumes.  Round 5 calibrates on that worst case: 0.0036.)
  const double budget2 = opt.budget * opt.budget, ce1 = 0.14 * 0.14, ce2 = 0.07 * 0.07, ce6 = 0.0036 * 0.0036;
  int t2 = n_tiles, t3 = n_tiles, t6 = n_tiles;
  while (t2 > 0 && ce1 * worst_sum(t2 - 1, n_tiles) <= 0.75 * budget2) --t2;  // (the P = 1 tail may use 3/4 of the budget)
  t3 = t6 = t2;
  const double left = budget2 - ce1 * worst_sum(t2, n_tiles);
  if (opt.use_f6) {
    while (t3 > 0 && ce6 * worst_sum(t3 - 1, t2) <= left) --t3;
    t6 = t2;
  } else {
    while (t3 > 0 && ce2 * worst_sum(t3 - 1, t2) <= left) --t3;
    t6 = t3;
  }
  if (opt.forced_p) {  // the same class in every tile (6 = F6)
    const int v = opt.forced_p;
    t3 = v == 3 ? n_tiles : 0;
    t6 = v == 6 ? n_tiles : t3;
    t2 = v >= 2 ? n_tiles : 0;
  }
  plan->t3 = t3; plan->t6 = t6; plan->t2 = t2;
  const int cnt[4] = {n_tiles - t2, t2 - t6, t3, t6 - t3}, cls[4] = {1, 2, 3, 6};
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (cnt[i] > cnt[best]) best = i;
  plan->want_p = cls[best];
}

// The images are in LOG2 units: every parameter is multiplied by log2 e in float64 and then split into its f16
// terms -- the accumulators of k_gmm_fx2w then hold the exponent of 2 directly and its logsumexp update needs
// no multiplication (gmm_wide_kernel.hip).  There is no common power-of-two factor to undo either; instead every
// DIMENSION d is balanced by an exact power of two of its own: the frames' x_d is multiplied by 2^kd[d], the
// linear parameters by 2^-kd[d] (x_d^2 by 2^kq[d], the quadratic ones by 2^-kq[d]), chosen from the spread
// sd[d] of the dimension under the base model so that |x_d| 2^kd ~ 1 and x_d^2 2^kq ~ 1: the parameters -- whose
// rounding is the same for every frame -- then sit around 1 .. 10 where both f16 terms are normal numbers (22
// significant bits), the frames keep theirs down to |x_d| = sd/8 and an absolute 2^-25 below.
static void delta_balance(const FbGmmParams &g, int NKF, FbGmmDeltaPlan *plan) {
  const int M = g.M, C = g.C, D = g.D;
  const float *gconsts = g.gconsts, *miv = g.miv, *iv = g.iv;
  std::vector<int> &kd = plan->kd, &kq = plan->kq;
  kd.assign(16 * NKF, 0);
  kq.assign(16 * NKF, 0);
  bool fits = true;
  for (int k = 0; k < D; ++k) {
    double m1 = 0.0, m2 = 0.0, vs = 0.0;  // spread of dimension k: mean component variance + variance of the means
    for (int c = 0; c < C; ++c) {
      const double var = 1.0 / (double)iv[(size_t)c * D + k], mu = (double)miv[(size_t)c * D + k] * var;
      m1 += mu; m2 += mu * mu; vs += var;
    }
    const double sd2 = vs / C + std::max(0.0, m2 / C - (m1 / C) * (m1 / C));
    const int e2 = sd2 > 0.0 && std::isfinite(sd2) ? (int)lrint(-0.5 * log2(sd2)) : 0;
    kd[k] = std::min(24, std::max(-24, e2));
    kq[k] = 2 * kd[k];
    double pl = 0.0, pq = 0.0;  // the largest scaled parameters must stay inside f16's range
    for (int m = 0; m < M; ++m)
      for (int c = 0; c < C; ++c) pl = std::max(pl, fabs((double)miv[((size_t)m * C + c) * D + k]));
    for (int c = 0; c < C; ++c) pq = std::max(pq, 0.5 * (double)iv[(size_t)c * D + k]);
    fits = fits && ldexp(L2E * pl, -kd[k]) < 60000.0 && ldexp(L2E * pq, -kq[k]) < 60000.0;
  }
  for (int c = 0; c < M * C; ++c) fits = fits && L2E * fabs((double)gconsts[c]) < 60000.0;
  plan->fits = fits;
}

FbGmmDeltaPlan fb_gmm_delta_plan(const FbGmmParams &g, int NKF, const FbGmmPrepOptions &opt) {
  const int M = g.M, C = g.C;
  FbGmmDeltaPlan plan;
  std::vector<double> wk, b2, key;
  delta_weights_and_bounds(g, wk, b2, key);
  plan.perm.resize(C);
  for (int c = 0; c < C; ++c) plan.perm[c] = c;
  std::stable_sort(plan.perm.begin(), plan.perm.end(), [&](int x, int y) { return key[x] > key[y]; });
  delta_tile_classes(g, wk, b2, opt, &plan);
  {  // (reported by fb_gmm_kernel_variant: the equal-weight statistic of round 3)
    double sumsq = 0.0;
    for (double v : b2) sumsq += v;
    plan.delta_rms = sqrt(sumsq / ((double)(M - 1) * C));
  }
  delta_balance(g, NKF, &plan);
  // More than FB_FXW_MAX_M models (the LDS holds a tile of 1 + M items and the state of M models) run as SEVERAL
  // PASSES of the kernel: pass p scores the base model again and its share of the others -- the M - 1 delta models dealt
  // evenly over ceil((M - 1) / (FB_FXW_MAX_M - 1)) launches
  plan.n_pass = (M - 1 + FB_FXW_MAX_M - 2) / (FB_FXW_MAX_M - 1);
  for (int p = 0; p <= FB_FXW_MAX_PASS; ++p) plan.pass_lo[p] = 1;
  for (int p = 0; p <= plan.n_pass; ++p) plan.pass_lo[p] = 1 + (int)(((long long)(M - 1) * p) / plan.n_pass);
  return plan;
}

// ------------------------------------------------------------------------------------------------ the F6 item
int fb_f6_scale_for(const double *val, int n, double top) {
  double mx = 0.0;
  for (int u = 0; u < n; ++u) mx = std::max(mx, fabs(val[u]));
  int ex = -126;
  if (mx > 0.0) {
    ex = (int)ceil(log2(mx / top));
    while (ldexp(mx, -ex) > top) ++ex;
    while (ldexp(mx, -(ex - 1)) <= top) --ex;
    ex = std::min(127, std::max(-126, ex));
  }
  return ex;
}
int fb_f6_code_e2m3(double v, int ex, double *got) {
  const double q = fabs(ldexp(v, -ex));
  const double step = q < 2.0 ? 0.125 : (q < 4.0 ? 0.25 : 0.5), base = q < 2.0 ? 0.0 : (q < 4.0 ? 2.0 : 4.0);
  int code = std::min((q < 2.0 ? 0 : (q < 4.0 ? 16 : 24)) + (int)nearbyint((q - base) / step), 31);
  const double dq = code < 16 ? code * 0.125 : (code < 24 ? 2.0 + (code - 16) * 0.25 : 4.0 + (code - 24) * 0.5);
  *got = (v < 0.0 ? -1.0 : 1.0) * ldexp(dq, ex);
  return code | (v < 0.0 ? 32 : 0);
}
int fb_f6_code_e2m1(double v, int ex, double *got) {
  const double q = fabs(ldexp(v, -ex));
  const double step = q < 2.0 ? 0.5 : (q < 4.0 ? 1.0 : 2.0), base = q < 2.0 ? 0.0 : (q < 4.0 ? 2.0 : 4.0);
  int code = std::min((q < 2.0 ? 0 : (q < 4.0 ? 4 : 6)) + (int)nearbyint((q - base) / step), 7);
  const double dq = code < 4 ? code * 0.5 : (code < 6 ? 2.0 + (code - 4) * 1.0 : 4.0 + (code - 6) * 2.0);
  *got = (v < 0.0 ? -1.0 : 1.0) * ldexp(dq, ex);
  return code | (v < 0.0 ? 8 : 0);
}
void fb_f6_put6(uint64_t (&bits)[3], int u, int code) {
  const int bit = 6 * u;
  bits[bit >> 6] |= (uint64_t)code << (bit & 63);
  if ((bit & 63) > 58) bits[(bit >> 6) + 1] |= (uint64_t)code >> (64 - (bit & 63));
}

// F6 item: [0, 5 KB) the leading f16 term as in every delta item; then, per lane (kh, cc) -- the lane that holds the
// component's K places 8 kh .. 8 kh + 7 of every chunk, as in the f16 fragments -- blocks of 32 codes with
// one power-of-two scale each (value u in bits [6u, 6u + 6) resp. [4u, 4u + 4) of the lane's operand):
//   block 0 (e2m3): u = 8 c + i, c < 4: delta's SECOND term d2 at dimension 16 c + 8 kh + i  (against x_1)
//   block L (e2m1): the same places: what block 0's codes leave of d2                     (against x_1)
//   block 1 (e2m3): the same places: delta's LEADING term times 2^-12                (against x_2 2^12)
//   block 2 (e2m3, lanes kh = 0 only -- the frames' side is zero for kh = 1 --): u < 8: d2 at dimension
//            64 + u; 8 <= u < 16: leading term 2^-12 at 64 + u - 8; 16 <= u < 24: what the first eight
//            codes leave of d2; zero where the dimension is past D and for u >= 24
// The parameters are the same for every frame, so what their rounding leaves does not average out over
// an utterance the way the frames' does: d2 in ONE e2m3 term left 1.45e-5 of an utterance average in the
// float64 model of this class (tools/probes/f6_corr_emul.py, scratch of round 4: the frames' 4 bits and
// the leading term's cost ~1e-6 each), the second term brings that to 3.8e-6.  (The 2^-12 / 2^12 pair
// keeps block 2's kinds of values inside one scale's range on both sides.)
// Bytes: the FB_F6_* offsets of fb_prepare.h.  What the codes leave out at the component's own mean is added to *cst.
void fb_gmm_f6_pack_component(uint8_t *ib, int cc, int D, const double *vv, const double *aa, const double *mean,
                              double *cst) {
  const int DC = 64;  // dimensions of the chunks 0 .. 3
  for (int kh = 0; kh < 2; ++kh) {
    const int lane = kh * 32 + cc;
    uint32_t scales = 0;
    int dim[32];
    double v2[32], v1[32], left[32], got;
    for (int u = 0; u < 32; ++u) {
      const int k = 16 * (u / 8) + 8 * kh + (u % 8);
      dim[u] = k < D && k < DC ? k : -1;
      v2[u] = dim[u] < 0 ? 0.0 : vv[k] - aa[k];
      v1[u] = dim[u] < 0 ? 0.0 : ldexp(aa[k], -12);
    }
    {  // block 0 and block L
      const int ex = fb_f6_scale_for(v2, 32, 7.5);
      uint64_t bits[3] = {0, 0, 0};
      for (int u = 0; u < 32; ++u) {
        fb_f6_put6(bits, u, fb_f6_code_e2m3(v2[u], ex, &got));
        left[u] = v2[u] - got;
      }
      memcpy(ib + FB_F6_B0_LO + (size_t)lane * 16, &bits[0], 16);
      memcpy(ib + FB_F6_B0_HI + (size_t)lane * 8, &bits[2], 8);
      scales |= (uint32_t)(ex + 127);
      const int exl = fb_f6_scale_for(left, 32, 6.0);
      uint64_t lb[2] = {0, 0};
      for (int u = 0; u < 32; ++u) {
        lb[(4 * u) >> 6] |= (uint64_t)fb_f6_code_e2m1(left[u], exl, &got) << ((4 * u) & 63);
        if (dim[u] >= 0) *cst += (left[u] - got) * mean[dim[u]];  // what both terms leave, at the component's mean
      }
      memcpy(ib + FB_F6_BL + (size_t)lane * 16, lb, 16);
      scales |= (uint32_t)(exl + 127) << 16;
    }
    {  // block 1
      const int ex = fb_f6_scale_for(v1, 32, 7.5);
      uint64_t bits[3] = {0, 0, 0};
      for (int u = 0; u < 32; ++u) fb_f6_put6(bits, u, fb_f6_code_e2m3(v1[u], ex, &got));
      memcpy(ib + FB_F6_B1_LO + (size_t)lane * 16, &bits[0], 16);
      memcpy(ib + FB_F6_B1_HI + (size_t)lane * 8, &bits[2], 8);
      scales |= (uint32_t)(ex + 127) << 8;
    }
    if (kh == 0) {  // block 2: the dimensions of chunk 4
      double val[32] = {0.0};
      for (int u = 0; u < 8; ++u) {
        const int k = DC + u;
        if (k < D) { val[u] = vv[k] - aa[k]; val[8 + u] = ldexp(aa[k], -12); }
      }
      const int ex = fb_f6_scale_for(val, 16, 7.5);
      uint64_t bits[3] = {0, 0, 0};
      for (int u = 0; u < 16; ++u) {
        fb_f6_put6(bits, u, fb_f6_code_e2m3(val[u], ex, &got));
        if (u < 8) val[16 + u] = val[u] - got;
      }
      for (int u = 16; u < 24; ++u) {
        fb_f6_put6(bits, u, fb_f6_code_e2m3(val[u], ex, &got));
        if (DC + u - 16 < D) *cst += (val[u] - got) * mean[DC + u - 16];
      }
      memcpy(ib + FB_F6_B2_LO + (size_t)cc * 16, &bits[0], 16);
      memcpy(ib + FB_F6_B2_HI + (size_t)cc * 8, &bits[2], 8);
      scales |= (uint32_t)(ex + 127) << 24;
    } else {
      scales |= 127u << 24;
    }
    memcpy(ib + FB_F6_SCALES + (size_t)lane * 4, &scales, 4);
  }
}

// ------------------------------------------------------------------------------------------------ delta images
// One component (place cc) of one item of a delta image: m = -1 the quadratic item, 0 the base model, else model m's delta
// of tile class P.
// The constants (gconst of the base model, its difference for the others) stand in the K padding against 1.0 in
// the frame operand, as THREE f16 terms at K = D, D + 1, D + 2 of the FIRST parameter term: they come out with 33
// bits whatever P.  With P = 1 a delta item's linear parameters are their leading f16 term only; what that
// leaves out at the component's own mean, sum_d (delta' - f16(delta'))_kd mu'_kd -- a constant per (model,
// component), the same for every frame the component explains --, goes into that constant.
static void pack_delta_component(const FbGmmParams &g, int NKF, const FbGmmDeltaPlan &plan, uint16_t *im, int m, int P,
                                 int c, int cc) {
  const int C = g.C, D = g.D;
  const float *gconsts = g.gconsts, *miv = g.miv, *iv = g.iv;
  const std::vector<int> &kd = plan.kd, &kq = plan.kq;
  auto at = [&](int term, int k) { return &im[fb_gmm_frag_index(term, NKF, k, cc)]; };
  // the component's mean in the frames' balanced units (mu' = mu 2^kd)
  auto mean_at = [&](int k) { return ldexp((double)miv[(size_t)c * D + k] / (double)iv[(size_t)c * D + k], kd[k]); };
  double cst = m == 0 ? L2E * (double)gconsts[c] : (m > 0 ? L2E * (double)(gconsts[(size_t)m * C + c] - gconsts[c]) : 0.0);
  double vv[96] = {0.0}, aa[96] = {0.0};  // the linear parameters and their leading f16 terms (F6 items)
  for (int k = 0; k < D; ++k) {
    double v;
    if (m < 0) v = ldexp(L2E * (double)(-0.5f * iv[(size_t)c * D + k]), -kq[k]);
    else if (m == 0) v = ldexp(L2E * (double)miv[(size_t)c * D + k], -kd[k]);
    else v = ldexp(L2E * (double)(miv[((size_t)m * C + c) * D + k] - miv[(size_t)c * D + k]), -kd[k]);
    const double a = f16r(v);
    put16(a, at(0, k));
    vv[k] = v;
    aa[k] = a;
    if (m > 0 && P == 6) continue;  // (the second half of the item holds the fp6 operands: below)
    put16(v - a, at(1, k));
    if (m > 0 && P == 1) cst += (v - a) * mean_at(k);  // the dropped second term at the component's mean
  }
  if (m > 0 && P == 6) {
    double mean[96] = {0.0};
    for (int k = 0; k < D; ++k) mean[k] = mean_at(k);
    fb_gmm_f6_pack_component(reinterpret_cast<uint8_t *>(im), cc, D, vv, aa, mean, &cst);
  }
  if (m < 0) {  // the frames' reference stands in their x^2 operand as -(R mod 2048), -(R div 2048) (gmm_wide_kernel.hip)
    put16(1.0, at(0, D + 3));
    put16(2048.0, at(0, D + 4));
  }
  if (m >= 0) {
    const double c1 = f16r(cst), c2 = f16r(cst - c1);
    put16(c1, at(0, D));
    put16(c2, at(0, D + 1));
    put16(cst - c1 - c2, at(0, D + 2));
  }
}

std::vector<uint16_t> fb_gmm_pack_delta_pass(const FbGmmParams &g, int NKF, const FbGmmDeltaPlan &plan, int pass) {
  const int n_tiles = g.C / 32;
  const size_t per_item = (size_t)2 * NKF * 64 * 8;
  const int n_items_p = 2 + plan.pass_lo[pass + 1] - plan.pass_lo[pass];  // Q, base, the pass's deltas
  std::vector<uint16_t> fd((size_t)n_tiles * n_items_p * per_item, 0);
  for (int t = 0; t < n_tiles; ++t)
    for (int it = 0; it < n_items_p; ++it) {
      uint16_t *im = &fd[((size_t)t * n_items_p + it) * per_item];
      const int m = it < 2 ? it - 1 : plan.pass_lo[pass] + it - 2;  // -1: the quadratic item, 0: the base model
      for (int cc = 0; cc < 32; ++cc) pack_delta_component(g, NKF, plan, im, m, plan.tile_p(t), plan.perm[t * 32 + cc], cc);
    }
  return fd;
}

// The anchors of k_gmm_fx2w's reference: the base model's FB_FXW_ANCHORS widest components.  The log2-likelihood
// of a frame under one of them is a lower bound of the base model's log2 sum; every other model's sum is at least
// that minus |dgconst| + |dlinear|_2 |x|_2 (Cauchy-Schwarz on the delta line above, in the frames' balanced units),
// whose two maxima over the models go along.  Table: [0, 80) the frames' balancing factors 2^kd, [80, 160) those of
// their squares 2^kq, then per anchor {80 linear terms with gconst at D, 80 quadratic terms -- in balanced units:
// the kernel evaluates them on the leading f16 term of its frame operand, hence the + 2 --, max |dgconst| + 2,
// max |dlinear|_2, 0, 0}.
std::vector<float> fb_gmm_anchor_table(const FbGmmParams &g, int NKF, const FbGmmDeltaPlan &plan, bool *fits) {
  const int M = g.M, C = g.C, D = g.D;
  const float *gconsts = g.gconsts, *miv = g.miv, *iv = g.iv;
  const std::vector<int> &kd = plan.kd, &kq = plan.kq;
  std::vector<int> order(C);
  std::vector<double> vol(C);
  for (int c = 0; c < C; ++c) {
    order[c] = c;
    double lv = 0.0;
    for (int k = 0; k < D; ++k) lv -= log((double)iv[(size_t)c * D + k]);
    vol[c] = lv;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return vol[a] > vol[b]; });
  const int W = 16 * NKF;
  std::vector<float> an(2 * W + FB_FXW_ANCHORS * (2 * W + 4), 0.0f);
  for (int k = 0; k < W; ++k) {
    an[k] = ldexpf(1.0f, kd[k]);
    an[W + k] = ldexpf(1.0f, kq[k]);
  }
  for (int a = 0; a < FB_FXW_ANCHORS; ++a) {
    const int ks = order[std::min(a, C - 1)];
    float *at = &an[2 * W + (size_t)a * (2 * W + 4)];
    for (int k = 0; k < D; ++k) {
      at[k] = (float)ldexp(L2E * (double)miv[(size_t)ks * D + k], -kd[k]);
      at[W + k] = (float)ldexp(L2E * (double)(-0.5f * iv[(size_t)ks * D + k]), -kq[k]);
    }
    at[D] = (float)(L2E * (double)gconsts[ks]);
    double mg = 0.0, ml = 0.0;
    for (int m = 1; m < M; ++m) {
      double l2 = 0.0;
      for (int k = 0; k < D; ++k) {
        const double dl = ldexp((double)miv[((size_t)m * C + ks) * D + k] - (double)miv[(size_t)ks * D + k], -kd[k]);
        l2 += dl * dl;
      }
      ml = std::max(ml, L2E * sqrt(l2));
      mg = std::max(mg, L2E * fabs((double)gconsts[(size_t)m * C + ks] - (double)gconsts[ks]));
    }
    at[2 * W] = (float)(mg * 1.000001 + 4.0);
    at[2 * W + 1] = (float)(ml * 1.000001);
  }
  // f16 copies of the anchors' 2 x W terms behind the float table: what the kernel's packed dot products read.
  // The bound stays a bound: the rounding of the copies and of the f16 squares (2^-11 each, relative to terms
  // that add up to a few hundred at most) is inside the + 2 of the slack above
  const size_t nf = an.size();
  an.resize(nf + (size_t)FB_FXW_ANCHORS * W, 0.0f);
  uint16_t *hp = reinterpret_cast<uint16_t *>(&an[nf]);
  for (int a = 0; a < FB_FXW_ANCHORS; ++a)
    for (int k = 0; k < 2 * W; ++k) {
      const float v = an[2 * W + (size_t)a * (2 * W + 4) + k];
      *fits = *fits && fabsf(v) < 60000.0f;
      const _Float16 hv = (_Float16)v;
      memcpy(&hp[(size_t)a * 2 * W + k], &hv, 2);
    }
  return an;
}

// ------------------------------------------------------------------------------------------------ the whole load
int fb_prepare_gmm(const FbGmmParams &g, const FbGmmPrepOptions &opt, FbGmmPrepared *out, std::string *err) {
  const int M = g.M, C = g.C, D = g.D;
  char msg[160];
  if (M <= 0 || C <= 0 || D <= 0) {
    snprintf(msg, sizeof(msg), "bad GMM shape M=%d C=%d D=%d", M, C, D);
    *err = msg;
    return FB_E_ARG;
  }
  if (D > 80) {
    snprintf(msg, sizeof(msg), "feature dim %d > 80 unsupported by the MFMA kernels", D);
    *err = msg;
    return FB_E_ARG;
  }
  FbGmmPrepared p;
  const FbGmmGroups gr = fb_gmm_group_by_variance(g);
  const int G = (int)gr.group_rep.size();
  p.M = M; p.C = C; p.D = D;
  p.n_groups = G;
  p.item_model = gr.item_model;
  p.n_items = (int)gr.item_model.size();
  p.n_tiles = (C + 31) / 32;
  p.NK = (D + 3 + 15) / 16 < 3 ? 3 : (D + 3 + 15) / 16;   // k_gmm_bx3 is instantiated for NK = 3..6 (zero padding is free)
  p.NKF = (D + 1 + 15) / 16 < 2 ? 2 : (D + 1 + 15) / 16;  // k_gmm_fx2 for 2..6
  p.mode = opt.forced_mode ? opt.forced_mode : FB_GMM_MODE_FX2;
  // k_gmm_fx2w scores the models of ONE variance group as deltas from model 0 (the UBM for OSI / SV, the first
  // speaker for CSI): delta images are built when the kernel's shape conditions hold (fb_gmm_use_wide); beyond
  // fb_gmm_max_wide_models() models the general kernel takes over
  p.too_many_for_wide = G == 1 && M > fb_gmm_max_wide_models() && (C & 31) == 0;
  const bool want_delta = G == 1 && M >= 2 && M <= fb_gmm_max_wide_models() && (C & 31) == 0 && p.NKF == 5 &&
                          D + 5 <= 16 * p.NKF && (D & 3) == 0;  // (K places for the constants' three terms and the frames' reference)
  FbGmmFxScaling sc = {false, 0, 0, 0, 0, 0};
  if (p.mode == FB_GMM_MODE_FX2) {
    sc = fb_gmm_fx2_scaling(g, p.NKF, want_delta);
    if (!sc.ok) p.mode = FB_GMM_MODE_BX3;
  }
  if (p.mode == FB_GMM_MODE_FX2) {
    p.kx = sc.kx; p.kx2 = sc.kx2; p.kacc = sc.kacc;
    p.fx = fb_gmm_pack_fx2(g, gr, p.NKF, sc);
    if (want_delta) {
      const FbGmmDeltaPlan plan = fb_gmm_delta_plan(g, p.NKF, opt);
      p.delta_rms = plan.delta_rms;
      p.perm = plan.perm;
      for (int q = 0; q <= FB_FXW_MAX_PASS; ++q) p.pass_lo[q] = plan.pass_lo[q];
      if (plan.fits) {  // (k_gmm_fx2 scores a model that does not fit)
        bool fits = true;
        for (int pass = 0; pass < plan.n_pass; ++pass) p.fd[pass] = fb_gmm_pack_delta_pass(g, p.NKF, plan, pass);
        p.anchor = fb_gmm_anchor_table(g, p.NKF, plan, &fits);
        if (fits) {
          p.delta_p = plan.want_p; p.delta_t3 = plan.t3; p.delta_t6 = plan.t6; p.delta_t2 = plan.t2;
          p.n_pass = plan.n_pass;
        }
      }
    }
  } else {
    p.bx = fb_gmm_pack_bx3(g, gr, p.NK);
  }
  *out = std::move(p);
  return FB_OK;
}
