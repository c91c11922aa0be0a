// whitebox_device.h -- the one-thread bodies of the white-box loop, shared by k_wb_ctl (whitebox_kernels.hip) and its
// per-replica form k_wb_ctl_rep (whitebox_bpda_kernels.hip), and by k_wb_iv_ctl (whitebox_iv_kernels.hip) and its per-replica
// form k_wb_iv_ctl_rep (whitebox_universal_kernels.hip).
#pragma once
#include <math.h>

#include "fb_device.h"
#include "fb_kernels.h"

// w[M] = d loss / d raw[m] from the system scores scores[S].  The maxima take the FIRST maximal index, as fb_loss_row and
// make_decisions do (replace on strict >).
__device__ __forceinline__ void fb_wb_weights(const double *__restrict__ scores, int M, int task, int attack_type,
                                              const double *__restrict__ z_std, double threshold, int target, int true_label,
                                              double *__restrict__ w) {
  const int S = task == FB_TASK_CSI ? M : M - 1;
  for (int m = 0; m < M; ++m) w[m] = 0.0;
  auto first_max_but = [&](int skip) -> int {
    int idx = -1;
    double om = -INFINITY;
    for (int m = 0; m < S; ++m)
      if (m != skip && scores[m] > om) { om = scores[m]; idx = m; }
    return idx;
  };
  if (task == FB_TASK_SV) {                                     // (thr + kappa) - s[0]
    w[1] = -1.0; w[0] = 1.0;
  } else if (task == FB_TASK_OSI && attack_type == FB_UNTARGETED) {   // (thr + kappa) - max s
    const int j = first_max_but(-1);
    if (j >= 0) { w[1 + j] = -1.0; w[0] = 1.0; }
  } else if (task == FB_TASK_OSI) {                             // (max(max_{j != t} s[j], thr) + kappa) - s[t]
    const int j = first_max_but(target);
    double ubm = 1.0;
    w[1 + target] = -1.0;
    if (j >= 0 && scores[j] > threshold) { w[1 + j] = 1.0; ubm = 0.0; }
    w[0] = ubm;
  } else if (attack_type == FB_TARGETED) {                      // (max_{j != t} s[j] + kappa) - s[t]
    const int j = first_max_but(target);
    w[target] = -1.0 / z_std[target];
    if (j >= 0) w[j] = 1.0 / z_std[j];
  } else {                                                      // (s[true] + kappa) - max_{j != true} s[j]
    const int j = first_max_but(true_label);
    w[true_label] = 1.0 / z_std[true_label];
    if (j >= 0) w[j] = -1.0 / z_std[j];
  }
}

// ... for an i-vector system: w[S] = d loss / d raw[s].  Such a system scores (raw[s] - z_mean[s]) / z_std[s] in every task
// (fb_loss_row, znorm_all), so d loss / d raw[s] = (d loss / d score_s) / z_std[s]; the same first-maximum rule
__device__ __forceinline__ void fb_wb_iv_weights(const double *__restrict__ scores, int S, int task, int attack_type,
                                                 const double *__restrict__ z_std, double threshold, int target, int true_label,
                                                 double *__restrict__ w) {
  for (int s = 0; s < S; ++s) w[s] = 0.0;
  auto first_max_but = [&](int skip) -> int {
    int idx = -1;
    double om = -INFINITY;
    for (int m = 0; m < S; ++m)
      if (m != skip && scores[m] > om) { om = scores[m]; idx = m; }
    return idx;
  };
  if (task == FB_TASK_SV) {                                           // (thr + kappa) - s[0]
    w[0] = -1.0 / z_std[0];
  } else if (task == FB_TASK_OSI && attack_type == FB_UNTARGETED) {   // (thr + kappa) - max s
    const int j = first_max_but(-1);
    if (j >= 0) w[j] = -1.0 / z_std[j];
  } else if (task == FB_TASK_OSI) {                                   // (max(max_{j != t} s[j], thr) + kappa) - s[t]
    const int j = first_max_but(target);
    w[target] = -1.0 / z_std[target];
    if (j >= 0 && scores[j] > threshold) w[j] = 1.0 / z_std[j];
  } else if (attack_type == FB_TARGETED) {                            // (max_{j != t} s[j] + kappa) - s[t]
    const int j = first_max_but(target);
    w[target] = -1.0 / z_std[target];
    if (j >= 0) w[j] = 1.0 / z_std[j];
  } else {                                                            // (s[true] + kappa) - max_{j != true} s[j]
    const int j = first_max_but(true_label);
    w[true_label] = 1.0 / z_std[true_label];
    if (j >= 0) w[j] = -1.0 / z_std[j];
  }
}

// FakeBob.attack's loop control on the result block `out` and the scores of the trace row (k_wb_ctl's description)
__device__ __forceinline__ void fb_wb_loop_control(const double *__restrict__ scores, const FbNesDev *__restrict__ out, int M,
                                                   int task, FbCtlDev *__restrict__ ctl, double *__restrict__ trace, int it) {
  const int S = task == FB_TASK_CSI ? M : M - 1;
  // FakeBob.attack's loop control (FAKEBOB.py:181, :195-200) with adver_loss in the plateau window: there is no noisy mean
  if (out->err) { ctl->err = out->err; ctl->stop = 1; return; }
  const double al = out->adver_loss;
  double lr = ctl->lr;
  if (al < 0.0 && !ctl->disable_stop) {
    ctl->stop = 1; ctl->broke = 1; ctl->stop_iter = it;
  } else if (ctl->plateau_length > 0) {
    const int PL = ctl->plateau_length;
    int n = ctl->n_ls;
    double *ls = ctl->ls;
    if (n < PL) {
      ls[n++] = al;
    } else {
      for (int i = 1; i < PL; ++i) ls[i - 1] = ls[i];
      ls[PL - 1] = al;
    }
    if (n == PL && ls[PL - 1] > ls[0]) {
      if (lr > ctl->min_lr) {
        const double l2 = lr / ctl->plateau_drop;
        lr = l2 > ctl->min_lr ? l2 : ctl->min_lr;
        ctl->lr = lr;
      }
      n = 0;
    }
    ctl->n_ls = n;
  }
  if (trace) {
    double *row = trace + (size_t)it * (3 + S);
    row[0] = out->distance; row[1] = al; row[2] = lr;
    for (int m = 0; m < S; ++m) row[3 + m] = scores[m];
  }
  if (ctl->ticks) ctl->ticks[it + 1] = wall_clock64();
  ctl->iters_done = it + 1;
}
