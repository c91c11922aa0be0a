// cw2_device.h -- what the tanh-space attacks share on the device (fb_attack_cw2: cw2_kernels.hip; fb_attack_psy:
// psy_kernels.hip): the fixed summation orders of the L2 contract, the decisions of a control kernel behind its own distortion
// and `take` test, and the Adam step of a step kernel behind its own expression for G.  The only definitions of each.
// All arithmetic is float64, one rounding per operation; no floating-point atomics.
#pragma once
#include <math.h>

#include "fb_device.h"
#include "fb_kernels.h"

// The sum of the 256 terms d[0 .. 255] of a block (terms past N are +0.0), lane i holding d[i]: for h = 128, 64, 32, ..., 1 in
// this order d[i] = d[i] + d[i + h] for every i < h; the block's sum is d[0].  (h = 128 and 64 through LDS, the rest inside
// wave 0.)  Valid in thread 0.
__device__ __forceinline__ double cw2_block_sum(double d, double *__restrict__ lds) {
  const int i = threadIdx.x;
  lds[i] = d;
  __syncthreads();
  if (i < 128) lds[i] = __dadd_rn(lds[i], lds[i + 128]);
  __syncthreads();
  if (i >= 64) return 0.0;
  d = __dadd_rn(lds[i], lds[i + 64]);
  for (int h = 32; h >= 1; h >>= 1) d = __dadd_rn(d, __shfl_down(d, h, 64));
  return d;
}

__device__ __forceinline__ double cw2_sq_diff(double x, double a) {
  const double d = __dsub_rn(x, a);
  return __dmul_rn(d, d);
}

// ((0 + src[0]) + src[1]) + ... + src[n - 1] by a workgroup of one wave: the wave fetches 64 partials at a time into part[64]
// (one thread alone would wait for every load in turn: 13 us at 188 blocks), thread 0 adds them in ascending order.  Valid in
// thread 0.
__device__ __forceinline__ double cw2_wave_sum(const double *__restrict__ src, int n, double *__restrict__ part) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int base = 0; base < n; base += 64) {
    part[lane] = base + lane < n ? src[base + lane] : 0.0;
    __syncthreads();
    if (lane == 0) {
      const int m = n - base < 64 ? n - base : 64;
      for (int b = 0; b < m; ++b) s = __dadd_rn(s, part[b]);
    }
    __syncthreads();
  }
  return s;
}

// What a control kernel's deciding thread does once it has the distortion `dist` of the scored iterate (CW2: l2 itself) and
// its own `take`: gate, L = (c gate) adver_loss + dist, found, the abort rule on L, then l2 / gate / take / mode / rows for the
// step launch and the host, iters_done and the clock stamp.  row = cw->rows, the trace row this iteration wrote.
__device__ __forceinline__ void cw2_decide(FbCw2Dev *__restrict__ cw, FbCtlDev *__restrict__ ctl, double al, double l2, double dist,
                                           int take, int row, int t, int abort_every) {
  const int gate = al > 0.0 ? 1 : 0;
  const double L = __dadd_rn(__dmul_rn(gate ? cw->c : 0.0, al), dist);
  if (al < 0.0) cw->found = 1;
  int step = 1;
  if (abort_every > 0 && t % abort_every == 0) {
    if (L > __dmul_rn(0.9999, cw->prev)) { step = 0; cw->aborted = 1; ctl->stop = 1; }   // the row is written, no step is taken
    else cw->prev = L;
  }
  cw->l2 = l2;
  cw->gate = gate;
  cw->take = take;
  cw->mode = take | (step << 1);
  cw->rows = row + 1;
  ctl->iters_done = row + 1;
  if (ctl->ticks) ctl->ticks[row + 1] = wall_clock64();
}

// Element n of a step kernel from its G on: the moments, mod, x = tanh(w0 + mod); returns the new (x - a0)^2 (an = a0[n]).
// omb = 1 - beta; step_size = lr / (1 - beta1^(t+1)) and bc2s = sqrt(1 - beta2^(t+1)) come from the host, the powers by
// repeated multiplication.
__device__ __forceinline__ double cw2_adam_step(double G, int64_t n, double an, const double *__restrict__ w0,
                                                double beta1, double omb1, double beta2, double omb2, double step_size, double bc2s,
                                                double adam_eps, double *__restrict__ mod, double *__restrict__ m1,
                                                double *__restrict__ m2, double *__restrict__ x) {
  const double a = __dadd_rn(__dmul_rn(beta1, m1[n]), __dmul_rn(omb1, G));
  const double b = __dadd_rn(__dmul_rn(beta2, m2[n]), __dmul_rn(__dmul_rn(omb2, G), G));
  m1[n] = a;
  m2[n] = b;
  const double den = __dadd_rn(__ddiv_rn(__dsqrt_rn(b), bc2s), adam_eps);
  const double md = __dsub_rn(mod[n], __ddiv_rn(__dmul_rn(step_size, a), den));
  mod[n] = md;
  const double xo = tanh(__dadd_rn(w0[n], md));
  x[n] = xo;
  return cw2_sq_diff(xo, an);
}
