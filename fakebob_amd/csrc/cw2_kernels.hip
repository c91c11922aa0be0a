// cw2_kernels.hip -- the per-iteration arithmetic of the L2 white-box attack (fb_attack_cw2; the "CW2" contract of
// include/fakebob_hip.h), gfx950.  The forward and the whole backward are fb_attack_wb's (wb_enqueue); these launches follow them.
//
//   k_cw2_reset   start of a search step: mod = m1 = m2 = 0, x = tanh(w0), the L2 partials of x; thread 0 of block 0 resets the
//                 step's control (c, found, prev, the stop word)
//   k_cw2_l2      the L2 partials of a given x (the test hook: an attack's iterates get theirs from the launch that wrote them)
//   k_cw2_ctl     one wave, thread 0 deciding: l2 = the partials in ascending block order, gate, take, found, the best distortion,
//                 the abort rule, the trace row, the clock stamp -- decided BEFORE the element-wise launch reads them
//   k_cw2_step    element-wise: the copy to the best slots when `take`, the Adam step in tanh space, x_next, its L2 partials
// All arithmetic is float64, one rounding per operation (no contraction); division and square root are correctly rounded, so
// m1, m2 and mod are bit-exact contracts; tanh is the device library's.  No floating-point atomics: a block of 256 consecutive
// samples is summed by the fixed tree below and the blocks are added in ascending order by one thread.
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

__global__ __launch_bounds__(256) void k_cw2_reset(const double *__restrict__ w0, const double *__restrict__ a0, int64_t N, double c,
                                                   double *__restrict__ mod, double *__restrict__ m1, double *__restrict__ m2,
                                                   double *__restrict__ x, double *__restrict__ l2_part, FbCw2Dev *__restrict__ cw,
                                                   FbCtlDev *__restrict__ ctl) {
  __shared__ double lds[256];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double d = 0.0;
  if (n < N) {
    const double xn = tanh(w0[n]);
    mod[n] = 0.0; m1[n] = 0.0; m2[n] = 0.0;
    x[n] = xn;
    d = cw2_sq_diff(xn, a0[n]);
  }
  d = cw2_block_sum(d, lds);
  if (threadIdx.x != 0) return;
  l2_part[blockIdx.x] = d;
  if (blockIdx.x == 0) {   // (no other thread of this launch reads them)
    cw->c = c; cw->prev = INFINITY; cw->found = 0; cw->aborted = 0; cw->gate = 0; cw->mode = 0;
    if (ctl && !ctl->err) ctl->stop = 0;
  }
}

__global__ __launch_bounds__(256) void k_cw2_l2(const double *__restrict__ x, const double *__restrict__ a0, int64_t N,
                                                double *__restrict__ l2_part) {
  __shared__ double lds[256];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double d = cw2_block_sum(n < N ? cw2_sq_diff(x[n], a0[n]) : 0.0, lds);
  if (threadIdx.x == 0) l2_part[blockIdx.x] = d;
}

// One wave, thread 0 decides.  out / scores: the loss launch's result block and row 0 of its scores (under fb_set_eot the
// means over the replicas); l2_part[n_part]: the partials of the iterate that was scored.  t: the iteration within the search step.
__global__ __launch_bounds__(64) void k_cw2_ctl(const FbNesDev *__restrict__ out, const double *__restrict__ scores, int S,
                                                const double *__restrict__ l2_part, int n_part, FbCw2Dev *__restrict__ cw,
                                                FbCtlDev *__restrict__ ctl, double *__restrict__ trace, int t, int abort_every) {
  __shared__ double part[64];
  const int lane = threadIdx.x;
  if (ctl->stop) {   // behind the stopping iteration: k_cw2_step has nothing to do
    if (lane == 0) cw->mode = 0;
    return;
  }
  // the one wave fetches 64 partials at a time (one thread alone would wait for every load in turn: 13 us at 188 blocks);
  // thread 0 adds them in ascending block order
  double l2 = 0.0;
  for (int base = 0; base < n_part; base += 64) {
    part[lane] = base + lane < n_part ? l2_part[base + lane] : 0.0;
    __syncthreads();
    if (lane == 0) {
      const int m = n_part - base < 64 ? n_part - base : 64;
      for (int b = 0; b < m; ++b) l2 = __dadd_rn(l2, part[b]);
    }
    __syncthreads();
  }
  if (lane != 0) return;
  const double al = out->adver_loss, c = cw->c;
  const int gate = al > 0.0 ? 1 : 0;
  const double L = __dadd_rn(__dmul_rn(gate ? c : 0.0, al), l2);
  const int row = cw->rows;
  if (trace) {
    double *r = trace + (size_t)row * (3 + S);
    r[0] = l2; r[1] = al; r[2] = c;
    for (int m = 0; m < S; ++m) r[3 + m] = scores[m];
  }
  int take = 0;
  if (al < 0.0 && l2 < cw->gbest_l2) { cw->gbest_l2 = l2; take = 1; }
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

// step_size = lr / (1 - beta1^(t+1)) and bc2s = sqrt(1 - beta2^(t+1)) come from the host, the powers by repeated multiplication.
// row: the int16 row the forward scored (the cast of x).
__global__ __launch_bounds__(256) void k_cw2_step(const double *__restrict__ g, const double *__restrict__ a0,
                                                  const double *__restrict__ w0, int64_t N, double beta1, double omb1, double beta2,
                                                  double omb2, double step_size, double bc2s, double adam_eps,
                                                  double *__restrict__ mod, double *__restrict__ m1, double *__restrict__ m2,
                                                  double *__restrict__ x, const int16_t *__restrict__ row,
                                                  int16_t *__restrict__ best_row, double *__restrict__ best_x,
                                                  double *__restrict__ l2_part, const FbCw2Dev *__restrict__ cw) {
  __shared__ double lds[256];
  const int mode = cw->mode;   // (written by k_cw2_ctl, the launch before: 0 behind a stop)
  if (mode == 0) return;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = n < N;
  if (in && (mode & 1)) { best_row[n] = row[n]; best_x[n] = x[n]; }
  if (!(mode & 2)) return;
  double d = 0.0;
  if (in) {
    const double xn = x[n], an = a0[n];
    const double cg = cw->gate ? cw->c : 0.0;
    const double G = __dmul_rn(__dadd_rn(__dmul_rn(cg, g[n]), __dmul_rn(2.0, __dsub_rn(xn, an))), __dsub_rn(1.0, __dmul_rn(xn, xn)));
    const double a = __dadd_rn(__dmul_rn(beta1, m1[n]), __dmul_rn(omb1, G));
    const double b = __dadd_rn(__dmul_rn(beta2, m2[n]), __dmul_rn(__dmul_rn(omb2, G), G));
    m1[n] = a;
    m2[n] = b;
    const double den = __dadd_rn(__ddiv_rn(__dsqrt_rn(b), bc2s), adam_eps);
    const double md = __dsub_rn(mod[n], __ddiv_rn(__dmul_rn(step_size, a), den));
    mod[n] = md;
    const double xo = tanh(__dadd_rn(w0[n], md));
    x[n] = xo;
    d = cw2_sq_diff(xo, an);
  }
  d = cw2_block_sum(d, lds);
  if (threadIdx.x == 0) l2_part[blockIdx.x] = d;
}

static inline unsigned cw2_blocks(int64_t N) { return (unsigned)((N + 255) / 256); }

void fb_launch_cw2_reset(hipStream_t s, const double *w0, const double *a0, int64_t N, double c, double *mod, double *m1, double *m2,
                         double *x, double *l2_part, FbCw2Dev *cw, FbCtlDev *ctl) {
  hipLaunchKernelGGL(k_cw2_reset, dim3(cw2_blocks(N)), dim3(256), 0, s, w0, a0, N, c, mod, m1, m2, x, l2_part, cw, ctl);
}
void fb_launch_cw2_l2(hipStream_t s, const double *x, const double *a0, int64_t N, double *l2_part) {
  hipLaunchKernelGGL(k_cw2_l2, dim3(cw2_blocks(N)), dim3(256), 0, s, x, a0, N, l2_part);
}
void fb_launch_cw2_ctl(hipStream_t s, const FbNesDev *out, const double *scores, int S, const double *l2_part, int64_t N, FbCw2Dev *cw,
                       FbCtlDev *ctl, double *trace, int t, int abort_every) {
  hipLaunchKernelGGL(k_cw2_ctl, dim3(1), dim3(64), 0, s, out, scores, S, l2_part, (int)cw2_blocks(N), cw, ctl, trace, t, abort_every);
}
void fb_launch_cw2_step(hipStream_t s, const double *g, const double *a0, const double *w0, int64_t N, double beta1, double beta2,
                        double step_size, double bc2s, double adam_eps, double *mod, double *m1, double *m2, double *x,
                        const int16_t *row, int16_t *best_row, double *best_x, double *l2_part, const FbCw2Dev *cw) {
  hipLaunchKernelGGL(k_cw2_step, dim3(cw2_blocks(N)), dim3(256), 0, s, g, a0, w0, N, beta1, 1.0 - beta1, beta2, 1.0 - beta2, step_size,
                     bc2s, adam_eps, mod, m1, m2, x, row, best_row, best_x, l2_part, cw);
}
