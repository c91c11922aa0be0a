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
// samples is summed by a fixed tree and the blocks are added in ascending order by one thread.  Those two sums, the decisions of
// k_cw2_ctl behind its `take` test and the Adam step of k_cw2_step behind its G are cw2_device.h's, shared with psy_kernels.hip.
#include "cw2_device.h"

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
  const double l2 = cw2_wave_sum(l2_part, n_part, part);   // ascending block order
  if (lane != 0) return;
  const double al = out->adver_loss;
  const int row = cw->rows;
  if (trace) {
    double *r = trace + (size_t)row * (3 + S);
    r[0] = l2; r[1] = al; r[2] = cw->c;
    for (int m = 0; m < S; ++m) r[3 + m] = scores[m];
  }
  int take = 0;
  if (al < 0.0 && l2 < cw->gbest_l2) { cw->gbest_l2 = l2; take = 1; }
  cw2_decide(cw, ctl, al, l2, l2, take, row, t, abort_every);
}

// row: the int16 row the forward scored (the cast of x).  The Adam constants: cw2_adam_step.
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
    d = cw2_adam_step(G, n, an, w0, beta1, omb1, beta2, omb2, step_size, bc2s, adam_eps, mod, m1, m2, x);
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
