// psy_kernels.hip -- the psychoacoustic distortion of fb_attack_psy (the "masking" contract of include/fakebob_hip.h), gfx950.
// The forward and the whole backward of the victim are fb_attack_wb's (wb_enqueue); these launches follow them.
//
//   k_psy_frames  one workgroup per STFT frame, the frame in LDS: delta = x - a0 under the periodic Hann window, a radix-2
//                 decimation-in-frequency FFT of W points (natural order in, bit-reversed order out), P = |X|^2 * scale against
//                 the threshold (uploaded in the same bit-reversed order, +inf above the Nyquist bin, so the one-sided mask is a
//                 compare), the hinge and n_over partials of the frame, the masked spectrum through the decimation-in-time
//                 inverse (bit-reversed in, natural out), the window again: gf[f][W], the frame's share of dD / d delta
//   k_psy_ctl     one wave, thread 0 deciding: D and n_over from the frame partials and l2 from the block partials, the two
//                 float64 sums in ascending order (cw2_wave_sum), its own trace row and `take` test, then k_cw2_ctl's
//                 decisions on dist = D + l2_weight * l2 (cw2_decide)
//   k_psy_step    element-wise: gd by overlap-add of at most four frames in ascending f, then k_cw2_step's Adam step
//                 (cw2_adam_step, cw2_block_sum) with G = (((c gate) g + gd) + l2_weight (2 (x - a0))) (1 - x x)
// All arithmetic is float64, nothing contracted; no floating-point atomics: every sum has one fixed order, so a run repeats bit
// for bit.  The twiddles come from a host table (cos and sin of 2 pi t / W, t < W / 2, exact at the octants), copied to LDS
// once per workgroup; the window is read off the same table.  What this attack shares with CW2 on the device is cw2_device.h's.
#include "cw2_device.h"

template <int W> struct PsyLog2;
template <> struct PsyLog2<512> { static constexpr int v = 9; };
template <> struct PsyLog2<1024> { static constexpr int v = 10; };
template <> struct PsyLog2<2048> { static constexpr int v = 11; };

// W / 4 threads: two butterflies per thread and stage, four points per thread in the element-wise passes.
// x, a0: [N]; delta past N is zero (the zero extension of the last frame).  theta_br[F][W]: theta[f][k] at position
// bitrev(k), +inf at the positions of k > W / 2.  scale = (8/3) / W^2 * 10^9.6 / psd_max; coef = 2 scale / (F K).
// P_out (nullable): [F][K] in natural order.  ctl (nullable): a launch behind the stopping iteration returns at once.
template <int W>
__global__ __launch_bounds__(W / 4) void k_psy_frames(const double *__restrict__ x, const double *__restrict__ a0, int64_t N,
                                                      const double *__restrict__ tw, const double *__restrict__ theta_br,
                                                      double scale, double coef, double *__restrict__ gf,
                                                      double *__restrict__ d_part, int *__restrict__ n_part,
                                                      double *__restrict__ P_out, const FbCtlDev *__restrict__ ctl) {
  constexpr int T = W / 4, H = W / 2, LOGW = PsyLog2<W>::v, NW = T / 64;
  __shared__ double re[W], im[W], tc[H], ts[H];
  __shared__ double red_d[NW];
  __shared__ int red_n[NW];
  if (ctl && ctl->stop) return;
  const int tid = threadIdx.x;
  const int f = blockIdx.x;
  const int64_t base = (int64_t)f * (W / 4);
  for (int t = tid; t < H; t += T) { tc[t] = tw[t]; ts[t] = tw[H + t]; }
  __syncthreads();
  for (int n = tid; n < W; n += T) {
    const int64_t m = base + n;
    const double d = m < N ? x[m] - a0[m] : 0.0;
    const double cs = n < H ? tc[n] : -tc[n - H];
    re[n] = d * (0.5 - 0.5 * cs);
    im[n] = 0.0;
  }
  __syncthreads();
  // forward, decimation in frequency: w = exp(-2 pi i j / (2 half))
#pragma unroll
  for (int half = H; half >= 1; half >>= 1) {
    const int tstep = H / half;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int b = tid + r * T;
      const int j = b & (half - 1);
      const int i = ((b - j) << 1) + j;
      const double ar = re[i], ai = im[i], br = re[i + half], bi = im[i + half];
      const double dr = ar - br, di = ai - bi;
      const double wr = tc[j * tstep], wi = -ts[j * tstep];
      re[i] = ar + br;
      im[i] = ai + bi;
      re[i + half] = dr * wr - di * wi;
      im[i + half] = dr * wi + di * wr;
    }
    __syncthreads();
  }
  // the hinge and the mask, position by position
  double hinge = 0.0;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int pos = tid + r * T;
    const double xr = re[pos], xi = im[pos];
    const double P = (xr * xr + xi * xi) * scale;
    const double th = theta_br[(size_t)f * W + pos];
    const bool over = P > th;
    if (over) { hinge += P - th; cnt += 1; }
    else { re[pos] = 0.0; im[pos] = 0.0; }
    if (P_out) {
      const int k = (int)(__brev((unsigned)pos) >> (32 - LOGW));
      if (k <= H) P_out[(size_t)f * (H + 1) + k] = P;
    }
  }
  // the frame's partials: within a wave by the shuffle tree, the waves in ascending order by thread 0
  for (int h = 32; h >= 1; h >>= 1) {
    hinge += __shfl_down(hinge, h, 64);
    cnt += __shfl_down(cnt, h, 64);
  }
  if ((tid & 63) == 0) { red_d[tid >> 6] = hinge; red_n[tid >> 6] = cnt; }
  __syncthreads();   // (also: the masked spectrum is complete)
  if (tid == 0) {
    double d = red_d[0];
    int c = red_n[0];
    for (int w = 1; w < NW; ++w) { d += red_d[w]; c += red_n[w]; }
    d_part[f] = d;
    n_part[f] = c;
  }
  // inverse, decimation in time: w = exp(+2 pi i j / (2 half)); only the real part of the result is read
#pragma unroll
  for (int half = 1; half <= H; half <<= 1) {
    const int tstep = H / half;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int b = tid + r * T;
      const int j = b & (half - 1);
      const int i = ((b - j) << 1) + j;
      const double ar = re[i], ai = im[i], br = re[i + half], bi = im[i + half];
      const double wr = tc[j * tstep], wi = ts[j * tstep];
      const double cr = br * wr - bi * wi, ci = br * wi + bi * wr;
      re[i] = ar + cr;
      im[i] = ai + ci;
      re[i + half] = ar - cr;
      im[i + half] = ai - ci;
    }
    __syncthreads();
  }
  for (int n = tid; n < W; n += T) {
    const double cs = n < H ? tc[n] : -tc[n - H];
    gf[(size_t)f * W + n] = (re[n] * (0.5 - 0.5 * cs)) * coef;
  }
}

// One wave, thread 0 decides (k_cw2_ctl with the perceptual distortion).  d_part / n_part: [F] of the iterate that was scored;
// l2_part[n_l2] likewise.  FK = F * K as a double.  A trace row is {dist, l2, n_over, adver_loss, c, score0[S]}.
__global__ __launch_bounds__(64) void k_psy_ctl(const FbNesDev *__restrict__ out, const double *__restrict__ scores, int S,
                                                const double *__restrict__ l2_part, int n_l2, const double *__restrict__ d_part,
                                                const int *__restrict__ n_part, int F, double FK, double l2_weight,
                                                FbPsyDev *__restrict__ ps, FbCtlDev *__restrict__ ctl, double *__restrict__ trace,
                                                int t, int abort_every) {
  __shared__ double part[64];
  const int lane = threadIdx.x;
  FbCw2Dev *cw = &ps->cw;
  if (ctl->stop) {   // behind the stopping iteration: k_psy_step has nothing to do
    if (lane == 0) cw->mode = 0;
    return;
  }
  const double l2 = cw2_wave_sum(l2_part, n_l2, part);   // ascending block order
  const double dsum = cw2_wave_sum(d_part, F, part);     // ascending frames
  int n_over = 0;                                        // (an integer sum: any order)
  for (int f = lane; f < F; f += 64) n_over += n_part[f];
  for (int h = 32; h >= 1; h >>= 1) n_over += __shfl_down(n_over, h, 64);
  if (lane != 0) return;
  const double D = __ddiv_rn(dsum, FK);
  const double dist = __dadd_rn(D, __dmul_rn(l2_weight, l2));
  const double al = out->adver_loss;
  const int row = cw->rows;
  if (trace) {
    double *r = trace + (size_t)row * (5 + S);
    r[0] = dist; r[1] = l2; r[2] = (double)n_over; r[3] = al; r[4] = cw->c;
    for (int m = 0; m < S; ++m) r[5 + m] = scores[m];
  }
  int take = 0;
  if (al < 0.0 && dist < ps->gbest_dist) { ps->gbest_dist = dist; cw->gbest_l2 = l2; ps->gbest_n_over = n_over; take = 1; }
  ps->D = D;
  ps->dist = dist;
  ps->n_over = n_over;
  cw2_decide(cw, ctl, al, l2, dist, take, row, t, abort_every);
}

// gd[n] = sum_f gf[f][n - f hop] over the frames that hold sample n (hop = W / 4: at most four), added in ascending f
__device__ __forceinline__ double psy_ola(const double *__restrict__ gf, int F, int W, int64_t n) {
  const int hop = W >> 2;
  int64_t f_hi = n / hop;
  if (f_hi > F - 1) f_hi = F - 1;
  const int64_t f_lo = n >= W ? (n - W) / hop + 1 : 0;   // the first frame with n - f hop < W
  double gd = gf[(size_t)f_lo * W + (size_t)(n - f_lo * hop)];
  for (int64_t f = f_lo + 1; f <= f_hi; ++f) gd = __dadd_rn(gd, gf[(size_t)f * W + (size_t)(n - f * hop)]);
  return gd;
}

// the overlap-add alone (the test hook: an attack's k_psy_step does it in passing)
__global__ __launch_bounds__(256) void k_psy_ola(const double *__restrict__ gf, int F, int W, int64_t N, double *__restrict__ gd) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n < N) gd[n] = psy_ola(gf, F, W, n);
}

// k_cw2_step with the masking gradient.  F > 0: gf[F][W] are the frames' gradients and gd[n] is their overlap-add, ascending f
// (hop = W / 4: at most four); F == 0: gf is gd[N] itself (the test hook).
__global__ __launch_bounds__(256) void k_psy_step(const double *__restrict__ g, const double *__restrict__ gf, int F, int W,
                                                  const double *__restrict__ a0, const double *__restrict__ w0, int64_t N,
                                                  double l2_weight, double beta1, double omb1, double beta2, double omb2,
                                                  double step_size, double bc2s, double adam_eps, double *__restrict__ mod,
                                                  double *__restrict__ m1, double *__restrict__ m2, double *__restrict__ x,
                                                  const int16_t *__restrict__ row, int16_t *__restrict__ best_row,
                                                  double *__restrict__ best_x, double *__restrict__ l2_part,
                                                  const FbPsyDev *__restrict__ ps) {
  __shared__ double lds[256];
  const FbCw2Dev *cw = &ps->cw;
  const int mode = cw->mode;   // (written by k_psy_ctl, the launch before: 0 behind a stop)
  if (mode == 0) return;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = n < N;
  if (in && (mode & 1)) { best_row[n] = row[n]; best_x[n] = x[n]; }
  if (!(mode & 2)) return;
  double d = 0.0;
  if (in) {
    const double gd = F > 0 ? psy_ola(gf, F, W, n) : gf[n];
    const double xn = x[n], an = a0[n];
    const double cg = cw->gate ? cw->c : 0.0;
    const double G = __dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(cg, g[n]), gd), __dmul_rn(l2_weight, __dmul_rn(2.0, __dsub_rn(xn, an)))),
                               __dsub_rn(1.0, __dmul_rn(xn, xn)));
    d = cw2_adam_step(G, n, an, w0, beta1, omb1, beta2, omb2, step_size, bc2s, adam_eps, mod, m1, m2, x);
  }
  d = cw2_block_sum(d, lds);
  if (threadIdx.x == 0) l2_part[blockIdx.x] = d;
}

void fb_launch_psy_frames(hipStream_t s, int W, int F, const double *x, const double *a0, int64_t N, const double *tw,
                          const double *theta_br, double scale, double coef, double *gf, double *d_part, int *n_part, double *P_out,
                          const FbCtlDev *ctl) {
  if (W == 512)
    hipLaunchKernelGGL(k_psy_frames<512>, dim3(F), dim3(128), 0, s, x, a0, N, tw, theta_br, scale, coef, gf, d_part, n_part, P_out, ctl);
  else if (W == 1024)
    hipLaunchKernelGGL(k_psy_frames<1024>, dim3(F), dim3(256), 0, s, x, a0, N, tw, theta_br, scale, coef, gf, d_part, n_part, P_out, ctl);
  else
    hipLaunchKernelGGL(k_psy_frames<2048>, dim3(F), dim3(512), 0, s, x, a0, N, tw, theta_br, scale, coef, gf, d_part, n_part, P_out, ctl);
}
void fb_launch_psy_ola(hipStream_t s, const double *gf, int F, int W, int64_t N, double *gd) {
  hipLaunchKernelGGL(k_psy_ola, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, gf, F, W, N, gd);
}
void fb_launch_psy_ctl(hipStream_t s, const FbNesDev *out, const double *scores, int S, const double *l2_part, int64_t N,
                       const double *d_part, const int *n_part, int F, int K, double l2_weight, FbPsyDev *ps, FbCtlDev *ctl,
                       double *trace, int t, int abort_every) {
  hipLaunchKernelGGL(k_psy_ctl, dim3(1), dim3(64), 0, s, out, scores, S, l2_part, (int)((N + 255) / 256), d_part, n_part, F,
                     (double)F * (double)K, l2_weight, ps, ctl, trace, t, abort_every);
}
void fb_launch_psy_step(hipStream_t s, const double *g, const double *gf, int F, int W, const double *a0, const double *w0, int64_t N,
                        double l2_weight, double beta1, double beta2, double step_size, double bc2s, double adam_eps, double *mod,
                        double *m1, double *m2, double *x, const int16_t *row, int16_t *best_row, double *best_x, double *l2_part,
                        const FbPsyDev *ps) {
  hipLaunchKernelGGL(k_psy_step, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, g, gf, F, W, a0, w0, N, l2_weight, beta1,
                     1.0 - beta1, beta2, 1.0 - beta2, step_size, bc2s, adam_eps, mod, m1, m2, x, row, best_row, best_x, l2_part, ps);
}
