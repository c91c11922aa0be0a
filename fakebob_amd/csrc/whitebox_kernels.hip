// whitebox_kernels.hip -- the analytic gradient of the GMM-UBM victim (fb_get_grad_wb / fb_attack_wb; the "white-box
// gradients" contract of include/fakebob_hip.h), gfx950.
//
//   k_wb_ctl          loss weights w[M] = d loss / d raw[m] from the scores the forward left, and the attack's loop control
//   k_wb_gmm_bwd      the GMM backward on the compacted feature rows, per model (f32-input MFMA, online soft-max)
//   k_wb_sum_models   g = (1 / Tv) sum_m w_m part_m, float64, models ascending
//   k_wb_vad_scatter  the forward's voiced mask from its MFCC matrix; the cotangent scattered to the voiced frames
//   k_wb_cmvn_t       sliding-CMVN transpose
//   k_wb_delta_t      add-deltas transpose (clamped time index)
//   k_wb_mfcc_t       MFCC transpose per frame: the frame's forward recomputed in float64, then backwards through lifter,
//                     DCT, log mel, mel weights, power spectrum (one inverse transform of dP_k F_k), window, pre-emphasis, DC
//   k_wb_overlap_add  frames -> samples through the forward's index rule (reflection included), frames ascending
//   k_wb_update       the reference's momentum sign step on a gradient vector (FAKEBOB.py:193-203)
// No floating-point atomics anywhere: every sum has a fixed order, so a call gives the same bits on any engine.
#include <float.h>
#include <math.h>

#include "fb_device.h"
#include "fb_kernels.h"
#include "whitebox_device.h"

typedef float wb_f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ weights + loop control
// One thread.  scores[S]: row 0 of the loss launch's system scores; out: its result block.  The maxima take the FIRST maximal
// index, as fb_loss_row and make_decisions do (replace on strict >).
__global__ __launch_bounds__(64) void k_wb_ctl(const double *__restrict__ scores, const FbNesDev *__restrict__ out, int M, int task,
                                               int attack_type, const double *__restrict__ z_std, double threshold, int target,
                                               int true_label, double *__restrict__ w, FbCtlDev *__restrict__ ctl,
                                               double *__restrict__ trace, int it) {
  if (threadIdx.x != 0) return;
  if (ctl && ctl->stop) return;
  fb_wb_weights(scores, M, task, attack_type, z_std, threshold, target, true_label, w);
  if (ctl) fb_wb_loop_control(scores, out, M, task, ctl, trace, it);
}

void fb_launch_wb_ctl(hipStream_t s, const double *scores, const FbNesDev *out, int M, int task, int attack_type,
                      const double *z_std, double threshold, int target, int true_label, double *w, FbCtlDev *ctl, double *trace,
                      int it) {
  hipLaunchKernelGGL(k_wb_ctl, dim3(1), dim3(64), 0, s, scores, out, M, task, attack_type, z_std, threshold, target, true_label, w,
                     ctl, trace, it);
}

// ------------------------------------------------------------------------------------------------ GMM backward
// part[m][t][d] = sum_c gamma_mtc (miv_mc[d] - iv_mc[d] x_t[d]) for the voiced rows x_t of `feats` and every model with
// w[m] != 0 (the others return at once); row_base_ptr (nullable): the first of them, a row index into `feats`.  A workgroup
// takes 16 rows of one model; its four waves take the 16-component tiles
// c, c + 4, ... and merge their online soft-max states through LDS in wave order.  Everything is the transposed problem, so
// that no value changes lanes between the two products:
//   S^T [comp][row] = P [comp][k] E [k][row],  k over {x (D, padded to quads), -x^2 / 2 (likewise), 1}   v_mfma_f32_16x16x4_f32
//   the result has the row on lane & 15 and components 4 (lane >> 4) + r in register r; exp(S^T - max) of register r is the
//   B operand of k-step r of
//   O^T [d][row] += MIV^T [d][comp] G [comp][row]   (and IV^T likewise), with the A operand's component 4 (lane >> 4) + r.
// The f32-input MFMA is an exact float32 fma chain: component log-likelihoods (hundreds in magnitude) keep ~1e-4 absolute.
#define FB_WB_ROWS 16
#define FB_WB_MAX_KS 41   // k-steps of the first product: 2 ceil(D / 4) + 1, D <= 80
#define FB_WB_MAX_DT 5    // 16-wide tiles of D

__global__ __launch_bounds__(256) void k_wb_gmm_bwd(int C, int D, const float *__restrict__ gc, const float *__restrict__ miv,
                                                    const float *__restrict__ iv, const float *__restrict__ feats,
                                                    const int *__restrict__ n_rows_ptr, const int *__restrict__ row_base_ptr,
                                                    int rows_cap, const double *__restrict__ w,
                                                    float *__restrict__ part, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int m = blockIdx.y;
  if (w[m] == 0.0) return;
  const int n_rows = min(*n_rows_ptr, rows_cap);
  if (row_base_ptr) feats += (size_t)*row_base_ptr * D;   // (a replica's rows within the batch's compacted rows)
  const int f0 = blockIdx.x * FB_WB_ROWS;
  if (f0 >= n_rows) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & 15, lg = lane >> 4;
  const int Dq = (D + 3) >> 2, ks = 2 * Dq + 1, ndt = (D + 15) >> 4;
  const float *x = feats + (size_t)min(f0 + lc, n_rows - 1) * D;
  float xe[FB_WB_MAX_KS];
#pragma unroll
  for (int s = 0; s < FB_WB_MAX_KS; ++s) {
    float v = 0.0f;
    if (s < Dq) {
      const int k = 4 * s + lg;
      if (k < D) v = x[k];
    } else if (s < 2 * Dq) {
      const int k = 4 * (s - Dq) + lg;
      if (k < D) { const float t = x[k]; v = -0.5f * (t * t); }
    } else if (s == 2 * Dq) {
      v = lg == 0 ? 1.0f : 0.0f;
    }
    xe[s] = v;
  }
  const float *gcm = gc + (size_t)m * C, *mivm = miv + (size_t)m * C * D, *ivm = iv + (size_t)m * C * D;
  wb_f32x4 o1[FB_WB_MAX_DT], o2[FB_WB_MAX_DT];
#pragma unroll
  for (int t = 0; t < FB_WB_MAX_DT; ++t) { o1[t] = wb_f32x4{0.f, 0.f, 0.f, 0.f}; o2[t] = wb_f32x4{0.f, 0.f, 0.f, 0.f}; }
  float m_run = -INFINITY, l_run = 0.0f;
  const int n_tiles = (C + 15) >> 4;
  for (int ct = wave; ct < n_tiles; ct += 4) {
    const int c0 = ct * 16;
    const int ca = min(c0 + lc, C - 1);
    const float *pm = mivm + (size_t)ca * D, *pv = ivm + (size_t)ca * D;
    const float g0 = gcm[ca];
    wb_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < FB_WB_MAX_KS; ++s) {
      if (s < ks) {
        float a = 0.0f;
        if (s < Dq) {
          const int k = 4 * s + lg;
          if (k < D) a = pm[k];
        } else if (s < 2 * Dq) {
          const int k = 4 * (s - Dq) + lg;
          if (k < D) a = pv[k];
        } else {
          a = lg == 0 ? g0 : 0.0f;
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xe[s], acc, 0, 0, 0);
      }
    }
    // register r: component c0 + 4 lg + r of row lc
    float p[4];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = (c0 + 4 * lg + r < C) ? acc[r] : -INFINITY;
      mx = fmaxf(mx, p[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // (finite: a tile holds at least one component)
    const float m_new = fmaxf(m_run, mx);
    const float sc = expf(m_run - m_new);     // (exp(-inf) = 0 at the first tile)
    float ps = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { p[r] = expf(p[r] - m_new); ps += p[r]; }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * sc + ps;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < FB_WB_MAX_DT; ++t) { o1[t] *= sc; o2[t] *= sc; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cb = c0 + 4 * lg + r;
      const float *qm = mivm + (size_t)min(cb, C - 1) * D, *qv = ivm + (size_t)min(cb, C - 1) * D;
#pragma unroll
      for (int t = 0; t < FB_WB_MAX_DT; ++t) {
        if (t < ndt) {
          const int d = 16 * t + lc;
          const bool ok = cb < C && d < D;
          const float a1 = ok ? qm[d] : 0.0f, a2 = ok ? qv[d] : 0.0f;
          o1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, p[r], o1[t], 0, 0, 0);
          o2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, p[r], o2[t], 0, 0, 0);
        }
      }
    }
  }
  // merge the four waves' states in wave order
  __shared__ float s_m[4][FB_WB_ROWS], s_l[4][FB_WB_ROWS];
  __shared__ float s_o[4][2][FB_WB_MAX_DT][4][64];
  if (lg == 0) { s_m[wave][lc] = m_run; s_l[wave][lc] = l_run; }
#pragma unroll
  for (int t = 0; t < FB_WB_MAX_DT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s_o[wave][0][t][r][lane] = o1[t][r]; s_o[wave][1][t][r][lane] = o2[t][r]; }
  __syncthreads();
  for (int idx = threadIdx.x; idx < FB_WB_ROWS * D; idx += 256) {
    const int f = idx / D, d = idx - f * D;
    if (f0 + f >= n_rows) continue;
    float mm = s_m[0][f];
    for (int v = 1; v < 4; ++v) mm = fmaxf(mm, s_m[v][f]);
    const int t = d >> 4, row = d & 15, ln = (row >> 2) * 16 + f, r = row & 3;
    float L = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int v = 0; v < 4; ++v) {
      const float e = expf(s_m[v][f] - mm);
      L += s_l[v][f] * e;
      a1 += s_o[v][0][t][r][ln] * e;
      a2 += s_o[v][1][t][r][ln] * e;
    }
    const float xv = feats[(size_t)(f0 + f) * D + d];
    part[((size_t)m * rows_cap + f0 + f) * D + d] = (a1 - a2 * xv) / L;
  }
}

// g[t][d] = (sum over the models with w[m] != 0, ascending, of w[m] part[m][t][d]) / Tv
__global__ __launch_bounds__(256) void k_wb_sum_models(int M, int D, const int *__restrict__ n_rows_ptr, int rows_cap,
                                                       const double *__restrict__ w, const float *__restrict__ part,
                                                       double *__restrict__ g, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int n_rows = min(*n_rows_ptr, rows_cap);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_rows * D) return;
  double acc = 0.0;
  for (int m = 0; m < M; ++m) {
    const double wm = w[m];
    if (wm != 0.0) acc += wm * (double)part[(size_t)m * rows_cap * D + i];
  }
  g[i] = acc / (double)n_rows;
}

void fb_launch_wb_gmm_backward(hipStream_t s, int M, int C, int D, const float *gc, const float *miv, const float *iv,
                               const float *feats, const int *n_rows_ptr, int rows_cap, const double *w, float *part, double *g,
                               const int *stop, const int *row_base_ptr) {
  hipLaunchKernelGGL(k_wb_gmm_bwd, dim3((unsigned)((rows_cap + FB_WB_ROWS - 1) / FB_WB_ROWS), (unsigned)M), dim3(256), 0, s, C, D, gc,
                     miv, iv, feats, n_rows_ptr, row_base_ptr, rows_cap, w, part, stop);
  hipLaunchKernelGGL(k_wb_sum_models, dim3((unsigned)(((size_t)rows_cap * D + 255) / 256)), dim3(256), 0, s, M, D, n_rows_ptr, rows_cap,
                     w, part, g, stop);
}

// ------------------------------------------------------------------------------------------------ front-end backward
// deterministic sum over a 256-thread workgroup (fixed tree); every thread gets the result
__device__ __forceinline__ double wb_block_sum(double v, double *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// The forward's voiced mask of the ONE utterance (frames 0 .. T - 1 of mfcc), by k_vad's own arithmetic; rank[t] = the
// frame's row among the voiced ones or -1; dcm[t][j] = cot[rank[t]][j] or 0.  tv_fwd (nullable): the forward's count --
// a different count raises *status (the mask would not be the forward's).
__global__ __launch_bounds__(256) void k_wb_vad_scatter(FbFrontendDev fe, const float *__restrict__ mfcc, int T,
                                                        const double *__restrict__ cot, const int *__restrict__ tv_fwd,
                                                        int *__restrict__ rank, double *__restrict__ dcm,
                                                        int *__restrict__ status, const int *__restrict__ stop) {
  if (stop && *stop) return;
  __shared__ double red[256];
  __shared__ float s_thr;
  double part = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) part += (double)mfcc[(size_t)t * fe.nc];
  red[threadIdx.x] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) s_thr = (float)(fe.vad_thr + fe.vad_mean_scale * red[0] / (double)T);
  __syncthreads();
  const float thr = s_thr;
  for (int t = threadIdx.x; t < T; t += 256) {
    int num = 0, den = 0;
    for (int t2 = t - fe.vad_ctx; t2 <= t + fe.vad_ctx; ++t2)
      if (t2 >= 0 && t2 < T) { ++den; if (mfcc[(size_t)t2 * fe.nc] > thr) ++num; }
    rank[t] = ((float)num >= (float)den * fe.vad_prop) ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < T; ++t) rank[t] = rank[t] ? run++ : -1;
    if (tv_fwd && *tv_fwd != run) *status = 1;
  }
  __syncthreads();
  const int dim = fe.dim;
  for (int i = threadIdx.x; i < T * dim; i += 256) {
    const int t = i / dim, r = rank[t];
    dcm[i] = r >= 0 ? cot[(size_t)r * dim + (i - t * dim)] : 0.0;
  }
}

// apply-cmvn-sliding's window of frame t: [wb, we)
__device__ __forceinline__ void wb_cmn_window(int t, int T, int Wn, int &wb, int &we) {
  wb = t - Wn / 2;
  we = wb + Wn;
  if (wb < 0) { we -= wb; wb = 0; }
  if (we > T) { wb -= we - T; we = T; if (wb < 0) wb = 0; }
}
// ddf[u][j] = dcm[u][j] + sum over the frames t whose window holds u, ascending, of alpha_t dcm[t][j],
// alpha_t = (float)(-1 / (we - wb)) as the forward has it
__global__ __launch_bounds__(256) void k_wb_cmvn_t(int T, int dim, int Wn, const double *__restrict__ dcm, double *__restrict__ ddf,
                                                   const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * dim) return;
  const int u = i / dim, j = i - u * dim;
  double acc = 0.0;
  const int lo = max(0, u - Wn), hi = min(T - 1, u + Wn);
  for (int t = lo; t <= hi; ++t) {
    int wb, we;
    wb_cmn_window(t, T, Wn, wb, we);
    if (u >= wb && u < we) acc += (double)(float)(-1.0 / (double)(we - wb)) * dcm[(size_t)t * dim + j];
  }
  ddf[i] = dcm[i] + acc;
}

// dmf[tt][d] = sum over t ascending, orders i, taps j with clamp(t + j) == tt of scale_i[j] ddf[t][i nc + d]
__global__ __launch_bounds__(256) void k_wb_delta_t(FbFrontendDev fe, int T, const double *__restrict__ ddf, double *__restrict__ dmf,
                                                    const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nc = fe.nc;
  if (idx >= T * nc) return;
  const int tt = idx / nc, d = idx - tt * nc;
  const int R = fe.order * fe.dwin, maxlen = 2 * R + 1;
  double acc = 0.0;
  for (int t = max(0, tt - R); t <= min(T - 1, tt + R); ++t)
    for (int i = 0; i <= fe.order; ++i) {
      const int off = i * fe.dwin;
      const double *sc = fe.dscale + (size_t)i * maxlen;
      const double v = ddf[(size_t)t * fe.dim + i * nc + d];
      for (int j = -off; j <= off; ++j) {
        int tc = t + j;
        tc = tc < 0 ? 0 : (tc > T - 1 ? T - 1 : tc);
        if (tc == tt) acc += sc[j + off] * v;
      }
    }
  dmf[idx] = acc;
}

// the sample frame position (start + s) reads: the forward's rule, reflected until it is inside [0, n)
__device__ __forceinline__ int64_t wb_reflect(int64_t k, int64_t n) {
  while (k < 0 || k >= n) k = k < 0 ? -k - 1 : 2 * n - 1 - k;
  return k;
}
__device__ __forceinline__ int64_t wb_frame_start(const FbFrontendDev &fe, int f) {
  return fe.snip_edges ? (int64_t)f * fe.shift : (int64_t)f * fe.shift + fe.shift / 2 - fe.L / 2;
}

// in-place radix-2 complex FFT of P points in LDS, 256 threads; inverse: conjugate twiddles, not normalised.
// tw[k] = exp(-2 pi i k / P), k <= P / 2 (FbFrontendDev::tw_full)
__device__ __forceinline__ void wb_fft(double *re, double *im, int P, const double *__restrict__ tw, bool inverse) {
  int bits = 0;
  while ((1 << bits) < P) ++bits;
  __syncthreads();
  for (int i = threadIdx.x; i < P; i += 256) {
    const int r = (int)(__brev((unsigned)i) >> (32 - bits));
    if (r > i) {
      double a = re[i]; re[i] = re[r]; re[r] = a;
      a = im[i]; im[i] = im[r]; im[r] = a;
    }
  }
  for (int len = 2; len <= P; len <<= 1) {
    const int half = len >> 1, step = P / len;
    __syncthreads();
    for (int b = threadIdx.x; b < P / 2; b += 256) {
      const int k = b % half, i0 = (b / half) * len + k, i1 = i0 + half;
      const double wr = tw[2 * (k * step)], wi = inverse ? -tw[2 * (k * step) + 1] : tw[2 * (k * step) + 1];
      const double xr = re[i1] * wr - im[i1] * wi, xi = re[i1] * wi + im[i1] * wr;
      re[i1] = re[i0] - xr; im[i1] = im[i0] - xi;
      re[i0] = re[i0] + xr; im[i0] = im[i0] + xi;
    }
  }
  __syncthreads();
}

#define FB_WB_MAX_P 512
#define FB_WB_MAX_NB 128
// One workgroup per frame: dxf[f][s] = d <dmf[f], mfcc(frame f)> / d (the frame's s-th sample as extracted), float64.
// A floor that is active contributes nothing: a mel energy below FLT_EPSILON, a frame energy below it, energy_floor.
// dk (fb_set_wb_frontend): with dk.amp > 0 the frame is recomputed from what the forward extracted under Kaldi's dither,
// (double) x + amp (double) z, z the normal of (utterance dk.utt0, frame f, sample s) of the dither RNG contract -- the draws
// k_mfcc / k_mfcc_f32 added, constants here (additive: the derivative with respect to the sample is unchanged).  amp = 0 draws
// nothing and computes what the kernel computed before it took the key.
__global__ __launch_bounds__(256) void k_wb_mfcc_t(FbFrontendDev fe, const int16_t *__restrict__ wav, int64_t n,
                                                   const double *__restrict__ dmf, double *__restrict__ dxf,
                                                   const int *__restrict__ stop, FbDitherKey dk) {
  if (stop && *stop) return;
  __shared__ double re[FB_WB_MAX_P], im[FB_WB_MAX_P], xs[FB_WB_MAX_P], aux[FB_WB_MAX_P], red[256];
  __shared__ double s_de[FB_WB_MAX_NB], s_dc[FB_WB_MAX_NB];
  const int f = blockIdx.x, L = fe.L, P = fe.P, nb = fe.nb, nc = fe.nc, nfft = P / 2;
  const int64_t start = wb_frame_start(fe, f);
  const double eps = (double)FLT_EPSILON;
  // ---- the frame's forward
  double v = 0.0;
  if (dk.amp > 0.0) {
    for (int s = threadIdx.x; s < L; s += 256) {
      float z0, z1;
      fb_dither2(dk.k0, dk.k1, dk.epoch, dk.utt0, (unsigned)f, (unsigned)(s >> 2), (s >> 1) & 1, z0, z1);
      double x = (double)wav[wb_reflect(start + s, n)];
      x += dk.amp * (double)((s & 1) ? z1 : z0);
      xs[s] = x;
      v += x;
    }
  } else {
    for (int s = threadIdx.x; s < L; s += 256) { xs[s] = (double)wav[wb_reflect(start + s, n)]; v += xs[s]; }
  }
  if (fe.remove_dc) {
    const double mean = wb_block_sum(v, red) / (double)L;
    for (int s = threadIdx.x; s < L; s += 256) xs[s] -= mean;
  }
  __syncthreads();
  double E = 0.0;
  if (fe.raw_energy) {
    v = 0.0;
    for (int s = threadIdx.x; s < L; s += 256) v += xs[s] * xs[s];
    E = wb_block_sum(v, red);
  }
  for (int s = threadIdx.x; s < P; s += 256) {
    double y = 0.0;
    if (s < L) y = (xs[s] - fe.preemph * xs[s > 0 ? s - 1 : 0]) * fe.window[s];
    re[s] = y; im[s] = 0.0;
    aux[s] = y;   // the windowed frame, kept for the energy of raw_energy = 0
  }
  if (!fe.raw_energy) {
    __syncthreads();
    v = 0.0;
    for (int s = threadIdx.x; s < L; s += 256) v += aux[s] * aux[s];
    E = wb_block_sum(v, red);
  }
  wb_fft(re, im, P, fe.tw_full, false);
  // ---- cepstra -> log mel -> mel energies
  double dlogE = 0.0;
  for (int k = threadIdx.x; k < nc; k += 256) s_dc[k] = (k == 0 && fe.use_energy) ? 0.0 : dmf[(size_t)f * nc + k] * fe.lifter[k];
  if (fe.use_energy) {
    const double le = log(E > eps ? E : eps);
    if (E >= eps && le >= fe.log_energy_floor) dlogE = dmf[(size_t)f * nc];
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += 256) {
    double e = 0.0;
    const double *wm = fe.mel_w + fe.mel_off[b];
    const int first = fe.mel_first[b];
    for (int i = 0; i < fe.mel_len[b]; ++i) e += wm[i] * (re[first + i] * re[first + i] + im[first + i] * im[first + i]);
    double dl = 0.0;
    for (int k = 0; k < nc; ++k) dl += fe.dct[(size_t)k * nb + b] * s_dc[k];
    s_de[b] = e >= eps ? dl / e : 0.0;
  }
  __syncthreads();
  // ---- power spectrum: Z_k = dP_k F_k on the nfft bins the mel bank reads, then dy_s = 2 Re sum_k Z_k exp(+2 pi i k s / P)
  for (int i = threadIdx.x; i < P; i += 256) {
    double dp = 0.0;
    if (i < nfft)
      for (int b = 0; b < nb; ++b) {
        const int o = i - fe.mel_first[b];
        if (o >= 0 && o < fe.mel_len[b]) dp += fe.mel_w[fe.mel_off[b] + o] * s_de[b];
      }
    re[i] *= dp; im[i] *= dp;
  }
  wb_fft(re, im, P, fe.tw_full, true);
  // ---- window, pre-emphasis, energy, DC
  const double ge = (dlogE != 0.0) ? 2.0 * dlogE / E : 0.0;
  for (int s = threadIdx.x; s < L; s += 256) {
    double dy = 2.0 * re[s];
    if (!fe.raw_energy) dy += ge * aux[s];
    im[s] = dy * fe.window[s];   // dz
  }
  __syncthreads();
  v = 0.0;
  for (int s = threadIdx.x; s < L; s += 256) {
    double dx = im[s] - (s + 1 < L ? fe.preemph * im[s + 1] : 0.0);
    if (s == 0) dx -= fe.preemph * im[0];
    if (fe.raw_energy) dx += ge * xs[s];
    re[s] = dx;
    v += dx;
  }
  double mean = 0.0;
  if (fe.remove_dc) mean = wb_block_sum(v, red) / (double)L;
  for (int s = threadIdx.x; s < L; s += 256) dxf[(size_t)f * L + s] = re[s] - mean;
}

// grad[i] = scale * sum over the frames f ascending, positions s ascending with index(f, s) == i, of dxf[f][s]
__global__ __launch_bounds__(256) void k_wb_overlap_add(FbFrontendDev fe, int T, int64_t n, const double *__restrict__ dxf,
                                                        double scale, double *__restrict__ grad, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int L = fe.L;
  double acc = 0.0;
  // frames that reach outside [0, n) fold back onto the L samples next to an edge (anywhere when n < L)
  const bool near_edge = n < L || i < L || i >= n - L;
  for (int f = 0; f < T; ++f) {
    const int64_t start = wb_frame_start(fe, f);
    if (start >= 0 && start + L <= n) {
      if (i >= start && i < start + L) acc += dxf[(size_t)f * L + (i - start)];
    } else if (near_edge) {
      for (int s = 0; s < L; ++s)
        if (wb_reflect(start + s, n) == i) acc += dxf[(size_t)f * L + s];
    }
  }
  grad[i] = scale * acc;
}

void fb_launch_wb_frontend_vjp(hipStream_t s, const FbFrontendDev &fe, const int16_t *wav, int64_t n, int T, const float *mfcc,
                               const double *cot, const int *tv_fwd, int *rank, double *dcm, double *ddf, double *dmf, double *dxf,
                               double scale, double *grad, int *status, const int *stop, const FbDitherKey *dk) {
  const FbDitherKey dkv = (dk && dk->amp > 0.0) ? *dk : FbDitherKey{};
  hipLaunchKernelGGL(k_wb_vad_scatter, dim3(1), dim3(256), 0, s, fe, mfcc, T, cot, tv_fwd, rank, dcm, status, stop);
  hipLaunchKernelGGL(k_wb_cmvn_t, dim3((unsigned)((T * fe.dim + 255) / 256)), dim3(256), 0, s, T, fe.dim, fe.cmn_window, dcm, ddf, stop);
  hipLaunchKernelGGL(k_wb_delta_t, dim3((unsigned)((T * fe.nc + 255) / 256)), dim3(256), 0, s, fe, T, ddf, dmf, stop);
  hipLaunchKernelGGL(k_wb_mfcc_t, dim3((unsigned)T), dim3(256), 0, s, fe, wav, n, dmf, dxf, stop, dkv);
  hipLaunchKernelGGL(k_wb_overlap_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fe, T, n, dxf, scale, grad, stop);
}

// ------------------------------------------------------------------------------------------------ update
// FAKEBOB.py:193-203 on the gradient g: grad_m = momentum grad_m + (1 - momentum) g; adver -= lr sign(grad_m); clip to the
// epsilon ball and to [-1, 1] -- the float64 operations of fb_update_perturb_body, one rounding each
__global__ __launch_bounds__(256) void k_wb_update(const double *__restrict__ g, int64_t N, double momentum, double one_minus_m,
                                                   double epsilon, const double *__restrict__ audio, double *__restrict__ grad_m,
                                                   double *__restrict__ adver, const FbCtlDev *__restrict__ ctl) {
  if (ctl->stop) return;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double lr = ctl->lr;
  const double gm = __dadd_rn(__dmul_rn(momentum, grad_m[n]), __dmul_rn(one_minus_m, g[n]));
  grad_m[n] = gm;
  const double sg = gm > 0.0 ? 1.0 : (gm < 0.0 ? -1.0 : gm);  // np.sign (0 -> 0, nan -> nan)
  double a = __dsub_rn(adver[n], __dmul_rn(lr, sg));
  const double au = audio[n];
  double lo = __dsub_rn(au, epsilon), hi = __dadd_rn(au, epsilon);
  lo = lo < -1.0 ? -1.0 : (lo > 1.0 ? 1.0 : lo);
  hi = hi < -1.0 ? -1.0 : (hi > 1.0 ? 1.0 : hi);
  a = a < lo ? lo : a;
  a = a > hi ? hi : a;
  adver[n] = a;
}

void fb_launch_wb_update(hipStream_t s, const double *g, int64_t N, double momentum, double one_minus_m, double epsilon,
                         const double *audio, double *grad_m, double *adver, const FbCtlDev *ctl) {
  hipLaunchKernelGGL(k_wb_update, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, g, N, momentum, one_minus_m, epsilon, audio,
                     grad_m, adver, ctl);
}
