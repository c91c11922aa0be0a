// whitebox_iv_kernels.hip -- the analytic gradient of the i-vector-PLDA victim's back end (fb_set_wb_ivector; the "white-box
// gradients" contract of include/fakebob_hip.h, i-vector case), gfx950.  Everything is float64.
//
//   k_wb_iv_ctl        loss weights w[S] = d loss / d raw[s] (every task z-normalises) and the attack's loop control
//   k_wb_iv_backend_t  wbar[R] = d (sum_s w_s LLR_s) / d ivec: the back end's forward recomputed in LDS, then backwards through
//                      the LLR, the two length normalisations, the PLDA transform and the LDA
//   (the adjoint solve lambda = quad^-1 wbar is the forward's own k_iv_solve_ll on a copy of the forward's matrix)
//   k_wb_iv_stats_t    the hot path: one stream over the rows of U and Sigma^-1 M of the active components,
//                        Fbar_k[d] = sum_r (Sigma^-1 M)_k[d][r] lambda_r,   npart[chunk][k] = sum_{e in chunk} U_k[e] Sym[e],
//                      Sym = the packed image of (lambda w' + w lambda') / (1 + delta_ij), built once per workgroup in LDS
//   k_wb_iv_nbar       Nbar_k = - sum over the chunks of npart, chunks ascending
//   k_wb_iv_post_t     wave = voiced frame: gammabar, the soft-max transpose on the kept slots, row t of the cotangent
// No floating-point atomics: every output element has one owner and every sum a fixed order.
#include <math.h>

#include "fb_device.h"
#include "fb_kernels.h"
#include "whitebox_device.h"

// ------------------------------------------------------------------------------------------------ weights + loop control
// One thread.  The weights are whitebox_device.h's fb_wb_iv_weights (the 1 / z_std inside, first-maximum index).
__global__ __launch_bounds__(64) void k_wb_iv_ctl(const double *__restrict__ scores, const FbNesDev *__restrict__ out, int S, int task,
                                                  int attack_type, const double *__restrict__ z_std, double threshold, int target,
                                                  int true_label, double *__restrict__ w, FbCtlDev *__restrict__ ctl,
                                                  double *__restrict__ trace, int it) {
  if (threadIdx.x != 0) return;
  if (ctl && ctl->stop) return;
  fb_wb_iv_weights(scores, S, task, attack_type, z_std, threshold, target, true_label, w);
  // (fb_wb_loop_control counts M - 1 scores outside CSI: hand it the M that gives S)
  if (ctl) fb_wb_loop_control(scores, out, task == FB_TASK_CSI ? S : S + 1, task, ctl, trace, it);
}

void fb_launch_wb_iv_ctl(hipStream_t s, const double *scores, const FbNesDev *out, int S, int task, int attack_type,
                         const double *z_std, double threshold, int target, int true_label, double *w, FbCtlDev *ctl, double *trace,
                         int it) {
  hipLaunchKernelGGL(k_wb_iv_ctl, dim3(1), dim3(64), 0, s, scores, out, S, task, attack_type, z_std, threshold, target, true_label, w,
                     ctl, trace, it);
}

// ------------------------------------------------------------------------------------------------ back end, transposed
#define FB_WBIV_BT 512
__device__ __forceinline__ double wbiv_block_sum(double v, double *red) {
  v = fb_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += red[i];
  return r;
}
// LDS (doubles): x[R] z0[L] z[L] y0[L] gy[L] gz[L] red[16] part[4][L].  The forward is fb_iv_backend_body's (fb_iv_tail.h): the
// i-vector through float32, - mean.vec, LDA (+ offset column), * sqrt(L) / |.|, - plda mean, PLDA transform,
// * sqrt(L / sum y0^2 / (psi + 1)), LLR with n = 1.  A zero LDA output (ratio == 0: the forward leaves the vector as it is)
// gets the identity for that normalisation.  The two forward mat-vecs are split four ways along the contraction index
// (share = tid / 128: four chains of R / 4 coalesced loads instead of one of R), the shares added in fixed order.
__host__ __device__ __forceinline__ size_t wbiv_backend_doubles(int R, int L) { return (size_t)R + 9 * (size_t)L + 16; }
__global__ __launch_bounds__(FB_WBIV_BT) void k_wb_iv_backend_t(FbIvDev iv, const double *__restrict__ ivec, const double *__restrict__ w,
                                                                double *__restrict__ wbar, const int *__restrict__ stop) {
  if (stop && *stop) return;
  extern __shared__ __attribute__((aligned(16))) double wbiv_sm[];
  const int R = iv.R, L = iv.L, S = iv.S, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = FB_WBIV_BT / 64;
  double *x = wbiv_sm, *z0 = x + R, *z = z0 + L, *y0 = z + L, *gy = y0 + L, *gz = gy + L, *red = gz + L, *part = red + 16;
  const int sh = tid >> 7, st = tid & 127;   // share of the contraction index, thread within the share
  for (int r = tid; r < R; r += FB_WBIV_BT) x[r] = (double)(float)ivec[r] - iv.mean_vec[r];
  __syncthreads();
  {
    const int r0 = (int)((long long)R * sh / 4), r1 = (int)((long long)R * (sh + 1) / 4);
    for (int l = st; l < L; l += 128) {
      double acc = (sh == 0 && iv.lda_cols == R + 1) ? iv.ldaT[(size_t)R * L + l] : 0.0;
#pragma unroll 10
      for (int r = r0; r < r1; ++r) acc = fma(iv.ldaT[(size_t)r * L + l], x[r], acc);
      part[sh * L + l] = acc;
    }
  }
  __syncthreads();
  double nrm2 = 0.0;
  for (int l = tid; l < L; l += FB_WBIV_BT) {
    const double acc = ((part[l] + part[L + l]) + part[2 * L + l]) + part[3 * L + l];
    z0[l] = acc;
    nrm2 = fma(acc, acc, nrm2);
  }
  nrm2 = wbiv_block_sum(nrm2, red);
  const double nrm = sqrt(nrm2), sqL = sqrt((double)L);
  const double a1 = nrm != 0.0 ? sqL / nrm : 1.0;   // z1 = a1 z0
  __syncthreads();
  for (int l = tid; l < L; l += FB_WBIV_BT) z[l] = a1 * z0[l] - iv.plda_mean[l];
  __syncthreads();
  {
    const int m0 = (int)((long long)L * sh / 4), m1 = (int)((long long)L * (sh + 1) / 4);
    for (int l = st; l < L; l += 128) {
      double acc = 0.0;
#pragma unroll 10
      for (int m = m0; m < m1; ++m) acc = fma(iv.pldaT[(size_t)m * L + l], z[m], acc);
      part[sh * L + l] = acc;
    }
  }
  __syncthreads();
  double dot = 0.0;
  for (int l = tid; l < L; l += FB_WBIV_BT) {
    const double acc = ((part[l] + part[L + l]) + part[2 * L + l]) + part[3 * L + l];
    y0[l] = acc;
    dot += acc * acc / (iv.plda_psi[l] + 1.0);
  }
  dot = wbiv_block_sum(dot, red);
  const double nf = sqrt((double)L / dot);
  // gy[l] = sum_s w_s d LLR_s / d y_l,  LLR_s = -1/2 sum_l [(y_l - mean_sl)^2 / var_l - y_l^2 / (psi_l + 1)] + const
  double gdot = 0.0;   // sum_l gy_l y0_l
  for (int l = tid; l < L; l += FB_WBIV_BT) {
    const double psi = iv.plda_psi[l], yl = nf * y0[l];
    const double var = 1.0 + psi / (psi + 1.0);
    double g = 0.0;
    for (int s = 0; s < S; ++s) {
      const double ws = w[s];
      if (ws != 0.0) g += ws * (yl / (psi + 1.0) - (yl - psi / (psi + 1.0) * iv.train[(size_t)s * L + l]) / var);
    }
    gy[l] = g;
    gdot = fma(g, y0[l], gdot);
  }
  gdot = wbiv_block_sum(gdot, red);
  __syncthreads();
  // y = nf y0, nf = sqrt(L / dot):  gy0_l = nf (gy_l - gdot / dot * y0_l / (psi_l + 1))
  for (int l = tid; l < L; l += FB_WBIV_BT) gy[l] = nf * (gy[l] - gdot / dot * y0[l] / (iv.plda_psi[l] + 1.0));
  __syncthreads();
  // gz_m = sum_l pldaT[m][l] gy0_l: wave = row m (contiguous), lanes over l
  for (int m = wv; m < L; m += NW) {
    double acc = 0.0;
    for (int l = lane; l < L; l += 64) acc = fma(iv.pldaT[(size_t)m * L + l], gy[l], acc);
    acc = fb_wave_sum(acc);
    if (lane == 0) gz[m] = acc;
  }
  __syncthreads();
  // z1 = sqrt(L) z0 / |z0|:  gz0_l = a1 (gz_l - z0_l <gz, z0> / |z0|^2)
  double zd = 0.0;
  for (int l = tid; l < L; l += FB_WBIV_BT) zd = fma(gz[l], z0[l], zd);
  zd = wbiv_block_sum(zd, red);
  __syncthreads();
  for (int l = tid; l < L; l += FB_WBIV_BT) gz[l] = nrm != 0.0 ? a1 * (gz[l] - z0[l] * zd / nrm2) : gz[l];
  __syncthreads();
  for (int r = wv; r < R; r += NW) {
    double acc = 0.0;
    for (int l = lane; l < L; l += 64) acc = fma(iv.ldaT[(size_t)r * L + l], gz[l], acc);
    acc = fb_wave_sum(acc);
    if (lane == 0) wbar[r] = acc;
  }
}
void fb_launch_wb_iv_backend_t(hipStream_t s, const FbIvDev &iv, const double *ivec, const double *w, double *wbar, const int *stop) {
  hipLaunchKernelGGL(k_wb_iv_backend_t, dim3(1), dim3(FB_WBIV_BT), sizeof(double) * wbiv_backend_doubles(iv.R, iv.L), s, iv, ivec, w,
                     wbar, stop);
}

// ------------------------------------------------------------------------------------------------ the parameter stream
// quad = I + sum_k N_k U_k, lin = sum_k A_k' F_k, w = quad^-1 lin.  With lambda = quad^-1 wbar:
//   Fbar_k = A_k lambda                         (A_k = (Sigma^-1 M)_k, [D][R] row-major)
//   Nbar_k = - lambda' U_k w = - sum_{i >= j} U_k[i][j] Sym[i][j],  Sym[i][j] = lambda_i w_j + lambda_j w_i (i > j), lambda_i w_i (i = j)
// (U packed lower-triangular: an off-diagonal element stands for two of the full matrix, the diagonal for one).
// Grid (x, y): x < n_uc -- chunk x of FB_WBIV_CH packed elements of U: the workgroup builds Sym for its chunk in LDS once, then
// every wave streams that chunk of the components kk = 4 y + wave, + 4 gridDim.y, ... of the active list (64 lanes x 16 bytes
// per request, 16 requests in flight) and leaves one partial; x >= n_uc -- rows of Sigma^-1 M: wave = (component, d), lambda in
// registers.  One launch, every byte of both tables of an active component read once.
#define FB_WBIV_CH 2048     // packed elements of U per chunk (16 KB of LDS)
#define FB_WBIV_FX 24       // workgroup columns of the Sigma^-1 M part
int fb_wb_iv_uchunks(const FbIvDev &iv) { return (iv.triR + FB_WBIV_CH - 1) / FB_WBIV_CH; }
static int wbiv_stats_gy(const FbIvDev &iv) {
  const int g = (iv.C + 3) / 4;
  // (measured at the recipe's size, 143 active components: 32 rows of workgroups 36 us, 8 rows -- every Sym chunk serving four
  //  times as many components -- 85 us: the stream wants the requests of many waves in flight more than it minds the rebuilds)
  return g < 1 ? 1 : (g > 32 ? 32 : g);
}
__global__ __launch_bounds__(256) void k_wb_iv_stats_t(FbIvDev iv, const int *__restrict__ active, const double *__restrict__ lam,
                                                       const double *__restrict__ ivec, int n_uc, double *__restrict__ fbar,
                                                       double *__restrict__ npart, const int *__restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __attribute__((aligned(16))) double sym[FB_WBIV_CH];
  const int R = iv.R, D = iv.D, triR = iv.triR, C = iv.C;
  const int n_active = min(active[C], C);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if ((int)blockIdx.x < n_uc) {
    if ((int)blockIdx.y * 4 >= n_active) return;
    const int e0 = blockIdx.x * FB_WBIV_CH, e1 = min(e0 + FB_WBIV_CH, triR);
    for (int e = e0 + tid; e < e0 + FB_WBIV_CH; e += 256) {
      double v = 0.0;
      if (e < e1) {
        int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        while (i * (i + 1) / 2 > e) --i;
        const int j = e - i * (i + 1) / 2;
        // (w = the i-vector with the prior offset back in element 0)
        const double wi = ivec[i] + (i == 0 ? iv.prior_offset : 0.0), wj = ivec[j] + (j == 0 ? iv.prior_offset : 0.0);
        v = i == j ? lam[i] * wi : fma(lam[i], wj, lam[j] * wi);
      }
      sym[e - e0] = v;   // (zeros behind the end of the triangle)
    }
    __syncthreads();
    const bool vec = (triR & 1) == 0;   // every component's chunk starts on 16 bytes
    for (int kk = blockIdx.y * 4 + wv; kk < n_active; kk += 4 * gridDim.y) {
      const int k = active[kk];
      const double *u = iv.u + (size_t)k * triR + e0;
      double acc0 = 0.0, acc1 = 0.0;
      if (vec && e0 + FB_WBIV_CH <= triR) {
        const double2 *u2 = reinterpret_cast<const double2 *>(u);
        const double2 *s2 = reinterpret_cast<const double2 *>(sym);
#pragma unroll
        for (int q = 0; q < FB_WBIV_CH / 128; ++q) {
          const double2 a = u2[q * 64 + lane], b = s2[q * 64 + lane];
          acc0 = fma(a.x, b.x, acc0);
          acc1 = fma(a.y, b.y, acc1);
        }
      } else if (vec) {
        const double2 *u2 = reinterpret_cast<const double2 *>(u);
        const double2 *s2 = reinterpret_cast<const double2 *>(sym);
        const int n2 = (e1 - e0) >> 1;   // (triR even and e0 even: the tail is whole pairs)
        for (int q = lane; q < n2; q += 64) {
          const double2 a = u2[q], b = s2[q];
          acc0 = fma(a.x, b.x, acc0);
          acc1 = fma(a.y, b.y, acc1);
        }
      } else {
        for (int q = lane; q < e1 - e0; q += 64) acc0 = fma(u[q], sym[q], acc0);
      }
      const double sum = fb_wave_sum(acc0 + acc1);
      if (lane == 0) npart[(size_t)blockIdx.x * C + kk] = sum;
    }
  } else {
    const int fx = blockIdx.x - n_uc;
    // lambda: lane holds elements 2 (lane + 64 q), + 1 of it (R <= 512: four pairs)
    double l0[4], l1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 2 * (lane + 64 * q);
      l0[q] = r < R ? lam[r] : 0.0;
      l1[q] = r + 1 < R ? lam[r + 1] : 0.0;
    }
    const bool vec = (R & 1) == 0;   // every row starts on 16 bytes
    const long long n_task = (long long)n_active * D;
    const long long stride = 4LL * FB_WBIV_FX * gridDim.y;
    for (long long t = ((long long)blockIdx.y * FB_WBIV_FX + fx) * 4 + wv; t < n_task; t += stride) {
      const int kk = (int)(t / D), d = (int)(t - (long long)kk * D);
      const int k = active[kk];
      const double *a = iv.sim + ((size_t)k * D + d) * R;
      double acc0 = 0.0, acc1 = 0.0;
      if (vec) {
        const double2 *a2 = reinterpret_cast<const double2 *>(a);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = lane + 64 * q;
          if (2 * p < R) {
            const double2 v = a2[p];
            acc0 = fma(v.x, l0[q], acc0);
            acc1 = fma(v.y, l1[q], acc1);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 2 * (lane + 64 * q);
          if (r < R) acc0 = fma(a[r], l0[q], acc0);
          if (r + 1 < R) acc1 = fma(a[r + 1], l1[q], acc1);
        }
      }
      const double sum = fb_wave_sum(acc0 + acc1);
      if (lane == 0) fbar[(size_t)k * D + d] = sum;
    }
  }
}
// Nbar[k] = - sum_chunks npart[chunk][kk] for the active components, chunks ascending
__global__ __launch_bounds__(256) void k_wb_iv_nbar(int C, const int *__restrict__ active, int n_uc, const double *__restrict__ npart,
                                                    double *__restrict__ nbar, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int n_active = min(active[C], C);
  const int kk = blockIdx.x * 256 + threadIdx.x;
  if (kk >= n_active) return;
  double acc = 0.0;
  for (int c = 0; c < n_uc; ++c) acc += npart[(size_t)c * C + kk];
  nbar[active[kk]] = -acc;
}
void fb_launch_wb_iv_stats_t(hipStream_t s, const FbIvDev &iv, const int *active, const double *lam, const double *ivec, double *fbar,
                             double *npart, double *nbar, const int *stop) {
  const int n_uc = fb_wb_iv_uchunks(iv);
  hipLaunchKernelGGL(k_wb_iv_stats_t, dim3(n_uc + FB_WBIV_FX, wbiv_stats_gy(iv)), dim3(256), 0, s, iv, active, lam, ivec, n_uc, fbar,
                     npart, stop);
  hipLaunchKernelGGL(k_wb_iv_nbar, dim3((iv.C + 255) / 256), dim3(256), 0, s, iv.C, active, n_uc, npart, nbar, stop);
}

// ------------------------------------------------------------------------------------------------ posteriors, transposed
// wave = voiced row t.  gamma_s = post[t][s] (0: not kept -- the slot is skipped, whatever Fbar / Nbar hold for its component),
//   gammabar_s = Nbar_k + Fbar_k . x_t                                    (lane = slot)
//   llbar_s    = gamma_s (gammabar_s - sum_j gamma_j gammabar_j)          (the soft-max on the kept set; one kept slot: 0)
//   xbar_t[d]  = sum_s gamma_s Fbar_k[d] + llbar_s (mic_k[d] - (P_k x_t)[d])   (lane = dimension d, and d + 64)
// P_k: the packed float32 inv_covars the forward's kernels read (row-major lower triangle), mic_k the means_invcovars.
__global__ __launch_bounds__(256) void k_wb_iv_post_t(FbIvDev iv, const float *__restrict__ feats, const int *__restrict__ n_rows_ptr,
                                                      int rows_cap, const int *__restrict__ sel, const float *__restrict__ post,
                                                      const double *__restrict__ fbar, const double *__restrict__ nbar,
                                                      double *__restrict__ g, const int *__restrict__ stop,
                                                      const int *__restrict__ row_base_ptr) {
  if (stop && *stop) return;
  __shared__ double xs[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int out_row = blockIdx.x * 4 + wv;
  const int n_rows = min(*n_rows_ptr, rows_cap);
  if (out_row >= n_rows) return;   // (wave-uniform; no workgroup barrier below)
  // (row_base_ptr: the rows are a replica's within the batch -- feats / sel / post are read from there, g is the replica's own)
  const int row = out_row + (row_base_ptr ? *row_base_ptr : 0);
  const int D = iv.D, nsel = iv.nsel, triD = iv.triD;
  double *x = xs[wv];
  for (int d = lane; d < 128; d += 64) x[d] = d < D ? (double)feats[(size_t)row * D + d] : 0.0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int k = -1;
  double gam = 0.0;
  if (lane < nsel) {
    k = sel[(size_t)row * nsel + lane];
    gam = (double)post[(size_t)row * nsel + lane];
    if (k < 0 || k >= iv.C) gam = 0.0;
  }
  double gb = 0.0;
  if (gam != 0.0) {
    const double *fk = fbar + (size_t)k * D;
    double acc = nbar[k];
    for (int d = 0; d < D; ++d) acc = fma(fk[d], x[d], acc);
    gb = acc;
  }
  const double mean = fb_wave_sum(gam * gb);
  const double llb = gam * (gb - mean);
  const int d0 = lane, d1 = lane + 64;
  const bool two = d1 < D;
  double o0 = 0.0, o1 = 0.0;
  for (int s = 0; s < nsel; ++s) {
    const double gs = __shfl(gam, s, 64);
    if (gs == 0.0) continue;   // wave-uniform
    const int ks = __shfl(k, s, 64);
    const double ls = __shfl(llb, s, 64);
    const double *fk = fbar + (size_t)ks * D;
    const float *P = iv.fg_P + (size_t)ks * triD, *mic = iv.fg_mic + (size_t)ks * D;
    if (d0 < D) o0 = fma(gs, fk[d0], o0);
    if (two) o1 = fma(gs, fk[d1], o1);
    if (ls != 0.0) {
      double p0 = 0.0, p1 = 0.0;
      if (d0 < D) {
        const float *pr = P + (size_t)d0 * (d0 + 1) / 2;
        for (int e = 0; e <= d0; ++e) p0 = fma((double)pr[e], x[e], p0);
        for (int e = d0 + 1; e < D; ++e) p0 = fma((double)P[(size_t)e * (e + 1) / 2 + d0], x[e], p0);
        o0 = fma(ls, (double)mic[d0] - p0, o0);
      }
      if (two) {
        const float *pr = P + (size_t)d1 * (d1 + 1) / 2;
        for (int e = 0; e <= d1; ++e) p1 = fma((double)pr[e], x[e], p1);
        for (int e = d1 + 1; e < D; ++e) p1 = fma((double)P[(size_t)e * (e + 1) / 2 + d1], x[e], p1);
        o1 = fma(ls, (double)mic[d1] - p1, o1);
      }
    }
  }
  if (d0 < D) g[(size_t)out_row * D + d0] = o0;
  if (two) g[(size_t)out_row * D + d1] = o1;
}
void fb_launch_wb_iv_post_t(hipStream_t s, const FbIvDev &iv, const float *feats, const int *n_rows_ptr, int rows_cap, const int *sel,
                            const float *post, const double *fbar, const double *nbar, double *g, const int *stop,
                            const int *row_base_ptr) {
  if (rows_cap <= 0) return;
  hipLaunchKernelGGL(k_wb_iv_post_t, dim3((rows_cap + 3) / 4), dim3(256), 0, s, iv, feats, n_rows_ptr, rows_cap, sel, post, fbar, nbar,
                     g, stop, row_base_ptr);
}
