// whitebox_bpda_kernels.hip -- the transposes of the defence stages for white-box gradients through a defended victim
// (fb_set_wb_bpda; the "white-box gradients" contract of include/fakebob_hip.h), gfx950.
//
//   k_wb_ctl_rep   replica j's loss weights w_j[M] / r from ITS scores (k_loss_eot's per-replica rows); replica 0's launch also
//                  runs the attack's loop control on the EOT mean the loss launch left
//   k_wb_chain_t   the input-transform chain transposed for one replica: the vector-Jacobian product of a float64 cotangent
//                  on the chain's output (the codec behind the chain is the identity: BPDA) with the surrogate derivative of
//                  every stage, and the accumulation of the replicas' gradients in ascending order
//
// k_wb_chain_t.  One workgroup per tile of FB_WBT_TILE samples of dx; the launch is one replica.  The forward keeps no
// intermediates, so the workgroup reruns the chain forward in LDS -- the arithmetic of k_input_transform, stage by stage, from
// input_transform_device.h, the noise stages redrawn from the absolute sample index -- and keeps one byte per (stage, sample):
// the saturation bit of a QUANT / FIR / NOISE stage, the window position a MEDIAN stage selected.  Then the stages run in
// reverse on a float64 cotangent tile.  With H the sum of the radii:
//   dx on the tile [t0, t0 + TILE)  needs  the cotangent of the chain's output on [t0 - H, t0 + TILE + H)        (Wc = TILE + 2 H)
//   the bytes of the LAST stage on that region  need  the chain's input on [t0 - 2 H, t0 + TILE + 2 H)            (Wf = TILE + 4 H)
// -- a transposed FIR reads dy from where the forward wrote, so the cotangent's halo is the sum of the radii on the other
// side.  LDS: 2 Wc float64 (cotangent, two buffers) + 2 (Wf + 4) int16 (forward, two buffers) + n Wf bytes.  The worst chain
// the contract allows (n = 8, H = 1024) at TILE = 2048: 65536 + 24592 + 49152 = 139280 bytes of the compute unit's 163840;
// TILE = 4096, the forward's, would need 212992.  A radius-0 chain of two stages takes 45 KB.  
// A lane owns samples of dx and gathers: no atomics, every sum in a fixed order (FIR: taps ascending; MEDIAN: outputs
// ascending).  Nothing is exchanged between workgroups.
#include <math.h>

#include "fb_device.h"
#include "fb_kernels.h"
#include "input_transform_device.h"
#include "whitebox_device.h"

#define WBT_THREADS 256
#define WBT_PAD 4

// ------------------------------------------------------------------------------------------------ weights per replica
// One thread.  rep_scores[S]: replica j's system scores (k_loss_eot's rep_sc row); w = w_j / r.  Replica 0's launch (do_ctl)
// then runs k_wb_ctl's loop control on `out` and the mean scores -- what k_loss_eot averaged over the replicas.
__global__ __launch_bounds__(64) void k_wb_ctl_rep(const double *__restrict__ rep_scores, const double *__restrict__ mean_scores,
                                                   const FbNesDev *__restrict__ out, int M, int r, int task, int attack_type,
                                                   const double *__restrict__ z_std, double threshold, int target, int true_label,
                                                   double *__restrict__ w, FbCtlDev *__restrict__ ctl, int do_ctl,
                                                   double *__restrict__ trace, int it) {
  if (threadIdx.x != 0) return;
  if (ctl && ctl->stop) return;
  fb_wb_weights(rep_scores, M, task, attack_type, z_std, threshold, target, true_label, w);
  if (r > 1) {
    const double inv = 1.0 / (double)r;
    for (int m = 0; m < M; ++m) w[m] *= inv;
  }
  if (ctl && do_ctl) fb_wb_loop_control(mean_scores, out, M, task, ctl, trace, it);
}

void fb_launch_wb_ctl_rep(hipStream_t s, const double *rep_scores, const double *mean_scores, const FbNesDev *out, int M, int r,
                          int task, int attack_type, const double *z_std, double threshold, int target, int true_label, double *w,
                          FbCtlDev *ctl, int do_ctl, double *trace, int it) {
  hipLaunchKernelGGL(k_wb_ctl_rep, dim3(1), dim3(64), 0, s, rep_scores, mean_scores, out, M, r, task, attack_type, z_std, threshold,
                     target, true_label, w, ctl, do_ctl, trace, it);
}

// ------------------------------------------------------------------------------------------------ the chain, transposed
// FB_TF_MEDIAN with the position: the element of rank (k - 1) / 2 of w0[0 .. k) under the strict order (value, position), as
// tf_median counts it; *sel = its position in the window
template <int KMAX>
static __device__ __forceinline__ int wbt_median_sel(const int16_t *w0, int k, int *sel) {
  int w[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) w[j] = j < k ? (int)w0[j] : 0x10000;
  const int r = (k - 1) >> 1;
  int med = 0, at = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    int rank = 0;
#pragma unroll
    for (int m = 0; m < KMAX; ++m)
      if (m != j) rank += (m < j) ? (w[m] <= w[j]) : (w[m] < w[j]);
    if (rank == r) { med = w[j]; at = j; }
  }
  *sel = at;
  return med;
}

#define WBT_NONE 0xFF  // a byte no window position equals: outside the utterance

__global__ __launch_bounds__(WBT_THREADS) void k_wb_chain_t(FbTfChain ch, const double *__restrict__ taps,
                                                            const int16_t *__restrict__ wav, int64_t n, FbTfRnd rn, int replica,
                                                            const double *__restrict__ cot, double *__restrict__ grad,
                                                            int accumulate, const int *__restrict__ stop) {
  if (stop && *stop) return;
  extern __shared__ double wbt_lds[];
  const int64_t t0 = (int64_t)blockIdx.x * FB_WBT_TILE;
  if (t0 >= n) return;
  const int H = ch.H, Wc = FB_WBT_TILE + 2 * H, Wf = FB_WBT_TILE + 4 * H;
  double *ca = wbt_lds, *cb = wbt_lds + Wc;
  int16_t *a = reinterpret_cast<int16_t *>(wbt_lds + 2 * Wc), *b = a + Wf + WBT_PAD;
  unsigned char *aux = reinterpret_cast<unsigned char *>(b + Wf + WBT_PAD);
  const int tid = threadIdx.x;
  // forward position p <-> sample g0 + p; cotangent position pc <-> sample c0 + pc = g0 + H + pc
  const int64_t g0 = t0 - 2 * H, c0 = t0 - H;
  for (int p = tid; p < Wf; p += WBT_THREADS) {
    const int64_t i = g0 + p;
    a[p] = (i >= 0 && i < n) ? wav[i] : (int16_t)0;
  }
  for (int pc = tid; pc < Wc; pc += WBT_THREADS) {
    const int64_t i = c0 + pc;
    ca[pc] = (i >= 0 && i < n) ? cot[i] : 0.0;
  }
  __syncthreads();
  // ---- the chain forward, as k_input_transform runs it, keeping one byte per (stage, sample)
  int lo = 0, hi = Wf;
  for (int s = 0; s < ch.n; ++s) {
    const int kind = ch.kind[s], k = ch.k[s];
    unsigned char *ax = aux + (size_t)s * Wf;
    if (kind == FB_TF_NOISE) {
      const double sc = tf_noise_scale(k, taps[ch.tap_off[s]], k ? rn.power[0] : 0ull, n);
      const int64_t i_first = ((g0 + lo) >> 2) << 2;
      for (int64_t i4 = i_first + 4 * tid; i4 < g0 + hi; i4 += 4 * WBT_THREADS) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (i4 + 3 >= 0 && i4 < n) tf_noise4(rn, 0u, s, replica, (uint32_t)(i4 >> 2), z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t i = i4 + q;
          const int p = (int)(i - g0);
          if (p >= lo && p < hi) {
            int y = 0;
            unsigned char sat = 1;
            if (i >= 0 && i < n) {
              const double v = rint(__dadd_rn((double)a[p], __dmul_rn(sc, (double)z[q])));
              sat = (v < -32768.0 || v > 32767.0) ? 1 : 0;
              y = (int)fmin(fmax(v, -32768.0), 32767.0);
            }
            b[p] = (int16_t)y;
            ax[p] = sat;
          }
        }
      }
    } else if (kind == FB_TF_FIR) {
      const int c = (k - 1) >> 1;
      const double *__restrict__ h = taps + ch.tap_off[s];
      lo += c;
      hi -= c;
      for (int p = lo + tid; p < hi; p += WBT_THREADS) {
        const int64_t i = g0 + p;
        int y = 0;
        unsigned char sat = 1;
        if (i >= 0 && i < n) {
          double acc = 0.0;
          for (int j = 0; j < k; ++j) acc = __dadd_rn(acc, __dmul_rn(h[j], (double)a[p + c - j]));
          const double v = rint(acc);
          sat = (v < -32768.0 || v > 32767.0) ? 1 : 0;
          y = (int)fmin(fmax(v, -32768.0), 32767.0);
        }
        b[p] = (int16_t)y;
        ax[p] = sat;
      }
    } else if (kind == FB_TF_MEDIAN) {
      const int r = (k - 1) >> 1;
      lo += r;
      hi -= r;
      for (int p = lo + tid; p < hi; p += WBT_THREADS) {
        const int64_t i = g0 + p;
        int y = 0, sel = WBT_NONE;
        if (i >= 0 && i < n) {
          const int16_t *w0 = a + p - r;
          y = k <= 3 ? wbt_median_sel<3>(w0, k, &sel) : k <= 5 ? wbt_median_sel<5>(w0, k, &sel)
            : k <= 7 ? wbt_median_sel<7>(w0, k, &sel) : k <= 15 ? wbt_median_sel<15>(w0, k, &sel)
            : wbt_median_sel<31>(w0, k, &sel);
        }
        b[p] = (int16_t)y;
        ax[p] = (unsigned char)sel;
      }
    } else {  // FB_TF_QUANT, FB_TF_DECIMATE
      for (int p = lo + tid; p < hi; p += WBT_THREADS) {
        const int64_t i = g0 + p;
        int y = 0;
        unsigned char sat = 1;
        if (i >= 0 && i < n) {
          if (kind == FB_TF_QUANT) {
            const int x = a[p], q2 = x + k / 2;
            int d = q2 / k;
            if (q2 % k != 0 && q2 < 0) d -= 1;
            const int v = k * d;
            sat = (v < -32768 || v > 32767) ? 1 : 0;
            y = tf_clip16(v);
          } else {
            sat = (unsigned)i % (unsigned)k == 0 ? 0 : 1;   // (a decimation stage's byte: the sample is dropped)
            y = sat ? 0 : (int)a[p];
          }
        }
        b[p] = (int16_t)y;
        ax[p] = sat;
      }
    }
    __syncthreads();
    int16_t *t = a;
    a = b;
    b = t;
  }
  // ---- the stages in reverse on the cotangent: [clo, chi) of `ca` holds the cotangent of stage s's output
  int clo = 0, chi = Wc;
  for (int s = ch.n - 1; s >= 0; --s) {
    const int kind = ch.kind[s], k = ch.k[s];
    const unsigned char *ax = aux + (size_t)s * Wf + H;   // indexed by pc
    if (kind == FB_TF_FIR) {
      const int c = (k - 1) >> 1;
      const double *__restrict__ h = taps + ch.tap_off[s];
      for (int pc = clo + tid; pc < chi; pc += WBT_THREADS)
        if (ax[pc]) ca[pc] = 0.0;   // saturated outputs (and positions outside the utterance) pass nothing
      __syncthreads();
      clo += c;
      chi -= c;
      for (int pc = clo + tid; pc < chi; pc += WBT_THREADS) {
        const int64_t i = c0 + pc;
        double acc = 0.0;
        if (i >= 0 && i < n)
          for (int j = 0; j < k; ++j) acc = __dadd_rn(acc, __dmul_rn(h[j], ca[pc - c + j]));
        cb[pc] = acc;
      }
    } else if (kind == FB_TF_MEDIAN) {
      const int r = (k - 1) >> 1;
      clo += r;
      chi -= r;
      for (int pc = clo + tid; pc < chi; pc += WBT_THREADS) {
        const int64_t i = c0 + pc;
        double acc = 0.0;
        if (i >= 0 && i < n)
          for (int o = pc - r; o <= pc + r; ++o)   // output o selected window position pc - o + r?
            if ((int)ax[o] == pc - o + r) acc = __dadd_rn(acc, ca[o]);
        cb[pc] = acc;
      }
    } else {  // QUANT, NOISE: straight through unless saturated; DECIMATE: the kept samples
      for (int pc = clo + tid; pc < chi; pc += WBT_THREADS) cb[pc] = ax[pc] ? 0.0 : ca[pc];
    }
    __syncthreads();
    double *t = ca;
    ca = cb;
    cb = t;
  }
  // clo == H, chi == H + TILE: the tile
  for (int pc = H + tid; pc < H + FB_WBT_TILE; pc += WBT_THREADS) {
    const int64_t i = c0 + pc;
    if (i < n) grad[i] = accumulate ? __dadd_rn(grad[i], ca[pc]) : ca[pc];
  }
}

size_t fb_wb_chain_t_lds_bytes(const FbTfChain &ch) {
  const size_t Wc = FB_WBT_TILE + 2 * (size_t)ch.H, Wf = FB_WBT_TILE + 4 * (size_t)ch.H;
  return 2 * Wc * sizeof(double) + 2 * (Wf + WBT_PAD) * sizeof(int16_t) + (size_t)ch.n * Wf;
}

bool fb_launch_wb_chain_t(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav, int64_t n, const FbTfRnd &rn,
                          int replica, const double *cot, double *grad, int accumulate, const int *stop) {
  const size_t shm = fb_wb_chain_t_lds_bytes(ch);
  static std::atomic<unsigned long long> optin{0};
  unsigned long long bit = 0;
  if (shm > 64 * 1024 && fb_device_needs_optin(optin, &bit)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_wb_chain_t), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return false;
    optin.fetch_or(bit, std::memory_order_release);
  }
  const unsigned tiles = (unsigned)((n + FB_WBT_TILE - 1) / FB_WBT_TILE);
  hipLaunchKernelGGL(k_wb_chain_t, dim3(tiles > 0 ? tiles : 1), dim3(WBT_THREADS), shm, s, ch, taps, wav, n, rn, replica, cot, grad,
                     accumulate, stop);
  return true;
}
