// whitebox_universal_kernels.hip -- the composition of fb_set_companions transposed, for white-box gradients of a universal
// perturbation (fb_set_wb_universal; the "Universal perturbations" paragraph of include/fakebob_hip.h), gfx950.
//
//   k_wb_compose_t     grad[i] = sum_rho m_{u(rho)}[i] * cot[rho][i], rho = u * eot + j ascending, float64 from +0.0, one rounding
//                      per addition: ONE launch for all R = K * eot replicas.  m_0 = 1; for u >= 1 m_u[i] = 1 where
//                      comp[u - 1][i] + q[i] - a0[i], int32 -- tf_composed's arithmetic before its clip --, lies inside
//                      [-32768, 32767] (a sample AT a rail that was not clipped passes), 0 elsewhere: a masked term adds +0.0.
//   k_wb_iv_ctl_rep    k_wb_iv_ctl for one replica of R > 1: an i-vector system's weights from replica rho's OWN scores, over R;
//                      replica 0's launch also runs the loop control on the means the loss launch left (k_wb_ctl_rep's twin)
//   k_wb_compose_rows  the K composed rows as tf_composed forms them, written out: the chain's transpose (k_wb_chain_t) reads
//                      the row the chain read, which the forward kept in LDS only.
//
// k_wb_compose_t is a pure stream: R * 8 + (K + 1) * 2 bytes read and 8 written per sample, nothing reused, so no LDS.  A lane
// owns whole samples -- two neighbours per step when n is even, so that every row of cot starts on a 16-byte boundary and the
// cotangents come in 16-byte loads, the int16 streams in 4-byte ones; one sample per step when n is odd -- and sums its rho in
// the loop's order: no atomics, nothing exchanged, the same bits on every run and in either form.  Grid-stride over n.  An
// utterance's int16 samples are read once per replica of it: the eot - 1 repeats hit the cache, HBM sees them once.  Workgroups
// of 64: at N = 48 000 there are 24 000 lanes' worth of work, which 256-thread workgroups would put on 94 of the 256 compute units.
#include "fb_device.h"
#include "fb_kernels.h"
#include "whitebox_device.h"

#define WBU_THREADS 256      // k_wb_compose_rows
#define WBU_T_THREADS 64     // k_wb_compose_t
#define WBU_MAX_BLOCKS 2048  // (8 workgroups on each of 256 compute units)

static __device__ __forceinline__ bool wbu_inside(int v) { return v >= -32768 && v <= 32767; }

__global__ __launch_bounds__(WBU_T_THREADS) void k_wb_compose_t(const double *__restrict__ cot, const int16_t *__restrict__ q,
                                                              const int16_t *__restrict__ a0, const int16_t *__restrict__ comp,
                                                              int K, int eot, int64_t n, double *__restrict__ grad,
                                                              const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int64_t first = (int64_t)blockIdx.x * WBU_T_THREADS + threadIdx.x, step = (int64_t)gridDim.x * WBU_T_THREADS;
  const int R = K * eot;
  if ((n & 1) == 0) {
    for (int64_t p = first; 2 * p < n; p += step) {
      const int64_t i = 2 * p;
      const short2 qv = *reinterpret_cast<const short2 *>(q + i), av = *reinterpret_cast<const short2 *>(a0 + i);
      const int d0 = (int)qv.x - (int)av.x, d1 = (int)qv.y - (int)av.y;
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 4
      for (int rho = 0; rho < R; ++rho) {   // (the loads of four replicas are in flight before the first addition waits for one)
        const int u = rho / eot;
        bool m0 = true, m1 = true;
        if (u > 0) {
          const short2 cv = *reinterpret_cast<const short2 *>(comp + (int64_t)(u - 1) * n + i);
          m0 = wbu_inside((int)cv.x + d0);
          m1 = wbu_inside((int)cv.y + d1);
        }
        const double2 g = *reinterpret_cast<const double2 *>(cot + (int64_t)rho * n + i);
        acc0 = __dadd_rn(acc0, m0 ? g.x : 0.0);
        acc1 = __dadd_rn(acc1, m1 ? g.y : 0.0);
      }
      *reinterpret_cast<double2 *>(grad + i) = make_double2(acc0, acc1);
    }
  } else {
    for (int64_t i = first; i < n; i += step) {
      const int d = (int)q[i] - (int)a0[i];
      double acc = 0.0;
#pragma unroll 4
      for (int rho = 0; rho < R; ++rho) {
        const int u = rho / eot;
        const bool m = u == 0 || wbu_inside((int)comp[(int64_t)(u - 1) * n + i] + d);
        acc = __dadd_rn(acc, m ? cot[(int64_t)rho * n + i] : 0.0);
      }
      grad[i] = acc;
    }
  }
}

// rows[u][i], u = 0 .. K - 1: q for u = 0, else clip16(comp[u - 1][i] + q[i] - a0[i]) (tf_composed)
__global__ __launch_bounds__(WBU_THREADS) void k_wb_compose_rows(const int16_t *__restrict__ q, const int16_t *__restrict__ a0,
                                                                 const int16_t *__restrict__ comp, int K, int64_t n,
                                                                 int16_t *__restrict__ rows, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int64_t step = (int64_t)gridDim.x * WBU_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * WBU_THREADS + threadIdx.x; i < n; i += step) {
    const int v = q[i], d = v - (int)a0[i];
    rows[i] = (int16_t)v;
    for (int u = 1; u < K; ++u) {
      const int c = (int)comp[(int64_t)(u - 1) * n + i] + d;
      rows[(int64_t)u * n + i] = (int16_t)(c < -32768 ? -32768 : c > 32767 ? 32767 : c);
    }
  }
}

// One thread (k_wb_ctl_rep's shape).  1 / R is a power of two only for some R: the product is rounded once per weight.
__global__ __launch_bounds__(64) void k_wb_iv_ctl_rep(const double *__restrict__ rep_scores, const double *__restrict__ mean_scores,
                                                      const FbNesDev *__restrict__ out, int S, int R, int task, int attack_type,
                                                      const double *__restrict__ z_std, double threshold, int target, int true_label,
                                                      double *__restrict__ w, FbCtlDev *__restrict__ ctl, int do_ctl,
                                                      double *__restrict__ trace, int it) {
  if (threadIdx.x != 0) return;
  if (ctl && ctl->stop) return;
  fb_wb_iv_weights(rep_scores, S, task, attack_type, z_std, threshold, target, true_label, w);
  if (R > 1) {
    const double inv = 1.0 / (double)R;
    for (int s = 0; s < S; ++s) w[s] *= inv;
  }
  if (ctl && do_ctl) fb_wb_loop_control(mean_scores, out, task == FB_TASK_CSI ? S : S + 1, task, ctl, trace, it);
}

void fb_launch_wb_iv_ctl_rep(hipStream_t s, const double *rep_scores, const double *mean_scores, const FbNesDev *out, int S, int R,
                             int task, int attack_type, const double *z_std, double threshold, int target, int true_label, double *w,
                             FbCtlDev *ctl, int do_ctl, double *trace, int it) {
  hipLaunchKernelGGL(k_wb_iv_ctl_rep, dim3(1), dim3(64), 0, s, rep_scores, mean_scores, out, S, R, task, attack_type, z_std, threshold,
                     target, true_label, w, ctl, do_ctl, trace, it);
}

static unsigned wbu_blocks(int64_t items, int threads = WBU_THREADS) {
  const int64_t b = (items + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : b > WBU_MAX_BLOCKS ? WBU_MAX_BLOCKS : b);
}

void fb_launch_wb_compose_t(hipStream_t s, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp, int K, int eot,
                            int64_t n, double *grad, const int *stop) {
  hipLaunchKernelGGL(k_wb_compose_t, dim3(wbu_blocks((n & 1) == 0 ? n / 2 : n, WBU_T_THREADS)), dim3(WBU_T_THREADS), 0, s, cot, q, a0, comp, K, eot, n,
                     grad, stop);
}

void fb_launch_wb_compose_rows(hipStream_t s, const int16_t *q, const int16_t *a0, const int16_t *comp, int K, int64_t n, int16_t *rows,
                               const int *stop) {
  hipLaunchKernelGGL(k_wb_compose_rows, dim3(wbu_blocks(n)), dim3(WBU_THREADS), 0, s, q, a0, comp, K, n, rows, stop);
}
