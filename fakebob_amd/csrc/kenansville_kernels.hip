// kenansville_kernels.hip -- the decision-only attack's device side (fb_attack_kenansville; the "decision-only attack"
// section of include/fakebob_hip.h): the spectral analysis of the utterance, once per attack, and the candidates of a
// round, written straight into the int16 batch the front end scores.  Everything that scores a batch is the ordinary path.
//
// k_kv_analyse     one workgroup per KV_WIN windows.  The forward transform is a GEMM on the float64 matrix cores:
//                  AB[w][c] = sum_n X[w][n] * T[n][c],  X[w][n] = x[w W + n] (0 beyond N),  T[n][c] = CF[(n c) mod W] for
//                  c < K and SF[(n (c - K)) mod W] for K <= c < 2 K.  Every product is an integer below 2^45 and every partial
//                  sum one of at most 2^52 < 2^53, so v_mfma_f64_16x16x4_f64 is exact whatever order it sums in.  The sums
//                  go to LDS as integers; then a thread per (window, bin) rounds a and b, forms p and e, and finds cum[k] by
//                  counting: the sum of e[j] over the bins j whose pair (p[j], j) is not above (p[k], k) -- the prefix sum of
//                  the sorted order without the sort (K <= 65: at most 65 compares per bin).
// k_kv_candidates  one workgroup per window, all rows of the round.  The removed part is a GEMM again:
//                  R[row][n] = sum_c M[row][c] * IT[c][n],  M[row][c] = the coefficient m a[k] (c = k < K) or m b[k]
//                  (c = K + k) where cum[k] <= thr[row] and 0 elsewhere -- formed at the read from cum, E and the round's q
//                  list --, IT[c][n] = CI / SI[(n k) mod W].  Products below 2^45, sums of magnitudes at most 2^48: exact.
//                  Then r = floor((2 R + D) / (2 D)), y = clip16(x - r), one int16 store per sample; the 16 lanes of an
//                  accumulator register write 16 consecutive samples of a row.
//                  A 64-bit integer VALU form of both contractions was not built, so the choice is not a measured one: the
//                  matrix form is the exact one already in use here (k_air_conv); tools/kenansville_rate.py times it.
// Nothing is exchanged between workgroups, there are no atomics, and every global index is checked against [0, N) or the
// window count.  f64 MFMA lane maps: see air_channel_kernel.hip.
#include "fb_device.h"
#include "fb_kernels.h"

#define KV_THREADS 256
#define KV_WIN 16                          // windows per workgroup of k_kv_analyse: one MFMA tile's rows
#define KV_MAXW FB_KV_MAX_WINDOW           // 128
#define KV_MAXK (KV_MAXW / 2 + 1)          // 65
#define KV_COLS (((2 * KV_MAXK) + 15) / 16 * 16)   // 144: the columns of AB, padded to whole tiles

typedef double kv_d4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ int kv_bin_weight(int k, int W) { return (k == 0 || ((W & 1) == 0 && k == W / 2)) ? 1 : 2; }

__global__ __launch_bounds__(KV_THREADS) void k_kv_analyse(const int16_t *__restrict__ x, int64_t N, int W, int nw,
                                                           const int32_t *__restrict__ tab, int32_t *__restrict__ ma,
                                                           int32_t *__restrict__ mb, long long *__restrict__ cum,
                                                           long long *__restrict__ E) {
  __shared__ double s_cf[KV_MAXW], s_sf[KV_MAXW];
  __shared__ long long s_ab[KV_WIN][KV_COLS];      // the sums A (columns 0 .. K - 1) and B (K .. 2 K - 1); later p and e
  __shared__ int s_ma[KV_WIN][KV_MAXK], s_mb[KV_WIN][KV_MAXK];
  const int tid = threadIdx.x, K = W / 2 + 1;
  const int w0 = blockIdx.x * KV_WIN;
  for (int j = tid; j < W; j += KV_THREADS) {
    s_cf[j] = (double)tab[j];
    s_sf[j] = (double)tab[W + j];
  }
  __syncthreads();
  const int wv = tid / FB_WAVE, lane = tid % FB_WAVE;
  const int r16 = lane & 15, kk = lane >> 4;
  const int n_ct = (2 * K + 15) / 16;              // column tiles in use (at most 9)
  const int64_t xbase = (int64_t)(w0 + r16) * W;   // the A operand's window
  const bool win_ok = w0 + r16 < nw;
  for (int ct = wv; ct < n_ct; ct += KV_THREADS / FB_WAVE) {
    const int c = 16 * ct + r16;                   // the B operand's column
    const int kc = c < K ? c : c - K;
    const double *tb = c < K ? s_cf : s_sf;
    const bool col_ok = c < 2 * K;
    kv_d4 acc = kv_d4{0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < W; s += 4) {
      const int n = s + kk;
      double xv = 0.0, tv = 0.0;
      if (n < W) {
        const int64_t i = xbase + n;
        if (win_ok && i < N) xv = (double)x[i];
        if (col_ok) tv = tb[(n * kc) % W];
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, tv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) s_ab[kk + 4 * g][16 * ct + r16] = (long long)acc[g];   // exact integers, |.| <= 2^52
  }
  __syncthreads();
  // a, b (rounded, arithmetic shift), m a, m b; p and e take the places of A and B
  for (int t = tid; t < KV_WIN * K; t += KV_THREADS) {
    const int w = t / K, k = t - w * K;
    const long long a = (s_ab[w][k] + (1ll << 29)) >> 30, b = (s_ab[w][K + k] + (1ll << 29)) >> 30;
    const int m = kv_bin_weight(k, W);
    s_ma[w][k] = (int)(m * a);
    s_mb[w][k] = (int)(m * b);
    const long long p = a * a + b * b;
    s_ab[w][k] = p;
    s_ab[w][K + k] = m * p;
  }
  __syncthreads();
  for (int t = tid; t < KV_WIN * K; t += KV_THREADS) {
    const int w = t / K, k = t - w * K;
    if (w0 + w >= nw) continue;
    const long long pk = s_ab[w][k];
    long long c = 0, tot = 0;
    for (int j = 0; j < K; ++j) {
      const long long pj = s_ab[w][j], ej = s_ab[w][K + j];
      tot += ej;
      if (pj < pk || (pj == pk && j <= k)) c += ej;
    }
    const int64_t o = (int64_t)(w0 + w) * K + k;
    ma[o] = s_ma[w][k];
    mb[o] = s_mb[w][k];
    cum[o] = c;
    if (k == 0) E[w0 + w] = tot;
  }
}

struct KvQ { int q[FB_KV_MAX_ROWS]; };

// y[row][N] (row = 0 .. rows - 1, at out + row * N): candidate q.q[row] of x
__global__ __launch_bounds__(KV_THREADS) void k_kv_candidates(const int16_t *__restrict__ x, int64_t N, int W, int rows, KvQ q,
                                                              const int32_t *__restrict__ tab, const int32_t *__restrict__ ma,
                                                              const int32_t *__restrict__ mb, const long long *__restrict__ cum,
                                                              const long long *__restrict__ E, int16_t *__restrict__ out) {
  __shared__ double s_ci[KV_MAXW], s_si[KV_MAXW], s_coef[2 * KV_MAXK];
  __shared__ long long s_cum[KV_MAXK], s_thr[FB_KV_MAX_ROWS];
  const int tid = threadIdx.x, K = W / 2 + 1;
  const int w = blockIdx.x;
  for (int j = tid; j < W; j += KV_THREADS) {
    s_ci[j] = (double)tab[2 * W + j];
    s_si[j] = (double)tab[3 * W + j];
  }
  for (int k = tid; k < K; k += KV_THREADS) {
    const int64_t o = (int64_t)w * K + k;
    s_coef[k] = (double)ma[o];
    s_coef[K + k] = (double)mb[o];
    s_cum[k] = cum[o];
  }
  if (tid < FB_KV_MAX_ROWS) {
    long long thr = -1;                            // rows beyond the round's: nothing is removed (cum >= 0), nothing is written
    if (tid < rows) {
      const long long Ew = E[w], qq = q.q[tid];
      thr = (Ew >> 16) * qq + (((Ew & 0xFFFF) * qq) >> 16);   // floor(E q / 65536), no overflow
    }
    s_thr[tid] = thr;
  }
  __syncthreads();
  const int wv = tid / FB_WAVE, lane = tid % FB_WAVE;
  const int r16 = lane & 15, kk = lane >> 4;
  const int n_nt = (W + 15) / 16, n_rt = (rows + 15) / 16;      // tiles over samples (columns) and over rows
  const long long D = (long long)W << 22;
  const int64_t base = (int64_t)w * W;
  for (int t = wv; t < n_nt * n_rt; t += KV_THREADS / FB_WAVE) {
    const int rt = t / n_nt, nt = t - rt * n_nt;
    const long long thr = s_thr[16 * rt + r16];   // the A operand's row
    const int n = 16 * nt + r16;                  // the B operand's sample
    kv_d4 acc = kv_d4{0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < 2 * K; s += 4) {
      const int c = s + kk;
      double mv = 0.0, tv = 0.0;
      if (c < 2 * K) {
        const int k = c < K ? c : c - K;
        if (s_cum[k] <= thr) mv = s_coef[c];
        tv = (c < K ? s_ci : s_si)[(n * k) % W];
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(mv, tv, acc, 0, 0, 0);
    }
    const int64_t i = base + n;
    if (n < W && i < N) {
      const int xv = x[i];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = 16 * rt + kk + 4 * g;
        if (row < rows) {
          const long long R = (long long)acc[g];  // an exact integer, |R| <= 2^48
          // floor((2 R + D) / (2 D)) with 2 D = W * 2^23: the arithmetic shift floors, then a 32-bit floor division by W
          // (floor(floor(v / 2^23) / W) = floor(v / (2^23 W)); the shifted value is below 2^27)
          const int num = (int)((2 * R + D) >> 23);
          int r = num / W;
          if (num < 0 && r * W != num) --r;
          const int y = xv - r;
          out[(int64_t)row * N + i] = (int16_t)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
        }
      }
    }
  }
}

}  // namespace

void fb_launch_kv_analyse(hipStream_t s, const int16_t *x, int64_t N, int W, const int32_t *tab, int32_t *ma, int32_t *mb,
                          long long *cum, long long *E) {
  const int nw = (int)((N + W - 1) / W);
  hipLaunchKernelGGL(k_kv_analyse, dim3((unsigned)((nw + KV_WIN - 1) / KV_WIN)), dim3(KV_THREADS), 0, s, x, N, W, nw, tab, ma, mb,
                     cum, E);
}

void fb_launch_kv_candidates(hipStream_t s, const int16_t *x, int64_t N, int W, int rows, const int *q, const int32_t *tab,
                             const int32_t *ma, const int32_t *mb, const long long *cum, const long long *E, int16_t *out) {
  const int nw = (int)((N + W - 1) / W);
  KvQ kq = {};
  for (int j = 0; j < rows && j < FB_KV_MAX_ROWS; ++j) kq.q[j] = q[j];
  hipLaunchKernelGGL(k_kv_candidates, dim3((unsigned)nw), dim3(KV_THREADS), 0, s, x, N, W, rows, kq, tab, ma, mb, cum, E, out);
}
