// input_transform_kernel.hip -- the input-transform chain of a defended system (fb_set_input_transform): up to 8
// int16 -> int16 stages (quantisation, median, FIR, decimation; the stage contract is in include/fakebob_hip.h) applied
// to every utterance of the batch in ONE launch, between the int16 cast and the MFCC.
//
// One workgroup = one (utterance, tile of FB_TF_TILE output samples).  It loads the tile plus a halo of H samples on
// either side -- H = the sum of the stages' radii -- into LDS, zeros wherever the index falls outside the utterance,
// and runs the stages between two LDS buffers with a barrier after each.  A stage of radius r reads [p - r, p + r], so
// the region that holds valid values shrinks by r per stage and ends as exactly the tile.  The contract's "indices
// outside [0, n) read as 0 at EVERY stage" is kept by writing 0, not the stage's value, at such positions.
// No workgroup reads what another one wrote: nothing is exchanged, nothing has to be restored behind a stopped attack.
//
// The stage list is a kernel argument and the taps are read at a wave-uniform index (scalar loads); a lane owns output
// samples.  The FIR sum is the contract's: float64, one rounding per product and per sum, taps ascending, no fused
// multiply-add (__dmul_rn / __dadd_rn; the library is built with contraction off as well).
//
// LDS: 2 * (FB_TF_TILE + 2 H + 4) int16 = 16 KB for a radius-0 chain, 24 KB at the largest halo (H = 1024) -- requested per
// launch, so that a workgroup fits beside another attack's k_gmm_fx2w workgroup (101 KB) on a compute unit.
#include "fb_kernels.h"

#define TF_THREADS 256
#define TF_PAD 4  // int16 behind each LDS buffer, kept zero: the FIR's groups of four outputs read up to 3 past the region

static __device__ __forceinline__ int tf_clip16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// FB_TF_QUANT: clip(q * floor_div(x + q / 2, q)), int32 arithmetic
static __device__ __forceinline__ int tf_quant(int x, int q) {
  const int a = x + q / 2;
  int d = a / q;
  if (a % q != 0 && a < 0) d -= 1;  // C division truncates: round toward -inf
  return tf_clip16(q * d);
}

// FB_TF_MEDIAN: the element of rank (k - 1) / 2 of w0[0 .. k), k <= KMAX.  The window sits in registers, padded to KMAX
// with a value above every int16 (the padding sorts last and leaves the rank of the median alone); an element's rank is
// counted under the strict order (value, position), so exactly one element has the wanted rank.
template <int KMAX>
static __device__ __forceinline__ int tf_median(const int16_t *w0, int k) {
  int w[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) w[j] = j < k ? (int)w0[j] : 0x10000;
  const int r = (k - 1) >> 1;
  int med = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    int rank = 0;
#pragma unroll
    for (int m = 0; m < KMAX; ++m)
      if (m != j) rank += (m < j) ? (w[m] <= w[j]) : (w[m] < w[j]);
    if (rank == r) med = w[j];
  }
  return med;
}

__global__ __launch_bounds__(TF_THREADS) void k_input_transform(FbTfChain ch, const double *__restrict__ taps,
                                                                const int16_t *__restrict__ wav,
                                                                const int64_t *__restrict__ wav_off,
                                                                int16_t *__restrict__ out, const int *__restrict__ stop) {
  extern __shared__ int16_t tf_lds[];
  if (stop && *stop) return;
  const int u = blockIdx.y;
  const int64_t base = wav_off[u];
  const int64_t n = wav_off[u + 1] - base;
  const int64_t t0 = (int64_t)blockIdx.x * FB_TF_TILE;
  if (t0 >= n) return;  // (the grid is sized for the longest utterance of the batch)
  const int H = ch.H, W = FB_TF_TILE + 2 * H;
  int16_t *a = tf_lds, *b = tf_lds + W + TF_PAD;
  const int tid = threadIdx.x;
  // LDS position p of either buffer <-> sample g0 + p of the utterance
  const int64_t g0 = t0 - H;
  for (int p = tid; p < W + TF_PAD; p += TF_THREADS) {
    const int64_t i = g0 + p;
    a[p] = (p < W && i >= 0 && i < n) ? wav[base + i] : (int16_t)0;
    if (p >= W) b[p] = 0;
  }
  __syncthreads();
  int lo = 0, hi = W;  // positions [lo, hi) of `a` hold the signal after the stages run so far
  for (int s = 0; s < ch.n; ++s) {
    const int kind = ch.kind[s], k = ch.k[s];
    if (kind == FB_TF_FIR) {
      const int c = (k - 1) >> 1;
      const double *__restrict__ h = taps + ch.tap_off[s];
      lo += c;
      hi -= c;
      // a lane owns four neighbouring outputs: the window slides by one sample per tap, one LDS read serves all four
      for (int p0 = lo + 4 * tid; p0 < hi; p0 += 4 * TF_THREADS) {
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        double v1 = (double)a[p0 + c + 1], v2 = (double)a[p0 + c + 2], v3 = (double)a[p0 + c + 3];
        for (int j = 0; j < k; ++j) {
          const double v0 = (double)a[p0 + c - j], hj = h[j];
          acc0 = __dadd_rn(acc0, __dmul_rn(hj, v0));
          acc1 = __dadd_rn(acc1, __dmul_rn(hj, v1));
          acc2 = __dadd_rn(acc2, __dmul_rn(hj, v2));
          acc3 = __dadd_rn(acc3, __dmul_rn(hj, v3));
          v3 = v2;
          v2 = v1;
          v1 = v0;
        }
        const double acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = p0 + q;
          const int64_t i = g0 + p;
          if (p < hi) {
            // |acc| <= 511 * 2^20 * 2^15 < 2^45: rint (ties to even) is exact, the clamp happens in float64
            const double y = fmin(fmax(rint(acc[q]), -32768.0), 32767.0);
            b[p] = (i >= 0 && i < n) ? (int16_t)(int)y : (int16_t)0;
          }
        }
      }
    } else if (kind == FB_TF_MEDIAN) {
      const int r = (k - 1) >> 1;
      lo += r;
      hi -= r;
      for (int p = lo + tid; p < hi; p += TF_THREADS) {
        const int64_t i = g0 + p;
        int y = 0;
        if (i >= 0 && i < n) {
          const int16_t *w0 = a + p - r;
          y = k <= 3 ? tf_median<3>(w0, k) : k <= 5 ? tf_median<5>(w0, k) : k <= 7 ? tf_median<7>(w0, k)
            : k <= 15 ? tf_median<15>(w0, k) : tf_median<31>(w0, k);
        }
        b[p] = (int16_t)y;
      }
    } else {  // FB_TF_QUANT, FB_TF_DECIMATE: sample by sample (zeros outside the utterance stay zeros)
      for (int p = lo + tid; p < hi; p += TF_THREADS) {
        const int64_t i = g0 + p;
        int y = 0;
        if (i >= 0 && i < n)  // (i < 2^31: an utterance's length is checked on the host)
          y = kind == FB_TF_QUANT ? tf_quant(a[p], k) : ((unsigned)i % (unsigned)k == 0 ? (int)a[p] : 0);
        b[p] = (int16_t)y;
      }
    }
    __syncthreads();
    int16_t *t = a;
    a = b;
    b = t;
  }
  // lo == H, hi == H + FB_TF_TILE: the tile
  for (int p = H + tid; p < H + FB_TF_TILE; p += TF_THREADS) {
    const int64_t i = g0 + p;
    if (i < n) out[base + i] = a[p];
  }
}

size_t fb_input_transform_lds_bytes(const FbTfChain &ch) { return sizeof(int16_t) * 2 * (size_t)(FB_TF_TILE + 2 * ch.H + TF_PAD); }

void fb_launch_input_transform(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                               const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  hipLaunchKernelGGL(k_input_transform, dim3(tiles > 0 ? tiles : 1, B), dim3(TF_THREADS), fb_input_transform_lds_bytes(ch), s,
                     ch, taps, wav, wav_off, out, stop);
}
