// input_transform_device.h -- the stage arithmetic of the input-transform chain (the stage contract of include/fakebob_hip.h),
// shared by the forward kernels (input_transform_kernel.hip) and by the transposed chain that recomputes the forward's values
// (whitebox_bpda_kernels.hip): one statement of every rounding, so that the two cannot drift apart.
#pragma once
#include "fb_device.h"
#include "fb_kernels.h"

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

// FB_TF_NOISE: the standard normals of samples 4 q .. 4 q + 3 of utterance `utt` for (stage, replica) at the launch's point
// of the noise RNG contract
static __device__ __forceinline__ void tf_noise4(const FbTfRnd &rn, uint32_t utt, int stage, int replica, uint32_t q, float z[4]) {
  uint32_t r[4];
  fb_philox4x32_10(q, (uint32_t)(stage + 8 * replica), rn.utt0 + utt, rn.epoch, rn.k0, rn.k1, r);
  fb_box_muller_sel(r[0], r[1], z[0], z[1]);
  fb_box_muller_sel(r[2], r[3], z[2], z[3]);
}
// ... and the stage's scale: taps[0] itself (absolute mode) or sqrt(E / n / rho), E the utterance's exact sum of squares
static __device__ __forceinline__ double tf_noise_scale(int mode, double t0, unsigned long long E, int64_t n) {
  if (mode == 0) return t0;
  return __dsqrt_rn(__ddiv_rn(__ddiv_rn((double)E, (double)n), t0));
}
