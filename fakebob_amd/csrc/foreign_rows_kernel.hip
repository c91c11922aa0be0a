// foreign_rows_kernel.hip -- the two launches between the int16 batch of fb_attack_pso / fb_attack_kenansville / fb_attack_hsj
// and a foreign victim (the "foreign victims for the swarm and the decision-only attacks" section of include/fakebob_hip.h).
//
// k_rows_to_model<T>: q [rows][N] int16 -> x [rows][N] T, x = (T)q * 2^-(bits - 1).  |q| <= 2^15 and the scale is a power of
//   two, so the product is exact in float32 as in float64: this is the audio an attacker would submit as a wav file.  A pure
//   bandwidth pass (2 bytes read, 4 or 8 written per sample): every thread takes 8 consecutive samples of the FLAT range
//   rows * N -- one 16-byte load, two (float) or four (double) 16-byte stores --, so an odd N misaligns nothing, and the grid
//   strides over the range.  The last total % 8 samples, and everything when x is not 16-byte aligned, go one by one.
//   Plain vector stores; no atomics, no LDS, no scratch.
// k_decide_foreign<T>: scores [rows][S] T -> the look block {decisions [rows] int32, scores [rows][S] float64}.  One thread per
//   row (S <= 62, rows <= 1024: a few thousand values, the launch is there so that the host reads ONE block per batch and the
//   device path copies no score back on its own).  The rule is the make_decisions rule of the "decision-only attack"
//   section; float32 scores are widened (exactly) before any comparison.
#include "fb_device.h"
#include "fb_kernels.h"

#define ROWS_BLOCK 256
#define ROWS_MAX_BLOCKS 2048   // 256 CUs x 8 workgroups: beyond that the grid strides

typedef short fb_short8 __attribute__((ext_vector_type(8)));

template <typename T> struct RowsVec;
template <> struct RowsVec<float> { typedef float type __attribute__((ext_vector_type(4))); enum { PER = 4 }; };
template <> struct RowsVec<double> { typedef double type __attribute__((ext_vector_type(2))); enum { PER = 2 }; };

template <typename T, bool VEC>
__global__ __launch_bounds__(ROWS_BLOCK) void k_rows_to_model(const int16_t *__restrict__ q, long long total, T scale,
                                                              T *__restrict__ x) {
  const long long stride = (long long)gridDim.x * ROWS_BLOCK;
  const long long tid = (long long)blockIdx.x * ROWS_BLOCK + threadIdx.x;
  if (VEC) {
    typedef typename RowsVec<T>::type V;
    const int PER = RowsVec<T>::PER;
    const long long groups = total >> 3;   // whole groups of 8 samples: q + 8 g and x + 8 g are 16-byte aligned
    for (long long g = tid; g < groups; g += stride) {
      const fb_short8 v = *reinterpret_cast<const fb_short8 *>(q + 8 * g);
      V *out = reinterpret_cast<V *>(x + 8 * g);
#pragma unroll
      for (int c = 0; c < 8 / PER; ++c) {
        V o;
#pragma unroll
        for (int i = 0; i < PER; ++i) o[i] = (T)v[c * PER + i] * scale;
        out[c] = o;
      }
    }
    const long long i = (groups << 3) + tid;   // the tail: fewer than 8 samples
    if (i < total) x[i] = (T)q[i] * scale;
  } else {
    for (long long i = tid; i < total; i += stride) x[i] = (T)q[i] * scale;
  }
}

template <typename T>
__global__ __launch_bounds__(ROWS_BLOCK) void k_decide_foreign(const T *__restrict__ scores, int rows, int S, int task,
                                                               double threshold, int *__restrict__ decisions,
                                                               double *__restrict__ scores_out) {
  const int b = blockIdx.x * ROWS_BLOCK + threadIdx.x;
  if (b >= rows) return;
  const T *s = scores + (size_t)b * S;
  double *o = scores_out + (size_t)b * S;
  double best = (double)s[0];
  int am = 0;
  o[0] = best;
  for (int m = 1; m < S; ++m) {   // the first maximum: a NaN never displaces the running maximum
    const double v = (double)s[m];
    o[m] = v;
    if (v > best) { best = v; am = m; }
  }
  int d;
  if (task == FB_TASK_SV) d = best >= threshold ? 1 : -1;
  else d = (task == FB_TASK_OSI && best < threshold) ? -1 : am;
  decisions[b] = d;
}

static unsigned rows_grid(long long work) {
  const long long blocks = (work + ROWS_BLOCK - 1) / ROWS_BLOCK;
  return (unsigned)(blocks < 1 ? 1 : (blocks > ROWS_MAX_BLOCKS ? ROWS_MAX_BLOCKS : blocks));
}

void fb_launch_rows_to_model(hipStream_t s, int x_dtype, const int16_t *q, int rows, int64_t N, int bits, void *x) {
  const long long total = (long long)rows * (long long)N;
  const double scale = ldexp(1.0, -(bits - 1));
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
  const unsigned grid = rows_grid(vec ? (total + 7) / 8 : total);
  if (x_dtype == FB_DT_F32) {
    if (vec) hipLaunchKernelGGL((k_rows_to_model<float, true>), dim3(grid), dim3(ROWS_BLOCK), 0, s, q, total, (float)scale, static_cast<float *>(x));
    else hipLaunchKernelGGL((k_rows_to_model<float, false>), dim3(grid), dim3(ROWS_BLOCK), 0, s, q, total, (float)scale, static_cast<float *>(x));
  } else {
    if (vec) hipLaunchKernelGGL((k_rows_to_model<double, true>), dim3(grid), dim3(ROWS_BLOCK), 0, s, q, total, scale, static_cast<double *>(x));
    else hipLaunchKernelGGL((k_rows_to_model<double, false>), dim3(grid), dim3(ROWS_BLOCK), 0, s, q, total, scale, static_cast<double *>(x));
  }
}

void fb_launch_decide_foreign(hipStream_t s, int score_dtype, const void *scores, int rows, int S, int task, double threshold,
                              int *decisions, double *scores_out) {
  const dim3 grid((unsigned)((rows + ROWS_BLOCK - 1) / ROWS_BLOCK));
  if (score_dtype == FB_DT_F32)
    hipLaunchKernelGGL(k_decide_foreign<float>, grid, dim3(ROWS_BLOCK), 0, s, static_cast<const float *>(scores), rows, S, task,
                       threshold, decisions, scores_out);
  else
    hipLaunchKernelGGL(k_decide_foreign<double>, grid, dim3(ROWS_BLOCK), 0, s, static_cast<const double *>(scores), rows, S, task,
                       threshold, decisions, scores_out);
}
