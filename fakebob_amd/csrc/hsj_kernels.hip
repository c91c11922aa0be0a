// hsj_kernels.hip -- HopSkipJump's device side (fb_attack_hsj; the "decision-only attack II" section of include/fakebob_hip.h).
// Everything that scores a batch is the ordinary batch path; the kernels here write the batches and keep the float64 state.
//
// One layout serves all of them: a workgroup of 256 threads stands on one CHUNK of 1024 samples, thread t on samples
// 1024 c + 4 t .. + 3 -- one Philox group of the NES generator (counter word 0 = 256 c + t) and one leaf of the contract's
// sum of squares, whose tree is the workgroup's.  With N a multiple of four every row starts 8-byte aligned as int16 and
// 32-byte aligned as float64, and a thread moves its group in 16-byte accesses (two for float64, one 8-byte store for
// int16); otherwise the group goes element by element (VEC = false).  No exchange between workgroups inside a launch, no
// atomics: the partial sums are added up by a launch of one workgroup (k_hsj_sum).
//
// All float64 arithmetic is written with explicit round-to-nearest operations, one per operation of the contract, so that a
// numpy restatement (tests/hsj_ref.py) reproduces every value bit for bit.
#include "fb_device.h"
#include "fb_kernels.h"

#define HSJ_BLOCK 256
#define HSJ_CHUNK 1024
#define HSJ_PROBE_ROWS 16   // rows a probes workgroup walks (grid.y = ceil(B / 16)): 64 x 188 workgroups at B = 1024, N = 48 000

namespace {

__device__ __forceinline__ double hsj_clip1(double s) {   // clip(s, -1, 1) = min(max(s, -1), 1)
  s = s < -1.0 ? -1.0 : s;
  return s > 1.0 ? 1.0 : s;
}

// the group's samples i0 .. i0 + cnt - 1 of a float64 row (cnt = 4 inside the row, less at its end; zero beyond it)
template <bool VEC>
__device__ __forceinline__ void hsj_ld4(const double *__restrict__ p, int cnt, double (&o)[4]) {
  if constexpr (VEC) {
    const double2 lo = *reinterpret_cast<const double2 *>(p), hi = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = lo.x; o[1] = lo.y; o[2] = hi.x; o[3] = hi.y;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = k < cnt ? p[k] : 0.0;
  }
}
template <bool VEC>
__device__ __forceinline__ void hsj_st4(double *__restrict__ p, int cnt, const double (&o)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<double2 *>(p) = make_double2(o[0], o[1]);
    *reinterpret_cast<double2 *>(p + 2) = make_double2(o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) p[k] = o[k];
  }
}
template <bool VEC>
__device__ __forceinline__ void hsj_stq4(int16_t *__restrict__ p, int cnt, const double (&o)[4], double qscale) {
  int16_t q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = fb_quantize(o[k], qscale);
  if constexpr (VEC) {
    *reinterpret_cast<short4 *>(p) = make_short4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) p[k] = q[k];
  }
}
template <bool VEC>
__device__ __forceinline__ void hsj_ldz4(const float *__restrict__ p, int cnt, float (&z)[4]) {
  if constexpr (VEC) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    z[0] = t.x; z[1] = t.y; z[2] = t.z; z[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = k < cnt ? p[k] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void hsj_stz4(float *__restrict__ p, int cnt, const float (&z)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4 *>(p) = make_float4(z[0], z[1], z[2], z[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) p[k] = z[k];
  }
}

// The NES generator's four normals of counter (n4, j, t, stream) under `key` -- fb_noise4's values bit for bit, with the
// quadrant applied by selects (fb_box_muller_sel).  With fb_noise4 itself (fb_box_muller's if-chain) inside k_hsj_probes' row
// loop the second normal of a pair came out wrong on the MI355X in some rows (tests/test_gpu_hsj.py at N = 2, B = 63); with
// the select form every value agrees with the oracle.  fb_device.h describes the same finding in the float64 MFCC kernels
// and traces it to how hipcc structures the if-chain; that was not looked into again here.
__device__ __forceinline__ void hsj_noise4(uint64_t key, uint32_t t, uint32_t stream, uint32_t n4, uint32_t j, float (&z)[4]) {
  uint32_t r[4];
  fb_philox4x32_10(n4, j, t, stream, (uint32_t)key, (uint32_t)(key >> 32), r);
  fb_box_muller_sel(r[0], r[1], z[0], z[1]);
  fb_box_muller_sel(r[2], r[3], z[2], z[3]);
}

// where thread t of chunk blockIdx.x stands: its first sample and how many of its four exist (0: none -- the thread still
// takes part in the chunk's sum, with zeros)
__device__ __forceinline__ int hsj_group(int64_t N, int64_t &i0) {
  i0 = (int64_t)blockIdx.x * HSJ_CHUNK + 4 * (int64_t)threadIdx.x;
  const int64_t left = N - i0;
  return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}

// ssq's chunk: s_t = ((v0^2 + v1^2) + v2^2) + v3^2, then s_t += s_{t + stride} for stride = 128 .. 1; thread 0 writes P_c.
// Every thread of the workgroup calls it (values beyond N are zero).
__device__ __forceinline__ void hsj_chunk_ssq(const double (&v)[4], double *__restrict__ part) {
  __shared__ double s_s[HSJ_BLOCK];
  const int t = threadIdx.x;
  double s = __dadd_rn(__dmul_rn(v[0], v[0]), __dmul_rn(v[1], v[1]));
  s = __dadd_rn(s, __dmul_rn(v[2], v[2]));
  s = __dadd_rn(s, __dmul_rn(v[3], v[3]));
  s_s[t] = s;
  __syncthreads();
#pragma unroll
  for (int stride = HSJ_BLOCK / 2; stride > 0; stride >>= 1) {
    if (t < stride) s_s[t] = __dadd_rn(s_s[t], s_s[t + stride]);
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = s_s[0];
}

// line(y, q) = a + (q 2^-20) (y - a): the difference, the exact scale, the product, the sum
__device__ __forceinline__ double hsj_line(double a, double y, double sc) {
  return __dadd_rn(a, __dmul_rn(sc, __dsub_rn(y, a)));
}

struct HsjQ { int q[FB_HSJ_MAX_GRID]; };

// row blockIdx.y of the round: the int16 cast of line(y, q.q[row])
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_line(const double *__restrict__ a, const double *__restrict__ y, int64_t N,
                                                        HsjQ q, double qscale, int16_t *__restrict__ out) {
  int64_t i0;
  const int cnt = hsj_group(N, i0);
  if (cnt == 0) return;
  const int row = blockIdx.y;
  const double sc = __dmul_rn((double)q.q[row], 0x1p-20);   // exact
  double av[4], yv[4], o[4];
  hsj_ld4<VEC>(a + i0, cnt, av);
  hsj_ld4<VEC>(y + i0, cnt, yv);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = hsj_line(av[k], yv[k], sc);
  hsj_stq4<VEC>(out + (int64_t)row * N + i0, cnt, o, qscale);
}

// the adopt launch: x = line(y, q) in float64 and the chunk sums of ssq(x - a)
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_adopt(const double *__restrict__ a, const double *__restrict__ y, int64_t N,
                                                         int q, double *__restrict__ x, double *__restrict__ part) {
  int64_t i0;
  const int cnt = hsj_group(N, i0);
  const double sc = __dmul_rn((double)q, 0x1p-20);
  double d[4] = {0.0, 0.0, 0.0, 0.0};
  if (cnt > 0) {
    double av[4], yv[4], o[4];
    hsj_ld4<VEC>(a + i0, cnt, av);
    hsj_ld4<VEC>(y + i0, cnt, yv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = hsj_line(av[k], yv[k], sc);
      d[k] = k < cnt ? __dsub_rn(o[k], av[k]) : 0.0;
    }
    hsj_st4<VEC>(x + i0, cnt, o);
  }
  hsj_chunk_ssq(d, part);
}

// ssq = P_0 + P_1 + ... in ascending c: one workgroup, the chunk sums staged through LDS a block at a time, one thread adds
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_sum(const double *__restrict__ part, int n, double *__restrict__ out) {
  __shared__ double s_p[HSJ_BLOCK];
  double acc = 0.0;
  for (int base = 0; base < n; base += HSJ_BLOCK) {
    const int i = base + (int)threadIdx.x;
    s_p[threadIdx.x] = i < n ? part[i] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = n - base < HSJ_BLOCK ? n - base : HSJ_BLOCK;
      for (int k = 0; k < m; ++k) acc = __dadd_rn(acc, s_p[k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = acc;
}

// rows j0 .. of the probes: the int16 cast of clip(x + sigma z_j, -1, 1); z_j of the NES generator under the probes' key.
// zkeep (nullable): the normals as float32 [B][N], for a direction launch that reads them back instead of drawing again
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_probes(const double *__restrict__ x, int64_t N, int B, double sigma,
                                                          uint64_t key, uint32_t t, uint32_t stream, double qscale,
                                                          int16_t *__restrict__ out, float *__restrict__ zkeep) {
  int64_t i0;
  const int cnt = hsj_group(N, i0);
  if (cnt == 0) return;
  const uint32_t n4 = (uint32_t)(i0 >> 2);
  double xv[4];
  hsj_ld4<VEC>(x + i0, cnt, xv);
  const int j0 = blockIdx.y * HSJ_PROBE_ROWS, j1 = min(j0 + HSJ_PROBE_ROWS, B);
  for (int j = j0; j < j1; ++j) {
    float z[4];
    hsj_noise4(key, t, stream, n4, (uint32_t)j, z);
    double o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = hsj_clip1(__dadd_rn(xv[k], __dmul_rn(sigma, (double)z[k])));
    hsj_stq4<VEC>(out + (int64_t)j * N + i0, cnt, o, qscale);
    if (zkeep) hsj_stz4<VEC>(zkeep + (int64_t)j * N + i0, cnt, z);
  }
}

// v[i] = sum_j (double)w_j (double)z_j[i]: from 0.0, j ascending, one rounded add per j (every product is exact: |w_j| <= 2 B
// <= 2^11 times a float32).  The order of the adds is fixed, the order of the DRAWS is not, and the draws are the work (a
// Philox block and two Box-Muller transforms per four samples and row against one add per sample and row): a workgroup
// stands on 16 groups = 64 samples and draws 16 rows side by side -- thread (g, r) = (tid & 15, tid >> 4) draws group g of
// row j0 + r into LDS --, and wave 0's thread s adds the 16 rows of sample s in ascending j while the other waves draw the
// next 16 (two LDS buffers, one barrier per 16 rows).  One thread walking all the rows of its group, as k_hsj_probes does
// for 16 of them, took 591 us at B = 1024, N = 48 000: 188 workgroups, 1024 draws deep.
// zkept (nullable): the probes launch's normals instead of fresh draws.
#define HSJ_DIR_GROUPS 16
#define HSJ_DIR_LANES 16
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_dir(const int32_t *__restrict__ w, int B, int64_t N, uint64_t key, uint32_t t,
                                                       uint32_t stream, const float *__restrict__ zkept, double *__restrict__ v) {
  __shared__ double s_w[FB_HSJ_MAX_EVALS];
  __shared__ __attribute__((aligned(16))) float s_z[2][HSJ_DIR_LANES][4 * HSJ_DIR_GROUPS];
  const int tid = threadIdx.x, g = tid & (HSJ_DIR_GROUPS - 1), r = tid / HSJ_DIR_GROUPS;
  for (int j = tid; j < B; j += HSJ_BLOCK) s_w[j] = (double)w[j];
  const int64_t n4 = (int64_t)blockIdx.x * HSJ_DIR_GROUPS + g, i0 = 4 * n4, left = N - i0;
  const int cnt = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  double acc = 0.0;
  int buf = 0;
  for (int j0 = 0; j0 < B; j0 += HSJ_DIR_LANES, buf ^= 1) {
    const int j = j0 + r;
    if (j < B) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (cnt > 0) {
        if (zkept) hsj_ldz4<VEC>(zkept + (int64_t)j * N + i0, cnt, z);
        else hsj_noise4(key, t, stream, (uint32_t)n4, (uint32_t)j, z);
      }
      *reinterpret_cast<float4 *>(&s_z[buf][r][4 * g]) = make_float4(z[0], z[1], z[2], z[3]);
    }
    __syncthreads();   // (also: s_w is complete before its first use)
    if (tid < 4 * HSJ_DIR_GROUPS) {
      const int rows = B - j0 < HSJ_DIR_LANES ? B - j0 : HSJ_DIR_LANES;
#pragma unroll 4
      for (int rr = 0; rr < rows; ++rr) acc = __dadd_rn(acc, __dmul_rn(s_w[j0 + rr], (double)s_z[buf][rr][tid]));
    }
    // no second barrier: the next trip writes the other buffer, and nobody writes this one again before the barrier of
    // the next trip, which wave 0 reaches only after these reads
  }
  const int64_t i = (int64_t)blockIdx.x * (4 * HSJ_DIR_GROUPS) + tid;
  if (tid < 4 * HSJ_DIR_GROUPS && i < N) v[i] = acc;
}

// the chunk sums of ssq(v)
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_ssq(const double *__restrict__ v, int64_t N, double *__restrict__ part) {
  int64_t i0;
  const int cnt = hsj_group(N, i0);
  double d[4] = {0.0, 0.0, 0.0, 0.0};
  if (cnt > 0) hsj_ld4<VEC>(v + i0, cnt, d);
  hsj_chunk_ssq(d, part);
}

// y_m = clip(x + c_m v, -1, 1), c_m = S > 0 ? (xi 2^-m) / sqrt(S) : 0, m = m0 + blockIdx.y; as int16 rows (rows != null: row
// blockIdx.y) or as ONE float64 row (yout)
template <bool VEC>
__global__ __launch_bounds__(HSJ_BLOCK) void k_hsj_step(const double *__restrict__ x, const double *__restrict__ v,
                                                        const double *__restrict__ S_dev, double xi, int m0, int64_t N,
                                                        double qscale, int16_t *__restrict__ rows, double *__restrict__ yout) {
  int64_t i0;
  const int cnt = hsj_group(N, i0);
  if (cnt == 0) return;
  const int m = m0 + (int)blockIdx.y;
  const double S = *S_dev;
  const double two_m = __longlong_as_double((long long)(1023 - m) << 52);   // 2^-m, m <= 63
  const double c = S > 0.0 ? __ddiv_rn(__dmul_rn(xi, two_m), __dsqrt_rn(S)) : 0.0;
  double xv[4], vv[4], o[4];
  hsj_ld4<VEC>(x + i0, cnt, xv);
  hsj_ld4<VEC>(v + i0, cnt, vv);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = hsj_clip1(__dadd_rn(xv[k], __dmul_rn(c, vv[k])));
  if (rows) hsj_stq4<VEC>(rows + (int64_t)blockIdx.y * N + i0, cnt, o, qscale);
  else hsj_st4<VEC>(yout + i0, cnt, o);
}

inline unsigned hsj_chunks(int64_t N) { return (unsigned)((N + HSJ_CHUNK - 1) / HSJ_CHUNK); }
inline uint64_t hsj_key(uint64_t seed) { return seed ^ (uint64_t)FB_HSJ_KEY; }

}  // namespace

int fb_hsj_chunks(int64_t N) { return (int)hsj_chunks(N); }

void fb_launch_hsj_line(hipStream_t s, const double *a, const double *y, int64_t N, int rows, const int *q, int bits,
                        int16_t *out) {
  HsjQ hq = {};
  for (int j = 0; j < rows && j < FB_HSJ_MAX_GRID; ++j) hq.q[j] = q[j];
  const dim3 grid(hsj_chunks(N), (unsigned)rows);
  if ((N & 3) == 0) hipLaunchKernelGGL(k_hsj_line<true>, grid, dim3(HSJ_BLOCK), 0, s, a, y, N, hq, ldexp(1.0, bits - 1), out);
  else hipLaunchKernelGGL(k_hsj_line<false>, grid, dim3(HSJ_BLOCK), 0, s, a, y, N, hq, ldexp(1.0, bits - 1), out);
}

void fb_launch_hsj_sum(hipStream_t s, const double *part, int n, double *out) {
  hipLaunchKernelGGL(k_hsj_sum, dim3(1), dim3(HSJ_BLOCK), 0, s, part, n, out);
}

void fb_launch_hsj_adopt(hipStream_t s, const double *a, const double *y, int64_t N, int q, double *x, double *part) {
  const dim3 grid(hsj_chunks(N));
  if ((N & 3) == 0) hipLaunchKernelGGL(k_hsj_adopt<true>, grid, dim3(HSJ_BLOCK), 0, s, a, y, N, q, x, part);
  else hipLaunchKernelGGL(k_hsj_adopt<false>, grid, dim3(HSJ_BLOCK), 0, s, a, y, N, q, x, part);
}

void fb_launch_hsj_probes(hipStream_t s, const double *x, int64_t N, int B, double sigma, uint64_t seed, uint32_t stream,
                          uint32_t t, int bits, int16_t *out, float *zkeep) {
  const dim3 grid(hsj_chunks(N), (unsigned)((B + HSJ_PROBE_ROWS - 1) / HSJ_PROBE_ROWS));
  if ((N & 3) == 0)
    hipLaunchKernelGGL(k_hsj_probes<true>, grid, dim3(HSJ_BLOCK), 0, s, x, N, B, sigma, hsj_key(seed), t, stream,
                       ldexp(1.0, bits - 1), out, zkeep);
  else
    hipLaunchKernelGGL(k_hsj_probes<false>, grid, dim3(HSJ_BLOCK), 0, s, x, N, B, sigma, hsj_key(seed), t, stream,
                       ldexp(1.0, bits - 1), out, zkeep);
}

void fb_launch_hsj_dir(hipStream_t s, const int32_t *w, int B, int64_t N, uint64_t seed, uint32_t stream, uint32_t t,
                       const float *zkept, double *v, double *part) {
  const dim3 grid((unsigned)((N + 4 * HSJ_DIR_GROUPS - 1) / (4 * HSJ_DIR_GROUPS)));
  if ((N & 3) == 0) {
    hipLaunchKernelGGL(k_hsj_dir<true>, grid, dim3(HSJ_BLOCK), 0, s, w, B, N, hsj_key(seed), t, stream, zkept, v);
    hipLaunchKernelGGL(k_hsj_ssq<true>, dim3(hsj_chunks(N)), dim3(HSJ_BLOCK), 0, s, v, N, part);
  } else {
    hipLaunchKernelGGL(k_hsj_dir<false>, grid, dim3(HSJ_BLOCK), 0, s, w, B, N, hsj_key(seed), t, stream, zkept, v);
    hipLaunchKernelGGL(k_hsj_ssq<false>, dim3(hsj_chunks(N)), dim3(HSJ_BLOCK), 0, s, v, N, part);
  }
}

void fb_launch_hsj_step(hipStream_t s, const double *x, const double *v, const double *S_dev, double xi, int m0, int count,
                        int64_t N, int bits, int16_t *rows, double *yout) {
  const dim3 grid(hsj_chunks(N), (unsigned)(rows ? count : 1));
  if ((N & 3) == 0)
    hipLaunchKernelGGL(k_hsj_step<true>, grid, dim3(HSJ_BLOCK), 0, s, x, v, S_dev, xi, m0, N, ldexp(1.0, bits - 1), rows, yout);
  else
    hipLaunchKernelGGL(k_hsj_step<false>, grid, dim3(HSJ_BLOCK), 0, s, x, v, S_dev, xi, m0, N, ldexp(1.0, bits - 1), rows, yout);
}
