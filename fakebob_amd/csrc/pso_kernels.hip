// pso_kernels.hip -- the particle-swarm attack's device side (fb_attack_pso; the "particle-swarm attack" section of
// include/fakebob_hip.h): the swarm's initialisation and its update.  Everything that scores a swarm is the ordinary
// batch path; these two kernels are element-wise, with no exchange between threads, no atomics and no loop control.
//
// All float64 arithmetic is written with explicit round-to-nearest operations, one per operation of the contract, so that
// a numpy restatement reproduces every position, velocity and int16 sample bit for bit.
#include "fb_device.h"
#include "fb_kernels.h"

#define FB_PSO_BLOCK 64   // threads of a workgroup: at N = 48 000 a launch has 24 000 threads, 375 workgroups over the 256 CUs

namespace {

// clip(s, l, h) = min(max(s, l), h)
__device__ __forceinline__ double pso_clip(double s, double l, double h) {
  s = s < l ? l : s;
  return s > h ? h : s;
}
// U(w) = ((double)w + 0.5) * 2^-32: exact, inside (0, 1)
__device__ __forceinline__ double pso_u(uint32_t w) { return __dmul_rn(__dadd_rn((double)w, 0.5), 0x1p-32); }

// the element pair (i0, i0 + 1) of a row: one 16-byte access when VEC (N even: every row starts 16-byte aligned and the
// pair is whole), two scalar ones otherwise (`two`: the second element exists)
template <bool VEC>
__device__ __forceinline__ void pso_ld2(const double *p, bool two, double (&o)[2]) {
  if constexpr (VEC) {
    const double2 t = *reinterpret_cast<const double2 *>(p);
    o[0] = t.x; o[1] = t.y;
  } else {
    o[0] = p[0];
    o[1] = two ? p[1] : 0.0;
  }
}
template <bool VEC>
__device__ __forceinline__ void pso_st2(double *p, bool two, const double (&o)[2]) {
  if constexpr (VEC) {
    *reinterpret_cast<double2 *>(p) = make_double2(o[0], o[1]);
  } else {
    p[0] = o[0];
    if (two) p[1] = o[1];
  }
}
template <bool VEC>
__device__ __forceinline__ void pso_stq(int16_t *p, bool two, const double (&o)[2], double qscale) {
  const int16_t q0 = fb_quantize(o[0], qscale), q1 = fb_quantize(o[1], qscale);
  if constexpr (VEC) {
    *reinterpret_cast<short2 *>(p) = make_short2(q0, q1);
  } else {
    p[0] = q0;
    if (two) p[1] = q1;
  }
}
// lo = clip(a - eps, -1, 1), hi = clip(a + eps, -1, 1)  (FAKEBOB.py:163-164)
__device__ __forceinline__ void pso_ball(const double (&a)[2], double eps, double (&lo)[2], double (&hi)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    lo[h] = pso_clip(__dsub_rn(a[h], eps), -1.0, 1.0);
    hi[h] = pso_clip(__dadd_rn(a[h], eps), -1.0, 1.0);
  }
}

// grid.x over element pairs, grid.y over particles (nothing is shared between particles here)
template <bool VEC>
__global__ __launch_bounds__(FB_PSO_BLOCK) void k_pso_init(const double *__restrict__ audio, int64_t N, double eps, double vmax,
                                                           uint32_t k0, uint32_t k1, double qscale, double *__restrict__ x,
                                                           double *__restrict__ v, int16_t *__restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * FB_PSO_BLOCK + threadIdx.x;
  const int64_t i0 = 2 * j;
  if (i0 >= N) return;
  const bool two = i0 + 1 < N;
  const int p = blockIdx.y;
  double a[2], xv[2], vv[2];
  pso_ld2<VEC>(audio + i0, two, a);
  if (p == 0) {  // the swarm's first particle is the original audio at rest
    xv[0] = a[0]; xv[1] = a[1];
    vv[0] = vv[1] = 0.0;
  } else {
    double lo[2], hi[2];
    pso_ball(a, eps, lo, hi);
    uint32_t r[4];
    fb_philox4x32_10((uint32_t)j, (uint32_t)p, 0u, 0u, k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double ux = pso_u(r[2 * h]), uv = pso_u(r[2 * h + 1]);
      xv[h] = pso_clip(__dadd_rn(lo[h], __dmul_rn(ux, __dsub_rn(hi[h], lo[h]))), lo[h], hi[h]);
      vv[h] = __dmul_rn(__dsub_rn(__dmul_rn(2.0, uv), 1.0), vmax);  // 2 u - 1 is exact
    }
  }
  const int64_t off = (int64_t)p * N + i0;
  pso_st2<VEC>(x + off, two, xv);
  pso_st2<VEC>(v + off, two, vv);
  pso_stq<VEC>(q + off, two, xv, qscale);
}

// One thread owns the element pair (2 j, 2 j + 1) of ALL particles and walks over them.  Nobody else touches its columns, so
// the launch also takes along what the host decided from this iteration's losses: the new global best (gb <- x of particle
// g_new, read before the walk overwrites that column), the new personal bests (pb_p <- x_p where bit p of `improved` is set)
// and the int16 cast of the new positions into the next batch.  The ball is recomputed from the audio.
template <bool VEC>
__global__ __launch_bounds__(FB_PSO_BLOCK) void k_pso_step(const double *__restrict__ audio, int64_t N, int P, double eps,
                                                           double *__restrict__ x, double *__restrict__ v, double *__restrict__ pb,
                                                           double *__restrict__ gb, unsigned long long improved, int g_new,
                                                           double w, double c1, double c2, double vmax, uint32_t k0, uint32_t k1,
                                                           uint32_t t, double qscale, int16_t *__restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * FB_PSO_BLOCK + threadIdx.x;
  const int64_t i0 = 2 * j;
  if (i0 >= N) return;
  const bool two = i0 + 1 < N;
  double a[2], lo[2], hi[2], g[2];
  pso_ld2<VEC>(audio + i0, two, a);
  if (g_new >= 0) {
    pso_ld2<VEC>(x + (int64_t)g_new * N + i0, two, g);
    pso_st2<VEC>(gb + i0, two, g);
  } else {
    pso_ld2<VEC>(gb + i0, two, g);
  }
  pso_ball(a, eps, lo, hi);
  const double nvmax = -vmax;
#pragma unroll 4
  for (int p = 0; p < P; ++p) {
    const int64_t off = (int64_t)p * N + i0;
    double xv[2], vv[2], bv[2];
    pso_ld2<VEC>(x + off, two, xv);
    pso_ld2<VEC>(v + off, two, vv);
    if ((improved >> p) & 1ull) {
      bv[0] = xv[0]; bv[1] = xv[1];
      pso_st2<VEC>(pb + off, two, bv);
    } else {
      pso_ld2<VEC>(pb + off, two, bv);
    }
    uint32_t r[4];
    fb_philox4x32_10((uint32_t)j, (uint32_t)p, t, 0u, k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double r1 = pso_u(r[2 * h]), r2 = pso_u(r[2 * h + 1]);
      const double inert = __dmul_rn(w, vv[h]);
      const double cog = __dmul_rn(__dmul_rn(c1, r1), __dsub_rn(bv[h], xv[h]));
      const double soc = __dmul_rn(__dmul_rn(c2, r2), __dsub_rn(g[h], xv[h]));
      vv[h] = pso_clip(__dadd_rn(__dadd_rn(inert, cog), soc), nvmax, vmax);
      xv[h] = pso_clip(__dadd_rn(xv[h], vv[h]), lo[h], hi[h]);
    }
    pso_st2<VEC>(x + off, two, xv);
    pso_st2<VEC>(v + off, two, vv);
    pso_stq<VEC>(q + off, two, xv, qscale);
  }
}

inline unsigned pso_blocks(int64_t N) { return (unsigned)(((N + 1) / 2 + FB_PSO_BLOCK - 1) / FB_PSO_BLOCK); }

}  // namespace

void fb_launch_pso_init(hipStream_t s, const double *audio, int64_t N, int P, double eps, double vmax, uint64_t seed,
                        uint32_t stream, int bits, double *x, double *v, int16_t *q) {
  const uint32_t k0 = (uint32_t)seed ^ FB_PSO_KEY, k1 = (uint32_t)(seed >> 32) ^ stream;
  const dim3 grid(pso_blocks(N), (unsigned)P);
  if ((N & 1) == 0)
    hipLaunchKernelGGL(k_pso_init<true>, grid, dim3(FB_PSO_BLOCK), 0, s, audio, N, eps, vmax, k0, k1, ldexp(1.0, bits - 1), x, v, q);
  else
    hipLaunchKernelGGL(k_pso_init<false>, grid, dim3(FB_PSO_BLOCK), 0, s, audio, N, eps, vmax, k0, k1, ldexp(1.0, bits - 1), x, v, q);
}

void fb_launch_pso_step(hipStream_t s, const double *audio, int64_t N, int P, double eps, double *x, double *v, double *pb,
                        double *gb, unsigned long long improved, int g_new, double w, double c1, double c2, double vmax,
                        uint64_t seed, uint32_t stream, uint32_t t, int bits, int16_t *q) {
  const uint32_t k0 = (uint32_t)seed ^ FB_PSO_KEY, k1 = (uint32_t)(seed >> 32) ^ stream;
  const dim3 grid(pso_blocks(N));
  if ((N & 1) == 0)
    hipLaunchKernelGGL(k_pso_step<true>, grid, dim3(FB_PSO_BLOCK), 0, s, audio, N, P, eps, x, v, pb, gb, improved, g_new, w, c1,
                       c2, vmax, k0, k1, t, ldexp(1.0, bits - 1), q);
  else
    hipLaunchKernelGGL(k_pso_step<false>, grid, dim3(FB_PSO_BLOCK), 0, s, audio, N, P, eps, x, v, pb, gb, improved, g_new, w, c1,
                       c2, vmax, k0, k1, t, ldexp(1.0, bits - 1), q);
}
