// whitebox_air_kernels.hip -- the over-the-air channel transposed, for white-box gradients through it (fb_set_wb_air; the
// contract is the last paragraph of "Defended victims: BPDA and EOT" in include/fakebob_hip.h), gfx950.
//
// k_air_conv_t   one workgroup per (row, chunk of AIRT_CHUNK samples of dx): the correlation of a float64 cotangent with the
//                row's int16 taps as the Toeplitz GEMM of k_air_conv (air_channel_kernel.hip), mirrored.  With m = 16 a + b:
//                    dX[a][b] = sum_j G[a][j] * H[j][b],   G[a][j] = g[16 a + j],   H[j][b] = t[j - b] (zero outside [0, L)),
//                j = 0 .. L + 14, on v_mfma_f64_16x16x4_f64 -- the forward read L - 1 samples of history, this reads L + 14
//                FUTURE samples; g is the cotangent on the channel's output, zero at or beyond n and wherever the forward's
//                value saturated (one byte per output sample, written by k_air_conv<true>: the rail itself proves nothing,
//                32767 is a legitimate value).  dx = 2^-14 * the sum (the scaling is exact).  The lane maps are the f64 ones
//                documented at the top of air_channel_kernel.hip; a wave owns AIRT_TILES blocks of 16 x 16 outputs, which
//                share one H fragment per K step, and its stores are contiguous.
// k_air_sum_t    grad[i] = sum_j dx[j][i], j ascending, one rounding per sum: the replicas of one row.
// All rows of a launch have the same length n (the replicas of the one row of a white-box call), so one launch covers them:
// grid (chunks, rows).  Nothing is exchanged between workgroups, there are no atomics, every global index is checked
// against [0, n), and the `stop` flag is honoured.
//
// LDS.  The A operand is float64 here: a chunk and its future halo cost 8 bytes per sample where the forward's cost 2, so
// the forward's 4096-output chunk does not fit under 64 KB at L = 4096 (8192 samples: 64 KB before the taps).  The chunk is
// 2048 outputs, not the 160 KB opt-in k_wb_chain_t takes: 2048 + 4096 samples in 18 slots per 16 are 55.3 KB, the taps
// (int16, widened at the read as in the forward) 8.3 KB -- 63.6 KB, no opt-in, no second resident-workgroup limit to think
// about -- and a 48 000-sample row becomes 24 workgroups instead of 12 on a device that one row leaves mostly idle.  The
// price is the halo: at L = 4096 a workgroup loads three samples per output where a 4096 chunk would load two; the
// multiply-adds per output, L + 15, do not depend on the chunk.
// The pad.  Rows of an A fragment are 16 samples = 128 B apart: without a pad the 16 rows of a fragment fall on two groups
// of LDS banks.  With 16 samples in 18 slots a row is 36 banks further (mod 64: sixteen distinct multiples of four), and the
// two K columns of a half wave fill the other two banks of each group: the 32 lanes of a pass read 64 distinct banks.
// 17 slots leave one pair of lanes in conflict.  AIRT_PAD is the template parameter; FB_AIRT_PAD=16|17 in the environment
// selects the other instantiations for timing (same bits: the layout changes no sum).  DESIGN.md section 6 has the figures.
#include <stdlib.h>

#include "fb_device.h"
#include "fb_kernels.h"

#define AIRT_THREADS 256
#define AIRT_TILES 2                                                 // 16 x 16 output blocks per wave
#define AIRT_CHUNK ((AIRT_THREADS / FB_WAVE) * AIRT_TILES * 256)      // samples of dx per workgroup: 2048

typedef double airt_d4 __attribute__((ext_vector_type(4)));

// K steps' worth of future samples: the j range 0 .. L + 14 rounded up to whole steps of 4, less the 16 of the tile itself
// (air_hist of the forward)
static __host__ __device__ __forceinline__ int airt_fut(int L) { return ((L + 15 + 3) & ~3) - 16; }
// LDS slot of sample position p: 16 samples take PAD slots
template <int PAD>
static __host__ __device__ __forceinline__ int airt_xpos(int p) { return p + (PAD - 16) * (p >> 4); }

// dx row R (R = blockIdx.y; rows of n samples) = 2^-14 * the correlation of cot row R -- zeroed where sat row R (nullable)
// is set -- with taps[R][L]
template <int PAD>
__global__ __launch_bounds__(AIRT_THREADS) void k_air_conv_t(const double *__restrict__ cot, const unsigned char *__restrict__ sat,
                                                             int64_t n, const int16_t *__restrict__ taps, int L,
                                                             double *__restrict__ dx, const int *__restrict__ stop) {
  extern __shared__ double airt_lds[];
  if (stop && *stop) return;
  const int R = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * AIRT_CHUNK;
  if (c0 >= n) return;
  const int FUT = airt_fut(L), NX = AIRT_CHUNK + FUT, NT = FUT + 31;
  double *gs = airt_lds;                                                          // slot airt_xpos(p) <-> sample c0 + p, p in [0, NX)
  int16_t *ts = reinterpret_cast<int16_t *>(airt_lds + ((airt_xpos<PAD>(NX) + 1) & ~1));  // ts[q] = t[q - 15], q in [0, NT)
  const int tid = threadIdx.x;
  const int64_t rbase = (int64_t)R * n;
  for (int p = tid; p < NX; p += AIRT_THREADS) {
    const int64_t i = c0 + p;
    double v = 0.0;
    if (i < n && !(sat && sat[rbase + i])) v = cot[rbase + i];
    gs[airt_xpos<PAD>(p)] = v;
  }
  for (int q = tid; q < NT; q += AIRT_THREADS) {
    const int k = q - 15;
    ts[q] = (k >= 0 && k < L) ? taps[(int64_t)R * L + k] : (int16_t)0;
  }
  __syncthreads();
  const int wv = tid / FB_WAVE, lane = tid % FB_WAVE;
  const int64_t w0 = c0 + (int64_t)wv * (AIRT_TILES * 256);  // the wave's first output
  if (w0 >= n) return;
  const int b = lane & 15, kk = lane >> 4;
  airt_d4 acc[AIRT_TILES];
#pragma unroll
  for (int T = 0; T < AIRT_TILES; ++T) acc[T] = airt_d4{0.0, 0.0, 0.0, 0.0};
  // K step s covers j = s + kk: the A operand of block T is sample position wv * 512 + 256 T + 16 b + s + kk, the B operand
  // (lane: k = kk, column b) is t[j - b] = ts[s + kk - b + 15]
  const int pa = wv * (AIRT_TILES * 256) + 16 * b + kk;
  const int qb = kk - b + 15;
  // Near the row's end the future is zeros: at step s the wave's A operands are the samples w0 + s and later -- the steps at
  // which even that one lies at or beyond n add nothing and are left out (wave-uniform)
  const int64_t left = n - w0;  // > 0
  const int s_end = left < (int64_t)(FUT + 16) ? (int)((left + 3) & ~(int64_t)3) : FUT + 16;
  for (int s = 0; s < s_end; s += 4) {
    const double hv = (double)ts[qb + s];
#pragma unroll
    for (int T = 0; T < AIRT_TILES; ++T) {
      const double gv = gs[airt_xpos<PAD>(pa + 256 * T + s)];
      acc[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(gv, hv, acc[T], 0, 0, 0);
    }
  }
#pragma unroll
  for (int T = 0; T < AIRT_TILES; ++T) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t i = w0 + 256 * T + 64 * g + lane;
      if (i < n) dx[rbase + i] = __dmul_rn(acc[T][g], 6.103515625e-05);  // 2^-14
    }
  }
}

__global__ __launch_bounds__(256) void k_air_sum_t(const double *__restrict__ dx, int r, int64_t n, double *__restrict__ grad,
                                                   const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = dx[i];
  for (int j = 1; j < r; ++j) acc = __dadd_rn(acc, dx[(int64_t)j * n + i]);
  grad[i] = acc;
}

template <int PAD>
static size_t airt_lds_bytes(int L) {
  const int FUT = airt_fut(L), NX = AIRT_CHUNK + FUT;
  return sizeof(double) * (size_t)((airt_xpos<PAD>(NX) + 1) & ~1) + sizeof(int16_t) * (size_t)(FUT + 31 + 1);
}

int fb_air_conv_t_chunk(void) { return AIRT_CHUNK; }

void fb_launch_air_conv_t(hipStream_t s, const double *cot, const unsigned char *sat, int rows, int64_t n, const int16_t *taps, int L,
                          double *dx, const int *stop) {
  const unsigned chunks = (unsigned)((n + AIRT_CHUNK - 1) / AIRT_CHUNK);
  const dim3 grid(chunks > 0 ? chunks : 1, rows);
  static const int pad = [] {
    const char *ev = getenv("FB_AIRT_PAD");
    const int v = ev ? atoi(ev) : 18;
    return v == 16 || v == 17 ? v : 18;
  }();
  if (pad == 16) hipLaunchKernelGGL(k_air_conv_t<16>, grid, dim3(AIRT_THREADS), airt_lds_bytes<16>(L), s, cot, sat, n, taps, L, dx, stop);
  else if (pad == 17) hipLaunchKernelGGL(k_air_conv_t<17>, grid, dim3(AIRT_THREADS), airt_lds_bytes<17>(L), s, cot, sat, n, taps, L, dx, stop);
  else hipLaunchKernelGGL(k_air_conv_t<18>, grid, dim3(AIRT_THREADS), airt_lds_bytes<18>(L), s, cot, sat, n, taps, L, dx, stop);
}

void fb_launch_air_sum_t(hipStream_t s, const double *dx, int r, int64_t n, double *grad, const int *stop) {
  hipLaunchKernelGGL(k_air_sum_t, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dx, r, n, grad, stop);
}
