// play_offset_kernels.hip -- the play offset (fb_set_play_offset; the "Play offset" section of include/fakebob_hip.h), gfx950.
//
//   k_play_compose        out[R][i] = clip16(a_u[i] + q_b[s] - a_0[s]), s = (i - tau_R) mod n, for the rows R = b * r' + rho of the
//                         replicated batch (u = rho / eot; a_u = a_0 for u = 0), and tau[R], drawn here: ONE launch in front of
//                         the air and chain launches, which then run in their "input already replicated" modes.
//   k_wb_play_compose_t   the same composition transposed: grad[k] = sum over rho ascending of m_rho[i] * cot[rho][i] at
//                         i = (k + tau_rho) mod n, float64 from +0.0, one rounding per addition, a masked term adding +0.0.
//
// k_play_compose is a pure stream: B * r' * n * 2 bytes written, the sources (q_b, a_0, the companions) re-read r' times out
// of L2.  `out` is taken as ONE flat array of 16-byte chunks of eight samples, whatever n is, so every store is a 16-byte one
// on a 16-byte boundary; the workgroups of row R own the chunks that START in row R.  A lane owns a chunk.  Its three source
// runs of eight samples start anywhere: each is read as the four or five ALIGNED dwords that cover it and, where it starts
// in the upper half of a dword, realigned in registers (v_alignbit by 16).  Two kinds of chunk leave that path and go sample by
// sample, each sample picked out of the aligned dword that holds it: the chunk whose rotated source meets the wrap (one per
// row, wherever it falls in a workgroup's tile), and a chunk that runs over the end of its row into the next rows (n not a
// multiple of eight) -- its later samples are the next rows', composed with THEIR offsets.  No division or remainder per
// sample: one per workgroup for (b, rho, u), conditional subtractions elsewhere.
#include "fb_device.h"
#include "fb_kernels.h"

#define PO_THREADS 256
#define PO_CHUNK 8                         // samples of one 16-byte store
#define PO_TILE (PO_THREADS * PO_CHUNK)    // samples of a workgroup's tile
#define PO_T_THREADS 64                    // k_wb_play_compose_t (k_wb_compose_t's shape)
#define PO_T_MAX_BLOCKS 2048

static __device__ __forceinline__ int po_clip16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// tau of (utterance row utt, replica rho): word 0 of the Philox call, scaled to 0 .. S
static __device__ __forceinline__ uint32_t po_draw(const FbPlay &pk, uint32_t utt, uint32_t rho) {
  uint32_t r[4];
  fb_philox4x32_10(0u, rho, pk.utt0 + utt, pk.epoch, pk.k0, pk.k1, r);
  return __umulhi(r[0], pk.S + 1u);
}

// the sample at p, out of the aligned dword that holds it
static __device__ __forceinline__ int po_ld1(const int16_t *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t w = *reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
  return (int)(int16_t)((a & 2) ? (w >> 16) : (w & 0xffffu));
}
// the eight samples from p on as four dwords: the aligned dwords that cover them, shifted by 16 bits where p is the upper half
// of one (every dword read holds at least one of the samples asked for)
static __device__ __forceinline__ void po_ld8(const int16_t *p, uint32_t w[4]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t *d = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
  const uint32_t x0 = d[0], x1 = d[1], x2 = d[2], x3 = d[3];
  if (a & 2) {
    const uint32_t x4 = d[4];
    w[0] = __builtin_amdgcn_alignbit(x1, x0, 16);
    w[1] = __builtin_amdgcn_alignbit(x2, x1, 16);
    w[2] = __builtin_amdgcn_alignbit(x3, x2, 16);
    w[3] = __builtin_amdgcn_alignbit(x4, x3, 16);
  } else {
    w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
  }
}
static __device__ __forceinline__ int po_lo(uint32_t w) { return (int)(int16_t)(w & 0xffffu); }
static __device__ __forceinline__ int po_hi(uint32_t w) { return (int)(int16_t)(w >> 16); }

// one composed sample of row R (b, rho, u known), the slow way
static __device__ __forceinline__ int po_one(const int16_t *qb, const int16_t *a0, const int16_t *au, int64_t n, int64_t i, int64_t tau) {
  int64_t s = i - tau;
  if (s < 0) s += n;
  return po_clip16(po_ld1(au + i) + po_ld1(qb + s) - po_ld1(a0 + s));
}

__global__ __launch_bounds__(PO_THREADS) void k_play_compose(FbPlay pk, const int16_t *__restrict__ q, FbTfComp cn, int eot, int rows,
                                                             int16_t *__restrict__ out, uint32_t *__restrict__ tau_out,
                                                             const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int64_t n = cn.N;
  const int R = blockIdx.y, rr = cn.K * eot;
  const int b = R / rr, rho = R - b * rr, u = rho / eot;
  const uint32_t tau = po_draw(pk, (uint32_t)b, (uint32_t)rho);
  if (blockIdx.x == 0 && threadIdx.x == 0) tau_out[R] = tau;
  // the chunks that start in row R: flat samples 8 c in [R n, (R + 1) n)
  const int64_t f0 = (int64_t)R * n, c_lo = (f0 + PO_CHUNK - 1) >> 3, c_hi = (f0 + n + PO_CHUNK - 1) >> 3;
  const int64_t c = c_lo + (int64_t)blockIdx.x * PO_THREADS + threadIdx.x;
  if (c >= c_hi) return;
  const int64_t i = 8 * c - f0;  // 0 <= i < n
  const int16_t *qb = q + (int64_t)b * n, *au = u == 0 ? cn.a0 : cn.comp + (int64_t)(u - 1) * n;
  int64_t s = i - (int64_t)tau;
  if (s < 0) s += n;
  uint32_t o[4];
  if (i + PO_CHUNK <= n && s + PO_CHUNK <= n) {
    uint32_t wa[4], wq[4], w0[4];
    po_ld8(au + i, wa);
    po_ld8(qb + s, wq);
    po_ld8(cn.a0 + s, w0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int lo = po_clip16(po_lo(wa[k]) + po_lo(wq[k]) - po_lo(w0[k]));
      const int hi = po_clip16(po_hi(wa[k]) + po_hi(wq[k]) - po_hi(w0[k]));
      o[k] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
    }
  } else {
    // the wrap inside the chunk, or the chunk runs into the next rows: sample by sample, moving on a row where one ends
    int Rk = R, bk = b, rhok = rho;
    int64_t ik = i, tk = tau;
    const int16_t *qk = qb, *ak = au;
    int v[PO_CHUNK];
#pragma unroll
    for (int k = 0; k < PO_CHUNK; ++k) {
      if (ik >= n) {  // (n < 8: more than once per chunk)
        ik = 0;
        Rk += 1;
        rhok += 1;
        if (rhok == rr) { rhok = 0; bk += 1; }
        if (Rk < rows) {
          int uk = 0;
          for (int t = rhok; t >= eot; t -= eot) uk += 1;
          tk = po_draw(pk, (uint32_t)bk, (uint32_t)rhok);
          qk = q + (int64_t)bk * n;
          ak = uk == 0 ? cn.a0 : cn.comp + (int64_t)(uk - 1) * n;
        }
      }
      v[k] = Rk < rows ? po_one(qk, cn.a0, ak, n, ik, tk) : 0;  // (behind the last row: the buffer's padding)
      ik += 1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ((uint32_t)v[2 * k] & 0xffffu) | ((uint32_t)v[2 * k + 1] << 16);
  }
  *reinterpret_cast<uint4 *>(out + 8 * c) = make_uint4(o[0], o[1], o[2], o[3]);
}

// the draw alone (fb_debug_play_offsets): tau[R], R = b * r + rho
__global__ __launch_bounds__(64) void k_play_offsets(FbPlay pk, int r, int rows, uint32_t *__restrict__ tau_out) {
  const int R = blockIdx.x * 64 + threadIdx.x;
  if (R >= rows) return;
  const int b = R / r;
  tau_out[R] = po_draw(pk, (uint32_t)b, (uint32_t)(R - b * r));
}

// A lane owns whole output samples k and sums its rho in the loop's order: no atomics, the same bits on every run.  The
// difference d = q[k] - a0[k] is the lane's own; replica rho's mask and cotangent sit at i = (k + tau_rho) mod n.
__global__ __launch_bounds__(PO_T_THREADS) void k_wb_play_compose_t(const double *__restrict__ cot, const int16_t *__restrict__ q,
                                                                  const int16_t *__restrict__ a0, const int16_t *__restrict__ comp,
                                                                  const uint32_t *__restrict__ tau, int K, int eot, int64_t n,
                                                                  double *__restrict__ grad, const int *__restrict__ stop) {
  if (stop && *stop) return;
  __shared__ uint32_t s_tau[32];
  const int R = K * eot;
  if (threadIdx.x < R) s_tau[threadIdx.x] = tau[threadIdx.x];
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * PO_T_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * PO_T_THREADS + threadIdx.x; k < n; k += step) {
    const int d = (int)q[k] - (int)a0[k];
    double acc = 0.0;
    int u = 0, j = 0;
#pragma unroll 4
    for (int rho = 0; rho < R; ++rho) {
      int64_t i = k + (int64_t)s_tau[rho];
      if (i >= n) i -= n;
      const int16_t *au = u == 0 ? a0 : comp + (int64_t)(u - 1) * n;
      const int v = (int)au[i] + d;
      const bool m = v >= -32768 && v <= 32767;
      acc = __dadd_rn(acc, m ? cot[(int64_t)rho * n + i] : 0.0);
      if (++j == eot) { j = 0; u += 1; }
    }
    grad[k] = acc;
  }
}

void fb_launch_play_compose(hipStream_t s, const FbPlay &pk, const int16_t *q, const FbTfComp &cn, int eot, int B, int16_t *out,
                            uint32_t *tau, const int *stop) {
  const int rows = B * cn.K * eot;
  const int64_t chunks = (cn.N + PO_CHUNK - 1) / PO_CHUNK + 1;  // (a row's share of the flat chunks: at most this many)
  hipLaunchKernelGGL(k_play_compose, dim3((unsigned)((chunks + PO_THREADS - 1) / PO_THREADS), (unsigned)rows), dim3(PO_THREADS), 0, s, pk, q,
                     cn, eot, rows, out, tau, stop);
}

void fb_launch_play_offsets(hipStream_t s, const FbPlay &pk, int r, int rows, uint32_t *tau) {
  hipLaunchKernelGGL(k_play_offsets, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, pk, r, rows, tau);
}

void fb_launch_wb_play_compose_t(hipStream_t s, const double *cot, const int16_t *q, const int16_t *a0, const int16_t *comp,
                                 const uint32_t *tau, int K, int eot, int64_t n, double *grad, const int *stop) {
  const int64_t b = (n + PO_T_THREADS - 1) / PO_T_THREADS;
  hipLaunchKernelGGL(k_wb_play_compose_t, dim3((unsigned)(b < 1 ? 1 : b > PO_T_MAX_BLOCKS ? PO_T_MAX_BLOCKS : b)), dim3(PO_T_THREADS), 0, s,
                     cot, q, a0, comp, tau, K, eot, n, grad, stop);
}
