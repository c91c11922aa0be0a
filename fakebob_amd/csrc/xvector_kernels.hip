// xvector_kernels.hip -- the x-vector (TDNN) system between the front end's feature rows and the embedding (the "x-vector"
// section of fakebob_hip.h):
//   k_xv_rowinfo   {first row, rows} of its utterance for every voiced row of the batch
//   k_xv_rowmax    max |x| of every input row of a layer: what the per-row power of two of k_xv_affine is taken from
//   k_xv_affine    one frame layer: splice, affine on the matrix cores (three f16 products per K step), bias / ReLU /
//                  scale-offset epilogue; on request the ReLU's decisions, a byte per (row, channel)
//   k_xv_pool      mean and standard deviation per (utterance, channel), float64
//   k_xv_segment   the segment affine, float64
// Every result is a function of the utterance's own rows and the layer's shape: no atomics, no order that depends on the
// batch.  A workgroup's tile may hold rows of several utterances; an output element is one dot product whatever stands
// beside it.
#include "gmm_split.h"

#define XV_RT 4    // row tiles of 32 rows per workgroup
#define XV_CT 4    // column tiles of 32 channels per workgroup: one per wave
#define XV_KS 4    // K steps of 16 per LDS stage
#define XV_ROWS (32 * XV_RT)
static_assert(XV_RT == 4 && XV_CT == 4, "wave w of four builds row tile w's fragments and owns column tile w");

__global__ __launch_bounds__(256) void k_xv_rowinfo(const int *__restrict__ row_off, int2 *__restrict__ rowinfo) {
  const int b = blockIdx.x, r0 = row_off[b], T = row_off[b + 1] - r0;
  for (int t = threadIdx.x; t < T; t += 256) rowinfo[r0 + t] = make_int2(r0, T);
}
void fb_launch_xv_rowinfo(hipStream_t s, const int *row_off, int B, int2 *rowinfo) {
  hipLaunchKernelGGL(k_xv_rowinfo, dim3(B), dim3(256), 0, s, row_off, rowinfo);
}

// one wave per row
__global__ __launch_bounds__(256) void k_xv_rowmax(const float *__restrict__ x, int din, const int *__restrict__ n_rows_ptr,
                                                   float *__restrict__ amax) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= *n_rows_ptr) return;
  const float *xr = x + (size_t)row * din;
  float m = 0.0f;
  for (int c = lane; c < din; c += 64) m = fmaxf(m, fabsf(xr[c]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) amax[row] = m;
}
void fb_launch_xv_rowmax(hipStream_t s, const float *x, int din, const int *n_rows_ptr, int rows_cap, float *amax) {
  if (rows_cap <= 0) return;
  hipLaunchKernelGGL(k_xv_rowmax, dim3((rows_cap + 3) / 4), dim3(256), 0, s, x, din, n_rows_ptr, amax);
}

// y[row][ch] = scale[ch] * max(W[ch] . splice(x, row) + bias[ch], 0) + offset[ch].
// A workgroup of four waves owns XV_ROWS rows x 128 channels; wave w owns channels 32 (4 blockIdx.y + w) .. + 31 of all its
// rows (XV_RT accumulator tiles of 32 x 32).  The MFMA's A operand is the spliced input (M = row), its B operand the weights
// (N = channel), so a lane of the result holds ONE channel and 16 rows: the epilogue's per-channel constants are per lane
// and the stores of a register are 128 contiguous bytes per half wave.
// Per stage of XV_KS K steps: the waves gather the stage's spliced values (wave w those of row tile w), scale each row by its
// power of two, split them into their two f16 terms and leave them in LDS in fragment order -- 16 bytes per lane, a
// fragment is 1 KB contiguous, read back with one ds_read_b128 per lane and no bank conflict; then every wave runs
// hi.hi, hi.lo, lo.hi per (K step, row tile) against its own weight fragments, fetched from the load-time image with one
// global_load_dwordx4 per term.  The K order of an output element is ascending K step, the three products in that order.
__global__ __launch_bounds__(256) void k_xv_affine(FbXvLayerDev ly, const float *__restrict__ x, const float *__restrict__ amax,
                                                   const int2 *__restrict__ rowinfo, const int *__restrict__ n_rows_ptr,
                                                   float *__restrict__ y, unsigned char *__restrict__ mask) {
  __shared__ u32x4 sA[XV_KS][XV_RT][2][64];      // 32 KB
  __shared__ int sSrc[XV_ROWS][FB_XV_MAX_CTX];   // source row of (row, context place); -1: the row does not exist
  __shared__ int sSh[XV_ROWS];                   // the row's values are multiplied by 2^-sSh
  const int n_rows = *n_rows_ptr, row0 = blockIdx.x * XV_ROWS;
  if (row0 >= n_rows) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int din = ly.din, K = ly.K, n_steps = ly.n_steps;
  if (tid < XV_ROWS) {
    const int g = row0 + tid;
    int sh = 0;
    if (g < n_rows) {
      const int2 info = rowinfo[g];
      float am = 0.0f;
      for (int j = 0; j < ly.n_ctx; ++j) {
        const int src = info.x + min(max(g - info.x + ly.ctx[j], 0), info.y - 1);
        sSrc[tid][j] = src;
        am = fmaxf(am, amax[src]);
      }
      if (am > 0.0f) sh = (int)((__float_as_uint(am) >> 23) & 0xffu) - 127 - 14;   // am 2^-sh in [2^14, 2^15)
    } else {
      for (int j = 0; j < ly.n_ctx; ++j) sSrc[tid][j] = -1;
    }
    sSh[tid] = sh;
  }
  __syncthreads();
  const int ct = blockIdx.y * XV_CT + wave;
  const bool active = ct * 32 < ly.dout;
  const u32x4 *wimg = reinterpret_cast<const u32x4 *>(ly.w) + (size_t)ct * n_steps * 2 * 64 + lane;
  f32x16 acc[XV_RT];
#pragma unroll
  for (int rt = 0; rt < XV_RT; ++rt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[rt][i] = 0.0f;
  const int m_own = wave * 32 + (lane & 31);     // the row whose fragments this lane builds
  const int sh_own = sSh[m_own];
  for (int c0 = 0; c0 < n_steps; c0 += XV_KS) {
    const int ns = min(XV_KS, n_steps - c0);
    for (int s = 0; s < ns; ++s) {
      const int k0 = (c0 + s) * 16 + 8 * (lane >> 5);
      float v[8];
      if ((din & 7) == 0) {   // the 8 places lie in one context block
        float4 t0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), t1 = t0;
        if (k0 < K) {
          const int j = k0 / din, src = sSrc[m_own][j];
          if (src >= 0) {
            const float4 *p = reinterpret_cast<const float4 *>(x + (size_t)src * din + (k0 - j * din));
            t0 = p[0];
            t1 = p[1];
          }
        }
        v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = k0 + i;
          float t = 0.0f;
          if (k < K) {
            const int j = k / din, src = sSrc[m_own][j];
            if (src >= 0) t = x[(size_t)src * din + (k - j * din)];
          }
          v[i] = t;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = ldexpf(v[i], -sh_own);
      u32x4 f1, f2;
      fb_split2_frag(v, f1, f2);
      sA[s][wave][0][lane] = f1;
      sA[s][wave][1][lane] = f2;
    }
    __syncthreads();
    if (active) {
      for (int s = 0; s < ns; ++s) {
        const u32x4 b1 = wimg[(size_t)(c0 + s) * 128], b2 = wimg[(size_t)(c0 + s) * 128 + 64];
#pragma unroll
        for (int rt = 0; rt < XV_RT; ++rt) {
          const u32x4 a1 = sA[s][rt][0][lane], a2 = sA[s][rt][1][lane];
          FB_FX_MFMA(a1, b1, acc[rt]);
          FB_FX_MFMA(a1, b2, acc[rt]);
          FB_FX_MFMA(a2, b1, acc[rt]);
        }
      }
    }
    __syncthreads();
  }
  const int ch = ct * 32 + (lane & 31);
  if (!active || ch >= ly.dout) return;   // (a last column tile may be partial: its image holds zeros there)
  const float bias = ly.bias[ch], sc = ly.scale[ch], of = ly.offset[ch];
#pragma unroll
  for (int rt = 0; rt < XV_RT; ++rt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = rt * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3), g = row0 + m;
      if (g < n_rows) {
        float t = ldexpf(acc[rt][i], sSh[m] + ly.kw);
        t = __fadd_rn(t, bias);
        if (mask) mask[(size_t)g * ly.dout + ch] = t > 0.0f ? 1 : 0;   // the ReLU's decision, kept for the white-box backward
        t = fmaxf(t, 0.0f);
        y[(size_t)g * ly.dout + ch] = __fadd_rn(__fmul_rn(sc, t), of);
      }
    }
}
void fb_launch_xv_affine(hipStream_t s, const FbXvLayerDev &ly, const float *x, const float *amax, const int2 *rowinfo,
                         const int *n_rows_ptr, int rows_cap, float *y, unsigned char *mask) {
  if (rows_cap <= 0) return;
  const dim3 grid((rows_cap + XV_ROWS - 1) / XV_ROWS, (ly.dout + 32 * XV_CT - 1) / (32 * XV_CT));
  hipLaunchKernelGGL(k_xv_affine, grid, dim3(256), 0, s, ly, x, amax, rowinfo, n_rows_ptr, y, mask);
}

// One workgroup per (utterance, 64 channels): thread (q, c) sums quarter q of the utterance's rows, [T q / 4, T (q + 1) / 4),
// in ascending order; the quarters are added in fixed order.  stats[b] = {mean[P], std[P]}.
__global__ __launch_bounds__(256) void k_xv_pool(const float *__restrict__ h, int P, const int *__restrict__ row_off,
                                                 double *__restrict__ stats) {
  __shared__ double ps[4][64], pss[4][64];
  const int b = blockIdx.x, cl = threadIdx.x & 63, c = blockIdx.y * 64 + cl, q = threadIdx.x >> 6;
  const int r0 = row_off[b], T = row_off[b + 1] - r0;
  const int t0 = (int)((long long)T * q / 4), t1 = (int)((long long)T * (q + 1) / 4);
  double s = 0.0, ss = 0.0;
  if (c < P)
    for (int t = t0; t < t1; ++t) {
      const double v = (double)h[(size_t)(r0 + t) * P + c];
      s += v;
      ss = fma(v, v, ss);
    }
  ps[q][cl] = s;
  pss[q][cl] = ss;
  __syncthreads();
  if (q == 0 && c < P) {
    const double S = ((ps[0][cl] + ps[1][cl]) + ps[2][cl]) + ps[3][cl];
    const double SS = ((pss[0][cl] + pss[1][cl]) + pss[2][cl]) + pss[3][cl];
    const double mean = T > 0 ? S / (double)T : 0.0;
    const double var = (T > 0 ? SS / (double)T : 0.0) - mean * mean;
    stats[(size_t)b * 2 * P + c] = mean;
    stats[(size_t)b * 2 * P + P + c] = sqrt(fmax(var, 1.0e-10));
  }
}
void fb_launch_xv_pool(hipStream_t s, const float *h, int P, const int *row_off, int B, double *stats) {
  hipLaunchKernelGGL(k_xv_pool, dim3(B, (P + 63) / 64), dim3(256), 0, s, h, P, row_off, stats);
}

// One workgroup per (two utterances, 64 outputs): thread (g, r) runs share g of the contraction, [2P g / 4, 2P (g + 1) / 4),
// as one fma chain per utterance; the shares are added in fixed order, then the bias.  Two utterances share a weight
// fetch; each has its own chains.
#define XV_SEG_UB 2
__global__ __launch_bounds__(256) void k_xv_segment(FbXvDev xv, const double *__restrict__ stats, int B, double *__restrict__ emb) {
  extern __shared__ __attribute__((aligned(16))) double xv_sm[];
  const int P2 = 2 * xv.P, R = xv.R, b0 = blockIdx.x * XV_SEG_UB;
  const int rl = threadIdx.x & 63, r = blockIdx.y * 64 + rl, g = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < XV_SEG_UB * P2; i += 256) {
    const int u = i / P2;
    xv_sm[i] = b0 + u < B ? stats[(size_t)b0 * P2 + i] : 0.0;
  }
  __syncthreads();
  const int k0 = (int)((long long)P2 * g / 4), k1 = (int)((long long)P2 * (g + 1) / 4);
  double a0 = 0.0, a1 = 0.0;
  if (r < R) {
#pragma unroll 8
    for (int k = k0; k < k1; ++k) {
      const double w = xv.segT[(size_t)k * R + r];
      a0 = fma(w, xv_sm[k], a0);
      a1 = fma(w, xv_sm[P2 + k], a1);
    }
  }
  __syncthreads();   // the statistics are read: the shares take their place
  xv_sm[(g * XV_SEG_UB + 0) * 64 + rl] = a0;
  xv_sm[(g * XV_SEG_UB + 1) * 64 + rl] = a1;
  __syncthreads();
  if (g == 0 && r < R) {
    const double bias = xv.seg_bias[r];
#pragma unroll
    for (int u = 0; u < XV_SEG_UB; ++u)
      if (b0 + u < B) {
        const double v = ((xv_sm[(0 * XV_SEG_UB + u) * 64 + rl] + xv_sm[(1 * XV_SEG_UB + u) * 64 + rl]) +
                          xv_sm[(2 * XV_SEG_UB + u) * 64 + rl]) + xv_sm[(3 * XV_SEG_UB + u) * 64 + rl];
        emb[(size_t)(b0 + u) * R + r] = v + bias;
      }
  }
}
void fb_launch_xv_segment(hipStream_t s, const FbXvDev &xv, const double *stats, int B, double *emb) {
  size_t doubles = (size_t)XV_SEG_UB * 2 * xv.P;
  if (doubles < 4 * XV_SEG_UB * 64) doubles = 4 * XV_SEG_UB * 64;
  hipLaunchKernelGGL(k_xv_segment, dim3((B + XV_SEG_UB - 1) / XV_SEG_UB, (xv.R + 63) / 64), dim3(256), sizeof(double) * doubles, s,
                     xv, stats, B, emb);
}
