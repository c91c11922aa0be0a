// whitebox_xv_kernels.hip -- the x-vector (TDNN) system's backward, from the cotangent on an embedding to the cotangent on the
// feature rows (fb_set_wb_xvector; the x-vector part of the "white-box gradients" section of fakebob_hip.h):
//   k_wb_xv_segment_t   sbar = seg_W' ebar, float64
//   k_wb_xv_pool_t      the pooling rule: the float32 cotangent on the last frame layer's output
//   k_wb_xv_act_t       zbar = ybar * bn_scale * mask with the forward's own ReLU decisions, and max |zbar| of every row
//   k_wb_xv_affine_t    G = zbar W on the matrix cores: k_xv_affine's tiling and operand path against the transposed image,
//                       no splice, a plain epilogue
//   k_wb_xv_unsplice    the splice transposed: a replicated edge row collects every place that read it, float64 sums
// As in the forward, every result is a function of the utterance's own rows and the layer's shape: no atomics, no order that
// depends on the batch.
#include "gmm_split.h"

#define WXV_RT 4    // row tiles of 32 rows per workgroup
#define WXV_CT 4    // column tiles of 32 columns per workgroup: one per wave
#define WXV_KS 4    // K steps of 16 per LDS stage
#define WXV_ROWS (32 * WXV_RT)
static_assert(WXV_RT == 4 && WXV_CT == 4, "wave w of four builds row tile w's fragments and owns column tile w");

// One wave per output k of utterance b: lane l takes r = l, l + 64, .. ascending as one fma chain, the lanes are added by a
// butterfly.  segT is [2 P][R]: the wave reads a row of it contiguously.
__global__ __launch_bounds__(256) void k_wb_xv_segment_t(FbXvDev xv, const double *__restrict__ ebar, double *__restrict__ sbar,
                                                         const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int P2 = 2 * xv.P, R = xv.R, b = blockIdx.x, k = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= P2) return;
  const double *w = xv.segT + (size_t)k * R, *eb = ebar + (size_t)b * R;
  double a = 0.0;
  for (int r = lane; r < R; r += 64) a = fma(w[r], eb[r], a);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) sbar[(size_t)b * P2 + k] = a;
}
void fb_launch_wb_xv_segment_t(hipStream_t s, const FbXvDev &xv, const double *ebar, int B, double *sbar, const int *stop) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_wb_xv_segment_t, dim3(B, (2 * xv.P + 3) / 4), dim3(256), 0, s, xv, ebar, sbar, stop);
}

// One workgroup per (utterance, 64 channels), thread (q, c) the rows q, q + 4, ..:
//   ybar[t][c] = f32( mbar[c] / T + sbar[c] (h[t][c] - mean[c]) / (T std[c]) ),  the second term only where the variance floor
// was not active -- std above the floor's own value sqrt(1e-10), which is what k_xv_pool stored for every floored channel.
__global__ __launch_bounds__(256) void k_wb_xv_pool_t(const float *__restrict__ h, int P, const int *__restrict__ row_off,
                                                      const double *__restrict__ stats, const double *__restrict__ sbar,
                                                      float *__restrict__ ybar, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  if (c >= P) return;
  const int r0 = row_off[b], T = row_off[b + 1] - r0;
  if (T <= 0) return;
  const double mean = stats[(size_t)b * 2 * P + c], sd = stats[(size_t)b * 2 * P + P + c];
  const double mbar = sbar[(size_t)b * 2 * P + c], sb = sbar[(size_t)b * 2 * P + P + c];
  const double dT = (double)T, m_part = mbar / dT;
  const bool live = sd > sqrt(1.0e-10);
  const double den = dT * sd;
  for (int t = q; t < T; t += 4) {
    const size_t i = (size_t)(r0 + t) * P + c;
    double v = m_part;
    if (live) v += sb * ((double)h[i] - mean) / den;
    ybar[i] = (float)v;
  }
}
void fb_launch_wb_xv_pool_t(hipStream_t s, const float *h, int P, const int *row_off, int B, const double *stats, const double *sbar,
                            float *ybar, const int *stop) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_wb_xv_pool_t, dim3(B, (P + 63) / 64), dim3(256), 0, s, h, P, row_off, stats, sbar, ybar, stop);
}

// one wave per row: zbar = mask ? ybar * scale : 0 (one rounding), amax[row] = max |zbar|
__global__ __launch_bounds__(256) void k_wb_xv_act_t(const float *__restrict__ ybar, const unsigned char *__restrict__ mask,
                                                     const float *__restrict__ scale, int dout, const int *__restrict__ n_rows_ptr,
                                                     float *__restrict__ zbar, float *__restrict__ amax, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= *n_rows_ptr) return;
  const size_t o = (size_t)row * dout;
  float m = 0.0f;
  for (int c = lane; c < dout; c += 64) {
    const float z = mask[o + c] ? __fmul_rn(ybar[o + c], scale[c]) : 0.0f;
    zbar[o + c] = z;
    m = fmaxf(m, fabsf(z));
  }
#pragma unroll
  for (int o2 = 32; o2 >= 1; o2 >>= 1) m = fmaxf(m, __shfl_xor(m, o2, 64));
  if (lane == 0) amax[row] = m;
}
void fb_launch_wb_xv_act_t(hipStream_t s, const FbXvLayerDev &ly, const float *ybar, const unsigned char *mask, const int *n_rows_ptr,
                           int rows_cap, float *zbar, float *amax, const int *stop) {
  if (rows_cap <= 0) return;
  hipLaunchKernelGGL(k_wb_xv_act_t, dim3((rows_cap + 3) / 4), dim3(256), 0, s, ybar, mask, ly.scale, ly.dout, n_rows_ptr, zbar, amax, stop);
}

// G[row][n] = sum_c zbar[row][c] W[c][n], n over the layer's K columns, the contraction over its dout channels.
// k_xv_affine's workgroup: four waves own WXV_ROWS rows x 128 columns, wave w the columns 32 (4 blockIdx.y + w) .. + 31 of all
// its rows.  Per stage of WXV_KS K steps the waves scale their row tile's values by the row's power of two (max |zbar| of the
// row in [2^14, 2^15)), split them into two f16 terms and leave them in LDS in fragment order; then every wave runs hi.hi, hi.lo,
// lo.hi per (K step, row tile) against the transposed image's fragments.  The order of an output element's sum is ascending
// K step, the three products in that order: the layer's shape alone.  Rows past n_rows and channels past dout enter as zeros
// (the image holds zeros there too); columns past K are not stored.
__global__ __launch_bounds__(256) void k_wb_xv_affine_t(FbXvLayerDev ly, const float *__restrict__ zbar, const float *__restrict__ amax,
                                                        const int *__restrict__ n_rows_ptr, float *__restrict__ G,
                                                        const int *__restrict__ stop) {
  __shared__ u32x4 sA[WXV_KS][WXV_RT][2][64];   // 32 KB
  __shared__ int sSh[WXV_ROWS];                 // the row's values are multiplied by 2^-sSh
  if (stop && *stop) return;
  const int n_rows = *n_rows_ptr, row0 = blockIdx.x * WXV_ROWS;
  if (row0 >= n_rows) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int dout = ly.dout, K = ly.K, n_steps = ly.nt_steps;
  if (tid < WXV_ROWS) {
    const int g = row0 + tid;
    int sh = 0;
    if (g < n_rows) {
      const float am = amax[g];
      if (am > 0.0f) sh = (int)((__float_as_uint(am) >> 23) & 0xffu) - 127 - 14;   // am 2^-sh in [2^14, 2^15)
    }
    sSh[tid] = sh;
  }
  __syncthreads();
  const int ct = blockIdx.y * WXV_CT + wave;
  const bool active = ct * 32 < K;
  const u32x4 *wimg = reinterpret_cast<const u32x4 *>(ly.wt) + (size_t)(active ? ct : 0) * n_steps * 2 * 64 + lane;
  f32x16 acc[WXV_RT];
#pragma unroll
  for (int rt = 0; rt < WXV_RT; ++rt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[rt][i] = 0.0f;
  const int m_own = wave * 32 + (lane & 31), g_own = row0 + m_own;   // the row whose fragments this lane builds
  const int sh_own = sSh[m_own];
  const float *zr = zbar + (size_t)(g_own < n_rows ? g_own : 0) * dout;
  for (int c0 = 0; c0 < n_steps; c0 += WXV_KS) {
    const int ns = min(WXV_KS, n_steps - c0);
    for (int s = 0; s < ns; ++s) {
      const int k0 = (c0 + s) * 16 + 8 * (lane >> 5);
      float v[8];
      if ((dout & 7) == 0) {   // (k0 < dout then means k0 + 8 <= dout)
        float4 t0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), t1 = t0;
        if (g_own < n_rows && k0 < dout) {
          const float4 *p = reinterpret_cast<const float4 *>(zr + k0);
          t0 = p[0];
          t1 = p[1];
        }
        v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (g_own < n_rows && k0 + i < dout) ? zr[k0 + i] : 0.0f;
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
        for (int rt = 0; rt < WXV_RT; ++rt) {
          const u32x4 a1 = sA[s][rt][0][lane], a2 = sA[s][rt][1][lane];
          FB_FX_MFMA(a1, b1, acc[rt]);
          FB_FX_MFMA(a1, b2, acc[rt]);
          FB_FX_MFMA(a2, b1, acc[rt]);
        }
      }
    }
    __syncthreads();
  }
  const int n = ct * 32 + (lane & 31);
  if (!active || n >= K) return;
#pragma unroll
  for (int rt = 0; rt < WXV_RT; ++rt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = rt * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3), g = row0 + m;
      if (g < n_rows) G[(size_t)g * K + n] = ldexpf(acc[rt][i], sSh[m] + ly.kwt);
    }
}
void fb_launch_wb_xv_affine_t(hipStream_t s, const FbXvLayerDev &ly, const float *zbar, const float *amax, const int *n_rows_ptr,
                              int rows_cap, float *G, const int *stop) {
  if (rows_cap <= 0) return;
  const dim3 grid((rows_cap + WXV_ROWS - 1) / WXV_ROWS, (ly.K + 32 * WXV_CT - 1) / (32 * WXV_CT));
  hipLaunchKernelGGL(k_wb_xv_affine_t, grid, dim3(256), 0, s, ly, zbar, amax, n_rows_ptr, G, stop);
}

// One thread per (row t' of its utterance, input channel d): context places j ascending, and within a place the rows t that
// read t' ascending -- t' - ctx[j] itself, and at an utterance's first / last row every t whose t + ctx[j] fell outside.  The
// sum is float64, rounded once (layers above 0) or handed on as it is (layer 0, to the front end's backward).
__global__ __launch_bounds__(256) void k_wb_xv_unsplice(FbXvLayerDev ly, const float *__restrict__ G, const int2 *__restrict__ rowinfo,
                                                        const int *__restrict__ row_off, int B, const int *__restrict__ n_rows_ptr,
                                                        float *__restrict__ out32, double *__restrict__ out64, int cap64,
                                                        const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int din = ly.din, K = ly.K;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int g = (int)(e / din), d = (int)(e - (long long)g * din);
  if (g >= *n_rows_ptr) return;
  const int2 info = rowinfo[g];
  const int tp = g - info.x, T = info.y;
  double a = 0.0;
  for (int j = 0; j < ly.n_ctx; ++j) {
    const int c = ly.ctx[j];
    int lo = tp == 0 ? 0 : tp - c, hi = tp == T - 1 ? T - 1 : tp - c;
    lo = max(lo, 0);
    hi = min(hi, T - 1);
    for (int t = lo; t <= hi; ++t)
      if (min(max(t + c, 0), T - 1) == tp) a += (double)G[(size_t)(info.x + t) * K + (size_t)j * din + d];
  }
  if (out64) {
    int b0 = 0, b1 = B;   // the utterance: the last b with row_off[b] <= g (empty utterances share a start with their successor)
    while (b1 - b0 > 1) {
      const int mid = (b0 + b1) >> 1;
      if (row_off[mid] <= g) b0 = mid; else b1 = mid;
    }
    if (tp < cap64) out64[((size_t)b0 * cap64 + tp) * din + d] = a;
  } else {
    out32[(size_t)g * din + d] = (float)a;
  }
}
void fb_launch_wb_xv_unsplice(hipStream_t s, const FbXvLayerDev &ly, const float *G, const int2 *rowinfo, const int *row_off, int B,
                              const int *n_rows_ptr, int rows_cap, float *out32, double *out64, int cap64, const int *stop) {
  if (rows_cap <= 0) return;
  const long long n = (long long)rows_cap * ly.din;
  hipLaunchKernelGGL(k_wb_xv_unsplice, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ly, G, rowinfo, row_off, B, n_rows_ptr, out32,
                     out64, cap64, stop);
}
