// feature_compress_kernel.hip -- feature compression (fb_set_feature_compression; SpeakerGuard's FeCo): k-means over the
// voiced feature rows of every utterance row of a batch, the k = ratio * T cluster centres written in the frames' place.
// The stage contract -- keyed initialisation, float32 distance chains without fused multiply-add, float64 means in ascending
// frame order -- is in include/fakebob_hip.h; everything here follows it to the bit.
//
// One workgroup of 1024 threads = one (replicated) utterance row, from the keys to the centres.  No workgroup reads what
// another one wrote: a workgroup sums the k's of the rows in front of it from the input offsets itself and writes its own
// entry of the new offset table (the last one the total as well), so there is nothing to exchange, nothing to restore behind
// a stopped attack and nothing for the FB_XCH_* build to change.
//
// Fast path (the row, its centres and five ints per frame fit the launch's LDS: an NES row of 300 frames x 72 with up to
// T / 2 centres is 137 KB of gfx950's 160 KB): X with an odd row stride (a lane per frame reads conflict-free), the centres
// with a stride of whole float4 (a wave reads one centre: broadcast), keys / labels / sorted order / counts / starts behind.
// General path (anything longer): the same code with X read from the feature buffer, the centres kept in the output rows
// and the five arrays in a workspace in global memory; correct, not fast.  fc_body is instantiated once per path so that
// the compiler resolves the address spaces.
//   keys     a thread per frame: one Philox call, word t & 3
//   select   rank of (key, t) by counting the smaller pairs; the frames of rank < k, counted in ascending t, are the centres
//   assign   a wave = 64 frames x one group of centres (as many groups as the 16 waves allow), four centres per pass over
//            the dimensions; per group the first smallest distance, then the groups in ascending order: the lowest j wins
//   update   stable counting sort of the frames by label (counts by integer atomics, positions by counting the earlier
//            frames of the same label), then a thread per (centre, dimension) adds its members in ascending t in float64
// The loop stops early once an iteration changes no assignment (the contract allows it: the centres are a function of
// the assignment).
// White-box calls (fb_set_wb_frontend) ask the kernel to keep that final assignment -- labels, member counts, k -- and
// k_wb_feco_t, below, is the stage transposed at it.
#include "fb_device.h"
#include "fb_kernels.h"

#define FC_THREADS 1024
#define FC_WAVES (FC_THREADS / 64)
#define FC_JB 4  // centres a lane scores per pass over its frame's dimensions
// dynamic LDS a launch may ask for: 160 KB less the static arrays below
#define FC_LDS_MAX (160 * 1024 - 2 * 4 * FC_THREADS - 256)

static __host__ __device__ __forceinline__ int fc_k(int T, double ratio) {
  if (T <= 0) return 0;
#ifdef __HIP_DEVICE_COMPILE__
  const int k = (int)floor(__dmul_rn((double)T, ratio));
#else
  const int k = (int)floor((double)T * ratio);
#endif
  return k < 1 ? 1 : k;
}
static __host__ __device__ __forceinline__ int fc_xs(int D) { return D | 1; }
static __host__ __device__ __forceinline__ int fc_cs(int D) { return (D + 3) & ~3; }
static __host__ __device__ __forceinline__ size_t fc_lds_bytes(int T, int k, int D) {
  return sizeof(float) * ((size_t)k * fc_cs(D) + (size_t)T * fc_xs(D) + (size_t)FB_FECO_WS_INTS * T);
}

static __device__ __forceinline__ uint32_t fc_key(const FbFeco &fc, uint32_t utt, int replica, uint32_t t) {
  uint32_t r[4];
  fb_philox4x32_10(t >> 2, 0x100u + (uint32_t)replica, utt, fc.epoch, fc.k0, fc.k1, r);
  const uint32_t w = t & 3u;
  return w == 0 ? r[0] : (w == 1 ? r[1] : (w == 2 ? r[2] : r[3]));
}

// one dimension of the contract's chain: diff = x - c, sq = diff * diff, acc = acc + sq, each rounded to float32
static __device__ __forceinline__ float fc_step(float acc, float x, float c) {
  const float diff = __fsub_rn(x, c);
  return __fadd_rn(acc, __fmul_rn(diff, diff));
}

// X[T][xs], C[k][cs] (the centres; written here), aux: FB_FECO_WS_INTS * T ints.  LDS: X, C and aux live in LDS (C rows 16-byte
// aligned, cs a multiple of 4).  s_bd / s_bj: FC_THREADS entries each, s_changed: one int (all static LDS)
template <bool LDS>
static __device__ __forceinline__ void fc_body(const FbFeco &fc, uint32_t utt, int replica, const float *X, int xs, float *C,
                                               int cs, int *aux, int T, int k, int D, float *s_bd, int *s_bj, int *s_changed) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t *key = reinterpret_cast<uint32_t *>(aux);
  int *label = aux + T, *order = aux + 2 * (size_t)T, *cnt = aux + 3 * (size_t)T, *start = aux + 4 * (size_t)T;
  for (int t = tid; t < T; t += FC_THREADS) {
    key[t] = fc_key(fc, utt, replica, (uint32_t)t);
    label[t] = -1;
  }
  __syncthreads();
  // the k frames of smallest (key, t): cnt[t] = 1 for a chosen frame
  for (int t = tid; t < T; t += FC_THREADS) {
    const uint32_t kt = key[t];
    int rank = 0;
    for (int u = 0; u < T; ++u) {
      const uint32_t ku = key[u];
      rank += (ku < kt || (ku == kt && u < t)) ? 1 : 0;
    }
    cnt[t] = rank < k ? 1 : 0;
  }
  __syncthreads();
  // ... in ascending t: order[j] = the frame that starts centre j
  for (int t = tid; t < T; t += FC_THREADS) {
    if (!cnt[t]) continue;
    int j = 0;
    for (int u = 0; u < t; ++u) j += cnt[u];
    order[j] = t;
  }
  __syncthreads();
  for (long long i = tid; i < (long long)k * D; i += FC_THREADS) {
    const int j = (int)(i / D), d = (int)(i - (long long)j * D);
    C[(size_t)j * cs + d] = X[(size_t)order[j] * xs + d];
  }
  __syncthreads();

  const int n_fb = (T + 63) / 64;  // blocks of 64 frames
  int G = FC_WAVES / n_fb;         // groups the centres split into: G * n_fb <= FC_WAVES, so G * n_fb * 64 <= FC_THREADS entries of s_bd / s_bj
  if (G < 1) G = 1;
  if (G > k) G = k;
  for (int it = 0; it < fc.iters; ++it) {
    if (tid == 0) *s_changed = 0;
    __syncthreads();
    // ---- assign
    for (int item = wave; item < n_fb * G; item += FC_WAVES) {
      const int fbk = item % n_fb, g = item / n_fb;
      const int t = fbk * 64 + lane;
      const float *xr = X + (size_t)(t < T ? t : T - 1) * xs;
      const int j0 = (int)((long long)g * k / G), j1 = (int)((long long)(g + 1) * k / G);
      float best = INFINITY;
      int bj = j0;
      for (int j = j0; j < j1; j += FC_JB) {
        // (a group that ends inside the four: the last centre again, its distances ignored below)
        const float *c0 = C + (size_t)j * cs, *c1 = C + (size_t)(j + 1 < j1 ? j + 1 : j1 - 1) * cs,
                    *c2 = C + (size_t)(j + 2 < j1 ? j + 2 : j1 - 1) * cs, *c3 = C + (size_t)(j + 3 < j1 ? j + 3 : j1 - 1) * cs;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int d = 0;
        if (LDS) {
          for (; d + 4 <= D; d += 4) {
            const float4 v0 = *reinterpret_cast<const float4 *>(c0 + d), v1 = *reinterpret_cast<const float4 *>(c1 + d),
                         v2 = *reinterpret_cast<const float4 *>(c2 + d), v3 = *reinterpret_cast<const float4 *>(c3 + d);
            const float x0 = xr[d], x1 = xr[d + 1], x2 = xr[d + 2], x3 = xr[d + 3];
            a0 = fc_step(a0, x0, v0.x); a1 = fc_step(a1, x0, v1.x); a2 = fc_step(a2, x0, v2.x); a3 = fc_step(a3, x0, v3.x);
            a0 = fc_step(a0, x1, v0.y); a1 = fc_step(a1, x1, v1.y); a2 = fc_step(a2, x1, v2.y); a3 = fc_step(a3, x1, v3.y);
            a0 = fc_step(a0, x2, v0.z); a1 = fc_step(a1, x2, v1.z); a2 = fc_step(a2, x2, v2.z); a3 = fc_step(a3, x2, v3.z);
            a0 = fc_step(a0, x3, v0.w); a1 = fc_step(a1, x3, v1.w); a2 = fc_step(a2, x3, v2.w); a3 = fc_step(a3, x3, v3.w);
          }
        }
        for (; d < D; ++d) {
          const float x = xr[d];
          a0 = fc_step(a0, x, c0[d]); a1 = fc_step(a1, x, c1[d]); a2 = fc_step(a2, x, c2[d]); a3 = fc_step(a3, x, c3[d]);
        }
        if (a0 < best) { best = a0; bj = j; }
        if (j + 1 < j1 && a1 < best) { best = a1; bj = j + 1; }
        if (j + 2 < j1 && a2 < best) { best = a2; bj = j + 2; }
        if (j + 3 < j1 && a3 < best) { best = a3; bj = j + 3; }
      }
      if (G == 1) {
        if (t < T) {
          if (label[t] != bj) { label[t] = bj; *s_changed = 1; }
        }
      } else {
        s_bd[(g * n_fb + fbk) * 64 + lane] = best;
        s_bj[(g * n_fb + fbk) * 64 + lane] = bj;
      }
    }
    __syncthreads();
    if (G > 1) {  // (T <= 64 * FC_WAVES / 2 then: one pass)
      for (int t = tid; t < T; t += FC_THREADS) {
        float best = s_bd[t];
        int bj = s_bj[t];
        for (int g = 1; g < G; ++g) {
          const float v = s_bd[g * n_fb * 64 + t];
          if (v < best) { best = v; bj = s_bj[g * n_fb * 64 + t]; }
        }
        if (label[t] != bj) { label[t] = bj; *s_changed = 1; }
      }
      __syncthreads();
    }
    if (it > 0 && *s_changed == 0) break;  // (uniform: every thread reads the word behind the barrier)
    // ---- update: stable counting sort by label ...
    for (int j = tid; j < k; j += FC_THREADS) cnt[j] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += FC_THREADS) atomicAdd(&cnt[label[t]], 1);
    __syncthreads();
    for (int j = tid; j < k; j += FC_THREADS) {
      int sum = 0;
      for (int u = 0; u < j; ++u) sum += cnt[u];
      start[j] = sum;
    }
    __syncthreads();
    for (int t = tid; t < T; t += FC_THREADS) {
      const int l = label[t];
      int pos = 0;
      for (int u = 0; u < t; ++u) pos += label[u] == l ? 1 : 0;
      order[start[l] + pos] = t;
    }
    __syncthreads();
    // ... then the float64 means, members in ascending t
    for (long long i = tid; i < (long long)k * D; i += FC_THREADS) {
      const int j = (int)(i / D), d = (int)(i - (long long)j * D);
      const int n = cnt[j];
      if (n == 0) continue;  // an empty cluster keeps its centre
      const int *m = order + start[j];
      double S = 0.0;
      for (int q = 0; q < n; ++q) S = __dadd_rn(S, (double)X[(size_t)m[q] * xs + d]);
      C[(size_t)j * cs + d] = (float)__ddiv_rn(S, (double)n);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(FC_THREADS) void k_feature_compress(FbFeco fc, int D, const float *__restrict__ feats,
                                                                  const int *__restrict__ row_off, int rows,
                                                                  float *__restrict__ out, int *__restrict__ out_off,
                                                                  int *__restrict__ ws, int lds_bytes,
                                                                  const int *__restrict__ stop, int *__restrict__ keep_label,
                                                                  int *__restrict__ keep_cnt, int *__restrict__ keep_k) {
  extern __shared__ __attribute__((aligned(16))) float fc_lds[];
  __shared__ float s_bd[FC_THREADS];
  __shared__ int s_bj[FC_THREADS];
  __shared__ int s_part[FC_WAVES];
  __shared__ int s_changed;
  if (stop && *stop) return;
  const int u = blockIdx.x, tid = threadIdx.x;
  // this row's place in the output: the k's of the rows in front of it
  int part = 0;
  for (int v = tid; v < u; v += FC_THREADS) part += fc_k(row_off[v + 1] - row_off[v], fc.ratio);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = part;
  __syncthreads();
  int o_off = 0;
  for (int w = 0; w < FC_WAVES; ++w) o_off += s_part[w];
  const int i_off = row_off[u];
  const int T = row_off[u + 1] - i_off;
  const int k = fc_k(T, fc.ratio);
  if (tid == 0) {
    out_off[u] = o_off;
    if (u == rows - 1) out_off[rows] = o_off + k;
    if (keep_k) keep_k[u] = k;
  }
  if (T <= 0) return;
  const float *X = feats + (size_t)i_off * D;
  float *O = out + (size_t)o_off * D;
  const uint32_t utt = fc.utt0 + (uint32_t)(u / fc.r);
  const int replica = u % fc.r;
  const int *aux_end;  // the five arrays as fc_body left them: labels at T, counts at 3 T
  if (fc_lds_bytes(T, k, D) <= (size_t)lds_bytes) {
    const int xs = fc_xs(D), cs = fc_cs(D);
    float *Cl = fc_lds, *Xl = fc_lds + (size_t)k * cs;
    int *aux = reinterpret_cast<int *>(Xl + (size_t)T * xs);
    for (long long i = tid; i < (long long)T * D; i += FC_THREADS) {
      const int t = (int)(i / D), d = (int)(i - (long long)t * D);
      Xl[(size_t)t * xs + d] = X[i];
    }
    __syncthreads();
    fc_body<true>(fc, utt, replica, Xl, xs, Cl, cs, aux, T, k, D, s_bd, s_bj, &s_changed);
    __syncthreads();
    for (long long i = tid; i < (long long)k * D; i += FC_THREADS) {
      const int j = (int)(i / D), d = (int)(i - (long long)j * D);
      O[i] = Cl[(size_t)j * cs + d];
    }
    aux_end = aux;
  } else {
    int *aux = ws + (size_t)FB_FECO_WS_INTS * i_off;
    fc_body<false>(fc, utt, replica, X, D, O, D, aux, T, k, D, s_bd, s_bj, &s_changed);
    __syncthreads();
    aux_end = aux;
  }
  // the assignment the centres were last written under (after the last update, or at the early break, where it is the one
  // that update used) and its member counts, kept for the white-box backward: label of input row i_off + t, count of
  // centre o_off + j
  if (keep_label)
    for (int t = tid; t < T; t += FC_THREADS) keep_label[(size_t)i_off + t] = aux_end[(size_t)T + t];
  if (keep_cnt)
    for (int j = tid; j < k; j += FC_THREADS) keep_cnt[(size_t)o_off + j] = aux_end[3 * (size_t)T + j];
}

// The k-means stage transposed at a constant assignment (fb_set_wb_frontend; "White-box gradients through the front end" in
// include/fakebob_hip.h): a centre with members is their mean, so frame t of row R receives its centre's cotangent divided by
// the member count -- xbar[t][d] = cbar[label[t]][d] / (double) n_label[t], one correctly rounded division, no sum at all; a
// centre without members kept an earlier value and its cotangent is read by nobody.  One thread per (frame, dimension) of row
// row0 + blockIdx.y; offsets and counts are read here.  packed: cbar / xbar hold every row (at out_off / in_off); else they
// hold the one row alone, from 0.
__global__ __launch_bounds__(256) void k_wb_feco_t(int D, const int *__restrict__ label, const int *__restrict__ cnt,
                                                   const int *__restrict__ in_off, const int *__restrict__ out_off, int row0,
                                                   int packed, const double *__restrict__ cbar, double *__restrict__ xbar,
                                                   const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int R = row0 + blockIdx.y;
  const int i_off = in_off[R], T = in_off[R + 1] - i_off, o_off = out_off[R], k = out_off[R + 1] - o_off;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)T * D) return;
  const int t = (int)(i / D), d = (int)(i - (long long)t * D);
  const int l = label[(size_t)i_off + t];
  if (l < 0 || l >= k) return;  // (never: every frame of a row with T > 0 is assigned)
  const double c = cbar[((size_t)(packed ? o_off : 0) + l) * D + d];
  xbar[((size_t)(packed ? i_off : 0) + t) * D + d] = __ddiv_rn(c, (double)cnt[(size_t)o_off + l]);
}
void fb_launch_wb_feco_t(hipStream_t s, int D, const int *label, const int *cnt, const int *in_off, const int *out_off, int row0,
                         int rows, int t_max, bool packed, const double *cbar, double *xbar, const int *stop) {
  if (rows <= 0 || t_max <= 0) return;
  hipLaunchKernelGGL(k_wb_feco_t, dim3((unsigned)(((size_t)t_max * D + 255) / 256), (unsigned)rows), dim3(256), 0, s, D, label, cnt,
                     in_off, out_off, row0, packed ? 1 : 0, cbar, xbar, stop);
}

__global__ __launch_bounds__(256) void k_feco_keys(FbFeco fc, int replica, int T, uint32_t *__restrict__ keys) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T) keys[t] = fc_key(fc, fc.utt0, replica, (uint32_t)t);
}
void fb_launch_feco_keys(hipStream_t s, const FbFeco &fc, int replica, int T, uint32_t *keys) {
  hipLaunchKernelGGL(k_feco_keys, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, fc, replica, T, keys);
}

bool fb_launch_feature_compress(hipStream_t s, const FbFeco &fc, int D, const float *feats, const int *row_off, int rows,
                                int t_max, float *out, int *out_off, int *ws, const int *stop, int *keep_label, int *keep_cnt,
                                int *keep_k) {
  if (rows <= 0) return true;
  // the LDS the longest row could need (k grows with T), capped: rows beyond it take the general path
  size_t shm = fc_lds_bytes(t_max, fc_k(t_max, fc.ratio), D);
  if (shm > (size_t)FC_LDS_MAX) shm = FC_LDS_MAX;
  if (shm > 64 * 1024) {
    static std::atomic<unsigned long long> optin{0};  // raise the dynamic-LDS limit once per device
    unsigned long long bit = 0;
    if (fb_device_needs_optin(optin, &bit)) {
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_feature_compress), hipFuncAttributeMaxDynamicSharedMemorySize,
                              FC_LDS_MAX) != hipSuccess)
        return false;
      optin.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(k_feature_compress, dim3((unsigned)rows), dim3(FC_THREADS), shm, s, fc, D, feats, row_off, rows, out,
                     out_off, ws, (int)shm, stop, keep_label, keep_cnt, keep_k);
  return true;
}
