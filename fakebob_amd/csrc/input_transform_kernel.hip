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
//
// RND (the second instantiation): the chain holds an FB_TF_NOISE stage, or the batch is replicated for an
// expectation-over-transformation attack (fb_set_eot, r > 1).  The tile is loaded ONCE into a third LDS buffer and the
// chain runs r times from it, replica j into row u * r + j of the output, its noise stages drawing from replica j's
// stream (the "Noise RNG contract" of fakebob_hip.h).  A sample's normal depends on its absolute index only, so the halo
// positions two neighbouring workgroups both compute get the same value.  An SNR stage scales by the utterance's power,
// which k_tf_power -- the launch in front -- summed: nothing is exchanged inside a kernel here either.  The instantiation
// without RND is the kernel as it was: a chain without noise and without replication runs the same code as before.
// With rn.pre set (the over-the-air channel, air_channel_kernel.hip, has written the replicas already) the RND form runs
// the chain once per input row and only the two indices a noise stage draws with are taken from the row's number.
#include "fb_device.h"
#include "fb_kernels.h"
#include "input_transform_device.h"

#define TF_THREADS 256
#define TF_PAD 4  // int16 behind each LDS buffer, kept zero: the FIR's groups of four outputs read up to 3 past the region

// The composed read of fb_set_companions (CMP; the "Composition" paragraph of fakebob_hip.h): sample i of utterance c of NES
// row b, whose int16 samples q start at `q`.  Utterance 0 is q itself; a companion takes the attacker's int16 difference
// q - a0 on top of its own samples, int32 arithmetic, clipped before the chain sees it.
static __device__ __forceinline__ int16_t tf_composed(const FbTfComp &cn, const int16_t *__restrict__ q, int c, int64_t i) {
  const int v = q[i];
  if (c == 0) return (int16_t)v;
  return (int16_t)tf_clip16((int)cn.comp[(int64_t)(c - 1) * cn.N + i] + v - (int)cn.a0[i]);
}

// The body of k_input_transform (RND as described above) and of k_input_transform_cmp (CMP, which implies RND): with
// companions the workgroup of (NES row u, tile) writes cn.K * rn.r replicas -- replica rho = c * rn.r + j is the chain's
// draw j over utterance c as composed for this row.  The composed tile and its halo are formed once per utterance c, into
// the buffer the replicas are run from: three int16 streams per sample, not per tap.
template <bool RND, bool CMP>
static __device__ __forceinline__ void tf_tile(int16_t *tf_lds, const FbTfChain &ch, const double *__restrict__ taps,
                                               const int16_t *__restrict__ wav, const int64_t *__restrict__ wav_off,
                                               int16_t *__restrict__ out, const int *__restrict__ stop,
                                               const int64_t *__restrict__ out_off, const FbTfRnd &rn, const FbTfComp &cn) {
  if (stop && *stop) return;
  const int u = blockIdx.y;
  const int64_t base = wav_off[u];
  const int64_t n = wav_off[u + 1] - base;
  const int64_t t0 = (int64_t)blockIdx.x * FB_TF_TILE;
  if (t0 >= n) return;  // (the grid is sized for the longest utterance of the batch)
  const int H = ch.H, W = FB_TF_TILE + 2 * H;
  int16_t *a = tf_lds, *b = tf_lds + W + TF_PAD;
  int16_t *const src = RND ? tf_lds + 2 * (W + TF_PAD) : a;  // RND: the tile as loaded, kept for every replica
  const int tid = threadIdx.x;
  // LDS position p of either buffer <-> sample g0 + p of the utterance
  const int64_t g0 = t0 - H;
  for (int p = tid; p < W + TF_PAD; p += TF_THREADS) {
    const int64_t i = g0 + p;
    if (!CMP) src[p] = (p < W && i >= 0 && i < n) ? wav[base + i] : (int16_t)0;
    if (p >= W) {
      if (CMP) src[p] = 0;
      b[p] = 0;
      if (RND) a[p] = 0;
    }
  }
  __syncthreads();
  const int reps = CMP ? cn.K * rn.r : (RND ? (rn.pre ? 1 : rn.r) : 1);
  for (int rep = 0; rep < reps; ++rep) {
  if (CMP && rep % rn.r == 0) {  // the next utterance (the replica before it has left the buffers: the barrier at the loop's end)
    const int c = rep / rn.r;
    for (int p = tid; p < W; p += TF_THREADS) {
      const int64_t i = g0 + p;
      src[p] = (i >= 0 && i < n) ? tf_composed(cn, wav + base, c, i) : (int16_t)0;
    }
    __syncthreads();
  }
  if (RND) {
    a = src;
    b = tf_lds;  // the first stage reads src and writes the first working buffer
  }
  int lo = 0, hi = W;  // positions [lo, hi) of `a` hold the signal after the stages run so far
  for (int s = 0; s < ch.n; ++s) {
    const int kind = ch.kind[s], k = ch.k[s];
    if (RND && kind == FB_TF_NOISE) {
      const double sc = tf_noise_scale(k, taps[ch.tap_off[s]], k ? rn.power[CMP ? u * cn.K + rep / rn.r : u] : 0ull, n);
      // a lane owns the four samples of one Philox call: groups of four by ABSOLUTE index (i >> 2), whatever the tile
      const int64_t i_first = ((g0 + lo) >> 2) << 2;  // (arithmetic shift: rounds toward -inf for the halo in front of sample 0)
      for (int64_t i4 = i_first + 4 * tid; i4 < g0 + hi; i4 += 4 * TF_THREADS) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        // (rn.pre: the over-the-air channel wrote the replicas -- row u is replica u % pre of utterance row u / pre)
        if (i4 + 3 >= 0 && i4 < n)
          tf_noise4(rn, (uint32_t)(!CMP && rn.pre ? u / rn.pre : u), s, !CMP && rn.pre ? u % rn.pre : rep, (uint32_t)(i4 >> 2), z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t i = i4 + q;
          const int p = (int)(i - g0);
          if (p >= lo && p < hi) {
            int y = 0;
            if (i >= 0 && i < n) {
              const double v = __dadd_rn((double)a[p], __dmul_rn(sc, (double)z[q]));
              y = (int)fmin(fmax(rint(v), -32768.0), 32767.0);
            }
            b[p] = (int16_t)y;
          }
        }
      }
    } else if (kind == FB_TF_FIR) {
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
    if (RND && s == 0) {  // src stays as loaded: from here on the two working buffers alternate
      a = b;
      b = tf_lds + ((a == tf_lds) ? W + TF_PAD : 0);
    } else {
      int16_t *t = a;
      a = b;
      b = t;
    }
  }
  // lo == H, hi == H + FB_TF_TILE: the tile
  const int64_t obase = RND ? out_off[(int64_t)u * reps + rep] : base;
  for (int p = H + tid; p < H + FB_TF_TILE; p += TF_THREADS) {
    const int64_t i = g0 + p;
    if (i < n) out[obase + i] = a[p];
  }
  if (RND && rep + 1 < reps) __syncthreads();  // the next replica overwrites the buffers this one's result is read from
  }
}

template <bool RND>
__global__ __launch_bounds__(TF_THREADS) void k_input_transform(FbTfChain ch, const double *__restrict__ taps,
                                                                const int16_t *__restrict__ wav,
                                                                const int64_t *__restrict__ wav_off,
                                                                int16_t *__restrict__ out, const int *__restrict__ stop,
                                                                const int64_t *__restrict__ out_off, FbTfRnd rn) {
  extern __shared__ int16_t tf_lds[];
  tf_tile<RND, false>(tf_lds, ch, taps, wav, wav_off, out, stop, out_off, rn, FbTfComp{});
}

// fb_set_companions: the replicating launch over the composed utterances (rows of cn.N samples each, checked on the host)
__global__ __launch_bounds__(TF_THREADS) void k_input_transform_cmp(FbTfChain ch, const double *__restrict__ taps,
                                                                    const int16_t *__restrict__ wav,
                                                                    const int64_t *__restrict__ wav_off,
                                                                    int16_t *__restrict__ out, const int *__restrict__ stop,
                                                                    const int64_t *__restrict__ out_off, FbTfRnd rn, FbTfComp cn) {
  extern __shared__ int16_t tf_lds[];
  tf_tile<true, true>(tf_lds, ch, taps, wav, wav_off, out, stop, out_off, rn, cn);
}

// E_u of the noise stage's SNR mode: the exact integer sum of squares of every utterance as it is handed to the chain.
// One workgroup per (utterance, tile); 64-bit partial sums, one integer atomic per workgroup into the utterance's word
// (zeroed by the launcher): integer addition is associative, so the result does not depend on the order.  Its only
// reader is the next launch.
__global__ __launch_bounds__(TF_THREADS) void k_tf_power(const int16_t *__restrict__ wav, const int64_t *__restrict__ wav_off,
                                                         unsigned long long *__restrict__ power, const int *__restrict__ stop) {
  if (stop && *stop) return;
  const int u = blockIdx.y;
  const int64_t base = wav_off[u];
  const int64_t n = wav_off[u + 1] - base;
  const int64_t t0 = (int64_t)blockIdx.x * FB_TF_TILE;
  if (t0 >= n) return;
  const int64_t t1 = t0 + FB_TF_TILE < n ? t0 + FB_TF_TILE : n;
  unsigned long long acc = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += TF_THREADS) {
    const int v = wav[base + i];
    acc += (unsigned long long)(v * v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  __shared__ unsigned long long s_part[TF_THREADS / 64];
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < TF_THREADS / 64; ++w) t += s_part[w];
    atomicAdd(power + u, t);
  }
}

// ... with companions: one E per (NES row b, utterance c), word b * K + c, of the row as composed -- what the chain is handed
__global__ __launch_bounds__(TF_THREADS) void k_tf_power_cmp(const int16_t *__restrict__ wav, const int64_t *__restrict__ wav_off,
                                                             unsigned long long *__restrict__ power, const int *__restrict__ stop,
                                                             FbTfComp cn) {
  if (stop && *stop) return;
  const int b = blockIdx.y / cn.K, c = blockIdx.y % cn.K;
  const int64_t base = wav_off[b];
  const int64_t n = wav_off[b + 1] - base;
  const int64_t t0 = (int64_t)blockIdx.x * FB_TF_TILE;
  if (t0 >= n) return;
  const int64_t t1 = t0 + FB_TF_TILE < n ? t0 + FB_TF_TILE : n;
  unsigned long long acc = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += TF_THREADS) {
    const int v = tf_composed(cn, wav + base, c, i);
    acc += (unsigned long long)(v * v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  __shared__ unsigned long long s_part[TF_THREADS / 64];
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < TF_THREADS / 64; ++w) t += s_part[w];
    atomicAdd(power + blockIdx.y, t);
  }
}

// the normals of one (utterance, replica, stage) of the noise contract: z[n] for samples i0 .. i0 + n - 1 (fb_debug_tf_noise)
__global__ __launch_bounds__(256) void k_tf_noise(FbTfRnd rn, int replica, int stage, int64_t i0, int64_t n, float *__restrict__ z) {
  const int64_t q0 = i0 >> 2;
  const int64_t q = q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * q >= i0 + n) return;
  float v[4];
  tf_noise4(rn, 0u, stage, replica, (uint32_t)q, v);
  for (int k = 0; k < 4; ++k) {
    const int64_t i = 4 * q + k;
    if (i >= i0 && i < i0 + n) z[i - i0] = v[k];
  }
}
void fb_launch_tf_noise(hipStream_t s, const FbTfRnd &rn, int replica, int stage, int64_t i0, int64_t n, float *z) {
  const int64_t quads = ((i0 + n + 3) >> 2) - (i0 >> 2);
  hipLaunchKernelGGL(k_tf_noise, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, rn, replica, stage, i0, n, z);
}

size_t fb_input_transform_lds_bytes(const FbTfChain &ch, bool rnd) {
  return sizeof(int16_t) * (rnd ? 3 : 2) * (size_t)(FB_TF_TILE + 2 * ch.H + TF_PAD);
}

void fb_launch_input_transform(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                               const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  hipLaunchKernelGGL(k_input_transform<false>, dim3(tiles > 0 ? tiles : 1, B), dim3(TF_THREADS), fb_input_transform_lds_bytes(ch, false), s,
                     ch, taps, wav, wav_off, out, stop, nullptr, FbTfRnd{});
}

hipError_t fb_launch_tf_power(hipStream_t s, const int16_t *wav, const int64_t *wav_off, int B, int64_t n_max,
                              unsigned long long *power, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  const hipError_t er = hipMemsetAsync(power, 0, sizeof(unsigned long long) * (size_t)B, s);
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(k_tf_power, dim3(tiles > 0 ? tiles : 1, B), dim3(TF_THREADS), 0, s, wav, wav_off, power, stop);
  return hipSuccess;
}

void fb_launch_input_transform_rnd(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                                   const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int64_t *out_off,
                                   const FbTfRnd &rn, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  hipLaunchKernelGGL(k_input_transform<true>, dim3(tiles > 0 ? tiles : 1, B), dim3(TF_THREADS), fb_input_transform_lds_bytes(ch, true), s,
                     ch, taps, wav, wav_off, out, stop, out_off, rn);
}

hipError_t fb_launch_tf_power_cmp(hipStream_t s, const int16_t *wav, const int64_t *wav_off, int B, int64_t n_max,
                                  unsigned long long *power, const FbTfComp &cn, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  const hipError_t er = hipMemsetAsync(power, 0, sizeof(unsigned long long) * (size_t)B * cn.K, s);
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(k_tf_power_cmp, dim3(tiles > 0 ? tiles : 1, B * cn.K), dim3(TF_THREADS), 0, s, wav, wav_off, power, stop, cn);
  return hipSuccess;
}

void fb_launch_input_transform_cmp(hipStream_t s, const FbTfChain &ch, const double *taps, const int16_t *wav,
                                   const int64_t *wav_off, int B, int64_t n_max, int16_t *out, const int64_t *out_off,
                                   const FbTfRnd &rn, const FbTfComp &cn, const int *stop) {
  const unsigned tiles = (unsigned)((n_max + FB_TF_TILE - 1) / FB_TF_TILE);
  hipLaunchKernelGGL(k_input_transform_cmp, dim3(tiles > 0 ? tiles : 1, B), dim3(TF_THREADS), fb_input_transform_lds_bytes(ch, true), s,
                     ch, taps, wav, wav_off, out, stop, out_off, rn, cn);
}
