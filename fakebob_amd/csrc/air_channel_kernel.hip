// air_channel_kernel.hip -- the over-the-air channel (fb_set_air_channel; the contract is in include/fakebob_hip.h): every
// row the input-transform chain would see is first convolved with a random room impulse response of its own, L <= 4096
// int16 taps in Q14.  Two launches in front of the chain:
//
// k_air_taps   one workgroup per output row (utterance row b, replica rho): the decay's word, the blocked envelope (thread 0:
//              63 + 1 + 63 sequential float64 products), then a lane per Philox call of four normals writes four taps.
// k_air_conv   one workgroup per (output row, chunk of AIR_CHUNK output samples): the convolution as a Toeplitz GEMM on the
//              float64 matrix cores.  With i = 16 a + b:  Y[a][b] = sum_j X[a][j] * H[j][b],  X[a][j] = x[16 a + j],
//              H[j][b] = t[b - j] (zero outside [0, L)),  j = -(L - 1) .. 15 -- L + 15 multiply-adds executed per output
//              for L useful ones.  Every product is an integer below 2^30 and every partial sum one below 2^42 < 2^53, so
//              v_mfma_f64_16x16x4_f64 is exact whatever order it sums in; a 16-bit or f32 matrix instruction would not be.
//              The chunk's samples -- composed on the fly when companions are set, exactly as tf_composed composes them --
//              with HIST >= L - 1 samples of history in front, and the row's taps, sit in LDS as int16 (zeros wherever the
//              index falls outside the utterance or the response) and are widened at the read.  A wave owns AIR_TILES
//              blocks of 16 x 16 outputs; they share one H fragment per K step.
// Nothing is exchanged between workgroups, there are no atomics, every global index is checked against [0, n), and the
// `stop` flag is honoured as the transform kernels honour it.
// k_air_conv is a template on KEEP_SAT: <true>, taken by white-box calls under fb_set_wb_air only, also writes one byte per
// output sample -- saturated before the clip or not -- for the transposed kernel (whitebox_air_kernels.hip); <false> is the
// kernel every other caller takes.
//
// f64 MFMA lane maps (they are not the f32 ones): A -- lane l holds X[row l & 15][k = l >> 4]; B -- H[k = l >> 4][col l & 15];
// C / D -- register g of lane l is Y[row (l >> 4) + 4 g][col l & 15].  So register g of a block holds outputs
// 64 g + l of the block's 256: the stores of a wave are contiguous.
//
// LDS: the samples are swizzled (16 samples take 18 slots) with the aim that the 16 rows of an A fragment, 32 bytes apart,
// fall into different banks (not timed against the plain layout).  At L = 4096: 18.1 KB of samples + 8.1 KB of taps, below the 64 KB that need no opt-in.
//
// The float64 arithmetic of k_air_taps is the contract's "one rounding per written operation, no fused multiply-add".
// __dmul_rn / __dadd_rn do not by themselves keep hipcc from contracting a product into the sum that follows it: the file
// depends on -ffp-contract=off, which build.py passes to every source (as input_transform_kernel.hip does).
#include "fb_device.h"
#include "fb_kernels.h"

#define AIR_THREADS 256
#define AIR_TILES 4                                                // 16 x 16 output blocks per wave
#define AIR_CHUNK ((AIR_THREADS / FB_WAVE) * AIR_TILES * 256)      // output samples per workgroup: 4096

typedef double air_d4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ int air_clip16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// LDS slot of sample position p
static __device__ __forceinline__ int air_xpos(int p) { return p + 2 * (p >> 4); }
// K steps' worth of history: the j range -(L - 1) .. 15 rounded up to whole steps of 4, less the 16 of the tile itself
static __host__ __device__ __forceinline__ int air_hist(int L) { return ((L + 15 + 3) & ~3) - 16; }

// taps[R][L] for output rows R = 0 .. rows - 1: utterance row ac.utt0 + R / ac.r, replica rep0 + R % ac.r.  z (nullable):
// the normals z[R][4 * ceil(L / 4)] as drawn; w (nullable): the decay's word of every row.
__global__ __launch_bounds__(AIR_THREADS) void k_air_taps(FbAir ac, int rep0, int16_t *__restrict__ taps, float *__restrict__ z_out,
                                                          uint32_t *__restrict__ w_out, const int *__restrict__ stop) {
  if (stop && *stop) return;
  __shared__ double s_q[64], s_p[64];
  const int R = blockIdx.x, L = ac.L, d = ac.d;
  const uint32_t utt = ac.utt0 + (uint32_t)(R / ac.r), rep = (uint32_t)(rep0 + R % ac.r);
  if (threadIdx.x == 0) {
    uint32_t r[4];
    fb_philox4x32_10(0xFFFFFFFFu, rep, utt, ac.epoch, ac.k0, ac.k1, r);
    if (w_out) w_out[R] = r[0];
    const double U = __dmul_rn(__dadd_rn((double)r[0], 0.5), 2.3283064365386963e-10);  // 2^-32
    const double rho = fmin(fmax(__dadd_rn(ac.rho_lo, __dmul_rn(U, __dadd_rn(ac.rho_hi, -ac.rho_lo))), ac.rho_lo), ac.rho_hi);
    double q = 1.0;
    s_q[0] = q;
    for (int i = 1; i < 64; ++i) {
      q = __dmul_rn(q, rho);
      s_q[i] = q;
    }
    const double S = __dmul_rn(q, rho);
    double p = 1.0;
    s_p[0] = p;
    for (int j = 1; j < 64; ++j) {
      p = __dmul_rn(p, S);
      s_p[j] = p;
    }
  }
  __syncthreads();
  const int L4 = (L + 3) >> 2;
  for (int c = threadIdx.x; c < L4; c += AIR_THREADS) {
    float z[4];
    uint32_t r[4];
    fb_philox4x32_10((uint32_t)c, rep, utt, ac.epoch, ac.k0, ac.k1, r);
    fb_box_muller_sel(r[0], r[1], z[0], z[1]);
    fb_box_muller_sel(r[2], r[3], z[2], z[3]);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int k = 4 * c + h;
      if (z_out) z_out[(int64_t)R * (4 * L4) + k] = z[h];
      if (k >= L) continue;
      int t = 0;
      if (k == 0) t = 16384;
      else if (k >= d) {
        const int m = k - d;
        const double env = __dmul_rn(s_p[m >> 6], s_q[m & 63]);
        const double v = __dmul_rn(__dmul_rn(ac.amp, (double)z[h]), env);
        t = (int)fmin(fmax(rint(v), -32767.0), 32767.0);
      }
      taps[(int64_t)R * L + k] = (int16_t)t;
    }
  }
}

// out row R (at out_off[R]) = the convolution of input row R / r (in_off) -- with cn.K > 1 utterance (R % r) / eot of that
// row as composed -- with taps[R][L]; r: output rows per input row.  KEEP_SAT (the white-box call under fb_set_wb_air): sat,
// laid out as out, gets one byte per output sample -- 1 where (y + 8192) >> 14 lay outside [-32768, 32767] before the clip;
// the instantiation every other caller takes, <false>, is the kernel as it was and touches no sat
template <bool KEEP_SAT>
__global__ __launch_bounds__(AIR_THREADS) void k_air_conv(const int16_t *__restrict__ wav, const int64_t *__restrict__ in_off, int r, int eot,
                                                          const int16_t *__restrict__ taps, int L, int16_t *__restrict__ out,
                                                          const int64_t *__restrict__ out_off, FbTfComp cn, const int *__restrict__ stop,
                                                          unsigned char *__restrict__ sat) {
  extern __shared__ int16_t air_lds[];
  if (stop && *stop) return;
  const int R = blockIdx.y, u = R / r;
  const int64_t base = in_off[u];
  const int64_t n = in_off[u + 1] - base;
  const int64_t c0 = (int64_t)blockIdx.x * AIR_CHUNK;
  if (c0 >= n) return;  // (the grid is sized for the longest utterance of the batch)
  const int HIST = air_hist(L), NX = HIST + AIR_CHUNK, NT = HIST + 31;
  int16_t *xs = air_lds;                          // slot air_xpos(p) <-> sample c0 - HIST + p of the row, p in [0, NX)
  int16_t *ts = air_lds + ((air_xpos(NX) + 3) & ~3);  // ts[q] = t[q - 15], q in [0, NT)
  const int tid = threadIdx.x;
  const int c = cn.K > 1 ? (R % r) / eot : 0;
  for (int p = tid; p < NX; p += AIR_THREADS) {
    const int64_t i = c0 - HIST + p;
    int v = 0;
    if (i >= 0 && i < n) {
      v = wav[base + i];
      if (c > 0) v = air_clip16((int)cn.comp[(int64_t)(c - 1) * cn.N + i] + v - (int)cn.a0[i]);  // (tf_composed's arithmetic)
    }
    xs[air_xpos(p)] = (int16_t)v;
  }
  for (int q = tid; q < NT; q += AIR_THREADS) {
    const int k = q - 15;
    ts[q] = (k >= 0 && k < L) ? taps[(int64_t)R * L + k] : (int16_t)0;
  }
  __syncthreads();
  const int wv = tid / FB_WAVE, lane = tid % FB_WAVE;
  const int64_t w0 = c0 + (int64_t)wv * (AIR_TILES * 256);  // the wave's first output
  if (w0 >= n) return;
  const int b = lane & 15, kk = lane >> 4;
  air_d4 acc[AIR_TILES];
#pragma unroll
  for (int T = 0; T < AIR_TILES; ++T) acc[T] = air_d4{0.0, 0.0, 0.0, 0.0};
  // K step s covers j = s - HIST + kk: the A operand of block T is sample position wv * 1024 + 256 T + 16 b + s + kk (the
  // HIST of the position and the -HIST of j cancel), the B operand is t[b - j] = ts[b - kk + 15 + HIST - s]
  const int pa = wv * (AIR_TILES * 256) + 16 * b + kk;
  const int qb = b - kk + 15 + HIST;
  // Near the row's start the history is zeros: at step s the wave's A operands are the samples c0 - HIST + p + s, p at most
  // pmax -- the steps at which even that sample lies in front of sample 0 add nothing and are left out (wave-uniform)
  const int pmax = wv * (AIR_TILES * 256) + (AIR_TILES - 1) * 256 + 16 * 15 + 3;
  const long long lead = (long long)HIST - c0 - pmax;  // steps s < lead read zeros only
  const int s0 = lead > 0 ? (int)lead & ~3 : 0;
  for (int s = s0; s < HIST + 16; s += 4) {
    const double hv = (double)ts[qb - s];
#pragma unroll
    for (int T = 0; T < AIR_TILES; ++T) {
      const double xv = (double)xs[air_xpos(pa + 256 * T + s)];
      acc[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, hv, acc[T], 0, 0, 0);
    }
  }
  const int64_t obase = out_off[R];
#pragma unroll
  for (int T = 0; T < AIR_TILES; ++T) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t i = w0 + 256 * T + 64 * g + lane;
      if (i < n) {
        const long long y = (long long)acc[T][g];  // an exact integer, |y| < 2^42
        const long long o = (y + 8192) >> 14;      // (arithmetic shift: floor)
        out[obase + i] = (int16_t)(o < -32768 ? -32768 : (o > 32767 ? 32767 : o));
        if (KEEP_SAT) sat[obase + i] = (o < -32768 || o > 32767) ? 1 : 0;
      }
    }
  }
}

void fb_launch_air_taps(hipStream_t s, const FbAir &ac, int rep0, int rows, int16_t *taps, float *z, uint32_t *w, const int *stop) {
  hipLaunchKernelGGL(k_air_taps, dim3(rows), dim3(AIR_THREADS), 0, s, ac, rep0, taps, z, w, stop);
}

size_t fb_air_conv_lds_bytes(int L) {
  const int HIST = air_hist(L), NX = HIST + AIR_CHUNK;
  return sizeof(int16_t) * (size_t)(((NX + 2 * (NX >> 4) + 3) & ~3) + HIST + 31 + 1);
}

void fb_launch_air_conv(hipStream_t s, const int16_t *wav, const int64_t *in_off, int rows, int r, int eot, int64_t n_max,
                        const int16_t *taps, int L, int16_t *out, const int64_t *out_off, const FbTfComp *cn, const int *stop,
                        unsigned char *sat) {
  const unsigned chunks = (unsigned)((n_max + AIR_CHUNK - 1) / AIR_CHUNK);
  const dim3 grid(chunks > 0 ? chunks : 1, rows);
  const FbTfComp none{1, 0, nullptr, nullptr};
  if (sat)
    hipLaunchKernelGGL(k_air_conv<true>, grid, dim3(AIR_THREADS), fb_air_conv_lds_bytes(L), s, wav, in_off, r, eot, taps, L, out, out_off,
                       cn ? *cn : none, stop, sat);
  else
    hipLaunchKernelGGL(k_air_conv<false>, grid, dim3(AIR_THREADS), fb_air_conv_lds_bytes(L), s, wav, in_off, r, eot, taps, L, out, out_off,
                       cn ? *cn : none, stop, sat);
}
