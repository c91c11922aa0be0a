// codec_kernel.hip -- the telephone-line codec (fb_set_codec; the contract is in include/fakebob_hip.h): every row the front
// end reads goes through the round trip of G.711 mu-law, G.711 A-law or IMA ADPCM, directly behind the input-transform
// chain.  One launch, k_codec<kind>, int32 arithmetic only.
//
// G.711     element-wise: a thread per sample pair, one 32-bit load and store where the row starts at an even sample and
//           both samples lie in the row, 16-bit ones otherwise (a row of odd length leaves the next one at an odd offset).
// ADPCM     sequential along a row, parallel across rows only: a workgroup owns CODEC_ROWS rows, lane r of wave 0 walks row
//           r, waves 1 .. 3 move the tiles.  The rows pass through LDS in tiles of FB_CODEC_TILE samples, two buffers: while
//           wave 0 walks tile t in one, the other waves write tile t - 1 out of the second and fetch tile t + 1 into it
//           (coalesced along the row), one barrier per tile.  The walker reads eight samples with one 128-bit LDS read,
//           one group ahead, and writes the eight results in place; the row stride (tile + 8 samples = 260 dwords) puts the
//           16 lanes' reads into 16 different groups of four banks.
//           What bounds the launch is ONE row's 48 000-odd dependent samples on a lone wave, which issues one vector
//           instruction per four cycles: the time of a sample is its instruction count (measured: DESIGN.md section 6), then
//           whatever it waits for.  The step table lives in LDS arranged by what the NEXT sample can need: entry ix holds, for
//           the five index moves -1, +2, +4, +6, +8, the clamped index (as the entry's byte offset) and its step in one word
//           -- five words, fetched by two reads at the start of a sample, under its arithmetic; the sample's code then only
//           selects among them (no clamp, no dependent table read behind the last decision; the wait is placed behind the
//           arithmetic by scheduling barriers).  Sample and predictor carry a bias of 32768 so that |d| is one unsigned
//           absolute difference, each of the quantiser's three decisions is a subtraction and an unsigned minimum whose
//           borrow is the decision, and the new predictor is formed from x (vp +- |d| = x) for either sign and bit-selected.
//           A lane past its row's end idles; the loop runs to the workgroup's longest row.
// Rows are independent, nothing is exchanged between workgroups, there are no atomics, every global index is checked
// against [0, n), and the `stop` flag is honoured as the transform kernels honour it.  `out` may be `wav` (in place): every
// sample is read, then written, by the same thread (G.711) or fetched into LDS by the thread that later writes it (ADPCM).
#include "fb_device.h"
#include "fb_kernels.h"

#define CODEC_THREADS 256
#define CODEC_ROWS 16                          // rows of one ADPCM workgroup: lanes 0 .. 15 of wave 0 walk them
#define CODEC_STRIDE (FB_CODEC_TILE + 8)       // samples between two rows of an LDS tile (16-byte aligned; the read-ahead's pad)
#define CODEC_PAIRS (CODEC_ROWS * FB_CODEC_TILE / 2)

__device__ static const int16_t CODEC_STEP[89] = {
    7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
    230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
    1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
    7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

static __device__ __forceinline__ int codec_ulaw(int x) {
  const int v = x >> 2;
  const bool neg = v < 0;
  const int m = min(neg ? -v : v, 8159) + 33;
  int seg = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) seg += m > ((0x40 << k) - 1);  // 0x3F, 0x7F, ..., 0x1FFF
  int q = (m >> (seg + 1)) & 15;
  if (seg == 8) {  // (m = 8192 only)
    seg = 7;
    q = 15;
  }
  const int t = (((q << 3) + 0x84) << seg) - 0x84;
  return neg ? -t : t;
}

static __device__ __forceinline__ int codec_alaw(int x) {
  const int v = x >> 3;
  const bool neg = v < 0;
  const int m = neg ? -v - 1 : v;
  int seg = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) seg += m > ((0x20 << k) - 1);  // 0x1F, 0x3F, ..., 0xFFF
  const int q = seg < 2 ? (m >> 1) & 15 : (m >> seg) & 15;
  const int t = q << 4;
  const int u = seg == 0 ? t + 8 : (seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1));
  return neg ? -u : u;
}

template <int KIND>
static __device__ __forceinline__ void codec_g711(const int16_t *wav, const int64_t *__restrict__ off, int16_t *out) {
  const int64_t base = off[blockIdx.y], n = off[blockIdx.y + 1] - base;
  const int64_t i = 2 * ((int64_t)blockIdx.x * CODEC_THREADS + threadIdx.x);
  if (i >= n) return;  // (the grid is sized for the longest row of the batch)
  if ((base & 1) == 0 && i + 1 < n) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(wav + base + i);
    const int a = (int16_t)(w & 0xffffu), b = (int16_t)(w >> 16);
    const int ya = KIND == FB_CODEC_ULAW ? codec_ulaw(a) : codec_alaw(a), yb = KIND == FB_CODEC_ULAW ? codec_ulaw(b) : codec_alaw(b);
    *reinterpret_cast<uint32_t *>(out + base + i) = ((uint32_t)ya & 0xffffu) | ((uint32_t)yb << 16);
    return;
  }
  for (int64_t j = i; j < n && j < i + 2; ++j) {
    const int a = wav[base + j];
    out[base + j] = (int16_t)(KIND == FB_CODEC_ULAW ? codec_ulaw(a) : codec_alaw(a));
  }
}

// One sample of the ADPCM round trip for one lane.  xb, vpb: the sample and the predictor plus 32768 (0 .. 65535), so that
// |d| is one unsigned absolute difference; step: STEP[ix]; ea: the byte offset of entry ix in tab (the five candidates of the
// next sample).  Returns the new predictor, biased: it is the decoded sample.
static __device__ __forceinline__ uint32_t codec_adpcm_sample(uint32_t xb, uint32_t &vpb, uint32_t &step, uint32_t &ea, const unsigned char *tab) {
  const uint4 c = *reinterpret_cast<const uint4 *>(tab + ea);  // index moves -1, +2, +4, +6
  const uint32_t c8 = *reinterpret_cast<const uint32_t *>(tab + ea + 16);  // ... and +8
  __builtin_amdgcn_sched_barrier(0);  // (the reads go out first: their latency is what the arithmetic below covers)
  const uint32_t h = step >> 1, q = step >> 2, e = step >> 3;
  const uint32_t m = (uint32_t)((int)(xb - vpb) >> 31);  // all ones when d < 0
  uint32_t ad;
  asm("v_sad_u32 %0, %1, %2, 0" : "=v"(ad) : "v"(xb), "v"(vpb));  // |xb - vpb|: one instruction where hipcc issues three
  // the quantiser's three decisions on the remainder of |d|: r - part wraps above r exactly when r < part, so the unsigned
  // minimum is the conditional subtraction, and the decisions themselves (n: not taken) stand beside the chain
  const bool n2 = ad < step;
  const uint32_t r2 = min(ad, ad - step);
  const bool n1 = r2 < h;
  const uint32_t r1 = min(r2, r2 - h);
  const bool n0 = r1 < q;
  const uint32_t r0 = min(r1, r1 - q);
  // vd = |d| - r0 + (step >> 3), and vp +- |d| is x itself: the new predictor is x -+ (r0 - e), clipped
  const int up = (int)((xb + e) - r0), dn = (int)((xb - e) + r0);
  int nv;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(nv) : "v"(m), "v"(dn), "v"(up));  // m ? dn : up as a bit select: no mask register to wait for
  vpb = (uint32_t)min(max(nv, 0), 65535);
  // everything above runs under the table's latency; the candidates are first needed here
  __builtin_amdgcn_sched_barrier(0);
  // delta = 4 b2 + 2 b1 + b0 (b = !n): below 4 the index moves by -1, else by 2 (delta - 3); the last decision selects last
  uint32_t lo = n1 ? c.y : c.w, hi = n1 ? c.z : c8;
  lo = n2 ? c.x : lo;
  hi = n2 ? c.x : hi;
  const uint32_t r = n0 ? lo : hi;
  step = r & 0xffffu;
  ea = r >> 16;
  return vpb;
}

static __device__ __forceinline__ void codec_adpcm(const int16_t *wav, const int64_t *__restrict__ off, int B, int16_t *out) {
  __shared__ __attribute__((aligned(16))) int16_t s_buf[2][CODEC_ROWS * CODEC_STRIDE];
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[89 * 8];  // entry ix: five candidate words (byte offset << 16 | step), three unused
  __shared__ int64_t s_base[CODEC_ROWS], s_n[CODEC_ROWS];
  const int tid = threadIdx.x;
  const int R0 = blockIdx.x * CODEC_ROWS;
  if (tid < CODEC_ROWS) {
    const int R = R0 + tid;
    s_base[tid] = R < B ? off[R] : 0;
    s_n[tid] = R < B ? off[R + 1] - off[R] : 0;  // (a row past the batch: no samples, its lane and its pairs idle)
  }
  if (tid >= FB_WAVE && tid < FB_WAVE + 89) {
    const int ix = tid - FB_WAVE;
    const int mv[5] = {-1, 2, 4, 6, 8};
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int nx = min(max(ix + mv[c], 0), 88);
      s_tab[ix * 8 + c] = ((uint32_t)(nx * 32) << 16) | (uint32_t)CODEC_STEP[nx];
    }
  }
  __syncthreads();
  int64_t n_max = 0;
  for (int r = 0; r < CODEC_ROWS; ++r) n_max = max(n_max, s_n[r]);
  const int tiles = (int)((n_max + FB_CODEC_TILE - 1) / FB_CODEC_TILE);  // (rows of up to 2^31 samples: below 2^22 tiles)

  // waves 1 .. 3: pair p of a tile (samples 2 k, 2 k + 1 of row r) stays with one thread -- it writes tile t_out's results
  // out of `buf`, then fetches tile t_in's samples into the same two slots (either tile may be -1: none)
  auto stage = [&](int t_out, int t_in, int16_t *buf) {
    for (int p = tid - FB_WAVE; p < CODEC_PAIRS; p += CODEC_THREADS - FB_WAVE) {
      const int r = p / (FB_CODEC_TILE / 2), k = p % (FB_CODEC_TILE / 2);
      const int64_t base = s_base[r], n = s_n[r];
      const bool even = (base & 1) == 0;
      uint32_t *slot = reinterpret_cast<uint32_t *>(buf + r * CODEC_STRIDE + 2 * k);
      if (t_out >= 0) {
        const int64_t i = (int64_t)t_out * FB_CODEC_TILE + 2 * k;
        if (i < n) {
          const uint32_t w = *slot;
          if (even && i + 1 < n) *reinterpret_cast<uint32_t *>(out + base + i) = w;
          else {
            out[base + i] = (int16_t)(w & 0xffffu);
            if (i + 1 < n) out[base + i + 1] = (int16_t)(w >> 16);
          }
        }
      }
      if (t_in >= 0) {
        const int64_t i = (int64_t)t_in * FB_CODEC_TILE + 2 * k;
        if (i < n) {
          uint32_t w;
          if (even && i + 1 < n) w = *reinterpret_cast<const uint32_t *>(wav + base + i);
          else {
            w = (uint16_t)wav[base + i];
            if (i + 1 < n) w |= (uint32_t)(uint16_t)wav[base + i + 1] << 16;
          }
          *slot = w;
        }
      }
    }
  };

  if (tid >= FB_WAVE) stage(-1, 0, s_buf[0]);
  __syncthreads();
  uint32_t vpb = 32768u, step = (uint32_t)CODEC_STEP[0], ea = 0;  // the state (0, 0), the predictor biased
  const unsigned char *tab = reinterpret_cast<const unsigned char *>(s_tab);
  for (int t = 0; t < tiles; ++t) {
    if (tid >= FB_WAVE) {
      stage(t >= 1 ? t - 1 : -1, t + 1 < tiles ? t + 1 : -1, s_buf[(t + 1) & 1]);
    } else if (tid < CODEC_ROWS) {
      const int64_t left = s_n[tid] - (int64_t)t * FB_CODEC_TILE;
      const int groups = left <= 0 ? 0 : (int)((min(left, (int64_t)FB_CODEC_TILE) + 7) >> 3);
      int16_t *row = s_buf[t & 1] + tid * CODEC_STRIDE;
      uint4 cur = *reinterpret_cast<const uint4 *>(row);
      for (int g = 0; g < groups; ++g) {
        // (the last group of a tile reads the row's pad; samples past the row's end in a group are computed and never
        //  written out -- the state behind the row's end is not used)
        const uint4 nxt = *reinterpret_cast<const uint4 *>(row + 8 * (g + 1));
        const uint32_t in[4] = {cur.x ^ 0x80008000u, cur.y ^ 0x80008000u, cur.z ^ 0x80008000u, cur.w ^ 0x80008000u};  // + 32768 each
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t ya = codec_adpcm_sample(in[j] & 0xffffu, vpb, step, ea, tab);
          const uint32_t yb = codec_adpcm_sample(in[j] >> 16, vpb, step, ea, tab);
          o[j] = (ya | (yb << 16)) ^ 0x80008000u;
        }
        *reinterpret_cast<uint4 *>(row + 8 * g) = uint4{o[0], o[1], o[2], o[3]};
        cur = nxt;
      }
    }
    __syncthreads();
  }
  if (tid >= FB_WAVE && tiles > 0) stage(tiles - 1, -1, s_buf[(tiles - 1) & 1]);
}

// out row R (at off[R], as in wav) = the round trip of row R of wav through codec KIND; out == wav is allowed
template <int KIND>
__global__ __launch_bounds__(CODEC_THREADS) void k_codec(const int16_t *wav, const int64_t *__restrict__ off, int B, int16_t *out,
                                                         const int *__restrict__ stop) {
  if (stop && *stop) return;
  if constexpr (KIND == FB_CODEC_ADPCM) codec_adpcm(wav, off, B, out);
  else codec_g711<KIND>(wav, off, out);
}

void fb_launch_codec(hipStream_t s, int kind, const int16_t *wav, const int64_t *off, int B, int64_t n_max, int16_t *out, const int *stop) {
  if (kind == FB_CODEC_ADPCM) {
    hipLaunchKernelGGL(k_codec<FB_CODEC_ADPCM>, dim3((B + CODEC_ROWS - 1) / CODEC_ROWS), dim3(CODEC_THREADS), 0, s, wav, off, B, out, stop);
    return;
  }
  const unsigned chunks = (unsigned)((n_max + 2 * CODEC_THREADS - 1) / (2 * CODEC_THREADS));
  const dim3 grid(chunks > 0 ? chunks : 1, B);
  if (kind == FB_CODEC_ULAW) hipLaunchKernelGGL(k_codec<FB_CODEC_ULAW>, grid, dim3(CODEC_THREADS), 0, s, wav, off, B, out, stop);
  else hipLaunchKernelGGL(k_codec<FB_CODEC_ALAW>, grid, dim3(CODEC_THREADS), 0, s, wav, off, B, out, stop);
}
