// fb_prepare_xvector.cpp -- what fb_load_xvector uploads, prepared on the host (fb_prepare.h): the argument checks of the
// "x-vector" section of fakebob_hip.h, the frame layers' weights as k_xv_affine's f16 fragment images (and, transposed, k_wb_xv_affine_t's), the segment affine
// transposed in float64, and the back end's table (fb_iv_backend_table, shared with the i-vector loader).  No HIP.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "fb_prepare.h"

static int refuse(std::string *err, const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return FB_E_ARG;
}

int fb_xvector_check(const fb_xvector_system *sy, std::string *err) {
  if (!sy) return refuse(err, "null argument");
  if (sy->D <= 0 || sy->D > 2048) return refuse(err, "x-vector system: feature dim D=%d outside 1 .. 2048", sy->D);
  if (sy->n_layers < 1 || sy->n_layers > FB_XV_MAX_LAYERS)
    return refuse(err, "x-vector system: n_layers=%d outside 1 .. %d", sy->n_layers, FB_XV_MAX_LAYERS);
  for (int l = 0; l < sy->n_layers; ++l) {
    const fb_xvector_layer &y = sy->layers[l];
    if (y.dout < 1 || y.dout > 2048) return refuse(err, "x-vector system: layer %d dout=%d outside 1 .. 2048", l, y.dout);
    if (y.n_ctx < 1 || y.n_ctx > FB_XV_MAX_CTX)
      return refuse(err, "x-vector system: layer %d n_ctx=%d outside 1 .. %d", l, y.n_ctx, FB_XV_MAX_CTX);
    for (int j = 0; j < y.n_ctx; ++j) {
      if (y.ctx[j] < -8 || y.ctx[j] > 8) return refuse(err, "x-vector system: layer %d context offset %d outside -8 .. 8", l, y.ctx[j]);
      if (j && y.ctx[j] <= y.ctx[j - 1]) return refuse(err, "x-vector system: layer %d context offsets must ascend", l);
    }
    if (!y.W || !y.bias || !y.bn_scale || !y.bn_offset) return refuse(err, "x-vector system: null array in layer %d", l);
  }
  const int R = sy->R, L = sy->L, S = sy->S;
  if (R < 32 || R > 2048 || R % 32) return refuse(err, "x-vector system: R=%d must be a multiple of 32 in 32 .. 2048", R);
  if (L <= 0 || L > 512) return refuse(err, "x-vector system: L=%d outside 1 .. 512", L);
  if (S <= 0) return refuse(err, "x-vector system: S=%d", S);
  if (S > 60) return refuse(err, "at most 60 enrolled speakers per engine");
  if (sy->lda_cols != R && sy->lda_cols != R + 1) return refuse(err, "transform.mat must have R or R+1 columns");
  if (!sy->seg_W || !sy->seg_bias || !sy->mean_vec || !sy->lda || !sy->plda_mean || !sy->plda_transform || !sy->plda_psi ||
      !sy->enrolled || !sy->z_mean || !sy->z_std)
    return refuse(err, "null array in fb_xvector_system");
  return FB_OK;
}

int fb_prepare_xvector(const fb_xvector_system *sy, FbXvPrepared *out, std::string *err) {
  const int rc = fb_xvector_check(sy, err);
  if (rc != FB_OK) return rc;
  FbXvPrepared p;
  p.D = sy->D;
  p.n_layers = sy->n_layers;
  p.R = sy->R;
  p.max_width = sy->D;
  int din = sy->D;
  for (int l = 0; l < sy->n_layers; ++l) {
    const fb_xvector_layer &y = sy->layers[l];
    FbXvLayerPrepared &q = p.layer[l];
    q.din = din; q.dout = y.dout; q.n_ctx = y.n_ctx;
    for (int j = 0; j < y.n_ctx; ++j) q.ctx[j] = y.ctx[j];
    q.K = y.n_ctx * din;
    q.n_steps = (q.K + 15) / 16;
    const size_t nW = (size_t)y.dout * q.K;
    float amax = 0.0f;
    for (size_t i = 0; i < nW; ++i) {
      if (!isfinite(y.W[i])) return refuse(err, "x-vector system: layer %d has a non-finite weight", l);
      amax = fmaxf(amax, fabsf(y.W[i]));
    }
    q.kw = 0;
    if (amax > 0.0f) {
      int ex;
      (void)frexpf(amax, &ex);   // amax in [2^(ex-1), 2^ex)
      q.kw = ex - 1 - 14;
      if (q.kw < -100) q.kw = -100;
    }
    const size_t per_tile = (size_t)q.n_steps * 2 * 64 * 8;
    q.w.assign((size_t)((y.dout + 31) / 32) * per_tile, 0);   // (the channels past dout of the last tile: zeros)
    for (int o = 0; o < y.dout; ++o) {
      uint16_t *tile = q.w.data() + (size_t)(o / 32) * per_tile;
      for (int k = 0; k < q.K; ++k) {
        const float v = ldexpf(y.W[(size_t)o * q.K + k], -q.kw);   // exact, except below 2^-149 of the layer's maximum
        const _Float16 a = (_Float16)v;                             // round to nearest even
        const _Float16 b = (_Float16)(v - (float)a);                // the residual is exact in float32
        uint16_t ua, ub;
        __builtin_memcpy(&ua, &a, 2);
        __builtin_memcpy(&ub, &b, 2);
        tile[fb_xv_frag_index(0, k, o % 32)] = ua;
        tile[fb_xv_frag_index(1, k, o % 32)] = ub;
      }
    }
    // W transposed, the same two terms under the same power of two: channel place = a K column, K position = an output channel
    q.nt_steps = (y.dout + 15) / 16;
    q.kwt = q.kw;
    const size_t per_tile_t = (size_t)q.nt_steps * 2 * 64 * 8;
    q.wt.assign((size_t)((q.K + 31) / 32) * per_tile_t, 0);   // (zeros past K and past dout)
    for (int k = 0; k < q.K; ++k) {
      uint16_t *tile = q.wt.data() + (size_t)(k / 32) * per_tile_t;
      for (int o = 0; o < y.dout; ++o) {
        const float v = ldexpf(y.W[(size_t)o * q.K + k], -q.kwt);
        const _Float16 a = (_Float16)v;
        const _Float16 b = (_Float16)(v - (float)a);
        uint16_t ua, ub;
        __builtin_memcpy(&ua, &a, 2);
        __builtin_memcpy(&ub, &b, 2);
        tile[fb_xv_frag_index(0, o, k % 32)] = ua;
        tile[fb_xv_frag_index(1, o, k % 32)] = ub;
      }
    }
    q.bias.assign(y.bias, y.bias + y.dout);
    q.scale.assign(y.bn_scale, y.bn_scale + y.dout);
    q.offset.assign(y.bn_offset, y.bn_offset + y.dout);
    din = y.dout;
    if (din > p.max_width) p.max_width = din;
  }
  p.P = din;
  const int P2 = 2 * p.P, R = sy->R;
  p.segT.resize((size_t)P2 * R);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < P2; ++k) p.segT[(size_t)k * R + r] = (double)sy->seg_W[(size_t)r * P2 + k];
  p.seg_bias.resize(R);
  for (int r = 0; r < R; ++r) p.seg_bias[r] = (double)sy->seg_bias[r];
  // the back end: the i-vector system's members of the same names
  fb_ivector_system be = {};
  be.R = sy->R; be.L = sy->L; be.S = sy->S; be.lda_cols = sy->lda_cols;
  be.mean_vec = sy->mean_vec; be.lda = sy->lda; be.plda_mean = sy->plda_mean; be.plda_transform = sy->plda_transform;
  be.plda_psi = sy->plda_psi; be.enrolled = sy->enrolled; be.z_mean = sy->z_mean; be.z_std = sy->z_std;
  fb_iv_backend_table(&be, &p.be);
  *out = std::move(p);
  return FB_OK;
}
