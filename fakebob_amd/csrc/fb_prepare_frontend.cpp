// fb_prepare_frontend.cpp -- the Kaldi front-end's host tables and their packed device image (fb_prepare.h).
// float32-stored Kaldi constants are rounded to float first.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "fb_prepare.h"

static double mel_scale(double f) { return 1127.0 * log(1.0 + f / 700.0); }

static int mel_banks(const fb_frontend_cfg *c, FbFrontendTables *t, std::string *err) {
  const int P = c->padded_length, nb = c->num_mel_bins, Nc = P / 2;
  t->mel_first.assign(nb, 0);
  t->mel_len.assign(nb, 0);
  t->mel_off.assign(nb, 0);
  t->mel_w.clear();
  const double nyq = 0.5 * c->sample_freq;
  const double hi = c->high_freq > 0.0 ? c->high_freq : nyq + c->high_freq;
  if (c->low_freq < 0.0 || hi <= c->low_freq || hi > nyq) {
    *err = "bad mel frequency range";
    return FB_E_ARG;
  }
  const double bw = c->sample_freq / P;
  const double mlo = mel_scale(c->low_freq), mhi = mel_scale(hi), md = (mhi - mlo) / (nb + 1);
  for (int b = 0; b < nb; ++b) {
    const double left = mlo + b * md, center = mlo + (b + 1) * md, right = mlo + (b + 2) * md;
    int first = -1, last = -1;
    std::vector<double> wts;
    for (int i = 0; i < Nc; ++i) {
      const double mel = mel_scale(bw * i);
      if (mel > left && mel < right) {
        const double wv = mel <= center ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first < 0) first = i;
        last = i;
        wts.push_back((double)(float)wv);
      }
    }
    // [EXT] Kaldi's MelBanks refuses a bin that takes no FFT bin ("You may have set --num-mel-bins too large"): its
    // log-energy would be the constant log(FLT_EPSILON)
    if (first < 0) {
      char msg[96];
      snprintf(msg, sizeof(msg), "mel bin %d covers no FFT bin (num_mel_bins %d too large)", b, nb);
      *err = msg;
      return FB_E_ARG;
    }
    t->mel_first[b] = first;
    t->mel_len[b] = last - first + 1;
    t->mel_off[b] = (int)t->mel_w.size();
    t->mel_w.insert(t->mel_w.end(), wts.begin(), wts.end());
  }
  return FB_OK;
}

// the add-deltas kernels of orders 0 .. order, each 2 * order * W + 1 long (Kaldi's DeltaFeatures)
static std::vector<double> delta_scales(int order, int W) {
  const int maxlen = 2 * order * W + 1;
  std::vector<double> dscale((size_t)(order + 1) * maxlen, 0.0);
  dscale[0] = 1.0;
  for (int i = 1; i <= order; ++i) {
    const double *prev = &dscale[(size_t)(i - 1) * maxlen];
    double *cur = &dscale[(size_t)i * maxlen];
    const int poff = (i - 1) * W, coff = i * W;
    double normalizer = 0.0;
    for (int j = -W; j <= W; ++j) {
      normalizer += (double)j * j;
      for (int k = -poff; k <= poff; ++k) cur[j + k + coff] += (double)j * prev[k + poff];
    }
    for (int k = 0; k < 2 * coff + 1; ++k) cur[k] = (double)(float)(cur[k] / normalizer);
  }
  return dscale;
}

int fb_frontend_tables(const fb_frontend_cfg *c, FbFrontendTables *out, std::string *err) {
  const int L = c->frame_length, P = c->padded_length, nb = c->num_mel_bins, nc = c->num_ceps, Nc = P / 2;
  FbFrontendTables t;
  t.window.resize(L);
  t.tw_half.resize(2 * (size_t)(Nc > 1 ? Nc : 1));
  t.tw_full.resize(2 * (size_t)(Nc + 1));
  const double a = 2.0 * M_PI / (L - 1);
  for (int i = 0; i < L; ++i) t.window[i] = (double)(float)pow(0.5 - 0.5 * cos(a * i), 0.85);
  for (int m = 0; m < Nc; ++m) { t.tw_half[2 * m] = cos(-2.0 * M_PI * m / Nc); t.tw_half[2 * m + 1] = sin(-2.0 * M_PI * m / Nc); }
  for (int k = 0; k <= Nc; ++k) { t.tw_full[2 * k] = cos(-2.0 * M_PI * k / P); t.tw_full[2 * k + 1] = sin(-2.0 * M_PI * k / P); }
  const int rc = mel_banks(c, &t, err);
  if (rc != FB_OK) return rc;
  t.dct.resize((size_t)nc * nb);
  t.lifter.resize(nc);
  for (int k = 0; k < nc; ++k)
    for (int n = 0; n < nb; ++n)
      t.dct[(size_t)k * nb + n] = (k == 0) ? (double)(float)sqrt(1.0 / nb)
                                           : (double)(float)(sqrt(2.0 / nb) * cos(M_PI / nb * (n + 0.5) * k));
  for (int i = 0; i < nc; ++i)
    t.lifter[i] = c->cepstral_lifter != 0.0
                      ? (double)(float)(1.0 + 0.5 * c->cepstral_lifter * sin(M_PI * i / c->cepstral_lifter))
                      : 1.0;
  t.dscale = delta_scales(c->delta_order, c->delta_window);
  *out = std::move(t);
  return FB_OK;
}

FbFrontendBlob fb_frontend_pack(const FbFrontendTables &t) {
  FbFrontendBlob b;
  const size_t nb = t.mel_first.size();
  size_t off = 0;
  auto place = [&off](size_t bytes) {  // the next 64-byte aligned piece
    const size_t at = off;
    off = (off + bytes + 63) & ~(size_t)63;
    return at;
  };
  b.o_window = place(sizeof(double) * t.window.size());
  b.o_twh = place(sizeof(double) * t.tw_half.size());
  b.o_twf = place(sizeof(double) * t.tw_full.size());
  b.o_mf = place(sizeof(int) * nb);
  b.o_ml = place(sizeof(int) * nb);
  b.o_mo = place(sizeof(int) * nb);
  b.o_mw = place(sizeof(double) * (t.mel_w.size() + 1));
  b.o_dct = place(sizeof(double) * t.dct.size());
  b.o_lift = place(sizeof(double) * t.lifter.size());
  b.o_ds = place(sizeof(double) * t.dscale.size());
  b.bytes.assign(off, 0);
  char *host = b.bytes.data();
  memcpy(host + b.o_window, t.window.data(), sizeof(double) * t.window.size());
  memcpy(host + b.o_twh, t.tw_half.data(), sizeof(double) * t.tw_half.size());
  memcpy(host + b.o_twf, t.tw_full.data(), sizeof(double) * t.tw_full.size());
  memcpy(host + b.o_mf, t.mel_first.data(), sizeof(int) * nb);
  memcpy(host + b.o_ml, t.mel_len.data(), sizeof(int) * nb);
  memcpy(host + b.o_mo, t.mel_off.data(), sizeof(int) * nb);
  if (!t.mel_w.empty()) memcpy(host + b.o_mw, t.mel_w.data(), sizeof(double) * t.mel_w.size());
  memcpy(host + b.o_dct, t.dct.data(), sizeof(double) * t.dct.size());
  memcpy(host + b.o_lift, t.lifter.data(), sizeof(double) * t.lifter.size());
  memcpy(host + b.o_ds, t.dscale.data(), sizeof(double) * t.dscale.size());
  return b;
}
