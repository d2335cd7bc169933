// AutoAssignHead on the HIP step: the two normalisers (dsl_aa_assign) and the loss with every gradient (dsl_aa_loss) of a dsl_aa_desc.
// Restates mmdet/models/dense_heads/autoassign_head.py:81-119 (centre prior), :173-187 (points), :204-212 (forward), :238-256
// (positive loss), :282-310 (negative loss), :384-437 (IoU, normalisers, centre loss, the batch without boxes), :492-509 (inside
// mask) and bbox_overlaps / GIoULoss by way of box_loss.hpp; semantics and refusals: include/dsl_hip.h.
//
// No float atomics anywhere: a (point, box) pair is visited by the box's wavefront (sums over the box's footprint, lane partial sums
// in footprint order, then the xor butterfly) and by the point's wavefront (one lane per box, contributions to one class added in
// box order), the workgroups' sums go through block records added in a fixed order, the prior's gradients through one record per box
// added per class in box order.  A second run is bit-identical, and no sum depends on how a level is cut into workgroups.
#include "common.hpp"
#pragma clang fp contract(off)
#include "head_common.hpp"
#include "box_loss.hpp"

namespace {

constexpr int AA_CH = 64;       // boxes staged per LDS chunk (the per-point IoU pass), and the boxes one wavefront holds at a time
constexpr int AA_REC = 16;      // floats per box record
constexpr float AA_EPS = 1e-12f;
// box record columns
enum { BR_C = 0, BR_W = 1, BR_PW = 2, BR_TMIN = 3, BR_TMAX = 4, BR_CNT = 5, BR_TERM = 6, BR_DM = 8 /* dmean x, y, dsigma x, y */ };

struct AaK : HeadK {
  float w_pos, w_neg, w_center;
  int max_gt;
  const float* gt_boxes; const long long* gt_labels; const int* gt_off;
  const float* mean; const float* sigma; float* g_mean; float* g_sigma;
  float* iou; float* stats;
  float* box_rec;      // [max_gt][AA_REC], behind the block records in the workspace
  float* img_rec;      // [n][4]: sum c, inside pairs, d loss_center / d c (times grad_scale), loss_center term
};

// the image of box b (gt_off is ascending, n is small)
__device__ __forceinline__ int aa_box_image(const AaK& p, int b) {
  int img = 0;
  for (int i = 1; i < p.n; ++i)
    if (b >= p.gt_off[i]) img = i;
  return img;
}

// The cells of level l a box can contain, conservatively (the exact test is aa_inside): x s > x1 and x s < x2
__device__ __forceinline__ void aa_footprint(const AaK& p, int l, const f32x4 b, int& xlo, int& ylo, int& nx, int& ny) {
  const float fs = (float)p.stride[l];
  const float w = (float)p.w[l], h = (float)p.h[l];
  xlo = (int)fminf(fmaxf(floorf(b[0] / fs), 0.f), w);
  ylo = (int)fminf(fmaxf(floorf(b[1] / fs), 0.f), h);
  const int xhi = (int)fminf(fmaxf(ceilf(b[2] / fs), -1.f), w - 1.f);
  const int yhi = (int)fminf(fmaxf(ceilf(b[3] / fs), -1.f), h - 1.f);
  nx = xhi - xlo + 1;
  ny = yhi - ylo + 1;
  if (nx < 0) nx = 0;
  if (ny < 0) ny = 0;
}

// min(l, t, r, b) > 0 in fp32, the reference's four differences (:498-504); false for a NaN coordinate
__device__ __forceinline__ bool aa_inside(float px, float py, const f32x4 b) {
  return fminf(fminf(px - b[0], py - b[1]), fminf(b[2] - px, b[3] - py)) > 0.f;
}

// c(i, g) and its factors' arguments (:95-98): u_d = (p_d - centre_d) / s - mean_d
struct AaPrior { float mx, my, sx, sy; };
__device__ __forceinline__ float aa_prior(float px, float py, float fs, const f32x4 b, const AaPrior& q, float& ux, float& uy) {
  ux = (px - (b[0] + b[2]) / 2.f) / fs - q.mx;
  uy = (py - (b[1] + b[3]) / 2.f) / fs - q.my;
  return expf(-(ux * ux) / (2.f * (q.sx * q.sx))) * expf(-(uy * uy) / (2.f * (q.sy * q.sy)));
}

__device__ __forceinline__ float aa_sigmoid(float x) {
  const float e = __expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  return x >= 0.f ? inv : e * inv;
}

// the decoded box of location m: relu(scale x) s from the point (x s, y s) (:173-187, :204-212)
__device__ __forceinline__ f32x4 aa_decode(const AaK& p, int m, int lvl, float px, float py, f32x4& raw) {
  raw = *reinterpret_cast<const f32x4*>(p.regctr + (long long)m * p.ld_rc);
  const float sc = p.scales[lvl], fs = (float)p.stride[lvl];
  f32x4 o;
  o[0] = px - fmaxf(sc * raw[0], 0.f) * fs;
  o[1] = py - fmaxf(sc * raw[1], 0.f) * fs;
  o[2] = px + fmaxf(sc * raw[2], 0.f) * fs;
  o[3] = py + fmaxf(sc * raw[3], 0.f) * fs;
  return o;
}

// plain IoU of bbox_overlaps (union clamped at 1e-6)
__device__ __forceinline__ float aa_iou(const f32x4 a, const f32x4 b) {
  const float a1 = (a[2] - a[0]) * (a[3] - a[1]), a2 = (b[2] - b[0]) * (b[3] - b[1]);
  const float iw = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f), ih = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
  const float ov = iw * ih;
  return ov / fmaxf(a1 + a2 - ov, 1e-6f);
}

// What one (point, box) pair contributes: p_pos, w = exp(3 p_pos) c, and dl = d(1 - giou) / d(decoded box)
struct AaPair { float p, c, e, pc, po, ux, uy; float dl[4]; };
__device__ __forceinline__ void aa_pair(const AaK& p, int m, int lvl, float px, float py, const f32x4 b, int label, const AaPrior& q, AaPair& r) {
  f32x4 raw;
  const f32x4 d = aa_decode(p, m, lvl, px, py, raw);
  const float reg = p.w_bbox * box_loss_giou(false, d[0], d[1], d[2], d[3], b[0], b[1], b[2], b[3], r.dl);
  r.pc = aa_sigmoid(p.cls_logits[(long long)m * p.ld_cls + label]);
  r.po = aa_sigmoid(p.regctr[(long long)m * p.ld_rc + 4]);
  r.p = r.pc * r.po * expf(-reg);
  r.c = aa_prior(px, py, (float)p.stride[lvl], b, q, r.ux, r.uy);
  r.e = expf(3.f * r.p);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// d BCE(R, 1) / dR as torch's backward forms it: (R - 1) / max((1 - R) R, 1e-12)
__device__ __forceinline__ float aa_bce1_grad(float R) { return (R - 1.f) / fmaxf((1.f - R) * R, AA_EPS); }

// ---- per box: walk the footprint, one wavefront per box ------------------------------------------------------------------------------
// kMode 0 (assignment): sum c.  kMode 1 (loss, forward): sum c, sum w, sum p w, min / max t, inside pairs, the box's loss term.
// kMode 2 (loss, backward): the box's d mean / d sigma record.
template <int kMode>
__global__ __launch_bounds__(256) void aa_box_kernel(const AaK p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.max_gt || b >= p.gt_off[p.n]) return;      // (wave-uniform)
  const int img = aa_box_image(p, b);
  const f32x4 box = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * b);
  const long long lab = p.gt_labels[b];
  float* rec = p.box_rec + (long long)b * AA_REC;
  if (lab < 0 || lab >= p.num_classes) {      // a label the prior has no row for: the box takes no part
    if (lane < AA_REC && (kMode != 2 || lane >= BR_DM)) rec[lane] = 0.f;
    return;
  }
  const int label = (int)lab;
  const AaPrior q = {p.mean[2 * label], p.mean[2 * label + 1], p.sigma[2 * label], p.sigma[2 * label + 1]};
  float s_c = 0.f, s_w = 0.f, s_pw = 0.f, tmin = __builtin_inff(), tmax = -__builtin_inff(), cnt = 0.f;
  float dm[4] = {0.f, 0.f, 0.f, 0.f};
  float dLdR = 0.f, R = 0.f, D = 1.f, flagD = 0.f, dcen = 0.f;
  if (kMode == 2) {
    const float sw = rec[BR_W];
    D = fmaxf(sw, AA_EPS);
    flagD = sw >= AA_EPS ? 1.f : 0.f;
    R = rec[BR_PW] / D;
    const float npos = fmaxf(p.norm[0] * p.inv_world, 1.0f);
    dLdR = p.w_pos / npos * p.grad_scale * aa_bce1_grad(R);
    dcen = p.img_rec[4 * img + 2];
  }
  for (int l = 0; l < p.nlvl; ++l) {
    int xlo, ylo, nx, ny;
    aa_footprint(p, l, box, xlo, ylo, nx, ny);
    const float fs = (float)p.stride[l];
    const int base = p.mstart[l] + img * p.h[l] * p.w[l];
    for (int k = lane; k < nx * ny; k += 64) {
      const int yy = k / nx, y = ylo + yy, x = xlo + (k - yy * nx);
      const float px = (float)x * fs, py = (float)y * fs;
      if (!aa_inside(px, py, box)) continue;
      if (kMode == 0) {
        float ux, uy;
        s_c += aa_prior(px, py, fs, box, q, ux, uy);
        continue;
      }
      const int m = base + y * p.w[l] + x;
      AaPair r;
      aa_pair(p, m, l, px, py, box, label, q, r);
      if (kMode == 1) {
        const float w = r.e * r.c;
        const float t = 1.f / fmaxf(1.f - p.iou[m], AA_EPS);      // (:293)
        s_c += r.c; s_w += w; s_pw += r.p * w; cnt += 1.f;
        tmin = fminf(tmin, t); tmax = fmaxf(tmax, t);
      } else {
        // d L / d c of the pair: through w = e c in R (numerator and clamped denominator) and through the image's centre loss
        const float g = dLdR * r.e * (r.p - R * flagD) / D + dcen;
        const float gc = g * r.c;
        dm[0] += gc * (r.ux / (q.sx * q.sx));
        dm[1] += gc * (r.uy / (q.sy * q.sy));
        dm[2] += gc * (r.ux * r.ux / (q.sx * q.sx * q.sx));
        dm[3] += gc * (r.uy * r.uy / (q.sy * q.sy * q.sy));
      }
    }
  }
  if (kMode == 0) {
    s_c = wave_sum(s_c);
    if (lane == 0) rec[BR_C] = s_c;
  } else if (kMode == 1) {
    s_c = wave_sum(s_c); s_w = wave_sum(s_w); s_pw = wave_sum(s_pw); cnt = wave_sum(cnt);
    tmin = wave_min(tmin); tmax = wave_max(tmax);
    if (lane == 0) {
      const float Rg = s_pw / fmaxf(s_w, AA_EPS);
      rec[BR_C] = s_c; rec[BR_W] = s_w; rec[BR_PW] = s_pw; rec[BR_TMIN] = tmin; rec[BR_TMAX] = tmax; rec[BR_CNT] = cnt;
      rec[BR_TERM] = -fmaxf(logf(Rg), -100.f);      // BCE(R, 1) (:251-254); R = 0 for a box without a point: 100
      rec[7] = 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) dm[k] = wave_sum(dm[k]);
    if (lane < 4) rec[BR_DM + lane] = lane == 0 ? dm[0] : lane == 1 ? dm[1] : lane == 2 ? dm[2] : dm[3];
  }
}

// stats[0] = boxes in the batch, stats[1] = sum c - the box records added in box order; stats[2..7] = 0
__global__ __launch_bounds__(REC_T) void aa_assign_finalize_kernel(const AaK p) {
  __shared__ float sh[REC_T];
  const int G = p.gt_off[p.n] < p.max_gt ? p.gt_off[p.n] : p.max_gt;
  const float t = record_sum(p.box_rec, G, AA_REC, BR_C, 1, sh);
  if (threadIdx.x == 0) {
    p.stats[0] = (float)G;
    p.stats[1] = t;
  }
  if (threadIdx.x >= 2 && threadIdx.x < 8) p.stats[threadIdx.x] = 0.f;
}

// ---- per point: iou(i) = max over ALL boxes of the image of the plain IoU with the point's decoded box (:384-394) -----------------------
__global__ __launch_bounds__(256) void aa_iou_kernel(const AaK p) {
  __shared__ f32x4 sbox[AA_CH];
  const int m = blockIdx.x * 256 + threadIdx.x;
  const bool live = m < p.M;
  int lvl = 0, img = 0, y = 0, x = 0, g0 = 0, g1 = 0;
  f32x4 d = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    head_loc(p, m, lvl, img, y, x);
    g0 = p.gt_off[img];
    g1 = p.gt_off[img + 1];
    f32x4 raw;
    d = aa_decode(p, m, lvl, (float)x * (float)p.stride[lvl], (float)y * (float)p.stride[lvl], raw);
  }
  // the union of the workgroup's box ranges (fovea_loss.hip): workgroup-uniform, so every thread runs the chunk loop's barriers
  const int m_first = blockIdx.x * 256, m_last = m_first + 255 < p.M ? m_first + 255 : p.M - 1;
  int l_first, i_first, l_last, i_last, yy, xx;
  head_loc(p, m_first, l_first, i_first, yy, xx);
  head_loc(p, m_last, l_last, i_last, yy, xx);
  const int gend = p.gt_off[p.n] < p.max_gt ? p.gt_off[p.n] : p.max_gt;
  int gmin = p.gt_off[l_first == l_last ? i_first : 0], gmax = p.gt_off[l_first == l_last ? i_last + 1 : p.n];
  if (gmax > gend) gmax = gend;
  if (g1 > gend) g1 = gend;
  float best = 0.f;
  for (int c0 = gmin; c0 < gmax; c0 += AA_CH) {
    __syncthreads();
    const int gs = c0 + (int)threadIdx.x;
    if (threadIdx.x < AA_CH && gs < gmax) sbox[threadIdx.x] = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * gs);
    __syncthreads();
    const int ga = g0 > c0 ? g0 : c0, gb = g1 < c0 + AA_CH ? g1 : c0 + AA_CH;
    for (int g = ga; g < gb; ++g) best = fmaxf(best, aa_iou(d, sbox[g - c0]));
  }
  if (live) p.iou[m] = best;
}

// ---- per image: sum c and the inside pairs from the box records in box order; the centre loss term and d / d c ------------------------
__global__ __launch_bounds__(64) void aa_image_kernel(const AaK p) {
  const int gend = p.gt_off[p.n] < p.max_gt ? p.gt_off[p.n] : p.max_gt;
  for (int i = threadIdx.x; i < p.n; i += 64) {
    int g0 = p.gt_off[i], g1 = p.gt_off[i + 1];
    if (g1 > gend) g1 = gend;
    float sc = 0.f, cnt = 0.f;
    for (int g = g0; g < g1; ++g) {
      sc += p.box_rec[(long long)g * AA_REC + BR_C];
      cnt += p.box_rec[(long long)g * AA_REC + BR_CNT];
    }
    const float nb = (float)(g1 > g0 ? g1 - g0 : 0);
    float term = 0.f, dc = 0.f;
    if (cnt > 0.f) {      // (:422-425) n_boxes / clamp(sum c, 1e-12); the clamp passes the gradient where sum c >= 1e-12
      const float den = fmaxf(sc, AA_EPS);
      term = nb / den;
      dc = sc >= AA_EPS ? -(nb / (den * den)) * (p.w_center / (float)p.n) * p.grad_scale : 0.f;
    }
    float* r = p.img_rec + 4 * i;
    r[0] = sc; r[1] = cnt; r[2] = dc; r[3] = term;
  }
}

// ---- per point, forward and backward: one wavefront per location --------------------------------------------------------------------
// A lane per box of the image (64 at a time) for the positive terms; then the boxes that hold the point are taken in ascending index
// by the lane that owns their class, so that contributions to one class are added in box order and the highest index of a class
// leaves its negative weight (:303-304).  Then a lane per class (two classes above 64) for the negative loss.
// Block records [neg, g_scale x 5, 0 ...] of 16 floats.
__global__ __launch_bounds__(256) void aa_point_kernel(const AaK p) {
  __shared__ float sh[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = p.num_classes;
  const float npos = fmaxf(p.norm[0] * p.inv_world, 1.0f), nneg = fmaxf(p.norm[1] * p.inv_world, 1.0f);
  const float a_pos = p.w_pos / npos * p.grad_scale, a_neg = p.w_neg / nneg * p.grad_scale;
  const int gend = p.gt_off[p.n] < p.max_gt ? p.gt_off[p.n] : p.max_gt;
  float neg_acc = 0.f;
  float gsc[DSL_MAX_SEG] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const int ngroup = (p.M + 3) / 4;
  for (int grp = blockIdx.x; grp < ngroup; grp += gridDim.x) {
    const int m = grp * 4 + wave;
    if (m >= p.M) continue;      // (wave-uniform; no barrier inside the loop)
    int lvl, img, y, x;
    head_loc(p, m, lvl, img, y, x);
    const float fs = (float)p.stride[lvl];
    const float px = (float)x * fs, py = (float)y * fs;
    const int g0 = p.gt_off[img];
    int g1 = p.gt_off[img + 1];
    if (g1 > gend) g1 = gend;
    const float iou = p.iou[m];
    const float t = 1.f / fmaxf(1.f - iou, AA_EPS);
    const float xo = p.regctr[(long long)m * p.ld_rc + 4];
    const float po = aa_sigmoid(xo);
    const int c0 = lane, c1 = lane + 64;
    float wn0 = 1.f, wn1 = 1.f, gp0 = 0.f, gp1 = 0.f;      // negative weight and positive-term gradient of the lane's classes
    float gobj = 0.f, gbox[4] = {0.f, 0.f, 0.f, 0.f};
    for (int cb = g0; cb < g1; cb += AA_CH) {
      const int g = cb + lane;
      bool ins = false;
      int label = -1;
      float dcls = 0.f, wn = 1.f, dob = 0.f, db[4] = {0.f, 0.f, 0.f, 0.f};
      if (g < g1) {
        const f32x4 box = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * g);
        const long long lab = p.gt_labels[g];
        if (lab >= 0 && lab < C && aa_inside(px, py, box)) {
          ins = true;
          label = (int)lab;
          const AaPrior q = {p.mean[2 * label], p.mean[2 * label + 1], p.sigma[2 * label], p.sigma[2 * label + 1]};
          AaPair r;
          aa_pair(p, m, lvl, px, py, box, label, q, r);
          const float* rec = p.box_rec + (long long)g * AA_REC;
          const float sw = rec[BR_W];
          const float D = fmaxf(sw, AA_EPS), flagD = sw >= AA_EPS ? 1.f : 0.f;
          const float R = rec[BR_PW] / D;
          const float w = r.e * r.c;
          // d L_pos / d p_pos: R = sum p w / clamp(sum w), w = exp(3 p) c
          const float dLdp = a_pos * aa_bce1_grad(R) * (w * (1.f + 3.f * r.p) - 3.f * w * R * flagD) / D;
          dcls = dLdp * r.p * (1.f - r.pc);
          dob = dLdp * r.p * (1.f - r.po);
          const float dreg = -dLdp * r.p * p.w_bbox;      // p_loc = exp(-reg)
#pragma unroll
          for (int k = 0; k < 4; ++k) db[k] = dreg * r.dl[k];
          const float tn = (t - rec[BR_TMIN] + AA_EPS) / (rec[BR_TMAX] - rec[BR_TMIN] + AA_EPS);      // (:295-296)
          wn = 1.f - tn;
        }
      }
      gobj += wave_sum(dob);
#pragma unroll
      for (int k = 0; k < 4; ++k) gbox[k] += wave_sum(db[k]);
      unsigned long long mask = __ballot(ins);
      while (mask) {
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int lj = __shfl(label, j, 64);
        const float dj = __shfl(dcls, j, 64), wj = __shfl(wn, j, 64);
        if (lj == c0) { wn0 = wj; gp0 += dj; }
        if (lj == c1) { wn1 = wj; gp1 += dj; }
      }
    }
    // negative loss over the classes (:306-310): q = sigmoid(cls) sigmoid(obj) p_neg_weight, q^2 BCE(q, 0)
    float nl = 0.f, dobj_neg = 0.f;
    const float* xr = p.cls_logits + (long long)m * p.ld_cls;
    uint16_t* gr = p.g_cls + (long long)m * p.ld_gcls;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = h ? c1 : c0;
      if (c >= C) continue;
      const float wn = h ? wn1 : wn0;
      const float pc = aa_sigmoid(xr[c]);
      const float qq = pc * po * wn;
      const float bce = -fmaxf(log1pf(-qq), -100.f);
      nl += qq * qq * bce;
      const float dq = a_neg * (2.f * qq * bce + qq * qq * (qq / fmaxf((1.f - qq) * qq, AA_EPS)));
      dobj_neg += dq * wn * pc * (po * (1.f - po));
      gr[c] = f2bf(dq * wn * po * (pc * (1.f - pc)) + (h ? gp1 : gp0));
    }
    neg_acc += wave_sum(nl);
    gobj += wave_sum(dobj_neg);
    if (lane == 0) {
      const f32x4 raw = *reinterpret_cast<const f32x4*>(p.regctr + (long long)m * p.ld_rc);
      const float sc = p.scales[lvl];
      const float dd[4] = {-gbox[0], -gbox[1], gbox[2], gbox[3]};      // d / d distance from d / d (x1, y1, x2, y2)
      float go[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float on = sc * raw[k] > 0.f ? 1.f : 0.f;      // ReLU
        go[k] = dd[k] * fs * on * sc;
        const float v = dd[k] * fs * on * raw[k];
#pragma unroll
        for (int l = 0; l < DSL_MAX_SEG; ++l) gsc[l] += l == lvl ? v : 0.f;      // (static indices: the sums stay in registers)
      }
      u32x4 o = {pack2bf(go[0], go[1]), pack2bf(go[2], go[3]), pack2bf(gobj, 0.f), 0u};
      *reinterpret_cast<u32x4*>(p.g_rc + (long long)m * p.ld_grc) = o;
    }
  }
  // (neg_acc is the same in every lane; gsc lives in lane 0 of each wavefront)
  float* rec = p.part + 16ll * blockIdx.x;
  const float v0 = block_sum(lane == 0 ? neg_acc : 0.f, sh);
  if (threadIdx.x == 0) rec[0] = v0;
#pragma unroll
  for (int l = 0; l < DSL_MAX_SEG; ++l) {
    const float v = block_sum(lane == 0 ? gsc[l] : 0.f, sh);
    if (threadIdx.x == 0) rec[1 + l] = v;
  }
  if (threadIdx.x >= 1 + DSL_MAX_SEG && threadIdx.x < 16) rec[threadIdx.x] = 0.f;
}

// ---- the sums: losses[4] (pos, neg, center, 0), logvec[4], g_scales[5], g_mean / g_sigma [C][2] ------------------------------------------
__global__ __launch_bounds__(REC_T) void aa_finalize_kernel(const AaK p, int nblocks) {
  __shared__ float sh[REC_T];
  __shared__ float out[4];
  const int G = p.gt_off[p.n] < p.max_gt ? p.gt_off[p.n] : p.max_gt;
  const float t = record_sum(p.part, nblocks, 16, 0, 8, sh);      // thread v < 8: neg, g_scale x 5, 0, 0
  const float pos = record_sum(p.box_rec, G, AA_REC, BR_TERM, 1, sh);
  if (threadIdx.x == 0) {
    const float npos = fmaxf(p.norm[0] * p.inv_world, 1.0f), nneg = fmaxf(p.norm[1] * p.inv_world, 1.0f);
    float cen = 0.f;
    for (int i = 0; i < p.n; ++i) cen += p.img_rec[4 * i + 3];
    // a batch without boxes (:433-437): loss_pos = loss_center = 0
    out[0] = p.losses[0] = G > 0 ? pos * p.w_pos / npos : 0.f;
    out[1] = p.losses[1] = t * p.w_neg / nneg;
    out[2] = p.losses[2] = G > 0 ? cen / (float)p.n * p.w_center : 0.f;
    p.losses[3] = 0.f;
  } else if (threadIdx.x >= 1 && threadIdx.x <= DSL_MAX_SEG) {
    p.g_scales[threadIdx.x - 1] = threadIdx.x - 1 < p.nlvl ? t : 0.f;
  }
  // the prior's gradients: per class the boxes' records in box order
  for (int i = threadIdx.x; i < 4 * p.num_classes; i += REC_T) {
    const int c = i >> 2, k = i & 3;
    float a = 0.f;
    for (int g = 0; g < G; ++g)
      if (p.gt_labels[g] == c) a += p.box_rec[(long long)g * AA_REC + BR_DM + k];
    (k < 2 ? p.g_mean : p.g_sigma)[2 * c + (k & 1)] = a;
  }
  if (p.logvec) {
    __syncthreads();
    if (threadIdx.x == 0) {
      p.logvec[0] = out[0]; p.logvec[1] = out[1]; p.logvec[2] = out[2];
      p.logvec[3] = out[0] + out[1] + out[2];
    }
  }
}

}  // namespace

// what a DSL_HEAD_AUTOASSIGN descriptor adds to dsl_fcos_workspace_bytes, behind the block records: the box and the image records
size_t dsl_aa_workspace_extra(const dsl_fcos_desc* d) {
  const dsl_aa_desc* f = reinterpret_cast<const dsl_aa_desc*>(d);
  if (f->max_gt < 1 || f->max_gt > (1 << 20) || d->n < 1) return 0;
  return ((size_t)f->max_gt * AA_REC + (size_t)d->n * 4) * sizeof(float);
}

namespace {

// a dsl_aa_desc the kernels build, or -1 with dsl_last_error naming the field
int aa_fill(const dsl_aa_desc* f, AaK& k, const char* who) {
  DSL_CHECK(f, "%s: null descriptor", who);
  const dsl_fcos_desc* d = &f->fcos;
  DSL_CHECK(d->head_flags == (DSL_HEAD_AUTOASSIGN | DSL_HEAD_LOSS_EXT),
            "%s: fcos.head_flags must be DSL_HEAD_AUTOASSIGN | DSL_HEAD_LOSS_EXT and nothing else (got %d)", who, d->head_flags);
  k = AaK{};
  if (head_fill(d, k, who)) return -1;
  DSL_CHECK(d->num_classes >= 1 && d->num_classes <= 128, "%s: fcos.num_classes must be in 1..128 (a lane owns two classes)", who);
  DSL_CHECK(!d->ig_boxes && !d->ig_off, "%s: fcos.ig_boxes / ig_off must be null (the head has no ignore boxes)", who);
  DSL_CHECK(d->soft_weight == 0.f, "%s: fcos.soft_weight must be 0 (no sisoft term)", who);
  DSL_CHECK(d->loss_weight == 1.0f, "%s: fcos.loss_weight must be 1 (no stream weight)", who);
  DSL_CHECK(!d->ctr && !d->g_ctr, "%s: fcos.ctr / g_ctr must be null (the objectness is regctr's column 4)", who);
  DSL_CHECK(f->max_gt >= 1 && f->max_gt <= (1 << 20), "%s: max_gt must be in 1..2^20 (the capacity of fcos.gt_boxes)", who);
  DSL_CHECK(f->w_pos >= 0.f && f->w_pos < 1e30f && f->w_neg >= 0.f && f->w_neg < 1e30f && f->w_center >= 0.f && f->w_center < 1e30f,
            "%s: w_pos / w_neg / w_center must be finite and >= 0", who);
  DSL_CHECK(d->gt_boxes && d->gt_labels && d->gt_off && f->mean && f->sigma, "%s: null pointer (ground truth, mean or sigma)", who);
  DSL_CHECK(((uintptr_t)d->gt_boxes & 15) == 0, "%s: fcos.gt_boxes must be 16-byte aligned", who);
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d) && ((uintptr_t)d->workspace & 15) == 0,
            "%s: fcos.workspace too small or not 16-byte aligned", who);
  k.w_pos = f->w_pos; k.w_neg = f->w_neg; k.w_center = f->w_center; k.max_gt = f->max_gt;
  k.gt_boxes = d->gt_boxes; k.gt_labels = (const long long*)d->gt_labels; k.gt_off = d->gt_off;
  k.mean = f->mean; k.sigma = f->sigma; k.g_mean = f->g_mean; k.g_sigma = f->g_sigma;
  k.iou = f->iou; k.stats = d->stats;
  k.box_rec = reinterpret_cast<float*>(static_cast<char*>(d->workspace) + (dsl_fcos_workspace_bytes(d) - dsl_aa_workspace_extra(d)));
  k.img_rec = k.box_rec + (size_t)f->max_gt * AA_REC;
  return 0;
}

}  // namespace

extern "C" int dsl_aa_assign(const dsl_aa_desc* f, void* stream) {
  AaK k;
  if (aa_fill(f, k, "dsl_aa_assign")) return -1;
  DSL_CHECK(f->fcos.stats, "dsl_aa_assign: fcos.stats is null");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(aa_box_kernel<0>, dim3((k.max_gt + 3) / 4), dim3(256), 0, st, k);
  hipLaunchKernelGGL(aa_assign_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k);
  DSL_LAUNCH_CHECK("aa_box_kernel");
  return 0;
}

extern "C" int dsl_aa_loss(const dsl_aa_desc* f, void* stream) {
  AaK k;
  if (aa_fill(f, k, "dsl_aa_loss")) return -1;
  const dsl_fcos_desc* d = &f->fcos;
  DSL_CHECK(d->cls_logits && d->regctr && d->scales && d->norm && d->g_cls && d->g_rc && d->g_scales && d->losses && f->g_mean && f->g_sigma &&
                f->iou, "dsl_aa_loss: null pointer (head outputs, scales, norm, gradients, losses or iou)");
  DSL_CHECK(d->ld_cls >= d->num_classes && d->ld_gcls >= d->num_classes, "dsl_aa_loss: fcos.ld_cls / ld_gcls must hold C columns");
  DSL_CHECK(d->ld_rc >= 8 && d->ld_rc % 4 == 0 && ((uintptr_t)d->regctr & 15) == 0,
            "dsl_aa_loss: fcos.ld_rc must be a multiple of 4 that holds the box and the objectness, regctr 16-byte aligned");
  DSL_CHECK(d->ld_grc >= 8 && d->ld_grc % 8 == 0 && ((uintptr_t)d->g_rc & 15) == 0,
            "dsl_aa_loss: fcos.ld_grc must be a multiple of 8, g_rc 16-byte aligned");
  DSL_CHECK(d->box_kind == DSL_BOX_GIOU, "dsl_aa_loss: fcos.box_kind must be DSL_BOX_GIOU");
  DSL_CHECK(d->w_bbox >= 0.f && d->w_bbox < 1e30f, "dsl_aa_loss: fcos.w_bbox must be finite and >= 0");
  k.w_bbox = d->w_bbox;
  hipStream_t st = (hipStream_t)stream;
  const int ngroup = (k.M + 3) / 4;
  const int blocks = ngroup > 2048 ? 2048 : ngroup;
  hipLaunchKernelGGL(aa_iou_kernel, dim3((k.M + 255) / 256), dim3(256), 0, st, k);
  hipLaunchKernelGGL(aa_box_kernel<1>, dim3((k.max_gt + 3) / 4), dim3(256), 0, st, k);
  hipLaunchKernelGGL(aa_image_kernel, dim3(1), dim3(64), 0, st, k);
  hipLaunchKernelGGL(aa_point_kernel, dim3(blocks), dim3(256), 0, st, k);
  hipLaunchKernelGGL(aa_box_kernel<2>, dim3((k.max_gt + 3) / 4), dim3(256), 0, st, k);
  hipLaunchKernelGGL(aa_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k, blocks);
  DSL_LAUNCH_CHECK("aa_point_kernel");
  return 0;
}
