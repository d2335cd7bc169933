// GFLHead on the HIP step: the quality pass (IoU score and weight of every positive, the second normaliser) and the loss pass
// (Quality Focal Loss, box loss and Distribution Focal Loss with their gradients, one launch) of a dsl_gfl_desc.
// Restates mmdet/models/dense_heads/gfl_head.py:15-48 (Integral), :210-296 (loss_single), :348-370 (avg_factor),
// mmdet/models/losses/gfocal_loss.py:11-78 (quality_focal_loss, distribution_focal_loss), mmdet/core/bbox/transforms.py:165-186
// (bbox2distance) and bbox_overlaps(is_aligned=True) (iou2d_calculator.py:212-260); semantics: include/dsl_hip.h.
// LDHead's loss pass (dsl_ld_loss on a dsl_ld_desc: ld_head.py:99-126,253-261, losses/kd_loss.py:27-35) is the same kernel with the
// Localization Distillation term behind a template argument.
//
// Positives are a few hundred among tens of thousands of locations, and each costs 4 (reg_max + 1) loads and exponentials.  They
// are neither compacted into a list (a second launch and an ordering to keep the sums reproducible) nor left to single lanes (a
// wavefront would run the 68-wide row serially for one active lane): each wavefront takes 64 consecutive locations, ballots its
// positives and processes them one after the other with all 64 lanes - 16 lanes per box side, two bins per lane, reductions inside
// the 16-lane group - so every branch is wavefront-uniform.  The rows of the non-positives are zeroed by the same wavefront with
// 16-byte stores, several rows per store.
#include "common.hpp"
#pragma clang fp contract(off)
#include "box_loss.hpp"
#include "head_common.hpp"

namespace {

struct GfK : HeadK {
  int R;                  // reg_max + 1
  float* score; float* weight;
  float beta, w_dfl;
  float tmax;             // reg_max - 0.1 (bbox2distance's clamp, transforms.py:183-184)
  // dsl_ld_loss only (gfl_loss_kernel<., true>; all zero otherwise)
  const float* soft; int ld_soft; const float* soft_scales;
  float T, w_ld;
};

// reductions inside a 16-lane group (one box side)
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One positive location, the whole wavefront: lane = 16 k + j holds bins j and j + 16 of side k (R <= 17).  raw = the predictor's
// logits, z = scale * raw, p = softmax(z_k), lse = log sum exp z_k, d[0..3] = the four sides' expectations (gfl_head.py:15-48).
struct GflRow {
  bool has0, has1;
  float raw0, raw1, z0, z1, p0, p1, lse, dk, d[4], sc;
};
__device__ __forceinline__ void gfl_row(const GfK& p, int m, int lvl, int lane, GflRow& o) {
  const int k = lane >> 4, j = lane & 15;
  o.has0 = j < p.R;
  o.has1 = j + 16 < p.R;
  const float* row = p.regctr + (long long)m * p.ld_rc + k * p.R;
  o.sc = p.scales[lvl];
  o.raw0 = o.has0 ? row[j] : 0.f;
  o.raw1 = o.has1 ? row[j + 16] : 0.f;
  o.z0 = o.raw0 * o.sc;
  o.z1 = o.raw1 * o.sc;
  const float ninf = -__builtin_inff();
  const float mx = group_max(fmaxf(o.has0 ? o.z0 : ninf, o.has1 ? o.z1 : ninf));      // (bins 0 and 1 always exist: finite)
  const float e0 = o.has0 ? expf(o.z0 - mx) : 0.f, e1 = o.has1 ? expf(o.z1 - mx) : 0.f;
  const float S = group_sum(e0 + e1);
  o.p0 = e0 / S;
  o.p1 = e1 / S;
  o.lse = mx + logf(S);
  o.dk = group_sum((float)j * o.p0 + (float)(j + 16) * o.p1);
#pragma unroll
  for (int q = 0; q < 4; ++q) o.d[q] = __shfl(o.dk, 16 * q, 64);
}

// softmax(v / T) and its logarithm over one side's bins (kd_loss.py:27-35: F.softmax(soft_label / T), F.log_softmax(pred / T)); the
// student's and the teacher's rows go through this one function, so equal rows give equal bits
__device__ __forceinline__ void ld_softmax(float v0, float v1, bool has0, bool has1, float T, float& p0, float& p1, float& l0, float& l1) {
  const float a0 = v0 / T, a1 = v1 / T;
  const float ninf = -__builtin_inff();
  const float mx = group_max(fmaxf(has0 ? a0 : ninf, has1 ? a1 : ninf));
  const float e0 = has0 ? expf(a0 - mx) : 0.f, e1 = has1 ? expf(a1 - mx) : 0.f;
  const float S = group_sum(e0 + e1);
  const float lS = logf(S);
  p0 = e0 / S;
  p1 = e1 / S;
  l0 = (a0 - mx) - lS;
  l1 = (a1 - mx) - lS;
}

__device__ __forceinline__ float gfl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- quality pass ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gfl_quality_kernel(const GfK p) {
  __shared__ float sh[16];
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int base = m - lane;
  const bool pos = m < p.M && (int)p.labels[m] < p.num_classes;
  float my_s = 0.f, my_w = 0.f;
  unsigned long long mask = __ballot(pos);
  while (mask) {
    const int r = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int mm = base + r;
    int lvl, img, y, x;
    head_loc(p, mm, lvl, img, y, x);
    GflRow o;
    gfl_row(p, mm, lvl, lane, o);
    const float s = (float)p.stride[lvl];
    const f32x4 t = *reinterpret_cast<const f32x4*>(p.bbox_targets + 4ll * mm);
    const float X1 = t[0] / s, Y1 = t[1] / s, X2 = t[2] / s, Y2 = t[3] / s;
    const float x1 = (float)x - o.d[0], y1 = (float)y - o.d[1], x2 = (float)x + o.d[2], y2 = (float)y + o.d[3];
    // bbox_overlaps(is_aligned=True), mode 'iou', eps 1e-6
    const float a1 = (x2 - x1) * (y2 - y1), a2 = (X2 - X1) * (Y2 - Y1);
    const float iw = fmaxf(fminf(x2, X2) - fmaxf(x1, X1), 0.f), ih = fmaxf(fminf(y2, Y2) - fmaxf(y1, Y1), 0.f);
    const float ov = iw * ih;
    const float iou = ov / fmaxf(a1 + a2 - ov, 1e-6f);
    // max_c sigmoid(cls): the sigmoid of the largest logit (sigmoid is monotonic)
    float best = -__builtin_inff();
    const float* c = p.cls_logits + (long long)mm * p.ld_cls;
    for (int i = lane; i < p.num_classes; i += 64) best = fmaxf(best, c[i]);
#pragma unroll
    for (int q = 32; q > 0; q >>= 1) best = fmaxf(best, __shfl_xor(best, q, 64));
    const float wv = gfl_sigmoid(best);
    if (lane == r) {
      my_s = iou;
      my_w = wv;
    }
  }
  if (m < p.M) {
    p.score[m] = my_s;
    p.weight[m] = my_w;
  }
  const float bs = block_sum(my_w, sh);
  if (threadIdx.x == 0) p.part[blockIdx.x] = bs;
}

// stats[1] = the sum of the block records (the weights), in block order
__global__ __launch_bounds__(REC_T) void gfl_quality_finalize_kernel(const GfK p, int nblocks, float* out) {
  __shared__ float sh[REC_T];
  const float t = record_sum(p.part, nblocks, 1, 0, 1, sh);
  if (threadIdx.x == 0) out[0] = t;
}

// ---- Quality Focal Loss of one logit and dloss/dx (gfocal_loss.py:11-52) ---------------------------------------------------------
// negative: BCE(x, 0) p^beta; the positive's label column: BCE(x, t) |t - p|^beta with t = the IoU score, a constant.
// d/dx = p^beta (beta q sp + p), and sign(p - t) (a^(beta + 1) + beta BCE p q a^(beta - 1)) with a = |t - p|; a == 0: 0.
__device__ __forceinline__ void qfl_fb(float x, bool pos, float t, float beta, bool beta2, float& loss, float& grad) {
  const float e = __expf(-fabsf(x));
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float pp = x >= 0.f ? inv : e * inv;   // sigmoid(x)
  const float q = x >= 0.f ? e * inv : inv;    // sigmoid(-x)
  if (!pos) {
    const float sp = fmaxf(x, 0.f) + l1p;      // -log(1 - p)
    const float mod = beta2 ? pp * pp : powf(pp, beta);
    loss = mod * sp;
    grad = mod * (beta * q * sp + pp);
    return;
  }
  const float bce = fmaxf(x, 0.f) - x * t + l1p;
  const float a = fabsf(t - pp);
  const float sg = pp > t ? 1.f : -1.f;
  if (beta2) {
    loss = bce * (a * a);
    grad = sg * a * (a * a + 2.f * bce * pp * q);
  } else if (a == 0.f) {
    loss = bce * powf(0.f, beta);
    grad = 0.f;
  } else {
    const float mod = powf(a, beta);
    loss = bce * mod;
    grad = sg * (mod * a + beta * bce * pp * q * (mod / a));
  }
}

// ---- loss pass: block records [cls, ld (0 without kLd), bbox, dfl, g_scale x 5, pad] ----------------------------------------------
// kLd (dsl_ld_loss, ld_head.py:99-126, kd_loss.py:27-35): per positive and side, T^2 / R KL(softmax(s / T) || softmax(z / T)) against the
// teacher's row s, weighted like the box terms; its gradient joins the row's in front of the bf16 rounding.  Compiled out of the GFL
// instantiations.
template <bool kTail, bool kLd>
__global__ __launch_bounds__(256) void gfl_loss_kernel(const GfK p) {
  __shared__ float sh[16];
  const int M = p.M, C = p.num_classes;
  const int c4 = kTail ? (C + 3) / 4 : C / 4;
  const float num = fmaxf(p.norm[0] * p.inv_world, 1.0f);
  const float avg = fmaxf(p.norm[1] * p.inv_world, 1.0f);
  const bool beta2 = p.beta == 2.f;

  // ---------------- QFL: one thread per 4 consecutive classes of one location ----------
  float lsum = 0.f;
  const long long total = (long long)M * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / c4);
    const int c = (int)(i - (long long)m * c4) * 4;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(p.cls_logits + (long long)m * p.ld_cls + c);
    const int label = (int)p.labels[m];
    const float wgt = p.cls_weight[m];
    const float gs = wgt / num * p.grad_scale * p.w_cls;
    const bool mine = label >= c && label < c + 4 && label < C;
    const float sc = mine ? p.score[m] : 0.f;
    float g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float l, d;
      qfl_fb(xv[e], mine && label == c + e, sc, p.beta, beta2, l, d);
      if (kTail && c + e >= C) l = d = 0.f;
      lsum += l * wgt;
      g[e] = d * gs;
    }
    u32x2 o = {pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
    *reinterpret_cast<u32x2*>(p.g_cls + (long long)m * p.ld_gcls + c) = o;
  }
  lsum = block_sum(lsum, sh);
  float* rec = p.part + 16ll * blockIdx.x;
  if (threadIdx.x == 0) {
    rec[0] = lsum;
    if constexpr (!kLd) rec[1] = 0.f;
  }

  // ---------------- boxes + DFL: one wavefront per 64 consecutive locations ----------------------
  float bsum = 0.f, dsum = 0.f;
  [[maybe_unused]] float ksum = 0.f;
  float gsc[DSL_MAX_SEG] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane >> 4, j = lane & 15;
  const int nchunk = (M + 63) / 64;
  const int lpr = p.ld_grc / 8;          // 16-byte stores per row of g_rc (a power of two <= 64)
  const int rps = 64 / lpr;              // rows per wavefront store
  for (int ch = blockIdx.x * 4 + wave; ch < nchunk; ch += gridDim.x * 4) {
    const int base = ch * 64;
    const int m = base + lane;
    const bool pos = m < M && (int)p.labels[m] < C;
    unsigned long long mask = __ballot(pos);
    for (int r0 = 0; r0 < 64; r0 += rps) {
      const int r = r0 + lane / lpr;
      if (base + r < M && !((mask >> r) & 1ull))
        *reinterpret_cast<u32x4*>(p.g_rc + (long long)(base + r) * p.ld_grc + (lane % lpr) * 8) = u32x4{0u, 0u, 0u, 0u};
    }
    while (mask) {
      const int r = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int mm = base + r;
      int lvl, img, y, x;
      head_loc(p, mm, lvl, img, y, x);
      GflRow o;
      gfl_row(p, mm, lvl, lane, o);
      const float s = (float)p.stride[lvl];
      const f32x4 t = *reinterpret_cast<const f32x4*>(p.bbox_targets + 4ll * mm);
      const float X1 = t[0] / s, Y1 = t[1] / s, X2 = t[2] / s, Y2 = t[3] / s;
      const float fx = (float)x, fy = (float)y;
      const float x1 = fx - o.d[0], y1 = fy - o.d[1], x2 = fx + o.d[2], y2 = fy + o.d[3];
      const float wv = p.weight[mm];
      float dl[4];
      const float bl = p.box_kind <= DSL_BOX_IOU_LOG ? box_loss_giou(p.box_kind == DSL_BOX_IOU_LOG, x1, y1, x2, y2, X1, Y1, X2, Y2, dl)
                                                     : box_loss_ext(p.box_kind, p.box_eps, x1, y1, x2, y2, X1, Y1, X2, Y2, dl);
      const float coef_b = wv / avg * p.grad_scale * p.w_bbox;
      const float coef_d = wv / avg * p.grad_scale * p.w_dfl * 0.25f;
      // x1 = x - d0, y1 = y - d1, x2 = x + d2, y2 = y + d3
      const float ddk = coef_b != 0.f ? coef_b * (k == 0 ? -dl[0] : k == 1 ? -dl[1] : k == 2 ? dl[2] : dl[3]) : 0.f;
      // DFL (gfocal_loss.py:55-78) against bbox2distance's clamped target of this side
      const float td = k == 0 ? fx - X1 : k == 1 ? fy - Y1 : k == 2 ? X2 - fx : Y2 - fy;
      const float tt = fminf(fmaxf(td, 0.f), p.tmax);
      const float lf = floorf(tt);
      const int li = (int)lf;
      const float wl = (lf + 1.f) - tt, wr = tt - lf;
      const float s0 = j == li ? wl : (j == li + 1 ? wr : 0.f);
      const float s1 = j + 16 == li ? wl : (j + 16 == li + 1 ? wr : 0.f);
      const float zt = group_sum((o.has0 ? s0 * o.z0 : 0.f) + (o.has1 ? s1 * o.z1 : 0.f));
      const float dfl = o.lse * wl + o.lse * wr - zt;      // CE(z, l) wl + CE(z, l + 1) wr
      float g0 = o.has0 ? ddk * (o.p0 * ((float)j - o.dk)) + coef_d * (o.p0 * wl + o.p0 * wr - s0) : 0.f;
      float g1 = o.has1 ? ddk * (o.p1 * ((float)(j + 16) - o.dk)) + coef_d * (o.p1 * wl + o.p1 * wr - s1) : 0.f;
      if constexpr (kLd) {
        const float* srow = p.soft + (long long)mm * p.ld_soft + k * p.R;
        const float ssc = p.soft_scales[lvl];
        const float s0r = o.has0 ? srow[j] : 0.f, s1r = o.has1 ? srow[j + 16] : 0.f;
        float q0, q1, lq0, lq1, t0, t1, lt0, lt1;
        ld_softmax(o.z0, o.z1, o.has0, o.has1, p.T, q0, q1, lq0, lq1);
        ld_softmax(s0r * ssc, s1r * ssc, o.has0, o.has1, p.T, t0, t1, lt0, lt1);
        // F.kl_div: target (log target - input), 0 where the target is 0; .mean(1) * T^2
        const float kl = group_sum((t0 > 0.f ? t0 * (lt0 - lq0) : 0.f) + (t1 > 0.f ? t1 * (lt1 - lq1) : 0.f));
        const float kd = kl * (p.T * p.T) / (float)p.R;
        // d kd / d z_j = T / R (p_j - t_j); not divided by avg (ld_head.py:253-261 leaves loss_ld as weighted_loss returned it)
        const float coef_l = wv * p.grad_scale * p.w_ld * 0.25f * (p.T / (float)p.R);
        const float a0 = coef_l * (q0 - t0), a1 = coef_l * (q1 - t1);
        if (o.has0 && a0 != 0.f) g0 += a0;      // (a zero term leaves the row's bits alone, the sign of a zero included)
        if (o.has1 && a1 != 0.f) g1 += a1;
        if (j == 0) ksum += wv * kd;
      }
      uint16_t* gr = p.g_rc + (long long)mm * p.ld_grc + k * p.R;
      if (o.has0) gr[j] = f2bf(g0 * o.sc);
      if (o.has1) gr[j + 16] = f2bf(g1 * o.sc);
      // the row's padding columns 4R .. ld_grc: zero, so that every row of g_rc is rewritten whole by every launch
      for (int i = 4 * p.R + lane; i < p.ld_grc; i += 64) p.g_rc[(long long)mm * p.ld_grc + i] = 0;
      const float gs = g0 * o.raw0 + g1 * o.raw1;
#pragma unroll
      for (int l = 0; l < DSL_MAX_SEG; ++l) gsc[l] += l == lvl ? gs : 0.f;
      if (lane == 0) bsum += wv * bl;
      if (j == 0) dsum += wv * dfl;
    }
  }
  bsum = block_sum(bsum, sh);
  dsum = block_sum(dsum, sh);
  if (threadIdx.x == 0) {
    rec[2] = bsum;
    rec[3] = dsum;
  }
  if constexpr (kLd) {
    ksum = block_sum(ksum, sh);
    if (threadIdx.x == 0) rec[1] = ksum;
  }
#pragma unroll
  for (int l = 0; l < DSL_MAX_SEG; ++l) {
    const float v = block_sum(gsc[l], sh);
    if (threadIdx.x == 0) rec[4 + l] = v;
  }
#pragma unroll
  for (int l = 4 + DSL_MAX_SEG; l < 16; ++l)
    if (threadIdx.x == 0) rec[l] = 0.f;
}

// fixed-order sum of the 16-float block records -> losses[4] (cls, bbox, dfl, 0), g_scales[5], logvec[4] (cls, bbox, dfl, their sum);
// kLd: losses[3] = w_ld / 4 * the records' LD sums (no normaliser), logvec[5] (cls, bbox, dfl, ld, their sum)
template <bool kLd>
__global__ __launch_bounds__(REC_T) void gfl_finalize_kernel(const GfK p, int nblocks) {
  __shared__ float sh[REC_T];
  const float t = record_sum(p.part, nblocks, 16, 0, 16, sh);
  if (threadIdx.x < 16) {
    const float num = fmaxf(p.norm[0] * p.inv_world, 1.0f), avg = fmaxf(p.norm[1] * p.inv_world, 1.0f);
    float fv = 0.f;
    if (threadIdx.x == 0) p.losses[0] = fv = t / num * p.w_cls;
    else if (threadIdx.x == 1) p.losses[3] = fv = kLd ? t * (p.w_ld * 0.25f) : 0.f;
    else if (threadIdx.x == 2) p.losses[1] = fv = t / avg * p.w_bbox;
    else if (threadIdx.x == 3) p.losses[2] = fv = t / avg * (p.w_dfl * 0.25f);
    else if (threadIdx.x - 4 < DSL_MAX_SEG) p.g_scales[threadIdx.x - 4] = t;
    if (threadIdx.x < 4) sh[threadIdx.x] = fv;
  }
  if (p.logvec) {      // the log vector of _parse_losses (detectors/base.py:175-208): the loss terms and their sum
    __syncthreads();
    if (threadIdx.x == 0) {
      const float cls = sh[0], bbox = sh[2], dfl = sh[3];
      p.logvec[0] = cls; p.logvec[1] = bbox; p.logvec[2] = dfl;
      if constexpr (kLd) {
        p.logvec[3] = sh[1];
        p.logvec[4] = ((cls + bbox) + dfl) + sh[1];
      } else {
        p.logvec[3] = (cls + bbox) + dfl;
      }
    }
  }
}

int gfl_fill(const dsl_gfl_desc* g, GfK& k, const char* who) {
  DSL_CHECK(g, "%s: null descriptor", who);
  const dsl_fcos_desc* d = &g->fcos;
  DSL_CHECK(d->nlvl >= 1 && d->nlvl <= DSL_MAX_SEG && d->n >= 1 && d->num_classes >= 1, "%s: bad descriptor", who);
  DSL_CHECK((d->head_flags & DSL_HEAD_GFL) && (d->head_flags & DSL_HEAD_ATSS) && (d->head_flags & DSL_HEAD_LOSS_EXT),
            "%s: a dsl_gfl_desc needs DSL_HEAD_GFL | DSL_HEAD_ATSS | DSL_HEAD_LOSS_EXT in fcos.head_flags", who);
  DSL_CHECK((d->head_flags & (DSL_HEAD_INSIDE_BOX | DSL_HEAD_RAW_TARGETS | DSL_HEAD_EXP_DECODE)) == 0,
            "%s: DSL_HEAD_GFL goes with no FCOS assignment / decode flag", who);      // (DSL_HEAD_IOU_LOSS: replaced by fcos.box_kind)
  DSL_CHECK(!d->ctr && !d->g_ctr, "%s: a GFL head has no centerness", who);
  DSL_CHECK(d->loss_weight == 1.0f && d->soft_weight == 0.f, "%s: no DSL stream weight / sisoft term", who);
  DSL_CHECK(g->reg_max >= 1 && g->reg_max <= DSL_GFL_MAX_REG, "%s: reg_max must be in 1..%d, got %d", who, DSL_GFL_MAX_REG, g->reg_max);
  k = GfK{};
  if (head_fill(d, k, who)) return -1;
  k.R = g->reg_max + 1;
  DSL_CHECK(d->labels && d->bbox_targets && d->cls_weight && d->cls_logits && d->regctr && d->scales && d->stats && g->score && g->weight,
            "%s: null pointer", who);
  DSL_CHECK(d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_rc >= 4 * k.R, "%s: ld_cls / ld_rc do not hold C / 4 (reg_max + 1) columns", who);
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d) && ((uintptr_t)d->workspace & 15) == 0,
            "%s: workspace too small or not 16-byte aligned", who);
  k.score = g->score; k.weight = g->weight;
  k.tmax = (float)((double)g->reg_max - 0.1);
  return 0;
}

// what the loss passes check and fill beyond gfl_fill
int gfl_loss_fill(const dsl_gfl_desc* g, GfK& k, const char* who) {
  if (gfl_fill(g, k, who)) return -1;
  const dsl_fcos_desc* d = &g->fcos;
  if (head_loss_ptrs(d, who)) return -1;
  DSL_CHECK(d->ld_gcls % 4 == 0 && d->ld_gcls >= d->ld_cls, "%s: ld_gcls must be a multiple of 4 and >= ld_cls", who);
  DSL_CHECK(d->ld_grc >= 8 && d->ld_grc <= 512 && (d->ld_grc & (d->ld_grc - 1)) == 0 && d->ld_grc >= 4 * k.R && ((uintptr_t)d->g_rc & 15) == 0,
            "%s: ld_grc must be a power of two in 8..512 and >= 4 (reg_max + 1), g_rc 16-byte aligned", who);
  if (head_loss_settings(d, g->w_dfl, k, who)) return -1;
  DSL_CHECK(g->qfl_beta >= 0.f && g->qfl_beta < 1e30f, "%s: qfl_beta must be finite and >= 0", who);
  k.beta = g->qfl_beta; k.w_dfl = g->w_dfl;
  return 0;
}

// the loss kernel [C % 4 != 0][LD] and the sum of its records
void gfl_loss_launch(const GfK& k, bool ld, hipStream_t st) {
  static void (*const kernel[2][2])(const GfK) = {{gfl_loss_kernel<false, false>, gfl_loss_kernel<false, true>},
                                                  {gfl_loss_kernel<true, false>, gfl_loss_kernel<true, true>}};
  const int blocks = head_loss_blocks(k);
  hipLaunchKernelGGL(kernel[k.num_classes % 4 != 0][ld], dim3(blocks), dim3(256), 0, st, k);
  hipLaunchKernelGGL(ld ? gfl_finalize_kernel<true> : gfl_finalize_kernel<false>, dim3(1), dim3(REC_T), 0, st, k, blocks);
}

}  // namespace

extern "C" int dsl_gfl_quality(const dsl_gfl_desc* g, void* stream) {
  GfK k;
  if (gfl_fill(g, k, "dsl_gfl_quality")) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (k.M + 255) / 256;      // (<= the workspace's (M + 255) / 256 * 2 floats)
  hipLaunchKernelGGL(gfl_quality_kernel, dim3(nb), dim3(256), 0, st, k);
  hipLaunchKernelGGL(gfl_quality_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k, nb, g->fcos.stats + 1);
  DSL_LAUNCH_CHECK("gfl_quality_kernel");
  return 0;
}

extern "C" int dsl_gfl_loss(const dsl_gfl_desc* g, void* stream) {
  GfK k;
  if (gfl_loss_fill(g, k, "dsl_gfl_loss")) return -1;
  gfl_loss_launch(k, false, (hipStream_t)stream);
  DSL_LAUNCH_CHECK("gfl_loss_kernel");
  return 0;
}

extern "C" int dsl_ld_loss(const dsl_ld_desc* l, void* stream) {
  DSL_CHECK(l, "dsl_ld_loss: null descriptor");
  const dsl_gfl_desc* g = &l->gfl;
  DSL_CHECK((g->fcos.head_flags & DSL_HEAD_LD) && (g->fcos.head_flags & DSL_HEAD_GFL),
            "dsl_ld_loss: a dsl_ld_desc needs DSL_HEAD_LD | DSL_HEAD_GFL in gfl.fcos.head_flags");
  GfK k;
  if (gfl_loss_fill(g, k, "dsl_ld_loss")) return -1;
  DSL_CHECK(l->soft && l->soft_scales, "dsl_ld_loss: soft / soft_scales null");
  DSL_CHECK(l->ld_soft >= 4 * k.R, "dsl_ld_loss: ld_soft does not hold 4 (reg_max + 1) columns (got %d)", l->ld_soft);
  DSL_CHECK(l->T >= 1.f && l->T < 1e30f, "dsl_ld_loss: T must be finite and >= 1");
  DSL_CHECK(l->w_ld >= 0.f && l->w_ld < 1e30f, "dsl_ld_loss: w_ld must be finite and >= 0");
  k.soft = l->soft; k.ld_soft = l->ld_soft; k.soft_scales = l->soft_scales; k.T = l->T; k.w_ld = l->w_ld;
  gfl_loss_launch(k, true, (hipStream_t)stream);
  DSL_LAUNCH_CHECK("gfl_loss_kernel");
  return 0;
}
