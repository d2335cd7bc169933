// FoveaHead on the HIP step: the target assignment (painted fovea rectangles, smallest covering box) and the loss pass (focal loss
// and SmoothL1 on log distances with their gradients, one launch) of a dsl_fovea_desc.
// Restates mmdet/models/dense_heads/fovea_head.py:130-132 (points), :134-182 (loss), :206-265 (_get_target_single),
// mmdet/models/losses/smooth_l1_loss.py:11-29 and losses/focal_loss.py:11-56; semantics, tie rule and refusals: include/dsl_hip.h.
//
// The assignment's decisions (the level a box hits, the rectangle it paints) must be the reference's fp32 torch arithmetic: the file
// is compiled with floating-point contraction off, every sum and product of the ceil / floor arguments is a separate operation in
// the reference's order, and sqrtf and the divisions are the correctly rounded ones (hipcc's default; no fast-math flag here).
// logf is the device library's: the log targets agree with torch's to a few ulps, which is what the tests ask.
#include "common.hpp"
#pragma clang fp contract(off)
#include "head_common.hpp"

namespace {

constexpr int FV_CH = 64;      // boxes staged per LDS chunk, by the workgroup's first wavefront (COCO images hold 7 boxes on average)

struct FvK : HeadK {
  float base_len[DSL_MAX_SEG], lo[DSL_MAX_SEG], hi[DSL_MAX_SEG];
  float oms, ops;         // 1 - sigma, 1 + sigma: formed in fp64 and rounded once, as the reference's Python floats are
  float beta, gamma, alpha;
  int pow2;               // every stride is a power of two: box / stride is formed as box * (1 / stride), the same bits (see the kernel)
  const float* gt_boxes; const long long* gt_labels; const int* gt_off;
  int* assign_idx; float* pos_weight; float* stats;
};

// ---- assignment: one thread per location; block record = the workgroup's positives --------------------------------------------------
// A workgroup's 256 consecutive locations lie in one image, or in several images and levels (the small levels): it stages a range
// [gmin, gmax) that holds its locations' box ranges chunk by chunk, and each thread scans the part of a chunk that belongs to its image.
__global__ __launch_bounds__(256) void fovea_assign_kernel(const FvK p) {
  __shared__ f32x4 sbox[FV_CH];
  __shared__ float sarea[FV_CH];
  __shared__ int slabel[FV_CH];
  __shared__ float sh[16];
  const int m = blockIdx.x * 256 + threadIdx.x;
  const bool live = m < p.M;
  int lvl = 0, img = 0, y = 0, x = 0, g0 = 0, g1 = 0;
  if (live) {
    head_loc(p, m, lvl, img, y, x);
    g0 = p.gt_off[img];
    g1 = p.gt_off[img + 1];
  }
  // the union of the workgroup's box ranges, from its first and last location - workgroup-uniform without a barrier, every thread
  // runs the chunk loop and its barriers: inside a level the images are consecutive; across a level boundary, the whole batch
  const int m_first = blockIdx.x * 256, m_last = m_first + 255 < p.M ? m_first + 255 : p.M - 1;
  int l_first, i_first, l_last, i_last, yy, xx;
  head_loc(p, m_first, l_first, i_first, yy, xx);
  head_loc(p, m_last, l_last, i_last, yy, xx);
  const int gmin = p.gt_off[l_first == l_last ? i_first : 0], gmax = p.gt_off[l_first == l_last ? i_last + 1 : p.n];

  // gt_bboxes_raw / stride (:233).  A power-of-two stride (8 .. 128 in every config): the product with its reciprocal, which is exact,
  // is the correctly rounded quotient - the same bits as the division for every box coordinate that is not subnormal - at a
  // fraction of its instructions; any other stride divides
  const float fs = (float)p.stride[lvl], inv = 1.f / fs;
  const float lo = p.lo[lvl], hi = p.hi[lvl];
  const float xmax = (float)(p.w[lvl] - 1), ymax = (float)(p.h[lvl] - 1);
  const float fx = (float)x, fy = (float)y;
  float best = __builtin_inff();
  int best_g = -1, best_label = 0;
  f32x4 best_b = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = gmin; c0 < gmax; c0 += FV_CH) {
    __syncthreads();      // the previous chunk is consumed
    const int gs = c0 + (int)threadIdx.x;
    if (threadIdx.x < FV_CH && gs < gmax) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * gs);
      sbox[threadIdx.x] = b;
      sarea[threadIdx.x] = sqrtf((b[2] - b[0]) * (b[3] - b[1]));      // gt_areas (fovea_head.py:212-213)
      slabel[threadIdx.x] = (int)p.gt_labels[gs];
    }
    __syncthreads();
    const int ga = g0 > c0 ? g0 : c0, gb = g1 < c0 + FV_CH ? g1 : c0 + FV_CH;
    for (int g = ga; g < gb; ++g) {
      const float area = sarea[g - c0];
      if (!(area >= lo && area <= hi)) continue;      // scale assignment (:225-226); a NaN area hits nothing
      // painted in order of decreasing area, so the smallest covering hit stays; equal areas: the higher index (header: unpinned)
      if (!(area <= best)) continue;
      const f32x4 b = sbox[g - c0];
      const float bx1 = p.pow2 ? b[0] * inv : b[0] / fs, by1 = p.pow2 ? b[1] * inv : b[1] / fs;
      const float bx2 = p.pow2 ? b[2] * inv : b[2] / fs, by2 = p.pow2 ? b[3] * inv : b[3] / fs;
      const float hw = 0.5f * (bx2 - bx1), hh = 0.5f * (by2 - by1);
      // (:238-249) ((x1 + (1 -+ sigma) * half) - 0.5), then ceil / floor, then the clamp to the level
      const float l = fminf(fmaxf(ceilf(bx1 + p.oms * hw - 0.5f), 0.f), xmax);
      const float r = fminf(fmaxf(floorf(bx1 + p.ops * hw - 0.5f), 0.f), xmax);
      const float t = fminf(fmaxf(ceilf(by1 + p.oms * hh - 0.5f), 0.f), ymax);
      const float d = fminf(fmaxf(floorf(by1 + p.ops * hh - 0.5f), 0.f), ymax);
      // labels[py1:py2 + 1, px1:px2 + 1]: empty when either range is empty after the clamp
      if (l <= r && t <= d && fx >= l && fx <= r && fy >= t && fy <= d) {
        best = area;
        best_g = g;
        best_b = b;
        best_label = slabel[g - c0];
      }
    }
  }

  float is_pos = 0.f;
  if (live) {
    long long label = p.num_classes;
    f32x4 tg = {0.f, 0.f, 0.f, 0.f};
    if (best_g >= 0) {
      is_pos = 1.f;
      label = best_label;
      const f32x4 b = best_b;
      const float px = fs * (fx + 0.5f), py = fs * (fy + 0.5f);      // (:130-132)
      const float bl = p.base_len[lvl];
      const float raw[4] = {(px - b[0]) / bl, (py - b[1]) / bl, (b[2] - px) / bl, (b[3] - py) / bl};      // (:254-261)
#pragma unroll
      for (int k = 0; k < 4; ++k) tg[k] = logf(fminf(fmaxf(raw[k], 1.f / 16.f), 16.f));      // (:262-264)
    }
    p.labels[m] = label;
    p.assign_idx[m] = best_g >= 0 ? best_g - g0 : -1;
    *reinterpret_cast<f32x4*>(p.bbox_targets + 4ll * m) = tg;
    p.cls_weight[m] = 1.f;
    p.pos_weight[m] = 1.f;
  }
  const float np = block_sum(is_pos, sh);      // (<= 256: exact)
  if (threadIdx.x == 0) p.part[blockIdx.x] = np;
}

// stats[0] = num_pos + n, stats[1] = max(num_pos, 1) from the workgroups' counts added in workgroup order (exact in fp32 below 2^24
// positives); stats[2..7] are reserved, kept zero
__global__ __launch_bounds__(REC_T) void fovea_assign_finalize_kernel(const FvK p, int nblocks) {
  __shared__ float sh[REC_T];
  const float t = record_sum(p.part, nblocks, 1, 0, 1, sh);
  if (threadIdx.x == 0) {
    p.stats[0] = t + (float)p.n;
    p.stats[1] = fmaxf(t, 1.f);
  }
  if (threadIdx.x >= 2 && threadIdx.x < 8) p.stats[threadIdx.x] = 0.f;
}

// ---- focal loss and dloss/dx of one logit, gamma >= 0, 0 <= alpha <= 1 (focal_loss.py:34-40) ------------------------------------------
// gamma == 2 (launch-uniform): the default head's q * q sequence.  Otherwise the modulating factor is exp(-gamma * softplus) - p^gamma
// = exp(gamma log p) from the -log p = softplus(-x) that the other branch's loss term needs anyway - one exponential per logit, where
// FocalLoss(gamma=1.5) of configs/foveabox would cost a powf; the gradient is formed as -+alpha q^gamma (gamma p sp + q), without
// q^(gamma - 1), so it is finite for gamma < 1 at a saturated sigmoid (the loss family's rule).  gamma == 0: exp(-0) = 1, as pow(x, 0).
__device__ __forceinline__ void fovea_focal_fb(float x, bool t, float gamma, float alpha, bool gamma2, float& loss, float& grad) {
  const float e = __expf(-fabsf(x));
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float pp = x >= 0.f ? inv : e * inv;      // sigmoid(x)
  const float q = x >= 0.f ? e * inv : inv;       // sigmoid(-x)
  const float nlp = fmaxf(-x, 0.f) + l1p, nlq = fmaxf(x, 0.f) + l1p;      // -log p, -log(1 - p)
  if (t) {
    const float mod = gamma2 ? q * q : __expf(-gamma * nlq);
    loss = alpha * mod * nlp;
    grad = -alpha * mod * (gamma * pp * nlp + q);
  } else {
    const float mod = gamma2 ? pp * pp : __expf(-gamma * nlp);
    loss = (1.f - alpha) * mod * nlq;
    grad = (1.f - alpha) * mod * (gamma * q * nlq + pp);
  }
}

// ---- loss pass: block records [cls, 0, bbox, 0 ...] of 16 floats ------------------------------------------------------------------
// kTail: C % 4 != 0, the last group of 4 classes of a location is partial; its lanes c + e >= C add no loss, write 0 into g_cls and
// do not use what they loaded (the logit rows' padding may hold anything).
template <bool kTail>
__global__ __launch_bounds__(256) void fovea_loss_kernel(const FvK p) {
  __shared__ float sh[16];
  const int M = p.M, C = p.num_classes;
  const int c4 = kTail ? (C + 3) / 4 : C / 4;
  const float num = fmaxf(p.norm[0] * p.inv_world, 1.0f);      // num_pos + num_imgs
  const float avg = fmaxf(p.norm[1] * p.inv_world, 1.0f);      // num_pos
  const bool gamma2 = p.gamma == 2.f;

  // ---------------- focal loss: one thread per 4 consecutive classes of one location ----------
  float lsum = 0.f;
  const long long total = (long long)M * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / c4);
    const int c = (int)(i - (long long)m * c4) * 4;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(p.cls_logits + (long long)m * p.ld_cls + c);
    const int label = (int)p.labels[m];
    const float wgt = p.cls_weight[m];
    const float gs = wgt / num * p.grad_scale * p.w_cls;
    float g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float l = 0.f, d = 0.f;
      if (!kTail || c + e < C) fovea_focal_fb(xv[e], label == c + e, p.gamma, p.alpha, gamma2, l, d);
      lsum += l * wgt;
      g[e] = d * gs;
    }
    u32x2 o = {pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
    *reinterpret_cast<u32x2*>(p.g_cls + (long long)m * p.ld_gcls + c) = o;
  }
  lsum = block_sum(lsum, sh);
  float* rec = p.part + 16ll * blockIdx.x;
  if (threadIdx.x == 0) rec[0] = lsum;

  // ---------------- SmoothL1 on the log distances: a wavefront walks 64 consecutive locations, one per lane ------------------------
  float bsum = 0.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = (M + 63) / 64;
  const float coef = p.w_bbox / avg * p.grad_scale;
  for (int ch = blockIdx.x * 4 + wave; ch < nchunk; ch += gridDim.x * 4) {
    const int m = ch * 64 + lane;
    if (m >= M) continue;
    float gr[4] = {0.f, 0.f, 0.f, 0.f};
    if ((int)p.labels[m] < C) {
      const f32x4 pr = *reinterpret_cast<const f32x4*>(p.regctr + (long long)m * p.ld_rc);
      const f32x4 tg = *reinterpret_cast<const f32x4*>(p.bbox_targets + 4ll * m);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = pr[k] - tg[k];
        const float a = fabsf(d);
        if (a < p.beta) {      // smooth_l1_loss.py:26-27
          bsum += 0.5f * a * a / p.beta;
          gr[k] = coef != 0.f ? coef * (d / p.beta) : 0.f;
        } else {
          bsum += a - 0.5f * p.beta;
          gr[k] = coef != 0.f ? (d > 0.f ? coef : -coef) : 0.f;
        }
      }
    }
    u32x4 o = {pack2bf(gr[0], gr[1]), pack2bf(gr[2], gr[3]), 0u, 0u};
    *reinterpret_cast<u32x4*>(p.g_rc + (long long)m * p.ld_grc) = o;
  }
  bsum = block_sum(bsum, sh);
  if (threadIdx.x == 0) {
    rec[1] = 0.f;
    rec[2] = bsum;
  }
  if (threadIdx.x >= 3 && threadIdx.x < 16) rec[threadIdx.x] = 0.f;
}

// fixed-order sum of the block records -> losses[4] (cls, bbox, 0, 0) and logvec[3] (cls, bbox, their sum)
__global__ __launch_bounds__(REC_T) void fovea_finalize_kernel(const FvK p, int nblocks) {
  __shared__ float sh[REC_T];
  const float t = record_sum(p.part, nblocks, 16, 0, 4, sh);
  if (threadIdx.x < 4) {
    const float num = fmaxf(p.norm[0] * p.inv_world, 1.0f), avg = fmaxf(p.norm[1] * p.inv_world, 1.0f);
    float fv = 0.f;
    if (threadIdx.x == 0) p.losses[0] = fv = t / num * p.w_cls;
    else if (threadIdx.x == 2) p.losses[1] = fv = t / avg * p.w_bbox;
    else p.losses[threadIdx.x == 1 ? 2 : 3] = 0.f;
    sh[threadIdx.x] = fv;
  }
  if (p.logvec) {      // the log vector of _parse_losses (detectors/base.py:175-208): the loss terms and their sum
    __syncthreads();
    if (threadIdx.x == 0) {
      p.logvec[0] = sh[0];
      p.logvec[1] = sh[2];
      p.logvec[2] = sh[0] + sh[2];
    }
  }
}

// a dsl_fovea_desc the kernels build, or -1 with dsl_last_error naming the field
int fovea_fill(const dsl_fovea_desc* f, FvK& k, const char* who) {
  DSL_CHECK(f, "%s: null descriptor", who);
  const dsl_fcos_desc* d = &f->fcos;
  DSL_CHECK(d->head_flags == (DSL_HEAD_FOVEA | DSL_HEAD_LOSS_EXT),
            "%s: fcos.head_flags must be DSL_HEAD_FOVEA | DSL_HEAD_LOSS_EXT and nothing else (got %d)", who, d->head_flags);
  k = FvK{};
  if (head_fill(d, k, who)) return -1;
  DSL_CHECK(d->num_classes >= 1, "%s: fcos.num_classes must be >= 1", who);
  DSL_CHECK(!d->ig_boxes && !d->ig_off, "%s: fcos.ig_boxes / ig_off must be null (the head has no ignore boxes)", who);
  DSL_CHECK(d->soft_weight == 0.f, "%s: fcos.soft_weight must be 0 (no sisoft term)", who);
  DSL_CHECK(d->loss_weight == 1.0f, "%s: fcos.loss_weight must be 1 (no stream weight)", who);
  DSL_CHECK(!d->ctr && !d->g_ctr, "%s: fcos.ctr / g_ctr must be null (the head has no centerness)", who);
  DSL_CHECK(f->sigma > 0.f && f->sigma <= 1.f, "%s: sigma must be in (0, 1]", who);
  DSL_CHECK(f->smooth_l1_beta > 0.f && f->smooth_l1_beta < 1e30f, "%s: smooth_l1_beta must be finite and > 0", who);
  for (int l = 0; l < d->nlvl; ++l) {
    DSL_CHECK(f->base_len[l] > 0.f && f->base_len[l] < 1e30f, "%s: base_len[%d] must be finite and > 0", who, l);
    DSL_CHECK(f->lo[l] <= f->hi[l], "%s: lo[%d] > hi[%d] (or a NaN bound)", who, l, l);
    k.base_len[l] = f->base_len[l]; k.lo[l] = f->lo[l]; k.hi[l] = f->hi[l];
  }
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d) && ((uintptr_t)d->workspace & 15) == 0,
            "%s: fcos.workspace too small or not 16-byte aligned", who);
  k.oms = (float)(1.0 - (double)f->sigma);
  k.ops = (float)(1.0 + (double)f->sigma);
  k.beta = f->smooth_l1_beta;
  k.pow2 = 1;
  for (int l = 0; l < d->nlvl; ++l) k.pow2 &= (d->stride[l] & (d->stride[l] - 1)) == 0;
  k.gt_boxes = d->gt_boxes; k.gt_labels = (const long long*)d->gt_labels; k.gt_off = d->gt_off;
  k.assign_idx = d->assign_idx; k.pos_weight = d->pos_weight; k.stats = d->stats;
  return 0;
}

}  // namespace

extern "C" int dsl_fovea_assign(const dsl_fovea_desc* f, void* stream) {
  FvK k;
  if (fovea_fill(f, k, "dsl_fovea_assign")) return -1;
  const dsl_fcos_desc* d = &f->fcos;
  DSL_CHECK(d->gt_boxes && d->gt_labels && d->gt_off && d->labels && d->bbox_targets && d->assign_idx && d->cls_weight && d->pos_weight &&
                d->stats, "dsl_fovea_assign: null pointer in fcos (ground truth, targets or stats)");
  DSL_CHECK(((uintptr_t)d->gt_boxes & 15) == 0 && ((uintptr_t)d->bbox_targets & 15) == 0,
            "dsl_fovea_assign: fcos.gt_boxes / bbox_targets must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (k.M + 255) / 256;
  hipLaunchKernelGGL(fovea_assign_kernel, dim3(nb), dim3(256), 0, st, k);
  hipLaunchKernelGGL(fovea_assign_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k, nb);
  DSL_LAUNCH_CHECK("fovea_assign_kernel");
  return 0;
}

extern "C" int dsl_fovea_loss(const dsl_fovea_desc* f, void* stream) {
  FvK k;
  if (fovea_fill(f, k, "dsl_fovea_loss")) return -1;
  const dsl_fcos_desc* d = &f->fcos;
  DSL_CHECK(d->labels && d->bbox_targets && d->cls_weight && d->cls_logits && d->regctr && d->norm && d->g_cls && d->g_rc && d->losses,
            "dsl_fovea_loss: null pointer in fcos (targets, head outputs, norm, gradients or losses)");
  DSL_CHECK(d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_gcls % 4 == 0 && d->ld_gcls >= d->ld_cls,
            "dsl_fovea_loss: fcos.ld_cls / ld_gcls must be multiples of 4 that hold C columns");
  DSL_CHECK(d->ld_rc >= 4 && d->ld_rc % 4 == 0 && ((uintptr_t)d->regctr & 15) == 0 && ((uintptr_t)d->bbox_targets & 15) == 0,
            "dsl_fovea_loss: fcos.ld_rc must be a multiple of 4, regctr and bbox_targets 16-byte aligned");
  DSL_CHECK(d->ld_grc >= 8 && d->ld_grc % 8 == 0 && ((uintptr_t)d->g_rc & 15) == 0,
            "dsl_fovea_loss: fcos.ld_grc must be a multiple of 8, g_rc 16-byte aligned");
  DSL_CHECK(d->focal_gamma >= 0.f && d->focal_gamma < 1e30f && d->focal_alpha >= 0.f && d->focal_alpha <= 1.f,
            "dsl_fovea_loss: fcos.focal_gamma must be >= 0 and focal_alpha in [0, 1]");
  DSL_CHECK(d->w_cls >= 0.f && d->w_cls < 1e30f && d->w_bbox >= 0.f && d->w_bbox < 1e30f,
            "dsl_fovea_loss: fcos.w_cls / w_bbox must be finite and >= 0");
  k.gamma = d->focal_gamma; k.alpha = d->focal_alpha; k.w_cls = d->w_cls; k.w_bbox = d->w_bbox;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = head_loss_blocks(k);
  hipLaunchKernelGGL(d->num_classes % 4 != 0 ? fovea_loss_kernel<true> : fovea_loss_kernel<false>, dim3(blocks), dim3(256), 0, st, k);
  hipLaunchKernelGGL(fovea_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k, blocks);
  DSL_LAUNCH_CHECK("fovea_loss_kernel");
  return 0;
}
