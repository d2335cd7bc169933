// FCOS per-location target assignment and the fused focal + GIoU + centerness (+ DSL scale-invariant
// soft) loss, forward and backward in one pass, fp32.
//
// Restates mmdet/models/dense_heads/fcos_head.py:170-338 (loss), :550-560 (points), :562-705
// (targets), :707-726 (centerness target); mmdet/models/losses/focal_loss.py:11-56;
// mmdet/models/losses/iou_loss.py:85-102,329-366 with core/bbox/iou_calculators/iou2d_calculator.py:212-260;
// mmdet/models/losses/cross_entropy_loss.py:73-112 of the reference.
//
// Head options (dsl_fcos_desc.head_flags, uniform per launch; 0 = the fcos_semi "tricks" head): inside-box assignment
// (center_sampling=False, fcos_head.py:676-678), unnormalised targets and exp decode (norm_on_bbox=False, :162-167, :618),
// the IoU log loss (losses/iou_loss.py:14-36), and the centerness logit / gradient at a caller-given address
// (centerness_on_reg=False, :155-158: it belongs to the classification tower's predictor then).
//
// Loss family (DSL_HEAD_LOSS_EXT, uniform per launch; the loss_kernel<., true> instantiation - the default head's instruction stream
// is the kExt = false one, unchanged): loss_bbox of kind DSL_BOX_* - the linear IoU loss 1 - clamp(iou, eps) (losses/iou_loss.py:14-36),
// DIoU (:105-157) and CIoU (:160-219) beside GIoU and the IoU log loss; the focal loss with gamma >= 0 and 0 <= alpha <= 1
// (focal_loss.py:11-56); loss_weight of loss_cls / loss_bbox / loss_centerness (focal_loss.py:174, iou_loss.py:398,438,
// cross_entropy_loss.py:203) on the reported terms and on their gradients.  Two deliberate deviations from the reference's fp32
// arithmetic, both at their sites below: the CIoU aspect penalty v^2 / (1 - iou + v) and its gradient are 0 where v == 0 (the
// reference gives 0/0 = NaN when prediction and target coincide; 0 is the fp64 value), and the focal gradient is formed as
// -+alpha q^gamma (gamma p sp + q), which has no q^(gamma-1) and is finite where the reference's autograd returns NaN (gamma < 1 with
// a sigmoid saturated to exactly 0 or 1; the kernel returns the limit, 0).
//
// ATSS (DSL_HEAD_ATSS, uniform per launch): dsl_atss_assign restates mmdet/core/bbox/assigners/atss_assigner.py:66-178 over the
// anchors of core/anchor/anchor_generator.py:99-143,287-412 (one square anchor per location, valid flags with allowed_border = -1) and
// the target step of mmdet/models/dense_heads/atss_head.py:569-684; the loss_kernel<., true, true> instantiation restates
// atss_head.py:142-215,268-309 with delta2bbox of core/bbox/coder/delta_xywh_bbox_coder.py:144-266.  Tie rules and the two deliberate
// simplifications (the stored ground-truth box stands for decode(encode(gt))) are stated in include/dsl_hip.h and at their sites.
//
// The assignment must be BIT-identical to the reference's fp32 torch arithmetic, so this file is
// compiled with floating-point contraction off and the comparisons are written exactly as there.
#include "common.hpp"
#pragma clang fp contract(off)
#include "box_loss.hpp"      // (behind the pragma: its functions are compiled without contraction too)
#include "head_common.hpp"

namespace {

constexpr float kINF = 1e8f;   // fcos_head.py:11

struct FcK : HeadK {
  int n_labeled;
  float lo[DSL_MAX_SEG], hi[DSL_MAX_SEG];
  float radius, loss_weight, soft_weight;
  const float* gt_boxes; const long long* gt_labels; const int* gt_off;
  const float* ig_boxes; const int* ig_off;
  int* assign_idx; float* pos_weight;
  float* stats;
  int flags;              // DSL_HEAD_*
  const float* ctr; int ld_ctr;      // centerness logit of location m: ctr[m * ld_ctr]
  uint16_t* g_ctr; int ld_gctr;      // its gradient, when it does not live in column 4 of g_rc (else null)
  // loss family (loss_kernel<., true> only; box kind and eps, w_cls, w_bbox: HeadK): focal gamma / alpha, loss_centerness's weight
  float gamma, alpha, w_ctr;
  // ATSS (DSL_HEAD_ATSS: the atss_* kernels and loss_kernel<., true, true> only)
  float anchor_scale, stds[4];
  int topk;
  const int* pad_shapes;            // [n][2] (pad_h, pad_w)
  unsigned long long* akeys;        // [M] (IoU bits << 32 | ~gt index) of the winning box, 0 = none (workspace)
  int* npos;                        // [n] positives per image
  // PAA (DSL_HEAD_PAA: the paa_* kernels and loss_kernel<., true, true, true> only)
  float pos_iou_thr;
  float* pos_loss; float* iou_target;     // [M]
  int* cand_gt;                     // [M] the first assignment's box index within the image, -1 = none
  int* gmm_iters; int* gmm_flags;   // [max_gt]
  float* gtmax;                     // [max_gt] every box's maximum IoU over its image's valid anchors (workspace)
  int max_gt;
};

// one image, one location against a list of boxes: area-argmin with centre sampling + range test
// (fcos_head.py:632-700).  Returns min_area; idx = first argmin; ltrb of that box in t[4].
// in_box: the location only has to lie inside the box itself (center_sampling=False, fcos_head.py:676-678)
__device__ __forceinline__ float assign_one(float px, float py, float rs, float lo, float hi,
                                            const float* __restrict__ boxes, int g0, int g1, int& idx,
                                            float t[4], bool in_box) {
  float best = kINF;
  idx = 0;
  t[0] = t[1] = t[2] = t[3] = 0.f;
  for (int g = g0; g < g1; ++g) {
    const float x1 = boxes[4 * g], y1 = boxes[4 * g + 1], x2 = boxes[4 * g + 2], y2 = boxes[4 * g + 3];
    float area = (x2 - x1) * (y2 - y1);
    const float l = px - x1, tp = py - y1, r = x2 - px, b = y2 - py;
    const float cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
    const float xmin = cx - rs, ymin = cy - rs, xmax = cx + rs, ymax = cy + rs;
    const float c0 = xmin > x1 ? xmin : x1;
    const float c1 = ymin > y1 ? ymin : y1;
    const float c2 = xmax > x2 ? x2 : xmax;
    const float c3 = ymax > y2 ? y2 : ymax;
    const float cmin = in_box ? fminf(fminf(l, tp), fminf(r, b)) : fminf(fminf(px - c0, py - c1), fminf(c2 - px, c3 - py));
    const bool inside = cmin > 0.f;
    const float mx = fmaxf(fmaxf(l, tp), fmaxf(r, b));
    const bool in_range = (mx >= lo) && (mx <= hi);
    if (!inside || !in_range) area = kINF;
    if (g == g0 || area < best) {   // first index wins ties (torch.min over dim)
      best = area;
      idx = g - g0;
      t[0] = l; t[1] = tp; t[2] = r; t[3] = b;
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void assign_kernel(const FcK p) {
  __shared__ float sh[16];
  const int M = p.M;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float is_pos = 0.f, ctr = 0.f;
  if (m < M) {
    int lvl, img, y, x;
    head_loc(p, m, lvl, img, y, x);
    const int s = p.stride[lvl];
    const float px = (float)x * (float)s + (float)(s / 2);
    const float py = (float)y * (float)s + (float)(s / 2);
    const float rs = (float)s * p.radius;
    const bool in_box = (p.flags & DSL_HEAD_INSIDE_BOX) != 0;
    int idx;
    float t[4];
    const int g0 = p.gt_off[img], g1 = p.gt_off[img + 1];
    long long label = p.num_classes;
    int aidx = -1;
    if (g1 > g0) {
      const float best = assign_one(px, py, rs, p.lo[lvl], p.hi[lvl], p.gt_boxes, g0, g1, idx, t, in_box);
      if (best != kINF) {
        label = p.gt_labels[g0 + idx];
        aidx = idx;
      }
    } else {
      t[0] = t[1] = t[2] = t[3] = 0.f;
    }
    const float fs = (p.flags & DSL_HEAD_RAW_TARGETS) ? 1.f : (float)s;   // norm_on_bbox=False: targets stay in pixels (fcos_head.py:618)
    const float n0 = t[0] / fs, n1 = t[1] / fs, n2 = t[2] / fs, n3 = t[3] / fs;   // norm_on_bbox
    p.labels[m] = label;
    p.assign_idx[m] = aidx;
    *reinterpret_cast<f32x4*>(p.bbox_targets + 4ll * m) = f32x4{n0, n1, n2, n3};
    // ignore weight: 0 iff the location falls in an ignore box (same procedure) and is background
    float wgt = 1.f;
    if (p.ig_boxes && p.ig_off) {
      const int i0 = p.ig_off[img], i1 = p.ig_off[img + 1];
      if (i1 > i0) {
        int ii;
        float tt[4];
        const float bi = assign_one(px, py, rs, p.lo[lvl], p.hi[lvl], p.ig_boxes, i0, i1, ii, tt, in_box);
        if (bi != kINF && label == p.num_classes) wgt = 0.f;
      }
    }
    const float sw = (p.loss_weight != 1.0f && img >= p.n_labeled) ? p.loss_weight : 1.f;
    p.cls_weight[m] = wgt * sw;
    p.pos_weight[m] = sw;
    if (label < p.num_classes) {
      is_pos = 1.f;
      const float lr_min = fminf(n0, n2), lr_max = fmaxf(n0, n2);
      const float tb_min = fminf(n1, n3), tb_max = fmaxf(n1, n3);
      ctr = sqrtf((lr_min / lr_max) * (tb_min / tb_max));
    }
  }
  const float np = block_sum(is_pos, sh);
  const float cs = block_sum(ctr, sh);
  if (threadIdx.x == 0) {
    p.part[2 * blockIdx.x] = np;
    p.part[2 * blockIdx.x + 1] = cs;
  }
}

// ---- ATSS assignment (atss_assigner.py:66-178, atss_head.py:569-684; semantics and tie rules: include/dsl_hip.h) ---------------
constexpr int ATSS_T = 256;
constexpr int ATSS_MAXC = DSL_MAX_SEG * DSL_ATSS_MAX_TOPK;
constexpr float kMaxRatio = 4.135166556742356f;      // |log(16 / 1000)|, wh_ratio_clip of delta2bbox (delta_xywh_bbox_coder.py:227)

// the anchor of location (x, y): AnchorGenerator's base anchor [-0.5 ws, 0.5 ws] (center_offset 0) shifted by (x s, y s)
// (anchor_generator.py:99-143,287-352)
__device__ __forceinline__ void atss_anchor(const FcK& p, int lvl, int x, int y, float a[4]) {
  const float s = (float)p.stride[lvl];
  const float hw = 0.5f * (s * p.anchor_scale);
  const float sx = (float)x * s, sy = (float)y * s;
  a[0] = sx + (0.f - hw); a[1] = sy + (0.f - hw); a[2] = sx + hw; a[3] = sy + hw;
}

// valid extent of a level in image img: valid_flags with allowed_border = -1 (anchor_generator.py:354-412)
__device__ __forceinline__ void atss_valid(const FcK& p, int lvl, int img, int& vh, int& vw) {
  const int s = p.stride[lvl];
  const int ph = p.pad_shapes[2 * img], pw = p.pad_shapes[2 * img + 1];
  vh = min(max((ph + s - 1) / s, 0), p.h[lvl]);
  vw = min(max((pw + s - 1) / s, 0), p.w[lvl]);
}

// BboxOverlaps2D, mode 'iou' (iou2d_calculator.py:212-260)
__device__ __forceinline__ float atss_iou(const float a[4], float x1, float y1, float x2, float y2) {
  const float a1 = (a[2] - a[0]) * (a[3] - a[1]), a2 = (x2 - x1) * (y2 - y1);
  const float w = fmaxf(fminf(a[2], x2) - fmaxf(a[0], x1), 0.f), h = fmaxf(fminf(a[3], y2) - fmaxf(a[1], y1), 0.f);
  const float ov = w * h;
  return ov / fmaxf(a1 + a2 - ov, 1e-6f);
}

__global__ __launch_bounds__(ATSS_T) void atss_zero_kernel(const FcK p) {
  const int M = p.M;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) p.akeys[i] = 0ull;
  if (i < p.n) p.npos[i] = 0;
}

// One workgroup per ground-truth box: its candidates level by level (topk rounds of "the smallest (distance, index) above the last
// one" over every valid anchor of the level), the IoU threshold, and the positives' claims on their anchors.
__global__ __launch_bounds__(ATSS_T) void atss_cand_kernel(const FcK p) {
  __shared__ unsigned long long red[ATSS_T];
  __shared__ int c_idx[ATSS_MAXC], c_lvl[ATSS_MAXC];
  __shared__ float c_iou[ATSS_MAXC];
  __shared__ float s_thr;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= p.gt_off[p.n]) return;
  int img = 0;
  for (int i = 1; i < p.n; ++i)
    if (g >= p.gt_off[i]) img = i;
  const float x1 = p.gt_boxes[4 * g], y1 = p.gt_boxes[4 * g + 1], x2 = p.gt_boxes[4 * g + 2], y2 = p.gt_boxes[4 * g + 3];
  const float gcx = (x1 + x2) / 2.0f, gcy = (y1 + y2) / 2.0f;
  int ncand = 0;
  for (int lvl = 0; lvl < p.nlvl; ++lvl) {
    int vh, vw;
    atss_valid(p, lvl, img, vh, vw);
    const int nvalid = vh * vw, W = p.w[lvl];
    const int k = min(p.topk, nvalid);
    unsigned long long last = 0ull;
    for (int r = 0; r < k; ++r) {
      unsigned long long best = ~0ull;
      for (int i = tid; i < nvalid; i += ATSS_T) {
        const int y = i / vw, x = i - y * vw;
        float a[4];
        atss_anchor(p, lvl, x, y, a);
        const float dx = (a[0] + a[2]) / 2.0f - gcx, dy = (a[1] + a[3]) / 2.0f - gcy;
        const float d = sqrtf(dx * dx + dy * dy);
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(y * W + x);
        if ((r == 0 || key > last) && key < best) best = key;
      }
      red[tid] = best;
      __syncthreads();
      for (int o = ATSS_T / 2; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] < red[tid]) red[tid] = red[tid + o];
        __syncthreads();
      }
      last = red[0];
      __syncthreads();
      if (tid == 0) {
        c_idx[ncand + r] = (int)(unsigned)last;
        c_lvl[ncand + r] = lvl;
      }
    }
    ncand += k;
  }
  __syncthreads();
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int m = 0;
  if (tid < ncand) {
    const int lvl = c_lvl[tid], W = p.w[lvl];
    const int y = c_idx[tid] / W, x = c_idx[tid] - y * W;
    atss_anchor(p, lvl, x, y, a);
    m = p.mstart[lvl] + (img * p.h[lvl] + y) * W + x;
    c_iou[tid] = atss_iou(a, x1, y1, x2, y2);
  }
  __syncthreads();
  if (tid == 0) {      // mean + unbiased std, in (level, rank) order (atss_assigner.py:131-134)
    float sum = 0.f;
    for (int c = 0; c < ncand; ++c) sum += c_iou[c];
    const float mean = sum / (float)ncand;
    float ss = 0.f;
    for (int c = 0; c < ncand; ++c) ss += (c_iou[c] - mean) * (c_iou[c] - mean);
    s_thr = mean + sqrtf(ss / (float)(ncand - 1));      // one candidate: 0 / 0 = NaN, no positive (torch.std of one element)
  }
  __syncthreads();
  if (tid < ncand) {
    const float cx = (a[0] + a[2]) / 2.0f, cy = (a[1] + a[3]) / 2.0f;
    const float inside = fminf(fminf(cx - x1, cy - y1), fminf(x2 - cx, y2 - cy));
    const float iou = c_iou[tid];
    if (iou >= s_thr && inside > 0.01f)      // the highest IoU wins an anchor, equal IoUs the lower box (atss_assigner.py:156-166)
      atomicMax(p.akeys + m, ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)~(unsigned)(g - p.gt_off[img]));
  }
}

// one thread per anchor: the outputs of dsl_fcos_assign from the winning claim; block records [positives, centerness targets]
__global__ __launch_bounds__(ATSS_T) void atss_write_kernel(const FcK p) {
  __shared__ float sh[16];
  const int M = p.M;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float is_pos = 0.f, ctr = 0.f;
  if (m < M) {
    int lvl, img, y, x, vh, vw;
    head_loc(p, m, lvl, img, y, x);
    atss_valid(p, lvl, img, vh, vw);
    const bool valid = y < vh && x < vw;
    const unsigned long long key = p.akeys[m];
    long long label = p.num_classes;
    int aidx = -1;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (valid && key != 0ull) {
      aidx = (int)~(unsigned)key;
      const int g = p.gt_off[img] + aidx;
      label = p.gt_labels[g];
      t = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * g);
      float a[4];
      atss_anchor(p, lvl, x, y, a);
      // centerness target (atss_head.py:293-309) from the anchor centre and the ground-truth box itself; the reference uses
      // decode(encode(gt)), which differs from gt by rounding only
      const float cx = (a[2] + a[0]) / 2, cy = (a[3] + a[1]) / 2;
      const float l = cx - t[0], tp = cy - t[1], r = t[2] - cx, b = t[3] - cy;
      ctr = sqrtf((fminf(l, r) / fmaxf(l, r)) * (fminf(tp, b) / fmaxf(tp, b)));
      is_pos = 1.f;
      atomicAdd(p.npos + img, 1);
    }
    p.labels[m] = label;
    p.assign_idx[m] = aidx;
    *reinterpret_cast<f32x4*>(p.bbox_targets + 4ll * m) = t;
    p.cls_weight[m] = valid ? 1.f : 0.f;
    p.pos_weight[m] = 1.f;
  }
  const float np = block_sum(is_pos, sh);
  const float cs = block_sum(ctr, sh);
  if (threadIdx.x == 0) {
    p.part[2 * blockIdx.x] = np;
    p.part[2 * blockIdx.x + 1] = cs;
  }
}

// The assignment's block records [positives, centerness targets], added in block order -> stats[0] = num_pos, stats[1] = the sum of
// the centerness targets (this rank); stats[2..7] are reserved, kept zero.  kAtss: stats[0] = sum_i max(npos_i, 1) (atss_head.py:554)
template <bool kAtss>
__global__ __launch_bounds__(REC_T) void assign_finalize_kernel(const FcK p, int nblocks) {
  __shared__ float sh[REC_T];
  if constexpr (kAtss) {
    const float t = record_sum(p.part, nblocks, 2, 1, 1, sh);
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int i = 0; i < p.n; ++i) tot += max(p.npos[i], 1);
      p.stats[0] = (float)tot;
      p.stats[1] = t;
    }
  } else {
    const float t = record_sum(p.part, nblocks, 2, 0, 2, sh);
    if (threadIdx.x < 2) p.stats[threadIdx.x] = t;
  }
  if (threadIdx.x >= 2 && threadIdx.x < 8) p.stats[threadIdx.x] = 0.f;
}

// The loss records [cls, sisoft, bbox, centerness, g_scale x 5, pad], added in block order -> losses[4], g_scales[5] and logvec.
// kAtss: loss_bbox's normaliser is clamped at 1 (atss_head.py:286), not at 1e-6
// kHead: 0 FCOS, 1 ATSS, 2 PAA (loss_cls over max(num_pos, images), loss_bbox over the sum of the IoU targets: loss_kernel)
template <int kHead>
__global__ __launch_bounds__(REC_T) void fcos_finalize_kernel(const FcK p, int nblocks) {
  __shared__ float sh[REC_T];
  constexpr bool kAtss = kHead == 1, kPaa = kHead == 2;
  const float t = record_sum(p.part, nblocks, 16, 0, 16, sh);
  if (threadIdx.x < 16) {
    const float num_ctr = fmaxf(p.norm[0] * p.inv_world, 1.0f);
    const float num_pos = kPaa ? fmaxf(p.norm[0] * p.inv_world, (float)p.n) : num_ctr;
    const float denorm = kPaa ? (p.norm[1] * p.inv_world > 0.f ? p.norm[1] * p.inv_world : 1.0f)
                              : fmaxf(p.norm[1] * p.inv_world, kAtss ? 1.0f : 1e-6f);
    float fv = t;
    // (loss_weight * the mean, as the loss modules do; a weight of 1 leaves the bits as they are)
    if (threadIdx.x == 0) p.losses[0] = fv = t / num_pos * p.w_cls;
    else if (threadIdx.x == 1) p.losses[3] = fv = t * p.soft_weight;
    else if (threadIdx.x == 2) p.losses[1] = fv = t / denorm * p.w_bbox;
    else if (threadIdx.x == 3) p.losses[2] = fv = t / num_ctr * p.w_ctr;
    else if (threadIdx.x - 4 < DSL_MAX_SEG) p.g_scales[threadIdx.x - 4] = t;
    if (threadIdx.x < 4) sh[threadIdx.x] = fv;
  }
  if (p.logvec) {       // the log vector of _parse_losses (detectors/base.py:175-208): the loss terms and their sum
    __syncthreads();
    if (threadIdx.x == 0) {
      const float cls = sh[0], soft = sh[1], bbox = sh[2], ctr = sh[3];
      float tot = (cls + bbox) + ctr;
      int n = 3;
      p.logvec[0] = cls; p.logvec[1] = bbox; p.logvec[2] = ctr;
      if (p.soft_weight != 0.f) { p.logvec[n++] = soft; tot += soft; }
      p.logvec[n] = tot;
    }
  }
}

__global__ void points_kernel(const FcK p, float* __restrict__ pts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.M / p.n) return;
  int l = 0, q = i;
  while (q >= p.h[l] * p.w[l]) {
    q -= p.h[l] * p.w[l];
    ++l;
  }
  const int y = q / p.w[l], x = q - y * p.w[l], s = p.stride[l];
  pts[2 * i] = (float)x * (float)s + (float)(s / 2);
  pts[2 * i + 1] = (float)y * (float)s + (float)(s / 2);
}

// ---- focal helpers: loss and dloss/dx for target 0/1 (alpha .25, gamma 2) ----------------------
__device__ __forceinline__ void focal_fb(float x, bool t, float& loss, float& grad) {
  const float alpha = 0.25f;
  const float e = __expf(-fabsf(x));
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float pp = x >= 0.f ? inv : e * inv;   // sigmoid(x)
  const float q = 1.f - pp;
  if (t) {
    const float sp = fmaxf(-x, 0.f) + l1p;      // -log p
    loss = alpha * q * q * sp;
    grad = -alpha * q * q * (2.f * pp * sp + q);
  } else {
    const float sp = fmaxf(x, 0.f) + l1p;       // -log(1-p)
    loss = (1.f - alpha) * pp * pp * sp;
    grad = (1.f - alpha) * pp * pp * (2.f * q * sp + pp);
  }
}

// ---- loss family (kExt) -------------------------------------------------------------------------------------------------------
// focal loss and dloss/dx with gamma >= 0, 0 <= alpha <= 1 (focal_loss.py:34-40).  gamma == 2 keeps focal_fb's q * q sequence
// (launch-uniform branch).  Otherwise q = 1 - p is formed as sigmoid(-x), without cancellation, and the gradient as
// -+alpha q^gamma (gamma p sp + q): no q^(gamma-1), so it is finite for gamma < 1 at a saturated sigmoid, where the reference's autograd
// (pow's backward, 0 * inf) returns NaN - the value here is the limit, 0.  powf(0, 0) is 1, as torch's pow.
__device__ __forceinline__ void focal_fb_ext(float x, bool t, float gamma, float alpha, bool gamma2, float& loss, float& grad) {
  const float e = __expf(-fabsf(x));
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float pp = x >= 0.f ? inv : e * inv;   // sigmoid(x)
  if (gamma2) {
    const float q = 1.f - pp;
    if (t) {
      const float sp = fmaxf(-x, 0.f) + l1p;      // -log p
      loss = alpha * q * q * sp;
      grad = -alpha * q * q * (2.f * pp * sp + q);
    } else {
      const float sp = fmaxf(x, 0.f) + l1p;       // -log(1-p)
      loss = (1.f - alpha) * pp * pp * sp;
      grad = (1.f - alpha) * pp * pp * (2.f * q * sp + pp);
    }
    return;
  }
  const float q = x >= 0.f ? e * inv : inv;     // sigmoid(-x)
  if (t) {
    const float sp = fmaxf(-x, 0.f) + l1p;
    const float mod = powf(q, gamma);
    loss = alpha * mod * sp;
    grad = -alpha * mod * (gamma * pp * sp + q);
  } else {
    const float sp = fmaxf(x, 0.f) + l1p;
    const float mod = powf(pp, gamma);
    loss = (1.f - alpha) * mod * sp;
    grad = (1.f - alpha) * mod * (gamma * q * sp + pp);
  }
}

// kTail: C % 4 != 0, the last group of 4 classes of a location is partial.  Its lanes c + e >= C add no loss and no
// sisoft term and write 0 into g_cls; for C % 4 == 0 the kTail = false instantiation is the only one launched.
// kExt: the loss family (box kind, focal gamma / alpha, loss weights); kExt = false is the default head's kernel, which reads none
// of those fields.
// kAtss (with kExt): DSL_HEAD_ATSS - delta2bbox decode against the location's anchor, the stored ground-truth box as target, the
// normaliser of loss_bbox clamped at 1 (atss_head.py:142-215,268-287); the kAtss = false instantiations are the FCOS kernels, unchanged.
// kPaa (with kAtss): DSL_HEAD_PAA - loss_cls over max(num_pos, images), the IoU branch's BCE against iou_target over num_pos, loss_bbox
// weighted by max(iou_target, 1e-12) over the sum of the IoU targets (paa_head.py:169-199); kPaa = false leaves the other
// instantiations as they were.
template <bool kTail, bool kExt, bool kAtss = false, bool kPaa = false>
__global__ __launch_bounds__(256) void loss_kernel(const FcK p) {
  __shared__ float sh[16];
  const int M = p.M;
  const int C = p.num_classes;
  const int c4 = kTail ? (C + 3) / 4 : C / 4;
  const float num_pos = fmaxf(p.norm[0] * p.inv_world, kPaa ? (float)p.n : 1.0f);
  const float num_iou = fmaxf(p.norm[0] * p.inv_world, 1.0f);      // kPaa: avg_factor of loss_iou (no positive: nothing is divided)
  // kPaa: the sum of the IoU targets.  The reference divides by it as it is (0 / 0 when every positive's IoU is 0); here a sum that
  // is not positive counts as 1
  const float denorm = kPaa ? (p.norm[1] * p.inv_world > 0.f ? p.norm[1] * p.inv_world : 1.0f)
                            : fmaxf(p.norm[1] * p.inv_world, kAtss ? 1.0f : 1e-6f);
  const bool sisoft = (p.soft_weight != 0.f) && (p.n % 2 != 0) && p.n >= 3;

  // ---------------- classification: one thread per 4 consecutive classes of one location ----------
  float lsum = 0.f, ssum = 0.f;
  const long long total = (long long)M * c4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / c4);
    const int c = (int)(i - (long long)m * c4) * 4;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(p.cls_logits + (long long)m * p.ld_cls + c);
    const int label = (int)p.labels[m];
    const float wgt = p.cls_weight[m];
    const float gs = kExt ? wgt / num_pos * p.grad_scale * p.w_cls : wgt / num_pos * p.grad_scale;
    float g[4];
    bool live[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) live[e] = !kTail || c + e < C;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float l, d;
      if constexpr (kExt) focal_fb_ext(xv[e], label == c + e, p.gamma, p.alpha, p.gamma == 2.f, l, d);
      else focal_fb(xv[e], label == c + e, l, d);
      if (kTail && !live[e]) l = d = 0.f;
      lsum += l * wgt;
      g[e] = d * gs;
    }
    if (sisoft) {
      int lvl, img, y, x;
      head_loc(p, m, lvl, img, y, x);
      if (img == p.n - 2 && lvl >= 1) {
        // this is cls_scores[lvl][B-2]; partner cls_scores[lvl-1][B-1][:, :h, :w]  (fcos_head.py:315-319)
        const int pl = lvl - 1;
        const int m2 = p.mstart[pl] + ((p.n - 1) * p.h[pl] + y) * p.w[pl] + x;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.cls_logits + (long long)m2 * p.ld_cls + c);
        const float inv_cnt = 1.f / ((float)C * (float)p.h[lvl] * (float)p.w[lvl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = (kTail && !live[e]) ? 0.f : xv[e] - bv[e];
          ssum += d * d * inv_cnt;
          g[e] += 2.f * d * inv_cnt * p.soft_weight * p.grad_scale;
        }
      }
      if (img == p.n - 1 && lvl + 1 < p.nlvl && y < p.h[lvl + 1] && x < p.w[lvl + 1]) {
        const int nl = lvl + 1;
        const int m2 = p.mstart[nl] + ((p.n - 2) * p.h[nl] + y) * p.w[nl] + x;
        const f32x4 av = *reinterpret_cast<const f32x4*>(p.cls_logits + (long long)m2 * p.ld_cls + c);
        const float inv_cnt = 1.f / ((float)C * (float)p.h[nl] * (float)p.w[nl]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (!kTail || live[e]) g[e] -= 2.f * (av[e] - xv[e]) * inv_cnt * p.soft_weight * p.grad_scale;
      }
    }
    u32x2 o = {pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
    *reinterpret_cast<u32x2*>(p.g_cls + (long long)m * p.ld_gcls + c) = o;
  }
  lsum = block_sum(lsum, sh);
  ssum = block_sum(ssum, sh);
  float* rec = p.part + 16ll * blockIdx.x;          // [cls, sisoft, bbox, centerness, g_scale x 5, pad]
  if (threadIdx.x == 0) {
    rec[0] = lsum;
    rec[1] = ssum;
  }

  // ---------------- boxes + centerness: one thread per location ---------------------------------
  float bsum = 0.f, csum = 0.f;
  float gsc[DSL_MAX_SEG] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const bool exp_dec = (p.flags & DSL_HEAD_EXP_DECODE) != 0, iou_loss = (p.flags & DSL_HEAD_IOU_LOSS) != 0;
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
    float gr[4] = {0.f, 0.f, 0.f, 0.f}, gc = 0.f;
    const int label = (int)p.labels[m];
    if (label < C) {
      int lvl, img, y, x;
      head_loc(p, m, lvl, img, y, x);
      const int s = p.stride[lvl];
      const float px = (float)x * (float)s + (float)(s / 2), py = (float)y * (float)s + (float)(s / 2);
      const float sc = p.scales[lvl];
      const float* rc = p.regctr + (long long)m * p.ld_rc;
      float raw[4], d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        raw[k] = rc[k];
        const float z = raw[k] * sc;
        if constexpr (kAtss) d[k] = z * p.stds[k];      // denorm_deltas = deltas * stds + means, means 0 (delta_xywh_bbox_coder.py:209)
        else d[k] = exp_dec ? expf(z) : fmaxf(z, 0.f);      // fcos_head.py:162-167
      }
      const f32x4 t = *reinterpret_cast<const f32x4*>(p.bbox_targets + 4ll * m);
      const float pw = p.pos_weight[m];
      float ct, x1, y1, x2, y2, X1, Y1, X2, Y2;
      float aw = 0.f, gw = 0.f, gh = 0.f;      // kAtss: anchor side, decoded width / height
      if constexpr (kAtss) {
        // the anchor's centre (x s, y s) and side a = anchor_scale * s; delta2bbox (delta_xywh_bbox_coder.py:209-246), no clip in training
        const float acx = (float)x * (float)s, acy = (float)y * (float)s;
        aw = p.anchor_scale * (float)s;
        gw = aw * expf(fminf(fmaxf(d[2], -kMaxRatio), kMaxRatio));
        gh = aw * expf(fminf(fmaxf(d[3], -kMaxRatio), kMaxRatio));
        const float gx = acx + aw * d[0], gy = acy + aw * d[1];
        x1 = gx - gw * 0.5f; y1 = gy - gh * 0.5f; x2 = gx + gw * 0.5f; y2 = gy + gh * 0.5f;
        // target: the stored ground-truth box.  The reference decodes encode(gt) (atss_head.py:194-195), which differs from gt by
        // rounding only; the centerness target (:293-309) likewise, from the anchor centre
        X1 = t[0]; Y1 = t[1]; X2 = t[2]; Y2 = t[3];
        const float l = acx - X1, tp = acy - Y1, r = X2 - acx, b = Y2 - acy;
        ct = sqrtf((fminf(l, r) / fmaxf(l, r)) * (fminf(tp, b) / fmaxf(tp, b)));
      } else {
        ct = sqrtf((fminf(t[0], t[2]) / fmaxf(t[0], t[2])) * (fminf(t[1], t[3]) / fmaxf(t[1], t[3])));
        // decode (distance2bbox, core/bbox/transforms.py:119-162; no clip in training)
        x1 = px - d[0]; y1 = py - d[1]; x2 = px + d[2]; y2 = py + d[3];
        X1 = px - t[0]; Y1 = py - t[1]; X2 = px + t[2]; Y2 = py + t[3];
      }
      if constexpr (kPaa) ct = p.iou_target[m];      // the target of the IoU branch, a constant for the gradient (paa_head.py:183-184)
      const float wb = (kPaa ? fmaxf(ct, 1e-12f) : ct) * pw;
      float dbox[4];
      if (kExt && p.box_kind >= DSL_BOX_IOU_LINEAR) {
        float dl[4];
        bsum += wb * box_loss_ext(p.box_kind, p.box_eps, x1, y1, x2, y2, X1, Y1, X2, Y2, dl);
        const float coef = wb / denorm * p.grad_scale * p.w_bbox;   // dL/dloss; 0: no positive weight or loss_weight 0 - exactly-zero gradients
#pragma unroll
        for (int k = 0; k < 4; ++k) dbox[k] = coef != 0.f ? coef * dl[k] : 0.f;
      } else {
        // (kept inline, not box_loss_giou: that forms the IoU log loss's gradient as c * (dg / iouc), this block as (c / iouc) * dg -
        // other bits in the plain FCOS head's gradients)
        const float eps = 1e-6f;
        const float a1 = (x2 - x1) * (y2 - y1), a2 = (X2 - X1) * (Y2 - Y1);
        const float ltx = fmaxf(x1, X1), lty = fmaxf(y1, Y1), rbx = fminf(x2, X2), rby = fminf(y2, Y2);
        const float w0 = rbx - ltx, h0 = rby - lty;
        const float iw = fmaxf(w0, 0.f), ih = fmaxf(h0, 0.f);
        const float ov = iw * ih;
        const float u0 = a1 + a2 - ov;
        const float U = fmaxf(u0, eps);
        const float ex1 = fminf(x1, X1), ey1 = fminf(y1, Y1), ex2 = fmaxf(x2, X2), ey2 = fmaxf(y2, Y2);
        const float ew0 = ex2 - ex1, eh0 = ey2 - ey1;
        const float ew = fmaxf(ew0, 0.f), eh = fmaxf(eh0, 0.f);
        const float e0 = ew * eh;
        const float E = fmaxf(e0, eps);
        // IoULoss (iou_loss.py:14-36): -log(clamp(iou, eps)); clamp passes the gradient where iou >= eps
        const float iou = ov / U;
        float coef_iou = 0.f;                             // dL/diou of the log loss (set below, IoU mode only)
        if (iou_loss) {
          const float iouc = fmaxf(iou, eps);
          bsum += wb * (-logf(iouc));
          coef_iou = (-wb / denorm * p.grad_scale) / iouc;
        } else {
          const float giou = iou - (E - U) / E;
          bsum += wb * (1.f - giou);
        }
        // ---- backward of (1 - giou) w.r.t. (x1, y1, x2, y2) ----
        const float cw = w0 >= 0.f ? 1.f : 0.f, chh = h0 >= 0.f ? 1.f : 0.f;   // clamp(min=0) passes grad at 0
        const float dw_x1 = -dmax_a(x1, X1) * cw, dw_x2 = dmin_a(x2, X2) * cw;
        const float dh_y1 = -dmax_a(y1, Y1) * chh, dh_y2 = dmin_a(y2, Y2) * chh;
        const float dov[4] = {ih * dw_x1, iw * dh_y1, ih * dw_x2, iw * dh_y2};
        const float da1[4] = {-(y2 - y1), -(x2 - x1), (y2 - y1), (x2 - x1)};
        const float ug = u0 > eps ? 1.f : (u0 == eps ? 0.5f : 0.f);
        const float cew = ew0 >= 0.f ? 1.f : 0.f, ceh = eh0 >= 0.f ? 1.f : 0.f;
        const float dew_x1 = -dmin_a(x1, X1) * cew, dew_x2 = dmax_a(x2, X2) * cew;
        const float deh_y1 = -dmin_a(y1, Y1) * ceh, deh_y2 = dmax_a(y2, Y2) * ceh;
        const float eg = e0 > eps ? 1.f : (e0 == eps ? 0.5f : 0.f);
        const float de[4] = {eh * dew_x1 * eg, ew * deh_y1 * eg, eh * dew_x2 * eg, ew * deh_y2 * eg};
        const float coef = -wb / denorm * p.grad_scale;   // dL/dgiou
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float dU = (da1[k] - dov[k]) * ug;
          if (iou_loss) {
            const float dg = dov[k] / U - ov * dU / (U * U);
            dbox[k] = iou >= eps ? coef_iou * dg : 0.f;
          } else {
            const float dg = dov[k] / U - ov * dU / (U * U) + dU / E - U * de[k] / (E * E);
            dbox[k] = coef * dg;
          }
        }
        if constexpr (kExt) {
#pragma unroll
          for (int k = 0; k < 4; ++k) dbox[k] *= p.w_bbox;
        }
      }
      if constexpr (kAtss) {
        // x1 = gx - gw / 2, x2 = gx + gw / 2 with gx = acx + a d0, gw = a exp(clamp(d2)): no gradient through an active clamp
        // (torch.clamp passes it on the closed interval), then d[k] = scale * raw[k] * stds[k]
        const float dz[4] = {(dbox[0] + dbox[2]) * aw, (dbox[1] + dbox[3]) * aw,
                             (d[2] >= -kMaxRatio && d[2] <= kMaxRatio) ? 0.5f * (dbox[2] - dbox[0]) * gw : 0.f,
                             (d[3] >= -kMaxRatio && d[3] <= kMaxRatio) ? 0.5f * (dbox[3] - dbox[1]) * gh : 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          gr[k] = dz[k] * p.stds[k] * sc;
          gsc[lvl] += dz[k] * p.stds[k] * raw[k];
        }
      } else {
        const float dd[4] = {-dbox[0], -dbox[1], dbox[2], dbox[3]};   // x1 = px - d0, ... x2 = px + d2
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float on = exp_dec ? d[k] : ((raw[k] * sc > 0.f) ? 1.f : 0.f);     // d exp(z) / dz = exp(z); relu's gate
          gr[k] = dd[k] * on * sc;
          gsc[lvl] += dd[k] * on * raw[k];
        }
      }
      // centerness BCE-with-logits (cross_entropy_loss.py:73-112)
      const float cl = p.ctr[(long long)m * p.ld_ctr];
      const float e = __expf(-fabsf(cl));
      const float sig = cl >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      csum += (fmaxf(cl, 0.f) - cl * ct + log1pf(e)) * pw;
      gc = (sig - ct) * pw / (kPaa ? num_iou : num_pos) * p.grad_scale;
      if constexpr (kExt) gc *= p.w_ctr;
    }
    if (p.g_ctr) {      // the centerness gradient belongs to the classification predictor's columns
      u32x4 o = {pack2bf(gr[0], gr[1]), pack2bf(gr[2], gr[3]), 0u, 0u};
      *reinterpret_cast<u32x4*>(p.g_rc + (long long)m * p.ld_grc) = o;
      p.g_ctr[(long long)m * p.ld_gctr] = f2bf(gc);
    } else {
      u32x4 o = {pack2bf(gr[0], gr[1]), pack2bf(gr[2], gr[3]), pack2bf(gc, 0.f), 0u};
      *reinterpret_cast<u32x4*>(p.g_rc + (long long)m * p.ld_grc) = o;
    }
  }
  bsum = block_sum(bsum, sh);
  csum = block_sum(csum, sh);
  if (threadIdx.x == 0) {
    rec[2] = bsum;
    rec[3] = csum;
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

// ---- PAA (paa_head.py:86-399, max_iou_assigner.py:127-212; semantics, tie rules and deviations: include/dsl_hip.h) ---------------
constexpr int PAA_MAXS = DSL_MAX_SEG * DSL_ATSS_MAX_TOPK;      // samples of one mixture fit

// gtmax[g] = the box's maximum IoU over the valid anchors of its image (gt_max_overlaps); -1 for an unused slot
__global__ __launch_bounds__(ATSS_T) void paa_gtmax_kernel(const FcK p) {
  __shared__ float red[ATSS_T];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= p.gt_off[p.n]) {
    if (tid == 0) p.gtmax[g] = -1.f;
    return;
  }
  int img = 0;
  for (int i = 1; i < p.n; ++i)
    if (g >= p.gt_off[i]) img = i;
  const float x1 = p.gt_boxes[4 * g], y1 = p.gt_boxes[4 * g + 1], x2 = p.gt_boxes[4 * g + 2], y2 = p.gt_boxes[4 * g + 3];
  float best = -1.f;
  for (int lvl = 0; lvl < p.nlvl; ++lvl) {
    int vh, vw;
    atss_valid(p, lvl, img, vh, vw);
    const int nvalid = vh * vw;
    for (int i = tid; i < nvalid; i += ATSS_T) {
      const int y = i / vw, x = i - y * vw;
      float a[4];
      atss_anchor(p, lvl, x, y, a);
      best = fmaxf(best, atss_iou(a, x1, y1, x2, y2));
    }
  }
  red[tid] = best;
  __syncthreads();
  for (int o = ATSS_T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (tid == 0) p.gtmax[g] = red[0];
}

// one thread per anchor: assign_wrt_overlaps.  The argmax box if its IoU >= pos_iou_thr (equal maxima: the lower box), then the
// low-quality pass in box order - the LAST box whose maximum over anchors this anchor's IoU equals takes it (the same atss_iou bits
// on both sides of the comparison)
__global__ __launch_bounds__(ATSS_T) void paa_write_kernel(const FcK p) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m == 0) {
    for (int i = 0; i < 8; ++i) p.stats[i] = 0.f;
    for (int i = 0; i < p.n; ++i) p.npos[i] = 0;
  }
  if (m >= p.M) return;
  int lvl, img, y, x, vh, vw;
  head_loc(p, m, lvl, img, y, x);
  atss_valid(p, lvl, img, vh, vw);
  const bool valid = y < vh && x < vw;
  const int g0 = p.gt_off[img], g1 = p.gt_off[img + 1];
  int cand = -1;
  if (valid && g1 > g0) {
    float a[4];
    atss_anchor(p, lvl, x, y, a);
    float best = -1.f;
    int arg = 0, low = -1;
    for (int g = g0; g < g1; ++g) {
      const float iou = atss_iou(a, p.gt_boxes[4 * g], p.gt_boxes[4 * g + 1], p.gt_boxes[4 * g + 2], p.gt_boxes[4 * g + 3]);
      if (iou > best) { best = iou; arg = g - g0; }
      if (iou == p.gtmax[g]) low = g - g0;
    }
    cand = low >= 0 ? low : (best >= p.pos_iou_thr ? arg : -1);
  }
  long long label = p.num_classes;
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
  if (cand >= 0) {
    label = p.gt_labels[g0 + cand];
    t = *reinterpret_cast<const f32x4*>(p.gt_boxes + 4ll * (g0 + cand));
  }
  p.cand_gt[m] = cand;
  p.assign_idx[m] = cand;
  p.labels[m] = label;
  *reinterpret_cast<f32x4*>(p.bbox_targets + 4ll * m) = t;
  p.cls_weight[m] = valid ? 1.f : 0.f;
  p.pos_weight[m] = 1.f;
}

// one thread per anchor: a candidate's loss w_cls * sum_c focal + w_bbox * box_loss(decode, target), reduction 'none'
// (paa_head.py:201-255), and the aligned IoU of the same two boxes, which dsl_paa_reassign keeps as iou_target for the positives
__global__ __launch_bounds__(256) void paa_pos_loss_kernel(const FcK p) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= p.M) return;
  float pl = 0.f, it = 0.f;
  if (p.cand_gt[m] >= 0) {
    const int C = p.num_classes, label = (int)p.labels[m];
    const float* row = p.cls_logits + (long long)m * p.ld_cls;
    const bool gamma2 = p.gamma == 2.f;
    float acc = 0.f;
    for (int c = 0; c < C; c += 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e < C) {
          float l, d;
          focal_fb_ext(xv[e], label == c + e, p.gamma, p.alpha, gamma2, l, d);
          acc += l;
        }
      }
    }
    int lvl, img, y, x;
    head_loc(p, m, lvl, img, y, x);
    const float s = (float)p.stride[lvl], sc = p.scales[lvl];
    const float* rc = p.regctr + (long long)m * p.ld_rc;
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = rc[k] * sc * p.stds[k];
    // delta2bbox against the anchor (centre (x s, y s), side anchor_scale * s): loss_kernel<., true, true>'s lines
    const float acx = (float)x * s, acy = (float)y * s, aw = p.anchor_scale * s;
    const float gw = aw * expf(fminf(fmaxf(d[2], -kMaxRatio), kMaxRatio)), gh = aw * expf(fminf(fmaxf(d[3], -kMaxRatio), kMaxRatio));
    const float gx = acx + aw * d[0], gy = acy + aw * d[1];
    const float x1 = gx - gw * 0.5f, y1 = gy - gh * 0.5f, x2 = gx + gw * 0.5f, y2 = gy + gh * 0.5f;
    const f32x4 t = *reinterpret_cast<const f32x4*>(p.bbox_targets + 4ll * m);
    float dl[4];
    const float bl = p.box_kind >= DSL_BOX_IOU_LINEAR ? box_loss_ext(p.box_kind, p.box_eps, x1, y1, x2, y2, t[0], t[1], t[2], t[3], dl)
                                                      : box_loss_giou(p.box_kind == DSL_BOX_IOU_LOG, x1, y1, x2, y2, t[0], t[1], t[2], t[3], dl);
    pl = p.w_cls * acc + p.w_bbox * bl;
    const float a1 = (x2 - x1) * (y2 - y1), a2 = (t[2] - t[0]) * (t[3] - t[1]);
    const float iw = fmaxf(fminf(x2, t[2]) - fmaxf(x1, t[0]), 0.f), ih = fmaxf(fminf(y2, t[3]) - fmaxf(y1, t[1]), 0.f);
    const float ov = iw * ih;
    it = ov / fmaxf(a1 + a2 - ov, 1e-6f);      // bbox_overlaps, is_aligned (paa_head.py:183-184)
  }
  p.pos_loss[m] = pl;
  p.iou_target[m] = it;
}

// fixed-order butterfly sum over the wavefront: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  return m + log(exp(a - m) + exp(b - m));
}

// weighted log probabilities of a lane's two samples under both components, as sklearn's _estimate_log_gaussian_prob ('diag') +
// log(weights) forms them: -0.5 (log(2 pi) + mu^2 P - 2 x (mu P) + x^2 P) + log(prec_chol) + log(w), log(2 pi) rounded to float32
__device__ __forceinline__ void paa_wlp(const double mu[2], const double mu2[2], const double pc[2], const double lw[2], double x0, double xx0,
                                        double x1, double xx1, double& a00, double& a01, double& a10, double& a11) {
  const double c2pi = (double)1.8378770664093453f;      // np.log(2 * np.pi).astype(float32)
  double b[2][2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double prec = pc[k] * pc[k], mp = mu[k] * prec, ld = log(pc[k]);
    const double l0 = mu2[k] * prec - 2.0 * (x0 * mp) + xx0 * prec, l1 = mu2[k] * prec - 2.0 * (x1 * mp) + xx1 * prec;
    b[0][k] = -0.5 * (c2pi + l0) + ld + lw[k];
    b[1][k] = -0.5 * (c2pi + l1) + ld + lw[k];
  }
  a00 = b[0][0]; a01 = b[0][1]; a10 = b[1][0]; a11 = b[1][1];
}

// One workgroup per ground-truth box: its candidates' per-level top-k by loss, the sorted sample list, the mixture fit by the first
// wavefront (two samples per lane, float64 on the float32 losses, sklearn's GaussianMixture(2, 'diag') as paa_head.py:326-345 sets
// it up), the separation scheme (:392-399) and the demotion of every candidate that is not kept.  Block record [positives, sum of
// their IoU targets].  iou_target is paa_pos_loss_kernel's: kept where an anchor stays positive, cleared where not - the two launches
// are an ordered pair (include/dsl_hip.h).
__global__ __launch_bounds__(ATSS_T) void paa_reassign_kernel(const FcK p) {
  __shared__ unsigned long long red[ATSS_T];
  __shared__ unsigned long long c_key[PAA_MAXS], s_key[PAA_MAXS];      // (loss bits << 32 | location): a loss is >= 0, so the bits order it
  __shared__ int s_keep[PAA_MAXS];
  __shared__ int s_iters, s_flag;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= p.gt_off[p.n]) {
    if (tid == 0) {
      p.part[2 * g] = 0.f; p.part[2 * g + 1] = 0.f;
      p.gmm_iters[g] = 0; p.gmm_flags[g] = 0;
    }
    return;
  }
  int img = 0;
  for (int i = 1; i < p.n; ++i)
    if (g >= p.gt_off[i]) img = i;
  const int gl = g - p.gt_off[img];
  int ncand = 0;
  for (int lvl = 0; lvl < p.nlvl; ++lvl) {      // TIE RULE: equal losses go to the lower location index
    const int hw = p.h[lvl] * p.w[lvl], base = p.mstart[lvl] + img * hw;
    unsigned long long last = 0ull;
    int found = 0;
    for (int r = 0; r < p.topk; ++r) {
      unsigned long long best = ~0ull;
      for (int i = tid; i < hw; i += ATSS_T) {
        const int m = base + i;
        if (p.cand_gt[m] != gl) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(p.pos_loss[m]) << 32) | (unsigned)m;
        if ((r == 0 || key > last) && key < best) best = key;
      }
      red[tid] = best;
      __syncthreads();
      for (int o = ATSS_T / 2; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] < red[tid]) red[tid] = red[tid + o];
        __syncthreads();
      }
      last = red[0];
      __syncthreads();
      if (last == ~0ull) break;      // (uniform: fewer than topk candidates on this level)
      if (tid == 0) c_key[ncand + found] = last;
      ++found;
    }
    ncand += found;
  }
  __syncthreads();
  if (tid < ncand) {      // rank sort: the keys are distinct (the location is part of them)
    const unsigned long long key = c_key[tid];
    int rank = 0;
    for (int j = 0; j < ncand; ++j) rank += c_key[j] < key ? 1 : 0;
    s_key[rank] = key;
    s_keep[tid] = 0;
  }
  if (tid == 0) { s_iters = 0; s_flag = ncand < 2 ? 1 : 0; }      // fewer than two samples: the box keeps none (paa_head.py:320-321)
  __syncthreads();
  if (tid < 64 && ncand >= 2) {
    const int n = ncand, i0 = tid, i1 = tid + 64;
    const bool v0 = i0 < n, v1 = i1 < n;
    const float f0 = v0 ? __uint_as_float((unsigned)(s_key[i0] >> 32)) : 0.f, f1 = v1 ? __uint_as_float((unsigned)(s_key[i1] >> 32)) : 0.f;
    // sklearn keeps float32 samples: X * X, X**2 and the initial means**2 are float32 products, widened afterwards
    const double x0 = f0, x1 = f1, xx0 = (double)(f0 * f0), xx1 = (double)(f1 * f1);
    const float fmin_ = __uint_as_float((unsigned)(s_key[0] >> 32)), fmax_ = __uint_as_float((unsigned)(s_key[n - 1] >> 32));
    double mu[2] = {(double)fmin_, (double)fmax_}, mu2[2] = {(double)(fmin_ * fmin_), (double)(fmax_ * fmax_)};
    double pc[2] = {1.0, 1.0}, lw[2] = {log(0.5), log(0.5)};
    double lower = -INFINITY;
    int it = 0, flag = 0;
    double a00 = 0, a01 = 0, a10 = 0, a11 = 0;
    for (it = 1; it <= 100; ++it) {
      const double prev = lower;
      paa_wlp(mu, mu2, pc, lw, x0, xx0, x1, xx1, a00, a01, a10, a11);
      const double n0 = lse2(a00, a01), n1 = lse2(a10, a11);
      const double r00 = v0 ? exp(a00 - n0) : 0.0, r01 = v0 ? exp(a01 - n0) : 0.0;
      const double r10 = v1 ? exp(a10 - n1) : 0.0, r11 = v1 ? exp(a11 - n1) : 0.0;
      const double nk0 = wave_sum_f64(r00 + r10) + 10.0 * 2.220446049250313e-16, nk1 = wave_sum_f64(r01 + r11) + 10.0 * 2.220446049250313e-16;
      const double sx0 = wave_sum_f64(r00 * x0 + r10 * x1), sx1 = wave_sum_f64(r01 * x0 + r11 * x1);
      const double sq0 = wave_sum_f64(r00 * xx0 + r10 * xx1), sq1 = wave_sum_f64(r01 * xx0 + r11 * xx1);
      const double sn = wave_sum_f64((v0 ? n0 : 0.0) + (v1 ? n1 : 0.0));
      mu[0] = sx0 / nk0; mu[1] = sx1 / nk1;
      mu2[0] = mu[0] * mu[0]; mu2[1] = mu[1] * mu[1];
      const double var0 = sq0 / nk0 - mu2[0] + 1e-6, var1 = sq1 / nk1 - mu2[1] + 1e-6;
      const double wsum = nk0 + nk1;
      lw[0] = log(nk0 / wsum); lw[1] = log(nk1 / wsum);
      if (!(var0 > 0.0) || !(var1 > 0.0)) {      // sklearn raises here ("ill-defined empirical covariance"): the box keeps no positive
        flag = 2;
        break;
      }
      pc[0] = 1.0 / sqrt(var0); pc[1] = 1.0 / sqrt(var1);
      lower = sn / (double)n;
      if (fabs(lower - prev) < 1e-3) break;
    }
    if (it > 100) it = 100;
    if (flag == 0) {
      paa_wlp(mu, mu2, pc, lw, x0, xx0, x1, xx1, a00, a01, a10, a11);      // predict / score_samples with the parameters of the last M-step
      const bool fg0 = v0 && !(a01 > a00), fg1 = v1 && !(a11 > a10);      // argmax: ties go to component 0
      const double sc0 = lse2(a00, a01), sc1 = lse2(a10, a11);
      // the foreground sample with the highest score (equal scores: the first in sorted order)
      double bs = fg0 ? sc0 : -INFINITY;
      int bi = fg0 ? i0 : 0x7fffffff;
      if (fg1 && (sc1 > bs || bi == 0x7fffffff)) { bs = sc1; bi = i1; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
      }
      if (fg0 && i0 <= bi) s_keep[i0] = 1;      // the first j + 1 foreground samples (paa_head.py:396-397)
      if (fg1 && i1 <= bi) s_keep[i1] = 1;
    }
    if (tid == 0) { s_iters = it; s_flag = flag; }
  }
  __syncthreads();
  // every candidate of the box that is not kept: background, no box weight (cls_weight stays 1: nothing is ignored)
  for (int lvl = 0; lvl < p.nlvl; ++lvl) {
    const int hw = p.h[lvl] * p.w[lvl], base = p.mstart[lvl] + img * hw;
    for (int i = tid; i < hw; i += ATSS_T) {
      const int m = base + i;
      if (p.cand_gt[m] != gl) continue;
      bool keep = false;
      for (int j = 0; j < ncand; ++j) keep = keep || ((int)(unsigned)s_key[j] == m && s_keep[j]);
      if (!keep) {
        p.labels[m] = p.num_classes;
        p.assign_idx[m] = -1;
        p.pos_weight[m] = 0.f;
        p.iou_target[m] = 0.f;
      }
    }
  }
  if (tid == 0) {
    int np = 0;
    float isum = 0.f;
    for (int j = 0; j < ncand; ++j)      // in sorted order
      if (s_keep[j]) { ++np; isum += p.iou_target[(int)(unsigned)s_key[j]]; }
    p.part[2 * g] = (float)np; p.part[2 * g + 1] = isum;
    p.gmm_iters[g] = s_iters; p.gmm_flags[g] = s_flag;
  }
}

// npos per image, stats[0] = their sum (not clamped per image), stats[1] = the sum of the IoU targets: the boxes' records in box order
__global__ __launch_bounds__(REC_T) void paa_finalize_kernel(const FcK p, int nrec) {
  __shared__ float sh[REC_T];
  const float t = record_sum(p.part, nrec, 2, 0, 2, sh);
  if (threadIdx.x < 2) p.stats[threadIdx.x] = t;
  if (threadIdx.x >= 2 && threadIdx.x < 8) p.stats[threadIdx.x] = 0.f;
  for (int i = threadIdx.x; i < p.n; i += REC_T) {
    int c = 0;
    for (int g = p.gt_off[i]; g < p.gt_off[i + 1]; ++g) c += (int)p.part[2 * g];
    p.npos[i] = c;
  }
}

int fill(const dsl_fcos_desc* d, FcK& k) {
  k = FcK{};
  if (head_fill(d, k, "fcos")) return -1;
  k.n_labeled = d->n / 2;      // fcos_head.py:225-231: first floor(B/2) images are the labeled stream
  for (int l = 0; l < d->nlvl; ++l) {
    k.lo[l] = d->range_lo[l]; k.hi[l] = d->range_hi[l];
  }
  k.radius = d->radius; k.loss_weight = d->loss_weight; k.soft_weight = d->soft_weight;
  k.gt_boxes = d->gt_boxes; k.gt_labels = (const long long*)d->gt_labels; k.gt_off = d->gt_off;
  k.ig_boxes = d->ig_boxes; k.ig_off = d->ig_off;
  k.assign_idx = d->assign_idx; k.pos_weight = d->pos_weight; k.stats = d->stats;
  k.flags = d->head_flags;
  // centerness_on_reg=False: the logit and its gradient live with the classification predictor (caller-given addresses)
  k.ctr = d->ctr ? d->ctr : (d->regctr ? d->regctr + 4 : nullptr);
  k.ld_ctr = d->ctr ? d->ld_ctr : d->ld_rc;
  k.g_ctr = (uint16_t*)d->g_ctr; k.ld_gctr = d->ld_gctr;
  // loss family: the fields behind ld_gctr count only with DSL_HEAD_LOSS_EXT; without it they are not read (zero-filled descriptors)
  k.box_kind = (k.flags & DSL_HEAD_IOU_LOSS) ? DSL_BOX_IOU_LOG : DSL_BOX_GIOU;
  k.box_eps = 1e-6f; k.gamma = 2.f; k.alpha = 0.25f; k.w_cls = k.w_bbox = k.w_ctr = 1.f;
  if (k.flags & DSL_HEAD_LOSS_EXT) {
    if (head_loss_settings(d, d->w_ctr, k, "fcos")) return -1;
    DSL_CHECK(d->focal_gamma >= 0.f && d->focal_gamma < 1e30f && d->focal_alpha >= 0.f && d->focal_alpha <= 1.f,
              "fcos: focal gamma must be >= 0 and alpha in [0, 1]");
    k.gamma = d->focal_gamma; k.alpha = d->focal_alpha; k.w_ctr = d->w_ctr;
    k.flags = (k.flags & ~DSL_HEAD_IOU_LOSS) | (k.box_kind == DSL_BOX_IOU_LOG ? DSL_HEAD_IOU_LOSS : 0);
  }
  if (k.flags & DSL_HEAD_ATSS) {
    const dsl_atss_desc* a = d->atss;
    DSL_CHECK(a, "fcos: DSL_HEAD_ATSS needs dsl_fcos_desc.atss");
    DSL_CHECK(a->anchor_scale > 0.f && a->anchor_scale < 1e30f, "atss: anchor_scale must be finite and > 0");
    for (int e = 0; e < 4; ++e) {
      DSL_CHECK(a->delta_stds[e] > 0.f && a->delta_stds[e] < 1e30f, "atss: delta_stds must be finite and > 0");
      k.stds[e] = a->delta_stds[e];
    }
    DSL_CHECK((k.flags & (DSL_HEAD_INSIDE_BOX | DSL_HEAD_RAW_TARGETS | DSL_HEAD_EXP_DECODE)) == 0 && !d->ctr,
              "atss: DSL_HEAD_ATSS goes with no other assignment / decode flag and centerness on the regression tower");
    DSL_CHECK(d->loss_weight == 1.0f && d->soft_weight == 0.f, "atss: no DSL stream weight / sisoft term");
    k.anchor_scale = a->anchor_scale;
  }
  return 0;
}

// ATSS workspace: the block records of atss_write_kernel, then one 64-bit claim per anchor
size_t atss_assign_bytes(long long M) { return ((size_t)((M + ATSS_T - 1) / ATSS_T) * 2 * sizeof(float) + 15) / 16 * 16 + (size_t)M * 8; }

// the default head's loss terms (GIoU or the IoU log loss, gamma 2, alpha 0.25, weights 1): the kExt = false kernel computes them
bool loss_is_default(const FcK& k) {
  return k.box_kind <= DSL_BOX_IOU_LOG && k.gamma == 2.f && k.alpha == 0.25f && k.w_cls == 1.f && k.w_bbox == 1.f && k.w_ctr == 1.f;
}

// loss_kernel's instantiations, [C % 4 != 0][0 the default head, 1 the loss family, 2 ATSS (always the loss family's kernel: with
// the default settings it computes the default terms)]
void (*const kLossKernel[2][4])(const FcK) = {
    {loss_kernel<false, false>, loss_kernel<false, true>, loss_kernel<false, true, true>, loss_kernel<false, true, true, true>},
    {loss_kernel<true, false>, loss_kernel<true, true>, loss_kernel<true, true, true>, loss_kernel<true, true, true, true>}};

// PAA workspace: the boxes' records [positives, IoU sum] of paa_reassign_kernel, then gtmax
size_t paa_bytes(int max_gt) { return (size_t)max_gt * 3 * sizeof(float); }

// a dsl_paa_desc the kernels build, or -1 with dsl_last_error naming the field
int paa_fill(const dsl_paa_desc* q, FcK& k, const char* who) {
  DSL_CHECK(q, "%s: null descriptor", who);
  const dsl_fcos_desc* d = &q->fcos;
  const int want = DSL_HEAD_ATSS | DSL_HEAD_PAA | DSL_HEAD_LOSS_EXT;
  DSL_CHECK((d->head_flags & want) == want && !(d->head_flags & (DSL_HEAD_GFL | DSL_HEAD_LD)),
            "%s: head_flags must be DSL_HEAD_ATSS | DSL_HEAD_PAA | DSL_HEAD_LOSS_EXT", who);
  if (fill(d, k)) return -1;
  const dsl_atss_desc* a = d->atss;
  DSL_CHECK(a->topk >= 1 && a->topk <= DSL_ATSS_MAX_TOPK, "%s: atss.topk must be in 1..16", who);
  DSL_CHECK(a->max_gt >= 1 && a->max_gt <= 65535, "%s: atss.max_gt must be in 1..65535", who);
  DSL_CHECK(a->pad_shapes, "%s: atss.pad_shapes is null", who);
  DSL_CHECK(a->npos, "%s: atss.npos is null", who);
  DSL_CHECK(q->pos_iou_thr > 0.f && q->pos_iou_thr < 1.f, "%s: pos_iou_thr must be in (0, 1)", who);
  DSL_CHECK(q->pos_loss, "%s: pos_loss is null", who);
  DSL_CHECK(q->iou_target, "%s: iou_target is null", who);
  DSL_CHECK(q->cand_gt, "%s: cand_gt is null", who);
  DSL_CHECK(q->gmm_iters, "%s: gmm_iters is null", who);
  DSL_CHECK(q->gmm_flags, "%s: gmm_flags is null", who);
  DSL_CHECK(d->gt_boxes && d->gt_labels && d->gt_off && d->labels && d->bbox_targets && d->assign_idx && d->cls_weight && d->pos_weight &&
                d->stats, "%s: null pointer in fcos (ground truth, targets or stats)", who);
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d) && ((uintptr_t)d->workspace & 15) == 0,
            "%s: fcos.workspace too small or not 16-byte aligned", who);
  k.topk = a->topk; k.pad_shapes = a->pad_shapes; k.npos = a->npos; k.max_gt = a->max_gt;
  k.pos_iou_thr = q->pos_iou_thr; k.pos_loss = q->pos_loss; k.iou_target = q->iou_target; k.cand_gt = q->cand_gt;
  k.gmm_iters = q->gmm_iters; k.gmm_flags = q->gmm_flags;
  k.gtmax = (float*)d->workspace + 2 * (size_t)a->max_gt;
  return 0;
}

int paa_head_outputs(const dsl_fcos_desc* d, const char* who) {
  DSL_CHECK(d->cls_logits && d->regctr && d->scales, "%s: null head output (fcos.cls_logits, regctr, scales)", who);
  DSL_CHECK(d->num_classes >= 1 && d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_rc >= 5,
            "%s: unsupported fcos.ld_cls / ld_rc / num_classes", who);
  return 0;
}

}  // namespace

extern "C" size_t dsl_fcos_workspace_bytes(const dsl_fcos_desc* d) {
  HeadGeom g;
  if (head_geom(d, g, "dsl_fcos_workspace_bytes")) return 0;
  // (DSL_HEAD_FOVEA: one count per assignment workgroup and the loss records - within `need`)
  const size_t assign_rec = (size_t)((g.M + 255) / 256) * 2, loss_rec = 2048 * 16;
  const size_t need = (assign_rec > loss_rec ? assign_rec : loss_rec) * sizeof(float);
  if (d->head_flags & DSL_HEAD_AUTOASSIGN) return need + dsl_aa_workspace_extra(d);      // the boxes' and the images' records (max_gt, n)
  if (d->head_flags & DSL_HEAD_PAA) {      // the boxes' records and maxima (d->atss->max_gt of them)
    const size_t paa = d->atss ? paa_bytes(d->atss->max_gt > 0 ? d->atss->max_gt : 0) : 0;
    return need > paa ? need : paa;
  }
  if (d->head_flags & DSL_HEAD_ATSS) return need > atss_assign_bytes(g.M) ? need : atss_assign_bytes(g.M);
  return need;
}

extern "C" int dsl_fcos_points(const dsl_fcos_desc* d, float* points, void* stream) {
  FcK k;
  if (fill(d, k)) return -1;
  DSL_CHECK(points, "dsl_fcos_points: null output");
  hipLaunchKernelGGL(points_kernel, dim3((k.M / k.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, k, points);
  DSL_LAUNCH_CHECK("points_kernel");
  return 0;
}

extern "C" int dsl_fcos_assign(const dsl_fcos_desc* d, void* stream) {
  FcK k;
  if (fill(d, k)) return -1;
  DSL_CHECK(d->gt_boxes && d->gt_labels && d->gt_off && d->labels && d->bbox_targets && d->assign_idx &&
                d->cls_weight && d->pos_weight && d->stats,
            "dsl_fcos_assign: null pointer");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_ATSS), "dsl_fcos_assign: a DSL_HEAD_ATSS descriptor is assigned by dsl_atss_assign");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_FOVEA), "dsl_fcos_assign: a DSL_HEAD_FOVEA descriptor is assigned by dsl_fovea_assign");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_AUTOASSIGN), "dsl_fcos_assign: a DSL_HEAD_AUTOASSIGN descriptor is assigned by dsl_aa_assign");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (k.M + 255) / 256;
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d), "dsl_fcos_assign: workspace too small");
  hipLaunchKernelGGL(assign_kernel, dim3(nb), dim3(256), 0, st, k);
  hipLaunchKernelGGL(assign_finalize_kernel<false>, dim3(1), dim3(REC_T), 0, st, k, nb);
  DSL_LAUNCH_CHECK("assign_kernel");
  return 0;
}

extern "C" int dsl_atss_assign(const dsl_fcos_desc* d, const dsl_atss_desc* a, void* stream) {
  FcK k;
  DSL_CHECK(d && a && d->atss == a && (d->head_flags & DSL_HEAD_ATSS), "dsl_atss_assign: DSL_HEAD_ATSS and d->atss == a are required");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_PAA), "dsl_atss_assign: a DSL_HEAD_PAA descriptor is assigned by dsl_paa_assign");
  if (fill(d, k)) return -1;
  DSL_CHECK(d->gt_boxes && d->gt_labels && d->gt_off && d->labels && d->bbox_targets && d->assign_idx && d->cls_weight &&
                d->pos_weight && d->stats && a->pad_shapes && a->npos,
            "dsl_atss_assign: null pointer");
  DSL_CHECK(a->topk >= 1 && a->topk <= DSL_ATSS_MAX_TOPK, "dsl_atss_assign: topk must be in 1..16");
  DSL_CHECK(a->max_gt >= 1 && a->max_gt <= 65535, "dsl_atss_assign: max_gt must be in 1..65535");
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d) && ((uintptr_t)d->workspace & 15) == 0,
            "dsl_atss_assign: workspace too small or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int M = k.M;
  const int nb = (M + ATSS_T - 1) / ATSS_T;
  k.topk = a->topk; k.pad_shapes = a->pad_shapes; k.npos = a->npos;
  k.akeys = (unsigned long long*)((char*)d->workspace + (atss_assign_bytes(M) - (size_t)M * 8));
  const int nz = (M > d->n ? M : d->n);
  hipLaunchKernelGGL(atss_zero_kernel, dim3((nz + ATSS_T - 1) / ATSS_T), dim3(ATSS_T), 0, st, k);
  hipLaunchKernelGGL(atss_cand_kernel, dim3(a->max_gt), dim3(ATSS_T), 0, st, k);
  hipLaunchKernelGGL(atss_write_kernel, dim3(nb), dim3(ATSS_T), 0, st, k);
  hipLaunchKernelGGL(assign_finalize_kernel<true>, dim3(1), dim3(REC_T), 0, st, k, nb);
  DSL_LAUNCH_CHECK("atss_assign");
  return 0;
}

extern "C" int dsl_fcos_loss(const dsl_fcos_desc* d, void* stream) {
  FcK k;
  if (fill(d, k)) return -1;
  DSL_CHECK(!(d->head_flags & DSL_HEAD_GFL), "dsl_fcos_loss: a DSL_HEAD_GFL descriptor's loss is dsl_gfl_loss");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_PAA), "dsl_fcos_loss: a DSL_HEAD_PAA descriptor's loss is dsl_paa_loss");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_FOVEA), "dsl_fcos_loss: a DSL_HEAD_FOVEA descriptor's loss is dsl_fovea_loss");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_AUTOASSIGN), "dsl_fcos_loss: a DSL_HEAD_AUTOASSIGN descriptor's loss is dsl_aa_loss");
  if (head_loss_ptrs(d, "dsl_fcos_loss")) return -1;
  DSL_CHECK(d->pos_weight, "dsl_fcos_loss: null pointer");
  DSL_CHECK(d->num_classes >= 1 && d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_gcls % 4 == 0 &&
                d->ld_gcls >= d->ld_cls && d->ld_grc % 8 == 0 && d->ld_rc >= (d->ctr ? 4 : 5),
            "dsl_fcos_loss: unsupported strides / class count");
  DSL_CHECK((d->ctr != nullptr) == (d->g_ctr != nullptr), "dsl_fcos_loss: ctr and g_ctr go together");
  hipStream_t st = (hipStream_t)stream;
  DSL_CHECK(d->workspace && d->workspace_bytes >= dsl_fcos_workspace_bytes(d), "dsl_fcos_loss: workspace too small");
  const bool atss = (k.flags & DSL_HEAD_ATSS) != 0;
  const int blocks = head_loss_blocks(k);
  hipLaunchKernelGGL(kLossKernel[d->num_classes % 4 != 0][atss ? 2 : !loss_is_default(k)], dim3(blocks), dim3(256), 0, st, k);
  hipLaunchKernelGGL(atss ? fcos_finalize_kernel<1> : fcos_finalize_kernel<0>, dim3(1), dim3(REC_T), 0, st, k, blocks);
  DSL_LAUNCH_CHECK("loss_kernel");
  return 0;
}

extern "C" int dsl_paa_assign(const dsl_paa_desc* q, void* stream) {
  FcK k;
  if (paa_fill(q, k, "dsl_paa_assign")) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(paa_gtmax_kernel, dim3(k.max_gt), dim3(ATSS_T), 0, st, k);
  hipLaunchKernelGGL(paa_write_kernel, dim3((k.M + ATSS_T - 1) / ATSS_T), dim3(ATSS_T), 0, st, k);
  DSL_LAUNCH_CHECK("paa_assign");
  return 0;
}

extern "C" int dsl_paa_pos_loss(const dsl_paa_desc* q, void* stream) {
  FcK k;
  if (paa_fill(q, k, "dsl_paa_pos_loss") || paa_head_outputs(&q->fcos, "dsl_paa_pos_loss")) return -1;
  hipLaunchKernelGGL(paa_pos_loss_kernel, dim3((k.M + 255) / 256), dim3(256), 0, (hipStream_t)stream, k);
  DSL_LAUNCH_CHECK("paa_pos_loss");
  return 0;
}

extern "C" int dsl_paa_reassign(const dsl_paa_desc* q, void* stream) {
  FcK k;
  if (paa_fill(q, k, "dsl_paa_reassign")) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(paa_reassign_kernel, dim3(k.max_gt), dim3(ATSS_T), 0, st, k);
  hipLaunchKernelGGL(paa_finalize_kernel, dim3(1), dim3(REC_T), 0, st, k, k.max_gt);
  DSL_LAUNCH_CHECK("paa_reassign");
  return 0;
}

extern "C" int dsl_paa_loss(const dsl_paa_desc* q, void* stream) {
  FcK k;
  if (paa_fill(q, k, "dsl_paa_loss") || paa_head_outputs(&q->fcos, "dsl_paa_loss")) return -1;
  const dsl_fcos_desc* d = &q->fcos;
  if (head_loss_ptrs(d, "dsl_paa_loss")) return -1;
  DSL_CHECK(d->ld_gcls % 4 == 0 && d->ld_gcls >= d->ld_cls && d->ld_grc % 8 == 0, "dsl_paa_loss: unsupported fcos.ld_gcls / ld_grc");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = head_loss_blocks(k);
  hipLaunchKernelGGL(kLossKernel[d->num_classes % 4 != 0][3], dim3(blocks), dim3(256), 0, st, k);
  hipLaunchKernelGGL(fcos_finalize_kernel<2>, dim3(1), dim3(REC_T), 0, st, k, blocks);
  DSL_LAUNCH_CHECK("paa_loss");
  return 0;
}

/* one dispatch for every head: the entry point a descriptor's head_flags name (include/dsl_hip.h) */
extern "C" int dsl_head_assign(const dsl_fcos_desc* d, void* stream) {
  DSL_CHECK(d, "dsl_head_assign: null descriptor");
  if (d->head_flags & DSL_HEAD_AUTOASSIGN) return dsl_aa_assign((const dsl_aa_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_FOVEA) return dsl_fovea_assign((const dsl_fovea_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_PAA) return dsl_paa_assign((const dsl_paa_desc*)d, stream);
  return (d->head_flags & DSL_HEAD_ATSS) ? dsl_atss_assign(d, d->atss, stream) : dsl_fcos_assign(d, stream);
}

extern "C" int dsl_head_loss(const dsl_fcos_desc* d, void* stream) {
  DSL_CHECK(d, "dsl_head_loss: null descriptor");
  if (d->head_flags & DSL_HEAD_AUTOASSIGN) return dsl_aa_loss((const dsl_aa_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_FOVEA) return dsl_fovea_loss((const dsl_fovea_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_PAA) return dsl_paa_loss((const dsl_paa_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_LD) return dsl_ld_loss((const dsl_ld_desc*)d, stream);
  if (d->head_flags & DSL_HEAD_GFL) return dsl_gfl_loss((const dsl_gfl_desc*)d, stream);
  return dsl_fcos_loss(d, stream);
}
