// Teacher-sweep post-processing on the GPU: per-level top-k by max_c(score*centerness), box decode +
// clip + rescale, score threshold, class-aware greedy NMS, top max_per_img.
//
// Restates FCOSHead._get_bboxes (mmdet/models/dense_heads/fcos_head.py:406-548), multiclass_nms
// (mmdet/core/post_processing/bbox_nms.py:7-94) and mmcv.ops.batched_nms / nms (mmcv-full 1.3.10,
// un-vendored: class-offset trick boxes + label*(max+1), suppress IoU > thr, offset 0, scores sorted
// descending) of the reference, replacing the GPU->CPU numpy->JSON round trip of
// mmdet/runner/hooks/unlabel_pred_hook.py:194-293.
//
// Test-time augmentation (BBoxTestMixin.aug_test_bboxes / merge_aug_bboxes, dense_heads/dense_test_mixins.py:38-108, 173-200;
// bbox_mapping_back / bbox_flip, core/bbox/transforms.py:5-55) splits the same work where the reference's with_nms=False
// returns: dsl_fcos_detect_collect does a view's top-k, decode, clip and map-back into a pool of candidate rows,
// dsl_fcos_detect_finish the threshold, compaction, sort, NMS and cut over the pool of all views.
//
// Soft-NMS (dsl_det_desc.nms_method != 0; mmcv's batched_nms with type='soft_nms', stated by the reference's
// mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127) replaces the suppression stage of all three entry points: det_soft_kernel runs the
// pick / decay loop per (image, class), det_soft_final_kernel pools the picks and keeps the best max_per_img.
//
// ATSSHead (DSL_HEAD_ATSS in head_flags, the descriptor then being a dsl_det_atss_desc; ATSSHead._get_bboxes,
// mmdet/models/dense_heads/atss_head.py:420-495): det_decode decodes anchor deltas (delta2bbox,
// core/bbox/coder/delta_xywh_bbox_coder.py:144-269, clipped to img_shape) instead of distances; every stage behind it is shared.
//
// GFLHead (DSL_HEAD_GFL, the descriptor then being a dsl_det_gfl_desc; GFLHead._get_bboxes, mmdet/models/dense_heads/gfl_head.py:
// 372-443): det_decode takes the distances as Integral(scale x) * stride (gfl_head.py:15-48) from the anchor centre.  There is no
// centerness factor: the kernels' centerness logit is then one constant whose sigmoid is exactly 1 (kNoCtr, row stride 0), so
// key, pair score and pool rows are the class sigmoid alone and no kernel in front of or behind the decode branches on the head.
//
// PAAHead (DSL_HEAD_PAA beside DSL_HEAD_ATSS, the descriptor then being a dsl_det_paa_desc; PAAHead._get_bboxes and score_voting,
// mmdet/models/dense_heads/paa_head.py:519-673): ATSS's decode; the key and the pair score are sqrt(sigmoid(cls) * sigmoid(iou)),
// which score_thr tests and which is the final score (no centerness factor); with score_voting det_vote_kernel runs behind the NMS.
//
// FoveaHead (DSL_HEAD_FOVEA, the descriptor then being a dsl_det_fovea_desc; FoveaHead._get_bboxes, mmdet/models/dense_heads/
// fovea_head.py:298-348): det_decode takes the distances as base_len * exp(x) from the point s (x + 0.5) and clamps to img_shape - 1;
// no Scale and no centerness factor (GFL's unit logit kNoCtr).  dsl_fcos_detect_collect refuses the flag.
//
// AutoAssignHead (DSL_HEAD_AUTOASSIGN on a plain dsl_det_desc; autoassign_head.py:173-187,204-212 with FCOSHead.get_bboxes): FCOS's
// decode relu(scale x) s and score sigmoid(cls) * sigmoid(objectness) from the point (x s, y s) - no half-stride offset - in the
// single-view path and in a view's collect alike (both decode through det_decode).
#include "common.hpp"
#pragma clang fp contract(off)

namespace {

constexpr int CAND_CAP = 16384;
constexpr int NMS_THREADS = 1024;

struct DetK {
  int nlvl, n, num_classes, nms_pre, max_per_img;
  int h[DSL_MAX_SEG], w[DSL_MAX_SEG], stride[DSL_MAX_SEG];
  int mstart[DSL_MAX_SEG + 1];
  float score_thr, iou_thr;
  const float* cls; int ld_cls;
  const float* rc; int ld_rc;
  const float* ctr; int ld_ctr;      // centerness logit of location m: ctr[m * ld_ctr] (column 4 of rc, or the classification predictor's)
  int exp_decode;                    // norm_on_bbox=False: exp(scale x), no stride multiply (fcos_head.py:162-167)
  int atss;                          // DSL_HEAD_ATSS: delta2bbox against the location's anchor (atss_head.py:420-495)
  float anchor_scale, stds[4];
  int gfl_R;                         // DSL_HEAD_GFL: reg_max + 1 bins per side (0 = not a GFL head)
  int paa;                           // DSL_HEAD_PAA: the pair score is sqrt(sigmoid(cls) * sigmoid(iou)), threshold and final score alike
  int point_origin;                  // DSL_HEAD_AUTOASSIGN: the point is (x s, y s), FCOS's decode otherwise
  int fovea;                         // DSL_HEAD_FOVEA: base_len * exp(x) from the point s (x + 0.5), clamp to img_shape - 1; no Scale
  float base_len[DSL_MAX_SEG];
  const float* scales; const float* img_shapes; const float* scale_factors;
  float* dets; long long* det_labels; int* det_count;
  // workspace
  float* keys; int* sel; int* selcnt; float* cbox; float* cscore; int* clabel; int* ccount; float* pairscore;
  // merged views (dsl_fcos_detect_finish): candidate rows [box 4, centerness, num_classes scores] of pool_ld floats, row =
  // pair index / num_classes; `nlvl` then counts (view, level) groups and the per-level arrays above are not read
  const float* pool; int pool_ld;
  // Soft-NMS: DSL_NMS_* of the descriptor, and the current score per candidate slot (workspace): >= 0 while the candidate is in
  // the running and once it is emitted, -1 when it is out
  int nms_method; float soft_sigma, soft_min_score; float* sscore;
};

// what dsl_fcos_detect_collect adds to a view's DetK
constexpr int AUG_MAGIC = 0x41554731;
struct AugK {
  int view, flip;              // DSL_FLIP_*
  float* rows; int ld;         // the pool's rows; this view's start at (view * nlvl) * nms_pre
  int* rec;                    // the pool's record per view [view][4]: AUG_MAGIC, nlvl, nms_pre, num_classes of its collect
  int* selcnt;                 // the pool's valid rows per (view, level)
  float* sf;                   // the pool's copy of every view's scale factor [view][4]
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// the "centerness logit" of a head without centerness (DSL_HEAD_GFL, DSL_HEAD_FOVEA): expf(-100) is 0, sigmoidf_ gives exactly 1
__device__ __attribute__((used)) float kNoCtr = 100.f;      // (never written)

// key[m] = max_c sigmoid(cls) * sigmoid(ctr)     (fcos_head.py:472-473).  Full groups of 4 classes, then the partial
// last group (C % 4 != 0) with its lanes c >= C left out: the row's padding columns hold whatever the buffer held.
__global__ void det_key_kernel(const DetK p) {
  const int M = p.mstart[p.nlvl];
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float* c = p.cls + (long long)m * p.ld_cls;
  const float ctr = sigmoidf_(p.ctr[(long long)m * p.ld_ctr]);
  float best = -1.f;
  const int full = p.num_classes & ~3;
  for (int k = 0; k < full; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(c + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) best = fmaxf(best, p.paa ? sqrtf(sigmoidf_(v[e]) * ctr) : sigmoidf_(v[e]) * ctr);
  }
  if (full < p.num_classes) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(c + full);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (full + e < p.num_classes) best = fmaxf(best, p.paa ? sqrtf(sigmoidf_(v[e]) * ctr) : sigmoidf_(v[e]) * ctr);
  }
  p.keys[m] = best;
}

// Block-wide radix select over non-negative floats (bit pattern is monotonic): returns the bit pattern
// of the k-th largest value and how many elements equal to it belong to the top k.  11 + 11 + 10 bits.
__device__ void radix_select_block(const float* keys, int P, int k, unsigned* hist /*2048 + 1024, blockDim 1024*/, unsigned* s_tmp /*2*/,
                                   unsigned& prefix_out, unsigned& need_out) {
  unsigned prefix = 0, mask = 0, need = (unsigned)k;
  const int shifts[3] = {21, 10, 0};
  const int bits[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << bits[pass];
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      const float f = keys[i];
      const unsigned u = f > 0.f ? __float_as_uint(f) : 0u;
      // (non-positive keys all fall into bin 0 of the first pass: hundreds of thousands of atomics on one LDS word for the
      // dense pair scores, so they are left out of the histogram: with fewer positive keys than asked for the result is prefix 0
      // and need = k - their number, and the callers' tie predicate decides which zeros count - all of a level's keys, only the
      // valid pairs' zero scores)
      if (u != 0u && (u & mask) == prefix) atomicAdd(&hist[(u >> shifts[pass]) & (nb - 1)], 1u);
    }
    __syncthreads();
    // the bin that holds the need-th largest key: suffix sums over the bins, in parallel (a single thread walking 2 048 LDS
    // words took ~80 us per pass).  Thread t owns bins 2t, 2t+1; Hillis-Steele suffix scan over the 1 024 pair sums in place.
    {
      unsigned* pair = hist + 2048;                  // caller provides 2048 + 1024 words
      const int t = threadIdx.x;
      const unsigned h0 = hist[2 * t], h1 = hist[2 * t + 1];
      pair[t] = h0 + h1;
      __syncthreads();
      for (int d = 1; d < 1024; d <<= 1) {
        const unsigned add = t + d < 1024 ? pair[t + d] : 0u;
        __syncthreads();
        pair[t] += add;
        __syncthreads();
      }
      // pair[t] = number of keys in bins >= 2t; above bin 2t+1: pair[t] - h0 - h1
      const unsigned above1 = pair[t] - h0 - h1, above0 = above1 + h1;       // keys in bins > 2t+1, > 2t
      if (above1 < need && above1 + h1 >= need) { s_tmp[0] = prefix | ((unsigned)(2 * t + 1) << shifts[pass]); s_tmp[1] = need - above1; }
      if (above0 < need && above0 + h0 >= need) { s_tmp[0] = prefix | ((unsigned)(2 * t) << shifts[pass]); s_tmp[1] = need - above0; }
      if (t == 0 && pair[0] < need) { s_tmp[0] = prefix; s_tmp[1] = need - (pair[0] - h0); }     // fewer keys than asked for: bin 0 (as before)
    }
    __syncthreads();
    prefix = s_tmp[0];
    need = s_tmp[1];
    mask |= ((unsigned)(nb - 1)) << shifts[pass];
    __syncthreads();
  }
  prefix_out = prefix;
  need_out = need;
}

// Ordered stream compaction by one workgroup: element i of [0, P) is taken when take(i) says so, taken elements get
// consecutive output slots IN INDEX ORDER (no atomics: results do not depend on wave arrival order).  Among the
// elements for which tie(i) holds only the first `need` (lowest indices) are taken - the deterministic version of
// "any `need` of the equal keys", and the choice torch.topk makes on the CPU path of the reference.
// Two passes over wave-contiguous segments: count (ballot + popcount), workgroup scan of the 16 wave totals, write.
template <typename Take, typename Tie, typename Emit>
__device__ void ordered_compact(int P, unsigned need, unsigned* s_wave /* >= 2 * 16 + 2 */, Take take, Tie tie, Emit emit,
                                unsigned* total_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  constexpr int U = 4;                                           // 64-element groups per iteration: U predicate loads in flight
  const int seg = ((P + nw - 1) / nw + 64 * U - 1) / (64 * U) * (64 * U);      // elements per wave, multiple of 64 * U
  const int lo = wave * seg, hi = min(P, lo + seg);
  unsigned ntake = 0, ntie = 0;
  for (int i0 = lo; i0 < hi; i0 += 64 * U) {
    bool tk[U], ti[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 64 + lane;
      const bool in = i < hi;
      tk[u] = in && take(i);
      ti[u] = in && tie(i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ntake += __popcll(__ballot(tk[u]));
      ntie += __popcll(__ballot(ti[u]));
    }
  }
  if (lane == 0) {
    s_wave[wave] = ntake;
    s_wave[16 + wave] = ntie;
  }
  __syncthreads();
  // ties taken from the waves in front of this one, and the output slots they (and their sure takes) use
  unsigned tie_before = 0, out_before = 0;
  for (int w = 0; w < wave; ++w) {
    const unsigned t = s_wave[16 + w];
    const unsigned used = tie_before < need ? min(t, need - tie_before) : 0u;
    out_before += s_wave[w] + used;
    tie_before += t;
  }
  unsigned out = out_before, tr = tie_before;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int i0 = lo; i0 < hi; i0 += 64 * U) {
    bool tk[U], ti[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 64 + lane;
      const bool in = i < hi;
      tk[u] = in && take(i);
      ti[u] = in && tie(i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {                   // index order: group u before group u + 1
      const int i = i0 + u * 64 + lane;
      const unsigned long long bt = __ballot(ti[u]);
      const unsigned my_tr = tr + (unsigned)__popcll(bt & lt);
      const bool sel = tk[u] || (ti[u] && my_tr < need);
      const unsigned long long bs = __ballot(sel);
      if (sel) emit(i, out + (unsigned)__popcll(bs & lt));
      out += (unsigned)__popcll(bs);
      tr += (unsigned)__popcll(bt);
    }
  }
  if (total_out) {
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) *total_out = out;       // the last wave's running offset = the total
    __syncthreads();
  }
}

// one block per (image, level): indices of the top nms_pre keys (all of them when the level is smaller), in index order
__global__ __launch_bounds__(1024) void det_select_kernel(const DetK p) {
  __shared__ unsigned hist[2048 + 1024];
  __shared__ unsigned s_tmp[2], s_wave[34], s_total;
  const int lvl = blockIdx.x, img = blockIdx.y;
  const int P = p.h[lvl] * p.w[lvl];
  const int base = p.mstart[lvl] + img * P;
  int* sel = p.sel + ((long long)img * p.nlvl + lvl) * p.nms_pre;
  int* cnt = p.selcnt + img * p.nlvl + lvl;
  const int k = p.nms_pre;
  if (!(k > 0 && k < P)) {        // get_k_for_topk: take everything
    for (int i = threadIdx.x; i < P; i += blockDim.x) sel[i] = i;
    if (threadIdx.x == 0) *cnt = P;
    return;
  }
  unsigned prefix, need;
  radix_select_block(p.keys + base, P, k, hist, s_tmp, prefix, need);
  const float* keys = p.keys + base;
  auto bits = [&](int i) { const float f = keys[i]; return f > 0.f ? __float_as_uint(f) : 0u; };
  ordered_compact(
      P, need, s_wave, [&](int i) { return bits(i) > prefix; }, [&](int i) { return bits(i) == prefix; },
      [&](int i, unsigned slot) { sel[slot] = i; }, &s_total);
  if (threadIdx.x == 0) *cnt = (int)s_total;
}

// dense final scores of every (selected location, class) pair: score*centerness if score > score_thr
// (bbox_nms.py:54: validity is tested BEFORE the centerness factor), else -1.  A valid pair whose centerness sigmoid
// underflows has final score 0 and stays a candidate, as in the reference: every consumer tests det_valid (>= 0), never > 0.
__device__ __forceinline__ bool det_valid(float ps) { return ps >= 0.f; }
// the radix select's view of a final score: the bit pattern of a positive one, 0 for a zero (and for the -1 of an invalid pair,
// which det_valid keeps out first)
__device__ __forceinline__ unsigned det_bits(float ps) { return ps > 0.f ? __float_as_uint(ps) : 0u; }
__global__ void det_pairscore_kernel(const DetK p) {
  const int img = blockIdx.z, lvl = blockIdx.y;
  const int nsel = p.selcnt[img * p.nlvl + lvl];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nms_pre * p.num_classes) return;
  const int slot = t / p.num_classes, c = t - slot * p.num_classes;
  float out = -1.f;
  if (slot < nsel) {
    const int P = p.h[lvl] * p.w[lvl];
    const int loc = p.sel[((long long)img * p.nlvl + lvl) * p.nms_pre + slot];
    const int m = p.mstart[lvl] + img * P + loc;
    const float score = sigmoidf_(p.cls[(long long)m * p.ld_cls + c]);
    if (p.paa) {      // paa_head.py:587-599: the NMS score itself is thresholded, score_factors=None
      const float ns = sqrtf(score * sigmoidf_(p.ctr[(long long)m * p.ld_ctr]));
      if (ns > p.score_thr) out = ns;
    } else if (score > p.score_thr) out = score * sigmoidf_(p.ctr[(long long)m * p.ld_ctr]);
  }
  p.pairscore[((long long)img * p.nlvl + lvl) * p.nms_pre * p.num_classes + t] = out;
}

// the box of location `loc` of (image, level), row m of the head outputs: decode and clip to the image's img_shape
__device__ __forceinline__ void det_decode(const DetK& p, int img, int lvl, int loc, int m, float* b) {
  const float* rc = p.rc + (long long)m * p.ld_rc;
  const int s = p.stride[lvl];
  const int y = loc / p.w[lvl], x = loc - y * p.w[lvl];
  const float H = p.img_shapes[2 * img], W = p.img_shapes[2 * img + 1];
  if (p.fovea) {
    // the point (s (x + 0.5), s (y + 0.5)), distances base_len * exp(raw) - no Scale: p.scales is not read - and the clamp to
    // img_shape - 1 (fovea_head.py:130-132,317,326-333)
    const float fx = (float)s * ((float)x + 0.5f), fy = (float)s * ((float)y + 0.5f);
    const float bl = p.base_len[lvl];
    b[0] = fminf(fmaxf(fx - bl * expf(rc[0]), 0.f), W - 1.f);
    b[1] = fminf(fmaxf(fy - bl * expf(rc[1]), 0.f), H - 1.f);
    b[2] = fminf(fmaxf(fx + bl * expf(rc[2]), 0.f), W - 1.f);
    b[3] = fminf(fmaxf(fy + bl * expf(rc[3]), 0.f), H - 1.f);
    return;
  }
  const float half = p.point_origin ? 0.f : (float)(s / 2);      // (autoassign_head.py:173-187: no half-stride offset)
  const float px = (float)x * (float)s + half, py = (float)y * (float)s + half;
  const float sc = p.scales[lvl];
  if (p.gfl_R) {
    // per side the softmax expectation over its R bins of scale x (Integral, gfl_head.py:15-48), times the stride; distance2bbox from
    // the anchor centre (x s, y s), clipped to img_shape (gfl_head.py:416-426)
    float d[4];
    for (int e = 0; e < 4; ++e) {
      const float* z = rc + e * p.gfl_R;
      float mx = z[0] * sc;
      for (int j = 1; j < p.gfl_R; ++j) mx = fmaxf(mx, z[j] * sc);
      float S = 0.f, A = 0.f;
      for (int j = 0; j < p.gfl_R; ++j) {
        const float ex = expf(z[j] * sc - mx);
        S += ex;
        A += (float)j * ex;
      }
      d[e] = A / S * (float)s;
    }
    const float ax = (float)x * (float)s, ay = (float)y * (float)s;
    b[0] = fminf(fmaxf(ax - d[0], 0.f), W);
    b[1] = fminf(fmaxf(ay - d[1], 0.f), H);
    b[2] = fminf(fmaxf(ax + d[2], 0.f), W);
    b[3] = fminf(fmaxf(ay + d[3], 0.f), H);
    return;
  }
  if (p.atss) {
    // anchor centre (x s, y s), side a = anchor_scale * s; delta2bbox with max_shape = img_shape (delta_xywh_bbox_coder.py:209-269):
    // d = scale * x * stds, dw / dh clamped to +-|log(16 / 1000)|
    const float mr = 4.135166556742356f;
    const float a = p.anchor_scale * (float)s;
    const float d0 = rc[0] * sc * p.stds[0], d1 = rc[1] * sc * p.stds[1], d2 = rc[2] * sc * p.stds[2], d3 = rc[3] * sc * p.stds[3];
    const float gw = a * expf(fminf(fmaxf(d2, -mr), mr)), gh = a * expf(fminf(fmaxf(d3, -mr), mr));
    const float gx = (float)x * (float)s + a * d0, gy = (float)y * (float)s + a * d1;
    b[0] = fminf(fmaxf(gx - gw * 0.5f, 0.f), W);
    b[1] = fminf(fmaxf(gy - gh * 0.5f, 0.f), H);
    b[2] = fminf(fmaxf(gx + gw * 0.5f, 0.f), W);
    b[3] = fminf(fmaxf(gy + gh * 0.5f, 0.f), H);
    return;
  }
  float d[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = p.exp_decode ? expf(rc[e] * sc) : fmaxf(rc[e] * sc, 0.f) * (float)s;      // fcos_head.py:159-167 (eval)
  b[0] = px - d[0]; b[1] = py - d[1]; b[2] = px + d[2]; b[3] = py + d[3];
  b[0] = fminf(fmaxf(b[0], 0.f), W);                    // distance2bbox clip (transforms.py:150-160)
  b[1] = fminf(fmaxf(b[1], 0.f), H);
  b[2] = fminf(fmaxf(b[2], 0.f), W);
  b[3] = fminf(fmaxf(b[3], 0.f), H);
}

// one candidate: decode the box of pair i (level, slot, class) and store it in candidate slot `out`
__device__ __forceinline__ void det_emit(const DetK& p, int img, const float* ps, int i, unsigned out) {
  if (out >= (unsigned)CAND_CAP) return;
  const float f = ps[i];
  const int c = i % p.num_classes;
  float b[4];
  if (p.pool) {          // merged views: the row holds the box, decoded and mapped back by its view's collect
    const float* row = p.pool + (long long)(i / p.num_classes) * p.pool_ld;
    b[0] = row[0]; b[1] = row[1]; b[2] = row[2]; b[3] = row[3];
  } else {
    const int slot = (i / p.num_classes) % p.nms_pre;
    const int lvl = i / (p.num_classes * p.nms_pre);
    const int P = p.h[lvl] * p.w[lvl];
    const int loc = p.sel[((long long)img * p.nlvl + lvl) * p.nms_pre + slot];
    det_decode(p, img, lvl, loc, p.mstart[lvl] + img * P + loc, b);
  }
  if (p.scale_factors) {
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = b[e] / p.scale_factors[4 * img + e];
  }
  float* cb = p.cbox + ((long long)img * CAND_CAP + out) * 4;
  cb[0] = b[0]; cb[1] = b[1]; cb[2] = b[2]; cb[3] = b[3];
  p.cscore[(long long)img * CAND_CAP + out] = f;
  p.clabel[(long long)img * CAND_CAP + out] = c;
}

// Candidate compaction, common case (at most CAND_CAP valid pairs - always, once the detector is trained): DET_CB
// workgroups per image, each owns a contiguous chunk of the (level, slot, class) index range.  Pass 1 counts the chunk's
// valid pairs; pass 2 places them behind the chunks in front of it, in index order inside the chunk (ordered_compact):
// the same candidate order as one workgroup walking all 400 000 pairs, which took 370 us.
constexpr int DET_CB = 64;
__device__ __forceinline__ void det_chunk(const DetK& p, int& lo, int& hi) {
  const int per_img = p.nlvl * p.nms_pre * p.num_classes;
  const int chunk = ((per_img + DET_CB - 1) / DET_CB + 255) / 256 * 256;
  lo = min(per_img, (int)blockIdx.x * chunk);
  hi = min(per_img, lo + chunk);
}
__global__ __launch_bounds__(1024) void det_count_kernel(const DetK p) {
  __shared__ unsigned s_cnt;
  const int img = blockIdx.y;
  const float* ps = p.pairscore + (long long)img * p.nlvl * p.nms_pre * p.num_classes;
  int lo, hi;
  det_chunk(p, lo, hi);
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  unsigned local = 0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) local += det_valid(ps[i]) ? 1u : 0u;
  atomicAdd(&s_cnt, local);            // integer count: order-independent
  __syncthreads();
  if (threadIdx.x == 0) p.ccount[p.n + img * DET_CB + blockIdx.x] = (int)s_cnt;
}
__global__ __launch_bounds__(1024) void det_scatter_kernel(const DetK p) {
  __shared__ unsigned s_wave[34], s_total;
  const int img = blockIdx.y;
  const int* cnt = p.ccount + p.n + img * DET_CB;
  unsigned total = 0, before = 0;
  for (int b = 0; b < DET_CB; ++b) {
    const unsigned c = (unsigned)cnt[b];
    total += c;
    before += b < (int)blockIdx.x ? c : 0u;
  }
  if (total > (unsigned)CAND_CAP) return;            // rare: det_compact_kernel selects the best CAND_CAP
  if (blockIdx.x == 0 && threadIdx.x == 0) p.ccount[img] = (int)total;
  const float* ps = p.pairscore + (long long)img * p.nlvl * p.nms_pre * p.num_classes;
  int lo, hi;
  det_chunk(p, lo, hi);
  if (cnt[blockIdx.x] == 0) return;
  ordered_compact(
      hi - lo, 0u, s_wave, [&](int i) { return det_valid(ps[lo + i]); }, [&](int) { return false; },
      [&](int i, unsigned out) { det_emit(p, img, ps, lo + i, before + out); }, &s_total);
}

// one block per image: keep the CAND_CAP best pairs when more than that are valid; candidate slots are assigned in
// (level, slot, class) index order (ordered_compact), so the score-tie order of the NMS below - and with it the whole
// result - is reproducible
__global__ __launch_bounds__(1024) void det_compact_kernel(const DetK p) {
  __shared__ unsigned hist[2048 + 1024];
  __shared__ unsigned s_tmp[2], s_wave[34], s_total;
  const int img = blockIdx.x;
  const int per_img = p.nlvl * p.nms_pre * p.num_classes;
  const float* ps = p.pairscore + (long long)img * per_img;
  unsigned nvalid = 0;
  for (int b = 0; b < DET_CB; ++b) nvalid += (unsigned)p.ccount[p.n + img * DET_CB + b];
  if (nvalid <= (unsigned)CAND_CAP) return;          // det_scatter_kernel did it
  unsigned prefix = 0, need = 0;
  radix_select_block(ps, per_img, CAND_CAP, hist, s_tmp, prefix, need);
  ordered_compact(
      per_img, need, s_wave, [&](int i) { return det_bits(ps[i]) > prefix; },
      // (fewer positive scores than CAND_CAP: prefix 0, and the valid zero scores are the tie group)
      [&](int i) { const float f = ps[i]; return det_valid(f) && det_bits(f) == prefix; },
      [&](int i, unsigned out) { det_emit(p, img, ps, i, out); }, &s_total);
  if (threadIdx.x == 0) p.ccount[img] = min((int)s_total, CAND_CAP);
}

// ---- test-time augmentation: collect a view into the pool, finish over the pool ------------------------------------
// One thread per (level, slot, column) of the view's selected locations (n == 1): column 0 decodes the box, clips it to the
// view's img_shape (get_bboxes with rescale=False), maps it back - bbox_flip against img_shape (transforms.py:20-30), then the
// division by the 4-element scale factor (:54) - and stores it with the centerness; column 1 + c stores sigmoid(cls c).
__global__ void aug_collect_kernel(const DetK p, const AugK a) {
  const int lvl = blockIdx.y;
  const int cols = p.num_classes + 1;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nsel = p.selcnt[lvl];
  if (t == 0) {
    a.selcnt[a.view * p.nlvl + lvl] = nsel;
    if (lvl == 0) {
      for (int e = 0; e < 4; ++e) a.sf[4 * a.view + e] = p.scale_factors[e];
      int* rec = a.rec + 4 * a.view;
      rec[0] = AUG_MAGIC; rec[1] = p.nlvl; rec[2] = p.nms_pre; rec[3] = p.num_classes;
    }
  }
  if (t >= p.nms_pre * cols) return;
  const int slot = t / cols, col = t - slot * cols;
  if (slot >= nsel) return;            // rows behind the count are never read
  const int loc = p.sel[lvl * p.nms_pre + slot];
  const int m = p.mstart[lvl] + loc;
  float* row = a.rows + ((long long)(a.view * p.nlvl + lvl) * p.nms_pre + slot) * a.ld;
  if (col > 0) {
    row[4 + col] = sigmoidf_(p.cls[(long long)m * p.ld_cls + col - 1]);
    return;
  }
  float b[4];
  det_decode(p, 0, lvl, loc, m, b);
  const float H = p.img_shapes[0], W = p.img_shapes[1];
  if (a.flip & 1) { const float x1 = W - b[2], x2 = W - b[0]; b[0] = x1; b[2] = x2; }
  if (a.flip & 2) { const float y1 = H - b[3], y2 = H - b[1]; b[1] = y1; b[3] = y2; }
#pragma unroll
  for (int e = 0; e < 4; ++e) row[e] = b[e] / p.scale_factors[e];
  row[4] = sigmoidf_(p.ctr[(long long)m * p.ld_ctr]);
}

// det_pairscore_kernel over the pool: pair = (view, level, slot, class) in that order, the order merge_aug_bboxes concatenates
__device__ __forceinline__ bool aug_view_ok(const int* rec, int view, int nlvl, const DetK& p) {
  const int* r = rec + 4 * view;
  return r[0] == AUG_MAGIC && r[1] == nlvl && r[2] == p.nms_pre && r[3] == p.num_classes;
}
__global__ void aug_pairscore_kernel(const DetK p, const int* rec, int nlvl, const int* selcnt, long long npair) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npair) return;
  const long long r = t / p.num_classes;
  const int c = (int)(t - r * p.num_classes);
  const int slot = (int)(r % p.nms_pre), grp = (int)(r / p.nms_pre);
  float out = -1.f;
  // a view without this pool's record (not collected for this image, or with other nlvl / nms_pre / num_classes) gives no pair:
  // its counts and rows are not read
  if (aug_view_ok(rec, grp / nlvl, nlvl, p) && slot < selcnt[grp]) {
    const float* row = p.pool + r * p.pool_ld;
    const float score = row[5 + c];
    if (score > p.score_thr) out = score * row[4];
  }
  p.pairscore[t] = out;
}

// rescale=False: the kept boxes in the FIRST view's coordinates (dense_test_mixins.py:99-104)
__global__ void aug_scale_kernel(const DetK p, const float* sf) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.det_count[0] * 4) return;
  p.dets[(t >> 2) * 5 + (t & 3)] *= sf[t & 3];
}

// last launch of finish: det_count = -1 when a view's record is missing or does not match, and the records are consumed, so that
// the counts of this image cannot pass for the next image's in a reused pool
__global__ void aug_status_kernel(const DetK p, int* rec, int nlvl, int nviews) {
  bool ok = true;
  for (int v = 0; v < nviews; ++v) ok = ok && aug_view_ok(rec, v, nlvl, p);
  __syncthreads();                   // one block: every thread has read the records
  if (!ok)                           // the boxes of the views that were there are not a result
    for (int i = threadIdx.x; i < p.max_per_img * 5; i += blockDim.x) p.dets[i] = 0.f;
  if (threadIdx.x == 0) {
    for (int v = 0; v < nviews; ++v) rec[4 * v] = 0;
    if (!ok) p.det_count[0] = -1;
  }
}

__device__ __forceinline__ bool iou_gt(const float* a, const float* b, float thr) {
  // mmcv nms_cuda_kernel.cuh IoU with offset 0
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]), sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (sa + sb - inter) > thr;
}

// descending bitonic sort of np2 (a power of two) keys in LDS by the whole workgroup; the keys are written and a barrier passed
__device__ __forceinline__ void bitonic_desc(unsigned long long* keyidx, int np2) {
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < np2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keyidx[i], b = keyidx[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) {
            keyidx[i] = b;
            keyidx[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
}

// one block per image: sort candidates by score (bitonic, LDS), greedy class-aware NMS, keep max_per_img
__global__ __launch_bounds__(NMS_THREADS) void det_nms_kernel(const DetK p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* keyidx = reinterpret_cast<unsigned long long*>(smem);          // CAND_CAP * 8
  float* kept = reinterpret_cast<float*>(smem + (size_t)CAND_CAP * 8);                // max_per_img * 4 (offset boxes)
  __shared__ float s_red[NMS_THREADS / 64];
  __shared__ int s_nkept, s_flag;
  const int img = blockIdx.x;
  int n = p.ccount[img];
  if (n > CAND_CAP) n = CAND_CAP;
  const float* cbox = p.cbox + (long long)img * CAND_CAP * 4;
  const float* cscore = p.cscore + (long long)img * CAND_CAP;
  const int* clabel = p.clabel + (long long)img * CAND_CAP;
  // max coordinate over the valid boxes (batched_nms: offsets = idxs * (boxes.max() + 1))
  float mx = -3.0e38f;
  for (int i = threadIdx.x; i < n * 4; i += blockDim.x) mx = fmaxf(mx, cbox[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = s_red[0];
  for (int i = 1; i < NMS_THREADS / 64; ++i) mx = fmaxf(mx, s_red[i]);
  const float offs = mx + 1.0f;
  // sort descending by score; ties by ascending candidate slot (deterministic given the slot order)
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = threadIdx.x; i < np2; i += blockDim.x) {
    unsigned long long k = 0ull;
    if (i < n) k = ((unsigned long long)__float_as_uint(cscore[i]) << 32) | (unsigned)(0xffffffffu - (unsigned)i);
    keyidx[i] = k;
  }
  __syncthreads();
  bitonic_desc(keyidx, np2);
  if (threadIdx.x == 0) s_nkept = 0;
  __syncthreads();
  // greedy scan: candidate i survives iff no kept box (same label via the offset trick) has IoU > thr
  const int maxk = p.max_per_img;
  for (int i = 0; i < n; ++i) {
    const int nk = s_nkept;
    if (nk >= maxk) break;
    const int ci = (int)(0xffffffffu - (unsigned)(keyidx[i] & 0xffffffffu));
    const float off = (float)clabel[ci] * offs;
    const float bi[4] = {cbox[4 * ci] + off, cbox[4 * ci + 1] + off, cbox[4 * ci + 2] + off, cbox[4 * ci + 3] + off};
    if (threadIdx.x == 0) s_flag = 0;
    __syncthreads();
    if ((int)threadIdx.x < nk && iou_gt(kept + 4 * threadIdx.x, bi, p.iou_thr)) s_flag = 1;
    __syncthreads();
    if (threadIdx.x == 0 && !s_flag) {
      kept[4 * nk] = bi[0]; kept[4 * nk + 1] = bi[1]; kept[4 * nk + 2] = bi[2]; kept[4 * nk + 3] = bi[3];
      float* o = p.dets + ((long long)img * maxk + nk) * 5;
      o[0] = cbox[4 * ci]; o[1] = cbox[4 * ci + 1]; o[2] = cbox[4 * ci + 2]; o[3] = cbox[4 * ci + 3];
      o[4] = cscore[ci];
      p.det_labels[(long long)img * maxk + nk] = clabel[ci];
      s_nkept = nk + 1;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) p.det_count[img] = s_nkept;
}

// ---- Soft-NMS ------------------------------------------------------------------------------------------------------------------
// The rule of soft_nms_cpu.pyx:39-125, per image and class (batched_nms's class offset keeps classes apart; here a workgroup only
// ever sees one class): pick the highest current score (:52-56), emit it with that score (:59-64), multiply every other
// remaining score of the class by w(IoU with the pick) (:98-111) and drop the candidates that fall below min_score (:115-123).
// IoU is iou_gt's expression on the class-offset boxes, so that DSL_NMS_NAIVE decides exactly as det_nms_kernel does.
constexpr int SOFT_T = 256;
constexpr unsigned SOFT_OUT = 0x8000u;      // s_idx flag: emitted or dropped (candidate slots need 14 bits)

__device__ __forceinline__ float iou_of(const float* a, const float* b) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]), sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (sa + sb - inter);
}

// w of soft_nms_cpu.pyx:98-109.  0 / 0 of two zero-area boxes is no overlap, as in the hard NMS (`>` is false for a NaN)
__device__ __forceinline__ float soft_weight(int method, float iou, float thr, float sigma) {
  if (method == DSL_NMS_GAUSSIAN) return iou > 0.f ? expf(-(iou * iou) / sigma) : 1.f;
  if (!(iou > thr)) return 1.f;
  return method == DSL_NMS_LINEAR ? 1.f - iou : 0.f;
}

// One workgroup per (class, image).  The class's candidate slots are gathered into LDS in slot order; thread t owns list entries
// t, t + T, ...: it alone reads and writes their flags and current scores, so the loop needs one barrier per pick, for the
// arg-max across waves.  A list of at most 64 entries is run by wave 0 alone, without a barrier.  The arg-max key is (score bits,
// ~slot): among equal current scores the lowest candidate slot wins - the order of det_nms_kernel's sort.
__global__ __launch_bounds__(SOFT_T) void det_soft_kernel(const DetK p) {
  __shared__ unsigned short s_idx[CAND_CAP];
  __shared__ unsigned s_wave[34], s_total;
  __shared__ float s_red[SOFT_T / 64];
  __shared__ unsigned long long s_best[2][SOFT_T / 64];
  const int cls = blockIdx.x, img = blockIdx.y;
  int n = p.ccount[img];
  if (n > CAND_CAP) n = CAND_CAP;
  const float* cbox = p.cbox + (long long)img * CAND_CAP * 4;
  const float* cscore = p.cscore + (long long)img * CAND_CAP;
  const int* clabel = p.clabel + (long long)img * CAND_CAP;
  float* cur = p.sscore + (long long)img * CAND_CAP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the class offset of det_nms_kernel: label * (max coordinate over the image's candidates + 1)
  float mx = -3.0e38f;
  for (int i = threadIdx.x; i < n * 4; i += SOFT_T) mx = fmaxf(mx, cbox[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = s_red[0];
  for (int i = 1; i < SOFT_T / 64; ++i) mx = fmaxf(mx, s_red[i]);
  const float off = (float)cls * (mx + 1.0f);
  ordered_compact(
      n, 0u, s_wave, [&](int i) { return clabel[i] == cls; }, [&](int) { return false; },
      [&](int i, unsigned slot) { s_idx[slot] = (unsigned short)i; }, &s_total);
  const int len = (int)s_total;
  const bool wide = len > 64;
  if (!wide && wave) return;
  const int first = wide ? (int)threadIdx.x : lane, step = wide ? SOFT_T : 64;
  for (int k = first; k < len; k += step) cur[s_idx[k]] = cscore[s_idx[k]];
  // A class places at most max_per_img detections in the result and its picks come out in descending score order (a score only
  // ever shrinks, and a pick is the maximum of what is left): the picks behind the first max_per_img cannot be among the image's
  // best max_per_img, so stopping here is exact.
  for (int it = 0; it < p.max_per_img; ++it) {
    unsigned long long best = 0ull;                  // no entry left; an entry's key is never 0 (~slot != 0)
    for (int k = first; k < len; k += step) {
      const unsigned e = s_idx[k];
      if (e & SOFT_OUT) continue;
      const unsigned long long key = ((unsigned long long)__float_as_uint(cur[e]) << 32) | (0xffffffffu - e);
      best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (wide) {
      // two buffers by parity: a wave that is early for pick it + 1 writes the other buffer, and nobody writes this one again
      // before every wave has passed the barrier of pick it + 1, behind its reads of pick it
      if (lane == 0) s_best[it & 1][wave] = best;
      __syncthreads();
      best = s_best[it & 1][0];
      for (int w = 1; w < SOFT_T / 64; ++w) best = s_best[it & 1][w] > best ? s_best[it & 1][w] : best;
    }
    if (best == 0ull) break;
    const unsigned pick = 0xffffffffu - (unsigned)(best & 0xffffffffu);
    const float bp[4] = {cbox[4 * pick] + off, cbox[4 * pick + 1] + off, cbox[4 * pick + 2] + off, cbox[4 * pick + 3] + off};
    for (int k = first; k < len; k += step) {
      const unsigned e = s_idx[k];
      if (e & SOFT_OUT) continue;
      if (e == pick) {                               // emitted with its current score, which stays in cur
        s_idx[k] = (unsigned short)(e | SOFT_OUT);
        continue;
      }
      const float be[4] = {cbox[4 * e] + off, cbox[4 * e + 1] + off, cbox[4 * e + 2] + off, cbox[4 * e + 3] + off};
      float s = cur[e] * soft_weight(p.nms_method, iou_of(bp, be), p.iou_thr, p.soft_sigma);
      if (s < p.soft_min_score) {
        s_idx[k] = (unsigned short)(e | SOFT_OUT);
        s = -1.f;
      }
      cur[e] = s;
    }
  }
  for (int k = first; k < len; k += step)            // still in the running behind the class's last pick: not emitted
    if (!(s_idx[k] & SOFT_OUT)) cur[s_idx[k]] = -1.f;
}

// one block per image: the emitted candidates of all classes by rescored score, descending (equal scores: ascending candidate
// slot), the first max_per_img
__global__ __launch_bounds__(NMS_THREADS) void det_soft_final_kernel(const DetK p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* keyidx = reinterpret_cast<unsigned long long*>(smem);          // CAND_CAP * 8
  __shared__ int s_count;
  const int img = blockIdx.x;
  int n = p.ccount[img];
  if (n > CAND_CAP) n = CAND_CAP;
  const float* cbox = p.cbox + (long long)img * CAND_CAP * 4;
  const int* clabel = p.clabel + (long long)img * CAND_CAP;
  const float* cur = p.sscore + (long long)img * CAND_CAP;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = threadIdx.x; i < np2; i += blockDim.x) {
    unsigned long long k = 0ull;                     // not emitted: behind every emitted one, whose key is never 0
    if (i < n && cur[i] >= 0.f) k = ((unsigned long long)__float_as_uint(cur[i]) << 32) | (unsigned)(0xffffffffu - (unsigned)i);
    keyidx[i] = k;
  }
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  bitonic_desc(keyidx, np2);
  const int maxk = p.max_per_img, lim = min(n, maxk);
  for (int r = threadIdx.x; r < lim; r += blockDim.x) {
    const unsigned long long key = keyidx[r];
    if (key == 0ull) continue;
    const int ci = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
    float* o = p.dets + ((long long)img * maxk + r) * 5;
    o[0] = cbox[4 * ci]; o[1] = cbox[4 * ci + 1]; o[2] = cbox[4 * ci + 2]; o[3] = cbox[4 * ci + 3];
    o[4] = cur[ci];
    p.det_labels[(long long)img * maxk + r] = clabel[ci];
    if (r + 1 == lim || keyidx[r + 1] == 0ull) s_count = r + 1;          // the last emitted rank: one writer
  }
  __syncthreads();
  if (threadIdx.x == 0) p.det_count[img] = s_count;
}

// ---- pseudo-label fuse step of the refresh (unlabel_pred_hook.py:84-171) -----------------------------------------
// One block per image over its <= max_per_img detections: keep score >= parse_thr, truncate the coordinates toward
// zero (int(), parse_det_results :27), round the score to 6 decimals (:35), then per class (ascending, classes
// 0 .. num_classes-1) mmcv.ops.nms(boxes, scores, iou_threshold, score_threshold): candidates with score > nms_thr in
// descending score order (ties: earlier detection first), greedy, suppress IoU > iou_thr (offset 0).
// fuse_history=True (:131-141): the image's previous labels (old_*: boxes, scores and class indices as the label file
// held them - not truncated, not thresholded by parse_thr) come first in the candidate list, the new detections after.
struct FuseK {
  int n, maxk, num_classes, max_old, max_out;
  float parse_thr, iou_thr, nms_thr;
  const float* dets; const long long* labels; const int* count;
  const float* old_boxes; const float* old_scores; const long long* old_labels; const int* old_count;
  float* out_boxes; float* out_scores; long long* out_labels; int* out_count;
};

constexpr int FUSE_T = 256, FUSE_MAX = 1024;
__global__ __launch_bounds__(FUSE_T) void pseudo_fuse_kernel(const FuseK p) {
  __shared__ float bx[FUSE_MAX][4];
  __shared__ float sc[FUSE_MAX];
  __shared__ int lb[FUSE_MAX];          // -1: dropped
  __shared__ int order[FUSE_MAX];       // candidate index at each rank of (label asc, score desc, index asc)
  __shared__ int kept[FUSE_MAX];
  __shared__ int s_nk, s_flag, s_ncand, s_cls0;
  const int img = blockIdx.x;
  const int ko = p.old_boxes ? min(p.old_count[img], p.max_old) : 0;
  const int k = ko + min(p.count[img], p.maxk);          // ko + k <= FUSE_MAX (checked by the caller)
  for (int i = threadIdx.x; i < ko; i += FUSE_T) {
    const long long o = (long long)img * p.max_old + i;
    const float s = p.old_scores[o];
    const int l = (int)p.old_labels[o];
#pragma unroll
    for (int e = 0; e < 4; ++e) bx[i][e] = p.old_boxes[o * 4 + e];
    sc[i] = s;
    lb[i] = (l >= 0 && l < p.num_classes && s > p.nms_thr) ? l : -1;
  }
  for (int i = ko + threadIdx.x; i < k; i += FUSE_T) {
    const float* d = p.dets + ((long long)img * p.maxk + (i - ko)) * 5;
    const float s = d[4];
    const int l = (int)p.labels[(long long)img * p.maxk + (i - ko)];
    const float rs = (float)(nearbyint((double)s * 1e6) / 1e6);
#pragma unroll
    for (int e = 0; e < 4; ++e) bx[i][e] = (float)(int)d[e];
    sc[i] = rs;
    lb[i] = (s >= p.parse_thr && l >= 0 && l < p.num_classes && rs > p.nms_thr) ? l : -1;
  }
  if (threadIdx.x == 0) {
    s_nk = 0;
    s_ncand = 0;
  }
  __syncthreads();
  // rank by counting (k <= 1024): dropped entries go last
  for (int i = threadIdx.x; i < k; i += FUSE_T) {
    int r = 0;
    const int li = lb[i] < 0 ? 0x7fffffff : lb[i];
    for (int j = 0; j < k; ++j) {
      const int lj = lb[j] < 0 ? 0x7fffffff : lb[j];
      const bool before = lj < li || (lj == li && (sc[j] > sc[i] || (sc[j] == sc[i] && j < i)));
      r += before ? 1 : 0;
    }
    order[r] = i;
    if (lb[i] >= 0) atomicAdd(&s_ncand, 1);
  }
  __syncthreads();
  const int nc = s_ncand;
  for (int r = 0; r < nc; ++r) {
    const int ci = order[r];
    const int nk = s_nk;
    if (threadIdx.x == 0) {
      s_flag = 0;
      if (r == 0 || lb[order[r - 1]] != lb[ci]) s_cls0 = nk;      // first kept slot of this class
    }
    __syncthreads();
    for (int t = s_cls0 + threadIdx.x; t < nk; t += FUSE_T)
      if (iou_gt(bx[kept[t]], bx[ci], p.iou_thr)) s_flag = 1;
    __syncthreads();
    if (threadIdx.x == 0 && !s_flag) {
      kept[nk] = ci;
      s_nk = nk + 1;
    }
    __syncthreads();
  }
  const int nk = s_nk;      // <= max_out: max_out >= max_old + maxk
  for (int t = threadIdx.x; t < nk; t += FUSE_T) {
    const int ci = kept[t];
    float* ob = p.out_boxes + ((long long)img * p.max_out + t) * 4;
    ob[0] = bx[ci][0]; ob[1] = bx[ci][1]; ob[2] = bx[ci][2]; ob[3] = bx[ci][3];
    p.out_scores[(long long)img * p.max_out + t] = sc[ci];
    p.out_labels[(long long)img * p.max_out + t] = lb[ci];
  }
  if (threadIdx.x == 0) p.out_count[img] = nk;
}

// ---- PAA score voting (paa_head.py:608-673) ---------------------------------------------------------------------------------------
// One workgroup per image, one wavefront per kept detection at a time: over the image's candidates of the detection's class (the pairs
// dsl_fcos_detect keeps, every one above score_thr) with IoU > 0.01 against the kept box - bbox_overlaps, union clamped at 1e-6 -
// p = exp(-(1 - iou)^2 / 0.025) * score; the box becomes sum p * box / sum p (accumulated in fp64, butterfly sums of fixed order), the
// score stays.  Then the detections are rewritten class ascending, within a class in the NMS's order (the reference's loop order).
__global__ __launch_bounds__(NMS_THREADS) void det_vote_kernel(const DetK p) {
  __shared__ float s_box[NMS_THREADS * 5];
  __shared__ int s_lab[NMS_THREADS];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = p.det_count[img];
  int n = p.ccount[img];
  if (n > CAND_CAP) n = CAND_CAP;
  const float* cbox = p.cbox + (long long)img * CAND_CAP * 4;
  const float* cscore = p.cscore + (long long)img * CAND_CAP;
  const int* clabel = p.clabel + (long long)img * CAND_CAP;
  float* dets = p.dets + (long long)img * p.max_per_img * 5;
  long long* labels = p.det_labels + (long long)img * p.max_per_img;
  for (int k = wave; k < nk; k += NMS_THREADS / 64) {
    const float d0 = dets[5 * k], d1 = dets[5 * k + 1], d2 = dets[5 * k + 2], d3 = dets[5 * k + 3];
    const int lab = (int)labels[k];
    const float ad = (d2 - d0) * (d3 - d1);
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < n; i += 64) {
      if (clabel[i] != lab) continue;
      const f32x4 b = *reinterpret_cast<const f32x4*>(cbox + 4 * i);
      const float iw = fmaxf(fminf(d2, b[2]) - fmaxf(d0, b[0]), 0.f), ih = fmaxf(fminf(d3, b[3]) - fmaxf(d1, b[1]), 0.f);
      const float ov = iw * ih;
      const float iou = ov / fmaxf(ad + (b[2] - b[0]) * (b[3] - b[1]) - ov, 1e-6f);
      if (!(iou > 0.01f)) continue;
      const float w = expf(-((1.f - iou) * (1.f - iou)) / 0.025f) * cscore[i];
      acc[0] += (double)w * b[0]; acc[1] += (double)w * b[1]; acc[2] += (double)w * b[2]; acc[3] += (double)w * b[3];
      acc[4] += (double)w;
    }
#pragma unroll
    for (int e = 0; e < 5; ++e)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    if (lane == 0) {
      // (the kept box is one of its own candidates at IoU 1, so the sum is positive; a pool cut at CAND_CAP could drop it: keep the box)
      const bool ok = acc[4] > 0.0;
      s_box[5 * k] = ok ? (float)(acc[0] / acc[4]) : d0; s_box[5 * k + 1] = ok ? (float)(acc[1] / acc[4]) : d1;
      s_box[5 * k + 2] = ok ? (float)(acc[2] / acc[4]) : d2; s_box[5 * k + 3] = ok ? (float)(acc[3] / acc[4]) : d3;
      s_box[5 * k + 4] = dets[5 * k + 4];
      s_lab[k] = lab;
    }
  }
  __syncthreads();
  if (tid < nk) {
    const int lab = s_lab[tid];
    int rank = 0;
    for (int j = 0; j < nk; ++j) rank += (s_lab[j] < lab || (s_lab[j] == lab && j < tid)) ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 5; ++e) dets[5 * rank + e] = s_box[5 * tid + e];
    labels[rank] = lab;
  }
}

size_t ws_layout(const dsl_det_desc* d, size_t off[9]) {
  long long M = 0;
  for (int l = 0; l < d->nlvl; ++l) M += (long long)d->n * d->h[l] * d->w[l];
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) / 256 * 256; return r; };
  off[0] = take(M * 4);                                           // keys
  off[1] = take((size_t)d->n * d->nlvl * d->nms_pre * 4);         // sel
  off[2] = take((size_t)d->n * d->nlvl * 4);                      // selcnt
  off[3] = take((size_t)d->n * CAND_CAP * 16);                    // cbox
  off[4] = take((size_t)d->n * CAND_CAP * 4);                     // cscore
  off[5] = take((size_t)d->n * CAND_CAP * 4);                     // clabel
  off[6] = take((size_t)d->n * 4 * (1 + DET_CB));                 // ccount, then DET_CB chunk counts per image
  off[7] = take((size_t)d->n * d->nlvl * d->nms_pre * d->num_classes * 4);   // pairscore
  off[8] = take(d->nms_method ? (size_t)d->n * CAND_CAP * 4 : 0);  // Soft-NMS: current scores (a zeroed field: the size as before)
  return o;
}

// the pool of `nviews` views: [0] per-view records and valid rows per (view, level), [1] scale factors, [2] rows, then what finish needs
size_t aug_layout(const dsl_det_desc* d, int nviews, size_t off[10]) {
  const size_t rows = (size_t)nviews * d->nlvl * d->nms_pre;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) / 256 * 256; return r; };
  off[0] = take((size_t)nviews * (4 + d->nlvl) * 4);             // per-view records [nviews][4], then the counts [nviews][nlvl]
  off[1] = take((size_t)nviews * 16);
  off[2] = take(rows * (d->num_classes + 5) * 4);
  off[3] = take(rows * d->num_classes * 4);                      // pairscore
  off[4] = take((size_t)CAND_CAP * 16);                           // cbox
  off[5] = take((size_t)CAND_CAP * 4);                            // cscore
  off[6] = take((size_t)CAND_CAP * 4);                            // clabel
  off[7] = take((size_t)4 * (1 + DET_CB));                        // ccount
  off[8] = take(d->nms_method ? (size_t)CAND_CAP * 4 : 0);        // Soft-NMS: current scores
  off[9] = o;
  return o;
}

int aug_check(const dsl_det_desc* d, int nviews, const char* who) {
  DSL_CHECK(d && d->nlvl >= 1 && d->nlvl <= DSL_MAX_SEG, "%s: bad descriptor", who);
  DSL_CHECK(nviews >= 1 && nviews <= DSL_MAX_AUG, "%s: %d views, at most DSL_MAX_AUG = %d are merged", who, nviews, DSL_MAX_AUG);
  DSL_CHECK(d->n == 1, "%s: one image per view (n == 1, as aug_test_bboxes), got n = %d", who, d->n);
  DSL_CHECK(d->num_classes >= 1, "%s: num_classes must be >= 1, got %d", who, d->num_classes);
  DSL_CHECK(d->nms_pre > 0, "%s: nms_pre must be > 0, got %d", who, d->nms_pre);
  DSL_CHECK((long long)nviews * d->nlvl * d->nms_pre * d->num_classes < (1ll << 31), "%s: nms_pre * num_classes too large", who);
  return 0;
}

// the nms_method / soft_* fields of a descriptor (all zero: the hard NMS)
int soft_check(const dsl_det_desc* d, const char* who) {
  DSL_CHECK(d->nms_method >= DSL_NMS_HARD && d->nms_method <= DSL_NMS_NAIVE, "%s: nms_method must be a DSL_NMS_* code, got %d", who, d->nms_method);
  DSL_CHECK(d->nms_method != DSL_NMS_GAUSSIAN || d->soft_sigma > 0.f, "%s: soft_sigma must be > 0 for DSL_NMS_GAUSSIAN, got %g", who,
            (double)d->soft_sigma);
  DSL_CHECK(d->nms_method == DSL_NMS_HARD || d->soft_min_score >= 0.f, "%s: soft_min_score must be >= 0, got %g", who, (double)d->soft_min_score);
  return 0;
}

void launch_nms(const DetK& k, int n, hipStream_t st) {
  if (k.nms_method != DSL_NMS_HARD) {
    static bool soft_attr = false;
    if (!soft_attr) {
      hipFuncSetAttribute((const void*)det_soft_final_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)CAND_CAP * 8));
      soft_attr = true;
    }
    hipLaunchKernelGGL(det_soft_kernel, dim3(k.num_classes, n), dim3(SOFT_T), 0, st, k);
    hipLaunchKernelGGL(det_soft_final_kernel, dim3(n), dim3(NMS_THREADS), (size_t)CAND_CAP * 8, st, k);
    return;
  }
  const size_t lds = (size_t)CAND_CAP * 8 + (size_t)k.max_per_img * 16;
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)det_nms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)CAND_CAP * 8 + NMS_THREADS * 16));
    attr = true;
  }
  hipLaunchKernelGGL(det_nms_kernel, dim3(n), dim3(NMS_THREADS), lds, st, k);
}

// fills the per-view part of a DetK (geometry, head outputs, the view's scratch)
int view_detk(const dsl_det_desc* d, DetK& k, int& m_out, const char* who) {
  size_t off[9];
  const size_t need = ws_layout(d, off);
  DSL_CHECK(d->workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, d->workspace_bytes, need);
  memset(&k, 0, sizeof(k));
  k.nlvl = d->nlvl; k.n = d->n; k.num_classes = d->num_classes; k.nms_pre = d->nms_pre; k.max_per_img = d->max_per_img;
  int m = 0;
  for (int l = 0; l < d->nlvl; ++l) {
    k.h[l] = d->h[l]; k.w[l] = d->w[l]; k.stride[l] = d->stride[l];
    k.mstart[l] = m;
    m += d->n * d->h[l] * d->w[l];
  }
  k.mstart[d->nlvl] = m;
  k.score_thr = d->score_thr; k.iou_thr = d->iou_thr;
  k.cls = d->cls_logits; k.ld_cls = d->ld_cls; k.rc = d->regctr; k.ld_rc = d->ld_rc;
  k.ctr = d->ctr ? d->ctr : d->regctr + 4; k.ld_ctr = d->ctr ? d->ld_ctr : d->ld_rc;
  k.exp_decode = (d->head_flags & DSL_HEAD_EXP_DECODE) ? 1 : 0;
  if (d->head_flags & DSL_HEAD_ATSS) {
    const dsl_atss_desc* a = reinterpret_cast<const dsl_det_atss_desc*>(d)->atss;      // the flag says: d is a dsl_det_atss_desc's first member
    DSL_CHECK(a && a->anchor_scale > 0.f && a->anchor_scale < 1e30f, "%s: DSL_HEAD_ATSS needs a dsl_det_atss_desc whose atss has anchor_scale > 0", who);
    DSL_CHECK(!k.exp_decode && !d->ctr, "%s: DSL_HEAD_ATSS goes with no other decode flag and centerness on the regression tower", who);
    k.atss = 1; k.anchor_scale = a->anchor_scale;
    for (int e = 0; e < 4; ++e) {
      DSL_CHECK(a->delta_stds[e] > 0.f && a->delta_stds[e] < 1e30f, "%s: delta_stds must be finite and > 0", who);
      k.stds[e] = a->delta_stds[e];
    }
  }
  if (d->head_flags & DSL_HEAD_GFL) {
    const dsl_det_gfl_desc* g = reinterpret_cast<const dsl_det_gfl_desc*>(d);      // the flag says: d is a dsl_det_gfl_desc's first member
    DSL_CHECK(g->reg_max >= 1 && g->reg_max <= DSL_GFL_MAX_REG, "%s: DSL_HEAD_GFL needs a dsl_det_gfl_desc with reg_max in 1..16", who);
    DSL_CHECK(!k.exp_decode && !k.atss && !d->ctr, "%s: DSL_HEAD_GFL goes with no other decode flag and has no centerness", who);
    DSL_CHECK(d->ld_rc >= 4 * (g->reg_max + 1), "%s: ld_rc must hold 4 (reg_max + 1) columns", who);
    k.gfl_R = g->reg_max + 1;
  }
  if (d->head_flags & DSL_HEAD_FOVEA) {
    const dsl_det_fovea_desc* f = reinterpret_cast<const dsl_det_fovea_desc*>(d);      // the flag says: d is a dsl_det_fovea_desc's first member
    DSL_CHECK(d->head_flags == DSL_HEAD_FOVEA && !d->ctr, "%s: DSL_HEAD_FOVEA goes with no other flag and has no centerness", who);
    for (int l = 0; l < d->nlvl; ++l) {
      DSL_CHECK(f->base_len[l] > 0.f && f->base_len[l] < 1e30f, "%s: DSL_HEAD_FOVEA needs a dsl_det_fovea_desc with base_len > 0", who);
      k.base_len[l] = f->base_len[l];
    }
    k.fovea = 1;
  }
  if (d->head_flags & DSL_HEAD_AUTOASSIGN) {
    DSL_CHECK(d->head_flags == DSL_HEAD_AUTOASSIGN && !d->ctr,
              "%s: DSL_HEAD_AUTOASSIGN goes with no other flag and the objectness on the regression tower (ctr must be null)", who);
    k.point_origin = 1;
  }
  if (d->head_flags & (DSL_HEAD_GFL | DSL_HEAD_FOVEA)) {      // no centerness factor: the unit "logit"
    void* one = nullptr;
    DSL_CHECK(hipGetSymbolAddress(&one, HIP_SYMBOL(kNoCtr)) == hipSuccess && one, "%s: no address for the unit centerness", who);
    k.ctr = (const float*)one; k.ld_ctr = 0;
  }
  if (d->head_flags & DSL_HEAD_PAA) {
    DSL_CHECK(k.atss, "%s: DSL_HEAD_PAA goes with DSL_HEAD_ATSS (the descriptor is a dsl_det_paa_desc around a dsl_det_atss_desc)", who);
    k.paa = 1;
  }
  k.scales = d->scales; k.img_shapes = d->img_shapes; k.scale_factors = d->scale_factors;
  k.dets = d->dets; k.det_labels = (long long*)d->det_labels; k.det_count = d->det_count;
  unsigned char* ws = (unsigned char*)d->workspace;
  k.keys = (float*)(ws + off[0]); k.sel = (int*)(ws + off[1]); k.selcnt = (int*)(ws + off[2]);
  k.cbox = (float*)(ws + off[3]); k.cscore = (float*)(ws + off[4]); k.clabel = (int*)(ws + off[5]);
  k.ccount = (int*)(ws + off[6]);
  k.pairscore = (float*)(ws + off[7]);
  k.nms_method = d->nms_method; k.soft_sigma = d->soft_sigma; k.soft_min_score = d->soft_min_score;
  k.sscore = (float*)(ws + off[8]);
  m_out = m;
  return 0;
}

}  // namespace

extern "C" size_t dsl_detect_workspace_bytes(const dsl_det_desc* d) {
  size_t off[9];
  return ws_layout(d, off);
}

extern "C" int dsl_fcos_detect(const dsl_det_desc* d, void* stream) {
  DSL_CHECK(d && d->nlvl >= 1 && d->nlvl <= DSL_MAX_SEG && d->n >= 1, "dsl_fcos_detect: bad descriptor");
  const bool fovea = (d->head_flags & DSL_HEAD_FOVEA) != 0;      // no Scale, four box columns
  DSL_CHECK(d->cls_logits && d->regctr && (d->scales || fovea) && d->img_shapes && d->dets && d->det_labels && d->det_count &&
                d->workspace,
            "dsl_fcos_detect: null pointer");
  DSL_CHECK(d->num_classes >= 1 && d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_rc >= (d->ctr || fovea ? 4 : 5),
            "dsl_fcos_detect: unsupported layout");
  DSL_CHECK(d->max_per_img > 0 && d->max_per_img <= NMS_THREADS && d->nms_pre > 0, "dsl_fcos_detect: max_per_img must be in 1..%d", NMS_THREADS);
  if (soft_check(d, "dsl_fcos_detect")) return -1;
  DetK k;
  int m = 0;
  if (view_detk(d, k, m, "dsl_fcos_detect")) return -1;
  const bool vote = k.paa && reinterpret_cast<const dsl_det_paa_desc*>(d)->score_voting != 0;
  DSL_CHECK(!vote || d->nms_method == DSL_NMS_HARD, "dsl_fcos_detect: score_voting is built behind the hard NMS only (nms_method)");
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(k.ccount, 0, sizeof(int) * d->n, st);
  hipMemsetAsync(d->dets, 0, sizeof(float) * 5 * d->n * d->max_per_img, st);
  hipLaunchKernelGGL(det_key_kernel, dim3((m + 255) / 256), dim3(256), 0, st, k);
  hipLaunchKernelGGL(det_select_kernel, dim3(d->nlvl, d->n), dim3(1024), 0, st, k);
  const int per_lvl = d->nms_pre * d->num_classes;
  hipLaunchKernelGGL(det_pairscore_kernel, dim3((per_lvl + 255) / 256, d->nlvl, d->n), dim3(256), 0, st, k);
  hipLaunchKernelGGL(det_count_kernel, dim3(DET_CB, d->n), dim3(1024), 0, st, k);
  hipLaunchKernelGGL(det_scatter_kernel, dim3(DET_CB, d->n), dim3(1024), 0, st, k);
  hipLaunchKernelGGL(det_compact_kernel, dim3(d->n), dim3(1024), 0, st, k);
  launch_nms(k, d->n, st);
  if (vote) hipLaunchKernelGGL(det_vote_kernel, dim3(d->n), dim3(NMS_THREADS), 0, st, k);
  DSL_LAUNCH_CHECK("dsl_fcos_detect");
  return 0;
}

extern "C" size_t dsl_detect_aug_workspace_bytes(const dsl_det_desc* d, int nviews) {
  if (aug_check(d, nviews, "dsl_detect_aug_workspace_bytes")) return 0;
  size_t off[10];
  return aug_layout(d, nviews, off);
}

extern "C" int dsl_fcos_detect_collect(const dsl_det_desc* d, const dsl_det_desc* pool_desc, int view, int nviews, int flip, void* pool,
                                       size_t pool_bytes, void* stream) {
  if (aug_check(d, nviews, "dsl_fcos_detect_collect")) return -1;
  DSL_CHECK(!(d->head_flags & DSL_HEAD_PAA), "dsl_fcos_detect_collect: DSL_HEAD_PAA has no test-time augmentation (paa_head.py:536-538)");
  DSL_CHECK(!(d->head_flags & DSL_HEAD_FOVEA),
            "dsl_fcos_detect_collect: DSL_HEAD_FOVEA has no test-time augmentation (FoveaHead.get_bboxes has no with_nms argument)");
  DSL_CHECK(pool_desc, "dsl_fcos_detect_collect: null pool descriptor");
  if (soft_check(pool_desc, "dsl_fcos_detect_collect")) return -1;          // its nms_method sizes the pool's scratch (aug_layout)
  // the pool is laid out by ITS nlvl / nms_pre / num_classes: a view that differs would write into other views' rows
  DSL_CHECK(d->nlvl == pool_desc->nlvl && d->nms_pre == pool_desc->nms_pre && d->num_classes == pool_desc->num_classes,
            "dsl_fcos_detect_collect: view %d has nlvl %d, nms_pre %d, num_classes %d, the pool %d, %d, %d", view, d->nlvl, d->nms_pre,
            d->num_classes, pool_desc->nlvl, pool_desc->nms_pre, pool_desc->num_classes);
  DSL_CHECK(view >= 0 && view < nviews, "dsl_fcos_detect_collect: view %d of %d", view, nviews);
  DSL_CHECK(flip >= DSL_FLIP_NONE && flip <= DSL_FLIP_DIAGONAL, "dsl_fcos_detect_collect: flip must be a DSL_FLIP_* code, got %d", flip);
  DSL_CHECK(d->cls_logits && d->regctr && d->scales && d->img_shapes && d->scale_factors && d->workspace && pool,
            "dsl_fcos_detect_collect: null pointer (the map-back needs img_shapes and scale_factors)");
  DSL_CHECK(d->ld_cls % 4 == 0 && d->ld_cls >= d->num_classes && d->ld_rc >= (d->ctr ? 4 : 5), "dsl_fcos_detect_collect: unsupported layout");
  size_t off[10];
  const size_t need = aug_layout(pool_desc, nviews, off);
  DSL_CHECK(pool_bytes >= need, "dsl_fcos_detect_collect: pool too small (%zu < %zu)", pool_bytes, need);
  DetK k;
  int m = 0;
  if (view_detk(d, k, m, "dsl_fcos_detect_collect")) return -1;
  unsigned char* pw = (unsigned char*)pool;
  AugK a;
  a.view = view; a.flip = flip;
  a.rec = (int*)(pw + off[0]); a.selcnt = a.rec + 4 * nviews; a.sf = (float*)(pw + off[1]);
  a.rows = (float*)(pw + off[2]); a.ld = d->num_classes + 5;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(det_key_kernel, dim3((m + 255) / 256), dim3(256), 0, st, k);
  hipLaunchKernelGGL(det_select_kernel, dim3(d->nlvl, 1), dim3(1024), 0, st, k);
  const int per_lvl = d->nms_pre * (d->num_classes + 1);
  hipLaunchKernelGGL(aug_collect_kernel, dim3((per_lvl + 255) / 256, d->nlvl), dim3(256), 0, st, k, a);
  DSL_LAUNCH_CHECK("dsl_fcos_detect_collect");
  return 0;
}

extern "C" int dsl_fcos_detect_finish(const dsl_det_desc* d, int nviews, int rescale, void* pool, size_t pool_bytes, void* stream) {
  if (aug_check(d, nviews, "dsl_fcos_detect_finish")) return -1;
  DSL_CHECK(d->max_per_img > 0 && d->max_per_img <= NMS_THREADS, "dsl_fcos_detect_finish: max_per_img must be in 1..%d, got %d", NMS_THREADS,
            d->max_per_img);
  DSL_CHECK(d->dets && d->det_labels && d->det_count && pool, "dsl_fcos_detect_finish: null pointer");
  if (soft_check(d, "dsl_fcos_detect_finish")) return -1;
  size_t off[10];
  const size_t need = aug_layout(d, nviews, off);
  DSL_CHECK(pool_bytes >= need, "dsl_fcos_detect_finish: pool too small (%zu < %zu)", pool_bytes, need);
  unsigned char* pw = (unsigned char*)pool;
  DetK k;
  memset(&k, 0, sizeof(k));
  k.nlvl = nviews * d->nlvl;           // (view, level) groups: only nlvl * nms_pre * num_classes is formed from it
  k.n = 1; k.num_classes = d->num_classes; k.nms_pre = d->nms_pre; k.max_per_img = d->max_per_img;
  k.score_thr = d->score_thr; k.iou_thr = d->iou_thr;
  k.dets = d->dets; k.det_labels = (long long*)d->det_labels; k.det_count = d->det_count;
  k.pool = (const float*)(pw + off[2]); k.pool_ld = d->num_classes + 5;
  k.pairscore = (float*)(pw + off[3]);
  k.cbox = (float*)(pw + off[4]); k.cscore = (float*)(pw + off[5]); k.clabel = (int*)(pw + off[6]);
  k.ccount = (int*)(pw + off[7]);
  k.nms_method = d->nms_method; k.soft_sigma = d->soft_sigma; k.soft_min_score = d->soft_min_score;
  k.sscore = (float*)(pw + off[8]);
  const long long npair = (long long)k.nlvl * k.nms_pre * k.num_classes;
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(k.ccount, 0, sizeof(int), st);
  hipMemsetAsync(d->dets, 0, sizeof(float) * 5 * d->max_per_img, st);
  int* rec = (int*)(pw + off[0]);
  hipLaunchKernelGGL(aug_pairscore_kernel, dim3((unsigned)((npair + 255) / 256)), dim3(256), 0, st, k, (const int*)rec, d->nlvl,
                     (const int*)(rec + 4 * nviews), npair);
  hipLaunchKernelGGL(det_count_kernel, dim3(DET_CB, 1), dim3(1024), 0, st, k);
  hipLaunchKernelGGL(det_scatter_kernel, dim3(DET_CB, 1), dim3(1024), 0, st, k);
  hipLaunchKernelGGL(det_compact_kernel, dim3(1), dim3(1024), 0, st, k);
  launch_nms(k, 1, st);
  if (!rescale)
    hipLaunchKernelGGL(aug_scale_kernel, dim3((4 * d->max_per_img + 255) / 256), dim3(256), 0, st, k, (const float*)(pw + off[1]));
  hipLaunchKernelGGL(aug_status_kernel, dim3(1), dim3(64), 0, st, k, rec, d->nlvl, nviews);
  DSL_LAUNCH_CHECK("dsl_fcos_detect_finish");
  return 0;
}

extern "C" int dsl_pseudo_label_fuse_history(const float* dets, const int64_t* labels, const int32_t* count, int n, int max_per_img,
                                             const float* old_boxes, const float* old_scores, const int64_t* old_labels,
                                             const int32_t* old_count, int max_old, int num_classes, float parse_thr, float iou_thr,
                                             float nms_thr, float* out_boxes, float* out_scores, int64_t* out_labels,
                                             int32_t* out_count, int max_out, void* stream) {
  DSL_CHECK(dets && labels && count && out_boxes && out_scores && out_labels && out_count, "dsl_pseudo_label_fuse: null pointer");
  DSL_CHECK(n >= 1 && max_per_img >= 1 && max_old >= 0 && max_per_img + max_old <= FUSE_MAX,
            "dsl_pseudo_label_fuse: max_per_img + max_old must be in 1..%d", FUSE_MAX);
  DSL_CHECK(max_old == 0 || (old_boxes && old_scores && old_labels && old_count), "dsl_pseudo_label_fuse_history: null pointer (old labels)");
  DSL_CHECK(max_out >= max_per_img + max_old, "dsl_pseudo_label_fuse: max_out (%d) < max_per_img + max_old (%d)", max_out,
            max_per_img + max_old);
  FuseK k;
  k.n = n; k.maxk = max_per_img; k.num_classes = num_classes; k.max_old = max_old; k.max_out = max_out;
  k.parse_thr = parse_thr; k.iou_thr = iou_thr; k.nms_thr = nms_thr;
  k.dets = dets; k.labels = (const long long*)labels; k.count = count;
  k.old_boxes = max_old ? old_boxes : nullptr; k.old_scores = old_scores; k.old_labels = (const long long*)old_labels;
  k.old_count = old_count;
  k.out_boxes = out_boxes; k.out_scores = out_scores; k.out_labels = (long long*)out_labels; k.out_count = out_count;
  hipLaunchKernelGGL(pseudo_fuse_kernel, dim3(n), dim3(FUSE_T), 0, (hipStream_t)stream, k);
  DSL_LAUNCH_CHECK("pseudo_fuse_kernel");
  return 0;
}

extern "C" int dsl_pseudo_label_fuse(const float* dets, const int64_t* labels, const int32_t* count, int n, int max_per_img,
                                     int num_classes, float parse_thr, float iou_thr, float nms_thr, float* out_boxes,
                                     float* out_scores, int64_t* out_labels, int32_t* out_count, void* stream) {
  DSL_CHECK(dets && labels && count && out_boxes && out_scores && out_labels && out_count, "dsl_pseudo_label_fuse: null pointer");
  DSL_CHECK(n >= 1 && max_per_img >= 1 && max_per_img <= FUSE_MAX, "dsl_pseudo_label_fuse: max_per_img must be in 1..%d", FUSE_MAX);
  return dsl_pseudo_label_fuse_history(dets, labels, count, n, max_per_img, nullptr, nullptr, nullptr, nullptr, 0, num_classes,
                                       parse_thr, iou_thr, nms_thr, out_boxes, out_scores, out_labels, out_count, max_per_img,
                                       stream);
}
