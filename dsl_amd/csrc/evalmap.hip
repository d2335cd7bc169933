// On-device detection evaluation (dsl_amd/evaluation.py: coco_bbox_eval's cell body and accumulation, tpfp_default).
//
// Every figure here is an integer count, a max, or an fp64 / fp32 product, sum, quotient or comparison that the host path
// computes too, so the kernels restate the host's operation ORDER and are compared bit for bit (tests/test_eval_device_gpu.py).
// That is why contraction is off for the whole file: a fused multiply-add changes the last bit of `inter` or `union` and flips
// a match that sits on a threshold.  No fast-math intrinsic, no reciprocal-multiply for a division.
#pragma clang fp contract(off)
#include <limits.h>

#include "common.hpp"

#define EV_GCAP 128                 // ground-truth boxes of one cell staged in LDS (boxes, flags, matched bits / claims)
#define EV_WORDS (EV_GCAP / 32)

// ---------------------------------------------------------------------------------------------------------------------
// COCO: one wave per (category, image) cell, lane = range * T + threshold runs coco_bbox_eval's greedy loop (evaluation.py
// "for ti, t in enumerate(iou_thrs)" body) for its own (range, threshold) over the cell's detections in rank order.
// Ground-truth flag byte: bit 0 crowd, bit 1 + r ignored in range r (crowd | ignore | area outside [lo, hi]).
__device__ __forceinline__ uint32_t ev_gflag(double area, uint32_t crowd, uint32_t ign, const double* ranges, int R) {
  uint32_t f = crowd ? 1u : 0u;
  for (int r = 0; r < R; ++r) {
    const double lo = ranges[2 * r], hi = ranges[2 * r + 1];
    if (crowd || ign || area < lo || area > hi) f |= 2u << r;
  }
  return f;
}

__global__ __launch_bounds__(64) void k_eval_match_coco(int NI, int M, int G, int max_gt, const float* __restrict__ det_boxes,
                                                        const int32_t* __restrict__ det_off, const double* __restrict__ gbox,
                                                        const double* __restrict__ garea, const uint8_t* __restrict__ gcrowd,
                                                        const uint8_t* __restrict__ gign, const int32_t* __restrict__ gt_off,
                                                        const double* __restrict__ thrs, int T, const double* __restrict__ ranges,
                                                        int R, uint8_t* __restrict__ matched, uint8_t* __restrict__ ignored,
                                                        int32_t* __restrict__ npos, uint8_t* __restrict__ ws) {
  __shared__ double s_box[EV_GCAP * 4];
  __shared__ uint8_t s_flag[EV_GCAP];
  __shared__ uint32_t s_bits[EV_WORDS * 64];      // matched ground truth: word w of lane l at [w * 64 + l]
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int d0 = det_off[cell], d1 = det_off[cell + 1], g0 = gt_off[cell], g1 = gt_off[cell + 1];
  if (d0 < 0 || d1 < d0 || d1 > M || g0 < 0 || g1 < g0 || g1 > G) return;
  const int nd = d1 - d0, ng = g1 - g0;
  if (nd == 0 && ng == 0) return;
  const bool staged = ng <= EV_GCAP;
  if (!staged && (ng > max_gt || ws == nullptr)) return;      // the caller sized the workspace for max_gt boxes per cell
  const double* cbox = gbox + (size_t)g0 * 4;
  uint8_t* cws = staged ? nullptr : ws + (size_t)g0 * 64;     // beyond the LDS bitset: one byte per (ground truth, lane)
  if (staged) {
    for (int gi = lane; gi < ng; gi += 64) {
      for (int k = 0; k < 4; ++k) s_box[gi * 4 + k] = cbox[gi * 4 + k];
      s_flag[gi] = (uint8_t)ev_gflag(garea[g0 + gi], gcrowd[g0 + gi], gign[g0 + gi], ranges, R);
    }
    for (int w = 0; w < EV_WORDS; ++w) s_bits[w * 64 + lane] = 0u;
  } else {
    for (int gi = 0; gi < ng; ++gi) cws[(size_t)gi * 64 + lane] = 0;
  }
  __syncthreads();
  auto flag = [&](int gi) -> uint32_t {
    return staged ? (uint32_t)s_flag[gi] : ev_gflag(garea[g0 + gi], gcrowd[g0 + gi], gign[g0 + gi], ranges, R);
  };
  const int c = cell / NI;
  if (lane < R) {
    int cnt = 0;
    for (int gi = 0; gi < ng; ++gi) cnt += ((flag(gi) >> (1 + lane)) & 1u) ? 0 : 1;
    if (cnt) atomicAdd(&npos[c * R + lane], cnt);
  }
  if (nd == 0 || lane >= R * T) return;          // no barrier below this line
  const int r = lane / T, t = lane - r * T;
  const double thr = thrs[t], lo = ranges[2 * r], hi = ranges[2 * r + 1];
  const double cap = 1.0 - 1e-10;
  const double start = thr <= cap ? thr : cap;   // min(t, 1 - 1e-10)
  uint8_t* mrow = matched + (size_t)lane * M + d0;
  uint8_t* irow = ignored + (size_t)lane * M + d0;
  for (int di = 0; di < nd; ++di) {
    const float* b = det_boxes + (size_t)(d0 + di) * 4;
    // xyxy2xywh on .tolist() values: the fp32 corners widened, the extent subtracted in fp64
    const double x = (double)b[0], y = (double)b[1], w = (double)b[2] - (double)b[0], h = (double)b[3] - (double)b[1];
    const double dx2 = x + w, dy2 = y + h, da = w * h;
    double best = start;
    int m = -1;
    for (int pass = 0; pass < 2; ++pass) {
      // the stable partition argsort(gig, kind='mergesort') gives: regular boxes in annotation order, then the ignored ones;
      // the host's `break` fires at the first ignored candidate once a regular box is held, so pass 1 runs only without one
      if (pass == 1 && m >= 0) break;
      for (int gi = 0; gi < ng; ++gi) {
        const uint32_t f = flag(gi);
        if ((int)((f >> (1 + r)) & 1u) != pass) continue;
        const bool crowd = f & 1u;
        if (!crowd) {
          const bool taken = staged ? ((s_bits[(gi >> 5) * 64 + lane] >> (gi & 31)) & 1u) : (cws[(size_t)gi * 64 + lane] != 0);
          if (taken) continue;
        }
        const double* g = staged ? s_box + gi * 4 : cbox + (size_t)gi * 4;
        const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
        const double gx2 = gx + gw, gy2 = gy + gh;
        const double mx2 = dx2 < gx2 ? dx2 : gx2, mx1 = x > gx ? x : gx;
        const double my2 = dy2 < gy2 ? dy2 : gy2, my1 = y > gy ? y : gy;
        double iw = mx2 - mx1, ih = my2 - my1;
        iw = iw > 0.0 ? iw : 0.0;
        ih = ih > 0.0 ? ih : 0.0;
        const double inter = iw * ih;
        const double ga = gw * gh;
        const double uni = crowd ? da : (da + ga) - inter;
        const double iou = inter / (uni > 1e-12 ? uni : 1e-12);
        if (iou < best) continue;
        best = iou;                                // replace on equal: the last of several equal candidates wins
        m = gi;
      }
    }
    uint8_t mt = 0, ig;
    if (m >= 0) {
      mt = 1;
      ig = (uint8_t)((flag(m) >> (1 + r)) & 1u);
      if (staged) s_bits[(m >> 5) * 64 + lane] |= 1u << (m & 31);
      else cws[(size_t)m * 64 + lane] = 1;
    } else {
      ig = (da < lo || da > hi) ? 1 : 0;
    }
    mrow[di] = mt;
    irow[di] = ig;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// VOC: tpfp_default with area_ranges=None for one (class, image) cell.  IoU in fp32 as _overlaps; per detection the max and
// its first argmax over regular + ignore boxes; in rank order the first detection that selects a regular box is the true
// positive, every later one a false positive - stated as a per-box minimum of the ranks that select it ("claim").
__device__ __forceinline__ void ev_voc_best(const float* a, const float* sb, const double* gb, bool staged, int ng, float& best,
                                            int& arg) {
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
  const float area_a = (a2 - a0) * (a3 - a1);
  best = 0.f;
  arg = 0;
  for (int j = 0; j < ng; ++j) {
    float b0, b1, b2, b3;
    if (staged) {
      b0 = sb[j * 4], b1 = sb[j * 4 + 1], b2 = sb[j * 4 + 2], b3 = sb[j * 4 + 3];
    } else {
      b0 = (float)gb[(size_t)j * 4], b1 = (float)gb[(size_t)j * 4 + 1], b2 = (float)gb[(size_t)j * 4 + 2], b3 = (float)gb[(size_t)j * 4 + 3];
    }
    const float area_b = (b2 - b0) * (b3 - b1);
    float iw = (a2 < b2 ? a2 : b2) - (a0 > b0 ? a0 : b0);
    float ih = (a3 < b3 ? a3 : b3) - (a1 > b1 ? a1 : b1);
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    const float uni = (area_a + area_b) - inter;
    const float iou = inter / (uni > 1e-6f ? uni : 1e-6f);
    if (j == 0 || iou > best) {
      best = iou;
      arg = j;
    }
  }
}

__global__ __launch_bounds__(64) void k_eval_match_voc(int M, int G, int max_gt, const float* __restrict__ det_boxes,
                                                       const int32_t* __restrict__ det_off, const double* __restrict__ gbox,
                                                       const uint8_t* __restrict__ gign, const int32_t* __restrict__ gt_off,
                                                       const double* __restrict__ thrs, uint8_t* __restrict__ tp,
                                                       uint8_t* __restrict__ fp, int32_t* __restrict__ ws) {
  __shared__ float s_box[EV_GCAP * 4];
  __shared__ uint8_t s_ig[EV_GCAP];
  __shared__ int32_t s_claim[EV_GCAP];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int d0 = det_off[cell], d1 = det_off[cell + 1], g0 = gt_off[cell], g1 = gt_off[cell + 1];
  if (d0 < 0 || d1 < d0 || d1 > M || g0 < 0 || g1 < g0 || g1 > G) return;
  const int nd = d1 - d0, ng = g1 - g0;
  if (nd == 0) return;
  if (ng == 0) {                                   // no ground truth at all: every detection is a false positive
    for (int di = lane; di < nd; di += 64) tp[d0 + di] = 0, fp[d0 + di] = 1;
    return;
  }
  const bool staged = ng <= EV_GCAP;
  if (!staged && (ng > max_gt || ws == nullptr)) return;
  const double* cbox = gbox + (size_t)g0 * 4;
  const uint8_t* cig = gign + g0;
  int32_t* cws = staged ? nullptr : ws + g0;
  for (int gi = lane; gi < ng; gi += 64) {
    if (staged) {
      for (int k = 0; k < 4; ++k) s_box[gi * 4 + k] = (float)cbox[gi * 4 + k];
      s_ig[gi] = cig[gi];
      s_claim[gi] = INT_MAX;
    } else {
      __hip_atomic_store(&cws[gi], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  const double thr = thrs[0];
  for (int di = lane; di < nd; di += 64) {
    float best;
    int arg;
    ev_voc_best(det_boxes + (size_t)(d0 + di) * 4, s_box, cbox, staged, ng, best, arg);
    if ((double)best >= thr && !(staged ? s_ig[arg] : cig[arg])) {
      if (staged) atomicMin(&s_claim[arg], di);
      else atomicMin(&cws[arg], di);
    }
  }
  __syncthreads();
  for (int di = lane; di < nd; di += 64) {
    float best;
    int arg;
    ev_voc_best(det_boxes + (size_t)(d0 + di) * 4, s_box, cbox, staged, ng, best, arg);
    uint8_t t = 0, f = 0;
    if ((double)best >= thr) {
      if (!(staged ? s_ig[arg] : cig[arg])) {
        const int first = staged ? s_claim[arg] : __hip_atomic_load(&cws[arg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (first == di) t = 1;
        else f = 1;                                // the box is covered by a better-ranked detection
      }
    } else {
      f = 1;
    }
    tp[d0 + di] = t;
    fp[d0 + di] = f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// COCO accumulation: block = category, lane = range * T + threshold walks the category's detections through `perm` (by
// descending score).  tp / fp are integer prefix counts; the walk runs BACKWARDS from their totals so that the precision
// envelope (a suffix max) is at hand, and since rc = tp / npos moves only where tp increments, q[k] = envelope at the first
// i with rc[i] >= recThr[k] is written at exactly those steps (and at i = 0).
#define EV_MAX_REC 128
__global__ __launch_bounds__(64) void k_eval_accumulate(int C, int NI, int M, int R, int T, int NR, const uint8_t* __restrict__ matched,
                                                        const uint8_t* __restrict__ ignored, const int32_t* __restrict__ npos,
                                                        const int32_t* __restrict__ det_off, const int32_t* __restrict__ perm,
                                                        const double* __restrict__ rec_thrs, double* __restrict__ prec) {
  __shared__ double s_thr[EV_MAX_REC];
  const int c = blockIdx.x, lane = threadIdx.x;
  for (int k = lane; k < NR; k += 64) s_thr[k] = rec_thrs[k];
  __syncthreads();
  if (lane >= R * T) return;
  const int r = lane / T;
  double* out = prec + (size_t)lane * NR * C + c;          // prec[r][t][k][c]
  const int np_ = npos[c * R + r];
  if (np_ <= 0) {
    for (int k = 0; k < NR; ++k) out[(size_t)k * C] = -1.0;
    return;
  }
  for (int k = 0; k < NR; ++k) out[(size_t)k * C] = 0.0;
  const int s0 = det_off[c * NI], s1 = det_off[(c + 1) * NI];
  if (s0 < 0 || s1 < s0 || s1 > M) return;
  const int n = s1 - s0;
  if (n == 0) return;
  const uint8_t* mrow = matched + (size_t)lane * M;
  const uint8_t* irow = ignored + (size_t)lane * M;
  const double npd = (double)np_;
  int tp = 0, fp = 0;
  for (int i = 0; i < n; ++i) {
    const int p = perm[s0 + i];
    if ((unsigned)p >= (unsigned)M || irow[p]) continue;
    if (mrow[p]) ++tp;
    else ++fp;
  }
  int kp = 0;                                              // recall thresholds <= rc[i] form a prefix [0, kp)
  {
    const double rc = (double)tp / npd;
    while (kp < NR && s_thr[kp] <= rc) ++kp;
  }
  double env = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    const int p = perm[s0 + i];
    const bool ok = (unsigned)p < (unsigned)M && !irow[p];
    const bool is_tp = ok && mrow[p], is_fp = ok && !mrow[p];
    const double den = (double)(tp + fp);
    const double pr = (double)tp / (den > 2.220446049250313e-16 ? den : 2.220446049250313e-16);
    env = env > pr ? env : pr;
    if (i == 0) {
      for (int k = 0; k < kp; ++k) out[(size_t)k * C] = env;
      break;
    }
    if (is_tp) {
      const double rc_prev = (double)(tp - 1) / npd;
      int kq = kp;
      while (kq > 0 && s_thr[kq - 1] > rc_prev) --kq;
      for (int k = kq; k < kp; ++k) out[(size_t)k * C] = env;
      kp = kq;
      --tp;
    } else if (is_fp) {
      --fp;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t dsl_eval_match_workspace_bytes(int num_gt, int max_gt_per_cell) {
  if (num_gt <= 0 || max_gt_per_cell <= EV_GCAP) return 0;
  return (size_t)num_gt * 64;
}

extern "C" int dsl_eval_match(int mode, int num_cats, int num_imgs, int num_det, int num_gt, int max_gt_per_cell,
                              const float* det_boxes, const int32_t* det_off, const double* gt_boxes, const double* gt_area,
                              const uint8_t* gt_crowd, const uint8_t* gt_ignore, const int32_t* gt_off, const double* iou_thrs,
                              int num_thrs, const double* area_ranges, int num_ranges, uint8_t* out_a, uint8_t* out_b,
                              int32_t* npos, void* workspace, size_t workspace_bytes, void* stream) {
  DSL_CHECK(mode == DSL_EVAL_COCO || mode == DSL_EVAL_VOC, "dsl_eval_match: mode %d", mode);
  DSL_CHECK(num_cats >= 0 && num_imgs >= 0 && num_det >= 0 && num_gt >= 0 && max_gt_per_cell >= 0, "dsl_eval_match: negative size");
  DSL_CHECK(num_thrs >= 1 && num_thrs <= DSL_EVAL_MAX_THRS, "dsl_eval_match: num_thrs must be in 1..%d", DSL_EVAL_MAX_THRS);
  DSL_CHECK(num_ranges >= 1 && num_ranges <= DSL_EVAL_MAX_RANGES, "dsl_eval_match: num_ranges must be in 1..%d", DSL_EVAL_MAX_RANGES);
  DSL_CHECK(num_ranges * num_thrs <= 64, "dsl_eval_match: num_ranges * num_thrs must be <= 64");
  if (mode == DSL_EVAL_VOC)
    DSL_CHECK(num_ranges == 1 && num_thrs == 1, "dsl_eval_match: DSL_EVAL_VOC takes one threshold and no area ranges (num_ranges == 1)");
  const long long cells = (long long)num_cats * num_imgs;
  DSL_CHECK(cells < (1ll << 31) - 1, "dsl_eval_match: num_cats * num_imgs too large");
  DSL_CHECK((long long)num_det * num_ranges * num_thrs < (1ll << 40), "dsl_eval_match: too many detections");
  const size_t need = dsl_eval_match_workspace_bytes(num_gt, max_gt_per_cell);
  DSL_CHECK(need == 0 || (workspace && workspace_bytes >= need), "dsl_eval_match: workspace %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (mode == DSL_EVAL_COCO && num_cats > 0) {
    DSL_CHECK(npos, "dsl_eval_match: npos is null");
    hipError_t e = hipMemsetAsync(npos, 0, sizeof(int32_t) * (size_t)num_cats * num_ranges, st);
    DSL_CHECK(e == hipSuccess, "dsl_eval_match: memset failed: %s", hipGetErrorString(e));
  }
  if (cells == 0 || (num_det == 0 && num_gt == 0)) return 0;
  if (mode == DSL_EVAL_VOC && num_det == 0) return 0;
  DSL_CHECK(det_off && gt_off && iou_thrs, "dsl_eval_match: null offsets or thresholds");
  DSL_CHECK(num_det == 0 || (det_boxes && out_a && out_b), "dsl_eval_match: null detection arrays");
  DSL_CHECK(num_gt == 0 || (gt_boxes && gt_ignore), "dsl_eval_match: null ground-truth arrays");
  if (mode == DSL_EVAL_COCO) {
    DSL_CHECK(area_ranges, "dsl_eval_match: area_ranges is null");
    DSL_CHECK(num_gt == 0 || (gt_area && gt_crowd), "dsl_eval_match: null ground-truth arrays");
    hipLaunchKernelGGL(k_eval_match_coco, dim3((unsigned)cells), dim3(64), 0, st, num_imgs, num_det, num_gt, max_gt_per_cell, det_boxes,
                       det_off, gt_boxes, gt_area, gt_crowd, gt_ignore, gt_off, iou_thrs, num_thrs, area_ranges, num_ranges, out_a,
                       out_b, npos, (uint8_t*)(need ? workspace : nullptr));
    DSL_LAUNCH_CHECK("k_eval_match_coco");
  } else {
    hipLaunchKernelGGL(k_eval_match_voc, dim3((unsigned)cells), dim3(64), 0, st, num_det, num_gt, max_gt_per_cell, det_boxes, det_off,
                       gt_boxes, gt_ignore, gt_off, iou_thrs, out_a, out_b, (int32_t*)(need ? workspace : nullptr));
    DSL_LAUNCH_CHECK("k_eval_match_voc");
  }
  return 0;
}

extern "C" int dsl_eval_accumulate(int num_cats, int num_imgs, int num_det, int num_ranges, int num_thrs, int num_rec,
                                   const uint8_t* matched, const uint8_t* ignored, const int32_t* npos, const int32_t* det_off,
                                   const int32_t* perm, const double* rec_thrs, double* prec, void* stream) {
  DSL_CHECK(num_cats >= 0 && num_imgs >= 0 && num_det >= 0, "dsl_eval_accumulate: negative size");
  DSL_CHECK(num_thrs >= 1 && num_thrs <= DSL_EVAL_MAX_THRS && num_ranges >= 1 && num_ranges <= DSL_EVAL_MAX_RANGES &&
                num_ranges * num_thrs <= 64,
            "dsl_eval_accumulate: num_ranges (1..%d) * num_thrs (1..%d) must be <= 64", DSL_EVAL_MAX_RANGES, DSL_EVAL_MAX_THRS);
  DSL_CHECK(num_rec >= 1 && num_rec <= EV_MAX_REC, "dsl_eval_accumulate: num_rec must be in 1..%d", EV_MAX_REC);
  if (num_cats == 0) return 0;
  DSL_CHECK(npos && det_off && rec_thrs && prec, "dsl_eval_accumulate: null pointer");
  DSL_CHECK(num_det == 0 || (matched && ignored && perm), "dsl_eval_accumulate: null detection arrays");
  hipLaunchKernelGGL(k_eval_accumulate, dim3((unsigned)num_cats), dim3(64), 0, (hipStream_t)stream, num_cats, num_imgs, num_det,
                     num_ranges, num_thrs, num_rec, matched, ignored, npos, det_off, perm, rec_thrs, prec);
  DSL_LAUNCH_CHECK("k_eval_accumulate");
  return 0;
}
