// What the head-loss translation units (fcos_loss.hip, gfl_loss.hip, fovea_loss.hip, autoassign_loss.hip) share: the level geometry of a dsl_fcos_desc with its one host
// fill, the location decoder, the kernel arguments every head's kernels read, and the fixed-order sum of per-block records.
// Include after common.hpp.
#pragma once

// locations are level-major, [level][image][y][x]; level l starts at mstart[l], M = mstart[nlvl]
struct HeadGeom {
  int nlvl, n, M;
  int h[DSL_MAX_SEG], w[DSL_MAX_SEG], stride[DSL_MAX_SEG];
  int mstart[DSL_MAX_SEG + 1];
};

// `who` prefixes the messages.  M stays below 2^31 - 256: location indices are ints, rounded up to whole workgroups
inline int head_geom(const dsl_fcos_desc* d, HeadGeom& g, const char* who) {
  DSL_CHECK(d && d->nlvl >= 1 && d->nlvl <= DSL_MAX_SEG && d->n >= 1, "%s: bad descriptor", who);
  const long long lim = (1ll << 31) - 256;
  g = HeadGeom{};
  g.nlvl = d->nlvl; g.n = d->n;
  long long m = 0;
  for (int l = 0; l < d->nlvl; ++l) {
    DSL_CHECK(d->h[l] >= 1 && d->w[l] >= 1 && d->stride[l] >= 1, "%s: bad level %d", who, l);
    g.h[l] = d->h[l]; g.w[l] = d->w[l]; g.stride[l] = d->stride[l];
    g.mstart[l] = (int)m;
    const long long hw = (long long)d->h[l] * d->w[l];
    DSL_CHECK(hw < lim && m + d->n * hw < lim, "%s: too many locations", who);
    m += d->n * hw;
  }
  g.mstart[d->nlvl] = g.M = (int)m;
  return 0;
}

__device__ __forceinline__ void head_loc(const HeadGeom& p, int m, int& lvl, int& img, int& y, int& x) {
  lvl = 0;
#pragma unroll
  for (int s = 1; s < DSL_MAX_SEG; ++s)
    if (s < p.nlvl && m >= p.mstart[s]) lvl = s;
  const int q = m - p.mstart[lvl];
  const int hw = p.h[lvl] * p.w[lvl];
  img = q / hw;
  const int r = q - img * hw;
  y = r / p.w[lvl];
  x = r - y * p.w[lvl];
}

// kernel arguments of every head: FcK (fcos_loss.hip) and GfK (gfl_loss.hip) add what is theirs
struct HeadK : HeadGeom {
  int num_classes;
  long long* labels; float* bbox_targets; float* cls_weight;      // written by the assignment, read by the quality and loss passes
  const float* cls_logits; int ld_cls;
  const float* regctr; int ld_rc;
  const float* scales; const float* norm;
  float inv_world, grad_scale;
  uint16_t* g_cls; int ld_gcls; uint16_t* g_rc; int ld_grc;
  float* g_scales; float* losses; float* logvec;
  float* part;            // block records of the loss / assignment sums (fixed-order second pass, no float atomics)
  int box_kind;           // DSL_BOX_*, eps of DIoU / CIoU, loss_weight of loss_cls / loss_bbox (head_loss_settings)
  float box_eps, w_cls, w_bbox;
};

inline int head_fill(const dsl_fcos_desc* d, HeadK& k, const char* who) {
  if (head_geom(d, k, who)) return -1;
  k.num_classes = d->num_classes;
  k.labels = (long long*)d->labels; k.bbox_targets = d->bbox_targets; k.cls_weight = d->cls_weight;
  k.cls_logits = d->cls_logits; k.ld_cls = d->ld_cls; k.regctr = d->regctr; k.ld_rc = d->ld_rc;
  k.scales = d->scales; k.norm = d->norm; k.inv_world = d->inv_world; k.grad_scale = d->grad_scale;
  k.g_cls = (uint16_t*)d->g_cls; k.ld_gcls = d->ld_gcls; k.g_rc = (uint16_t*)d->g_rc; k.ld_grc = d->ld_grc;
  k.g_scales = d->g_scales; k.losses = d->losses; k.logvec = d->logvec;
  k.part = (float*)d->workspace;
  return 0;
}

// what every loss pass reads and writes
inline int head_loss_ptrs(const dsl_fcos_desc* d, const char* who) {
  DSL_CHECK(d->labels && d->bbox_targets && d->cls_weight && d->cls_logits && d->regctr && d->scales && d->norm && d->g_cls && d->g_rc &&
                d->g_scales && d->losses,
            "%s: null pointer", who);
  return 0;
}

// the loss settings of a DSL_HEAD_LOSS_EXT descriptor that every loss pass reads; w3 = the pass's third loss weight (w_ctr, w_dfl)
inline int head_loss_settings(const dsl_fcos_desc* d, float w3, HeadK& k, const char* who) {
  DSL_CHECK(d->box_kind >= DSL_BOX_GIOU && d->box_kind <= DSL_BOX_CIOU, "%s: box_kind is not a DSL_BOX_* value", who);
  DSL_CHECK(d->box_kind < DSL_BOX_DIOU || (d->box_eps > 0.f && d->box_eps < 1.f), "%s: DIoU / CIoU need 0 < box_eps < 1", who);
  DSL_CHECK(d->w_cls >= 0.f && d->w_cls < 1e30f && d->w_bbox >= 0.f && d->w_bbox < 1e30f && w3 >= 0.f && w3 < 1e30f,
            "%s: loss weights must be finite and >= 0", who);
  k.box_kind = d->box_kind; k.box_eps = d->box_eps; k.w_cls = d->w_cls; k.w_bbox = d->w_bbox;
  return 0;
}

// autoassign_loss.hip: what a DSL_HEAD_AUTOASSIGN descriptor (the first member of a dsl_aa_desc) adds to dsl_fcos_workspace_bytes
size_t dsl_aa_workspace_extra(const dsl_fcos_desc* d);

// grid of a loss pass: one thread per 4 classes of a location, capped at the 2048 records of 16 floats the workspace holds
inline int head_loss_blocks(const HeadK& k) {
  const long long b = ((long long)k.M * ((k.num_classes + 3) / 4) + 255) / 256;
  return b > 2048 ? 2048 : (int)b;
}

// Fixed-order sum of per-block records by one workgroup of REC_T threads: column col0 + v (v < V, V a divisor of REC_T) of
// `nblocks` records `stride` floats apart.  Thread (q, v), Q = REC_T / V, adds blocks q, q + Q, ... in that order; then thread v < V
// adds the Q partial sums in order and returns the total (the other threads return 0).  `sh` is free again on return.
constexpr int REC_T = 256;
__device__ __forceinline__ float record_sum(const float* __restrict__ part, int nblocks, int stride, int col0, int V, float* sh /* REC_T */) {
  const int Q = REC_T / V;
  const int v = threadIdx.x % V, q = threadIdx.x / V;
  float a = 0.f;
#pragma unroll 8                    // (the loads of eight records in flight; the additions stay in record order)
  for (int b = q; b < nblocks; b += Q) a += part[(long long)b * stride + col0 + v];
  sh[threadIdx.x] = a;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < V)
    for (int k = 0; k < Q; ++k) t += sh[k * V + threadIdx.x];
  __syncthreads();
  return t;
}
