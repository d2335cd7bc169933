// Box losses on decoded boxes with their gradients, shared by fcos_loss.hip (loss_kernel<., true>) and gfl_loss.hip.
// Include after common.hpp, inside a translation unit compiled with floating-point contraction off.
#pragma once

// grad of max(a,b) w.r.t. a (ties split evenly, as torch.maximum) and of min(a,b) w.r.t. a
__device__ __forceinline__ float dmax_a(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float dmin_a(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// One positive location's box loss of kind DSL_BOX_IOU_LINEAR / DIOU / CIOU on the decoded boxes (prediction x, target X) and
// dl[k] = dloss / d(x1, y1, x2, y2), written as the reference's torch lines so that the subgradients are autograd's (max / min ties
// split 0.5, clamp(min=0) passes the gradient at 0).
__device__ __forceinline__ float box_loss_ext(int kind, float eps, float x1, float y1, float x2, float y2, float X1, float Y1,
                                              float X2, float Y2, float dl[4]) {
  const float a1 = (x2 - x1) * (y2 - y1), a2 = (X2 - X1) * (Y2 - Y1);
  const float ltx = fmaxf(x1, X1), lty = fmaxf(y1, Y1), rbx = fminf(x2, X2), rby = fminf(y2, Y2);
  const float w0 = rbx - ltx, h0 = rby - lty;
  const float iw = fmaxf(w0, 0.f), ih = fmaxf(h0, 0.f);
  const float ov = iw * ih;
  const float u0 = a1 + a2 - ov;
  const float cw = w0 >= 0.f ? 1.f : 0.f, chh = h0 >= 0.f ? 1.f : 0.f;
  const float dov[4] = {ih * (-dmax_a(x1, X1) * cw), iw * (-dmax_a(y1, Y1) * chh), ih * (dmin_a(x2, X2) * cw), iw * (dmin_a(y2, Y2) * chh)};
  const float da1[4] = {-(y2 - y1), -(x2 - x1), (y2 - y1), (x2 - x1)};
  if (kind == DSL_BOX_IOU_LINEAR) {
    // iou_loss.py:31-33: 1 - bbox_overlaps(...).clamp(min=eps); union = max(., eps) (iou2d_calculator.py:242-247), both eps 1e-6
    const float e6 = 1e-6f;
    const float U = fmaxf(u0, e6);
    const float ug = u0 > e6 ? 1.f : (u0 == e6 ? 0.5f : 0.f);
    const float iou = ov / U;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dU = (da1[k] - dov[k]) * ug;
      dl[k] = iou >= e6 ? -(dov[k] / U - ov * dU / (U * U)) : 0.f;      // no gradient where the clamp is active
    }
    return 1.f - fmaxf(iou, e6);
  }
  // diou_loss / ciou_loss (iou_loss.py:121-156, :177-218): union = ap + ag - overlap + eps (an add), c2 = cw^2 + ch^2 + eps
  const float U = u0 + eps;
  const float iou = ov / U;
  const float ew0 = fmaxf(x2, X2) - fminf(x1, X1), eh0 = fmaxf(y2, Y2) - fminf(y1, Y1);
  const float ew = fmaxf(ew0, 0.f), eh = fmaxf(eh0, 0.f);
  const float cew = ew0 >= 0.f ? 1.f : 0.f, ceh = eh0 >= 0.f ? 1.f : 0.f;
  const float c2 = ew * ew + eh * eh + eps;
  const float dc2[4] = {2.f * ew * (-dmin_a(x1, X1) * cew), 2.f * eh * (-dmin_a(y1, Y1) * ceh), 2.f * ew * (dmax_a(x2, X2) * cew),
                        2.f * eh * (dmax_a(y2, Y2) * ceh)};
  const float sx = (X1 + X2) - (x1 + x2), sy = (Y1 + Y2) - (y1 + y2);
  const float rho2 = sx * sx / 4.f + sy * sy / 4.f;
  const float drho[4] = {-sx / 2.f, -sy / 2.f, -sx / 2.f, -sy / 2.f};
  float pen = 0.f, kv = 0.f, ki = 0.f;
  float dv[4] = {0.f, 0.f, 0.f, 0.f};
  if (kind == DSL_BOX_CIOU) {
    const float w1 = x2 - x1, h1 = y2 - y1 + eps, w2 = X2 - X1, h2 = Y2 - Y1 + eps;
    const float r = w1 / h1;
    const float A = atanf(w2 / h2) - atanf(r);
    const float f = 0.40528473456935109f;          // 4 / pi^2
    const float v = f * (A * A);
    // DEVIATION: the reference's v^2 / (1 - iou + v) is 0/0 = NaN in fp32 when prediction and target coincide (1 - iou + v rounds to
    // 0); the penalty and its gradient are taken as 0 where v == 0, which is the fp64 value
    if (v != 0.f) {
      const float D = 1.f - iou + v;
      pen = v * v / D;
      ki = pen / D;                                 // d pen / d iou  = v^2 / D^2
      kv = 2.f * v / D - ki;                        // d pen / d v
      const float da = 2.f * f * A / (1.f + r * r); // -dv / d(w1 / h1)
      const float dvw = -da / h1, dvh = da * (w1 / (h1 * h1));
      dv[0] = -dvw; dv[1] = -dvh; dv[2] = dvw; dv[3] = dvh;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dU = da1[k] - dov[k];
    const float diou = dov[k] / U - ov * dU / (U * U);
    dl[k] = -diou + (drho[k] / c2 - rho2 * dc2[k] / (c2 * c2)) + (kv * dv[k] + ki * diou);
  }
  return 1.f - (iou - (rho2 / c2 + pen));
}

// GIoULoss (DSL_BOX_GIOU: 1 - giou, iou_loss.py:85-102 on bbox_overlaps mode 'giou', eps 1e-6 on union and enclosing area) and
// IoULoss (DSL_BOX_IOU_LOG: -log(clamp(iou, 1e-6)), iou_loss.py:14-36) in the same form: the loss and dl[k] = dloss / d(x1, y1, x2, y2).
// The arithmetic is the one loss_kernel carries inline for these two kinds.
__device__ __forceinline__ float box_loss_giou(bool iou_log, float x1, float y1, float x2, float y2, float X1, float Y1, float X2,
                                               float Y2, float dl[4]) {
  const float eps = 1e-6f;
  const float a1 = (x2 - x1) * (y2 - y1), a2 = (X2 - X1) * (Y2 - Y1);
  const float ltx = fmaxf(x1, X1), lty = fmaxf(y1, Y1), rbx = fminf(x2, X2), rby = fminf(y2, Y2);
  const float w0 = rbx - ltx, h0 = rby - lty;
  const float iw = fmaxf(w0, 0.f), ih = fmaxf(h0, 0.f);
  const float ov = iw * ih;
  const float u0 = a1 + a2 - ov;
  const float U = fmaxf(u0, eps);
  const float ew0 = fmaxf(x2, X2) - fminf(x1, X1), eh0 = fmaxf(y2, Y2) - fminf(y1, Y1);
  const float ew = fmaxf(ew0, 0.f), eh = fmaxf(eh0, 0.f);
  const float e0 = ew * eh;
  const float E = fmaxf(e0, eps);
  const float iou = ov / U;
  const float cw = w0 >= 0.f ? 1.f : 0.f, chh = h0 >= 0.f ? 1.f : 0.f;   // clamp(min=0) passes grad at 0
  const float dov[4] = {ih * (-dmax_a(x1, X1) * cw), iw * (-dmax_a(y1, Y1) * chh), ih * (dmin_a(x2, X2) * cw), iw * (dmin_a(y2, Y2) * chh)};
  const float da1[4] = {-(y2 - y1), -(x2 - x1), (y2 - y1), (x2 - x1)};
  const float ug = u0 > eps ? 1.f : (u0 == eps ? 0.5f : 0.f);
  const float cew = ew0 >= 0.f ? 1.f : 0.f, ceh = eh0 >= 0.f ? 1.f : 0.f;
  const float eg = e0 > eps ? 1.f : (e0 == eps ? 0.5f : 0.f);
  const float de[4] = {eh * (-dmin_a(x1, X1) * cew) * eg, ew * (-dmin_a(y1, Y1) * ceh) * eg, eh * (dmax_a(x2, X2) * cew) * eg,
                       ew * (dmax_a(y2, Y2) * ceh) * eg};
  const float iouc = fmaxf(iou, eps);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dU = (da1[k] - dov[k]) * ug;
    const float diou = dov[k] / U - ov * dU / (U * U);
    if (iou_log) dl[k] = iou >= eps ? -diou / iouc : 0.f;
    else dl[k] = -(diou + dU / E - U * de[k] / (E * E));
  }
  return iou_log ? -logf(iouc) : 1.f - (iou - (E - U) / E);
}
