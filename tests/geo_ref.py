"""The CPU model dsl_image_geo is held to: a step list (kind, a[, fill]) of include/dsl_hip.h's dsl_geo_step rendered FORWARD, one
step after the other, with numpy slices - the way the reference's transforms produce their images (RandomCrop / MinIoURandomCrop
slice, Expand fills a canvas and pastes, RandomShift pastes into zeros, CutOut assigns a rectangle)."""
import numpy as np

CROP, EXPAND, SHIFT, CUTOUT = 1, 2, 3, 4


def render(img, steps):
    """img: uint8 [h, w, 3]; returns the image after the last step."""
    img = np.ascontiguousarray(img)
    for st in steps:
        kind, a = st[0], [int(v) for v in st[1]]
        fill = np.asarray(st[2][:3] if len(st) > 2 else (0, 0, 0), np.uint8)
        h, w = img.shape[:2]
        if kind == CROP:
            x0, y0, cw, ch = a
            assert 0 <= x0 and 0 <= y0 and cw > 0 and ch > 0 and x0 + cw <= w and y0 + ch <= h, (st, img.shape)
            img = img[y0:y0 + ch, x0:x0 + cw].copy()
        elif kind == EXPAND:
            left, top, big_w, big_h = a
            assert 0 <= left and 0 <= top and left + w <= big_w and top + h <= big_h, (st, img.shape)
            out = np.empty((big_h, big_w, 3), np.uint8)
            out[:] = fill
            out[top:top + h, left:left + w] = img
            img = out
        elif kind == SHIFT:
            dx, dy = a[:2]
            assert abs(dx) < w and abs(dy) < h, (st, img.shape)
            out = np.zeros_like(img)
            nh, nw = h - abs(dy), w - abs(dx)
            out[max(0, dy):max(0, dy) + nh, max(0, dx):max(0, dx) + nw] = img[max(0, -dy):max(0, -dy) + nh, max(0, -dx):max(0, -dx) + nw]
            img = out
        elif kind == CUTOUT:
            x1, y1, x2, y2 = a
            assert 0 <= x1 <= x2 <= w and 0 <= y1 <= y2 <= h, (st, img.shape)
            img = img.copy()
            img[y1:y2, x1:x2] = fill
        else:
            raise ValueError(f'unknown step kind {kind}')
    return img


def render_into(img, steps, dst_h, dst_w):
    """The dst_h x dst_w rectangle dsl_image_geo writes: the rendered image, zero outside it."""
    out = render(img, steps)
    canvas = np.zeros((dst_h, dst_w, 3), np.uint8)
    canvas[:out.shape[0], :out.shape[1]] = out
    return canvas
