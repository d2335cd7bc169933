"""Time dsl_image_geo on full-size canvases against dsl_image_prep_u8 without resampling, which moves the same bytes (one uint8 BGR
read and one write per pixel).  A report, not a gate (DESIGN.md section 3.6 holds the figures).

  python tools/bench_geo.py [--n 8] [--h 800] [--w 1344] [--launches 50] [--alternations 3]

Variants: a 1-step crop, a 4-step chain (crop, expand, shift, cutout) and a 32-step CutOut list, each writing the whole n x h x w
canvas.  Every alternation times each variant once (--launches back-to-back launches between two device events, after a warm-up);
one JSON line per variant with the per-alternation microseconds per launch, their median, and the median's bytes per second
(2 * n * h * w * 3 bytes per launch: what the pass has to read and write)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--h', type=int, default=800)
    ap.add_argument('--w', type=int, default=1344)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--alternations', type=int, default=3)
    args = ap.parse_args()
    from dsl_amd import _lib as L
    assert torch.cuda.is_available(), 'bench_geo needs the GPU'
    n, h, w = args.n, args.h, args.w
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    rng = np.random.RandomState(0)
    lists = {
        'geo_crop_1step': [(L.GEO_CROP, (8, 8, w - 16, h - 16))],
        'geo_chain_4step': [(L.GEO_CROP, (w // 12, h // 16, w - w // 6, h - h // 8)), (L.GEO_EXPAND, (w // 24, h // 32, w, h), (123, 116, 103)),
                            (L.GEO_SHIFT, (5, -7)), (L.GEO_CUTOUT, (w // 4, h // 4, w // 4 + 200, h // 4 + 200), (0, 0, 0))],
        'geo_cutout_32step': [(L.GEO_CUTOUT, (x, y, x + 64, y + 64), (114, 114, 114))
                              for x, y in zip(rng.randint(0, w - 64, 32), rng.randint(0, h - 64, 32))],
    }
    runs, keep = {}, []
    for name, steps in lists.items():
        its = (L.GeoItem * n)()
        for i in range(n):
            L.geo_fill_item(its[i], steps, src[i].data_ptr(), h, w, w, dst[i].data_ptr(), h, w, w)
        tab = torch.frombuffer(bytearray(bytes(its)), dtype=torch.uint8).cuda()
        keep += [its, tab]
        runs[name] = lambda its=its, tab=tab: L.check(
            L.lib.dsl_image_geo(ctypes.cast(its, ctypes.c_void_p), L.ptr(tab), n, h, w, L.stream_ptr()), 'dsl_image_geo')
    items = (L.ImagePrepItem * n)()
    for i in range(n):
        items[i].src, items[i].src_h, items[i].src_w, items[i].new_h, items[i].new_w = src[i].data_ptr(), h, w, h, w
    ptab = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    runs['prep_u8_no_resample'] = lambda: L.check(L.lib.dsl_image_prep_u8(L.ptr(ptab), n, L.ptr(dst), h, w, L.stream_ptr()), 'dsl_image_prep_u8')

    def timed(f):
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    series = {k: [] for k in runs}
    for _ in range(args.alternations):
        for k, f in runs.items():
            series[k].append(timed(f))
    nbytes = 2 * n * h * w * 3
    for k, v in series.items():
        med = statistics.median(v)
        print(json.dumps(dict(variant=k, n=n, h=h, w=w, us_per_launch=[round(x, 2) for x in v], median_us=round(med, 2),
                              gbytes_per_s=round(nbytes / med / 1e3, 1))), flush=True)


if __name__ == '__main__':
    main()
