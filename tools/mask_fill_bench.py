#!/usr/bin/env python3
"""Time of `SAM2Transforms.postprocess_to_mask_async` on 16 x 1 x 1024 x 1024 mask logits that have real small components, with both areas 0
(the resize-only path) and with both areas 8 (hole / sprinkle removal in front of the resize, csrc/mask_cc.hip), alternating in the same
process: the median of --reps calls per setting after a warm-up, by device events.  Then the labelling's four launches one by one (kernel
durations from torch's profiler, per call) with the bytes the algorithm moves per pixel beside each.
The logits: smooth blobs (a low-pass filtered noise field) plus isolated specks and pinholes of 1 .. 12 pixels, seeded.
Usage: python tools/mask_fill_bench.py [--planes 16] [--size 1024] [--out 900 1200] [--reps 20] [--areas 8]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circuitvision_amd.sam2_infer import SAM2Transforms  # noqa: E402

# bytes per pixel each launch has to move (f32 logits, i32 roots and areas); the seam pass touches only the tiles' first rows and columns
BYTES_PER_PIXEL = {"mask_cc_tile_kernel": 4 + 4 + 4,        # read x; write the tile-local root and the zeroed area slot
                   "mask_cc_seam_kernel": 0,
                   "mask_cc_flatten_kernel": 4 + 4,         # read the root slot; write the final root (+ one atomic per tile and root)
                   "mask_cc_apply_kernel": 4 + 4 + 4 + 4}   # read x, root, the root's area; write y


def logits(planes, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(planes, 1, size // 32, size // 32, generator=g)
    x = torch.nn.functional.interpolate(low, size=(size, size), mode="bicubic", align_corners=False) * 4
    flip = torch.zeros(planes, 1, size, size)
    n = size * size // 2048                                  # specks / pinholes per plane
    for p in range(planes):
        ys, xs = torch.randint(0, size - 4, (n,), generator=g), torch.randint(0, size - 4, (n,), generator=g)
        hs, ws = torch.randint(1, 4, (n,), generator=g), torch.randint(1, 5, (n,), generator=g)
        for y0, x0, hh, ww in zip(ys.tolist(), xs.tolist(), hs.tolist(), ws.tolist()):
            flip[p, 0, y0:y0 + hh, x0:x0 + ww] = 1
    return torch.where(flip > 0, -x, x).contiguous()


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", type=int, nargs=2, default=[900, 1200])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--areas", type=float, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_fill_bench needs the GPU: nothing is measured without one")
    m = logits(a.planes, a.size).cuda()
    hw = tuple(a.out)
    tr0, tr8 = SAM2Transforms(a.size, 0.0, 0, 0), SAM2Transforms(a.size, 0.0, a.areas, a.areas)
    u0, _ = tr0.postprocess_to_mask_async(m, hw)              # warm-up: code objects, allocator
    u8, _ = tr8.postprocess_to_mask_async(m, hw)
    tr8.fill_small_regions(m)
    torch.cuda.synchronize()
    line = {"planes": a.planes, "size": a.size, "out": list(hw), "areas": a.areas, "reps": a.reps,
            "mask_pixels_changed_by_the_fill": int((u0 != u8).sum())}
    t0, t8, tf = [], [], []
    for _ in range(3):                                        # alternate the settings: other work shares the machine
        t0.append(median_ms(lambda: tr0.postprocess_to_mask_async(m, hw), a.reps))
        t8.append(median_ms(lambda: tr8.postprocess_to_mask_async(m, hw), a.reps))
        tf.append(median_ms(lambda: tr8.fill_small_regions(m), a.reps))
    line["areas_0_ms"], line["areas_on_ms"], line["fill_alone_ms"] = float(np.median(t0)), float(np.median(t8)), float(np.median(tf))
    line["areas_0_ms_runs"], line["areas_on_ms_runs"] = t0, t8
    pixels = a.planes * a.size * a.size
    line["fill_bytes_per_pixel"] = sum(BYTES_PER_PIXEL.values())
    line["fill_alone_GBps"] = pixels * line["fill_bytes_per_pixel"] / (line["fill_alone_ms"] * 1e-3) / 1e9
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(a.reps):
            tr8.fill_small_regions(m)
        torch.cuda.synchronize()
    per = {}
    for ev in prof.key_averages():
        for name, bpp in BYTES_PER_PIXEL.items():
            dur = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if name in ev.key and dur:
                us = dur / max(1, ev.count)
                per[name] = {"us_per_call": us, "bytes_per_pixel": bpp, "GBps": pixels * bpp / (us * 1e-6) / 1e9}
    line["sub_launches"] = per if per else "not measured (the profiler reported no kernel)"
    print(json.dumps(line))


if __name__ == "__main__":
    main()
