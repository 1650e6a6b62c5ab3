#!/usr/bin/env python3
"""GPU time of terminal reclassification (wires.reclassify_terminals) per sub-stage -- segment (cvmi_segment_circuit), contours
(cvmi_external_contours + its D2H), hits (cvmi_contour_hits) -- between CUDA events, on 64 synthetic circuit images of a crop-like size with
a few terminal boxes each, next to the host time of the restatement it replaces (tests/segment_ref.py reclassify, per image), and the
segment kernel's distance from its byte floor: 3 B read + 1 B written per pixel at --hbm-gbs.
Usage: python tools/terminal_reclass_bench.py [--images 64] [--reps 5] [--ref-images 4] [--terminals 4] [--hbm-gbs 8000]"""
import argparse
import json
import os
import sys
import time
from copy import deepcopy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import segment_ref as S  # noqa: E402
from circuitvision_amd import wires  # noqa: E402
from synth import circuit_image  # noqa: E402

NAMES = {0: "resistor", 1: "terminal", 2: "voltage.dc"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=4)
    ap.add_argument("--terminals", type=int, default=4)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate the byte floor is taken at (MI355X: 8 TB/s peak)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    shapes = [(600, int(rng.integers(760, 841))) for _ in range(a.images)]
    images = [circuit_image(h, w, seed=100 + i) for i, (h, w) in enumerate(shapes)]
    boxes = []
    for h, w in shapes:
        bb = [{"class": "resistor", "xmin": 100, "ymin": 100, "xmax": 160, "ymax": 140}]
        for k in range(a.terminals):
            x, y = int(rng.integers(0, w - 60)), int(rng.integers(0, h - 60))
            bb.append({"class": "terminal", "_yolo_class_id_temp": 1, "xmin": x, "ymin": y, "xmax": x + int(rng.integers(20, 60)), "ymax": y + int(rng.integers(20, 60)),
                       "persistent_uid": f"t{k}"})
        boxes.append(bb)
    dev = [torch.from_numpy(im).cuda() for im in images]
    counts = wires.reclassify_terminals(dev, deepcopy(boxes), NAMES)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    stages, walls = {}, []
    for _ in range(a.reps):
        ev = []
        bb = deepcopy(boxes)
        t0 = time.perf_counter()
        wires.reclassify_terminals(dev, bb, NAMES, events=ev)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        for (_, e0), (n, e1) in zip(ev, ev[1:]):
            stages.setdefault(n, []).append(e0.elapsed_time(e1))
    gpu = {n: float(np.median(v)) for n, v in stages.items()}
    # the segment kernel alone, on the packed batch (no packing copy, no rectangles upload in the timed span)
    src, planes = wires._rgb_planes(dev, None)
    rects = [wires.emptying_rects(bb, h, w) for bb, (h, w) in zip(boxes, shapes)]
    seg = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        wires.segment_packed(src, planes, rects, 0)
        e1.record()
        torch.cuda.synchronize()
        seg.append(e0.elapsed_time(e1))
    seg_ms = float(np.median(seg[1:]))
    pixels = sum(h * w for h, w in shapes)
    floor_ms = pixels * 4 / (a.hbm_gbs * 1e9) * 1e3
    t0 = time.perf_counter()
    for im, bb in list(zip(images, deepcopy(boxes)))[:a.ref_images]:
        S.reclassify(im, bb, NAMES, 0)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(1, a.ref_images)
    out = {"images": a.images, "shape": "600 x 760..840", "terminals_per_image": a.terminals, "pixels_total": pixels,
           "reclassified_total": int(sum(v >= 2 for c in counts for v in c.values())), "gpu_ms_per_stage": gpu,
           "segment_gpu_ms": gpu["segment"], "contours_gpu_ms": gpu["contours"], "hits_gpu_ms": gpu["hits"],
           "gpu_ms_per_image": sum(gpu.values()) / a.images, "segment_call_ms (wrapper: rectangles H2D + memset + 2 launches)": seg_ms,
           "segment_byte_floor_ms": floor_ms, "segment_fraction_of_byte_floor": floor_ms / seg_ms, "segment_gb_per_s": pixels * 4 / (seg_ms * 1e-3) / 1e9,
           "wall_ms_per_call": float(np.median(walls)) * 1e3, "segment_ref_cpu_ms_per_image": ref_ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
