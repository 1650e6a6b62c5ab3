#!/usr/bin/env python3
"""GPU time of the node-analysis front end (wires.node_contours) per sub-stage on 64 wire masks of ~600 x 800 from synth.circuit_image,
timed with torch.cuda events, plus the longest traced border and, for context, the CPU time of the numpy restatement (tests/wire_ref.py;
cv2 is not available to compare with).  Usage: python tools/node_stage_bench.py [--images 64] [--reps 5] [--ref-images 4]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wire_ref as W  # noqa: E402
from circuitvision_amd import wires  # noqa: E402
from synth import circuit_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=4)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    shapes = [(600, int(rng.integers(760, 841))) for _ in range(a.images)]
    masks = [W.wire_mask(circuit_image(h, w, seed=100 + i)) for i, (h, w) in enumerate(shapes)]
    boxes = [[{"class": "resistor", "xmin": 100, "ymin": 100, "xmax": 160, "ymax": 140},
              {"class": "junction", "xmin": 300, "ymin": 300, "xmax": 320, "ymax": 320}] for _ in shapes]
    dev = [torch.from_numpy(m).cuda() for m in masks]
    wires.node_contours(dev, boxes)                                   # warm-up: library load, allocator
    torch.cuda.synchronize()
    stages, walls, longest = {}, [], 0
    for _ in range(a.reps):
        ev = []
        t0 = time.perf_counter()
        wires.node_contours(dev, boxes, events=ev)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        marks = [(n, e) for n, e in ev if isinstance(e, torch.cuda.Event)]
        for (_, e0), (n, e1) in zip(marks, marks[1:]):
            stages.setdefault(n, []).append(e0.elapsed_time(e1))
        longest = max(longest, dict(ev)["longest_border"])
    gpu = {n: float(np.median(v)) for n, v in stages.items()}
    # contours = labelling + tracing + the D2H of the points; its event closes after the host has read them back
    t0 = time.perf_counter()
    for m, bb in zip(masks[:a.ref_images], boxes):
        W.node_contours(m, bb)
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(1, a.ref_images)
    out = {"images": a.images, "shape": "600 x 760..840", "gpu_ms_per_stage": gpu, "gpu_ms_total": sum(gpu.values()),
           "gpu_ms_per_image": sum(gpu.values()) / a.images, "wall_ms_per_call": float(np.median(walls)) * 1e3,
           "longest_border_steps": int(longest), "wire_ref_cpu_ms_per_image": ref_ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
