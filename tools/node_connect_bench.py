#!/usr/bin/env python3
"""GPU time of the contour x box stage (wires.node_connections' "connect" mark: cvmi_node_connect, between its two events) next to the
contours stage of the same run, on the 64 wire masks and the boxes of tools/node_stage_bench.py, plus the host time of the loop it
replaces (tests/node_ref.py node_tail, per image).  --boxes K adds K random component boxes per image to the two of node_stage_bench.
Usage: python tools/node_connect_bench.py [--images 64] [--reps 5] [--ref-images 4] [--boxes 0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import node_ref as R  # noqa: E402
import wire_ref as W  # noqa: E402
from circuitvision_amd import wires  # noqa: E402
from synth import circuit_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    shapes = [(600, int(rng.integers(760, 841))) for _ in range(a.images)]
    masks = [W.wire_mask(circuit_image(h, w, seed=100 + i)) for i, (h, w) in enumerate(shapes)]
    boxes = [[{"class": "resistor", "xmin": 100, "ymin": 100, "xmax": 160, "ymax": 140},
              {"class": "junction", "xmin": 300, "ymin": 300, "xmax": 320, "ymax": 320}] for _ in shapes]
    kinds = ["resistor", "capacitor.unpolarized", "voltage.dc", "diode", "inductor", "transistor.bjt"]
    for bb, (h, w) in zip(boxes, shapes):
        for k in range(a.boxes):
            x, y = int(rng.integers(0, w - 60)), int(rng.integers(0, h - 60))
            bb.append({"class": kinds[k % len(kinds)], "xmin": x, "ymin": y, "xmax": x + int(rng.integers(20, 60)), "ymax": y + int(rng.integers(20, 60)),
                       "persistent_uid": f"c{k}"})
    dev = [torch.from_numpy(m).cuda() for m in masks]
    res = wires.node_connections(dev, boxes)                          # warm-up: library load, allocator
    torch.cuda.synchronize()
    stages, walls = {}, []
    for _ in range(a.reps):
        ev = []
        t0 = time.perf_counter()
        wires.node_connections(dev, boxes, events=ev)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        marks = [(n, e) for n, e in ev if isinstance(e, torch.cuda.Event)]
        for (_, e0), (n, e1) in zip(marks, marks[1:]):
            stages.setdefault(n, []).append(e0.elapsed_time(e1))
    gpu = {n: float(np.median(v)) for n, v in stages.items()}
    t0 = time.perf_counter()
    for r in res[:a.ref_images]:                                      # the interpreted triple loop on the same contours and boxes
        R.node_tail(r["contours"], r["resized_bboxes"])
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(1, a.ref_images)
    out = {"images": a.images, "shape": "600 x 760..840", "visited_boxes_per_image": float(np.mean([sum(b["class"] not in wires.NON_COMPONENTS for b in bb) for bb in boxes])),
           "contours_total": int(sum(len(r["contours"]) for r in res)), "contour_points_total": int(sum(len(c["contour"]) for r in res for c in r["contours"])),
           "nodes_total": int(sum(len(r["nodes"]) for r in res)), "connect_gpu_ms": gpu["connect"], "connect_gpu_ms_per_image": gpu["connect"] / a.images,
           "contours_gpu_ms": gpu["contours"], "contours_gpu_ms_per_image": gpu["contours"] / a.images, "gpu_ms_per_stage": gpu,
           "wall_ms_per_call": float(np.median(walls)) * 1e3, "node_ref_loop_cpu_ms_per_image": ref_ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
