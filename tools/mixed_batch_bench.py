#!/usr/bin/env python3
"""Wall time of `CircuitPipeline(crop=True).run_batch` on 64 uploads of 16 distinct sizes with the images grouped by size (mixed_batch=False: a
detector batch, a staging buffer and a plan per size -- the path of the commit before) and handed to the detector as one mixed batch
(mixed_batch=True: one packed upload, a ragged letterbox launch and a square plan per chunk), in the same process.  Reported per setting: the
FIRST call (plan creation, graph capture, staging allocation show there), the median of --reps calls after it, the per-phase `timings` of those
calls (per call, ms) and the number of detector plans and staging buffers the detector holds afterwards.  The two settings do not compute the
same thing (a rectangle per size against the imgsz x imgsz square for every image: ultralytics' rule for a mixed list), so detections differ and
only times are compared.  Models: YOLO11-n with calibrated synthetic weights under a label map that gives real crop windows, and the mini SAM 2 of
the tests (--seg l: SAM 2.1-L with synthetic weights).
Usage: timeout 600 python tools/mixed_batch_bench.py [--images 64] [--sizes 16] [--reps 5] [--seg mini|l] [--seg-batch 16] [--dtype f16]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circuitvision_amd.detector import YOLO  # noqa: E402
from circuitvision_amd.pipeline import CircuitPipeline  # noqa: E402
from circuitvision_amd.sam2 import SamSyntheticParams  # noqa: E402
from circuitvision_amd.sam2_infer import SAM2Model, SAM2Transforms  # noqa: E402
from helpers import save_converted_yolo  # noqa: E402
from oracle import preprocess as opre  # noqa: E402
from synth import calibrated_yolo_params, circuit_image  # noqa: E402

NAMES = {i: (f"component{i}" if i % 10 == 0 else "junction" if i % 10 == 1 else "text" if i % 10 == 2 else "explanatory") for i in range(62)}


def upload_sizes(n):
    """n distinct (h, w): phone and scanner aspect ratios, landscape and portrait, 600 .. 1600 pixels a side."""
    base = [(900, 1200), (1200, 900), (768, 1024), (1024, 768), (720, 1280), (1280, 720), (1080, 1080), (600, 800), (800, 600), (1000, 1500),
            (1500, 1000), (960, 1280), (1280, 960), (640, 1600), (1100, 850), (850, 1100)]
    out = list(base[:n])
    k = 0
    while len(out) < n:
        out.append((700 + 37 * k, 1000 + 53 * k))
        k += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--sizes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", choices=("mini", "l"), default="mini")
    ap.add_argument("--seg-batch", type=int, default=16)
    ap.add_argument("--dtype", default="f16")
    a = ap.parse_args()
    sizes = upload_sizes(a.sizes)
    images = [circuit_image(*sizes[(i * 7) % len(sizes)], seed=300 + i) for i in range(a.images)]           # sizes interleaved, as uploads arrive
    x = torch.cat([torch.from_numpy(opre.yolo_preprocess(circuit_image(900, 1200, seed=300 + i))) for i in range(4)])
    yp = calibrated_yolo_params("n", 62, 4, x)
    if a.seg == "mini":
        from test_oracle_sam2_cpu import MINI, mini_targets
        R = 256
        seg = SAM2Model(MINI, R, dtype=a.dtype, use_refinement=True).load_params(SamSyntheticParams(seed=8, lora_targets=mini_targets(), std=0.05))
    else:
        from circuitvision_amd.sam2 import HIERA_L
        R = 1024
        seg = SAM2Model(HIERA_L, R, dtype=a.dtype, use_refinement=True).load_params(SamSyntheticParams(seed=8, std=0.02))
    tr = SAM2Transforms(resolution=R, mask_threshold=0, max_hole_area=0, max_sprinkle_area=0)
    line = {"images": a.images, "distinct_sizes": len({im.shape[:2] for im in images}), "seg": a.seg, "seg_batch": a.seg_batch, "dtype": a.dtype, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp:
        path = save_converted_yolo(os.path.join(tmp, "y.pt"), yp, "n", 62)
        for mixed in (False, True):
            det = YOLO(path, dtype=a.dtype, graph_lanes=0)              # a detector of its own per setting: plans and staging start empty
            det.names = det.model.names = dict(NAMES)
            pipe = CircuitPipeline(det, seg, tr, crop=True, crop_padding=80, seg_batch=a.seg_batch, mixed_batch=mixed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pipe.run_batch(images, "learned")                     # the first call: plans, graphs, staging, allocator
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            pipe.timings.clear()
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = pipe.run_batch(images, "learned")
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            key = "mixed" if mixed else "grouped"
            line[key + "_first_call_ms"] = first * 1e3
            line[key + "_ms"] = float(np.median(walls)) * 1e3
            line[key + "_ms_per_image"] = line[key + "_ms"] / a.images
            line[key + "_detector_plans"] = len(det._plans)
            line[key + "_staging_buffers"] = len(det._staging) + (det._flat_staging[0] is not None)
            line[key + "_timings_ms"] = {k: v * 1e3 / a.reps for k, v in pipe.timings.items()}
            line[key + "_boxes"] = sum(len(r["bboxes"]) for _, r in res)
            line[key + "_real_windows"] = sum(r["window"] is not None for _, r in res)
    line["mixed_over_grouped"] = line["mixed_ms"] / line["grouped_ms"]
    line["mixed_over_grouped_first_call"] = line["mixed_first_call_ms"] / line["grouped_first_call_ms"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
