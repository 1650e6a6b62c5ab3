#!/usr/bin/env python3
"""Wall time of `CircuitPipeline(crop=True).run_batch` with the glue between detector and segmenter on the host (device_glue=False) and on
the device (device_glue=True), in the same process, on 64 and on 8 images of 900 x 1200 (a batch, and one rank's share of it): the median of
--reps runs per setting after a warm-up run, and the per-phase `timings` of both settings (per run, ms).  Models: YOLO11-n with calibrated
synthetic weights under a label map that gives real crop windows, and the mini SAM 2 of the tests (--seg l: SAM 2.1-L with synthetic
weights) -- the glue's share of the wall time is what is measured, not the models.
Usage: python tools/device_glue_bench.py [--images 64 8] [--reps 5] [--seg mini|l] [--seg-batch 16] [--dtype f16]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", choices=("mini", "l"), default="mini")
    ap.add_argument("--seg-batch", type=int, default=16)
    ap.add_argument("--dtype", default="f16")
    a = ap.parse_args()
    H, W = 900, 1200
    images = [circuit_image(H, W, seed=300 + i) for i in range(max(a.images))]
    x = torch.cat([torch.from_numpy(opre.yolo_preprocess(im)) for im in images[:4]])
    yp = calibrated_yolo_params("n", 62, 4, x)
    with tempfile.TemporaryDirectory() as tmp:
        det = YOLO(save_converted_yolo(os.path.join(tmp, "y.pt"), yp, "n", 62), dtype=a.dtype, graph_lanes=0)
    det.names = det.model.names = dict(NAMES)
    if a.seg == "mini":
        from test_oracle_sam2_cpu import MINI, mini_targets
        R = 256
        seg = SAM2Model(MINI, R, dtype=a.dtype, use_refinement=True).load_params(SamSyntheticParams(seed=8, lora_targets=mini_targets(), std=0.05))
    else:
        from circuitvision_amd.sam2 import HIERA_L
        R = 1024
        seg = SAM2Model(HIERA_L, R, dtype=a.dtype, use_refinement=True).load_params(SamSyntheticParams(seed=8, std=0.02))
    tr = SAM2Transforms(resolution=R, mask_threshold=0, max_hole_area=0, max_sprinkle_area=0)
    for n in a.images:
        batch = images[:n]
        line = {"images": n, "shape": f"{H} x {W}", "seg": a.seg, "seg_batch": a.seg_batch, "dtype": a.dtype, "reps": a.reps}
        windows = None
        for on in (False, True):
            pipe = CircuitPipeline(det, seg, tr, crop=True, crop_padding=80, seg_batch=a.seg_batch, device_glue=on)
            res = pipe.run_batch(batch, "learned")                      # warm-up: plans, graphs, allocator
            torch.cuda.synchronize()
            pipe.timings.clear()
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = pipe.run_batch(batch, "learned")
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            key = "device_glue" if on else "host_glue"
            line[key + "_ms"] = float(np.median(walls)) * 1e3
            line[key + "_ms_per_image"] = line[key + "_ms"] / n
            line[key + "_timings_ms"] = {k: v * 1e3 / a.reps for k, v in pipe.timings.items()}
            wins = [r["window"] for _, r in res]
            assert windows is None or wins == windows, "both settings must decide the same windows"
            windows = wins
        line["real_windows"] = sum(w is not None and (w[2] - w[0], w[3] - w[1]) != (W, H) for w in windows)
        line["device_over_host"] = line["device_glue_ms"] / line["host_glue_ms"]
        print(json.dumps(line))


if __name__ == "__main__":
    main()
