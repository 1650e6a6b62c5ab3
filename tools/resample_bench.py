#!/usr/bin/env python3
"""Time of the resampling launches at the pipeline's sizes (tests/resample_bits_cases.py WORKLOAD: 16 images of 768 x 1024, the segmenter at
1024): the f16 transform with swap_rb through `batch` and `rects_dev`, the mask return through cvmi_mask_postprocess, _sizes and _rects_dev.
Per launch: device events around --launches back-to-back calls after a warm-up, in microseconds per call.  One JSON line.  The library is the
one CVMI_LIB_PATH names (default: the tree's), so an A/B of two builds is this tool run alternately, one process per run.
Usage: python tools/resample_bench.py [--launches 50] [--warmup 5] [--label NAME]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from circuitvision_amd import _lib  # noqa: E402
from resample_bits_cases import WORKLOAD, workload_calls, workload_operands  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU: nothing is measured without one")
    lib = _lib.load()
    calls, _outs, _sizes = workload_calls(lib, *workload_operands())
    line = {"tool": "resample_bench", "label": a.label, "lib": os.path.basename(_lib.LIB_PATH), "workload": WORKLOAD, "launches": a.launches, "us_per_call": {}}
    for name, call in calls.items():
        for _ in range(a.warmup):
            assert call() == 0, lib.cvmi_last_error().decode()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            call()
        t1.record()
        t1.synchronize()
        line["us_per_call"][name] = round(t0.elapsed_time(t1) * 1e3 / a.launches, 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
