#!/usr/bin/env python3
"""What the automatic mask generator's crop layers cost, and what the window writer replaces.
Kernel, GPU time between events, 64 low-res planes (256 x 256 f32, smooth blobs) per call, full-image planes of 1024 x 1024 and 1536 x 2048, one
entry per layer-1 window of amg_utils.generate_crop_boxes (boxes 1 .. 4):
  window        cvmi_amg_score_window: the crop's masks and the zeros around them in one pass over the u8 [64, PH, PW] planes
  composition   what it replaces: torch.zeros of the planes, cvmi_amg_score's mask mode into a crop-sized temporary, a slice copy into the window
  plane         cvmi_amg_score's mask mode at the plane's own size (the same bytes written, every pixel sampled), for scale
Algorithmic bytes: the window writes PH * PW per plane; the composition writes PH * PW + H * W, reads H * W and writes H * W again.
The generator (SAM 2.1 Hiera-L, synthetic weights, f16, thresholds = the medians of the first chunk as in tools/amg_bench.py), on a u8 image of
each size, host call to synchronised result: generate() with crop_n_layers = 0 and 1 (5 crops: one upload, five encodes, 5 x 1024 points).
Median of --rounds windows of --calls calls, the forms alternated round by round.  One JSON line per size, appended to profiles/amg_crop_bench.jsonl.
Usage: python tools/amg_crop_bench.py [--calls 5] [--rounds 5] [--sizes 1024x1024,1536x2048] [--planes 64] [--no-generate]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from amg_bench import alternate, event_ms, wall_ms  # noqa: E402

F0 = 256
LEVELS = (-1.0, 0.0, 1.0)


def low_planes(n, seed=0):
    """f32 [n, 256, 256] smooth logits: a coarse random field upsampled, so that masks are blobs with long borders."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(n, 1, 8, 8, generator=g)
    return (torch.nn.functional.interpolate(coarse, size=(F0, F0), mode="bicubic", align_corners=False)[:, 0] * 4).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1024x1024,1536x2048")
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amg_crop_bench needs the GPU: nothing is measured without one")
    from circuitvision_amd import _lib, amg_utils
    lib = _lib.load()
    sp = torch.cuda.current_stream().cuda_stream
    lo, mid, hi = LEVELS
    N = a.planes
    low = low_planes(N).cuda()
    stats = torch.empty(N, 8, dtype=torch.int32, device="cuda")
    gen = None if a.no_generate else _generator()
    for size in a.sizes.split(","):
        PH, PW = (int(v) for v in size.split("x"))
        boxes, _ = amg_utils.generate_crop_boxes((PH, PW), 1, 512 / 1500)
        planes = torch.empty(N, PH, PW, dtype=torch.uint8, device="cuda")
        variants = {"plane": (lambda: _lib.check(lib.cvmi_amg_score(low.data_ptr(), N, F0, F0, PH, PW, lo, mid, hi, stats.data_ptr(), planes.data_ptr(), sp),
                                                 "amg_score"), event_ms)}
        for k, (x0, y0, x1, y1) in enumerate(boxes[1:], 1):
            H, W = y1 - y0, x1 - x0
            tmp = torch.empty(N, H, W, dtype=torch.uint8, device="cuda")

            def window(H=H, W=W, x0=x0, y0=y0):
                _lib.check(lib.cvmi_amg_score_window(low.data_ptr(), N, F0, F0, H, W, lo, mid, hi, stats.data_ptr(), planes.data_ptr(), PH, PW, x0, y0, sp),
                           "amg_score_window")

            def composition(H=H, W=W, x0=x0, y0=y0, tmp=tmp):
                out = torch.zeros(N, PH, PW, dtype=torch.uint8, device="cuda")
                _lib.check(lib.cvmi_amg_score(low.data_ptr(), N, F0, F0, H, W, lo, mid, hi, stats.data_ptr(), tmp.data_ptr(), sp), "amg_score")
                out[:, y0:y0 + H, x0:x0 + W] = tmp
                return out
            window()
            want = composition()
            torch.cuda.synchronize()
            assert torch.equal(planes, want), "the window writer and the composition disagree"
            variants[f"window_{k}"] = (window, event_ms)
            variants[f"composition_{k}"] = (composition, event_ms)
        if gen is not None:
            img = _image(PH, PW)
            variants["generate_layers0"] = (lambda: gen.generate(img), wall_ms)
            variants["generate_layers1"] = (lambda: gen.generate(img, crop_n_layers=1), wall_ms)
        t = alternate(variants, a.calls, a.rounds)
        ms = {k: v["ms"] for k, v in t.items()}
        line = {"what": f"{N} planes 256 x 256 -> a layer-1 window of u8 planes {PH} x {PW}; kernels: GPU ms between events; generate: host call to synchronised "
                        "result; ms = median of the windows",
                "PH": PH, "PW": PW, "planes": N, "calls_per_window": a.calls, "rounds": a.rounds, "windows": boxes[1:], **t,
                "window_over_composition": {k: ms[f"window_{k}"] / ms[f"composition_{k}"] for k in range(1, len(boxes))},
                "window_GBps_written": {k: N * PH * PW / (ms[f"window_{k}"] * 1e-3) / 1e9 for k in range(1, len(boxes))},
                "window_beats_composition": all(ms[f"window_{k}"] < ms[f"composition_{k}"] for k in range(1, len(boxes)))}
        if gen is not None:
            line.update(generate_masks_layers0=len(gen.generate(img)), generate_masks_layers1=len(gen.generate(img, crop_n_layers=1)))
        for k, v in t.items():
            print(f"{PH}x{PW} {k:20s} {v['ms']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, {a.rounds} windows of {a.calls})")
        print(json.dumps(line))
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "amg_crop_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        del planes


def _image(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(3, (H + 63) // 64, (W + 63) // 64, generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :H, :W]
    return (coarse * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def _generator():
    """The model of tools/amg_bench.py; thresholds = the medians of the first chunk of the whole 1024 x 1024 image."""
    from circuitvision_amd import _lib
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    from circuitvision_amd.sam2 import HIERA_L, LORA_TARGETS_REFERENCE, SamSyntheticParams
    from circuitvision_amd.sam2_infer import SAM2Model
    lib = _lib.load()
    R, Pb, C = 1024, 64, 3
    model = SAM2Model(HIERA_L, R, dtype="f16", use_refinement=True).load_params(SamSyntheticParams(seed=0, lora_targets=LORA_TARGETS_REFERENCE))
    probe = Sam2AutomaticMaskGenerator(model)
    x = probe.transforms.forward_batch([_image(1024, 1024)])
    emb = model.encode_images(x)
    _, low, iou = model.infer_masks(emb, points=probe.points_in[:Pb].view(1, Pb, 1, 2), point_labels=torch.ones(1, Pb, 1, dtype=torch.int32), multimask_output=True,
                                    return_high_res=False)
    low, iou = low.view(Pb * C, F0, F0).contiguous(), iou.view(Pb * C).contiguous()
    lo, mid, hi = probe.levels
    stats = torch.empty(Pb * C, 8, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_amg_score(low.data_ptr(), Pb * C, F0, F0, 1024, 1024, lo, mid, hi, stats.data_ptr(), None, None), "amg_score")
    st = stats.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
    return Sam2AutomaticMaskGenerator(model, pred_iou_thresh=max(float(np.median(iou.cpu().numpy())), 0.0), stability_score_thresh=float(np.nanmedian(stab)))


if __name__ == "__main__":
    main()
