#!/usr/bin/env python3
"""Time of `cvmi_mask_prompt_embed` (csrc/mask_prompt.hip) at the production geometry -- B = 16 images, 32 prompts each, a 64 x 64 embedding, the
16-bit copy on -- next to the pair of launches it replaces on the same buffers, `cvmi_repeat_images` + the `cvmi_cast` of the image stream,
and of `infer_masks` at 16 x 32 box prompts with and without `mask_input` (SAM 2.1 Hiera-L, synthetic weights, graph replay).
Device events around windows of --launches launches, every shape warmed first, the variants alternating in the same process over --rounds
rounds (other work shares the machine); the median window is reported.  Bytes are what the algorithm has to move, computed from the shapes;
the fraction is of 8 TB/s.  `repeat_images` alone (the f32 stores of the same stream) stands beside them as the store-rate yardstick.
Usage: python tools/mask_prompt_bench.py [--B 16] [--P 32] [--fs 64] [--launches 100] [--rounds 3] [--model-calls 10] [--no-model]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circuitvision_amd import _lib  # noqa: E402
from circuitvision_amd._lib import F16, F32  # noqa: E402

PEAK_BPS = 8e12


def window_ms(fn, launches):
    """Milliseconds per call over one window of `launches` back-to-back calls (device events around the window)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def alternate(variants, launches, rounds):
    """{name: median ms per call} with the variants' windows interleaved round by round."""
    for fn in variants.values():                                # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            runs[k].append(window_ms(fn, launches))
    return {k: float(np.median(v)) for k, v in runs.items()}, runs


def rate(bytes_, ms):
    bps = bytes_ / (ms * 1e-3)
    return {"ms": ms, "bytes": bytes_, "TBps": bps / 1e12, "of_8TBps": bps / PEAK_BPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--P", type=int, default=32)
    ap.add_argument("--fs", type=int, default=64)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model-calls", type=int, default=10)
    ap.add_argument("--no-model", action="store_true", help="the kernels only: skip the two infer_masks timings (Hiera-L weights take a while to pack)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_prompt_bench needs the GPU: nothing is measured without one")
    lib = _lib.load()
    B, P, fs = a.B, a.P, a.fs
    n, pix = B * P, fs * fs
    g = torch.Generator().manual_seed(0)
    mask = (6 * torch.randn(n, 4 * fs, 4 * fs, generator=g)).cuda()
    emb = torch.randn(B, pix, 256, generator=g).cuda()
    prm = (0.05 * torch.randn(4684, generator=g)).cuda()
    keys = torch.empty(n, pix, 256, device="cuda")
    kn = torch.empty(n, pix, 256, device="cuda", dtype=torch.float16)

    def embed():
        _lib.check(lib.cvmi_mask_prompt_embed(mask.data_ptr(), emb.data_ptr(), prm.data_ptr(), keys.data_ptr(), kn.data_ptr(), F16, B, P, fs, None), "mask_prompt_embed")

    def repeat():
        _lib.check(lib.cvmi_repeat_images(emb.data_ptr(), keys.data_ptr(), pix * 256 * 4, B, P, None), "repeat_images")

    def repeat_cast():
        repeat()
        _lib.check(lib.cvmi_cast(keys.data_ptr(), 256, F32, kn.data_ptr(), 256, F16, n * pix, 256, None), "cast")

    k4, k2 = n * pix * 256 * 4, n * pix * 256 * 2
    bytes_ = {"mask_prompt_embed": mask.numel() * 4 + emb.numel() * 4 + k4 + k2,          # read the masks and emb; write both copies of the stream
              "repeat_images+cast": emb.numel() * 4 + k4 + k4 + k2,                        # read emb, write f32; read f32, write the 16-bit copy
              "repeat_images": emb.numel() * 4 + k4}
    ms, runs = alternate({"mask_prompt_embed": embed, "repeat_images+cast": repeat_cast, "repeat_images": repeat}, a.launches, a.rounds)
    line = {"B": B, "P": P, "fs": fs, "copy": "f16", "launches_per_window": a.launches, "rounds": a.rounds,
            "timed_launches_per_variant": a.launches * a.rounds}
    for k in ms:
        line[k] = rate(bytes_[k], ms[k])
        line[k]["ms_windows"] = runs[k]
    line["embed_over_pair_time"] = ms["mask_prompt_embed"] / ms["repeat_images+cast"]
    if not a.no_model:
        from circuitvision_amd.sam2 import HIERA_L, LORA_TARGETS_REFERENCE, SamSyntheticParams
        from circuitvision_amd.sam2_infer import SAM2Model
        R = 16 * fs
        model = SAM2Model(HIERA_L, R, dtype="f16", use_refinement=True).load_params(SamSyntheticParams(seed=0, lora_targets=LORA_TARGETS_REFERENCE))
        x = torch.randn(B, 3, R, R, generator=g).cuda()
        side = (24 + 176 * torch.rand(B, P, 2, generator=g)) * (R / 1024)
        xy = torch.rand(B, P, 2, generator=g) * (R - side)
        boxes = torch.cat((xy, xy + side), -1)
        _, lo, _ = model.infer_masks(x, boxes, return_high_res=False)                     # the second pass feeds the first pass's logits back
        mk = lo.clone()
        t, r = alternate({"infer_masks": lambda: model.infer_masks(x, boxes, return_high_res=False),
                          "infer_masks+mask_input": lambda: model.infer_masks(x, boxes, return_high_res=False, mask_input=mk)}, a.model_calls, a.rounds)
        line["infer_masks_ms"], line["infer_masks_mask_input_ms"] = t["infer_masks"], t["infer_masks+mask_input"]
        line["infer_masks_ms_windows"], line["infer_masks_mask_input_ms_windows"] = r["infer_masks"], r["infer_masks+mask_input"]
        line["infer_masks_what"] = f"SAM 2.1 Hiera-L {R}^2 f16, {B} x {P} box prompts, return_high_res=False, host call to synchronised result"
    print(json.dumps(line))


if __name__ == "__main__":
    main()
