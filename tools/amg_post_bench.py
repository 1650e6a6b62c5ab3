#!/usr/bin/env python3
"""What the automatic mask generator's two per-call options cost, and what they replace.
Kernels, on 64 u8 planes at 1024 x 1024 and at 1536 x 2048 (smooth blobs plus specks and pinholes of 1 .. 12 pixels: the recipe of
tools/mask_fill_bench.py, thresholded), GPU time between events:
  rle               cvmi_mask_rle with a capacity that fits                     algorithmic bytes per pixel: 1 (the mask, read once) + 2 / 8 (the bit-plane
                                                                                written and read twice) + 4 per run
  remove_small      cvmi_mask_remove_small, phases = 3, min_area = 8              two labellings (9 + 8 each: the u8 read, root and area slot written, root
                                                                                read and rewritten) + two apply passes (1 + 4 + 4 gathered, + 1 where written)
  ... and per launch from torch's profiler (a run of its own), beside the tile / seam / flatten rates tools/mask_fill_bench.py reports for f32 logits.
The composition they replace, wall time: D2H of the planes, then the numpy / scipy loop of tests/amg_post_ref.py per plane (`--ref-planes` of
them, scaled to 64).
The generator (SAM 2.1 Hiera-L, synthetic weights, f16, thresholds = the medians of the first chunk as in tools/amg_bench.py), host call to
synchronised result: generate() as it is, with output_mode="uncompressed_rle", with min_mask_region_area, and with both -- once with the default
box_nms_thresh (the synthetic weights' candidates are near-duplicates: NMS leaves ONE mask, so these forms show the options' fixed cost), and once as
`many`: pred_iou_thresh at the 90th percentile and box_nms_thresh = 1, so that a few hundred masks come back, as a trained model's do.
Median of --rounds windows of --calls calls, the forms alternated round by round.  One JSON line per size, appended to profiles/amg_post_bench.jsonl.
Usage: python tools/amg_post_bench.py [--calls 5] [--rounds 5] [--sizes 1024x1024,1536x2048] [--planes 64] [--ref-planes 2] [--no-generate]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from amg_bench import alternate, event_ms, wall_ms  # noqa: E402

MIN_AREA = 8
KERNELS = ("rle_bits_kernel", "rle_reduce_kernel", "rle_scan_kernel", "rle_emit_kernel", "mask_cc_tile_kernel", "mask_cc_seam_kernel", "mask_cc_flatten_kernel",
           "remove_best_kernel", "remove_apply_kernel")
# bytes per pixel each launch has to move (u8 planes, i32 roots and areas, 1 bit per pixel in the transposed bit-plane)
BYTES_PER_PIXEL = {"rle_bits_kernel": 1 + 1 / 8, "rle_reduce_kernel": 1 / 8, "rle_emit_kernel": 1 / 8, "mask_cc_tile_kernel": 1 + 4 + 4, "mask_cc_flatten_kernel": 4 + 4,
                   "remove_best_kernel": 4, "remove_apply_kernel": 1 + 4 + 4}


def planes_u8(n, H, W, seed=0):
    """The logits of tools/mask_fill_bench.py at H x W, thresholded at 0 -> u8 {0, 255} [n, H, W]."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, 1, H // 32, W // 32, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False) * 4
    flip = torch.zeros(n, 1, H, W)
    k = H * W // 2048
    for p in range(n):
        ys, xs = torch.randint(0, H - 4, (k,), generator=g), torch.randint(0, W - 4, (k,), generator=g)
        hs, ws = torch.randint(1, 4, (k,), generator=g), torch.randint(1, 5, (k,), generator=g)
        for y0, x0, hh, ww in zip(ys.tolist(), xs.tolist(), hs.tolist(), ws.tolist()):
            flip[p, 0, y0:y0 + hh, x0:x0 + ww] = 1
    return ((torch.where(flip > 0, -x, x) > 0)[:, 0].to(torch.uint8) * 255).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1024x1024,1536x2048")
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--ref-planes", type=int, default=2)
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amg_post_bench needs the GPU: nothing is measured without one")
    import amg_post_ref as ref
    from circuitvision_amd import _lib, amg_utils
    lib = _lib.load()
    sp = torch.cuda.current_stream().cuda_stream
    gen_for = None if a.no_generate else _generator()
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        N = a.planes
        host = planes_u8(N, H, W)
        src = host.cuda()
        work = src.clone()
        pixels = N * H * W
        # -- the two kernels
        rle_bytes = int(lib.cvmi_mask_rle_workspace(N, H, W))
        ws_rle = torch.empty(rle_bytes, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(N + 1, dtype=torch.int32, device="cuda")
        _lib.check(lib.cvmi_mask_rle(src.data_ptr(), N, H, W, 0, offsets.data_ptr(), None, ws_rle.data_ptr(), rle_bytes, sp), "mask_rle")
        total = int(offsets[N])
        counts = torch.empty(total, dtype=torch.int32, device="cuda")
        rle = lambda: _lib.check(lib.cvmi_mask_rle(src.data_ptr(), N, H, W, total, offsets.data_ptr(), counts.data_ptr(), ws_rle.data_ptr(), rle_bytes, sp), "mask_rle")
        ws_rm = torch.empty(int(lib.cvmi_mask_remove_small_workspace(N, H, W)), dtype=torch.uint8, device="cuda")
        info = torch.empty(N, 8, dtype=torch.int32, device="cuda")

        def remove_small():                                                     # (the copy that restores the input is timed apart and subtracted)
            work.copy_(src)
            _lib.check(lib.cvmi_mask_remove_small(work.data_ptr(), N, H, W, MIN_AREA, 3, info.data_ptr(), ws_rm.data_ptr(), sp), "mask_remove_small")
        restore = lambda: work.copy_(src)
        remove_small()
        rle()
        torch.cuda.synchronize()
        changed = info.cpu().numpy()
        # -- the composition they replace, on a few planes (the loop is the same per plane)
        t0 = time.perf_counter()
        down = src.cpu()
        d2h_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for p in down[:a.ref_planes].numpy():
            ref.mask_to_rle(p)
        ref_rle_ms = (time.perf_counter() - t0) * 1e3 * N / a.ref_planes
        t0 = time.perf_counter()
        for p in down[:a.ref_planes].numpy():
            ref.remove_small_regions(p, MIN_AREA, "both")
        ref_remove_ms = (time.perf_counter() - t0) * 1e3 * N / a.ref_planes
        variants = {"rle": (rle, event_ms), "remove_small_and_restore": (remove_small, event_ms), "restore": (restore, event_ms),
                    "d2h_counts": (lambda: (offsets.cpu(), counts.cpu()), wall_ms), "d2h_planes": (lambda: src.cpu(), wall_ms)}
        if gen_for is not None:
            gen, many, x, area = gen_for(H, W)
            for tag, g in (("generate", gen), ("many", many)):
                variants.update({tag: (lambda g=g: g.generate_batch(x, orig_hw=[(H, W)]), wall_ms),
                                 tag + "_rle": (lambda g=g: g.generate_batch(x, orig_hw=[(H, W)], output_mode="uncompressed_rle"), wall_ms),
                                 tag + "_min_area": (lambda g=g: g.generate_batch(x, orig_hw=[(H, W)], min_mask_region_area=area), wall_ms),
                                 tag + "_both": (lambda g=g: g.generate_batch(x, orig_hw=[(H, W)], min_mask_region_area=area, output_mode="uncompressed_rle"), wall_ms)})
        t = alternate(variants, a.calls, a.rounds)
        ms = {k: v["ms"] for k, v in t.items()}
        remove_ms = ms["remove_small_and_restore"] - ms["restore"]
        rle_bpp = 1 + 2 / 8 + 4 * total / pixels
        remove_bpp = 2 * (9 + 8) + 2 * 9 + 4
        line = {"what": f"{N} u8 planes of {H} x {W} (blobs, specks, pinholes); kernels: GPU ms between events; d2h / generate: host call to synchronised result; "
                        "ms = median of the windows",
                "H": H, "W": W, "planes": N, "calls_per_window": a.calls, "rounds": a.rounds, **t,
                "runs_total": total, "rle_bytes_per_pixel": rle_bpp, "rle_GBps": pixels * rle_bpp / (ms["rle"] * 1e-3) / 1e9,
                "remove_small_ms": remove_ms, "remove_small_bytes_per_pixel": remove_bpp, "remove_small_GBps": pixels * remove_bpp / (remove_ms * 1e-3) / 1e9,
                "min_area": MIN_AREA, "planes_changed": int(changed[:, 0].sum()), "pixels_filled": int(changed[:, 6].sum()), "pixels_removed": int(changed[:, 7].sum()),
                "composition_d2h_planes_ms_once": d2h_ms, "composition_ref_rle_ms": ref_rle_ms, "composition_ref_remove_ms": ref_remove_ms,
                "composition_planes_timed": a.ref_planes}
        if gen_for is not None:
            one = lambda g, **kw: g.generate_batch(x, orig_hw=[(H, W)], **kw)[0]
            line.update(generate_masks=len(one(gen)), min_mask_region_area=area, generate_masks_after_min_area=len(one(gen, min_mask_region_area=area)),
                        many_masks=len(one(many)), many_masks_after_min_area=len(one(many, min_mask_region_area=area)),
                        many_runs=sum(len(d["segmentation"]["counts"]) for d in one(many, output_mode="uncompressed_rle")))
        line["sub_launches"] = _per_launch(rle, remove_small, pixels, a.calls)
        for k, v in t.items():
            print(f"{H}x{W} {k:26s} {v['ms']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, {a.rounds} windows of {a.calls})")
        print(json.dumps(line))
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "amg_post_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        del src, work, ws_rm, ws_rle, counts


def _per_launch(rle, remove_small, pixels, calls):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            rle()
            remove_small()
        torch.cuda.synchronize()
    per = {}
    for ev in prof.key_averages():
        for name in KERNELS:
            dur = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if name in ev.key and dur:
                us = dur / max(1, ev.count)
                entry = per.setdefault(name, {"us_per_launch": 0.0, "launches_per_call": 0})
                entry["us_per_launch"] += us * ev.count / calls                    # (instances of a template add up)
                entry["launches_per_call"] += ev.count / calls
    for name, entry in per.items():
        entry["us_per_launch"] /= max(entry["launches_per_call"], 1e-9)
        if name in BYTES_PER_PIXEL:
            entry["bytes_per_pixel"] = BYTES_PER_PIXEL[name]
            entry["GBps"] = pixels * BYTES_PER_PIXEL[name] / (entry["us_per_launch"] * 1e-6) / 1e9
    return per if per else "not measured (the profiler reported no kernel)"


def _generator():
    """-> a function (H, W) -> (generator, generator `many`, image tensor, min_mask_region_area): the model of tools/amg_bench.py, thresholds from
    its first chunk."""
    from circuitvision_amd import _lib
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    from circuitvision_amd.sam2 import HIERA_L, LORA_TARGETS_REFERENCE, SamSyntheticParams
    from circuitvision_amd.sam2_infer import SAM2Model
    lib = _lib.load()
    R, f0, Pb, C = 1024, 256, 64, 3
    model = SAM2Model(HIERA_L, R, dtype="f16", use_refinement=True).load_params(SamSyntheticParams(seed=0, lora_targets=LORA_TARGETS_REFERENCE))
    x = torch.randn(1, 3, R, R, generator=torch.Generator().manual_seed(0)).cuda()
    emb = model.encode_images(x)
    probe = Sam2AutomaticMaskGenerator(model)
    _, low, iou = model.infer_masks(emb, points=probe.points_in[:Pb].view(1, Pb, 1, 2), point_labels=torch.ones(1, Pb, 1, dtype=torch.int32), multimask_output=True,
                                    return_high_res=False)
    low, iou = low.view(Pb * C, f0, f0).contiguous(), iou.view(Pb * C).contiguous()
    lo, mid, hi = probe.levels

    def at(H, W):
        stats = torch.empty(Pb * C, 8, dtype=torch.int32, device="cuda")
        _lib.check(lib.cvmi_amg_score(low.data_ptr(), Pb * C, f0, f0, H, W, lo, mid, hi, stats.data_ptr(), None, None), "amg_score")
        st = stats.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
        ious, stab_t = iou.cpu().numpy(), float(np.nanmedian(stab))
        gen = Sam2AutomaticMaskGenerator(model, pred_iou_thresh=max(float(np.median(ious)), 0.0), stability_score_thresh=stab_t)
        many = Sam2AutomaticMaskGenerator(model, pred_iou_thresh=max(float(np.quantile(ious, 0.9)), 0.0), stability_score_thresh=stab_t, box_nms_thresh=1.0)
        return gen, many, x, 100
    return at


if __name__ == "__main__":
    main()
