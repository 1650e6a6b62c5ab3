#!/usr/bin/env python3
"""What automatic mask generation costs, stage by stage (SAM 2.1 Hiera-L, synthetic weights, f16, R = 1024, one image, a 32 x 32 point grid in
chunks of 64 points = 192 candidate planes per chunk), at original sizes 1024 x 1024 and 1536 x 2048:
  encode            encode_images(image)                                              host call to synchronised result
  decode            infer_masks(embeddings, 64 points, multimask_output=True)         host call to synchronised result, per chunk
  score             cvmi_amg_score on the chunk's 192 planes                          GPU time (events), per chunk
  composition       what the score stage replaces, built from the parent commit's entry points on the same planes: cvmi_bilinear_f32 writing the
                    f32 map, then torch counts at the three levels and the extents of the mask       GPU time (events), per chunk
  select            cvmi_amg_select of the chunk                                      GPU time (events), per chunk
  nms               cvmi_yolo_nms on the packed block after the last chunk            GPU time (events)
  final_masks       index_select of the survivors + cvmi_amg_score in mask mode       GPU time (events)
  generate          Sam2AutomaticMaskGenerator.generate_batch(image tensor)           host call to synchronised result
The synthetic weights' predicted IoUs and stabilities are not a trained model's, so the thresholds are the medians of the first chunk's values
(about a quarter of the candidates pass both); the counts are reported.  The score stage is also given as a share of the f32 VALU rate
(VALU_PER_SAMPLE instructions per sample, counted in the kernel's inner loop, against 157.3 TFLOP/s / 2 lane-operations per second) and of 8 TB/s
(source planes read once).  Windows alternate round by round; the median window is reported with min and max.  One JSON line per size is printed
and appended to profiles/amg_bench.jsonl.
Usage: python tools/amg_bench.py [--calls 5] [--rounds 5] [--sizes 1024x1024,1536x2048]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

VALU_PER_SAMPLE = 19                             # amg_score_kernel<false, false>: 76 VALU instructions per row of 4 samples in the band loop
VALU_RATE = 157.3e12 / 2                         # f32 lane-operations per second (an FMA counts two FLOP)
HBM_RATE = 8e12


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def event_ms(fn, calls):
    """GPU milliseconds per call between two events around `calls` back-to-back enqueues on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(variants, calls, rounds):
    """{name: {ms, min, max}}: variants = {name: (fn, timer)}; the windows interleave round by round."""
    for fn, _ in variants.values():
        fn()
        fn()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, timer) in variants.items():
            runs[k].append(timer(fn, calls))
    return {k: {"ms": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in runs.items()}


def torch_counts(m, lo, mid, hi):
    """Counts and extents of f32 maps [M, H, W] with torch reductions: what a caller had before cvmi_amg_score."""
    on = m > mid
    n_hi, n_lo, area = (m > hi).sum((1, 2)), (m > lo).sum((1, 2)), on.sum((1, 2))
    cols, rows = on.any(1), on.any(2)
    W, H = cols.shape[1], rows.shape[1]
    x0, x1 = cols.int().argmax(1), W - 1 - cols.flip(1).int().argmax(1)
    y0, y1 = rows.int().argmax(1), H - 1 - rows.flip(1).int().argmax(1)
    return torch.stack([n_hi, n_lo, area, x0, y0, x1, y1], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1024x1024,1536x2048")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amg_bench needs the GPU: nothing is measured without one")
    from circuitvision_amd import _lib
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    from circuitvision_amd.sam2 import HIERA_L, LORA_TARGETS_REFERENCE, SamSyntheticParams
    from circuitvision_amd.sam2_infer import SAM2Model
    lib = _lib.load()
    R, f0, Pb, C = 1024, 256, 64, 3
    M = Pb * C
    model = SAM2Model(HIERA_L, R, dtype="f16", use_refinement=True).load_params(SamSyntheticParams(seed=0, lora_targets=LORA_TARGETS_REFERENCE))
    x = torch.randn(1, 3, R, R, generator=torch.Generator().manual_seed(0)).cuda()
    emb = model.encode_images(x)
    probe = Sam2AutomaticMaskGenerator(model)
    pts = probe.points_in[:Pb].view(1, Pb, 1, 2)
    labels = torch.ones(1, Pb, 1, dtype=torch.int32)
    decode = lambda: model.infer_masks(emb, points=pts, point_labels=labels, multimask_output=True, return_high_res=False)
    _, low, iou = decode()
    low, iou = low.view(M, f0, f0).contiguous(), iou.view(M).contiguous()
    lo, mid, hi = probe.levels
    sp = torch.cuda.current_stream().cuda_stream
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        stats = torch.empty(M, 8, dtype=torch.int32, device="cuda")
        score = lambda: _lib.check(lib.cvmi_amg_score(low.data_ptr(), M, f0, f0, H, W, lo, mid, hi, stats.data_ptr(), None, sp), "amg_score")
        score()
        ymap = torch.empty(M, H, W, device="cuda")

        def composition():
            _lib.check(lib.cvmi_bilinear_f32(low.data_ptr(), M, f0, f0, ymap.data_ptr(), H, W, None, 0.0, sp), "bilinear")
            return torch_counts(ymap, lo, mid, hi)
        same = bool(torch.equal(composition()[:, :3].int(), stats[:, :3]))                  # the composition counts what the kernel counts
        st = stats.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
        iou_t, stab_t = max(float(np.median(iou.cpu().numpy())), 0.0), float(np.nanmedian(stab))
        gen = Sam2AutomaticMaskGenerator(model, pred_iou_thresh=iou_t, stability_score_thresh=stab_t)
        cap = gen.cap
        counter = torch.zeros(2, dtype=torch.int32, device="cuda")
        records = torch.zeros(cap, len(_lib.AMG_RECORD), dtype=torch.int32, device="cuda")
        pool = torch.empty(cap, f0, f0, device="cuda")
        block = torch.zeros(5, cap, device="cuda")
        block[4] = float("-inf")

        def select():
            counter.zero_()
            _lib.check(lib.cvmi_amg_select(stats.data_ptr(), iou.data_ptr(), low.data_ptr(), M, M, C, 0, iou_t, stab_t, f0 * f0, cap, counter.data_ptr(),
                                           records.data_ptr(), pool.data_ptr(), block.data_ptr(), sp), "amg_select")
        out = gen.generate_batch(x, orig_hw=[(H, W)])[0]                                    # also leaves a realistic pool size: K survivors
        K = max(len(out), 1)
        # NMS and the final pass on what a whole call leaves: rebuild the packed block of all 16 chunks once
        full = _packed_block(gen, emb, (H, W))
        ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(1, cap)), dtype=torch.uint8, device="cuda")
        det = torch.empty(min(cap, 4096), 6, device="cuda")
        kidx = torch.empty(min(cap, 4096), dtype=torch.int32, device="cuda")
        kn = torch.empty(1, dtype=torch.int32, device="cuda")
        nms = lambda: _lib.check(lib.cvmi_yolo_nms(full["block"].data_ptr(), 1, 1, cap, iou_t, gen.box_nms_thresh, min(cap, 4096), 0.0, det.data_ptr(),
                                                   kidx.data_ptr(), kn.data_ptr(), ws.data_ptr(), sp), "yolo_nms")
        nms()
        masks = torch.empty(K, H, W, dtype=torch.uint8, device="cuda")
        fstats = torch.empty(K, 8, dtype=torch.int32, device="cuda")

        def final_masks():
            planes = full["pool"].index_select(0, kidx[:K].long())
            _lib.check(lib.cvmi_amg_score(planes.data_ptr(), K, f0, f0, H, W, lo, mid, hi, fstats.data_ptr(), masks.data_ptr(), sp), "amg_score")
        t = alternate({"encode": (lambda: model.encode_images(x), wall_ms), "decode": (decode, wall_ms), "score": (score, event_ms),
                       "composition": (composition, event_ms), "select": (select, event_ms), "nms": (nms, event_ms), "final_masks": (final_masks, event_ms),
                       "generate": (lambda: gen.generate_batch(x, orig_hw=[(H, W)]), wall_ms)}, a.calls, a.rounds)
        ms = {k: v["ms"] for k, v in t.items()}
        samples = M * H * W
        line = {"what": f"SAM 2.1 Hiera-L {R}^2 f16 synthetic weights, one image at {H} x {W}, 32 x 32 grid in 16 chunks of {Pb} points ({M} planes), ms: median of "
                        "the windows, min and max beside it; encode / decode / generate host call to synchronised result, the other stages GPU time between events",
                "H": H, "W": W, "calls_per_window": a.calls, "rounds": a.rounds, **t,
                "pred_iou_thresh": iou_t, "stability_score_thresh": stab_t, "kept_by_filter": int(full["count"]), "masks_after_nms": len(out), "max_candidates": cap,
                "composition_counts_equal": same, "composition_over_score": ms["composition"] / ms["score"], "score_over_decode": ms["score"] / ms["decode"],
                "score_samples_per_s": samples / (ms["score"] * 1e-3), "score_share_of_f32_valu": samples * VALU_PER_SAMPLE / (ms["score"] * 1e-3) / VALU_RATE,
                "score_share_of_8TBps": M * f0 * f0 * 4 / (ms["score"] * 1e-3) / HBM_RATE,
                "composition_bytes": M * f0 * f0 * 4 + 2 * samples * 4}
        for k, v in t.items():
            print(f"{H}x{W} {k:14s} {v['ms']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, {a.rounds} windows of {a.calls})")
        print(json.dumps(line))
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "amg_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        del ymap, masks


def _packed_block(gen, emb, hw):
    """The pool, the packed NMS block and the kept count one whole call builds for an image (the generator's own chunk loop)."""
    st = gen._candidates(emb, [hw])
    torch.cuda.synchronize()
    return dict(pool=st["pool"][0], block=st["block"][0], count=min(int(st["counter"][0, 0]), gen.cap))


if __name__ == "__main__":
    main()
