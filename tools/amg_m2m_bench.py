#!/usr/bin/env python3
"""What the mask-to-mask pass costs and what the in-call form saves (SAM 2.1 Hiera-L, synthetic weights, f16, R = 1024, one image, chunks of 64
points = 192 candidate planes of 256 x 256):
  (a) fanout          cvmi_m2m_fanout for one chunk: clamp of the 192 planes into the second plan's mask_in + the prompt tables     GPU time (events)
      torch_fanout    the torch composition it replaces on the same buffers: torch.clamp, repeat_interleave of coords / labels,
                      copy_ into mask_in / coords / labels                                                                      GPU time (events)
  (b) m2m_in_call     infer_masks(embeddings, 64 points, multimask_output=True, m2m=True)                      host call to synchronised result
      m2m_composed    the same result through the host, as a caller composed it before: infer_masks(multimask_output=True), torch.clamp,
                      infer_masks(points repeated 3 times, mask_input=...)                                    host call to synchronised result
      decode          the chunk without the pass: infer_masks(embeddings, 64 points, multimask_output=True)    host call to synchronised result
  (c) generate / generate_m2m   Sam2AutomaticMaskGenerator.generate_batch(image tensor) without and with use_m2m=True, a 32 x 32 grid in 16
                      chunks, at original sizes 1024 x 1024 and 1536 x 2048                                    host call to synchronised result
The synthetic weights' predicted IoUs and stabilities are not a trained model's, so the thresholds are the medians of the first chunk's refined
values; the mask counts are reported.  Windows alternate round by round; the median window is reported with min and max.  One JSON line per
size is printed and appended to profiles/amg_m2m_bench.jsonl (the rows of (a) and (b) do not depend on the size and are in the first line only).
Usage: python tools/amg_m2m_bench.py [--calls 5] [--rounds 5] [--sizes 1024x1024,1536x2048]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from amg_bench import alternate, event_ms, wall_ms  # noqa: E402

HBM_RATE = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1024x1024,1536x2048")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amg_m2m_bench needs the GPU: nothing is measured without one")
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
    pts3, labels3 = pts.repeat_interleave(C, 1), labels.repeat_interleave(C, 1)
    decode = lambda: model.infer_masks(emb, points=pts, point_labels=labels, multimask_output=True, return_high_res=False)
    in_call = lambda: model.infer_masks(emb, points=pts, point_labels=labels, multimask_output=True, return_high_res=False, m2m=True)

    def composed():
        _, low, _ = decode()
        return model.infer_masks(emb, points=pts3, point_labels=labels3, mask_input=torch.clamp(low, -32.0, 32.0).view(1, M, f0, f0), return_high_res=False)
    got, want = in_call(), composed()
    same = bool(torch.equal(got[1].reshape(-1), want[1].reshape(-1)) and torch.equal(got[2].reshape(-1), want[2].reshape(-1)))
    # (a) on the two plans' own buffers
    p1 = model.plan(1, prompts=Pb, high_res=False, points=2, multimask=True, stage="decode")
    p2 = model.plan(1, prompts=M, high_res=False, points=2, mask_prompt=True, stage="decode")
    sp = torch.cuda.current_stream().cuda_stream
    K = p1.coords.shape[1]
    fanout = lambda: _lib.check(lib.cvmi_m2m_fanout(p1.low_res.data_ptr(), C, 32.0, p2.mask_in.data_ptr(), p1.coords.data_ptr(), p1.labels.data_ptr(), None,
                                                    p2.coords.data_ptr(), p2.labels.data_ptr(), None, Pb, f0 * f0, K, sp), "m2m_fanout")

    def torch_fanout():
        p2.mask_in.copy_(torch.clamp(p1.low_res, -32.0, 32.0).view(M, f0, f0))
        p2.coords.copy_(p1.coords.repeat_interleave(C, 0))
        p2.labels.copy_(p1.labels.repeat_interleave(C, 0))
    torch.cuda.synchronize()
    torch_fanout()
    ref_mask = p2.mask_in.clone()
    p2.mask_in.zero_()
    fanout()
    torch.cuda.synchronize()
    fan_same = bool(torch.equal(p2.mask_in, ref_mask))
    chunk = alternate({"fanout": (fanout, event_ms), "torch_fanout": (torch_fanout, event_ms), "decode": (decode, wall_ms), "m2m_in_call": (in_call, wall_ms),
                       "m2m_composed": (composed, wall_ms)}, a.calls, a.rounds)
    cms = {k: v["ms"] for k, v in chunk.items()}
    for k, v in chunk.items():
        print(f"chunk {k:14s} {v['ms']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, {a.rounds} windows of {a.calls})")
    iou_t, stab_t = _thresholds(probe, got)
    for n, size in enumerate(a.sizes.split(",")):
        H, W = (int(v) for v in size.split("x"))
        gen = Sam2AutomaticMaskGenerator(model, pred_iou_thresh=iou_t, stability_score_thresh=stab_t)
        plain = lambda: gen.generate_batch(x, orig_hw=[(H, W)])
        m2m = lambda: gen.generate_batch(x, orig_hw=[(H, W)], use_m2m=True)
        counts = (len(plain()[0]), len(m2m()[0]))
        t = alternate({"generate": (plain, wall_ms), "generate_m2m": (m2m, wall_ms)}, a.calls, a.rounds)
        line = {"what": f"SAM 2.1 Hiera-L {R}^2 f16 synthetic weights, one image at {H} x {W}, 32 x 32 grid in 16 chunks of {Pb} points ({M} planes), ms: median "
                        "of the windows, min and max beside it; fanout / torch_fanout GPU time between events, the rest host call to synchronised result",
                "H": H, "W": W, "calls_per_window": a.calls, "rounds": a.rounds, **t, "masks": counts[0], "masks_m2m": counts[1],
                "pred_iou_thresh": iou_t, "stability_score_thresh": stab_t, "m2m_over_plain_generate": t["generate_m2m"]["ms"] / t["generate"]["ms"]}
        if n == 0:
            line.update(chunk, in_call_equals_composed=same, fanout_equals_torch=fan_same, torch_over_fanout=cms["torch_fanout"] / cms["fanout"],
                        composed_over_in_call=cms["m2m_composed"] / cms["m2m_in_call"], in_call_over_decode=cms["m2m_in_call"] / cms["decode"],
                        fanout_share_of_8TBps=2 * M * f0 * f0 * 4 / (cms["fanout"] * 1e-3) / HBM_RATE,
                        plan_act_bytes={"pass_1_64_pairs": int(p1.act_bytes), "pass_2_192_pairs": int(p2.act_bytes)})
        for k, v in t.items():
            print(f"{H}x{W} {k:14s} {v['ms']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, {a.rounds} windows of {a.calls}); masks {counts}")
        print(json.dumps(line))
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "amg_m2m_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")


def _thresholds(probe, refined):
    """Medians of the first chunk's refined predicted IoUs and of their stabilities at 1024 x 1024 (cvmi_amg_score on the refined planes)."""
    from circuitvision_amd import _lib
    lib = _lib.load()
    _, low, iou = refined
    M, f0 = low.numel() // (low.shape[-1] * low.shape[-2]), low.shape[-1]
    low = low.reshape(M, f0, f0).contiguous()
    stats = torch.empty(M, 8, dtype=torch.int32, device="cuda")
    lo, mid, hi = probe.levels
    _lib.check(lib.cvmi_amg_score(low.data_ptr(), M, f0, f0, 1024, 1024, lo, mid, hi, stats.data_ptr(), None, torch.cuda.current_stream().cuda_stream), "amg_score")
    st = stats.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
    return max(float(np.median(iou.cpu().numpy())), 0.0), float(np.nanmedian(stab))


if __name__ == "__main__":
    main()
