#!/usr/bin/env python3
"""Time of `infer_masks` with one prompt list per image (`Sam2Plan(pairs=cap)`) next to the tensor form `boxes[B,P,4]` the pipeline pads its
box lists into -- SAM 2.1 Hiera-L, B = 16, synthetic weights, graph replay, f16 and bf16, return_high_res=False as the pipeline calls it.
The prompt counts per image are the fixed list COUNTS below (drawn once with seed 0: mean 12, maximum 48, one image without a box).
  (a) tensor_cut_padded   the tensor form at [16, 32]: every list cut at 32, short lists filled with their first box, an empty one with the
                          whole-image box -- what `CircuitPipeline(max_prompts=32)` runs today; 512 pairs for 176 kept results
  (b) lists_uncut         the list form on the same prompts, nothing cut: 193 pairs in a plan of 224 (pair_bucket 32)
  (c) lists_uniform32     the list form with 32 prompts on every image, against (a): the same 512 pairs, the pair-to-image table in the place
                          of b / P -- what the table itself costs
Device-synchronised host calls, every variant warmed first, the variants alternating in the same process over --rounds rounds of --calls
calls (other work shares the machine); the median round is reported, all rounds are printed.  One JSON line per dtype.
Usage: python tools/ragged_prompt_bench.py [--calls 10] [--rounds 3] [--dtypes f16,bf16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, CAP = 16, 32
COUNTS = [3, 48, 7, 12, 0, 21, 5, 9, 33, 2, 14, 6, 10, 4, 11, 8]          # 193 prompts: mean 12.06, max 48


def window_ms(fn, calls):
    """Milliseconds per call over `calls` synchronous calls (each returns a synchronised result)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(variants, calls, rounds):
    for fn in variants.values():                                # warm-up: plan build, graph capture, allocator
        fn()
        fn()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            runs[k].append(window_ms(fn, calls))
    return {k: float(np.median(v)) for k, v in runs.items()}, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtypes", default="f16,bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_prompt_bench needs the GPU: nothing is measured without one")
    from circuitvision_amd.sam2 import HIERA_L, LORA_TARGETS_REFERENCE, SamSyntheticParams
    from circuitvision_amd.sam2_infer import SAM2Model
    R = 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, R, R, generator=g).cuda()

    def boxes(n):
        side = 24 + 176 * torch.rand(n, 2, generator=g)
        xy = torch.rand(n, 2, generator=g) * (R - side)
        return torch.cat((xy, xy + side), -1)

    lists = [boxes(n) for n in COUNTS]
    padded = torch.zeros(B, CAP, 4)
    for b, l in enumerate(lists):                               # pipeline._segment_chunk with max_prompts = 32
        l = l[:CAP]
        padded[b] = torch.tensor([0.0, 0.0, R, R]) if l.shape[0] == 0 else torch.cat((l, l[:1].repeat(CAP - l.shape[0], 1)))
    uniform = [boxes(CAP) for _ in range(B)]
    for dtype in a.dtypes.split(","):
        model = SAM2Model(HIERA_L, R, dtype=dtype, use_refinement=True).load_params(SamSyntheticParams(seed=0, lora_targets=LORA_TARGETS_REFERENCE))
        variants = {"tensor_cut_padded": lambda: model.infer_masks(x, padded, return_high_res=False),
                    "lists_uncut": lambda: model.infer_masks(x, lists, return_high_res=False),
                    "lists_uniform32": lambda: model.infer_masks(x, uniform, return_high_res=False)}
        ms, runs = alternate(variants, a.calls, a.rounds)
        n_b = sum(COUNTS)
        line = {"what": f"SAM 2.1 Hiera-L {R}^2 {dtype}, B = {B}, infer_masks(return_high_res=False), host call to synchronised result",
                "dtype": dtype, "calls_per_round": a.calls, "rounds": a.rounds, "counts": COUNTS, "pair_bucket": model.pair_bucket,
                "pairs": {"tensor_cut_padded": B * CAP, "lists_uncut": -(-n_b // model.pair_bucket) * model.pair_bucket, "lists_uniform32": B * CAP},
                "results_returned": {"tensor_cut_padded": sum(min(c, CAP) for c in COUNTS), "lists_uncut": n_b, "lists_uniform32": B * CAP},
                "ms": ms, "ms_rounds": runs,
                "spread_ms": {k: max(v) - min(v) for k, v in runs.items()},
                "b_over_a": ms["lists_uncut"] / ms["tensor_cut_padded"], "c_over_a": ms["lists_uniform32"] / ms["tensor_cut_padded"]}
        print(json.dumps(line), flush=True)
        del model, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
