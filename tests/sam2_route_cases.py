"""Configurations whose Hiera launch sequence is pinned (tests/test_sam2_route_cpu.py against tests/sam2_route_fixture.json, tests/test_sam2_route_gpu.py
against the plan itself), and the fixture's form: per configuration the trunk's launches block by block, labels without their `b{i}.` prefix and
kernels as their family (cvmi_last_kernel's name up to `_kernel`), equal consecutive blocks collapsed to [count, [[suffix, kind, family], ...]].

`python tests/sam2_route_cases.py OUT.json` (on a GPU) records the fixture from the plans as they are built: run it BEFORE a change that is meant to
leave the launches alone, or after one that changes routing on purpose (and say so in that pull request).

HEAD_CASES below do the same for everything outside the blocks (tests/test_decoder_route_cpu.py / _gpu.py against tests/decoder_route_fixture.json)."""
import json
import os
import re
import sys

SWITCHES = ("CVMI_SAM_FUSED_MLP", "CVMI_SAM_TOKLIN", "CVMI_SAM_QLOG2", "CVMI_SAM_QKVATTN", "CVMI_SAM_QKVATTN16", "CVMI_SAM_QKVTOK_TRANS",
            "CVMI_SAM_POOLFUSE", "CVMI_SAM_LNSTATS", "CVMI_SAM_LNSTATS_FC2", "CVMI_SAM_PROJMLP", "CVMI_SAM_NECKCAST", "CVMI_SAM_SHARE_L0")


def _case(id, hiera, size, dtype, B, attn="16", prompts=0, env=None):
    return dict(id=id, hiera=hiera, size=size, dtype=dtype, B=B, attn=attn, prompts=prompts, env=env or {})


CASES = [
    _case("L_f16_B16", "HIERA_L", 1024, "f16", 16),
    _case("L_f16_B2", "HIERA_L", 1024, "f16", 2),
    _case("L_bf16_B2", "HIERA_L", 1024, "bf16", 2),
    _case("L_f32_B1", "HIERA_L", 1024, "f32", 1),
    _case("L_f16_B2_fp8", "HIERA_L", 1024, "f16", 2, attn="fp8"),
    _case("L_f16_B2_prompts2", "HIERA_L", 1024, "f16", 2, prompts=2),
    _case("mini144_f16_B2", "MINI144", 256, "f16", 2),                   # tests/test_proj_mlp_gpu.py
    _case("mini16_f32_B2", "MINI", 256, "f32", 2),                       # test_sam2_wrapper_mini_matches_oracle
    _case("mini16_f16_B2", "MINI", 256, "f16", 2),
    _case("mini16_bf16_B2", "MINI", 256, "bf16", 2),
    _case("tiny_f32_B1", "HIERA_T", 1024, "f32", 1),                     # test_sam2_hiera_tiny_padded_windows_match_oracle
    _case("tiny_f16_B1", "HIERA_T", 1024, "f16", 1),
] + [_case(f"L_f16_B16_{name[9:]}=0", "HIERA_L", 1024, "f16", 16, env={name: "0"}) for name in SWITCHES]


def hiera_of(name):
    if name == "MINI144":
        from test_proj_mlp_gpu import MINI144
        return MINI144
    if name == "MINI":
        from test_oracle_sam2_cpu import MINI
        return MINI
    from circuitvision_amd import sam2
    return getattr(sam2, name)


def lora_targets_of(name):
    from circuitvision_amd.sam2 import LORA_TARGETS_REFERENCE
    if name == "HIERA_L":
        return LORA_TARGETS_REFERENCE
    if name == "HIERA_T":
        return [x for x in LORA_TARGETS_REFERENCE if ".trunk." not in x]
    from test_oracle_sam2_cpu import mini_targets
    return mini_targets()


def dtype_of(name):
    from circuitvision_amd._lib import BF16, F16, F32
    return dict(f16=F16, bf16=BF16, f32=F32)[name]


BLOCK_LABEL = re.compile(r"b(\d+)\.(.+)")


def trunk_blocks(launches):
    """[(label, kind, kernel)] of a whole plan -> per Hiera block the [suffix, kind, family] of its launches, in order."""
    blocks = []
    for op in launches:
        m = BLOCK_LABEL.fullmatch(op[0])
        if m:
            i = int(m.group(1))
            assert i in (len(blocks) - 1, len(blocks)), op[0]
            if i == len(blocks):
                blocks.append([])
            blocks[i].append([m.group(2), op[1], op[2].split("_kernel")[0]])
    return blocks


def family_implied(suffix, family, route, window):
    """Is `family` the kernel family the route's choice for launch b{i}.<suffix> implies?  Token-stationary launches run tok_linear / tok_linear16
    and nothing else does; a fused qkv runs qkv_attn64 (8 x 8 windows) / qkv_attn16 (4 x 4); the MLP launch is proj_mlp with the proj prologue,
    hiera_mlp without."""
    tok = dict(dimproj_pool=True, qkv=route.qkv == "tok", proj=route.proj == "tok", fc1=route.mlp == "tok_fc1")
    if suffix == "attn":
        return family == {8: "qkv_attn64", 4: "qkv_attn16"}[window] if route.qkv == "fused" else not family.startswith("qkv_attn")
    if suffix == "mlp":
        return family == ("proj_mlp" if route.proj == "fused" else "hiera_mlp")
    return family.startswith("tok_linear") == tok.get(suffix, False)


def collapse(blocks):
    out = []
    for b in blocks:
        if out and out[-1][1] == b:
            out[-1][0] += 1
        else:
            out.append([1, b])
    return out


def expand(runs):
    return [b for n, b in runs for _ in range(n)]


def build_plan(case, params_cache=None):
    """Sam2Weights + Sam2Plan of a case under its switches (GPU).  params_cache: {hiera name: SamSyntheticParams} shared between cases."""
    import torch
    from circuitvision_amd.sam2 import Sam2Plan, Sam2Weights, SamSyntheticParams
    params_cache = {} if params_cache is None else params_cache
    if case["hiera"] not in params_cache:
        params_cache[case["hiera"]] = SamSyntheticParams(seed=5, lora_targets=lora_targets_of(case["hiera"]), std=0.05)
    old = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        wt = Sam2Weights(params_cache[case["hiera"]], hiera_of(case["hiera"]), case["size"], dtype_of(case["dtype"]))
        return Sam2Plan(wt, case["B"], torch.cuda.Stream(), attn=case["attn"], prompts=case["prompts"])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- everything after the trunk: neck, mask decoder, tail (circuitvision_amd/decoder_route.py) ------------------------------------------------
# tests/decoder_route_fixture.json, per configuration {"act_bytes": the plan's, "launches": [[label, kind, bytes, flops, kernel family], ...]} of
# every launch whose label is not a block's (the two stem launches in front of the trunk included), in launch order.
# `python tests/sam2_route_cases.py --head OUT.json` (on a GPU) records it, under the same rule as the trunk's fixture.
def _head(id, dtype, hiera="MINI", refinement=True, env=None, **plan):
    return dict(id=id, hiera=hiera, size=256, dtype=dtype, B=2, refinement=refinement, env=env or {}, plan=plan)


_NO_SHARE, _NO_NECKCAST = {"CVMI_SAM_SHARE_L0": "0"}, {"CVMI_SAM_NECKCAST": "0"}
HEAD_CASES = [
    _head("learned_f16", "f16"), _head("learned_bf16", "bf16"), _head("learned_f32", "f32"),
    _head("learned_f16_norefine", "f16", refinement=False),
    _head("learned_f16_lowres", "f16", high_res=False),
    _head("prompts2_f16", "f16", prompts=2), _head("prompts2_f32", "f32", prompts=2),
    _head("prompts2_f16_SHARE_L0=0", "f16", prompts=2, env=_NO_SHARE),
    _head("prompts2_mask_f16", "f16", prompts=2, mask_prompt=True), _head("prompts2_mask_f32", "f32", prompts=2, mask_prompt=True),
    _head("prompts2_multimask_f16", "f16", prompts=2, multimask=True),
    _head("pairs3_f16", "f16", pairs=3), _head("pairs3_f32", "f32", pairs=3),
    _head("pairs3_f16_SHARE_L0=0", "f16", pairs=3, env=_NO_SHARE),
    _head("pairs3_mask_f16", "f16", pairs=3, mask_prompt=True),
    _head("mini144_learned_f16", "f16", hiera="MINI144"),                # MINI's 16 / 32-wide stage outputs have no token-stationary neck; 144 / 288 do
    _head("mini144_learned_f16_NECKCAST=0", "f16", hiera="MINI144", env=_NO_NECKCAST),
]
STEM = [["s2d4", "stem"], ["patch_embed", "stem"]]                       # what the fixture holds in front of the route's launches


def head_params(hiera):
    """The synthetic checkpoint the prompt tests build their mini models from (MINI144: test_proj_mlp_gpu's)."""
    if hiera == "MINI":
        from test_mask_prompt_gpu import _params
        return _params()
    from circuitvision_amd.sam2 import SamSyntheticParams
    return SamSyntheticParams(seed=5, lora_targets=lora_targets_of(hiera), std=0.05)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def build_head_plan(case, cache=None):
    """Sam2Plan of a HEAD_CASE under its switches (GPU).  cache: {(hiera, dtype, refinement): Sam2Weights} shared between cases (the two
    switches the cases set are plan-level)."""
    import torch
    from circuitvision_amd.sam2 import Sam2Plan, Sam2Weights
    cache = {} if cache is None else cache
    key = (case["hiera"], case["dtype"], case["refinement"])
    if key not in cache:
        cache[key] = Sam2Weights(head_params(case["hiera"]), hiera_of(case["hiera"]), case["size"], dtype_of(case["dtype"]), use_refinement=case["refinement"])
    return _with_env(case["env"], lambda: Sam2Plan(cache[key], case["B"], torch.cuda.Stream(), **case["plan"]))


def head_launches(sp):
    """[[label, kind, bytes, flops, kernel family]] of a plan's launches outside the Hiera blocks (one timed eager pass)."""
    return [[t[0], t[1], t[3], t[4], t[5].split("_kernel")[0]] for t in sp.plan.timed_eager(with_kernels=True) if not BLOCK_LABEL.fullmatch(t[0])]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    cache, fixture = {}, {}
    if sys.argv[1] == "--head":
        for case in HEAD_CASES:
            sp = build_head_plan(case, cache)
            fixture[case["id"]] = dict(act_bytes=sp.act_bytes, launches=head_launches(sp))
            del sp
    else:
        for case in CASES:
            sp = build_plan(case, cache)
            fixture[case["id"]] = collapse(trunk_blocks([(t[0], t[1], t[5]) for t in sp.plan.timed_eager(with_kernels=True)]))
            del sp
    with open(sys.argv[-1], "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
