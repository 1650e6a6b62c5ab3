"""Mask prompts and multimask output without a GPU: the reference the GPU tests compare with (tests/mask_prompt_ref.py) against an independent
implementation and a by-hand known answer, the wrong implementations the op comparison has to catch, and the weight plumbing
(`SamSyntheticParams.mask_prompt_state_dict`, `Sam2Weights.const["mask_down"]`, the broadcast list, a checkpoint without the stack)."""
import math
import os
import sys

import pytest
import torch

import mask_prompt_ref as ref
from circuitvision_amd._lib import F32
from circuitvision_amd.sam2 import MASK_DOWN_PARAMS, Sam2Weights, SamBlankParams, SamStateDictParams, SamSyntheticParams
from test_oracle_sam2_cpu import MINI, mini_oracle, mini_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(seed=9):
    return SamSyntheticParams(seed=seed, lora_targets=mini_targets(), std=0.05)


def full_sd(p):
    """Everything the reference reads: the oracle's state dict plus the mask stack."""
    return {**p.state_dict(), **p.mask_prompt_state_dict()}


def test_reference_stack_matches_independent_implementation():
    tr = pytest.importorskip("transformers")
    from transformers.models.sam2 import configuration_sam2 as C
    from transformers.models.sam2 import modeling_sam2 as M
    sd = _params().mask_prompt_state_dict()
    hf = M.Sam2MaskEmbedding(C.Sam2PromptEncoderConfig()).eval()
    names = {"conv1": 0, "layer_norm1": 1, "conv2": 3, "layer_norm2": 4, "conv3": 6}
    hf.load_state_dict({f"{n}.{part}": sd[f"{ref.MD}.{i}.{part}"] for n, i in names.items() for part in ("weight", "bias")}, strict=True)
    mask = 6 * torch.randn(3, 1, 36, 36, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = hf(mask)
    got = ref.mask_downscaling(sd, mask, torch.float32)
    assert got.shape == want.shape == (3, 256, 9, 9)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ref.mask_downscaling(sd, mask, torch.float64).float(), want, rtol=1e-5, atol=1e-5)


def test_reference_stack_known_answer_by_hand():
    """One 4 x 4 mask.  Conv 1: channel c copies tap c (dy, dx = c // 2, c % 2) of its 2 x 2 block, and every block holds [a, a; a + 2, a + 2] with its own
    a -> the four channels are a, a, a + 2, a + 2: mean a + 1, deviations -1, -1, 1, 1, biased variance 1 -> LayerNorm -r, -r, r, r with
    r = 1 / sqrt(1 + 1e-6), whatever a is; GELU -> n, n, p, p.  Conv 2: channels 0..7 copy channel 2 of block (0, 0) (= p), channels 8..15 channel 0
    of block (0, 0) (= n): mean (p + n) / 2, deviations +-e with e = (p - n) / 2, variance e^2 -> +-r2 with r2 = e / sqrt(e^2 + 1e-6); weight 2, bias
    0.5, GELU -> P = gelu(2 r2 + 0.5), N = gelu(-2 r2 + 0.5).  Conv 3: out[k] = k / 256 * h[0] + h[15] - k = k / 256 * P + N - k."""
    gelu = lambda v: 0.5 * v * (1 + math.erf(v / math.sqrt(2)))
    sd = {k: torch.zeros(s, dtype=torch.float64) for k, s in ref.SHAPES.items()}
    for c in range(4):
        sd[f"{ref.MD}.0.weight"][c, 0, c // 2, c % 2] = 1
    sd[f"{ref.MD}.1.weight"][:] = 1
    sd[f"{ref.MD}.3.weight"][:8, 2, 0, 0] = 1
    sd[f"{ref.MD}.3.weight"][8:, 0, 0, 0] = 1
    sd[f"{ref.MD}.4.weight"][:] = 2
    sd[f"{ref.MD}.4.bias"][:] = 0.5
    k = torch.arange(256, dtype=torch.float64)
    sd[f"{ref.MD}.6.weight"][:, 0, 0, 0] = k / 256
    sd[f"{ref.MD}.6.weight"][:, 15, 0, 0] = 1
    sd[f"{ref.MD}.6.bias"][:] = -k
    mask = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    for (sy, sx), a in {(0, 0): 3.0, (0, 1): -7.0, (1, 0): 0.25, (1, 1): 40.0}.items():
        mask[0, 0, 2 * sy, 2 * sx:2 * sx + 2] = a
        mask[0, 0, 2 * sy + 1, 2 * sx:2 * sx + 2] = a + 2
    r = 1 / math.sqrt(1 + 1e-6)
    p, n = gelu(r), gelu(-r)
    e = (p - n) / 2
    r2 = e / math.sqrt(e * e + 1e-6)
    P, N = gelu(2 * r2 + 0.5), gelu(-2 * r2 + 0.5)
    got = ref.mask_downscaling(sd, mask, torch.float64)
    assert got.shape == (1, 256, 1, 1)
    torch.testing.assert_close(got.reshape(256), k / 256 * P + N - k, rtol=0, atol=1e-12)
    # the taps are not symmetric: transposing them in the first convolution swaps channels 1 and 2 (a and a + 2) -> another answer
    assert float((ref.mask_downscaling(sd, mask, torch.float64, "taps1") - got).abs().max()) > 0.1


@pytest.mark.parametrize("B,rep,fs", ref.OP_SHAPES[:4])
def test_op_comparison_catches_wrong_implementations(B, rep, fs):
    """The GPU op test compares cvmi_mask_prompt_embed with the float64 reference at 8 x the error of the f32 evaluation of that reference.
    On the op test's own inputs that bound tells every mutant from the reference.  (The fifth shape repeats the fourth's geometry with more
    pairs for the capped grid, which is no property of the reference; it is left to the GPU.)"""
    sd = ref.op_state_dict(_params())
    mask, emb = ref.op_inputs(B, rep, fs, sd)
    assert not mask[0, :4].any() and set(mask[-1, -4:].unique().tolist()) == {-30.0, 30.0} and mask.unique().numel() > mask.numel() // 4
    want = ref.mask_prompt_keys(sd, mask, emb, rep)
    bound = 8 * float((ref.mask_prompt_keys(sd, mask, emb, rep, torch.float32).double() - want).abs().max())
    assert 0 < bound < 1e-5, bound
    for mutant in ref.MUTANTS:
        if mutant == "pair_major" and (B == 1 or rep == 1):
            continue                                           # (the two orders coincide)
        err = float((ref.mask_prompt_keys(sd, mask, emb, rep, mutant=mutant) - want).abs().max())
        assert err > 100 * bound, (mutant, err, bound)
    assert any(B_ > 1 and r_ > 1 for B_, r_, _ in ref.OP_SHAPES[:4])          # pair_major is judged somewhere


def test_synthetic_state_dict_is_unchanged_and_still_loads_strictly():
    p = _params()
    p0 = _params()
    Sam2Weights(p0, MINI, 256, F32, device="cpu", use_refinement=True)
    before = set(p0.state_dict())
    assert not any("mask_downscaling" in k for k in before)
    wt = Sam2Weights(p, MINI, 256, F32, device="cpu")
    assert wt.mask_prompt_ok and wt.prompt_ok
    assert set(p.state_dict()) == before                       # reading the mask stack adds no key
    p.mask_prompt_state_dict()
    assert set(p.state_dict()) == before
    mini_oracle(p, 256)                                        # strict=True inside
    msd = p.mask_prompt_state_dict()
    assert {k: tuple(v.shape) for k, v in msd.items()} == ref.SHAPES
    fresh = _params().mask_prompt_state_dict()                 # the same tensors whether or not Sam2Weights read them first
    assert all(torch.equal(msd[k], fresh[k]) for k in msd)
    for i in (1, 4):                                           # gammas are of the "gamma" kind
        g = msd[f"{ref.MD}.{i}.weight"]
        assert float(g.min()) >= 0.8 and float(g.max()) <= 1.2


def test_packed_parameter_vector_layout():
    p = _params()
    wt = Sam2Weights(p, MINI, 256, F32, device="cpu")
    v = wt.const["mask_down"]
    assert v.dtype == torch.float32 and v.numel() == MASK_DOWN_PARAMS == 4684
    sd = full_sd(p)
    assert torch.equal(v, ref.pack_params(sd))
    off = 0
    for k, shape in ref.SHAPES.items():
        n = math.prod(shape)
        want = sd[k].reshape(-1)
        if k.endswith("6.bias"):
            want = want - sd[ref.NO_MASK].reshape(-1)          # b3' = b3 - no_mask_embed
        assert torch.equal(v[off:off + n], want), k
        off += n
    assert off == 4684
    hdr = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    assert "#define CVMI_MASK_PROMPT_PARAMS 4684" in hdr


def test_blank_params_and_broadcast_list():
    from circuitvision_amd.distributed import weight_tensors
    wb = Sam2Weights(SamBlankParams(), MINI, 256, F32, device="cpu")
    assert wb.mask_prompt_ok and wb.const["mask_down"].numel() == 4684 and not wb.const["mask_down"].any()
    wt = Sam2Weights(_params(), MINI, 256, F32, device="cpu")
    sent = {t.data_ptr() for t in weight_tensors(wt)}
    assert wt.const["mask_down"].data_ptr() in sent
    assert wb.const["mask_down"].data_ptr() in {t.data_ptr() for t in weight_tensors(wb)}


def test_state_dict_with_and_without_the_mask_stack():
    p = _params()
    want = Sam2Weights(p, MINI, 256, F32, device="cpu").const["mask_down"]
    sd = {"sam2_model.base_model.model." + k if not k.startswith(("dense_", "sparse_", "refinement_")) else k: v for k, v in full_sd(p).items()}
    wt = Sam2Weights(SamStateDictParams(sd), MINI, 256, F32, device="cpu")
    assert wt.mask_prompt_ok and torch.equal(wt.const["mask_down"], want)
    stripped = {k: v for k, v in sd.items() if "mask_downscaling." not in k}
    assert len(stripped) == len(sd) - 10
    ws = Sam2Weights(SamStateDictParams(stripped), MINI, 256, F32, device="cpu")
    assert ws.prompt_ok and not ws.mask_prompt_ok and "mask_down" not in ws.const


def test_reference_predictor_takes_a_mask_per_prompt_and_the_gpu_cases_select_clearly():
    """The oracle decoder accepts a per-prompt dense prompt; the mask prompt moves the logits (single-mask and multimask) by far more than
    any tolerance; and on the inputs the GPU tests use (MINI_SEED, REPLAY_SEED) no single-mask selection is within rounding of flipping."""
    p = _params()
    Sam2Weights(p, MINI, 256, F32, device="cpu")
    sd, oracle = full_sd(p), mini_oracle(p, 256)
    c = ref.mini_inputs(ref.MINI_SEED)
    kinds = (dict(boxes=c["boxes"]), dict(points=c["points"], labels=c["labels"]), dict(boxes=c["boxes"], points=c["points"], labels=c["labels"]))
    with torch.no_grad():
        for kw in kinds:
            hi, lo, iou, stab, iou4 = ref.predict_prompts_masked(oracle, sd, c["x"], mask_input=c["mask"], margins=True, **kw)
            assert hi.shape == (2, 3, 1, 256, 256) and lo.shape == (2, 3, 1, 64, 64) and iou.shape == (2, 3, 1)
            assert ref.selection_is_clear(stab, iou4), kw.keys()
        c2 = ref.mini_inputs(ref.REPLAY_SEED)
        *_, stab, iou4 = ref.predict_prompts_masked(oracle, sd, c2["x"], boxes=c2["boxes"], mask_input=c2["mask"], margins=True)
        assert ref.selection_is_clear(stab, iou4)
        _, lo0, _ = ref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"])
        _, lo1, _ = ref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"], mask_input=c["mask"])
        _, m0, i0 = ref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"], multimask_output=True)
        _, m1, _ = ref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"], mask_input=c["mask"], multimask_output=True)
    assert m0.shape == (2, 3, 3, 64, 64) and i0.shape == (2, 3, 3)
    assert float((lo1 - lo0).abs().max()) > 0.1 and float((m1 - m0).abs().max()) > 0.1
    # without a mask the reference is the oracle's own predictor
    from oracle import sam2_model as osam
    with torch.no_grad():
        _, rlo, _ = osam.predict_prompts(oracle, c["x"], boxes=c["boxes"])
    assert torch.equal(lo0[:, :, 0], rlo)
