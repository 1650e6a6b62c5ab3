"""Mask prompts and multimask output on the GPU (csrc/mask_prompt.hip, `Sam2Plan(mask_prompt=, multimask=)`, `infer_masks(mask_input=,
multimask_output=)`) against tests/mask_prompt_ref.py: the kernel through the C ABI vs float64, the mini model in f32 and F16 vs the
reference predictor, the multimask tail, graph replay and the error paths.  The op and model tests print their measured errors before they assert
(`pytest -s`)."""
import functools

import pytest
import torch

import mask_prompt_ref as ref
from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE
from test_oracle_sam2_cpu import MINI, mini_oracle, mini_targets

pytestmark = pytest.mark.gpu
R, B, P = 256, 2, 3
F0 = R // 4
TOL32 = dict(rtol=1e-3, atol=1e-3)               # the project's f32 bound (test_infer_masks_click_prompts_match_oracle)
TOL16 = dict(rtol=3e-2, atol=3e-2)               # test_sam2_box_prompts_mini_match_oracle, F16
GUARD = 512                                      # elements behind every output the kernel must leave alone


@functools.lru_cache(None)
def _params():
    from circuitvision_amd.sam2 import SamSyntheticParams
    return SamSyntheticParams(seed=9, lora_targets=mini_targets(), std=0.05)


@functools.lru_cache(None)
def _model():
    from circuitvision_amd.sam2_infer import SAM2Model
    return SAM2Model(MINI, R, dtype="f32", use_refinement=True).load_params(_params())


@functools.lru_cache(None)
def _oracle():
    _model()                                                          # (the packed model has read every tensor the oracle loads)
    p = _params()
    return mini_oracle(p, R), {**p.state_dict(), **p.mask_prompt_state_dict()}


def _kind(c, kind):
    return dict(boxes=c["boxes"] if "boxes" in kind else None, points=c["points"] if "points" in kind else None,
                labels=c["labels"] if "points" in kind else None)


@functools.lru_cache(None)
def _reference(seed, kind, masked, multimask):
    """The reference predictor's result, computed once per case: (high_res, low_res, iou), all [B,P,n,...]; single-mask cases assert the
    precondition first -- every pair selects clearly (mask_prompt_ref.selection_is_clear)."""
    oracle, sd = _oracle()
    c = ref.mini_inputs(seed)
    with torch.no_grad():
        out = ref.predict_prompts_masked(oracle, sd, c["x"], mask_input=c["mask"] if masked else None, multimask_output=multimask,
                                         margins=not multimask, **_kind(c, kind))
    if not multimask:
        assert ref.selection_is_clear(out[3], out[4]), (seed, kind, masked)
    return out[:3]


def _call(c, kind, **kw):
    k = _kind(c, kind)
    return _model().infer_masks(c["x"], boxes=k["boxes"], points=k["points"], point_labels=k["labels"], **kw)


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------------------------
def _embed(mask_d, emb_d, prm_d, rep, fs, lp=None):
    """-> (keys f32 [n, fs*fs, 256], 16-bit copy or None, kernel tag); both outputs carry a guard band that must come back untouched."""
    lib = _lib.load()
    n, Bn = mask_d.shape[0], emb_d.shape[0]
    numel = n * fs * fs * 256
    keys = torch.full((numel + GUARD,), -7.0, device="cuda")
    klp = torch.full((numel + GUARD,), -7.0, device="cuda", dtype=TORCH_DTYPE[lp]) if lp is not None else None
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _lib.check(lib.cvmi_mask_prompt_embed(mask_d.data_ptr(), emb_d.data_ptr(), prm_d.data_ptr(), keys.data_ptr(), klp.data_ptr() if lp is not None else None,
                                          lp if lp is not None else 0, Bn, rep, fs, None), "mask_prompt_embed")
    tag = lib.cvmi_last_kernel().decode()
    torch.cuda.synchronize()
    assert bool((keys[numel:] == -7.0).all()) and (klp is None or bool((klp[numel:] == -7.0).all())), "wrote past the end"
    return keys[:numel].view(n, fs * fs, 256), (klp[:numel].view(n, fs * fs, 256) if lp is not None else None), tag


@pytest.mark.parametrize("Bn,rep,fs", ref.OP_SHAPES)
def test_mask_prompt_embed_vs_fp64(Bn, rep, fs):
    """cvmi_mask_prompt_embed vs the float64 reference.  Bound: 8 x the error of the f32 torch evaluation of the same reference on the same inputs
    (the device's erff and division are a few ulp where torch's are correctly rounded).  The 16-bit copies are the kernel's own f32 output
    rounded once, bit for bit; a second run repeats the first bit for bit."""
    sd = ref.op_state_dict(_params())
    mask, emb = ref.op_inputs(Bn, rep, fs, sd)
    want = ref.mask_prompt_keys(sd, mask, emb, rep)
    f32_err = float((ref.mask_prompt_keys(sd, mask, emb, rep, torch.float32).double() - want).abs().max())
    mask_d, emb_d, prm_d = mask.cuda(), emb.cuda(), ref.pack_params(sd).cuda()
    keys, k16, tag = _embed(mask_d, emb_d, prm_d, rep, fs, F16)
    err = float((keys.double() - want.cuda()).abs().max())
    print(f"mask_prompt_embed B={Bn} rep={rep} fs={fs}: |kernel - f64| = {err:.3e}, |torch f32 - f64| = {f32_err:.3e} "
          f"(x{err / f32_err:.2f}), output std {float(want.std()):.3f}")
    assert tag == "mask_prompt_embed_kernel<_Float16>"
    assert err <= 8 * f32_err, (err, f32_err)
    assert torch.equal(k16, keys.to(torch.float16))
    keys_b, kbf, tag_b = _embed(mask_d, emb_d, prm_d, rep, fs, BF16)
    assert tag_b == "mask_prompt_embed_kernel<__bf16>"
    assert torch.equal(keys_b, keys) and torch.equal(kbf, keys.to(torch.bfloat16))
    keys_n, none, _ = _embed(mask_d, emb_d, prm_d, rep, fs)            # no 16-bit copy
    assert none is None and torch.equal(keys_n, keys)


@pytest.mark.parametrize("Bn,rep,fs", ref.OP_SHAPES[:4])
def test_mask_prompt_embed_without_dense_term_is_repeat_images(Bn, rep, fs):
    """w3 = 0 and b3' = 0: what is left is the image-major broadcast of emb, bit for bit what cvmi_repeat_images writes."""
    lib = _lib.load()
    sd = ref.op_state_dict(_params())
    mask, emb = ref.op_inputs(Bn, rep, fs, sd)
    prm = ref.pack_params(sd)
    prm[332:] = 0
    keys, _, _ = _embed(mask.cuda(), emb.cuda(), prm.cuda(), rep, fs)
    emb_d = emb.cuda()
    want = torch.zeros(Bn * rep, fs * fs, 256, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_repeat_images(emb_d.data_ptr(), want.data_ptr(), fs * fs * 256 * 4, Bn, rep, None), "repeat_images")
    torch.cuda.synchronize()
    assert torch.equal(keys, want) and torch.equal(want.cpu(), emb.repeat_interleave(rep, 0))


def test_mask_prompt_embed_rejects_bad_arguments():
    lib = _lib.load()
    t = torch.zeros(4684 + 64, device="cuda")
    ok = (t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr())
    assert lib.cvmi_mask_prompt_embed(*ok, t.data_ptr(), F32, 1, 1, 1, None) != 0          # the copy must be a 16-bit type
    assert lib.cvmi_mask_prompt_embed(*ok, None, 0, 1, 0, 1, None) != 0
    assert lib.cvmi_mask_prompt_embed(*ok, None, 0, 1, 1, 0, None) != 0
    assert lib.cvmi_mask_prompt_embed(None, *ok[1:], None, 0, 1, 1, 1, None) != 0
    assert lib.cvmi_mask_prompt_embed(t.data_ptr() + 4, *ok[1:], None, 0, 1, 1, 1, None) != 0
    assert b"mask_prompt_embed" in lib.cvmi_last_error()


def test_multimask_out_copies_tokens_1_to_3():
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for n, P0 in ((3, 64 * 64), (2, 37)):                               # the 16-byte path and the scalar one
        masks, iou = torch.randn(n, 4, P0, generator=g).cuda(), torch.rand(n, 4, generator=g).cuda()
        low, iou3 = torch.zeros(n, 3, P0, device="cuda"), torch.zeros(n, 3, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.cvmi_multimask_out(masks.data_ptr(), iou.data_ptr(), 4, low.data_ptr(), iou3.data_ptr(), n, P0, None), "multimask_out")
        torch.cuda.synchronize()
        assert torch.equal(low, masks[:, 1:]) and torch.equal(iou3, iou[:, 1:])


# ---- the model, f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["boxes", "points", "boxes+points"])
def test_infer_masks_mask_input_matches_reference(kind):
    c = ref.mini_inputs(ref.MINI_SEED)
    rhi, rlo, riou = _reference(ref.MINI_SEED, kind, True, False)
    hi, lo, iou = _call(c, kind, mask_input=c["mask"])
    assert hi.shape == (B, P, R, R) and lo.shape == (B, P, F0, F0) and iou.shape == (B, P)
    print(f"mask_input [{kind}] f32: |low_res - reference| = {float((lo.cpu() - rlo[:, :, 0]).abs().max()):.2e}")
    torch.testing.assert_close(lo.cpu(), rlo[:, :, 0], **TOL32)
    torch.testing.assert_close(hi.cpu(), rhi[:, :, 0], **TOL32)
    torch.testing.assert_close(iou.cpu(), riou[:, :, 0], **TOL32)
    _, lo0, _ = _call(c, kind, return_high_res=False)
    assert float((lo - lo0).abs().max()) > 0.1                         # the mask prompt moves the logits
    _, lo_d, _ = _call(c, kind, mask_input=c["mask"].cuda().double(), return_high_res=False)      # a device tensor of another float type
    assert torch.equal(lo_d, lo)


# ---- the plan, F16 ----------------------------------------------------------------------------------------------------------------------
def _labels(sp):
    return [op[0] for op in sp.plan.ops]


def test_mask_prompt_plan_f16_matches_reference_and_replaces_repeat_and_cast(monkeypatch):
    from circuitvision_amd.sam2 import Sam2Plan, Sam2Weights
    seed = ref.REPLAY_SEED
    c = ref.mini_inputs(seed)
    x = c["x"].half().float()
    oracle, sd = _oracle()
    with torch.no_grad():
        rhi, rlo, riou, stab, iou4 = ref.predict_prompts_masked(oracle, sd, x, boxes=c["boxes"], mask_input=c["mask"], margins=True)
    assert ref.selection_is_clear(stab, iou4)
    wt = Sam2Weights(_params(), MINI, R, F16)
    sp = Sam2Plan(wt, B, torch.cuda.Stream(), prompts=P, mask_prompt=True)
    sp.x_in.t.copy_(x.permute(0, 2, 3, 1).half())
    sp.coords[:, :2].copy_(c["boxes"].reshape(B * P, 2, 2))
    sp.labels.copy_(torch.tensor([2, 3, -1], dtype=torch.int32).expand(B * P, 3))
    sp.mask_in.copy_(c["mask"].reshape(B * P, F0, F0))
    torch.cuda.synchronize()
    sp.plan.run_eager()
    torch.cuda.synchronize()
    print(f"mask_input F16 plan: |low_res - reference| = {float((sp.low_res.view(B, P, F0, F0).cpu() - rlo[:, :, 0]).abs().max()):.2e}")
    torch.testing.assert_close(sp.low_res.view(B, P, F0, F0).cpu(), rlo[:, :, 0], **TOL16)
    torch.testing.assert_close(sp.iou.view(B, P).cpu(), riou[:, :, 0], **TOL16)
    torch.testing.assert_close(sp.high_res.view(B, P, R, R).cpu(), rhi[:, :, 0], **TOL16)
    lab = _labels(sp)
    assert "mask_prompt_embed" in lab and "repeat_embed" not in lab and "l0.t2i.castk" not in lab and not sp.share_l0
    assert lab.index("mask_prompt_embed") == lab.index("embed") + 1
    # plans without the flags: the launches they had before (layer-0 sharing on: no repeat pass; off: the repeat pass; the cast in both)
    new = {"mask_prompt_embed", "multimask_out"}
    lists = {}
    for share in ("1", "0"):
        monkeypatch.setenv("CVMI_SAM_SHARE_L0", share)
        lists[share] = _labels(Sam2Plan(wt, B, torch.cuda.Stream(), prompts=P))
        assert not new & set(lists[share]) and "l0.t2i.castk" in lists[share] and "select_mask" in lists[share]
        assert ("repeat_embed" in lists[share]) == (share == "0")
    assert [l for l in lists["0"] if l != "repeat_embed"] == lists["1"]
    # the masked plan is the unshared plan with the one launch in the place of the repeat pass and without layer 0's cast
    assert [l for l in lab if l != "mask_prompt_embed"] == [l for l in lists["0"] if l not in ("repeat_embed", "l0.t2i.castk")]
    with pytest.raises(ValueError):
        Sam2Plan(wt, B, torch.cuda.Stream(), mask_prompt=True)
    with pytest.raises(ValueError):
        Sam2Plan(wt, B, torch.cuda.Stream(), multimask=True)


# ---- multimask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_infer_masks_multimask_matches_reference_tokens_1_to_3(masked):
    c = ref.mini_inputs(ref.MINI_SEED)
    rhi, rlo, riou = _reference(ref.MINI_SEED, "boxes", masked, True)
    kw = dict(mask_input=c["mask"]) if masked else {}
    hi, lo, iou = _call(c, "boxes", multimask_output=True, **kw)
    assert hi.shape == (B, P, 3, R, R) and lo.shape == (B, P, 3, F0, F0) and iou.shape == (B, P, 3)
    torch.testing.assert_close(lo.cpu(), rlo, **TOL32)
    torch.testing.assert_close(hi.cpu(), rhi, **TOL32)
    torch.testing.assert_close(iou.cpu(), riou, **TOL32)
    none, lo2, iou2 = _call(c, "boxes", multimask_output=True, return_high_res=False, **kw)
    assert none is None and torch.equal(lo2, lo) and torch.equal(iou2, iou)
    # the single-mask call runs the same kernels on the same shapes in the same order up to the tail: where it falls back to multimask
    # candidate k (sel = k > 0), its mask IS candidate k - 1, bit for bit
    _, lo1, iou1 = _call(c, "boxes", return_high_res=False, **kw)
    sel = _model().plan(B, prompts=P, high_res=False, points=3, mask_prompt=masked).sel.view(B, P).cpu()
    assert int((sel > 0).sum()) > 0
    for b in range(B):
        for p in range(P):
            k = int(sel[b, p])
            if k > 0:
                assert torch.equal(lo1[b, p], lo[b, p, k - 1]) and torch.equal(iou1[b, p], iou[b, p, k - 1])


# ---- replay ------------------------------------------------------------------------------------------------------------------------------
def test_mask_input_replay_through_the_cached_plan():
    model = _model()
    first = None
    for seed in (ref.MINI_SEED, ref.REPLAY_SEED, ref.MINI_SEED):
        c = ref.mini_inputs(seed)
        rhi, rlo, riou = _reference(seed, "boxes", True, False)
        hi, lo, iou = _call(c, "boxes", mask_input=c["mask"])
        torch.testing.assert_close(lo.cpu(), rlo[:, :, 0], **TOL32)
        torch.testing.assert_close(iou.cpu(), riou[:, :, 0], **TOL32)
        torch.testing.assert_close(hi.cpu(), rhi[:, :, 0], **TOL32)
        if first is None:
            first = (hi, lo, iou)
    assert all(torch.equal(a, b) for a, b in zip(first, (hi, lo, iou)))          # the first call again: bit-identical
    plans = [k for k in model._plans if k[1] == P and k[2] and k[3] == 3 and k[5] and not k[6]]
    assert len(plans) == 1 and model._plans[plans[0]].plan.graph is not None      # one captured plan served all three


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_mask_input_and_multimask_errors():
    from circuitvision_amd.sam2_infer import SAM2Model
    model = _model()
    c = ref.mini_inputs(ref.MINI_SEED)
    x, boxes, mask = c["x"], c["boxes"], c["mask"]
    with pytest.raises(ValueError):
        model.infer_masks(x, mask_input=mask)                          # a mask-only prompt
    with pytest.raises(ValueError):
        model.infer_masks(x, boxes, mask_input=mask[..., :F0 - 1])     # wrong spatial size
    with pytest.raises(ValueError):
        model.infer_masks(x, boxes, mask_input=torch.zeros(B, P, R, R))
    with pytest.raises(ValueError):
        model.infer_masks(x, boxes, mask_input=mask[:, :P - 1])        # P disagrees with the boxes
    with pytest.raises(ValueError):
        model.infer_masks(x, boxes, mask_input=(mask > 0))             # not float logits
    with pytest.raises(NotImplementedError):
        model.infer_masks(x, multimask_output=True)
    p = _params()
    sd = {("sam2_model.base_model.model." + k if not k.startswith(("dense_", "sparse_", "refinement_")) else k): v
          for k, v in {**p.state_dict(), **p.mask_prompt_state_dict()}.items() if "mask_downscaling." not in k}
    stripped = SAM2Model(MINI, R, dtype="f32", use_refinement=True)
    stripped.load_state_dict(sd)
    assert stripped.weights.prompt_ok and not stripped.weights.mask_prompt_ok
    with pytest.raises(RuntimeError, match="mask_downscaling"):
        stripped.infer_masks(x, boxes, mask_input=mask)
    _, lo, _ = stripped.infer_masks(x, boxes, return_high_res=False)   # boxes alone still work, and equal the full checkpoint's
    _, lo_full, _ = model.infer_masks(x, boxes, return_high_res=False)
    assert torch.equal(lo, lo_full)
