"""Embedding reuse and mask feedback on the GPU (`Sam2Plan(stage=)`, `SAM2Model.encode_images`, `infer_masks(Sam2Embeddings, ...)`,
`infer_masks(refine_steps=)`, csrc/mask_prompt.hip best_candidate_kernel, `CircuitPipeline.segment(prompts="both")`) on the mini model of
tests/test_mask_prompt_gpu.py: the kernel through the C ABI against tests/embed_reuse_ref.py bit for bit; decode-from-embeddings against the
one-shot call bit for bit (the same kernels on the same inputs; replays are held bit-identical elsewhere); the plans' launches against the
route; refine_steps against the host loop bit for bit and against the reference predictor's recipe; the pipeline key for key."""
import functools

import pytest
import torch

import embed_reuse_ref as ref
import mask_prompt_ref as mref
import sam2_route_cases as rc
from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from test_mask_prompt_gpu import _params
from test_oracle_sam2_cpu import MINI, mini_oracle

pytestmark = pytest.mark.gpu
R, B, P = 256, 2, 3
F0 = R // 4
TOL32 = dict(rtol=1e-3, atol=1e-3)               # the project's f32 bound
TOL16 = dict(rtol=3e-2, atol=3e-2)               # ... and its 16-bit one
GUARD = 512                                      # elements behind every output the kernel must leave alone
DTYPES = ("f32", "f16", "bf16")


@functools.lru_cache(None)
def _model(dtype="f32"):
    """A model of this file's own (the plan-cache assertions of other files count the plans of theirs)."""
    from circuitvision_amd.sam2_infer import SAM2Model
    return SAM2Model(MINI, R, dtype=dtype, use_refinement=True).load_params(_params())


@functools.lru_cache(None)
def _embeddings(dtype, seed):
    return _model(dtype).encode_images(mref.mini_inputs(seed)["x"])


@functools.lru_cache(None)
def _oracle():
    _model()                                                          # (the packed model has read every tensor the oracle loads)
    p = _params()
    return mini_oracle(p, R), {**p.state_dict(), **p.mask_prompt_state_dict()}


def _same(a, b):
    """torch.equal on every output of two infer_masks results: tensors, lists of tensors, or None."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. the kernel through the C ABI -------------------------------------------------------------------------------------------------------
def _best(low_d, iou_d, NM, n, P0, with_sel=True):
    """-> (mask [n, P0], sel [n] or None, tag); both outputs carry a -7 guard band that must come back untouched."""
    lib = _lib.load()
    mask = torch.full((n * P0 + GUARD,), -7.0, device="cuda")
    sel = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") if with_sel else None
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _lib.check(lib.cvmi_best_candidate(low_d.data_ptr(), iou_d.data_ptr(), NM, mask.data_ptr(), sel.data_ptr() if with_sel else None, n, P0, None),
               "best_candidate")
    tag = lib.cvmi_last_kernel().decode()
    torch.cuda.synchronize()
    assert bool((mask[n * P0:] == -7.0).all()) and (sel is None or bool((sel[n:] == -7).all())), "wrote past the end"
    return mask[:n * P0].view(n, P0), (sel[:n] if with_sel else None), tag


@pytest.mark.parametrize("NM", [1, 3])
@pytest.mark.parametrize("P0", [4, 64 * 64])
@pytest.mark.parametrize("n", [1, 33])
def test_best_candidate_matches_reference_bit_for_bit(n, P0, NM):
    low, iou = ref.candidate_inputs(n, NM, P0)
    want_mask, want_sel = ref.best_candidate(low, iou)
    low_d, iou_d = low.cuda(), iou.cuda()
    mask, sel, tag = _best(low_d, iou_d, NM, n, P0)
    assert tag == f"best_candidate_kernel<{NM}>"
    assert torch.equal(sel.cpu(), want_sel) and torch.equal(mask.cpu(), want_mask)
    if NM == 1:
        assert not sel.any() and torch.equal(mask, low_d[:, 0])      # a copy
    mask_n, none, _ = _best(low_d, iou_d, NM, n, P0, with_sel=False)  # sel_out = NULL
    assert none is None and torch.equal(mask_n, mask)
    mask_2, sel_2, _ = _best(low_d, iou_d, NM, n, P0)                 # a second run repeats the first
    assert torch.equal(mask_2, mask) and torch.equal(sel_2, sel)


def test_best_candidate_rejects_bad_arguments_and_skips_an_empty_batch():
    lib = _lib.load()
    t = torch.zeros(3 * 64 + 64, device="cuda")
    s = torch.zeros(8, dtype=torch.int32, device="cuda")
    call = lambda low, iou, NM, out, n, P0: _lib.check(lib.cvmi_best_candidate(low, iou, NM, out, s.data_ptr(), n, P0, None), "best_candidate")
    ptr = t.data_ptr()
    for args in ((ptr, ptr, 3, ptr, 1, 6), (ptr, ptr, 2, ptr, 1, 4), (ptr, ptr, 0, ptr, 1, 4), (ptr + 4, ptr, 3, ptr, 1, 4), (ptr, ptr + 4, 3, ptr, 1, 4),
                 (ptr, ptr, 3, ptr + 8, 1, 4), (ptr, ptr, 3, ptr, 1, 0), (ptr, ptr, 3, ptr, -1, 4), (None, ptr, 3, ptr, 1, 4)):
        with pytest.raises(_lib.CvmiError, match="best_candidate"):
            call(*args)
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    out = torch.full((16,), -7.0, device="cuda")
    call(ptr, ptr, 3, out.data_ptr(), 0, 4)                             # n = 0: no launch
    assert lib.cvmi_last_kernel().decode() == ""
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- 2. decode from embeddings == the one-shot call ----------------------------------------------------------------------------------------
def _lists(c):
    """[2 boxes, 0 boxes]: an image without a prompt."""
    return [c["boxes"][0, :2], torch.zeros(0, 4)]


CASES = {
    "no_prompt": lambda c: dict(),
    "boxes": lambda c: dict(boxes=c["boxes"]),
    "boxes+clicks": lambda c: dict(boxes=c["boxes"], points=c["points"], point_labels=c["labels"]),
    "mask_input": lambda c: dict(boxes=c["boxes"], mask_input=c["mask"]),
    "multimask": lambda c: dict(boxes=c["boxes"], multimask_output=True),
    "lists_with_an_empty_image": lambda c: dict(boxes=_lists(c)),
    "lists_mask_multimask": lambda c: dict(boxes=_lists(c), mask_input=[c["mask"][0, :2], c["mask"][1, :0]], multimask_output=True),
    "low_res_only": lambda c: dict(boxes=c["boxes"], return_high_res=False),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_infer_masks_from_embeddings_equals_the_one_shot_call(dtype, case):
    model, c = _model(dtype), mref.mini_inputs(mref.MINI_SEED)
    kw = CASES[case](c)
    want = model.infer_masks(c["x"], **kw)
    got = model.infer_masks(_embeddings(dtype, mref.MINI_SEED), **kw)
    assert len(got) == 3 and all(_same(g, w) for g, w in zip(got, want))
    assert torch.isfinite(torch.cat(got[1]) if isinstance(got[1], list) else got[1]).all()
    again = model.infer_masks(model.encode_images(c["x"]), **kw)       # a fresh encode, a replayed decode plan
    assert all(_same(g, w) for g, w in zip(again, want))


def test_embeddings_are_a_plain_container_of_the_seam_tensors():
    model = _model("f16")
    e = _embeddings("f16", mref.MINI_SEED)
    assert len(e) == B and e.image_size == R and e.dtype == F16 and e.weights_id == model.weights_id
    assert e.feat_s0.shape == (B, F0, F0, 32) and e.feat_s0.dtype == torch.float16 and e.feat_s1.shape == (B, F0 // 2, F0 // 2, 64)
    assert e.emb.shape == e.dense.shape == (B, R // 16, R // 16, 256) and e.emb.dtype == e.dense.dtype == torch.float32
    assert e.nbytes == sum(t.numel() * t.element_size() for t in (e.feat_s0, e.feat_s1, e.emb, e.dense))
    with pytest.raises(ValueError):
        model.encode_images(torch.zeros(B, 3, R, R // 2))
    with pytest.raises(ValueError, match="other weights"):
        _model("f32").infer_masks(e)                                    # another model's embeddings
    with pytest.raises(ValueError, match="on the device"):
        model.infer_masks(e._like(lambda t: t.cpu()))
    with pytest.raises(ValueError):
        model.infer_masks(e, boxes=mref.mini_inputs(mref.MINI_SEED)["boxes"][:1])      # the same validation: B disagrees


# ---- 3. embeddings do not alias plan buffers -------------------------------------------------------------------------------------------------
def test_embeddings_survive_later_calls_and_batch_across_encodes():
    from circuitvision_amd.sam2_infer import Sam2Embeddings
    model = _model("f32")
    c1, c2 = mref.mini_inputs(mref.MINI_SEED), mref.mini_inputs(mref.REPLAY_SEED)
    kw = dict(boxes=c1["boxes"])
    want1 = model.infer_masks(c1["x"], **kw)
    e1 = model.encode_images(c1["x"])
    e2 = model.encode_images(c2["x"])                                   # the encode plan's buffers now hold x2,
    want2 = model.infer_masks(c2["x"], **kw)                            # and so do the full plan's
    got1, got2 = model.infer_masks(e1, **kw), model.infer_masks(e2, **kw)
    assert all(_same(g, w) for g, w in zip(got1, want1)) and all(_same(g, w) for g, w in zip(got2, want2))
    assert not torch.equal(got1[1], got2[1])
    for a, b in zip(model.infer_masks(e1), model(c1["x"])):            # the learned-prompt decode too
        assert torch.equal(a, b)
    # a batch out of cached images: row 0 is image 1 of x1, row 1 image 0 of x2 (per-image independence of the whole pass is pinned by
    # test_sam2_hiera_l_baseline_size_permutation_and_replay_properties)
    mixed = model.infer_masks(Sam2Embeddings.cat([e1[1:2], e2[0:1]]), boxes=c1["boxes"][[1, 0]])      # (each image with the boxes it had)
    for m, a, b in zip(mixed, got1, got2):
        assert torch.equal(m[0], a[1]) and torch.equal(m[1], b[0])
    mixed0 = model.infer_masks(Sam2Embeddings.cat([e1[1], e2[0]]))
    for m, a, b in zip(mixed0, model.infer_masks(e1), model.infer_masks(e2)):
        assert torch.equal(m[0], a[1]) and torch.equal(m[1], b[0])


# ---- 4. the plans -----------------------------------------------------------------------------------------------------------------------------
def _ops(sp):
    return [(op[0], op[1]) for op in sp.plan.ops]


@functools.lru_cache(None)
def _weights(dtype):
    from circuitvision_amd.sam2 import Sam2Weights
    return Sam2Weights(_params(), MINI, R, dtype)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_encode_plan_is_the_trunk_the_neck_and_both_embeds(dtype):
    from circuitvision_amd.sam2 import Sam2Plan
    wt = _weights(dtype)
    sp = Sam2Plan(wt, B, torch.cuda.Stream(), stage="encode")
    full = Sam2Plan(wt, B, torch.cuda.Stream())
    ops = _ops(sp)
    head = [op for op in ops if not rc.BLOCK_LABEL.fullmatch(op[0])]
    assert [list(op) for op in head[:2]] == rc.STEM
    assert head[2:] == sp.droute.neck_launches() + [("embed_box", "neck")] and ops[-len(head) + 2:] == head[2:]
    assert [op for op in ops if rc.BLOCK_LABEL.fullmatch(op[0])] == [op for op in _ops(full) if rc.BLOCK_LABEL.fullmatch(op[0])]
    assert sp.droute.neck_launches() == full.droute.neck_launches()
    assert sp.emb.t.shape == sp.keys0.t.shape == (B, R // 16, R // 16, 256) and sp.emb.t.data_ptr() != sp.keys0.t.data_ptr()
    for kw in (dict(prompts=2), dict(pairs=3), dict(prompts=2, multimask=True)):
        with pytest.raises(ValueError):
            Sam2Plan(wt, B, torch.cuda.Stream(), stage="encode", **kw)
    with pytest.raises(ValueError):
        Sam2Plan(wt, B, torch.cuda.Stream(), stage="half")


ROUTES = [("learned", {}, {}), ("prompts", dict(prompts=P), {}), ("prompts_unshared", dict(prompts=P), {"CVMI_SAM_SHARE_L0": "0"}),
          ("mask_prompt", dict(prompts=P, mask_prompt=True), {}), ("multimask_low_res", dict(prompts=P, multimask=True, high_res=False), {}),
          ("pairs", dict(pairs=32), {}), ("pairs_unshared", dict(pairs=32), {"CVMI_SAM_SHARE_L0": "0"}), ("pairs_mask", dict(pairs=32, mask_prompt=True), {})]


@pytest.mark.parametrize("name,kw,env", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("dtype", [F16, F32])
def test_decode_plan_is_exactly_the_decoder_launches(dtype, name, kw, env, monkeypatch):
    from circuitvision_amd.sam2 import Sam2Plan
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wt = _weights(dtype)
    sp = Sam2Plan(wt, B, torch.cuda.Stream(), stage="decode", **kw)
    assert _ops(sp) == sp.droute.decoder_launches()
    assert not any(rc.BLOCK_LABEL.fullmatch(l) or l in ("s2d4", "patch_embed", "embed") or l.startswith(("feat_s", "cast.s")) for l, _ in _ops(sp))
    assert getattr(sp, "x_in", None) is None and not hasattr(sp, "stage_out")
    assert sp.feat_s0.t.shape == (B, F0, F0, 32) and sp.feat_s1.t.shape == (B, F0 // 2, F0 // 2, 64)
    assert sp.feat_s0.t.dtype == sp.feat_s1.t.dtype == {F16: torch.float16, F32: torch.float32}[dtype]
    seam = sp.emb if sp.droute.prompted else sp.keys0
    assert seam.t.shape == (B, R // 16, R // 16, 256) and seam.t.dtype == torch.float32
    assert (sp.emb is None) == (not sp.droute.prompted)
    streams = {"learned": "dense", "prompts": "shared" if dtype == F16 else "repeat", "prompts_unshared": "repeat", "mask_prompt": "mask_prompt",
               "multimask_low_res": "shared" if dtype == F16 else "repeat", "pairs": "shared" if dtype == F16 else "gather", "pairs_unshared": "gather",
               "pairs_mask": "mask_prompt"}
    assert sp.droute.stream == streams[name]
    torch.cuda.synchronize()
    sp.plan.run_eager()                                                 # on its zero inputs
    torch.cuda.synchronize()
    assert torch.isfinite(sp.low_res).all()


def test_model_caches_stage_plans_beside_the_full_ones():
    model, c = _model("f16"), mref.mini_inputs(mref.MINI_SEED)
    e = _embeddings("f16", mref.MINI_SEED)
    model.infer_masks(c["x"], boxes=c["boxes"]), model.infer_masks(e, boxes=c["boxes"]), model.infer_masks(e, boxes=c["boxes"])
    keys = [k for k in model._plans if k[:4] == (B, P, True, 3) and not k[5] and not k[6]]
    assert sorted(len(k) for k in keys) == [8, 9] and [k[8] for k in keys if len(k) == 9] == ["decode"]
    assert sum(1 for k in model._plans if k[-1] == "encode") == 1
    assert all(model._plans[k].plan.graph is not None for k in keys)


# ---- 5. refine_steps ----------------------------------------------------------------------------------------------------------------------------
def _pick(lo, iou):
    """The best candidate of every pair, on the host side with torch: tensors [B,P,(3,)...] or lists of [P_b,(3,)...]."""
    if isinstance(lo, list):
        return [_pick(l, i) for l, i in zip(lo, iou)]
    if lo.dim() == iou.dim() + 2 and iou.shape[-1] == 3 and lo.shape[-3] == 3:
        idx = torch.argmax(iou, -1)[..., None, None, None].expand(*iou.shape[:-1], 1, F0, F0)
        return torch.gather(lo, -3, idx).squeeze(-3)
    return lo


def _host_loop(model, e, kw, multimask, steps, return_high_res=True):
    hi, lo, iou = model.infer_masks(e, multimask_output=multimask, return_high_res=False, **kw)
    for i in range(steps):
        picked = _pick(lo, iou) if multimask and i == 0 else lo
        hi, lo, iou = model.infer_masks(e, mask_input=picked, return_high_res=return_high_res and i == steps - 1, **kw)
    return hi, lo, iou


@pytest.mark.parametrize("form", ["tensor", "lists"])
@pytest.mark.parametrize("source", ["images", "embeddings"])
@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("steps", [1, 2])
def test_refine_steps_equal_the_host_loop(steps, multimask, source, form):
    model, c = _model("f32"), mref.mini_inputs(mref.MINI_SEED)
    e = _embeddings("f32", mref.MINI_SEED)
    kw = dict(boxes=c["boxes"]) if form == "tensor" else dict(boxes=_lists(c))
    want = _host_loop(model, e, kw, multimask, steps)
    got = model.infer_masks(c["x"] if source == "images" else e, multimask_output=multimask, refine_steps=steps, **kw)
    assert all(_same(g, w) for g, w in zip(got, want))
    if form == "tensor":
        assert got[0].shape == (B, P, R, R) and got[1].shape == (B, P, F0, F0) and got[2].shape == (B, P)
    else:
        assert [t.shape for t in got[1]] == [(2, F0, F0), (0, F0, F0)] and [t.shape for t in got[2]] == [(2,), (0,)]
    _, lo0, _ = model.infer_masks(e, return_high_res=False, **kw)
    assert not _same(lo0, got[1])                                       # the feedback moved the logits
    none, lo_only, iou_only = model.infer_masks(e, multimask_output=multimask, refine_steps=steps, return_high_res=False, **kw)
    assert none is None and _same(lo_only, got[1]) and _same(iou_only, got[2])


def test_refine_steps_zero_is_the_plain_call_and_clicks_and_a_first_mask_pass_through():
    model, c = _model("f32"), mref.mini_inputs(mref.MINI_SEED)
    e = _embeddings("f32", mref.MINI_SEED)
    kw = dict(boxes=c["boxes"], points=c["points"], point_labels=c["labels"])
    assert all(_same(g, w) for g, w in zip(model.infer_masks(c["x"], refine_steps=0, **kw), model.infer_masks(c["x"], **kw)))
    got = model.infer_masks(c["x"], mask_input=c["mask"], refine_steps=1, **kw)        # pass 1 with a mask prompt of its own
    _, lo1, _ = model.infer_masks(e, mask_input=c["mask"], return_high_res=False, **kw)
    want = model.infer_masks(e, mask_input=lo1, **kw)
    assert all(_same(g, w) for g, w in zip(got, want))


@functools.lru_cache(None)
def _recipe(seed, multimask, half):
    oracle, sd = _oracle()
    c = mref.mini_inputs(seed)
    out, clear = ref.refine_recipe(oracle, sd, c["x"].half().float() if half else c["x"], c["boxes"], multimask)
    assert clear, (seed, multimask, half)                               # the precondition (tests/test_embed_reuse_cpu.py holds the seeds to it)
    return out


@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("seed", ref.REFINE_SEEDS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_refine_steps_match_the_reference_recipe(dtype, seed, multimask):
    c = mref.mini_inputs(seed)
    rhi, rlo, riou = _recipe(seed, multimask, dtype == "f16")
    hi, lo, iou = _model(dtype).infer_masks(c["x"], boxes=c["boxes"], multimask_output=multimask, refine_steps=1)
    print(f"refine_steps=1 {dtype} seed {seed} multimask={multimask}: |low_res - reference| = {float((lo.cpu() - rlo).abs().max()):.2e}, "
          f"|iou - reference| = {float((iou.cpu() - riou).abs().max()):.2e}")
    tol = TOL32 if dtype == "f32" else TOL16
    torch.testing.assert_close(lo.cpu(), rlo, **tol)
    torch.testing.assert_close(iou.cpu(), riou, **tol)
    torch.testing.assert_close(hi.cpu(), rhi, **tol)


def test_refine_steps_errors():
    from circuitvision_amd.sam2_infer import SAM2Model
    model, c = _model("f32"), mref.mini_inputs(mref.MINI_SEED)
    x, boxes = c["x"], c["boxes"]
    with pytest.raises(ValueError):
        model.infer_masks(x, refine_steps=1)                            # no prompt
    with pytest.raises(ValueError):
        model.infer_masks(_embeddings("f32", mref.MINI_SEED), refine_steps=1)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="refine_steps"):
            model.infer_masks(x, boxes, refine_steps=bad)
    with pytest.raises(ValueError, match="refine_steps"):
        model.infer_masks(x, _lists(c), refine_steps=-2)
    p = _params()
    sd = {("sam2_model.base_model.model." + k if not k.startswith(("dense_", "sparse_", "refinement_")) else k): v
          for k, v in {**p.state_dict(), **p.mask_prompt_state_dict()}.items() if "mask_downscaling." not in k}
    stripped = SAM2Model(MINI, R, dtype="f32", use_refinement=True)
    stripped.load_state_dict(sd)
    assert stripped.weights.prompt_ok and not stripped.weights.mask_prompt_ok
    with pytest.raises(RuntimeError, match="mask_downscaling"):
        stripped.infer_masks(x, boxes, refine_steps=1)
    with pytest.raises(RuntimeError, match="mask_downscaling"):
        stripped.infer_masks(x, _lists(c), refine_steps=1)
    _, lo, _ = stripped.infer_masks(stripped.encode_images(x), boxes, return_high_res=False)      # decode without the mask stack still works
    _, lo_full, _ = model.infer_masks(x, boxes, return_high_res=False)
    assert torch.equal(lo, lo_full)


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_prompts", [2, None])
def test_pipeline_both_carries_learned_and_boxes(max_prompts):
    from circuitvision_amd.pipeline import CircuitPipeline
    from circuitvision_amd.sam2_infer import SAM2Transforms
    from synth import circuit_image
    seg = _model("f32")
    tr = SAM2Transforms(resolution=R, mask_threshold=0, max_hole_area=0, max_sprinkle_area=0)
    images = [circuit_image(300, 420, seed=300), circuit_image(240, 320, seed=301)]           # two sizes
    box = lambda x0, y0, x1, y1: dict(xmin=x0, ymin=y0, xmax=x1, ymax=y1, class_name="resistor", confidence=0.9)
    bboxes = [[box(30, 40, 200, 160), box(220, 60, 400, 280), box(10, 200, 120, 290)], []]      # ... one of them without a box
    pipe = CircuitPipeline(None, seg, tr, max_prompts=max_prompts)
    learned, boxes, both = (pipe.segment(images, bboxes, m) for m in ("learned", "boxes", "both"))
    same = lambda a, b: torch.equal(a, b) if torch.is_tensor(a) else a == b
    for rl, rb, r in zip(learned, boxes, both):
        assert set(r) == set(rl) | {"masks", "extents", "box_iou"}
        for k in ("mask", "extent", "iou", "bboxes", "crop_debug_info"):
            assert same(r[k], rl[k]), k
        assert r["image"] is rl["image"]
        for k, kb in (("masks", "masks"), ("extents", "extents"), ("box_iou", "iou")):
            assert same(r[k], rb[kb]), k
    n0 = 3 if max_prompts is None else 2
    assert both[0]["masks"].shape == (n0, 300, 420) and both[1]["masks"].shape == (0, 240, 320) and both[0]["mask"].shape == (300, 420)
    assert int((both[0]["masks"] > 0).sum()) > 0
    with pytest.raises(ValueError):
        pipe.segment(images, bboxes, "neither")
    with pytest.raises(ValueError, match="nodes=True needs"):
        CircuitPipeline(None, seg, tr, nodes=True).run_batch(images, "boxes")
