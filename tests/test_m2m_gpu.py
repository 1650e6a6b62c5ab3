"""The mask-to-mask pass on the GPU (csrc/mask_prompt.hip m2m_fanout_kernel, `infer_masks(m2m=True)`, `generate(use_m2m=True)`) on the mini
model of tests/test_mask_prompt_gpu.py: the fan-out through the C ABI against tests/m2m_ref.py bit for bit; `infer_masks(m2m=True)` against the
two-call composition through the host bit for bit and against the reference predictor at the mask-prompt pass's bound; the generator against a
host loop whose chunks are that composition, alone and with the other per-call options."""
import functools

import numpy as np
import pytest
import torch

import amg_crop_ref as cref
import amg_ref
import m2m_ref as ref
import mask_prompt_ref as mref
from circuitvision_amd import _lib
from test_amg_gpu import F0, GUARD, R, SIZES, _images
from test_amg_gpu import _host_loop as _plain_host_loop
from test_amg_gpu import _model as _amg_model
from test_mask_prompt_gpu import TOL32, _oracle, _params
from test_oracle_sam2_cpu import MINI

pytestmark = pytest.mark.gpu
B, P = 2, 3
C32 = ref.UPSTREAM_CLAMP


@functools.lru_cache(None)
def _model(dtype="f32"):
    """A model of this file's own (the plan-cache assertions of other files count the plans of theirs)."""
    from circuitvision_amd.sam2_infer import SAM2Model
    return SAM2Model(MINI, R, dtype=dtype, use_refinement=True).load_params(_params())


@functools.lru_cache(None)
def _embeddings(dtype, seed):
    return _model(dtype).encode_images(mref.mini_inputs(seed)["x"])


def _same(a, b):
    """torch.equal on every output of two infer_masks results: tensors, lists of tensors, or None."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. the kernel through the C ABI -------------------------------------------------------------------------------------------------------
def _fanout(low, c, coords, labels, pair_image):
    """cvmi_m2m_fanout on outputs pre-filled with -7 and a guard band behind each -> ((mask, coords, labels, pair_image or None) as numpy, tag)."""
    lib = _lib.load()
    n, NM, Pl = low.shape
    K = coords.shape[1]
    src = [torch.from_numpy(a).cuda() if a is not None else None for a in (low, coords, labels, pair_image)]
    sizes = (n * NM * Pl, n * NM * K * 2, n * NM * K, n * NM)
    outs = [torch.full((sizes[0] + GUARD,), -7.0, device="cuda"), torch.full((sizes[1] + GUARD,), -7.0, device="cuda"),
            torch.full((sizes[2] + GUARD,), -7, dtype=torch.int32, device="cuda"),
            torch.full((sizes[3] + GUARD,), -7, dtype=torch.int32, device="cuda") if pair_image is not None else None]
    ptr = lambda t: t.data_ptr() if t is not None else None
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _lib.check(lib.cvmi_m2m_fanout(ptr(src[0]), NM, c, ptr(outs[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), n, Pl, K, None),
               "m2m_fanout")
    tag = lib.cvmi_last_kernel().decode()
    torch.cuda.synchronize()
    for t, s in zip(outs, sizes):
        assert t is None or bool((t[s:] == -7).all()), "wrote past the end"
    shapes = ((n * NM, Pl), (n * NM, K, 2), (n * NM, K), (n * NM,))
    return tuple(t[:s].view(*shp).cpu().numpy() if t is not None else None for t, s, shp in zip(outs, sizes, shapes)), tag


@pytest.mark.parametrize("c", (C32, 0.75))
@pytest.mark.parametrize("row", ref.ROWS, ids=lambda r: "n%d_nm%d_p%d_k%d" % r)
def test_fanout_matches_reference_bit_for_bit(row, c):
    """The last row is longer than one pass of the grid-stride loop at the grid cap (m2m_ref.GRID_PASS_FLOATS = 64 workgroups x 256 threads x 4
    floats per pair; tests/test_m2m_ref_cpu.py holds the figure to the kernel's constants).  Every row holds +-c, the next floats beyond them, +-inf, NaN
    and -0.0; the comparison is through the int32 view; with and without the pair table; twice."""
    n, NM, Pl, K = row
    low, coords, labels, pair_image = ref.fanout_inputs(n, NM, Pl, K, c)
    for table in (pair_image, None):
        want = ref.fanout(low, c, coords, labels, table)
        got, tag = _fanout(low, c, coords, labels, table)
        assert tag == f"m2m_fanout_kernel<{NM}>"
        assert ref.same_fanout(got, want), (row, c, table is not None, [g is None or ref.same_bits(g, w) for g, w in zip(got, want)])
        again, _ = _fanout(low, c, coords, labels, table)
        assert ref.same_fanout(again, got)
    assert np.isnan(got[0]).any() and (np.signbit(got[0]) & (got[0] == 0)).any() and float(np.nanmax(np.abs(got[0]))) == c


def test_fanout_rejects_bad_arguments_and_skips_an_empty_batch():
    lib = _lib.load()
    t = torch.zeros(3 * 64 + 64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((3 * 64 + 64,), -7.0, device="cuda")
    iout = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    cout, pout = torch.full((64,), -7.0, device="cuda"), torch.full((64,), -7, dtype=torch.int32, device="cuda")
    ok = dict(low=t.data_ptr(), NM=3, c=32.0, mask=out.data_ptr(), coords=t.data_ptr(), labels=i.data_ptr(), pi=i.data_ptr(), co=cout.data_ptr(), lo=iout.data_ptr(),
              po=pout.data_ptr(), n=1, P=4, K=1)
    call = lambda **kw: (lambda a: lib.cvmi_m2m_fanout(a["low"], a["NM"], a["c"], a["mask"], a["coords"], a["labels"], a["pi"], a["co"], a["lo"], a["po"], a["n"], a["P"],
                                                       a["K"], None))({**ok, **kw})
    bad = (dict(NM=2), dict(NM=0), dict(NM=4), dict(P=6), dict(P=0), dict(P=-4), dict(low=t.data_ptr() + 4), dict(mask=out.data_ptr() + 8),
           dict(coords=t.data_ptr() + 2), dict(labels=i.data_ptr() + 1), dict(pi=i.data_ptr() + 2), dict(co=cout.data_ptr() + 2), dict(lo=iout.data_ptr() + 2),
           dict(po=pout.data_ptr() + 2), dict(low=None), dict(mask=None), dict(coords=None), dict(labels=None), dict(co=None), dict(lo=None),
           dict(pi=None), dict(po=None), dict(n=-1), dict(n=65536), dict(K=0), dict(c=-1.0), dict(c=float("nan")))
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"m2m_fanout" in lib.cvmi_last_error(), kw
    assert call(n=65536) != 0 and b"65535" in lib.cvmi_last_error()              # the pair count the grid can address is stated
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    assert call(n=0) == 0 and call(n=0, pi=None, po=None) == 0                   # n = 0: no launch
    assert lib.cvmi_last_kernel().decode() == ""
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (out, cout, iout, pout))
    assert call() == 0 and call(pi=None, po=None) == 0                           # the good call, with and without the pair table
    torch.cuda.synchronize()
    assert bool((out[:12] == 0).all()) and bool((out[12:] == -7.0).all()) and bool((cout[:6] == 0).all()) and bool((cout[6:] == -7.0).all())
    assert bool((iout[:3] == 0).all()) and bool((iout[3:] == -7).all()) and bool((pout[:3] == 0).all()) and bool((pout[3:] == -7).all())


# ---- 2. infer_masks(m2m=True) == the two-call composition through the host ----------------------------------------------------------------------------
def _rep(v, NM):
    """A prompt argument with every prompt repeated NM times in place: tensors [B, P, ...] or lists of [P_b, ...]."""
    return [t.repeat_interleave(NM, 0) for t in v] if isinstance(v, (list, tuple)) else torch.as_tensor(v).repeat_interleave(NM, 1)


def _compose(infer, e, kw, multimask, c=C32, return_high_res=True):
    """What a caller could do before, with infer = a model's `infer_masks`: pass 1, torch.clamp on the host side, pass 2 with every candidate as
    a prompt of its own.  -> ((high_res, low_res, iou) in pass 1's shapes, pass 1's low_res)."""
    NM = 3 if multimask else 1
    _, lo1, _ = infer(e, multimask_output=multimask, return_high_res=False, **kw)
    prompts = {k: _rep(v, NM) for k, v in kw.items() if k != "mask_input"}
    if isinstance(lo1, list):
        mask = [torch.clamp(t, -c, c).reshape(-1, F0, F0) for t in lo1]
        out = infer(e, mask_input=mask, return_high_res=return_high_res, **prompts)
        if NM == 3:
            out = tuple([t.view(t.shape[0] // 3, 3, *t.shape[1:]) for t in o] if o is not None else None for o in out)
    else:
        out = infer(e, mask_input=torch.clamp(lo1, -c, c).reshape(lo1.shape[0], -1, F0, F0), return_high_res=return_high_res, **prompts)
        if NM == 3:
            out = tuple(o.view(o.shape[0], o.shape[1] // 3, 3, *o.shape[2:]) if o is not None else None for o in out)
    return out, lo1


def _lists(c):
    """[2 prompts, 0 prompts]: an image without a prompt."""
    return dict(boxes=[c["boxes"][0, :2], torch.zeros(0, 4)], points=[c["points"][0, :2], torch.zeros(0, 2, 2)],
                point_labels=[c["labels"][0, :2], torch.zeros(0, 2, dtype=torch.long)])


CASES = {
    "points": (lambda c: dict(points=c["points"], point_labels=c["labels"]), True),
    "boxes+points": (lambda c: dict(boxes=c["boxes"], points=c["points"], point_labels=c["labels"]), True),
    "lists_with_an_empty_image": (_lists, True),
    "single_mask": (lambda c: dict(boxes=c["boxes"]), False),
    "lists_single_mask": (lambda c: dict(boxes=_lists(c)["boxes"]), False),
    "mask_input_on_pass_1": (lambda c: dict(boxes=c["boxes"], mask_input=c["mask"]), True),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_m2m_equals_the_host_composition(dtype, case):
    """torch.equal on low_res, iou and high_res, from embeddings and from images, and again on a replay of the cached plans after another input."""
    model = _model(dtype)
    make, multimask = CASES[case]
    first = None
    for seed in (mref.MINI_SEED, mref.REPLAY_SEED, mref.MINI_SEED):
        c, e = mref.mini_inputs(seed), _embeddings(dtype, seed)
        kw = make(c)
        want, lo1 = _compose(model.infer_masks, e, kw, multimask)
        got = model.infer_masks(e, multimask_output=multimask, m2m=True, **kw)
        assert len(got) == 3 and all(_same(g, w) for g, w in zip(got, want)), (dtype, case, seed)
        assert not _same(got[1], lo1)                                   # the second pass moved the logits
        if first is None:
            first = got
            from_images = model.infer_masks(c["x"], multimask_output=multimask, m2m=True, **kw)
            assert all(_same(g, w) for g, w in zip(from_images, want))
            none, lo_only, iou_only = model.infer_masks(e, multimask_output=multimask, m2m=True, return_high_res=False, **kw)
            assert none is None and _same(lo_only, got[1]) and _same(iou_only, got[2])
    assert all(_same(a, b) for a, b in zip(first, got))                 # the first input again: bit-identical
    NM = (3,) if multimask else ()
    if isinstance(got[1], list):
        assert [tuple(t.shape) for t in got[1]] == [(2, *NM, F0, F0), (0, *NM, F0, F0)] and [tuple(t.shape) for t in got[2]] == [(2, *NM), (0, *NM)]
        assert [tuple(t.shape) for t in got[0]] == [(2, *NM, R, R), (0, *NM, R, R)]
    else:
        assert got[0].shape == (B, P, *NM, R, R) and got[1].shape == (B, P, *NM, F0, F0) and got[2].shape == (B, P, *NM)
    assert torch.isfinite(torch.cat(got[1]) if isinstance(got[1], list) else got[1]).all()


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_m2m_clamp_bites_at_the_median_logit(dtype):
    """m2m_clamp = the median of |low_res| of the first pass: some logits lie above it and some below (asserted on the reference side), so a missing
    or misplaced clamp cannot equal the composition."""
    model, c, e = _model(dtype), mref.mini_inputs(mref.MINI_SEED), _embeddings(dtype, mref.MINI_SEED)
    kw = dict(points=c["points"], point_labels=c["labels"])
    _, lo1, _ = model.infer_masks(e, multimask_output=True, return_high_res=False, **kw)
    bound = float(lo1.abs().median())
    above, below = int((lo1.abs() > bound).sum()), int((lo1.abs() < bound).sum())
    print(f"[m2m {dtype}] |low_res| of pass 1: median {bound:.4f}, max {float(lo1.abs().max()):.4f}; {above} logits above the bound, {below} below")
    assert above > 0 and below > 0 and bound > 0 and float(lo1.abs().max()) < C32
    want, _ = _compose(model.infer_masks, e, kw, True, c=bound)
    got = model.infer_masks(e, multimask_output=True, m2m=True, m2m_clamp=bound, **kw)
    assert all(_same(g, w) for g, w in zip(got, want))
    unclamped = model.infer_masks(e, multimask_output=True, m2m=True, **kw)           # no logit reaches 32: the pass without a clamp
    assert not _same(unclamped[1], got[1])
    assert all(_same(g, w) for g, w in zip(unclamped, _compose(model.infer_masks, e, kw, True)[0]))


# ---- 3. against the reference predictor ------------------------------------------------------------------------------------------------------------------
# REPLAY_SEED: on the reference, fed its own clamped first pass, every one of the 18 pairs of both prompt kinds selects clearly (two best IoU
# predictions >= 0.017 apart, stabilities >= 0.3 from the threshold); MINI_SEED's click prompts do not
ORACLE_CASES = (("boxes", mref.REPLAY_SEED), ("points", mref.REPLAY_SEED))


@pytest.mark.parametrize("kind,seed", ORACLE_CASES)
def test_m2m_matches_the_reference_fed_the_clamped_first_pass(kind, seed):
    """The reference's mask-prompted single-mask decode (mask_prompt_ref.predict_prompts_masked, as test_mask_prompt_gpu._reference drives it with
    masked=True, multimask=False; that helper takes its mask from mini_inputs, so the call is restated here) on the GPU's own clamped first-pass
    logits, every candidate a prompt: the refined output agrees at the bound of test_infer_masks_mask_input_matches_reference (TOL32, imported)."""
    model, c = _model("f32"), mref.mini_inputs(seed)
    kw = dict(boxes=c["boxes"]) if kind == "boxes" else dict(points=c["points"], point_labels=c["labels"])
    _, lo1, _ = model.infer_masks(c["x"], multimask_output=True, return_high_res=False, **kw)
    mask = torch.clamp(lo1, -C32, C32).reshape(B, P * 3, F0, F0).cpu()
    oracle, sd = _oracle()
    okw = dict(boxes=c["boxes"].repeat_interleave(3, 1)) if kind == "boxes" else dict(points=c["points"].repeat_interleave(3, 1),
                                                                                         labels=c["labels"].repeat_interleave(3, 1))
    with torch.no_grad():
        rhi, rlo, riou, stab, iou4 = mref.predict_prompts_masked(oracle, sd, c["x"], mask_input=mask, multimask_output=False, margins=True, **okw)
    assert mref.selection_is_clear(stab, iou4), (kind, seed)            # the precondition of every single-mask comparison
    hi, lo, iou = model.infer_masks(c["x"], multimask_output=True, m2m=True, **kw)
    print(f"m2m [{kind}] f32: |low_res - reference| = {float((lo.cpu().reshape(B, P * 3, F0, F0) - rlo[:, :, 0]).abs().max()):.2e}, "
          f"|iou - reference| = {float((iou.cpu().reshape(B, P * 3) - riou[:, :, 0]).abs().max()):.2e}")
    torch.testing.assert_close(lo.cpu().reshape(B, P * 3, F0, F0), rlo[:, :, 0], **TOL32)
    torch.testing.assert_close(hi.cpu().reshape(B, P * 3, R, R), rhi[:, :, 0], **TOL32)
    torch.testing.assert_close(iou.cpu().reshape(B, P * 3), riou[:, :, 0], **TOL32)


# ---- 4. the generator ------------------------------------------------------------------------------------------------------------------------------------
PPS, PPB = 4, 6
NMS_THRESHOLDS = (0.7, 0.5, 0.3, 0.1)


def _composed_infer(model):
    """`model.infer_masks` as the generator's chunks call it (points, low-res only), computed by the two-call composition."""
    plain = model.infer_masks                                             # the bound method: the composition's own calls do not see the patch

    def call(emb, points=None, point_labels=None, multimask_output=False, return_high_res=False):
        assert not return_high_res
        (_, lo, iou), _ = _compose(plain, emb, dict(points=points, point_labels=point_labels), multimask_output, return_high_res=False)
        return None, lo, iou
    return call


class _composed:
    """with _composed(model): every `model.infer_masks(...)` of a reference-side helper is the composition; restored on exit."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.model.infer_masks = _composed_infer(self.model)

    def __exit__(self, *exc):
        del self.model.infer_masks


@functools.lru_cache(None)
def _m2m_host_loop(dtype, multimask=True):
    """test_amg_gpu._host_loop with every chunk decoded by the composition: cvmi_bilinear_f32 maps, amg_ref on the CPU; the thresholds are the
    medians of its own values, the NMS threshold the first that drops a candidate.  -> (emb, thresholds, [dicts per image])."""
    lib, model = _lib.load(), _amg_model(dtype)
    C = 3 if multimask else 1
    grid = amg_ref.point_grid(PPS)
    pts_in = torch.from_numpy(grid.astype(np.float32)) * float(R)
    emb = model.encode_images(_images())
    lows, ious = [], []
    with _composed(model):
        for base in range(0, 16, PPB):
            pts = pts_in[base:base + PPB]
            if pts.shape[0] < PPB:
                pts = torch.cat([pts, pts[-1:].expand(PPB - pts.shape[0], 2)])
            _, low, iou = model.infer_masks(emb, points=pts.view(1, PPB, 1, 2).expand(2, PPB, 1, 2), point_labels=torch.ones(2, PPB, 1, dtype=torch.int32),
                                            multimask_output=multimask, return_high_res=False)
            lows.append(low.view(2, PPB, C, F0, F0))
            ious.append(iou.view(2, PPB, C))
    low, iou = torch.cat(lows, 1).contiguous(), torch.cat(ious, 1).cpu()                   # [2, 18, C, 64, 64], [2, 18, C]: points 16, 17 are padding
    lv = amg_ref.levels(0.0, 1.0)
    maps, stats = [], []
    for b, (H, W) in enumerate(SIZES):
        m = torch.empty(18 * C, H, W, device="cuda")
        _lib.check(lib.cvmi_bilinear_f32(low[b].data_ptr(), 18 * C, F0, F0, m.data_ptr(), H, W, None, 0.0, None), "bilinear")
        torch.cuda.synchronize()
        maps.append(m.cpu())
        stats.append(amg_ref.score_planes(maps[-1], *lv))
    valid_iou = np.concatenate([iou[b].reshape(-1)[:16 * C].numpy() for b in range(2)])
    valid_stab = np.concatenate([amg_ref.stability(stats[b].numpy())[:16 * C] for b in range(2)])
    iou_t, stab_t = float(np.median(valid_iou)), float(np.nanmedian(valid_stab))
    run = lambda nms_t: [amg_ref.generate_ref(low[b].cpu(), iou[b].numpy(), maps[b], grid, 16, H, W, iou_t, stab_t, lv, nms_t) for b, (H, W) in enumerate(SIZES)]
    no_nms = run(2.0)
    nms_t = next((t for t in NMS_THRESHOLDS if sum(map(len, run(t))) < sum(map(len, no_nms))), None)
    print(f"[amg m2m {dtype} multimask={multimask}] iou median {iou_t:.6f} (range {valid_iou.min():.4f} .. {valid_iou.max():.4f}), stability median {stab_t:.6f}, "
          f"kept by the filter {[len(d) for d in no_nms]} of {16 * C}, box_nms_thresh {nms_t}, after NMS {[len(d) for d in run(nms_t)] if nms_t else None}")
    assert nms_t is not None, "NMS drops no candidate at any of the thresholds"
    assert 0 < sum(map(len, no_nms)) < 2 * 16 * C                                          # the filter keeps some but not all
    return emb, (iou_t, stab_t, nms_t), run(nms_t)


def _generator(dtype, thresholds, **kw):
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    iou_t, stab_t, nms_t = thresholds
    args = dict(points_per_side=PPS, points_per_batch=PPB, pred_iou_thresh=iou_t, stability_score_thresh=stab_t, box_nms_thresh=nms_t)
    args.update(kw)
    return Sam2AutomaticMaskGenerator(_amg_model(dtype), **args)


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_generator_with_m2m_equals_the_host_loop(dtype):
    """B = 2 at (96, 160) and (256, 256), a 4 x 4 grid in chunks of 6, 6, 4: key for key and bit for bit the host loop over the composition, from
    images and from embeddings, on a first call and on a replay; the list differs from the plain one of the same generator, and a use_m2m=False
    call afterwards is still test_amg_gpu._host_loop's result at ITS thresholds."""
    emb, t, want = _m2m_host_loop(dtype)
    gen = _generator(dtype, t)
    got = gen.generate_batch(_images(), orig_hw=SIZES, use_m2m=True)
    torch.cuda.synchronize()
    for b in range(2):
        assert amg_ref.same_dicts(got[b], want[b]), (dtype, b, len(got[b]), len(want[b]))
        for d in got[b]:
            assert d["segmentation"].is_cuda and d["segmentation"].dtype == torch.uint8 and tuple(d["segmentation"].shape) == SIZES[b]
            assert d["area"] == int((d["segmentation"] != 0).sum())
        assert [d["predicted_iou"] for d in got[b]] == sorted((d["predicted_iou"] for d in got[b]), reverse=True)
    again = gen.generate_batch(emb, orig_hw=SIZES, use_m2m=True)                            # embeddings the caller holds; the plans replay
    torch.cuda.synchronize()
    assert all(amg_ref.same_dicts(again[b], want[b]) for b in range(2))
    plain = gen.generate_batch(emb, orig_hw=SIZES)                                          # the same generator without the pass
    assert not all(amg_ref.same_dicts(plain[b], got[b]) for b in range(2))
    assert all(amg_ref.same_dicts(p, q) for p, q in zip(plain, gen.generate_batch(emb, orig_hw=SIZES, use_m2m=False)))
    _, pt, pwant, _ = _plain_host_loop(dtype)                                               # the default path is untouched
    pgen = _generator(dtype, pt)
    pgen.generate_batch(emb, orig_hw=SIZES, use_m2m=True)
    pgot = pgen.generate_batch(emb, orig_hw=SIZES)
    assert all(amg_ref.same_dicts(pgot[b], pwant[b]) for b in range(2))


def test_generator_with_m2m_and_single_mask_output():
    emb, t, want = _m2m_host_loop("f32", False)
    gen = _generator("f32", t, multimask_output=False)
    got = gen.generate_batch(emb, orig_hw=SIZES, use_m2m=True)
    assert all(amg_ref.same_dicts(got[b], want[b]) for b in range(2)), [(len(g), len(w)) for g, w in zip(got, want)]
    assert sum(map(len, got)) > 0


# ---- 5. with the other per-call options ------------------------------------------------------------------------------------------------------------------
def test_m2m_composes_with_small_region_removal_and_rle():
    from circuitvision_amd import amg_utils
    emb, t, want = _m2m_host_loop("f32")
    gen = _generator("f32", t)
    base = gen.generate_batch(emb, orig_hw=SIZES, use_m2m=True)
    assert all(amg_ref.same_dicts(base[b], want[b]) for b in range(2)) and sum(map(len, base)) > 0
    rle = gen.generate_batch(emb, orig_hw=SIZES, use_m2m=True, output_mode="uncompressed_rle")
    for b in range(2):
        assert len(rle[b]) == len(base[b])
        assert [r["segmentation"] for r in rle[b]] == amg_utils.mask_to_rle(torch.stack([p["segmentation"] for p in base[b]])) or not base[b]
        for r, p in zip(rle[b], base[b]):
            assert tuple(r) == amg_ref.KEYS and r["area"] == p["area"] and all(r[k] == p[k] for k in amg_ref.KEYS[2:])
    for area in (8, 256):
        small = gen.generate_batch(emb, orig_hw=SIZES, use_m2m=True, min_mask_region_area=area)
        for b in range(2):
            assert amg_ref.same_dicts(small[b], amg_utils.postprocess_small_regions(base[b], area, t[2])), (area, b)


@functools.lru_cache(None)
def _m2m_crop_host_loop(dtype):
    """test_amg_crop_gpu._crop_host_loop on the 96 x 160 image with the chunk decode of its helper `_decode_crops` replaced by the composition.  The
    thresholds come from the m2m reference's own values, as there: the medians, and the first pair of NMS thresholds with which that file's four
    conditions hold -- or, when none does with the refined masks, the first pair that leaves a candidate (recorded in the output)."""
    import test_amg_crop_gpu as crop
    model = _amg_model(dtype)
    H, W, seed = crop.CANDIDATES[-1]
    assert (H, W) == (96, 160)
    img = crop._image(H, W, seed)
    with _composed(model):
        crops = crop._decode_crops(dtype, img, 1, 1)
    lv = amg_ref.levels(0.0, 1.0)
    valid_iou = np.concatenate([c["iou"].reshape(-1)[:c["n_points"] * 3] for c in crops])
    valid_stab = np.concatenate([amg_ref.stability(c["stats"].numpy())[:c["n_points"] * 3] for c in crops])
    t = dict(pred_iou_thresh=float(np.median(valid_iou)), stability_score_thresh=float(np.nanmedian(valid_stab)), lv=lv)
    fallback, tried = None, []
    for box_t in crop.NMS_THRESHOLDS:
        for crop_t in crop.NMS_THRESHOLDS:
            info = {}
            want = cref.generate_crops_ref(crops, H, W, box_nms_thresh=box_t, crop_nms_thresh=crop_t, info=info, **t)
            cond = crop._conditions(info)
            tried.append((box_t, crop_t, cond, len(want)))
            if all(cond):
                print(f"[amg m2m crops {dtype}] all four conditions hold: iou median {t['pred_iou_thresh']:.6f}, stability median "
                      f"{t['stability_score_thresh']:.6f}, box_nms_thresh {box_t}, crop_nms_thresh {crop_t}, {len(want)} masks from crops {info['crops_in_result']}")
                return img, dict(t, box_nms_thresh=box_t, crop_nms_thresh=crop_t), want
            if fallback is None and len(want) > 0:
                fallback = (dict(t, box_nms_thresh=box_t, crop_nms_thresh=crop_t), want, cond, info)
    assert fallback is not None, f"no candidate survives with m2m at any thresholds: {tried}"
    tt, want, cond, info = fallback
    print(f"[amg m2m crops {dtype}] the four conditions do not hold together with the refined masks at any of the {len(tried)} threshold pairs (conditions met: "
          f"{sorted({c for _, _, c, _ in tried})}); using box_nms_thresh {tt['box_nms_thresh']}, crop_nms_thresh {tt['crop_nms_thresh']}: conditions {cond}, "
          f"per crop {info['per_crop']}, {len(want)} masks from crops {info['crops_in_result']}")
    return img, tt, want


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_m2m_composes_with_one_crop_layer(dtype):
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    img, t, want = _m2m_crop_host_loop(dtype)
    gen = Sam2AutomaticMaskGenerator(_amg_model(dtype), points_per_side=PPS, points_per_batch=PPB, pred_iou_thresh=t["pred_iou_thresh"],
                                     stability_score_thresh=t["stability_score_thresh"], box_nms_thresh=t["box_nms_thresh"])
    got = gen.generate(img, crop_n_layers=1, crop_nms_thresh=t["crop_nms_thresh"], use_m2m=True)
    torch.cuda.synchronize()
    assert len(want) > 0 and amg_ref.same_dicts(got, want), (dtype, len(got), len(want), [d["crop_box"] for d in got], [d["crop_box"] for d in want])
    plain = gen.generate(img, crop_n_layers=1, crop_nms_thresh=t["crop_nms_thresh"])
    assert not amg_ref.same_dicts(plain, got)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------------------
def test_m2m_errors(monkeypatch):
    from circuitvision_amd import sam2_infer
    from circuitvision_amd.sam2_infer import SAM2Model
    model, c = _model("f32"), mref.mini_inputs(mref.MINI_SEED)
    x, boxes = c["x"], c["boxes"]
    with pytest.raises(ValueError, match="refine_steps"):
        model.infer_masks(x, boxes, refine_steps=1, m2m=True)
    with pytest.raises(ValueError, match="refine_steps"):
        model.infer_masks(x, _lists(c)["boxes"], refine_steps=2, m2m=True)
    with pytest.raises(ValueError, match="m2m"):
        model.infer_masks(x, m2m=True)                                  # no prompt
    with pytest.raises(ValueError, match="m2m"):
        model.infer_masks(_embeddings("f32", mref.MINI_SEED), m2m=True)
    with pytest.raises(ValueError, match="m2m_clamp"):
        model.infer_masks(x, boxes, m2m=True, m2m_clamp=-1.0)
    monkeypatch.setattr(sam2_infer, "M2M_MAX_PAIRS", B * P - 1)         # more pairs than the kernel's limit: refused before anything runs
    plans = len(model._plans)
    with pytest.raises(ValueError, match="at most"):
        model.infer_masks(x, boxes, multimask_output=True, m2m=True)
    assert len(model._plans) == plans
    monkeypatch.undo()
    p = _params()
    sd = {("sam2_model.base_model.model." + k if not k.startswith(("dense_", "sparse_", "refinement_")) else k): v
          for k, v in {**p.state_dict(), **p.mask_prompt_state_dict()}.items() if "mask_downscaling." not in k}
    stripped = SAM2Model(MINI, R, dtype="f32", use_refinement=True)
    stripped.load_state_dict(sd)
    assert stripped.weights.prompt_ok and not stripped.weights.mask_prompt_ok
    with pytest.raises(RuntimeError, match="mask_downscaling"):
        stripped.infer_masks(x, boxes, m2m=True)
    with pytest.raises(RuntimeError, match="mask_downscaling"):
        stripped.infer_masks(x, _lists(c)["boxes"], m2m=True)
