"""Prompt lists without a GPU: the host packing of `infer_masks` with one prompt list per image (`sam2_infer.pack_prompt_lists`: coords,
labels, the pair-to-image table, cap, the split sizes, the padding slots, every error path), the precondition of the reference the GPU
tests compare with (tests/ragged_prompt_ref.py), and the attention descriptor's field order against its ctypes mirror."""
import functools
import os
import re

import pytest
import torch

import mask_prompt_ref as mref
import ragged_prompt_ref as ref
from circuitvision_amd import _lib
from circuitvision_amd._lib import F32
from circuitvision_amd.sam2 import Sam2Weights, SamSyntheticParams
from circuitvision_amd.sam2_infer import pack_prompt_lists
from test_oracle_sam2_cpu import MINI, mini_oracle, mini_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, F0 = 256, 64


# ---- the host packing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [1, 8, 32])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_packing_of_every_case(name, bucket):
    c = ref.CASES[name]()
    B = c["x"].shape[0]
    sizes = [int(t.shape[0]) for t in c["boxes"]]
    N = sum(sizes)
    pk = pack_prompt_lists(B, R, boxes=c["boxes"], points=c["points"], point_labels=c["labels"], mask_input=c["mask"], pair_bucket=bucket)
    cap = -(-N // bucket) * bucket
    assert (pk["sizes"], pk["N"], pk["cap"], pk["K"], pk["has_mask"]) == (sizes, N, cap, 2 + 2 + 1, True)
    assert cap % bucket == 0 and N <= cap < N + bucket
    assert pk["coords"].shape == (cap, 5, 2) and pk["coords"].dtype == torch.float32
    assert pk["labels"].shape == (cap, 5) and pk["labels"].dtype == torch.int32
    assert pk["pair_image"].shape == (cap,) and pk["pair_image"].dtype == torch.int32
    # real pairs: image-major, each image's prompts in their own order
    want_img = [b for b, n in enumerate(sizes) for _ in range(n)]
    assert pk["pair_image"][:N].tolist() == want_img
    assert torch.equal(pk["coords"][:N, :2].reshape(N, 4), torch.cat(c["boxes"]))
    assert torch.equal(pk["coords"][:N, 2:4], torch.cat(c["points"]))
    assert torch.equal(pk["labels"][:N, 2:4], torch.cat(c["labels"]).to(torch.int32))
    assert bool((pk["labels"][:N, :2] == torch.tensor([2, 3], dtype=torch.int32)).all()) and bool((pk["labels"][:, 4] == -1).all())
    assert bool((pk["coords"][:, 4] == 0).all())
    # padding slots: image 0, the whole-image box, no click
    assert pk["pair_image"][N:].tolist() == [0] * (cap - N)
    assert torch.equal(pk["coords"][N:, :2].reshape(cap - N, 4), torch.tensor([0.0, 0.0, R, R]).expand(cap - N, 4))
    assert bool((pk["coords"][N:, 2:] == 0).all())
    assert pk["labels"][N:].tolist() == [[2, 3, -1, -1, -1]] * (cap - N)
    # every table value names an image
    assert 0 <= int(pk["pair_image"].min()) and int(pk["pair_image"].max()) < B


def test_packing_of_each_prompt_kind():
    c = ref.case_counts((1, 3))
    pb = pack_prompt_lists(2, R, boxes=c["boxes"], pair_bucket=8)
    assert (pb["K"], pb["N"], pb["cap"], pb["has_mask"]) == (3, 4, 8, False)
    assert pb["labels"].tolist() == [[2, 3, -1]] * 8
    pp = pack_prompt_lists(2, R, points=c["points"], point_labels=c["labels"], pair_bucket=8)
    assert (pp["K"], pp["N"], pp["cap"]) == (3, 4, 8)
    assert torch.equal(pp["coords"][:4, :2], torch.cat(c["points"])) and pp["labels"][:4].tolist() == [[1, 0, -1]] * 4
    # without boxes a padding slot holds not-a-point tokens only
    assert pp["labels"][4:].tolist() == [[-1, -1, -1]] * 4 and bool((pp["coords"][4:] == 0).all())
    # tuples are lists; devices and float types of the entries do not matter to the packing
    pt = pack_prompt_lists(2, R, boxes=tuple(t.double() for t in c["boxes"]), pair_bucket=1)
    assert pt["cap"] == 4 and torch.equal(pt["coords"], pb["coords"][:4])


def test_packing_refuses_what_it_cannot_serve():
    c = ref.case_counts((2, 2))
    bx, pts, lab, mk = c["boxes"], c["points"], c["labels"], c["mask"]
    bad = [
        dict(boxes=bx[:1]),                                                    # wrong list length
        dict(boxes=bx + [bx[0]]),
        dict(boxes=bx, points=pts[:1], point_labels=lab[:1]),
        dict(boxes=bx, mask_input=mk + [mk[0]]),
        dict(boxes=[bx[0], bx[1][:1]], points=pts, point_labels=lab),          # counts differ between the arguments
        dict(boxes=bx, points=pts, point_labels=[lab[0], lab[1][:1]]),
        dict(boxes=bx, mask_input=[mk[0], mk[1][:1]]),
        dict(boxes=[bx[0][:0], bx[1][:0]]),                                    # N == 0
        dict(boxes=[bx[0], bx[1].tolist()]),                                   # entries that are not tensors
        dict(boxes=[bx[0], None]),
        dict(boxes=bx, mask_input=[mk[0], mk[1].numpy()]),
        dict(boxes=torch.stack(bx), mask_input=mk),                            # a tensor beside a list
        dict(boxes=bx, points=torch.stack(pts), point_labels=lab),
        dict(boxes=[bx[0][:, :3], bx[1]]),                                     # shapes
        dict(boxes=[bx[0].reshape(-1), bx[1]]),
        dict(boxes=bx, points=pts),                                            # points without labels
        dict(points=[pts[0], pts[1][:, :1]], point_labels=[lab[0], lab[1][:, :1]]),      # K differs between images
        dict(points=[p[:, :0] for p in pts], point_labels=[l[:, :0] for l in lab]),      # K == 0
        dict(points=pts, point_labels=[lab[0] + 2, lab[1]]),                   # labels outside -1 .. 1
        dict(boxes=bx, mask_input=[m[..., :F0 - 1] for m in mk]),              # mask size
        dict(boxes=bx, mask_input=[m > 0 for m in mk]),                        # not float logits
        dict(mask_input=mk),                                                   # a mask-only prompt
        dict(boxes=bx, pair_bucket=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            pack_prompt_lists(2, R, **kw)
    pack_prompt_lists(2, R, boxes=bx, points=pts, point_labels=lab, mask_input=mk)        # ... and the complete call passes


# ---- the reference's precondition ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _oracle():
    p = SamSyntheticParams(seed=9, lora_targets=mini_targets(), std=0.05)
    Sam2Weights(p, MINI, R, F32, device="cpu")                       # (the packed model reads every tensor the oracle loads)
    return mini_oracle(p, R), {**p.state_dict(), **p.mask_prompt_state_dict()}


# (case, kind, masked, 16-bit input) of every single-mask comparison tests/test_ragged_prompts_gpu.py makes
GPU_SINGLE = ([(n, k, False, False) for n in ("counts_3_1", "counts_0_3", "b3") for k in ref.KINDS]
              + [("counts_1_3", "boxes", True, False), ("counts_2_2", "boxes", False, False), ("counts_3_1", "boxes", False, True), ("b3", "boxes", False, True)])


@pytest.mark.parametrize("name,kind,masked,half", GPU_SINGLE, ids=["%s-%s%s%s" % (n, k, "-mask" if m else "", "-f16" if h else "") for n, k, m, h in GPU_SINGLE])
def test_every_gpu_case_selects_clearly_on_the_reference(name, kind, masked, half):
    oracle, sd = _oracle()
    c = ref.CASES[name]()
    if half:
        c["x"] = c["x"].half().float()
    hi, lo, iou, clear = ref.predict_lists(oracle, sd, c, kind, masked=masked)
    assert clear, (name, kind, masked)
    for b, t in enumerate(c["boxes"]):
        k = t.shape[0]
        assert hi[b].shape == (k, 1, R, R) and lo[b].shape == (k, 1, F0, F0) and iou[b].shape == (k, 1)


def test_list_reference_equals_the_batched_reference_on_uniform_counts():
    """Pairs are independent: the per-image reference with all three prompts of each image is the batched reference, bit for bit."""
    oracle, sd = _oracle()
    c = mref.mini_inputs(mref.MINI_SEED)
    with torch.no_grad():
        hi, lo, iou = mref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"])
    lhi, llo, liou, _ = ref.predict_lists(oracle, sd, ref.case_counts((3, 3)), "boxes")
    assert torch.equal(torch.stack(llo), lo) and torch.equal(torch.stack(liou), iou) and torch.equal(torch.stack(lhi), hi)


# ---- the attention descriptor --------------------------------------------------------------------------------------------------------------
def test_attn_desc_field_order_equals_the_ctypes_mirror():
    hdr = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    body = hdr[hdr.index("typedef struct cvmi_attn_desc {") + len("typedef struct cvmi_attn_desc {"):hdr.index("} cvmi_attn_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"\b(const|void|float|int|long)\b", " ", decl)
        fields += [n for n in re.findall(r"[A-Za-z_][A-Za-z_0-9]*", decl)]
    assert fields == [n for n, _ in _lib.AttnDesc._fields_], "AttnDesc field order differs from cvmi_attn_desc"
    assert fields[-2:] == ["q_bmap", "kv_bmap"]
    assert [n for n, _ in _lib.ConvDesc._fields_][-1] == "res_map"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all('"%s"' % n in doc for n in ("res_map", "q_bmap", "kv_bmap"))
