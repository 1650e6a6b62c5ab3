"""Reference and inputs for `infer_masks` with one prompt list per image (`Sam2Plan(pairs=cap)`, csrc/pair_ops.hip), plain torch.

The reference of a list call is `mask_prompt_ref.predict_prompts_masked` called image by image, each image with its own prompts; an image
without prompts gives empty tensors.  The inputs are subsets of `mask_prompt_ref.mini_inputs(MINI_SEED)` (B = 2, P = 3), chosen so that every
pair selects its single mask clearly on the reference (pairs are independent in the decoder); every single-mask comparison asserts
`selection_is_clear` on its own reference again, over all its pairs (tests/test_ragged_prompts_cpu.py does so without a GPU)."""
import torch

import mask_prompt_ref as ref

# per-image prompt counts of the B = 2 cases -> the image of mini_inputs(MINI_SEED) each batch slot holds; slot b keeps the first counts[b]
# prompts of its image.  (0, 3) puts image 1 first and takes the three prompts from image 0: the third click prompt of image 1 has its two
# best multimask IoU predictions 9.4e-3 apart when there is no mask prompt (`selection_is_clear` asks for 1e-2; every other pair of every
# kind: >= 1.1e-2), and the (0, 3) case runs click prompts without a mask.  (1, 3) runs box prompts only, where all of image 1 is clear.
COUNTS = {(3, 1): (0, 1), (1, 3): (0, 1), (2, 2): (0, 1), (0, 3): (1, 0)}
KINDS = ("boxes", "points", "boxes+points")


def case_counts(counts, order=(0, 1), seed=ref.MINI_SEED):
    """The B = 2 case `counts` on the images `order`: -> dict(x [2,3,R,R], boxes / points / labels / mask: lists of 2 tensors [P_b, ...])."""
    c = ref.mini_inputs(seed)
    return dict(x=c["x"][list(order)].clone(), **{k: [c[k][i, :n].clone() for i, n in zip(order, counts)] for k in ("boxes", "points", "labels", "mask")})


def case_b3(seed=ref.MINI_SEED):
    """B = 3: images (x0, x1, x0) with the lists (prompts0[:2], [], prompts0[2:]) -- an image without prompts in the middle and an image
    that appears twice."""
    c = ref.mini_inputs(seed)
    x = torch.stack((c["x"][0], c["x"][1], c["x"][0]))
    return dict(x=x, **{k: [c[k][0, :2].clone(), c[k][0, :0].clone(), c[k][0, 2:].clone()] for k in ("boxes", "points", "labels", "mask")})


CASES = {**{"counts_%d_%d" % cn: (lambda cn=cn, order=order: case_counts(cn, order)) for cn, order in COUNTS.items()}, "b3": case_b3}


def kind_args(c, kind):
    """The prompt arguments of `kind` ("boxes", "points", "boxes+points") as `infer_masks` takes them."""
    return dict(boxes=c["boxes"] if "boxes" in kind else None, points=c["points"] if "points" in kind else None,
                point_labels=c["labels"] if "points" in kind else None)


def predict_lists(wrapper, sd, c, kind, masked=False, multimask=False):
    """-> (high_res, low_res, iou, clear): lists of B tensors [P_b, n, ...] (n = 3 for multimask, else 1), as the per-image reference gives
    them; clear: every pair of a single-mask case selects clearly (True for multimask: nothing is selected)."""
    his, los, ious, clear = [], [], [], True
    R = c["x"].shape[-1]
    n = 3 if multimask else 1
    for b in range(c["x"].shape[0]):
        k = int(c["boxes"][b].shape[0])
        if k == 0:
            his.append(torch.zeros(0, n, R, R)); los.append(torch.zeros(0, n, R // 4, R // 4)); ious.append(torch.zeros(0, n))
            continue
        kw = dict(boxes=c["boxes"][b][None] if "boxes" in kind else None, points=c["points"][b][None] if "points" in kind else None,
                  labels=c["labels"][b][None] if "points" in kind else None, mask_input=c["mask"][b][None] if masked else None)
        with torch.no_grad():
            out = ref.predict_prompts_masked(wrapper, sd, c["x"][b:b + 1], multimask_output=multimask, margins=not multimask, **kw)
        if not multimask:
            clear = clear and ref.selection_is_clear(out[3], out[4])
        his.append(out[0][0]); los.append(out[1][0]); ious.append(out[2][0])
    return his, los, ious, clear
