"""Reference for embedding reuse and mask feedback (`SAM2Model.encode_images`, `infer_masks(emb, ...)`, `infer_masks(refine_steps=)`,
csrc/mask_prompt.hip best_candidate_kernel), plain torch / plain Python.

`best_candidate` restates cvmi_best_candidate; tests/test_embed_reuse_cpu.py holds it to `torch.argmax` and shows that the rows of
`selection_rows` tell it from two wrong selections.  `refine_recipe` is upstream's notebook recipe for ambiguous prompts on the reference predictor
(tests/mask_prompt_ref.py): a first pass, the candidate with the highest predicted IoU, a single-mask pass with its logits as the mask prompt."""
import itertools
import math

import torch

import mask_prompt_ref as mref

MUTANTS = ("last_max", "ignore_nan")             # wrong selections the comparison must tell from the right one


def select(row, mutant=None):
    """argmax of a list of floats as torch.argmax defines it: the lowest index among equal maxima, a NaN greater than every number (the first
    NaN wins).  Mutants: "last_max" takes the highest index among equal maxima, "ignore_nan" never selects a NaN (unless all are)."""
    sel = 0
    for k in range(1, len(row)):
        best, x = row[sel], row[k]
        if mutant == "ignore_nan":
            if math.isnan(best) or (not math.isnan(x) and x > best):
                sel = k
        elif not math.isnan(best) and (math.isnan(x) or x > best or (mutant == "last_max" and x == best)):
            sel = k
    return sel


def best_candidate(low_res, iou, mutant=None):
    """low_res [n, NM, P], iou [n, NM] -> (mask [n, P] = low_res[i, sel[i]], sel int32 [n])."""
    sel = torch.tensor([select(row, mutant) for row in iou.tolist()], dtype=torch.int64)
    return low_res[torch.arange(low_res.shape[0]), sel], sel.to(torch.int32)


def selection_rows(NM):
    """The IoU rows every selection test starts with: a tie of the two largest at every pair of positions (the third value below and above
    the tie), all equal, a NaN at each position (beside larger and smaller numbers, and +inf), two NaNs, all NaN, and signed zeros."""
    if NM == 1:
        return torch.tensor([[0.5], [float("nan")], [-1.0]])
    nan, inf = float("nan"), float("inf")
    rows = []
    for i, j in itertools.combinations(range(NM), 2):
        for other in (0.25, 0.9):
            r = [other] * NM
            r[i] = r[j] = 0.75
            rows.append(r)
    rows.append([0.5] * NM)
    for i in range(NM):
        for fill in ((0.1, 0.9), (0.9, 0.1), (inf, 0.2)):
            r = list(fill[:NM - 1])
            r.insert(i, nan)
            rows.append(r)
    for i, j in itertools.combinations(range(NM), 2):
        r = [0.7] * NM
        r[i] = r[j] = nan
        rows.append(r)
    rows += [[nan] * NM, [0.0, -0.0, 0.0], [-0.0, 0.0, -1.0]]
    return torch.tensor(rows)


def candidate_inputs(n, NM, P, seed=0):
    """Inputs of the op test: randn logits, IoU rows = selection_rows, repeated / cut to n, the rest uniform random."""
    g = torch.Generator().manual_seed(100 * n + 10 * NM + seed)
    low = torch.randn(n, NM, P, generator=g)
    iou = torch.rand(n, NM, generator=g)
    rows = selection_rows(NM)
    k = min(n, rows.shape[0])
    iou[n - k:] = rows[:k]                        # n = 1: the first tie row
    return low, iou


# input seeds of the refine_steps GPU tests (weights: seed 9, std 0.05; box prompts; mask_prompt_ref's MINI_SEED and REPLAY_SEED): on the
# reference, with the inputs as they are and rounded to F16, every pair of pass 1 has its two best IoU predictions at least 1e-2 apart -- and,
# single-mask, selects clearly -- and every pair of pass 2 selects clearly; checked on the CPU by tests/test_embed_reuse_cpu.py
REFINE_SEEDS = (28, 11)


def refine_recipe(oracle, sd, x, boxes, multimask):
    """-> (pass 2's (high_res [B,P,R,R], low_res [B,P,R/4,R/4], iou [B,P]), clear: the preconditions of comparing a device run with it)."""
    with torch.no_grad():
        if multimask:
            _, lo1, iou1 = mref.predict_prompts_masked(oracle, sd, x, boxes=boxes, multimask_output=True)
            top = iou1.sort(-1, descending=True).values
            clear = bool(((top[..., 0] - top[..., 1]) >= 1e-2).all())
        else:
            _, lo1, iou1, stab1, iou41 = mref.predict_prompts_masked(oracle, sd, x, boxes=boxes, margins=True)
            clear = mref.selection_is_clear(stab1, iou41)
        B, P, NM = iou1.shape
        picked, _ = best_candidate(lo1.reshape(B * P, NM, -1), iou1.reshape(B * P, NM))
        picked = picked.reshape(B, P, *lo1.shape[-2:])
        hi2, lo2, iou2, stab2, iou42 = mref.predict_prompts_masked(oracle, sd, x, boxes=boxes, mask_input=picked, margins=True)
    return (hi2[:, :, 0], lo2[:, :, 0], iou2[:, :, 0]), clear and mref.selection_is_clear(stab2, iou42)
