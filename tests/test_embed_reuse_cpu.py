"""Embedding reuse and mask feedback without a GPU: the route's cut at the seam (`DecoderRoute.neck_launches` / `decoder_launches`), the
`Sam2Embeddings` container on CPU tensors, the reference of cvmi_best_candidate (tests/embed_reuse_ref.py) against `torch.argmax` with its proof
of bite, and the preconditions of the refine_steps GPU tests on the reference predictor."""
import pytest
import torch

import embed_reuse_ref as ref
import mask_prompt_ref as mref
import sam2_route_cases as rc
from circuitvision_amd import decoder_route as dr
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import is16
from circuitvision_amd.sam2 import Sam2Weights
from circuitvision_amd.sam2_infer import Sam2Embeddings
from test_decoder_route_cpu import FIXTURE, _route
from test_mask_prompt_cpu import _params, full_sd
from test_oracle_sam2_cpu import MINI, mini_oracle
from test_sam2_route_cpu import _switches


# ---- the route ---------------------------------------------------------------------------------------------------------------------------
def _trunk_case_route(case):
    dims = [rc.hiera_of(case["hiera"])["embed_dim"] * 2 ** s for s in range(4)]
    dt = rc.dtype_of(case["dtype"])
    tok = tuple(is16(dt) and d <= 288 and dr.tok_linear_supported(d, dt, 256) for d in dims[:2])
    return dr.route_decoder(dt, case["B"], case["size"], _switches(case["env"]), prompts=case["prompts"], neck_tok=tok, stage_dims=dims)


ROUTES = [(c["id"], _route, c) for c in rc.HEAD_CASES] + [(c["id"], _trunk_case_route, c) for c in rc.CASES]


@pytest.mark.parametrize("make,case", [x[1:] for x in ROUTES], ids=[x[0] for x in ROUTES])
def test_neck_and_decoder_launches_cut_launches_behind_embed(make, case):
    r = make(case)
    neck, dec = r.neck_launches(), r.decoder_launches()
    assert neck + dec == r.launches()
    assert neck[-1] == ("embed", "neck") and all(kind in ("cast", "neck") for _, kind in neck)
    assert all(kind in ("cast", "layernorm", "decoder", "tail") for _, kind in dec) and not any(l.startswith(("cast.s", "feat_s", "embed")) for l, _ in dec)
    if case["id"] in FIXTURE:                                            # ... and the recorded sequence, cut at the same place
        want = [tuple(x[:2]) for x in FIXTURE[case["id"]]["launches"][2:]]
        cut = want.index(("embed", "neck")) + 1
        assert neck == want[:cut] and dec == want[cut:]


# ---- the container ------------------------------------------------------------------------------------------------------------------------
def _emb(B, seed=0, weights_id=1, dtype=F16, R=64, prompted=True):
    g = torch.Generator().manual_seed(seed)
    f0, fs = R // 4, R // 16
    td = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}[dtype]
    return Sam2Embeddings(torch.randn(B, f0, f0, 32, generator=g).to(td), torch.randn(B, f0 // 2, f0 // 2, 64, generator=g).to(td),
                          torch.randn(B, fs, fs, 256, generator=g) if prompted else None, torch.randn(B, fs, fs, 256, generator=g), R, dtype, weights_id)


def _same(a, b):
    return a.signature() == b.signature() and all(torch.equal(x, y) for (_, x), (_, y) in zip(a.tensors(), b.tensors()))


def test_embeddings_index_and_cat_round_trip():
    e = _emb(4)
    assert len(e) == 4 and e.image_size == 64 and e.dtype == F16 and e.weights_id == 1
    assert e.nbytes == 4 * (16 * 16 * 32 * 2 + 8 * 8 * 64 * 2 + 2 * 4 * 4 * 256 * 4)
    assert len(e[2]) == 1 and torch.equal(e[2].emb, e.emb[2:3]) and torch.equal(e[-1].dense, e.dense[3:])
    assert len(e[1:3]) == 2 and torch.equal(e[1:3].feat_s0, e.feat_s0[1:3])
    assert torch.equal(e[[3, 0, 3]].feat_s1, e.feat_s1[[3, 0, 3]])
    assert isinstance(e[0], Sam2Embeddings) and isinstance(e[[1]], Sam2Embeddings)
    assert _same(Sam2Embeddings.cat([e[i] for i in range(4)]), e)
    assert _same(Sam2Embeddings.cat([e[0:1], e[1:4]]), e)
    assert _same(Sam2Embeddings.cat([e[[2, 1]], e[3]]), e[[2, 1, 3]])
    assert _same(Sam2Embeddings.cat([e]), e)
    learned = _emb(2, prompted=False)                                   # a checkpoint without a prompt encoder: no `emb`
    assert learned.emb is None and len(learned[1]) == 1 and learned[1].emb is None and _same(Sam2Embeddings.cat([learned[0], learned[1]]), learned)
    assert learned.nbytes == 2 * (16 * 16 * 32 * 2 + 8 * 8 * 64 * 2 + 4 * 4 * 256 * 4)
    with pytest.raises(IndexError):
        e[4]
    with pytest.raises(IndexError):
        e[[0, -5]]
    with pytest.raises(TypeError):
        e["0"]


def test_embeddings_refuse_a_mix_and_wrong_shapes():
    e = _emb(2)
    for other in (_emb(1, weights_id=2), _emb(1, dtype=BF16), _emb(1, dtype=F32), _emb(1, R=128), _emb(1, prompted=False)):
        with pytest.raises(ValueError, match="do not mix"):
            Sam2Embeddings.cat([e, other])
        with pytest.raises(ValueError, match="do not mix"):
            Sam2Embeddings.cat([other, e[0]])
    with pytest.raises(ValueError, match="empty"):
        Sam2Embeddings.cat([])
    with pytest.raises(TypeError):
        Sam2Embeddings.cat([e, e.emb])
    with pytest.raises(ValueError, match="feat_s1"):
        Sam2Embeddings(e.feat_s0, e.feat_s1[:1], e.emb, e.dense, 64, F16, 1)
    with pytest.raises(ValueError, match="emb"):
        Sam2Embeddings(e.feat_s0, e.feat_s1, e.emb[:, :2], e.dense, 64, F16, 1)


# ---- the reference of cvmi_best_candidate -------------------------------------------------------------------------------------------------
def _argmax_truth(low, iou):
    sel = torch.argmax(iou, dim=1)
    return low[torch.arange(low.shape[0]), sel], sel.to(torch.int32)


@pytest.mark.parametrize("NM", [1, 3])
def test_best_candidate_reference_is_torch_argmax(NM):
    rows = ref.selection_rows(NM)
    g = torch.Generator().manual_seed(3)
    iou = torch.cat((rows, torch.rand(64, NM, generator=g)))
    low = torch.randn(iou.shape[0], NM, 8, generator=g)
    mask, sel = ref.best_candidate(low, iou)
    want_mask, want_sel = _argmax_truth(low, iou)
    assert torch.equal(sel, want_sel) and torch.equal(mask, want_mask)
    if NM == 1:
        assert not sel.any() and torch.equal(mask, low[:, 0])
        return
    # the rows say what they are meant to: a tie at every pair of positions, all equal, a NaN at each position
    t = rows.tolist()
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert any(r[i] == r[j] == max(r) and r[3 - i - j] < r[i] for r in t)
    assert any(r[0] == r[1] == r[2] for r in t)
    for i in range(3):
        assert any(r[i] != r[i] and all(x == x for k, x in enumerate(r) if k != i) and max(x for x in r if x == x) > 0.5 for r in t)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_best_candidate_comparison_catches_wrong_selections(mutant):
    """On the very inputs the GPU op test uses (`candidate_inputs`, n = 33), a selection that takes the last maximum, and one that ignores NaN, both
    differ from torch.argmax -- in `sel` and in the mask."""
    low, iou = ref.candidate_inputs(33, 3, 4)
    want_mask, want_sel = _argmax_truth(low, iou)
    mask, sel = ref.best_candidate(low, iou)
    assert torch.equal(sel, want_sel) and torch.equal(mask, want_mask)
    bad_mask, bad_sel = ref.best_candidate(low, iou, mutant)
    assert not torch.equal(bad_sel, want_sel) and not torch.equal(bad_mask, want_mask)


def test_candidate_inputs_hold_the_edge_rows():
    for n in (1, 33):
        low, iou = ref.candidate_inputs(n, 3, 4)
        assert low.shape == (n, 3, 4) and iou.shape == (n, 3)
        rows = ref.selection_rows(3)
        k = min(n, rows.shape[0])
        assert torch.equal(iou[n - k:].nan_to_num(nan=-5.0), rows[:k].nan_to_num(nan=-5.0))
    assert ref.selection_rows(3).shape[0] <= 33                         # n = 33 holds every row


# ---- the oracle recipe: the seeds of the GPU tests -----------------------------------------------------------------------------------------
def test_refine_recipe_moves_the_masks_and_the_gpu_seeds_select_clearly():
    p = _params()
    Sam2Weights(p, MINI, 256, F32, device="cpu")
    sd, oracle = full_sd(p), mini_oracle(p, 256)
    for seed in ref.REFINE_SEEDS:
        c = mref.mini_inputs(seed)
        for x in (c["x"], c["x"].half().float()):
            for multimask in (True, False):
                (hi, lo, iou), clear = ref.refine_recipe(oracle, sd, x, c["boxes"], multimask)
                assert clear, (seed, multimask)
                assert hi.shape == (2, 3, 256, 256) and lo.shape == (2, 3, 64, 64) and iou.shape == (2, 3)
        with torch.no_grad():
            _, lo0, _ = mref.predict_prompts_masked(oracle, sd, c["x"], boxes=c["boxes"])
        (_, lo1, _), _ = ref.refine_recipe(oracle, sd, c["x"], c["boxes"], False)
        assert float((lo1 - lo0[:, :, 0]).abs().max()) > 0.1            # the feedback pass is not the first pass again
