"""Prompt lists on the GPU (`infer_masks` with one prompt list per image, `Sam2Plan(pairs=cap)`, csrc/pair_ops.hip and the table forms of
cvmi_mask_prompt_embed / cvmi_conv2d / cvmi_attention).  The ops are compared bit for bit with the existing path on operands gathered by
`torch.index_select` -- the arithmetic is the same, only addresses differ -- behind guard bands; the mini model against the per-image
reference of tests/ragged_prompt_ref.py.  Model tests print their measured errors before they assert (`pytest -s`)."""
import ctypes as C
import functools

import pytest
import torch

import mask_prompt_ref as mref
import ragged_prompt_ref as ref
from circuitvision_amd import _lib
from circuitvision_amd._lib import ACT_GELU, BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, Buf, PackedConv, Plan, op_conv
from circuitvision_amd.sam2_infer import pack_prompt_lists
from helpers import quant, run, stream, to_buf
from op_matrix import SHARE_ROWS
from test_attention_matrix_gpu import SENTINEL, _desc, _launch, _tok
from test_oracle_sam2_cpu import MINI, mini_oracle, mini_targets

pytestmark = pytest.mark.gpu
R, F0 = 256, 64
TOL32 = dict(rtol=1e-3, atol=1e-3)               # the project's f32 bound
TOL16 = dict(rtol=3e-2, atol=3e-2)               # ... and its 16-bit one
GUARD = 512                                      # elements behind every output the kernel must leave alone


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


# ---- cvmi_gather_images ----------------------------------------------------------------------------------------------------------------------
PAST_CAP = 64 * 256 * 16 + 16 * 37               # one 16-byte chunk row past 64 workgroups of 256 threads: the loop runs twice


def _gather(src, table, lp):
    """src f32 [images, n] -> (dst f32 [pairs, n], 16-bit copy or None, tag), both outputs behind a guard band."""
    lib = _lib.load()
    n, pairs = src.shape[1], len(table)
    dst = torch.full((pairs * n + GUARD,), -7.0, device="cuda")
    dlp = torch.full((pairs * n + GUARD,), -7.0, device="cuda", dtype=TORCH_DTYPE[lp]) if lp is not None else None
    tab = _i32(table)
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _lib.check(lib.cvmi_gather_images(src.data_ptr(), dst.data_ptr(), dlp.data_ptr() if lp is not None else None, lp if lp is not None else 0,
                                      n * 4, tab.data_ptr(), pairs, None), "gather_images")
    tag = lib.cvmi_last_kernel().decode()
    torch.cuda.synchronize()
    assert bool((dst[pairs * n:] == -7.0).all()) and (dlp is None or bool((dlp[pairs * n:] == -7.0).all())), "wrote past the end"
    return dst[:pairs * n].view(pairs, n), (dlp[:pairs * n].view(pairs, n) if lp is not None else None), tag


@pytest.mark.parametrize("nbytes", [16, 16 * 37, PAST_CAP])
@pytest.mark.parametrize("images,table", [(1, [0]), (3, [1, 1, 1, 2, 2]), (3, [2, 0, 2, 1, 0])], ids=["1x1", "unused_image", "non_monotone"])
def test_gather_images_equals_index_select(images, table, nbytes):
    g = torch.Generator().manual_seed(images * 1000 + nbytes)
    src = (3 * torch.randn(images, nbytes // 4, generator=g)).cuda()
    want = src.index_select(0, _i32(table).long())
    dst, none, tag = _gather(src, table, None)
    assert none is None and torch.equal(dst, want) and tag == "gather_images_kernel<_Float16>"
    for lp, name in ((F16, "_Float16"), (BF16, "__bf16")):
        d2, d16, tag = _gather(src, table, lp)
        assert tag == f"gather_images_kernel<{name}>"
        assert torch.equal(d2, want) and torch.equal(d16, want.to(TORCH_DTYPE[lp])), name      # the f32 output rounded once


def test_gather_images_rejects_bad_arguments():
    lib = _lib.load()
    t, tab = torch.zeros(64, device="cuda"), _i32([0])
    p = t.data_ptr()
    assert lib.cvmi_gather_images(p, p + 64, None, 0, 24, tab.data_ptr(), 1, None) != 0           # not a multiple of 16
    assert lib.cvmi_gather_images(p, p + 64, None, 0, 16, None, 1, None) != 0                     # no table
    assert lib.cvmi_gather_images(p, p + 64, None, 0, 16, tab.data_ptr(), 0, None) != 0
    assert lib.cvmi_gather_images(p + 4, p + 64, None, 0, 16, tab.data_ptr(), 1, None) != 0       # misaligned
    assert lib.cvmi_gather_images(p, p + 64, p + 128, F32, 16, tab.data_ptr(), 1, None) != 0      # the copy must be a 16-bit type
    assert b"gather_images" in lib.cvmi_last_error()


# ---- cvmi_mask_prompt_embed_pairs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _params():
    from circuitvision_amd.sam2 import SamSyntheticParams
    return SamSyntheticParams(seed=9, lora_targets=mini_targets(), std=0.05)


def _embed(mask_d, emb_d, prm_d, fs, lp, rep=None, table=None):
    """cvmi_mask_prompt_embed (rep) or cvmi_mask_prompt_embed_pairs (table) -> (keys, 16-bit copy, tag), outputs behind guard bands."""
    lib = _lib.load()
    n = mask_d.shape[0]
    numel = n * fs * fs * 256
    keys = torch.full((numel + GUARD,), -7.0, device="cuda")
    klp = torch.full((numel + GUARD,), -7.0, device="cuda", dtype=TORCH_DTYPE[lp])
    head = (mask_d.data_ptr(), emb_d.data_ptr(), prm_d.data_ptr(), keys.data_ptr(), klp.data_ptr(), lp)
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    if table is None:
        _lib.check(lib.cvmi_mask_prompt_embed(*head, emb_d.shape[0], rep, fs, None), "mask_prompt_embed")
    else:
        tab = _i32(table)
        _lib.check(lib.cvmi_mask_prompt_embed_pairs(*head, n, tab.data_ptr(), fs, None), "mask_prompt_embed_pairs")
    tag = lib.cvmi_last_kernel().decode()
    torch.cuda.synchronize()
    assert bool((keys[numel:] == -7.0).all()) and bool((klp[numel:] == -7.0).all()), "wrote past the end"
    return keys[:numel].view(n, fs * fs, 256), klp[:numel].view(n, fs * fs, 256), tag


@pytest.mark.parametrize("lp", [F16, BF16])
def test_mask_prompt_embed_pairs_equals_the_uniform_form(lp):
    sd = mref.op_state_dict(_params())
    mask, emb = mref.op_inputs(2, 3, 16, sd)
    mask_d, emb_d, prm_d = mask.cuda(), emb.cuda(), mref.pack_params(sd).cuda()
    keys, k16, tag = _embed(mask_d, emb_d, prm_d, 16, lp, rep=3)
    keys_t, k16_t, tag_t = _embed(mask_d, emb_d, prm_d, 16, lp, table=[0, 0, 0, 1, 1, 1])
    assert tag_t == tag and torch.equal(keys_t, keys) and torch.equal(k16_t, k16)


def test_mask_prompt_embed_pairs_vs_fp64():
    """Table [1, 0, 1] against the float64 reference applied pair by pair; bound as in tests/test_mask_prompt_gpu.py: 8 x the error of the f32
    torch evaluation of the same reference on the same inputs."""
    sd = mref.op_state_dict(_params())
    table, fs = [1, 0, 1], 9
    mask, emb = mref.op_inputs(3, 1, fs, sd)
    emb = emb[:2].contiguous()
    per_pair = lambda dt: torch.cat([mref.mask_prompt_keys(sd, mask[i:i + 1], emb[b:b + 1], 1, dt) for i, b in enumerate(table)])
    want = per_pair(torch.float64)
    f32_err = float((per_pair(torch.float32).double() - want).abs().max())
    keys, k16, _ = _embed(mask.cuda(), emb.cuda(), mref.pack_params(sd).cuda(), fs, F16, table=table)
    err = float((keys.double() - want.cuda()).abs().max())
    print(f"mask_prompt_embed_pairs {table}: |kernel - f64| = {err:.3e}, |torch f32 - f64| = {f32_err:.3e}")
    assert err <= 8 * f32_err, (err, f32_err)
    assert torch.equal(k16, keys.to(torch.float16))
    lib, t = _lib.load(), torch.zeros(4684 + 64, device="cuda")
    assert lib.cvmi_mask_prompt_embed_pairs(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 0, 1, None, 1, None) != 0      # no table
    assert b"mask_prompt_embed_pairs" in lib.cvmi_last_error()


# ---- cvmi_conv2d with res_map ----------------------------------------------------------------------------------------------------------------
CONV_TABLE = [2, 0, 2, 1, 0]                     # 5 pairs over 3 residual images, non-monotone


def _conv_res(form, dtype, mapped):
    """One launch of the form ("shuffle": ConvTranspose scatter 4 x 4 -> 8 x 8; "mod": 16 rows per image, N = 32), the residual read through
    the table (mapped) or gathered in full -> (output incl. one guard image, descriptor)."""
    g = torch.Generator().manual_seed(17)
    pairs, imgs, Cin = len(CONV_TABLE), 3, 64
    x = quant(torch.randn(pairs, Cin, 4, 4, generator=g), dtype)
    sc = 32 if form == "shuffle" else 0
    N = 4 * sc if sc else 32
    oh = 8 if sc else 4
    w = quant(torch.randn(N, Cin, 1, 1, generator=g) / 8, dtype)
    skip = quant(torch.randn(imgs, sc or N, oh, oh, generator=g), dtype)
    pc = PackedConv(w, torch.randn(N, generator=g), dtype)
    xb = to_buf(x, dtype)
    tab = _i32(CONV_TABLE)
    sb = to_buf(skip if mapped else skip.index_select(0, tab.long().cpu()), dtype)
    yfull = Buf(pairs + 1, oh, oh, sc or N, dtype)
    yfull.t.fill_(SENTINEL)
    yb = yfull.images(0, pairs)
    plan = Plan(stream())
    kw = dict(shuffle_cout=sc, act=ACT_GELU, act_after_res=True) if sc else dict(res_mod=16 if mapped else 0)
    d = op_conv(plan, "c", pc, [(xb.view(), 0)], yb.view(), res=sb.view(), res_map=tab if mapped else None, **kw)
    run(plan)
    return yfull.t.clone(), d, (xb, sb, yfull, pc, tab)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("form", ["shuffle", "mod"])
def test_conv2d_res_map_equals_the_gathered_residual(form, dtype):
    got, _, _ = _conv_res(form, dtype, True)
    want, _, _ = _conv_res(form, dtype, False)
    assert bool((got[-1] == SENTINEL).all()), "wrote past the last pair"
    assert torch.equal(got, want)
    assert float(got[:-1].float().abs().max()) > 0.5 and bool(torch.isfinite(got.float()).all())


def test_conv2d_res_map_rejects_what_it_cannot_serve():
    lib = _lib.load()
    _, d, keep = _conv_res("mod", F16, True)
    torch.cuda.synchronize()
    assert lib.cvmi_conv2d(C.byref(d), None) == 0
    torch.cuda.synchronize()
    for field, value in (("res", None), ("res_rep", 5), ("res_mod", 0), ("res_mod", 8)):
        old = getattr(d, field)
        setattr(d, field, value)
        assert lib.cvmi_conv2d(C.byref(d), None) != 0, field
        assert b"res_map" in lib.cvmi_last_error(), field
        setattr(d, field, old)
    assert lib.cvmi_conv2d(C.byref(d), None) == 0
    torch.cuda.synchronize()


# ---- cvmi_attention with q_bmap / kv_bmap ----------------------------------------------------------------------------------------------------
ATTN_TABLE = [0, 1, 1, 0, 1]
MAP_ROWS = sorted({(s[0],) + s[3:] for s in SHARE_ROWS if s[1] == 2})          # (mode, heads, Nq, Nk, d, expected kernel) of the rows with two images


def _attn_desc(mode, H, Nq, Nk, d, dtype, q, k, v, table):
    """Descriptor and buffers of a 5-entry launch; table None: every operand has 5 batch entries."""
    td, B, C_ = TORCH_DTYPE[dtype], len(ATTN_TABLE), H * d
    qd = _tok(q).to(td).cuda().contiguous()
    kv = torch.cat((_tok(k), _tok(v)), -1).to(td).cuda().contiguous()
    od = torch.full((B + 1, Nq, C_), SENTINEL, dtype=td, device="cuda")
    es = kv.element_size()
    desc = _desc(q=qd.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr() + C_ * es, o=od.data_ptr(),
                 q_sb=Nq * C_, q_sh=d, q_st=C_, k_sb=Nk * 2 * C_, k_sh=d, k_st=2 * C_, v_sb=Nk * 2 * C_, v_sh=d, v_st=2 * C_,
                 o_sb=Nq * C_, o_sh=d, o_st=C_, B=B, heads=H, Nq=Nq, Nk=Nk, dqk=d, dv=d, scale=d ** -0.5, dtype=dtype,
                 q_bmap=table.data_ptr() if (table is not None and mode == "i2t") else None,
                 kv_bmap=table.data_ptr() if (table is not None and mode == "t2i") else None)
    return desc, (qd, kv, table), od


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("row", MAP_ROWS, ids=[r[0] for r in MAP_ROWS])
def test_attention_batch_map_equals_the_gathered_operand(row, dtype):
    mode, H, Nq, Nk, d, expect = row
    lib, B, imgs = _lib.load(), len(ATTN_TABLE), 2
    g = torch.Generator().manual_seed(7 + Nq)
    nq_b, nk_b = (B, imgs) if mode == "t2i" else (imgs, B)
    q = quant(torch.randn(nq_b, H, Nq, d, generator=g), dtype)
    k = quant(torch.randn(nk_b, H, Nk, d, generator=g), dtype)
    v = quant(torch.randn(nk_b, H, Nk, d, generator=g), dtype)
    tab = _i32(ATTN_TABLE)
    outs = {}
    for mapped in (True, False):
        qq, kk, vv = q, k, v
        if not mapped:
            if mode == "t2i":
                kk, vv = k[ATTN_TABLE], v[ATTN_TABLE]
            else:
                qq = q[ATTN_TABLE]
        desc, keep, od = _attn_desc(mode, H, Nq, Nk, d, dtype, qq, kk, vv, tab if mapped else None)
        tag, outs[mapped], same = _launch(desc, keep, od, lambda od=od: od.clone(), lib)
        assert tag == expect, (mapped, tag)
        assert same, "a second launch of the same plan differs"
        assert bool((od[-1] == SENTINEL).all()), "wrote past the last batch entry"
    assert torch.equal(outs[True], outs[False]), "table launch differs from the one on the gathered operand"
    assert bool((outs[True][:-1] != SENTINEL).all())


def test_attention_batch_map_rejects_window_f32_and_a_divisor():
    lib = _lib.load()
    mode, H, Nq, Nk, d, _ = next(r for r in MAP_ROWS if r[0] == "t2i")
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(n, H, t, d, generator=g) for n, t in ((5, Nq), (2, Nk), (2, Nk)))
    tab = _i32(ATTN_TABLE)
    desc, keep, od = _attn_desc(mode, H, Nq, Nk, d, F16, q, k, v, tab)
    torch.cuda.synchronize()
    assert lib.cvmi_attention(C.byref(desc), None) == 0
    torch.cuda.synchronize()
    for field, value in (("dtype", F32), ("kv_bdiv", 5), ("win", 8)):
        old = getattr(desc, field)
        setattr(desc, field, value)
        assert lib.cvmi_attention(C.byref(desc), None) != 0, field
        assert b"attention" in lib.cvmi_last_error()
        setattr(desc, field, old)
    desc.q_bmap, desc.q_bdiv = tab.data_ptr(), 5
    assert lib.cvmi_attention(C.byref(desc), None) != 0 and b"q_bmap" in lib.cvmi_last_error()
    torch.cuda.synchronize()


# ---- the model, f32 ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _model():
    from circuitvision_amd.sam2_infer import SAM2Model
    m = SAM2Model(MINI, R, dtype="f32", use_refinement=True).load_params(_params())
    assert m.pair_bucket == 32                                        # the default
    m.pair_bucket = 8
    return m


@functools.lru_cache(None)
def _oracle():
    _model()                                                          # (the packed model has read every tensor the oracle loads)
    p = _params()
    return mini_oracle(p, R), {**p.state_dict(), **p.mask_prompt_state_dict()}


@functools.lru_cache(None)
def _reference(name, kind, masked=False, multimask=False, half=False):
    """The per-image reference of a case, computed once and left unchanged: (high_res, low_res, iou, clear)."""
    oracle, sd = _oracle()
    c = ref.CASES[name]()
    if half:
        c["x"] = c["x"].half().float()
    return ref.predict_lists(oracle, sd, c, kind, masked=masked, multimask=multimask)


def _call(c, kind, **kw):
    return _model().infer_masks(c["x"], **ref.kind_args(c, kind), **kw)


def _check_lists(c, out, want, tol, squeeze=True, what=""):
    """Structure (lists of B tensors of the right shapes, views of one packed block) and values of a list call against the reference lists."""
    sizes = [int(t.shape[0]) for t in c["boxes"]]
    errs = []
    for got, wnt, tail in zip(out, want[:3], ((R, R), (F0, F0), ())):
        assert isinstance(got, list) and len(got) == len(sizes)
        base = got[0]._base
        assert base is not None and base.shape[0] == sum(sizes) and all(t._base is base for t in got), "not torch.split views of one packed block"
        for b, (t, w) in enumerate(zip(got, wnt)):
            w = w[:, 0] if squeeze else w
            assert t.shape == w.shape and t.shape[0] == sizes[b] and tuple(t.shape[t.dim() - len(tail):]) == tail, (b, t.shape, w.shape)
            errs.append(float((t.cpu() - w).abs().max()) if t.numel() else 0.0)
    print(f"{what}: max |got - reference| = {max(errs):.2e}")
    for got, wnt in zip(out, want[:3]):
        for t, w in zip(got, wnt):
            torch.testing.assert_close(t.cpu(), w[:, 0] if squeeze else w, **tol)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", ["counts_3_1", "counts_0_3", "b3"])
def test_lists_match_the_per_image_reference(name, kind):
    c = ref.CASES[name]()
    want = _reference(name, kind)
    out = _call(c, kind)
    top = [float(w.max()) for w in want[2] if w.numel()]
    err = max(float((t.cpu() - w[:, 0]).abs().max()) for t, w in zip(out[1], want[1]) if t.numel())
    print(f"{name} [{kind}]: reference selects clearly: {want[3]} (iou range {min(top):.3f} .. {max(top):.3f}); max |low_res - reference| = {err:.2e}")
    assert want[3], "a pair of this case is within rounding of another selection on the reference (selection_is_clear)"
    _check_lists(c, out, want, TOL32, what=f"{name} [{kind}] f32")
    if kind == "boxes":
        none, lo, iou = _call(c, kind, return_high_res=False)
        assert none is None and all(torch.equal(a, b) for a, b in zip(lo + iou, out[1] + out[2]))


def test_lists_with_mask_input_and_with_multimask():
    c = ref.CASES["counts_1_3"]()
    want = _reference("counts_1_3", "boxes", masked=True)
    assert want[3]
    out = _call(c, "boxes", mask_input=c["mask"])
    _check_lists(c, out, want, TOL32, what="counts_1_3 [boxes] mask_input f32")
    _, lo0, _ = _call(c, "boxes", return_high_res=False)
    assert float((torch.cat(out[1]) - torch.cat(lo0)).abs().max()) > 0.1                  # the mask prompt moves the logits
    _, lo_d, _ = _call(c, "boxes", mask_input=[m.cuda().double() for m in c["mask"]], return_high_res=False)      # device tensors of another float type
    assert all(torch.equal(a, b) for a, b in zip(lo_d, out[1]))
    want3 = _reference("counts_1_3", "boxes", multimask=True)
    out3 = _call(c, "boxes", multimask_output=True)
    assert [tuple(t.shape) for t in out3[1]] == [(1, 3, F0, F0), (3, 3, F0, F0)] and [tuple(t.shape) for t in out3[2]] == [(1, 3), (3, 3)]
    _check_lists(c, out3, want3, TOL32, squeeze=False, what="counts_1_3 [boxes] multimask f32")


def test_padding_slots_replay_and_both_caps():
    """cap > N (bucket 8) and cap == N (bucket 1) both meet the bound; a replay is bit-identical; so is a run after another call has left
    different prompts in the slots that are padding now."""
    model = _model()
    c = ref.CASES["counts_2_2"]()
    want = _reference("counts_2_2", "boxes")
    assert want[3]
    first = _call(c, "boxes")
    _check_lists(c, first, want, TOL32, what="counts_2_2 [boxes] cap 8 > N 4")
    again = _call(c, "boxes")
    assert all(torch.equal(a, b) for x, y in zip(first, again) for a, b in zip(x, y)), "replay differs"
    full = ref.case_counts((3, 3))                                    # 6 pairs in the same cap-8 plan: slots 4 and 5 hold real prompts now
    plan = model.plan(2, high_res=True, points=3, pairs=8)
    _call(full, "boxes")
    assert plan.pair_image.tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
    third = _call(c, "boxes")
    assert plan.pair_image.tolist() == [0, 0, 1, 1, 0, 0, 0, 0] and model.plan(2, high_res=True, points=3, pairs=8) is plan
    assert plan.coords[4:, :2].reshape(4, 4).tolist() == [[0.0, 0.0, R, R]] * 4
    assert all(torch.equal(a, b) for x, y in zip(first, third) for a, b in zip(x, y)), "the real pairs depend on what the padding slots held"
    assert plan.plan.graph is not None                                # one captured plan served all of it
    model.pair_bucket = 1
    try:
        exact = _call(c, "boxes")
        assert (2, 0, True, 3, 0, False, False, 4) in model._plans     # keyed on cap = N = 4
    finally:
        model.pair_bucket = 8
    _check_lists(c, exact, want, TOL32, what="counts_2_2 [boxes] cap 4 == N")


def test_tensor_form_is_undisturbed_and_equals_the_list_form_at_uniform_counts():
    model = _model()
    c = mref.mini_inputs(mref.MINI_SEED)
    before = model.infer_masks(c["x"], c["boxes"])
    lists = ref.case_counts((3, 3))
    for name in ("counts_3_1", "counts_0_3"):
        _call(ref.CASES[name](), "boxes")
    model.pair_bucket = 1
    try:
        got = _call(lists, "boxes")                                   # cap = N = B * P: the same launches on the same shapes
    finally:
        model.pair_bucket = 8
    after = model.infer_masks(c["x"], c["boxes"])
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "the tensor form changed after list calls"
    assert all(torch.is_tensor(t) and t.shape[:2] == (2, 3) for t in after)
    for t, l in zip(after, got):
        assert torch.equal(t, torch.stack(l)), "list form at uniform counts differs from the tensor form"


def test_list_errors():
    model = _model()
    c = ref.CASES["counts_2_2"]()
    x, bx = c["x"], c["boxes"]
    for kw in (dict(boxes=bx[:1]), dict(boxes=bx, points=c["points"][:1], point_labels=c["labels"][:1]), dict(boxes=bx, mask_input=[c["mask"][0], c["mask"][1][:1]]),
               dict(boxes=[bx[0][:0], bx[1][:0]]), dict(boxes=[bx[0], bx[1].tolist()]), dict(boxes=torch.stack(bx), mask_input=c["mask"]), dict(mask_input=c["mask"])):
        with pytest.raises(ValueError):
            model.infer_masks(x, **kw)
    with pytest.raises(ValueError):
        model.infer_masks(x[:, :, :R - 1], boxes=bx)


# ---- the plan, F16 -------------------------------------------------------------------------------------------------------------------------------
def _labels(sp):
    return [op[0] for op in sp.plan.ops]


@pytest.mark.parametrize("name", ["counts_3_1", "b3"])
def test_f16_plans_shared_and_unshared_match_the_reference_and_each_other(name, monkeypatch):
    from circuitvision_amd.sam2 import Sam2Plan, Sam2Weights
    c = ref.CASES[name]()
    x = c["x"].half().float()
    B = x.shape[0]
    rhi, rlo, riou, clear = _reference(name, "boxes", half=True)
    assert clear
    pk = pack_prompt_lists(B, R, boxes=c["boxes"], pair_bucket=8)
    N, cap = pk["N"], pk["cap"]
    wt = Sam2Weights(_params(), MINI, R, F16)
    outs, labels = {}, {}
    for share in ("1", "0"):
        monkeypatch.setenv("CVMI_SAM_SHARE_L0", share)
        sp = Sam2Plan(wt, B, torch.cuda.Stream(), pairs=cap)
        assert sp.share_l0 == (share == "1") and sp.pair_image.dtype == torch.int32 and sp.pair_image.shape == (cap,) and int(sp.pair_image.abs().max()) == 0
        sp.x_in.t.copy_(x.permute(0, 2, 3, 1).half())
        sp.coords.copy_(pk["coords"]); sp.labels.copy_(pk["labels"]); sp.pair_image.copy_(pk["pair_image"])
        torch.cuda.synchronize()
        sp.plan.run_eager()
        torch.cuda.synchronize()
        outs[share] = (sp.high_res[:N, 0].cpu(), sp.low_res[:N, 0].cpu(), sp.iou[:N, 0].cpu())
        labels[share] = _labels(sp)
        print(f"{name} F16 plan share_l0={share}: |low_res - reference| = {float((outs[share][1] - torch.cat(rlo)[:, 0]).abs().max()):.2e}")
        for got, want in zip(outs[share], (rhi, rlo, riou)):
            torch.testing.assert_close(got, torch.cat(want)[:, 0], **TOL16)
    for a, b in zip(outs["1"], outs["0"]):
        torch.testing.assert_close(a, b, **TOL16)
    # shared: neither pass; unshared: the gather where the repeat pass stands, which also writes layer 0's operand copy
    assert "gather_embed" not in labels["1"] and "repeat_embed" not in labels["1"] and "l0.t2i.castk" in labels["1"]
    assert "gather_embed" in labels["0"] and "repeat_embed" not in labels["0"] and "l0.t2i.castk" not in labels["0"]
    assert labels["0"].index("gather_embed") == labels["0"].index("embed") + 1
    assert [l for l in labels["0"] if l != "gather_embed"] == [l for l in labels["1"] if l != "l0.t2i.castk"]
    uniform = _labels(Sam2Plan(wt, B, torch.cuda.Stream(), prompts=3))
    assert "gather_embed" not in uniform and "repeat_embed" in uniform                     # (share_l0 is off here) prompts = P plans keep their launches
    with pytest.raises(ValueError):
        Sam2Plan(wt, B, torch.cuda.Stream(), prompts=3, pairs=8)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_without_a_prompt_cap(tmp_path):
    """max_prompts=None: every image returns as many masks as it has stage-2 boxes (more than the cap of 6 the same detector is cut to
    otherwise), an image without boxes none; masks and extents are `infer_masks` on the lists + `postprocess_to_mask` bit for bit; and
    max_prompts=6 still returns what the tensor form built by hand returns."""
    from circuitvision_amd.pipeline import CircuitPipeline
    from test_pipeline_gpu import _mini_setup
    images, det, yo, seg, tr, so, _ = _mini_setup(tmp_path, n_images=3)
    seg.pair_bucket = 8
    free, capped = CircuitPipeline(det, seg, tr, max_prompts=None), CircuitPipeline(det, seg, tr, max_prompts=6)
    bboxes = free.detect(images)
    bboxes[1] = []                                                    # an image without boxes
    assert max(len(b) for b in bboxes) > 6
    res = free.segment(images, bboxes, "boxes")
    x = tr.forward_batch(images, swap_rb=True)
    lists = [tr.transform_boxes(torch.tensor([[d["xmin"], d["ymin"], d["xmax"], d["ymax"]] for d in bb], dtype=torch.float32).reshape(-1, 4),
                                normalize=True, orig_hw=im.shape[:2]).reshape(-1, 4) for im, bb in zip(images, bboxes)]
    _, lo, iou = seg.infer_masks(x, lists, return_high_res=False)
    for b, (r, im, bb) in enumerate(zip(res, images, bboxes)):
        k = len(bb)
        assert r["bboxes"] == bb and r["masks"].shape == (k, *im.shape[:2]) and len(r["extents"]) == k and r["iou"].shape == (k,)
        assert torch.equal(r["iou"], iou[b])
        if k:
            u8, ext = tr.postprocess_to_mask(lo[b].unsqueeze(0), im.shape[:2])
            assert torch.equal(r["masks"], u8[0]) and r["extents"] == ext, b
            assert int((r["masks"] > 0).sum()) > 0
    assert res[1]["masks"].shape[0] == 0 and res[1]["extents"] == []
    # the capped pipeline: the tensor form on the lists cut at 6 and filled with their first box, as before
    resc = capped.segment(images, bboxes, "boxes")
    bx = torch.zeros(len(images), 6, 4)
    for b, l in enumerate(lists):
        bx[b] = torch.tensor([0.0, 0.0, 256, 256]) if l.shape[0] == 0 else torch.cat((l[:6], l[:1].repeat(max(0, 6 - l.shape[0]), 1)))
    _, lot, iout = seg.infer_masks(x, bx, return_high_res=False)
    for b, (r, im, bb) in enumerate(zip(resc, images, bboxes)):
        k = min(len(bb), 6)
        assert r["masks"].shape[0] == k and torch.equal(r["iou"], iout[b, :k])
        if k:
            u8, ext = tr.postprocess_to_mask(lot[b, :k].unsqueeze(0), im.shape[:2])
            assert torch.equal(r["masks"], u8[0]) and r["extents"] == ext, b
