"""The plan audit (tests/plan_audit.py) without a GPU.
  * every [label, kind, lane, kernel] of every case in tests/yolo_route_fixture.json resolves to an adapter or is `sync`, and the recorded kernel
    belongs to the adapter's family: a new launch kind without an adapter fails here;
  * every judge, on operands at one layer shape of YOLO11-n at 96 x 160 (values pre-rounded to fp16, as a snapshot holds them), passes chain32
    -- the same statement accumulated in fp32 -- as the "output" and fails the named mutants of fused_ref / helper_ref / detect_ref, a conv whose
    activation is applied after the residual, and a conv whose tap outside the image reads the neighbouring row;
  * the outside-the-view check catches one changed byte in a neighbouring channel slice and in another buffer (plain CPU tensors as buffers)."""
import json
import os

import pytest
import torch

import plan_audit as pa
import yolo_route_cases as rc
from circuitvision_amd import yolo_route as yr
from circuitvision_amd._lib import ACT_NONE, ACT_SILU

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "yolo_route_fixture.json")) as f:
    FIXTURE = json.load(f)["cases"]

F16, F32T = torch.float16, torch.float32
B = 2


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _x(g, *shape):
    return torch.randn(*shape, generator=g).to(F16)


def _w(g, n, cin, kh, kw, nchw=True):
    """fp16-valued float weight ~ 1 / sqrt(fan_in): NCHW [n, cin, kh, kw] for the fused references, [n, kh, kw, cin] (as stored) for conv."""
    w = (torch.randn(n, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5).to(F16)
    return w.float() if nchw else w.permute(0, 2, 3, 1).contiguous()


def _b(g, n):
    return 0.3 + 0.1 * torch.randn(n, generator=g)


# ---- the fixture resolves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_every_recorded_launch_has_an_adapter(case):
    lanes = 3 if case["lanes"] is None else case["lanes"]
    route = yr.route_yolo(case["scale"], rc.NC, rc.dtype_of(case["dtype"]), yr.YoloSwitches(*rc.switches_of(case)), lanes)
    seen = set()
    for op in FIXTURE[case["id"]]["ops"]:
        label, kind = op[0], op[1]
        adapter = pa.resolve(label, kind, route)
        assert (adapter is None) == (kind == "sync"), op
        if adapter is not None:
            assert adapter in pa.ADAPTERS and adapter in pa.JUDGES
            assert pa.kernel_fits(adapter, op[3] if len(op) > 3 else None), op
            seen.add(adapter)
    assert {"conv", "dwconv", "sppf_pool", "attention", "decode", "nms"} <= seen
    assert (set(pa.FUSED_FAMILY) <= seen) == (case["id"] in ("n_f16", "n_f16_160x224") or case["id"].startswith("n_f16_lanes"))


def test_a_launch_kind_without_an_adapter_raises():
    route = yr.route_yolo("n", rc.NC, rc.dtype_of("f16"), yr.YoloSwitches(True, True, True), 3)
    with pytest.raises(KeyError):
        pa.resolve("model.99.new", "layernorm", route)
    assert not pa.kernel_fits("conv", "c3k2_kernel<16, 8, 64, 32>") and not pa.kernel_fits("c3k2", "igemm_kernel<float, float, 64, 64, 2, 2, 64, true, 1>")


# ---- judges: chain32 passes, mutants fail -----------------------------------------------------------------------------------------------------
def _conv_case(which):
    g = _g(11)
    if which == "bottleneck":                                   # model.6.m.0.m.0.cv2: 3x3, 32 -> 32 on P4 (6 x 10), SiLU, residual
        i = dict(srcs=[_x(g, B, 6, 10, 32)], w=_w(g, 32, 32, 3, 3, nchw=False), bias=_b(g, 32), res=_x(g, B, 6, 10, 32))
        p = dict(stride=1, pad=1, OH=6, OW=10, ups=[0], act=ACT_SILU, act_after_res=0, out=F16, fast=True)
    elif which == "two_sources_up":                             # model.13.cv1: 1x1 over [model.10 upsampled | model.6], 384 -> 128 on P4
        i = dict(srcs=[_x(g, B, 3, 5, 256), _x(g, B, 6, 10, 128)], w=_w(g, 128, 384, 1, 1, nchw=False), bias=_b(g, 128), res=None)
        p = dict(stride=1, pad=0, OH=6, OW=10, ups=[1, 0], act=ACT_SILU, act_after_res=0, out=F16, fast=True)
    elif which == "stem_out_hw":                                # model.0 on the space-to-depth input: 2x2, pad 1, output cropped to 48 x 80
        i = dict(srcs=[_x(g, B, 48, 80, 16)], w=_w(g, 16, 16, 2, 2, nchw=False), bias=_b(g, 16), res=None)
        p = dict(stride=1, pad=1, OH=48, OW=80, ups=[0], act=ACT_SILU, act_after_res=0, out=F16, fast=True)
    elif which == "stride2":                                    # model.3: 3x3 / s2, 64 -> 64, P2 -> P3 (24 x 40 -> 12 x 20)
        i = dict(srcs=[_x(g, B, 24, 40, 64)], w=_w(g, 64, 64, 3, 3, nchw=False), bias=_b(g, 64), res=None)
        p = dict(stride=2, pad=1, OH=12, OW=20, ups=[0], act=ACT_SILU, act_after_res=0, out=F16, fast=True)
    else:                                                       # model.10.m.0.ffn.1 in f32 mode: 1x1, 256 -> 128 on P5, no activation, residual
        i = dict(srcs=[torch.randn(B, 3, 5, 256, generator=g)], w=_w(g, 128, 256, 1, 1, nchw=False).float(), bias=_b(g, 128), res=torch.randn(B, 3, 5, 128, generator=g))
        p = dict(stride=1, pad=0, OH=3, OW=5, ups=[0], act=ACT_NONE, act_after_res=0, out=F32T, fast=False)
    return i, p


@pytest.mark.parametrize("which", ["bottleneck", "two_sources_up", "stem_out_hw", "stride2", "f32_residual"])
def test_conv_judge_passes_chain32(which):
    i, p = _conv_case(which)
    ratio, idx, note = pa.judge_conv(i, p, pa.conv_stored(i, p, torch.float32))
    print(which, ratio, idx, note)
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", pa.CONV_MUTANTS)
def test_conv_judge_fails_the_mutants(mutant):
    i, p = _conv_case("bottleneck")
    ratio, idx, note = pa.judge_conv(i, p, pa.conv_stored(i, p, torch.float32, mutant))
    print(mutant, ratio, idx, note)
    assert ratio > 1.0
    if mutant == "tap_wraps_row":
        assert idx[2] == 9 and idx[1] < 5                       # the last column of a row that has a next row


def test_conv_statement_agrees_with_conv2d():
    """The unfold statement (two sources, upsample, stride, cropped output) against F.conv2d on the logical input."""
    import torch.nn.functional as Fn
    for which in ("two_sources_up", "stem_out_hw", "stride2", "bottleneck"):
        i, p = _conv_case(which)
        X = pa.conv_input(i["srcs"], p["ups"])
        got = pa.conv_sum(X, i["w"], p, torch.float64)
        ref = Fn.conv2d(pa.nchw(X).double(), i["w"].permute(0, 3, 1, 2).double(), stride=p["stride"], padding=p["pad"])[:, :, :p["OH"], :p["OW"]]
        assert float((got - pa.nhwc(ref)).abs().max()) < 1e-12, which
    up = pa.conv_input([torch.arange(4.0).view(1, 2, 2, 1)], [1])[0, :, :, 0]
    assert up.tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [2, 2, 3, 3]]


def _c3k2_case():                                               # model.2: 32 -> [16 | 16], hidden 8, out 64, on P2 (24 x 40)
    g = _g(12)
    i = dict(x=_x(g, B, 24, 40, 32), w0=_w(g, 32, 32, 1, 1), b0=_b(g, 32), w1=_w(g, 8, 16, 3, 3), b1=_b(g, 8), w2=_w(g, 16, 8, 3, 3), b2=_b(g, 16),
             w3=_w(g, 64, 48, 1, 1), b3=_b(g, 64))
    return i, dict(shortcut=True, fuse_cv1=True)


def _stem2_case():                                              # model.0 + model.1: 3 -> 16 -> 32 on a 96 x 160 image
    from circuitvision_amd.yolo11 import Yolo11Weights
    g = _g(13)
    img = torch.rand(B, 3, 96, 160, generator=g).to(F16)
    x = torch.zeros(B, 48, 80, 16, dtype=F16)
    x[..., :12] = img.reshape(B, 3, 48, 2, 80, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, 48, 80, 12)     # Yolo11Plan.set_input_nchw
    w3 = _w(g, 16, 3, 3, 3)
    w2 = torch.zeros(16, 16, 2, 2)
    m = {0: (0, 1), 1: (1, 0), 2: (1, 1)}                       # Yolo11Weights._stem
    for ky in range(3):
        for kx in range(3):
            (ty, sy), (tx, sx) = m[ky], m[kx]
            w2[:, (sy * 2 + sx) * 3:(sy * 2 + sx) * 3 + 3, ty, tx] = w3[:, :, ky, kx]
    assert torch.equal(pa.stem_weight_3x3(w2), w3) and torch.equal(pa.s2d_to_image(x), img) and Yolo11Weights._stem is not None
    return dict(x=x, w0=w2, b0=_b(g, 16), w1=_w(g, 32, 16, 3, 3), b1=_b(g, 32)), {}


def _dwpw_case():                                               # model.23.cv3.1.0: dw 3x3 on 128 channels + 1x1 128 -> 64, on P4
    g = _g(14)
    return dict(x=_x(g, B, 6, 10, 128), wd=_w(g, 128, 1, 3, 3), bd=_b(g, 128), w1=_w(g, 64, 128, 1, 1), b1=_b(g, 64)), {}


def _dwconv_case():                                             # model.10.m.0.attn.pe.h0: dw 3x3 on one head's 64 v channels, residual, on P5
    g = _g(15)
    return dict(x=_x(g, B, 3, 5, 64), w=_w(g, 64, 1, 3, 3), b=_b(g, 64), res=_x(g, B, 3, 5, 64)), dict(act="none", stored="f16")


FUSED = {"c3k2": (_c3k2_case, pa.c3k2_out, pa.judge_c3k2, ("no_shortcut", "rows_bleed")),
         "stem2": (_stem2_case, pa.stem2_out, pa.judge_stem2, ("rows_bleed",)),
         "dwpw": (_dwpw_case, pa.dwpw_out, pa.judge_dwpw, ("dw_first_chunk_taps", "rows_bleed")),
         "dwconv": (_dwconv_case, pa.dwconv_out, pa.judge_dwconv, ("dw_tail_reads_next_row",))}


@pytest.mark.parametrize("kind", list(FUSED))
def test_fused_and_dwconv_judges(kind):
    case, out, judge, mutants = FUSED[kind]
    i, p = case()
    ratio, idx, note = judge(i, p, out(i, p, torch.float32).to(F16))
    print(kind, "chain32", ratio, note)
    assert ratio <= 1.0
    for m in mutants:
        ratio, idx, note = judge(i, p, out(i, p, torch.float64, m).to(F16))
        print(kind, m, ratio, idx, note)
        assert ratio > 1.0, m


def test_dwconv_judge_in_f32_mode():
    i, p = _dwconv_case()
    i = {k: v.float() for k, v in i.items()}
    p = dict(act="silu", stored="f32")
    assert pa.judge_dwconv(i, p, pa.dwconv_out(i, p, torch.float32))[0] <= 1.0
    assert pa.judge_dwconv(i, p, pa.dwconv_out(i, p, torch.float64, "dw_tail_reads_next_row").float())[0] > 1.0


def test_sppf_judge():                                          # model.9.pool: 128 channels on P5; mostly negative, so a window clipped with 0 shows
    x = (torch.randn(B, 3, 5, 128, generator=_g(16)) * 1.5 - 2.0).to(F16)
    i = dict(x=x)
    assert pa.judge_sppf_pool(i, {}, pa.sppf_out(i, {}))[0] == 0.0
    ratio, idx, note = pa.judge_sppf_pool(i, {}, pa.sppf_out(i, {}, "sppf_clip_zero"))
    print(note)
    assert ratio > 1.0


def test_attention_judge():                                     # model.10.m.0.attn.sdpa: 2 heads, N = 15, key dim 32, head dim 64
    g = _g(17)
    i = dict(q=_x(g, B, 2, 15, 32), k=_x(g, B, 2, 15, 32), v=_x(g, B, 2, 15, 64))
    p = dict(scale=32 ** -0.5, out=F16)
    o32 = pa.attention_out(i, p, torch.float32)[0].to(F16)
    assert pa.judge_attention(i, p, o32)[0] <= 1.0
    unscaled = pa.attention_out(i, dict(p, scale=1.0), torch.float64)[0].to(F16)
    assert pa.judge_attention(i, p, unscaled)[0] > 1.0
    rolled = pa.attention_out(dict(i, v=i["v"].roll(1, 2)), p, torch.float64)[0].to(F16)          # every key's value taken from its neighbour
    assert pa.judge_attention(i, p, rolled)[0] > 1.0


def _decode_case():
    g = _g(18)
    return [((torch.randn(B, h, w, 64, generator=g) * 2).to(F16).float(), (torch.randn(B, h, w, 62, generator=g) * 2).to(F16).float())
            for h, w in ((12, 20), (6, 10), (3, 5))]


def _decode_got(pred):
    s, c = pred[:, 4:].max(1)
    return dict(pred=pred, best_score=s.reshape(-1).contiguous(), best_cls=c.int().reshape(-1).contiguous())


def test_decode_judge():
    import detect_ref
    levels = _decode_case()
    i, p = dict(levels=levels), dict(nc=62)
    c32 = detect_ref.decode_chain32(dict(nc=62), levels).float()
    assert pa.judge_decode(i, p, _decode_got(c32))[0] <= 1.0
    ratio, idx, note = pa.judge_decode(i, p, _decode_got(detect_ref.decode_ref(levels, mutant="anchor_no_half").float()))
    print(ratio, idx, note)
    assert ratio > 1.0 and idx[1] < 2                           # the centre rows
    last = _decode_got(c32)
    last["best_cls"] = last["best_cls"].flip(0)
    assert pa.judge_decode(i, p, last)[0] > 1.0                 # best class must be the first maximum of the kernel's own rows


def test_nms_judge():
    from oracle import nms as onms
    from synth import nms_stress_pred
    pred = nms_stress_pred(B, 62, (96, 160), seed=1)
    p = dict(conf=0.25, iou=0.7, max_det=300)
    det, idx = onms.yolo_nms(pred, 0.25, 0.7, 300, return_indices=True)
    assert min(d.shape[0] for d in det) >= 3
    got = dict(det=torch.zeros(B, 300, 6), det_idx=torch.zeros(B, 300, dtype=torch.int32), det_count=torch.tensor([d.shape[0] for d in det], dtype=torch.int32))
    for b in range(B):
        got["det"][b, :det[b].shape[0]] = det[b]
        got["det_idx"][b, :det[b].shape[0]] = idx[b].int()
    assert pa.judge_nms(dict(pred=pred), p, got)[0] == 0.0
    for key, b in (("det_count", 1), ("det_idx", 0), ("det", 1)):
        bad = {k: v.clone() for k, v in got.items()}
        if key == "det_count":
            bad[key][b] -= 1
        elif key == "det_idx":
            bad[key][b, :2] = bad[key][b, :2].flip(0)
        else:
            bad[key][b, 0, 0] += 0.5
        assert pa.judge_nms(dict(pred=pred), p, bad)[0] > 1.0, key


# ---- outside the view -------------------------------------------------------------------------------------------------------------------------
def test_ledger_catches_one_byte_outside_the_view():
    g = _g(19)
    concat = torch.randn(2, 3, 4, 12, generator=g).to(F16)      # a concat buffer: the launch writes channels [4, 8)
    other = torch.randn(2, 3, 4, 6, generator=g)                # another buffer (f32)
    count = torch.zeros(3, dtype=torch.int32)
    ledger = pa.Ledger([("concat", concat), ("other", other), ("count", count)])
    writes = [(concat, (4, 8))]
    assert ledger.changed_outside(writes) is None
    concat[..., 4:8] = 1.0                                       # the launch's own output: allowed, whatever it writes
    assert ledger.changed_outside(writes) is None

    def flip_byte(t, element):
        raw = t.view(-1).view(torch.uint8)
        raw[element * t.element_size()] ^= 1

    flip_byte(concat, concat[1, 2, 3].storage_offset() + 8)      # channel 8: the live neighbour right behind the view
    msg = ledger.changed_outside(writes)
    assert msg is not None and "concat" in msg and "(1, 2, 3, 8)" in msg and msg.startswith("1 bytes"), msg
    assert ledger.changed_outside(writes) is None               # the image follows: one report per change
    flip_byte(concat, concat[0, 0, 0].storage_offset() + 3)      # channel 3: right in front of it
    assert "(0, 0, 0, 3)" in ledger.changed_outside(writes)
    flip_byte(other, 17)
    msg = ledger.changed_outside(writes)
    assert msg is not None and "other" in msg, msg
    count[2] = 1
    assert "count" in ledger.changed_outside(writes)
    count[2] = 5
    assert ledger.changed_outside(writes + [(count, None)]) is None
    with pytest.raises(KeyError):
        ledger.changed_outside([(torch.zeros(3), None)])
