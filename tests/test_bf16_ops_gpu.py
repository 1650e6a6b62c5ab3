"""The bf16 build (-DCVMI_OPERAND_BF16, common.hpp) op by op: every dual-built entry point that has no bf16 test elsewhere (tests/op_matrix.py
BF16_OPS), against a float64 or exact reference on operands pre-rounded to bf16.  Exact ops (pooling, layout changes, casts, the bf16 copies
of f32 results) are compared bit for bit; arithmetic at bounds stated in units of bf16's unit roundoff u = 2^-8."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from circuitvision_amd import _lib
from circuitvision_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, Buf, PackedConv, Plan, op_conv, op_layernorm, op_maxpool2
from helper_ref import _check_ln, _ln_ref
from helpers import TOL, from_view, quant, run, stream, to_buf

pytestmark = pytest.mark.gpu
ACT_FN = {ACT_NONE: lambda x: x, ACT_SILU: F.silu, ACT_RELU: F.relu, ACT_GELU: F.gelu}
SENTINEL = -12288.0


class _ConstRes:
    """Constant [rows, C] device tensor posing as a residual view (ptr, ld), as the SAM 2 plan passes positional tables."""

    def __init__(self, t):
        self.t, self.c = t, t.shape[-1]

    ptr = property(lambda s: s.t.data_ptr())
    ld = property(lambda s: s.c)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


# ---- cvmi_conv2d ------------------------------------------------------------------------------------------------------
def _conv_bf16(B, Cin, H, W, Cout, k, s, act, res=None, pad=None, out_hw=None, out_f32=False, expect=None, seed=0):
    """One bf16 convolution vs float64 conv2d of the rounded operands.  res: None, "full" (a per-pixel residual of the output type) or
    "bcast" (one [OH * OW, Cout] table shared by every image: res_mod)."""
    g = torch.Generator().manual_seed(seed + Cin * 7 + Cout)
    x = quant(torch.randn(B, Cin, H, W, generator=g), BF16)
    w = quant(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5, BF16)
    b = torch.randn(Cout, generator=g)
    pad = k // 2 if pad is None else pad
    if k == 1 and s == 1 and pad == 0:                   # 1x1: one BLAS GEMM (float64 conv2d on the CPU has no fast path)
        y = torch.einsum("bchw,nc->bnhw", x.double(), w.double()[:, :, 0, 0]) + b.double().view(1, -1, 1, 1)
    else:
        y = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=pad)
    if out_hw is not None:
        y = y[..., :out_hw[0], :out_hw[1]]
    OH, OW = y.shape[2:]
    odt = F32 if out_f32 else BF16
    kw = {}
    if res == "full":
        r = quant(torch.randn(B, Cout, OH, OW, generator=g), odt)
        rb = to_buf(r, odt)
        kw = dict(res=rb.view())
        ref = ACT_FN[act](y) + r.double()                  # act_after_res = 0: the activation, then the residual
    elif res == "bcast":
        r = quant(torch.randn(OH * OW, Cout, generator=g), odt)
        kw = dict(res=_ConstRes(r.to(TORCH_DTYPE[odt]).cuda()), res_mod=OH * OW)
        ref = ACT_FN[act](y) + r.t().reshape(1, Cout, OH, OW).double()
    else:
        ref = ACT_FN[act](y)
    xb = to_buf(x, BF16)
    yb = Buf(B, OH, OW, Cout, odt)
    yb.t.fill_(SENTINEL)
    plan = Plan(stream())
    op_conv(plan, "t", PackedConv(w, b, BF16), [(xb.view(), 0)], yb.view(), stride=s, pad=pad, act=act, out_hw=out_hw,
            scalar_gather=(Cin % 8 != 0), **kw)
    lib = _lib.load()
    lib.cvmi_last_kernel()
    run(plan)
    tag = lib.cvmi_last_kernel().decode()
    got = from_view(yb.view())
    err = float((got.double() - ref).abs().max())
    print(f"conv bf16 {B}x{Cin}x{H}x{W} -> {Cout} k{k} s{s} res={res} f32out={out_f32}: {tag}  max|err| {err:.3e}")
    if expect is not None:
        assert tag == expect, tag
    torch.testing.assert_close(got.double(), ref, **TOL[BF16])
    first = yb.t.clone()
    run(plan)
    assert torch.equal(yb.t, first)


@pytest.mark.parametrize("cfg", [
    # B, Cin, H, W, Cout, k, s, act, res, out_f32, expected kernel (None: any)
    (2, 256, 16, 16, 256, 1, 1, ACT_NONE, None, False, None),                   # 1x1 neck conv
    (2, 64, 17, 13, 64, 3, 1, ACT_GELU, "full", False, None),                   # 3x3 + residual, odd spatial size
    (1, 32, 20, 24, 96, 3, 2, ACT_RELU, None, False, None),                     # 3x3 stride 2
    (3, 256, 8, 8, 256, 1, 1, ACT_NONE, "bcast", False, None),                  # broadcast residual (the decoder's kv_pe / q_pe tables)
    (2, 96, 12, 10, 144, 1, 1, ACT_NONE, "full", True, None),                   # f32 output + f32 residual
    (1, 8, 9, 7, 16, 3, 1, ACT_SILU, None, False, None),                        # tiny channels: K = 72 -> Kpad 96
    (1, 12, 9, 7, 16, 3, 1, ACT_NONE, None, False, None),                       # Cin = 12: scalar gather
    (1, 256, 256, 256, 256, 1, 1, ACT_NONE, "full", False, "gemm256_kernel<__bf16, true>"),     # 256 x 256 counted-DMA GEMM
    (1, 256, 256, 256, 256, 1, 1, ACT_NONE, None, False, "gemm256p_kernel"),                   # its persistent form (no residual)
    (1, 256, 256, 256, 192, 1, 1, ACT_SILU, None, False, "gemm_glds_kernel<__bf16, __bf16, 128, 64, 2, 2>"),   # direct-to-LDS GEMM
    (2, 256, 20, 20, 64, 3, 1, ACT_SILU, None, False, "igemm_kernel<__bf16, __bf16, 64, 64, 2, 2, 64, false, 4>"),   # split-K: 4 groups
    (3, 384, 20, 20, 128, 1, 1, ACT_SILU, None, False, "igemm_kernel<__bf16, __bf16, 64, 128, 2, 2, 64, true, 2>"),  # split-K: 2 groups
])
def test_conv2d_bf16(cfg):
    B, Cin, H, W, Cout, k, s, act, res, out_f32, expect = cfg
    _conv_bf16(B, Cin, H, W, Cout, k, s, act, res=res, out_f32=out_f32, expect=expect)


def test_conv2d_bf16_patch_embed():
    """Hiera's 7 x 7 / stride 4 patch embedding as the SAM 2 plan runs it: space_to_depth(4) of the image, a 2 x 2 conv over 48 channels with pad 1
    cropped to out_hw, f32 output + the positional table broadcast to every image (res_mod)."""
    g = 16
    _conv_bf16(2, 48, g, g, 144, 2, 1, ACT_NONE, res="bcast", pad=1, out_hw=(g, g), out_f32=True)


def test_conv2d_bf16_transpose_shuffle():
    """The decoder's ConvTranspose 2 x 2 / stride 2 as a 1x1 conv scattered to 2 x 2 output pixels (shuffle_cout), the skip feature shared by the
    prompts of one image (res_rep) and GELU after the residual (act_after_res), all in bf16."""
    g = torch.Generator().manual_seed(3)
    x = quant(torch.randn(6, 64, 6, 5, generator=g), BF16)
    w = quant(torch.randn(64, 32, 2, 2, generator=g) / 8, BF16)
    b = torch.randn(32, generator=g)
    skip = quant(torch.randn(2, 32, 12, 10, generator=g), BF16)
    ref = F.gelu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2) + skip.double().repeat_interleave(3, 0))
    pc = PackedConv(w.permute(2, 3, 1, 0).reshape(128, 64, 1, 1), b.repeat(4), BF16)
    xb, sb = to_buf(x, BF16), to_buf(skip, BF16)
    yb = Buf(6, 12, 10, 32, BF16, zero=True)
    plan = Plan(stream())
    op_conv(plan, "ct", pc, [(xb.view(), 0)], yb.view(), act=ACT_GELU, res=sb.view(), shuffle_cout=32, act_after_res=True, res_rep=3)
    run(plan)
    torch.testing.assert_close(from_view(yb.view()).double(), ref, **TOL[BF16])


def test_conv2d_bf16_rejects_bad_arguments():
    """A configuration the bf16 build cannot run is refused cleanly: nonzero return and a message."""
    lib = _lib.load()
    x = Buf(1, 4, 4, 12, BF16, zero=True)              # 12 channels without scalar gather: not a multiple of 8
    y = Buf(1, 4, 4, 16, BF16, zero=True)
    d = op_conv(Plan(stream()), "bad", PackedConv(torch.zeros(16, 12, 1, 1), None, BF16), [(x.view(), 0)], y.view())
    torch.cuda.synchronize()
    assert lib.cvmi_conv2d(C.byref(d), None) != 0
    assert b"multiples" in lib.cvmi_last_error()


# ---- cvmi_layernorm / cvmi_layernorm_dual ---------------------------------------------------------------------------
@pytest.mark.parametrize("din,dout", [(F32, BF16), (BF16, BF16), (BF16, F32)])
@pytest.mark.parametrize("C_,act", [(16, ACT_NONE), (64, ACT_GELU), (144, ACT_NONE), (256, ACT_NONE), (1152, ACT_NONE)])
def test_layernorm_bf16(din, dout, C_, act):
    g = torch.Generator().manual_seed(C_ + 3)
    x = quant(torch.randn(3, 5, 7, C_, generator=g) * 3 + 1, din)
    gam, bet = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    ref, scale = _ln_ref(x, gam, bet, 1e-6, act)
    xb = Buf(3, 5, 7, C_, din); xb.t.copy_(x.to(TORCH_DTYPE[din]))
    yb = Buf(3, 5, 7, C_, dout); yb.t.fill_(SENTINEL)
    plan = Plan(stream())
    op_layernorm(plan, "ln", xb.view(), gam.cuda(), bet.cuda(), yb.view(), 1e-6, act)
    run(plan)
    _check_ln(yb.t.cpu(), ref, scale, dout, f"layernorm {din}->{dout} C={C_} act={act}")


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_layernorm_padded_grid(dt):
    """pad = (H, W, Hp, Wp): the rows are the pixels of [*, H, W] images and land in a [*, Hp, Wp] grid (Hiera's pad to a window multiple).
    The header's contract: the caller's grid is zero-initialised and its padding "stays 0" -- the kernel writes the valid region only.  So:
    (1) on a sentinel-filled grid the valid region matches the reference and every padding row still holds the sentinel (no row lands
    elsewhere); (2) on a zero-filled grid, as the SAM 2 plan allocates it, the whole grid equals the zero-padded reference."""
    C_, imgs, H, W, Hp, Wp = 144, 2, 5, 7, 8, 8
    g = torch.Generator().manual_seed(9)
    x = quant(torch.randn(imgs, H, W, C_, generator=g) * 2 - 1, dt)
    gam, bet = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    ref, scale = _ln_ref(x, gam, bet, 1e-6, ACT_NONE)
    xb = Buf(imgs, H, W, C_, dt); xb.t.copy_(x.to(TORCH_DTYPE[dt]))
    for fill in (SENTINEL, 0.0):
        yb = Buf(imgs, Hp, Wp, C_, dt); yb.t.fill_(fill)
        plan = Plan(stream())
        op_layernorm(plan, "ln_pad", xb.view(), gam.cuda(), bet.cuda(), yb.view(), 1e-6, pad=(H, W, Hp, Wp))
        run(plan)
        got = yb.t.cpu()
        _check_ln(got[:, :H, :W], ref, scale, dt, f"layernorm padded grid {dt} fill {fill}")
        pad_mask = torch.ones(imgs, Hp, Wp, dtype=torch.bool)
        pad_mask[:, :H, :W] = False
        assert bool((got[pad_mask].float() == fill).all()), "a padding row of the grid was written"


def test_layernorm_dual_bf16_copy():
    """f32 stream -> f32 result + a bf16 operand copy in one pass: the copy is the f32 result rounded to nearest even, bit for bit."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, 11, 256, generator=g) * 2 - 0.5
    gam, bet = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    ref, _ = _ln_ref(x, gam, bet, 1e-5, ACT_NONE)
    xb = Buf(2, 9, 11, 256, F32); xb.t.copy_(x)
    yb = Buf(2, 9, 11, 256, BF16); yb.t.fill_(SENTINEL)
    plan = Plan(stream())
    op_layernorm(plan, "ln", xb.view(), gam.cuda(), bet.cuda(), xb.view(), 1e-5, dst2=yb.view())
    run(plan)
    torch.testing.assert_close(xb.t.cpu().double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(_bits(yb.t.cpu()), _bits(xb.t.cpu().to(torch.bfloat16)))


# ---- pooling and layout ----------------------------------------------------------------------------------------------
def test_maxpool_and_space_to_depth_bf16():
    """cvmi_maxpool2x2 and cvmi_space_to_depth4 in bf16: bit-exact (including -0, the largest finite value and a column wider than C)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    x = quant(torch.randn(2, 24, 8, 12, generator=g) * 100, BF16)
    x[0, 0, 0, 0], x[0, 1, 2, 2] = 3.3895313892515355e38, -0.0
    xb = to_buf(x, BF16, c_total=32)
    yb = Buf(2, 4, 6, 40, BF16); yb.t.fill_(SENTINEL)
    plan = Plan(stream())
    op_maxpool2(plan, "mp", xb.view(0, 24), yb.view(8, 24))
    run(plan)
    ref = F.max_pool2d(x, 2, 2)
    assert torch.equal(_bits(yb.t[..., 8:32].cpu()), _bits(ref.permute(0, 2, 3, 1).to(torch.bfloat16)))
    assert bool((yb.t[..., :8] == SENTINEL).all()) and bool((yb.t[..., 32:] == SENTINEL).all())
    img = quant(torch.randn(3, 16, 20, 3, generator=g) * 2, BF16).to(torch.bfloat16).cuda()
    out = torch.full((3, 4, 5, 48), SENTINEL, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_space_to_depth4(img.data_ptr(), out.data_ptr(), 3, 16, 20, BF16, None), "s2d4")
    torch.cuda.synchronize()
    ref = img.cpu().view(3, 4, 4, 5, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(3, 4, 5, 48)      # channel = (sy * 4 + sx) * 3 + c
    assert torch.equal(_bits(out.cpu()), _bits(ref))


def _cast_launch(x, xdt, ydt, rows, C_, x_ld, y_ld):
    lib = _lib.load()
    y = torch.full((rows, y_ld), SENTINEL, dtype=TORCH_DTYPE[ydt], device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_cast(x.data_ptr(), x_ld, xdt, y.data_ptr(), y_ld, ydt, rows, C_, None), "cast")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[:, C_:].float() == SENTINEL).all())
    return y[:, :C_]


def _crafted_f32():
    """f32 bit patterns at bf16's rounding decisions: ties (low half 0x8000) with an even and an odd upper half, one below / above the tie,
    carries into the next binade, +-0, the largest finite bf16 and its neighbours."""
    pats = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x404A, 0xBF80, 0xBF81, 0x0080, 0x7F7E, 0x3F7F, 0x407F, 0xC07F):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
            pats.append((hi << 16) | lo)
    pats += [0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF, 0xFF7F7FFF]
    return torch.tensor(pats, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_cast_bf16():
    """cvmi_cast F32 -> BF16 is round-to-nearest-even, bit-identical to torch's conversion, on random values and crafted rounding decisions;
    BF16 -> F32 and BF16 -> BF16 are exact.  Edges beyond that, as the kernel handles them (measured, asserted here):
      - f32 subnormals: kept as bf16 subnormals, rounded to nearest even like every other value (no flush to zero);
      - values that round past the largest finite bf16 (>= 0x7F7F8000): become +-inf, as IEEE rounding and torch give."""
    g = torch.Generator().manual_seed(1)
    rnd = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-30, 30, (4096,), generator=g).float())
    sub = torch.tensor([0x00000001, 0x00007FFF, 0x00008000, 0x00018000, 0x007F8000, 0x007FFFFF, 0x80008000, 0x80400000],
                       dtype=torch.int64).to(torch.int32).view(torch.float32)
    over = torch.tensor([0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF], dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat((rnd, _crafted_f32(), sub, over))
    n = x.numel()
    rows, C_ = 2, n // 2
    xs = x[:rows * C_].view(rows, C_)
    xd = torch.zeros(rows, C_ + 4).cuda()
    xd[:, :C_] = xs.cuda()
    got = _cast_launch(xd, F32, BF16, rows, C_, C_ + 4, C_ + 8)
    want = xs.to(torch.bfloat16)
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, [(hex(int(xs.view(torch.int32)[r, c]) & 0xFFFFFFFF), hex(int(_bits(got)[r, c]) & 0xFFFF),
                               hex(int(_bits(want)[r, c]) & 0xFFFF)) for r, c in bad[:12].tolist()]
    assert bool(torch.isinf(got.float()[torch.isin(xs, over)]).all())
    # bf16 -> f32 and bf16 -> bf16: exact (every bf16 pattern but NaNs)
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    allb = allb[~torch.isnan(allb.float())]
    m = allb.numel() // 4 * 4
    bsrc = allb[:m].view(4, m // 4).cuda()
    got32 = _cast_launch(bsrc, BF16, F32, 4, m // 4, m // 4, m // 4 + 4)
    assert torch.equal(_bits(got32), _bits(bsrc.cpu().float()))
    got16 = _cast_launch(bsrc, BF16, BF16, 4, m // 4, m // 4, m // 4 + 8)
    assert torch.equal(_bits(got16), _bits(bsrc.cpu()))


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, BF16), (BF16, F32)])
def test_nchw_to_nhwc_bf16(src, dst):
    """cvmi_nchw_to_nhwc with a bf16 side: a permutation plus (F32 -> BF16) a round-to-nearest-even, bit-identical to torch, into a wider
    destination row whose extra channels keep their sentinel."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 10, 14, generator=g) * 3
    x.view(-1)[:len(_crafted_f32())] = _crafted_f32()
    xs = x.to(TORCH_DTYPE[src]).cuda()
    ld = 8
    y = torch.full((2, 10, 14, ld), SENTINEL, dtype=TORCH_DTYPE[dst], device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_nchw_to_nhwc(xs.data_ptr(), src, y.data_ptr(), dst, ld, 2, 3, 10, 14, None), "nchw_to_nhwc")
    torch.cuda.synchronize()
    want = xs.cpu().permute(0, 2, 3, 1).to(TORCH_DTYPE[dst])
    assert torch.equal(_bits(y[..., :3].cpu()), _bits(want))
    assert bool((y[..., 3:] == SENTINEL).all())


# ---- mask decoder pieces -------------------------------------------------------------------------------------------------
def test_prompt_tokens_bf16():
    """cvmi_prompt_tokens with dtype BF16: the f32 tokens at the oracle bound of the fp16 test, the bf16 copy == the f32 tokens rounded
    to nearest even, bit for bit."""
    from oracle import sam2_model as osam
    lib = _lib.load()
    pe = osam.randomize_(osam.PromptEncoder(256, 1024), seed=4, std=0.5).eval()
    g = torch.Generator().manual_seed(1)
    out_tokens = torch.randn(6, 256, generator=g)
    n, K = 37, 3
    coords = torch.rand(n, K, 2, generator=g) * 1024
    labels = torch.randint(-1, 4, (n, K), generator=g).int()
    with torch.no_grad():
        ref = pe.embed_points(coords, labels.long(), pad=False)
    ref = torch.cat((out_tokens[None].expand(n, -1, -1), ref), 1)
    table = torch.cat([pe.not_a_point_embed.weight] + [e.weight for e in pe.point_embeddings], 0).detach().contiguous().cuda()
    gauss = pe.pe_layer.positional_encoding_gaussian_matrix.contiguous().cuda()
    cd, ld, od = coords.cuda(), labels.cuda(), out_tokens.cuda()
    t32 = torch.zeros(n, 6 + K, 256, device="cuda")
    tlp = torch.full((n, 6 + K, 256), SENTINEL, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_prompt_tokens(cd.data_ptr(), ld.data_ptr(), gauss.data_ptr(), od.data_ptr(), table.data_ptr(), 1024.0,
                                      t32.data_ptr(), tlp.data_ptr(), BF16, n, K, 6, None), "prompt_tokens")
    torch.cuda.synchronize()
    torch.testing.assert_close(t32.cpu(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(_bits(tlp.cpu()), _bits(t32.cpu().to(torch.bfloat16)))


def test_hyper_masks_bf16():
    """cvmi_hyper_masks with bf16 up-scaled features: masks = hyper [B, 4, C] (f32) x up [B, P, C] (bf16) vs float64 on the same values.  Every
    product is exact in fp32; the fp32 chain of C fused multiply-adds errs by at most C u32 sum_c |h_c up_c| (u32 = 2^-24).  The areas (mask 0
    above +delta / above -delta) must be exact for every prompt none of whose mask-0 values lies within that bound of +-delta."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    B, P, Cc, up_ld, delta = 4, 1000, 32, 40, 0.05
    up = quant(torch.randn(B, P, Cc, generator=g), BF16)
    hyper = torch.randn(B, 4, Cc, generator=g) * 0.3
    hyper[1, 0] *= 1e-2
    ref = hyper.double() @ up.double().transpose(1, 2)
    bound = Cc * 2.0 ** -24 * (hyper.double().abs() @ up.double().abs().transpose(1, 2)) + 1e-30
    upd = torch.zeros(B, P, up_ld, dtype=torch.bfloat16)
    upd[..., :Cc] = up.to(torch.bfloat16)
    upd = upd.cuda()
    hd = hyper.cuda()
    masks = torch.full((B, 4, P), SENTINEL, device="cuda")
    areas = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.cvmi_hyper_masks(hd.data_ptr(), Cc, upd.data_ptr(), up_ld, BF16, Cc, masks.data_ptr(), areas.data_ptr(), B, P, delta, None), "hm")
    torch.cuda.synchronize()
    err = (masks.cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"hyper_masks bf16: max|err| {float(err.max()):.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    m0, b0 = ref[:, 0], bound[:, 0]
    clear = ~(((m0 - delta).abs() <= b0) | ((m0 + delta).abs() <= b0)).any(1)
    assert int(clear.sum()) >= B - 1
    want = torch.stack(((m0 > delta).sum(1), (m0 > -delta).sum(1)), 1).int()
    got = areas.cpu()
    assert torch.equal(got[clear], want[clear]), (got, want)
