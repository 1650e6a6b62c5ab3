"""GPU parity of the proj + MLP launch (csrc/proj_mlp.hpp): x <- x1 + mlp(norm2(x1)), x1 = x + ao Wp^T + bp, in one launch, against an fp64
statement of the same arithmetic and against the two launches it replaces; and the plan that takes it for Hiera's stages 1 - 2."""
import functools

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import (Buf, PackedHieraMlp, PackedProjMlp, PackedTokLinear, Plan, TORCH_DTYPE, op_hiera_mlp, op_tok_linear)
from helpers import run, stream
from proj_mlp_cases import PROJ_MLP_ROWS

pytestmark = pytest.mark.gpu


def _q(t, dt):
    return t.to(TORCH_DTYPE[dt]).double()


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("row", PROJ_MLP_ROWS, ids=[r["id"] for r in PROJ_MLP_ROWS])
def test_proj_mlp_fused_vs_fp64_and_the_two_launches(row, dt):
    """Reference: fp64 on the operands rounded to the 16-bit type -- x1 = x + ao Wp^T + bp, then the MLP as test_hiera_mlp_fused_vs_torch states
    it (normalised row and hidden activation rounded to the operand type) -- at that test's tolerance (3e-3 fp16 / 2.4e-2 bf16).  The pair of
    launches the fused one replaces, on the same inputs, must agree within the same tolerance (a packing mistake the reference construction
    could share shows there).  x has a row stride of C + 4 with NaN padding, a NaN row block in front and three rows behind; ao a stride of
    C + 8 with NaN padding: whatever is not an updated value must be bit-unchanged, ao included."""
    C_, rows = row["C"], row["rows"]
    td = TORCH_DTYPE[dt]
    g = torch.Generator().manual_seed(C_ + rows)
    x = torch.randn(rows + 3, C_, generator=g) * 1.5 + 0.3
    ao = (torch.randn(rows, C_, generator=g)).to(td)
    gam, bet = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.2
    wp = torch.randn(C_, C_, generator=g) / C_ ** 0.5
    bp = torch.randn(C_, generator=g) * 0.3
    w1 = torch.randn(4 * C_, C_, generator=g) / C_ ** 0.5
    b1 = torch.randn(4 * C_, generator=g) * 0.3
    w2 = torch.randn(C_, 4 * C_, generator=g) / (4 * C_) ** 0.5
    b2 = torch.randn(C_, generator=g) * 0.3
    # ---- fp64 reference
    x1 = x[:rows].double() + ao.double() @ _q(wp, dt).t() + bp.double()
    xn = _q(torch.nn.functional.layer_norm(x1, (C_,), gam.double(), bet.double(), 1e-6), dt)
    hid = _q(torch.nn.functional.gelu(xn @ _q(w1, dt).t() + b1.double()), dt)
    ref = x1 + hid @ _q(w2, dt).t() + b2.double()
    # ---- the fused launch
    xb = Buf(2, 1, rows + 3, C_ + 4, F32)
    xb.t.fill_(float("nan"))
    xb.t[1, 0, :, :C_] = x.cuda()
    x0 = xb.t.clone()
    aob = Buf(1, 1, rows, C_ + 8, dt)
    aob.t.fill_(float("nan"))
    aob.t[0, 0, :, :C_] = ao.cuda()
    ao0 = aob.t.clone()
    view = xb.images(1, 1).view(0, C_)
    view.buf.W = rows                                             # the op covers the first `rows` rows only
    pm = PackedProjMlp(wp, bp, w1, b1, w2, b2, dtype=dt)
    stats = torch.full((rows, 2), -7.0, device="cuda")
    plan = Plan(stream())
    op_hiera_mlp(plan, "projmlp", None, view, gam.cuda(), bet.cuda(), 1e-6, stats_out=stats, stats_eps=1e-6, proj=(pm, aob.view(0, C_)))
    lib = _lib.load()
    lib.cvmi_last_kernel()
    run(plan)
    assert lib.cvmi_last_kernel().decode() == row["expect"]
    out, stats1 = xb.t.clone(), stats.clone()
    got = out[1, 0, :rows, :C_].cpu().double()
    # untouched memory: the NaN block in front, the padding columns, the rows behind `rows`; ao
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(out[0], x0[0]) and same(out[1, 0, :, C_:], x0[1, 0, :, C_:]) and same(out[1, 0, rows:], x0[1, 0, rows:])
    assert torch.equal(aob.t.view(torch.int16), ao0.view(torch.int16))
    assert torch.isfinite(got).all()
    tol = 3e-3 if dt == F16 else 2.4e-2
    err = (got - ref).abs().max().item()
    print(f"{row['id']} {'f16' if dt == F16 else 'bf16'}: max |fused - fp64| {err:.3e}")
    # forwarded statistics of the updated rows
    g32 = out[1, 0, :rows, :C_].cpu()
    exp_stats = torch.stack((g32.mean(1), 1.0 / torch.sqrt(g32.var(1, unbiased=False) + 1e-6)), 1)
    # ---- the two launches, on the same inputs (op_tok_linear takes whole 256-row workgroups: the rows are padded with finite values)
    R = (rows + 255) // 256 * 256
    xc = Buf(1, 1, R, C_, F32)
    xc.t.fill_(0.25)
    xc.t[0, 0, :rows] = x[:rows].cuda()
    ac = Buf(1, 1, R, C_, dt)
    ac.t.fill_(0.5)
    ac.t[0, 0, :rows] = ao.cuda()
    chain = Plan(stream())
    op_tok_linear(chain, "proj", PackedTokLinear(wp, bp, dtype=dt), ac.view(), xc.view(), residual=True)
    op_hiera_mlp(chain, "mlp", PackedHieraMlp(w1, b1, w2, b2, dtype=dt), xc.view(), gam.cuda(), bet.cuda(), 1e-6)
    run(chain)
    two = xc.t[0, 0, :rows].cpu().double()
    err2 = (got - two).abs().max().item()
    print(f"{row['id']}: max |fused - two launches| {err2:.3e}, max |two launches - fp64| {(two - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, rtol=tol, atol=tol)
    torch.testing.assert_close(got, two, rtol=tol, atol=tol)
    torch.testing.assert_close(stats.cpu(), exp_stats, rtol=2e-5, atol=2e-5)
    # ---- replay on restored inputs: outputs and forwarded statistics bit-identical
    xb.t.copy_(x0)
    stats.fill_(-7.0)
    run(plan)
    assert same(xb.t, out) and same(stats, stats1)


MINI144 = dict(embed_dim=144, num_heads=2, stages=(1, 2, 3, 2), global_att_blocks=(4,), window_spec=(8, 4, 16, 8))


@functools.lru_cache(maxsize=None)
def _mini144(dtype):
    """The mini Hiera of test_sam2_wrapper_mini_matches_oracle (same stages, windows, global block and LoRA targets) at the stage widths the
    launch is built for (144 / 288 / ..): at embed_dim 16 no block has a fused MLP.  256^2 input: 64 x 64 and 32 x 32 token grids, whole
    8 x 8 / 4 x 4 windows -- stages 1 - 2 are unpadded."""
    import oracle.sam2_model as osam
    from circuitvision_amd.sam2 import Sam2Weights, SamSyntheticParams
    from test_oracle_sam2_cpu import mini_targets
    p = SamSyntheticParams(seed=5, lora_targets=mini_targets(), std=0.05)
    wt = Sam2Weights(p, MINI144, 256, dtype)
    core = osam.SAM2Core(MINI144, lora=True, lora_trunk={3: ("attn.qkv", "mlp.layers.0", "proj"), 5: ("attn.qkv",)}, image_size=256)
    w = osam.SAM2ImageWrapper(core).eval()
    w.load_state_dict({("sam2_model." + k if not (k.startswith("dense_") or k.startswith("sparse_") or k.startswith("refinement_")) else k): v
                       for k, v in p.state_dict().items()}, strict=True)
    x = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(TORCH_DTYPE[dtype]).float()
    with torch.no_grad():
        hi, lo, iou, inter = w(x, return_intermediates=True)
    return wt, x, (hi, lo, iou, inter)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_sam2_plan_takes_the_fused_launch_in_stages_1_and_2(dtype, fused, monkeypatch):
    """Sam2Plan with CVMI_SAM_PROJMLP = 0 / 1: the fused setting launches proj_mlp_kernel for blocks 0 - 2 and no b{i}.proj there; both settings
    meet test_sam2_wrapper_mini_matches_oracle's tolerance against the fp32 oracle."""
    from circuitvision_amd.sam2 import Sam2Plan
    monkeypatch.setenv("CVMI_SAM_PROJMLP", fused)
    wt, x, (hi, lo, iou, inter) = _mini144(dtype)
    sp = Sam2Plan(wt, 2, torch.cuda.Stream())
    sp.x_in.t.copy_(x.permute(0, 2, 3, 1).to(TORCH_DTYPE[dtype]))
    torch.cuda.synchronize()
    timed = sp.plan.timed_eager(with_kernels=True)
    torch.cuda.synchronize()
    labels = [t[0] for t in timed]
    kern = {t[0]: t[5] for t in timed}
    for i, tag in ((0, "<144, 1>"), (1, "<288, 2>"), (2, "<288, 2>")):
        if fused == "1":
            assert f"b{i}.proj" not in labels and kern[f"b{i}.mlp"] == "proj_mlp_kernel" + tag, (i, kern[f"b{i}.mlp"])
        else:
            assert f"b{i}.proj" in labels and kern[f"b{i}.mlp"] == "hiera_mlp_kernel" + tag, (i, kern[f"b{i}.mlp"])
    assert "b3.proj" in labels                                    # stage 3 keeps its launches
    tol = dict(rtol=3e-2, atol=3e-2) if dtype == F16 else dict(rtol=2e-1, atol=2e-1)
    for name, buf, ref in (("feat_s0", sp.feat_s0, inter["s0"]), ("feat_s1", sp.feat_s1, inter["s1"])):
        torch.testing.assert_close(buf.t.float().permute(0, 3, 1, 2).cpu(), ref, **tol, msg=lambda m: f"{name}: {m}")
    torch.testing.assert_close(sp.low_res.cpu(), lo, **tol)
    torch.testing.assert_close(sp.iou.cpu(), iou, **tol)
    torch.testing.assert_close(sp.high_res.cpu(), hi, **tol)
