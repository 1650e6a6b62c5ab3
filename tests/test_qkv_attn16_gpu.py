"""The fused qkv + 4 x 4-window attention launch (cvmi_attention with cvmi_attn_desc.proj_x, win = 4, proj_K = 288; csrc/qkv_attn16.hpp) on the
rows of tests/qkv_attn16_cases.py, in fp16 and bf16, q_log2 on and off.

The launch projects q, k, v exactly as op_tok_linear does, but its window attention runs on the matrix pipe with a 16-bit P where the unfused
attn_win16_kernel runs f32 dot products per thread: `ao` is NOT bit-equal to the pair of launches.  The reference is float64 window attention
on the 16-bit qkv the UNFUSED projection wrote, judged by the bound tests/test_attention_matrix_gpu.py applies to its 16-bit MFMA window kernels
(imported): error / bound <= 1.  The two-launch result is within one bound of the same reference, so |fused - two-launch| <= 2 x bound is
checked elementwise too; the two-launch path's own error / bound is printed beside the fused one.
Every row runs with an input ld of K + 4 whose padding columns are NaN, a NaN row block in front of the offset view, guard columns around `ao`
that must keep their sentinel, LayerNorm statistics absent and forwarded as the rows' own (mean, rstd), and a second launch on restored
buffers that must be bit-identical.  The `kinds` rows carry the five LayerNorm row kinds of tests/tok_ref.py; the seam test takes rows and
statistics from a proj_mlp launch, as production does, instead of float64-made pairs.  The last test runs the plan that takes the launch for Hiera's stage 2, with the switch on and off."""
import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, PackedQkvAttn, PackedTokLinear, Plan, Rows, make_attn_desc, op_attention, op_tok_linear
from helpers import run, stream
from qkv_attn16_cases import QKV_ATTN16_ROWS
from test_attention_matrix_gpu import LN2, LOG2E, SENTINEL, _bound, _pool_q, _reference
from test_qkv_attn_gpu import _windows, token_rows

pytestmark = pytest.mark.gpu
DT = {"f16": F16, "bf16": BF16}
HD, WIN, PADR, OPAD, EPS = 72, 4, 8, 8, 1e-6


@pytest.mark.parametrize("q_log2", [0, 1], ids=["scale", "qlog2"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("row", QKV_ATTN16_ROWS, ids=[r["id"] for r in QKV_ATTN16_ROWS])
def test_qkv_attn16_against_fp64_and_the_two_launches(row, dt, q_log2):
    _case(row, dt, q_log2)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_proj_mlp_hands_rows_and_statistics_to_qkv_attn16(dt):
    """The seam of stage 2: proj_mlp_kernel<288, 2> writes x and stats_out, qkv_attn16_kernel takes them as proj_x / proj_stats.  Inside the
    imported bound against float64 window attention on the qkv of the unfused projection fed the same written statistics, within 2 x bound of
    the two launches, and inside the bound of what the launches produce with the statistics absent."""
    _case(next(r for r in QKV_ATTN16_ROWS if r["id"] == "kinds_2x16x24"), dt, 0, seam=True)


def _case(row, dt, q_log2, seam=False):
    dtype, lib = DT[dt], _lib.load()
    td = TORCH_DTYPE[dtype]
    (B, H, W), K, heads = row["grid"], row["K"], row["heads"]
    qp = row["q_pool"]
    C_, rows, ld = heads * HD, B * H * W, K + 4
    nwin = rows // (WIN * WIN)
    orows, nq = (rows // 4, WIN * WIN // 4) if qp else (rows, WIN * WIN)       # q_pool: ao on the half-resolution grid
    g = torch.Generator().manual_seed(19 * rows + K + q_log2)
    w = torch.randn(3 * C_, K, generator=g) * 0.06
    bias = torch.randn(3 * C_, generator=g) * 0.1
    if q_log2:                                               # the q rows carry scale * log2(e), as Sam2Weights folds it
        w[:C_] *= HD ** -0.5 * LOG2E
        bias[:C_] *= HD ** -0.5 * LOG2E
    gam, bet = (1 + 0.2 * torch.randn(K, generator=g)).cuda(), (0.1 * torch.randn(K, generator=g)).cuda()
    x_rows, own, xbuf = token_rows(row, dt, g, seam)
    pt, pq = PackedTokLinear(w, bias, "cuda", dtype), PackedQkvAttn(w, bias, heads, "cuda", dtype)
    scale = 123.0 if q_log2 else HD ** -0.5                  # (q_log2: the descriptor's scale is ignored)
    common = dict(q_sb=0, q_sh=HD, q_st=3 * C_, k_sb=0, k_sh=HD, k_st=3 * C_, v_sb=0, v_sh=HD, v_st=3 * C_, o_sb=0, o_sh=HD, o_st=C_ + 2 * OPAD,
                  B=nwin, heads=heads, Nq=nq, Nk=WIN * WIN, dqk=HD, dv=HD, scale=scale, dtype=dtype, win=WIN, grid_h=H, grid_w=W, q_pool=qp,
                  q_bdiv=0, kv_bdiv=0, av_fp8=0, q_log2=q_log2)
    failures, absent = [], None
    for stats in (None, own):
        what = "stats forwarded" if stats is not None else "stats absent"
        qkv = torch.full((rows, 3 * C_), SENTINEL, dtype=td, device="cuda")
        o_ref = torch.full((orows, C_ + 2 * OPAD), SENTINEL, dtype=td, device="cuda")
        o_got = o_ref.clone()
        es = qkv.element_size()
        ref_plan = Plan(stream())
        op_tok_linear(ref_plan, "qkv", pt, x_rows, Rows(qkv, rows, 3 * C_), ln=(gam, bet, EPS), stats_in=stats)
        op_attention(ref_plan, "attn", make_attn_desc(q=qkv.data_ptr(), k=qkv.data_ptr() + C_ * es, v=qkv.data_ptr() + 2 * C_ * es,
                                                      o=o_ref.data_ptr() + OPAD * es, **common), (qkv, o_ref))
        run(ref_plan)
        plan = Plan(stream())
        desc = make_attn_desc(q=None, k=None, v=None, o=o_got.data_ptr() + OPAD * es, proj_x=x_rows.ptr, proj_ld=ld, proj_K=K, proj_w=pq.w.data_ptr(),
                              proj_gamma=gam.data_ptr(), proj_beta=bet.data_ptr(), proj_eps=EPS, proj_stats=stats.data_ptr() if stats is not None else None,
                              **common)
        op_attention(plan, "qkv_attn16", desc, (xbuf, o_got, pq, gam, bet, stats))
        lib.cvmi_last_kernel()                               # clears the tag
        run(plan)
        tag = lib.cvmi_last_kernel().decode()
        first = o_got.clone()
        o_got.fill_(SENTINEL)                                # restored buffers, second launch
        run(plan)
        if tag != row["expect"]:
            failures.append(f"{what}: kernel {tag!r}, expected {row['expect']!r}")
        if not torch.equal(o_got, first):
            failures.append(f"{what}: a second launch on restored buffers differs")
        if not (bool((first[:, :OPAD] == SENTINEL).all()) and bool((first[:, OPAD + C_:] == SENTINEL).all())):
            failures.append(f"{what}: guard columns around ao were written")
        # float64 window attention on the 16-bit qkv of the unfused projection
        qh = qkv.float().cpu()
        q, k, v = (_windows(qh[:, i * C_:(i + 1) * C_].contiguous(), B, H, W, heads, WIN) for i in range(3))
        ref, absref = _reference(_pool_q(q, WIN) if qp else q, k, v, LN2 if q_log2 else HD ** -0.5)
        ogrid = (B, H // 2, W // 2, heads, WIN // 2) if qp else (B, H, W, heads, WIN)
        got = _windows(first[:, OPAD:OPAD + C_].float().cpu().contiguous(), *ogrid)
        two = _windows(o_ref[:, OPAD:OPAD + C_].float().cpu().contiguous(), *ogrid)
        bound = _bound(dtype, ref, absref)
        ratio = float(((got.double() - ref).abs() / bound).max())
        ratio_two = float(((two.double() - ref).abs() / bound).max())
        between = float(((got.double() - two.double()).abs() / bound).max())
        print(f"QKV-ATTN16 {row['id']} {dt} q_log2={q_log2} {what}: {tag}  err/bound vs fp64 {ratio:.3f} (two launches {ratio_two:.3f}), |fused - two| / bound {between:.3f}")
        if not bool(torch.isfinite(got).all()):
            failures.append(f"{what}: non-finite output")
        if not ratio <= 1.0:
            failures.append(f"{what}: err/bound {ratio:.3f} against float64 window attention (two launches: {ratio_two:.3f})")
        if not between <= 2.0:
            failures.append(f"{what}: |fused - two launches| / bound {between:.3f} > 2")
        if stats is None:
            absent = (ref, bound)
        elif seam:                                           # the written statistics against what the launches make of the rows themselves
            r0 = float(((got.double() - absent[0]).abs() / absent[1]).max())
            print(f"QKV-ATTN16 {row['id']} {dt} seam: err/bound vs fp64 on the statistics-absent qkv {r0:.3f}")
            if not r0 <= 1.0:
                failures.append(f"{what}: err/bound {r0:.3f} against float64 window attention on the statistics-absent qkv")
    assert not failures, f"{row['id']} {dt} q_log2={q_log2}:\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_sam2_plan_takes_the_fused_launch_in_stage_2(dt, fused, monkeypatch):
    """Sam2Plan with CVMI_SAM_QKVATTN16 = 0 / 1 on the mini Hiera of tests/test_proj_mlp_gpu.py (block 2: 288 wide, 4 heads, 4 x 4 windows; block 3:
    the q-pooled 288 -> 576 transition): the fused setting launches qkv_attn16_kernel for both and no b{i}.qkv there, the other setting the two
    launches; the 8 x 8 blocks keep qkv_attn64_kernel either way, and both settings meet that test's tolerance against the fp32 oracle."""
    from circuitvision_amd.sam2 import Sam2Plan, Sam2Weights, SamSyntheticParams
    from test_oracle_sam2_cpu import mini_targets
    from test_proj_mlp_gpu import MINI144, _mini144
    dtype = DT[dt]
    _, x, (hi, lo, iou, inter) = _mini144(dtype)             # (the oracle's side; its cached weights were packed under the default settings)
    monkeypatch.setenv("CVMI_SAM_QKVATTN16", fused)
    wt = Sam2Weights(SamSyntheticParams(seed=5, lora_targets=mini_targets(), std=0.05), MINI144, 256, dtype)
    sp = Sam2Plan(wt, 2, torch.cuda.Stream())
    sp.x_in.t.copy_(x.permute(0, 2, 3, 1).to(TORCH_DTYPE[dtype]))
    torch.cuda.synchronize()
    timed = sp.plan.timed_eager(with_kernels=True)
    torch.cuda.synchronize()
    labels = [t[0] for t in timed]
    kern = {t[0]: t[5] for t in timed}
    assert kern["b0.attn"] == "qkv_attn64_kernel<144, 2, false>" and kern["b1.attn"] == "qkv_attn64_kernel<144, 4, true>", kern
    for i, tag, two in ((2, "<288, 4, false>", "attn_win16_kernel<16, 9>"), (3, "<288, 8, true>", "attn_win16_kernel<4, 9>")):
        if fused == "1":
            assert f"b{i}.qkv" not in labels and kern[f"b{i}.attn"] == "qkv_attn16_kernel" + tag, (i, kern[f"b{i}.attn"])
        else:
            assert f"b{i}.qkv" in labels and kern[f"b{i}.attn"] == two, (i, kern[f"b{i}.attn"])
    assert "b4.qkv" in labels                                     # stage 3 keeps its launches
    tol = dict(rtol=3e-2, atol=3e-2) if dtype == F16 else dict(rtol=2e-1, atol=2e-1)
    for name, buf, ref in (("feat_s0", sp.feat_s0, inter["s0"]), ("feat_s1", sp.feat_s1, inter["s1"])):
        torch.testing.assert_close(buf.t.float().permute(0, 3, 1, 2).cpu(), ref, **tol, msg=lambda m: f"{name}: {m}")
    torch.testing.assert_close(sp.low_res.cpu(), lo, **tol)
    torch.testing.assert_close(sp.iou.cpu(), iou, **tol)
    torch.testing.assert_close(sp.high_res.cpu(), hi, **tol)
