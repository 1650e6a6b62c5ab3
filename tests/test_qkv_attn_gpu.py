"""The fused qkv + 8 x 8-window attention launch (cvmi_attention with cvmi_attn_desc.proj_x; csrc/qkv_attn.hpp) on the rows of
tests/qkv_attn_cases.py, in fp16 and bf16, q_log2 on and off.

The oracle is the pair of launches it replaces: op_tok_linear (LayerNorm + qkv into a [tokens, 432] buffer) followed by op_attention on that
buffer -- every piece is reused in the same order, so `ao` must be BIT-EQUAL (torch.equal).  Independently, float64 window attention on the
16-bit qkv the unfused projection wrote, judged by the bound tests/test_attention_matrix_gpu.py applies to its attn_res64 rows (imported).
Every row runs with an input ld of K + 4 whose padding columns are NaN, a NaN row block in front of the offset view, guard columns around `ao`
that must keep their sentinel, LayerNorm statistics absent and forwarded as the rows' own (mean, rstd), and a second launch on restored
buffers that must be bit-identical.  The `kinds` rows carry the five LayerNorm row kinds of tests/tok_ref.py; the seam test takes rows and
statistics from a proj_mlp launch, as production does, instead of float64-made pairs."""
import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, PackedQkvAttn, PackedTokLinear, Plan, Rows, make_attn_desc, op_attention, op_tok_linear
from helpers import run, stream
from op_matrix import proj_pick
from qkv_attn_cases import QKV_ATTN_ROWS
from test_attention_matrix_gpu import LN2, LOG2E, SENTINEL, _bound, _pool_q, _reference
from tok_ref import judge, proj_mlp_ref, proj_operands, row_kinds

pytestmark = pytest.mark.gpu
DT = {"f16": F16, "bf16": BF16}
HD, WIN, PADR, OPAD, EPS = 72, 8, 8, 8, 1e-6


def _windows(t, B, H, W, heads, win=WIN):
    """[B * H * W, heads * HD] -> [nwin, heads, win^2, HD]."""
    t = t.view(B, H // win, win, W // win, win, heads, HD).permute(0, 1, 3, 5, 2, 4, 6)
    return t.reshape(-1, heads, win * win, HD)


def token_rows(row, dt, g, seam):
    """The f32 token rows a fused qkv launch normalises: (Rows view, forwarded (mean, rstd) on the device, what must stay alive).  The view has a
    row stride of K + 4 with NaN padding columns and a NaN row block in front.  Plain: seeded rows, on a `kinds` row shaped by tok_ref.row_kinds,
    and their own statistics from the CPU.  seam: the rows and the statistics a proj_mlp launch on `kinds` operands wrote (x and stats_out of
    tests/test_tok_matrix_gpu.py launch_proj, itself held to the matrix's bound here), handed over as production does."""
    (B, H, W), K = row["grid"], row["K"]
    rows, ld = B * H * W, K + 4
    if seam:
        from test_tok_matrix_gpu import launch_proj
        prow = dict(id="seam_c%d_rows%d" % (K, rows), expect=proj_pick(K), C=K, rows=rows, x_ld=ld, ao_ld=K + 8, stats_out=True, kinds=True, proj=True, pipe=None)
        o = proj_operands(prow, dt)
        tag, out, stats, layout, same, (xb, written) = launch_proj(prow, dt, o)
        ratio, _, fails = judge(prow, dt, o, proj_mlp_ref(prow, o, dt), out, stats)
        print(f"SEAM {prow['id']} {dt}: {tag}  err/bound {ratio:.3f}")
        assert tag == prow["expect"] and same and not layout and not fails, (tag, same, layout, fails)
        return Rows(xb.t, rows, K, ld=ld, offset=(rows + 3) * ld, dtype=F32), written, (xb, written)
    xh = torch.randn(rows, K, generator=g) * (1 + torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    if row.get("kinds"):
        row_kinds(xh)
    xbuf = torch.full((PADR + rows, ld), float("nan"))       # NaN row block in front, NaN padding columns
    xbuf[PADR:, :K] = xh
    xbuf = xbuf.cuda()
    mean = xh.mean(1)
    own = torch.stack((mean, 1.0 / torch.sqrt(((xh - mean[:, None]) ** 2).mean(1) + EPS)), 1).contiguous().cuda()
    return Rows(xbuf, rows, K, ld=ld, offset=PADR * ld, dtype=F32), own, xbuf


@pytest.mark.parametrize("q_log2", [0, 1], ids=["scale", "qlog2"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("row", QKV_ATTN_ROWS, ids=[r["id"] for r in QKV_ATTN_ROWS])
def test_qkv_attn_is_the_two_launches_bit_for_bit(row, dt, q_log2):
    _case(row, dt, q_log2)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_proj_mlp_hands_rows_and_statistics_to_qkv_attn64(dt):
    """The seam of stage 1: proj_mlp_kernel<144, 1> writes x and stats_out, qkv_attn64_kernel takes them as proj_x / proj_stats.  Bit-equal to
    the two launches fed the same written statistics, and inside the bound of float64 window attention on what the launches produce with the
    statistics absent."""
    _case(next(r for r in QKV_ATTN_ROWS if r["id"] == "kinds_2x16x24"), dt, 0, seam=True)


def _case(row, dt, q_log2, seam=False):
    dtype, lib = DT[dt], _lib.load()
    td = TORCH_DTYPE[dtype]
    (B, H, W), K, heads = row["grid"], row["K"], row["heads"]
    qp = row["q_pool"]
    C_, rows, ld = heads * HD, B * H * W, K + 4
    nwin = rows // (WIN * WIN)
    orows, nq = (rows // 4, WIN * WIN // 4) if qp else (rows, WIN * WIN)       # q_pool: ao on the half-resolution grid
    g = torch.Generator().manual_seed(17 * rows + K + q_log2)
    w = torch.randn(3 * C_, K, generator=g) * 0.08
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
        op_attention(plan, "qkv_attn", desc, (xbuf, o_got, pq, gam, bet, stats))
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
        if not torch.equal(first, o_ref):
            d = (first.float() - o_ref.float()).abs()
            failures.append(f"{what}: ao differs from tok_linear + attention in {int((first != o_ref).sum())} of {first.numel()} elements, max |diff| {float(d.max()):.3e}")
        # float64 window attention on the 16-bit qkv of the unfused projection
        qh = qkv.float().cpu()
        q, k, v = (_windows(qh[:, i * C_:(i + 1) * C_].contiguous(), B, H, W, heads) for i in range(3))
        ref, absref = _reference(_pool_q(q, WIN) if qp else q, k, v, LN2 if q_log2 else HD ** -0.5)
        got = _windows(first[:, OPAD:OPAD + C_].float().cpu().contiguous(), B, H // 2, W // 2, heads, WIN // 2) if qp else \
            _windows(first[:, OPAD:OPAD + C_].float().cpu().contiguous(), B, H, W, heads)
        ratio = float(((got.double() - ref).abs() / _bound(dtype, ref, absref)).max())
        print(f"QKV-ATTN {row['id']} {dt} q_log2={q_log2} {what}: {tag}  err/bound vs fp64 {ratio:.3f}")
        if not bool(torch.isfinite(got).all()):
            failures.append(f"{what}: non-finite output")
        if not ratio <= 1.0:
            failures.append(f"{what}: err/bound {ratio:.3f} against float64 window attention")
        if stats is None:
            absent = (ref, _bound(dtype, ref, absref))
        elif seam:                                           # the written statistics against what the launches make of the rows themselves
            r0 = float(((got.double() - absent[0]).abs() / absent[1]).max())
            print(f"QKV-ATTN {row['id']} {dt} seam: err/bound vs fp64 on the statistics-absent qkv {r0:.3f}")
            if not r0 <= 1.0:
                failures.append(f"{what}: err/bound {r0:.3f} against float64 window attention on the statistics-absent qkv")
    assert not failures, f"{row['id']} {dt} q_log2={q_log2}:\n  " + "\n  ".join(failures)
