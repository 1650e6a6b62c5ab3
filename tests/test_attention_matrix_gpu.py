"""The attention dispatch matrix (tests/op_matrix.py ATTN_ROWS): every kernel family and template instance cvmi_attention picks, pinned by the
name cvmi_last_kernel() reports, in fp16 and bf16, against a float64 softmax(q k^T scale) v of the same rounded operands.

Bound per element, u = the 16-bit type's unit roundoff (2^-11 fp16, 2^-8 bf16):
    |o - ref| <= 3 u sum_k p_k |v_k| + u |ref| + 1e-6
(P rounded to 16 bits before the PV product, fp32 accumulation, the 16-bit store).  fp32 rows: |o - ref| <= 1e-5 + 1e-4 |ref|.

Every row runs these score structures, built from designed q and k (tests/test_attention_matrix_gpu.py _design):
  random     q, k, v ~ N(0, 1)
  uniform    q = 0: every row is the mean of V
  dom_first  one key scores 24 log2 units above the rest, in the first key tile
  dom_last   the same in the last key tile
  far_max    row maxima around 100 log2 units
  climb7.9   the row maximum climbs by 7.9 log2 units per 64 keys (below DEFER_LOG2 = 8: the deferred rescale waits)
  climb8.1   ... by 8.1 (above it: every climb rescales)
  big_v      |V| up to 3e4 (fp16) / 1e30 (bf16)
and checks the kernel tag, finiteness, the bound, a bit-identical second launch, and (o_pad rows) that the columns around the output keep
their sentinel."""
import math

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, Plan, make_attn_desc, op_attention
from helpers import quant, run, stream
from op_matrix import ATTN_ROWS, SHARE_ROWS

pytestmark = pytest.mark.gpu
DT = {"f16": F16, "bf16": BF16, "f32": F32}
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
SENTINEL = -12288.0                                 # exact in every type
STRUCTS = ("random", "uniform", "dom_first", "dom_last", "far_max", "climb7.9", "climb8.1", "big_v")
STRUCTS_F32 = ("random", "uniform", "dom_first", "dom_last")
SIG_DIMS = 3                                        # q = 1 in these dims; a key's score lives in them (greedy 3-part encoding: ~24 bits)
# per-row relaxations of the bound (row id -> factor), each with its measured worst ratio: none needed
RELAX = {}


def _encode(t_log2, c, dtype):
    """[Nk] target scores in log2 units -> [Nk, SIG_DIMS] key entries whose rounded values sum to t / c (q = 1 in those dims)."""
    r = t_log2.double() / c
    parts = []
    for _ in range(SIG_DIMS):
        p = quant(r.float(), dtype).double()
        parts.append(p)
        r = r - p
    return torch.stack(parts, -1).float()


def _design(kind, B, H, Nq, Nk, dqk, dv, c, dtype, g):
    """Unrounded q [B,H,Nq,dqk], k [B,H,Nk,dqk], v [B,H,Nk,dv] of one score structure; c = log2 units per unit of q.k."""
    rn = lambda *s: torch.randn(*s, generator=g)
    v = rn(B, H, Nk, dv)
    if kind in ("random", "big_v"):
        if kind == "big_v":
            v = v.clamp(-4, 4) * (7.5e3 if dtype == F16 else 2.5e29)
        return rn(B, H, Nq, dqk), rn(B, H, Nk, dqk), v
    if kind == "uniform":
        return torch.zeros(B, H, Nq, dqk), rn(B, H, Nk, dqk), v
    sig = (1.0 / (c * math.sqrt(dqk - SIG_DIMS))) ** 0.5      # noise dims: score noise of std ~1 log2 unit
    q = rn(B, H, Nq, dqk) * sig
    q[..., :SIG_DIMS] = 1.0
    k = rn(B, H, Nk, dqk) * sig
    t = torch.zeros(Nk, dtype=torch.float64)
    if kind in ("dom_first", "dom_last"):
        j = min(3, Nk - 1) if kind == "dom_first" else Nk - 1
        t[j] = 24.0
        k[..., j, SIG_DIMS:] = 0.0
    elif kind == "far_max":
        t = 100.0 - 3.0 * torch.rand(Nk, generator=g, dtype=torch.float64)
    else:
        step, blk = float(kind[5:]), 64
        nb = -(-Nk // blk)
        top = min(nb, 6)
        for b in range(nb):
            lo, hi = b * blk, min(Nk, (b + 1) * blk)
            t[lo:hi] = step * min(b, top - 1) - 6.0
            if b < top:                                       # the block's peak key: exactly step above the previous one
                j = min(lo + 37, hi - 1)
                t[j] = step * b
                k[..., j, SIG_DIMS:] = 0.0
    k[..., :SIG_DIMS] = _encode(t, c, dtype)
    return q, k, v


def _climbs(k, c, Nk):
    """The climbs of the peak keys' scores in log2 units, from the ROUNDED keys (k [.., Nk, d] with q = 1 in the signal dims)."""
    peaks = [min(b * 64 + 37, min(Nk, (b + 1) * 64) - 1) for b in range(min(-(-Nk // 64), 6))]
    s = k[0, 0, peaks, :SIG_DIMS].double().sum(-1) * c
    return (s[1:] - s[:-1]).tolist()


def _tok(t):
    """[B, H, N, d] -> [B, N, H * d]."""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def _desc(**kw):
    base = dict(q_bdiv=0, kv_bdiv=0, av_fp8=0, q_log2=0, win=0, grid_h=0, grid_w=0, q_pool=0)
    base.update(kw)
    return make_attn_desc(**base)


def _setup_global(row, dtype, q, k, v, scale):
    B, H, Nq, Nk, dqk, dv, o_pad = (row[x] for x in ("B", "heads", "Nq", "Nk", "dqk", "dv", "o_pad"))
    td = TORCH_DTYPE[dtype]
    Cq, Cv = H * dqk, H * dv
    dev = lambda t: t.to(td).cuda().contiguous()
    if row["layout"] == "sep":
        keep = (dev(_tok(q)), dev(_tok(k)), dev(_tok(v)))
        (qp, kp, vp), (q_st, k_st, v_st) = (t.data_ptr() for t in keep), (Cq, Cq, Cv)
    elif row["layout"] == "qkv":
        assert Nq == Nk
        buf = dev(torch.cat((_tok(q), _tok(k), _tok(v)), -1))
        es, keep = buf.element_size(), (buf,)
        qp, kp, vp = buf.data_ptr(), buf.data_ptr() + Cq * es, buf.data_ptr() + 2 * Cq * es
        q_st = k_st = v_st = 2 * Cq + Cv
    else:                                                    # kv256: K and V halves of one token buffer
        qd, kv = dev(_tok(q)), dev(torch.cat((_tok(k), _tok(v)), -1))
        es, keep = kv.element_size(), (qd, kv)
        qp, kp, vp = qd.data_ptr(), kv.data_ptr(), kv.data_ptr() + Cq * es
        q_st, k_st, v_st = Cq, Cq + Cv, Cq + Cv
    o_ld = Cv + 2 * o_pad
    od = torch.full((B, Nq, o_ld), SENTINEL, dtype=td, device="cuda")
    desc = _desc(q=qp, k=kp, v=vp, o=od.data_ptr() + o_pad * od.element_size(),
                 q_sb=Nq * q_st, q_sh=dqk, q_st=q_st, k_sb=Nk * k_st, k_sh=dqk, k_st=k_st, v_sb=Nk * v_st, v_sh=dv, v_st=v_st,
                 o_sb=Nq * o_ld, o_sh=dv, o_st=o_ld, B=B, heads=H, Nq=Nq, Nk=Nk, dqk=dqk, dv=dv, scale=scale, dtype=dtype, q_log2=row["q_log2"], av_fp8=row["av_fp8"])
    get = lambda: od[..., o_pad:o_pad + Cv].float().cpu().view(B, Nq, H, dv).permute(0, 2, 1, 3)
    return desc, keep, od, get


def _pool_q(qf, win):
    """2 x 2 max-pool of a window's query tokens: [nwin, H, win^2, d] -> [nwin, H, (win/2)^2, d]."""
    n, H, _, d = qf.shape
    return qf.view(n, H, win // 2, 2, win // 2, 2, d).amax((3, 5)).reshape(n, H, (win // 2) ** 2, d)


def _setup_window(row, dtype, qf, k, v, scale):
    imgs, gh, gw, win, H, o_pad, qp_ = (row[x] for x in ("imgs", "gh", "gw", "win", "heads", "o_pad", "q_pool"))
    td, hd = TORCH_DTYPE[dtype], 72
    C_ = H * hd

    def grid(t):                                             # [nwin, H, win^2, hd] -> [imgs, gh, gw, C]
        t = t.transpose(1, 2).reshape(imgs, gh // win, gw // win, win, win, C_)
        return t.permute(0, 1, 3, 2, 4, 5).reshape(imgs, gh, gw, C_)
    qkv = torch.cat((grid(qf), grid(k), grid(v)), -1).to(td).cuda().contiguous()
    es = qkv.element_size()
    ow = win // 2 if qp_ else win
    ogh, ogw = (gh // 2, gw // 2) if qp_ else (gh, gw)
    o_ld = C_ + 2 * o_pad
    od = torch.full((imgs, ogh, ogw, o_ld), SENTINEL, dtype=td, device="cuda")
    desc = _desc(q=qkv.data_ptr(), k=qkv.data_ptr() + C_ * es, v=qkv.data_ptr() + 2 * C_ * es, o=od.data_ptr() + o_pad * es,
                 q_sb=0, q_sh=hd, q_st=3 * C_, k_sb=0, k_sh=hd, k_st=3 * C_, v_sb=0, v_sh=hd, v_st=3 * C_, o_sb=0, o_sh=hd, o_st=o_ld,
                 B=row["B"], heads=H, Nq=row["Nq"], Nk=row["Nk"], dqk=hd, dv=hd, scale=scale, dtype=dtype, win=win, grid_h=gh, grid_w=gw,
                 q_pool=qp_, q_log2=row["q_log2"], av_fp8=row["av_fp8"])

    def get():
        o = od[..., o_pad:o_pad + C_].float().cpu().view(imgs, ogh // ow, ow, ogw // ow, ow, H, hd)
        return o.permute(0, 1, 3, 2, 4, 5, 6).reshape(-1, ow * ow, H, hd).transpose(1, 2)
    return desc, (qkv,), od, get


def _reference(q, k, v, scale_ref):
    """float64 softmax(q k^T scale) v and softmax(q k^T scale) |v|."""
    p = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale_ref, -1)
    return p @ v.double(), p @ v.double().abs()


def _bound(dtype, ref, absref):
    if dtype == F32:
        return 1e-5 + 1e-4 * ref.abs()
    u = UNIT[dtype]
    return 3 * u * absref + u * ref.abs() + 1e-6


def _launch(desc, keep, od, get, lib):
    plan = Plan(stream())
    op_attention(plan, "attn", desc, keep)
    lib.cvmi_last_kernel()                                   # clears the tag
    run(plan)
    tag = lib.cvmi_last_kernel().decode()
    first = od.clone()
    run(plan)
    return tag, get(), torch.equal(od, first)


@pytest.mark.parametrize("row,dt", [(r, dt) for r in ATTN_ROWS for dt in r["dtypes"]], ids=[f"{r['id']}-{dt}" for r in ATTN_ROWS for dt in r["dtypes"]])
def test_attention_matrix(row, dt):
    dtype, lib = DT[dt], _lib.load()
    B, H, Nq, Nk, dqk, dv = (row[x] for x in ("B", "heads", "Nq", "Nk", "dqk", "dv"))
    scale = dqk ** -0.5
    scale_ref = LN2 if row["q_log2"] else scale              # q_log2: q carries scale * log2(e); the descriptor's scale is ignored
    c = scale_ref * LOG2E
    win = row["win"]
    failures, worst = [], (0.0, "")
    for si, kind in enumerate(STRUCTS if dtype != F32 else STRUCTS_F32):
        if kind.startswith("climb") and Nk < 128:
            continue
        g = torch.Generator().manual_seed(1000 * si + Nq + 7 * Nk + dqk)
        q, k, v = _design(kind, B, H, win * win if win else Nq, Nk, dqk, dv, c, dtype, g)
        q, k, v = quant(q, dtype), quant(k, dtype), quant(v, dtype)
        if kind.startswith("climb"):
            cl, step = _climbs(k, c, Nk), float(kind[5:])
            assert all((x < 8.0) == (step < 8.0) and abs(x - step) < 0.02 for x in cl), (kind, cl)
        if win:
            desc, keep, od, get = _setup_window(row, dtype, q, k, v, 123.0 if row["q_log2"] else scale)
            q = _pool_q(q, win) if row["q_pool"] else q
        else:
            desc, keep, od, get = _setup_global(row, dtype, q, k, v, 123.0 if row["q_log2"] else scale)
        tag, got, same = _launch(desc, keep, od, get, lib)
        ref, absref = _reference(q, k, v, scale_ref)
        err = (got.double() - ref).abs()
        ratio = float((err / _bound(dtype, ref, absref)).max()) / RELAX.get(row["id"], 1.0)
        if ratio > worst[0]:
            worst = (ratio, kind)
        print(f"{row['id']} {dt} {kind}: {tag}  max|err| {float(err.max()):.3e}  err/bound {ratio:.3f}")
        if tag != row["expect"]:
            failures.append(f"{kind}: kernel {tag!r}, expected {row['expect']!r}")
        if not bool(torch.isfinite(got).all()):
            failures.append(f"{kind}: non-finite output")
        if not ratio <= 1.0:
            i = int(torch.argmax(err / _bound(dtype, ref, absref)))
            failures.append(f"{kind}: err/bound {ratio:.3f} (max |err| {float(err.max()):.3e}; worst element {i}: got {float(got.flatten()[i]):.6e} "
                            f"ref {float(ref.flatten()[i]):.6e})")
        if not same:
            failures.append(f"{kind}: a second launch of the same plan differs")
        if row["o_pad"]:
            p = row["o_pad"]
            if not (bool((od[..., :p] == SENTINEL).all()) and bool((od[..., od.shape[-1] - p:] == SENTINEL).all())):
                failures.append(f"{kind}: columns outside the output were written")
    print(f"ATTN-MATRIX {row['id']} {dt}: {row['expect']}  worst err/bound {worst[0]:.3f} ({worst[1]})")
    assert not failures, f"{row['id']} {dt}:\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("share", SHARE_ROWS, ids=[f"{s[0]}_img{s[1]}_np{s[2]}" for s in SHARE_ROWS])
def test_attention_batch_sharing(share, dt):
    """q_bdiv / kv_bdiv (box prompts, decoder layer 0): batch b reads the shared operand of b / NP.  Bit-identical to the same launch with the
    shared tensor physically repeated, and within the bound of the float64 reference."""
    mode, imgs, NP, H, Nq, Nk, d, expect = share
    dtype, lib, td = DT[dt], _lib.load(), TORCH_DTYPE[DT[dt]]
    B = imgs * NP
    g = torch.Generator().manual_seed(31 * NP + imgs + Nq)
    nq_b, nk_b = (B, imgs) if mode == "t2i" else (imgs, B)
    q = quant(torch.randn(nq_b, H, Nq, d, generator=g), dtype)
    k = quant(torch.randn(nk_b, H, Nk, d, generator=g), dtype)
    v = quant(torch.randn(nk_b, H, Nk, d, generator=g), dtype)
    scale, C_ = d ** -0.5, H * d
    outs = {}
    for shared in (True, False):
        qq, kk, vv = q, k, v
        if not shared:
            if mode == "t2i":
                kk, vv = k.repeat_interleave(NP, 0), v.repeat_interleave(NP, 0)
            else:
                qq = q.repeat_interleave(NP, 0)
        qd = _tok(qq).to(td).cuda().contiguous()
        kv = torch.cat((_tok(kk), _tok(vv)), -1).to(td).cuda().contiguous()
        od = torch.full((B, Nq, C_), SENTINEL, dtype=td, device="cuda")
        es = kv.element_size()
        desc = _desc(q=qd.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr() + C_ * es, o=od.data_ptr(),
                     q_sb=Nq * C_, q_sh=d, q_st=C_, k_sb=Nk * 2 * C_, k_sh=d, k_st=2 * C_, v_sb=Nk * 2 * C_, v_sh=d, v_st=2 * C_,
                     o_sb=Nq * C_, o_sh=d, o_st=C_, B=B, heads=H, Nq=Nq, Nk=Nk, dqk=d, dv=d, scale=scale, dtype=dtype,
                     q_bdiv=NP if (shared and mode == "i2t") else 0, kv_bdiv=NP if (shared and mode == "t2i") else 0)
        get = lambda od=od: od.float().cpu().view(B, Nq, H, d).permute(0, 2, 1, 3)
        tag, outs[shared], same = _launch(desc, (qd, kv), od, get, lib)
        assert tag == expect, (shared, tag)
        assert same, "a second launch of the same plan differs"
    assert torch.equal(outs[True], outs[False]), "batch-shared launch differs from the physically repeated one"
    if mode == "t2i":
        k, v = k.repeat_interleave(NP, 0), v.repeat_interleave(NP, 0)
    else:
        q = q.repeat_interleave(NP, 0)
    ref, absref = _reference(q, k, v, scale)
    ratio = float(((outs[True].double() - ref).abs() / _bound(dtype, ref, absref)).max())
    print(f"ATTN-SHARE {mode} images {imgs} NP {NP} {dt}: {tag}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
