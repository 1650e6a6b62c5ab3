"""The token-path matrix (tests/op_matrix.py TOK_ROWS / MLP_ROWS): every built instance of tok_linear_kernel, tok_linear16_kernel and
hiera_mlp_kernel, pinned by the tag cvmi_last_kernel() reports, at the shapes where a token-stationary kernel goes wrong -- chunk counts below,
at and one past the weight ring's depth, ragged last chunks, the direct-store route, K = 576 row blocks shared between workgroups, pool grids
whose half width is no power of two, per-slice statistics whose slice means lie far apart, ragged MLP tiles -- in fp16 and bf16, against the fp64
reference of tests/tok_ref.py under |y - ref64| <= ATOL[family, dtype] + RTOL[stored type] |ref64| per element.  ATOL comes from the CPU
(tok_ref.py: 4 x the fp32 chain's own deviation from fp64), never from a kernel; tests/test_tok_ref_cpu.py proves on the CPU that this comparison
catches the classic mistakes.

Every launch goes through engine.py's wrappers over Buf / View operands (which carry their own sizes).  Each row also checks that the input's
padding columns (NaN) and the rows in front of an offset view (NaN) are not read, that guard columns behind the output and rows behind the
MLP's last one are bit-untouched, that forwarded statistics are those of the rows as written, and that a second launch on restored buffers is
bit-identical.

PROJ_ROWS hold proj_mlp_kernel (the proj form of op_hiera_mlp) to the same method at every count of MLP_ROW_COUNTS, without statistics out, at
tight strides and on `kinds` operands -- LayerNorm inputs 500 away from zero, ramped along C, with a spread of 1e-3, with an outlier in channel
0 and in the last channel; MLP_KIND_ROWS run hiera_mlp_kernel on the same kinds.  The `kinds` rows of proj_mlp also meet the two launches the
fused one replaced."""
import time

import pytest
import torch

from circuitvision_amd._lib import ACT_GELU, ACT_NONE, BF16, F16, F32
from circuitvision_amd.engine import Buf, PackedHieraMlp, PackedProjMlp, PackedTokLinear, Plan, op_hiera_mlp, op_tok_linear, op_tok_linear_pool, tok_linear_stats_parts
from helpers import run, stream
from op_matrix import MLP_KIND_ROWS, MLP_ROWS, PROJ_ROWS, TOK_KS, TOK_ROWS, TOK_SPLIT_TABLE, tl16_splits
from tok_ref import ATOL, LN_EPS, STATS_PAIR_TOL, family, judge, reference, row_case, stats_ref, tok_operands

pytestmark = pytest.mark.gpu
CODE = {"f16": F16, "bf16": BF16}
CASES = [(r, dt) for r in TOK_ROWS for dt in r["dtypes"]]
MLP_CASES = [(r, dt) for r in MLP_ROWS + MLP_KIND_ROWS for dt in r["dtypes"]]
PROJ_CASES = [(r, dt) for r in PROJ_ROWS for dt in r["dtypes"]]
NAN = float("nan")


def _first_tag(plan):
    torch.cuda.synchronize()                                               # buffer fills ran on the default stream
    return plan.timed_eager(with_kernels=True)[0][5]


def launch_tok(row, dt, o):
    """Build the row's buffers, launch once (reading the tag), launch again on restored buffers.  Returns (tag, the whole output buffer after the
    first launch as a CPU float tensor [rows | rows / 4, out_ld], its statistics or None, second launch bit-identical, the output Buf)."""
    K, N, rows, in_ld, out_ld = row["K"], row["N"], row["rows"], row["in_ld"], row["out_ld"]
    code = CODE[dt]
    f32in, f32out = row["ln"] != 0, row["res"] or row["pool"]
    if row["pool"]:
        B, H, W = row["grid"]
        sb = Buf(B, H, W, in_ld, F32)
        src = sb.view(0, K)
        db = Buf(B, H // 2, W // 2, out_ld, F32)
    else:
        off = row["row_off"]
        assert rows % 256 == 0 and off % 256 == 0
        sb = Buf((off + rows) // 256, 1, 256, in_ld, F32 if f32in else code)
        src = sb.images(off // 256, rows // 256).view(0, K)
        db = Buf(rows // 256, 1, 256, out_ld, F32 if f32out else code)
    sb.t.fill_(NAN)                                                         # padding columns and the rows in front of the view poison what reads them
    src.tensor().copy_(o["x"].view(src.tensor().shape))
    dst = db.view(0, N)
    dst0 = o["dst0"].view(db.t.shape).to(db.t.dtype).cuda()
    db.t.copy_(dst0)
    pt = PackedTokLinear(o["w"], o["b"], dtype=code)
    gam, bet = o["gam"].cuda(), o["bet"].cuda()
    stats_in = o["stats_in"].cuda() if o["stats_in"] is not None else None
    stats = None
    plan = Plan(stream())
    if row["pool"]:
        op_tok_linear_pool(plan, row["id"], pt, src, dst, (gam, bet, LN_EPS), stats_in=stats_in)
    else:
        if row["stats_out"]:
            P = tok_linear_stats_parts(rows, K, N)
            stats = torch.full((rows, P, 2) if P else (rows, 2), -7.0, device="cuda")
        ln = None if row["ln"] == 0 else "cast" if row["ln"] == 2 else (gam, bet, LN_EPS)
        op_tok_linear(plan, row["id"], pt, src, dst, ln=ln, act=ACT_GELU if row["gelu"] else ACT_NONE, residual=row["res"], stats_in=stats_in,
                      stats_out=stats, stats_eps=LN_EPS, stats_parts=row["stats_in"] if isinstance(row["stats_in"], int) else 0)
    tag = _first_tag(plan)
    first = db.t.clone()
    first_stats = stats.clone() if stats is not None else None
    db.t.copy_(dst0)
    if stats is not None:
        stats.fill_(-7.0)
    run(plan)
    same = torch.equal(db.t, first) and (stats is None or torch.equal(stats, first_stats))
    out = first.view(-1, out_ld).float().cpu()
    return tag, out, (first_stats.cpu() if stats is not None else None), same, db


def _pair_ratio(row, out, stats):
    """err / bound of a forwarded (mean, rstd) pair against the rows as written (what judge holds it to), for the printed line."""
    if stats is None:
        return ""
    exp = stats_ref(out[:row["rows"]], row["C"])
    return "  statistics err/bound %.3f" % float(((stats.double() - exp).abs() / (STATS_PAIR_TOL[1] + STATS_PAIR_TOL[0] * exp.abs())).max())


def _verdict(what, row, dt, tag, ratio, mx, fails, same, t0, more=""):
    print(f"TOK-MATRIX {row['id']} {dt}: {tag}  family {family(row)}  max|err| {mx:.3e}  err/bound {ratio:.3f}  (atol {ATOL[family(row), dt]:.3e}){more}  {time.time() - t0:.2f} s")
    fails = list(fails)
    if tag != row["expect"]:
        fails.insert(0, f"kernel {tag!r}, expected {row['expect']!r}")
    if not same:
        fails.append("a second launch on restored buffers differs")
    assert not fails, f"{what} {row['id']} {dt}:\n  " + "\n  ".join(fails)


@pytest.mark.parametrize("row,dt", CASES, ids=[f"{r['id']}-{dt}" for r, dt in CASES])
def test_tok_matrix(row, dt):
    t0 = time.time()
    _, o, ref = row_case(row["id"], dt)
    tag, out, stats, same, db = launch_tok(row, dt, o)
    ratio, mx, fails = judge(row, dt, o, ref, out, stats)
    if row["ns"] is not None and row["N"] % 32 == 0:                       # the mirror against the library's own split count
        P = tok_linear_stats_parts(row["rows"], row["K"], row["N"])
        want = tl16_splits(row["rows"], row["N"], True)
        if P != (want if want > 1 else 0):
            fails.append(f"cvmi_tok_linear_stats_parts says {P}, the mirror {want}")
    if row["chain"]:
        fails += _consume_parts(row, dt, out, stats)
    _verdict("tok_linear", row, dt, tag, ratio, mx, fails, same, t0)


def _consume_parts(row, dt, written, parts):
    """The rows a split statistics-out launch wrote, normalised by a second launch from the P per-slice pairs it wrote beside them -- against
    the same launch with the two-pass prologue (today's bound) and against fp64 on the rows as written."""
    K, rows, P = row["N"], row["rows"], row["ns"]
    assert row["K"] == row["N"] == row["out_ld"] and parts is not None and tuple(parts.shape) == (rows, P, 2)
    fails = []
    for how in ("parts", "two_pass"):
        row2 = dict(next(r for r in TOK_ROWS if r["id"] == "k576_ln1_n72_ld80_parts6"), id=row["id"] + "_consumer", rows=rows, ns=tl16_splits(rows, 72, False),
                    stats_in=P if how == "parts" else None)
        o2 = tok_operands(row2, dt)
        o2.update(x=written[:, :K].clone(), stats_in=parts.clone() if how == "parts" else None)
        tag, out, _, same, _ = launch_tok(row2, dt, o2)
        ratio, mx, f = judge(row2, dt, o2, reference(row2, o2, dt), out)
        print(f"TOK-MATRIX {row2['id']} {dt} ({how}): {tag}  max|err| {mx:.3e}  err/bound {ratio:.3f}")
        fails += [f"consumer ({how}): {m}" for m in f] + ([] if tag == row2["expect"] and same else [f"consumer ({how}): tag {tag!r} / second launch differs"])
        if how == "parts":
            fwd = out
        else:
            tol = 2e-3 * (1.0 if dt == "f16" else 8.0)
            worst = float(((fwd[:, :72] - out[:, :72]).abs() / (tol + tol * out[:, :72].abs())).max())
            if not worst <= 1.0:
                fails.append(f"forwarded statistics against the two-pass prologue: err/bound {worst:.3f}")
    return fails


@pytest.mark.parametrize("row,dt", MLP_CASES, ids=[f"{r['id']}-{dt}" for r, dt in MLP_CASES])
def test_mlp_matrix(row, dt, monkeypatch):
    t0 = time.time()
    if row["pipe"] is None:
        monkeypatch.delenv("CVMI_MLP_PIPE", raising=False)
    else:
        monkeypatch.setenv("CVMI_MLP_PIPE", row["pipe"])                     # the library reads the test hook per call
    _, o, ref = row_case(row["id"], dt)
    C, rows, x_ld = row["C"], row["rows"], row["x_ld"]
    pm = PackedHieraMlp(o["w1"], o["b1"], o["w2"], o["b2"], dtype=CODE[dt])
    xb = Buf(rows + 3, 1, 1, x_ld, F32)
    x0 = o["x0"].view(xb.t.shape).cuda()
    xb.t.copy_(x0)
    stats = torch.full((rows, 2), -7.0, device="cuda") if row["stats_out"] else None
    plan = Plan(stream())
    op_hiera_mlp(plan, row["id"], pm, xb.images(0, rows).view(0, C), o["gam"].cuda(), o["bet"].cuda(), LN_EPS, stats_out=stats, stats_eps=LN_EPS)
    tag = _first_tag(plan)
    first, first_stats = xb.t.clone(), (stats.clone() if stats is not None else None)
    xb.t.copy_(x0)
    if stats is not None:
        stats.fill_(-7.0)
    run(plan)
    same = torch.equal(xb.t, first) and (stats is None or torch.equal(stats, first_stats))
    out, wrote = first.view(rows + 3, x_ld).cpu(), (first_stats.cpu() if stats is not None else None)
    ratio, mx, fails = judge(row, dt, o, ref, out, wrote)
    _verdict("hiera_mlp", row, dt, tag, ratio, mx, fails, same, t0, _pair_ratio(row, out, wrote))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def two_launches(row, dt, o):
    """op_tok_linear(residual) + op_hiera_mlp on a proj row's operands: the updated rows [rows, C] as a CPU float tensor.  op_tok_linear takes
    whole 256-row workgroups: the rows are padded with finite values."""
    C, rows, code = row["C"], row["rows"], CODE[dt]
    R = (rows + 255) // 256 * 256
    xc = Buf(1, 1, R, C, F32)
    xc.t.fill_(0.25)
    xc.t[0, 0, :rows] = o["x0"][:rows, :C].cuda()
    ac = Buf(1, 1, R, C, code)
    ac.t.fill_(0.5)
    ac.t[0, 0, :rows] = o["ao"].cuda()
    chain = Plan(stream())
    op_tok_linear(chain, "proj", PackedTokLinear(o["wp"], o["bp"], dtype=code), ac.view(), xc.view(), residual=True)
    op_hiera_mlp(chain, "mlp", PackedHieraMlp(o["w1"], o["b1"], o["w2"], o["b2"], dtype=code), xc.view(), o["gam"].cuda(), o["bet"].cuda(), LN_EPS)
    run(chain)
    return xc.t[0, 0, :rows].float().cpu()


def launch_proj(row, dt, o):
    """One PROJ_ROWS launch and its replay on restored buffers.  x lies behind a NaN row block and has three rows behind `rows`; its padding
    columns and ao's are NaN.  Returns (tag, the buffer [rows + 3, x_ld] after the first launch as a CPU tensor, its statistics or None, list of
    layout failures, second launch bit-identical, (x Buf, statistics tensor))."""
    C, rows, x_ld, ao_ld, code = row["C"], row["rows"], row["x_ld"], row["ao_ld"], CODE[dt]
    xb = Buf(2, 1, rows + 3, x_ld, F32)
    xb.t.fill_(NAN)
    xb.t[1, 0].copy_(o["x0"])
    x0 = xb.t.clone()
    aob = Buf(1, 1, rows, ao_ld, code)
    aob.t[0, 0].copy_(o["ao_buf"])
    ao0 = aob.t.clone()
    view = xb.images(1, 1).view(0, C)
    view.buf.W = rows                                                       # the op covers the first `rows` rows only
    pm = PackedProjMlp(o["wp"], o["bp"], o["w1"], o["b1"], o["w2"], o["b2"], dtype=code)
    stats = torch.full((rows, 2), -7.0, device="cuda") if row["stats_out"] else None
    plan = Plan(stream())
    op_hiera_mlp(plan, row["id"], None, view, o["gam"].cuda(), o["bet"].cuda(), LN_EPS, stats_out=stats, stats_eps=LN_EPS, proj=(pm, aob.view(0, C)))
    tag = _first_tag(plan)
    first, first_stats = xb.t.clone(), (stats.clone() if stats is not None else None)
    fails = []
    if not torch.equal(_bits(first[0]), _bits(x0[0])):
        fails.append("the NaN row block in front of x was written")
    if not torch.equal(_bits(aob.t), _bits(ao0)):
        fails.append("ao was written")
    xb.t.copy_(x0)
    if stats is not None:
        stats.fill_(-7.0)
    run(plan)
    same = torch.equal(_bits(xb.t), _bits(first)) and (stats is None or torch.equal(stats, first_stats))
    return tag, first[1, 0].cpu(), (first_stats.cpu() if stats is not None else None), fails, same, (xb, stats)


@pytest.mark.parametrize("row,dt", PROJ_CASES, ids=[f"{r['id']}-{dt}" for r, dt in PROJ_CASES])
def test_proj_mlp_matrix(row, dt):
    """proj_mlp_kernel against tok_ref.proj_mlp_ref under the projmlp bound.  A NaN that the launch read from x's or ao's padding, or from the
    row block in front, would reach the updated rows and fail the bound; on the `kinds` rows the launch also meets op_tok_linear(residual) +
    op_hiera_mlp on the same inputs within the sum of the two families' bounds."""
    t0 = time.time()
    _, o, ref = row_case(row["id"], dt)
    tag, out, stats, layout, same, _ = launch_proj(row, dt, o)
    ratio, mx, fails = judge(row, dt, o, ref, out, stats)
    if not bool(torch.isfinite(out[:row["rows"], :row["C"]]).all()):
        fails.append("non-finite updated values: padding was read")
    if row["kinds"]:
        two = two_launches(row, dt, o)
        bound = ATOL["projmlp", dt] + ATOL["mlp_kinds", dt]
        worst = float((out[:row["rows"], :row["C"]].double() - two.double()).abs().max()) / bound
        print(f"TOK-MATRIX {row['id']} {dt}: |fused - two launches| / (projmlp + mlp_kinds bound) {worst:.3f}")
        if not worst <= 1.0:
            fails.append(f"|fused - two launches| is {worst:.3f} of the two families' bounds")
    _verdict("proj_mlp", row, dt, tag, ratio, mx, layout + fails, same, t0, _pair_ratio(row, out, stats))


def test_tl16_splits_mirrors_the_library():
    """op_matrix.tl16_splits against cvmi_tok_linear_stats_parts for every (rows, N % 32 == 0) of the table; the other formats never split."""
    pairs = {(rows, N) for rows, N, _ in TOK_SPLIT_TABLE} | {(r["rows"], r["N"]) for r in TOK_ROWS if r["K"] == 576}
    pairs |= {(65536, 576), (32768, 576), (512, 576), (4096, 2304), (8192, 1728)}
    n = 0
    for rows, N in sorted(pairs):
        if N % 32:
            continue
        ns = tl16_splits(rows, N, True)
        assert tok_linear_stats_parts(rows, 576, N) == (ns if ns > 1 else 0), (rows, N, ns)
        n += 1
    assert n >= 12
    assert all(tok_linear_stats_parts(2048, K, K) == 0 for K in TOK_KS if K != 576)
    for rows, N, ns in TOK_SPLIT_TABLE:
        assert tl16_splits(rows, N, False) == ns, (rows, N)
