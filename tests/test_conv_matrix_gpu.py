"""The convolution / GEMM dispatch matrix (tests/op_matrix.py CONV_ROWS): every kernel family and template instance cvmi_conv2d picks, pinned by the
name cvmi_last_kernel() reports, in fp16, bf16 and f32, each with its epilogue options, against a plain reference of the same rounded operands.

What every epilogue in igemm.hip and conv_tile.hip does (csrc/conv_epilogue.hpp states this contract once; gemm_epilogue, gemm256_kernel and
gemm256x192_kernel finish through its finish_chunk / store_out_chunk, conv_tile_kernel through its own store loop):
    t = TO(act(acc + bias))           acc in fp32; TO = the output type; with act_after_res the activation is skipped here
    y = TO(act2(float(t) + res))      only with a residual or act_after_res; act2 = the activation iff act_after_res
so a 16-bit output with a residual is rounded TWICE (the tile passes through LDS in the output type before the residual is added); without one, or
with an f32 output, once.  gemm256p_kernel takes no residual; gemm256x192r_kernel has an f32 output.

Three operand structures per row and dtype, each on a fresh Plan:
  integer  x in {-3..3}, w in {-2..2}, bias in {-4..4}, residual in {-8..8}, activation NONE or RELU.  Every product and partial sum is an
           integer below 2^24 (asserted: 6 K + 12 < 2^24), so fp32 accumulation is exact in any order, split or not, and the output must be
           BIT-IDENTICAL to the exact sum pushed through the two lines above.  In fp16 and f32 every intermediate is below 2048 in magnitude, t is
           exact and the result equals the exact sum rounded once (asserted); only bf16 with a residual sees the first rounding.
  random   x, bias, residual ~ N(0, 1), w ~ N(0, 1) / sqrt(K), rounded to their storage types; the row's own activation; float64 reference.
           Per element, u = 2^-11 (fp16), 2^-8 (bf16), 2^-24 (f32 output), A = conv(|x|, |w|) + |bias|, L = the activation's largest slope
           (1, 1.10 SiLU, 1.13 GELU), e_act = the fast activation's documented error (common.hpp: gelu_fast 2.5e-5; SiLU 4 * 2^-24 |y|; 0 in f32 mode):
               |y - ref| <= u |ref| + L (K + 2) 2^-24 A + e_act + 1e-7   (+ L2 u |t| where the epilogue rounds twice; L2 = L with act_after_res, else 1)
  ones     x = 1, w = 1, bias 0, residual 0, no activation (a row's RELU stays: the identity here, and gemm256x192r_kernel's dispatch depends on it):
           the output is Cin x (taps inside the image), exact; a failure names the pixel.
Each case also checks the kernel tag, finiteness, that a second run of the plan is bit-identical, and that a sentinel survives in every column of
the output buffer outside the view (y_pad rows, ragged Cout) and in one spare image allocated behind the last one.
A row with row_stats also checks, in every structure, the statistics the launch writes per row and 96-column slice -- (mean, sum of squared
deviations from it) of the values AS STORED -- against their float64 moments.  With u = 2^-24, A = the slice's largest |value| and m2 its sum of
squared deviations: the kernel forms 24 means of 4 and merges them pairwise in f32, fewer than 48 roundings on a path, so |mean - ref| <= 48 u A
=: e; a deviation then carries e + u A <= 2 e, its square 2 |dev| 2 e <= 8 A e, and 96 of them with < 48 roundings of the sum:
|m2 - ref| <= 96 * 8 A e + 48 u m2."""
import ctypes as C
import math
import time

import pytest
import torch
import torch.nn.functional as F

from circuitvision_amd import _lib
from circuitvision_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, BF16, F16, F32
from circuitvision_amd.engine import ESIZE, TORCH_DTYPE, Buf, PackedConv, Plan, op_conv
from helpers import run, stream
from op_matrix import CONV_ROWS, conv_expect

pytestmark = pytest.mark.gpu
DT = {"f16": F16, "bf16": BF16, "f32": F32}
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}
ACT = {"none": ACT_NONE, "relu": ACT_RELU, "silu": ACT_SILU, "gelu": ACT_GELU}
ACT_REF = {"none": lambda v: v, "relu": torch.relu, "silu": F.silu, "gelu": F.gelu}
SLOPE = {"none": 1.0, "relu": 1.0, "silu": 1.10, "gelu": 1.13}
SENTINEL = -12288.0                                 # exact in every type
STRUCTS = ("integer", "random", "ones")
# per-row relaxations of the random structure's bound (row id -> factor), each with its measured worst ratio: none needed
RELAX = {}


class _Table:
    """Constant [rows, C] device tensor posing as a residual view (ptr, ld): the broadcast tables of the SAM 2 plan."""

    def __init__(self, t):
        self.t, self.c = t, t.shape[-1]

    ptr = property(lambda s: s.t.data_ptr())
    ld = property(lambda s: s.c)


def _cu_count(lib):
    info = (C.c_int * 4)()
    assert lib.cvmi_device_info(0, info) == 0
    return int(info[0])


def _geometry(row, ncu):
    B = ncu // 2 if row["B"] == "cu/2" else row["B"]
    c0, c1 = row["Cin"] if isinstance(row["Cin"], tuple) else (row["Cin"], 0)
    k, s, pad, H, W = row["k"], row["stride"], row["pad"], row["H"], row["W"]
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    crop = row["out_hw"] or (OH, OW)
    return B, c0, c1, H, W, crop[0], crop[1], k * k * (c0 + c1)


def _shuffle(t, sc):
    """[B, OH, OW, 4 sc] -> [B, 2 OH, 2 OW, sc]: column (dy * 2 + dx) * sc + co goes to pixel (2 oy + dy, 2 ox + dx), channel co."""
    if not sc:
        return t
    B, OH, OW, _ = t.shape
    return t.view(B, OH, OW, 2, 2, sc).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, sc)


def _logical_input(row, srcs):
    """The NHWC sources (source `up` at half resolution) as one logical [B, H, W, c0 + c1] input."""
    full = [t.repeat_interleave(2, 1).repeat_interleave(2, 2) if i == row["up"] else t for i, t in enumerate(srcs)]
    return full[0] if len(full) == 1 else torch.cat(full, -1)


def _conv_ref(row, X, w, OH, OW, dtype):
    """sum_k A[m, k] w[n, k] as [B, OH, OW, N] in `dtype` (float32: exact for the integer operands; float64 otherwise), on BLAS."""
    B, H, W, ctot = X.shape
    k, s, pad, N = row["k"], row["stride"], row["pad"], w.shape[0]
    if k == 1 and s == 1 and pad == 0:
        return (X.reshape(-1, ctot).to(dtype) @ w.reshape(N, ctot).to(dtype).t()).view(B, H, W, N)[:, :OH, :OW]
    wm = w.reshape(N, -1).to(dtype).t()                                   # rows in (c, ky, kx) order, as F.unfold lists them
    OHf, OWf = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    out = []
    for b in range(B):                                                    # per image: bounds the size of the unfolded matrix
        cols = F.unfold(X[b:b + 1].permute(0, 3, 1, 2).to(dtype), k, padding=pad, stride=s)[0]
        out.append((cols.t() @ wm).view(OHf, OWf, N)[:OH, :OW])
    return torch.stack(out)


def _operands(kind, row, dtype, odt, geo, g):
    """CPU float32 tensors holding values already rounded to their storage types: sources (NHWC), w [N, ctot, k, k], bias [N], residual or None."""
    B, c0, c1, H, W, OH, OW, K = geo
    N, k, sc, rep = row["Cout"], row["k"], row["shuffle_cout"], max(row["res_rep"], 1)
    td, to = TORCH_DTYPE[dtype], TORCH_DTYPE[odt]
    shapes = [(B, H >> (row["up"] == i), W >> (row["up"] == i), c) for i, c in enumerate((c0, c1)) if c]
    rshape = {"none": None, "full": (B, OH, OW, N), "bcast": (OH * OW, N), "rep": (B // rep, OH, OW, N)}[row["res"]]
    if rshape is not None and sc:
        rshape = (rshape[0], 2 * OH, 2 * OW, sc)
    if kind == "integer":
        ri = lambda shape, a: torch.randint(-a, a + 1, shape, generator=g).float()
        srcs, w, b = [ri(s_, 3) for s_ in shapes], ri((N, c0 + c1, k, k), 2), ri((N,), 4)
        r = ri(rshape, 8) if rshape else None
    elif kind == "ones":
        srcs, w, b = [torch.ones(s_) for s_ in shapes], torch.ones(N, c0 + c1, k, k), torch.zeros(N)
        r = torch.zeros(rshape) if rshape else None
    else:
        rn = lambda shape: torch.randn(shape, generator=g)
        srcs, w, b = [rn(s_).to(td).float() for s_ in shapes], (rn((N, c0 + c1, k, k)) / math.sqrt(K)).to(td).float(), rn((N,))
        r = rn(rshape).to(to).float() if rshape else None
    return srcs, w, b, r


def _expand_res(row, r, B, OH, OW):
    """The residual as the [B, OHo, OWo, Nst] tensor the output sees."""
    if row["res"] == "bcast":
        return r.view(1, OH, OW, -1)
    if row["res"] == "rep":
        return r.repeat_interleave(row["res_rep"], 0)
    return r


def _launch(row, dtype, odt, geo, srcs, w, b, r, act, lib):
    B, c0, c1, H, W, OH, OW, K = geo
    N, sc, y_pad = row["Cout"], row["shuffle_cout"], row["y_pad"]
    td, to, ovec = TORCH_DTYPE[dtype], TORCH_DTYPE[odt], 16 // ESIZE[odt]
    OHo, OWo, Nst = (2 * OH, 2 * OW, sc) if sc else (OH, OW, N)
    width = -(-Nst // ovec) * ovec + 2 * y_pad
    bufs = []
    for t in srcs:
        xb = Buf(t.shape[0], t.shape[1], t.shape[2], t.shape[3], dtype)
        xb.t.copy_(t.to(td))
        bufs.append(xb)
    yb = Buf(B + 1, OHo, OWo, width, odt)                                  # one spare image behind the last: a tile that runs past M lands there
    yb.t.fill_(SENTINEL)
    dst = yb.images(0, B).view(y_pad, Nst)
    kw = {}
    if row["res"] == "bcast":
        kw = dict(res=_Table(r.to(to).cuda()), res_mod=OH * OW)
    elif row["res"] != "none":
        rb = Buf(r.shape[0], OHo, OWo, width, odt, zero=True)
        rb.t[..., y_pad:y_pad + Nst] = r.to(to).cuda()
        kw = dict(res=rb.view(y_pad, Nst))
        if row["res"] == "rep":
            kw.update(res_rep=row["res_rep"], res_mod=0 if sc else OH * OW)
    stats = torch.full((B * OH * OW, N // 96, 2), SENTINEL, device="cuda") if row["row_stats"] else None
    if stats is not None:
        kw["row_stats"] = stats
    plan = Plan(stream())
    op_conv(plan, row["id"], PackedConv(w, b, dtype), [(xb.view(), 1 if row["up"] == i else 0) for i, xb in enumerate(bufs)], dst,
            stride=row["stride"], pad=row["pad"], act=act, out_hw=row["out_hw"], scalar_gather=row["scalar_gather"],
            act_after_res=row["act_after_res"], shuffle_cout=sc, **kw)
    lib.cvmi_last_kernel()                                                 # clears the tag
    run(plan)
    tag = lib.cvmi_last_kernel().decode()
    first, stats1 = yb.t.clone(), (stats.clone() if stats is not None else None)
    run(plan)
    same = torch.equal(yb.t, first) and (stats is None or torch.equal(stats, stats1))
    got = first[:B, :, :, y_pad:y_pad + Nst].cpu()
    outside = torch.cat((first[:B, :, :, :y_pad].flatten(), first[:B, :, :, y_pad + Nst:].flatten(), first[B].flatten()))
    return tag, got, same, bool((outside == SENTINEL).all()), (stats1.cpu() if stats is not None else None)


def _stats_failure(got, stats):
    """The statistics of the rows as stored, or None when they hold (bound: the module's docstring)."""
    u = 2.0 ** -24
    sl = got.double().reshape(-1, got.shape[-1] // 96, 96)
    mu = sl.mean(2)
    m2 = ((sl - mu[..., None]) ** 2).sum(2)
    A = sl.abs().amax(2)
    e = 48 * u * A + 1e-30
    r_mean, r_m2 = ((stats[..., 0].double() - mu).abs() / e).max(), ((stats[..., 1].double() - m2).abs() / (96 * 8 * A * e + 48 * u * m2 + 1e-30)).max()
    print(f"  row_stats: mean err/bound {float(r_mean):.3f}  m2 err/bound {float(r_m2):.3f}")
    return None if float(r_mean) <= 1.0 and float(r_m2) <= 1.0 else f"row_stats: mean err/bound {float(r_mean):.3f}, m2 err/bound {float(r_m2):.3f}"


def _exact_model(row, s, b, r, act, to, geo):
    """The epilogue's two lines on the exact fp32 sums `s` [B, OH, OW, N]: (result as stored, the same with a single rounding at the end)."""
    B, _, _, _, _, OH, OW, _ = geo
    aar, sc = row["act_after_res"], row["shuffle_cout"]
    v = s + b
    a1 = (lambda t: t) if aar else ACT_REF[act]
    a2 = ACT_REF[act] if aar else (lambda t: t)
    t = _shuffle(a1(v).to(to).float(), sc)
    once = _shuffle(a1(v), sc)
    if r is not None or aar:
        rr = _expand_res(row, r, B, OH, OW) if r is not None else 0.0
        return a2(t + rr).to(to), a2(once + rr).to(to)
    return t.to(to), once.to(to)


def _where(idx, shape):
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(idx), shape))


@pytest.mark.parametrize("row,dt", [(r, dt) for r in CONV_ROWS for dt in r["dtypes"]], ids=[f"{r['id']}-{dt}" for r in CONV_ROWS for dt in r["dtypes"]])
def test_conv_matrix(row, dt):
    dtype, lib = DT[dt], _lib.load()
    ncu = _cu_count(lib)
    if row["B"] == "cu/2" and ncu % 8 != 0:
        pytest.skip(f"{row['id']}: gemm256x192r_kernel needs whole rounds of tiles on a CU count that is a multiple of 8; this device has {ncu}")
    t_start = time.time()
    odt = F32 if (dtype == F32 or row["out_f32"]) else dtype
    to, u = TORCH_DTYPE[odt], UNIT[odt]
    geo = _geometry(row, ncu)
    B, c0, c1, H, W, OH, OW, K = geo
    expect = conv_expect(row, dt)
    fast = dtype != F32
    twice = odt != F32 and (row["res"] != "none" or row["act_after_res"])
    failures, ratio_random = [], 0.0
    for si, kind in enumerate(STRUCTS):
        g = torch.Generator().manual_seed(1000 * si + 7 * K + row["Cout"] + B)
        act = row["act"]
        if kind == "integer":
            act = "none" if act == "none" else "relu"
        elif kind == "ones":
            act = "relu" if act == "relu" else "none"                       # RELU is the identity on the counts; it stays, since dispatch may depend on it
        srcs, w, b, r = _operands(kind, row, dtype, odt, geo, g)
        tag, got, same, clean, stats = _launch(row, dtype, odt, geo, srcs, w, b, r, ACT[act], lib)
        X = _logical_input(row, srcs)
        note = ""
        if kind == "integer":
            assert 6 * K + 12 < 2 ** 24                                     # sum |x| |w| + |b| + |r| <= 3 * 2 * K + 4 + 8: every partial sum exact in fp32
            ref, once = _exact_model(row, _conv_ref(row, X, w, OH, OW, torch.float32), b, r, act, to, geo)
            if not (odt == BF16 and twice):
                assert torch.equal(ref.float(), once.float()), "test error: the first rounding was expected to be exact here"
            bad = got.float() != ref.float()
            if bool(bad.any()):
                i = int(torch.nonzero(bad.flatten())[0])
                failures.append(f"integer: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at [b, y, x, c] = "
                                f"{_where(i, got.shape)}: got {float(got.flatten()[i])} exact {float(ref.flatten()[i])}")
        elif kind == "ones":
            cnt = F.conv2d(torch.ones(1, 1, H, W), torch.ones(1, 1, row["k"], row["k"]), stride=row["stride"], padding=row["pad"])[0, 0, :OH, :OW]
            ref = _shuffle((cnt * (c0 + c1)).view(1, OH, OW, 1).expand(B, OH, OW, row["Cout"]).contiguous(), row["shuffle_cout"]).to(to)
            bad = got.float() != ref.float()
            if bool(bad.any()):
                i = int(torch.nonzero(bad.flatten())[0])
                failures.append(f"ones: {int(bad.sum())} of {bad.numel()} elements wrong; first at [b, y, x, c] = {_where(i, got.shape)}: got "
                                f"{float(got.flatten()[i])}, {c0 + c1} channels x taps inside the image = {float(ref.flatten()[i])}")
        else:
            L = SLOPE[act]
            bd = b.double()
            v = _conv_ref(row, X, w, OH, OW, torch.float64) + bd
            A = _conv_ref(row, X.abs(), w.abs(), OH, OW, torch.float64) + bd.abs()
            aar, sc = row["act_after_res"], row["shuffle_cout"]
            t = _shuffle(v if aar else ACT_REF[act](v), sc)
            ref = t
            if r is not None or aar:
                ref = t + (_expand_res(row, r, B, OH, OW).double() if r is not None else 0.0)
                if aar:
                    ref = ACT_REF[act](ref)
            e_act = 0.0
            if fast and act == "gelu":
                e_act = 2.5e-5
            elif fast and act == "silu":
                e_act = 4 * 2.0 ** -24 * (ref if aar else t).abs()
            bound = u * ref.abs() + L * (K + 2) * 2.0 ** -24 * _shuffle(A, sc) + e_act + 1e-7
            if twice:
                bound = bound + (L if aar else 1.0) * u * t.abs()
            bound = bound * RELAX.get(row["id"], 1.0)
            err = (got.double() - ref).abs()
            ratio_random = float((err / bound).max())
            note = f"  max|err| {float(err.max()):.3e}  err/bound {ratio_random:.3f}"
            if not ratio_random <= 1.0:
                i = int(torch.argmax(err / bound))
                failures.append(f"random: err/bound {ratio_random:.3f} at [b, y, x, c] = {_where(i, got.shape)}: got {float(got.flatten()[i]):.6e} "
                                f"ref {float(ref.flatten()[i]):.6e} bound {float(bound.flatten()[i]):.3e}")
        print(f"{row['id']} {dt} {kind}: {tag}{note}")
        if stats is not None and _stats_failure(got, stats):
            failures.append(f"{kind}: " + _stats_failure(got, stats))
        if tag != expect:
            failures.append(f"{kind}: kernel {tag!r}, expected {expect!r}")
        if not bool(torch.isfinite(got.float()).all()):
            failures.append(f"{kind}: non-finite output")
        if not same:
            failures.append(f"{kind}: a second run of the same plan differs")
        if not clean:
            failures.append(f"{kind}: the sentinel around the output (padding columns / the spare image behind the last one) was overwritten")
    print(f"CONV-MATRIX {row['id']} {dt}: {expect}  random err/bound {ratio_random:.3f}  {time.time() - t_start:.1f} s")
    assert not failures, f"{row['id']} {dt}:\n  " + "\n  ".join(failures)
