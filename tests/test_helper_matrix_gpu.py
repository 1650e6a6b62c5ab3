"""The helper-kernel matrix (tests/op_matrix.py LN_ROWS, LN_DUAL_ROWS, HELPER_ROWS): every template instance of layernorm_kernel in every type form,
both SPPF kernels on either side of the LDS limit, both refinement kernels, the depthwise 3x3 strip kernel at every strip tail, and the second pass
of every grid-capped loop -- each pinned by the tag cvmi_last_kernel() reports ("" for a dispatcher with one kernel) and compared with the
references of tests/helper_ref.py: bit for bit where the op is exact, under the project's LayerNorm bounds, or under
|y - ref64| <= ATOL[family] + RTOL[stored type] |ref64| with ATOL measured on the CPU (helper_ref.py), never from a kernel.
tests/test_helper_ref_cpu.py proves on the CPU that these comparisons catch the classic mistakes.

Every row also checks that sentinel columns, sentinel rows, padding and the guard elements behind an output are untouched, that input columns
outside the view hold values the kernel must not read, and that a second launch is bit-identical."""
import ctypes as C
import time

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from helper_ref import (ACT, CODE, LN_EPS, SENTINEL, TDT, _check_ln, case, family, ln_case, ln_grid, ln_ratio, ln_types, mask_and_extent, refine_params,
                        select_ref, sppf_ref, tol_ratio)
from op_matrix import HELPER_ROWS, LN_DUAL_ROWS, LN_ROWS, ln_tag

pytestmark = pytest.mark.gpu
ESIZE = {"f16": 2, "bf16": 2, "f32": 4}
GUARD = 64                                              # sentinel elements behind an output that has no leading dimension to widen


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _full(shape, dt, value=SENTINEL):
    return torch.full(shape, value, dtype=TDT[dt] if isinstance(dt, str) else dt, device="cuda")


def _noise(shape, dt, seed=1):
    """Values an output would visibly carry if the kernel read them."""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 64 + 512).to(TDT[dt]).cuda()


def _twice(lib, call, outs, reset=None):
    """Clear the tag, launch, read the tag, snapshot `outs`, launch again: (tag, first outputs on the CPU, second launch identical)."""
    lib.cvmi_last_kernel()
    torch.cuda.synchronize()
    _lib.check(call(), "first launch")
    torch.cuda.synchronize()
    tag = lib.cvmi_last_kernel().decode()
    first = [t.cpu() for t in outs]
    if reset is not None:
        reset()
        torch.cuda.synchronize()
    _lib.check(call(), "second launch")
    torch.cuda.synchronize()
    same = all(_same_bits(a, t.cpu()) for a, t in zip(first, outs))
    return tag, first, same


# ---- cvmi_layernorm ---------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(r["id"], dt) for r in LN_ROWS for dt in r["dtypes"]]


@pytest.mark.parametrize("rid,dt", LN_CASES, ids=["%s-%s" % c for c in LN_CASES])
def test_layernorm_matrix(rid, dt):
    """Every (form, G, NCH) of launch_ln in fp16 and bf16 (CODE: "f16" -> F16, "bf16" -> BF16, "f32" -> F32)."""
    lib = _lib.load()
    row, o, ref, scale = ln_case(rid, dt)
    din, dout = ln_types(row, dt)
    assert CODE[din] in (F16, BF16, F32) and CODE[dout] in (F16, BF16, F32)
    rows, C_ = row["rows"], row["C"]
    xbuf = _noise((rows, row["x_ld"]), din)
    xbuf[:, row["x_off"]:row["x_off"] + C_] = o["x"].to(TDT[din]).cuda()
    want = ln_grid(row, ref, float("nan"))                                     # [output rows, C]; NaN = a padding row of the grid
    ybuf = _full((want.shape[0], row["y_ld"]), dout)
    gam, bet = o["gam"].cuda(), o["bet"].cuda()
    pad = row["pad"] or (0, 0, 0, 0)

    def call():
        return lib.cvmi_layernorm(xbuf.data_ptr() + row["x_off"] * ESIZE[din], row["x_ld"], CODE[din], gam.data_ptr(), bet.data_ptr(),
                                  ybuf.data_ptr() + row["y_off"] * ESIZE[dout], row["y_ld"], CODE[dout], rows, C_, LN_EPS, ACT[row["act"]], *pad, None)

    tag, (first,), same = _twice(lib, call, [ybuf])
    got = first[:, row["y_off"]:row["y_off"] + C_]
    valid = ~torch.isnan(want[:, 0])
    ratio, mx = ln_ratio(got[valid], want[valid], scale, CODE[dout])
    print(f"LN-MATRIX {rid} {dt}: {tag}  G {row['G']}  max|err| {mx:.3e}  err/bound {ratio:.3f}")
    failures = []
    if tag != ln_tag(row["form"], row["NCH"], dt):
        failures.append(f"kernel {tag!r}, expected {ln_tag(row['form'], row['NCH'], dt)!r}")
    if not ratio <= 1.0:
        failures.append(f"err/bound {ratio:.3f}")
    if not bool((first[:, :row["y_off"]].float() == SENTINEL).all() and (first[:, row["y_off"] + C_:].float() == SENTINEL).all()):
        failures.append("columns outside the output view were written")
    if not bool((got[~valid].float() == SENTINEL).all()):
        failures.append("a padding row of the grid was written")
    if not same:
        failures.append("a second launch differs")
    assert not failures, f"{rid} {dt}:\n  " + "\n  ".join(failures)


LN_DUAL_CASES = [(r["id"], dt) for r in LN_DUAL_ROWS for dt in r["dtypes"]]


@pytest.mark.parametrize("rid,dt", LN_DUAL_CASES, ids=["%s-%s" % c for c in LN_DUAL_CASES])
def test_layernorm_dual_matrix(rid, dt):
    """cvmi_layernorm_dual in place on the f32 stream with an fp16 (F16) or bf16 (BF16) copy: the copy is the f32 result rounded to nearest even, bit
    for bit, inside a wider buffer."""
    lib = _lib.load()
    row, o, ref, scale = ln_case(rid, dt)
    rows, C_ = row["rows"], row["C"]
    x = o["x"].cuda()
    y2 = _full((rows, C_ + 8), dt)
    gam, bet = o["gam"].cuda(), o["bet"].cuda()

    def call():
        return lib.cvmi_layernorm_dual(x.data_ptr(), C_, gam.data_ptr(), bet.data_ptr(), x.data_ptr(), C_, y2.data_ptr(), C_ + 8, CODE[dt], rows, C_, LN_EPS, None)

    tag, (y, copy), same = _twice(lib, call, [x, y2], reset=lambda: x.copy_(o["x"]))
    assert tag == row["expect"], tag
    _check_ln(y, ref, scale, F32, f"LN-DUAL {rid} {dt}: {tag}")
    assert _same_bits(copy[:, :C_], y.to(TDT[dt])), "the 16-bit copy is not the f32 result rounded to nearest even"
    assert bool((copy[:, C_:].float() == SENTINEL).all()), "columns behind the copy were written"
    assert same, "a second launch differs"


# ---- HELPER_ROWS: one runner per op; each returns (tag, failures, one line for the log) ----------------------------------------------------------
def _nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


def _run_sppf(lib, row, dt):
    B, H, W, C_, ld = row["B"], row["H"], row["W"], row["C"], row["ld"]
    if row["B"] * H * W * C_ > 1 << 22:                                       # the one large row: not cached
        from helper_ref import operands
        o = operands(row, dt)
        ref = sppf_ref(o["x"])
    else:
        _, o, ref = case(row["id"], dt)
    buf = _full((B, H, W, ld), dt)
    buf[..., :C_] = _nhwc(o["x"], dt).cuda()
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_sppf_pool(buf.data_ptr(), ld, B, H, W, C_, CODE[dt], None), [buf])
    fails = []
    if not _same_bits(first[..., :4 * C_], _nhwc(ref, dt)):
        bad = (first[..., :4 * C_].float() != _nhwc(ref, dt).float())
        fails.append(f"{int(bad.sum())} of {bad.numel()} elements differ; by stage (x, y1, y2, y3): {[int(bad[..., i * C_:(i + 1) * C_].sum()) for i in range(4)]}")
    if not bool((first[..., 4 * C_:].float() == SENTINEL).all()):
        fails.append("columns behind the four stages were written")
    return tag, fails, same, "exact"


def _run_refine(lib, row, dt):
    _, o, ref = case(row["id"], dt)
    N, h, w, H, W, sh = row["N"], row["h"], row["w"], row["H"], row["W"], row["y_shift"]
    low, prm = o["low"].cuda(), refine_params(o).cuda()
    ks = (C.c_int * len(row["ks"]))(*row["ks"])
    out = _full((sh + N * H * W + GUARD,), "f32")
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_upsample_refine(low.data_ptr(), N, h, w, out.data_ptr() + 4 * sh, H, W, prm.data_ptr(), ks, len(row["ks"]), 4, None), [out])
    ratio, mx = tol_ratio(first[sh:sh + N * H * W].view(N, 1, H, W), ref, "refine", "f32")
    fails = [] if ratio <= 1.0 else [f"err/tol {ratio:.3f}"]
    if not bool((first[:sh] == SENTINEL).all() and (first[sh + N * H * W:] == SENTINEL).all()):
        fails.append("elements outside the output were written")
    return tag, fails, same, f"max|err| {mx:.3e}  err/tol {ratio:.3f}"


def _run_dwconv(lib, row, dt):
    _, o, ref = case(row["id"], dt)
    B, H, W, C_, g = row["B"], row["H"], row["W"], row["C"], row["y_guard"]
    xbuf = _noise((B, H, W, C_ + row["x_extra"]), dt)
    xbuf[..., row["x_off"]:row["x_off"] + C_] = _nhwc(o["x"], dt).cuda()
    wt = o["w"].reshape(C_, 9).t().contiguous().to(TDT[dt]).cuda()            # [9][C] tap-major
    bias = o["b"].cuda()
    res = _nhwc(o["res"], dt).cuda() if row["res"] else None
    ybuf = _full((B, H, W, C_ + 2 * g), dt)

    def call():
        return lib.cvmi_dwconv3x3(xbuf.data_ptr() + row["x_off"] * ESIZE[dt], xbuf.shape[-1], wt.data_ptr(), bias.data_ptr(), res.data_ptr() if row["res"] else None,
                                  C_, ybuf.data_ptr() + g * ESIZE[dt], ybuf.shape[-1], B, H, W, C_, ACT[row["act"]], CODE[dt], None)

    tag, (first,), same = _twice(lib, call, [ybuf])
    got = first[..., g:g + C_].permute(0, 3, 1, 2)
    ratio, mx = tol_ratio(got, ref, family(row, dt), dt)
    fails = [] if ratio <= 1.0 else [f"err/tol {ratio:.3f}"]
    if not bool((first[..., :g].float() == SENTINEL).all() and (first[..., g + C_:].float() == SENTINEL).all()):
        fails.append("guard channels around the output were written")
    return tag, fails, same, f"max|err| {mx:.3e}  err/tol {ratio:.3f}"


def _rand(shape, dt, seed, scale=8.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(TDT[dt])


def _exact(first, want, sentinel_part=None):
    fails = []
    if not _same_bits(first, want):
        fails.append(f"{int((_bits(first) != _bits(want)).sum())} of {want.numel()} elements differ" if first.shape == want.shape else f"shape {first.shape}")
    if sentinel_part is not None and not bool((sentinel_part.float() == SENTINEL).all()):
        fails.append("elements outside the output were written")
    return fails


def _run_cast(lib, row, dt):
    rows, C_, dst = row["rows"], row["C"], row["dst"]
    x = _noise((rows, row["x_ld"]), dt)
    src = _rand((rows, C_), dt, 3)
    x[:, :C_] = src.cuda()
    y = _full((rows, row["y_ld"]), dst)
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_cast(x.data_ptr(), row["x_ld"], CODE[dt], y.data_ptr(), row["y_ld"], CODE[dst], rows, C_, None), [y])
    return tag, _exact(first[:, :C_], src.to(TDT[dst]), first[:, C_:]), same, "exact"


def _run_maxpool(lib, row, dt):
    B, H, W, C_ = row["B"], row["H"], row["W"], row["C"]
    src = _rand((B, H, W, C_), dt, 4)
    x = src.cuda()
    y = _full((B, H // 2, W // 2, C_ + 8), dt)
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_maxpool2x2(x.data_ptr(), C_, y.data_ptr(), C_ + 8, B, H, W, C_, CODE[dt], None), [y])
    s = src.float()
    want = torch.maximum(torch.maximum(s[:, 0::2, 0::2], s[:, 0::2, 1::2]), torch.maximum(s[:, 1::2, 0::2], s[:, 1::2, 1::2])).to(TDT[dt])
    return tag, _exact(first[..., :C_], want, first[..., C_:]), same, "exact"


def _run_s2d4(lib, row, dt):
    B, H, W = row["B"], row["H"], row["W"]
    src = _rand((B, H, W, 3), dt, 5)
    x = src.cuda()
    n = B * (H // 4) * (W // 4) * 48
    y = _full((n + GUARD,), dt)
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_space_to_depth4(x.data_ptr(), y.data_ptr(), B, H, W, CODE[dt], None), [y])
    want = src.view(B, H // 4, 4, W // 4, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(-1)          # channel = (sy * 4 + sx) * 3 + c
    return tag, _exact(first[:n], want, first[n:]), same, "exact"


def _run_nchw_to_nhwc(lib, row, dt):
    B, C_, H, W, ld, dst = row["B"], row["C"], row["H"], row["W"], row["ld"], row["dst"]
    src = _rand((B, C_, H, W), dt, 6)
    x = src.cuda()
    y = _full((B, H, W, ld), dst)
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_nchw_to_nhwc(x.data_ptr(), CODE[dt], y.data_ptr(), CODE[dst], ld, B, C_, H, W, None), [y])
    return tag, _exact(first[..., :C_], src.permute(0, 2, 3, 1).to(TDT[dst]), first[..., C_:]), same, "exact"


def _run_nhwc_to_nchw(lib, row, dt):
    B, C_, H, W, ld = row["B"], row["C"], row["H"], row["W"], row["ld"]
    src = _rand((B, H, W, C_), dt, 7)
    x = _noise((B, H, W, ld), dt)
    x[..., :C_] = src.cuda()
    n = B * C_ * H * W
    y = _full((n + GUARD,), "f32")
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_nhwc_to_nchw_f32(x.data_ptr(), CODE[dt], ld, y.data_ptr(), B, C_, H, W, None), [y])
    return tag, _exact(first[:n], src.permute(0, 3, 1, 2).float().reshape(-1), first[n:]), same, "exact"


def _run_repeat(lib, row, dt):
    B, rep, chunks = row["B"], row["rep"], row["chunks"]
    src = _rand((B, chunks * 4), "f32", 8)
    x = src.cuda()
    n = B * rep * chunks * 4
    y = _full((n + GUARD,), "f32")
    tag, (first,), same = _twice(lib, lambda: lib.cvmi_repeat_images(x.data_ptr(), y.data_ptr(), chunks * 16, B, rep, None), [y])
    return tag, _exact(first[:n], src.repeat_interleave(rep, 0).reshape(-1), first[n:]), same, "exact"


def _run_bilinear(lib, row, dt):
    _, o, ref = case(row["id"], dt)
    N, h, w, H, W = row["N"], row["h"], row["w"], row["H"], row["W"]
    low = o["low"].cuda()
    n = N * H * W
    mask = torch.full((n + GUARD,), 7, dtype=torch.uint8, device="cuda")
    want_mask, want_ext = mask_and_extent(ref, 0.0)
    if row["op"] == "bilinear":
        y = _full((n + GUARD,), "f32")
        tag, (first, m), same = _twice(lib, lambda: lib.cvmi_bilinear_f32(low.data_ptr(), N, h, w, y.data_ptr(), H, W, mask.data_ptr(), 0.0, None), [y, mask])
        ratio, mx = tol_ratio(first[:n].view(N, H, W), ref, "bilinear", "f32")
        fails = [] if ratio <= 1.0 else [f"err/tol {ratio:.3f}"]
        if not bool((first[n:] == SENTINEL).all()):
            fails.append("elements behind the map were written")
        info = f"max|err| {mx:.3e}  err/tol {ratio:.3f}"
    else:
        ext = torch.full((N + 2, 4), -7, dtype=torch.int32, device="cuda")
        tag, (m, e), same = _twice(lib, lambda: lib.cvmi_mask_postprocess(low.data_ptr(), N, h, w, H, W, 0.0, mask.data_ptr(), ext.data_ptr(), None), [mask, ext])
        fails = [] if torch.equal(e[:N], want_ext) and bool((e[N:] == -7).all()) else [f"extent {e.tolist()}, expected {want_ext.tolist()}"]
        info = "exact"
    if not torch.equal(m[:n].view(N, H, W), want_mask):                        # no reference value lies within the bound of the threshold (CPU test)
        fails.append(f"{int((m[:n].view(N, H, W) != want_mask).sum())} mask elements differ")
    if not bool((m[n:] == 7).all()):
        fails.append("elements behind the mask were written")
    return tag, fails, same, info


def _run_hyper(lib, row, dt):
    _, o, ref = case(row["id"], dt)
    B, P, C_, up_ld = row["B"], row["P"], row["C"], row["up_ld"]
    up = _noise((B, P, up_ld), dt)
    up[..., :C_] = o["up"].to(TDT[dt]).cuda()
    hyper, iou = o["hyper"].cuda(), o["iou"].cuda()
    masks, low = _full((B * 4 * P + GUARD,), "f32"), _full((B * P + GUARD,), "f32")
    areas = torch.full((B + 1, 2), -7, dtype=torch.int32, device="cuda")
    iou_o, sel = _full((B + 1,), "f32"), torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")

    def call():
        rc = lib.cvmi_hyper_masks(hyper.data_ptr(), C_, up.data_ptr(), up_ld, CODE[dt], C_, masks.data_ptr(), areas.data_ptr(), B, P, row["delta"], None)
        return rc or lib.cvmi_select_mask(masks.data_ptr(), areas.data_ptr(), iou.data_ptr(), 4, 1, row["thresh"], low.data_ptr(), iou_o.data_ptr(), sel.data_ptr(), B, P, None)

    tag, (m, a, lo, io, s), same = _twice(lib, call, [masks, areas, low, iou_o, sel])
    got = m[:B * 4 * P].view(B, 4, P)
    ratio, mx = tol_ratio(got, ref, "hyper_masks", "f32")
    want_areas, want_sel, _ = select_ref(ref, o["iou"], row["delta"], row["thresh"])
    fails = [] if ratio <= 1.0 else [f"err/tol {ratio:.3f}"]
    if not torch.equal(a[:B], want_areas):                                     # no mask-0 value lies within the bound of +-delta (CPU test)
        fails.append(f"areas {a[:B].tolist()}, expected {want_areas.tolist()}")
    if not torch.equal(s[:B], want_sel):
        fails.append(f"selected {s[:B].tolist()}, expected {want_sel.tolist()}")
    else:
        pick = torch.stack([got[b, int(want_sel[b])] for b in range(B)])
        if not _same_bits(lo[:B * P].view(B, P), pick):
            fails.append("the selected mask is not a copy of the mask it names")
        if not _same_bits(io[:B], torch.stack([o["iou"][b, int(want_sel[b])] for b in range(B)])):
            fails.append("iou_out is not the selected mask's score")
    if not bool((m[B * 4 * P:] == SENTINEL).all() and (lo[B * P:] == SENTINEL).all() and (a[B:] == -7).all() and (s[B:] == -7).all() and (io[B:] == SENTINEL).all()):
        fails.append("elements behind an output were written")
    return tag, fails, same, f"max|err| {mx:.3e}  err/tol {ratio:.3f}"


RUNNERS = {"sppf_pool": _run_sppf, "refine": _run_refine, "dwconv3x3": _run_dwconv, "cast": _run_cast, "maxpool2x2": _run_maxpool, "space_to_depth4": _run_s2d4,
           "nchw_to_nhwc": _run_nchw_to_nhwc, "nhwc_to_nchw_f32": _run_nhwc_to_nchw, "repeat_images": _run_repeat, "bilinear": _run_bilinear,
           "mask_postprocess": _run_bilinear, "hyper_masks": _run_hyper}
HELPER_CASES = [(r, dt) for r in HELPER_ROWS for dt in r["dtypes"]]


@pytest.mark.parametrize("row,dt", HELPER_CASES, ids=["%s-%s" % (r["id"], dt) for r, dt in HELPER_CASES])
def test_helper_matrix(row, dt):
    lib = _lib.load()
    t0 = time.time()
    tag, failures, same, info = RUNNERS[row["op"]](lib, row, dt)
    print(f"HELPER-MATRIX {row['id']} {dt}: {tag or '(untagged)'}  {info}  {time.time() - t0:.1f} s")
    if tag != row["expect"]:
        failures.insert(0, f"kernel {tag!r}, expected {row['expect']!r}")
    if not same:
        failures.append("a second launch differs")
    assert not failures, f"{row['id']} {dt}:\n  " + "\n  ".join(failures)


# ---- argument rejection: every call below returns before any launch ---------------------------------------------------------------------------
def _rejected(lib, rc, text):
    assert rc != 0
    err = lib.cvmi_last_error().decode()
    assert text in err, err
    assert lib.cvmi_last_kernel().decode() == "", "a rejected call must not reach a launch"


def test_layernorm_rejects_bad_arguments():
    lib = _lib.load()
    wide = 4 * (64 * 9 + 1)                                                    # one f32 chunk more than 64 lanes x 9 slots hold
    x, y = torch.zeros(2, wide + 8, device="cuda"), torch.zeros(2, wide + 8, device="cuda")
    gam = torch.ones(wide + 8, device="cuda")
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()

    def call(C_=96, x_ld=wide, y_ld=wide, xoff=0, ydt=F32, pad=(0, 0, 0, 0)):
        return lib.cvmi_layernorm(x.data_ptr() + xoff, x_ld, F32, gam.data_ptr(), gam.data_ptr(), y.data_ptr(), y_ld, ydt, 2, C_, LN_EPS, 0, *pad, None)

    _rejected(lib, call(C_=wide), "too wide")
    _rejected(lib, call(C_=2 * wide, x_ld=2 * wide, y_ld=2 * wide, ydt=F16), "too wide")     # the wide f32 -> fp16 form: slots of 8
    _rejected(lib, call(xoff=4), "not 16-byte aligned")
    _rejected(lib, call(x_ld=wide + 2), "not 16-byte aligned")
    _rejected(lib, call(C_=98), "not 16-byte aligned")
    _rejected(lib, call(x_ld=92), "not 16-byte aligned")                        # x_ld < C
    _rejected(lib, call(pad=(5, 7, 8, 8)), "bad padding geometry")              # 2 rows are no whole 5 x 7 image
    _rejected(lib, lib.cvmi_layernorm_dual(x.data_ptr(), wide, gam.data_ptr(), gam.data_ptr(), x.data_ptr(), wide, y.data_ptr(), wide, F16, 2, 96, LN_EPS, None),
              "not 16-byte aligned")
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0


def test_sppf_pool_rejects_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(2, 4, 4, 64, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _rejected(lib, lib.cvmi_sppf_pool(buf.data_ptr() + 2, 64, 2, 4, 4, 16, F16, None), "pointer not 16-byte aligned")
    _rejected(lib, lib.cvmi_sppf_pool(buf.data_ptr(), 56, 2, 4, 4, 16, F16, None), "bad shape")        # ld < 4 C
    _rejected(lib, lib.cvmi_sppf_pool(buf.data_ptr(), 64, 2, 4, 4, 12, F16, None), "bad shape")        # C not in 16-byte chunks
    _rejected(lib, lib.cvmi_sppf_pool(buf.data_ptr(), 68, 2, 4, 4, 16, F16, None), "bad shape")        # ld not in 16-byte chunks
    _rejected(lib, lib.cvmi_sppf_pool(buf.data_ptr(), 64, 2, 4, 4, 16, BF16, None), "bad dtype")
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def test_upsample_refine_rejects_bad_arguments():
    lib = _lib.load()
    low, out, prm = torch.zeros(1, 8, 8, device="cuda"), torch.zeros(1, 16, 16, device="cuda"), torch.zeros(2048, device="cuda")
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()

    def call(ks, ic=4):
        return lib.cvmi_upsample_refine(low.data_ptr(), 1, 8, 8, out.data_ptr(), 16, 16, prm.data_ptr(), (C.c_int * len(ks))(*ks), len(ks), ic, None)

    _rejected(lib, call((3, 4, 7)), "kernel sizes must be odd")
    _rejected(lib, call((3, 5, 7, 17)), "kernel sizes must be odd and <= 15")
    _rejected(lib, call((3, 5, 7, 11, 13)), "branches of 4 channels")
    _rejected(lib, call((3, 5), ic=8), "branches of 4 channels")
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
