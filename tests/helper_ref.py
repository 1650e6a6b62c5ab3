"""Plain references of the helper kernels in sam_ops.hip and vision_ops.hip, the seeded operands of every row of op_matrix.LN_ROWS / LN_DUAL_ROWS /
HELPER_ROWS and the bounds the helper matrix (tests/test_helper_matrix_gpu.py) holds the kernels to.  CPU only, plain torch: importing this module
needs neither a GPU nor the library.

Exact ops (SPPF pooling, casts and layout copies, max-pool, the u8 mask away from the threshold, the mask areas away from +-delta) are compared bit
for bit.  LayerNorm keeps the project's own bounds (_check_ln).  The other arithmetic ops follow tests/fused_ref.py: the reference states the op
in `dtype` on operands that arrive pre-rounded to their storage type and rounds where the kernel stores; dtype = float64 is the yardstick, the
same statement at float32 ("chain32") stands for an implementation that is right but computes in fp32 and calibrates the absolute term.
mutant= selects one deliberately wrong statement, so that tests/test_helper_ref_cpu.py can prove without a GPU that rows and bounds catch it.

`PYTHONPATH=. python tests/helper_ref.py` (from the repository root) prints the measured chain32 deviations behind CHAIN32_DEV."""
import functools
import zlib

import torch
import torch.nn.functional as F

from circuitvision_amd._lib import ACT_GELU, ACT_NONE, ACT_SILU, BF16, F16, F32

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
CODE = {"f16": F16, "bf16": BF16, "f32": F32}
ACT = {"none": ACT_NONE, "silu": ACT_SILU, "gelu": ACT_GELU}
SENTINEL = -12288.0                                    # exact in fp16 and bf16
LN_EPS = 1e-6

LN_MUTANTS = ("ln_stats_over_slots", "ln_rows_shift_at_wg", "ln_pad_row_uses_w")
HELPER_MUTANTS = ("sppf_clip_zero", "sppf_two_stages", "refine_pad_before_upsample", "refine_taps_transposed", "dw_tail_reads_next_row")

# |y - ref64| <= ATOL[family] + RTOL[stored type] |ref64| per element.  RTOL is one step of the stored output (a correct kernel may round the other
# way next to a tie).  ATOL = FACTOR x the largest |chain32 - ref64| over the rows of the family, measured on the CPU (main() below; the CPU test
# fails when a row change moves a measurement past its constant or leaves the constant more than 4 x too loose).  The factor covers what chain32
# does not reproduce: the kernels' summation order, fused multiply-adds, __expf / fast-reciprocal SiLU in fp16.  No kernel enters these numbers.
RTOL = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 2.0 ** -23}
FACTOR = 4.0
# measured largest |chain32 - ref64| per family (PYTHONPATH=. python tests/helper_ref.py), rounded up to two digits:
#   dwconv3x3_f32  4.8e-7   9 taps + bias + SiLU + residual on O(1) values
#   dwconv3x3_f16  0        on these rows the fp32 chain never rounds an fp16 output the other way.  Its outputs pass through the same fp32
#                           arithmetic as the f32 family's before the rounding, so its absolute term is the f32 family's (an output next to 0 has
#                           fp16 steps far below that arithmetic's error, which RTOL |ref64| cannot cover)
#   refine         2.9e-5   (constant 3.5e-5: the only statement that goes through a convolution library, whose summation order may differ by host) bilinear source coordinates in fp32 on a map with slopes ~6 per source pixel, up to 121 taps x 4 channels x 4 branches,
#                           exact GELU, combiner; outputs up to ~20
#   bilinear       1.3e-4   fp32 source coordinates (one ulp of 130 is 1.5e-5) times the steepest slope of the blob input (~25 per source pixel)
#   hyper_masks    3.2e-5   a sequential fp32 chain of up to 64 products; mask-0 values reach ~70 on the two stable images
CHAIN32_DEV = {"dwconv3x3_f16": 0.0, "dwconv3x3_f32": 4.8e-7, "refine": 3.5e-5, "bilinear": 1.3e-4, "hyper_masks": 3.2e-5}
ATOL = {k: FACTOR * v for k, v in CHAIN32_DEV.items()}
ATOL["dwconv3x3_f16"] += ATOL["dwconv3x3_f32"]


def rT(t, dt):
    """Round to the storage type dt ("f16" | "bf16" | "f32") and come back: the places where a kernel stores."""
    return t if dt == "f32" and t.dtype != torch.float64 else t.to(TDT[dt]).to(t.dtype)


def family(row, dt):
    return "dwconv3x3_" + dt if row["op"] == "dwconv3x3" else {"mask_postprocess": "bilinear"}.get(row["op"], row["op"])


def tol_ratio(y, ref64, fam, stored):
    """max over elements of |y - ref64| / (ATOL[fam] + RTOL[stored] |ref64|): <= 1 passes.  Also returns the largest |y - ref64|."""
    err = (y.double() - ref64.double()).abs()
    return float((err / (ATOL[fam] + RTOL[stored] * ref64.double().abs())).max()), float(err.max())


def _gen(rid, dt="", seed=0):
    return torch.Generator().manual_seed(zlib.crc32((rid + dt).encode()) + seed)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------------
def _ulp16(x, dtype):
    """One unit in the last place of the 16-bit type at |x| (bf16: 8 significant bits, fp16: 11, normal range)."""
    mant = 8 if dtype == BF16 else 11
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.pow(2.0, e - (mant - 1))


def _ln_ref(x, gam, bet, eps, act, denom=None):
    """denom (mutants only): what the row sums are divided by instead of the row width."""
    xd = x.double()
    if denom is None:
        mean, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    else:
        mean = xd.sum(-1, keepdim=True) / denom
        var = ((xd - mean) ** 2).sum(-1, keepdim=True) / denom
    xh = (xd - mean) / torch.sqrt(var + eps)
    y = xh * gam.double() + bet.double()
    scale = (xh * gam.double()).abs() + bet.double().abs()         # magnitude of the fp32 terms the kernel adds
    return (F.gelu(y) if act == ACT_GELU else y), scale


def ln_ratio(got, ref, scale, dout):
    """max err / bound under the project's LayerNorm bounds: 1e-5 + 1e-5 |ref| for f32 output; 2 ulp of the 16-bit result + the fp32 arithmetic
    that feeds the rounding (1e-6 scale) for 16-bit output."""
    err = (got.double() - ref).abs()
    bound = 1e-5 + 1e-5 * ref.abs() if dout == F32 else 2 * _ulp16(ref, dout) + 1e-6 * scale
    return float((err / bound).max()), float(err.max())


def _check_ln(got, ref, scale, dout, what):
    ratio, mx = ln_ratio(got, ref, scale, dout)
    print(f"{what}: max|err| {mx:.3e}  err/bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


def ln_types(row, dt):
    """(input, output) storage types of a LayerNorm row in dtype dt."""
    from op_matrix import LN_FORMS
    ti, to = LN_FORMS[row["form"]][:2]
    return (dt if ti == "16" else "f32"), (dt if to == "16" else "f32")


def ln_operands(row, dt):
    g = _gen(row["id"], dt)
    din = ln_types(row, dt)[0] if "form" in row else "f32"
    x = rT(torch.randn(row["rows"], row["C"], generator=g) * 3 + 1, din)
    return dict(x=x, gam=torch.rand(row["C"], generator=g) + 0.5, bet=torch.randn(row["C"], generator=g))


def ln_reference(row, o, mutant=None):
    """(ref64 [rows, C], scale) of a LayerNorm row."""
    assert mutant is None or mutant in LN_MUTANTS, mutant
    from op_matrix import LN_FORMS
    x, denom = o["x"], None
    if mutant == "ln_stats_over_slots":                   # mean and variance over every slot of the lane group, idle ones included
        denom = row["G"] * row["NCH"] * LN_FORMS[row["form"]][2]
    elif mutant == "ln_rows_shift_at_wg":                 # every workgroup but the first starts one row early
        wg = 4 * 64 // row["G"]
        assert row["rows"] > wg, "ln_rows_shift_at_wg needs a second workgroup"
        x = torch.cat((x[:wg], x[wg - 1:-1]))
    return _ln_ref(x, o["gam"], o["bet"], LN_EPS, ACT[row.get("act", "none")], denom)


def ln_grid(row, values, fill, mutant=None):
    """The output buffer's rows as the kernel must leave them: `values` [rows, C] scattered into the padded grid of a pad row (every other grid row
    keeps `fill`), or as they are."""
    if not row.get("pad"):
        return values
    H, W, Hp, Wp = row["pad"]
    r = torch.arange(row["rows"])
    img, rem = r // (H * W), r % (H * W)
    stride = W if mutant == "ln_pad_row_uses_w" else Wp     # the mutant strides the padded grid by the image width
    out = torch.full((row["rows"] // (H * W) * Hp * Wp, values.shape[1]), fill, dtype=values.dtype)
    out[img * Hp * Wp + (rem // W) * stride + rem % W] = values
    return out


@functools.lru_cache(maxsize=None)
def ln_case(rid, dt):
    """(row, operands, ref64, scale) of a LayerNorm row (LN_ROWS or LN_DUAL_ROWS): computed once per process, never modified."""
    from op_matrix import LN_DUAL_ROWS, LN_ROWS
    row = next(r for r in LN_ROWS + LN_DUAL_ROWS if r["id"] == rid)
    o = ln_operands(row, dt)
    ref, scale = ln_reference(row, o)
    return row, o, ref, scale


# ---- SPPF: three chained 5x5 / s1 / p2 max-pools, exact ----------------------------------------------------------------------------------------
def sppf_ref(x, mutant=None):
    """[B, C, H, W] -> [B, 4 C, H, W] = (x, y1, y2, y3).  max_pool2d pads with -inf, as the kernels clip their windows."""
    assert mutant in (None, "sppf_clip_zero", "sppf_two_stages"), mutant
    if mutant == "sppf_clip_zero":
        pool = lambda t: F.max_pool2d(F.pad(t, (2, 2, 2, 2), value=0.0), 5, 1, 0)
    else:
        pool = lambda t: F.max_pool2d(t, 5, 1, 2)
    y1 = pool(x)
    y2 = pool(y1)
    y3 = y2 if mutant == "sppf_two_stages" else pool(y2)   # the mutant's 13-window is the 9-window again
    return torch.cat((x, y1, y2, y3), 1)


# ---- upsample + MultiKernelRefinement ---------------------------------------------------------------------------------------------------------
def refine_params(o):
    """The flat parameter vector cvmi_upsample_refine reads: per branch weight [4, k, k] then bias [4]; combiner weight [nk * 4], bias [1]."""
    parts = []
    for w, b in zip(o["ws"], o["bs"]):
        parts += [w.reshape(-1), b]
    return torch.cat(parts + [o["cw"], o["cb"]])


def refine_ref(low, ws, bs, cw, cb, H, W, dtype=torch.float64, mutant=None):
    """out = combiner(cat_j GELU(conv_kj(up))) with up = bilinear(low -> H x W, align_corners False) and 'same' ZERO padding of `up`."""
    assert mutant in (None, "refine_pad_before_upsample", "refine_taps_transposed"), mutant
    low, cw, cb = low.to(dtype), cw.to(dtype), cb.to(dtype)
    ws, bs = [w.to(dtype) for w in ws], [b.to(dtype) for b in bs]
    if mutant == "refine_taps_transposed":
        j = max(range(len(ws)), key=lambda i: ws[i].shape[-1])
        ws[j] = ws[j].transpose(-1, -2)
    halo = max(w.shape[-1] for w in ws) // 2
    if mutant == "refine_pad_before_upsample":             # the low-resolution map is zero-padded and the halo is interpolated from it
        ys = ((torch.arange(-halo, H + halo, dtype=dtype) + 0.5) / H) * 2 - 1
        xs = ((torch.arange(-halo, W + halo, dtype=dtype) + 0.5) / W) * 2 - 1
        grid = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1)[None].expand(low.shape[0], -1, -1, -1)
        up = F.grid_sample(low, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    else:
        up = F.pad(F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False), (halo,) * 4)
    feats = []
    for w, b in zip(ws, bs):
        c = halo - w.shape[-1] // 2
        feats.append(F.gelu(F.conv2d(up[..., c:up.shape[-2] - c, c:up.shape[-1] - c], w, b)))
    return F.conv2d(torch.cat(feats, 1), cw.view(1, -1, 1, 1), cb)


# ---- depthwise 3x3 ----------------------------------------------------------------------------------------------------------------------------
def dwconv_ref(x, w, b, res, act, stored, dtype=torch.float64, mutant=None):
    """y = act(dw3x3(x) + b) [+ res] -> stored type.  Nine explicit taps, so the fp32 chain is the same sum on every machine."""
    assert mutant in (None, "dw_tail_reads_next_row"), mutant
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    if mutant == "dw_tail_reads_next_row":                  # column W of row y is the NHWC neighbour in memory: pixel 0 of row y + 1
        xp[:, :, 1:H, W + 1] = x[:, :, 1:, 0]
    acc = b.view(1, C, 1, 1).expand(B, C, H, W).clone()
    for ky in range(3):
        for kx in range(3):
            acc = acc + w[:, 0, ky, kx].view(1, C, 1, 1) * xp[:, :, ky:ky + H, kx:kx + W]
    y = F.silu(acc) if act == "silu" else acc
    if res is not None:
        y = y + res.to(dtype)
    return rT(y, stored)


# ---- bilinear resize, mask bits and extent ------------------------------------------------------------------------------------------------------
def bilinear_ref(low, H, W, dtype=torch.float64):
    return F.interpolate(low.to(dtype)[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]


def mask_and_extent(ref, thresh):
    """u8 mask {0, 255} of ref > thresh and its per-plane extent (x0, y0, x1, y1), {W, H, -1, -1} for an empty plane."""
    on = ref > thresh
    N, H, W = on.shape
    ext = []
    for n in range(N):
        ys, xs = torch.nonzero(on[n], as_tuple=True)
        ext.append([int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if ys.numel() else [W, H, -1, -1])
    return on.to(torch.uint8) * 255, torch.tensor(ext, dtype=torch.int32)


def clear_of(ref, level, fam="bilinear", stored="f32"):
    """No element of ref lies within the family's bound of `level`: a correct kernel cannot land on the other side."""
    return bool(((ref - level).abs() > ATOL[fam] + RTOL[stored] * ref.abs()).all())


# ---- mask decoder tail --------------------------------------------------------------------------------------------------------------------------
def hyper_ref(hyper, up, dtype=torch.float64):
    """masks [B, 4, P] = hyper [B, 4, C] x up [B, P, C]^T.  At float32: one sequential chain of C products per element (not a BLAS call, whose
    blocked summation is not what a plain fp32 implementation does)."""
    if dtype == torch.float64:
        return hyper.double() @ up.double().transpose(1, 2)
    acc = torch.zeros(hyper.shape[0], 4, up.shape[1], dtype=dtype)
    for c in range(hyper.shape[2]):
        acc = acc + hyper[:, :, c, None].to(dtype) * up[:, None, :, c].to(dtype)
    return acc


def select_ref(masks64, iou, delta, thresh):
    """(areas [B, 2], selected index [B]) of dynamic multimask-via-stability: mask 0 unless its stability (area above +delta / area above -delta)
    is below thresh, then the best of masks 1..3 by predicted IoU (first maximum)."""
    m0 = masks64[:, 0]
    areas = torch.stack(((m0 > delta).sum(1), (m0 > -delta).sum(1)), 1).int()
    stab = torch.where(areas[:, 1] > 0, areas[:, 0].float() / areas[:, 1].float().clamp(min=1), torch.ones(len(areas)))
    sel = torch.where(stab >= thresh, torch.zeros(len(areas), dtype=torch.long), 1 + iou[:, 1:4].argmax(1))
    return areas, sel.int(), stab


# ---- operands and references of a HELPER_ROWS row -----------------------------------------------------------------------------------------------
def operands(row, dt):
    """Seeded operands of one HELPER_ROWS row in dtype dt as CPU tensors whose values are already rounded to their storage type."""
    g = _gen("bilinear" if row["op"] in ("bilinear", "mask_postprocess") else row["id"], dt, row.get("seed", 0))               # seed: moved until the exact comparisons have nothing to excuse (test_helper_ref_cpu.py)
    op = row["op"]
    if op == "sppf_pool":                                   # mostly negative, borders included: a window clipped with 0 instead of -inf shows
        return dict(x=rT(torch.randn(row["B"], row["C"], row["H"], row["W"], generator=g) * 1.5 - 2.0, dt))
    if op == "refine":
        ks = row["ks"]
        return dict(low=torch.randn(row["N"], 1, row["h"], row["w"], generator=g) * 4,
                    ws=[torch.randn(4, 1, k, k, generator=g) / k for k in ks], bs=[0.1 * torch.randn(4, generator=g) for _ in ks],
                    cw=0.3 * torch.randn(4 * len(ks), generator=g), cb=0.1 * torch.randn(1, generator=g))
    if op == "dwconv3x3":
        B, C, H, W = row["B"], row["C"], row["H"], row["W"]
        return dict(x=rT(torch.randn(B, C, H, W, generator=g), dt), w=rT(torch.randn(C, 1, 3, 3, generator=g) / 3, dt), b=0.3 + 0.1 * torch.randn(C, generator=g),
                    res=rT(torch.randn(B, C, H, W, generator=g), dt) if row["res"] else None)
    if op in ("bilinear", "mask_postprocess"):              # one blob per plane on a negative background: the mask has a non-trivial extent
        N, h, w = row["N"], row["h"], row["w"]
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        low = torch.randn(N, h, w, generator=g) * 2
        for n in range(N):
            cy, cx = h * (0.35 + 0.3 * n), w * (0.6 - 0.25 * n)
            low[n] += torch.where(((yy - cy) / (0.22 * h)) ** 2 + ((xx - cx) / (0.3 * w)) ** 2 < 1, 10.0, -10.0)
        return dict(low=low)
    if op == "hyper_masks":
        B, P, C = row["B"], row["P"], row["C"]
        hyper = torch.randn(B, 4, C, generator=g) * 0.3
        hyper[:, 0] *= 8                                    # images 0 and 2: few mask-0 values inside +-delta -> stable
        hyper[1, 0] *= 1e-4                                 # image 1: every mask-0 value inside +-delta -> the dynamic fallback
        return dict(hyper=hyper, up=rT(torch.randn(B, P, C, generator=g), dt), iou=torch.rand(B, 4, generator=g))
    raise ValueError(op)


def reference(row, o, dt, dtype=torch.float64, mutant=None):
    op = row["op"]
    if op == "sppf_pool":
        return sppf_ref(o["x"], mutant)
    if op == "refine":
        return refine_ref(o["low"], o["ws"], o["bs"], o["cw"], o["cb"], row["H"], row["W"], dtype, mutant)
    if op == "dwconv3x3":
        return dwconv_ref(o["x"], o["w"], o["b"], o["res"], row["act"], dt, dtype, mutant)
    if op in ("bilinear", "mask_postprocess"):
        return bilinear_ref(o["low"], row["H"], row["W"], dtype)
    if op == "hyper_masks":
        return hyper_ref(o["hyper"], o["up"], dtype)
    raise ValueError(op)


TOLERANCED = ("refine", "dwconv3x3", "bilinear", "mask_postprocess", "hyper_masks")


@functools.lru_cache(maxsize=None)
def case(rid, dt):
    """(row, operands, reference) of a HELPER_ROWS row with a computed reference: once per process, shared, never modified."""
    from op_matrix import HELPER_ROWS
    row = next(r for r in HELPER_ROWS if r["id"] == rid)
    o = operands(row, dt)
    return row, o, reference(row, o, dt)


def measure_chain32():
    """{family: largest |chain32 - ref64|} over every toleranced row and dtype."""
    from op_matrix import HELPER_ROWS
    dev = {}
    for row in HELPER_ROWS:
        if row["op"] not in TOLERANCED or row["op"] == "mask_postprocess":
            continue
        for dt in row["dtypes"]:
            _, o, ref = case(row["id"], dt)
            fam = family(row, dt)
            d = float((reference(row, o, dt, torch.float32).double() - ref).abs().max())
            dev[fam] = max(dev.get(fam, 0.0), d)
    return dev


if __name__ == "__main__":
    for fam, d in sorted(measure_chain32().items()):
        print(f"{fam}: largest |chain32 - ref64| {d:.4e}   CHAIN32_DEV {CHAIN32_DEV[fam]:.4e}   ATOL {ATOL[fam]:.4e}")
