"""Plain references of the three fused YOLO11 kernels (c3k2_fused.hip, stem_fused.hip, dwpw_fused.hip), the seeded operands of every row of
op_matrix.FUSED_ROWS and the tolerance the fused matrix holds the kernels to.  CPU only, plain torch: importing this module needs neither a
GPU nor the library.

Each reference states the block with F.conv2d in `dtype` on operands that arrive pre-rounded to fp16 (biases stay f32, as the kernels read
them) and rounds to fp16 exactly where the kernel's contract says it stores fp16.  dtype = float64 is the yardstick; the same function at
float32 ("chain32") stands for an implementation that is right but accumulates in fp32, and calibrates the tolerance.  mutant= selects one
deliberately wrong statement -- the classic mistakes of a fused conv chain -- so that tests/test_fused_ref_cpu.py can prove, without a GPU,
that the rows and the tolerance would catch them.  All tensors are NCHW."""
import functools
import zlib

import torch
import torch.nn.functional as F

C3K2_MUTANTS = ("t_from_padded_b", "ab_bias_outside", "no_shortcut", "always_shortcut", "rows_bleed")
STEM2_MUTANTS = ("stem_t_bias_outside", "rows_bleed")
DWPW_MUTANTS = ("dw_first_chunk_taps", "rows_bleed")

# |y - ref64| <= ATOL[kernel] + RTOL |ref64| per element.  RTOL is one fp16 step of the stored output: a correct kernel may round the other way
# when its fp32 value sits next to a tie.  ATOL = FACTOR x the largest |chain32 - ref64| over all non-persistent rows of the kernel (measured
# on the CPU by test_fused_ref_cpu.py, which fails when a row change moves it past the constant): the fp32 chain's own deviation, the
# occasional one-step flip of an fp16 intermediate or of the output included.  The factor covers what chain32 does not reproduce: the MFMA
# summation order and the kernels' __expf / fast-reciprocal SiLU.  The kernel under test never enters these numbers.
RTOL = 2.0 ** -10
FACTOR = 4.0
# measured largest |chain32 - ref64|: c3k2 1.953e-3 (2^-9), stem2 9.766e-4 (2^-10), dwpw 1.953e-3 (2^-9) -- each is ONE fp16 step of an output in
# [2, 4) resp. [1, 2) that the fp32 chain rounds the other way; beyond RTOL |ref64| the chain deviates by at most 4.6e-4 / 7.2e-5 / 1.6e-4
CHAIN32_DEV = {"c3k2": 2.0 ** -9, "stem2": 2.0 ** -10, "dwpw": 2.0 ** -9}
ATOL = {k: FACTOR * v for k, v in CHAIN32_DEV.items()}             # c3k2 7.8125e-3, stem2 3.90625e-3, dwpw 7.8125e-3


def r16(t):
    """Round to fp16 and come back: the places where a kernel stores fp16."""
    return t.to(torch.float16).to(t.dtype)


def _cast(dtype, *ts):
    return [None if t is None else t.to(dtype) for t in ts]


def _tall(x):
    """[B, C, H, W] -> [1, C, B H, W]: the batch as one tall image (what a kernel sees when its row test forgets the image boundary)."""
    B, C, H, W = x.shape
    return x.permute(1, 0, 2, 3).reshape(1, C, B * H, W)


def _untall(y, B):
    _, C, BH, W = y.shape
    return y.reshape(C, B, BH // B, W).permute(1, 0, 2, 3).contiguous()


def _ring(inner, fill, n=1):
    """`inner` with a ring of n pixels around it that holds the per-channel value `fill`."""
    B, C, H, W = inner.shape
    out = fill.view(1, C, 1, 1).expand(B, C, H + 2 * n, W + 2 * n).clone()
    out[:, :, n:-n, n:-n] = inner
    return out


def c3k2_ref(x, w0, b0, w1, b1, w2, b2, w3, b3, shortcut, fuse_cv1, dtype=torch.float64, mutant=None):
    """C3k2 (c3k = False, n = 1) as the header of c3k2_fused.hip states it:
        [a|b] = SiLU(cv1 x)              1x1, only with fuse_cv1 (else x IS [a|b])          -> fp16
        t     = SiLU(m.cv1 (*) b)        3x3, zero padding                                  -> fp16
        s     = SiLU(m.cv2 (*) t)        3x3, zero padding                                  -> fp16
        m     = b + s  (shortcut) | s                                                       -> fp16
        out   = SiLU(cv2 [a|b|m])        1x1                                                -> fp16"""
    assert mutant is None or mutant in C3K2_MUTANTS, mutant
    if mutant == "rows_bleed":
        return _untall(c3k2_ref(_tall(x), w0, b0, w1, b1, w2, b2, w3, b3, shortcut, fuse_cv1, dtype), x.shape[0])
    x, w0, b0, w1, b1, w2, b2, w3, b3 = _cast(dtype, x, w0, b0, w1, b1, w2, b2, w3, b3)
    if mutant == "no_shortcut":
        shortcut = False
    elif mutant == "always_shortcut":
        shortcut = True
    ab = r16(F.silu(F.conv2d(x, w0, b0))) if fuse_cv1 else x
    c = ab.shape[1] // 2
    b = ab[:, c:]
    if mutant == "t_from_padded_b":                       # t on the ring around the image is SiLU(b1 + taps inside) instead of m.cv2's zero padding
        t = r16(F.silu(F.conv2d(F.pad(b, (2, 2, 2, 2)), w1, b1)))
        s = r16(F.silu(F.conv2d(t, w2, b2)))
    else:
        if mutant == "ab_bias_outside":                   # cv1 of the zero-filled halo: SiLU(b0), not m.cv1's zero padding
            assert fuse_cv1, "ab_bias_outside needs the fused cv1"
            t = r16(F.silu(F.conv2d(_ring(b, r16(F.silu(b0))[c:]), w1, b1)))
        else:
            t = r16(F.silu(F.conv2d(b, w1, b1, padding=1)))
        s = r16(F.silu(F.conv2d(t, w2, b2, padding=1)))
    m = r16(s + b) if shortcut else s
    return r16(F.silu(F.conv2d(torch.cat((ab, m), 1), w3, b3)))


def stem2_ref(img, w0, b0, w1, b1, dtype=torch.float64, mutant=None):
    """model.0 + model.1 on the original image [B, 3, 2 H2, 2 W2]: t = SiLU(conv 3x3 s2 p1) -> fp16, out = SiLU(conv 3x3 s2 p1 (t)) -> fp16."""
    assert mutant is None or mutant in STEM2_MUTANTS, mutant
    if mutant == "rows_bleed":
        assert img.shape[2] % 4 == 0, "rows_bleed: every image must end on a whole output row"
        return _untall(stem2_ref(_tall(img), w0, b0, w1, b1, dtype), img.shape[0])
    img, w0, b0, w1, b1 = _cast(dtype, img, w0, b0, w1, b1)
    t = r16(F.silu(F.conv2d(img, w0, b0, stride=2, padding=1)))
    if mutant == "stem_t_bias_outside":                   # model.0 of the zero-filled patch outside the image: SiLU(b0), not model.1's zero padding
        return r16(F.silu(F.conv2d(_ring(t, r16(F.silu(b0))), w1, b1, stride=2)))
    return r16(F.silu(F.conv2d(t, w1, b1, stride=2, padding=1)))


def dwpw_ref(x, wd, bd, w1, b1, w2=None, b2=None, dtype=torch.float64, mutant=None):
    """u = SiLU(dw 3x3 (*) x) -> fp16, v = SiLU(pw1 u) -> fp16, out = v | pw2 v (no activation) -> fp16."""
    assert mutant is None or mutant in DWPW_MUTANTS, mutant
    if mutant == "rows_bleed":
        return _untall(dwpw_ref(_tall(x), wd, bd, w1, b1, w2, b2, dtype), x.shape[0])
    x, wd, bd, w1, b1, w2, b2 = _cast(dtype, x, wd, bd, w1, b1, w2, b2)
    C = x.shape[1]
    if mutant == "dw_first_chunk_taps":                   # the taps staged for chunk 0 serve every 64-channel chunk
        assert C > 64, "dw_first_chunk_taps needs more than one chunk"
        wd = wd[:64].repeat(C // 64, 1, 1, 1)
    u = r16(F.silu(F.conv2d(x, wd, bd, padding=1, groups=C)))
    v = r16(F.silu(F.conv2d(u, w1, b1)))
    return v if w2 is None else r16(F.conv2d(v, w2, b2))


# ---- operands of a row --------------------------------------------------------------------------------------------------------------------
def _gen(row):
    return torch.Generator().manual_seed(zlib.crc32(row["id"].encode()) + row.get("seed", 0))


def _w(g, n, cin, k, groups_fan=None):
    fan = groups_fan or cin * k * k
    return r16(torch.randn(n, cin, k, k, generator=g) / fan ** 0.5)


def _b(g, n):
    return 0.3 + 0.1 * torch.randn(n, generator=g)        # f32, as the kernels read them


def operands(row, B=None):
    """Seeded operands of one FUSED_ROWS row as a dict of CPU float32 tensors (values already rounded to fp16, biases f32): inputs randn, weights
    randn / sqrt(fan_in), biases about 0.3, so every stage's activations are O(1) and every image of the batch differs.  B: the batch of a
    persistent row, which is only known on the device."""
    g = _gen(row)
    B = row["B"] if B is None else B
    H, W = row["H"], row["W"]
    if row["kernel"] == "c3k2":
        C, HR, C2, C1 = row["inst"]
        o = dict(x=r16(torch.randn(B, C1 or 2 * C, H, W, generator=g)), w0=None, b0=None)
        if C1:
            o.update(w0=_w(g, 2 * C, C1, 1), b0=_b(g, 2 * C))
        o.update(w1=_w(g, HR, C, 3), b1=_b(g, HR), w2=_w(g, C, HR, 3), b2=_b(g, C), w3=_w(g, C2, 3 * C, 1), b3=_b(g, C2))
        return o
    if row["kernel"] == "stem2":                          # H, W: the space-to-depth grid; the image is twice that
        return dict(img=r16(torch.randn(B, 3, 2 * H, 2 * W, generator=g)), w0=_w(g, 16, 3, 3), b0=_b(g, 16), w1=_w(g, 32, 16, 3), b1=_b(g, 32))
    C, N1, N2 = row["C"], row["N1"], row["N2"]
    o = dict(x=r16(torch.randn(B, C, H, W, generator=g)), wd=_w(g, C, 1, 3), bd=_b(g, C), w1=_w(g, N1, C, 1), b1=_b(g, N1), w2=None, b2=None)
    if N2:
        o.update(w2=_w(g, N2, N1, 1), b2=_b(g, N2))
    return o


def reference(row, o, dtype=torch.float64, mutant=None):
    """The row's output [B, C, H, W] in `dtype` from operands `o`."""
    if row["kernel"] == "c3k2":
        return c3k2_ref(o["x"], o["w0"], o["b0"], o["w1"], o["b1"], o["w2"], o["b2"], o["w3"], o["b3"], bool(row["shortcut"]), row["inst"][3] > 0, dtype, mutant)
    if row["kernel"] == "stem2":
        return stem2_ref(o["img"], o["w0"], o["b0"], o["w1"], o["b1"], dtype, mutant)
    return dwpw_ref(o["x"], o["wd"], o["bd"], o["w1"], o["b1"], o["w2"], o["b2"], dtype, mutant)


@functools.lru_cache(maxsize=None)
def _row_case(rid):
    from op_matrix import FUSED_ROWS
    row = next(r for r in FUSED_ROWS if r["id"] == rid)
    o = operands(row)
    return row, o, reference(row, o)


def row_case(rid):
    """(row, operands, fp64 reference) of a non-persistent row: computed once per process, shared by every test, never modified."""
    return _row_case(rid)


def tol_ratio(y, ref64, kernel, atol=None):
    """max over elements of |y - ref64| / (atol + RTOL |ref64|): <= 1 passes.  Also returns the largest |y - ref64|."""
    atol = ATOL[kernel] if atol is None else atol
    err = (y.double() - ref64.double()).abs()
    return float((err / (atol + RTOL * ref64.double().abs())).max()), float(err.max())
