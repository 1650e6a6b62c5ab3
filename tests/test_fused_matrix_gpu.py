"""The fused-kernel matrix (tests/op_matrix.py FUSED_ROWS): every built instance of c3k2_kernel, stem2_kernel and dwpw_kernel, pinned by the tag
cvmi_last_kernel() reports, at the sizes where a fused conv chain goes wrong -- below one tile, exactly one tile, one pixel past a tile, an
interior tile, the input inside a wider buffer, guard channels around the output, and (c3k2) the persistent tile loop with at least two tiles
on EVERY workgroup -- against the fp64 reference of tests/fused_ref.py under |y - ref64| <= ATOL[kernel] + 2^-10 |ref64| per element.  ATOL comes
from the CPU (fused_ref.py: 4 x the fp32 chain's own deviation from fp64), never from a kernel; tests/test_fused_ref_cpu.py proves on the CPU
that this comparison catches a chain whose halo handling, shortcut, batch boundary or per-chunk taps are wrong.

Each row also checks that channels outside the output view (guards, the padding behind a ragged channel tail) and one spare image behind the last
are still exactly zero, that every channel of the input buffer outside the view holds noise the kernel must not read, and that a second launch is
bit-identical."""
import ctypes as C
import time

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import F16, F32
from circuitvision_amd.engine import Buf, PackedConv, PackedDW, Plan, op_c3k2, op_dwpw, op_stem2
from fused_ref import ATOL, operands, reference, row_case, tol_ratio
from helpers import run, stream
from op_matrix import C3K2_TILE, FUSED_ROWS

pytestmark = pytest.mark.gpu


def _cu_count(lib):
    info = (C.c_int * 4)()
    assert lib.cvmi_device_info(0, info) == 0
    return int(info[0])


def persistent_batch(row, ncu):
    """Smallest B of a persistent row for which every workgroup runs >= 2 tiles whatever occupancy the launcher's query returned (grid <= k CUs,
    k = the hardware ceiling of resident workgroups per CU): tiles >= 2 k CUs + 5; and for which no possible grid (w CUs, w = 1..k) divides the
    tile count, so some workgroups run one tile more than others."""
    tpi = -(-row["H"] // C3K2_TILE[0]) * -(-row["W"] // C3K2_TILE[1])
    need = 2 * row["k"] * ncu + 5
    B = -(-need // tpi)
    while any(B * tpi % (w * ncu) == 0 for w in range(1, row["k"] + 1)):
        B += 1
    return B, B * tpi


def _input_buf(x, row):
    """NCHW fp16-valued tensor -> Buf with the tensor at channel x_off; every other channel holds noise."""
    B, c, H, W = x.shape
    buf = Buf(B, H, W, c + row["x_extra"], F16)
    if row["x_extra"]:
        buf.t.copy_(torch.randn(buf.t.shape, generator=torch.Generator().manual_seed(1)).to(torch.float16) * 4 + 8)
    buf.t[..., row["x_off"]:row["x_off"] + c] = x.permute(0, 2, 3, 1).to(torch.float16).cuda()
    return buf.view(row["x_off"], c)


def _s2d(img, w0):
    """Image [B, 3, 2 H2, 2 W2] -> space-to-depth(2) [B, 16, H2, W2] (12 real channels, (sy, sx, rgb) order), and model.0's 3x3 / s2 weights as
    the 2x2 / s1 conv on it that Yolo11Weights.stem packs: window row ky sits in block row ty with sub-row sy: 0 -> (0, 1), 1 -> (1, 0), 2 -> (1, 1)."""
    B, _, H, W = img.shape
    x = torch.zeros(B, 16, H // 2, W // 2)
    x[:, :12] = img.reshape(B, 3, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 12, H // 2, W // 2)
    w = torch.zeros(w0.shape[0], 16, 2, 2)
    m = {0: (0, 1), 1: (1, 0), 2: (1, 1)}
    for ky in range(3):
        for kx in range(3):
            (ty, sy), (tx, sx) = m[ky], m[kx]
            w[:, (sy * 2 + sx) * 3:(sy * 2 + sx) * 3 + 3, ty, tx] = w0[:, :, ky, kx]
    return x, w


def build_plan(row, o):
    """(plan, output Buf with one spare image, channel offset of the view, its width) for one row's launch."""
    g, kern = row["y_guard"], row["kernel"]
    plan = Plan(stream())
    if kern == "c3k2":
        c, h, c2, c1 = row["inst"]
        src = _input_buf(o["x"], row)
        nout = c2
        yb = Buf(src.B + 1, src.H, src.W, nout + 2 * g, F16, zero=True)
        pc0 = PackedConv(o["w0"], o["b0"], F16) if c1 else None
        op_c3k2(plan, row["id"], src, yb.images(0, src.B).view(g, nout), pc0, PackedConv(o["w1"], o["b1"], F16), PackedConv(o["w2"], o["b2"], F16),
                PackedConv(o["w3"], o["b3"], F16), c, h, fuse_cv1=c1 > 0, shortcut=bool(row["shortcut"]))
    elif kern == "stem2":
        x, w0 = _s2d(o["img"], o["w0"])
        src = _input_buf(x, row)
        nout = 32
        yb = Buf(src.B + 1, (src.H - 1) // 2 + 1, (src.W - 1) // 2 + 1, nout + 2 * g, F16, zero=True)
        op_stem2(plan, row["id"], PackedConv(w0, o["b0"], F16), PackedConv(o["w1"], o["b1"], F16), src, yb.images(0, src.B).view(g, nout))
    else:
        src = _input_buf(o["x"], row)
        nout = row["N2"] or row["N1"]
        yb = Buf(src.B + 1, src.H, src.W, -(-nout // 8) * 8 + 2 * g, F16, zero=True)
        pc2 = PackedConv(o["w2"], o["b2"], F16) if row["N2"] else None
        op_dwpw(plan, row["id"], PackedDW(o["wd"], o["bd"], F16), PackedConv(o["w1"], o["b1"], F16), src, yb.images(0, src.B).view(g, nout), pc2=pc2)
    return plan, yb, g, nout


@pytest.mark.parametrize("row", FUSED_ROWS, ids=[r["id"] for r in FUSED_ROWS])
def test_fused_matrix(row):
    lib = _lib.load()
    t_start = time.time()
    note = ""
    if row["B"] == "persist":
        ncu = _cu_count(lib)
        B, ntiles = persistent_batch(row, ncu)
        assert ntiles >= 2 * row["k"] * ncu + 5
        note = f"  B {B}: {ntiles} tiles on {ncu} CUs, at most {row['k']} workgroups per CU -> every workgroup runs >= {ntiles // (row['k'] * ncu)} tiles"
        o = operands(row, B)
        ref = reference(row, o)
    else:
        _, o, ref = row_case(row["id"])
        B = row["B"]
    plan, yb, g, nout = build_plan(row, o)
    lib.cvmi_last_kernel()                                                 # clears the tag
    run(plan)
    tag = lib.cvmi_last_kernel().decode()
    first = yb.t.clone()
    run(plan)
    same = torch.equal(yb.t, first)
    got = first[:B, :, :, g:g + nout].permute(0, 3, 1, 2).float().cpu()
    outside = torch.cat((first[:B, :, :, :g].flatten(), first[:B, :, :, g + nout:].flatten(), first[B].flatten()))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ratio, mx = tol_ratio(got, ref, row["kernel"])
    print(f"FUSED-MATRIX {row['id']}: {tag}  max|err| {mx:.3e}  err/tol {ratio:.3f}  (atol {ATOL[row['kernel']]:.3e}){note}  {time.time() - t_start:.1f} s")
    failures = []
    if tag != row["expect"]:
        failures.append(f"kernel {tag!r}, expected {row['expect']!r}")
    if not bool(torch.isfinite(got).all()):
        failures.append("non-finite output")
    if not ratio <= 1.0:
        err = (got.double() - ref).abs() / (ATOL[row["kernel"]] + 2.0 ** -10 * ref.abs())
        i = tuple(int(v) for v in torch.unravel_index(torch.argmax(err), err.shape))
        failures.append(f"err/tol {ratio:.3f} at [b, c, y, x] = {i}: got {float(got[i]):.6e} ref {float(ref[i]):.6e}; {int((err > 1).sum())} of {err.numel()} elements over")
    if not bool((outside == 0).all()):
        failures.append("channels outside the output view (or the spare image behind the last one) were written")
    if not same:
        failures.append("a second launch differs")
    assert not failures, f"{row['id']}:\n  " + "\n  ".join(failures)


# ---- argument rejection: every call below returns before any launch -----------------------------------------------------------------------
def _rejected(lib, rc, text):
    assert rc != 0
    err = lib.cvmi_last_error().decode()
    assert text in err, err
    assert lib.cvmi_last_kernel().decode() == "", "a rejected call must not reach a launch"


def _row(rid):
    return next(r for r in FUSED_ROWS if r["id"] == rid)


def test_c3k2_rejects_bad_arguments():
    lib = _lib.load()
    for rid in ("c3k2_16_8_64_32_9x17", "c3k2_32_16_64_0_9x17"):
        row, o, _ = row_case(rid)
        plan, _, _, _ = build_plan(row, o)
        d = plan.keep[-1][0]
        lib.cvmi_last_kernel()

        def call(**kw):
            e = _lib.C3k2Desc.from_buffer_copy(d)
            for k, v in kw.items():
                setattr(e, k, v)
            return lib.cvmi_c3k2(C.byref(e), plan.sptr)

        _rejected(lib, call(c2=96), "is not built")
        _rejected(lib, call(h=d.h * 2), "is not built")
        _rejected(lib, call(dtype=F32), "is not built")
        _rejected(lib, call(x_ld=d.x_ld + 4), "bad shape / ld")
        _rejected(lib, call(y_ld=d.c2 - 8), "bad shape / ld")
        _rejected(lib, call(kpad1=9 * d.c - 8), "Kpad too small")
        _rejected(lib, call(kpad3=3 * d.c - 8), "Kpad too small")
        if d.fuse_cv1:
            _rejected(lib, call(w0=None), "fuse_cv1 needs the cv1 weights")
            _rejected(lib, call(kpad0=d.c1 - 8), "Kpad too small")
        else:
            _rejected(lib, call(fuse_cv1=1, c1=64, c2=128), "fuse_cv1 needs the cv1 weights")


def test_stem2_rejects_bad_arguments():
    lib = _lib.load()
    row, o, _ = row_case("stem2_17x33")
    x, w0 = _s2d(o["img"], o["w0"])
    src = _input_buf(x, row)
    yb = Buf(src.B, 9, 17, 32, F16, zero=True)
    pc0, pc1 = PackedConv(w0, o["b0"], F16), PackedConv(o["w1"], o["b1"], F16)
    st = stream()
    lib.cvmi_last_kernel()

    def call(x_ld=src.ld, kpad0=pc0.Kpad, kpad1=pc1.Kpad, c0=16, c1=32, dtype=F16):
        return lib.cvmi_stem2(src.ptr, x_ld, pc0.w.data_ptr(), pc0.bias.data_ptr(), kpad0, pc1.w.data_ptr(), pc1.bias.data_ptr(), kpad1,
                              yb.t.data_ptr(), 32, src.B, src.H, src.W, c0, c1, dtype, st.cuda_stream)

    _rejected(lib, call(c0=64, c1=128), "is not built")
    _rejected(lib, call(dtype=F32), "is not built")
    _rejected(lib, call(x_ld=20), "bad shape / ld")
    _rejected(lib, call(x_ld=8), "bad shape / ld")
    _rejected(lib, call(kpad0=56), "Kpad too small")
    _rejected(lib, call(kpad1=136), "Kpad too small")


def test_dwpw_rejects_bad_arguments():
    lib = _lib.load()
    row, o, _ = row_case("dwpw_c64_n64_cls62")
    plan, _, _, _ = build_plan(row, o)
    d = plan.keep[-1][0]
    lib.cvmi_last_kernel()

    def call(**kw):
        e = _lib.DwPwDesc.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(e, k, v)
        return lib.cvmi_dwpw(C.byref(e), plan.sptr)

    _rejected(lib, call(C=48), "is not built")
    _rejected(lib, call(C=128), "is not built")                             # the chained conv is built for C = 64 and 80 only
    _rejected(lib, call(N1=60), "is not built")
    _rejected(lib, call(dtype=F32), "is not built")
    _rejected(lib, call(x_ld=d.x_ld + 4), "bad shape / ld")
    _rejected(lib, call(y_ld=56), "bad shape / ld")
    _rejected(lib, call(kpad1=56), "Kpad too small")
    _rejected(lib, call(kpad2=56), "Kpad too small")
    _rejected(lib, call(w2=None), "chained conv needs w2 / b2")
