"""The resampling matrix (tests/op_matrix.py RESAMPLE_ROWS): the five forms of cvmi_sam2_transform* in every output type, and the four forms of the
bilinear mask return with cvmi_mask_extent, each called directly through the C ABI and compared with the references of tests/resample_ref.py:
|y - ref64| <= ATOL[family] + RTOL[stored type] |ref64| for the transform's outputs and the f32 map (ATOL measured on the CPU, never from a
kernel), bit for bit for the u8 masks and their extents.  tests/test_resample_ref_cpu.py proves on the CPU that these comparisons catch the classic
mistakes and that no mask element has to be excused.

Every output starts as a sentinel with guard elements before and after it that must survive, every launch runs twice on restored buffers and must
repeat bit for bit, and a refused call must leave every output element untouched and reach no launch."""
import time

import numpy as np
import pytest
import torch

from circuitvision_amd import _lib
from helper_ref import CODE, SENTINEL, TDT, rT
from op_matrix import RECT_MAX, RESAMPLE_GRID_CAP, RESAMPLE_ROWS
from resample_ref import extent_planes, mask_expected, mask_operands, mask_planes, mask_sizes, tf_images, tf_reference, tol_ratio
from test_helper_matrix_gpu import GUARD, _full, _twice

pytestmark = pytest.mark.gpu
ESIZE = {"f16": 2, "bf16": 2, "f32": 4}
MASK_FILL, EXT_FILL = 7, -7                            # what a u8 mask / an extent holds before a launch


def _refused(lib, rc, text, outs):
    """A refused call: the error text, no launch, and every element of every output (guards included) as it was."""
    torch.cuda.synchronize()
    fails = []
    if rc == 0:
        fails.append("the call was accepted")
    else:
        err = lib.cvmi_last_error().decode()
        if text not in err:
            fails.append(f"error {err!r}, expected {text!r}")
    if lib.cvmi_last_kernel().decode() != "":
        fails.append("a refused call reached a tagged launch")
    for name, t, fill in outs:
        left = int((t.float() != fill).sum())
        if left:
            fails.append(f"{left} of {t.numel()} elements of {name} were written by the refused call")
    return fails


# ---- the transform ------------------------------------------------------------------------------------------------------------------------------------
def _pack_srcs(row, imgs):
    """One u8 buffer holding every image at an ODD byte offset (filler bytes between them) and the row table of cvmi_sam2_transform_srcs."""
    offs, pos = [], 1
    for im in imgs:
        pos += 1 - pos % 2
        offs.append(pos)
        pos += im.size
    buf = np.full(pos + 3, 0x55, dtype=np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    tab = np.zeros(len(row["items"]), dtype=_lib.SAM2_SRC_ROW)
    for b, (k, x0, y0, w, h) in enumerate(row["items"]):
        tab[b] = (offs[k], imgs[k].shape[0], imgs[k].shape[1], x0, y0, w, h)
    assert all(o % 2 == 1 for o in offs)
    return torch.from_numpy(buf).cuda(), tab


def _transform_call(lib, row, form, dt, swap, dst_ptr):
    """(call, what must stay alive) of one launch of the row through `form`."""
    imgs = tf_images(row["id"])
    R, n = row["R"], len(row["items"])
    H, W = row["images"][0]
    if form in ("single", "batch"):
        src = torch.from_numpy(np.stack(imgs)).cuda()
        if form == "single":
            assert swap == 0 and n == 1
            return (lambda: lib.cvmi_sam2_transform(src.data_ptr(), H, W, dst_ptr, R, CODE[dt], None)), (src,)
        return (lambda: lib.cvmi_sam2_transform_batch(src.data_ptr(), n, H, W, dst_ptr, R, CODE[dt], swap, None)), (src,)
    if form in ("rects", "rects_dev"):
        src = torch.from_numpy(np.stack(imgs)).cuda()
        stride = 0 if row["stride0"] else H * W * 3
        rects = np.ascontiguousarray(np.array([it[1:] for it in row["items"]], dtype=np.int32))
        if form == "rects":
            return (lambda: lib.cvmi_sam2_transform_rects(src.data_ptr(), stride, H, W, rects.ctypes.data, n, dst_ptr, R, CODE[dt], swap, None)), (src, rects)
        dev = torch.from_numpy(rects).cuda()
        return (lambda: lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), stride, H, W, dev.data_ptr(), n, dst_ptr, R, CODE[dt], swap, None)), (src, dev)
    assert form == "srcs", form
    buf, tab = _pack_srcs(row, imgs)
    return (lambda: lib.cvmi_sam2_transform_srcs(buf.data_ptr(), buf.numel(), tab.ctypes.data, n, dst_ptr, R, CODE[dt], swap, None)), (buf, tab)


TF_CASES = [(r, f, dt) for r in RESAMPLE_ROWS if r["op"] == "transform" for f in r["forms"] for dt in r["dtypes"]]
MASK_CASES = [(r, f) for r in RESAMPLE_ROWS if r["op"] != "transform" for f in r["forms"]]


@pytest.mark.parametrize("row,form,dt", TF_CASES, ids=["%s-%s-%s" % (r["id"], f, dt) for r, f, dt in TF_CASES])
def test_transform_matrix(row, form, dt):
    lib = _lib.load()
    t0 = time.time()
    rid, R, n = row["id"], row["R"], len(row["items"])
    per = R * R * 3
    cap = RESAMPLE_GRID_CAP["transform"]                                        # pixels of one grid pass
    assert ("second_pass" in row["tags"]) == (R * R > cap)
    dst = _full((GUARD + n * per + GUARD,), dt)
    dst_ptr = dst.data_ptr() + GUARD * ESIZE[dt]
    failures = []
    for swap in ((0,) if form == "single" else row["swaps"]):
        call, keep = _transform_call(lib, row, form, dt, swap, dst_ptr)
        if form in row["refuse"]:
            torch.cuda.synchronize()
            lib.cvmi_last_kernel()
            failures += _refused(lib, call(), row["refuse"][form], [("the output", dst, SENTINEL)])
            print(f"RESAMPLE-MATRIX {rid} {form} {dt} swap {swap}: refused  {time.time() - t0:.1f} s")
            continue
        _, (first,), same = _twice(lib, call, [dst], reset=lambda: dst.fill_(SENTINEL))
        dst.fill_(SENTINEL)
        got = first[GUARD:GUARD + n * per].view(n, R * R, 3)
        ref = rT(tf_reference(rid, swap), dt).view(n, R * R, 3)
        ratio, mx = tol_ratio(got, ref, "aa_transform", dt)
        line = f"RESAMPLE-MATRIX {rid} {form} {dt} swap {swap}: max|err| {mx:.3e}  err/bound {ratio:.3f}"
        if not ratio <= 1.0:
            worst = (got.double() - ref).abs().amax((1, 2))
            failures.append(f"swap {swap}: err/bound {ratio:.3f} (max|err| {mx:.3e}); per item max|err| {[f'{v:.2e}' for v in worst.tolist()[:8]]}, worst item {int(worst.argmax())}")
        if R * R > cap:                                                        # the pixels only the second pass of the grid-stride loop writes
            r2, m2 = tol_ratio(got[:, cap:], ref[:, cap:], "aa_transform", dt)
            line += f"  pixels >= {cap} (second pass): max|err| {m2:.3e}  err/bound {r2:.3f}"
            if not r2 <= 1.0:
                failures.append(f"swap {swap}: the {R * R - cap} pixels >= 1024^2 of each image, which the second grid pass writes: err/bound {r2:.3f}")
        if n > RECT_MAX:                                                       # the outputs of the second 64-entry table
            r3, _ = tol_ratio(got[RECT_MAX:], ref[RECT_MAX:], "aa_transform", dt)
            line += f"  items >= {RECT_MAX}: err/bound {r3:.3f}"
            if not r3 <= 1.0:
                failures.append(f"swap {swap}: outputs {RECT_MAX}.. (the second table): err/bound {r3:.3f}")
        print(line + f"  {time.time() - t0:.1f} s")
        if not bool((first[:GUARD].float() == SENTINEL).all() and (first[GUARD + n * per:].float() == SENTINEL).all()):
            failures.append(f"swap {swap}: guard elements around the output were written")
        if not same:
            failures.append(f"swap {swap}: a second launch differs")
        del keep
    assert not failures, f"{rid} {form} {dt}:\n  " + "\n  ".join(failures)


# ---- the mask return -----------------------------------------------------------------------------------------------------------------------------------
def _mask_launch(lib, row, form, thresh):
    """One threshold of one mask-return row through `form`: (failures, log line).  Planes lie back to back (or one per plane_stride for rects_dev)
    inside a buffer of MASK_FILL with guards; extents inside a table of EXT_FILL with a guard row before and after."""
    rid = row["id"]
    low = mask_operands(rid).cuda()
    N, h, w = low.shape
    sizes = mask_sizes(row)
    refs = mask_planes(rid)
    stride = row["plane_stride"] if row["op"] == "mask_rects_dev" else (row["H"] * row["W"] + 5 if form == "mask_postprocess_rects_dev" else None)
    offs, pos = [], 0
    for n, s in enumerate(sizes):
        offs.append(n * stride if stride else pos)
        pos += s[0] * s[1] if s else 0
    total = N * stride if stride else pos
    mask = torch.full((GUARD + total + GUARD,), MASK_FILL, dtype=torch.uint8, device="cuda")
    ext = torch.full((N + 2, 4), EXT_FILL, dtype=torch.int32, device="cuda")
    mptr, eptr = mask.data_ptr() + GUARD, ext.data_ptr() + 16
    outs, ymap = [mask, ext], None
    if form == "bilinear_f32":
        ymap = _full((GUARD + total + GUARD,), "f32")
        call = lambda: lib.cvmi_bilinear_f32(low.data_ptr(), N, h, w, ymap.data_ptr() + 4 * GUARD, row["H"], row["W"], mptr, thresh, None)
        outs = [mask, ext, ymap]
    elif form == "mask_postprocess":
        call = lambda: lib.cvmi_mask_postprocess(low.data_ptr(), N, h, w, row["H"], row["W"], thresh, mptr, eptr, None)
    elif form == "mask_postprocess_sizes":
        tab = np.ascontiguousarray(np.array(row["sizes"] if row["op"] == "mask_sizes" else sizes, dtype=np.int32))
        call = lambda: lib.cvmi_mask_postprocess_sizes(low.data_ptr(), N, h, w, tab.ctypes.data, thresh, mptr, eptr, None)
    else:
        assert form == "mask_postprocess_rects_dev", form
        wins = row["windows"] if row["op"] == "mask_rects_dev" else [(3, 4, row["W"], row["H"])] * N
        dev = torch.tensor(wins, dtype=torch.int32).cuda()
        call = lambda: lib.cvmi_mask_postprocess_rects_dev(low.data_ptr(), N, h, w, dev.data_ptr(), stride, thresh, mptr, eptr, None)
    if row.get("refuse"):
        torch.cuda.synchronize()
        lib.cvmi_last_kernel()
        return _refused(lib, call(), row["refuse"], [("the mask", mask, MASK_FILL), ("the extents", ext, EXT_FILL)]), "refused"

    def reset():
        mask.fill_(MASK_FILL)
        ext.fill_(EXT_FILL)
        if ymap is not None:
            ymap.fill_(SENTINEL)

    _, first, same = _twice(lib, call, outs, reset=reset)
    m, e = first[0], first[1]
    fails, info = [], "exact"
    written = torch.zeros(total, dtype=torch.bool)
    bad = 0
    want_ext = []
    for n, s in enumerate(sizes):
        wm, we = mask_expected(refs[n], thresh)
        want_ext.append(we[0])
        k = s[0] * s[1]
        written[offs[n]:offs[n] + k] = True
        bad += int((m[GUARD + offs[n]:GUARD + offs[n] + k] != wm.reshape(-1)).sum())    # no reference value lies within the bound of a threshold (CPU test)
    if bad:
        fails.append(f"{bad} of {int(written.sum())} mask elements differ")
    body = m[GUARD:GUARD + total]
    if not bool((m[:GUARD] == MASK_FILL).all() and (m[GUARD + total:] == MASK_FILL).all() and (body[~written] == MASK_FILL).all()):
        fails.append("mask bytes outside the planes (guards, or the rest of a plane's stride) were written")
    if form == "bilinear_f32":
        if not bool((e == EXT_FILL).all()):
            fails.append("cvmi_bilinear_f32 wrote an extent")
        y = first[2]
        ratio, mx = tol_ratio(y[GUARD:GUARD + total].view(N, row["H"], row["W"]), torch.cat(refs), "bilinear_edge", "f32")
        info = f"max|err| {mx:.3e}  err/bound {ratio:.3f}"
        if not ratio <= 1.0:
            fails.append(f"err/bound {ratio:.3f}")
        if not bool((y[:GUARD] == SENTINEL).all() and (y[GUARD + total:] == SENTINEL).all()):
            fails.append("elements around the f32 map were written")
    else:
        want_ext = torch.stack(want_ext)
        if not torch.equal(e[1:N + 1], want_ext):
            diff = [(n, e[1 + n].tolist(), want_ext[n].tolist()) for n in range(N) if not torch.equal(e[1 + n], want_ext[n])]
            fails.append(f"{len(diff)} extents differ: (plane, got, expected) {diff[:4]}")
        if not bool((e[0] == EXT_FILL).all() and (e[N + 1] == EXT_FILL).all()):
            fails.append("rows around the extent table were written")
    if not same:
        fails.append("a second launch differs")
    return fails, info


def _extent_launch(lib, row):
    planes = extent_planes(row)
    N, H, W = planes.shape
    m = planes.cuda()
    ext = torch.full((N + 2, 4), EXT_FILL, dtype=torch.int32, device="cuda")
    _, (e,), same = _twice(lib, lambda: lib.cvmi_mask_extent(m.data_ptr(), N, H, W, ext.data_ptr() + 16, None), [ext], reset=lambda: ext.fill_(EXT_FILL))
    want = mask_expected(planes.double(), 0.5)[1]
    fails = [] if torch.equal(e[1:N + 1], want) else [f"extent {e[1:N + 1].tolist()}, expected {want.tolist()}"]
    if not bool((e[0] == EXT_FILL).all() and (e[N + 1] == EXT_FILL).all()):
        fails.append("rows around the extent table were written")
    if not torch.equal(m.cpu(), planes):
        fails.append("the input mask was modified")
    if not same:
        fails.append("a second launch differs")
    return fails, "exact"


@pytest.mark.parametrize("row,form", MASK_CASES, ids=["%s-%s" % (r["id"], f) for r, f in MASK_CASES])
def test_mask_return_matrix(row, form):
    lib = _lib.load()
    t0 = time.time()
    failures = []
    if row["op"] == "extent":
        failures, info = _extent_launch(lib, row)
        print(f"RESAMPLE-MATRIX {row['id']} {form}: {info}  {time.time() - t0:.1f} s")
    else:
        for thresh in row["thresholds"]:
            fails, info = _mask_launch(lib, row, form, thresh)
            failures += [f"threshold {thresh}: {f}" for f in fails]
            print(f"RESAMPLE-MATRIX {row['id']} {form} threshold {thresh}: {info}  {time.time() - t0:.1f} s")
    assert not failures, f"{row['id']} {form}:\n  " + "\n  ".join(failures)
