"""The bits of the resampling kernels (csrc/resample.hip), three ways:

* against the commit before the family moved into one file: tests/resample_bits_fixture.json holds the SHA-256 of every non-refused transform case
  of the resampling matrix and of cvmi_bilinear_f32 / cvmi_mask_postprocess on two shapes, recorded from that commit's library
  (tests/resample_bits_cases.py).  Equality is the bar; an operand whose own hash is off fails the test, it does not skip it.
* the four forms of the mask return against each other: at thresholds the f32 map itself takes, the u8 masks of cvmi_bilinear_f32,
  cvmi_mask_postprocess, _sizes and _rects_dev are equal byte for byte and equal to (map > t), and the three extent tables are equal.  An equality
  between forms: no tolerance is involved.
* a window against a contiguous copy of it: `rects`, `rects_dev` and `srcs` on a window == `batch` on the copy, bit for bit, in every output type
  and for both swap_rb values."""
import json
import os

import numpy as np
import pytest
import torch

from circuitvision_amd import _lib
from helper_ref import CODE, TDT
from resample_bits_cases import (MASK_SHAPES, N_THRESHOLDS, mask_hashes, mask_id, mask_operand, sha, transform_hashes, transform_operand_hash,
                                 transform_rows)

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample_bits_fixture.json")) as f:
    FIXTURE = json.load(f)


def _compare(got, want, what):
    assert sorted(got) == sorted(want), f"{what}: the cases changed: {sorted(set(got) ^ set(want))}"
    off = sorted(k for k in want if got[k] != want[k])
    assert not off, f"{what}: {len(off)} of {len(want)} outputs differ from the recorded bits: {off}"


@pytest.mark.parametrize("row", transform_rows(), ids=lambda r: r["id"])
def test_transform_bits_are_the_recorded_ones(row):
    rec = FIXTURE["transform"][row["id"]]
    assert transform_operand_hash(row) == rec["operand"], "the seeded source images are not the recorded ones on this host"
    _compare(transform_hashes(_lib.load(), row), rec["out"], row["id"])


def test_every_recorded_transform_row_is_still_run():
    assert sorted(FIXTURE["transform"]) == sorted(r["id"] for r in transform_rows())


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=mask_id)
def test_bilinear_and_mask_postprocess_bits_are_the_recorded_ones(shape):
    rec = FIXTURE["mask"][mask_id(shape)]
    assert sha(mask_operand(*shape[:3])) == rec["operand"], "the seeded planes are not the recorded ones on this host"
    _compare(mask_hashes(_lib.load(), shape), rec["out"], mask_id(shape))


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=mask_id)
def test_four_forms_of_the_mask_return_give_one_answer(shape):
    lib = _lib.load()
    N, h, w, H, W = shape
    low = mask_operand(N, h, w).cuda()
    ymap = torch.empty(N, H, W, dtype=torch.float32, device="cuda")
    assert lib.cvmi_bilinear_f32(low.data_ptr(), N, h, w, ymap.data_ptr(), H, W, None, 0.0, None) == 0
    flat = ymap.view(-1)
    step = flat.numel() // N_THRESHOLDS
    thresholds = flat[step // 2::step][:N_THRESHOLDS].cpu().tolist()               # fixed strided positions: every threshold is a value the map takes
    assert len(thresholds) == N_THRESHOLDS
    stride = H * W + 5                                                             # rects_dev: a stride a little larger than the plane
    sizes = np.ascontiguousarray(np.array([[H, W]] * N, dtype=np.int32))
    win = torch.tensor([[2, 3, W, H]] * N, dtype=torch.int32).cuda()
    y2 = torch.empty_like(ymap)
    masks = {k: torch.empty(N, H * W, dtype=torch.uint8, device="cuda") for k in ("bilinear_f32", "mask_postprocess", "mask_postprocess_sizes")}
    masks["mask_postprocess_rects_dev"] = torch.empty(N, stride, dtype=torch.uint8, device="cuda")
    exts = {k: torch.empty(N, 4, dtype=torch.int32, device="cuda") for k in list(masks)[1:]}
    failures = []
    for i, t in enumerate(thresholds):
        for m in masks.values():
            m.fill_(7)
        rcs = (lib.cvmi_bilinear_f32(low.data_ptr(), N, h, w, y2.data_ptr(), H, W, masks["bilinear_f32"].data_ptr(), t, None),
               lib.cvmi_mask_postprocess(low.data_ptr(), N, h, w, H, W, t, masks["mask_postprocess"].data_ptr(), exts["mask_postprocess"].data_ptr(), None),
               lib.cvmi_mask_postprocess_sizes(low.data_ptr(), N, h, w, sizes.ctypes.data, t, masks["mask_postprocess_sizes"].data_ptr(),
                                               exts["mask_postprocess_sizes"].data_ptr(), None),
               lib.cvmi_mask_postprocess_rects_dev(low.data_ptr(), N, h, w, win.data_ptr(), stride, t, masks["mask_postprocess_rects_dev"].data_ptr(),
                                                   exts["mask_postprocess_rects_dev"].data_ptr(), None))
        assert rcs == (0, 0, 0, 0), lib.cvmi_last_error().decode()
        want = ((ymap > t).view(N, H * W).to(torch.uint8) * 255)
        if not torch.equal(y2, ymap):
            failures.append(f"threshold {i} ({t!r}): cvmi_bilinear_f32's map depends on the threshold")
        for k, m in masks.items():
            bad = int((m[:, :H * W] != want).sum())
            if bad:
                failures.append(f"threshold {i} ({t!r}): {bad} of {N * H * W} bytes of {k}'s mask differ from (map > t)")
        e0 = exts["mask_postprocess"]
        for k in ("mask_postprocess_sizes", "mask_postprocess_rects_dev"):
            if not torch.equal(exts[k], e0):
                failures.append(f"threshold {i} ({t!r}): the extents of {k} {exts[k].tolist()} differ from cvmi_mask_postprocess's {e0.tolist()}")
    print(f"RESAMPLE-BITS {mask_id(shape)}: {N_THRESHOLDS} thresholds from the map, {len(failures)} disagreements")
    assert not failures, f"{len(failures)} disagreements:\n  " + "\n  ".join(failures[:12])


WIN_IMAGE, WINDOW = (40, 56), (7, 5, 33, 21)                                       # H, W of the image; x0, y0, w, h: interior, odd offsets and sizes


@pytest.mark.parametrize("dt", ("f16", "bf16", "f32"))
@pytest.mark.parametrize("R", (16, 40))                                            # both axes down (33 x 21 -> 16); both up (-> 40)
def test_a_window_is_transformed_like_a_contiguous_copy_of_it(R, dt):
    lib = _lib.load()
    (H, W), (x0, y0, w, h) = WIN_IMAGE, WINDOW
    img = np.random.RandomState(7).randint(0, 256, size=(H, W, 3), dtype=np.uint8)
    src = torch.from_numpy(img).cuda()
    crop = torch.from_numpy(np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])).cuda()
    packed = torch.cat([torch.full((3,), 0x55, dtype=torch.uint8), torch.from_numpy(img).view(-1)]).cuda()      # the image at an odd byte offset
    rects = np.ascontiguousarray(np.array([[x0, y0, w, h]], dtype=np.int32))
    rects_dev = torch.from_numpy(rects).cuda()
    rows = np.zeros(1, dtype=_lib.SAM2_SRC_ROW)
    rows[0] = (3, H, W, x0, y0, w, h)
    new = lambda: torch.full((R, R, 3), -3.0, dtype=TDT[dt], device="cuda")
    failures = []
    for swap in (0, 1):
        want, got = new(), {k: new() for k in ("rects", "rects_dev", "srcs")}
        rcs = (lib.cvmi_sam2_transform_batch(crop.data_ptr(), 1, h, w, want.data_ptr(), R, CODE[dt], swap, None),
               lib.cvmi_sam2_transform_rects(src.data_ptr(), H * W * 3, H, W, rects.ctypes.data, 1, got["rects"].data_ptr(), R, CODE[dt], swap, None),
               lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), H * W * 3, H, W, rects_dev.data_ptr(), 1, got["rects_dev"].data_ptr(), R, CODE[dt], swap, None),
               lib.cvmi_sam2_transform_srcs(packed.data_ptr(), packed.numel(), rows.ctypes.data, 1, got["srcs"].data_ptr(), R, CODE[dt], swap, None))
        assert rcs == (0, 0, 0, 0), lib.cvmi_last_error().decode()
        torch.cuda.synchronize()
        assert bool((want.float() != -3.0).any())
        for k, g in got.items():
            bad = int((g.view(torch.uint8) != want.view(torch.uint8)).sum())
            if bad:
                failures.append(f"swap_rb {swap}: {k} differs from batch on the copy in {bad} bytes")
    assert not failures, "\n".join(failures)
