"""Host side of mixed-size batches (no GPU): the table the ragged letterbox reads is ultralytics' LetterBox(auto=False) geometry per image on one
imgsz x imgsz canvas, the packed layout is monotone and non-overlapping, `PackedImages` slices are views of the same buffer, and the two C ABI
entry points are declared, bound and exported with matching table rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd.detector import YOLO, PackedImages, letterbox_rows, pack_layout
from oracle import preprocess as opre

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sources of the GPU test: one-row / one-column, padding-only tiles, general cases, up-scaling
SHAPES = [(1, 50), (50, 1), (37, 1000), (1000, 37), (64, 64), (300, 200), (493, 712)]


@pytest.mark.parametrize("imgsz", [32, 64, 160, 640])
def test_table_rows_are_the_oracle_geometry_on_a_square_canvas(imgsz):
    shapes = SHAPES + [(imgsz, imgsz)]
    offsets, total = pack_layout(shapes)
    rows = letterbox_rows(shapes, offsets, imgsz)
    assert rows.dtype.itemsize == ctypes.sizeof(_lib.LetterboxRow) == 32 and len(rows) == len(shapes)
    for r, (h, w), off in zip(rows, shapes, offsets):
        nw, nh, top, bottom, left, right = opre.letterbox_geometry(h, w, imgsz, auto=False)
        assert (int(r["src_byte_offset"]), int(r["H"]), int(r["W"])) == (off, h, w)
        assert (int(r["new_w"]), int(r["new_h"]), int(r["top"]), int(r["left"])) == (nw, nh, top, left), (h, w)
        assert nh + top + bottom == imgsz and nw + left + right == imgsz, "every image gets the full imgsz x imgsz canvas"
        assert r["new_h"] >= 1 and r["new_w"] >= 1 and r["top"] + r["new_h"] <= imgsz and r["left"] + r["new_w"] <= imgsz
    ident = rows[-1]
    assert (ident["new_h"], ident["new_w"], ident["top"], ident["left"]) == (imgsz, imgsz, 0, 0)


def test_packed_layout_is_monotone_and_non_overlapping():
    offsets, total = pack_layout(SHAPES)
    assert offsets[0] == 0
    for (h, w), a, b in zip(SHAPES, offsets, offsets[1:] + [total]):
        assert b - a == h * w * 3 > 0
    assert total == sum(h * w * 3 for h, w in SHAPES)
    assert any(o % 2 for o in pack_layout([(3, 3), (5, 5), (2, 2)])[0]), "no alignment is added: odd offsets occur"
    with pytest.raises(ValueError):
        pack_layout([(4, 0)])


def test_packed_images_views_and_slices_share_the_buffer():
    g = np.random.default_rng(0)
    images = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(3, 5), (7, 2), (1, 9), (4, 4)]]
    host = torch.empty(sum(im.size for im in images) + 5, dtype=torch.uint8)
    offsets, total = PackedImages.stage(images, host)
    assert total == host.numel() - 5
    p = PackedImages(host, offsets, [im.shape[:2] for im in images])
    assert len(p) == 4 and p.shapes == [(3, 5), (7, 2), (1, 9), (4, 4)]
    for b, im in enumerate(images):
        assert p.image(b).shape == im.shape and np.array_equal(p.image(b).numpy(), im)
    s = p[1:3]
    assert len(s) == 2 and s.data.data_ptr() == p.data.data_ptr() and s.offsets == p.offsets[1:3] and s.shapes == p.shapes[1:3]
    for b in range(2):
        assert s.image(b).data_ptr() == p.image(1 + b).data_ptr() and torch.equal(s.image(b), p.image(1 + b))
    s.image(0)[0, 0, 0] = 255 - int(images[1][0, 0, 0])                  # a view: the parent sees the write
    assert int(p.image(1)[0, 0, 0]) == 255 - int(images[1][0, 0, 0])
    assert len(p[2:][1:]) == 1 and p[2:][1:].offsets == [p.offsets[3]]
    with pytest.raises(TypeError):
        p[0]
    with pytest.raises(ValueError):
        PackedImages(host, [host.numel() - 10], [(2, 2)])               # leaves the buffer
    with pytest.raises(ValueError):
        PackedImages.stage(images, torch.empty(10, dtype=torch.uint8))


def test_rect_rule_is_ultralytics():
    a, b = np.zeros((4, 6, 3), np.uint8), np.zeros((6, 4, 3), np.uint8)
    assert YOLO._square([a, a], None) is False and YOLO._square([a, a], True) is False      # same shapes and rect: the rectangle
    assert YOLO._square([a, a], False) is True                                                # forced square: one plan whatever arrives
    assert YOLO._square([a, b], None) is True and YOLO._square([a, b], True) is True          # mixed: always the square
    assert YOLO._square([a], None) is False


def test_entry_points_are_declared_bound_and_rows_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name, mirror, rec in (("cvmi_letterbox_ragged", _lib.LetterboxRow, _lib.LETTERBOX_ROW), ("cvmi_sam2_transform_srcs", _lib.Sam2SrcRow, _lib.SAM2_SRC_ROW)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        struct = {"cvmi_letterbox_ragged": "cvmi_letterbox_row", "cvmi_sam2_transform_srcs": "cvmi_sam2_src_row"}[name]
        body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
        fields = [n.strip() for decl_ in re.findall(r"(?:long long|int)\s+([^;]+);", body) for n in decl_.split(",")]
        assert fields == [n for n, _ in mirror._fields_] == [n for n, _ in rec], name
        assert np.dtype(rec).itemsize == ctypes.sizeof(mirror) == 32
