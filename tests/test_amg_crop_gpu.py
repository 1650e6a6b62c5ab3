"""The automatic mask generator's crop layers on the GPU (csrc/mask_amg.hip: cvmi_amg_select_crop, cvmi_amg_score_window; circuitvision_amd/amg.py
with crop_n_layers > 0) against tests/amg_crop_ref.py: the border filter in the ordered append on synthetic rows, the window writer against
cvmi_amg_score's mask mode on the same planes (no precondition: the same f32 value per pixel), and the generator on the mini model against a
host loop over contiguous crop copies and the same public calls."""
import functools

import numpy as np
import pytest
import torch

import amg_crop_ref as cref
import amg_ref as ref
from circuitvision_amd import _lib
from test_amg_crop_ref_cpu import window_rows
from test_amg_gpu import F0, GUARD, IOU_T, P_SEL, R, STAB_T, _Image, _model, _planes, _score, _stats_rows

pytestmark = pytest.mark.gpu
TOL = cref.EDGE_TOL


# ---- the border filter in the ordered append ----------------------------------------------------------------------------------------------------------
class _CropImage(_Image):
    def select_crop(self, stats, iou, low, n_valid, ncand, base, crop, W, H, tol=TOL, check=True):
        lib = _lib.load()
        self.keep = (stats.cuda(), iou.cuda(), low.cuda())
        s, i, l = self.keep
        rc = lib.cvmi_amg_select_crop(s.data_ptr(), i.data_ptr(), l.data_ptr(), s.shape[0], n_valid, ncand, base, IOU_T, STAB_T, P_SEL, self.cap,
                                      self.counter.data_ptr(), self.records.data_ptr(), self.pool.data_ptr(), self.block.data_ptr(), *crop, W, H, tol, None)
        torch.cuda.synchronize()
        if check:
            _lib.check(rc, "amg_select_crop")
        return rc


def _border_chunk(rows, tag):
    """Synthetic stats that pass the score filters, one per row of a border case, with distinct areas and planes."""
    stats = _stats_rows([(20, 20, 100 + k, box) for k, (_, box, _) in enumerate(rows)])
    iou = torch.tensor([0.6 + 0.01 * k for k in range(len(rows))])
    return stats, iou, _planes(tag, len(rows))


def _expected_append(chunks, cap):
    """[(stats, iou, low, kept indices, base)] -> (count, records, pool rows, block): the reference append of the kept candidates in order."""
    recs, rows = [], []
    block = torch.zeros(5, cap)
    block[4] = float("-inf")
    for stats, iou, low, kept, base in chunks:
        stab = ref.stability(stats.numpy())
        for i in kept:
            s = stats[i].tolist()
            block[:, len(recs)] = torch.tensor([(s[3] + s[5]) / 2, (s[4] + s[6]) / 2, s[5] - s[3], s[6] - s[4], float(iou[i])])
            recs.append((float(iou[i]), float(stab[i]), s[2], s[3], s[4], s[5], s[6], base + int(i), 0, 0))
            rows.append(low[i])
    return len(recs), recs, rows, block


@pytest.mark.parametrize("case", cref.BORDER_CASES, ids=lambda c: "crop_%d_%d_%d_%d" % tuple(c[0]))
def test_border_filter_drops_what_a_crop_edge_cuts(case):
    """Each side at distance 20 (dropped) and 21 (kept) from an interior crop edge, a side near the crop's AND the image's edge (kept), the empty
    mask's box, a dropped candidate between two kept ones: the slots are dense, in candidate order, records and block in crop coordinates.  Twice
    on one counter: the second call appends behind the first."""
    crop, (W, H), rows = case
    stats, iou, low = _border_chunk(rows, 1)
    kept = cref.select(stats.numpy(), iou.numpy(), len(rows), IOU_T, STAB_T, crop, H, W).tolist()
    assert kept == [k for k, (_, _, keep) in enumerate(rows) if keep]
    cap = 2 * len(rows)
    runs = []
    for _ in range(2):
        img = _CropImage(cap)
        img.select_crop(stats, iou, low, len(rows), 1, 0, crop, W, H)
        first = _expected_append([(stats, iou, low, kept, 0)], cap)
        img.select_crop(stats, iou, _planes(2, len(rows)), len(rows), 1, 7, crop, W, H)           # the same candidates again, as points 7 ..
        both = _expected_append([(stats, iou, low, kept, 0), (stats, iou, _planes(2, len(rows)), kept, 7)], cap)
        counter, recs, pool, block = img.read()
        n = both[0]
        assert counter == [n, 0] and n == 2 * len(kept) and first[0] == len(kept) and img.guards_intact()
        assert [tuple(r.tolist()) for r in recs[:n]] == [tuple(np.array([r], dtype=_lib.AMG_RECORD)[0].tolist()) for r in both[1]]
        assert torch.equal(pool[:n], torch.stack(both[2])) and torch.equal(block, both[3]) and bool((pool[n:] == -7.0).all())
        runs.append((recs.tobytes(), pool, block))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_border_filter_tolerance_and_score_filters_together():
    """edge_tol is an argument: at 19 the distance-20 rows stay, at 21 the distance-21 rows go; a row that fails the score filters stays out."""
    crop, (W, H), rows = cref.BORDER_CASES[0]
    stats, iou, low = _border_chunk(rows, 3)
    iou[1] = 0.4                                                                 # "left_21" fails pred_iou_thresh
    for tol in (19, 20, 21):
        want = cref.select(stats.numpy(), iou.numpy(), len(rows), IOU_T, STAB_T, crop, H, W, tol).tolist()
        img = _CropImage(16)
        img.select_crop(stats, iou, low, len(rows), 1, 0, crop, W, H, tol)
        counter, recs, _, _ = img.read()
        assert counter == [len(want), 0] and [int(r["point"]) for r in recs[:len(want)]] == want and img.guards_intact(), tol
    assert 1 not in want and len({tuple(cref.select(stats.numpy(), iou.numpy(), len(rows), IOU_T, STAB_T, crop, H, W, t).tolist()) for t in (19, 20, 21)}) == 3


def test_crop_equal_to_the_image_is_amg_select_byte_for_byte():
    from test_amg_gpu import CHUNK1, CHUNK2, IOU1, IOU2
    rows = [r for _, _, rs in cref.BORDER_CASES for r in rs]
    chunks = [(CHUNK1, IOU1, _planes(1, 6), 6, 3, 0), (CHUNK2, IOU2, _planes(2, 6), 3, 3, 2), (*_border_chunk(rows, 3), len(rows), 1, 4)]
    for W, H in ((160, 96), (256, 256)):
        a, b = _CropImage(64), _CropImage(64)
        for c in chunks:
            a.select(*c, IOU_T, STAB_T)
            b.select_crop(*c, [0, 0, W, H], W, H)
        assert a.guards_intact() and b.guards_intact() and a.read()[0] == b.read()[0] and a.read()[0][0] > len(rows)
        for x, y in ((a.counter, b.counter), (a.records, b.records), (a.pool, b.pool), (a.block, b.block)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_select_crop_refuses_a_crop_outside_the_image():
    lib = _lib.load()
    crop, (W, H), rows = cref.BORDER_CASES[0]
    stats, iou, low = _border_chunk(rows, 1)
    img = _CropImage(16)
    for bad in ([64, 32, 161, 96], [64, 32, 160, 97], [-1, 32, 160, 96], [64, -1, 160, 96], [64, 32, 64, 96], [64, 40, 160, 40], [0, 0, 0, 0]):
        assert img.select_crop(stats, iou, low, len(rows), 1, 0, bad, W, H, check=False) != 0, bad
        assert b"amg_select_crop" in lib.cvmi_last_error()
    assert img.select_crop(stats, iou, low, len(rows), 1, 0, crop, W, H, tol=-1, check=False) != 0
    assert img.select_crop(stats, iou, low, len(rows), 1, 0, crop, 0, H, check=False) != 0
    assert img.read()[0] == [0, 0] and img.guards_intact() and bool((img.pool[:16 * P_SEL] == -7.0).all())


# ---- the window writer ------------------------------------------------------------------------------------------------------------------------------------
LV = ref.levels(0.0, 1.0)


def _score_window(low_d, row, fill=-7):
    """cvmi_amg_score_window twice on buffers that start at 7, with a guard band -> (stats i32 [M, 8] on the host, u8 [M, PH, PW] on the device)."""
    lib = _lib.load()
    _, M, h, w, H, W, PH, PW, wx0, wy0 = row
    runs = []
    for _ in range(2):
        stats = torch.full((M * 8 + GUARD,), fill, dtype=torch.int32, device="cuda")
        m = torch.full((M * PH * PW + GUARD,), 7, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cvmi_amg_score_window(low_d.data_ptr(), M, h, w, H, W, LV[0], LV[1], LV[2], stats.data_ptr(), m.data_ptr(), PH, PW, wx0, wy0, None),
                   "amg_score_window")
        torch.cuda.synchronize()
        assert bool((stats[M * 8:] == fill).all()), "stats: wrote past the end"
        assert bool((m[M * PH * PW:] == 7).all()), "mask: wrote past the end"
        runs.append((stats[:M * 8].view(M, 8).cpu(), m[:M * PH * PW].view(M, PH, PW)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    return runs[0]


@pytest.mark.parametrize("row", window_rows(), ids=lambda r: r[0])
def test_window_writer_equals_the_mask_mode_inside_and_zero_outside(row):
    """Random planes, no precondition: inside the window the bytes are cvmi_amg_score's mask mode on the same planes and the stats are its stats
    (crop coordinates); every byte outside is 0 -- none keeps the 7 the buffer started with."""
    _, M, h, w, H, W, PH, PW, wx0, wy0 = row
    low = cref.window_planes(row).cuda()
    want_stats, want_mask = _score(low, H, W, LV, mask=True)
    assert H * W < 64 or 0 < int(want_stats[:, 2].sum()) < M * H * W                                # the level cuts through the planes
    stats, planes = _score_window(low, row)
    assert torch.equal(stats, want_stats), (row[0], (stats - want_stats).abs().amax(0).tolist())
    assert torch.equal(planes[:, wy0:wy0 + H, wx0:wx0 + W], want_mask), row[0]
    outside = planes.clone()
    outside[:, wy0:wy0 + H, wx0:wx0 + W] = 0
    assert int(outside.count_nonzero()) == 0, row[0]
    if (H, W) == (PH, PW):                                                                          # window = plane: cvmi_amg_score bit for bit
        assert torch.equal(planes, want_mask)
    want = torch.stack([cref.uncrop_mask(m, [wx0, wy0, wx0 + W, wy0 + H], PH, PW) for m in want_mask.cpu()])
    assert torch.equal(planes.cpu(), want)


def test_score_window_refuses_bad_arguments():
    lib = _lib.load()
    low = torch.zeros(2, 8, 8, device="cuda")
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    m = torch.full((2 * 20 * 24 + GUARD,), 7, dtype=torch.uint8, device="cuda")
    call = lambda **k: lib.cvmi_amg_score_window(k.get("low", low.data_ptr()), k.get("M", 2), 8, 8, k.get("H", 10), k.get("W", 12), -1.0, 0.0, 1.0,
                                                 k.get("stats", s.data_ptr()), k.get("mask", m.data_ptr()), k.get("PH", 20), k.get("PW", 24), k.get("wx0", 3),
                                                 k.get("wy0", 4), None)
    for bad in (dict(wx0=-1), dict(wy0=-1), dict(wx0=13), dict(wy0=11), dict(PW=11), dict(PH=9), dict(H=0), dict(W=0), dict(PH=0)):
        assert call(**bad) != 0, bad
        assert b"amg_score_window" in lib.cvmi_last_error()
    for bad in (dict(mask=None), dict(low=None), dict(stats=None), dict(M=0), dict(M=65536), dict(PH=1 << 16, PW=1 << 15)):
        assert call(**bad) != 0, bad
        assert b"amg_score_window" in lib.cvmi_last_error()
    torch.cuda.synchronize()
    assert int(s.abs().sum()) == 0 and bool((m == 7).all())
    assert call(wx0=12, wy0=10) == 0                                                                # right- and bottom-flush is inside
    torch.cuda.synchronize()
    assert bool((m[2 * 20 * 24:] == 7).all()) and not bool((m[:2 * 20 * 24] == 7).any())


# ---- end to end on the mini model ------------------------------------------------------------------------------------------------------------------------
# (H, W, seed) of the u8 image, tried in this order until the reference side meets its four conditions (below).  On an MI355X the mini model's
# masks are large: at 256 x 256 (and 192 x 256, 128 x 128, 320 x 320, with noise and with blocks of 16, 32 and 64 pixels) the border filter cuts
# every candidate of at least three of the four layer-1 crops, so the result never holds two of them; (96, 160, 11) is the first image that
# meets all four, in both dtypes.  CHOSEN records that pick and the NMS thresholds found with it; the test asserts them, so a change is seen.
CANDIDATES = ((256, 256, 11), (96, 160, 11))
CHOSEN = {"f32": ((96, 160, 11), 0.7, 0.3), "f16": ((96, 160, 11), 0.7, 0.3)}
PPS, PPB = 4, 6
NMS_THRESHOLDS = (0.7, 0.5, 0.3, 0.1)


def _image(H, W, seed):
    """A u8 image of 32 x 32 blocks of uniform colour: a crop sees other block borders than the whole image."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(3, (H + 31) // 32, (W + 31) // 32, generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W]
    return (c * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def _decode_crops(dtype, img, n_layers, downscale):
    """The host loop up to the maps: contiguous crop copies through SAM2Transforms.forward_batch, ONE encode in crop order, infer_masks per chunk for
    the crops of a layer together, cvmi_bilinear_f32 maps at each crop's size.  -> the `crops` list amg_crop_ref.generate_crops_ref takes."""
    from circuitvision_amd.sam2_infer import SAM2Transforms
    lib, model = _lib.load(), _model(dtype)
    H, W = img.shape[:2]
    boxes, layers = cref.crop_boxes(H, W, n_layers)
    grids = cref.layer_grids(PPS, n_layers, downscale)
    x = SAM2Transforms(R, 0.0).forward_batch([np.ascontiguousarray(img[y0:y1, x0:x1]) for x0, y0, x1, y1 in boxes])
    emb = model.encode_images(x)
    crops = []
    for layer in range(n_layers + 1):
        idx = [c for c, l in enumerate(layers) if l == layer]
        grid = grids[layer]
        pts_in = torch.from_numpy(grid.astype(np.float32)) * float(R)
        lows, ious = [], []
        for base in range(0, len(grid), PPB):
            pts = pts_in[base:base + PPB]
            if pts.shape[0] < PPB:
                pts = torch.cat([pts, pts[-1:].expand(PPB - pts.shape[0], 2)])
            _, low, iou = model.infer_masks(emb[idx[0]:idx[-1] + 1], points=pts.view(1, PPB, 1, 2).expand(len(idx), PPB, 1, 2),
                                            point_labels=torch.ones(len(idx), PPB, 1, dtype=torch.int32), multimask_output=True, return_high_res=False)
            lows.append(low)
            ious.append(iou)
        low, iou = torch.cat(lows, 1).contiguous(), torch.cat(ious, 1).cpu()                 # [n, Np, 3, 64, 64], [n, Np, 3]; points >= len(grid) are padding
        for k, c in enumerate(idx):
            x0, y0, x1, y1 = boxes[c]
            n = low.shape[1] * 3
            m = torch.empty(n, y1 - y0, x1 - x0, device="cuda")
            _lib.check(lib.cvmi_bilinear_f32(low[k].data_ptr(), n, F0, F0, m.data_ptr(), y1 - y0, x1 - x0, None, 0.0, None), "bilinear")
            torch.cuda.synchronize()
            crops.append(dict(box=boxes[c], iou=iou[k].numpy(), maps=m.cpu(), grid=grid, n_points=len(grid), stats=ref.score_planes(m.cpu(), *LV)))
    return crops


def _conditions(info):
    per = info["per_crop"]
    return (any(p["cut"] > 0 and p["passed"] - p["cut"] > 0 for p in per[1:5]), sum(p["suppressed"] for p in per) > 0, info["cross_suppressed"] > 0,
            0 in info["crops_in_result"] and len([c for c in info["crops_in_result"] if 1 <= c <= 4]) >= 2)


@functools.lru_cache(None)
def _crop_host_loop(dtype):
    """The reference side with one crop layer.  Thresholds: the medians of the reference's own predicted IoUs and stabilities over the valid
    candidates of all crops; the two NMS thresholds the first of NMS_THRESHOLDS with which the per-crop NMS, resp. the NMS across the crops,
    suppresses something.  The image is the first of CANDIDATES for which the four conditions hold:
      the border filter drops at least one and keeps at least one candidate of an interior (layer-1) crop; the per-crop NMS suppresses at
      least one; the NMS across the crops suppresses at least one; the result holds masks of layer 0 and of at least two layer-1 crops.
    -> (image, thresholds dict, want dicts)."""
    lv = ref.levels(0.0, 1.0)
    tried = []
    for H, W, seed in CANDIDATES:
        img = _image(H, W, seed)
        crops = _decode_crops(dtype, img, 1, 1)
        valid_iou = np.concatenate([c["iou"].reshape(-1)[:c["n_points"] * 3] for c in crops])
        valid_stab = np.concatenate([ref.stability(c["stats"].numpy())[:c["n_points"] * 3] for c in crops])
        t = dict(pred_iou_thresh=float(np.median(valid_iou)), stability_score_thresh=float(np.nanmedian(valid_stab)), lv=lv)
        for box_t in NMS_THRESHOLDS:
            for crop_t in NMS_THRESHOLDS:
                info = {}
                want = cref.generate_crops_ref(crops, H, W, box_nms_thresh=box_t, crop_nms_thresh=crop_t, info=info, **t)
                tried.append(((H, W, seed), box_t, crop_t, _conditions(info)))
                if all(_conditions(info)):
                    print(f"[amg crops {dtype}] image {(H, W, seed)}, iou median {t['pred_iou_thresh']:.6f}, stability median {t['stability_score_thresh']:.6f}, "
                          f"box_nms_thresh {box_t}, crop_nms_thresh {crop_t}, per crop {info['per_crop']}, across the crops suppressed "
                          f"{info['cross_suppressed']}, result from crops {info['crops_in_result']}, {len(want)} masks")
                    assert CHOSEN[dtype] in (None, ((H, W, seed), box_t, crop_t)), (CHOSEN[dtype], (H, W, seed), box_t, crop_t)
                    return img, dict(t, box_nms_thresh=box_t, crop_nms_thresh=crop_t), want
    raise AssertionError(f"no candidate image meets the four conditions: {tried}")


def _crop_generator(dtype, **kw):
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    _, t, _ = _crop_host_loop(dtype)
    args = dict(points_per_side=PPS, points_per_batch=PPB, pred_iou_thresh=t["pred_iou_thresh"], stability_score_thresh=t["stability_score_thresh"],
                box_nms_thresh=t["box_nms_thresh"])
    args.update(kw)
    return Sam2AutomaticMaskGenerator(_model(dtype), **args)


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_generator_with_one_crop_layer_equals_the_host_loop(dtype):
    img, t, want = _crop_host_loop(dtype)
    H, W = img.shape[:2]
    gen = _crop_generator(dtype)
    got = gen.generate(img, crop_n_layers=1, crop_nms_thresh=t["crop_nms_thresh"])
    torch.cuda.synchronize()
    assert ref.same_dicts(got, want), (dtype, len(got), len(want), [d["crop_box"] for d in got], [d["crop_box"] for d in want])
    for d in got:
        assert d["segmentation"].is_cuda and d["segmentation"].dtype == torch.uint8 and tuple(d["segmentation"].shape) == (H, W)
        assert d["area"] == int((d["segmentation"] != 0).sum())
        cx0, cy0, cw, ch = d["crop_box"]
        outside = d["segmentation"].clone()
        outside[cy0:cy0 + ch, cx0:cx0 + cw] = 0
        assert int(outside.count_nonzero()) == 0
    again = gen.generate_batch([img, img], crop_n_layers=1, crop_nms_thresh=t["crop_nms_thresh"])                      # each image on its own; the plans replay
    assert len(again) == 2 and all(ref.same_dicts(a, want) for a in again)
    # crop_n_layers = 0 given explicitly is the call without the argument
    assert ref.same_dicts(gen.generate(img, crop_n_layers=0, crop_nms_thresh=0.1), gen.generate(img))


@pytest.mark.parametrize("dtype", ("f32",))
def test_two_crop_layers_downscaled_grids_and_sub_batches(dtype, monkeypatch):
    """21 crops with grids of 4, 2 and 1 points per side equal the reference; with the pool budget lowered so that the crops split into three or more
    sub-batches (layer groups cut at sub-batch borders) the call equals the unsplit one."""
    from circuitvision_amd import amg
    img, t, _ = _crop_host_loop(dtype)
    H, W = img.shape[:2]
    crops = _decode_crops(dtype, img, 2, 2)
    assert [c["n_points"] for c in crops] == [16] + [4] * 4 + [1] * 16
    want = cref.generate_crops_ref(crops, H, W, **t)
    gen = _crop_generator(dtype)
    kw = dict(crop_n_layers=2, crop_n_points_downscale_factor=2, crop_nms_thresh=t["crop_nms_thresh"])
    got = gen.generate(img, **kw)
    assert ref.same_dicts(got, want) and len(got) > 0, (len(got), len(want))
    full = cref.generate_crops_ref(_decode_crops(dtype, img, 2, 1), H, W, **t)                        # the same 21 crops with the 4 x 4 grid in every layer
    got_full = gen.generate(img, crop_n_layers=2, crop_nms_thresh=t["crop_nms_thresh"])
    print(f"[amg crops {dtype}] two layers: {len(got)} masks from crops {sorted({tuple(d['crop_box']) for d in got})} with grids 4, 2, 1; "
          f"{len(got_full)} from {sorted({tuple(d['crop_box']) for d in got_full})} with grids 4, 4, 4")
    assert ref.same_dicts(got_full, full) and len(got_full) > 0, (len(got_full), len(full))
    monkeypatch.setattr(amg, "POOL_BYTES_IN_FLIGHT", 8 * gen.cap * F0 * F0 * 4)                     # 8 crops per sub-batch: 8 + 8 + 5
    split = gen.generate(img, **kw)
    assert ref.same_dicts(split, got)


def test_crops_compose_with_the_per_call_options():
    from circuitvision_amd import amg_utils
    img, t, _ = _crop_host_loop("f32")
    gen = _crop_generator("f32")
    kw = dict(crop_n_layers=1, crop_nms_thresh=t["crop_nms_thresh"])
    plain = gen.generate(img, **kw)
    rle = gen.generate(img, output_mode="uncompressed_rle", **kw)
    assert len(rle) == len(plain) > 0
    for r, p in zip(rle, plain):
        assert tuple(r) == ref.KEYS and np.array_equal(amg_utils.rle_to_mask(r["segmentation"]), p["segmentation"].cpu().numpy() != 0)
        assert r["area"] == p["area"] and all(r[k] == p[k] for k in ref.KEYS[2:])
    small = gen.generate(img, min_mask_region_area=8, **kw)
    post = amg_utils.postprocess_small_regions(plain, 8, max(t["box_nms_thresh"], t["crop_nms_thresh"]))
    assert ref.same_dicts(small, post) and len(small) > 0


def test_crops_refuse_inputs_without_pixels():
    gen = _crop_generator("f32")
    img, _, _ = _crop_host_loop("f32")
    from circuitvision_amd.sam2_infer import SAM2Transforms
    x = SAM2Transforms(R, 0.0)(img)[None]
    with pytest.raises(ValueError, match="list of RGB u8 images"):
        gen.generate_batch(x, orig_hw=[img.shape[:2]], crop_n_layers=1)
    with pytest.raises(ValueError, match="list of RGB u8 images"):
        gen.generate_batch(_model("f32").encode_images(x), orig_hw=[img.shape[:2]], crop_n_layers=1)
    with pytest.raises(RuntimeError, match="max_candidates"):
        _crop_generator("f32", max_candidates=1).generate(img, crop_n_layers=1)
