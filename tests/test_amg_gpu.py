"""The automatic mask generator on the GPU (csrc/mask_amg.hip: cvmi_amg_score, cvmi_amg_select; circuitvision_amd/amg.py) against tests/amg_ref.py:
the scorer's counts and boxes vs the fp64 resize (rows whose every pixel is clear of every level: test_amg_ref_cpu.py) and vs the map
cvmi_bilinear_f32 writes (no precondition: the same f32 value per pixel), its mask mode vs cvmi_mask_postprocess, the ordered append, NMS through
the packed block vs torchvision's, and the generator on the mini model vs the host loop over the same public calls."""
import functools

import numpy as np
import pytest
import torch

import amg_ref as ref
from circuitvision_amd import _lib
from test_amg_ref_cpu import scorer_rows

pytestmark = pytest.mark.gpu
GUARD = 512                                      # sentinel elements behind every output
R, F0 = 256, 64
SIZES = [(96, 160), (256, 256)]


def _score(low_d, H, W, lv, mask=False, fill=-7):
    """cvmi_amg_score twice on pre-filled outputs with a guard band -> (stats i32 [M, 8] on the host, u8 [M, H, W] device tensor or None)."""
    lib = _lib.load()
    M, h, w = low_d.shape
    runs = []
    for _ in range(2):
        stats = torch.full((M * 8 + GUARD,), fill, dtype=torch.int32, device="cuda")
        m = torch.full((M * H * W + GUARD,), 7, dtype=torch.uint8, device="cuda") if mask else None
        _lib.check(lib.cvmi_amg_score(low_d.data_ptr(), M, h, w, H, W, lv[0], lv[1], lv[2], stats.data_ptr(), m.data_ptr() if mask else None, None), "amg_score")
        torch.cuda.synchronize()
        assert bool((stats[M * 8:] == fill).all()), "stats: wrote past the end"
        assert m is None or bool((m[M * H * W:] == 7).all()), "mask: wrote past the end"
        runs.append((stats[:M * 8].view(M, 8).cpu(), m[:M * H * W].view(M, H, W) if mask else None))
    assert torch.equal(runs[0][0], runs[1][0]) and (not mask or torch.equal(runs[0][1], runs[1][1])), "two runs differ"
    return runs[0]


# ---- the scorer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ref.LEVEL_PAIRS, ids=lambda p: "thr%g_off%g" % p)
@pytest.mark.parametrize("row", scorer_rows(), ids=lambda r: r[0])
def test_score_equals_the_fp64_reference(row, pair):
    """Every pixel of the fp64 resize is clear of every level (asserted on the CPU), so the counts and the box are decided: exact equality."""
    M, H, W = row[1], row[4], row[5]
    lv = ref.levels(*pair)
    want = ref.score_planes(ref.scorer_reference(row), *lv)
    got, _ = _score(ref.scorer_planes(row).cuda(), H, W, lv)
    assert torch.equal(got.long(), want), (row[0], (got.long() - want).abs().amax(0).tolist())


RANDOM_SHAPES = ((7, 16, 16, 61, 77), (3, 64, 64, 256, 256), (2, 64, 64, 96, 160), (4, 8, 8, 1030, 9), (2, 40, 24, 21, 2050), (3, 12, 10, 5, 3))


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "%dx%dx%d_to_%dx%d" % s)
def test_score_equals_the_counts_of_the_map_bilinear_f32_writes(shape):
    """Random planes, values anywhere (no precondition): the scorer's sample is cvmi_bilinear_f32's f32 value, so the counts and extents of the
    map that entry point writes are the scorer's, exactly -- with and without the mask."""
    lib = _lib.load()
    M, h, w, H, W = shape
    g = torch.Generator().manual_seed(1234 + M * H + W)
    low = (torch.randn(M, h, w, generator=g) * 1.5).cuda()
    ymap = torch.empty(M, H, W, device="cuda")
    _lib.check(lib.cvmi_bilinear_f32(low.data_ptr(), M, h, w, ymap.data_ptr(), H, W, None, 0.0, None), "bilinear")
    torch.cuda.synchronize()
    ymap = ymap.cpu()
    for pair in ref.LEVEL_PAIRS + ((0.1, 0.3),):
        lv = ref.levels(*pair)
        want = ref.score_planes(ymap, *lv)
        assert 0 < int(want[:, 2].sum()) and int(want[:, 0].sum()) < M * H * W               # the levels cut through the planes
        got, _ = _score(low, H, W, lv)
        assert torch.equal(got.long(), want), (shape, pair, (got.long() - want).abs().amax(0).tolist())
        got_m, mask = _score(low, H, W, lv, mask=True)
        assert torch.equal(got_m, got)
        assert torch.equal(mask.cpu(), (ymap > lv[1]).to(torch.uint8) * 255)


MASK_SHAPES = ((3, 16, 16, 64, 64), (5, 16, 12, 67, 131), (2, 16, 16, 9, 7), (2, 64, 64, 96, 160), (1, 8, 8, 1, 1))


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "%dx%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("thresh", (0.0, 0.5))
def test_mask_mode_equals_mask_postprocess(shape, thresh):
    """The u8 planes and the extents are cvmi_mask_postprocess's bit for bit (W a multiple of 4: one 4-byte store per thread; otherwise bytes);
    an empty plane's box is {0, 0, 0, 0} here and {W, H, -1, -1} there.  stats is the score-only call's."""
    lib = _lib.load()
    M, h, w, H, W = shape
    g = torch.Generator().manual_seed(77 + H)
    low = torch.randn(M, h, w, generator=g) * 2
    low[0] = -3.0 - low[0].abs()                                                            # plane 0: empty at both thresholds
    low = low.cuda()
    u8 = torch.empty(M, H, W, dtype=torch.uint8, device="cuda")
    ext = torch.empty(M, 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_mask_postprocess(low.data_ptr(), M, h, w, H, W, thresh, u8.data_ptr(), ext.data_ptr(), None), "mask_postprocess")
    torch.cuda.synchronize()
    lv = ref.levels(thresh, 1.0)
    stats, mask = _score(low, H, W, lv, mask=True)
    plain, _ = _score(low, H, W, lv)
    assert torch.equal(stats, plain)
    assert torch.equal(mask, u8)
    ext = ext.cpu()
    assert ext[0].tolist() == [W, H, -1, -1] and stats[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    assert torch.equal(stats[1:, 3:7], ext[1:]) or M == 1
    assert torch.equal(stats[:, 2].long(), (u8 != 0).sum((1, 2)).cpu())


def test_score_refuses_bad_arguments():
    lib = _lib.load()
    t = torch.zeros(4096, device="cuda")
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert lib.cvmi_amg_score(None, 1, 8, 8, 8, 8, -1.0, 0.0, 1.0, s.data_ptr(), None, None) != 0
    assert lib.cvmi_amg_score(t.data_ptr(), 0, 8, 8, 8, 8, -1.0, 0.0, 1.0, s.data_ptr(), None, None) != 0
    assert lib.cvmi_amg_score(t.data_ptr(), 65536, 8, 8, 8, 8, -1.0, 0.0, 1.0, s.data_ptr(), None, None) != 0
    assert lib.cvmi_amg_score(t.data_ptr(), 1, 8, 8, 0, 8, -1.0, 0.0, 1.0, s.data_ptr(), None, None) != 0
    assert lib.cvmi_amg_score(t.data_ptr(), 1, 8, 8, 8, 8, -1.0, 0.0, 1.0, None, None, None) != 0
    assert b"amg_score" in lib.cvmi_last_error()
    assert lib.cvmi_amg_score(t.data_ptr(), 1, 1, 1 << 20, 1, 4, -1.0, 0.0, 1.0, s.data_ptr(), None, None) != 0       # one output row needs 2^20 staged floats
    assert b"staging buffer" in lib.cvmi_last_error()
    torch.cuda.synchronize()
    assert int(s.abs().sum()) == 0


# ---- the ordered append ---------------------------------------------------------------------------------------------------------------------
P_SEL = 24                                       # floats per plane in the select tests (a multiple of 4)
NREC = len(_lib.AMG_RECORD)


def _stats_rows(rows):
    return torch.tensor([[hi, lo, area, x0, y0, x1, y1, 0] for hi, lo, area, (x0, y0, x1, y1) in rows], dtype=torch.int32)


class _Image:
    """One image's select state with a guard band behind every buffer."""

    def __init__(self, cap, fill=-7.0):
        self.cap = cap
        self.counter = torch.zeros(2 + GUARD, dtype=torch.int32, device="cuda")
        self.counter[2:] = -7
        self.records = torch.full((cap * NREC + GUARD,), -7, dtype=torch.int32, device="cuda")
        self.pool = torch.full((cap * P_SEL + GUARD,), fill, device="cuda")
        self.block = torch.full((5 * cap + GUARD,), fill, device="cuda")
        self.block[:5 * cap].view(5, cap).zero_()
        self.block[4 * cap:5 * cap] = float("-inf")

    def select(self, stats, iou, low, n_valid, ncand, base, iou_t, stab_t):
        lib = _lib.load()
        self.keep = (stats.cuda(), iou.cuda(), low.cuda())
        s, i, l = self.keep
        _lib.check(lib.cvmi_amg_select(s.data_ptr(), i.data_ptr(), l.data_ptr(), s.shape[0], n_valid, ncand, base, iou_t, stab_t, P_SEL, self.cap,
                                       self.counter.data_ptr(), self.records.data_ptr(), self.pool.data_ptr(), self.block.data_ptr(), None), "amg_select")
        torch.cuda.synchronize()

    def guards_intact(self):
        cap = self.cap
        return (bool((self.counter[2:] == -7).all()) and bool((self.records[cap * NREC:] == -7).all()) and bool((self.pool[cap * P_SEL:] == -7.0).all())
                and bool((self.block[5 * cap:] == -7.0).all()))

    def read(self):
        cap = self.cap
        recs = self.records[:cap * NREC].cpu().numpy().view(_lib.AMG_RECORD).reshape(cap)
        return self.counter[:2].tolist(), recs, self.pool[:cap * P_SEL].view(cap, P_SEL).cpu(), self.block[:5 * cap].view(5, cap).cpu()


BOX = (2, 3, 9, 7)
CHUNK1 = _stats_rows([(19, 20, 30, BOX), (0, 0, 0, (0, 0, 0, 0)), (20, 20, 31, BOX), (20, 20, 32, (1, 1, 4, 8)), (18, 20, 33, BOX), (20, 20, 34, (5, 5, 5, 5))])
IOU1 = torch.tensor([0.9, 0.9, 0.5, 0.7, 0.9, 0.6])                     # plane 1: NaN stability; 2: iou == thresh; 4: 18 / 20 < 0.95
CHUNK2 = _stats_rows([(20, 20, 40, BOX), (20, 20, 41, BOX), (20, 20, 42, (0, 0, 11, 12)), (20, 20, 43, BOX), (20, 20, 44, BOX), (20, 20, 45, BOX)])
IOU2 = torch.tensor([0.8, 0.4, 0.95, 0.99, 0.99, 0.99])                 # planes 3..5 are padding: they would pass
IOU_T, STAB_T = 0.5, 0.95                                                # plane 0 of chunk 1: f32(19) / f32(20) == f32(0.95), kept by >=


def _planes(tag, n):
    return (torch.arange(n * P_SEL, dtype=torch.float32).view(n, P_SEL) + 1000.0 * tag)


def _expected(chunks, cap):
    """Reference append of [(stats, iou, low, n_valid, ncand, base)] -> (count, [(record fields...)], pool rows, block)."""
    recs, rows = [], []
    block = torch.zeros(5, cap)
    block[4] = float("-inf")
    count = 0
    for stats, iou, low, n_valid, ncand, base in chunks:
        kept = ref.select(stats.numpy(), iou.numpy(), n_valid, IOU_T, STAB_T)
        stab = ref.stability(stats.numpy())
        for i in kept:
            if count < cap:
                s = stats[i].tolist()
                recs.append((float(iou[i]), float(stab[i]), s[2], s[3], s[4], s[5], s[6], base + int(i) // ncand, int(i) % ncand, 0))
                rows.append(low[i])
                x0, y0, x1, y1 = (float(v) for v in s[3:7])
                block[:, count] = torch.tensor([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, float(iou[i])])
            count += 1
    return count, recs, rows, block


def test_select_appends_two_chunks_in_candidate_order():
    cap = 8
    img = _Image(cap)
    chunks = [(CHUNK1, IOU1, _planes(1, 6), 6, 3, 0), (CHUNK2, IOU2, _planes(2, 6), 3, 3, 2)]
    want_n = 0
    for k, c in enumerate(chunks):
        img.select(*c, IOU_T, STAB_T)
        want_n, recs, rows, block = _expected(chunks[:k + 1], cap)
        counter, got_recs, pool, got_block = img.read()
        assert counter == [want_n, 0] and img.guards_intact()
        assert [tuple(r.tolist()) for r in got_recs[:want_n]] == [tuple(np.array([r], dtype=_lib.AMG_RECORD)[0].tolist()) for r in recs]
        assert torch.equal(pool[:want_n], torch.stack(rows))
        assert torch.equal(got_block, block)
        assert bool((got_block[4, want_n:] == float("-inf")).all()) and bool((got_block[:4, want_n:] == 0).all())    # the unused columns remain
        assert bool((pool[want_n:] == -7.0).all())
    assert want_n == 5
    _, recs, _, _ = img.read()
    assert [int(r["point"]) for r in recs[:5]] == [0, 1, 1, 2, 2] and [int(r["token"]) for r in recs[:5]] == [0, 0, 2, 0, 2]
    assert float(recs[0]["stability"]) == float(np.float32(19) / np.float32(20))


def test_select_counts_past_cap_and_writes_nothing_there():
    cap = 2
    img = _Image(cap)
    chunk = (CHUNK1, IOU1, _planes(1, 6), 6, 3, 0)
    img.select(*chunk, IOU_T, STAB_T)
    want_n, recs, rows, block = _expected([chunk], cap)
    counter, got_recs, pool, got_block = img.read()
    assert want_n == 3 and counter == [3, 0] and img.guards_intact()
    assert [tuple(r.tolist()) for r in got_recs] == [tuple(np.array([r], dtype=_lib.AMG_RECORD)[0].tolist()) for r in recs]
    assert torch.equal(pool, torch.stack(rows)) and torch.equal(got_block, block)
    img.select(*chunk, IOU_T, STAB_T)                                                       # full: the count goes on, nothing moves
    counter2, got_recs2, pool2, got_block2 = img.read()
    assert counter2 == [6, 0] and img.guards_intact()
    assert got_recs2.tobytes() == got_recs.tobytes() and torch.equal(pool2, pool) and torch.equal(got_block2, got_block)


def test_select_with_no_valid_plane_or_bad_arguments():
    lib = _lib.load()
    img = _Image(4)
    img.select(CHUNK1, IOU1, _planes(1, 6), 0, 3, 0, IOU_T, STAB_T)
    counter, _, pool, _ = img.read()
    assert counter == [0, 0] and bool((pool == -7.0).all()) and img.guards_intact()
    s, i, l = img.keep
    args = lambda **kw: [kw.get("s", s.data_ptr()), i.data_ptr(), l.data_ptr(), 6, kw.get("n_valid", 6), 3, 0, IOU_T, STAB_T, kw.get("P", P_SEL), kw.get("cap", 4),
                         img.counter.data_ptr(), img.records.data_ptr(), img.pool.data_ptr(), img.block.data_ptr(), None]
    assert lib.cvmi_amg_select(*args(s=None)) != 0 and lib.cvmi_amg_select(*args(n_valid=7)) != 0 and lib.cvmi_amg_select(*args(P=6)) != 0
    assert lib.cvmi_amg_select(*args(cap=0)) != 0 and b"amg_select" in lib.cvmi_last_error()
    torch.cuda.synchronize()
    assert img.read()[0] == [0, 0]


# ---- NMS through the packed block ---------------------------------------------------------------------------------------------------------------
NMS_BOXES = [(0, 0, 10, 10), (0, 0, 10, 5), (0, 0, 10, 6), (3, 3, 3, 3), (3, 3, 3, 3), (20, 20, 30, 30), (20, 20, 30, 30), (21, 21, 30, 30), (0, 0, 40, 40),
             (100, 7, 163, 95), (101, 8, 164, 96), (1000, 2000, 3001, 2047)]
NMS_SCORES = [0.9, 0.8, 0.8, 0.85, 0.85, 0.7, 0.7, 0.95, 0.6, 0.75, 0.75, 0.65]


@pytest.mark.parametrize("thresh", (0.5, 0.7, 0.1))
def test_nms_through_the_packed_block_is_torchvision_nms(thresh):
    """Integer boxes with equal scores, two one-pixel boxes (area 0) and a pair whose IoU is exactly 0.5: cvmi_amg_select packs them, cvmi_yolo_nms
    (nc = 1, A = cap) keeps what oracle.nms.torchvision_nms keeps, in its order."""
    lib = _lib.load()
    n, cap = len(NMS_BOXES), 16
    stats = _stats_rows([(20, 20, 1, b) for b in NMS_BOXES])
    iou = torch.tensor(NMS_SCORES)
    img = _Image(cap)
    img.select(stats, iou, _planes(3, n), n, 1, 0, 0.5, 0.95)
    assert img.read()[0] == [n, 0]
    want = ref.nms(NMS_BOXES, NMS_SCORES, thresh).tolist()
    assert ref.nms([NMS_BOXES[0], NMS_BOXES[1]], [0.9, 0.8], 0.5).tolist() == [0, 1]      # IoU exactly 0.5 at threshold 0.5: kept
    ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(1, cap)), dtype=torch.uint8, device="cuda")
    det = torch.empty(cap, 6, device="cuda")
    idx = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_yolo_nms(img.block.data_ptr(), 1, 1, cap, 0.5, thresh, cap, 0.0, det.data_ptr(), idx.data_ptr(), cnt.data_ptr(), ws.data_ptr(), None), "yolo_nms")
    torch.cuda.synchronize()
    k = int(cnt[0])
    assert idx[:k].tolist() == want, (thresh, idx[:k].tolist(), want)
    assert torch.equal(det[:k, :4].cpu(), torch.tensor([NMS_BOXES[i] for i in want], dtype=torch.float32))             # cx - w / 2 gives the corner back


# ---- the generator on the mini model ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _model(dtype):
    from circuitvision_amd.sam2_infer import SAM2Model
    from test_mask_prompt_gpu import _params
    from test_oracle_sam2_cpu import MINI
    return SAM2Model(MINI, R, dtype=dtype, use_refinement=True).load_params(_params())


@functools.lru_cache(None)
def _images():
    return torch.randn(2, 3, R, R, generator=torch.Generator().manual_seed(31))


@functools.lru_cache(None)
def _host_loop(dtype):
    """The reference side: infer_masks per chunk from one embedding, cvmi_bilinear_f32 maps, amg_ref on the CPU; the thresholds are chosen here,
    from its own values.  -> (emb, thresholds, [dicts per image], the same with box_nms_thresh = 1: nothing suppressed)."""
    lib, model = _lib.load(), _model(dtype)
    grid = ref.point_grid(4)
    pts_in = torch.from_numpy(grid.astype(np.float32)) * float(R)
    emb = model.encode_images(_images())
    lows, ious = [], []
    for base in (0, 6, 12):
        pts = pts_in[base:base + 6]
        if pts.shape[0] < 6:
            pts = torch.cat([pts, pts[-1:].expand(6 - pts.shape[0], 2)])
        _, low, iou = model.infer_masks(emb, points=pts.view(1, 6, 1, 2).expand(2, 6, 1, 2), point_labels=torch.ones(2, 6, 1, dtype=torch.int32),
                                        multimask_output=True, return_high_res=False)
        lows.append(low)
        ious.append(iou)
    low, iou = torch.cat(lows, 1).contiguous(), torch.cat(ious, 1).cpu()                   # [2, 18, 3, 64, 64], [2, 18, 3]: points 16, 17 are padding
    lv = ref.levels(0.0, 1.0)
    maps, stats = [], []
    for b, (H, W) in enumerate(SIZES):
        m = torch.empty(54, H, W, device="cuda")
        _lib.check(lib.cvmi_bilinear_f32(low[b].data_ptr(), 54, F0, F0, m.data_ptr(), H, W, None, 0.0, None), "bilinear")
        torch.cuda.synchronize()
        maps.append(m.cpu())
        stats.append(ref.score_planes(maps[-1], *lv))
    valid_iou = np.concatenate([iou[b].reshape(-1)[:48].numpy() for b in range(2)])
    valid_stab = np.concatenate([ref.stability(stats[b].numpy())[:48] for b in range(2)])
    iou_t, stab_t = float(np.median(valid_iou)), float(np.nanmedian(valid_stab))
    run = lambda nms_t: [ref.generate_ref(low[b].cpu(), iou[b].numpy(), maps[b], grid, 16, H, W, iou_t, stab_t, lv, nms_t) for b, (H, W) in enumerate(SIZES)]
    no_nms = run(2.0)
    nms_t = next((t for t in (0.7, 0.5, 0.3, 0.1) if sum(map(len, run(t))) < sum(map(len, no_nms))), None)
    print(f"[amg {dtype}] iou median {iou_t:.6f} (range {valid_iou.min():.4f} .. {valid_iou.max():.4f}), stability median {stab_t:.6f}, "
          f"kept by the filter {[len(d) for d in no_nms]} of 48, box_nms_thresh {nms_t}, after NMS {[len(d) for d in run(nms_t)] if nms_t else None}")
    assert nms_t is not None, "NMS drops no candidate at any of the thresholds"
    assert 0 < sum(map(len, no_nms)) < 96                                                  # the filter keeps some but not all
    return emb, (iou_t, stab_t, nms_t), run(nms_t), run(1.0)


def _generator(dtype, **kw):
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    _, (iou_t, stab_t, nms_t), _, _ = _host_loop(dtype)
    args = dict(points_per_side=4, points_per_batch=6, pred_iou_thresh=iou_t, stability_score_thresh=stab_t, box_nms_thresh=nms_t)
    args.update(kw)
    return Sam2AutomaticMaskGenerator(_model(dtype), **args)


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_generator_equals_the_host_loop(dtype):
    """B = 2 at (96, 160) and (256, 256), a 4 x 4 grid in chunks of 6, 6, 4 (the last one padded): the dicts equal the host loop's key for key and
    bit for bit, from images and from embeddings, on a first call and on a replay of the cached plans."""
    emb, _, want, want_all = _host_loop(dtype)
    gen = _generator(dtype)
    got = gen.generate_batch(_images(), orig_hw=SIZES)
    torch.cuda.synchronize()
    for b in range(2):
        assert ref.same_dicts(got[b], want[b]), (dtype, b, len(got[b]), len(want[b]))
        for d in got[b]:
            assert d["segmentation"].is_cuda and d["segmentation"].dtype == torch.uint8 and tuple(d["segmentation"].shape) == SIZES[b]
            assert d["area"] == int((d["segmentation"] != 0).sum())
        assert [d["predicted_iou"] for d in got[b]] == sorted((d["predicted_iou"] for d in got[b]), reverse=True)
    again = gen.generate_batch(emb, orig_hw=SIZES)                                          # embeddings the caller holds; the plans replay
    torch.cuda.synchronize()
    assert all(ref.same_dicts(again[b], want[b]) for b in range(2))
    every = _generator(dtype, box_nms_thresh=1.0).generate_batch(emb, orig_hw=SIZES)      # no IoU exceeds 1: every kept candidate comes back, in score order
    torch.cuda.synchronize()
    assert sum(map(len, want_all)) > sum(map(len, want))
    assert all(ref.same_dicts(every[b], want_all[b]) for b in range(2)), [(len(e), len(w)) for e, w in zip(every, want_all)]


def test_generate_takes_one_u8_image():
    """`generate` on an RGB u8 image = SAM2Transforms + encode_images + generate_batch on the same image."""
    from circuitvision_amd.sam2_infer import SAM2Transforms
    gen = _generator("f32")
    img = torch.randint(0, 256, (96, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).numpy()
    got = gen.generate(img)
    x = SAM2Transforms(R, 0.0)(img)[None]
    want = gen.generate_batch(x, orig_hw=[(96, 160)])[0]
    assert ref.same_dicts(got, want)
    single = _generator("f32", multimask_output=False).generate_batch(x, orig_hw=[(96, 160)])[0]       # the single-mask plan: one candidate per point
    assert all(d["area"] == int((d["segmentation"] != 0).sum()) for d in single)


def test_generator_error_paths():
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    model = _model("f32")
    for kw in (dict(crop_n_layers=1), dict(min_mask_region_area=10), dict(use_m2m=True), dict(output_mode="uncompressed_rle"), dict(output_mode="coco_rle")):
        with pytest.raises(NotImplementedError):
            Sam2AutomaticMaskGenerator(model, **kw)
    emb, _, want, _ = _host_loop("f32")
    assert max(len(w) for w in want) > 0
    with pytest.raises(RuntimeError, match="max_candidates"):
        _generator("f32", max_candidates=1).generate_batch(emb, orig_hw=SIZES)
    with pytest.raises(ValueError, match="orig_hw"):
        _generator("f32").generate_batch(emb, orig_hw=SIZES[:1])
    with pytest.raises(ValueError, match="orig_hw"):
        _generator("f32").generate_batch(emb)
