"""Mask RLE and small-region removal on the GPU (csrc/mask_rle.hip: cvmi_mask_rle; csrc/mask_cc.hip: cvmi_mask_remove_small;
circuitvision_amd/amg_utils.py; the per-call arguments of circuitvision_amd/amg.py) against tests/amg_post_ref.py (numpy / scipy).  All
outputs are integers: every comparison is exact.  Every kernel case runs twice into pre-filled outputs with guard bands behind them, and
the two runs must be equal."""
import functools

import numpy as np
import pytest
import torch

import amg_post_ref as ref
import amg_ref
from circuitvision_amd import _lib, amg_utils

pytestmark = pytest.mark.gpu
GUARD = 512                                      # sentinel elements behind every output
RLE_ROWS = dict(ref.rle_rows())
REMOVE_ROWS = {r[0]: r for r in ref.remove_rows()}


# ---- cvmi_mask_rle --------------------------------------------------------------------------------------------------------------------------------
def _rle(mask_d, cap, null_counts=False):
    """cvmi_mask_rle twice -> (offsets int64 [N + 1], counts int64 [cap]) on the host; guards checked, the two runs equal."""
    lib = _lib.load()
    N, H, W = mask_d.shape
    nbytes = int(lib.cvmi_mask_rle_workspace(N, H, W))
    assert nbytes > 0
    runs = []
    for fill in (-7, -9):
        offsets = torch.full((N + 1 + GUARD,), fill, dtype=torch.int32, device="cuda")
        counts = torch.full((cap + GUARD,), fill, dtype=torch.int32, device="cuda")
        ws = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cvmi_mask_rle(mask_d.data_ptr(), N, H, W, cap, offsets.data_ptr(), None if null_counts else counts.data_ptr(), ws.data_ptr(), nbytes, None), "mask_rle")
        torch.cuda.synchronize()
        assert bool((offsets[N + 1:] == fill).all()), "offsets: wrote past the end"
        assert bool((counts[cap:] == fill).all()), "counts: wrote at or past cap_runs"
        assert bool((ws[nbytes:] == 0x5A).all()), "workspace: wrote past the end"
        total = int(offsets[N])
        assert bool((counts[min(total, cap):cap] == fill).all())
        runs.append((offsets[:N + 1].cpu().numpy().astype(np.int64), counts[:min(total, cap)].cpu().numpy().astype(np.int64)))
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"
    return runs[0]


@pytest.mark.parametrize("rid", sorted(RLE_ROWS))
def test_rle_equals_the_reference_at_three_capacities(rid):
    """Capacity exact, one short, and 0 with counts = NULL: offsets equal in all three, the counts a prefix, nothing written past the capacity."""
    planes = RLE_ROWS[rid]
    want_off, want = ref.stack_rle(planes)
    total = int(want_off[-1])
    mask = torch.tensor(planes).cuda()
    off, counts = _rle(mask, total)
    assert np.array_equal(off, want_off), (rid, off.tolist()[:8], want_off.tolist()[:8])
    assert np.array_equal(counts, want), rid
    off1, counts1 = _rle(mask, total - 1)
    assert np.array_equal(off1, want_off) and np.array_equal(counts1, want[:-1])
    off0, counts0 = _rle(mask, 0, null_counts=True)
    assert np.array_equal(off0, want_off) and counts0.size == 0
    offg, countsg = _rle(mask, total + 100)                                    # a generous capacity: the slack stays untouched (checked in _rle)
    assert np.array_equal(offg, want_off) and np.array_equal(countsg, want)


def test_rle_known_answers_and_run_counts():
    off, counts = _rle(torch.tensor(RLE_ROWS["known_2x2"]).cuda(), 16)
    assert off.tolist() == [0, 2, 5] and counts.tolist() == [1, 3, 0, 1, 3]
    off, counts = _rle(torch.tensor(RLE_ROWS["alternating_clear_first"]).cuda(), 80)
    assert off.tolist() == [0, 64] and counts.tolist() == [1] * 64
    off, counts = _rle(torch.tensor(RLE_ROWS["alternating_set_first"]).cuda(), 80)
    assert off.tolist() == [0, 65] and counts.tolist() == [0] + [1] * 64
    off, counts = _rle(torch.tensor(RLE_ROWS["column_pairs"]).cuda(), 16)
    assert counts.tolist() == [14, 2, 14, 14, 1, 15]
    off, counts = _rle(torch.tensor(RLE_ROWS["all_set_5x3"]).cuda(), 4)
    assert counts.tolist() == [0, 15]


def test_rle_reads_bytes_where_the_planes_are_not_word_aligned():
    """W % 4 == 0 takes the 4-byte loads only from an aligned base: the same planes one byte into a buffer take the byte path, same runs."""
    planes = RLE_ROWS["random_64x64_d0.5"]
    want_off, want = ref.stack_rle(planes)
    buf = torch.zeros(planes.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.tensor(planes).cuda().reshape(-1)
    shifted = buf[1:].view(planes.shape)
    assert shifted.data_ptr() % 4 == 1
    off, counts = _rle(shifted, int(want_off[-1]))
    assert np.array_equal(off, want_off) and np.array_equal(counts, want)


def test_rle_refuses_bad_arguments():
    lib = _lib.load()
    m = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    args = lambda **kw: [kw.get("m", m.data_ptr()), kw.get("N", 1), kw.get("H", 8), kw.get("W", 8), kw.get("cap", 64), kw.get("off", off.data_ptr()),
                         kw.get("cnt", cnt.data_ptr()), kw.get("ws", ws.data_ptr()), kw.get("nbytes", 4096), None]
    assert lib.cvmi_mask_rle(*args()) == 0
    for bad in (dict(m=None), dict(off=None), dict(ws=None), dict(cnt=None), dict(N=0), dict(H=0), dict(W=-1), dict(cap=-1), dict(N=1 << 15, H=1 << 8, W=1 << 8),
                dict(nbytes=int(lib.cvmi_mask_rle_workspace(1, 8, 8)) - 1), dict(ws=ws.data_ptr() + 4)):
        assert lib.cvmi_mask_rle(*args(**bad)) != 0, bad
        assert b"mask_rle" in lib.cvmi_last_error()
    assert lib.cvmi_mask_rle(*args(cnt=None, cap=0)) == 0                       # the pure count
    assert lib.cvmi_mask_rle_workspace(1 << 15, 1 << 8, 1 << 8) == 0 and lib.cvmi_mask_rle_workspace(0, 8, 8) == 0 and lib.cvmi_mask_rle_workspace(1, 8, 8) > 0
    torch.cuda.synchronize()
    assert off[:2].tolist() == [0, 1] and int(cnt[0]) == 64


# ---- cvmi_mask_remove_small -------------------------------------------------------------------------------------------------------------------------
def _remove(planes, min_area, phases):
    """cvmi_mask_remove_small twice on copies -> (u8 [N, H, W], info int64 [N, 8]) on the host; guards checked, the two runs equal."""
    lib = _lib.load()
    N, H, W = planes.shape
    nbytes = int(lib.cvmi_mask_remove_small_workspace(N, H, W))
    assert nbytes == 8 * N * H * W + 8 * N
    runs = []
    for fill in (-7, -9):
        mask = torch.full((planes.size + GUARD,), 7, dtype=torch.uint8, device="cuda")
        mask[:planes.size] = torch.tensor(planes).cuda().reshape(-1)
        info = torch.full((N * 8 + GUARD,), fill, dtype=torch.int32, device="cuda")
        ws = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cvmi_mask_remove_small(mask.data_ptr(), N, H, W, min_area, phases, info.data_ptr(), ws.data_ptr(), None), "mask_remove_small")
        torch.cuda.synchronize()
        assert bool((mask[planes.size:] == 7).all()), "mask: wrote past the end"
        assert bool((info[N * 8:] == fill).all()), "info: wrote past the end"
        assert bool((ws[nbytes:] == 0x5A).all()), "workspace: wrote past the end"
        runs.append((mask[:planes.size].view(N, H, W).cpu().numpy(), info[:N * 8].view(N, 8).cpu().numpy().astype(np.int64)))
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"
    return runs[0]


@pytest.mark.parametrize("phases", (1, 2, 3))
@pytest.mark.parametrize("rid", sorted(REMOVE_ROWS))
def test_remove_small_equals_the_reference(rid, phases):
    _, planes, min_area = REMOVE_ROWS[rid]
    want, want_info = ref.remove_small_stack(planes, min_area, phases)
    got, info = _remove(planes, min_area, phases)
    for k, name in enumerate(ref.INFO):
        assert np.array_equal(info[:, k], want_info[:, k]), (rid, phases, name, info[:, k].tolist()[:8], want_info[:, k].tolist()[:8])
    assert np.array_equal(got, want), (rid, phases, int((got != want).sum()))


def test_remove_small_known_answers():
    got, info = _remove(ref.art("#.#")[None], 2, 3)
    assert got.tolist() == [[[255, 255, 255]]] and info.tolist() == [[1, 3, 0, 0, 2, 0, 1, 0]]
    got, info = _remove(np.zeros((1, 1, 1), np.uint8), 2, 3)
    assert got.tolist() == [[[255]]] and info.tolist() == [[1, 1, 0, 0, 0, 0, 1, 0]]
    got, info = _remove(ref.art("#.#")[None], 2, 2)                              # both small, equal: the raster-first one stays
    assert got.tolist() == [[[255, 0, 0]]] and info.tolist() == [[1, 1, 0, 0, 0, 0, 0, 1]]
    _, planes, a = REMOVE_ROWS["plain"]                                          # empty, full, foreground bytes of 1: untouched, changed 0
    got, info = _remove(planes, a, 3)
    assert np.array_equal(got, planes) and not info[:, 0].any() and info[:, 1].tolist() == [0, 480, 192] and info[0, 2:6].tolist() == [0, 0, 0, 0]
    _, planes, a = REMOVE_ROWS["all_small"]
    got, info = _remove(planes, a, 3)
    assert got[1, 1, 1:4].all() and not got[1, 3:5].any() and info[:, 1].tolist() == [3, 3]


def test_remove_small_refuses_bad_arguments():
    lib = _lib.load()
    m = torch.zeros(64, dtype=torch.uint8, device="cuda")
    info = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    args = lambda **kw: [kw.get("m", m.data_ptr()), kw.get("N", 1), kw.get("H", 8), kw.get("W", 8), kw.get("min_area", 4), kw.get("phases", 3),
                         kw.get("info", info.data_ptr()), kw.get("ws", ws.data_ptr()), None]
    for bad in (dict(min_area=0), dict(min_area=-3), dict(phases=0), dict(phases=4), dict(m=None), dict(info=None), dict(ws=None), dict(N=0), dict(H=0), dict(W=0),
                dict(N=1 << 15, H=1 << 8, W=1 << 8)):
        assert lib.cvmi_mask_remove_small(*args(**bad)) != 0, bad
        assert b"mask_remove_small" in lib.cvmi_last_error()
    assert lib.cvmi_mask_remove_small_workspace(1 << 15, 1 << 8, 1 << 8) == 0 and lib.cvmi_mask_remove_small_workspace(1, 0, 8) == 0
    torch.cuda.synchronize()
    assert bool((info == -7).all()) and not bool(m.any())


# ---- the utilities --------------------------------------------------------------------------------------------------------------------------------------
def test_mask_to_rle_on_a_stack_and_through_the_repeat(monkeypatch):
    planes = np.concatenate([REMOVE_ROWS["blobs_130x70"][1], RLE_ROWS["random_130x70_d0.5"]])
    want = [ref.mask_to_rle(p) for p in planes]
    dev = torch.tensor(planes).cuda()
    assert sum(len(r["counts"]) for r in want) > planes.shape[0] * (amg_utils.RLE_RUNS_PER_COLUMN * 70 + 2)      # more runs than the guess: the repeat
    assert amg_utils.mask_to_rle(dev) == want
    few = amg_utils.mask_to_rle(dev[:3])                                         # ... and within the guess: one call
    assert few == want[:3] and all(amg_utils.area_from_rle(r) == int((p != 0).sum()) for r, p in zip(few, planes))
    assert all(np.array_equal(amg_utils.rle_to_mask(r), p != 0) for r, p in zip(few, planes))
    assert amg_utils.mask_to_rle(dev[:0]) == []


@pytest.mark.parametrize("mode", ("holes", "islands", "both"))
def test_remove_small_regions_through_more_planes_than_a_chunk_holds(mode, monkeypatch):
    _, planes, min_area = REMOVE_ROWS["blobs_33_planes"]
    N, H, W = planes.shape
    monkeypatch.setattr(amg_utils, "REMOVE_SMALL_WORKSPACE_BYTES", 8 * H * W * 4)          # four planes per call: nine calls, the last with one plane
    want, want_info = ref.remove_small_stack(planes, min_area, amg_utils.PHASES[mode])
    dev = torch.tensor(planes).cuda()
    out, changed = amg_utils.remove_small_regions(dev, min_area, mode)
    assert out is dev and changed.dtype == torch.bool and changed.cpu().tolist() == (want_info[:, 0] != 0).tolist()
    assert np.array_equal(dev.cpu().numpy(), want)


def _on_device(dicts):
    return [dict(d, segmentation=d["segmentation"].cuda()) for d in dicts]


def test_postprocess_small_regions_on_a_hand_built_list():
    """Two masks that differ only by a speck, the speckled one listed first: the unchanged one survives; unchanged masks come first."""
    dicts, min_area, nms_t = ref.post_case()
    want = ref.postprocess_small_regions(list(dicts), min_area, nms_t)
    dev = _on_device(dicts)
    keep = [d["segmentation"].clone() for d in dev]
    got = amg_utils.postprocess_small_regions(dev, min_area, nms_t)
    assert amg_ref.same_dicts(got, want), [d["predicted_iou"] for d in got]
    assert [d["predicted_iou"] for d in got] == [0.85, 0.8, 0.9]
    assert all(d["segmentation"].is_cuda for d in got) and all(torch.equal(d["segmentation"], k) for d, k in zip(dev, keep))       # the input is not modified
    rle = amg_utils.postprocess_small_regions(dev, min_area, nms_t, output_mode="uncompressed_rle")
    assert rle == ref.postprocess_small_regions(list(dicts), min_area, nms_t, output_mode="uncompressed_rle")
    for mutant in ref.POST_MUTANTS:
        assert not amg_ref.same_dicts(got, ref.postprocess_small_regions(list(dicts), min_area, nms_t, mutant=mutant)), mutant


# ---- the generator on the mini model of tests/test_amg_gpu.py --------------------------------------------------------------------------------------------
AREAS = (4, 16, 64, 256, 1024, 4096)


@functools.lru_cache(None)
def _base(dtype):
    """(generator, what generate_batch returns today on the two images, min_area): the smallest area of AREAS at which the reference post-process
    changes a mask of each image's list or drops one."""
    from test_amg_gpu import SIZES, _generator, _images
    gen = _generator(dtype)
    base = gen.generate_batch(_images(), orig_hw=SIZES)
    torch.cuda.synchronize()
    assert all(len(b) > 0 for b in base)
    for a in AREAS:
        post = [ref.postprocess_small_regions(b, a, gen.box_nms_thresh) for b in base]
        moved = [len(p) != len(b) or any(not torch.equal(x["segmentation"], y["segmentation"].cpu()) for x, y in zip(p, b)) for p, b in zip(post, base)]
        print(f"[amg_post {dtype}] min_area {a}: masks {[len(b) for b in base]} -> {[len(p) for p in post]}, lists changed {moved}")
        if any(moved):
            return gen, base, a
    raise AssertionError("no area of AREAS changes a mask: the test would pass with the post-process skipped")


def _same_but_rle(got, want):
    """`got` (RLE mode) equals `want` (binary or reference planes): the runs decode to the planes, area = area_from_rle, every other key equal."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        plane = torch.as_tensor(w["segmentation"]).cpu().numpy() != 0
        seg = g["segmentation"]
        if tuple(g) != amg_ref.KEYS or seg["size"] != list(plane.shape) or not np.array_equal(amg_utils.rle_to_mask(seg), plane) or seg != ref.mask_to_rle(plane):
            return False
        if g["area"] != amg_utils.area_from_rle(seg) or g["area"] != w["area"] or any(g[k] != w[k] for k in amg_ref.KEYS[2:]):
            return False
    return True


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_generator_per_call_options(dtype):
    from test_amg_gpu import SIZES, _images
    gen, base, a = _base(dtype)
    t = gen.box_nms_thresh
    want = [ref.postprocess_small_regions(b, a, t) for b in base]
    got = gen.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=a)
    for b in range(2):
        assert amg_ref.same_dicts(got[b], want[b]), (dtype, b, len(got[b]), len(want[b]))
        assert all(d["segmentation"].is_cuda and d["area"] == int((d["segmentation"] != 0).sum()) for d in got[b])
    rle = gen.generate_batch(_images(), orig_hw=SIZES, output_mode="uncompressed_rle")
    assert all(_same_but_rle(rle[b], base[b]) for b in range(2))
    both = gen.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=a, output_mode="uncompressed_rle")
    assert all(_same_but_rle(both[b], want[b]) for b in range(2))
    again = gen.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=0, output_mode="binary_mask")        # the defaults: today's path and result
    assert all(amg_ref.same_dicts(again[b], base[b]) for b in range(2))
    with pytest.raises(NotImplementedError, match="pycocotools"):
        gen.generate_batch(_images(), orig_hw=SIZES, output_mode="coco_rle")
    # box_nms_thresh = 1: the first NMS drops nothing, so the lists are long, the second NMS has an order to get right, and the RLE chunks many planes
    from test_amg_gpu import _generator
    every = _generator(dtype, box_nms_thresh=1.0)
    plain = every.generate_batch(_images(), orig_hw=SIZES)
    assert sum(map(len, plain)) > sum(map(len, base))
    for area in AREAS:
        want = [ref.postprocess_small_regions(b, area, 1.0) for b in plain]
        got = every.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=area)
        print(f"[amg_post {dtype}] box_nms_thresh 1, min_area {area}: {[len(b) for b in plain]} masks, order moved "
              f"{[[d['predicted_iou'] for d in w] != [d['predicted_iou'] for d in b] for w, b in zip(want, plain)]}")
        assert all(amg_ref.same_dicts(got[b], want[b]) for b in range(2)), (dtype, area)
    assert all(_same_but_rle(r, w) for r, w in zip(every.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=AREAS[-1], output_mode="uncompressed_rle"), want))


def test_generator_encodes_in_chunks_and_repeats_a_short_guess(monkeypatch):
    """The RLE mode with one plane per chunk and a capacity guess of two runs per plane: every chunk is rebuilt and encoded again; same lists."""
    from test_amg_gpu import SIZES, _images
    gen, base, a = _base("f32")
    want = [ref.postprocess_small_regions(b, a, gen.box_nms_thresh) for b in base]
    monkeypatch.setattr(amg_utils, "MASK_CHUNK_BYTES", 1)
    monkeypatch.setattr(amg_utils, "RLE_RUNS_PER_COLUMN", 0)
    rle = gen.generate_batch(_images(), orig_hw=SIZES, output_mode="uncompressed_rle")
    assert all(_same_but_rle(rle[b], base[b]) for b in range(2))
    both = gen.generate_batch(_images(), orig_hw=SIZES, min_mask_region_area=a, output_mode="uncompressed_rle")
    assert all(_same_but_rle(both[b], want[b]) for b in range(2))


def test_generate_takes_the_options_for_one_u8_image():
    _, _, a = _base("f32")
    from test_amg_gpu import _generator
    gen = _generator("f32")
    img = torch.randint(0, 256, (96, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).numpy()
    plain = gen.generate(img)
    assert amg_ref.same_dicts(gen.generate(img, min_mask_region_area=0, output_mode="binary_mask"), plain)
    want = ref.postprocess_small_regions(plain, a, gen.box_nms_thresh)
    assert amg_ref.same_dicts(gen.generate(img, min_mask_region_area=a), want)
    assert amg_ref.same_dicts(amg_utils.postprocess_small_regions(plain, a, gen.box_nms_thresh), want)
    assert _same_but_rle(gen.generate(img, min_mask_region_area=a, output_mode="uncompressed_rle"), want)
    assert _same_but_rle(gen.generate(img, output_mode="uncompressed_rle"), plain)
