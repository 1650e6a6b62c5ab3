"""The outputs of the resampling kernels whose bits are pinned (tests/test_resample_bits_gpu.py against tests/resample_bits_fixture.json), and the
recorder of that fixture.

What is hashed (SHA-256 of the output bytes):
  transform  every non-refused (row, form, output type, swap_rb) case of op_matrix.RESAMPLE_ROWS, as tests/test_resample_matrix_gpu.py launches it;
  mask       cvmi_bilinear_f32 (the f32 map and the u8 mask) and cvmi_mask_postprocess (the u8 mask and the extents) on MASK_SHAPES.
Operands: the transform's are the matrix' seeded u8 images; the mask planes are integer draws times 2^-10, so neither depends on the host CPU.
Every operand's own hash is recorded too, and the test asserts it first.

`python tests/resample_bits_cases.py OUT.json` (on a GPU, from the repository root) records.  The fixture in the tree was recorded with
CVMI_LIB_PATH naming a library built from the commit BEFORE the family moved to resample.hip: run the recorder only before a change that is
meant to leave these outputs alone, or after one that changes them on purpose (and say so in that pull request).
`python tests/resample_bits_cases.py --print` prints the same hashes plus those of WORKLOAD (the pipeline's sizes) as JSON lines, for an A/B of
two builds (tools/resample_bench.py times the same launches); for the _sizes and _rects_dev forms also the number of mask bytes that differ from
cvmi_mask_postprocess's in the same process."""
import hashlib
import json
import os
import sys

import numpy as np

MASK_SHAPES = ((3, 12, 10, 33, 29), (1, 64, 64, 513, 512))     # N, h, w, H, W; 513 x 512 > 1024 x 256: the grid's second pass
MASK_THRESHOLD = 0.0
N_THRESHOLDS = 64                                                  # thresholds the four-forms test takes from the map itself
# the pipeline's sizes: 768 x 1024 images, B = 16, the segmenter at 1024
WORKLOAD = dict(B=16, H=768, W=1024, R=1024)


def sha(t):
    """SHA-256 of a tensor's (or array's) bytes."""
    if hasattr(t, "detach"):
        import torch
        t = t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def mask_operand(N, h, w):
    """f32 [N, h, w]: integers in [-2^15, 2^15) times 2^-10 -- values in [-32, 32) on a 2^-10 grid, the same bits on every host."""
    import torch
    rs = np.random.RandomState(1000 * h + w)
    return torch.from_numpy((rs.randint(-2 ** 15, 2 ** 15, size=(N, h, w)).astype(np.float32) * np.float32(2.0 ** -10)))


def mask_id(shape):
    return "mask_%dx%dx%d_to_%dx%d" % shape


def transform_rows():
    from op_matrix import RESAMPLE_ROWS
    return [r for r in RESAMPLE_ROWS if r["op"] == "transform" and set(r["forms"]) - set(r["refuse"])]


def transform_operand_hash(row):
    from resample_ref import tf_images
    h = hashlib.sha256()
    for im in tf_images(row["id"]):
        h.update(np.ascontiguousarray(im).tobytes())
    return h.hexdigest()


def transform_hashes(lib, row):
    """{form/type/swap: SHA-256 of the whole output} of the row's non-refused cases."""
    import torch
    from helper_ref import TDT
    from test_resample_matrix_gpu import _transform_call
    out = {}
    n, R = len(row["items"]), row["R"]
    for form in row["forms"]:
        if form in row["refuse"]:
            continue
        for dt in row["dtypes"]:
            for swap in ((0,) if form == "single" else row["swaps"]):
                dst = torch.zeros(n * R * R * 3, dtype=TDT[dt], device="cuda")
                call, keep = _transform_call(lib, row, form, dt, swap, dst.data_ptr())
                assert call() == 0, (row["id"], form, dt, swap, lib.cvmi_last_error().decode())
                torch.cuda.synchronize()
                out["%s/%s/swap%d" % (form, dt, swap)] = sha(dst)
                del keep
    return out


def mask_hashes(lib, shape):
    """{output: SHA-256} of cvmi_bilinear_f32 and cvmi_mask_postprocess on one of MASK_SHAPES."""
    import torch
    N, h, w, H, W = shape
    low = mask_operand(N, h, w).cuda()
    y = torch.zeros(N, H, W, dtype=torch.float32, device="cuda")
    m0, m1 = (torch.zeros(N, H, W, dtype=torch.uint8, device="cuda") for _ in range(2))
    ext = torch.zeros(N, 4, dtype=torch.int32, device="cuda")
    assert lib.cvmi_bilinear_f32(low.data_ptr(), N, h, w, y.data_ptr(), H, W, m0.data_ptr(), MASK_THRESHOLD, None) == 0
    assert lib.cvmi_mask_postprocess(low.data_ptr(), N, h, w, H, W, MASK_THRESHOLD, m1.data_ptr(), ext.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return {"bilinear_f32/map": sha(y), "bilinear_f32/mask": sha(m0), "mask_postprocess/mask": sha(m1), "mask_postprocess/extent": sha(ext)}


def record(lib):
    fx = {"transform": {}, "mask": {}}
    for row in transform_rows():
        fx["transform"][row["id"]] = {"operand": transform_operand_hash(row), "out": transform_hashes(lib, row)}
    for shape in MASK_SHAPES:
        fx["mask"][mask_id(shape)] = {"operand": sha(mask_operand(*shape[:3])), "out": mask_hashes(lib, shape)}
    return fx


# ---- the pipeline's sizes (A/B of two builds; not in the fixture: 100 MB of operands are no test) ------------------------------------------------
def workload_operands():
    """(u8 images [B,H,W,3], device windows int32 [B,4] = the whole image, logits f32 [B,R,R]) on the device, seeded."""
    import torch
    B, H, W, R = (WORKLOAD[k] for k in "BHWR")
    rs = np.random.RandomState(5)
    src = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3), dtype=np.uint8)).cuda()
    win = torch.tensor([[0, 0, W, H]] * B, dtype=torch.int32).cuda()
    coarse = torch.from_numpy(rs.randint(-2 ** 12, 2 ** 12, size=(B, 1, 32, 32)).astype(np.float32) * np.float32(2.0 ** -10))
    low = torch.nn.functional.interpolate(coarse, size=(R, R), mode="bilinear", align_corners=False)[:, 0].contiguous().cuda()     # smooth blobs, like logits
    return src, win, low


def workload_calls(lib, src, win, low):
    """{name: (call, outputs)} of the launches the pipeline makes at its sizes: the f16 transform with swap_rb through `batch` and `rects_dev`,
    the mask return through mask_postprocess, _sizes and _rects_dev."""
    import torch
    from circuitvision_amd._lib import F16
    B, H, W, R = (WORKLOAD[k] for k in "BHWR")
    x = {k: torch.zeros(B, R, R, 3, dtype=torch.float16, device="cuda") for k in ("batch", "rects_dev")}
    u8 = {k: torch.zeros(B, H * W, dtype=torch.uint8, device="cuda") for k in ("mask_postprocess", "mask_postprocess_sizes", "mask_postprocess_rects_dev")}
    ext = {k: torch.zeros(B, 4, dtype=torch.int32, device="cuda") for k in u8}
    sizes = np.ascontiguousarray(np.array([[H, W]] * B, dtype=np.int32))
    thr = MASK_THRESHOLD
    calls = {
        "batch": lambda: lib.cvmi_sam2_transform_batch(src.data_ptr(), B, H, W, x["batch"].data_ptr(), R, F16, 1, None),
        "rects_dev": lambda: lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), H * W * 3, H, W, win.data_ptr(), B, x["rects_dev"].data_ptr(), R, F16, 1, None),
        "mask_postprocess": lambda: lib.cvmi_mask_postprocess(low.data_ptr(), B, R, R, H, W, thr, u8["mask_postprocess"].data_ptr(), ext["mask_postprocess"].data_ptr(), None),
        "mask_postprocess_sizes": lambda: lib.cvmi_mask_postprocess_sizes(low.data_ptr(), B, R, R, sizes.ctypes.data, thr, u8["mask_postprocess_sizes"].data_ptr(),
                                                                          ext["mask_postprocess_sizes"].data_ptr(), None),
        "mask_postprocess_rects_dev": lambda: lib.cvmi_mask_postprocess_rects_dev(low.data_ptr(), B, R, R, win.data_ptr(), H * W, thr,
                                                                                  u8["mask_postprocess_rects_dev"].data_ptr(), ext["mask_postprocess_rects_dev"].data_ptr(), None),
    }
    outs = {k: ((x[k],) if k in x else (u8[k], ext[k])) for k in calls}
    return calls, outs, sizes


def main(argv):
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    from circuitvision_amd import _lib
    lib = _lib.load()
    fx = record(lib)
    if argv[:1] != ["--print"]:
        with open(argv[0], "w") as f:
            json.dump(fx, f, indent=0, sort_keys=True)
            f.write("\n")
        print("recorded %d transform rows, %d mask shapes with %s" % (len(fx["transform"]), len(fx["mask"]), _lib.LIB_PATH))
        return
    for kind in ("transform", "mask"):
        for rid, rec in sorted(fx[kind].items()):
            for name, h in sorted(rec["out"].items()):
                print(json.dumps({"case": "%s/%s" % (rid, name), "sha256": h}))
    src, win, low = workload_operands()
    calls, outs, _sizes = workload_calls(lib, src, win, low)
    for name, call in calls.items():
        assert call() == 0, (name, lib.cvmi_last_error().decode())
        torch.cuda.synchronize()
        rec = {"case": "workload/" + name, "sha256": [sha(t) for t in outs[name]]}
        if name in ("mask_postprocess_sizes", "mask_postprocess_rects_dev"):        # the same planes at the same places: bytes unlike cvmi_mask_postprocess's
            rec["bytes_unlike_mask_postprocess"] = int((outs[name][0] != outs["mask_postprocess"][0]).sum())
        print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
