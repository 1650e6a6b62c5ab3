"""The mask-to-mask pass without a GPU: the numpy statement of cvmi_m2m_fanout (tests/m2m_ref.py) against torch.clamp / repeat_interleave, a
proof that the comparison tests/test_m2m_gpu.py makes tells every deliberately wrong variant from it, and the host side of the feature
(declaration, binding, the per-call arguments and the constructor's refusal)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import m2m_ref as ref
from circuitvision_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (ref.UPSTREAM_CLAMP, 0.75))
@pytest.mark.parametrize("row", ref.ROWS[:3], ids=lambda r: "n%d_nm%d_p%d_k%d" % r)
def test_reference_is_torch_clamp_and_repeat_interleave(row, c):
    n, NM, P, K = row
    low, coords, labels, pair_image = ref.fanout_inputs(n, NM, P, K, c)
    mask, co, la, pi = ref.fanout(low, c, coords, labels, pair_image)
    t = torch.clamp(torch.from_numpy(low), -c, c)
    assert ref.same_bits(mask, t.reshape(n * NM, P).numpy())
    assert ref.same_bits(mask, np.clip(low, np.float32(-c), np.float32(c)).reshape(n * NM, P))
    for got, src in ((co, coords), (la, labels), (pi, pair_image)):
        assert ref.same_bits(got, torch.from_numpy(src).repeat_interleave(NM, 0).numpy())
    for i in range(n):
        for k in range(NM):
            assert ref.same_bits(mask[i * NM + k], ref.clamp(low[i, k], c))                     # candidate-major inside the pair
            assert ref.same_bits(co[i * NM + k], coords[i]) and ref.same_bits(la[i * NM + k], labels[i]) and pi[i * NM + k] == pair_image[i]
    assert ref.fanout(low, c, coords, labels, None)[3] is None


def test_clamp_keeps_nan_and_the_sign_of_zero_and_bounds_the_infinities():
    c = np.float32(32.0)
    sp = ref.specials(c)
    got = ref.clamp(sp, c)
    inside_hi, inside_lo = np.nextafter(c, np.float32(0)), np.nextafter(-c, np.float32(0))
    want = np.array([c, -c, c, -c, inside_hi, inside_lo, c, -c, np.nan, -0.0, 0.0], dtype=np.float32)
    assert ref.same_bits(got, want)
    assert np.isnan(got[8]) and np.signbit(got[9]) and not np.signbit(got[10])
    assert not ref.same_bits(np.array([-0.0], dtype=np.float32), np.array([0.0], dtype=np.float32))          # the int32 view tells the zeros apart
    assert ref.same_bits(np.array([np.nan], dtype=np.float32), np.array([np.nan], dtype=np.float32))        # ... and equates a NaN with itself


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_comparison_rejects_every_wrong_variant(mutant):
    """On the rows of the GPU test with n > 1 and NM > 1 (where the orders differ), each wrong variant fails the bit-for-bit comparison."""
    for n, NM, P, K in ref.ROWS[1:3]:
        low, coords, labels, pair_image = ref.fanout_inputs(n, NM, P, K)
        want = ref.fanout(low, ref.UPSTREAM_CLAMP, coords, labels, pair_image)
        assert ref.same_fanout(ref.fanout(low, ref.UPSTREAM_CLAMP, coords, labels, pair_image), want)
        bad = ref.fanout(low, ref.UPSTREAM_CLAMP, coords, labels, pair_image, mutant)
        assert not ref.same_fanout(bad, want), (mutant, n, NM, P, K)
    # every row of the GPU test holds a NaN, a value beyond the bound and a -0.0 (or, in the 4-float row, as many as fit)
    for n, NM, P, K in ref.ROWS:
        low = ref.fanout_inputs(n, NM, P, K)[0]
        assert np.isnan(low).any() and (np.abs(low[np.isfinite(low)]) > ref.UPSTREAM_CLAMP).any() and (np.signbit(low) & (low == 0)).any(), (n, NM, P, K)
        for m in ("no_clamp", "nan_to_bound"):
            c, l, p = ref.fanout_inputs(n, NM, P, K)[1:]
            assert not ref.same_fanout(ref.fanout(low, ref.UPSTREAM_CLAMP, c, l, p, m), ref.fanout(low, ref.UPSTREAM_CLAMP, c, l, p)), (m, n, NM, P, K)


def test_the_long_row_needs_a_second_pass_of_the_grid_stride_loop():
    src = open(os.path.join(ROOT, "circuitvision_amd", "csrc", "mask_prompt.hip")).read()
    nt = int(re.search(r"constexpr int NT = (\d+)", src).group(1))
    gx = int(re.search(r"constexpr int M2M_GRID_X = (\d+)", src).group(1))
    assert ref.GRID_PASS_FLOATS == gx * nt * 4
    n, NM, P, K = ref.ROWS[-1]
    assert NM * P > ref.GRID_PASS_FLOATS and P % 4 == 0 and -(-(NM * P // 4) // nt) > gx and n > 1


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    decl = re.search(r"\nint cvmi_m2m_fanout\(([^;]*)\);", header)
    assert decl and "cvmi_m2m_fanout" in _lib.SIGNATURES
    args = [a.strip() for a in decl.group(1).split(",")]
    res, bound = _lib.SIGNATURES["cvmi_m2m_fanout"]
    kind = lambda a: ctypes.c_void_p if ("*" in a or a.startswith("cvmi_stream_t")) else {"int": ctypes.c_int, "float": ctypes.c_float}[a.split()[0]]
    assert res is ctypes.c_int and [kind(a) for a in args] == bound
    assert [a.split()[-1].lstrip("*") for a in args] == ["low_res", "NM", "clamp", "mask_out", "coords", "labels", "pair_image", "coords_out", "labels_out",
                                                         "pair_image_out", "n", "P", "K", "stream"]


def test_per_call_arguments_and_the_constructor_refusal():
    from circuitvision_amd import amg, sam2_infer
    model = types.SimpleNamespace(image_size=256)
    with pytest.raises(NotImplementedError, match=re.escape("generate(image, use_m2m=True)")) as e:
        amg.Sam2AutomaticMaskGenerator(model, use_m2m=True)
    assert "use_m2m" in str(e.value) and "per-call" in str(e.value) and "generate_batch" in str(e.value)
    gen = amg.Sam2AutomaticMaskGenerator(model, points_per_side=2)
    for fn in (gen.generate, gen.generate_batch):
        assert inspect.signature(fn).parameters["use_m2m"].default is False
    p = inspect.signature(sam2_infer.SAM2Model.infer_masks).parameters
    assert p["m2m"].default is False and p["m2m_clamp"].default == 32.0 and p["refine_steps"].default == 0
    assert list(p)[-3:] == ["refine_steps", "m2m", "m2m_clamp"]                                   # appended: positional callers are untouched
    check = sam2_infer.SAM2Model._check_m2m
    assert check(False, 32.0, 0) is None and check(False, 32.0, 2) is None and check(True, 32, 0) == 32.0
    with pytest.raises(ValueError, match="refine_steps"):
        check(True, 32.0, 1)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="m2m_clamp"):
            check(True, bad, 0)
    assert sam2_infer.M2M_MAX_PAIRS == 65535


def test_sub_batches_bound_the_second_plan():
    """With use_m2m the images decoded together keep the second plan at or below M2M_PAIRS_IN_FLIGHT pairs; without it the step is the pool's."""
    from circuitvision_amd import amg
    gen = amg.Sam2AutomaticMaskGenerator(types.SimpleNamespace(image_size=1024), points_per_side=32, points_per_batch=64)
    pool_step = amg.POOL_BYTES_IN_FLIGHT // (gen.cap * 256 * 256 * 4)
    assert gen._images_in_flight(False) == pool_step == 5
    assert gen._images_in_flight(True) == min(pool_step, amg.M2M_PAIRS_IN_FLIGHT // (3 * 64)) == 5
    big = amg.Sam2AutomaticMaskGenerator(types.SimpleNamespace(image_size=256), points_per_side=8, points_per_batch=64)
    assert big._images_in_flight(False) > 5 and big._images_in_flight(True) == 5 and 5 * 3 * 64 <= amg.M2M_PAIRS_IN_FLIGHT
    one = amg.Sam2AutomaticMaskGenerator(types.SimpleNamespace(image_size=256), points_per_side=8, points_per_batch=1024)
    assert one._images_in_flight(True) == 1                                                     # one image always goes through
