"""The decoder route (circuitvision_amd/decoder_route.py) without a GPU: the (label, kind) launch sequence after the trunk of every configuration
in tests/sam2_route_cases.py's HEAD_CASES, derived from `route_decoder` alone, against tests/decoder_route_fixture.json; and the relations between
the route's fields that the emitter relies on.

The fixture was recorded on a GPU from the plans of the commit BEFORE the route was separated from the emitter (`Sam2Plan._neck_decoder` as one
method), so it is not a copy of what the code under test says.  A later change that alters these launches on purpose regenerates it on a GPU with
`python tests/sam2_route_cases.py --head tests/decoder_route_fixture.json`, reviews the diff of the file, and says so; a change that is meant to leave
the launches alone must pass against the file as it stands."""
import itertools
import json
import os

import pytest

import sam2_route_cases as rc
from circuitvision_amd import decoder_route as dr
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import is16
from test_sam2_route_cpu import ON, _switches

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "decoder_route_fixture.json")) as f:
    FIXTURE = json.load(f)


def _route(case):
    dims = [rc.hiera_of(case["hiera"])["embed_dim"] * 2 ** s for s in range(4)]
    dt = rc.dtype_of(case["dtype"])
    # Sam2Weights packs feat_s0 / feat_s1 for tok_linear on 16-bit plans where the kernel is built for the stage width (at most 288)
    tok = tuple(is16(dt) and d <= 288 and dr.tok_linear_supported(d, dt, 256) for d in dims[:2])
    return dr.route_decoder(dt, case["B"], case["size"], _switches(case["env"]), refine=case["refinement"], neck_tok=tok, stage_dims=dims, **case["plan"])


@pytest.mark.parametrize("case", rc.HEAD_CASES, ids=[c["id"] for c in rc.HEAD_CASES])
def test_route_gives_the_recorded_launch_sequence(case):
    """... and the neck launches run the kernel family the route's arm implies (tok_linear, or anything else)."""
    want = FIXTURE[case["id"]]["launches"]
    r = _route(case)
    assert [x[:2] for x in want[:2]] == rc.STEM
    assert [list(lk) for lk in r.launches()] == [x[:2] for x in want[2:]]
    family = {x[0]: x[4] for x in want}
    for j, arm in enumerate(r.neck):
        assert family[f"feat_s{j}"].startswith("tok_linear") == (arm == "tok"), (j, arm, family[f"feat_s{j}"])


def test_the_cases_reach_every_arm():
    routes = [_route(c) for c in rc.HEAD_CASES]
    assert {r.stream for r in routes} == {"dense", "shared", "repeat", "gather", "mask_prompt"}
    assert {r.masks for r in routes} == {"multimask_out", "select_mask"} and {r.upsample for r in routes} == {"upsample_refine", "upsample", None}
    assert {r.neck for r in routes} == {("tok", "tok"), ("gemm", "gemm")} and {r.tokens for r in routes} == {"const", "prompt"}
    assert {r.castk[0] for r in routes} == {"emb", "keys", None}


MODES = [dict(), dict(prompts=2), dict(prompts=2, mask_prompt=True), dict(prompts=2, multimask=True), dict(pairs=3), dict(pairs=3, mask_prompt=True)]
TABLE = list(itertools.product((F16, BF16, F32), (True, False), MODES))       # dtype x CVMI_SAM_SHARE_L0 x prompt mode


@pytest.mark.parametrize("dtype,share,mode", TABLE)
def test_stream_and_castk_follow_from_mode_dtype_and_switch(dtype, share, mode):
    r = dr.route_decoder(dtype, 2, 256, ON._replace(share_l0=share), **mode)
    prompted, masked = bool(mode.get("prompts") or mode.get("pairs")), bool(mode.get("mask_prompt"))
    assert r.prompted == prompted and r.NB == (mode.get("pairs") or 2 * mode.get("prompts", 1)) and r.T == (9 if prompted else 38)
    assert (r.stream == "shared") == (prompted and is16(dtype) and share and not masked)
    assert (r.stream == "dense") == (not prompted) and (r.stream == "mask_prompt") == masked
    if r.stream in ("repeat", "gather"):
        assert (r.stream == "gather") == bool(mode.get("pairs"))
    # layer 0's operand copy: cast from the per-image embedding exactly when shared; no cast exactly when the stream's own launch wrote it
    assert (r.castk[0] == "emb") == (r.stream == "shared")
    assert (r.castk[0] is None) == (r.stream in ("gather", "mask_prompt") and is16(dtype))
    assert r.castk[0] in ("emb", "keys", None)
    # layer 1 and the final attention: norm4 has written a 16-bit plan's copy; an f32 plan casts (copies) the stream
    assert r.castk[1:] == ((None, None) if is16(dtype) else ("keys", "keys"))
    assert r.tokens == ("prompt" if prompted else "const")
    assert r.masks == ("multimask_out" if mode.get("multimask") else "select_mask")
    assert r.upsample == ("upsample" if prompted else "upsample_refine")
    labels = [l for l, _ in r.launches()]
    assert len(set(labels)) == len(labels)
    for name, launch in dr.STREAM_LAUNCH.items():
        assert (launch in labels) == (r.stream == name)
    assert [l for l in labels if l.endswith("castk")] == [f"{p}.castk" for p, c in zip(("l0.t2i", "l1.t2i", "final"), r.castk) if c]


def test_upsample_and_neck_arms():
    kw = dict(neck_tok=(True, True), stage_dims=(144, 288, 576, 1152))
    assert dr.route_decoder(F16, 2, 256, ON, high_res=False).upsample is None
    assert dr.route_decoder(F16, 2, 256, ON, refine=False).upsample == "upsample"
    r = dr.route_decoder(F16, 2, 256, ON, **kw)
    assert r.neck == ("tok", "tok") and r.casts == (2, 3)
    assert dr.route_decoder(F16, 2, 256, ON._replace(neckcast=False), **kw).casts == (0, 1, 2, 3)
    assert dr.route_decoder(F16, 1, 64, ON, **kw).neck == ("tok", "gemm")                   # 16 x 16 = 256 rows, 8 x 8 = 64: no whole workgroup
    r32 = dr.route_decoder(F32, 2, 256, ON, **kw)
    assert r32.neck == ("gemm", "gemm") and r32.casts == ()                                  # f32: the stage outputs are the operands


def test_argument_checks_raise():
    with pytest.raises(ValueError, match="alternatives"):
        dr.route_decoder(F16, 2, 256, ON, prompts=3, pairs=8)
    for pairs in (-1, 65536):
        with pytest.raises(ValueError, match="pairs must be in 1 .. 65535"):
            dr.route_decoder(F16, 2, 256, ON, pairs=pairs)
    for kw in (dict(mask_prompt=True), dict(multimask=True)):
        with pytest.raises(ValueError, match="need prompts > 0"):
            dr.route_decoder(F16, 2, 256, ON, **kw)
    assert dr.route_decoder(F16, 2, 256, ON, pairs=65535, mask_prompt=True, multimask=True).NB == 65535
