"""The Hiera route (circuitvision_amd/hiera_route.py) without a GPU: the trunk's (label, kind) launch sequence of every configuration in
tests/sam2_route_cases.py, derived from the pure functions alone, against tests/sam2_route_fixture.json.

The fixture was recorded on a GPU from the plans of the commit BEFORE the route was separated from the emitter, so it is not a copy of what the
code under test says.  A later change that alters routing on purpose regenerates it on a GPU with `python tests/sam2_route_cases.py
tests/sam2_route_fixture.json` (it records `Sam2Plan(...).plan.timed_eager(with_kernels=True)`: labels, kinds and the kernels dispatched), reviews the diff of the file, and says so; a change that is meant to leave
the launches alone must pass against the file as it stands."""
import ast
import json
import os

import pytest

import sam2_route_cases as rc
from circuitvision_amd import hiera_route as hr

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "sam2_route_fixture.json")) as f:
    FIXTURE = json.load(f)

ON = hr.SamSwitches(*(True,) * len(hr.SamSwitches._fields))
FIELD_OF = {name: f for f, (name, _, _) in hr.SWITCH_TABLE.items()}


def _switches(env):
    return ON._replace(**{FIELD_OF[k]: v != "0" for k, v in env.items()})


def _routes(case, sw=None):
    sw = _switches(case["env"]) if sw is None else sw
    return hr.route_trunk(rc.hiera_of(case["hiera"]), case["size"], case["B"], rc.dtype_of(case["dtype"]), case["attn"] == "fp8", sw)


L16 = next(c for c in rc.CASES if c["id"] == "L_f16_B16")


def test_switch_table_is_the_twelve_switches():
    assert tuple(hr.SWITCH_TABLE) == hr.SamSwitches._fields and [n for n, _, _ in hr.SWITCH_TABLE.values()] == list(rc.SWITCHES)
    assert hr.WEIGHT_SWITCHES == hr.SamSwitches._fields[:5] and {r for _, r, _ in hr.SWITCH_TABLE.values()} == {"weights", "plan"}
    with open(os.path.join(os.path.dirname(HERE), "INTEGRATION.md")) as f:
        doc = f.read()
    for name, reader, _ in hr.SWITCH_TABLE.values():                       # the documented table says what the code's table says
        assert f"| `{name}` | `{'Sam2Weights' if reader == 'weights' else 'Sam2Plan'}` |" in doc, name
    assert doc.count("| `CVMI_SAM_") == len(hr.SWITCH_TABLE)


def test_sam_switches_reads_the_environment_when_called(monkeypatch):
    for name in rc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert hr.sam_switches() == ON
    for name in rc.SWITCHES:
        monkeypatch.setenv(name, "0")
        assert hr.sam_switches() == ON._replace(**{FIELD_OF[name]: False})
        monkeypatch.setenv(name, "2")                    # anything but "0" leaves the switch on
        assert hr.sam_switches() == ON
        monkeypatch.delenv(name)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_route_gives_the_recorded_launch_sequence(case):
    """... and every recorded kernel is of the family the route's choice implies: a fused or token-stationary path that stops being taken fails
    here, not only in the benchmark."""
    routes = _routes(case)
    blocks, _ = hr.hiera_blocks(rc.hiera_of(case["hiera"]))
    got = [[[label.split(".", 1)[1], kind] for label, kind in r.launches(i)] for i, r in enumerate(routes)]
    want = rc.expand(FIXTURE[case["id"]])
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == [x[:2] for x in w], (case["id"], i)
        for suffix, _, family in w:
            assert rc.family_implied(suffix, family, routes[i], blocks[i].window), (case["id"], i, suffix, family, routes[i])


def test_hiera_l_f16_b16_takes_the_fused_launches_in_stages_1_and_2_only():
    routes = _routes(L16)
    blocks, stage_ends = hr.hiera_blocks(rc.hiera_of("HIERA_L"))
    assert stage_ends == [1, 7, 43, 47]
    assert [i for i, r in enumerate(routes) if r.qkv == "fused"] == list(range(9))
    assert all(r.attn == "window" for r in routes[:9])
    assert [i for i, r in enumerate(routes) if r.proj == "fused"] == list(range(8))
    assert [i for i, r in enumerate(routes) if r.mlp == "fused"] == list(range(8))
    # stage 3 = blocks 8 .. 43 (8 is the transition INTO it and still attends in stage 2's windows): none fused from block 9 on
    assert all(r.qkv != "fused" and r.proj != "fused" for r in routes[9:])


# the Hiera-L (f16, B = 16) blocks whose route each switch governs -- reasoned from the trunk's shape, not read off the code under test:
# stage 1 = 0 - 1 (144 wide), stage 2 = 2 - 7 (288), stage 3 = 8 - 43 (576), stage 4 = 44 - 47 (1152); 2 / 8 / 44 are the q-pooling transitions,
# which read the narrower width; no grid is padded; tok_linear is built for K = 144 / 288 / 576, the fused MLP for 144 / 288
GOVERNS = {
    "CVMI_SAM_FUSED_MLP": set(range(0, 9)),                  # the MLP launch of 0 - 7, and the statistics it wrote for the norm1 of 1 - 8
    "CVMI_SAM_TOKLIN": set(range(0, 45)),                    # every tok_linear launch, 44's pooled dimproj included
    "CVMI_SAM_QLOG2": set(range(0, 48)),                     # every attention descriptor
    "CVMI_SAM_QKVATTN": set(range(0, 9)),
    "CVMI_SAM_QKVATTN16": set(range(3, 9)),
    "CVMI_SAM_QKVTOK_TRANS": {2, 8, 44},
    "CVMI_SAM_POOLFUSE": {2, 8, 44},
    "CVMI_SAM_LNSTATS": set(range(0, 45)),                   # producers 0 - 43 (MLP, proj -> fc1, fc2) and consumers 1 - 44 (K = 576 qkv)
    "CVMI_SAM_LNSTATS_FC2": set(range(8, 45)),               # fc2 of 8 - 43, norm1 of 9 - 44
    "CVMI_SAM_PROJMLP": set(range(0, 8)),
    "CVMI_SAM_NECKCAST": set(),                              # neck
    "CVMI_SAM_SHARE_L0": set(),                              # decoder
}


@pytest.mark.parametrize("name", rc.SWITCHES)
def test_each_switch_changes_only_the_blocks_it_governs(name):
    """Every switch set to "0" alone changes the route of at least one Hiera-L block (the two that govern the neck and the decoder: of none) and
    of no block outside GOVERNS[name]."""
    base, off = _routes(L16), _routes(L16, _switches({name: "0"}))
    changed = {i for i, (a, b) in enumerate(zip(base, off)) if a != b}
    assert changed <= GOVERNS[name], sorted(changed - GOVERNS[name])
    assert bool(changed) == bool(GOVERNS[name])


@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_routes_name_only_packed_forms_the_packing_function_produces(case):
    sw = _switches(case["env"])
    blocks, _ = hr.hiera_blocks(rc.hiera_of(case["hiera"]))
    packed = hr.block_packings(blocks, rc.dtype_of(case["dtype"]), sw)
    for i, r in enumerate(_routes(case)):
        need = {f"b{i}.dimproj"} if r.dimproj == "tok_pool" else set()
        need |= {f"b{i}.qkv", f"b{i}.qkv_attn"} if r.qkv == "fused" else {f"b{i}.qkv"} if r.qkv == "tok" else set()
        need |= {f"b{i}.projmlp"} if r.proj == "fused" else {f"b{i}.proj"} if r.proj == "tok" else set()
        need |= {f"b{i}"} if r.mlp == "fused" else {f"b{i}.fc1"} if r.mlp == "tok_fc1" else set()
        assert need <= packed, (case["id"], i, sorted(need - packed))
        assert (r.proj == "fused") <= (r.mlp == "fused"), (case["id"], i)           # the proj prologue belongs to the fused MLP launch


def test_weights_pack_what_the_packing_function_names():
    """Sam2Weights (built on the CPU) holds exactly block_packings' keys beside the neck's two."""
    from circuitvision_amd._lib import F16
    from circuitvision_amd.sam2 import Sam2Weights, SamSyntheticParams
    hiera = rc.hiera_of("MINI144")
    wt = Sam2Weights(SamSyntheticParams(seed=5, lora_targets=rc.lora_targets_of("MINI144"), std=0.05), hiera, 256, F16, device="cpu")
    blocks, stage_ends = hr.hiera_blocks(hiera)
    assert (wt.blocks, wt.stage_ends) == (blocks, stage_ends)
    assert (set(wt.tl) | set(wt.mlp)) - {"feat_s0", "feat_s1"} == wt.packed_keys == hr.block_packings(blocks, F16, wt.sw)
    assert {"b0.qkv_attn", "b2.qkv_attn", "b3.qkv_attn", "b0.projmlp", "b2", "b3.fc1", "b3.dimproj"} <= wt.packed_keys and "b4.qkv_attn" not in wt.packed_keys
    # ... and distributed.weight_tensors, which walks a weights object's dicts of packed tensors by attribute name, still finds every one of them
    from circuitvision_amd.distributed import packed_tensors, weight_tensors
    got = {id(t) for t in weight_tensors(wt)}
    for d in (wt.pc, wt.tl, wt.mlp):
        assert d and {id(t) for t in packed_tensors(d)} <= got


def test_statistics_are_consumed_only_for_the_rows_they_were_written_for():
    """The statistics state carries the producer's row count: a consumer with other rows (here the same block asked at another batch) takes none."""
    blocks, _ = hr.hiera_blocks(rc.hiera_of("HIERA_L"))
    from circuitvision_amd._lib import F16
    packed = hr.block_packings(blocks, F16, ON)
    r0 = hr.route_block(blocks, packed, 0, 16, 256, 256, F16, False, ON, None)
    assert r0.stats_next == (16 * 256 * 256, 0) and r0.stats_mlp
    assert hr.route_block(blocks, packed, 1, 16, 256, 256, F16, False, ON, r0.stats_next).stats_in == 0
    assert hr.route_block(blocks, packed, 1, 8, 256, 256, F16, False, ON, r0.stats_next).stats_in is None


@pytest.mark.parametrize("module", ["sam2.py", "hiera_route.py"])
def test_only_the_switch_function_touches_the_environment(module):
    path = os.path.join(os.path.dirname(HERE), "circuitvision_amd", module)
    with open(path) as f:
        src = f.read()
    tree = ast.parse(src)
    spans = [(n.lineno, n.end_lineno) for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "sam_switches"]
    hits = [k + 1 for k, line in enumerate(src.splitlines()) if "os.environ" in line or "getenv" in line or "import os" in line and module == "sam2.py"]
    assert all(any(a <= k <= b for a, b in spans) for k in hits), (module, hits)
    assert (module == "hiera_route.py") == bool(hits)
