"""The emitter against the route: everything Sam2Plan appends outside the Hiera blocks is what decoder_route.route_decoder names, with the byte and
flop counts, and the buffers, of tests/decoder_route_fixture.json -- recorded on a GPU from the plans of the commit BEFORE the route was separated
from the emitter (tests/test_decoder_route_cpu.py says how it is regenerated).  Four of the fixture's configurations: learned prompts, shared
layer 0, a mask prompt through the pair table, and the f32 repeat pass."""
import pytest
import torch

import sam2_route_cases as rc
from test_decoder_route_cpu import FIXTURE

pytestmark = pytest.mark.gpu

CASES = [c for c in rc.HEAD_CASES if c["id"] in ("learned_f16", "prompts2_f16", "pairs3_mask_f16", "prompts2_f32")]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_emits_what_the_route_names(case):
    sp = rc.build_head_plan(case)
    want = FIXTURE[case["id"]]
    head = [op for op in sp.plan.ops if not rc.BLOCK_LABEL.fullmatch(op[0])]
    assert [[op[0], op[1], op[3], op[4]] for op in head] == [x[:4] for x in want["launches"]]
    assert [[op[0], op[1]] for op in head[:2]] == rc.STEM and [(op[0], op[1]) for op in head[2:]] == sp.droute.launches()
    assert [(op[0], op[1]) for op in sp.plan.ops[-len(head) + 2:]] == sp.droute.launches()           # one contiguous run behind the trunk
    assert sp.act_bytes == want["act_bytes"]
    g = torch.Generator(device="cuda").manual_seed(0)
    sp.x_in.t.normal_(generator=g)
    if sp.droute.prompted:
        sp.coords[:, :2].copy_(torch.tensor([[40.0, 50.0], [200.0, 180.0]], device="cuda"))           # one box per pair
        sp.labels.copy_(torch.tensor([2, 3, -1], dtype=torch.int32, device="cuda").expand_as(sp.labels))
    if sp.mask_prompt:
        sp.mask_in.normal_(generator=g)
    if sp.pairs:
        sp.pair_image.copy_(torch.tensor([1, 0, 1], dtype=torch.int32))
    torch.cuda.synchronize()
    sp.plan.run_eager()
    torch.cuda.synchronize()
    assert torch.isfinite(sp.low_res).all()
