"""The emitter against the route, and the detector against what it computed before the route was separated from it: Yolo11Plan appends exactly
the launches yolo_route.route_yolo names, allocates the recorded bytes, and -- for the hash cases -- its outputs after an eager pass and after a
captured replay are bit for bit the recorded ones (tests/yolo_route_fixture.json; the library is the same, so equality is the bar).  2 x 96 x 160:
the smallest shape the whole-model tests use; the route depends on neither the batch nor the image size."""
import json
import os

import pytest

import yolo_route_cases as rc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "yolo_route_fixture.json")) as f:
    FIXTURE = json.load(f)["cases"]

HASHED = [c for c in rc.CASES if c["hashed"]]


@pytest.fixture(scope="module")
def weights_cache():
    return {}


@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_plan_emits_what_the_route_names(case, weights_cache):
    plan, rec = rc.build_plan(case, weights_cache), FIXTURE[case["id"]]
    assert plan.lanes == (3 if case["lanes"] is None else case["lanes"]) and tuple(plan.sw) == rc.switches_of(case)
    assert [tuple(op) for op in rc.plan_ops(plan)] == plan.route.launches()
    assert (plan.act_bytes, plan.wt.param_bytes) == (rec["act_bytes"], rec["param_bytes"])


@pytest.mark.parametrize("case", HASHED, ids=[c["id"] for c in HASHED])
def test_outputs_are_bit_for_bit_the_recorded_ones(case, weights_cache):
    got, want = rc.run_hashes(case, weights_cache), FIXTURE[case["id"]]["hashes"]
    print(case["id"], got["detections"])
    assert got["detections"] == want["detections"] and all(got["detections"])
    assert got["eager"] == want["eager"]
    assert got["graph"] == want["graph"]
