"""Configurations whose YOLO11 launch sequence, buffer sizes, packed weights and output bits are pinned (tests/test_yolo_route_cpu.py and
tests/test_yolo_route_gpu.py against tests/yolo_route_fixture.json), and the recorder of that fixture.

`python tests/yolo_route_cases.py --weights OUT.json` (no GPU) records, per scale in WEIGHT_SCALES, the parameters `Yolo11Weights` pulls (names and
shapes in pull order), its packed keys in order and one SHA-256 over every packed tensor.  `python tests/yolo_route_cases.py OUT.json` (on a GPU)
adds, per case, every op of the plan as [label, kind, lane, kernel dispatched], `act_bytes`, `param_bytes` and, for the hash cases, the SHA-256 of
the outputs after one eager pass and after one captured replay.  It uses nothing but `Yolo11Plan(...).plan.ops`, `.plan.lanes` and
`plan.timed_eager(with_kernels=True)`: run it BEFORE a change that is meant to leave the detector alone, or after one that changes it on purpose
(and say so in that pull request).  The weights are `exact_params()`, so that neither part of the file depends on the CPU it was recorded on."""
import hashlib
import json
import os
import sys

NC, SEED, CONF = 62, 11, 0.001               # seeded random weights score every anchor low: a threshold below their scores, so that NMS has work
SWITCHES = ("CVMI_FUSE_C3K2", "CVMI_FUSE_DWPW", "CVMI_FUSE_STEM")
WEIGHT_SCALES = ("n", "l")


def _case(id, scale, dtype, H=96, W=160, env=None, fuse=True, lanes=None, hashed=False, runs=True):
    return dict(id=id, scale=scale, dtype=dtype, B=2, H=H, W=W, env=env or {}, fuse=fuse, lanes=lanes, hashed=hashed, runs=runs)


# 2 x 96 x 160 (and 2 x 160 x 224 for n): the smallest shapes the whole-model tests use; the route depends on neither B nor H x W
CASES = [
    _case("n_f16", "n", "f16", hashed=True), _case("n_f16_160x224", "n", "f16", 160, 224),
    _case("s_f16", "s", "f16"), _case("m_f16", "m", "f16"), _case("l_f16", "l", "f16", hashed=True), _case("x_f16", "x", "f16"),
    _case("n_f32", "n", "f32", hashed=True), _case("l_f32", "l", "f32"),
    # a bf16 plan builds, but the detector's helper kernels (dwconv3x3, sppf_pool, detect_decode) are built for f16 / f32: it is not run
    _case("n_bf16", "n", "bf16", runs=False),
] + [_case(f"n_f16_{name[5:]}=0", "n", "f16", env={name: "0"}) for name in SWITCHES] + [
    _case("n_f16_all=0", "n", "f16", env={name: "0" for name in SWITCHES}),
    _case("n_f16_fuse_c3k2=False", "n", "f16", fuse=False, hashed=True),
] + [_case(f"n_f16_lanes{k}", "n", "f16", lanes=k, hashed=k in (0, 3)) for k in range(6)]

FUSED_FAMILIES = ("c3k2_kernel", "stem2_kernel", "dwpw_kernel")


def dtype_of(name):
    from circuitvision_amd._lib import BF16, F16, F32
    return dict(f16=F16, bf16=BF16, f32=F32)[name]


def switches_of(case):
    """The case's three switches as (fuse_c3k2, fuse_dwpw, fuse_stem): `fuse=False` turns all three off."""
    return tuple(case["fuse"] and case["env"].get(name, "1") != "0" for name in SWITCHES)


def exact_params(seed=SEED, nc=NC):
    """SyntheticParams whose packed bits do not depend on the host.  Two things in the ordinary ones do (measured: the same commit, two hosts, two
    hashes): `normal_` draws BatchNorm shifts and biases through a vectorised log / cos, and the BatchNorm fold takes `torch.sqrt`, which the CPU
    backend hands to a vendor math library -- neither rounds the same way on every CPU.  Here every value is a 16-bit integer of the seeded
    Mersenne generator scaled by a power of two, and a running variance is 1/4, 1 or 4 less the fold's epsilon, so that the square root is taken of
    a power of four; everything else the packing does (add, multiply, divide, convert) is one correctly rounded operation.  Same ranges as
    SyntheticParams otherwise."""
    import torch
    from circuitvision_amd.yolo11 import BN_EPS, SyntheticParams

    class ExactParams(SyntheticParams):
        def get(self, name, shape):
            if name not in self.sd and not name.endswith("num_batches_tracked"):
                r = torch.randint(0, 1 << 16, tuple(shape), generator=self._gen(name)).float() / 65536          # [0, 1) on a 2^-16 grid
                if name.endswith("bn.running_var"):
                    p = torch.tensor([0.25, 1.0, 4.0])[(r * 3).long()]
                    t = p - BN_EPS
                    assert torch.equal(t + BN_EPS, p), name
                elif name.endswith("bn.weight"):
                    t = 0.5 + r
                elif name.endswith("bn.bias") or name.endswith("bn.running_mean"):
                    t = (r - 0.5) * 0.25
                elif name.endswith("weight"):
                    fan_in = shape[1] * shape[2] * shape[3]
                    t = (2 * r - 1) * 2.0 ** -(fan_in.bit_length() // 2)                                        # ~ 1 / sqrt(fan_in)
                    t = t * 4.0 if ".cv3." in name and name.endswith(".2.weight") else t                        # class logits: spread them out
                else:
                    t = (r - 0.5) + (-6.0 if ".cv3." in name else 1.0)                                          # class bias: sparse detections; DFL bias
                self.sd[name] = t
            return super().get(name, shape)

    return ExactParams(seed, nc)


def build_plan(case, cache=None):
    """Yolo11Plan of a case under its switches (GPU).  cache: {(scale, dtype): Yolo11Weights} shared between cases."""
    import torch
    from circuitvision_amd.yolo11 import Yolo11Plan, Yolo11Weights
    from sam2_route_cases import _with_env
    cache = {} if cache is None else cache
    key = (case["scale"], case["dtype"])
    if key not in cache:
        cache[key] = Yolo11Weights(case["scale"], NC, exact_params(), dtype_of(case["dtype"]))
    return _with_env(case["env"], lambda: Yolo11Plan(cache[key], case["B"], case["H"], case["W"], torch.cuda.Stream(), conf=CONF,
                                                     fuse_c3k2=case["fuse"], lanes=case["lanes"]))


def plan_ops(plan):
    """[[label, kind, lane]] of a plan, the fork / join entries with their -1 / -2 marks."""
    return [[op[0], op[1], lane] for op, lane in zip(plan.plan.ops, plan.plan.lanes)]


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def output_hashes(plan):
    out = dict(pred=_sha(plan.pred), det=_sha(plan.det), det_idx=_sha(plan.det_idx), det_count=_sha(plan.det_count))
    out.update({f"feat{i}": _sha(f.tensor()) for i, f in enumerate(plan.feats)})
    return out


def run_hashes(case, cache=None):
    """{"eager": ..., "graph": ...}: the output hashes of a fresh plan on the seeded input after one eager pass, then after one captured replay."""
    import torch
    plan = build_plan(case, cache)
    plan.set_input_nchw(torch.rand(case["B"], 3, case["H"], case["W"], generator=torch.Generator().manual_seed(1)))
    torch.cuda.synchronize()
    plan.plan.run_eager()
    torch.cuda.synchronize()
    out = dict(eager=output_hashes(plan))
    plan.plan.run()
    torch.cuda.synchronize()
    out["graph"] = output_hashes(plan)
    out["detections"] = plan.det_count.tolist()             # per image, so that the file shows the hashed detections are not empty tables
    return out


def weights_record(scale):
    """What Yolo11Weights(scale) pulls and packs, built on the CPU in f32."""
    from circuitvision_amd._lib import F32
    from circuitvision_amd.distributed import packed_tensors
    from circuitvision_amd.yolo11 import Yolo11Weights
    params = exact_params()
    wt = Yolo11Weights(scale, NC, params, F32, device="cpu")
    h = hashlib.sha256()
    for t in packed_tensors(wt.packed):
        h.update(t.contiguous().numpy().tobytes())
    return dict(params=[[k, list(v.shape)] for k, v in params.state_dict().items()], packed=list(wt.packed), sha256=h.hexdigest(),
                param_bytes=wt.param_bytes)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--weights":
        fixture = dict(weights={s: weights_record(s) for s in WEIGHT_SCALES})
    else:
        with open(sys.argv[-1]) as f:                       # the weights part is recorded first, without a GPU
            fixture = json.load(f)
        import torch
        cache, fixture["cases"] = {}, {}
        for case in CASES:
            plan = build_plan(case, cache)
            ops = plan_ops(plan)
            if case["runs"]:
                plan.x_in.t.normal_(generator=torch.Generator(device="cuda").manual_seed(0))
                torch.cuda.synchronize()
                timed = plan.plan.timed_eager(with_kernels=True)
                torch.cuda.synchronize()
                assert [t[0] for t in timed] == [op[0] for op in ops]
                ops = [op + [t[5]] for op, t in zip(ops, timed)]
            rec = dict(ops=ops, act_bytes=plan.act_bytes, param_bytes=plan.wt.param_bytes)
            del plan
            if case["hashed"]:
                rec["hashes"] = run_hashes(case, cache)
                if run_hashes(case, cache) != rec["hashes"]:
                    raise SystemExit(f"{case['id']}: two runs of the same plan gave different output bits; no fixture written")
                if not all(rec["hashes"]["detections"]):
                    raise SystemExit(f"{case['id']}: an image without detections; no fixture written")
            fixture["cases"][case["id"]] = rec
            print(case["id"], len(ops), "ops", flush=True)
    with open(sys.argv[-1], "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
