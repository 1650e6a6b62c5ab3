"""CPU guard of the proj + MLP launch (csrc/proj_mlp.hpp, the proj form of cvmi_hiera_mlp): every instance the header can launch has a
case row; the packed stream gives back its matrices; the documented index formulas, evaluated in fp64 on the unpacked fragments, are the plain
formula; what the host refuses; and the shape of the compiled kernels (MFMA hazards, MFMA count, registers, spills)."""
import ctypes
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, PackedProjMlp, proj_mlp_k_order
from proj_mlp_cases import PROJ_MLP_ROWS, PROJ_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuitvision_amd", "csrc")
HEADER = os.path.join(CSRC, "proj_mlp.hpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libcvmi355.so not built")


def header_instances(text):
    return ["proj_mlp_kernel<%s, %s>" % m for m in re.findall(r"return launch_proj_mlp<(\d+), (\d)>\(", text)]


def test_every_instance_the_header_launches_has_a_row():
    text = open(HEADER).read()
    assert 'cvmi_note_kernel("proj_mlp_kernel<%d, %d>", C, VAR);' in text
    assert "getenv" not in text
    inst = header_instances(text)
    assert inst and len(inst) == len(set(inst)), inst       # the parser still finds the call sites
    tags = {r["expect"] for r in PROJ_MLP_ROWS}
    assert set(inst) == tags, (inst, tags)
    probe = text + "\n  return launch_proj_mlp<288, 0>(d, s);\n"
    assert set(header_instances(probe)) - tags == {"proj_mlp_kernel<288, 0>"}
    for r in PROJ_MLP_ROWS:
        assert r["expect"] == "proj_mlp_kernel<%d, %d>" % (r["C"], 1 if r["C"] == 144 else 2), r["id"]
    today = {(144, 5), (144, 1000), (144, 128 * 3 + 37), (288, 5), (288, 777)}
    assert {(r["C"], r["rows"]) for r in PROJ_MLP_ROWS} >= today and {(r["C"], r["rows"]) for r in PROJ_ROWS} >= today
    assert len(PROJ_MLP_ROWS) == len({r["id"] for r in PROJ_MLP_ROWS}) and {r["expect"] for r in PROJ_ROWS} == tags


def _weights(C_, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(wp=torch.randn(C_, C_, generator=g) / C_ ** 0.5, bp=torch.randn(C_, generator=g) * 0.3,
                w1=torch.randn(4 * C_, C_, generator=g) / C_ ** 0.5, b1=torch.randn(4 * C_, generator=g) * 0.3,
                w2=torch.randn(C_, 4 * C_, generator=g) / (4 * C_) ** 0.5, b2=torch.randn(C_, generator=g) * 0.3)


@needs_lib
@pytest.mark.parametrize("C_", [144, 288])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_unpack_gives_back_the_matrices(dtype, C_):
    td = TORCH_DTYPE[dtype]
    wt = _weights(C_)
    pm = PackedProjMlp(**wt, device="cpu", dtype=dtype)
    assert pm.w.numel() * 2 == _lib.load().cvmi_hiera_mlp_proj_packed_bytes(C_) == ((C_ + 31) // 32) * (C_ // 16) * 1024 + _lib.load().cvmi_hiera_mlp_packed_bytes(C_)
    assert torch.equal(pm.bias, torch.cat((wt["bp"], wt["b2"])))
    u = pm.unpack()
    for k in ("wp", "w1", "w2"):
        assert torch.equal(u[k], wt[k].to(td).float()), k
    assert torch.equal(u["bp"], wt["bp"]) and torch.equal(u["b2"], wt["b2"])
    b_hi = wt["b1"].to(td).float()
    assert torch.equal(u["b1"], b_hi + (wt["b1"] - b_hi).to(td).float())
    order = proj_mlp_k_order(C_)
    assert sorted(order.tolist()) == list(range(C_))
    k = torch.arange(16)
    assert torch.equal(order[:16], 8 * ((k & 7) >> 2) + 4 * (k >> 3) + (k & 3)) and torch.equal(order[16:32], order[:16] + 16)


@needs_lib
@pytest.mark.parametrize("C_", [144, 288])
def test_fp64_evaluation_from_the_fragments_is_the_plain_formula(C_):
    """The kernel's arithmetic restated in fp64 on the packed stream itself, with the index formulas of include/cvmi355.h / proj_mlp.hpp: lane
    (token, half lh) of the proj accumulator holds channel 32 t + 8 g + 4 lh + e in register 4 g + e of tile t; registers 8 h .. 8 h + 7 are
    fc1's B fragment of k-step 2 t + h (element i of lane half lh = k index 8 lh + i); fc2's k order is cvmi_hiera_mlp's."""
    wt = _weights(C_)
    pm = PackedProjMlp(**wt, device="cpu", dtype=F16)
    nt, ks, ks1, nch = (C_ + 31) // 32, C_ // 16, C_ // 16 + 1, 4 * C_ // 32
    w = pm.w.double().reshape(-1)
    P = w[:nt * ks * 512].view(nt, ks, 64, 8)                         # P(t, s)[l][e]
    ch = w[nt * ks * 512:].view(nch, ks1 + 2 * nt, 64, 8)             # chunk j: F1(j, s), then F2(j, t, s2)
    g = torch.Generator().manual_seed(C_)
    T = 3
    x = torch.randn(T, C_, generator=g, dtype=torch.float64)
    ao = torch.randn(T, C_, generator=g).half().double()
    gam, bet = torch.rand(C_, generator=g, dtype=torch.float64) + 0.5, torch.randn(C_, generator=g, dtype=torch.float64)
    bias = pm.bias.double()
    bp, b2 = bias[:C_], bias[C_:]
    # proj: acc[t][r] over k-steps; A lane l = (r = l & 31, h = l >> 5) holds k = 8 h + e; B lane (token, lh) holds ao[16 s + 8 lh + e]
    x1 = torch.zeros(T, nt * 32, dtype=torch.float64)
    for t in range(nt):
        for s in range(ks):
            A = P[t, s].view(2, 32, 8).permute(1, 0, 2).reshape(32, 16)            # [row r][k]
            x1[:, 32 * t:32 * t + 32] += ao[:, 16 * s:16 * s + 16] @ A.t()
    assert not x1[:, C_:].any()
    x1 = x[:, :C_] + (x1[:, :C_] + bp)
    mean, var = x1.mean(1, keepdim=True), x1.var(1, unbiased=False, keepdim=True)
    xn = (x1 - mean) / torch.sqrt(var + 1e-6) * gam + bet
    # fc1's B fragments: k-step 2 t + h, k index kappa = 8 lh + i  <-  channel 32 t + 16 h + 8 (i >> 2) + 4 lh + (i & 3)
    Bf = torch.zeros(T, ks1, 16, dtype=torch.float64)
    for k in range(ks):
        t, h = k >> 1, k & 1
        for lh in range(2):
            for i in range(8):
                Bf[:, k, 8 * lh + i] = xn[:, 32 * t + 16 * h + 8 * (i >> 2) + 4 * lh + (i & 3)]
    Bf[:, ks, 0] = Bf[:, ks, 1] = 1.0                                  # the bias step's constant-1 columns
    y = torch.zeros(T, nt * 32, dtype=torch.float64)
    hid_all = torch.zeros(T, 4 * C_, dtype=torch.float64)
    for j in range(nch):
        hacc = torch.zeros(T, 32, dtype=torch.float64)
        for s in range(ks1):
            A = ch[j, s].view(2, 32, 8).permute(1, 0, 2).reshape(32, 16)
            hacc += Bf[:, s] @ A.t()
        hid = torch.nn.functional.gelu(hacc)
        hid_all[:, 32 * j:32 * j + 32] = hid
        # fc2's B: lane (token, lh), element i of k-half s2 = hidden unit 16 s2 + 8 (i >> 2) + 4 lh + (i & 3) (accumulator register 8 s2 + i)
        for t in range(nt):
            for s2 in range(2):
                A = ch[j, ks1 + 2 * t + s2].view(2, 32, 8).permute(1, 0, 2).reshape(32, 16)
                Bk = torch.stack([hid[:, 16 * s2 + 8 * (i >> 2) + 4 * lh + (i & 3)] for lh in range(2) for i in range(8)], 1)
                y[:, 32 * t:32 * t + 32] += Bk @ A.t()
    got = x1 + y[:, :C_] + b2
    u = pm.unpack()
    r1 = x + ao @ u["wp"].double().t() + bp
    rn = torch.nn.functional.layer_norm(r1, (C_,), gam, bet, 1e-6)
    ref = r1 + torch.nn.functional.gelu(rn @ u["w1"].double().t() + u["b1"].double()) @ u["w2"].double().t() + b2
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


@needs_lib
def test_the_host_refuses_what_is_not_built():
    """Each refusal happens on the host before anything is launched (no GPU needed); the pointers are never dereferenced."""
    lib = _lib.load()
    A = 1 << 20                                              # an aligned, never-dereferenced address

    def call(C_=144, dtype=F16, proj="good", **kw):
        d = _lib.MlpDesc(x=A, x_ld=C_, gamma=A, beta=A, eps=1e-6, w_packed=A, b2=A, rows=256, C=C_, dtype=dtype)
        for k, v in ({**dict(ao=A, bp=A, ao_ld=C_), **kw} if proj == "good" else {}).items():
            setattr(d, k, v)
        return lib.cvmi_hiera_mlp(ctypes.byref(d), None)

    def refused(match, **kw):
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_lib.CvmiError, match=match):
            _lib.check(rc, "proj_mlp")

    for dtype in (F16, BF16):
        refused("not built", dtype=dtype, C_=576)
        refused("not built", dtype=dtype, C_=160)
        refused("needs ao", dtype=dtype, ao=None)
        refused("needs ao", dtype=dtype, w_packed=None)
        refused("needs ao", dtype=dtype, bp=None)
        refused("not aligned", dtype=dtype, ao=A + 8)
        refused("not aligned", dtype=dtype, w_packed=A + 2)
        refused("not aligned", dtype=dtype, bp=A + 4)
        refused("ao_ld", dtype=dtype, ao_ld=136)
        refused("ao_ld", dtype=dtype, ao_ld=148)
        refused("ao_ld", dtype=dtype, C_=288, ao_ld=144)
    refused("dtype must be", dtype=F32)
    # ao = bp = NULL: the plain form -- its own refusals answer (nothing is launched: C = 576 is not built)
    rc = call(C_=576, proj=None)
    assert rc != 0
    with pytest.raises(_lib.CvmiError, match=r"hiera_mlp: C=576 is not built"):
        _lib.check(rc, "hiera_mlp")
    assert lib.cvmi_version() >= 129                          # 129: cvmi_mlp_desc (127: the proj form)


def _metadata(asm, name):
    """(vgpr_count, agpr_count, vgpr_spill_count, private_segment_fixed_size) of the kernel whose symbol contains `name`, from the code
    object's metadata notes in the device assembly."""
    blocks = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])
    for b in blocks[1:]:
        b = ".agpr_count:" + b
        if re.search(r"\.name:\s+\S*" + re.escape(name), b):
            f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, b).group(1))
            return f("vgpr_count"), f("agpr_count"), f("vgpr_spill_count"), f("private_segment_fixed_size")
    raise KeyError(name)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("extra", [(), ("-DCVMI_OPERAND_BF16",)], ids=["f16", "bf16"])
def test_compiled_kernels_keep_their_wait_states_and_registers(extra):
    """proj_mlp_kernel<288, 2> issues its MFMAs from inline asm like hiera_mlp_kernel<288, 2>: tools/check_asm_mfma.py's check() must find no
    hazard, and the count the source's structure implies: the pipelined loop's 148 (19 of fc1(0) + 35 iterations of 37 + 18 of the last fc2;
    tests/test_oracle_cpu.py) + the proj phase's NT * KS = 9 * 18 = 162, fully unrolled  = 310.  <144, 1> must fit two workgroups per CU
    (<= 256 registers); neither instance may spill or use scratch."""
    spec = importlib.util.spec_from_file_location("check_asm_mfma", os.path.join(ROOT, "tools", "check_asm_mfma.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    asm = m.device_asm("hiera_mlp.hip", extra)
    n, bad = m.check(m.kernel_body(asm, "proj_mlp_kernelILi288ELi2EE"))
    assert n == 148 + 9 * 18 and bad == [], (n, bad[:3])
    n, bad = m.check(m.kernel_body(asm, m.KERNEL))               # ... and the kernel whose pieces it shares is what it was
    assert n == 148 and bad == [], (n, bad[:3])
    # (.vgpr_count is the unified register file's allocation on this target: VGPRs and AGPRs together)
    v, a, spill, priv = _metadata(asm, "proj_mlp_kernelILi144ELi1EE")
    assert v <= 256 and a <= v and spill == 0 and priv == 0, (v, a, spill, priv)
    v, a, spill, priv = _metadata(asm, "proj_mlp_kernelILi288ELi2EE")
    assert v <= 512 and a <= v and spill == 0 and priv == 0, (v, a, spill, priv)
