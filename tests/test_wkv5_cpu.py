"""CPU tier of the WKV5 (RWKV-5, static decay) operator.

* The identity every WKV5 test rests on: WKV5(r,k,v,w,u) == WKV6(r,k,v,broadcast(w),u) and gw5[h][i] = sum_{b,t} gw6[b][t][h*64+i],
  so the pinned fp64 WKV6 oracle checks WKV5.  A literal fp64 restatement of the WKV5 recurrences with an independently derived
  adjoint (tests/wkv5_numpy.py) must equal the oracle used that way.
* The C ABI refuses bad arguments with the header's codes before it touches a device; the wrappers refuse what the kernels
  cannot serve.
* ISA guards on csrc/wkv5_scan.hip compiled for gfx950.
* The time-mix caller's glue with the operator stubbed by the restatement.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import wkv5_numpy as w5
from conftest import max_norm_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_listing                                                  # noqa: E402

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
P = 1                                       # a non-NULL dummy pointer


# ---- the identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay_set", ["ramp", "stress"])
def test_restatement_equals_the_wkv6_oracle_with_broadcast_decay(oracle, decay_set):
    p = w5.problem(2, 7, 2, seed=3, decay_set=decay_set)
    y = w5.forward(p["r"], p["k"], p["v"], p["w"], p["u"])
    g = w5.backward(p["r"], p["k"], p["v"], p["w"], p["u"], p["gy"])
    yo, go = w5.oracle_pair(oracle, **p)
    assert max_norm_err(yo, y) <= 1e-6
    for n in ("gr", "gk", "gv", "gw_b", "gu_b", "gw", "gu"):
        assert max_norm_err(go[n], g[n]) <= 1e-6, n


@pytest.mark.parametrize("T", [1, 2, 3])
def test_gw_is_exactly_zero_up_to_two_tokens(oracle, T):
    """dS_t/dd is 0 for t <= 1 (S_0 = 0, S_1 = k_0 v_0^T), so no token of a row of T <= 2 sees the decay: the reference's gw
    loop (cuda/wkv5_cuda.cu:119-142) is empty there."""
    p = w5.problem(2, T, 2, seed=10 + T)
    g = w5.backward(p["r"], p["k"], p["v"], p["w"], p["u"], p["gy"])
    _, go = w5.oracle_pair(oracle, **p)
    if T <= 2:
        assert not g["gw_b"].any() and not g["gw"].any()
    else:
        assert np.abs(g["gw"]).max() > 1e-3
    assert max_norm_err(go["gw_b"], g["gw_b"]) <= 1e-6
    assert max_norm_err(go["gu_b"], g["gu_b"]) <= 1e-6


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def cuda_fwd(B=1, T=4, C=64, H=1, r=P, k=P, v=P, w=P, u=P, y=P):
    return (B, T, C, H, r, k, v, w, u, y, None)


def cuda_bwd(B=1, T=4, C=64, H=1, r=P, k=P, v=P, w=P, ew=P, u=P, gy=P, gr=P, gk=P, gv=P, gw=P, gu=P):
    return (B, T, C, H, r, k, v, w, ew, u, gy, gr, gk, gv, gw, gu, None)


def ex_fwd(flags=1, **kw):
    return cuda_fwd(**kw)[:-1] + (flags, None)


def ex_bwd(flags=1, **kw):
    return cuda_bwd(**kw)[:-1] + (flags, None)


ENTRY = {"wkv5_cuda_forward": (cuda_fwd, ["r", "k", "v", "w", "u", "y"]),
         "wkv5_cuda_backward": (cuda_bwd, ["r", "k", "v", "w", "ew", "u", "gy", "gr", "gk", "gv"]),
         "wkv5_forward_ex": (ex_fwd, ["r", "k", "v", "w", "u", "y"]),
         "wkv5_backward_ex": (ex_bwd, ["r", "k", "v", "w", "u", "gy", "gr", "gk", "gv"])}


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_entry_points_reject_bad_arguments_without_a_device(lib, name):
    fn, (args, required) = getattr(lib, name), ENTRY[name]
    for kw in ({"B": 0}, {"T": 0}, {"B": -1}, {"T": -3}, {"C": 0, "H": 0}, {"H": 0}, {"H": -1}):
        assert fn(*args(**kw)) == EINVAL, kw
    for C, H in ((128, 1), (64, 2), (96, 1), (2048, 31)):               # C != 64 H
        assert fn(*args(C=C, H=H)) == EINVAL, (C, H)
    for p in required:
        assert fn(*args(**{p: None})) == ENULL, p


def test_extended_entry_points_reject_unknown_flags_and_a_missing_ew(lib):
    for flags in (4, 32, 64, 256, 1 << 20):                             # S0_PER_BATCH, CKPT_VALID, BI_KEEP_CKPT, unknown bits
        assert lib.wkv5_forward_ex(*ex_fwd(flags=flags | 1)) == EUNSUPPORTED, flags
        assert lib.wkv5_backward_ex(*ex_bwd(flags=flags | 1)) == EUNSUPPORTED, flags
    # without WKV6_W_RAW the decay is given as fp32 eew and gw = ew (.) eew (.) dL/d eew needs ew
    assert lib.wkv5_backward_ex(*ex_bwd(flags=0, ew=None)) == ENULL


def test_library_and_header_agree_on_the_wkv5_symbols(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    for name in ENTRY:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES_WKV5 and getattr(lib, name) is not None


# ---- wrappers -------------------------------------------------------------------------------------------------------------
def test_wkv5_wrappers_refuse_cpu_and_non_bf16_tensors():
    from rwkv_lm_ext_amd import wkv6_op
    from rwkv_lm_ext_amd.wkv import WKV_5, RUN_CUDA_RWKV5
    bf = torch.bfloat16
    B, T, H = 1, 4, 1
    C = 64 * H
    r = torch.zeros(B, T, C, dtype=bf)
    w = torch.zeros(H, 64, dtype=bf)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        WKV_5.apply(B, T, C, H, r, r, r, w, w)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        RUN_CUDA_RWKV5(B, T, C, H, r, r, r, w, w)
    for bad in range(5):                                                # any one of r, k, v, w, u not bf16
        args = [r, r, r, w, w]
        args[bad] = args[bad].float()
        with pytest.raises(AssertionError):
            WKV_5.apply(B, T, C, H, *args)
    with pytest.raises(AssertionError):
        WKV_5.apply(B, T, C, H, r.transpose(1, 2).contiguous().transpose(1, 2), r, r, w, w)     # not contiguous
    y = torch.zeros(B, T, C, dtype=bf)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        wkv6_op.wkv5.forward(B, T, C, H, r, r, r, w.float(), w, y)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        wkv6_op.wkv5_forward_ex(r, r, r, w, w, H)
    assert hasattr(torch.ops.wkv5, "forward") and hasattr(torch.ops.wkv5, "backward")


# ---- ISA ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wkv5_asm():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    return isa_listing.listing("wkv5_scan.hip")


BF16_KERNELS = ("wkv5_fwd_kernelItE", "wkv5_bwd_a_kernelItE", "wkv5_bwd_g_kernelItE")       # t = unsigned short = raw bf16


def test_no_spill_and_no_scratch_in_the_wkv5_kernels(wkv5_asm):
    spills, private, vgprs = (isa_listing.kernel_meta(wkv5_asm, k) for k in ("vgpr_spill_count", "private_segment_fixed_size", "vgpr_count"))
    for want in BF16_KERNELS:
        hit = [n for n in spills if want in n]
        assert len(hit) == 1, (want, list(spills))
        assert spills[hit[0]] == 0 and private[hit[0]] == 0, (hit[0], spills[hit[0]], private[hit[0]])
        assert vgprs[hit[0]] <= 128, (hit[0], vgprs[hit[0]])            # 512 threads: two workgroups per CU stay possible
    assert all(v == 0 for v in spills.values()) and all(v == 0 for v in private.values())       # the fp32 flavour too
    assert not re.search(r"^\s+scratch_", wkv5_asm, re.M)


def test_no_decay_stream_and_no_exp_inside_the_token_loops(wkv5_asm):
    """The loops of the forward read three streams from memory (r, k, v) and those of the backward passes four (r, k, v, gy):
    a decay stream would be one more load per batch of tokens, and a per-token decay an exponential inside the loop."""
    seen = 0
    for name, fn in isa_listing.functions(wkv5_asm).items():
        if not any(k in name for k in BF16_KERNELS):
            continue
        seen += 1
        loads, stores = 0, 0
        for line in (x for _, c, lines in isa_listing.blocks(fn) if "Loop" in c for x in lines):
            op = line.strip().split(" ")[0] if line.strip() else ""
            assert not op.startswith("v_exp"), (name, line.strip())
            assert not op.startswith("s_load") and not op.startswith("s_buffer_load"), (name, line.strip())
            loads += bool(re.match(r"(global|buffer|flat)_load", op))
            stores += bool(re.match(r"(global|buffer|flat)_store", op))
        fwd = "fwd" in name
        assert loads == (3 if fwd else 4), (name, loads)
        assert stores == (2 if "bwd_g" in name else 1), (name, stores)
    assert seen == 3


def test_wkv5_sources_are_built_into_the_library():
    from rwkv_lm_ext_amd import _build
    assert "wkv5_scan.hip" in _build.SOURCES and "wkv5_scan.h" in _build.HEADERS


# ---- the time-mix caller --------------------------------------------------------------------------------------------------
REFERENCE_KEYS = ["time_mix_k", "time_mix_v", "time_mix_r", "time_mix_g", "time_decay", "time_faaaa", "receptance.weight",
                  "key.weight", "value.weight", "output.weight", "gate.weight", "ln_x.weight", "ln_x.bias"]


def _tmix(n_embd=128, seed=0):
    from rwkv_lm_ext_amd.callers import RWKV_Tmix_x052
    torch.manual_seed(seed)
    tm = RWKV_Tmix_x052(n_embd, n_embd, wkv=w5.numpy_wkv5).init_like_reference(layer_id=1, n_layer=4)
    with torch.no_grad():
        for lin in (tm.receptance, tm.key, tm.value, tm.gate, tm.output):
            lin.weight.normal_(0, n_embd ** -0.5)
        tm.ln_x.weight.uniform_(0.5, 1.5)
        tm.ln_x.bias.normal_(0, 0.1)
    return tm


def test_tmix_x052_has_the_reference_state_dict_and_its_glue():
    """The module against the block's formulas written out (src/model.py:340-374) in fp64, the operator being the restatement on
    both sides: token shift with a zero row in front, four static lerps, projections, GroupNorm(y / 8) * silu(gate), output."""
    tm = _tmix().double()
    assert sorted(tm.state_dict()) == sorted(REFERENCE_KEYS)
    assert tuple(tm.time_decay.shape) == (2, 64) and tuple(tm.time_mix_k.shape) == (1, 1, 128)
    assert float(tm.time_decay.min()) == -6.0 and abs(float(tm.time_decay.max()) + 1.0) < 1e-12         # the ramp's ends
    B, T, C, H = 2, 9, 128, 2
    x = torch.randn(B, T, C, dtype=torch.float64)
    out = tm(x)
    sd = {k: v.detach().numpy() for k, v in tm.state_dict().items()}
    xn = x.numpy()
    xx = np.concatenate([np.zeros((B, 1, C)), xn[:, :-1]], 1)
    mix = lambda m: xn * sd["time_mix_" + m] + xx * (1 - sd["time_mix_" + m])
    r, k, v = mix("r") @ sd["receptance.weight"].T, mix("k") @ sd["key.weight"].T, mix("v") @ sd["value.weight"].T
    gate = mix("g") @ sd["gate.weight"].T
    gate = gate / (1 + np.exp(-gate))
    y = w5.forward(r, k, v, sd["time_decay"], sd["time_faaaa"]).reshape(B * T, H, 64) / 8
    yn = (y - y.mean(-1, keepdims=True)) / np.sqrt(y.var(-1, keepdims=True) + 1e-5)
    yn = yn.reshape(B, T, C) * sd["ln_x.weight"] + sd["ln_x.bias"]
    want = (yn * gate) @ sd["output.weight"].T
    assert max_norm_err(out.detach().numpy(), want) <= 1e-10
    # the first token of every row sees a zero predecessor: changing the LAST token changes nothing before it
    x2 = x.clone()
    x2[:, -1] += 1.0
    assert torch.equal(tm(x2)[:, :-1], out[:, :-1])


def test_tmix_x052_backward_through_the_restatement_matches_finite_differences():
    tm = _tmix(seed=1).double()
    x = torch.randn(1, 5, 128, dtype=torch.float64, requires_grad=True)
    probe = torch.randn(1, 5, 128, dtype=torch.float64)
    (tm(x) * probe).sum().backward()
    g = tm.time_decay.grad.clone()
    eps = 1e-6
    for (h, i) in ((0, 3), (1, 40)):
        with torch.no_grad():
            tm.time_decay[h, i] += eps
            up = float((tm(x) * probe).sum())
            tm.time_decay[h, i] -= 2 * eps
            dn = float((tm(x) * probe).sum())
            tm.time_decay[h, i] += eps
        fd = (up - dn) / (2 * eps)
        assert abs(fd - float(g[h, i])) <= 1e-6 * max(1.0, abs(fd)), (h, i, fd, float(g[h, i]))
