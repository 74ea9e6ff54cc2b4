"""CPU tier of the fused mix kernels (csrc/wkv6_mix.hip): every entry point refuses bad arguments with its documented code before
it launches anything, the Python wrappers refuse what the kernels cannot serve, and the device-side bf16 metric of the GPU tests
(oracle.contract.bf16_report_torch) is the suite's numpy bf16_report.

The pointers passed here are dummies (1): every call must return from its argument checks, as in
test_oracle_cpu.test_abi_rejects_bad_arguments_without_launching."""
import numpy as np
import pytest
import torch

from conftest import bf16_report
from oracle.contract import bf16_report_torch

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
P = 1                                       # a non-NULL dummy pointer


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


# ---- argument lists of each entry point, valid except where a test changes them ---------------------------------------------
def lerp_fwd(B=1, T=4, C=64, NS=1, x=P, shifted0=None, m=None, maa=P, out=P):
    return (B, T, C, NS, x, shifted0, m, maa, out, None)


def lerp_rev_fwd(B=1, T=4, C=64, NS=1, x=P, shifted0=None, m=None, maa=P, rev_n=P, out=P):
    return (B, T, C, NS, x, shifted0, m, maa, rev_n, out, None)


def lerp_bwd(B=1, T=4, C=64, NS=1, x=P, shifted0=None, m=None, maa=P, dout=P, dx=P, dm=None, part=P, nparts=1):
    return (B, T, C, NS, x, shifted0, m, maa, dout, dx, dm, part, nparts, None)


def lerp_rev_bwd(B=1, T=4, C=64, NS=1, x=P, shifted0=None, m=None, maa=P, rev_n=P, dout=P, dx=P, dm=None, part=P, nparts=1):
    return (B, T, C, NS, x, shifted0, m, maa, rev_n, dout, dx, dm, part, nparts, None)


def gn_fwd(rows=4, C=64, H=1, y=P, g=P, gamma=P, beta=P, eps=1e-5, out=P, stats=None):
    return (rows, C, H, y, g, gamma, beta, eps, out, stats, None)


def gn_bwd(rows=4, C=64, H=1, y=P, g=P, gamma=P, beta=P, stats=P, dout=P, dy=P, dg=P, pg=P, pb=P, nparts=1):
    return (rows, C, H, y, g, gamma, beta, stats, dout, dy, dg, pg, pb, nparts, None)


LERP = {"wkv6_ddlerp_forward": lerp_fwd, "wkv6_ddlerp_rev_forward": lerp_rev_fwd,
        "wkv6_ddlerp_backward": lerp_bwd, "wkv6_ddlerp_rev_backward": lerp_rev_bwd}
GN = {"wkv6_gn_gate_forward": gn_fwd, "wkv6_gn_gate_backward": gn_bwd}
FLAT = {"wkv6_sqrelu_forward": ("x", "out"), "wkv6_sqrelu_backward": ("x", "dout", "dx"),
        "wkv6_sigmul_forward": ("r", "kv", "out"), "wkv6_sigmul_backward": ("r", "kv", "dout", "dr", "dkv")}


def flat(name, n=64, null=None):
    return (n,) + tuple(None if p == null else P for p in FLAT[name]) + (None,)


@pytest.mark.parametrize("name", sorted(LERP))
def test_ddlerp_entry_points_reject_bad_shapes(lib, name):
    fn, args = getattr(lib, name), LERP[name]
    for kw in ({"B": 0}, {"T": 0}, {"B": -1}, {"T": -5}):
        assert fn(*args(**kw)) == EINVAL, kw
    for C in (0, 32, 96, 4160, -64):                # multiples of 64 in [64, 4096] only (C / 4 threads per row)
        assert fn(*args(C=C)) == EINVAL, C
    if "backward" in name:
        for nparts in (0, -1):
            assert fn(*args(nparts=nparts)) == EINVAL, nparts
    assert fn(*args(B=1 << 14, T=1 << 14, C=4096)) == EUNSUPPORTED      # B T C >= 2^40 token-channels


@pytest.mark.parametrize("name", sorted(LERP))
def test_ddlerp_entry_points_reject_unsupported_instantiations(lib, name):
    """(NS, m) must be one of (1, NULL), (1, m), (5, m), (2, NULL); m given in the backward needs dm."""
    fn, args = getattr(lib, name), LERP[name]
    bwd = "backward" in name
    for NS, m in ((2, P), (3, None), (5, None), (4, P), (0, None), (6, P)):
        kw = dict(NS=NS, m=m) | ({"dm": P} if bwd and m else {})
        assert fn(*args(**kw)) == EUNSUPPORTED, (NS, m)


@pytest.mark.parametrize("name", sorted(LERP))
def test_ddlerp_entry_points_reject_null_pointers(lib, name):
    fn, args = getattr(lib, name), LERP[name]
    required = ["x", "maa", "out"] if "forward" in name else ["x", "maa", "dout", "dx", "part"]
    base = dict(NS=5, m=P) | ({"dm": P} if "backward" in name else {})
    for p in required:
        assert fn(*args(**(base | {p: None}))) == ENULL, p
    if "backward" in name:
        assert fn(*args(**(base | {"dm": None}))) == ENULL          # m given, dm missing


@pytest.mark.parametrize("name", sorted(GN))
def test_gn_gate_entry_points_reject_bad_arguments(lib, name):
    fn, args = getattr(lib, name), GN[name]
    for rows in (0, -1):
        assert fn(*args(rows=rows)) == EINVAL, rows
    for C in (0, 32, 96, 4160):
        assert fn(*args(C=C, H=max(C // 64, 1))) == EINVAL, C
    for C, H in ((128, 1), (128, 3), (64, 0), (4096, 32)):          # H * 64 != C
        assert fn(*args(C=C, H=H)) == EINVAL, (C, H)
    if name == "wkv6_gn_gate_backward":
        for nparts in (0, -3):
            assert fn(*args(nparts=nparts)) == EINVAL, nparts
    assert fn(*args(rows=1 << 28, C=4096, H=64)) == EUNSUPPORTED
    assert fn(*args(rows=1 << 34, C=64, H=1)) == EUNSUPPORTED
    required = (["y", "g", "gamma", "beta", "out"] if name == "wkv6_gn_gate_forward" else
                ["y", "g", "gamma", "beta", "stats", "dout", "dy", "dg", "pg", "pb"])
    for p in required:
        assert fn(*args(**{p: None})) == ENULL, p


@pytest.mark.parametrize("name", sorted(FLAT))
def test_flat_entry_points_reject_bad_arguments(lib, name):
    fn = getattr(lib, name)
    for n in (0, 4, 12, -8, 7):                     # a positive multiple of 8 elements
        assert fn(*flat(name, n=n)) == EINVAL, n
    for p in FLAT[name]:
        assert fn(*flat(name, null=p)) == ENULL, p


def test_wrappers_refuse_cpu_and_non_bf16_tensors():
    from rwkv_lm_ext_amd import mix_op
    x = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    maa = torch.zeros(1, 64, dtype=torch.bfloat16)
    y = torch.zeros(8, 64, dtype=torch.bfloat16)
    gam = torch.ones(64, dtype=torch.bfloat16)
    for call in (lambda: mix_op.ddlerp(x, maa), lambda: mix_op.ddlerp(x.float(), maa), lambda: mix_op.ddlerp(x, maa.half()),
                 lambda: mix_op.sqrelu(x), lambda: mix_op.sqrelu(x.float()), lambda: mix_op.sigmoid_mul(x, x),
                 lambda: mix_op.gn_gate_forward(y, y, gam, gam, 1, 1e-5), lambda: mix_op.group_norm_gate(y, y, gam, gam, 1, 1e-5),
                 lambda: mix_op.gn_gate_backward(y, y, gam, gam, torch.zeros(8, 1, 2), y, 1)):
        with pytest.raises(RuntimeError, match="bf16 GPU tensor"):
            call()
    with pytest.raises(RuntimeError, match="bf16 GPU tensor"):
        mix_op._require(np.zeros(8), "x")
    # fusable: bf16 GPU tensors whose element count is a multiple of 8 (the GPU side is in test_mix_kernels_gpu.py)
    assert not mix_op.fusable(x)
    assert not mix_op.fusable(x.float())
    assert not mix_op.fusable(np.zeros(8, np.float32))


def _bits_to_f32(u16):
    return (np.asarray(u16, np.uint32) << 16).view(np.float32)


def test_device_bf16_metric_equals_the_numpy_contract():
    """bf16_report_torch returns the numbers of conftest.bf16_report: random references, exact ties between two bf16 values
    (the RNE tie break), zeros, references below the floors, outputs off by whole ulps."""
    rng = np.random.default_rng(5)
    for case in range(12):
        n = int(rng.integers(1, 3000))
        ref = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4)
        k = rng.integers(0, n, size=n // 4)
        hi = np.float32(ref[k]).view(np.uint32) & np.uint32(0xFFFF0000)
        ref[k] = (hi | np.uint32(0x8000)).view(np.float32)            # exactly between two bf16 values
        ref[rng.integers(0, n, size=n // 8)] = 0.0
        ref[rng.integers(0, n, size=n // 8)] *= 1e-6                   # under the 1 % floor
        if case == 0:
            ref[:] = 0.0                                              # all-zero reference: both floors at 1e-3
        if case == 1:
            ref = np.abs(ref)
        want = np.float32(ref).view(np.uint32)
        want = ((want.astype(np.uint64) + 0x7FFF + ((want >> 16) & 1)) >> 16).astype(np.uint16)
        bits = want.astype(np.int64) + rng.choice([0, 0, 0, 1, -1, 2], size=n) * (case % 3 != 0)
        bits[want == 0] = 0
        out = _bits_to_f32(np.clip(bits, 0, 0xFFFF).astype(np.uint16))
        out[ref == 0] = 0.0
        ref_t = torch.from_numpy(ref)
        out_t = torch.from_numpy(out.copy()).to(torch.bfloat16)
        assert torch.equal(out_t.float(), torch.from_numpy(out))      # out holds bf16 values
        for floor in (1e-3, 0.1):
            a = bf16_report(out, ref, floor)
            b = bf16_report_torch(out_t, ref_t, floor)
            assert a[1] == b[1], (case, a, b)
            assert np.allclose(a[0], b[0], rtol=1e-12, atol=0) and np.allclose(a[2], b[2], rtol=1e-12, atol=0), (case, a, b)
    # the tie rule itself: 1 + 2^-8 lies between 1 and 1 + 2^-7 and rounds to the even 1.0; 1 + 3 * 2^-8 rounds up
    ref = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert bf16_report_torch(torch.tensor([1.0, 1 + 2 * 2.0 ** -7]), ref)[1] == 0.0
    assert bf16_report_torch(torch.tensor([1 + 2.0 ** -7, 1 + 2 * 2.0 ** -7]), ref)[1] == 0.5
