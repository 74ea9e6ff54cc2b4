"""The chunked kernels' split sites (csrc/wkv6_chunk.h: the bf16 hi | lo split with its residual formed by one MFMA per wave) at the smallest
shapes that reach every one of them: B = 1, H = 2 and T in {1, 16, 33, 64, 97, 130} -- a lone token, one block, an odd stage with a one-token
tail, one full checkpoint pair, a pair + an odd stage + a tail, two pairs + a two-token tail -- forward + backward in bf16 I/O, with both decay
kinds of test_wkv6_gpu.py (init and stress), in both launch shapes: two workgroups per (batch, head), which is what the library picks for so
few pairs (the producers of both workgroups, the row waves' own copy of G, the column waves' own score tiles), and one workgroup per pair as
at the benched shapes (the shared dA / score tiles, the published G operand).

Reference: the fp64 oracle, at the suite's bf16 contract (test_wkv6_gpu.py: check) -- never the kernels themselves."""
import pytest
import torch

from conftest import max_norm_err
from test_wkv6_gpu import PART_TOL, check, dev, host, rand_inputs

pytestmark = pytest.mark.gpu

B, H = 1, 2
LENGTHS = [1, 16, 33, 64, 97, 130]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    assert wkv6_op.selftest() == 0
    return wkv6_op


@pytest.fixture(scope="module")
def cases(oracle):
    """(T, kind) -> inputs and the oracle's outputs, computed once and shared by both launch shapes."""
    out = {}
    for T in LENGTHS:
        for kind in ("init", "stress"):
            x = rand_inputs(7000 + T + (1000 if kind == "init" else 0), B, T, H, kind)
            out[T, kind] = (x, oracle.forward(*x[:5]), oracle.backward(*x))
    return out


@pytest.mark.parametrize("split", [None, 0], ids=["two_workgroups", "one_workgroup"])
@pytest.mark.parametrize("kind", ["init", "stress"])
@pytest.mark.parametrize("T", LENGTHS)
def test_split_sites_against_the_oracle(ops, cases, T, kind, split):
    bf = torch.bfloat16
    (r, k, v, w, u, gy), yo, og = cases[T, kind]
    d = [dev(x, bf) for x in (r, k, v, w, u, gy)]
    with ops.dispatch(split=split):
        ck = ops.new_checkpoint(B, T, H * 64, H, "cuda")
        check(ops.forward_ex(*d[:5], H, ckpt=ck), yo, bf, f"T={T} {kind} y")
        gr, gk, gv, gw, gu, _ = ops.backward_ex(*d, H, ckpt=ck)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        check(t, og[n], bf, f"T={T} {kind} {n}")
    assert max_norm_err(host(gu), og["gu_b"]) <= PART_TOL
