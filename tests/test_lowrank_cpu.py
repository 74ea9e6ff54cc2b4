"""CPU tier of the fused low-rank time-mix inputs (callers.Tmix_x060.fuse_lowrank, mix_op.tmix_inputs, mix_op.decay_lowrank).

(a) The restatement of tests/lowrank_common.py, with its roundings switched off, is the formula of Tmix_x060.jit_func: on fp32 CPU tensors
    the two agree to 1e-5 of the largest value, dense with a `shifted` stream and packed with carried tokens.  This pins what the GPU
    tests compare the kernels with to the module.
(b) The routing of `fuse_lowrank`: off by default; when on, the two calls are taken on the fused path where nothing requires a gradient
    and rev_n is None, with the weights in nn.Linear layout, and skipped under grad, with rev_n, on fp32 and on the CPU.
(c) The transposed copies are kept on the module and rebuilt after an in-place update or a replaced parameter tensor."""
import pytest
import torch
import torch.nn.functional as F

import lowrank_common as lc

C, D, DD = 128, 32, 64


def module(p, dtype):
    from rwkv_lm_ext_amd.callers import Tmix_x060
    m = Tmix_x060(C, C)
    with torch.no_grad():
        m.time_maa_x.copy_(p["maa_x"].view(1, 1, C))
        for i, n in enumerate("wkvrg"):
            getattr(m, "time_maa_" + n).copy_(p["maa5"][i].view(1, 1, C))
        m.time_maa_w1.copy_(p["W1"])
        m.time_maa_w2.copy_(p["W2"])
        m.time_decay.copy_(p["time_decay"].view(1, 1, C))
        m.time_decay_w1.copy_(p["D1"])
        m.time_decay_w2.copy_(p["D2"])
        for lin in (m.receptance, m.key, m.value, m.gate):              # identities: r, k, v are the blends themselves, g = silu(xg)
            lin.weight.copy_(torch.eye(C))
    return m.to(dtype)


def check_formula(got, p, xp):
    r, k, v, g, w = (t.double().reshape(-1, C) for t in got)
    out, _, _ = lc.restate_tmix(p, xp, rounded=False)
    dec, _ = lc.restate_decay(p, out[0], rounded=False)
    for name, a, b in (("r", r, out[3]), ("k", k, out[1]), ("v", v, out[2]), ("g", g, F.silu(out[4])), ("w", w, dec)):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 1e-5, (name, err)


def test_the_restatement_without_roundings_is_the_formula_of_jit_func():
    B, T = 3, 7
    p = lc.make_inputs(C, D, DD, B * T)
    m = module(p, torch.float32)
    x = p["x"].float().view(B, T, C)
    first = p["front"][:B].float()
    shifted = torch.cat([first.unsqueeze(1), x[:, :-1]], 1)
    with torch.no_grad():
        got = m.jit_func(x, shifted=shifted)
    xp = lc.token_in_front(p["x"], None, p["front"][:B], None, n_seq=B)
    assert torch.equal(xp.view(B, T, C).float(), shifted)
    check_formula(got, p, xp)
    with torch.no_grad():                                                # zero-padded
        got = m.jit_func(x)
    check_formula(got, p, lc.token_in_front(p["x"], None, None, None, n_seq=B))
    cu = [0, 4, 4, 15, 21]                                               # packed, an empty sequence, carried tokens
    with torch.no_grad():
        got = m.jit_func(x.reshape(1, B * T, C), cu_seqlens=torch.tensor(cu, dtype=torch.int32), shifted0=p["front"].float())
    check_formula(got, p, lc.token_in_front(p["x"], cu, p["front"], None))


def _yardstick(shares_and_ratios, what):
    from test_lowrank_gpu import K_BOUND
    share, ratio = max(shares_and_ratios[0::2]), max(shares_and_ratios[1::2])
    print(f"{what}: largest share {share * 100:.4f} %, largest ratio at k = 1 {ratio:.3f}")
    assert ratio <= K_BOUND / 2, f"{what}: the emulation lies {ratio:.3f} bounds (k = 1) from the restatement; K_BOUND / 2 = {K_BOUND / 2}"
    assert share <= lc.CAP, f"{what}: {share * 100:.4f} % of the emulation's elements differ (cap {lc.CAP * 100} %)"


@pytest.mark.parametrize("width", lc.WIDTHS + (lc.MANY_WIDTH + (lc.MANY_T,),), ids=lambda w: "-".join(map(str, w)))
def test_the_emulations_keep_half_of_k_bound_on_the_parity_inputs(width):
    """The yardstick of the GPU parity tests, guarded for as long as their inputs live (tools/lowrank_parity.py prints the same figures
    into profiles/lowrank_parity.txt): on every input set of lc.TMIX_CASES the fp32-accumulating emulation of the chain, under each of the
    three summation orders, lies within K_BOUND / 2 bounds (k = 1) of the restatement on out and on w and differs from it in at most CAP of
    the elements.  A width or a seed that fails here cannot carry a parity case: exchange it, never K_BOUND or CAP."""
    (C, D, Dd), rows = width[:3], width[3:] or lc.ROWS                     # (a fourth entry: the one row count of the many-tiles case)
    assert all((C, D, Dd, r) in lc.TMIX_CASES for r in rows)
    seen = []
    for total_T in rows:
        case = lc.tmix_case(C, D, Dd, total_T)
        for mm in lc.ORDERS.values():
            seen += lc.emulate_tmix(case, mm)
    _yardstick(seen, f"C={C} D={D} Dd={Dd} rows={rows}")


@pytest.mark.parametrize("C,N,Dd", lc.DECAY_CASES)
def test_the_emulations_keep_half_of_k_bound_on_the_decay_inputs_with_dim_att_unlike_n_embd(C, N, Dd):
    assert N != C
    seen = []
    for rows in lc.ROWS:
        assert (C, N, Dd, rows) in lc.DECAY_NC_CASES
        case = lc.decay_case(C, N, Dd, rows)
        assert tuple(case["w"].shape) == (rows, N) and tuple(case["xw"].shape) == (rows, C)
        for mm in lc.ORDERS.values():
            seen += lc.emulate_decay(case, mm)
    _yardstick(seen, f"decay C={C} N={N} Dd={Dd}")


class Calls:
    """Stand-ins for the three ops of mix_op that the fused path of jit_func calls: eager on the CPU, recorded."""

    def __init__(self):
        self.tmix, self.decay, self.ddlerp = [], [], 0

    def ddlerp_(self, x, maa, m=None, shifted0=None, rev_n=None, cu_seqlens=None):
        self.ddlerp += 1
        first = torch.zeros_like(x[:, 0]) if shifted0 is None else shifted0
        prev = torch.cat([first.unsqueeze(1), x[:, :-1]], 1)
        maa = maa.reshape(-1, 1, 1, x.shape[-1])
        return x + (prev - x) * (maa + (0 if m is None else m))

    def tmix_(self, x, maa_x, W1t, W2t, maa5, cu_seqlens=None, shifted0=None, shift_pool=None, slots=None):
        self.tmix.append((x, maa_x, W1t, W2t, maa5, cu_seqlens, shifted0, shift_pool, slots))
        return torch.zeros((5,) + tuple(x.shape), dtype=x.dtype)

    def decay_(self, xw, D1t, D2t, time_decay):
        self.decay.append((xw, D1t, D2t, time_decay))
        return torch.zeros(tuple(xw.shape[:-1]) + (D2t.shape[0],), dtype=xw.dtype)


@pytest.fixture
def calls(monkeypatch):
    from rwkv_lm_ext_amd import mix_op
    c = Calls()
    monkeypatch.setattr(mix_op, "ddlerp", c.ddlerp_)
    monkeypatch.setattr(mix_op, "tmix_inputs", c.tmix_)
    monkeypatch.setattr(mix_op, "decay_lowrank", c.decay_)
    return c


def test_fuse_lowrank_routing(calls):
    bf = torch.bfloat16
    B, T = 2, 5
    p = lc.make_inputs(C, D, DD, B * T)
    m = module(p, bf)
    assert m.fuse_lowrank is False
    m.fused = True                                                       # the fused path, here on the CPU behind the stand-ins
    x = p["x"].view(B, T, C)
    first = p["front"][:B]
    shifted = torch.cat([first.unsqueeze(1), x[:, :-1]], 1)
    with torch.no_grad():
        m.jit_func(x, shifted=shifted)
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (0, 0, 2)                # off by default: today's calls

    m.fuse_lowrank = True
    with torch.no_grad():
        out = m.jit_func(x, shifted=shifted)
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (1, 1, 2) and len(out) == 5
    gx, maa_x, W1t, W2t, maa5, cu, s0, pool, slots = calls.tmix[0]
    assert torch.equal(gx, x) and cu is None and pool is None and slots is None and torch.equal(s0, first)
    assert torch.equal(maa_x, m.time_maa_x.view(C)) and torch.equal(maa5, m._maa5())
    assert tuple(W1t.shape) == (5 * D, C) and W1t.is_contiguous() and torch.equal(W1t, m.time_maa_w1.t())
    assert tuple(W2t.shape) == (5, C, D) and W2t.is_contiguous() and torch.equal(W2t, m.time_maa_w2.transpose(1, 2))
    xw, D1t, D2t, td = calls.decay[0]
    assert tuple(xw.shape) == (B, T, C) and xw.is_contiguous()
    assert tuple(D1t.shape) == (DD, C) and D1t.is_contiguous() and torch.equal(D1t, m.time_decay_w1.t())
    assert tuple(D2t.shape) == (C, DD) and D2t.is_contiguous() and torch.equal(D2t, m.time_decay_w2.t())
    assert torch.equal(td, m.time_decay.view(C))

    m.jit_func(x, shifted=shifted)                                       # a gradient is required (the parameters): today's calls
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (1, 1, 4)
    m.requires_grad_(False)
    m.jit_func(x, shifted=shifted)                                       # grad mode on, but nothing requires one
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (2, 2, 4)
    m.jit_func(x.clone().requires_grad_(), shifted=shifted)              # ... except x
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (2, 2, 6)
    with torch.no_grad():
        m.jit_func(x, rev_n=torch.tensor([2, 3], dtype=torch.int32))     # a reversal map
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (2, 2, 8)

    m.fused = None                                                       # bf16 on the CPU, and fp32: the eager path, none of the three ops
    with torch.no_grad():
        m.jit_func(x)
        m.float().jit_func(x.float())
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (2, 2, 8)
    m.fused = True                                                       # forced onto the fused path, fp32 still keeps today's calls
    with torch.no_grad():
        m.jit_func(x.float())
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (2, 2, 10)


def test_widths_the_kernels_do_not_have_keep_todays_calls(calls):
    from rwkv_lm_ext_amd.callers import Tmix_x060
    m = Tmix_x060(C, C).bfloat16()
    m.time_maa_w1 = torch.nn.Parameter(torch.zeros(C, 5 * 16, dtype=torch.bfloat16))         # D = 16
    m.time_maa_w2 = torch.nn.Parameter(torch.zeros(5, 16, C, dtype=torch.bfloat16))
    m.fused, m.fuse_lowrank = True, True
    with torch.no_grad():
        m.jit_func(torch.zeros(1, 3, C, dtype=torch.bfloat16))
    assert (len(calls.tmix), len(calls.decay), calls.ddlerp) == (0, 0, 2)


def test_the_weight_copies_are_kept_and_rebuilt_after_an_update():
    p = lc.make_inputs(C, D, DD, 4)
    m = module(p, torch.bfloat16)
    held = m._lowrank_weights()
    again = m._lowrank_weights()
    assert all(a is b for a, b in zip(held, again))                      # kept: no copy per call
    with torch.no_grad():
        m.time_maa_w1.add_(1.0)                                          # an optimizer step: same storage, new version
    new = m._lowrank_weights()
    assert new[1] is not held[1] and torch.equal(new[1], m.time_maa_w1.t()) and not torch.equal(new[1], held[1])
    assert all(a is b for a, b in zip(new, m._lowrank_weights()))
    m.time_decay.data = torch.full((1, 1, C), -3.0, dtype=torch.bfloat16)          # a replaced tensor (load, .to()): new storage
    assert torch.equal(m._lowrank_weights()[6], torch.full((C,), -3.0, dtype=torch.bfloat16))
    with torch.no_grad():
        m.time_maa_k.mul_(0.5)
    assert torch.equal(m._lowrank_weights()[3], m._maa5())
    assert "_lowrank_cache" not in m.state_dict()
    held = m._lowrank_weights()
    m.time_decay_w1.data.mul_(2.0)                                       # a write through .data: neither key changes, the copy is stale ...
    assert m._lowrank_weights()[4] is held[4] and not torch.equal(held[4], m.time_decay_w1.t())
    m.drop_lowrank_weights()                                             # ... until it is dropped
    assert torch.equal(m._lowrank_weights()[4], m.time_decay_w1.t())
