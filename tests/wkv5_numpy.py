"""A literal fp64 numpy statement of the WKV5 recurrence and of its gradients (cuda/wkv5_cuda.cu:25-188), shared by
tests/test_wkv5_cpu.py and tests/test_wkv5_gpu.py.  Per (batch, head), d[i] = exp(-exp(w[h][i])):

    y_t[j]        = sum_i r_t[i] (u[i] k_t[i] v_t[j] + S_t[i][j])
    S_{t+1}[i][j] = d[i] S_t[i][j] + k_t[i] v_t[j],   S_0 = 0

The gradients are the plain adjoint sweep (G = dL/dS carried from the last token to the first) -- not the kernels' forward
sensitivity D = dS/dd -- so the two derivations check one another.  gw is the gradient with respect to the RAW w.
"""
import numpy as np
import torch

N = 64


def _split(x, H):
    B, T, C = x.shape
    return np.asarray(x, np.float64).reshape(B, T, H, C // H)


def decay(w):
    return np.exp(-np.exp(np.asarray(w, np.float64)))


def forward(r, k, v, w, u, return_states=False):
    """r,k,v [B,T,C]; w,u [H,N] -> y [B,T,C] (fp64)."""
    B, T, C = r.shape
    H = np.shape(u)[0]
    r_, k_, v_ = (_split(x, H) for x in (r, k, v))
    d, u_ = decay(w), np.asarray(u, np.float64)
    S = np.zeros((B, H, C // H, C // H))                     # [b][h][key i][value j]
    y = np.empty((B, T, H, C // H))
    states = []
    for t in range(T):
        if return_states:
            states.append(S.copy())
        kv = k_[:, t, :, :, None] * v_[:, t, :, None, :]
        y[:, t] = np.einsum("bhi,bhij->bhj", r_[:, t], u_[None, :, :, None] * kv + S)
        S = d[None, :, :, None] * S + kv
    y = y.reshape(B, T, C)
    return (y, states) if return_states else y


def backward(r, k, v, w, u, gy):
    """dict(gr, gk, gv [B,T,C]; gw_b, gu_b [B,C] per-batch partials; gw, gu [H,N] summed over the batch), fp64."""
    B, T, C = r.shape
    H = np.shape(u)[0]
    n = C // H
    r_, k_, v_, g_ = (_split(x, H) for x in (r, k, v, gy))
    d, u_ = decay(w), np.asarray(u, np.float64)
    _, states = forward(r, k, v, w, u, return_states=True)
    gr, gk, gv = (np.zeros((B, T, H, n)) for _ in range(3))
    gu_b, gd_b = np.zeros((B, H, n)), np.zeros((B, H, n))
    G = np.zeros((B, H, n, n))                                # dL/dS_{t+1}
    for t in range(T - 1, -1, -1):
        S = states[t]
        vg = np.einsum("bhj,bhj->bh", v_[:, t], g_[:, t])[:, :, None]
        gr[:, t] = np.einsum("bhij,bhj->bhi", S, g_[:, t]) + u_[None] * k_[:, t] * vg
        gu_b += r_[:, t] * k_[:, t] * vg
        gk[:, t] = np.einsum("bhij,bhj->bhi", G, v_[:, t]) + u_[None] * r_[:, t] * vg
        ruk = np.einsum("bhi,bhi->bh", r_[:, t] * u_[None], k_[:, t])[:, :, None]
        gv[:, t] = np.einsum("bhij,bhi->bhj", G, k_[:, t]) + ruk * g_[:, t]
        gd_b += np.einsum("bhij,bhij->bhi", G, S)
        G = d[None, :, :, None] * G + r_[:, t, :, :, None] * g_[:, t, :, None, :]
    gw_b = gd_b * (d * -np.exp(np.asarray(w, np.float64)))[None]      # dd/dw = d * ew, ew = -exp(w)
    return dict(gr=gr.reshape(B, T, C), gk=gk.reshape(B, T, C), gv=gv.reshape(B, T, C),
                gw_b=gw_b.reshape(B, C), gu_b=gu_b.reshape(B, C), gw=gw_b.sum(0), gu=gu_b.sum(0))


def oracle_pair(orc, r, k, v, w, u, gy):
    """The pinned fp64 WKV6 oracle on the same problem: w broadcast over batch and time, gw summed over time.
    Returns (y, dict like backward()) from the oracle's fp32 outputs."""
    B, T, C = r.shape
    H = np.shape(u)[0]
    f = lambda a: np.ascontiguousarray(a, np.float32)
    wb = f(np.broadcast_to(np.asarray(w, np.float32).reshape(1, 1, C), (B, T, C)))
    y = orc.forward(f(r), f(k), f(v), wb, f(u))
    g = orc.backward(f(r), f(k), f(v), wb, f(u), f(gy))
    gw_b = g["gw"].astype(np.float64).sum(1)
    return y, dict(gr=g["gr"], gk=g["gk"], gv=g["gv"], gw_b=gw_b, gu_b=g["gu_b"].astype(np.float64),
                   gw=gw_b.sum(0).reshape(H, C // H), gu=g["gu_b"].astype(np.float64).sum(0).reshape(H, C // H))


class NumpyWKV5(torch.autograd.Function):
    """The restatement as a differentiable torch operator (CPU, any float dtype): the stand-in for the HIP operator in the
    tests of the time-mix caller."""

    @staticmethod
    def forward(ctx, B, T, C, H, r, k, v, w, u):
        ctx.save_for_backward(r, k, v, w, u)
        a = [t.detach().double().numpy() for t in (r, k, v, w, u)]
        return torch.from_numpy(forward(*a)).to(r.dtype)

    @staticmethod
    def backward(ctx, gy):
        r, k, v, w, u = ctx.saved_tensors
        a = [t.detach().double().numpy() for t in (r, k, v, w, u)]
        g = backward(*a, gy.detach().double().numpy())
        t = lambda x, like: torch.from_numpy(np.ascontiguousarray(x)).to(like.dtype).view_as(like)
        return (None, None, None, None, t(g["gr"], r), t(g["gk"], k), t(g["gv"], v), t(g["gw"], w), t(g["gu"], u))


def numpy_wkv5(B, T, C, H, r, k, v, w, u):
    return NumpyWKV5.apply(B, T, C, H, r, k, v, w, u)


def problem(B, T, H, seed, decay_set="stress"):
    """Random bf16-representable inputs as float32 arrays: r, k, v, gy [B,T,C]; w, u [H,N].  decay_set: "ramp" = the model's
    initial decay ramp (src/model.py:318-321, w in [-6, -1], layer 0), "stress" = the suite's w ~ N(-1, 0.5^2)."""
    g = torch.Generator().manual_seed(seed)
    C = H * N
    bf = lambda t: t.to(torch.bfloat16).float().numpy()
    r, k, v = (bf(torch.randn(B, T, C, generator=g) * 0.5) for _ in range(3))
    gy = bf(torch.randn(B, T, C, generator=g))
    u = bf(torch.randn(H, N, generator=g) * 0.3)
    if decay_set == "ramp":
        n = torch.arange(C, dtype=torch.float32)
        w = bf((-6 + 5 * (n / (C - 1)) ** 0.7).view(H, N))
    else:
        w = bf(-1 + 0.5 * torch.randn(H, N, generator=g))
    return dict(r=r, k=k, v=v, w=w, u=u, gy=gy)
