// Exact-fp32 token-serial WKV5 kernels for gfx950: WKV6 with a decay that is constant over batch and time
// (cuda/wkv5_cuda.cu:25-188).  w and u are [H,N] parameters; per (batch, head), d[i] = exp(-exp(w[h][i])):
//     y_t[j]        = sum_i r_t[i] (u[i] k_t[i] v_t[j] + S_t[i][j])
//     S_{t+1}[i][j] = d[i] S_t[i][j] + k_t[i] v_t[j],   S_0 = 0
// Layout as the WKV6 scan kernels (wkv6_scan.h): one 512-thread workgroup (8 wave64) per (batch, head), the 64x64 state
// tiled over the lanes, r/k/v(/gy) rows staged 16 tokens at a time through a double-buffered LDS image, DPP / permlane
// reductions.  What the static decay removes: the decay stream (no w loads, no per-token exp, no decay rows in LDS: every
// lane keeps the d of its own key rows in registers for the whole row) and the [B,T,C] gw output with its fp32 scratch
// tensor -- gw and gu are accumulated in fp32 registers over the whole row and written once per (batch, head).
//
// Backward = two independent kernels (neither reads what the other writes, so there is no scratch tensor between them):
//   ascending  pass: carries S and D = dS/dd,  D_{t+1} = d (.) D_t + S_t  (D_0 = D_1 = 0), and emits
//       gr_t[i] = sum_j gy_t[j] S_t[i][j] + u[i] k_t[i] (v_t . gy_t)
//       gu[i]  += r_t[i] k_t[i] (v_t . gy_t)
//       gd[i]  += r_t[i] sum_j gy_t[j] D_t[i][j]                 (= dL/dd[i]; every lane sums its own 4 columns over
//                                                                   the row, the 16 lanes of a key row are added once)
//       gw[b][i] = ew[i] d[i] gd[i],  ew = -exp(w)                (gradient with respect to the RAW w, as the reference's
//                                                                   `ww * gw`, cuda/wkv5_cuda.cu:119-143)
//     One extra state instead of the reference's two (saaaa / sbbbb), no T-sized array, any T >= 1; T <= 2 gives gw = 0.
//   descending pass: G <- d (.) G + r_t gy_t^T;  gk_t[i] = sum_j G[i][j] v_t[j] + u[i] r_t[i] (v_t . gy_t),
//       gv_t[j] = sum_i k_t[i] G[i][j] + (sum_i u[i] r_t[i] k_t[i]) gy_t[j]        (cuda/wkv5_cuda.cu:145-187).
// Every sum has a fixed order (no atomics): two calls on the same inputs are bit-identical.
#pragma once
#include "wkv6_common.h"

namespace wkv6 {

struct Wkv5Args {
    int B, T, C, H;
    const void *r, *k, *v, *u;      // [B,T,C] x3, [H,N], I/O type
    const void* w;                  // [H,N]: raw w in the I/O type when wkind == 1, fp32 decay eew = exp(-exp(w)) when 0
    const float* ew;                // [H,N] fp32 -exp(w): backward with wkind == 0 only
    int wkind;
    void* y;                        // forward output
    const void* gy;                 // backward input
    void *gr, *gk, *gv;             // backward outputs [B,T,C], I/O type
    void *gw, *gu;                  // [B,C] per-batch partials (null: skip): fp32 when part_f32 or fp32 I/O, else bf16
    int part_f32;
};

hipError_t launch_wkv5_fwd(const Wkv5Args& a, bool io_f32, hipStream_t st);
hipError_t launch_wkv5_bwd(const Wkv5Args& a, bool io_f32, hipStream_t st);

}  // namespace wkv6
