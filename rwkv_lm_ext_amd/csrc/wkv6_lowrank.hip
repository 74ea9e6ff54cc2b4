// The two low-rank pairs in front of the RWKV-6 time-mix projections (include/wkv6_amd.h: wkv6_tmix_lerp_lowrank_bf16,
// wkv6_decay_lowrank_bf16), hand-written for gfx950, forward only: the data-dependent lerp (src/model.py:435-448)
//     lead = x + (xp - x) (.) maa_x;   low = tanh(lead W1);   corr_s = low_s W2[s];   out_s = x + (xp - x) (.) (maa5[s] + corr_s),  s = 0..4
// and the decay (src/model.py:451-452)
//     w = time_decay + tanh(xw D1) D2
// in two launches each, "shrink" and "expand", with the bf16 `low` [rows, 5 D] / [rows, Dd] between them in the workspace.  lead, corr and
// the products in front of tanh never reach memory.  The rounding points are those of the chain of ddlerp kernels and torch matmuls they
// stand for: lead, the product in front of tanh, low and corr are each rounded to bf16 once; what differs is how the sums inside the
// two contractions are taken (the shrink's: 32 products in fp32 inside an MFMA, the steps in fp64; the expand's: an fp32 MFMA chain).
//
// Both kernels work on the 16-row MFMA tile of wkv6_tile16.h (lane roles, K walk, expand tile), shared with wkv6_lora.hip, here without
// adapter groups and with the weights in nn.Linear layout [out, in]: a row's bits do not depend on the rows beside it, on its place in the
// tile or on the batch.  A row past the end is a literal zero operand, never loaded, never stored.
//
// Which token stands in front of a row is the rule of ddlerp_fwd_slots_kernel (wkv6_mix.hip), front_of below.
#include <climits>
#include "wkv6_host.h"                 // launch<>, to_rc, overlap
#include "wkv6_tile16.h"

namespace wkv6 {
namespace {

constexpr int SHRINK_WAVES = 4;        // waves of a shrink workgroup = the most K chunks: wave q sums chunk q
constexpr int EXPAND_WAVES = 4;        // waves of an expand workgroup: wave w serves column block 4 blockIdx.y + w of the tile

struct LowrankArgs {
    int rows, n_seq, C, N, DT, n_slots;   // C: width of x / xw (the shrink's K);  N: output columns of the expand;  DT: columns of low
    const int* cu;            // [n_seq + 1] or null (dense: sequence s owns rows [s T, (s + 1) T), T = rows / n_seq)
    const int* slot;          // [n_seq] or null (slot = sequence index)
    const bf16_t* x;          // [rows,C]  (the decay: xw)
    const bf16_t* front;      // [n_slots,C] or null (zero tokens)
    const bf16_t* maa_x;      // [C]
    const bf16_t* W1t;        // [DT,C]
    const bf16_t* W2t;        // lerp: [5,N,D];  bias: [N,Dd]
    const bf16_t* bias;       // lerp: maa5 [5,N];  bias: time_decay [N]
    bf16_t* out;              // lerp: [5,rows,N];  bias: [rows,N]
    bf16_t* low;              // [rows,DT]  (workspace)
};

// The token in front of row `row` (0 <= row < rows): where its C channels lie, or null for a zero token.  Row t is the first row of
// sequence s = seq_of_row(t) iff cu[s] == t; every other row, rows outside every sequence included, takes row t - 1, and row 0 takes zero
// if it opens nothing.  A first row takes front[slot[s]] (slot null: front[s]); no front, or a slot outside the pool, is a zero token.
// The sequence number is below n_seq by construction and the slot is judged before an address is formed from it.
__device__ __forceinline__ const bf16_t* front_of(const LowrankArgs& a, long row)
{
    int sq;
    bool first;
    if (a.cu) {
        sq = seq_of_row(a.cu, a.n_seq, row);
        first = sq >= 0 && (long)a.cu[sq] == row;
    } else {
        const int T = a.rows / a.n_seq;
        sq = clampi((int)(row / T), 0, a.n_seq - 1);
        first = row % T == 0;
    }
    if (!first) return row > 0 ? a.x + (row - 1) * a.C : nullptr;
    if (!a.front) return nullptr;
    const int sl = a.slot ? a.slot[sq] : sq;
    return sl >= 0 && sl < a.n_slots ? a.front + (long)sl * a.C : nullptr;
}

// bf16(fmaf(xp - x, maa, x)) of 8 channels: the fp32 arithmetic of lerp_store (wkv6_mix.hip)
__device__ __forceinline__ b8v lerp8(v4u x, v4u xp, v4u m)
{
    v4u o;
#pragma unroll
    for (int p = 0; p < 4; ++p)
        o[p] = pack_bf2(fmaf(bf_lo(xp[p]) - bf_lo(x[p]), bf_lo(m[p]), bf_lo(x[p])), fmaf(bf_hi(xp[p]) - bf_hi(x[p]), bf_hi(m[p]), bf_hi(x[p])));
    return __builtin_bit_cast(b8v, o);
}

// fp64 -> bf16, rounded to nearest even ONCE: the fp32 value in between is rounded to odd (truncated, its last bit set when anything was
// cut off), so the rounding to bf16 behind it sees on which side of a tie the fp64 value lay
__device__ __forceinline__ float to_odd_f32(double v)
{
    const float f = __double2float_rz(v);
    return (double)f != v ? __uint_as_float(__float_as_uint(f) | 1u) : f;       // (NaN: the quiet bit pattern keeps its class)
}

// ---- shrink: low = bf16(tanh(float(bf16(a W1t^T)))), a = the rows of x (the decay) or the lerp with maa_x formed in registers (LERP).
// One workgroup per (tile of 16 rows, 16 columns j of low); MFMA rows = j, columns = tokens, so lane (c, g) ends with low[row c][j0 + 4g
// .. + 3].  K = C is walked in the chunks of for_each_kstep (wkv6_tile16.h), wave q takes chunk q.  Every MFMA sums its 32 products in
// fp32 from a zero accumulator and the steps' results are added in fp64 (four adds a lane and step): the product in front of tanh is
// then off its exact value by about 1e-8 at C = 4096, where an fp32 chain over the steps is off by 2e-7 and rounds to the other bf16
// neighbour ten times as often.  The waves leave their fp64 sums in LDS, and after the barrier wave 0 adds a token's chunks
// (sum_chunks), rounds once to bf16, takes the tanh of the rounded value in fp64 and rounds once.
template <bool LERP>
__global__ void __launch_bounds__(SHRINK_WAVES * 64) lowrank_shrink_kernel(const LowrankArgs a)
{
    __shared__ __align__(32) double part[SHRINK_WAVES][TILE][16];               // (sum_chunks reads four at a time)
    const Lane16 ln;
    const int wave = ln.wave, c = ln.c, g = ln.g;
    const long row = (long)blockIdx.x * TILE + c;
    const bool in = row < a.rows;
    const int nsteps = a.C / 32, nch = min(SHRINK_WAVES, nsteps);
    const bf16_t* wr = a.W1t + ((long)blockIdx.y * 16 + c) * a.C + 8 * g;       // DT is a multiple of 16: every j is there
    const bf16_t* xr = a.x + row * a.C + 8 * g;                                 // (formed, not dereferenced, for rows past the end)
    const bf16_t* pr = nullptr;
    const bf16_t* mr = nullptr;
    if constexpr (LERP) {
        mr = a.maa_x + 8 * g;
        if (in) {
            const bf16_t* p = front_of(a, row);
            if (p) pr = p + 8 * g;
        }
    }
    auto token = [&](v4u xv, v4u pv, v4u mv) -> b8v {
        if constexpr (LERP) return lerp8(xv, pv, mv);
        else return __builtin_bit_cast(b8v, xv);
    };
    const v4u z = {0u, 0u, 0u, 0u};
    if (wave < nch) {
        const f4v zero = {0.f, 0.f, 0.f, 0.f};
        double acc[4] = {0., 0., 0., 0.};
        b8v wf[4];
        v4u xv[4], pv[4], mv[4];
        for_each_kstep(wave, nch, nsteps,
                       [&](int u, int k) {
                           wf[u] = load8(wr + k);
                           xv[u] = in ? ld16(xr + k) : z;
                           if constexpr (LERP) {
                               pv[u] = pr ? ld16(pr + k) : z;
                               mv[u] = ld16(mr + k);
                           }
                       },
                       [&](int u) {
                           const f4v p = mfma32(wf[u], in ? token(xv[u], pv[u], mv[u]) : zero8(), zero);
#pragma unroll
                           for (int i = 0; i < 4; ++i) acc[i] += (double)p[i];
                       });
        if (in) {
#pragma unroll
            for (int i = 0; i < 4; ++i) part[wave][c][4 * g + i] = acc[i];
        }
    }
    __syncthreads();
    if (wave == 0 && in) {
        const auto sum = sum_chunks(part, nch, c, g);
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float z = bf_lo(pack_bf2(to_odd_f32(sum[i]), 0.f));                     // the product, rounded as the matmul's output is
            t[i] = to_odd_f32(tanh((double)z));
        }
        *reinterpret_cast<v2u*>(a.low + row * a.DT + blockIdx.y * 16 + 4 * g) = v2u{pack_bf2(t[0], t[1]), pack_bf2(t[2], t[3])};
    }
}

// ---- expand: corr = bf16(low W2t^T) and one of two epilogues.  One workgroup per tile of 16 rows and 4 blocks of 64 output columns, a
// wave per block.  Contraction over j in R / 32 steps; the tile and its column map are expand_pass's (wkv6_tile16.h): lane (c, g) ends with
// the 16 consecutive columns n0 + 16 g .. + 15 of its token.
//   LERP:  out[s][t,n] = bf16(fmaf(xp - x, maa5[s][n] + corr_s[t,n], x)),  s = 0..4 with low_s = low[t, s R .. (s + 1) R) and W2t[s] [N,R];
//          x and xp - x of the lane's 16 channels are loaded once and serve the five planes
//   else:  out[t,n] = bf16(bias[n] + corr[t,n])
template <int R, bool LERP>
__global__ void __launch_bounds__(EXPAND_WAVES * 64) lowrank_expand_kernel(const LowrankArgs a)
{
    constexpr int STEPS = R / 32, NS = LERP ? 5 : 1;
    const Lane16 ln;
    const int wave = ln.wave, c = ln.c, g = ln.g;
    const long row = (long)blockIdx.x * TILE + c;
    const bool in = row < a.rows;
    const int nb = blockIdx.y * EXPAND_WAVES + wave;
    if (nb >= a.N / EXPAND_NB) return;                   // (wave-uniform; the kernel has no barrier)
    const int n0 = nb * EXPAND_NB, nl = n0 + 16 * g;
    float x[16], d[16];                                  // LERP: the lane's channels of x and of xp - x
    if constexpr (LERP) {
        if (in) {
            const bf16_t* p = front_of(a, row);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const v4u xv = ld16(a.x + row * a.C + nl + 8 * h);
                const v4u pv = p ? ld16(p + nl + 8 * h) : v4u{0u, 0u, 0u, 0u};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    x[8 * h + 2 * q] = bf_lo(xv[q]); x[8 * h + 2 * q + 1] = bf_hi(xv[q]);
                    d[8 * h + 2 * q] = bf_lo(pv[q]) - bf_lo(xv[q]); d[8 * h + 2 * q + 1] = bf_hi(pv[q]) - bf_hi(xv[q]);
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        b8v lf[STEPS];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) lf[st] = in ? load8(a.low + row * a.DT + s * R + 32 * st + 8 * g) : zero8();
        const bf16_t* wp = a.W2t + (long)s * a.N * R + 8 * g;
        f4v acc[4];
        expand_pass<R, STEPS>(acc, wp, true, n0, c, lf);
        if (in) {
            const bf16_t* bp = a.bias + (long)s * a.N + nl;
            v4u* op = reinterpret_cast<v4u*>(a.out + ((long)s * a.rows + row) * a.N + nl);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const v4u b = ld16(bp + 8 * h);
                op[h] = expand_half(acc, h, [&](int p, float lo, float hi) {
                    const int e = 8 * h + 2 * p;                                       // the word's lower column among the lane's 16
                    const unsigned corr = pack_bf2(lo, hi);                            // rounded as the matmul's output is
                    if constexpr (LERP) return pack_bf2(fmaf(d[e], bf_lo(b[p]) + bf_lo(corr), x[e]), fmaf(d[e + 1], bf_hi(b[p]) + bf_hi(corr), x[e + 1]));
                    else return pack_bf2(bf_lo(b[p]) + bf_lo(corr), bf_hi(b[p]) + bf_hi(corr));
                });
            }
        }
    }
}

// shrink, then expand, in stream order; R: the expand's contraction width (D, Dd)
template <int R, bool LERP> hipError_t launch_lowrank(const LowrankArgs& a, hipStream_t st)
{
    const unsigned tiles = (unsigned)(((long)a.rows + TILE - 1) / TILE), nblocks = (unsigned)(a.N / EXPAND_NB);
    if (hipError_t e = launch<lowrank_shrink_kernel<LERP>>(dim3(tiles, a.DT / 16), dim3(SHRINK_WAVES * 64), 0, st, a)) return e;
    return launch<lowrank_expand_kernel<R, LERP>>(dim3(tiles, (nblocks + EXPAND_WAVES - 1) / EXPAND_WAVES), dim3(EXPAND_WAVES * 64), 0, st, a);
}

// a row width the kernels have: a multiple of 64, at most 4096 (check_rows of wkv6_mix.hip)
bool width_ok(int C) { return C >= 64 && C % 64 == 0 && C <= 4096; }

}  // namespace
}  // namespace wkv6

using namespace wkv6;

extern "C" {

size_t wkv6_lowrank_workspace_bytes(long rows, int D_total)
{
    if (rows < 1 || rows > 0x7fffffffL) return 0;
    if (D_total != 5 * 32 && D_total != 5 * 64 && D_total != 64 && D_total != 128) return 0;
    return ((size_t)rows * D_total * 2 + 255) & ~(size_t)255;
}

int wkv6_tmix_lerp_lowrank_bf16(long total_T, int n_seq, int C, int D, const int* cu_seqlens, const void* x, const void* front, int n_slots,
                                const int* slot, const void* maa_x, const void* W1t, const void* W2t, const void* maa5, void* out,
                                void* workspace, size_t workspace_bytes, void* stream)
{
    // the order of the refusals is part of the contract (include/wkv6_amd.h)
    if (total_T < 1 || n_seq < 1 || D < 1 || !width_ok(C)) return WKV6_EINVAL;
    if (!cu_seqlens && total_T % n_seq) return WKV6_EINVAL;                       // dense: n_seq sequences of one length
    if (front && (n_slots < 1 || (!slot && n_slots < n_seq))) return WKV6_EINVAL; // slot = sequence index: the pool must hold n_seq slots
    if ((D != 32 && D != 64) || total_T > 0x7fffffffL) return WKV6_EUNSUPPORTED;  // cu_seqlens is int32
    if (!x || !maa_x || !W1t || !W2t || !maa5 || !out || !workspace) return WKV6_ENULL;
    if (((uintptr_t)x | (uintptr_t)front | (uintptr_t)maa_x | (uintptr_t)W1t | (uintptr_t)W2t | (uintptr_t)maa5 | (uintptr_t)out |
         (uintptr_t)workspace) & 15)
        return WKV6_EINVAL;
    if (((uintptr_t)cu_seqlens | (uintptr_t)slot) & 3) return WKV6_EINVAL;
    const size_t row_bytes = (size_t)C * 2, out_bytes = 5 * (size_t)total_T * row_bytes, w_bytes = 5 * (size_t)D * row_bytes;
    const size_t need = wkv6_lowrank_workspace_bytes(total_T, 5 * D);
    if (overlap(out, out_bytes, x, total_T * row_bytes) || overlap(out, out_bytes, front, (size_t)n_slots * row_bytes) ||
        overlap(out, out_bytes, maa_x, row_bytes) || overlap(out, out_bytes, W1t, w_bytes) || overlap(out, out_bytes, W2t, w_bytes) ||
        overlap(out, out_bytes, maa5, 5 * row_bytes) || overlap(out, out_bytes, workspace, need))
        return WKV6_EINVAL;
    if (workspace_bytes < need) return WKV6_EWORKSPACE;
    LowrankArgs a = {};
    a.rows = (int)total_T; a.n_seq = n_seq; a.C = C; a.N = C; a.DT = 5 * D; a.n_slots = front ? n_slots : 0;
    a.cu = cu_seqlens; a.slot = slot;
    a.x = (const bf16_t*)x; a.front = (const bf16_t*)front; a.maa_x = (const bf16_t*)maa_x;
    a.W1t = (const bf16_t*)W1t; a.W2t = (const bf16_t*)W2t; a.bias = (const bf16_t*)maa5;
    a.out = (bf16_t*)out; a.low = (bf16_t*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    return to_rc(D == 32 ? launch_lowrank<32, true>(a, st) : launch_lowrank<64, true>(a, st));
}

int wkv6_decay_lowrank_bf16(long rows, int C, int Dd, int N, const void* xw, const void* D1t, const void* D2t, const void* time_decay,
                            void* w, void* workspace, size_t workspace_bytes, void* stream)
{
    if (rows < 1 || Dd < 1 || !width_ok(C) || !width_ok(N)) return WKV6_EINVAL;
    if ((Dd != 64 && Dd != 128) || rows > 0x7fffffffL) return WKV6_EUNSUPPORTED;
    if (!xw || !D1t || !D2t || !time_decay || !w || !workspace) return WKV6_ENULL;
    if (((uintptr_t)xw | (uintptr_t)D1t | (uintptr_t)D2t | (uintptr_t)time_decay | (uintptr_t)w | (uintptr_t)workspace) & 15) return WKV6_EINVAL;
    const size_t w_bytes = (size_t)rows * N * 2, need = wkv6_lowrank_workspace_bytes(rows, Dd);
    if (overlap(w, w_bytes, xw, (size_t)rows * C * 2) || overlap(w, w_bytes, D1t, (size_t)Dd * C * 2) ||
        overlap(w, w_bytes, D2t, (size_t)N * Dd * 2) || overlap(w, w_bytes, time_decay, (size_t)N * 2) || overlap(w, w_bytes, workspace, need))
        return WKV6_EINVAL;
    if (workspace_bytes < need) return WKV6_EWORKSPACE;
    LowrankArgs a = {};
    a.rows = (int)rows; a.n_seq = 1; a.C = C; a.N = N; a.DT = Dd;
    a.x = (const bf16_t*)xw; a.W1t = (const bf16_t*)D1t; a.W2t = (const bf16_t*)D2t; a.bias = (const bf16_t*)time_decay;
    a.out = (bf16_t*)w; a.low = (bf16_t*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    return to_rc(Dd == 64 ? launch_lowrank<64, false>(a, st) : launch_lowrank<128, false>(a, st));
}

}  // extern "C"
