// Sentence pooling on a packed variable-length batch (include/wkv6_amd.h: wkv6_pool_packed_forward / _backward): the embedding head of
// RwkvForSequenceEmbedding (src/model_ext.py:1708-1738) without the padded [B,T,C] tensor.  bf16 I/O, fp32 arithmetic, one rounding.
//
// Forward: a workgroup owns one sequence and 512 channels (64 lanes x 8 bf16 = one 16-byte load per lane and token, 1 KiB contiguous per
// wave); its four waves take the tokens t = wave, wave + 4, ... with four loads in flight each and fp32 accumulators in registers, and
// meet once in LDS where wave 0 adds the four partial sums in wave order.  At the training shape (96 sequences, C = 2048) that is 384
// workgroups of four waves with 16 row loads in flight per workgroup.  Which token a wave adds when depends on the token's index in its
// sequence alone, so a sequence's row has the same bits alone or in a batch, wherever it lies.  No atomics.
// Backward: a workgroup per row of gx; the row finds its sequence by bisection in cu_seqlens (workgroup-uniform scalar loads) and writes
// weight * gout[s], or +0 where it belongs to nothing that was summed.
#include "wkv6_host.h"                 // launch<>, to_rc

namespace wkv6 {

namespace {

constexpr int POOL_WAVES = 4, POOL_UNROLL = 4, POOL_COLS = 64 * 8;     // waves per workgroup, loads in flight per wave, channels per workgroup

struct PoolArgs {
    long total_T;
    int n_seq, C, ncb;               // ncb: workgroups per sequence (forward)
    const int *cu, *actual;          // cu_seqlens [n_seq + 1]; actual_len [n_seq] or null
    const bf16_t* in;                // forward: x [total_T,C]; backward: gout [n_seq,C]
    bf16_t* out;                     // forward: out [n_seq,C]; backward: gx [total_T,C]
};

// sequence s: first row, length and pooled position a_s, every cu_seqlens entry clamped into [0, total_T] before anything is formed from it
struct Span {
    int start, len, a;
};
__device__ __forceinline__ Span span_of(const PoolArgs& p, int s)
{
    const int T = (int)p.total_T;
    Span sp;
    sp.start = clampi(p.cu[s], 0, T);
    sp.len = max(clampi(p.cu[s + 1], 0, T) - sp.start, 0);
    sp.a = p.actual ? clampi(p.actual[s], 0, sp.len - 1) : sp.len - 1;
    return sp;
}

__device__ __forceinline__ void unpack8(uint4 raw, float (&o)[8])
{
    o[0] = bf_lo(raw.x); o[1] = bf_hi(raw.x); o[2] = bf_lo(raw.y); o[3] = bf_hi(raw.y);
    o[4] = bf_lo(raw.z); o[5] = bf_hi(raw.z); o[6] = bf_lo(raw.w); o[7] = bf_hi(raw.w);
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8])
{
    return make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
}
constexpr unsigned BF16_NAN2 = 0x7fc07fc0u;      // two quiet NaNs

template <int KIND> __global__ __launch_bounds__(POOL_WAVES * 64) void pool_fwd_kernel(PoolArgs p)
{
    __shared__ float part[POOL_WAVES - 1][8][64];
    const int s = blockIdx.x / p.ncb, cb = blockIdx.x - s * p.ncb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (cb * 64 + lane) * 8;
    const bool live = col < p.C;
    const Span sp = span_of(p, s);
    uint4* const dst = reinterpret_cast<uint4*>(p.out + (long)s * p.C + col);
    const bf16_t* const xs = p.in + (long)sp.start * p.C + col;          // rows start .. start + a only are ever read

    // ---- the rows that need no sum (workgroup-uniform): an empty sequence, the copy, the 0 / 0 of a mean at a_s == 0
    if (sp.len == 0 || KIND == WKV6_POOL_LASTTOKEN || sp.a == 0) {
        if (wave == 0 && live) {
            if (sp.len == 0) *dst = make_uint4(0u, 0u, 0u, 0u);
            else if (KIND == WKV6_POOL_LASTTOKEN) *dst = *reinterpret_cast<const uint4*>(xs + (long)sp.a * p.C);
            else *dst = make_uint4(BF16_NAN2, BF16_NAN2, BF16_NAN2, BF16_NAN2);
        }
        return;
    }

    const int n = KIND == WKV6_POOL_WEIGHTEDMEAN ? sp.a + 1 : sp.a;      // tokens 0 .. n - 1 are summed
    float acc[8] = {};
    for (int t0 = wave; t0 < n; t0 += POOL_WAVES * POOL_UNROLL) {
        uint4 raw[POOL_UNROLL];
#pragma unroll
        for (int j = 0; j < POOL_UNROLL; ++j) {
            const int t = t0 + j * POOL_WAVES;
            raw[j] = make_uint4(0u, 0u, 0u, 0u);
            if (live && t < n) raw[j] = *reinterpret_cast<const uint4*>(xs + (long)t * p.C);
        }
#pragma unroll
        for (int j = 0; j < POOL_UNROLL; ++j) {
            const int t = t0 + j * POOL_WAVES;
            if (t < n) {
                float x[8];
                unpack8(raw[j], x);
                const float w = KIND == WKV6_POOL_WEIGHTEDMEAN ? (float)(t + 1) : 1.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(w, x[i], acc[i]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) part[wave - 1][i][lane] = acc[i];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
    const float fa = (float)sp.a;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int q = 0; q < POOL_WAVES - 1; ++q) acc[i] += part[q][i][lane];      // wave order: 0 + 1 + 2 + 3
        acc[i] = KIND == WKV6_POOL_WEIGHTEDMEAN ? acc[i] / fa / fa : acc[i] / fa;
    }
    *dst = pack8(acc);
}

template <int KIND> __global__ __launch_bounds__(256) void pool_bwd_kernel(PoolArgs p)
{
    const long row = blockIdx.x;
    const int s = seq_of_row(p.cu, p.n_seq, row);
    bool summed = false;
    float w = 1.f;
    if (s >= 0) {
        const Span sp = span_of(p, s);
        if (row >= sp.start && row < (long)sp.start + sp.len) {
            const int t = (int)(row - sp.start);
            const float fa = (float)sp.a;
            if (KIND == WKV6_POOL_WEIGHTEDMEAN) {
                summed = t <= sp.a;
                w = sp.a == 0 ? __builtin_nanf("") : (float)(t + 1) / fa / fa;
            } else if (KIND == WKV6_POOL_AVG) {
                summed = t < sp.a;
                w = 1.f / fa;
            } else {
                summed = t == sp.a;
            }
        }
    }
    const uint4* const g = reinterpret_cast<const uint4*>(p.in + (long)max(s, 0) * p.C);
    uint4* const dst = reinterpret_cast<uint4*>(p.out + row * p.C);
    for (int c = threadIdx.x; c < p.C / 8; c += blockDim.x) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (summed) {
            v = g[c];
            if (KIND != WKV6_POOL_LASTTOKEN) {
                float x[8];
                unpack8(v, x);
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] *= w;
                v = pack8(x);
            }
        }
        dst[c] = v;
    }
}

hipError_t launch_pool(const PoolArgs& p, int kind, bool bwd, hipStream_t st)
{
    if (bwd) {
        const dim3 grid((unsigned)p.total_T), block(min(256, (p.C / 8 + 63) / 64 * 64));
        if (kind == WKV6_POOL_WEIGHTEDMEAN) return launch<pool_bwd_kernel<WKV6_POOL_WEIGHTEDMEAN>>(grid, block, 0, st, p);
        if (kind == WKV6_POOL_AVG) return launch<pool_bwd_kernel<WKV6_POOL_AVG>>(grid, block, 0, st, p);
        return launch<pool_bwd_kernel<WKV6_POOL_LASTTOKEN>>(grid, block, 0, st, p);
    }
    const dim3 grid((unsigned)(p.n_seq * p.ncb)), block(POOL_WAVES * 64);
    if (kind == WKV6_POOL_WEIGHTEDMEAN) return launch<pool_fwd_kernel<WKV6_POOL_WEIGHTEDMEAN>>(grid, block, 0, st, p);
    if (kind == WKV6_POOL_AVG) return launch<pool_fwd_kernel<WKV6_POOL_AVG>>(grid, block, 0, st, p);
    return launch<pool_fwd_kernel<WKV6_POOL_LASTTOKEN>>(grid, block, 0, st, p);
}

}  // namespace

}  // namespace wkv6

using namespace wkv6;

extern "C" {

// ---- the entry points (include/wkv6_amd.h); the order of the refusals is part of the contract
static int pool_packed(bool bwd, long total_T, int n_seq, int C, int kind, const int* cu_seqlens, const int* actual_len, const void* in,
                       void* out, void* stream)
{
    if (total_T < 1 || n_seq < 1 || C < 8 || C % 8) return WKV6_EINVAL;
    if (kind != WKV6_POOL_WEIGHTEDMEAN && kind != WKV6_POOL_LASTTOKEN && kind != WKV6_POOL_AVG) return WKV6_EINVAL;
    const int ncb = (C + POOL_COLS - 1) / POOL_COLS;
    if (total_T > 0x7fffffffL || (long)n_seq * ncb > 0x7fffffffL) return WKV6_EUNSUPPORTED;      // cu_seqlens is int32; the forward's grid
    if (!cu_seqlens || !in || !out) return WKV6_ENULL;
    if (((uintptr_t)in | (uintptr_t)out) & 15) return WKV6_EINVAL;
    if (((uintptr_t)cu_seqlens | (uintptr_t)actual_len) & 3) return WKV6_EINVAL;
    PoolArgs p = {};
    p.total_T = total_T; p.n_seq = n_seq; p.C = C; p.ncb = ncb;
    p.cu = cu_seqlens; p.actual = actual_len;
    p.in = reinterpret_cast<const bf16_t*>(in); p.out = reinterpret_cast<bf16_t*>(out);
    return to_rc(launch_pool(p, kind, bwd, (hipStream_t)stream));
}
int wkv6_pool_packed_forward(long total_T, int n_seq, int C, int kind, const int* cu_seqlens, const int* actual_len, const void* x, void* out,
                             void* stream)
{
    return pool_packed(false, total_T, n_seq, C, kind, cu_seqlens, actual_len, x, out, stream);
}
int wkv6_pool_packed_backward(long total_T, int n_seq, int C, int kind, const int* cu_seqlens, const int* actual_len, const void* gout, void* gx,
                              void* stream)
{
    return pool_packed(true, total_T, n_seq, C, kind, cu_seqlens, actual_len, gout, gx, stream);
}

}  // extern "C"
