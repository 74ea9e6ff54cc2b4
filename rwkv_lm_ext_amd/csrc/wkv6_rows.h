// Rows of [n, V] logits streamed 16 bytes per lane: what the sampler (wkv6_sample.hip), the beam-search row kernel (wkv6_beam.hip) and the
// cross-entropy kernels (wkv6_ce.hip) share -- the 8-element loads and stores, and behind them the streamed-row radix selection of the
// sampler and the beam kernel: one workgroup of 1024 threads per row, the row in neither registers nor LDS, every pass streaming it again.
// Everything here is integer arithmetic or moves data: the two files set `#pragma clang fp contract(off)` behind their includes, and every
// floating-point expression of a score or a weight is written there and comes here as a callable.
#pragma once
#include "wkv6_common.h"

namespace wkv6 {

// ---- 8 consecutive elements of a row as fp32
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&x)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&x)[8])
{
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&x)[8])
{
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u raw = *reinterpret_cast<const v4u*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = bf_lo(raw[i]); x[2 * i + 1] = bf_hi(raw[i]); }
}
template <> __device__ __forceinline__ void load8<f16_t>(const f16_t* p, float (&x)[8])
{
    typedef f16_t h8 __attribute__((ext_vector_type(8)));
    const h8 raw = *reinterpret_cast<const h8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (float)raw[i];
}
template <typename T> __device__ __forceinline__ float load1(const T* p) { return (float)*p; }
template <> __device__ __forceinline__ float load1<bf16_t>(const bf16_t* p) { return __uint_as_float((unsigned)*p << 16); }

// ---- and back: one rounding to nearest even into the row's type
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&x)[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&x)[8])
{
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(x[4], x[5], x[6], x[7]);
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&x)[8])
{
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf2(x[0], x[1]), pack_bf2(x[2], x[3]), pack_bf2(x[4], x[5]), pack_bf2(x[6], x[7]));
}
template <> __device__ __forceinline__ void store8<f16_t>(f16_t* p, const float (&x)[8])
{
    typedef f16_t h8 __attribute__((ext_vector_type(8)));
    const h8 raw = {(f16_t)x[0], (f16_t)x[1], (f16_t)x[2], (f16_t)x[3], (f16_t)x[4], (f16_t)x[5], (f16_t)x[6], (f16_t)x[7]};
    *reinterpret_cast<h8*>(p) = raw;
}
template <typename T> __device__ __forceinline__ void store1(T* p, float x) { *p = (T)x; }
template <> __device__ __forceinline__ void store1<bf16_t>(bf16_t* p, float x) { *p = (bf16_t)(pack_bf2(x, 0.f) & 0xffffu); }

// ================================ streamed-row radix selection (wkv6_sample.hip, wkv6_beam.hip) ================================
typedef unsigned long long u64;

constexpr int ROW_THREADS = 1024, ROW_WAVES = ROW_THREADS / 64;      // one workgroup per row
constexpr float FIX = 70368744177664.f;                              // 2^46: a weight in [0, 1] is summed as the integer floor(w * 2^46)
constexpr float NEG_INF = -__builtin_inff();

// ---- the monotone key of a (non-NaN) float: a > b  <=>  key(a) > key(b); no float has key 0 but a NaN
__device__ __forceinline__ unsigned key_of(float z)
{
    const unsigned b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float z_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- f(n, x, o) for every token n < V of the row lg with the occurrence row occ (null: o = 0, nothing is loaded), thread t on the chunks
// of 8 tokens t, t + 1024, ...  The loads of BATCH chunks are issued before the first of them is used: a pass is a handful of dependent
// round trips to L2 per thread, and this is what keeps them from queueing one behind the other.
template <int BATCH, typename T, typename F> __device__ __forceinline__ void for_each_row_token(const T* lg, const float* occ, int V, int nch, F f)
{
    for (int c0 = threadIdx.x; c0 < nch; c0 += BATCH * ROW_THREADS) {
        float x[BATCH][8], o[BATCH][8];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int c = c0 + u * ROW_THREADS;
            if (c < nch) {
                load8<T>(lg + 8 * c, x[u]);
                if (occ) load8<float>(occ + 8 * c, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int c = c0 + u * ROW_THREADS;
            if (c < nch) {
                __builtin_assume(8 * c < V);                 // nch = ceil(V / 8): a chunk's first token is there
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (8 * c + j < V) f(8 * c + j, x[u][j], occ ? o[u][j] : 0.f);
            }
        }
    }
}

// ---- workgroup and wave primitives.  Integer maxima and sums: any order gives the same bits.
__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const u64 t = __shfl_xor(v, off);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <bool SUM> __device__ __forceinline__ u64 block_reduce(u64 v, u64* red)       // red[ROW_WAVES]
{
    v = SUM ? wave_sum(v) : wave_max(v);
    __syncthreads();                                         // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 m = red[0];
#pragma unroll
    for (int w = 1; w < ROW_WAVES; ++w) m = SUM ? m + red[w] : (red[w] > m ? red[w] : m);
    return m;
}
template <typename N> __device__ __forceinline__ N wave_inclusive_scan(N v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const N t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// ---- one digit of a radix selection over a 256-bin histogram of N = u64 (masses) or unsigned (counts)
template <typename N> struct Pick { unsigned digit; N above, equal; };
// One wave: the largest bin d of hist[256] with hist[d] > 0 and above + sum_{d' >= d} hist[d'] >= target; where there is none (rounding,
// or fewer entries than the target), the smallest bin with hist[d] > 0 (an empty histogram: bin 0).  .above: `above` plus everything in
// the bins over d; .equal: hist[d].
template <typename N> __device__ __forceinline__ Pick<N> select_bin(const N* hist, N above, N target)
{
    const int lane = threadIdx.x & 63;
    N h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = hist[255 - (4 * lane + j)];         // lane 0 holds the top four bins
    const N mine = h[0] + h[1] + h[2] + h[3];
    int first = -1, last = -1;
    N first_above = 0, first_equal = 0, last_above = 0, last_equal = 0, acc = above + wave_inclusive_scan(mine, lane) - mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (h[j] > 0) {
            if (first < 0 && acc + h[j] >= target) { first = 255 - (4 * lane + j); first_above = acc; first_equal = h[j]; }
            last = 255 - (4 * lane + j); last_above = acc; last_equal = h[j];
        }
        acc += h[j];
    }
    const u64 hit = __ballot(first >= 0), any = __ballot(last >= 0);
    Pick<N> p = {0u, above, 0};
    if (hit) {
        const int src = __ffsll((long long)hit) - 1;
        p.digit = (unsigned)__shfl(first, src); p.above = __shfl(first_above, src); p.equal = __shfl(first_equal, src);
    } else if (any) {
        const int src = 63 - __clzll((long long)any);
        p.digit = (unsigned)__shfl(last, src); p.above = __shfl(last_above, src); p.equal = __shfl(last_equal, src);
    }
    return p;
}

// a thread's run of equal digits is added to the histogram once (the top digit of a row's keys takes a handful of values)
template <typename N> struct Run {
    unsigned digit = 0;
    N sum = 0;
    __device__ __forceinline__ void add(N* hist, unsigned d, N v)
    {
        if (d != digit) { flush(hist); digit = d; }
        sum += v;
    }
    __device__ __forceinline__ void flush(N* hist)
    {
        if (sum) atomicAdd(&hist[digit], sum);
        sum = 0;
    }
};

// One pass of a selection with one histogram: zero it, walk the row -- walk(add) calls add(digit, amount) for every token that takes part
// --, flush, wave 0 selects against `target` with `above` already counted, and every thread gets the pick (published through *slot).
template <typename N, typename W> __device__ __forceinline__ Pick<N> radix_step(N* hist, Pick<N>* slot, N above, N target, W walk)
{
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    Run<N> run;
    walk([&](unsigned digit, N amount) { run.add(hist, digit, amount); });
    run.flush(hist);
    __syncthreads();
    if (threadIdx.x < 64) {
        const Pick<N> p = select_bin(hist, above, target);
        if (threadIdx.x == 0) *slot = p;
    }
    __syncthreads();
    return *slot;
}

// The ties at a boundary key: of the tokens there the `keep` lowest ids stay.  Where that is not all of them, the same selection over
// 65535 - n (two passes) finds the last id that stays: tokens at the boundary stay while 65535 - n >= the value returned.  walk(at) calls
// at(n) for every token n that sits at the boundary key.
template <typename N, typename W> __device__ __forceinline__ unsigned tie_cut(N* hist, Pick<N>* slot, N keep, W walk)
{
    unsigned rid_cut = 0;
    N above_id = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = 8 - 8 * pass;
        const Pick<N> p = radix_step(hist, slot, above_id, keep, [&](auto add) {
            walk([&](int n) {
                const unsigned rid = 65535u - (unsigned)n;
                if (pass == 0 || (rid ^ rid_cut) >> 8 == 0) add((rid >> shift) & 255u, (N)1);
            });
        });
        rid_cut |= p.digit << shift;
        above_id = p.above;
    }
    return rid_cut;
}

}  // namespace wkv6
