// LM-head cross-entropy with L2Wrap on [n_rows, V] logits (include/wkv6_amd.h: wkv6_ce_rows_forward_* / _backward_*), hand-written for
// gfx950: what follows head(ln_out(x)) in every language-model training step of the reference (F.cross_entropy, then L2Wrap:
// src/model.py:937-974, 1244-1283).  The header states the operation; this is how it is done.
//
// One workgroup per row, up to 1024 threads (64 per 512 columns, so that a short row does not pay for idle waves); thread t takes the
// chunks of 8 columns t, t + threads, ... as 16-byte loads (two for fp32), four in flight.
// Statistics, one trip through memory: a thread keeps a running (max, argmax, sum of exp(z - max)) and rescales its sum when its max
// moves -- once per chunk at most: the chunk's maximum is taken first --; the triples meet in a fixed-order tree over the wave
// (__shfl_down, lane 0 holds the result) and then over the waves through LDS.  Which column a thread adds when depends on V alone, and
// so does the tree: the same row gives the same bits in any batch.  No atomics.
// Gradient pass: the row is read again (in the fused mode it was streamed a moment ago and sits in L2 / Infinity Cache), p = exp(z - lse)
// is formed and 16 bytes per lane are stored.  A chunk is read and written by the same lane, the load in front of the store, and the
// barriers of the reduction lie between the last read of the statistics pass and the first store: glogits may be the logits buffer.
// Rows that need no logits -- ignored ones, and the NaN rows of a bad target or a non-finite lse -- are written without a load.
#include <cmath>
#include "wkv6_rows.h"
#include "wkv6_host.h"                 // launch<>, to_rc

// the gradient expression is inlined into two kernels (fused forward, backward) and must give the same bits in both
#pragma clang fp contract(off)

namespace wkv6 {
namespace {

constexpr int CE_THREADS = 1024, CE_WAVES = CE_THREADS / 64, CE_UNROLL = 4;
constexpr long long CE_IGNORE = -100;
enum { CE_STATS = 0, CE_FUSED = 1, CE_GRAD = 2 };            // statistics only; statistics and gradient in one launch; gradient from stored statistics

struct CeArgs {
    int V;
    long ld, ld_g;
    const void* logits;              // [n_rows,ld]
    const long long* targets;        // [n_rows]
    float *loss_row, *lse, *zmax;    // [n_rows]: written by the forward, lse and zmax read by the backward
    int* imax;
    const float *ce_scale, *l2_scale;
    void* glogits;                   // [n_rows,ld_g]
};

// (max, lowest column that attains it, sum of exp(z - max)) of a set of columns; the empty set is (-inf, INT_MAX, 0)
struct Stat {
    float m;
    int i;
    float s;
};
// exp(part - whole) for part <= whole, without the inf - inf of two equal infinities
__device__ __forceinline__ float rescale(float part, float whole) { return part == whole ? 1.f : expf(part - whole); }
__device__ __forceinline__ Stat combine(float am, int ai, float as, float bm, int bi, float bs)
{
    const bool take_b = bm > am || (bm == am && bi < ai);
    const float m = take_b ? bm : am;
    Stat r;
    r.m = m;
    r.i = take_b ? bi : ai;
    r.s = as * rescale(am, m) + bs * rescale(bm, m);
    return r;
}
// one level of a tree over the lanes: lane l takes in what lane l + off holds
__device__ __forceinline__ Stat fold_down(Stat v, int off)
{
    return combine(v.m, v.i, v.s, __shfl_down(v.m, off), __shfl_down(v.i, off), __shfl_down(v.s, off));
}
// columns [8 c, 8 c + 8) below V join the thread's triple.  A -inf logit adds 0 (not exp(-inf - -inf)); a NaN is never a maximum and
// poisons the sum; +inf becomes the maximum and poisons the sum as inf - inf.
__device__ __forceinline__ void add_chunk(Stat& st, const float (&x)[8], int c, int V)
{
    float m = st.m;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned n = 8u * (unsigned)c + j;
        if (n < (unsigned)V && x[j] > m) { m = x[j]; st.i = (int)n; }
    }
    if (m != st.m) { st.s = st.s * expf(st.m - m); st.m = m; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned n = 8u * (unsigned)c + j;
        if (n < (unsigned)V && x[j] != NEG_INF) st.s = st.s + expf(x[j] - m);
    }
}

template <typename T, int MODE>
__global__ void __launch_bounds__(CE_THREADS) ce_rows_kernel(const CeArgs a)
{
    __shared__ Stat red[CE_WAVES + 1];                       // one per wave, then the row's
    const long row = blockIdx.x;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, nch = (V - 1) / 8 + 1;
    const T* const lg = static_cast<const T*>(a.logits) + row * a.ld;

    // the target is judged before an address is formed from it
    const long long tgt = a.targets[row];
    const bool ignored = tgt == CE_IGNORE, bad_target = !ignored && (tgt < 0 || tgt >= (long long)V);
    float ce = 0.f, l2 = 0.f;
    if (MODE != CE_STATS) { ce = a.ce_scale[row]; l2 = a.l2_scale[row]; }
    const bool untouched = MODE != CE_STATS && ignored && l2 == 0.f;      // nothing of this row is read

    Stat st = {NEG_INF, 0x7fffffff, 0.f};
    float lse = 0.f;
    if (MODE == CE_GRAD) {
        if (!untouched) { st.m = a.zmax[row]; st.i = a.imax[row]; lse = a.lse[row]; }
    } else if (untouched) {
        if (tid == 0) { a.loss_row[row] = 0.f; a.lse[row] = 0.f; a.zmax[row] = 0.f; a.imax[row] = 0; }
    } else {
        const float zt = tid == 0 && !ignored && !bad_target ? load1<T>(lg + tgt) : 0.f;   // read in front of the barriers: in place the
                                                                                             // gradient pass overwrites it
        for (int c0 = tid; c0 < nch; c0 += nthr * CE_UNROLL) {
            float x[CE_UNROLL][8];
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u)
                if (c0 + u * nthr < nch) load8<T>(lg + 8L * (c0 + u * nthr), x[u]);
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u)
                if (c0 + u * nthr < nch) add_chunk(st, x[u], c0 + u * nthr, V);
        }
        // the wave's lanes, then the workgroup's waves: two trees of a fixed shape, the result in lane 0 of wave 0
#pragma unroll
        for (int off = 32; off; off >>= 1) st = fold_down(st, off);
        if (lane == 0) red[wave] = st;
        __syncthreads();
        if (wave == 0) {
            const bool has = lane < (nthr >> 6);
            st.m = has ? red[lane].m : NEG_INF; st.i = has ? red[lane].i : 0x7fffffff; st.s = has ? red[lane].s : 0.f;
#pragma unroll
            for (int off = CE_WAVES / 2; off; off >>= 1) st = fold_down(st, off);
            if (lane == 0) red[CE_WAVES] = st;
        }
        __syncthreads();
        st = red[CE_WAVES];
        // a row with a NaN (the sum is NaN), a +inf (inf - inf) or no finite logit at all has no lse
        lse = st.m > NEG_INF && st.m < __builtin_inff() ? st.m + logf(st.s) : __builtin_nanf("");
        if (st.i == 0x7fffffff) st.i = 0;
        if (tid == 0) {
            a.loss_row[row] = ignored ? 0.f : bad_target ? __builtin_nanf("") : lse - zt;
            a.lse[row] = lse; a.zmax[row] = st.m; a.imax[row] = st.i;
        }
    }
    if (MODE == CE_STATS) return;

    // ---- the gradient row: every column below V is written
    T* const g = static_cast<T*>(a.glogits) + row * a.ld_g;
    const bool nan_row = bad_target || (!untouched && lse != lse);
    const bool reads = !ignored && !nan_row;
    const float l2z = l2 * st.m;
    const int itgt = ignored || bad_target ? -1 : (int)tgt, imax = untouched ? -1 : st.i;
    for (int c0 = tid; c0 < nch; c0 += nthr * CE_UNROLL) {
        float x[CE_UNROLL][8];
        if (reads) {
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u)
                if (c0 + u * nthr < nch) load8<T>(lg + 8L * (c0 + u * nthr), x[u]);
        }
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            const int c = c0 + u * nthr;
            if (c >= nch) continue;
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = (int)(8u * (unsigned)c + j);
                float v = 0.f;
                if (reads) v = ce * (expf(x[u][j] - lse) - (n == itgt ? 1.f : 0.f));
                if (n == imax) v = v + l2z;
                o[j] = nan_row ? __builtin_nanf("") : v;
            }
            if (8u * (unsigned)c + 8u <= (unsigned)V) {
                store8<T>(g + 8L * c, o);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (8u * (unsigned)c + j < (unsigned)V) store1<T>(g + 8L * c + j, o[j]);
            }
        }
    }
}

template <typename T> hipError_t launch_ce_mode(const CeArgs& a, int mode, dim3 grid, dim3 block, hipStream_t st)
{
    if (mode == CE_STATS) return launch<ce_rows_kernel<T, CE_STATS>>(grid, block, 0, st, a);
    if (mode == CE_FUSED) return launch<ce_rows_kernel<T, CE_FUSED>>(grid, block, 0, st, a);
    return launch<ce_rows_kernel<T, CE_GRAD>>(grid, block, 0, st, a);
}

hipError_t launch_ce(const CeArgs& a, long n_rows, int mode, int io, hipStream_t st)
{
    const int nch = (a.V - 1) / 8 + 1;
    const dim3 grid((unsigned)n_rows), block(nch >= CE_THREADS ? CE_THREADS : (nch + 63) / 64 * 64);
    if (io == IO_F32) return launch_ce_mode<float>(a, mode, grid, block, st);
    if (io == IO_F16) return launch_ce_mode<f16_t>(a, mode, grid, block, st);
    return launch_ce_mode<bf16_t>(a, mode, grid, block, st);
}

// ---- the entry points (include/wkv6_amd.h); the order of the refusals is part of the contract
int ce_rows(bool bwd, long n_rows, int V, long ld, const void* logits, const long long* targets, float* loss_row, float* lse, float* zmax,
            int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g, int io, void* stream)
{
    const bool grad = bwd || glogits;
    if (n_rows < 1 || V < 1 || ld < V || ld % 8) return WKV6_EINVAL;
    if (grad && (ld_g < V || ld_g % 8)) return WKV6_EINVAL;
    if (n_rows > 0x7fffffffL) return WKV6_EUNSUPPORTED;                     // the grid
    if (!logits || !targets || !lse || !zmax || !imax || (!bwd && !loss_row)) return WKV6_ENULL;
    if (grad && (!glogits || !ce_scale || !l2_scale)) return WKV6_ENULL;
    if (((uintptr_t)logits | (uintptr_t)glogits) & 15) return WKV6_EINVAL;                  // a NULL glogits passes
    if ((uintptr_t)targets & 7) return WKV6_EINVAL;
    if (((uintptr_t)loss_row | (uintptr_t)lse | (uintptr_t)zmax | (uintptr_t)imax) & 3) return WKV6_EINVAL;
    if (grad && (((uintptr_t)ce_scale | (uintptr_t)l2_scale) & 3)) return WKV6_EINVAL;      // without a gradient they are not looked at
    if (grad && !(glogits == logits && ld_g == ld)) {                       // in place is the one defined overlap
        const size_t es = io == IO_F32 ? 4 : 2;
        const uintptr_t lo = (uintptr_t)logits, go = (uintptr_t)glogits;
        if (lo < go + (size_t)n_rows * ld_g * es && go < lo + (size_t)n_rows * ld * es) return WKV6_EINVAL;
    }
    CeArgs a = {};
    a.V = V; a.ld = ld; a.ld_g = ld_g;
    a.logits = logits; a.targets = targets;
    a.loss_row = loss_row; a.lse = lse; a.zmax = zmax; a.imax = imax;
    a.ce_scale = ce_scale; a.l2_scale = l2_scale; a.glogits = glogits;
    return to_rc(launch_ce(a, n_rows, bwd ? CE_GRAD : glogits ? CE_FUSED : CE_STATS, io, (hipStream_t)stream));
}

}  // namespace
}  // namespace wkv6

using namespace wkv6;

extern "C" {

#define WKV6_CE_ENTRY(suffix, io)                                                                                                             \
    int wkv6_ce_rows_forward_##suffix(long n_rows, int V, long ld, const void* logits, const long long* targets, float* loss_row, float* lse, \
                                      float* zmax, int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g,         \
                                      void* stream)                                                                                           \
    {                                                                                                                                         \
        return ce_rows(false, n_rows, V, ld, logits, targets, loss_row, lse, zmax, imax, ce_scale, l2_scale, glogits, ld_g, io, stream);      \
    }                                                                                                                                         \
    int wkv6_ce_rows_backward_##suffix(long n_rows, int V, long ld, const void* logits, const long long* targets, const float* lse,           \
                                       const float* zmax, const int* imax, const float* ce_scale, const float* l2_scale, void* glogits,       \
                                       long ld_g, void* stream)                                                                               \
    {                                                                                                                                         \
        return ce_rows(true, n_rows, V, ld, logits, targets, nullptr, const_cast<float*>(lse), const_cast<float*>(zmax),                      \
                       const_cast<int*>(imax), ce_scale, l2_scale, glogits, ld_g, io, stream);                                                \
    }
WKV6_CE_ENTRY(bf16, IO_BF16)
WKV6_CE_ENTRY(fp16, IO_F16)
WKV6_CE_ENTRY(fp32, IO_F32)
#undef WKV6_CE_ENTRY

}  // extern "C"
