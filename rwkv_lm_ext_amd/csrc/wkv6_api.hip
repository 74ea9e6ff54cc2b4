// extern "C" entry points of librwkv6_amd.so (declared in include/wkv6_amd.h).
#include "../../include/wkv6_amd.h"
#include "wkv6_scan.h"
#include "wkv5_scan.h"
#include "wkv6_sample.h"

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <vector>
#include <cstdint>
#include <cstring>
#include <cmath>

using namespace wkv6;

// ---- launch-shape policy (host side): how many workgroups the chunked kernels run on.  The library's rules decide from the shape and
// the device's CU count; wkv6_set_dispatch() (include/wkv6_amd.h) overrides them, so that tests can reach every mode at small shapes.
namespace wkv6 {
namespace {
std::atomic<int> g_dispatch[4] = {-1, -1, -1, -1};    // by WKV6_DISPATCH_*; -1: the library's own choice
int dispatch_override(int what) { return g_dispatch[what].load(std::memory_order_relaxed); }
}  // namespace

int cu_count()              // compute units of the current device (0: unknown)
{
    static int cus[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    if (!cus[dev]) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        cus[dev] = prop.multiProcessorCount;
    }
    return cus[dev];
}
// two workgroups per (batch, head) when one each would leave at least half of the CUs without work
int want_split(int BH)
{
    if (const int o = dispatch_override(WKV6_DISPATCH_SPLIT); o != -1) return o != 0;
    return 2 * BH <= cu_count();
}
// workgroup slots of the persistent wkv6_bi launches: one per CU at most (0: the halves run as two launches).  An override n >= 1 pins
// min(n, BH) slots, more than the CUs included: the slots never wait for one another (workgroup-private scratch, LDS-only tags), and the
// compact side buffers' slot carve (slot * T * 64) stays inside the [B,T,C] buffers as long as slots <= BH.
int bi_slots(int BH)
{
    if (want_split(BH)) return 0;
    if (dispatch_override(WKV6_DISPATCH_BI_FUSED) == 0) return 0;
    if (const int want = dispatch_override(WKV6_DISPATCH_BI_SLOTS); want >= 1) return BH < want ? BH : want;
    const int cus = cu_count();
    return cus > 0 ? (BH < cus ? BH : cus) : 0;
}
// segments of the two-level forward over T (1: one pass)
int tsplit_segments(const ScanArgs& a)
{
    if (a.lens || a.reverse || a.rev_n || a.order || a.accumulate || a.y_f32 || a.zero_tail || a.dsum || a.gn_out) return 1;
    if (a.g_f32[0] || a.g_f32[1] || a.g_f32[2] || a.g_f32[3]) return 1;
    if (const int want = dispatch_override(WKV6_DISPATCH_TSPLIT); want != -1) {   // 0 / 1 = off, n = exactly n segments (if T divides)
        if (want <= 1) return 1;
        return a.T % (64 * want) == 0 ? want : 1;
    }
    const int cus = cu_count();
    int S = 1;
    while (2 * S <= 16 && (long)a.B * a.H * 2 * S <= cus && a.T % (64 * 2 * S) == 0 && a.T / (2 * S) >= 512) S *= 2;
    return S >= 4 ? S : 1;      // two segments do not pay for the extra state pass (two workgroups per pair serve that case)
}
}  // namespace wkv6

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

int check_shape(int B, int T, int C, int H)
{
    if (B < 1 || T < 1 || C < 1 || H < 1) return WKV6_EINVAL;
    if ((long)H * HEAD != (long)C) return WKV6_EINVAL;      // reference: assert(H*_N_ == C)
    if (((long)T + 64) * C >= (1L << 31)) return WKV6_EUNSUPPORTED; // one sequence (rounded up to whole groups) must stay 32-bit
                                                                  // addressable: per-lane byte offsets of bf16 tensors are 32-bit
    return WKV6_OK;
}

// Scratch for callers that pass no workspace (the reference-signature entry points have no such argument): a stream-ordered
// allocation (hipMallocFromPoolAsync on the caller's stream, hipFreeAsync right behind the launches that use it), so concurrent
// streams never share a buffer and nothing synchronises the device.  The memory comes from a pool this library owns (one per
// device, created on first use), not from the device's default pool, whose settings belong to the host application; the pool
// keeps up to SCRATCH_KEEP bytes between calls (the steady state of ordinary shapes is an O(1) pool hit) and gives the rest back.
// Under stream capture the allocation becomes part of the graph like any other stream-ordered allocation; callers that
// replay graphs should pass a workspace instead (every *_ex entry point takes one).
constexpr unsigned long long SCRATCH_KEEP = 1ull << 30;
struct StreamScratch {
    void* ptr = nullptr;
    hipStream_t st = nullptr;
    static hipMemPool_t pool_of(int dev)
    {
        static std::mutex mu;
        static hipMemPool_t pools[64] = {};
        if (dev < 0 || dev >= 64) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        if (!pools[dev]) {
            hipMemPoolProps props = {};
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = dev;
            hipMemPool_t pool = nullptr;
            if (hipMemPoolCreate(&pool, &props) != hipSuccess) return nullptr;
            unsigned long long keep = SCRATCH_KEEP;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            pools[dev] = pool;
        }
        return pools[dev];
    }
    void* get(size_t bytes, hipStream_t stream)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        st = stream;
        hipMemPool_t pool = pool_of(dev);
        const hipError_t e = pool ? hipMallocFromPoolAsync(&ptr, bytes, pool, st) : hipMallocAsync(&ptr, bytes, st);
        if (e != hipSuccess) ptr = nullptr;
        return ptr;
    }
    ~StreamScratch()
    {
        if (ptr) (void)hipFreeAsync(ptr, st);
    }
};

// lens[b] = 1 + index of the first zero of mask[b][:], or T when the row has no zero
// (cuda/wkv6_bi_cuda.cu:21-69 breaks AFTER processing the first masked token).
__global__ void mask_to_lens_kernel(const int* __restrict__ mask, int* __restrict__ lens, int T)
{
    const int b = blockIdx.x;
    int first = T;                                           // "no zero" sentinel
    for (int t = threadIdx.x; t < T; t += blockDim.x)
        if (mask[(long)b * T + t] == 0) { first = t; break; }
    __shared__ int red[256];
    red[threadIdx.x] = first;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) lens[b] = min(red[0] + 1, T);
}

// order[rank] = b with the rows ranked by decreasing length (ties: by index): workgroups are dispatched in blockIdx order, so the
// longest sequences start first and the short ones fill the tail (list scheduling; ~9 % on ragged batches of 1536 workgroups)
__global__ void length_order_kernel(const int* __restrict__ lens, int* __restrict__ order, int B)
{
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int lb = lens[b];
        int rank = 0;
        for (int o = 0; o < B; ++o) {
            const int lo = lens[o];
            rank += (lo > lb) || (lo == lb && o < b);
        }
        order[rank] = b;
    }
}

// Packed variable-length batches: from cu_seqlens[n_seq + 1] (token boundaries of the sequences in a [total_T, C] tensor), per sequence
//   lens    = clamp(cu[s + 1] - cu[s], 0, max_seqlen), cut so that the row ends at or before total_T,
//   tok_off = clamp(cu[s], 0, total_T),
//   ck_off  = exclusive prefix sum of ceil(lens / 64): the sequence's first checkpoint slot within its head (a sequence whose slots would
//             pass ck_stride -- only a cu_seqlens that is not a partition of [0, total_T) can do that -- is given length 0),
//   order   = the sequences by decreasing length (as length_order_kernel).
// Everything the kernels index with is clamped here, on the device: the host never reads cu_seqlens.
__device__ __forceinline__ void varlen_span(const int* __restrict__ cu, int s, long total_T, int max_seqlen, long& t0, long& len)
{
    const long c0 = cu[s], c1 = cu[s + 1];
    t0 = min(max(c0, 0L), total_T);
    len = min(min(max(c1 - c0, 0L), (long)max_seqlen), total_T - t0);
}

// Rows of the [total_T, C] outputs that no sequence serves -- gap j, j = 0 .. n_seq, lies between the end of sequence j - 1 (row 0 for
// j = 0) and the first row of sequence j (total_T for j = n_seq): the rows before cu[0], from cu[n_seq] on, and what max_seqlen cuts off a
// sequence -- are zeroed, nothing else is written: a batch that covers every row costs each workgroup one look at n_seq + 1 boundaries.
struct VarlenFill {
    void* out[8];                   // y, or gr, gk, gv, gw (of both problems of a pair call)
    int n_out;
    long row_bytes;                 // C * element size: a multiple of 128
};

// Workgroup 0 prepares (one workgroup: `prepare` = 0 skips it, the arrays are already there); workgroups 1 .. gridDim.x - 1 zero the
// gaps, which they take from cu_seqlens by the same rule, so that they need not wait for workgroup 0.
// (the work of workgroups 1 .. gridDim.x - 1 of a preparation launch)
__device__ __forceinline__ void varlen_fill_gaps(const int* __restrict__ cu, int n_seq, long total_T, int max_seqlen, const VarlenFill& fill)
{
    __shared__ long g0[256], g1[256];
    __shared__ int n_gaps;
    const int tid = threadIdx.x;
    const long nfill = gridDim.x - 1, me = (long)(blockIdx.x - 1) * 256 + tid;
    for (long jb = 0; jb <= n_seq; jb += 256) {
        if (tid == 0) n_gaps = 0;
        __syncthreads();
        const long j = jb + tid;
        if (j <= n_seq) {
            long start = 0, end = total_T, t0, len;
            if (j > 0) { varlen_span(cu, (int)j - 1, total_T, max_seqlen, t0, len); start = t0 + len; }
            if (j < n_seq) { varlen_span(cu, (int)j, total_T, max_seqlen, t0, len); end = t0; }
            if (end > start) {
                const int i = atomicAdd(&n_gaps, 1);
                g0[i] = start; g1[i] = end;
            }
        }
        __syncthreads();
        const int n = n_gaps;
        for (int i = 0; i < n; ++i) {
            const long first = g0[i] * fill.row_bytes, n16 = (g1[i] - g0[i]) * fill.row_bytes / 16;
            for (int o = 0; o < fill.n_out; ++o) {
                uint4* const p = reinterpret_cast<uint4*>(reinterpret_cast<char*>(fill.out[o]) + first);
                for (long q = me; q < n16; q += nfill * 256) p[q] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
    }
}
// (the work of workgroup 0 of a preparation launch, 256 threads: lens, tok_off, ck_off and order as described above)
__device__ __forceinline__ void varlen_prepare_rows(const int* __restrict__ cu, int n_seq, long total_T, int max_seqlen, long ck_stride, int* lens,
                                                    int* __restrict__ tok_off, int* __restrict__ ck_off, int* __restrict__ order)
{
    __shared__ long part[256];
    const int tid = threadIdx.x;
    const int per = (n_seq + 255) / 256;
    const int s_begin = min(tid * per, n_seq), s_end = min(s_begin + per, n_seq);
    long slots = 0;
    for (int s = s_begin; s < s_end; ++s) {
        long t0, len;
        varlen_span(cu, s, total_T, max_seqlen, t0, len);
        lens[s] = (int)len;
        tok_off[s] = (int)t0;
        slots += (len + 63) / 64;
    }
    part[tid] = slots;
    __syncthreads();
    long off = 0;
    for (int t = 0; t < tid; ++t) off += part[t];
    for (int s = s_begin; s < s_end; ++s) {
        long n = (lens[s] + 63) / 64;
        if (off + n > ck_stride) { lens[s] = 0; n = 0; }
        ck_off[s] = (int)off;
        off += n;
    }
    __syncthreads();                                         // (one workgroup: its global writes are visible to it behind the barrier)
    for (int s = tid; s < n_seq; s += 256) {
        const int ls = lens[s];
        int rank = 0;
        for (int o = 0; o < n_seq; ++o) {
            const int lo = lens[o];
            rank += (lo > ls) || (lo == ls && o < s);
        }
        order[rank] = s;
    }
}
__global__ __launch_bounds__(256) void varlen_prepare_kernel(const int* __restrict__ cu, int n_seq, long total_T, int max_seqlen, long ck_stride,
                                                             int* lens, int* __restrict__ tok_off, int* __restrict__ ck_off, int* __restrict__ order,
                                                             int prepare, const VarlenFill fill)
{
    if (blockIdx.x != 0) {
        varlen_fill_gaps(cu, n_seq, total_T, max_seqlen, fill);
        return;
    }
    if (!prepare) return;
    varlen_prepare_rows(cu, n_seq, total_T, max_seqlen, ck_stride, lens, tok_off, ck_off, order);
}

// ---- packed stateful inference with long sequences cut over T (rwkv6_forward_varlen_split_bf16).  The item table, in dispatch order:
//   items [0, n_full): the FULL segments (seg_len tokens each) of the split sequences, sequence by sequence -- segment g of sequence s is item
//                      full0[s] + g;
//   items [n_full, n_items): per sequence at most one more -- a split sequence's tail (len % seg_len tokens) or an unsplit sequence whole --
//                      longest first; rest[s] is that item, -1: none.
// A sequence is split when len > seg_len and its full segments (len / seg_len), summed with those of the long sequences in front of it, still
// fit under max_extra = total_T / seg_len -- any partition of total_T tokens fits; so n_full never passes max_extra (the state pass's grid) and
// the table never n_seq + max_extra entries.  A sequence that does not fit (a cu_seqlens that is no partition) runs unsplit.  Sequences
// below INFER_CHUNK_MIN_T tokens get no item: the exact scan serves them from the per-sequence arrays.
struct SegTable {
    int* counts;                    // [2]: n_items, n_full
    int *full0, *rest;              // [n_seq]; full0: -1 = not split
    int *len, *tok, *seq, *pos;     // [n_seq + max_extra] per item: tokens, first row in the packed tensors, sequence, first position in it
    int seg_len;
    long max_extra;
};
__global__ __launch_bounds__(256) void varlen_split_prepare_kernel(const int* __restrict__ cu, int n_seq, long total_T, int max_seqlen, long ck_stride,
                                                                   int* lens, int* __restrict__ tok_off, int* __restrict__ ck_off,
                                                                   int* __restrict__ order, const SegTable tb, const VarlenFill fill)
{
    if (blockIdx.x != 0) {
        varlen_fill_gaps(cu, n_seq, total_T, max_seqlen, fill);
        return;
    }
    varlen_prepare_rows(cu, n_seq, total_T, max_seqlen, ck_stride, lens, tok_off, ck_off, order);
    __syncthreads();
    __shared__ long extra_part[256], full_part[256];
    __shared__ int rest_part[256];
    const int tid = threadIdx.x, seg = tb.seg_len;
    const int per = (n_seq + 255) / 256;
    const int s_begin = min(tid * per, n_seq), s_end = min(s_begin + per, n_seq);
    long extra = 0;
    for (int s = s_begin; s < s_end; ++s) {
        const int len = lens[s];
        if (len > seg) extra += len / seg;
    }
    extra_part[tid] = extra;
    __syncthreads();
    long eoff = 0;
    for (int t = 0; t < tid; ++t) eoff += extra_part[t];
    long nfull = 0;
    int nrest = 0;
    for (int s = s_begin; s < s_end; ++s) {              // first pass: who is split (full0 = 0 / -1 for now), and the two counts
        const int len = lens[s];
        const long e = len > seg ? len / seg : 0;
        const bool cut = e > 0 && eoff + e <= tb.max_extra;
        eoff += e;
        tb.full0[s] = cut ? 0 : -1;
        nfull += cut ? len / seg : 0;
        nrest += (len >= INFER_CHUNK_MIN_T && (cut ? len % seg : len) > 0) ? 1 : 0;
    }
    full_part[tid] = nfull;
    rest_part[tid] = nrest;
    __syncthreads();
    long foff = 0, ftotal = 0;
    int rtotal = 0;
    for (int t = 0; t < 256; ++t) {
        if (t < tid) foff += full_part[t];
        ftotal += full_part[t];
        rtotal += rest_part[t];
    }
    for (int s = s_begin; s < s_end; ++s) {
        if (tb.full0[s] < 0) continue;
        tb.full0[s] = (int)foff;
        foff += lens[s] / seg;
    }
    if (tid == 0) { tb.counts[0] = (int)ftotal + rtotal; tb.counts[1] = (int)ftotal; }
    __syncthreads();
    // the full segments: the workgroup walks the sequences, its threads a sequence's segments
    for (int s = 0; s < n_seq; ++s) {
        const int f0 = tb.full0[s];
        if (f0 < 0) continue;
        const int n = lens[s] / seg, t0 = tok_off[s];
        for (int g = tid; g < n; g += 256) {
            tb.len[f0 + g] = seg; tb.tok[f0 + g] = t0 + g * seg; tb.seq[f0 + g] = s; tb.pos[f0 + g] = g * seg;
        }
    }
    // the tails and the unsplit sequences, longest first: ranked over the sequences (as order[] above), never over the items
    const auto rest_len = [&](int s) {
        const int len = lens[s];
        if (len < INFER_CHUNK_MIN_T) return 0;
        return tb.full0[s] >= 0 ? len % seg : len;
    };
    for (int s = tid; s < n_seq; s += 256) {
        const int rl = rest_len(s);
        if (rl <= 0) { tb.rest[s] = -1; continue; }
        int rank = 0;
        for (int o = 0; o < n_seq; ++o) {
            const int ro = rest_len(o);
            rank += (ro > rl) || (ro == rl && o < s);
        }
        const int it = (int)ftotal + rank, p = lens[s] - rl;
        tb.rest[s] = it;
        tb.len[it] = rl; tb.tok[it] = tok_off[s] + p; tb.seq[it] = s; tb.pos[it] = p;
    }
}

// Entry states of the items of the split sequences, one workgroup per (sequence, head): the arithmetic of tsplit_combine_kernel below over the
// sequence's items -- cur = 2^{dsum_item} (.) cur + A_item, from the sequence's source slot (validated as state_slot_of does: outside the pool
// means zero).  Sin of EVERY item of a split sequence is written, the first one's being a copy of the source slot: the forward's first item
// then never reads the slot its last item may store to (the in-place update), in whatever order the two workgroups run.  The pool is only read.
__global__ __launch_bounds__(256) void varlen_split_chain_kernel(const float* __restrict__ pool, const int* __restrict__ state_slot, int n_slots,
                                                                 const int* __restrict__ lens, const SegTable tb, const float* __restrict__ A,
                                                                 const float* __restrict__ dsum, float* __restrict__ Sin, int H)
{
    const int s = blockIdx.x / H, h = blockIdx.x % H;
    const int f0 = tb.full0[s];
    if (f0 < 0) return;
    const int len = lens[s], nfull = len / tb.seg_len, rest = tb.rest[s];
    const int slot = state_slot ? state_slot[s] : s;
    const bool have = len > 0 && slot >= 0 && slot < n_slots;
    for (int m = 0; m < HEAD * HEAD / 256; ++m) {
        const int e = threadIdx.x + 256 * m, i = e & (HEAD - 1);       // state layout [j][i]: i = key channel
        float cur = have ? pool[((long)slot * H + h) * HEAD * HEAD + e] : 0.f;
        for (int g = 0; g < nfull; ++g) {
            const long bp = (long)(f0 + g) * H + h;
            Sin[bp * HEAD * HEAD + e] = cur;
            if (g + 1 == nfull && rest < 0) break;                       // (the last item: no state pass ran for it)
            float dl = 0.f;
            for (int q = 0; q < 4; ++q) dl += dsum[(bp * 4 + q) * HEAD + i];
            cur = fmaf(__builtin_amdgcn_exp2f(dl), cur, A[bp * HEAD * HEAD + e]);
        }
        if (rest >= 0) Sin[((long)rest * H + h) * HEAD * HEAD + e] = cur;
    }
}

int to_rc(hipError_t e) { return e == hipSuccess ? WKV6_OK : (int)e; }

// ---- forward over few, long sequences (inference prefill: B*H << CUs): two-level scan over T.  The sequence is cut into S
// segments that run as S times as many workgroups:
//   1. state pass per segment from a zero state: A_seg = the segment's own contribution to the state, and the per-channel sum
//      of its log-decays (ScanArgs::dsum);
//   2. one small kernel chains the segments:  S_in(seg+1) = 2^{dsum_seg} (.) S_in(seg) + A_seg  (the recurrence of
//      cuda/wkv6_cuda.cu:44-57 applied to whole segments), giving every segment its entry state and the final state;
//   3. the ordinary forward per segment from its entry state.
// 1.7x the work of one pass at S times the parallelism.  The backward still walks whole sequences; the forward's checkpoints
// for it keep their whole-sequence layout (ScanArgs::ckpt_segs).
__global__ void tsplit_combine_kernel(const void* s0, int s_f32, long s0_bstride, const float* __restrict__ A,
                                      const float* __restrict__ dsum, float* __restrict__ Sin, void* s_out, int H, int S)
{
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    for (int m = 0; m < HEAD * HEAD / 256; ++m) {
        const int e = threadIdx.x + 256 * m, i = e & (HEAD - 1);       // state layout [j][i]: i = key channel
        float cur = 0.f;
        if (s0) {
            const long o = (long)b * s0_bstride + (long)h * HEAD * HEAD + e;
            cur = s_f32 ? reinterpret_cast<const float*>(s0)[o] : bf_lo((uint32_t)reinterpret_cast<const bf16_t*>(s0)[o]);
        }
        for (int seg = 0; seg < S; ++seg) {
            const long bp = ((long)b * S + seg) * H + h;
            Sin[bp * HEAD * HEAD + e] = cur;
            float dl = 0.f;
            for (int q = 0; q < 4; ++q) dl += dsum[(bp * 4 + q) * HEAD + i];
            cur = fmaf(__builtin_amdgcn_exp2f(dl), cur, A[bp * HEAD * HEAD + e]);
        }
        if (s_out) {
            const long o = ((long)b * H + h) * HEAD * HEAD + e;
            if (s_f32) reinterpret_cast<float*>(s_out)[o] = cur;
            else reinterpret_cast<bf16_t*>(s_out)[o] = (bf16_t)(pack_bf2(cur, 0.f) & 0xffffu);
        }
    }
}

// segment entry states of a two-level forward: state pass per segment from zero (A, dsum), chained by tsplit_combine_kernel
hipError_t tsplit_entry_states(const ScanArgs& a, int S, float* A, float* Sin, float* dsum, hipStream_t st)
{
    ScanArgs p = a;
    p.B = a.B * S; p.T = a.T / S;
    p.s0 = nullptr; p.s0_bstride = 0; p.s_out = A; p.state_f32 = 1; p.y = nullptr; p.dsum = dsum; p.ckpt = nullptr;
    if (hipError_t e = launch_chunk_state_pass(p, st)) return e;
    hipLaunchKernelGGL(tsplit_combine_kernel, dim3(a.B * a.H), dim3(256), 0, st, a.s0, a.state_f32, a.s0_bstride, A, dsum, Sin,
                       a.s_out, a.H, S);
    return hipGetLastError();
}

hipError_t chunk_forward(const ScanArgs& a_, hipStream_t st)
{
    ScanArgs a = a_;
    const int S = tsplit_segments(a);
    if (S <= 1) return launch_chunk_fwd(a, st);
    const size_t nstate = (size_t)a.B * S * a.H * HEAD * HEAD;                 // floats
    const size_t ndsum = (size_t)a.B * S * a.H * 4 * HEAD;
    StreamScratch scratch;
    float* const buf = reinterpret_cast<float*>(scratch.get((2 * nstate + ndsum) * sizeof(float), st));
    if (!buf) return hipErrorOutOfMemory;
    float* const A = buf, * const Sin = buf + nstate, * const dsum = buf + 2 * nstate;
    if (hipError_t e = tsplit_entry_states(a, S, A, Sin, dsum, st)) return e;
    ScanArgs p = a;
    p.B = a.B * S; p.T = a.T / S;
    p.s0 = Sin; p.s0_bstride = (long)a.H * HEAD * HEAD; p.state_f32 = 1; p.s_out = nullptr;
    p.ckpt_segs = S;                               // checkpoints (training forward) land in the whole sequences' slots
    return launch_chunk_fwd(p, st);
}

// ---- backward over few, long sequences as a two-level scan over T: the S segments of a sequence run as S
// workgroups.  What a segment needs from beyond its end is closed-form:
//   * the adjoint state G entering it from the future.  G_t = d_t (.) G_{t+1} + r_t gy_t^T is the forward recurrence
//     S_{t+1} = d_t (.) S_t + k_t v_t^T read backwards with k := r, v := gy: the state-only pass of the forward kernel over the
//     reversed segment gives its own contribution from a zero end state (and the decay sums), and the chaining kernel walks
//     the segments last to first, G_start(seg) = 2^{dsum_seg} (.) G_end(seg) + A_seg;  G_start(first) is gs;
//   * the gw suffix sum beyond its end: a_s - b_s = Phi_s - Phi_{s+1} with Phi_s[i] = sum_j G_s[i][j] S_s[i][j] (G_s the adjoint of
//     the state S_s in front of token s), so sum_{s >= end} (a_s - b_s) = Phi_end, from the entering G and the forward checkpoint at
//     the boundary;
//   * gu sums over the segments.
__global__ void tsplit_combine_rev_kernel(const float* __restrict__ A, const float* __restrict__ dsum, const float* __restrict__ ckpt,
                                          float* __restrict__ Gin, float* __restrict__ phi, void* gs, int gs_f32, int H, int S,
                                          long nslots_seg, int C)
{
    const int bh = blockIdx.x, b = bh / H, h = bh % H, tid = threadIdx.x;
    __shared__ float red[256];
    float cur[HEAD * HEAD / 256];
    for (int m = 0; m < HEAD * HEAD / 256; ++m) cur[m] = 0.f;
    for (int seg = S - 1; seg >= 0; --seg) {
        const long bp = ((long)b * S + seg) * H + h;
        float part = 0.f;
        // forward state at this segment's end = the checkpoint at the next segment's start (row order, wkv6_scan.h)
        const float* const ck = ckpt + (((long)(b * H + h) * S + (seg + 1)) * nslots_seg) * (HEAD * HEAD);
        for (int m = 0; m < HEAD * HEAD / 256; ++m) {
            const int e = tid + 256 * m, i = e & (HEAD - 1), j = e >> 6;          // state layout [j][i]
            Gin[bp * HEAD * HEAD + e] = cur[m];
            if (seg < S - 1) {
                const int jt = 2 * (j >> 5) + ((j >> 2) & 1), gb = (j >> 3) & 3, qb = j & 3;
                part = fmaf(cur[m], ck[((((i >> 4) * 4 + jt) * 64 + 16 * gb + (i & 15)) << 2) + qb], part);
            }
        }
        red[tid] = part;                                  // the four threads tid, tid + 64, ... share key row i = tid & 63
        __syncthreads();
        if (tid < HEAD) phi[((long)b * S + seg) * C + h * HEAD + tid] = red[tid] + red[tid + 64] + red[tid + 128] + red[tid + 192];
        __syncthreads();
        for (int m = 0; m < HEAD * HEAD / 256; ++m) {
            const int e = tid + 256 * m, i = e & (HEAD - 1);
            float dl = 0.f;
            for (int q = 0; q < 4; ++q) dl += dsum[(bp * 4 + q) * HEAD + i];
            cur[m] = fmaf(__builtin_amdgcn_exp2f(dl), cur[m], A[bp * HEAD * HEAD + e]);
        }
    }
    if (gs) {
        for (int m = 0; m < HEAD * HEAD / 256; ++m) {
            const long o = ((long)b * H + h) * HEAD * HEAD + tid + 256 * m;
            if (gs_f32) reinterpret_cast<float*>(gs)[o] = cur[m];
            else reinterpret_cast<bf16_t*>(gs)[o] = (bf16_t)(pack_bf2(cur[m], 0.f) & 0xffffu);
        }
    }
}
__global__ void tsplit_gu_kernel(const float* __restrict__ part, void* gu, int gu_f32, int S, int C)
{
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int seg = 0; seg < S; ++seg) s += part[((long)b * S + seg) * C + c];
        if (gu_f32) reinterpret_cast<float*>(gu)[(long)b * C + c] = s;
        else reinterpret_cast<bf16_t*>(gu)[(long)b * C + c] = (bf16_t)(pack_bf2(s, 0.f) & 0xffffu);
    }
}

hipError_t chunk_backward(const ScanArgs& a_, hipStream_t st)
{
    ScanArgs a = a_;
    const int S = tsplit_segments(a);
    if (S <= 1) return launch_chunk_bwd(a_, st);
    const int Ts = a.T / S;
    const size_t nstate = (size_t)a.B * S * a.H * HEAD * HEAD, ndsum = (size_t)a.B * S * a.H * 4 * HEAD, nrow = (size_t)a.B * S * a.C;
    StreamScratch scratch;
    float* const buf = reinterpret_cast<float*>(scratch.get((2 * nstate + ndsum + 2 * nrow) * sizeof(float), st));
    if (!buf) return hipErrorOutOfMemory;
    float* const A = buf, * const Gin = buf + nstate, * const dsum = buf + 2 * nstate, * const phi = dsum + ndsum, * const gup = phi + nrow;
    if (!a.ckpt_valid) {                               // self-contained: the forward's states first (two-level, like chunk_forward)
        ScanArgs f = a;
        f.y = nullptr; f.s_out = nullptr; f.gy = nullptr;
        if (hipError_t e = tsplit_entry_states(f, S, A, Gin, dsum, st)) return e;
        ScanArgs p = f;
        p.B = a.B * S; p.T = Ts;
        p.s0 = Gin; p.s0_bstride = (long)a.H * HEAD * HEAD; p.state_f32 = 1;
        p.ckpt_segs = S;
        if (hipError_t e = launch_chunk_state_pass(p, st)) return e;
    }
    {   // the segments' own adjoint contributions: state-only pass over the reversed segments with k := r, v := gy
        ScanArgs p = a;
        p.B = a.B * S; p.T = Ts;
        p.k = a.r; p.v = a.gy; p.reverse = 1;
        p.s0 = nullptr; p.s0_bstride = 0; p.s_out = A; p.state_f32 = 1; p.y = nullptr; p.dsum = dsum; p.ckpt = nullptr;
        if (hipError_t e = launch_chunk_state_pass(p, st)) return e;
    }
    hipLaunchKernelGGL(tsplit_combine_rev_kernel, dim3(a.B * a.H), dim3(256), 0, st, A, dsum, a.ckpt, Gin, phi, a.gs, a.part_f32, a.H, S,
                       (long)(Ts / 64), a.C);
    if (hipError_t e = hipGetLastError()) return e;
    ScanArgs p = a;
    p.B = a.B * S; p.T = Ts;
    p.s0 = nullptr; p.s0_bstride = 0;
    p.g_in = Gin; p.rc_in = phi; p.ckpt_segs = S; p.ckpt_valid = 1; p.split = 0;
    p.gu = a.gu ? gup : nullptr; p.gs = nullptr; p.part_f32 = 1;
    if (hipError_t e = launch_chunk_bwd12k(p, st)) return e;
    if (a.gu) {
        hipLaunchKernelGGL(tsplit_gu_kernel, dim3(a.B), dim3(256), 0, st, gup, a.gu, a.part_f32, S, a.C);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// forward dispatch: chunked MFMA kernel for bf16 I/O unless the caller forces the exact scan
hipError_t run_fwd(const ScanArgs& a, unsigned flags, hipStream_t st)
{
    if ((flags & WKV6_IO_F32) || (flags & WKV6_ALGO_SCAN)) return launch_scan_fwd(a, (flags & WKV6_IO_F32) ? IO_F32 : IO_BF16, st);
    return chunk_forward(a, st);
}

hipError_t run_bwd(ScanArgs& a, unsigned flags, float* scratch, hipStream_t st)
{
    if ((flags & WKV6_IO_F32) || (flags & WKV6_ALGO_SCAN)) {
        a.aux = scratch;
        return launch_scan_bwd(a, flags & WKV6_IO_F32, st);
    }
    a.ckpt = scratch;
    a.ckpt_valid = (flags & WKV6_CKPT_VALID) ? 1 : 0;
    return chunk_backward(a, st);
}

ScanArgs base_args(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                   const void* w, const void* u, unsigned flags)
{
    ScanArgs a = {};
    a.B = B; a.T = T; a.C = C; a.H = H;
    a.r = r; a.k = k; a.v = v; a.w = w; a.u = u;
    a.wkind = (flags & WKV6_W_RAW) ? 1 : 0;
    a.part_f32 = (flags & WKV6_PARTIALS_F32) ? 1 : 0;
    a.use_u = 1;
    return a;
}

}  // namespace

#if defined(WKV6_STAMP) || defined(WKV6_CLOCK) || defined(WKV6_DEBUG)
namespace wkv6 { unsigned long long* g_stamp_buffer = nullptr; }
extern "C" void wkv6_set_debug_buffer(void* p) { wkv6::g_stamp_buffer = reinterpret_cast<unsigned long long*>(p); }
#endif

namespace wkv6 {
namespace {
__global__ void pass_marker_kernel() {}
// the clock ring: [2 kinds][n_launches][n_slots][4] uint64 of caller-owned device memory; the launchers of one process may run on
// several threads (the autograd engine's), so the ring's description and the launch counts are read and advanced under a lock
struct ClockRing {
    std::mutex mu;
    unsigned long long* buf = nullptr;
    int slots = 0, launches = 0;
    long count[2] = {0, 0};
} g_clock;
}
unsigned long long* clock_claim(int kind, int* slots)
{
    std::lock_guard<std::mutex> lk(g_clock.mu);
    *slots = g_clock.slots;
    if (!g_clock.buf) return nullptr;
    const long n = g_clock.count[kind]++;
    return g_clock.buf + ((size_t)kind * g_clock.launches + (size_t)(n % g_clock.launches)) * g_clock.slots * 4;
}
}

extern "C" {

const char* wkv6_amd_version(void) { return "0.1"; }

void wkv6_set_clock_ring(void* buf, int n_slots, int n_launches)
{
    std::lock_guard<std::mutex> lk(wkv6::g_clock.mu);
    const bool on = buf && n_slots > 0 && n_launches > 0;
    wkv6::g_clock.buf = on ? reinterpret_cast<unsigned long long*>(buf) : nullptr;
    wkv6::g_clock.slots = on ? n_slots : 0;
    wkv6::g_clock.launches = on ? n_launches : 0;
    wkv6::g_clock.count[0] = wkv6::g_clock.count[1] = 0;
}
void wkv6_clock_ring_counts(long* fwd, long* bwd)
{
    std::lock_guard<std::mutex> lk(wkv6::g_clock.mu);
    if (fwd) *fwd = wkv6::g_clock.count[0];
    if (bwd) *bwd = wkv6::g_clock.count[1];
}
int wkv6_pass_marker(void* stream)
{
    hipLaunchKernelGGL(wkv6::pass_marker_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream);
    return to_rc(hipGetLastError());
}
int wkv6_set_dispatch(int what, int value)
{
    if (what < WKV6_DISPATCH_SPLIT || what > WKV6_DISPATCH_BI_SLOTS) return WKV6_EINVAL;
    return wkv6::g_dispatch[what].exchange(value);
}

size_t wkv6_backward_workspace_bytes(int B, int T, int C, int H)
{
    // scan path: one fp32 [B,T,C] array; chunked path: one fp32 64x64 state per CKPT_TOK tokens and head
    const size_t scan = (size_t)B * T * C * sizeof(float);
    const size_t chunk = chunk_ckpt_floats(B, T, H) * sizeof(float);
    return align_up(scan > chunk ? scan : chunk);
}
// wkv6_bi workspace: lens, order | checkpoints / scratch of the forward-direction scan | ... of the reverse-direction scan |
//                    4 fp32 [B,T,C] side buffers (the forward uses the first one for y, the backward all four)
struct BiWorkspace {
    int* lens;
    int* order;
    float* scan[2];
    float* side[4];
};
static size_t bi_side_bytes(int B, int T, int C) { return align_up((size_t)B * T * C * sizeof(float)); }
// the part that lives from the forward to the backward (lens, order, both scans' checkpoints); the four side buffers behind it
// are per-call scratch
size_t wkv6bi_kept_bytes(int B, int T, int C, int H)
{
    return align_up((size_t)2 * B * sizeof(int)) + 2 * wkv6_backward_workspace_bytes(B, T, C, H);
}
static BiWorkspace bi_carve(void* workspace, void* side, int B, int T, int C, int H)
{
    char* p = reinterpret_cast<char*>(workspace);
    BiWorkspace w;
    w.lens = reinterpret_cast<int*>(p);
    w.order = w.lens + B;
    p += align_up((size_t)2 * B * sizeof(int));
    for (int i = 0; i < 2; ++i) { w.scan[i] = reinterpret_cast<float*>(p); p += wkv6_backward_workspace_bytes(B, T, C, H); }
    if (side) p = reinterpret_cast<char*>(side);
    for (int i = 0; i < 4; ++i) { w.side[i] = reinterpret_cast<float*>(p); p += bi_side_bytes(B, T, C); }
    return w;
}
size_t wkv6bi_workspace_bytes(int B, int T, int C, int H)
{
    return wkv6bi_kept_bytes(B, T, C, H) + 4 * bi_side_bytes(B, T, C);
}
// workspace == NULL: everything is stream-ordered scratch for the call; >= wkv6bi_workspace_bytes(): everything is carved from
// it; EXACTLY wkv6bi_kept_bytes(): the caller keeps only the part that must survive until the backward and the `nside` fp32 side
// buffers this call needs are stream-ordered scratch (an explicit choice: any other short size is an undersized buffer and is
// refused, so that a caller sized for an older layout gets WKV6_EWORKSPACE instead of hidden allocations).  Returns false when
// the workspace is refused or the allocation fails.
static bool bi_workspace(void* workspace, size_t workspace_bytes, int nside, int B, int T, int C, int H, hipStream_t st,
                         StreamScratch& scratch, BiWorkspace& ws)
{
    const size_t full = wkv6bi_workspace_bytes(B, T, C, H), kept = wkv6bi_kept_bytes(B, T, C, H);
    if (!workspace) {
        workspace = scratch.get(full, st);
        if (!workspace) return false;
        ws = bi_carve(workspace, nullptr, B, T, C, H);
    } else if (workspace_bytes >= full) {
        ws = bi_carve(workspace, nullptr, B, T, C, H);
    } else if (workspace_bytes == kept) {
        void* const side = scratch.get((size_t)nside * bi_side_bytes(B, T, C), st);
        if (!side) return false;
        ws = bi_carve(workspace, side, B, T, C, H);
    } else {
        return false;
    }
    return true;
}

// The caller's workspace where it gave one of `need` bytes, else stream-ordered scratch of `scratch_need` bytes, released when `scratch`
// goes out of scope.  Null (the workspace is too small, or the allocation failed) is WKV6_EWORKSPACE.
static void* acquire(void* workspace, size_t workspace_bytes, size_t need, StreamScratch& scratch, hipStream_t st, size_t scratch_need)
{
    if (workspace) return workspace_bytes >= need ? workspace : nullptr;
    return scratch.get(scratch_need, st);
}
static void* acquire(void* workspace, size_t workspace_bytes, size_t need, StreamScratch& scratch, hipStream_t st)
{
    return acquire(workspace, workspace_bytes, need, scratch, st, need);
}
// the initial state: one for the whole batch, or one per batch entry (WKV6_S0_PER_BATCH)
static void set_state(ScanArgs& a, const void* s0, unsigned flags)
{
    a.s0 = s0;
    a.s0_bstride = (flags & WKV6_S0_PER_BATCH) ? (long)a.H * HEAD * HEAD : 0;
}
// the per-tensor reversal map: no lengths, no map
static void set_rev(ScanArgs& a, const int* rev_n, unsigned rev_mask)
{
    a.rev_n = rev_n;
    a.rev_mask = rev_n ? rev_mask : 0u;
}

int wkv6_forward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                    const void* w, const void* u, const void* s0, void* s_out, void* y,
                    unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !y) return WKV6_ENULL;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    set_state(a, s0, flags);
    a.s_out = s_out;
    a.y = y;
    return to_rc(run_fwd(a, flags, (hipStream_t)stream));
}

int wkv6_forward_ckpt_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                         const void* w, const void* u, const void* s0, void* s_out, void* y,
                         void* ckpt, size_t ckpt_bytes, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !y || !ckpt) return WKV6_ENULL;
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    if (ckpt_bytes < wkv6_backward_workspace_bytes(B, T, C, H)) return WKV6_EWORKSPACE;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    set_state(a, s0, flags);
    a.s_out = s_out;
    a.y = y;
    a.ckpt = reinterpret_cast<float*>(ckpt);
    return to_rc(chunk_forward(a, (hipStream_t)stream));
}

int wkv6_forward_gn_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const void* u,
                       const void* s0, void* s_out, void* y, void* ckpt, size_t ckpt_bytes, const void* gate, const void* gamma,
                       const void* beta, float eps, void* out, float* stats, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !gate || !gamma || !beta || !out) return WKV6_ENULL;
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    if (ckpt && ckpt_bytes < wkv6_backward_workspace_bytes(B, T, C, H)) return WKV6_EWORKSPACE;
    if (want_split(B * H)) return WKV6_EUNSUPPORTED;      // two workgroups per (batch, head): a head's statistics span both
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    set_state(a, s0, flags);
    a.s_out = s_out;
    a.y = y;
    a.ckpt = reinterpret_cast<float*>(ckpt);
    a.gn_gate = gate; a.gn_gamma = gamma; a.gn_beta = beta; a.gn_eps = eps; a.gn_out = out; a.gn_stats = stats;
    return to_rc(launch_chunk_fwd(a, (hipStream_t)stream));
}

int wkv6_backward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                     const void* w, const void* u, const void* s0, const void* gy, void* gr,
                     void* gk, void* gv, void* gw, void* gu, void* gs, void* workspace,
                     size_t workspace_bytes, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !gy || !gr || !gk || !gv || !gw) return WKV6_ENULL;
    StreamScratch scratch;                     // released (stream-ordered) when this call returns
    workspace = acquire(workspace, workspace_bytes, wkv6_backward_workspace_bytes(B, T, C, H), scratch, (hipStream_t)stream);
    if (!workspace) return WKV6_EWORKSPACE;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    set_state(a, s0, flags);
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu; a.gs = gs;
    return to_rc(run_bwd(a, flags, reinterpret_cast<float*>(workspace), (hipStream_t)stream));
}

// ---- packed variable-length batches -----------------------------------------------------------------------------------------
// workspace: lens, tok_off, ck_off, order (int32 [n_seq] each) | checkpoints [H][ck_stride][4096] fp32, ck_stride = total_T / 64 + n_seq
// (sum_s ceil(len_s / 64) <= total_T / 64 + n_seq for any partition of total_T tokens); the scan path's fp32 [total_T, C] scratch lies
// over the checkpoint area (H * (total_T / 64) * 16 KB = total_T * C * 4 B).
static long varlen_ck_stride(long total_T, int n_seq) { return total_T / CKPT_TOK + n_seq; }
static size_t varlen_int_bytes(int n_seq) { return align_up((size_t)4 * n_seq * sizeof(int)); }
size_t wkv6_varlen_workspace_bytes(long total_T, int n_seq, int C, int H)
{
    if (total_T < 1 || n_seq < 1 || H < 1 || (long)H * HEAD != (long)C) return 0;
    return varlen_int_bytes(n_seq) + align_up((size_t)H * (size_t)varlen_ck_stride(total_T, n_seq) * HEAD * HEAD * sizeof(float));
}
constexpr unsigned VARLEN_FLAGS = WKV6_W_RAW | WKV6_IO_F32 | WKV6_S0_PER_BATCH | WKV6_ALGO_SCAN | WKV6_CKPT_VALID | WKV6_PARTIALS_F32;
// (the rev / pair calls have no initial state: WKV6_S0_PER_BATCH is an unknown bit there)
constexpr unsigned VARLEN_REV_FLAGS = VARLEN_FLAGS & ~(unsigned)WKV6_S0_PER_BATCH;
constexpr unsigned VARLEN_PAIR_FLAGS = WKV6_W_RAW | WKV6_PARTIALS_F32 | WKV6_IO_F32 | WKV6_ALGO_SCAN;     // (the last two: known, refused)
static int varlen_check(long total_T, int n_seq, int max_seqlen, int C, int H, unsigned flags, unsigned known = VARLEN_FLAGS)
{
    if (total_T < 1 || n_seq < 1 || max_seqlen < 1 || C < 1 || H < 1) return WKV6_EINVAL;
    if ((long)H * HEAD != (long)C) return WKV6_EINVAL;
    if (flags & ~known) return WKV6_EINVAL;
    if (total_T > 0x7fffffffL) return WKV6_EUNSUPPORTED;                 // cu_seqlens is int32
    // one ROW must stay 32-bit addressable (per-lane byte offsets; half of that with the fp32 ew decay of the chunked kernels); the row
    // origin is 64-bit, so total_T * C may pass 2^31
    const bool chunked = !(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN));
    const long lim = (chunked && !(flags & WKV6_W_RAW)) ? (1L << 30) : (1L << 31);
    if (((long)max_seqlen + 64) * C >= lim) return WKV6_EUNSUPPORTED;
    return WKV6_OK;
}
// the gaps are zeroed with 16-byte stores (every row is a multiple of 128 bytes, so the base decides)
static bool varlen_aligned(std::initializer_list<const void*> out)
{
    for (const void* p : out)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}
static void varlen_carve(ScanArgs& a, void* workspace, long total_T, int n_seq, float** area)
{
    int* const ints = reinterpret_cast<int*>(workspace);
    a.lens = ints; a.tok_off = ints + n_seq; a.ck_off = ints + 2 * (size_t)n_seq; a.order = ints + 3 * (size_t)n_seq;
    a.ck_stride = varlen_ck_stride(total_T, n_seq);
    *area = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + varlen_int_bytes(n_seq));
}
// One launch: workgroup 0 derives the int arrays (prepare), the others zero the rows of `out` that lie in no sequence -- as many workgroups
// as would zero the whole tensors with eight 16-byte stores per lane and tensor (nobody reads cu_seqlens here, so the launch cannot know
// how much there is to zero), 1024 at the most.
struct FillLaunch { VarlenFill fill; unsigned nwg; };      // the gap-zeroing part of a preparation launch: its arguments and workgroups
static FillLaunch make_fill(long row_bytes, long total_T, std::initializer_list<void*> out)
{
    FillLaunch f = {};
    for (void* p : out) f.fill.out[f.fill.n_out++] = p;
    f.fill.row_bytes = row_bytes;
    const long per_wg = 256L * 16 * 8;
    f.nwg = (unsigned)std::min<long>(1024, (total_T * row_bytes + per_wg - 1) / per_wg);
    return f;
}
static hipError_t varlen_prepare(const ScanArgs& a, const int* cu, long total_T, int max_seqlen, bool prepare, unsigned flags,
                                 std::initializer_list<void*> out, hipStream_t st)
{
    const FillLaunch f = make_fill((long)a.C * ((flags & WKV6_IO_F32) ? 4 : 2), total_T, out);
    hipLaunchKernelGGL(varlen_prepare_kernel, dim3(1 + f.nwg), dim3(256), 0, st, cu, a.B, total_T, max_seqlen, a.ck_stride, const_cast<int*>(a.lens),
                       const_cast<int*>(a.tok_off), const_cast<int*>(a.ck_off), const_cast<int*>(a.order), prepare ? 1 : 0, f.fill);
    return hipGetLastError();
}

// rev_n (device int32 [n_seq], null: no map) / rev_mask: the per-tensor reversal map within every sequence (the *_varlen_rev_ex calls)
static int varlen_forward(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                          const void* v, const void* w, const void* u, const void* s0, void* s_out, void* y, void* workspace,
                          size_t workspace_bytes, const int* rev_n, unsigned rev_mask, unsigned flags, unsigned known, void* stream)
{
    if (int rc = varlen_check(total_T, n_seq, max_seqlen, C, H, flags, known)) return rc;
    if (rev_mask & ~(unsigned)REV_ALL) return WKV6_EINVAL;
    if (!cu_seqlens || !r || !k || !v || !w || !u || !y) return WKV6_ENULL;
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;
    const bool keep = workspace != nullptr;
    // (scratch: the int arrays only: no checkpoints are kept)
    workspace = acquire(workspace, workspace_bytes, wkv6_varlen_workspace_bytes(total_T, n_seq, C, H), scratch, st, varlen_int_bytes(n_seq));
    if (!workspace) return WKV6_EWORKSPACE;
    if (!varlen_aligned({y})) return WKV6_EINVAL;
    ScanArgs a = base_args(n_seq, max_seqlen, C, H, r, k, v, w, u, flags);
    float* area = nullptr;
    varlen_carve(a, workspace, total_T, n_seq, &area);
    set_state(a, s0, flags);
    a.s_out = s_out;
    a.y = y;
    set_rev(a, rev_n, rev_mask);
    if (hipError_t e = varlen_prepare(a, cu_seqlens, total_T, max_seqlen, true, flags, {y}, st)) return to_rc(e);
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) return to_rc(launch_scan_fwd_varlen(a, flags & WKV6_IO_F32, st));
    a.ckpt = keep ? area : nullptr;
    return to_rc(launch_chunk_fwd_varlen(a, false, st));
}

static int varlen_backward(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                           const void* v, const void* w, const void* u, const void* s0, const void* gy, void* gr, void* gk, void* gv,
                           void* gw, void* gu, void* gs, void* workspace, size_t workspace_bytes, const int* rev_n, unsigned rev_mask,
                           unsigned flags, unsigned known, void* stream)
{
    if (int rc = varlen_check(total_T, n_seq, max_seqlen, C, H, flags, known)) return rc;
    if (rev_mask & ~(unsigned)REV_ALL) return WKV6_EINVAL;
    if (!cu_seqlens || !r || !k || !v || !w || !u || !gy || !gr || !gk || !gv || !gw) return WKV6_ENULL;
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;
    if (!workspace && (flags & WKV6_CKPT_VALID)) return WKV6_ENULL;  // the checkpoints live in the workspace
    workspace = acquire(workspace, workspace_bytes, wkv6_varlen_workspace_bytes(total_T, n_seq, C, H), scratch, st);
    if (!workspace) return WKV6_EWORKSPACE;
    if (!varlen_aligned({gr, gk, gv, gw})) return WKV6_EINVAL;
    ScanArgs a = base_args(n_seq, max_seqlen, C, H, r, k, v, w, u, flags);
    float* area = nullptr;
    varlen_carve(a, workspace, total_T, n_seq, &area);
    set_state(a, s0, flags);
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu; a.gs = gs;
    set_rev(a, rev_n, rev_mask);
    const bool scan = flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN);
    // (WKV6_CKPT_VALID on the chunked path: the forward left the int arrays beside its checkpoints; the launch only zeroes the gaps)
    if (hipError_t e = varlen_prepare(a, cu_seqlens, total_T, max_seqlen, scan || !(flags & WKV6_CKPT_VALID), flags, {gr, gk, gv, gw}, st))
        return to_rc(e);
    if (scan) {
        a.aux = area;
        return to_rc(launch_scan_bwd_varlen(a, flags & WKV6_IO_F32, st));
    }
    a.ckpt = area;
    a.ckpt_valid = (flags & WKV6_CKPT_VALID) ? 1 : 0;
    return to_rc(launch_chunk_bwd_varlen(a, st));
}

int wkv6_forward_varlen_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                           const void* v, const void* w, const void* u, const void* s0, void* s_out, void* y, void* workspace,
                           size_t workspace_bytes, unsigned flags, void* stream)
{
    return varlen_forward(total_T, n_seq, max_seqlen, C, H, cu_seqlens, r, k, v, w, u, s0, s_out, y, workspace, workspace_bytes, nullptr, 0u,
                          flags, VARLEN_FLAGS, stream);
}

int wkv6_backward_varlen_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                            const void* v, const void* w, const void* u, const void* s0, const void* gy, void* gr, void* gk, void* gv,
                            void* gw, void* gu, void* gs, void* workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    return varlen_backward(total_T, n_seq, max_seqlen, C, H, cu_seqlens, r, k, v, w, u, s0, gy, gr, gk, gv, gw, gu, gs, workspace,
                           workspace_bytes, nullptr, 0u, flags, VARLEN_FLAGS, stream);
}

int wkv6_forward_varlen_rev_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                               const void* v, const void* w, const void* u, void* y, void* workspace, size_t workspace_bytes,
                               const int* rev_n, unsigned rev_mask, unsigned flags, void* stream)
{
    return varlen_forward(total_T, n_seq, max_seqlen, C, H, cu_seqlens, r, k, v, w, u, nullptr, nullptr, y, workspace, workspace_bytes, rev_n,
                          rev_mask, flags, VARLEN_REV_FLAGS, stream);
}

int wkv6_backward_varlen_rev_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                                const void* v, const void* w, const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw,
                                void* gu, void* workspace, size_t workspace_bytes, const int* rev_n, unsigned rev_mask, unsigned flags,
                                void* stream)
{
    return varlen_backward(total_T, n_seq, max_seqlen, C, H, cu_seqlens, r, k, v, w, u, nullptr, gy, gr, gk, gv, gw, gu, nullptr, workspace,
                           workspace_bytes, rev_n, rev_mask, flags, VARLEN_REV_FLAGS, stream);
}

// The packed pair: both problems over the same sequences.  s[i].ckpt / ckpt_bytes is one wkv6_varlen_workspace_bytes() workspace per
// problem; the prepared int arrays (which both problems read) live in s[0]'s.  The forward may keep no checkpoints (either ckpt null; the
// int arrays then live in stream-ordered scratch when s[0].ckpt is null); the backward needs both, as the forward left them.
static int varlen_pair_args(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu, const void* u, const wkv6_seq_set* s,
                            unsigned flags, bool bwd, ScanArgs (&a)[2], float* (&area)[2])
{
    if (int rc = varlen_check(total_T, n_seq, max_seqlen, C, H, flags, VARLEN_PAIR_FLAGS)) return rc;
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    if (!cu || !u || !s) return WKV6_ENULL;
    const size_t need = wkv6_varlen_workspace_bytes(total_T, n_seq, C, H);
    for (int i = 0; i < 2; ++i) {
        const wkv6_seq_set& q = s[i];
        if (q.rev_mask & ~(unsigned)REV_ALL) return WKV6_EINVAL;
        if (!q.r || !q.k || !q.v || !q.w) return WKV6_ENULL;
        if (bwd ? (!q.gy || !q.gr || !q.gk || !q.gv || !q.gw || !q.ckpt) : !q.y) return WKV6_ENULL;
        if (q.ckpt && q.ckpt_bytes < need) return WKV6_EWORKSPACE;
        if (bwd ? !varlen_aligned({q.gr, q.gk, q.gv, q.gw}) : !varlen_aligned({q.y})) return WKV6_EINVAL;
    }
    for (int i = 0; i < 2; ++i) {
        const wkv6_seq_set& q = s[i];
        a[i] = base_args(n_seq, max_seqlen, C, H, q.r, q.k, q.v, q.w, u, flags);
        set_rev(a[i], q.rev_n, q.rev_mask);
        area[i] = q.ckpt ? reinterpret_cast<float*>(reinterpret_cast<char*>(q.ckpt) + varlen_int_bytes(n_seq)) : nullptr;
        if (bwd) { a[i].gy = q.gy; a[i].gr = q.gr; a[i].gk = q.gk; a[i].gv = q.gv; a[i].gw = q.gw; a[i].gu = q.gu; }
        else a[i].y = q.y;
    }
    return WKV6_OK;
}

int wkv6_forward_varlen_pair_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* u,
                                const wkv6_seq_set* s, unsigned flags, void* stream)
{
    ScanArgs a[2];
    float* area[2];
    if (int rc = varlen_pair_args(total_T, n_seq, max_seqlen, C, H, cu_seqlens, u, s, flags, false, a, area)) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;
    // (the int arrays only: they lead s[0].ckpt, whose size varlen_pair_args has checked, where the caller keeps checkpoints)
    void* const ints = acquire(s[0].ckpt, s[0].ckpt_bytes, varlen_int_bytes(n_seq), scratch, st);
    if (!ints) return WKV6_EWORKSPACE;
    float* unused = nullptr;
    for (int i = 0; i < 2; ++i) {
        varlen_carve(a[i], ints, total_T, n_seq, &unused);
        a[i].ckpt = area[i];
    }
    if (hipError_t e = varlen_prepare(a[0], cu_seqlens, total_T, max_seqlen, true, flags, {s[0].y, s[1].y}, st)) return to_rc(e);
    return to_rc(launch_chunk_fwd_varlen_pair(a[0], a[1], st));
}

int wkv6_backward_varlen_pair_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* u,
                                 const wkv6_seq_set* s, unsigned flags, void* stream)
{
    ScanArgs a[2];
    float* area[2];
    if (int rc = varlen_pair_args(total_T, n_seq, max_seqlen, C, H, cu_seqlens, u, s, flags, true, a, area)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* unused = nullptr;
    for (int i = 0; i < 2; ++i) {
        varlen_carve(a[i], s[0].ckpt, total_T, n_seq, &unused);
        a[i].ckpt = area[i];
        a[i].ckpt_valid = 1;
    }
    // (the forward left the int arrays beside s[0]'s checkpoints: the one preparation launch only zeroes the gaps of all eight outputs)
    if (hipError_t e = varlen_prepare(a[0], cu_seqlens, total_T, max_seqlen, false, flags,
                                      {s[0].gr, s[0].gk, s[0].gv, s[0].gw, s[1].gr, s[1].gk, s[1].gv, s[1].gw}, st))
        return to_rc(e);
    return to_rc(launch_chunk_bwd_varlen_pair(a[0], a[1], st));
}

int wkv6_forward_rev_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w,
                        const void* u, void* y, void* ckpt, size_t ckpt_bytes, const int* rev_n, unsigned rev_mask,
                        unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !y || !rev_n) return WKV6_ENULL;
    if (rev_mask & ~(unsigned)REV_ALL) return WKV6_EUNSUPPORTED;
    if (ckpt && ckpt_bytes < wkv6_backward_workspace_bytes(B, T, C, H)) return WKV6_EWORKSPACE;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    a.y = y;
    set_rev(a, rev_n, rev_mask);
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN))        // exact scan kernels (fp32 I/O, or forced): same index maps, no checkpoints
        return to_rc(launch_scan_fwd(a, (flags & WKV6_IO_F32) ? IO_F32 : IO_BF16, (hipStream_t)stream));
    a.ckpt = reinterpret_cast<float*>(ckpt);
    return to_rc(launch_chunk_fwd(a, (hipStream_t)stream));
}

int wkv6_backward_rev_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w,
                         const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu,
                         void* workspace, size_t workspace_bytes, const int* rev_n, unsigned rev_mask, unsigned flags,
                         void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !gy || !gr || !gk || !gv || !gw || !rev_n) return WKV6_ENULL;
    if (rev_mask & ~(unsigned)REV_ALL) return WKV6_EUNSUPPORTED;
    StreamScratch scratch;                     // released (stream-ordered) when this call returns
    workspace = acquire(workspace, workspace_bytes, wkv6_backward_workspace_bytes(B, T, C, H), scratch, (hipStream_t)stream);
    if (!workspace) return WKV6_EWORKSPACE;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu;
    set_rev(a, rev_n, rev_mask);
    return to_rc(run_bwd(a, flags, reinterpret_cast<float*>(workspace), (hipStream_t)stream));
}

static int pair_args(int B, int T, int C, int H, const void* u, const wkv6_seq_set* s, unsigned flags, bool bwd, ScanArgs (&a)[2])
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!u || !s) return WKV6_ENULL;
    if (flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    const size_t need = wkv6_backward_workspace_bytes(B, T, C, H);
    for (int i = 0; i < 2; ++i) {
        const wkv6_seq_set& q = s[i];
        if (!q.r || !q.k || !q.v || !q.w) return WKV6_ENULL;
        if (bwd ? (!q.gy || !q.gr || !q.gk || !q.gv || !q.gw || !q.ckpt) : !q.y) return WKV6_ENULL;
        if (q.rev_mask & ~(unsigned)REV_ALL) return WKV6_EUNSUPPORTED;
        if (q.ckpt && q.ckpt_bytes < need) return WKV6_EWORKSPACE;
        a[i] = base_args(B, T, C, H, q.r, q.k, q.v, q.w, u, flags);
        a[i].ckpt = reinterpret_cast<float*>(q.ckpt);
        set_rev(a[i], q.rev_n, q.rev_mask);
        if (bwd) {
            a[i].gy = q.gy; a[i].gr = q.gr; a[i].gk = q.gk; a[i].gv = q.gv; a[i].gw = q.gw; a[i].gu = q.gu;
            a[i].ckpt_valid = 1;
        } else {
            a[i].y = q.y;
        }
    }
    return WKV6_OK;
}

int wkv6_forward_pair_ex(int B, int T, int C, int H, const void* u, const wkv6_seq_set* s, unsigned flags, void* stream)
{
    ScanArgs a[2];
    if (int rc = pair_args(B, T, C, H, u, s, flags, false, a)) return rc;
    return to_rc(launch_chunk_fwd_pair(a[0], a[1], (hipStream_t)stream));
}

int wkv6_backward_pair_ex(int B, int T, int C, int H, const void* u, const wkv6_seq_set* s, unsigned flags, void* stream)
{
    ScanArgs a[2];
    if (int rc = pair_args(B, T, C, H, u, s, flags, true, a)) return rc;
    return to_rc(launch_chunk_bwd_pair(a[0], a[1], (hipStream_t)stream));
}

// The chunked halves of wkv6_bi address their fp32 side buffers with 32-bit byte offsets (buffer resources; where two workgroups serve a
// pair the side buffers are [B,T,C] arrays, the one-launch path's are [T][64]).  Measured: the chunked backward agrees with the scan kernels
// at T = 2^23 - 1 (C = 64) and puts gr off at scattered reverse-scan group starts (and gw, through its suffix sum, everywhere) once a row's
// fp32 byte offsets pass 2^31, at T = 2^23 + 4096 and 2^24 - 129 -- so (T + 128) C fp32 elements must stay below 2^31 bytes, not 2^32.
// Longer rows take the exact scan kernels, whose indices are 64-bit -- decided before the call enqueues anything.
static unsigned bi_route(unsigned flags, int T, int C)
{
    if (!(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) && ((long)T + 128) * C >= (1L << 29)) flags |= WKV6_ALGO_SCAN;
    return flags;
}

int wkv6bi_forward_ex(int B, int T, int C, int H, const int* mask, const int* lens, const void* r,
                      const void* k, const void* v, const void* w, const void* u, void* y,
                      void* workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !y || (!mask && !lens)) return WKV6_ENULL;
    flags = bi_route(flags, T, C);             // (before anything is enqueued)
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;                     // released (stream-ordered) when this call returns
    BiWorkspace ws;
    if (!bi_workspace(workspace, workspace_bytes, 1, B, T, C, H, st, scratch, ws)) return WKV6_EWORKSPACE;
    if (!lens) {
        hipLaunchKernelGGL(mask_to_lens_kernel, dim3(B), dim3(256), 0, st, mask, ws.lens, T);
        lens = ws.lens;
    }
    const bool chunked = !(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN));
    const bool keep = (flags & WKV6_BI_KEEP_CKPT) && chunked;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    if (chunked && B > 1 && B <= 4096) {
        hipLaunchKernelGGL(length_order_kernel, dim3(1), dim3(256), 0, st, lens, ws.order, B);
        a.order = ws.order;
    }
    a.y = y;
    a.y_f32 = ws.side[0];                     // the two halves are summed in fp32 and rounded once
    a.lens = lens;
    a.zero_tail = 1;                          // y[t > L_b] = 0 (the reference leaves it uninitialised, Q2)
    a.ckpt = keep ? ws.scan[0] : nullptr;
    ScanArgs a2 = a;
    a2.reverse = 1; a2.use_u = 0; a2.accumulate = 1; a2.zero_tail = 0;   // cuda/wkv6_bi_cuda.cu:71-111
    a2.ckpt = keep ? ws.scan[1] : nullptr;
    if (chunked) {          // both halves in one persistent launch (the fp32 partial of a row stays in the slot's scratch: L2 / Infinity Cache)
        const hipError_t e = launch_chunk_fwd_bi(a, a2, nullptr, st);
        if (e != hipErrorNotSupported) return to_rc(e);
    }
    if (hipError_t e = run_fwd(a, flags, st)) return (int)e;
    return to_rc(run_fwd(a2, flags, st));
}

int wkv6bi_backward_ex(int B, int T, int C, int H, const int* mask, const int* lens, const void* r,
                       const void* k, const void* v, const void* w, const void* u, const void* gy,
                       void* gr, void* gk, void* gv, void* gw, void* gu, void* workspace,
                       size_t workspace_bytes, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !gy || !gr || !gk || !gv || !gw || (!mask && !lens)) return WKV6_ENULL;
    flags = bi_route(flags, T, C);             // (before anything is enqueued)
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;                     // released (stream-ordered) when this call returns
    BiWorkspace ws;
    if (!bi_workspace(workspace, workspace_bytes, 4, B, T, C, H, st, scratch, ws)) return WKV6_EWORKSPACE;
    if (!lens) {
        hipLaunchKernelGGL(mask_to_lens_kernel, dim3(B), dim3(256), 0, st, mask, ws.lens, T);
        lens = ws.lens;
    }
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu;
    a.lens = lens;
    a.zero_tail = 1;
    if (!(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN)) && B > 1 && B <= 4096) {
        hipLaunchKernelGGL(length_order_kernel, dim3(1), dim3(256), 0, st, lens, ws.order, B);
        a.order = ws.order;
    }
    if (!(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN))) {
        // chunked bf16 path: the first half goes to fp32 side buffers, the second adds it and rounds once
        // (the reference accumulates `_gr[t] += F(gr)` in bf16, cuda/wkv6_bi_cuda.cu:199-200)
        for (int i = 0; i < 4; ++i) a.g_f32[i] = ws.side[i];
    }
    if (!(flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN))) {
        // both halves in one persistent launch: the first half's four fp32 partials of a row stay in the slot's scratch
        ScanArgs a1 = a, a2 = a;
        a1.ckpt = ws.scan[0]; a2.ckpt = ws.scan[1];
        a1.ckpt_valid = a2.ckpt_valid = (flags & WKV6_CKPT_VALID) ? 1 : 0;
        a2.reverse = 1; a2.use_u = 0; a2.accumulate = 1; a2.zero_tail = 0; a2.gu = nullptr;
        const hipError_t e = launch_chunk_bwd_bi(a1, a2, nullptr, st);
        if (e != hipErrorNotSupported) return to_rc(e);
    }
    if (hipError_t e = run_bwd(a, flags, ws.scan[0], st)) return (int)e;             // adjoint of the forward scan
    a.reverse = 1; a.use_u = 0; a.accumulate = 1; a.zero_tail = 0; a.gu = nullptr;   // adjoint of the reverse scan
    return to_rc(run_bwd(a, flags, ws.scan[1], st));
}

// ---- wkv5: the static-decay operator (wkv5_scan.h).  Exact token-serial kernels only; no workspace ----------------
int wkv5_forward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const void* u,
                    void* y, unsigned flags, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !y) return WKV6_ENULL;
    if (flags & ~(unsigned)(WKV6_W_RAW | WKV6_IO_F32 | WKV6_PARTIALS_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    Wkv5Args a = {};
    a.B = B; a.T = T; a.C = C; a.H = H;
    a.r = r; a.k = k; a.v = v; a.w = w; a.u = u; a.y = y;
    a.wkind = (flags & WKV6_W_RAW) ? 1 : 0;
    return to_rc(launch_wkv5_fwd(a, flags & WKV6_IO_F32, (hipStream_t)stream));
}
int wkv5_backward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const float* ew,
                     const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu, unsigned flags,
                     void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!r || !k || !v || !w || !u || !gy || !gr || !gk || !gv) return WKV6_ENULL;
    if (!(flags & WKV6_W_RAW) && !ew && gw) return WKV6_ENULL;      // gw = ew (.) d (.) dL/dd needs ew beside the decay
    if (flags & ~(unsigned)(WKV6_W_RAW | WKV6_IO_F32 | WKV6_PARTIALS_F32 | WKV6_ALGO_SCAN)) return WKV6_EUNSUPPORTED;
    Wkv5Args a = {};
    a.B = B; a.T = T; a.C = C; a.H = H;
    a.r = r; a.k = k; a.v = v; a.w = w; a.ew = ew; a.u = u;
    a.wkind = (flags & WKV6_W_RAW) ? 1 : 0;
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu;
    a.part_f32 = (flags & WKV6_PARTIALS_F32) ? 1 : 0;
    return to_rc(launch_wkv5_bwd(a, flags & WKV6_IO_F32, (hipStream_t)stream));
}
int wkv5_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* eew, const void* u,
                      void* y, void* stream)
{
    return wkv5_forward_ex(B, T, C, H, r, k, v, eew, u, y, 0, stream);
}
int wkv5_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* eew, const float* ew,
                       const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu, void* stream)
{
    if (!ew) return WKV6_ENULL;
    return wkv5_backward_ex(B, T, C, H, r, k, v, eew, ew, u, gy, gr, gk, gv, gw, gu, 0, stream);
}

// ---- reference-signature entry points ------------------------------------------------------------
int wkv6_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                      const float* w, const void* u, void* y, void* stream)
{
    return wkv6_forward_ex(B, T, C, H, r, k, v, w, u, nullptr, nullptr, y, WKV6_W_EW_F32, stream);
}
int wkv6_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                       const float* w, const void* u, const void* gy, void* gr, void* gk, void* gv,
                       void* gw, void* gu, void* stream)
{
    return wkv6_backward_ex(B, T, C, H, r, k, v, w, u, nullptr, gy, gr, gk, gv, gw, gu, nullptr,
                            nullptr, 0, WKV6_W_EW_F32, stream);
}
int wkv6bi_cuda_forward(int B, int T, int C, int H, const int* mask, const void* r, const void* k,
                        const void* v, const float* w, const void* u, void* y, void* stream)
{
    return wkv6bi_forward_ex(B, T, C, H, mask, nullptr, r, k, v, w, u, y, nullptr, 0, WKV6_W_EW_F32, stream);
}
int wkv6bi_cuda_backward(int B, int T, int C, int H, const int* mask, const void* r, const void* k,
                         const void* v, const float* w, const void* u, const void* gy, void* gr,
                         void* gk, void* gv, void* gw, void* gu, void* stream)
{
    return wkv6bi_backward_ex(B, T, C, H, mask, nullptr, r, k, v, w, u, gy, gr, gk, gv, gw, gu,
                              nullptr, 0, WKV6_W_EW_F32, stream);
}
int wkv6state_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                           const void* w, const void* u, const void* s, void* y, void* stream)
{
    if (!s) return WKV6_ENULL;
    return wkv6_forward_ex(B, T, C, H, r, k, v, w, u, s, nullptr, y, WKV6_W_RAW, stream);
}
int wkv6state_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                            const void* w, const void* u, const void* s, const void* gy, void* gr,
                            void* gk, void* gv, void* gw, void* gu, void* gs, void* stream)
{
    if (!s) return WKV6_ENULL;
    return wkv6_backward_ex(B, T, C, H, r, k, v, w, u, s, gy, gr, gk, gv, gw, gu, gs, nullptr, 0,
                            WKV6_W_RAW, stream);
}
int wkv6infctx_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                            const void* w, const void* u, void* s, void* y, void* stream)
{
    if (!s) return WKV6_ENULL;
    return wkv6_forward_ex(B, T, C, H, r, k, v, w, u, s, s, y, WKV6_W_RAW | WKV6_S0_PER_BATCH, stream);
}
int wkv6infctx_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                             const void* w, const void* u, const void* s, const void* gy, void* gr,
                             void* gk, void* gv, void* gw, void* gu, void* gs, void* stream)
{
    if (!s) return WKV6_ENULL;
    return wkv6_backward_ex(B, T, C, H, r, k, v, w, u, s, gy, gr, gk, gv, gw, gu, gs, nullptr, 0,
                            WKV6_W_RAW | WKV6_S0_PER_BATCH, stream);
}

static int rwkv6_infer(int B, int T, int C, int H, float* state, const void* r, const void* k, const void* v,
                       const float* w, const void* u, void* y, int io, void* stream)
{
    if (int rc = check_shape(B, T, C, H)) return rc;
    if (!state || !r || !k || !v || !w || !u || !y) return WKV6_ENULL;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, 0);
    a.wkind = 2;                                  // w is the decay itself
    a.state_f32 = 1;
    a.s0 = state; a.s_out = state;
    a.s0_bstride = (long)H * HEAD * HEAD;
    a.y = y;
    // prefill-sized calls in bf16 go through the chunked MFMA kernel (log of the given decay, fp32 state I/O); decode
    // (a few tokens), fp32 I/O and fp16 I/O (r, k, v are not exact in bf16) use the exact scan
    if (io == IO_BF16 && T >= INFER_CHUNK_MIN_T) return to_rc(chunk_forward(a, (hipStream_t)stream));
    return to_rc(launch_scan_fwd(a, io, (hipStream_t)stream));
}
int rwkv6_cuda_forward_bf16(int B, int T, int C, int H, float* state, const void* r, const void* k, const void* v,
                            const float* w, const void* u, void* y, void* stream)
{
    return rwkv6_infer(B, T, C, H, state, r, k, v, w, u, y, IO_BF16, stream);
}
int rwkv6_cuda_forward_fp16(int B, int T, int C, int H, float* state, const void* r, const void* k, const void* v,
                            const float* w, const void* u, void* y, void* stream)
{
    return rwkv6_infer(B, T, C, H, state, r, k, v, w, u, y, IO_F16, stream);
}
int rwkv6_cuda_forward_fp32(int B, int T, int C, int H, float* state, const float* r, const float* k, const float* v,
                            const float* w, const float* u, float* y, void* stream)
{
    return rwkv6_infer(B, T, C, H, state, r, k, v, w, u, y, IO_F32, stream);
}

// ---- packed stateful inference: the sequences of one [total_T, C] buffer, each with its state in a slot of the caller's fp32 pool.
// One preparation launch (lengths, offsets, dispatch order, gap rows of y), then the kernels rwkv6_infer would pick per sequence: bf16
// sequences of INFER_CHUNK_MIN_T tokens and more on the chunked kernel, everything else on the exact scan -- two launches over the same
// prepared arrays, each serving its side of the length window (ScanArgs::len_lo / len_hi), so that the host never reads cu_seqlens.
size_t rwkv6_varlen_workspace_bytes(int n_seq) { return n_seq < 1 ? 0 : varlen_int_bytes(n_seq); }

// rwkv6_forward_varlen_snap_*: the final state goes to slot state_slot_out[s] (NULL: the source slot), and the state after every snap_every
// tokens to a slot of its own -- the SNAP instantiations of the two kernels; everything else as the plain call
struct SnapArgs {
    const int* state_slot_out;
    int snap_every;
    const int *cu_snap, *snap_slot;
    int n_snap;
};

// rwkv6_forward_varlen_split_bf16: behind the int arrays of the plain call, the item table (SegTable) and per item and head the state
// pass's result A (items with a successor: the first max_extra entries), the entry state Sin and the decay sums
struct SplitWorkspace {
    SegTable tb;
    long n_table;                   // bound of the item table
    float *A, *Sin, *dsum;
};
static long split_table_ints(int n_seq, long n_table) { return 2 + 2L * n_seq + 4 * n_table; }
static size_t split_workspace_bytes(long total_T, int n_seq, int seg_len, int H)
{
    const long extra = total_T / seg_len, n_table = n_seq + extra;
    const size_t st = (size_t)H * HEAD * HEAD * sizeof(float);
    return varlen_int_bytes(n_seq) + align_up((size_t)split_table_ints(n_seq, n_table) * sizeof(int)) + align_up((size_t)extra * st)
           + align_up((size_t)n_table * st) + align_up((size_t)extra * H * 4 * HEAD * sizeof(float));
}
static SplitWorkspace split_carve(float* area, long total_T, int n_seq, int seg_len, int H)
{
    SplitWorkspace sw = {};
    const long extra = total_T / seg_len;
    const size_t st = (size_t)H * HEAD * HEAD * sizeof(float);
    sw.n_table = n_seq + extra;
    int* const ints = reinterpret_cast<int*>(area);
    sw.tb.counts = ints;
    sw.tb.full0 = ints + 2; sw.tb.rest = sw.tb.full0 + n_seq;
    sw.tb.len = sw.tb.rest + n_seq; sw.tb.tok = sw.tb.len + sw.n_table; sw.tb.seq = sw.tb.tok + sw.n_table; sw.tb.pos = sw.tb.seq + sw.n_table;
    sw.tb.seg_len = seg_len;
    sw.tb.max_extra = extra;
    char* p = reinterpret_cast<char*>(area) + align_up((size_t)split_table_ints(n_seq, sw.n_table) * sizeof(int));
    sw.A = reinterpret_cast<float*>(p); p += align_up((size_t)extra * st);
    sw.Sin = reinterpret_cast<float*>(p); p += align_up((size_t)sw.n_table * st);
    sw.dsum = reinterpret_cast<float*>(p);
    return sw;
}
// varlen_prepare with the item table (bf16 rows)
static hipError_t varlen_split_prepare(const ScanArgs& a, const int* cu, long total_T, int max_seqlen, const SegTable& tb, void* y, hipStream_t st)
{
    const FillLaunch f = make_fill((long)a.C * 2, total_T, {y});
    hipLaunchKernelGGL(varlen_split_prepare_kernel, dim3(1 + f.nwg), dim3(256), 0, st, cu, a.B, total_T, max_seqlen, a.ck_stride,
                       const_cast<int*>(a.lens), const_cast<int*>(a.tok_off), const_cast<int*>(a.ck_off), const_cast<int*>(a.order), tb, f.fill);
    return hipGetLastError();
}

static int rwkv6_infer_varlen(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                              void* y, void* workspace, size_t workspace_bytes, unsigned flags, int io, void* stream,
                              const SnapArgs* snap = nullptr, int seg_len = 0)
{
    if (flags & ~(unsigned)WKV6_ALGO_SCAN) return WKV6_EINVAL;
    if (seg_len < 0 || seg_len % 64 != 0) return WKV6_EINVAL;
    if (snap) {
        if (snap->snap_every < 0 || snap->snap_every % 64 != 0 || snap->n_snap < 0) return WKV6_EINVAL;
        if (snap->snap_every > 0 && (!snap->cu_snap || !snap->snap_slot)) return WKV6_ENULL;
    }
    const bool chunked = io == IO_BF16 && !(flags & WKV6_ALGO_SCAN) && max_seqlen >= INFER_CHUNK_MIN_T;
    // (varlen_check's row limits: 2^30 on the chunked route with the fp32 decay, 2^31 on the scan route)
    if (int rc = varlen_check(total_T, n_seq, max_seqlen, C, H, chunked ? 0u : (unsigned)WKV6_ALGO_SCAN, WKV6_ALGO_SCAN)) return rc;
    if (n_slots < 1 || (!state_slot && n_slots < n_seq)) return WKV6_EINVAL;
    if (!cu_seqlens || !state_pool || !r || !k || !v || !w || !u || !y) return WKV6_ENULL;
    if (seg_len > 0 && (io != IO_BF16 || (flags & WKV6_ALGO_SCAN))) return WKV6_EUNSUPPORTED;    // the cut exists on the chunked route only
    const bool cut = seg_len > 0 && chunked;                // (no sequence of INFER_CHUNK_MIN_T tokens: nothing to cut, the plain path)
    const size_t need = cut ? split_workspace_bytes(total_T, n_seq, seg_len, H) : rwkv6_varlen_workspace_bytes(n_seq);
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch;
    workspace = acquire(workspace, workspace_bytes, need, scratch, st);
    if (!workspace) return WKV6_EWORKSPACE;
    if (!varlen_aligned({y})) return WKV6_EINVAL;
    ScanArgs a = base_args(n_seq, max_seqlen, C, H, r, k, v, w, u, 0);
    float* area = nullptr;
    varlen_carve(a, workspace, total_T, n_seq, &area);      // (no checkpoint is kept: the area behind the int arrays is never addressed)
    a.wkind = 2;                                            // w is the decay itself
    a.state_f32 = 1;
    a.s0 = state_pool; a.s_out = state_pool;
    a.s0_bstride = (long)H * HEAD * HEAD;
    a.state_slot = state_slot; a.n_slots = n_slots;
    a.y = y;
    SplitWorkspace sw = {};
    if (cut) {
        sw = split_carve(area, total_T, n_seq, seg_len, H);
        if (hipError_t e = varlen_split_prepare(a, cu_seqlens, total_T, max_seqlen, sw.tb, y, st)) return to_rc(e);
    } else if (hipError_t e = varlen_prepare(a, cu_seqlens, total_T, max_seqlen, true, io == IO_F32 ? (unsigned)WKV6_IO_F32 : 0u, {y}, st)) {
        return to_rc(e);
    }
    if (snap) {
        a.state_slot_out = snap->state_slot_out;
        a.snap_every = snap->snap_every; a.cu_snap = snap->cu_snap; a.snap_slot = snap->snap_slot; a.n_snap = snap->n_snap;
    }
    if (cut) {
        // the chunked side of the length window, per item: state pass of the items with a successor, chaining, forward (see SegTable)
        ScanArgs p = a;
        p.lens = sw.tb.len; p.tok_off = sw.tb.tok; p.ck_off = sw.tb.pos; p.order = nullptr;
        SegArgs sg = {sw.tb.counts, sw.tb.seq, sw.tb.pos, a.lens, sw.Sin};
        if (sw.tb.max_extra > 0) {
            ScanArgs q = p;
            q.B = (int)sw.tb.max_extra;                      // (the full segments lead the table; n_full <= max_extra)
            SegArgs sq = sg;
            sq.n = sw.tb.counts + 1;
            q.s0 = nullptr; q.s0_bstride = 0; q.s_out = sw.A; q.y = nullptr; q.dsum = sw.dsum;
            q.state_slot = nullptr; q.n_slots = 0; q.state_slot_out = nullptr; q.snap_every = 0; q.cu_snap = q.snap_slot = nullptr; q.n_snap = 0;
            if (hipError_t e = launch_chunk_fwd_seg(q, sq, true, st)) return to_rc(e);
            hipLaunchKernelGGL(varlen_split_chain_kernel, dim3(n_seq * H), dim3(256), 0, st, state_pool, state_slot, n_slots, a.lens, sw.tb, sw.A,
                               sw.dsum, sw.Sin, H);
            if (hipError_t e = hipGetLastError()) return to_rc(e);
        }
        p.B = (int)sw.n_table;
        if (hipError_t e = launch_chunk_fwd_seg(p, sg, false, st)) return to_rc(e);
        a.len_lo = 0; a.len_hi = INFER_CHUNK_MIN_T;
        return to_rc(launch_scan_fwd_snap(a, io, st));
    }
    if (!chunked) return to_rc(snap ? launch_scan_fwd_snap(a, io, st) : launch_scan_fwd_slots(a, io, st));   // a decode step, fp16 / fp32 I/O, WKV6_ALGO_SCAN: no window
    a.len_lo = INFER_CHUNK_MIN_T; a.len_hi = 0x7fffffff;
    if (hipError_t e = snap ? launch_chunk_fwd_snap(a, st) : launch_chunk_fwd_slots(a, st)) return to_rc(e);
    a.len_lo = 0; a.len_hi = INFER_CHUNK_MIN_T;
    // (SNAP below the window too: no sequence that short has a snapshot, but its final state goes to state_slot_out)
    return to_rc(snap ? launch_scan_fwd_snap(a, io, st) : launch_scan_fwd_slots(a, io, st));
}
int rwkv6_forward_varlen_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                              void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_BF16, stream);
}
int rwkv6_forward_varlen_fp16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                              void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_F16, stream);
}
int rwkv6_forward_varlen_fp32(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const float* r, const float* k, const float* v, const float* w,
                              const float* u, float* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_F32, stream);
}

int rwkv6_forward_varlen_snap_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                   void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                   int snap_every, const int* cu_snap, const int* snap_slot, int n_snap)
{
    const SnapArgs sn{state_slot_out, snap_every, cu_snap, snap_slot, n_snap};
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_BF16, stream, &sn);
}
size_t rwkv6_varlen_split_workspace_bytes(long total_T, int n_seq, int seg_len, int C, int H)
{
    if (n_seq < 1) return 0;
    if (total_T < 1 || H < 1 || (long)H * HEAD != (long)C || seg_len < 0 || seg_len % 64 != 0) return 0;
    return seg_len == 0 ? rwkv6_varlen_workspace_bytes(n_seq) : split_workspace_bytes(total_T, n_seq, seg_len, H);
}
int rwkv6_forward_varlen_split_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                    int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                    void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                    int snap_every, const int* cu_snap, const int* snap_slot, int n_snap, int seg_len)
{
    const SnapArgs sn{state_slot_out, snap_every, cu_snap, snap_slot, n_snap};
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_BF16, stream, &sn, seg_len);
}
int rwkv6_forward_varlen_snap_fp16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                   void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                   int snap_every, const int* cu_snap, const int* snap_slot, int n_snap)
{
    const SnapArgs sn{state_slot_out, snap_every, cu_snap, snap_slot, n_snap};
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_F16, stream, &sn);
}
int rwkv6_forward_varlen_snap_fp32(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const float* r, const float* k, const float* v, const float* w,
                                   const float* u, float* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream,
                                   const int* state_slot_out, int snap_every, const int* cu_snap, const int* snap_slot, int n_snap)
{
    const SnapArgs sn{state_slot_out, snap_every, cu_snap, snap_slot, n_snap};
    return rwkv6_infer_varlen(total_T, n_seq, max_seqlen, C, H, cu_seqlens, state_slot, n_slots, state_pool, r, k, v, w, u, y, workspace,
                              workspace_bytes, flags, IO_F32, stream, &sn);
}

// ---- device-side sampling with the penalty slot pool (csrc/wkv6_sample.hip); the order of the refusals is part of the contract
static int sample_slots(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                        const float* params, const float* u, int* tokens, float* logprob, int io, void* stream)
{
    if (n_seq < 1 || V < 1 || n_slots < 1 || ld < V || ld % 8) return WKV6_EINVAL;
    if (!slot && n_slots < n_seq) return WKV6_EINVAL;
    if (((uintptr_t)logits | (uintptr_t)occ_pool) & 15) return WKV6_EINVAL;
    if (((uintptr_t)slot | (uintptr_t)slot_out | (uintptr_t)params | (uintptr_t)u | (uintptr_t)tokens | (uintptr_t)logprob) & 3) return WKV6_EINVAL;
    const uintptr_t lo = (uintptr_t)logits, oc = (uintptr_t)occ_pool;
    const size_t lo_bytes = (size_t)n_seq * ld * (io == IO_F32 ? 4 : 2), oc_bytes = (size_t)n_slots * ld * 4;
    if (logits && occ_pool && lo < oc + oc_bytes && oc < lo + lo_bytes) return WKV6_EINVAL;
    if (V > SAMPLE_MAX_V) return WKV6_EUNSUPPORTED;
    if (!logits || !occ_pool || !params || !u || !tokens) return WKV6_ENULL;
    SampleArgs a = {};
    a.n_seq = n_seq; a.V = V; a.ld = ld; a.n_slots = n_slots;
    a.logits = logits; a.occ = occ_pool; a.slot = slot; a.slot_out = slot_out; a.params = params; a.u = u;
    a.tokens = tokens; a.logprob = logprob;
    return to_rc(launch_sample_slots(a, io, (hipStream_t)stream));
}
int rwkv6_sample_slots_bf16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_BF16, stream);
}
int rwkv6_sample_slots_fp16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_F16, stream);
}
int rwkv6_sample_slots_fp32(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_F32, stream);
}

static int selftest_problem(int B, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int T = 83, H = 2, C = H * HEAD;
    const size_t n = (size_t)B * T * C, nu = (size_t)C, ngu = (size_t)B * C;
    const size_t ws = wkv6_backward_workspace_bytes(B, T, C, H);
    // layout of one device allocation (bf16 elements): r k v w gy | y[2] gr[2] gk[2] gv[2] gw[2] | u | gu[2] ; then workspace
    const size_t elems = 5 * n + 10 * n + nu + 2 * ngu;
    const size_t bytes = align_up(elems * 2);
    char* dev = nullptr;
    if (hipMalloc(&dev, bytes + ws) != hipSuccess) return WKV6_EWORKSPACE;
    std::vector<unsigned short> host(elems, 0);
    unsigned lcg = 12345u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) & 0xffff) / 65536.0f - 0.5f; };   // U(-0.5, 0.5)
    auto to_bf = [](float f) { unsigned u; memcpy(&u, &f, 4); u += 0x7fffu + ((u >> 16) & 1u); return (unsigned short)(u >> 16); };
    for (size_t i = 0; i < n; ++i) {
        host[i] = to_bf(rnd());                      // r
        host[n + i] = to_bf(rnd());                  // k
        host[2 * n + i] = to_bf(rnd());              // v
        host[3 * n + i] = to_bf(-6.f + 7.f * (rnd() + 0.5f));   // w in [-6, 1]
        host[4 * n + i] = to_bf(rnd());              // gy
    }
    for (size_t i = 0; i < nu; ++i) host[15 * n + i] = to_bf(rnd());
    bf16_t* const p = reinterpret_cast<bf16_t*>(dev);
    hipError_t e = hipMemcpyAsync(dev, host.data(), elems * 2, hipMemcpyHostToDevice, st);
    int rc = e == hipSuccess ? WKV6_OK : (int)e;
    const unsigned base_flags = WKV6_W_RAW;
    for (int alg = 0; alg < 2 && rc == WKV6_OK; ++alg) {   // 0: chunked, 1: scan
        const unsigned fl = base_flags | (alg ? WKV6_ALGO_SCAN : 0u);
        rc = wkv6_forward_ex(B, T, C, H, p, p + n, p + 2 * n, p + 3 * n, p + 15 * n, nullptr, nullptr, p + (5 + alg) * n, fl, stream);
        if (rc == WKV6_OK)
            rc = wkv6_backward_ex(B, T, C, H, p, p + n, p + 2 * n, p + 3 * n, p + 15 * n, nullptr, p + 4 * n, p + (7 + alg) * n,
                                  p + (9 + alg) * n, p + (11 + alg) * n, p + (13 + alg) * n, p + 15 * n + nu + alg * ngu, nullptr,
                                  dev + bytes, ws, fl, stream);
    }
    if (rc == WKV6_OK) {
        e = hipMemcpyAsync(host.data(), dev, elems * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = (int)e;
    }
    (void)hipFree(dev);
    if (rc != WKV6_OK) return rc;
    auto bf = [&](size_t i) { unsigned u = (unsigned)host[i] << 16; float f; memcpy(&f, &u, 4); return f; };
    auto differ = [&](size_t a0, size_t b0, size_t cnt, float ulps) {   // max |a-b| in bf16 ulps of the tensor scale
        float scale = 0.f, diff = 0.f;
        for (size_t i = 0; i < cnt; ++i) {
            scale = fmaxf(scale, fabsf(bf(b0 + i)));
            diff = fmaxf(diff, fabsf(bf(a0 + i) - bf(b0 + i)));
        }
        return !(diff <= ulps * scale * 0.0078125f);   // also catches NaN
    };
    int bad = 0;
    bad += differ(5 * n, 6 * n, n, 2.f);          // y
    bad += differ(7 * n, 8 * n, n, 2.f);          // gr
    bad += differ(9 * n, 10 * n, n, 2.f);         // gk
    bad += differ(11 * n, 12 * n, n, 2.f);        // gv
    bad += differ(13 * n, 14 * n, n, 4.f);        // gw
    bad += differ(15 * n + nu, 15 * n + nu + ngu, ngu, 2.f);   // gu
    return bad ? WKV6_ESELFTEST : WKV6_OK;
}

// Device self-test: (1) the cross-lane primitives, (2) the chunked MFMA kernels against the exact scan kernels on a
// fixed pseudo-random problem (B=2, T=83, H=2: ragged last block and stage) -- catches a miscompiled or mis-scheduled
// build (e.g. the mixed-shape MFMA accumulation hazard) at load time instead of in training.
// Returns 0, a positive count of failed primitive checks, or WKV6_ESELFTEST.
int wkv6_selftest(void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    {
        int* d = nullptr;
        if (hipMalloc(&d, sizeof(int)) != hipSuccess) return WKV6_EWORKSPACE;
        int host = -1;
        hipError_t e = hipMemsetAsync(d, 0, sizeof(int), st);
        if (e == hipSuccess) e = launch_selftest(d, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&host, d, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(d);
        if (e != hipSuccess) return (int)e;
        if (host != 0) return host;
    }
    // two problems of T = 83 tokens (ragged last block and stage, an odd and an even stage of a 64-token pair), H = 2: B = 2 -- few
    // (batch, head) pairs: the launchers put two workgroups on each -- and the smallest B
    // that gets one workgroup per pair on this device (the mode of real shapes): both modes of wkv6_chunk_bwd12k.hip run
    const int cus = cu_count();
    const int batches[2] = {2, (cus > 0 ? cus : 256) / 4 + 1};
    for (int prob = 0; prob < 2; ++prob) {
        if (int rc = selftest_problem(batches[prob], stream)) return rc;
    }
    return WKV6_OK;
}

}  // extern "C"
