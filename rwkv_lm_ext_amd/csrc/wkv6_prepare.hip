// Packed variable-length batches: the preparation launch that every packed call starts with, the item table of the calls that cut long
// sequences over T, and the workspace layouts that go with them.  From cu_seqlens[n_seq + 1] (token boundaries of the sequences in a
// [total_T, C] tensor), per sequence
//   lens    = clamp(cu[s + 1] - cu[s], 0, max_seqlen), cut so that the row ends at or before total_T,
//   tok_off = clamp(cu[s], 0, total_T),
//   ck_off  = exclusive prefix sum of ceil(lens / 64): the sequence's first checkpoint slot within its head (a sequence whose slots would
//             pass ck_stride -- only a cu_seqlens that is not a partition of [0, total_T) can do that -- is given length 0),
//   order   = the sequences by decreasing length (length_rank).
// Everything the kernels index with is clamped here, on the device: the host never reads cu_seqlens.
#include "wkv6_host.h"

#include <algorithm>

using namespace wkv6;

namespace {            // (the kernels keep their names outside namespace wkv6: profile filters tell them from the operator kernels by it)

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
    for (int s = tid; s < n_seq; s += 256) order[length_rank(s, lens[s], n_seq, [&](int o) { return lens[o]; })] = s;
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
        const int it = (int)ftotal + length_rank(s, rl, n_seq, rest_len), p = lens[s] - rl;
        tb.rest[s] = it;
        tb.len[it] = rl; tb.tok[it] = tok_off[s] + p; tb.seq[it] = s; tb.pos[it] = p;
    }
}

// Entry states of the items of the split sequences, one workgroup per (sequence, head): the arithmetic of tsplit_combine_kernel
// (wkv6_tsplit.hip) over the sequence's items -- chain_step, from the sequence's source slot (validated as state_slot_of does: outside the pool
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
        const int e = threadIdx.x + 256 * m;                            // state layout [j][i]: i = key channel
        float cur = have ? pool[((long)slot * H + h) * HEAD * HEAD + e] : 0.f;
        for (int g = 0; g < nfull; ++g) {
            const long bp = (long)(f0 + g) * H + h;
            Sin[bp * HEAD * HEAD + e] = cur;
            if (g + 1 == nfull && rest < 0) break;                       // (the last item: no state pass ran for it)
            cur = chain_step(cur, A, dsum, bp, e);
        }
        if (rest >= 0) Sin[((long)rest * H + h) * HEAD * HEAD + e] = cur;
    }
}

// One launch: workgroup 0 derives the int arrays (prepare), the others zero the rows of `out` that lie in no sequence -- as many workgroups
// as would zero the whole tensors with eight 16-byte stores per lane and tensor (nobody reads cu_seqlens here, so the launch cannot know
// how much there is to zero), 1024 at the most.
struct FillLaunch { VarlenFill fill; unsigned nwg; };      // the gap-zeroing part of a preparation launch: its arguments and workgroups
FillLaunch make_fill(long row_bytes, long total_T, std::initializer_list<void*> out)
{
    FillLaunch f = {};
    for (void* p : out) f.fill.out[f.fill.n_out++] = p;
    f.fill.row_bytes = row_bytes;
    const long per_wg = 256L * 16 * 8;
    f.nwg = (unsigned)std::min<long>(1024, (total_T * row_bytes + per_wg - 1) / per_wg);
    return f;
}

// rwkv6_forward_varlen_split_bf16: behind the int arrays of the plain call, the item table (SegTable) and per item and head the state
// pass's result A (items with a successor: the first max_extra entries), the entry state Sin and the decay sums
struct SplitWorkspace {
    SegTable tb;
    long n_table;                   // bound of the item table
    float *A, *Sin, *dsum;
};
long split_table_ints(int n_seq, long n_table) { return 2 + 2L * n_seq + 4 * n_table; }
SplitWorkspace split_carve(float* area, long total_T, int n_seq, int seg_len, int H)
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
hipError_t varlen_split_prepare(const ScanArgs& a, const int* cu, long total_T, int max_seqlen, const SegTable& tb, void* y, hipStream_t st)
{
    const FillLaunch f = make_fill((long)a.C * 2, total_T, {y});
    return launch<varlen_split_prepare_kernel>(dim3(1 + f.nwg), dim3(256), 0, st, cu, a.B, total_T, max_seqlen, a.ck_stride,
                                               const_cast<int*>(a.lens), const_cast<int*>(a.tok_off), const_cast<int*>(a.ck_off),
                                               const_cast<int*>(a.order), tb, f.fill);
}

}  // namespace

namespace wkv6 {

void varlen_carve(ScanArgs& a, void* workspace, long total_T, int n_seq, float** area)
{
    int* const ints = reinterpret_cast<int*>(workspace);
    a.lens = ints; a.tok_off = ints + n_seq; a.ck_off = ints + 2 * (size_t)n_seq; a.order = ints + 3 * (size_t)n_seq;
    a.ck_stride = varlen_ck_stride(total_T, n_seq);
    *area = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + varlen_int_bytes(n_seq));
}

hipError_t varlen_prepare(const ScanArgs& a, const int* cu, long total_T, int max_seqlen, bool prepare, unsigned flags,
                          std::initializer_list<void*> out, hipStream_t st)
{
    const FillLaunch f = make_fill((long)a.C * ((flags & WKV6_IO_F32) ? 4 : 2), total_T, out);
    return launch<varlen_prepare_kernel>(dim3(1 + f.nwg), dim3(256), 0, st, cu, a.B, total_T, max_seqlen, a.ck_stride, const_cast<int*>(a.lens),
                                         const_cast<int*>(a.tok_off), const_cast<int*>(a.ck_off), const_cast<int*>(a.order), prepare ? 1 : 0,
                                         f.fill);
}

size_t split_workspace_bytes(long total_T, int n_seq, int seg_len, int H)
{
    const long extra = total_T / seg_len, n_table = n_seq + extra;
    const size_t st = (size_t)H * HEAD * HEAD * sizeof(float);
    return varlen_int_bytes(n_seq) + align_up((size_t)split_table_ints(n_seq, n_table) * sizeof(int)) + align_up((size_t)extra * st)
           + align_up((size_t)n_table * st) + align_up((size_t)extra * H * 4 * HEAD * sizeof(float));
}

// the chunked side of the length window, per item: state pass of the items with a successor, chaining, forward (see SegTable)
hipError_t varlen_split_forward(const ScanArgs& a, float* area, const int* cu, long total_T, int max_seqlen, int seg_len, hipStream_t st)
{
    const SplitWorkspace sw = split_carve(area, total_T, a.B, seg_len, a.H);
    if (hipError_t e = varlen_split_prepare(a, cu, total_T, max_seqlen, sw.tb, a.y, st)) return e;
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
        if (hipError_t e = launch_chunk_fwd_seg(q, sq, true, st)) return e;
        if (hipError_t e = launch<varlen_split_chain_kernel>(dim3(a.B * a.H), dim3(256), 0, st, reinterpret_cast<const float*>(a.s0), a.state_slot,
                                                             a.n_slots, a.lens, sw.tb, sw.A, sw.dsum, sw.Sin, a.H))
            return e;
    }
    p.B = (int)sw.n_table;
    return launch_chunk_fwd_seg(p, sg, false, st);
}

}  // namespace wkv6
