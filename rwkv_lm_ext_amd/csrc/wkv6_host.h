// What the host files of librwkv6_amd.so share (internal; the public interface is include/wkv6_amd.h); every section names the file
// that defines what it declares.
#pragma once
#include "../../include/wkv6_amd.h"
#include "wkv6_scan.h"

#include <initializer_list>

namespace wkv6 {

inline int to_rc(hipError_t e) { return e == hipSuccess ? WKV6_OK : (int)e; }

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

// do the byte ranges [p, p + pn) and [q, q + qn) meet?  A null pointer meets nothing: whether it may be null is the entry point's to say
inline bool overlap(const void* p, size_t pn, const void* q, size_t qn)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + qn && b < a + pn;
}

inline int check_shape(int B, int T, int C, int H)
{
    if (B < 1 || T < 1 || C < 1 || H < 1) return WKV6_EINVAL;
    if ((long)H * HEAD != (long)C) return WKV6_EINVAL;      // reference: assert(H*_N_ == C)
    if (((long)T + 64) * C >= (1L << 31)) return WKV6_EUNSUPPORTED; // one sequence (rounded up to whole groups) must stay 32-bit
                                                                  // addressable: per-lane byte offsets of bf16 tensors are 32-bit
    return WKV6_OK;
}

// the exact scan kernels serve the call (fp32 I/O, or forced); otherwise the chunked MFMA kernels (bf16 I/O)
inline bool scan_route(unsigned flags) { return flags & (WKV6_IO_F32 | WKV6_ALGO_SCAN); }

// ---- launch-shape policy (wkv6_policy.hip): how many workgroups the chunked kernels run on
int cu_count();                              // compute units of the current device (0: unknown)
int want_split(int BH);                      // two workgroups per (batch, head)?
int bi_slots(int BH);                        // workgroup slots of a persistent wkv6_bi launch (0: does not apply)

// ---- mutable state (wkv6_state.hip)
int dispatch_override(int what);             // by WKV6_DISPATCH_* (wkv6_set_dispatch); -1: the library's own choice
// In-run clock probe (wkv6_set_clock_ring): where launch number n of kind (0: chunked forward, 1: chunked backward) stamps, or null;
// takes the launch's place in the ring (host side, one atomic increment per launch)
unsigned long long* clock_claim(int kind, int* slots);

// Scratch for callers that pass no workspace (the reference-signature entry points have no such argument): a stream-ordered
// allocation (hipMallocFromPoolAsync on the caller's stream, hipFreeAsync right behind the launches that use it), so concurrent
// streams never share a buffer and nothing synchronises the device.  The memory comes from a pool this library owns (one per
// device, created on first use), not from the device's default pool, whose settings belong to the host application; the pool
// keeps up to SCRATCH_KEEP bytes between calls (the steady state of ordinary shapes is an O(1) pool hit) and gives the rest back.
// Under stream capture the allocation becomes part of the graph like any other stream-ordered allocation; callers that
// replay graphs should pass a workspace instead (every *_ex entry point takes one).
struct StreamScratch {
    void* ptr = nullptr;
    hipStream_t st = nullptr;
    void* get(size_t bytes, hipStream_t stream);
    ~StreamScratch()
    {
        if (ptr) (void)hipFreeAsync(ptr, st);
    }
};

// The caller's workspace where it gave one of `need` bytes, else stream-ordered scratch of `scratch_need` bytes (0: `need`), released when
// `scratch` goes out of scope.  Null (the workspace is too small, or the allocation failed) is WKV6_EWORKSPACE.
inline void* acquire(void* workspace, size_t workspace_bytes, size_t need, StreamScratch& scratch, hipStream_t st, size_t scratch_need = 0)
{
    if (workspace) return workspace_bytes >= need ? workspace : nullptr;
    return scratch.get(scratch_need ? scratch_need : need, st);
}

inline ScanArgs base_args(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const void* u, unsigned flags)
{
    ScanArgs a = {};
    a.B = B; a.T = T; a.C = C; a.H = H;
    a.r = r; a.k = k; a.v = v; a.w = w; a.u = u;
    a.wkind = (flags & WKV6_W_RAW) ? 1 : 0;
    a.part_f32 = (flags & WKV6_PARTIALS_F32) ? 1 : 0;
    a.use_u = 1;
    return a;
}
// the initial state: one for the whole batch, or one per batch entry (WKV6_S0_PER_BATCH)
inline void set_state(ScanArgs& a, const void* s0, unsigned flags)
{
    a.s0 = s0;
    a.s0_bstride = (flags & WKV6_S0_PER_BATCH) ? (long)a.H * HEAD * HEAD : 0;
}
// the per-tensor reversal map: no lengths, no map
inline void set_rev(ScanArgs& a, const int* rev_n, unsigned rev_mask)
{
    a.rev_n = rev_n;
    a.rev_mask = rev_n ? rev_mask : 0u;
}

// ---- the chunked kernels behind the two-level scan over T where the shape asks for it (wkv6_tsplit.hip)
hipError_t chunk_forward(const ScanArgs& a, hipStream_t st);
hipError_t chunk_backward(const ScanArgs& a, hipStream_t st);

// ---- the row arrays of wkv6_bi (wkv6_bi_rows.hip): a.lens = the caller's lens, or lens_buf filled from the mask; a.order = order_buf
// filled with the dispatch order where the chunked kernels run more than one row (B <= 4096: one workgroup ranks them)
hipError_t bi_row_arrays(ScanArgs& a, const int* mask, const int* lens, int* lens_buf, int* order_buf, bool chunked, hipStream_t st);

// ---- packed-batch preparation (wkv6_prepare.hip)
// workspace of the packed calls: lens, tok_off, ck_off, order (int32 [n_seq] each) | checkpoints [H][ck_stride][4096] fp32, ck_stride =
// total_T / 64 + n_seq (sum_s ceil(len_s / 64) <= total_T / 64 + n_seq for any partition of total_T tokens); the scan path's fp32
// [total_T, C] scratch lies over the checkpoint area (H * (total_T / 64) * 16 KB = total_T * C * 4 B).
inline long varlen_ck_stride(long total_T, int n_seq) { return total_T / CKPT_TOK + n_seq; }
inline size_t varlen_int_bytes(int n_seq) { return align_up((size_t)4 * n_seq * sizeof(int)); }
void varlen_carve(ScanArgs& a, void* workspace, long total_T, int n_seq, float** area);
// One launch: workgroup 0 derives the int arrays of `a` from cu_seqlens (`prepare` false: they are already there), the others zero the
// rows of `out` (C elements, fp32 under WKV6_IO_F32, else 16-bit) that lie in no sequence
hipError_t varlen_prepare(const ScanArgs& a, const int* cu, long total_T, int max_seqlen, bool prepare, unsigned flags,
                          std::initializer_list<void*> out, hipStream_t st);
// rwkv6_forward_varlen_split_bf16 (long sequences cut over T into items of seg_len tokens): the workspace behind the int arrays, and the
// chunked side of the call -- preparation with the item table, state pass, chaining, forward per item; `a` is the prepared plain problem
size_t split_workspace_bytes(long total_T, int n_seq, int seg_len, int H);
hipError_t varlen_split_forward(const ScanArgs& a, float* area, const int* cu, long total_T, int max_seqlen, int seg_len, hipStream_t st);

// ---- device helpers that kernels of more than one file share
// rank of row `self` of length `len` among n rows by decreasing length, ties by index: its place in the dispatch order (workgroups are
// dispatched in blockIdx order, so the longest rows start first and the short ones fill the tail)
template <typename Len>
__device__ __forceinline__ int length_rank(int self, int len, int n, const Len& len_of)
{
    int rank = 0;
    for (int o = 0; o < n; ++o) {
        const int lo = len_of(o);
        rank += (lo > len) || (lo == len && o < self);
    }
    return rank;
}
// one step of chaining segment summaries: the state behind segment (or item) row bp = 2^{dsum} (.) the state in front of it + the
// segment's own contribution A from a zero state; element e of the 64x64 state, key channel i = e & 63, dsum in four block-slot rows
__device__ __forceinline__ float chain_step(float cur, const float* __restrict__ A, const float* __restrict__ dsum, long bp, int e)
{
    const int i = e & (HEAD - 1);
    float dl = 0.f;
    for (int q = 0; q < 4; ++q) dl += dsum[(bp * 4 + q) * HEAD + i];
    return fmaf(__builtin_amdgcn_exp2f(dl), cur, A[bp * HEAD * HEAD + e]);
}

}  // namespace wkv6
