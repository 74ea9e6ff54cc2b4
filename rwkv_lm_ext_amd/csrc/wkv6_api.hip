// extern "C" entry points of the WKV6 families of librwkv6_amd.so (declared in include/wkv6_amd.h): argument checks and ScanArgs filling.
// Kernels, launches and everything with state live in the files that wkv6_host.h lists.
#include "wkv6_host.h"

#include <cstdint>

using namespace wkv6;

namespace {

// forward dispatch: chunked MFMA kernel for bf16 I/O unless the caller forces the exact scan
hipError_t run_fwd(const ScanArgs& a, unsigned flags, hipStream_t st)
{
    if (scan_route(flags)) return launch_scan_fwd(a, (flags & WKV6_IO_F32) ? IO_F32 : IO_BF16, st);
    return chunk_forward(a, st);
}

hipError_t run_bwd(ScanArgs& a, unsigned flags, float* scratch, hipStream_t st)
{
    if (scan_route(flags)) {
        a.aux = scratch;
        return launch_scan_bwd(a, flags & WKV6_IO_F32, st);
    }
    a.ckpt = scratch;
    a.ckpt_valid = (flags & WKV6_CKPT_VALID) ? 1 : 0;
    return chunk_backward(a, st);
}

}  // namespace

extern "C" {

const char* wkv6_amd_version(void) { return "0.1"; }

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
    if (scan_route(flags)) return WKV6_EUNSUPPORTED;
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
    if (scan_route(flags)) return WKV6_EUNSUPPORTED;
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

// ---- packed variable-length batches (workspace layout and preparation launch: wkv6_host.h, wkv6_prepare.hip) ------------------
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
    const bool chunked = !scan_route(flags);
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
    if (scan_route(flags)) return to_rc(launch_scan_fwd_varlen(a, flags & WKV6_IO_F32, st));
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
    const bool scan = scan_route(flags);
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

// One problem of a pair call, dense or packed: its refusals, then its tensors as ScanArgs.  The order of the refusals is part of the
// contract and differs in one place: the packed calls refuse a bad rev_mask first (mask_first) and with WKV6_EINVAL, the dense ones
// behind the null checks and with WKV6_EUNSUPPORTED.  need: bytes a checkpoint buffer must have where one is given
static int check_seq_set(const wkv6_seq_set& q, bool bwd, size_t need, int mask_rc, bool mask_first)
{
    const bool bad_mask = q.rev_mask & ~(unsigned)REV_ALL;
    if (bad_mask && mask_first) return mask_rc;
    if (!q.r || !q.k || !q.v || !q.w) return WKV6_ENULL;
    if (bwd ? (!q.gy || !q.gr || !q.gk || !q.gv || !q.gw || !q.ckpt) : !q.y) return WKV6_ENULL;
    if (bad_mask) return mask_rc;
    if (q.ckpt && q.ckpt_bytes < need) return WKV6_EWORKSPACE;
    return WKV6_OK;
}
static ScanArgs seq_set_args(int B, int T, int C, int H, const void* u, const wkv6_seq_set& q, unsigned flags, bool bwd)
{
    ScanArgs a = base_args(B, T, C, H, q.r, q.k, q.v, q.w, u, flags);
    set_rev(a, q.rev_n, q.rev_mask);
    if (bwd) {
        a.gy = q.gy; a.gr = q.gr; a.gk = q.gk; a.gv = q.gv; a.gw = q.gw; a.gu = q.gu;
        a.ckpt_valid = 1;                          // (the backward of a pair needs both problems' forward checkpoints)
    } else {
        a.y = q.y;
    }
    return a;
}

// The packed pair: both problems over the same sequences.  s[i].ckpt / ckpt_bytes is one wkv6_varlen_workspace_bytes() workspace per
// problem; the prepared int arrays (which both problems read) live in s[0]'s.  The forward may keep no checkpoints (either ckpt null; the
// int arrays then live in stream-ordered scratch when s[0].ckpt is null); the backward needs both, as the forward left them.
static int varlen_pair_args(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu, const void* u, const wkv6_seq_set* s,
                            unsigned flags, bool bwd, ScanArgs (&a)[2], float* (&area)[2])
{
    if (int rc = varlen_check(total_T, n_seq, max_seqlen, C, H, flags, VARLEN_PAIR_FLAGS)) return rc;
    if (scan_route(flags)) return WKV6_EUNSUPPORTED;
    if (!cu || !u || !s) return WKV6_ENULL;
    const size_t need = wkv6_varlen_workspace_bytes(total_T, n_seq, C, H);
    for (int i = 0; i < 2; ++i) {
        const wkv6_seq_set& q = s[i];
        if (int rc = check_seq_set(q, bwd, need, WKV6_EINVAL, true)) return rc;
        if (bwd ? !varlen_aligned({q.gr, q.gk, q.gv, q.gw}) : !varlen_aligned({q.y})) return WKV6_EINVAL;
    }
    for (int i = 0; i < 2; ++i) {
        a[i] = seq_set_args(n_seq, max_seqlen, C, H, u, s[i], flags, bwd);
        area[i] = s[i].ckpt ? reinterpret_cast<float*>(reinterpret_cast<char*>(s[i].ckpt) + varlen_int_bytes(n_seq)) : nullptr;
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
    if (scan_route(flags))        // exact scan kernels (fp32 I/O, or forced): same index maps, no checkpoints
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
    if (scan_route(flags)) return WKV6_EUNSUPPORTED;
    const size_t need = wkv6_backward_workspace_bytes(B, T, C, H);
    for (int i = 0; i < 2; ++i) {
        if (int rc = check_seq_set(s[i], bwd, need, WKV6_EUNSUPPORTED, false)) return rc;
        a[i] = seq_set_args(B, T, C, H, u, s[i], flags, bwd);
        a[i].ckpt = reinterpret_cast<float*>(s[i].ckpt);
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
    if (!scan_route(flags) && ((long)T + 128) * C >= (1L << 29)) flags |= WKV6_ALGO_SCAN;
    return flags;
}

// the reverse half of a wkv6_bi problem (cuda/wkv6_bi_cuda.cu:71-111): the tokens last to first, no bonus, added to what the forward half
// left; gu is the forward half's alone
static ScanArgs bi_reverse_half(ScanArgs a)
{
    a.reverse = 1; a.use_u = 0; a.accumulate = 1; a.zero_tail = 0; a.gu = nullptr;
    return a;
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
    const bool chunked = !scan_route(flags);
    const bool keep = (flags & WKV6_BI_KEEP_CKPT) && chunked;
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    if (hipError_t e = bi_row_arrays(a, mask, lens, ws.lens, ws.order, chunked, st)) return to_rc(e);
    a.y = y;
    a.y_f32 = ws.side[0];                     // the two halves are summed in fp32 and rounded once
    a.zero_tail = 1;                          // y[t > L_b] = 0 (the reference leaves it uninitialised, Q2)
    a.ckpt = keep ? ws.scan[0] : nullptr;
    ScanArgs a2 = bi_reverse_half(a);
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
    const bool chunked = !scan_route(flags);
    ScanArgs a = base_args(B, T, C, H, r, k, v, w, u, flags);
    if (hipError_t e = bi_row_arrays(a, mask, lens, ws.lens, ws.order, chunked, st)) return to_rc(e);
    a.gy = gy; a.gr = gr; a.gk = gk; a.gv = gv; a.gw = gw; a.gu = gu;
    a.zero_tail = 1;
    if (chunked) {
        // chunked bf16 path: the first half goes to fp32 side buffers, the second adds it and rounds once
        // (the reference accumulates `_gr[t] += F(gr)` in bf16, cuda/wkv6_bi_cuda.cu:199-200)
        for (int i = 0; i < 4; ++i) a.g_f32[i] = ws.side[i];
        // both halves in one persistent launch: the first half's four fp32 partials of a row stay in the slot's scratch
        ScanArgs a1 = a, a2 = bi_reverse_half(a);
        a1.ckpt = ws.scan[0]; a2.ckpt = ws.scan[1];
        a1.ckpt_valid = a2.ckpt_valid = (flags & WKV6_CKPT_VALID) ? 1 : 0;
        const hipError_t e = launch_chunk_bwd_bi(a1, a2, nullptr, st);
        if (e != hipErrorNotSupported) return to_rc(e);
    }
    if (hipError_t e = run_bwd(a, flags, ws.scan[0], st)) return (int)e;             // adjoint of the forward scan
    ScanArgs a2 = bi_reverse_half(a);                                                // adjoint of the reverse scan
    return to_rc(run_bwd(a2, flags, ws.scan[1], st));
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
    if (snap) {
        a.state_slot_out = snap->state_slot_out;
        a.snap_every = snap->snap_every; a.cu_snap = snap->cu_snap; a.snap_slot = snap->snap_slot; a.n_snap = snap->n_snap;
    }
    if (cut) {              // the chunked side of the length window per item of the cut sequences, the exact scan below the window
        if (hipError_t e = varlen_split_forward(a, area, cu_seqlens, total_T, max_seqlen, seg_len, st)) return to_rc(e);
        a.len_lo = 0; a.len_hi = INFER_CHUNK_MIN_T;
        return to_rc(launch_scan_fwd_snap(a, io, st));
    }
    if (hipError_t e = varlen_prepare(a, cu_seqlens, total_T, max_seqlen, true, io == IO_F32 ? (unsigned)WKV6_IO_F32 : 0u, {y}, st)) return to_rc(e);
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

}  // extern "C"
