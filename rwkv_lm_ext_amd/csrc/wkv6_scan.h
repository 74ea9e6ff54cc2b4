// Exact-fp32 token-serial WKV6 kernels for gfx950 ("scan" path).
//
// These kernels evaluate the recurrence of cuda/wkv6_cuda.cu:6-227 literally (fp32 state, one
// token after another), re-laid-out for CDNA4:
//   * one 512-thread workgroup (8 wave64) per (batch, head); the 64x64 state is tiled over the
//     waves, every lane owns a small i x j sub-block in registers;
//   * r/k/v/w(/gy) rows are staged 16 tokens at a time through a double-buffered LDS image
//     (coalesced 128-B row segments from HBM), decays exp(-exp(w)) are formed once per element
//     while staging;
//   * the per-token reductions use DPP row operations and v_permlane{16,32}_swap, not LDS;
//   * backward = two sweeps instead of the reference's five (kernel_backward_111 has three scans,
//     kernel_backward_222 two): sweep S (forward in scan order) recomputes the state and emits gr
//     and a_t = r_t (.) sum_j gy_t[j] S_t[.][j]; sweep G (reverse) carries G, emits gk, gv and
//     b_t = k_t (.) sum_j G_t[.][j] v_t[j] and forms gw from the suffix-sum identity
//     gew_t = sum_{s>t} a_s - sum_{s>=t} b_s   (fla/ops/rwkv6/recurrent_fuse.py:394-396),
//     which removes the reference's per-thread float[T] scratch array and its T <= _T_ limit.
//
// They are the reference-exact path (any T >= 1, any decay magnitude, optional initial / final
// state, either time direction, per-row lengths).
#pragma once
#include <cstdlib>
#include "wkv6_common.h"

namespace wkv6 {

// The chunked forward leaves fp32 state checkpoints for the chunked backward (wkv6_chunk_bwd12k.hip, one or two workgroups per
// (batch, head)): one 64x64 state per CKPT_TOK = 64 tokens and head (4 B per token-channel), laid out in the register order of
// that kernel's row waves -- [row wave i>>4][column tile jt][lane 16 g + (i & 15)][4 columns tile_ch(jt) + 8 g + q] -- so that a row
// wave takes its 16x64 slice with four coalesced 16-byte loads.  (Rounds 3-4 had a second, opt-in layout for the two-level backward
// experiment, now parked under tools/experiments/.)
constexpr int CKPT_TOK = 64;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device): the attribute is per device.
struct LdsAttrOnce {
    bool done[64] = {};
    hipError_t ensure(const void* fn, size_t bytes)
    {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return e;
        if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
        if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) return e;
        if (dev >= 0 && dev < 64) done[dev] = true;
        return hipSuccess;
    }
};

// The one way a kernel is launched: raise the kernel's LDS limit where the launch needs more than the default 64 KB (once per instantiation
// and device: Kernel is a template argument, so the static is the instantiation's own), launch, report the launch's error.
template <auto Kernel, typename... Args>
hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args)
{
    static LdsAttrOnce attr;
    if (lds > 64 * 1024)
        if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(Kernel), lds)) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

struct ScanArgs {
    int B, T, C, H;
    const void *r, *k, *v, *w, *u;   // w: float ew = -exp(w) when wkind == 0, raw w in the I/O type when 1,
    int wkind;                        //    float decay d = exp(-exp(w)) when 2 (inference kernel, cuda/rwkv6.cu:38)
    int state_f32;                    // s0 / s_out are fp32 regardless of the I/O type (cuda/rwkv6.cu:8)
    const void* s0;                   // initial state [.., H, N(j), N(i)] in the I/O type, or null (zero)
    long s0_bstride;                  // elements between batch entries of s0 (0: shared over the batch)
    void* s_out;                      // final state [B,H,N,N] in the I/O type, or null   (forward only)
    void* y;                          // forward output
    float* y_f32;                     // optional fp32 side buffer [B,T,C]: written INSTEAD of y when accumulate == 0,
                                      // read as the addend (instead of y) when accumulate == 1  (wkv6_bi halves)
    const void* gy;                   // backward input
    void *gr, *gk, *gv, *gw;          // backward outputs, I/O type
    float* g_f32[4];                  // optional fp32 side buffers [B,T,C] for gr,gk,gv,gw (chunked backward): written INSTEAD
                                      // of the outputs when accumulate == 0, read as the addend when accumulate == 1, so the
                                      // two halves of wkv6_bi are summed in fp32 and rounded once
    void* gu;                         // [B,C] per-batch partials, I/O type (null: skip)
    void* gs;                         // [B,H,N,N] per-batch dL/dS0, I/O type (null: skip)
    int part_f32;                     // gu and gs are fp32 whatever the I/O type (WKV6_PARTIALS_F32): the caller sums them over the batch
    float* aux;                       // [B,T,C] fp32 scratch carrying a_t from sweep S to sweep G
    float* ckpt;                      // chunked path: [B*H][ceil(T/CKPT_TOK)][4096] fp32 states at 64-token boundaries (forward / state pass -> backward)
    int ckpt_valid;                   // backward: ckpt was filled by the forward, skip the state pass
    const int* lens;                  // per-batch number of tokens to scan (null: T)
    const int* order;                 // chunked kernels: batch row served by workgroup slot blockIdx / H (null: identity) -- rows
                                      // sorted by decreasing length, so that the longest sequences start first (wkv6_bi)
    int reverse;                      // 1: scan tokens lens-1 .. 0
    const int* rev_n;                 // chunked kernels: per-batch number of leading tokens that the tensors named in rev_mask
    unsigned rev_mask;                //   hold in reverse order (scan position p < rev_n[b] <-> token rev_n[b]-1-p; positions
                                      //   beyond keep their place); every token is still scanned.  Bits: REV_*
    int use_u;                        // 0: bonus u treated as 0 (reverse half of wkv6_bi)
    int accumulate;                   // 1: add into y / gr,gk,gv,gw instead of overwriting
    int zero_tail;                    // 1: write zeros for tokens >= lens[b]
    int ckpt_segs;                    // chunked forward as a two-level scan: batch row b is segment b % ckpt_segs of sequence
                                      // b / ckpt_segs, and its checkpoints go to that sequence's slots (0 / 1: plain)
    float* dsum;                      // chunked forward / state pass: [B*H][4][64] per-block-slot sums of the (clamped) log2-decays
                                      // over the whole sequence (the segment summaries of the T-split forward), or null
    // chunked forward with the GroupNorm(H) * gate epilogue of the time-mix block fused into its store (src/model.py:462-468):
    const void *gn_gate, *gn_gamma, *gn_beta;   // gate [B,T,C], ln_x.weight / bias [C] (I/O type); gn_out != null enables it
    float gn_eps;
    void* gn_out;                     // [B,T,C]  GroupNorm_H(y) * gate  (y itself is stored too unless y == null)
    float* gn_stats;                  // [B*T, H, 2] mean, rstd of every (token, head) for the backward, or null
    const float* g_in;                // backward as a two-level scan over T (wkv6_tsplit.hip: chunk_backward): fp32 [B,H,N(j),N(i)] adjoint state
                                      // entering this row (= segment) from the future, or null (zero)
    const float* rc_in;               // ... and fp32 [B,C]: the gw suffix sum at the segment's end, sum_{s >= end} (a_s - b_s) =
                                      // Phi[i] = sum_j G[i][j] S[i][j] at the boundary, or null (zero)
    int side_compact;                 // chunked wkv6_bi halves in one launch: y_f32 / g_f32 are per-workgroup scratch, fp32 [slot][T][64]
                                      // (token stride 64), instead of [B,T,C] arrays addressed by (batch, head)
    unsigned long long* clk;          // chunked kernels: clock stamps of wave 0 of workgroup slots < clk_slots ({memtime, memrealtime} at start
    int clk_slots;                    //   and end: wkv6_set_clock_ring, include/wkv6_amd.h), or null (the default: no stamp executes)
    int split;                        // chunked kernels, set by the launcher when B*H leaves half the chip idle: two workgroups per
                                      // (batch, head), each with its own producers and half of the consuming waves
    // Packed variable-length batches (the *_varlen launchers; null / 0 everywhere else; kept at the end: the dense kernels' kernarg offsets
    // stay where they were).  Row b is sequence b of [total_T, C] tensors: B = number of sequences, T = the longest length allowed,
    // lens / order always set; all three arrays are written (and clamped) on the device by the API's preparation kernel.
    const int* tok_off;               // [B] first token of the sequence
    const int* ck_off;                // [B] first checkpoint slot of the sequence within its head: exclusive prefix sum of ceil(len / CKPT_TOK)
    long ck_stride;                   // checkpoint slots per head: a.ckpt is [H][ck_stride][4096]
    // Packed stateful inference (rwkv6_forward_varlen_*: the SLOTS instantiations of the packed forward kernels read these, nobody else
    // does; at the end again).  The state of sequence b is slot state_slot[b] (null: b) of a caller-owned pool [n_slots,H,N,N] of fp32 states,
    // s0 == s_out == the pool: the lanes that load an element are the lanes that store it, so the slot is updated in place.  A slot
    // outside [0, n_slots) is "no state": zero in, nothing out; the array is written on the device and never read by the host.
    const int* state_slot;
    int n_slots;
    int len_lo, len_hi;               // len_hi != 0: a workgroup whose sequence has a (clamped) length outside [len_lo, len_hi) returns
                                      // before it touches anything -- two launches over one prepared batch share it by length
    // State snapshots and a separate output slot (rwkv6_forward_varlen_snap_*: the SNAP instantiations read these, nobody else does; at the
    // end once more).  The final state of sequence b goes to slot state_slot_out[b] (null: its source slot, the in-place update above),
    // validated like the source.  Sequence b keeps m = min(len / snap_every, cu_snap[b+1] - cu_snap[b]) snapshots: the state after its
    // first (j + 1) * snap_every tokens goes to slot snap_slot[cu_snap[b] + j] of the same pool, j < m; a slot outside the pool is skipped.
    // cu_snap is clamped into [0, n_snap] on the device; none of the arrays is read by the host.
    const int* state_slot_out;
    int snap_every;                   // 0: no snapshots (cu_snap / snap_slot may be null), else a multiple of 64
    const int* cu_snap;               // [B + 1]
    const int* snap_slot;             // [n_snap]
    int n_snap;
};

// Long sequences cut over T (rwkv6_forward_varlen_split_bf16: the SEG instantiations of the packed forward take this beside their ScanArgs --
// an argument block of its own, so that ScanArgs and with it every other kernel's kernarg layout stay as they are).  Row b of the ScanArgs is
// ITEM b of a table the API's preparation kernel writes in dispatch order: a.lens / a.tok_off are per item (a.order is null, a.ck_off any
// array of as many ints), a.B is the number of table entries the launch covers; item b covers tokens [pos[b], pos[b] + a.lens[b]) of sequence
// seq[b], whose clamped length is seq_lens[seq[b]].  a.state_slot, a.state_slot_out and a.cu_snap stay indexed by the SEQUENCE.  An item that
// is not its sequence's only one starts from sin[b] (fp32 [a.B,H,N,N], the chaining kernel's entry states) instead of the pool; only a
// sequence's last item stores the final state.  n[0] items exist: workgroups past them return before anything else.
struct SegArgs {
    const int* n;
    const int* seq;
    const int* pos;
    const int* seq_lens;
    const float* sin;
};

// Shortest sequence the stateful inference calls (rwkv6_cuda_forward_bf16, rwkv6_forward_varlen_bf16) hand to the chunked kernel; shorter
// ones (decode steps) take the exact scan
constexpr int INFER_CHUNK_MIN_T = 32;

// State slot of sequence b of a packed stateful call, or -1: no state.  Decided before any address is formed: a garbage slot touches no memory.
__device__ __forceinline__ int state_slot_of(const ScanArgs& a, int b, int ntok)
{
    const int slot = a.state_slot ? a.state_slot[b] : b;
    return (ntok > 0 && slot >= 0 && slot < a.n_slots) ? slot : -1;
}
// SNAP: the slot that takes the final state of sequence b whose source slot is `src`, or -1: nothing is stored.  The same rule, on its own.
__device__ __forceinline__ int state_slot_out_of(const ScanArgs& a, int b, int ntok, int src)
{
    if (!a.state_slot_out) return src;
    const int slot = a.state_slot_out[b];
    return (ntok > 0 && slot >= 0 && slot < a.n_slots) ? slot : -1;
}
// SNAP: the snapshots of sequence b -- snap_slot[first + j] takes the state after (j + 1) * snap_every tokens, j < count.  first + count never
// passes n_snap, so every index formed from it lies inside snap_slot.
struct SnapPlan {
    int first, count;
};
__device__ __forceinline__ SnapPlan snap_plan(const ScanArgs& a, int b, int ntok)
{
    if (a.snap_every <= 0 || !a.cu_snap || !a.snap_slot || a.n_snap <= 0) return SnapPlan{0, 0};
    const int lo = min(max(a.cu_snap[b], 0), a.n_snap), hi = min(max(a.cu_snap[b + 1], 0), a.n_snap);
    return SnapPlan{lo, min(ntok / a.snap_every, max(hi - lo, 0))};
}
// slot of snapshot j < count, or -1: skipped (tested before any address is formed, like a state slot)
__device__ __forceinline__ int snap_slot_of(const ScanArgs& a, const SnapPlan& sp, int j)
{
    const int slot = a.snap_slot[sp.first + j];
    return (slot >= 0 && slot < a.n_slots) ? slot : -1;
}
// (decided once per workgroup, in front of everything else)
__device__ __forceinline__ bool outside_len_window(const ScanArgs& a, int ntok)
{
    return a.len_hi != 0 && (ntok < a.len_lo || ntok >= a.len_hi);
}

enum { REV_R = 1, REV_K = 2, REV_V = 4, REV_W = 8, REV_Y = 16, REV_ALL = 31 };   // REV_Y: y in the forward, gy in the backward;
                                                                                // every gradient follows its tensor's bit
// token a tensor holds at scan position p
struct RevMap {
    int n;
    unsigned mask;
    __device__ __forceinline__ int operator()(int p, unsigned bit) const { return ((mask & bit) && p < n) ? n - 1 - p : p; }
};
__device__ __forceinline__ RevMap make_revmap(const ScanArgs& a, int b, int ntok)
{
    if (a.reverse) return RevMap{ntok, REV_ALL};
    if (a.rev_n) return RevMap{min(max(a.rev_n[b], 0), ntok), a.rev_mask};
    return RevMap{0, 0u};
}

// Token addressing of the chunked kernels' global accesses.  AFF (chosen by the launchers: no per-tensor reversal map, a.rev_n == nullptr):
// scan position p of the row is token t0 + sgn * p of EVERY tensor (0, +1; or ntok - 1, -1 under a.reverse), so the element offset of
// (position pu + plane, channel ch) splits into a loop-invariant lane part, computed once in front of the stage loops, and a wave-uniform
// part that the scalar unit forms: one vector add per access where the general map costs a compare, a select, a subtraction and an
// integer multiply (half rate: 4.2 cycles, profiles/r05_issue2_microbench.txt) per access (round 5: ~45 of the backward's 1066 vector instructions per SIMD and stage).  Positions past the
// end map past the end (or below zero = far above it as unsigned): outside the row's buffer resources, as with the general map.
template <bool AFF>
struct TokAddr {
    RevMap m;
    int t0, sgn;
    __device__ __forceinline__ TokAddr(const ScanArgs& a, int b, int ntok) : m(make_revmap(a, b, ntok))
    {
        t0 = m.mask ? ntok - 1 : 0;
        sgn = m.mask ? -1 : 1;
    }
    // (explicit form: the whole row reversed or not -- the persistent wkv6_bi launches address the call that FOLLOWS the one whose argument
    // block they hold)
    __device__ __forceinline__ TokAddr(int ntok, bool rev) : m(RevMap{rev ? ntok : 0, rev ? (unsigned)REV_ALL : 0u})
    {
        t0 = rev ? ntok - 1 : 0;
        sgn = rev ? -1 : 1;
    }
    // lane part of the element offset: position `plane` within the uniform base, channel ch, `stride` elements between tokens
    __device__ __forceinline__ int lane(int plane, int ch, int stride) const { return AFF ? (t0 + sgn * plane) * stride + ch : 0; }
    __device__ __forceinline__ int token(int p, unsigned bit) const { return AFF ? t0 + sgn * p : m(p, bit); }
    // element offset of (position pu + plane, channel ch): pu wave-uniform; lane_part = lane(plane, ch, stride)
    __device__ __forceinline__ unsigned off(int pu, int plane, int ch, int stride, unsigned bit, int lane_part) const
    {
        if constexpr (AFF) return (unsigned)(lane_part + pu * (sgn * stride));
        else return (unsigned)(m(pu + plane, bit) * stride + ch);
    }
};

// Preconditions the chunked launchers share (wkv6_chunk.hip, wkv6_chunk_bwd12k.hip).
// per-lane byte offsets are 32-bit: bf16 tensors need (T + 64) C < 2^31 (checked by the API), the fp32 decay input half of that
inline bool offsets_fit(const ScanArgs& a) { return a.wkind == 1 || ((long)a.T + 64) * a.C < (1L << 30); }
// the int arrays of a packed batch, as the API's preparation kernel leaves them
inline bool packed_arrays_ok(const ScanArgs& a) { return a.tok_off && a.ck_off && a.lens && a.order; }
// two problems that one launch of 2 B H workgroups can serve ...
inline bool same_problem(const ScanArgs& a0, const ScanArgs& a1)
{
    return a0.B == a1.B && a0.T == a1.T && a0.C == a1.C && a0.H == a1.H && a0.wkind == a1.wkind;
}
// ... over the same packed sequences: one set of prepared int arrays
inline bool same_packed_arrays(const ScanArgs& a0, const ScanArgs& a1)
{
    return a0.tok_off == a1.tok_off && a0.ck_off == a1.ck_off && a0.lens == a1.lens && a0.order == a1.order && a0.ck_stride == a1.ck_stride;
}

enum { IO_BF16 = 0, IO_F32 = 1, IO_F16 = 2 };   // I/O element type of the scan forward (fp16: inference entry point only)
hipError_t launch_scan_fwd(const ScanArgs& a, int io, hipStream_t st);
hipError_t launch_scan_bwd(const ScanArgs& a, bool io_f32, hipStream_t st);
hipError_t launch_selftest(int* result, hipStream_t st);
// chunked MFMA forward (bf16 I/O only), wkv6_chunk.hip
hipError_t launch_chunk_fwd(const ScanArgs& a, hipStream_t st);
// two problems of one shape in one launch; the backward needs both problems' forward checkpoints
hipError_t launch_chunk_fwd_pair(const ScanArgs& a0, const ScanArgs& a1, hipStream_t st);
hipError_t launch_chunk_bwd_pair(const ScanArgs& a0, const ScanArgs& a1, hipStream_t st);
// chunked MFMA backward (bf16 I/O only): state pass + reverse pass; a.ckpt must hold chunk_ckpt_floats() floats
hipError_t launch_chunk_bwd(const ScanArgs& a, hipStream_t st);
// both halves of wkv6_bi in ONE persistent launch (one workgroup slot per CU walks (batch, head) rows: first half into the slot's fp32
// scratch, second half adds it and rounds): a1 / a2 = the forward-direction / reversed-direction problem; hipErrorNotSupported where
// the launch does not apply (two workgroups per pair) -- the caller then runs the halves as two launches
hipError_t launch_chunk_fwd_bi(const ScanArgs& a1, const ScanArgs& a2, int* slots, hipStream_t st);
hipError_t launch_chunk_bwd_bi(const ScanArgs& a1, const ScanArgs& a2, int* slots, hipStream_t st);
hipError_t launch_chunk_bwd12k(const ScanArgs& a, hipStream_t st);    // reverse pass over 64-token row-order checkpoints, a.split as given (wkv6_chunk_bwd12k.hip)
size_t chunk_ckpt_floats(int B, int T, int H);
// packed variable-length rows (ScanArgs: tok_off, ck_off, ck_stride), one workgroup per (sequence, head); bf16 I/O; a.rev_n ([B], indexed
// by the sequence) applies the per-tensor reversal map within each sequence
hipError_t launch_chunk_fwd_varlen(const ScanArgs& a, bool state_only, hipStream_t st);
hipError_t launch_chunk_bwd_varlen(const ScanArgs& a, hipStream_t st);   // a.ckpt_valid == 0: runs the state pass first
// two packed problems over the same sequences (shared lens / tok_off / ck_off / order) in one launch of 2 B H workgroups
hipError_t launch_chunk_fwd_varlen_pair(const ScanArgs& a0, const ScanArgs& a1, hipStream_t st);
hipError_t launch_chunk_bwd_varlen_pair(const ScanArgs& a0, const ScanArgs& a1, hipStream_t st);   // both with ckpt_valid
hipError_t launch_scan_fwd_varlen(const ScanArgs& a, bool io_f32, hipStream_t st);
hipError_t launch_scan_bwd_varlen(const ScanArgs& a, bool io_f32, hipStream_t st);
// packed stateful inference (ScanArgs: state_slot, n_slots, len_lo, len_hi; s0 == s_out == the fp32 pool, wkind == 2): the scan kernel in
// any I/O type, the chunked kernel in bf16.  Both return before touching anything for a sequence outside the length window.
inline bool slots_ok(const ScanArgs& a)
{
    return a.s0 && a.s0 == a.s_out && a.state_f32 && a.n_slots >= 1 && a.s0_bstride == (long)a.H * HEAD * HEAD && a.len_lo >= 0 && a.len_hi >= 0;
}
hipError_t launch_scan_fwd_slots(const ScanArgs& a, int io, hipStream_t st);
hipError_t launch_chunk_fwd_slots(const ScanArgs& a, hipStream_t st);
// ... with a separate output slot and state snapshots (ScanArgs: state_slot_out, snap_every, cu_snap, snap_slot, n_snap)
inline bool snap_ok(const ScanArgs& a)
{
    return a.snap_every >= 0 && a.snap_every % 64 == 0 && a.n_snap >= 0 && (a.snap_every == 0 || (a.cu_snap && a.snap_slot));
}
hipError_t launch_scan_fwd_snap(const ScanArgs& a, int io, hipStream_t st);
hipError_t launch_chunk_fwd_snap(const ScanArgs& a, hipStream_t st);
// ... over the item table of a split call (SegArgs): the state pass of the items that have a successor, or the forward per item
hipError_t launch_chunk_fwd_seg(const ScanArgs& a, const SegArgs& sg, bool state_only, hipStream_t st);
hipError_t launch_chunk_state_pass(const ScanArgs& a, hipStream_t st);   // state recurrence only (s_out, ckpt, dsum)
// (what the launchers ask of the host layer -- cu_count, want_split, bi_slots, clock_claim -- is declared in wkv6_host.h)

}  // namespace wkv6
