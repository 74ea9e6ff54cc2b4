/*
 * wkv6_amd.h -- C ABI of librwkv6_amd.so: the MI355X (gfx950) implementation of the RWKV-6 WKV
 * operator family of yynil/RWKV_LM_EXT.
 *
 * Every entry point takes plain device pointers and sizes (no torch types) plus the HIP stream to
 * launch on, and returns 0 on success or a negative WKV6_E* / positive hipError_t code; nothing is
 * launched when arguments are rejected.  All tensors are contiguous, layouts as in the reference:
 *   r,k,v,w,y,gy,gr,gk,gv,gw : [B,T,C]     u : [H,N]     gu : [B,C] (per-batch partials)
 *   N = C/H = 64 (the reference build's -D_N_, src/model.py:189)
 * bf16 buffers are passed as void* (raw bfloat16 bits).
 *
 * The first four pairs are drop-in replacements for the `cuda_forward` / `cuda_backward` C symbols
 * that the reference's torch-extension shims call; each has the reference's parameter list with
 * one trailing `stream`.  The *_ex entry points expose what the reference cannot express (bf16 raw
 * decay without the fp32 `ew` pass, fp32 I/O for numerics tests, separate in/out state, caller-owned
 * workspace, per-row lengths).  INTEGRATION.md shows the binding a maintainer would add.
 */
#ifndef WKV6_AMD_H
#define WKV6_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    WKV6_OK = 0,
    WKV6_EINVAL = -1,      /* bad shape: C != H*64, B/T/C/H < 1 (reference: assert(H*_N_ == C), cuda/wkv6_cuda.cu:231) */
    WKV6_ENULL = -2,       /* a required pointer is NULL */
    WKV6_EWORKSPACE = -3,  /* workspace too small / allocation failed */
    WKV6_EUNSUPPORTED = -4,
    WKV6_ESELFTEST = -5
};

/* ---- wkv6: replaces cuda_forward / cuda_backward of cuda/wkv6_op.cpp:5-6 (cuda/wkv6_cuda.cu:229-242).
 * `w` is the fp32 tensor ew = -exp(w_raw) that src/model.py:210 builds. */
int wkv6_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                      const float* w, const void* u, void* y, void* stream);
int wkv6_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                       const float* w, const void* u, const void* gy, void* gr, void* gk, void* gv,
                       void* gw, void* gu, void* stream);

/* ---- wkv6_bi: replaces cuda_forward / cuda_backward of cuda/wkv6_bi_op.cpp:5-6
 * (cuda/wkv6_bi_cuda.cu:363-377).  mask: int32 [B,T]; both scans cover tokens 0..L_b where L_b is
 * the first t with mask[b][t]==0 (T-1 if the row has no zero); y and the gradients are 0 for
 * t > L_b; the backward is the exact adjoint of the forward (deviations Q1-Q3). */
int wkv6bi_cuda_forward(int B, int T, int C, int H, const int* mask, const void* r, const void* k,
                        const void* v, const float* w, const void* u, void* y, void* stream);
int wkv6bi_cuda_backward(int B, int T, int C, int H, const int* mask, const void* r, const void* k,
                         const void* v, const float* w, const void* u, const void* gy, void* gr,
                         void* gk, void* gv, void* gw, void* gu, void* stream);

/* ---- wkv6state: replaces cuda/wkv6state_op.cpp:5-6.  `w` is the RAW bf16 decay parameter
 * (cuda/wkv6state_cuda.cu:30), s: bf16 [H,N,N] (value-major: s[h][j][i]), gs: bf16 [B,H,N,N]. */
int wkv6state_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                           const void* w, const void* u, const void* s, void* y, void* stream);
int wkv6state_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                            const void* w, const void* u, const void* s, const void* gy, void* gr,
                            void* gk, void* gv, void* gw, void* gu, void* gs, void* stream);

/* ---- wkv6infctx: replaces cuda/wkv6infctx_op.cpp:5-6.  s: bf16 [B,H,N,N]; the forward overwrites
 * it with the final state (cuda/wkv6infctx_cuda.cu:65-67).  The backward must be given the INITIAL
 * state (the reference hands it the overwritten one; the python wrapper keeps a copy). */
int wkv6infctx_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                            const void* w, const void* u, void* s, void* y, void* stream);
int wkv6infctx_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                             const void* w, const void* u, const void* s, const void* gy, void* gr,
                             void* gk, void* gv, void* gw, void* gu, void* gs, void* stream);

/* ---- rwkv6 (stateful forward-only inference): replaces cuda_forward_bf16 / cuda_forward_fp16 / cuda_forward_fp32 of
 * cuda/rwkv6_op.cpp:8-10 (cuda/rwkv6.cu:8-87).  `w` is the fp32 DECAY exp(-exp(w_raw)) (src/model_run.py:64),
 * `state` is fp32 [B,H,N,N] (value-major, like s above; [H,N,N] for B = 1 as the reference uses it) and is updated
 * in place.  The reference indexes the state without the batch (`wrong if B > 1`, cuda/rwkv6.cu:17); here every
 * batch row has its own state.  The fp16 flavour takes r, k, v, u, y in IEEE half: inputs are widened to fp32 in the
 * kernel (exact), the arithmetic and the state are fp32 and y is rounded to nearest even, as cuda/rwkv6.cu:8-71. */
int rwkv6_cuda_forward_bf16(int B, int T, int C, int H, float* state, const void* r, const void* k, const void* v,
                            const float* w, const void* u, void* y, void* stream);
int rwkv6_cuda_forward_fp16(int B, int T, int C, int H, float* state, const void* r, const void* k, const void* v,
                            const float* w, const void* u, void* y, void* stream);
int rwkv6_cuda_forward_fp32(int B, int T, int C, int H, float* state, const float* r, const float* k, const float* v,
                            const float* w, const float* u, float* y, void* stream);

/* ---- extended entry points -------------------------------------------------------------------------
 * flags (OR together): */
enum {
    WKV6_W_EW_F32 = 0,      /* w is fp32 ew = -exp(w_raw)                       (default) */
    WKV6_W_RAW = 1,         /* w is the raw decay in the I/O type               */
    WKV6_IO_F32 = 2,        /* every bf16 tensor is fp32 instead (numerics tests) */
    WKV6_S0_PER_BATCH = 4,  /* s0 is [B,H,N,N] (infctx) instead of [H,N,N] (state) */
    WKV6_ALGO_SCAN = 16,    /* force the exact token-serial kernels            */
    WKV6_CKPT_VALID = 32,   /* backward: `workspace` already holds the checkpoints written by wkv6_forward_ckpt_ex
                               (wkv6_bi: by wkv6bi_forward_ex with WKV6_BI_KEEP_CKPT) for the same inputs, so the backward
                               skips its own state pass(es) */
    WKV6_BI_KEEP_CKPT = 64, /* wkv6bi_forward_ex: also store the state checkpoints of both scans in `workspace` (which the
                               caller then hands to wkv6bi_backward_ex with WKV6_CKPT_VALID) */
    WKV6_PARTIALS_F32 = 128 /* backward: gu [B,C] and gs [B,H,N,N] are fp32 buffers -- they are per-batch partial sums that the
                               caller reduces over the batch, so keeping them unrounded lets the parameter gradient be rounded
                               once (the reference ABI, bf16 partials, rounds twice: src/model.py:181, 232) */
};
/* Bytes of scratch the backward needs (the forward needs none). */
size_t wkv6_backward_workspace_bytes(int B, int T, int C, int H);

/* s0 may be NULL (zero initial state); s_out may be NULL; s_out may alias s0. */
int wkv6_forward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                    const void* w, const void* u, const void* s0, void* s_out, void* y,
                    unsigned flags, void* stream);
/* Same as wkv6_forward_ex, and additionally stores the forward state every 64 tokens (fp32, 4 B per token-channel,
 * wkv6_backward_workspace_bytes() bytes in all) into `ckpt` -- the activation checkpoint a following
 * wkv6_backward_ex(..., workspace = ckpt, flags | WKV6_CKPT_VALID) consumes.  bf16 I/O, chunked kernels only;
 * returns WKV6_EUNSUPPORTED for WKV6_IO_F32 / WKV6_ALGO_SCAN. */
int wkv6_forward_ckpt_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                         const void* w, const void* u, const void* s0, void* s_out, void* y,
                         void* ckpt, size_t ckpt_bytes, unsigned flags, void* stream);
/* wkv6_forward_ckpt_ex with the per-head GroupNorm and the gate multiply that follow the operator in the time-mix block
 * (src/model.py:462-468: x = ln_x(x.view(B*T, C)).view(B, T, C); output(x * g)) fused into its store:
 *     out = GroupNorm_H(y; gamma, beta, eps) * gate,       y = the operator's bf16 output, exactly what nn.GroupNorm would see.
 * y may be NULL (inference: only `out` is written); ckpt may be NULL; stats (fp32 [B*T, H, 2]: mean, rstd per token and head,
 * what wkv6_gn_gate_backward consumes) may be NULL.  gate [B,T,C], gamma / beta [C], bf16.  bf16 I/O, chunked kernels only.
 * Returns WKV6_EUNSUPPORTED where the fusion does not apply (WKV6_IO_F32 / WKV6_ALGO_SCAN; so few (batch, head) pairs that two
 * workgroups share one): the caller then runs wkv6_forward_ckpt_ex + wkv6_gn_gate_forward. */
int wkv6_forward_gn_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const void* u,
                       const void* s0, void* s_out, void* y, void* ckpt, size_t ckpt_bytes, const void* gate, const void* gamma,
                       const void* beta, float eps, void* out, float* stats, unsigned flags, void* stream);
/* gu, gs may be NULL (skipped).  workspace: wkv6_backward_workspace_bytes() bytes, or NULL: the library takes a stream-ordered
 * allocation on `stream` for the duration of the call (hipMallocAsync / hipFreeAsync; safe from any number of streams). */
int wkv6_backward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v,
                     const void* w, const void* u, const void* s0, const void* gy, void* gr,
                     void* gk, void* gv, void* gw, void* gu, void* gs, void* workspace,
                     size_t workspace_bytes, unsigned flags, void* stream);
/* lens: int32 [B] device array, number of leading tokens both scans cover (NULL: derive from mask).
 * workspace: at least wkv6bi_workspace_bytes() bytes (NULL: stream-ordered allocation for the duration of the call), or EXACTLY
 * wkv6bi_kept_bytes() bytes -- the part that must live from a WKV6_BI_KEEP_CKPT forward to its backward (row lengths and the two
 * scans' checkpoints); the fp32 [B,T,C] side buffers (one in the forward, four in the backward) are then stream-ordered scratch
 * of the call.  Any other size is refused with WKV6_EWORKSPACE. */
int wkv6bi_forward_ex(int B, int T, int C, int H, const int* mask, const int* lens, const void* r,
                      const void* k, const void* v, const void* w, const void* u, void* y,
                      void* workspace, size_t workspace_bytes, unsigned flags, void* stream);
int wkv6bi_backward_ex(int B, int T, int C, int H, const int* mask, const int* lens, const void* r,
                       const void* k, const void* v, const void* w, const void* u, const void* gy,
                       void* gr, void* gk, void* gv, void* gw, void* gu, void* workspace,
                       size_t workspace_bytes, unsigned flags, void* stream);
size_t wkv6bi_workspace_bytes(int B, int T, int C, int H);
size_t wkv6bi_kept_bytes(int B, int T, int C, int H);

/* ---- packed variable-length batches ("varlen"): the sequences of a batch lie back to back in [total_T, C] tensors, no padding anywhere.
 * cu_seqlens: int32 [n_seq + 1] on the device, sequence s = tokens cu[s] .. cu[s+1]-1; the host never reads it (stream-ordered,
 * graph-capturable, nothing synchronises).  Lengths are clamped on the device: len_s = clamp(cu[s+1] - cu[s], 0, max_seqlen), and a
 * sequence never reaches past total_T; a zero-length sequence is legal and touches no token.  Every sequence starts from s0 (NULL: zero):
 *   r,k,v,w,y,gy,gr,gk,gv,gw : [total_T,C]     u : [H,N]
 *   s0 : [H,N,N] shared, or [n_seq,H,N,N] with WKV6_S0_PER_BATCH     s_out, gs : [n_seq,H,N,N]     gu : [n_seq,C]
 * (gu, gs are per-SEQUENCE partials that the caller sums, as over the batch elsewhere; s_out of an empty sequence is s0, its gu / gs are 0).
 * Rows outside every sequence: for a non-decreasing cu_seqlens, every row of y, gr, gk, gv, gw that lies in no served sequence -- the rows
 * before cu[0], the rows from cu[n_seq] on, and the part of a sequence that max_seqlen cuts off -- is written as +0, and the inputs on
 * those rows are never read (a fixed-capacity buffer that is filled differently every step needs no clearing by the caller, and what
 * lies in its unused rows, NaN included, reaches nothing).  Only these gaps are zeroed, by the preparation launch; a batch that covers
 * every row pays no memset (the chunked backward under WKV6_CKPT_VALID, which otherwise has no preparation launch, runs it for the
 * gaps alone: 2-4 us per call on an MI355X, profiles/varlen_time.txt).  The gaps are zeroed with 16-byte stores: y, gr, gk, gv, gw must
 * be 16-byte aligned, else WKV6_EINVAL (every row then is: a row is a multiple of 128 bytes).  A cu_seqlens that decreases somewhere is out of contract: the calls stay memory-safe (next paragraph),
 * what the rows hold is unspecified.
 * One workgroup per (sequence, head), longest sequences first.  Per-lane offsets are 32-bit within a sequence:
 * (max_seqlen + 64) * C < 2^31 (2^30 with the fp32 ew decay on the chunked kernels), else WKV6_EUNSUPPORTED; the sequence origin is
 * 64-bit, so total_T * C may pass 2^31.
 * flags: WKV6_W_RAW, WKV6_IO_F32, WKV6_ALGO_SCAN (the last two run the exact scan kernels), WKV6_S0_PER_BATCH, WKV6_PARTIALS_F32,
 * WKV6_CKPT_VALID as elsewhere; any other bit returns WKV6_EINVAL.
 * workspace: wkv6_varlen_workspace_bytes() bytes -- a host-side bound that needs no device data: H * (total_T / 64 + n_seq) checkpoint
 * slots of 16 KB (sequence s uses ceil(len_s / 64) of them per head) + four int32 [n_seq] arrays (lengths, token offsets, checkpoint
 * offsets, dispatch order).  It carries the checkpoints from the forward to a backward called with WKV6_CKPT_VALID on the same inputs;
 * without that flag the backward runs its own state pass.  Forward: workspace NULL = keep no checkpoints (the int arrays are a
 * stream-ordered allocation of the call).  Backward: NULL = stream-ordered allocation of the whole workspace (WKV6_ENULL together with
 * WKV6_CKPT_VALID).  A non-NULL workspace shorter than the bound is refused with WKV6_EWORKSPACE.
 * Reversal maps and the pair launch on packed rows: wkv6_*_varlen_rev_ex / wkv6_*_varlen_pair_ex below.
 * Not available packed (out of scope, not half-supported): two workgroups per head, the two-level scan over T, the GroupNorm epilogue,
 * wkv6_bi. */
size_t wkv6_varlen_workspace_bytes(long total_T, int n_seq, int C, int H);
int wkv6_forward_varlen_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                           const void* v, const void* w, const void* u, const void* s0, void* s_out, void* y, void* workspace,
                           size_t workspace_bytes, unsigned flags, void* stream);
int wkv6_backward_varlen_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                            const void* v, const void* w, const void* u, const void* s0, const void* gy, void* gr, void* gk, void* gv,
                            void* gw, void* gu, void* gs, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* ---- rwkv6 on packed batches (stateful forward-only inference for a serving loop): rwkv6_cuda_forward_* over the sequences of one
 * [total_T, C] buffer -- prompts of any mix of lengths, prefill next to one-token decode steps -- each with its state in a slot of a
 * caller-owned pool.  Padding a stateful operator is wrong, not just wasteful: the state would scan the pad tokens.
 *   r,k,v,y : [total_T,C] in the I/O type (bf16 / fp16 / fp32)     w : fp32 [total_T,C], the DECAY exp(-exp(w_raw)) as above     u : [H,N]
 *   state_pool : fp32 [n_slots,H,N,N], value-major as above        state_slot : int32 [n_seq] on the device, or NULL: slot = sequence
 *                                                                  index (n_slots >= n_seq then, else WKV6_EINVAL)
 * Sequence s reads its initial state from slot state_slot[s] and leaves its final state there, in place.  A slot outside [0, n_slots)
 * means "no state": the sequence starts from zero and its final state is not stored (the slot is tested on the device before any
 * address is formed: a garbage slot touches no memory).  A sequence of (clamped) length 0 neither reads nor writes its slot.  Two
 * sequences of non-zero length that name one slot in the same call are out of contract: what that slot holds afterwards is unspecified,
 * the call stays memory-safe.  Slots that no sequence names are not touched.
 * cu_seqlens follows the wkv6_*_varlen_ex rules above: device-only and clamped on the device, max_seqlen cuts a sequence, empty
 * sequences are legal, rows of y outside every sequence are written as +0 and the inputs there are never read, y must be 16-byte
 * aligned (WKV6_EINVAL).
 * Contract: for every sequence, y and the final state are bit-identical to rwkv6_cuda_forward_<io>(B = 1, T = len, ...) on that sequence
 * alone with its slot's state (for calls that one takes in one scan level, i.e. below 2048 tokens).
 * Routing, as that call does it per sequence: bf16 sequences of 32 tokens and more run on the chunked MFMA kernel, shorter ones and every
 * fp16 / fp32 sequence on the exact scan.  bf16 with max_seqlen < 32 (a decode step) is one scan launch; otherwise the chunked launch
 * serves the lengths [32, inf) and a scan launch the lengths [0, 32) of the same prepared batch -- the host never reads cu_seqlens.
 * flags: WKV6_ALGO_SCAN forces the scan for every length; any other bit returns WKV6_EINVAL.
 * Limits: (max_seqlen + 64) * C < 2^30 on the chunked route, < 2^31 on the scan route, else WKV6_EUNSUPPORTED.  Argument errors return
 * before anything is launched: WKV6_EINVAL (shapes, n_slots < 1, flags, alignment), WKV6_ENULL (state_pool, cu_seqlens or a tensor).
 * workspace: rwkv6_varlen_workspace_bytes(n_seq) bytes, the four prepared int32 [n_seq] arrays (no checkpoint is ever kept); NULL: a
 * stream-ordered allocation of the call (callers that replay graphs pass one); a non-NULL workspace shorter than that: WKV6_EWORKSPACE.
 * Out of scope, not half-supported: a raw-w decay kind, the GroupNorm epilogue, reversal maps, two workgroups per head, the two-level
 * scan over T, a backward, the C++ torch shim, snapshots at positions that are no multiple of 64 tokens of the call (the caller aligns
 * its chunk boundaries). */
size_t rwkv6_varlen_workspace_bytes(int n_seq);
int rwkv6_forward_varlen_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                              void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);
int rwkv6_forward_varlen_fp16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                              void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);
int rwkv6_forward_varlen_fp32(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                              int n_slots, float* state_pool, const float* r, const float* k, const float* v, const float* w,
                              const float* u, float* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* ---- ... with state snapshots and a separate output slot (prefix caching: the state of a prompt every few hundred tokens, and requests that
 * start from a cached state without overwriting it).  The argument list of rwkv6_forward_varlen_* and then
 *   state_slot_out : int32 [n_seq] on the device, or NULL      snap_every : 0, or a multiple of 64
 *   cu_snap : int32 [n_seq + 1], snap_slot : int32 [n_snap], both on the device (may be NULL when snap_every == 0)
 * Sequence s reads its initial state from slot state_slot[s] and leaves its final state in slot state_slot_out[s] of the same pool; each
 * of the two is validated on its own, on the device, before any address is formed: a source outside [0, n_slots) starts the sequence from
 * zero, a destination outside it stores nothing.  state_slot_out == NULL: the destination is the source, the in-place update of the plain
 * call.
 * Snapshots: with len_s the clamped length and cu_snap[s], cu_snap[s+1] clamped into [0, n_snap], sequence s keeps
 * m_s = min(len_s / snap_every, max(cu_snap[s+1] - cu_snap[s], 0)) snapshots; snapshot j < m_s is the state after the sequence's first
 * (j + 1) * snap_every tokens in this call and goes to slot snap_slot[cu_snap[s] + j] of the pool, in the pool's layout.  A snapshot slot
 * outside the pool is skipped.  A snapshot at position len_s is stored as well as the final state.  The host reads none of the arrays: the
 * call stays stream-ordered and graph-capturable.
 * Contract:
 *  - Any number of sequences of one call may name the same source slot (requests that fan out from one cached prefix).
 *  - Two writers of one slot in the same call are out of contract, and so is a slot that one sequence of non-zero length writes and
 *    another reads; final states and snapshots both count as writes.  What such slots hold afterwards is unspecified; the call stays
 *    memory-safe.  The one defined overlap is the in-place use: a sequence's destination is its own source.
 *  - A sequence of (clamped) length 0 reads nothing, writes nothing and takes no snapshot; it does not copy source to destination.
 *  - For every sequence, y and the destination slot are bit-identical to what rwkv6_forward_varlen_<io> leaves from the same source
 *    state, and snapshot j is bit-identical to the final state that call leaves when the sequence is cut to (j + 1) * snap_every tokens.
 * Routing, the length window, the limits and the workspace are those of rwkv6_forward_varlen_<io>.  Refused before anything is launched, in
 * addition to what that call refuses: snap_every < 0 or no multiple of 64, n_snap < 0 (WKV6_EINVAL); snap_every > 0 with a NULL cu_snap or
 * snap_slot (WKV6_ENULL). */
int rwkv6_forward_varlen_snap_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                   void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                   int snap_every, const int* cu_snap, const int* snap_slot, int n_snap);
int rwkv6_forward_varlen_snap_fp16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                   void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                   int snap_every, const int* cu_snap, const int* snap_slot, int n_snap);
int rwkv6_forward_varlen_snap_fp32(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                   int n_slots, float* state_pool, const float* r, const float* k, const float* v, const float* w,
                                   const float* u, float* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream,
                                   const int* state_slot_out, int snap_every, const int* cu_snap, const int* snap_slot, int n_snap);

/* ---- ... with long sequences cut over T (a long prompt of a serving batch: one workgroup per (sequence, head) leaves most of the chip idle
 * for the whole prefill).  The argument list of rwkv6_forward_varlen_snap_bf16 and then
 *   seg_len : 0, or a multiple of 64
 * seg_len == 0 is rwkv6_forward_varlen_snap_bf16: the same launches, the same results.  With seg_len > 0 every sequence whose clamped length
 * passes seg_len is cut at multiples of seg_len into ITEMS (item g = its tokens [g * seg_len, min((g + 1) * seg_len, len_s))) that run as one
 * workgroup per (item, head); every other sequence is one item and runs as in the snap call.  The cut is made on the device, behind the clamps
 * of cu_seqlens: the host never reads it and bounds the item table by n_seq + total_T / seg_len entries (the grid is that times H; workgroups
 * without an item return at once).  A sequence whose full segments do not fit under total_T / seg_len together with those in front of it --
 * only a cu_seqlens that is no partition of the rows can cause that -- runs uncut; the call stays memory-safe.  Dispatch order: the full
 * segments first, then the tails and the uncut sequences, longest first.
 * Three stages behind the one preparation launch, the two-level scan of the dense call on packed rows:
 *   1. every item that has a successor runs the state recurrence from a zero state (its own contribution A and its log-decay sums);
 *   2. one small kernel per (sequence, head) chains them from the source slot, S_in(g + 1) = 2^{dsum_g} (.) S_in(g) + A_g, into scratch;
 *   3. the forward per item from its entry state.
 * Every state the call stores is a running state of stage 3: the final state comes from a sequence's last item, snapshot j from the item
 * that contains position (j + 1) * snap_every.  Stages 1 and 2 only read the pool, and the first item of a cut sequence starts from a copy
 * of its source slot that stage 2 took, so the hazard rules of the snap call hold unchanged: fan-out from one source slot and the in-place
 * use are legal.
 * Contract:
 *  - Sequences that are not cut: y, the destination slot and the snapshots are bit-identical to rwkv6_forward_varlen_snap_bf16.
 *  - Cut sequences: rows [0, seg_len) of y and every snapshot at a position <= seg_len are bit-identical to that call; behind them the
 *    results differ from it by the re-association of the state across the cut (the entry state is rounded once per segment in another order),
 *    within the bounds of the dense two-level path, whose y it reproduces bit for bit (rwkv6_cuda_forward_bf16(B = 1) at the same cut).
 *  - Snapshot j is bit-identical to the final state of the same call, with the same seg_len, on the sequence cut to (j + 1) * snap_every
 *    tokens; a snapshot at position len_s equals the final state.
 * Routing: bf16 on the chunked route only; sequences below 32 tokens take the exact scan as before.  Refused before anything is launched, in
 * addition to what the snap call refuses (with the same codes): seg_len < 0 or no multiple of 64 (WKV6_EINVAL); seg_len > 0 together with
 * WKV6_ALGO_SCAN (WKV6_EUNSUPPORTED).  No relation between seg_len and snap_every is required.  Limits stay per sequence:
 * (max_seqlen + 64) * C < 2^30.
 * workspace: rwkv6_varlen_split_workspace_bytes(total_T, n_seq, seg_len, C, H) bytes from host data alone (0 for a bad shape or seg_len;
 * rwkv6_varlen_workspace_bytes(n_seq) at seg_len == 0): the int arrays of the plain call, the item table, and per item and head A, the
 * entry state (16 KB each) and the decay sums.  NULL: a stream-ordered allocation of the call; shorter than that: WKV6_EWORKSPACE.
 * Out of scope, not half-supported: what the snap call lists except the two-level scan over T, which this entry point is; fp16 / fp32 I/O
 * (they stay on the exact scan); the C++ torch shim; an automatic choice of seg_len (the caller knows its batch: INTEGRATION.md). */
size_t rwkv6_varlen_split_workspace_bytes(long total_T, int n_seq, int seg_len, int C, int H);
int rwkv6_forward_varlen_split_bf16(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const int* state_slot,
                                    int n_slots, float* state_pool, const void* r, const void* k, const void* v, const float* w, const void* u,
                                    void* y, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const int* state_slot_out,
                                    int snap_every, const int* cu_snap, const int* snap_slot, int n_snap, int seg_len);

/* ---- wkv5 (RWKV-5: the decay is a parameter, constant over batch and time): replaces cuda_forward / cuda_backward of
 * cuda/wkv5_op.cpp:5-6 (cuda/wkv5_cuda.cu:190-202).  w, u : [H,N];  gw, gu : [B,C] per-batch partials (the caller sums them over
 * the batch, src/model.py:283-284).  `eew` is the fp32 decay exp(-exp(w_raw)) and `ew` the fp32 -exp(w_raw) that src/model.py:260-261
 * builds; gw is the gradient with respect to the RAW w (gw[b][i] = ew[i] eew[i] dL_b/d eew[i], cuda/wkv5_cuda.cu:119-143) and is
 * exactly 0 for T <= 2.  Exact fp32 token-serial kernels with the decay, u and the gw / gu sums in registers: 8 B per token-channel
 * in the forward (r, k, v in, y out), 14 B of tensors in the backward (r, k, v, gy in, gr, gk, gv out), no workspace, no atomics
 * (results are bit-reproducible).  gw, gu may be NULL (skipped). */
int wkv5_cuda_forward(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* eew, const void* u,
                      void* y, void* stream);
int wkv5_cuda_backward(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* eew, const float* ew,
                       const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu, void* stream);
/* The same with flags (declared below; any other bit returns WKV6_EUNSUPPORTED):
 *   WKV6_W_RAW         w is the raw [H,N] parameter in the I/O type, decay and ew are formed in the kernel (`ew` is ignored, may be NULL);
 *                      without it w is the fp32 decay and the backward needs `ew` unless gw is NULL
 *   WKV6_IO_F32        every bf16 tensor (w under WKV6_W_RAW and the partials included) is fp32
 *   WKV6_PARTIALS_F32  gw, gu [B,C] are fp32: the parameter gradient is rounded once, after the caller's sum over the batch
 *   WKV6_ALGO_SCAN     accepted, no effect: these are the only kernels of the operator */
int wkv5_forward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const void* u,
                    void* y, unsigned flags, void* stream);
int wkv5_backward_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w, const float* ew,
                     const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu, unsigned flags,
                     void* stream);

/* ---- partially reversed sequences: replaces the torch.gather round trips around the operator in the
 * bidirectional compositions -- src/model_bi.py:331-348 (k, v reversed, y un-reversed) and src/model_ext.py:410-437 (every
 * tensor reversed).  For batch row b, tokens [0, rev_n[b]) of the tensors named in rev_mask are read in reverse order (scan
 * position p < rev_n[b] <-> token rev_n[b]-1-p, exactly reverse_x_idx of src/model_ext.py:410-417); positions >= rev_n[b]
 * keep their place and ARE scanned (the sentence-embedding position sits right behind the reversed span).  WKV6_REV_Y applies
 * to y (written through the map) and, in the backward, to gy; each gradient follows its tensor's bit.  rev_n: int32 [B] on
 * the device.  bf16 I/O on the chunked kernels; WKV6_IO_F32 / WKV6_ALGO_SCAN run the exact scan kernels with the same index
 * maps (ckpt is ignored there).  ckpt may be NULL. */
enum { WKV6_REV_R = 1, WKV6_REV_K = 2, WKV6_REV_V = 4, WKV6_REV_W = 8, WKV6_REV_Y = 16 };
int wkv6_forward_rev_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w,
                        const void* u, void* y, void* ckpt, size_t ckpt_bytes, const int* rev_n, unsigned rev_mask,
                        unsigned flags, void* stream);
int wkv6_backward_rev_ex(int B, int T, int C, int H, const void* r, const void* k, const void* v, const void* w,
                         const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw, void* gu,
                         void* workspace, size_t workspace_bytes, const int* rev_n, unsigned rev_mask, unsigned flags,
                         void* stream);

/* ---- both operator calls of a bidirectional time-mix layer in ONE launch (second half): the
 * forward-direction call and the reversed-direction call of src/model_bi.py:331-348 (composition B: same r, w, reversed k, v, y)
 * and src/model_ext.py:421-437 (composition C: separately projected, fully reversed) are two problems of one shape; a grid of
 * 2 B H workgroups serves problem s[0] with its first B H slots and s[1] with the rest -- one launch, one tail.  Each set names its
 * own tensors, reversal map (rev_n NULL = none) and checkpoint buffer (wkv6_backward_workspace_bytes() bytes each; required by
 * the backward, which must find them filled by wkv6_forward_pair_ex; may be NULL in a forward nobody differentiates).  u [H,N]
 * is shared.  bf16 I/O, chunked kernels; flags: WKV6_W_RAW / WKV6_PARTIALS_F32 as elsewhere (WKV6_EUNSUPPORTED with WKV6_IO_F32 /
 * WKV6_ALGO_SCAN).  Results are bit-identical to two wkv6_forward_rev_ex / wkv6_backward_rev_ex calls. */
typedef struct wkv6_seq_set {
    const void *r, *k, *v, *w;          /* [B,T,C] inputs */
    void* y;                            /* forward: [B,T,C] output */
    const void* gy;                     /* backward: [B,T,C] */
    void *gr, *gk, *gv, *gw;            /* backward: [B,T,C] gradients */
    void* gu;                           /* backward: [B,C] per-batch partials of this problem (bf16, or fp32 with WKV6_PARTIALS_F32) */
    void* ckpt;                         /* state checkpoints written by the forward, read by the backward */
    size_t ckpt_bytes;
    const int* rev_n;                   /* int32 [B] on the device, or NULL */
    unsigned rev_mask;                  /* WKV6_REV_* */
} wkv6_seq_set;
int wkv6_forward_pair_ex(int B, int T, int C, int H, const void* u, const wkv6_seq_set* s, unsigned flags, void* stream);
int wkv6_backward_pair_ex(int B, int T, int C, int H, const void* u, const wkv6_seq_set* s, unsigned flags, void* stream);

/* ---- reversal maps and the pair launch on packed variable-length batches: the bidirectional compositions without padding.
 * wkv6_*_varlen_rev_ex = wkv6_*_varlen_ex (same tensors, cu_seqlens, clamping, gap rows, alignment, row limit and workspace rules)
 * with the map of wkv6_*_rev_ex applied WITHIN every sequence: rev_n is int32 [n_seq] on the device (never read by the host), clamped
 * there to [0, len_s] with len_s taken after the max_seqlen clamp; scan position p < rev_n[s] of a tensor named in rev_mask is token
 * cu[s] + rev_n[s] - 1 - p, positions from rev_n[s] on keep their place and are scanned.  rev_n NULL = no map: the plain packed results,
 * bit for bit.  rev_mask bits outside WKV6_REV_* return WKV6_EINVAL.  There is no initial state (as in wkv6_*_rev_ex): every sequence
 * starts from zero, gu is [n_seq,C].
 * flags: WKV6_W_RAW, WKV6_IO_F32, WKV6_ALGO_SCAN (the last two: the exact scan kernels with the same maps), WKV6_PARTIALS_F32,
 * WKV6_CKPT_VALID; any other bit -- WKV6_S0_PER_BATCH included -- returns WKV6_EINVAL. */
int wkv6_forward_varlen_rev_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                               const void* v, const void* w, const void* u, void* y, void* workspace, size_t workspace_bytes,
                               const int* rev_n, unsigned rev_mask, unsigned flags, void* stream);
int wkv6_backward_varlen_rev_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* r, const void* k,
                                const void* v, const void* w, const void* u, const void* gy, void* gr, void* gk, void* gv, void* gw,
                                void* gu, void* workspace, size_t workspace_bytes, const int* rev_n, unsigned rev_mask, unsigned flags,
                                void* stream);
/* Two such problems over the SAME sequences in one grid of 2 n_seq H workgroups (slots [0, n_seq H) serve s[0], the rest s[1]), behind the
 * one preparation launch, which zeroes the gap rows of both problems' outputs.  Tensors of a set are [total_T,C], s[i].gu is [n_seq,C],
 * s[i].rev_n int32 [n_seq] or NULL.  s[i].ckpt / ckpt_bytes is one wkv6_varlen_workspace_bytes() workspace per problem; the prepared int
 * arrays, which both problems read, live in s[0]'s.  The backward needs both workspaces as wkv6_forward_varlen_pair_ex left them; a
 * forward nobody differentiates may pass NULL for either.  flags: WKV6_W_RAW, WKV6_PARTIALS_F32; WKV6_IO_F32 / WKV6_ALGO_SCAN return
 * WKV6_EUNSUPPORTED, any other bit WKV6_EINVAL.  Results (checkpoints included) are bit-identical to two wkv6_*_varlen_rev_ex calls. */
int wkv6_forward_varlen_pair_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* u,
                                const wkv6_seq_set* s, unsigned flags, void* stream);
int wkv6_backward_varlen_pair_ex(long total_T, int n_seq, int max_seqlen, int C, int H, const int* cu_seqlens, const void* u,
                                 const wkv6_seq_set* s, unsigned flags, void* stream);

/* ---- elementwise neighbours of the operator in the RWKV-6 time-mix block; bf16 only ----
 * ddlerp (src/model.py:435-448): xx = shift(x) - x; out[s] = x + xx * (maa[s] + m[s]), s < NS.
 *   x [B,T,C]; shifted0 [B,C] = token in front of each row (NULL: zero, nn.ZeroPad2d((0,0,1,-1))); m [NS,B,T,C] or NULL;
 *   maa [NS,C]; out [NS,B,T,C].  Supported: (NS=1, m NULL or not), (NS=5, m given), (NS=2, m NULL: the channel-mix FFN's
 *   two lerps); any other pair returns WKV6_EUNSUPPORTED.
 * backward: dx [B,T,C], dm [NS,B,T,C] (NULL iff m NULL), dmaa_part fp32 [nparts,NS,C] partial sums (caller adds them). */
int wkv6_ddlerp_forward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                        void* out, void* stream);
int wkv6_ddlerp_backward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                         const void* dout, void* dx, void* dm, float* dmaa_part, int nparts, void* stream);
/* The same with the shift taken over the stream "first rev_n[b] tokens of row b reversed, the rest in place" while x, m, out
 * stay in the original token order (row n2: the reversed half of src/model_ext.py:421-437 without gathering x).  rev_n: int32
 * [B] on the device, NULL = plain shift. */
int wkv6_ddlerp_rev_forward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                            const int* rev_n, void* out, void* stream);
int wkv6_ddlerp_rev_backward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                             const int* rev_n, const void* dout, void* dx, void* dm, float* dmaa_part, int nparts, void* stream);
/* The same on a packed variable-length batch: x, m, out, dout, dx, dm are [total_T,C] / [NS,total_T,C]; the token in front of the first
 * token of sequence s is shifted0[s] ([n_seq,C], NULL: zero), never the last token of sequence s-1.  cu_seqlens: int32 [n_seq + 1] on
 * the device (not read by the host).  A token finds its sequence by bisection in cu_seqlens: no per-token flag, 0 extra bytes per token. */
int wkv6_ddlerp_varlen_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                               const void* m, const void* maa, void* out, void* stream);
int wkv6_ddlerp_varlen_backward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                const void* m, const void* maa, const void* dout, void* dx, void* dm, float* dmaa_part, int nparts,
                                void* stream);
/* ... with the shift of sequence s taken over the stream "its first rev_n[s] tokens reversed, the rest in place" (rev_n int32 [n_seq] on
 * the device, clamped to the sequence's length; NULL = the plain packed shift).  The token in front of the stream's first token is
 * shifted0[s], never a token of another sequence. */
int wkv6_ddlerp_varlen_rev_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                   const void* m, const void* maa, const int* rev_n, void* out, void* stream);
int wkv6_ddlerp_varlen_rev_backward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                    const void* m, const void* maa, const int* rev_n, const void* dout, void* dx, void* dm,
                                    float* dmaa_part, int nparts, void* stream);
/* ---- the token-shift state of a serving loop as a device-side slot pool (bf16, forward only), beside the WKV state pool of
 * rwkv6_forward_varlen_*: shift_pool is bf16 [n_slots,C], one pool per sub-layer; row p is the last token slot p's sequence was served.
 *
 * wkv6_ddlerp_slots_forward: wkv6_ddlerp_varlen_forward, except that the token in front of sequence s is row slot[s] of shift_pool instead
 * of row s of a gathered shifted0.  The slot is judged on the device before an address is formed: a slot outside [0, n_slots) means a zero
 * token.  slot (int32 [n_seq] on the device, never read by the host) == NULL: slot = sequence index, which needs n_slots >= n_seq
 * (WKV6_EINVAL otherwise).  Any number of sequences may name one slot; the pool is only read.  Which row opens which sequence is the
 * rule of the varlen call (the last sequence whose boundary is the row), so an empty sequence never reads its slot.  Same (NS, m) pairs,
 * same arithmetic: results are bit-identical to wkv6_ddlerp_varlen_forward(shifted0 = the gathered rows).
 *
 * wkv6_shift_keep: one launch that stores what the batch leaves, writing only the rows that change.  With
 *   a_s = clamp(cu_seqlens[s], 0, total_T), b_s = clamp(cu_seqlens[s+1], 0, total_T), len_s = min(max(b_s - a_s, 0), max_seqlen):
 *   - if len_s > 0 and slot_out[s] lies in the pool, row a_s + len_s - 1 of x goes to shift_pool[slot_out[s]] (slot_out == NULL: the
 *     sequence index, n_slots >= n_seq as above);
 *   - snap_every > 0: with cu_snap clamped into [0, n_snap] and m_s = min(len_s / snap_every, max(cu_snap[s+1] - cu_snap[s], 0)), row
 *     a_s + (j + 1) * snap_every - 1 goes to shift_pool[snap_slot[cu_snap[s] + j]] for every j < m_s whose slot lies in the pool -- the
 *     clamps and the m_s of rwkv6_forward_varlen_snap_*, so that a snapshot's shift token and its WKV state land under one slot number.
 *     (No multiple-of-64 rule here: any snap_every >= 0.  snap_every == 0 or n_snap == 0: no snapshots, cu_snap / snap_slot may be NULL.)
 * One workgroup per candidate row (n_seq + n_snap of them; a snapshot entry finds its sequence by bisection in cu_snap); dead candidates
 * return before any access.  Every index is clamped or judged before use: garbage in any int array touches no memory outside x and the
 * pool.  The pool is not read; rows that no live candidate names keep their bits, and rows are copied as bits.  Two live writers of one
 * row are out of contract (one of them wins; the call stays memory-safe).
 *
 * The two are separate launches on purpose: with slot_out == slot (a decode loop's in-place use) the workgroup of a sequence's first
 * token reads the row that the workgroup of its last token writes; stream order between the launches makes that defined.
 *
 * Refused before any launch: WKV6_EINVAL -- C (as every kernel here: a multiple of 64, at most 4096), total_T, n_seq, n_slots or
 * max_seqlen < 1, snap_every < 0, n_snap < 0, x / out / shift_pool not 8-byte aligned, x (shift_keep) or out (ddlerp_slots) overlapping
 * the pool; WKV6_ENULL -- a NULL tensor, cu_seqlens or pool, cu_snap or snap_slot NULL while snap_every > 0 and n_snap > 0;
 * WKV6_EUNSUPPORTED -- total_T > INT_MAX, an (NS, m) pair the ddlerp does not have. */
int wkv6_ddlerp_slots_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x,
                              const void* shift_pool, int n_slots, const int* slot,
                              const void* m, const void* maa, void* out, void* stream);
int wkv6_shift_keep(long total_T, int n_seq, int max_seqlen, int C, const int* cu_seqlens, const void* x,
                    void* shift_pool, int n_slots, const int* slot_out,
                    int snap_every, const int* cu_snap, const int* snap_slot, int n_snap, void* stream);
/* ---- per-sequence LoRA adapters on a packed batch (bf16, forward only; csrc/wkv6_lora.hip): the reference switches one adapter per call
 * (src/layers.py: LoraLinear.set_adapter); here every sequence of the batch names its own, on the device, and the batch runs once.
 *   x bf16 [total_T,K];  y bf16 [total_T,N], updated in place: it already holds x W^T of the base GEMM;
 *   A_pool bf16 [n_adapters,R,K], B_pool bf16 [n_adapters,N,R] (the layout of nn.Linear weights = the reference's lora_A / lora_B);
 *   scale fp32 [n_adapters] = alpha / r;  adapter int32 [n_seq] and cu_seqlens int32 [n_seq + 1] on the device, never read by the host.
 * With a_s = clamp(cu_seqlens[s], 0, total_T), b_s = clamp(cu_seqlens[s+1], 0, total_T): a row t finds its sequence s by the varlen rule
 * (the last s with cu_seqlens[s] <= t) and is served when a_s <= t < b_s -- every row of the sequence, no max_seqlen cut -- and
 * a = adapter[s] lies in [0, n_adapters).  A served row gets
 *     xa[t,j] = bf16( sum_k x[t,k] A[a,j,k] )                                  (fp32 accumulation, rounded to bf16 once)
 *     y[t,n]  = bf16( fmaf(scale[a], sum_j xa[t,j] B[a,n,j], float(y[t,n])) )
 * Every other row -- in no sequence, or of a sequence whose adapter lies outside the pool; -1 is the value for "base model only" -- keeps
 * its bits: it is not read-modify-written.  The adapter number is judged before an address is formed from it, every cu_seqlens entry is
 * clamped or compared before use: garbage in either int array touches no memory outside the arguments.  An adapter of lower rank is
 * zero-padded to R by whoever fills the pools.
 * Two launches in stream order, "shrink" (xa into the workspace, bf16 [total_T,R]) and "expand"; tiles of 16 packed rows on the 16x16x32
 * bf16 MFMAs, operands straight from global memory.  Every output element is its own dot product: the split of K over the waves of a
 * shrink workgroup depends on K alone and is summed in a fixed order, there are no atomics, so a row's result does not depend on the
 * rows that share its tile or its batch -- a mixed batch equals one call per sequence bit for bit.  A tile that holds several adapters
 * is served group by group, rows selected by lane, never masked by a multiply: a NaN or Inf in one adapter's matrices reaches only the
 * rows that name it.
 * wkv6_lora_packed_workspace_bytes: total_T * R * 2 rounded up to a multiple of 256; 0 for a total_T or an R the call refuses.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- total_T, n_seq, n_adapters or R < 1, K or N not a multiple of 64 in
 * [64, 16384]; (2) WKV6_EUNSUPPORTED -- R outside {8, 16, 32, 64}, total_T > INT_MAX; (3) WKV6_ENULL -- any NULL pointer (workspace
 * included); (4) WKV6_EINVAL -- x, A_pool, B_pool, y or workspace not 16-byte aligned, cu_seqlens, adapter or scale not 4-byte aligned,
 * y overlapping x, A_pool or B_pool; (5) WKV6_EWORKSPACE -- workspace_bytes below wkv6_lora_packed_workspace_bytes(total_T, R). */
size_t wkv6_lora_packed_workspace_bytes(long total_T, int R);
int wkv6_lora_packed_bf16(long total_T, int n_seq, int K, int N, int R, int n_adapters,
                          const int* cu_seqlens, const int* adapter,
                          const void* x, const void* A_pool, const void* B_pool, const float* scale,
                          void* y, void* workspace, size_t workspace_bytes, void* stream);
/* ---- the two low-rank pairs in front of the time-mix projections (bf16, forward only; csrc/wkv6_lowrank.hip): the reference forms the
 * operator's inputs with a chain of small matmuls around its token-shift lerps (src/model.py:435-452); here each pair is two launches.
 * wkv6_tmix_lerp_lowrank_bf16, with xp[t] the token in front of row t (below) and fp32 arithmetic between the roundings:
 *     lead[t,k]    = bf16( fmaf(xp[t,k] - x[t,k], maa_x[k], x[t,k]) )                       (never stored)
 *     low[t,j]     = bf16( tanh( float( bf16( sum_k lead[t,k] W1t[j,k] ) ) ) )              j < 5 D; bf16 [total_T, 5 D] in the workspace
 *     corr_s[t,n]  = bf16( sum_j low[t, s D + j] W2t[s,n,j] )                               (never stored)
 *     out[s][t,n]  = bf16( fmaf(xp[t,n] - x[t,n], maa5[s,n] + corr_s[t,n], x[t,n]) )        s = 0..4: the planes w, k, v, r, g
 * wkv6_decay_lowrank_bf16:
 *     low[t,j] = bf16( tanh( float( bf16( sum_k xw[t,k] D1t[j,k] ) ) ) ),   w[t,n] = bf16( time_decay[n] + bf16( sum_j low[t,j] D2t[n,j] ) )
 * These are the rounding points of wkv6_ddlerp_*_forward (NS = 1), a bf16 matmul, tanh, a bf16 matmul and wkv6_ddlerp_*_forward (NS = 5)
 * in a row; only how the sums inside the two contractions are taken is the kernels' own: the shrink adds the fp32 results of its MFMAs (32
 * products each) in fp64 and rounds the sum to bf16 once, tanh is taken in fp64 and rounded once; the expand is an fp32 MFMA chain.
 *   x bf16 [total_T,C];  maa_x bf16 [C];  maa5 bf16 [5,C];  W1t bf16 [5 D,C] and W2t bf16 [5,C,D]: time_maa_w1 and time_maa_w2 in
 *   nn.Linear layout [out, in], as the LoRA pools are;  out bf16 [5,total_T,C];  D in {32, 64};  C a multiple of 64, at most 4096.
 *   xw bf16 [rows,C];  D1t bf16 [Dd,C];  D2t bf16 [N,Dd];  time_decay bf16 [N];  w bf16 [rows,N];  Dd in {64, 128};  C and N as C above.
 * The token in front of a row follows wkv6_ddlerp_slots_forward: row t is the first row of sequence s (the last s with cu_seqlens[s] <= t)
 * iff cu_seqlens[s] == t and then takes front[slot[s]]; every other row, rows outside every sequence included, takes row t - 1, and
 * row 0 takes zero if it opens nothing.  front bf16 [n_slots,C], NULL: zero tokens;  slot int32 [n_seq], NULL: slot = sequence index, which
 * needs n_slots >= n_seq -- this is also how carried tokens [n_seq,C] go in;  a slot outside [0, n_slots) is a zero token.  cu_seqlens ==
 * NULL is the dense form: total_T % n_seq == 0 and sequence s owns rows [s T, (s + 1) T), T = total_T / n_seq.  The int arrays live on
 * the device and are never read by the host; the slot is judged before an address is formed from it.
 * Two launches in stream order, "shrink" and "expand", on the 16x16x32 bf16 MFMAs, tiles of 16 rows, operands straight from global
 * memory.  Only the expand is an fp32 MFMA chain (one to four steps); in the shrink every MFMA sums its 32 products in fp32 from a zero
 * accumulator and the steps are added in fp64.  Every output element is its own dot product; the split of C over the waves of a shrink workgroup depends
 * on C alone and is summed in a fixed order; there are no atomics.  So a row's bits do not depend on the rows that share its tile or its
 * batch, nor on its place in a tile: a batch equals its sequences served one call at a time, bit for bit.  Rows >= total_T are neither
 * loaded nor stored and nothing is masked by a multiply: a NaN or Inf in a row of x reaches that row and the row behind it.
 * Aliasing: out / w may not overlap any input or the workspace.
 * wkv6_lowrank_workspace_bytes: rows * D_total * 2 rounded up to a multiple of 256, D_total = 5 D or Dd; 0 for a rows or a D_total the
 * calls refuse.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- total_T / rows, n_seq, D or Dd < 1, C or N not a multiple of 64 in
 * [64, 4096], cu_seqlens == NULL with total_T % n_seq != 0, with a front n_slots < 1 or slot == NULL with n_slots < n_seq;
 * (2) WKV6_EUNSUPPORTED -- D outside {32, 64}, Dd outside {64, 128}, total_T / rows > INT_MAX; (3) WKV6_ENULL -- a NULL tensor, weight or
 * workspace (cu_seqlens, front and slot may be NULL); (4) WKV6_EINVAL -- a tensor, weight or the workspace not 16-byte aligned, cu_seqlens
 * or slot not 4-byte aligned, out / w overlapping an input or the workspace; (5) WKV6_EWORKSPACE -- workspace_bytes below
 * wkv6_lowrank_workspace_bytes(total_T, 5 D) / (rows, Dd). */
size_t wkv6_lowrank_workspace_bytes(long rows, int D_total);
int wkv6_tmix_lerp_lowrank_bf16(long total_T, int n_seq, int C, int D, const int* cu_seqlens,
                                const void* x, const void* front, int n_slots, const int* slot,
                                const void* maa_x, const void* W1t, const void* W2t, const void* maa5,
                                void* out, void* workspace, size_t workspace_bytes, void* stream);
int wkv6_decay_lowrank_bf16(long rows, int C, int Dd, int N, const void* xw,
                            const void* D1t, const void* D2t, const void* time_decay,
                            void* w, void* workspace, size_t workspace_bytes, void* stream);
/* ---- device-side token sampling with a penalty slot pool (forward only; csrc/wkv6_sample.hip): the reference samples on the host, one
 * sequence at a time (src/model_run.py:1230-1304, src/logits_processors.py); here one launch turns the logits rows of a decode step into
 * token ids, every sequence with its own parameters, and the host reads nothing.  The sequence's decaying token-occurrence counts are a
 * fourth state under the slot number of its WKV state and shift tokens.
 *   logits [n_seq,ld] in the entry point's type, only columns < V count (ld % 8 == 0, ld >= V, 1 <= V <= 65536: a padded head);
 *   occ_pool fp32 [n_slots,ld], columns >= V never touched;  slot int32 [n_seq] or NULL (slot = sequence index, n_slots >= n_seq);
 *   slot_out int32 [n_seq] or NULL (in place);  params fp32 [n_seq,8] = temperature, top_p, top_k, alpha_presence, alpha_frequency,
 *   alpha_decay, repetition_penalty, 0 (top_k an integral value, 0 or >= V: off);  u fp32 [n_seq] in [0,1): the caller's uniform draw;
 *   tokens int32 [n_seq];  logprob fp32 [n_seq] or NULL.
 * Sequence s with o = occ_pool[slot[s]] (a slot outside the pool: o = 0), all values fp32, rows independent of each other:
 *   1. z[n] = logits[n] - (alpha_presence + o[n] * alpha_frequency) where o[n] > 0, else logits[n].  -inf logits are never drawn.
 *   2. the order is (z descending, n ascending); p = softmax(z).
 *   3. nucleus: c = the first position of the order whose inclusive cumulative p is >= top_p; kept = {n : z[n] >= z[order[c]]}, every
 *      tie at the cutoff included; top_p >= 1 keeps everything.
 *   4. top-k: with 0 < top_k < V only the first top_k of the order stay among the kept (the intersection of the two rules).
 *   5. repetition penalty (1: off): on kept n with o[n] > 0, z[n] = z[n] < 0 ? z[n] * pen : z[n] / pen.
 *   6. w[n] = exp((z[n] - max_kept z) / temperature) on the kept set, W = sum w.  temperature == 0 is greedy: 5. on every n, the token is
 *      argmax z with the lowest id among equals, logprob = 0.
 *   7. the draw runs in token-id order: the token is the smallest kept n with sum_{kept m <= n} w[m] > u W (none by rounding: the largest
 *      kept id); logprob = log(w[token] / W).
 *   8. occ_pool[(slot_out or slot)[s]] = o * alpha_decay, + 1 at the token (fp32 multiply, then add); a slot outside the pool stores nothing.
 * A row with a NaN or +inf among its V logits, no finite logit, or a non-finite or negative parameter is poisoned: token -1, logprob NaN,
 * its destination row untouched, its neighbours unaffected.  Pool entries are expected finite and >= 0.
 * Weights are held as integers floor(w * 2^46) and summed as integers, so every sum over a row is exact in any order: the same call gives
 * the same bits every time, and against exact arithmetic the CDF of 7. is off by at most V * 2^-46 of the largest weight.
 * Aliasing as rwkv6_forward_varlen_snap_*: any number of readers of a source slot; slot_out == slot (or NULL) is the defined in-place use;
 * two writers of one slot, or a slot one sequence writes and another reads, are out of contract but memory-safe.  Slot numbers and top_k
 * are judged on the device before an address is formed from them.  One launch, one workgroup per sequence, no workspace.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- n_seq, V or n_slots < 1, ld < V or ld % 8, slot == NULL with
 * n_slots < n_seq, logits or occ_pool not 16-byte aligned, any other pointer not 4-byte aligned, occ_pool overlapping logits;
 * (2) WKV6_EUNSUPPORTED -- V > 65536; (3) WKV6_ENULL -- a NULL logits, occ_pool, params, u or tokens. */
int rwkv6_sample_slots_bf16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot,
                            const int* slot_out, const float* params, const float* u, int* tokens, float* logprob, void* stream);
int rwkv6_sample_slots_fp16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot,
                            const int* slot_out, const float* params, const float* u, int* tokens, float* logprob, void* stream);
int rwkv6_sample_slots_fp32(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot,
                            const int* slot_out, const float* params, const float* u, int* tokens, float* logprob, void* stream);
/* ---- beam-search candidates on the rows of a packed decode step (forward only; csrc/wkv6_beam.hip): the reference runs beam search on the
 * host, one request at a time, with a log-softmax and a top-k over every beam's row and a clone of every state list per beam and token
 * (src/model_run.py:1317-1518); here one call gives, for every request (group) of a serving batch, the K best (parent row, token)
 * continuations by cumulative log-probability, and the host reads nothing.  The states fork through the slot pools
 * (rwkv6_forward_varlen_snap_*: several children read one parent slot and write slots of their own).
 *   logits [n_rows,ld] in the entry point's type, only columns < V count (ld % 8 == 0, ld >= V, 1 <= V <= 65536: a padded head);
 *   cum fp32 [n_rows]: the rows' running scores;  cu_rows int32 [n_groups + 1] on the device, never read by the host, every entry clamped
 *   into [0, n_rows]: group g owns rows cu_rows[g] .. cu_rows[g+1] - 1, of which at most the first 64 are considered;  K in [1, 64];
 *   occ_pool fp32 [n_slots,ld] (the sampler's occurrence counts), slot int32 [n_rows], penalty fp32 [n_groups]: all three NULL -- no
 *   penalty; with occ_pool and penalty, slot may be NULL (slot = row index, n_slots >= n_rows);
 *   parent, token int32 [n_groups,K], score fp32 [n_groups,K];  workspace: rwkv6_beam_candidates_workspace_bytes(n_rows, K) bytes (0 for
 *   an n_rows < 1 or a K outside [1, 64]), written and read by the call, nothing in it outlives the call.
 * Row r of group g with p = penalty[g] and o = occ_pool[slot[r]] (a slot outside the pool: o = 0), all values fp32, rows independent:
 *   1. a row with cum[r] == -inf is dead: its logits are not read (the dead rows of a fixed-shape search hold garbage) and it gives no
 *      candidate.
 *   2. a live row with a NaN or +inf among its V logits, no finite logit, a NaN or +inf cum[r], or a negative or non-finite p is poisoned
 *      and gives no candidate; its neighbours are unaffected.
 *   3. lp[n] = (z[n] - m) - L with m = max z and L = log sum exp(z - m).
 *   4. where p != 1 and o[n] > 0: lp[n] = lp[n] < 0 ? lp[n] * p : lp[n] / p (RepetitionPenaltyLogitsProcessor of
 *      src/logits_processors.py on log-probabilities; 0 / 0 counts as 0).
 *   5. s[n] = cum[r] + lp[n].  A -inf logit is never a candidate, nor is a score that comes out as -inf.
 *   6. the candidates (r, n) of the group are ordered by (s descending, r ascending, n ascending) and the first K go out: parent = r (the
 *      absolute row index), token = n, score = s; missing entries are parent = token = -1, score = -inf.
 * The denominator of 3. is held as the sum of the integers floor(exp(z - m) * 2^46), which is exact in any order, and L is the log of it
 * taken once per row in double and rounded to fp32: a row gives the same bits alone or in a batch, and the same call gives the same bits
 * every time.  No atomics on floats.  Slot numbers are judged on the device before an address is formed from them.  Two launches (one
 * workgroup per row, one wave per group).  Outputs and workspace may not overlap the inputs.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- n_rows, V or n_groups < 1, ld < V or ld % 8, K outside [1, 64], with an
 * occ_pool n_slots < 1 or slot == NULL with n_slots < n_rows, logits or occ_pool not 16-byte aligned, any other pointer (workspace
 * included) not 4-byte aligned, parent, token, score or the workspace overlapping an input; (2) WKV6_EUNSUPPORTED -- V > 65536;
 * (3) WKV6_ENULL -- a NULL logits, cum, cu_rows, parent, token, score or workspace, occ_pool without penalty or penalty without occ_pool,
 * slot without occ_pool; (4) WKV6_EWORKSPACE -- workspace_bytes below rwkv6_beam_candidates_workspace_bytes(n_rows, K). */
size_t rwkv6_beam_candidates_workspace_bytes(int n_rows, int K);
int rwkv6_beam_candidates_bf16(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream);
int rwkv6_beam_candidates_fp16(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream);
int rwkv6_beam_candidates_fp32(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream);
/* ---- sentence pooling on a packed batch (bf16, forward and backward; csrc/wkv6_pool.hip): RwkvForSequenceEmbedding.pooling
 * (src/model_ext.py:1708-1738) without the padded [B,T,C] tensor.
 *   x bf16 [total_T,C], C a multiple of 8;  cu_seqlens int32 [n_seq + 1] and actual_len int32 [n_seq] (or NULL) on the device, never read
 *   by the host;  out bf16 [n_seq,C];  backward: gout bf16 [n_seq,C], gx bf16 [total_T,C].
 * Sequence s, every cu_seqlens entry clamped into [0, total_T] first (cu = the clamped values):
 *     len_s = clamp(cu[s+1] - cu[s], 0, total_T - cu[s]);   a_s = clamp(actual_len[s], 0, len_s - 1), with actual_len NULL a_s = len_s - 1
 * (a_s is the row's position of the first emb_id token, as the reference's argmax gives it), x_t = x[cu[s] + t].  fp32 arithmetic, one
 * rounding to bf16 at the end:
 *     WKV6_POOL_WEIGHTEDMEAN   out[s] = ( sum_{t = 0 .. a_s} (t + 1) x_t ) / a_s / a_s        (the emb_id token included, as the reference)
 *     WKV6_POOL_AVG            out[s] = ( sum_{t < a_s} x_t ) / a_s
 *     WKV6_POOL_LASTTOKEN      out[s] = x[cu[s] + a_s]                                        (a copy: bit-exact)
 * a_s == 0 gives a NaN row for the two means (0 / 0, as the dense function does); an empty sequence (len_s == 0) gives a +0 row.  Rows of
 * x outside every sequence, and rows of a sequence past a_s (for WKV6_POOL_AVG: from a_s on), are never read: a NaN there reaches nothing
 * (the dense function multiplies it by a zero weight).
 * backward: gx[cu[s] + t] = bf16(weight_t gout[s]) with the forward's weights -- (t + 1) / a_s / a_s for t <= a_s, 1 / a_s for t < a_s,
 * the copy of gout[s] at t == a_s; the weighted mean's row of a sequence with a_s == 0 gets NaN.  EVERY row of gx is written (the caller
 * passes uninitialised memory): rows outside every sequence, rows of a sequence that the forward did not sum and every row of an empty
 * sequence get +0.  A row finds its sequence by the varlen rule (the last s with cu_seqlens[s] <= row).
 * Every index is clamped or compared before an address is formed from it: garbage in either int array touches no memory outside the
 * arguments.  One launch each, stream-ordered, capturable, no workspace, no atomics: the order of a sequence's token sum depends on the
 * token's index in the sequence alone (four interleaved partial sums, added in a fixed order), so the same call gives the same bits every
 * time and a sequence's row has the same bits alone or in a batch, wherever it lies in x.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- total_T or n_seq < 1, C < 8 or no multiple of 8, an unknown kind;
 * (2) WKV6_EUNSUPPORTED -- total_T > INT_MAX, n_seq * ceil(C / 512) > INT_MAX; (3) WKV6_ENULL -- a NULL cu_seqlens, x / gout or out / gx
 * (actual_len may be NULL); (4) WKV6_EINVAL -- x / gout or out / gx not 16-byte aligned, cu_seqlens or actual_len not 4-byte aligned. */
enum { WKV6_POOL_WEIGHTEDMEAN = 0, WKV6_POOL_LASTTOKEN = 1, WKV6_POOL_AVG = 2 };
int wkv6_pool_packed_forward(long total_T, int n_seq, int C, int kind, const int* cu_seqlens, const int* actual_len,
                             const void* x, void* out, void* stream);
int wkv6_pool_packed_backward(long total_T, int n_seq, int C, int kind, const int* cu_seqlens, const int* actual_len,
                              const void* gout, void* gx, void* stream);
/* ---- LM-head cross-entropy with L2Wrap on rows of logits (forward and backward; csrc/wkv6_ce.hip): what every language-model training step
 * of the reference does behind head(ln_out(x)) -- F.cross_entropy(logits.view(-1, V), targets.view(-1)), then L2Wrap.apply(loss, logits)
 * (src/model.py:937-974, 1244-1283) -- as one pass for the statistics and one for the gradient, no [n_rows, V] tensor besides the logits.
 *   logits [n_rows,ld] in the entry point's type, only columns < V count (ld >= V, ld % 8 == 0, V >= 1 with no upper limit: a padded head);
 *   targets int64 [n_rows] on the device, as torch holds them; -100 means the row is ignored;
 *   loss_row, lse, zmax fp32 [n_rows], imax int32 [n_rows];  ce_scale, l2_scale fp32 [n_rows] on the device;  glogits [n_rows,ld_g] in the
 *   type of the logits (ld_g >= V, ld_g % 8 == 0).
 * All arithmetic is fp32, rows are independent of each other.  Forward, row r with z = its V logits:
 *     zmax[r] = max_n z[n];   imax[r] = the lowest n that attains it (torch.max leaves ties open; this rule closes them);
 *     lse[r] = zmax + log(sum_n exp(z[n] - zmax));   loss_row[r] = lse[r] - z[target], +0 for an ignored row.
 * Backward, row r and column n < V, rounded once to the type of the logits:
 *     g[r,n] = ce_scale[r] * (exp(z[n] - lse[r]) - [n == target]) + l2_scale[r] * zmax[r] * [n == imax[r]]
 * An ignored row has no cross-entropy term, whatever ce_scale says.  A row that is ignored with l2_scale[r] == 0 is written as +0 without
 * its logits being read: a NaN there reaches nothing, by the rule of "rows outside every sequence" above (the fused forward does not read
 * such a row either and reports lse = zmax = +0, imax = 0 for it).  EVERY column < V of every row of g is written (the caller passes
 * uninitialised memory); columns >= V are never used and never written (the 16-byte load of a row's last chunk covers them, masked by
 * lane, never multiplied by zero).  glogits may be the logits buffer itself (in place, ld_g == ld): that is a defined use.
 * A target other than -100 outside [0, V): loss_row and the whole gradient row are NaN, no address is formed from the target, the row's
 * lse, zmax, imax are what its logits give, and its neighbours are unaffected.
 * Non-finite logits follow fp32 arithmetic: a -inf logit has p = 0.  A row with a NaN, a +inf or no finite logit has lse = NaN, hence a
 * NaN loss (+0 when it is ignored) and a NaN gradient row (unless it is ignored with l2_scale == 0), for that row alone; the zmax and
 * imax of a row with a NaN are taken over its other logits.
 * One launch, one workgroup per row, stream-ordered, capturable, no workspace, no atomics: the order of a row's sum depends on V and the
 * thread layout alone, so the same call gives the same bits every time and a row has the same bits alone or in a batch.
 * wkv6_ce_rows_forward_*: glogits == NULL is statistics only (ce_scale, l2_scale, ld_g are then not looked at); a non-NULL glogits writes
 * the gradient in the same launch -- the fused mode of a chunked head, which knows its scales before it has any loss --, bit-identical
 * to the forward followed by wkv6_ce_rows_backward_* on what it stored.
 * Refused before any launch, in this order: (1) WKV6_EINVAL -- n_rows or V < 1, ld < V or ld % 8, with a gradient ld_g < V or ld_g % 8;
 * (2) WKV6_EUNSUPPORTED -- n_rows > INT_MAX; (3) WKV6_ENULL -- a NULL logits, targets, lse, zmax, imax or (forward) loss_row, with a
 * gradient a NULL ce_scale or l2_scale, in the backward a NULL glogits; (4) WKV6_EINVAL -- logits or glogits not 16-byte aligned, targets
 * not 8-byte aligned, any other array that the call looks at not 4-byte aligned, glogits overlapping logits in any way but the in-place
 * one. */
int wkv6_ce_rows_forward_bf16(long n_rows, int V, long ld, const void* logits, const long long* targets, float* loss_row, float* lse,
                              float* zmax, int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g, void* stream);
int wkv6_ce_rows_forward_fp16(long n_rows, int V, long ld, const void* logits, const long long* targets, float* loss_row, float* lse,
                              float* zmax, int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g, void* stream);
int wkv6_ce_rows_forward_fp32(long n_rows, int V, long ld, const void* logits, const long long* targets, float* loss_row, float* lse,
                              float* zmax, int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g, void* stream);
int wkv6_ce_rows_backward_bf16(long n_rows, int V, long ld, const void* logits, const long long* targets, const float* lse,
                               const float* zmax, const int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g,
                               void* stream);
int wkv6_ce_rows_backward_fp16(long n_rows, int V, long ld, const void* logits, const long long* targets, const float* lse,
                               const float* zmax, const int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g,
                               void* stream);
int wkv6_ce_rows_backward_fp32(long n_rows, int V, long ld, const void* logits, const long long* targets, const float* lse,
                               const float* zmax, const int* imax, const float* ce_scale, const float* l2_scale, void* glogits, long ld_g,
                               void* stream);
/* gn_gate (src/model.py:462-468): out = GroupNorm_H(y; gamma, beta, eps) * g on rows of C = 64 H channels (nn.GroupNorm(H, C)
 * applied to [rows, C]); stats fp32 [rows,H,2] (mean, rstd) is written for the backward (may be NULL in inference).
 * backward: dy, dg [rows,C]; dgamma_part, dbeta_part fp32 [nparts,C] partial sums. */
int wkv6_gn_gate_forward(long rows, int C, int H, const void* y, const void* g, const void* gamma, const void* beta,
                         float eps, void* out, float* stats, void* stream);
int wkv6_gn_gate_backward(long rows, int C, int H, const void* y, const void* g, const void* gamma, const void* beta,
                          const float* stats, const void* dout, void* dy, void* dg, float* dgamma_part, float* dbeta_part,
                          int nparts, void* stream);

/* Elementwise neighbours of the channel-mix FFN's GEMMs (src/model.py:636-644), bf16, n elements (a multiple of 8), one pass each:
 * sqrelu: out = relu(x)^2, dx = 2 relu(x) dout;  sigmul: out = sigmoid(r) * kv, dr = dout kv s (1 - s), dkv = dout s.
 * (The FFN's token shift and its two lerps are wkv6_ddlerp_* with NS = 2, m = NULL.) */
int wkv6_sqrelu_forward(long n, const void* x, void* out, void* stream);
int wkv6_sqrelu_backward(long n, const void* x, const void* dout, void* dx, void* stream);
int wkv6_sigmul_forward(long n, const void* r, const void* kv, void* out, void* stream);
int wkv6_sigmul_backward(long n, const void* r, const void* kv, const void* dout, void* dr, void* dkv, void* stream);

/* Device self-test: the cross-lane primitives, then the chunked MFMA kernels against the exact scan kernels on two fixed
 * pseudo-random problems -- one small enough that two workgroups serve a (batch, head) pair, one with one workgroup per pair, so
 * that both backward kernels run -- (forward and backward, all outputs within 2 bf16 ulps of the tensor scale, 4 for gw).
 * Returns 0 when it passes, WKV6_ESELFTEST (or the number of failed primitive checks) otherwise. */
int wkv6_selftest(void* stream);
/* Debug entry: the two forms of the chunked kernels' split of fp32 into bf16 hi + lo (csrc/wkv6_chunk.h: the residual lo = x - float(hi)
 * by v_dot2c per lane, or by one MFMA per wave) on `rows` rows of 64 lanes x 4 floats at `x`.  out: 4 * rows * 256 bf16 bit patterns,
 * [hi, lo of the v_dot2c form | hi, lo of the MFMA form][rows][64][4].  An Inf in one hi makes NaN of the MFMA form's residuals in the
 * same lane % 16 of its row (all four lane groups, all four slots); nothing else crosses lanes. */
int wkv6_debug_split(long rows, const void* x, void* out, void* stream);
/* Measurement aids (bench.py; no effect on results).
 * wkv6_set_clock_ring: while `buf` (device memory, 2 * n_launches * n_slots * 4 uint64) is set, wave 0 of the first n_slots workgroups of
 * the n-th chunked forward launch since the call writes {s_memtime, s_memrealtime} at its start and its end into
 * buf[((n % n_launches) * n_slots + slot) * 4 .. + 3], and of the n-th chunked backward launch into the second half of buf likewise:
 * the in-kernel shader clock of a launch is d(s_memtime) / d(s_memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS give-back item 6), its
 * duration max(end s_memrealtime) - min(start s_memrealtime) over the slots.  buf = NULL (the default) switches it off: the kernels
 * then execute one scalar branch for it and no stamp.  Process-wide; the caller keeps `buf` alive until it has switched the probe off.
 * wkv6_clock_ring_counts: chunked forward / backward launches since the ring was set.
 * wkv6_pass_marker: launches an empty kernel named wkv6::pass_marker_kernel on `stream`: a phase boundary in a profiler's
 * dispatch list.
 * wkv6_set_dispatch: overrides one of the library's launch-shape choices, process-wide (tests and A/Bs reach every mode with it).
 * WKV6_DISPATCH_SPLIT: != 0 forces two workgroups per (batch, head), 0 forces one.
 * WKV6_DISPATCH_BI_FUSED: 0 runs the two halves of wkv6_bi as two launches, any other value leaves the choice to the library.
 * WKV6_DISPATCH_TSPLIT: 0 or 1 turns the two-level forward over T off, n forces n segments where T % (64 n) == 0 (off otherwise).
 * WKV6_DISPATCH_BI_SLOTS: n >= 1 makes both persistent wkv6_bi launches use min(n, B*H) workgroup slots instead of min(B*H, CUs)
 * (so that a test pins the rows each slot walks on any CU count); WKV6_DISPATCH_SPLIT and WKV6_DISPATCH_BI_FUSED = 0 take precedence. */
void wkv6_set_clock_ring(void* buf, int n_slots, int n_launches);
void wkv6_clock_ring_counts(long* fwd, long* bwd);
int wkv6_pass_marker(void* stream);
enum { WKV6_DISPATCH_SPLIT = 0, WKV6_DISPATCH_BI_FUSED = 1, WKV6_DISPATCH_TSPLIT = 2, WKV6_DISPATCH_BI_SLOTS = 3 };
/* value -1: the library's own choice (default).  Returns the previous value, or WKV6_EINVAL for an unknown selector. */
int wkv6_set_dispatch(int what, int value);
/* "major.minor" of the library. */
const char* wkv6_amd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WKV6_AMD_H */
