// The chunked kernels over few, long sequences (inference prefill: B*H << CUs): a two-level scan over T, forward and backward.
#include "wkv6_host.h"

using namespace wkv6;

namespace {            // (the kernels keep their names outside namespace wkv6: profile filters tell them from the operator kernels by it)

// ---- forward: the sequence is cut into S segments that run as S times as many workgroups:
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
        const int e = threadIdx.x + 256 * m;                            // state layout [j][i]: i = key channel
        float cur = 0.f;
        if (s0) {
            const long o = (long)b * s0_bstride + (long)h * HEAD * HEAD + e;
            cur = s_f32 ? reinterpret_cast<const float*>(s0)[o] : bf_lo((uint32_t)reinterpret_cast<const bf16_t*>(s0)[o]);
        }
        for (int seg = 0; seg < S; ++seg) {
            const long bp = ((long)b * S + seg) * H + h;
            Sin[bp * HEAD * HEAD + e] = cur;
            cur = chain_step(cur, A, dsum, bp, e);
        }
        if (s_out) store_partial(s_out, s_f32, ((long)b * H + h) * HEAD * HEAD + e, cur);
    }
}

// ---- backward: the S segments of a sequence run as S workgroups.  What a segment needs from beyond its end is
// closed-form:
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
        for (int m = 0; m < HEAD * HEAD / 256; ++m) cur[m] = chain_step(cur[m], A, dsum, bp, tid + 256 * m);
    }
    if (gs)
        for (int m = 0; m < HEAD * HEAD / 256; ++m) store_partial(gs, gs_f32, ((long)b * H + h) * HEAD * HEAD + tid + 256 * m, cur[m]);
}
__global__ void tsplit_gu_kernel(const float* __restrict__ part, void* gu, int gu_f32, int S, int C)
{
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int seg = 0; seg < S; ++seg) s += part[((long)b * S + seg) * C + c];
        store_partial(gu, gu_f32, (long)b * C + c, s);
    }
}

// segments of the two-level scan over T (1: one pass)
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

// the S segments of every row as rows of their own: row b of the view is segment b % S of row b / S, from a zero state -- or from its
// fp32 entry state in Sin, its checkpoints then landing in the whole sequences' slots
ScanArgs segment_view(const ScanArgs& a, int S, const float* Sin = nullptr)
{
    ScanArgs p = a;
    p.B = a.B * S; p.T = a.T / S;
    p.s0 = Sin; p.s0_bstride = Sin ? (long)a.H * HEAD * HEAD : 0;
    if (Sin) { p.state_f32 = 1; p.ckpt_segs = S; }
    return p;
}
// ... as a state-only pass from a zero state: the segment's own contribution to the state (A) and its decay sums
hipError_t segment_summaries(ScanArgs p, float* A, float* dsum, hipStream_t st)
{
    p.s_out = A; p.state_f32 = 1; p.y = nullptr; p.dsum = dsum; p.ckpt = nullptr;
    return launch_chunk_state_pass(p, st);
}

// segment entry states of a two-level forward: state pass per segment from zero (A, dsum), chained by tsplit_combine_kernel
hipError_t tsplit_entry_states(const ScanArgs& a, int S, float* A, float* Sin, float* dsum, hipStream_t st)
{
    if (hipError_t e = segment_summaries(segment_view(a, S), A, dsum, st)) return e;
    return launch<tsplit_combine_kernel>(dim3(a.B * a.H), dim3(256), 0, st, a.s0, a.state_f32, a.s0_bstride, A, dsum, Sin, a.s_out, a.H, S);
}

}  // namespace

namespace wkv6 {

hipError_t chunk_forward(const ScanArgs& a, hipStream_t st)
{
    const int S = tsplit_segments(a);
    if (S <= 1) return launch_chunk_fwd(a, st);
    const size_t nstate = (size_t)a.B * S * a.H * HEAD * HEAD;                 // floats
    const size_t ndsum = (size_t)a.B * S * a.H * 4 * HEAD;
    StreamScratch scratch;
    float* const buf = reinterpret_cast<float*>(scratch.get((2 * nstate + ndsum) * sizeof(float), st));
    if (!buf) return hipErrorOutOfMemory;
    float* const A = buf, * const Sin = buf + nstate, * const dsum = buf + 2 * nstate;
    if (hipError_t e = tsplit_entry_states(a, S, A, Sin, dsum, st)) return e;
    ScanArgs p = segment_view(a, S, Sin);          // (checkpoints: the training forward's)
    p.s_out = nullptr;
    return launch_chunk_fwd(p, st);
}

hipError_t chunk_backward(const ScanArgs& a, hipStream_t st)
{
    const int S = tsplit_segments(a);
    if (S <= 1) return launch_chunk_bwd(a, st);
    const size_t nstate = (size_t)a.B * S * a.H * HEAD * HEAD, ndsum = (size_t)a.B * S * a.H * 4 * HEAD, nrow = (size_t)a.B * S * a.C;
    StreamScratch scratch;
    float* const buf = reinterpret_cast<float*>(scratch.get((2 * nstate + ndsum + 2 * nrow) * sizeof(float), st));
    if (!buf) return hipErrorOutOfMemory;
    float* const A = buf, * const Gin = buf + nstate, * const dsum = buf + 2 * nstate, * const phi = dsum + ndsum, * const gup = phi + nrow;
    if (!a.ckpt_valid) {                               // self-contained: the forward's states first (two-level, like chunk_forward)
        ScanArgs f = a;
        f.y = nullptr; f.s_out = nullptr; f.gy = nullptr;
        if (hipError_t e = tsplit_entry_states(f, S, A, Gin, dsum, st)) return e;
        if (hipError_t e = launch_chunk_state_pass(segment_view(f, S, Gin), st)) return e;
    }
    {   // the segments' own adjoint contributions: state-only pass over the reversed segments with k := r, v := gy
        ScanArgs p = segment_view(a, S);
        p.k = a.r; p.v = a.gy; p.reverse = 1;
        if (hipError_t e = segment_summaries(p, A, dsum, st)) return e;
    }
    if (hipError_t e = launch<tsplit_combine_rev_kernel>(dim3(a.B * a.H), dim3(256), 0, st, A, dsum, a.ckpt, Gin, phi, a.gs, a.part_f32, a.H,
                                                         S, (long)(a.T / S / 64), a.C))
        return e;
    ScanArgs p = segment_view(a, S);
    p.g_in = Gin; p.rc_in = phi; p.ckpt_segs = S; p.ckpt_valid = 1; p.split = 0;
    p.gu = a.gu ? gup : nullptr; p.gs = nullptr; p.part_f32 = 1;
    if (hipError_t e = launch_chunk_bwd12k(p, st)) return e;
    if (a.gu) return launch<tsplit_gu_kernel>(dim3(a.B), dim3(256), 0, st, gup, a.gu, a.part_f32, S, a.C);
    return hipSuccess;
}

}  // namespace wkv6
