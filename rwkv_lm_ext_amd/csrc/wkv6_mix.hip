// Memory-bound elementwise kernels either side of the WKV6 operator in the RWKV-6 time-mix block,
// hand-written for gfx950: one pass over HBM each instead of the 5-12 eager PyTorch kernels of the reference.
//
//   ddlerp  (src/model.py:435-448):  xx = shift(x) - x;   out_s = x + xx (.) (maa_s + m_s),  s = 0..NS-1
//           NS = 1, m = null: the input of the first low-rank GEMM (x + xx (.) time_maa_x);
//           NS = 5: xw, xk, xv, xr, xg from the five low-rank corrections m_s (the bmm output, [5,B,T,C] contiguous).
//           NS = 2, m = null: the channel-mix FFN's two inputs x + xx (.) time_maa_k, x + xx (.) time_maa_r (src/model.py:636-638).
//   sqrelu  (src/model.py:640-641):  out = relu(x)^2 on the FFN's key projection;   backward dx = 2 relu(x) dout.
//   sigmul  (src/model.py:643-644):  out = sigmoid(r) (.) kv, the receptance gate on the FFN's value projection;
//           backward dr = dout kv s (1 - s), dkv = dout s.
//   gn_gate (src/model.py:462-468):  out = GroupNorm_H(y) (.) g  -- per-head normalisation of the WKV output over its 64
//           channels (nn.GroupNorm(H, C, eps) on [B*T, C]) fused with the gate multiply that feeds the output GEMM.
//   ddlerp_slots / shift_keep (forward only, packed batches): the token-shift state of a serving loop as a slot pool [n_slots,C] -- the
//           lerp with the token in front of a sequence fetched from the pool by slot number, and the one launch that stores what the batch
//           leaves (last tokens, snapshot tokens), writing only the rows that change (include/wkv6_amd.h).
// Forward and backward of both; parameter gradients (time_maa_*, ln_x.weight/bias) leave as per-workgroup fp32 partial rows
// that the caller sums (deterministic, no atomics).
//
// Layout: rows of C bf16 channels; a thread owns 4 consecutive channels (8-byte accesses, a 64-channel head = 16 lanes =
// one DPP row, so the GroupNorm statistics are DPP row reductions); one workgroup of C/4 threads per row.
#include <type_traits>
#include "wkv6_host.h"                 // launch<>, to_rc

namespace wkv6 {
namespace {


struct LerpArgs {
    int B, T, C, NS;
    const bf16_t* x;          // [B,T,C]
    const bf16_t* shifted0;   // [B,C] token in front of every row (infctx), or null (zero)
    const int* rev_n;         // [B] or null: the shift runs over the stream "first rev_n[b] tokens reversed, rest in place"
    const bf16_t* m;          // [NS,B,T,C] or null
    const bf16_t* maa;        // [NS,C]
    bf16_t* out;              // [NS,B,T,C]
    // backward
    const bf16_t* dout;       // [NS,B,T,C]
    bf16_t* dx;               // [B,T,C]
    bf16_t* dm;               // [NS,B,T,C] or null
    float* dmaa_part;         // [nparts,NS,C]
    int nparts;
    // packed variable-length batch (the VARLEN instantiations; B = 1, T = total_T): token boundaries of the n_seq sequences; shifted0 is
    // then [n_seq,C], the token in front of each sequence's first one
    const int* cu;            // [n_seq + 1]
    int n_seq;
};
// ddlerp_fwd_slots_kernel (forward, packed): shifted0 is a pool [n_slots,C] and the token in front of sequence s its row slot[s]
struct SlotLerpArgs : LerpArgs {
    const int* slot;          // [n_seq] or null (slot = sequence index)
    int n_slots;
};

// (packed batches: the sequence that holds a row is seq_of_row of wkv6_common.h)
__device__ __forceinline__ void ld4(const bf16_t* p, float (&o)[4]) { io4<bf16_t>::load(p, o); }

// Token shift over a partially reversed stream, in the ORIGINAL token order: the bidirectional encoder
// reverses the first n tokens of a row (reverse_x_idx, src/model_ext.py:410-417), runs the time-mix on that stream and
// un-reverses the result.  Stream position of token t: n-1-t for t < n, t otherwise.  prev_tok = the token one stream
// position earlier (-1: the row's leading pad), next_tok = the token one stream position later (-1: none); n = 0: plain.
__device__ __forceinline__ int prev_tok(int t, int n)
{
    if (n <= 0 || t > n) return t - 1;
    if (t < n - 1) return t + 1;
    return t == n ? 0 : -1;                              // t == n: behind the reversed span sits token 0; t == n-1: stream start
}
__device__ __forceinline__ int next_tok(int t, int n, int T)
{
    if (n <= 0 || t >= n) return t + 1 < T ? t + 1 : -1;
    if (t >= 1) return t - 1;
    return n < T ? n : -1;                               // token 0 closes the reversed span
}

// The one lerp of the forward kernels: the NS blends of x, the row's channels at element `at` of a plane, with xp, the token in front of
// it; planes `plane` elements apart.  All a forward kernel decides is where xp comes from.  (Here and in the backward helpers the row's
// offset joins the base pointer before the plane's: one vector address per tensor and a scalar step per plane, as the kernels had it.)
template <int NS, bool HAS_M>
__device__ __forceinline__ void lerp_store(const LerpArgs& a, long plane, long at, int c, const float (&x)[4], const float (&xp)[4])
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float maa[4], m[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        ld4(a.maa + c + (long)s * a.C, maa);
        if constexpr (HAS_M) ld4(a.m + at + s * plane, m);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = fmaf(xp[q] - x[q], maa[q] + m[q], x[q]);
        io4<bf16_t>::store(a.out + at + s * plane, o);
    }
}

template <int NS, bool HAS_M, bool VARLEN = false>
__global__ void ddlerp_fwd_kernel(const LerpArgs a)
{
    const long row = blockIdx.x;                         // b*T + t
    const int t = (int)(row % a.T), b = (int)(row / a.T);
    const int c = 4 * threadIdx.x;
    float x[4], xp[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(a.x + row * a.C + c, x);
    if constexpr (VARLEN) {
        const int sq = seq_of_row(a.cu, a.n_seq, row);
        const bool first = sq >= 0 && (long)a.cu[sq] == row;
        if (!first) { if (row > 0) ld4(a.x + (row - 1) * a.C + c, xp); }
        else if (a.shifted0) ld4(a.shifted0 + (long)sq * a.C + c, xp);
    } else {
        const int nrev = a.rev_n ? min(max(a.rev_n[b], 0), a.T) : 0;
        const int tp = prev_tok(t, nrev);
        if (tp >= 0) ld4(a.x + ((long)b * a.T + tp) * a.C + c, xp);
        else if (a.shifted0) ld4(a.shifted0 + (long)b * a.C + c, xp);
    }
    lerp_store<NS, HAS_M>(a, (long)a.B * a.T * a.C, row * a.C + c, c, x, xp);
}

// The VARLEN forward with the token in front of a sequence taken from a slot pool (wkv6_ddlerp_slots_forward): the same loads of x, the same
// lerp.  A kernel of its own rather than one more flag of ddlerp_fwd_kernel: the kernels of the training path keep their names, their
// argument block and their instruction streams.
template <int NS, bool HAS_M>
__global__ void ddlerp_fwd_slots_kernel(const SlotLerpArgs a)
{
    const long row = blockIdx.x;
    const int c = 4 * threadIdx.x;
    float x[4], xp[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(a.x + row * a.C + c, x);
    const int sq = seq_of_row(a.cu, a.n_seq, row);
    const bool first = sq >= 0 && (long)a.cu[sq] == row;
    if (!first) { if (row > 0) ld4(a.x + (row - 1) * a.C + c, xp); }
    else {                                               // the slot is judged before an address is formed: outside the pool = zero token
        const int sl = a.slot ? a.slot[sq] : sq;
        if (sl >= 0 && sl < a.n_slots) ld4(a.shifted0 + (long)sl * a.C + c, xp);
    }
    lerp_store<NS, HAS_M>(a, (long)a.T * a.C, row * a.C + c, c, x, xp);
}

// Backward: dx_t = sum_s dout_{s,t} (1 - c_{s,t}) + sum_s dout_{s,t+1} c_{s,t+1}  (c = maa + m; the second term is the adjoint
// of the token shift), dm_{s,t} = dout_{s,t} xx_t, dmaa_s = sum_rows dout_s xx.  Plain stream: workgroup p walks the contiguous
// rows [p per, (p + 1) per), per = ceil(rows / nparts), backwards; reversed-span streams: workgroup p handles rows p, p + nparts, ...
// (VARLEN: the plain walk, with "first token of a sequence" and "nothing behind this token" taken from cu_seqlens: one bisection per
// workgroup for the sequence of its last row and one for the row behind it, then the boundaries are walked downwards with the rows)

// what every backward kernel opens and closes with: maa in registers and a zero dmaa sum; the workgroup's partial row of dmaa_part
template <int NS> __device__ __forceinline__ void bwd_open(const LerpArgs& a, int c, float (&maa)[NS][4], float (&acc)[NS][4])
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        ld4(a.maa + (long)s * a.C + c, maa[s]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[s][q] = 0.f;
    }
}
template <int NS> __device__ __forceinline__ void bwd_close(const LerpArgs& a, int c, const float (&acc)[NS][4])
{
#pragma unroll
    for (int s = 0; s < NS; ++s)
        *reinterpret_cast<float4*>(a.dmaa_part + ((long)blockIdx.x * NS + s) * a.C + c) =
            make_float4(acc[s][0], acc[s][1], acc[s][2], acc[s][3]);
}
// The hand-over: what row rn, the one behind row t in the stream, gives row t -- the part of its blends that came from x_t,
// sum_s dout[s][rn] (maa_s + m_s[rn]) -- added to g plane by plane, s = 0 first.  Every path sums it in this order, on top of zeros, and
// adds row t's own terms afterwards: the plain walk, the dense reversed branch and the packed kernels agree bit for bit.
template <int NS, bool HAS_M>
__device__ __forceinline__ void hand_over(const LerpArgs& a, int c, long rn, const float (&maa)[NS][4], float (&g)[4])
{
    const long plane = (long)a.B * a.T * a.C, at = rn * a.C + c;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float dn[4], mn[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(a.dout + at + s * plane, dn);
        if constexpr (HAS_M) ld4(a.m + at + s * plane, mn);
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = fmaf(dn[q], maa[s][q] + mn[q], g[q]);
    }
}
// Backward of a row whose stream neighbours are not the adjacent rows: xp_src = the [C] row of the token in front (null: zero), rown = the
// row one stream position later (-1: none), fetched by a hand-over of its own (54 bytes per token-channel at NS = 5, where the plain
// walk carries it: 34).  All a kernel decides is the two neighbours.
template <int NS, bool HAS_M>
__device__ __forceinline__ void bwd_far_row(const LerpArgs& a, int c, long row, const bf16_t* xp_src, long rown,
                                            const float (&maa)[NS][4], float (&acc)[NS][4])
{
    const long plane = (long)a.B * a.T * a.C, at = row * a.C + c;
    float x[4], xp[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(a.x + at, x);
    if (xp_src) ld4(xp_src + c, xp);
    if (rown >= 0) hand_over<NS, HAS_M>(a, c, rown, maa, g);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float d[4], m[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(a.dout + at + s * plane, d);
        if constexpr (HAS_M) ld4(a.m + at + s * plane, m);
        float dm[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            g[q] = fmaf(d[q], 1.f - (maa[s][q] + m[q]), g[q]);
            dm[q] = d[q] * (xp[q] - x[q]);
            acc[s][q] += dm[q];
        }
        if constexpr (HAS_M) io4<bf16_t>::store(a.dm + at + s * plane, dm);
    }
    io4<bf16_t>::store(a.dx + at, g);
}

template <int NS, bool HAS_M, bool VARLEN = false>
__global__ void ddlerp_bwd_kernel(const LerpArgs a)
{
    const int c = 4 * threadIdx.x;
    const long plane = (long)a.B * a.T * a.C, rows = (long)a.B * a.T;
    float maa[NS][4], acc[NS][4];
    bwd_open<NS>(a, c, maa, acc);
    if (VARLEN || !a.rev_n) {
        // Plain stream: a workgroup walks a contiguous run of rows backwards, so what token t+1 hands to token t is four floats
        // carried in registers instead of a second read of dout and m (54 -> 34 bytes per token-channel at NS = 5).
        const long per = (rows + gridDim.x - 1) / gridDim.x, r0 = (long)blockIdx.x * per, r1 = min(rows, r0 + per);
        float carry[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] int sq = -1;                             // VARLEN: sequence of the row at hand, its first row,
        [[maybe_unused]] long sq_row0 = -1;
        [[maybe_unused]] bool next_opens = true;                  //         and whether the row behind it opens a sequence
        if constexpr (VARLEN) {
            if (r1 > r0) {
                sq = seq_of_row(a.cu, a.n_seq, r1 - 1);
                sq_row0 = sq >= 0 ? (long)a.cu[sq] : -1;
                if (r1 < rows) {
                    const int sn = seq_of_row(a.cu, a.n_seq, r1);
                    next_opens = sn >= 0 && (long)a.cu[sn] == r1;
                }
            }
        }
        if (r1 > r0 && r1 < rows && (VARLEN ? !next_opens : r1 % a.T != 0))            // the run ends inside a sequence: fetch the next row's hand-over once
            hand_over<NS, HAS_M>(a, c, r1, maa, carry);
        for (long row = r1 - 1; row >= r0; --row) {
            const int t = (int)(row % a.T), b = (int)(row / a.T);
            float x[4], xp[4] = {0.f, 0.f, 0.f, 0.f}, g[4], own[4] = {0.f, 0.f, 0.f, 0.f};
            ld4(a.x + row * a.C + c, x);
            bool last;
            if constexpr (VARLEN) {
                while (sq >= 0 && row < sq_row0) { --sq; sq_row0 = sq >= 0 ? (long)a.cu[sq] : -1; }
                const bool first = sq >= 0 && row == sq_row0;
                if (!first) { if (row > 0) ld4(a.x + (row - 1) * a.C + c, xp); }
                else if (a.shifted0) ld4(a.shifted0 + (long)sq * a.C + c, xp);
                last = next_opens;
                next_opens = first;
            } else {
                if (t > 0) ld4(a.x + (row - 1) * a.C + c, xp);
                else if (a.shifted0) ld4(a.shifted0 + (long)b * a.C + c, xp);
                last = t == a.T - 1;                              // nothing behind the last token of a sequence
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = last ? 0.f : carry[q];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float d[4], m[4] = {0.f, 0.f, 0.f, 0.f}, dm[4];
                ld4(a.dout + s * plane + row * a.C + c, d);
                if constexpr (HAS_M) ld4(a.m + s * plane + row * a.C + c, m);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float wgt = maa[s][q] + m[q];
                    g[q] = fmaf(d[q], 1.f - wgt, g[q]);
                    own[q] = fmaf(d[q], wgt, own[q]);
                    dm[q] = d[q] * (xp[q] - x[q]);
                    acc[s][q] += dm[q];
                }
                if constexpr (HAS_M) io4<bf16_t>::store(a.dm + s * plane + row * a.C + c, dm);
            }
            io4<bf16_t>::store(a.dx + row * a.C + c, g);
#pragma unroll
            for (int q = 0; q < 4; ++q) carry[q] = own[q];
        }
    } else
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {       // reversed-span streams: the neighbours are not adjacent rows
        const int t = (int)(row % a.T), b = (int)(row / a.T);
        const int nrev = min(max(a.rev_n[b], 0), a.T);
        const int tp = prev_tok(t, nrev), tn = next_tok(t, nrev, a.T);
        bwd_far_row<NS, HAS_M>(a, c, row, tp >= 0 ? a.x + ((long)b * a.T + tp) * a.C : a.shifted0 ? a.shifted0 + (long)b * a.C : nullptr,
                               tn >= 0 ? (long)b * a.T + tn : -1, maa, acc);
    }
    bwd_close<NS>(a, c, acc);
}

// Packed batch under a reversal map (a.cu and a.rev_n, [n_seq]): the stream of sequence s is "its first rev_n[s] tokens reversed, the rest in
// place" (rev_n clamped to the sequence's length), and the token in front of the stream's first token is shifted0[s] (null: zero), never a
// token of another sequence.  A row's sequence comes from the bisection of the plain packed kernels; the neighbours are prev_tok / next_tok
// within the sequence, so the backward walks rows p, p + nparts, ... as the dense reversed-stream branch does, with the same summation
// order.  Rows in front of cu[0] belong to no sequence and take the plain neighbour; rows from cu[n_seq] on continue the last sequence
// in place, as in the plain packed kernels.
struct SeqSpan {
    long start;               // first row of the sequence (clamped to [0, rows])
    int slen, nrev;           // rows the stream walks; reversed span
    int sq;                   // sequence, -1: none
};
__device__ __forceinline__ SeqSpan seq_span(const LerpArgs& a, long row)
{
    const long rows = (long)a.B * a.T;
    SeqSpan p;
    p.sq = seq_of_row(a.cu, a.n_seq, row);
    if (p.sq < 0) { p.start = 0; p.slen = (int)min((long)a.cu[0], rows); p.nrev = 0; return p; }      // (row < cu[0])
    p.start = max((long)a.cu[p.sq], 0L);
    const long end = min(max((long)a.cu[p.sq + 1], p.start), rows);                  // (row >= cu[sq], so start <= row < rows)
    p.slen = (int)((p.sq + 1 < a.n_seq ? end : rows) - p.start);
    p.nrev = (int)min((long)max(a.rev_n[p.sq], 0), end - p.start);
    return p;
}
// the token in front of a token of the span, tp = its prev_tok within the span: row start + tp, or (-1) the sequence's carried token
__device__ __forceinline__ const bf16_t* span_xp_src(const LerpArgs& a, const SeqSpan& sp, int tp)
{
    if (tp >= 0) return a.x + (sp.start + tp) * a.C;
    return a.shifted0 && sp.sq >= 0 ? a.shifted0 + (long)sp.sq * a.C : nullptr;
}

template <int NS, bool HAS_M>
__global__ void ddlerp_fwd_varlen_rev_kernel(const LerpArgs a)
{
    const long row = blockIdx.x;
    const int c = 4 * threadIdx.x;
    float x[4], xp[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(a.x + row * a.C + c, x);
    const SeqSpan sp = seq_span(a, row);
    const int tp = prev_tok((int)(row - sp.start), sp.nrev);
    if (tp >= 0) ld4(a.x + (sp.start + tp) * a.C + c, xp);
    else if (a.shifted0 && sp.sq >= 0) ld4(a.shifted0 + (long)sp.sq * a.C + c, xp);
    lerp_store<NS, HAS_M>(a, (long)a.B * a.T * a.C, row * a.C + c, c, x, xp);
}

template <int NS, bool HAS_M>
__global__ void ddlerp_bwd_varlen_rev_kernel(const LerpArgs a)
{
    const int c = 4 * threadIdx.x;
    const long rows = (long)a.B * a.T;
    float maa[NS][4], acc[NS][4];
    bwd_open<NS>(a, c, maa, acc);
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const SeqSpan sp = seq_span(a, row);
        const int t = (int)(row - sp.start);
        const int tn = next_tok(t, sp.nrev, sp.slen);
        bwd_far_row<NS, HAS_M>(a, c, row, span_xp_src(a, sp, prev_tok(t, sp.nrev)), tn >= 0 ? sp.start + tn : -1, maa, acc);
    }
    bwd_close<NS>(a, c, acc);
}

struct GnArgs {
    long rows;
    int C, H;
    float eps;
    const bf16_t *y, *g, *gamma, *beta;
    bf16_t* out;
    float* stats;             // [rows, H, 2] mean, rstd (saved by the forward for the backward)
    const bf16_t* dout;
    bf16_t *dy, *dg;
    float *dgamma_part, *dbeta_part;   // [nparts, C]
    int nparts;
};

__global__ void gn_gate_fwd_kernel(const GnArgs a)
{
    const long row = blockIdx.x;
    const int c = 4 * threadIdx.x, head = c >> 6;
    float y[4], g[4], ga[4], be[4], o[4];
    ld4(a.y + row * a.C + c, y);
    ld4(a.g + row * a.C + c, g);
    ld4(a.gamma + c, ga);
    ld4(a.beta + c, be);
    const float mean = row_sum16(y[0] + y[1] + y[2] + y[3]) * (1.f / 64.f);
    float var = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) var = fmaf(y[q] - mean, y[q] - mean, var);
    var = row_sum16(var) * (1.f / 64.f);                  // biased variance, as nn.GroupNorm
    const float rstd = rsqrtf(var + a.eps);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = fmaf((y[q] - mean) * rstd, ga[q], be[q]) * g[q];
    io4<bf16_t>::store(a.out + row * a.C + c, o);
    if (a.stats && (threadIdx.x & 15) == 0) {
        a.stats[(row * a.H + head) * 2] = mean;
        a.stats[(row * a.H + head) * 2 + 1] = rstd;
    }
}

// no = xhat gamma + beta, out = no g:  dg = dout no;  dno = dout g;  dxhat = dno gamma;
// dy = rstd (dxhat - mean_64(dxhat) - xhat mean_64(dxhat xhat));  dgamma += dno xhat;  dbeta += dno.
__global__ void gn_gate_bwd_kernel(const GnArgs a)
{
    const int c = 4 * threadIdx.x, head = c >> 6;
    float ga[4], be[4], accg[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(a.gamma + c, ga);
    ld4(a.beta + c, be);
    for (long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        float y[4], g[4], d[4], dy[4], dg[4], dxh[4], xh[4];
        ld4(a.y + row * a.C + c, y);
        ld4(a.g + row * a.C + c, g);
        ld4(a.dout + row * a.C + c, d);
        const float mean = a.stats[(row * a.H + head) * 2], rstd = a.stats[(row * a.H + head) * 2 + 1];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xh[q] = (y[q] - mean) * rstd;
            dg[q] = d[q] * fmaf(xh[q], ga[q], be[q]);
            const float dno = d[q] * g[q];
            accg[q] = fmaf(dno, xh[q], accg[q]);
            accb[q] += dno;
            dxh[q] = dno * ga[q];
            s1 += dxh[q];
            s2 = fmaf(dxh[q], xh[q], s2);
        }
        s1 = row_sum16(s1) * (1.f / 64.f);
        s2 = row_sum16(s2) * (1.f / 64.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) dy[q] = rstd * (dxh[q] - s1 - xh[q] * s2);
        io4<bf16_t>::store(a.dy + row * a.C + c, dy);
        io4<bf16_t>::store(a.dg + row * a.C + c, dg);
    }
    *reinterpret_cast<float4*>(a.dgamma_part + (long)blockIdx.x * a.C + c) = make_float4(accg[0], accg[1], accg[2], accg[3]);
    *reinterpret_cast<float4*>(a.dbeta_part + (long)blockIdx.x * a.C + c) = make_float4(accb[0], accb[1], accb[2], accb[3]);
}

// ---- flat elementwise kernels of the channel-mix FFN: 8 bf16 per lane (16-byte accesses), grid-stride over n / 8 units -----------
struct FlatArgs {
    long n8;                  // number of 8-element units (n / 8)
    const bf16_t *a, *b, *dout;
    bf16_t *out, *da, *db;
};
__device__ __forceinline__ void ld8(const bf16_t* p, float (&o)[8])
{
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    o[0] = bf_lo(raw.x); o[1] = bf_hi(raw.x); o[2] = bf_lo(raw.y); o[3] = bf_hi(raw.y);
    o[4] = bf_lo(raw.z); o[5] = bf_hi(raw.z); o[6] = bf_lo(raw.w); o[7] = bf_hi(raw.w);
}
__device__ __forceinline__ void st8(bf16_t* p, const float (&v)[8])
{
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
}
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

template <bool BWD> __global__ __launch_bounds__(256) void sqrelu_kernel(const FlatArgs a)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n8; i += (long)gridDim.x * blockDim.x) {
        float x[8], o[8];
        ld8(a.a + 8 * i, x);
        if constexpr (BWD) {
            float d[8];
            ld8(a.dout + 8 * i, d);
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = fmaxf(x[q], 0.f) * d[q] * 2.f;   // r d first: exact, so inf only where 2 r d overflows
            st8(a.da + 8 * i, o);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) { const float r = fmaxf(x[q], 0.f); o[q] = r * r; }
            st8(a.out + 8 * i, o);
        }
    }
}
template <bool BWD> __global__ __launch_bounds__(256) void sigmul_kernel(const FlatArgs a)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n8; i += (long)gridDim.x * blockDim.x) {
        float r[8], kv[8], o[8];
        ld8(a.a + 8 * i, r);
        ld8(a.b + 8 * i, kv);
        if constexpr (BWD) {
            float d[8], o2[8];
            ld8(a.dout + 8 * i, d);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float s = sigmoidf_(r[q]);
                o[q] = d[q] * kv[q] * s * (1.f - s);
                o2[q] = d[q] * s;
            }
            st8(a.da + 8 * i, o);
            st8(a.db + 8 * i, o2);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = sigmoidf_(r[q]) * kv[q];
            st8(a.out + 8 * i, o);
        }
    }
}
// wkv6_shift_keep: what a packed batch leaves in a token-shift slot pool.  One workgroup per candidate row: workgroup i < n_seq carries the
// last served token of sequence i to slot_out[i], workgroup n_seq + e carries snapshot entry e (its sequence by bisection in the clamped
// cu_snap) to snap_slot[e].  Every index is clamped or judged before it forms an address; a dead candidate leaves before any access to x or
// the pool, which is never read.  Rows are copied as bits (8 bytes per thread), not through fp32: a NaN keeps its payload.
struct KeepArgs {
    int total_T, n_seq, max_seqlen, C, n_slots, snap_every, n_snap;
    const int* cu;            // [n_seq + 1]
    const bf16_t* x;          // [total_T,C]
    bf16_t* pool;             // [n_slots,C]
    const int* slot_out;      // [n_seq] or null (slot = sequence index)
    const int* cu_snap;       // [n_seq + 1]
    const int* snap_slot;     // [n_snap]
};

__global__ void shift_keep_kernel(const KeepArgs a)
{
    const int i = blockIdx.x;
    const bool last = i < a.n_seq;
    const int e = i - a.n_seq;                           // snapshot entry (!last): 0 <= e < n_snap by the grid
    int s = i;
    if (!last) {                                         // the last s < n_seq with cu_snap[s] <= e
        s = seq_of_row(a.cu_snap, a.n_seq, e, [&](int v) { return clampi(v, 0, a.n_snap); });
        if (s < 0) return;
    }
    const int a0 = clampi(a.cu[s], 0, a.total_T), b0 = clampi(a.cu[s + 1], 0, a.total_T);
    const int len = min(max(b0 - a0, 0), a.max_seqlen);
    if (len <= 0) return;
    int row, dst;
    if (last) {
        row = a0 + len - 1;
        dst = a.slot_out ? a.slot_out[s] : s;
    } else {
        const int c0 = clampi(a.cu_snap[s], 0, a.n_snap), c1 = clampi(a.cu_snap[s + 1], 0, a.n_snap);
        const int j = e - c0;                            // >= 0 by the bisection
        if (j >= min(len / a.snap_every, max(c1 - c0, 0))) return;
        row = a0 + (j + 1) * a.snap_every - 1;           // (j + 1) snap_every <= len: inside the sequence, no overflow
        dst = a.snap_slot[e];
    }
    if (dst < 0 || dst >= a.n_slots) return;
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    const int c = 4 * threadIdx.x;
    *(v2u*)(a.pool + (long)dst * a.C + c) = *(const v2u*)(a.x + (long)row * a.C + c);
}

template <auto Kernel> int launch_flat(const FlatArgs& a, hipStream_t st)
{
    const long blocks = (a.n8 + 255) / 256;
    return to_rc(launch<Kernel>(dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, a));
}

int check_rows(long rows, int C)
{
    if (rows < 1 || C < 64 || C % 64 != 0 || C / 4 > 1024) return WKV6_EINVAL;
    if (rows * (long)C >= (1L << 40)) return WKV6_EUNSUPPORTED;
    return WKV6_OK;
}

// The (NS, m) pairs the lerp kernels are built for, in one place: f(NS, HAS_M), both as integral constants, launches; any other pair is
// refused.
template <typename F> int dispatch_lerp(int NS, bool has_m, F f)
{
    if (NS == 1 && !has_m) return to_rc(f(std::integral_constant<int, 1>(), std::false_type()));
    if (NS == 5 && has_m) return to_rc(f(std::integral_constant<int, 5>(), std::true_type()));
    if (NS == 1 && has_m) return to_rc(f(std::integral_constant<int, 1>(), std::true_type()));
    if (NS == 2 && !has_m) return to_rc(f(std::integral_constant<int, 2>(), std::false_type()));
    return WKV6_EUNSUPPORTED;
}

// forward: one workgroup per row; backward: nparts workgroups.  The kernel by the arrays that are there: cu -> packed, rev_n -> reversal map
template <int NS, bool HAS_M> hipError_t launch_lerp(const LerpArgs& a, bool bwd, hipStream_t st)
{
    const dim3 grid(bwd ? (unsigned)a.nparts : (unsigned)((long)a.B * a.T)), block(a.C / 4);
    if (a.cu && a.rev_n)
        return bwd ? launch<ddlerp_bwd_varlen_rev_kernel<NS, HAS_M>>(grid, block, 0, st, a)
                   : launch<ddlerp_fwd_varlen_rev_kernel<NS, HAS_M>>(grid, block, 0, st, a);
    if (a.cu) return bwd ? launch<ddlerp_bwd_kernel<NS, HAS_M, true>>(grid, block, 0, st, a) : launch<ddlerp_fwd_kernel<NS, HAS_M, true>>(grid, block, 0, st, a);
    return bwd ? launch<ddlerp_bwd_kernel<NS, HAS_M>>(grid, block, 0, st, a) : launch<ddlerp_fwd_kernel<NS, HAS_M>>(grid, block, 0, st, a);
}

// ---- what the eight wkv6_ddlerp_* entry points share: an entry point types its tensors into the argument block (lerp_tensors, and
// set_grads for a backward), adds the arrays of its form, and ddlerp checks sizes, then nulls, then dispatches
enum LerpForm { DENSE, PACKED, SLOTS };

SlotLerpArgs lerp_tensors(int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa, const int* rev_n)
{
    SlotLerpArgs a = {};
    a.C = C; a.NS = NS;
    a.x = (const bf16_t*)x; a.shifted0 = (const bf16_t*)shifted0; a.m = (const bf16_t*)m; a.maa = (const bf16_t*)maa;
    a.rev_n = rev_n;
    return a;
}
void set_grads(LerpArgs& a, const void* dout, void* dx, void* dm, float* dmaa_part, int nparts)
{
    a.dout = (const bf16_t*)dout; a.dx = (bf16_t*)dx; a.dm = (bf16_t*)dm; a.dmaa_part = dmaa_part; a.nparts = nparts;
}
// B x T rows as the caller gave them (PACKED, SLOTS: 1 x total_T).  The order of the refusals is part of the interface.
int ddlerp(LerpForm form, bool bwd, long B, long T, SlotLerpArgs a, void* stream)
{
    const bool packed = form != DENSE;
    if (B < 1 || T < 1 || (packed && a.n_seq < 1) || (form == SLOTS && a.n_slots < 1) || (bwd && a.nparts < 1)) return WKV6_EINVAL;
    if (int rc = check_rows(B * T, a.C)) return rc;
    if (packed && T > 0x7fffffffL) return WKV6_EUNSUPPORTED;                  // cu_seqlens is int32
    if (form == SLOTS && !a.slot && a.n_slots < a.n_seq) return WKV6_EINVAL;  // slot = sequence index: the pool must hold n_seq slots
    if ((packed && !a.cu) || !a.x || !a.maa || (form == SLOTS && !a.shifted0)) return WKV6_ENULL;
    if (bwd ? !a.dout || !a.dx || !a.dmaa_part || (a.m && !a.dm) : !a.out) return WKV6_ENULL;
    if (form == SLOTS) {
        if (((uintptr_t)a.x | (uintptr_t)a.out | (uintptr_t)a.shifted0) & 7) return WKV6_EINVAL;
        if (overlap(a.out, (size_t)a.NS * T * a.C * 2, a.shifted0, (size_t)a.n_slots * a.C * 2)) return WKV6_EINVAL;
    }
    a.B = (int)B; a.T = (int)T;
    const hipStream_t st = (hipStream_t)stream;
    return dispatch_lerp(a.NS, a.m != nullptr, [&](auto ns, auto has_m) {
        if (form == SLOTS) return launch<ddlerp_fwd_slots_kernel<ns(), has_m()>>(dim3((unsigned)a.T), dim3(a.C / 4), 0, st, a);
        return launch_lerp<ns(), has_m()>(a, bwd, st);
    });
}

}  // namespace
}  // namespace wkv6

using namespace wkv6;

extern "C" {

int wkv6_ddlerp_forward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                        void* out, void* stream)
{
    return wkv6_ddlerp_rev_forward(B, T, C, NS, x, shifted0, m, maa, nullptr, out, stream);
}
int wkv6_ddlerp_rev_forward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                            const int* rev_n, void* out, void* stream)
{
    SlotLerpArgs a = lerp_tensors(C, NS, x, shifted0, m, maa, rev_n);
    a.out = (bf16_t*)out;
    return ddlerp(DENSE, false, B, T, a, stream);
}
int wkv6_ddlerp_backward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                         const void* dout, void* dx, void* dm, float* dmaa_part, int nparts, void* stream)
{
    return wkv6_ddlerp_rev_backward(B, T, C, NS, x, shifted0, m, maa, nullptr, dout, dx, dm, dmaa_part, nparts, stream);
}
int wkv6_ddlerp_rev_backward(int B, int T, int C, int NS, const void* x, const void* shifted0, const void* m, const void* maa,
                             const int* rev_n, const void* dout, void* dx, void* dm, float* dmaa_part, int nparts, void* stream)
{
    SlotLerpArgs a = lerp_tensors(C, NS, x, shifted0, m, maa, rev_n);
    set_grads(a, dout, dx, dm, dmaa_part, nparts);
    return ddlerp(DENSE, true, B, T, a, stream);
}

// (the packed calls: rev_n == null is the plain packed shift)
int wkv6_ddlerp_varlen_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                               const void* m, const void* maa, void* out, void* stream)
{
    return wkv6_ddlerp_varlen_rev_forward(total_T, n_seq, C, NS, cu_seqlens, x, shifted0, m, maa, nullptr, out, stream);
}
int wkv6_ddlerp_varlen_rev_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                   const void* m, const void* maa, const int* rev_n, void* out, void* stream)
{
    SlotLerpArgs a = lerp_tensors(C, NS, x, shifted0, m, maa, rev_n);
    a.cu = cu_seqlens; a.n_seq = n_seq;
    a.out = (bf16_t*)out;
    return ddlerp(PACKED, false, 1, total_T, a, stream);
}
int wkv6_ddlerp_varlen_backward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                const void* m, const void* maa, const void* dout, void* dx, void* dm, float* dmaa_part, int nparts,
                                void* stream)
{
    return wkv6_ddlerp_varlen_rev_backward(total_T, n_seq, C, NS, cu_seqlens, x, shifted0, m, maa, nullptr, dout, dx, dm, dmaa_part, nparts,
                                           stream);
}
int wkv6_ddlerp_varlen_rev_backward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shifted0,
                                    const void* m, const void* maa, const int* rev_n, const void* dout, void* dx, void* dm,
                                    float* dmaa_part, int nparts, void* stream)
{
    SlotLerpArgs a = lerp_tensors(C, NS, x, shifted0, m, maa, rev_n);
    a.cu = cu_seqlens; a.n_seq = n_seq;
    set_grads(a, dout, dx, dm, dmaa_part, nparts);
    return ddlerp(PACKED, true, 1, total_T, a, stream);
}

int wkv6_ddlerp_slots_forward(long total_T, int n_seq, int C, int NS, const int* cu_seqlens, const void* x, const void* shift_pool,
                              int n_slots, const int* slot, const void* m, const void* maa, void* out, void* stream)
{
    SlotLerpArgs a = lerp_tensors(C, NS, x, shift_pool, m, maa, nullptr);
    a.cu = cu_seqlens; a.n_seq = n_seq; a.slot = slot; a.n_slots = n_slots;
    a.out = (bf16_t*)out;
    return ddlerp(SLOTS, false, 1, total_T, a, stream);
}

int wkv6_shift_keep(long total_T, int n_seq, int max_seqlen, int C, const int* cu_seqlens, const void* x, void* shift_pool, int n_slots,
                    const int* slot_out, int snap_every, const int* cu_snap, const int* snap_slot, int n_snap, void* stream)
{
    if (total_T < 1 || n_seq < 1 || n_slots < 1 || max_seqlen < 1 || snap_every < 0 || n_snap < 0) return WKV6_EINVAL;
    if (int rc = check_rows(total_T, C)) return rc;
    if (total_T > 0x7fffffffL) return WKV6_EUNSUPPORTED;          // cu_seqlens is int32
    if (!slot_out && n_slots < n_seq) return WKV6_EINVAL;
    if (!cu_seqlens || !x || !shift_pool) return WKV6_ENULL;
    const bool snaps = snap_every > 0 && n_snap > 0;
    if (snaps && (!cu_snap || !snap_slot)) return WKV6_ENULL;
    if (((uintptr_t)x | (uintptr_t)shift_pool) & 7) return WKV6_EINVAL;
    if (overlap(x, (size_t)total_T * C * 2, shift_pool, (size_t)n_slots * C * 2)) return WKV6_EINVAL;
    const long grid = (long)n_seq + (snaps ? n_snap : 0);
    if (grid > 0x7fffffffL) return WKV6_EUNSUPPORTED;
    KeepArgs a = {};
    a.total_T = (int)total_T; a.n_seq = n_seq; a.max_seqlen = max_seqlen; a.C = C; a.n_slots = n_slots;
    a.snap_every = snaps ? snap_every : 0; a.n_snap = snaps ? n_snap : 0;
    a.cu = cu_seqlens; a.x = (const bf16_t*)x; a.pool = (bf16_t*)shift_pool; a.slot_out = slot_out;
    a.cu_snap = cu_snap; a.snap_slot = snap_slot;
    return to_rc(launch<shift_keep_kernel>(dim3((unsigned)grid), dim3(C / 4), 0, (hipStream_t)stream, a));
}

int wkv6_sqrelu_forward(long n, const void* x, void* out, void* stream)
{
    if (n < 8 || n % 8) return WKV6_EINVAL;
    if (!x || !out) return WKV6_ENULL;
    FlatArgs a = {};
    a.n8 = n / 8; a.a = (const bf16_t*)x; a.out = (bf16_t*)out;
    return launch_flat<sqrelu_kernel<false>>(a, (hipStream_t)stream);
}
int wkv6_sqrelu_backward(long n, const void* x, const void* dout, void* dx, void* stream)
{
    if (n < 8 || n % 8) return WKV6_EINVAL;
    if (!x || !dout || !dx) return WKV6_ENULL;
    FlatArgs a = {};
    a.n8 = n / 8; a.a = (const bf16_t*)x; a.dout = (const bf16_t*)dout; a.da = (bf16_t*)dx;
    return launch_flat<sqrelu_kernel<true>>(a, (hipStream_t)stream);
}
int wkv6_sigmul_forward(long n, const void* r, const void* kv, void* out, void* stream)
{
    if (n < 8 || n % 8) return WKV6_EINVAL;
    if (!r || !kv || !out) return WKV6_ENULL;
    FlatArgs a = {};
    a.n8 = n / 8; a.a = (const bf16_t*)r; a.b = (const bf16_t*)kv; a.out = (bf16_t*)out;
    return launch_flat<sigmul_kernel<false>>(a, (hipStream_t)stream);
}
int wkv6_sigmul_backward(long n, const void* r, const void* kv, const void* dout, void* dr, void* dkv, void* stream)
{
    if (n < 8 || n % 8) return WKV6_EINVAL;
    if (!r || !kv || !dout || !dr || !dkv) return WKV6_ENULL;
    FlatArgs a = {};
    a.n8 = n / 8; a.a = (const bf16_t*)r; a.b = (const bf16_t*)kv; a.dout = (const bf16_t*)dout; a.da = (bf16_t*)dr; a.db = (bf16_t*)dkv;
    return launch_flat<sigmul_kernel<true>>(a, (hipStream_t)stream);
}

int wkv6_gn_gate_forward(long rows, int C, int H, const void* y, const void* g, const void* gamma, const void* beta,
                         float eps, void* out, float* stats, void* stream)
{
    if (int rc = check_rows(rows, C)) return rc;
    if (H * HEAD != C) return WKV6_EINVAL;
    if (!y || !g || !gamma || !beta || !out) return WKV6_ENULL;
    GnArgs a = {};
    a.rows = rows; a.C = C; a.H = H; a.eps = eps;
    a.y = (const bf16_t*)y; a.g = (const bf16_t*)g; a.gamma = (const bf16_t*)gamma; a.beta = (const bf16_t*)beta;
    a.out = (bf16_t*)out; a.stats = stats;
    return to_rc(launch<gn_gate_fwd_kernel>(dim3((unsigned)rows), dim3(C / 4), 0, (hipStream_t)stream, a));
}

int wkv6_gn_gate_backward(long rows, int C, int H, const void* y, const void* g, const void* gamma, const void* beta,
                          const float* stats, const void* dout, void* dy, void* dg, float* dgamma_part, float* dbeta_part,
                          int nparts, void* stream)
{
    if (int rc = check_rows(rows, C)) return rc;
    if (H * HEAD != C || nparts < 1) return WKV6_EINVAL;
    if (!y || !g || !gamma || !beta || !stats || !dout || !dy || !dg || !dgamma_part || !dbeta_part) return WKV6_ENULL;
    GnArgs a = {};
    a.rows = rows; a.C = C; a.H = H;
    a.y = (const bf16_t*)y; a.g = (const bf16_t*)g; a.gamma = (const bf16_t*)gamma; a.beta = (const bf16_t*)beta;
    a.stats = const_cast<float*>(stats); a.dout = (const bf16_t*)dout; a.dy = (bf16_t*)dy; a.dg = (bf16_t*)dg;
    a.dgamma_part = dgamma_part; a.dbeta_part = dbeta_part; a.nparts = nparts;
    return to_rc(launch<gn_gate_bwd_kernel>(dim3(nparts), dim3(C / 4), 0, (hipStream_t)stream, a));
}

}  // extern "C"
