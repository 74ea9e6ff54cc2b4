// The staging pipeline of the exact token-serial kernels, once: scan_fwd / scan_bwd_s / scan_bwd_g (wkv6_scan.hip) and
// wkv5_fwd / wkv5_bwd_a / wkv5_bwd_g (wkv5_scan.hip) are the same machine -- a workgroup of NW waves per (row, head) that stages TB tokens
// at a time through a double-buffered LDS image (staging role: thread -> (token slot spp, channels sc0..)), scans them out of LDS with the
// state in registers (compute role: lane -> i x j tile), and stores the batch's results as whole row segments behind the barrier.
// Device only.  What lives here, each piece once:
//   geometry         TB, ROW, PLANE, Geo<NW>, pick<NV>, the compute roles ColTile<NW> (forward) and RowTile<NW> (backward)
//   LDS image        Lds<NIN, COEF, NOUT>: float offsets of the sub-buffers and the byte count, for the kernel's carving AND the launcher
//   row prologue     open_row<NW>(args): ScanArgs (packed rows, lens, reversal map) or Wkv5Args (dense, identity map); StageRow::at is
//                    the one form of "element offset of tensor X at scan position p"; load_u; load_at / store_at / put_at
//   pipeline driver  run_pipeline<ASCENDING>(ntok, load, stage, take, scan, mid, behind, emit)
//   per-token bodies fwd_tokens, asc_tokens (sweep S / WKV5 ascending pass), adj_tokens (sweep G / WKV5 descending pass); the decay
//                    comes from an LDS plane (DecayPlane) or from registers (DecayRegs)
//   epilogues        sum_waves (gv), store_slot_partial (gu, and what WKV5 stores beside it), zero_tile / load_tile / store_tile (states)
//
// Invariants (the kernels' results are bit-identical to the hand-written copies these pieces replace):
//   * Floating-point order is fixed: ii outer / jj inner in the bodies' FMA chains, the token_sum reductions, waves w_ = 0..NW-1 in
//     sum_waves, token slots pp = 0..TB-1 in store_slot_partial (and later positions first in scan_bwd_g's finish_gw).
//   * Every __syncthreads() here is reached by the whole workgroup: the driver's trip count depends on ntok alone, which is uniform over
//     the workgroup, and a kernel that leaves early (the SLOTS length window) does so before it calls anything but open_row.  open_row
//     reads only the int arrays of the argument block (order, lens, tok_off, rev_n), which hold an entry for every row.
//   * No helper forms an address from a state slot: the kernels test the slot (-1: no state) and only then compute the offset they pass.
//
// Three forms decide the code the compiler makes of these pieces (profiles/scan_fold.txt; each was measured the other way round):
//   * A kernel's load and emit pieces form every offset they need FIRST, in front of their `if (valid)` and their LDS reads (a reversal
//     map makes an offset a compare, two selects and a 64-bit multiply-add).  Formed where they are used, the arithmetic lands between
//     the global loads, which no longer issue back to back (+1 % on the bf16 forward), and the decay's offset behind the branch splits
//     the loads over two exec-mask regions (ten instructions per token batch; 1.4 - 2.9 % of the WKV6 kernels' time).
//   * WKV6's load pieces fetch the decay LAST (load_ew behind the other loads).  Fetched first, the 16-bit kernels wait for it and
//     convert it before they issue the other loads (+0.7 % forward, +2.7 % backward in bf16); a scheduling barrier in front of the
//     conversion makes the fp32 kernels wait for all loads (+2 - 4 %).  What is left of the order's effect: the fp32 sweep G issues
//     half its loads behind the conversion's wait, +0.6 - 0.8 % on the fp32 backward against the hand-written copy.
//   * The two arms of an either-or access (y or its fp32 side buffer) go through the SAME helper (load_at / store_at), so that with fp32
//     I/O they fold into one instruction as they did when written out.
#pragma once
#include "wkv5_scan.h"
#include "wkv6_scan.h"

namespace wkv6 {

constexpr int TB = 16;                 // tokens staged per LDS batch
constexpr int ROW = HEAD;              // floats per staged token row
constexpr int PLANE = TB * ROW;        // floats of one tensor's batch in LDS

template <int NV> __device__ __forceinline__ float pick(const float (&v)[NV], int s)
{
    float o = v[0];
#pragma unroll
    for (int q = 1; q < NV; ++q) o = (s == q) ? v[q] : o;
    return o;
}

// Per-thread staging geometry.
template <int NW> struct Geo {
    static constexpr int NT = NW * 64;
    static constexpr int CPT = TB * ROW / NT;      // channels staged per thread (4 or 2)
    static constexpr int TPT = ROW / CPT;          // threads per token (16 or 32)
    static_assert(CPT == 2 || CPT == 4, "unsupported wave count");
};

// Compute role of the forward kernels: wave wv owns value columns [wv*JPW, (wv+1)*JPW); lane (jb = lane>>4, ib = lane&15) owns
// S[4ib..4ib+3][j0..j0+JR-1].
template <int NW> struct ColTile {
    static constexpr int JPW = HEAD / NW, JR = JPW / 4;
    int ib, i0, j0;
    __device__ __forceinline__ ColTile(int lane, int wv) : ib(lane & 15), i0((lane & 15) * 4), j0(wv * JPW + (lane >> 4) * JR) {}
};
// ... of the backward kernels: wave wv owns key rows [wv*IPW, (wv+1)*IPW); lane (irow = lane>>4, jl = lane&15) owns
// S[i0..i0+IR-1][4jl..4jl+3].
template <int NW> struct RowTile {
    static constexpr int IPW = HEAD / NW, IR = IPW / 4;
    int irow, jl, i0, j0;
    __device__ __forceinline__ RowTile(int lane, int wv) : irow(lane >> 4), jl(lane & 15), i0(wv * IPW + (lane >> 4) * IR), j0((lane & 15) * 4) {}
};

// LDS image of a kernel, in floats: [2][NIN] staged input planes, [2][TB] per-token coefficients in 64 reserved floats (COEF), then NOUT
// double-buffered result planes [2][TB][ROW] (result k at out(k); a group of NW consecutive ones holds the waves' partial planes).
template <int NIN, bool COEF, int NOUT> struct Lds {
    static constexpr int BUF = NIN * PLANE;                     // one buffer of the input image
    static constexpr int IN = 0, COEF_AT = 2 * BUF, OUT = COEF_AT + (COEF ? 64 : 0);
    static constexpr int out(int k) { return OUT + 2 * k * PLANE; }
    static constexpr size_t BYTES = (size_t)(OUT + 2 * NOUT * PLANE) * sizeof(float);
};

// ---- row prologue ----------------------------------------------------------------------------------------------------------------
struct IdMap {      // dense rows: every tensor holds token p at scan position p
    __device__ __forceinline__ int operator()(int p, unsigned) const { return p; }
};
// The workgroup's row and the thread's staging role: token slot spp of a batch, channels sc0.. of the head.
template <typename Map> struct StageRow {
    int tid, lane, wv, b, h, ntok, C, spp, sc0;
    long base;          // element offset of (first token of the row, first channel of the head)
    Map tokmap;         // token each tensor holds at scan position p
    // element offset of the thread's channels of tensor `bit` (REV_*; 0: scratch indexed by scan position) at scan position p
    __device__ __forceinline__ long at(int p, unsigned bit) const { return base + (long)tokmap(p, bit) * C + sc0; }
    __device__ __forceinline__ long tail(int t) const { return base + (long)t * C + sc0; }      // token t, beyond the scanned ones
    __device__ __forceinline__ int seg() const { return spp * ROW + sc0; }                       // the thread's segment of an LDS plane
};
// the CPT channels at element offset idx of a tensor with elements of type T
template <typename T, int CPT> __device__ __forceinline__ void load_at(const void* x, long idx, float (&o)[CPT])
{
    ion<T, CPT>::load(reinterpret_cast<const T*>(x) + idx, o);
}
template <typename T, int CPT> __device__ __forceinline__ void store_at(void* x, long idx, const float (&v)[CPT])
{
    ion<T, CPT>::store(reinterpret_cast<T*>(x) + idx, v);
}
// store, or add to what is there (accumulate)
template <typename T, int CPT> __device__ __forceinline__ void put_at(void* x, long idx, float (&o)[CPT], int accumulate)
{
    if (accumulate) {
        float old[CPT];
        load_at<T>(x, idx, old);
#pragma unroll
        for (int c = 0; c < CPT; ++c) o[c] += old[c];
    }
    store_at<T>(x, idx, o);
}

template <int NW, typename Map>
__device__ __forceinline__ StageRow<Map> stage_row(int b, int h, int ntok, int C, long first_tok, Map tokmap)
{
    using G = Geo<NW>;
    const int tid = threadIdx.x;
    return StageRow<Map>{tid, tid & 63, tid >> 6, b, h, ntok, C, tid / G::TPT, (tid % G::TPT) * G::CPT, first_tok * C + (long)h * HEAD, tokmap};
}
// (packed variable-length batch, a.tok_off set: sequence a.order[slot], longest first, tokens from a.tok_off[b] of [total_T, C])
template <int NW> __device__ __forceinline__ StageRow<RevMap> open_row(const ScanArgs& a)
{
    const int b = a.tok_off ? a.order[blockIdx.x / a.H] : blockIdx.x / a.H, h = blockIdx.x % a.H;
    int ntok = a.T;
    if (a.lens) ntok = min(max(a.lens[b], 0), a.T);
    return stage_row<NW>(b, h, ntok, a.C, a.tok_off ? (long)a.tok_off[b] : (long)b * a.T, make_revmap(a, b, ntok));
}
template <int NW> __device__ __forceinline__ StageRow<IdMap> open_row(const Wkv5Args& a)
{
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    return stage_row<NW>(b, h, a.T, a.C, (long)b * a.T, IdMap{});
}

template <int N, typename... More> __device__ __forceinline__ void zero(float (&x)[N], More&... more)
{
#pragma unroll
    for (int c = 0; c < N; ++c) x[c] = 0.f;
    if constexpr (sizeof...(More) > 0) zero(more...);
}
// the bonus u of the thread's staged channels (use == 0: treated as 0)
template <typename T, int CPT, typename Map> __device__ __forceinline__ void load_u(const void* u, int use, const StageRow<Map>& w, float (&uu)[CPT])
{
    zero(uu);
    if (use) load_at<T>(u, (long)(w.h * HEAD + w.sc0), uu);
}

// ---- staging helpers -----------------------------------------------------------------------------------------------------------
// the thread's channels of consecutive planes of an input buffer (seg: the buffer's base + StageRow::seg())
template <int CPT, typename... P> __device__ __forceinline__ void stage_planes(float* seg, const P&... planes)
{
    int i = 0;
    (lds_store<CPT>(seg + (i++) * PLANE, planes), ...);
}
// the thread's part of sum_c x[c] y[c] and of sum_c r[c] u[c] k[c] over a token's channels (token_sum adds the parts)
template <int CPT> __device__ __forceinline__ float dot_part(const float (&x)[CPT], const float (&y)[CPT])
{
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < CPT; ++c) part = fmaf(x[c], y[c], part);
    return part;
}
template <int CPT> __device__ __forceinline__ float bonus_part(const float (&r)[CPT], const float (&u)[CPT], const float (&k)[CPT])
{
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < CPT; ++c) part = fmaf(r[c] * u[c], k[c], part);
    return part;
}
template <int N> __device__ __forceinline__ void copy(float (&to)[N], const float (&from)[N])
{
#pragma unroll
    for (int c = 0; c < N; ++c) to[c] = from[c];
}

// ---- pipeline driver -----------------------------------------------------------------------------------------------------------
struct Nothing {    // a piece a kernel does not have
    template <typename... A> __device__ __forceinline__ void operator()(A&&...) const {}
};
// Batches q = 0..nq-1 of TB tokens (ASCENDING) or nq-1..0, buffer q & 1.  Per batch: take() hands the staged batch's register values
// over to the scan ("n* -> c*"), load(q') fetches the next batch into registers, scan(q, buf, nb) walks the nb staged tokens,
// mid(q) runs between scan and stage (SNAP's state store), stage(buf') writes the next batch to LDS, and behind the barrier behind()
// (scan_bwd_g's pending gw) and emit(q, buf), the coalesced store of the batch's results.  A row without tokens passes the barrier only.
template <bool ASCENDING, typename Load, typename Stage, typename Take, typename Scan, typename Mid, typename Behind, typename Emit>
__device__ __forceinline__ void run_pipeline(int ntok, Load&& load, Stage&& stage, Take&& take, Scan&& scan, Mid&& mid, Behind&& behind, Emit&& emit)
{
    const int nq = (ntok + TB - 1) / TB;
    if (nq > 0) {
        const int q0 = ASCENDING ? 0 : nq - 1;
        load(q0);
        stage(q0 & 1);
    }
    __syncthreads();
    auto batch = [&](int q, bool more, int next) {
        const int buf = q & 1;
        take();
        if (more) load(next);
        scan(q, buf, min(TB, ntok - q * TB));
        mid(q);
        if (more) stage(buf ^ 1);
        __syncthreads();
        behind();
        emit(q, buf);
    };
    if constexpr (ASCENDING) {
        for (int q = 0; q < nq; ++q) batch(q, q + 1 < nq, q + 1);
    } else {
        for (int q = nq - 1; q >= 0; --q) batch(q, q > 0, q - 1);
    }
}

// ---- per-token bodies ----------------------------------------------------------------------------------------------------------
// Where a body finds the decays of its N key rows i0.. at token slot pp: a staged plane (WKV6: a decay per token) or the registers that
// hold them for the whole row (WKV5).
template <int N> struct DecayPlane {
    const float* plane;
    __device__ __forceinline__ void get(int pp, int i0, float (&d)[N]) const { lds_load<N>(plane + pp * ROW + i0, d); }
};
template <int N> struct DecayRegs {
    const float (&regs)[N];
    __device__ __forceinline__ void get(int, int, float (&d)[N]) const { copy(d, regs); }
};

// forward:  y_t[j] = sum_i r_t[i] S_t[i][j] + cf[t] v_t[j],  S <- d_t (.) S + k_t v_t^T   (cf: the staged sum_i r_t[i] u[i] k_t[i])
template <int NW, typename Decay>
__device__ __forceinline__ void fwd_tokens(float (&S)[4][ColTile<NW>::JR], const ColTile<NW>& t, const float* rs, const float* ks, const float* vs,
                                           const Decay& dec, const float* cf, float* yb, int nb)
{
    constexpr int JR = ColTile<NW>::JR;
    for (int pp = 0; pp < nb; ++pp) {
        float r4[4], k4[4], d4[4], vv[JR], yacc[JR];
        lds_load<4>(rs + pp * ROW + t.i0, r4);
        lds_load<4>(ks + pp * ROW + t.i0, k4);
        dec.get(pp, t.i0, d4);
        lds_load<JR>(vs + pp * ROW + t.j0, vv);
        zero(yacc);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < JR; ++jj) {
                const float kv = k4[ii] * vv[jj];
                yacc[jj] = fmaf(r4[ii], S[ii][jj], yacc[jj]);
                S[ii][jj] = fmaf(S[ii][jj], d4[ii], kv);
            }
        const float tot = row_reduce(yacc, t.ib);
        if (t.ib < JR) {
            const int jj = row_sel<JR>(t.ib);
            yb[pp * ROW + t.j0 + jj] = fmaf(cf[pp], pick<JR>(vv, jj), tot);
        }
    }
}

// ascending backward pass:  dq_t[i] = sum_j gy_t[j] S_t[i][j],  S <- d_t (.) S + k_t v_t^T.  also(pp, g4) sees gy_t and the state BEFORE
// the update (WKV5: its D = dS/dd term).
template <int NW, typename Decay, typename Also>
__device__ __forceinline__ void asc_tokens(float (&S)[RowTile<NW>::IR][4], const RowTile<NW>& t, const float* ks, const float* vs, const float* gs,
                                           const Decay& dec, float* qb, int nb, Also&& also)
{
    constexpr int IR = RowTile<NW>::IR;
    for (int pp = 0; pp < nb; ++pp) {
        float kk[IR], dd[IR], v4[4], g4[4], dq[IR];
        lds_load<IR>(ks + pp * ROW + t.i0, kk);
        dec.get(pp, t.i0, dd);
        lds_load<4>(vs + pp * ROW + t.j0, v4);
        lds_load<4>(gs + pp * ROW + t.j0, g4);
        also(pp, g4);
#pragma unroll
        for (int ii = 0; ii < IR; ++ii) {
            dq[ii] = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                dq[ii] = fmaf(g4[jj], S[ii][jj], dq[ii]);
                S[ii][jj] = fmaf(S[ii][jj], dd[ii], kk[ii] * v4[jj]);
            }
        }
        const float tot = row_reduce(dq, t.jl);
        if (t.jl < IR) qb[pp * ROW + t.i0 + row_sel<IR>(t.jl)] = tot;
    }
}

// adjoint (descending) pass:  dk_t[i] = sum_j G[i][j] v_t[j] -> kb,  wave wv's part of sum_i k_t[i] G[i][j] -> vb (its own plane),
// G <- d_t (.) G + r_t gy_t^T
template <int NW, typename Decay>
__device__ __forceinline__ void adj_tokens(float (&Gs)[RowTile<NW>::IR][4], const RowTile<NW>& t, const float* rs, const float* ks, const float* vs,
                                           const float* gs, const Decay& dec, float* kb, float* vb, int nb)
{
    constexpr int IR = RowTile<NW>::IR;
    for (int pp = nb - 1; pp >= 0; --pp) {
        float rr[IR], kk[IR], dd[IR], v4[4], g4[4], gkp[IR], gvp[4];
        lds_load<IR>(rs + pp * ROW + t.i0, rr);
        lds_load<IR>(ks + pp * ROW + t.i0, kk);
        dec.get(pp, t.i0, dd);
        lds_load<4>(vs + pp * ROW + t.j0, v4);
        lds_load<4>(gs + pp * ROW + t.j0, g4);
        zero(gvp);
#pragma unroll
        for (int ii = 0; ii < IR; ++ii) {
            gkp[ii] = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                gkp[ii] = fmaf(v4[jj], Gs[ii][jj], gkp[ii]);
                gvp[jj] = fmaf(kk[ii], Gs[ii][jj], gvp[jj]);
                Gs[ii][jj] = fmaf(Gs[ii][jj], dd[ii], rr[ii] * g4[jj]);
            }
        }
        const float dk = row_reduce(gkp, t.jl);
        if (t.jl < IR) kb[pp * ROW + t.i0 + row_sel<IR>(t.jl)] = dk;
        const float gvt = col_reduce(gvp);
        vb[pp * ROW + t.j0 + col_sel(t.irow)] = gvt;
    }
}

// ---- epilogues -----------------------------------------------------------------------------------------------------------------
// the NW waves' partial planes of one buffer, summed in wave order (seg: the first wave's plane + StageRow::seg())
template <int NW, int CPT> __device__ __forceinline__ void sum_waves(const float* seg, float (&sum)[CPT])
{
    zero(sum);
#pragma unroll
    for (int w_ = 0; w_ < NW; ++w_) {
        float t2[CPT];
        lds_load<CPT>(seg + w_ * PLANE, t2);
#pragma unroll
        for (int c = 0; c < CPT; ++c) sum[c] += t2[c];
    }
}

// Per-row partial of what the staging threads accumulated per (token slot, channel): summed over the TB slots in slot order through the LDS
// plane `lds` and stored to element (b, h, channel) of `out` (null: skipped), fp32 or rounded to bf16.  also_stage() puts further per-channel
// values into LDS between the barriers, also_store(o) stores them (thread tid < HEAD, o = its element).  Workgroup-uniform.
template <int CPT, typename Map, typename AlsoStage, typename AlsoStore>
__device__ __forceinline__ void store_slot_partial(void* out, int f32, float* lds, const StageRow<Map>& w, const float (&acc)[CPT],
                                                   AlsoStage&& also_stage, AlsoStore&& also_store)
{
    __syncthreads();
    lds_store<CPT>(lds + w.seg(), acc);
    also_stage();
    __syncthreads();
    if (w.tid < HEAD) {
        const long o = (long)w.b * w.C + w.h * HEAD + w.tid;
        if (out) {
            float s = 0.f;
#pragma unroll
            for (int pp = 0; pp < TB; ++pp) s += lds[pp * ROW + w.tid];
            store_partial(out, f32, o, s);
        }
        also_store(o);
    }
}

// The lane's NI x NJ tile of a state [.., N(j), N(i)] with elements of type U: rows j0.., NI contiguous elements from column i0; `at` is
// the element offset of (j0, i0).
template <int NI, int NJ> __device__ __forceinline__ void zero_tile(float (&S)[NI][NJ])
{
#pragma unroll
    for (int ii = 0; ii < NI; ++ii)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) S[ii][jj] = 0.f;
}
template <typename U, int NI, int NJ> __device__ __forceinline__ void load_tile(const void* s, long at, float (&S)[NI][NJ])
{
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        float t[NI];
        ion<U, NI>::load(reinterpret_cast<const U*>(s) + at + (long)jj * HEAD, t);
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) S[ii][jj] = t[ii];
    }
}
template <typename U, int NI, int NJ> __device__ __forceinline__ void store_tile(void* s, long at, const float (&S)[NI][NJ])
{
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        float t[NI];
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) t[ii] = S[ii][jj];
        ion<U, NI>::store(reinterpret_cast<U*>(s) + at + (long)jj * HEAD, t);
    }
}
// element offset of the tile (j0, i0) of head h within one batch entry [H, N, N]
__device__ __forceinline__ long tile_at(int h, int j0, int i0) { return ((long)h * HEAD + j0) * HEAD + i0; }

}  // namespace wkv6
