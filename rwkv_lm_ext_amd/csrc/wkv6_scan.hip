// Exact-fp32 token-serial WKV6 kernels for gfx950.  Design notes: wkv6_scan.h; the staging pipeline they share with WKV5: wkv6_scan_stage.h.
#include "wkv6_scan_stage.h"

namespace wkv6 {
namespace {

template <typename T, int CPT>
__device__ __forceinline__ void load_ew(const ScanArgs& a, long idx, bool valid, float (&ew)[CPT])
{
    zero(ew);
    if (!valid) return;
    if (a.wkind != 1) {
        load_at<float>(a.w, idx, ew);      // (ew, or d when wkind == 2)
    } else {
        float w[CPT];
        load_at<T>(a.w, idx, w);
#pragma unroll
        for (int c = 0; c < CPT; ++c) ew[c] = -__expf(w[c]);
    }
}

// =====================================================================================================
// forward:  y_t[j] = sum_i r_t[i] S_t[i][j] + (sum_i r_t[i]u[i]k_t[i]) v_t[j];  S <- d_t (.) S + k_t v_t^T
// (cuda/wkv6_cuda.cu:44-57).  Lane layout: ColTile (wkv6_scan_stage.h).
// =====================================================================================================
// SLOTS (packed stateful inference, launch_scan_fwd_slots): the fp32 state of sequence b lives in slot a.state_slot[b] of the pool
// a.s0 == a.s_out and is updated in place; a.len_lo / a.len_hi select the sequences this launch serves (wkv6_scan.h).  Instantiations of
// their own: the dense and the packed training kernels keep their instruction streams.
// SNAP (launch_scan_fwd_snap): SLOTS, and the final state goes to slot a.state_slot_out[b], the state after every a.snap_every tokens to a
// slot of its own (wkv6_scan.h: SnapPlan) -- the registers S after a token batch, through the epilogue's per-lane store.  SNAP implies
// SLOTS and is instantiated as <T, NW, false, true>: the ISA guard of the SLOTS instantiations picks them by the prefix
// scan_fwd_kernel<T, 8, true of their mangled names, which has to stay theirs alone.
using FwdLds = Lds<4, true, 1>;        // r,k,d,v; coef; y
template <typename T, int NW, bool SLOTS_ = false, bool SNAP = false>
__global__ __launch_bounds__(NW * 64) void scan_fwd_kernel(const ScanArgs a)
{
    constexpr bool SLOTS = SLOTS_ || SNAP;
    using G = Geo<NW>;
    using L = FwdLds;
    constexpr int CPT = G::CPT, TPT = G::TPT, JR = ColTile<NW>::JR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const coef = smem + L::COEF_AT;
    float* const ys = smem + L::out(0);

    const auto w = open_row<NW>(a);
    [[maybe_unused]] int slot = -1;
    if constexpr (SLOTS) {
        if (outside_len_window(a, w.ntok)) return;      // (workgroup-uniform, in front of the first barrier and the first tensor or state access)
        slot = state_slot_of(a, w.b, w.ntok);
    }
    [[maybe_unused]] int slot_out = slot;               // SNAP: where the final state goes, -1: nowhere
    [[maybe_unused]] SnapPlan snaps{0, 0};
    [[maybe_unused]] int snap_j = 0, snap_at = 0;       // SNAP: the next snapshot and the token batch that completes it
    if constexpr (SNAP) {
        slot_out = state_slot_out_of(a, w.b, w.ntok, slot);
        snaps = snap_plan(a, w.b, w.ntok);
        snap_at = a.snap_every / TB;
    }
    float uu[CPT];
    load_u<T>(a.u, a.use_u, w, uu);

    const ColTile<NW> t(w.lane, w.wv);
    float S[4][JR];
    zero_tile(S);
    if (SLOTS ? slot >= 0 : a.s0 != nullptr) {
        const long at = (long)(SLOTS ? slot : w.b) * a.s0_bstride + tile_at(w.h, t.j0, t.i0);
        if (a.state_f32) load_tile<float>(a.s0, at, S);
        else load_tile<T>(a.s0, at, S);
    }

    float pr[CPT], pk[CPT], pv[CPT], pew[CPT];
    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const bool valid = p < w.ntok;
        const long idx_r = w.at(p, REV_R), idx_k = w.at(p, REV_K), idx_v = w.at(p, REV_V), idx_w = w.at(p, REV_W);
        zero(pr, pk, pv);
        if (valid) {
            load_at<T>(a.r, idx_r, pr);
            load_at<T>(a.k, idx_k, pk);
            load_at<T>(a.v, idx_v, pv);
        }
        load_ew<T, CPT>(a, idx_w, valid, pew);
    };
    auto stage = [&](int buf) {
        float d[CPT];
#pragma unroll
        for (int c = 0; c < CPT; ++c) d[c] = a.wkind == 2 ? pew[c] : __expf(pew[c]);
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pr, pk, d, pv);
        const float part = token_sum<TPT>(bonus_part(pr, uu, pk));
        if ((w.tid % TPT) == 0) coef[buf * TB + w.spp] = part;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        fwd_tokens<NW>(S, t, in, in + PLANE, in + 3 * PLANE, DecayPlane<4>{in + 2 * PLANE}, coef + buf * TB, ys + buf * PLANE, nb);
    };
    auto snap = [&](int q) {
        if constexpr (SNAP) {
            // (snap_j < count: (snap_j + 1) * snap_every <= ntok, so this batch was a full one; workgroup-uniform)
            if (snap_j < snaps.count && q + 1 == snap_at) {
                const int ss = snap_slot_of(a, snaps, snap_j);
                if (ss >= 0) store_tile<float>(a.s_out, ((long)ss * a.H + w.h) * HEAD * HEAD + (long)t.j0 * HEAD + t.i0, S);
                ++snap_j;
                snap_at += a.snap_every / TB;
            }
        }
    };
    auto emit = [&](int q, int buf) {      // coalesced store of this batch's outputs
        const int p = q * TB + w.spp;
        if (p < w.ntok) {
            const long idx_y = w.at(p, REV_Y);
            float o[CPT];
            lds_load<CPT>(ys + buf * PLANE + w.seg(), o);
            if (a.accumulate) {
                float old[CPT];
                if (a.y_f32) load_at<float>(a.y_f32, idx_y, old);
                else load_at<T>(a.y, idx_y, old);
#pragma unroll
                for (int c = 0; c < CPT; ++c) o[c] += old[c];
            }
            if (a.y_f32 && !a.accumulate) store_at<float>(a.y_f32, idx_y, o);
            else store_at<T>(a.y, idx_y, o);
        }
    };
    run_pipeline<true>(w.ntok, load, stage, Nothing{}, scan, snap, Nothing{}, emit);

    if (SLOTS ? (SNAP ? slot_out : slot) >= 0 : a.s_out != nullptr) {
        const long at = ((long)(SLOTS ? (SNAP ? slot_out : slot) : w.b) * a.H + w.h) * HEAD * HEAD + (long)t.j0 * HEAD + t.i0;
        if (a.state_f32) store_tile<float>(a.s_out, at, S);
        else store_tile<T>(a.s_out, at, S);
    }
    if (a.zero_tail && !a.accumulate) {
        const float z[CPT] = {};
        for (int tk = w.ntok + w.spp; tk < a.T; tk += TB) store_at<T>(a.y, w.tail(tk), z);
    }
}

// =====================================================================================================
// backward sweep S (scan order):  dq_t[i] = sum_j gy_t[j] S_t[i][j]   (cuda/wkv6_cuda.cu:100-109 minus
// its u-term), gr_t = dq_t + u (.) k_t (v_t.gy_t), aux a_t = r_t (.) dq_t, gu += r_t (.) k_t (v_t.gy_t)
// (cuda/wkv6_cuda.cu:106-112).  Lane layout: RowTile (wkv6_scan_stage.h).
// =====================================================================================================
using BwdSLds = Lds<4, false, 1>;      // k,d,v,gy; dq
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void scan_bwd_s_kernel(const ScanArgs a)
{
    using G = Geo<NW>;
    using L = BwdSLds;
    constexpr int CPT = G::CPT, TPT = G::TPT, IR = RowTile<NW>::IR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const dqs = smem + L::out(0);

    const auto w = open_row<NW>(a);
    float uu[CPT];
    load_u<T>(a.u, a.use_u, w, uu);

    const RowTile<NW> t(w.lane, w.wv);
    float S[IR][4];
    zero_tile(S);
    if (a.s0) load_tile<T>(a.s0, (long)w.b * a.s0_bstride + tile_at(w.h, t.j0, t.i0), S);

    float pr[CPT], pk[CPT], pv[CPT], pew[CPT], pgy[CPT];
    float nr[CPT], nk[CPT], nvg = 0.f;                 // values of the batch just written to LDS
    float cr[CPT], ck[CPT], cvg = 0.f;                 // values of the batch being scanned
    float gu_acc[CPT];
    zero(gu_acc, nr, nk, cr, ck);

    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const bool valid = p < w.ntok;
        const long idx_r = w.at(p, REV_R), idx_k = w.at(p, REV_K), idx_v = w.at(p, REV_V), idx_w = w.at(p, REV_W), idx_y = w.at(p, REV_Y);
        zero(pr, pk, pv, pgy);
        if (valid) {
            load_at<T>(a.r, idx_r, pr);
            load_at<T>(a.k, idx_k, pk);
            load_at<T>(a.v, idx_v, pv);
            load_at<T>(a.gy, idx_y, pgy);
        }
        load_ew<T, CPT>(a, idx_w, valid, pew);
    };
    auto stage = [&](int buf) {
        float d[CPT];
#pragma unroll
        for (int c = 0; c < CPT; ++c) d[c] = __expf(pew[c]);
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pk, d, pv, pgy);
        nvg = token_sum<TPT>(dot_part(pv, pgy));
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            nr[c] = pr[c]; nk[c] = pk[c];
            gu_acc[c] = fmaf(pr[c] * pk[c], nvg, gu_acc[c]);
        }
    };
    auto take = [&]() {
        copy(cr, nr); copy(ck, nk);
        cvg = nvg;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        asc_tokens<NW>(S, t, in, in + 2 * PLANE, in + 3 * PLANE, DecayPlane<IR>{in + PLANE}, dqs + buf * PLANE, nb, Nothing{});
    };
    auto emit = [&](int q, int buf) {
        const int p = q * TB + w.spp;
        if (p < w.ntok) {
            const long idx_p = w.at(p, 0), idx_r = w.at(p, REV_R);      // (the scratch is indexed by scan position)
            float dq[CPT], av[CPT], o[CPT];
            lds_load<CPT>(dqs + buf * PLANE + w.seg(), dq);
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                av[c] = cr[c] * dq[c];
                o[c] = fmaf(uu[c] * ck[c], cvg, dq[c]);
            }
            store_at<float>(a.aux, idx_p, av);
            put_at<T>(a.gr, idx_r, o, a.accumulate);
        }
    };
    run_pipeline<true>(w.ntok, load, stage, take, scan, Nothing{}, Nothing{}, emit);

    if (a.gu) store_slot_partial(a.gu, sizeof(T) == 4 || a.part_f32, dqs, w, gu_acc, Nothing{}, Nothing{});
}

// =====================================================================================================
// backward sweep G (reverse scan order):  G <- d_t (.) G + r_t gy_t^T  (cuda/wkv6_cuda.cu:128-132),
//   dk_t[i] = sum_j G[i][j] v_t[j],  gk_t = dk_t + u (.) r_t (v_t.gy_t)          (:126-134)
//   gv_t[j] = sum_i k_t[i] G[i][j] + (sum_i u[i]r_t[i]k_t[i]) gy_t[j]            (:149-157)
//   gw_t = ew_t (.) (sum_{s>t} a_s - sum_{s>=t} b_s),  b_t = k_t (.) dk_t        (replaces :161-227)
//   gs = dL/dS_0 = G after the last step                                          (wkv6state_cuda.cu:172-190)
// Same lane layout as sweep S.
// =====================================================================================================
template <int NW> using BwdGLds = Lds<5, false, 1 + NW + 1>;      // r,k,d,v,gy; dk, the waves' gv parts, delta
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void scan_bwd_g_kernel(const ScanArgs a)
{
    using G_ = Geo<NW>;
    using L = BwdGLds<NW>;
    constexpr int CPT = G_::CPT, TPT = G_::TPT, IR = RowTile<NW>::IR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const dks = smem + L::out(0);
    float* const gvs = smem + L::out(1);                      // [2][NW][TB][ROW]
    float* const dls = smem + L::out(1 + NW);

    const auto w = open_row<NW>(a);
    float uu[CPT];
    load_u<T>(a.u, a.use_u, w, uu);

    const RowTile<NW> t(w.lane, w.wv);
    float Gs[IR][4];
    zero_tile(Gs);

    float pr[CPT], pk[CPT], pv[CPT], pew[CPT], pgy[CPT], pa[CPT];
    // n*: batch just written to LDS; c*: batch being scanned; d*: batch whose gw is still pending
    float nr[CPT], nk[CPT], ngy[CPT], new_[CPT], na[CPT], ncoef = 0.f, nvg = 0.f;
    float cr[CPT], ck[CPT], cgy[CPT], cew[CPT], ca[CPT], ccoef = 0.f, cvg = 0.f;
    float db[CPT], dew[CPT], R[CPT];
    long didx = 0;
    int dbuf = -1;
    bool dvalid = false;
    zero(nr, nk, ngy, new_, na);
    zero(cr, ck, cgy, cew, ca);
    zero(db, dew, R);

    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const bool valid = p < w.ntok;
        const long idx_r = w.at(p, REV_R), idx_k = w.at(p, REV_K), idx_v = w.at(p, REV_V), idx_w = w.at(p, REV_W), idx_y = w.at(p, REV_Y);
        const long idx_p = w.at(p, 0);          // the scratch is indexed by scan position
        zero(pr, pk, pv, pgy, pa);
        if (valid) {
            load_at<T>(a.r, idx_r, pr);
            load_at<T>(a.k, idx_k, pk);
            load_at<T>(a.v, idx_v, pv);
            load_at<T>(a.gy, idx_y, pgy);
            load_at<float>(a.aux, idx_p, pa);
        }
        load_ew<T, CPT>(a, idx_w, valid, pew);
    };
    auto stage = [&](int buf) {
        float d[CPT];
#pragma unroll
        for (int c = 0; c < CPT; ++c) d[c] = __expf(pew[c]);
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pr, pk, d, pv, pgy);
        ncoef = token_sum<TPT>(bonus_part(pr, uu, pk));
        nvg = token_sum<TPT>(dot_part(pv, pgy));
        copy(nr, pr); copy(nk, pk); copy(ngy, pgy); copy(new_, pew); copy(na, pa);
    };
    auto take = [&]() {
        copy(cr, nr); copy(ck, nk); copy(cgy, ngy); copy(cew, new_); copy(ca, na);
        ccoef = ncoef; cvg = nvg;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        adj_tokens<NW>(Gs, t, in, in + PLANE, in + 3 * PLANE, in + 4 * PLANE, DecayPlane<IR>{in + 2 * PLANE}, dks + buf * PLANE,
                       gvs + (buf * NW + w.wv) * PLANE, nb);
    };
    // gw of the pending batch: needs every slot's delta of that batch (written before the last barrier)
    auto finish_gw = [&]() {
        if (dbuf < 0) return;
        const float* const dl = dls + dbuf * PLANE + w.sc0;
        float after[CPT], total[CPT];
        zero(after, total);
#pragma unroll
        for (int pp = TB - 1; pp >= 0; --pp) {       // later scan positions first (fixed order)
            float t_[CPT];
            lds_load<CPT>(dl + pp * ROW, t_);
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                if (pp == w.spp) after[c] = total[c];
                total[c] += t_[c];
            }
        }
        if (dvalid) {
            float o[CPT];
#pragma unroll
            for (int c = 0; c < CPT; ++c) o[c] = (R[c] + after[c] - db[c]) * dew[c];
            put_at<T>(a.gw, didx, o, a.accumulate);
        }
#pragma unroll
        for (int c = 0; c < CPT; ++c) R[c] += total[c];
        dbuf = -1;
    };
    auto emit = [&](int q, int buf) {
        const int p = q * TB + w.spp;
        const bool valid = p < w.ntok;
        const long idx_k = w.at(p, REV_K), idx_v = w.at(p, REV_V), idx_w = w.at(p, REV_W);
        float dk[CPT], gvsum[CPT], dl[CPT];
        lds_load<CPT>(dks + buf * PLANE + w.seg(), dk);
        sum_waves<NW>(gvs + buf * NW * PLANE + w.seg(), gvsum);
        float ogk_[CPT], ogv_[CPT];
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            if (!valid) { dk[c] = 0.f; }
            ogk_[c] = fmaf(uu[c] * cr[c], cvg, dk[c]);
            ogv_[c] = fmaf(ccoef, cgy[c], gvsum[c]);
            db[c] = ck[c] * dk[c];
            dl[c] = ca[c] - db[c];
            dew[c] = cew[c];
        }
        lds_store<CPT>(dls + buf * PLANE + w.seg(), dl);
        dbuf = buf; dvalid = valid; didx = idx_w;
        if (valid) {
            if (a.accumulate) {
                float o1[CPT], o2[CPT];
                load_at<T>(a.gk, idx_k, o1);
                load_at<T>(a.gv, idx_v, o2);
#pragma unroll
                for (int c = 0; c < CPT; ++c) { ogk_[c] += o1[c]; ogv_[c] += o2[c]; }
            }
            store_at<T>(a.gk, idx_k, ogk_);
            store_at<T>(a.gv, idx_v, ogv_);
        }
    };
    // behind the barrier: gw of batch q+1 (its deltas were complete one barrier ago), then batch q's stores
    run_pipeline<false>(w.ntok, load, stage, take, scan, Nothing{}, finish_gw, emit);
    __syncthreads();
    finish_gw();                                       // batch 0

    if (a.gs) {
        const long at = ((long)w.b * a.H + w.h) * HEAD * HEAD + (long)t.j0 * HEAD + t.i0;
        if (sizeof(T) == 4 || a.part_f32) store_tile<float>(a.gs, at, Gs);
        else store_tile<T>(a.gs, at, Gs);
    }
    if (a.zero_tail && !a.accumulate) {
        const float z[CPT] = {};
        for (int tk = w.ntok + w.spp; tk < a.T; tk += TB) {
            const long idx = w.tail(tk);
            store_at<T>(a.gr, idx, z);
            store_at<T>(a.gk, idx, z);
            store_at<T>(a.gv, idx, z);
            store_at<T>(a.gw, idx, z);
        }
    }
}

// ---- device self-test of the cross-lane primitives (tests call it once) ---------------------------
__global__ void selftest_kernel(int* result)
{
    const int lane = threadIdx.x & 63;
    int bad = 0;
    // pseudo-random but exactly representable values
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = (float)((lane * 37 + q * 11) % 101) - 50.f;
    {   // col_reduce against shuffles
        const float got = col_reduce(x);
        const float ref = col_reduce_ref(x, lane >> 4);
        if (got != ref) bad |= 1;
    }
    {   // row_reduce<4>
        const float got = row_reduce(x, lane & 15);
        float t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s = x[q];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
            t[q] = s;
        }
        if (got != pick<4>(t, row_sel<4>(lane & 15))) bad |= 2;
    }
    {   // row_reduce<2>
        const float y2[2] = {x[0], x[3]};
        const float got = row_reduce(y2, lane & 15);
        float t[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float s = y2[q];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
            t[q] = s;
        }
        if (got != pick<2>(t, row_sel<2>(lane & 15))) bad |= 4;
    }
    {   // row_sum16
        float s = x[1];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        if (row_sum16(x[1]) != s) bad |= 8;
    }
    if (bad) atomicOr(result, bad);
}

constexpr int NWAVES = 8;

// the scan forward in its I/O type: plain, or the packed stateful instantiations (SLOTS / SNAP)
template <bool SLOTS, bool SNAP> hipError_t launch_scan_fwd_io(const ScanArgs& a, int io, hipStream_t st)
{
    const dim3 grid(a.B * a.H), block(NWAVES * 64);
    if (io == IO_F32) return launch<scan_fwd_kernel<float, NWAVES, SLOTS, SNAP>>(grid, block, FwdLds::BYTES, st, a);
    if (io == IO_F16) return launch<scan_fwd_kernel<f16_t, NWAVES, SLOTS, SNAP>>(grid, block, FwdLds::BYTES, st, a);
    return launch<scan_fwd_kernel<bf16_t, NWAVES, SLOTS, SNAP>>(grid, block, FwdLds::BYTES, st, a);
}

// sweep S, then sweep G
template <typename T> hipError_t launch_scan_bwd_io(const ScanArgs& a, hipStream_t st)
{
    constexpr auto G = scan_bwd_g_kernel<T, NWAVES>, S = scan_bwd_s_kernel<T, NWAVES>;   // (named in the order the device code lists them)
    const dim3 grid(a.B * a.H), block(NWAVES * 64);
    if (hipError_t e = launch<S>(grid, block, BwdSLds::BYTES, st, a)) return e;
    return launch<G>(grid, block, BwdGLds<NWAVES>::BYTES, st, a);
}

}  // namespace

hipError_t launch_scan_fwd(const ScanArgs& a, int io, hipStream_t st) { return launch_scan_fwd_io<false, false>(a, io, st); }

hipError_t launch_scan_bwd(const ScanArgs& a, bool io_f32, hipStream_t st)
{
    return io_f32 ? launch_scan_bwd_io<float>(a, st) : launch_scan_bwd_io<bf16_t>(a, st);
}

// Packed variable-length rows: the same kernels, addressed through a.tok_off / a.order (one workgroup per (sequence, head)); a reversal
// map (a.rev_n, a.reverse) is read by the sequence index b = a.order[slot] in all three kernels and applies within the sequence
static bool varlen_scan_ok(const ScanArgs& a)
{
    return a.tok_off && a.lens && a.order && !a.accumulate && !a.zero_tail && !a.y_f32;
}
hipError_t launch_scan_fwd_varlen(const ScanArgs& a, bool io_f32, hipStream_t st)
{
    if (!varlen_scan_ok(a)) return hipErrorInvalidValue;
    return launch_scan_fwd(a, io_f32 ? IO_F32 : IO_BF16, st);
}
hipError_t launch_scan_bwd_varlen(const ScanArgs& a, bool io_f32, hipStream_t st)
{
    if (!varlen_scan_ok(a) || !a.aux) return hipErrorInvalidValue;
    return launch_scan_bwd(a, io_f32, st);
}
// Packed stateful inference: the state pool a.s0 == a.s_out (fp32, a.n_slots slots) is addressed through a.state_slot and updated in place
hipError_t launch_scan_fwd_slots(const ScanArgs& a, int io, hipStream_t st)
{
    if (!varlen_scan_ok(a) || !slots_ok(a) || a.reverse || a.rev_n) return hipErrorInvalidValue;
    return launch_scan_fwd_io<true, false>(a, io, st);
}
// ... with the final state in slot a.state_slot_out and the snapshots of wkv6_scan.h: SnapPlan
hipError_t launch_scan_fwd_snap(const ScanArgs& a, int io, hipStream_t st)
{
    if (!varlen_scan_ok(a) || !slots_ok(a) || !snap_ok(a) || a.reverse || a.rev_n) return hipErrorInvalidValue;
    return launch_scan_fwd_io<false, true>(a, io, st);
}

hipError_t launch_selftest(int* result, hipStream_t st) { return launch<selftest_kernel>(dim3(1), dim3(64), 0, st, result); }

}  // namespace wkv6
