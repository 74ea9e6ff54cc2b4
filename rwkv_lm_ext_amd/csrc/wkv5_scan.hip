// Exact-fp32 token-serial WKV5 (static decay) kernels for gfx950.  Design notes: wkv5_scan.h; the staging pipeline they share with WKV6:
// wkv6_scan_stage.h.
#include "wkv6_scan_stage.h"
#include "wkv6_host.h"                 // launch<>, check_shape, to_rc

namespace wkv6 {
namespace {

constexpr int NW = 8;                  // waves per workgroup
constexpr int NT = Geo<NW>::NT;
constexpr int CPT = Geo<NW>::CPT;      // channels staged per thread (2)
constexpr int TPT = Geo<NW>::TPT;      // threads per token (32)
static_assert(CPT == 2 && TPT == 32, "staging geometry");

// decay d and ew = -exp(w) of channel hc: once per lane, in front of the token loops.  Formed in fp64 and rounded once: a
// relative error e of d becomes t e on a contribution t tokens back, and slow channels (w = -6: d = 0.9975) remember hundreds
// of tokens, so the fast exp's few ulps would show in fp32 I/O; at once per lane the fp64 routine costs nothing.
template <typename T> __device__ __forceinline__ void load_decay(const Wkv5Args& a, int hc, float& d, float& ew)
{
    if (a.wkind == 1) {
        const double e = exp((double)ion<T, CPT>::load1(reinterpret_cast<const T*>(a.w) + hc));
        ew = -(float)e;
        d = (float)exp(-e);
    } else {
        d = reinterpret_cast<const float*>(a.w)[hc];
        ew = a.ew ? a.ew[hc] : 0.f;
    }
}
// ... of the N key rows i0.. of head h that a lane keeps for the whole row
template <typename T, int N> __device__ __forceinline__ void load_decays(const Wkv5Args& a, int h, int i0, float (&d)[N])
{
#pragma unroll
    for (int ii = 0; ii < N; ++ii) {
        float ew_;
        load_decay<T>(a, h * HEAD + i0 + ii, d[ii], ew_);
    }
}

// =====================================================================================================
// forward (cuda/wkv5_cuda.cu:25-61).  Lane layout: ColTile (wkv6_scan_stage.h); a lane keeps the four decays of its key rows.
// =====================================================================================================
using FwdLds = Lds<3, true, 1>;        // r,k,v; coef; y
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_fwd_kernel(const Wkv5Args a)
{
    using L = FwdLds;
    constexpr int JR = ColTile<NW>::JR;
    static_assert(JR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const coef = smem + L::COEF_AT;
    float* const ys = smem + L::out(0);

    const auto w = open_row<NW>(a);
    float uu[CPT];
    load_u<T>(a.u, 1, w, uu);

    const ColTile<NW> t(w.lane, w.wv);
    float S[4][JR], d4[4];
    load_decays<T>(a, w.h, t.i0, d4);
    zero_tile(S);

    float pr[CPT], pk[CPT], pv[CPT];
    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const long idx = w.at(p, 0);
        zero(pr, pk, pv);
        if (p < w.ntok) {
            load_at<T>(a.r, idx, pr);
            load_at<T>(a.k, idx, pk);
            load_at<T>(a.v, idx, pv);
        }
    };
    auto stage = [&](int buf) {
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pr, pk, pv);
        const float part = token_sum<TPT>(bonus_part(pr, uu, pk));
        if ((w.tid % TPT) == 0) coef[buf * TB + w.spp] = part;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        fwd_tokens<NW>(S, t, in, in + PLANE, in + 2 * PLANE, DecayRegs<4>{d4}, coef + buf * TB, ys + buf * PLANE, nb);
    };
    auto emit = [&](int q, int buf) {      // coalesced store of this batch's outputs
        const int p = q * TB + w.spp;
        if (p < w.ntok) {
            float o[CPT];
            lds_load<CPT>(ys + buf * PLANE + w.seg(), o);
            store_at<T>(a.y, w.at(p, 0), o);
        }
    };
    run_pipeline<true>(w.ntok, load, stage, Nothing{}, scan, Nothing{}, Nothing{}, emit);
}

// =====================================================================================================
// backward, ascending pass: gr, gu, gw (wkv5_scan.h).  Lane layout: RowTile (wkv6_scan_stage.h); a lane owns S and D = dS/dd at
// [i0, i0+1][4jl..4jl+3] and the decays of its two key rows.
// =====================================================================================================
using BwdALds = Lds<4, false, 1>;      // r,k,v,gy; dq
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_bwd_a_kernel(const Wkv5Args a)
{
    using L = BwdALds;
    constexpr int IR = RowTile<NW>::IR;
    static_assert(IR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const dqs = smem + L::out(0);

    const auto w = open_row<NW>(a);
    float uu[CPT];
    load_u<T>(a.u, 1, w, uu);

    const RowTile<NW> t(w.lane, w.wv);
    float S[IR][4], D[IR][4], dd[IR], gd[IR];
    load_decays<T>(a, w.h, t.i0, dd);
    zero(gd);
    zero_tile(S);
    zero_tile(D);

    float pr[CPT], pk[CPT], pv[CPT], pgy[CPT];
    float nk[CPT], nvg = 0.f;                          // values of the batch just written to LDS
    float ck[CPT], cvg = 0.f;                          // values of the batch being scanned
    float gu_acc[CPT];
    zero(gu_acc, nk, ck);

    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const long idx = w.at(p, 0);
        zero(pr, pk, pv, pgy);
        if (p < w.ntok) {
            load_at<T>(a.r, idx, pr);
            load_at<T>(a.k, idx, pk);
            load_at<T>(a.v, idx, pv);
            load_at<T>(a.gy, idx, pgy);
        }
    };
    auto stage = [&](int buf) {
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pr, pk, pv, pgy);
        nvg = token_sum<TPT>(dot_part(pv, pgy));
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            nk[c] = pk[c];
            gu_acc[c] = fmaf(pr[c] * pk[c], nvg, gu_acc[c]);
        }
    };
    auto take = [&]() {
        copy(ck, nk);
        cvg = nvg;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        // WKV5's own term, on the state before the update:  gd[i] += r_t[i] sum_j gy_t[j] D_t[i][j],  D <- d (.) D + S
        auto d_term = [&](int pp, const float (&g4)[4]) {
            float rr[IR];
            lds_load<IR>(in + pp * ROW + t.i0, rr);
#pragma unroll
            for (int ii = 0; ii < IR; ++ii) {
                float dD = 0.f;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    dD = fmaf(g4[jj], D[ii][jj], dD);
                    D[ii][jj] = fmaf(D[ii][jj], dd[ii], S[ii][jj]);
                }
                gd[ii] = fmaf(rr[ii], dD, gd[ii]);
            }
        };
        asc_tokens<NW>(S, t, in + PLANE, in + 2 * PLANE, in + 3 * PLANE, DecayRegs<IR>{dd}, dqs + buf * PLANE, nb, d_term);
    };
    auto emit = [&](int q, int buf) {
        const int p = q * TB + w.spp;
        if (p < w.ntok) {
            float dq[CPT], o[CPT];
            lds_load<CPT>(dqs + buf * PLANE + w.seg(), dq);
#pragma unroll
            for (int c = 0; c < CPT; ++c) o[c] = fmaf(uu[c] * ck[c], cvg, dq[c]);
            store_at<T>(a.gr, w.at(p, 0), o);
        }
    };
    run_pipeline<true>(w.ntok, load, stage, take, scan, Nothing{}, Nothing{}, emit);

    // per-batch partials: gu from the staging threads' accumulators, gd from the 16 lanes of each key row (in the plane behind gu's)
    auto stage_gd = [&]() {
#pragma unroll
        for (int ii = 0; ii < IR; ++ii) {
            const float s = row_sum16(gd[ii]);
            if (t.jl == 0) dqs[PLANE + t.i0 + ii] = s;
        }
    };
    auto store_gw = [&](long o) {
        if (a.gw) {
            float d, ew;
            load_decay<T>(a, w.h * HEAD + w.tid, d, ew);
            store_partial(a.gw, sizeof(T) == 4 || a.part_f32, o, ew * d * dqs[PLANE + w.tid]);
        }
    };
    store_slot_partial(a.gu, sizeof(T) == 4 || a.part_f32, dqs, w, gu_acc, stage_gd, store_gw);
}

// =====================================================================================================
// backward, descending pass: gk, gv (wkv5_scan.h).  Same lane layout as the ascending pass.
// =====================================================================================================
using BwdGLds = Lds<4, false, 1 + NW>;     // r,k,v,gy; dk, the waves' gv parts
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_bwd_g_kernel(const Wkv5Args a)
{
    using L = BwdGLds;
    constexpr int IR = RowTile<NW>::IR;
    static_assert(IR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem + L::IN;
    float* const dks = smem + L::out(0);
    float* const gvs = smem + L::out(1);                      // [2][NW][TB][ROW]

    const auto w = open_row<NW>(a);
    float uu[CPT];
    load_u<T>(a.u, 1, w, uu);

    const RowTile<NW> t(w.lane, w.wv);
    float Gs[IR][4], dd[IR];
    load_decays<T>(a, w.h, t.i0, dd);
    zero_tile(Gs);

    float pr[CPT], pk[CPT], pv[CPT], pgy[CPT];
    float nr[CPT], ngy[CPT], ncoef = 0.f, nvg = 0.f;   // batch just written to LDS
    float cr[CPT], cgy[CPT], ccoef = 0.f, cvg = 0.f;   // batch being scanned
    zero(nr, ngy, cr, cgy);

    auto load = [&](int q) {
        const int p = q * TB + w.spp;
        const long idx = w.at(p, 0);
        zero(pr, pk, pv, pgy);
        if (p < w.ntok) {
            load_at<T>(a.r, idx, pr);
            load_at<T>(a.k, idx, pk);
            load_at<T>(a.v, idx, pv);
            load_at<T>(a.gy, idx, pgy);
        }
    };
    auto stage = [&](int buf) {
        stage_planes<CPT>(inb + buf * L::BUF + w.seg(), pr, pk, pv, pgy);
        ncoef = token_sum<TPT>(bonus_part(pr, uu, pk));
        nvg = token_sum<TPT>(dot_part(pv, pgy));
        copy(nr, pr); copy(ngy, pgy);
    };
    auto take = [&]() {
        copy(cr, nr); copy(cgy, ngy);
        ccoef = ncoef; cvg = nvg;
    };
    auto scan = [&](int, int buf, int nb) {
        const float* const in = inb + buf * L::BUF;
        adj_tokens<NW>(Gs, t, in, in + PLANE, in + 2 * PLANE, in + 3 * PLANE, DecayRegs<IR>{dd}, dks + buf * PLANE,
                       gvs + (buf * NW + w.wv) * PLANE, nb);
    };
    auto emit = [&](int q, int buf) {
        const int p = q * TB + w.spp;
        if (p < w.ntok) {
            float dk[CPT], gvsum[CPT], ogk_[CPT], ogv_[CPT];
            lds_load<CPT>(dks + buf * PLANE + w.seg(), dk);
            sum_waves<NW>(gvs + buf * NW * PLANE + w.seg(), gvsum);
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                ogk_[c] = fmaf(uu[c] * cr[c], cvg, dk[c]);
                ogv_[c] = fmaf(ccoef, cgy[c], gvsum[c]);
            }
            const long idx = w.at(p, 0);
            store_at<T>(a.gk, idx, ogk_);
            store_at<T>(a.gv, idx, ogv_);
        }
    };
    run_pipeline<false>(w.ntok, load, stage, take, scan, Nothing{}, Nothing{}, emit);
}

template <typename T> hipError_t launch_bwd(const Wkv5Args& a, hipStream_t st)
{
    static_assert(BwdGLds::BYTES > 64 * 1024 && BwdGLds::BYTES <= 160 * 1024, "the descending pass needs the large LDS window");
    constexpr auto G = wkv5_bwd_g_kernel<T>, A = wkv5_bwd_a_kernel<T>;   // (named in the order the device code lists them)
    const dim3 grid(a.B * a.H), block(NT);
    if (hipError_t e = launch<A>(grid, block, BwdALds::BYTES, st, a)) return e;
    return launch<G>(grid, block, BwdGLds::BYTES, st, a);
}

}  // namespace

hipError_t launch_wkv5_fwd(const Wkv5Args& a, bool io_f32, hipStream_t st)
{
    const dim3 grid(a.B * a.H), block(NT);
    return io_f32 ? launch<wkv5_fwd_kernel<float>>(grid, block, FwdLds::BYTES, st, a) : launch<wkv5_fwd_kernel<bf16_t>>(grid, block, FwdLds::BYTES, st, a);
}

hipError_t launch_wkv5_bwd(const Wkv5Args& a, bool io_f32, hipStream_t st)
{
    return io_f32 ? launch_bwd<float>(a, st) : launch_bwd<bf16_t>(a, st);
}

}  // namespace wkv6

using namespace wkv6;

// ---- the entry points (include/wkv6_amd.h).  Exact token-serial kernels only; no workspace
extern "C" {

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

}  // extern "C"
