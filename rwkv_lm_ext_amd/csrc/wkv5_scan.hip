// Exact-fp32 token-serial WKV5 (static decay) kernels for gfx950.  Design notes: wkv5_scan.h.
#include "wkv5_scan.h"
#include "wkv6_host.h"                 // launch<>, check_shape, to_rc

namespace wkv6 {
namespace {

constexpr int TB = 16;                 // tokens staged per LDS batch
constexpr int ROW = HEAD;              // floats per staged token row
constexpr int NW = 8;                  // waves per workgroup
constexpr int NT = NW * 64;
constexpr int CPT = TB * ROW / NT;     // channels staged per thread (2)
constexpr int TPT = ROW / CPT;         // threads per token (32)
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

// =====================================================================================================
// forward (cuda/wkv5_cuda.cu:25-61).  Wave `wv` owns value columns [8 wv, 8 wv + 8); lane (jb = lane>>4, ib = lane&15)
// owns S[4ib..4ib+3][j0, j0+1] and the four decays of its key rows.
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_fwd_kernel(const Wkv5Args a)
{
    constexpr int JPW = HEAD / NW, JR = JPW / 4;
    static_assert(JR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem;                          // [2][3][TB][ROW]  r,k,v
    float* const coef = smem + 2 * 3 * TB * ROW;      // [2][TB] (64 floats reserved)
    float* const ys = coef + 64;                      // [2][TB][ROW]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const T* const gr_ = reinterpret_cast<const T*>(a.r);
    const T* const gk_ = reinterpret_cast<const T*>(a.k);
    const T* const gv_ = reinterpret_cast<const T*>(a.v);
    T* const gy_ = reinterpret_cast<T*>(a.y);
    const int ntok = a.T;
    const long base = (long)b * a.T * a.C + (long)h * HEAD;

    // staging role
    const int spp = tid / TPT, sc0 = (tid % TPT) * CPT;
    float uu[CPT];
    ion<T, CPT>::load(reinterpret_cast<const T*>(a.u) + h * HEAD + sc0, uu);

    // compute role
    const int jb = lane >> 4, ib = lane & 15;
    const int i0 = ib * 4, j0 = wv * JPW + jb * JR;
    float S[4][JR], d4[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
        float ew_;
        load_decay<T>(a, h * HEAD + i0 + ii, d4[ii], ew_);
#pragma unroll
        for (int jj = 0; jj < JR; ++jj) S[ii][jj] = 0.f;
    }

    float pr[CPT], pk[CPT], pv[CPT];
    auto load_regs = [&](int q) {
        const int p = q * TB + spp;
        const long idx = base + (long)p * a.C + sc0;
#pragma unroll
        for (int c = 0; c < CPT; ++c) { pr[c] = 0.f; pk[c] = 0.f; pv[c] = 0.f; }
        if (p < ntok) {
            ion<T, CPT>::load(gr_ + idx, pr);
            ion<T, CPT>::load(gk_ + idx, pk);
            ion<T, CPT>::load(gv_ + idx, pv);
        }
    };
    auto write_lds = [&](int buf) {
        float* const ib_ = inb + buf * 3 * TB * ROW + spp * ROW + sc0;
        float part = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; ++c) part = fmaf(pr[c] * uu[c], pk[c], part);
        lds_store<CPT>(ib_, pr);
        lds_store<CPT>(ib_ + TB * ROW, pk);
        lds_store<CPT>(ib_ + 2 * TB * ROW, pv);
        part = token_sum<TPT>(part);
        if ((tid % TPT) == 0) coef[buf * TB + spp] = part;
    };

    const int nq = (ntok + TB - 1) / TB;
    load_regs(0);
    write_lds(0);
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const int buf = q & 1;
        if (q + 1 < nq) load_regs(q + 1);
        {   // ---- scan the staged tokens
            const float* const rs = inb + buf * 3 * TB * ROW;
            const float* const ks = rs + TB * ROW;
            const float* const vs = rs + 2 * TB * ROW;
            float* const yb = ys + buf * TB * ROW;
            const int nb = min(TB, ntok - q * TB);

            for (int pp = 0; pp < nb; ++pp) {
                float r4[4], k4[4], vv[JR], yacc[JR];
                lds_load<4>(rs + pp * ROW + i0, r4);
                lds_load<4>(ks + pp * ROW + i0, k4);
                lds_load<2>(vs + pp * ROW + j0, vv);
#pragma unroll
                for (int jj = 0; jj < JR; ++jj) yacc[jj] = 0.f;
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int jj = 0; jj < JR; ++jj) {
                        const float kv = k4[ii] * vv[jj];
                        yacc[jj] = fmaf(r4[ii], S[ii][jj], yacc[jj]);
                        S[ii][jj] = fmaf(S[ii][jj], d4[ii], kv);
                    }
                const float tot = row_reduce(yacc, ib);
                if (ib < JR) {
                    const int jj = row_sel<JR>(ib);
                    yb[pp * ROW + j0 + jj] = fmaf(coef[buf * TB + pp], jj ? vv[1] : vv[0], tot);
                }
            }
        }
        if (q + 1 < nq) write_lds(buf ^ 1);
        __syncthreads();
        {   // ---- coalesced store of this batch's outputs
            const int p = q * TB + spp;
            if (p < ntok) {
                float o[CPT];
                lds_load<2>(ys + buf * TB * ROW + spp * ROW + sc0, o);
                ion<T, CPT>::store(gy_ + base + (long)p * a.C + sc0, o);
            }
        }
    }
}

// =====================================================================================================
// backward, ascending pass: gr, gu, gw (wkv5_scan.h).  Wave `wv` owns key rows [8 wv, 8 wv + 8); lane (irow = lane>>4,
// jl = lane&15) owns S and D = dS/dd at [i0, i0+1][4jl..4jl+3] and the decays of its two key rows.
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_bwd_a_kernel(const Wkv5Args a)
{
    constexpr int IPW = HEAD / NW, IR = IPW / 4;
    static_assert(IR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem;                          // [2][4][TB][ROW]  r,k,v,gy
    float* const dqs = smem + 2 * 4 * TB * ROW;       // [2][TB][ROW]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const T* const gr_ = reinterpret_cast<const T*>(a.r);
    const T* const gk_ = reinterpret_cast<const T*>(a.k);
    const T* const gv_ = reinterpret_cast<const T*>(a.v);
    const T* const ggy = reinterpret_cast<const T*>(a.gy);
    T* const ogr = reinterpret_cast<T*>(a.gr);
    const int ntok = a.T;
    const long base = (long)b * a.T * a.C + (long)h * HEAD;

    const int spp = tid / TPT, sc0 = (tid % TPT) * CPT;
    float uu[CPT];
    ion<T, CPT>::load(reinterpret_cast<const T*>(a.u) + h * HEAD + sc0, uu);

    const int irow = lane >> 4, jl = lane & 15;
    const int i0 = wv * IPW + irow * IR, j0 = jl * 4;
    float S[IR][4], D[IR][4], dd[IR], gd[IR];
#pragma unroll
    for (int ii = 0; ii < IR; ++ii) {
        float ew_;
        load_decay<T>(a, h * HEAD + i0 + ii, dd[ii], ew_);
        gd[ii] = 0.f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) { S[ii][jj] = 0.f; D[ii][jj] = 0.f; }
    }

    float pr[CPT], pk[CPT], pv[CPT], pgy[CPT];
    float nk[CPT], nvg = 0.f;                          // values of the batch just written to LDS
    float ck[CPT], cvg = 0.f;                          // values of the batch being scanned
    float gu_acc[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) { gu_acc[c] = 0.f; nk[c] = ck[c] = 0.f; }

    auto load_regs = [&](int q) {
        const int p = q * TB + spp;
        const long idx = base + (long)p * a.C + sc0;
#pragma unroll
        for (int c = 0; c < CPT; ++c) { pr[c] = 0.f; pk[c] = 0.f; pv[c] = 0.f; pgy[c] = 0.f; }
        if (p < ntok) {
            ion<T, CPT>::load(gr_ + idx, pr);
            ion<T, CPT>::load(gk_ + idx, pk);
            ion<T, CPT>::load(gv_ + idx, pv);
            ion<T, CPT>::load(ggy + idx, pgy);
        }
    };
    auto write_lds = [&](int buf) {
        float* const ib_ = inb + buf * 4 * TB * ROW + spp * ROW + sc0;
        float part = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; ++c) part = fmaf(pv[c], pgy[c], part);
        lds_store<CPT>(ib_, pr);
        lds_store<CPT>(ib_ + TB * ROW, pk);
        lds_store<CPT>(ib_ + 2 * TB * ROW, pv);
        lds_store<CPT>(ib_ + 3 * TB * ROW, pgy);
        nvg = token_sum<TPT>(part);
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            nk[c] = pk[c];
            gu_acc[c] = fmaf(pr[c] * pk[c], nvg, gu_acc[c]);
        }
    };

    const int nq = (ntok + TB - 1) / TB;
    load_regs(0);
    write_lds(0);
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const int buf = q & 1;
#pragma unroll
        for (int c = 0; c < CPT; ++c) ck[c] = nk[c];
        cvg = nvg;
        if (q + 1 < nq) load_regs(q + 1);
        {
            const float* const rs = inb + buf * 4 * TB * ROW;
            const float* const ks = rs + TB * ROW;
            const float* const vs = rs + 2 * TB * ROW;
            const float* const gs = rs + 3 * TB * ROW;
            float* const qb = dqs + buf * TB * ROW;
            const int nb = min(TB, ntok - q * TB);

            for (int pp = 0; pp < nb; ++pp) {
                float rr[IR], kk[IR], v4[4], g4[4], dq[IR];
                lds_load<2>(rs + pp * ROW + i0, rr);
                lds_load<2>(ks + pp * ROW + i0, kk);
                lds_load<4>(vs + pp * ROW + j0, v4);
                lds_load<4>(gs + pp * ROW + j0, g4);
#pragma unroll
                for (int ii = 0; ii < IR; ++ii) {
                    float dD = 0.f;
                    dq[ii] = 0.f;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        dq[ii] = fmaf(g4[jj], S[ii][jj], dq[ii]);
                        dD = fmaf(g4[jj], D[ii][jj], dD);
                        D[ii][jj] = fmaf(D[ii][jj], dd[ii], S[ii][jj]);
                        S[ii][jj] = fmaf(S[ii][jj], dd[ii], kk[ii] * v4[jj]);
                    }
                    gd[ii] = fmaf(rr[ii], dD, gd[ii]);
                }
                const float tot = row_reduce(dq, jl);
                if (jl < IR) qb[pp * ROW + i0 + row_sel<IR>(jl)] = tot;
            }
        }
        if (q + 1 < nq) write_lds(buf ^ 1);
        __syncthreads();
        {
            const int p = q * TB + spp;
            if (p < ntok) {
                float dq[CPT], o[CPT];
                lds_load<2>(dqs + buf * TB * ROW + spp * ROW + sc0, dq);
#pragma unroll
                for (int c = 0; c < CPT; ++c) o[c] = fmaf(uu[c] * ck[c], cvg, dq[c]);
                ion<T, CPT>::store(ogr + base + (long)p * a.C + sc0, o);
            }
        }
    }
    // per-batch partials: gu from the staging threads' accumulators (summed over the TB token slots), gd from the 16 lanes of each key row
    __syncthreads();
    lds_store<CPT>(dqs + spp * ROW + sc0, gu_acc);
#pragma unroll
    for (int ii = 0; ii < IR; ++ii) {
        const float s = row_sum16(gd[ii]);
        if (jl == 0) dqs[TB * ROW + i0 + ii] = s;
    }
    __syncthreads();
    if (tid < HEAD) {
        const long o = (long)b * a.C + h * HEAD + tid;
        if (a.gu) {
            float s = 0.f;
#pragma unroll
            for (int pp = 0; pp < TB; ++pp) s += dqs[pp * ROW + tid];
            store_partial(a.gu, sizeof(T) == 4 || a.part_f32, o, s);
        }
        if (a.gw) {
            float d, ew;
            load_decay<T>(a, h * HEAD + tid, d, ew);
            store_partial(a.gw, sizeof(T) == 4 || a.part_f32, o, ew * d * dqs[TB * ROW + tid]);
        }
    }
}

// =====================================================================================================
// backward, descending pass: gk, gv (wkv5_scan.h).  Same lane layout as the ascending pass.
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(NT) void wkv5_bwd_g_kernel(const Wkv5Args a)
{
    constexpr int IPW = HEAD / NW, IR = IPW / 4;
    static_assert(IR == 2, "lane tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const inb = smem;                                  // [2][4][TB][ROW]  r,k,v,gy
    float* const dks = inb + 2 * 4 * TB * ROW;                // [2][TB][ROW]
    float* const gvs = dks + 2 * TB * ROW;                    // [2][NW][TB][ROW]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const T* const gr_ = reinterpret_cast<const T*>(a.r);
    const T* const gk_ = reinterpret_cast<const T*>(a.k);
    const T* const gv_ = reinterpret_cast<const T*>(a.v);
    const T* const ggy = reinterpret_cast<const T*>(a.gy);
    T* const ogk = reinterpret_cast<T*>(a.gk);
    T* const ogv = reinterpret_cast<T*>(a.gv);
    const int ntok = a.T;
    const long base = (long)b * a.T * a.C + (long)h * HEAD;

    const int spp = tid / TPT, sc0 = (tid % TPT) * CPT;
    float uu[CPT];
    ion<T, CPT>::load(reinterpret_cast<const T*>(a.u) + h * HEAD + sc0, uu);

    const int irow = lane >> 4, jl = lane & 15;
    const int i0 = wv * IPW + irow * IR, j0 = jl * 4;
    float Gs[IR][4], dd[IR];
#pragma unroll
    for (int ii = 0; ii < IR; ++ii) {
        float ew_;
        load_decay<T>(a, h * HEAD + i0 + ii, dd[ii], ew_);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) Gs[ii][jj] = 0.f;
    }

    float pr[CPT], pk[CPT], pv[CPT], pgy[CPT];
    float nr[CPT], ngy[CPT], ncoef = 0.f, nvg = 0.f;   // batch just written to LDS
    float cr[CPT], cgy[CPT], ccoef = 0.f, cvg = 0.f;   // batch being scanned
#pragma unroll
    for (int c = 0; c < CPT; ++c) nr[c] = ngy[c] = cr[c] = cgy[c] = 0.f;

    auto load_regs = [&](int q) {
        const int p = q * TB + spp;
        const long idx = base + (long)p * a.C + sc0;
#pragma unroll
        for (int c = 0; c < CPT; ++c) { pr[c] = 0.f; pk[c] = 0.f; pv[c] = 0.f; pgy[c] = 0.f; }
        if (p < ntok) {
            ion<T, CPT>::load(gr_ + idx, pr);
            ion<T, CPT>::load(gk_ + idx, pk);
            ion<T, CPT>::load(gv_ + idx, pv);
            ion<T, CPT>::load(ggy + idx, pgy);
        }
    };
    auto write_lds = [&](int buf) {
        float* const ib_ = inb + buf * 4 * TB * ROW + spp * ROW + sc0;
        float p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            p1 = fmaf(pr[c] * uu[c], pk[c], p1);
            p2 = fmaf(pv[c], pgy[c], p2);
        }
        lds_store<CPT>(ib_, pr);
        lds_store<CPT>(ib_ + TB * ROW, pk);
        lds_store<CPT>(ib_ + 2 * TB * ROW, pv);
        lds_store<CPT>(ib_ + 3 * TB * ROW, pgy);
        ncoef = token_sum<TPT>(p1);
        nvg = token_sum<TPT>(p2);
#pragma unroll
        for (int c = 0; c < CPT; ++c) { nr[c] = pr[c]; ngy[c] = pgy[c]; }
    };

    const int nq = (ntok + TB - 1) / TB;
    load_regs(nq - 1);
    write_lds((nq - 1) & 1);
    __syncthreads();
    for (int q = nq - 1; q >= 0; --q) {
        const int buf = q & 1;
#pragma unroll
        for (int c = 0; c < CPT; ++c) { cr[c] = nr[c]; cgy[c] = ngy[c]; }
        ccoef = ncoef; cvg = nvg;
        if (q > 0) load_regs(q - 1);
        {
            const float* const rs = inb + buf * 4 * TB * ROW;
            const float* const ks = rs + TB * ROW;
            const float* const vs = rs + 2 * TB * ROW;
            const float* const gs = rs + 3 * TB * ROW;
            float* const kb = dks + buf * TB * ROW;
            float* const vb = gvs + (buf * NW + wv) * TB * ROW;
            const int nb = min(TB, ntok - q * TB);
            for (int pp = nb - 1; pp >= 0; --pp) {
                float rr[IR], kk[IR], v4[4], g4[4], gkp[IR], gvp[4];
                lds_load<2>(rs + pp * ROW + i0, rr);
                lds_load<2>(ks + pp * ROW + i0, kk);
                lds_load<4>(vs + pp * ROW + j0, v4);
                lds_load<4>(gs + pp * ROW + j0, g4);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) gvp[jj] = 0.f;
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
                const float dk = row_reduce(gkp, jl);
                if (jl < IR) kb[pp * ROW + i0 + row_sel<IR>(jl)] = dk;
                const float gvt = col_reduce(gvp);
                vb[pp * ROW + j0 + col_sel(irow)] = gvt;
            }
        }
        if (q > 0) write_lds(buf ^ 1);
        __syncthreads();
        {
            const int p = q * TB + spp;
            if (p < ntok) {
                float dk[CPT], gvsum[CPT], ogk_[CPT], ogv_[CPT];
                lds_load<2>(dks + buf * TB * ROW + spp * ROW + sc0, dk);
#pragma unroll
                for (int c = 0; c < CPT; ++c) gvsum[c] = 0.f;
#pragma unroll
                for (int w_ = 0; w_ < NW; ++w_) {      // fixed order over the waves' partial sums
                    float t2[CPT];
                    lds_load<2>(gvs + (buf * NW + w_) * TB * ROW + spp * ROW + sc0, t2);
#pragma unroll
                    for (int c = 0; c < CPT; ++c) gvsum[c] += t2[c];
                }
#pragma unroll
                for (int c = 0; c < CPT; ++c) {
                    ogk_[c] = fmaf(uu[c] * cr[c], cvg, dk[c]);
                    ogv_[c] = fmaf(ccoef, cgy[c], gvsum[c]);
                }
                const long idx = base + (long)p * a.C + sc0;
                ion<T, CPT>::store(ogk + idx, ogk_);
                ion<T, CPT>::store(ogv + idx, ogv_);
            }
        }
    }
}

constexpr size_t LDS_FWD = (2 * 3 * TB * ROW + 64 + 2 * TB * ROW) * sizeof(float);
constexpr size_t LDS_BWD_A = (2 * 4 * TB * ROW + 2 * TB * ROW) * sizeof(float);
constexpr size_t LDS_BWD_G = (2 * 4 * TB * ROW + 2 * TB * ROW + 2 * NW * TB * ROW) * sizeof(float);

template <typename T> hipError_t launch_bwd(const Wkv5Args& a, hipStream_t st)
{
    static_assert(LDS_BWD_G > 64 * 1024 && LDS_BWD_G <= 160 * 1024, "the descending pass needs the large LDS window");
    constexpr auto G = wkv5_bwd_g_kernel<T>, A = wkv5_bwd_a_kernel<T>;   // (named in the order the device code lists them)
    const dim3 grid(a.B * a.H), block(NT);
    if (hipError_t e = launch<A>(grid, block, LDS_BWD_A, st, a)) return e;
    return launch<G>(grid, block, LDS_BWD_G, st, a);
}

}  // namespace

hipError_t launch_wkv5_fwd(const Wkv5Args& a, bool io_f32, hipStream_t st)
{
    const dim3 grid(a.B * a.H), block(NT);
    return io_f32 ? launch<wkv5_fwd_kernel<float>>(grid, block, LDS_FWD, st, a) : launch<wkv5_fwd_kernel<bf16_t>>(grid, block, LDS_FWD, st, a);
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
