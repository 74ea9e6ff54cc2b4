// Per-sequence LoRA adapters on a packed batch (include/wkv6_amd.h: wkv6_lora_packed_bf16), hand-written for gfx950: the segmented
// low-rank matmul behind a base GEMM.  Every sequence of the batch names its adapter on the device; a row t of sequence s with
// a = adapter[s] inside the pool gets
//     xa[t,j] = bf16( sum_k x[t,k] A[a,j,k] )                                  ("shrink",  A_pool bf16 [n_adapters,R,K])
//     y[t,n]  = bf16( fmaf(scale[a], sum_j xa[t,j] B[a,n,j], float(y[t,n])) )   ("expand",  B_pool bf16 [n_adapters,N,R])
// and every other row keeps its bits.  Two launches in stream order with the bf16 xa [total_T,R] between them in the workspace.
//
// Both kernels work on the 16-row MFMA tile of wkv6_tile16.h (lane roles, K walk, expand tile), shared with wkv6_lowrank.hip; the token
// operand is x[row] / xa[row], the weight operand A[a,j] / B[a,n].  This file's own are the adapter groups:
//
// A tile may hold up to 16 adapters (decode tokens).  Each wave finds the adapter of the tile's 16 rows (bisection in cu_seqlens, the
// rule of the packed kernels of wkv6_mix.hip; the adapter number is judged before anything is addressed with it) and walks the GROUPS of
// rows that share an adapter: one pass of MFMAs per group with that adapter's matrices, the token operand of rows outside the group a
// literal zero, and only the lanes of the group's rows keep (select by lane) what the pass computed.  Nothing is masked by a multiply:
// a NaN in adapter a's matrices stays in the discarded columns of a's pass.
#include <climits>
#include "wkv6_host.h"                 // launch<>, to_rc, overlap
#include "wkv6_tile16.h"

namespace wkv6 {
namespace {

constexpr int SHRINK_WAVES = 8;        // waves of a shrink workgroup: they share the (group, K chunk) work items of one tile
constexpr int SHRINK_CHUNKS = 4;       // K is cut into min(4, K / 32) interleaved chunks of 32-wide steps: fixed by K alone
constexpr int EXPAND_WAVES = 4;        // waves of an expand workgroup: wave w serves the tile's groups w, w + 4, ...
constexpr int EXPAND_GRID_Y = 16;      // at most this many workgroups share a tile's N / 64 column blocks

struct LoraArgs {
    int total_T, n_seq, K, N, R, n_adapters;
    const int* cu;            // [n_seq + 1]
    const int* adapter;       // [n_seq]
    const bf16_t* x;          // [total_T,K]
    const bf16_t* A;          // [n_adapters,R,K]
    const bf16_t* B;          // [n_adapters,N,R]
    const float* scale;       // [n_adapters]
    bf16_t* y;                // [total_T,N]
    bf16_t* xa;               // [total_T,R]  (workspace)
};

// The packed-argument gate of the two launchers, kin of packed_arrays_ok (wkv6_scan.h): the int arrays and every tensor are there, the
// sizes are ones the kernels have (the API refuses everything else with its own code before it gets here).
inline bool lora_arrays_ok(const LoraArgs& a) { return a.cu && a.adapter && a.x && a.A && a.B && a.scale && a.y && a.xa; }
inline bool lora_sizes_ok(const LoraArgs& a)
{
    return a.total_T >= 1 && a.n_seq >= 1 && a.n_adapters >= 1 && a.K >= 64 && a.K % 64 == 0 && a.N >= 64 && a.N % 64 == 0 &&
           (a.R == 8 || a.R == 16 || a.R == 32 || a.R == 64);
}

// Adapter of packed row `row`, -1: the row is not served (outside [0,total_T), in no sequence, or its sequence's adapter lies outside the
// pool).  Row t belongs to sequence s = seq_of_row(t) (wkv6_common.h) when a_s <= t < b_s with the bounds clamped into [0,total_T]; the
// adapter number is judged here, before any address is formed from it.
__device__ __forceinline__ int row_adapter(const LoraArgs& a, long row)
{
    if (row >= a.total_T) return -1;
    const int s = seq_of_row(a.cu, a.n_seq, row);
    if (s < 0) return -1;
    if (row < clampi(a.cu[s], 0, a.total_T) || row >= clampi(a.cu[s + 1], 0, a.total_T)) return -1;
    const int ad = a.adapter[s];
    return ad >= 0 && ad < a.n_adapters ? ad : -1;
}

// Walks the groups of equal adapter among the tile's 16 rows (`mine`: the adapter of row lane & 15, -1: none; the four 16-lane rows of
// the wave hold copies).  f(index, adapter, in_group): adapter is wave-uniform, in_group per lane.
template <typename F> __device__ __forceinline__ void for_each_group(int mine, F f)
{
    unsigned todo = (unsigned)__ballot(mine >= 0) & 0xffffu;
    for (int gi = 0; todo; ++gi) {
        const int first = __ffs(todo) - 1;
        const int ad = __builtin_amdgcn_readlane(mine, first);
        const bool in = mine == ad;
        todo &= ~((unsigned)__ballot(in) & 0xffffu);
        f(gi, ad, in);
    }
}

// ---- shrink: xa = bf16(x A[a]^T).  One workgroup per (tile of 16 rows, 16 columns j of xa); MFMA rows = j, columns = tokens, so lane
// (c, g) ends with xa[row c][j0 + 4g .. + 3].  The work items of a tile are (group, K chunk of for_each_kstep) and go round the waves.  An
// item chains its steps in one fp32 accumulator and leaves it in LDS (a token is in one group only, so the items never meet); after the
// barrier wave 0 adds a token's chunks (sum_chunks), rounds once and stores.  Rows of R that do not exist (R = 8: j = 8..15) are literal
// zeros, never loaded; a token outside the group, or past total_T, is a literal zero too.
template <int R>
__global__ void __launch_bounds__(SHRINK_WAVES * 64) lora_shrink_kernel(const LoraArgs a)
{
    __shared__ __align__(16) float part[SHRINK_CHUNKS][TILE][16];     // (written and read four at a time)
    const Lane16 ln;
    const int wave = ln.wave, c = ln.c, g = ln.g;
    const long row = (long)blockIdx.x * TILE + c;
    const int j = blockIdx.y * 16 + c;                   // the pool row this lane feeds
    const bool j_ok = j < R;
    const int mine = row_adapter(a, row);
    const int nsteps = a.K / 32, nch = min(SHRINK_CHUNKS, nsteps);
    const bf16_t* xr = a.x + row * a.K + 8 * g;          // (formed, not dereferenced, for rows that are not served)
    int item = 0;
    for_each_group(mine, [&](int, int ad, bool in) {
        const bf16_t* ar = a.A + ((long)ad * R + (j_ok ? j : 0)) * a.K + 8 * g;
        for (int q = 0; q < nch; ++q, ++item) {
            if (item % SHRINK_WAVES != wave) continue;
            f4v acc = {0.f, 0.f, 0.f, 0.f};
            b8v af[4], xf[4];
            for_each_kstep(q, nch, nsteps,
                           [&](int u, int k) {
                               af[u] = j_ok ? load8(ar + k) : zero8();
                               xf[u] = in ? load8(xr + k) : zero8();
                           },
                           [&](int u) { acc = mfma32(af[u], xf[u], acc); });
            if (in) *reinterpret_cast<float4*>(&part[q][c][4 * g]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
    });
    __syncthreads();
    const int j0 = blockIdx.y * 16 + 4 * g;
    if (wave == 0 && mine >= 0 && j0 < R) {
        const auto sum = sum_chunks(part, nch, c, g);
        *reinterpret_cast<v2u*>(a.xa + row * R + j0) = v2u{pack_bf2(sum[0], sum[1]), pack_bf2(sum[2], sum[3])};
    }
}

// ---- expand: y = bf16(fmaf(scale[a], xa B[a]^T, y)).  One workgroup per tile of 16 rows and share of the N / 64 column blocks; wave w
// serves the tile's groups w, w + 4, ...  MFMA rows = n, columns = tokens, contraction over j: one step of 32 for R <= 32 (for R = 8 and
// 16 the lanes whose 8 j lie past R hold literal zeros in both operands), two for R = 64.  The tile and its column map are expand_pass's
// (wkv6_tile16.h): the read-modify-write of y is two 16-byte accesses per lane.  Only the lanes of the group's rows touch y.
template <int R>
__global__ void __launch_bounds__(EXPAND_WAVES * 64) lora_expand_kernel(const LoraArgs a)
{
    constexpr int STEPS = R == 64 ? 2 : 1;
    const Lane16 ln;
    const int wave = ln.wave, c = ln.c, g = ln.g;
    const long row = (long)blockIdx.x * TILE + c;
    const int mine = row_adapter(a, row);
    const bool j_ok = 8 * g < R;                         // (R >= 32: every lane)
    const int nblocks = a.N / EXPAND_NB;
    for_each_group(mine, [&](int gi, int ad, bool in) {
        if (gi % EXPAND_WAVES != wave) return;
        const float sc = a.scale[ad];
        b8v xf[STEPS];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) xf[st] = in && j_ok ? load8(a.xa + row * R + 32 * st + 8 * g) : zero8();
        const bf16_t* bp = a.B + (long)ad * a.N * R + 8 * g;
        for (int nb = blockIdx.y; nb < nblocks; nb += gridDim.y) {
            const int n0 = nb * EXPAND_NB;
            f4v acc[4];
            expand_pass<R, STEPS>(acc, bp, j_ok, n0, c, xf);
            if (in) {
                v4u* yp = reinterpret_cast<v4u*>(a.y + row * a.N + n0 + 16 * g);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const v4u old = yp[h];
                    yp[h] = expand_half(acc, h, [&](int p, float lo, float hi) {
                        return pack_bf2(fmaf(sc, lo, bf_lo(old[p])), fmaf(sc, hi, bf_hi(old[p])));
                    });
                }
            }
        }
    });
}

template <int R> hipError_t launch_lora(const LoraArgs& a, hipStream_t st)
{
    const unsigned tiles = (unsigned)(((long)a.total_T + TILE - 1) / TILE);
    if (hipError_t e = launch<lora_shrink_kernel<R>>(dim3(tiles, (R + 15) / 16), dim3(SHRINK_WAVES * 64), 0, st, a)) return e;
    return launch<lora_expand_kernel<R>>(dim3(tiles, min(a.N / EXPAND_NB, EXPAND_GRID_Y)), dim3(EXPAND_WAVES * 64), 0, st, a);
}

// shrink, then expand, in stream order
hipError_t launch_lora_packed(const LoraArgs& a, hipStream_t st)
{
    if (!lora_arrays_ok(a) || !lora_sizes_ok(a)) return hipErrorInvalidValue;
    switch (a.R) {
    case 8: return launch_lora<8>(a, st);
    case 16: return launch_lora<16>(a, st);
    case 32: return launch_lora<32>(a, st);
    default: return launch_lora<64>(a, st);
    }
}

bool rank_ok(int R) { return R == 8 || R == 16 || R == 32 || R == 64; }

}  // namespace
}  // namespace wkv6

using namespace wkv6;

extern "C" {

size_t wkv6_lora_packed_workspace_bytes(long total_T, int R)
{
    if (total_T < 1 || total_T > 0x7fffffffL || !rank_ok(R)) return 0;
    return ((size_t)total_T * R * 2 + 255) & ~(size_t)255;
}

int wkv6_lora_packed_bf16(long total_T, int n_seq, int K, int N, int R, int n_adapters, const int* cu_seqlens, const int* adapter,
                          const void* x, const void* A_pool, const void* B_pool, const float* scale, void* y, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    // the order of the refusals is part of the contract (include/wkv6_amd.h)
    if (total_T < 1 || n_seq < 1 || n_adapters < 1 || R < 1) return WKV6_EINVAL;
    if (K < 64 || K % 64 || K > 16384 || N < 64 || N % 64 || N > 16384) return WKV6_EINVAL;
    if (!rank_ok(R) || total_T > 0x7fffffffL) return WKV6_EUNSUPPORTED;           // cu_seqlens is int32
    if (!cu_seqlens || !adapter || !x || !A_pool || !B_pool || !scale || !y || !workspace) return WKV6_ENULL;
    if (((uintptr_t)x | (uintptr_t)A_pool | (uintptr_t)B_pool | (uintptr_t)y | (uintptr_t)workspace) & 15) return WKV6_EINVAL;
    if (((uintptr_t)cu_seqlens | (uintptr_t)adapter | (uintptr_t)scale) & 3) return WKV6_EINVAL;
    const size_t y_bytes = (size_t)total_T * N * 2, need = wkv6_lora_packed_workspace_bytes(total_T, R);
    if (overlap(y, y_bytes, x, (size_t)total_T * K * 2) || overlap(y, y_bytes, A_pool, (size_t)n_adapters * R * K * 2) ||
        overlap(y, y_bytes, B_pool, (size_t)n_adapters * N * R * 2))
        return WKV6_EINVAL;
    if (workspace_bytes < need) return WKV6_EWORKSPACE;
    LoraArgs a = {};
    a.total_T = (int)total_T; a.n_seq = n_seq; a.K = K; a.N = N; a.R = R; a.n_adapters = n_adapters;
    a.cu = cu_seqlens; a.adapter = adapter;
    a.x = (const bf16_t*)x; a.A = (const bf16_t*)A_pool; a.B = (const bf16_t*)B_pool; a.scale = scale;
    a.y = (bf16_t*)y; a.xa = (bf16_t*)workspace;
    const hipError_t e = launch_lora_packed(a, (hipStream_t)stream);
    return to_rc(e);
}

}  // extern "C"
