// Beam-search candidate selection (include/wkv6_amd.h: rwkv6_beam_candidates_*), hand-written for gfx950: from the logits rows of a packed
// decode step and the beams' running scores, the K best (parent row, token) continuations of every request by cumulative log-probability.
// The header states the operation; this is how it is done.  Two launches.
//
// Row kernel, one workgroup of 1024 threads (16 waves) per row, on the streamed-row radix selection of wkv6_rows.h that the sampler
// (wkv6_sample.hip) uses too: every pass streams the row again as 16-byte loads (after the first from L2 / Infinity Cache) and recomputes
// the score, because the repetition penalty makes the score non-monotone in the logit.  Pass A: is the row sound, and m = max z.  Pass B: the softmax
// denominator as a sum of the integers floor(exp(z - m) * 2^46) -- exact, so the order in which waves arrive cannot change it and a row has
// the same bits alone or in a batch; L = log of it, once per row, in double.  Then the row's K best scores by radix selection over the
// monotone 32-bit key of the score -- four passes of 8 bits, most significant first, one 256-bin COUNT histogram in LDS -- the ties at the
// boundary cut by two more passes over the token id where there are more than fit.  A last pass collects the at most K winners in LDS,
// one wave ranks them, and they leave as a sorted list.  The row is never sorted; nothing of size V is written.
//
// Merge kernel, one wave per group: the rows' lists (at most 64 x K entries) are copied to LDS, lane l owns the list of the group's row l,
// and K rounds of a wave arg-max over the list heads give the group's candidates in order.  Exact: the group's K best lie in the union of
// its rows' K best.  Equal scores fall to the lower row (the arg-max carries 63 - lane under the key), within a row to the lower token
// (the order of the list).
#include <cmath>
#include "wkv6_beam.h"
#include "wkv6_rows.h"                 // the row walker, the radix selection, block_reduce
#include "wkv6_host.h"                 // to_rc, align_up, overlap

// the same expression must give the same bits wherever it is inlined (the score is formed again on every pass)
#pragma clang fp contract(off)

namespace wkv6 {
namespace {

// ---- what a row's scores are made of
struct Row {
    const float* occ;         // the occurrence row, null: no penalty on this row
    int V, nch;               // tokens, chunks of 8
    float m, L, cum, pen;
};

// steps 3 to 5 of the definition; -inf: no candidate.  -0 becomes +0 (equal values, one key).
__device__ __forceinline__ float score_of(float x, float o, const Row& r)
{
    if (!(x > NEG_INF)) return NEG_INF;
    float lp = (x - r.m) - r.L;
    if (r.occ && o > 0.f) {
        lp = lp < 0.f ? lp * r.pen : lp / r.pen;
        if (lp != lp) lp = 0.f;                              // 0 / 0: a log-probability of 0 under a penalty of 0
    }
    float s = r.cum + lp;
    if (s == 0.f) s = 0.f;
    return s;
}

// f(n, x, o) for every token of the row, four chunks' loads in flight (for_each_row_token); a row without a penalty loads no occurrences
constexpr int BATCH = 4;
template <typename T, typename F> __device__ __forceinline__ void for_each_token(const T* lg, const Row& r, F f)
{
    if (r.occ) for_each_row_token<BATCH>(lg, r.occ, r.V, r.nch, f);
    else for_each_row_token<BATCH>(lg, nullptr, r.V, r.nch, f);
}
// ... and for the passes in front of the scores, which read the logits alone
template <typename T, typename F> __device__ __forceinline__ void for_each_logit(const T* lg, const Row& r, F f)
{
    for_each_row_token<BATCH>(lg, nullptr, r.V, r.nch, [&](int, float x, float) { f(x); });
}

struct Shared {
    unsigned hist[256];
    u64 red[ROW_WAVES];
    u64 won[BEAM_MAX_K];              // the winners as key << 32 | 65535 - token, in the order they arrived
    Pick<unsigned> pick;
    unsigned n_won;
};

__device__ __forceinline__ void no_winners(const BeamArgs& a, int r)
{
    if ((int)threadIdx.x < a.K) a.keys[(long)r * a.K + threadIdx.x] = a.ids[(long)r * a.K + threadIdx.x] = 0u;
}

template <typename T>
__global__ void __launch_bounds__(ROW_THREADS) beam_rows_kernel(const BeamArgs a)
{
    __shared__ Shared sh;
    const int r = blockIdx.x, tid = threadIdx.x, K = a.K;
    const T* lg = static_cast<const T*>(a.logits) + (long)r * a.ld;

    // the group of the row: rows in no group, behind the first 64 of theirs, and dead rows leave an empty list and read nothing else
    const auto bound = [&](int v) { return clampi(v, 0, a.n_rows); };
    const int g = seq_of_row(a.cu_rows, a.n_groups, r, bound);
    const float cum = a.cum[r];
    if (g < 0 || r >= bound(a.cu_rows[g + 1]) || r - bound(a.cu_rows[g]) >= BEAM_MAX_ROWS || cum == NEG_INF) return no_winners(a, r);
    // parameters and slots: judged before anything is addressed with them
    const float pen = a.penalty ? a.penalty[g] : 1.f;
    if (!(cum < __builtin_inff()) || !(pen >= 0.f && pen < __builtin_inff())) return no_winners(a, r);
    const int slot = a.slot ? a.slot[r] : r;
    Row row;
    row.occ = a.occ && pen != 1.f && slot >= 0 && slot < a.n_slots ? a.occ + (long)slot * a.ld : nullptr;
    row.V = a.V; row.nch = (a.V + 7) / 8;
    row.cum = cum; row.pen = pen; row.m = 0.f; row.L = 0.f;

    // ---- pass A: is the row sound, and max z.  (A logit of +inf has no softmax: it poisons the row like a NaN.)
    int bad = 0;
    unsigned kmax = 0;
    for_each_logit(lg, row, [&](float x) {
        bad |= !(x < __builtin_inff());
        kmax = max(kmax, key_of(x));
    });
    bad = __syncthreads_or(bad);
    row.m = z_of((unsigned)block_reduce<false>(kmax, sh.red));
    if (bad || !(row.m > NEG_INF)) return no_winners(a, r);

    // ---- pass B: the denominator, an integer (at least 2^46: the maximum itself), and its log
    u64 part = 0;
    for_each_logit(lg, row, [&](float x) { part += (u64)(expf(x - row.m) * FIX); });
    row.L = (float)log((double)block_reduce<true>(part, sh.red) / (double)FIX);

    // ---- radix selection, 8 bits a pass: key_k = the K-th largest key of the candidates (fewer than K: the smallest).  A pass adds to
    // the histogram only the tokens that match the digits found so far.
    unsigned key_k = 0, above_k = 0, equal_k = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const Pick<unsigned> p = radix_step(sh.hist, &sh.pick, above_k, (unsigned)K, [&](auto add) {
            for_each_token(lg, row, [&](int, float x, float o) {
                const float s = score_of(x, o, row);
                const unsigned key = key_of(s);
                if (s > NEG_INF && (pass == 0 || (key ^ key_k) >> (shift + 8) == 0)) add((key >> shift) & 255u, 1u);
            });
        });
        key_k |= p.digit << shift; above_k = p.above; equal_k = p.equal;
    }
    // ---- ties at the boundary: of the equal_k tokens at key_k the K - above_k lowest ids stay (tie_cut)
    unsigned rid_cut = 0;                                    // tokens at key_k stay while 65535 - n >= rid_cut
    if (above_k < (unsigned)K && (unsigned)K - above_k < equal_k)
        rid_cut = tie_cut(sh.hist, &sh.pick, (unsigned)K - above_k, [&](auto at) {
            for_each_token(lg, row, [&](int n, float x, float o) {
                if (key_of(score_of(x, o, row)) == key_k) at(n);
            });
        });

    // ---- the winners, in the order they arrive (at most K by construction; the bound is checked where the list is written all the same)
    if (tid == 0) sh.n_won = 0;
    __syncthreads();
    for_each_token(lg, row, [&](int n, float x, float o) {
        const float s = score_of(x, o, row);
        const unsigned key = key_of(s), rid = 65535u - (unsigned)n;
        if (s > NEG_INF && (key > key_k || (key == key_k && rid >= rid_cut))) {
            const unsigned at = atomicAdd(&sh.n_won, 1u);
            if (at < (unsigned)K) sh.won[at] = ((u64)key << 32) | rid;
        }
    });
    __syncthreads();
    // ---- ... ranked by (score descending, token ascending): the values are distinct, a winner's rank is the number of larger ones
    const int n_won = min((int)sh.n_won, K);
    if (tid < K) {
        int at = tid;
        unsigned key = 0, id = 0;
        if (tid < n_won) {
            const u64 v = sh.won[tid];
            at = 0;
            for (int j = 0; j < n_won; ++j) at += sh.won[j] > v;
            key = (unsigned)(v >> 32); id = 65535u - (unsigned)(v & 0xffffffffu);
        }
        a.keys[(long)r * K + at] = key;
        a.ids[(long)r * K + at] = id;
    }
}

// ---- one wave per group
__global__ void __launch_bounds__(64) beam_merge_kernel(const BeamArgs a)
{
    __shared__ unsigned keys[BEAM_MAX_ROWS * BEAM_MAX_K], ids[BEAM_MAX_ROWS * BEAM_MAX_K];
    const int g = blockIdx.x, lane = threadIdx.x, K = a.K;
    const int lo = clampi(a.cu_rows[g], 0, a.n_rows), hi = clampi(a.cu_rows[g + 1], 0, a.n_rows);
    const int rows = clampi(hi - lo, 0, BEAM_MAX_ROWS);
    for (int i = lane; i < rows * K; i += 64) {
        keys[i] = a.keys[(long)lo * K + i];
        ids[i] = a.ids[(long)lo * K + i];
    }
    __syncthreads();
    int head = 0;
    for (int j = 0; j < K; ++j) {
        const unsigned mine = lane < rows && head < K ? keys[lane * K + head] : 0u;
        const u64 best = wave_max(mine ? ((u64)mine << 32) | (unsigned)(63 - lane) : 0);
        const long out = (long)g * K + j;
        if (best == 0) {                                     // every list is used up: the rest is missing
            if (lane == 0) { a.parent[out] = -1; a.token[out] = -1; a.score[out] = NEG_INF; }
        } else if (lane == 63 - (int)(best & 63u)) {
            a.parent[out] = lo + lane;
            a.token[out] = (int)ids[lane * K + head];
            a.score[out] = z_of(mine);
            ++head;
        }
    }
}

}  // namespace

hipError_t launch_beam_candidates(const BeamArgs& a, int io, hipStream_t st)
{
    if (!(a.logits && a.cum && a.cu_rows && a.parent && a.token && a.score && a.keys && a.ids)) return hipErrorInvalidValue;
    if (a.n_rows < 1 || a.n_groups < 1 || a.K < 1 || a.K > BEAM_MAX_K || a.V < 1 || a.V > BEAM_MAX_V || a.ld < a.V || a.ld % 8) return hipErrorInvalidValue;
    if (a.occ && a.n_slots < 1) return hipErrorInvalidValue;
    const dim3 grid(a.n_rows), block(ROW_THREADS);
    hipError_t e;
    if (io == IO_F32) e = launch<beam_rows_kernel<float>>(grid, block, 0, st, a);
    else if (io == IO_F16) e = launch<beam_rows_kernel<f16_t>>(grid, block, 0, st, a);
    else e = launch<beam_rows_kernel<bf16_t>>(grid, block, 0, st, a);
    if (e != hipSuccess) return e;
    return launch<beam_merge_kernel>(dim3(a.n_groups), dim3(64), 0, st, a);
}

}  // namespace wkv6

using namespace wkv6;

extern "C" {

// ---- the entry points (include/wkv6_amd.h); the order of the refusals is part of the contract
static size_t list_bytes(int n_rows, int K) { return align_up((size_t)n_rows * K * sizeof(unsigned)); }

size_t rwkv6_beam_candidates_workspace_bytes(int n_rows, int K)
{
    if (n_rows < 1 || K < 1 || K > BEAM_MAX_K) return 0;
    return 2 * list_bytes(n_rows, K);
}

static int beam_candidates(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                           const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token, float* score,
                           void* workspace, size_t workspace_bytes, int io, void* stream)
{
    if (n_rows < 1 || V < 1 || n_groups < 1 || ld < V || ld % 8 || K < 1 || K > BEAM_MAX_K) return WKV6_EINVAL;
    if (occ_pool && (n_slots < 1 || (!slot && n_slots < n_rows))) return WKV6_EINVAL;
    if (((uintptr_t)logits | (uintptr_t)occ_pool) & 15) return WKV6_EINVAL;
    if (((uintptr_t)cum | (uintptr_t)cu_rows | (uintptr_t)slot | (uintptr_t)penalty | (uintptr_t)parent | (uintptr_t)token | (uintptr_t)score
         | (uintptr_t)workspace) & 3) return WKV6_EINVAL;
    const size_t out_bytes = (size_t)n_groups * K * 4, need = rwkv6_beam_candidates_workspace_bytes(n_rows, K);
    const struct { const void* p; size_t bytes; } outs[] = {{parent, out_bytes}, {token, out_bytes}, {score, out_bytes}, {workspace, need}},
        ins[] = {{logits, (size_t)n_rows * ld * (io == IO_F32 ? 4 : 2)}, {cum, (size_t)n_rows * 4}, {cu_rows, ((size_t)n_groups + 1) * 4},
                 {occ_pool, (size_t)(n_slots > 0 ? n_slots : 0) * ld * 4}, {slot, (size_t)n_rows * 4}, {penalty, (size_t)n_groups * 4}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            if (overlap(o.p, o.bytes, i.p, i.bytes)) return WKV6_EINVAL;
    if (V > BEAM_MAX_V) return WKV6_EUNSUPPORTED;
    if (!logits || !cum || !cu_rows || !parent || !token || !score || !workspace) return WKV6_ENULL;
    if ((occ_pool == nullptr) != (penalty == nullptr) || (slot && !occ_pool)) return WKV6_ENULL;
    if (workspace_bytes < need) return WKV6_EWORKSPACE;
    BeamArgs a = {};
    a.n_rows = n_rows; a.V = V; a.ld = ld; a.n_groups = n_groups; a.K = K; a.n_slots = n_slots;
    a.logits = logits; a.cum = cum; a.cu_rows = cu_rows; a.occ = occ_pool; a.slot = slot; a.penalty = penalty;
    a.parent = parent; a.token = token; a.score = score;
    a.keys = static_cast<unsigned*>(workspace);
    a.ids = a.keys + list_bytes(n_rows, K) / sizeof(unsigned);
    return to_rc(launch_beam_candidates(a, io, (hipStream_t)stream));
}
int rwkv6_beam_candidates_bf16(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream)
{
    return beam_candidates(n_rows, V, ld, logits, cum, n_groups, cu_rows, K, occ_pool, n_slots, slot, penalty, parent, token, score, workspace,
                           workspace_bytes, IO_BF16, stream);
}
int rwkv6_beam_candidates_fp16(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream)
{
    return beam_candidates(n_rows, V, ld, logits, cum, n_groups, cu_rows, K, occ_pool, n_slots, slot, penalty, parent, token, score, workspace,
                           workspace_bytes, IO_F16, stream);
}
int rwkv6_beam_candidates_fp32(int n_rows, int V, int ld, const void* logits, const float* cum, int n_groups, const int* cu_rows, int K,
                               const float* occ_pool, int n_slots, const int* slot, const float* penalty, int* parent, int* token,
                               float* score, void* workspace, size_t workspace_bytes, void* stream)
{
    return beam_candidates(n_rows, V, ld, logits, cum, n_groups, cu_rows, K, occ_pool, n_slots, slot, penalty, parent, token, score, workspace,
                           workspace_bytes, IO_F32, stream);
}

}  // extern "C"
