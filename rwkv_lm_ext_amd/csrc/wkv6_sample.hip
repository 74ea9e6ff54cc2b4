// Device-side token sampling with a penalty slot pool (include/wkv6_amd.h: rwkv6_sample_slots_*), hand-written for gfx950: one launch
// turns the logits rows of a packed decode step into token ids, every sequence with its own temperature / top-p / top-k / penalties, and
// keeps the sequence's decaying token-occurrence counts under its slot number.  The header states the operation; this is how it is done.
//
// One workgroup of 1024 threads (16 waves) per sequence.  The row is not sorted and nothing of size V leaves the chip except the
// occurrence row itself: the kept set of the definition is a THRESHOLD on the penalised logit z, so it is found by radix selection over
// the monotone 32-bit key of z -- four passes of 8 bits, most significant digit first, with one 256-bin histogram of probability MASS
// (nucleus) and one of COUNTS (top-k) in LDS -- and the ties at the top-k boundary are cut by a second radix selection over the token id.
// The pieces of the selection (keys, row walker, histogram runs, select_bin, tie_cut) are those of wkv6_rows.h, shared with wkv6_beam.hip;
// the pass that fills both histograms in ONE walk of the row is this file's own.
//
// Where the row lives: in neither registers nor LDS.  Every pass streams the row again as 16-byte loads (thread t takes the chunks of 8
// tokens t, t + 1024, ...) and recomputes z; after the first pass the loads are served by L2 / Infinity Cache, so a logits row and an
// occurrence row cross HBM once in each direction.  64 fp32 values per lane would fit the 128-VGPR budget of 16 waves only with every
// pass unrolled 64 times; a bf16 row in LDS does not hold the PENALISED logits exactly.  DESIGN.md 4.21 has the numbers.
//
// No floating-point sum runs over the row at all.  A weight exp(.) in [0, 1] becomes the integer floor(w * 2^46) the moment it is formed,
// and every sum over the row (softmax denominator, histogram masses, W, the CDF of the draw) is a sum of these 64-bit integers: exact,
// so its value cannot depend on the order in which waves or LDS atomics arrive, and the call is bit-reproducible.  65536 terms of at most
// 2^46 stay below 2^63.  The quantisation is 2^-46 of the largest weight per term.
#include <cmath>
#include "wkv6_sample.h"
#include "wkv6_rows.h"                 // load8, load1, the row walker, the radix selection, block_reduce
#include "wkv6_host.h"                 // to_rc, overlap

// the same expression must give the same bits wherever it is inlined (weights are formed once for W and once more for the draw)
#pragma clang fp contract(off)

namespace wkv6 {
namespace {

constexpr int PARTS = SAMPLE_MAX_V / 8 / 64;                  // 128: the chunks of 8 tokens come in blocks of 64 (one wave, one round)

// ---- what a sequence's row is made of
struct Row {
    const float* src;         // the occurrence row read, null: all zero
    int V, nch;               // tokens, chunks of 8
    float ap, af, pen;        // alpha_presence, alpha_frequency, repetition_penalty
};

// step 1 of the definition.  -0 becomes +0 (equal values, one key); a NaN can only come from a non-finite pool entry and counts as -inf.
__device__ __forceinline__ float penalise(float x, float o, const Row& r)
{
    float z = o > 0.f ? x - (r.ap + o * r.af) : x;
    if (z == 0.f) z = 0.f;
    return z == z ? z : NEG_INF;
}
// step 5
__device__ __forceinline__ float repeat_penalty(float z, float o, const Row& r)
{
    if (!(o > 0.f) || r.pen == 1.f) return z;
    float y = z < 0.f ? z * r.pen : z / r.pen;
    if (y == 0.f) y = 0.f;
    return y == y ? y : NEG_INF;
}
// floor(exp((z - top) / t) * 2^46): at most 2^46, 0 for z = -inf (and for a NaN, which only garbage parameters can make)
__device__ __forceinline__ u64 weight(float z, float top, float t) { return (u64)(expf((z - top) / t) * FIX); }

// z and o of the 8 tokens of chunk c, for the passes that keep a chunk's weights in registers (W and the draw)
template <typename T> __device__ __forceinline__ void load_chunk(const T* lg, const Row& r, int c, float (&z)[8], float (&o)[8])
{
    float x[8];
    load8<T>(lg + 8 * c, x);
    if (r.src) load8<float>(r.src + 8 * c, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!r.src) o[j] = 0.f;
        z[j] = penalise(x[j], o[j], r);
    }
}
// f(n, z, o) for every token n < V, one chunk's loads in flight (for_each_row_token)
template <typename T, typename F> __device__ __forceinline__ void for_each_token(const T* lg, const Row& r, F f)
{
    for_each_row_token<1>(lg, r.src, r.V, r.nch, [&](int n, float x, float o) { f(n, penalise(x, o, r), o); });
}

struct Shared {
    u64 hist_p[256], hist_k[256];     // nucleus: mass per digit; top-k (and the id selection behind it): count per digit
    u64 red[ROW_WAVES];
    u64 part[PARTS];                  // W per (round, wave) = per 512 consecutive tokens
    Pick<u64> pick_p, pick_k;
    u64 base;                         // the draw: W in front of the block that holds the token, and the block
    int block, token;
};

template <typename T>
__global__ void __launch_bounds__(ROW_THREADS) sample_slots_kernel(const SampleArgs a)
{
    __shared__ Shared sh;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* lg = static_cast<const T*>(a.logits) + (long)s * a.ld;

    // parameters and slots: judged before anything is addressed with them
    float prm[8];
    bool poisoned = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        prm[i] = a.params[(long)s * 8 + i];
        poisoned |= !(prm[i] >= 0.f && prm[i] < __builtin_inff());
    }
    const float temperature = prm[0], top_p = prm[1], decay = prm[5];
    const int from = a.slot ? a.slot[s] : s, to = a.slot_out ? a.slot_out[s] : from;
    Row r;
    r.src = from >= 0 && from < a.n_slots ? a.occ + (long)from * a.ld : nullptr;
    float* const dst = to >= 0 && to < a.n_slots ? a.occ + (long)to * a.ld : nullptr;
    r.V = a.V; r.nch = (a.V + 7) / 8;
    r.ap = prm[3]; r.af = prm[4]; r.pen = prm[6];
    const int k = prm[2] >= 1.f && prm[2] < (float)a.V ? (int)prm[2] : 0;            // 0: top-k is off
    const bool use_p = top_p < 1.f, use_k = k > 0;

    // ---- pass A: is the row sound, and max z.  (A logit of +inf has no softmax: it poisons the row like a NaN.)
    int bad = 0, finite = 0;
    unsigned kmax = 0;
    for_each_row_token<1>(lg, r.src, r.V, r.nch, [&](int, float x, float o) {
        bad |= !(x < __builtin_inff());
        finite |= x > NEG_INF;
        kmax = max(kmax, key_of(penalise(x, o, r)));
    });
    bad = __syncthreads_or(bad);
    finite = __syncthreads_or(finite);
    const float top = z_of((unsigned)block_reduce<false>(kmax, sh.red));
    if (poisoned || bad || !finite || !(top > NEG_INF)) {
        if (tid == 0) {
            a.tokens[s] = -1;
            if (a.logprob) a.logprob[s] = __builtin_nanf("");
        }
        return;
    }

    int token;
    float top_kept = 0.f;
    u64 W = 0;
    if (temperature == 0.f) {
        // ---- greedy: argmax of the repetition-penalised z, the lowest id among equals
        u64 best = 0;
        for_each_token(lg, r, [&](int n, float z, float o) {
            const u64 v = ((u64)key_of(repeat_penalty(z, o, r)) << 32) | (0xffffffffu - (unsigned)n);
            best = v > best ? v : best;
        });
        token = (int)(0xffffffffu - (unsigned)block_reduce<false>(best, sh.red));
    } else {
        // ---- radix selection, 8 bits a pass: key_p = the largest key whose mass {key >= key_p} reaches top_p of the total, key_k = the
        // k-th largest key.  A pass adds to the histograms only the tokens that match the digits found so far.
        unsigned key_p = 0, key_k = 0;
        u64 above_p = 0, above_k = 0, equal_k = 0, target_p = 0;
        for (int pass = 0; pass < 4 && (use_p || use_k); ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) sh.hist_p[tid] = sh.hist_k[tid] = 0;
            __syncthreads();
            Run<u64> run_p, run_k;
            for_each_token(lg, r, [&](int, float z, float) {
                const unsigned key = key_of(z), digit = (key >> shift) & 255u;
                if (use_p && (pass == 0 || (key ^ key_p) >> (shift + 8) == 0)) run_p.add(sh.hist_p, digit, weight(z, top, 1.f));
                if (use_k && (pass == 0 || (key ^ key_k) >> (shift + 8) == 0)) run_k.add(sh.hist_k, digit, 1);
            });
            run_p.flush(sh.hist_p);
            run_k.flush(sh.hist_k);
            __syncthreads();
            if (wave == 0 && use_p) {
                if (pass == 0) {        // the softmax denominator is the whole first histogram
                    const u64 S = wave_sum(sh.hist_p[lane] + sh.hist_p[lane + 64] + sh.hist_p[lane + 128] + sh.hist_p[lane + 192]);
                    const double t = ceil((double)top_p * (double)S);
                    target_p = t >= (double)S ? S : (u64)t;
                }
                const Pick<u64> p = select_bin(sh.hist_p, above_p, target_p);
                if (lane == 0) sh.pick_p = p;
            }
            if (wave == 1 && use_k) {
                const Pick<u64> p = select_bin(sh.hist_k, above_k, (u64)k);
                if (lane == 0) sh.pick_k = p;
            }
            __syncthreads();
            if (use_p) { key_p |= sh.pick_p.digit << shift; above_p = sh.pick_p.above; }
            if (use_k) { key_k |= sh.pick_k.digit << shift; above_k = sh.pick_k.above; equal_k = sh.pick_k.equal; }
        }
        // ---- ties at the top-k boundary: of the equal_k tokens at key_k the k - above_k lowest ids stay (tie_cut)
        unsigned rid_cut = 0;                                 // tokens at key_k stay while 65535 - n >= rid_cut
        if (use_k && (u64)k - above_k < equal_k)
            rid_cut = tie_cut(sh.hist_k, &sh.pick_k, (u64)k - above_k, [&](auto at) {
                for_each_token(lg, r, [&](int n, float z, float) {
                    if (key_of(z) == key_k) at(n);
                });
            });
        const auto kept = [&](int n, float z) {
            const unsigned key = key_of(z);
            return key >= key_p && (!use_k || key > key_k || (key == key_k && 65535u - (unsigned)n >= rid_cut));
        };

        // ---- pass C: the largest repetition-penalised z of the kept set, and its largest id
        unsigned ktop = 0, nmax = 0;
        for_each_token(lg, r, [&](int n, float z, float o) {
            if (kept(n, z)) { ktop = max(ktop, key_of(repeat_penalty(z, o, r))); nmax = (unsigned)n + 1; }
        });
        top_kept = z_of((unsigned)block_reduce<false>(ktop, sh.red));
        const int last_kept = (int)block_reduce<false>(nmax, sh.red) - 1;

        // ---- pass D: W, kept per block of 512 consecutive tokens (one wave, one round) for the draw
        if (tid < PARTS) sh.part[tid] = 0;
        if (tid == 0) { sh.block = -1; sh.token = last_kept; }
        __syncthreads();
        const int rounds = (r.nch + ROW_THREADS - 1) / ROW_THREADS;
        const auto chunk_weights = [&](int c, u64 (&w)[8]) {
            float z[8], o[8];
            load_chunk(lg, r, c, z, o);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                w[j] = 8 * c + j < r.V && kept(8 * c + j, z[j]) ? weight(repeat_penalty(z[j], o[j], r), top_kept, temperature) : 0;
        };
        for (int i = 0; i < rounds; ++i) {
            const int c = tid + ROW_THREADS * i;
            u64 w[8], sum = 0;
            if (c < r.nch) {
                chunk_weights(c, w);
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += w[j];
            }
            sum = wave_sum(sum);
            if (lane == 0) sh.part[i * ROW_WAVES + wave] = sum;
        }
        __syncthreads();
        // ---- the draw, in token-id order: wave 0 finds the block of 512 tokens in which the CDF passes u W, that block's wave the token
        u64 target = 0;
        if (wave == 0) {
            const u64 p0 = sh.part[2 * lane], p1 = sh.part[2 * lane + 1];
            const u64 incl = wave_inclusive_scan(p0 + p1, lane), before = incl - (p0 + p1);
            W = __shfl(incl, 63);
            const float uu = a.u[s];
            const double t = (double)(uu >= 0.f ? uu : 0.f) * (double)W;       // (a NaN u draws as 0)
            target = W == 0 ? 0 : t >= (double)W ? W - 1 : (u64)t;
            const int blk = before + p0 > target ? 2 * lane : incl > target ? 2 * lane + 1 : -1;
            const u64 hit = __ballot(blk >= 0);
            if (hit && lane == __ffsll((long long)hit) - 1) {
                sh.block = blk;
                sh.base = blk & 1 ? before + p0 : before;
            }
            if (lane == 0) { sh.red[0] = W; sh.red[1] = target; }
        }
        __syncthreads();
        W = sh.red[0]; target = sh.red[1];
        if (sh.block >= 0 && wave == (sh.block & (ROW_WAVES - 1))) {
            const int c = tid + ROW_THREADS * (sh.block / ROW_WAVES);
            u64 w[8] = {}, sum = 0;
            if (c < r.nch) chunk_weights(c, w);
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += w[j];
            u64 acc = sh.base + wave_inclusive_scan(sum, lane) - sum;
            int found = -1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc += w[j];
                if (found < 0 && acc > target) found = 8 * c + j;
            }
            const u64 hit = __ballot(found >= 0);
            if (hit && lane == __ffsll((long long)hit) - 1) sh.token = found;
        }
        __syncthreads();
        token = sh.token;                                    // (where rounding left none: the largest kept id)
    }
    if (token < 0 || token >= r.V) {                         // no kept token at all: only garbage in the pool or the parameters gets here
        if (tid == 0) {
            a.tokens[s] = -1;
            if (a.logprob) a.logprob[s] = __builtin_nanf("");
        }
        return;
    }
    if (tid == 0) {
        a.tokens[s] = token;
        if (a.logprob) {
            float lp = 0.f;                                  // greedy: the distribution is the one token
            if (temperature != 0.f) {
                const float o = r.src ? r.src[token] : 0.f;
                const float z = repeat_penalty(penalise(load1<T>(lg + token), o, r), o, r);
                lp = (float)((double)((z - top_kept) / temperature) - log((double)W / (double)FIX));
            }
            a.logprob[s] = lp;
        }
    }
    __syncthreads();                                         // the row is read for the last time above: now it may be overwritten

    // ---- the update: dst = o * alpha_decay, + 1 at the token; columns >= V are not touched
    if (dst == nullptr) return;
    for (int c = tid; c < r.nch; c += ROW_THREADS) {
        float o[8];
        if (r.src) load8<float>(r.src + 8 * c, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = r.src ? o[j] * decay : 0.f;
            if (8 * c + j == token) o[j] = o[j] + 1.f;
        }
        if (8 * c + 8 <= r.V) {
            *reinterpret_cast<float4*>(dst + 8 * c) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4*>(dst + 8 * c + 4) = make_float4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * c + j < r.V) dst[8 * c + j] = o[j];
        }
    }
}

}  // namespace

hipError_t launch_sample_slots(const SampleArgs& a, int io, hipStream_t st)
{
    if (!(a.logits && a.occ && a.params && a.u && a.tokens)) return hipErrorInvalidValue;
    if (a.n_seq < 1 || a.n_slots < 1 || a.V < 1 || a.V > SAMPLE_MAX_V || a.ld < a.V || a.ld % 8) return hipErrorInvalidValue;
    const dim3 grid(a.n_seq), block(ROW_THREADS);
    if (io == IO_F32) return launch<sample_slots_kernel<float>>(grid, block, 0, st, a);
    if (io == IO_F16) return launch<sample_slots_kernel<f16_t>>(grid, block, 0, st, a);
    return launch<sample_slots_kernel<bf16_t>>(grid, block, 0, st, a);
}

}  // namespace wkv6

using namespace wkv6;

extern "C" {

// ---- the entry points (include/wkv6_amd.h); the order of the refusals is part of the contract
static int sample_slots(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                        const float* params, const float* u, int* tokens, float* logprob, int io, void* stream)
{
    if (n_seq < 1 || V < 1 || n_slots < 1 || ld < V || ld % 8) return WKV6_EINVAL;
    if (!slot && n_slots < n_seq) return WKV6_EINVAL;
    if (((uintptr_t)logits | (uintptr_t)occ_pool) & 15) return WKV6_EINVAL;
    if (((uintptr_t)slot | (uintptr_t)slot_out | (uintptr_t)params | (uintptr_t)u | (uintptr_t)tokens | (uintptr_t)logprob) & 3) return WKV6_EINVAL;
    if (overlap(logits, (size_t)n_seq * ld * (io == IO_F32 ? 4 : 2), occ_pool, (size_t)n_slots * ld * 4)) return WKV6_EINVAL;
    if (V > SAMPLE_MAX_V) return WKV6_EUNSUPPORTED;
    if (!logits || !occ_pool || !params || !u || !tokens) return WKV6_ENULL;
    SampleArgs a = {};
    a.n_seq = n_seq; a.V = V; a.ld = ld; a.n_slots = n_slots;
    a.logits = logits; a.occ = occ_pool; a.slot = slot; a.slot_out = slot_out; a.params = params; a.u = u;
    a.tokens = tokens; a.logprob = logprob;
    return to_rc(launch_sample_slots(a, io, (hipStream_t)stream));
}
int rwkv6_sample_slots_bf16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_BF16, stream);
}
int rwkv6_sample_slots_fp16(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_F16, stream);
}
int rwkv6_sample_slots_fp32(int n_seq, int V, int ld, const void* logits, float* occ_pool, int n_slots, const int* slot, const int* slot_out,
                            const float* params, const float* u, int* tokens, float* logprob, void* stream)
{
    return sample_slots(n_seq, V, ld, logits, occ_pool, n_slots, slot, slot_out, params, u, tokens, logprob, IO_F32, stream);
}

}  // extern "C"
