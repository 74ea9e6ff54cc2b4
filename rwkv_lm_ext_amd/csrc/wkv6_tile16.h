// The 16-row MFMA tile that the per-sequence LoRA pair (wkv6_lora.hip) and the low-rank time-mix pairs (wkv6_lowrank.hip) are built on.
//
// Tiles of 16 rows on v_mfma_f32_16x16x32_bf16 with the TOKEN as the MFMA column: lane (c = lane & 15, g = lane >> 4) feeds 8 consecutive
// k of token c (one 16-byte global load) and 8 consecutive k of weight row c (one 16-byte load of a matrix in [out, in] layout), and
// receives rows 4g..4g+3 of column c -- four consecutive outputs of its own token.  No LDS for the operands.  Every output element is its
// own dot product in the MFMA's own k order, so a row's bits do not depend on the rows beside it.  An operand that does not exist is a
// literal zero, never loaded; nothing is masked by a multiply.
//
// Here: the vector types and loads, the walk of a "shrink" kernel over K with the sum of its chunk partials, and the tile of an "expand"
// kernel (row-to-column map, MFMA pass, epilogue walk).  How work is spread over waves and workgroups, the operand masks and every
// epilogue's arithmetic are the files' own.
#pragma once
#include "wkv6_common.h"

namespace wkv6 {

typedef __bf16 b8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

constexpr int TILE = 16;               // rows per tile (the MFMA's 16 columns)
constexpr int EXPAND_NB = 64;          // output columns of one expand pass (4 MFMA tiles: 16 consecutive n per lane)

__device__ __forceinline__ b8v zero8() { return __builtin_bit_cast(b8v, v4u{0u, 0u, 0u, 0u}); }
__device__ __forceinline__ v4u ld16(const bf16_t* p) { return *reinterpret_cast<const v4u*>(p); }
__device__ __forceinline__ b8v load8(const bf16_t* p) { return __builtin_bit_cast(b8v, ld16(p)); }
__device__ __forceinline__ f4v mfma32(b8v a, b8v b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// the roles of a thread: its wave, and its lane as (column c, row group g) of the tile
struct Lane16 {
    int lane, wave, c, g;
    __device__ __forceinline__ Lane16() : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), c(lane & 15), g(lane >> 4) {}
};

// ---- shrink.  K is cut into nch = min(4, K / 32) interleaved chunks of 32-wide steps -- fixed by K alone --; a chunk takes the steps
// first, first + stride, ... below nsteps (stride = nch).  load(u, k) fetches the operands of the step at element offset k into the
// caller's slot u, use(u) consumes them: four steps' loads in flight, then the rest one by one.
template <typename L, typename U> __device__ __forceinline__ void for_each_kstep(int first, int stride, int nsteps, L load, U use)
{
    int s = first;
    for (; s + 3 * stride < nsteps; s += 4 * stride) {
#pragma unroll
        for (int u = 0; u < 4; ++u) load(u, 32 * (s + u * stride));
#pragma unroll
        for (int u = 0; u < 4; ++u) use(u);
    }
    for (; s < nsteps; s += stride) {
        load(0, 32 * s);
        use(0);
    }
}

// The chunks leave their partial sums in LDS at [chunk][token][j]; one lane adds the four j = 4g.. of its token over the chunks in the order
// 0, 1, .., nch - 1 (the order is part of the result's bits).  The caller rounds.
template <typename P> __device__ __forceinline__ auto sum_chunks(const P (*part)[TILE][16], int nch, int c, int g)
{
    typedef P p4 __attribute__((ext_vector_type(4)));
    p4 sum = *reinterpret_cast<const p4*>(&part[0][c][4 * g]);
#pragma unroll 1                       // (at most three trips)
    for (int q = 1; q < nch; ++q) sum +=*reinterpret_cast<const p4*>(&part[q][c][4 * g]);
    return sum;
}

// ---- expand.  MFMA rows = n, columns = tokens.  MFMA row rho of tile i stands for column n0 + 16 (rho >> 2) + 4 i + (rho & 3), so that lane
// (c, g) ends with the 16 CONSECUTIVE columns n0 + 16 g .. + 15 of its token: every access of the epilogue is two 16-byte accesses per
// lane, 128 contiguous bytes per token.
//
// One pass for the 64 columns from n0: acc[i] = sum over the STEPS steps of 32 of w[n][..] tok[..], w = the weight rows [N,R] at the lane's
// 8 g; w_ok false: the lane's weight operand is a literal zero.
template <int R, int STEPS>
__device__ __forceinline__ void expand_pass(f4v (&acc)[4], const bf16_t* w, bool w_ok, int n0, int c, const b8v (&tok)[STEPS])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + 16 * (c >> 2) + 4 * i + (c & 3);
        acc[i] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < STEPS; ++st) acc[i] = mfma32(w_ok ? load8(w + (long)n * R + 32 * st) : zero8(), tok[st], acc[i]);
    }
}
// Half h (8 columns, one 16-byte access) of the lane's 16 as four words: word p holds columns 8 h + 2 p, + 1 = tile i = 2 h + (p >> 1),
// rows 2 (p & 1), + 1.  word(p, lower column's sum, upper column's sum) makes the word.
template <typename F> __device__ __forceinline__ v4u expand_half(const f4v (&acc)[4], int h, F word)
{
    v4u out;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = 2 * h + (p >> 1), q = 2 * (p & 1);
        out[p] = word(p, acc[i][q], acc[i][q + 1]);
    }
    return out;
}

}  // namespace wkv6
