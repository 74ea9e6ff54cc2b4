// Rows of [n, V] logits streamed 16 bytes per lane: what the sampler (wkv6_sample.hip) and the cross-entropy kernels (wkv6_ce.hip) share.
#pragma once
#include "wkv6_common.h"

namespace wkv6 {

// ---- 8 consecutive elements of a row as fp32
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&x)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&x)[8])
{
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&x)[8])
{
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u raw = *reinterpret_cast<const v4u*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = bf_lo(raw[i]); x[2 * i + 1] = bf_hi(raw[i]); }
}
template <> __device__ __forceinline__ void load8<f16_t>(const f16_t* p, float (&x)[8])
{
    typedef f16_t h8 __attribute__((ext_vector_type(8)));
    const h8 raw = *reinterpret_cast<const h8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (float)raw[i];
}
template <typename T> __device__ __forceinline__ float load1(const T* p) { return (float)*p; }
template <> __device__ __forceinline__ float load1<bf16_t>(const bf16_t* p) { return __uint_as_float((unsigned)*p << 16); }

// ---- and back: one rounding to nearest even into the row's type
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&x)[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&x)[8])
{
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(x[4], x[5], x[6], x[7]);
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&x)[8])
{
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf2(x[0], x[1]), pack_bf2(x[2], x[3]), pack_bf2(x[4], x[5]), pack_bf2(x[6], x[7]));
}
template <> __device__ __forceinline__ void store8<f16_t>(f16_t* p, const float (&x)[8])
{
    typedef f16_t h8 __attribute__((ext_vector_type(8)));
    const h8 raw = {(f16_t)x[0], (f16_t)x[1], (f16_t)x[2], (f16_t)x[3], (f16_t)x[4], (f16_t)x[5], (f16_t)x[6], (f16_t)x[7]};
    *reinterpret_cast<h8*>(p) = raw;
}
template <typename T> __device__ __forceinline__ void store1(T* p, float x) { *p = (T)x; }
template <> __device__ __forceinline__ void store1<bf16_t>(bf16_t* p, float x) { *p = (bf16_t)(pack_bf2(x, 0.f) & 0xffffu); }

}  // namespace wkv6
