// The row arrays of wkv6_bi, made on the device in front of its launches: lens from the mask, and the order the rows are dispatched in.
#include "wkv6_host.h"

using namespace wkv6;

namespace {            // (the kernels keep their names outside namespace wkv6: profile filters tell them from the operator kernels by it)

// lens[b] = 1 + index of the first zero of mask[b][:], or T when the row has no zero
// (cuda/wkv6_bi_cuda.cu:21-69 breaks AFTER processing the first masked token).
__global__ void mask_to_lens_kernel(const int* __restrict__ mask, int* __restrict__ lens, int T)
{
    const int b = blockIdx.x;
    int first = T;                                           // "no zero" sentinel
    for (int t = threadIdx.x; t < T; t += blockDim.x)
        if (mask[(long)b * T + t] == 0) { first = t; break; }
    __shared__ int red[256];
    red[threadIdx.x] = first;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) lens[b] = min(red[0] + 1, T);
}

// order[rank] = b with the rows ranked by decreasing length (length_rank: list scheduling; ~9 % on ragged batches of 1536 workgroups)
__global__ void length_order_kernel(const int* __restrict__ lens, int* __restrict__ order, int B)
{
    for (int b = threadIdx.x; b < B; b += blockDim.x) order[length_rank(b, lens[b], B, [&](int o) { return lens[o]; })] = b;
}

}  // namespace

namespace wkv6 {

hipError_t bi_row_arrays(ScanArgs& a, const int* mask, const int* lens, int* lens_buf, int* order_buf, bool chunked, hipStream_t st)
{
    if (!lens) {
        if (hipError_t e = launch<mask_to_lens_kernel>(dim3(a.B), dim3(256), 0, st, mask, lens_buf, a.T)) return e;
        lens = lens_buf;
    }
    a.lens = lens;
    if (chunked && a.B > 1 && a.B <= 4096) {
        if (hipError_t e = launch<length_order_kernel>(dim3(1), dim3(256), 0, st, lens, order_buf, a.B)) return e;
        a.order = order_buf;
    }
    return hipSuccess;
}

}  // namespace wkv6
