// Device-side token sampling with a penalty slot pool (include/wkv6_amd.h: rwkv6_sample_slots_*; kernel in wkv6_sample.hip).
#pragma once
#include "wkv6_scan.h"

namespace wkv6 {

constexpr int SAMPLE_MAX_V = 65536;

struct SampleArgs {
    int n_seq, V, ld, n_slots;
    const void* logits;       // [n_seq,ld] in the I/O type
    float* occ;               // [n_slots,ld]
    const int* slot;          // [n_seq] or null: the sequence index
    const int* slot_out;      // [n_seq] or null: in place
    const float* params;      // [n_seq,8]
    const float* u;           // [n_seq]
    int* tokens;              // [n_seq]
    float* logprob;           // [n_seq] or null
};

// one launch, one workgroup per sequence; io: IO_BF16 / IO_F16 / IO_F32 of the logits
hipError_t launch_sample_slots(const SampleArgs& a, int io, hipStream_t st);

}  // namespace wkv6
