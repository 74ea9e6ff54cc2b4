// Beam-search candidate selection on rows of logits (include/wkv6_amd.h: rwkv6_beam_candidates_*; kernels in wkv6_beam.hip).
#pragma once
#include "wkv6_scan.h"

namespace wkv6 {

constexpr int BEAM_MAX_V = 65536, BEAM_MAX_K = 64, BEAM_MAX_ROWS = 64;      // BEAM_MAX_ROWS: rows of a group that are considered

struct BeamArgs {
    int n_rows, V, ld, n_groups, K, n_slots;
    const void* logits;       // [n_rows,ld] in the I/O type
    const float* cum;         // [n_rows]
    const int* cu_rows;       // [n_groups + 1]
    const float* occ;         // [n_slots,ld] or null: no penalty
    const int* slot;          // [n_rows] or null: the row index
    const float* penalty;     // [n_groups] or null: no penalty
    int *parent, *token;      // [n_groups,K]
    float* score;             // [n_groups,K]
    unsigned *keys, *ids;     // the workspace: [n_rows,K] each, a row's winners best first (key 0: none)
};

// two launches: one workgroup per row, then one wave per group; io: IO_BF16 / IO_F16 / IO_F32 of the logits
hipError_t launch_beam_candidates(const BeamArgs& a, int io, hipStream_t st);

}  // namespace wkv6
