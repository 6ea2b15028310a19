// What the decoder (ans.hip) and the encoder (ans_enc.hip) of the entropy-coded
// frame stream (version 2) share: the coder's constants, the
// layout of the frequency tables, and bounds-checked aligned reads.
#pragma once

#include "stream.h"

namespace gsvc {

constexpr int kAnsChannels = 7;
constexpr int kProbBits = 12;
constexpr int kProbOne = 1 << kProbBits;
constexpr unsigned kRansL = 1u << 16;
constexpr int kMaxSegment = 4096;
constexpr int kAnsSymbols = 3 * 64 + 2 * 8 + 2 * 256;
constexpr int kTableBytes = 2 * kAnsSymbols;
constexpr int kCodedFixedBytes = kHeaderBytes + kTableBytes;  // what precedes the low plane

__host__ __device__ constexpr int ans_alphabet(int c) { return c < 3 ? 64 : c < 5 ? 8 : 256; }
// symbols before channel c in the tables
__host__ __device__ constexpr int ans_first(int c) {
    return c < 3 ? 64 * c : c < 5 ? 192 + 8 * (c - 3) : 208 + 256 * (c - 5);
}
static_assert(ans_first(6) + ans_alphabet(6) == kAnsSymbols, "table layout");

// The aligned dword at q, with bytes outside [lo, hi) read as 0.
__device__ __forceinline__ unsigned ld_dword(uintptr_t q, uintptr_t lo, uintptr_t hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const unsigned *>(q);
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (q + b >= lo && q + b < hi) v |= (unsigned)*reinterpret_cast<const unsigned char *>(q + b) << (8 * b);
    return v;
}

}  // namespace gsvc
