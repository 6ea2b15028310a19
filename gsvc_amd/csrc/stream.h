// The frame stream's layout (include/gsvc_amd.h), shared by the
// fixed-length codec (quant.hip) and the entropy-coded one (ans.hip).
#pragma once

#include "common.h"

namespace gsvc {

constexpr unsigned kStreamMagic = GSVC_STREAM_MAGIC;
constexpr int kHeaderBytes = GSVC_STREAM_HEADER_BYTES;
constexpr int kSplatBytes = GSVC_STREAM_SPLAT_BYTES;
// header field offsets
constexpr int kOffMagic = 0, kOffVersion = 4, kOffN = 8, kOffH = 12, kOffW = 16, kOffFlags = 20,
              kOffScale = 24, kOffBeta = 36, kOffCodebooks = 48;
// version 2 only: u16 S, u16 prob_bits, u32 n_seg, u32 payload_bytes, u32 zero
constexpr int kOffSegment = 240, kOffProbBits = 242, kOffNumSeg = 244, kOffPayload = 248,
              kOffReserved = 252;

// little-endian reads at any byte offset
__host__ __device__ __forceinline__ unsigned rd_u16(const unsigned char *p) {
    return (unsigned)p[0] | (unsigned)p[1] << 8;
}
__host__ __device__ __forceinline__ unsigned rd_u32(const unsigned char *p) {
    return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
}

// quant.hip: the frame walk (unpack_kernel) over num_frames version-1 frames of
// total_bytes at stream_dev, nmax the largest frame's splat count.  The caller
// has validated the frames; returns a gsvc status.
int launch_unpack_walk(const char *what, int num_frames, const unsigned char *stream_dev,
                       long long total_bytes, long long total_splats, long long nmax,
                       const float *cholesky_bound, const float *prev_xyz,
                       const float *prev_cholesky, const float *prev_features, int prev_points,
                       float *xq, float *Lq, float *cq, float *Lpre, hipStream_t s);

}  // namespace gsvc
