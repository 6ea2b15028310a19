// Per-splat 2D projection shared by project2d.hip (the op) and frame.hip
// (the fused frame render), and its VJP shared by project2d.hip and train.hip
// (the fused training step): one op sequence, so all give identical bits.
#pragma once

#include "common.h"

namespace gsvc {

// helpers.cuh:45-68 compute_cov2d_bounds
__device__ __forceinline__ bool cov2d_bounds(float cxx, float cxy, float cyy,
                                             float &c0, float &c1, float &c2, float &radius) {
    const float det = cxx * cyy - cxy * cxy;
    if (det == 0.0f) return false;
    const float inv_det = 1.0f / det;
    c0 = cyy * inv_det;
    c1 = -cxy * inv_det;
    c2 = cxx * inv_det;
    const float b = 0.5f * (cxx + cyy);
    const float disc = fmaxf(0.1f, b * b - det);
    const float v1 = b + sqrtf(disc);
    const float v2 = b - sqrtf(disc);
    radius = ceilf(3.0f * sqrtf(fmaxf(v1, v2)));
    return true;
}

struct SplatProj {
    float2 xy;
    float c0, c1, c2;  // conic
    int rad, hit;      // radius (pixels), tiles of the bbox
};

// foward2d.cu:12-69 for one splat: means2d (NDC) and Cholesky factor
// (l11, l21, l22) -> centre in pixels, conic, radius, tile count.
// Degenerate covariances give zeros (the reference leaves them unwritten
// after zero-filling).
__device__ __forceinline__ SplatProj project_splat(float mx, float my, float l11, float l21,
                                                   float l22, float hw, float hh, int tbx, int tby) {
    const float cx = fmaf(hw, mx, hw);
    const float cy = fmaf(hh, my, hh);
    const float cxx = l11 * l11;
    const float cxy = l11 * l21;
    const float cyy = l21 * l21 + l22 * l22;
    SplatProj P;
    P.xy = make_float2(0.0f, 0.0f);
    P.c0 = P.c1 = P.c2 = 0.0f;
    P.rad = P.hit = 0;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, radius = 0.0f;
    if (cov2d_bounds(cxx, cxy, cyy, c0, c1, c2, radius)) {
        P.xy = make_float2(cx, cy);
        P.c0 = c0;
        P.c1 = c1;
        P.c2 = c2;
        P.rad = cvt_i32(radius);
        unsigned x0, y0, x1, y1;
        tile_bbox(cx, cy, radius, tbx, tby, x0, y0, x1, y1);
        const int area = (int)((x1 - x0) * (y1 - y0));
        P.hit = area > 0 ? area : 0;
    }
    return P;
}

// backward2d.cu:8-51 for one splat of radius > 0: conic X (symmetric), its
// gradient G and the bounded Cholesky entries -> v_cov2d = {g11, g12, g22} and
// v_L.  cov2d_to_conic_vjp (helpers.cuh:71-82) expanded in glm's column-major
// mat2 product order, V = ((-X) * G) * X; this expression tree is the contract
// (project2d.hip's backward and train.hip's splat step give the same bits).
__device__ __forceinline__ void project2d_vjp(float X00, float X01, float X11, float G00, float G01,
                                              float G11, float l11, float l21, float l22,
                                              float (&v_cov2d)[3], float (&v_L)[3]) {
    const float X10 = X01, G10 = G01;
    const float N00 = -X00, N01 = -X01, N10 = -X10, N11 = -X11;
    const float P00 = N00 * G00 + N10 * G01;
    const float P01 = N01 * G00 + N11 * G01;
    const float P10 = N00 * G10 + N10 * G11;
    const float P11 = N01 * G10 + N11 * G11;
    const float V00 = P00 * X00 + P10 * X01;
    const float V01 = P01 * X00 + P11 * X01;
    const float V10 = P00 * X10 + P10 * X11;
    const float V11 = P01 * X10 + P11 * X11;
    const float g11 = V00, g12 = V10 + V01, g22 = V11;
    v_cov2d[0] = g11;
    v_cov2d[1] = g12;
    v_cov2d[2] = g22;
    v_L[0] = 2.0f * l11 * g11 + 2.0f * g12 * l21;  // doubled cross term: backward2d.cu:39
    v_L[1] = 2.0f * l11 * g12 + 2.0f * l21 * g22;
    v_L[2] = 2.0f * l22 * g22;
}

}  // namespace gsvc
