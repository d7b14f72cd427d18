// The tile of a turned plane, shared by angle_cost_kernel, angle_cost_shared_kernel (angle.hip), turned_template_kernel
// (locate_turned.hip) and tests/cpp/turned_tile_test.cpp; the arithmetic compiles without HIP.  include/ssw.h states the two maps
// (ssw_find_angle_rgb8: the original's plane turned forward; ssw_locate_turned_rgb8: the suspect's luma turned back); both are
//     p  = 2 f X + f - dw                         q  = 2 f Y + f - dh
//     Rx = (sw - f) * 65536 + C p + S q           Ry = (sh - f) * 65536 - S p + C q
//     X0 = Rx >> shift, fx = (Rx >> (shift - 8)) & 255; Y0, fy likewise of Ry                (arithmetic shifts)
// for pixel (X, Y) of a destination plane, with the taps (X0, Y0) .. (X0 + 1, Y0 + 1) of a source plane: the angle search has
// sw x sh = dw x dh, the template f = 1, a template of its own size and the opposite sign of S -- as data, see Turn.
//
// A block of TURN_THREADS threads takes a tile of TURN_TILE_W x TURN_TILE_H destination pixels.  Rx and Ry are monotone in X and
// in Y, so the sample points of the tile's four corners bound the box of the source plane the tile can touch: the box is staged in
// LDS and all four taps come from there.  The tile's origin is formed in 64 bits (at 20 000 pixels C p passes 2^31), the box's
// origin subtracted, and a pixel adds its own offset in 32 bits -- integer adds, exact.
//
// The box.  The sample points of a tile spread over 2 f 31 (C + |S|) / 2^shift = 31 (C + |S|) / 65536 <= 31 sqrt(2) = 43.9 source
// pixels across and down (at 45 degrees): their floors take at most 45 values, the second tap adds one -- 46 x 46, rows padded to
// 48.  turned_tile_test checks that for every angle, both factors and both signs, and that no 32-bit quantity below overflows.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SSW_TILE_HD __host__ __device__ __forceinline__
#else
#define SSW_TILE_HD inline
#endif

namespace ssw {

constexpr unsigned TURN_TILE_W = 32, TURN_TILE_H = 32, TURN_THREADS = 256;
constexpr unsigned TURN_BOX_W = 48, TURN_BOX_H = 46;

// One turn: sizes in full-resolution pixels; the planes are 1 / f of them
struct Turn {
    int32_t C, S;                // the angle search: C(a), S(a); the template of angle n: C(n), -S(n)
    uint32_t f, shift;           // 1, 17 or 4, 19
    uint32_t sw, sh, dw, dh;     // source and destination
};

// A tile of it: the origin, the box of the source plane (columns bx0 .. bx1, rows by0 .. by1; bw x bh of it are staged) and the
// origin as the box sees it
struct TurnedTile {
    int64_t Rx0, Ry0, bx0, bx1, by0, by1;
    int32_t bw, bh, lrx0, lry0;
};

SSW_TILE_HD int64_t turn_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
SSW_TILE_HD int32_t turn_min(int32_t a, int32_t b) { return a < b ? a : b; }
SSW_TILE_HD int32_t turn_max(int32_t a, int32_t b) { return a > b ? a : b; }

// the tile whose first pixel is (Xt, Yt) of the destination plane, nx x ny pixels of it in use
SSW_TILE_HD TurnedTile turned_tile(const Turn& m, uint32_t Xt, uint32_t Yt, int nx, int ny) {
    TurnedTile tl;
    const int32_t C = m.C, S = m.S;
    const int64_t f = m.f;
    const int64_t p0 = 2 * f * Xt + f - (int64_t)m.dw, q0 = 2 * f * Yt + f - (int64_t)m.dh;
    tl.Rx0 = ((int64_t)m.sw - f) * 65536 + C * p0 + S * q0;
    tl.Ry0 = ((int64_t)m.sh - f) * 65536 - S * p0 + C * q0;
    // the four corners' offsets from it bound every pixel's: 2 f (C dx + S dy) and 2 f (-S dx + C dy)
    const int32_t f2 = 2 * (int32_t)m.f, ex = f2 * (nx - 1), ey = f2 * (ny - 1);
    const int32_t cxx = C * ex, sxy = S * ey, syx = -S * ex, cyy = C * ey;
    const int32_t oxmin = turn_min(0, cxx) + turn_min(0, sxy), oxmax = turn_max(0, cxx) + turn_max(0, sxy);
    const int32_t oymin = turn_min(0, syx) + turn_min(0, cyy), oymax = turn_max(0, syx) + turn_max(0, cyy);
    tl.bx0 = (tl.Rx0 + oxmin) >> m.shift; tl.bx1 = ((tl.Rx0 + oxmax) >> m.shift) + 1;
    tl.by0 = (tl.Ry0 + oymin) >> m.shift; tl.by1 = ((tl.Ry0 + oymax) >> m.shift) + 1;
    tl.bw = (int32_t)turn_clamp(tl.bx1 - tl.bx0 + 1, 2, TURN_BOX_W);       // (the bound holds: the clamp never bites)
    tl.bh = (int32_t)turn_clamp(tl.by1 - tl.by0 + 1, 2, TURN_BOX_H);
    tl.lrx0 = (int32_t)(tl.Rx0 - tl.bx0 * ((int64_t)1 << m.shift));
    tl.lry0 = (int32_t)(tl.Ry0 - tl.by0 * ((int64_t)1 << m.shift));
    return tl;
}

// pixel (dx, dy) of the tile as the box sees it: local X0 = lrx >> shift, fx = (lrx >> (shift - 8)) & 255; Y0, fy likewise
SSW_TILE_HD void turned_pixel(const Turn& m, const TurnedTile& tl, int dx, int dy, int32_t* lrx, int32_t* lry) {
    const int32_t f2 = 2 * (int32_t)m.f;
    *lrx = tl.lrx0 + f2 * (m.C * dx + m.S * dy);
    *lry = tl.lry0 + f2 * (m.C * dy - m.S * dx);
}
SSW_TILE_HD uint32_t turned_frac(const Turn& m, int32_t lr) { return (uint32_t)(lr >> (m.shift - 8)) & 255u; }

// the bilinear tap
SSW_TILE_HD uint32_t turned_tap(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, uint32_t fx, uint32_t fy) {
    return ((256u - fx) * (256u - fy) * v00 + fx * (256u - fy) * v01 + (256u - fx) * fy * v10 + fx * fy * v11 + 32768u) >> 16;
}

#if defined(__HIPCC__)
using TurnedBox = uint8_t[TURN_BOX_H][TURN_BOX_W];

// The block stages the tile's box of the plane [ph][pitch] (pw bytes of a row in use); positions outside the plane become 0.
// Ends with the block's barrier.
__device__ __forceinline__ void turned_stage(TurnedBox& s_box, const uint8_t* __restrict__ plane, uint32_t pitch, uint32_t pw, uint32_t ph,
                                             const TurnedTile& tl) {
    for (int i = (int)threadIdx.x; i < tl.bw * tl.bh; i += (int)TURN_THREADS) {
        const int r = i / tl.bw, c = i - r * tl.bw;
        const int64_t gx = tl.bx0 + c, gy = tl.by0 + r;
        const bool in = gx >= 0 && gx < (int64_t)pw && gy >= 0 && gy < (int64_t)ph;
        s_box[r][c] = in ? plane[(size_t)gy * pitch + (size_t)gx] : (uint8_t)0;
    }
    __syncthreads();
}

// the value at (lrx, lry), whose local (X0, Y0) the caller has found inside 0 .. bw - 2, 0 .. bh - 2
__device__ __forceinline__ uint32_t turned_value(const TurnedBox& s_box, const Turn& m, int32_t X0, int32_t Y0, int32_t lrx, int32_t lry) {
    return turned_tap(s_box[Y0][X0], s_box[Y0][X0 + 1], s_box[Y0 + 1][X0], s_box[Y0 + 1][X0 + 1], turned_frac(m, lrx), turned_frac(m, lry));
}
#endif

}  // namespace ssw
