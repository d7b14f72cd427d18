// The bound that the staged box of csrc/turned_tile.hpp rests on, as a stand-alone program: the box of every tile fits
// TURN_BOX_W x TURN_BOX_H (the clamp never bites), a pixel's taps computed in 32 bits from the box's origin are the definition's of
// include/ssw.h computed in 64 bits, they lie inside the staged box, and no 32-bit quantity leaves int32.
//   turned_tile_test     "turned tile: ok (N tiles, M pixels)", or the first offending case on stderr and exit status 1
//
// Cases.  Every angle n = -1440 .. 1440; both levels (f = 1, shift 17; f = 4, shift 19); both signs of S; tile extents (nx, ny) in
// {1, 8, 31, 32}^2; the first and the last tile of the frames below.  With S as angle_table gives it a case is the cost map of
// ssw_find_angle_rgb8, with -S and f = 1 the template map of ssw_locate_turned_rgb8 (the other two combinations are the same
// arithmetic and run as well).  The template's sizes differ: a 70 x 66 suspect with the template size of the angle (angles that
// have no template are skipped there).
// Pixels.  The four corners of every tile of every case; ALL pixels of the tile for the angles 0, +-1, +-1439, +-1440 and the
// multiples of 45 / 8 degrees (n = 180 k) -- the full product takes minutes under the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "turned_tables.hpp"
#include "turned_tile.hpp"

namespace {

using namespace ssw;

struct Case { int32_t n; Turn m; uint32_t Xt, Yt; int nx, ny; };
unsigned long long g_tiles = 0, g_pixels = 0;

[[noreturn]] void fail(const Case& c, const char* what, long long a, long long b, int dx = -1, int dy = -1) {
    std::fprintf(stderr, "turned tile: %s (%lld, %lld) at n %d C %d S %d f %u shift %u source %u x %u destination %u x %u tile %u,%u extent %d x %d pixel %d,%d\n",
                 what, a, b, (int)c.n, (int)c.m.C, (int)c.m.S, c.m.f, c.m.shift, c.m.sw, c.m.sh, c.m.dw, c.m.dh, c.Xt, c.Yt, c.nx, c.ny, dx, dy);
    std::exit(1);
}
bool fits32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

// the definition: the sample point of pixel (X, Y) of the destination plane
void point(const Turn& m, int64_t X, int64_t Y, int64_t* Rx, int64_t* Ry) {
    const int64_t f = m.f, p = 2 * f * X + f - (int64_t)m.dw, q = 2 * f * Y + f - (int64_t)m.dh;
    *Rx = ((int64_t)m.sw - f) * 65536 + (int64_t)m.C * p + (int64_t)m.S * q;
    *Ry = ((int64_t)m.sh - f) * 65536 - (int64_t)m.S * p + (int64_t)m.C * q;
}

void check_pixel(const Case& c, const TurnedTile& tl, int dx, int dy) {
    const Turn& m = c.m;
    // the 32-bit path beside itself in 64 bits
    const int64_t f2 = 2 * (int64_t)m.f;
    const int64_t cx = (int64_t)m.C * dx, sy = (int64_t)m.S * dy, cy = (int64_t)m.C * dy, sx = (int64_t)m.S * dx;
    const int64_t wide[] = {cx, sy, cy, sx, cx + sy, cy - sx, f2 * (cx + sy), f2 * (cy - sx), tl.lrx0 + f2 * (cx + sy), tl.lry0 + f2 * (cy - sx)};
    for (int64_t v : wide)
        if (!fits32(v)) fail(c, "a pixel's 32-bit quantity overflows", v, 0, dx, dy);
    int32_t lrx = 0, lry = 0;
    turned_pixel(m, tl, dx, dy, &lrx, &lry);
    if (lrx != wide[8] || lry != wide[9]) fail(c, "the 32-bit offsets are not the 64-bit ones", lrx, lry, dx, dy);
    // the definition
    int64_t Rx = 0, Ry = 0;
    point(m, (int64_t)c.Xt + dx, (int64_t)c.Yt + dy, &Rx, &Ry);
    if (m.f == 1) {                                                     // ... which at f = 1 is the template's of the opposite S
        int64_t Tx = 0, Ty = 0;
        turned_point(m.sw, m.sh, m.C, -m.S, m.dw, m.dh, (int64_t)c.Xt + dx, (int64_t)c.Yt + dy, &Tx, &Ty);
        if (Tx != Rx || Ty != Ry) fail(c, "the template's point differs", Tx, Ty, dx, dy);
    }
    const int32_t X0 = lrx >> m.shift, Y0 = lry >> m.shift;
    if ((Rx >> m.shift) != tl.bx0 + X0 || (Ry >> m.shift) != tl.by0 + Y0) fail(c, "X0, Y0 differ from the definition's", Rx >> m.shift, Ry >> m.shift, dx, dy);
    if ((uint32_t)((Rx >> (m.shift - 8)) & 255) != turned_frac(m, lrx) || (uint32_t)((Ry >> (m.shift - 8)) & 255) != turned_frac(m, lry))
        fail(c, "fx, fy differ from the definition's", turned_frac(m, lrx), turned_frac(m, lry), dx, dy);
    if (X0 < 0 || X0 > tl.bw - 2 || Y0 < 0 || Y0 > tl.bh - 2) fail(c, "a tap outside the staged box", X0, Y0, dx, dy);
    ++g_pixels;
}

void check_tile(const Case& c, bool every_pixel) {
    const Turn& m = c.m;
    // the tile's own 32-bit quantities, in 64 bits
    const int64_t f2 = 2 * (int64_t)m.f, ex = f2 * (c.nx - 1), ey = f2 * (c.ny - 1);
    const int64_t cxx = m.C * ex, sxy = m.S * ey, syx = -(int64_t)m.S * ex, cyy = m.C * ey;
    for (int64_t v : {cxx, sxy, syx, cyy, cxx + sxy, syx + cyy})
        if (!fits32(v)) fail(c, "a corner's 32-bit quantity overflows", v, 0);
    const TurnedTile tl = turned_tile(m, c.Xt, c.Yt, c.nx, c.ny);
    int64_t Rx = 0, Ry = 0;
    point(m, c.Xt, c.Yt, &Rx, &Ry);
    if (Rx != tl.Rx0 || Ry != tl.Ry0) fail(c, "the origin differs from the definition's", tl.Rx0, tl.Ry0);
    if (tl.bx1 - tl.bx0 + 1 > (int64_t)TURN_BOX_W || tl.by1 - tl.by0 + 1 > (int64_t)TURN_BOX_H) fail(c, "the box is larger than the staged one", tl.bx1 - tl.bx0 + 1, tl.by1 - tl.by0 + 1);
    if (tl.bw != tl.bx1 - tl.bx0 + 1 || tl.bh != tl.by1 - tl.by0 + 1) fail(c, "the clamp bites", tl.bw, tl.bh);
    const int64_t one = (int64_t)1 << m.shift;
    if (!fits32(tl.Rx0 - tl.bx0 * one) || !fits32(tl.Ry0 - tl.by0 * one) || tl.lrx0 != tl.Rx0 - tl.bx0 * one || tl.lry0 != tl.Ry0 - tl.by0 * one)
        fail(c, "the local origin overflows", tl.Rx0 - tl.bx0 * one, tl.Ry0 - tl.by0 * one);
    ++g_tiles;
    if (every_pixel) {
        for (int dy = 0; dy < c.ny; ++dy)
            for (int dx = 0; dx < c.nx; ++dx) check_pixel(c, tl, dx, dy);
    } else {
        for (int k = 0; k < 4; ++k) check_pixel(c, tl, (k & 1) ? c.nx - 1 : 0, (k & 2) ? c.ny - 1 : 0);
    }
}

// the first and the last tile of the destination plane, at every extent
void check_turn(int32_t n, const Turn& m, bool every_pixel) {
    const uint32_t wr = m.dw / m.f, hr = m.dh / m.f;
    const uint32_t Xl = (wr - 1) / TURN_TILE_W * TURN_TILE_W, Yl = (hr - 1) / TURN_TILE_H * TURN_TILE_H;
    for (int nx : {1, 8, 31, 32})
        for (int ny : {1, 8, 31, 32}) {
            check_tile(Case{n, m, 0, 0, nx, ny}, every_pixel);
            check_tile(Case{n, m, Xl, Yl, nx, ny}, every_pixel);
        }
}

}  // namespace

int main() {
    const uint32_t frames[][2] = {{32, 32}, {65, 41}, {20000, 32}, {32, 20000}, {65535, 64}};
    for (int32_t n = -1440; n <= 1440; ++n) {
        const bool every_pixel = n == 0 || n == 1 || n == -1 || n == 1439 || n == -1439 || n % 180 == 0;
        int32_t C = 0, S = 0;
        angle_table(n, &C, &S);
        for (int level = 0; level < 2; ++level)
            for (int sign = 1; sign >= -1; sign -= 2) {
                const uint32_t f = level ? 4 : 1, shift = level ? 19 : 17;
                for (const auto& fr : frames) check_turn(n, Turn{C, sign * S, f, shift, fr[0], fr[1], fr[0], fr[1]}, every_pixel);
                uint32_t tw = 0, th = 0;
                if (turned_template_size(70, 66, n, &tw, &th)) check_turn(n, Turn{C, sign * S, f, shift, 70, 66, tw, th}, every_pixel);
            }
    }
    std::printf("turned tile: ok (%llu tiles, %llu pixels)\n", g_tiles, g_pixels);
    return 0;
}
