// wm::affine, wm::rotate, wm::rotate_attack and wm::unrotate of include/ssw.hpp against the C calls they wrap
// (tests/test_rotate_gpu.py builds and runs it): two 33 x 17 frames and an original, a shrink into 16 x 8, a rotation, three
// attack jobs and two suspects turned back, every byte.  Prints the six entries of rotation_matrix(1.5, 33, 17) as hexadecimal
// floats for the Python test to hold against Python's, then "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ssw.hpp"

#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

int main() {
    const size_t w = 33, h = 17, fb = w * h * 3;
    wm::Context ctx(0);
    wm::ImageRgb8 a(w, h), b(w, h), orig(w, h);
    uint32_t s = 12345;
    for (size_t i = 0; i < fb; ++i) {
        s = s * 1664525u + 1013904223u;
        a.data[i] = (uint8_t)(s >> 24);
        b.data[i] = (uint8_t)((i / 3 % w + i / 3 / w) % 2 ? 255 : 0);
        orig.data[i] = (uint8_t)(255 - a.data[i]);
    }
    const std::vector<const wm::ImageRgb8*> frames{&a, &b};
    std::vector<uint8_t> host(3 * fb);
    std::copy(a.data.begin(), a.data.end(), host.begin());
    std::copy(b.data.begin(), b.data.end(), host.begin() + fb);
    std::copy(orig.data.begin(), orig.data.end(), host.begin() + 2 * fb);
    uint8_t *dev = nullptr, *out = nullptr;
    CHECK(ssw_dev_alloc(ctx.get(), 3 * fb, (void**)&dev) == SSW_OK && ssw_dev_alloc(ctx.get(), 3 * fb, (void**)&out) == SSW_OK, "alloc");
    CHECK(ssw_copy_to_dev(ctx.get(), dev, host.data(), 3 * fb) == SSW_OK, "copy");
    const uint8_t* dev_orig = dev + 2 * fb;
    std::vector<uint8_t> got(3 * fb);

    const wm::Matrix m = wm::rotation_matrix(1.5, w, h);
    std::printf("%a %a %a %a %a %a\n", m[0], m[1], m[2], m[3], m[4], m[5]);

    const size_t ow = 16, oh = 8, ob = ow * oh * 3;
    const wm::Matrix shrink{{2.0, 0.0, 0.5, 0.0, 2.0, 0.25}};
    const std::array<uint8_t, 3> fill{{255, 0, 255}};
    const std::vector<wm::ImageRgb8> small = wm::affine(ctx, frames, ow, oh, shrink, wm::AffineFilter::Bilinear, fill);
    CHECK(small.size() == 2 && small[0].width == ow && small[0].height == oh && small[1].data.size() == ob, "affine: shapes");
    CHECK(ssw_affine_rgb8(ctx.get(), dev, 2, w, h, ow, oh, shrink.data(), SSW_AFFINE_BILINEAR, fill.data(), out) == SSW_OK, "ssw_affine_rgb8");
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 2 * ob) == SSW_OK, "copy back");
    for (size_t f = 0; f < 2; ++f)
        for (size_t i = 0; i < ob; ++i) CHECK(small[f].data[i] == got[f * ob + i], "affine: bytes");

    const std::vector<wm::ImageRgb8> turned = wm::rotate(ctx, frames, 1.5, wm::AffineFilter::Bicubic, fill);
    CHECK(ssw_affine_rgb8(ctx.get(), dev, 2, w, h, w, h, m.data(), SSW_AFFINE_BICUBIC, fill.data(), out) == SSW_OK, "ssw_affine_rgb8 (rotation)");
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 2 * fb) == SSW_OK, "copy back");
    for (size_t f = 0; f < 2; ++f)
        for (size_t i = 0; i < fb; ++i) CHECK(turned[f].data[i] == got[f * fb + i], "rotate: bytes");
    const wm::ImageRgb8 far = wm::rotate(ctx, frames, 30.0, wm::AffineFilter::Bilinear, fill).at(0);
    CHECK(far.data[0] == 255 && far.data[1] == 0 && far.data[2] == 255, "rotate: at 30 degrees the corner is the fill");
    CHECK(wm::rotate(ctx, frames, 0.0).at(1).data == b.data, "rotate: angle 0 is the frame");

    const std::vector<wm::Rotate> jobs{wm::Rotate{1, 1.5}, wm::Rotate{0, -30.0, wm::AffineFilter::Bilinear, fill}, wm::Rotate{1, 0.0}};
    const std::vector<wm::ImageRgb8> back = wm::rotate_attack(ctx, orig, frames, jobs);
    CHECK(back.size() == 3 && back[0].width == w && back[2].height == h, "rotate_attack: shapes");
    ssw_rotate_job cj[3];
    for (int j = 0; j < 3; ++j) cj[j] = jobs[j].job(w, h);
    CHECK(cj[1].frame == 0 && cj[1].filter == SSW_AFFINE_BILINEAR && cj[1].fill[0] == 255 && cj[0].forward[0] == m[0] && cj[0].forward[5] == m[5], "Rotate::job");
    const wm::Matrix mb = wm::rotation_matrix(-1.5, w, h);
    for (int i = 0; i < 6; ++i) CHECK(cj[0].back[i] == mb[i], "Rotate::job: the way back is the matrix of the negative angle");
    CHECK(ssw_rotate_attack_rgb8(ctx.get(), dev_orig, dev, 2, w, h, cj, 3, out) == SSW_OK, "ssw_rotate_attack_rgb8");
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 3 * fb) == SSW_OK, "copy back");
    for (size_t j = 0; j < 3; ++j)
        for (size_t i = 0; i < fb; ++i) CHECK(back[j].data[i] == got[j * fb + i], "rotate_attack: bytes");
    CHECK(back[2].data == b.data, "rotate_attack: angle 0 is a copy");
    CHECK(back[0].data[0] == orig.data[0] && back[0].data != b.data && back[0].data != orig.data, "rotate_attack: the corner is the original's");

    const std::vector<const wm::ImageRgb8*> suspects{&turned[0], &turned[1]};
    const std::vector<wm::ImageRgb8> undone = wm::unrotate(ctx, orig, suspects, {1.5, 1.5});
    CHECK(ssw_copy_to_dev(ctx.get(), dev, turned[0].data.data(), fb) == SSW_OK && ssw_copy_to_dev(ctx.get(), dev + fb, turned[1].data.data(), fb) == SSW_OK, "copy");
    const ssw_rotate_job uj[2] = {wm::Rotate{0, 1.5}.job(w, h), wm::Rotate{1, 1.5}.job(w, h)};
    CHECK(ssw_unrotate_rgb8(ctx.get(), dev_orig, dev, 2, w, h, uj, out) == SSW_OK, "ssw_unrotate_rgb8");
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 2 * fb) == SSW_OK, "copy back");
    for (size_t j = 0; j < 2; ++j)
        for (size_t i = 0; i < fb; ++i) CHECK(undone[j].data[i] == got[j * fb + i], "unrotate: bytes");
    CHECK(undone[1].data == back[0].data, "unrotate of a rotation = that attack job");
    ssw_dev_free(ctx.get(), dev);
    ssw_dev_free(ctx.get(), out);
    std::printf("ok\n");
    return 0;
}
