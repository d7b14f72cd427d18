// wm::resample and wm::scale_attack of include/ssw.hpp against the C calls they wrap (tests/test_resample_gpu.py builds and runs
// it): two 33 x 17 frames, a thumbnail of 16 x 8 by LANCZOS and three scale jobs, every byte.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ssw.hpp"

#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

int main() {
    const size_t w = 33, h = 17, fb = w * h * 3;
    wm::Context ctx(0);
    wm::ImageRgb8 a(w, h), b(w, h);
    uint32_t s = 12345;
    for (size_t i = 0; i < fb; ++i) {
        s = s * 1664525u + 1013904223u;
        a.data[i] = (uint8_t)(s >> 24);
        b.data[i] = (uint8_t)((i / 3 % w + i / 3 / w) % 2 ? 255 : 0);
    }
    const std::vector<const wm::ImageRgb8*> frames{&a, &b};
    std::vector<uint8_t> host(2 * fb);
    std::copy(a.data.begin(), a.data.end(), host.begin());
    std::copy(b.data.begin(), b.data.end(), host.begin() + fb);
    uint8_t *dev = nullptr, *out = nullptr;
    CHECK(ssw_dev_alloc(ctx.get(), 2 * fb, (void**)&dev) == SSW_OK && ssw_dev_alloc(ctx.get(), 3 * fb, (void**)&out) == SSW_OK, "alloc");
    CHECK(ssw_copy_to_dev(ctx.get(), dev, host.data(), 2 * fb) == SSW_OK, "copy");

    const size_t nw = 16, nh = 8, ob = nw * nh * 3;
    const std::vector<wm::ImageRgb8> small = wm::resample(ctx, frames, nw, nh, wm::ResampleFilter::Lanczos);
    CHECK(small.size() == 2 && small[0].width == nw && small[0].height == nh && small[1].data.size() == ob, "resample: shapes");
    CHECK(ssw_resample_rgb8(ctx.get(), dev, 2, w, h, nw, nh, SSW_RESAMPLE_LANCZOS, out) == SSW_OK, "ssw_resample_rgb8");
    std::vector<uint8_t> got(3 * fb);
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 2 * ob) == SSW_OK, "copy back");
    for (size_t f = 0; f < 2; ++f)
        for (size_t i = 0; i < ob; ++i) CHECK(small[f].data[i] == got[f * ob + i], "resample: bytes");
    CHECK(wm::resample(ctx, frames, w, h).at(1).data == b.data, "resample: the same size is a copy");

    const wm::Scale half = wm::Scale::by(1, w, h, 0.5);
    CHECK(half.frame == 1 && half.nw == 17 && half.nh == 9 && half.filter == wm::ResampleFilter::Bicubic, "Scale::by rounds half up");
    const std::vector<wm::Scale> jobs{half, wm::Scale{0, 40, 5, wm::ResampleFilter::Box}, wm::Scale{1, 33, 17, wm::ResampleFilter::Bilinear}};
    const std::vector<wm::ImageRgb8> back = wm::scale_attack(ctx, frames, jobs);
    CHECK(back.size() == 3 && back[0].width == w && back[2].height == h, "scale_attack: shapes");
    const ssw_scale_job cj[3] = {{1, 17, 9, SSW_RESAMPLE_BICUBIC}, {0, 40, 5, SSW_RESAMPLE_BOX}, {1, 33, 17, SSW_RESAMPLE_BILINEAR}};
    CHECK(ssw_scale_attack_rgb8(ctx.get(), dev, 2, w, h, cj, 3, out) == SSW_OK, "ssw_scale_attack_rgb8");
    CHECK(ssw_copy_to_host(ctx.get(), got.data(), out, 3 * fb) == SSW_OK, "copy back");
    for (size_t j = 0; j < 3; ++j)
        for (size_t i = 0; i < fb; ++i) CHECK(back[j].data[i] == got[j * fb + i], "scale_attack: bytes");
    CHECK(back[2].data == b.data, "scale_attack: the same size is a copy");
    ssw_dev_free(ctx.get(), dev);
    ssw_dev_free(ctx.get(), out);
    std::printf("ok\n");
    return 0;
}
