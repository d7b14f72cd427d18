// wm::crop_attack and wm::crop_search_attack of include/ssw_crop.hpp over the stubs (crop_stub.cpp for the two new C functions,
// ssw_stub.cpp for the rest): argument order, the packed thumbnails and their sizes, the optional output, the answers of a
// search, and a thrown status with nothing left alive.  tests/test_crop_cpp_cpu.py builds and runs it, plain and under ASan/UBSan.
#include <cstdio>
#include <vector>

#include "ssw_crop.hpp"

extern "C" {
double crop_stub_last(size_t k);
void crop_stub_fail(int status);
uint64_t crop_stub_checksum(void);
void ssw_stub_live(size_t out[5]);
}

#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

static bool nothing_but_the_context() {
    size_t live[5];
    ssw_stub_live(live);
    return live[0] == 0 && live[1] == 0 && live[2] == 1 && live[3] == 0 && live[4] == 0;
}

int main() {
    const size_t w = 37, h = 33, fb = w * h * 3;
    {
        wm::Context ctx(0);
        wm::ImageRgb8 orig(w, h), a(w, h), b(w, h);
        for (size_t i = 0; i < fb; ++i) { orig.data[i] = (uint8_t)(i * 7 + 3); a.data[i] = (uint8_t)(i + 10); b.data[i] = (uint8_t)(i * 3 + 150); }
        const std::vector<const wm::ImageRgb8*> frames{&a, &b};
        const wm::ImageRgb8* img[2] = {&a, &b};
        // three jobs: frame 1 unscaled, frame 0 as a thumbnail, frame 1 again as a 1 x 1 piece
        std::vector<wm::Crop> jobs(3);
        jobs[0].frame = 1; jobs[0].x = 3; jobs[0].y = 2; jobs[0].cw = 11; jobs[0].ch = 7;
        jobs[1].frame = 0; jobs[1].x = 0; jobs[1].y = 1; jobs[1].cw = 37; jobs[1].ch = 32; jobs[1].tw = 5; jobs[1].th = 9; jobs[1].filter = wm::ResampleFilter::Lanczos;
        jobs[2].frame = 1; jobs[2].x = 36; jobs[2].y = 32; jobs[2].cw = 1; jobs[2].ch = 1;
        const size_t tw[3] = {11, 5, 1}, th[3] = {7, 9, 1};

        const wm::Cropped r = wm::crop_attack(ctx, orig, frames, jobs, true);
        CHECK(crop_stub_last(0) == 2 && crop_stub_last(1) == (double)w && crop_stub_last(2) == (double)h && crop_stub_last(3) == 3, "n_frames, w, h, n_jobs");
        CHECK(crop_stub_last(4) == 1.0 && crop_stub_last(5) == 0.0, "thumbnails asked for, not searched");
        CHECK(crop_stub_last(6) == 36 && crop_stub_last(7) == 32 && crop_stub_last(8) == 1 && crop_stub_last(9) == 1 && crop_stub_last(10) == 0 &&
              crop_stub_last(11) == 0 && crop_stub_last(12) == 0, "the last job's rectangle, unscaled");
        CHECK(r.frames.size() == 3 && r.thumbs.size() == 3 && r.found.empty(), "one entry per job; no answers of a search");
        for (size_t i = 0; i < 3; ++i) {
            const wm::ImageRgb8& src = *img[jobs[i].frame];
            CHECK(r.frames[i].width == w && r.frames[i].height == h && r.frames[i].data.size() == fb, "frames of the original's size");
            for (size_t k = 0; k < fb; ++k) CHECK(r.frames[i].data[k] == (uint8_t)(src.data[k] ^ 0x3C), "job i is made of its frame");
            CHECK(r.thumbs[i].width == tw[i] && r.thumbs[i].height == th[i] && r.thumbs[i].data.size() == tw[i] * th[i] * 3, "a thumbnail's size");
            const uint8_t first = src.data[(jobs[i].y * w + jobs[i].x) * 3];
            for (size_t k = 0; k < r.thumbs[i].data.size(); ++k) CHECK(r.thumbs[i].data[k] == (uint8_t)(first + k + i), "thumbnails packed in job order");
        }
        CHECK(nothing_but_the_context(), "its device blocks are freed");

        const uint64_t before = crop_stub_checksum();
        const wm::Cropped s = wm::crop_attack(ctx, orig, frames, {jobs[1]});
        CHECK(s.frames.size() == 1 && s.thumbs.empty() && s.found.empty(), "no thumbnails unless asked for");
        CHECK(crop_stub_last(3) == 1 && crop_stub_last(4) == 0.0 && crop_stub_last(10) == 5 && crop_stub_last(11) == 9 && crop_stub_last(12) == 3.0, "a thumbnail, lanczos");
        CHECK(crop_stub_checksum() != before, "one job");
        CHECK(wm::crop_attack(ctx, orig, frames, {}).frames.empty() && crop_stub_last(3) == 1, "no jobs, no call");

        // searched: every piece at its own size by default; ranges go with their jobs
        const wm::Cropped q = wm::crop_search_attack(ctx, orig, frames, jobs);
        CHECK(crop_stub_last(5) == 1.0 && crop_stub_last(13) == 0 && crop_stub_last(14) == 0 && crop_stub_last(4) == 0.0, "searched, own size, no thumbnails");
        CHECK(q.frames.size() == 3 && q.found.size() == 3 && q.thumbs.empty(), "one answer per job");
        for (size_t i = 0; i < 3; ++i) {
            CHECK(q.found[i].placement.x == jobs[i].x + 1 && q.found[i].placement.y == jobs[i].y + 2 && q.found[i].placement.w == tw[i] &&
                  q.found[i].placement.h == th[i], "x, y, pw, ph in their places");
            CHECK(q.found[i].sad == 1000 * i + jobs[i].cw && q.found[i].mean_abs_diff == (double)q.found[i].sad / (double)(tw[i] * th[i]), "sad and its mean");
        }
        std::vector<wm::CropSearch> ranges(3);
        ranges[1].wmin = 32; ranges[1].wmax = 37;
        ranges[2].wmin = 40; ranges[2].wmax = 50;
        const wm::Cropped t = wm::crop_search_attack(ctx, orig, frames, jobs, ranges, true);
        CHECK(crop_stub_last(13) == 40 && crop_stub_last(14) == 50 && crop_stub_last(4) == 1.0, "the last range; thumbnails asked for");
        CHECK(t.found[0].placement.w == 11 && t.found[1].placement.w == 37 && t.found[1].placement.h == 32 && t.found[2].placement.w == 50, "ranges go with their jobs");
        CHECK(t.thumbs.size() == 3 && t.thumbs[1].data.size() == 5 * 9 * 3 && t.thumbs[2].data[0] == (uint8_t)(b.data[(32 * w + 36) * 3] + 2), "thumbnails of a search");
        CHECK(nothing_but_the_context(), "its device blocks are freed");

        // a thrown status, nothing left alive
        for (int pass = 0; pass < 6; ++pass) {
            bool thrown = false;
            try {
                if (pass == 0) { crop_stub_fail(SSW_ERR_OUT_OF_MEMORY); wm::crop_attack(ctx, orig, frames, jobs, true); }
                if (pass == 1) { crop_stub_fail(SSW_ERR_UNSUPPORTED); wm::crop_search_attack(ctx, orig, frames, jobs, ranges, true); }
                if (pass == 2) { wm::ImageRgb8 odd(w + 1, h); wm::crop_attack(ctx, orig, {&a, &odd}, jobs); }      // a frame of another size
                if (pass == 3) { std::vector<wm::Crop> far(1, jobs[0]); far[0].frame = 2; wm::crop_attack(ctx, orig, frames, far); }      // no such frame
                if (pass == 4) { std::vector<wm::Crop> out(1, jobs[0]); out[0].x = 27; wm::crop_search_attack(ctx, orig, frames, out); }      // the rectangle leaves the frame
                if (pass == 5) wm::crop_search_attack(ctx, orig, frames, jobs, std::vector<wm::CropSearch>(2));      // two ranges for three jobs
            } catch (const wm::Error& e) {
                thrown = true;
                CHECK(e.status() == (pass == 0 ? SSW_ERR_OUT_OF_MEMORY : pass == 1 ? SSW_ERR_UNSUPPORTED : pass == 2 ? SSW_ERR_BAD_DIMS : SSW_ERR_BAD_ARG),
                      "the status that was thrown");
            }
            CHECK(thrown && nothing_but_the_context(), "a thrown status leaves nothing alive");
        }
    }
    size_t live[5];
    ssw_stub_live(live);
    CHECK(live[2] == 0, "the context is gone");
    std::printf("crop wrappers: ok\n");
    return 0;
}
