// wm::rotate_search_attack of include/ssw_rotate_search.hpp over the stubs (rotate_search_stub.cpp for the new C function,
// angle_stub.cpp and ssw_stub.cpp for the rest): argument order, vector sizes, the optional outputs, and a thrown status with
// nothing left alive.  tests/test_rotate_search_cpp_cpu.py builds and runs it, plain and under ASan/UBSan.
#include <cstdio>
#include <vector>

#include "ssw_rotate_search.hpp"

extern "C" {
double rotate_search_stub_last(size_t k);
void rotate_search_stub_fail(int status);
uint64_t rotate_search_stub_checksum(void);
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
        // three jobs: frame 1 twice, frame 0 once; the last one bilinear with a fill
        std::vector<wm::Rotate> jobs(3);
        jobs[0].frame = 1; jobs[0].angle = 1.5;
        jobs[1].frame = 0; jobs[1].angle = -2.0;
        jobs[2].frame = 1; jobs[2].angle = 0.25; jobs[2].filter = wm::AffineFilter::Bilinear; jobs[2].fill = {{9, 8, 7}};

        const wm::RotateSearched r = wm::rotate_search_attack(ctx, orig, frames, jobs, -1.3, 2.0, true, true);
        CHECK(rotate_search_stub_last(0) == 2 && rotate_search_stub_last(1) == (double)w && rotate_search_stub_last(2) == (double)h &&
              rotate_search_stub_last(3) == 3, "n_frames, w, h, n_jobs");
        CHECK(rotate_search_stub_last(4) == -1.3 && rotate_search_stub_last(5) == 2.0, "amin, amax");
        CHECK(rotate_search_stub_last(6) == 1.0 && rotate_search_stub_last(7) == 1.0, "the turned frames and the rungs were asked for");
        CHECK(rotate_search_stub_last(8) == 0.0 && rotate_search_stub_last(9) == 0.25 && rotate_search_stub_last(10) == 8.0, "the last job's filter, angle and fill");
        CHECK(r.frames.size() == 3 && r.found.size() == 3 && r.kept.size() == 3 && r.turned.size() == 3, "one entry per job");
        const uint32_t n_rungs = 8 - (-6) + 1;
        CHECK(r.rungs.size() == 3 * n_rungs * 2, "[job][rung][2]");
        for (size_t i = 0; i < 3; ++i) {
            const wm::ImageRgb8& src = *img[jobs[i].frame];
            CHECK(r.frames[i].width == w && r.frames[i].height == h && r.turned[i].data.size() == fb, "frames of the original's size");
            for (size_t k = 0; k < fb; ++k)
                CHECK(r.frames[i].data[k] == (uint8_t)(src.data[k] ^ 0x5A) && r.turned[i].data[k] == (uint8_t)(src.data[k] + 1), "job i is made of its frame; out and turned apart");
            CHECK(r.found[i].n == (int32_t)src.data[0] - 128 && r.found[i].angle == (double)r.found[i].n / 32.0, "the angle is n / 32");
            CHECK(r.found[i].sad == 1000 * i + src.data[fb - 1] && r.found[i].count == w * h, "sad, count");
            CHECK(r.found[i].mean == (double)r.found[i].sad / (double)(w * h), "the mean");
            CHECK(r.kept[i] == (double)(w * h - i) / (double)(w * h), "kept: a share of the frame");
            for (uint32_t k = 0; k < n_rungs; ++k)
                CHECK(r.rungs[(i * n_rungs + k) * 2] == 100 * i + k && r.rungs[(i * n_rungs + k) * 2 + 1] == (uint64_t)orig.data[0] + k, "rung sums");
        }
        CHECK(nothing_but_the_context(), "its device blocks are freed");

        const uint64_t before = rotate_search_stub_checksum();
        const wm::RotateSearched s = wm::rotate_search_attack(ctx, orig, frames, {jobs[1]});
        CHECK(s.frames.size() == 1 && s.turned.empty() && s.rungs.empty(), "no turned frames and no rungs unless asked for");
        CHECK(rotate_search_stub_last(3) == 1 && rotate_search_stub_last(4) == -10.0 && rotate_search_stub_last(5) == 10.0 &&
              rotate_search_stub_last(6) == 0.0 && rotate_search_stub_last(7) == 0.0 && rotate_search_stub_last(8) == 1.0, "the default range, bicubic");
        CHECK(s.found[0].n == (int32_t)a.data[0] - 128 && rotate_search_stub_checksum() != before, "one job");
        CHECK(wm::rotate_search_attack(ctx, orig, frames, {}).frames.empty() && rotate_search_stub_last(3) == 1, "no jobs, no call");

        // a thrown status, nothing left alive
        for (int pass = 0; pass < 4; ++pass) {
            bool thrown = false;
            try {
                if (pass == 0) { rotate_search_stub_fail(SSW_ERR_OUT_OF_MEMORY); wm::rotate_search_attack(ctx, orig, frames, jobs, -1.0, 1.0, true, true); }
                if (pass == 1) wm::rotate_search_attack(ctx, orig, frames, jobs, 2.0, 1.0);                  // the library's own refusal
                if (pass == 2) { wm::ImageRgb8 odd(w + 1, h); wm::rotate_search_attack(ctx, orig, {&a, &odd}, jobs); }      // a frame of another size
                if (pass == 3) { std::vector<wm::Rotate> far(1); far[0].frame = 2; wm::rotate_search_attack(ctx, orig, frames, far); }      // no such frame
            } catch (const wm::Error& e) {
                thrown = true;
                CHECK(e.status() == (pass == 0 ? SSW_ERR_OUT_OF_MEMORY : pass == 2 ? SSW_ERR_BAD_DIMS : SSW_ERR_BAD_ARG), "the status that was thrown");
            }
            CHECK(thrown && nothing_but_the_context(), "a thrown status leaves nothing alive");
        }
        wm::ImageRgb8 tiny(31, 40), tiny2(31, 40);
        bool thrown = false;
        try { wm::rotate_search_attack(ctx, tiny, {&tiny2}, {wm::Rotate{}}); } catch (const wm::Error& e) { thrown = e.status() == SSW_ERR_BAD_DIMS; }
        CHECK(thrown && nothing_but_the_context(), "a side of 31");
    }
    size_t live[5];
    ssw_stub_live(live);
    CHECK(live[2] == 0, "the context is gone");
    std::printf("rotate search wrappers: ok\n");
    return 0;
}
