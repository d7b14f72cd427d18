// wm::locate_turned and wm::restore_turned of include/ssw_turned.hpp over the stubs (turned_stub.cpp for the new C functions,
// ssw_stub.cpp for everything of ssw.hpp): argument order, vector sizes, suspects of mixed sizes, and a thrown status with nothing
// left alive.  tests/test_locate_turned_cpu.py builds and runs it, plain and under ASan/UBSan.
#include <cstdio>
#include <vector>

#include "ssw_turned.hpp"

extern "C" {
double turned_stub_last(size_t k);
void turned_stub_fail(int status);
uint64_t turned_stub_checksum(void);
void ssw_stub_live(size_t out[5]);
}

#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

static bool nothing_but_the_context() {
    size_t live[5];
    ssw_stub_live(live);
    return live[0] == 0 && live[1] == 0 && live[2] == 1 && live[3] == 0 && live[4] == 0;
}

int main() {
    const size_t w = 97, h = 83, fb = w * h * 3;
    {
        wm::Context ctx(0);
        wm::ImageRgb8 orig(w, h), a(64, 64), b(70, 66), c(41, 57);
        for (size_t i = 0; i < fb; ++i) orig.data[i] = (uint8_t)(i * 7 + 3);
        for (size_t i = 0; i < a.data.size(); ++i) a.data[i] = (uint8_t)(i + 10);
        for (size_t i = 0; i < b.data.size(); ++i) b.data[i] = (uint8_t)(i * 3 + 150);
        for (size_t i = 0; i < c.data.size(); ++i) c.data[i] = (uint8_t)(255 - i);
        const std::vector<const wm::ImageRgb8*> suspects{&a, &b, &c};
        const wm::ImageRgb8* img[3] = {&a, &b, &c};

        std::vector<uint64_t> rungs;
        const std::vector<wm::LocatedTurned> f = wm::locate_turned(ctx, orig, suspects, -1.3, 2.0, &rungs);
        CHECK(turned_stub_last(0) == 3 && turned_stub_last(1) == (double)w && turned_stub_last(2) == (double)h, "locate_turned: n, w, h");
        CHECK(turned_stub_last(3) == -1.3 && turned_stub_last(4) == 2.0 && turned_stub_last(5) == 1.0, "locate_turned: amin, amax, the rungs");
        CHECK(f.size() == 3, "locate_turned: one answer per suspect");
        const uint32_t n_rungs = 8 - (-6) + 1;
        CHECK(rungs.size() == 3 * n_rungs * 4, "locate_turned: [suspect][rung][4]");
        for (size_t i = 0; i < 3; ++i) {
            const uint32_t tw = (uint32_t)(img[i]->width / 8 * 8), th = (uint32_t)(img[i]->height / 8 * 8);
            CHECK(f[i].n == (int32_t)img[i]->data[0] - 128 && f[i].angle == (double)f[i].n / 32.0, "locate_turned: suspect i is image i; the angle is n / 32");
            CHECK(f[i].tw == tw && f[i].th == th, "locate_turned: the shapes go with their suspects");
            CHECK(f[i].cx == 10.0 * i + tw / 2.0 && f[i].cy == 10.0 * i + 1 + th / 2.0, "locate_turned: the centre is x + tw / 2, y + th / 2");
            CHECK(f[i].sad == 1000 * i + img[i]->data.back() && f[i].mean == (double)f[i].sad / ((double)tw * th), "locate_turned: sad, mean");
            for (uint32_t r = 0; r < n_rungs; ++r)
                CHECK(rungs[(i * n_rungs + r) * 4 + 2] == 100 * i + 4 * r + 2 && rungs[(i * n_rungs + r) * 4 + 3] == (uint64_t)orig.data[0] + r, "locate_turned: rung entries");
        }
        CHECK(nothing_but_the_context(), "locate_turned: its device blocks are freed");

        const uint64_t before = turned_stub_checksum();
        const std::vector<wm::LocatedTurned> g = wm::locate_turned(ctx, orig, {&b});
        CHECK(g.size() == 1 && turned_stub_last(0) == 1 && turned_stub_last(3) == -10.0 && turned_stub_last(4) == 10.0 && turned_stub_last(5) == 0.0,
              "locate_turned: the default range, no rungs");
        CHECK(g[0].n == (int32_t)b.data[0] - 128 && turned_stub_checksum() != before, "locate_turned: one suspect");
        CHECK(wm::locate_turned(ctx, orig, {}).empty() && turned_stub_last(0) == 1, "locate_turned: no suspects, no call");

        const std::vector<wm::ImageRgb8> back = wm::restore_turned(ctx, orig, suspects, f);
        CHECK(back.size() == 3 && turned_stub_last(0) == 3 && turned_stub_last(1) == (double)w && turned_stub_last(2) == (double)h, "restore_turned: n, w, h");
        CHECK(turned_stub_last(3) == f[0].angle && turned_stub_last(4) == f[2].cy, "restore_turned: the jobs in order");
        for (size_t i = 0; i < 3; ++i) {
            CHECK(back[i].width == w && back[i].height == h && back[i].data.size() == fb, "restore_turned: frames of the original's size");
            CHECK(back[i].data[0] == img[i]->data[0] && back[i].data[1] == orig.data[1], "restore_turned: suspect i over the original");
            CHECK(back[i].data[fb - 1] == (uint8_t)(int)(f[i].angle + f[i].cx + f[i].cy), "restore_turned: job i goes with suspect i");
        }
        const std::vector<wm::ImageRgb8> one = wm::restore_turned(ctx, orig, {&c}, std::vector<ssw_turned_job>{{1.5, 20.25, 30.0}});
        CHECK(one.size() == 1 && one[0].data[fb - 1] == 51 && turned_stub_last(3) == 1.5, "restore_turned: a triple given");
        CHECK(wm::restore_turned(ctx, orig, {}, std::vector<ssw_turned_job>{}).empty(), "restore_turned: no suspects, no call");
        CHECK(nothing_but_the_context(), "restore_turned: its device blocks are freed");

        // a thrown status, nothing left alive
        for (int pass = 0; pass < 5; ++pass) {
            bool thrown = false;
            int want = SSW_ERR_BAD_ARG;
            try {
                if (pass == 0) { want = SSW_ERR_OUT_OF_MEMORY; turned_stub_fail(want); wm::locate_turned(ctx, orig, suspects, -1.0, 1.0, &rungs); }
                if (pass == 1) wm::locate_turned(ctx, orig, suspects, 2.0, 1.0);                 // the library's own refusal
                if (pass == 2) { want = SSW_ERR_BAD_DIMS; wm::ImageRgb8 tiny(30, 30); wm::locate_turned(ctx, orig, {&a, &tiny}); }      // every rung dropped
                if (pass == 3) { want = SSW_ERR_LENGTH_MISMATCH; wm::restore_turned(ctx, orig, suspects, std::vector<ssw_turned_job>{{0.0, 1.0, 1.0}}); }
                if (pass == 4) { want = SSW_ERR_OUT_OF_MEMORY; turned_stub_fail(want); wm::restore_turned(ctx, orig, suspects, f); }
            } catch (const wm::Error& e) {
                thrown = true;
                CHECK(e.status() == want, "the status that was thrown");
            }
            CHECK(thrown && nothing_but_the_context(), "a thrown status leaves nothing alive");
        }
    }
    size_t live[5];
    ssw_stub_live(live);
    CHECK(live[2] == 0, "the context is gone");
    std::printf("turned wrappers: ok\n");
    return 0;
}
