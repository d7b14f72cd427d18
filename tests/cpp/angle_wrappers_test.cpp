// wm::find_angle and wm::angle_table of include/ssw_angle.hpp over the stubs (angle_stub.cpp for the two new C functions,
// ssw_stub.cpp for everything of ssw.hpp): argument order, vector sizes, and a thrown status with nothing left alive.
// tests/test_angle_cpu.py builds and runs it, plain and under ASan/UBSan.
#include <cstdio>
#include <vector>

#include "ssw_angle.hpp"

extern "C" {
double angle_stub_last(size_t k);
void angle_stub_fail(int status);
uint64_t angle_stub_checksum(void);
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
        wm::ImageRgb8 orig(w, h), a(w, h), b(w, h), c(w, h);
        for (size_t i = 0; i < fb; ++i) { orig.data[i] = (uint8_t)(i * 7 + 3); a.data[i] = (uint8_t)(i + 10); b.data[i] = (uint8_t)(i * 3 + 150); c.data[i] = (uint8_t)(255 - i); }
        const std::vector<const wm::ImageRgb8*> suspects{&a, &b, &c};

        CHECK(wm::angle_table(-5) == std::make_pair((int32_t)65531, (int32_t)5), "angle_table: n, then c and s");

        std::vector<uint64_t> rungs;
        const std::vector<wm::FoundAngle> f = wm::find_angle(ctx, orig, suspects, -1.3, 2.0, &rungs);
        CHECK(angle_stub_last(0) == 3 && angle_stub_last(1) == (double)w && angle_stub_last(2) == (double)h, "find_angle: n, w, h");
        CHECK(angle_stub_last(3) == -1.3 && angle_stub_last(4) == 2.0 && angle_stub_last(5) == 1.0, "find_angle: amin, amax, the rungs");
        CHECK(f.size() == 3, "find_angle: one answer per suspect");
        const uint32_t n_rungs = 8 - (-6) + 1;
        CHECK(rungs.size() == 3 * n_rungs * 2, "find_angle: [suspect][rung][2]");
        const wm::ImageRgb8* img[3] = {&a, &b, &c};
        for (size_t i = 0; i < 3; ++i) {
            CHECK(f[i].n == (int32_t)img[i]->data[0] - 128 && f[i].angle == (double)f[i].n / 32.0, "find_angle: suspect i is frame i; the angle is n / 32");
            CHECK(f[i].sad == 1000 * i + img[i]->data[fb - 1] && f[i].count == w * h, "find_angle: sad, count");
            CHECK(f[i].mean == (double)f[i].sad / (double)(w * h), "find_angle: the mean");
            for (uint32_t r = 0; r < n_rungs; ++r)
                CHECK(rungs[(i * n_rungs + r) * 2] == 100 * i + r && rungs[(i * n_rungs + r) * 2 + 1] == (uint64_t)orig.data[0] + r, "find_angle: rung sums");
        }
        CHECK(nothing_but_the_context(), "find_angle: its device blocks are freed");

        const uint64_t before = angle_stub_checksum();
        const std::vector<wm::FoundAngle> g = wm::find_angle(ctx, orig, {&b});
        CHECK(g.size() == 1 && angle_stub_last(0) == 1 && angle_stub_last(3) == -10.0 && angle_stub_last(4) == 10.0 && angle_stub_last(5) == 0.0,
              "find_angle: the default range, no rungs");
        CHECK(g[0].n == (int32_t)b.data[0] - 128 && angle_stub_checksum() != before, "find_angle: one suspect");
        CHECK(wm::find_angle(ctx, orig, {}).empty() && angle_stub_last(0) == 1, "find_angle: no suspects, no call");

        // a thrown status, nothing left alive
        for (int pass = 0; pass < 3; ++pass) {
            bool thrown = false;
            try {
                if (pass == 0) { angle_stub_fail(SSW_ERR_OUT_OF_MEMORY); wm::find_angle(ctx, orig, suspects, -1.0, 1.0, &rungs); }
                if (pass == 1) wm::find_angle(ctx, orig, suspects, 2.0, 1.0);                    // the library's own refusal
                if (pass == 2) { wm::ImageRgb8 odd(w + 1, h); wm::find_angle(ctx, orig, {&a, &odd}); }      // a suspect of another size
            } catch (const wm::Error& e) {
                thrown = true;
                CHECK(e.status() == (pass == 0 ? SSW_ERR_OUT_OF_MEMORY : pass == 1 ? SSW_ERR_BAD_ARG : SSW_ERR_BAD_DIMS), "the status that was thrown");
            }
            CHECK(thrown && nothing_but_the_context(), "a thrown status leaves nothing alive");
        }
        wm::ImageRgb8 tiny(31, 40), tiny2(31, 40);
        bool thrown = false;
        try { wm::find_angle(ctx, tiny, {&tiny2}); } catch (const wm::Error& e) { thrown = e.status() == SSW_ERR_BAD_DIMS; }
        CHECK(thrown && nothing_but_the_context(), "a side of 31");
    }
    size_t live[5];
    ssw_stub_live(live);
    CHECK(live[2] == 0, "the context is gone");
    std::printf("angle wrappers: ok\n");
    return 0;
}
