// wm::locate_free of include/ssw_locate_free.hpp over the stubs (locate_free_stub.cpp for the new C function, ssw_stub.cpp for
// the rest): argument order, RGB and RGBA suspects of their own sizes, ranges and slacks that go with their suspects, the
// answers, and a thrown status with nothing left alive.  tests/test_locate_free_cpp_cpu.py builds and runs it, plain and under
// ASan/UBSan.
#include <cstdio>
#include <vector>

#include "ssw_locate_free.hpp"

extern "C" {
double locate_free_stub_last(size_t k);
void locate_free_stub_fail(int status);
uint64_t locate_free_stub_checksum(void);
void ssw_stub_live(size_t out[5]);
}

#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

static bool nothing_but_the_context() {
    size_t live[5];
    ssw_stub_live(live);
    return live[0] == 0 && live[1] == 0 && live[2] == 1 && live[3] == 0 && live[4] == 0;
}

int main() {
    const size_t w = 67, h = 45;
    {
        wm::Context ctx(0);
        wm::ImageRgb8 orig(w, h), a(21, 17), c(40, 40);
        wm::ImageRgba8 b(33, 9);
        for (size_t i = 0; i < orig.data.size(); ++i) orig.data[i] = (uint8_t)(i * 7 + 3);
        for (size_t i = 0; i < a.data.size(); ++i) a.data[i] = (uint8_t)(i + 10);
        for (size_t i = 0; i < b.data.size(); ++i) b.data[i] = (uint8_t)(i * 3 + 150);
        for (size_t i = 0; i < c.data.size(); ++i) c.data[i] = (uint8_t)(i * 5 + 1);
        const std::vector<wm::Suspect> suspects{wm::Suspect(a), wm::Suspect(b), wm::Suspect(c)};
        const std::vector<wm::ScaleRange> ranges{{32, 60}, {40, 67}, {33, 33}};
        const std::vector<uint32_t> slack{1, 4, 2};
        const size_t sw[3] = {21, 33, 40};

        const std::vector<wm::Located> r = wm::locate_free(ctx, orig, suspects, ranges, slack);
        CHECK(locate_free_stub_last(0) == 3 && locate_free_stub_last(1) == (double)w && locate_free_stub_last(2) == (double)h, "n, w, h");
        CHECK(locate_free_stub_last(3) == 40 && locate_free_stub_last(4) == 40 && locate_free_stub_last(5) == 3, "the last suspect's shape");
        CHECK(locate_free_stub_last(6) == 33 && locate_free_stub_last(7) == 33 && locate_free_stub_last(8) == 2, "the last range and slack");
        CHECK(r.size() == 3, "one answer per suspect");
        for (size_t i = 0; i < 3; ++i) {
            CHECK(r[i].placement.w == ranges[i].wmax && r[i].placement.h == ranges[i].wmin + slack[i], "pw, ph in their places: ranges and slacks go with their suspects");
            CHECK(r[i].placement.x == i + 1 && r[i].placement.y == 2 * i + slack[i], "x, y in their places");
            CHECK(r[i].sad == 1000 * i + sw[i] && r[i].mean_abs_diff == (double)r[i].sad / ((double)r[i].placement.w * (double)r[i].placement.h), "sad and its mean");
        }
        CHECK(nothing_but_the_context(), "its device blocks are freed");

        const uint64_t before = locate_free_stub_checksum();
        const std::vector<wm::Located> one = wm::locate_free(ctx, orig, {wm::Suspect(b)}, {{40, 67}}, {3});
        CHECK(one.size() == 1 && locate_free_stub_last(0) == 1 && locate_free_stub_last(5) == 4 && locate_free_stub_last(8) == 3, "one RGBA suspect");
        CHECK(locate_free_stub_checksum() != before, "its bytes were read");
        CHECK(wm::locate_free(ctx, orig, {}, {}, {}).empty() && locate_free_stub_last(0) == 1, "no suspects, no call");
        CHECK(nothing_but_the_context(), "its device blocks are freed");

        // a thrown status, nothing left alive
        for (int pass = 0; pass < 7; ++pass) {
            bool thrown = false;
            try {
                if (pass == 0) { locate_free_stub_fail(SSW_ERR_OUT_OF_MEMORY); wm::locate_free(ctx, orig, suspects, ranges, slack); }
                if (pass == 1) { locate_free_stub_fail(SSW_ERR_UNSUPPORTED); wm::locate_free(ctx, orig, suspects, ranges, slack); }
                if (pass == 2) wm::locate_free(ctx, orig, suspects, ranges, {1, 5, 2});                               // a slack above 4
                if (pass == 3) wm::locate_free(ctx, orig, suspects, ranges, {1, 0, 2});                               // no slack
                if (pass == 4) wm::locate_free(ctx, orig, suspects, {{32, 60}, {67, 40}, {33, 33}}, slack);           // wmin > wmax
                if (pass == 5) wm::locate_free(ctx, orig, suspects, ranges, {1, 2});                                  // two slacks for three suspects
                if (pass == 6) wm::locate_free(ctx, orig, suspects, {{32, 60}, {40, 67}}, slack);                     // two ranges for three suspects
            } catch (const wm::Error& e) {
                thrown = true;
                CHECK(e.status() == (pass == 0 ? SSW_ERR_OUT_OF_MEMORY : pass == 1 ? SSW_ERR_UNSUPPORTED : pass >= 5 ? SSW_ERR_BAD_DIMS : SSW_ERR_BAD_ARG),
                      "the status that was thrown");
            }
            CHECK(thrown && nothing_but_the_context(), "a thrown status leaves nothing alive");
        }
    }
    size_t live[5];
    ssw_stub_live(live);
    CHECK(live[2] == 0, "the context is gone");
    std::printf("locate_free wrappers: ok\n");
    return 0;
}
