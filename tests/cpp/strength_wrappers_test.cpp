// Runs the five host-image wrappers of the strength report in include/ssw.hpp (wm::quality, ssim, collude, jpeg, filter) on
// frames read from files and writes what they return; tests/test_cpp_surface.py compares it with the Python wrappers' answers.
//   strength_wrappers_test <original.u8> <copy0.u8> <copy1.u8> <w> <h> <frames_out.u8>
// stdout: one line per Quality and per Ssim; frames_out: collude's 2 frames, jpeg's 4, filter's 6, in that order.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "ssw.hpp"

static wm::ImageRgb8 read_frame(const char* path, size_t w, size_t h) {
    wm::ImageRgb8 im(w, h);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(im.data.data()), (std::streamsize)im.data.size());
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return im;
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    try {
        const size_t w = std::strtoul(argv[4], nullptr, 10), h = std::strtoul(argv[5], nullptr, 10);
        const wm::ImageRgb8 original = read_frame(argv[1], w, h), c0 = read_frame(argv[2], w, h), c1 = read_frame(argv[3], w, h);
        const std::vector<const wm::ImageRgb8*> copies{&c0, &c1};
        wm::Context ctx(0);
        for (const wm::Quality& q : wm::quality(ctx, original, copies))
            std::cout << "quality " << q.sse[0] << " " << q.sse[1] << " " << q.sse[2] << " " << q.sse_luma << " " << q.changed << " " << q.max_abs
                      << " " << q.pixels << "\n";
        for (const wm::Ssim& s : wm::ssim(ctx, original, copies))
            std::cout << "ssim " << s.sum << " " << s.worst << " " << s.worst_x << " " << s.worst_y << " " << s.windows << "\n";
        std::vector<wm::ImageRgb8> frames = wm::collude(ctx, copies, {{SSW_COLLUDE_MEDIAN, {0, 1}}, {SSW_COLLUDE_MOSAIC, {1}}});
        for (wm::ImageRgb8& f : wm::jpeg(ctx, copies, {{0, 75}, {0, 10}, {1, 75}, {1, 10}})) frames.push_back(std::move(f));
        std::vector<wm::FilterJob> jobs;
        for (uint32_t i = 0; i < 2; ++i) {
            jobs.push_back(wm::FilterJob::blur(i, 1.5f));
            jobs.push_back(wm::FilterJob::median(i));
            jobs.push_back(wm::FilterJob::unsharp(i));
        }
        for (wm::ImageRgb8& f : wm::filter(ctx, copies, jobs)) frames.push_back(std::move(f));
        std::ofstream out(argv[6], std::ios::binary);
        for (const wm::ImageRgb8& f : frames) {
            if (f.width != w || f.height != h || f.data.size() != w * h * 3) return 3;
            out.write(reinterpret_cast<const char*>(f.data.data()), (std::streamsize)f.data.size());
        }
        if (!out) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
