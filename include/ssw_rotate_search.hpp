// wm::rotate_search_attack -- the C++ face of ssw_rotate_search_attack_rgb8 (include/ssw.h states the definition): every frame
// turned as Pillow's Image.rotate does it, its angle searched for as a tracer must who is not told it, and the frame turned back
// by the angle FOUND.  A header of its own beside ssw.hpp, as ssw_angle.hpp and ssw_turned.hpp are.
#ifndef SSW_ROTATE_SEARCH_HPP
#define SSW_ROTATE_SEARCH_HPP

#include <vector>

#include "ssw_angle.hpp"

namespace wm {

// What a call answers, one entry per job: the restored frames, the angles found, the share of the frame the undoing took from the
// turned copy; when asked for, the turned frames themselves and the ladder's sums [job][rung][2] = D, c
struct RotateSearched {
    std::vector<ImageRgb8> frames;
    std::vector<FoundAngle> found;
    std::vector<double> kept;
    std::vector<ImageRgb8> turned;
    std::vector<uint64_t> rungs;
};

// ssw_rotate_search_attack_rgb8 on host images of the original's size; jobs as for wm::rotate_attack (the angle, filter and fill
// of the turn); the angle is searched for in amin .. amax degrees (within +-45).
inline RotateSearched rotate_search_attack(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& frames,
                                           const std::vector<Rotate>& jobs, double amin = -10.0, double amax = 10.0, bool want_turned = false,
                                           bool want_rungs = false) {
    RotateSearched out;
    if (jobs.empty()) return out;
    if (frames.empty()) throw Error(SSW_ERR_BAD_ARG, "rotate_search_attack");
    const size_t n = frames.size(), m = jobs.size(), w = original.width, h = original.height, fb = w * h * 3;
    detail::DeviceFrames base(ctx.get(), fb, "rotate_search_attack"), dev(ctx.get(), n * fb, "rotate_search_attack"),
        made(ctx.get(), m * fb, "rotate_search_attack"), turned(ctx.get(), want_turned ? m * fb : 0, "rotate_search_attack");
    base.put({&original}, w, h, "rotate_search_attack");
    dev.put(frames, w, h, "rotate_search_attack");
    std::vector<ssw_rotate_job> jb(m);
    for (size_t i = 0; i < m; ++i) jb[i] = jobs[i].job(w, h);
    std::vector<ssw_angle_found> got(m);
    std::vector<uint64_t> kept(m), sums(want_rungs ? m * 361 * 2 : 0);          // at most 361 rungs: 0.25 degrees over +-45
    check(ssw_rotate_search_attack_rgb8(ctx.get(), base.p, dev.p, n, w, h, jb.data(), m, amin, amax, made.p, want_turned ? turned.p : nullptr,
                                        got.data(), want_rungs ? sums.data() : nullptr, kept.data()), "rotate_search_attack");
    out.frames.assign(m, ImageRgb8(w, h));
    for (size_t i = 0; i < m; ++i) check(ssw_copy_to_host(ctx.get(), out.frames[i].data.data(), made.p + i * fb, fb), "rotate_search_attack");
    if (want_turned) {
        out.turned.assign(m, ImageRgb8(w, h));
        for (size_t i = 0; i < m; ++i) check(ssw_copy_to_host(ctx.get(), out.turned[i].data.data(), turned.p + i * fb, fb), "rotate_search_attack");
    }
    out.found.resize(m);
    out.kept.resize(m);
    for (size_t i = 0; i < m; ++i) {
        out.found[i] = FoundAngle{(double)got[i].n / 32.0, got[i].n, got[i].sad, got[i].count, got[i].count ? (double)got[i].sad / (double)got[i].count : 0.0};
        out.kept[i] = (double)kept[i] / (double)(w * h);
    }
    if (want_rungs) out.rungs.assign(sums.begin(), sums.begin() + m * got[0].n_rungs * 2);
    return out;
}

}  // namespace wm

#endif  // SSW_ROTATE_SEARCH_HPP
