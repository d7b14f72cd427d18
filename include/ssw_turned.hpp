// wm::locate_turned and wm::restore_turned -- the C++ face of ssw_locate_turned_rgb8 and ssw_restore_turned_rgb8 (include/ssw.h
// states the definitions): where does a cut-out of a turned copy lie, by which angle was it turned, and the frame a tracer makes
// of it.  A header of its own beside ssw.hpp, which it includes.
#ifndef SSW_TURNED_HPP
#define SSW_TURNED_HPP

#include <memory>
#include <vector>

#include "ssw.hpp"

namespace wm {

// One answer: the angle in degrees (n / 32; counter-clockwise, as PIL.Image.rotate's), the suspect's centre in pixels of the
// original, the size of the turned-back part of the suspect that was compared, the sum of absolute luma differences there and
// their mean -- a few units for a true match
struct LocatedTurned {
    double angle = 0.0;
    int32_t n = 0;
    double cx = 0.0, cy = 0.0;
    uint32_t tw = 0, th = 0;
    uint64_t sad = 0;
    double mean = 0.0;
};

namespace detail {
// suspects of any sizes on the device, one block each, and what the two calls take of them
struct TurnedSuspects {
    std::vector<std::unique_ptr<DeviceFrames>> dev;
    std::vector<const void*> ptrs;
    std::vector<ssw_turned_shape> shapes;
    TurnedSuspects(Context& ctx, const std::vector<const ImageRgb8*>& suspects, const char* where) {
        for (const ImageRgb8* s : suspects) {
            dev.emplace_back(new DeviceFrames(ctx.get(), s->width * s->height * 3, where));
            dev.back()->put({s}, s->width, s->height, where);
            ptrs.push_back(dev.back()->p);
            shapes.push_back(ssw_turned_shape{(uint32_t)s->width, (uint32_t)s->height, 3u});
        }
    }
};
}  // namespace detail

// ssw_locate_turned_rgb8 on host images: one LocatedTurned per suspect (RGB, any sizes), searched in amin .. amax degrees (within
// +-45).  rungs (optional): the ladder's entries, [suspect][rung][4] = D, n_j, x, y, one suspect after the other.
inline std::vector<LocatedTurned> locate_turned(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& suspects, double amin = -10.0,
                                                double amax = 10.0, std::vector<uint64_t>* rungs = nullptr) {
    std::vector<LocatedTurned> out(suspects.size());
    if (rungs) rungs->clear();
    if (suspects.empty()) return out;
    const size_t n = suspects.size(), w = original.width, h = original.height;
    detail::DeviceFrames base(ctx.get(), w * h * 3, "locate_turned");
    base.put({&original}, w, h, "locate_turned");
    detail::TurnedSuspects sus(ctx, suspects, "locate_turned");
    std::vector<ssw_turned_found> got(n);
    // the rungs of any range: at most 361 (a step of 0.25 degrees over +-45); sized after the call says how many there were
    std::vector<uint64_t> entries(rungs ? n * 361 * 4 : 0);
    check(ssw_locate_turned_rgb8(ctx.get(), base.p, w, h, sus.ptrs.data(), sus.shapes.data(), n, amin, amax, got.data(), rungs ? entries.data() : nullptr),
          "locate_turned");
    for (size_t i = 0; i < n; ++i) {
        const ssw_turned_found& f = got[i];
        out[i] = LocatedTurned{(double)f.n / 32.0, f.n, (double)f.x + (double)f.tw / 2.0, (double)f.y + (double)f.th / 2.0, f.tw, f.th, f.sad,
                               (double)f.sad / ((double)f.tw * (double)f.th)};
    }
    if (rungs) rungs->assign(entries.begin(), entries.begin() + n * got[0].n_rungs * 4);
    return out;
}

// ssw_restore_turned_rgb8 on host images: suspect i, turned by jobs[i].angle degrees with its centre at (jobs[i].cx, jobs[i].cy)
// pixels of the original, laid back into the original's frame; one frame of the original's size per suspect
inline std::vector<ImageRgb8> restore_turned(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& suspects,
                                             const std::vector<ssw_turned_job>& jobs) {
    if (jobs.size() != suspects.size()) throw Error(SSW_ERR_LENGTH_MISMATCH, "restore_turned");
    std::vector<ImageRgb8> out;
    if (suspects.empty()) return out;
    const size_t n = suspects.size(), w = original.width, h = original.height, fb = w * h * 3;
    detail::DeviceFrames base(ctx.get(), fb, "restore_turned"), res(ctx.get(), n * fb, "restore_turned");
    base.put({&original}, w, h, "restore_turned");
    detail::TurnedSuspects sus(ctx, suspects, "restore_turned");
    check(ssw_restore_turned_rgb8(ctx.get(), base.p, w, h, sus.ptrs.data(), sus.shapes.data(), jobs.data(), n, res.p), "restore_turned");
    for (size_t i = 0; i < n; ++i) {
        out.emplace_back(w, h);
        check(ssw_copy_to_host(ctx.get(), out.back().data.data(), res.p + i * fb, fb), "restore_turned");
    }
    return out;
}

// ... with the answers of locate_turned
inline std::vector<ImageRgb8> restore_turned(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& suspects,
                                             const std::vector<LocatedTurned>& found) {
    std::vector<ssw_turned_job> jobs;
    for (const LocatedTurned& f : found) jobs.push_back(ssw_turned_job{f.angle, f.cx, f.cy});
    return restore_turned(ctx, original, suspects, jobs);
}

}  // namespace wm

#endif  // SSW_TURNED_HPP
