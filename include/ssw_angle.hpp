// wm::find_angle -- the C++ face of ssw_find_angle_rgb8 (include/ssw.h states the definition): by which angle was each suspect
// turned?  A header of its own beside ssw.hpp, which it includes.
#ifndef SSW_ANGLE_HPP
#define SSW_ANGLE_HPP

#include <vector>

#include "ssw.hpp"

namespace wm {

// One answer: the angle in degrees (n / 32; counter-clockwise, as PIL.Image.rotate's), the sum of absolute luma differences
// between the original turned by it and the suspect over `count` pixels, and their mean -- a few units for a true match
struct FoundAngle {
    double angle = 0.0;
    int32_t n = 0;
    uint64_t sad = 0, count = 0;
    double mean = 0.0;
};

// C(n), S(n) of the angle n / 32 degrees (ssw_angle_table): all the search uses of Pillow's matrix
inline std::pair<int32_t, int32_t> angle_table(int32_t n) {
    int32_t c = 0, s = 0;
    check(ssw_angle_table(n, &c, &s), "angle_table");
    return {c, s};
}

// ssw_find_angle_rgb8 on host images of the original's size: one FoundAngle per suspect, searched in amin .. amax degrees (within
// +-45).  rungs (optional): the ladder's sums, [suspect][rung][2] = D, c, one suspect after the other.
inline std::vector<FoundAngle> find_angle(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& suspects, double amin = -10.0,
                                          double amax = 10.0, std::vector<uint64_t>* rungs = nullptr) {
    std::vector<FoundAngle> out(suspects.size());
    if (rungs) rungs->clear();
    if (suspects.empty()) return out;
    const size_t n = suspects.size(), w = original.width, h = original.height, fb = w * h * 3;
    detail::DeviceFrames base(ctx.get(), fb, "find_angle"), dev(ctx.get(), n * fb, "find_angle");
    base.put({&original}, w, h, "find_angle");
    dev.put(suspects, w, h, "find_angle");
    std::vector<ssw_angle_found> got(n);
    // the rungs of any range: at most 361 (a step of 0.25 degrees over +-45); sized after the call says how many there were
    std::vector<uint64_t> sums(rungs ? n * 361 * 2 : 0);
    check(ssw_find_angle_rgb8(ctx.get(), base.p, dev.p, n, w, h, amin, amax, got.data(), rungs ? sums.data() : nullptr), "find_angle");
    for (size_t i = 0; i < n; ++i)
        out[i] = FoundAngle{(double)got[i].n / 32.0, got[i].n, got[i].sad, got[i].count, got[i].count ? (double)got[i].sad / (double)got[i].count : 0.0};
    if (rungs) rungs->assign(sums.begin(), sums.begin() + n * got[0].n_rungs * 2);
    return out;
}

}  // namespace wm

#endif  // SSW_ANGLE_HPP
