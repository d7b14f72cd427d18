// wm::locate_free -- the C++ face of ssw_locate_free_rgb8 (include/ssw.h states the definition): the scale ladder of
// wm::locate_scaled, then the sizes within `slack` pixels of its answer rescored at full resolution in both dimensions, for
// cut-outs whose sides were rounded on their own when they were scaled.  A header of its own beside ssw.hpp, as ssw_crop.hpp
// and ssw_turned.hpp are.
#ifndef SSW_LOCATE_FREE_HPP
#define SSW_LOCATE_FREE_HPP

#include <vector>

#include "ssw.hpp"

namespace wm {

// ssw_locate_free_rgb8 on host images: ranges[i] and slack[i] (1 .. 4) go with suspects[i]; Located::placement carries the size
// that was found.
inline std::vector<Located> locate_free(Context& ctx, const ImageRgb8& original, const std::vector<Suspect>& suspects,
                                        const std::vector<ScaleRange>& ranges, const std::vector<uint32_t>& slack) {
    const size_t n = suspects.size();
    if (ranges.size() != n || slack.size() != n || original.data.size() != original.width * original.height * 3) throw Error(SSW_ERR_BAD_DIMS, "locate_free");
    if (n == 0) return {};
    std::vector<void*> dev(n + 1, nullptr);
    struct Free {
        ssw_ctx* c; std::vector<void*>& d;
        ~Free() { for (void* p : d) if (p) ssw_dev_free(c, p); }
    } guard{ctx.get(), dev};
    auto put = [&](const void* src, size_t bytes, void** out) {
        check(ssw_dev_alloc(ctx.get(), bytes, out), "locate_free");
        check(ssw_copy_to_dev(ctx.get(), *out, src, bytes), "locate_free");
    };
    put(original.data.data(), original.data.size(), &dev[n]);
    std::vector<ssw_placement> pl(n);
    std::vector<ssw_scale_range> rg(n);
    for (size_t i = 0; i < n; ++i) {
        if (ranges[i].wmin > 0xFFFFFFFFull || ranges[i].wmax > 0xFFFFFFFFull) throw Error(SSW_ERR_BAD_DIMS, "locate_free");
        put(suspects[i].data, suspects[i].width * suspects[i].height * suspects[i].channels, &dev[i]);
        pl[i] = ssw_placement{(uint32_t)suspects[i].width, (uint32_t)suspects[i].height, (uint32_t)suspects[i].channels, 0u, 0u, 0u, 0u};
        rg[i] = ssw_scale_range{(uint32_t)ranges[i].wmin, (uint32_t)ranges[i].wmax};
    }
    std::vector<uint64_t> sad(n);
    check(ssw_locate_free_rgb8(ctx.get(), static_cast<const uint8_t*>(dev[n]), original.width, original.height, dev.data(), pl.data(), rg.data(),
                               slack.data(), n, sad.data()), "locate_free");
    std::vector<Located> out(n);
    for (size_t i = 0; i < n; ++i) {
        const double px = (double)pl[i].pw * (double)pl[i].ph;
        out[i] = Located{Placement{pl[i].x, pl[i].y, pl[i].pw, pl[i].ph}, sad[i], px > 0 ? (double)sad[i] / px : 0.0};
    }
    return out;
}

}  // namespace wm

#endif  // SSW_LOCATE_FREE_HPP
