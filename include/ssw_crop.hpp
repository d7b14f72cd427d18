// wm::crop_attack and wm::crop_search_attack -- the C++ faces of ssw_crop_attack_rgb8 and ssw_crop_search_attack_rgb8
// (include/ssw.h states the definitions): a rectangle cut out of every frame, perhaps made a thumbnail as Pillow's Image.resize
// makes it, and laid over the original again -- where the caller says, or where the tracer's own search finds it.  A header of
// its own beside ssw.hpp, as ssw_turned.hpp and ssw_rotate_search.hpp are.
#ifndef SSW_CROP_HPP
#define SSW_CROP_HPP

#include <vector>

#include "ssw.hpp"

namespace wm {

// One job: the rectangle (x, y, cw, ch) of frame `frame`; tw = th = 0: the piece is not scaled, else it is made a tw x th
// thumbnail with `filter`
struct Crop {
    uint32_t frame = 0;
    size_t x = 0, y = 0, cw = 0, ch = 0, tw = 0, th = 0;
    ResampleFilter filter = ResampleFilter::Bicubic;
    ssw_crop_job job() const {
        return ssw_crop_job{frame, (uint32_t)x, (uint32_t)y, (uint32_t)cw, (uint32_t)ch, (uint32_t)tw, (uint32_t)th, tw ? (uint32_t)filter : 0u};
    }
    size_t thumb_width() const { return tw ? tw : cw; }
    size_t thumb_height() const { return tw ? th : ch; }
};
// The widths a searched piece may have had in the original; {0, 0}: its own size, only the position is searched
struct CropSearch { uint32_t wmin = 0, wmax = 0; };

// What a call answers, one entry per job: the restored frames; when asked for, the pieces as they would leak; for the searched
// form where each piece was found
struct Cropped {
    std::vector<ImageRgb8> frames;
    std::vector<ImageRgb8> thumbs;
    std::vector<Located> found;
};

namespace detail {
inline Cropped crop_run(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& frames, const std::vector<Crop>& jobs,
                        const std::vector<CropSearch>* searches, bool want_thumbs, const char* where) {
    Cropped out;
    if (jobs.empty()) return out;
    if (frames.empty() || (searches && searches->size() != jobs.size())) throw Error(SSW_ERR_BAD_ARG, where);
    const size_t n = frames.size(), m = jobs.size(), w = original.width, h = original.height, fb = w * h * 3;
    std::vector<ssw_crop_job> jb(m);
    std::vector<size_t> off(m + 1, 0);
    for (size_t i = 0; i < m; ++i) {
        if (jobs[i].x > 0xFFFFFFFFull || jobs[i].y > 0xFFFFFFFFull || jobs[i].cw > 0xFFFFFFFFull || jobs[i].ch > 0xFFFFFFFFull ||
            jobs[i].tw > 0xFFFFFFFFull || jobs[i].th > 0xFFFFFFFFull) throw Error(SSW_ERR_BAD_DIMS, where);
        jb[i] = jobs[i].job();
        off[i + 1] = off[i] + jobs[i].thumb_width() * jobs[i].thumb_height() * 3;
    }
    DeviceFrames base(ctx.get(), fb, where), dev(ctx.get(), n * fb, where), made(ctx.get(), m * fb, where),
        pieces(ctx.get(), want_thumbs ? off[m] : 0, where);
    base.put({&original}, w, h, where);
    dev.put(frames, w, h, where);
    if (searches) {
        std::vector<ssw_crop_search> sr(m);
        for (size_t i = 0; i < m; ++i) sr[i] = ssw_crop_search{(*searches)[i].wmin, (*searches)[i].wmax};
        std::vector<ssw_placement> got(m);
        std::vector<uint64_t> sad(m);
        check(ssw_crop_search_attack_rgb8(ctx.get(), base.p, dev.p, n, w, h, jb.data(), sr.data(), m, made.p, want_thumbs ? pieces.p : nullptr,
                                          got.data(), sad.data()), where);
        out.found.resize(m);
        for (size_t i = 0; i < m; ++i) {
            const double px = (double)got[i].pw * (double)got[i].ph;
            out.found[i] = Located{Placement{got[i].x, got[i].y, got[i].pw, got[i].ph}, sad[i], px > 0 ? (double)sad[i] / px : 0.0};
        }
    } else {
        check(ssw_crop_attack_rgb8(ctx.get(), base.p, dev.p, n, w, h, jb.data(), m, made.p, want_thumbs ? pieces.p : nullptr), where);
    }
    out.frames.assign(m, ImageRgb8(w, h));
    for (size_t i = 0; i < m; ++i) check(ssw_copy_to_host(ctx.get(), out.frames[i].data.data(), made.p + i * fb, fb), where);
    if (want_thumbs) {
        out.thumbs.reserve(m);
        for (size_t i = 0; i < m; ++i) {
            out.thumbs.emplace_back(jobs[i].thumb_width(), jobs[i].thumb_height());
            check(ssw_copy_to_host(ctx.get(), out.thumbs[i].data.data(), pieces.p + off[i], off[i + 1] - off[i]), where);
        }
    }
    return out;
}
}  // namespace detail

// ssw_crop_attack_rgb8 on host images of the original's size: the tracer is told every rectangle
inline Cropped crop_attack(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& frames, const std::vector<Crop>& jobs,
                           bool want_thumbs = false) {
    return detail::crop_run(ctx, original, frames, jobs, nullptr, want_thumbs, "crop_attack");
}

// ssw_crop_search_attack_rgb8: the tracer searches for every piece; searches[i] goes with jobs[i] (an empty `searches`: every
// piece at its own size)
inline Cropped crop_search_attack(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& frames, const std::vector<Crop>& jobs,
                                  const std::vector<CropSearch>& searches = {}, bool want_thumbs = false) {
    const std::vector<CropSearch> own(jobs.size());
    return detail::crop_run(ctx, original, frames, jobs, searches.empty() ? &own : &searches, want_thumbs, "crop_search_attack");
}

}  // namespace wm

#endif  // SSW_CROP_HPP
