// Host-side check of the context's workspace enumeration (csrc/ssw_internal.hpp: for_each_buf, lane_bytes_held): every Buf
// is visited exactly once under a name of its own, none is left out, and the ones counted towards the automatic pass size
// are the lanes' f32 planes, operand slots, compact planes, index lists, gathered bases and prune tables -- nothing else.
// No GPU: a default-constructed context, no HIP call.
#include <cstdio>
#include <set>
#include <string>
#include <vector>
#include "../../spread_spectrum_watermarking_amd/csrc/ssw_internal.hpp"

using namespace ssw;

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s (line %d)\n", what, #cond, __LINE__); ++failures; } } while (0)

struct Entry { int lane; std::string group, name; Buf* buf; bool counted; };

int main() {
    ssw_ctx* ctx = new ssw_ctx();
    std::vector<Entry> all;
    for_each_buf(*ctx, [&](int lane, const char* group, const char* name, Buf& b, bool counted) { all.push_back({lane, group, name, &b, counted}); });

    // once each: distinct addresses inside the context, distinct names
    std::set<const Buf*> addrs;
    std::set<std::string> names;
    for (const Entry& e : all) {
        addrs.insert(e.buf);
        names.insert(std::to_string(e.lane) + "/" + e.group + "/" + e.name);
        const char *lo = reinterpret_cast<const char*>(ctx), *p = reinterpret_cast<const char*>(e.buf);
        CHECK(p >= lo && p + sizeof(Buf) <= lo + sizeof(ssw_ctx), "a buffer of this context");
        CHECK(e.buf->p == nullptr && e.buf->bytes == 0, "empty at first");
    }
    CHECK(addrs.size() == all.size(), "distinct addresses");
    CHECK(names.size() == all.size(), "distinct names");

    // every Buf there is: the groups are nothing but Bufs (static_assert in the header), so their sizes count them; a lane
    // adds its index list and base_prune, the streaming ring 3 x NB + 3, the frame stages one each
    const size_t lane_bufs = (sizeof(LanePlanes) + sizeof(LaneOperands) + sizeof(LaneCompact) + sizeof(PruneBufs)) / sizeof(Buf) + 2;
    CHECK(sizeof(ssw_ctx::Lane) == lane_bufs * sizeof(Buf) + sizeof(SelectWorkspace) + sizeof(hipStream_t) + sizeof(hipEvent_t), "a lane: its Bufs, the selection, a stream, an event");
    const size_t own_bufs = (sizeof(ssw_ctx::Trace) + sizeof(LocateBufs) + sizeof(CatalogueBufs) + sizeof(FingerprintBufs) + sizeof(SharedBufs)) / sizeof(Buf);
    CHECK(sizeof(ssw_ctx::Trace) == sizeof(TraceBufs) + sizeof(PruneBufs), "the trace's buffers and its prune tables");
    const size_t ring_bufs = 3 * ssw_ctx::HostStream::NB + 3, stage_bufs = sizeof(ctx->frame_stage) / sizeof(ctx->frame_stage[0]);
    CHECK(all.size() == ssw_ctx::MAX_LANES * lane_bufs + own_bufs + ring_bufs + stage_bufs, "every Buf is visited");
    CHECK(LanePlanes::count == 4 && LaneOperands::count == 6 && LaneCompact::count == 2 && PruneBufs::count == 3, "the lane's groups");

    // counted: exactly the lanes' six kinds
    std::set<const Buf*> expect;
    for (auto& ln : ctx->lane) {
        for (Buf* b : {&ln.plane.y, &ln.plane.i_derived, &ln.plane.q_scratch, &ln.plane.scratch}) expect.insert(b);
        for (Buf* b : {&ln.operand.s_cop, &ln.operand.odd_t2, &ln.operand.ss_a1, &ln.operand.sd, &ln.operand.even, &ln.operand.deep}) expect.insert(b);
        for (Buf* b : {&ln.compact.rows, &ln.compact.cols, &ln.idx, &ln.prune.gathered, &ln.prune.gathered_frag, &ln.prune.u32}) expect.insert(b);
    }
    std::set<const Buf*> counted;
    for (const Entry& e : all) if (e.counted) counted.insert(e.buf);
    CHECK(counted == expect, "counted: planes, operand slots, compact planes, index list, gathered bases, prune tables");
    CHECK(expect.size() == ssw_ctx::MAX_LANES * (lane_bufs - 1), "all of a lane but base_prune");

    // ... and those, and only those, move the total that effective_chunk adds to the free memory
    CHECK(lane_bytes_held(ctx) == 0, "nothing held at first");
    size_t want = 0, step = 4096;
    for (const Entry& e : all) {
        const size_t before = lane_bytes_held(ctx);
        e.buf->bytes = step;
        CHECK(lane_bytes_held(ctx) == before + (e.counted ? step : 0), "a buffer's bytes move the total iff it is counted");
        if (e.counted) want += step;
        step += 4096;          // (every buffer its own size: a buffer counted twice or mistaken for another shows)
    }
    CHECK(lane_bytes_held(ctx) == want, "the total");
    for (const Entry& e : all) e.buf->bytes = 0;
    // the selection workspaces and the handles' plane pool are no part of it either
    ctx->lane[0].sel.frames = 7; ctx->lane[0].sel.cap = 1 << 20; ctx->plane_pool_bytes = 1 << 24;
    CHECK(lane_bytes_held(ctx) == 0, "selection workspaces and the plane pool are not counted");

    delete ctx;
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
