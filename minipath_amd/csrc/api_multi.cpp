// C ABI (include/minipath_hip.h): mp_render_frame_multi / mp_render_pass_multi -- one pass (or whole frame) over n ranks, each
// rendering its shard of the tiles on its own device and stream, and optionally the gather + un-tile on ctxs[0]'s device
// (SURVEY 8e).  The buffers live in each context's mp_ctx::MultiBuf.
#include "api_common.h"

using namespace mp;

namespace {

// What one call works on: the arguments, the pass and the partition of the frame's tiles over the ranks.
struct Frame {
    mp_ctx* const* ctxs;
    const mp_scene* const* scenes;
    int n;
    const mp_camera_sampler* sampler;
    const mp_settings* st;
    bool gather, acc, final_pass;
    uint32_t p_begin, p_end;
    size_t per_rank, tile_bytes;
    // rank-major slots of the gather buffer: slot r*per_rank + k = k-th tile of rank r (tiles r, r+n, r+2n, ... of the grid; the
    // last slots of a rank may be empty blocks), and the same tiles per rank
    std::vector<mp_block> order;
    std::vector<std::vector<mp_block>> shard;
    std::vector<char> staged;  // how each rank's shard reaches device 0, decided once for both legs of the copy
    size_t shard_bytes() const { return per_rank * tile_bytes; }
    mp_ctx::PassState state(int r) const {
        return {st->seed, st->width, st->height, st->tile_size, st->sample_count, st->flags, st->max_depth, static_cast<uint32_t>(n),
                static_cast<uint32_t>(r), scenes[r]};
    }
};

void partition(Frame& f) {
    const mp_settings& st = *f.st;
    f.acc = (st.flags & MP_FLAG_ACCUMULATE) != 0;
    f.p_begin = f.acc ? st.pass_begin : 0u;
    f.p_end = f.p_begin + pass_samples(st);
    f.final_pass = f.p_end == st.sample_count;
    const size_t n = static_cast<size_t>(f.n);
    const std::vector<mp_block> all = tile_ordering(mp_block{0, 0, st.width, st.height}, st.tile_size, 0);
    f.per_rank = (all.size() + n - 1) / n;
    f.tile_bytes = static_cast<size_t>(st.tile_size) * st.tile_size * 16;
    f.order.assign(f.per_rank * n, mp_block{0, 0, 0, 0});
    f.shard.resize(n);
    f.staged.assign(n, 0);
    for (size_t t = 0; t < all.size(); t++) {
        f.order[(t % n) * f.per_rank + t / n] = all[t];
        f.shard[t % n].push_back(all[t]);
    }
}

// direct peer copies where the two devices can reach each other (xGMI), in both directions: the copy runs on the source device's
// stream and writes device 0's memory
bool enable_peers(int dev0, int d) {
    int can01 = 0, can10 = 0;
    if (hipDeviceCanAccessPeer(&can01, dev0, d) != hipSuccess || hipDeviceCanAccessPeer(&can10, d, dev0) != hipSuccess || !can01 || !can10) return false;
    hipError_t e1 = hipDeviceEnablePeerAccess(d, 0), e2;
    {
        DeviceGuard gd(d);
        e2 = hipDeviceEnablePeerAccess(dev0, 0);
    }
    const bool ok = (e1 == hipSuccess || e1 == hipErrorPeerAccessAlreadyEnabled) && (e2 == hipSuccess || e2 == hipErrorPeerAccessAlreadyEnabled);
    if (e1 != hipSuccess || e2 != hipSuccess) (void)hipGetLastError();
    return ok;
}

// The gathering context's buffer, event and peer table (asked once per device); then how every rank's shard travels.
int ensure_gather(Frame& f) {
    mp_ctx* c0 = f.ctxs[0];
    mp_ctx::MultiBuf& m0 = c0->multi;
    DeviceGuard g(c0->device);
    if (m0.gather.bytes() < f.order.size() * f.tile_bytes) {
        if (m0.untiled_valid) (void)hipEventSynchronize(m0.untiled.get());  // the last un-tile still reads the old buffer
        MP_HIP(m0.gather.grow(f.order.size() * f.tile_bytes));
    }
    MP_HIP(m0.untiled.ensure());
    int ndev = 0;
    MP_HIP(hipGetDeviceCount(&ndev));
    if (m0.peer.size() < static_cast<size_t>(ndev)) m0.peer.resize(static_cast<size_t>(ndev), 0);
    const bool force = c0->multi_gather_staged.load() != 0u;
    for (int r = 1; r < f.n; r++) {
        const int d = f.ctxs[r]->device;
        if (d != c0->device && d >= 0 && d < ndev && m0.peer[static_cast<size_t>(d)] == 0)
            m0.peer[static_cast<size_t>(d)] = enable_peers(c0->device, d) ? 1 : 2;  // staged through pinned host memory otherwise
        f.staged[static_cast<size_t>(r)] = force || (d != c0->device && m0.peer[static_cast<size_t>(d)] == 2);
    }
    return MP_OK;
}

// A pass is all or nothing: every rank is checked before anything is launched, so a refusal leaves every shard as it was.
int check_ranks(const Frame& f) {
    for (int r = 0; r < f.n; r++) {
        if (f.shard[static_cast<size_t>(r)].empty()) continue;
        if (int rc = render_refusal(f.scenes[r], *f.st)) return rc;
        if (!f.acc || f.p_begin == 0) continue;
        // the running state in the shard must be this render's, at this sample (a shard that is too small has none)
        const mp_ctx::MultiBuf& m = f.ctxs[r]->multi;
        if (!(m.acc == f.state(r) && m.acc_next == f.p_begin && m.shard.bytes() >= f.shard_bytes()))
            return fail(MP_ERR_INVALID, "progressive pass does not continue the state this rank's shard holds (pass_begin must be the previous pass's end, same settings, same ranks)");
    }
    return MP_OK;
}

// One rank renders its shard in one launch on its own stream (machinery.rs:51-116: the workers own their tiles) and, when the
// frame is gathered, sends it to device 0 on that same stream: n copies on n streams, each peer over its own link.
int launch_rank(const Frame& f, int r) {
    mp_ctx *c = f.ctxs[r], *c0 = f.ctxs[0];
    const std::vector<mp_block>& tiles = f.shard[static_cast<size_t>(r)];
    DeviceGuard g(c->device);
    LaunchScope record(c);
    mp_ctx::MultiBuf& m = c->multi;
    MP_HIP(m.stream.ensure());
    MP_HIP(m.copied.ensure());
    if (m.shard.bytes() < f.shard_bytes()) {
        MP_HIP(hipStreamSynchronize(m.stream.get()));  // its render and its copy (issued in order on this stream) are done with the old buffer
        MP_HIP(m.shard.grow(f.shard_bytes()));
    }
    const mp_block* d_tiles = nullptr;
    mp_ctx::TileListRef keep;
    if (int rc = c->device_tiles(tiles.data(), tiles.size(), nullptr, keep, &d_tiles, nullptr)) return rc;
    if (int rc = render_tiles_device(c, f.scenes[r], *f.sampler, *f.st, d_tiles, tiles.size(), m.shard.as<float>(), m.stream.get())) return rc;
    if (!f.gather) return MP_OK;
    // the previous frame's un-tile must have read the gather buffer before this frame's copy overwrites its slot
    if (c0->multi.untiled_valid) MP_HIP(hipStreamWaitEvent(m.stream.get(), c0->multi.untiled.get(), 0));
    const size_t bytes = tiles.size() * f.tile_bytes;
    if (!f.staged[static_cast<size_t>(r)]) {
        void* dst = c0->multi.gather.as<unsigned char>() + static_cast<size_t>(r) * f.shard_bytes();
        MP_HIP(hipMemcpyPeerAsync(dst, c0->device, m.shard.get(), c->device, bytes, m.stream.get()));
    } else {
        if (m.stage.bytes() < f.shard_bytes()) {
            // the last frame's legs through the old buffer (this stream's, then device 0's before its un-tile) are done with it
            MP_HIP(hipStreamSynchronize(m.stream.get()));
            if (c0->multi.untiled_valid) MP_HIP(hipEventSynchronize(c0->multi.untiled.get()));
            MP_HIP(m.stage.grow(f.shard_bytes()));
        }
        MP_HIP(hipMemcpyAsync(m.stage.get(), m.shard.get(), bytes, hipMemcpyDeviceToHost, m.stream.get()));
    }
    MP_HIP(hipEventRecord(m.copied.get(), m.stream.get()));
    return MP_OK;
}

// The shards' state is committed only once every rank's pass is enqueued; after a failed launch no shard's state is known.
void commit_state(const Frame& f, bool launched) {
    for (int r = 0; r < f.n; r++) {
        if (f.shard[static_cast<size_t>(r)].empty()) continue;
        mp_ctx::MultiBuf& m = f.ctxs[r]->multi;
        m.acc_next = (launched && f.acc && !f.final_pass) ? f.p_end : 0u;
        if (launched && f.acc) m.acc = f.state(r);
    }
}

// On device 0, on the caller's stream: wait for every rank's copy, run the second leg of the staged ones, un-tile.
int gather_untile(const Frame& f, float* d_image_f32, uint8_t* d_image_u8, hipStream_t st0) {
    mp_ctx* c0 = f.ctxs[0];
    mp_ctx::MultiBuf& m0 = c0->multi;
    DeviceGuard g0(c0->device);
    uint32_t staged_ranks = 0;
    for (int r = 0; r < f.n; r++) {
        const size_t nt = f.shard[static_cast<size_t>(r)].size();
        if (nt == 0) continue;
        MP_HIP(hipStreamWaitEvent(st0, f.ctxs[r]->multi.copied.get(), 0));
        if (!f.staged[static_cast<size_t>(r)]) continue;
        MP_HIP(hipMemcpyAsync(m0.gather.as<unsigned char>() + static_cast<size_t>(r) * f.shard_bytes(), f.ctxs[r]->multi.stage.get(),
                              nt * f.tile_bytes, hipMemcpyHostToDevice, st0));
        staged_ranks++;
    }
    m0.staged_ranks = staged_ranks;
    const mp_block* d_order = nullptr;
    mp_ctx::TileListRef keep0;
    if (int rc = c0->device_tiles(f.order.data(), f.order.size(), nullptr, keep0, &d_order, nullptr)) return rc;
    LaunchScope record(c0);
    std::string err;
    // a gather before the last pass shows a preview: the running sums scaled by the samples drawn so far (the shards keep their state)
    const uint32_t mode = (f.acc && !f.final_pass) ? ((f.st->flags & MP_FLAG_CHUNKED_SUM) ? 2u : 1u) : 0u;
    int rc = launch_untile(f.st->width, f.st->height, f.st->tile_size, d_order, static_cast<uint32_t>(f.order.size()), m0.gather.as<float>(),
                           d_image_f32, d_image_u8, st0, err, mode, f.p_end);
    if (rc) return fail(rc, err);
    MP_HIP(hipEventRecord(m0.untiled.get(), st0));
    m0.untiled_valid = true;
    return MP_OK;
}

int render_multi(mp_ctx* const* ctxs, const mp_scene* const* scenes, int n, const mp_camera_sampler* sampler,
                 const mp_settings* settings, bool gather, float* d_image_f32, uint8_t* d_image_u8, uint64_t* ray_segments, void* stream) {
    if (!ctxs || !scenes || n < 1 || n > 64 || !sampler || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (settings->flags & MP_FLAG_WAVEFRONT) return fail(MP_ERR_INVALID, "the multi-device frame uses the fused kernels");
    for (int i = 0; i < n; i++) {
        if (!ctxs[i] || !scenes[i] || scenes[i]->ctx != ctxs[i]) return fail(MP_ERR_INVALID, "scenes[i] must live on ctxs[i]");
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return fail(MP_ERR_INVALID, "every rank needs its own context (two contexts may share a device)");
    }
    Frame f{ctxs, scenes, n, sampler, settings, gather};
    partition(f);
    // A context takes part in one multi-device frame at a time: the locks of all ranks are taken once, in address order (two
    // calls over the same contexts in another rank order cannot deadlock), and held for the call.
    std::vector<mp_ctx*> by_address(ctxs, ctxs + n);
    std::sort(by_address.begin(), by_address.end(), std::less<mp_ctx*>());
    std::vector<std::unique_lock<std::mutex>> locks;
    for (mp_ctx* c : by_address) locks.emplace_back(c->multi_mu);
    if (int rc = gather ? ensure_gather(f) : MP_OK) return rc;
    if (int rc = check_ranks(f)) return rc;
    int launched = MP_OK;
    for (int r = 0; r < n && launched == MP_OK; r++)
        if (!f.shard[static_cast<size_t>(r)].empty()) launched = launch_rank(f, r);
    commit_state(f, launched == MP_OK);
    if (launched != MP_OK) return launched;
    // reference semantics only (0 with MP_FLAG_PATHS: use mp_render_tiles_device_counted); the ranks' tiles cover the frame
    if (ray_segments) *ray_segments = (settings->flags & MP_FLAG_PATHS) ? 0 : reference_segments(static_cast<uint64_t>(settings->width) * settings->height, *settings);
    return gather ? gather_untile(f, d_image_f32, d_image_u8, static_cast<hipStream_t>(stream)) : MP_OK;
}

}  // namespace

extern "C" {

int mp_render_frame_multi(mp_ctx* const* ctxs, const mp_scene* const* scenes, int n, const mp_camera_sampler* sampler,
                          const mp_settings* settings, float* d_image_f32, uint8_t* d_image_u8, uint64_t* ray_segments,
                          void* stream) {
    return guarded([&]() -> int {
    if (settings && (settings->flags & MP_FLAG_ACCUMULATE)) return fail(MP_ERR_INVALID, "mp_render_frame_multi renders whole frames: progressive passes go through mp_render_pass_multi");
    return render_multi(ctxs, scenes, n, sampler, settings, true, d_image_f32, d_image_u8, ray_segments, stream);
    });
}

int mp_render_pass_multi(mp_ctx* const* ctxs, const mp_scene* const* scenes, int n, const mp_camera_sampler* sampler,
                         const mp_settings* settings, int gather, float* d_image_f32, uint8_t* d_image_u8, uint64_t* ray_segments,
                         void* stream) {
    return guarded([&]() -> int {
    if (settings && !(settings->flags & MP_FLAG_ACCUMULATE)) return fail(MP_ERR_INVALID, "mp_render_pass_multi takes MP_FLAG_ACCUMULATE settings (pass_begin / pass_count)");
    return render_multi(ctxs, scenes, n, sampler, settings, gather != 0, d_image_f32, d_image_u8, ray_segments, stream);
    });
}

}  // extern "C"
