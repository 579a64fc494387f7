// What the units behind the C ABI (api_*.cpp) share: the error helpers, the exception guard, the context and the scene.
// Internal to the host side of libminipath_hip.so.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "hip_owned.h"
#include "mp_internal.h"

namespace mp {

inline int fail(int code, const std::string& msg) {
    set_last_error(msg);
    return code;
}
inline int hip_fail(hipError_t e, const char* what) { return fail(MP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// No exception crosses the C ABI: every extern "C" body runs inside guarded().
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try { set_last_error("out of host memory (std::bad_alloc)"); } catch (...) {}
        return MP_ERR_NOMEM;
    } catch (const std::exception& ex) {
        try { set_last_error(std::string("unexpected exception: ") + ex.what()); } catch (...) {}
        return MP_ERR_INVALID;
    } catch (...) {
        try { set_last_error("unexpected exception"); } catch (...) {}
        return MP_ERR_INVALID;
    }
}

// An entry point that only checks its pointers: MP_ERR_INVALID with `what` unless `ok`, else `body` and MP_OK.
template <class F>
int checked(bool ok, const char* what, F&& body) noexcept {
    return guarded([&]() -> int {
        if (!ok) return fail(MP_ERR_INVALID, what);
        body();
        return MP_OK;
    });
}

#define MP_HIP(call)                                  \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

}  // namespace mp

struct mp_ctx {
    int device = 0;
    int cu_count = 0;
    // work-queue heads: one per launch, handed out round-robin so that launches on different streams never share one
    static constexpr uint32_t kCounters = 256;
    mp::DeviceBuffer counters;
    std::atomic<uint32_t> next_counter{0};
    std::atomic<uint32_t> packet_stack_regs{64};
    std::atomic<uint32_t> packet_tree_slots{16};  // slots per node of the cached packet walk's tree (read when a scene is uploaded)
    std::atomic<uint32_t> packet_samples{0};  // 0 = chosen by the launcher
    std::atomic<uint32_t> rays_per_lane{1};   // packet kernel: 1 = 64-ray walks, 2 = 128-ray walks (two rays per lane)
    std::atomic<uint32_t> blocks_per_cu{0};   // 0 = as many as fit (diagnostic knob: resident workgroups per CU)
    std::atomic<uint32_t> render_batch{0};    // tiles per launch of render() (0 = automatic)
    std::atomic<uint32_t> mask_cache{1};      // packet kernel: per-unit mask cache of the packet-level child rejection
    std::atomic<uint32_t> paths_pooled{1};    // path extension: 0 = render_paths_kernel, 1 = auto, 2 / 3 = always pooled (RenderLaunch::paths_pooled)
    std::atomic<uint32_t> multi_gather_staged{0};  // as the gathering context: 1 = every rank but rank 0 staged through pinned host memory
    uint32_t* take_counter() {  // one set of work-queue heads per launch in flight
        return counters.as<uint32_t>() +
               static_cast<size_t>(next_counter.fetch_add(1, std::memory_order_relaxed) % kCounters) * mp::kWorkQueues * mp::kWorkQueueStride;
    }
    // diagnostic knob: fewer resident workgroups per CU (the launchers size their grids as cu_count x blocks that fit)
    int launch_cus() const {
        const uint32_t bpc = blocks_per_cu.load();
        return bpc ? std::max(1, cu_count * static_cast<int>(bpc) / 8) : cu_count;
    }
    // Device copies of the tile lists (and hand-out orders) callers pass as host arrays.  A frame loop passes the same list every
    // frame: uploading it per launch would put a pageable host-to-device copy in the stream, which blocks the calling thread
    // until the stream has drained (measured: a full frame) and so serialises host and GPU.  Entries are compared by content.
    struct TileList {
        std::vector<mp_block> tiles;
        std::vector<uint32_t> order;
        mp::DeviceBuffer buf;  // tiles, then order; freed when the cache AND every caller that still holds the list have let go
        uint64_t last_use = 0;
    };
    using TileListRef = std::shared_ptr<TileList>;
    // Buffers of the render() worker (stream, device tile-major f32/u8 + tile list, pinned host mirrors), kept between calls:
    // creating and freeing them costs several milliseconds per render() otherwise.
    struct WorkerSlot {
        mp::Stream stream;
        mp::DeviceBuffer f32, u8, tile_list;
        mp::PinnedBuffer pinned_f32, pinned_u8;
        size_t tiles = 0, per_tile = 0;  // capacity: `tiles` tile slots of per_tile floats
        size_t first = 0, n = 0;  // batch in flight
        bool busy = false;
        ~WorkerSlot() {  // wait for the stream, free what it used, then destroy it
            stream.sync();
            for (mp::DeviceBuffer* b : {&f32, &u8, &tile_list}) b->reset();
            for (mp::PinnedBuffer* b : {&pinned_f32, &pinned_u8}) b->reset();
            stream.reset();
        }
    };
    using SlotRef = std::unique_ptr<WorkerSlot>;
    std::mutex slot_mutex;
    std::vector<SlotRef> free_slots;
    int acquire_slot(size_t tiles, size_t per_tile, SlotRef& out);
    void release_slot(SlotRef s);
    // progressive accumulation over several ranks: the render a shard's running state belongs to
    struct PassState {
        uint64_t seed = 0;
        uint32_t w = 0, h = 0, ts = 0, spp = 0, flags = 0, depth = 0, n = 0, rank = 0;
        const mp_scene* scene = nullptr;
        bool operator==(const PassState& o) const {
            return seed == o.seed && w == o.w && h == o.h && ts == o.ts && spp == o.spp && flags == o.flags && depth == o.depth &&
                   n == o.n && rank == o.rank && scene == o.scene;
        }
    };
    // Buffers of mp_render_frame_multi / mp_render_pass_multi.  As a rank: this device's shard (tile-major; between
    // MP_FLAG_ACCUMULATE passes it holds the running per-pixel state and never leaves the device), the rank's stream -- render and
    // the copy of the shard towards the gathering device are issued on it in order, so every rank's copy runs on its own stream
    // (its own xGMI link) and overlaps the others -- and the event recorded after the copy.  As the gathering context (ctxs[0]):
    // the rank-major gather buffer, the event after which it may be overwritten by the next frame's copies, and per peer device
    // whether direct peer access works (checked once) or the shard is staged through pinned host memory.
    struct MultiBuf {
        mp::Stream stream;
        mp::DeviceBuffer shard;
        mp::Event copied;
        mp::PinnedBuffer stage;  // only without peer access to the gathering device
        mp::DeviceBuffer gather;
        mp::Event untiled;
        bool untiled_valid = false;
        uint32_t staged_ranks = 0;  // as the gathering context: ranks of the last gathered frame staged through pinned host memory
        std::vector<int> peer;  // by device id: 0 = not asked yet, 1 = direct peer copies, 2 = staged through the host
        PassState acc;          // what the shard's running state belongs to ...
        uint32_t acc_next = 0;  // ... and the next sample it expects (0: none)
        ~MultiBuf() {  // wait for the stream, free what it used, then destroy it
            stream.sync();
            for (mp::DeviceBuffer* b : {&shard, &gather}) b->reset();
            stage.reset();
            for (mp::Event* e : {&copied, &untiled}) e->reset();
            stream.reset();
        }
    } multi;
    std::mutex multi_mu;
    // mp_ctx_last_kernels: the kernels of the last launching call (LaunchScope)
    std::mutex diag_mu;
    std::string last_kernels;
    static constexpr size_t kTileLists = 32;
    std::mutex tile_mutex;
    std::vector<TileListRef> tile_lists;
    uint64_t tile_clock = 0;
    // Returns device pointers and `keep`, a reference on the cache entry: the caller holds it until its launch is enqueued, so a
    // concurrent caller that evicts the entry (LRU, 32 lists) cannot free the buffer in between; the buffer is freed when the
    // last reference goes (the free then waits for the kernels already enqueued).
    int device_tiles(const mp_block* tiles, size_t n, const uint32_t* order, TileListRef& keep, const mp_block** d_tiles,
                     const uint32_t** d_order);
};

namespace mp {
// default material of the build-defined path extension: grey 0.75, no emission, no texture
inline mp_material default_material() {
    mp_material m{};
    for (int c = 0; c < 3; c++) m.albedo[c] = m.albedo2[c] = 0.75f;
    return m;
}
}  // namespace mp

struct mp_scene {
    mp_ctx* ctx = nullptr;
    mp::HostBvh host;
    mp::DevScene dev;  // borrowed pointers into the buffers below (an object group: into its members')
    mp::DeviceBuffer shade, vidx, vtex, tris_aos, pkt_valid;
    mp::DeviceBuffer nodes_aos, nodes_lit, nodes_pk;  // wide, literal and packet tree (empty: the cached packet walk keeps the wide tree)
    uint32_t packet_tree_slots = 16;  // the context's option when the scene was made (host-only scene: the default)
    uint32_t wide_nodes = 0, absorbed_nodes = 0;
    // material table of the path extension: shared by reference with the instanced scenes made from this scene (each keeps the
    // table it was created with alive; mp_scene_set_materials gives a scene a new table of its own)
    std::shared_ptr<mp::DeviceBuffer> mat_table;
    mp::DeviceBuffer inst;                // object group (mp_scene_group / mp_scene_instances): DevObject per member
    const mp_scene* inst_of = nullptr;    // ... first member; the group borrows its members' device arrays
    std::vector<const mp_scene*> members;
    bool one_object = false;              // mp_scene_instances: every member is inst_of
    std::vector<float> inst_t;
    std::vector<mp_material> materials{mp::default_material()};  // build-defined path extension defaults
    float sky = 1.0f;
    uint32_t material_count = 1;  // max TriangleShadingData.material + 1
    uint64_t device_bytes = 0;
    // An object group borrows its members' device arrays and host trees: every group holds one reference on each of its members,
    // so mp_scene_destroy on a member only drops the caller's reference and the arrays live until the last group has gone too.
    std::atomic<int> refs{1};
};

namespace mp {

// One record of mp_ctx_last_kernels: the launchers note their kernels in a list of the calling thread (family_launch.h: MP_LAUNCH); the
// outermost scope on a thread empties that list when it opens and, if anything was launched, files it with the context when it
// closes.  Entry points nest (mp_render_tile calls mp_render_tiles_device): the inner scopes do nothing.
struct LaunchScope {
    static inline thread_local int depth = 0;
    mp_ctx* ctx;
    explicit LaunchScope(mp_ctx* c) : ctx(c) {
        if (depth++ == 0) launch_log_clear();
    }
    ~LaunchScope() {
        if (--depth != 0 || !ctx) return;
        try {
            std::string names = launch_log_text();
            if (names.empty()) return;
            std::lock_guard<std::mutex> lk(ctx->diag_mu);
            ctx->last_kernels.swap(names);
        } catch (...) {}
    }
    LaunchScope(const LaunchScope&) = delete;
    LaunchScope& operator=(const LaunchScope&) = delete;
};

// api_sync.cpp
bool valid_settings(const mp_settings* st);
uint32_t pass_samples(const mp_settings& st);  // samples per pixel drawn by one launch
// ray segments of one pass over `pixels` pixels under the reference semantics: one Object::intersect per sample
uint64_t reference_segments(uint64_t pixels, const mp_settings& st);
// The refusals of render_tiles_device that the scene and the settings decide alone, before anything is launched (0 = none).
int render_refusal(const mp_scene* scene, const mp_settings& st);
// Renders `tiles` into a tile-major device buffer (launch only).
int render_tiles_device(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler& sampler, const mp_settings& st,
                        const mp_block* d_tiles, size_t n, float* d_out, void* stream, uint64_t* d_segments = nullptr,
                        const uint32_t* d_tile_order = nullptr, uint64_t* d_tile_cost = nullptr);

}  // namespace mp
