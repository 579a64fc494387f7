// C ABI (include/minipath_hip.h): the context -- create, destroy, options, queries, its tile-list cache and its pool of render()
// worker slots -- and the camera and tile-ordering wrappers.  The thread's last error lives here.
#include "api_common.h"

namespace mp {
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
}  // namespace mp

using namespace mp;

int mp_ctx::device_tiles(const mp_block* tiles, size_t n, const uint32_t* order, TileListRef& keep, const mp_block** d_tiles,
                         const uint32_t** d_order) {
    TileListRef evicted;  // released after the lock is dropped: its free may wait for the device
    {
        std::lock_guard<std::mutex> lock(tile_mutex);
        const size_t tb = n * sizeof(mp_block), ob = order ? n * sizeof(uint32_t) : 0;
        TileListRef hit;
        for (TileListRef& e : tile_lists)
            if (e->tiles.size() == n && e->order.size() == (order ? n : 0) && std::memcmp(e->tiles.data(), tiles, tb) == 0 &&
                (!order || std::memcmp(e->order.data(), order, ob) == 0)) {
                hit = e;
                break;
            }
        if (!hit) {
            if (tile_lists.size() >= kTileLists) {  // evict the least recently used list
                size_t lru = 0;
                for (size_t i = 1; i < tile_lists.size(); i++)
                    if (tile_lists[i]->last_use < tile_lists[lru]->last_use) lru = i;
                evicted = std::move(tile_lists[lru]);
                tile_lists.erase(tile_lists.begin() + static_cast<std::ptrdiff_t>(lru));
            }
            auto e = std::make_shared<TileList>();
            e->tiles.assign(tiles, tiles + n);
            if (order) e->order.assign(order, order + n);
            MP_HIP(e->buf.grow(tb + ob));
            hipError_t err = hipMemcpy(e->buf.get(), tiles, tb, hipMemcpyHostToDevice);
            if (err == hipSuccess && order) err = hipMemcpy(e->buf.as<unsigned char>() + tb, order, ob, hipMemcpyHostToDevice);
            if (err != hipSuccess) return hip_fail(err, "hipMemcpy(tile list)");
            tile_lists.push_back(e);
            hit = e;
        }
        hit->last_use = ++tile_clock;
        *d_tiles = hit->buf.as<const mp_block>();
        if (d_order) *d_order = order ? reinterpret_cast<const uint32_t*>(hit->buf.as<unsigned char>() + tb) : nullptr;
        keep = std::move(hit);
    }
    return MP_OK;
}

int mp_ctx::acquire_slot(size_t tiles, size_t per_tile, SlotRef& out) {
    {
        std::lock_guard<std::mutex> lock(slot_mutex);
        for (size_t i = 0; i < free_slots.size(); i++)
            if (free_slots[i]->tiles * free_slots[i]->per_tile >= tiles * per_tile && free_slots[i]->tiles >= tiles) {
                out = std::move(free_slots[i]);
                free_slots.erase(free_slots.begin() + static_cast<std::ptrdiff_t>(i));
                out->busy = false;
                return MP_OK;
            }
    }
    auto s = std::make_unique<WorkerSlot>();
    s->tiles = tiles;
    s->per_tile = per_tile;
    hipError_t e = s->stream.ensure();
    if (e == hipSuccess) e = s->f32.grow(tiles * per_tile * 4);
    if (e == hipSuccess) e = s->u8.grow(tiles * per_tile);
    if (e == hipSuccess) e = s->tile_list.grow(tiles * sizeof(mp_block));
    if (e == hipSuccess) e = s->pinned_f32.grow(tiles * per_tile * 4);
    if (e == hipSuccess) e = s->pinned_u8.grow(tiles * per_tile);
    if (e != hipSuccess) return hip_fail(e, "render worker buffers");
    out = std::move(s);
    return MP_OK;
}

void mp_ctx::release_slot(SlotRef s) {
    if (!s) return;
    std::lock_guard<std::mutex> lock(slot_mutex);
    if (free_slots.size() < 8) free_slots.push_back(std::move(s));
}

namespace {

// mp_ctx_set_option: the keys, their ranges and the refusal of a value outside
struct Option {
    const char* key;
    std::atomic<uint32_t> mp_ctx::*field;
    bool (*ok)(int);
    const char* refusal;
};
const Option kOptions[] = {
    {"packet_stack_registers", &mp_ctx::packet_stack_regs, [](int v) { return v >= 1 && v <= 64; }, "packet_stack_registers must be in 1..64"},
    {"packet_tree_slots", &mp_ctx::packet_tree_slots, [](int v) { return v == 8 || v == 16; }, "packet_tree_slots must be 8 or 16"},
    {"packet_mask_cache", &mp_ctx::mask_cache, [](int v) { return v >= 0 && v <= 2; }, "packet_mask_cache must be 0 (off), 1 or 2 (on)"},
    {"paths_pooled", &mp_ctx::paths_pooled, [](int v) { return v >= 0 && v <= 3; },
     "paths_pooled must be 0 (one pass per walk), 1 (auto), 2 (always, two passes) or 3 (always, up to four passes)"},
    {"multi_gather_staged", &mp_ctx::multi_gather_staged, [](int v) { return v >= 0 && v <= 1; },
     "multi_gather_staged must be 0 (direct copies where the devices reach each other) or 1 (through pinned host memory)"},
    {"packet_rays_per_lane", &mp_ctx::rays_per_lane, [](int v) { return v == 1 || v == 2; }, "packet_rays_per_lane must be 1 or 2"},
    {"render_batch_tiles", &mp_ctx::render_batch, [](int v) { return v >= 0 && v <= 65536; }, "render_batch_tiles must be in 0..65536 (0 = automatic)"},
    {"blocks_per_cu", &mp_ctx::blocks_per_cu, [](int v) { return v >= 0 && v <= 8; }, "blocks_per_cu must be in 0..8 (0 = as many as fit)"},
    {"packet_samples_in_flight", &mp_ctx::packet_samples, [](int v) { return v >= 0 && v <= 64 && (v & (v - 1)) == 0; },
     "packet_samples_in_flight must be 0 (automatic) or a power of two up to 64"},
};

}  // namespace

extern "C" {

const char* mp_last_error(void) { return g_last_error.c_str(); }
const char* mp_version(void) { return "minipath_hip 0.2 (gfx950)"; }

int mp_ctx_create(int device_id, mp_ctx** out) {
    return guarded([&]() -> int {
    if (!out) return fail(MP_ERR_INVALID, "out is NULL");
    int count = 0;
    MP_HIP(hipGetDeviceCount(&count));
    if (device_id < 0 || device_id >= count) return fail(MP_ERR_INVALID, "device_id out of range");
    DeviceGuard g(device_id);
    if (!g.ok) return fail(MP_ERR_HIP, "hipSetDevice failed");
    hipDeviceProp_t prop;
    MP_HIP(hipGetDeviceProperties(&prop, device_id));
    auto ctx = std::make_unique<mp_ctx>();
    ctx->device = device_id;
    ctx->cu_count = prop.multiProcessorCount;
    const size_t counter_bytes = static_cast<size_t>(mp_ctx::kCounters) * kWorkQueues * kWorkQueueStride * sizeof(uint32_t);
    MP_HIP(ctx->counters.grow(counter_bytes));
    MP_HIP(hipMemset(ctx->counters.get(), 0, counter_bytes));
    *out = ctx.release();
    return MP_OK;
    });
}

void mp_ctx_destroy(mp_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    delete ctx;
}

int mp_ctx_set_option(mp_ctx* ctx, const char* key, int value) {
    return guarded([&]() -> int {
    if (!ctx || !key) return fail(MP_ERR_INVALID, "NULL argument");
    for (const Option& o : kOptions)
        if (std::strcmp(key, o.key) == 0) {
            if (!o.ok(value)) return fail(MP_ERR_INVALID, o.refusal);
            (ctx->*o.field).store(static_cast<uint32_t>(value));
            return MP_OK;
        }
    return fail(MP_ERR_INVALID, std::string("unknown option: ") + key);
    });
}

int mp_ctx_query(mp_ctx* ctx, const char* key, uint64_t* value) {
    return guarded([&]() -> int {
    if (!ctx || !key || !value) return fail(MP_ERR_INVALID, "NULL argument");
    if (std::strcmp(key, "multi_staged_ranks") == 0) {
        std::lock_guard<std::mutex> lk(ctx->multi_mu);
        *value = ctx->multi.staged_ranks;
        return MP_OK;
    }
    return fail(MP_ERR_INVALID, std::string("unknown query: ") + key);
    });
}

int mp_ctx_last_kernels(mp_ctx* ctx, char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int {
    if (!ctx || (cap && !buf)) return fail(MP_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ctx->diag_mu);
    if (needed) *needed = ctx->last_kernels.size();
    if (cap) {
        const size_t n = std::min(cap - 1, ctx->last_kernels.size());
        std::memcpy(buf, ctx->last_kernels.data(), n);
        buf[n] = 0;
    }
    return MP_OK;
    });
}

int mp_ctx_device(const mp_ctx* ctx, int* device_id, int* cu_count) {
    return checked(ctx, "ctx is NULL", [&] {
        if (device_id) *device_id = ctx->device;
        if (cu_count) *cu_count = ctx->cu_count;
    });
}

// ---- camera ---------------------------------------------------------------------------------------------------
int mp_camera_default(mp_camera* cam) {
    return checked(cam, "cam is NULL", [&] { camera_default(*cam); });
}
int mp_camera_look_at(mp_camera* cam, const float eye[3], const float at[3], const float up[3]) {
    return checked(cam && eye && at && up, "NULL argument", [&] { camera_look_at(*cam, eye, at, up); });
}
int mp_camera_look_direction(mp_camera* cam, const float eye[3], const float fwd[3], const float up[3]) {
    return checked(cam && eye && fwd && up, "NULL argument", [&] { camera_look_direction(*cam, eye, fwd, up); });
}
int mp_camera_translate(mp_camera* cam, const float t[3]) {
    return checked(cam && t, "NULL argument", [&] {
        for (int k = 0; k < 3; k++) cam->t[k] = t[k] + cam->t[k];  // (Translation3 * Isometry3).translation
    });
}
int mp_camera_basis(const mp_camera* cam, float center[3], float fwd[3], float up[3], float right[3]) {
    return checked(cam && center && fwd && up && right, "NULL argument", [&] { camera_basis(*cam, center, fwd, up, right); });
}
int mp_camera_build_sampler(const mp_camera* cam, uint32_t width, uint32_t height, mp_camera_sampler* out) {
    return guarded([&]() -> int {
    if (!cam || !out) return fail(MP_ERR_INVALID, "NULL argument");
    if (width == 0 || height == 0) return fail(MP_ERR_INVALID, "empty resolution");
    camera_build_sampler(*cam, width, height, *out);
    return MP_OK;
    });
}

int mp_tile_ordering(mp_block block, uint32_t tile_size, uint64_t shuffle_seed, mp_block* out, size_t cap, size_t* n) {
    return guarded([&]() -> int {
    if (tile_size == 0) return fail(MP_ERR_INVALID, "tile_size must be non-zero (NonZeroU32)");
    if (!n) return fail(MP_ERR_INVALID, "n is NULL");
    std::vector<mp_block> t = tile_ordering(block, tile_size, shuffle_seed);
    *n = t.size();
    if (out && !t.empty() && cap) std::memcpy(out, t.data(), std::min(cap, t.size()) * sizeof(mp_block));
    return MP_OK;
    });
}

}  // extern "C"
