// C ABI (include/minipath_hip.h): the asynchronous render() / RenderProgress machinery (reference: src/renderer/machinery.rs).
#include <chrono>
#include <cstdlib>
#include <thread>

#include "api_common.h"

using namespace mp;

#ifndef MP_RENDER_SLOTS
#define MP_RENDER_SLOTS 3  // batches of tiles in flight per render() worker (measured on the metric's frame: 2 -> 50.4-51.1 ms, 3 -> 49.1-49.5, 4 -> 49.4-49.7; bare launch 48.8)
#endif

struct mp_render {
    // one worker thread per device (machinery.rs:51-116: one worker per core); worker i renders on ctxs[i] / scenes[i]
    std::vector<mp_ctx*> ctxs;
    std::vector<const mp_scene*> scenes;
    mp_camera_sampler sampler{};
    mp_settings settings{};
    mp_tile_started_cb started = nullptr;
    mp_tile_finished_cb finished = nullptr;
    void* user = nullptr;
    std::vector<mp_block> tiles;                // tile_ordering (machinery.rs:41-42)
    std::atomic<size_t> next_tile{0};           // next_tile_index (machinery.rs:43)
    std::atomic<size_t> done_tiles{0};
    std::atomic<bool> finished_flag{false};
    std::mutex image_mu;                        // Mutex<RgbaImage> (machinery.rs:39)
    // the host images: calloc'ed (zero pages come from the OS on first touch, i.e. when a worker files a tile -- not as a 40-MB fill
    // before the first launch), sizes in elements
    struct FreeDeleter { void operator()(void* p) const { std::free(p); } };
    std::unique_ptr<uint8_t, FreeDeleter> image_u8;
    std::unique_ptr<float, FreeDeleter> image_f32;
    size_t image_elems = 0;   // width * height * 4
    std::chrono::steady_clock::time_point start;
    std::mutex end_mu;
    bool ended = false;
    std::chrono::nanoseconds elapsed{0};
    std::vector<std::thread> workers;
    std::atomic<int> live_workers{0};
    size_t worker_count = 1;                     // contexts / worker threads of this render
    std::mutex status_mu;
    int status = MP_OK;                          // first error of any worker
    std::string error;
    size_t batch = 1;                            // tiles per get_next_tile() grab
};

namespace {

void render_worker(mp_render* r, size_t wi) {
    mp_ctx* ctx = r->ctxs[wi];
    const mp_scene* scene = r->scenes[wi];
    const mp_settings& st = r->settings;
    const uint32_t ts = st.tile_size;
    const size_t per_tile = static_cast<size_t>(ts) * ts * 4;  // floats (and u8 bytes) per tile slot
    // kSlots batches (mp_render_begin_multi sizes them) are in flight, each on its own stream: while the GPU renders and quantises
    // (color_to_image) the later ones and copies them to pinned host memory (the tail of one launch overlaps the start of the
    // next), this thread files the oldest batch's rows into the image and runs its callbacks.
    const size_t batch = r->batch;
    int my_status = MP_OK;  // this worker's view; the shared status records the first error of any worker
    auto set_error = [&](int code, const std::string& msg) {
        my_status = code;
        std::lock_guard<std::mutex> lk(r->status_mu);
        if (r->status == MP_OK) {
            r->status = code;
            r->error = msg;
        }
        r->next_tile.store(r->tiles.size(), std::memory_order_release);  // no new tiles for the other workers either
    };
    using Slot = mp_ctx::WorkerSlot;
    constexpr int kSlots = MP_RENDER_SLOTS;
    mp_ctx::SlotRef slot[kSlots];  // all held once the loop below runs
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) set_error(MP_ERR_HIP, std::string("render worker setup: ") + hipGetErrorString(e));
    for (mp_ctx::SlotRef& s : slot)
        if (my_status == MP_OK) {
            int rc = ctx->acquire_slot(batch, per_tile, s);
            if (rc) set_error(rc, mp_last_error());
        }

    const size_t total = r->tiles.size();
    // waits for the slot's batch and files it into the image (machinery.rs:78-99)
    auto retire = [&](Slot& s) {
        if (!s.busy) return;
        s.busy = false;
        hipError_t se = hipStreamSynchronize(s.stream.get());
        if (se != hipSuccess) { set_error(MP_ERR_HIP, std::string("tile readback: ") + hipGetErrorString(se)); return; }
        for (size_t i = 0; i < s.n; i++) {
            const mp_block& b = r->tiles[s.first + i];
            const size_t w = b.max_x - b.min_x;
            {
                std::lock_guard<std::mutex> lk(r->image_mu);  // image.lock().copy_from(..) machinery.rs:78-89
                for (uint32_t y = b.min_y; y < b.max_y; y++) {
                    const size_t src = i * per_tile + static_cast<size_t>(y - b.min_y) * ts * 4;
                    const size_t dst = (static_cast<size_t>(y) * st.width + b.min_x) * 4;
                    if (r->image_f32) std::memcpy(r->image_f32.get() + dst, s.pinned_f32.as<float>() + src, w * 16);
                    std::memcpy(r->image_u8.get() + dst, s.pinned_u8.as<uint8_t>() + src, w * 4);
                }
            }
            size_t done = r->done_tiles.fetch_add(1, std::memory_order_acq_rel) + 1;
            if (r->finished) r->finished(r->user, b, mp_progress{done, total});  // machinery.rs:93-99
        }
    };
    int cur = 0;
    while (my_status == MP_OK) {
        // get_next_tile (machinery.rs:205-208): abort() stores `len` so no new tiles are handed out
        // Batches taper towards the end of the frame (guided self-scheduling): the last batch's readback and filing are not
        // overlapped by rendering, so the last ones are small -- a quarter of what is left per slot and worker, at least four tiles.
        size_t first = r->next_tile.load(std::memory_order_acquire), take = 0;
        for (;;) {
            if (first >= total) break;
            const size_t left = total - first;
            take = std::min(left, std::max<size_t>(std::min<size_t>(batch, 4), std::min(batch, left / (4 * static_cast<size_t>(kSlots) * r->worker_count))));
            if (r->next_tile.compare_exchange_weak(first, first + take, std::memory_order_acq_rel, std::memory_order_acquire)) break;
        }
        if (first >= total) break;
        Slot& s = *slot[cur];
        retire(s);  // the batch issued kSlots rounds ago
        if (my_status != MP_OK) break;
        s.first = first, s.n = take;
        const mp_block* t = &r->tiles[first];
        if (r->started)
            for (size_t i = 0; i < s.n; i++) r->started(r->user, t[i]);  // machinery.rs:75
        const hipStream_t stream = s.stream.get();
        mp_block* d_tiles = s.tile_list.as<mp_block>();
        float* d_f32 = s.f32.as<float>();
        e = hipMemcpyAsync(d_tiles, t, s.n * sizeof(mp_block), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { set_error(MP_ERR_HIP, std::string("hipMemcpyAsync(tiles): ") + hipGetErrorString(e)); break; }
        int rc;
        {
            LaunchScope record(ctx);  // one batch = one record of mp_ctx_last_kernels
            rc = render_tiles_device(ctx, scene, r->sampler, st, d_tiles, s.n, d_f32, stream);
            std::string err;
            if (!rc) {
                rc = launch_quantise(d_f32, s.u8.as<uint8_t>(), static_cast<uint64_t>(s.n) * ts * ts, stream, err);
                if (rc) fail(rc, err);
            }
        }
        if (rc) { set_error(rc, mp_last_error()); break; }
        e = r->image_f32 ? hipMemcpyAsync(s.pinned_f32.get(), d_f32, s.n * per_tile * 4, hipMemcpyDeviceToHost, stream) : hipSuccess;
        if (e == hipSuccess) e = hipMemcpyAsync(s.pinned_u8.get(), s.u8.get(), s.n * per_tile, hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) { set_error(MP_ERR_HIP, std::string("tile readback: ") + hipGetErrorString(e)); break; }
        s.busy = true;
        cur = (cur + 1) % kSlots;
    }
    // drain in issue order: slot[cur] holds the older batch
    for (int k = 0; k < kSlots; k++)
        if (Slot* s = slot[(cur + k) % kSlots].get()) retire(*s);
    for (mp_ctx::SlotRef& s : slot) {
        if (!s) continue;
        s->stream.sync();
        s->busy = false;
        ctx->release_slot(std::move(s));
    }
    if (r->live_workers.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // the last worker out closes the render
        {
            std::lock_guard<std::mutex> lk(r->end_mu);  // machinery.rs:107-113
            r->elapsed = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - r->start);
            r->ended = true;
        }
        r->finished_flag.store(true, std::memory_order_release);
    }
}

}  // namespace

extern "C" {

int mp_render_begin(mp_ctx* ctx, const mp_scene* scene, const mp_camera* camera, const mp_settings* settings,
                    mp_tile_started_cb started, mp_tile_finished_cb finished, void* user, mp_render** out) {
    return mp_render_begin_multi(&ctx, &scene, 1, camera, settings, started, finished, user, out);
}

int mp_render_begin_multi(mp_ctx* const* ctxs, const mp_scene* const* scenes, int n, const mp_camera* camera,
                          const mp_settings* settings, mp_tile_started_cb started, mp_tile_finished_cb finished, void* user,
                          mp_render** out) {
    return guarded([&]() -> int {
    if (!ctxs || !scenes || n < 1 || n > 64 || !camera || !out || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (settings->flags & MP_FLAG_ACCUMULATE) return fail(MP_ERR_INVALID, "render() draws every sample of a tile at once (worker.rs:32-49): MP_FLAG_ACCUMULATE is for mp_render_tiles_device");
    for (int i = 0; i < n; i++) {
        if (!ctxs[i] || !scenes[i]) return fail(MP_ERR_INVALID, "NULL context / scene");
        if (scenes[i]->ctx != ctxs[i]) return fail(MP_ERR_INVALID, "scenes[i] must live on ctxs[i] (the scene is replicated per device)");
    }
    auto r = std::make_unique<mp_render>();
    r->ctxs.assign(ctxs, ctxs + n);
    r->scenes.assign(scenes, scenes + n);
    r->settings = *settings;
    camera_build_sampler(*camera, settings->width, settings->height, r->sampler);  // machinery.rs:65
    r->started = started;
    r->finished = finished;
    r->user = user;
    uint64_t shuffle = 0;
    if (settings->flags & MP_FLAG_SHUFFLE_TILES)
        shuffle = static_cast<uint64_t>(std::chrono::steady_clock::now().time_since_epoch().count()) | 1ull;
    r->tiles = tile_ordering(mp_block{0, 0, settings->width, settings->height}, settings->tile_size, shuffle);
    r->image_elems = static_cast<size_t>(settings->width) * settings->height * 4;
    r->image_u8.reset(static_cast<uint8_t*>(std::calloc(std::max<size_t>(r->image_elems, 1), 1)));   // RgbaImage::new :34 (zeroed)
    const bool want_f32 = !(settings->flags & MP_FLAG_IMAGE_U8_ONLY);
    if (want_f32) r->image_f32.reset(static_cast<float*>(std::calloc(std::max<size_t>(r->image_elems, 1), sizeof(float))));
    if (!r->image_u8 || (want_f32 && !r->image_f32)) return fail(MP_ERR_NOMEM, "host image allocation failed");
    // A batch is what one launch renders: enough work units to fill every CU a few times over, small enough that the tile
    // callbacks keep flowing and that several devices share the queue evenly (the reference hands out one tile per worker).
    const uint32_t ts = settings->tile_size;
    const size_t units_per_tile = static_cast<size_t>((ts + 7) / 8) * ((ts + 7) / 8);
    // (round 3: 32 tiles on 256 CUs -- measured on the metric's frame now that its kernel takes 22 ms: 16 / 32 / 64 / 128 / 510 tiles per
    // launch -> 24.2-26.3 / 24.2-24.5 / 24.8-25.8 / 25.3-26.1 / 28.2-28.8 ms wall; the last batch's readback is not overlapped)
    size_t batch = std::max<size_t>(1, (static_cast<size_t>(ctxs[0]->cu_count) * 8 + units_per_tile - 1) / units_per_tile);
    if (n > 1) batch = std::max<size_t>(1, std::min(batch, r->tiles.size() / (static_cast<size_t>(n) * 4)));
    if (ctxs[0]->render_batch.load() != 0) batch = ctxs[0]->render_batch.load();
    r->batch = std::max<size_t>(1, std::min(batch, r->tiles.size()));  // (the slots' buffers are sized by it)
    r->start = std::chrono::steady_clock::now();
    r->live_workers.store(n);
    r->worker_count = static_cast<size_t>(n);
    try {
        for (int i = 0; i < n; i++) r->workers.emplace_back(render_worker, r.get(), static_cast<size_t>(i));
    } catch (const std::exception& ex) {
        r->next_tile.store(r->tiles.size(), std::memory_order_release);  // the workers already running find no tiles
        for (auto& t : r->workers) t.join();
        return fail(MP_ERR_UNSUPPORTED, std::string("thread spawn failed: ") + ex.what());  // machinery.rs:116
    }
    *out = r.release();
    return MP_OK;
    });
}

int mp_render_progress(const mp_render* r, mp_progress* out) {
    return checked(r && out, "NULL argument", [&] {
        out->finished = r->done_tiles.load(std::memory_order_acquire);
        out->total = r->tiles.size();
    });
}

int mp_render_is_finished(const mp_render* r, int* finished) {
    return checked(r && finished, "NULL argument", [&] { *finished = r->finished_flag.load(std::memory_order_acquire) ? 1 : 0; });
}

int mp_render_elapsed_ns(const mp_render* rc, uint64_t* ns) {
    return guarded([&]() -> int {
    if (!rc || !ns) return fail(MP_ERR_INVALID, "NULL argument");
    mp_render* r = const_cast<mp_render*>(rc);
    std::lock_guard<std::mutex> lk(r->end_mu);
    auto d = r->ended ? r->elapsed
                      : std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - r->start);
    *ns = static_cast<uint64_t>(d.count());
    return MP_OK;
    });
}

int mp_render_abort(mp_render* r) {
    return checked(r, "NULL argument", [&] { r->next_tile.store(r->tiles.size(), std::memory_order_release); });  // machinery.rs:161-165
}

int mp_render_wait(mp_render* r) {
    return guarded([&]() -> int {
    if (!r) return fail(MP_ERR_INVALID, "NULL argument");
    for (auto& t : r->workers)
        if (t.joinable()) t.join();
    if (r->status != MP_OK) return fail(r->status, r->error);
    return MP_OK;
    });
}

int mp_render_image_u8(mp_render* r, uint8_t* dst) {
    return checked(r && dst, "NULL argument", [&] {
        std::lock_guard<std::mutex> lk(r->image_mu);
        std::memcpy(dst, r->image_u8.get(), r->image_elems);
    });
}

int mp_render_image_f32(mp_render* r, float* dst) {
    return guarded([&]() -> int {
    if (!r || !dst) return fail(MP_ERR_INVALID, "NULL argument");
    if (!r->image_f32) return fail(MP_ERR_UNSUPPORTED, "this render keeps the u8 image only (MP_FLAG_IMAGE_U8_ONLY)");
    std::lock_guard<std::mutex> lk(r->image_mu);
    std::memcpy(dst, r->image_f32.get(), r->image_elems * 4);
    return MP_OK;
    });
}

void mp_render_destroy(mp_render* r) {
    if (!r) return;
    r->next_tile.store(r->tiles.size(), std::memory_order_release);
    for (auto& t : r->workers)
        if (t.joinable()) t.join();
    delete r;
}

}  // extern "C"
