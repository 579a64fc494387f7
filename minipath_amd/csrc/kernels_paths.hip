// The fused path kernels of the build-defined path extension: one pass per walk (render_paths_kernel) and the pooled form with its
// per-wave pool in global memory.
// One translation unit and one code object of libminipath_hip.so (kernel_table.h); the lane mapping and the arithmetic contract
// are described in kernels.hip.
// The unit triangle masks of this family stay without their far-side terms (mask_cache.h, tri_may_hit): only the camera pass of a
// path runs the cached walk, the terms gain nothing measurable here (the stand-in's depth-8 paths: 546.2 against 546.8 ms), and
// leaf_mask_slow's changed register use moved these kernels' allocation, which cost the teapot's depth-8 paths 2.7 % (45.47 ->
// 46.71 ms over five alternating rounds, profiles/mask_far_notes.md).  Without them the unit's device code is what it was.
#ifndef MP_NO_MASK_FAR
#define MP_NO_MASK_FAR
#endif
// Nor does this family take the one-test pass entry (packet_walk.h, trace_packet): one pass in depth + 1 of a path is a camera pass,
// so the saving is out of reach of a measurement here, while any change of these kernels' register allocation is not (above).
#ifndef MP_NO_ENTRY_FOLD
#define MP_NO_ENTRY_FOLD
#endif
#include "packet_walk.h"
#include "render_state.h"
#include "path_shading.h"

namespace mp {
namespace {

// MCACHE: the camera pass runs the cached packet walk (MaskCache; the wave's header + tables are the last kMaskCacheDwords dwords of
// its LDS region)
template <int S, bool OBJ, bool RGB, bool MCACHE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MP_PATHS_WPE, 8))) void render_paths_kernel(RenderParams) {
    constexpr int N = RGB ? 3 : 1;
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;  // RenderParams through short-lived views (params_view)
    MaskCache mc{nullptr};
    if (MCACHE) {
        const RenderParams& P0 = params_view(KP);
        mc.lds = reinterpret_cast<uint32_t*>(smem + static_cast<size_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6) + 1) * P0.lds_per_wave) - kMaskCacheDwords;
    }
    constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : 2;
    constexpr int BH = 64 / S / BW;
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    const int pix = lane / S, sub = lane % S;
    unsigned long long segs = 0;  // wave-uniform
    uint32_t qstate = blockIdx.x % kWorkQueues;
    for (;;) {
        const RenderParams& P = params_view(KP);  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc[N], cnt;  // pixel_sum (r=g=b for a grey table: one channel) and alpha (worker.rs:40)
        if (RGB) pixel_state_load3(P, off, inpix, reinterpret_cast<float (&)[3]>(acc[0]), cnt);
        else pixel_state_load(P, off, inpix, sub == 0, acc[0], cnt);
        if (MCACHE) {  // a new unit: other pixels, other bounds
            if (lane == 0) mc.lds[kHdrState] = 0xFFFFFFFFu;
            wave_lds_sync();
        }
        // passes are aligned to multiples of S in the absolute sample index, so that a chunk boundary (MP_FLAG_CHUNKED_SUM) never
        // falls inside a pass; lanes outside [s_begin, s_end) add +0.0, which is exact
        const uint32_t s_begin = P.s_begin, s_end = P.s_end, max_depth = P.max_depth;
        for (uint32_t s0 = s_begin & ~static_cast<uint32_t>(S - 1); s0 < s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            const bool act = inpix && s >= s_begin && s < s_end;
            Rng rng;
            rng_zero(rng);
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            {
                const RenderParams& G = params_view(KP);  // ray generation
                if (act) {
                    rng_seed(rng, sample_key(G.gen, px, py, s));
                    sample_ray_rng(G.gen, px, py, rng, r);
                }
            }
            float L[N], thr[N];
#pragma unroll
            for (int c = 0; c < N; c++) { L[c] = 0.0f; thr[c] = 1.0f; }
            bool alive = act, primary_hit = false;
            PacketHit h;
            for (uint32_t depth = 1; depth <= max_depth; depth++) {
                const uint64_t alive_m = __ballot(alive);
                if (alive_m == 0) break;
                segs += static_cast<unsigned long long>(__popcll(alive_m));
                h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                uint32_t hinst = 0u;
                {
                    const RenderParams& W = params_view(KP);  // walk
                    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * W.lds_per_wave);
                    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
                    if (depth == 1 && OBJ) {  // camera rays of an object group: one packet walk per member
                        RegStack rst(nullptr, lane);
                        HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet_objects<false>(W.scene, r, alive, hst, h, hinst);
                        else trace_packet_objects<(S >= 8)>(W.scene, r, alive, rst, h, hinst);
                    } else if (depth == 1) {
                        const bool go = alive && may_hit_scene(W.scene, r);
                        if (__ballot(go) != 0) {
                            RegStack rst(nullptr, lane);
                            HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                            if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet<false>(W.scene, r, go, hst, h);
                            else trace_packet<(S >= 8), RegStack, MCACHE>(W.scene, r, go, rst, h, mc);
                        }
                    } else {
                        // bounce rays: group walk (once per member of an object group)
                        GroupHit gh;
                        trace_objects<OBJ>(W.scene, r, alive, q, stack, gh);
                        h.t = gh.t; h.u = gh.u; h.v = gh.v; h.prim = gh.prim;
                        hinst = gh.inst;
                    }
                }
                const RenderParams& V = params_view(KP);  // shade + bounce
                if (alive) alive = path_vertex<OBJ, N>(V.scene, h, depth, max_depth, rng, r, L, thr, primary_hit, hinst);
            }
            {   // (the mask of this pixel's lanes is rebuilt from the lane id here: two registers less across the walks)
                int l_ = lane;
                asm volatile("" : "+v"(l_));
                const uint64_t pixel_lanes = (S == 64 ? ~0ull : ((1ull << (S & 63)) - 1ull)) << (l_ & ~(S - 1));
                cnt += static_cast<float>(__popcll(__ballot(primary_hit) & pixel_lanes));
            }
#pragma unroll
            for (int c = 0; c < N; c++) add_samples_in_order<S>(acc[c], L[c], lane);
            const RenderParams& A = params_view(KP);  // accumulation
            if (!RGB && A.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= s_end) chunk_flush(A, off, inpix && sub == 0, acc[0]);
        }
        const RenderParams& E = params_view(KP);  // unit end
        if (inpix && sub == 0) {
            if (RGB) pixel_state_store3(E, off, reinterpret_cast<const float (&)[3]>(acc[0]), cnt);
            else pixel_state_store(E, off, acc[0], cnt);
        }
        if (E.tile_cost && lane == 0) atomicAdd(E.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
    const RenderParams& Z = params_view(KP);
    if (lane == 0 && Z.segments && segs) atomicAdd(Z.segments, segs);
}

// ---- pooled form of render_paths_kernel (round 3) ----------------------------------------------------------------------------
// The fused kernel above traces the bounce rays of ONE pass (8 pixels x 8 samples = at most 64 rays) per call of the 8-lane-group
// walk, and a ray's walk takes 10 to 80 steps: when the queue runs dry the groups idle until the slowest ray of the call finishes
// -- 13 % of the group-iterations of a 64-ray call on the stand-in, 6.5 % of a 256-ray call (tools/sim_collapse.py's traces;
// profiles/r03_notes.md).  Here a wave keeps NSUB passes in flight: per bounce, the passes are shaded one after the other, lane =
// path, and their rays are compacted into ONE queue of up to 64 * NSUB rays that the walk drains in a single call.  The state of
// the passes that are not being shaded -- RNG, radiance, throughput, flags: 11 dwords per path -- and the queue itself (origin,
// direction, inverse direction, hit: 13 dwords per ray) live in a per-wave slab of global memory (RenderParams::pool, 24 dwords
// x 64 * NSUB per wave, L2-resident): the "rays laid out SoA + stream compaction" of the north star, inside one persistent wave.
// Nothing of a path is live in registers across the walk, so the kernel fits 64 VGPRs = 8 waves per SIMD.
// Per path the operations, their order and the RNG stream are those of render_paths_kernel (same path_vertex, same walks, samples
// added in index order): the frame is bit-identical (tests run both kernels on the same cases).
#ifndef MP_POOL_WPE
#define MP_POOL_WPE 8
#endif
constexpr int kPoolQueueRows = 13, kPoolStateRows = 11;
__host__ __device__ constexpr uint32_t pool_floats_per_wave(int nsub) { return static_cast<uint32_t>((kPoolQueueRows + kPoolStateRows) * 64 * nsub); }
constexpr uint32_t kPoolAlive = 1u, kPoolPrimary = 2u, kPoolQueued = 4u;  // flags word: bits 0..2, queue slot << 8

template <int NSUB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MP_POOL_WPE, 8))) void render_paths_pooled_kernel(RenderParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;
    constexpr int S = 8, BW = 4, BH = 2, QN = 64 * NSUB;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);  // uniform: the pool / stack pointers stay in SGPRs
    const int pix = lane / S, sub = lane % S;
    unsigned long long segs = 0;  // wave-uniform
    uint32_t qstate = blockIdx.x % kWorkQueues;
    float* q;        // ray queue: kPoolQueueRows rows x QN slots
    uint32_t* park;  // parked path state: kPoolStateRows rows x QN (slot = pass * 64 + lane): rng 8, L, thr, flags
    uint2* stack;
    {
        const RenderParams& P0 = params_view(KP);
        q = P0.pool + static_cast<size_t>(blockIdx.x * 4u + static_cast<uint32_t>(wave)) * P0.pool_stride;
        park = reinterpret_cast<uint32_t*>(q + kPoolQueueRows * QN);
        stack = reinterpret_cast<uint2*>(smem + static_cast<size_t>(wave) * P0.lds_per_wave);
    }
    auto park_store = [&](int j, const Rng& rng, float L, float thr, uint32_t flags) {
        // streamed (non-temporal): 200 MB of parked state per launch must not push the scene out of the L2
        uint32_t* p = park + j * 64 + lane;
        __builtin_nontemporal_store(rng.s0.lo, p + 0 * QN); __builtin_nontemporal_store(rng.s0.hi, p + 1 * QN);
        __builtin_nontemporal_store(rng.s1.lo, p + 2 * QN); __builtin_nontemporal_store(rng.s1.hi, p + 3 * QN);
        __builtin_nontemporal_store(rng.s2.lo, p + 4 * QN); __builtin_nontemporal_store(rng.s2.hi, p + 5 * QN);
        __builtin_nontemporal_store(rng.s3.lo, p + 6 * QN); __builtin_nontemporal_store(rng.s3.hi, p + 7 * QN);
        __builtin_nontemporal_store(as_u(L), p + 8 * QN); __builtin_nontemporal_store(as_u(thr), p + 9 * QN); __builtin_nontemporal_store(flags, p + 10 * QN);
    };
    // bounce ray of a path that is still alive: into the queue (compacted over the lanes whose ray can reach the scene at all)
    auto push_ray = [&](const DevScene& sc, const Ray& r, bool alive, uint32_t& nq, uint32_t& flags) {
        const bool queued = alive && may_hit_scene(sc, r);
        const uint64_t am = __ballot(queued);
        const uint32_t slot = nq + static_cast<uint32_t>(rank_below(am));
        if (queued) {
            q[0 * QN + slot] = r.ox; q[1 * QN + slot] = r.oy; q[2 * QN + slot] = r.oz;
            q[3 * QN + slot] = r.dx; q[4 * QN + slot] = r.dy; q[5 * QN + slot] = r.dz;
            q[6 * QN + slot] = r.ix; q[7 * QN + slot] = r.iy; q[8 * QN + slot] = r.iz;
            flags |= kPoolQueued | (slot << 8);
        }
        nq += static_cast<uint32_t>(__popcll(am));
    };
    for (;;) {
        const RenderParams& P = params_view(KP);  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc, cnt;  // pixel_sum (grey table: one channel) and alpha (worker.rs:40)
        pixel_state_load(P, off, inpix, sub == 0, acc, cnt);
        const uint32_t s_begin = P.s_begin, s_end = P.s_end, max_depth = P.max_depth;
        // a batch = NSUB consecutive passes of S samples, aligned in the absolute sample index (so that a 256-sample chunk boundary
        // of MP_FLAG_CHUNKED_SUM never falls inside a batch); samples outside [s_begin, s_end) add +0.0, which is exact
        for (uint32_t s0 = s_begin & ~static_cast<uint32_t>(S * NSUB - 1); s0 < s_end; s0 += S * NSUB) {
            uint32_t nq = 0, na = 0;  // rays in the queue / paths alive, over all passes of the batch (wave-uniform)
            // ---- segment 1: camera rays of every pass as one packet each, then the first vertex
#pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                const uint32_t s = s0 + static_cast<uint32_t>(j * S + sub);
                const bool act = inpix && s >= s_begin && s < s_end;
                Rng rng;
                rng_zero(rng);
                Ray r;
                r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
                {
                    const RenderParams& G = params_view(KP);  // ray generation
                    if (act) {
                        rng_seed(rng, sample_key(G.gen, px, py, s));
                        sample_ray_rng(G.gen, px, py, rng, r);
                    }
                }
                segs += static_cast<unsigned long long>(__popcll(__ballot(act)));
                PacketHit h;
                h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                {
                    const RenderParams& W = params_view(KP);  // walk
                    const bool go = act && may_hit_scene(W.scene, r);
                    if (__ballot(go) != 0) {
                        RegStack rst(nullptr, lane);
                        HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet<false>(W.scene, r, go, hst, h);
                        else trace_packet<true>(W.scene, r, go, rst, h);
                    }
                }
                const RenderParams& V = params_view(KP);  // shade + bounce
                float L[1] = {0.0f}, thr[1] = {1.0f};
                bool alive = act, primary_hit = false;
                if (alive) alive = path_vertex<false, 1>(V.scene, h, 1u, max_depth, rng, r, L, thr, primary_hit);
                uint32_t flags = (alive ? kPoolAlive : 0u) | (primary_hit ? kPoolPrimary : 0u);
                push_ray(V.scene, r, alive, nq, flags);
                na += static_cast<uint32_t>(__popcll(__ballot(alive)));
                park_store(j, rng, L[0], thr[0], flags);
            }
            // ---- segments 2 .. max_depth: one walk over the rays of all passes, then the passes' vertices one after the other
            for (uint32_t depth = 2; depth <= max_depth && na != 0u; depth++) {
                segs += na;
                wave_mem_sync();  // the queue written above is read by other lanes of this wave
                if (nq != 0u) {
                    const RenderParams& W = params_view(KP);
                    trace_wave_pool<QN>(W.scene, q, stack, static_cast<int>(nq));
                }
                wave_mem_sync();
                nq = 0;
                na = 0;
    #pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                    const uint32_t* p = park + j * 64 + lane;
                    uint32_t flags = __builtin_nontemporal_load(p + 10 * QN);
                    bool alive = (flags & kPoolAlive) != 0u;
                    if (__ballot(alive) == 0) continue;  // the whole pass is finished: its parked L / flags stay as they are
                    Rng rng;
                    auto ld = [&](int row) { return static_cast<uint64_t>(__builtin_nontemporal_load(p + row * QN)); };
                    auto ld2 = [&](int row) { return rm::U64{__builtin_nontemporal_load(p + row * QN), __builtin_nontemporal_load(p + (row + 1) * QN)}; };
                    rng.s0 = ld2(0); rng.s1 = ld2(2);
                    rng.s2 = ld2(4); rng.s3 = ld2(6);
                    float L[1] = {as_f(static_cast<uint32_t>(ld(8)))}, thr[1] = {as_f(static_cast<uint32_t>(ld(9)))};
                    bool primary_hit = (flags & kPoolPrimary) != 0u;
                    Ray r;
                    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
                    PacketHit h;
                    h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                    if (alive && (flags & kPoolQueued)) {  // the ray this path shot and what it hit (a ray that was not queued missed)
                        const uint32_t slot = flags >> 8;
                        r.ox = q[0 * QN + slot]; r.oy = q[1 * QN + slot]; r.oz = q[2 * QN + slot];
                        r.dx = q[3 * QN + slot]; r.dy = q[4 * QN + slot]; r.dz = q[5 * QN + slot];
                        h.t = q[9 * QN + slot]; h.prim = as_u(q[10 * QN + slot]); h.u = q[11 * QN + slot]; h.v = q[12 * QN + slot];
                    }
                    const RenderParams& V = params_view(KP);
                    if (alive) alive = path_vertex<false, 1>(V.scene, h, depth, max_depth, rng, r, L, thr, primary_hit);
                    flags = (alive ? kPoolAlive : 0u) | (primary_hit ? kPoolPrimary : 0u);
                    // every lane of this pass has read its old slot (the loads above feed the stores below); the new slots are no
                    // higher than the old ones of this pass, so later passes' rays and hits are untouched
                    push_ray(V.scene, r, alive, nq, flags);
                    na += static_cast<uint32_t>(__popcll(__ballot(alive)));
                    park_store(j, rng, L[0], thr[0], flags);
                }
            }
            // ---- pixel_sum += sample, strictly in sample order (worker.rs:41-43): the passes in index order
#pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                const uint32_t* p = park + j * 64 + lane;
                const float L = as_f(p[8 * QN]);
                const bool primary_hit = (p[10 * QN] & kPoolPrimary) != 0u;
                {
                    int l_ = lane;
                    asm volatile("" : "+v"(l_));
                    const uint64_t pixel_lanes = ((1ull << S) - 1ull) << (l_ & ~(S - 1));
                    cnt += static_cast<float>(__popcll(__ballot(primary_hit) & pixel_lanes));
                }
                add_samples_in_order<S>(acc, L, lane);
            }
            const RenderParams& A = params_view(KP);  // accumulation
            if (A.chunked && ((s0 + S * NSUB) & (kSumChunk - 1u)) == 0u && s0 + S * NSUB <= s_end) chunk_flush(A, off, inpix && sub == 0, acc);
        }
        const RenderParams& E = params_view(KP);  // unit end
        if (inpix && sub == 0) pixel_state_store(E, off, acc, cnt);
        if (E.tile_cost && lane == 0) atomicAdd(E.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
    const RenderParams& Z = params_view(KP);
    if (lane == 0 && Z.segments && segs) atomicAdd(Z.segments, segs);
}

static_assert(kPlanPoolFloatsPerSub == pool_floats_per_wave(1), "launch_plan.h sizes the launches with the device code's constants");

MP_FAMILY_LAUNCHER(MP_KERNELS_PATHS)

}  // namespace

// launch_render_tiles with a path extension (L.max_depth > 0): `plan` is plan_render_tiles(L), not refused
int launch_paths(const RenderLaunch& L, const LaunchPlan& plan, hipStream_t st, std::string& err) {
    RenderParams P;
    fill_render(P, L, plan);
    int rc = zero_work_queues(L, st, err);
    if (rc) return rc;
    if (plan.pool_bytes) {
        rc = check(hipMallocAsync(reinterpret_cast<void**>(&P.pool), plan.pool_bytes, st), "hipMallocAsync(path pool)", err);
        if (rc) return rc;
    }
    rc = launch(plan.kernel, plan.grid, 256, plan.lds, st, err, P);
    if (P.pool) (void)hipFreeAsync(P.pool, st);
    return rc;
}

#ifdef MP_PROF_MISSES
int prof_add_paths(unsigned long long* sum, int reset) { return prof_add_unit(sum, reset); }
#endif

}  // namespace mp
