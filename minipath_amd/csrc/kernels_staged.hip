// The staged ("wavefront") evaluation of the path extension: its six kernels, their state in global memory, and the batch / chunk /
// depth loops that launch them.
// One translation unit and one code object of libminipath_hip.so (kernel_table.h); the lane mapping and the arithmetic contract
// are described in kernels.hip.
#include <algorithm>

#include "packet_walk.h"
#include "render_state.h"
#include "path_shading.h"

namespace mp {
namespace {

// ---- staged ("wavefront") evaluation of the path extension: MP_FLAG_WAVEFRONT --------------------------------------
// The north star's formulation, kept beside the fused render_paths_kernel: the paths of a batch (a few tiles x a chunk of
// samples, ~2 M paths) live in HBM as SoA streams (RNG state, ray, throughput, radiance, hit); per segment: a vertex kernel
// (shade + bounce, one thread per path), a counting sort of the live paths by (tile, direction bin) = stream compaction, and a
// trace kernel over the sorted stream.  Per-path RNG stream and operations are those of the fused kernel (path_vertex), every
// ray's result is independent of its neighbours, and the per-pixel sum is taken in sample order at the end: the frame is
// bit-identical to the fused kernel's and the oracle's (the two pipelines cross-check each other in the tests).  Measured slower
// than the fused kernel, which therefore stays the default.
constexpr uint32_t kDirBins = 512;  // 8 octants x 8 x 8 cells of the octahedral map of |d|

struct WfState {
    uint64_t* rng;       // 4 rows x n
    float* ray;          // 6 rows x n : origin, unit direction
    float* thr;          // nchan rows x n (nchan = 3 for a coloured / textured material table, else 1)
    float* L;            // nchan rows x n
    float* hit_t;        // n
    uint32_t* hit_prim;  // n
    float* hit_u;        // n
    float* hit_v;        // n
    uint32_t* hit_inst;  // n : member of the object group that was hit (groups only; otherwise unused)
    uint32_t* flags;     // n : kWfAlive | kWfPrimaryHit | kWfValid
    uint32_t* key;       // n : sort key of a live path
    uint32_t* idx;       // n : live paths in key order
    uint32_t* hist;      // nbins + 1 : per-key counts of the segment being generated ; [nbins] unused
    uint32_t* offs;      // nbins + 1 : exclusive scan of hist ; [nbins] = number of live paths
    uint32_t* cursor;    // nbins
    uint32_t n, nbins, nchan;
};
constexpr uint32_t kWfAlive = 1u, kWfPrimaryHit = 2u, kWfValid = 4u;

struct WfParams {
    DevScene scene;
    RayGen gen;
    const mp_block* tiles;  // this batch's tiles (device)
    uint32_t n_tiles, tile_size;
    uint32_t tile_base;     // index of the batch's first tile in the caller's tile list (output slot)
    uint32_t s0, sc, s_end; // the chunk covers samples [s0, min(s0 + sc, s_end))
    uint32_t depth, max_depth;
    float* out;
    float inv_spp;
    uint32_t carry_in, finalize, chunked;
    uint32_t lds_per_wave;
    unsigned long long* segments;
    WfState st;
};

__device__ __forceinline__ uint32_t direction_bin(float dx, float dy, float dz) {
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const float inv = __builtin_amdgcn_rcpf(ax + ay + az);  // approximate: the bin only steers the sort
    const uint32_t qx = min(7u, static_cast<uint32_t>(ax * inv * 8.0f)), qy = min(7u, static_cast<uint32_t>(ay * inv * 8.0f));
    const uint32_t oct = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    return oct * 64u + qx * 8u + qy;
}

// path p = (tile_local * ts*ts + (y - min_y) * ts + (x - min_x)) * sc + (s - s0)
// Stage 1: camera rays, generated and walked as packets of 2x2 pixels x 16 samples like render_tiles_packet_kernel.
template <bool LDS_STACK, bool OBJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8))) void wf_camera_kernel(WfParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const __attribute__((address_space(4))) WfParams* kwf_t;
    kwf_t KP = (kwf_t)__builtin_amdgcn_kernarg_segment_ptr();  // WfParams through short-lived views (see params_view)
    const WfParams& P0 = kernarg_view<WfParams>(KP);
    constexpr int S = 16, BW = 2, BH = 2;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int pix = lane / S, sub = lane % S;
    const uint32_t ts = P0.tile_size, bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P0.n_tiles * upt;
    const uint32_t n = P0.st.n;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    unsigned long long segs = 0;  // camera segments of this wave (wave-uniform)
    for (uint32_t unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); unit < total; unit += n_waves) {
        const WfParams& Pu = kernarg_view<WfParams>(KP);
        const uint32_t tile_l = unit / upt, b = unit % upt;
        const mp_block T = Pu.tiles[tile_l];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        const uint32_t pbase = ((tile_l * ts + (py - T.min_y)) * ts + (px - T.min_x)) * Pu.sc;
        const uint32_t sc_ = Pu.sc;
        for (uint32_t sl0 = 0; sl0 < sc_; sl0 += S) {
            const WfParams& P = kernarg_view<WfParams>(KP);  // one view per pass
            const uint32_t sl = sl0 + static_cast<uint32_t>(sub), s = P.s0 + sl;
            const bool slot = inpix && sl < P.sc;       // a path slot of the batch exists for this lane
            const bool act = slot && s < P.s_end;       // ... and holds a sample of this launch
            Rng rng;
            rng_zero(rng);
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            if (act) {
                rng_seed(rng, sample_key(P.gen, px, py, s));
                sample_ray_rng(P.gen, px, py, rng, r);
            }
            segs += static_cast<unsigned long long>(__popcll(__ballot(act)));
            PacketHit h;
            h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
            uint32_t hinst = 0u;
            float* lds = reinterpret_cast<float*>(smem + static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * P.lds_per_wave);
            if (OBJ) {  // object group: one packet walk per member
                if (LDS_STACK) {
                    HybridStack st(lds, lane, P.scene.stack_cap, P.scene.packet_stack_regs);
                    trace_packet_objects<false>(P.scene, r, act, st, h, hinst);
                } else {
                    RegStack st(lds, lane);
                    trace_packet_objects<true>(P.scene, r, act, st, h, hinst);
                }
            } else {
                const bool go = act && may_hit_scene(P.scene, r);
                if (__ballot(go) != 0) {
                    if (LDS_STACK) {
                        HybridStack st(lds, lane, P.scene.stack_cap, P.scene.packet_stack_regs);
                        trace_packet<false>(P.scene, r, go, st, h);
                    } else {
                        RegStack st(lds, lane);
                        trace_packet<true>(P.scene, r, go, st, h);
                    }
                }
            }
            if (slot) {
                const uint32_t p = pbase + sl;
                P.st.flags[p] = act ? (kWfAlive | kWfValid) : 0u;
                if (act) {
                    P.st.rng[0 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s0); P.st.rng[1 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s1);
                    P.st.rng[2 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s2); P.st.rng[3 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s3);
                    P.st.ray[0 * static_cast<size_t>(n) + p] = r.ox; P.st.ray[1 * static_cast<size_t>(n) + p] = r.oy;
                    P.st.ray[2 * static_cast<size_t>(n) + p] = r.oz; P.st.ray[3 * static_cast<size_t>(n) + p] = r.dx;
                    P.st.ray[4 * static_cast<size_t>(n) + p] = r.dy; P.st.ray[5 * static_cast<size_t>(n) + p] = r.dz;
                    for (uint32_t c = 0; c < P.st.nchan; c++) {
                        P.st.thr[c * static_cast<size_t>(n) + p] = 1.0f;
                        P.st.L[c * static_cast<size_t>(n) + p] = 0.0f;
                    }
                    P.st.hit_t[p] = h.t; P.st.hit_prim[p] = h.prim; P.st.hit_u[p] = h.u; P.st.hit_v[p] = h.v;
                    if (OBJ) P.st.hit_inst[p] = hinst;
                }
            }
        }
    }
    if (lane == 0 && P0.segments && segs) atomicAdd(P0.segments, segs);
}

// Stage 2: one thread per path: shade the hit of segment P.depth, draw the bounce ray, count it under its sort key.
template <int N, bool OBJ>
__global__ __launch_bounds__(256) void wf_vertex_kernel(WfParams P) {
    const uint32_t n = P.st.n;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t fl = P.st.flags[p];
        if (!(fl & kWfAlive)) continue;
        Rng rng;
        rng.s0 = rm::u64_split(P.st.rng[0 * static_cast<size_t>(n) + p]); rng.s1 = rm::u64_split(P.st.rng[1 * static_cast<size_t>(n) + p]);
        rng.s2 = rm::u64_split(P.st.rng[2 * static_cast<size_t>(n) + p]); rng.s3 = rm::u64_split(P.st.rng[3 * static_cast<size_t>(n) + p]);
        Ray r;
        r.ox = P.st.ray[0 * static_cast<size_t>(n) + p]; r.oy = P.st.ray[1 * static_cast<size_t>(n) + p];
        r.oz = P.st.ray[2 * static_cast<size_t>(n) + p]; r.dx = P.st.ray[3 * static_cast<size_t>(n) + p];
        r.dy = P.st.ray[4 * static_cast<size_t>(n) + p]; r.dz = P.st.ray[5 * static_cast<size_t>(n) + p];
        r.ix = r.iy = r.iz = 0.0f;  // not used by path_vertex
        PacketHit h;
        h.t = P.st.hit_t[p]; h.prim = P.st.hit_prim[p]; h.u = P.st.hit_u[p]; h.v = P.st.hit_v[p];
        float L[N], thr[N];
#pragma unroll
        for (int c = 0; c < N; c++) { L[c] = P.st.L[c * static_cast<size_t>(n) + p]; thr[c] = P.st.thr[c * static_cast<size_t>(n) + p]; }
        bool primary = (fl & kWfPrimaryHit) != 0u;
        const bool alive = path_vertex<OBJ, N>(P.scene, h, P.depth, P.max_depth, rng, r, L, thr, primary, OBJ ? P.st.hit_inst[p] : 0u);
        fl = (fl & ~(kWfAlive | kWfPrimaryHit)) | (alive ? kWfAlive : 0u) | (primary ? kWfPrimaryHit : 0u);
        P.st.flags[p] = fl;
#pragma unroll
        for (int c = 0; c < N; c++) { P.st.L[c * static_cast<size_t>(n) + p] = L[c]; P.st.thr[c * static_cast<size_t>(n) + p] = thr[c]; }
        if (alive) {
            P.st.rng[0 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s0); P.st.rng[1 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s1);
            P.st.rng[2 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s2); P.st.rng[3 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s3);
            P.st.ray[0 * static_cast<size_t>(n) + p] = r.ox; P.st.ray[1 * static_cast<size_t>(n) + p] = r.oy;
            P.st.ray[2 * static_cast<size_t>(n) + p] = r.oz; P.st.ray[3 * static_cast<size_t>(n) + p] = r.dx;
            P.st.ray[4 * static_cast<size_t>(n) + p] = r.dy; P.st.ray[5 * static_cast<size_t>(n) + p] = r.dz;
            const uint32_t tile_l = p / (P.tile_size * P.tile_size * P.sc);
            const uint32_t k = tile_l * kDirBins + direction_bin(r.dx, r.dy, r.dz);
            P.st.key[p] = k;
            atomicAdd(P.st.hist + k, 1u);
        }
    }
}

// Stage 3: exclusive scan of the key histogram (one workgroup), cursors and histogram reset for the next segment, and the
// number of live paths = ray segments of the next stage.
__global__ __launch_bounds__(1024) void wf_scan_kernel(WfParams P) {
    __shared__ uint32_t part[1024];
    const uint32_t nb = P.st.nbins, per = (nb + 1023u) / 1024u, t = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t i = t * per; i < min(nb, (t + 1u) * per); i++) sum += P.st.hist[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t i = t * per; i < min(nb, (t + 1u) * per); i++) {
        const uint32_t c = P.st.hist[i];
        P.st.offs[i] = run;
        P.st.cursor[i] = 0u;
        P.st.hist[i] = 0u;
        run += c;
    }
    if (t == 1023u) {
        P.st.offs[nb] = part[1023];
        if (P.segments) atomicAdd(P.segments, static_cast<unsigned long long>(part[1023]));
    }
}

// Stage 4: scatter the live paths to their key's range (order inside a key is arbitrary: results do not depend on it).
__global__ __launch_bounds__(256) void wf_scatter_kernel(WfParams P) {
    const uint32_t n = P.st.n;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        if (!(P.st.flags[p] & kWfAlive)) continue;
        const uint32_t k = P.st.key[p];
        P.st.idx[P.st.offs[k] + atomicAdd(P.st.cursor + k, 1u)] = p;
    }
}

// Stage 5: the sorted rays through the 8-lane-group traversal, 64 per wave.  (Walking 64 sorted rays as ONE packet was measured
// too: diffuse bounce rays do not share enough of the tree even when sorted -- 2 586 VALU per ray against ~500 here; see
// profiles/r01_notes.md.)  The sort serves cache locality.
template <bool OBJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void wf_trace_groups_kernel(WfParams P) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * P.lds_per_wave);
    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
    const uint32_t n = P.st.n, live = P.st.offs[P.st.nbins];
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6), chunks = (live + 63u) / 64u;
    for (uint32_t c = blockIdx.x * (blockDim.x >> 6) + static_cast<uint32_t>(wave); c < chunks; c += n_waves) {
        const uint32_t slot = c * 64u + static_cast<uint32_t>(lane);
        const bool act = slot < live;
        const uint32_t p = act ? P.st.idx[slot] : 0u;
        Ray r;
        r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
        if (act) {
            r.ox = P.st.ray[0 * static_cast<size_t>(n) + p]; r.oy = P.st.ray[1 * static_cast<size_t>(n) + p];
            r.oz = P.st.ray[2 * static_cast<size_t>(n) + p]; r.dx = P.st.ray[3 * static_cast<size_t>(n) + p];
            r.dy = P.st.ray[4 * static_cast<size_t>(n) + p]; r.dz = P.st.ray[5 * static_cast<size_t>(n) + p];
            r.ix = (r.dx == 0.0f) ? INFINITY : 1.0f / r.dx;
            r.iy = (r.dy == 0.0f) ? INFINITY : 1.0f / r.dy;
            r.iz = (r.dz == 0.0f) ? INFINITY : 1.0f / r.dz;
        }
        // compaction of the rays that can reach the object into the wave's queue + the 8-lane-group walk (once per member of an
        // object group, closest wins)
        GroupHit gh;
        trace_objects<OBJ>(P.scene, r, act, q, stack, gh);
        if (act) {
            P.st.hit_t[p] = gh.t;
            P.st.hit_prim[p] = gh.prim;
            P.st.hit_u[p] = gh.u;
            P.st.hit_v[p] = gh.v;
            if (OBJ) P.st.hit_inst[p] = gh.inst;
        }
    }
}

// Stage 6: pixel_sum += sample in sample order (worker.rs:41-43), one thread per pixel of the batch.
__global__ __launch_bounds__(256) void wf_accumulate_kernel(WfParams P) {
    const uint32_t ts = P.tile_size, npx = P.n_tiles * ts * ts;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        const uint32_t tile_l = i / (ts * ts), q = i % (ts * ts), x = q % ts, y = q / ts;
        const mp_block T = P.tiles[tile_l];
        if (!(T.min_x + x < T.max_x && T.min_y + y < T.max_y)) continue;
        float* o = P.out + (static_cast<size_t>(P.tile_base + tile_l) * ts * ts + q) * 4;
        if (P.st.nchan == 3u) {  // coloured / textured material table: slot = {sum r, sum g, sum b, hit count}; never chunked
            float a3[3] = {0.0f, 0.0f, 0.0f}, c3 = 0.0f;
            if (P.carry_in) {
                const float4 prev = *reinterpret_cast<const float4*>(o);
                a3[0] = prev.x; a3[1] = prev.y; a3[2] = prev.z; c3 = prev.w;
            }
            const uint32_t ns3 = min(P.sc, P.s_end - P.s0);
            const uint32_t pb3 = i * P.sc;
            for (uint32_t sl = 0; sl < ns3; sl++) {
                for (uint32_t c = 0; c < 3u; c++) a3[c] += P.st.L[c * static_cast<size_t>(P.st.n) + pb3 + sl];
                c3 += (P.st.flags[pb3 + sl] & kWfPrimaryHit) ? 1.0f : 0.0f;
            }
            const float sc3 = P.finalize ? P.inv_spp : 1.0f;
            *reinterpret_cast<float4*>(o) = make_float4(a3[0] * sc3, a3[1] * sc3, a3[2] * sc3, c3 * sc3);
            continue;
        }
        float acc = 0.0f, cnt = 0.0f;
        double tot = 0.0;  // MP_FLAG_CHUNKED_SUM: slot = {chunk sum, hit count, f64 total} (pixel_state_load)
        if (P.carry_in) {
            const float4 prev = *reinterpret_cast<const float4*>(o);
            acc = prev.x;
            cnt = P.chunked ? prev.y : prev.w;
            if (P.chunked) tot = *reinterpret_cast<const double*>(o + 2);
        }
        const uint32_t ns = min(P.sc, P.s_end - P.s0);
        const uint32_t pbase = i * P.sc;
        for (uint32_t sl = 0; sl < ns; sl++) {
            acc += P.st.L[pbase + sl];
            cnt += (P.st.flags[pbase + sl] & kWfPrimaryHit) ? 1.0f : 0.0f;
            if (P.chunked && ((P.s0 + sl + 1u) & (kSumChunk - 1u)) == 0u) { tot = tot + static_cast<double>(acc); acc = 0.0f; }
        }
        if (P.chunked) {
            if (!P.finalize) {
                *reinterpret_cast<float2*>(o) = make_float2(acc, cnt);
                *reinterpret_cast<double*>(o + 2) = tot;
                continue;
            }
            if (((P.s0 + ns) & (kSumChunk - 1u)) != 0u) tot = tot + static_cast<double>(acc);
            const double inv = 1.0 / static_cast<double>(P.gen.spp);
            const float m = static_cast<float>(tot * inv), a = static_cast<float>(static_cast<double>(cnt) * inv);
            *reinterpret_cast<float4*>(o) = make_float4(m, m, m, a);
            continue;
        }
        const float m = P.finalize ? acc * P.inv_spp : acc, a = P.finalize ? cnt * P.inv_spp : cnt;
        *reinterpret_cast<float4*>(o) = make_float4(m, m, m, a);
    }
}

static_assert(kPlanDirBins == kDirBins, "launch_plan.h sizes the launches with the device code's constants");

MP_FAMILY_LAUNCHER(MP_KERNELS_STAGED)

}  // namespace

// launch_render_paths_wavefront: `plan` is plan_render_paths_wavefront(L), not refused
int launch_staged(const RenderLaunch& L, const WavefrontPlan& plan, hipStream_t st, std::string& err) {
    WfParams P;
    fill_common(P, L);
    P.lds_per_wave = plan.cam_lds_per_wave;
    P.st.nchan = plan.nchan;
    const size_t n64 = plan.n64, bin_bytes = (static_cast<size_t>(plan.nbins) + 64) * 4;
    unsigned char* ws = nullptr;
    int rc = check(hipMallocAsync(reinterpret_cast<void**>(&ws), plan.ws_bytes, st), "hipMallocAsync(path state)", err);
    if (rc) return rc;
    unsigned char* w = ws;
    auto take = [&](size_t b) { unsigned char* r = w; w += b; return r; };
    P.st.rng = reinterpret_cast<uint64_t*>(take(n64 * 32));
    P.st.ray = reinterpret_cast<float*>(take(n64 * 24));
    P.st.thr = reinterpret_cast<float*>(take(n64 * 4 * plan.nchan));
    P.st.L = reinterpret_cast<float*>(take(n64 * 4 * plan.nchan));
    P.st.hit_t = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_prim = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.hit_u = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_v = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_inst = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.flags = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.key = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.idx = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.hist = reinterpret_cast<uint32_t*>(take(bin_bytes));
    P.st.offs = reinterpret_cast<uint32_t*>(take(bin_bytes));
    P.st.cursor = reinterpret_cast<uint32_t*>(take(bin_bytes));
    for (uint32_t tile_base = 0; tile_base < L.n_tiles && !rc; tile_base += plan.tb) {
        const uint32_t ntb = std::min(plan.tb, L.n_tiles - tile_base);
        const WavefrontBatch B = plan.batch(ntb);
        P.tiles = L.d_tiles + tile_base;
        P.n_tiles = ntb;
        P.tile_base = tile_base;
        for (uint32_t s0 = L.pass_begin; s0 < L.pass_end && !rc; s0 += plan.sc) {
            P.s0 = s0;
            P.sc = plan.sc;
            P.s_end = L.pass_end;
            P.st.n = B.n;
            P.st.nbins = B.nbins;
            P.carry_in = (L.carry_in || s0 > L.pass_begin) ? 1u : 0u;
            P.finalize = (L.finalize && s0 + plan.sc >= L.pass_end) ? 1u : 0u;
            rc = check(hipMemsetAsync(P.st.hist, 0, (static_cast<size_t>(P.st.nbins) + 1) * 4, st), "hipMemsetAsync(histogram)", err);
            if (rc) break;
            // path slots of pixels outside a clipped tile are never written by the camera stage: they must read as dead
            rc = check(hipMemsetAsync(P.st.flags, 0, static_cast<size_t>(P.st.n) * 4, st), "hipMemsetAsync(path flags)", err);
            if (rc) break;
            rc = launch(plan.camera, B.cam_grid, 256, plan.cam_lds, st, err, P);
            WfParams G = P;  // bounce stage: LDS ray queue + eight traversal stacks per wave
            G.lds_per_wave = plan.trace_lds_per_wave;
            for (uint32_t depth = 1; depth <= L.max_depth && !rc; depth++) {
                P.depth = depth;
                rc = launch(plan.vertex, B.flat_grid, 256, 0, st, err, P);
                if (rc || depth == L.max_depth) break;
                rc = launch(K_WF_SCAN, 1, 1024, 0, st, err, P);
                if (!rc) rc = launch(K_WF_SCATTER, B.flat_grid, 256, 0, st, err, P);
                if (!rc) rc = launch(plan.trace, plan.trace_grid, 256, plan.trace_lds, st, err, G);
            }
            if (!rc) rc = launch(K_WF_ACCUMULATE, B.px_grid, 256, 0, st, err, P);
        }
    }
    (void)hipFreeAsync(ws, st);
    return rc;
}

}  // namespace mp
