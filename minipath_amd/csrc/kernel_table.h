// Every kernel instantiation libminipath_hip.so can launch, written down once, as one sub-table per kernel family.  The list
// generates the ids the launch plans (launch_plan.h) return, the names mp_ctx_last_kernels reports -- the kernel with its template
// arguments as the row writes them -- and the switch that records the name and launches (family_launch.h), which every translation
// unit expands over the sub-table of its own family (the unit's name stands above each).  No HIP header: the planning source
// includes it too.
//
// A row is X(id, kernel).  MP_KERNEL_TABLE is the sub-tables in the order the ids have always had.  Templates stand in the order the
// launchers have always named them: the compiler emits device code in the order of first use, so moving a row moves its kernel
// inside its unit's code object (and nothing in any other unit's).
#pragma once

#ifndef MP_MCACHE_WPE
#define MP_MCACHE_WPE 8  // waves per SIMD of the cached packet kernel; a variant build may give another (tools/build_variant.sh)
#endif

// clang-format off
// kernels_paths.hip
#define MP_KERNELS_PATHS(X)                                                                         \
    /* path extension: pooled <NSUB>, then <S, OBJ, RGB[, MCACHE]> */                               \
    X(K_PATHS_POOLED_4,        render_paths_pooled_kernel<4>)                                       \
    X(K_PATHS_POOLED_2,        render_paths_pooled_kernel<2>)                                       \
    X(K_PATHS_8_RGB_CACHED,    render_paths_kernel<8, false, true, true>)                           \
    X(K_PATHS_8_GREY_CACHED,   render_paths_kernel<8, false, false, true>)                          \
    X(K_PATHS_8_OBJ_RGB,       render_paths_kernel<8, true, true>)                                  \
    X(K_PATHS_8_OBJ_GREY,      render_paths_kernel<8, true, false>)                                 \
    X(K_PATHS_8_RGB,           render_paths_kernel<8, false, true>)                                 \
    X(K_PATHS_8_GREY,          render_paths_kernel<8, false, false>)                                \
    X(K_PATHS_4_OBJ_RGB,       render_paths_kernel<4, true, true>)                                  \
    X(K_PATHS_4_OBJ_GREY,      render_paths_kernel<4, true, false>)                                 \
    X(K_PATHS_4_RGB,           render_paths_kernel<4, false, true>)                                 \
    X(K_PATHS_4_GREY,          render_paths_kernel<4, false, false>)                                \
    X(K_PATHS_2_OBJ_RGB,       render_paths_kernel<2, true, true>)                                  \
    X(K_PATHS_2_OBJ_GREY,      render_paths_kernel<2, true, false>)                                 \
    X(K_PATHS_2_RGB,           render_paths_kernel<2, false, true>)                                 \
    X(K_PATHS_2_GREY,          render_paths_kernel<2, false, false>)                                \
    X(K_PATHS_1_OBJ_RGB,       render_paths_kernel<1, true, true>)                                  \
    X(K_PATHS_1_OBJ_GREY,      render_paths_kernel<1, true, false>)                                 \
    X(K_PATHS_1_RGB,           render_paths_kernel<1, false, true>)                                 \
    X(K_PATHS_1_GREY,          render_paths_kernel<1, false, false>)

// kernels_tiles.hip
#define MP_KERNELS_TILES(X)                                                                         \
    /* 8-lane groups <S, OBJ>, two rays per lane <W> */                                             \
    X(K_GROUPS_OBJ,            render_tiles_kernel<1, true>)                                        \
    X(K_GROUPS,                render_tiles_kernel<1, false>)                                       \
    X(K_PACKET2,               render_tiles_packet2_kernel<6>)                                      \
    /* packets <S, LDS_STACK, W[, OBJ[, MCACHE]]>: cached, object group, then by samples in flight */ \
    X(K_PACKET_32_CACHED,      render_tiles_packet_kernel<32, false, MP_MCACHE_WPE, false, true>)   \
    X(K_PACKET_8_CACHED,       render_tiles_packet_kernel<8, false, MP_MCACHE_WPE, false, true>)    \
    X(K_PACKET_4_CACHED,       render_tiles_packet_kernel<4, false, MP_MCACHE_WPE, false, true>)    \
    X(K_PACKET_16_CACHED,      render_tiles_packet_kernel<16, false, MP_MCACHE_WPE, false, true>)   \
    X(K_PACKET_16_OBJ_LDS,     render_tiles_packet_kernel<16, true, 6, true>)                       \
    X(K_PACKET_16_OBJ,         render_tiles_packet_kernel<16, false, 6, true>)                      \
    X(K_PACKET_1_OBJ_LDS,      render_tiles_packet_kernel<1, true, 6, true>)                        \
    X(K_PACKET_1_OBJ,          render_tiles_packet_kernel<1, false, 6, true>)                       \
    X(K_PACKET_64_LDS,         render_tiles_packet_kernel<64, true, 7>)                             \
    X(K_PACKET_64,             render_tiles_packet_kernel<64, false, 7>)                            \
    X(K_PACKET_32_BIG_LDS,     render_tiles_packet_kernel<32, true, 8>)                             \
    X(K_PACKET_32_BIG,         render_tiles_packet_kernel<32, false, 8>)                            \
    X(K_PACKET_32_LDS,         render_tiles_packet_kernel<32, true, 7>)                             \
    X(K_PACKET_32,             render_tiles_packet_kernel<32, false, 7>)                            \
    X(K_PACKET_16_BIG_LDS,     render_tiles_packet_kernel<16, true, 8>)                             \
    X(K_PACKET_16_BIG,         render_tiles_packet_kernel<16, false, 8>)                            \
    X(K_PACKET_16_LDS,         render_tiles_packet_kernel<16, true, 7>)                             \
    X(K_PACKET_16,             render_tiles_packet_kernel<16, false, 7>)                            \
    X(K_PACKET_8_LDS,          render_tiles_packet_kernel<8, true, 7>)                              \
    X(K_PACKET_8,              render_tiles_packet_kernel<8, false, 7>)                             \
    X(K_PACKET_4_LDS,          render_tiles_packet_kernel<4, true, 7>)                              \
    X(K_PACKET_4,              render_tiles_packet_kernel<4, false, 7>)                             \
    X(K_PACKET_2_LDS,          render_tiles_packet_kernel<2, true, 7>)                              \
    X(K_PACKET_2,              render_tiles_packet_kernel<2, false, 7>)                             \
    X(K_PACKET_1_LDS,          render_tiles_packet_kernel<1, true, 7>)                              \
    X(K_PACKET_1,              render_tiles_packet_kernel<1, false, 7>)                             \
    /* (end of the fused tiles) */

// kernels_aov.hip
#define MP_KERNELS_AOV(X)                                                                           \
    /* feature planes <S, LDS_STACK, W[, OBJ[, MCACHE]]> */                                         \
    X(K_AOV_16_CACHED,         render_aov_packet_kernel<16, false, 8, false, true>)                 \
    X(K_AOV_4_CACHED,          render_aov_packet_kernel<4, false, 8, false, true>)                  \
    X(K_AOV_16_OBJ_LDS,        render_aov_packet_kernel<16, true, 6, true>)                         \
    X(K_AOV_16_OBJ,            render_aov_packet_kernel<16, false, 6, true>)                        \
    X(K_AOV_1_OBJ_LDS,         render_aov_packet_kernel<1, true, 6, true>)                          \
    X(K_AOV_1_OBJ,             render_aov_packet_kernel<1, false, 6, true>)                         \
    X(K_AOV_16_LDS,            render_aov_packet_kernel<16, true, 8>)                               \
    X(K_AOV_1_LDS,             render_aov_packet_kernel<1, true, 8>)                                \
    X(K_AOV_16,                render_aov_packet_kernel<16, false, 8>)                              \
    X(K_AOV_4,                 render_aov_packet_kernel<4, false, 8>)                               \
    X(K_AOV_1,                 render_aov_packet_kernel<1, false, 8>)

// kernels_staged.hip
#define MP_KERNELS_STAGED(X)                                                                        \
    /* staged path evaluation: camera <LDS_STACK, OBJ>, vertex <NCHAN, OBJ>, trace <OBJ> */         \
    X(K_WF_CAMERA_LDS_OBJ,     wf_camera_kernel<true, true>)                                        \
    X(K_WF_CAMERA_OBJ,         wf_camera_kernel<false, true>)                                       \
    X(K_WF_CAMERA_LDS,         wf_camera_kernel<true, false>)                                       \
    X(K_WF_CAMERA,             wf_camera_kernel<false, false>)                                      \
    X(K_WF_VERTEX_RGB_OBJ,     wf_vertex_kernel<3, true>)                                           \
    X(K_WF_VERTEX_RGB,         wf_vertex_kernel<3, false>)                                          \
    X(K_WF_VERTEX_OBJ,         wf_vertex_kernel<1, true>)                                           \
    X(K_WF_VERTEX,             wf_vertex_kernel<1, false>)                                          \
    X(K_WF_SCAN,               wf_scan_kernel)                                                      \
    X(K_WF_SCATTER,            wf_scatter_kernel)                                                   \
    X(K_WF_TRACE_OBJ,          wf_trace_groups_kernel<true>)                                        \
    X(K_WF_TRACE,              wf_trace_groups_kernel<false>)                                       \
    X(K_WF_ACCUMULATE,         wf_accumulate_kernel)

// kernels_queries.hip
#define MP_KERNELS_QUERIES(X)                                                                       \
    /* ray queries <OBJ[, MODE]> */                                                                 \
    X(K_TRACE_OBJ,             trace_rays_kernel<true>)                                             \
    X(K_TRACE,                 trace_rays_kernel<false>)                                            \
    X(K_QUERY_ANY_OBJ,         query_rays_kernel<true, kAnyHit>)                                    \
    X(K_QUERY_ANY,             query_rays_kernel<false, kAnyHit>)                                   \
    X(K_QUERY_BOUNDED_OBJ,     query_rays_kernel<true, kBounded>)                                   \
    X(K_QUERY_BOUNDED,         query_rays_kernel<false, kBounded>)

// kernels.hip
#define MP_KERNELS_UTILITIES(X)                                                                     \
    /* utilities */                                                                                 \
    X(K_SET_U64,               set_u64_kernel)                                                      \
    X(K_GENERATE_RAYS,         generate_rays_kernel)                                                \
    X(K_UNTILE,                untile_kernel)                                                       \
    X(K_QUANTISE,              quantise_kernel)

#define MP_KERNEL_TABLE(X) \
    MP_KERNELS_PATHS(X) MP_KERNELS_TILES(X) MP_KERNELS_AOV(X) MP_KERNELS_STAGED(X) MP_KERNELS_QUERIES(X) MP_KERNELS_UTILITIES(X)
// clang-format on

namespace mp {

enum KernelId : int {
#define MP_X(id, ...) id,
    MP_KERNEL_TABLE(MP_X)
#undef MP_X
    K_COUNT
};

}  // namespace mp
