// Host check of the scene and context ownership behind the C ABI, a program of its own (nothing of it is loaded into Python):
//   make -C minipath_amd/csrc host_ownership_check && minipath_amd/csrc/host_ownership_check
// prints "host_ownership_check: ok" and exits 0, or names the first line that does not hold.  It is compiled with
// -fsanitize=address,undefined and linked from the objects of libminipath_hip_asan.so, leak detection on: two host-only scenes
// (ctx = NULL), a group and an instance set of them, materials on a member and on the group, the members destroyed before the groups that
// still borrow from them, then the groups.  It ends with mp_ctx_create, which without a GPU must come back with an error status
// and nothing held; with one, the context is destroyed again.
#include <cstdio>
#include <cstring>

#include "../include/minipath_hip.h"

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("host_ownership_check: line %d: %s (%s)\n", __LINE__, #cond, mp_last_error()); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

// a strip of 2 * quads triangles, material id = triangle index % materials
static int strip(uint32_t quads, uint32_t materials, float y, mp_scene** out) {
    float pos[64 * 2 * 3];
    uint32_t tri[63 * 2 * 3], mat[63 * 2];
    for (uint32_t i = 0; i <= quads; i++)
        for (uint32_t k = 0; k < 2; k++) {
            float* p = &pos[(i * 2 + k) * 3];
            p[0] = static_cast<float>(i), p[1] = y + 0.25f * static_cast<float>(i & 1u), p[2] = static_cast<float>(k);
        }
    for (uint32_t i = 0; i < quads; i++) {
        const uint32_t a = i * 2, t[6] = {a, a + 1, a + 2, a + 1, a + 3, a + 2};
        std::memcpy(&tri[i * 6], t, sizeof(t));
        mat[i * 2] = (i * 2) % materials, mat[i * 2 + 1] = (i * 2 + 1) % materials;
    }
    return mp_scene_from_triangles_mat(nullptr, pos, nullptr, nullptr, (quads + 1) * 2, tri, mat, quads * 2, out);
}

int main() {
    mp_scene *a = nullptr, *b = nullptr, *group = nullptr, *inst = nullptr;
    EXPECT(strip(63, 3, 0.0f, &a) == MP_OK && a);
    EXPECT(strip(20, 1, 2.0f, &b) == MP_OK && b);
    mp_scene_info info;
    EXPECT(mp_scene_info_get(a, &info) == MP_OK && info.triangle_count == 126 && info.material_count == 3 && info.device_bytes == 0);

    const mp_scene* members[2] = {a, b};
    const float t[3 * 3] = {0, 0, 0, 5, 0, 0, 0, 5, 0}, q[2 * 4] = {0, 0, 0, 1, 0, 0.70710678f, 0, 0.70710678f};
    EXPECT(mp_scene_group(nullptr, members, q, t, 2, &group) == MP_OK && group);
    EXPECT(mp_scene_instances(nullptr, b, t, 3, &inst) == MP_OK && inst);
    EXPECT(mp_scene_group(nullptr, &group, nullptr, t, 1, &inst) == MP_ERR_UNSUPPORTED);  // no groups of groups; inst untouched

    mp_material table[4];
    std::memset(table, 0, sizeof(table));
    for (int i = 0; i < 4; i++) table[i].albedo[0] = table[i].albedo[1] = table[i].albedo[2] = 0.25f * static_cast<float>(i);
    EXPECT(mp_scene_set_materials(a, table, 4, 0.5f) == MP_OK);
    table[1].albedo[0] = 0.9f;  // a coloured table for the group
    EXPECT(mp_scene_set_materials(group, table, 3, 0.75f) == MP_OK);
    EXPECT(mp_scene_set_materials(a, table, 2, 0.5f) == MP_ERR_INVALID);  // shorter than material_count: the scene keeps its table
    table[0].texture = 7u;
    EXPECT(mp_scene_set_materials(group, table, 3, 0.75f) == MP_ERR_INVALID);

    // the members' handles go first: the groups hold a reference on each and still answer for them
    mp_scene_destroy(a);
    mp_scene_destroy(b);
    EXPECT(mp_scene_info_get(group, &info) == MP_OK && info.triangle_count == 126 + 40 && info.material_count == 3);
    EXPECT(mp_scene_info_get(inst, &info) == MP_OK && info.triangle_count == 40);
    mp_scene_destroy(group);
    mp_scene_destroy(inst);
    mp_scene_destroy(nullptr);

    mp_ctx* ctx = nullptr;
    const int rc = mp_ctx_create(0, &ctx);
    EXPECT((rc == MP_OK) == (ctx != nullptr));
    EXPECT(rc == MP_OK || mp_last_error()[0] != 0);
    mp_ctx_destroy(ctx);
    std::printf("host_ownership_check: mp_ctx_create returned %d\n", rc);
    std::printf("host_ownership_check: ok\n");
    return 0;
}
