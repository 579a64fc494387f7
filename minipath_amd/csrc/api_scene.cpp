// C ABI (include/minipath_hip.h): scenes -- upload of a built tree, the from_* constructors, object groups, materials, info,
// export and the device tree.
#include <cmath>

#include "api_common.h"

using namespace mp;

namespace {

constexpr float kInvU16Max = 1.0f / 65535.0f;
inline float dequantise(uint16_t q, float size, float mn) {  // compressed_geometry.rs:48-51,95-110
    return std::fmaf(size, static_cast<float>(static_cast<int32_t>(q)) * kInvU16Max, mn);
}

// a table of grey (r = g = b), untextured materials runs the one-channel kernels (bit-identical to the three-channel ones)
bool table_is_grey(const std::vector<mp_material>& t) {
    for (const mp_material& m : t)
        if (m.texture != MP_TEXTURE_NONE || std::memcmp(&m.albedo[0], &m.albedo[1], 4) != 0 || std::memcmp(&m.albedo[0], &m.albedo[2], 4) != 0 ||
            std::memcmp(&m.emission[0], &m.emission[1], 4) != 0 || std::memcmp(&m.emission[0], &m.emission[2], 4) != 0)
            return false;
    return true;
}

// One array to the device: at least 16 bytes, zeroed, then the data.
int upload(DeviceBuffer& dst, const void* src, size_t bytes) {
    const size_t cap = std::max<size_t>(bytes, 16);
    MP_HIP(dst.grow(cap));
    MP_HIP(hipMemset(dst.get(), 0, cap));
    if (bytes) MP_HIP(hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice));
    return MP_OK;
}
template <class T> int upload(DeviceBuffer& dst, const std::vector<T>& v) { return upload(dst, v.data(), v.size() * sizeof(T)); }

int upload_scene(mp_scene* s) {
    const HostBvh& h = s->host;
    const size_t np = h.packets.size();
    std::vector<float> tris(np * kPacketDwords, 0.0f);
    std::vector<float> shade(np * 8 * 12, 0.0f);
    std::vector<uint32_t> vidx(np * 8 * 3, 0);
    for (size_t p = 0; p < np; p++) {
        const TriPacketRef& pk = h.packets[p];
        const Box3& e = h.packet_box[p];
        float size[3] = {e.mx[0] - e.mn[0], e.mx[1] - e.mn[1], e.mx[2] - e.mn[2]};
        float* o = &tris[p * kPacketDwords];
        for (int i = 0; i < 8; i++) {
            float v[3][3];
            for (int a = 0; a < 3; a++)
                for (int k = 0; k < 3; k++) v[a][k] = dequantise(pk.v[a][k][i], size[k], e.mn[k]);  // :160-162
            for (int k = 0; k < 3; k++) {
                o[k * 8 + i] = v[0][k];
                o[(3 + k) * 8 + i] = v[1][k] - v[0][k];  // e1, triangle.rs:195
                o[(6 + k) * 8 + i] = v[2][k] - v[0][k];  // e2, triangle.rs:196
            }
            const TriShadingRef& sh = h.shading[p * 8 + i];
            float* so = &shade[(p * 8 + i) * 12];
            for (int a = 0; a < 3; a++) {
                for (int k = 0; k < 3; k++) so[a * 3 + k] = h.vnormal[3 * static_cast<size_t>(sh.vi[a]) + k];
                vidx[(p * 8 + i) * 3 + a] = sh.vi[a];
            }
            uint32_t flat = sh.flat, mat = h.material.empty() ? 0u : h.material[p * 8 + i];
            std::memcpy(&so[9], &flat, 4);
            std::memcpy(&so[10], &mat, 4);
        }
    }
    // node arrays (device_tree.cpp): the wide tree the walks normally use and the literal reference tree for rays with an
    // infinite inverse direction component.  The sign-specialised slab test of the packet walk relies on min <= max for every
    // real child box of either.
    const std::vector<uint32_t> pkt_valid = packet_real_counts(h);
    DeviceTree wide, lit, pk;
    bool use_pk = false;
    {
        std::string err;
        int trc = build_device_tree(h, pkt_valid, true, wide, err);
        if (!trc) trc = build_device_tree(h, pkt_valid, false, lit, err);
        if (!trc && s->packet_tree_slots == 16u) {
            trc = build_device_tree(h, pkt_valid, true, pk, err, 16);
            use_pk = !trc && packet_tree_applies(pk, wide, lit, s->packet_tree_slots);
        }
        if (trc) return fail(trc, err);
    }
    // (the packet tree holds the wide tree's boxes -- the same floats -- in other slots)
    s->dev.boxes_ordered = (wide.boxes_ordered && lit.boxes_ordered && (!use_pk || pk.boxes_ordered)) ? 1u : 0u;
    s->wide_nodes = wide.count;
    s->absorbed_nodes = wide.absorbed;
    std::vector<float> tris_aos(np * 8 * kTriDwords + 4 * kTriDwords, 0.0f);  // + tail padding: the triangle loop prefetches up to two ahead
    for (size_t p = 0; p < np; p++)
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 9; k++) tris_aos[(p * 8 + i) * kTriDwords + k] = tris[p * kPacketDwords + k * 8 + i];
    // magnitude bound behind the packet walk's triangle masks (mask_cache.h, tri_may_hit; packet_walk.h, leaf_mask_slow): no overflow in the interval evaluation
    s->dev.tris_bounded = 1u;
    for (size_t i = 0; i < np * 8 && s->dev.tris_bounded; i++)
        for (int k = 0; k < 9; k++) {
            const float v = tris_aos[i * kTriDwords + k];
            if (!(std::fabs(v) <= (k < 3 ? 1073741824.0f : 2147483648.0f))) { s->dev.tris_bounded = 0u; break; }
        }
    auto up = [&](DeviceBuffer& dst, const auto& v) {  // allocate, zero, copy and count one array
        const int rc = upload(dst, v);
        s->device_bytes += dst.bytes();
        return rc;
    };
    int rc;
    if ((rc = up(s->shade, shade)) || (rc = up(s->vidx, vidx)) || (rc = up(s->vtex, h.vtex)) || (rc = up(s->nodes_aos, wide.nodes)) ||
        (rc = up(s->nodes_lit, lit.nodes)) || (use_pk && (rc = up(s->nodes_pk, pk.nodes))) || (rc = up(s->tris_aos, tris_aos)) ||
        (rc = up(s->pkt_valid, pkt_valid)))
        return rc;
    s->mat_table = std::make_shared<DeviceBuffer>();
    if ((rc = up(*s->mat_table, s->materials))) return rc;
    s->dev.materials = s->mat_table->as<const float>();
    s->dev.sky = s->sky;
    s->dev.shade = s->shade.as<const float>();
    s->dev.vidx = s->vidx.as<const uint32_t>();
    s->dev.vtex = s->vtex.as<const float>();
    s->dev.nodes_aos = s->nodes_aos.as<const float>();
    s->dev.nodes_lit = s->nodes_lit.as<const float>();
    // the cached packet walk's tree: the packet tree, or the wide tree again (same pointer, 8-bit masks)
    s->dev.nodes_pk = use_pk ? s->nodes_pk.as<const float>() : s->dev.nodes_aos;
    s->dev.pk_count = use_pk ? pk.count : wide.count;
    s->dev.pk_mask_bits = use_pk ? 16u : 8u;
    s->dev.tris_aos = s->tris_aos.as<const float>();
    s->dev.pkt_valid = s->pkt_valid.as<const uint32_t>();
    s->dev.root = wide.root;
    s->dev.root_lit = lit.root;
    s->dev.inner_count = wide.count;
    s->dev.packet_count = static_cast<uint32_t>(np);
    // exact bound of the traversal stack (device_tree.cpp), over both trees: the walks share their stack storage
    s->dev.stack_cap = std::max(wide.stack_bound, lit.stack_bound);
    // union of the literal root's child boxes (the wide root's slots lie inside it: absorbed children are FP-nested)
    s->dev.has_pre = 0;
    if ((h.root & 7u) == 0u && h.root != MP_LINK_NULL) {  // root is an inner node
        const float* o = &lit.nodes[static_cast<size_t>(h.root >> 3) * 64];
        bool any = false;
        for (int i = 0; i < 8; i++) {
            if (h.inner[h.root >> 3].link[i] == MP_LINK_NULL) continue;
            for (int k = 0; k < 3; k++) {
                float mn = o[i * 8 + k], mx = o[i * 8 + 3 + k];
                s->dev.pre_min[k] = any ? std::fmin(s->dev.pre_min[k], mn) : mn;
                s->dev.pre_max[k] = any ? std::fmax(s->dev.pre_max[k], mx) : mx;
            }
            any = true;
        }
        s->dev.has_pre = any ? 1u : 0u;
    }
    return MP_OK;
}

int finish_scene(mp_ctx* ctx, std::unique_ptr<mp_scene> s, mp_scene** out) {
    s->ctx = ctx;
    if (ctx) s->packet_tree_slots = ctx->packet_tree_slots.load();
    uint32_t mc = 0;
    for (uint32_t m : s->host.material) mc = std::max(mc, m);
    if (mc >= MP_MAX_MATERIALS) return fail(MP_ERR_INVALID, "material id out of range (MP_MAX_MATERIALS)");  // build_bvh / bvh_from_arrays reject these already
    s->material_count = mc + 1;
    s->materials.assign(s->material_count, default_material());
    if (ctx) {  // (a host-only scene: build + export work, nothing is uploaded and nothing can be rendered)
        DeviceGuard g(ctx->device);
        if (!g.ok) return fail(MP_ERR_HIP, "hipSetDevice failed");
        if (int rc = upload_scene(s.get())) return rc;
    }
    *out = s.release();
    return MP_OK;
}

// UnitQuaternion * Vector3, the operation order of the oracle and of the device code (group_walk.h: quat_rotate)
void quat_rotate_host(const float q[4], const float v[3], float out[3]) {
    const float tx = (q[1] * v[2] - q[2] * v[1]) * 2.0f, ty = (q[2] * v[0] - q[0] * v[2]) * 2.0f, tz = (q[0] * v[1] - q[1] * v[0]) * 2.0f;
    const float cx = q[1] * tz - q[2] * ty, cy = q[2] * tx - q[0] * tz, cz = q[0] * ty - q[1] * tx;
    out[0] = tx * q[3] + cx + v[0];
    out[1] = ty * q[3] + cy + v[1];
    out[2] = tz * q[3] + cz + v[2];
}

// {object, rigid transform} x n behind one Object (include/minipath_hip.h: mp_scene_group).  The group borrows its members' device
// arrays; it owns the descriptor array and its own material table.
int make_group(mp_ctx* ctx, const mp_scene* const* objects, const float* rotations, const float* translations, uint32_t n,
               bool one_object, mp_scene** out) {
    if (!objects || !translations || !out || n == 0) return fail(MP_ERR_INVALID, "bad argument");
    if (n > (1u << 20)) return fail(MP_ERR_INVALID, "too many members");
    for (uint32_t i = 0; i < n; i++) {
        const mp_scene* o = objects[i];
        if (!o) return fail(MP_ERR_INVALID, "NULL member");
        if (o->inst_of) return fail(MP_ERR_UNSUPPORTED, "the members of an object group are TriangleBvh or Sphere scenes, not groups");
        if (one_object && o->dev.kind != 0u) return fail(MP_ERR_UNSUPPORTED, "instances are made of a TriangleBvh scene");
        if (o->ctx != ctx) return fail(MP_ERR_INVALID, "member belongs to another context");
    }
    auto s = std::make_unique<mp_scene>();
    s->ctx = ctx;
    s->inst_of = objects[0];
    s->one_object = one_object;
    s->members.assign(objects, objects + n);
    s->inst_t.assign(translations, translations + static_cast<size_t>(n) * 3);
    s->host.root = objects[0]->host.root;
    s->host.material_names = objects[0]->host.material_names;
    s->material_count = 1;
    s->dev = DevScene{};  // kind 0; every geometry field comes from the member descriptors
    s->dev.packet_stack_regs = objects[0]->dev.packet_stack_regs;
    s->dev.materials = objects[0]->dev.materials;
    s->dev.sky = objects[0]->sky;
    for (uint32_t i = 0; i < n; i++) {
        const mp_scene* o = objects[i];
        s->host.depth = std::max(s->host.depth, o->host.depth);
        if (!one_object || i == 0) {  // instances of one object report the object's own counts
            s->host.vertex_count += o->host.vertex_count;
            s->host.triangle_count += o->host.triangle_count;
        }
        s->material_count = std::max(s->material_count, o->material_count);
        s->dev.stack_cap = std::max(s->dev.stack_cap, o->dev.stack_cap);
    }
    // get_bounding_box: union of the members' boxes in the world frame (a rotated member: the box of its box's eight rotated corners)
    for (uint32_t i = 0; i < n; i++) {
        const Box3& ob = objects[i]->host.bbox;
        float lo[3], hi[3];
        if (rotations) {
            const float* q = rotations + 4 * static_cast<size_t>(i);
            for (int c = 0; c < 8; c++) {
                const float v[3] = {(c & 1) ? ob.mx[0] : ob.mn[0], (c & 2) ? ob.mx[1] : ob.mn[1], (c & 4) ? ob.mx[2] : ob.mn[2]};
                float w[3];
                quat_rotate_host(q, v, w);
                for (int k = 0; k < 3; k++) {
                    lo[k] = c ? std::fmin(lo[k], w[k]) : w[k];
                    hi[k] = c ? std::fmax(hi[k], w[k]) : w[k];
                }
            }
        } else {
            for (int k = 0; k < 3; k++) { lo[k] = ob.mn[k]; hi[k] = ob.mx[k]; }
        }
        for (int k = 0; k < 3; k++) {
            const float a = lo[k] + translations[3 * i + k], b = hi[k] + translations[3 * i + k];
            s->host.bbox.mn[k] = i ? std::fmin(s->host.bbox.mn[k], a) : a;
            s->host.bbox.mx[k] = i ? std::fmax(s->host.bbox.mx[k], b) : b;
        }
    }
    // material table of the group: the first member's, padded with the default material up to the largest id any member uses
    s->materials = objects[0]->materials;
    if (s->materials.size() < s->material_count) s->materials.resize(s->material_count, default_material());
    s->sky = objects[0]->sky;
    s->dev.materials_rgb = table_is_grey(s->materials) ? 0u : 1u;
    s->dev.inst_count = n;
    s->dev.has_pre = 0;
    if (ctx) {
        DeviceGuard g(ctx->device);
        std::vector<DevObject> desc(n);
        for (uint32_t i = 0; i < n; i++) {
            const DevScene& d = objects[i]->dev;
            DevObject& o = desc[i];
            std::memset(&o, 0, sizeof(o));
            o.shade = d.shade; o.nodes_aos = d.nodes_aos; o.nodes_lit = d.nodes_lit; o.tris_aos = d.tris_aos; o.vidx = d.vidx; o.vtex = d.vtex;
            o.root = d.root; o.root_lit = d.root_lit; o.has_pre = d.has_pre;
            o.kind = d.kind; o.sphere_radius = d.sphere_radius;
            for (int k = 0; k < 3; k++) {
                o.pre_min[k] = d.pre_min[k]; o.pre_max[k] = d.pre_max[k]; o.t[k] = translations[3 * i + k];
                o.sphere_center[k] = d.sphere_center[k];
            }
            if (rotations) {
                for (int k = 0; k < 4; k++) o.q[k] = rotations[4 * static_cast<size_t>(i) + k];
                o.rotated = 1u;
            }
        }
        const size_t bytes = desc.size() * sizeof(DevObject);
        MP_HIP(s->inst.grow(bytes));
        hipError_t e = hipMemcpy(s->inst.get(), desc.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(object group)");
        s->dev.objects = s->inst.as<const DevObject>();
        s->device_bytes = bytes;
        // the group's own copy of the table: a later mp_scene_set_materials on a member does not reach the group
        auto tb = std::make_shared<DeviceBuffer>();
        e = tb->grow(std::max<size_t>(16, s->materials.size() * sizeof(mp_material)));
        if (e == hipSuccess) e = hipMemcpy(tb->get(), s->materials.data(), s->materials.size() * sizeof(mp_material), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "material table of the object group");
        s->mat_table = std::move(tb);
        s->dev.materials = s->mat_table->as<const float>();
    }
    // the group is complete: one reference per member it borrows from (instances of one object: one in all)
    for (size_t i = 0; i < (one_object ? 1 : static_cast<size_t>(n)); i++) const_cast<mp_scene*>(objects[i])->refs.fetch_add(1, std::memory_order_relaxed);
    *out = s.release();
    return MP_OK;
}

// Drops one reference; the last one destroys the scene (its buffers go with it) and, for an object group, drops the group's
// reference on each member.
void scene_release(mp_scene* s) {
    if (!s || s->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    const size_t held = !s->inst_of ? 0 : s->one_object ? 1 : s->members.size();
    for (size_t i = 0; i < held; i++) scene_release(const_cast<mp_scene*>(s->members[i]));
    delete s;
}

}  // namespace

extern "C" {

const char* mp_scene_material_name(const mp_scene* scene, uint32_t id) {
    if (!scene || id >= scene->material_count) return nullptr;
    return id < scene->host.material_names.size() ? scene->host.material_names[id].c_str() : "";
}

int mp_scene_from_obj(mp_ctx* ctx, const char* path, mp_scene** out) {
    return guarded([&]() -> int {
    if (!path || !out) return fail(MP_ERR_INVALID, "NULL argument");
    std::vector<float> pos, nrm, tex;
    std::vector<uint32_t> tri, tri_mat;
    std::vector<std::string> names;
    std::string err;
    int rc = load_obj(path, pos, nrm, tex, tri, tri_mat, names, err);
    if (rc) return fail(rc, err);
    auto s = std::make_unique<mp_scene>();
    rc = build_bvh(pos.data(), nrm.data(), tex.data(), static_cast<uint32_t>(pos.size() / 3), tri.data(), tri_mat.data(),
                   static_cast<uint32_t>(tri.size() / 3), s->host, err);
    if (rc) return fail(rc, err);
    s->host.material_names = std::move(names);
    return finish_scene(ctx, std::move(s), out);
    });
}

int mp_scene_from_triangles(mp_ctx* ctx, const float* positions, const float* normals, const float* tex,
                            uint32_t vertex_count, const uint32_t* indices, uint32_t triangle_count, mp_scene** out) {
    return mp_scene_from_triangles_mat(ctx, positions, normals, tex, vertex_count, indices, nullptr, triangle_count, out);
}

int mp_scene_from_triangles_mat(mp_ctx* ctx, const float* positions, const float* normals, const float* tex,
                                uint32_t vertex_count, const uint32_t* indices, const uint32_t* tri_material,
                                uint32_t triangle_count, mp_scene** out) {
    return guarded([&]() -> int {
    if (!positions || !indices || !out) return fail(MP_ERR_INVALID, "NULL argument");
    auto s = std::make_unique<mp_scene>();
    std::string err;
    int rc = build_bvh(positions, normals, tex, vertex_count, indices, tri_material, triangle_count, s->host, err);
    if (rc) return fail(rc, err);
    return finish_scene(ctx, std::move(s), out);
    });
}

int mp_scene_from_arrays(mp_ctx* ctx, const mp_bvh_desc* desc, mp_scene** out) {
    return guarded([&]() -> int {
    if (!desc || !out) return fail(MP_ERR_INVALID, "NULL argument");
    auto s = std::make_unique<mp_scene>();
    std::string err;
    int rc = bvh_from_arrays(*desc, s->host, err);
    if (rc) return fail(rc, err);
    return finish_scene(ctx, std::move(s), out);
    });
}

int mp_scene_group(mp_ctx* ctx, const mp_scene* const* objects, const float* rotations, const float* translations, uint32_t n,
                   mp_scene** out) {
    return guarded([&]() -> int { return make_group(ctx, objects, rotations, translations, n, false, out); });
}

int mp_scene_instances(mp_ctx* ctx, const mp_scene* object, const float* translations, uint32_t n, mp_scene** out) {
    return guarded([&]() -> int {
    if (!object || n == 0 || n > (1u << 20)) return fail(MP_ERR_INVALID, "bad argument");
    std::vector<const mp_scene*> objs(n, object);
    return make_group(ctx, objs.data(), nullptr, translations, n, true, out);
    });
}

int mp_scene_set_materials(mp_scene* scene, const mp_material* table, uint32_t n, float sky_radiance) {
    return guarded([&]() -> int {
    if (!scene || !table) return fail(MP_ERR_INVALID, "NULL argument");
    if (scene->dev.kind != 0u) return fail(MP_ERR_UNSUPPORTED, "materials belong to TriangleBvh scenes");
    if (n < scene->material_count) return fail(MP_ERR_INVALID, "material table shorter than the scene's material_count");
    for (uint32_t i = 0; i < n; i++)
        if (table[i].texture != MP_TEXTURE_NONE && table[i].texture != MP_TEXTURE_CHECKER) return fail(MP_ERR_INVALID, "unknown texture kind in the material table");
    std::vector<mp_material> materials(table, table + n);
    std::shared_ptr<DeviceBuffer> tb;
    if (scene->ctx) {  // a new table for this scene; instanced scenes made earlier keep the one they were created with
        DeviceGuard g(scene->ctx->device);
        tb = std::make_shared<DeviceBuffer>();
        MP_HIP(tb->grow(std::max<size_t>(16, n * sizeof(mp_material))));
        MP_HIP(hipMemcpy(tb->get(), materials.data(), n * sizeof(mp_material), hipMemcpyHostToDevice));
    }
    // the scene changes only now that the new table is on the device
    scene->materials = std::move(materials);
    scene->sky = sky_radiance;
    scene->dev.materials_rgb = table_is_grey(scene->materials) ? 0u : 1u;
    if (tb) {
        scene->mat_table = std::move(tb);  // the old table is freed when its last holder lets go (the free waits for the device)
        scene->dev.materials = scene->mat_table->as<const float>();
        scene->dev.sky = sky_radiance;
    }
    return MP_OK;
    });
}

int mp_scene_sphere(mp_ctx* ctx, const float center[3], float radius, mp_scene** out) {
    return guarded([&]() -> int {
    if (!center || !out) return fail(MP_ERR_INVALID, "NULL argument");
    auto s = std::make_unique<mp_scene>();
    s->ctx = ctx;
    s->dev.kind = 1;
    for (int k = 0; k < 3; k++) {
        s->dev.sphere_center[k] = center[k];
        s->host.bbox.mn[k] = center[k] - radius;  // get_bounding_box, primitives.rs:50-56
        s->host.bbox.mx[k] = center[k] + radius;
    }
    s->dev.sphere_radius = radius;
    s->dev.stack_cap = 1;
    *out = s.release();
    return MP_OK;
    });
}

void mp_scene_destroy(mp_scene* s) { scene_release(s); }

int mp_scene_info_get(const mp_scene* s, mp_scene_info* out) {
    return guarded([&]() -> int {
    if (!s || !out) return fail(MP_ERR_INVALID, "NULL argument");
    out->root_link = s->host.root;
    out->inner_count = static_cast<uint32_t>(s->host.inner.size());
    out->packet_count = static_cast<uint32_t>(s->host.packets.size());
    if (s->inst_of) {  // object group: sums over the members (instances of one object: the object's own counts)
        uint64_t ni = 0, np = 0;
        for (size_t i = 0; i < (s->one_object ? 1 : s->members.size()); i++) {
            ni += s->members[i]->host.inner.size();
            np += s->members[i]->host.packets.size();
        }
        out->inner_count = static_cast<uint32_t>(ni);
        out->packet_count = static_cast<uint32_t>(np);
    }
    out->vertex_count = s->host.vertex_count;
    out->triangle_count = s->host.triangle_count;
    out->depth = s->host.depth;
    out->stack_bound = s->ctx ? s->dev.stack_cap : 0;
    for (int k = 0; k < 3; k++) {
        out->bbox_min[k] = s->host.bbox.mn[k];
        out->bbox_max[k] = s->host.bbox.mx[k];
    }
    out->device_bytes = s->device_bytes;
    out->material_count = s->material_count;
    out->reserved = 0;
    return MP_OK;
    });
}

int mp_scene_export(const mp_scene* s, void* inner_nodes, void* packets, void* tri_shading, float* vertex_normals,
                    float* vertex_tex, uint32_t* tri_material) {
    return guarded([&]() -> int {
    if (!s) return fail(MP_ERR_INVALID, "scene is NULL");
    if (s->inst_of && !s->one_object) return fail(MP_ERR_UNSUPPORTED, "an object group has no arrays of its own: export its members");
    const HostBvh& h = s->inst_of ? s->inst_of->host : s->host;
    if (inner_nodes && !h.inner.empty()) std::memcpy(inner_nodes, h.inner.data(), h.inner.size() * sizeof(InnerNodeRef));
    if (packets && !h.packets.empty()) std::memcpy(packets, h.packets.data(), h.packets.size() * sizeof(TriPacketRef));
    if (tri_shading && !h.shading.empty()) std::memcpy(tri_shading, h.shading.data(), h.shading.size() * sizeof(TriShadingRef));
    if (vertex_normals && !h.vnormal.empty()) std::memcpy(vertex_normals, h.vnormal.data(), h.vnormal.size() * 4);
    if (vertex_tex && !h.vtex.empty()) std::memcpy(vertex_tex, h.vtex.data(), h.vtex.size() * 4);
    if (tri_material && !h.material.empty()) std::memcpy(tri_material, h.material.data(), h.material.size() * 4);
    return MP_OK;
    });
}

int mp_scene_device_tree(const mp_scene* s, int which, float* nodes, uint32_t* count, uint32_t* root_dlink, uint32_t* stack_bound,
                         uint32_t* absorbed) {
    return guarded([&]() -> int {
    if (!s) return fail(MP_ERR_INVALID, "scene is NULL");
    if (which < 0 || which > 2) return fail(MP_ERR_INVALID, "which must be 0 (wide tree), 1 (literal tree) or 2 (packet tree)");
    if (s->dev.kind != 0u || (s->inst_of && !s->one_object)) return fail(MP_ERR_UNSUPPORTED, "only a TriangleBvh scene has a node tree of its own");
    const mp_scene* own = s->inst_of ? s->inst_of : s;
    const HostBvh& h = own->host;
    const std::vector<uint32_t> pkt_valid = packet_real_counts(h);
    DeviceTree t;
    std::string err;
    int rc = build_device_tree(h, pkt_valid, which != 1, t, err);  // rebuilt from the host tree: same code, same floats as the upload
    if (!rc && which == 2 && own->packet_tree_slots == 16u) {  // the upload's choice between the packet tree and the wide tree
        DeviceTree lit, pk;
        rc = build_device_tree(h, pkt_valid, false, lit, err);
        if (!rc) rc = build_device_tree(h, pkt_valid, true, pk, err, 16);
        if (!rc && packet_tree_applies(pk, t, lit, own->packet_tree_slots)) t = std::move(pk);
    }
    if (rc) return fail(rc, err);
    // which = 2: the ROOT's record behind the last node travels too (the cached walk starts there)
    const size_t dwords = static_cast<size_t>(t.count) * t.slots * 8 + (which == 2 ? 8 : 0);
    if (nodes && dwords) std::memcpy(nodes, t.nodes.data(), dwords * sizeof(float));
    if (count) *count = t.count;
    if (root_dlink) *root_dlink = t.root;
    if (stack_bound) *stack_bound = t.stack_bound;
    if (absorbed) *absorbed = t.absorbed;
    return MP_OK;
    });
}

}  // extern "C"
