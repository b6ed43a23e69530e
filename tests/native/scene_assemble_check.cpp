/* Host check of pm_scene.cpp's scene assembly (tests/test_scene_assemble.py):
 * builds four scenes from a fixed LCG (12, 100 and 3,000 triangles — the
 * last with a disk and a sphere — and one 32-triangle object instanced three
 * times), assembles each and checks the blob the kernels would read: the
 * layout (aligned, canonical order, no overlap, inside the blob, sizes =
 * element counts), the refs, tri_id a permutation of the global ids,
 * tri_geo / tri_shade / tri_info of every slot = tri_record of its triangle,
 * relocated object trees inside their node ranges, and the planner giving
 * the device-build path the same placement of the shared sections. Prints
 * one line per scene with a hash of the blob (the test compares them across
 * PM_BUILD_THREADS) and "bad N". */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>

#include "pm_scene.h"
using namespace pm;

static uint32_t g_lcg = 12345u;
static float rnd() { g_lcg = g_lcg * 1664525u + 1013904223u; return (float)(g_lcg >> 8) * (1.0f / 16777216.0f); }

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { printf("FAIL %s: ", name); printf(__VA_ARGS__); printf("\n"); } } } while (0)

/* n random triangles with normals and uvs, as pm_add_trimesh stores them */
static void add_soup(HostScene &hs, int n) {
    const int mesh = (int)hs.meshes.size(), base = (int)(hs.P.size() / 3);
    hs.meshes.push_back(HMesh{0, -1, 1, 1});
    for (int t = 0; t < n; ++t) {
        const float c[3] = {30.f + 495.f * rnd(), 30.f + 495.f * rnd(), 30.f + 495.f * rnd()};
        for (int q = 0; q < 3; ++q) {
            for (int a = 0; a < 3; ++a) hs.P.push_back(c[a] + 8.f * rnd() - 4.f);
            for (int a = 0; a < 3; ++a) hs.N.push_back(rnd() - 0.5f);
            for (int a = 0; a < 2; ++a) hs.UV.push_back(rnd());
        }
        hs.tris.push_back(HTri{{base + 3 * t, base + 3 * t + 1, base + 3 * t + 2}, mesh, (uint32_t)hs.next_tri_id++});
    }
}
static void add_basics(HostScene &hs) {
    hs.materials.push_back(f4(0.5f, 0.5f, 0.5f, ibits(PM_MATTE)));
    LightDev L{};
    L.o_type = f4(278.f, 500.f, 278.f, ibits(PM_LIGHT_POINT));
    L.p1_ns = f4(0, 0, 0, ibits(1));
    L.le = f4(100.f, 100.f, 100.f, 0.f);
    hs.lights.push_back(L);
}
static void add_disk_and_sphere(HostScene &hs) {
    const float o[3] = {278.f, 540.f, 278.f}, x[3] = {60.f, 0.f, 0.f}, y[3] = {0.f, 0.f, 60.f}, z[3] = {0.f, -1.f, 0.f};
    hs.disks.push_back(f4(o[0], o[1], o[2], 0.f));
    hs.disks.push_back(f4(x[0], x[1], x[2], 6.2831853f));
    hs.disks.push_back(f4(y[0], y[1], y[2], o[0] * z[0] + o[1] * z[1] + o[2] * z[2]));
    hs.disks.push_back(f4(z[0], z[1], z[2], 1.f / 3600.f));
    hs.disks.push_back(f4(1.f / 3600.f, ibits(0), ibits(-1), ibits(0)));
    const float m[16] = {1, 0, 0, 100, 0, 1, 0, 80, 0, 0, 1, 120, 0, 0, 0, 1};
    hs.spheres.push_back(f4(1, 0, 0, -100));
    hs.spheres.push_back(f4(0, 1, 0, -80));
    hs.spheres.push_back(f4(0, 0, 1, -120));
    hs.spheres.push_back(f4(40.f, ibits(0), ibits(-1), ibits(0)));
    hs.sphere_o2w.insert(hs.sphere_o2w.end(), m, m + 16);
}
static void add_instances(HostScene &hs, int obj_tris, int n_inst) {
    HObj o;
    for (int t = 0; t < obj_tris; ++t) {
        const float c[3] = {20.f * rnd(), 20.f * rnd(), 20.f * rnd()};
        for (int q = 0; q < 3; ++q) {
            for (int a = 0; a < 3; ++a) o.P.push_back(c[a] + 2.f * rnd() - 1.f);
            o.idx.push_back(3 * t + q);
        }
    }
    hs.objs.push_back(o);
    for (int i = 0; i < n_inst; ++i) {
        HInst in{};
        in.obj = 0;
        const float tx = 100.f + 150.f * i, s = 1.f + i;
        const float m[16] = {s, 0, 0, tx, 0, s, 0, 50, 0, 0, s, 200, 0, 0, 0, 1};
        const float mi[16] = {1 / s, 0, 0, -tx / s, 0, 1 / s, 0, -50 / s, 0, 0, 1 / s, -200 / s, 0, 0, 0, 1};
        std::memcpy(in.m, m, sizeof m);
        std::memcpy(in.minv, mi, sizeof mi);
        in.gid_base = (uint32_t)hs.next_tri_id;
        hs.next_tri_id += obj_tris;
        hs.insts.push_back(in);
    }
}

static void check_scene(const char *name, HostScene &hs) {
    std::string err;
    int rc = validate_scene(hs, err);
    CHECK(rc == PM_OK, "validate: %s", err.c_str());
    std::vector<BuildPrim> prims;
    float lo[3], hi[3];
    scene_boxes(hs, prims, lo, hi);
    const size_t n_prims = prims.size();
    SceneBlob B;
    rc = assemble_scene(hs, prims, BuildOptions(), std::chrono::steady_clock::now(), B, err);
    CHECK(rc == PM_OK, "assemble: %s", err.c_str());
    if (rc != PM_OK) return;
    const SceneLayout &L = B.layout;
    const unsigned char *b = B.bytes.data();

    /* layout: aligned, in order, disjoint, inside the blob */
    CHECK(L.bytes == B.bytes.size() && L.bytes % 16 == 0, "bytes %zu vs %zu", L.bytes, B.bytes.size());
    for (int s = 0; s < SEC_COUNT; ++s) {
        CHECK(L.off[s] % 16 == 0, "section %d offset %zu not aligned", s, L.off[s]);
        CHECK(L.off[s] + L.size[s] <= L.bytes, "section %d ends past the blob", s);
        if (s) CHECK(L.off[s] >= L.off[s - 1] + L.size[s - 1], "section %d overlaps section %d", s, s - 1);
    }
    /* sizes = element counts */
    const size_t nd = hs.disks.size() / 5, ns = hs.spheres.size() / 4, ni = hs.insts.size();
    CHECK((size_t)L.n_refs == n_prims, "n_refs %lld vs %zu prims", (long long)L.n_refs, n_prims);
    CHECK((size_t)L.n_tris == hs.tris.size(), "n_tris %lld", (long long)L.n_tris);
    CHECK(L.size[SEC_NODES] % NODE_BYTES == 0 && (ni || L.size[SEC_NODES] == NODE_BYTES * (size_t)L.n_nodes), "nodes size");
    CHECK(L.size[SEC_REFS] == REF_BYTES * (size_t)L.n_refs, "refs size");
    CHECK(L.size[SEC_GEO] == TRI_GEO_BYTES * (size_t)L.n_tris && L.size[SEC_SHADE] == TRI_SHADE_BYTES * (size_t)L.n_tris &&
          L.size[SEC_TID] == TRI_ID_BYTES * (size_t)L.n_tris && L.size[SEC_INFO] == TRI_INFO_BYTES * (size_t)L.n_tris, "triangle sizes");
    CHECK(L.size[SEC_NORMS] == 16 * (hs.N.size() / 3) && L.size[SEC_DISKS] == 80 * nd && L.size[SEC_SPHERES] == 64 * ns &&
          L.size[SEC_MATS] == 16 * hs.materials.size() && L.size[SEC_LIGHTS] == sizeof(LightDev) * hs.lights.size(), "shape sizes");
    CHECK(L.size[SEC_INSTS] == INST_BYTES * ni && L.size[SEC_OBJV] == OBJ_TRI_BYTES * (size_t)B.obj_tris_stored &&
          L.size[SEC_OBJINFO] == 16 * (size_t)B.obj_tris_stored, "instance sizes");
    CHECK(L.size[SEC_WNODES] == (L.wide ? wide_node_bytes(L.wide) * (size_t)B.bvh4_nodes : 0), "wide nodes size");
    CHECK(L.id_order == (ni == 0 && n_prims <= (size_t)BRUTE_MAX_PRIMS), "id_order");
    CHECK(B.tri_pairs.size() == (L.id_order ? (size_t)std::max<int64_t>(L.n_tris / 2, 1) * 24 : 0), "tri_pairs size");
    CHECK((L.wide != 0) == (ni > 0 || L.bytes > LDS_SCENE_MAX), "wide %d for %zu bytes", L.wide, L.bytes);

    /* refs address stored primitives */
    const uint32_t *refs = (const uint32_t *)(b + L.off[SEC_REFS]);
    for (int64_t i = 0; i < L.n_refs; ++i) {
        const uint32_t kind = refs[i] >> 30, idx = refs[i] & 0x3fffffffu;
        const size_t lim = kind == PRIM_TRI ? (size_t)L.n_tris : kind == PRIM_DISK ? nd : kind == PRIM_SPHERE ? ns : ni;
        CHECK(idx < lim, "ref %lld = %u:%u out of range", (long long)i, kind, idx);
    }
    /* tri_id: a permutation of the triangles' global ids; every slot holds its triangle's record */
    const uint32_t *tid = (const uint32_t *)(b + L.off[SEC_TID]);
    std::vector<uint32_t> want_ids, got_ids(tid, tid + L.n_tris);
    std::vector<uint32_t> tri_of_gid((size_t)hs.next_tri_id, ~0u);
    for (size_t t = 0; t < hs.tris.size(); ++t) { want_ids.push_back(hs.tris[t].gid); tri_of_gid[hs.tris[t].gid] = (uint32_t)t; }
    std::sort(want_ids.begin(), want_ids.end());
    std::sort(got_ids.begin(), got_ids.end());
    CHECK(want_ids == got_ids, "tri_id is not a permutation of the global ids");
    if (want_ids == got_ids)
        for (int64_t k = 0; k < L.n_tris; ++k) {
            float geo[TRI_GEO_FLOATS], shade[TRI_SHADE_FLOATS];
            int info[TRI_INFO_INTS];
            tri_record(hs, tri_of_gid[tid[k]], geo, shade, info);
            CHECK(!std::memcmp(geo, b + L.off[SEC_GEO] + TRI_GEO_BYTES * k, TRI_GEO_BYTES), "tri_geo of slot %lld", (long long)k);
            CHECK(!std::memcmp(shade, b + L.off[SEC_SHADE] + TRI_SHADE_BYTES * k, TRI_SHADE_BYTES), "tri_shade of slot %lld", (long long)k);
            CHECK(!std::memcmp(info, b + L.off[SEC_INFO] + TRI_INFO_BYTES * k, TRI_INFO_BYTES), "tri_info of slot %lld", (long long)k);
            if (L.id_order) CHECK(tid[k] == (uint32_t)k, "id order: slot %lld holds %u", (long long)k, tid[k]);
        }
    /* instanced: the top-level tree's nodes first, then each object's; internal child codes stay in their tree */
    if (ni) {
        CHECK(L.wide == 2, "instanced scene without quantized 4-wide trees");
        const float4 *insts = (const float4 *)(b + L.off[SEC_INSTS]);
        std::set<uint32_t> roots;
        for (size_t i = 0; i < ni; ++i) roots.insert((uint32_t)fbits_h(insts[8 * i + 6].x));
        std::vector<uint32_t> bound(roots.begin(), roots.end()); /* tree k: nodes [bound[k-1], bound[k]) */
        bound.push_back((uint32_t)B.bvh4_nodes);
        CHECK(bound[0] > 0 && bound[0] < B.bvh4_nodes, "first object root %u of %lld nodes", bound[0], (long long)B.bvh4_nodes);
        for (size_t i = 0; i < ni; ++i) {
            const uint32_t r = (uint32_t)fbits_h(insts[8 * i + 6].x);
            CHECK(r >= bound[0] && r < (uint32_t)B.bvh4_nodes, "instance %zu root %u", i, r);
            CHECK((size_t)fbits_h(insts[8 * i + 6].y) + (size_t)fbits_h(insts[8 * i + 6].w) <= (size_t)B.obj_tris_stored, "instance %zu slots", i);
        }
        const uint32_t *q = (const uint32_t *)(b + L.off[SEC_WNODES]);
        for (uint32_t nd4 = 0; nd4 < (uint32_t)B.bvh4_nodes; ++nd4) {
            const size_t tree = std::upper_bound(bound.begin(), bound.end(), nd4) - bound.begin();
            const uint32_t first = tree ? bound[tree - 1] : 0u, last = bound[tree];
            for (int k = 0; k < 4; ++k) {
                const int16_t cnt = (int16_t)((q[16 * nd4 + 10 + k / 2] >> (16 * (k & 1))) & 0xffffu);
                const uint32_t child = q[16 * nd4 + 12 + k];
                if (cnt == 0) CHECK(child >= first && child < last && child != nd4, "node %u child %d -> %u outside [%u, %u)", nd4, k, child, first, last);
            }
        }
    }
    /* the planner: re-planning the same sizes gives the same offsets, and with
     * the device path's sizes (16-B node placeholder, 64 B for each of n - 1
     * wide nodes; the shared sections counted alike) those sections keep
     * their places relative to each other */
    SceneLayout R = L, D;
    plan_layout(R, ni > 0);
    CHECK(!std::memcmp(R.off, L.off, sizeof R.off) && R.bytes == L.bytes, "re-planning moved a section");
    count_sections(D, hs, L.n_refs, L.n_tris);
    D.size[SEC_NODES] = NODE_PLACEHOLDER_BYTES;
    D.size[SEC_WNODES] = BVH4Q_NODE_BYTES * (size_t)(L.n_refs - 1);
    plan_layout(D, true);
    CHECK(D.off[SEC_NODES] == 0 && D.off[SEC_REFS] == 16 && D.bytes > LDS_SCENE_MAX, "device layout start");
    for (int s = SEC_REFS; s <= SEC_LIGHTS; ++s) {
        CHECK(D.size[s] == L.size[s], "device path counts section %d differently", s);
        CHECK(D.off[s] - D.off[SEC_REFS] == L.off[s] - L.off[SEC_REFS], "device path places section %d differently", s);
    }
    CHECK(D.off[SEC_WNODES] + D.size[SEC_WNODES] <= D.bytes && D.off[SEC_WNODES] >= D.off[SEC_LIGHTS] + D.size[SEC_LIGHTS], "device wide nodes");

    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) { const unsigned char *c = (const unsigned char *)p; for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; } };
    mix(B.bytes.data(), B.bytes.size());
    mix(B.tri_pairs.data(), B.tri_pairs.size() * 4);
    printf("%s: %zu prims, %zu bytes, wide %d, %lld wide nodes, depth %d, hash %016llx\n", name, n_prims, L.bytes, L.wide,
           (long long)B.bvh4_nodes, B.bvh_depth, h);
}

int main() {
    { HostScene hs; add_basics(hs); add_soup(hs, 12); check_scene("tris12", hs); }
    { HostScene hs; add_basics(hs); add_soup(hs, 100); check_scene("tris100", hs); }
    { HostScene hs; add_basics(hs); add_soup(hs, 3000); add_disk_and_sphere(hs); check_scene("tris3000+disk+sphere", hs); }
    { HostScene hs; add_basics(hs); add_instances(hs, 32, 3); check_scene("object32x3", hs); }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
