/*
 * pm_scene.h — the host scene and its assembly into the scene blob the
 * kernels read (SceneDev, pm_device.h). Host code only, no HIP: pm_api_scene.cpp
 * fills a HostScene through the pm_add_* calls; pm_commit makes the
 * primitive boxes, assembles the blob here (or lets the device build the
 * tree, with the same layout) and uploads it. tests/native checks the
 * assembly on the CPU.
 */
#pragma once
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "pm_build.h"
#include "pm_scene_pod.h"

namespace pm {

inline float4 f4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
inline int4 i4(int x, int y, int z, int w) { int4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
inline float ibits(int v) { float f; std::memcpy(&f, &v, 4); return f; }
inline int fbits_h(float f) { int v; std::memcpy(&v, &f, 4); return v; }
inline float bits_f(uint32_t v) { float f; std::memcpy(&f, &v, 4); return f; }

/* ------------------------------------------------------------ host scene */
struct HMesh { int material, light, has_n, has_uv; };
struct HTri { int v[3]; int mesh; uint32_t gid; }; /* gid: global id (insertion order over all triangles) */
/* two-level instancing: an object mesh stored once in object space, and its
 * instances (pbrt ObjectBegin / ObjectInstance) */
struct HObj {
    std::vector<float> P, N, UV;
    std::vector<int> idx;
    int material = 0, light = -1;
    bool has_n = false, has_uv = false;
};
struct HInst { int obj; float m[16], minv[16]; uint32_t gid_base; };

struct HostScene {
    std::vector<float4> materials;
    std::vector<float> P, N, UV;
    std::vector<HMesh> meshes;
    std::vector<HTri> tris;
    int64_t next_tri_id = 0;     /* global ids handed out to triangles (meshes and instances); < 2^31 */
    std::vector<HObj> objs;
    std::vector<HInst> insts;
    std::vector<float4> disks;   /* 5 per disk */
    std::vector<float4> spheres; /* 4 per sphere */
    std::vector<float> sphere_o2w;
    std::vector<LightDev> lights;
    std::vector<LightTri> light_tris; /* the mesh lights' emitting triangles, light after light (SceneDev::light_tris) */
    /* textures (pm_add_texture_*): the records, every image's texels (rgb, 0),
     * and per material its Kd texture (-1: none; may be shorter than
     * materials, the missing entries meaning none) */
    std::vector<TexRec> textures;
    std::vector<float4> texels;
    std::vector<int> mat_tex;
    /* the physical specular model (pm_add_material_specular): per material 2
     * float4, (Kr, index) (Kt, 1 as int bits); may be shorter than materials,
     * the missing entries and all-zero ones meaning the reference's model */
    std::vector<float4> mat_spec;
};

/* Everything below that can fail returns PM_OK or an error code with its
 * message in `err` (pm_commit hands both to the caller unchanged). */

/* a committable scene has lights and shapes and fewer than 2^30 primitives
 * of a kind; numbers the disks and spheres: global ids are triangles (meshes
 * and instances, in insertion order), then disks, then spheres */
int validate_scene(HostScene &hs, std::string &err);

/* ------------------------------------------------------ geometry helpers */
void tri_frame(const float *p0, const float *p1, const float *p2, const float *UV, const int *v, const float *n,
               float *ns, float *dpdu);
/* per triangle t: (p0, e0, e1, n) for the intersector (3 float4), the
 * normalized shading frame for hits (2 float4), vertex ids + mesh (1 int4) */
void tri_record(const HostScene &hs, uint32_t t, float *geo, float *shade, int *info);
std::vector<float4> vertex_normals(const HostScene &hs);
/* an instance's world vertex as pbrt's Transform::operator()(Point) computes
 * it for an affine transform (w == 1): the device's inst_point, bit for bit */
inline void inst_point_h(const float *m, const float *p, float *o) {
    for (int a = 0; a < 3; ++a) o[a] = m[4 * a] * p[0] + m[4 * a + 1] * p[1] + m[4 * a + 2] * p[2] + m[4 * a + 3];
}

/* ------------------------------------------------------- primitive boxes */
/* the build box of a primitive: its bounds padded by 1e-4 of their magnitude (at least 1e-4) */
BuildPrim make_box(const float lo[3], const float hi[3], uint32_t ref);
/* one box per triangle (in parallel chunks), disk, sphere and instance, in
 * that order, and the unpadded bounds of the scene */
void scene_boxes(const HostScene &hs, std::vector<BuildPrim> &prims, float blo[3], float bhi[3]);

/* ---------------------------------------------------------------- layout */
/* the sections of the scene blob, in the order they lie in it */
enum SceneSection {
    SEC_NODES,   /* binary BVH nodes, 4 float4 each */
    SEC_REFS, SEC_GEO, SEC_SHADE, SEC_TID, SEC_INFO, SEC_NORMS, SEC_DISKS, SEC_SPHERES, SEC_MATS, SEC_LIGHTS,
    SEC_OBJV, SEC_OBJINFO, SEC_OBJN, SEC_OBJUV, SEC_OBJMESH, SEC_INSTS, /* instancing */
    SEC_WNODES,  /* the wide tree; with instances the objects' trees follow the top-level one */
    SEC_COUNT
};
/* bytes per element of a section */
constexpr size_t NODE_BYTES = 64, REF_BYTES = 4, TRI_GEO_BYTES = 48, TRI_SHADE_BYTES = 32, TRI_ID_BYTES = 4,
                 TRI_INFO_BYTES = 16, NODE_PLACEHOLDER_BYTES = 16 /* a scene without a binary tree */, INST_BYTES = 128, OBJ_TRI_BYTES = 48, BVH4Q_NODE_BYTES = 64,
                 BVH8Q_NODE_BYTES = 128;
constexpr size_t TRI_GEO_FLOATS = TRI_GEO_BYTES / 4, TRI_SHADE_FLOATS = TRI_SHADE_BYTES / 4, TRI_INFO_INTS = TRI_INFO_BYTES / 4;
constexpr size_t wide_node_bytes(int wide) { return wide == 3 ? BVH8Q_NODE_BYTES : BVH4Q_NODE_BYTES; }

/* where each section of the scene blob lies. One blob of 16-B aligned
 * sections: the same offsets address it in HBM and, for scenes that fit
 * (SceneDev::lds_bytes), in each block's LDS copy */
struct SceneLayout {
    size_t off[SEC_COUNT] = {}, size[SEC_COUNT] = {}; /* size: the bytes in use (an absent section has none) */
    size_t bytes = 0;
    int64_t n_nodes = 0, n_refs = 0, n_tris = 0;
    bool id_order = false;
    int wide = 0, wide_stack = 0; /* SceneDev::wide, the wide tree's stack bound */
};
/* sizes of the sections both builders fill from the host scene as it is */
void count_sections(SceneLayout &L, const HostScene &hs, int64_t n_refs, int64_t n_tris);
/* the planner: off[] and bytes from size[]. never_lds keeps the blob above
 * LDS_SCENE_MAX (scenes whose traversal reads no binary tree: instanced or device-built) */
void plan_layout(SceneLayout &L, bool never_lds);

/* --------------------------------------------------------- build options */
/* the build knobs of a commit, read from the environment when it starts
 * (tests switch them between contexts) */
struct BuildOptions {
    std::string build = "auto"; /* PM_BVH_BUILD */
    int64_t gpu_min = 1 << 16;  /* PM_BVH_GPU_MIN */
    int ploc_radius = 3;        /* PM_PLOC_RADIUS */
    bool bfs_set = false, bfs = false; /* PM_BVH4_BFS: set at all (a host-path switch), and non-zero */
    bool bvh8 = false;          /* PM_BVH8 */
    bool times = false;         /* PM_COMMIT_TIMES */
};
BuildOptions build_options_from_env();
bool gpu_bvh_wanted(const BuildOptions &opt, int64_t nprims);

/* -------------------------------------------------------- host assembly */
struct SceneBlob {
    std::vector<unsigned char> bytes;
    SceneLayout layout;
    /* id-ordered (brute-force) scenes: pair j = storage slots 2j, 2j + 1,
     * each of the 12 (p0, e0, e1, n) components as two adjacent floats, so a
     * scalar load puts the packed operand of both triangles in an aligned
     * SGPR pair (SceneDev::tri_pairs_g); empty otherwise */
    std::vector<float> tri_pairs;
    int bvh_depth = 0;
    int64_t bvh4_nodes = 0; /* nodes of the wide tree (0: binary traversal) */
    int bvh4_depth = 0;
    int64_t obj_tris_stored = 0; /* object triangles in the blob (each mesh once) */
    std::vector<float4> tri_uv;  /* textured scenes: SceneDev::tri_uv in storage order (triangle_uvs); else empty */
};
/* The blob with every tree built on the host. prims: scene_boxes' (the
 * builder reorders them); t0: the commit's start, for the PM_COMMIT_TIMES lines. */
int assemble_scene(const HostScene &hs, std::vector<BuildPrim> &prims, const BuildOptions &opt,
                   std::chrono::steady_clock::time_point t0, SceneBlob &out, std::string &err);

/* quantized 4-wide nodes moved to start at node `base`: internal child codes shift */
void relocate_bvh4(std::vector<uint32_t> &q, uint32_t base);

/* ---------------------------------------------------------- distant light */
/* pbrt's CoordinateSystem(v, &v1, &v2) for a unit v, in double */
void coordinate_system(const double v[3], double v1[3], double v2[3]);
/* the record of pm_add_light_distant (pm_api.h), its parameters checked; it
 * carries the direction only (n_area.xyz = -to_light) until finish_lights */
int make_distant_light(const float to_light[3], const float L[3], LightDev &out, std::string &err);
/* the world sphere (pm_api.h pm_add_light_distant) of scene_boxes' unpadded
 * bounds: sphere = centre xyz, radius */
void world_sphere(const float blo[3], const float bhi[3], float sphere[4]);
/* a commit's last word on the lights, before either builder copies them:
 * the world sphere, and every distant light's record filled from it */
int finish_lights(HostScene &hs, const float blo[3], const float bhi[3], float sphere[4], std::string &err);

/* --------------------------------------------------------------- textures */
/* The pm_add_texture_* calls of pm_api.h. The check_* functions look at the
 * arguments alone (pm_api_scene.cpp runs them before it touches the context); the
 * add_* ones repeat them, resolve operand ids against the scene and append
 * the record. An operand id names a TEX_SINGLE record (an image or a
 * constant); a checkerboard or a scale as an operand is refused. */
int check_texture_image(const float *rgb, int w, int h, int wrap, const float *mapping, const float *scale, std::string &err);
int check_texture_operands(const char *who, const float *mapping, bool need_mapping, int tex1, const float *rgb1, int tex2,
                           const float *rgb2, std::string &err);
int add_texture_image(HostScene &hs, const float *rgb, int w, int h, int wrap, const float *mapping, const float *scale,
                      int *out_tex, std::string &err);
int add_texture_checker(HostScene &hs, const float *mapping, int tex1, const float *rgb1, int tex2, const float *rgb2,
                        int *out_tex, std::string &err);
int add_texture_scale(HostScene &hs, int tex1, const float *rgb1, int tex2, const float *rgb2, int *out_tex, std::string &err);
/* a matte whose Kd is texture kd_tex: (1, 1, 1) in the materials table (the
 * gathers sum with f = 1 / pi; pm_final applies the texel), kd_tex in mat_tex */
int check_material_textured(int type, std::string &err);
int add_material_textured(HostScene &hs, int type, int kd_tex, int *out_id, std::string &err);
/* does a material of the scene carry a texture? */
bool scene_textured(const HostScene &hs);
/* SceneDev::mat_tex: one entry per material */
std::vector<int> material_textures(const HostScene &hs);
/* SceneDev::tri_uv: per storage slot k the uvs of triangle tri_order[k]'s
 * corners, (uv0, uv1) (uv2, 0, 0); tri_frame's default corners for a mesh
 * without uvs, so a surface's frame and its texture coordinates agree */
std::vector<float4> triangle_uvs(const HostScene &hs, const uint32_t *tri_order, int64_t n);
/* the largest |component| texture t can return, and whether one can be negative */
double texture_bound(const HostScene &hs, int t, bool *negative);

/* ------------------------------------------------------ specular materials */
/* pm_add_material_specular (pm_api.h): check_ looks at the arguments alone
 * (a mirror's kt and index are not looked at), add_ repeats it and appends
 * the material: (0, 0, 0, type) in the materials table, as pm_add_material
 * stores a specular type, and its parameters in mat_spec */
int check_material_specular(int type, const float *kr, const float *kt, float index, std::string &err);
int add_material_specular(HostScene &hs, int type, const float *kr, const float *kt, float index, int *out_id,
                          std::string &err);
/* does a material of the scene use the physical model? */
bool scene_specular(const HostScene &hs);
/* SceneDev::mat_spec: two entries per material, zero for the others */
std::vector<float4> material_specular_table(const HostScene &hs);

/* --------------------------------------------------------- light summary */
/* pm_light_selection_cdf (pm_api.h) */
int light_selection_cdf(const int *types, const float *le_rgb, const float *areas, int n, float *cdf_out, std::string &err);
struct LightSummary {
    /* bounds for the fixed-point flux scale: emit_max the largest single
     * light's Le / pdf bound (a fixed light_source_index); emit_max_all the
     * same under PM_ALL_LIGHTS, where the pick's probability divides the
     * weight: max_l(bound_l / pmf_l) over the lights with pmf_l > 0 of the
     * float table */
    double emit_max = 1.0, emit_max_all = 1.0, kd_max = 1.0;
    /* the largest lobe colour (>= 1) of the materials of the physical specular
     * model: a photon's flux grows by at most spec_max^max_specular_depth */
    double spec_max = 1.0;
    bool scene_nonneg = true; /* no negative emission / albedo component (fixed-point sums in double) */
    /* PM_ALL_LIGHTS: the selection table over the scene's lights; all zero
     * and cdf_ok false when their total selection weight is 0 or not finite */
    std::vector<float> cdf;
    bool cdf_ok = false;
};
int light_summary(const HostScene &hs, LightSummary &out, std::string &err);

} // namespace pm
