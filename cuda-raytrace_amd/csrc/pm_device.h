/*
 * pm_device.h — what every kernel unit sees of the scene: its layout in HBM
 * (SceneDev) and the block's view of it (scene_view), Ray and Hit, the
 * record-to-pixel map and the census helpers (wave_sum, count4). Included by
 * pm_kernels.h, so by every kernel unit and the API units. The units that
 * trace or shade (pm_trace.hip; pm_eye.hip and pm_fgather.hip through
 * pm_eye_dev.h) add pm_traverse.h (boxes: pm_slab.h, primitives: pm_leaf.h;
 * pm_trace.hip alone the resumable walk, pm_trav_step.h) and pm_shade.h;
 * the vector math is pm_math.h.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pm_api.h"
#include "pm_math.h"
#include "pm_scene_pod.h"

#pragma clang fp contract(off)

namespace pm {

/* ---------------------------------------------------------- scene layout */
/* prim refs, LightDev, LightTri, LDS_SCENE_MAX, BRUTE_MAX_PRIMS, BVH_STACK_DEPTH: pm_scene_pod.h */
struct SceneDev {
    const float4 *nodes;     /* 4 float4 per BVH node */
    const uint32_t *refs;    /* leaf primitive refs */
    const float4 *tri_geo;   /* 3 float4 per triangle: (p0, e0.x) (e0.yz, e1.xy) (e1.z, n) */
    const int4 *tri_info;    /* (v0, v1, v2, mesh) */
    const uint32_t *tri_id;  /* global primitive id (tie-break) */
    /* 2 float4 per triangle, computed on the host with the device's exact
     * IEEE operations (pm_commit): (normalize(n).xyz, material | has_n<<31)
     * (normalize(dpdu).xyz, light). Hit shading is two loads, not ~60 VALU
     * ops + 2 sqrt + 3 divides behind a tri_info -> mesh -> vertex chain. */
    const float4 *tri_shade;
    const float4 *norms;
    const float4 *disks;     /* 5 float4 per disk */
    const float4 *spheres;   /* 4 float4 per sphere */
    const float4 *materials; /* (kd.xyz, type bits) */
    const LightDev *lights;
    int n_lights;
    int n_nodes;
    int stack_depth; /* LDS stack entries per lane (>= BVH depth, <= BVH_STACK_DEPTH) */
    int n_refs;      /* primitives (leaf refs) */
    int n_tris, n_disks, n_spheres;
    int brute;       /* 1: test every primitive wave-uniformly instead of the BVH (tiny LDS scenes) */
    /* HBM copies of tri_geo / tri_id (never rebased to LDS): MODE_BRUTE reads
     * them with wave-uniform indices through the scalar cache into SGPRs */
    const float4 *tri_geo_g;
    const uint32_t *tri_id_g;
    /* brute-force scenes: triangles 2j, 2j + 1 interleaved component by
     * component (24 floats per pair, pm_commit), so each packed operand of
     * isect_tri_pair is one aligned SGPR pair of a scalar load */
    const float *tri_pairs_g;
    /* wide BVH (4 uint4 per quantized 4-wide node, pm_build.h quantize_bvh4;
     * 8 uint4 per 8-wide node, quantize_bvh8) for scenes traversed from HBM
     * (MODE_GLOBAL) when wide != 0; the binary nodes stay for the LDS modes */
    const float4 *wnodes;
    int wide;        /* wide BVH in wnodes: 2 = 64-B quantized 4-wide nodes, 3 = 128-B quantized 8-wide (pm_build.h) */
    /* two-level instancing (pm_add_object_mesh / pm_add_mesh_instance): each
     * object mesh is stored once, in object space, with its own quantized
     * 4-wide tree in wnodes; the top-level tree's instance leaves (PRIM_INST
     * refs) enter it. Per instance 8 float4 (inst_*): the object-to-world
     * rows m[0..11], the world-to-object rows minv[0..11] (pbrt Transform's
     * m and mInv), then (tree root, first object slot, first global id,
     * triangles) and (tree stack bound, 0, 0, 0) as ints. Per object slot:
     * obj_v 3 float4 (object-space p0, p1, p2; p0.w = the triangle's index
     * in its mesh), obj_info (vertex ids into obj_n / obj_uv, mesh). A
     * triangle is intersected and shaded in world space from its vertices
     * transformed exactly as pbrt's Transform does (Transform::operator()),
     * so every hit equals the hit of the instance flattened to world space. */
    const float4 *insts;
    const float4 *obj_v;
    const int4 *obj_info;
    const float4 *obj_n;  /* object vertex normals (xyz) */
    const float4 *obj_uv; /* object vertex uvs (xy) */
    const int4 *obj_mesh; /* per object mesh: material, light, has_n, has_uv */
    int n_inst;
    /* the emitting triangles of the mesh lights (PM_LIGHT_AREA_MESH), light
     * after light; a buffer of its own in HBM, never part of the blob: the LDS
     * modes budget their LDS for the scene, and a lane's search through a
     * light's cdf diverges, so it is read with plain vector loads (L2 / TCP
     * keep the small read-only table) */
    const LightTri *light_tris;
    /* textures (pm_texture.h), buffers of their own in HBM like light_tris, so
     * a small scene stays LDS-resident whatever its images' size: the records,
     * the texels (float4: rgb, 0) of every image, per material the index of
     * its Kd texture (-1: none), and per triangle storage slot its corners'
     * uvs, 2 float4 (uv0, uv1) (uv2, 0, 0). All null unless the committed
     * scene has a textured material: that selects the TEX instantiations of
     * the trace, eye and simple kernels; the others never read them */
    const TexRec *tex_recs;
    const float4 *texels;
    const int *mat_tex;
    const float4 *tri_uv;
    /* the physical specular model (pm_add_material_specular): 2 float4 per
     * material, (Kr.xyz, index) (Kt.xyz, flag as int bits: 1 = the material
     * uses the model, 0 = it keeps the reference's), a buffer of its own in
     * HBM like the textures'. Null unless the committed scene has such a
     * material: that selects the SPEC instantiations of the trace and eye
     * kernels, which also hold the texture code; mat_tex is then non-null too
     * (all -1 in a scene without textures) */
    const float4 *mat_spec;
    /* all arrays above but light_tris, the textures' and mat_spec are 16-B aligned sections of one blob in HBM */
    const char *blob;
    uint32_t blob_bytes;
    uint32_t lds_bytes; /* = blob_bytes when the blob fits LDS_SCENE_MAX (LDS-resident mode), else 0 */
};

/* SceneMode, mode_lds: pm_scene_pod.h */

struct Ray { v3 o, d; float tmin, tmax; };

struct Hit {
    uint32_t ref;   /* prim ref of the winner */
    uint32_t gid;   /* global id (tie-break) */
    float t, beta, gamma;
};

/* The scene as a kernel sees it. LDS=true: the whole blob is copied into
 * `lds` by the block (every thread calls; __syncthreads() before use) and
 * every pointer is rebased into it. The rebased pointers derive from a
 * __shared__ array, so the compiler emits ds_read (not flat) loads. */
template <bool LDS>
PMD SceneDev scene_view(const SceneDev &S, uint4 *lds, int tid, int nthreads) {
    if (!LDS) return S;
    const uint4 *src = reinterpret_cast<const uint4 *>(S.blob);
    for (int i = tid; i < (int)(S.lds_bytes / 16); i += nthreads) lds[i] = src[i];
    SceneDev V = S;
    const char *b = reinterpret_cast<const char *>(lds);
#define PM_REBASE(f) V.f = reinterpret_cast<decltype(V.f)>(b + (reinterpret_cast<const char *>(S.f) - S.blob))
    PM_REBASE(nodes); PM_REBASE(refs); PM_REBASE(tri_geo); PM_REBASE(tri_info); PM_REBASE(tri_id);
    PM_REBASE(tri_shade); PM_REBASE(norms); PM_REBASE(disks); PM_REBASE(spheres); PM_REBASE(materials);
    PM_REBASE(lights);
#undef PM_REBASE
    V.blob = b;
    return V;
}

/* ------------------------------------------------------------- census */
PMD unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

/* four census counters summed over the wave, one atomic each per wave (only
 * in counting launches, never in timed ones); every lane of the wave calls */
PMD void count4(unsigned long long *c, unsigned long long a, unsigned long long b, unsigned long long d,
                unsigned long long e) {
    a = wave_sum(a); b = wave_sum(b); d = wave_sum(d); e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&c[0], a); atomicAdd(&c[1], b); atomicAdd(&c[2], d); atomicAdd(&c[3], e);
    }
}

/* record index -> pixel of an 8x8-tile ordering */
PMD void rec_to_pixel(int64_t r, int W, int *px, int *py) {
    int64_t tile = r >> 6;
    int lane = (int)(r & 63);
    int tilesX = (W + 7) / 8;
    *px = (int)(tile % tilesX) * 8 + (lane & 7);
    *py = (int)(tile / tilesX) * 8 + (lane >> 3);
}

} // namespace pm
