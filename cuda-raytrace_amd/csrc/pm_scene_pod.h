/*
 * pm_scene_pod.h — the plain structs and constants of the committed scene
 * that both the kernels (pm_device.h, pm_shade.h, pm_kernels.h) and the
 * host-only scene assembly (pm_scene.h) read. A HIP translation unit includes it after
 * hip_runtime.h and gets HIP's float4 / int4; a plain C++ unit gets the two
 * stand-ins below, laid out the same (four 32-bit lanes x y z w, 16-B
 * aligned), so the structs have one layout on both sides. The two kinds of
 * unit share them in memory only: a function one calls in the other takes
 * no float4 / int4 parameter (pm_scene.h).
 */
#pragma once
#include <stdint.h>

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_H
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
#endif
static_assert(sizeof(float4) == 16 && alignof(float4) == 16 && sizeof(int4) == 16 && alignof(int4) == 16,
              "float4 / int4: four lanes, 16-B aligned");

namespace pm {

/* prim ref = (kind << 30) | index */
/* PRIM_INST: an object instance (pm_add_mesh_instance) in the top-level
 * tree; a hit on one of its triangles carries (PRIM_INST << 30) | the
 * object triangle's storage slot, and the triangle's global id */
enum : uint32_t { PRIM_TRI = 0u, PRIM_DISK = 1u, PRIM_SPHERE = 2u, PRIM_INST = 3u };

struct LightDev {      /* CudaLightDevice (common.cu.h:47-59), 80 B */
    float4 o_type;     /* o.xyz, type (int bits) */
    float4 p1_ns;      /* p1.xyz, nSample (int bits) */
    float4 p2_r2d;     /* p2.xyz, random2DStart (int bits) */
    float4 n_area;     /* normal.xyz, area */
    float4 le;         /* intensity.xyz, 0 */
    /* PM_LIGHT_AREA_MESH (ours) has no o / p1 / p2 / normal: o_type.x, .y
     * hold (int bits) the first entry and the entry count of its triangles
     * in SceneDev::light_tris, o_type.z its reverse_orientation flag;
     * n_area.w is the mesh's total area, the other lanes as above */
    /* PM_LIGHT_DISTANT (ours): the disk light's lanes for the world sphere's
     * disk, filled at commit (pm_scene.h finish_lights): o = C + R to_light,
     * p1 / p2 = R v1, R v2, normal = -to_light (set when the light is added,
     * the one lane a commit reads), n_area.w = pi R R, le.w = 2 R,
     * p2_r2d.w = 0, nSample = 1 */
};

/* one emitting triangle of a mesh light, 64 B (four 16-B loads per lane) */
struct LightTri {
    float4 p0_cdf;     /* p0.xyz, cdf[k] of the light's area distribution */
    float4 e1;         /* p1 - p0, 0 */
    float4 e2;         /* p2 - p0, 0 */
    float4 n;          /* unit normal of the emitting side, 0 */
};
static_assert(sizeof(LightDev) == 80 && sizeof(LightTri) == 64, "light records as the kernels load them");

/* Textures of a matte Kd (pm_add_texture_*, pm_api.h). One operand is a
 * constant rgb (texel0 < 0) or an image: w x h float4 texels (rgb, 0) from
 * texel0 of SceneDev::texels, row 0 at v = 0, its own UVMapping2D map =
 * (su, sv, du, dv), a wrap mode, and rgb = the image's scale. */
enum : int { TEX_SINGLE = 0, TEX_CHECKER = 1, TEX_SCALE = 2 };
enum : int { TEX_WRAP_REPEAT = 0, TEX_WRAP_BLACK = 1, TEX_WRAP_CLAMP = 2 };
struct TexOperand {    /* 48 B */
    float rgb[3];
    int texel0;
    int w, h, wrap, pad;
    float map[4];
};
/* kind TEX_SINGLE: op[0]; TEX_CHECKER: op[0] / op[1] picked through map (the
 * checkerboard's own mapping); TEX_SCALE: op[0] * op[1]. No nesting: an
 * operand is never a checkerboard or a scale, so there is no evaluation stack */
struct TexRec {        /* 128 B */
    int kind, pad[3];
    float map[4];
    TexOperand op[2];
};
static_assert(sizeof(TexOperand) == 48 && sizeof(TexRec) == 128, "texture records as the kernels load them");

/* Scenes up to this size are copied into each block's LDS and traversed from
 * there (Cornell C2: ~4 KB); larger ones are traversed from HBM/L2. */
constexpr uint32_t LDS_SCENE_MAX = 16384;
/* LDS scenes with at most this many primitives skip the BVH: every lane
 * tests every primitive (MODE_BRUTE) */
constexpr int BRUTE_MAX_PRIMS = 64;

/* how the kernels see the scene (template argument of the traversal kernels) */
enum SceneMode : int { MODE_GLOBAL = 0, MODE_LDS = 1, MODE_BRUTE = 2, MODE_INST = 3 };
/* MODE_INST: a MODE_GLOBAL scene with object instances (two-level 4-wide trees) */
constexpr bool mode_lds(int mode) { return mode == MODE_LDS || mode == MODE_BRUTE; }

constexpr int BVH_STACK_DEPTH = 48; /* LDS stack entries per lane (builder caps depth below it) */
constexpr int BVH_STACK = BVH_STACK_DEPTH; /* >= max BVH depth (builder enforces it) */
/* the 8-wide tree's exact stack bound (seven pushes per level) runs deeper:
 * its stacks hold up to 96 entries (k_trace_pool8 keeps PM_POOL_STACK of them
 * in LDS and spills the rest; the eye pass's LDS columns take the bound) */
constexpr int BVH8_STACK = 96;

} // namespace pm
