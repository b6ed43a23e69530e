/*
 * pm_api.h — C-ABI of the MI355X photon-mapping renderer (libpmhip.so).
 *
 * This is the drop-in boundary. The reference exposes a C++ plugin surface to
 * pbrt-v2 (cuda_render/cudaapi.h:8-19 + class CudaRender : Renderer,
 * cuda_render/cudarender.h:22-91) whose implementation talks to OptiX. Here
 * that surface is kept by a thin C++ adapter (cuda-raytrace_amd/adapter/,
 * see INTEGRATION.md) that flattens pbrt objects into the POD calls below.
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns
 * an int status (PM_OK = 0) and never throws; the message of the last failure
 * is available from pm_last_error(). Caller-owned input arrays are copied
 * during the call. A context is single-threaded (like the reference's global
 * gContext, cudarender.cpp:14) and bound to one HIP device.
 *
 * Mapping to the reference (file:line of the function each entry replaces):
 *   pm_create / pm_destroy        CudaRenderInit        cudaapi.cpp:4-7, cudarender.cpp:17-36
 *   pm_add_material               CudaMaterial::createCudaMeteral  util/material/cudamaterial.cpp:8-21
 *   pm_add_trimesh                CudaTriangleMesh::setupGeometry  util/shape/cudatrianglemesh.cpp:16-73
 *   pm_add_sphere                 CudaSphere::setupTransform       util/shape/cudasphere.cpp:15-40
 *   pm_add_disk                   CudaDisk::setupGeometry          util/shape/cudadisk.cpp:15-45
 *   pm_add_light_point            CudaLight::setupLight<PointLight>        util/light/cudalight.cpp:16-24
 *   pm_add_light_disk             CudaLight::setupLight<DiffuseAreaLight>  util/light/cudalight.cpp:26-59
 *   pm_add_light_mesh             (new: the reference emits from disks only, cudalight.cpp:35-56)
 *   pm_add_light_distant          (new: pbrt-v2 DistantLight; the reference warns and skips it)
 *   pm_set_eye_rays               PbrtCamera::preLaunch (bRays, bRandom2D) util/camera/pbrtcamera.cpp:57-122
 *   pm_set_pinhole                (on-device eye rays for synthetic benches)
 *   pm_set_camera / pm_film       (new: pbrt-v2 PerspectiveCamera::GenerateRay, StratifiedSampler, ImageFilm)
 *   pm_commit                     CudaRender::Render → assembleNode (Sbvh build)  cudarender.cpp:38-75,112-123
 *   pm_render                     PhotonMappingRenderer::render    photon_mapping/photonmappingrenderer.cpp:31-45
 *   pm_eye_pass                   RaytracingPass                   photonmappingrenderer.cpp:108-139 (+ raytracing.cu)
 *   pm_trace_photons              PhotonTracingPass                photonmappingrenderer.cpp:204-226 (+ photontracing.cu)
 *   pm_build_photon_map           CreatePhotonMap                  photonmappingrenderer.cpp:150-180
 *   pm_gather                     PhotonGatheringPass              photonmappingrenderer.cpp:228-232 (+ gathering.cu:104-126)
 *   pm_final                      FinalGatheringPass               photonmappingrenderer.cpp:234-277 (+ gathering.cu:129-146)
 *   pm_render_simple              SimpleRenderer::render           simple_render/simplerender.cpp:18-103 (+ simplerender.cu)
 */
#ifndef PM_API_H
#define PM_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define PM_OK 0
#define PM_ERR_INVALID 1     /* bad argument / call order */
#define PM_ERR_HIP 2         /* HIP runtime failure (message has hipGetErrorString) */
#define PM_ERR_NO_PHOTONS 3  /* 0 valid photons: reference raises Severe, photonmappingrenderer.cpp:165-167 */
#define PM_ERR_NOMEM 4

/* ---- enums (values equal the reference's) ----------------------------- */
/* MaterialType, util/common.cu.h:61-63 */
#define PM_MATTE 0
#define PM_MIRROR 1
#define PM_GLASS 2
/* CudaLightDevice::LightType, util/common.cu.h:48 */
#define PM_LIGHT_POINT 1
#define PM_LIGHT_AREA_DISK 3
/* ours (the reference's enum ends at 3): a triangle mesh that emits, pm_add_light_mesh */
#define PM_LIGHT_AREA_MESH 4
/* ours too: pbrt-v2's distant light, pm_add_light_distant (5 is kept for a spot light) */
#define PM_LIGHT_DISTANT 6
/* RayTracingRecord flags, photon_mapping/photonmapping.h:25-26 (+ INVALID for padding) */
#define PM_REC_EXCEPTION 0x01u
#define PM_REC_MISS 0x02u
#define PM_REC_INVALID 0x04u
/* the eye ray hit the back of the shading normal: dot(ns, wo) < 0 with
 * wo = -ray.direction (RayTracingRecord::direction, photonmapping.h:18) —
 * what pbrt's Faceforward(nn, wo) needs in the kNN estimator */
#define PM_REC_BACKFACE 0x08u
/* gather structures */
#define PM_GATHER_GRID 0   /* hashed uniform grid of photon buckets (default, fastest) */
#define PM_GATHER_KDTREE 1 /* reference-layout kd-tree (CudaPhoton nodes, pbrt median split) */
/* multi-GPU photon exchange */
#define PM_EXCHANGE_REDUCE 0   /* local maps, per-record (M, L) reduce-scatter */
#define PM_EXCHANGE_ALLGATHER 1 /* all-gather photon slots, replicated map */
/* radiance estimators of the gather (pm_render_params::estimator) */
#define PM_ESTIMATOR_PPM 0 /* the reference's: fixed-radius query + progressive update (gathering.cu:17-146) */
#define PM_ESTIMATOR_KNN 1 /* pbrt-v2 PhotonIntegrator::LPhoton: k nearest photons, Simpson kernel */
#define PM_KNN_MAX 64      /* largest knn_lookup */
/* pm_render_params::light_source_index: photon paths start on every light,
 * each path on one light chosen by emitted power (the light selection table
 * below, pm_light_selection_cdf); any value >= 0 is the reference's single
 * light (photonmappingrenderer.cpp:211). Other negative values are invalid. */
#define PM_ALL_LIGHTS (-1)

/* ---- POD layouts shared with tests / other hosts ----------------------- */

/* Photon slot == kd-node, bit-for-bit the reference's CudaPhoton
 * (photon_mapping/photonmapping.h:32-41): word = hasLeftChild:1 | splitAxis:2
 * | rightChild:29 (LSB first). Before the tree is built bit 0 is the valid
 * bit (photonmapping.h:43-56). 40 bytes. */
typedef struct pm_photon {
    uint32_t bits;
    float p[3];
    float alpha[3];
    float wi[3];
} pm_photon;
#define PM_PHOTON_MAX_RIGHT_CHILD ((1u << 29) - 1u) /* photonmapping.h:41 */

/* Gather-point record (the subset of RayTracingRecord, photonmapping.h:7-24,
 * that the gather and final passes read). 64 bytes, AoS for exchange; the
 * device keeps it as SoA. Under PM_ESTIMATOR_KNN,
 * flux accumulates the per-pass sums, radius2 holds the last pass's r_k^2
 * (pbrt's shrunk maxDistSquared) and photon_count its number of photons
 * found. In a scene with textures, the flux of a record on a textured matte
 * is the sum with Kd = 1: the gathers run with f = 1 / pi for it, and
 * pm_final multiplies its indirect term by the record's albedo factor
 * (pm_download_record_albedo). dl already contains the texel. */
typedef struct pm_record {
    float pos[3];
    uint32_t flags;
    float ns[3];    /* normalized world shading normal */
    int32_t material;
    float flux[3];
    float radius2;
    float dl[3];    /* direct light */
    float photon_count;
} pm_record;

typedef struct pm_config {
    int device;          /* HIP device ordinal (n_devices == 0) */
    /* n_devices > 0: one context over devices[0 .. n_devices) of this node
     * (photon paths sharded by global id, RCCL all-gather of
     * the slots, interleaved 8-row bands per device). It takes the scene
     * calls, pm_render and pm_render_simple; the stage API needs one context
     * per device (one process per GPU, pmrender/dist.py). The reference is
     * single-context (cudarender.cpp:14), so this is new surface. */
    int n_devices;
    const int *devices;
    int reserved[4];
} pm_config;

/* Render parameters. Defaults (pm_default_params) are the reference's
 * hard-coded constants. */
typedef struct pm_render_params {
    float scene_epsilon;     /* 0.1   photonmappingrenderer.cpp:52 */
    float initial_radius2;   /* 4.0   raytracing.cu:123 */
    float ppm_alpha;         /* 0.7   gathering.cu:115 */
    int max_photon_count;    /* 4     photonmappingrenderer.cpp:183 (deposits per path) */
    int64_t paths_per_pass;  /* 262144 = 512*512, photonmappingrenderer.cpp:184-185,214 */
    int passes;              /* 1     photonmappingrenderer.cpp:38 */
    int light_source_index;  /* 0     photonmappingrenderer.cpp:211; PM_ALL_LIGHTS: every light */
    int max_specular_depth;  /* 10    raytracing.cu:98 (eye); build cap for photons (SURVEY App.B 5) */
    uint32_t rng_seed;       /* 777   util/random/cudarandom.h:15 */
    uint32_t light_rng_seed; /* 2047  (cudalight.cpp:530, commented-out light RNG seed) */
    int gather_structure;    /* PM_GATHER_GRID */
    /* PM_ESTIMATOR_PPM (default) or PM_ESTIMATOR_KNN: per pass, the knn_lookup
     * nearest photons with d^2 < initial_radius2 (pbrt's maxdist^2) give
     * sum_i Simpson(d_i^2, r_k^2) / r_k^2 * alpha_i over photons on the
     * viewer's side (pbrt photonmap.cpp LPhoton, diffuse branch); passes are
     * averaged. Photon-bucket gather only; not linear in the photon set, so
     * no partial/split gathers (multi-GPU: the all-gather exchange). */
    int estimator;
    int knn_lookup;          /* 50    pbrt PhotonIntegrator "nused" */
    int reserved[4];
} pm_render_params;

typedef struct pm_stats {
    int64_t paths_emitted;    /* total over passes */
    int64_t photons_valid;    /* last pass */
    int64_t gather_points;    /* active records (not MISS/EXC/INVALID) */
    int64_t nodes_visited;    /* last gather pass: photons tested (grid) or kd nodes visited */
    int64_t photons_in_radius;/* last gather pass: sum of M */
    double ms_eye, ms_trace, ms_build, ms_gather, ms_final; /* device time, summed over passes */
} pm_stats;

/* ---- lifecycle -------------------------------------------------------- */
void pm_default_params(pm_render_params *p);
int pm_create(void **ctx, const pm_config *cfg);
void pm_destroy(void *ctx);
const char *pm_last_error(void *ctx);
const char *pm_version(void);

/* ---- scene ------------------------------------------------------------ */
/* returns material id in *out_id. rgb = Kd (matte) / Kr (mirror, ignored by
 * the device as in cudamaterial.cu.h:101-105) / unused (glass). */
int pm_add_material(void *ctx, int type, const float rgb[3], int *out_id);
/* Textures for the Kd of a PM_MATTE (ours: the reference evaluates a texture
 * once, at a default point).
 * Surface (u, v) of a triangle hit (flattened or instanced mesh): b0 uv0 +
 * b1 uv1 + b2 uv2 from the hit's barycentrics, summed left to right in fp32; a
 * mesh without uvs has the corners (0,0) (1,0) (0,1) its shading frame uses.
 * A disk: pbrt-v2's u = phi / phiMax, v = 1 - (r - r_i) / (R - r_i). A (full)
 * sphere: pbrt-v2's u = phi / 2 pi, v = (theta - pi) / (0 - pi), theta =
 * acos(z / r) evaluated as atan2(sqrt(x^2 + y^2), z) in object space.
 *   image: w x h float RGB texels, row 0 at v = 0, a UVMapping2D mapping =
 *     (su, sv, du, dv): s = su u + du, t = sv v + dv,
 *     a wrap mode and an rgb scale. Level 0 only (pbrt-v2's
 *     MIPMap::triangle(0, s, t)), in fp32 without contraction:
 *       x = s w - 0.5, y = t h - 0.5 (each held to [-1e9, 1e9]),
 *       x0 = floorf(x), fx = x - x0, likewise y; the texels (x0, y0),
 *       (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) through the wrap mode
 *       (repeat: pbrt's Mod; clamp; black: 0 outside); blended as
 *       a + f (b - a) along x on both rows, then along y; times scale.
 *     Four equal texels return that texel (times scale) bit for bit.
 *   checker: pbrt-v2's Checkerboard2DTexture, dimension 2, aamode "none", with
 *     its own mapping: ((int)floorf(s) + (int)floorf(t)) % 2 == 0 picks
 *     operand 1, else operand 2.
 *   scale: operand 1 times operand 2 per channel.
 * An operand is rgbN when texN < 0, else the image (or constant) texture
 * texN; a checker or scale as an operand is refused, so nothing nests.
 * pm_add_material_textured makes a matte whose Kd is kd_tex; the photon
 * bounce, the direct light and pm_render_simple look the texel up at the hit.
 * PM_ERR_INVALID: a null pointer; w or h <= 0 or too many texels; a texel,
 * mapping, scale or colour value that is not finite; an unknown wrap mode; an
 * operand or texture id that is out of range or not an image; type !=
 * PM_MATTE. What needs no context is checked before the context is. */
#define PM_TEX_WRAP_REPEAT 0
#define PM_TEX_WRAP_BLACK 1
#define PM_TEX_WRAP_CLAMP 2
int pm_add_texture_image(void *ctx, const float *rgb, int w, int h, int wrap, const float mapping[4],
                         const float scale[3], int *out_tex);
int pm_add_texture_checker(void *ctx, const float mapping[4], int tex1, const float rgb1[3], int tex2,
                           const float rgb2[3], int *out_tex);
int pm_add_texture_scale(void *ctx, int tex1, const float rgb1[3], int tex2, const float rgb2[3], int *out_tex);
int pm_add_material_textured(void *ctx, int type, int kd_tex, int *out_id);
/* A specular material of the physical model (ours, opt-in: pm_add_material's
 * PM_MIRROR and PM_GLASS keep the reference's, which reflects 100 % and
 * refracts with a fixed 1.5, never reflecting, a path ending at total internal
 * reflection). type is PM_MIRROR (kt and index are not looked at) or PM_GLASS.
 * Everything is fp32 without contraction, in the order written, in the local
 * shading frame (wo = the direction back along the ray, cos = wo.z):
 *   mirror: wi = (-wo.x, -wo.y, wo.z), weight Kr, no random number.
 *   glass (pbrt-v2's FresnelDielectric(1, index), a specular reflection lobe
 *   Kr and a specular transmission lobe Kt):
 *     entering = wo.z > 0; ei = entering ? 1 : index; et = entering ? index : 1;
 *     eta = ei / et; sini2 = max(0, 1 - wo.z^2); sint2 = eta^2 sini2;
 *     sint2 >= 1 (total internal reflection): F = 1; else
 *       cost = sqrt(max(0, 1 - sint2)), ci = |wo.z|,
 *       rpar = (et ci - ei cost) / (et ci + ei cost),
 *       rper = (ei ci - et cost) / (ei ci + et cost), F = 0.5 (rpar^2 + rper^2);
 *     wr = F Kr, wt = (1 - F) Kt; both black: the path or chain ends.
 *     q = 1 if wt is black, 0 if wr is black, else F. One uniform u is always
 *     drawn; the step reflects iff u < q. For 0 < q < 1 its weight is Kr
 *     (reflected) or Kt (transmitted) exactly, the probability cancelling;
 *     otherwise wr or wt. Reflected wi: the mirror's; transmitted wi:
 *     (eta -wo.x, eta -wo.y, entering ? -cost : cost).
 * A photon path carries flux: alpha *= weight, with no index scaling (pbrt-v2
 * scales photons by (ei / et)^2 as well; pbrt-v3 corrected that, and we follow
 * v3). An eye chain carries radiance: it follows one branch per eye sample
 * (the camera's strata average the branches) and keeps an rgb throughput T,
 * T *= weight, and for a transmitted step T *= eta^2. The record then holds
 * dl = T L (emitted term included) and the albedo factor T x (the texel, or
 * 1) (pm_download_record_albedo). A chain that runs past max_specular_depth
 * or whose lobes are both black ends as PM_REC_EXCEPTION. pm_render_simple
 * follows no chain.
 * Random numbers, u = pmdm_u01(o[0]) of pmdm_philox4x32_10(counter; key):
 *   photon: (pm_index + nI, pass, spec, 0; rng_seed, 0): pm_index = path id x
 *     max_photon_count, nI the path's deposit counter at the hit (>= 1: a
 *     path's first hit makes it 1 before the draw, so no two paths share a
 *     counter), spec the path's specular count including this hit (>= 1; the
 *     Lambert bounce draws with 0 there).
 *   eye: (lo32(q), hi32(q), 2, depth; light_rng_seed, 0): q the sample or
 *     record index that keys the light samples, depth the chain's depth
 *     including this hit (the camera draws with word 2 = 1, the light samples
 *     with word 2 = 0).
 * Both models may share a scene. PM_ERR_INVALID: a null pointer, another
 * type, a colour component that is negative or not finite, an index that is
 * not finite or <= 0; checked before the context is. */
int pm_add_material_specular(void *ctx, int type, const float kr[3], const float kt[3], float index, int *out_id);
/* World-space mesh (pbrt TriangleMesh::p is already world space,
 * cudatrianglemesh.cpp:24-30). N and uv may be NULL. light_index = index of
 * the area light this shape emits for, -1 otherwise. */
int pm_add_trimesh(void *ctx, const float *P, int nverts, const int *indices, int ntris,
                   const float *N, const float *uv, int material, int light_index);
/* Object instancing (the reference's CudaObjectInstance, cudaapi.h:17 /
 * cudarender.cpp:88-103: an OptiX Transform over the instance's group).
 * pm_add_object_mesh stores a mesh once, in object space (arguments as
 * pm_add_trimesh), without rendering it; *out_object = its id.
 * pm_add_mesh_instance places it with a row-major affine object-to-world
 * matrix (last row 0 0 0 1, else PM_ERR_INVALID) and its inverse: the scene
 * gets a two-level tree (the object's own 4-wide tree, entered from the
 * top-level one), and every hit, shading frame and photon equals the hit of
 * the mesh flattened to world space with pbrt's Transform (points:
 * m[0]*x + m[1]*y + m[2]*z + m[3] per row, left to right; normals: the
 * transpose of w2o) and added with pm_add_trimesh at this call (global ids
 * in call order). */
int pm_add_object_mesh(void *ctx, const float *P, int nverts, const int *indices, int ntris,
                       const float *N, const float *uv, int material, int light_index, int *out_object);
int pm_add_mesh_instance(void *ctx, int object, const float o2w[16], const float w2o[16]);
/* Object-space sphere (cudasphere.cpp:15-40): row-major 4x4 matrices. */
int pm_add_sphere(void *ctx, float radius, const float o2w[16], const float w2o[16],
                  int material, int light_index);
/* World-space disk, already flattened as in cudadisk.cpp:24-43: o = O2W(0,0,h),
 * x = O2W(r,0,0), y = O2W(0,r,0), z = normalize(O2W(0,0,1)),
 * inner_norm = innerRadius/radius, phi_max in radians. */
int pm_add_disk(void *ctx, const float o[3], const float x[3], const float y[3],
                const float z[3], float inner_norm, float phi_max, int material, int light_index);
int pm_add_light_point(void *ctx, const float pos[3], const float intensity[3]);
/* Disk area light (cudalight.cpp:34-53): o centre, p1/p2 world radius vectors,
 * n normal, Le emitted radiance, area, n_samples shadow samples. */
int pm_add_light_disk(void *ctx, const float o[3], const float p1[3], const float p2[3],
                      const float n[3], const float Le[3], float area, int n_samples);
/* Triangle-mesh area light (pbrt's DiffuseAreaLight over a trianglemesh; the
 * reference has none). World-space vertices and indices as pm_add_trimesh;
 * only the emitter is created here: the caller adds the visible geometry with
 * pm_add_trimesh(..., light_index = *out_light) from the same arrays, as
 * pm_add_disk pairs with pm_add_light_disk. Triangle k emits from the side of
 * normalize(cross(p1 - p0, p2 - p0)), negated when reverse_orientation is set.
 * A point is drawn by area: per-triangle areas 0.5 |cross(p1 - p0, p2 - p0)|
 * in double from the float vertices, running sum in double in index order,
 * cdf[k] = (float)(sum[k] / sum[n - 1]), cdf[n - 1] = 1; the sample picks the
 * first k with cdf[k] > min(u, 1 - 2^-24) (a zero-area triangle is never picked), remaps u
 * into the bin and places the point with pbrt's UniformSampleTriangle as
 * p0 + b1 (p1 - p0) + (1 - b0 - b1) (p2 - p0). n_samples 2-D randoms are
 * registered as for the disk light. PM_ERR_INVALID: a null pointer,
 * ntris <= 0, an index out of range, a total area of 0 or not finite. */
int pm_add_light_mesh(void *ctx, const float *P, int nverts, const int *indices, int ntris,
                      int reverse_orientation, const float Le[3], int n_samples, int *out_light);
/* Distant light (pbrt-v2 DistantLight): radiance L arriving from the direction
 * to_light (any non-zero length: normalised in double, stored as float). A
 * delta light: one shadow sample per gather point, no 2-D light sample.
 * pm_commit computes the world sphere (PM_SCENE_WORLD_SPHERE):
 * centre C = the midpoint of the exact, unpadded bounds of all world-space
 * geometry (mesh vertices, instance boxes, disks, spheres), in double, rounded
 * to float; radius R = the distance from that float centre to the farthest
 * bound corner in double, rounded up to float. The light's record is then the
 * disk light's: centre (float)(C + R to_light), radius vectors (float)(R v1),
 * (float)(R v2) with (v1, v2) = CoordinateSystem(to_light), normal -to_light,
 * area (float)(pi R R), all evaluated in double.
 *   emission: the disk light's point for (lu1, lu2), o + x p1 + y p2 with
 *       (x, y) the concentric-disk map; direction -to_light = Ns; tmin =
 *       scene_epsilon; Le = L area and pdf = 1, i.e. L over the density
 *       1 / (pi R R), as the disk light carries its area
 *   direct light: uwi = -(-to_light (2 R)) (2 R as a stored float), pdf = 1,
 *       li = L; the shadow segment [0.001, 0.999] uwi leaves the world sphere
 *       from any point inside it
 * PM_ERR_INVALID here: a null pointer, a value that is not finite, a zero
 * direction (checked before the context is); at pm_commit: R = 0 or not
 * finite (the message names the light). */
int pm_add_light_distant(void *ctx, const float to_light[3], const float L[3], int *out_light);

/* The largest |component| of an eye-ray origin (2^20). Up to it every
 * traversal mode returns the same hit bit for bit for any finite eye ray
 * (tested to that bound, tests/test_ray_query_gpu.py); far beyond it an ulp
 * of the origin exceeds the triangles and the triangle test itself accepts
 * hits that lie in no box. Both calls below return PM_ERR_INVALID for an
 * origin beyond it and for a non-finite origin or direction. The guarantee
 * covers eye rays only, in scenes that themselves lie within the bound:
 * light positions (the origins of photon and shadow rays) and geometry are
 * not checked, and rays that start on surfaces or lights beyond 2^20 are
 * outside what was tested. */
#define PM_MAX_RAY_ORIGIN 1048576.0f

/* Eye samples. Either a pinhole camera evaluated on the device (records in
 * 8x8-pixel tile order, output in raster order) ... */
int pm_set_pinhole(void *ctx, const float eye[3], const float fwd[3], const float right[3],
                   const float up[3], int width, int height);
/* ... or host-generated rays in sampler order, as PbrtCamera::preLaunch
 * packs them (o.xyz, d.xyz per ray; rand2d = n2d float2 per ray, indexed
 * [ray][random2DStart + s], cudalight.cu.h:34-35). */
int pm_set_eye_rays(void *ctx, const float *rays, int64_t nrays, const float *rand2d, int n2d);

/* ... or a supersampled thin-lens camera with an on-device filtered film
 * (pbrt-v2's perspective camera, stratified sampler and ImageFilm).
 *
 * Sample raster: WS = width * xsamples, HS = height * ysamples; sample
 * (ix, iy) has index q = iy * WS + ix. After pm_set_camera the context
 * behaves as a pinhole context of size WS x HS: record count and order,
 * pm_record_pixel (it returns q), pm_final, the record views and the
 * multi-device bands all work on the sample raster.
 *
 * Ray of sample q, in fp32, no contraction, operations in this order:
 *   o = pmdm_philox4x32_10(lo32(q), hi32(q), 1, 0; key sample_seed, 0)
 *   ju, jv = pmdm_u01(o[0]), pmdm_u01(o[1]) with jitter != 0, else 0.5
 *   lu, lv = pmdm_u01(o[2]), pmdm_u01(o[3])
 *   ndc_x = 2 (ix + ju) / WS - 1,  ndc_y = 1 - 2 (iy + jv) / HS
 *   d0 = fwd + ndc_x right + ndc_y up
 *   lens_radius == 0: origin eye, direction normalize(d0) (with jitter off
 *     the pm_set_pinhole ray of a WS x HS image, bit for bit)
 *   lens_radius > 0: (cx, cy) = the concentric-disk map of (lu, lv),
 *     o' = eye + lens_radius (cx normalize(right) + cy normalize(up)),
 *     Pf = eye + d0 (focal_distance / |fwd|), direction normalize(Pf - o')
 *     (pbrt's PerspectiveCamera::GenerateRay in the world basis)
 *   film position, in pixels: fx = (ix + ju) / xsamples, fy = (iy + jv) / ysamples
 * The light samples of the eye pass are keyed by q as pm_set_pinhole keys
 * them by pixel.
 *
 * Film (pbrt-v2 ImageFilm restated as a gather; deterministic, no atomics):
 * with dx = fx - 0.5, dy = fy - 0.5 sample q contributes to pixel (x, y) iff
 * ceilf(dx - xwidth) <= x <= floorf(dx + xwidth) and likewise in y, with
 * weight table[jy * 16 + jx], jx = min((int)floorf(fabsf((x - dx) * (1 /
 * xwidth) * 16)), 15), jy likewise. A pixel sums w L per channel and w in
 * fp32 in ascending q; sum w == 0 gives black, else each channel is
 * max(0, sum / sum w), one IEEE division per channel. */
#define PM_FILTER_NONE 0      /* no film: outputs are the sample raster */
#define PM_FILTER_BOX 1
#define PM_FILTER_TRIANGLE 2
#define PM_FILTER_GAUSSIAN 3  /* a = alpha */
#define PM_FILTER_MITCHELL 4  /* a = B, b = C */
#define PM_FILM_TABLE 16      /* pbrt ImageFilm's FILTER_TABLE_SIZE */
typedef struct pm_filter { int type; float xwidth, ywidth, a, b; } pm_filter;
typedef struct pm_camera {
    float eye[3], fwd[3], right[3], up[3];  /* as pm_set_pinhole */
    int width, height;                      /* image pixels */
    int xsamples, ysamples;                 /* strata per pixel, 1..8 each */
    int jitter;                             /* 0: stratum centres */
    float lens_radius, focal_distance;      /* 0: pinhole */
    uint32_t sample_seed;
    pm_filter filter;
    int reserved[4];
} pm_camera;
/* PM_ERR_INVALID: a null pointer, a non-finite vector, |eye| + lens_radius
 * beyond PM_MAX_RAY_ORIGIN, width or height <= 0, a sample count outside
 * 1..8, WS * HS >= 2^31, lens_radius < 0, lens_radius > 0 with
 * focal_distance <= 0, an unknown filter type, a real filter with a width
 * outside (0, 4] or with WS or HS above 2^20 (fp32 film positions). A multi-device context takes the call as well. */
int pm_set_camera(void *ctx, const pm_camera *cam);
/* The film as a stage: d_samples float3 x WS * HS in raster order (what
 * pm_final writes), d_image float3 x width * height. Needs a camera with a
 * real filter. pm_render and pm_render_simple run it themselves and write the
 * width x height image; with PM_FILTER_NONE they write the sample raster. */
int pm_film(void *ctx, const void *d_samples, void *d_image, void *stream);
/* Rays (o.xyz, d.xyz) and film positions (fx, fy) of samples [first, first +
 * count), computed on the device by the function the eye pass calls, into
 * host arrays; either may be null. A test hook like pm_scene_section. */
int pm_camera_rays(void *ctx, int64_t first, int64_t count, float *rays6, float *film_xy);
/* The same for eye pass `pass` of a resampled render (pm_eye_resample), by the
 * same device function: pm_camera_rays is pass = 0. PM_ERR_INVALID also for
 * pass < 0 (checked before the context is). */
int pm_camera_rays_pass(void *ctx, int pass, int64_t first, int64_t count, float *rays6, float *film_xy);
/* Host only: table[j * 16 + i] = (float)F((i + 0.5) / 16 * xwidth, (j + 0.5) /
 * 16 * ywidth), F in double from the float parameters: box 1; triangle
 * max(0, xw - |x|) max(0, yw - |y|); gaussian g(x, xw) g(y, yw) with g(t, w) =
 * max(0, exp(-a t^2) - exp(-a w^2)); mitchell M(x / xw) M(y / yw) with
 * t = |2 x|, M = ((-B - 6C) t^3 + (6B + 30C) t^2 + (-12B - 48C) t + (8B + 24C))
 * / 6 for t > 1, else ((12 - 9B - 6C) t^3 + (-18 + 12B + 6C) t^2 + (6 - 2B)) / 6. */
int pm_film_filter_table(const pm_filter *f, float out[PM_FILM_TABLE * PM_FILM_TABLE]);

/* Builds the BVH and uploads the scene. Must follow the last pm_add_*. */
int pm_commit(void *ctx);

/* ---- whole render (PhotonMappingRenderer::render) ---------------------- */
/* out_rgb: host float[3 * nrays] (rays mode) or float[3 * W * H] (pinhole,
 * raster order), NaN/negative/inf sanitized to black like
 * photonmappingrenderer.cpp:251-268. stats may be NULL. */
int pm_render(void *ctx, const pm_render_params *params, float *out_rgb, pm_stats *stats);

/* ---- resampled render: a fresh eye sample every pass ----------------------
 * Stochastic progressive photon mapping (Hachisuka and Jensen 2009): one
 * record per pixel keeps its statistics (flux, radius2, photon_count) while
 * its hit point moves under them, every pass, to a fresh sample of
 * pm_set_camera's jitter and lens. The lens and the pixel area are integrated
 * over the photon passes; memory and gather cost stay at one record per pixel.
 *
 * pm_eye_resample(pass) is eye pass `pass` of such a render:
 *   pass == 0: pm_eye_pass, bit for bit; the context's eye-sample count is 1.
 *   pass  > 0: a pending pm_reset_records is applied first. Sample q of pass k
 *     draws its camera randoms from pmdm_philox4x32_10(lo32(q), hi32(q), 1, k;
 *     sample_seed, 0) (pm_set_camera's ray with counter word 3 = k) and its
 *     light samples from (q, slot, 0, k; light_rng_seed, 0). Record r gets
 *     pos (the hit and this sample's flags: MISS, EXCEPTION, BACKFACE as in
 *     pm_eye_pass) and ns / material; dl += L, one fp32 add per channel, L
 *     this sample's direct light with the emitted term, (0, 0, 0) for a miss
 *     or an exception. flux, radius2 and photon_count are not written, padding
 *     records (PM_REC_INVALID) not touched. The count goes up by one.
 *   Both then drop the tile list and the grid plan and rebuild an active
 *   record view, as pm_eye_pass does. pm_eye_pass sets the count back to 1;
 *   pm_set_camera, pm_set_pinhole and pm_set_eye_rays to 0; pm_upload_records
 *   leaves it.
 * While the count is above 1, pm_final and pm_final_view write, for every
 * record that is not padding, whatever its last sample's flags,
 *   dl / (float)count + (flux (1 / pi)) (1 / (radius2 emitted))
 * per channel in that order (one IEEE division of dl; the second term 0 while
 * photon_count is 0), sanitised as always: a pixel whose last sample missed
 * keeps what its earlier samples gathered. A pixel whose pass-0 sample
 * missed keeps radius2 = 0 and shows direct light only.
 * PM_ERR_INVALID, with the reason in the message: null params or pass < 0
 * (checked before the context is); a multi-device context; no pm_set_camera,
 * or one with xsamples or ysamples != 1 or a filter other than PM_FILTER_NONE
 * (a record is a pixel; the passes are the samples); an estimator other than
 * PM_ESTIMATOR_PPM (the kNN final applies the Kd of the record's current
 * material); a scene with a textured material or one of
 * pm_add_material_specular (their factor is applied in pm_final, once per
 * record, which is wrong when the hit moves); pass > 0 before an eye pass or
 * resample wrote this camera's records. */
int pm_eye_resample(void *ctx, const pm_render_params *params, int pass, void *stream);
/* pm_render with pm_eye_resample(pass) in front of each pass's trace and the
 * final above with count = passes (for passes == 1 the image of pm_render).
 * out_rgb: float[3 * width * height], raster order. ms_eye is summed over the
 * passes, gather_points counts the last pass's active records. */
int pm_render_resampled(void *ctx, const pm_render_params *params, float *out_rgb, pm_stats *stats);

/* ---- final gathering: cosine-sampled gather rays, a kNN estimate at their hits
 * pbrt-v2's photon integrator does not show the photon map directly: at each
 * eye hit it shoots gather rays over the hemisphere and takes the density
 * estimate at their hits. The trace deposits a path's first diffuse hit only
 * behind a specular bounce, so the map holds indirect and caustic light; the
 * direct light at every hit comes from the eye pass's shading.
 *
 * Primary records are pm_eye_pass's; N = n_gather in 1..256. Secondary record
 * s = r N + j is gather ray j of primary record r. A record is active when it
 * has none of MISS, EXCEPTION, INVALID. All of it fp32 without contraction, in
 * the order written:
 *   rotation  o = pmdm_philox4x32_10(lo32(r), hi32(r), 3, pass; light_rng_seed, 0),
 *             ru = pmdm_u01(o[0]), rv = pmdm_u01(o[1])
 *   sample    a = ((float)j + 0.5f) / (float)N + ru, u1 = a - floorf(a);
 *             b = (float)bitreverse32(j) * 2^-32 + rv, u2 = b - floorf(b);
 *             both held to at most 1 - 2^-24 (a rotated Hammersley set)
 *   direction (dx, dy) = the concentric disk map of (u1, u2) (the disk light's);
 *             z = sqrtf(fmaxf(0, 1 - dx dx - dy dy)); n = the record's ns,
 *             negated under PM_REC_BACKFACE; (v1, v2) = pbrt's
 *             CoordinateSystem(n): |n.x| > |n.y| ? il = 1 / sqrtf(n.x n.x + n.z n.z),
 *             v1 = (-n.z il, 0, n.x il) : il = 1 / sqrtf(n.y n.y + n.z n.z),
 *             v1 = (0, n.z il, -n.y il); v2 = cross(n, v1);
 *             v = (dx v1 + dy v2) + z n, d = v * (1 / sqrtf(v.v)), the dot
 *             product summed x, y, z. A ray with z == 0 is not traced.
 *   ray       origin the record's pos, tmin = scene_epsilon, no far limit
 *   hit       found and shaded as pm_eye_pass does for a host-supplied ray
 *             (the traversal of the scene's mode, the reference model's mirror
 *             and glass chain up to max_specular_depth, the same flags, ns and
 *             material), with two differences: the 2-D sample of light slot t
 *             is (pmdm_u01(o[0]), pmdm_u01(o[1])) of pmdm_philox4x32_10(lo32(s),
 *             hi32(s), 0, pass; light_rng_seed, t), and the emitted term of a
 *             hit on a light is left out (the primary record's dl holds it).
 *             The secondary record starts with flux 0, photon_count 0, radius2
 *             = initial_radius2. A ray that is not traced, or of an inactive
 *             primary record, gives a MISS record.
 *   radiance  the kNN gather of PM_ESTIMATOR_KNN (knn_lookup, initial_radius2)
 *             over the secondary records against the built photon buckets,
 *             then pm_final's kNN form with emitted = paths_per_pass: Li_j,
 *             sanitised, 0 for an inactive record
 *   sum       A_r += Li_j per channel in ascending j. pass == 0 starts A from
 *             0 and the pass count P from 0; every call adds 1 to P.
 * pm_final_gather_resolve writes out_r = dl_r + Kd_r x (A_r / (float)(N P)),
 * one IEEE division per channel, Kd_r the materials table's for the record's
 * material (0 unless PM_MATTE), sanitised as pm_final does; an inactive record
 * gets what pm_final writes for it; raster order for pinhole and camera
 * contexts, else record order, [rec_begin, rec_begin + rec_count) as pm_final.
 * Secondary records are made and used in chunks of whole 64-record primary
 * tiles, at most 2^22 of them at a time (env PM_FG_CHUNK, for tests); the
 * result does not depend on the chunk. The primary records, the tile list,
 * the record view and the estimator the records are read under stay as they
 * were (pm_caustic_gather, below, is the one final-gather call that writes the
 * primary records).
 * PM_ERR_INVALID, with the reason in the message: null params, n_gather
 * outside 1..256, pass < 0 (these before the context is checked); a
 * multi-device context; gather_structure != PM_GATHER_GRID; no eye pass yet;
 * no built bucket map; records of pm_eye_resample; a scene with a textured
 * material or one of pm_add_material_specular (a secondary hit would need its
 * texel or throughput); pass > 0 with another n_gather or other records than
 * pass 0's; a resolve before any pass. */
#define PM_FG_MAX 256
int pm_final_gather_pass(void *ctx, const pm_render_params *params, int n_gather, int pass, void *stream);
int pm_final_gather_resolve(void *ctx, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream);
/* One eye pass; per pass trace, bucket build, pm_final_gather_pass(pass);
 * resolve; the film as pm_render applies it. The primary records' own gather
 * is not run. ms_gather carries the final-gather time (stages "fgrays": the
 * rays, "fgather": the kNN gather, final and sum over them), ms_final the
 * resolve. */
int pm_render_final_gather(void *ctx, const pm_render_params *params, int n_gather, float *out_rgb, pm_stats *stats);
/* Test hooks like pm_camera_rays: the rays (o.xyz, d.xyz) of secondary records
 * [first, first + count) by the device function pm_final_gather_pass calls,
 * with a zero direction for a ray that is not traced (all six zero for the
 * rays of an inactive record); and A (rgb) of the first n primary records. */
int pm_final_gather_rays(void *ctx, const pm_render_params *params, int n_gather, int pass, int64_t first,
                         int64_t count, float *rays6);
int pm_download_gather_sum(void *ctx, float *out_rgb, int64_t n);

/* ---- final gathering: the caustic map, looked up directly at the eye hit
 * The gather rays leave the emitted term out, so light -> specular chain ->
 * diffuse eye hit (L S+ D E) is in no term of dl + Kd x mean(Li). pbrt-v2's
 * photon integrator adds it from a map of its own: a kNN estimate at the eye
 * hit over the caustic photons.
 *
 * A deposit is a caustic photon when its path had at least one hit before it
 * and every earlier hit was specular (pbrt-v2's specularPath &&
 * nIntersections > 1). The slot index does not tell: slot k * mpc + 0 also
 * holds the second diffuse hit of an L D D path. Only the trace knows.
 *
 * pm_set_caustic_map(on != 0): off is the default and leaves every call as it
 * is without this section. On:
 *   trace    pm_trace_photons sets bit 1 of pm_photon::bits on each caustic
 *            photon; bit 0 stays the valid bit. Every other word it writes —
 *            slots, fused keys, ranks up to their order inside a cell, bucket
 *            counts — is the unmarked trace's, bit for bit.
 *   map      pm_build_caustic_map, after pm_build_photon_map on the buckets:
 *            a bucket set of its own over the slots with bit 1 set, on the
 *            built map's grid, each entry keeping its slot index.
 *   lookup   pm_caustic_gather(pass): the kNN gather of PM_ESTIMATOR_KNN
 *            (knn_lookup, initial_radius2) over the primary records against
 *            the caustic map. The records' flux, radius2 and photon_count are
 *            written as that estimator writes them, flux summed over the
 *            passes; pass == 0 starts from flux 0 and the pass count C from 0,
 *            every call adds 1 to C. This changes what final gathering leaves
 *            alone: with the switch off the primary records' flux, radius2 and
 *            photon_count stay as they were; with it on they are the caustic
 *            gather's, and the records read as PM_ESTIMATOR_KNN's afterwards.
 *   radiance Lc_r = pm_final's kNN form less dl_r with emitted =
 *            (float)(C x paths_per_pass): (flux_r * (1 / emitted)) * (Kd_r *
 *            (1 / pi)) per channel in fp32, the reciprocal correctly rounded,
 *            Kd_r as in the resolve; 0 for an inactive record; not sanitised
 *            on its own.
 *   resolve  with C == P > 0 pm_final_gather_resolve writes out_r = (dl_r +
 *            Lc_r) + Kd_r x (A_r / (float)(N P)), fp32 in the order written,
 *            one IEEE division per channel, sanitised as before. C == 0 writes
 *            the line above without Lc_r; any other C is refused.
 *   render   pm_render_final_gather runs pm_build_caustic_map and
 *            pm_caustic_gather after each pass's bucket build (stage
 *            "caustic", added to ms_gather).
 * Secondary hits keep the full map: L S+ D D E is indirect light.
 * PM_ERR_INVALID, with the reason in the message: a multi-device context;
 * pm_trace_photons under the switch with PM_GATHER_KDTREE (the kd-tree build
 * owns the bits word) or in a scene with a textured material or one of
 * pm_add_material_specular; pm_build_caustic_map with the switch off or no
 * bucket map built; pm_caustic_gather with null params or pass < 0 (before the
 * context is checked), the switch off, no caustic map, a map built for another
 * estimator or initial_radius2, what pm_final_gather_pass refuses of the
 * records and the scene, or pass > 0 that continues no pass 0. */
int pm_set_caustic_map(void *ctx, int on);
int pm_build_caustic_map(void *ctx, void *stream);
int pm_caustic_gather(void *ctx, const pm_render_params *params, int pass, void *stream);
/* Test hooks: the photons in the caustic map (-1: none built); the slot indices
 * of its first n entries in map order; the first n words of its cell_start
 * (cells + 1 words, the last one the count); Lc (rgb) of the first n primary
 * records. */
int64_t pm_caustic_map_count(void *ctx);
int pm_download_caustic_slots(void *ctx, uint32_t *out, int64_t n);
int pm_download_caustic_cell_start(void *ctx, uint32_t *out, int64_t n);
int pm_download_caustic_radiance(void *ctx, float *out_rgb, int64_t n);

/* ---- simple renderer (SimpleRenderer::render, simple_render/simplerender.cpp:18-103)
 * Direct light only: closest hit of each eye sample, one shadow-tested sample
 * per light (sample index 0, no pdf division, no emitted term,
 * simplerender.cu:40-72), miss = black; NaN / negative / inf sanitized like
 * simplerender.cpp:70-87. The reference sets scene_epsilon to 0.01 for it
 * (simplerender.cpp:23, PM_SIMPLE_SCENE_EPSILON); params->scene_epsilon is
 * used as given, and params->light_rng_seed feeds the pinhole mode's disk
 * samples. out_rgb as pm_render. */
#define PM_SIMPLE_SCENE_EPSILON 0.01f
int pm_render_simple(void *ctx, const pm_render_params *params, float *out_rgb, pm_stats *stats);
/* the same into a device buffer (float3 per output sample) on `stream` */
int pm_simple_pass(void *ctx, const pm_render_params *params, void *d_out, void *stream);

/* ---- stage-level API (device-resident state, explicit stream) ---------- */
/* `stream` is a hipStream_t (NULL = the context's own stream). */
int pm_eye_pass(void *ctx, const pm_render_params *params, void *stream);
/* Emits paths [path_begin, path_begin + path_count) of `pass` into the
 * context's slot buffer at slot offset (path - slot_path_base) * max_photon_count.
 * Global path ids keep the Halton / Philox streams identical for any sharding. */
int pm_trace_photons(void *ctx, const pm_render_params *params, int pass, int64_t path_begin,
                     int64_t path_count, int64_t slot_path_base, void *stream);
/* Builds the gather structure from the first n_slots slots (n_slots<=0: all). */
int pm_build_photon_map(void *ctx, const pm_render_params *params, int64_t n_slots, void *stream);
/* Fused range query + PPM update over all records ... */
int pm_gather(void *ctx, const pm_render_params *params, void *stream);
/* ... or over records [rec_begin, rec_begin + rec_count) (tile-owned gather). */
int pm_gather_range(void *ctx, const pm_render_params *params, int64_t rec_begin, int64_t rec_count,
                    void *stream);
/* Range query only: writes per record four int64 (M, L.r, L.g, L.b) to
 * d_partial (device pointer, 32 B x records of the view, see
 * pm_set_record_view); L is in the gather's exact fixed point, so partials of
 * photon shards sum to the 1-GPU result. */
int pm_gather_partial(void *ctx, const pm_render_params *params, void *d_partial, void *stream);
/* The "reduce" exchange's split partials: per view record an int32 photon
 * count M (d_count, n_view entries) and the flux sum as three int64 in the
 * gather's fixed point (d_flux, 3 x n_view, record-major). Summed over the
 * photon shards they equal a 1-GPU gather exactly. A pending pm_reset_records
 * is honoured (initial radius) and left to pm_ppm_update_split. */
int pm_gather_split(void *ctx, const pm_render_params *params, void *d_count, void *d_flux, void *stream);
/* PPM update (gathering.cu:115-125) from split partials summed over ranks:
 * radius2 and photon count of EVERY view record from the global counts
 * (d_count, n_view int32: all-reduced, so every rank updates every radius
 * itself and no radius exchange is needed), flux of view records
 * [v_begin, v_begin + v_count) from d_flux_chunk (3 int64 each:
 * reduce-scattered to the owner). Consumes a pending pm_reset_records. */
int pm_ppm_update_split(void *ctx, const pm_render_params *params, const void *d_count, const void *d_flux_chunk,
                        int64_t v_begin, int64_t v_count, void *stream);
/* The same update in two halves, so that the flux reduce-scatter of pass k
 * can still be in flight while pass k + 1 gathers (pmrender/dist.py):
 * pm_ppm_update_split_radius applies the global counts (d_count) to radius2
 * and photon count of every view record and writes each record's ratio
 * N'/(N + M) to d_ratio (n_view floats; < 0: nothing to apply), consuming a
 * pending pm_reset_records (a fresh record's flux is set to 0);
 * pm_ppm_update_split_flux later applies flux = (flux + L) * ratio to view
 * records [v_begin, v_begin + v_count) from d_flux_chunk. Together they are
 * pm_ppm_update_split bit for bit (gathering.cu:115-125 order of operations). */
int pm_ppm_update_split_radius(void *ctx, const pm_render_params *params, const void *d_count, void *d_ratio,
                               void *stream);
int pm_ppm_update_split_flux(void *ctx, const pm_render_params *params, const void *d_ratio,
                             const void *d_flux_chunk, int64_t v_begin, int64_t v_count, void *stream);
/* Record view of pm_gather_partial, pm_ppm_update, pm_get_radius2 and
 * pm_set_radius2 (their rec_begin / rec_count and buffers index the view):
 * active_only = 0 -> all records (default); 1 -> only active records (not
 * MISS / EXCEPTION / INVALID), compacted in record order — what a multi-GPU
 * exchange has to move (53% of the records at C2). The view is rebuilt by
 * every pm_eye_pass / pm_upload_records. *n_view = records in the view. */
int pm_set_record_view(void *ctx, int active_only, int64_t *n_view);
/* With the active view set: final radiance of view records [v_begin,
 * v_begin + v_count) into d_out (float3 each, view order) and the view's
 * record indices (uint32 x n_view) — records outside the view are black. */
int pm_final_view(void *ctx, double emitted, int64_t v_begin, int64_t v_count, void *d_out, void *stream);
int pm_record_view_list(void *ctx, void *d_out, void *stream);
/* the size of the active view as it stands (pm_set_record_view rebuilds it) */
int pm_record_view_size(void *ctx, int64_t *n_view);
/* PPM update of records [rec_begin, rec_begin+rec_count) from summed partials
 * (d_partial points at the partial of rec_begin). */
int pm_ppm_update(void *ctx, const pm_render_params *params, const void *d_partial,
                  int64_t rec_begin, int64_t rec_count, void *stream);
/* radius^2 of records [rec_begin, rec_begin+rec_count) to / from a device
 * float array (d_out[i] / d_in[i] is record rec_begin + i). The owner of a
 * record chunk publishes its updated radii so every rank queries the next
 * pass with the current radius (multi-GPU "reduce" exchange). */
int pm_get_radius2(void *ctx, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream);
int pm_set_radius2(void *ctx, const void *d_in, int64_t rec_begin, int64_t rec_count, void *stream);
/* Final radiance of records [rec_begin, rec_begin+rec_count) into the device
 * buffer d_out (float3 per record, RECORD order) — emitted = total paths. */
int pm_final(void *ctx, double emitted, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream);

/* ---- buffers, sizes, host transfer (tests / distributed glue) ---------- */
int64_t pm_num_records(void *ctx);
int pm_record_pixel(void *ctx, int64_t rec, int64_t *pixel); /* -1 if padding */
/* slot buffer capacity management; returns device pointer of the slots */
int pm_reserve_slots(void *ctx, int64_t n_slots, void **d_slots);
/* Use a caller-owned device buffer (n_slots pm_photon) as the slot buffer,
 * e.g. a torch tensor that an RCCL all-gather fills; NULL reverts to the
 * context's own buffer. The caller keeps it alive while the context uses it. */
int pm_set_slot_buffer(void *ctx, void *d_slots, int64_t n_slots);
int pm_download_slots(void *ctx, pm_photon *out, int64_t n);
int pm_upload_slots(void *ctx, const pm_photon *in, int64_t n);
int pm_download_records(void *ctx, pm_record *out, int64_t n);
int pm_upload_records(void *ctx, const pm_record *in, int64_t n); /* leaves the albedo factors below as they are */
/* Scenes with a textured material or one of pm_add_material_specular only
 * (else PM_ERR_INVALID): per record the rgb factor pm_final applies to the
 * indirect term, written by pm_eye_pass: the texel at a textured matte hit,
 * (1, 1, 1) on any other surface (whose Kd the gather already applied), times
 * the throughput T of the record's specular chain (pm_add_material_specular);
 * 0 for an inactive record. Final radiance:
 * PPM dl + (factor flux) (1 / pi) / (radius2 emitted), kNN dl + flux / emitted
 * (Kd / pi factor). Upload takes n = pm_num_records values. */
int pm_download_record_albedo(void *ctx, float *out_rgb, int64_t n);
int pm_upload_record_albedo(void *ctx, const float *in_rgb, int64_t n);
/* kd-tree nodes of the last PM_GATHER_KDTREE build (reference layout) */
int64_t pm_kdtree_nodes(void *ctx);
int pm_download_kdtree(void *ctx, pm_photon *out, int64_t n);
/* counters of the last gather: [0] photons (grid) or kd nodes visited,
 * [1] photons in radius (sum of M), [2] bucket rows read (grid), [3] active records */
int pm_gather_counters(void *ctx, int64_t out[4]);
/* counters of the last pm_trace_photons with counting on: [0] rays traced,
 * [1] BVH nodes entered, [2] primitive intersection tests, [3] photons
 * deposited (the traffic census behind the trace roofline) */
int pm_trace_counters(void *ctx, int64_t out[4]);
/* the loaded scene as the traversal kernels see it: [0] triangles rendered
 * (an instanced mesh counted once per instance), [1] disks, [2] spheres,
 * [3] BVH nodes, [4] BVH depth, [5] traversal mode (0 BVH in HBM, 1 BVH in
 * LDS, 2 brute force over an LDS-sized scene, 3 two-level: top tree over
 * instance boxes + one tree per object mesh), [6] scene bytes.
 * [3] / [4] describe the tree the kernels traverse: with mode 0 that is the
 * 4-wide quantized BVH (its node count and its depth in 4-wide levels),
 * whichever builder made it (device PLOC for >= 65,536 primitives, else the
 * host SAH build collapsed); with mode 1 the binary SAH tree */
int pm_scene_info(void *ctx, int64_t out[7]);
/* diagnostics: one section of the committed scene as the kernels read it
 * (refs; per storage slot the triangle records geo 48 B, shade 32 B, id,
 * info 16 B; the quantized wide nodes, 64 B 4-wide or 128 B 8-wide). *bytes = its
 * size; out may be null to query it, else max_bytes must hold it. Lets a
 * test compare the device-built tree with its host restatement. */
#define PM_SCENE_REFS 0
#define PM_SCENE_TRI_GEO 1
#define PM_SCENE_TRI_SHADE 2
#define PM_SCENE_TRI_ID 3
#define PM_SCENE_TRI_INFO 4
#define PM_SCENE_BVH4 5
#define PM_SCENE_INSTANCES 6 /* 128 B per instance (pm_device.h SceneDev::insts) */
#define PM_SCENE_OBJ_TRIS 7  /* 48 B per stored object triangle (object-space p0, p1, p2) */
/* 64 B per emitting triangle, mesh lights in light order: (p0, cdf[k]) (p1 - p0, 0)
 * (p2 - p0, 0) (emitting-side unit normal, 0); pm_device.h SceneDev::light_tris */
#define PM_SCENE_LIGHT_TRIS 8
/* 4 B per light: the light selection table cdf[l] (float) of PM_ALL_LIGHTS,
 * pm_light_selection_cdf over the scene's lights as pm_commit calls it (all
 * zero when that call fails: the scene emits nothing) */
#define PM_SCENE_LIGHT_CDF 9
/* 16 B, host values: the world sphere of the last pm_commit, centre x y z and
 * radius (float), as pm_add_light_distant states it */
#define PM_SCENE_WORLD_SPHERE 10
/* textured scenes (else empty): the texture records, 128 B each (pm_scene_pod.h
 * TexRec: kind, the checkerboard's mapping, two operands of 48 B: rgb or
 * scale, first texel or -1, w, h, wrap, 0, the image's mapping), and per
 * material the int index of its Kd texture (-1: none) */
#define PM_SCENE_TEXTURES 11
#define PM_SCENE_MAT_TEX 12
/* scenes with a material of pm_add_material_specular (else empty): 32 B per
 * material, (Kr rgb, index) (Kt rgb, 1 as int bits) for such a material (a
 * mirror's Kt and index are stored as 0), all zero for any other */
#define PM_SCENE_MAT_SPEC 13
int pm_scene_section(void *ctx, int section, void *out, int64_t max_bytes, int64_t *bytes);
/* the current photon map (pm_build_photon_map; the reference's
 * CreatePhotonMap, photonmappingrenderer.cpp:150-180): [0] structure
 * (PM_GATHER_GRID / PM_GATHER_KDTREE, -1 none), [1] valid photons in it,
 * [2] slots it was built from, [3] grid cells (0 for the kd-tree) */
int pm_map_info(void *ctx, int64_t out[4]);
/* Test hooks: the photon buckets of the last pm_build_photon_map, read only.
 * Each waits for the context's stream first and returns PM_ERR_INVALID, with
 * a message that names the call, for a null context or pointer, a size that
 * is negative or beyond what is held, and while no map is built on the buckets
 * (PM_GATHER_GRID). With cells = dims[0] dims[1] dims[2] (pm_map_info [3]):
 *  pm_map_grid                 the grid: cells per axis, the origin (the scene
 *                              box's low corner) and the bits of the float32
 *                              1 / cell edge. A photon at p lies in cell
 *                              (cz dims[1] + cy) dims[0] + cx, c = floor((p -
 *                              origin) inv_cs) in float32, clamped to the grid.
 *  pm_download_map_cell_start  the first n <= cells + 1 words of cell_start:
 *                              cell k holds photons [cell_start[k],
 *                              cell_start[k + 1]); cell_start[cells] = valid
 *                              photons.
 *  pm_download_map_counters    the first n <= cells + 1 bucket counters; every
 *                              build's scan leaves them zero.
 *  pm_download_map_photons     the first n <= valid photons in map order:
 *                              ph_a 4 floats each (p.xyz, wi.x), ph_b 8 floats
 *                              each (alpha.rgb, wi.y | wi.z, the photon's slot
 *                              index as uint32 bits, 0, 0). */
int pm_map_grid(void *ctx, int32_t dims[3], float origin[3], uint32_t *inv_cs_bits);
int pm_download_map_cell_start(void *ctx, uint32_t *out, int64_t n);
int pm_download_map_counters(void *ctx, uint32_t *out, int64_t n);
int pm_download_map_photons(void *ctx, float *ph_a, float *ph_b, int64_t n);
/* Test hook: the tile list of the full-range tile gathers, built first if the
 * records changed since the last one (so it exists after pm_upload_records):
 * *n = its length, *sorted = 1 once a gather's measured costs reordered it, and
 * with out != NULL (room for max_n >= *n entries) the ids of the 64-record
 * tiles that hold an active record, ascending until sorted. Waits for the
 * device. PM_ERR_INVALID as above, and without records. */
int pm_download_tile_list(void *ctx, uint32_t *out, int64_t max_n, int64_t *n, int *sorted);
/* Phase profile of the trace kernel, summed over waves and launches since the
 * last reset: shader-clock cycles in [0] emission, [1] BVH traversal,
 * [2] shading + bounce + deposit, [3] compaction barrier, [4] state exchange,
 * [5] unused, [6] wave lifetime, [7] waves. All zero unless the library was
 * built with PROF=1 (lib/libpmhip_prof.so); a measurement hook, not used by
 * the render path. */
int pm_trace_profile(void *ctx, int64_t out[8], int reset);
/* enable/disable census counters in the trace and gather kernels (off by
 * default: costs an atomic per wave) */
int pm_set_counting(void *ctx, int enabled);
int pm_synchronize(void *ctx);
/* Stage timings measured with HIP events recorded on the stream the kernels
 * run on. Stage names: "eye", "trace", "build", "gather", "update", "final",
 * "reset", "film", "simple", "fgrays", "fgather". last = most recent launch; total = sum over launches since
 * pm_timing_reset (synchronizes on the last event only when read). */
int pm_last_kernel_ms(void *ctx, const char *name, double *ms);
/* Which stages record events: "all" (default), "" / NULL (none) or a comma
 * list ("gather"). Each timed stage boundary costs a few us of GPU idle
 * time, so a throughput run times only the stage it reports on. */
int pm_set_stage_timing(void *ctx, const char *stages);
int pm_timing_reset(void *ctx);
int pm_timing_total(void *ctx, const char *name, int64_t *count, double *total_ms);
/* Restores every active record to the eye pass's initial PPM state
 * (flux 0, photon_count 0, radius2 = initial_radius2). */
int pm_reset_records(void *ctx, const pm_render_params *params, void *stream);

/* Host-only (no device needed): the canonical pbrt-v2 KdTree over the valid
 * slots in the reference node layout, i.e. what CreatePhotonMap
 * (photonmappingrenderer.cpp:150-180) uploads. nodes_out holds >= nslots
 * entries; returns the node count (= valid photons). */
int64_t pm_kdtree_build_host(const pm_photon *slots, int64_t nslots, pm_photon *nodes_out);

/* Halton permutation of PermutedHalton(5, RNG(seed)) (28 uints), exposed for tests. */
int pm_halton_permutation(uint32_t seed, uint32_t out[28]);

/* Host-only: the light selection table of PM_ALL_LIGHTS (pbrt-v2's photon
 * shooter picks a light per path from a power cdf and divides the path weight
 * by the probability of the pick; the reference emits from light 0 only).
 * Light l has type types[l] (PM_LIGHT_*), colour le_rgb[3l .. 3l+2] (a point
 * light's intensity, an area light's emitted radiance Le) and area areas[l]
 * (disk: its area; mesh: its total area; ignored for a point light; distant:
 * the world disk's area pi R R). All in double, from the float inputs:
 *   y(c) = 0.212671 r + 0.715160 g + 0.072169 b     (pbrt's luminance, summed
 *                                                    left to right)
 *   w[l] = y(c) * (4 pi)         point light        (pbrt PointLight::Power)
 *   w[l] = y(c) * (pi * area)    disk or mesh light (DiffuseAreaLight::Power;
 *          also the mean of the path weight |cos| Le area / pdf that the
 *          emission produces with its uniform-hemisphere direction)
 *   w[l] = y(c) * area           distant light      (DistantLight::Power)
 * with pi = M_PI; a negative w[l] counts as 0. Running sum in double in light
 * order, cdf[l] = (float)(sum[l] / sum[n - 1]), cdf[n - 1] = 1 (the
 * pm_add_light_mesh convention). A path with selection sample u — dimension 5
 * of the permuted Halton sequence (base 11, table entries 17..27 of
 * pm_halton_permutation) at the path's first slot index, evaluated as the
 * other four dimensions are — starts on the first light l with
 * cdf[l] > min(u, 1 - 2^-24), so a light of weight 0 is never picked; its
 * weight is the single light's, divided last by the float
 * pmf[l] = cdf[l] - (l ? cdf[l - 1] : 0). Dimensions 1-4 and the bounce
 * stream are the single light's, so path p is otherwise the path p of
 * light_source_index = l. Returns PM_OK, or PM_ERR_INVALID for n <= 0, a null
 * pointer, an unknown type, or a total weight that is 0 or not finite. */
int pm_light_selection_cdf(const int *types, const float *le_rgb, const float *areas, int n, float *cdf_out);

#ifdef __cplusplus
}
#endif
#endif /* PM_API_H */
