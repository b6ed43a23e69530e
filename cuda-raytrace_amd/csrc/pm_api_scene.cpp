/*
 * pm_api_scene.cpp — the scene half of the C-ABI: materials, textures,
 * meshes / instances / spheres / disks, every light, the eye rays, the
 * camera and its film table, and pm_commit: the device BVH build
 * (commit_gpu_bvh) or the host assembly of pm_scene.cpp, the upload and the
 * SceneDev the kernels read (fill_scene_dev). The arguments are checked, and
 * the records built, in the host-only pm_scene.cpp wherever no HIP call is
 * needed.
 */
#include "pm_ctx.h"

namespace {

template <class T>
int upload(Ctx *c, DevBuf &b, const std::vector<T> &v) {
    HIPCHK(c, b.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) HIPCHK(c, hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PM_OK;
}

struct TmpBuf : DevBuf {
    ~TmpBuf() { release(); }
};

/* the scene blob with the BVH built on the device: boxes from the host's
 * parallel pass uploaded, gpu_bvh_build writes the 4-wide nodes and refs in
 * place, the triangle records (computed on the host in triangle-id order
 * while the device builds) are uploaded and permuted into storage order.
 * built = false: the caller runs the host build (the device tree exceeded a
 * limit the traversal has, or the build failed — reported on stderr) */
int commit_gpu_bvh(Ctx *c, const std::vector<BuildPrim> &prims, const BuildOptions &opt, SceneLayout &L, bool &built) {
    built = false;
    const HostScene &hs = c->hs;
    const int64_t nt = (int64_t)hs.tris.size();
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const int n = (int)prims.size();
    GpuBvhIn in{};
    in.n = n;
    in.radius = opt.ploc_radius;
    ploc_morton_frame(prims, in.frame_lo, in.frame_scale);
    std::vector<float> geo(TRI_GEO_FLOATS * (size_t)nt), shade(TRI_SHADE_FLOATS * (size_t)nt);
    std::vector<int> info(TRI_INFO_INTS * (size_t)nt);
    struct Joiner {
        std::thread t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } records;
    records.t = std::thread([&] {
        parallel_for(nt, [&](int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; ++k) tri_record(hs, (uint32_t)k, &geo[TRI_GEO_FLOATS * k], &shade[TRI_SHADE_FLOATS * k], &info[TRI_INFO_INTS * k]);
        });
    });
    std::vector<float4> hb(2 * (size_t)n);
    parallel_for(n, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const BuildPrim &p = prims[i];
            hb[2 * i] = f4(p.lo[0], p.lo[1], p.lo[2], bits_f(p.ref));
            hb[2 * i + 1] = f4(p.hi[0], p.hi[1], p.hi[2], 0.f);
        }
    });
    TmpBuf d_box, d_tord, d_src;
    HIPCHK(c, d_box.ensure(hb.size() * sizeof(float4)));
    HIPCHK(c, hipMemcpy(d_box.p, hb.data(), hb.size() * sizeof(float4), hipMemcpyHostToDevice));
    in.box = d_box.as<float4>();
    /* the host assembly's layout; no binary tree (a placeholder), room
     * for the n - 1 nodes a 4-wide tree over n leaves can have. Never
     * LDS-resident: the LDS modes traverse the binary tree this path does not build */
    const std::vector<float4> norms = vertex_normals(hs);
    L = SceneLayout();
    count_sections(L, hs, n, nt);
    L.size[SEC_NODES] = NODE_PLACEHOLDER_BYTES;
    L.size[SEC_WNODES] = BVH4Q_NODE_BYTES * (size_t)(n - 1);
    plan_layout(L, true);
    HIPCHK(c, c->d_scene.ensure(L.bytes));
    char *base = c->d_scene.as<char>();
    HIPCHK(c, hipMemsetAsync(base + L.off[SEC_NODES], 0, L.size[SEC_NODES], c->stream));
    auto put = [&](SceneSection sec, const void *src) {
        return L.size[sec] ? hipMemcpyAsync(base + L.off[sec], src, L.size[sec], hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIPCHK(c, put(SEC_NORMS, norms.data()));
    HIPCHK(c, put(SEC_DISKS, hs.disks.data()));
    HIPCHK(c, put(SEC_SPHERES, hs.spheres.data()));
    HIPCHK(c, put(SEC_MATS, hs.materials.data()));
    HIPCHK(c, put(SEC_LIGHTS, hs.lights.data()));
    HIPCHK(c, d_tord.ensure(sizeof(uint32_t) * (size_t)std::max<int64_t>(nt, 1)));
    GpuBvhOut out;
    out.wnodes = reinterpret_cast<uint4 *>(base + L.off[SEC_WNODES]);
    out.refs = reinterpret_cast<uint32_t *>(base + L.off[SEC_REFS]);
    out.tri_order = d_tord.as<uint32_t>();
    out.max_nodes = n - 1;
    const double t_up = ms();
    const hipError_t e = gpu_bvh_build(in, out, c->stream);
    const double t_build = ms();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fprintf(stderr, "pm_commit: device BVH build failed (%s); host build\n", hipGetErrorString(e));
        return PM_OK;
    }
    if (out.max_stack > BVH_STACK || out.n_tris != nt) {
        fprintf(stderr, "pm_commit: device BVH stack bound %d (limit %d), %lld triangles; host build\n", out.max_stack,
                BVH_STACK, (long long)out.n_tris);
        return PM_OK;
    }
    records.t.join();
    const double t_rec = ms();
    HIPCHK(c, d_src.ensure((TRI_GEO_BYTES + TRI_SHADE_BYTES + TRI_INFO_BYTES) * (size_t)std::max<int64_t>(nt, 1)));
    float4 *src_geo = d_src.as<float4>(), *src_shade = reinterpret_cast<float4 *>(d_src.as<char>() + TRI_GEO_BYTES * (size_t)nt);
    int4 *src_info = reinterpret_cast<int4 *>(d_src.as<char>() + (TRI_GEO_BYTES + TRI_SHADE_BYTES) * (size_t)nt);
    HIPCHK(c, hipMemcpyAsync(src_geo, geo.data(), geo.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(src_shade, shade.data(), shade.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(src_info, info.data(), info.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_tri_permute(d_tord.as<uint32_t>(), nt, src_geo, src_shade, src_info,
                                 reinterpret_cast<float4 *>(base + L.off[SEC_GEO]),
                                 reinterpret_cast<float4 *>(base + L.off[SEC_SHADE]),
                                 reinterpret_cast<uint32_t *>(base + L.off[SEC_TID]),
                                 reinterpret_cast<int4 *>(base + L.off[SEC_INFO]),
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (opt.times)
        fprintf(stderr, "pm_commit: device build: boxes up %.1f ms, PLOC + collapse %.1f ms (%d rounds, %lld nodes, depth %d, "
                        "stack %d), records %.1f ms, permute %.1f ms\n", t_up, t_build - t_up, out.rounds,
                (long long)out.nodes, out.depth, out.max_stack, t_rec, ms());
    c->bvh_depth = out.depth;
    c->bvh4_nodes = out.nodes;
    c->bvh4_depth = out.depth;
    L.n_nodes = out.nodes;
    L.size[SEC_WNODES] = BVH4Q_NODE_BYTES * (size_t)out.nodes; /* the nodes in use */
    L.wide = 2;
    L.wide_stack = out.max_stack;
    built = true;
    return PM_OK;
}

} // namespace

/* the eye kernels' camera block (all of it the pinhole's when no camera is set) */
void eye_camera(const Ctx *c, EyeParams &E) {
    E.pinhole = c->pinhole; E.W = c->W; E.H = c->H; E.n2d = c->n2d;
    E.eye = make_float4(c->eye[0], c->eye[1], c->eye[2], 0); E.fwd = make_float4(c->fwd[0], c->fwd[1], c->fwd[2], 0);
    E.right = make_float4(c->right[0], c->right[1], c->right[2], 0); E.up = make_float4(c->up[0], c->up[1], c->up[2], 0);
    E.camera = c->camera;
    if (c->camera) {
        E.cam.xs = c->cam.xsamples; E.cam.ys = c->cam.ysamples; E.cam.jitter = c->cam.jitter != 0;
        E.cam.lens_radius = c->cam.lens_radius; E.cam.focal = c->cam.focal_distance; E.cam.seed = c->cam.sample_seed;
    }
}

extern "C" {

/* ------------------------------------------------------------------ scene */
int pm_add_material(void *ptr, int type, const float rgb[3], int *out_id) {
    GROUP_FWD(ptr, pm_add_material(sub, type, rgb, out_id));
    GETCTX(ptr);
    if (type != PM_MATTE && type != PM_MIRROR && type != PM_GLASS) FAIL(c, PM_ERR_INVALID, "bad material type %d", type);
    float r = rgb ? rgb[0] : 0.f, g = rgb ? rgb[1] : 0.f, b = rgb ? rgb[2] : 0.f;
    c->hs.materials.push_back(f4(r, g, b, ibits(type)));
    if (out_id) *out_id = (int)c->hs.materials.size() - 1;
    c->committed = false;
    return PM_OK;
}

/* textures: the arguments are checked, and the records built, in the
 * host-only unit (pm_scene.cpp); what needs no context is checked before the
 * context is looked at */
int pm_add_texture_image(void *ptr, const float *rgb, int w, int h, int wrap, const float mapping[4], const float scale[3],
                         int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_image: null pointer");
    if (int rc = check_texture_image(rgb, w, h, wrap, mapping, scale, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_image(sub, rgb, w, h, wrap, mapping, scale, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_image(c->hs, rgb, w, h, wrap, mapping, scale, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_texture_checker(void *ptr, const float mapping[4], int tex1, const float rgb1[3], int tex2, const float rgb2[3],
                           int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_checker: null pointer");
    if (int rc = check_texture_operands("pm_add_texture_checker", mapping, true, tex1, rgb1, tex2, rgb2, err))
        FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_checker(sub, mapping, tex1, rgb1, tex2, rgb2, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_checker(c->hs, mapping, tex1, rgb1, tex2, rgb2, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_texture_scale(void *ptr, int tex1, const float rgb1[3], int tex2, const float rgb2[3], int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_scale: null pointer");
    if (int rc = check_texture_operands("pm_add_texture_scale", nullptr, false, tex1, rgb1, tex2, rgb2, err))
        FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_scale(sub, tex1, rgb1, tex2, rgb2, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_scale(c->hs, tex1, rgb1, tex2, rgb2, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_material_textured(void *ptr, int type, int kd_tex, int *out_id) {
    std::string err;
    if (int rc = check_material_textured(type, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    if (!out_id) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_material_textured: null pointer");
    GROUP_FWD(ptr, pm_add_material_textured(sub, type, kd_tex, out_id));
    GETCTX(ptr);
    if (int rc = add_material_textured(c->hs, type, kd_tex, out_id, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_material_specular(void *ptr, int type, const float kr[3], const float kt[3], float index, int *out_id) {
    std::string err;
    if (int rc = check_material_specular(type, kr, kt, index, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    if (!out_id) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_material_specular: null pointer");
    GROUP_FWD(ptr, pm_add_material_specular(sub, type, kr, kt, index, out_id));
    GETCTX(ptr);
    if (int rc = add_material_specular(c->hs, type, kr, kt, index, out_id, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_trimesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, const float *N, const float *uv,
                   int material, int light) {
    GROUP_FWD(ptr, pm_add_trimesh(sub, P, nverts, idx, ntris, N, uv, material, light));
    GETCTX(ptr);
    if (!P || !idx || nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty or null mesh");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    if (c->hs.next_tri_id + ntris >= ((int64_t)1 << 31)) FAIL(c, PM_ERR_INVALID, "too many triangles (global ids reach 2^31)");
    int64_t base = (int64_t)c->hs.P.size() / 3;
    c->hs.P.insert(c->hs.P.end(), P, P + 3 * (size_t)nverts);
    if (N) c->hs.N.insert(c->hs.N.end(), N, N + 3 * (size_t)nverts);
    else c->hs.N.insert(c->hs.N.end(), 3 * (size_t)nverts, 0.f);
    if (uv) c->hs.UV.insert(c->hs.UV.end(), uv, uv + 2 * (size_t)nverts);
    else c->hs.UV.insert(c->hs.UV.end(), 2 * (size_t)nverts, 0.f);
    int mid = (int)c->hs.meshes.size();
    c->hs.meshes.push_back(HMesh{material, light, N != nullptr, uv != nullptr});
    for (int t = 0; t < ntris; ++t)
        c->hs.tris.push_back(HTri{{(int)(base + idx[3 * t]), (int)(base + idx[3 * t + 1]), (int)(base + idx[3 * t + 2])}, mid,
                               (uint32_t)c->hs.next_tri_id++});
    c->committed = false;
    return PM_OK;
}

int pm_add_object_mesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, const float *N,
                       const float *uv, int material, int light, int *out_object) {
    GROUP_FWD(ptr, pm_add_object_mesh(sub, P, nverts, idx, ntris, N, uv, material, light, out_object));
    GETCTX(ptr);
    if (!P || !idx || nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty or null object mesh");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    HObj o;
    o.P.assign(P, P + 3 * (size_t)nverts);
    if (N) o.N.assign(N, N + 3 * (size_t)nverts);
    if (uv) o.UV.assign(uv, uv + 2 * (size_t)nverts);
    o.idx.assign(idx, idx + 3 * (size_t)ntris);
    o.material = material; o.light = light; o.has_n = N != nullptr; o.has_uv = uv != nullptr;
    c->hs.objs.push_back(std::move(o));
    if (out_object) *out_object = (int)c->hs.objs.size() - 1;
    c->committed = false;
    return PM_OK;
}

int pm_add_mesh_instance(void *ptr, int object, const float o2w[16], const float w2o[16]) {
    GROUP_FWD(ptr, pm_add_mesh_instance(sub, object, o2w, w2o));
    GETCTX(ptr);
    if (object < 0 || object >= (int)c->hs.objs.size()) FAIL(c, PM_ERR_INVALID, "bad object id %d", object);
    if (!o2w || !w2o) FAIL(c, PM_ERR_INVALID, "null instance transform");
    if (o2w[12] != 0.f || o2w[13] != 0.f || o2w[14] != 0.f || o2w[15] != 1.f)
        FAIL(c, PM_ERR_INVALID, "instance transform is not affine (flatten it with pm_add_trimesh)");
    /* every instance takes global ids for all of its triangles (as the
     * flattened scene would): heavy instancing must not wrap them */
    const int64_t n_obj_tris = (int64_t)(c->hs.objs[object].idx.size() / 3);
    if (c->hs.next_tri_id + n_obj_tris >= ((int64_t)1 << 31))
        FAIL(c, PM_ERR_INVALID, "too many instanced triangles (global ids reach 2^31)");
    HInst in;
    in.obj = object;
    std::memcpy(in.m, o2w, sizeof in.m);
    std::memcpy(in.minv, w2o, sizeof in.minv);
    in.gid_base = (uint32_t)c->hs.next_tri_id;
    c->hs.next_tri_id += n_obj_tris;
    c->hs.insts.push_back(in);
    c->committed = false;
    return PM_OK;
}

int pm_add_sphere(void *ptr, float radius, const float o2w[16], const float w2o[16], int material, int light) {
    GROUP_FWD(ptr, pm_add_sphere(sub, radius, o2w, w2o, material, light));
    GETCTX(ptr);
    if (!o2w || !w2o || !(radius > 0.f)) FAIL(c, PM_ERR_INVALID, "bad sphere");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    c->hs.spheres.push_back(f4(w2o[0], w2o[1], w2o[2], w2o[3]));
    c->hs.spheres.push_back(f4(w2o[4], w2o[5], w2o[6], w2o[7]));
    c->hs.spheres.push_back(f4(w2o[8], w2o[9], w2o[10], w2o[11]));
    c->hs.spheres.push_back(f4(radius, ibits(material), ibits(light), ibits(0)));
    c->hs.sphere_o2w.insert(c->hs.sphere_o2w.end(), o2w, o2w + 16);
    c->committed = false;
    return PM_OK;
}

/* derived uniforms as cudadisk.cpp:24-43 computes them */
int pm_add_disk(void *ptr, const float o[3], const float x[3], const float y[3], const float z[3], float inner,
                float phimax, int material, int light) {
    GROUP_FWD(ptr, pm_add_disk(sub, o, x, y, z, inner, phimax, material, light));
    GETCTX(ptr);
    if (!o || !x || !y || !z) FAIL(c, PM_ERR_INVALID, "null disk vector");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    float inv_rx2 = 1.f / (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    float inv_ry2 = 1.f / (y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    float moffset = o[0] * z[0] + o[1] * z[1] + o[2] * z[2];
    c->hs.disks.push_back(f4(o[0], o[1], o[2], inner));
    c->hs.disks.push_back(f4(x[0], x[1], x[2], phimax));
    c->hs.disks.push_back(f4(y[0], y[1], y[2], moffset));
    c->hs.disks.push_back(f4(z[0], z[1], z[2], inv_rx2));
    c->hs.disks.push_back(f4(inv_ry2, ibits(material), ibits(light), ibits(0)));
    c->committed = false;
    return PM_OK;
}

int pm_add_light_point(void *ptr, const float pos[3], const float I[3]) {
    GROUP_FWD(ptr, pm_add_light_point(sub, pos, I));
    GETCTX(ptr);
    if (!pos || !I) FAIL(c, PM_ERR_INVALID, "null point light");
    LightDev L{};
    L.o_type = f4(pos[0], pos[1], pos[2], ibits(PM_LIGHT_POINT));
    L.p1_ns = f4(0, 0, 0, ibits(1)); /* nSample = 1, cudalight.cpp:22 */
    L.p2_r2d = f4(0, 0, 0, ibits(0));
    L.n_area = f4(0, 0, 0, 0);
    L.le = f4(I[0], I[1], I[2], 0);
    c->hs.lights.push_back(L);
    c->committed = false;
    return PM_OK;
}

int pm_add_light_disk(void *ptr, const float o[3], const float p1[3], const float p2[3], const float n[3],
                      const float Le[3], float area, int nsamples) {
    GROUP_FWD(ptr, pm_add_light_disk(sub, o, p1, p2, n, Le, area, nsamples));
    GETCTX(ptr);
    if (!o || !p1 || !p2 || !n || !Le) FAIL(c, PM_ERR_INVALID, "null disk light vector");
    int ns = std::max(1, nsamples);
    LightDev L{};
    L.o_type = f4(o[0], o[1], o[2], ibits(PM_LIGHT_AREA_DISK));
    L.p1_ns = f4(p1[0], p1[1], p1[2], ibits(ns));
    L.p2_r2d = f4(p2[0], p2[1], p2[2], ibits(c->rand2d_total)); /* CudaSample::Add2D offset */
    L.n_area = f4(n[0], n[1], n[2], area);
    L.le = f4(Le[0], Le[1], Le[2], 0);
    c->rand2d_total += ns;
    c->hs.lights.push_back(L);
    c->committed = false;
    return PM_OK;
}

/* the emission table of a mesh light, as pm_api.h states it (tests restate it) */
int pm_add_light_mesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, int reverse,
                      const float Le[3], int nsamples, int *out_light) {
    GROUP_FWD(ptr, pm_add_light_mesh(sub, P, nverts, idx, ntris, reverse, Le, nsamples, out_light));
    GETCTX(ptr);
    if (!P || !idx || !Le || !out_light) FAIL(c, PM_ERR_INVALID, "null mesh light argument");
    if (nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty mesh light");
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    if (c->hs.light_tris.size() + (size_t)ntris >= ((size_t)1 << 31)) FAIL(c, PM_ERR_INVALID, "too many emitting triangles");
    std::vector<LightTri> tris((size_t)ntris);
    std::vector<double> sum((size_t)ntris);
    double total = 0.0;
    for (int t = 0; t < ntris; ++t) {
        const float *p0 = P + 3 * (size_t)idx[3 * t], *p1 = P + 3 * (size_t)idx[3 * t + 1], *p2 = P + 3 * (size_t)idx[3 * t + 2];
        const double a[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
        const double b[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        total += 0.5 * len;
        sum[t] = total;
        /* a zero-area triangle is never sampled: its normal is left zero */
        const double inv = len > 0.0 ? (reverse ? -1.0 : 1.0) / len : 0.0;
        LightTri &T = tris[t];
        T.p0_cdf = f4(p0[0], p0[1], p0[2], 0.f);
        T.e1 = f4(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], 0.f);
        T.e2 = f4(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], 0.f);
        T.n = f4((float)(n[0] * inv), (float)(n[1] * inv), (float)(n[2] * inv), 0.f);
    }
    if (!(total > 0.0) || !std::isfinite(total) || !std::isfinite((float)total))
        FAIL(c, PM_ERR_INVALID, "mesh light area %g is zero or not finite", total);
    for (int t = 0; t < ntris; ++t) tris[t].p0_cdf.w = (float)(sum[t] / total);
    tris[ntris - 1].p0_cdf.w = 1.0f;
    const int ns = std::max(1, nsamples);
    LightDev L{};
    L.o_type = f4(ibits((int)c->hs.light_tris.size()), ibits(ntris), ibits(reverse ? 1 : 0), ibits(PM_LIGHT_AREA_MESH));
    L.p1_ns = f4(0, 0, 0, ibits(ns));
    L.p2_r2d = f4(0, 0, 0, ibits(c->rand2d_total)); /* CudaSample::Add2D offset, as the disk light */
    L.n_area = f4(0, 0, 0, (float)total);
    L.le = f4(Le[0], Le[1], Le[2], 0);
    c->rand2d_total += ns;
    c->hs.light_tris.insert(c->hs.light_tris.end(), tris.begin(), tris.end());
    c->hs.lights.push_back(L);
    *out_light = (int)c->hs.lights.size() - 1;
    c->committed = false;
    return PM_OK;
}

/* the record is made, and the parameters checked, in the host-only unit
 * (pm_scene.cpp), before the context is looked at */
int pm_add_light_distant(void *ptr, const float to_light[3], const float Lrgb[3], int *out_light) {
    LightDev L{};
    std::string err;
    if (!out_light) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_light_distant: null pointer");
    if (int rc = make_distant_light(to_light, Lrgb, L, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_light_distant(sub, to_light, Lrgb, out_light));
    GETCTX(ptr);
    c->hs.lights.push_back(L);
    *out_light = (int)c->hs.lights.size() - 1;
    c->committed = false;
    return PM_OK;
}

int pm_set_pinhole(void *ptr, const float eye[3], const float fwd[3], const float right[3], const float up[3], int W,
                   int H) {
    GROUP_FWD(ptr, pm_set_pinhole(sub, eye, fwd, right, up, W, H));
    GETCTX(ptr);
    if (W <= 0 || H <= 0 || !eye || !fwd || !right || !up) FAIL(c, PM_ERR_INVALID, "bad pinhole camera");
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(eye[a]) <= PM_MAX_RAY_ORIGIN) || !std::isfinite(fwd[a]) || !std::isfinite(right[a]) || !std::isfinite(up[a]))
            FAIL(c, PM_ERR_INVALID, "pinhole camera: eye beyond 2^20 or a non-finite vector");
    c->pinhole = 1; c->W = W; c->H = H; c->camera = 0; c->eye_samples = 0; c->fg_passes = 0;
    std::memcpy(c->eye, eye, 12); std::memcpy(c->fwd, fwd, 12);
    std::memcpy(c->right, right, 12); std::memcpy(c->up, up, 12);
    return PM_OK;
}

int pm_set_eye_rays(void *ptr, const float *rays, int64_t nrays, const float *rand2d, int n2d) {
    GROUP_FWD(ptr, pm_set_eye_rays(sub, rays, nrays, rand2d, n2d));
    GETCTX(ptr);
    if (!rays || nrays <= 0) FAIL(c, PM_ERR_INVALID, "no rays");
    /* the traversal modes agree bit for bit for finite rays with |o| <= 2^20 (pm_slab.h box_near) */
    for (int64_t i = 0; i < nrays; ++i)
        for (int a = 0; a < 3; ++a)
            if (!(fabsf(rays[6 * i + a]) <= PM_MAX_RAY_ORIGIN) || !std::isfinite(rays[6 * i + 3 + a]))
                FAIL(c, PM_ERR_INVALID, "ray %lld: origin beyond 2^20 or a non-finite component", (long long)i);
    c->pinhole = 0; c->camera = 0; c->eye_samples = 0; c->fg_passes = 0;
    c->nrays = nrays;
    c->rays.assign(rays, rays + 6 * nrays);
    c->n2d = (rand2d && n2d > 0) ? n2d : 0;
    if (c->n2d) c->rand2d.assign(rand2d, rand2d + (size_t)2 * n2d * nrays);
    else c->rand2d.clear();
    HIPCHK(c, c->d_rays.ensure(c->rays.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(c->d_rays.p, c->rays.data(), c->rays.size() * sizeof(float), hipMemcpyHostToDevice));
    if (c->n2d) {
        HIPCHK(c, c->d_rand2d.ensure(c->rand2d.size() * sizeof(float)));
        HIPCHK(c, hipMemcpy(c->d_rand2d.p, c->rand2d.data(), c->rand2d.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return PM_OK;
}

/* ---- camera + film (pm_api.h pm_set_camera) ------------------------------ */
int pm_film_filter_table(const pm_filter *f, float out[PM_FILM_TABLE * PM_FILM_TABLE]) {
    if (!f || !out) { g_last_error = "pm_film_filter_table: null pointer"; return PM_ERR_INVALID; }
    if (f->type < PM_FILTER_BOX || f->type > PM_FILTER_MITCHELL || !(f->xwidth > 0.f && f->xwidth <= 4.f) ||
        !(f->ywidth > 0.f && f->ywidth <= 4.f)) {
        g_last_error = "pm_film_filter_table: unknown filter type or a width outside (0, 4]";
        return PM_ERR_INVALID;
    }
    const double xw = f->xwidth, yw = f->ywidth, a = f->a, b = f->b;
    auto gauss = [&](double t, double w) { return std::max(0.0, std::exp(-a * t * t) - std::exp(-a * w * w)); };
    auto mitchell = [&](double x) { /* pbrt-v2 MitchellFilter::Mitchell1D, B = a, C = b */
        const double t = std::fabs(2.0 * x);
        if (t > 1.0)
            return ((-a - 6 * b) * t * t * t + (6 * a + 30 * b) * t * t + (-12 * a - 48 * b) * t + (8 * a + 24 * b)) / 6.0;
        return ((12 - 9 * a - 6 * b) * t * t * t + (-18 + 12 * a + 6 * b) * t * t + (6 - 2 * a)) / 6.0;
    };
    for (int j = 0; j < PM_FILM_TABLE; ++j)
        for (int i = 0; i < PM_FILM_TABLE; ++i) {
            const double x = (i + 0.5) / PM_FILM_TABLE * xw, y = (j + 0.5) / PM_FILM_TABLE * yw;
            double v = 1.0;
            switch (f->type) {
            case PM_FILTER_TRIANGLE: v = std::max(0.0, xw - std::fabs(x)) * std::max(0.0, yw - std::fabs(y)); break;
            case PM_FILTER_GAUSSIAN: v = gauss(x, xw) * gauss(y, yw); break;
            case PM_FILTER_MITCHELL: v = mitchell(x / xw) * mitchell(y / yw); break;
            default: break;
            }
            out[j * PM_FILM_TABLE + i] = (float)v;
        }
    return PM_OK;
}

int pm_set_camera(void *ptr, const pm_camera *cam) {
    GROUP_FWD(ptr, pm_set_camera(sub, cam));
    GETCTX(ptr);
    if (!cam) FAIL(c, PM_ERR_INVALID, "null camera");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cam->eye[a]) || !std::isfinite(cam->fwd[a]) || !std::isfinite(cam->right[a]) ||
            !std::isfinite(cam->up[a]))
            FAIL(c, PM_ERR_INVALID, "camera: a non-finite vector");
    if (cam->width <= 0 || cam->height <= 0) FAIL(c, PM_ERR_INVALID, "camera: bad image size");
    if (cam->xsamples < 1 || cam->xsamples > 8 || cam->ysamples < 1 || cam->ysamples > 8)
        FAIL(c, PM_ERR_INVALID, "camera: %d x %d samples per pixel (1..8 each)", cam->xsamples, cam->ysamples);
    const int64_t WS = (int64_t)cam->width * cam->xsamples, HS = (int64_t)cam->height * cam->ysamples;
    if (WS >= (1ll << 31) || HS >= (1ll << 31) || WS * HS >= (1ll << 31))
        FAIL(c, PM_ERR_INVALID, "camera: %lld x %lld samples (2^31 or more)", (long long)WS, (long long)HS);
    if (!(cam->lens_radius >= 0.f) || !std::isfinite(cam->lens_radius))
        FAIL(c, PM_ERR_INVALID, "camera: lens_radius must be >= 0");
    if (cam->lens_radius > 0.f && !(cam->focal_distance > 0.f && std::isfinite(cam->focal_distance)))
        FAIL(c, PM_ERR_INVALID, "camera: a lens needs a focal_distance > 0");
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(cam->eye[a]) + cam->lens_radius <= PM_MAX_RAY_ORIGIN))
            FAIL(c, PM_ERR_INVALID, "camera: eye + lens_radius beyond 2^20");
    const pm_filter &f = cam->filter;
    if (f.type < PM_FILTER_NONE || f.type > PM_FILTER_MITCHELL) FAIL(c, PM_ERR_INVALID, "camera: unknown filter type %d", f.type);
    float table[PM_FILM_TABLE * PM_FILM_TABLE];
    if (real_filter(f)) {
        /* film positions are fp32 pixel coordinates: beyond 2^20 samples per
         * axis they no longer resolve a stratum (and k_film's halo margin,
         * pm_film.hip film_halo, is sized for this bound) */
        if (WS > (1 << 20) || HS > (1 << 20))
            FAIL(c, PM_ERR_INVALID, "camera: a filmed raster of %lld x %lld samples (2^20 per axis at most)", (long long)WS, (long long)HS);
        if (!(f.xwidth > 0.f && f.xwidth <= 4.f) || !(f.ywidth > 0.f && f.ywidth <= 4.f))
            FAIL(c, PM_ERR_INVALID, "camera: filter width (%g, %g) outside (0, 4]", f.xwidth, f.ywidth);
        if (pm_film_filter_table(&f, table)) FAIL(c, PM_ERR_INVALID, "camera: bad filter");
        HIPCHK(c, c->d_film_table.ensure(sizeof(table)));
        HIPCHK(c, hipMemcpy(c->d_film_table.p, table, sizeof(table), hipMemcpyHostToDevice));
    }
    c->cam = *cam;
    c->camera = 1; c->pinhole = 1; c->W = (int)WS; c->H = (int)HS; c->eye_samples = 0; c->fg_passes = 0;
    std::memcpy(c->eye, cam->eye, 12); std::memcpy(c->fwd, cam->fwd, 12);
    std::memcpy(c->right, cam->right, 12); std::memcpy(c->up, cam->up, 12);
    return PM_OK;
}

int pm_camera_rays(void *ptr, int64_t first, int64_t count, float *rays6, float *film_xy) {
    return pm_camera_rays_pass(ptr, 0, first, count, rays6, film_xy);
}

int pm_camera_rays_pass(void *ptr, int pass, int64_t first, int64_t count, float *rays6, float *film_xy) {
    if (pass < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_camera_rays: pass %d is negative", pass);
    if (Group *g_ = group_of(ptr)) {
        (void)hipSetDevice(g_->subs[0]->device);
        const int rc_ = pm_camera_rays_pass(g_->subs[0], pass, first, count, rays6, film_xy);
        return rc_ ? group_fail(ptr, g_->subs[0], rc_) : PM_OK;
    }
    GETCTX(ptr);
    if (!c->camera) FAIL(c, PM_ERR_INVALID, "pm_camera_rays: no camera (pm_set_camera)");
    if (first < 0 || count < 0 || first + count > (int64_t)c->W * c->H) FAIL(c, PM_ERR_INVALID, "pm_camera_rays: bad sample range");
    if (count == 0) return PM_OK;
    EyeParams E{};
    eye_camera(c, E);
    E.pass = (uint32_t)pass;
    DevBuf d_r, d_f;
    int rc = PM_OK;
    hipError_t e = hipSuccess;
    if (rays6) e = d_r.ensure((size_t)count * 6 * sizeof(float));
    if (e == hipSuccess && film_xy) e = d_f.ensure((size_t)count * 2 * sizeof(float));
    if (e == hipSuccess) e = launch_camera_rays(E, first, count, d_r.as<float>(), d_f.as<float>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && rays6) e = hipMemcpy(rays6, d_r.p, (size_t)count * 6 * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && film_xy) e = hipMemcpy(film_xy, d_f.p, (size_t)count * 2 * sizeof(float), hipMemcpyDeviceToHost);
    d_r.release(); d_f.release();
    if (e != hipSuccess) { c->err = std::string("pm_camera_rays: ") + hipGetErrorString(e); g_last_error = c->err; rc = PM_ERR_HIP; }
    return rc;
}

/* SceneDev from the committed layout: every section pointer, the counts, the traversal mode and stack */
static void fill_scene_dev(Ctx *c) {
    const SceneLayout &L = c->L;
    const HostScene &hs = c->hs;
    SceneDev &S = c->S;
    const char *base = c->d_scene.as<char>();
    const int64_t ni = (int64_t)hs.insts.size();
    S.blob = base;
    S.blob_bytes = (uint32_t)std::min<size_t>(L.bytes, 0xffffffffu);
    S.lds_bytes = L.bytes <= LDS_SCENE_MAX ? (uint32_t)L.bytes : 0u;
    S.nodes = (const float4 *)(base + L.off[SEC_NODES]); S.refs = (const uint32_t *)(base + L.off[SEC_REFS]);
    S.tri_geo = (const float4 *)(base + L.off[SEC_GEO]); S.tri_shade = (const float4 *)(base + L.off[SEC_SHADE]);
    S.tri_id = (const uint32_t *)(base + L.off[SEC_TID]); S.tri_info = (const int4 *)(base + L.off[SEC_INFO]);
    S.norms = (const float4 *)(base + L.off[SEC_NORMS]); S.disks = (const float4 *)(base + L.off[SEC_DISKS]);
    S.spheres = (const float4 *)(base + L.off[SEC_SPHERES]); S.materials = (const float4 *)(base + L.off[SEC_MATS]);
    S.lights = (const LightDev *)(base + L.off[SEC_LIGHTS]);
    S.n_lights = (int)hs.lights.size(); S.n_nodes = (int)L.n_nodes;
    S.n_refs = (int)L.n_refs;
    S.n_tris = (int)L.n_tris; S.n_disks = (int)(hs.disks.size() / 5); S.n_spheres = (int)(hs.spheres.size() / 4);
    S.tri_geo_g = S.tri_geo; S.tri_id_g = S.tri_id;
    S.tri_pairs_g = L.id_order ? c->d_tripairs.as<float>() : nullptr;
    S.light_tris = c->d_light_tris.as<LightTri>();
    S.tex_recs = c->textured ? c->d_tex_recs.as<TexRec>() : nullptr;
    S.texels = c->textured ? c->d_texels.as<float4>() : nullptr;
    S.mat_tex = c->albedo() ? c->d_mat_tex.as<int>() : nullptr;
    S.mat_spec = c->specular ? c->d_mat_spec.as<float4>() : nullptr;
    S.tri_uv = c->textured ? c->d_tri_uv.as<float4>() : nullptr;
    S.n_inst = (int)ni;
    S.insts = ni ? (const float4 *)(base + L.off[SEC_INSTS]) : nullptr;
    S.obj_v = ni ? (const float4 *)(base + L.off[SEC_OBJV]) : nullptr;
    S.obj_info = ni ? (const int4 *)(base + L.off[SEC_OBJINFO]) : nullptr;
    S.obj_n = ni ? (const float4 *)(base + L.off[SEC_OBJN]) : nullptr;
    S.obj_uv = ni ? (const float4 *)(base + L.off[SEC_OBJUV]) : nullptr;
    S.obj_mesh = ni ? (const int4 *)(base + L.off[SEC_OBJMESH]) : nullptr;
    S.brute = (S.lds_bytes > 0 && L.id_order) ? 1 : 0;
    /* a push happens only when descending a level, so depth + 1 entries suffice;
     * sizing the LDS stack by the actual tree keeps occupancy VGPR-bound */
    S.stack_depth = std::min(BVH_STACK, std::max(2, c->bvh_depth + 2));
    S.wide = L.wide;
    S.wnodes = L.wide ? (const float4 *)(base + L.off[SEC_WNODES]) : nullptr;
    /* wide scenes traverse only the 4-wide tree (traverse() dispatches every
     * MODE_GLOBAL query to traverse4): its exact stack bound sizes the LDS
     * stacks, not the binary tree's depth — k_trace_pool's 256-thread blocks
     * then fit four per CU (its VGPR occupancy) instead of three */
    if (L.wide) S.stack_depth = std::min(L.wide == 3 ? BVH8_STACK : BVH_STACK, std::max(2, L.wide_stack + 1));
}

int pm_commit(void *ptr) {
    GROUP_FWD(ptr, pm_commit(sub));
    GETCTX(ptr);
    std::string err;
    int rc;
    if ((rc = validate_scene(c->hs, err))) FAIL(c, rc, "%s", err.c_str());
    const BuildOptions opt = build_options_from_env();
    const auto t_commit0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    std::vector<BuildPrim> prims;
    scene_boxes(c->hs, prims, c->bbox_lo, c->bbox_hi);
    /* the distant lights' records, before either builder copies the lights */
    if ((rc = finish_lights(c->hs, c->bbox_lo, c->bbox_hi, c->world_sphere, err))) FAIL(c, rc, "%s", err.c_str());

    bool built = false;
    c->textured = scene_textured(c->hs);
    c->specular = scene_specular(c->hs);
    std::vector<float4> tri_uv; /* textured scenes: SceneDev::tri_uv */
    if (c->hs.insts.empty() && !opt.bvh8 && gpu_bvh_wanted(opt, (int64_t)prims.size())) {
        if ((rc = commit_gpu_bvh(c, prims, opt, c->L, built))) return rc;
        if (opt.times && built) fprintf(stderr, "pm_commit: device build, total %.1f ms\n", since(t_commit0));
        if (built && c->textured) {
            /* the device chose the storage order: without instances a triangle's
             * global id (SEC_TID, per storage slot) is its index */
            std::vector<uint32_t> order((size_t)c->L.n_tris);
            HIPCHK(c, hipMemcpy(order.data(), c->d_scene.as<char>() + c->L.off[SEC_TID], order.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
            for (uint32_t t : order)
                if (t >= c->hs.tris.size()) FAIL(c, PM_ERR_INVALID, "device build: triangle id %u out of range", t);
            tri_uv = triangle_uvs(c->hs, order.data(), (int64_t)order.size());
        }
    }
    if (!built) {
        SceneBlob blob;
        if ((rc = assemble_scene(c->hs, prims, opt, t_commit0, blob, err))) FAIL(c, rc, "%s", err.c_str());
        const auto t_u0 = std::chrono::steady_clock::now();
        if ((rc = upload(c, c->d_scene, blob.bytes))) return rc;
        if (blob.layout.id_order && (rc = upload(c, c->d_tripairs, blob.tri_pairs))) return rc;
        if (opt.times) fprintf(stderr, "pm_commit: upload %.1f ms (%zu bytes), total %.1f ms\n", since(t_u0), blob.bytes.size(),
                               since(t_commit0));
        c->L = blob.layout;
        c->bvh_depth = blob.bvh_depth;
        if (blob.layout.wide) { c->bvh4_nodes = blob.bvh4_nodes; c->bvh4_depth = blob.bvh4_depth; }
        tri_uv.swap(blob.tri_uv);
    }
    if ((rc = upload(c, c->d_light_tris, c->hs.light_tris))) return rc;
    if (c->textured) {
        if ((rc = upload(c, c->d_tex_recs, c->hs.textures))) return rc;
        if ((rc = upload(c, c->d_texels, c->hs.texels))) return rc;
        if ((rc = upload(c, c->d_tri_uv, tri_uv))) return rc;
    }
    if (c->albedo() && (rc = upload(c, c->d_mat_tex, material_textures(c->hs)))) return rc;
    if (c->specular && (rc = upload(c, c->d_mat_spec, material_specular_table(c->hs)))) return rc;
    fill_scene_dev(c);

    if ((rc = light_summary(c->hs, c->lsum, err))) FAIL(c, rc, "%s", err.c_str());
    if ((rc = upload(c, c->d_light_cdf, c->lsum.cdf))) return rc;
    c->committed = true;
    return PM_OK;
}

} /* extern "C" */
