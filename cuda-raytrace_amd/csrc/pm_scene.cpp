/*
 * pm_scene.cpp — scene assembly on the host (pm_scene.h): primitive boxes,
 * triangle records, the blob layout, the host-built trees laid into the
 * blob, the light summary. Plain C++, compiled with -ffp-contract=off: the
 * triangle frames are part of the numerics contract.
 */
#include "pm_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>

namespace pm {

namespace {

int fail(std::string &err, const char *fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    err = b;
    return PM_ERR_INVALID;
}

std::chrono::steady_clock::time_point tnow() { return std::chrono::steady_clock::now(); }
double tms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

template <class T> size_t vbytes(const std::vector<T> &v) { return v.size() * sizeof(T); }

} // namespace

int validate_scene(HostScene &hs, std::string &err) {
    if (hs.lights.empty()) return fail(err, "scene has no lights");
    const int64_t nt = (int64_t)hs.tris.size(), nd = (int64_t)hs.disks.size() / 5, ns = (int64_t)hs.spheres.size() / 4;
    if (nt + nd + ns + (int64_t)hs.insts.size() == 0) return fail(err, "scene has no shapes");
    if (nt >= (1 << 30) || nd >= (1 << 30) || ns >= (1 << 30)) return fail(err, "too many primitives");
    const int64_t nt_ids = hs.next_tri_id;
    if (nt_ids + nd + ns >= (int64_t)1 << 31) return fail(err, "too many primitives");
    for (int64_t i = 0; i < nd; ++i) hs.disks[5 * i + 4].w = ibits((int)(nt_ids + i));
    for (int64_t i = 0; i < ns; ++i) hs.spheres[4 * i + 3].w = ibits((int)(nt_ids + nd + i));
    return PM_OK;
}

/* Normalized shading frame of one triangle: the same IEEE float operations
 * in the same order as the closest-hit program (cudatrianglemesh.cu:36-78,
 * then normalize as cudamaterial.cu.h:84-85), so the device reads values
 * bit-identical to computing them per hit. n = e1 x e0 as in tri_geo. */
void tri_frame(const float *p0, const float *p1, const float *p2, const float *UV, const int *v, const float *n,
               float *ns, float *dpdu) {
    float uv0x = 0.f, uv0y = 0.f, uv1x = 1.f, uv1y = 0.f, uv2x = 0.f, uv2y = 1.f;
    if (UV) {
        uv0x = UV[2 * v[0]]; uv0y = UV[2 * v[0] + 1];
        uv1x = UV[2 * v[1]]; uv1y = UV[2 * v[1] + 1];
        uv2x = UV[2 * v[2]]; uv2y = UV[2 * v[2] + 1];
    }
    const float du1 = uv0x - uv2x, du2 = uv1x - uv2x, dv1 = uv0y - uv2y, dv2 = uv1y - uv2y;
    const float determinant = du1 * dv2 - dv1 * du2;
    float d[3];
    if (determinant == 0.0f) {
        if (std::fabs(n[0]) > std::fabs(n[1])) {
            float invLen = 1.f / std::sqrt(n[0] * n[0] + n[2] * n[2]);
            d[0] = -n[2] * invLen; d[1] = 0.f; d[2] = n[0] * invLen;
        } else {
            float invLen = 1.f / std::sqrt(n[1] * n[1] + n[2] * n[2]);
            d[0] = 0.f; d[1] = n[2] * invLen; d[2] = n[1] * invLen;
        }
    } else {
        const float invdet = 1.f / determinant;
        for (int a = 0; a < 3; ++a) {
            float dp1 = p0[a] - p2[a], dp2 = p1[a] - p2[a];
            d[a] = (dv2 * dp1 - dv1 * dp2) * invdet;
        }
    }
    auto normalize3 = [](const float *x, float *out) {
        float inv = 1.0f / std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        for (int a = 0; a < 3; ++a) out[a] = x[a] * inv;
    };
    normalize3(n, ns);
    normalize3(d, dpdu);
}

void tri_record(const HostScene &hs, uint32_t t, float *geo, float *shade, int *info) {
    const float *V = hs.P.data();
    const HTri &tr = hs.tris[t];
    const HMesh &m = hs.meshes[tr.mesh];
    const float *p0 = V + 3 * tr.v[0], *p1 = V + 3 * tr.v[1], *p2 = V + 3 * tr.v[2];
    float e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    float e1[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
    float n[3] = {e1[1] * e0[2] - e1[2] * e0[1], e1[2] * e0[0] - e1[0] * e0[2], e1[0] * e0[1] - e1[1] * e0[0]};
    const float g[TRI_GEO_FLOATS] = {p0[0], p0[1], p0[2], e0[0], e0[1], e0[2], e1[0], e1[1], e1[2], n[0], n[1], n[2]};
    std::memcpy(geo, g, sizeof g);
    float ns[3], dpdu[3];
    tri_frame(p0, p1, p2, m.has_uv ? &hs.UV[0] : nullptr, tr.v, n, ns, dpdu);
    const float s[TRI_SHADE_FLOATS] = {ns[0], ns[1], ns[2], bits_f((uint32_t)m.material | (m.has_n ? 0x80000000u : 0u)),
                        dpdu[0], dpdu[1], dpdu[2], bits_f((uint32_t)m.light)};
    std::memcpy(shade, s, sizeof s);
    const int i[TRI_INFO_INTS] = {tr.v[0], tr.v[1], tr.v[2], tr.mesh};
    std::memcpy(info, i, sizeof i);
}

std::vector<float4> vertex_normals(const HostScene &hs) {
    std::vector<float4> norms(hs.N.size() / 3);
    for (size_t i = 0; i < norms.size(); ++i) norms[i] = f4(hs.N[3 * i], hs.N[3 * i + 1], hs.N[3 * i + 2], 0.f);
    return norms;
}

BuildPrim make_box(const float lo[3], const float hi[3], uint32_t ref) {
    BuildPrim bp;
    for (int a = 0; a < 3; ++a) {
        float pad = 1e-4f * std::max(1.0f, std::max(fabsf(lo[a]), fabsf(hi[a])));
        bp.lo[a] = lo[a] - pad; bp.hi[a] = hi[a] + pad;
    }
    bp.ref = ref;
    return bp;
}

void scene_boxes(const HostScene &hs, std::vector<BuildPrim> &prims, float blo[3], float bhi[3]) {
    const int64_t nt = (int64_t)hs.tris.size(), nd = (int64_t)hs.disks.size() / 5, ns = (int64_t)hs.spheres.size() / 4,
                  ni = (int64_t)hs.insts.size();
    prims.assign(nt, BuildPrim());
    for (int a = 0; a < 3; ++a) { blo[a] = INFINITY; bhi[a] = -INFINITY; }
    auto add_box = [&](float lo[3], float hi[3], uint32_t ref) {
        for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], lo[a]); bhi[a] = std::max(bhi[a], hi[a]); }
        prims.push_back(make_box(lo, hi, ref));
    };
    const float *V = hs.P.data();
    { /* triangle boxes in parallel chunks; the scene box merged per chunk */
        std::mutex mu;
        parallel_for(nt, [&](int64_t t0, int64_t t1) {
            float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int64_t t = t0; t < t1; ++t) {
                const HTri &tr = hs.tris[t];
                float lo[3], hi[3];
                for (int a = 0; a < 3; ++a) {
                    float v0 = V[3 * tr.v[0] + a], v1 = V[3 * tr.v[1] + a], v2 = V[3 * tr.v[2] + a];
                    lo[a] = std::min(v0, std::min(v1, v2)); hi[a] = std::max(v0, std::max(v1, v2));
                    clo[a] = std::min(clo[a], lo[a]); chi[a] = std::max(chi[a], hi[a]);
                }
                prims[t] = make_box(lo, hi, (PRIM_TRI << 30) | (uint32_t)t);
            }
            std::lock_guard<std::mutex> g(mu);
            for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], clo[a]); bhi[a] = std::max(bhi[a], chi[a]); }
        });
    }
    for (int64_t i = 0; i < nd; ++i) {
        const float4 *d = &hs.disks[5 * i];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int sx = -1; sx <= 1; sx += 2)
            for (int sy = -1; sy <= 1; sy += 2) { /* cudadisk.cu:87-96 */
                float p[3] = {d[0].x + sx * d[1].x + sy * d[2].x, d[0].y + sx * d[1].y + sy * d[2].y,
                              d[0].z + sx * d[1].z + sy * d[2].z};
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
            }
        add_box(lo, hi, (PRIM_DISK << 30) | (uint32_t)i);
    }
    for (int64_t i = 0; i < ns; ++i) {
        const float *m = &hs.sphere_o2w[16 * i];
        float r = hs.spheres[4 * i + 3].x;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 8; ++k) {
            float x = (k & 1) ? r : -r, y = (k & 2) ? r : -r, z = (k & 4) ? r : -r;
            float w[3] = {m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7],
                          m[8] * x + m[9] * y + m[10] * z + m[11]};
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], w[a]); hi[a] = std::max(hi[a], w[a]); }
        }
        add_box(lo, hi, (PRIM_SPHERE << 30) | (uint32_t)i);
    }
    /* instances: the box of the world vertices the device rebuilds */
    for (int64_t i = 0; i < ni; ++i) {
        const HInst &in = hs.insts[i];
        const HObj &o = hs.objs[in.obj];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int v : o.idx) {
            float w[3];
            inst_point_h(in.m, &o.P[3 * (size_t)v], w);
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], w[a]); hi[a] = std::max(hi[a], w[a]); }
        }
        add_box(lo, hi, (PRIM_INST << 30) | (uint32_t)i);
    }
}

/* ---------------------------------------------------------------- layout */
void count_sections(SceneLayout &L, const HostScene &hs, int64_t n_refs, int64_t n_tris) {
    L.size[SEC_REFS] = REF_BYTES * (size_t)n_refs;
    L.size[SEC_GEO] = TRI_GEO_BYTES * (size_t)n_tris;
    L.size[SEC_SHADE] = TRI_SHADE_BYTES * (size_t)n_tris;
    L.size[SEC_TID] = TRI_ID_BYTES * (size_t)n_tris;
    L.size[SEC_INFO] = TRI_INFO_BYTES * (size_t)n_tris;
    L.size[SEC_NORMS] = (hs.N.size() / 3) * sizeof(float4);
    L.size[SEC_DISKS] = vbytes(hs.disks);
    L.size[SEC_SPHERES] = vbytes(hs.spheres);
    L.size[SEC_MATS] = vbytes(hs.materials);
    L.size[SEC_LIGHTS] = vbytes(hs.lights);
    L.n_refs = n_refs;
    L.n_tris = n_tris;
}

static_assert(LDS_SCENE_MAX % 16 == 0, "a blob of 16-B sections is compared with it");
void plan_layout(SceneLayout &L, bool never_lds) {
    size_t end = 0;
    for (int s = 0; s < SEC_COUNT; ++s) {
        L.off[s] = (end + 15) & ~(size_t)15;
        end = L.off[s] + L.size[s];
    }
    L.bytes = std::max<size_t>((end + 15) & ~(size_t)15, never_lds ? (size_t)LDS_SCENE_MAX + 16 : 16);
}

/* --------------------------------------------------------- build options */
BuildOptions build_options_from_env() {
    BuildOptions o;
    /* env PM_BVH_BUILD: "gpu" (the device PLOC build, pm_bvh_gpu.hip), "host"
     * (the binned-SAH host build), "ploc-host" (the device's algorithm on the
     * host: A/B of the tree quality and test oracle); unset or "auto": the
     * device for scenes of at least PM_BVH_GPU_MIN (65,536) primitives, whose
     * host build dominated the scene setup (C3: 0.28 s SAH of a 0.51 s commit) */
    if (const char *e = getenv("PM_BVH_BUILD")) o.build = e;
    if (const char *e = getenv("PM_BVH_GPU_MIN")) o.gpu_min = std::max<int64_t>(2, atoll(e));
    /* PLOC neighbour radius (env PM_PLOC_RADIUS, 1..32). C3 trace per 1M paths
     * on the host-built PLOC tree (same box): r 1 5.87 ms, 2 4.70, 3 4.50, 4
     * 4.58–4.63, 8 5.12, 16 5.73; the binned-SAH tree 4.50–4.51 */
    if (const char *e = getenv("PM_PLOC_RADIUS")) o.ploc_radius = std::max(1, std::min(32, atoi(e)));
    /* env PM_BVH4_BFS=1 renumbers the host's 4-wide tree breadth-first, the
     * order the device build produces (tests/test_bvh_gpu.py compares them) */
    if (const char *e = getenv("PM_BVH4_BFS")) { o.bfs_set = true; o.bfs = atoi(e) != 0; }
    /* env PM_BVH8=1 (round 6): scenes traversed from HBM get an 8-wide
     * quantized tree (host build; pm_build.h quantize_bvh8) instead of the
     * 4-wide one; instanced scenes keep 4-wide trees */
    if (const char *e = getenv("PM_BVH8")) o.bvh8 = atoi(e) != 0;
    /* env PM_COMMIT_TIMES=1: the build's phases on stderr (setup-time study) */
    o.times = getenv("PM_COMMIT_TIMES") != nullptr;
    return o;
}

bool gpu_bvh_wanted(const BuildOptions &opt, int64_t nprims) {
    const bool want = opt.build == "gpu" ? nprims >= 2 : (opt.build == "auto" && nprims >= opt.gpu_min);
    if (!want) return false;
    /* the breadth-first renumbering of the host tree is a host-path switch */
    return !opt.bfs_set;
}

/* -------------------------------------------------------- host assembly */
void relocate_bvh4(std::vector<uint32_t> &q, uint32_t base) {
    for (size_t nd = 0; nd + 16 <= q.size(); nd += 16)
        for (int k = 0; k < 4; ++k) {
            const int16_t cnt = (int16_t)((q[nd + 10 + k / 2] >> (16 * (k & 1))) & 0xffffu);
            if (cnt == 0) q[nd + 12 + k] += base;
        }
}

namespace {

/* the object meshes of an instanced scene (two-level trees) */
struct InstLayout {
    std::vector<uint32_t> qn;     /* every object's quantized 4-wide nodes, object 0 first (relocated by the caller) */
    std::vector<float4> insts;    /* 8 per instance (SceneDev::insts) */
    int max_stack = 0;            /* the deepest object tree's stack bound */
    std::vector<float4> objv, objn, objuv;
    std::vector<int4> objinfo, objmesh;
};

/* Each object mesh once: its triangles (object space) in the leaf order of
 * its own binned-SAH tree, collapsed to 4-wide and quantized (every leaf a
 * LEAF_TRIS run of object slots); the instance records point at them. */
int commit_objects(const HostScene &hs, InstLayout &IL, std::string &err) {
    std::vector<uint32_t> root(hs.objs.size()), slot0(hs.objs.size());
    std::vector<int> stack(hs.objs.size());
    uint32_t vbase = 0;
    for (size_t oi = 0; oi < hs.objs.size(); ++oi) {
        const HObj &o = hs.objs[oi];
        const int nt = (int)(o.idx.size() / 3);
        std::vector<BuildPrim> prims(nt);
        for (int t = 0; t < nt; ++t) {
            float lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                const float v0 = o.P[3 * o.idx[3 * t] + a], v1 = o.P[3 * o.idx[3 * t + 1] + a], v2 = o.P[3 * o.idx[3 * t + 2] + a];
                lo[a] = std::min(v0, std::min(v1, v2)); hi[a] = std::max(v0, std::max(v1, v2));
            }
            prims[t] = make_box(lo, hi, (PRIM_TRI << 30) | (uint32_t)t);
        }
        BvhOut bvh;
        build_bvh(prims, BVH_STACK - 2, bvh);
        Bvh4Out w;
        collapse_bvh4(bvh, 1, w);
        /* storage: the tree's leaf order, at global object slots */
        const uint32_t s0 = (uint32_t)(IL.objv.size() / 3);
        std::vector<uint32_t> refs(bvh.refs.size());
        for (size_t k = 0; k < bvh.refs.size(); ++k) {
            const uint32_t t = bvh.refs[k] & 0x3fffffffu;
            refs[k] = (PRIM_TRI << 30) | (s0 + (uint32_t)k);
            for (int q = 0; q < 3; ++q) {
                const float *v = &o.P[3 * (size_t)o.idx[3 * t + q]];
                IL.objv.push_back(f4(v[0], v[1], v[2], q == 0 ? ibits((int)t) : 0.f));
            }
            IL.objinfo.push_back(i4((int)vbase + o.idx[3 * t], (int)vbase + o.idx[3 * t + 1], (int)vbase + o.idx[3 * t + 2],
                                    (int)oi));
        }
        std::vector<uint32_t> qn;
        if (!quantize_bvh4(w.nodes, refs, qn)) return fail(err, "object mesh %zu: tree not codable", oi);
        for (size_t nd = 0; nd + 16 <= qn.size(); nd += 16)
            for (int k = 0; k < 4; ++k) {
                const int16_t cnt = (int16_t)((qn[nd + 10 + k / 2] >> (16 * (k & 1))) & 0xffffu);
                if (cnt > 0 && !(cnt & LEAF_TRIS)) return fail(err, "object mesh %zu: a leaf is not a triangle run", oi);
            }
        const uint32_t at = (uint32_t)(IL.qn.size() / 16);
        relocate_bvh4(qn, at);
        root[oi] = at;
        slot0[oi] = s0;
        stack[oi] = w.max_stack;
        IL.max_stack = std::max(IL.max_stack, w.max_stack);
        IL.qn.insert(IL.qn.end(), qn.begin(), qn.end());
        const int nv = (int)(o.P.size() / 3);
        for (int v = 0; v < nv; ++v) {
            IL.objn.push_back(o.has_n ? f4(o.N[3 * v], o.N[3 * v + 1], o.N[3 * v + 2], 0.f) : f4(0.f, 0.f, 0.f, 0.f));
            IL.objuv.push_back(o.has_uv ? f4(o.UV[2 * v], o.UV[2 * v + 1], 0.f, 0.f) : f4(0.f, 0.f, 0.f, 0.f));
        }
        vbase += (uint32_t)nv;
        IL.objmesh.push_back(i4(o.material, o.light, o.has_n ? 1 : 0, o.has_uv ? 1 : 0));
    }
    for (const HInst &in : hs.insts) {
        for (int r = 0; r < 3; ++r) IL.insts.push_back(f4(in.m[4 * r], in.m[4 * r + 1], in.m[4 * r + 2], in.m[4 * r + 3]));
        for (int r = 0; r < 3; ++r)
            IL.insts.push_back(f4(in.minv[4 * r], in.minv[4 * r + 1], in.minv[4 * r + 2], in.minv[4 * r + 3]));
        const int nt = (int)(hs.objs[in.obj].idx.size() / 3);
        IL.insts.push_back(f4(ibits((int)root[in.obj]), ibits((int)slot0[in.obj]), ibits((int)in.gid_base), ibits(nt)));
        /* blas_isect's (pm_traverse.h) box pad, 1e-5 (a (2 |o| + W) + k B): a = |w2o|, W
         * bounds the world extent by |o2w| B + |translation|, k = |o2w| |w2o|
         * (infinity norms of the linear parts), B the object's extent */
        double B = 0.0, nm = 0.0, ni_ = 0.0, tr = 0.0;
        const std::vector<float> &P = hs.objs[in.obj].P;
        for (float v : P) B = std::max(B, (double)fabsf(v));
        for (int r = 0; r < 3; ++r) {
            nm = std::max(nm, fabs(in.m[4 * r]) + fabs(in.m[4 * r + 1]) + fabs(in.m[4 * r + 2]));
            ni_ = std::max(ni_, fabs(in.minv[4 * r]) + fabs(in.minv[4 * r + 1]) + fabs(in.minv[4 * r + 2]));
            tr = std::max(tr, (double)fabsf(in.m[4 * r + 3]));
        }
        const double W = nm * B + tr;
        IL.insts.push_back(f4(ibits(stack[in.obj]), (float)(ni_ * 1.001), (float)((ni_ * W + nm * ni_ * B) * 1.001), 0.f));
    }
    return PM_OK;
}

} // namespace

int assemble_scene(const HostScene &hs, std::vector<BuildPrim> &prims, const BuildOptions &opt,
                   std::chrono::steady_clock::time_point t0, SceneBlob &out, std::string &err) {
    out = SceneBlob();
    SceneLayout &L = out.layout;
    const int64_t nt = (int64_t)hs.tris.size(), ni = (int64_t)hs.insts.size();
    const bool ptimes = opt.times;
    BvhOut bvh;
    BvhCost cost;
    const auto t_build0 = tnow();
    if (opt.build == "ploc-host" && prims.size() > 1) {
        PlocTree pt;
        build_ploc(prims, opt.ploc_radius, pt);
        ploc_to_bvh(prims, pt, bvh);
    } else {
        build_bvh(prims, BVH_STACK - 2, bvh, cost);
    }
    if (ptimes) fprintf(stderr, "pm_commit: %zu prims (boxes %.1f ms), host build %.1f ms\n", prims.size(),
                        tms(t0, t_build0), tms(t_build0, tnow()));
    out.bvh_depth = bvh.depth;
    if (bvh.depth >= BVH_STACK) return fail(err, "BVH too deep (%d)", bvh.depth);

    /* tiny LDS scenes skip the BVH (MODE_BRUTE). Their triangles are stored
     * in global-id order (pm_leaf.h brute_isect's tie-break relies on it), others in
     * leaf order. */
    const bool id_order = ni == 0 && (int64_t)bvh.refs.size() <= BRUTE_MAX_PRIMS;
    std::vector<uint32_t> tri_order; /* triangle ids in storage order */
    tri_order.reserve(nt);
    if (id_order) {
        for (int64_t t = 0; t < nt; ++t) tri_order.push_back((uint32_t)t);
    } else {
        for (uint32_t ref : bvh.refs)
            if ((ref >> 30) == PRIM_TRI) tri_order.push_back(ref & 0x3fffffffu);
    }
    std::vector<uint32_t> slot_of(nt);
    for (size_t k = 0; k < tri_order.size(); ++k) slot_of[tri_order[k]] = (uint32_t)k;
    parallel_for((int64_t)bvh.refs.size(), [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            uint32_t &ref = bvh.refs[i];
            if ((ref >> 30) == PRIM_TRI) ref = (PRIM_TRI << 30) | slot_of[ref & 0x3fffffffu];
        }
    });

    /* per-triangle precomputed (p0, e0, e1, n) for the intersector and the
     * normalized shading frame for hits (in parallel chunks of storage slots) */
    const int64_t nst = (int64_t)tri_order.size();
    std::vector<float> tri_geo(TRI_GEO_FLOATS * nst), tri_shade(TRI_SHADE_FLOATS * nst);
    std::vector<int> tri_info(TRI_INFO_INTS * nst);
    std::vector<uint32_t> tri_id(nst);
    parallel_for(nst, [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; ++k) {
            tri_record(hs, tri_order[k], &tri_geo[TRI_GEO_FLOATS * k], &tri_shade[TRI_SHADE_FLOATS * k], &tri_info[TRI_INFO_INTS * k]);
            tri_id[k] = hs.tris[tri_order[k]].gid;
        }
    });
    if (scene_textured(hs)) out.tri_uv = triangle_uvs(hs, tri_order.data(), nst);
    if (ptimes) fprintf(stderr, "pm_commit: triangle records done at %.1f ms\n", tms(t0, tnow()));
    const std::vector<float4> norms = vertex_normals(hs);

    count_sections(L, hs, (int64_t)bvh.refs.size(), nst);
    L.size[SEC_NODES] = vbytes(bvh.nodes);
    /* instances: each object mesh's own tree and object-space triangles */
    InstLayout IL;
    if (ni > 0) {
        if (int rc = commit_objects(hs, IL, err)) return rc;
        L.size[SEC_OBJV] = vbytes(IL.objv);
        L.size[SEC_OBJINFO] = vbytes(IL.objinfo);
        L.size[SEC_OBJN] = vbytes(IL.objn);
        L.size[SEC_OBJUV] = vbytes(IL.objuv);
        L.size[SEC_OBJMESH] = vbytes(IL.objmesh);
        out.obj_tris_stored = (int64_t)IL.objinfo.size();
    }
    plan_layout(L, false);
    const bool hbm = L.bytes > LDS_SCENE_MAX; /* without a wide tree the scene would still be traversed from HBM */
    /* scenes traversed from HBM also get the 4-wide BVH (half the dependent
     * node fetches per ray; binary leaves of one primitive);
     * instanced scenes always (their objects' trees are 4-wide) */
    std::vector<uint32_t> qn; /* the wide tree's quantized nodes */
    Bvh4Out w;                /* the collapsed tree the quantizer reads */
    if (opt.bvh8 && ni == 0 && hbm) {
        collapse_bvh8(bvh, 1, w);
        if (quantize_bvh8(w.nodes, bvh.refs, qn) && w.max_stack <= BVH8_STACK) {
            L.wide = 3;
            L.wide_stack = w.max_stack;
            out.bvh4_nodes = (int64_t)(qn.size() / 32);
            out.bvh4_depth = w.depth;
        }
    }
    if (L.wide == 0 && (hbm || ni > 0)) {
        const auto t_c0 = tnow();
        w = Bvh4Out();
        collapse_bvh4(bvh, 1, w);
        if (ptimes) fprintf(stderr, "pm_commit: collapse %.1f ms\n", tms(t_c0, tnow()));
        /* a leaf the quantized count cannot code (>= LEAF_TRIS primitives,
         * possible at build_bvh's depth limit) keeps the binary traversal,
         * like a tree whose stack bound exceeds BVH_STACK */
        if (opt.bfs) bvh4_bfs_order(w.nodes);
        const auto t_q0 = tnow();
        qn.clear();
        const bool coded = quantize_bvh4(w.nodes, bvh.refs, qn);
        if (ptimes) fprintf(stderr, "pm_commit: quantize %.1f ms\n", tms(t_q0, tnow()));
        if (ni > 0 && !(coded && w.max_stack + IL.max_stack + 1 <= BVH_STACK))
            return fail(err, "instanced scene: top-level tree not codable (stack %d + %d)", w.max_stack, IL.max_stack);
        if (coded && w.max_stack <= BVH_STACK) {
            if (ni > 0) { /* the objects' nodes follow the top-level tree's */
                const uint32_t top = (uint32_t)(qn.size() / 16);
                relocate_bvh4(IL.qn, top);
                for (int64_t i = 0; i < ni; ++i) IL.insts[8 * i + 6].x = ibits(fbits_h(IL.insts[8 * i + 6].x) + (int)top);
                qn.insert(qn.end(), IL.qn.begin(), IL.qn.end());
                L.size[SEC_INSTS] = vbytes(IL.insts);
            }
            L.wide = 2;
            L.wide_stack = w.max_stack + (ni > 0 ? IL.max_stack : 0);
            out.bvh4_nodes = (int64_t)(qn.size() / 16);
            out.bvh4_depth = w.depth;
        }
    }
    L.size[SEC_WNODES] = L.wide == 0 ? 0 : vbytes(qn);
    /* instanced scenes never go LDS-resident (MODE_INST walks the 4-wide trees from HBM) */
    plan_layout(L, ni > 0);

    /* one allocation for every section (no regrowth copies of a 250 MB blob); the gaps stay zero */
    out.bytes.assign(L.bytes, 0);
    const void *src[SEC_COUNT] = {};
    src[SEC_NODES] = bvh.nodes.data(); src[SEC_REFS] = bvh.refs.data();
    src[SEC_GEO] = tri_geo.data(); src[SEC_SHADE] = tri_shade.data();
    src[SEC_TID] = tri_id.data(); src[SEC_INFO] = tri_info.data();
    src[SEC_NORMS] = norms.data(); src[SEC_DISKS] = hs.disks.data();
    src[SEC_SPHERES] = hs.spheres.data(); src[SEC_MATS] = hs.materials.data();
    src[SEC_LIGHTS] = hs.lights.data();
    src[SEC_OBJV] = IL.objv.data(); src[SEC_OBJINFO] = IL.objinfo.data();
    src[SEC_OBJN] = IL.objn.data(); src[SEC_OBJUV] = IL.objuv.data();
    src[SEC_OBJMESH] = IL.objmesh.data(); src[SEC_INSTS] = IL.insts.data();
    src[SEC_WNODES] = qn.data();
    for (int s = 0; s < SEC_COUNT; ++s)
        if (L.size[s]) std::memcpy(&out.bytes[L.off[s]], src[s], L.size[s]);

    if (id_order) {
        const int64_t np = nst / 2;
        out.tri_pairs.assign((size_t)std::max<int64_t>(np, 1) * 24, 0.f);
        const float *geo = tri_geo.data();
        for (int64_t j = 0; j < np; ++j)
            for (int q = 0; q < 12; ++q)
                for (int h = 0; h < 2; ++h) out.tri_pairs[(size_t)j * 24 + 2 * q + h] = geo[(size_t)(2 * j + h) * 12 + q];
    }
    L.n_nodes = (int64_t)(bvh.nodes.size() / 16);
    /* the traversal loops' guard: with instances it must cover an object's tree too */
    if (ni > 0) L.n_nodes = std::max<int64_t>(L.n_nodes, out.bvh4_nodes);
    L.id_order = id_order;
    return PM_OK;
}

/* ---------------------------------------------------------- distant light */
void coordinate_system(const double v[3], double v1[3], double v2[3]) {
    if (std::fabs(v[0]) > std::fabs(v[1])) {
        const double inv = 1.0 / std::sqrt(v[0] * v[0] + v[2] * v[2]);
        v1[0] = -v[2] * inv; v1[1] = 0.0; v1[2] = v[0] * inv;
    } else {
        const double inv = 1.0 / std::sqrt(v[1] * v[1] + v[2] * v[2]);
        v1[0] = 0.0; v1[1] = v[2] * inv; v1[2] = -v[1] * inv;
    }
    v2[0] = v[1] * v1[2] - v[2] * v1[1];
    v2[1] = v[2] * v1[0] - v[0] * v1[2];
    v2[2] = v[0] * v1[1] - v[1] * v1[0];
}

namespace {

bool finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

/* the unit vector of v in double, rounded to float; false for a zero v */
bool unit3(const float v[3], float out[3]) {
    const double len = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; ++a) out[a] = (float)((double)v[a] / len);
    return true;
}

} // namespace

int make_distant_light(const float to_light[3], const float L[3], LightDev &out, std::string &err) {
    if (!to_light || !L) return fail(err, "pm_add_light_distant: null pointer");
    if (!finite3(to_light) || !finite3(L)) return fail(err, "pm_add_light_distant: a value is not finite");
    float w[3];
    if (!unit3(to_light, w)) return fail(err, "pm_add_light_distant: zero direction");
    out = LightDev{};
    out.o_type = f4(0, 0, 0, ibits(PM_LIGHT_DISTANT));
    out.p1_ns = f4(0, 0, 0, ibits(1));
    out.p2_r2d = f4(0, 0, 0, 0);
    out.n_area = f4(-w[0], -w[1], -w[2], 0);
    out.le = f4(L[0], L[1], L[2], 0);
    return PM_OK;
}

void world_sphere(const float blo[3], const float bhi[3], float sphere[4]) {
    double r2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        sphere[a] = (float)(0.5 * ((double)blo[a] + (double)bhi[a]));
        const double d = std::max(std::fabs((double)bhi[a] - (double)sphere[a]), std::fabs((double)blo[a] - (double)sphere[a]));
        r2 += d * d;
    }
    const double r = std::sqrt(r2);
    float rf = (float)r;
    if ((double)rf < r) rf = std::nextafter(rf, INFINITY);
    sphere[3] = rf;
}

int finish_lights(HostScene &hs, const float blo[3], const float bhi[3], float sphere[4], std::string &err) {
    world_sphere(blo, bhi, sphere);
    const double R = sphere[3];
    for (size_t l = 0; l < hs.lights.size(); ++l) {
        LightDev &L = hs.lights[l];
        if (fbits_h(L.o_type.w) != PM_LIGHT_DISTANT) continue;
        const double area = M_PI * R * R;
        if (!(sphere[3] > 0.f) || !std::isfinite(sphere[0]) || !std::isfinite(sphere[1]) || !std::isfinite(sphere[2]) ||
            !std::isfinite((float)area))
            return fail(err, "distant light %zu: the world sphere's radius %g is 0 or not finite", l, R);
        const double w[3] = {-(double)L.n_area.x, -(double)L.n_area.y, -(double)L.n_area.z};
        double v1[3], v2[3];
        coordinate_system(w, v1, v2);
        L.o_type = f4((float)(sphere[0] + R * w[0]), (float)(sphere[1] + R * w[1]), (float)(sphere[2] + R * w[2]),
                      ibits(PM_LIGHT_DISTANT));
        L.p1_ns = f4((float)(R * v1[0]), (float)(R * v1[1]), (float)(R * v1[2]), ibits(1));
        L.p2_r2d = f4((float)(R * v2[0]), (float)(R * v2[1]), (float)(R * v2[2]), 0.f);
        L.n_area.w = (float)area;
        L.le.w = 2.f * sphere[3];
        if (!std::isfinite(L.le.w)) return fail(err, "distant light %zu: the world sphere's radius %g is not finite", l, R);
    }
    return PM_OK;
}

/* --------------------------------------------------------------- textures */
namespace {

bool finite_n(const float *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

/* operand k of a checkerboard or scale: a constant rgb, or a copy of the
 * TEX_SINGLE record `tex` names */
int resolve_operand(const HostScene &hs, const char *who, int k, int tex, const float *rgb, TexOperand &o, std::string &err) {
    if (tex < 0) {
        o = TexOperand{};
        o.rgb[0] = rgb[0]; o.rgb[1] = rgb[1]; o.rgb[2] = rgb[2];
        o.texel0 = -1;
        return PM_OK;
    }
    if (tex >= (int)hs.textures.size()) return fail(err, "%s: tex%d = %d is out of range (%zu textures)", who, k, tex, hs.textures.size());
    if (hs.textures[(size_t)tex].kind != TEX_SINGLE)
        return fail(err, "%s: tex%d = %d is a checkerboard or a scale; an operand is an image or a constant", who, k, tex);
    o = hs.textures[(size_t)tex].op[0];
    return PM_OK;
}

} // namespace

int check_texture_image(const float *rgb, int w, int h, int wrap, const float *mapping, const float *scale, std::string &err) {
    if (!rgb || !mapping || !scale) return fail(err, "pm_add_texture_image: null pointer");
    if (w <= 0 || h <= 0) return fail(err, "pm_add_texture_image: image size %d x %d", w, h);
    /* 16 B per stored texel; texel offsets are ints */
    if ((int64_t)w > (INT64_MAX / 16) / (int64_t)h || (int64_t)w * (int64_t)h >= ((int64_t)1 << 31))
        return fail(err, "pm_add_texture_image: %d x %d texels are too many", w, h);
    if (wrap != TEX_WRAP_REPEAT && wrap != TEX_WRAP_BLACK && wrap != TEX_WRAP_CLAMP)
        return fail(err, "pm_add_texture_image: unknown wrap mode %d", wrap);
    if (!finite_n(mapping, 4) || !finite_n(scale, 3)) return fail(err, "pm_add_texture_image: a mapping or scale value is not finite");
    const int64_t n = 3 * (int64_t)w * (int64_t)h;
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(rgb[i])) return fail(err, "pm_add_texture_image: texel value %lld is not finite", (long long)i);
    return PM_OK;
}

int check_texture_operands(const char *who, const float *mapping, bool need_mapping, int tex1, const float *rgb1, int tex2,
                           const float *rgb2, std::string &err) {
    if (need_mapping && !mapping) return fail(err, "%s: null pointer", who);
    if ((tex1 < 0 && !rgb1) || (tex2 < 0 && !rgb2)) return fail(err, "%s: null pointer", who);
    if (need_mapping && !finite_n(mapping, 4)) return fail(err, "%s: a mapping value is not finite", who);
    if ((tex1 < 0 && !finite_n(rgb1, 3)) || (tex2 < 0 && !finite_n(rgb2, 3))) return fail(err, "%s: a colour is not finite", who);
    return PM_OK;
}

int add_texture_image(HostScene &hs, const float *rgb, int w, int h, int wrap, const float *mapping, const float *scale,
                      int *out_tex, std::string &err) {
    if (!out_tex) return fail(err, "pm_add_texture_image: null pointer");
    if (int rc = check_texture_image(rgb, w, h, wrap, mapping, scale, err)) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (hs.texels.size() + n >= ((size_t)1 << 31)) return fail(err, "pm_add_texture_image: too many texels in the scene");
    TexRec T{};
    T.kind = TEX_SINGLE;
    TexOperand &o = T.op[0];
    for (int a = 0; a < 3; ++a) o.rgb[a] = scale[a];
    o.texel0 = (int)hs.texels.size();
    o.w = w; o.h = h; o.wrap = wrap;
    for (int a = 0; a < 4; ++a) o.map[a] = mapping[a];
    T.op[1].texel0 = -1;
    hs.texels.reserve(hs.texels.size() + n);
    for (size_t i = 0; i < n; ++i) hs.texels.push_back(f4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f));
    hs.textures.push_back(T);
    *out_tex = (int)hs.textures.size() - 1;
    return PM_OK;
}

int add_texture_checker(HostScene &hs, const float *mapping, int tex1, const float *rgb1, int tex2, const float *rgb2,
                        int *out_tex, std::string &err) {
    const char *who = "pm_add_texture_checker";
    if (!out_tex) return fail(err, "%s: null pointer", who);
    if (int rc = check_texture_operands(who, mapping, true, tex1, rgb1, tex2, rgb2, err)) return rc;
    TexRec T{};
    T.kind = TEX_CHECKER;
    for (int a = 0; a < 4; ++a) T.map[a] = mapping[a];
    if (int rc = resolve_operand(hs, who, 1, tex1, rgb1, T.op[0], err)) return rc;
    if (int rc = resolve_operand(hs, who, 2, tex2, rgb2, T.op[1], err)) return rc;
    hs.textures.push_back(T);
    *out_tex = (int)hs.textures.size() - 1;
    return PM_OK;
}

int add_texture_scale(HostScene &hs, int tex1, const float *rgb1, int tex2, const float *rgb2, int *out_tex, std::string &err) {
    const char *who = "pm_add_texture_scale";
    if (!out_tex) return fail(err, "%s: null pointer", who);
    if (int rc = check_texture_operands(who, nullptr, false, tex1, rgb1, tex2, rgb2, err)) return rc;
    TexRec T{};
    T.kind = TEX_SCALE;
    if (int rc = resolve_operand(hs, who, 1, tex1, rgb1, T.op[0], err)) return rc;
    if (int rc = resolve_operand(hs, who, 2, tex2, rgb2, T.op[1], err)) return rc;
    hs.textures.push_back(T);
    *out_tex = (int)hs.textures.size() - 1;
    return PM_OK;
}

int check_material_textured(int type, std::string &err) {
    if (type != PM_MATTE) return fail(err, "pm_add_material_textured: only PM_MATTE takes a Kd texture (type %d)", type);
    return PM_OK;
}

int add_material_textured(HostScene &hs, int type, int kd_tex, int *out_id, std::string &err) {
    if (int rc = check_material_textured(type, err)) return rc;
    if (!out_id) return fail(err, "pm_add_material_textured: null pointer");
    if (kd_tex < 0 || kd_tex >= (int)hs.textures.size())
        return fail(err, "pm_add_material_textured: texture id %d is out of range (%zu textures)", kd_tex, hs.textures.size());
    hs.materials.push_back(f4(1.f, 1.f, 1.f, ibits(PM_MATTE)));
    hs.mat_tex.resize(hs.materials.size(), -1);
    hs.mat_tex.back() = kd_tex;
    *out_id = (int)hs.materials.size() - 1;
    return PM_OK;
}

bool scene_textured(const HostScene &hs) {
    for (size_t m = 0; m < hs.mat_tex.size() && m < hs.materials.size(); ++m)
        if (hs.mat_tex[m] >= 0) return true;
    return false;
}

std::vector<int> material_textures(const HostScene &hs) {
    std::vector<int> t(hs.materials.size(), -1);
    for (size_t m = 0; m < t.size() && m < hs.mat_tex.size(); ++m) t[m] = hs.mat_tex[m];
    return t;
}

std::vector<float4> triangle_uvs(const HostScene &hs, const uint32_t *tri_order, int64_t n) {
    std::vector<float4> uv(2 * (size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const HTri &tr = hs.tris[tri_order[k]];
        float c[6] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f}; /* tri_frame's default corners */
        if (hs.meshes[tr.mesh].has_uv)
            for (int q = 0; q < 3; ++q) { c[2 * q] = hs.UV[2 * (size_t)tr.v[q]]; c[2 * q + 1] = hs.UV[2 * (size_t)tr.v[q] + 1]; }
        uv[2 * k] = f4(c[0], c[1], c[2], c[3]);
        uv[2 * k + 1] = f4(c[4], c[5], 0.f, 0.f);
    }
    return uv;
}

double texture_bound(const HostScene &hs, int t, bool *negative) {
    const TexRec &T = hs.textures[(size_t)t];
    bool neg = false;
    auto operand = [&](const TexOperand &o) {
        double c = 0.0;
        for (int a = 0; a < 3; ++a) { c = std::max(c, std::fabs((double)o.rgb[a])); neg = neg || o.rgb[a] < 0.f; }
        if (o.texel0 < 0) return c;
        /* the bilinear blend stays between its texels (f in [0, 1)), black adds 0 */
        double m = 0.0;
        const size_t n = (size_t)o.w * (size_t)o.h;
        for (size_t i = 0; i < n; ++i) {
            const float4 &x = hs.texels[(size_t)o.texel0 + i];
            m = std::max({m, std::fabs((double)x.x), std::fabs((double)x.y), std::fabs((double)x.z)});
            neg = neg || x.x < 0.f || x.y < 0.f || x.z < 0.f;
        }
        return m * c;
    };
    const double a = operand(T.op[0]);
    double r = a;
    if (T.kind == TEX_CHECKER) r = std::max(a, operand(T.op[1]));
    else if (T.kind == TEX_SCALE) r = a * operand(T.op[1]);
    if (negative) *negative = neg;
    return r * (1.0 + 1e-6); /* the blend's and the products' rounding */
}

/* ------------------------------------------------------ specular materials */
int check_material_specular(int type, const float *kr, const float *kt, float index, std::string &err) {
    const char *who = "pm_add_material_specular";
    if (type != PM_MIRROR && type != PM_GLASS) return fail(err, "%s: type %d is neither PM_MIRROR nor PM_GLASS", who, type);
    if (!kr) return fail(err, "%s: null pointer", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(kr[a]) || kr[a] < 0.f) return fail(err, "%s: Kr component %d is %g (negative or not finite)", who, a, (double)kr[a]);
    if (type == PM_MIRROR) return PM_OK;
    if (!kt) return fail(err, "%s: null pointer", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(kt[a]) || kt[a] < 0.f) return fail(err, "%s: Kt component %d is %g (negative or not finite)", who, a, (double)kt[a]);
    if (!std::isfinite(index) || !(index > 0.f)) return fail(err, "%s: index %g is not finite or not above 0", who, (double)index);
    return PM_OK;
}

int add_material_specular(HostScene &hs, int type, const float *kr, const float *kt, float index, int *out_id,
                          std::string &err) {
    if (int rc = check_material_specular(type, kr, kt, index, err)) return rc;
    if (!out_id) return fail(err, "pm_add_material_specular: null pointer");
    hs.materials.push_back(f4(0.f, 0.f, 0.f, ibits(type)));
    hs.mat_spec.resize(2 * hs.materials.size(), f4(0.f, 0.f, 0.f, 0.f));
    const bool glass = type == PM_GLASS;
    hs.mat_spec[hs.mat_spec.size() - 2] = f4(kr[0], kr[1], kr[2], glass ? index : 0.f);
    hs.mat_spec[hs.mat_spec.size() - 1] = f4(glass ? kt[0] : 0.f, glass ? kt[1] : 0.f, glass ? kt[2] : 0.f, ibits(1));
    *out_id = (int)hs.materials.size() - 1;
    return PM_OK;
}

bool scene_specular(const HostScene &hs) {
    for (size_t m = 0; 2 * m + 1 < hs.mat_spec.size() && m < hs.materials.size(); ++m)
        if (fbits_h(hs.mat_spec[2 * m + 1].w) != 0) return true;
    return false;
}

std::vector<float4> material_specular_table(const HostScene &hs) {
    std::vector<float4> t(2 * hs.materials.size(), f4(0.f, 0.f, 0.f, 0.f));
    for (size_t i = 0; i < t.size() && i < hs.mat_spec.size(); ++i) t[i] = hs.mat_spec[i];
    return t;
}

/* --------------------------------------------------------- light summary */
int light_selection_cdf(const int *types, const float *le_rgb, const float *areas, int n, float *cdf_out, std::string &err) {
    if (!types || !le_rgb || !areas || !cdf_out) return fail(err, "pm_light_selection_cdf: null pointer");
    if (n <= 0) return fail(err, "pm_light_selection_cdf: no lights");
    std::vector<double> sum((size_t)n);
    double total = 0.0;
    for (int l = 0; l < n; ++l) {
        const double y = 0.212671 * (double)le_rgb[3 * l] + 0.715160 * (double)le_rgb[3 * l + 1] +
                         0.072169 * (double)le_rgb[3 * l + 2];
        double w;
        switch (types[l]) {
        case PM_LIGHT_POINT: w = y * (4.0 * M_PI); break;
        case PM_LIGHT_AREA_DISK:
        case PM_LIGHT_AREA_MESH: w = y * (M_PI * (double)areas[l]); break;
        case PM_LIGHT_DISTANT: w = y * (double)areas[l]; break;
        default: return fail(err, "pm_light_selection_cdf: light %d has unknown type %d", l, types[l]);
        }
        if (w < 0.0) w = 0.0;
        total += w;
        sum[(size_t)l] = total;
    }
    if (!(total > 0.0) || !std::isfinite(total))
        return fail(err, "pm_light_selection_cdf: total selection weight %g of %d lights is 0 or not finite", total, n);
    for (int l = 0; l < n; ++l) cdf_out[l] = (float)(sum[(size_t)l] / total);
    cdf_out[n - 1] = 1.0f;
    return PM_OK;
}

/* emitted power bound of a light (sample_le's Le / pdf): a point light's
 * 4 pi I; a disk's Le area 2 pi; a mesh's the same with its total area
 * (n_area.w); a distant light's L pi R^2 (a hair above the device's
 * |d.d| L area: 1.001). Negative: a type that has none */
static double light_power_bound(const LightDev &L) {
    const double le = std::max({std::fabs(L.le.x), std::fabs(L.le.y), std::fabs(L.le.z)});
    switch (fbits_h(L.o_type.w)) {
    case PM_LIGHT_POINT: return le * 4.0 * M_PI;
    case PM_LIGHT_AREA_DISK:
    case PM_LIGHT_AREA_MESH: return le * L.n_area.w * 2.0 * M_PI;
    case PM_LIGHT_DISTANT: return le * L.n_area.w * 1.001;
    default: return -1.0;
    }
}

int light_summary(const HostScene &hs, LightSummary &out, std::string &err) {
    out = LightSummary();
    double em = 0.0, kd = 1.0;
    for (const LightDev &L : hs.lights) {
        const double bound = light_power_bound(L);
        if (bound < 0.0) return fail(err, "light type %d has no emitted-power bound", fbits_h(L.o_type.w));
        em = std::max(em, bound);
    }
    for (const float4 &m : hs.materials)
        if (fbits_h(m.w) == PM_MATTE) kd = std::max({kd, (double)m.x, (double)m.y, (double)m.z});
    out.emit_max = std::max(em, 1e-30);
    out.kd_max = kd;
    /* PM_ALL_LIGHTS: the selection table, and the weight bound with the pick's
     * probability divided out. A scene that emits nothing keeps a zero table:
     * a fixed light_source_index still renders it, PM_ALL_LIGHTS is refused
     * (check_params) */
    const size_t nl = hs.lights.size();
    std::vector<int> types(nl);
    std::vector<float> rgb(3 * nl), areas(nl);
    for (size_t l = 0; l < nl; ++l) {
        const LightDev &L = hs.lights[l];
        types[l] = fbits_h(L.o_type.w);
        rgb[3 * l] = L.le.x; rgb[3 * l + 1] = L.le.y; rgb[3 * l + 2] = L.le.z;
        areas[l] = L.n_area.w;
    }
    out.cdf.assign(nl, 0.f);
    std::string why; /* a scene without selection weight is not an error here */
    out.cdf_ok = light_selection_cdf(types.data(), rgb.data(), areas.data(), (int)nl, out.cdf.data(), why) == PM_OK;
    if (!out.cdf_ok) out.cdf.assign(nl, 0.f);
    double em_all = 0.0;
    for (size_t l = 0; l < nl && out.cdf_ok; ++l) {
        const float pmf = out.cdf[l] - (l ? out.cdf[l - 1] : 0.f);
        if (!(pmf > 0.f)) continue; /* never picked */
        em_all = std::max(em_all, light_power_bound(hs.lights[l]) / (double)pmf);
    }
    out.emit_max_all = std::max(em_all, 1e-30);
    bool nn = true;
    for (const LightDev &L : hs.lights) nn = nn && L.le.x >= 0.f && L.le.y >= 0.f && L.le.z >= 0.f && L.n_area.w >= 0.f;
    for (const float4 &m : hs.materials)
        if (fbits_h(m.w) == PM_MATTE) nn = nn && m.x >= 0.f && m.y >= 0.f && m.z >= 0.f;
    /* a textured matte's Kd is its texture, not the table's (1, 1, 1): the
     * largest value the texture can return bounds it, and a negative texel,
     * scale or colour ends the non-negative guarantee */
    for (size_t m = 0; m < hs.mat_tex.size() && m < hs.materials.size(); ++m) {
        if (hs.mat_tex[m] < 0) continue;
        bool neg = false;
        out.kd_max = std::max(out.kd_max, texture_bound(hs, hs.mat_tex[m], &neg));
        nn = nn && !neg;
    }
    /* a step through a material of the physical specular model scales a
     * photon's flux by Kr or Kt (at most: F Kr, (1 - F) Kt), both >= 0; a
     * path takes up to max_specular_depth such steps, so the bound is kept
     * apart from kd_max, which counts max_photon_count Lambert bounces */
    for (size_t m = 0; 2 * m + 1 < hs.mat_spec.size() && m < hs.materials.size(); ++m) {
        const float4 &a = hs.mat_spec[2 * m], &b = hs.mat_spec[2 * m + 1];
        if (fbits_h(b.w) == 0) continue;
        out.spec_max = std::max({out.spec_max, (double)a.x, (double)a.y, (double)a.z, (double)b.x, (double)b.y, (double)b.z});
    }
    out.scene_nonneg = nn;
    return PM_OK;
}

} // namespace pm
