/*
 * pm_render_cli — renders a scene through the pbrt-facing C++ layer
 * (pm_cudarender.h), the way pbrt-v2 drives the reference plugin:
 *   CudaRenderInit -> CreateCudaShape x N (ObjectBegin/Instance optional)
 *   -> CreateCudaRenderer -> Render(lights, camera) -> Film::AddSample
 * and writes the image as PFM. Used by tests/test_adapter.py (GPU) to check
 * that this host path produces the same image as the Python stage driver.
 *
 *   pm_render_cli --scene cornell --width W --height H --camera e0 e1 e2 f0 f1 f2 r0 r1 r2 u0 u1 u2
 *                 [--paths N] [--passes P] [--structure grid|kd] [--instanced]
 *                 [--renderer photonmapping|simple] [--light N|all] --out img.pfm
 *   pm_render_cli --pbrt scene.pbrt [--out img.pfm] [--renderer R] [--paths N] [--passes P] [--structure S]
 *                 [--light N|all]
 *                 (a pbrt-v2 scene file through pm_pbrt.h; command-line options override the file)
 *                 [--spp XxY] [--filter name[:xw[:yw[:a[:b]]]]] [--lens R:F] [--no-jitter]   (the device camera + film)
 *                 [--final-gather N]   (N in 1..256 gather rays per eye hit with a kNN estimate at their hits,
 *                 pm_render_final_gather; as Renderer "cuda" "integer finalgathersamples" [N] in the scene file; 0: off)
 *                 [--caustic-map]   (with final gathering: the caustic map looked up at the eye hits, pm_set_caustic_map;
 *                 as Renderer "cuda" "bool causticmap" ["true"] in the scene file; warns without final gathering)
 *                 [--resample]   (a fresh jitter and lens sample per pixel every pass, pm_render_resampled: one
 *                 stratum, no film, jitter on; as Renderer "cuda" "bool resample" ["true"] in the scene file)
 *   pm_render_cli --pbrt scene.pbrt --dump   (parse only, no device: the plugin calls as JSON, with the
 *                 renderer's light_source_index and the scene's light selection table)
 * --light: the light the photon paths start on; "all" (or -1) starts them on
 * every light, picked per path by emitted power (PM_ALL_LIGHTS).
 *   pm_render_cli --selftest      (host-only checks, no device needed)
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pm_cudarender.h"
#include "pm_pbrt.h"

using namespace pmcuda;

namespace {

/* one sample per pixel: the film is the pixel grid */
struct PixelFilm : Film {
    int W, H;
    std::vector<float> rgb;
    std::string path;
    PixelFilm(int w, int h, std::string p) : W(w), H(h), rgb((size_t)3 * w * h, 0.f), path(std::move(p)) {}
    void AddSample(const CameraSample &s, const float c[3]) override {
        const int x = (int)std::floor(s.imageX), y = (int)std::floor(s.imageY);
        if (x < 0 || y < 0 || x >= W || y >= H) return;
        float *d = &rgb[3 * ((size_t)y * W + x)];
        d[0] = c[0]; d[1] = c[1]; d[2] = c[2];
    }
    void WriteImage() override { /* PFM: rows bottom to top, little endian */
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) throw Error("cannot write " + path);
        std::fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
        for (int y = H - 1; y >= 0; --y) std::fwrite(&rgb[3 * (size_t)y * W], sizeof(float), 3 * (size_t)W, f);
        std::fclose(f);
    }
};

Shape quads(const std::vector<std::vector<float>> &q) {
    Shape s;
    for (const auto &quad : q) {
        const int b = (int)(s.P.size() / 3);
        s.P.insert(s.P.end(), quad.begin(), quad.end());
        const int idx[6] = {b, b + 1, b + 2, b, b + 2, b + 3};
        s.indices.insert(s.indices.end(), idx, idx + 6);
    }
    return s;
}

/* The classic Cornell box of pmrender/scenes.py cornell_box() (C2), issued
 * as pbrt would: world-space triangle meshes, a disk area light under
 * Translate 278 548.7 279.5 + Rotate 90 about x (exact matrix). */
void cornell(bool instanced, std::vector<Light> &lights) {
    static const Material white{Material::Matte, {0.73f, 0.73f, 0.73f}};
    static const Material red{Material::Matte, {0.63f, 0.065f, 0.05f}};
    static const Material green{Material::Matte, {0.14f, 0.45f, 0.091f}};
    static const Material black{Material::Matte, {0.f, 0.f, 0.f}};
    CreateCudaShape("trianglemesh", quads({{552.8f, 0, 0, 0, 0, 0, 0, 0, 559.2f, 549.6f, 0, 559.2f},
                                           {556.0f, 548.8f, 0, 556.0f, 548.8f, 559.2f, 0, 548.8f, 559.2f, 0, 548.8f, 0},
                                           {549.6f, 0, 559.2f, 0, 0, 559.2f, 0, 548.8f, 559.2f, 556.0f, 548.8f, 559.2f}}),
                    nullptr, &white, -1);
    CreateCudaShape("trianglemesh", quads({{0, 0, 559.2f, 0, 0, 0, 0, 548.8f, 0, 0, 548.8f, 559.2f}}), nullptr, &green,
                    -1);
    CreateCudaShape("trianglemesh",
                    quads({{552.8f, 0, 0, 549.6f, 0, 559.2f, 556.0f, 548.8f, 559.2f, 556.0f, 548.8f, 0}}), nullptr,
                    &red, -1);
    const Shape shortb = quads({{130, 165, 65, 82, 165, 225, 240, 165, 272, 290, 165, 114},
                                {290, 0, 114, 290, 165, 114, 240, 165, 272, 240, 0, 272},
                                {130, 0, 65, 130, 165, 65, 290, 165, 114, 290, 0, 114},
                                {82, 0, 225, 82, 165, 225, 130, 165, 65, 130, 0, 65},
                                {240, 0, 272, 240, 165, 272, 82, 165, 225, 82, 0, 225}});
    const Shape tallb = quads({{423, 330, 247, 265, 330, 296, 314, 330, 456, 472, 330, 406},
                               {423, 0, 247, 423, 330, 247, 472, 330, 406, 472, 0, 406},
                               {472, 0, 406, 472, 330, 406, 314, 330, 456, 314, 0, 456},
                               {314, 0, 456, 314, 330, 456, 265, 330, 296, 265, 0, 296},
                               {265, 0, 296, 265, 330, 296, 423, 330, 247, 423, 0, 247}});
    if (instanced) { /* ObjectBegin "blocks" ... ObjectEnd; ObjectInstance "blocks" (identity) */
        static const int key = 0;
        CreateCudaShape("trianglemesh", shortb, &key, &white, -1);
        CreateCudaShape("trianglemesh", tallb, &key, &white, -1);
        CudaObjectInstance(&key, Transform::identity());
    } else {
        CreateCudaShape("trianglemesh", shortb, nullptr, &white, -1);
        CreateCudaShape("trianglemesh", tallb, nullptr, &white, -1);
    }
    Light L;
    L.kind = Light::AreaDisk;
    L.disk.radius = 65.f;
    L.disk.o2w = Transform::identity();
    const float m[16] = {1, 0, 0, 278.f, 0, 0, -1, 548.7f, 0, 1, 0, 279.5f, 0, 0, 0, 1};
    const float mi[16] = {1, 0, 0, -278.f, 0, 0, 1, -279.5f, 0, -1, 0, 548.7f, 0, 0, 0, 1};
    std::memcpy(L.disk.o2w.m, m, sizeof(m));
    std::memcpy(L.disk.o2w.minv, mi, sizeof(mi));
    L.Lemit = {17.f, 17.f, 17.f};
    L.n_samples = 1;
    lights.push_back(L);
    CreateCudaShape("disk", L.disk, nullptr, &black, 0);
}

int selftest() {
    int bad = 0;
    auto near = [&](float a, float b, const char *what) {
        if (std::fabs(a - b) > 1e-5f * (1.f + std::fabs(b))) { std::printf("FAIL %s: %g vs %g\n", what, a, b); ++bad; }
    };
    const Transform t = Transform::translate(1, 2, 3) * Transform::rotate_x(90.f);
    const float p[3] = {0, 0, 1};
    float o[3];
    t.point(p, o); /* rotate (0,0,1) -> (0,-1,0), then translate */
    near(o[0], 1.f, "point.x"); near(o[1], 1.f, "point.y"); near(o[2], 3.f, "point.z");
    const float v[3] = {0, 1, 0};
    t.vector(v, o); /* (0,1,0) -> (0,0,1), translation ignored */
    near(o[0], 0.f, "vector.x"); near(o[1], 0.f, "vector.y"); near(o[2], 1.f, "vector.z");
    float r[16];
    for (int i = 0; i < 4; ++i) /* m * minv == I */
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s += t.m[4 * i + k] * t.minv[4 * k + j];
            r[4 * i + j] = s;
            near(s, i == j ? 1.f : 0.f, "m*minv");
        }
    const float n[3] = {0, 0, 1};
    t.normal(n, o); /* normals follow the inverse transpose: same as vectors for a rotation */
    near(o[0], 0.f, "normal.x"); near(o[1], -1.f, "normal.y"); near(o[2], 0.f, "normal.z");
    (void)r;
    std::printf(bad ? "selftest: %d failures\n" : "selftest: ok\n", bad);
    return bad ? 1 : 0;
}

/* --dump: records the plugin calls a scene file produces, as JSON (floats
 * printed round-trip exact) — the parse checked without a device */
struct DumpSink : PbrtSink {
    std::string out;
    std::map<const void *, int> keys;
    static void arr(std::string &o, const float *v, size_t n) {
        o += "[";
        char b[32];
        for (size_t i = 0; i < n; ++i) { std::snprintf(b, sizeof b, "%s%.9g", i ? ", " : "", v[i]); o += b; }
        o += "]";
    }
    int key(const void *k) {
        if (!k) return -1;
        auto it = keys.find(k);
        if (it != keys.end()) return it->second;
        const int id = (int)keys.size();
        keys[k] = id;
        return id;
    }
    void shape(const std::string &name, const Shape &s, const void *inst, const Material *m, int li) override {
        char b[160];
        if (!out.empty()) out += ",\n";
        std::snprintf(b, sizeof b, "{\"call\": \"shape\", \"name\": \"%s\", \"instance\": %d, \"light\": %d, ",
                      name.c_str(), key(inst), li);
        out += b;
        const int kind = !m ? -1 : (int)m->kind;
        const float k[3] = {m ? m->k.r : 0.f, m ? m->k.g : 0.f, m ? m->k.b : 0.f};
        std::snprintf(b, sizeof b, "\"material\": %d, \"k\": ", kind);
        out += b;
        arr(out, k, 3);
        if (m && m->kd_tex) { /* the Kd texture: kind 0 single, 1 checkerboard, 2 scale */
            const TextureDesc &t = *m->kd_tex;
            out += ", \"kd_tex\": {\"kind\": " + std::to_string((int)t.kind) + ", \"map\": ";
            arr(out, t.map, 4);
            out += ", \"ops\": [";
            for (int q = 0; q < (t.kind == TextureDesc::Single ? 1 : 2); ++q) {
                const TexOperand &o = t.op[q];
                const float c[3] = {o.rgb.r, o.rgb.g, o.rgb.b};
                out += std::string(q ? ", " : "") + "{\"image\": " + (o.image ? "1" : "0") + ", \"rgb\": ";
                arr(out, c, 3);
                out += ", \"w\": " + std::to_string(o.w) + ", \"h\": " + std::to_string(o.h) + ", \"wrap\": " +
                       std::to_string(o.wrap) + ", \"map\": ";
                arr(out, o.map, 4);
                out += ", \"texels\": ";
                arr(out, o.texels.data(), o.texels.size());
                out += "}";
            }
            out += "]}";
        }
        if (m && m->physical && (m->kind == Material::Mirror || m->kind == Material::Glass)) {
            /* Renderer "string specular" "pbrt": the parameters of pm_add_material_specular */
            const float kr[3] = {m->kr.r, m->kr.g, m->kr.b}, kt[3] = {m->kt.r, m->kt.g, m->kt.b};
            out += ", \"specular\": {\"kr\": ";
            arr(out, kr, 3);
            if (m->kind == Material::Glass) {
                out += ", \"kt\": ";
                arr(out, kt, 3);
                out += ", \"index\": ";
                arr(out, &m->index, 1);
            }
            out += "}";
        }
        out += ", \"P\": "; arr(out, s.P.data(), s.P.size());
        out += ", \"N\": "; arr(out, s.N.data(), s.N.size());
        out += ", \"uv\": "; arr(out, s.uv.data(), s.uv.size());
        out += ", \"indices\": [";
        for (size_t i = 0; i < s.indices.size(); ++i) out += (i ? ", " : "") + std::to_string(s.indices[i]);
        out += "], \"o2w\": "; arr(out, s.o2w.m, 16);
        out += ", \"w2o\": "; arr(out, s.o2w.minv, 16);
        const float sc[4] = {s.radius, s.height, s.inner_radius, s.phi_max};
        out += ", \"radius_height_inner_phimax\": "; arr(out, sc, 4);
        out += "}";
    }
    void objectInstance(const void *k, const Transform &tr) override {
        if (!out.empty()) out += ",\n";
        out += "{\"call\": \"instance\", \"instance\": " + std::to_string(key(k)) + ", \"o2w\": ";
        arr(out, tr.m, 16);
        out += "}";
    }
};

/* the area pm_commit's selection table sees for an area light: the disk's as
 * CudaRender::addLights passes it (pbrt Disk::Area), the mesh's as
 * pm_add_light_mesh sums it (per-triangle areas in double, in index order) */
float lightArea(const Light &L) {
    if (L.kind != Light::AreaMesh) {
        const float r = L.disk.radius, ri = L.disk.inner_radius;
        return L.disk.phi_max * 0.5f * (r * r - ri * ri);
    }
    double total = 0.0;
    const std::vector<float> &P = L.mesh.P;
    for (size_t t = 0; t + 2 < L.mesh.indices.size(); t += 3) {
        const float *p0 = &P[3 * (size_t)L.mesh.indices[t]], *p1 = &P[3 * (size_t)L.mesh.indices[t + 1]],
                    *p2 = &P[3 * (size_t)L.mesh.indices[t + 2]];
        const double a[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
        const double b[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        total += 0.5 * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    }
    return (float)total;
}

/* --spp XxY, --filter name[:xw[:yw[:a[:b]]]], --lens R:F, --no-jitter over the scene file's camera.
 * Each flag replaces what the scene file says about the same thing and
 * nothing else: jitter stays the Sampler's unless --no-jitter is given. The
 * device camera is used by the scene file's own rule: more than one sample
 * per pixel, a pixel filter, or a lens. */
struct CameraFlags {
    std::string spp, filter, lens;
    bool no_jitter = false;
    /* --resample: Renderer "bool resample" from the command line; --spp, --filter
     * and --no-jitter are then ignored with a warning, --lens still sets the lens */
    bool resample = false;
    bool any() const { return !spp.empty() || !filter.empty() || !lens.empty() || no_jitter || resample; }
};
float flag_float(const std::string &flag, const std::string &v) {
    char *end = nullptr;
    const float f = std::strtof(v.c_str(), &end);
    if (v.empty() || *end || !std::isfinite(f)) throw Error(flag + ": \"" + v + "\" is not a number");
    return f;
}
std::vector<std::string> split_colon(const std::string &v) {
    std::vector<std::string> part;
    size_t i = 0;
    while (true) {
        const size_t j = v.find(':', i);
        part.push_back(v.substr(i, j == std::string::npos ? j : j - i));
        if (j == std::string::npos) break;
        i = j + 1;
    }
    return part;
}
void apply_camera_flags(const CameraFlags &f, Camera &c) {
    if (!f.spp.empty()) {
        int n = 0;
        if (std::sscanf(f.spp.c_str(), "%dx%d%n", &c.xsamples, &c.ysamples, &n) != 2 || (size_t)n != f.spp.size() ||
            c.xsamples < 1 || c.xsamples > 8 || c.ysamples < 1 || c.ysamples > 8)
            throw Error("--spp " + f.spp + ": expected XxY with 1..8 each");
    }
    bool filter_given = c.device_camera && c.filter.type != PM_FILTER_NONE;
    if (!f.filter.empty()) {
        const std::vector<std::string> part = split_colon(f.filter);
        pm_filter k = {PM_FILTER_NONE, 2.f, 2.f, 0.f, 0.f};
        if (part[0] == "box") { k.type = PM_FILTER_BOX; k.xwidth = k.ywidth = 0.5f; }
        else if (part[0] == "triangle") k.type = PM_FILTER_TRIANGLE;
        else if (part[0] == "gaussian") { k.type = PM_FILTER_GAUSSIAN; k.a = 2.f; }
        else if (part[0] == "mitchell") { k.type = PM_FILTER_MITCHELL; k.a = k.b = 1.f / 3.f; }
        else throw Error("--filter " + f.filter + ": box, triangle, gaussian or mitchell");
        if (part.size() > 5) throw Error("--filter " + f.filter + ": expected name[:xw[:yw[:a[:b]]]]");
        if (part.size() > 1) k.xwidth = k.ywidth = flag_float("--filter", part[1]);
        if (part.size() > 2) k.ywidth = flag_float("--filter", part[2]);
        if (part.size() > 3) k.a = flag_float("--filter", part[3]);
        if (part.size() > 4) k.b = flag_float("--filter", part[4]);
        if (!(k.xwidth > 0.f && k.xwidth <= 4.f) || !(k.ywidth > 0.f && k.ywidth <= 4.f))
            throw Error("--filter " + f.filter + ": widths outside (0, 4]");
        c.filter = k;
        filter_given = true;
    }
    if (!f.lens.empty()) {
        const std::vector<std::string> part = split_colon(f.lens);
        if (part.size() != 2) throw Error("--lens " + f.lens + ": expected R:F");
        c.lens_radius = flag_float("--lens", part[0]);
        c.focal_distance = flag_float("--lens", part[1]);
        if (c.lens_radius < 0.f || (c.lens_radius > 0.f && !(c.focal_distance > 0.f)))
            throw Error("--lens " + f.lens + ": R >= 0, and F > 0 with a lens");
    }
    if (f.no_jitter) c.jitter = false;
    c.device_camera = c.xsamples * c.ysamples > 1 || filter_given || c.lens_radius > 0.f;
    if (c.device_camera && !filter_given) c.filter = pm_filter{PM_FILTER_BOX, 0.5f, 0.5f, 0.f, 0.f};
    if (!c.device_camera) c.filter = pm_filter{PM_FILTER_NONE, 0.f, 0.f, 0.f, 0.f};
}
/* the same, then the resampled render's camera over it (--resample, or the scene file's Renderer "bool resample") */
void apply_camera_flags(const CameraFlags &f, PbrtOptions &o) {
    const bool from_file = o.resample;
    if (f.resample) o.resample = true;
    if (!o.resample) { apply_camera_flags(f, o.camera); return; }
    if (!from_file) { /* the file's own Sampler / PixelFilter: the parser has warned where the file asked */
        const int over = resampleCamera(o.camera);
        if (over & 1) { std::fprintf(stderr, "Warning: --resample: the scene's Sampler is ignored (the passes are the samples)\n"); o.warnings++; }
        if (over & 2) { std::fprintf(stderr, "Warning: --resample: the scene's PixelFilter is ignored\n"); o.warnings++; }
    }
    if (!f.spp.empty() || !f.filter.empty() || f.no_jitter) {
        std::fprintf(stderr, "Warning: --spp, --filter and --no-jitter are ignored under resampling\n");
        o.warnings++;
    }
    CameraFlags lens;
    lens.lens = f.lens;
    apply_camera_flags(lens, o.camera);
    resampleCamera(o.camera);
}

/* --specular pbrt|reference: overrides the file's Renderer "string specular" */
std::string g_specular;
/* --final-gather N: overrides the file's Renderer "integer finalgathersamples" (-1: not given) */
int g_final_gather = -1;
/* --caustic-map: as the file's Renderer "bool causticmap" ["true"] */
bool g_caustic_map = false;

/* the command line's final-gather settings over the file's; the caustic map is honoured only together with
 * final gathering and warns otherwise */
void apply_final_gather_flags(PbrtOptions &o) {
    if (g_final_gather >= 0) o.settings.final_gather = g_final_gather;
    if (g_caustic_map) o.settings.caustic_map = true;
    if (o.settings.caustic_map && o.settings.final_gather == 0) {
        std::fprintf(stderr, "Warning: the caustic map (Renderer \"causticmap\", --caustic-map) needs final gathering "
                             "(\"finalgathersamples\", --final-gather): it is off\n");
        o.settings.caustic_map = false;
        o.warnings++;
    }
}

int dump(const std::string &path, const CameraFlags &cflags) {
    DumpSink sink;
    PbrtOptions o;
    o.specular_override = g_specular;
    PbrtParser parser;
    parser.parseFile(path, sink, o);
    apply_camera_flags(cflags, o);
    apply_final_gather_flags(o);
    std::string lights;
    for (const Light &L : o.lights) {
        if (!lights.empty()) lights += ",\n";
        char b[128];
        if (L.kind == Light::Point) {
            const float I[3] = {L.intensity.r, L.intensity.g, L.intensity.b};
            lights += "{\"kind\": \"point\", \"pos\": ";
            DumpSink::arr(lights, L.pos, 3);
            lights += ", \"I\": ";
            DumpSink::arr(lights, I, 3);
        } else if (L.kind == Light::Distant) {
            const float Lr[3] = {L.intensity.r, L.intensity.g, L.intensity.b};
            lights += "{\"kind\": \"distant\", \"to_light\": ";
            DumpSink::arr(lights, L.dir, 3);
            lights += ", \"L\": ";
            DumpSink::arr(lights, Lr, 3);
        } else if (L.kind == Light::AreaMesh) {
            const float Le[3] = {L.Lemit.r, L.Lemit.g, L.Lemit.b};
            std::snprintf(b, sizeof b, "{\"kind\": \"mesh\", \"nsamples\": %d, \"reverse_orientation\": %d, \"Le\": ",
                          L.n_samples, L.reverse_orientation ? 1 : 0);
            lights += b;
            DumpSink::arr(lights, Le, 3);
            lights += ", \"P\": ";
            DumpSink::arr(lights, L.mesh.P.data(), L.mesh.P.size());
            lights += ", \"indices\": [";
            for (size_t i = 0; i < L.mesh.indices.size(); ++i) lights += (i ? ", " : "") + std::to_string(L.mesh.indices[i]);
            lights += "]";
        } else {
            const float Le[3] = {L.Lemit.r, L.Lemit.g, L.Lemit.b};
            std::snprintf(b, sizeof b, "{\"kind\": \"disk\", \"nsamples\": %d, \"Le\": ", L.n_samples);
            lights += b;
            DumpSink::arr(lights, Le, 3);
            lights += ", \"o2w\": ";
            DumpSink::arr(lights, L.disk.o2w.m, 16);
            const float sc[4] = {L.disk.radius, L.disk.height, L.disk.inner_radius, L.disk.phi_max};
            lights += ", \"radius_height_inner_phimax\": ";
            DumpSink::arr(lights, sc, 4);
        }
        lights += "}";
    }
    const Camera &c = o.camera;
    std::printf("{\"calls\": [\n%s],\n\"lights\": [\n%s],\n\"camera\": {\"width\": %d, \"height\": %d, \"eye\": ",
                sink.out.c_str(), lights.c_str(), c.width, c.height);
    std::string cam;
    DumpSink::arr(cam, c.eye, 3); cam += ", \"fwd\": ";
    DumpSink::arr(cam, c.fwd, 3); cam += ", \"right\": ";
    DumpSink::arr(cam, c.right, 3); cam += ", \"up\": ";
    DumpSink::arr(cam, c.up, 3);
    {
        static const char *names[] = {"none", "box", "triangle", "gaussian", "mitchell"};
        char b[512];
        std::snprintf(b, sizeof b, ", \"device_camera\": %d, \"xsamples\": %d, \"ysamples\": %d, \"jitter\": %d, "
                      "\"lens_radius\": %.9g, \"focal_distance\": %.9g, \"sample_seed\": %u, \"filter\": {\"type\": \"%s\", "
                      "\"xwidth\": %.9g, \"ywidth\": %.9g, \"a\": %.9g, \"b\": %.9g}",
                      c.device_camera ? 1 : 0, c.xsamples, c.ysamples, c.jitter ? 1 : 0, c.lens_radius, c.focal_distance,
                      c.sample_seed, names[c.filter.type], c.filter.xwidth, c.filter.ywidth, c.filter.a, c.filter.b);
        cam += b;
    }
    const pm_render_params &p = o.settings.params;
    /* the light selection table of PM_ALL_LIGHTS as pm_commit would build it
     * (host only); [] for a scene that emits nothing */
    std::string cdf = "[";
    {
        std::vector<int> types;
        std::vector<float> rgb, areas, table(o.lights.size());
        bool known = true; /* a distant light's weight needs the commit's world sphere: no table here */
        for (const Light &L : o.lights) {
            const bool delta = L.kind == Light::Point || L.kind == Light::Distant;
            const RGB c = delta ? L.intensity : L.Lemit;
            types.push_back(L.kind == Light::Point ? PM_LIGHT_POINT : L.kind == Light::Distant ? PM_LIGHT_DISTANT :
                            L.kind == Light::AreaMesh ? PM_LIGHT_AREA_MESH : PM_LIGHT_AREA_DISK);
            rgb.push_back(c.r); rgb.push_back(c.g); rgb.push_back(c.b);
            if (L.kind == Light::Distant) known = false;
            areas.push_back(delta ? 0.f : lightArea(L));
        }
        if (!o.lights.empty() && known &&
            pm_light_selection_cdf(types.data(), rgb.data(), areas.data(), (int)types.size(), table.data()) == PM_OK) {
            cdf.clear();
            DumpSink::arr(cdf, table.data(), table.size());
            cdf.pop_back();
        }
    }
    std::printf("%s},\n\"renderer\": \"%s\", \"paths\": %lld, \"passes\": %d, \"gather\": %d, \"film\": \"%s\", "
                "\"light_source_index\": %d, \"light_cdf\": %s], \"resample\": %d, \"final_gather\": %d, \"caustic_map\": %d, \"warnings\": %d}\n",
                cam.c_str(), o.renderer.c_str(), (long long)p.paths_per_pass, p.passes, p.gather_structure,
                o.film_filename.c_str(), p.light_source_index, cdf.c_str(), o.resample ? 1 : 0, o.settings.final_gather,
                o.settings.caustic_map ? 1 : 0, o.warnings);
    return 0;
}

/* a .pbrt scene through the plugin surface, as pbrt-v2 + the reference would run it */
/* --light N|all: the light the photon paths start on (all: PM_ALL_LIGHTS) */
int parse_light(const std::string &v) {
    if (v == "all") return PM_ALL_LIGHTS;
    char *end = nullptr;
    const long k = std::strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || k < -1 || k > 2147483647L) throw Error("--light " + v + ": expected a light index, -1 or \"all\"");
    return (int)k;
}
void check_light(int k, size_t n_lights) {
    if (k != PM_ALL_LIGHTS && (k < 0 || (size_t)k >= n_lights))
        throw Error("--light " + std::to_string(k) + " out of range: the scene has " + std::to_string(n_lights) + " lights");
}

int render_pbrt(const std::string &path, std::string out, const std::string &renderer, long long paths, int passes,
                const std::string &structure, const std::string &light, const CameraFlags &cflags = CameraFlags()) {
    CudaRenderInit(0);
    PbrtOptions o;
    o.specular_override = g_specular;
    CudaApiSink sink;
    PbrtParser parser;
    parser.parseFile(path, sink, o);
    if (!renderer.empty()) o.renderer = renderer;
    pm_render_params &p = o.settings.params;
    if (paths > 0) p.paths_per_pass = paths;
    if (passes > 0) p.passes = passes;
    if (!structure.empty()) p.gather_structure = structure == "kd" ? PM_GATHER_KDTREE : PM_GATHER_GRID;
    if (!light.empty()) { p.light_source_index = parse_light(light); check_light(p.light_source_index, o.lights.size()); }
    if (out.empty()) out = o.film_filename;
    apply_camera_flags(cflags, o);
    apply_final_gather_flags(o);
    CudaRender *render = CreateCudaRenderer(o.settings, o.renderer);
    PixelFilm film(o.camera.width, o.camera.height, out); /* the device film writes one value per pixel */
    o.camera.film = &film;
    render->Render(o.lights, o.camera);
    if (auto *pm = dynamic_cast<PhotonMappingRenderer *>(render->subRenderer()))
        std::printf("{\"renderer\": \"photonmapping\", \"paths_emitted\": %lld, \"photons_valid\": %lld, "
                    "\"gather_points\": %lld}\n",
                    (long long)pm->stats.paths_emitted, (long long)pm->stats.photons_valid,
                    (long long)pm->stats.gather_points);
    else
        std::printf("{\"renderer\": \"simple\", \"samples\": %lld}\n",
                    (long long)static_cast<SimpleRenderer *>(render->subRenderer())->stats.gather_points);
    delete render;
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    std::string scene = "cornell", out, structure, renderer, pbrt, light;
    bool dump_only = false;
    int W = 64, H = 48;
    long long paths = 512 * 512;
    int passes = 1;
    bool instanced = false, have_cam = false, paths_set = false, passes_set = false;
    float cam[12] = {0};
    CameraFlags cflags;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        if (a == "--selftest") return selftest();
        else if (a == "--scene") scene = next();
        else if (a == "--width") W = std::atoi(next());
        else if (a == "--height") H = std::atoi(next());
        else if (a == "--paths") { paths = std::atoll(next()); paths_set = true; }
        else if (a == "--passes") { passes = std::atoi(next()); passes_set = true; }
        else if (a == "--structure") structure = next();
        else if (a == "--light") light = next();
        else if (a == "--instanced") instanced = true;
        else if (a == "--renderer") renderer = next();
        else if (a == "--pbrt") pbrt = next();
        else if (a == "--dump") dump_only = true;
        else if (a == "--specular") {
            g_specular = next();
            if (g_specular != "pbrt" && g_specular != "reference") {
                std::fprintf(stderr, "--specular %s: expected pbrt or reference\n", g_specular.c_str());
                return 2;
            }
        }
        else if (a == "--out") out = next();
        else if (a == "--spp") cflags.spp = next();
        else if (a == "--filter") cflags.filter = next();
        else if (a == "--lens") cflags.lens = next();
        else if (a == "--no-jitter") cflags.no_jitter = true;
        else if (a == "--resample") cflags.resample = true;
        else if (a == "--final-gather") {
            g_final_gather = std::atoi(next());
            if (g_final_gather < 0 || g_final_gather > PM_FG_MAX) {
                std::fprintf(stderr, "--final-gather %d: expected 0..%d\n", g_final_gather, PM_FG_MAX);
                return 2;
            }
        }
        else if (a == "--caustic-map") g_caustic_map = true;
        else if (a == "--camera") {
            for (float &c : cam) c = std::strtof(next(), nullptr);
            have_cam = true;
        } else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (!pbrt.empty()) {
        try {
            if (dump_only) return dump(pbrt, cflags);
            return render_pbrt(pbrt, out, renderer, paths_set ? paths : 0, passes_set ? passes : 0, structure, light, cflags);
        } catch (const Error &e) {
            std::fprintf(stderr, "pm_render_cli: %s\n", e.what());
            return 1;
        }
    }
    if (cflags.any() || g_final_gather >= 0 || g_caustic_map) {
        std::fprintf(stderr, "--spp, --filter, --lens, --no-jitter, --resample, --final-gather and --caustic-map need --pbrt scene.pbrt\n");
        return 2;
    }
    if (out.empty()) out = "out.pfm";
    if (scene != "cornell" || !have_cam) {
        std::fprintf(stderr, "usage: %s --scene cornell --camera <12 floats> [--width W --height H] [--light N|all] "
                             "--out f.pfm\n", argv[0]);
        return 2;
    }
    try {
        CudaRenderInit(0);
        std::vector<Light> lights;
        cornell(instanced, lights);
        RenderSettings settings;
        settings.params.paths_per_pass = paths;
        settings.params.passes = passes;
        settings.params.gather_structure = structure == "kd" ? PM_GATHER_KDTREE : PM_GATHER_GRID;
        if (!light.empty()) { settings.params.light_source_index = parse_light(light); check_light(settings.params.light_source_index, lights.size()); }
        CudaRender *render = CreateCudaRenderer(settings, renderer.empty() ? "photonmapping" : renderer);
        PixelFilm film(W, H, out);
        Camera camera;
        camera.pinhole = true;
        std::memcpy(camera.eye, cam, 12);
        std::memcpy(camera.fwd, cam + 3, 12);
        std::memcpy(camera.right, cam + 6, 12);
        std::memcpy(camera.up, cam + 9, 12);
        camera.width = W;
        camera.height = H;
        camera.film = &film;
        render->Render(lights, camera);
        auto *pmr = dynamic_cast<PhotonMappingRenderer *>(render->subRenderer());
        const pm_stats &st = pmr ? pmr->stats : static_cast<SimpleRenderer *>(render->subRenderer())->stats;
        std::printf("{\"paths_emitted\": %lld, \"photons_valid\": %lld, \"gather_points\": %lld}\n",
                    (long long)st.paths_emitted, (long long)st.photons_valid, (long long)st.gather_points);
        delete render;
    } catch (const Error &e) {
        std::fprintf(stderr, "pm_render_cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
