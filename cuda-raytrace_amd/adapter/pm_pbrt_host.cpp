/*
 * pm_pbrt_host.cpp — a pbrt-v2-shaped host for the plugin boundary: it makes
 * the calls pbrt-v2's api.cpp (the reference's fork) makes, in its order,
 * with pbrt objects (adapter/pbrt_stub):
 *   pbrtInit            -> CudaRenderInit()
 *   Shape directives    -> CreateCudaShape(name, Reference<Shape>, currentInstance, Material*, areaLightIndex)
 *   ObjectInstance      -> CudaObjectInstance(&instance, Transform)
 *   MakeRenderer "cuda" -> CreateCudaRenderer(sampler, camera, ParamSet, rendername)
 *   pbrtWorldEnd        -> renderer->Render(scene); delete renderer
 * for the Cornell box of pmrender/scenes.py, with a one-sample-per-pixel
 * sampler (pixel centres, raster order; light 2D randoms from a fixed hash),
 * a pinhole camera and a film that keeps what Film::AddSample receives. The
 * rays, light randoms and film image go to a binary file, so a test can
 * render the same inputs through the stage driver and compare bit for bit.
 *
 * usage: pm_pbrt_host --out f.bin [--width W --height H --paths N
 *        --photonmap grid|kdtree --renderer photonmap|simple --nsamples S --instanced
 *        --quad-light]   (the box's own 130 x 105 quad light, a trianglemesh, instead of the disk)
 *        [--two-lights]  (scenes/cornell-two-lights.pbrt: the disk, then a blue quad light on the green wall)
 *        [--sun]         (scenes/cornell-sun.pbrt: a DistantLight through the open front, the last light)
 *        [--lightsource K]  (Renderer "cuda" "integer lightsource" [K]; -1: photons from every light)
 *        [--caustic]     (scenes/caustic-fresnel.pbrt: a GlassMaterial sphere and a MirrorMaterial sphere instead of the blocks)
 *        [--specular pbrt|reference]  (Renderer "cuda" "string specular": pbrt = the Fresnel model with the materials' Kr, Kt, index)
 *        [--caustic-map]  (Renderer "cuda" "bool causticmap" ["true"]: the caustic map at the eye hits; with --final-gather)
 *        [--final-gather N]  (Renderer "cuda" "integer finalgathersamples" [N]: N gather rays per eye hit, pm_render_final_gather)
 *        [--resample]    (Renderer "cuda" "bool resample" ["true"]: a fresh eye sample per pass; --lensradius R --focaldistance F --passes P)
 * The header's third word is the number of light 2D samples per ray
 * (nsamples per area light).
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "core/film.h"
#include "cudaapi.h"
#include "lights/diffuse.h"
#include "lights/distant.h"
#include "materials/glass.h"
#include "materials/matte.h"
#include "materials/mirror.h"
#include "shapes/disk.h"
#include "shapes/sphere.h"
#include "shapes/trianglemesh.h"

namespace {

struct Opts {
    int W = 64, H = 48, paths = 16384, nsamples = 1;
    std::string photonmap = "grid", renderer = "photonmap", out;
    bool instanced = false, quad_light = false, two_lights = false, sun = false;
    bool caustic = false; /* --caustic (scenes/caustic-fresnel.pbrt): a glass and a mirror sphere instead of the blocks */
    std::string specular; /* --specular pbrt|reference: the Renderer "cuda" ParamSet's "string specular" */
    bool checker = false; /* --checker (scenes/cornell-checker.pbrt): the floor's Kd is a checkerboard */
    int lightsource = 0;
    bool lightsource_set = false;
    /* --devicecamera: the Renderer "cuda" ParamSet's device camera + film */
    int devicecamera = 0, xsamples = 1, ysamples = 1, jitter = 1;
    float lensradius = 0.f, focaldistance = 0.f, xwidth = 0.f;
    std::string pixelfilter;
    bool resample = false; /* --resample: the ParamSet's "bool resample" (with --lensradius / --focaldistance / --passes) */
    int passes = 1;
    int final_gather = 0; /* --final-gather N: the ParamSet's "integer finalgathersamples" */
    bool caustic_map = false; /* --caustic-map: the ParamSet's "bool causticmap" */
};

/* pixel centres in raster order, one sample per pixel; light 2D randoms:
 * a fixed integer hash of (pixel, dimension) */
class CentreSampler : public Sampler {
public:
    CentreSampler(int W, int H) : Sampler(0, W, 0, H, 1, 0.f, 1.f), next(0), W_(W), H_(H) {}
    int GetMoreSamples(Sample *sample, RNG &) {
        if (next >= W_ * H_) return 0;
        const int x = next % W_, y = next / W_;
        sample->imageX = (float)x + 0.5f;
        sample->imageY = (float)y + 0.5f;
        sample->lensU = sample->lensV = 0.5f;
        sample->time = 0.f;
        for (size_t d = 0; d < sample->n2D.size(); ++d)
            for (uint32_t k = 0; k < 2 * sample->n2D[d]; ++k) {
                sample->twoD[d][k] = hash01((uint32_t)next * 977u + (uint32_t)(d * 64 + k));
                rand2d.push_back(sample->twoD[d][k]);
            }
        ++next;
        return 1;
    }
    int MaximumSampleCount() { return 1; }
    int RoundSize(int size) const { return size; }
    std::vector<float> rand2d; /* every light 2D random handed out, in sample order */
private:
    static float hash01(uint32_t v) {
        v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
        return (float)(v >> 8) * (1.f / 16777216.f);
    }
    int next, W_, H_;
};

/* the pinhole of pmrender/scenes.py pinhole(): eye (278, 273, -800) looking
 * +z, fov 39.3 deg over the shorter axis, image x towards -x world */
class PinholeCamera : public Camera {
public:
    PinholeCamera(Film *f, int W, int H) : Camera(f), W_(W), H_(H) {
        const double t = std::tan(39.3 * M_PI / 180.0 / 2.0);
        sx = (float)(W >= H ? t * W / H : t);
        sy = (float)(W >= H ? t : t * H / W);
    }
    float GenerateRay(const CameraSample &cs, Ray *ray) const {
        const float u = 2.f * cs.imageX / (float)W_ - 1.f, v = 1.f - 2.f * cs.imageY / (float)H_;
        Vector d(-u * sx, v * sy, 1.f);
        ray->o = Point(278.f, 273.f, -800.f);
        ray->d = Normalize(d);
        return 1.f;
    }
private:
    int W_, H_;
    float sx, sy;
};

class KeepFilm : public Film {
public:
    KeepFilm(int W, int H) : Film(W, H), rgb(3 * (size_t)W * H, 0.f) {}
    void AddSample(const CameraSample &s, const Spectrum &L) {
        const int x = (int)std::floor(s.imageX), y = (int)std::floor(s.imageY);
        if (x < 0 || y < 0 || x >= xResolution || y >= yResolution) return;
        float c[3];
        L.ToRGB(c);
        std::memcpy(&rgb[3 * ((size_t)y * xResolution + x)], c, sizeof c);
        ++added;
    }
    void GetSampleExtent(int *xs, int *xe, int *ys, int *ye) const { *xs = 0; *xe = xResolution; *ys = 0; *ye = yResolution; }
    void WriteImage(float) { ++written; }
    std::vector<float> rgb;
    long added = 0;
    int written = 0;
};

/* records the rays the renderer asked for (for the stage-driver comparison) */
class RecordingCamera : public PinholeCamera {
public:
    using PinholeCamera::PinholeCamera;
    float GenerateRayDifferential(const CameraSample &cs, RayDifferential *rd) const {
        const float w = PinholeCamera::GenerateRayDifferential(cs, rd);
        rays.insert(rays.end(), {rd->o.x, rd->o.y, rd->o.z, rd->d.x, rd->d.y, rd->d.z});
        return w;
    }
    mutable std::vector<float> rays;
};

Reference<Texture<Spectrum> > constant(float r, float g, float b) {
    const float c[3] = {r, g, b};
    return Reference<Texture<Spectrum> >(new ConstantTexture<Spectrum>(RGBSpectrum::FromRGB(c)));
}

Reference<Shape> quads(const Transform *o2w, const std::vector<std::vector<float> > &qs, const float *uv = NULL) {
    std::vector<Point> P;
    std::vector<int> idx;
    for (const std::vector<float> &q : qs) {
        const int b = (int)P.size();
        for (int k = 0; k < 4; ++k) P.push_back(Point(q[3 * k], q[3 * k + 1], q[3 * k + 2]));
        idx.insert(idx.end(), {b, b + 1, b + 2, b, b + 2, b + 3});
    }
    return Reference<Shape>(new TriangleMesh(o2w, o2w, false, (int)idx.size() / 3, (int)P.size(), idx.data(), P.data(),
                                             NULL, NULL, uv));
}

int run(const Opts &o) {
    static const Transform identity;
    /* pbrtInit */
    CudaRenderInit();
    Reference<Material> white(new MatteMaterial(constant(0.73f, 0.73f, 0.73f), NULL, NULL));
    Reference<Material> red(new MatteMaterial(constant(0.63f, 0.065f, 0.05f), NULL, NULL));
    Reference<Material> green(new MatteMaterial(constant(0.14f, 0.45f, 0.091f), NULL, NULL));
    Reference<Material> black(new MatteMaterial(constant(0.f, 0.f, 0.f), NULL, NULL));
    /* WorldBegin ... Shape directives (pmrender/scenes.py cornell_box order) */
    Reference<Shape> s;
    Reference<Material> checks; /* lives as long as the scene: materials are keyed by address */
    if (o.checker) { /* Texture "checks" "color" "checkerboard" uscale 8 vscale 8 aamode none; the floor a mesh of its own with uvs */
        checks = Reference<Material>(new MatteMaterial(
            Reference<Texture<Spectrum> >(new Checkerboard2DTexture<Spectrum>(new UVMapping2D(8.f, 8.f, 0.f, 0.f), constant(0.73f, 0.73f, 0.73f),
                                                                             constant(0.15f, 0.17f, 0.25f), "none")), NULL, NULL));
        const float uv[8] = {0, 0, 1, 0, 1, 1, 0, 1};
        s = quads(&identity, {{552.8f, 0, 0, 0, 0, 0, 0, 0, 559.2f, 549.6f, 0, 559.2f}}, uv);
        CreateCudaShape("trianglemesh", s, NULL, checks.GetPtr(), -1);
        s = quads(&identity, {{556.0f, 548.8f, 0, 556.0f, 548.8f, 559.2f, 0, 548.8f, 559.2f, 0, 548.8f, 0},
                              {549.6f, 0, 559.2f, 0, 0, 559.2f, 0, 548.8f, 559.2f, 556.0f, 548.8f, 559.2f}});
    } else
    s = quads(&identity, {{552.8f, 0, 0, 0, 0, 0, 0, 0, 559.2f, 549.6f, 0, 559.2f},
                          {556.0f, 548.8f, 0, 556.0f, 548.8f, 559.2f, 0, 548.8f, 559.2f, 0, 548.8f, 0},
                          {549.6f, 0, 559.2f, 0, 0, 559.2f, 0, 548.8f, 559.2f, 556.0f, 548.8f, 559.2f}});
    CreateCudaShape("trianglemesh", s, NULL, white.GetPtr(), -1);
    s = quads(&identity, {{0, 0, 559.2f, 0, 0, 0, 0, 548.8f, 0, 0, 548.8f, 559.2f}});
    CreateCudaShape("trianglemesh", s, NULL, green.GetPtr(), -1);
    s = quads(&identity, {{552.8f, 0, 0, 549.6f, 0, 559.2f, 556.0f, 548.8f, 559.2f, 556.0f, 548.8f, 0}});
    CreateCudaShape("trianglemesh", s, NULL, red.GetPtr(), -1);
    /* --caustic: Material "glass" Kr 1 Kt 1 index 1.5 on a sphere r 100 at (370, 100, 250),
     * Material "mirror" Kr 0.9 on a sphere r 90 at (150, 90, 380) (pmrender/scenes.py caustic_fresnel) */
    Reference<Material> glass(new GlassMaterial(constant(1.f, 1.f, 1.f), constant(1.f, 1.f, 1.f),
                                                Reference<Texture<float> >(new ConstantTexture<float>(1.5f)), NULL));
    Reference<Material> mirror(new MirrorMaterial(constant(0.9f, 0.9f, 0.9f), NULL));
    float g[4][4] = {{1, 0, 0, 370.f}, {0, 1, 0, 100.f}, {0, 0, 1, 250.f}, {0, 0, 0, 1}};
    float gi[4][4] = {{1, 0, 0, -370.f}, {0, 1, 0, -100.f}, {0, 0, 1, -250.f}, {0, 0, 0, 1}};
    float r[4][4] = {{1, 0, 0, 150.f}, {0, 1, 0, 90.f}, {0, 0, 1, 380.f}, {0, 0, 0, 1}};
    float ri[4][4] = {{1, 0, 0, -150.f}, {0, 1, 0, -90.f}, {0, 0, 1, -380.f}, {0, 0, 0, 1}};
    static const Transform g2w{Matrix4x4(g), Matrix4x4(gi)}, w2g{Matrix4x4(gi), Matrix4x4(g)};
    static const Transform r2w{Matrix4x4(r), Matrix4x4(ri)}, w2r{Matrix4x4(ri), Matrix4x4(r)};
    std::vector<Reference<Primitive> > blocks; /* RenderOptions::instances["blocks"] */
    std::vector<Reference<Primitive> > *inst = o.instanced ? &blocks : NULL;
    s = quads(&identity, {{130, 165, 65, 82, 165, 225, 240, 165, 272, 290, 165, 114},
                          {290, 0, 114, 290, 165, 114, 240, 165, 272, 240, 0, 272},
                          {130, 0, 65, 130, 165, 65, 290, 165, 114, 290, 0, 114},
                          {82, 0, 225, 82, 165, 225, 130, 165, 65, 130, 0, 65},
                          {240, 0, 272, 240, 165, 272, 82, 165, 225, 82, 0, 225}});
    if (!o.caustic) CreateCudaShape("trianglemesh", s, inst, white.GetPtr(), -1);
    s = quads(&identity, {{423, 330, 247, 265, 330, 296, 314, 330, 456, 472, 330, 406},
                          {423, 0, 247, 423, 330, 247, 472, 330, 406, 472, 0, 406},
                          {472, 0, 406, 472, 330, 406, 314, 330, 456, 314, 0, 456},
                          {314, 0, 456, 314, 330, 456, 265, 330, 296, 265, 0, 296},
                          {265, 0, 296, 265, 330, 296, 423, 330, 247, 423, 0, 247}});
    if (!o.caustic) CreateCudaShape("trianglemesh", s, inst, white.GetPtr(), -1);
    if (o.instanced && !o.caustic) CudaObjectInstance(&blocks, identity); /* ObjectInstance "blocks" */
    if (o.caustic) {
        s = Reference<Shape>(new Sphere(&g2w, &w2g, false, 100.f, -100.f, 100.f, 360.f));
        CreateCudaShape("sphere", s, NULL, glass.GetPtr(), -1);
        s = Reference<Shape>(new Sphere(&r2w, &w2r, false, 90.f, -90.f, 90.f, 360.f));
        CreateCudaShape("sphere", s, NULL, mirror.GetPtr(), -1);
    }
    /* AttributeBegin; Translate 278 548.7 279.5; Rotate 90 1 0 0;
     * AreaLightSource "diffuse" "rgb L" [17 17 17]; Shape "disk" "float radius" 65 */
    float m[4][4] = {{1, 0, 0, 278.f}, {0, 0, -1, 548.7f}, {0, 1, 0, 279.5f}, {0, 0, 0, 1}};
    float mi[4][4] = {{1, 0, 0, -278.f}, {0, 0, 1, -279.5f}, {0, -1, 0, 548.7f}, {0, 0, 0, 1}};
    static const Transform light2world{Matrix4x4(m), Matrix4x4(mi)}, world2light{Matrix4x4(mi), Matrix4x4(m)};
    Reference<Shape> disk(new Disk(&light2world, &world2light, false, 0.f, 65.f, 0.f, 360.f));
    /* --quad-light (scenes/cornell-quad-light.pbrt): AreaLightSource "diffuse" on
     * Shape "trianglemesh", the quad wound to face down */
    Reference<Shape> emitter = o.quad_light ? quads(&identity, {{343, 548.7f, 227, 343, 548.7f, 332, 213, 548.7f, 332, 213, 548.7f, 227}})
                                            : disk;
    const float Le[3] = {17.f, 17.f, 17.f};
    DiffuseAreaLight *area = new DiffuseAreaLight(o.quad_light ? identity : light2world,
                                                  RGBSpectrum::FromRGB(Le, SPECTRUM_ILLUMINANT), o.nsamples, emitter);
    Scene scene;
    scene.lights.push_back(area);
    CreateCudaShape(o.quad_light ? "trianglemesh" : "disk", emitter, NULL, black.GetPtr(), 0);
    /* --two-lights (scenes/cornell-two-lights.pbrt): AreaLightSource "diffuse"
     * "rgb L" [4 8 20] on a quad just off the green wall, wound to face +x */
    DiffuseAreaLight *area2 = NULL;
    if (o.two_lights) {
        Reference<Shape> wallq = quads(&identity, {{1, 200, 230, 1, 300, 230, 1, 300, 330, 1, 200, 330}});
        const float Le2[3] = {4.f, 8.f, 20.f};
        area2 = new DiffuseAreaLight(identity, RGBSpectrum::FromRGB(Le2, SPECTRUM_ILLUMINANT), o.nsamples, wallq);
        scene.lights.push_back(area2);
        CreateCudaShape("trianglemesh", wallq, NULL, black.GetPtr(), 1);
    }
    /* --sun (scenes/cornell-sun.pbrt): LightSource "distant" "rgb L" [3 2.7 2.1]
     * "point from" [0 120 -400] "point to" [0 0 0], the last light */
    DistantLight *sun = NULL;
    if (o.sun) {
        const float Ls[3] = {3.f, 2.7f, 2.1f};
        sun = new DistantLight(identity, RGBSpectrum::FromRGB(Ls, SPECTRUM_ILLUMINANT), Vector(0.f, 120.f, -400.f));
        scene.lights.push_back(sun);
    }
    /* MakeRenderer: Renderer "cuda" */
    KeepFilm *film = new KeepFilm(o.W, o.H);
    RecordingCamera *camera = new RecordingCamera(film, o.W, o.H);
    ParamSet params; /* Renderer "cuda" "integer photonpaths" [N] "string photonmap" [...] */
    params.AddInt("photonpaths", &o.paths, 1);
    params.AddString("photonmap", &o.photonmap, 1);
    if (o.lightsource_set) params.AddInt("lightsource", &o.lightsource, 1);
    if (!o.specular.empty()) params.AddString("specular", &o.specular, 1);
    if (o.devicecamera) {
        params.AddInt("devicecamera", &o.devicecamera, 1);
        params.AddInt("xsamples", &o.xsamples, 1);
        params.AddInt("ysamples", &o.ysamples, 1);
        params.AddInt("jitter", &o.jitter, 1);
        params.AddFloat("lensradius", &o.lensradius, 1);
        params.AddFloat("focaldistance", &o.focaldistance, 1);
        if (!o.pixelfilter.empty()) params.AddString("pixelfilter", &o.pixelfilter, 1);
        if (o.xwidth > 0.f) { params.AddFloat("xwidth", &o.xwidth, 1); params.AddFloat("ywidth", &o.xwidth, 1); }
    }
    if (o.resample) {
        params.AddBool("resample", &o.resample, 1);
        if (!o.devicecamera) { params.AddFloat("lensradius", &o.lensradius, 1); params.AddFloat("focaldistance", &o.focaldistance, 1); }
    }
    if (o.passes != 1) params.AddInt("passes", &o.passes, 1);
    if (o.final_gather) params.AddInt("finalgathersamples", &o.final_gather, 1);
    if (o.caustic_map) params.AddBool("causticmap", &o.caustic_map, 1);
    CentreSampler *sampler = new CentreSampler(o.W, o.H);
    Renderer *renderer = CreateCudaRenderer(sampler, camera, params, o.renderer == "simple" ? "simple" : "photonmap");
    /* pbrtWorldEnd */
    renderer->Render(&scene);
    FILE *f = std::fopen(o.out.c_str(), "wb");
    if (!f) { std::perror("fopen"); return 2; }
    const int hdr[4] = {o.W, o.H, o.nsamples * (o.two_lights ? 2 : 1), (int)film->written};
    std::fwrite(hdr, sizeof hdr, 1, f);
    std::fwrite(camera->rays.data(), sizeof(float), camera->rays.size(), f);
    std::fwrite(sampler->rand2d.data(), sizeof(float), sampler->rand2d.size(), f);
    std::fwrite(film->rgb.data(), sizeof(float), film->rgb.size(), f);
    std::fclose(f);
    std::printf("pm_pbrt_host: %ld samples added, image written %d time(s)\n", film->added, film->written);
    delete renderer; /* pbrt deletes its Renderer */
    delete area;
    delete area2;
    delete sun;
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    Opts o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
        if (a == "--width") o.W = std::stoi(val());
        else if (a == "--height") o.H = std::stoi(val());
        else if (a == "--paths") o.paths = std::stoi(val());
        else if (a == "--nsamples") o.nsamples = std::stoi(val());
        else if (a == "--photonmap") o.photonmap = val();
        else if (a == "--renderer") o.renderer = val();
        else if (a == "--instanced") o.instanced = true;
        else if (a == "--quad-light") o.quad_light = true;
        else if (a == "--two-lights") o.two_lights = true;
        else if (a == "--sun") o.sun = true;
        else if (a == "--checker") o.checker = true;
        else if (a == "--caustic") o.caustic = true;
        else if (a == "--specular") o.specular = val();
        else if (a == "--lightsource") { o.lightsource = std::stoi(val()); o.lightsource_set = true; }
        else if (a == "--out") o.out = val();
        else if (a == "--devicecamera") o.devicecamera = 1;
        else if (a == "--xsamples") o.xsamples = std::stoi(val());
        else if (a == "--ysamples") o.ysamples = std::stoi(val());
        else if (a == "--no-jitter") o.jitter = 0;
        else if (a == "--lensradius") o.lensradius = std::stof(val());
        else if (a == "--focaldistance") o.focaldistance = std::stof(val());
        else if (a == "--pixelfilter") o.pixelfilter = val();
        else if (a == "--filterwidth") o.xwidth = std::stof(val());
        else if (a == "--resample") o.resample = true;
        else if (a == "--passes") o.passes = std::stoi(val());
        else if (a == "--final-gather") o.final_gather = std::stoi(val());
        else if (a == "--caustic-map") o.caustic_map = true;
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (o.out.empty()) { std::fprintf(stderr, "usage: %s --out f.bin [options]\n", argv[0]); return 2; }
    return run(o);
}
