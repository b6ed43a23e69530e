/*
 * cudaapi.cpp — the reference's pbrt plugin surface (cuda_render/cudaapi.cpp,
 * cudarender.cpp:105-196, util/shape/cuda{trianglemesh,sphere,disk}.cpp, util/light/cudalight.cpp:16-59,
 * util/material/cudamaterial.cpp:8-58, util/camera/pbrtcamera.cpp:57-122,
 * photonmappingrenderer.cpp:234-283) with pbrt-v2 types at the boundary and
 * the MI355X renderer underneath: pbrt objects are read exactly where the
 * reference reads them and handed to the C++ host layer (pm_cudarender.h),
 * which drives the C-ABI (include/pm_api.h). No HIP or OptiX header here.
 */
#include "cudaapi.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "core/film.h"
#include "cudarender.h"
#include "lights/diffuse.h"
#include "lights/distant.h"
#include "lights/point.h"
#include "materials/glass.h"
#include "materials/matte.h"
#include "materials/mirror.h"
#include "shapes/disk.h"
#include "shapes/sphere.h"
#include "shapes/trianglemesh.h"
#include "textures/checkerboard.h"
#include "textures/imagemap.h"
#include "textures/scale.h"

/* ---------------------------------------------------------------- pbrt -> descriptors */
static pmcuda::Transform toPm(const Transform &t) {
    pmcuda::Transform r;
    std::memcpy(r.m, &t.GetMatrix().m[0][0], sizeof r.m);
    std::memcpy(r.minv, &t.GetInverseMatrix().m[0][0], sizeof r.minv);
    return r;
}

static pmcuda::RGB toPm(const Spectrum &s) {
    float c[3];
    s.ToRGB(c);
    return pmcuda::RGB{c[0], c[1], c[2]};
}

/* what CudaShape::CreateCudaShape reads: the world-space triangle mesh
 * (cudatrianglemesh.cpp:18-66), the sphere's radius and transforms
 * (cudasphere.cpp:17-29), the disk's height / radii / phiMax and
 * ObjectToWorld (cudadisk.cpp:17-35). false: a shape the reference skips. */
static bool toPm(const Shape *s, pmcuda::Shape &d) {
    if (const TriangleMesh *tm = dynamic_cast<const TriangleMesh *>(s)) {
        d.P.resize(3 * (size_t)tm->nverts);
        for (int i = 0; i < tm->nverts; ++i) {
            d.P[3 * i] = tm->p[i].x; d.P[3 * i + 1] = tm->p[i].y; d.P[3 * i + 2] = tm->p[i].z;
        }
        d.indices.assign(tm->vertexIndex, tm->vertexIndex + 3 * (size_t)tm->ntris);
        if (tm->n) { /* copied raw, object-space pbrt normals (cudatrianglemesh.cpp:46-51) */
            d.N.resize(3 * (size_t)tm->nverts);
            for (int i = 0; i < tm->nverts; ++i) {
                d.N[3 * i] = tm->n[i].x; d.N[3 * i + 1] = tm->n[i].y; d.N[3 * i + 2] = tm->n[i].z;
            }
        }
        if (tm->uvs) d.uv.assign(tm->uvs, tm->uvs + 2 * (size_t)tm->nverts);
        return true;
    }
    if (const Sphere *sp = dynamic_cast<const Sphere *>(s)) {
        d.radius = sp->radius;
        d.o2w = toPm(*sp->ObjectToWorld);
        return true;
    }
    if (const Disk *dk = dynamic_cast<const Disk *>(s)) {
        d.radius = dk->radius;
        d.height = dk->height;
        d.inner_radius = dk->innerRadius;
        d.phi_max = dk->phiMax;
        d.o2w = toPm(*dk->ObjectToWorld);
        return true;
    }
    return false;
}

/* ---------------------------------------------------------------- CudaRender */
static int device_ordinal() {
    const char *e = std::getenv("PM_DEVICE");
    return e ? std::atoi(e) : 0;
}

CudaRender::CudaRender() : impl_(device_ordinal()), sampler_(NULL), camera_(NULL) {}

CudaRender::~CudaRender() { /* the sub-renderer's pbrt objects (photonmappingrenderer.cpp:25-29) */
    delete sampler_;
    delete camera_;
}

/* a pbrt spectrum texture as the operand of a Kd texture: a constant, or an
 * image with a UVMapping2D; false for anything else */
static bool toPmOperand(const Texture<Spectrum> *t, pmcuda::TexOperand &o) {
    DifferentialGeometry dg;
    if (dynamic_cast<const ConstantTexture<Spectrum> *>(t)) {
        o = pmcuda::TexOperand();
        o.rgb = toPm(t->Evaluate(dg));
        return true;
    }
    if (const ImageTexture<RGBSpectrum, Spectrum> *im = dynamic_cast<const ImageTexture<RGBSpectrum, Spectrum> *>(t)) {
        const UVMapping2D *uv = dynamic_cast<const UVMapping2D *>(im->mapping);
        if (!uv || !im->mipmap) return false;
        o = pmcuda::TexOperand();
        o.image = true;
        o.w = im->mipmap->Width(); o.h = im->mipmap->Height();
        o.wrap = im->mipmap->wrapMode == TEXTURE_BLACK ? PM_TEX_WRAP_BLACK
                 : im->mipmap->wrapMode == TEXTURE_CLAMP ? PM_TEX_WRAP_CLAMP : PM_TEX_WRAP_REPEAT;
        o.map[0] = uv->su; o.map[1] = uv->sv; o.map[2] = uv->du; o.map[3] = uv->dv;
        o.texels.resize(3 * (size_t)o.w * (size_t)o.h);
        for (int y = 0; y < o.h; ++y)
            for (int x = 0; x < o.w; ++x) im->mipmap->Texel(0, x, y).ToRGB(&o.texels[3 * ((size_t)y * o.w + x)]);
        return true; /* pbrt-v2 bakes the imagemap's scale into the texels: rgb stays 1 */
    }
    return false;
}

/* the Kd texture of a matte, for the classes the device evaluates per hit:
 * imagemap, checkerboard (2-D; its antialiasing is not reproduced) and scale,
 * over constant or image operands; null: the reference's single evaluation */
static std::shared_ptr<const pmcuda::TextureDesc> toPmTexture(const Texture<Spectrum> *t) {
    auto d = std::make_shared<pmcuda::TextureDesc>();
    if (const Checkerboard2DTexture<Spectrum> *c = dynamic_cast<const Checkerboard2DTexture<Spectrum> *>(t)) {
        const UVMapping2D *uv = dynamic_cast<const UVMapping2D *>(c->mapping);
        if (!uv || !toPmOperand(c->tex1.GetPtr(), d->op[0]) || !toPmOperand(c->tex2.GetPtr(), d->op[1])) return nullptr;
        d->kind = pmcuda::TextureDesc::Checker;
        d->map[0] = uv->su; d->map[1] = uv->sv; d->map[2] = uv->du; d->map[3] = uv->dv;
        return d;
    }
    if (const ScaleTexture<Spectrum, Spectrum> *s = dynamic_cast<const ScaleTexture<Spectrum, Spectrum> *>(t)) {
        if (!toPmOperand(s->tex1.GetPtr(), d->op[0]) || !toPmOperand(s->tex2.GetPtr(), d->op[1])) return nullptr;
        d->kind = pmcuda::TextureDesc::Scale;
        return d;
    }
    if (dynamic_cast<const ImageTexture<RGBSpectrum, Spectrum> *>(t) && toPmOperand(t, d->op[0])) return d;
    return nullptr; /* any other texture class: as today */
}

/* CudaMaterial::createCudaMeteral (cudamaterial.cpp:8-21): Kd / Kr evaluated
 * at a default DifferentialGeometry; anything else is matte 0.5 */
const pmcuda::Material *CudaRender::material(const Material *m) {
    auto it = materials_.find(m);
    if (it != materials_.end()) return &it->second;
    pmcuda::Material d;
    DifferentialGeometry dg;
    if (const MatteMaterial *mm = dynamic_cast<const MatteMaterial *>(m)) {
        d.kind = pmcuda::Material::Matte;
        d.k = toPm(mm->Kd->Evaluate(dg));
        d.kd_tex = toPmTexture(mm->Kd.GetPtr());
    } else if (const MirrorMaterial *mi = dynamic_cast<const MirrorMaterial *>(m)) {
        d.kind = pmcuda::Material::Mirror;
        d.k = toPm(mi->Kr->Evaluate(dg));
        d.kr = d.k; /* the physical model's parameters (flush decides whether they are used) */
    } else if (const GlassMaterial *gl = dynamic_cast<const GlassMaterial *>(m)) {
        d.kind = pmcuda::Material::Glass;
        d.k = pmcuda::RGB{1.f, 1.f, 1.f};
        d.kr = toPm(gl->Kr->Evaluate(dg));
        d.kt = toPm(gl->Kt->Evaluate(dg));
        d.index = gl->index->Evaluate(dg);
    } else {
        d.kind = pmcuda::Material::Unknown;
    }
    return &(materials_[m] = d);
}

void CudaRender::createCudaShape(const std::string &name, Reference<Shape> &shape,
                                 std::vector<Reference<Primitive> > *currentInstance, const Material *kMaterial,
                                 int lightIndex) {
    pmcuda::Shape d;
    if (!toPm(shape.GetPtr(), d)) {
        Warning("shape:%s not implemented yet", name.c_str()); /* cudarender.cpp:141-144 */
        return;
    }
    /* kept until Render: pbrt hands over the Renderer's ParamSet (its "specular"
     * key decides how mirrors and glass go in) after the shapes */
    Pending p;
    p.name = name; p.shape = d; p.key = currentInstance; p.material = material(kMaterial); p.light = lightIndex;
    pending_.push_back(p);
}

/* the kept scene calls, in their order, once the specular model is known */
void CudaRender::flush() {
    for (auto &m : materials_)
        if (m.second.kind == pmcuda::Material::Mirror || m.second.kind == pmcuda::Material::Glass) m.second.physical = physical_;
    try {
        for (const Pending &p : pending_) {
            if (p.instance) impl_.objectInstance(p.key, p.tr);
            else impl_.createCudaShape(p.name, p.shape, p.key, p.material, p.light);
        }
    } catch (const pmcuda::Error &e) {
        Severe("%s", e.what());
    }
    pending_.clear();
}

void CudaRender::objectInstance(std::vector<Reference<Primitive> > *instance, const Transform &tr) {
    Pending p;
    p.instance = true; p.key = instance; p.tr = toPm(tr);
    pending_.push_back(p);
}

void CudaRender::createSubRenderer(Sampler *sampler, Camera *camera, const ParamSet &params,
                                   const std::string &rendername) {
    sampler_ = sampler;
    camera_ = camera;
    /* the reference hard-codes its constants (pm_render_params defaults);
     * the ParamSet may scale the photon pass, which the reference cannot */
    pmcuda::RenderSettings s;
    s.params.paths_per_pass = params.FindOneInt("photonpaths", (int)s.params.paths_per_pass);
    s.params.passes = params.FindOneInt("passes", s.params.passes);
    /* "integer finalgathersamples" [N], N in 1..256: the photon-mapping renderer shoots N gather rays from
     * every eye hit and takes the kNN estimate at their hits (pm_render_final_gather); 0 (the default): pm_render */
    s.final_gather = params.FindOneInt("finalgathersamples", 0);
    if (s.final_gather < 0 || s.final_gather > PM_FG_MAX) {
        Warning("Renderer \"finalgathersamples\" %d outside 0..%d: final gathering is off", s.final_gather, PM_FG_MAX);
        s.final_gather = 0;
    }
    /* "bool causticmap" ["true"]: the caustic map looked up at the eye hits (pm_set_caustic_map), with final gathering only */
    s.caustic_map = params.FindOneBool("causticmap", false);
    if (s.caustic_map && s.final_gather == 0) {
        Warning("Renderer \"causticmap\" needs \"finalgathersamples\": the caustic map is off%s", "");
        s.caustic_map = false;
    }
    if (params.FindOneString("photonmap", "grid") == "kdtree") s.params.gather_structure = PM_GATHER_KDTREE;
    /* the light the photon paths start on; -1 (PM_ALL_LIGHTS): every light, picked per path by power */
    s.params.light_source_index = params.FindOneInt("lightsource", s.params.light_source_index);
    /* "string specular" "pbrt": MirrorMaterial's Kr and GlassMaterial's Kr, Kt,
     * index go into the physical model (pm_add_material_specular); "reference"
     * (the default): the reference's mirror and glass */
    const std::string spec = params.FindOneString("specular", "reference");
    if (spec != "pbrt" && spec != "reference") Warning("Renderer \"specular\" \"%s\" unknown: using \"reference\"", spec.c_str());
    physical_ = spec == "pbrt";
    /* the device camera + film (pm_set_camera): "integer devicecamera" [1]
     * hands the camera to the device (strata "integer xsamples" / "ysamples",
     * "integer jitter" [0|1], "integer sampleseed"; thin lens "float
     * lensradius" / "focaldistance"; "string pixelfilter" "box" | "triangle" |
     * "gaussian" | "mitchell" with "float xwidth" / "ywidth" / "alpha" / "B" /
     * "C", pbrt's defaults). Without it the sampler's rays are used as before. */
    devcam_ = pmcuda::Camera();
    devcam_.device_camera = params.FindOneInt("devicecamera", 0) != 0;
    if (devcam_.device_camera) {
        devcam_.xsamples = params.FindOneInt("xsamples", 1);
        devcam_.ysamples = params.FindOneInt("ysamples", 1);
        devcam_.jitter = params.FindOneInt("jitter", 1) != 0;
        devcam_.sample_seed = (uint32_t)params.FindOneInt("sampleseed", 0);
        devcam_.lens_radius = params.FindOneFloat("lensradius", 0.f);
        devcam_.focal_distance = params.FindOneFloat("focaldistance", 0.f);
        const std::string fn = params.FindOneString("pixelfilter", "box");
        pm_filter f = {PM_FILTER_BOX, 0.5f, 0.5f, 0.f, 0.f};
        if (fn == "triangle") f = pm_filter{PM_FILTER_TRIANGLE, 2.f, 2.f, 0.f, 0.f};
        else if (fn == "gaussian") f = pm_filter{PM_FILTER_GAUSSIAN, 2.f, 2.f, params.FindOneFloat("alpha", 2.f), 0.f};
        else if (fn == "mitchell")
            f = pm_filter{PM_FILTER_MITCHELL, 2.f, 2.f, params.FindOneFloat("B", 1.f / 3.f), params.FindOneFloat("C", 1.f / 3.f)};
        else if (fn != "box") Severe("Renderer \"cuda\": pixelfilter \"%s\" not supported", fn.c_str());
        f.xwidth = params.FindOneFloat("xwidth", f.xwidth);
        f.ywidth = params.FindOneFloat("ywidth", f.ywidth);
        devcam_.filter = f;
    }
    /* "bool resample" ["true"]: a fresh jitter and lens sample per pixel every
     * photon pass (pm_render_resampled). The camera goes to the device with
     * one stratum, no film and jitter on, whatever "devicecamera" and its keys
     * say (a filter or strata there warn); "float lensradius" /
     * "focaldistance" and "integer sampleseed" are read as above. */
    if (params.FindOneBool("resample", false)) {
        if (!devcam_.device_camera) {
            devcam_.sample_seed = (uint32_t)params.FindOneInt("sampleseed", 0);
            devcam_.lens_radius = params.FindOneFloat("lensradius", 0.f);
            devcam_.focal_distance = params.FindOneFloat("focaldistance", 0.f);
        }
        const bool strata = devcam_.device_camera && devcam_.xsamples * devcam_.ysamples > 1;
        const bool filtered = devcam_.device_camera && params.FindOneString("pixelfilter", "") != "";
        pmcuda::resampleCamera(devcam_);
        if (strata) Warning("Renderer \"cuda\": xsamples / ysamples ignored under \"resample\" (the passes are the samples)");
        if (filtered) Warning("Renderer \"cuda\": pixelfilter ignored under \"resample\"");
    }
    impl_.createSubRenderer(s, rendername);
}

/* Film::AddSample of each eye sample in sampler order, with the reference's
 * host-side sanitising (photonmappingrenderer.cpp:247-272) */
namespace {
struct PbrtFilm : pmcuda::Film {
    ::Film *film;
    const std::vector<CameraSample> *samples;
    size_t next = 0;
    void AddSample(const pmcuda::CameraSample &cs, const float rgb[3]) override {
        Spectrum result = RGBSpectrum::FromRGB(rgb);
        if (result.HasNaNs()) {
            Error("Not-a-number radiance value returned for image sample.  Setting to black.");
            result = Spectrum(0.f);
        } else if (result.y() < -1e-5f) {
            Error("Negative luminance value, %f, returned for image sample.  Setting to black.", result.y());
            result = Spectrum(0.f);
        } else if (std::isinf(result.y())) {
            Error("Infinite luminance value returned for image sample.  Setting to black.");
            result = Spectrum(0.f);
        }
        if (samples) { film->AddSample((*samples)[next++], result); return; }
        /* device camera: one filmed value per pixel at (x + 0.5, y + 0.5) */
        CameraSample at = CameraSample();
        at.imageX = cs.imageX; at.imageY = cs.imageY; at.lensU = at.lensV = 0.5f;
        film->AddSample(at, result);
    }
    void WriteImage() override { film->WriteImage(); } /* PhotonMappingRenderer::postLaunch */
};
} // namespace

void CudaRender::Render(const Scene *scene) {
    if (!camera_ || !sampler_) Severe("CreateCudaRenderer must precede Render");
    flush();
    /* lights (CudaLight::preLaunch, cudalight.cpp:105-120): point lights, and
     * the disks and triangle meshes of diffuse area lights, each with its 2D light samples
     * registered in sampler order (CudaSample::Add2D rounds the count) */
    std::vector<pmcuda::Light> lights;
    Sample proto(NULL, NULL, NULL, scene);
    uint32_t n2d = 0;
    for (Light *l : scene->lights) {
        if (PointLight *pl = dynamic_cast<PointLight *>(l)) {
            pmcuda::Light L;
            L.kind = pmcuda::Light::Point;
            L.pos[0] = pl->lightPos.x; L.pos[1] = pl->lightPos.y; L.pos[2] = pl->lightPos.z;
            L.intensity = toPm(pl->Intensity);
            lights.push_back(L);
        } else if (DistantLight *dl = dynamic_cast<DistantLight *>(l)) { /* beyond the reference */
            pmcuda::Light L;
            L.kind = pmcuda::Light::Distant;
            L.dir[0] = dl->lightDir.x; L.dir[1] = dl->lightDir.y; L.dir[2] = dl->lightDir.z;
            L.intensity = toPm(dl->L);
            lights.push_back(L);
        } else if (DiffuseAreaLight *al = dynamic_cast<DiffuseAreaLight *>(l)) {
            uint32_t samplePerShape = (uint32_t)std::max(1, al->nSamples);
            for (const Reference<Shape> &s : al->shapeSet->shapes) {
                if (const Disk *disk = dynamic_cast<const Disk *>(s.GetPtr())) {
                    samplePerShape = (uint32_t)sampler_->RoundSize((int)samplePerShape);
                    proto.Add2D(samplePerShape);
                    n2d += samplePerShape;
                    pmcuda::Light L;
                    L.kind = pmcuda::Light::AreaDisk;
                    toPm(disk, L.disk);
                    L.Lemit = toPm(al->Lemit);
                    L.n_samples = (int)samplePerShape;
                    lights.push_back(L);
                } else if (const TriangleMesh *tm = dynamic_cast<const TriangleMesh *>(s.GetPtr())) {
                    /* beyond the reference: the mesh as one light, its samples registered like a disk's */
                    samplePerShape = (uint32_t)sampler_->RoundSize((int)samplePerShape);
                    proto.Add2D(samplePerShape);
                    n2d += samplePerShape;
                    pmcuda::Light L;
                    L.kind = pmcuda::Light::AreaMesh;
                    toPm(tm, L.mesh);
                    L.reverse_orientation = tm->ReverseOrientation;
                    L.Lemit = toPm(al->Lemit);
                    L.n_samples = (int)samplePerShape;
                    lights.push_back(L);
                } else {
                    Warning("UnImplemented Cuda Area Light Source");
                }
            }
        } else {
            Warning("UnImplemented Cuda Light Source");
        }
    }
    /* the eye samples (PbrtCamera::preLaunch, pbrtcamera.cpp:57-122): the
     * sampler's stream in its own order, rays with differentials scaled by
     * 1/sqrt(spp), the light 2D randoms of each sample */
    if (devcam_.device_camera) {
        /* The camera's world basis through pbrt's public interface: rays from
         * the lens centre through the image centre, the middle of the right
         * edge and the middle of the top edge. A perspective camera's
         * direction is fwd + ndc_x right + ndc_y up up to length, so with
         * fwd = the centre direction, right = dr / (dr . fwd) - fwd and up
         * likewise. The 2D light samples are the device's own (Philox by
         * sample index), so none are registered with the sampler. */
        const int W = camera_->film->xResolution, H = camera_->film->yResolution;
        auto probe = [&](float x, float y, Ray *r) {
            CameraSample cs = CameraSample();
            cs.imageX = x; cs.imageY = y; cs.lensU = cs.lensV = 0.5f; cs.time = 0.f;
            camera_->GenerateRay(cs, r);
            r->d = Normalize(r->d);
        };
        Ray c, r, u;
        probe(0.5f * W, 0.5f * H, &c);
        probe((float)W, 0.5f * H, &r);
        probe(0.5f * W, 0.f, &u);
        const float kr = 1.f / (r.d.x * c.d.x + r.d.y * c.d.y + r.d.z * c.d.z);
        const float ku = 1.f / (u.d.x * c.d.x + u.d.y * c.d.y + u.d.z * c.d.z);
        pmcuda::Camera cam = devcam_;
        cam.pinhole = true;
        cam.width = W; cam.height = H;
        cam.eye[0] = c.o.x; cam.eye[1] = c.o.y; cam.eye[2] = c.o.z;
        cam.fwd[0] = c.d.x; cam.fwd[1] = c.d.y; cam.fwd[2] = c.d.z;
        cam.right[0] = r.d.x * kr - c.d.x; cam.right[1] = r.d.y * kr - c.d.y; cam.right[2] = r.d.z * kr - c.d.z;
        cam.up[0] = u.d.x * ku - c.d.x; cam.up[1] = u.d.y * ku - c.d.y; cam.up[2] = u.d.z * ku - c.d.z;
        PbrtFilm film;
        film.film = camera_->film;
        film.samples = NULL;
        cam.film = &film;
        try {
            impl_.Render(lights, cam);
        } catch (const pmcuda::Error &e) {
            Severe("%s", e.what());
        }
        return;
    }
    int xs, xe, ys, ye;
    camera_->film->GetSampleExtent(&xs, &xe, &ys, &ye);
    const int spp = sampler_->samplesPerPixel;
    const int64_t maximal = (int64_t)(xe - xs) * (ye - ys) * spp;
    const int maxSamples = sampler_->MaximumSampleCount();
    Sample *samples = proto.Duplicate(maxSamples);
    RNG rng;
    pmcuda::Camera cam;
    cam.pinhole = false;
    cam.n2d = (int)n2d;
    std::vector<CameraSample> csamples;
    int count;
    while ((count = sampler_->GetMoreSamples(samples, rng)) > 0) {
        for (int i = 0; i < count; ++i) {
            if ((int64_t)csamples.size() >= maximal) Severe("Too many samples. expect:%lld", (long long)maximal);
            RayDifferential rd;
            camera_->GenerateRayDifferential(samples[i], &rd);
            rd.ScaleDifferentials(1.f / std::sqrt((float)spp));
            cam.rays.insert(cam.rays.end(), {rd.o.x, rd.o.y, rd.o.z, rd.d.x, rd.d.y, rd.d.z});
            if (n2d) cam.rand2d.insert(cam.rand2d.end(), samples[i].twoD[0], samples[i].twoD[0] + 2 * n2d);
            csamples.push_back(samples[i]);
            cam.samples.push_back(pmcuda::CameraSample{samples[i].imageX, samples[i].imageY});
        }
    }
    delete[] samples;
    if ((int64_t)csamples.size() != maximal) Warning("pbrt camera do not generate enough samples");
    PbrtFilm film;
    film.film = camera_->film;
    film.samples = &csamples;
    cam.film = &film;
    try {
        impl_.Render(lights, cam);
    } catch (const pmcuda::Error &e) {
        Severe("%s", e.what());
    }
}

/* ---------------------------------------------------------------- cudaapi.cpp:3-26 */
static CudaRender *cudaRender = NULL;

void CudaRenderInit() {
    try {
        cudaRender = new CudaRender();
    } catch (const pmcuda::Error &e) {
        Severe("%s", e.what());
    }
}

void CreateCudaShape(const std::string &name, Reference<Shape> &shape,
                     std::vector<Reference<Primitive> > *currentInstance, const Material *material, int lightIndex) {
    if (!cudaRender) Severe("CudaRenderInit must precede CreateCudaShape");
    cudaRender->createCudaShape(name, shape, currentInstance, material, lightIndex);
}

void CudaObjectInstance(std::vector<Reference<Primitive> > *key, const Transform &transform) {
    if (!cudaRender) Severe("CudaRenderInit must precede CudaObjectInstance");
    cudaRender->objectInstance(key, transform);
}

Renderer *CreateCudaRenderer(Sampler *sampler, Camera *camera, const ParamSet &params,
                             const std::string &rendername) {
    if (!cudaRender) Severe("CudaRenderInit must precede CreateCudaRenderer");
    cudaRender->createSubRenderer(sampler, camera, params, rendername);
    return cudaRender;
}
