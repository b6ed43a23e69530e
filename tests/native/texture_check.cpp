/* Host check of pm_scene.cpp's texture assembly (tests/test_texture.py): the
 * argument checks of the pm_add_texture_* calls, the records and the
 * per-material table they build, the per-triangle uvs, and light_summary's
 * kd_max / scene_nonneg over textures. Built with the address and undefined-behaviour sanitizers. Prints the
 * records as text for the test to compare with texture_ref, then "bad N". */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "pm_image.h"
#include "pm_scene.h"
using namespace pm;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void print_operand(const TexOperand &o) {
    printf(" op %a %a %a %d %d %d %d %a %a %a %a", o.rgb[0], o.rgb[1], o.rgb[2], o.texel0, o.w, o.h, o.wrap, o.map[0], o.map[1],
           o.map[2], o.map[3]);
}

int main() {
    std::string err;
    HostScene hs;
    const float map1[4] = {1.f, 1.f, 0.f, 0.f}, map2[4] = {2.5f, -1.5f, 0.25f, 0.75f}, one[3] = {1.f, 1.f, 1.f};
    const float sc[3] = {0.5f, 2.f, 1.f}, nanv[4] = {1.f, NAN, 0.f, 0.f}, infv[3] = {1.f, INFINITY, 1.f};
    float img[2 * 3 * 3]; /* 3 wide, 2 high; the largest texel component is 3.0 */
    for (int i = 0; i < 18; ++i) img[i] = 0.125f * (float)i;
    img[7] = 3.0f;
    float img2[4 * 3]; /* 2 x 2, largest 0.75 */
    for (int i = 0; i < 12; ++i) img2[i] = 0.0625f * (float)i;
    img2[5] = 0.75f;
    int t = -1;

    /* ---- argument checks, case by case */
    CHECK(check_texture_image(nullptr, 3, 2, 0, map1, one, err) == PM_ERR_INVALID, "null texels");
    CHECK(check_texture_image(img, 3, 2, 0, nullptr, one, err) == PM_ERR_INVALID, "null mapping");
    CHECK(check_texture_image(img, 3, 2, 0, map1, nullptr, err) == PM_ERR_INVALID, "null scale");
    CHECK(check_texture_image(img, 0, 2, 0, map1, one, err) == PM_ERR_INVALID, "w = 0");
    CHECK(check_texture_image(img, 3, -1, 0, map1, one, err) == PM_ERR_INVALID, "h < 0");
    /* sizes whose byte count overflows: refused before a texel is read */
    CHECK(check_texture_image(img, std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 0, map1, one, err) == PM_ERR_INVALID, "huge image");
    CHECK(check_texture_image(img, 1 << 16, 1 << 15, 0, map1, one, err) == PM_ERR_INVALID, "2^31 texels");
    CHECK(check_texture_image(img, 3, 2, 3, map1, one, err) == PM_ERR_INVALID && err.find("wrap") != std::string::npos, "wrap 3");
    CHECK(check_texture_image(img, 3, 2, -1, map1, one, err) == PM_ERR_INVALID, "wrap -1");
    CHECK(check_texture_image(img, 3, 2, 0, nanv, one, err) == PM_ERR_INVALID, "nan mapping");
    CHECK(check_texture_image(img, 3, 2, 0, map1, infv, err) == PM_ERR_INVALID, "inf scale");
    { float bad[18]; std::memcpy(bad, img, sizeof bad); bad[17] = NAN;
      CHECK(check_texture_image(bad, 3, 2, 0, map1, one, err) == PM_ERR_INVALID, "nan texel"); }
    CHECK(check_texture_image(img, 3, 2, 2, map2, sc, err) == PM_OK, "valid image: %s", err.c_str());
    CHECK(add_texture_image(hs, img, 3, 2, 2, map2, sc, nullptr, err) == PM_ERR_INVALID, "null out");
    CHECK(check_texture_operands("c", nullptr, true, -1, one, -1, one, err) == PM_ERR_INVALID, "checker: null mapping");
    CHECK(check_texture_operands("c", map1, true, -1, nullptr, -1, one, err) == PM_ERR_INVALID, "checker: null rgb1");
    CHECK(check_texture_operands("c", map1, true, 0, nullptr, -1, nullptr, err) == PM_ERR_INVALID, "checker: null rgb2");
    CHECK(check_texture_operands("c", nanv, true, -1, one, -1, one, err) == PM_ERR_INVALID, "checker: nan mapping");
    CHECK(check_texture_operands("c", map1, true, -1, infv, -1, one, err) == PM_ERR_INVALID, "checker: inf colour");
    CHECK(check_texture_operands("s", nullptr, false, 0, nullptr, 1, nullptr, err) == PM_OK, "scale of two ids needs no pointer");
    CHECK(check_material_textured(PM_MIRROR, err) == PM_ERR_INVALID && check_material_textured(PM_GLASS, err) == PM_ERR_INVALID &&
          check_material_textured(PM_MATTE, err) == PM_OK, "material type");

    /* ---- records */
    int ti = -1, ti2 = -1, tc = -1, ts = -1, tss = -1, tk = -1;
    CHECK(add_texture_image(hs, img, 3, 2, 2, map2, sc, &ti, err) == PM_OK && ti == 0, "image: %s", err.c_str());
    CHECK(add_texture_image(hs, img2, 2, 2, 0, map1, one, &ti2, err) == PM_OK && ti2 == 1, "image 2: %s", err.c_str());
    CHECK(hs.texels.size() == 10 && hs.textures[1].op[0].texel0 == 6, "texel offsets");
    CHECK(hs.texels[2].x == img[6] && hs.texels[2].y == img[7] && hs.texels[2].z == img[8] && hs.texels[2].w == 0.f, "texel 2");
    const float c1[3] = {0.8f, 0.7f, 0.2f}, c2[3] = {0.1f, 0.2f, 0.6f};
    CHECK(add_texture_checker(hs, map2, ti, nullptr, -1, c2, &tc, err) == PM_OK && tc == 2, "checker: %s", err.c_str());
    CHECK(add_texture_scale(hs, ti, nullptr, ti2, nullptr, &ts, err) == PM_OK && ts == 3, "scale: %s", err.c_str());
    CHECK(add_texture_scale(hs, -1, c1, -1, c2, &tk, err) == PM_OK && tk == 4, "scale of constants");
    /* operands out of range, or not an image: refused, nothing appended */
    CHECK(add_texture_scale(hs, 7, nullptr, ti, nullptr, &tss, err) == PM_ERR_INVALID && err.find("out of range") != std::string::npos, "operand out of range");
    CHECK(add_texture_checker(hs, map1, tc, nullptr, -1, c2, &t, err) == PM_ERR_INVALID, "checker of a checker");
    CHECK(add_texture_scale(hs, ti, nullptr, ts, nullptr, &t, err) == PM_ERR_INVALID, "scale of a scale");
    CHECK(hs.textures.size() == 5, "a refused texture was appended");

    /* ---- materials */
    hs.materials.push_back(f4(0.5f, 0.5f, 0.5f, ibits(PM_MATTE))); /* as pm_add_material: mat_tex stays shorter */
    int m1 = -1, m2 = -1, m3 = -1;
    CHECK(add_material_textured(hs, PM_MATTE, 9, &m1, err) == PM_ERR_INVALID, "texture id out of range");
    CHECK(add_material_textured(hs, PM_MATTE, -1, &m1, err) == PM_ERR_INVALID, "texture id -1");
    CHECK(add_material_textured(hs, PM_GLASS, ti, &m1, err) == PM_ERR_INVALID, "textured glass");
    CHECK(add_material_textured(hs, PM_MATTE, ti, nullptr, err) == PM_ERR_INVALID, "null out id");
    CHECK(!scene_textured(hs), "no textured material yet");
    CHECK(add_material_textured(hs, PM_MATTE, ti, &m1, err) == PM_OK && m1 == 1, "textured material: %s", err.c_str());
    hs.materials.push_back(f4(0.9f, 0.1f, 0.1f, ibits(PM_MATTE)));
    CHECK(add_material_textured(hs, PM_MATTE, ts, &m2, err) == PM_OK && m2 == 3, "second textured material");
    CHECK(scene_textured(hs), "scene_textured");
    const std::vector<int> mt = material_textures(hs);
    CHECK(mt.size() == 4 && mt[0] == -1 && mt[1] == ti && mt[2] == -1 && mt[3] == ts, "per-material table");
    CHECK(hs.materials[1].x == 1.f && hs.materials[1].y == 1.f && hs.materials[1].z == 1.f && fbits_h(hs.materials[1].w) == PM_MATTE,
          "a textured matte's table Kd is 1");

    /* ---- kd_max and the sign */
    LightDev Pt{};
    Pt.o_type = f4(0.f, 50.f, 0.f, ibits(PM_LIGHT_POINT));
    Pt.p1_ns = f4(0, 0, 0, ibits(1));
    Pt.le = f4(100.f, 100.f, 100.f, 0.f);
    hs.lights.push_back(Pt);
    LightSummary ls;
    CHECK(light_summary(hs, ls, err) == PM_OK, "summary: %s", err.c_str());
    /* image 1: largest texel 3.0 times the largest scale 2.0 = 6; the scale of both: 6 * 0.75 = 4.5 */
    bool neg = true;
    const double b1 = texture_bound(hs, ti, &neg), b2 = texture_bound(hs, ts, nullptr);
    CHECK(b1 >= 6.0 && b1 <= 6.0 * 1.00001 && !neg, "image bound %g", b1);
    CHECK(b2 >= 4.5 && b2 <= 4.5 * 1.00001, "scale bound %g", b2);
    CHECK(ls.kd_max >= 6.0 && ls.kd_max <= 6.0 * 1.00001, "kd_max %g", ls.kd_max);
    CHECK(ls.scene_nonneg, "non-negative scene");
    {   /* an image whose largest texel is 3.0, scale 1 */
        HostScene h2;
        h2.lights.push_back(Pt);
        int a = -1, m = -1;
        CHECK(add_texture_image(h2, img, 3, 2, 0, map1, one, &a, err) == PM_OK && add_material_textured(h2, PM_MATTE, a, &m, err) == PM_OK, "h2");
        LightSummary l2;
        CHECK(light_summary(h2, l2, err) == PM_OK && l2.kd_max >= 3.0 && l2.kd_max <= 3.0 * 1.00001 && l2.scene_nonneg, "kd_max %g of a 3.0 texel", l2.kd_max);
        /* an unused texture does not count; a negative texel of a used one ends the guarantee */
        float ng[3] = {0.5f, -0.25f, 9.f};
        int b = -1;
        CHECK(add_texture_image(h2, ng, 1, 1, 0, map1, one, &b, err) == PM_OK, "negative texel is finite");
        CHECK(light_summary(h2, l2, err) == PM_OK && l2.kd_max <= 3.0 * 1.00001 && l2.scene_nonneg, "unused texture counted");
        CHECK(add_material_textured(h2, PM_MATTE, b, &m, err) == PM_OK && light_summary(h2, l2, err) == PM_OK, "h2 b");
        CHECK(l2.kd_max >= 9.0 && !l2.scene_nonneg, "negative texel: kd_max %g nonneg %d", l2.kd_max, (int)l2.scene_nonneg);
    }

    /* ---- per-triangle uvs: a mesh with uvs, one without (tri_frame's default corners) */
    const float P[18] = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 5, 5, 5, 6, 5, 5};
    hs.P.assign(P, P + 18);
    const float UV[12] = {0.1f, 0.2f, 0.9f, 0.2f, 0.9f, 0.8f, 0.1f, 0.8f, 0, 0, 0, 0};
    hs.UV.assign(UV, UV + 12);
    hs.meshes.push_back(HMesh{m1, -1, 0, 1});
    hs.meshes.push_back(HMesh{m2, -1, 0, 0});
    hs.tris.push_back(HTri{{0, 1, 2}, 0, 0});
    hs.tris.push_back(HTri{{0, 2, 3}, 0, 1});
    hs.tris.push_back(HTri{{3, 4, 5}, 1, 2});
    const uint32_t order[3] = {2, 0, 1};
    const std::vector<float4> uv = triangle_uvs(hs, order, 3);
    CHECK(uv.size() == 6, "uv size");
    CHECK(uv[0].x == 0.f && uv[0].y == 0.f && uv[0].z == 1.f && uv[0].w == 0.f && uv[1].x == 0.f && uv[1].y == 1.f, "default corners");
    CHECK(uv[2].x == 0.1f && uv[2].y == 0.2f && uv[2].z == 0.9f && uv[2].w == 0.2f && uv[3].x == 0.9f && uv[3].y == 0.8f, "triangle 0");
    CHECK(uv[4].z == 0.9f && uv[4].w == 0.8f && uv[5].x == 0.1f && uv[5].y == 0.8f && uv[5].z == 0.f && uv[5].w == 0.f, "triangle 1");

    /* ---- the image readers: every prefix of a valid file, and headers that
     * promise more than the file holds, are errors and read nothing past the
     * buffer (each buffer is a heap block of exactly its size: the address
     * sanitizer sees one byte too many) */
    {
        using pmcuda::Image;
        using pmcuda::decode_image;
        std::vector<unsigned char> pfm;
        const char *hd = "PF\n3 2\n-1.0\n";
        pfm.insert(pfm.end(), hd, hd + std::strlen(hd));
        for (int i = 0; i < 18; ++i) { unsigned char b[4]; std::memcpy(b, &img[i], 4); pfm.insert(pfm.end(), b, b + 4); }
        std::vector<unsigned char> tga(18, 0);
        tga[2] = 2; tga[12] = 3; tga[14] = 2; tga[16] = 24; tga[17] = 0x20;
        for (int i = 0; i < 18; ++i) tga.push_back((unsigned char)(10 * i));
        Image im;
        std::string e;
        auto run = [&](const std::vector<unsigned char> &v, const char *name) {
            unsigned char *heap = new unsigned char[v.size() ? v.size() : 1];
            if (!v.empty()) std::memcpy(heap, v.data(), v.size());
            const bool ok = decode_image(heap, v.size(), name, im, e);
            delete[] heap;
            return ok;
        };
        CHECK(run(pfm, "a.pfm") && im.w == 3 && im.h == 2 && im.rgb.size() == 18 && im.rgb[7] == 3.0f, "valid PFM: %s", e.c_str());
        CHECK(run(tga, "a.tga") && im.w == 3 && im.h == 2 && im.rgb[3 * 3 + 0] == 20.f / 255.f && im.rgb[3 * 3 + 2] == 0.f, "valid TGA (top origin flipped): %s", e.c_str());
        for (size_t n = 0; n < pfm.size(); ++n)
            CHECK(!run(std::vector<unsigned char>(pfm.begin(), pfm.begin() + n), "a.pfm") && e.find("a.pfm") != std::string::npos, "PFM prefix %zu accepted", n);
        for (size_t n = 0; n < tga.size(); ++n)
            CHECK(!run(std::vector<unsigned char>(tga.begin(), tga.begin() + n), "a.tga") && e.find("a.tga") != std::string::npos, "TGA prefix %zu accepted", n);
        const char *over[] = {"PF\n65536 65536\n-1.0\n", "PF\n2147483647 2147483647\n-1.0\n", "PF\n99999999999 1\n-1.0\n", "PF\n-3 2\n-1.0\n",
                              "Pf\n16384 16384\n1.0\n", "PF\n3 2\n-1.0", "PF 3 2 nan\n", "PF\n3\n", "PF"};
        for (const char *h : over) {
            std::vector<unsigned char> v(h, h + std::strlen(h));
            v.insert(v.end(), 40, 0);
            CHECK(!run(v, "big.pfm"), "oversized header accepted: %s", h);
        }
        std::vector<unsigned char> t2 = tga;
        t2[12] = 0xff; t2[13] = 0xff; t2[14] = 0xff; t2[15] = 0xff; /* 65535 x 65535 */
        CHECK(!run(t2, "big.tga"), "oversized TGA accepted");
        t2 = tga; t2[0] = 255; /* an id field longer than the file */
        CHECK(!run(t2, "id.tga"), "TGA id past the end accepted");
        t2 = tga; t2[16] = 32;
        CHECK(!run(t2, "bpp.tga"), "32-bit header over 24-bit data accepted");
        CHECK(!run(pfm, "a.exr") && !run(tga, "a.png"), "unknown format accepted");
    }

    for (size_t i = 0; i < hs.textures.size(); ++i) {
        const TexRec &T = hs.textures[i];
        printf("tex %zu kind %d map %a %a %a %a", i, T.kind, T.map[0], T.map[1], T.map[2], T.map[3]);
        print_operand(T.op[0]);
        print_operand(T.op[1]);
        printf("\n");
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
