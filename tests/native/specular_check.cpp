/*
 * specular_check.cpp — the host side of pm_add_material_specular
 * (csrc/pm_scene.cpp) on the CPU: the argument checks case by case, the
 * table as a commit uploads it, scene_specular and light_summary's bound.
 * tests/test_specular.py builds it with g++ (plain and under the address and
 * undefined-behaviour sanitizers) and reads the lines it prints:
 *   "spec <material> <8 hex floats>" per table entry, then "bad <count>".
 */
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "pm_api.h"
#include "pm_scene.h"

using namespace pm;

static int bad = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++bad; } \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float one[3] = {1.f, 1.f, 1.f}, kr[3] = {0.9f, 0.5f, 0.25f}, kt[3] = {0.8f, 1.0f, 0.9f};
    std::string err;
    int id = -1;

    /* the argument checks */
    EXPECT(check_material_specular(PM_MATTE, one, one, 1.5f, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(7, one, one, 1.5f, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(PM_GLASS, nullptr, one, 1.5f, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(PM_GLASS, one, nullptr, 1.5f, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(PM_MIRROR, nullptr, one, 1.5f, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(PM_MIRROR, one, nullptr, nan, err) == PM_OK); /* a mirror's kt and index: not looked at */
    for (int a = 0; a < 3; ++a) {
        for (float v : {-1e-3f, inf, -inf, nan}) {
            float c[3] = {1.f, 1.f, 1.f};
            c[a] = v;
            EXPECT(check_material_specular(PM_GLASS, c, one, 1.5f, err) == PM_ERR_INVALID);
            EXPECT(check_material_specular(PM_GLASS, one, c, 1.5f, err) == PM_ERR_INVALID);
            EXPECT(check_material_specular(PM_MIRROR, c, one, 1.5f, err) == PM_ERR_INVALID);
        }
    }
    for (float v : {0.f, -1.5f, inf, nan}) EXPECT(check_material_specular(PM_GLASS, one, one, v, err) == PM_ERR_INVALID);
    EXPECT(check_material_specular(PM_GLASS, one, one, 1.33f, err) == PM_OK);

    /* the table: materials 0 (matte), 1 (old glass), 2 (new glass), 3 (new mirror), 4 (matte, after) */
    HostScene hs;
    EXPECT(!scene_specular(hs));
    hs.materials.push_back(f4(0.5f, 0.5f, 0.5f, ibits(PM_MATTE)));
    hs.materials.push_back(f4(1.f, 1.f, 1.f, ibits(PM_GLASS)));
    EXPECT(add_material_specular(hs, PM_GLASS, kr, kt, 1.33f, nullptr, err) == PM_ERR_INVALID);
    EXPECT(add_material_specular(hs, PM_GLASS, kr, kt, -1.f, &id, err) == PM_ERR_INVALID);
    EXPECT(hs.materials.size() == 2 && !scene_specular(hs)); /* a refused call adds nothing */
    EXPECT(material_specular_table(hs).size() == 4);
    EXPECT(add_material_specular(hs, PM_GLASS, kr, kt, 1.33f, &id, err) == PM_OK && id == 2);
    EXPECT(add_material_specular(hs, PM_MIRROR, kr, nullptr, nan, &id, err) == PM_OK && id == 3);
    hs.materials.push_back(f4(0.2f, 0.2f, 0.2f, ibits(PM_MATTE)));
    EXPECT(scene_specular(hs));
    EXPECT(fbits_h(hs.materials[2].w) == PM_GLASS && fbits_h(hs.materials[3].w) == PM_MIRROR);
    const std::vector<float4> t = material_specular_table(hs);
    EXPECT(t.size() == 2 * hs.materials.size());
    for (size_t m = 0; m < hs.materials.size(); ++m) {
        const float4 &a = t[2 * m], &b = t[2 * m + 1];
        printf("spec %zu %a %a %a %a %a %a %a %d\n", m, a.x, a.y, a.z, a.w, b.x, b.y, b.z, fbits_h(b.w));
    }

    /* the flux bound keeps the lobes' colours apart from the Lambert weights */
    float big[3] = {0.5f, 3.f, 0.5f};
    EXPECT(add_material_specular(hs, PM_GLASS, one, big, 1.5f, &id, err) == PM_OK);
    LightDev L{};
    L.o_type = f4(0.f, 0.f, 0.f, ibits(PM_LIGHT_POINT));
    L.le = f4(1.f, 1.f, 1.f, 0.f);
    hs.lights.push_back(L);
    LightSummary sum;
    EXPECT(light_summary(hs, sum, err) == PM_OK);
    EXPECT(sum.spec_max == 3.0 && sum.kd_max == 1.0 && sum.scene_nonneg);

    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
