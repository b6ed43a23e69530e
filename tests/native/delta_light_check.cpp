/* Host check of pm_scene.cpp's distant light (tests/test_delta_lights.py): the
 * parameter checks of make_distant_light and, for a small scene of a mesh, a
 * disk and a sphere with a distant light, the commit's world sphere and the
 * light's record (finish_lights) against the same quantities evaluated in
 * long double from the float inputs; then the selection table and summary.
 * Prints "bad N". */
#include <cmath>
#include <cstdio>
#include <cstring>

#include "pm_scene.h"
using namespace pm;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static bool close_to(float got, long double ref, long double scale) { return fabsl((long double)got - ref) <= 1e-6L * scale; }

int main() {
    std::string err;
    LightDev D{};
    const float axis[3] = {0.3f, -2.f, 0.5f}, I[3] = {10.f, 20.f, 30.f};
    const float zero[3] = {0.f, 0.f, 0.f}, nan3[3] = {0.f, NAN, 0.f};
    /* parameter checks */
    CHECK(make_distant_light(zero, I, D, err) == PM_ERR_INVALID && err.find("zero direction") != std::string::npos, "zero direction");
    CHECK(make_distant_light(nan3, I, D, err) == PM_ERR_INVALID, "nan direction");
    CHECK(make_distant_light(axis, nullptr, D, err) == PM_ERR_INVALID, "null radiance");

    /* the scene: a two-triangle mesh, a disk and a sphere; a point light, the distant light */
    HostScene hs;
    hs.materials.push_back(f4(0.5f, 0.5f, 0.5f, ibits(PM_MATTE)));
    const float P[12] = {-10.f, 0.f, -20.f, 30.5f, 0.f, -20.f, 30.5f, 7.25f, 40.f, -10.f, 3.f, 40.f};
    hs.P.assign(P, P + 12);
    hs.N.assign(12, 0.f);
    hs.UV.assign(8, 0.f);
    hs.meshes.push_back(HMesh{0, -1, 0, 0});
    hs.tris.push_back(HTri{{0, 1, 2}, 0, (uint32_t)hs.next_tri_id++});
    hs.tris.push_back(HTri{{0, 2, 3}, 0, (uint32_t)hs.next_tri_id++});
    { /* disk at (5, 60, 5), radius 8, facing -y: bounds x, z in [-3, 13], y = 60 */
        hs.disks.push_back(f4(5.f, 60.f, 5.f, 0.f));
        hs.disks.push_back(f4(8.f, 0.f, 0.f, 6.2831853f));
        hs.disks.push_back(f4(0.f, 0.f, 8.f, -60.f));
        hs.disks.push_back(f4(0.f, -1.f, 0.f, 1.f / 64.f));
        hs.disks.push_back(f4(1.f / 64.f, ibits(0), ibits(-1), ibits(0)));
    }
    { /* sphere of radius 4 at (-20, 10, 0): bounds x in [-24, -16] */
        const float m[16] = {1, 0, 0, -20, 0, 1, 0, 10, 0, 0, 1, 0, 0, 0, 0, 1};
        hs.spheres.push_back(f4(1, 0, 0, 20));
        hs.spheres.push_back(f4(0, 1, 0, -10));
        hs.spheres.push_back(f4(0, 0, 1, 0));
        hs.spheres.push_back(f4(4.f, ibits(0), ibits(-1), ibits(0)));
        hs.sphere_o2w.insert(hs.sphere_o2w.end(), m, m + 16);
    }
    LightDev Pt{};
    Pt.o_type = f4(0.f, 50.f, 0.f, ibits(PM_LIGHT_POINT));
    Pt.p1_ns = f4(0, 0, 0, ibits(1));
    Pt.le = f4(100.f, 100.f, 100.f, 0.f);
    hs.lights.push_back(Pt);
    const float to_light[3] = {1.f, 2.f, -0.5f}, Lr[3] = {3.f, 2.f, 1.f};
    CHECK(make_distant_light(to_light, Lr, D, err) == PM_OK, "distant: %s", err.c_str());
    hs.lights.push_back(D);
    CHECK(validate_scene(hs, err) == PM_OK, "validate: %s", err.c_str());

    std::vector<BuildPrim> prims;
    float blo[3], bhi[3], sph[4];
    scene_boxes(hs, prims, blo, bhi);
    const float elo[3] = {-24.f, 0.f, -20.f}, ehi[3] = {30.5f, 60.f, 40.f};
    for (int a = 0; a < 3; ++a) CHECK(blo[a] == elo[a] && bhi[a] == ehi[a], "bounds[%d] %g %g", a, blo[a], bhi[a]);
    CHECK(finish_lights(hs, blo, bhi, sph, err) == PM_OK, "finish_lights: %s", err.c_str());
    long double C[3], r2 = 0;
    for (int a = 0; a < 3; ++a) {
        C[a] = ((long double)elo[a] + ehi[a]) / 2;
        CHECK(sph[a] == (float)C[a], "centre[%d] %g", a, sph[a]);
        const long double d = fmaxl(fabsl(ehi[a] - (long double)sph[a]), fabsl(elo[a] - (long double)sph[a]));
        r2 += d * d;
    }
    const long double R = sqrtl(r2);
    CHECK((long double)sph[3] >= R && (long double)sph[3] <= R * (1 + 2e-7L), "radius %.9g vs %.9Lg", sph[3], R);
    /* every bound corner inside the sphere */
    for (int k = 0; k < 8; ++k) {
        long double d2 = 0;
        for (int a = 0; a < 3; ++a) { const long double d = ((k >> a) & 1 ? ehi[a] : elo[a]) - (long double)sph[a]; d2 += d * d; }
        CHECK(sqrtl(d2) <= (long double)sph[3], "corner %d outside", k);
    }
    {
        const LightDev &L = hs.lights[1];
        const long double Rf = sph[3];
        const long double len = sqrtl((long double)to_light[0] * to_light[0] + (long double)to_light[1] * to_light[1] + (long double)to_light[2] * to_light[2]);
        const float n[3] = {L.n_area.x, L.n_area.y, L.n_area.z}, o[3] = {L.o_type.x, L.o_type.y, L.o_type.z},
                    p1[3] = {L.p1_ns.x, L.p1_ns.y, L.p1_ns.z}, p2[3] = {L.p2_r2d.x, L.p2_r2d.y, L.p2_r2d.z};
        long double d11 = 0, d22 = 0, d12 = 0, d1n = 0, d2n = 0;
        for (int a = 0; a < 3; ++a) {
            CHECK(close_to(n[a], -to_light[a] / len, 1), "normal[%d]", a);
            CHECK(close_to(o[a], (long double)sph[a] - Rf * n[a], Rf), "disk centre[%d] %g", a, o[a]);
            d11 += (long double)p1[a] * p1[a]; d22 += (long double)p2[a] * p2[a]; d12 += (long double)p1[a] * p2[a];
            d1n += (long double)p1[a] * n[a]; d2n += (long double)p2[a] * n[a];
        }
        CHECK(fabsl(sqrtl(d11) - Rf) < 1e-6L * Rf && fabsl(sqrtl(d22) - Rf) < 1e-6L * Rf, "radius vectors' length");
        CHECK(fabsl(d12) < 1e-6L * Rf * Rf && fabsl(d1n) < 1e-6L * Rf && fabsl(d2n) < 1e-6L * Rf, "radius vectors not orthogonal");
        /* |to_light.x| < |to_light.y|: v1 = (0, z, -y) / |(y, z)| of the unit direction, v2 = w x v1 */
        const long double w[3] = {-(long double)n[0], -(long double)n[1], -(long double)n[2]};
        const long double il = 1 / sqrtl(w[1] * w[1] + w[2] * w[2]);
        CHECK(p1[0] == 0.f && close_to(p1[1], Rf * w[2] * il, Rf) && close_to(p1[2], -Rf * w[1] * il, Rf), "p1");
        CHECK(close_to(p2[0], Rf * (w[1] * (-w[1] * il) - w[2] * (w[2] * il)), Rf), "p2 = R (w x v1)");
        CHECK(close_to(L.n_area.w, M_PIl * Rf * Rf, M_PIl * Rf * Rf), "area %g", L.n_area.w);
        CHECK(L.le.w == 2.f * sph[3] && fbits_h(L.p1_ns.w) == 1 && fbits_h(L.o_type.w) == PM_LIGHT_DISTANT && L.p2_r2d.w == 0.f, "lanes");
        CHECK(L.le.x == Lr[0] && L.le.y == Lr[1] && L.le.z == Lr[2], "radiance");
        /* a second commit (more geometry) refills the record from the kept direction */
        const float n0[3] = {n[0], n[1], n[2]};
        float bhi2[3] = {bhi[0] + 100.f, bhi[1], bhi[2]}, sph2[4];
        CHECK(finish_lights(hs, blo, bhi2, sph2, err) == PM_OK && sph2[3] > sph[3], "second commit");
        CHECK(hs.lights[1].n_area.x == n0[0] && hs.lights[1].n_area.y == n0[1] && hs.lights[1].n_area.z == n0[2], "direction moved");
        CHECK(hs.lights[1].le.w == 2.f * sph2[3], "second commit's 2R");
        CHECK(finish_lights(hs, blo, bhi, sph, err) == PM_OK, "back");
    }
    /* the summary: table = light_selection_cdf of (4 pi, solid angle, pi R^2) weights; bounds cover Le / pdf */
    LightSummary ls;
    CHECK(light_summary(hs, ls, err) == PM_OK && ls.cdf_ok && ls.scene_nonneg, "summary: %s", err.c_str());
    {
        const long double y0 = 0.212671L * 100 + 0.715160L * 100 + 0.072169L * 100,
                          y2 = 0.212671L * Lr[0] + 0.715160L * Lr[1] + 0.072169L * Lr[2];
        const long double w0 = y0 * 4 * M_PIl, w2 = y2 * (long double)hs.lights[1].n_area.w;
        CHECK(close_to(ls.cdf[0], w0 / (w0 + w2), 1) && ls.cdf[1] == 1.f, "table %g %g", ls.cdf[0], ls.cdf[1]);
        const long double b_dist = 3 * (long double)hs.lights[1].n_area.w;
        CHECK(ls.emit_max >= (double)b_dist && ls.emit_max <= 1.01 * (double)fmaxl(b_dist, 400 * M_PIl), "emit_max %g", ls.emit_max);
    }
    /* a distant light over a degenerate scene (one point) fails, naming the light */
    {
        float one[3] = {1.f, 1.f, 1.f}, s4[4];
        const int rc = finish_lights(hs, one, one, s4, err);
        CHECK(rc == PM_ERR_INVALID && err.find("distant light 1") != std::string::npos, "degenerate: %d %s", rc, err.c_str());
        float inf_hi[3] = {INFINITY, 1.f, 1.f};
        CHECK(finish_lights(hs, one, inf_hi, s4, err) == PM_ERR_INVALID, "infinite bounds");
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
