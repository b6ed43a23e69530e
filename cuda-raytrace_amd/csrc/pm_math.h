/*
 * pm_math.h — the vector math every device unit builds on: PMD, v3 and its
 * operators with the reference's (OptiX) rounding semantics, rcp_exact, the
 * constants, fbits and the scalar-cache pointer types. Included by
 * pm_device.h, so by every kernel unit.
 *
 * Numerics contract: compiled with
 * -ffp-contract=off; every expression keeps the operation order of the
 * reference program it restates, so results match the CPU oracle bit for
 * bit. Transcendentals come from include/pm_detmath.h.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pm_detmath.h"

#pragma clang fp contract(off)

#define PMD __device__ __forceinline__

namespace pm {

/* ------------------------------------------------------------------ v3 */
struct v3 { float x, y, z; };
PMD v3 mk(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
PMD v3 operator+(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
PMD v3 operator-(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
PMD v3 operator-(v3 a) { return mk(-a.x, -a.y, -a.z); }
PMD v3 operator*(v3 a, v3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
PMD v3 operator*(v3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
PMD v3 operator*(float s, v3 a) { return mk(s * a.x, s * a.y, s * a.z); }
/* OptiX float3 / float multiplies by the reciprocal */
/* IEEE correctly rounded 1/x in 3 instructions instead of the ~10 of the
 * scaled division sequence: one FMA Newton step on v_rcp_f32. Checked bit for
 * bit against 1.0f / x for every float with 2^-125 <= |x| < 2^125
 * (tools/rcp_exhaustive.hip: 0 mismatches on gfx950); other inputs (zero,
 * denormal, huge, inf, nan) take the full division. */
PMD float rcp_exact(float x) {
    const float r0 = __builtin_amdgcn_rcpf(x);
    float r = __builtin_fmaf(__builtin_fmaf(-x, r0, 1.0f), r0, r0);
    if (__builtin_expect(((__float_as_uint(x) >> 23) & 0xffu) - 2u > 249u, 0)) r = 1.0f / x;
    return r;
}
PMD v3 operator/(v3 a, float s) { float inv = rcp_exact(s); return a * inv; }
PMD float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PMD v3 cross(v3 a, v3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
PMD v3 normalize(v3 v) { float inv = rcp_exact(sqrtf(dot(v, v))); return v * inv; }
PMD float absdot(v3 a, v3 b) { return fabsf(dot(a, b)); }
PMD bool is_black(v3 s) { return s.x == 0.0f && s.y == 0.0f && s.z == 0.0f; }
PMD v3 xyz(float4 a) { return mk(a.x, a.y, a.z); }
PMD float comp(v3 v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

constexpr float INV_PI = 0.31830988618379067154f;
constexpr float INV_TWOPI = 0.15915494309189533577f;
constexpr float RT_DEFAULT_MAX = 1.e27f;

PMD int fbits(float f) { return __float_as_int(f); }

/* pointers into the constant address space: loads through them with a
 * wave-uniform address go through the scalar cache into SGPRs (the
 * brute-force pair test, the gathers' photon streams) */
typedef const float __attribute__((address_space(4))) *const_f32_ptr;
typedef const uint32_t __attribute__((address_space(4))) *const_u32_ptr;

} // namespace pm
