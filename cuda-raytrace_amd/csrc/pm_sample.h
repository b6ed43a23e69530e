/*
 * pm_sample.h — the samplers: the concentric disk and uniform sphere maps and
 * the permuted Halton sequence of the photon pass (permuted_radical_inverse,
 * permuted_halton4). Included by pm_shade.h (the Lambert lobe, the lights),
 * pm_trace.hip (emission) and pm_eye.hip (the thin lens).
 */
#pragma once
#include "pm_math.h"

#pragma clang fp contract(off)

namespace pm {

/* ------------------------------------------------------------ samplers */
/* util.cu.h:23-65 */
PMD void concentric_sample_disk(float u1, float u2, float *dx, float *dy) {
    float r, theta;
    float sx = 2 * u1 - 1;
    float sy = 2 * u2 - 1;
    if (sx == 0.0f && sy == 0.0f) { *dx = 0.0f; *dy = 0.0f; return; }
    /* the reference's four branches each divide; here the branch only selects
     * (r, numerator, offset) and one IEEE division follows. Bit-identical:
     * c - a/r == c + (-a)/r, and 0 + q == q for the q > 0 of that case. */
    float num, base;
    if (sx >= -sy) {
        if (sx > sy) { r = sx; num = sy; base = (sy > 0.0f) ? 0.0f : 8.0f; }
        else { r = sy; num = -sx; base = 2.0f; }
    } else {
        if (sx <= sy) { r = -sx; num = -sy; base = 4.0f; }
        else { r = -sy; num = sx; base = 6.0f; }
    }
    theta = base + num / r;
    theta = (float)((double)theta * (M_PI / 4.f));
    float st, ct;
    pmdm_sincosf(theta, &st, &ct);
    *dx = r * ct;
    *dy = r * st;
}

/* cudalight.cu.h:66-73 */
PMD v3 uniform_sample_sphere(float u1, float u2) {
    float z = 1.f - 2.f * u1;
    float r = sqrtf(fmaxf(0.f, 1.f - z * z));
    float phi = (float)(2.f * M_PI * (double)u2);
    float sp, cp;
    pmdm_sincosf(phi, &sp, &cp);
    return mk(r * cp, r * sp, z);
}

/* photontracing.cu:19-43 — permutation table in LDS/constant, 28 uints */
PMD float permuted_radical_inverse(uint32_t n, uint32_t base, const uint32_t *p) {
    float val = 0;
    float invBase = 1.f / base, invBi = invBase;
    while (n > 0) {
        uint32_t d_i = p[n % base];
        val += d_i * invBi;
        n = (uint32_t)((float)n * invBase); /* reference quirk: n *= invBase */
        invBi *= invBase;
    }
    return val;
}

/* The four dimensions (bases 2, 3, 5, 7; table offsets 0, 2, 5, 10) of
 * photontracing.cu:33-43, each exactly permuted_radical_inverse:
 *  - base 2 in closed form for n < 2^24: there the quirk n *= 0.5f is an exact
 *    shift, so the digits are the L = bitlength(n) bits of n, and every term
 *    d_i * 2^-(i+1) and partial sum is an exact dyadic fraction (<= 24
 *    significant bits): the loop's float sum equals rev = brev(n) / 2^32
 *    (table (0,1)) or (1 - 2^-L) - rev (table (1,0)) bit for bit;
 *  - bases 3, 5, 7 as three interleaved chains of one loop (independent
 *    digit steps overlap), bounded by base 3, which has the most digits. The
 *    permutation tables come packed, 3 bits per digit (pbits[k] >> 3r & 7:
 *    no LDS load in the digit chain). Below 12,582,912 the quirk's
 *    truncated product equals floor(m / base) for these bases (exhaustive
 *    check over all m < 2^24: first mismatch at 12,582,912 for base 7 and
 *    12,582,914 for base 3), so the digit is m - base * next instead of a
 *    modulo; larger indices (C4/C5) take the modulo. */
template <bool EXACT>
PMD void halton_chains(uint32_t n, const uint32_t pbits[3], float out[3]) {
    const uint32_t base[3] = {3u, 5u, 7u};
    float val[3], invBase[3], invBi[3];
    uint32_t m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        val[k] = 0.f;
        invBase[k] = 1.f / base[k];
        invBi[k] = invBase[k];
        m[k] = n;
    }
    while ((m[0] | m[1] | m[2]) != 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (m[k] > 0) {
                const uint32_t next = (uint32_t)((float)m[k] * invBase[k]); /* reference quirk: n *= invBase */
                const uint32_t r = EXACT ? m[k] - next * base[k] : m[k] % base[k];
                const uint32_t d_i = (pbits[k] >> (3u * r)) & 7u;
                val[k] += d_i * invBi[k];
                m[k] = next;
                invBi[k] *= invBase[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = val[k];
}
PMD void permuted_halton4(uint32_t n, const uint32_t *p, const uint32_t pbits[3], float out[4]) {
    if (n < (1u << 24)) {
        const float rev = (float)__builtin_bitreverse32(n) * 0x1p-32f;
        const int L = n ? 32 - __builtin_clz(n) : 0;
        out[0] = p[0] == 0u ? rev : (1.0f - __builtin_ldexpf(1.0f, -L)) - rev;
    } else {
        out[0] = permuted_radical_inverse(n, 2u, p);
    }
    if (n < 12582912u) halton_chains<true>(n, pbits, out + 1);
    else halton_chains<false>(n, pbits, out + 1);
}

} // namespace pm
