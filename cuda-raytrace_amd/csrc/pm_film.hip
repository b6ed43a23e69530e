/*
 * pm_film.hip — the filtered film (HIP/CDNA4): pbrt-v2 ImageFilm::AddSample
 * + WriteImage restated as a gather from the sample raster of pm_set_camera
 * to the image, deterministic and without atomics (pm_api.h pm_film).
 *
 *   k_film   one workgroup per FILM_TILE x FILM_TILE output pixels, one lane
 *            per pixel. The tile's sample footprint (tile x strata plus the
 *            filter halo) goes through LDS in bands of whole sample rows,
 *            ascending: radiance with the sample's film position (Philox once
 *            per staged sample, not once per pixel that reads it). Each lane
 *            then walks its own footprint inside the band in ascending q, so
 *            a pixel's sum has one order whatever the tile or band size.
 *
 * LDS: 5 planes (r, g, b, fx, fy) x band capacity + the 16 x 16 weight table;
 * the capacity is FILM_LDS_SAMPLES at most (61 KB: two workgroups per CU of
 * 160 KB), and a small footprint (2 x 2 strata, width 2: 1,600 samples, 33 KB)
 * takes one band and leaves room for four workgroups per CU.
 */
#include <hip/hip_runtime.h>

#include "pm_kernels.h"

#pragma clang fp contract(off)

namespace pm {

constexpr int FILM_BLOCK = FILM_TILE * FILM_TILE;

__global__ __launch_bounds__(FILM_BLOCK) void k_film(FilmParams P) {
    extern __shared__ __attribute__((aligned(16))) float film_lds[];
    const int cap = P.row_w * P.band_rows;
    float *s_tab = film_lds;
    float *s_r = s_tab + PM_FILM_TABLE * PM_FILM_TABLE;
    float *s_g = s_r + cap, *s_b = s_g + cap, *s_fx = s_b + cap, *s_fy = s_fx + cap;

    const int t = threadIdx.x;
    if (t < PM_FILM_TABLE * PM_FILM_TABLE) s_tab[t] = P.table[t];

    const int tx0 = blockIdx.x * FILM_TILE, ty0 = blockIdx.y * FILM_TILE;
    const int x = tx0 + (t & (FILM_TILE - 1)), y = ty0 + t / FILM_TILE;
    const int xs = P.cam.xs, ys = P.cam.ys;
    /* the tile's footprint in the sample raster; c0 may be negative (columns
     * left of the raster are never staged or read) */
    const int c0 = (tx0 - P.hx) * xs;
    const int tr0 = max(0, (ty0 - P.hy) * ys), tr1 = min(P.HS, (ty0 + FILM_TILE + P.hy) * ys);
    const int sc0 = max(0, c0), sc1 = min(P.WS, c0 + P.row_w);
    /* this lane's candidate samples: the strata of pixels x - hx .. x + hx */
    const int lx0 = max(0, (x - P.hx) * xs), lx1 = min(P.WS, (x + P.hx + 1) * xs);
    const int ly0 = max(0, (y - P.hy) * ys), ly1 = min(P.HS, (y + P.hy + 1) * ys);
    const float xf = (float)x, yf = (float)y;

    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
    for (int r0 = tr0; r0 < tr1; r0 += P.band_rows) {
        const int r1 = min(tr1, r0 + P.band_rows);
        __syncthreads(); /* the previous band is read (first band: the table is written) */
        const int ncol = sc1 - sc0;
        for (int iy = r0; iy < r1; ++iy) {
            /* a row segment is 3 ncol consecutive floats: lane k reads float
             * k, k + 256, ... (whole 256-B lines per wave) and drops it into
             * its plane; no division but the one by the constant 3 */
            const int64_t q0 = (int64_t)iy * P.WS + sc0;
            const float *row = P.samples + 3 * q0;
            const int lb = (iy - r0) * P.row_w + (sc0 - c0);
            for (int k = t; k < 3 * ncol; k += FILM_BLOCK) {
                const int j = k / 3, ch = k - 3 * j;
                (ch == 0 ? s_r : ch == 1 ? s_g : s_b)[lb + j] = row[k];
            }
            for (int j = t; j < ncol; j += FILM_BLOCK) {
                float ju, jv, lu, lv, fx, fy;
                if (P.cam.jitter) camera_randoms(P.cam, q0 + j, 0u, &ju, &jv, &lu, &lv);
                else ju = jv = 0.5f; /* the lens randoms are the eye pass's alone */
                camera_film_xy(P.cam, sc0 + j, iy, ju, jv, &fx, &fy);
                s_fx[lb + j] = fx; s_fy[lb + j] = fy;
            }
        }
        __syncthreads();
#ifdef PM_FILM_STAGE_ONLY /* measurement builds (make variant): staging alone, one LDS read per band */
        sw = sw + s_fx[t % (ncol > 0 ? ncol : 1)];
        continue;
#endif
        for (int iy = max(ly0, r0); iy < min(ly1, r1); ++iy) {
            const int base = (iy - r0) * P.row_w - c0;
            for (int ix = lx0; ix < lx1; ++ix) {
                const int li = base + ix;
                const float dx = s_fx[li] - 0.5f, dy = s_fy[li] - 0.5f;
                if (!(ceilf(dx - P.xw) <= xf && xf <= floorf(dx + P.xw) && ceilf(dy - P.yw) <= yf &&
                      yf <= floorf(dy + P.yw)))
                    continue;
                const int jx = min((int)floorf(fabsf((xf - dx) * P.inv_xw * (float)PM_FILM_TABLE)), PM_FILM_TABLE - 1);
                const int jy = min((int)floorf(fabsf((yf - dy) * P.inv_yw * (float)PM_FILM_TABLE)), PM_FILM_TABLE - 1);
                const float w = s_tab[jy * PM_FILM_TABLE + jx];
                sr = sr + w * s_r[li];
                sg = sg + w * s_g[li];
                sb = sb + w * s_b[li];
                sw = sw + w;
            }
        }
    }
    if (x >= P.W || y >= P.H) return;
    float *o = P.image + 3 * ((int64_t)y * P.W + x);
    if (sw == 0.f) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
    o[0] = fmaxf(0.f, sr / sw);
    o[1] = fmaxf(0.f, sg / sw);
    o[2] = fmaxf(0.f, sb / sw);
}

/* Halo of the footprint in pixels per side. A sample of pixel p has
 * fx in [p, p + 1] (the fp32 sum ix + ju may round up to the next stratum),
 * so it reaches the pixels x with |x + 0.5 - fx| <= w: p - floor(w + 0.5) ..
 * p + floor(w + 0.5). The membership test rounds dx -+ w in fp32, an error
 * below 2^-23 (extent + 8): the margin keeps the halo conservative when
 * w + 0.5 sits just below an integer. pm_set_camera holds a filmed raster to
 * 2^20 samples per axis, so the margin stays below 0.26 and the halo at 4. The kernel applies the exact test to
 * every staged sample, so a larger halo never changes a result. */
static int film_halo(float w, int extent) { return (int)floorf(w + 0.5f + (float)(extent + 8) * 2.4e-7f); }

hipError_t launch_film(FilmParams p, hipStream_t s) {
    if (p.W <= 0 || p.H <= 0) return hipSuccess;
    p.hx = film_halo(p.xw, p.W);
    p.hy = film_halo(p.yw, p.H);
    p.row_w = (FILM_TILE + 2 * p.hx) * p.cam.xs;
    const int rows = (FILM_TILE + 2 * p.hy) * p.cam.ys;
    if (p.row_w > FILM_LDS_SAMPLES) return hipErrorInvalidValue; /* widths <= 4 and <= 8 strata: 192 at most */
    p.band_rows = std::min(rows, FILM_LDS_SAMPLES / p.row_w);
    const size_t lds = ((size_t)5 * p.row_w * p.band_rows + PM_FILM_TABLE * PM_FILM_TABLE) * sizeof(float);
    const dim3 grid((unsigned)((p.W + FILM_TILE - 1) / FILM_TILE), (unsigned)((p.H + FILM_TILE - 1) / FILM_TILE));
    pm_launch(k_film, grid, dim3(FILM_BLOCK), (uint32_t)lds, s, p);
    return hipGetLastError();
}

} // namespace pm
