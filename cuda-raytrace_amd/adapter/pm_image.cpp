/*
 * pm_image.cpp — see pm_image.h. Every read is checked against the buffer's
 * size first; sizes are computed in 64 bits from bounded dimensions.
 */
#include "pm_image.h"

#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

namespace pmcuda {

namespace {

bool fail(std::string &err, const std::string &name, const std::string &what) {
    err = name + ": " + what;
    return false;
}

bool dims_ok(int64_t w, int64_t h) {
    return w > 0 && h > 0 && w <= IMAGE_MAX_DIM && h <= IMAGE_MAX_DIM && w * h < ((int64_t)1 << 28);
}

/* one whitespace-delimited header token of a PFM, at most 31 characters */
bool pfm_token(const unsigned char *d, size_t n, size_t &i, std::string &tok) {
    while (i < n && (d[i] == ' ' || d[i] == '\t' || d[i] == '\n' || d[i] == '\r')) ++i;
    tok.clear();
    while (i < n && !(d[i] == ' ' || d[i] == '\t' || d[i] == '\n' || d[i] == '\r')) {
        if (tok.size() >= 31) return false;
        tok.push_back((char)d[i++]);
    }
    return !tok.empty();
}

bool parse_int(const std::string &s, int64_t &v) {
    char *end = nullptr;
    const long long x = std::strtoll(s.c_str(), &end, 10);
    if (!end || *end != '\0' || s.size() > 10) return false;
    v = x;
    return true;
}

bool decode_pfm(const unsigned char *d, size_t n, const std::string &name, Image &out, std::string &err) {
    size_t i = 0;
    std::string magic, sw, sh, ss;
    if (!pfm_token(d, n, i, magic) || !pfm_token(d, n, i, sw) || !pfm_token(d, n, i, sh) || !pfm_token(d, n, i, ss))
        return fail(err, name, "truncated PFM header");
    if (magic != "PF" && magic != "Pf") return fail(err, name, "not a PFM file (no PF / Pf magic)");
    const int ch = magic == "PF" ? 3 : 1;
    int64_t w = 0, h = 0;
    if (!parse_int(sw, w) || !parse_int(sh, h) || !dims_ok(w, h)) return fail(err, name, "bad PFM size " + sw + " x " + sh);
    char *end = nullptr;
    const double scale = std::strtod(ss.c_str(), &end);
    if (!end || *end != '\0' || scale == 0.0 || !std::isfinite(scale)) return fail(err, name, "bad PFM scale " + ss);
    if (i >= n) return fail(err, name, "truncated PFM header");
    ++i; /* the single whitespace byte that ends the header */
    const uint64_t need = (uint64_t)w * (uint64_t)h * (uint64_t)ch * 4u;
    if ((uint64_t)(n - i) < need) return fail(err, name, "truncated PFM data");
    const bool little = scale < 0.0;
    out.w = (int)w; out.h = (int)h;
    out.rgb.resize(3 * (size_t)w * (size_t)h);
    const unsigned char *p = d + i;
    for (size_t k = 0; k < (size_t)w * (size_t)h; ++k) /* the first row is the bottom one: no flip */
        for (int c = 0; c < 3; ++c) {
            const unsigned char *b = p + 4 * (k * (size_t)ch + (size_t)(ch == 3 ? c : 0));
            const uint32_t u = little ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24
                                      : (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24;
            float f;
            std::memcpy(&f, &u, 4);
            if (!std::isfinite(f)) return fail(err, name, "PFM value that is not finite");
            out.rgb[3 * k + (size_t)c] = f;
        }
    return true;
}

bool decode_tga(const unsigned char *d, size_t n, const std::string &name, Image &out, std::string &err) {
    if (n < 18) return fail(err, name, "truncated TGA header");
    const int idlen = d[0], cmap = d[1], type = d[2], bpp = d[16], desc = d[17];
    const int64_t w = (int64_t)d[12] | (int64_t)d[13] << 8, h = (int64_t)d[14] | (int64_t)d[15] << 8;
    if (cmap != 0) return fail(err, name, "colour-mapped TGA not supported");
    if (!((type == 2 && (bpp == 24 || bpp == 32)) || (type == 3 && bpp == 8)))
        return fail(err, name, "TGA type " + std::to_string(type) + " with " + std::to_string(bpp) +
                                   " bits not supported (uncompressed 24/32-bit colour or 8-bit grey)");
    if (!dims_ok(w, h)) return fail(err, name, "bad TGA size");
    const size_t bytes = (size_t)bpp / 8, start = 18 + (size_t)idlen;
    if (n < start || (uint64_t)(n - start) < (uint64_t)w * (uint64_t)h * bytes) return fail(err, name, "truncated TGA data");
    const bool top = (desc & 0x20) != 0, right = (desc & 0x10) != 0;
    out.w = (int)w; out.h = (int)h;
    out.rgb.resize(3 * (size_t)w * (size_t)h);
    for (int64_t y = 0; y < h; ++y)
        for (int64_t x = 0; x < w; ++x) {
            const unsigned char *b = d + start + ((size_t)y * (size_t)w + (size_t)x) * bytes;
            const size_t oy = (size_t)(top ? h - 1 - y : y), ox = (size_t)(right ? w - 1 - x : x);
            float *o = &out.rgb[3 * (oy * (size_t)w + ox)];
            if (bytes == 1) o[0] = o[1] = o[2] = (float)b[0] / 255.f;
            else { o[0] = (float)b[2] / 255.f; o[1] = (float)b[1] / 255.f; o[2] = (float)b[0] / 255.f; } /* stored B G R (A) */
        }
    return true;
}

bool ends_with(const std::string &s, const char *suffix) {
    const size_t n = std::strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

} // namespace

bool decode_image(const unsigned char *data, size_t size, const std::string &name, Image &out, std::string &err) {
    out = Image();
    if (!data && size) return fail(err, name, "no data");
    if (ends_with(name, ".tga")) return decode_tga(data, size, name, out, err);
    if (ends_with(name, ".pfm")) return decode_pfm(data, size, name, out, err);
    return fail(err, name, "image format not supported (PFM and uncompressed TGA only)");
}

bool read_image(const std::string &path, Image &out, std::string &err) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return fail(err, path, "cannot open image file");
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string s = ss.str();
    return decode_image(reinterpret_cast<const unsigned char *>(s.data()), s.size(), path, out, err);
}

} // namespace pmcuda
