/*
 * pm_image.h — image file readers for imagemap textures. Host-only C++.
 *
 *   PFM   "PF" (colour) and "Pf" (grey), both byte orders (the sign of the
 *         scale line); its first row is the bottom one
 *   TGA   uncompressed 24- and 32-bit true colour (type 2) and 8-bit grey
 *         (type 3), honouring the origin bit; bytes divide by 255, no gamma,
 *         as pbrt-v2's ReadImage does for TGA; alpha is dropped
 *
 * The result is w x h float RGB with row 0 the picture's bottom row, which is
 * v = 0 of pm_add_texture_image (pbrt-v2's imagemap flips its top-down images
 * for the same reason): a file whose first row is the top is flipped here.
 * Anything else, and any truncated or inconsistent file, is an error that
 * names the file; no byte past the buffer is read.
 */
#pragma once

#include <cstddef>
#include <string>
#include <vector>

namespace pmcuda {

struct Image {
    int w = 0, h = 0;
    std::vector<float> rgb; /* 3 * w * h, row 0 = bottom */
};

/* largest width or height accepted (the texel count must also stay below 2^28) */
constexpr int IMAGE_MAX_DIM = 1 << 16;

/* false with `err` set (it names `name`) on any malformed input */
bool decode_image(const unsigned char *data, size_t size, const std::string &name, Image &out, std::string &err);
bool read_image(const std::string &path, Image &out, std::string &err);

} // namespace pmcuda
