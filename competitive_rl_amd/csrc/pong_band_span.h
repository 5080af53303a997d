// pong_band_span.h -- which chunk columns of the score band a single point changes.  Pure host C++ (nothing from HIP).
//
// The score band is one rendered text line per (score_l, score_r); a point replaces the image of (a, b) by that of (a + 1, b) or
// (a, b + 1).  The band is not separable by field (the left number's width moves the right number), so the span comes from the
// pair and the kind of transition: for every pair and kind, the first and last SOURCE chunk column -- 16-byte chunks of the
// unmirrored RGB row, pixel x holding bytes 3x .. 3x + 2 -- in which the two images differ on any row.  The raw delta writer
// (pong_raster_raw.hip) stores only these columns of the ink rows when a point is scored.  Derived from the atlas the context was
// created with: nothing about a font is assumed.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace crl {

static constexpr int kBandKinds = 2;  // 0: left + 1, 1: right + 1 (a pair's two entries are four bytes: the kernel loads them as one dword)
// an entry is two bytes {first, last}; first > last marks "the images are equal", {0, 255} "the successor lies outside the atlas:
// store the whole band"
static constexpr uint8_t kBandEmptyFirst = 255, kBandEmptyLast = 0, kBandWholeFirst = 0, kBandWholeLast = 255;

inline size_t pong_band_span_bytes(int scores) { return (size_t)scores * scores * kBandKinds * 2; }

// atlas: gray [scores][scores][rows][width]; table: pong_band_span_bytes(scores) bytes, entry ((a * scores + b) * kBandKinds + kind).
// Returns 0, or 1 + the entry index of the first transition with a differing pixel outside the ink rows [ink_row0, ink_row1) -- the
// delta writer's rule (every row outside them is white in every image) does not hold for such an atlas; such an entry is marked
// "whole band".
inline int pong_band_span_table(const uint8_t *atlas, int scores, int rows, int width, int ink_row0, int ink_row1, uint8_t *table) {
    int bad = 0;
    for (int a = 0; a < scores; a++)
        for (int b = 0; b < scores; b++)
            for (int kind = 0; kind < kBandKinds; kind++) {
                const int entry = (a * scores + b) * kBandKinds + kind;
                uint8_t *t = table + (size_t)entry * 2;
                const int a2 = a + (kind == 0), b2 = b + (kind == 1);
                if (a2 >= scores || b2 >= scores) {
                    t[0] = kBandWholeFirst, t[1] = kBandWholeLast;
                    continue;
                }
                const uint8_t *p = atlas + ((size_t)a * scores + b) * rows * width, *q = atlas + ((size_t)a2 * scores + b2) * rows * width;
                int x0 = width, x1 = -1;
                bool outside = false;
                for (int r = 0; r < rows; r++)
                    for (int x = 0; x < width; x++)
                        if (p[(size_t)r * width + x] != q[(size_t)r * width + x]) {
                            x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1;
                            outside |= r < ink_row0 || r >= ink_row1;
                        }
                if (outside) {
                    if (!bad) bad = 1 + entry;
                    t[0] = kBandWholeFirst, t[1] = kBandWholeLast;
                } else if (x1 < 0) {
                    t[0] = kBandEmptyFirst, t[1] = kBandEmptyLast;
                } else {
                    t[0] = (uint8_t)(3 * x0 / 16), t[1] = (uint8_t)((3 * x1 + 2) / 16);
                }
            }
    return bad;
}

}  // namespace crl
