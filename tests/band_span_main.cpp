// Stand-alone caller of csrc/pong_band_span.h for tests/test_band_span_host.py (built with the host compiler under
// -fsanitize=address,undefined):  band_span_main <atlas file> <scores> <rows> <width> <ink_row0> <ink_row1>
// prints "a b kind first last" for every entry, then "status <return value>".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pong_band_span.h"

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const int scores = atoi(argv[2]), rows = atoi(argv[3]), width = atoi(argv[4]), r0 = atoi(argv[5]), r1 = atoi(argv[6]);
    std::vector<uint8_t> atlas((size_t)scores * scores * rows * width);  // (exactly the atlas: a read past it is reported)
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(atlas.data(), 1, atlas.size(), f) != atlas.size()) return 3;
    fclose(f);
    std::vector<uint8_t> table(crl::pong_band_span_bytes(scores));
    const int bad = crl::pong_band_span_table(atlas.data(), scores, rows, width, r0, r1, table.data());
    for (int a = 0; a < scores; a++)
        for (int b = 0; b < scores; b++)
            for (int k = 0; k < crl::kBandKinds; k++) {
                const uint8_t *t = &table[(size_t)((a * scores + b) * crl::kBandKinds + k) * 2];
                printf("%d %d %d %d %d\n", a, b, k, t[0], t[1]);
            }
    printf("status %d\n", bad);
    return 0;
}
