// jpeg_prefix_driver.cpp -- CPU-only developer check (tests/tools/jpeg_sanitize.sh): every proper prefix of the JPEG files named on the
// command line, plus randomly damaged copies, through savp_jpeg_info / savp_jpeg_entropy_decode, each in a heap buffer of exactly its
// length and with a coefficient buffer of exactly total_blocks * 64, so that AddressSanitizer sees any read or write one byte outside.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "savp_io.h"

int main(int argc, char** argv) {
    long calls = 0, accepted_prefixes = 0, damaged_ok = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
        fclose(f);
        SavpJpegInfo full;
        if (savp_jpeg_info(data.data(), data.size(), &full)) { fprintf(stderr, "%s: %s\n", argv[a], savp_jpeg_error()); return 2; }
        int16_t* coef = (int16_t*)malloc((size_t)full.total_blocks * 64 * sizeof(int16_t));
        uint16_t* qtab = (uint16_t*)malloc((size_t)full.components * 64 * sizeof(uint16_t));
        if (savp_jpeg_entropy_decode(data.data(), data.size(), &full, coef, qtab)) { fprintf(stderr, "%s: %s\n", argv[a], savp_jpeg_error()); return 2; }
        for (size_t len = 0; len < data.size(); ++len) {
            uint8_t* p = (uint8_t*)malloc(len ? len : 1);
            memcpy(p, data.data(), len);
            SavpJpegInfo info;
            savp_jpeg_info(p, len, &info);
            if (savp_jpeg_entropy_decode(p, len, &full, coef, qtab) == 0) ++accepted_prefixes;
            calls += 2;
            free(p);
        }
        uint64_t s = 88172645463325252ull + (uint64_t)a;
        for (int k = 0; k < 20000; ++k) {
            uint8_t* p = (uint8_t*)malloc(data.size());
            memcpy(p, data.data(), data.size());
            for (int j = 0; j < 1 + k % 4; ++j) {
                s ^= s << 13; s ^= s >> 7; s ^= s << 17;
                p[2 + s % (data.size() - 2)] = (uint8_t)(s >> 32);
            }
            SavpJpegInfo info;
            if (savp_jpeg_info(p, data.size(), &info) == 0 && info.total_blocks == full.total_blocks && info.components == full.components &&
                savp_jpeg_entropy_decode(p, data.size(), &info, coef, qtab) == 0) ++damaged_ok;
            calls += 2;
            free(p);
        }
        free(coef); free(qtab);
    }
    printf("%ld calls, %ld proper prefixes accepted (must be 0), %ld damaged copies still decoded\n", calls, accepted_prefixes, damaged_ok);
    return accepted_prefixes ? 1 : 0;
}
