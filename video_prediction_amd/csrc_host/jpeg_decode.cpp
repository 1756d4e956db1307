// jpeg_decode.cpp -- the host half of JPEG decoding (libsavp_io.so): marker walk + baseline Huffman decoding (ITU T.81 annex F), the
// serial part of tf.image.decode_jpeg (base_dataset.py:161-162, ucf101_dataset.py:48,52).  It stops at the quantised coefficients:
// dequantisation, IDCT, chroma upsampling and colour conversion run on the device (savp_jpeg_decode_u8, csrc/jpeg_decode.hip).
// Restated from the published format; no libjpeg is linked.  Every read is bounds-checked against [data, data + len), every
// coefficient write against the block it belongs to; nothing here allocates per call except the two small Huffman tables.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "savp_io.h"

namespace {
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                             62, 63};

thread_local char g_msg[160] = "";
int fail(int code, const char* msg) { snprintf(g_msg, sizeof(g_msg), "%s", msg); return code; }

struct Huff {                       // canonical code of one DHT table
    bool present = false;
    uint8_t counts[16];
    uint8_t values[256];
    // decoding: 9-bit lookahead (length << 8 | value, 0 = longer code), then the maxcode walk of T.81 F.2.2.3
    uint16_t look[512];
    int32_t maxcode[18];            // maxcode[l] = largest code of length l (-1: none)
    int32_t valptr[17], mincode[17];
    bool build() {
        int code = 0, k = 0;
        memset(look, 0, sizeof(look));
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = k; mincode[l] = code;
            for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
                if (code >= (1 << l)) return false;
                if (l <= 9) {
                    const int base = code << (9 - l);
                    for (int j = 0; j < (1 << (9 - l)); ++j) look[base + j] = (uint16_t)((l << 8) | values[k]);
                }
            }
            maxcode[l] = counts[l - 1] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        return true;
    }
};

struct Component { int id, h, v, tq, td, ta; };

struct Header {
    int width = 0, height = 0, nc = 0;
    Component c[3];
    uint16_t qt[4][64]; bool qt_present[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart = 0;
    uint64_t scan_pos = 0;          // offset of the entropy-coded data
    int mcus_x = 0, mcus_y = 0;
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Walk the markers up to and including SOS.
int parse(const uint8_t* d, uint64_t len, Header& h) {
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(SAVP_IO_ECORRUPT, "jpeg: no SOI marker");
    uint64_t i = 2;
    bool have_frame = false;
    int adobe = -1;
    for (;;) {
        if (i >= len) return fail(SAVP_IO_ECORRUPT, "jpeg: truncated before SOS");
        if (d[i] != 0xFF) return fail(SAVP_IO_ECORRUPT, "jpeg: marker expected");
        while (i < len && d[i] == 0xFF) ++i;                                  // fill bytes
        if (i >= len) return fail(SAVP_IO_ECORRUPT, "jpeg: truncated before SOS");
        const int m = d[i++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;     // markers without a length
        if (m == 0xD9) return fail(SAVP_IO_ECORRUPT, "jpeg: EOI before SOS");
        if (len - i < 2) return fail(SAVP_IO_ECORRUPT, "jpeg: truncated segment");
        const uint64_t n = ((uint64_t)d[i] << 8) | d[i + 1];
        if (n < 2 || len - i < n) return fail(SAVP_IO_ECORRUPT, "jpeg: truncated segment");
        const uint8_t* s = d + i + 2;
        const int sl = (int)n - 2;
        i += n;
        switch (m) {
            case 0xC0: case 0xC1: {
                if (have_frame) return fail(SAVP_IO_ECORRUPT, "jpeg: more than one frame header");
                if (sl < 6) return fail(SAVP_IO_ECORRUPT, "jpeg: short SOF");
                if (s[0] != 8) return fail(SAVP_IO_EUNSUPPORTED, s[0] == 12 ? "jpeg: 12-bit precision is not supported" : "jpeg: sample precision is not 8 bits");
                h.height = (s[1] << 8) | s[2]; h.width = (s[3] << 8) | s[4]; h.nc = s[5];
                if (h.nc == 4) return fail(SAVP_IO_EUNSUPPORTED, "jpeg: 4 components (CMYK / YCCK) are not supported");
                if (h.nc != 1 && h.nc != 3) return fail(SAVP_IO_EUNSUPPORTED, "jpeg: component count is not 1 or 3");
                if (sl != 6 + 3 * h.nc || h.height == 0 || h.width == 0) return fail(SAVP_IO_ECORRUPT, "jpeg: malformed SOF");
                for (int c = 0; c < h.nc; ++c) {
                    h.c[c].id = s[6 + 3 * c]; h.c[c].h = s[7 + 3 * c] >> 4; h.c[c].v = s[7 + 3 * c] & 15; h.c[c].tq = s[8 + 3 * c];
                    if (h.c[c].tq > 3) return fail(SAVP_IO_ECORRUPT, "jpeg: malformed SOF");
                }
                have_frame = true;
                break;
            }
            case 0xC2: return fail(SAVP_IO_EUNSUPPORTED, "jpeg: progressive streams are not supported");
            case 0xC3: case 0xC7: case 0xCB: case 0xCF: return fail(SAVP_IO_EUNSUPPORTED, "jpeg: lossless streams are not supported");
            case 0xC9: case 0xCA: case 0xCD: case 0xCE: case 0xCC: return fail(SAVP_IO_EUNSUPPORTED, "jpeg: arithmetic coding is not supported");
            case 0xC5: case 0xC6: return fail(SAVP_IO_EUNSUPPORTED, "jpeg: hierarchical streams are not supported");
            case 0xC4: {
                int j = 0;
                while (j < sl) {
                    if (j + 17 > sl) return fail(SAVP_IO_ECORRUPT, "jpeg: short DHT");
                    const int tc = s[j] >> 4, th = s[j] & 15;
                    int tot = 0;
                    for (int k = 0; k < 16; ++k) tot += s[j + 1 + k];
                    if (tc > 1 || th > 3 || tot > 256 || j + 17 + tot > sl) return fail(SAVP_IO_ECORRUPT, "jpeg: malformed DHT");
                    Huff& t = tc ? h.ac[th] : h.dc[th];
                    memcpy(t.counts, s + j + 1, 16);
                    memset(t.values, 0, sizeof(t.values));
                    memcpy(t.values, s + j + 17, (size_t)tot);
                    if (!t.build()) return fail(SAVP_IO_ECORRUPT, "jpeg: over-subscribed DHT");
                    t.present = true;
                    j += 17 + tot;
                }
                break;
            }
            case 0xDB: {
                int j = 0;
                while (j < sl) {
                    const int pq = s[j] >> 4, tq = s[j] & 15;
                    if (pq == 1) return fail(SAVP_IO_EUNSUPPORTED, "jpeg: 16-bit DQT tables are not supported");
                    if (pq > 1 || tq > 3 || j + 65 > sl) return fail(SAVP_IO_ECORRUPT, "jpeg: malformed DQT");
                    for (int k = 0; k < 64; ++k) h.qt[tq][kZigzag[k]] = s[j + 1 + k];
                    h.qt_present[tq] = true;
                    j += 65;
                }
                break;
            }
            case 0xDD:
                if (sl != 2) return fail(SAVP_IO_ECORRUPT, "jpeg: malformed DRI");
                h.restart = (s[0] << 8) | s[1];
                break;
            case 0xEE:
                if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = s[11];
                break;
            case 0xDA: {
                if (!have_frame) return fail(SAVP_IO_ECORRUPT, "jpeg: SOS before SOF");
                if (adobe >= 0 && h.nc == 3 && adobe != 1) return fail(SAVP_IO_EUNSUPPORTED, "jpeg: Adobe marker with a transform other than YCbCr");
                if (h.nc == 1) { h.c[0].h = h.c[0].v = 1; }                   // a one-component scan is never interleaved
                else if (!(h.c[1].h == 1 && h.c[1].v == 1 && h.c[2].h == 1 && h.c[2].v == 1 &&
                           ((h.c[0].h == 1 && h.c[0].v == 1) || (h.c[0].h == 2 && h.c[0].v == 1) || (h.c[0].h == 2 && h.c[0].v == 2))))
                    return fail(SAVP_IO_EUNSUPPORTED, "jpeg: chroma sampling other than 4:4:4, 4:2:2 (2x1) and 4:2:0 is not supported");
                if (sl < 1 || s[0] != h.nc || sl != 4 + 2 * h.nc) {
                    if (sl >= 1 && s[0] >= 1 && s[0] < h.nc && sl == 4 + 2 * s[0])
                        return fail(SAVP_IO_EUNSUPPORTED, "jpeg: non-interleaved scans are not supported");
                    return fail(SAVP_IO_ECORRUPT, "jpeg: malformed SOS");
                }
                for (int c = 0; c < h.nc; ++c) {
                    if (s[1 + 2 * c] != h.c[c].id) return fail(SAVP_IO_ECORRUPT, "jpeg: scan components out of order");
                    h.c[c].td = s[2 + 2 * c] >> 4; h.c[c].ta = s[2 + 2 * c] & 15;
                    if (h.c[c].td > 3 || h.c[c].ta > 3 || !h.dc[h.c[c].td].present || !h.ac[h.c[c].ta].present)
                        return fail(SAVP_IO_ECORRUPT, "jpeg: scan names a Huffman table that was not defined");
                    if (!h.qt_present[h.c[c].tq]) return fail(SAVP_IO_ECORRUPT, "jpeg: frame names a quantisation table that was not defined");
                }
                h.mcus_x = ceil_div(h.width, 8 * h.c[0].h); h.mcus_y = ceil_div(h.height, 8 * h.c[0].v);
                h.scan_pos = i;
                return SAVP_IO_OK;
            }
            default: break;                                                   // APPn, COM, anything else with a length: skipped
        }
    }
}

void fill_info(const Header& h, SavpJpegInfo* o) {
    memset(o, 0, sizeof(*o));
    o->width = h.width; o->height = h.height; o->components = h.nc;
    int32_t off = 0;
    for (int c = 0; c < h.nc; ++c) {
        o->h[c] = h.c[c].h; o->v[c] = h.c[c].v;
        o->blocks_w[c] = h.mcus_x * h.c[c].h; o->blocks_h[c] = h.mcus_y * h.c[c].v;
        o->block_offset[c] = off;
        off += o->blocks_w[c] * o->blocks_h[c];
    }
    o->total_blocks = off;
}

struct Bits {                         // MSB-first bit reader over the entropy-coded segment; 0xFF00 -> 0xFF, any other 0xFFxx ends the data
    const uint8_t* d; uint64_t len, pos;
    uint64_t acc = 0; int n = 0;      // n valid bits at the bottom of acc
    bool starved = false;             // bits were asked for that the stream does not hold
    // Top the accumulator up to more than 32 bits where the stream has them: four bytes at a time while none of them is 0xFF, else byte
    // by byte (a stuffed 0xFF00 gives 0xFF; a marker or the end of the data stops the refill, and the bits that are missing are noticed
    // when they are consumed).
    void refill() {
        while (n <= 32) {
            if (len - pos >= 4) {
                const uint32_t v = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
                if (!((~v - 0x01010101u) & v & 0x80808080u)) { acc = (acc << 32) | v; n += 32; pos += 4; return; }
            }
            if (pos >= len) return;
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= len || d[pos + 1] != 0) return;
                pos += 2;
            } else ++pos;
            acc = (acc << 8) | b; n += 8;
        }
    }
    // the next k (<= 16) bits without consuming them; missing bits read as 0
    uint32_t peek(int k) const {
        if (n >= k) return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1);
        return (uint32_t)(acc << (k - n)) & ((1u << k) - 1);
    }
    void skip(int k) { if (n < k) { starved = true; n = 0; } else n -= k; }
    // one Huffman symbol followed by its `& 15` extra bits need at most 16 + 15 bits: one refill covers both
    int decode(const Huff& t) {
        if (n <= 32) refill();
        const uint32_t p = peek(16);
        const uint16_t e = t.look[p >> 7];
        if (e) { skip(e >> 8); return e & 0xff; }
        for (int l = 10; l <= 16; ++l) {
            const int32_t code = (int32_t)(p >> (16 - l));
            if (code <= t.maxcode[l]) { skip(l); return t.values[(t.valptr[l] + code - t.mincode[l]) & 0xff]; }
        }
        return -1;
    }
    uint32_t get(int k) { if (!k) return 0; const uint32_t v = peek(k); skip(k); return v; }
    // drop the padding bits and read the marker that follows; -1 when there is none
    int marker() {
        n = 0; acc = 0;
        if (pos >= len || d[pos] != 0xFF) return -1;
        while (pos < len && d[pos] == 0xFF) ++pos;
        if (pos >= len) return -1;
        return d[pos++];
    }
};

inline int extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }
}  // namespace

extern "C" const char* savp_jpeg_error(void) { return g_msg; }

extern "C" int savp_jpeg_info(const uint8_t* data, uint64_t len, SavpJpegInfo* out) {
    if (!data || !out) return fail(SAVP_IO_EINVAL, "jpeg: null argument");
    Header h;
    const int rc = parse(data, len, h);
    if (rc) return rc;
    fill_info(h, out);
    return SAVP_IO_OK;
}

extern "C" int savp_jpeg_entropy_decode(const uint8_t* data, uint64_t len, const SavpJpegInfo* expect, int16_t* coef, uint16_t* qtab) {
    if (!data || !expect || !coef || !qtab) return fail(SAVP_IO_EINVAL, "jpeg: null argument");
    Header h;
    int rc = parse(data, len, h);
    if (rc) return rc;
    SavpJpegInfo got;
    fill_info(h, &got);
    if (got.width != expect->width || got.height != expect->height || got.components != expect->components || got.total_blocks != expect->total_blocks ||
        memcmp(got.h, expect->h, sizeof(got.h)) || memcmp(got.v, expect->v, sizeof(got.v)) || memcmp(got.blocks_w, expect->blocks_w, sizeof(got.blocks_w)) ||
        memcmp(got.blocks_h, expect->blocks_h, sizeof(got.blocks_h)) || memcmp(got.block_offset, expect->block_offset, sizeof(got.block_offset)))
        return fail(SAVP_IO_ECORRUPT, "jpeg: geometry differs from the expected one");
    for (int c = 0; c < h.nc; ++c) memcpy(qtab + 64 * c, h.qt[h.c[c].tq], 64 * sizeof(uint16_t));
    memset(coef, 0, (size_t)got.total_blocks * 64 * sizeof(int16_t));
    Bits br{data, len, h.scan_pos};
    int pred[3] = {0, 0, 0};
    int rst = 0;
    long long mcu = 0;
    for (int my = 0; my < h.mcus_y; ++my) {
        for (int mx = 0; mx < h.mcus_x; ++mx, ++mcu) {
            if (h.restart && mcu && mcu % h.restart == 0) {
                if (br.marker() != 0xD0 + rst) return fail(SAVP_IO_ECORRUPT, "jpeg: restart marker expected");
                rst = (rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.nc; ++c) {
                const Huff &td = h.dc[h.c[c].td], &ta = h.ac[h.c[c].ta];
                for (int v = 0; v < h.c[c].v; ++v) {
                    for (int x = 0; x < h.c[c].h; ++x) {
                        // inside [0, total_blocks): my * v + v' < blocks_h, mx * h + x < blocks_w by construction of fill_info
                        int16_t* blk = coef + ((size_t)got.block_offset[c] + (size_t)(my * h.c[c].v + v) * got.blocks_w[c] + mx * h.c[c].h + x) * 64;
                        int s = br.decode(td);
                        if (s < 0 || s > 15) return fail(SAVP_IO_ECORRUPT, "jpeg: bad DC code");
                        pred[c] += extend(br.get(s), s);
                        if (pred[c] < -32768 || pred[c] > 32767) return fail(SAVP_IO_ECORRUPT, "jpeg: DC coefficient out of range");
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = br.decode(ta);
                            if (rs < 0) return fail(SAVP_IO_ECORRUPT, "jpeg: bad AC code");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;                           // EOB
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(SAVP_IO_ECORRUPT, "jpeg: AC run past the end of the block");
                            blk[kZigzag[k]] = (int16_t)extend(br.get(s), s);
                            ++k;
                        }
                        if (br.starved) return fail(SAVP_IO_ECORRUPT, "jpeg: entropy-coded data ends early");
                    }
                }
            }
        }
    }
    const int m = br.marker();
    if (m == 0xDA) return fail(SAVP_IO_EUNSUPPORTED, "jpeg: non-interleaved scans are not supported");
    if (m != 0xD9) return fail(SAVP_IO_ECORRUPT, "jpeg: EOI expected after the scan");
    return SAVP_IO_OK;
}
