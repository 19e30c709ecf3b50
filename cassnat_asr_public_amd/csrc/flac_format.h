// FLAC (RFC 9639) frame headers, the two CRCs and the exact frame index of a stream.  Plain C++ that hipcc (host and device pass) and a
// host compiler accept: the library's host side (cn_host_flac_index, ops.hip), the decode kernels (flac.hip, through flac_decode.h)
// and the stand-alone checker (tools/flac_check.cpp) include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CN_FLAC_HD __host__ __device__
#else
#define CN_FLAC_HD
#endif

struct FlacFrameHeader {
    int variable;     // blocking-strategy bit: the coded number counts samples (1) or frames (0)
    int block_size;   // samples per channel, 1 .. 65536
    int rate;         // Hz; 0: "as STREAMINFO says"
    int assignment;   // 0-7: that many + 1 independent channels; 8 left/side, 9 side/right, 10 mid/side
    int channels;
    int bits;         // bits per sample; 0: "as STREAMINFO says"
    uint64_t number;  // the coded frame / sample number
    int length;       // bytes of the header, its CRC-8 included
};

CN_FLAC_HD inline uint8_t flac_crc8(const uint8_t* p, int n) {  // polynomial 0x07, initial value 0
    uint32_t c = 0;
    for (int i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    return (uint8_t)c;
}

// The header that starts at p (avail bytes are readable) -> its length, 0 when p does not begin a well-formed header.  check_crc: the
// CRC-8 behind it must match (the index: always; the kernels trust an index that was built so).
CN_FLAC_HD inline int flac_parse_header(const uint8_t* p, int64_t avail, FlacFrameHeader* h, bool check_crc) {
    if (avail < 6 || p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return 0;  // 15-bit sync, reserved bit 0
    h->variable = p[1] & 1;
    const int bs_code = p[2] >> 4, rate_code = p[2] & 15, ch_code = p[3] >> 4, size_code = (p[3] >> 1) & 7;
    if ((p[3] & 1) || bs_code == 0 || rate_code == 15 || ch_code > 10 || size_code == 3) return 0;
    h->assignment = ch_code;
    h->channels = ch_code < 8 ? ch_code + 1 : 2;
    h->bits = size_code == 0 ? 0 : size_code == 1 ? 8 : size_code == 2 ? 12 : size_code == 4 ? 16 : size_code == 5 ? 20 : size_code == 6 ? 24 : 32;
    // the coded number: 0xxxxxxx, or 110xxxxx .. 11111110 followed by 1 .. 6 bytes 10xxxxxx
    const int b0 = p[4];
    int extra = 0;
    uint64_t v = 0;
    if (b0 < 0x80) v = (uint64_t)b0;
    else if (b0 < 0xC0 || b0 == 0xFF) return 0;
    else {
        while (extra < 7 && (b0 & (0x80 >> extra))) ++extra;  // leading ones
        v = (uint64_t)(b0 & (0x7F >> extra));
        --extra;
    }
    int n = 5;
    if (avail < n + extra + 1) return 0;
    for (int i = 0; i < extra; ++i, ++n) {
        if ((p[n] & 0xC0) != 0x80) return 0;
        v = (v << 6) | (uint64_t)(p[n] & 0x3F);
    }
    h->number = v;
    const int tail = (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + (rate_code == 12 ? 1 : rate_code >= 13 ? 2 : 0);
    if (avail < n + tail + 1) return 0;
    if (bs_code == 1) h->block_size = 192;
    else if (bs_code <= 5) h->block_size = 576 << (bs_code - 2);
    else if (bs_code == 6) h->block_size = p[n++] + 1;
    else if (bs_code == 7) {
        h->block_size = ((p[n] << 8) | p[n + 1]) + 1;
        n += 2;
    } else h->block_size = 256 << (bs_code - 8);
    switch (rate_code) {
        case 0: h->rate = 0; break;
        case 1: h->rate = 88200; break;
        case 2: h->rate = 176400; break;
        case 3: h->rate = 192000; break;
        case 4: h->rate = 8000; break;
        case 5: h->rate = 16000; break;
        case 6: h->rate = 22050; break;
        case 7: h->rate = 24000; break;
        case 8: h->rate = 32000; break;
        case 9: h->rate = 44100; break;
        case 10: h->rate = 48000; break;
        case 11: h->rate = 96000; break;
        case 12: h->rate = p[n++] * 1000; break;
        case 13: h->rate = (p[n] << 8) | p[n + 1]; n += 2; break;
        default: h->rate = ((p[n] << 8) | p[n + 1]) * 10; n += 2; break;
    }
    if (check_crc && flac_crc8(p, n) != p[n]) return 0;
    h->length = n + 1;
    return n + 1;
}

// ---- host only from here: the CRC-16 and the index
struct FlacCrc16Table {  // polynomial 0x8005, initial value 0, most significant bit first; t[k][i]: byte i followed by k zero bytes
    uint16_t t[8][256];
    FlacCrc16Table() {
        for (int i = 0; i < 256; ++i) {
            uint32_t c = (uint32_t)i << 8;
            for (int b = 0; b < 8; ++b) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
            t[0][i] = (uint16_t)c;
        }
        for (int k = 1; k < 8; ++k)
            for (int i = 0; i < 256; ++i) t[k][i] = (uint16_t)((t[k - 1][i] << 8) ^ t[0][t[k - 1][i] >> 8]);
    }
};

inline const FlacCrc16Table& flac_crc16_table() {
    static const FlacCrc16Table table;
    return table;
}

// the CRC-16 c of some bytes, continued over p[0, n): eight bytes per step
inline uint16_t flac_crc16_update(uint16_t c, const uint8_t* p, int64_t n) {
    const FlacCrc16Table& T = flac_crc16_table();
    for (; n >= 8; p += 8, n -= 8)
        c = (uint16_t)(T.t[7][(c >> 8) ^ p[0]] ^ T.t[6][(c & 0xFF) ^ p[1]] ^ T.t[5][p[2]] ^ T.t[4][p[3]] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^
                       T.t[0][p[7]]);
    for (; n > 0; ++p, --n) c = (uint16_t)((c << 8) ^ T.t[0][(c >> 8) ^ p[0]]);
    return c;
}

inline uint16_t flac_crc16(const uint8_t* p, int64_t n) { return flac_crc16_update(0, p, n); }

enum { FLAC_INDEX_OK = 0, FLAC_INDEX_NO_CHAIN = -2, FLAC_INDEX_FORMAT = -3, FLAC_INDEX_CAPACITY = -5, FLAC_INDEX_RANGE = -6 };

// The exact frame index of the audio bytes d[0, n) of a stream whose STREAMINFO says (rate, channels, bits): one linear pass.  From
// the start of the current frame a running CRC-16 is kept; a later position becomes the next frame start only when a complete,
// matching header with the expected next number stands there AND the two bytes in front of it are the running CRC-16 of everything
// before them - a sync pattern inside a payload, even one with a correct CRC-8, is stepped over.  The last frame ends at n, where its
// CRC-16 is checked.  (Only a position that shows the two sync bytes - or the end - can pass, so the running CRC is brought up to
// such positions in strides and compared there; every byte still goes through it once.)  out (cap rows of three int32, or NULL to
// count): byte offset, byte length, first sample.  *bad: the offset of the frame whose end was never found (NO_CHAIN) or of the
// header that differs from STREAMINFO (FORMAT).
inline int flac_index(const uint8_t* d, int64_t n, int rate, int channels, int bits, int32_t* out, int64_t cap, int64_t* frames, int64_t* samples,
                      int64_t* bad) {
    *frames = *samples = *bad = 0;
    if (n >= ((int64_t)1 << 31)) return FLAC_INDEX_RANGE;
    FlacFrameHeader cur, nxt;
    if (!flac_parse_header(d, n, &cur, true) || cur.number != 0) return FLAC_INDEX_NO_CHAIN;
    auto differs = [&](const FlacFrameHeader& h) { return (h.rate && h.rate != rate) || h.channels != channels || (h.bits && h.bits != bits); };
    if (differs(cur)) return FLAC_INDEX_FORMAT;
    const int variable = cur.variable;
    int64_t start = 0, nf = 0, total = 0, crc_pos = 0;  // crc: the CRC-16 of d[start, crc_pos)
    uint16_t crc = 0;
    int64_t q = cur.length + 3;  // the first position at which the current frame can end: header, a subframe byte, the CRC-16
    for (;;) {
        if (q > n) break;
        if (q < n) {  // on to the next position that shows the sync bytes, else to the end
            const void* hit = q + 1 < n ? memchr(d + q, 0xFF, (size_t)(n - 1 - q)) : nullptr;
            q = hit ? static_cast<const uint8_t*>(hit) - d : n;
            if (q < n && d[q + 1] != (0xF8 | variable)) {
                ++q;
                continue;
            }
        }
        crc = flac_crc16_update(crc, d + crc_pos, q - 2 - crc_pos);
        crc_pos = q - 2;
        if (crc == (uint16_t)((d[q - 2] << 8) | d[q - 1])) {
            bool next = false;
            if (q < n && flac_parse_header(d + q, n - q, &nxt, true) && nxt.number == (uint64_t)(variable ? total + cur.block_size : nf + 1)) {
                if (differs(nxt)) {
                    *bad = q;
                    return FLAC_INDEX_FORMAT;
                }
                next = true;
            }
            if (next || q == n) {
                if (out) {
                    if (nf >= cap) return FLAC_INDEX_CAPACITY;
                    out[3 * nf] = (int32_t)start;
                    out[3 * nf + 1] = (int32_t)(q - start);
                    out[3 * nf + 2] = (int32_t)total;
                }
                ++nf;
                total += cur.block_size;
                if (total >= ((int64_t)1 << 31)) return FLAC_INDEX_RANGE;
                if (q == n) {
                    *frames = nf;
                    *samples = total;
                    return FLAC_INDEX_OK;
                }
                start = crc_pos = q;
                cur = nxt;
                crc = 0;
                q = start + cur.length + 3;
                continue;
            }
        }
        if (q == n) break;
        ++q;
    }
    *bad = start;
    return FLAC_INDEX_NO_CHAIN;
}
