// Decoding ONE FLAC frame of a 16-bit stream (RFC 9639) in three steps that the kernels of flac.hip run with different shapes - and
// that tools/flac_check.cpp runs on the CPU, the same code:
//   flac_entropy_frame    the serial bitstream: header, subframe headers, warm-up samples, Rice / escaped residuals -> int32 words
//   flac_restore_channel  the prediction recurrence of one channel, in place (it reads back the samples it has written)
//   flac_output_sample    wasted bits, channel decorrelation undone: the int32 value of sample i of channel c
// A frame's words: [0] 1 once the entropy step has passed (else nothing behind it is read), [1] block size, [2] channel assignment,
// [3] channels; then per channel FLAC_DESC words - kind, order, shift, wasted bits, 32 coefficients - and block-size samples.  Word k
// lies at w[k * stride]: the kernels interleave the words of 64 frames (stride 64), the host uses stride 1.
// Every read of the bitstream is bounded by the frame's byte span (behind it the reader yields zeros and the frame fails), every word
// index by frame_words.
#pragma once
#include "flac_format.h"

enum { FLAC_HDR = 4, FLAC_DESC = 36, FLAC_CONSTANT = 0, FLAC_VERBATIM = 1, FLAC_FIXED = 2, FLAC_LPC = 3 };

// words a frame of `channels` x `block_size` needs
CN_FLAC_HD inline int64_t flac_frame_words(int channels, int block_size) { return FLAC_HDR + (int64_t)channels * (FLAC_DESC + block_size); }

CN_FLAC_HD inline int flac_clz64(uint64_t v) { return __builtin_clzll(v); }  // (v != 0)

struct FlacBits {
    const uint8_t* p;
    int64_t pos, end;  // next byte to load, bytes there are
    uint64_t acc;      // the next n bits, from bit 63 down; zeros below them
    int n;
    CN_FLAC_HD FlacBits(const uint8_t* p_, int64_t len) : p(p_), pos(0), end(len), acc(0), n(0) {}
    CN_FLAC_HD void refill() {
        while (n <= 56) {
            const uint64_t b = pos < end ? p[pos] : 0;
            ++pos;
            acc |= b << (56 - n);
            n += 8;
        }
    }
    CN_FLAC_HD int64_t consumed() const { return pos * 8 - n; }  // bits taken so far
    CN_FLAC_HD bool past_end() const { return consumed() > end * 8; }
    CN_FLAC_HD uint32_t read(int k) {  // 0 <= k <= 32
        if (k == 0) return 0;
        refill();
        const uint32_t v = (uint32_t)(acc >> (64 - k));
        acc <<= k;
        n -= k;
        return v;
    }
    CN_FLAC_HD int32_t read_signed(int k) {  // k-bit two's complement
        if (k == 0) return 0;
        const uint32_t v = read(k);
        return (int32_t)(v << (32 - k)) >> (32 - k);
    }
    // zeros up to the next one bit, which is taken too; false once the run leaves the frame
    CN_FLAC_HD bool unary(uint32_t* count) {
        uint32_t c = 0;
        for (;;) {
            refill();
            if (acc == 0) {
                c += (uint32_t)n;
                n = 0;
                if (pos >= end) return false;
                continue;
            }
            const int lz = flac_clz64(acc);
            c += (uint32_t)lz;
            acc <<= lz;
            acc <<= 1;
            n -= lz + 1;
            *count = c;
            return true;
        }
    }
};

// The entropy step of the frame p[0, len) of an utterance of `channels` channels that has `room` samples per channel left from this
// frame's first one.  0: passed (w[0] = 1); otherwise w[0] = 0 and the reason: 1 header, 2 channels / sample size, 3 block size does
// not fit the utterance or frame_words, 4 subframe header, 5 residual, 6 footer.
CN_FLAC_HD inline int flac_entropy_frame(const uint8_t* p, int64_t len, int channels, int64_t room, int64_t frame_words, int32_t* w, int64_t stride,
                                         bool check_crc8) {
    w[0] = 0;
    FlacFrameHeader h;
    const int hl = flac_parse_header(p, len, &h, check_crc8);
    if (!hl) return 1;
    if (h.channels != channels || (h.bits != 0 && h.bits != 16)) return 2;
    const int bs = h.block_size;
    if (bs > room || flac_frame_words(channels, bs) > frame_words) return 3;
    w[1 * stride] = bs;
    w[2 * stride] = h.assignment;
    w[3 * stride] = channels;
    FlacBits br(p + hl, len - hl);
    for (int c = 0; c < channels; ++c) {
        const bool side = (h.assignment == 8 && c == 1) || (h.assignment == 9 && c == 0) || (h.assignment == 10 && c == 1);
        int bps = 16 + (side ? 1 : 0);
        if (br.read(1)) return 4;
        const int type = (int)br.read(6);
        int wasted = 0;
        if (br.read(1)) {
            uint32_t k;
            if (!br.unary(&k) || k + 1 >= (uint32_t)bps) return 4;
            wasted = (int)k + 1;
        }
        bps -= wasted;
        int32_t* d = w + (FLAC_HDR + (int64_t)c * (FLAC_DESC + bs)) * stride;  // the descriptor
        int32_t* s = d + FLAC_DESC * stride;                                    // the samples
        int kind, order = 0, shift = 0;
        if (type == 0) {
            kind = FLAC_CONSTANT;
            s[0] = br.read_signed(bps);
        } else if (type == 1) {
            kind = FLAC_VERBATIM;
            for (int i = 0; i < bs; ++i) s[i * stride] = br.read_signed(bps);
        } else if ((type & 0x38) == 0x08) {
            kind = FLAC_FIXED;
            order = type & 7;
            if (order > 4) return 4;
        } else if (type & 0x20) {
            kind = FLAC_LPC;
            order = (type & 31) + 1;
        } else return 4;
        if (order > bs) return 4;
        if (kind >= FLAC_FIXED) {
            for (int i = 0; i < order; ++i) s[i * stride] = br.read_signed(bps);
            if (kind == FLAC_LPC) {
                const int prec = (int)br.read(4) + 1;
                shift = br.read_signed(5);
                if (prec == 16 || shift < 0) return 4;
                for (int j = 0; j < order; ++j) d[(4 + j) * stride] = br.read_signed(prec);
            }
            // the residual: 2^po partitions of bs >> po samples, the first short by the predictor order
            const int method = (int)br.read(2);
            if (method > 1) return 5;
            const int pbits = 4 + method, po = (int)br.read(4);
            const int psize = bs >> po;
            if ((psize << po) != bs || psize < order) return 5;
            int i = order;
            for (int part = 0; part < (1 << po); ++part) {
                const int cnt = part ? psize : psize - order;
                const int k = (int)br.read(pbits);
                if (k == (1 << pbits) - 1) {  // escape: raw two's-complement residuals
                    const int nb = (int)br.read(5);
                    for (int e = 0; e < cnt; ++e, ++i) s[i * stride] = br.read_signed(nb);
                } else {
                    for (int e = 0; e < cnt; ++e, ++i) {
                        uint32_t q;
                        if (!br.unary(&q)) return 5;
                        const uint32_t u = (q << k) | br.read(k);
                        s[i * stride] = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
                    }
                }
                if (br.past_end()) return 5;
            }
        }
        if (br.past_end()) return 4;
        d[0] = kind;
        d[1 * stride] = order;
        d[2 * stride] = shift;
        d[3 * stride] = wasted;
    }
    // the footer: zero bits up to the byte boundary, then exactly the two bytes of the CRC-16
    const int padbits = (int)((8 - (br.consumed() & 7)) & 7);
    if (br.read(padbits) != 0 || br.consumed() + 16 != (len - hl) * 8) return 6;
    w[0] = 1;
    return 0;
}

// The prediction of channel c of a frame that passed, in place.  The recurrence reads the samples it has written (no history is kept
// in registers beyond the four of the fixed predictors); sums are 64-bit, the shift arithmetic.
CN_FLAC_HD inline void flac_restore_channel(int32_t* w, int64_t stride, int c) {
    if (w[0] != 1) return;
    const int bs = w[1 * stride];
    int32_t* d = w + (FLAC_HDR + (int64_t)c * (FLAC_DESC + bs)) * stride;
    int32_t* s = d + FLAC_DESC * stride;
    const int kind = d[0], order = d[1 * stride], shift = d[2 * stride];
    if (kind == FLAC_CONSTANT) {
        const int32_t v = s[0];
        for (int i = 1; i < bs; ++i) s[i * stride] = v;
    } else if (kind == FLAC_FIXED) {
        int64_t s1 = order >= 1 ? s[(order - 1) * stride] : 0, s2 = order >= 2 ? s[(order - 2) * stride] : 0;
        int64_t s3 = order >= 3 ? s[(order - 3) * stride] : 0, s4 = order >= 4 ? s[(order - 4) * stride] : 0;
        if (order == 0) return;
        for (int i = order; i < bs; ++i) {
            const int64_t pred = order == 1 ? s1 : order == 2 ? 2 * s1 - s2 : order == 3 ? 3 * s1 - 3 * s2 + s3 : 4 * s1 - 6 * s2 + 4 * s3 - s4;
            const int32_t v = (int32_t)(uint32_t)((int64_t)s[i * stride] + pred);
            s[i * stride] = v;
            s4 = s3;
            s3 = s2;
            s2 = s1;
            s1 = v;
        }
    } else if (kind == FLAC_LPC) {
        for (int i = order; i < bs; ++i) {
            int64_t sum = 0;
            for (int j = 0; j < order; ++j) sum += (int64_t)d[(4 + j) * stride] * (int64_t)s[(i - 1 - j) * stride];  // coefficient 0: the most recent sample
            s[i * stride] = (int32_t)(uint32_t)((int64_t)s[i * stride] + (sum >> shift));
        }
    }
}

// Sample i of channel c of a restored frame as the file's PCM holds it: the wasted bits shifted back in, then left/side, side/right
// or mid/side undone (independent channels pass through).
CN_FLAC_HD inline int32_t flac_output_sample(const int32_t* w, int64_t stride, int c, int i) {
    const int bs = w[1 * stride], assignment = w[2 * stride];
    if (assignment < 8) {
        const int32_t* d = w + (FLAC_HDR + (int64_t)c * (FLAC_DESC + bs)) * stride;
        return (int32_t)((uint32_t)d[(FLAC_DESC + i) * stride] << d[3 * stride]);
    }
    const int32_t* d0 = w + FLAC_HDR * stride;
    const int32_t* d1 = w + (FLAC_HDR + (int64_t)(FLAC_DESC + bs)) * stride;
    const int64_t a = (int32_t)((uint32_t)d0[(FLAC_DESC + i) * stride] << d0[3 * stride]);
    const int64_t b = (int32_t)((uint32_t)d1[(FLAC_DESC + i) * stride] << d1[3 * stride]);
    if (assignment == 8) return (int32_t)(c == 0 ? a : a - b);  // left, side
    if (assignment == 9) return (int32_t)(c == 0 ? a + b : b);  // side, right
    const int64_t m = a * 2 + (b & 1);                          // mid, side
    return (int32_t)((c == 0 ? m + b : m - b) >> 1);
}
