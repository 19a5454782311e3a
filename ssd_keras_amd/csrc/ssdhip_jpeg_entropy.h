// Baseline JPEG entropy decoding of ONE restart segment, as text that compiles for the device (csrc/ssdhip_jpeg.hip: one lane per
// segment) and for the host (tests/test_jpeg_entropy_host_cpu.py builds it with the host compiler; a CPU sanitizer build reads the
// same text).  Sequential Huffman decoding as libjpeg performs it: FF 00 unstuffing, DC prediction from 0 at the start of the
// segment, EOB / ZRL, an 8-bit look-ahead table with a bit-by-bit continuation up to 16 bits.
//
// Memory-safe by construction, whatever the compressed bytes are:
//   * every loop has a trip count fixed before it starts (MCUs of the segment, blocks of an MCU, 63 coefficients, 16 code bits,
//     one word or 5 bytes per refill);
//   * a byte is read only at begin <= pos < end (four at once only where pos + 4 <= end); behind `end`, or behind a marker (FF followed by anything but 00), the reader
//     delivers zero bits, and CONSUMING one of those sets SSDHIP_JPEG_ST_TRUNCATED and stops the segment;
//   * every table index is masked or clamped, every coefficient index is checked against 63;
//   * a code no table row holds (SSDHIP_JPEG_ST_BADCODE) and a run that passes coefficient 63 (SSDHIP_JPEG_ST_RUN) stop the
//     segment too.  libjpeg only warns about those and goes on; here the image goes back to the host decoder, whose result or
//     exception is what the caller sees.
// The caller gets the status as the return value and stores it (ordinary stores; a non-zero word per image).
//
// A segment can also be entered at the start of any MCU row, given an ENTRY: where the next unread bit lies and what the DC predictors
// are there (struct ssdhip_jpeg_entry).  `ssdhip_jpeg_decode_span` RECORDS the entries of a segment while it decodes it sequentially,
// and later decodes one entry's MCUs alone, one lane per entry.  Each lane VERIFIES that it ends exactly where the next entry begins
// (byte, bit, predictors, MCU number), the first entry must be the segment's own start and the last must end at its last MCU: so if
// every lane returns 0, lane 0 decoded what the sequential decoder decodes, ended in the sequential decoder's state, which is lane
// 1's entry, and so on -- the coefficients are the sequential ones by induction, whatever the entries were.  Entries are untrusted
// input like the bytes: a field out of range is SSDHIP_JPEG_ST_DESC, an entry that does not chain SSDHIP_JPEG_ST_INDEX.
#ifndef SSDHIP_JPEG_ENTROPY_H
#define SSDHIP_JPEG_ENTROPY_H

#if defined(__HIPCC__)
#define SSDHIP_JPEG_HD __host__ __device__
#else
#define SSDHIP_JPEG_HD
#endif

#define SSDHIP_JPEG_ST_TRUNCATED 1   /* the segment's bits ran out (its end, or a marker inside it) */
#define SSDHIP_JPEG_ST_BADCODE 2     /* 16 bits that are no code of the table                        */
#define SSDHIP_JPEG_ST_RUN 4         /* a zero run or ZRL that passes coefficient 63                 */
#define SSDHIP_JPEG_ST_RANGE 8       /* block stage: values no 8-bit image produces (ssdhip_jpeg.hip) */
#define SSDHIP_JPEG_ST_DESC 16       /* a descriptor that does not describe the buffers              */
#define SSDHIP_JPEG_ST_INDEX 32      /* an entry the lane in front of it does not end on (or a first / last entry that is none) */

#define SSDHIP_JPEG_IMAGE_WORDS 24
#define SSDHIP_JPEG_SEGMENT_WORDS 4
#define SSDHIP_JPEG_HUFF_BYTES 912
#define SSDHIP_JPEG_ENTRY_WORDS 8

// One Huffman table in look-up form.  look[b]: (code length << 8) | symbol for the code that starts the 8 bits b, 0 if it is longer
// than 8 bits; maxcode[l] the largest code of length l (-1: none), valoff[l] = index of its first symbol minus its first code.
struct ssdhip_jpeg_huff {
    unsigned short look[256];
    int maxcode[18];
    int valoff[18];
    unsigned char vals[256];
};

// One image of a batch (SSDHIP_JPEG_IMAGE_WORDS ints).  Component c has hs_c x vs_c blocks per MCU (luma hs x vs, chroma 1 x 1),
// its blocks form a (mcuy vs_c) x (mcux hs_c) grid, and the grids follow each other from block `coef_base` of the workspace.
struct ssdhip_jpeg_image {
    int height, width, ncomp, hs, vs, mcux, mcuy, interval;      // interval: MCUs per segment (all of them without DRI)
    int qt[3], dc[3], ac[3];                                     // table numbers in the batch's quantisation / Huffman arrays
    int coef_base;                                               // first block of the image in the coefficient / plane workspace
    long long out_offset;                                        // byte offset of the image in the output buffer
    int nblocks, pad0, pad1, pad2;
};

struct ssdhip_jpeg_segment {
    int image, begin, end, first_mcu;                            // begin / end: byte range in the batch's compressed bytes
};

// One entry point into a segment (SSDHIP_JPEG_ENTRY_WORDS ints): MCUs first_mcu .. first_mcu + n_mcus - 1 of `image` start at bit
// `bit` (0..7, counted from the most significant) of the raw byte at offset `byte` of the batch's compressed bytes -- the byte that
// holds the next unread bit, never the 00 of an FF 00 pair -- with the DC predictors pred0..2.
struct ssdhip_jpeg_entry {
    int image, byte, bit, first_mcu, n_mcus, pred0, pred1, pred2;
};

struct ssdhip_jpeg_bits {
    const unsigned char* data;
    int pos, end;
    unsigned long long acc; // the low `nbits` bits are the next bits of the stream, most significant first
    int nbits, fake;        // fake: how many of them (the lowest) were made up behind the segment's end
};

// Refill to more than 32 bits: a Huffman code (<= 16) and the value bits behind it (<= 15) need no second refill.  Four bytes at
// once where the segment has four more and none of them is FF (nothing to unstuff, no marker); byte by byte otherwise.
SSDHIP_JPEG_HD static inline void ssdhip_jpeg_fill(ssdhip_jpeg_bits& r) {
    if (r.nbits > 32) return;
    if (r.pos + 4 <= r.end) {
        unsigned int w;
        __builtin_memcpy(&w, r.data + r.pos, 4);
        if ((((w & 0x7F7F7F7Fu) + 0x01010101u) & w & 0x80808080u) == 0) {       // no byte of w is FF
            r.acc = (r.acc << 32) | __builtin_bswap32(w);
            r.nbits += 32;
            r.pos += 4;
            return;
        }
    }
    for (int k = 0; k < 5; ++k) {
        if (r.nbits > 32) break;
        unsigned int b = 0;
        if (r.pos < r.end) {
            b = r.data[r.pos++];
            if (b == 0xFF) {
                if (r.pos < r.end && r.data[r.pos] == 0) {
                    ++r.pos;                                     // FF 00: a stuffed FF
                } else {
                    b = 0;                                       // a marker (or the end right behind FF): no data from here on,
                    r.end = --r.pos;                             // and pos stays on the first byte that is none
                    r.fake += 8;
                }
            }
        } else {
            r.fake += 8;
        }
        r.acc = (r.acc << 8) | b;
        r.nbits += 8;
    }
}

// Take n <= 16 bits (nbits >= n: a fill leaves more than 32, a code takes at most 16 of them); returns 0 if made-up bits were consumed.
SSDHIP_JPEG_HD static inline int ssdhip_jpeg_take(ssdhip_jpeg_bits& r, int n, unsigned int* value) {
    r.nbits -= n;
    *value = (unsigned int)(r.acc >> r.nbits) & ((1u << n) - 1u);
    return r.nbits >= r.fake;
}

// One Huffman symbol; returns 0 or a status.
SSDHIP_JPEG_HD static inline int ssdhip_jpeg_symbol(ssdhip_jpeg_bits& r, const ssdhip_jpeg_huff* h, int* symbol) {
    ssdhip_jpeg_fill(r);
    const unsigned int top = (unsigned int)(r.acc >> (r.nbits - 16)) & 0xFFFFu;      // the next 16 bits
    unsigned int look = h->look[top >> 8], code = 0;
    int len = (int)(look >> 8);
    if (len >= 1 && len <= 8) {
        *symbol = (int)(look & 255u);
    } else {
        len = 17;
        for (int l = 9; l <= 16; ++l) {
            const unsigned int c = top >> (16 - l);
            if (len == 17 && (int)c <= h->maxcode[l]) {
                len = l;
                code = c;
            }
        }
        if (len == 17) return SSDHIP_JPEG_ST_BADCODE;
        *symbol = h->vals[((int)code + h->valoff[len]) & 255];
    }
    unsigned int ignored;
    return ssdhip_jpeg_take(r, len, &ignored) ? 0 : SSDHIP_JPEG_ST_TRUNCATED;
}

SSDHIP_JPEG_HD static inline int ssdhip_jpeg_extend(unsigned int v, int s) {
    return s == 0 ? 0 : ((int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v);
}

// Where the next unread bit lies in the raw bytes: the reader is `real` = nbits - fake genuine bits ahead of it, so step back from
// pos over ceil(real / 8) data bytes (a trip count fixed before the loop starts, at most 8), taking FF 00 as the one byte it is.  A
// 00 behind an FF is always the stuffing, never data.  Reads stay inside [begin, pos).
SSDHIP_JPEG_HD static inline void ssdhip_jpeg_position(const ssdhip_jpeg_bits& r, int begin, int* byte, int* bit) {
    const int real = r.nbits > r.fake ? r.nbits - r.fake : 0;
    const int back = (real + 7) >> 3;
    int q = r.pos;
    for (int i = 0; i < back; ++i) {
        if (q > begin) --q;
        if (q > begin && q < r.pos && r.data[q] == 0 && r.data[q - 1] == 0xFF) --q;
    }
    *byte = q;
    *bit = back * 8 - real;
}

// The one decoder behind ssdhip_jpeg_decode_segment and ssdhip_jpeg_decode_span (always inlined: each caller passes constants for
// the modes it does not use).  entry == null: the segment from its start; else that entry's MCUs, `first` saying that no entry of the
// segment precedes it.  next: the entry to end on (verifying mode).  ckpt: ckpt_rows entries to record into, [MCU row].
SSDHIP_JPEG_HD static inline __attribute__((always_inline)) int ssdhip_jpeg_decode_core(
    const ssdhip_jpeg_image* im, const ssdhip_jpeg_segment* seg, const ssdhip_jpeg_huff* huff, int n_huff, const unsigned char* data,
    int data_bytes, short* coef, long long coef_blocks, const ssdhip_jpeg_entry* entry, int first, const ssdhip_jpeg_entry* next,
    ssdhip_jpeg_entry* ckpt, int ckpt_rows) {
    const unsigned char natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const int ncomp = im->ncomp, hs = im->hs, vs = im->vs, mcux = im->mcux, mcuy = im->mcuy;
    if ((ncomp != 1 && ncomp != 3) || hs < 1 || hs > 2 || vs < 1 || vs > hs || (ncomp == 1 && (hs != 1 || vs != 1)) || mcux < 1 ||
        mcuy < 1 || mcux > 8192 || mcuy > 8192 || im->interval < 1 || n_huff < 1 || im->coef_base < 0)
        return SSDHIP_JPEG_ST_DESC;
    const int total = mcux * mcuy;
    if (seg->first_mcu < 0 || seg->first_mcu >= total || seg->begin < 0 || seg->end < seg->begin || seg->end > data_bytes)
        return SSDHIP_JPEG_ST_DESC;
    int last_mcu = im->interval < total - seg->first_mcu ? seg->first_mcu + im->interval : total;
    int first_mcu = seg->first_mcu;

    ssdhip_jpeg_bits r;
    r.data = data, r.pos = seg->begin, r.end = seg->end, r.acc = 0, r.nbits = 0, r.fake = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;                         // (scalars, not arrays indexed by c: those would live in scratch memory)
    const int base1 = mcux * hs * mcuy * vs, base2 = base1 + mcux * mcuy;   // component grids inside the image's blocks

    if (entry) {                                                 // every field is untrusted
        const int bit = entry->bit & 7;
        if (entry->first_mcu < first_mcu || entry->first_mcu >= last_mcu || entry->n_mcus < 1 ||
            entry->n_mcus > last_mcu - entry->first_mcu || entry->byte < seg->begin || entry->byte > seg->end || bit != entry->bit)
            return SSDHIP_JPEG_ST_DESC;
        if (first && (entry->first_mcu != first_mcu || entry->byte != seg->begin || bit != 0 || entry->pred0 != 0 || entry->pred1 != 0 ||
                      entry->pred2 != 0))
            return SSDHIP_JPEG_ST_INDEX;
        if (next ? next->first_mcu != entry->first_mcu + entry->n_mcus : entry->first_mcu + entry->n_mcus != last_mcu)
            return SSDHIP_JPEG_ST_INDEX;
        first_mcu = entry->first_mcu, last_mcu = entry->first_mcu + entry->n_mcus;
        pred0 = entry->pred0, pred1 = entry->pred1, pred2 = entry->pred2;
        r.pos = entry->byte;
        if (bit != 0) {                                          // drop the bits of the first byte that belong to the MCU in front
            ssdhip_jpeg_fill(r);
            r.nbits -= bit;
            if (r.nbits < r.fake) return SSDHIP_JPEG_ST_TRUNCATED;
        }
    }

    for (int mcu = first_mcu; mcu < last_mcu; ++mcu) {
        const int my = mcu / mcux, mx = mcu - my * mcux;
        if (ckpt && (mx == 0 || mcu == first_mcu)) {             // recording: the entry of this MCU row
            if (my >= ckpt_rows) return SSDHIP_JPEG_ST_DESC;
            ssdhip_jpeg_entry e;
            ssdhip_jpeg_position(r, seg->begin, &e.byte, &e.bit);
            e.image = seg->image, e.first_mcu = mcu, e.n_mcus = mcux - mx < last_mcu - mcu ? mcux - mx : last_mcu - mcu;
            e.pred0 = pred0, e.pred1 = pred1, e.pred2 = pred2;
            ckpt[my] = e;
        }
        for (int c = 0; c < ncomp; ++c) {
            const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
            const int grid_base = c == 0 ? 0 : (c == 1 ? base1 : base2), grid_w = c == 0 ? mcux * hs : mcux;
            const int idc = im->dc[c], iac = im->ac[c];
            const ssdhip_jpeg_huff* hdc = huff + (idc < 0 ? 0 : (idc >= n_huff ? n_huff - 1 : idc));
            const ssdhip_jpeg_huff* hac = huff + (iac < 0 ? 0 : (iac >= n_huff ? n_huff - 1 : iac));
            for (int b = 0; b < ch * cv; ++b) {
                const int by = my * cv + b / ch, bx = mx * ch + b % ch;
                const long long block = (long long)im->coef_base + grid_base + (long long)by * grid_w + bx;
                if (block < 0 || block >= coef_blocks) return SSDHIP_JPEG_ST_DESC;
                short* out = coef + block * 64;
                for (int k = 0; k < 64; ++k) out[k] = 0;

                int sym, st;
                unsigned int v;
                if ((st = ssdhip_jpeg_symbol(r, hdc, &sym)) != 0) return st;
                const int sdc = sym & 15;                        // the plan admits DC tables with categories 0..15 only
                if (!ssdhip_jpeg_take(r, sdc, &v)) return SSDHIP_JPEG_ST_TRUNCATED;
                const int dc = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + ssdhip_jpeg_extend(v, sdc);
                pred0 = c == 0 ? dc : pred0, pred1 = c == 1 ? dc : pred1, pred2 = c == 2 ? dc : pred2;
                out[0] = (short)dc;

                int k = 1;
                for (int it = 0; it < 63; ++it) {
                    if (k > 63) break;
                    if ((st = ssdhip_jpeg_symbol(r, hac, &sym)) != 0) return st;
                    const int run = sym >> 4, s = sym & 15;
                    if (s == 0) {
                        if (run != 15) break;                    // EOB
                        k += 16;                                 // ZRL
                        if (k > 64) return SSDHIP_JPEG_ST_RUN;
                    } else {
                        k += run;
                        if (k > 63) return SSDHIP_JPEG_ST_RUN;
                        if (!ssdhip_jpeg_take(r, s, &v)) return SSDHIP_JPEG_ST_TRUNCATED;
                        out[natural[k & 63]] = (short)ssdhip_jpeg_extend(v, s);
                        ++k;
                    }
                }
            }
        }
    }
    if (next) {                                                  // verifying: this lane ends exactly where the next one was told to start
        int byte, bit;
        ssdhip_jpeg_position(r, seg->begin, &byte, &bit);
        if (byte != next->byte || bit != next->bit || pred0 != next->pred0 || pred1 != next->pred1 || pred2 != next->pred2)
            return SSDHIP_JPEG_ST_INDEX;
    }
    return 0;
}

// Decode segment `seg` of image `im`: its MCUs first_mcu .. first_mcu + interval - 1 (clipped to the image), coefficients as int16
// [block][64] in natural order into `coef` (the WHOLE workspace of `coef_blocks` blocks; this function zero-fills and writes only
// the segment's own blocks, each checked against coef_blocks).  `huff`: the batch's n_huff tables, `data`: its data_bytes
// compressed bytes.  Returns 0 or the status that stopped the segment.
SSDHIP_JPEG_HD static inline int ssdhip_jpeg_decode_segment(const ssdhip_jpeg_image* im, const ssdhip_jpeg_segment* seg,
                                                            const ssdhip_jpeg_huff* huff, int n_huff, const unsigned char* data,
                                                            int data_bytes, short* coef, long long coef_blocks) {
    return ssdhip_jpeg_decode_core(im, seg, huff, n_huff, data, data_bytes, coef, coef_blocks, nullptr, 0, nullptr, nullptr, 0);
}

// Two modes, both writing coefficients exactly as ssdhip_jpeg_decode_segment does (zero-filling every block they start).
//   RECORDING (ckpt_out != null; entry, next_entry ignored): the whole segment, sequentially; at the start of MCU row `my` the entry
//     that describes that point goes to ckpt_out[my] (my < ckpt_rows is checked).  Status 0 means every row's entry was written.
//   SPAN (ckpt_out == null): the MCUs of `entry` only.  `first` != 0: no entry of the segment precedes it, so it must be the
//     segment's start.  next_entry != null: the lane must end on it (VERIFYING, header comment); null: the entry must end at the
//     segment's last MCU, and the sequential rules hold from there.  SSDHIP_JPEG_ST_DESC for a field outside the segment / image,
//     SSDHIP_JPEG_ST_INDEX for an entry that does not chain; never a read or write out of range.
SSDHIP_JPEG_HD static inline int ssdhip_jpeg_decode_span(const ssdhip_jpeg_image* im, const ssdhip_jpeg_segment* seg,
                                                         const ssdhip_jpeg_entry* entry, const ssdhip_jpeg_entry* next_entry, int first,
                                                         const ssdhip_jpeg_huff* huff, int n_huff, const unsigned char* data,
                                                         int data_bytes, short* coef, long long coef_blocks,
                                                         ssdhip_jpeg_entry* ckpt_out, int ckpt_rows) {
    if (ckpt_out)
        return ssdhip_jpeg_decode_core(im, seg, huff, n_huff, data, data_bytes, coef, coef_blocks, nullptr, 0, nullptr, ckpt_out, ckpt_rows);
    if (!entry) return SSDHIP_JPEG_ST_DESC;
    return ssdhip_jpeg_decode_core(im, seg, huff, n_huff, data, data_bytes, coef, coef_blocks, entry, first, next_entry, nullptr, 0);
}

#endif /* SSDHIP_JPEG_ENTROPY_H */
