// Stand-alone host program around the entry-point decoder of csrc/ssdhip_jpeg_entropy.h (tests/test_jpeg_index_host_cpu.py builds
// and runs it; the same text builds with -fsanitize=address,undefined for a sanitizer run on the CPU).  Each case is the descriptor
// buffer jpeg_decode.pack_plans makes for ONE image without restart markers (one segment), plus an operation:
//   op 0  RECORD: ssdhip_jpeg_decode_span in recording mode, ckpt_rows entries of room;
//   op 1  INDEXED: one call per entry of the given table, as the entry kernel's lanes make them (first = no entry in front, next =
//         the entry behind or null), the status words ORed.
// Every case also runs ssdhip_jpeg_decode_segment on the same bytes.
//
//   jpeg_index_main IN OUT
//   IN : int32 n_cases, then per case int32[16] {magic 0x4A504958, n_huff, off_images, off_segments, off_huff, off_data, data_bytes,
//        total_blocks, desc_bytes, op, n_entries, ckpt_rows, 0, 0, 0, 0}, desc_bytes bytes, int32 entries[n_entries][8]
//   OUT: per case int32 {sequential status, status}, int16 sequential coef[total_blocks][64], int16 coef[total_blocks][64],
//        int32 ckpt[ckpt_rows][8] (rows never written: -1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ssdhip_jpeg_entropy.h"

static_assert(sizeof(ssdhip_jpeg_entry) == 4 * SSDHIP_JPEG_ENTRY_WORDS, "entry layout");

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_cases = 0;
    if (!read_all(in, &n_cases, 4) || n_cases < 0) return 3;
    for (int c = 0; c < n_cases; ++c) {
        int h[16];
        if (!read_all(in, h, sizeof h) || h[0] != 0x4A504958) return 3;
        const int n_huff = h[1], data_bytes = h[6], total_blocks = h[7], desc_bytes = h[8], op = h[9], n_entries = h[10], ckpt_rows = h[11];
        if (n_huff <= 0 || total_blocks <= 0 || desc_bytes <= 0 || data_bytes < 0 || n_entries < 0 || ckpt_rows < 0 || op < 0 || op > 1)
            return 3;
        // exact-size heap copies of every part: an access one byte outside a part is an access outside an allocation
        std::vector<unsigned char> desc(desc_bytes);
        if (!read_all(in, desc.data(), desc.size())) return 3;
        auto part = [&](int off, long long bytes) {
            if (off < 0 || off + bytes > desc_bytes) exit(3);
            unsigned char* p = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
            memcpy(p, desc.data() + off, bytes);
            return p;
        };
        ssdhip_jpeg_image* image = reinterpret_cast<ssdhip_jpeg_image*>(part(h[2], sizeof(ssdhip_jpeg_image)));
        ssdhip_jpeg_segment* seg = reinterpret_cast<ssdhip_jpeg_segment*>(part(h[3], sizeof(ssdhip_jpeg_segment)));
        ssdhip_jpeg_huff* huff = reinterpret_cast<ssdhip_jpeg_huff*>(part(h[4], (long long)sizeof(ssdhip_jpeg_huff) * n_huff));
        unsigned char* data = part(h[5], data_bytes);
        ssdhip_jpeg_entry* entries = static_cast<ssdhip_jpeg_entry*>(malloc(n_entries ? sizeof(ssdhip_jpeg_entry) * n_entries : 1));
        if (!read_all(in, entries, sizeof(ssdhip_jpeg_entry) * n_entries)) return 3;
        ssdhip_jpeg_entry* ckpt = static_cast<ssdhip_jpeg_entry*>(malloc(ckpt_rows ? sizeof(ssdhip_jpeg_entry) * ckpt_rows : 1));
        memset(ckpt, 0xFF, sizeof(ssdhip_jpeg_entry) * ckpt_rows);
        short* coef_seq = static_cast<short*>(calloc((size_t)total_blocks * 64, sizeof(short)));
        short* coef = static_cast<short*>(calloc((size_t)total_blocks * 64, sizeof(short)));
        if (seg->image != 0) return 3;

        int status[2] = {0, 0};
        status[0] = ssdhip_jpeg_decode_segment(image, seg, huff, n_huff, data, data_bytes, coef_seq, total_blocks);
        if (op == 0) {
            status[1] = ssdhip_jpeg_decode_span(image, seg, nullptr, nullptr, 0, huff, n_huff, data, data_bytes, coef, total_blocks, ckpt,
                                                ckpt_rows);
        } else {
            for (int e = 0; e < n_entries; ++e)
                status[1] |= ssdhip_jpeg_decode_span(image, seg, entries + e, e + 1 < n_entries ? entries + e + 1 : nullptr, e == 0, huff,
                                                     n_huff, data, data_bytes, coef, total_blocks, nullptr, 0);
        }
        fwrite(status, 4, 2, out);
        fwrite(coef_seq, 2, (size_t)total_blocks * 64, out);
        fwrite(coef, 2, (size_t)total_blocks * 64, out);
        fwrite(ckpt, sizeof(ssdhip_jpeg_entry), ckpt_rows, out);
        free(image), free(seg), free(huff), free(data), free(entries), free(ckpt), free(coef_seq), free(coef);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
