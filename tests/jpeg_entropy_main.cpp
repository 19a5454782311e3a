// Stand-alone host program around csrc/ssdhip_jpeg_entropy.h (tests/test_jpeg_entropy_host_cpu.py builds and runs it; the same text
// builds with -fsanitize=address,undefined for a sanitizer run on the CPU).  It reads cases written by the test -- each one the
// descriptor buffer jpeg_decode.pack_plans makes for the device -- decodes every segment of every case with the function the
// entropy kernel calls, and writes status words and coefficients.
//
//   jpeg_entropy_main IN OUT
//   IN : int32 n_cases, then per case int32[12] {magic 0x4A504547, n_images, n_segments, n_huff, off_images, off_segments, off_huff,
//        off_data, data_bytes, total_blocks, desc_bytes, 0} and desc_bytes bytes
//   OUT: per case int32 status[n_images], int16 coef[total_blocks][64]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ssdhip_jpeg_entropy.h"

static_assert(sizeof(ssdhip_jpeg_image) == 4 * SSDHIP_JPEG_IMAGE_WORDS, "image descriptor layout");
static_assert(sizeof(ssdhip_jpeg_segment) == 4 * SSDHIP_JPEG_SEGMENT_WORDS, "segment descriptor layout");
static_assert(sizeof(ssdhip_jpeg_huff) == SSDHIP_JPEG_HUFF_BYTES, "Huffman table layout");

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
        int h[12];
        if (!read_all(in, h, sizeof h) || h[0] != 0x4A504547) return 3;
        const int n_images = h[1], n_segments = h[2], n_huff = h[3], data_bytes = h[8], total_blocks = h[9], desc_bytes = h[10];
        if (n_images <= 0 || n_segments <= 0 || n_huff <= 0 || total_blocks <= 0 || desc_bytes <= 0 || data_bytes < 0) return 3;
        // exact-size heap copies of every part: a read one byte outside a part is a read outside an allocation
        std::vector<unsigned char> desc(desc_bytes);
        if (!read_all(in, desc.data(), desc.size())) return 3;
        auto part = [&](int off, long long bytes) {
            if (off < 0 || off + bytes > desc_bytes) exit(3);
            unsigned char* p = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
            memcpy(p, desc.data() + off, bytes);
            return p;
        };
        ssdhip_jpeg_image* images = reinterpret_cast<ssdhip_jpeg_image*>(part(h[4], (long long)sizeof(ssdhip_jpeg_image) * n_images));
        ssdhip_jpeg_segment* segments = reinterpret_cast<ssdhip_jpeg_segment*>(part(h[5], (long long)sizeof(ssdhip_jpeg_segment) * n_segments));
        ssdhip_jpeg_huff* huff = reinterpret_cast<ssdhip_jpeg_huff*>(part(h[6], (long long)sizeof(ssdhip_jpeg_huff) * n_huff));
        unsigned char* data = part(h[7], data_bytes);
        short* coef = static_cast<short*>(calloc((size_t)total_blocks * 64, sizeof(short)));
        std::vector<int> status(n_images, 0);
        for (int s = 0; s < n_segments; ++s) {
            const ssdhip_jpeg_segment seg = segments[s];
            if (seg.image < 0 || seg.image >= n_images) return 3;
            const int st = ssdhip_jpeg_decode_segment(&images[seg.image], &seg, huff, n_huff, data, data_bytes, coef, total_blocks);
            status[seg.image] |= st;
        }
        fwrite(status.data(), 4, n_images, out);
        fwrite(coef, 2, (size_t)total_blocks * 64, out);
        free(images), free(segments), free(huff), free(data), free(coef);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
