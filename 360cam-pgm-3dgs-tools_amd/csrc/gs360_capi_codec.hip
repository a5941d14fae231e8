// gs360_capi_codec.hip -- host-only image-codec helpers of libgs360hip.so (include/gs360.h): PNG scanline unfiltering and TIFF
// LZW strip decoding for the Python-side codec (gs360/imageio.py).  No GPU involved.
#include "gs360_capi_internal.h"

using namespace gs360;

// PNG scanline reconstruction (filter types 0-4) in place: `data` holds h rows of (1 + stride) bytes as inflated from the
// IDAT stream; on return row y's pixels sit at data + y * (stride + 1) + 1.  Both directions of a PNG filter are
// sequential (left neighbour and previous row), so the Python-side codec (gs360/imageio.py, used for 16-bit PNG, which
// Pillow cannot deliver at full depth for RGB) calls this instead of looping over bytes.  No GPU involved.
int gs360_png_unfilter(uint8_t* data, int h, int stride, int bpp) {
    if (!data || h < 0 || stride < 1 || bpp < 1 || bpp > 8) return fail(GS360_ERR_ARG, "bad PNG geometry");
    const size_t pitch = (size_t)stride + 1;
    for (int y = 0; y < h; ++y) {
        uint8_t* cur = data + (size_t)y * pitch + 1;
        const uint8_t* up = y ? cur - pitch : nullptr;
        const int ft = cur[-1];
        switch (ft) {
            case 0: break;
            case 1: for (int i = bpp; i < stride; ++i) cur[i] = (uint8_t)(cur[i] + cur[i - bpp]); break;
            case 2: if (up) for (int i = 0; i < stride; ++i) cur[i] = (uint8_t)(cur[i] + up[i]); break;
            case 3:
                for (int i = 0; i < stride; ++i) {
                    const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0;
                    cur[i] = (uint8_t)(cur[i] + ((a + b) >> 1));
                }
                break;
            case 4:
                for (int i = 0; i < stride; ++i) {
                    const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
                    const int pp = a + b - c, pa = std::abs(pp - a), pb = std::abs(pp - b), pc = std::abs(pp - c);
                    cur[i] = (uint8_t)(cur[i] + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c)));
                }
                break;
            default: return fail(GS360_ERR_ARG, "PNG row %d has unknown filter type %d", y, ft);
        }
    }
    return GS360_OK;
}

// TIFF LZW strip decoder (compression 5: MSB-first codes of 9..12 bits, ClearCode 256, EndOfInformation 257, "early change").
// Host helper like gs360_png_unfilter: 16-bit TIFF panoramas are commonly LZW-compressed and the Python-side codec cannot loop
// over codes at image scale.  Writes at most out_cap bytes; *out_len receives the number produced.
int gs360_tiff_lzw_decode(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!in || !out || !out_len) return fail(GS360_ERR_ARG, "NULL argument");
    struct Entry { uint32_t pos, len; };                 // every string is a slice of the output written so far
    std::vector<Entry> tab(4096);
    size_t op = 0, bitpos = 0;
    int next = 258, width = 9;
    int64_t prev = -1;
    const size_t nbits = in_len * 8;
    auto emit = [&](const uint8_t* srcp, uint32_t len) -> bool {
        if (op + len > out_cap) len = (uint32_t)(out_cap - op);
        for (uint32_t i = 0; i < len; ++i) out[op + i] = srcp[i];      // may overlap forwards: byte copy
        op += len;
        return op < out_cap;
    };
    while (bitpos + width <= nbits) {
        uint32_t code = 0;
        for (int b = 0; b < width; ++b) {
            const size_t bp = bitpos + b;
            code = (code << 1) | ((in[bp >> 3] >> (7 - (bp & 7))) & 1u);
        }
        bitpos += width;
        if (code == 257) break;
        if (code == 256) { next = 258; width = 9; prev = -1; continue; }
        const uint32_t start = (uint32_t)op;
        if (prev < 0) {                                   // first code after a clear: a literal
            if (code > 255) return fail(GS360_ERR_ARG, "corrupt LZW stream (code %u after clear)", code);
            const uint8_t lit = (uint8_t)code;
            tab[code] = Entry{start, 1};
            if (!emit(&lit, 1)) break;
            prev = code;
            continue;
        }
        const Entry pe = prev < 256 ? Entry{0, 1} : tab[prev];
        uint8_t plit = (uint8_t)prev;
        const uint8_t* pstr = prev < 256 ? &plit : out + pe.pos;
        bool more;
        if (code < 256) {
            const uint8_t lit = (uint8_t)code;
            more = emit(&lit, 1);
        } else if ((int)code < next) {
            const Entry e = tab[code];
            more = emit(out + e.pos, e.len);
        } else if ((int)code == next) {                  // KwKwK: previous string + its own first byte
            const uint32_t plen = prev < 256 ? 1u : pe.len;
            const uint8_t first = pstr[0];
            more = emit(pstr, plen);
            if (more) more = emit(&first, 1);
        } else {
            return fail(GS360_ERR_ARG, "corrupt LZW stream (code %u, table size %d)", code, next);
        }
        if (next < 4096) {                                // new entry = previous string + first byte of this one; it is
            const uint32_t plen = prev < 256 ? 1u : pe.len;   // exactly the bytes [start - plen, start + 1) of the output
            tab[next] = Entry{start - plen, plen + 1};
            ++next;
            if (next + 1 >= (1 << width) && width < 12) ++width;       // early change
        }
        prev = code;
        if (!more) break;
    }
    *out_len = op;
    return GS360_OK;
}
