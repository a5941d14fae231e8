// gs360_capi_codec.hip -- image-codec entry points of libgs360hip.so (include/gs360.h): PNG scanline unfiltering and TIFF LZW strip
// decoding for the Python-side codec (gs360/imageio.py; host only, no GPU involved), and the glue of the device JPEG scans
// (gs360_jpeg.hip), of the device JPEG decoder (gs360_jpegdec.hip) and of the device PNG encoder (gs360_png.hip).
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

// ---- baseline JPEG scans on the device (JPG-SPEC v1; kernels in gs360_jpeg.hip) ------------------------------------------
namespace {

// the sides every codec here takes; what: "JPEG sides are" or "the PNG encoder's sides are"
int check_sides(const char* what, int H, int W) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return fail(GS360_ERR_ARG, "%s 1..65535 (got %d x %d)", what, W, H);
    return 0;
}

// what an encoder's call and each of its jobs have in common (gs360_jpeg_job and gs360_png_job name these fields alike)
int check_encoder_call(gs360_ctx* c, const void* jobs, int n_jobs, bool outputs, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_jobs < 0) return fail(GS360_ERR_ARG, "n_jobs < 0");
    if (n_jobs > 0 && (!jobs || !outputs)) return fail(GS360_ERR_ARG, "NULL argument");
    return 0;
}
template <class Job>
int check_encoder_job(const Job& j, int k, size_t row_bytes) {
    if (!j.src || !j.out) return fail(GS360_ERR_ARG, "job %d: NULL image or output", k);
    if (j.src_stride && j.src_stride < row_bytes) return fail(GS360_ERR_ARG, "job %d: src_stride below a row", k);
    return 0;
}

// the sides and components either codec ("encoder", "decoder") takes
int check_jpeg_image(const char* codec, int H, int W, int C) {
    if (int rc = check_sides("JPEG sides are", H, W)) return rc;
    if (C != 1 && C != 3) return fail(GS360_ERR_UNSUPPORTED, "the JPEG %s takes C = 1 or 3 (got %d)", codec, C);
    return 0;
}

int check_jpeg_geometry(int H, int W, int C, int restart_interval) {
    if (int rc = check_jpeg_image("encoder", H, W, C)) return rc;
    if (restart_interval < 1 || restart_interval > 65535) return fail(GS360_ERR_ARG, "restart interval %d outside 1..65535", restart_interval);
    return 0;
}

int check_jpeg_subsampling(int subsampling) {
    if (subsampling != GS360_JPEG_444 && subsampling != GS360_JPEG_420)
        return fail(GS360_ERR_ARG, "JPEG subsampling %d is neither GS360_JPEG_444 nor GS360_JPEG_420", subsampling);
    return 0;
}

}  // namespace

int gs360_jpeg_scan_bound(int H, int W, int C, int restart_interval, size_t* bytes) {
    return gs360_jpeg_scan_bound_sub(H, W, C, restart_interval, GS360_JPEG_444, bytes);
}

int gs360_jpeg_scan_bound_sub(int H, int W, int C, int restart_interval, int subsampling, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_jpeg_geometry(H, W, C, restart_interval)) return rc;
    if (int rc = check_jpeg_subsampling(subsampling)) return rc;
    // a block's 64 coefficients cost at most 26 bits each (a 16-bit code and 10 value bits): 208 bytes, twice that when every byte is
    // stuffed; an interval adds at most its marker and one slack byte
    const JpGrid g = jpeg_grid(H, W, C, subsampling);
    const size_t mcus = (size_t)g.mcus();
    const size_t intervals = (mcus + restart_interval - 1) / restart_interval;
    *bytes = mcus * g.bpm * 416 + intervals * 3;
    return GS360_OK;
}

namespace {

// scratch of a launch batch: coefficients (at 0), the quantiser table, the intervals' lengths and offsets and, with optimal tables, the
// images' symbol counts and coder tables
constexpr size_t kJpTableWords = 2 * 272;
struct JpScratch { size_t quant, int_len, int_off, hist, total; };
JpScratch jpeg_scratch(int64_t blocks, int64_t intervals, int images, bool optimal) {
    Carve v;
    JpScratch a{};
    v.take((size_t)blocks * 128);
    a.quant = v.take(128 * sizeof(JpQuant), 256);
    a.int_len = v.take(round_up((size_t)intervals * 4, 256));
    a.int_off = v.take((size_t)intervals * 8);
    if (optimal) a.hist = v.take(2 * (size_t)images * kJpTableWords * sizeof(uint32_t), 256);
    a.total = v.at;
    return a;
}

// gs360_jpeg_scan_sub_u8; gs360_jpeg_scan_u8 (the Annex K tables) and gs360_jpeg_scan_opt_u8 (per-image optimal tables) with
// GS360_JPEG_444
int jpeg_scan(gs360_ctx* c, const gs360_jpeg_job* jobs, int n_jobs, int quality, int restart_interval, int subsampling,
              uint64_t* lengths_dev, uint8_t* tables_dev, bool optimal, int slot) {
    if (int rc = check_encoder_call(c, jobs, n_jobs, lengths_dev && (!optimal || tables_dev), slot)) return rc;
    if (n_jobs == 0) return GS360_OK;
    if (quality < 1 || quality > 100) return fail(GS360_ERR_ARG, "quality %d outside 1..100", quality);
    if (int rc = check_jpeg_subsampling(subsampling)) return rc;
    std::vector<JpGrid> grid(n_jobs);            // each job's MCU grid: checked here, then read by the sizing and the fill
    for (int k = 0; k < n_jobs; ++k) {
        const gs360_jpeg_job& j = jobs[k];
        if (int rc = check_jpeg_geometry(j.H, j.W, j.C, restart_interval)) return rc;
        if (int rc = check_encoder_job(j, k, (size_t)j.W * j.C)) return rc;
        // the table construction's range: counts in uint32 below libjpeg's 10^9 sentinel, code lengths below 64 before limiting
        const JpGrid& g = grid[k] = jpeg_grid(j.H, j.W, j.C, subsampling);
        if (optimal && g.mcus() * g.bpm * 64 >= 1000000000ll)
            return fail(GS360_ERR_UNSUPPORTED, "job %d: optimal Huffman tables take images below 10^9 coefficients", k);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    Staging& st = c->stage[slot];
    // the scratch is sized for the call's largest batch before the first launch (growing it later would free memory that queued
    // kernels still use)
    size_t need = 0;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        int64_t blocks = 0, intervals = 0;
        for (int k = k0; k < std::min(n_jobs, k0 + GS360_MAX_VIEWS); ++k) {
            const int64_t mcus = grid[k].mcus();
            blocks += mcus * grid[k].bpm;
            intervals += (mcus + restart_interval - 1) / restart_interval;
        }
        need = std::max(need, jpeg_scratch(blocks, intervals, std::min(GS360_MAX_VIEWS, n_jobs - k0), optimal).total);
    }
    if (int rc = ensure(&st.d_jpeg, &st.jpeg_cap, need)) return rc;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        JpLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.n_jobs = std::min(GS360_MAX_VIEWS, n_jobs - k0);
        L.quality = quality;
        L.ri = restart_interval;
        int64_t blocks = 0, tiles = 0, intervals = 0;
        for (int k = 0; k < L.n_jobs; ++k) {
            const gs360_jpeg_job& j = jobs[k0 + k];
            JpJob& J = L.job[k];
            J.src = (const uint8_t*)j.src;
            J.out = (uint8_t*)j.out;
            J.cap = j.out_capacity;
            J.stride = (int64_t)(j.src_stride ? j.src_stride : (size_t)j.W * j.C);
            J.H = j.H; J.W = j.W; J.C = j.C;
            const JpGrid& g = grid[k0 + k];
            J.bw = g.mw;
            J.bpm = g.bpm;
            J.n_mcu = g.mw * g.mh;
            J.n_int = (J.n_mcu + restart_interval - 1) / restart_interval;
            J.tiles_x = (g.mw * g.mcu_w + 255) / 256;                             // strips of 256 columns, one MCU row high
            J.coef_base = blocks; J.tile_base = (int32_t)tiles; J.int_base = (int32_t)intervals;
            blocks += (int64_t)J.n_mcu * g.bpm;
            tiles += (int64_t)J.tiles_x * g.mh;
            intervals += J.n_int;
            if (g.bpm == 6) L.any420 = 1;
        }
        if (tiles > INT32_MAX || intervals > INT32_MAX) return fail(GS360_ERR_ARG, "JPEG batch too large");
        L.total_tiles = (int32_t)tiles;
        L.total_int = (int32_t)intervals;
        const JpScratch at = jpeg_scratch(blocks, intervals, L.n_jobs, optimal);
        if (at.total > st.jpeg_cap) return fail(GS360_ERR_ARG, "JPEG scratch layout");
        uint8_t* base = (uint8_t*)st.d_jpeg;
        L.coef = (int16_t*)base;
        L.quant = (JpQuant*)(base + at.quant);
        L.int_len = (uint32_t*)(base + at.int_len);
        L.int_off = (uint64_t*)(base + at.int_off);
        L.lengths = lengths_dev + k0;
        if (optimal) {
            L.hist = (uint32_t*)(base + at.hist);
            L.huff = L.hist + (size_t)L.n_jobs * kJpTableWords;
            L.tables = tables_dev + (size_t)k0 * 4 * GS360_JPEG_TABLE_BYTES;
            L.count_waves = opt(c, kOptJpegCountWaves);
        }
        HIP_TRY(launch_jpeg_scan(L, s));
    }
    return GS360_OK;
}

}  // namespace

int gs360_jpeg_scan_u8(gs360_ctx* c, const gs360_jpeg_job* jobs, int n_jobs, int quality, int restart_interval,
                       uint64_t* lengths_dev, int slot) {
    return jpeg_scan(c, jobs, n_jobs, quality, restart_interval, GS360_JPEG_444, lengths_dev, nullptr, false, slot);
}

int gs360_jpeg_scan_opt_u8(gs360_ctx* c, const gs360_jpeg_job* jobs, int n_jobs, int quality, int restart_interval,
                           uint64_t* lengths_dev, uint8_t* tables_dev, int slot) {
    return jpeg_scan(c, jobs, n_jobs, quality, restart_interval, GS360_JPEG_444, lengths_dev, tables_dev, true, slot);
}

int gs360_jpeg_scan_sub_u8(gs360_ctx* c, const gs360_jpeg_job* jobs, int n_jobs, int quality, int restart_interval, int subsampling,
                           uint64_t* lengths_dev, uint8_t* tables_dev, int slot) {
    return jpeg_scan(c, jobs, n_jobs, quality, restart_interval, subsampling, lengths_dev, tables_dev, tables_dev != nullptr, slot);
}

int gs360_jpeg_huff_tables(gs360_ctx* c, const uint32_t* hist_dev, int n_tables, uint8_t* tables_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_tables < 0) return fail(GS360_ERR_ARG, "n_tables < 0");
    if (n_tables == 0) return GS360_OK;
    if (!hist_dev || !tables_dev) return fail(GS360_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_jpeg_huff_tables(hist_dev, n_tables, tables_dev, c->stream[slot]));
    return GS360_OK;
}

// ---- baseline JPEG files decoded on the device (JPD-SPEC v1; kernels in gs360_jpegdec.hip) --------------------------------
namespace {

int check_jpeg_dec_geometry(int H, int W, int C, int subsampling) {
    if (int rc = check_jpeg_image("decoder", H, W, C)) return rc;
    if (subsampling != GS360_JPEG_444 && subsampling != GS360_JPEG_422 && subsampling != GS360_JPEG_420 &&
        subsampling != GS360_JPEG_440 && subsampling != GS360_JPEG_411)
        return fail(GS360_ERR_UNSUPPORTED, "the JPEG decoder takes GS360_JPEG_444, _422, _420, _440 or _411 (got %d)", subsampling);
    return 0;
}

}  // namespace

int gs360_jpeg_decode_scratch(int H, int W, int C, int subsampling, uint32_t n_subseq, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_jpeg_dec_geometry(H, W, C, subsampling)) return rc;
    if (n_subseq < 1 || n_subseq > (1u << 31) / kJdSubseq) return fail(GS360_ERR_ARG, "n_subseq %u outside 1..2^24", n_subseq);
    *bytes = jd_layout(H, W, C, subsampling, n_subseq).total;
    return GS360_OK;
}

namespace {

// gs360_jpeg_decode_u8 (gray false: H x W x C out) and gs360_jpeg_decode_gray_u8 (gray true: an H x W plane)
int jpeg_decode(gs360_ctx* c, const gs360_jpeg_dec_job* jobs, int n_jobs, uint32_t* status_dev, bool gray, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_jobs < 0) return fail(GS360_ERR_ARG, "n_jobs < 0");
    if (n_jobs == 0) return GS360_OK;
    if (!jobs || !status_dev) return fail(GS360_ERR_ARG, "NULL argument");
    for (int k = 0; k < n_jobs; ++k) {
        const gs360_jpeg_dec_job& j = jobs[k];
        if (int rc = check_jpeg_dec_geometry(j.H, j.W, j.C, j.subsampling)) return rc;
        if (!j.scan || !j.segments || !j.tables || !j.scratch || !j.out) return fail(GS360_ERR_ARG, "job %d: NULL pointer", k);
        if (j.scan_len < 1 || j.scan_len > (uint32_t)INT32_MAX) return fail(GS360_ERR_ARG, "job %d: scan of %u bytes outside 1..2^31-1", k, j.scan_len);
        if (j.n_segments < 1 || (uint32_t)j.n_segments > j.scan_len) return fail(GS360_ERR_ARG, "job %d: %d segments for %u bytes", k, j.n_segments, j.scan_len);
        if (j.restart_interval < 0 || j.restart_interval > 65535) return fail(GS360_ERR_ARG, "job %d: restart interval %d outside 0..65535", k, j.restart_interval);
        if (j.out_stride && j.out_stride < (size_t)j.W * (gray ? 1 : j.C)) return fail(GS360_ERR_ARG, "job %d: out_stride below a row", k);
        if ((uintptr_t)j.scratch % 256) return fail(GS360_ERR_ARG, "job %d: scratch is not 256-byte aligned", k);
        if ((uintptr_t)j.segments % 16) return fail(GS360_ERR_ARG, "job %d: segments is not 16-byte aligned", k);
        for (int q = 0; q < j.C; ++q)
            if (j.comp_tq[q] > 3 || j.comp_td[q] > 1 || j.comp_ta[q] > 1) return fail(GS360_ERR_UNSUPPORTED, "job %d: table selector outside baseline", k);
        // every interval takes at least one subsequence and none crosses an interval
        if (j.n_subseq < 1 || j.n_subseq > (uint64_t)j.scan_len / kJdSubseq + (uint32_t)j.n_segments)
            return fail(GS360_ERR_ARG, "job %d: %u subsequences for %u bytes in %d segments", k, j.n_subseq, j.scan_len, j.n_segments);
        if (jd_layout(j.H, j.W, j.C, j.subsampling, j.n_subseq).total > j.scratch_bytes)
            return fail(GS360_ERR_ARG, "job %d: scratch too small", k);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        JdLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.n_jobs = std::min(GS360_MAX_VIEWS, n_jobs - k0);
        L.status = status_dev + k0;
        int64_t wgs = 0, tiles = 0;
        for (int k = 0; k < L.n_jobs; ++k) {
            const gs360_jpeg_dec_job& j = jobs[k0 + k];
            JdJob& J = L.job[k];
            jd_fill_job(J, j, gray);
            J.wg_base = (int32_t)wgs;
            J.tile_base = (int32_t)tiles;
            wgs += J.lay.n_wg;
            tiles += (int64_t)J.tiles_x * ((j.H + 63) / 64);
            L.max_dc_chunks = std::max(L.max_dc_chunks, J.lay.dc_chunks);
        }
        if (wgs > INT32_MAX || tiles > INT32_MAX) return fail(GS360_ERR_ARG, "JPEG batch too large");
        L.total_wg = (int32_t)wgs;
        L.total_tiles = (int32_t)tiles;
        HIP_TRY(launch_jpeg_decode(L, gray, s));
    }
    return GS360_OK;
}

}  // namespace

int gs360_jpeg_decode_u8(gs360_ctx* c, const gs360_jpeg_dec_job* jobs, int n_jobs, uint32_t* status_dev, int slot) {
    return jpeg_decode(c, jobs, n_jobs, status_dev, false, slot);
}

int gs360_jpeg_decode_gray_u8(gs360_ctx* c, const gs360_jpeg_dec_job* jobs, int n_jobs, uint32_t* status_dev, int slot) {
    return jpeg_decode(c, jobs, n_jobs, status_dev, true, slot);
}

// ---- PNG deflate streams on the device (PNG-SPEC v1; kernels in gs360_png.hip) --------------------------------------------
namespace {

int check_png_geometry(int H, int W, int C, int bytes_per_sample) {
    if (int rc = check_sides("the PNG encoder's sides are", H, W)) return rc;
    if (C != 1 && C != 3 && C != 4) return fail(GS360_ERR_UNSUPPORTED, "the PNG encoder takes C = 1, 3 or 4 (got %d)", C);
    if (bytes_per_sample != 1 && bytes_per_sample != 2)
        return fail(GS360_ERR_UNSUPPORTED, "the PNG encoder takes 1 or 2 bytes per sample (got %d)", bytes_per_sample);
    return 0;
}

inline size_t png_filtered(int H, int W, int C, int bps) { return (size_t)H * (1 + (size_t)W * C * bps); }
inline size_t png_chunks(size_t n) { return (n + kPnChunk - 1) / kPnChunk; }

// scratch of a launch batch: the filtered streams (at 0; filt: their bytes, each image's rounded up), then per chunk its length,
// offset, code tables and segment offsets
struct PnScratch { size_t chunk_len, chunk_off, codes, seg_off, total; };
PnScratch png_scratch(size_t filt, size_t chunks) {
    Carve v;
    PnScratch a{};
    v.take(filt + 4);
    a.chunk_len = v.take(chunks * 4, 256);
    a.chunk_off = v.take(chunks * 8, 256);
    a.codes = v.take(chunks * 320 * 4);
    a.seg_off = v.take(chunks * kPnThreads * 4);
    a.total = v.at;
    return a;
}

}  // namespace

int gs360_png_bound(int H, int W, int C, int bytes_per_sample, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_png_geometry(H, W, C, bytes_per_sample)) return rc;
    // a literal costs at most 15 bits, a match of three or more bytes at most 15 + 5 + 15 + 13: two bytes per filtered byte; a chunk
    // adds its header (168 bytes), the end of block and the stored block (7 bytes)
    const size_t n = png_filtered(H, W, C, bytes_per_sample);
    *bytes = 2 * n + png_chunks(n) * 176;
    return GS360_OK;
}

int gs360_png_deflate(gs360_ctx* c, const gs360_png_job* jobs, int n_jobs, uint64_t* lengths_dev, uint32_t* adler_dev, int slot) {
    if (int rc = check_encoder_call(c, jobs, n_jobs, lengths_dev && adler_dev, slot)) return rc;
    if (n_jobs == 0) return GS360_OK;
    for (int k = 0; k < n_jobs; ++k) {
        const gs360_png_job& j = jobs[k];
        if (int rc = check_png_geometry(j.H, j.W, j.C, j.bytes_per_sample)) return rc;
        if (int rc = check_encoder_job(j, k, (size_t)j.W * j.C * j.bytes_per_sample)) return rc;
        if (j.bytes_per_sample == 2 && (((uintptr_t)j.src | j.src_stride) & 1)) return fail(GS360_ERR_ARG, "job %d: 16-bit rows are not 2-byte aligned", k);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    Staging& st = c->stage[slot];
    // the scratch is sized for the call's largest batch before the first launch
    size_t need = 0;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        size_t filt = 0, chunks = 0;
        for (int k = k0; k < std::min(n_jobs, k0 + GS360_MAX_VIEWS); ++k) {
            const size_t n = png_filtered(jobs[k].H, jobs[k].W, jobs[k].C, jobs[k].bytes_per_sample);
            filt += round_up(n + 4, 256);
            chunks += png_chunks(n);
        }
        need = std::max(need, png_scratch(filt, chunks).total);
    }
    if (int rc = ensure(&st.d_png, &st.png_cap, need)) return rc;
    size_t chunks_before = 0;                             // adler_dev: two words per chunk, the jobs' chunks in job order
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        PnLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.n_jobs = std::min(GS360_MAX_VIEWS, n_jobs - k0);
        size_t filt = 0;
        int64_t rows = 0, chunks = 0;
        for (int k = 0; k < L.n_jobs; ++k) {
            const gs360_png_job& j = jobs[k0 + k];
            PnJob& J = L.job[k];
            J.src = (const uint8_t*)j.src;
            J.out = (uint8_t*)j.out;
            J.cap = j.out_capacity;
            J.bpp = j.C * j.bytes_per_sample;
            J.Wb = j.W * J.bpp;
            J.stride = (int64_t)(j.src_stride ? j.src_stride : (size_t)J.Wb);
            J.H = j.H;
            J.swap = j.bytes_per_sample == 2;
            J.n = (int64_t)png_filtered(j.H, j.W, j.C, j.bytes_per_sample);
            J.filt_base = (int64_t)filt;
            J.row_base = (int32_t)rows; J.chunk_base = (int32_t)chunks;
            J.n_chunks = (int32_t)png_chunks((size_t)J.n);
            const int cand[3] = {1, J.bpp, 1 + J.Wb};
            for (int q = 0; q < 3; ++q) {
                const int d = cand[q];
                if (d > 32768 || (q > 0 && d == cand[q - 1])) continue;            // (bpp = 1 repeats the first: the earlier one wins every tie)
                J.dist[q] = d;
                const uint32_t x = (uint32_t)d - 1;                                // RFC 1951 3.2.5
                const int e = x < 4 ? 0 : 30 - __builtin_clz(x);                   // floor(log2(x)) - 1
                J.dsym[q] = (uint8_t)(x < 4 ? x : 2 * e + 2 + ((x >> e) & 1));
                J.dbits[q] = (uint8_t)e;
                J.dval[q] = (uint16_t)(x & ((1u << e) - 1));
            }
            filt += round_up((size_t)J.n + 4, 256);
            rows += j.H;
            chunks += J.n_chunks;
        }
        if (rows > INT32_MAX || chunks > INT32_MAX) return fail(GS360_ERR_ARG, "PNG batch too large");
        L.total_rows = (int32_t)rows;
        L.total_chunks = (int32_t)chunks;
        const PnScratch at = png_scratch(filt, (size_t)chunks);
        if (at.total > st.png_cap) return fail(GS360_ERR_ARG, "PNG scratch layout");
        uint8_t* base = (uint8_t*)st.d_png;
        L.filt = base;
        L.chunk_len = (uint32_t*)(base + at.chunk_len);
        L.chunk_off = (uint64_t*)(base + at.chunk_off);
        L.codes = (uint32_t*)(base + at.codes);
        L.seg_off = (uint32_t*)(base + at.seg_off);
        L.lengths = lengths_dev + k0;
        L.adler = adler_dev + 2 * chunks_before;
        chunks_before += (size_t)chunks;
        HIP_TRY(launch_png_deflate(L, s));
    }
    return GS360_OK;
}
