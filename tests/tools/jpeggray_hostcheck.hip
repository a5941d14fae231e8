// jpeggray_hostcheck.hip -- the device JPEG decoder's gray output mode (gs360_jpeg_decode_gray_u8, csrc/gs360_jpegdec.hip) stepped lane
// by lane on the host.  The stepping of the entropy stages and of the DC sums is that of jpegdec_hostcheck.hip (see there); what
// differs is the last stage and its output: the job is filled as the gray entry point fills it, the pixels step runs in gray mode, and
// the output plane is allocated at exactly H x stride bytes (stride = W + row padding), so that a build with
// -fsanitize=address,undefined (tests/test_jpeggray_hostcheck.py) turns three bytes per pixel, or an x * C address into the one-byte
// plane, into a failure.  Usage and the input file: as jpegdec_hostcheck; OUT = the H x stride plane.
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_jpegdec.hip"
#include <cstdio>
#include <vector>
#include <cstring>
using namespace gs360;
int main(int argc, char** argv) {
    FILE* f = argc >= 3 ? fopen(argv[1], "rb") : nullptr;
    int32_t hd[16];
    if (!f || fread(hd, 4, 16, f) != 16) return 2;
    int H = hd[0], W = hd[1], C = hd[2], sub = hd[3], ri = hd[4], scan_len = hd[5], n_seg = hd[6], n_sub = hd[7], pad = hd[11];
    std::vector<uint8_t> scan(scan_len), meta(4 * 272 + 256);
    std::vector<uint32_t> seg(n_seg * 4);
    uint8_t sel[12];
    if (fread(sel, 1, 12, f) != 12 || fread(scan.data(), 1, scan_len, f) != (size_t)scan_len ||
        fread(seg.data(), 4, n_seg * 4, f) != (size_t)n_seg * 4 || fread(meta.data(), 1, meta.size(), f) != meta.size()) return 2;
    fclose(f);
    JdLayout l = jd_layout(H, W, C, sub, n_sub);
    std::vector<uint8_t> scratch(l.total);   // exact size: the sanitizer guards its end
    size_t stride = (size_t)W + pad;          // one byte per pixel, whatever C is
    std::vector<uint8_t> out(stride * H, 0xA5);
    gs360_jpeg_dec_job job = {};
    job.scan = scan.data(); job.scan_len = scan_len; job.n_subseq = n_sub; job.segments = seg.data(); job.n_segments = n_seg;
    job.tables = meta.data(); job.H = H; job.W = W; job.C = C; job.subsampling = sub; job.restart_interval = ri;
    memcpy(job.comp_tq, sel, 4); memcpy(job.comp_td, sel + 4, 4); memcpy(job.comp_ta, sel + 8, 4);
    job.scratch = scratch.data(); job.scratch_bytes = scratch.size(); job.out = out.data(); job.out_stride = stride;
    JdJob J;
    memset(&J, 0, sizeof(J));
    jd_fill_job(J, job, true);               // the set-up of gs360_jpeg_decode_gray_u8
    if (J.lay.total != l.total || J.lay.blocks != (int64_t)J.mw * J.mh * J.bpm) return 3;
    memset(scratch.data() + l.coef, 0, l.blocks * 128);
    memset(scratch.data() + l.dc, 0, l.blocks * 4);
    JdTables* T = new JdTables;
    for (int t = 0; t < 256; ++t) jd_tables_first(J.meta, *T, t, 256);
    for (int t = 0; t < 256; ++t) jd_tables_second(*T, t, 256);
    uint32_t* exits = (uint32_t*)(J.scratch + J.lay.exits);
    uint32_t* sums = (uint32_t*)(J.scratch + J.lay.sums);
    uint32_t* used = (uint32_t*)(J.scratch + J.lay.used);
    JdHeader* hdr = (JdHeader*)J.scratch;
    int max_rounds_wg = 0;
    // jd_sync_kernel
    for (int wg = 0; wg < J.lay.n_wg; ++wg) {
        uint32_t sh[256] = {}, cur[256] = {};
        bool active[256];
        JdSegment S[256];
        for (int t = 0; t < 256; ++t) {
            uint32_t j = wg * 256 + t;
            active[t] = j < J.n_sub;
            if (active[t]) {
                S[t] = jd_find_segment(J, j);
                cur[t] = jd_decode<false>(*T, J, S[t], j - S[t].first_sub, jd_cold(S[t].bytes, S[t].len, j - S[t].first_sub), nullptr, nullptr, 0, nullptr);
            }
            sh[t] = cur[t];
        }
        for (int r = 1; r < 256; ++r) {
            bool any = false;
            uint32_t nsh[256];
            memcpy(nsh, sh, sizeof(sh));
            for (int t = 0; t < 256; ++t) {
                uint32_t j = wg * 256 + t;
                if (active[t]) {
                    uint32_t tt = t + r, jj = j + r;
                    if (tt >= 256 || jj >= S[t].end_sub) active[t] = false;
                    else {
                        uint32_t x = jd_decode<false>(*T, J, S[t], jj - S[t].first_sub, cur[t] & kStateMask, nullptr, nullptr, 0, nullptr);
                        uint32_t old = sh[tt];
                        nsh[tt] = x;
                        if ((x & kStateMask) == (old & kStateMask)) active[t] = false;
                        cur[t] = x;
                    }
                }
                any |= active[t];
            }
            memcpy(sh, nsh, sizeof(sh));
            if (r > max_rounds_wg) max_rounds_wg = r;
            if (!any) break;
        }
        for (int t = 0; t < 256; ++t) if ((uint32_t)(wg * 256 + t) < J.n_sub) exits[wg * 256 + t] = sh[t];
    }
    // jd_chain_kernel
    for (int w = 1; w < J.lay.n_wg; ++w) { uint32_t j0 = w * 256; JdSegment S = jd_find_segment(J, j0); used[w] = jd_cold(S.bytes, S.len, j0 - S.first_sub); }
    uint32_t rounds = 0;
    for (int r = 0; r < J.lay.n_wg; ++r) {
        int changed = 0;
        for (int w = 1; w < J.lay.n_wg; ++w) {
            uint32_t j0 = w * 256; JdSegment S = jd_find_segment(J, j0);
            if (j0 == S.first_sub) continue;
            uint32_t ent = exits[j0 - 1] & kStateMask;
            if (ent == used[w]) continue;
            used[w] = ent; changed = 1;
            uint32_t cur = ent, j1 = jd_min(jd_min(j0 + 256u, S.end_sub), J.n_sub);
            for (uint32_t j = j0; j < j1; ++j) {
                uint32_t x = jd_decode<false>(*T, J, S, j - S.first_sub, cur, nullptr, nullptr, 0, nullptr);
                uint32_t old = exits[j]; exits[j] = x;
                if ((x & kStateMask) == (old & kStateMask)) break;
                cur = x & kStateMask;
            }
        }
        ++rounds;
        if (!changed) break;
    }
    hdr->err = 0; hdr->ok = 0; hdr->rounds = rounds;
    uint32_t acc = 0;
    for (uint32_t j = 0; j < J.n_sub; ++j) { sums[j] = acc; acc += exits[j] >> 18; }
    // jd_write_kernel
    for (uint32_t j = 0; j < J.n_sub; ++j) {
        JdSegment S = jd_find_segment(J, j);
        uint32_t k = j - S.first_sub, state = k == 0 ? 0u : exits[j - 1] & kStateMask, done = sums[j] - sums[S.first_sub];
        if (done >= S.blk_end - S.blk0) continue;
        jd_decode<true>(*T, J, S, k, state, (int16_t*)(J.scratch + J.lay.coef), (int32_t*)(J.scratch + J.lay.dc), S.blk0 + done, hdr);
    }
    // DC (serial stand-in for the scan kernels)
    int32_t* dc = (int32_t*)(J.scratch + J.lay.dc);
    for (int comp = 0; comp < C; ++comp) {
        JdDcSeq Q = jd_dc_seq(J, comp);
        int run = 0;
        for (uint32_t q = 0; q < Q.n; ++q) {
            uint32_t m = q / Q.per_mcu, sb = q % Q.per_mcu, at = m * J.bpm + Q.off + sb;
            bool head = sb == 0 && (J.ri ? m % J.ri == 0 : m == 0);
            run = jd_carry_in(run, dc[at], head);
            dc[at] = run;
        }
    }
    // jd_pixels_kernel<true>
    JdTile* TL = new JdTile;
    for (int ty = 0; ty < (H + 63) / 64; ++ty)
        for (int tx = 0; tx < J.tiles_x; ++tx) {
            for (int t = 0; t < 256; ++t) jd_tile_quant(J, *TL, t);
            for (int t = 0; t < 256; ++t) jd_tile_blocks(J, *TL, tx, ty, t);
            for (int t = 0; t < 256; ++t) jd_tile_pixels<true>(J, *TL, tx, ty, t);
        }
    uint32_t status = hdr->err ? 1u : (hdr->ok != J.n_seg ? 2u : 0u);
    delete T;
    delete TL;
    printf("status %u rounds %u wg_rounds %d n_sub %u n_wg %d sampling %dx%d bpm %d\n", status, rounds, max_rounds_wg, J.n_sub, J.lay.n_wg, J.hs, J.vs, J.bpm);
    f = fopen(argv[2], "wb"); fwrite(out.data(), 1, out.size(), f); fclose(f);
    return 0;
}
