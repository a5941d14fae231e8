// gs360_jpegdec.hip -- baseline JPEG files decoded on the device (JPD-SPEC v1).
//
// Entropy stage.  The scan is cut at its restart markers into segments (the host finds them) and every segment into subsequences of
// kJdSubseq bytes; one lane owns one subsequence.  A lane's decoder state is (bit position, block of the MCU cycle, zig-zag index).
// Only a segment's first subsequence knows its entry state; every other lane starts from "block 0, coefficient 0" at its first byte
// and Huffman codes make such a decoder fall into step with the true one after a few symbols (Weissenberger and Schmidt 2018,
// PAPERS.md).  Nothing is taken on trust, though: a lane's exit state is recorded per subsequence, lanes run on into the following
// subsequences until the state they arrive with is the one recorded there (jd_sync_kernel, within a workgroup), one workgroup per file
// then carries the exit of each workgroup's last subsequence into the next workgroup until no entry state changes any more
// (jd_chain_kernel), and that fixed point is the sequential decoder's state at every subsequence boundary, exactly.  The same kernel
// sums the blocks completed per subsequence, so the second decode pass (jd_write_kernel) knows every lane's first block and writes the
// coefficients.  DC differences are summed per component within each segment by a three-step segmented scan (jd_dc_kernel /
// jd_dc_carry_kernel, both over jd_seg_scan), and jd_pixels_kernel turns 64 x 128 pixel tiles of blocks into pixels: RGB (or Y) for
// gs360_jpeg_decode_u8, one byte of FS-SPEC's gray for gs360_jpeg_decode_gray_u8 (its template parameter).
//
// Every loop below is bounded by a launch-time size: symbols of a subsequence (each takes at least one bit), subsequences of a
// workgroup, workgroups of a file, segments (binary search), chunks of a scan.  No workgroup waits for another one.  Every byte
// fetch is checked against the segment's length (beyond it the reader sees 0xFF) and every coefficient write against the segment's
// last block, so a truncated, corrupt or over-long stream sets the file's status and touches nothing outside its buffers.
#include "gs360_kernels.h"

namespace gs360 {
namespace {

// state word: bits 0-7 bit offset past the subsequence's first byte, 8-10 block of the MCU cycle, 11-16 zig-zag index; 18-31 blocks completed
constexpr uint32_t kStateMask = 0x3FFFF;
constexpr int kFastBits = 9;

// The stages' arithmetic is written as plain functions of (job, lane, shared arrays), host-callable as well: the kernels below only
// add the lane numbers and the barriers, and a host program can step the same code lane by lane.
#define JD_HD __host__ __device__

JD_HD inline uint32_t jd_natural(uint32_t z) {             // zig-zag position -> natural (row-major) index
    constexpr uint8_t kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                      13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                                      45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return kNatural[z & 63];
}
template <class T> JD_HD inline T jd_min(T a, T b) { return a < b ? a : b; }
template <class T> JD_HD inline T jd_max(T a, T b) { return a > b ? a : b; }
JD_HD inline void jd_or(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
JD_HD inline void jd_add(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

struct JdHeader { uint32_t err, ok, rounds, pad; };

// decoding tables of a file's four Huffman tables (index: 2 * id + class, i.e. DC0, AC0, DC1, AC1), built in LDS per workgroup
struct JdTables {
    uint16_t fast[4][1 << kFastBits];    // (length << 8) | symbol for codes of at most kFastBits bits, else 0
    uint32_t limit[4][17];               // [l]: the codes of length <= l, left-aligned in 16 bits, lie below this
    uint16_t first[4][17], valptr[4][17];
    uint8_t bits[4][17];
    uint8_t huffval[4][256];
};

JD_HD inline void jd_tables_first(const uint8_t* meta, JdTables& T, int tid, int nt) {
    for (int k = tid; k < 4 * 256; k += nt) T.huffval[k >> 8][k & 255] = meta[(k >> 8) * GS360_JPEG_TABLE_BYTES + 16 + (k & 255)];
    for (int k = tid; k < 4 << kFastBits; k += nt) T.fast[k >> kFastBits][k & ((1 << kFastBits) - 1)] = 0;
    if (tid < 4) {
        uint32_t code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            const uint32_t n = meta[tid * GS360_JPEG_TABLE_BYTES + l - 1];
            T.bits[tid][l] = (uint8_t)n;
            T.first[tid][l] = (uint16_t)code;
            T.valptr[tid][l] = (uint16_t)k;
            code += n;
            k += n;
            T.limit[tid][l] = jd_min(code << (16 - l), 65536u);
            code <<= 1;
        }
    }
}
JD_HD inline void jd_tables_second(JdTables& T, int tid, int nt) {
    for (int t = 0; t < 4; ++t) {
        for (int k = tid; k < 256; k += nt) {
            int len = 0;
            for (int l = 1; l <= kFastBits; ++l)
                if (k >= T.valptr[t][l] && k < T.valptr[t][l] + T.bits[t][l]) len = l;
            if (!len) continue;
            const uint32_t code = T.first[t][len] + (k - T.valptr[t][len]);
            const uint32_t lo = code << (kFastBits - len), n = 1u << (kFastBits - len);
            if (lo + n > (1u << kFastBits)) continue;
            const uint16_t e = (uint16_t)((len << 8) | T.huffval[t][k]);
            for (uint32_t f = 0; f < n; ++f) T.fast[t][lo + f] = e;
        }
    }
}
__device__ void jd_build_tables(const uint8_t* meta, JdTables& T) {
    jd_tables_first(meta, T, threadIdx.x, blockDim.x);
    __syncthreads();
    jd_tables_second(T, threadIdx.x, blockDim.x);
    __syncthreads();
}

// Bit reader over one segment.  `i` is the raw index of the byte that holds the next unread bit and `b` the bits of it already read,
// so (i, b) is a position in the file's own bytes; an 0xFF takes the byte behind it along (the stuffed 0x00).  Bytes past the
// segment's end read as 0xFF.
struct JdReader {
    const uint8_t* p;
    uint32_t len, i, ld;
    uint64_t buf, ffq;
    int cnt, b;
    uint32_t bad;

    JD_HD void init(const uint8_t* seg, uint32_t seg_len, uint32_t at, int bit) {
        p = seg; len = seg_len; i = at; ld = at; buf = 0; ffq = 0; cnt = 0; b = 0; bad = 0;
        refill();
        buf <<= bit; cnt -= bit; b = bit;
    }
    JD_HD void refill() {
        for (int k = 0; k < 8 && cnt <= 56; ++k) {
            const uint32_t v = ld < len ? p[ld] : 0xFFu;
            const uint32_t ff = v == 0xFF;
            if (ff && ld + 1 < len && p[ld + 1] != 0) bad = 1;
            ld += 1 + ff;
            ffq = (ffq << 1) | ff;
            buf |= (uint64_t)v << (56 - cnt);
            cnt += 8;
        }
    }
    JD_HD uint32_t step_of_current() const { return 1 + (uint32_t)((ffq >> (((b + cnt) >> 3) - 1)) & 1); }
    JD_HD void skip(int n) {
        buf <<= n; cnt -= n; b += n;
        for (int k = 0; k < 5 && b >= 8; ++k) {
            i += step_of_current();
            b -= 8;
        }
    }
    JD_HD uint32_t take(int n) {      // 1 <= n <= 16
        const uint32_t v = (uint32_t)(buf >> (64 - n));
        skip(n);
        return v;
    }
};

JD_HD inline int jd_extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

JD_HD inline uint32_t jd_cold(const uint8_t* seg, uint32_t len, uint32_t k) {      // entry state of a speculative start at subsequence k
    return (k > 0 && (uint64_t)k * kJdSubseq <= len && seg[k * kJdSubseq - 1] == 0xFF) ? 8u : 0u;   // (on the stuffed 0x00 of a pair: skip it)
}

struct JdSegment { const uint8_t* bytes; uint32_t len, first_sub, end_sub, blk0, blk_end; };

JD_HD inline JdSegment jd_find_segment(const JdJob& J, uint32_t j) {         // the segment subsequence j lies in
    uint32_t lo = 0, hi = J.n_seg;                                         // last segment whose first subsequence is <= j
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        if (J.seg[mid].z <= j) lo = mid; else hi = mid;
    }
    const uint4 s = J.seg[lo];
    JdSegment S;                                                           // (clamped: a segment table that lies reads no byte outside the scan)
    const uint32_t start = jd_min(s.x, J.scan_len);
    S.bytes = J.scan + start;
    S.first_sub = jd_min(s.z, j);
    S.len = jd_min(jd_min(s.y, J.scan_len - start), (uint32_t)INT32_MAX);
    if ((uint64_t)(j - S.first_sub) * kJdSubseq >= S.len) S.len = 0;       // (then nothing is fetched at all)
    S.end_sub = S.first_sub + (S.len + kJdSubseq - 1) / kJdSubseq;
    const uint32_t n_mcu = (uint32_t)J.mw * J.mh;
    const uint32_t m0 = jd_min(s.w, n_mcu), m1 = J.ri ? jd_min(m0 + (uint32_t)J.ri, n_mcu) : n_mcu;
    S.blk0 = m0 * J.bpm;
    S.blk_end = m1 * J.bpm;
    return S;
}

// Decodes subsequence k of a segment from `state` until the position passes the subsequence's last byte: -> the exit state with the
// number of blocks completed.  kWrite: `state` is the true one; coefficients of block `blk` on go to coef / dc, nothing at or past
// blk_end is written, and the header's counters record an invalid code and the segment's last block ending at its last byte.
template <bool kWrite>
JD_HD uint32_t jd_decode(const JdTables& T, const JdJob& J, const JdSegment& S, uint32_t k, uint32_t state, int16_t* coef, int32_t* dc,
                              uint32_t blk, JdHeader* hdr) {
    JdReader R;
    R.init(S.bytes, S.len, k * kJdSubseq + ((state & 255) >> 3), state & 7);
    uint32_t c = (state >> 8) & 7, z = (state >> 11) & 63, n = 0, err = 0;
    const uint32_t boundary = jd_min((k + 1) * kJdSubseq, S.len);
    const uint32_t bpm = J.bpm, n_luma = (uint32_t)(J.hs * J.vs);     // an MCU's cycle: n_luma Y blocks, then one block per further component
    for (int it = 0; it < kJdSubseq * 8 + 64; ++it) {      // every symbol takes at least one bit
        if (R.i >= boundary) break;
        if (kWrite && blk >= S.blk_end) break;
        R.refill();
        const uint32_t comp = c < n_luma ? 0 : c - n_luma + 1;
        const uint32_t t = z == 0 ? J.td[comp] * 2 : J.ta[comp] * 2 + 1;
        const uint32_t code = (uint32_t)(R.buf >> 48);
        uint32_t e = T.fast[t][code >> (16 - kFastBits)], len = e >> 8, sym = e & 255;
        if (!e) {
            len = 0;
            for (int l = kFastBits + 1; l <= 16; ++l)
                if (!len && code < T.limit[t][l]) len = l;
            if (len) {
                const uint32_t idx = T.valptr[t][len] + ((code >> (16 - len)) - T.first[t][len]);
                sym = T.huffval[t][idx & 255];
            }
        }
        if (!len) {
            if (R.i + 1 < S.len) err = 1;                  // (in the segment's last byte: the padding of 1-bits, the stream is over)
            R.i = S.len;
            break;
        }
        R.skip(len);
        const int s = z == 0 ? sym : sym & 15;
        if (z == 0) {
            if (s > 15) { err = 1; break; }
            const int v = s ? jd_extend(R.take(s), s) : 0;
            if (kWrite) dc[blk] = v;
            z = 1;
        } else if (s == 0) {
            z = (sym >> 4) == 15 ? z + 16 : 64;
        } else {
            z += sym >> 4;
            if (z > 63) { err = 1; break; }
            const int v = jd_extend(R.take(s), s);
            if (kWrite) coef[(size_t)blk * 64 + jd_natural(z)] = (int16_t)v;
            ++z;
        }
        if (z >= 64) {
            z = 0;
            c = c + 1 == bpm ? 0 : c + 1;
            ++n;
            ++blk;
            if (kWrite && blk == S.blk_end) {
                const uint32_t end = R.b > 0 ? R.i + R.step_of_current() : R.i;
                if (end == S.len) jd_add(&hdr->ok, 1u);
            }
        }
    }
    err |= R.bad;
    if (err) {          // a speculative decoder starts afresh at the next subsequence; the true one (kWrite) has found a corrupt stream
        if (kWrite) jd_or(&hdr->err, 1u);
        return n << 18;
    }
    const uint32_t next = (k + 1) * kJdSubseq;
    const uint32_t rel = R.i >= next ? jd_min((R.i - next) * 8 + R.b, 255u) : 0u;
    return rel | (c << 8) | (z << 11) | (n << 18);
}

// pass 1: every lane decodes its subsequence from the cold state, then runs on until it arrives with the recorded state
__global__ __launch_bounds__(kJdWgSubs) void jd_sync_kernel(const JdLaunch L) {
    __shared__ JdTables T;
    __shared__ uint32_t sh[kJdWgSubs];
    const JdJob& J = L.job[job_of(L, blockIdx.x, &JdJob::wg_base)];
    jd_build_tables(J.meta, T);
    const int t = threadIdx.x;
    const uint32_t j = (uint32_t)(blockIdx.x - J.wg_base) * kJdWgSubs + t;
    bool active = j < J.n_sub;
    JdSegment S = {};
    uint32_t cur = 0;
    if (active) {
        S = jd_find_segment(J, j);
        cur = jd_decode<false>(T, J, S, j - S.first_sub, jd_cold(S.bytes, S.len, j - S.first_sub), nullptr, nullptr, 0, nullptr);
    }
    sh[t] = cur;
    __syncthreads();
    for (int r = 1; r < kJdWgSubs; ++r) {
        if (active) {
            const uint32_t tt = t + r, jj = j + r;
            if (tt >= kJdWgSubs || jj >= S.end_sub) {
                active = false;
            } else {
                const uint32_t x = jd_decode<false>(T, J, S, jj - S.first_sub, cur & kStateMask, nullptr, nullptr, 0, nullptr);
                const uint32_t old = sh[tt];
                sh[tt] = x;                                 // (only this lane touches sh[t + r] in round r)
                if ((x & kStateMask) == (old & kStateMask)) active = false;
                cur = x;
            }
        }
        if (!__syncthreads_or(active)) break;
    }
    if (j < J.n_sub) ((uint32_t*)(J.scratch + J.lay.exits))[j] = sh[t];
}

// pass 2, one workgroup per file: carries exit states across the workgroup boundaries of pass 1 until nothing changes, then sums the
// blocks completed per subsequence (exclusive, over the whole file)
__global__ __launch_bounds__(1024) void jd_chain_kernel(const JdLaunch L) {
    __shared__ JdTables T;
    __shared__ uint32_t sh[1024];
    const JdJob& J = L.job[blockIdx.x];
    jd_build_tables(J.meta, T);
    const int t = threadIdx.x;
    volatile uint32_t* exits = (volatile uint32_t*)(J.scratch + J.lay.exits);
    uint32_t* used = (uint32_t*)(J.scratch + J.lay.used);
    uint32_t* sums = (uint32_t*)(J.scratch + J.lay.sums);
    JdHeader* hdr = (JdHeader*)J.scratch;
    for (int w = 1 + t; w < J.lay.n_wg; w += 1024) {
        const uint32_t j0 = (uint32_t)w * kJdWgSubs;
        const JdSegment S = jd_find_segment(J, j0);
        used[w] = jd_cold(S.bytes, S.len, j0 - S.first_sub);
    }
    uint32_t rounds = 0;
    for (int r = 0; r < J.lay.n_wg; ++r) {                      // a round settles at least one more boundary
        int changed = 0;
        for (int w = 1 + t; w < J.lay.n_wg; w += 1024) {
            const uint32_t j0 = (uint32_t)w * kJdWgSubs;
            const JdSegment S = jd_find_segment(J, j0);
            if (j0 == S.first_sub) continue;                // a segment starts here: its entry state is known
            const uint32_t ent = exits[j0 - 1] & kStateMask;
            if (ent == used[w]) continue;
            used[w] = ent;
            changed = 1;
            uint32_t cur = ent;
            const uint32_t j1 = min(min(j0 + kJdWgSubs, S.end_sub), J.n_sub);
            for (uint32_t j = j0; j < j1; ++j) {
                const uint32_t x = jd_decode<false>(T, J, S, j - S.first_sub, cur, nullptr, nullptr, 0, nullptr);
                const uint32_t old = exits[j];
                exits[j] = x;
                if ((x & kStateMask) == (old & kStateMask)) break;
                cur = x & kStateMask;
            }
        }
        ++rounds;
        __threadfence();
        if (!__syncthreads_or(changed)) break;
    }
    if (t == 0) { hdr->err = 0; hdr->ok = 0; hdr->rounds = rounds; hdr->pad = 0; }
    // exclusive sum of the block counts
    uint32_t carry = 0;
    for (uint32_t base = 0; base < J.n_sub; base += 1024) {
        const uint32_t j = base + t;
        const uint32_t v = j < J.n_sub ? exits[j] >> 18 : 0;
        __syncthreads();
        sh[t] = v;
        __syncthreads();
        uint32_t acc = v;
        for (int d = 1; d < 1024; d <<= 1) {
            const uint32_t o = t >= d ? sh[t - d] : 0;
            __syncthreads();
            acc += o;
            sh[t] = acc;
            __syncthreads();
        }
        if (j < J.n_sub) sums[j] = carry + acc - v;
        carry += sh[1023];
    }
}

// pass 3: the same decode from the true entry states, writing coefficients
__global__ __launch_bounds__(kJdWgSubs) void jd_write_kernel(const JdLaunch L) {
    __shared__ JdTables T;
    const JdJob& J = L.job[job_of(L, blockIdx.x, &JdJob::wg_base)];
    jd_build_tables(J.meta, T);
    const uint32_t j = (uint32_t)(blockIdx.x - J.wg_base) * kJdWgSubs + threadIdx.x;
    if (j >= J.n_sub) return;
    const JdSegment S = jd_find_segment(J, j);
    const uint32_t* exits = (const uint32_t*)(J.scratch + J.lay.exits);
    const uint32_t* sums = (const uint32_t*)(J.scratch + J.lay.sums);
    const uint32_t k = j - S.first_sub;
    const uint32_t state = k == 0 ? 0u : exits[j - 1] & kStateMask;
    const uint32_t done = sums[j] - sums[S.first_sub];
    if (done >= S.blk_end - S.blk0) return;                // the segment holds more than its blocks: its end check has failed already
    jd_decode<true>(T, J, S, k, state, (int16_t*)(J.scratch + J.lay.coef), (int32_t*)(J.scratch + J.lay.dc), S.blk0 + done,
                    (JdHeader*)J.scratch);
}

// ---- DC prediction: per component a segmented inclusive sum of the differences, segments = restart intervals ------------------------
struct JdDcSeq { uint32_t n, per_mcu, off; };
JD_HD inline JdDcSeq jd_dc_seq(const JdJob& J, int comp) {
    JdDcSeq q;
    q.per_mcu = comp == 0 ? J.hs * J.vs : 1;
    q.off = comp == 0 ? 0 : J.hs * J.vs + comp - 1;
    q.n = (uint32_t)J.mw * J.mh * q.per_mcu;
    return q;
}

// what a value continues from: the carry, unless a segment started at or before `sum`'s last term
JD_HD inline int jd_carry_in(int carry, int sum, int flag) { return flag ? sum : carry + sum; }

// 256 lanes' (sum since the lane's last segment start, whether it holds one) -> the same over lanes 0..t, in place and in S
struct JdScan { int sum[256], flag[256]; };
__device__ __forceinline__ void jd_seg_scan(JdScan& S, int t, int& sum, int& flag) {
    S.sum[t] = sum; S.flag[t] = flag;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int os = t >= d ? S.sum[t - d] : 0, of = t >= d ? S.flag[t - d] : 0;
        __syncthreads();
        if (!flag) sum += os;
        flag |= of;
        S.sum[t] = sum; S.flag[t] = flag;
        __syncthreads();
    }
}
// after the scan: what lane t's own values continue from, `carry` being what lane 0's do
__device__ __forceinline__ int jd_scan_before(const JdScan& S, int t, int carry) {
    return t == 0 ? carry : jd_carry_in(carry, S.sum[t - 1], S.flag[t - 1]);
}

// kApply false: the chunk's aggregate (sum since its last segment start, whether it holds one) -> recs; true: carry in, DC values out
template <bool kApply>
__global__ __launch_bounds__(256) void jd_dc_kernel(const JdLaunch L) {
    __shared__ JdScan S;
    const int comp = blockIdx.y % 3;
    const JdJob& J = L.job[blockIdx.y / 3];
    if (comp >= J.C) return;
    const JdDcSeq Q = jd_dc_seq(J, comp);
    const uint32_t chunk = blockIdx.x, q0 = chunk * kJdDcChunk + threadIdx.x * 4;
    if (chunk * kJdDcChunk >= Q.n) return;
    int32_t* dc = (int32_t*)(J.scratch + J.lay.dc);
    int v[4], head[4];
    uint32_t at[4];
    int sum = 0, flag = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t q = q0 + e, m = q / Q.per_mcu, sub = q - m * Q.per_mcu;
        at[e] = m * J.bpm + Q.off + sub;
        head[e] = sub == 0 && (J.ri ? m % (uint32_t)J.ri == 0 : m == 0);
        v[e] = q < Q.n ? dc[at[e]] : 0;
        if (q < Q.n) {
            if (head[e]) { sum = v[e]; flag = 1; } else sum += v[e];
        }
    }
    const int t = threadIdx.x;
    jd_seg_scan(S, t, sum, flag);
    if (!kApply) {
        if (t == 255) ((int2*)(J.scratch + J.lay.recs))[comp * J.lay.dc_chunks + chunk] = make_int2(sum, flag);
        return;
    }
    int run = jd_scan_before(S, t, ((const int*)(J.scratch + J.lay.carry))[comp * J.lay.dc_chunks + chunk]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (q0 + e >= Q.n) break;
        run = jd_carry_in(run, v[e], head[e]);
        dc[at[e]] = run;
    }
}

// exclusive scan of the chunk aggregates: what every chunk's first value continues from
__global__ __launch_bounds__(256) void jd_dc_carry_kernel(const JdLaunch L) {
    __shared__ JdScan S;
    const int comp = blockIdx.x % 3, t = threadIdx.x;
    const JdJob& J = L.job[blockIdx.x / 3];
    if (comp >= J.C) return;
    const JdDcSeq Q = jd_dc_seq(J, comp);
    const int chunks = (int)((Q.n + kJdDcChunk - 1) / kJdDcChunk);
    const int2* recs = (const int2*)(J.scratch + J.lay.recs) + comp * J.lay.dc_chunks;
    int* carry = (int*)(J.scratch + J.lay.carry) + comp * J.lay.dc_chunks;
    int run = 0;
    for (int base = 0; base < chunks; base += 256) {
        const int ch = base + t;
        int2 rec = ch < chunks ? recs[ch] : make_int2(0, 0);
        __syncthreads();                                    // (the previous round still reads S)
        jd_seg_scan(S, t, rec.x, rec.y);
        if (ch < chunks) carry[ch] = jd_scan_before(S, t, run);
        run = jd_carry_in(run, S.sum[255], S.flag[255]);
    }
}

// ---- reconstruction ---------------------------------------------------------------------------------------------------------------
// libjpeg's jidctint.c ("islow") on eight values: CONST_BITS 13, the even part scaled by 2^13, `descale` = 11 (columns, PASS1_BITS 2
// kept) or 18 (rows)
JD_HD __forceinline__ void jd_idct8(int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7, int descale) {
    int z1 = (v2 + v6) * 4433;
    const int tmp2e = z1 + v6 * -15137, tmp3e = z1 + v2 * 6270;
    const int tmp0e = (v0 + v4) * 8192, tmp1e = (v0 - v4) * 8192;
    const int tmp10 = tmp0e + tmp3e, tmp13 = tmp0e - tmp3e, tmp11 = tmp1e + tmp2e, tmp12 = tmp1e - tmp2e;
    int tmp0 = v7, tmp1 = v5, tmp2 = v3, tmp3 = v1;
    z1 = tmp0 + tmp3;
    int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int half = 1 << (descale - 1);
    v0 = (tmp10 + tmp3 + half) >> descale; v7 = (tmp10 - tmp3 + half) >> descale;
    v1 = (tmp11 + tmp2 + half) >> descale; v6 = (tmp11 - tmp2 + half) >> descale;
    v2 = (tmp12 + tmp1 + half) >> descale; v5 = (tmp12 - tmp1 + half) >> descale;
    v3 = (tmp13 + tmp0 + half) >> descale; v4 = (tmp13 - tmp0 + half) >> descale;
}

JD_HD inline uint32_t jd_clamp8(int v) { return (uint32_t)jd_min(jd_max(v, 0), 255); }

// one block: dequantise, inverse DCT, +128, clamp; 8 rows of 8 bytes to `dst` (LDS, 8-byte aligned rows of `pitch` bytes).  Always
// inline: its 64 values live in registers, and as a called function (what the compiler chooses once every sampling's code has a
// call site) the pixel kernel would take 180 VGPRs and run two wavefronts per SIMD instead of four
JD_HD __forceinline__ void jd_block(const int16_t* coef, int dcv, const uint8_t* quant, uint8_t* dst, int pitch) {
    int w[64];
    const uint4* src = (const uint4*)coef;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 c = src[r];
        const uint32_t u[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[r * 8 + 2 * k] = (int)(int16_t)(u[k] & 0xFFFF) * quant[r * 8 + 2 * k];
            w[r * 8 + 2 * k + 1] = (int)(int16_t)(u[k] >> 16) * quant[r * 8 + 2 * k + 1];
        }
    }
    w[0] = dcv * quant[0];
#pragma unroll
    for (int c = 0; c < 8; ++c) jd_idct8(w[c], w[8 + c], w[16 + c], w[24 + c], w[32 + c], w[40 + c], w[48 + c], w[56 + c], 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        jd_idct8(w[r * 8], w[r * 8 + 1], w[r * 8 + 2], w[r * 8 + 3], w[r * 8 + 4], w[r * 8 + 5], w[r * 8 + 6], w[r * 8 + 7], 18);
        uint2 o;
        o.x = jd_clamp8(w[r * 8] + 128) | (jd_clamp8(w[r * 8 + 1] + 128) << 8) | (jd_clamp8(w[r * 8 + 2] + 128) << 16) |
              (jd_clamp8(w[r * 8 + 3] + 128) << 24);
        o.y = jd_clamp8(w[r * 8 + 4] + 128) | (jd_clamp8(w[r * 8 + 5] + 128) << 8) | (jd_clamp8(w[r * 8 + 6] + 128) << 16) |
              (jd_clamp8(w[r * 8 + 7] + 128) << 24);
        *(uint2*)(dst + r * pitch) = o;
    }
}

constexpr int kTileH = 64, kTileW = 128;

// One workgroup, one 64 x 128 pixel tile: its blocks' samples go to LDS, then every lane converts and stores pixels.  Where chroma is
// subsampled along an axis that libjpeg filters (by two), the chroma blocks next to the tile along that axis come along as a halo, so
// the upsampling filter never leaves LDS and Y is read from memory once.
struct JdTile {
    __attribute__((aligned(16))) uint8_t plane[3][kTileH * kTileW];
    uint8_t quant[3][64];                                  // per component, natural order
};

// A tile's chroma plane under luma sampling kHs x kVs, in 8 x 8 blocks: 16 / kHs x 8 / kVs of them and the halo.
//   1x1 (4:4:4, gray)  128 x 64 samples, no halo              128 blocks, rows of 128 bytes
//   2x2 (4:2:0)         64 x 32, one block all round           60 blocks, rows of 80
//   2x1 (4:2:2)         64 x 64, one block left and right      80 blocks, rows of 80
//   1x2 (4:4:0)        128 x 32, one block above and below     96 blocks, rows of 128
//   4x1 (4:1:1)         32 x 64, no halo (plain replication)   32 blocks, rows of 32
template <int kHs, int kVs>
struct JdChroma {
    static constexpr int hs = kHs, vs = kVs, halo_x = kHs == 2, halo_y = kVs == 2;
    static constexpr int bw = 16 / kHs + 2 * halo_x, bh = 8 / kVs + 2 * halo_y, blocks = bw * bh, pitch = 8 * bw;
    static_assert(blocks * 64 <= kTileH * kTileW, "a chroma plane with its halo fits the plane of a tile");
};

// calls f(JdChroma<hs, vs>) for the job's sampling: the one place the decoder branches on it, uniform over a workgroup
template <class F>
JD_HD inline void jd_with_sampling(const JdJob& J, F f) {
    switch (J.hs * 4 + J.vs) {
        case 1 * 4 + 1: f(JdChroma<1, 1>()); break;
        case 2 * 4 + 2: f(JdChroma<2, 2>()); break;
        case 2 * 4 + 1: f(JdChroma<2, 1>()); break;
        case 1 * 4 + 2: f(JdChroma<1, 2>()); break;
        case 4 * 4 + 1: f(JdChroma<4, 1>()); break;
        default: break;                                    // (jd_fill_job sets no other)
    }
}

JD_HD inline void jd_tile_quant(const JdJob& J, JdTile& T, int tid) {
    if (tid < 192) {
        const int comp = tid >> 6, z = tid & 63;
        T.quant[comp][jd_natural(z)] = comp < J.C ? J.meta[4 * GS360_JPEG_TABLE_BYTES + J.tq[comp] * 64 + z] : 1;
    }
}

template <int kHs, int kVs>
JD_HD inline void jd_tile_blocks_s(const JdJob& J, JdTile& T, int tx, int ty, int tid) {
    using G = JdChroma<kHs, kVs>;
    const int16_t* coef = (const int16_t*)(J.scratch + J.lay.coef);
    const int32_t* dc = (const int32_t*)(J.scratch + J.lay.dc);
    const int bpm = kHs * kVs > 1 ? kHs * kVs + 2 : J.C;
    const int n_tasks = 128 + (J.C == 3 ? 2 * G::blocks : 0);
    for (int task = tid; task < n_tasks; task += 256) {
        int comp = 0, blk = -1, pitch = kTileW, at;
        if (task < 128) {
            const int by = task >> 4, bx = task & 15, gx = tx * 16 + bx, gy = ty * 8 + by;
            at = by * 8 * kTileW + bx * 8;
            if (gx < kHs * J.mw && gy < kVs * J.mh) blk = ((gy / kVs) * J.mw + gx / kHs) * bpm + (gy % kVs) * kHs + gx % kHs;
        } else {
            const int ci = task - 128;
            comp = 1 + ci / G::blocks;
            const int bi = ci % G::blocks, cy = bi / G::bw, cx = bi % G::bw;
            const int gx = tx * (16 / kHs) - G::halo_x + cx, gy = ty * (8 / kVs) - G::halo_y + cy;
            pitch = G::pitch;
            at = cy * 8 * G::pitch + cx * 8;
            if (gx >= 0 && gy >= 0 && gx < J.mw && gy < J.mh) blk = (gy * J.mw + gx) * bpm + kHs * kVs + comp - 1;
        }
        if (blk >= 0) jd_block(coef + (size_t)blk * 64, dc[blk], T.quant[comp], &T.plane[comp][at], pitch);
    }
}

// libjpeg's upsampling of a chroma plane cropped to cw x ch samples, the cropped edges replicated, at pixel (gx, gy):
//   by two along one axis ("fancy" h2v1 / h1v2): (3 s + the nearer neighbour + 1 (even pixels) or 2 (odd)) >> 2
//   by two along both (h2v2): that filter down the columns without its shift, then along the rows: + 8 (even) or 7 (odd), >> 4
//   by four (h4v1): the sample itself
//   by two along x (h2v1, h2v2) of a plane of one or two samples a row: the sample itself on both axes; libjpeg picks its filters
//   only for planes more than two samples wide
// kGray: the output is an H x W plane of FS-SPEC's gray, (4899 R + 9617 G + 1868 B + 8192) >> 14 of the pixel the RGB mode stores
// (gray_of<3> with red = 0, after libjpeg's colour conversion and its clamps; not the file's Y, which differs by rounding); a
// C = 1 file's byte is its Y sample in both modes
template <int kHs, int kVs, bool kGray>
JD_HD inline void jd_tile_pixels_s(const JdJob& J, const JdTile& T, int tx, int ty, int tid) {
    using G = JdChroma<kHs, kVs>;
    const int x = tid & 127, gx = tx * kTileW + x;
    if (gx >= J.W) return;
    const int cw = (J.W + kHs - 1) / kHs, ch = (J.H + kVs - 1) / kVs;
    const int x0 = tx * (kTileW / kHs) - 8 * G::halo_x, y0 = ty * (kTileH / kVs) - 8 * G::halo_y;   // the chroma tile's first sample
    const int cx = gx / kHs, nx = (gx & 1) ? jd_min(cx + 1, cw - 1) : jd_max(cx - 1, 0);
    const int lcx = cx - x0, lnx = nx - x0;
    for (int i = 0; i < kTileH / 2; ++i) {
        const int y = (tid >> 7) + 2 * i, gy = ty * kTileH + y;
        if (gy >= J.H) break;
        uint8_t* o = J.out + (size_t)gy * J.stride + (size_t)gx * (kGray ? 1 : J.C);
        const int Y = T.plane[0][y * kTileW + x];
        if (kHs * kVs == 1 && J.C == 1) {
            o[0] = (uint8_t)Y;
            continue;
        }
        const int cy = gy / kVs, ny = (gy & 1) ? jd_min(cy + 1, ch - 1) : jd_max(cy - 1, 0);
        const int r0 = (cy - y0) * G::pitch, r1 = (ny - y0) * G::pitch;
        int cb, cr;
        if (kHs == 2 && cw <= 2) {
            cb = T.plane[1][r0 + lcx];
            cr = T.plane[2][r0 + lcx];
        } else if (kHs == 2 && kVs == 2) {
            const int bias = (gx & 1) ? 7 : 8;
            const int sb = 3 * T.plane[1][r0 + lcx] + T.plane[1][r1 + lcx], sbn = 3 * T.plane[1][r0 + lnx] + T.plane[1][r1 + lnx];
            const int sr = 3 * T.plane[2][r0 + lcx] + T.plane[2][r1 + lcx], srn = 3 * T.plane[2][r0 + lnx] + T.plane[2][r1 + lnx];
            cb = (3 * sb + sbn + bias) >> 4;
            cr = (3 * sr + srn + bias) >> 4;
        } else if (kHs == 2) {
            const int bias = (gx & 1) ? 2 : 1;
            cb = (3 * T.plane[1][r0 + lcx] + T.plane[1][r0 + lnx] + bias) >> 2;
            cr = (3 * T.plane[2][r0 + lcx] + T.plane[2][r0 + lnx] + bias) >> 2;
        } else if (kVs == 2) {
            const int bias = (gy & 1) ? 2 : 1;
            cb = (3 * T.plane[1][r0 + lcx] + T.plane[1][r1 + lcx] + bias) >> 2;
            cr = (3 * T.plane[2][r0 + lcx] + T.plane[2][r1 + lcx] + bias) >> 2;
        } else {
            cb = T.plane[1][r0 + lcx];
            cr = T.plane[2][r0 + lcx];
        }
        cb -= 128; cr -= 128;
        const uint32_t r = jd_clamp8(Y + ((91881 * cr + 32768) >> 16));
        const uint32_t g = jd_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        const uint32_t b = jd_clamp8(Y + ((116130 * cb + 32768) >> 16));
        if (kGray) {
            o[0] = (uint8_t)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14);
        } else {
            o[0] = (uint8_t)r;
            o[1] = (uint8_t)g;
            o[2] = (uint8_t)b;
        }
    }
}

// the two steps for whatever the job's sampling is (a host program steps these)
JD_HD inline void jd_tile_blocks(const JdJob& J, JdTile& T, int tx, int ty, int tid) {
    jd_with_sampling(J, [&](auto g) { jd_tile_blocks_s<decltype(g)::hs, decltype(g)::vs>(J, T, tx, ty, tid); });
}
template <bool kGray = false>
JD_HD inline void jd_tile_pixels(const JdJob& J, const JdTile& T, int tx, int ty, int tid) {
    jd_with_sampling(J, [&](auto g) { jd_tile_pixels_s<decltype(g)::hs, decltype(g)::vs, kGray>(J, T, tx, ty, tid); });
}

template <bool kGray>
__global__ __launch_bounds__(256) void jd_pixels_kernel(const JdLaunch L) {
    __shared__ JdTile T;
    const JdJob& J = L.job[job_of(L, blockIdx.x, &JdJob::tile_base)];
    const int tile = blockIdx.x - J.tile_base, tx = tile % J.tiles_x, ty = tile / J.tiles_x;
    jd_tile_quant(J, T, threadIdx.x);
    __syncthreads();
    jd_with_sampling(J, [&](auto g) {                      // one switch per workgroup: each sampling has its own blocks and pixels code
        jd_tile_blocks_s<decltype(g)::hs, decltype(g)::vs>(J, T, tx, ty, threadIdx.x);
        __syncthreads();
        jd_tile_pixels_s<decltype(g)::hs, decltype(g)::vs, kGray>(J, T, tx, ty, threadIdx.x);
    });
}

__global__ void jd_status_kernel(const JdLaunch L) {
    const int k = threadIdx.x;
    if (k >= L.n_jobs) return;
    const JdHeader* h = (const JdHeader*)L.job[k].scratch;
    L.status[k] = h->err ? 1u : (h->ok != L.job[k].n_seg ? 2u : 0u);
}

}  // namespace

hipError_t launch_jpeg_decode(const JdLaunch& L, bool gray, hipStream_t s) {
    for (int k = 0; k < L.n_jobs; ++k) {
        const JdJob& J = L.job[k];
        if (hipError_t e = hipMemsetAsync(J.scratch + J.lay.coef, 0, (size_t)J.lay.blocks * 128, s)) return e;
        if (hipError_t e = hipMemsetAsync(J.scratch + J.lay.dc, 0, (size_t)J.lay.blocks * 4, s)) return e;
    }
    hipLaunchKernelGGL(jd_sync_kernel, dim3(L.total_wg), dim3(kJdWgSubs), 0, s, L);
    hipLaunchKernelGGL(jd_chain_kernel, dim3(L.n_jobs), dim3(1024), 0, s, L);
    hipLaunchKernelGGL(jd_write_kernel, dim3(L.total_wg), dim3(kJdWgSubs), 0, s, L);
    hipLaunchKernelGGL(jd_dc_kernel<false>, dim3(L.max_dc_chunks, L.n_jobs * 3), dim3(256), 0, s, L);
    hipLaunchKernelGGL(jd_dc_carry_kernel, dim3(L.n_jobs * 3), dim3(256), 0, s, L);
    hipLaunchKernelGGL(jd_dc_kernel<true>, dim3(L.max_dc_chunks, L.n_jobs * 3), dim3(256), 0, s, L);
    if (gray) hipLaunchKernelGGL(jd_pixels_kernel<true>, dim3(L.total_tiles), dim3(256), 0, s, L);
    else hipLaunchKernelGGL(jd_pixels_kernel<false>, dim3(L.total_tiles), dim3(256), 0, s, L);
    hipLaunchKernelGGL(jd_status_kernel, dim3(1), dim3(64), 0, s, L);
    return hipGetLastError();
}

}  // namespace gs360
