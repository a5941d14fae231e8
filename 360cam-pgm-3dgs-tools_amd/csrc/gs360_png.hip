// gs360_png.hip -- the deflate stream of PNG files from 8- and 16-bit images resident on the device (PNG-SPEC v1).
//
// Reference: the PNG writers behind the views (gs360/imageio.py: Pillow at compress_level 3 for 8 bits, filter 0 + zlib level 3 for
// 16), which compress on one host thread per view.  Everything is integer arithmetic and every choice has a stated tie-break, so the
// stream is pinned byte for byte (tests/pngenc_np.py).
//
//   filter     one workgroup per row: the five PNG filters' costs (sum of |residual as int8|) in one sweep, a wave reduction, the
//              smallest (ties to the lower type) written as the row's 1 + W * bpp bytes of the filtered stream
//   parse      one workgroup per chunk of 64 KiB, the chunk in LDS (a pad dword per segment keeps the lanes on their own banks), one
//              lane per segment of 512 bytes: a greedy walk over the three candidate distances (1, bpp, 1 + W * bpp) adds to the
//              chunk's literal/length and distance histograms and to its Adler-32 partial sums; wavefront 0 and 1 build the two
//              code tables (the Huffman steps jp_tables_kernel takes, gs360_codecsteps.h, lengths limited to 15); the walk runs again for the
//              segments' bit counts, whose exclusive scan places them
//   placement  one workgroup per image: exclusive scan of the chunks' byte lengths, the stream's length (UINT64_MAX past the capacity)
//   emit       the parse kernel's walk a third time, writing: each lane owns the bytes that begin inside its segment's bits, stores them
//              as bytes and completes its last one from the leading bits the lanes behind it publish in LDS
// The walk is repeated instead of stored: a symbol list would take twice the filtered stream in device memory, the walk reads LDS only.
#include "gs360_codecsteps.h"

namespace gs360 {
namespace {

constexpr int kPnFilterThreads = 256;
constexpr int kPnSegDw = kPnSegment / 4 + 1;             // dwords of a staged segment with its pad
constexpr int kPnHeadBits = 74 + 4 * kPnSyms;            // the block header: 17 bits, 19 x 3 code-length-code lengths, 316 x 4
constexpr int kPnHeadDw = (kPnHeadBits + 31) / 32;
static_assert(kPnHeadBits % 8 != 0, "the header ends inside a byte that segment 0 completes");
static_assert(kPnThreads == 128 && kPnChunk / kPnSegment == kPnThreads, "two wavefronts: one per code table, one lane per segment");

// ---- filter ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pn_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ uint32_t pn_cost(int r) {
    r &= 255;
    return (uint32_t)(r < 128 ? r : 256 - r);
}
// the residual of filter `type` for byte x with left a, upper b and upper-left c
__device__ __forceinline__ int pn_residual(int type, int x, int a, int b, int c) {
    return type == 0 ? x : type == 1 ? x - a : type == 2 ? x - b : type == 3 ? x - ((a + b) >> 1) : x - pn_paeth(a, b, c);
}

__global__ void __launch_bounds__(kPnFilterThreads) pn_filter_kernel(const PnLaunch L) {
    __shared__ uint32_t wsum[kPnFilterThreads / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PnJob J = L.job[job_of(L, blockIdx.x, &PnJob::row_base)];
    const int y = blockIdx.x - J.row_base, Wb = J.Wb, bpp = J.bpp, sw = J.swap;    // sw: 16-bit samples leave big-endian
    const uint8_t* cur = J.src + (int64_t)y * J.stride;
    const uint8_t* up = y ? cur - J.stride : nullptr;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < Wb; i += kPnFilterThreads) {
        const int x = cur[i ^ sw], a = i >= bpp ? cur[(i - bpp) ^ sw] : 0;
        const int b = up ? up[i ^ sw] : 0, c = (up && i >= bpp) ? up[(i - bpp) ^ sw] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += pn_cost(pn_residual(t, x, a, b, c));
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cost[t] += __shfl_xor(cost[t], o, 64);
        if (lane == 0) wsum[wave][t] = cost[t];
    }
    __syncthreads();
    int pick = 0;
    uint32_t best = UINT32_MAX;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kPnFilterThreads / 64; ++w) s += wsum[w][t];
        if (s < best) { best = s; pick = t; }                                      // ties: the lower type
    }
    uint8_t* dst = L.filt + J.filt_base + (int64_t)y * (1 + Wb);
    if (tid == 0) dst[0] = (uint8_t)pick;
    for (int i = tid; i < Wb; i += kPnFilterThreads) {
        const int x = cur[i ^ sw], a = i >= bpp ? cur[(i - bpp) ^ sw] : 0;
        const int b = up ? up[i ^ sw] : 0, c = (up && i >= bpp) ? up[(i - bpp) ^ sw] : 0;
        dst[1 + i] = (uint8_t)pn_residual(pick, x, a, b, c);
    }
}

// ---- the walk over a staged chunk ------------------------------------------------------------------------------------------------
struct PnChunk {                                         // a workgroup's chunk
    int c, len, nseg, last;                              // chunk of the image, its bytes and segments; last: the image's last chunk
};
__device__ __forceinline__ PnChunk pn_chunk_of(const PnJob& J) {
    PnChunk k;
    k.c = blockIdx.x - J.chunk_base;
    k.len = (int)min((int64_t)kPnChunk, J.n - (int64_t)k.c * kPnChunk);
    k.nseg = (k.len + kPnSegment - 1) / kPnSegment;
    k.last = k.c + 1 == J.n_chunks;
    return k;
}
// the chunk's bytes -> LDS, segment s at dword s * kPnSegDw (the filtered stream of an image starts 256-byte aligned and has a dword of
// slack behind it: whole dwords are read)
__device__ __forceinline__ void pn_stage(uint32_t* data, const uint8_t* filt, const PnJob& J, const PnChunk& k) {
    const uint32_t* src = (const uint32_t*)(filt + J.filt_base + (int64_t)k.c * kPnChunk);
    for (int i = threadIdx.x; i < (k.len + 3) >> 2; i += kPnThreads) data[i + i / (kPnSegment / 4)] = src[i];
}
__device__ __forceinline__ int pn_byte(const uint8_t* d, int q) { return d[q + (q / kPnSegment) * 4]; }

// the three candidates of an image as named scalars (indexed members of the job would put it into scratch memory)
struct PnCand {
    int d0, d1, d2, s0, s1, s2, b0, b1, b2;
    uint32_t v0, v1, v2;
    __device__ __forceinline__ explicit PnCand(const PnJob& J)
        : d0(J.dist[0]), d1(J.dist[1]), d2(J.dist[2]), s0(J.dsym[0]), s1(J.dsym[1]), s2(J.dsym[2]), b0(J.dbits[0]), b1(J.dbits[1]),
          b2(J.dbits[2]), v0(J.dval[0]), v1(J.dval[1]), v2(J.dval[2]) {}
    // candidate k's distance symbol among the chunk's 316 (286 literal/length, then 30 distance), its extra bits and their value
    __device__ __forceinline__ int sym(int k) const { return kPnLitLen + (k == 0 ? s0 : k == 1 ? s1 : s2); }
    __device__ __forceinline__ int bits(int k) const { return k == 0 ? b0 : k == 1 ? b1 : b2; }
    __device__ __forceinline__ uint32_t val(int k) const { return k == 0 ? v0 : k == 1 ? v1 : v2; }
};

// the symbol at chunk position q of a segment that ends at `end`: -> its length (1: the literal) and candidate
struct PnSym { int len, k; };
__device__ __forceinline__ void pn_try(const uint8_t* d, int q, int maxl, int dk, int k, PnSym& s) {
    if (dk == 0 || dk > q) return;                       // unusable candidate, or a source in front of the chunk
    // it is taken only if it is longer than the best so far and than 2, so the byte that would make it so is looked at first: most
    // positions end here, and a run that an earlier candidate already followed to its end is not followed again
    const int need = max(s.len, 2);
    if (need >= maxl || pn_byte(d, q + need) != pn_byte(d, q + need - dk)) return;
    int l = 0;
    while (l < maxl && pn_byte(d, q + l) == pn_byte(d, q + l - dk)) ++l;
    if (l >= 3 && l > s.len) { s.len = l; s.k = k; }     // ties: the earlier candidate
}
__device__ __forceinline__ PnSym pn_step(const uint8_t* d, int q, int end, const PnCand& K) {
    PnSym s{1, 0};
    const int maxl = min(258, end - q);
    pn_try(d, q, maxl, K.d0, 0, s);
    pn_try(d, q, maxl, K.d1, 1, s);
    pn_try(d, q, maxl, K.d2, 2, s);
    return s;
}
// RFC 1951 3.2.5: a match length's symbol, extra bits and their value
__device__ __forceinline__ void pn_len_code(int len, int& sym, int& eb, int& ev) {
    const int l = len - 3;
    eb = 0; ev = 0;
    if (len == 258) { sym = 285; return; }
    if (l < 8) { sym = 257 + l; return; }
    eb = 29 - __clz(l);                                  // floor(log2(l)) - 2
    sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
    ev = l & ((1 << eb) - 1);
}

// ---- parse: histograms, code tables, bit counts ---------------------------------------------------------------------------------------
// Code lengths of one alphabet by one wavefront, entry e = lane + 64 * k, from the steps jp_tables_kernel takes as well
// (gs360_codecsteps.h): Huffman's merges (huff_merge), the counts of lengths above 15 folded down by T.81 K.3's procedure
// (huff_fold_lengths), the final lengths handed out in order of (unlimited length, symbol) (huff_rank).  An alphabet with no symbol
// used gives symbol 0 one bit, with one symbol used that symbol one bit.
// The codes are RFC 1951's canonical ones, kept bit-reversed (the stream is LSB-first) as (code << 5) | length.
struct PnTableLds {
    uint8_t cs[2][320], lim[2][320];
    int bits[2][64];
};
__device__ __forceinline__ void pn_build_tables(PnTableLds& T, const uint32_t* hist, uint32_t* code) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = wave ? kPnDist : kPnLitLen, at = wave ? kPnLitLen : 0;
    uint32_t f[5];
    int len[5];
    bool used[5];
    int nused = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k;
        f[k] = e < n ? hist[at + e] : 0u;
        used[k] = f[k] != 0;
        nused += __popcll(__ballot(used[k]));
    }
    T.bits[wave][lane] = 0;
    huff_merge(f, used, len, lane);
    __syncthreads();                                                              // bits[] zeroed
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        T.cs[wave][lane + 64 * k] = (uint8_t)len[k];
        if (len[k]) atomicAdd(&T.bits[wave][len[k] & 63], 1);
    }
    __syncthreads();
    if (lane == 0) {
        // (its j > 0 guard never binds for a complete code; it keeps other input from walking out of bits[])
        huff_fold_lengths(T.bits[wave], 15);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k, le = len[k];
        int l = 0;
        if (nused < 2) {
            l = (nused ? used[k] : e == 0) ? 1 : 0;
        } else if (le) {
            int rank = huff_rank(T.cs[wave], n, le, e);
            l = 1;
            while (l < 15 && rank >= T.bits[wave][l]) { rank -= T.bits[wave][l]; ++l; }
        }
        T.lim[wave][e] = (uint8_t)l;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k, l = T.lim[wave][e];
        if (e >= n) continue;
        uint32_t c = 0;                                                           // RFC 1951 3.2.2, summed per entry
        for (int s = 0; s < n; ++s) {
            const int ls = T.lim[wave][s];
            if (ls && ls < l) c += 1u << (l - ls);
            else if (ls == l && s < e) c += 1u;
        }
        code[at + e] = l ? ((__brev(c) >> (32 - l)) << 5) | (uint32_t)l : 0u;
    }
    __syncthreads();
}

struct PnLds {
    uint32_t data[kPnThreads * kPnSegDw];
    uint32_t code[320];                                  // (reversed code << 5) | length: 286 literal/length symbols, then 30 distances
};

__global__ void __launch_bounds__(kPnThreads) pn_parse_kernel(const PnLaunch L) {
    __shared__ PnLds S;
    __shared__ PnTableLds T;
    __shared__ uint32_t hist[320];
    __shared__ unsigned long long adler[2];
    __shared__ uint32_t wsum[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PnJob J = L.job[job_of(L, blockIdx.x, &PnJob::chunk_base)];
    const PnChunk k = pn_chunk_of(J);
    const PnCand K(J);
    pn_stage(S.data, L.filt, J, k);
    for (int i = tid; i < 320; i += kPnThreads) hist[i] = i == 256 ? 1u : 0u;     // the end-of-block symbol
    if (tid < 2) adler[tid] = 0;
    __syncthreads();
    const uint8_t* d = (const uint8_t*)S.data;
    const int q0 = tid * kPnSegment, end = min(k.len, q0 + kPnSegment);
    if (tid < k.nseg) {
        unsigned long long a = 0, b = 0;                                          // sum of the bytes, sum of (len - q) * byte
        for (int q = q0; q < end; ++q) {
            const unsigned long long v = (unsigned long long)pn_byte(d, q);
            a += v;
            b += v * (unsigned long long)(k.len - q);
        }
        atomicAdd(&adler[0], a);
        atomicAdd(&adler[1], b);
        for (int q = q0; q < end;) {
            const PnSym s = pn_step(d, q, end, K);
            if (s.len == 1) {
                atomicAdd(&hist[pn_byte(d, q)], 1u);
            } else {
                int sym, eb, ev;
                pn_len_code(s.len, sym, eb, ev);
                atomicAdd(&hist[sym], 1u);
                atomicAdd(&hist[K.sym(s.k)], 1u);
            }
            q += s.len;
        }
    }
    __syncthreads();
    pn_build_tables(T, hist, S.code);
    uint32_t nbits = 0;
    if (tid < k.nseg) {
        for (int q = q0; q < end;) {
            const PnSym s = pn_step(d, q, end, K);
            if (s.len == 1) {
                nbits += S.code[pn_byte(d, q)] & 31u;
            } else {
                int sym, eb, ev;
                pn_len_code(s.len, sym, eb, ev);
                nbits += (S.code[sym] & 31u) + (uint32_t)eb + (S.code[K.sym(s.k)] & 31u) + (uint32_t)K.bits(s.k);
            }
            q += s.len;
        }
    }
    const uint32_t incl = wave_scan(nbits, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    const size_t chunk = blockIdx.x;
    L.seg_off[chunk * kPnThreads + tid] = (uint32_t)kPnHeadBits + (wave ? wsum[0] : 0u) + incl - nbits;
    for (int i = tid; i < 320; i += kPnThreads) L.codes[chunk * 320 + i] = S.code[i];
    if (tid == 0) {
        // header, symbols, end of block, the stored block's three header bits, padding to a byte, LEN and NLEN
        const uint32_t total = (uint32_t)kPnHeadBits + wsum[0] + wsum[1] + (S.code[256] & 31u) + 3u;
        L.chunk_len[chunk] = ((total + 7u) >> 3) + 4u;
        L.adler[chunk * 2] = (uint32_t)(adler[0] % 65521ull);
        L.adler[chunk * 2 + 1] = (uint32_t)(adler[1] % 65521ull);
    }
}

// ---- placement: one workgroup per image, exclusive scan of its chunks' lengths ------------------------------------------------------
__global__ void __launch_bounds__(kPlaceThreads) pn_offsets_kernel(const PnLaunch L) {
    const PnJob J = L.job[blockIdx.x];
    const unsigned long long run = place_pieces(L.chunk_len + J.chunk_base, L.chunk_off + J.chunk_base, J.n_chunks);
    if (threadIdx.x == 0) L.lengths[blockIdx.x] = run <= J.cap ? run : UINT64_MAX;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------
// the header's first 74 bits, LSB first: BFINAL 0, BTYPE 2, HLIT 286 - 257, HDIST 30 - 1, HCLEN 19 - 4, then the code-length code's
// lengths in RFC 1951's order 16 17 18 0 8 7 ...: 0 for the three repeat symbols, 4 for the lengths 0..15
struct PnHead { uint32_t w[3]; };
constexpr PnHead pn_make_head() {
    PnHead h{};
    unsigned __int128 v = (2u << 1) | ((unsigned)(kPnLitLen - 257) << 3) | ((unsigned)(kPnDist - 1) << 8) | (15u << 13);
    for (int k = 3; k < 19; ++k) v |= (unsigned __int128)4 << (17 + 3 * k);
    h.w[0] = (uint32_t)v; h.w[1] = (uint32_t)(v >> 32); h.w[2] = (uint32_t)(v >> 64);
    return h;
}
constexpr PnHead kPnHead = pn_make_head();

// A lane's bit writer.  The lane's bits start at stream bit `at` of the chunk; it stores every byte that BEGINS inside them (so not a
// first byte it shares with the lanes in front) and keeps what is left of its last byte for pn_finish.  lead / count: its first bits,
// at most seven, for the lanes in front whose last bytes they complete.
struct PnWriter {
    uint8_t* p;
    uint64_t acc = 0;
    int nacc;
    bool skip;
    uint32_t lead = 0, count = 0;
    __device__ __forceinline__ PnWriter(uint8_t* chunk_out, uint32_t at) : p(chunk_out + (at >> 3)), nacc((int)(at & 7)), skip((at & 7) != 0) {}
    __device__ __forceinline__ void put(uint64_t v, int n) {                      // n <= 48
        if (count < 7) lead |= (uint32_t)(v << count) & 127u;
        count = min(count + (uint32_t)n, 7u);
        acc |= v << nacc;
        nacc += n;
        while (nacc >= 8) {
            if (skip) skip = false;
            else *p = (uint8_t)acc;
            ++p;
            acc >>= 8;
            nacc -= 8;
        }
    }
};

__global__ void __launch_bounds__(kPnThreads) pn_emit_kernel(const PnLaunch L) {
    __shared__ PnLds S;
    __shared__ uint32_t head[kPnHeadDw];
    __shared__ uint32_t lead[kPnThreads], count[kPnThreads];
    const int tid = threadIdx.x;
    const int j = job_of(L, blockIdx.x, &PnJob::chunk_base);
    const PnJob J = L.job[j];
    const PnChunk k = pn_chunk_of(J);
    const PnCand K(J);
    if (L.lengths[j] == UINT64_MAX) return;                           // the stream does not fit: nothing of it is written
    const size_t chunk = blockIdx.x;
    uint8_t* out = J.out + L.chunk_off[chunk];
    pn_stage(S.data, L.filt, J, k);
    for (int i = tid; i < 320; i += kPnThreads) S.code[i] = L.codes[chunk * 320 + i];
    if (tid < kPnHeadDw) head[tid] = tid < 3 ? kPnHead.w[tid] : 0u;
    __syncthreads();
    for (int i = tid; i < kPnSyms; i += kPnThreads) {                             // the code lengths, each as its fixed 4-bit code
        const uint32_t l = S.code[i] & 31u, v = __brev(l) >> 28;
        const int pos = 74 + 4 * i, sh = pos & 31;
        atomicOr(&head[pos >> 5], v << sh);
        if (sh > 28) atomicOr(&head[(pos >> 5) + 1], v >> (32 - sh));
    }
    __syncthreads();
    for (int i = tid; i < kPnHeadBits / 8; i += kPnThreads) out[i] = (uint8_t)(head[i >> 2] >> (8 * (i & 3)));
    const uint8_t* d = (const uint8_t*)S.data;
    const int q0 = tid * kPnSegment, end = min(k.len, q0 + kPnSegment);
    PnWriter w(out, tid < k.nseg ? L.seg_off[chunk * kPnThreads + tid] : 0u);
    if (tid < k.nseg) {
        for (int q = q0; q < end;) {
            const PnSym s = pn_step(d, q, end, K);
            if (s.len == 1) {
                const uint32_t e = S.code[pn_byte(d, q)];
                w.put(e >> 5, (int)(e & 31u));
            } else {
                int sym, eb, ev;
                pn_len_code(s.len, sym, eb, ev);
                const uint32_t e1 = S.code[sym], e2 = S.code[K.sym(s.k)];
                const int l1 = (int)(e1 & 31u), l2 = (int)(e2 & 31u), db = K.bits(s.k);
                const uint64_t v = (uint64_t)(e1 >> 5) | ((uint64_t)ev << l1) | ((uint64_t)(e2 >> 5) << (l1 + eb)) |
                                   ((uint64_t)K.val(s.k) << (l1 + eb + l2));
                w.put(v, l1 + eb + l2 + db);
            }
            q += s.len;
        }
        if (tid == k.nseg - 1) {                                                  // end of block, then the empty stored block
            w.put(S.code[256] >> 5, (int)(S.code[256] & 31u));
            w.put(k.last ? 1u : 0u, 3);
            if (w.nacc) w.put(0, 8 - w.nacc);
            w.put(0xFFFF0000ull, 32);
        }
        lead[tid] = w.lead;
        count[tid] = w.count;
    }
    __syncthreads();
    // a last byte that is not full: the bits behind it are the next segments' first ones (the last segment brings at least seven)
    if (tid < k.nseg && w.nacc && !w.skip) {
        uint32_t v = (uint32_t)w.acc & 255u;
        int have = w.nacc;
        for (int t = tid + 1; have < 8 && t < k.nseg; ++t) { v |= lead[t] << have; have += (int)count[t]; }
        *w.p = (uint8_t)v;
    }
    if (tid == 0) {                                                               // the header's last byte, shared with segment 0
        constexpr int kByte = kPnHeadBits / 8;
        uint32_t v = (head[kByte >> 2] >> (8 * (kByte & 3))) & 255u;
        int have = kPnHeadBits & 7;
        for (int t = 0; have < 8 && t < k.nseg; ++t) { v |= lead[t] << have; have += (int)count[t]; }
        out[kByte] = (uint8_t)v;
    }
}

}  // namespace

hipError_t launch_png_deflate(const PnLaunch& L, hipStream_t s) {
    hipLaunchKernelGGL(pn_filter_kernel, dim3(L.total_rows), dim3(kPnFilterThreads), 0, s, L);
    hipLaunchKernelGGL(pn_parse_kernel, dim3(L.total_chunks), dim3(kPnThreads), 0, s, L);
    hipLaunchKernelGGL(pn_offsets_kernel, dim3(L.n_jobs), dim3(kPlaceThreads), 0, s, L);
    hipLaunchKernelGGL(pn_emit_kernel, dim3(L.total_chunks), dim3(kPnThreads), 0, s, L);
    return hipGetLastError();
}

}  // namespace gs360
