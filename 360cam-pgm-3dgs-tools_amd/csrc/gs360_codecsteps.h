// gs360_codecsteps.h -- the steps the two device encoders share (gs360_jpeg.hip, JPG-SPEC v1; gs360_png.hip, PNG-SPEC v1): the wave
// scan and minimum, Huffman's merges with the fold of over-long lengths and the rank that hands the limited lengths out, and the
// placement of an image's pieces.  Private to those two files; what differs between the codecs (the length limit, what becomes of
// the limited lengths, where the arrays live, the bit writers) stays in them.
#pragma once
#include "gs360_kernels.h"

namespace gs360 {

// inclusive sum over the lanes of a wavefront
template <class T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = __shfl_xor((unsigned long long)v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// Huffman's merges over up to 320 entries by one wavefront, entry e = lane + 64 * k with count f[k] (0: the entry takes no part;
// used[k]: it had a count to begin with).  A step takes the two smallest non-zero counts, ties to the LARGEST index (two wave minima
// of count << 9 | 511 - index), adds the second to the first and lengthens every entry of both trees: each entry carries its tree's id
// (the index that holds the tree's count), so the lanes lengthen and relabel their own entries, the same set of symbols libjpeg's
// jpeg_gen_optimal_table reaches along its others[] chain.  -> len[k], the unlimited code lengths; f[] is used up.
__device__ __forceinline__ void huff_merge(uint32_t (&f)[5], const bool (&used)[5], int (&len)[5], int lane) {
    int grp[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        grp[k] = lane + 64 * k;
        len[k] = 0;
    }
    for (;;) {
        uint64_t best = UINT64_MAX;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint64_t key = ((uint64_t)f[k] << 9) | (uint64_t)(511 - (lane + 64 * k));
            if (f[k] && key < best) best = key;
        }
        const uint64_t key1 = wave_min(best);
        const int c1 = 511 - (int)(key1 & 511);
        best = UINT64_MAX;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int e = lane + 64 * k;
            const uint64_t key = ((uint64_t)f[k] << 9) | (uint64_t)(511 - e);
            if (f[k] && e != c1 && key < best) best = key;
        }
        const uint64_t key2 = wave_min(best);
        if (key2 == UINT64_MAX) break;
        const int c2 = 511 - (int)(key2 & 511);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int e = lane + 64 * k;
            if (e == c1) f[k] += (uint32_t)(key2 >> 9);
            if (e == c2) f[k] = 0;
            if (used[k] && (grp[k] == c1 || grp[k] == c2)) { ++len[k]; grp[k] = c1; }
        }
    }
}

// T.81 K.3 (figure K.3), run by one lane: bits[l] counts the codes of unlimited length l < 64; those above `limit` are folded down
// pair by pair, each pair's prefix taking the place of the deepest shorter code, which moves one level down beside one of the pair
__device__ __forceinline__ void huff_fold_lengths(int* bits, int limit) {
    for (int i = 63; i > limit; --i) {
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) --j;
            if (j == 0) { bits[i] = 0; break; }
            bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
        }
    }
}

// the place of entry e of unlimited length le > 0 among the n entries' lengths cs[] (0: no code), in order of (length, index)
__device__ __forceinline__ int huff_rank(const uint8_t* cs, int n, int le, int e) {
    int rank = 0;
    for (int s = 0; s < n; ++s) {
        const int ls = cs[s];
        rank += (ls && (ls < le || (ls == le && s < e))) ? 1 : 0;
    }
    return rank;
}

// Placement, by a workgroup of kPlaceThreads: the exclusive scan of an image's n piece lengths -> the pieces' offsets; -> their sum
constexpr int kPlaceThreads = 256;
__device__ __forceinline__ unsigned long long place_pieces(const uint32_t* len, uint64_t* off, int n) {
    __shared__ unsigned long long wsum[kPlaceThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long run = 0;
    for (int i0 = 0; i0 < n; i0 += kPlaceThreads) {
        const int i = i0 + tid;
        const unsigned long long mine = i < n ? len[i] : 0ull;
        const unsigned long long incl = wave_scan(mine, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long before = run, all = run;
#pragma unroll
        for (int w = 0; w < kPlaceThreads / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < n) off[i] = before + incl - mine;
        run = all;
        __syncthreads();
    }
    return run;
}

}  // namespace gs360
