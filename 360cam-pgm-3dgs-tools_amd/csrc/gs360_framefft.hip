// gs360_framefft.hip -- the FFT sharpness energy of the FrameSelector's fft / hybrid metrics on the GPU (include/gs360.h,
// "frame FFT energy"; FS-FFT v1 in DESIGN.md).
//
// Reference: fft_energy_fast, cli_tools/gs360_FrameSelector.py:742-786, after its resize: |fftshift(fft2(g))| over a donut around
// the centre, averaged over the resized valid mask.  Both sides of g are <= 512 and arbitrary (512 x 204, 512 x 409 with 409
// prime), so the 2-D DFT is evaluated as two matrix products on the real input instead of a radix FFT:
//   row pass     X[y,k] = sum_j g[y,j] e^{-2 pi i jk/w}     for the w/2+1 Hermitian columns k      (ff_rows_kernel)
//   column pass  F[u,k] = sum_y e^{-2 pi i uy/h} X[y,k]                                            (ff_cols_kernel)
// fused with |F|, the donut, the valid mask and a per-workgroup partial sum; |F(-u,-k)| = |F(u,k)| credits the mirrored
// position of every column except the self-mirrored k = 0 and, for even w, k = w/2.  ff_final_kernel adds the partials of a frame
// in a fixed order.  Every sum is float32 in a fixed order (products) or double in a fixed order (means, magnitudes), so a call
// is bit-reproducible; no float atomics.
//
// DC removal: twiddles rounded to float32 leak the DC term into every bin (a constant image would read ~1e-4 instead of 0).  The
// row pass transforms g - mean(row) for k != 0 and takes X[y,0] = the row's sum; the column pass does the same with the column
// means of X for u != 0.  Both are exact rewrites in real arithmetic (sum_j e^{-2 pi i jk/w} = 0 for k != 0 mod w).
//
// Both passes are LDS-tiled float32 GEMMs on the vector ALUs: 64 x 64 outputs per 256-thread workgroup, 4 x 4 per thread, the inner
// dimension in chunks of kFfKc.  Twiddle tiles are built in LDS from a per-workgroup table of cos / sin(2 pi m/N) (double sincospi,
// rounded to float), indexed by (j*k) mod N, which each thread advances by (kFfKc*k) mod N per chunk.
#include "gs360_framepx.h"

namespace gs360 {

namespace {

constexpr int kFfThreads = 256;
constexpr int kFfTile = 64;                    // output rows x columns per workgroup
constexpr int kFfKc = 16;                      // inner-dimension chunk
constexpr int kFfPitch = kFfTile + 4;          // LDS row pitch (floats): float4 reads stay 16-byte aligned

__device__ __forceinline__ void build_table(float2* tab, int N) {
    for (int m = threadIdx.x; m < N; m += kFfThreads) {
        double s, c;
        sincospi(2.0 * m / N, &s, &c);
        tab[m] = make_float2((float)c, (float)s);
    }
}

// Row pass: X = (g - row mean) . [C_w | -S_w], column 0 = the row sums.  Grid (k tiles, row tiles, frames).
__global__ void __launch_bounds__(kFfThreads) ff_rows_kernel(const FfLaunch L) {
    __shared__ float2 tab[GS360_FFT_MAX_SIDE];
    __shared__ double mean[kFfTile];
    __shared__ double rsum[kFfTile];
    __shared__ __attribute__((aligned(16))) float As[kFfKc][kFfPitch];
    __shared__ __attribute__((aligned(16))) float Bc[kFfKc][kFfPitch];
    __shared__ __attribute__((aligned(16))) float Bs[kFfKc][kFfPitch];
    const int h = L.h, w = L.w, K = L.K;
    const int k0 = blockIdx.x * kFfTile, y0 = blockIdx.y * kFfTile, f = blockIdx.z;
    const float* const g = L.small[f];
    const int tid = threadIdx.x;
    build_table(tab, w);
    {   // row sums in double: four lanes per row, strided, combined by two butterfly steps (fixed order)
        const int r = tid >> 2, q = tid & 3, y = y0 + r;
        double s = 0.0;
        if (y < h)
            for (int j = q; j < w; j += 4) s += (double)g[(int64_t)y * w + j];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (q == 0) { rsum[r] = s; mean[r] = s / w; }
    }
    // this thread's twiddle-tile elements: (jj, kk) = (tid / 64 + 4 e, tid % 64), index (j*k) mod w
    const int kk_b = tid & 63, k_b = k0 + kk_b;
    const int step = (int)(((int64_t)kFfKc * k_b) % w);
    int m[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = (int)(((int64_t)((tid >> 6) + 4 * e) * k_b) % w);
    const int ty = tid >> 4, tx = tid & 15;
    float ar[4][4] = {}, ai[4][4] = {};
    __syncthreads();
    for (int j0 = 0; j0 < w; j0 += kFfKc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // A: 16 consecutive j of one row per 16 lanes
            const int i = tid + kFfThreads * e, jj = i & 15, yy = i >> 4, j = j0 + jj, y = y0 + yy;
            As[jj][yy] = (j < w && y < h) ? (float)((double)g[(int64_t)y * w + j] - mean[yy]) : 0.0f;
            const float2 t = tab[m[e]];
            Bc[(tid >> 6) + 4 * e][kk_b] = t.x;
            Bs[(tid >> 6) + 4 * e][kk_b] = t.y;
            m[e] += step;
            if (m[e] >= w) m[e] -= w;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kFfKc; ++kk) {
            const float4 a = *(const float4*)&As[kk][ty * 4];
            const float4 c = *(const float4*)&Bc[kk][tx * 4];
            const float4 s = *(const float4*)&Bs[kk][tx * 4];
            const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w}, sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jx = 0; jx < 4; ++jx) {
                    ar[i][jx] += av[i] * cv[jx];
                    ai[i][jx] -= av[i] * sv[jx];
                }
        }
        __syncthreads();
    }
    float* const xr = L.x[f];
    float* const xi = xr + (int64_t)h * K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = ty * 4 + i, y = y0 + yy;
        if (y >= h) continue;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int k = k0 + tx * 4 + jx;
            if (k >= K) continue;
            xr[(int64_t)y * K + k] = k == 0 ? (float)rsum[yy] : ar[i][jx];
            xi[(int64_t)y * K + k] = k == 0 ? 0.0f : ai[i][jx];
        }
    }
}

// Column pass + |F|, donut, mask and this workgroup's partial sums.  Grid (k tiles, u tiles, frames).
__global__ void __launch_bounds__(kFfThreads) ff_cols_kernel(const FfLaunch L) {
    __shared__ float2 tab[GS360_FFT_MAX_SIDE];
    __shared__ double csum[2][4][kFfTile];       // column sums of X: re / im, four row phases
    __shared__ double mean[2][kFfTile];
    __shared__ __attribute__((aligned(16))) float Ac[kFfKc][kFfPitch];
    __shared__ __attribute__((aligned(16))) float As[kFfKc][kFfPitch];
    __shared__ __attribute__((aligned(16))) float Br[kFfKc][kFfPitch];
    __shared__ __attribute__((aligned(16))) float Bi[kFfKc][kFfPitch];
    __shared__ double red_d[2][kFfThreads / 64];
    __shared__ long long red_n[kFfThreads / 64];
    const int h = L.h, w = L.w, K = L.K;
    const int k0 = blockIdx.x * kFfTile, u0 = blockIdx.y * kFfTile, f = blockIdx.z;
    const float* const xr = L.x[f];
    const float* const xi = xr + (int64_t)h * K;
    const int tid = threadIdx.x;
    build_table(tab, h);
    {   // column sums in double: column tid % 64, rows tid / 64 + 4 q (coalesced along k); the four phases added in order below
        const int c = tid & 63, p = tid >> 6, k = k0 + c;
        double sr = 0.0, si = 0.0;
        if (k < K)
            for (int y = p; y < h; y += 4) {
                sr += (double)xr[(int64_t)y * K + k];
                si += (double)xi[(int64_t)y * K + k];
            }
        csum[0][p][c] = sr;
        csum[1][p][c] = si;
    }
    __syncthreads();
    if (tid < 2 * kFfTile) {
        const int part = tid >> 6, c = tid & 63;
        const double s = ((csum[part][0][c] + csum[part][1][c]) + csum[part][2][c]) + csum[part][3][c];
        csum[part][0][c] = s;
        mean[part][c] = s / h;
    }
    // this thread's twiddle-tile elements: (yy, uu) = (tid / 64 + 4 e, tid % 64), index (u*y) mod h
    const int uu_a = tid & 63, u_a = u0 + uu_a;
    const int step = (int)(((int64_t)kFfKc * u_a) % h);
    int m[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = (int)(((int64_t)((tid >> 6) + 4 * e) * u_a) % h);
    const int ty = tid >> 4, tx = tid & 15;
    float fr[4][4] = {}, fi[4][4] = {};
    __syncthreads();
    for (int yb = 0; yb < h; yb += kFfKc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int yy = (tid >> 6) + 4 * e, y = yb + yy, k = k0 + uu_a;
            const float2 t = tab[m[e]];
            Ac[yy][uu_a] = t.x;
            As[yy][uu_a] = t.y;
            m[e] += step;
            if (m[e] >= h) m[e] -= h;
            const bool in = y < h && k < K;
            Br[yy][uu_a] = in ? (float)((double)xr[(int64_t)y * K + k] - mean[0][uu_a]) : 0.0f;
            Bi[yy][uu_a] = in ? (float)((double)xi[(int64_t)y * K + k] - mean[1][uu_a]) : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kFfKc; ++kk) {
            const float4 c = *(const float4*)&Ac[kk][ty * 4];
            const float4 s = *(const float4*)&As[kk][ty * 4];
            const float4 r = *(const float4*)&Br[kk][tx * 4];
            const float4 q = *(const float4*)&Bi[kk][tx * 4];
            const float cv[4] = {c.x, c.y, c.z, c.w}, sv[4] = {s.x, s.y, s.z, s.w};
            const float rv[4] = {r.x, r.y, r.z, r.w}, qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jx = 0; jx < 4; ++jx) {   // (c - i s)(r + i q)
                    fr[i][jx] += cv[i] * rv[jx];
                    fr[i][jx] += sv[i] * qv[jx];
                    fi[i][jx] += cv[i] * qv[jx];
                    fi[i][jx] -= sv[i] * rv[jx];
                }
        }
        __syncthreads();
    }
    // epilogue: credit every computed bin, and its mirror, at its fftshift position (i, j)
    const int hc = h / 2, wc = w / 2;
    const int rd = max(1, min(h, w) / 8);
    const int64_t r4 = circle_r4(L.W, L.H);
    const int bh = L.y1 - L.y0;
    const float* const near = L.small[f] + (int64_t)h * w;
    double s_hf = 0.0, s_hfv = 0.0;
    long long n_v = 0;
    auto credit = [&](int u, int k, float mag) {
        const int i = u + hc < h ? u + hc : u + hc - h;
        const int j = k + wc < w ? k + wc : k + wc - w;
        const bool donut = (i - hc) * (i - hc) + (j - wc) * (j - wc) >= rd * rd;
        bool valid = true;
        if (L.circle) {   // the full-frame circle at INTER_NEAREST's sample (xs[j], ys[i])
            const int64_t x = nearest_index(j, L.scale_x, L.W);
            const int64_t y = L.y0 + nearest_index(i, L.scale_y, bh);
            const int64_t dx = 2 * x - (L.W - 1), dy = 2 * y - (L.H - 1);
            valid = dx * dx + dy * dy <= r4;
        }
        if (L.highlights) valid = valid && near[(int64_t)i * w + j] < 243.0f;
        if (donut) s_hf += (double)mag;
        if (donut && valid) s_hfv += (double)mag;
        n_v += valid;
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = u0 + ty * 4 + i;
        if (u >= h) continue;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int k = k0 + tx * 4 + jx;
            if (k >= K) continue;
            const float re = u == 0 ? (float)csum[0][0][tx * 4 + jx] : fr[i][jx];
            const float im = u == 0 ? (float)csum[1][0][tx * 4 + jx] : fi[i][jx];
            const float mag = sqrtf(re * re + im * im);
            credit(u, k, mag);
            if (k != 0 && 2 * k != w) credit(u == 0 ? 0 : h - u, w - k, mag);
        }
    }
    s_hf = wave_sum(s_hf);
    s_hfv = wave_sum(s_hfv);
    n_v = wave_sum(n_v);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red_d[0][wave] = s_hf; red_d[1][wave] = s_hfv; red_n[wave] = n_v; }
    __syncthreads();
    if (tid == 0) {
        FfPartial P;
        P.sum_hf = ((red_d[0][0] + red_d[0][1]) + red_d[0][2]) + red_d[0][3];
        P.sum_hf_valid = ((red_d[1][0] + red_d[1][1]) + red_d[1][2]) + red_d[1][3];
        P.n_valid = red_n[0] + red_n[1] + red_n[2] + red_n[3];
        L.part[(int64_t)f * L.n_part + blockIdx.y * gridDim.x + blockIdx.x] = P;
    }
}

// A frame's partials, added in workgroup order.  One wavefront per frame.
__global__ void __launch_bounds__(64) ff_final_kernel(const FfLaunch L) {
    const int f = blockIdx.x;
    if (threadIdx.x != 0) return;
    const FfPartial* p = L.part + (int64_t)f * L.n_part;
    gs360_frame_fft r;
    r.sum_hf = 0.0; r.sum_hf_valid = 0.0; r.n_valid = 0;
    for (int b = 0; b < L.n_part; ++b) {
        r.sum_hf += p[b].sum_hf;
        r.sum_hf_valid += p[b].sum_hf_valid;
        r.n_valid += p[b].n_valid;
    }
    r.n = (int64_t)L.h * L.w;
    L.out[f] = r;
}

}  // namespace

hipError_t launch_frame_fft(FfLaunch& L, hipStream_t s) {
    const unsigned kt = (unsigned)((L.K + kFfTile - 1) / kFfTile);
    hipLaunchKernelGGL(ff_rows_kernel, dim3(kt, (unsigned)((L.h + kFfTile - 1) / kFfTile), (unsigned)L.n_frames), dim3(kFfThreads), 0, s, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ff_cols_kernel, dim3(kt, (unsigned)((L.h + kFfTile - 1) / kFfTile), (unsigned)L.n_frames), dim3(kFfThreads), 0, s, L);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ff_final_kernel, dim3((unsigned)L.n_frames), dim3(64), 0, s, L);
    return hipGetLastError();
}

int frame_fft_partials(int h, int w) {
    return ((w / 2 + 1 + kFfTile - 1) / kFfTile) * ((h + kFfTile - 1) / kFfTile);
}

}  // namespace gs360
