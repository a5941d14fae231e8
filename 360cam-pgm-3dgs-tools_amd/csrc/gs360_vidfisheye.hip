// gs360_vidfisheye.hip -- VID-FISHEYE v1 on the GPU (include/gs360.h "decoded fisheye frames"): the planes of up
// to GS360_MAX_FRAMES decoded Y'CbCr fisheye frames -> S x S pinhole views in RGB, what the reference's
// `v360=<fisheye|equisolid>:rectilinear:...:interp=cubic` followed by its colorspace filter does on the host
// (cli_tools/gs360_Video2Frames.py:467-493).  The planes are interpolated, then converted: the order of the reference.
//
// A gather kernel: one output pixel per lane (gs360_vidfishsteps.h), 4 x 4 taps in each of the three planes.  A workgroup of 512
// lanes takes a tile of 32 x 16 output pixels and each of its wavefronts 16 x 4 of them, so that a wavefront's taps fall into a
// compact box of the source.  The four taps of a row come in as 2 (uint8) or 3 (uint16) aligned dwords; a lane whose window touches a
// plane edge, or the end of a row that is no dword multiple, and every lane of a job whose plane pointers or strides are not
// multiples of 4, reads sample by sample with clamped indices.  Nothing outside a plane's rows is read.
//
// Both transfer curves (72 KiB) and the 32 x 4 weights (256 bytes, built here from vf_weights) live in LDS: two workgroups per CU.
// The workgroups are persistent and load the tables once; the tiles of a call are numbered job by job, tile by tile.
#include "gs360_kernels.h"
#include "gs360_vidfishsteps.h"

namespace gs360 {

namespace {

constexpr int kVfThreads = kVfTileW * kVfTileH;          // 512
constexpr int kVfBlocks = 512;                           // persistent workgroups: 256 CUs x 2

template <typename S>
__global__ __launch_bounds__(kVfThreads) void vidfisheye_kernel(VfLaunch A) {
    __shared__ float lin[kVcLevels];
    __shared__ float2 enc[kVcEnc];
    __shared__ int16_t wtab[4 * kVfPhases];
    for (int i = threadIdx.x; i < kVcLevels; i += kVfThreads) lin[i] = A.lin[i];
    for (int i = threadIdx.x; i < kVcEnc; i += kVfThreads) enc[i] = A.enc[i];
    if (threadIdx.x < kVfPhases) vf_weights((int)threadIdx.x, wtab + 4 * threadIdx.x);
    __syncthreads();
    VcTables T;
    T.lin = lin;
    T.enc = enc;
#pragma unroll
    for (int k = 0; k < 9; ++k) T.m[k] = A.m[k];
    T.outmax = A.outmax;
    // lane -> pixel of the tile: wavefront w takes columns 16 (w & 1) .. + 15 of rows 4 (w >> 1) .. + 3
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = (wave & 1) * 16 + (lane & 15), ly = (wave >> 1) * 4 + (lane >> 4);
    const uint32_t per_job = (uint32_t)A.tiles_x * (uint32_t)A.tiles_y, total = per_job * (uint32_t)A.n_jobs;
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {
        const uint32_t job = t / per_job, tile = t - job * per_job;
        const uint32_t tyi = tile / (uint32_t)A.tiles_x, txi = tile - tyi * (uint32_t)A.tiles_x;
        const int i = (int)txi * kVfTileW + lx, j = (int)tyi * kVfTileH + ly;
        if (i < A.view.S && j < A.view.S) vf_pixel<S>(A.img[job], A.view, A.coef, T, wtab, i, j);
    }
}

}  // namespace

hipError_t launch_vidfisheye(VfLaunch& L, int depth, hipStream_t s) {
    L.tiles_x = (L.view.S + kVfTileW - 1) / kVfTileW;
    L.tiles_y = (L.view.S + kVfTileH - 1) / kVfTileH;
    const uint32_t total = (uint32_t)L.tiles_x * (uint32_t)L.tiles_y * (uint32_t)L.n_jobs;   // at most 512 * 1024 * 16
    if (total == 0) return hipSuccess;
    const dim3 grid(total < (uint32_t)kVfBlocks ? total : (uint32_t)kVfBlocks), block(kVfThreads);
    if (depth == 8) hipLaunchKernelGGL((vidfisheye_kernel<uint8_t>), grid, block, 0, s, L);
    else hipLaunchKernelGGL((vidfisheye_kernel<uint16_t>), grid, block, 0, s, L);
    return hipGetLastError();
}

}  // namespace gs360
