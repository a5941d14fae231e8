// gs360_vidcolor.hip -- VID-COLOR v1 on the GPU (include/gs360.h "decoded video frames"): the planes of up to
// GS360_MAX_FRAMES decoded Y'CbCr frames -> interleaved RGB, what the reference's `colorspace=iall=bt709:all=smpte170m` filter does on
// the host (cli_tools/gs360_Video2Frames.py:464-466).
//
// A streaming kernel: 1.5 to 6 bytes in, 3 to 6 bytes out per pixel.  A lane takes a group of 8 x 2 pixels (gs360_vidsteps.h): per row
// 8 (uint8) or 16 (uint16) bytes of luma and 4 to 16 bytes of chroma come in as whole dwords and 24 or 48 bytes of RGB leave as whole
// dwords; consecutive lanes take consecutive groups of a row, so a wavefront's loads and stores cover contiguous bytes.  The tail of a
// row, and every pixel of a job whose pointers or strides are not multiples of 4, goes sample by sample.  The third instantiation,
// uint16 planes -> uint8 RGB (VID-FEED v1), loads as the 10-bit one does and stores as the 8-bit one does.
//
// Both transfer curves are tables in LDS (64 KiB of linearised levels + 8 KiB of encode cells = 72 KiB: two workgroups per CU), read
// with data-dependent addresses, so bank conflicts are the rule; the workgroups are persistent and load the tables once.
#include "gs360_kernels.h"
#include "gs360_vidsteps.h"

namespace gs360 {

namespace {

constexpr int kVcThreads = 512;
constexpr int kVcBlocks = 512;       // persistent workgroups: 256 CUs x 2

template <typename S, typename D>
__global__ __launch_bounds__(kVcThreads) void vidcolor_kernel(VidLaunch A) {
    __shared__ float lin[kVcLevels];
    __shared__ float2 enc[kVcEnc];
    for (int i = threadIdx.x; i < kVcLevels; i += kVcThreads) lin[i] = A.lin[i];
    for (int i = threadIdx.x; i < kVcEnc; i += kVcThreads) enc[i] = A.enc[i];
    __syncthreads();
    VcTables T;
    T.lin = lin;
    T.enc = enc;
#pragma unroll
    for (int k = 0; k < 9; ++k) T.m[k] = A.m[k];
    T.outmax = A.outmax;
    const uint32_t total = A.tile_end[A.n_jobs - 1];
    int j = 0;
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {
        while (t >= A.tile_end[j]) ++j;                       // tiles are numbered job by job
        const VcImage& I = A.img[j];
        const uint32_t g = (t - (j ? A.tile_end[j - 1] : 0u)) * kVcThreads + threadIdx.x;
        if (g < (uint32_t)I.gpr * (uint32_t)((I.H + 1) >> 1)) vc_group<S, D>(I, A.coef, T, g);
    }
}

}  // namespace

hipError_t launch_vidcolor(VidLaunch& L, int depth, int out_bits, hipStream_t s) {
    uint32_t total = 0;
    for (int j = 0; j < L.n_jobs; ++j) {
        total += (vc_groups(L.img[j]) + kVcThreads - 1) / kVcThreads;
        L.tile_end[j] = total;
    }
    if (total == 0) return hipSuccess;
    const dim3 grid(total < (uint32_t)kVcBlocks ? total : (uint32_t)kVcBlocks), block(kVcThreads);
    if (depth == 8 && out_bits == 8) hipLaunchKernelGGL((vidcolor_kernel<uint8_t, uint8_t>), grid, block, 0, s, L);
    else if (depth == 10 && out_bits == 16) hipLaunchKernelGGL((vidcolor_kernel<uint16_t, uint16_t>), grid, block, 0, s, L);
    else if (depth == 10 && out_bits == 8) hipLaunchKernelGGL((vidcolor_kernel<uint16_t, uint8_t>), grid, block, 0, s, L);
    else return hipErrorInvalidValue;            // plan_create_out makes no other pair
    return hipGetLastError();
}

}  // namespace gs360
