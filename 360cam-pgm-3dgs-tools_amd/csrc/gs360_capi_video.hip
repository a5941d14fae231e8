// gs360_capi_video.hip -- C-ABI glue of the decoded-video colour conversion (include/gs360.h, VID-COLOR v1) and of the fisheye-to-pinhole
// views of decoded frames (VID-FISHEYE v1): the plan and the two calls.
#include "gs360_capi_internal.h"
#include "gs360_vidfishsteps.h"

using namespace gs360;

struct gs360_video_plan {
    int device = 0;
    int depth = 0;
    int out_bits = 0;               // 8 or 16: (8, 8), (10, 16) and, for VID-FEED v1, (10, 8)
    int outmax = 0;                 // 255 or 65535, what the encode table was built for
    VcCoef coef{};
    float m[9] = {};
    float* d_tables = nullptr;      // kVcLevels floats of linearised levels, then kVcEnc encode cells
};

// The integer coefficients of DESIGN.md 17.2 for a depth and range; tests/vidcolor_np.py derives the same numbers.
static VcCoef video_coefficients(int depth, int full_range) {
    const double Kr = 0.2126, Kb = 0.0722, Kg = 1.0 - Kr - Kb;
    const double scale = 16383.0 * 16384.0;
    const int s = 1 << (depth - 8), vmax = (1 << depth) - 1;
    const double dy = full_range ? (double)vmax : 219.0 * s, dc = full_range ? (double)vmax : 224.0 * s;
    VcCoef K;
    K.cy = (int32_t)std::nearbyint(scale / dy);
    K.crv = (int32_t)std::nearbyint((2.0 * (1.0 - Kr)) * scale / dc);
    K.cgu = (int32_t)std::nearbyint((Kb * (2.0 * (1.0 - Kb)) / Kg) * scale / dc);
    K.cgv = (int32_t)std::nearbyint((Kr * (2.0 * (1.0 - Kr)) / Kg) * scale / dc);
    K.cbu = (int32_t)std::nearbyint((2.0 * (1.0 - Kb)) * scale / dc);
    K.yoff = full_range ? 0 : 16 * s;
    K.coff = 128 * s;
    K.vmax = vmax;
    return K;
}

int gs360_video_plan_create(gs360_ctx* c, int depth, int full_range, int keep_rec709, const float* primaries, const float* linear,
                            const float* encode, gs360_video_plan** out) {
    return gs360_video_plan_create_out(c, depth, depth == 8 ? 8 : 16, full_range, keep_rec709, primaries, linear, encode, out);
}

int gs360_video_plan_create_out(gs360_ctx* c, int depth, int out_bits, int full_range, int keep_rec709, const float* primaries,
                                const float* linear, const float* encode, gs360_video_plan** out) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!primaries || !linear || !encode || !out) return fail(GS360_ERR_ARG, "NULL argument");
    if (depth != 8 && depth != 10) return fail(GS360_ERR_UNSUPPORTED, "video depth %d (8 and 10 bits are implemented)", depth);
    if (!((out_bits == 8) || (out_bits == 16 && depth == 10)))
        return fail(GS360_ERR_UNSUPPORTED, "%d-bit RGB from %d-bit planes (8 from 8, 16 from 10 and 8 from 10 are implemented)", out_bits, depth);
    if ((full_range | keep_rec709) & ~1) return fail(GS360_ERR_ARG, "full_range and keep_rec709 are 0 or 1");
    // the tables index each other: a linear value outside [0,1] or a matrix entry that is no number would leave the encode table
    const float outmax = out_bits == 8 ? 255.0f : 65535.0f;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(primaries[i])) return fail(GS360_ERR_ARG, "primaries[%d] is not finite", i);
    for (int i = 0; i < kVcLevels; ++i)
        if (!(linear[i] >= 0.0f && linear[i] <= 1.0f)) return fail(GS360_ERR_ARG, "linear[%d] outside [0,1]", i);
    for (int i = 0; i < kVcEnc; ++i) {
        const float lo = encode[2 * i], hi = lo + encode[2 * i + 1];
        if (!(lo >= 0.0f && lo <= outmax && hi >= 0.0f && hi <= outmax))
            return fail(GS360_ERR_ARG, "encode cell %d leaves [0,%d]", i, (int)outmax);
    }
    HIP_TRY(hipSetDevice(c->device));
    gs360_video_plan* p = new (std::nothrow) gs360_video_plan();
    if (!p) return fail(GS360_ERR_NOMEM, "out of host memory");
    p->device = c->device;
    p->depth = depth;
    p->out_bits = out_bits;
    p->outmax = (int)outmax;
    p->coef = video_coefficients(depth, full_range);
    std::memcpy(p->m, primaries, sizeof(p->m));
    const size_t n_lin = kVcLevels * sizeof(float), n_enc = kVcEnc * 2 * sizeof(float);
    hipError_t e = hipMalloc((void**)&p->d_tables, n_lin + n_enc);
    if (e == hipSuccess) e = hipMemcpy(p->d_tables, linear, n_lin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_tables + kVcLevels, encode, n_enc, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p->d_tables) (void)hipFree(p->d_tables);
        delete p;
        return fail(e == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "video plan setup failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return GS360_OK;
}

int gs360_video_plan_destroy(gs360_ctx* c, gs360_video_plan* p) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!p) return GS360_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    const hipError_t e = hipFree(p->d_tables);
    delete p;
    HIP_TRY(e);
    return GS360_OK;
}

// One job's checks and its VcImage, for a destination of dst_w pixels a row: sides, subsampling, strides (0 = tight) and, on whichever
// side has 16-bit samples, even addresses and strides.  src_bits / dst_bits: the planes' and the destination's pointers and strides
// OR'ed together.
static int video_job_image(const gs360_video_job& J, int j, const gs360_video_plan& P, int dst_w, VcImage& I, uintptr_t& src_bits,
                           uintptr_t& dst_bits) {
    const size_t bytes = P.depth == 8 ? 1 : 2, dbytes = P.out_bits == 8 ? 1 : 2;
    if (!J.y || !J.cb || !J.cr || !J.dst) return fail(GS360_ERR_ARG, "job %d: NULL plane or destination", j);
    if (J.W < 1 || J.H < 1 || J.W > 65535 || J.H > 65535) return fail(GS360_ERR_ARG, "job %d: size %d x %d outside 1..65535", j, J.W, J.H);
    if (J.subsampling != GS360_VIDEO_444 && J.subsampling != GS360_VIDEO_422 && J.subsampling != GS360_VIDEO_420)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: subsampling %d (4:4:4, 4:2:2 and 4:2:0 are implemented)", j, J.subsampling);
    I.sx = J.subsampling != GS360_VIDEO_444;
    I.sy = J.subsampling == GS360_VIDEO_420;
    const size_t y_row = (size_t)J.W * bytes, c_row = (size_t)((J.W + I.sx) >> I.sx) * bytes, d_row = 3 * (size_t)dst_w * dbytes;
    const size_t ys = J.y_stride ? J.y_stride : y_row, cbs = J.cb_stride ? J.cb_stride : c_row;
    const size_t crs = J.cr_stride ? J.cr_stride : c_row, ds = J.dst_stride ? J.dst_stride : d_row;
    if (ys < y_row || cbs < c_row || crs < c_row || ds < d_row) return fail(GS360_ERR_ARG, "job %d: stride smaller than a row", j);
    src_bits = (uintptr_t)J.y | (uintptr_t)J.cb | (uintptr_t)J.cr | ys | cbs | crs;
    dst_bits = (uintptr_t)J.dst | ds;
    if (bytes == 2 && (src_bits & 1)) return fail(GS360_ERR_ARG, "job %d: 10-bit planes need even addresses and strides", j);
    if (dbytes == 2 && (dst_bits & 1)) return fail(GS360_ERR_ARG, "job %d: a 16-bit destination needs an even address and stride", j);
    I.y = (const uint8_t*)J.y; I.cb = (const uint8_t*)J.cb; I.cr = (const uint8_t*)J.cr; I.dst = (uint8_t*)J.dst;
    I.ys = (int64_t)ys; I.cbs = (int64_t)cbs; I.crs = (int64_t)crs; I.ds = (int64_t)ds;
    I.W = J.W; I.H = J.H;
    return GS360_OK;
}

int gs360_video_rgb(gs360_ctx* c, const gs360_video_plan* p, const gs360_video_job* jobs, int n_jobs, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!p || (n_jobs > 0 && !jobs)) return fail(GS360_ERR_ARG, "NULL argument");
    if (p->device != c->device) return fail(GS360_ERR_ARG, "video plan belongs to device %d, ctx is device %d", p->device, c->device);
    if (n_jobs < 0 || n_jobs > GS360_MAX_FRAMES) return fail(GS360_ERR_ARG, "n_jobs %d outside [0,%d]", n_jobs, GS360_MAX_FRAMES);
    if (n_jobs == 0) return GS360_OK;
    VidLaunch L{};
    for (int j = 0; j < n_jobs; ++j) {                       // every job is checked before anything is launched
        uintptr_t src_bits = 0, dst_bits = 0;
        if (int rc = video_job_image(jobs[j], j, *p, jobs[j].W, L.img[j], src_bits, dst_bits)) return rc;
        L.img[j].fast = ((src_bits | dst_bits) & 3) == 0;
        L.img[j].gpr = (jobs[j].W + kVcGroup - 1) / kVcGroup;
    }
    L.lin = p->d_tables;
    L.enc = reinterpret_cast<const float2*>(p->d_tables + kVcLevels);
    std::memcpy(L.m, p->m, sizeof(L.m));
    L.outmax = p->outmax;
    L.coef = p->coef;
    L.n_jobs = n_jobs;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_vidcolor(L, p->depth, p->out_bits, c->stream[slot]));
    return GS360_OK;
}

// the float32 constants of a view, each a float64 expression rounded once; tests/vidfisheye_np.py derives the same.
static VfView fisheye_constants(const gs360_video_fisheye_view& v) {
    const double rad = M_PI / 180.0;
    const double W = (double)v.W, H = (double)v.H;
    double kx, ky;
    if (v.projection == GS360_FISHEYE_EQUISOLID) {
        const double s = std::sin(v.input_fov_deg * rad / 4.0);
        kx = (W / 2.0) / s; ky = (H / 2.0) / s;
    } else {
        kx = W / (v.input_fov_deg * rad); ky = H / (v.input_fov_deg * rad);
    }
    VfView V;
    V.proj = v.projection == GS360_FISHEYE_EQUISOLID ? kVfEquisolid : kVfEquidistant;
    V.S = v.size;
    V.tx = (float)(std::tan(v.h_fov_deg * rad / 2.0) / (double)v.size);
    V.ty = (float)(std::tan(v.v_fov_deg * rad / 2.0) / (double)v.size);
    V.kx32 = (float)(32.0 * kx); V.ky32 = (float)(32.0 * ky);
    V.kx16 = (float)(16.0 * kx); V.ky16 = (float)(16.0 * ky);
    V.ox32 = (float)(16 * v.W - 16); V.oy32 = (float)(16 * v.H - 16);
    V.ox16 = (float)(8 * v.W - 16); V.oy16 = (float)(8 * v.H - 16);
    return V;
}

int gs360_video_fisheye_rgb(gs360_ctx* c, const gs360_video_plan* p, const gs360_video_fisheye_view* view, const gs360_video_job* jobs,
                            int n_jobs, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!p || !view || (n_jobs > 0 && !jobs)) return fail(GS360_ERR_ARG, "NULL argument");
    if (p->device != c->device) return fail(GS360_ERR_ARG, "video plan belongs to device %d, ctx is device %d", p->device, c->device);
    if (n_jobs < 0 || n_jobs > GS360_MAX_FRAMES) return fail(GS360_ERR_ARG, "n_jobs %d outside [0,%d]", n_jobs, GS360_MAX_FRAMES);
    if (p->out_bits != (p->depth == 8 ? 8 : 16))
        return fail(GS360_ERR_UNSUPPORTED, "fisheye views of a %d-bit plan with %d-bit output are not implemented", p->depth, p->out_bits);
    const gs360_video_fisheye_view& v = *view;
    if (v.projection != GS360_FISHEYE_EQUIDISTANT && v.projection != GS360_FISHEYE_EQUISOLID)
        return fail(GS360_ERR_ARG, "fisheye projection %d (equidistant and equisolid are implemented)", v.projection);
    // 16384: a 1/32-px coordinate stays below 2^19 + 2^4, far inside float32's integers
    if (v.size < 1 || v.size > GS360_FISHEYE_MAX_SIDE) return fail(GS360_ERR_ARG, "view size %d outside 1..%d", v.size, GS360_FISHEYE_MAX_SIDE);
    if (v.W < 1 || v.H < 1 || v.W > GS360_FISHEYE_MAX_SIDE || v.H > GS360_FISHEYE_MAX_SIDE)
        return fail(GS360_ERR_ARG, "source %d x %d outside 1..%d", v.W, v.H, GS360_FISHEYE_MAX_SIDE);
    if (!(v.input_fov_deg >= 1.0 && v.input_fov_deg <= 360.0)) return fail(GS360_ERR_ARG, "input fov %g outside [1,360]", v.input_fov_deg);
    if (!(v.h_fov_deg >= 1.0 && v.h_fov_deg <= 179.0 && v.v_fov_deg >= 1.0 && v.v_fov_deg <= 179.0))
        return fail(GS360_ERR_ARG, "view fov %g x %g outside [1,179]", v.h_fov_deg, v.v_fov_deg);
    if (n_jobs == 0) return GS360_OK;
    VfLaunch L{};
    for (int j = 0; j < n_jobs; ++j) {                       // every job is checked before anything is launched
        uintptr_t src_bits = 0, dst_bits = 0;
        if (int rc = video_job_image(jobs[j], j, *p, v.size, L.img[j], src_bits, dst_bits)) return rc;
        if (jobs[j].W != v.W || jobs[j].H != v.H)
            return fail(GS360_ERR_ARG, "job %d: %d x %d is not the view's source size %d x %d", j, jobs[j].W, jobs[j].H, v.W, v.H);
        L.img[j].fast = (src_bits & 3) == 0;                 // the destination is written sample by sample
    }
    L.lin = p->d_tables;
    L.enc = reinterpret_cast<const float2*>(p->d_tables + kVcLevels);
    std::memcpy(L.m, p->m, sizeof(L.m));
    L.outmax = p->outmax;
    L.coef = p->coef;
    L.view = fisheye_constants(v);
    L.n_jobs = n_jobs;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_vidfisheye(L, p->depth, c->stream[slot]));
    return GS360_OK;
}
