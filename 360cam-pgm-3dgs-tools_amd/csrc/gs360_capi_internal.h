// gs360_capi_internal.h -- private to the C-ABI glue (gs360_capi*.hip): error state, options, the context and small shared checks.
// Not installed; the public interface is include/gs360.h.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "gs360_kernels.h"

namespace gs360 {

extern thread_local char g_err[512];     // the calling thread's last error text (defined once, gs360_capi.hip)

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(GS360_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr int kMaxSlots = 16;
constexpr int kEventsPerSlot = 8;
constexpr size_t kSlack = 64;
constexpr double kPi = 3.14159265358979323846;

// context options: name, default, range, environment seed (user switches only); the table is gs360_capi.hip's
enum Opt { kOptLanemap, kOptStage, kOptRing, kOptXcdGroup, kOptEqPersist, kOptTablePersist, kOptLanczosTable, kOptTableRows, kOptColorCube,
           kOptSrcMajor, kOptSrcMajorBx, kOptSrcMajorRows, kOptSrcMajorImages, kOptSrcMajorAdapt, kOptSrcMajorStage, kOptTableStage, kOptTableStageRows,
           kOptTableStageWgs, kOptJpegCountWaves, kOptCount };
struct OptDesc { const char* key; int def, lo, hi; const char* env; };
extern const OptDesc kOpts[kOptCount];

struct Staging {  // per-slot device staging used by the *_host conveniences
    void* d_src = nullptr; size_t src_cap = 0;
    void* d_dst = nullptr; size_t dst_cap = 0;
    void* d_aux = nullptr; size_t aux_cap = 0;
    void* d_maskbits = nullptr; size_t maskbits_cap = 0;   // keep-bit images of one masked equirect launch (<= GS360_MAX_FRAMES frames)
    void* d_fft = nullptr; size_t fft_cap = 0;             // row-pass spectra and partial sums of one frame-FFT launch
    void* d_flow = nullptr; size_t flow_cap = 0;           // resident frame-flow states, batch work areas and pair points
    void* d_jpeg = nullptr; size_t jpeg_cap = 0;           // coefficients, quantiser table and interval records of one JPEG batch
    void* d_png = nullptr; size_t png_cap = 0;             // filtered streams and chunk records of one PNG batch
};

}  // namespace gs360

struct gs360_ctx {
    int device = 0;
    int n_slots = 0;
    hipStream_t stream[gs360::kMaxSlots] = {};
    hipEvent_t event[gs360::kMaxSlots][gs360::kEventsPerSlot] = {};
    gs360::Staging stage[gs360::kMaxSlots];
    hipDeviceProp_t prop;
    int16_t* d_cubic = nullptr;   // 32*32*16 int16 cubic weight table, uploaded at context creation
    int16_t* d_lanczos = nullptr; // 32*32*64 int16 Lanczos4 weight table
    float* d_coef1d = nullptr;    // 448 float32 1-D phase coefficients for the 16-bit (float-weight) samplers
    uint32_t* d_lz_cen = nullptr; // 1024 x 2 dwords: the patched block of every Lanczos4 2-D phase (TableLaunch::lz_cen)
    bool lz_rebuild = false;      // the per-pixel weight rebuild reproduces d_lanczos (checked at context creation)
    // Options (gs360_ctx_set_option; seeded ONCE from the environment by gs360_ctx_create for the documented user switches).  The hot
    // path reads these atomics, never the environment: getenv racing a host thread's putenv is undefined behaviour.
    std::atomic<int> opt[gs360::kOptCount];
    std::atomic<int> last_sm_stage{0};        // read-only "last_srcmajor_stage": 1 = that launch staged its tiles through registers
    std::atomic<int> last_sm_rows{0}, last_sm_images{0};   // read-only "last_srcmajor_rows" / "last_srcmajor_images": tile rows and images per workgroup of that launch
    std::atomic<int> last_sm_box_pct{0};      // read-only option "last_srcmajor_box_pct": tile-box bytes of the last source-major plan in % of its grid cells
    std::atomic<int> last_eq_kernel{-1};      // read-only option "last_eq_kernel": 0 gather, 1 LDS-staged, 2 source-major (which kernel the last equirect call launched)
    std::atomic<int> last_table_kernel{-1};   // read-only option "last_table_kernel": jobs of the last 8-bit table call that took the LDS-staged kernel (-1 none yet)
    std::atomic<int> last_table_slow{0};      // read-only option "last_table_stage_slow_tiles": tiles of those jobs' stage plans without a box (redone from memory)
    // source-major plans of this context (gs360_srcmajor.hip), most recent calls' geometries
    gs360::SmCache sm;
};

namespace gs360 {

inline int opt(const gs360_ctx* c, Opt k) { return c->opt[k].load(std::memory_order_relaxed); }

inline int check_ctx_slot(gs360_ctx* ctx, int slot) {
    if (!ctx) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (slot < 0 || slot >= ctx->n_slots) return fail(GS360_ERR_ARG, "slot %d out of range [0,%d)", slot, ctx->n_slots);
    return 0;
}
inline int check_channels(int C) {
    if (C != 1 && C != 3 && C != 4) return fail(GS360_ERR_ARG, "C must be 1, 3 or 4 (got %d)", C);
    return 0;
}
inline int check_table_interp(int interp) {   // the samplers of the table remap and the fused fisheye path
    if (interp != GS360_INTERP_LINEAR && interp != GS360_INTERP_NEAREST && interp != GS360_INTERP_CUBIC &&
        interp != GS360_INTERP_LANCZOS4)
        return fail(GS360_ERR_UNSUPPORTED, "interp %d not implemented (nearest=0, linear=1, cubic=2, lanczos4=4)", interp);
    return 0;
}

inline int ensure(void** p, size_t* cap, size_t need) {   // grows a slot's staging buffer (contents are not kept)
    if (*cap >= need) return 0;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *cap = 0;
    size_t want = need + need / 4 + kSlack;
    HIP_TRY(hipMalloc(p, want));
    *cap = want - kSlack;
    return 0;
}

inline double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// an offset cursor over a slot's scratch: take() -> where the next piece starts, aligned
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes, size_t align = 1) {
        const size_t start = round_up(at, align);
        at = start + bytes;
        return start;
    }
};

}  // namespace gs360
