// gs360_capi.hip -- C-ABI glue of libgs360hip.so (include/gs360.h): error text, devices, the context and its options, memory, streams,
// events, the arithmetic self-test; the other entry points by domain in gs360_capi_{equirect,remap,color,codec}.hip.  Host side only: no
// CPU compute path exists on purpose: without a GPU every entry point fails with GS360_ERR_NODEV / GS360_ERR_HIP.
#include <cctype>

#include "gs360_capi_internal.h"

using namespace gs360;

namespace gs360 {
thread_local char g_err[512] = "";

const OptDesc kOpts[kOptCount] = {
    {"lanemap", -1, -1, 1, "GS360_LANEMAP"},          // -1 auto (per view, by minification), 0 rows, 1 blocked       (env: rows | blocked)
    {"stage", -1, -1, 1, "GS360_STAGE"},              // LDS-staged kernel: -1 auto, 0 never, 1 every call that can
    {"ring", 0, 0, GS360_MAX_VIEWS, nullptr},         // 0 auto; n: at most n views share a coordinate evaluation
    {"xcd_group", -2, -2, 12, nullptr},               // -2 auto; -1 contiguous chunks; g: runs of 2^g tiles
    {"eq_persist", 0, 0, 1 << 20, nullptr},           // grid cap of the cubic equirect kernels (0: one tile per workgroup)
    {"table_persist", -1, -1, 1 << 20, nullptr},      // -1 auto; grid cap of the bicubic table / fisheye kernels
    {"lanczos_table", 0, 0, 1, nullptr},              // 1: read the 128 KiB Lanczos-4 table instead of rebuilding weights per pixel
    {"table_rows", 0, 0, 1, nullptr},                 // 1: table kernel in row form even for tight outputs (A/B of the flat spans)
    {"color_cube", -1, -1, 1, "GS360_COLOR_CUBE"},    // -1 / 1: tabulate the 8-bit colour stage (64 MiB per plan); 0: evaluate per pixel
    {"srcmajor", -1, -1, 1, "GS360_SRCMAJOR"},        // source-major kernel: -1 auto (strongly minified level rings), 0 never, 1 whenever eligible
    {"srcmajor_bx", 768, 256, 4032, nullptr},         // its tile: bytes per box row (multiple of 16) ...
    {"srcmajor_rows", 32, 8, 128, nullptr},           // ... and source rows
    {"srcmajor_images", 0, 0, 12, nullptr},           // images of a tile one workgroup walks (0 auto; must divide twice the ring size)
    {"srcmajor_adapt", 1, 0, 1, nullptr},             // 1: jobs that do not fill the GPU take tiles of half the height; 0: srcmajor_rows as given (probes)
    {"srcmajor_stage", 0, 0, 1, nullptr},             // 0: a loader wavefront copies tiles with global_load_lds; 1: the consumers stage them through registers
    {"table_stage", -1, -1, 1, "GS360_TABLE_STAGE"},  // LDS-staged table kernel (bilinear RGB through map plans): -1 auto, 0 never, 1 every job that can
    {"table_stage_rows", 32, 8, 32, nullptr},         // its output tile: rows (multiple of 8) of 64 pixels
    {"table_stage_wgs", 0, 0, 4, nullptr},            // workgroups per CU (0 auto: what the LDS holds, at most three)
    {"jpeg_count_waves", 256, 1, 65535, nullptr},     // optimal Huffman tables: wavefronts that share the count pass of one image
};

}  // namespace gs360

int gs360_abi_version(void) { return GS360_ABI_VERSION; }

int gs360_last_error(char* buf, size_t n) {
    size_t len = std::strlen(g_err);
    if (buf && n) {
        size_t c = len < n - 1 ? len : n - 1;
        std::memcpy(buf, g_err, c);
        buf[c] = 0;
    }
    return (int)len;
}

int gs360_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        fail(GS360_ERR_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
        return 0;
    }
    return n;
}

int gs360_ctx_create(int device, int n_slots, gs360_ctx** out) {
    if (!out) return fail(GS360_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n_slots < 1 || n_slots > kMaxSlots) return fail(GS360_ERR_ARG, "n_slots must be in [1,%d]", kMaxSlots);
    int n = gs360_device_count();
    if (n <= 0) return fail(GS360_ERR_NODEV, "no HIP device visible (libgs360hip has no CPU path)");
    if (device < 0 || device >= n) return fail(GS360_ERR_ARG, "device %d out of range [0,%d)", device, n);
    gs360_ctx* c = new (std::nothrow) gs360_ctx();
    if (!c) return fail(GS360_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->n_slots = n_slots;
    for (int k = 0; k < kOptCount; ++k) {
        int v = kOpts[k].def;
        if (kOpts[k].env)
            if (const char* e = std::getenv(kOpts[k].env)) {       // the ONLY place the library reads its switches from the environment
                if (k == kOptLanemap) v = !std::strcmp(e, "rows") ? 0 : (!std::strcmp(e, "blocked") ? 1 : -1);
                else v = std::atoi(e) != 0 ? 1 : 0;
            }
        c->opt[k].store(v, std::memory_order_relaxed);
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&c->prop, device);
    for (int s = 0; s < n_slots && e == hipSuccess; ++s) {
        e = hipStreamCreateWithFlags(&c->stream[s], hipStreamNonBlocking);
        for (int k = 0; k < kEventsPerSlot && e == hipSuccess; ++k) e = hipEventCreate(&c->event[s][k]);
    }
    if (e != hipSuccess) {
        int rc = fail(GS360_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        gs360_ctx_destroy(c);
        return rc;
    }
    if (std::strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
        int rc = fail(GS360_ERR_NODEV, "device %d is %s; this library carries gfx950 code objects only", device,
                      c->prop.gcnArchName);
        gs360_ctx_destroy(c);
        return rc;
    }
    {
        float coef[448];                                  // 1-D phase tables of the 16-bit samplers; [192, 448) Lanczos-4
        build_coef1d(coef);
        std::vector<int16_t> tab(32 * 32 * 16);
        build_cubic_table(tab.data());
        e = hipMalloc((void**)&c->d_cubic, tab.size() * sizeof(int16_t));
        if (e == hipSuccess) e = hipMemcpy(c->d_cubic, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            tab.assign(32 * 32 * 64, 0);
            build_lanczos4_table(tab.data());
            e = hipMalloc((void**)&c->d_lanczos, tab.size() * sizeof(int16_t));
            if (e == hipSuccess) e = hipMemcpy(c->d_lanczos, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice);
            // the Lanczos kernel rebuilds the 2-D weights per pixel from the 1-D table: w = low 16 bits of the float
            // (cy * (cx * 2^15)) + 1.5 * 2^23 (round-to-nearest-even into the mantissa).  That reproduces every table entry except
            // the block [4,5] x [4,5] the sum fix-up patches (shipped per phase: `cen`) and the one saturated entry of phase 0
            // (handled in the kernel) -- verified here for all 1024 phases; on any mismatch the kernel keeps reading the table.
            std::vector<uint32_t> cen(1024 * 2);
            const float* c1 = coef + 192;
            bool rebuilt_ok = true;
            for (int p = 0; p < 1024; ++p) {
                const int16_t* k = tab.data() + p * 64;
                cen[2 * p] = (uint32_t)(uint16_t)k[4 * 8 + 4] | ((uint32_t)(uint16_t)k[4 * 8 + 5] << 16);
                cen[2 * p + 1] = (uint32_t)(uint16_t)k[5 * 8 + 4] | ((uint32_t)(uint16_t)k[5 * 8 + 5] << 16);
                const float* cy = c1 + (p >> 5) * 8;
                const float* cx = c1 + (p & 31) * 8;
                for (int a = 0; a < 8; ++a)
                    for (int b = 0; b < 8; ++b) {
                        if ((a == 4 || a == 5) && (b == 4 || b == 5)) continue;
                        volatile float cx32 = cx[b] * 32768.0f;
                        volatile float m = cy[a] * cx32;
                        volatile float t = m + 12582912.0f;
                        const float tf = t;
                        uint32_t bits;
                        std::memcpy(&bits, &tf, 4);
                        int16_t w = (int16_t)(uint16_t)(bits & 0xffffu);
                        if (p == 0 && a == 3 && b == 3) w = 32767;          // the kernel's phase-0 rule
                        if (w != k[a * 8 + b]) rebuilt_ok = false;
                    }
            }
            c->lz_rebuild = rebuilt_ok;
            if (e == hipSuccess) e = hipMalloc((void**)&c->d_lz_cen, cen.size() * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMemcpy(c->d_lz_cen, cen.data(), cen.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) e = hipMalloc((void**)&c->d_coef1d, sizeof(coef));
        if (e == hipSuccess) e = hipMemcpy(c->d_coef1d, coef, sizeof(coef), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            int rc = fail(GS360_ERR_HIP, "interpolation table upload failed: %s", hipGetErrorString(e));
            gs360_ctx_destroy(c);
            return rc;
        }
    }
    *out = c;
    return GS360_OK;
}

int gs360_ctx_destroy(gs360_ctx* c) {
    if (!c) return GS360_OK;
    (void)hipSetDevice(c->device);
    for (int s = 0; s < c->n_slots; ++s) {
        if (c->stream[s]) (void)hipStreamSynchronize(c->stream[s]);
        for (int k = 0; k < kEventsPerSlot; ++k)
            if (c->event[s][k]) (void)hipEventDestroy(c->event[s][k]);
        for (void* p : {c->stage[s].d_src, c->stage[s].d_dst, c->stage[s].d_aux, c->stage[s].d_maskbits, c->stage[s].d_fft, c->stage[s].d_flow,
                        c->stage[s].d_jpeg, c->stage[s].d_png})
            if (p) (void)hipFree(p);
        if (c->stream[s]) (void)hipStreamDestroy(c->stream[s]);
    }
    for (void* p : {(void*)c->d_cubic, (void*)c->d_lanczos, (void*)c->d_coef1d, (void*)c->d_lz_cen})
        if (p) (void)hipFree(p);
    gs360::sm_cache_destroy(c->sm);
    delete c;
    return GS360_OK;
}

int gs360_ctx_set_option(gs360_ctx* c, const char* key, int value) {
    if (!c || !key) return fail(GS360_ERR_ARG, "NULL argument");
    for (int k = 0; k < kOptCount; ++k)
        if (!std::strcmp(key, kOpts[k].key)) {
            if (value < kOpts[k].lo || value > kOpts[k].hi)
                return fail(GS360_ERR_ARG, "option %s: %d outside [%d, %d]", key, value, kOpts[k].lo, kOpts[k].hi);
            if (k == kOptSrcMajorBx && value % 16) return fail(GS360_ERR_ARG, "option srcmajor_bx must be a multiple of 16");
            if (k == kOptTableStageRows && value % 8) return fail(GS360_ERR_ARG, "option table_stage_rows must be a multiple of 8");
            c->opt[k].store(value, std::memory_order_relaxed);
            return GS360_OK;
        }
    return fail(GS360_ERR_ARG, "unknown option '%s'", key);
}

int gs360_ctx_get_option(gs360_ctx* c, const char* key, int* value) {
    if (!c || !key || !value) return fail(GS360_ERR_ARG, "NULL argument");
    static const struct { const char* key; std::atomic<int> gs360_ctx::*v; } kReadOnly[] = {
        {"last_eq_kernel", &gs360_ctx::last_eq_kernel}, {"last_table_kernel", &gs360_ctx::last_table_kernel},
        {"last_table_stage_slow_tiles", &gs360_ctx::last_table_slow}, {"last_srcmajor_box_pct", &gs360_ctx::last_sm_box_pct},
        {"last_srcmajor_stage", &gs360_ctx::last_sm_stage}, {"last_srcmajor_rows", &gs360_ctx::last_sm_rows},
        {"last_srcmajor_images", &gs360_ctx::last_sm_images}};
    for (const auto& r : kReadOnly)
        if (!std::strcmp(key, r.key)) {
            *value = (c->*r.v).load(std::memory_order_relaxed);
            return GS360_OK;
        }
    if (!std::strcmp(key, "srcmajor_plan_build_us")) {
        std::lock_guard<std::mutex> lock(c->sm.mu);
        *value = (int)std::min<uint64_t>(c->sm.build_us, 0x7fffffffu);
        return GS360_OK;
    }
    if (!std::strcmp(key, "srcmajor_plan_builds") || !std::strcmp(key, "srcmajor_inline_frees") || !std::strcmp(key, "srcmajor_plans")) {
        std::lock_guard<std::mutex> lock(c->sm.mu);
        *value = !std::strcmp(key, "srcmajor_plan_builds") ? (int)c->sm.builds : (!std::strcmp(key, "srcmajor_inline_frees") ? (int)c->sm.inline_frees : (int)c->sm.plans.size());
        return GS360_OK;
    }
    for (int k = 0; k < kOptCount; ++k)
        if (!std::strcmp(key, kOpts[k].key)) {
            *value = opt(c, (Opt)k);
            return GS360_OK;
        }
    return fail(GS360_ERR_ARG, "unknown option '%s'", key);
}

int gs360_device_pci_bus_id(gs360_ctx* c, char* buf, size_t n) {
    if (!c || !buf || n < 16) return fail(GS360_ERR_ARG, "NULL argument or buffer shorter than 16 bytes");
    HIP_TRY(hipDeviceGetPCIBusId(buf, (int)n, c->device));
    return GS360_OK;
}

int gs360_device_info(gs360_ctx* c, char* name, size_t n, int32_t* cu_count, uint64_t* hbm_bytes) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (name && n) {
        // hipDeviceProp_t::name comes back empty on some driver stacks (the MI355X pool's): the amdgpu driver's product_name then
        char product[128] = "";
        std::snprintf(product, sizeof(product), "%s", c->prop.name);
        if (!product[0]) {
            char bus[32] = "", path[96];
            if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), c->device) == hipSuccess) {
                for (char* q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
                std::snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/product_name", bus);
                if (FILE* f = std::fopen(path, "r")) {
                    if (std::fgets(product, (int)sizeof(product), f)) product[std::strcspn(product, "\r\n")] = 0;
                    std::fclose(f);
                }
            }
            (void)hipGetLastError();
        }
        snprintf(name, n, "%s (%s)", product[0] ? product : "AMD GPU", c->prop.gcnArchName);
    }
    if (cu_count) *cu_count = c->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)c->prop.totalGlobalMem;
    return GS360_OK;
}

// ---- memory ------------------------------------------------------------------------------------
int gs360_dev_alloc(gs360_ctx* c, size_t bytes, void** dptr) {
    if (!c || !dptr) return fail(GS360_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const hipError_t e = hipMalloc(dptr, bytes + kSlack);
    if (e == hipErrorOutOfMemory) {               // its own code: a streaming caller (gs360/video.py) retires frames and tries again
        (void)hipGetLastError();
        return fail(GS360_ERR_NOMEM, "out of device memory (%zu bytes)", bytes);
    }
    HIP_TRY(e);
    return GS360_OK;
}
int gs360_dev_free(gs360_ctx* c, void* dptr) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!dptr) return GS360_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipFree(dptr));
    return GS360_OK;
}
int gs360_host_alloc(gs360_ctx* c, size_t bytes, void** hptr) {
    if (!c || !hptr) return fail(GS360_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(hptr, bytes, hipHostMallocDefault));
    return GS360_OK;
}
int gs360_host_free(gs360_ctx* c, void* hptr) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!hptr) return GS360_OK;
    HIP_TRY(hipHostFree(hptr));
    return GS360_OK;
}
int gs360_upload(gs360_ctx* c, void* dst_dev, const void* src_host, size_t bytes, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!dst_dev || !src_host) return fail(GS360_ERR_ARG, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream[slot]));
    return GS360_OK;
}
int gs360_download(gs360_ctx* c, void* dst_host, const void* src_dev, size_t bytes, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!dst_host || !src_dev) return fail(GS360_ERR_ARG, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream[slot]));
    return GS360_OK;
}
int gs360_dev_memset(gs360_ctx* c, void* dst_dev, int value, size_t bytes, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!dst_dev) return fail(GS360_ERR_ARG, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, c->stream[slot]));
    return GS360_OK;
}
int gs360_dev_bswap16(gs360_ctx* c, void* buf_dev, size_t n_samples, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!buf_dev || ((uintptr_t)buf_dev & 1)) return fail(GS360_ERR_ARG, "NULL or odd buffer address");
    if (n_samples == 0) return GS360_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_bswap16((uint16_t*)buf_dev, n_samples, c->stream[slot]));
    return GS360_OK;
}
int gs360_sync(gs360_ctx* c, int slot) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0) {
        for (int s = 0; s < c->n_slots; ++s) HIP_TRY(hipStreamSynchronize(c->stream[s]));
        gs360::sm_cache_drain(c->sm);             // every stream is idle: plans the cache evicted since the last time are released here
        return GS360_OK;
    }
    if (int rc = check_ctx_slot(c, slot)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream[slot]));
    return GS360_OK;
}

// ---- timing ------------------------------------------------------------------------------------
int gs360_event_record(gs360_ctx* c, int slot, int idx) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (idx < 0 || idx >= kEventsPerSlot) return fail(GS360_ERR_ARG, "event index %d out of range", idx);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->event[slot][idx], c->stream[slot]));
    return GS360_OK;
}
int gs360_event_elapsed_ms(gs360_ctx* c, int slot, int from, int to, float* ms) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!ms || from < 0 || to < 0 || from >= kEventsPerSlot || to >= kEventsPerSlot)
        return fail(GS360_ERR_ARG, "bad event arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->event[slot][to]));
    HIP_TRY(hipEventElapsedTime(ms, c->event[slot][from], c->event[slot][to]));
    return GS360_OK;
}

int gs360_event_sync(gs360_ctx* c, int slot, int idx) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (idx < 0 || idx >= kEventsPerSlot) return fail(GS360_ERR_ARG, "bad event index");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->event[slot][idx]));
    return GS360_OK;
}
int gs360_stream_wait_event(gs360_ctx* c, int waiting_slot, int event_slot, int idx) {
    if (int rc = check_ctx_slot(c, waiting_slot)) return rc;
    if (int rc = check_ctx_slot(c, event_slot)) return rc;
    if (idx < 0 || idx >= kEventsPerSlot) return fail(GS360_ERR_ARG, "bad event index");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamWaitEvent(c->stream[waiting_slot], c->event[event_slot][idx], 0));
    return GS360_OK;
}

// Self-test: the kernels replace `/` and sqrtf by shorter instruction sequences that are bit-identical on the operand domains
// of EQ-SPEC / FE-SPEC (gs360_eqspec.h).  This runs both forms on `n_millions` x 10^6 pseudo-random operand sets per form.
int gs360_selftest_arith(gs360_ctx* c, uint32_t seed, int n_millions, uint64_t* n_checked, uint64_t* n_mismatch) {
    if (int rc = check_ctx_slot(c, 0)) return rc;
    if (!n_checked || !n_mismatch || n_millions < 1 || n_millions > 100000) return fail(GS360_ERR_ARG, "bad self-test arguments");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long* d_bad = nullptr;
    HIP_TRY(hipMalloc((void**)&d_bad, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), c->stream[0]);
    const int iters = 1000, blocks = (int)(((long long)n_millions * 1000000 + 256LL * iters - 1) / (256LL * iters));
    if (e == hipSuccess) e = launch_arith_selftest(seed, blocks, iters, d_bad, c->stream[0]);
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream[0]);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return fail(GS360_ERR_HIP, "arithmetic self-test failed to run: %s", hipGetErrorString(e));
    *n_checked = (uint64_t)blocks * 256ull * (uint64_t)iters;
    *n_mismatch = bad;
    return GS360_OK;
}
