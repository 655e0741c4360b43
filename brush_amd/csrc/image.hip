// image.hip — the resampling of the reference's LoadImage::load (brush-dataset/src/load_image.rs:60-131): image::imageops::resize
// of the image crate 0.25 (a vertical pass into an f32 intermediate, a horizontal pass back to u8), the mask merge, and the
// standalone operator bh_resize_u8.  DESIGN.md §6h has the contract; tests/image_ref.py restates it in numpy.
//
// Exactness: the weights are computed on the HOST, in f32 with the C library's sinf (what Rust's f32::sin lowers to on Linux), and
// uploaded with the launch; the kernels only gather, multiply and add (-ffp-contract=off keeps t = t + v * w two roundings), so
// the bytes equal the reference's.
//
// MI355X shape: both passes are memory-bound.  The vertical pass gives every thread one source column of one output row: a wave
// reads 64 adjacent pixels of each tap row (coalesced u8 rows) and the row's weights are block-uniform.  Its intermediate keeps
// the channels the image has (4 / 12 / 16 B per pixel for 1 / 3 / 4 channels, not a fixed RGBA32F).  The horizontal pass gives
// every thread one output pixel of one row; neighbouring lanes read overlapping tap windows of the same intermediate row, which
// the caches serve.  In the upload ring it writes the packed rgba8 of view_to_packed_data directly (premultiplied when asked).
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

#include "context.h"

namespace bh {

constexpr int IMG_WG = 256;
constexpr uint32_t IMG_MAX_GRID_Y = 65535;

// ---- host: the weight table of one pass (sample.rs vertical_sample / horizontal_sample) --------------------------------
// Layout (int32 words): [0] dst  [1] stride (taps of the widest output) | left[dst] | count[dst] | (pad to 4 words) | f32 w[dst][stride]
__host__ __device__ inline size_t table_w_word(uint32_t dst) { return (4 + 2 * (size_t)dst + 3) & ~(size_t)3; }

static float sinc_f32(float t) {
    const float a = t * (float)M_PI;   // std::f32::consts::PI
    return t == 0.0f ? 1.0f : sinf(a) / a;
}
static float filter_kernel(uint32_t filter, float x) {
    if (filter == BH_FILTER_TRIANGLE) return fabsf(x) < 1.0f ? 1.0f - fabsf(x) : 0.0f;
    return fabsf(x) < 3.0f ? sinc_f32(x) * sinc_f32(x / 3.0f) : 0.0f;   // lanczos(x, 3)
}

struct PassGeom {
    float ratio, sratio, src_support;
};
static PassGeom pass_geom(uint32_t src, uint32_t dst, uint32_t filter) {
    PassGeom g;
    g.ratio = (float)src / (float)dst;
    g.sratio = g.ratio < 1.0f ? 1.0f : g.ratio;
    g.src_support = (filter == BH_FILTER_TRIANGLE ? 1.0f : 3.0f) * g.sratio;
    return g;
}
// [left, right) of output o, clamped as sample.rs does
static void pass_span(const PassGeom& g, uint32_t src, uint32_t o, int64_t* left, int64_t* right) {
    const float c = ((float)o + 0.5f) * g.ratio;
    int64_t l = (int64_t)floorf(c - g.src_support);
    l = l < 0 ? 0 : (l > (int64_t)src - 1 ? (int64_t)src - 1 : l);
    int64_t r = (int64_t)ceilf(c + g.src_support);
    r = r < l + 1 ? l + 1 : (r > (int64_t)src ? (int64_t)src : r);
    *left = l;
    *right = r;
}
static uint32_t pass_stride(uint32_t src, uint32_t dst, uint32_t filter) {
    const PassGeom g = pass_geom(src, dst, filter);
    int64_t mx = 1;
    for (uint32_t o = 0; o < dst; ++o) {
        int64_t l, r;
        pass_span(g, src, o, &l, &r);
        mx = r - l > mx ? r - l : mx;
    }
    return (uint32_t)mx;
}

size_t resize_table_bytes(uint32_t src, uint32_t dst, uint32_t filter) {
    return ((table_w_word(dst) + (size_t)dst * pass_stride(src, dst, filter)) * 4 + 15) & ~(size_t)15;
}

void build_resize_table(uint32_t src, uint32_t dst, uint32_t filter, void* host) {
    const PassGeom g = pass_geom(src, dst, filter);
    const uint32_t stride = pass_stride(src, dst, filter);
    int32_t* t = (int32_t*)host;
    std::memset(host, 0, resize_table_bytes(src, dst, filter));
    t[0] = (int32_t)dst;
    t[1] = (int32_t)stride;
    float* w = (float*)(t + table_w_word(dst));
    for (uint32_t o = 0; o < dst; ++o) {
        int64_t l, r;
        pass_span(g, src, o, &l, &r);
        const float c = ((float)o + 0.5f) * g.ratio - 0.5f;
        float* wo = w + (size_t)o * stride;
        float sum = 0.0f;
        for (int64_t i = l; i < r; ++i) {
            const float k = filter_kernel(filter, ((float)i - c) / g.sratio);
            wo[i - l] = k;
            sum += k;
        }
        for (int64_t i = l; i < r; ++i) wo[i - l] /= sum;
        t[4 + o] = (int32_t)l;
        t[4 + dst + o] = (int32_t)(r - l);
    }
}

// Every view of a dataset usually has the same (src, dst) pair, so a table is built once and kept: a small process-wide LRU
// shared by the uploaders and bh_resize_u8.  A miss builds outside the lock (a 4032 -> 1920 Lanczos3 table is ~0.3 ms of sinf).
constexpr size_t TABLE_CACHE_ENTRIES = 16;
struct TableEntry {
    uint32_t src, dst, filter;
    ResizeTable table;
};
static std::mutex g_table_mu;
static std::vector<TableEntry> g_tables;   // most recently used first

ResizeTable resize_table(uint32_t src, uint32_t dst, uint32_t filter) {
    {
        std::lock_guard<std::mutex> lk(g_table_mu);
        for (size_t i = 0; i < g_tables.size(); ++i) {
            if (g_tables[i].src == src && g_tables[i].dst == dst && g_tables[i].filter == filter) {
                TableEntry e = g_tables[i];
                g_tables.erase(g_tables.begin() + (ptrdiff_t)i);
                g_tables.insert(g_tables.begin(), e);
                return e.table;
            }
        }
    }
    auto t = std::make_shared<std::vector<uint8_t>>(resize_table_bytes(src, dst, filter));
    build_resize_table(src, dst, filter, t->data());
    std::lock_guard<std::mutex> lk(g_table_mu);
    g_tables.insert(g_tables.begin(), TableEntry{src, dst, filter, t});
    if (g_tables.size() > TABLE_CACHE_ENTRIES) g_tables.pop_back();
    return t;
}

// ---- device -----------------------------------------------------------------------------------------------------------
template <int C>
BH_DEV void load_px(const uint8_t* __restrict__ p, float* v) {
    if constexpr (C == 4) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);   // 4-byte aligned: the rows of an RGBA8 image are
        v[0] = (float)(u & 0xFFu); v[1] = (float)((u >> 8) & 0xFFu); v[2] = (float)((u >> 16) & 0xFFu); v[3] = (float)(u >> 24);
    } else {
        #pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (float)p[c];
    }
}

// vertical_sample: tmp[oy][x][c] = sum over the taps of src[left + i][x][c] * w[oy][i], unrounded
template <int C>
__global__ __launch_bounds__(IMG_WG) void resize_vertical_kernel(const uint8_t* __restrict__ src, uint32_t w, const int32_t* __restrict__ tab,
                                                                 uint32_t nh, float* __restrict__ tmp) {
    const uint32_t x = blockIdx.x * IMG_WG + threadIdx.x;
    if (x >= w) return;
    const uint32_t stride = (uint32_t)tab[1];
    const float* __restrict__ wt = reinterpret_cast<const float*>(tab + table_w_word(nh));
    const size_t row = (size_t)w * C;
    for (uint32_t oy = blockIdx.y; oy < nh; oy += gridDim.y) {
        const int32_t left = tab[4 + oy], n = tab[4 + nh + oy];
        const float* __restrict__ wo = wt + (size_t)oy * stride;
        const uint8_t* __restrict__ p = src + (size_t)left * row + (size_t)x * C;
        float t[C];
        #pragma unroll
        for (int c = 0; c < C; ++c) t[c] = 0.0f;
        for (int32_t i = 0; i < n; ++i, p += row) {
            const float wi = wo[i];
            float v[C];
            load_px<C>(p, v);
            #pragma unroll
            for (int c = 0; c < C; ++c) t[c] = t[c] + v[c] * wi;
        }
        float* __restrict__ o = tmp + ((size_t)oy * w + x) * C;
        if constexpr (C == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(t[0], t[1], t[2], t[3]);
        } else {
            #pragma unroll
            for (int c = 0; c < C; ++c) o[c] = t[c];
        }
    }
}

// FloatNearest(clamp(t, 0, 255)) as u8
BH_DEV uint32_t to_u8(float t) { return (uint32_t)roundf(t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t)); }

// horizontal_sample: out[y][ox] from tmp[y][left + i] * w[ox][i].  MODE RESIZE_OUT_*: C bytes, or one packed rgba8 word
// (C == 3: a = 255, scene.rs:111-116; C == 4: as is, or premultiplied as pack_rgba does, scene.rs:124-136)
template <int C, int MODE>
__global__ __launch_bounds__(IMG_WG) void resize_horizontal_kernel(const float* __restrict__ tmp, uint32_t w, const int32_t* __restrict__ tab,
                                                                   uint32_t nw, uint32_t nh, void* __restrict__ out) {
    const uint32_t ox = blockIdx.x * IMG_WG + threadIdx.x;
    if (ox >= nw) return;
    const uint32_t stride = (uint32_t)tab[1];
    const int32_t left = tab[4 + ox], n = tab[4 + nw + ox];
    const float* __restrict__ wo = reinterpret_cast<const float*>(tab + table_w_word(nw)) + (size_t)ox * stride;
    for (uint32_t y = blockIdx.y; y < nh; y += gridDim.y) {
        const float* __restrict__ p = tmp + ((size_t)y * w + left) * C;
        float t[C];
        #pragma unroll
        for (int c = 0; c < C; ++c) t[c] = 0.0f;
        for (int32_t i = 0; i < n; ++i, p += C) {
            const float wi = wo[i];
            float v[C];
            if constexpr (C == 4) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                #pragma unroll
                for (int c = 0; c < C; ++c) v[c] = p[c];
            }
            #pragma unroll
            for (int c = 0; c < C; ++c) t[c] = t[c] + v[c] * wi;
        }
        uint32_t q[C];
        #pragma unroll
        for (int c = 0; c < C; ++c) q[c] = to_u8(t[c]);
        const size_t px = (size_t)y * nw + ox;
        if constexpr (MODE == RESIZE_OUT_U8) {
            uint8_t* o = reinterpret_cast<uint8_t*>(out) + px * C;
            if constexpr (C == 4) {
                *reinterpret_cast<uint32_t*>(o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            } else {
                #pragma unroll
                for (int c = 0; c < C; ++c) o[c] = (uint8_t)q[c];
            }
        } else {
            static_assert(C >= 3, "packed output needs RGB or RGBA");
            uint32_t a = 255u, r = q[0], g = q[1], b = q[2];
            if constexpr (C == 4) {
                a = q[3];
                if constexpr (MODE == RESIZE_OUT_PACKED_PREMUL) {
                    r = (r * a + 127u) / 255u;
                    g = (g * a + 127u) / 255u;
                    b = (b * a + 127u) / 255u;
                }
            }
            reinterpret_cast<uint32_t*>(out)[px] = r | (g << 8) | (b << 16) | (a << 24);
        }
    }
}

// load_image.rs:69-112: the view becomes RGBA with alpha = mask (or 255 - mask); with `premultiply` packed as pack_rgba does
template <int C>
__global__ __launch_bounds__(IMG_WG) void mask_merge_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, uint64_t pixels,
                                                            int invert, int premultiply, uint32_t* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * IMG_WG + threadIdx.x;
    if (p >= pixels) return;
    uint32_t r, g, b;
    if constexpr (C == 4) {
        const uint32_t u = reinterpret_cast<const uint32_t*>(img)[p];
        r = u & 0xFFu; g = (u >> 8) & 0xFFu; b = (u >> 16) & 0xFFu;
    } else {
        r = img[p * 3]; g = img[p * 3 + 1]; b = img[p * 3 + 2];
    }
    const uint32_t m = mask[p];
    const uint32_t a = invert ? 255u - m : m;
    if (premultiply) {
        r = (r * a + 127u) / 255u;
        g = (g * a + 127u) / 255u;
        b = (b * a + 127u) / 255u;
    }
    out[p] = r | (g << 8) | (b << 16) | (a << 24);
}

template <int C, int MODE>
static hipError_t launch_resize_passes(hipStream_t st, const uint8_t* src, uint32_t w, uint32_t nw, uint32_t nh, const int32_t* vtab,
                                       const int32_t* htab, float* tmp, void* out) {
    const unsigned gy = nh < IMG_MAX_GRID_Y ? nh : IMG_MAX_GRID_Y;
    hipLaunchKernelGGL(resize_vertical_kernel<C>, dim3((w + IMG_WG - 1) / IMG_WG, gy), dim3(IMG_WG), 0, st, src, w, vtab, nh, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((resize_horizontal_kernel<C, MODE>), dim3((nw + IMG_WG - 1) / IMG_WG, gy), dim3(IMG_WG), 0, st, tmp, w, htab, nw, nh, out);
    return hipGetLastError();
}

hipError_t enqueue_resize(hipStream_t st, const uint8_t* src, uint32_t w, uint32_t h, uint32_t channels, uint32_t nw, uint32_t nh,
                          const int32_t* vtab, const int32_t* htab, float* tmp, void* out, int mode) {
    (void)h;
    if (mode == RESIZE_OUT_U8) {
        if (channels == 1) return launch_resize_passes<1, RESIZE_OUT_U8>(st, src, w, nw, nh, vtab, htab, tmp, out);
        if (channels == 3) return launch_resize_passes<3, RESIZE_OUT_U8>(st, src, w, nw, nh, vtab, htab, tmp, out);
        return launch_resize_passes<4, RESIZE_OUT_U8>(st, src, w, nw, nh, vtab, htab, tmp, out);
    }
    if (channels == 3) return launch_resize_passes<3, RESIZE_OUT_PACKED>(st, src, w, nw, nh, vtab, htab, tmp, out);
    if (mode == RESIZE_OUT_PACKED) return launch_resize_passes<4, RESIZE_OUT_PACKED>(st, src, w, nw, nh, vtab, htab, tmp, out);
    return launch_resize_passes<4, RESIZE_OUT_PACKED_PREMUL>(st, src, w, nw, nh, vtab, htab, tmp, out);
}

hipError_t enqueue_mask_merge(hipStream_t st, const uint8_t* img, uint32_t channels, const uint8_t* mask, uint64_t pixels, int invert,
                              int premultiply, uint32_t* out) {
    const dim3 grid((unsigned)((pixels + IMG_WG - 1) / IMG_WG));
    if (channels == 4)
        hipLaunchKernelGGL(mask_merge_kernel<4>, grid, dim3(IMG_WG), 0, st, img, mask, pixels, invert, premultiply, out);
    else
        hipLaunchKernelGGL(mask_merge_kernel<3>, grid, dim3(IMG_WG), 0, st, img, mask, pixels, invert, premultiply, out);
    return hipGetLastError();
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_view_output_size(uint32_t w, uint32_t h, uint32_t max_resolution, float scale, uint32_t* out_w, uint32_t* out_h) {
    if (w == 0 || h == 0 || !out_w || !out_h || !(scale > 0.0f) || !std::isfinite(scale)) return BH_ERR_INVALID_ARG;
    float s = scale;
    if (max_resolution != 0) {   // load_image.rs output_scale
        uint32_t m = w > h ? w : h;
        m = m > max_resolution ? m : max_resolution;
        s = (float)max_resolution / (float)m * scale;
    }
    s = s < 1.0f ? s : 1.0f;
    if (s < 1.0f) {
        const float fw = (float)w * s, fh = (float)h * s;
        *out_w = (uint32_t)(fw > 1.0f ? fw : 1.0f);
        *out_h = (uint32_t)(fh > 1.0f ? fh : 1.0f);
    } else {
        *out_w = w;
        *out_h = h;
    }
    return 0;
}

int bh_resize_u8(bh_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint32_t channels, uint8_t* dst, uint32_t nw, uint32_t nh,
                 uint32_t filter) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!src || !dst || w == 0 || h == 0 || nw == 0 || nh == 0 || (channels != 1 && channels != 3 && channels != 4) ||
        (filter != BH_FILTER_LANCZOS3 && filter != BH_FILTER_TRIANGLE))
        return set_error(ctx, BH_ERR_INVALID_ARG, "resize_u8: src / dst, non-zero sizes, channels 1 | 3 | 4 and a known filter");
    if (channels == 4 && (((uintptr_t)src | (uintptr_t)dst) & 3u))
        return set_error(ctx, BH_ERR_INVALID_ARG, "resize_u8: RGBA8 images must be 4-byte aligned");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (nw == w && nh == h) {   // sample.rs resize: the same size is a copy
        BH_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)w * h * channels, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    ResizeTable vt, ht;
    try {
        vt = resize_table(h, nh, filter);
        ht = resize_table(w, nw, filter);
    } catch (const std::bad_alloc&) {
        return set_error(ctx, BH_ERR_OOM, "resize_u8: out of host memory for the weight tables");
    }
    const size_t vbytes = vt->size(), hbytes = ht->size();
    const size_t tab_bytes = vbytes + hbytes;
    const size_t tmp_bytes = (((size_t)w * nh * channels * 4) + 255) & ~(size_t)255;
    // the pinned staging of the tables: free once the previous call's copy has run
    if (ctx->image_tab_ev) BH_HIP(ctx, hipEventSynchronize(ctx->image_tab_ev));
    else BH_HIP(ctx, hipEventCreateWithFlags(&ctx->image_tab_ev, hipEventDisableTiming));
    if (ctx->image_tab_cap < tab_bytes) {
        if (ctx->image_tab_host) BH_HIP(ctx, hipHostFree(ctx->image_tab_host));
        ctx->image_tab_host = nullptr;
        ctx->image_tab_cap = 0;
        BH_HIP(ctx, hipHostMalloc(&ctx->image_tab_host, tab_bytes, hipHostMallocDefault));
        ctx->image_tab_cap = tab_bytes;
    }
    uint8_t* host = (uint8_t*)ctx->image_tab_host;
    std::memcpy(host, vt->data(), vbytes);
    std::memcpy(host + vbytes, ht->data(), hbytes);
    uint8_t* scratch = (uint8_t*)ensure(ctx, SLOT_IMAGE, tmp_bytes + tab_bytes);
    if (!scratch) return BH_ERR_OOM;
    BH_HIP(ctx, hipMemcpyAsync(scratch + tmp_bytes, host, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    BH_HIP(ctx, hipEventRecord(ctx->image_tab_ev, ctx->stream));
    const int32_t* vtab = (const int32_t*)(scratch + tmp_bytes);
    const int32_t* htab = (const int32_t*)(scratch + tmp_bytes + vbytes);
    BH_HIP(ctx, enqueue_resize(ctx->stream, src, w, h, channels, nw, nh, vtab, htab, (float*)scratch, dst, RESIZE_OUT_U8));
    return 0;
}

}  // extern "C"
