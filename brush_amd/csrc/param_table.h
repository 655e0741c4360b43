// param_table.h — the host core of a learned device table (exposure.hip, bilagrid.hip, envmap.hip): V rows of `row` f32 parameters with
// their gradient, Adam moments and step count in one device allocation, owned by a bh_ctx.  The kinds differ in the row length, the
// moment type, the noun in their error text, the pattern a new row starts from and what else they keep in the allocation; everything
// else is written once here.  `who` is the entry point's name in an error.
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "context.h"

namespace bh {

enum ParamTableKind : int { PT_EXPOSURE = 0, PT_BILAGRID = 1, PT_ENVMAP = 2 };
// (a refusal has no table to read the noun from — the handle is of another kind, or of no kind — so it hangs on the kind)
inline const char* param_table_noun(ParamTableKind kind) {
    return kind == PT_EXPOSURE ? "an exposure table" : kind == PT_BILAGRID ? "a bilateral-grid table" : "an environment map";
}

struct ParamTable {
    ParamTableKind kind = PT_EXPOSURE;
    uint32_t n_views = 0;
    size_t row = 0;               // floats per view
    size_t moment_size = 8;       // bytes of a moment: 8 (f64) or 4 (f32)
    void* mem = nullptr;          // one allocation: the kind's extra bytes | m1 | m2 | param | grad | t (each part 8-byte aligned but t)
    void* m1 = nullptr;           // [V,row] moments
    void* m2 = nullptr;           // [V,row]
    float* param = nullptr;       // [V,row]
    float* grad = nullptr;        // [V,row]
    uint32_t* t = nullptr;        // [V]
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;   // passed to the update by value
    virtual ~ParamTable() {       // (a table is deleted through this base: bh_*_destroy, bh_destroy)
        if (mem) (void)hipFree(mem);
    }
};

}  // namespace bh

struct bh_exposure : bh::ParamTable {};   // (the base's defaults are this kind's)
struct bh_bilagrid : bh::ParamTable {
    uint32_t gw = 0, gh = 0, gl = 0;
    bh_bilagrid() { kind = bh::PT_BILAGRID; moment_size = 4; lr = 2e-3; eps = 1e-15; }
};
struct bh_envmap : bh::ParamTable {       // one row of 6 R R 3; its extra bytes are acc | ctl, cleared by one fill
    uint32_t res = 0;
    unsigned long long* acc = nullptr;    // [row] the quantised sums of the backward in flight
    uint32_t* ctl = nullptr;              // [4]: [0] the bits of m of the backward in flight
    uint32_t t_host = 0;                  // the step count the updates are computed from (t[0] is it as of the last update queued)
    bh_envmap() { kind = bh::PT_ENVMAP; moment_size = 4; eps = 1e-15; }
};

namespace bh {

// a new row of a colour table: the 3x4 identity, over and over
inline constexpr float COLOUR_IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

inline void param_table_detach(bh_ctx* ctx, const ParamTable* tab) {
    if (ctx->terms.exposure == tab) ctx->terms.exposure = nullptr;
    if (ctx->terms.bilagrid == tab) ctx->terms.bilagrid = nullptr;
    if (ctx->terms.envmap == tab) ctx->terms.envmap = nullptr;
}

inline void param_tables_free_all(bh_ctx* ctx) {   // bh_destroy
    for (ParamTable* tab : ctx->param_tables) {
        param_table_detach(ctx, tab);
        delete tab;
    }
    ctx->param_tables.clear();
}

// the handle is a table of this kind that the ctx owns (a handle of another kind is refused like any stranger)
inline int param_table_owned(bh_ctx* ctx, ParamTableKind kind, const ParamTable* tab, const char* who) {
    if (!tab || std::find(ctx->param_tables.begin(), ctx->param_tables.end(), tab) == ctx->param_tables.end() || tab->kind != kind)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": not " + param_table_noun(kind) + " of this context");
    return 0;
}

// ... and the views first .. first + count - 1 are rows of it
inline int check_rows(bh_ctx* ctx, ParamTableKind kind, const ParamTable* tab, uint32_t first, uint32_t count, const char* who) {
    BH_TRY(param_table_owned(ctx, kind, tab, who));
    if (first == 0 || count == 0 || first > tab->n_views || count > tab->n_views - first + 1)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": view out of range (views are numbered 1 .. n_views)");
    return 0;
}

// the [h,w,4] frame of an entry point that applies a table; below_2_31: its kernels index pixels with 32 bits
inline int check_image(bh_ctx* ctx, uint32_t h, uint32_t w, bool below_2_31, const char* who) {
    if (h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": an image of zero size");
    if (below_2_31 && (uint64_t)h * w > 0x7FFFFFFFull) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": h * w must stay below 2^31");
    return 0;
}

inline int read_back(bh_ctx* ctx, void* host, const void* dev, size_t bytes) {
    BH_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);
    return 0;
}

// the setters' tail: the caller's array may die on return (pageable host memory is staged, a temporary is gone at once)
inline int settle_writes(bh_ctx* ctx) {
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);
    return 0;
}

// bh_*_create's first refusals; *table = NULL from here on
template <class T>
int param_table_create_args(bh_ctx* ctx, T** table, uint32_t n_views, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!table) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    *table = nullptr;
    if (n_views == 0 || n_views > (1u << 24)) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": n_views must be 1 .. 2^24");
    return 0;
}

// ... and the table itself, in `fresh` (a new record of the kind; the ctx's from here on, deleted on failure): n_views rows of `row`
// floats, each `*pattern` over and over (NULL: zeros), and `extra` bytes of the kind's own at mem; everything else zero
inline int param_table_create(bh_ctx* ctx, ParamTable* fresh, uint32_t n_views, size_t row, size_t extra, const float (*pattern)[12], const char* who) {
    std::unique_ptr<ParamTable> tab(fresh);
    BH_HIP(ctx, hipSetDevice(ctx->device));
    extra = (extra + 7) & ~(size_t)7;
    const size_t v = n_views, cells = v * row, bytes = extra + cells * (2 * tab->moment_size + 8) + v * 4;
    hipError_t e = hipMalloc(&tab->mem, bytes);   // (each kind's refusal keeps the words it had before the kinds shared this)
    if (e != hipSuccess) return check_hip(ctx, e, tab->kind == PT_ENVMAP ? who : "hipMalloc(&mem, bytes)");
    tab->n_views = n_views;
    tab->row = row;
    tab->m1 = static_cast<char*>(tab->mem) + extra;
    tab->m2 = static_cast<char*>(tab->m1) + cells * tab->moment_size;
    tab->param = reinterpret_cast<float*>(static_cast<char*>(tab->m2) + cells * tab->moment_size);
    tab->grad = tab->param + cells;
    tab->t = reinterpret_cast<uint32_t*>(tab->grad + cells);
    std::vector<float> rows(pattern ? std::min<size_t>(cells, (size_t)12 << 16) : 0);   // staged in pieces of whole patterns
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (*pattern)[i % 12];
    e = hipMemsetAsync(tab->mem, 0, bytes, ctx->stream);
    for (size_t i = 0; i < cells && !rows.empty() && e == hipSuccess; i += rows.size())
        e = hipMemcpyAsync(tab->param + i, rows.data(), std::min(rows.size(), cells - i) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the staging vector dies here)
    if (e != hipSuccess) return check_hip(ctx, e, who);
    deliver_pending_loss(ctx);
    ctx->param_tables.push_back(tab.release());
    return 0;
}

inline int param_table_destroy(bh_ctx* ctx, ParamTableKind kind, ParamTable* tab, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(param_table_owned(ctx, kind, tab, who));
    param_table_detach(ctx, tab);   // an attached table is detached first
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // kernels queued on the table have run
    deliver_pending_loss(ctx);
    ctx->param_tables.erase(std::find(ctx->param_tables.begin(), ctx->param_tables.end(), tab));
    delete tab;
    return 0;
}

// bh_train_set_*: NULL detaches, anything else must be a table of this kind and ctx
inline int param_table_attachable(bh_ctx* ctx, ParamTableKind kind, const ParamTable* tab, const char* who) {
    return tab ? param_table_owned(ctx, kind, tab, who) : 0;
}

inline int param_table_set_params(bh_ctx* ctx, ParamTableKind kind, ParamTable* tab, uint32_t first, uint32_t count, const float* host, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, first, count, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemcpyAsync(tab->param + (size_t)(first - 1) * tab->row, host, (size_t)count * tab->row * 4, hipMemcpyHostToDevice, ctx->stream));
    return settle_writes(ctx);
}

// get_params / get_grad: `which` is &ParamTable::param or &ParamTable::grad
inline int param_table_get_rows(bh_ctx* ctx, ParamTableKind kind, const ParamTable* tab, float* ParamTable::*which, uint32_t first, uint32_t count, float* host,
                                const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, first, count, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return read_back(ctx, host, tab->*which + (size_t)(first - 1) * tab->row, (size_t)count * tab->row * 4);
}

// m1, m2: `row` moments of the table's own type each
inline int param_table_get_state(bh_ctx* ctx, ParamTableKind kind, const ParamTable* tab, uint32_t view, void* m1, void* m2, uint32_t* t, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!m1 || !m2 || !t) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, view, 1, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = tab->row * tab->moment_size, off = (size_t)(view - 1) * bytes;
    BH_HIP(ctx, hipMemcpyAsync(m1, static_cast<const char*>(tab->m1) + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(m2, static_cast<const char*>(tab->m2) + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return read_back(ctx, t, tab->t + (view - 1), 4);
}

inline int param_table_set_state(bh_ctx* ctx, ParamTableKind kind, ParamTable* tab, uint32_t view, const void* m1, const void* m2, uint32_t t, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!m1 || !m2) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, view, 1, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = tab->row * tab->moment_size, off = (size_t)(view - 1) * bytes;
    BH_HIP(ctx, hipMemcpyAsync(static_cast<char*>(tab->m1) + off, m1, bytes, hipMemcpyHostToDevice, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(static_cast<char*>(tab->m2) + off, m2, bytes, hipMemcpyHostToDevice, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(tab->t + (view - 1), &t, 4, hipMemcpyHostToDevice, ctx->stream));
    return settle_writes(ctx);
}

inline int param_table_set_adam(bh_ctx* ctx, ParamTableKind kind, ParamTable* tab, double lr, double beta1, double beta2, double eps, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(check_rows(ctx, kind, tab, 1, 1, who));
    if (!(lr >= 0.0) || !std::isfinite(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0) || !std::isfinite(eps))
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": needs lr >= 0, 0 <= beta < 1 and eps > 0, all finite");
    tab->lr = lr;
    tab->beta1 = beta1;
    tab->beta2 = beta2;
    tab->eps = eps;
    return 0;
}

}  // namespace bh
