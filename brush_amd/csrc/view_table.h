// view_table.h — the host core of a per-view parameter table (exposure.hip, bilagrid.hip): V rows of `row` f32 parameters with their
// gradient, Adam moments and step count in one device allocation, owned by a bh_ctx.  The two kinds differ in the row length, the
// moment type and the noun in their error text; everything else is written once here.  `who` is the entry point's name in an error.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "context.h"

namespace bh {

enum ViewTableKind : int { VT_EXPOSURE = 0, VT_BILAGRID = 1 };
// (a refusal has no table to read the noun from — the handle is of the other kind, or of no kind — so it hangs on the kind)
inline const char* view_table_noun(ViewTableKind kind) { return kind == VT_EXPOSURE ? "an exposure table" : "a bilateral-grid table"; }

struct ViewTable {
    ViewTableKind kind = VT_EXPOSURE;
    uint32_t n_views = 0;
    size_t row = 0;               // floats per view
    size_t moment_size = 8;       // bytes of a moment: 8 (f64) or 4 (f32)
    void* mem = nullptr;          // one allocation: m1 | m2 | param | grad | t (the moments first: f64 ones are 8-byte aligned)
    void* m1 = nullptr;           // [V,row] moments
    void* m2 = nullptr;           // [V,row]
    float* param = nullptr;       // [V,row]
    float* grad = nullptr;        // [V,row]
    uint32_t* t = nullptr;        // [V]
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;   // passed to the update by value
};

}  // namespace bh

struct bh_exposure : bh::ViewTable {};   // (the base's defaults are this kind's)
struct bh_bilagrid : bh::ViewTable {
    uint32_t gw = 0, gh = 0, gl = 0;
    bh_bilagrid() { kind = bh::VT_BILAGRID; moment_size = 4; lr = 2e-3; eps = 1e-15; }
};

namespace bh {

inline void view_table_free(ViewTable* tab) {
    if (tab->mem) (void)hipFree(tab->mem);
    if (tab->kind == VT_EXPOSURE) delete static_cast<bh_exposure*>(tab);
    else delete static_cast<bh_bilagrid*>(tab);
}

inline void view_table_detach(bh_ctx* ctx, const ViewTable* tab) {
    if (ctx->terms.exposure == tab) ctx->terms.exposure = nullptr;
    if (ctx->terms.bilagrid == tab) ctx->terms.bilagrid = nullptr;
}

inline void view_tables_free_all(bh_ctx* ctx) {   // bh_destroy
    for (ViewTable* tab : ctx->view_tables) view_table_free(tab);
    ctx->view_tables.clear();
    ctx->terms.exposure = nullptr;
    ctx->terms.bilagrid = nullptr;
}

// the handle is a table of this kind that the ctx owns (a handle of the other kind is refused like any stranger)
inline int view_table_owned(bh_ctx* ctx, ViewTableKind kind, const ViewTable* tab, const char* who) {
    if (!tab || std::find(ctx->view_tables.begin(), ctx->view_tables.end(), tab) == ctx->view_tables.end() || tab->kind != kind)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": not " + view_table_noun(kind) + " of this context");
    return 0;
}

// ... and the views first .. first + count - 1 are rows of it
inline int check_rows(bh_ctx* ctx, ViewTableKind kind, const ViewTable* tab, uint32_t first, uint32_t count, const char* who) {
    BH_TRY(view_table_owned(ctx, kind, tab, who));
    if (first == 0 || count == 0 || first > tab->n_views || count > tab->n_views - first + 1)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": view out of range (views are numbered 1 .. n_views)");
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
int view_table_create_args(bh_ctx* ctx, T** table, uint32_t n_views, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!table) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    *table = nullptr;
    if (n_views == 0 || n_views > (1u << 24)) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": n_views must be 1 .. 2^24");
    return 0;
}

// ... and the table itself: n_views rows of `row` floats, a multiple of 12 — every parameter row is ident12 over and over, everything
// else zero
inline int view_table_create(bh_ctx* ctx, ViewTableKind kind, uint32_t n_views, size_t row, const char* who, ViewTable** out) {
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ViewTable* tab = kind == VT_EXPOSURE ? static_cast<ViewTable*>(new bh_exposure) : new bh_bilagrid;
    const size_t v = n_views, cells = v * row, bytes = cells * (2 * tab->moment_size + 8) + v * 4;
    hipError_t e = hipMalloc(&tab->mem, bytes);
    if (e != hipSuccess) {
        view_table_free(tab);
        return check_hip(ctx, e, "hipMalloc(&mem, bytes)");
    }
    tab->n_views = n_views;
    tab->row = row;
    tab->m1 = tab->mem;
    tab->m2 = static_cast<char*>(tab->m1) + cells * tab->moment_size;
    tab->param = reinterpret_cast<float*>(static_cast<char*>(tab->m2) + cells * tab->moment_size);
    tab->grad = tab->param + cells;
    tab->t = reinterpret_cast<uint32_t*>(tab->grad + cells);
    static const float ident12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<float> ident(std::min<size_t>(cells, (size_t)12 << 16));   // staged in pieces of whole matrices
    for (size_t i = 0; i < ident.size(); ++i) ident[i] = ident12[i % 12];
    e = hipMemsetAsync(tab->mem, 0, bytes, ctx->stream);
    for (size_t i = 0; i < cells && e == hipSuccess; i += ident.size())
        e = hipMemcpyAsync(tab->param + i, ident.data(), std::min(ident.size(), cells - i) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the staging vector dies here)
    if (e != hipSuccess) {
        view_table_free(tab);
        return check_hip(ctx, e, who);
    }
    deliver_pending_loss(ctx);
    ctx->view_tables.push_back(tab);
    *out = tab;
    return 0;
}

inline int view_table_destroy(bh_ctx* ctx, ViewTableKind kind, ViewTable* tab, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(view_table_owned(ctx, kind, tab, who));
    view_table_detach(ctx, tab);   // an attached table is detached first
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // kernels queued on the table have run
    deliver_pending_loss(ctx);
    ctx->view_tables.erase(std::find(ctx->view_tables.begin(), ctx->view_tables.end(), tab));
    view_table_free(tab);
    return 0;
}

// bh_train_set_*: NULL detaches, anything else must be a table of this kind and ctx
inline int view_table_attachable(bh_ctx* ctx, ViewTableKind kind, const ViewTable* tab, const char* who) {
    return tab ? view_table_owned(ctx, kind, tab, who) : 0;
}

inline int view_table_set_params(bh_ctx* ctx, ViewTableKind kind, ViewTable* tab, uint32_t first, uint32_t count, const float* host, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, first, count, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemcpyAsync(tab->param + (size_t)(first - 1) * tab->row, host, (size_t)count * tab->row * 4, hipMemcpyHostToDevice, ctx->stream));
    return settle_writes(ctx);
}

// get_params / get_grad: `which` is &ViewTable::param or &ViewTable::grad
inline int view_table_get_rows(bh_ctx* ctx, ViewTableKind kind, const ViewTable* tab, float* ViewTable::*which, uint32_t first, uint32_t count, float* host,
                               const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, first, count, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return read_back(ctx, host, tab->*which + (size_t)(first - 1) * tab->row, (size_t)count * tab->row * 4);
}

// m1, m2: `row` moments of the table's own type each
inline int view_table_get_state(bh_ctx* ctx, ViewTableKind kind, const ViewTable* tab, uint32_t view, void* m1, void* m2, uint32_t* t, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!m1 || !m2 || !t) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_rows(ctx, kind, tab, view, 1, who));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = tab->row * tab->moment_size, off = (size_t)(view - 1) * bytes;
    BH_HIP(ctx, hipMemcpyAsync(m1, static_cast<const char*>(tab->m1) + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(m2, static_cast<const char*>(tab->m2) + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return read_back(ctx, t, tab->t + (view - 1), 4);
}

inline int view_table_set_state(bh_ctx* ctx, ViewTableKind kind, ViewTable* tab, uint32_t view, const void* m1, const void* m2, uint32_t t, const char* who) {
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

inline int view_table_set_adam(bh_ctx* ctx, ViewTableKind kind, ViewTable* tab, double lr, double beta1, double beta2, double eps, const char* who) {
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
