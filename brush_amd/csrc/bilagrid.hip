// bilagrid.hip — per-view bilateral grids (brush_hip_bilagrid.h): the trilinear slice of a view's grid of 3x4 colour
// matrices on the rasterizer's image, its backward, the total-variation term and Adam on the grid, all on the device.
//   bilagrid_slice_kernel     streaming: per pixel 8 corners x 3 float4 of the grid (the row is at most a few hundred KB: L1 / L2)
//   bilagrid_vg_kernel        v_g by destination: a block owns (xy cell, band of rows) — fx, fy are monotone, so the pixels of a cell are a
//                             rectangle — and each of its waves walks it once per level it owns with 4 corners x 12 f64 sums per lane;
//                             no atomics, no LDS, a fixed order
//   bilagrid_pixel_kernel     v_img per pixel (the same gather plus dA/dfz); behind the v_g pass, so that it may overwrite v'
//   bilagrid_final_kernel     per grid element: the units' partial rows in index order + the TV gradient -> grad and the f64 sum
//   bilagrid_step_kernel      Adam on the f64 sum (a launch of its own: the TV gradient above reads neighbouring parameters)
//   bilagrid_tv_kernel        TV of a row, one block, f64
// The table itself — a bh_bilagrid is a ParamTable of rows of gh gw gl 12 with f32 moments, plus the grid's sides — and every entry
// point that only manages it are param_table.h's, shared with exposure.hip and envmap.hip; the wave butterfly and the Adam step are device_f64_sum.h's.
#include "../../include/brush_hip_bilagrid.h"
#include "device_f64_sum.h"
#include "param_table.h"

namespace bh {

constexpr int BG_WG = 256;
constexpr int BG_WAVES = BG_WG / 64;
// slice and v_img: grid-stride over pixels, at most 8 blocks of 256 per CU
constexpr uint32_t BG_PIXEL_MAX_BLOCKS = 2048;
// v_g: a cell's rows are cut into bands of about this many pixels (8 per lane and level behind each block reduction) ...
constexpr uint32_t BG_UNIT_PIXELS = 2048;
// ... at most this many, and at most this many (unit, level) partial rows of 48 f64 in all (96 MB of scratch)
constexpr uint32_t BG_MAX_BANDS = 256;
constexpr uint32_t BG_MAX_UNIT_LEVELS = 1u << 18;
constexpr size_t BG_SCRATCH_HEAD = 16;   // bytes in front of the f64 sums: the train step's TV scalar

struct BgGeom {
    uint32_t w, h, gw, gh, gl;
    float sx, sy, sz;   // float(Wg-1) / float(w), float(Hg-1) / float(h), float(L-1)
};

// cell index, upper neighbour and fraction of a coordinate f >= 0 on an axis of n vertices
BH_DEV void bg_axis(float f, uint32_t n, uint32_t& i0, uint32_t& i1, float& t) {
    const int top = n >= 2u ? (int)n - 2 : 0;
    const int fl = (int)floorf(f);
    const int lo = fl < top ? fl : top;
    i0 = (uint32_t)lo;
    i1 = i0 + 1u < n - 1u ? i0 + 1u : n - 1u;
    t = __fsub_rn(f, (float)lo);
}
BH_DEV float bg_coord(uint32_t p, float s) { return __fmul_rn(__fadd_rn((float)p, 0.5f), s); }
BH_DEV float bg_lum(const float4& x) { return __fadd_rn(__fadd_rn(__fmul_rn(x.x, 0.299f), __fmul_rn(x.y, 0.587f)), __fmul_rn(x.z, 0.114f)); }
BH_DEV float bg_fz(float lum, float sz) { return __fmul_rn(fminf(fmaxf(lum, 0.0f), 1.0f), sz); }

// the smallest pixel index in [0, n] whose cell on an axis of `cells` cells is >= cell (n: none), by the pixel's own arithmetic
BH_DEV uint32_t bg_first(uint32_t n, float s, uint32_t cells, uint32_t cell) {
    if (cell == 0u) return 0u;
    if (cell >= cells) return n;
    uint32_t lo = 0u, hi = n;   // floor(coord) is monotone in the pixel index, and cell <= cells - 1 is below the clamp
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((int)floorf(bg_coord(mid, s)) >= (int)cell) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// One axis for the interpolation: the nearer vertex, the farther one and s = min(t, 1 - t) <= 1/2 (1 - t is exact for t >= 1/2).
struct BgSide {
    uint32_t near, far;
    float s;
    bool flipped;   // near is the upper vertex
};
BH_DEV BgSide bg_side(float f, uint32_t n) {
    uint32_t i0, i1;
    float t;
    bg_axis(f, n, i0, i1, t);
    BgSide a;
    a.flipped = t > 0.5f;
    a.near = a.flipped ? i1 : i0;
    a.far = a.flipped ? i0 : i1;
    a.s = a.flipped ? 1.0f - t : t;
    return a;
}

struct BgCorners {
    uint32_t base[8];   // float4 index of corner (y, x, z) = base[ny*4 + nx*2 + nz], n = 0 the nearer vertex of the axis
    float sy, sx, sz;
    float zsign;        // d tz / d sz: +1, or -1 where the z axis is flipped
    bool inside;
};

BH_DEV BgCorners bg_corners(const BgGeom& g, uint32_t px, uint32_t py, const float4& x) {
    BgCorners c;
    const BgSide ax = bg_side(bg_coord(px, g.sx), g.gw), ay = bg_side(bg_coord(py, g.sy), g.gh);
    const float lum = bg_lum(x);
    const BgSide az = bg_side(bg_fz(lum, g.sz), g.gl);
    c.inside = lum > 0.0f && lum < 1.0f;
    c.sy = ay.s; c.sx = ax.s; c.sz = az.s;
    c.zsign = az.flipped ? -1.0f : 1.0f;
    const uint32_t jj[2] = {ay.near, ay.far}, ii[2] = {ax.near, ax.far}, ll[2] = {az.near, az.far};
#pragma unroll
    for (int ny = 0; ny < 2; ++ny)
#pragma unroll
        for (int nx = 0; nx < 2; ++nx)
#pragma unroll
            for (int nz = 0; nz < 2; ++nz) c.base[ny * 4 + nx * 2 + nz] = ((jj[ny] * g.gw + ii[nx]) * g.gl + ll[nz]) * 3u;
    return c;
}

// a + s (b - a), anchored at the nearer vertex: s <= 1/2 keeps the rounding of b - a inside the pair's own mass (1 - s) |a| + s |b|,
// and equal vertices interpolate exactly — a constant grid is reproduced bit for bit
BH_DEV float bg_lerp(float a, float b, float s) { return fmaf(s, b - a, a); }
BH_DEV float4 bg_lerp4(const float4& a, const float4& b, float s) {
    return make_float4(bg_lerp(a.x, b.x, s), bg_lerp(a.y, b.y, s), bg_lerp(a.z, b.z, s), bg_lerp(a.w, b.w, s));
}

// A = the trilinear interpolation of the 8 corners as nested lerps: along z, then x, then y
BH_DEV void bg_matrix(const float4* __restrict__ grid, const BgCorners& c, float a[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float4 zx[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) zx[n] = bg_lerp4(grid[c.base[n * 2] + r], grid[c.base[n * 2 + 1] + r], c.sz);
        const float4 m = bg_lerp4(bg_lerp4(zx[0], zx[1], c.sx), bg_lerp4(zx[2], zx[3], c.sx), c.sy);
        a[4 * r] = m.x; a[4 * r + 1] = m.y; a[4 * r + 2] = m.z; a[4 * r + 3] = m.w;
    }
}

// y = A(p) x on rgb, alpha passes through; out may be img (a lane reads its pixel before it writes it)
__global__ __launch_bounds__(BG_WG) void bilagrid_slice_kernel(const float4* __restrict__ grid, const float4* img, float4* out, BgGeom g, uint32_t pixels) {
    const uint32_t stride = gridDim.x * BG_WG;
    for (uint32_t p = blockIdx.x * BG_WG + threadIdx.x; p < pixels; p += stride) {
        const float4 x = img[p];
        const uint32_t py = p / g.w, px = p - py * g.w;
        const BgCorners c = bg_corners(g, px, py, x);
        float a[12];
        bg_matrix(grid, c, a);
        float4 y;
        y.x = fmaf(a[0], x.x, fmaf(a[1], x.y, fmaf(a[2], x.z, a[3])));
        y.y = fmaf(a[4], x.x, fmaf(a[5], x.y, fmaf(a[6], x.z, a[7])));
        y.z = fmaf(a[8], x.x, fmaf(a[9], x.y, fmaf(a[10], x.z, a[11])));
        y.w = x.w;
        out[p] = y;
    }
}

// v_c = sum_r A[4r+c] v'_r (an f32 fma chain) + lumcoef_c (L-1) inside sum_q dA_q o_q (f64: the products v'_r x_k are exact there),
// one rounding of the sum; v_img may be v_sliced
__global__ __launch_bounds__(BG_WG) void bilagrid_pixel_kernel(const float4* __restrict__ grid, const float4* __restrict__ x_img, const float4* v_sliced,
                                                               float4* v_img, BgGeom g, uint32_t pixels) {
    const uint32_t stride = gridDim.x * BG_WG;
    for (uint32_t p = blockIdx.x * BG_WG + threadIdx.x; p < pixels; p += stride) {
        const float4 x = x_img[p];
        const float4 u = v_sliced[p];
        const uint32_t py = p / g.w, px = p - py * g.w;
        const BgCorners c = bg_corners(g, px, py, x);
        float a[12];
        bg_matrix(grid, c, a);
        const float va0 = fmaf(a[0], u.x, fmaf(a[4], u.y, a[8] * u.z));
        const float va1 = fmaf(a[1], u.x, fmaf(a[5], u.y, a[9] * u.z));
        const float va2 = fmaf(a[2], u.x, fmaf(a[6], u.y, a[10] * u.z));
        double guide = 0.0;
        if (c.inside && g.gl > 1u) {
            const double xs[4] = {x.x, x.y, x.z, 1.0}, us[3] = {u.x, u.y, u.z};
            const double wy[2] = {1.0 - (double)c.sy, (double)c.sy}, wx[2] = {1.0 - (double)c.sx, (double)c.sx};
#pragma unroll
            for (int n = 0; n < 4; ++n) {   // xy corner n: w_y w_x sum_q (g[far] - g[near])_q o_q
                double d = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 lo = grid[c.base[n * 2] + r], hi = grid[c.base[n * 2 + 1] + r];
                    const double dr = fma((double)hi.x - (double)lo.x, xs[0], fma((double)hi.y - (double)lo.y, xs[1],
                                      fma((double)hi.z - (double)lo.z, xs[2], (double)hi.w - (double)lo.w)));
                    d = fma(dr, us[r], d);
                }
                guide = fma(wy[n >> 1] * wx[n & 1], d, guide);
            }
            guide *= (double)c.zsign;
            guide *= (double)g.sz;
        }
        float4 v;
        v.x = (float)fma(0.299, guide, (double)va0);
        v.y = (float)fma(0.587, guide, (double)va1);
        v.z = (float)fma(0.114, guide, (double)va2);
        v.w = u.w;
        v_img[p] = v;
    }
}

// One halving step of the row butterfly: partners `mask` lanes apart split their N entries between them — the lane with the bit clear
// keeps the lower half, the other the upper half — and each adds the partner's copy of the half it keeps: N / 2 exchanges, not N.
template <int N>
BH_DEV void bg_halve(const double (&in)[N], double (&out)[N / 2], bool upper, int mask) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const double keep = upper ? in[k + N / 2] : in[k], send = upper ? in[k] : in[k + N / 2];
        out[k] = keep + __shfl_xor(send, mask, 64);
    }
}

// The 48 sums of a wave's 64 lanes in 51 exchanges instead of 288: four halving steps (48 -> 24 -> 12 -> 6 -> 3 entries per lane), then
// two plain steps.  Every lane ends with the wave's totals of entries base .. base + 2, base = 24 b5 + 12 b4 + 6 b3 + 3 b2 of its lane
// number; the pattern of additions is fixed, so the bits are.
BH_DEV uint32_t bg_wave_rows(const double (&s)[48], uint32_t lane, double (&r)[3]) {
    double a[24], b[12], c[6];
    bg_halve<48>(s, a, (lane & 32u) != 0u, 32);
    bg_halve<24>(a, b, (lane & 16u) != 0u, 16);
    bg_halve<12>(b, c, (lane & 8u) != 0u, 8);
    bg_halve<6>(c, r, (lane & 4u) != 0u, 4);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] += __shfl_xor(r[k], 2, 64);
        r[k] += __shfl_xor(r[k], 1, 64);
    }
    return ((lane >> 5) & 1u) * 24u + ((lane >> 4) & 1u) * 12u + ((lane >> 3) & 1u) * 6u + ((lane >> 2) & 1u) * 3u;
}

// block = (cell row jc, cell column ic, band): the rectangle of pixels whose (j0, i0) is the cell and whose row lies in the band.  Wave
// w of the block takes the levels w, w + 4, ...: per level every lane keeps 4 xy corners x 12 f64 sums of w o over its pixels of the
// rectangle (weights and products in f64: a term costs the add's rounding), then the row butterfly, and one row of 48 f64 per (unit,
// level) — zeros where the rectangle is empty or no pixel of it touches the level.  No LDS, no barrier.
__global__ __launch_bounds__(BG_WG) void bilagrid_vg_kernel(const float4* __restrict__ x_img, const float4* __restrict__ v_sliced, BgGeom g, uint32_t ncx,
                                                            uint32_t ncy, uint32_t bands, double* __restrict__ partials) {
    const uint32_t unit = blockIdx.x;
    const uint32_t band = unit % bands, cell = unit / bands, ic = cell % ncx, jc = cell / ncx;
    const uint32_t c0 = bg_first(g.w, g.sx, ncx, ic), c1 = bg_first(g.w, g.sx, ncx, ic + 1u);
    const uint32_t r0 = bg_first(g.h, g.sy, ncy, jc), r1 = bg_first(g.h, g.sy, ncy, jc + 1u);
    const uint32_t per = (r1 - r0 + bands - 1u) / bands;
    const uint32_t rb0 = r0 + band * per < r1 ? r0 + band * per : r1;
    const uint32_t rb1 = rb0 + per < r1 ? rb0 + per : r1;
    const uint32_t ncol = c1 - c0, count = ncol * (rb1 - rb0);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t l = wave; l < g.gl; l += BG_WAVES) {
        double s[48];
#pragma unroll
        for (int k = 0; k < 48; ++k) s[k] = 0.0;
        for (uint32_t k = lane; k < count; k += 64u) {
            const uint32_t ry = k / ncol, py = rb0 + ry, px = c0 + (k - ry * ncol);
            const float4 x = x_img[(size_t)py * g.w + px];
            uint32_t l0, l1, i0, i1;
            float tz, tx, ty;
            bg_axis(bg_fz(bg_lum(x), g.sz), g.gl, l0, l1, tz);
            const double wz = (l0 == l ? 1.0 - (double)tz : 0.0) + (l1 == l ? (double)tz : 0.0);
            if (wz == 0.0) continue;
            const float4 u = v_sliced[(size_t)py * g.w + px];
            bg_axis(bg_coord(px, g.sx), g.gw, i0, i1, tx);
            bg_axis(bg_coord(py, g.sy), g.gh, i0, i1, ty);
            const double wy[2] = {1.0 - (double)ty, (double)ty}, wx[2] = {1.0 - (double)tx, (double)tx};
            const double xs[3] = {x.x, x.y, x.z}, us[3] = {u.x, u.y, u.z};
            double o[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                o[4 * r] = us[r] * xs[0]; o[4 * r + 1] = us[r] * xs[1]; o[4 * r + 2] = us[r] * xs[2]; o[4 * r + 3] = us[r];
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const double wn = wy[n >> 1] * wx[n & 1] * wz;
#pragma unroll
                for (int q = 0; q < 12; ++q) s[n * 12 + q] = fma(wn, o[q], s[n * 12 + q]);
            }
        }
        double r[3];
        const uint32_t base = bg_wave_rows(s, lane, r);
        if ((lane & 3u) == 0u) {
            double* row = partials + ((size_t)unit * g.gl + l) * 48 + base;
            row[0] = r[0]; row[1] = r[1]; row[2] = r[2];
        }
    }
}

struct BgTv {
    double cz, cy, cx;   // 2 / count_d, 0 for an axis of one vertex
};

// dTV/dg[e] of one axis: (2 / count) ((g[e] - g[e - step]) - (g[e + step] - g[e])), each half where the neighbour exists
BH_DEV double bg_tv_axis(const float* __restrict__ param, size_t e, uint32_t idx, uint32_t n, size_t step, double c) {
    const double v = param[e];
    double d = 0.0;
    if (idx > 0u) d += v - (double)param[e - step];
    if (idx + 1u < n) d -= (double)param[e + step] - v;
    return c * d;
}

// one lane per grid element (j, i, l, q): its partial rows in (cell row, cell column, corner, band) order, the TV gradient, grad and
// the unrounded sum; with `update` the row's step count advances here, before the step kernel reads it
__global__ __launch_bounds__(BG_WG) void bilagrid_final_kernel(const double* __restrict__ partials, const float* __restrict__ param, float* __restrict__ grad,
                                                               double* __restrict__ gsum, uint32_t* t, BgGeom g, uint32_t ncx, uint32_t ncy, uint32_t bands,
                                                               uint32_t row, double tv_weight, BgTv tv, int update) {
    const uint32_t e = blockIdx.x * BG_WG + threadIdx.x;
    if (e == 0u && update) *t = *t + 1u;
    if (e >= row) return;
    const uint32_t q = e % 12u, l = (e / 12u) % g.gl, i = (e / (12u * g.gl)) % g.gw, j = e / (12u * g.gl * g.gw);
    double s = 0.0;
    for (uint32_t jc = j > 0u ? j - 1u : 0u; jc <= j && jc < ncy; ++jc)
        for (uint32_t cy = 0; cy < 2u; ++cy) {
            if ((jc + cy < g.gh - 1u ? jc + cy : g.gh - 1u) != j) continue;
            for (uint32_t ic = i > 0u ? i - 1u : 0u; ic <= i && ic < ncx; ++ic)
                for (uint32_t cx = 0; cx < 2u; ++cx) {
                    if ((ic + cx < g.gw - 1u ? ic + cx : g.gw - 1u) != i) continue;
                    const size_t first = ((size_t)(jc * ncx + ic) * bands * g.gl + l) * 48 + (cy * 2u + cx) * 12u + q;
                    for (uint32_t b = 0; b < bands; ++b) s += partials[first + (size_t)b * g.gl * 48];
                }
        }
    if (tv_weight != 0.0) {
        const double d = bg_tv_axis(param, e, l, g.gl, 12, tv.cz) + bg_tv_axis(param, e, j, g.gh, (size_t)12 * g.gl * g.gw, tv.cy) +
                         bg_tv_axis(param, e, i, g.gw, (size_t)12 * g.gl, tv.cx);
        s = fma(tv_weight, d, s);
    }
    grad[e] = (float)s;
    gsum[e] = s;
}

// Adam in f64 on the unrounded sum; the moments are stored rounded to f32, the parameter moves by the unrounded ones
__global__ __launch_bounds__(BG_WG) void bilagrid_step_kernel(const double* __restrict__ gsum, float* __restrict__ param, float* __restrict__ m1,
                                                              float* __restrict__ m2, const uint32_t* __restrict__ t, uint32_t row, double lr, double beta1,
                                                              double beta2, double eps) {
    const uint32_t e = blockIdx.x * BG_WG + threadIdx.x;
    if (e >= row) return;
    double a, b;
    param[e] = adam_step_f64(gsum[e], param[e], (double)m1[e], (double)m2[e], (double)*t, lr, beta1, beta2, eps, a, b);
    m1[e] = (float)a;
    m2[e] = (float)b;
}

// TV of a row: every lane adds the squared forward differences of its elements (e = lane, lane + 256, ...) over count_d, then the
// butterfly and the waves in order.  accum != NULL (the train step): accum[0] += weight * f32(TV), stored to accum_host too.
__global__ __launch_bounds__(BG_WG) void bilagrid_tv_kernel(const float* __restrict__ param, BgGeom g, uint32_t row, BgTv tv, float* __restrict__ value,
                                                            float weight, float* __restrict__ accum, float* __restrict__ accum_host) {
    __shared__ double wave_sums[BG_WAVES];
    const size_t sz = 12, sx = (size_t)12 * g.gl, sy = sx * g.gw;
    double s = 0.0;
    for (uint32_t e = threadIdx.x; e < row; e += BG_WG) {
        const uint32_t l = (e / 12u) % g.gl, i = (e / (12u * g.gl)) % g.gw, j = e / (12u * g.gl * g.gw);
        const double v = param[e];
        if (l + 1u < g.gl) { const double d = (double)param[e + sz] - v; s = fma(d * d, 0.5 * tv.cz, s); }
        if (j + 1u < g.gh) { const double d = (double)param[e + sy] - v; s = fma(d * d, 0.5 * tv.cy, s); }
        if (i + 1u < g.gw) { const double d = (double)param[e + sx] - v; s = fma(d * d, 0.5 * tv.cx, s); }
    }
    s = dl_wave_sum(s);
    if ((threadIdx.x & 63u) == 0u) wave_sums[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = wave_sums[0];
#pragma unroll
        for (int w = 1; w < BG_WAVES; ++w) r += wave_sums[w];
        const float f = (float)r;
        value[0] = f;
        if (accum) {   // the train step: its loss grows in place, in f32, and travels to the pinned word the host reads
            const float total = accum[0] + weight * f;
            accum[0] = total;
            if (accum_host) accum_host[0] = total;
        }
    }
}

static BgGeom geom_of(const bh_bilagrid* tab, uint32_t h, uint32_t w) {
    BgGeom g;
    g.w = w; g.h = h; g.gw = tab->gw; g.gh = tab->gh; g.gl = tab->gl;
    g.sx = (float)(tab->gw - 1u) / (float)w;
    g.sy = (float)(tab->gh - 1u) / (float)h;
    g.sz = (float)(tab->gl - 1u);
    return g;
}

static BgTv tv_of(const bh_bilagrid* tab) {
    const double cells = (double)tab->gh * tab->gw * tab->gl * 12.0;
    BgTv tv;
    tv.cz = tab->gl > 1u ? 2.0 / (cells / tab->gl * (tab->gl - 1u)) : 0.0;
    tv.cy = tab->gh > 1u ? 2.0 / (cells / tab->gh * (tab->gh - 1u)) : 0.0;
    tv.cx = tab->gw > 1u ? 2.0 / (cells / tab->gw * (tab->gw - 1u)) : 0.0;
    return tv;
}

static uint32_t pixel_grid(uint32_t pixels) {
    const uint32_t blocks = (pixels + BG_WG - 1) / BG_WG;
    return blocks < BG_PIXEL_MAX_BLOCKS ? blocks : BG_PIXEL_MAX_BLOCKS;
}

// bands per cell of the v_g pass: a function of the image and grid sizes alone
static uint32_t bilagrid_bands(uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t gl) {
    const uint32_t ncx = gw > 1u ? gw - 1u : 1u, ncy = gh > 1u ? gh - 1u : 1u;
    const uint64_t cell_px = (uint64_t)((w + ncx - 1u) / ncx) * ((h + ncy - 1u) / ncy);
    uint64_t bands = (cell_px + BG_UNIT_PIXELS - 1u) / BG_UNIT_PIXELS;
    const uint64_t room = BG_MAX_UNIT_LEVELS / ((uint64_t)ncx * ncy * gl);
    bands = std::min<uint64_t>(bands, std::min<uint64_t>(BG_MAX_BANDS, room));
    return (uint32_t)std::max<uint64_t>(bands, 1u);
}

int launch_bilagrid_slice(bh_ctx* ctx, const bh_bilagrid* tab, uint32_t view, const float* img, uint32_t h, uint32_t w, float* out) {
    const uint32_t pixels = h * w;
    hipLaunchKernelGGL(bilagrid_slice_kernel, dim3(pixel_grid(pixels)), dim3(BG_WG), 0, ctx->stream,
                       reinterpret_cast<const float4*>(tab->param + (size_t)(view - 1) * tab->row), reinterpret_cast<const float4*>(img),
                       reinterpret_cast<float4*>(out), geom_of(tab, h, w), pixels);
    BH_LAUNCH_CHECK(ctx, "bilagrid_slice_kernel");
    return 0;
}

int launch_bilagrid_tv(bh_ctx* ctx, const bh_bilagrid* tab, uint32_t view, float* value, float weight, float* accum, float* accum_host) {
    hipLaunchKernelGGL(bilagrid_tv_kernel, dim3(1), dim3(BG_WG), 0, ctx->stream, tab->param + (size_t)(view - 1) * tab->row, geom_of(tab, 1, 1),
                       (uint32_t)tab->row, tv_of(tab), value, weight, accum, accum_host);
    BH_LAUNCH_CHECK(ctx, "bilagrid_tv_kernel");
    return 0;
}

// the scratch slot: 16 bytes (the train step's TV scalar) | the f64 sums [row] | the partial rows [units, L, 48]
float* bilagrid_tv_scratch(bh_ctx* ctx) { return (float*)ensure(ctx, SLOT_BILAGRID, BG_SCRATCH_HEAD); }

int launch_bilagrid_backward(bh_ctx* ctx, bh_bilagrid* tab, uint32_t view, const float* img, const float* v_sliced, uint32_t h, uint32_t w, float* v_img,
                             float tv_weight, bool update) {
    const uint32_t pixels = h * w, row = (uint32_t)tab->row;
    const uint32_t ncx = tab->gw > 1u ? tab->gw - 1u : 1u, ncy = tab->gh > 1u ? tab->gh - 1u : 1u;
    const uint32_t bands = bilagrid_bands(h, w, tab->gh, tab->gw, tab->gl);
    const uint32_t units = ncx * ncy * bands;
    auto* scratch = (char*)ensure(ctx, SLOT_BILAGRID, BG_SCRATCH_HEAD + (size_t)row * 8 + (size_t)units * tab->gl * 48 * 8);
    if (!scratch) return BH_ERR_OOM;
    auto* gsum = reinterpret_cast<double*>(scratch + BG_SCRATCH_HEAD);
    double* partials = gsum + row;
    const BgGeom g = geom_of(tab, h, w);
    const size_t off = (size_t)(view - 1) * tab->row;
    hipLaunchKernelGGL(bilagrid_vg_kernel, dim3(units), dim3(BG_WG), 0, ctx->stream, reinterpret_cast<const float4*>(img),
                       reinterpret_cast<const float4*>(v_sliced), g, ncx, ncy, bands, partials);
    BH_LAUNCH_CHECK(ctx, "bilagrid_vg_kernel");
    hipLaunchKernelGGL(bilagrid_pixel_kernel, dim3(pixel_grid(pixels)), dim3(BG_WG), 0, ctx->stream, reinterpret_cast<const float4*>(tab->param + off),
                       reinterpret_cast<const float4*>(img), reinterpret_cast<const float4*>(v_sliced), reinterpret_cast<float4*>(v_img), g, pixels);
    BH_LAUNCH_CHECK(ctx, "bilagrid_pixel_kernel");
    const uint32_t blocks = (row + BG_WG - 1) / BG_WG;
    hipLaunchKernelGGL(bilagrid_final_kernel, dim3(blocks), dim3(BG_WG), 0, ctx->stream, partials, tab->param + off, tab->grad + off, gsum,
                       tab->t + (view - 1), g, ncx, ncy, bands, row, (double)tv_weight, tv_of(tab), update ? 1 : 0);
    BH_LAUNCH_CHECK(ctx, "bilagrid_final_kernel");
    if (update) {
        hipLaunchKernelGGL(bilagrid_step_kernel, dim3(blocks), dim3(BG_WG), 0, ctx->stream, gsum, tab->param + off, static_cast<float*>(tab->m1) + off,
                           static_cast<float*>(tab->m2) + off, tab->t + (view - 1), row, tab->lr, tab->beta1, tab->beta2, tab->eps);
        BH_LAUNCH_CHECK(ctx, "bilagrid_step_kernel");
    }
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_bilagrid_create(bh_ctx* ctx, uint32_t n_views, uint32_t grid_w, uint32_t grid_h, uint32_t grid_l, bh_bilagrid** table) {
    BH_TRY(param_table_create_args(ctx, table, n_views, "bilagrid_create"));
    if (grid_w == 0 || grid_h == 0 || grid_l == 0 || grid_w > 1024u || grid_h > 1024u || grid_l > 1024u ||
        (uint64_t)grid_w * grid_h * grid_l * 12u > (1ull << 22))
        return set_error(ctx, BH_ERR_INVALID_ARG, "bilagrid_create: grid sides must be 1 .. 1024 and a view at most 2^22 floats");
    bh_bilagrid* tab = new bh_bilagrid;
    BH_TRY(param_table_create(ctx, tab, n_views, (size_t)grid_w * grid_h * grid_l * 12, 0, &COLOUR_IDENTITY, "bilagrid_create"));
    tab->gw = grid_w; tab->gh = grid_h; tab->gl = grid_l;
    *table = tab;
    return 0;
}

int bh_bilagrid_destroy(bh_ctx* ctx, bh_bilagrid* table) { return param_table_destroy(ctx, PT_BILAGRID, table, "bilagrid_destroy"); }

int bh_bilagrid_dims(bh_ctx* ctx, bh_bilagrid* table, uint32_t* n_views, uint32_t* grid_w, uint32_t* grid_h, uint32_t* grid_l) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(check_rows(ctx, PT_BILAGRID, table, 1, 1, "bilagrid_dims"));
    if (n_views) *n_views = table->n_views;
    if (grid_w) *grid_w = table->gw;
    if (grid_h) *grid_h = table->gh;
    if (grid_l) *grid_l = table->gl;
    return 0;
}

int bh_bilagrid_set_params(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, const float* host) {
    return param_table_set_params(ctx, PT_BILAGRID, table, first_view, count, host, "bilagrid_set_params");
}

int bh_bilagrid_get_params(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, float* host) {
    return param_table_get_rows(ctx, PT_BILAGRID, table, &ParamTable::param, first_view, count, host, "bilagrid_get_params");
}

int bh_bilagrid_get_grad(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, float* host) {
    return param_table_get_rows(ctx, PT_BILAGRID, table, &ParamTable::grad, first_view, count, host, "bilagrid_get_grad");
}

int bh_bilagrid_get_state(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, float* m1, float* m2, uint32_t* t) {
    return param_table_get_state(ctx, PT_BILAGRID, table, view, m1, m2, t, "bilagrid_get_state");
}

int bh_bilagrid_set_state(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* m1, const float* m2, uint32_t t) {
    return param_table_set_state(ctx, PT_BILAGRID, table, view, m1, m2, t, "bilagrid_set_state");
}

int bh_bilagrid_set_adam(bh_ctx* ctx, bh_bilagrid* table, double lr, double beta1, double beta2, double eps) {
    return param_table_set_adam(ctx, PT_BILAGRID, table, lr, beta1, beta2, eps, "bilagrid_set_adam");
}

int bh_bilagrid_slice(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !out_hwc4) return set_error(ctx, BH_ERR_INVALID_ARG, "bilagrid_slice: null argument");
    BH_TRY(check_image(ctx, h, w, /*below_2_31=*/true, "bilagrid_slice"));
    BH_TRY(check_rows(ctx, PT_BILAGRID, table, view, 1, "bilagrid_slice"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_bilagrid_slice(ctx, table, view, img_hwc4, h, w, out_hwc4);
}

int bh_bilagrid_backward(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* img_hwc4, const float* v_sliced, uint32_t h, uint32_t w,
                         float* v_img, float tv_weight, int update) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !v_sliced || !v_img) return set_error(ctx, BH_ERR_INVALID_ARG, "bilagrid_backward: null argument");
    BH_TRY(check_image(ctx, h, w, /*below_2_31=*/true, "bilagrid_backward"));
    if (!(tv_weight >= 0.0f) || !std::isfinite(tv_weight)) return set_error(ctx, BH_ERR_INVALID_ARG, "bilagrid_backward: tv_weight must be finite and >= 0");
    BH_TRY(check_rows(ctx, PT_BILAGRID, table, view, 1, "bilagrid_backward"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_bilagrid_backward(ctx, table, view, img_hwc4, v_sliced, h, w, v_img, tv_weight, update != 0);
}

int bh_bilagrid_tv(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, float* value_dev) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!value_dev) return set_error(ctx, BH_ERR_INVALID_ARG, "bilagrid_tv: null argument");
    BH_TRY(check_rows(ctx, PT_BILAGRID, table, view, 1, "bilagrid_tv"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_bilagrid_tv(ctx, table, view, value_dev, 0.0f, nullptr, nullptr);
}

int bh_train_set_bilagrid(bh_ctx* ctx, bh_bilagrid* table, float tv_weight) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(param_table_attachable(ctx, PT_BILAGRID, table, "train_set_bilagrid"));
    if (table && (!(tv_weight >= 0.0f) || !std::isfinite(tv_weight)))
        return set_error(ctx, BH_ERR_INVALID_ARG, "train_set_bilagrid: tv_weight must be finite and >= 0");
    ctx->terms.bilagrid = table;
    ctx->terms.bilagrid_tv_weight = table ? tv_weight : 0.0f;
    return 0;
}

}  // extern "C"
