// Microbenchmark (dev tool): how many waves per SIMD / independent chains per wave does it take to saturate the gfx950
// VALU with DEPENDENT f32 ops?  One-wave workgroups, W waves per SIMD (grid = 1024 * W), C independent fma chains per lane.
// Prints cycles per wave-instruction per SIMD at the 2.4 GHz nominal clock.  Always run under `timeout`.
#include <hip/hip_runtime.h>
#include <cstdio>
template <int C>
__global__ __launch_bounds__(64) void chain(float* out, float a, float b, int iters) {
    float x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = threadIdx.x + c;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int c = 0; c < C; ++c) asm volatile("v_fma_f32 %0, %0, %1, %2\n" : "+v"(x[c]) : "v"(a), "v"(b));
        }
    }
    float s = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) s += x[c];
    out[blockIdx.x * 64 + threadIdx.x] = s;
}
// The same with a DPP add as the dependent op (K17's row reduction): a VALU write needs 2 wait states before a DPP op reads the
// register, which hand-written assembly pads itself (s_nop 1) and C independent chains hide behind each other.  KIND 0: plain
// v_add_f32 (no hazard); 1: row_ror:4, every bank; 2: row_ror:4 with a partial bank_mask (banks 1 and 3 written, the others keep
// the destination's value); 3: quad_perm.  PAD: an s_nop 1 in front of every op (what ONE chain needs; with C >= 3 the other
// chains already are the distance).
#define DPP_ROR4 " row_ror:4 row_mask:0xf bank_mask:0xf\n"
#define DPP_ROR4_BANK " row_ror:4 row_mask:0xf bank_mask:0xa\n"
#define DPP_QUAD " quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
template <int KIND, bool PAD, int C>
__global__ __launch_bounds__(64) void chain_dpp(float* out, float a, float b, int iters) {
    float x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = threadIdx.x + c;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (PAD) asm volatile("s_nop 1\n");
                if (KIND == 0) asm volatile("v_add_f32 %0, %0, %1\n" : "+v"(x[c]) : "v"(a));
                if (KIND == 1) asm volatile("v_add_f32_dpp %0, %0, %0" DPP_ROR4 : "+v"(x[c]));
                if (KIND == 2) asm volatile("v_add_f32_dpp %0, %0, %0" DPP_ROR4_BANK : "+v"(x[c]));
                if (KIND == 3) asm volatile("v_add_f32_dpp %0, %0, %0" DPP_QUAD : "+v"(x[c]));
            }
        }
    }
    float s = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) s += x[c];
    out[blockIdx.x * 64 + threadIdx.x] = s;
}
template <int KIND, bool PAD, int C>
static void run_dpp(float* d, int waves_per_simd) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 1024 * waves_per_simd, iters = 4000;
    hipLaunchKernelGGL((chain_dpp<KIND, PAD, C>), dim3(blocks), dim3(64), 0, 0, d, 0.999f, 0.001f, 10);
    hipEventRecord(e0);
    hipLaunchKernelGGL((chain_dpp<KIND, PAD, C>), dim3(blocks), dim3(64), 0, 0, d, 0.999f, 0.001f, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    const double winst = (double)blocks * iters * 16 * C;
    const double per_simd_per_s = winst / (ms * 1e-3) / 1024.0;
    static const char* names[] = {"add", "add_dpp ror4", "add_dpp ror4 bank 0xa", "add_dpp quad_perm"};
    printf("%-22s %s waves/SIMD %d chains %d: %.2f cycles/op/SIMD @2.4GHz   (per wave: one op every %.2f cycles)\n", names[KIND], PAD ? "s_nop 1 +" : "         ",
           waves_per_simd, C, 2.4e9 / per_simd_per_s, 2.4e9 / per_simd_per_s * waves_per_simd);
}
template <int C>
static void run(float* d, int waves_per_simd) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 1024 * waves_per_simd, iters = 4000;
    hipLaunchKernelGGL(chain<C>, dim3(blocks), dim3(64), 0, 0, d, 0.999f, 0.001f, 10);
    hipEventRecord(e0);
    hipLaunchKernelGGL(chain<C>, dim3(blocks), dim3(64), 0, 0, d, 0.999f, 0.001f, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    const double winst = (double)blocks * iters * 16 * C;
    const double per_simd_per_s = winst / (ms * 1e-3) / 1024.0;
    printf("waves/SIMD %d chains %d: %.2f cycles/inst/SIMD @2.4GHz   (per wave: one inst every %.2f cycles)\n", waves_per_simd, C, 2.4e9 / per_simd_per_s,
           2.4e9 / per_simd_per_s * waves_per_simd);
}
int main() {
    float* d; (void)hipMalloc(&d, 1024 * 8 * 64 * 4);
    for (int w : {1, 2, 3, 4, 6, 8}) { run<1>(d, w); run<2>(d, w); run<4>(d, w); }
    for (int w : {1, 5}) {   // (5: what K17's default variant runs at)
        run_dpp<0, false, 1>(d, w); run_dpp<1, true, 1>(d, w); run_dpp<2, true, 1>(d, w); run_dpp<3, true, 1>(d, w);
        run_dpp<1, false, 3>(d, w); run_dpp<2, false, 3>(d, w); run_dpp<3, false, 3>(d, w);
    }
    return 0;
}
