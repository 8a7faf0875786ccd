// Exhaustive GPU check of two FMA-corrected f32 divisions against the correctly rounded a / b
// (-fhip-fp32-correctly-rounded-divide-sqrt), for the mask quotient hp / (hp + rp + eps)
// (k_mask.hip) and the per-frame X / max quotient (k_features.hip):
//   D1 (general):   y = rcp(b); y1 = y + y (1 - b y); q0 = a y1; q = q0 + (a - b q0) y1
//   D2 (fixed b):   yr = 1 / b correctly rounded once per divisor; q = q0 + (a - b q0) yr, q0 = a yr
// Every step is a scaled-exact operation (FMA, products, the hardware reciprocal), so for normal
// operands whose intermediates stay normal the result depends only on the mantissas: the check runs
// every pair of mantissas (2^46 pairs, a and b in [1, 2)), and separately that v_rcp_f32 is
// scale-invariant (rcp(b 2^k) = rcp(b) 2^-k for every mantissa and every k that keeps b and 1/b
// normal).  The kernels apply the fast forms only where that holds (see their range guards).
//   hipcc --offload-arch=gfx950 -O3 -fhip-fp32-correctly-rounded-divide-sqrt -ffp-contract=off
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

__device__ __forceinline__ float div_d1(float a, float b) {
    const float y = __builtin_amdgcn_rcpf(b);
    const float y1 = __builtin_fmaf(__builtin_fmaf(-b, y, 1.0f), y, y);
    const float q0 = a * y1;
    return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y1, q0);
}
__device__ __forceinline__ float div_d2(float a, float b, float yr) {
    const float q0 = a * yr;
    return __builtin_fmaf(__builtin_fmaf(-b, q0, a), yr, q0);
}

__global__ void k_pairs(uint32_t a0, uint32_t na, unsigned long long* bad, uint32_t* ex) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // b mantissa index
    if (t >= (1u << 23)) return;
    const float b = __uint_as_float(0x3F800000u | t);
    const float yr = 1.0f / b;
    unsigned long long n1 = 0, n2 = 0;
    for (uint32_t i = 0; i < na; i++) {
        const float a = __uint_as_float(0x3F800000u | (a0 + i));
        const uint32_t ref = __float_as_uint(a / b);
        const uint32_t r1 = __float_as_uint(div_d1(a, b)), r2 = __float_as_uint(div_d2(a, b, yr));
        if (r1 != ref) {
            n1++;
            ex[0] = __float_as_uint(a);
            ex[1] = __float_as_uint(b);
        }
        if (r2 != ref) {
            n2++;
            ex[2] = __float_as_uint(a);
            ex[3] = __float_as_uint(b);
        }
    }
    if (n1) atomicAdd(&bad[0], n1);
    if (n2) atomicAdd(&bad[1], n2);
}

__global__ void k_rcp_scale(unsigned long long* bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << 23)) return;
    const float b = __uint_as_float(0x3F800000u | t);
    const uint32_t r0 = __float_as_uint(__builtin_amdgcn_rcpf(b));
    for (int k = -125; k <= 125; k++) {  // b 2^k and 1/(b 2^k) normal
        const float bk = __uint_as_float((uint32_t)((127 + k) << 23) | t);
        const uint32_t rk = __float_as_uint(__builtin_amdgcn_rcpf(bk));
        if (rk != r0 - (uint32_t)(k << 23)) atomicAdd(bad, 1ull);
    }
}

int main() {
    unsigned long long* bad;
    uint32_t* ex;
    (void)hipMalloc(&bad, 3 * 8);
    (void)hipMalloc(&ex, 4 * 4);
    (void)hipMemset(bad, 0, 3 * 8);
    (void)hipMemset(ex, 0, 4 * 4);
    const dim3 grid((1u << 23) / 256), block(256);
    hipLaunchKernelGGL(k_rcp_scale, grid, block, 0, 0, bad + 2);
    const uint32_t chunk = 1u << 13;
    for (uint32_t c = 0; c < (1u << 23) / chunk; c++) {
        hipLaunchKernelGGL(k_pairs, grid, block, 0, 0, c * chunk, chunk, bad, ex);
        if (c % 64 == 63) {
            (void)hipDeviceSynchronize();
            unsigned long long hb[3];
            (void)hipMemcpy(hb, bad, sizeof hb, hipMemcpyDeviceToHost);
            printf("a-chunks %u/%u: D1 %llu, D2 %llu mismatches; rcp scale %llu\n", c + 1, (1u << 23) / chunk, hb[0],
                   hb[1], hb[2]);
            fflush(stdout);
        }
    }
    unsigned long long hb[3];
    uint32_t he[4];
    (void)hipMemcpy(hb, bad, sizeof hb, hipMemcpyDeviceToHost);
    (void)hipMemcpy(he, ex, sizeof he, hipMemcpyDeviceToHost);
    printf("D1 general:   %llu mismatches of 2^46 (e.g. a=0x%08x b=0x%08x)\n", hb[0], he[0], he[1]);
    printf("D2 fixed b:   %llu mismatches of 2^46 (e.g. a=0x%08x b=0x%08x)\n", hb[1], he[2], he[3]);
    printf("rcp scaling:  %llu mismatches\n", hb[2]);
    return 0;
}
