// On which SIMD of a gfx950 CU does wave w of a 1024-thread workgroup run?  k_sweep's wave -> (point-group, lag-wave)
// mapping relies on the answer: a batch whose last lag-wave is padding only frees issue slots on EVERY SIMD when the
// four lag-waves of one point-group share a SIMD.  One workgroup of 1024 threads per CU with k_sweep's dynamic LDS size
// (159 KiB: one workgroup per CU); lane 0 of every wave records its wave index (threadIdx.x / 64) and the hardware-id
// register (gfx9 layout: WAVE_ID 3:0, SIMD_ID 5:4, PIPE_ID 7:6, CU_ID 11:8, SH_ID 12, SE_ID 15:13).  Prints, over all
// workgroups of several launches, how often wave w sat on SIMD s, whether SIMD = w mod 4 (or w / 4) held, and -- what the
// mapping needs -- whether waves w, w + 4, w + 8, w + 12 shared a SIMD and the four classes sat on four different ones.
// hipcc -O3 --offload-arch=gfx950 wave_simd.hip -o wave_simd && ./wave_simd
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr size_t kLdsBytes = 159 * 1024;

__global__ void __launch_bounds__(kThreads) k(unsigned* out, int spin) {
    extern __shared__ double lds[];
    // (touch the LDS and keep all 16 waves resident together for a moment, as a tile visit of k_sweep does)
    for (int i = threadIdx.x; i < 2048; i += kThreads) lds[i] = (double)i;
    __syncthreads();
    double s = lds[threadIdx.x];
    for (int i = 0; i < spin; ++i) s = fma(s, 1.0000001, 1e-9);
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));  // hwreg(HW_REG_HW_ID, 0, 32)
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) out[(size_t)blockIdx.x * kWaves + wave] = s == 12345.0 ? 0u : hw;
}

int main() {
    const int blocks = 256, launches = 8;
    unsigned* d;
    if (hipMalloc(&d, sizeof(unsigned) * blocks * kWaves) != hipSuccess) return 1;
    if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes) != hipSuccess) return 1;
    std::vector<unsigned> h((size_t)blocks * kWaves);
    long long count[kWaves][4] = {};
    long long n_wg = 0, n_mod4 = 0, n_div4 = 0, n_class = 0;
    for (int l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(k, dim3(blocks), dim3(kThreads), kLdsBytes, 0, d, l % 2 ? 20000 : 200);
        if (hipMemcpy(h.data(), d, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (int b = 0; b < blocks; ++b) {
            bool mod4 = true, div4 = true, cls = true;
            unsigned seen = 0;
            for (int w = 0; w < kWaves; ++w) {
                const int simd = (h[(size_t)b * kWaves + w] >> 4) & 3;
                count[w][simd]++;
                mod4 &= simd == (w & 3);
                div4 &= simd == (w >> 2);
                cls &= simd == (int)((h[(size_t)b * kWaves + (w & 3)] >> 4) & 3);
                if (w < 4) seen |= 1u << simd;
            }
            ++n_wg;
            n_mod4 += mod4;
            n_div4 += div4;
            n_class += cls && seen == 15u;
            if (l == 0 && b < 4) {
                printf("launch 0 workgroup %d: cu %u se %u | wave:simd(slot)", b, (h[(size_t)b * kWaves] >> 8) & 15,
                       (h[(size_t)b * kWaves] >> 13) & 7);
                for (int w = 0; w < kWaves; ++w)
                    printf(" %d:%u(%u)", w, (h[(size_t)b * kWaves + w] >> 4) & 3, h[(size_t)b * kWaves + w] & 15);
                printf("\n");
            }
        }
    }
    printf("wave  SIMD0  SIMD1  SIMD2  SIMD3   (%lld workgroups of %d waves, %d launches of %d)\n", n_wg, kWaves, launches, blocks);
    for (int w = 0; w < kWaves; ++w)
        printf("%4d %6lld %6lld %6lld %6lld\n", w, count[w][0], count[w][1], count[w][2], count[w][3]);
    printf("workgroups with SIMD = wave mod 4 for all 16 waves: %lld; with SIMD = wave / 4: %lld\n", n_mod4, n_div4);
    printf("workgroups whose waves w, w+4, w+8, w+12 share a SIMD, the four classes on four SIMDs: %lld of %lld\n", n_class, n_wg);
    (void)hipFree(d);
    return 0;
}
