// ubench.hip -- gfx950 integer-issue microbenchmarks that size the VALU roofline of the Poseidon
// and NTT kernels (the MI355X guides give no integer-multiply rates).  Standalone program:
//   hipcc --offload-arch=gfx950 -O3 -I.. ubench.hip -o ubench && ./ubench
// `./ubench mds` runs only the last part: the full-round MDS layer and the whole permutation, VALU form against matrix-pipe form.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../glf.h"
#include "../poseidon.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int ITERS = 4096;

__global__ void k_mad64(u64 *out, u32 a, u32 b) {
    u64 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i;
    u32 x = a + threadIdx.x, y = b;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[i]) : "v"(x), "v"(y) : "vcc");
    }
    u64 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_mullo(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 y = b | 1;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(acc[i]) : "v"(y));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_mulhi(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 y = b | 0x80000001u;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(acc[i]) : "v"(y));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_add32(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_add_u32 %0, %0, %1" : "+v"(acc[i]) : "v"(b));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_lshladd64(u64 *out, u32 a, u32 b) {
    u64 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u64 y = b;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(acc[i]) : "v"(y));
    }
    u64 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_addc(u64 *out, u32 a, u32 b) {
    u32 lo[8], hi[8];
    for (int i = 0; i < 8; i++) { lo[i] = threadIdx.x + i + a; hi[i] = i; }
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            asm volatile("v_add_co_u32 %0, vcc, %0, %2\n\tv_addc_co_u32 %1, vcc, %1, %2, vcc" : "+v"(lo[i]), "+v"(hi[i]) : "v"(b) : "vcc");
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= lo[i] ^ hi[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_dot2(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 x = a * 0x10001u + threadIdx.x, y = b | 0x00110017u;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_dot2_u32_u16 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(x), "v"(y));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_dot4(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 x = a * 0x01010101u + threadIdx.x, y = b | 0x11170f29u;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_dot4_u32_u8 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(x), "v"(y));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_perm(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 y = b + threadIdx.x, sel = 0x07060100u;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(acc[i]) : "v"(y), "v"(sel));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_mad24(u64 *out, u32 a, u32 b) {
    u32 acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i + a;
    u32 x = a + threadIdx.x, y = b | 17u;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(x), "v"(y));
    }
    u32 s = 0; for (int i = 0; i < 8; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_mulmod(u64 *out, u64 a, u64 b) {
    u64 acc[4];
    for (int i = 0; i < 4; i++) acc[i] = glf::canon(a + threadIdx.x + i);
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = glf::mul(acc[i], b);
    }
    u64 s = 0; for (int i = 0; i < 4; i++) s ^= acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void k_poseidon(u64 *out, u64 a, int reps) {
    u64 s[12];
    for (int i = 0; i < 12; i++) s[i] = glf::canon(a + threadIdx.x * 12 + i);
    for (int r = 0; r < reps; r++) pos::permute(s);
    u64 x = 0; for (int i = 0; i < 12; i++) x ^= s[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}
// ---- full-round MDS layer: VALU form against the matrix-pipe form (pos::mds_add_wave) ------------------------------------
// lane maps of v_mfma_i32_32x32x32_i8 as poseidon.h states them, on exact integers: A[32][32], B[32][32] int8 row-major, D = A B
__global__ void k_mfma_map(const signed char *A, const signed char *B, int *D) {
#if defined(__HIP_DEVICE_COMPILE__)        // the vector types and builtins exist in the device pass only
    const int l = threadIdx.x, c = l & 31, h = l >> 5;
    pos::v4i32 a, b;
    for (int w = 0; w < 4; w++) {
        u32 av = 0, bv = 0;
        for (int j = 0; j < 4; j++) {
            av |= (u32)(unsigned char)A[c * 32 + 16 * h + 4 * w + j] << (8 * j);
            bv |= (u32)(unsigned char)B[(16 * h + 4 * w + j) * 32 + c] << (8 * j);
        }
        a[w] = (int)av; b[w] = (int)bv;
    }
    pos::v16i32 d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    d = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, d, 0, 0, 0);
    for (int reg = 0; reg < 16; reg++) D[((reg & 3) + 8 * (reg >> 2) + 4 * h) * 32 + c] = d[reg];
#endif
}
__device__ __forceinline__ void ub_state(u64 s[12], u64 a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = 0; i < 12; i++) {
        u64 x = (a + t * 12 + i) * 0x9E3779B97F4A7C15ull;      // all 64 bits in use
        const u32 sel = (u32)(t + i) % 37;                      // and the byte patterns at the edge of the signed range
        if (sel == 0) x = 0; else if (sel == 1) x = ~0ull; else if (sel == 2) x = 0x8080808080808080ull; else if (sel == 3) x = 0x7f7f7f7f7f7f7f7full;
        s[i] = x;
    }
}
// full != null: every lane's whole state goes out (bit-for-bit comparison of the two forms); else one word per lane
template <bool WAVE> __global__ __launch_bounds__(256, 4) void k_mds_layer(u64 *out, u64 *full, u64 a, int reps) {
#if defined(__HIP_DEVICE_COMPILE__)
    const pos::MdsOperands mo = pos::mds_operands();
    u64 s[12];
    ub_state(s, a);
#pragma nounroll
    for (int r = 0; r < reps; r++) {
        if constexpr (WAVE) pos::mds_add_wave(s, pos::RCN.k[r & 7], mo); else pos::mds_add_nc(s, pos::RCN.k[r & 7]);
    }
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (full) for (int i = 0; i < 12; i++) full[12 * t + i] = s[i];
    u64 x = 0; for (int i = 0; i < 12; i++) x ^= s[i];
    out[t] = x;
#endif
}
template <bool WAVE> __global__ __launch_bounds__(256, 4) void k_poseidon_form(u64 *out, u64 *full, u64 a, int reps) {
    const pos::MdsOperands mo = pos::mds_operands();
    u64 s[12];
    ub_state(s, a);
    for (int i = 0; i < 12; i++) s[i] = glf::canon(s[i]);
#pragma nounroll
    for (int r = 0; r < reps; r++) {
        if constexpr (WAVE) pos::permute_wave(s, mo); else pos::permute(s);
    }
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (full) for (int i = 0; i < 12; i++) full[12 * t + i] = s[i];
    u64 x = 0; for (int i = 0; i < 12; i++) x ^= s[i];
    out[t] = x;
}

template <class F> static float time_ms(F launch) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    launch(); hipDeviceSynchronize();
    hipEventRecord(a); launch(); hipEventRecord(b); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    return ms;
}

// lane maps, then both forms of the layer and of the permutation: outputs compared bit for bit, timed alternately
static int mds_forms(int blocks, int threads, u64 *out, double lanes, double clk, int cus) {
    {
        std::vector<signed char> A(1024), B(1024);
        for (int i = 0; i < 32; i++) for (int k = 0; k < 32; k++) {           // asymmetric, the whole signed range
            A[i * 32 + k] = (signed char)((i * 37 + k * 11 + (i > k ? 5 : 0)) & 0xff);
            B[i * 32 + k] = (signed char)((i * 13 + k * 29 + (i < k ? 3 : 0) + 128) & 0xff);
        }
        signed char *dA, *dB; int *dD;
        CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dB, 1024)); CK(hipMalloc(&dD, 4096));
        CK(hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), 1024, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mfma_map, dim3(1), dim3(64), 0, 0, dA, dB, dD);
        std::vector<int> D(1024);
        CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < 32; i++) for (int j = 0; j < 32; j++) {
            int want = 0;
            for (int k = 0; k < 32; k++) want += (int)A[i * 32 + k] * (int)B[k * 32 + j];
            bad += want != D[i * 32 + j];
        }
        printf("v_mfma_i32_32x32x32_i8 lane maps (A, B, D): %d of 1024 entries differ from the host product\n", bad);
        hipFree(dA); hipFree(dB); hipFree(dD);
        if (bad) return 1;
    }
    const size_t words = (size_t)lanes * 12;
    u64 *f0, *f1; CK(hipMalloc(&f0, words * 8)); CK(hipMalloc(&f1, words * 8));
    std::vector<u64> h0(words), h1(words);
    auto same = [&](const char *what) {
        if (hipMemcpy(h0.data(), f0, words * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h1.data(), f1, words * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
        size_t bad = 0;
        for (size_t i = 0; i < words; i++) bad += h0[i] != h1[i];
        printf("%s: %zu of %zu output words differ between the forms\n", what, bad, words);
        return bad == 0;
    };
    hipLaunchKernelGGL(k_mds_layer<false>, dim3(blocks), dim3(threads), 0, 0, out, f0, (u64)7, 1);
    hipLaunchKernelGGL(k_mds_layer<true>, dim3(blocks), dim3(threads), 0, 0, out, f1, (u64)7, 1);
    if (!same("one MDS layer")) return 1;
    hipLaunchKernelGGL(k_mds_layer<false>, dim3(blocks), dim3(threads), 0, 0, out, f0, (u64)7, 9);
    hipLaunchKernelGGL(k_mds_layer<true>, dim3(blocks), dim3(threads), 0, 0, out, f1, (u64)7, 9);
    if (!same("nine MDS layers")) return 1;
    hipLaunchKernelGGL(k_poseidon_form<false>, dim3(blocks), dim3(threads), 0, 0, out, f0, (u64)7, 2);
    hipLaunchKernelGGL(k_poseidon_form<true>, dim3(blocks), dim3(threads), 0, 0, out, f1, (u64)7, 2);
    if (!same("two permutations")) return 1;
    hipFree(f0); hipFree(f1);
    const int lreps = 2048, preps = 64;
    for (int round = 0; round < 5; round++) {
        float a = time_ms([&] { hipLaunchKernelGGL(k_mds_layer<false>, dim3(blocks), dim3(threads), 0, 0, out, (u64 *)nullptr, (u64)99, lreps); });
        float b = time_ms([&] { hipLaunchKernelGGL(k_mds_layer<true>, dim3(blocks), dim3(threads), 0, 0, out, (u64 *)nullptr, (u64)99, lreps); });
        float c = time_ms([&] { hipLaunchKernelGGL(k_poseidon_form<false>, dim3(blocks), dim3(threads), 0, 0, out, (u64 *)nullptr, (u64)99, preps); });
        float d = time_ms([&] { hipLaunchKernelGGL(k_poseidon_form<true>, dim3(blocks), dim3(threads), 0, 0, out, (u64 *)nullptr, (u64)99, preps); });
        auto lc = [&](float ms, int reps) { return (ms * 1e-3) * clk * cus * 128.0 / (lanes * reps); };
        printf("round %d  MDS layer: valu %8.3f ms (%5.0f lane-clk)  matrix %8.3f ms (%5.0f lane-clk)   permutation: valu %8.3f ms (%6.0f lane-clk)  matrix %8.3f ms (%6.0f lane-clk)\n",
               round, a, lc(a, lreps), b, lc(b, lreps), c, lc(c, preps), d, lc(d, preps));
    }
    return 0;
}

int main(int argc, char **argv) {
    const bool only_mds = argc > 1 && !strcmp(argv[1], "mds");
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    int cus = prop.multiProcessorCount;
    double clk = prop.clockRate * 1e3;
    printf("device %s, %d CUs, clock %.0f MHz\n", prop.gcnArchName, cus, clk / 1e6);
    int blocks = cus * 8, threads = 256;
    u64 *out; CK(hipMalloc(&out, (size_t)blocks * threads * 8));
    double lanes = (double)blocks * threads;
    auto rep = [&](const char *name, float ms, double ops_per_lane) {
        double ops = lanes * ops_per_lane;
        double rate = ops / (ms * 1e-3);
        printf("%-22s %8.3f ms  %8.2f Gop/s  %6.2f lane-ops/clk/CU (peak 128 @ %.0f MHz)\n", name, ms, rate / 1e9, rate / cus / clk, clk / 1e6);
    };
    if (only_mds) { int rcode = mds_forms(blocks, threads, out, lanes, clk, cus); hipFree(out); return rcode; }
    rep("v_add_u32", time_ms([&] { hipLaunchKernelGGL(k_add32, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_mul_lo_u32", time_ms([&] { hipLaunchKernelGGL(k_mullo, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_mul_hi_u32", time_ms([&] { hipLaunchKernelGGL(k_mulhi, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_dot2_u32_u16", time_ms([&] { hipLaunchKernelGGL(k_dot2, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_dot4_u32_u8", time_ms([&] { hipLaunchKernelGGL(k_dot4, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_perm_b32", time_ms([&] { hipLaunchKernelGGL(k_perm, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_mad_u32_u24", time_ms([&] { hipLaunchKernelGGL(k_mad24, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_mad_u64_u32", time_ms([&] { hipLaunchKernelGGL(k_mad64, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_lshl_add_u64", time_ms([&] { hipLaunchKernelGGL(k_lshladd64, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("v_add_co+v_addc (pair)", time_ms([&] { hipLaunchKernelGGL(k_addc, dim3(blocks), dim3(threads), 0, 0, out, 1u, 3u); }), 8.0 * ITERS);
    rep("glf::mul (mulmod)", time_ms([&] { hipLaunchKernelGGL(k_mulmod, dim3(blocks), dim3(threads), 0, 0, out, (u64)12345, (u64)0xfedcba9876543210ull); }), 4.0 * ITERS);
    int reps = 64;
    float ms = time_ms([&] { hipLaunchKernelGGL(k_poseidon, dim3(blocks), dim3(threads), 0, 0, out, (u64)99, reps); });
    printf("%-22s %8.3f ms  %8.2f Mperm/s  (%.0f lane-clk per permutation per lane at 128 lanes/clk/CU)\n", "pos::permute", ms,
           lanes * reps / (ms * 1e-3) / 1e6, (ms * 1e-3) * clk * cus * 128.0 / (lanes * reps));
    int rcode = mds_forms(blocks, threads, out, lanes, clk, cus);
    hipFree(out);
    return rcode;
}
